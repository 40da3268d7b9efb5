"""Deterministic extractor inputs shared by test_extract_cases.py (CPU: each
input reaches the property it exists for, on the oracle alone),
test_oracle_kat.py (oracle vs pyref.extract) and test_gpu_extract_edges.py
(GPU vs oracle, byte for byte).  Everything is generated; no file is read.

synth.frame is one texture family: smooth value noise, shapes, +-3 noise.
These images are the ones it never produces: pixel values at 0 and 255, exact
ties in FAST scores and descriptor samples, symmetric patches (zero moments),
cells full of corners and frames without one, corners on the first and last
row and column of a FAST cell, and every cell shape the cell grid can make.

Cell coordinates come from the oracle's own cell loop (oracle.level_cells):
an interior [x0 + 3, x1 - 3) x [y0 + 3, y1 - 3) is what FAST evaluates."""
from __future__ import annotations

import functools

import numpy as np

from orb_slam_2_ros_amd import synth

W0, H0 = 152, 100          # levels 152x100, 127x83, 106x69 have cells; 88x58 has none
NLEVELS = 4
NFEATURES = 500
SCALE = 1.2

# (iniThFAST, minThFAST).  orbx_extractor_create does not range-check them; the
# oracle (cv::FAST clamps to [0, 255]) defines the behaviour.
THRESHOLDS = [(20, 7), (0, 0), (1, 0), (254, 1), (255, 255), (128, 127), (7, 20)]
GPU_THRESHOLDS = list(THRESHOLDS)   # (no pair had to be dropped: the oracle is well defined on all of them)

KFAST_LIST_CAP = 640       # kFastListCap, orbx_fast.hip


def _oracle():
    from oracle import oracle
    return oracle


# ---- plain images -------------------------------------------------------------
def uniform(w=W0, h=H0, seed=1):
    return np.random.default_rng(seed).integers(0, 256, (h, w)).astype(np.uint8)


def binary(w=W0, h=H0, seed=2):
    return (np.random.default_rng(seed).integers(0, 2, (h, w)) * 255).astype(np.uint8)


def checker(period, w=W0, h=H0):
    y, x = np.mgrid[0:h, 0:w]
    return ((((x // period) + (y // period)) & 1) * 255).astype(np.uint8)


def flat(v, w=W0, h=H0):
    return np.full((h, w), v, np.uint8)


def ramp(kind, w=W0, h=H0):
    y, x = np.mgrid[0:h, 0:w]
    if kind == "x":
        return (x * 255 // (w - 1)).astype(np.uint8)
    if kind == "y":
        return (y * 255 // (h - 1)).astype(np.uint8)
    return ((x + y) * 255 // (w + h - 2)).astype(np.uint8)


# ---- constructed corners --------------------------------------------------------
# An item is a handful of pixels on a locally flat background whose arc score S
# is known by construction: every one of a pixel's 16 ring pixels is background
# except at most one that belongs to the item, so some arc of 9 is all
# background and S = |value - background|.  No background pixel is a corner
# (at most 3 of its ring pixels belong to an item), and a background that
# varies along x only has none either: the ring pixels straight above and
# below equal the centre and every arc of 9 contains one of them.
def _item(kind, px):
    return {"kind": kind, "px": [(int(x), int(y), int(s)) for x, y, s in px]}


def _put(img, items, kind, pts):
    """pts: (x, y, value); S from the background the image has there now."""
    bg = [int(img[y, x]) for x, y, _ in pts]
    for x, y, v in pts:
        img[y, x] = v
    items.append(_item(kind, [(x, y, abs(v - b)) for (x, y, v), b in zip(pts, bg)]))


def _block(cx, cy, v, n=3):
    r = n // 2
    return [(cx + dx, cy + dy, v) for dy in range(-r, n - r) for dx in range(-r, n - r)]


def interiors(w, h):
    """FAST cell interiors (x0, y0, x1, y1) of a w x h level, from the oracle."""
    c = _oracle().level_cells(w, h)
    return [(int(a) + 3, int(b) + 3, int(cc) - 3, int(d) - 3) for a, b, cc, d in c]


def dots():
    """152 x 100: 1-px and 3 x 3 dots, 255 on 0 in the two left cell columns
    and 0 on 255 in the two right ones (a straight vertical edge between: no
    corner), on the first / last interior row and column of cells and within
    3 px of the line between neighbouring cells.  Returns (image, items)."""
    cells = interiors(W0, H0)
    xs = sorted({c[0] for c in cells}) + [max(c[2] for c in cells)]    # column lines
    ys = sorted({c[1] for c in cells}) + [max(c[3] for c in cells)]    # row lines
    assert len(xs) == 5 and len(ys) == 3, (xs, ys)
    img = np.zeros((H0, W0), np.uint8)
    img[:, xs[2]:] = 255
    items = []
    y0, ym, y1 = ys
    for half, (xb, xe) in enumerate([(xs[1], xs[0]), (xs[3], xs[4] - 1)]):
        v = 255 if half == 0 else 0
        # xb: the line between the half's two cell columns; xe: the image's
        # first (bright half) or last (dark half) interior column.  Items keep
        # 7 px apart, and the pairs' orientation discs (radius 15) hold nothing else.
        d1 = [
            (xe, y0), (xe, y0 + 17),                  # first row and first (last) column of the interior
            (xb - 19, y0), (xb - 8, y0),              # first row of a cell
            (xb - 1, y0 + 10),                        # last column of the left cell
            (xb, y0 + 16),                            # first column of the right cell
            (xb - 3, ym - 12), (xb + 2, ym - 5),      # within 3 px of the column line
            (xb - 11, ym - 1),                        # last row of the upper cell
            (xb - 4, ym),                             # first row of the lower cell
            (xb + 8, ym - 3), (xb + 16, ym + 2),      # within 3 px of the row line
            (xb - 6, y1 - 1),                         # last row of the interior
            (xb - 1, y1 - 1),                         # last row and last column of a cell
            # two on a row and two on a column, 5 px apart: one moment is 0, the other is not
            (xb + 14, y1 - 10), (xb + 19, y1 - 10),
            (xb - 20, ym + 12), (xb - 20, ym + 17),
        ]
        for x, y in d1:
            _put(img, items, "dot1", [(x, y, v)])
        # 3 x 3 dots: nine equal scores; one inside a cell, one across the column line
        _put(img, items, "dot3", _block(xb - 14, y0 + 9, v))
        _put(img, items, "dot3", _block(xb - 1, ym + 10, v))
    return img, items


def steps(ini, mn):
    """272 x 70, one row of eight cells.  Isolated 1-px corners whose ring
    differs from the centre by exactly th and by th + 1, th = ini in the four
    left cells and th = min in the four right ones; per th one cell each for
      A  centre 0,               ring th | th + 1          (brighter ring)
      B  centre 255 - th | - 1,  ring 255                  (v + th meets 255)
      C  centre 255,             ring 255 - th | - th - 1  (darker ring)
      D  centre th | th + 1,     ring 0                    (v - th meets 0)
    The ring value is the background of a full-height stripe (half a cell
    wide where the pair needs two), so nothing but the centres is a corner.
    A member whose value would leave [0, 255] is left out.  Returns (image, items)."""
    w, h = 272, 70
    cells = interiors(w, h)
    assert len(cells) == 8 and all(c[2] - c[0] == 30 for c in cells[:-1]), cells
    img = np.zeros((h, w), np.uint8)
    items = []
    ya, yb = cells[0][1] + 8, cells[0][1] + 24
    for g, th in enumerate((ini, mn)):
        th = min(max(int(th), 0), 255)
        plans = [
            ("A", [(0, th), (0, th + 1)]),
            ("B", [(255 - th, 255), (255 - th - 1, 255)]),
            ("C", [(255, 255 - th), (255, 255 - th - 1)]),
            ("D", [(th, 0), (th + 1, 0)]),
        ]
        for k, (name, pair) in enumerate(plans):
            x0 = cells[4 * g + k][0]
            x1 = x0 + 30
            lo = 0 if 4 * g + k == 0 else x0
            hi = w if 4 * g + k == 7 else x1
            spots = [(x0 + 7, ya), (x0 + 22, yb)]
            # stripes first (a value out of range: the other member's ring), then the centres
            ok = [0 <= v <= 255 and 0 <= r <= 255 for v, r in pair]
            rings = [r if o else None for (v, r), o in zip(pair, ok)]
            r0 = rings[0] if rings[0] is not None else rings[1]
            r1 = rings[1] if rings[1] is not None else rings[0]
            img[:, lo:x0 + 15] = r0
            img[:, x0 + 15:hi] = r1
            for (v, r), o, (x, y) in zip(pair, ok, spots):
                if o:
                    _put(img, items, f"step{name}{'ini' if g == 0 else 'min'}{'=' if abs(v - r) == th else '+'}",
                         [(x, y, v)])
    return img, items


def plateau():
    """152 x 100 on background 0: blocks of equal FAST score (strict NMS keeps
    none), unequal neighbours (one), and equal neighbours on either side of a
    cell line (both: a neighbour outside the cell counts 0).  Returns (image, items)."""
    cells = interiors(W0, H0)
    xs = sorted({c[0] for c in cells})
    ys = sorted({c[1] for c in cells})
    img = np.zeros((H0, W0), np.uint8)
    items = []
    x0, y0, xb, yb = xs[0], ys[0], xs[1], ys[1]
    _put(img, items, "eq3x3", _block(x0 + 8, y0 + 8, 255))
    _put(img, items, "eq2x2", _block(x0 + 18, y0 + 8, 255, 2))
    _put(img, items, "eq1x2", [(x0 + 8, y0 + 18, 200), (x0 + 9, y0 + 18, 200)])
    _put(img, items, "eq2x1", [(x0 + 18, y0 + 18, 255), (x0 + 18, y0 + 19, 255)])
    _put(img, items, "eqdiag", [(x0 + 8, y0 + 27, 90), (x0 + 9, y0 + 28, 90)])
    _put(img, items, "uneq1x2", [(xb + 8, y0 + 8, 255), (xb + 9, y0 + 8, 254)])
    _put(img, items, "peak3x3", _block(xb + 18, y0 + 8, 200)[:4] + [(xb + 18, y0 + 8, 255)] + _block(xb + 18, y0 + 8, 200)[5:])
    _put(img, items, "dip3x3", _block(xb + 8, y0 + 20, 255)[:4] + [(xb + 8, y0 + 20, 250)] + _block(xb + 8, y0 + 20, 255)[5:])
    # equal pairs across a column line, a row line, and the point where four cells meet
    _put(img, items, "eq_across_col", [(xb - 1, y0 + 27, 255), (xb, y0 + 27, 255)])
    _put(img, items, "eq_across_row", [(x0 + 25, yb - 1, 255), (x0 + 25, yb, 255)])
    _put(img, items, "eq2x2_across_both", _block(xs[2], yb, 255, 2))
    # The last cell filled to its candidate cap ceil(cw / 2) ceil(ch / 2): a corner
    # on every other pixel of every other row.  A lattice pixel's ring holds its
    # four diagonal lattice neighbours (ring points 2, 6, 10, 14) and twelve
    # background pixels, and every arc of 9 holds two or three of the four; with
    # values falling by LATTICE_STEP per lattice step away from the middle
    # (Chebyshev), the two neighbours further out are lower by the step, so
    # S = v - min over side-sharing neighbour pairs of the pair's maximum
    # >= LATTICE_STEP, and its 8 adjacent pixels are background (no corners).
    cx0, cy0, cx1, cy1 = cells[-1]
    nx, ny = (cx1 - cx0 + 1) // 2, (cy1 - cy0 + 1) // 2
    val = {(i, j): 255 - LATTICE_STEP * max(abs(i - nx // 2), abs(j - ny // 2)) for i in range(nx) for j in range(ny)}
    assert min(val.values()) > LATTICE_STEP
    px = []
    for (i, j), v in val.items():
        d = [val.get((i + a, j + b), 0) for a, b in ((1, 1), (1, -1), (-1, -1), (-1, 1))]   # ring order
        s = v - min(max(d[k], d[(k + 1) & 3]) for k in range(4))
        img[cy0 + 2 * j, cx0 + 2 * i] = v
        px.append((cx0 + 2 * i, cy0 + 2 * j, s))
    items.append(_item("lattice", px))
    return img, items


LATTICE_STEP = 21          # > 20: every lattice pixel is a corner at iniThFAST 20


def lattice_cell():
    """(index, candidate cap) of the plateau image's lattice cell."""
    cells = interiors(W0, H0)
    x0, y0, x1, y1 = cells[-1]
    return len(cells) - 1, ((x1 - x0 + 1) // 2) * ((y1 - y0 + 1) // 2)


def expected_level0(items, w, h, ini, mn):
    """The level-0 FAST candidates the items must give, from the definition:
    per cell, the item pixels inside the interior with S > iniThFAST and score
    S - 1 > every neighbour's score inside the same interior (strict 3 x 3; a
    score 0 never survives); if none, the same at minThFAST.  Sorted (y, x) per
    cell, cells in order, as (x, y, S - 1)."""
    ini, mn = min(max(ini, 0), 255), min(max(mn, 0), 255)
    S = {}
    for it in items:
        for x, y, s in it["px"]:
            S[(x, y)] = s
    out = []
    for (x0, y0, x1, y1) in interiors(w, h):
        inside = {p: s for p, s in S.items() if x0 <= p[0] < x1 and y0 <= p[1] < y1}
        for th in (ini, mn):
            sc = {p: s - 1 for p, s in inside.items() if s > th}
            keep = [(x, y, v) for (x, y), v in sc.items()
                    if all(v > sc.get((x + dx, y + dy), 0) for dy in (-1, 0, 1) for dx in (-1, 0, 1) if dx or dy)]
            if keep:
                break
        out += sorted(keep, key=lambda k: (k[1], k[0]))
    return out


# ---- the image set ---------------------------------------------------------------
IMAGE_NAMES = ["uniform", "binary", "binary91", "checker1", "checker2", "checker3", "checker4", "flat0", "flat128", "flat255",
               "ramp_x", "ramp_y", "ramp_xy", "dots", "steps", "plateau"]


@functools.lru_cache(maxsize=None)
def _image(name, ini, mn):
    if name == "uniform":
        r = uniform(), None
    elif name == "binary":
        r = binary(), None
    elif name == "binary91":
        r = binary(91, 91, 3), None
    elif name.startswith("checker"):
        r = checker(int(name[7:])), None
    elif name.startswith("flat"):
        r = flat(int(name[4:])), None
    elif name.startswith("ramp_"):
        r = ramp(name[5:]), None
    elif name == "dots":
        r = dots()
    elif name == "steps":
        r = steps(ini, mn)
    elif name == "plateau":
        r = plateau()
    else:
        raise KeyError(name)
    r[0].setflags(write=False)
    return r


def image(name, ini=20, mn=7):
    """The (read-only) image `name`; only `steps` depends on the thresholds."""
    return _image(name, *((ini, mn) if name == "steps" else (0, 0)))[0]


def items(name, ini=20, mn=7):
    return _image(name, *((ini, mn) if name == "steps" else (0, 0)))[1]


def nfeatures(name):
    """binary91 is the one 53 x 53 cell (the largest the grid makes) of a 91 x 91
    image: the only i.i.d. input with more than 640 compass passers in a cell at
    thresholds near 128, where it has about 30 corners; 50 features keep its
    level-0 quota (16) below that."""
    return 50 if name == "binary91" else NFEATURES


@functools.lru_cache(maxsize=None)
def oracle_extract(name, ini, mn):
    """The oracle's (keypoints, descriptors) of an image at a threshold pair, once per process."""
    return _oracle().extract(image(name, ini, mn), nfeatures(name), SCALE, NLEVELS, ini, mn)


MIXED_NAMES = ["flat128", "uniform", "synth", "flat0"]


def mixed(t=0):
    """The batch of consecutive streams (frame t of each): empty, full (the
    noise moves 2 px a frame, so consecutive frames match), ordinary, empty."""
    fr = [flat(128), np.roll(uniform(seed=1), 2 * t, axis=1), synth.frame(W0, H0, 77, t), flat(0)]
    return np.ascontiguousarray(np.stack(fr))


# ---- the compass pre-test, from its definition ------------------------------------
def compass_passers(img, th):
    """Per pixel (3 px inside the image): some cyclically adjacent pair of the four
    points at +-3 is all brighter than v + th or all darker than v - th."""
    a = img.astype(np.int32)
    v = a[3:-3, 3:-3]
    p = [a[6:, 3:-3], a[3:-3, 6:], a[:-6, 3:-3], a[3:-3, :-6]]     # below, right, above, left
    out = np.zeros(v.shape, bool)
    for k in range(4):
        q, r = p[k], p[(k + 1) & 3]
        out |= ((q > v + th) & (r > v + th)) | ((q < v - th) & (r < v - th))
    res = np.zeros(a.shape, bool)
    res[3:-3, 3:-3] = out
    return res


# ---- the cell-shape sweep ----------------------------------------------------------
SWEEP_FIXED = 70           # the other dimension: one row (column) of cells


@functools.lru_cache(maxsize=None)
def achievable_cell_sizes(lo=62, hi=4095):
    """{interior cell width: the smallest image width in [lo, hi] with such a cell}
    at one level (widths and heights follow the same rule)."""
    first = {}
    for w in range(lo, hi + 1):
        for (x0, _, x1, _) in interiors(w, SWEEP_FIXED):
            first.setdefault(x1 - x0, w)
    return first


def fast_list_cap(mw, mh):
    """fast_lds's survivor-list capacity for a launch whose largest cell is mw x mh."""
    need = max(((64 // ((((cw + 3) >> 2) + 1) >> 1)) + 1) * cw for cw in range(1, mw + 1))
    return min(mw * mh, max(KFAST_LIST_CAP, (need + 7) & ~7))


def fast_psc(mw):
    """k_fast's patch-stride instantiation for a launch whose widest cell is mw (fast_lds)."""
    ps = max((mw + 12) & ~3, 8 * ((mw + 7) // 8) + 8)
    return 48 if ps <= 48 else 64 if ps <= 64 else 0


def fast_staging(cw, ch, mw, mh):
    """'patch' (stage_fast_patch) or 'rows' (wave_stage_rows) for a cw x ch cell
    in a launch sized for mw x mh: k_fast's condition
    R && 8 R >= nr && (nr + R - 1) PS <= patch + score bytes."""
    ps = max((mw + 12) & ~3, 8 * ((mw + 7) // 8) + 8)
    ps = 48 if ps <= 48 else 64 if ps <= 64 else ps
    patch_bytes = (ps * (mh + 6) + 15) & ~15
    score_bytes = (ps * (mh + 2) + 15) & ~15
    nr, nd = ch + 6, (cw + 10) >> 2
    R = {1: 64, 2: 32, 3: 21, 4: 16, 5: 12, 6: 10, 7: 9, 8: 8, 9: 7, 10: 6, 11: 5, 12: 5}.get(nd, 0)
    return "patch" if R and 8 * R >= nr and (nr + R - 1) * ps <= patch_bytes + score_bytes else "rows"


@functools.lru_cache(maxsize=None)
def sweep_sizes():
    """A short list of image widths (at height 70; the same numbers serve as
    heights at width 70) whose cells cover every achievable interior size:
    the smallest and the largest single cell, both sides of the 48 / 64 stride
    boundary (widest cell 39 | 40), the coordinate limit 4095, then greedily the
    width that adds the most sizes not seen yet (ties: the smaller width).

    What each entry selects in k_fast (fast_psc / fast_staging, from the
    conditions in orbx_fast.hip; widths at height 70, cells n - 38 or as listed):
      62, 77                  one cell 24 | 39         stride 48, stage_fast_patch
      78, 79                  one cell 40 | 41         stride 64, stage_fast_patch
      80, 83..91              one cell 42, 45..53      stride 64, wave_stage_rows (13 dwords a row and up)
      95, 97, 100, 102, 104   25..30 beside 32..36     stride 48, stage_fast_patch
      118, 120                37 | 38 beside 43 | 44   stride 64, both paths in one launch
      123 + 30 k (k = 0..22)  31 beside 23 - k         stride 48, stage_fast_patch
      4095                    31 beside 27             stride 48, stage_fast_patch (x up to 4075: the 12-bit key field)
    As heights (at the narrowest width with a quadtree root, sweep_shape) the
    same cell heights: 62..80 stage_fast_patch, 83..91 and 118 | 120
    wave_stage_rows (more than 8 passes of rows), the rest stage_fast_patch;
    stride 48 throughout but 64 at 123 (78 px wide: one cell of 40)."""
    first = achievable_cell_sizes()
    want = set(first)
    seen = {}
    for w in range(62, 4096):
        seen[w] = {x1 - x0 for (x0, _, x1, _) in interiors(w, SWEEP_FIXED)}
    picked = [62, 77, 78, 91, 4095]
    assert max(seen[77]) == 39 and max(seen[78]) == 40
    got = set().union(*(seen[w] for w in picked))
    while got != want:
        best = max(range(62, 1200), key=lambda w: (len(seen[w] - got), -w))
        assert seen[best] - got
        picked.append(best)
        got |= seen[best]
    return tuple(sorted(picked))


def sweep_shape(axis, n):
    """(w, h) of sweep entry n: n x 70 for the widths; for the heights the
    narrowest width >= 70 whose quadtree still has a root,
    round((w - 32) / (h - 32)) >= 1 (the reference divides by zero below that,
    ORBextractor.cc:568, and orbx_extractor_reserve rejects such a size)."""
    if axis == "width":
        return n, SWEEP_FIXED
    return max(SWEEP_FIXED, 32 + (n - 32 + 1) // 2), n


def sweep_image(w, h, seed):
    """Dense corners of every strength along the swept dimension: uniform noise
    with a low-contrast and a binary stretch, in a band 70 px across (the whole
    image for the widths); flat 128 beside it."""
    bw, bh = (w, min(h, SWEEP_FIXED)) if w >= h else (min(w, SWEEP_FIXED), h)
    band = uniform(bw, bh, seed).copy()
    if bw >= bh:
        band[:, bw // 3: bw // 3 + max(bw // 6, 8)] //= 16
        band[:, 2 * bw // 3:] = binary(bw, bh, seed + 1)[:, 2 * bw // 3:]
    else:
        band[bh // 3: bh // 3 + max(bh // 6, 8), :] //= 16
        band[2 * bh // 3:, :] = binary(bw, bh, seed + 1)[2 * bh // 3:, :]
    img = np.full((h, w), 128, np.uint8)
    img[:bh, :bw] = band
    return img
