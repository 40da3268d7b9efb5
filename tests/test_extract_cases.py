"""Every input of extract_cases.py reaches, on the CPU oracle alone, the
property it exists for (test_gpu_extract_edges.py then holds the kernels to
the oracle on the same inputs).  An input that stops exercising its property
fails here instead of passing silently there.  The conditions are properties
of the inputs, not tolerances: each is computed from a definition (the
compass test, the arc score, the moments, the descriptor samples) with numpy
or pyref, independently of the oracle's FAST where a FAST result is expected."""
import numpy as np
import pytest

import extract_cases as ec
import pyref

PAIRS = ec.THRESHOLDS
LIVE = [p for p in PAIRS if p != (255, 255)]          # threshold 255: cv::FAST finds nothing at all


def _ids(pairs):
    return [f"{a}-{b}" for a, b in pairs]


def _cells_passers(oracle_mod, img, ini, mn):
    """Per level-0 cell: the compass passers of the passes the cell runs (iniThFAST
    always, minThFAST if that pass kept nothing) and its interior size."""
    h, w = img.shape
    c_ini, c_min = ec.compass_passers(img, min(ini, 255)), ec.compass_passers(img, min(mn, 255))
    out = []
    for (wx0, wy0, wx1, wy1), (x0, y0, x1, y1) in zip(oracle_mod.level_cells(w, h).tolist(), ec.interiors(w, h)):
        n = [int(c_ini[y0:y1, x0:x1].sum())]
        if len(oracle_mod.fast(img[wy0:wy1, wx0:wx1], ini)) == 0:
            n.append(int(c_min[y0:y1, x0:x1].sum()))
        out.append((max(n), (x1 - x0) * (y1 - y0)))
    return out


@pytest.mark.parametrize("name,ini,mn", [(n, a, b) for n in ("uniform", "binary91") for a, b in LIVE
                                         if (n, a, b) != ("uniform", 128, 127)])
def test_dense_cells_overflow_the_survivor_list(name, ini, mn, oracle_mod):
    """More compass survivors in a cell than k_fast's list holds (a flush in
    the middle of the cell), and more level-0 candidates than the quota.
    i.i.d. U{0..255} cannot do that at thresholds near 128: over three seeds the
    largest cell the grid makes (53 x 53) has 609-645 passers there, against
    1536 for i.i.d. {0, 255} (binary91), which therefore carries that pair."""
    img = ec.image(name)
    cells = _cells_passers(oracle_mod, img, ini, mn)
    best = max(n for n, _ in cells)
    k, _ = ec.oracle_extract(name, ini, mn)
    _, _, quota, _ = oracle_mod.levels(img.shape[1], img.shape[0], ec.nfeatures(name), ec.SCALE, ec.NLEVELS)
    n0 = len(oracle_mod.level_candidates(img, ini, mn))
    lw, lh, _, _ = oracle_mod.levels(img.shape[1], img.shape[0], ec.nfeatures(name), ec.SCALE, ec.NLEVELS)
    sizes = [(x1 - x0, y1 - y0) for w, h in zip(lw.tolist(), lh.tolist()) for (x0, y0, x1, y1) in ec.interiors(w, h)]
    cap = ec.fast_list_cap(max(c for c, _ in sizes), max(c for _, c in sizes))   # one launch for all levels
    print(f"{name} ({ini},{mn}): passers per cell {[n for n, _ in cells]} against a list of {cap}, "
          f"level-0 candidates {n0}, quota {quota[0]}")
    assert cap == ec.KFAST_LIST_CAP and best > cap
    assert n0 > quota[0] and int((k["octave"] == 0).sum()) == quota[0]


@pytest.mark.parametrize("ini,mn", PAIRS, ids=_ids(PAIRS))
def test_checker1_all_ties(ini, mn, oracle_mod):
    """Every pixel passes the compass test (its four points are the other colour)
    and none is a corner (the ring alternates); the resized levels have corners."""
    img = ec.image("checker1")
    k, _ = ec.oracle_extract("checker1", ini, mn)
    cnt = np.bincount(k["octave"], minlength=ec.NLEVELS)
    assert len(oracle_mod.level_candidates(img, ini, mn)) == 0 and cnt[0] == 0
    if (ini, mn) != (255, 255):
        assert all(n == area for n, area in _cells_passers(oracle_mod, img, ini, mn))
    if max(ini, mn) < 127:
        assert cnt[1] > 0 and cnt[2] > 0, cnt


@pytest.mark.parametrize("name", ["flat0", "flat128", "flat255", "ramp_x", "ramp_y", "ramp_xy"])
def test_flat_and_ramp_have_no_keypoint(name, oracle_mod):
    for ini, mn in PAIRS:
        k, d = ec.oracle_extract(name, ini, mn)
        assert len(k) == 0 and len(d) == 0


@pytest.mark.parametrize("ini,mn", LIVE, ids=_ids(LIVE))
def test_periodic_and_binary_images_have_keypoints(ini, mn):
    """checker2-4 and binary keep keypoints on some level at every live pair
    (checker2 only where both thresholds stay below the resized levels' contrast)."""
    for name in ("binary", "checker3", "checker4") + (("checker2",) if max(ini, mn) < 127 else ()):
        assert len(ec.oracle_extract(name, ini, mn)[0]) > 0, name


# ---- constructed corners ---------------------------------------------------------
CONSTRUCTED = ["dots", "steps", "plateau"]


def _level0(oracle_mod, name, ini, mn):
    img = ec.image(name, ini, mn)
    return img, [tuple(r) for r in oracle_mod.level_candidates(img, ini, mn).tolist()]


@pytest.mark.parametrize("name", CONSTRUCTED)
def test_constructed_scores_are_what_the_construction_says(name):
    """Every item pixel's arc score, by pyref's FAST arithmetic, is the S recorded for it."""
    for ini, mn in (PAIRS if name == "steps" else PAIRS[:1]):
        img = ec.image(name, ini, mn)
        for it in ec.items(name, ini, mn):
            for x, y, s in it["px"]:
                assert pyref.arc_score(img, x, y) == s, (it["kind"], x, y)


@pytest.mark.parametrize("ini,mn", PAIRS, ids=_ids(PAIRS))
@pytest.mark.parametrize("name", CONSTRUCTED)
def test_constructed_keep_drop_pattern(name, ini, mn, oracle_mod):
    """Level-0 FAST candidates: exactly the item pixels the definition keeps
    (S > th, strict 3 x 3 maximum inside the cell, minThFAST only for a cell
    iniThFAST left empty), nothing else, in cell order."""
    img, got = _level0(oracle_mod, name, ini, mn)
    assert got == ec.expected_level0(ec.items(name, ini, mn), img.shape[1], img.shape[0], ini, mn)


def _kept(items, got, kind):
    g = {(x, y) for x, y, _ in got}
    return [sum((x, y) in g for x, y, _ in it["px"]) for it in items if it["kind"] == kind]


def test_dots_pattern_explicit(oracle_mod):
    """At (20, 7): every 1-px dot is kept with score 254, bright or dark; of a
    3 x 3 dot's nine equal scores none is kept, also where a cell line cuts it;
    kept corners sit on the first and last row and column of cells."""
    img, got = _level0(oracle_mod, "dots", 20, 7)
    its = ec.items("dots")
    assert _kept(its, got, "dot1") == [1] * 36 and _kept(its, got, "dot3") == [0] * 4
    assert all(s == 254 for _, _, s in got) and len(got) == 36
    assert {int(img[y, x]) for x, y, _ in got} == {0, 255}
    cells = ec.interiors(*img.shape[::-1])
    edge = {"first row": 0, "last row": 0, "first column": 0, "last column": 0}
    for x, y, _ in got:
        (x0, y0, x1, y1), = [c for c in cells if c[0] <= x < c[2] and c[1] <= y < c[3]]
        edge["first row"] += y == y0
        edge["last row"] += y == y1 - 1
        edge["first column"] += x == x0
        edge["last column"] += x == x1 - 1
    assert all(v >= 2 for v in edge.values()), edge
    # all of them come out of the quadtree too
    k, _ = ec.oracle_extract("dots", 20, 7)
    assert sorted((int(x), int(y)) for x, y in zip(k["x"][k["octave"] == 0], k["y"][k["octave"] == 0])) == \
        sorted((x, y) for x, y, _ in got)


def test_plateau_pattern_explicit(oracle_mod):
    """At (20, 7): equal neighbours keep none, unequal ones the higher, equal
    ones on either side of a cell line both (a neighbour outside the cell's
    interior counts 0), and the lattice cell fills its candidate cap exactly."""
    img, got = _level0(oracle_mod, "plateau", 20, 7)
    its = ec.items("plateau")
    want = {"eq3x3": 0, "eq2x2": 0, "eq1x2": 0, "eq2x1": 0, "eqdiag": 0, "uneq1x2": 1, "peak3x3": 1, "dip3x3": 0,
            "eq_across_col": 2, "eq_across_row": 2, "eq2x2_across_both": 4}
    for kind, n in want.items():
        assert _kept(its, got, kind) == [n], kind
    ci, cap = ec.lattice_cell()
    for ini, mn in PAIRS:
        if max(min(ini, 255), 0) < ec.LATTICE_STEP or (ini >= 254 and mn < ec.LATTICE_STEP):
            _, cells = oracle_mod.level_candidates_cells(ec.image("plateau"), ini, mn)
            assert cells[ci] == cap == 168, (ini, mn, cells[ci])


@pytest.mark.parametrize("ini,mn", PAIRS, ids=_ids(PAIRS))
def test_steps_strict_threshold(ini, mn, oracle_mod):
    """A ring that differs by exactly th is no corner and one that differs by
    th + 1 is, for brighter and darker rings and centres at 0, th, 255 - th and
    255: at th = iniThFAST always, at th = minThFAST in cells iniThFAST leaves
    empty.  (S = 1 passes threshold 0 but scores S - 1 = 0, which the strict
    NMS never keeps: OpenCV's behaviour, and nothing is kept at (0, 0).)"""
    img, got = _level0(oracle_mod, "steps", ini, mn)
    its = ec.items("steps", ini, mn)
    g = {(x, y): s for x, y, s in got}
    for it in its:
        (x, y, s), = it["px"]
        kind = it["kind"]
        th = ini if "ini" in kind else mn
        assert s == (th if kind.endswith("=") else th + 1)
        # the th = minThFAST cells hold S = mn and mn + 1 only: empty at iniThFAST,
        # and so run at minThFAST, iff mn + 1 <= ini (otherwise test_constructed_keep_drop_pattern's
        # two-pass rule says what they keep)
        if "ini" in kind or mn + 1 <= ini:
            assert ((x, y) in g) == (kind.endswith("+") and s >= 2), kind
        if (x, y) in g:
            assert g[(x, y)] == s - 1
    groups = {it["kind"][4] for it in its if it["kind"].endswith("+") and it["px"][0][:2] in g}
    if ini < 255 and (ini, mn) != (0, 0):
        assert groups == set("ABCD"), groups
    if (ini, mn) == (20, 7):
        assert len(got) == 8 and sorted(s for _, _, s in got) == [7] * 4 + [20] * 4


# ---- orientation and descriptor ties -----------------------------------------------
def test_zero_moments_and_descriptor_ties(oracle_mod):
    """dots at (20, 7), level 0: keypoints with m01 == 0 only, m10 == 0 only and
    both (moments by pyref.ic_moments; the oracle's angle is fastAtan2 of them),
    and descriptors from patches where more than half of the 256 pairs tie."""
    img = ec.image("dots")
    k, d = ec.oracle_extract("dots", 20, 7)
    blur = oracle_mod.gauss7(img)
    pat = pyref.orb_pattern()
    seen = {"m01": 0, "m10": 0, "both": 0}
    ties = []
    for i in np.nonzero(k["octave"] == 0)[0]:
        x, y = int(k["x"][i]), int(k["y"][i])
        m01, m10 = pyref.ic_moments(img, x, y)
        assert k["angle"][i] == np.float32(oracle_mod.fast_atan2(float(m01), float(m10)))
        seen["both"] += m01 == 0 and m10 == 0
        seen["m01"] += m01 == 0 and m10 != 0
        seen["m10"] += m10 == 0 and m01 != 0
        s = pyref.orb_samples(blur, x, y, k["angle"][i], pat)
        ties.append(int((s[0::2] == s[1::2]).sum()))
        assert np.array_equal(d[i], pyref.orb_descriptor(blur, x, y, k["angle"][i], pat))
    print(f"zero moments {seen}; tied pairs per descriptor: max {max(ties)}, {sum(t > 128 for t in ties)} of {len(ties)} over 128")
    assert all(v >= 1 for v in seen.values()), seen
    assert max(ties) > 128
    # binary and checker levels: samples of few distinct values tie too
    for name in ("binary", "checker4"):
        kk, _ = ec.oracle_extract(name, 20, 7)
        assert len(kk) > 0


# ---- the cell-shape sweep --------------------------------------------------------------
def test_sweep_covers_every_cell_shape():
    """The sweep's widths (heights) produce every interior cell width (height) an
    image of 62..4095 px can, 1..53: a lone cell is its image minus 38, and with two
    or more columns wCell <= 45.  So fast_lds's runtime-stride instantiation
    (widest cell >= 56) cannot be selected, and the sweep stands on both sides of
    the one boundary that can (widest cell 39 | 40: stride 48 | 64) and takes both
    staging paths."""
    first = ec.achievable_cell_sizes()
    assert sorted(first) == list(range(1, 54))
    sizes = ec.sweep_sizes()
    seen = {"width": set(), "height": set()}
    psc, staging = set(), set()
    for axis in seen:
        for n in sizes:
            w, h = ec.sweep_shape(axis, n)
            cells = [(x1 - x0, y1 - y0) for (x0, y0, x1, y1) in ec.interiors(w, h)]
            mw, mh = max(c for c, _ in cells), max(c for _, c in cells)
            seen[axis] |= {c[axis == "height"] for c in cells}
            psc.add(ec.fast_psc(mw))
            staging |= {ec.fast_staging(cw, ch, mw, mh) for cw, ch in cells}
            if axis == "width":
                assert {ch for _, ch in cells} == {32}
            else:
                nini = pyref.round_half_away(np.float32(w - 32) / np.float32(h - 32))   # ORBextractor.cc:566
                assert nini >= 1 and (w == ec.SWEEP_FIXED or (w - 33) / (h - 32) < 0.5)
    print(f"sweep sizes {sizes}")
    assert seen["width"] == seen["height"] == set(first)
    assert psc == {48, 64} and staging == {"patch", "rows"}
    assert ec.fast_psc(39) == 48 and ec.fast_psc(40) == 64 and ec.fast_psc(55) == 64 and ec.fast_psc(56) == 0
    assert len(sizes) <= 48 and max(sizes) == 4095
