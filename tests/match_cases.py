"""Constructed inputs for the ORBmatcher searches: one named case per
comparison edge or kernel capacity (the matchers' counterpart of
extract_cases.py).

Nothing is drawn and hoped for.  Descriptors are a base descriptor with an
exact number of bits flipped, so every Hamming distance is known by
construction; positions and angles are the exact floats an edge needs.  A
projection case is a set of "islands": one query and its few keypoints, 50 px
from the next island and with a window of a few px, so each query's outcome is
known alone (`expect`: the keypoint it must end with, -1 for none).

test_match_cases.py shows on the CPU that each case reaches the edges it is
named for (CASE["edges"]) and that the oracle agrees with pyref;
test_gpu_match_edges.py holds the kernels to the oracle on the same inputs.

Reference lines are ORBmatcher.cc / Frame.cc of ORB-SLAM2.
"""
from __future__ import annotations

import numpy as np

from orb_slam_2_ros_amd import KEYPOINT_DTYPE
from orb_slam_2_ros_amd._lib import PROJ_QUERY_DTYPE
from orb_slam_2_ros_amd.synth import scale_tables

f32 = np.float32
W, H = 640, 480
BASE = np.random.default_rng(7).integers(0, 256, 32).astype(np.uint8)   # filler: any descriptor serves
# bounds of a distorted camera (tests/test_init_bounds.py)
BOUNDS_DISTORTED = (-13.37, 661.61, 7.25, 476.17)
TH_DEFAULT = {"localmap": 100, "lastframe": 100, "keyframe": 64, "sim3": 50, "fuse": 50, "fuse_sim3": 50}
PROJ_VARIANTS = list(TH_DEFAULT)
REPLAY_VARIANTS = ["localmap", "lastframe", "keyframe", "sim3"]   # Fuse has no greedy state


def flip(d, k, start=0):
    """d with k bits flipped from bit `start` on: Hamming distance k from d."""
    d = np.array(d, np.uint8, copy=True)
    for b in range(start, start + k):
        d[(b % 256) >> 3] ^= np.uint8(1 << (b & 7))
    return d


def below(v):
    return np.nextafter(f32(v), f32(-np.inf))


def above(v):
    return np.nextafter(f32(v), f32(np.inf))


class Scene:
    """Keypoints and queries of one projection case."""

    def __init__(self, bounds=(0.0, float(W), 0.0, float(H)), stereo=False):
        self.bounds, self.stereo = bounds, stereo
        self.k, self.d, self.ur, self.st = [], [], [], []
        self.q, self.qd, self.expect = [], [], []
        self.octave = 0        # default octave (7: sigma2 12.8, Fuse's chi-square gate passes up to 8 px)

    def kp(self, x, y, desc, octave=None, angle=0.0, ur=-1.0, state=0):
        octave = self.octave if octave is None else octave
        self.k.append((f32(x), f32(y), 31.0, f32(angle), 0.0, octave, -1))
        self.d.append(desc); self.ur.append(f32(ur)); self.st.append(state)
        return len(self.k) - 1

    def query(self, u, v, desc, r=8.0, min_level=0, max_level=-1, ur=0.0, ur_tol=0.0, angle=0.0, flags=3, expect=None):
        self.q.append((f32(u), f32(v), f32(r), f32(ur), f32(ur_tol), min_level, max_level, f32(angle), flags))
        self.qd.append(desc); self.expect.append(expect)
        return len(self.q) - 1

    def island(self, i):
        """Centre of island i (windows of <= 10 px never meet)."""
        return 35.0 + 50.0 * (i % 12), 35.0 + 50.0 * (i // 12)

    def build(self):
        sf, _ = scale_tables(1.2, 8)
        return dict(keys=np.array(self.k, KEYPOINT_DTYPE), desc=np.array(self.d, np.uint8).reshape(-1, 32),
                    queries=np.array(self.q, PROJ_QUERY_DTYPE), qdesc=np.array(self.qd, np.uint8).reshape(-1, 32),
                    bounds=tuple(float(f32(b)) for b in self.bounds),
                    uright=np.array(self.ur, np.float32) if self.stereo else None,
                    mp_state=np.array(self.st, np.uint8), inv_sigma2=(f32(1) / (sf * sf)).astype(np.float32),
                    expect=list(self.expect))


def _proj(name, variant, scene, edges, th_dist=None, nnratio=0.8, check_ori=False):
    return dict(family="proj", name=f"{name}-{variant}", variant=variant, edges=edges,
                th_dist=TH_DEFAULT[variant] if th_dist is None else th_dist, nnratio=nnratio, check_ori=check_ori,
                **scene.build())


# ---- E1: distance thresholds (ORBmatcher.cc:114, 386, 1417, 1551, 970, 1082: all '<=') ----------------
def proj_thresholds(variant, th_dist=None, bounds=None):
    th = TH_DEFAULT[variant] if th_dist is None else th_dist
    s = Scene(bounds or (0.0, float(W), 0.0, float(H)))
    for i, (dist, ok) in enumerate([(th - 1, True), (th, True), (th + 1, False), (256, False)]):
        x, y = s.island(i)
        k = s.kp(x + 1, y, flip(BASE, dist))
        s.query(x, y, BASE, expect=k if ok else -1)
    x, y = s.island(4)                       # 256 as the second best: never a second (bestDist2 stays 256)
    k = s.kp(x + 1, y, flip(BASE, th)); s.kp(x - 1, y, flip(BASE, 256))
    s.query(x, y, BASE, expect=k)
    tag = f"thresholds{th}" + ("-bounds" if bounds else "")
    return _proj(tag, variant, s, ["best==th", "best==th+1", "best==th-1", "best==256", "second==256"], th_dist=th)


# ---- E2: localmap's ratio test (ORBmatcher.cc:120): bestLevel == bestLevel2 && bestDist > ratio * bestDist2 ----
# (1.0: best == ratio * second needs a tie, so the pair is two keypoints at the same distance)
RATIO_PAIRS = {0.6: (18, 30), 0.75: (30, 40), 0.8: (40, 50), 0.9: (45, 50), 1.0: (37, 37)}


def proj_ratio(nnratio):
    b, b2 = RATIO_PAIRS[nnratio]
    s = Scene()
    r = f32(nnratio)
    n = 0
    for (d1, d2) in [(b, b2), (b + 1, b2), (b - 1, b2), (b, b2 + 1), (b, b2 - 1)] + ([(15, 25)] if nnratio == 0.6 else []):
        if d1 > d2:
            continue
        for oct2 in (0, 1):                  # second best on the same octave, then on another (no test)
            x, y = s.island(n); n += 1
            k = s.kp(x - 1, y, flip(BASE, d1)); s.kp(x + 1, y, flip(BASE, d2), octave=oct2)   # best first
            rejected = oct2 == 0 and f32(d1) > f32(r * f32(d2))
            s.query(x, y, BASE, expect=-1 if rejected else k)
    x, y = s.island(n)                        # one candidate: bestDist2 = 256, bestLevel2 = -1
    k = s.kp(x + 1, y, flip(BASE, 99))
    s.query(x, y, BASE, expect=k)
    edges = ["ratio==", "single-candidate"] + (["ratio-fail-other-octave"] if nnratio < 1.0 else [])
    return _proj(f"ratio{nnratio}", "localmap", s, edges, nnratio=nnratio)


# ---- E3: window (Frame.cc:395-396 / KeyFrame.cc:730-731: fabs(dx) < r) and cell range (:361-381) --------
def proj_window(variant):
    s = Scene()
    s.octave = 7
    near, far = flip(BASE, 0), flip(BASE, 10)
    i = 0
    for axis in (0, 1):
        for side, inside in [(8.0, False), (8.0, True), (-8.0, False), (-8.0, True)]:
            x, y = s.island(i); i += 1
            at = f32((x, y)[axis]) + f32(side)                        # at |d| == r, or the next float inside
            if inside:
                at = below(at) if side > 0 else above(at)
            ke = s.kp(at if axis == 0 else x, at if axis == 1 else y, near)
            kf = s.kp(x + 1, y + 1, far)
            s.query(x, y, BASE, expect=ke if inside else kf)
    x, y = s.island(i); i += 1               # radius 0: nothing is < 0 away
    s.kp(x, y, near)
    s.query(x, y, BASE, r=0.0, expect=-1)
    for (u, v, kx, ky) in [(2.0, 240.0, 1.0, 240.0), (638.0, 240.0, 634.0, 240.0),
                           (320.0, 2.0, 320.0, 1.0), (320.0, 478.0, 320.0, 474.0)]:   # range clamps at each side
        k = s.kp(kx, ky, near)
        s.query(u, v, BASE, expect=k)
    for (u, v) in [(-30.0, 100.0), (700.0, 100.0), (100.0, -30.0), (100.0, 520.0)]:      # empty range
        s.query(u, v, BASE, expect=-1)
    s.query(320.0, 240.0, flip(BASE, 3), r=330.0)                     # all 64 columns (takes what is left)
    return _proj("window", variant, s, ["|dx|==r", "|dy|==r", "next-inside", "radius0", "clamp-each-side",
                                        "empty-range", "all-columns"])


# ---- E4: grid membership (Frame::PosInGrid, Frame.cc:415-425: round, half away from zero) ---------------
def proj_grid(variant, bounds=None):
    s = Scene(bounds or (0.0, float(W), 0.0, float(H)))
    mnx, mxx, mny, mxy = [f32(b) for b in s.bounds]
    s.octave = 7
    near, far = flip(BASE, 0), flip(BASE, 10)
    cw, ch = f32(mxx - mnx) / f32(64), f32(mxy - mny) / f32(48)
    # (x - minX) * inv == -0.5: cell -1, outside (half-to-even would keep it in cell 0)
    s.kp(mnx - f32(0.5) * cw, mny + f32(100), near); kf = s.kp(mnx + 2, mny + f32(101), far)
    s.query(mnx + 1, mny + f32(100), BASE, expect=kf if bounds is None else None)
    s.kp(mnx + f32(200), mny - f32(0.5) * ch, near); kf = s.kp(mnx + f32(201), mny + 2, far)
    s.query(mnx + f32(200), mny + 1, BASE, expect=kf if bounds is None else None)
    # exactly k + .5 inside the frame: the cell, and with it the GetFeaturesInArea order of a tie
    ka = s.kp(mnx + f32(0.5) * cw, mny + f32(300), near)           # .5 -> column 1
    kb = s.kp(mnx + f32(0.4) * cw, mny + f32(300) + f32(0.6) * ch, near)   # column 0, a later row and index
    s.query(mnx + f32(0.45) * cw, mny + f32(300), BASE, r=1.5 * float(ch), expect=kb if bounds is None else None)
    ka2 = s.kp(mnx + f32(400), mny + f32(10.5) * ch, near)         # .5 -> row 11
    kb2 = s.kp(mnx + f32(400) + cw, mny + f32(10.4) * ch, near)
    s.query(mnx + f32(400), mny + f32(10.45) * ch, BASE, r=2 * float(cw))
    # on maxX / maxY (cell 64 / 48: outside), just under (rounds up: outside) and half a cell under (inside)
    for (kx, ky, ok) in [(mxx, mny + f32(200), False), (below(mxx), mny + f32(250), False),
                         (mxx - f32(0.6) * cw, mny + f32(300), True),
                         (mnx + f32(300), mxy, False), (mnx + f32(350), below(mxy), False),
                         (mnx + f32(450), mxy - f32(0.6) * ch, True)]:
        k = s.kp(kx, ky, near)
        s.query(f32(kx) - 1, f32(ky) - 1, BASE, expect=(k if ok else -1) if bounds is None else None)
    del ka, ka2, kb2
    return _proj("grid" + ("-bounds" if bounds else ""), variant, s,
                 ["cell==-.5", "cell==k+.5", "on-max", "under-max"] if bounds is None else ["nonzero-bounds"])


# ---- E5: level filter (Frame.cc:385-392: bCheckLevels = minLevel > 0 || maxLevel >= 0) ------------------
def proj_levels(variant):
    s = Scene()
    i = 0
    for (mn, mx, octs_ok) in [(0, -1, {0, 3, 7}), (2, -1, {2, 3, 7}), (2, 4, {2, 3, 4}), (0, 3, {0, 3})]:
        for octv in (0, 1, 2, 3, 4, 5, 7):
            x, y = s.island(i); i += 1
            k = s.kp(x + 1, y, flip(BASE, 5), octave=octv)
            ok = octv >= mn and (mx < 0 or octv <= mx)
            s.query(x, y, BASE, min_level=mn, max_level=mx, expect=k if ok else -1)
    return _proj("levels", variant, s, ["no-check", "min-only", "octave==min", "octave==max", "octave-outside"])


# ---- E6: stereo gate of localmap / lastframe (ORBmatcher.cc:91-96, 1406-1411) ---------------------------
def proj_stereo(variant):
    s = Scene(stereo=True)
    near, far = flip(BASE, 0), flip(BASE, 10)
    for i, (ur_kp, kept) in enumerate([(0.0, True), (42.0, True), (below(42.0), False), (58.0, True),
                                       (above(58.0), False), (-1.0, True)]):
        x, y = s.island(i)
        ke = s.kp(x + 1, y, near, ur=ur_kp)      # mvuRight 0: no gate ('> 0'); |er| == tol: kept ('>')
        kf = s.kp(x - 1, y, far)
        s.query(x, y, BASE, ur=50.0, ur_tol=8.0, expect=ke if kept else kf)
    return _proj("stereo", variant, s, ["uright==0", "|er|==tol", "|er|>tol"])


# ---- E7: rotation consistency (ORBmatcher.cc:1434-1469, 1568-1598; ComputeThreeMaxima :1603-1644) ------
def _rot_scene(rots):
    """One matched island per entry of rots: (query angle, keypoint angle, kept)."""
    s = Scene()
    for i, (qa, ka, kept) in enumerate(rots):
        x, y = s.island(i)
        k = s.kp(x + 1, y, flip(BASE, 1), angle=ka)
        s.query(x, y, BASE, angle=qa, expect=k if kept else -1)
    return s


def proj_rot_half(variant):
    # 15, 135, 255 deg: rot * (1/30f) is exactly .5, 4.5, 8.5 -> bins 1, 5, 9 (half-even: 0, 4, 8).
    # Bins 0, 4, 8 hold 5, 4, 4 matches, so the half-bin matches go with bins 1, 5, 9.
    rots = [(0.0, 0.0, True)] * 5 + [(10.0, 250.0, True)] * 4 + [(240.0, 0.0, True)] * 4    # (10 - 250 wraps by +360)
    rots += [(15.0, 0.0, False), (135.0, 0.0, False), (255.0, 0.0, False), (359.99, 0.0, False)]
    return _proj("rot-half", variant, _rot_scene(rots), ["rot-half-bin", "rot-wrap", "rot-near-360"], check_ori=True)


def proj_rot_histo(variant, name, rots, edge):
    return _proj(name, variant, _rot_scene(rots), [edge], check_ori=True)


# ---- E8: ties (first candidate in GetFeaturesInArea order: column, row, index) ---------------------------
def proj_ties(variant):
    s = Scene()
    s.kp(96.0, 100.0, flip(BASE, 4))             # index 0: column 10
    k1 = s.kp(94.0, 100.0, flip(BASE, 4, 8))     # index 1: column 9, first in area order
    s.kp(94.5, 101.0, flip(BASE, 4, 16), octave=1)   # k1's cell, after it: the second, on another octave
    s.query(95.0, 100.0, BASE, r=12.0, expect=k1)
    ka = s.kp(300.0, 96.0, flip(BASE, 4)); kb = s.kp(300.0, 94.0, flip(BASE, 4, 8))   # same column: row order
    s.query(300.0, 95.0, BASE, r=12.0, expect=kb if variant != "localmap" else -1)
    del ka
    return _proj("ties", variant, s, ["tie-across-columns", "tie-across-rows"])


# ---- E9: capacities of the projection replay -----------------------------------------------------------
def proj_entries(variant, count):
    """A blocking query with `count` entries within th_dist (the 4 kept ones and
    the `hard` registration from the fifth on), then queries that take from it."""
    s = Scene()
    x, y = s.island(0)
    ks = [s.kp(x - 3 + j, y + (j % 2), flip(BASE, j + 1), octave=j % 2) for j in range(count)]
    s.kp(x, y + 4, flip(BASE, 120))              # beyond every th_dist
    for j in range(count + 1):                   # each takes the best that is left; the last finds none
        s.query(x, y, BASE, expect=ks[j] if j < count else -1)
    return _proj(f"entries{count}", variant, s, [f"within-th=={count}", "taken-seen"])


def proj_chain(variant, nq=80):
    """Query i sees k(i-1) at distance 1 and k(i) at 2; k(i-1) goes to query
    i-1, so every decision waits on the one before: one query a round."""
    s = Scene()
    d = BASE
    ks = []
    for i in range(nq):
        d = flip(d, 3, 3 * i)                    # k(i) = k(i-1) with 3 more bits
        ks.append(s.kp(20.0 + 6.0 * i, 100.0, d))
    for i in range(nq):
        qd = flip(s.d[ks[i - 1]], 1, 3 * i) if i else flip(s.d[ks[0]], 2, 200)
        u = 20.0 + 6.0 * i - 3.0 if i else 20.0
        s.query(u, 100.0, qd, r=4.0, expect=ks[i])
    return _proj("chain", variant, s, ["chain>64"], th_dist=50)


def proj_queue(variant, nq=600):
    """Every query's 4 nearest keypoints are taken from the start and its fifth
    is its own: all need their full list in the first round (kFQ = 512)."""
    s = Scene()
    taken = 3 if variant in ("localmap", "lastframe") else 1
    for j in range(4):
        s.kp(300.0 + j, 200.0, flip(BASE, j + 1, 248), state=taken)   # 3 .. 6 from every query
    pairs = [(a, b) for a in range(40) for b in range(a + 1, 40)][:nq]
    own = []
    for q, (a, b) in enumerate(pairs):       # query q: two bits of its own; its keypoint: 10 more (the same 10)
        dq = flip(flip(BASE, 1, a), 1, b)
        own.append(s.kp(296.0 + (q % 30) * 0.25, 196.0 + (q // 30) * 0.25, flip(dq, 10, 40)))
        s.query(300.0, 200.0, dq, r=9.0, expect=own[q])
    # a free keypoint at 11 from every query: the second of the two free ones the ratio test reads, claimed by none
    s.kp(300.0, 204.0, flip(BASE, 9, 50))
    # own keypoint at 10, the shared one at 11, every other query's at 12 or 14: th_dist 10 leaves one claim past
    # the 4 kept, and nothing a query examines can go to an earlier one, so each is decided in the round it is scanned
    return _proj("queue", variant, s, ["full-list>512"], th_dist=10, nnratio=1.0)


def proj_overflow(variant, nq=64, n=100):
    """64 queries x 100 identical-descriptor keypoints in every window:
    6400 claims > hard_cap = 4 * 64 + 4096, everything is decided in order."""
    s = Scene()
    for j in range(n):
        s.kp(300.0 + (j % 10) * 1.5, 200.0 + (j // 10) * 1.5, BASE, octave=j % 2)
    for q in range(nq):
        s.query(306.0, 206.0, BASE, r=12.0)
    return _proj("overflow", variant, s, ["hard>cap"])


def proj_list_len(variant, T):
    """One window whose cell range holds exactly T keypoints (kEnt = 512), the
    best one last in area order."""
    s = Scene()
    for i in range(T - 1):
        s.kp(300.0 + (i % 30), 200.0 + (i // 30), flip(BASE, 30 + i % 7, i % 200))
    best = s.kp(338.0, 222.0, flip(BASE, 5))     # the highest column and row of the range
    s.query(318.0, 210.0, BASE, r=26.0, expect=best)
    s.query(318.0, 210.0, BASE, r=26.0)          # the same list with its best taken
    return _proj(f"list{T}", variant, s, [f"list=={T}"])


def proj_nonblocking(variant):
    """A non-blocking take (Observations() == 0) leaves the keypoint to the
    next query; a blocking one closes it."""
    s = Scene()
    x, y = s.island(0)
    a = s.kp(x + 1, y, flip(BASE, 1)); b = s.kp(x - 1, y, flip(BASE, 9), octave=1)
    s.query(x, y, BASE, flags=1, expect=a)
    s.query(x, y, BASE, flags=3, expect=a)
    s.query(x, y, BASE, flags=3, expect=b)
    return _proj("nonblocking", variant, s, ["nonblocking-retaken"])


def proj_fuse_long(variant):
    s = Scene()
    x, y = s.island(0)
    ks = [s.kp(x - 4 + j, y, flip(BASE, 40 - (j if j < 7 else 0))) for j in range(9)]
    s.query(x, y, BASE, expect=ks[6])
    return _proj("fuse-long", variant, s, ["fuse-min-late"])


def chi2_neighbours(limit):
    """The largest float <= limit and the smallest float > limit."""
    lo = f32(limit) if float(f32(limit)) <= limit else below(f32(limit))
    return lo, above(lo)


def _chi2_offset(limit, inside):
    """(d, e, octave): float errors with (e * e + d * d) * invSigma2[octave],
    each step in float, exactly the representable value next to the limit on
    that side.  e is a multiple of 1/1024 (exact as a coordinate offset), d free."""
    sf, _ = scale_tables(1.2, 8)
    isg = (f32(1) / (sf * sf)).astype(np.float32)
    target = chi2_neighbours(limit)[0 if inside else 1]
    for octv in range(8):
        e = (np.arange(0, 1024) / 1024.0).astype(np.float32)
        d = np.sqrt(float(target) / float(isg[octv]) - e.astype(np.float64) ** 2).astype(np.float32)
        for _ in range(40):
            d = np.nextafter(d, f32(-np.inf))
        for _ in range(80):
            hit = np.nonzero(((e * e + d * d) * isg[octv]).astype(np.float32) == target)[0]
            if len(hit):
                return f32(d[hit[0]]), f32(e[hit[0]]), octv
            d = np.nextafter(d, f32(np.inf))
    raise AssertionError(f"no float error lands on {target}")


def proj_fuse_chi2():
    """Fuse's reprojection gate (ORBmatcher.cc:903-932): mvuRight >= 0 takes
    the 3-term form (limit 7.8), else the 2-term form (5.99); '>' rejects."""
    s = Scene(stereo=True)
    near, far = flip(BASE, 0), flip(BASE, 10)
    x, y = s.island(0)             # mvuRight == 0 is stereo here ('>= 0'): ex = 1, er = 3 -> 10 > 7.8
    s.kp(x + 1, y, near, ur=0.0); kf = s.kp(x, y + 1, far)
    s.query(x, y, BASE, ur=3.0, expect=kf)
    x, y = s.island(1)             # mvuRight < 0: 2 terms, er ignored
    k = s.kp(x + 1, y, near, ur=-1.0); s.kp(x, y + 1, far)
    s.query(x, y, BASE, ur=300.0, expect=k)
    i = 2
    for limit, stereo in ((7.8, True), (5.99, False)):
        for inside in (True, False):
            x, y = s.island(i); i += 1
            d, e, octv = _chi2_offset(limit, inside)
            # stereo: e in ey, d in er (mvuRight 0, so er = Q.ur); mono: e in ex, d in ey (the keypoint at y = 0)
            if stereo:
                k = s.kp(x, y, near, octave=octv, ur=0.0)
                s.kp(x, y + 1, far, ur=-1.0)
                s.query(x, f32(y) + e, BASE, ur=d, expect=k if inside else k + 1)
            else:
                k = s.kp(x, 0.0, near, octave=octv, ur=-1.0)
                s.kp(x + 1, 0.0, far, octave=7, ur=-1.0)
                s.query(f32(x) + e, d, BASE, r=12.0, expect=k if inside else k + 1)
    return _proj("chi2", "fuse", s, ["fuse-uright==0", "fuse-mono", "chi2-7.8-inside", "chi2-7.8-outside",
                                     "chi2-5.99-inside", "chi2-5.99-outside"])


def proj_fuse_octave_outside():
    """Fuse with keypoint octaves outside [0, nlevels): the reference reads
    past mvInvLevelSigma2 there, so nothing decides the answer and the oracle
    refuses the input; liborbx takes invSigma2 as 0, so the gate passes.  For
    the GPU test alone, held to `expect`."""
    s = Scene(stereo=True)
    for i, (octv, ur) in enumerate([(8, -1.0), (-1, -1.0), (8, 0.0), (200, 5.0)]):
        x, y = s.island(i)
        k = s.kp(x + 7, y, flip(BASE, 3), octave=octv, ur=ur)      # 49 px^2: fails both limits at any real octave
        s.query(x, y, BASE, ur=40.0, expect=k)
    return _proj("octave-outside", "fuse", s, [])


def proj_cases():
    out = [proj_fuse_chi2()]
    for v in PROJ_VARIANTS:
        out += [proj_thresholds(v), proj_window(v), proj_grid(v), proj_levels(v), proj_ties(v),
                proj_thresholds(v, bounds=BOUNDS_DISTORTED), proj_grid(v, bounds=BOUNDS_DISTORTED)]
    out.append(proj_thresholds("keyframe", 100))
    out += [proj_ratio(r) for r in RATIO_PAIRS]
    for v in ("localmap", "lastframe"):
        out += [proj_stereo(v), proj_nonblocking(v)]
    for v in ("lastframe", "keyframe"):
        out += [proj_rot_half(v)] + [proj_rot_histo(v, name, rots, edge) for name, rots, edge in ROT_HISTOS]
    for v in REPLAY_VARIANTS:
        out += [proj_entries(v, 3), proj_entries(v, 4), proj_entries(v, 5), proj_chain(v), proj_list_len(v, 511),
                proj_list_len(v, 512), proj_list_len(v, 513)]
    for v in ("localmap", "keyframe"):
        out += [proj_queue(v), proj_overflow(v)]
    for v in ("fuse", "fuse_sim3"):
        out.append(proj_fuse_long(v))
    return out


# ======================= SearchByBoW x2 / SearchForTriangulation =========================================
class BowScene:
    """Nodes of (A features, B features); a feature is (descriptor, angle, flags)."""

    def __init__(self):
        self.a, self.b = [], []          # (desc, angle, flags, y)
        self.na, self.nb = {}, {}        # node id -> feature indices
        self.expect = {}

    def node(self, nid, A, B, expect=None):
        """A, B: lists of (desc[, angle[, flags[, x[, y[, octave]]]]]).  expect: per A feature of
        the node, the position in B it must match (None: no match)."""
        ia, ib = [], []
        for side, feats, idx in ((self.a, A, ia), (self.b, B, ib)):
            for f in feats:
                f = tuple(f) if isinstance(f, tuple) else (f,)
                desc, ang, fl = f[0], (f[1] if len(f) > 1 else 0.0), (f[2] if len(f) > 2 else 1)
                row = f32(20.0 + 2.0 * (nid % 200))                              # one image row per node
                side.append((desc, f32(ang), fl, f32(f[4]) if len(f) > 4 else row, f32(f[3]) if len(f) > 3 else None,
                             f[5] if len(f) > 5 else 0))
                idx.append(len(side) - 1)
        if A:
            self.na[nid] = ia
        if B:
            self.nb[nid] = ib
        if expect is not None:
            for i, e in zip(ia, expect):
                self.expect[i] = -1 if e is None else ib[e]

    def build(self):
        def side(feats, nodes):
            k = np.zeros(len(feats), KEYPOINT_DTYPE)
            k["x"] = [f32(10.0 + 3.0 * (i % 200)) if f[4] is None else f[4] for i, f in enumerate(feats)]
            k["y"] = [f[3] for f in feats]
            k["angle"] = [f[1] for f in feats]
            k["octave"] = [f[5] for f in feats]
            k["class_id"] = -1
            ids = np.array(sorted(nodes), np.uint32)
            off = np.zeros(len(ids) + 1, np.int32)
            feat = []
            for j, nid in enumerate(ids):
                feat += nodes[int(nid)]
                off[j + 1] = len(feat)
            return dict(keys=k, desc=np.array([f[0] for f in feats], np.uint8).reshape(-1, 32),
                        flags=np.array([f[2] for f in feats], np.uint8), ids=ids, off=off,
                        feat=np.array(feat, np.int32))
        return side(self.a, self.na), side(self.b, self.nb)


def _tri_params(epipole=(-5000.0, -5000.0), zero_f=False):
    # F12 maps (x1, y1) to the line y2 = y1: a = 0, b = 1, c = -y1.  The epipole is far away.
    sf, _ = scale_tables(1.2, 8)
    F = np.zeros(9, np.float32)
    if not zero_f:
        F[7] = 1.0; F[5] = -1.0
    return np.concatenate([F, [f32(epipole[0]), f32(epipole[1])], sf, (sf * sf)]).astype(np.float32)


def _bow(name, variant, scene, edges, nnratio=0.75, check_ori=False, tri=None):
    A, B = scene.build()
    expect = np.full(len(A["keys"]), -9, np.int32)
    for i, e in scene.expect.items():
        expect[i] = e
    return dict(family="bow", name=f"{name}-{variant}", variant=variant, A=A, B=B, edges=edges, nnratio=nnratio,
                check_ori=check_ori, expect=expect,
                tri=(_tri_params() if tri is None else tri) if variant == "triangulation" else None)


BOW_VARIANTS = ["kf_frame", "kf_kf", "triangulation"]


def bow_thresholds(variant):
    # ORBmatcher.cc:229 '<= TH_LOW' (KF, F); :600 '< TH_LOW' (KF, KF); :688/:740 '> TH_LOW -> continue'
    s = BowScene()
    ok = {49: True, 50: variant != "kf_kf", 51: False, 256: False}
    for n, dist in enumerate((49, 50, 51, 256)):
        s.node(10 + n, [BASE], [flip(BASE, dist)], expect=[0 if ok[dist] else None])
    s.node(20, [BASE], [flip(BASE, 48), flip(BASE, 256)], expect=[0])   # 256 as the second best
    return _bow("thresholds", variant, s, ["best==50", "best==49", "best==51", "best==256"], nnratio=0.95)


def bow_ratio(variant, nnratio):
    # :231 / :602: float(bestDist1) < mfNNratio * float(bestDist2), a float product
    b, b2 = RATIO_PAIRS[nnratio]
    s = BowScene()
    r = f32(nnratio)
    pairs = [(b, b2), (b + 1, b2), (b - 1, b2), (b, b2 + 1), (b, b2 - 1)] + ([(15, 25)] if nnratio == 0.6 else [])
    for n, (d1, d2) in enumerate(p for p in pairs if p[0] <= p[1]):
        acc = f32(d1) < f32(r * f32(d2))
        s.node(10 + n, [BASE], [flip(BASE, d2), flip(BASE, d1, 64)], expect=[1 if acc else None])
    s.node(90, [BASE], [flip(BASE, 49)], expect=[0 if f32(49) < f32(r * f32(256)) else None])  # best2 = 256
    return _bow(f"ratio{nnratio}", variant, s, ["ratio==", "single-candidate"], nnratio=nnratio)


def bow_rot(variant, rots, name, edges):
    s = BowScene()
    for n, (aa, ab, kept) in enumerate(rots):
        s.node(10 + n, [(BASE, aa)], [(flip(BASE, 1), ab)], expect=[0 if kept else None])
    return _bow(name, variant, s, edges, nnratio=0.95, check_ori=True)


def bow_ties(variant):
    # identical B descriptors: the first in node order wins in SearchByBoW ('<'), the last in
    # SearchForTriangulation (:688 'dist > bestDist -> continue')
    s = BowScene()
    # (a tie at the best fails every ratio test with mfNNratio <= 1: 1.2 lets the winner show)
    d = flip(BASE, 7)
    last = variant == "triangulation"
    s.node(10, [BASE], [d, d, flip(BASE, 30)], expect=[1 if last else 0])
    s.node(11, [BASE], [flip(BASE, 30), d, flip(BASE, 40), d], expect=[3 if last else 1])
    s.node(12, [BASE], [flip(BASE, 7), flip(BASE, 7, 64), flip(BASE, 45)], expect=[1 if last else 0])
    return _bow("ties", variant, s, ["tie-at-best"], nnratio=0.6 if last else 1.2)


def bow_flag_b(variant):
    # KF/KF: a B feature without a (good) map point is passed over (:588-596)
    s = BowScene()
    s.node(10, [BASE], [(flip(BASE, 2), 0.0, 0), flip(BASE, 20)], expect=[0 if variant == "kf_frame" else 1])
    s.node(11, [BASE], [], expect=[None])            # a node on one side only
    s.node(12, [], [flip(BASE, 1)])
    return _bow("flag-b", variant, s, ["b-flag-clear", "one-sided-node"], nnratio=0.95)


def tri_gates():
    """SearchForTriangulation's gates (ORBmatcher.cc:716-734): the epipole
    distance (both features monocular only, '< 100 * scale'), den == 0 of
    CheckDistEpipolarLine (:1647-1665 region) and dsqr < 3.84 * sigma2."""
    s = BowScene()
    ex, ey = 300.0, 40.0                       # nodes 10, 210, 410 ... share the image row y = 40
    near = flip(BASE, 3)
    nid = 10
    for (st1, st2, x2, ok) in [(0, 0, ex + 9.0, False), (2, 0, ex + 9.0, True), (0, 2, ex + 9.0, True),
                               (2, 2, ex + 9.0, True), (0, 0, ex + 10.0, True), (0, 0, below(ex + 10.0), False),
                               (0, 0, ex - 10.0, True), (0, 0, above(ex - 10.0), False)]:
        s.node(nid, [(BASE, 0.0, 1 | st1)], [(near, 0.0, 1 | st2, x2, ey)], expect=[0 if ok else None])
        nid += 200
    # dsqr = (y2 - y1)^2 at octave 0 (sigma2 1): the floats either side of sqrt(3.84), far from the epipole
    y1 = f32(20.0 + 2.0 * (nid % 200))
    lo = f32(y1 + f32(1.9))
    while float(f32(f32(above(lo) - y1) * f32(above(lo) - y1))) < 3.84:
        lo = above(lo)
    for y2, ok in [(lo, True), (above(lo), False), (f32(y1 - f32(lo - y1)), True)]:
        s.node(nid, [(BASE, 0.0, 1)], [(near, 0.0, 1, 100.0, y2)], expect=[0 if ok else None])
        nid += 200
    # an octave outside [0, nlevels) has no scale / sigma2 entry: both 0, so the epipolar test rejects the pair
    for octv in (-1, 8):
        s.node(nid, [(BASE, 0.0, 1)], [(near, 0.0, 1, 100.0, y1, octv)], expect=[None])
        nid += 200
    return _bow("tri-gates", "triangulation", s, ["epipole-gate-mono", "epipole-gate-stereo", "epipole==limit",
                                                  "dsqr-inside", "dsqr-outside", "tri-octave-outside"],
                nnratio=0.6,
                tri=_tri_params((ex, ey)))


def tri_den0():
    s = BowScene()
    s.node(10, [BASE], [flip(BASE, 3)], expect=[None])      # F12 maps the point to the zero line: rejected
    return _bow("tri-den0", "triangulation", s, ["den==0"], nnratio=0.6, tri=_tri_params(zero_f=True))


def bow_node_sizes(variant):
    """Node sizes around the 64-lane path on both sides: descriptors a few
    bits from one hub, so the taken state decides most features."""
    rng = np.random.default_rng(13)              # filler
    s = BowScene()
    nid = 100
    for nb in (1, 63, 64, 65, 129):
        for na in (1, 63, 64, 65, 129):
            A = [(flip(flip(BASE, int(rng.integers(0, 6)), int(rng.integers(0, 250))), 1, int(rng.integers(0, 256))),
                  float(rng.integers(0, 2)) * 40.0) for _ in range(na)]
            B = [(flip(flip(BASE, int(rng.integers(0, 6)), int(rng.integers(0, 250))), 1, int(rng.integers(0, 256))),
                  0.0) for _ in range(nb)]
            s.node(nid, A, B)
            nid += 7
    return _bow("node-sizes", variant, s, ["node-sizes"], nnratio=0.95, check_ori=True)


ROT_HALF = [(0.0, 0.0, True)] * 5 + [(10.0, 250.0, True)] * 4 + [(240.0, 0.0, True)] * 4 + \
    [(15.0, 0.0, False), (135.0, 0.0, False), (255.0, 0.0, False), (359.99, 0.0, False)]


# ComputeThreeMaxima histograms (one copy of it per kernel family): (name, pairs, edge)
ROT_HISTOS = [
    # four bins of 3: the first three by index stay (strict '>')
    ("rot-tie", [(0.0, 0.0, True)] * 3 + [(60.0, 0.0, True)] * 3 + [(120.0, 0.0, True)] * 3 + [(240.0, 0.0, False)] * 3,
     "histo-tie"),
    # max2 == 0.1f * max1 (10 and 1): kept; 11 and 1: dropped with the third
    ("rot-tenth10", [(0.0, 0.0, True)] * 10 + [(60.0, 0.0, True), (120.0, 0.0, True), (240.0, 0.0, False)],
     "histo-tenth=="),
    ("rot-tenth11", [(0.0, 0.0, True)] * 11 + [(60.0, 0.0, False), (120.0, 0.0, False), (240.0, 0.0, False)],
     "histo-tenth<"),
    # the third maximum on the boundary: 20, 5, 2 (2 == 0.1f * 20: kept) and a fourth bin of 1
    ("rot-third", [(0.0, 0.0, True)] * 20 + [(60.0, 0.0, True)] * 5 + [(120.0, 0.0, True)] * 2 + [(240.0, 0.0, False)],
     "histo-third=="),
    ("rot-two-bins", [(0.0, 0.0, True)] * 3 + [(60.0, 0.0, True)] * 2, "histo-two-bins"),
]


def bow_node_ids(variant, nb):
    """Side B's node-id list of nb ids (one feature a node), searched 64 pivots
    a round: every id of B is sought from A, and ids below, between and above."""
    s = BowScene()
    ids = [1000 + 10 * j for j in range(nb)]
    for j, nid in enumerate(ids):
        d = flip(BASE, 2, (7 * j) % 250)
        s.node(nid, [d], [flip(d, 1, 252)], expect=[0])
    for nid in (5, 1005, ids[-1] + 5) if nb > 1 else (5, ids[-1] + 5):
        s.node(nid, [BASE], [], expect=[None])
    return _bow(f"node-ids{nb}", variant, s, [f"ids=={nb}", "id-first", "id-last", "id-absent"], nnratio=0.95)


def bow_cases():
    out = []
    for v in BOW_VARIANTS:
        out += [bow_thresholds(v), bow_ties(v), bow_flag_b(v), bow_node_sizes(v),
                bow_rot(v, ROT_HALF, "rot-half", ["rot-half-bin", "rot-wrap"])]
        out += [bow_rot(v, rots, name, [edge]) for name, rots, edge in ROT_HISTOS]
        out += [bow_node_ids(v, nb) for nb in (1, 64, 65, 4097)]
    for v in ("kf_frame", "kf_kf"):
        out += [bow_ratio(v, r) for r in RATIO_PAIRS]
    return out + [tri_gates(), tri_den0()]


# ======================= SearchForInitialization (ORBmatcher.cc:406-521) =================================
def _init(name, f1, f2, edges, window=8, nnratio=0.9, check_ori=False, bounds=None, expect=None):
    def frame(feats):
        k = np.zeros(len(feats), KEYPOINT_DTYPE)
        for i, (x, y, _, ang) in enumerate(feats):
            k[i] = (f32(x), f32(y), 31.0, f32(ang), 0.0, 0, -1)
        return k, np.array([f[2] for f in feats], np.uint8).reshape(-1, 32)
    k1, d1 = frame(f1)
    k2, d2 = frame(f2)
    prev = np.ascontiguousarray(np.stack([k1["x"], k1["y"]], 1).astype(np.float32))
    return dict(family="init", name=name, k1=k1, d1=d1, k2=k2, d2=d2, prev=prev, window=window, nnratio=nnratio,
                check_ori=check_ori, bounds=bounds, edges=edges, expect=expect)


def _isl(i):
    return 35.0 + 50.0 * (i % 12), 35.0 + 50.0 * (i // 12)


def init_thresholds(bounds=None):
    f1, f2, exp = [], [], []
    for i, (dist, ok) in enumerate([(49, True), (50, True), (51, False), (256, False)]):   # :478 '<= TH_LOW'
        x, y = _isl(i)
        f1.append((x, y, BASE, 0.0)); f2.append((x + 1, y, flip(BASE, dist), 0.0)); exp.append(i if ok else -1)
    x, y = _isl(4)                         # 256 as the second best
    f1.append((x, y, BASE, 0.0)); f2 += [(x + 1, y, flip(BASE, 50), 0.0), (x - 1, y, flip(BASE, 256), 0.0)]
    exp.append(4)
    return _init("init-thresholds" + ("-bounds" if bounds else ""), f1, f2, ["best==50", "best==51", "second==256"],
                 nnratio=1.0, bounds=bounds, expect=exp)


def init_ratio(nnratio):
    b, b2 = RATIO_PAIRS[nnratio] if nnratio != 1.0 else (37, 37)
    b, b2 = min(b, 50), b2
    r = f32(nnratio)
    f1, f2, exp = [], [], []
    pairs = [(b, b2), (b - 1, b2), (b, b2 + 1), (b, b2 - 1)] + ([(15, 25)] if nnratio == 0.6 else [])
    for i, (d1, d2) in enumerate(p for p in pairs if p[0] <= p[1]):
        x, y = _isl(i)
        f1.append((x, y, BASE, 0.0))
        f2 += [(x + 2, y, flip(BASE, d2), 0.0), (x - 2, y, flip(BASE, d1, 64), 0.0)]
        exp.append(2 * i + 1 if f32(d1) < f32(f32(d2) * r) else -1)                         # :480
    x, y = _isl(len(f1))
    f1.append((x, y, BASE, 0.0)); f2.append((x + 1, y, flip(BASE, 50), 0.0)); exp.append(len(f2) - 1)   # best2 INT_MAX
    return _init(f"init-ratio{nnratio}", f1, f2, ["ratio==", "single-candidate"], nnratio=nnratio, expect=exp)


def init_ties_steal():
    f1, f2, exp = [], [], []
    x, y = _isl(0)                     # tie: the first in area order (column 3 before column 4)
    f1.append((x, y, BASE, 0.0)); f2 += [(x + 6, y, flip(BASE, 5), 0.0), (x - 6, y, flip(BASE, 5, 8), 0.0),
                                         (x, y + 3, flip(BASE, 30), 0.0)]
    exp.append(1)
    x, y = _isl(1)                     # steal: the later, closer feature takes the keypoint back (:482-486)
    f1 += [(x, y, flip(BASE, 9), 0.0), (x + 1, y, BASE, 0.0)]
    f2.append((x, y + 1, flip(BASE, 2), 0.0))
    exp += [-1, 3]
    x, y = _isl(2)                     # an equal distance does not steal (:462 'vMatchedDistance[i2] <= dist')
    f1 += [(x, y, flip(BASE, 4), 0.0), (x + 1, y, flip(BASE, 4, 100), 0.0)]
    f2.append((x, y + 1, BASE, 0.0))
    exp += [4, -1]
    for j, cnt in enumerate((3, 4, 5)):    # 3, 4, 5 candidates, the best last
        x, y = _isl(3 + j)
        f1.append((x, y, BASE, 0.0))
        for t in range(cnt):
            f2.append((x - 4 + 2 * t, y + 1, flip(BASE, 40 - 5 * t, 8 * t), 0.0))
        exp.append(len(f2) - 1)
    # (a tie at the best fails the ratio test with mfNNratio <= 1: 1.2 lets the winner show)
    return _init("init-ties-steal", f1, f2, ["tie-at-best", "steal", "equal-no-steal"], nnratio=1.2, expect=exp)


def init_rot_half():
    f1, f2, exp = [], [], []
    for i, (a1, a2, kept) in enumerate(ROT_HALF):
        x, y = _isl(i)
        f1.append((x, y, BASE, a1)); f2.append((x + 1, y, flip(BASE, 1), a2)); exp.append(i if kept else -1)
    return _init("init-rot-half", f1, f2, ["rot-half-bin", "rot-wrap"], check_ori=True, expect=exp)


def init_window_grid():
    """The window test (Frame.cc:395-396, 'fabs(d) < r') and PosInGrid's
    rounding (:415-425) as SearchForInitialization sees them (window 8)."""
    f1, f2, exp = [], [], []
    near, far = BASE, flip(BASE, 10)
    i = 0
    for axis in (0, 1):
        for side, inside in [(8.0, False), (8.0, True), (-8.0, False), (-8.0, True)]:
            x, y = _isl(i); i += 1
            at = f32((x, y)[axis]) + f32(side)
            if inside:
                at = below(at) if side > 0 else above(at)
            f1.append((x, y, BASE, 0.0))
            f2 += [(at if axis == 0 else x, at if axis == 1 else y, near, 0.0), (x + 1, y + 1, far, 0.0)]
            exp.append(len(f2) - (2 if inside else 1))
    # (x - 0) * (64 / 640) == -0.5: cell -1, outside the grid (half-to-even would keep it), on each axis
    for (px, py, kx, ky, fx, fy) in [(1.0, 100.0, -5.0, 100.0, 3.0, 100.0), (200.0, 1.0, 200.0, -5.0, 200.0, 3.0)]:
        f1.append((px, py, BASE, 0.0))
        f2 += [(kx, ky, near, 0.0), (fx, fy, far, 0.0)]
        exp.append(len(f2) - 1)
    # exactly .5 inside the frame: column 1 / row 1, so the tie goes to the keypoint of column 0 / row 0
    f1.append((4.5, 300.0, BASE, 0.0))
    f2 += [(5.0, 300.0, flip(BASE, 3), 0.0), (4.0, 306.0, flip(BASE, 3), 0.0)]   # (3 < 1.2 * 3 passes the ratio test)
    exp.append(len(f2) - 1)
    return _init("init-window-grid", f1, f2, ["init-|d|==r", "init-next-inside", "init-cell==-.5", "init-cell==k+.5"],
                 window=8, nnratio=1.2, expect=exp)


def init_rot(name, rots, edges):
    f1, f2, exp = [], [], []
    for i, (a1, a2, kept) in enumerate(rots):
        x, y = _isl(i)
        f1.append((x, y, BASE, a1)); f2.append((x + 1, y, flip(BASE, 1), a2)); exp.append(i if kept else -1)
    return _init(name, f1, f2, edges, check_ori=True, expect=exp)


def init_steal_in_bin():
    """A stolen pair stays in its rotation bin (ORBmatcher.cc:482-507: the
    rotHist entry of the loser is never removed).  Bins with the stolen pair:
    0: 2, 2: 3, 4: 3, 8: 2 -> bins 2, 4, 0 stay; without it bin 0 has 1 and
    bin 8 would take its place."""
    f1, f2, exp = [], [], []

    def pair(i, a1, kept):
        x, y = _isl(i)
        f1.append((x, y, BASE, a1)); f2.append((x + 1, y, flip(BASE, 1), 0.0)); exp.append(len(f2) - 1 if kept else -1)
    x, y = _isl(0)
    f1 += [(x, y, flip(BASE, 9), 0.0), (x + 1, y, BASE, 60.0)]       # loser (bin 0), then the stealer (bin 2)
    f2.append((x, y + 1, flip(BASE, 2), 0.0))
    exp += [-1, 0]
    pair(1, 0.0, True)                                               # bin 0's only standing match
    for i in (2, 3):
        pair(i, 60.0, True)
    for i in (4, 5, 6):
        pair(i, 120.0, True)
    for i in (7, 8):
        pair(i, 240.0, False)
    return _init("init-steal-in-bin", f1, f2, ["steal", "stolen-pair-decides-bins"], check_ori=True, expect=exp)


def init_replay():
    """The replay's paths, built: the full-list walk (three of a query's four
    nearest keypoints already hold closer matches, the fourth and a fifth are
    free), a steal 11 live queries after its victim (inside a 64-query batch)
    and one 71 live queries after (across batches)."""
    f1, f2, exp = [], [], []
    isl = iter(range(108))
    x, y = _isl(next(isl))
    ks = [flip(BASE, 1, 0), flip(BASE, 2, 10), flip(BASE, 3, 20), flip(BASE, 4, 30), flip(BASE, 30, 40)]
    for j, d in enumerate(ks):
        f2.append((x - 4 + 2 * j, y + 1, d, 0.0))
    for j in range(3):                       # each takes its keypoint at distance 0
        f1.append((x + j - 1, y, ks[j], 0.0)); exp.append(j)
    f1.append((x, y - 1, BASE, 0.0)); exp.append(3)   # kept four: 1, 2, 3 (all closed), 4; then 30

    def filler(count):
        for _ in range(count):
            fx, fy = _isl(next(isl))
            f1.append((fx, fy, BASE, 0.0)); f2.append((fx + 1, fy, flip(BASE, 1), 0.0)); exp.append(len(f2) - 1)
    for gap in (10, 70):
        x, y = _isl(next(isl))
        f2.append((x, y + 1, flip(BASE, 2), 0.0))
        k = len(f2) - 1
        f1.append((x, y, flip(BASE, 9), 0.0)); exp.append(-1)        # the victim
        filler(gap)
        f1.append((x + 1, y, BASE, 0.0)); exp.append(k)              # the stealer, gap + 1 live queries later
    return _init("init-replay", f1, f2, ["full-list-walk", "steal-within-64", "steal-beyond-64", ">64-live"],
                 expect=exp)


def init_many(n=200):
    """More than 64 live queries over few distinct descriptors: steals inside a
    64-query batch of the replay and across batches."""
    rng = np.random.default_rng(17)        # filler
    f1, f2 = [], []
    for i in range(n):
        x, y = 40.0 + 28.0 * (i % 20), 40.0 + 40.0 * (i // 20)
        f1.append((x, y, flip(BASE, int(rng.integers(0, 12)), int(rng.integers(0, 200))), 0.0))
    for i in range(n // 2):
        x, y = 54.0 + 56.0 * (i % 10), 40.0 + 40.0 * (i // 10)
        f2.append((x, y, flip(BASE, int(rng.integers(0, 3)), int(rng.integers(0, 200))), 0.0))
    return _init("init-many", f1, f2, ["steal", ">64-live"], window=30, nnratio=1.0)


def init_cases():
    return [init_thresholds(), init_thresholds(BOUNDS_DISTORTED), init_ties_steal(), init_rot_half(), init_many(),
            init_window_grid(), init_steal_in_bin(), init_replay()] + \
        [init_rot("init-" + name, rots, [edge]) for name, rots, edge in ROT_HISTOS] + \
        [init_ratio(r) for r in (0.6, 0.75, 0.8, 0.9, 1.0)]


# ======================= SearchBySim3 (ORBmatcher.cc:1104-1328) ==========================================
def sim3_case():
    def frame(pts):
        k = np.zeros(len(pts), KEYPOINT_DTYPE)
        for i, (x, y, _, octv) in enumerate(pts):
            k[i] = (f32(x), f32(y), 31.0, 0.0, 0.0, octv, -1)
        return dict(keys=k, desc=np.array([p[2] for p in pts], np.uint8).reshape(-1, 32),
                    bounds=(0.0, float(W), 0.0, float(H)))

    def queries(rows):
        return (np.array([(f32(u), f32(v), 8.0, 0.0, 0.0, mn, mx, 0.0, fl) for (u, v, _, mn, mx, fl) in rows],
                         PROJ_QUERY_DTYPE), np.array([r[2] for r in rows], np.uint8).reshape(-1, 32))
    D = [flip(BASE, 20, 30 * i) for i in range(8)]      # slot i's descriptor, 40 apart from each other
    # slot i of each keyframe sits on island i; slot i of KF1 and slot i of KF2 see the same point unless said
    p1 = [(*_isl(i), D[i], 1) for i in range(8)]
    p2 = [(*_isl(i), flip(D[i], 2), 1) for i in range(8)]
    p2[3] = (*_isl(3), flip(D[3], 100), 1)               # 1->2 at exactly TH_HIGH (kept), 2->1 close
    p2[4] = (*_isl(4), flip(D[4], 101), 1)               # 101: no 1->2 match
    p2[5] = (*_isl(5), flip(D[5], 2), 3)                 # octave above [min_level, max_level]
    q1 = [(*_isl(i), D[i], 0, 1, 1) for i in range(8)]                 # KF1's points in KF2
    q2 = [(*_isl(i), flip(D[i], 2), 0, 1, 1) for i in range(8)]        # KF2's points in KF1
    q2[1] = (*_isl(2), flip(D[2], 1), 0, 1, 1)           # KF2 slot 1 lands on KF1 slot 2: 1 -> 1 is not returned
    q2[3] = (*_isl(3), D[3], 0, 1, 1)
    q1[6] = (*_isl(6), D[6], 0, 1, 0)                    # skipped by the caller's tests on one side
    # slot 8: two equal keypoints in KF2; the first in area order (the lower column) is the one that points back
    x8, y8 = _isl(8)
    p1.append((x8, y8, D[0], 1)); q1.append((x8, y8, D[0], 0, 1, 1))
    p2 += [(x8 + 6, y8, flip(D[0], 4), 1), (x8 - 6, y8, flip(D[0], 4), 1)]       # KF2 slots 8 (later column) and 9
    q2 += [(x8, y8, D[0], 0, 1, 0), (x8, y8, D[0], 0, 1, 1)]
    kf1, kf2 = frame(p1), frame(p2)
    a1, b1 = queries(q1)
    a2, b2 = queries(q2)
    return dict(family="sim3", name="sim3-agreement", kf1=kf1, kf2=kf2, q1=a1, qd1=b1, q2=a2, qd2=b2, th_dist=100,
                edges=["sim3-nonreciprocal", "sim3-best==th", "sim3-best==th+1", "sim3-octave-outside",
                       "sim3-one-side-skipped", "tie-at-best"], expect=[0, -1, 2, 3, -1, -1, -1, 7, 9])


_CACHE = {}


def all_cases():
    if not _CACHE:
        for c in proj_cases() + bow_cases() + init_cases() + [sim3_case()]:
            assert c["name"] not in _CACHE, c["name"]
            _CACHE[c["name"]] = c
    return _CACHE
