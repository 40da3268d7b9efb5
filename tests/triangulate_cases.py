"""CreateNewMapPoints problems shared by test_triangulate_reference.py and
test_triangulate_host_text.py (CPU), test_gpu_triangulate.py and
test_triangulate_forwarder.py, and their pyref_triangulate results, computed
once per session.

SIZES are the kernel's workgroup edges (64 lanes, one pair each: a single
pair, one short of a workgroup, exactly one, one over, two and a remainder) in
mono, stereo and mixed problems.  The named cases are constructed, each to
reach what its name says; test_triangulate_reference.py asserts from
pyref_triangulate that it does.

Two things the issue's list asks for cannot be reached through a pair and are
covered where they can be:
  * an A of exact rank 2 needs identical rays, whose cosine rounds to 1.0f,
    which no stereo cosine exceeds, so the parallax test never lets it through
    to the SVD.  "identical-rays" is that pair (status 1); "near-rank-2" is the
    closest pair that passes (cosRays one ulp under 1, two singular values some
    five hundred times under the others); the exact rank-2 matrix goes to the SVD alone
    (RANK2_A: pyref against the host text, test_triangulate_host_text.py; a
    host-only check, since the device's SVD is reached only through pairs).
  * a float error cannot equal the double product 5.991 sigma2.  The edge is
    taken on sigma2 instead: "reproj-edge-kept" has the smallest float sigma2
    whose threshold is not below the pair's error, "reproj-edge-rejected" the
    float below it."""
from __future__ import annotations

import functools

import numpy as np

import pyref_triangulate as ref
from orb_slam_2_ros_amd.synth_ba import _rot
from orb_slam_2_ros_amd.synth_triangulate import make_triangulation_problem, make_view, observe, scale_tables

SIZES = (1, 63, 64, 65, 130)
KINDS = {"mono": 0.0, "stereo": 1.0, "mixed": 0.5}
SIZE_CASES = tuple((n, k) for n in SIZES for k in KINDS)

CAM = (512.0, 512.0, 320.0, 240.0)     # powers of two: xn is exact
I3, Z3 = np.eye(3), np.zeros(3)
RF = np.float32(1.5) * np.float32(1.2)


def _obs(R, t, X, octave=0, stereo=False, mbf=40.0, cam=CAM, noise=(0.0, 0.0), raw_shift=(0.25, -0.5)):
    return observe(R, t, cam, mbf, X, octave, stereo, noise, raw_shift)


def _problem(v1, v2, pairs, **extra):
    K = np.zeros(len(pairs), ref.PAIR_DTYPE)
    for i, (a, b) in enumerate(pairs):
        K["o1"][i], K["o2"][i] = a, b
    return dict({"v1": v1, "v2": v2, "ratio_factor": RF, "pairs": K}, **extra)


def _two(baseline=0.5, R2=I3, mbf1=40.0, mbf2=40.0):
    """camera 1 at the origin, camera 2 at (baseline, 0, 0) with rotation R2"""
    t2 = -R2 @ np.array([baseline, 0.0, 0.0])
    return make_view(I3, Z3, CAM, mbf1), make_view(R2, t2, CAM, mbf2), (I3, Z3), (R2, t2)


def _xn(x, y):
    """the mono observation at the normalised coordinates (x, y), octave 0"""
    u, v = CAM[0] * x + CAM[2], CAM[1] * y + CAM[3]
    return (u, v, -1.0, -1.0, u + 0.25, v - 0.5, 1.0, 1.0)


def _clean(X=(0.3, -0.2, 4.0), st1=False, st2=False, **kw):
    v1, v2, (R1, t1), (R2, t2) = _two(**kw)
    return v1, v2, _obs(R1, t1, X, stereo=st1, mbf=kw.get("mbf1", 40.0)), \
        _obs(R2, t2, X, stereo=st2, mbf=kw.get("mbf2", 40.0))


def _low_parallax():
    v1, v2, a, b = _clean(X=(1.0, 2.0, 500.0))
    return _problem(v1, v2, [(a, b)])


def _parallax_edge():
    """the same point pushed away until cosRays crosses 0.9998 (baseline 0.5: near 25)"""
    v1, v2, (R1, t1), (R2, t2) = _two()
    return _problem(v1, v2, [(_obs(R1, t1, (0.25, 0.1, z)), _obs(R2, t2, (0.25, 0.1, z))) for z in (20.0, 30.0)])


def _w_zero():
    """Both rotations the identity, rays (0, y, 1) and (0, -y, 1): only columns
    0 and 3 of A are not orthogonal, columns 1 and 2 live on the other two
    rows, so V's rows 1 and 2 stay unit vectors; column 2 (norm sqrt(2) y) is
    the smallest and vt.row(3) = (0, 0, 1, 0) exactly."""
    v1, v2, _, _ = _two()
    return _problem(v1, v2, [(_xn(0.0, 0.125), _xn(0.0, -0.125))])


def _behind_first():
    """rays that meet behind both cameras"""
    v1, v2, _, _ = _two()
    return _problem(v1, v2, [(_xn(-0.1, 0.0), _xn(0.1, 0.0))])


def _first_sweep():
    """A with orthogonal columns: camera 2 sees camera 1's centre, the rays are
    (x, y, 1) and (-x, -y, 1), column 3 is zero.  The Jacobi's first sweep
    rotates nothing; the point is camera 1's centre (z1 = 0)."""
    v1 = make_view(I3, Z3, CAM)
    v2 = make_view(I3, np.array([-0.125, -0.0625, 1.0]), CAM)
    return _problem(v1, v2, [(_xn(0.125, 0.0625), _xn(-0.125, -0.0625))])


def _stereo1_behind_second():
    """Stereo on side 1, the second ray parallel to the first (no parallax), so
    the point is side 1's unprojection; camera 2 stands beyond it."""
    v1 = make_view(I3, Z3, CAM)
    t2 = np.array([0.0, 0.0, -10.0])
    a = _obs(I3, Z3, (0.3, -0.2, 5.0), stereo=True)
    return _problem(v1, make_view(I3, t2, CAM), [(a, _xn((a[0] - CAM[2]) / CAM[0], (a[1] - CAM[3]) / CAM[1]))])


def _reproj(first):
    """the second observation 6 px off its epipolar line; the side that is not
    to fail has octave 7's sigma2"""
    v1, v2, a, b = _clean()
    _, sig = scale_tables()
    a, b = list(a), list(b)
    b[1] += 6.0
    (b if first else a)[6] = sig[7]
    return _problem(v1, v2, [(tuple(a), tuple(b))])


def _zero_distance():
    """orbx_tri_view carries Ow beside Tcw: the neighbour's set to the point itself"""
    v1, v2, a, b = _clean()
    P = _problem(v1, v2, [(a, b)])
    X, status, _ = ref.pair(v1[0], v2[0], RF, P["pairs"]["o1"][0], P["pairs"]["o2"][0])
    assert status == 0
    v2 = v2.copy()
    v2["Ow"][0] = X
    return dict(P, v2=v2)


def _scale_ratio():
    v1, v2, a, b = _clean()
    s, _ = scale_tables()
    a = list(a)
    a[7] = s[7]
    return _problem(v1, v2, [(tuple(a), b)])


def _stereo2():
    """stereo on side 2 only and a baseline of a centimetre: side 2's unprojection"""
    v1, v2, a, b = _clean(X=(0.3, -0.2, 6.0), st2=True, baseline=0.01)
    return _problem(v1, v2, [(a, b)])


def _both_stereo():
    """Both sides stereo, a centimetre apart.  Side 2's depth is made a tenth of
    a metre: its cosine, were it computed, would be far the smaller and the
    point would be side 2's.  It is not: cs2 stays cosRays + 1."""
    v1, v2, a, b = _clean(X=(0.3, -0.2, 6.0), st1=True, st2=True, baseline=0.01)
    b = list(b)
    b[3] = 0.1
    return _problem(v1, v2, [(a, tuple(b))])


def _cos_negative():
    R2 = _rot(np.array([0.0, np.deg2rad(100.0), 0.0]))
    v1, v2, _, _ = _two(R2=R2)
    return _problem(v1, v2, [(_xn(0.0, 0.0), _xn(0.0, 0.0)), (_xn(0.1, 0.05), _xn(-0.1, 0.0))])


def _reproj_edge(kept):
    def make():
        v1, v2, a, b = _clean()
        a = list(a)
        a[1] += 3.0   # off the (horizontal) epipolar line: an error of a pixel or two on side 1
        P = _problem(v1, v2, [(tuple(a), b)])
        P["pairs"]["o1"]["sigma2"][0] = 100.0
        _, _, d = ref.pair(v1[0], v2[0], RF, P["pairs"]["o1"][0], P["pairs"]["o2"][0])
        e = np.float64(d["err1"])
        assert e > 0.5
        s = np.float32(e / 5.991)
        while np.float64(5.991) * np.float64(s) < e:
            s = np.nextafter(s, np.float32(np.inf))
        while np.float64(5.991) * np.float64(np.nextafter(s, np.float32(0))) >= e:
            s = np.nextafter(s, np.float32(0))
        P["pairs"]["o1"]["sigma2"][0] = s if kept else np.nextafter(s, np.float32(0))
        P["edge_err"] = np.float32(e)
        return P
    return make


def _mbf_slip():
    """Two stereo keyframes with different mbf, side 2 stereo: its right
    coordinate was formed with its own mbf, the test uses the current
    keyframe's (:454)."""
    v1, v2, a, b = _clean(st2=True, mbf1=40.0, mbf2=60.0)
    return _problem(v1, v2, [(a, b)])


def _identical_rays():
    v1 = make_view(I3, Z3, CAM)
    return _problem(v1, v1.copy(), [(_xn(0.1, 0.05), _xn(0.1, 0.05))])


def _near_rank2():
    """side 1 stereo with a depth that makes its cosine 1.0f, the rays 4e-4 rad
    apart: cosRays is one ulp under 1 and the pair is triangulated"""
    v1, v2, _, _ = _two(baseline=0.004)
    a = list(_obs(I3, Z3, (1.0, 0.5, 10.0), stereo=True))
    a[3] = 4000.0
    return _problem(v1, v2, [(tuple(a), _obs(I3, np.array([-0.004, 0.0, 0.0]), (1.0, 0.5, 10.0)))])


def _nan():
    """tcw1's first entry NaN: the rays are untouched, A's fourth column is not"""
    v1, v2, a, b = _clean()
    v1 = v1.copy()
    v1["Tcw"][0][3] = np.nan
    return _problem(v1, v2, [(a, b)])


def _many_sweeps():
    P = make_triangulation_problem(6, seed=77, noise_px=0.5)
    return {k: P[k] for k in ("v1", "v2", "ratio_factor", "pairs")}


RANK2_A = np.array([[-1, 0, 0.125, 0.5], [0, -1, 0.25, -0.25], [-1, 0, 0.125, 0.5], [0, -1, 0.25, -0.25]], np.float32)

# name -> (constructor, the statuses it must produce, in pair order; None: any)
SPECIAL = {
    "low-parallax": (_low_parallax, [1]),
    "parallax-edge": (_parallax_edge, [0, 1]),
    "w-zero": (_w_zero, [2]),
    "behind-first": (_behind_first, [3]),
    "first-sweep": (_first_sweep, [3]),
    "stereo1-behind-second": (_stereo1_behind_second, [4]),
    "reproj-first": (lambda: _reproj(True), [5]),
    "reproj-second": (lambda: _reproj(False), [6]),
    "zero-distance": (_zero_distance, [7]),
    "scale-ratio": (_scale_ratio, [8]),
    "stereo2": (_stereo2, [0]),
    "both-stereo": (_both_stereo, [0]),
    "cos-negative": (_cos_negative, [1, 1]),
    "reproj-edge-kept": (_reproj_edge(True), [0]),
    "reproj-edge-rejected": (_reproj_edge(False), [5]),
    "mbf-slip": (_mbf_slip, [6]),
    "identical-rays": (_identical_rays, [1]),
    "near-rank-2": (_near_rank2, None),
    "many-sweeps": (_many_sweeps, None),
    "nan": (_nan, [0]),
}


@functools.lru_cache(maxsize=None)
def problem(name):
    """dict with v1, v2 (1,), ratio_factor, pairs (n,) (shared; do not modify)"""
    if isinstance(name, tuple):
        n, kind = name
        return make_triangulation_problem(n, seed=500 + n + 7 * list(KINDS).index(kind), stereo_frac=KINDS[kind],
                                          outlier_frac=0.2 if n > 1 else 0.0, noise_px=0.5)
    return SPECIAL[name][0]()


@functools.lru_cache(maxsize=None)
def reference(name):
    """(points, debug dicts) of pyref_triangulate over the case's pairs (shared; do not modify)"""
    P = problem(name)
    return ref.triangulate(P["v1"], P["v2"], P["ratio_factor"], P["pairs"], debug=True)


ALL = SIZE_CASES + tuple(SPECIAL)


def case_id(name):
    return f"{name[0]}-{name[1]}" if isinstance(name, tuple) else name


def canon(points):
    """the records as uint32 words, every NaN the same NaN"""
    f = np.frombuffer(np.ascontiguousarray(points).tobytes(), np.uint32).reshape(len(points), 4).copy()
    v = f[:, :3].view(np.float32)
    f[:, :3][np.isnan(v)] = 0x7fc00000
    return f


def assert_same(got, want, what=""):
    a, b = canon(got), canon(want)
    assert a.shape == b.shape, (what, a.shape, b.shape)
    bad = np.nonzero((a != b).any(1))[0]
    assert len(bad) == 0, (what, len(bad), bad[:5], got[bad[:3]], want[bad[:3]])


def batch(names_or_none):
    """One CSR batch of the named cases' problems (None: an empty problem with
    views of its own): (v1, v2, ratio_factor, pairs, offsets)"""
    Ps = [problem(nm) if nm is not None else dict(problem("scale-ratio"), pairs=np.zeros(0, ref.PAIR_DTYPE))
          for nm in names_or_none]
    off = np.concatenate([[0], np.cumsum([len(P["pairs"]) for P in Ps])]).astype(np.int32)
    return (np.concatenate([P["v1"] for P in Ps]), np.concatenate([P["v2"] for P in Ps]),
            np.array([P["ratio_factor"] for P in Ps], np.float32), np.concatenate([P["pairs"] for P in Ps]), off)
