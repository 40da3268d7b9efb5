"""ctypes wrapper of oracle/liborbx_oracle.so -- the CPU restatement.

TEST INFRASTRUCTURE ONLY (see orbx_oracle.h).  Imported by tests/,
__graft_entry__.smoke() and bench.py's cpu_baseline leg; never by the product
package.  Parity vs the reference binary: unpinned.
"""
from __future__ import annotations

import ctypes
import subprocess
from pathlib import Path

import numpy as np

HERE = Path(__file__).resolve().parent
LIB_PATH = HERE / "liborbx_oracle.so"

KEYPOINT_DTYPE = np.dtype([
    ("x", "<f4"), ("y", "<f4"), ("size", "<f4"), ("angle", "<f4"),
    ("response", "<f4"), ("octave", "<i4"), ("class_id", "<i4"),
])

P = ctypes.c_void_p
I32 = ctypes.c_int
F32 = ctypes.c_float
SZ = ctypes.c_size_t

_SIG = {
    "orbo_cv_round": (I32, [F32]),
    "orbo_fast_atan2": (F32, [F32, F32]),
    "orbo_sincosf": (None, [F32, P, P]),
    "orbo_descriptor_distance": (I32, [P, P]),
    "orbo_resize_linear": (None, [P, I32, I32, SZ, P, I32, I32, SZ]),
    "orbo_gauss7": (None, [P, I32, I32, SZ, P, SZ]),
    "orbo_fast": (I32, [P, I32, I32, SZ, I32, P, I32]),
    "orbo_levels": (None, [I32, I32, I32, F32, I32, P, P, P, P]),
    "orbo_pyramid": (SZ, [P, I32, I32, SZ, F32, I32, P]),
    "orbo_level_candidates": (I32, [P, I32, I32, I32, I32, P, I32]),
    "orbo_level_candidates_cells": (I32, [P, I32, I32, I32, I32, P, I32, P, I32, P]),
    "orbo_level_cells": (I32, [I32, I32, P, I32]),
    "orbo_distribute": (I32, [P, I32, I32, I32, I32, P]),
    "orbo_extract": (I32, [P, I32, I32, SZ, I32, F32, I32, I32, I32, P, P, I32, P]),
    "orbo_search_for_initialization": (I32, [P, P, I32, P, P, I32, I32, I32, P, P, I32, F32, I32]),
    "orbo_search_for_initialization_bounds": (I32, [P, P, I32, P, P, I32, F32, F32, F32, F32, P, P, I32, F32, I32]),
    "orbo_compute_stereo_matches": (I32, [P, P, P, P, I32, P, P, P, P, I32, P, P, I32, F32, F32, P, P]),
    "orbo_stereo_from_rgbd": (None, [P, P, I32, P, I32, I32, SZ, F32, P, P]),
}

_lib = None


def build() -> Path:
    subprocess.run(["make", "-s", "-C", str(HERE)], check=True)
    return LIB_PATH


def lib() -> ctypes.CDLL:
    global _lib
    if _lib is None:
        if not LIB_PATH.exists():
            build()
        _lib = _bind(LIB_PATH)
    return _lib


def _bind(path: Path) -> ctypes.CDLL:
    l = ctypes.CDLL(str(path))
    for name, (res, args) in _SIG.items():
        f = getattr(l, name)
        f.restype = res
        f.argtypes = args
    return l


def use_timing_build(timeout_s: float = 240.0) -> str:
    """Switch this process to the oracle's timing build (bench.py's
    cpu_baseline leg; SURVEY.md §8(d): -O3 -march=native).  The native build is
    compiled on the host that runs the bench (`make native`, so -march=native
    means that host); if that fails, the portable -O3 -march=x86-64-v3 build
    shipped in-tree is used.  Both keep -ffp-contract=off and no fast-math, so
    results are identical to the checker build.  Returns a description;
    use_checker_build() switches back."""
    global _lib
    desc = None
    try:
        r = subprocess.run(["make", "-s", "-C", str(HERE), "native"], timeout=timeout_s, capture_output=True)
        if r.returncode == 0 and (HERE / "_timing" / "liborbx_oracle_native.so").exists():
            _lib = _bind(HERE / "_timing" / "liborbx_oracle_native.so")
            desc = "g++ -O3 -march=native -ffp-contract=off (built on this host)"
    except (OSError, subprocess.TimeoutExpired):
        pass
    if desc is None:
        p = HERE / "liborbx_oracle_v3.so"
        if not p.exists():
            subprocess.run(["make", "-s", "-C", str(HERE), "liborbx_oracle_v3.so"], check=True)
        _lib = _bind(p)
        desc = "g++ -O3 -march=x86-64-v3 -ffp-contract=off (prebuilt; native build unavailable)"
    return desc


def use_checker_build() -> None:
    global _lib
    _lib = None


def _p(a):
    return ctypes.c_void_p(a.ctypes.data)


def levels(w, h, nfeatures=1000, scale=1.2, nlevels=8):
    lw = np.zeros(nlevels, np.int32); lh = np.zeros(nlevels, np.int32)
    q = np.zeros(nlevels, np.int32); s = np.zeros(nlevels, np.float32)
    lib().orbo_levels(w, h, nfeatures, scale, nlevels, _p(lw), _p(lh), _p(q), _p(s))
    return lw, lh, q, s


def pyramid(img: np.ndarray, scale=1.2, nlevels=8):
    img = np.ascontiguousarray(img)
    h, w = img.shape
    lw, lh, _, _ = levels(w, h, 1000, scale, nlevels)
    total = int((lw.astype(np.int64) * lh).sum())
    out = np.zeros(total, np.uint8)
    lib().orbo_pyramid(_p(img), w, h, img.strides[0], scale, nlevels, _p(out))
    res, off = [], 0
    for l in range(nlevels):
        n = int(lw[l]) * int(lh[l])
        res.append(out[off:off + n].reshape(lh[l], lw[l]))
        off += n
    return res


def resize_linear(src: np.ndarray, dw: int, dh: int) -> np.ndarray:
    src = np.ascontiguousarray(src)
    out = np.zeros((dh, dw), np.uint8)
    lib().orbo_resize_linear(_p(src), src.shape[1], src.shape[0], src.strides[0], _p(out), dw, dh, dw)
    return out


def gauss7(img: np.ndarray) -> np.ndarray:
    img = np.ascontiguousarray(img)
    out = np.zeros_like(img)
    lib().orbo_gauss7(_p(img), img.shape[1], img.shape[0], img.strides[0], _p(out), img.shape[1])
    return out


def fast(img: np.ndarray, threshold: int) -> np.ndarray:
    img = np.ascontiguousarray(img)
    cap = img.size
    out = np.zeros(3 * max(cap, 1), np.int32)
    n = lib().orbo_fast(_p(img), img.shape[1], img.shape[0], img.strides[0], threshold, _p(out), cap)
    return out[:3 * n].reshape(n, 3)


def level_candidates(lvl: np.ndarray, ini=20, mn=7) -> np.ndarray:
    lvl = np.ascontiguousarray(lvl)
    cap = lvl.size
    out = np.zeros(3 * cap, np.int32)
    n = lib().orbo_level_candidates(_p(lvl), lvl.shape[1], lvl.shape[0], ini, mn, _p(out), cap)
    assert n >= 0
    return out[:3 * n].reshape(n, 3)


def level_candidates_cells(lvl: np.ndarray, ini=20, mn=7):
    """(candidates, per-cell corner counts in the reference's cell order)."""
    lvl = np.ascontiguousarray(lvl)
    cap = lvl.size
    out = np.zeros(3 * cap, np.int32)
    cells = np.zeros(65536, np.int32)
    nc = ctypes.c_int(0)
    n = lib().orbo_level_candidates_cells(_p(lvl), lvl.shape[1], lvl.shape[0], ini, mn, _p(out), cap, _p(cells),
                                          len(cells), ctypes.byref(nc))
    assert n >= 0
    return out[:3 * n].reshape(n, 3), cells[:nc.value].copy()


def level_cells(w: int, h: int) -> np.ndarray:
    """The (x0, y0, x1, y1) windows FAST runs on for a w x h level, in cell
    order; a window's evaluated interior is 3 px inside it."""
    out = np.zeros((20000, 4), np.int32)   # 135 x 135 cells at 4095 x 4095
    n = lib().orbo_level_cells(int(w), int(h), _p(out), len(out))
    assert n >= 0
    return out[:n].copy()


def distribute(cands: np.ndarray, w: int, h: int, N: int) -> np.ndarray:
    c = np.ascontiguousarray(cands, dtype=np.int32)
    sel = np.zeros(max(len(c), 1) + 8, np.int32)
    n = lib().orbo_distribute(_p(c), len(c), w, h, N, _p(sel))
    return sel[:n].copy()


def extract(img: np.ndarray, nfeatures=1000, scale=1.2, nlevels=8, ini=20, mn=7):
    img = np.ascontiguousarray(img, dtype=np.uint8)
    h, w = img.shape
    cap = nfeatures + 16 * nlevels + 64
    kps = np.zeros(cap, KEYPOINT_DTYPE)
    desc = np.zeros((cap, 32), np.uint8)
    n = ctypes.c_int(0)
    rc = lib().orbo_extract(_p(img), w, h, img.strides[0], nfeatures, scale, nlevels, ini, mn,
                            _p(kps), _p(desc), cap, ctypes.byref(n))
    if rc != 0:
        raise RuntimeError(f"oracle extract failed ({rc}, n={n.value})")
    return kps[:n.value].copy(), desc[:n.value].copy()


def search_for_initialization(k1, d1, k2, d2, w, h, prev_xy, window=100, nnratio=0.9, check_ori=True,
                              bounds=None):
    """bounds: (mnMinX, mnMaxX, mnMinY, mnMaxY); None = (0, w, 0, h)."""
    k1 = np.ascontiguousarray(k1, KEYPOINT_DTYPE); k2 = np.ascontiguousarray(k2, KEYPOINT_DTYPE)
    d1 = np.ascontiguousarray(d1, np.uint8); d2 = np.ascontiguousarray(d2, np.uint8)
    prev = np.ascontiguousarray(prev_xy, np.float32).copy()
    m12 = np.full(max(len(k1), 1), -1, np.int32)
    if bounds is None:
        nm = lib().orbo_search_for_initialization(_p(k1), _p(d1), len(k1), _p(k2), _p(d2), len(k2), w, h,
                                                  _p(prev), _p(m12), window, nnratio, int(check_ori))
    else:
        nm = lib().orbo_search_for_initialization_bounds(_p(k1), _p(d1), len(k1), _p(k2), _p(d2), len(k2),
                                                         *[float(b) for b in bounds], _p(prev), _p(m12), window,
                                                         nnratio, int(check_ori))
    return nm, m12[:len(k1)].copy(), prev


def fast_atan2(y: float, x: float) -> float:
    return float(lib().orbo_fast_atan2(y, x))


def cv_round(v: float) -> int:
    return int(lib().orbo_cv_round(v))


def sincosf(a: float):
    s, c = ctypes.c_float(0), ctypes.c_float(0)
    lib().orbo_sincosf(a, ctypes.byref(s), ctypes.byref(c))
    return s.value, c.value


def descriptor_distance(a, b) -> int:
    a = np.ascontiguousarray(a, np.uint8); b = np.ascontiguousarray(b, np.uint8)
    return int(lib().orbo_descriptor_distance(_p(a), _p(b)))


def scale_tables(scale=1.2, nlevels=8):
    """mvScaleFactor / mvInvScaleFactor (ORBextractor.cc:424-438): float
    products computed in double (member scaleFactor is a double)."""
    sf = np.zeros(nlevels, np.float32)
    sf[0] = 1.0
    for i in range(1, nlevels):
        sf[i] = np.float32(float(sf[i - 1]) * float(np.float32(scale)))
    inv = (np.float32(1.0) / sf).astype(np.float32)
    return sf, inv


def compute_stereo_matches(pyr_l, pyr_r, kl, dl, kr, dr, mbf, mb, scale=1.2):
    """Frame::ComputeStereoMatches on oracle pyramids (lists of levels).
    Returns (uright, depth, kept)."""
    nlev = len(pyr_l)
    lw = np.array([p.shape[1] for p in pyr_l], np.int32)
    lh = np.array([p.shape[0] for p in pyr_l], np.int32)
    bl = np.ascontiguousarray(np.concatenate([p.ravel() for p in pyr_l]))
    br = np.ascontiguousarray(np.concatenate([p.ravel() for p in pyr_r]))
    sf, inv = scale_tables(scale, nlev)
    kl = np.ascontiguousarray(kl, KEYPOINT_DTYPE); kr = np.ascontiguousarray(kr, KEYPOINT_DTYPE)
    dl = np.ascontiguousarray(dl, np.uint8); dr = np.ascontiguousarray(dr, np.uint8)
    ur = np.zeros(max(len(kl), 1), np.float32)
    dp = np.zeros(max(len(kl), 1), np.float32)
    kept = lib().orbo_compute_stereo_matches(_p(bl), _p(br), _p(lw), _p(lh), nlev, _p(sf), _p(inv),
                                             _p(kl), _p(dl), len(kl), _p(kr), _p(dr), len(kr),
                                             mbf, mb, _p(ur), _p(dp))
    return ur[:len(kl)].copy(), dp[:len(kl)].copy(), kept


def stereo_from_rgbd(kps, dmap, mbf, kps_un=None):
    """Frame::ComputeStereoFromRGBD; dmap is float32 (h, w)."""
    kps = np.ascontiguousarray(kps, KEYPOINT_DTYPE)
    kun = kps if kps_un is None else np.ascontiguousarray(kps_un, KEYPOINT_DTYPE)
    dmap = np.ascontiguousarray(dmap, np.float32)
    ur = np.zeros(max(len(kps), 1), np.float32)
    dp = np.zeros(max(len(kps), 1), np.float32)
    lib().orbo_stereo_from_rgbd(_p(kps), _p(kun), len(kps), _p(dmap), dmap.shape[1], dmap.shape[0],
                                dmap.strides[0], mbf, _p(ur), _p(dp))
    return ur[:len(kps)].copy(), dp[:len(kps)].copy()


PROJ_QUERY_DTYPE = np.dtype([
    ("u", "<f4"), ("v", "<f4"), ("radius", "<f4"), ("ur", "<f4"), ("ur_tol", "<f4"),
    ("min_level", "<i4"), ("max_level", "<i4"), ("angle", "<f4"), ("flags", "<i4"),
])
PROJ_VARIANTS = {"localmap": 0, "lastframe": 1, "keyframe": 2, "sim3": 3, "fuse": 4, "fuse_sim3": 5}


def search_by_projection(variant, keys, desc, queries, qdesc, bounds, uright=None, mp_state=None,
                         inv_sigma2=None, th_dist=100, nnratio=0.6, check_ori=True):
    """ORBmatcher::SearchByProjection x4 / Fuse x2 (search part) on a query
    table.  Returns (nmatches, q_idx, q_dist, kp_final)."""
    lib().orbo_search_by_projection.restype = I32
    lib().orbo_search_by_projection.argtypes = [I32, P, P, P, P, P, I32, F32, F32, F32, F32, P, P, I32, I32,
                                                F32, I32, P, P, P]
    keys = np.ascontiguousarray(keys, KEYPOINT_DTYPE)
    desc = np.ascontiguousarray(desc, np.uint8).reshape(-1, 32)
    q = np.ascontiguousarray(queries, PROJ_QUERY_DTYPE)
    qd = np.ascontiguousarray(qdesc, np.uint8).reshape(-1, 32)
    ur = None if uright is None else np.ascontiguousarray(uright, np.float32)
    ms = None if mp_state is None else np.ascontiguousarray(mp_state, np.uint8)
    isg = None if inv_sigma2 is None else np.ascontiguousarray(inv_sigma2, np.float32)
    qi = np.full(max(len(q), 1), -1, np.int32)
    qdist = np.full(max(len(q), 1), -1, np.int32)
    kf = np.full(max(len(keys), 1), -1, np.int32)
    v = PROJ_VARIANTS[variant] if isinstance(variant, str) else int(variant)
    if v == PROJ_VARIANTS["fuse"] and len(keys) and (isg is None or keys["octave"].min() < 0
                                                      or keys["octave"].max() >= len(isg)):
        # Fuse indexes invSigma2 by the keypoint's octave (ORBmatcher.cc:905-930) and the entry carries no length
        raise ValueError("fuse: a keypoint octave outside inv_sigma2")
    nm = lib().orbo_search_by_projection(v, _p(keys), _p(desc), None if ur is None else _p(ur),
                                         None if ms is None else _p(ms), None if isg is None else _p(isg),
                                         len(keys), *[float(b) for b in bounds], _p(q), _p(qd), len(q),
                                         int(th_dist), float(nnratio), int(check_ori), _p(qi), _p(qdist), _p(kf))
    return nm, qi[:len(q)].copy(), qdist[:len(q)].copy(), kf[:len(keys)].copy()


BOW_VARIANTS = {"kf_frame": 0, "kf_kf": 1, "triangulation": 2}


def search_by_bow(variant, A, B, nnratio=0.6, check_ori=True, tri=None, nlevels=8):
    """SearchByBoW(KF, F) / SearchByBoW(KF1, KF2) / SearchForTriangulation.
    A, B: dicts with keys, desc, flags (u8), ids (u32, ascending), off (i32),
    feat (i32).  Returns (nmatches, match_a, match_b)."""
    f = lib().orbo_search_by_bow
    f.restype = I32
    f.argtypes = [I32, P, P, P, I32, P, P, P, I32, P, P, P, I32, P, P, P, I32, F32, I32, P, I32, P, P]

    def side(S):
        return (np.ascontiguousarray(S["keys"], KEYPOINT_DTYPE), np.ascontiguousarray(S["desc"], np.uint8),
                np.ascontiguousarray(S["flags"], np.uint8), np.ascontiguousarray(S["ids"], np.uint32),
                np.ascontiguousarray(S["off"], np.int32), np.ascontiguousarray(S["feat"], np.int32))
    ka, da, fa, ia, oa, fea = side(A)
    kb, db, fb, ib, ob, feb = side(B)
    t = None if tri is None else np.ascontiguousarray(tri, np.float32)
    ma = np.full(max(len(ka), 1), -1, np.int32)
    mb = np.full(max(len(kb), 1), -1, np.int32)
    v = BOW_VARIANTS[variant] if isinstance(variant, str) else int(variant)
    nm = f(v, _p(ka), _p(da), _p(fa), len(ka), _p(ia), _p(oa), _p(fea), len(ia),
           _p(kb), _p(db), _p(fb), len(kb), _p(ib), _p(ob), _p(feb), len(ib),
           float(nnratio), int(check_ori), None if t is None else _p(t), int(nlevels), _p(ma), _p(mb))
    return nm, ma[:len(ka)].copy(), mb[:len(kb)].copy()


def search_by_sim3(k1, d1, b1, k2, d2, b2, q1, qd1, q2, qd2, th_dist=100):
    """SearchBySim3 on per-slot query tables; returns (nfound, matches12)."""
    f = lib().orbo_search_by_sim3
    f.restype = I32
    f.argtypes = [P, P, I32, P, P, I32] + [F32] * 8 + [P, P, P, P, I32, P]
    k1 = np.ascontiguousarray(k1, KEYPOINT_DTYPE); k2 = np.ascontiguousarray(k2, KEYPOINT_DTYPE)
    d1 = np.ascontiguousarray(d1, np.uint8); d2 = np.ascontiguousarray(d2, np.uint8)
    q1 = np.ascontiguousarray(q1, PROJ_QUERY_DTYPE); q2 = np.ascontiguousarray(q2, PROJ_QUERY_DTYPE)
    qd1 = np.ascontiguousarray(qd1, np.uint8); qd2 = np.ascontiguousarray(qd2, np.uint8)
    m = np.full(max(len(k1), 1), -1, np.int32)
    nf = f(_p(k1), _p(d1), len(k1), _p(k2), _p(d2), len(k2), *[float(x) for x in b1], *[float(x) for x in b2],
           _p(q1), _p(qd1), _p(q2), _p(qd2), int(th_dist), _p(m))
    return nf, m[:len(k1)].copy()


def vocab_transform(voc, features, levelsup=4):
    """DBoW2 TemplatedVocabulary::transform on a vocabulary dict (L, scoring,
    weighting, parent i32, is_leaf u8, desc (n,32) u8, weight f64; node 0 the
    root).  Returns (bow: dict word -> value, fv: dict node -> [features],
    per-feature (word, weight, node))."""
    f = lib().orbo_vocab_transform
    f.restype = I32
    f.argtypes = [I32, I32, I32, I32, P, P, P, P, P, I32, I32, P, P, P, P, P, P, P, P, P, P]
    par = np.ascontiguousarray(voc["parent"], np.int32)
    leaf = np.ascontiguousarray(voc["is_leaf"], np.uint8)
    desc = np.ascontiguousarray(voc["desc"], np.uint8).reshape(-1, 32)
    wt = np.ascontiguousarray(voc["weight"], np.float64)
    feats = np.ascontiguousarray(features, np.uint8).reshape(-1, 32)
    n = len(feats)
    m = max(n, 1)
    bw = np.zeros(m, np.uint32); bv = np.zeros(m, np.float64)
    fn = np.zeros(m, np.uint32); fo = np.zeros(m + 1, np.int32); ff = np.zeros(m, np.int32)
    fw = np.zeros(m, np.uint32); fwt = np.zeros(m, np.float64); fnd = np.zeros(m, np.uint32)
    nb = ctypes.c_int(0); nf = ctypes.c_int(0)
    f(int(voc["L"]), int(voc["scoring"]), int(voc["weighting"]), len(par), _p(par), _p(leaf), _p(desc), _p(wt),
      _p(feats), n, int(levelsup), _p(bw), _p(bv), ctypes.byref(nb), _p(fn), _p(fo), _p(ff), ctypes.byref(nf),
      _p(fw), _p(fwt), _p(fnd))
    bow = {int(bw[i]): float(bv[i]) for i in range(nb.value)}
    fv = {int(fn[j]): [int(x) for x in ff[fo[j]:fo[j + 1]]] for j in range(nf.value)}
    return bow, fv, (fw[:n].copy(), fwt[:n].copy(), fnd[:n].copy())


class PreparedVocab:
    """The oracle's tree built once (for timing the per-frame descent)."""

    def __init__(self, voc):
        l = lib()
        l.orbo_vocab_prepare.restype = P
        l.orbo_vocab_prepare.argtypes = [I32, P, P]
        l.orbo_vocab_release.restype = None
        l.orbo_vocab_release.argtypes = [P]
        l.orbo_vocab_transform_prepared.restype = I32
        l.orbo_vocab_transform_prepared.argtypes = [P, I32, I32, I32, P, P, P, I32, I32] + [P] * 10
        self.voc = voc
        self.par = np.ascontiguousarray(voc["parent"], np.int32)
        self.leaf = np.ascontiguousarray(voc["is_leaf"], np.uint8)
        self.desc = np.ascontiguousarray(voc["desc"], np.uint8).reshape(-1, 32)
        self.wt = np.ascontiguousarray(voc["weight"], np.float64)
        self.h = l.orbo_vocab_prepare(len(self.par), _p(self.par), _p(self.leaf))

    def transform(self, features, levelsup=4):
        feats = np.ascontiguousarray(features, np.uint8).reshape(-1, 32)
        n = len(feats)
        m = max(n, 1)
        bw = np.zeros(m, np.uint32); bv = np.zeros(m, np.float64)
        fn = np.zeros(m, np.uint32); fo = np.zeros(m + 1, np.int32); ff = np.zeros(m, np.int32)
        nb = ctypes.c_int(0); nf = ctypes.c_int(0)
        lib().orbo_vocab_transform_prepared(self.h, int(self.voc["L"]), int(self.voc["scoring"]),
                                            int(self.voc["weighting"]), _p(self.desc), _p(self.wt), _p(feats), n,
                                            int(levelsup), _p(bw), _p(bv), ctypes.byref(nb), _p(fn), _p(fo), _p(ff),
                                            ctypes.byref(nf), None, None, None)
        return nb.value, nf.value

    def __del__(self):
        try:
            lib().orbo_vocab_release(self.h)
        except Exception:
            pass


def distinctive_descriptors(desc, offsets):
    f = lib().orbo_distinctive_descriptors
    f.restype = None
    f.argtypes = [P, P, I32, P]
    desc = np.ascontiguousarray(desc, np.uint8).reshape(-1, 32)
    offsets = np.ascontiguousarray(offsets, np.int32)
    npts = len(offsets) - 1
    best = np.full(max(npts, 1), -1, np.int32)
    f(_p(desc), _p(offsets), npts, _p(best))
    return best[:npts]


def undistort_points(xy, K, dist):
    f = lib().orbo_undistort_points
    f.restype = None
    f.argtypes = [P, I32, P, P, I32, P]
    xy = np.ascontiguousarray(xy, np.float32).reshape(-1, 2)
    K = np.ascontiguousarray(K, np.float32).reshape(9)
    dist = np.ascontiguousarray(dist, np.float32).reshape(-1)
    out = np.empty_like(xy)
    f(_p(xy), len(xy), _p(K), _p(dist), len(dist), _p(out))
    return out


def cvt_gray(img, rgb=True):
    f = lib().orbo_cvt_gray
    f.restype = None
    f.argtypes = [P, I32, I32, SZ, I32, I32, P, SZ]
    img = np.ascontiguousarray(img, np.uint8)
    h, w, cn = img.shape
    out = np.empty((h, w), np.uint8)
    f(_p(img), w, h, w * cn, cn, int(bool(rgb)), _p(out), w)
    return out


def depth_to_float(d16, scale):
    f = lib().orbo_depth_to_float
    f.restype = None
    f.argtypes = [P, I32, I32, SZ, F32, P, SZ]
    d16 = np.ascontiguousarray(d16, np.uint16)
    h, w = d16.shape
    out = np.empty((h, w), np.float32)
    f(_p(d16), w, h, 2 * w, float(scale), _p(out), 4 * w)
    return out


_COVIS = ctypes.CFUNCTYPE(ctypes.c_int, ctypes.c_void_p, ctypes.c_uint64, ctypes.POINTER(ctypes.c_uint64),
                          ctypes.c_int)


class KeyFrameDB:
    """The oracle's literal KeyFrameDatabase (inverted lists, per-keyframe
    query state)."""

    def __init__(self, n_words):
        l = lib()
        l.orbo_kfdb_create.restype = P
        l.orbo_kfdb_create.argtypes = [I32]
        l.orbo_kfdb_destroy.restype = None
        l.orbo_kfdb_destroy.argtypes = [P]
        l.orbo_kfdb_add.restype = None
        l.orbo_kfdb_add.argtypes = [P, ctypes.c_uint64, P, P, I32]
        l.orbo_kfdb_erase.restype = None
        l.orbo_kfdb_erase.argtypes = [P, ctypes.c_uint64]
        l.orbo_kfdb_clear.restype = None
        l.orbo_kfdb_clear.argtypes = [P]
        l.orbo_kfdb_detect.restype = I32
        l.orbo_kfdb_detect.argtypes = [P, I32, ctypes.c_uint64, P, P, I32, P, I32, F32, _COVIS, P, P, I32]
        l.orbo_bow_score_l1.restype = ctypes.c_double
        l.orbo_bow_score_l1.argtypes = [P, P, I32, P, P, I32]
        self.h = l.orbo_kfdb_create(int(n_words))

    def add(self, kf_id, words, values):
        w = np.ascontiguousarray(words, np.uint32); v = np.ascontiguousarray(values, np.float64)
        lib().orbo_kfdb_add(self.h, int(kf_id), _p(w), _p(v), len(w))

    def erase(self, kf_id):
        lib().orbo_kfdb_erase(self.h, int(kf_id))

    def clear(self):
        lib().orbo_kfdb_clear(self.h)

    def detect(self, reloc, qid, words, values, connected, min_score, covis):
        w = np.ascontiguousarray(words, np.uint32); v = np.ascontiguousarray(values, np.float64)
        conn = np.ascontiguousarray(sorted(connected or []), np.uint64)

        def cb(_c, kf, out, cap):
            ids = list(covis(int(kf)))[:cap]
            for i, k in enumerate(ids):
                out[i] = int(k)
            return len(ids)
        fn = _COVIS(cb)
        out = np.zeros(4096, np.uint64)
        n = lib().orbo_kfdb_detect(self.h, int(reloc), int(qid), _p(w), _p(v), len(w), _p(conn), len(conn),
                                   float(min_score), fn, None, _p(out), len(out))
        return [int(x) for x in out[:n]]

    def __del__(self):
        try:
            lib().orbo_kfdb_destroy(self.h)
        except Exception:
            pass


def bow_score_l1(w1, v1, w2, v2):
    lib().orbo_bow_score_l1.restype = ctypes.c_double
    lib().orbo_bow_score_l1.argtypes = [P, P, I32, P, P, I32]
    a = np.ascontiguousarray(w1, np.uint32); b = np.ascontiguousarray(v1, np.float64)
    c = np.ascontiguousarray(w2, np.uint32); d = np.ascontiguousarray(v2, np.float64)
    return lib().orbo_bow_score_l1(_p(a), _p(b), len(a), _p(c), _p(d), len(c))


def local_ba(Tcw, fixed, Xw, edges, iters=(5, 10)):
    from orb_slam_2_ros_amd.synth_ba import BA_EDGE_DTYPE
    f = lib().orbo_local_ba
    f.restype = I32
    f.argtypes = [P, P, I32, P, I32, P, I32, I32, I32, P, P, P, P]
    T = np.ascontiguousarray(Tcw, np.float32).reshape(-1, 3, 4)
    F = np.ascontiguousarray(fixed, np.uint8)
    X = np.ascontiguousarray(Xw, np.float32).reshape(-1, 3)
    E = np.ascontiguousarray(edges, BA_EDGE_DTYPE)
    To, Xo = np.empty_like(T), np.empty_like(X)
    out = np.zeros(max(len(E), 1), np.uint8)
    its = np.zeros(2, np.int32)
    f(_p(T), _p(F), len(T), _p(X), len(X), _p(E), len(E), int(iters[0]), int(iters[1]), _p(To), _p(Xo), _p(out),
      _p(its))
    return To, Xo, out[:len(E)].astype(bool), (int(its[0]), int(its[1]))


def ba_debug_step(Tcw, fixed, Xw, edges, robust=True, lam=1e-3):
    from orb_slam_2_ros_amd.synth_ba import BA_EDGE_DTYPE
    f = lib().orbo_ba_debug_step
    f.restype = I32
    f.argtypes = [P, P, I32, P, I32, P, I32, I32, ctypes.c_double, P, P]
    T = np.ascontiguousarray(Tcw, np.float32).reshape(-1, 3, 4)
    F = np.ascontiguousarray(fixed, np.uint8)
    X = np.ascontiguousarray(Xw, np.float32).reshape(-1, 3)
    E = np.ascontiguousarray(edges, BA_EDGE_DTYPE)
    n = 6 * int((F == 0).sum()) + 3 * len(X)
    x = np.zeros(max(n, 1), np.float64)
    chi2 = ctypes.c_double(0)
    ok = f(_p(T), _p(F), len(T), _p(X), len(X), _p(E), len(E), int(robust), float(lam), _p(x), ctypes.byref(chi2))
    return x[:n], chi2.value, bool(ok)
