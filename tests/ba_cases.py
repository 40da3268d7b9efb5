"""The bundle-adjustment problems of test_ba_reference.py and
test_gpu_ba_reference.py, and their dense references (pyref_ba), computed
once per process and shared.  Every problem comes from make_ba_problem, whose
first local keyframe is fixed: nf = n_local - 1 free cameras."""
from __future__ import annotations

import functools

import numpy as np

import pyref_ba
from orb_slam_2_ros_amd.synth_ba import make_ba_problem

# name: (n_local, n_fixed, n_points, stereo_frac) -- what the shape reaches
STEP_SHAPES = {
    "tiny": (3, 2, 40, 0.5),          # nf = 2, 12 pose unknowns
    "tile-30": (6, 2, 60, 0.5),       # 6 nf = 30 / 36: across the first 32-column tile of W
    "tile-36": (7, 2, 60, 0.5),
    "tile2-60": (11, 3, 60, 0.5),     # 6 nf = 60 / 66: across the next
    "tile2-66": (12, 3, 60, 0.5),
    "chunk-510": (12, 3, 170, 0.0),   # 3 npt = 510 / 513: one / two 512-row Schur chunks; mono only
    "chunk-513": (12, 3, 171, 0.0),
    "chol-126": (22, 2, 120, 1.0),    # 126 / 132 pose unknowns: the LDS or fast Cholesky / the global one; stereo only
    "chol-132": (23, 2, 120, 1.0),
    "words-64": (65, 2, 100, 0.5),    # nf = 64 / 65: the second 64-bit word of make_pairs' camera masks
    "words-65": (66, 2, 100, 0.5),
    "words2-129": (130, 2, 120, 0.5), # nf = 129: the third word
    "max-170": (171, 2, 120, 0.5),    # nf = 170, 1020 pose unknowns: the API's limit
}
STEP_CASES = list(STEP_SHAPES) + ["degenerate", "degenerate-unique"]
STEP_MODES = [(True, 1e-3), (False, 10.0)]
STEP_SEED = 11

# name: (n_local, n_fixed, n_points, seed, stereo_frac)
FULL_SHAPES = {
    "full-3": (3, 2, 40, 1, 0.5),
    "full-5-mono": (5, 2, 50, 8, 0.0),
    "full-7": (7, 3, 60, 2, 0.5),
    "full-6-stereo": (6, 2, 64, 3, 1.0),
}
FULL_CASES = list(FULL_SHAPES) + ["degenerate", "degenerate-unique", "behind"]


def degenerate_problem(repeat=True):
    """(5, 2, 50) edited: point 0 keeps one edge, made mono (a rank-2 point
    block); point 1 has no edge; free camera 6 (the last) has no edge; one
    (camera, point) observation is repeated (no point maps: the merge walk).
    repeat=False leaves the repetition out ("degenerate-unique"): the fast
    mode then keeps its dense Schur product, which a repeated observation
    turns off, and meets the other three edits there."""
    P = make_ba_problem(n_local=5, n_fixed=2, n_points=50, seed=5)
    E = P["edges"]
    free = P["fixed"] == 0
    E = E[(E["cam"] != 6) & (E["point"] != 1)]
    p0 = np.nonzero(E["point"] == 0)[0]
    on_free = [i for i in p0 if free[E["cam"][i]]]
    keep0 = on_free[0] if on_free else p0[0]
    E = E[(E["point"] != 0) | (np.arange(len(E)) == keep0)].copy()
    E["ur"][E["point"] == 0] = -1.0
    rep = np.nonzero(free[E["cam"]] & (E["point"] >= 2))[0][3]
    P["edges"] = np.concatenate([E, E[rep:rep + 1]]) if repeat else E
    assert (P["edges"]["point"] == 0).sum() == 1 and not (P["edges"]["point"] == 1).any()
    assert free[6] and not (P["edges"]["cam"] == 6).any()
    return P


def behind_problem():
    """(4, 2, 40) plus one point behind every camera, seen by one stereo edge
    of a free camera whose observation is the point's own projection at the
    initial estimate: chi2 ~ 0, only the depth test can flag it."""
    P = make_ba_problem(n_local=4, n_fixed=2, n_points=40, seed=4)
    cam = 4
    assert P["fixed"][cam] == 0
    X = np.concatenate([P["Xw"], np.array([[1.5, -0.5, -12.0]], np.float32)])
    R, t = pyref_ba.poses_in(P["Tcw"])
    e = P["edges"][:1].copy()
    e["cam"], e["point"], e["inv_sigma2"] = cam, len(X) - 1, 1.0
    p = R[cam] @ X[-1].astype(np.float64) + t[cam]
    assert p[2] < -5
    u = float(e["fx"][0]) * p[0] / p[2] + float(e["cx"][0])
    e["u"], e["v"] = u, float(e["fy"][0]) * p[1] / p[2] + float(e["cy"][0])
    e["ur"] = u - float(e["bf"][0]) / p[2]
    assert e["ur"][0] >= 0                               # (a stereo edge)
    P["Xw"] = X
    P["edges"] = np.concatenate([P["edges"], e])
    return P


@functools.lru_cache(maxsize=None)
def problem(name):
    if name.startswith("degenerate"):
        return degenerate_problem(repeat=name == "degenerate")
    if name == "behind":
        return behind_problem()
    if name in STEP_SHAPES:
        nl, nfx, npt, sf = STEP_SHAPES[name]
        return make_ba_problem(n_local=nl, n_fixed=nfx, n_points=npt, seed=STEP_SEED, stereo_frac=sf)
    nl, nfx, npt, seed, sf = FULL_SHAPES[name]
    return make_ba_problem(n_local=nl, n_fixed=nfx, n_points=npt, seed=seed, stereo_frac=sf)


def n_unknowns(P):
    return 6 * int((P["fixed"] == 0).sum()) + 3 * len(P["Xw"])


@functools.lru_cache(maxsize=None)
def step_reference(name, robust):
    """(H, b, rho0_sum) of the case's first linearisation, every edge active.
    Read-only: shared by every test of the case."""
    P = problem(name)
    H, b, s = pyref_ba.ba_dense_system(P["Tcw"], P["fixed"], P["Xw"], P["edges"], np.ones(len(P["edges"]), bool),
                                       robust)
    H.setflags(write=False)
    b.setflags(write=False)
    return H, b, s


@functools.lru_cache(maxsize=None)
def step_condition(name, robust, lam):
    H, _, _ = step_reference(name, robust)
    return float(np.linalg.cond(H.astype(np.float64) + lam * np.eye(len(H))))


@functools.lru_cache(maxsize=None)
def full_reference(name):
    P = problem(name)
    return pyref_ba.local_ba_ref(P["Tcw"], P["fixed"], P["Xw"], P["edges"], details=True)


def step_bound(P):
    """The backward-error bound of a step: m 2^-53 (c n eps, c = 1)."""
    return n_unknowns(P) * 2.0 ** -53


def ulps32(a, b):
    """max |a - b| in float32 ulps of the arrays' largest magnitude."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / np.spacing(np.float32(np.abs(b).max())))
