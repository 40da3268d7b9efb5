"""Sim3Solver problems shared by test_sim3solver_reference.py and
test_sim3solver_host_text.py (CPU), test_gpu_sim3solver.py and
test_sim3solver_forwarder.py, and their pyref_sim3solver results, computed
once per session.

SIZES are the kernel's chunk edges (a wave takes the correspondences 64 at a
time: the minimum of three, a part chunk, one short of a chunk, exactly one,
one over, two and a remainder); HYPS the workgroup edges (one workgroup forms
64 hypotheses: one, one short, exactly 64, one over, the reference's 300).
Every size case carries 300 triples; a run with h hypotheses uses the first h,
so one reference per (n, fix) serves all five."""
from __future__ import annotations

import functools

import numpy as np

import pyref_sim3solver as ref
from orb_slam_2_ros_amd.sim3solver import draw_triples
from orb_slam_2_ros_amd.synth_sim3solver import make_sim3solver_problem

SIZES = (3, 20, 63, 64, 65, 130)
HYPS = (1, 63, 64, 65, 300)
FIX = (False, True)


def _triples(n, count, seed):
    rng = np.random.default_rng(seed)
    return draw_triples(n, count, lambda lo, hi: int(rng.integers(lo, hi + 1)))


def _nan(P):
    """the first triple's camera-1 points identical and on the optical axis: Pr1 = 0, so N is exactly diagonal (zero)"""
    P["corr"]["X1c"][:3] = np.array([0, 0, 4], np.float32)
    P["triples"][0] = (0, 1, 2)
    return P


def _collinear(P):
    """the first triple's points on one line in both cameras"""
    for k in range(3):
        P["corr"]["X1c"][k] = np.array([0.5 + 0.25 * k, -0.25 + 0.5 * k, 4 + k], np.float32)
        P["corr"]["X2c"][k] = np.array([-0.5 + 0.5 * k, 0.25 * k, 5 + 0.5 * k], np.float32)
    P["triples"][0] = (0, 1, 2)
    return P


def _z0(P):
    """correspondence 5 in camera 1's plane z = 0, correspondence 6 in camera 2's"""
    P["corr"]["X1c"][5][2] = 0.0
    P["corr"]["X2c"][6][2] = 0.0
    P["triples"][1] = (5, 6, 7)   # and a hypothesis sampled from them
    return P


EDGE_HYP, EDGE_CORR = 0, 11


def _edge(inside):
    def edit(P):
        """correspondence 11's max_err1 is hypothesis 0's err1 itself (strictly
        less fails: outlier) or the next float above it (inlier)"""
        d = {}
        ref.hypothesis(P["cam1"][0], P["cam2"][0], P["fix_scale"], P["corr"], P["triples"][EDGE_HYP], d)
        e1, e2 = ref.errors(d["T12"], d["T21"], P["corr"], P["cam1"][0], P["cam2"][0])
        P["corr"]["max_err1"][EDGE_CORR] = np.nextafter(e1[EDGE_CORR], np.float32(np.inf)) if inside else e1[EDGE_CORR]
        P["edge_err"] = (e1[EDGE_CORR], e2[EDGE_CORR])
        return P
    return edit


# name -> (make_sim3solver_problem arguments, hypotheses, edit)
SPECIAL = {
    "nan": (dict(n=20, seed=21), 64, _nan),
    "collinear": (dict(n=20, seed=22), 64, _collinear),
    "z0": (dict(n=40, seed=23), 64, _z0),
    "edge-out": (dict(n=30, seed=24, noise_m=0.004), 8, _edge(False)),
    "edge-in": (dict(n=30, seed=24, noise_m=0.004), 8, _edge(True)),
    "fix-scale": (dict(n=40, seed=25, scale=1.3, fix_scale=True), 64, None),
    "large-rotation": (dict(n=40, seed=26, rot_sigma=2.0, scale=0.7), 64, None),
    "recovery": (dict(n=60, seed=27, outlier_frac=0.4, scale=1.2), 100, None),
}


@functools.lru_cache(maxsize=None)
def problem(name):
    """dict of make_sim3solver_problem plus triples (h, 3) int32 (shared; do not modify)"""
    if isinstance(name, tuple):
        n, fix = name
        P = make_sim3solver_problem(n, seed=200 + n, fix_scale=fix, outlier_frac=0.2 if n >= 20 else 0.0,
                                    noise_m=0.002, scale=1.0 if fix else 1.1)
        P["triples"] = _triples(n, max(HYPS), 300 + n)
        return P
    kw, h, edit = SPECIAL[name]
    P = make_sim3solver_problem(**kw)
    P["triples"] = _triples(kw["n"], h, 400 + kw["seed"])
    return edit(P) if edit else P


@functools.lru_cache(maxsize=None)
def reference(name):
    """(hyp, mask, details) of pyref_sim3solver.ransac over all the case's triples (shared; do not modify)"""
    P = problem(name)
    details = []
    hyp, mask = ref.ransac(P["cam1"], P["cam2"], P["fix_scale"], P["corr"], P["triples"], details)
    return hyp, mask, details


SIZE_CASES = tuple((n, f) for n in SIZES for f in FIX)
ALL = SIZE_CASES + tuple(SPECIAL)


def case_id(name):
    return f"{name[0]}-{'fixed' if name[1] else 'free'}" if isinstance(name, tuple) else name
