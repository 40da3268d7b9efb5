"""Sim3-optimisation problems shared by test_sim3_reference.py (CPU),
test_gpu_sim3.py and test_sim3_forwarder.py, and their pyref_sim3 results,
computed once per session.

SIZES are the kernel's lane-stride edges (one wave, 64 lanes, correspondence i
on lane i % 64) and the reference's own threshold of ten surviving
correspondences: nothing, one under ten, ten, nineteen and twenty (ten
survivors with about a tenth removed is the edge), one short of a full stride,
exactly one, one over, two strides and a remainder.  Each runs with the scale
free and fixed."""
from __future__ import annotations

import functools

import numpy as np

import pyref_sim3
from orb_slam_2_ros_amd.synth_sim3 import make_sim3_problem

SIZES = (0, 9, 10, 19, 20, 63, 64, 65, 130)
FIX = (False, True)


def _behind(P):
    """correspondence 5's camera-2 point placed so that the initial S12 maps it
    two metres behind camera 1; its camera-1 point stays in front of camera 2"""
    S = pyref_sim3.sim3_from(P["S12"])
    X = pyref_sim3.sim3_map(pyref_sim3.sim3_inverse(S), 0.3, -0.2, -2.0)
    P["corr"]["P2c"][5] = np.array(X, np.float32)
    return P


# name -> (make_sim3_problem arguments, edit).  Seeds chosen on the CPU so that
# pyref_sim3 alone reaches what test_sim3_reference.py asserts of each case.
SPECIAL = {
    "bad-then-10": (dict(n=80, seed=3, outlier_frac=0.1), None),
    "clean-5": (dict(n=40, seed=4, noise_px=0.3), None),
    "early-return": (dict(n=14, seed=5, outlier_frac=0.5), None),
    "rejected": (dict(n=65, seed=1, outlier_frac=0.1, sim3_error=(0.05, 0.3, 0.1)), None),
    "behind": (dict(n=40, seed=11), _behind),
    "one-sided": (dict(n=100, seed=6, outlier_frac=0.15, noise_px=0.5), None),
    "scale-2": (dict(n=60, seed=7, scale=2.0, init_scale=1.0), None),
    "fixed-scale": (dict(n=60, seed=8, scale=1.05, init_scale=1.05, fix_scale=True), None),
}


def size_case(n, fix):
    return make_sim3_problem(n, seed=100 + n, fix_scale=fix, outlier_frac=0.1)


@functools.lru_cache(maxsize=None)
def problem(name):
    if isinstance(name, tuple):
        return size_case(*name)
    kw, edit = SPECIAL[name]
    P = make_sim3_problem(**kw)
    return edit(P) if edit else P


def run_reference(P):
    return pyref_sim3.optimize_sim3(P["S12"], P["cam1"], P["cam2"], P["corr"], P["th2"], P["fix_scale"])


@functools.lru_cache(maxsize=None)
def reference(name):
    """pyref_sim3.optimize_sim3 of the case (shared; do not modify)"""
    return run_reference(problem(name))


SIZE_CASES = tuple((n, f) for n in SIZES for f in FIX)
ALL = SIZE_CASES + tuple(SPECIAL)


def case_id(name):
    return f"{name[0]}-{'fixed' if name[1] else 'free'}" if isinstance(name, tuple) else name


def trials(r):
    return [t for rd in r["rounds"] for it in rd["iterations"] for t in it["trials"]]
