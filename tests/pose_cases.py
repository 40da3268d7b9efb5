"""Pose-optimisation problems shared by test_pose_reference.py (CPU) and
test_gpu_pose.py, and their pyref_pose results, computed once per session.

SIZES are the kernel's lane-stride edges (one wave, 64 lanes, observation i
on lane i % 64): nothing, under three observations, under ten, one short of a
full stride, exactly one, one over, two strides and a remainder, and a
workload-like frame."""
from __future__ import annotations

import functools

import numpy as np

import pyref_pose
from orb_slam_2_ros_amd.synth_pose import make_pose_problem

SIZES = (0, 2, 3, 9, 10, 63, 64, 65, 130, 300)
KINDS = {"mixed": 0.5, "mono": 0.0, "stereo": 1.0}


def _behind(P):
    """observation 5's point moved behind the camera (two metres)"""
    T = P["Tcw_true"]
    Xc = np.array([0.3, -0.2, -2.0])
    P["obs"]["Xw"][5] = (T[:, :3].T @ (Xc - T[:, 3])).astype(np.float32)
    return P


def _ur_edges(P):
    """observation 3 stereo with ur = 0 exactly, observation 4 mono with ur = -1"""
    P["obs"]["ur"][3] = 0.0
    P["obs"]["ur"][4] = -1.0
    return P


# name -> (make_pose_problem arguments, edit).  Seeds chosen on the CPU so that
# each case reaches what test_pose_reference.py asserts of it.
SPECIAL = {
    "returns": (dict(n=130, seed=9, pose_error=(0.03, 0.3)), None),
    "rejected": (dict(n=65, seed=1), None),
    "non-improving": (dict(n=300, seed=0), None),
    "empty-round": (dict(n=12, seed=0, stereo_frac=0.0, noise_px=0.0, pose_error=(1.0, 10.0)), None),
    "nine": (dict(n=9, seed=2), None),
    "two": (dict(n=2, seed=3), None),
    "behind": (dict(n=40, seed=11), _behind),
    "ur-edges": (dict(n=40, seed=12, stereo_frac=0.5), _ur_edges),
}


def size_case(n, kind):
    return make_pose_problem(n, seed=100 + n, stereo_frac=KINDS[kind])


@functools.lru_cache(maxsize=None)
def problem(name):
    if isinstance(name, tuple):
        return size_case(*name)
    kw, edit = SPECIAL[name]
    P = make_pose_problem(**kw)
    return edit(P) if edit else P


@functools.lru_cache(maxsize=None)
def reference(name):
    """pyref_pose.pose_optimization of the case (shared; do not modify)"""
    P = problem(name)
    return pyref_pose.pose_optimization(P["Tcw"], P["cam"], P["obs"])


ALL = tuple((n, k) for n in SIZES for k in KINDS) + tuple(SPECIAL)


def case_id(name):
    return f"{name[1]}-{name[0]}" if isinstance(name, tuple) else name
