"""Synthetic Sim3-optimisation problems (Optimizer::OptimizeSim3): two
keyframes with different intrinsics that see one point cloud, a true relative
Sim3 S12 (camera-2 coordinates to camera-1 coordinates, x1 = s R x2 + t), the
points' float coordinates in either camera, their projections with
octave-scaled pixel noise (the octaves of the two observations of a point are
drawn independently, so the two edges of a correspondence carry different
information), a few planted gross outliers, and an initial Sim3 perturbed from
the truth."""
from __future__ import annotations

import numpy as np

from .synth_ba import _rot

SIM3_DTYPE = np.dtype([("q", "<f8", (4,)), ("t", "<f8", (3,)), ("s", "<f8")])
assert SIM3_DTYPE.itemsize == 64
SIM3_CAM_DTYPE = np.dtype([("fx", "<f4"), ("fy", "<f4"), ("cx", "<f4"), ("cy", "<f4")])
assert SIM3_CAM_DTYPE.itemsize == 16
SIM3_CORR_DTYPE = np.dtype([("P1c", "<f4", (3,)), ("P2c", "<f4", (3,)), ("u1", "<f4"), ("v1", "<f4"),
                            ("inv_sigma2_1", "<f4"), ("u2", "<f4"), ("v2", "<f4"), ("inv_sigma2_2", "<f4")])
assert SIM3_CORR_DTYPE.itemsize == 48


def quat_of(R):
    """(x, y, z, w) of a rotation matrix, w >= 0"""
    w = np.sqrt(max(0.0, 1.0 + R[0, 0] + R[1, 1] + R[2, 2])) / 2
    if w > 1e-6:
        return np.array([(R[2, 1] - R[1, 2]) / (4 * w), (R[0, 2] - R[2, 0]) / (4 * w), (R[1, 0] - R[0, 1]) / (4 * w), w])
    i = int(np.argmax(np.diag(R)))
    j, k = (i + 1) % 3, (i + 2) % 3
    t = np.sqrt(R[i, i] - R[j, j] - R[k, k] + 1.0)
    q = np.zeros(4)
    q[i] = 0.5 * t
    q[3] = (R[k, j] - R[j, k]) / (2 * t)
    q[j] = (R[j, i] + R[i, j]) / (2 * t)
    q[k] = (R[k, i] + R[i, k]) / (2 * t)
    return q


def sim3_record(R, t, s):
    S = np.zeros(1, SIM3_DTYPE)
    S["q"][0], S["t"][0], S["s"][0] = quat_of(R), t, s
    return S


def make_sim3_problem(n=40, seed=0, scale=1.0, fix_scale=False, outlier_frac=0.0, noise_px=1.0,
                      sim3_error=(0.01, 0.05, 0.02), init_scale=None, outlier_px=50.0, th2=10.0, w=640, h=480,
                      cam1=(520.9, 521.0, 325.1, 249.7), cam2=(535.4, 539.2, 320.1, 247.6)):
    """n correspondences.  scale: the true scale of S12; sim3_error: (rotation
    rad, translation m, log-scale) sigma of the initial Sim3; init_scale: the
    initial scale where it is not the perturbed truth (with fix_scale it is
    what the optimiser keeps); outlier_frac: the share whose u1 or u2 (drawn)
    is moved by +-outlier_px; noise_px: pixel sigma at octave 0 (times
    1.2^octave).  Returns dict: S12 SIM3_DTYPE (1,) (initial), cam1, cam2
    SIM3_CAM_DTYPE (1,), corr SIM3_CORR_DTYPE (n,), th2, fix_scale, planted
    (n,) bool, R_true, t_true, s_true."""
    rng = np.random.default_rng(seed)
    sf = 1.2 ** np.arange(8)
    inv_sigma2 = (1.0 / (sf * sf)).astype(np.float32)
    fx1, fy1, cx1, cy1 = cam1
    fx2, fy2, cx2, cy2 = cam2
    R = _rot(rng.normal(0, 0.08, 3))
    t = rng.normal(0, 0.3, 3)
    s = float(scale)
    # points through their pixels in image 1, so that every one projects inside it
    u = rng.uniform(40, w - 40, n)
    v = rng.uniform(40, h - 40, n)
    z = rng.uniform(3, 12, n)
    P1 = np.stack([(u - cx1) / fx1 * z, (v - cy1) / fy1 * z, z], 1)
    P2 = ((P1 - t) @ R) / s                      # R^T (P1 - t) / s
    P1f, P2f = P1.astype(np.float32), P2.astype(np.float32)
    P1d, P2d = P1f.astype(np.float64), P2f.astype(np.float64)
    # each observation is the projection of its own camera's float point
    oct1 = rng.choice(8, n, p=[0.3, 0.2, 0.15, 0.12, 0.09, 0.07, 0.04, 0.03])
    oct2 = rng.choice(8, n, p=[0.3, 0.2, 0.15, 0.12, 0.09, 0.07, 0.04, 0.03])
    u1 = fx1 * P1d[:, 0] / P1d[:, 2] + cx1 + rng.normal(0, 1, n) * sf[oct1] * noise_px
    v1 = fy1 * P1d[:, 1] / P1d[:, 2] + cy1 + rng.normal(0, 1, n) * sf[oct1] * noise_px
    u2 = fx2 * P2d[:, 0] / P2d[:, 2] + cx2 + rng.normal(0, 1, n) * sf[oct2] * noise_px
    v2 = fy2 * P2d[:, 1] / P2d[:, 2] + cy2 + rng.normal(0, 1, n) * sf[oct2] * noise_px
    planted = rng.random(n) < outlier_frac
    side = rng.random(n) < 0.5
    shift = rng.choice([-1.0, 1.0], n) * outlier_px
    u1 = u1 + np.where(planted & side, shift, 0.0)
    u2 = u2 + np.where(planted & ~side, shift, 0.0)
    corr = np.zeros(n, SIM3_CORR_DTYPE)
    corr["P1c"], corr["P2c"] = P1f, P2f
    corr["u1"], corr["v1"], corr["inv_sigma2_1"] = u1, v1, inv_sigma2[oct1]
    corr["u2"], corr["v2"], corr["inv_sigma2_2"] = u2, v2, inv_sigma2[oct2]
    dR = _rot(rng.normal(0, sim3_error[0], 3))
    s0 = s * float(np.exp(rng.normal(0, sim3_error[2]))) if init_scale is None else float(init_scale)
    S12 = sim3_record(dR @ R, t + rng.normal(0, sim3_error[1], 3), s0)
    return {"S12": S12, "cam1": np.array([cam1], SIM3_CAM_DTYPE), "cam2": np.array([cam2], SIM3_CAM_DTYPE),
            "corr": corr, "th2": float(th2), "fix_scale": bool(fix_scale), "planted": planted,
            "R_true": R, "t_true": t, "s_true": s}
