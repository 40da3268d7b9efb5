"""Synthetic Sim3Solver problems: two keyframes with different intrinsics, a
point cloud seen by both, related by a true Sim3 (x1 = s R x2 + t), the points'
float coordinates in either camera, a planted share of outliers (the second
camera's point replaced by an unrelated one), optional 3-D noise, and the
octave-derived thresholds the solver's constructor computes."""
from __future__ import annotations

import numpy as np

from .sim3solver import RANSAC_CORR_DTYPE, max_error
from .synth_ba import _rot
from .synth_sim3 import SIM3_CAM_DTYPE


def make_sim3solver_problem(n=40, seed=0, scale=1.0, fix_scale=False, outlier_frac=0.0, noise_m=0.0, rot_sigma=0.3,
                            w=640, h=480, cam1=(520.9, 521.0, 325.1, 249.7), cam2=(535.4, 539.2, 320.1, 247.6)):
    """n correspondences.  scale: the true scale; outlier_frac: the share whose
    X2c is an unrelated point; noise_m: sigma of the noise added to both
    points.  Returns dict: cam1, cam2 SIM3_CAM_DTYPE (1,), corr
    RANSAC_CORR_DTYPE (n,), fix_scale, planted (n,) bool, octaves, R_true,
    t_true, s_true."""
    rng = np.random.default_rng(seed)
    sigma2 = ((1.2 ** np.arange(8)).astype(np.float32) ** 2).astype(np.float32)   # mvLevelSigma2
    fx1, fy1, cx1, cy1 = cam1
    R = _rot(rng.normal(0, rot_sigma, 3))
    t = rng.normal(0, 0.3, 3)
    s = float(scale)
    u = rng.uniform(40, w - 40, n)
    v = rng.uniform(40, h - 40, n)
    z = rng.uniform(3, 12, n)
    P1 = np.stack([(u - cx1) / fx1 * z, (v - cy1) / fy1 * z, z], 1)
    P2 = ((P1 - t) @ R) / s                      # R^T (P1 - t) / s
    planted = rng.random(n) < outlier_frac
    wrong = np.stack([rng.uniform(-3, 3, n), rng.uniform(-2, 2, n), rng.uniform(3, 12, n)], 1)
    P2 = np.where(planted[:, None], wrong, P2)
    if noise_m:
        P1 = P1 + rng.normal(0, noise_m, P1.shape)
        P2 = P2 + rng.normal(0, noise_m, P2.shape)
    oct1 = rng.choice(8, n, p=[0.3, 0.2, 0.15, 0.12, 0.09, 0.07, 0.04, 0.03])
    oct2 = rng.choice(8, n, p=[0.3, 0.2, 0.15, 0.12, 0.09, 0.07, 0.04, 0.03])
    corr = np.zeros(n, RANSAC_CORR_DTYPE)
    corr["X1c"], corr["X2c"] = P1.astype(np.float32), P2.astype(np.float32)
    corr["max_err1"] = [max_error(sigma2[o]) for o in oct1]
    corr["max_err2"] = [max_error(sigma2[o]) for o in oct2]
    return {"cam1": np.array([cam1], SIM3_CAM_DTYPE), "cam2": np.array([cam2], SIM3_CAM_DTYPE), "corr": corr,
            "fix_scale": bool(fix_scale), "planted": planted, "octaves": (oct1, oct2), "R_true": R, "t_true": t,
            "s_true": s}
