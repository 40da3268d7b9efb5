"""Synthetic pose-optimisation problems (Optimizer::PoseOptimization): one
frame with a ground-truth pose, map points in front of it across the eight
octaves, their float projections with octave-scaled pixel noise, a few planted
gross outliers, and an initial pose perturbed from the truth."""
from __future__ import annotations

import numpy as np

from .synth_ba import _rot

POSE_OBS_DTYPE = np.dtype([("Xw", "<f4", (3,)), ("u", "<f4"), ("v", "<f4"), ("ur", "<f4"), ("inv_sigma2", "<f4")])
assert POSE_OBS_DTYPE.itemsize == 28
POSE_CAM_DTYPE = np.dtype([("fx", "<f4"), ("fy", "<f4"), ("cx", "<f4"), ("cy", "<f4"), ("bf", "<f4")])
assert POSE_CAM_DTYPE.itemsize == 20


def make_pose_problem(n=300, seed=0, stereo_frac=0.5, outlier_frac=0.05, noise_px=1.0, pose_error=(0.01, 0.05),
                      outlier_px=50.0, w=1241, h=376, fx=718.856, fy=718.856, cx=607.1928, cy=185.2157,
                      bf=386.1448):
    """n observations of one frame.  stereo_frac: the share with a right
    coordinate (1.0: all stereo, 0.0: all mono); outlier_frac: the share whose
    u is moved by +-outlier_px; noise_px: pixel sigma at octave 0 (times 1.2^
    octave); pose_error: (rotation rad, translation m) sigma of the initial
    pose.  Returns dict: Tcw (3, 4) f32 (perturbed), cam POSE_CAM_DTYPE (1,),
    obs POSE_OBS_DTYPE (n,), planted (n,) bool, Tcw_true (3, 4) f64."""
    rng = np.random.default_rng(seed)
    sf = 1.2 ** np.arange(8)
    inv_sigma2 = (1.0 / (sf * sf)).astype(np.float32)
    Rwc = _rot(rng.normal(0, 0.1, 3))
    twc = rng.normal(0, 1.0, 3)
    Rcw = Rwc.T
    Tt = np.hstack([Rcw, (-Rcw @ twc)[:, None]])
    # points through their pixels, so that every one projects inside the image
    u = rng.uniform(0, w, n)
    v = rng.uniform(0, h, n)
    z = rng.uniform(4, 40, n)
    Xc = np.stack([(u - cx) / fx * z, (v - cy) / fy * z, z], 1)
    Xw = (Xc - Tt[:, 3]) @ Rcw          # Rwc (Xc - tcw)
    Xw = Xw.astype(np.float32)
    Xc = Xw.astype(np.float64) @ Rcw.T + Tt[:, 3]
    octave = rng.choice(8, n, p=[0.3, 0.2, 0.15, 0.12, 0.09, 0.07, 0.04, 0.03])
    s = sf[octave] * noise_px
    pu = fx * Xc[:, 0] / Xc[:, 2] + cx
    pv = fy * Xc[:, 1] / Xc[:, 2] + cy
    stereo = rng.random(n) < stereo_frac
    ur = np.where(stereo, pu - bf / Xc[:, 2] + rng.normal(0, 1, n) * s, -1.0)
    un = pu + rng.normal(0, 1, n) * s
    vn = pv + rng.normal(0, 1, n) * s
    planted = rng.random(n) < outlier_frac
    un = un + np.where(planted, rng.choice([-1.0, 1.0], n) * outlier_px, 0.0)
    obs = np.zeros(n, POSE_OBS_DTYPE)
    obs["Xw"], obs["u"], obs["v"], obs["ur"], obs["inv_sigma2"] = Xw, un, vn, ur, inv_sigma2[octave]
    dR = _rot(rng.normal(0, pose_error[0], 3))
    T = np.hstack([dR @ Tt[:, :3], (dR @ Tt[:, 3] + rng.normal(0, pose_error[1], 3))[:, None]])
    cam = np.array([(fx, fy, cx, cy, bf)], POSE_CAM_DTYPE)
    return {"Tcw": T.astype(np.float32), "cam": cam, "obs": obs, "planted": planted, "Tcw_true": Tt}
