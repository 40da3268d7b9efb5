"""Synthetic CreateNewMapPoints problems: two posed keyframes with different
intrinsics and a baseline between them, world points in front of both, their
observations with pixel noise, octaves that fit the two distances, a share of
stereo observations (right coordinate and depth; the distorted keypoint differs
from the undistorted one) and a planted share of outliers (the second
keyframe's observation moved off its epipolar line)."""
from __future__ import annotations

import numpy as np

from .synth_ba import _rot
from .triangulate import TRI_PAIR_DTYPE, TRI_VIEW_DTYPE

SCALE_FACTOR = np.float32(1.2)
LEVELS = 8


def scale_tables():
    """(mvScaleFactors, mvLevelSigma2) as ORBextractor fills them, float32"""
    s = np.ones(LEVELS, np.float32)
    for i in range(1, LEVELS):
        s[i] = s[i - 1] * SCALE_FACTOR
    return s, (s * s).astype(np.float32)


def make_view(R, t, cam, mbf=40.0):
    """TRI_VIEW_DTYPE (1,) of the pose x_c = R x_w + t (float64 in, float32 as
    KeyFrame::SetPose stores it: Ow = -R^T t in float) and cam = (fx, fy, cx, cy)"""
    v = np.zeros(1, TRI_VIEW_DTYPE)
    R32, t32 = np.asarray(R, np.float32), np.asarray(t, np.float32)
    T = np.zeros((3, 4), np.float32)
    T[:, :3], T[:, 3] = R32, t32
    v["Tcw"][0] = T.reshape(-1)
    Rwc = R32.T
    v["Ow"][0] = [-np.float32((Rwc[i, 0] * t32[0] + Rwc[i, 1] * t32[1]) + Rwc[i, 2] * t32[2]) for i in range(3)]
    fx, fy, cx, cy = (np.float32(c) for c in cam)
    v["fx"], v["fy"], v["cx"], v["cy"] = fx, fy, cx, cy
    v["invfx"], v["invfy"] = np.float32(1.0) / fx, np.float32(1.0) / fy
    v["mbf"] = np.float32(mbf)
    v["mb"] = np.float32(mbf) / fx
    return v


def observe(R, t, cam, mbf, Xw, octave, stereo, noise=(0.0, 0.0), raw_shift=(0.0, 0.0)):
    """One observation (a TRI_OBS_DTYPE tuple) of the world point Xw, float64 geometry"""
    s, sig = scale_tables()
    fx, fy, cx, cy = cam
    c = np.asarray(R, np.float64) @ np.asarray(Xw, np.float64) + np.asarray(t, np.float64)
    u, v = fx * c[0] / c[2] + cx + noise[0], fy * c[1] / c[2] + cy + noise[1]
    ur, depth = (u - mbf / c[2], c[2]) if stereo else (-1.0, -1.0)
    return (u, v, ur, depth, u + raw_shift[0], v + raw_shift[1], sig[octave], s[octave])


def make_triangulation_problem(n=100, seed=0, stereo_frac=0.0, outlier_frac=0.0, noise_px=0.5, baseline=0.5,
                               depth=(2.0, 12.0), rot_sigma=0.08, mbf1=40.0, mbf2=40.0,
                               cam1=(520.9, 521.0, 325.1, 249.7), cam2=(535.4, 539.2, 320.1, 247.6), w=640, h=480,
                               pose1=None):
    """n pairs between a current keyframe and one neighbour.  stereo_frac: the
    share of observations (either side, independently) with a right coordinate
    and a depth; outlier_frac: the share whose second observation is moved by
    tens of pixels; noise_px: sigma of the pixel noise at octave 0 (times the
    octave's scale); pose1: (R1, t1) of the current keyframe instead of a drawn
    one.  Returns dict: v1, v2 TRI_VIEW_DTYPE (1,), ratio_factor
    float32, pairs TRI_PAIR_DTYPE (n,), X_true (n, 3) float64, planted (n,)
    bool, poses ((R1, t1), (R2, t2)) float64, octaves, stereo ((n,), (n,)) bool."""
    rng = np.random.default_rng(seed)
    scales, _ = scale_tables()
    R1, t1 = _rot(rng.normal(0, rot_sigma, 3)), rng.normal(0, 0.2, 3)
    if pose1 is not None:   # several neighbours of one current keyframe
        R1, t1 = np.asarray(pose1[0], np.float64), np.asarray(pose1[1], np.float64)
    R2 = _rot(rng.normal(0, rot_sigma, 3)) @ R1
    d = rng.normal(0, 1, 3) * [1.0, 0.3, 0.2]
    C2 = -R1.T @ t1 + R1.T @ (baseline * d / np.linalg.norm(d))     # the neighbour's centre
    t2 = -R2 @ C2
    u = rng.uniform(60, w - 60, n)
    v = rng.uniform(60, h - 60, n)
    z = rng.uniform(depth[0], depth[1], n)
    Xc = np.stack([(u - cam1[2]) / cam1[0] * z, (v - cam1[3]) / cam1[1] * z, z], 1)
    Xw = (Xc - t1) @ R1                                              # R1^T (Xc - t1)
    d1 = np.linalg.norm(Xw + R1.T @ t1, axis=1)
    d2 = np.linalg.norm(Xw - C2, axis=1)
    oct1 = rng.choice(5, n, p=[0.4, 0.25, 0.15, 0.12, 0.08])
    oct2 = np.clip(oct1 + np.rint(np.log(d1 / d2) / np.log(1.2)).astype(int), 0, LEVELS - 1)
    st1, st2 = rng.random(n) < stereo_frac, rng.random(n) < stereo_frac
    planted = rng.random(n) < outlier_frac
    pairs = np.zeros(n, TRI_PAIR_DTYPE)
    for i in range(n):
        n1, n2 = rng.normal(0, noise_px, 2) * scales[oct1[i]], rng.normal(0, noise_px, 2) * scales[oct2[i]]
        if planted[i]:
            n2 = n2 + rng.choice([-1, 1], 2) * rng.uniform(25, 60, 2)
        pairs["o1"][i] = observe(R1, t1, cam1, mbf1, Xw[i], oct1[i], st1[i], n1, rng.normal(0, 0.4, 2))
        pairs["o2"][i] = observe(R2, t2, cam2, mbf2, Xw[i], oct2[i], st2[i], n2, rng.normal(0, 0.4, 2))
    return {"v1": make_view(R1, t1, cam1, mbf1), "v2": make_view(R2, t2, cam2, mbf2),
            "ratio_factor": np.float32(1.5) * SCALE_FACTOR, "pairs": pairs, "X_true": Xw, "planted": planted,
            "poses": ((R1, t1), (R2, t2)), "octaves": (oct1, oct2), "stereo": (st1, st2)}
