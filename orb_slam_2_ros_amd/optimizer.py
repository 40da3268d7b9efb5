"""Host mirror of Optimizer::LocalBundleAdjustment (Optimizer.cc:517-900)
over liborbx's GPU bundle adjustment (include/orbx.h).  The
caller collects the graph (local keyframes, fixed cameras, local map points
and their observations) exactly as the reference does; this runs the two LM
passes and returns the optimised poses and points and the observations to
erase, and of Optimizer::PoseOptimization (Optimizer.cc:265-509), the
motion-only optimisation of a frame, single or as a batch of frames in one
kernel launch, and of Optimizer::OptimizeSim3 (Optimizer.cc:1177-1414), the
relative Sim3 of a loop candidate, single or batched likewise.  GPU only."""
from __future__ import annotations

import ctypes

import numpy as np

from ._lib import check, load, ptr
from .synth_ba import BA_EDGE_DTYPE
from .synth_pose import POSE_CAM_DTYPE, POSE_OBS_DTYPE
from .synth_sim3 import SIM3_CAM_DTYPE, SIM3_CORR_DTYPE, SIM3_DTYPE


def local_bundle_adjustment(Tcw, fixed, Xw, edges, iters=(5, 10), device: int = 0, fast: bool = False):
    """Tcw (ncam, 3, 4) f32, fixed (ncam,) bool, Xw (npt, 3) f32, edges
    BA_EDGE_DTYPE.  Returns (Tcw_out, Xw_out, outlier (ne,) bool,
    (iterations pass 1, pass 2)).  fast: orbx_local_ba_fast (the sums as
    parallel reductions; equal to the ordered mode to rounding)."""
    T = np.ascontiguousarray(Tcw, np.float32).reshape(-1, 3, 4)
    F = np.ascontiguousarray(fixed, np.uint8)
    X = np.ascontiguousarray(Xw, np.float32).reshape(-1, 3)
    E = np.ascontiguousarray(edges, BA_EDGE_DTYPE)
    To, Xo = np.empty_like(T), np.empty_like(X)
    out = np.zeros(max(len(E), 1), np.uint8)
    its = np.zeros(2, np.int32)
    fn = load().orbx_local_ba_fast if fast else load().orbx_local_ba
    check(fn(device, ptr(T), ptr(F), len(T), ptr(X), len(X), ptr(E), len(E), int(iters[0]),
             int(iters[1]), ptr(To), ptr(Xo), ptr(out), ptr(its)), "orbx_local_ba")
    return To, Xo, out[:len(E)].astype(bool), (int(its[0]), int(its[1]))


def debug_step(Tcw, fixed, Xw, edges, robust=True, lam=1e-3, device: int = 0, fast: bool = False):
    """One LM linear system of the first pass (test hook): (x, chi2, solved).
    fast: orbx_ba_debug_step_fast, the step as an orbx_local_ba_fast trial
    solves it."""
    T = np.ascontiguousarray(Tcw, np.float32).reshape(-1, 3, 4)
    F = np.ascontiguousarray(fixed, np.uint8)
    X = np.ascontiguousarray(Xw, np.float32).reshape(-1, 3)
    E = np.ascontiguousarray(edges, BA_EDGE_DTYPE)
    n = 6 * int((F == 0).sum()) + 3 * len(X)
    x = np.zeros(max(n, 1), np.float64)
    chi2 = ctypes.c_double(0)
    ok = ctypes.c_int(0)
    fn = load().orbx_ba_debug_step_fast if fast else load().orbx_ba_debug_step
    check(fn(device, ptr(T), ptr(F), len(T), ptr(X), len(X), ptr(E), len(E), int(robust), float(lam), ptr(x),
             ctypes.byref(chi2), ctypes.byref(ok)), "orbx_ba_debug_step")
    return x[:n], chi2.value, bool(ok.value)


def _pose_args(Tcw, cams, obs, offsets):
    T = np.ascontiguousarray(Tcw, np.float32).reshape(-1, 3, 4)
    C = np.ascontiguousarray(cams, POSE_CAM_DTYPE).reshape(-1)
    O = np.ascontiguousarray(obs, POSE_OBS_DTYPE).reshape(-1)
    off = np.ascontiguousarray(offsets, np.int32).reshape(-1)
    if len(C) != len(T) or len(off) != len(T) + 1:
        raise ValueError("pose batch: Tcw, cams and offsets disagree on the number of problems")
    return T, C, O, off


def pose_optimization(Tcw, cam, obs, device: int = 0):
    """Optimizer::PoseOptimization of one frame.  Tcw (3, 4) f32, cam
    POSE_CAM_DTYPE (one record), obs POSE_OBS_DTYPE: the features that have a
    map point, in feature order.  Returns (Tcw_out (3, 4) f32, outlier (n,)
    bool, chi2 (n,) f64, n_inliers, iterations per round (4,))."""
    T = np.ascontiguousarray(Tcw, np.float32).reshape(3, 4)
    C = np.ascontiguousarray(cam, POSE_CAM_DTYPE).reshape(1)
    O = np.ascontiguousarray(obs, POSE_OBS_DTYPE).reshape(-1)
    n = len(O)
    To = np.empty_like(T)
    out = np.zeros(max(n, 1), np.uint8)
    chi2 = np.zeros(max(n, 1), np.float64)
    ninl = ctypes.c_int(0)
    its = np.zeros(4, np.int32)
    check(load().orbx_pose_optimization(device, ptr(T), ptr(C), ptr(O), n, ptr(To), ptr(out), ptr(chi2),
                                        ctypes.byref(ninl), ptr(its)), "orbx_pose_optimization")
    return To, out[:n].astype(bool), chi2[:n], int(ninl.value), its


def pose_optimization_batch(Tcw, cams, obs, offsets, device: int = 0):
    """A batch of frames in one launch.  Tcw (P, 3, 4) f32, cams (P,)
    POSE_CAM_DTYPE, obs POSE_OBS_DTYPE in CSR by problem, offsets (P + 1,)
    int32.  Returns (Tcw_out, outlier (N,) bool, chi2 (N,), n_inliers (P,),
    iterations (P, 4)) as numpy arrays.

    With torch device tensors (Tcw (P, 3, 4) f32, cams (P, 5) f32, obs (N, 7)
    f32 in POSE_OBS_DTYPE's field order, offsets (P + 1,) int32) the call is
    orbx_pose_optimization_batch_device on the tensors' device and torch's
    current stream, asynchronous, and the results are device tensors (outlier
    as uint8)."""
    if hasattr(Tcw, "is_cuda"):
        return _pose_batch_device(Tcw, cams, obs, offsets)
    T, C, O, off = _pose_args(Tcw, cams, obs, offsets)
    P, N = len(T), len(O)
    if P and int(off[-1]) != N:
        raise ValueError("pose batch: offsets[-1] != len(obs)")
    To = np.empty_like(T)
    out = np.zeros(max(N, 1), np.uint8)
    chi2 = np.zeros(max(N, 1), np.float64)
    ninl = np.zeros(max(P, 1), np.int32)
    its = np.zeros((max(P, 1), 4), np.int32)
    check(load().orbx_pose_optimization_batch(device, ptr(T), ptr(C), ptr(O), ptr(off), P, ptr(To), ptr(out),
                                              ptr(chi2), ptr(ninl), ptr(its)), "orbx_pose_optimization_batch")
    return To, out[:N].astype(bool), chi2[:N], ninl[:P], its[:P]


def _pose_batch_device(Tcw, cams, obs, offsets):
    import torch
    for t, dt in ((Tcw, torch.float32), (cams, torch.float32), (obs, torch.float32), (offsets, torch.int32)):
        if not t.is_cuda or t.dtype != dt or not t.is_contiguous() or t.device != Tcw.device:
            raise ValueError("pose batch: contiguous tensors of one device, f32 / f32 / f32 / int32")
    P = Tcw.shape[0]
    N = obs.shape[0]
    if Tcw.numel() != 12 * P or cams.numel() != 5 * P or obs.numel() != 7 * N or offsets.numel() != P + 1:
        raise ValueError("pose batch: shapes (P, 3, 4), (P, 5), (N, 7), (P + 1,)")
    dev = Tcw.device
    with torch.cuda.device(dev):
        To = torch.empty_like(Tcw)
        out = torch.empty(max(N, 1), dtype=torch.uint8, device=dev)
        chi2 = torch.empty(max(N, 1), dtype=torch.float64, device=dev)
        ninl = torch.empty(max(P, 1), dtype=torch.int32, device=dev)
        its = torch.empty((max(P, 1), 4), dtype=torch.int32, device=dev)
        obs_p = obs.data_ptr() if N else out.data_ptr()   # (an empty tensor has no storage; nothing reads it)
        check(load().orbx_pose_optimization_batch_device(
            Tcw.data_ptr(), cams.data_ptr(), obs_p, offsets.data_ptr(), P, To.data_ptr(), out.data_ptr(),
            chi2.data_ptr(), ninl.data_ptr(), its.data_ptr(), torch.cuda.current_stream(dev).cuda_stream),
            "orbx_pose_optimization_batch_device")
    return To, out[:N], chi2[:N], ninl[:P], its[:P]


def pose_debug_step(Tcw, cam, obs, active=None, robust=True, lam=0.0, device: int = 0):
    """One linear system of a round at the input pose (test hook): (H (6, 6),
    b (6,), x (6,), robust chi2, solved)."""
    T = np.ascontiguousarray(Tcw, np.float32).reshape(3, 4)
    C = np.ascontiguousarray(cam, POSE_CAM_DTYPE).reshape(1)
    O = np.ascontiguousarray(obs, POSE_OBS_DTYPE).reshape(-1)
    A = None if active is None else np.ascontiguousarray(active, np.uint8)
    if A is not None and len(A) != len(O):
        raise ValueError("pose step: one active flag per observation")
    H, b, x = np.zeros((6, 6)), np.zeros(6), np.zeros(6)
    chi2 = ctypes.c_double(0)
    ok = ctypes.c_int(0)
    check(load().orbx_pose_debug_step(device, ptr(T), ptr(C), ptr(O), len(O), ptr(A), int(robust), float(lam),
                                      ptr(H), ptr(b), ptr(x), ctypes.byref(chi2), ctypes.byref(ok)),
          "orbx_pose_debug_step")
    return H, b, x, chi2.value, bool(ok.value)


def optimize_sim3(S12, cam1, cam2, corr, th2=10.0, fix_scale=False, device: int = 0):
    """Optimizer::OptimizeSim3 of one candidate.  S12 SIM3_DTYPE (one record),
    cam1, cam2 SIM3_CAM_DTYPE (one record each), corr SIM3_CORR_DTYPE in
    vnIndexEdge's order.  Returns (S12_out SIM3_DTYPE (1,), removed (n,) uint8
    (0 kept, 1 / 2 removed by the first / second classification), chi2_12,
    chi2_21 (n,) f64, n_inliers, iterations per round (2,))."""
    S = np.ascontiguousarray(S12, SIM3_DTYPE).reshape(1)
    C1 = np.ascontiguousarray(cam1, SIM3_CAM_DTYPE).reshape(1)
    C2 = np.ascontiguousarray(cam2, SIM3_CAM_DTYPE).reshape(1)
    K = np.ascontiguousarray(corr, SIM3_CORR_DTYPE).reshape(-1)
    n = len(K)
    So = np.zeros(1, SIM3_DTYPE)
    rem = np.zeros(max(n, 1), np.uint8)
    c12, c21 = np.zeros(max(n, 1)), np.zeros(max(n, 1))
    ninl = ctypes.c_int(0)
    its = np.zeros(2, np.int32)
    check(load().orbx_optimize_sim3(device, ptr(S), ptr(C1), ptr(C2), ptr(K), n, float(th2), int(bool(fix_scale)),
                                    ptr(So), ptr(rem), ptr(c12), ptr(c21), ctypes.byref(ninl), ptr(its)),
          "orbx_optimize_sim3")
    return So, rem[:n], c12[:n], c21[:n], int(ninl.value), its


def _sim3_batch_args(S12, cam1, cam2, corr, offsets, th2, fix_scale):
    S = np.ascontiguousarray(S12, SIM3_DTYPE).reshape(-1)
    C1 = np.ascontiguousarray(cam1, SIM3_CAM_DTYPE).reshape(-1)
    C2 = np.ascontiguousarray(cam2, SIM3_CAM_DTYPE).reshape(-1)
    K = np.ascontiguousarray(corr, SIM3_CORR_DTYPE).reshape(-1)
    off = np.ascontiguousarray(offsets, np.int32).reshape(-1)
    P = len(S)
    th = np.ascontiguousarray(np.broadcast_to(np.asarray(th2, np.float32), (P,)))
    fix = np.ascontiguousarray(np.broadcast_to(np.asarray(fix_scale).astype(np.int32), (P,)))
    if len(C1) != P or len(C2) != P or len(off) != P + 1:
        raise ValueError("sim3 batch: S12, cam1, cam2 and offsets disagree on the number of problems")
    return S, C1, C2, K, off, th, fix


def optimize_sim3_batch(S12, cam1, cam2, corr, offsets, th2=10.0, fix_scale=False, device: int = 0, stream=None):
    """A batch of candidates in one launch.  S12 (P,) SIM3_DTYPE, cam1, cam2
    (P,) SIM3_CAM_DTYPE, corr SIM3_CORR_DTYPE in CSR by problem, offsets
    (P + 1,) int32, th2 and fix_scale scalars or (P,).  Returns (S12_out (P,),
    removed (N,) uint8, chi2_12, chi2_21 (N,), n_inliers (P,), iterations
    (P, 2)) as numpy arrays.

    With a torch.cuda.Stream as `stream` the arrays are uploaded through
    torch, orbx_optimize_sim3_batch_device is enqueued on that stream, and the
    results are copied back after the stream is synchronised."""
    S, C1, C2, K, off, th, fix = _sim3_batch_args(S12, cam1, cam2, corr, offsets, th2, fix_scale)
    P, N = len(S), len(K)
    if P and int(off[-1]) != N:
        raise ValueError("sim3 batch: offsets[-1] != len(corr)")
    if stream is not None:
        return _sim3_batch_device(S, C1, C2, K, off, th, fix, stream)
    So = np.zeros(max(P, 1), SIM3_DTYPE)
    rem = np.zeros(max(N, 1), np.uint8)
    c12, c21 = np.zeros(max(N, 1)), np.zeros(max(N, 1))
    ninl = np.zeros(max(P, 1), np.int32)
    its = np.zeros((max(P, 1), 2), np.int32)
    check(load().orbx_optimize_sim3_batch(device, ptr(S), ptr(C1), ptr(C2), ptr(K), ptr(off), P, ptr(th), ptr(fix),
                                          ptr(So), ptr(rem), ptr(c12), ptr(c21), ptr(ninl), ptr(its)),
          "orbx_optimize_sim3_batch")
    return So[:P], rem[:N], c12[:N], c21[:N], ninl[:P], its[:P]


def sim3_device_buffers(S, C1, C2, K, off, th, fix, dev):
    """The batch as torch byte / typed tensors on dev plus its output tensors:
    (inputs, outputs) in orbx_optimize_sim3_batch_device's argument order"""
    import torch

    def up(a):
        raw = np.frombuffer(np.ascontiguousarray(a).tobytes() or b"\0", np.uint8).copy()
        return torch.from_numpy(raw).to(dev)
    P, N = len(S), len(K)
    ins = [up(S), up(C1), up(C2), up(K), up(off), up(th), up(fix)]
    outs = [torch.empty(64 * max(P, 1), dtype=torch.uint8, device=dev),
            torch.empty(max(N, 1), dtype=torch.uint8, device=dev),
            torch.empty(max(N, 1), dtype=torch.float64, device=dev),
            torch.empty(max(N, 1), dtype=torch.float64, device=dev),
            torch.empty(max(P, 1), dtype=torch.int32, device=dev),
            torch.empty((max(P, 1), 2), dtype=torch.int32, device=dev)]
    return ins, outs


def sim3_device_launch(ins, outs, P, stream):
    """orbx_optimize_sim3_batch_device on sim3_device_buffers' tensors, enqueued on the torch stream"""
    i, o = [t.data_ptr() for t in ins], [t.data_ptr() for t in outs]
    check(load().orbx_optimize_sim3_batch_device(i[0], i[1], i[2], i[3], i[4], P, i[5], i[6], o[0], o[1], o[2], o[3],
                                                 o[4], o[5], stream.cuda_stream),
          "orbx_optimize_sim3_batch_device")


def _sim3_batch_device(S, C1, C2, K, off, th, fix, stream):
    import torch
    P, N = len(S), len(K)
    dev = stream.device
    with torch.cuda.device(dev), torch.cuda.stream(stream):
        ins, outs = sim3_device_buffers(S, C1, C2, K, off, th, fix, dev)
        if P:
            sim3_device_launch(ins, outs, P, stream)
        stream.synchronize()
        So = np.frombuffer(outs[0].cpu().numpy().tobytes(), SIM3_DTYPE)[:P].copy()
        return (So, outs[1].cpu().numpy()[:N], outs[2].cpu().numpy()[:N], outs[3].cpu().numpy()[:N],
                outs[4].cpu().numpy()[:P], outs[5].cpu().numpy()[:P])


def sim3_debug_step(S12, cam1, cam2, corr, active=None, robust=True, lam=0.0, fix_scale=False, th2=10.0,
                    device: int = 0):
    """One linear system at S12 (test hook): (H (7, 7), b (7,), x (7,), robust
    chi2, solved)."""
    S = np.ascontiguousarray(S12, SIM3_DTYPE).reshape(1)
    C1 = np.ascontiguousarray(cam1, SIM3_CAM_DTYPE).reshape(1)
    C2 = np.ascontiguousarray(cam2, SIM3_CAM_DTYPE).reshape(1)
    K = np.ascontiguousarray(corr, SIM3_CORR_DTYPE).reshape(-1)
    A = None if active is None else np.ascontiguousarray(active, np.uint8)
    if A is not None and len(A) != len(K):
        raise ValueError("sim3 step: one active flag per correspondence")
    H, b, x = np.zeros((7, 7)), np.zeros(7), np.zeros(7)
    chi2 = ctypes.c_double(0)
    ok = ctypes.c_int(0)
    check(load().orbx_sim3_debug_step(device, ptr(S), ptr(C1), ptr(C2), ptr(K), len(K), float(th2),
                                      int(bool(fix_scale)), ptr(A), int(robust), float(lam), ptr(H), ptr(b), ptr(x),
                                      ctypes.byref(chi2), ctypes.byref(ok)), "orbx_sim3_debug_step")
    return H, b, x, chi2.value, bool(ok.value)


def sim3_debug_update(S, x, fix_scale=False, device: int = 0):
    """Sim3(x[k]) * S[k] (test hook): S (count,) SIM3_DTYPE, x (count, 7) f64.
    Returns (count,) SIM3_DTYPE."""
    Sa = np.ascontiguousarray(S, SIM3_DTYPE).reshape(-1)
    X = np.ascontiguousarray(x, np.float64).reshape(-1, 7)
    if len(X) != len(Sa):
        raise ValueError("sim3 update: one update vector per Sim3")
    out = np.zeros(max(len(Sa), 1), SIM3_DTYPE)
    check(load().orbx_sim3_debug_update(device, ptr(Sa), ptr(X), len(Sa), int(bool(fix_scale)), ptr(out)),
          "orbx_sim3_debug_update")
    return out[:len(Sa)]
