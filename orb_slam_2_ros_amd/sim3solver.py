"""Sim3Solver (Sim3Solver.cc:37-423) on the device: every RANSAC hypothesis of
a solver, or of a batch of solvers, in one launch (k_sim3_ransac, DESIGN.md
§3.15), and the mirror of the reference's class, whose iterate() walks the
stored results."""
from __future__ import annotations

import math

import numpy as np

from ._lib import check, load, ptr
from .synth_sim3 import SIM3_CAM_DTYPE

RANSAC_CORR_DTYPE = np.dtype([("X1c", "<f4", (3,)), ("X2c", "<f4", (3,)), ("max_err1", "<f4"), ("max_err2", "<f4")])
assert RANSAC_CORR_DTYPE.itemsize == 32
RANSAC_HYP_DTYPE = np.dtype([("R", "<f4", (9,)), ("t", "<f4", (3,)), ("s", "<f4"), ("n_inliers", "<i4")])
assert RANSAC_HYP_DTYPE.itemsize == 56


def sim3_ransac(cam1, cam2, fix_scale, corr, triples, device: int = 0):
    """All hypotheses of one solver.  cam1, cam2 SIM3_CAM_DTYPE (one record
    each), corr RANSAC_CORR_DTYPE (n,) in mvnIndices1's order, triples (h, 3)
    int32.  Returns (hyp (h,) RANSAC_HYP_DTYPE, mask (h, ceil(n / 64)) uint64:
    bit i of a row = correspondence i is an inlier)."""
    C1 = np.ascontiguousarray(cam1, SIM3_CAM_DTYPE).reshape(1)
    C2 = np.ascontiguousarray(cam2, SIM3_CAM_DTYPE).reshape(1)
    K = np.ascontiguousarray(corr, RANSAC_CORR_DTYPE).reshape(-1)
    T = np.ascontiguousarray(triples, np.int32).reshape(-1, 3)
    n, h = len(K), len(T)
    words = (n + 63) // 64
    hyp = np.zeros(max(h, 1), RANSAC_HYP_DTYPE)
    mask = np.zeros(max(h * words, 1), np.uint64)
    check(load().orbx_sim3_ransac(device, ptr(C1), ptr(C2), int(bool(fix_scale)), ptr(K), n, ptr(T), h, ptr(hyp),
                                  ptr(mask)), "orbx_sim3_ransac")
    return hyp[:h], mask[:h * words].reshape(h, words)


def mask_offsets(corr_offsets, hyp_offsets):
    """Each problem's first mask word: the running sum of h * ceil(n / 64)"""
    n = np.diff(np.asarray(corr_offsets, np.int64))
    h = np.diff(np.asarray(hyp_offsets, np.int64))
    return np.concatenate([[0], np.cumsum(h * ((n + 63) // 64))]).astype(np.int64)


def _batch_args(cam1, cam2, fix_scale, corr, corr_offsets, triples, hyp_offsets):
    C1 = np.ascontiguousarray(cam1, SIM3_CAM_DTYPE).reshape(-1)
    C2 = np.ascontiguousarray(cam2, SIM3_CAM_DTYPE).reshape(-1)
    P = len(C1)
    fix = np.ascontiguousarray(np.broadcast_to(np.asarray(fix_scale).astype(np.int32), (P,)))
    K = np.ascontiguousarray(corr, RANSAC_CORR_DTYPE).reshape(-1)
    T = np.ascontiguousarray(triples, np.int32).reshape(-1, 3)
    co = np.ascontiguousarray(corr_offsets, np.int32).reshape(-1)
    ho = np.ascontiguousarray(hyp_offsets, np.int32).reshape(-1)
    if len(C2) != P or len(co) != P + 1 or len(ho) != P + 1:
        raise ValueError("sim3 ransac batch: cameras and offsets disagree on the number of problems")
    if P and (int(co[-1]) != len(K) or int(ho[-1]) != len(T)):
        raise ValueError("sim3 ransac batch: the last offsets are not the array lengths")
    return C1, C2, fix, K, co, T, ho


def split_masks(mask, corr_offsets, hyp_offsets):
    """The flat mask words as one (h_p, words_p) array per problem"""
    mo = mask_offsets(corr_offsets, hyp_offsets)
    n = np.diff(np.asarray(corr_offsets, np.int64))
    h = np.diff(np.asarray(hyp_offsets, np.int64))
    return [mask[mo[p]:mo[p + 1]].reshape(int(h[p]), int((n[p] + 63) // 64)) for p in range(len(n))]


def sim3_ransac_batch(cam1, cam2, fix_scale, corr, corr_offsets, triples, hyp_offsets, device: int = 0, stream=None):
    """A batch of solvers in one launch, in CSR twice (correspondences and
    hypotheses).  cam1, cam2 (P,), fix_scale scalar or (P,), corr (N,),
    corr_offsets (P + 1,), triples (H, 3), hyp_offsets (P + 1,).  Returns (hyp
    (H,), mask words (flat; split_masks gives them per problem)).

    With a torch.cuda.Stream as `stream` the arrays are uploaded through
    torch, orbx_sim3_ransac_batch_device is enqueued on that stream, and the
    results are copied back after the stream is synchronised."""
    C1, C2, fix, K, co, T, ho = _batch_args(cam1, cam2, fix_scale, corr, corr_offsets, triples, hyp_offsets)
    P, H = len(C1), len(T)
    W = int(mask_offsets(co, ho)[-1]) if P else 0
    if stream is not None:
        return _batch_device(C1, C2, fix, K, co, T, ho, stream)
    hyp = np.zeros(max(H, 1), RANSAC_HYP_DTYPE)
    mask = np.zeros(max(W, 1), np.uint64)
    check(load().orbx_sim3_ransac_batch(device, ptr(C1), ptr(C2), ptr(fix), ptr(K), ptr(co), ptr(T), ptr(ho), P,
                                        ptr(hyp), ptr(mask)), "orbx_sim3_ransac_batch")
    return hyp[:H], mask[:W]


def ransac_device_buffers(C1, C2, fix, K, co, T, ho, dev):
    """The batch as torch byte tensors on dev plus its output tensors:
    (inputs, outputs) in orbx_sim3_ransac_batch_device's argument order"""
    import torch

    def up(a):
        raw = np.frombuffer(np.ascontiguousarray(a).tobytes() or b"\0", np.uint8).copy()
        return torch.from_numpy(raw).to(dev)
    mo = mask_offsets(co, ho)
    ins = [up(C1), up(C2), up(fix), up(K), up(co), up(T), up(ho), up(mo)]
    outs = [torch.empty(56 * max(len(T), 1), dtype=torch.uint8, device=dev),
            torch.empty(max(int(mo[-1]), 1), dtype=torch.int64, device=dev)]
    return ins, outs


def ransac_device_launch(ins, outs, P, max_hyp, stream):
    """orbx_sim3_ransac_batch_device on ransac_device_buffers' tensors, enqueued on the torch stream"""
    i, o = [t.data_ptr() for t in ins], [t.data_ptr() for t in outs]
    check(load().orbx_sim3_ransac_batch_device(i[0], i[1], i[2], i[3], i[4], i[5], i[6], i[7], P, int(max_hyp), o[0],
                                               o[1], stream.cuda_stream), "orbx_sim3_ransac_batch_device")


def _batch_device(C1, C2, fix, K, co, T, ho, stream):
    import torch
    P, H = len(C1), len(T)
    W = int(mask_offsets(co, ho)[-1]) if P else 0
    dev = stream.device
    with torch.cuda.device(dev), torch.cuda.stream(stream):
        ins, outs = ransac_device_buffers(C1, C2, fix, K, co, T, ho, dev)
        if P:
            ransac_device_launch(ins, outs, P, int(np.diff(ho).max()), stream)
        stream.synchronize()
        hyp = np.frombuffer(outs[0].cpu().numpy().tobytes(), RANSAC_HYP_DTYPE)[:H].copy()
        return hyp, outs[1].cpu().numpy().view(np.uint64)[:W].copy()


def debug_atan2(y, x, device: int = 0):
    """The device's double atan2 over arrays (test hook)"""
    Y, X = np.ascontiguousarray(y, np.float64).reshape(-1), np.ascontiguousarray(x, np.float64).reshape(-1)
    if len(Y) != len(X):
        raise ValueError("atan2: y and x differ in length")
    out = np.zeros(max(len(Y), 1))
    check(load().orbx_sim3_ransac_debug_atan2(device, ptr(Y), ptr(X), len(Y), ptr(out)),
          "orbx_sim3_ransac_debug_atan2")
    return out[:len(Y)]


def max_error(sigma2):
    """mvnMaxError's entry: 9.210 * sigmaSquare held in a size_t, read as a float"""
    return np.float32(int(9.210 * float(np.float32(sigma2))))


def draw_triples(n, count, random_int):
    """`count` index triples the way iterate() draws them (:163-177):
    random_int(lo, hi) is DUtils::Random::RandomInt, and a drawn index is
    replaced by the last available one."""
    out = np.zeros((count, 3), np.int32)
    for k in range(count):
        avail = list(range(n))
        for i in range(3):
            r = random_int(0, len(avail) - 1)
            out[k, i] = avail[r]
            avail[r] = avail[-1]
            avail.pop()
    return out


class Sim3Solver:
    """Mirror of ORB_SLAM2::Sim3Solver over prepared arrays.  corr: the N
    accepted correspondences (RANSAC_CORR_DTYPE) in mvnIndices1's order;
    indices1[i]: correspondence i's index into vpMatched12; n_matched: mN1;
    random_int(lo, hi): the caller's DUtils::Random::RandomInt.  All
    mRansacMaxIts triples are drawn and their hypotheses launched on the first
    iterate() (or by prepare(), which takes several solvers in one launch)."""

    def __init__(self, cam1, cam2, corr, indices1, n_matched, fix_scale=False, random_int=None, device: int = 0):
        self.cam1 = np.ascontiguousarray(cam1, SIM3_CAM_DTYPE).reshape(1)
        self.cam2 = np.ascontiguousarray(cam2, SIM3_CAM_DTYPE).reshape(1)
        self.corr = np.ascontiguousarray(corr, RANSAC_CORR_DTYPE).reshape(-1)
        self.indices1 = [int(i) for i in indices1]
        self.mN1, self.fix_scale, self.device = int(n_matched), bool(fix_scale), device
        if random_int is None:
            rng = np.random.default_rng(0)
            random_int = lambda lo, hi: int(rng.integers(lo, hi + 1))  # noqa: E731
        self.random_int = random_int
        self.best_inliers, self.best = 0, None
        self.hyp = self.mask = self.triples = None
        self.set_ransac_parameters()

    def set_ransac_parameters(self, probability=0.99, min_inliers=6, max_iterations=300):
        """SetRansacParameters (:114-138), on the host as it is"""
        self.N = len(self.corr)
        self.min_inliers = int(min_inliers)
        with np.errstate(all="ignore"):
            eps = np.float32(self.min_inliers) / np.float32(self.N)
            if self.min_inliers == self.N:
                nit = 1
            else:
                v = np.ceil(np.log(np.float64(1 - probability)) / np.log(np.float64(1) - np.float64(math.pow(float(eps), 3.0))))
                nit = int(v) if np.isfinite(v) and abs(v) < 2 ** 31 else -2 ** 31
        self.max_its = max(1, min(nit, int(max_iterations)))
        self.iterations = 0
        self.hyp = self.mask = self.triples = None   # (a new iteration count needs its own hypotheses)

    def draw(self):
        """The solver's mRansacMaxIts triples (none when iterate() returns at once)"""
        if self.N < self.min_inliers or self.N < 3:
            return np.zeros((0, 3), np.int32)
        return draw_triples(self.N, self.max_its, self.random_int)

    def _store(self, triples, hyp, mask):
        self.triples, self.hyp, self.mask = triples, hyp, mask

    @staticmethod
    def prepare(solvers, device: int = 0):
        """The hypotheses of several solvers in one launch"""
        solvers = [s for s in solvers if s.hyp is None]
        if not solvers:
            return
        T = [s.draw() for s in solvers]
        co = np.concatenate([[0], np.cumsum([len(s.corr) for s in solvers])]).astype(np.int32)
        ho = np.concatenate([[0], np.cumsum([len(t) for t in T])]).astype(np.int32)
        hyp, mask = sim3_ransac_batch(np.concatenate([s.cam1 for s in solvers]),
                                      np.concatenate([s.cam2 for s in solvers]),
                                      np.array([s.fix_scale for s in solvers], np.int32),
                                      np.concatenate([s.corr for s in solvers]), co, np.concatenate(T), ho, device)
        masks = split_masks(mask, co, ho)
        for p, s in enumerate(solvers):
            s._store(T[p], hyp[ho[p]:ho[p + 1]], masks[p])

    def iterate(self, n_iterations):
        """Returns (T12 (4, 4) float32 or None, bNoMore, vbInliers (mN1,) bool, nInliers)"""
        vb = np.zeros(self.mN1, bool)
        if self.N < self.min_inliers:
            return None, True, vb, 0
        if self.hyp is None:
            Sim3Solver.prepare([self], self.device)
        cur = 0
        while self.iterations < self.max_its and cur < n_iterations:
            cur += 1
            k = self.iterations
            self.iterations += 1
            count = int(self.hyp["n_inliers"][k])
            if count >= self.best_inliers:
                self.best, self.best_inliers = k, count
                if count > self.min_inliers:
                    for i in range(self.N):
                        if (int(self.mask[k][i >> 6]) >> (i & 63)) & 1:
                            vb[self.indices1[i]] = True
                    return self._T12(k), False, vb, count
        return None, self.iterations >= self.max_its, vb, 0

    def find(self):
        """Returns (T12 or None, vbInliers12, nInliers)"""
        T, _, vb, n = self.iterate(self.max_its)
        return T, vb, n

    def _T12(self, k):
        """[sR | t; 0 0 0 1]; sR is the float product the hypothesis itself used"""
        h = self.hyp[k]
        T = np.eye(4, dtype=np.float32)
        T[:3, :3] = h["s"] * h["R"].reshape(3, 3)
        T[:3, 3] = h["t"]
        return T

    def get_estimated_rotation(self):
        return None if self.best is None else self.hyp["R"][self.best].reshape(3, 3).copy()

    def get_estimated_translation(self):
        return None if self.best is None else self.hyp["t"][self.best].copy()

    def get_estimated_scale(self):
        return None if self.best is None else float(self.hyp["s"][self.best])
