"""CreateNewMapPoints' triangulation (LocalMapping.cc:334-480) on the device:
every matched pair of a neighbour, or of a batch of neighbours, in one launch
(k_triangulate), and the reference's loop as a walk over the
stored results."""
from __future__ import annotations

import numpy as np

from ._lib import check, load, ptr

TRI_VIEW_DTYPE = np.dtype([("Tcw", "<f4", (12,)), ("Ow", "<f4", (3,)), ("fx", "<f4"), ("fy", "<f4"), ("cx", "<f4"),
                           ("cy", "<f4"), ("invfx", "<f4"), ("invfy", "<f4"), ("mbf", "<f4"), ("mb", "<f4"),
                           ("pad", "<f4")])
assert TRI_VIEW_DTYPE.itemsize == 96
TRI_OBS_DTYPE = np.dtype([("u", "<f4"), ("v", "<f4"), ("ur", "<f4"), ("depth", "<f4"), ("raw_u", "<f4"),
                          ("raw_v", "<f4"), ("sigma2", "<f4"), ("scale", "<f4")])
assert TRI_OBS_DTYPE.itemsize == 32
TRI_PAIR_DTYPE = np.dtype([("o1", TRI_OBS_DTYPE), ("o2", TRI_OBS_DTYPE)])
assert TRI_PAIR_DTYPE.itemsize == 64
TRI_POINT_DTYPE = np.dtype([("X", "<f4", (3,)), ("status", "<i4")])
assert TRI_POINT_DTYPE.itemsize == 16

# orbx_tri_point.status
TRI_CREATED, TRI_LOW_PARALLAX, TRI_W_ZERO, TRI_Z1, TRI_Z2, TRI_REPROJ1, TRI_REPROJ2, TRI_ZERO_DIST, TRI_SCALE, \
    TRI_INVALID_STEREO = range(10)


def triangulate(v1, v2, ratio_factor, pairs, device: int = 0):
    """All pairs of one neighbour.  v1 (the current keyframe), v2 (the
    neighbour) TRI_VIEW_DTYPE (one record each), ratio_factor 1.5f *
    mfScaleFactor, pairs TRI_PAIR_DTYPE (n,).  Returns TRI_POINT_DTYPE (n,)."""
    V1 = np.ascontiguousarray(v1, TRI_VIEW_DTYPE).reshape(1)
    V2 = np.ascontiguousarray(v2, TRI_VIEW_DTYPE).reshape(1)
    K = np.ascontiguousarray(pairs, TRI_PAIR_DTYPE).reshape(-1)
    out = np.zeros(max(len(K), 1), TRI_POINT_DTYPE)
    check(load().orbx_triangulate(device, ptr(V1), ptr(V2), float(np.float32(ratio_factor)), ptr(K), len(K),
                                  ptr(out)), "orbx_triangulate")
    return out[:len(K)]


def _batch_args(v1, v2, ratio_factor, pairs, offsets):
    V1 = np.ascontiguousarray(v1, TRI_VIEW_DTYPE).reshape(-1)
    V2 = np.ascontiguousarray(v2, TRI_VIEW_DTYPE).reshape(-1)
    P = len(V1)
    rf = np.ascontiguousarray(np.broadcast_to(np.asarray(ratio_factor, np.float32), (P,)))
    K = np.ascontiguousarray(pairs, TRI_PAIR_DTYPE).reshape(-1)
    off = np.ascontiguousarray(offsets, np.int32).reshape(-1)
    if len(V2) != P or len(off) != P + 1:
        raise ValueError("triangulate batch: views and offsets disagree on the number of problems")
    if P and int(off[-1]) != len(K):
        raise ValueError("triangulate batch: the last offset is not the number of pairs")
    return V1, V2, rf, K, off


def triangulate_batch(v1, v2, ratio_factor, pairs, offsets, device: int = 0, stream=None):
    """A batch of neighbours in one launch, in CSR.  v1, v2 (P,), ratio_factor
    scalar or (P,), pairs (N,), offsets (P + 1,).  Returns TRI_POINT_DTYPE (N,).

    With a torch.cuda.Stream as `stream` the arrays are uploaded through
    torch, orbx_triangulate_batch_device is enqueued on that stream, and the
    results are copied back after the stream is synchronised."""
    V1, V2, rf, K, off = _batch_args(v1, v2, ratio_factor, pairs, offsets)
    if stream is not None:
        return _batch_device(V1, V2, rf, K, off, stream)
    out = np.zeros(max(len(K), 1), TRI_POINT_DTYPE)
    check(load().orbx_triangulate_batch(device, ptr(V1), ptr(V2), ptr(rf), ptr(K), ptr(off), len(V1), ptr(out)),
          "orbx_triangulate_batch")
    return out[:len(K)]


def triangulate_device_buffers(V1, V2, rf, K, off, dev):
    """The batch as torch byte tensors on dev plus its output tensor: (inputs,
    output) in orbx_triangulate_batch_device's argument order"""
    import torch

    def up(a):
        raw = np.frombuffer(np.ascontiguousarray(a).tobytes() or b"\0", np.uint8).copy()
        return torch.from_numpy(raw).to(dev)
    ins = [up(V1), up(V2), up(rf), up(K), up(off)]
    return ins, torch.empty(16 * max(len(K), 1), dtype=torch.uint8, device=dev)


def triangulate_device_launch(ins, out, P, total_pairs, stream):
    """orbx_triangulate_batch_device on triangulate_device_buffers' tensors, enqueued on the torch stream"""
    i = [t.data_ptr() for t in ins]
    check(load().orbx_triangulate_batch_device(i[0], i[1], i[2], i[3], i[4], P, int(total_pairs), out.data_ptr(),
                                               stream.cuda_stream), "orbx_triangulate_batch_device")


def _batch_device(V1, V2, rf, K, off, stream):
    import torch
    dev = stream.device
    with torch.cuda.device(dev), torch.cuda.stream(stream):
        ins, out = triangulate_device_buffers(V1, V2, rf, K, off, dev)
        if len(V1):
            triangulate_device_launch(ins, out, len(V1), len(K), stream)
        stream.synchronize()
        return np.frombuffer(out.cpu().numpy().tobytes(), TRI_POINT_DTYPE)[:len(K)].copy()


def create_new_map_points_walk(pairs_per_neighbour, points_per_neighbour, has_point, stop_after=None):
    """CreateNewMapPoints' loop (:276-498) over stored results.
    pairs_per_neighbour[i]: neighbour i's (idx1, idx2) list in
    SearchForTriangulation's order; points_per_neighbour[i]: its
    TRI_POINT_DTYPE results; has_point[idx1]: the current keyframe's feature
    already has a map point.  A pair is dropped when its idx1 has a point,
    initially or from an earlier neighbour of this call, or when its status is
    not 0.  stop_after = k: CheckNewKeyFrames() turns true before neighbour
    k > 0 (:280), and the walk returns there.  Returns [(neighbour, idx1, idx2,
    X (3,) float32)] in creation order."""
    claimed = {i for i, b in enumerate(has_point) if b}
    created = []
    for i, (pairs, points) in enumerate(zip(pairs_per_neighbour, points_per_neighbour)):
        if i > 0 and stop_after is not None and i >= stop_after:
            break
        if len(pairs) != len(points):
            raise ValueError(f"neighbour {i}: {len(pairs)} pairs, {len(points)} results")
        status = np.asarray(points["status"]) if len(points) else ()
        for k, (idx1, idx2) in enumerate(pairs):
            idx1 = int(idx1)
            if idx1 in claimed or status[k] != TRI_CREATED:
                continue
            claimed.add(idx1)
            created.append((i, idx1, int(idx2), np.array(points["X"][k], np.float32)))
    return created
