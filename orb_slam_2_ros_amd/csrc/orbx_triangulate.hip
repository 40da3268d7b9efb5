// orbx_triangulate.hip -- the inner loop of LocalMapping::CreateNewMapPoints
// (LocalMapping.cc:334-480) on gfx950: every matched pair of every neighbour of
// a batch in one launch.  A pair's result (the point and why it was or was not
// kept) is a pure function of the two poses, the two cameras and the two
// keypoints, so the reference's loop becomes a walk over results that exist.
// DESIGN.md §3.16 is the numeric specification, orbx_triangulate.h its text
// (shared with a host compile), tests/pyref_triangulate.py its numpy
// restatement.
//
//   k_triangulate   flat grid over the batch's pairs, 64-thread workgroups, one
//                   lane per pair.  A lane finds its problem by bisection of
//                   the offsets (log2(nproblems) loads the wave mostly shares),
//                   loads the two views and its pair, and runs the pair: scalar
//                   work, one long dependent chain, the 4x4 Jacobi's matrices
//                   and double norms in registers (pair order and sort are
//                   fixed, so every index is a constant).  The sweep loop is
//                   the only data-dependent one, bounded by 30.  Nothing is
//                   shared between lanes: no LDS, no barrier.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <mutex>

#include "orbx_device.h"
#include "orbx_triangulate.h"
#include "orbx_ws.h"

namespace orbx {
namespace {

constexpr int kTriLanes = 64;

__global__ __launch_bounds__(kTriLanes) void k_triangulate(const orbx_tri_view *v1, const orbx_tri_view *v2,
                                                           const float *ratio_factor, const orbx_tri_pair *pairs,
                                                           const int32_t *offsets, int nproblems, int total_pairs,
                                                           orbx_tri_point *out) {
    const int i = blockIdx.x * kTriLanes + threadIdx.x;
    if (i >= total_pairs) return;
    const int p = tri_problem_of(offsets, nproblems, i);
    const orbx_tri_view a = v1[p], b = v2[p];
    const orbx_tri_pair k = pairs[i];
    orbx_tri_point r;
    r.status = tri_pair(a, b, ratio_factor[p], k.o1, k.o2, r.X);
    out[i] = r;
}

// Per-device workspace of the host entry points, kept across calls
ArenaWs &tri_ws(int device) {
    static ArenaWs ws[64];
    return ws[device & 63];
}

}  // namespace
}  // namespace orbx

using namespace orbx;

extern "C" {

int orbx_triangulate_batch_device(const orbx_tri_view *d_v1, const orbx_tri_view *d_v2, const float *d_ratio_factor,
                                  const orbx_tri_pair *d_pairs, const int32_t *d_offsets, int nproblems,
                                  int total_pairs, orbx_tri_point *d_out, void *stream) {
    if (nproblems < 0 || total_pairs < 0) return ORBX_EINVAL;
    if (nproblems == 0 || total_pairs == 0) return ORBX_OK;
    if (!d_v1 || !d_v2 || !d_ratio_factor || !d_pairs || !d_offsets || !d_out) return ORBX_EINVAL;
    const dim3 grid((total_pairs + kTriLanes - 1) / kTriLanes);
    hipLaunchKernelGGL(k_triangulate, grid, dim3(kTriLanes), 0, static_cast<hipStream_t>(stream), d_v1, d_v2,
                       d_ratio_factor, d_pairs, d_offsets, nproblems, total_pairs, d_out);
    return hipGetLastError() == hipSuccess ? ORBX_OK : ORBX_EIO;
}

int orbx_triangulate_batch(int device, const orbx_tri_view *v1, const orbx_tri_view *v2, const float *ratio_factor,
                           const orbx_tri_pair *pairs, const int32_t *offsets, int nproblems, orbx_tri_point *out) {
    if (nproblems < 0) return ORBX_EINVAL;
    if (nproblems == 0) return ORBX_OK;
    if (!v1 || !v2 || !ratio_factor || !offsets || offsets[0] != 0) return ORBX_EINVAL;
    for (int p = 0; p < nproblems; ++p)
        if (offsets[p + 1] < offsets[p]) return ORBX_EINVAL;
    const size_t P = nproblems, N = offsets[nproblems];
    if (N == 0) return ORBX_OK;
    if (!pairs || !out) return ORBX_EINVAL;
    for (size_t i = 0; i < N; ++i)
        if (tri_obs_invalid(pairs[i].o1) || tri_obs_invalid(pairs[i].o2)) return ORBX_EINVAL;
    if (hipSetDevice(device) != hipSuccess) return ORBX_ENODEV;
    ArenaWs &ws = tri_ws(device);
    std::lock_guard<std::mutex> lock(ws.mu);
    // arena: inputs (one upload), then the output (one download)
    Layout L;
    const size_t o_v1 = L.add(sizeof(orbx_tri_view) * P), o_v2 = L.add(sizeof(orbx_tri_view) * P);
    const size_t o_rf = L.add(4 * P), o_off = L.add(4 * (P + 1)), o_pairs = L.add(sizeof(orbx_tri_pair) * N);
    const size_t in_end = L.size;
    const size_t o_out = L.add(sizeof(orbx_tri_point) * N);
    int rc = ws_reserve(ws, L.size);
    if (rc) return rc;
    put(ws, o_v1, v1, sizeof(orbx_tri_view) * P);
    put(ws, o_v2, v2, sizeof(orbx_tri_view) * P);
    put(ws, o_rf, ratio_factor, 4 * P);
    put(ws, o_off, offsets, 4 * (P + 1));
    put(ws, o_pairs, pairs, sizeof(orbx_tri_pair) * N);
    if (hipMemcpyAsync(ws.dev, ws.host, in_end, hipMemcpyHostToDevice, ws.st) != hipSuccess) return ORBX_EIO;
    uint8_t *d = ws.dev;
    rc = orbx_triangulate_batch_device(at<orbx_tri_view>(d, o_v1), at<orbx_tri_view>(d, o_v2), at<float>(d, o_rf),
                                       at<orbx_tri_pair>(d, o_pairs), at<int32_t>(d, o_off), nproblems, (int)N,
                                       at<orbx_tri_point>(d, o_out), ws.st);
    if (rc) return rc;
    if (hipMemcpyAsync(ws.host + o_out, d + o_out, sizeof(orbx_tri_point) * N, hipMemcpyDeviceToHost, ws.st) !=
            hipSuccess ||
        hipStreamSynchronize(ws.st) != hipSuccess)
        return ORBX_EIO;
    get(ws, o_out, out, sizeof(orbx_tri_point) * N);
    return ORBX_OK;
}

int orbx_triangulate(int device, const orbx_tri_view *v1, const orbx_tri_view *v2, float ratio_factor,
                     const orbx_tri_pair *pairs, int n, orbx_tri_point *out) {
    if (n < 0) return ORBX_EINVAL;
    const int32_t off[2] = {0, n};
    return orbx_triangulate_batch(device, v1, v2, &ratio_factor, pairs, off, 1, out);
}

}  // extern "C"
