// orbx_sim3_ransac.hip -- Sim3Solver (Sim3Solver.cc:37-423) on gfx950: every
// RANSAC hypothesis of every solver of a batch in one launch.  A hypothesis is
// a pure function of its three correspondence indices (Horn's closed form,
// then the reprojection test of all n correspondences in both images), so
// iterate()'s loop becomes a walk over results that exist (OrbxSim3Solver in
// orbx_orbslam2.hpp).  DESIGN.md §3.15 is the numeric specification,
// orbx_horn.h its text (shared with a host compile), tests/pyref_sim3solver.py
// its numpy restatement.
//
//   k_sim3_ransac   grid (ceil(max_hyp / 64), nproblems), one 64-thread
//                   workgroup (one wave) per 64 consecutive hypotheses of one
//                   problem.  Lane l forms hypothesis l: scalar work, the one
//                   long dependent chain; the Jacobi's 4x4 matrices are in LDS
//                   (element-major, lane-minor: no bank conflicts), because its
//                   pivot indices depend on the data.  Lane l leaves T12 and
//                   T21 (24 floats) in LDS.  The wave then takes the
//                   correspondences 64 at a time, lane = correspondence: each
//                   lane loads its correspondence and forms its own two
//                   projections once, then walks the 64 hypotheses (broadcast
//                   LDS reads of the 24 floats); one ballot per hypothesis and
//                   chunk is the mask word, kept by the lane that owns the
//                   hypothesis, whose popcount adds to that lane's count.
//                   Every loop bound is a constant, n or h; nothing waits on
//                   another workgroup or the host.
//   k_ransac_atan2  atan2 over an array (test hook)
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstring>
#include <mutex>
#include <vector>

#include "orbx_device.h"
#include "orbx_horn.h"
#include "orbx_ws.h"

namespace orbx {
namespace {

struct RansacLds {
    float jac[kJacobiFloats][kHornLanes];
    float T[24][kHornLanes];   // T12 rows of four, then T21
};

__global__ __launch_bounds__(kHornLanes) void k_sim3_ransac(
    const orbx_sim3_camera *cam1, const orbx_sim3_camera *cam2, const int32_t *fix_scale, const orbx_ransac_corr *corr,
    const int32_t *corr_offsets, const int32_t *triples, const int32_t *hyp_offsets, const int64_t *mask_offsets,
    int nproblems, orbx_ransac_hyp *hyp, uint64_t *mask) {
    __shared__ RansacLds lds;
    const int p = blockIdx.y, lane = threadIdx.x;
    if (p >= nproblems) return;
    const int64_t h0 = hyp_offsets[p];
    const int H = (int)(hyp_offsets[p + 1] - h0);
    const int first = blockIdx.x * kHornLanes;
    if (first >= H) return;   // (uniform over the workgroup)
    const int64_t c0 = corr_offsets[p];
    const int n = (int)(corr_offsets[p + 1] - c0);
    const orbx_ransac_corr *K = corr + c0;
    const orbx_sim3_camera k1 = cam1[p], k2 = cam2[p];
    const int count = min(kHornLanes, H - first);
    const int words = (n + 63) >> 6;
    const bool mine = lane < count;
    const int64_t hid = h0 + first + lane;

    if (mine) {
        int32_t tr[3];
        for (int k = 0; k < 3; ++k) tr[k] = triples[3 * hid + k];
        HornResult r;
        if (horn_triple_ok(tr, n)) {
            float P1[3][3], P2[3][3];
            for (int i = 0; i < 3; ++i) {
                const orbx_ransac_corr c = K[tr[i]];
                for (int rr = 0; rr < 3; ++rr) {
                    P1[rr][i] = c.X1c[rr];
                    P2[rr][i] = c.X2c[rr];
                }
            }
            horn_compute(P1, P2, fix_scale[p], &lds.jac[0][lane], kHornLanes, r);
        } else {
            const float nan = __int_as_float(0x7fc00000);
            for (int k = 0; k < 9; ++k) r.R[k] = nan;
            for (int k = 0; k < 3; ++k) r.t[k] = nan;
            r.s = nan;
            for (int k = 0; k < 12; ++k) r.T12[k] = r.T21[k] = nan;
        }
        for (int k = 0; k < 12; ++k) {
            lds.T[k][lane] = r.T12[k];
            lds.T[12 + k][lane] = r.T21[k];
        }
        orbx_ransac_hyp *o = hyp + hid;
        for (int k = 0; k < 9; ++k) o->R[k] = r.R[k];
        for (int k = 0; k < 3; ++k) o->t[k] = r.t[k];
        o->s = r.s;
    }
    __syncthreads();

    int inliers = 0;
    uint64_t *mrow = mask + mask_offsets[p] + (int64_t)(first + lane) * words;
    for (int w = 0; w < words; ++w) {
        const int i = (w << 6) + lane;
        const bool have = i < n;
        orbx_ransac_corr c;
        float u1o = 0.f, v1o = 0.f, u2o = 0.f, v2o = 0.f;
        if (have) {
            c = K[i];
            horn_own_projection(c.X1c, k1, u1o, v1o);
            horn_own_projection(c.X2c, k2, u2o, v2o);
        }
        uint64_t word = 0;
        for (int j = 0; j < count; ++j) {
            bool in = false;
            if (have) {
                float T12[12], T21[12];
                for (int k = 0; k < 12; ++k) {
                    T12[k] = lds.T[k][j];
                    T21[k] = lds.T[12 + k][j];
                }
                in = horn_inlier((const float *)T12, (const float *)T21, c, k1, k2, u1o, v1o, u2o, v2o);
            }
            const uint64_t b = __ballot(in);
            if (lane == j) word = b;
        }
        if (mine) {
            mrow[w] = word;
            inliers += __popcll(word);
        }
    }
    if (mine) hyp[hid].n_inliers = inliers;
}

__global__ void k_ransac_atan2(const double *y, const double *x, int count, double *out) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < count) out[i] = atan2(y[i], x[i]);
}

// Per-device workspace of the host entry points, kept across calls
ArenaWs &ransac_ws(int device) {
    static ArenaWs ws[64];
    return ws[device & 63];
}

}  // namespace
}  // namespace orbx

using namespace orbx;

extern "C" {

int orbx_sim3_ransac_batch_device(const orbx_sim3_camera *d_cam1, const orbx_sim3_camera *d_cam2,
                                  const int32_t *d_fix_scale, const orbx_ransac_corr *d_corr,
                                  const int32_t *d_corr_offsets, const int32_t *d_triples,
                                  const int32_t *d_hyp_offsets, const int64_t *d_mask_offsets, int nproblems,
                                  int max_hyp, orbx_ransac_hyp *d_hyp, uint64_t *d_mask, void *stream) {
    if (nproblems < 0 || max_hyp < 0 || nproblems > 65535) return ORBX_EINVAL;
    if (nproblems == 0 || max_hyp == 0) return ORBX_OK;
    if (!d_cam1 || !d_cam2 || !d_fix_scale || !d_corr || !d_corr_offsets || !d_triples || !d_hyp_offsets ||
        !d_mask_offsets || !d_hyp || !d_mask)
        return ORBX_EINVAL;
    const dim3 grid((max_hyp + kHornLanes - 1) / kHornLanes, nproblems);
    hipLaunchKernelGGL(k_sim3_ransac, grid, dim3(kHornLanes), 0, static_cast<hipStream_t>(stream), d_cam1, d_cam2,
                       d_fix_scale, d_corr, d_corr_offsets, d_triples, d_hyp_offsets, d_mask_offsets, nproblems,
                       d_hyp, d_mask);
    return hipGetLastError() == hipSuccess ? ORBX_OK : ORBX_EIO;
}

int orbx_sim3_ransac_batch(int device, const orbx_sim3_camera *cam1, const orbx_sim3_camera *cam2,
                           const int32_t *fix_scale, const orbx_ransac_corr *corr, const int32_t *corr_offsets,
                           const int32_t *triples, const int32_t *hyp_offsets, int nproblems, orbx_ransac_hyp *hyp,
                           uint64_t *mask) {
    if (nproblems < 0 || nproblems > 65535) return ORBX_EINVAL;
    if (nproblems == 0) return ORBX_OK;
    if (!cam1 || !cam2 || !fix_scale || !corr_offsets || !hyp_offsets || corr_offsets[0] != 0 || hyp_offsets[0] != 0)
        return ORBX_EINVAL;
    std::vector<int64_t> moff(nproblems + 1, 0);
    int max_hyp = 0;
    for (int p = 0; p < nproblems; ++p) {
        if (corr_offsets[p + 1] < corr_offsets[p] || hyp_offsets[p + 1] < hyp_offsets[p]) return ORBX_EINVAL;
        const int n = corr_offsets[p + 1] - corr_offsets[p], h = hyp_offsets[p + 1] - hyp_offsets[p];
        if (h > 0 && (n < 3 || !triples)) return ORBX_EINVAL;
        for (int64_t k = hyp_offsets[p]; k < hyp_offsets[p + 1]; ++k)
            if (!horn_triple_ok(triples + 3 * k, n)) return ORBX_EINVAL;
        moff[p + 1] = moff[p] + (int64_t)h * ((n + 63) / 64);
        max_hyp = std::max(max_hyp, h);
    }
    const size_t P = nproblems, N = corr_offsets[nproblems], Hn = hyp_offsets[nproblems], W = moff[nproblems];
    if (Hn == 0) return ORBX_OK;
    if (!corr || !hyp || !mask) return ORBX_EINVAL;
    if (hipSetDevice(device) != hipSuccess) return ORBX_ENODEV;
    ArenaWs &ws = ransac_ws(device);
    std::lock_guard<std::mutex> lock(ws.mu);
    // arena: inputs (one upload), then outputs (one download)
    Layout L;
    const size_t o_c1 = L.add(sizeof(orbx_sim3_camera) * P), o_c2 = L.add(sizeof(orbx_sim3_camera) * P);
    const size_t o_fix = L.add(4 * P), o_co = L.add(4 * (P + 1)), o_ho = L.add(4 * (P + 1)), o_mo = L.add(8 * (P + 1));
    const size_t o_corr = L.add(sizeof(orbx_ransac_corr) * N), o_tri = L.add(12 * Hn);
    const size_t in_end = L.size;
    const size_t o_hyp = L.add(sizeof(orbx_ransac_hyp) * Hn), o_mask = L.add(8 * (W + 1));
    int rc = ws_reserve(ws, L.size);
    if (rc) return rc;
    put(ws, o_c1, cam1, sizeof(orbx_sim3_camera) * P);
    put(ws, o_c2, cam2, sizeof(orbx_sim3_camera) * P);
    put(ws, o_fix, fix_scale, 4 * P);
    put(ws, o_co, corr_offsets, 4 * (P + 1));
    put(ws, o_ho, hyp_offsets, 4 * (P + 1));
    put(ws, o_mo, moff.data(), 8 * (P + 1));
    put(ws, o_corr, corr, sizeof(orbx_ransac_corr) * N);
    put(ws, o_tri, triples, 12 * Hn);
    if (hipMemcpyAsync(ws.dev, ws.host, in_end, hipMemcpyHostToDevice, ws.st) != hipSuccess) return ORBX_EIO;
    uint8_t *d = ws.dev;
    rc = orbx_sim3_ransac_batch_device(at<orbx_sim3_camera>(d, o_c1), at<orbx_sim3_camera>(d, o_c2),
                                       at<int32_t>(d, o_fix), at<orbx_ransac_corr>(d, o_corr), at<int32_t>(d, o_co),
                                       at<int32_t>(d, o_tri), at<int32_t>(d, o_ho), at<int64_t>(d, o_mo), nproblems,
                                       max_hyp, at<orbx_ransac_hyp>(d, o_hyp), at<uint64_t>(d, o_mask), ws.st);
    if (rc) return rc;
    if (hipMemcpyAsync(ws.host + o_hyp, d + o_hyp, L.size - o_hyp, hipMemcpyDeviceToHost, ws.st) != hipSuccess ||
        hipStreamSynchronize(ws.st) != hipSuccess)
        return ORBX_EIO;
    get(ws, o_hyp, hyp, sizeof(orbx_ransac_hyp) * Hn);
    get(ws, o_mask, mask, 8 * W);
    return ORBX_OK;
}

int orbx_sim3_ransac(int device, const orbx_sim3_camera *cam1, const orbx_sim3_camera *cam2, int fix_scale,
                     const orbx_ransac_corr *corr, int n, const int32_t *triples, int h, orbx_ransac_hyp *hyp,
                     uint64_t *mask) {
    if (n < 0 || h < 0) return ORBX_EINVAL;
    const int32_t co[2] = {0, n}, ho[2] = {0, h}, fix = fix_scale;
    return orbx_sim3_ransac_batch(device, cam1, cam2, &fix, corr, co, triples, ho, 1, hyp, mask);
}

int orbx_sim3_ransac_debug_atan2(int device, const double *y, const double *x, int count, double *out) {
    if (count < 0) return ORBX_EINVAL;
    if (count == 0) return ORBX_OK;
    if (!y || !x || !out) return ORBX_EINVAL;
    if (hipSetDevice(device) != hipSuccess) return ORBX_ENODEV;
    ArenaWs &ws = ransac_ws(device);
    std::lock_guard<std::mutex> lock(ws.mu);
    const size_t C = count;
    Layout L;
    const size_t o_y = L.add(8 * C), o_x = L.add(8 * C), in_end = L.size, o_out = L.add(8 * C);
    int rc = ws_reserve(ws, L.size);
    if (rc) return rc;
    put(ws, o_y, y, 8 * C);
    put(ws, o_x, x, 8 * C);
    if (hipMemcpyAsync(ws.dev, ws.host, in_end, hipMemcpyHostToDevice, ws.st) != hipSuccess) return ORBX_EIO;
    uint8_t *d = ws.dev;
    hipLaunchKernelGGL(k_ransac_atan2, dim3((count + 255) / 256), dim3(256), 0, ws.st, at<double>(d, o_y),
                       at<double>(d, o_x), count, at<double>(d, o_out));
    if (hipGetLastError() != hipSuccess) return ORBX_EIO;
    if (hipMemcpyAsync(ws.host + o_out, d + o_out, 8 * C, hipMemcpyDeviceToHost, ws.st) != hipSuccess ||
        hipStreamSynchronize(ws.st) != hipSuccess)
        return ORBX_EIO;
    get(ws, o_out, out, 8 * C);
    return ORBX_OK;
}

}  // extern "C"
