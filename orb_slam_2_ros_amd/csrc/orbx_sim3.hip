// orbx_sim3.hip -- Optimizer::OptimizeSim3 (Optimizer.cc:1177-1414) on gfx950:
// g2o's Levenberg-Marquardt over one free VertexSim3Expmap and, per
// correspondence, an EdgeSim3ProjectXYZ and an EdgeInverseSim3ProjectXYZ with
// Huber kernels, two rounds with the classification between them.  The edges
// have no analytic Jacobian in the reference, so g2o differentiates them
// numerically (central differences, delta = 1e-9), and so does this kernel:
// 30 projections per correspondence and linearisation.  DESIGN.md §3.14 is
// the numeric specification, orbx_sim3.h its text (shared with a host
// compile; the LM control, the solve and the lanes' fold are orbx_lm.h's, shared
// with orbx_pose.hip), tests/pyref_sim3.py its numpy restatement.
//
//   k_sim3_optimize   one wave (one 64-thread workgroup) per problem, the
//                     whole optimisation in the one launch.  Per
//                     linearisation lanes 0..14 form the estimate's 14
//                     perturbed estimates and the inverses of all 15 and put
//                     them in LDS; lane l then evaluates correspondences l,
//                     l + 64, ... against that table and keeps its 36 partial
//                     sums (H's upper triangle, b, the robust chi2) in
//                     registers; the partials meet in LDS, lane f adds column
//                     f in lane order, every lane reads the totals and runs
//                     the 7x7 solve, the update and the LM control itself.
//                     The control flow of a problem is uniform over its wave
//                     and nothing waits on another workgroup or on the host;
//                     every loop bound is a constant or n.
//   k_sim3_step       one linear system at a given active set and lambda
//   k_sim3_update     Sim3(x) * S for a list of update vectors (test hooks)
// All arithmetic is FP64, unfused (-ffp-contract=off).  The only state per
// correspondence between trials is the two chi2 arrays (an edge's last
// computed chi2) and the removal flags, all outputs, each element touched by
// lane i % 64 alone.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstring>
#include <mutex>

#include "orbx_device.h"
#include "orbx_sim3.h"
#include "orbx_ws.h"

namespace orbx {
namespace {

struct Sim3Lds {
    LmFoldLds<kSim3Sums> fold;
    Sim3 tab[kSim3Table], tabinv[kSim3Table];
};

// The device's executor of orbx_lm.h's lm_run and orbx_sim3.h's sim3_optimize
struct Sim3Wave {
    Sim3Problem pr;
    uint8_t *flags;
    int lane;
    Sim3Lds *lds;

    __device__ inline void build(const Sim3 &S, double *H, double *b, double *chi) {
        if (lane < kSim3Table) {   // the linearisation's table, once for the wave
            Sim3 a, ainv;
            sim3_table_entry(S, lane, pr.fix_scale, a, ainv);
            lds->tab[lane] = a;
            lds->tabinv[lane] = ainv;
        }
        __syncthreads();
        const Sim3TableRef ref = {lds->tab, lds->tabinv};
        double acc[kSim3Sums];
#pragma unroll
        for (int f = 0; f < kSim3Sums; ++f) acc[f] = 0.0;
        sim3_lane_build(pr, ref, lane, acc);
        double tot[kSim3Sums];
        // (the fold's barriers also keep the table until every lane is done with it)
        lm_fold<kSim3Sums>(lds->fold, acc, lane, tot);
        lm_unpack<7>(tot, H, b, chi);
    }

    __device__ inline double errors(const Sim3 &S) {
        Sim3 Sinv;
        sim3_inverse(S, Sinv);
        double acc[1] = {sim3_lane_errors(pr, S, Sinv, lane)};
        double tot[1];
        lm_fold<1>(lds->fold, acc, lane, tot);
        return tot[0];
    }

    __device__ inline void update(Sim3 &S, const double *x) { sim3_update(S, x, pr.fix_scale); }

    __device__ inline int classify(int mark) {
        int bad = 0;
        for (int base = 0; base < pr.n; base += kSim3Lanes) {
            const int i = base + lane;
            bool isbad = false;
            if (i < pr.n && flags[i] == 0) {
                isbad = pr.chi12[i] > pr.th2 || pr.chi21[i] > pr.th2;   // (a NaN stays an inlier)
                if (isbad) flags[i] = (uint8_t)mark;
            }
            bad += __popcll(__ballot(isbad));
        }
        return bad;
    }
};

__device__ inline Sim3 sim3_load(const orbx_sim3 *s) {
    Sim3 S;
    for (int k = 0; k < 4; ++k) S.q[k] = s->q[k];
    for (int k = 0; k < 3; ++k) S.t[k] = s->t[k];
    S.s = s->s;
    return S;
}

__device__ inline void sim3_store(const Sim3 &S, orbx_sim3 *o) {
    for (int k = 0; k < 4; ++k) o->q[k] = S.q[k];
    for (int k = 0; k < 3; ++k) o->t[k] = S.t[k];
    o->s = S.s;
}

__global__ __launch_bounds__(kSim3Lanes) void k_sim3_optimize(
    const orbx_sim3 *S12, const orbx_sim3_camera *cam1, const orbx_sim3_camera *cam2, const orbx_sim3_corr *corr,
    const int32_t *offsets, int nproblems, const float *th2, const int32_t *fix_scale, orbx_sim3 *S12_out,
    uint8_t *removed, double *chi2_12, double *chi2_21, int32_t *n_inliers, int32_t *iterations) {
    __shared__ Sim3Lds lds;
    const int p = blockIdx.x, lane = threadIdx.x;
    if (p >= nproblems) return;
    const int64_t o0 = offsets[p];
    const int n = (int)(offsets[p + 1] - o0);
    Sim3Wave ex;
    ex.pr.corr = corr + o0;
    ex.pr.n = n;
    ex.pr.flag = removed + o0;
    ex.pr.sense = false;
    ex.pr.chi12 = chi2_12 + o0;
    ex.pr.chi21 = chi2_21 + o0;
    ex.pr.c1 = sim3_cam(cam1[p]);
    ex.pr.c2 = sim3_cam(cam2[p]);
    sim3_problem_thresholds(ex.pr, th2[p]);
    ex.pr.fix_scale = fix_scale[p];
    ex.pr.robust = true;   // the kernels are set once and never removed: both rounds
    ex.flags = removed + o0;
    ex.lane = lane;
    ex.lds = &lds;
    for (int i = lane; i < n; i += kSim3Lanes) {   // (read back by this lane only)
        ex.flags[i] = 0;
        ex.pr.chi12[i] = 0.0;
        ex.pr.chi21[i] = 0.0;
    }
    const Sim3 S0 = sim3_load(S12 + p);
    Sim3 out;
    int nin, its[2];
    sim3_optimize(ex, S0, n, out, nin, its);
    if (lane == 0) {
        sim3_store(out, S12_out + p);
        n_inliers[p] = nin;
        if (iterations) {
            iterations[2 * (int64_t)p] = its[0];
            iterations[2 * (int64_t)p + 1] = its[1];
        }
    }
}

// res: H[49], b[7], x[7], chi2, solved (as a double)
__global__ __launch_bounds__(kSim3Lanes) void k_sim3_step(const orbx_sim3 *S12, const orbx_sim3_camera *cam1,
                                                          const orbx_sim3_camera *cam2, const orbx_sim3_corr *corr,
                                                          int n, float th2, int fix_scale, const uint8_t *active,
                                                          int robust, double lambda, double *chi2_12,
                                                          double *chi2_21, double *res) {
    __shared__ Sim3Lds lds;
    Sim3Wave ex;
    ex.pr.corr = corr;
    ex.pr.n = n;
    ex.pr.flag = active;
    ex.pr.sense = true;
    ex.pr.chi12 = chi2_12;
    ex.pr.chi21 = chi2_21;
    ex.pr.c1 = sim3_cam(*cam1);
    ex.pr.c2 = sim3_cam(*cam2);
    sim3_problem_thresholds(ex.pr, th2);
    ex.pr.fix_scale = fix_scale;
    ex.pr.robust = robust != 0;
    ex.flags = nullptr;
    ex.lane = threadIdx.x;
    ex.lds = &lds;
    double H[49], b[7], chi, x[7];
    ex.build(sim3_load(S12), H, b, &chi);
    const bool ok = lm_solve<7>(H, b, lambda, x);
    if (threadIdx.x == 0) {
        for (int j = 0; j < 49; ++j) res[j] = H[j];
        for (int j = 0; j < 7; ++j) res[49 + j] = b[j];
        for (int j = 0; j < 7; ++j) res[56 + j] = ok ? x[j] : 0.0;
        res[63] = chi;
        res[64] = ok ? 1.0 : 0.0;
    }
}

// One wave; lane l takes updates l, l + 64, ...
__global__ __launch_bounds__(kSim3Lanes) void k_sim3_update(const orbx_sim3 *S, const double *x, int count,
                                                            int fix_scale, orbx_sim3 *S_out) {
    for (int k = threadIdx.x; k < count; k += kSim3Lanes) {
        Sim3 s = sim3_load(S + k);
        double u[7];
        for (int j = 0; j < 7; ++j) u[j] = x[7 * (int64_t)k + j];
        sim3_update(s, u, fix_scale);
        sim3_store(s, S_out + k);
    }
}

// Per-device workspace of the host entry points, kept across calls
ArenaWs &sim3_ws(int device) {
    static ArenaWs ws[64];
    return ws[device & 63];
}

}  // namespace
}  // namespace orbx

using namespace orbx;

extern "C" {

int orbx_optimize_sim3_batch_device(const orbx_sim3 *d_S12, const orbx_sim3_camera *d_cam1,
                                    const orbx_sim3_camera *d_cam2, const orbx_sim3_corr *d_corr,
                                    const int32_t *d_offsets, int nproblems, const float *d_th2,
                                    const int32_t *d_fix_scale, orbx_sim3 *d_S12_out, uint8_t *d_removed,
                                    double *d_chi2_12, double *d_chi2_21, int32_t *d_n_inliers,
                                    int32_t *d_iterations, void *stream) {
    if (nproblems < 0) return ORBX_EINVAL;
    if (nproblems == 0) return ORBX_OK;
    if (!d_S12 || !d_cam1 || !d_cam2 || !d_corr || !d_offsets || !d_th2 || !d_fix_scale || !d_S12_out ||
        !d_removed || !d_chi2_12 || !d_chi2_21 || !d_n_inliers)
        return ORBX_EINVAL;
    hipLaunchKernelGGL(k_sim3_optimize, dim3(nproblems), dim3(kSim3Lanes), 0, static_cast<hipStream_t>(stream),
                       d_S12, d_cam1, d_cam2, d_corr, d_offsets, nproblems, d_th2, d_fix_scale, d_S12_out,
                       d_removed, d_chi2_12, d_chi2_21, d_n_inliers, d_iterations);
    return hipGetLastError() == hipSuccess ? ORBX_OK : ORBX_EIO;
}

int orbx_optimize_sim3_batch(int device, const orbx_sim3 *S12, const orbx_sim3_camera *cam1,
                             const orbx_sim3_camera *cam2, const orbx_sim3_corr *corr, const int32_t *offsets,
                             int nproblems, const float *th2, const int32_t *fix_scale, orbx_sim3 *S12_out,
                             uint8_t *removed, double *chi2_12, double *chi2_21, int *n_inliers, int *iterations) {
    if (nproblems < 0) return ORBX_EINVAL;
    if (nproblems == 0) return ORBX_OK;
    if (!S12 || !cam1 || !cam2 || !offsets || !th2 || !fix_scale || !S12_out || !n_inliers || offsets[0] != 0)
        return ORBX_EINVAL;
    for (int p = 0; p < nproblems; ++p)
        if (offsets[p + 1] < offsets[p]) return ORBX_EINVAL;
    const size_t P = nproblems, N = offsets[nproblems];
    if (N && (!corr || !removed)) return ORBX_EINVAL;
    if (hipSetDevice(device) != hipSuccess) return ORBX_ENODEV;
    ArenaWs &ws = sim3_ws(device);
    std::lock_guard<std::mutex> lock(ws.mu);
    // arena: inputs (one upload), then outputs (one download)
    Layout L;
    const size_t o_S = L.add(sizeof(orbx_sim3) * P), o_c1 = L.add(sizeof(orbx_sim3_camera) * P);
    const size_t o_c2 = L.add(sizeof(orbx_sim3_camera) * P), o_th = L.add(4 * P), o_fix = L.add(4 * P);
    const size_t o_off = L.add(4 * (P + 1)), o_corr = L.add(sizeof(orbx_sim3_corr) * (N + 1));
    const size_t in_end = L.size;
    const size_t o_So = L.add(sizeof(orbx_sim3) * P), o_ni = L.add(4 * P), o_it = L.add(8 * P);
    const size_t o_a = L.add(8 * (N + 1)), o_b = L.add(8 * (N + 1)), o_rm = L.add(N + 1);
    int rc = ws_reserve(ws, L.size);
    if (rc) return rc;
    put(ws, o_S, S12, sizeof(orbx_sim3) * P);
    put(ws, o_c1, cam1, sizeof(orbx_sim3_camera) * P);
    put(ws, o_c2, cam2, sizeof(orbx_sim3_camera) * P);
    put(ws, o_th, th2, 4 * P);
    put(ws, o_fix, fix_scale, 4 * P);
    put(ws, o_off, offsets, 4 * (P + 1));
    put(ws, o_corr, corr, sizeof(orbx_sim3_corr) * N);
    if (hipMemcpyAsync(ws.dev, ws.host, in_end, hipMemcpyHostToDevice, ws.st) != hipSuccess) return ORBX_EIO;
    uint8_t *d = ws.dev;
    rc = orbx_optimize_sim3_batch_device(at<orbx_sim3>(d, o_S), at<orbx_sim3_camera>(d, o_c1),
                                         at<orbx_sim3_camera>(d, o_c2), at<orbx_sim3_corr>(d, o_corr),
                                         at<int32_t>(d, o_off), nproblems, at<float>(d, o_th), at<int32_t>(d, o_fix),
                                         at<orbx_sim3>(d, o_So), d + o_rm, at<double>(d, o_a), at<double>(d, o_b),
                                         at<int32_t>(d, o_ni), at<int32_t>(d, o_it), ws.st);
    if (rc) return rc;
    if (hipMemcpyAsync(ws.host + o_So, d + o_So, L.size - o_So, hipMemcpyDeviceToHost, ws.st) != hipSuccess ||
        hipStreamSynchronize(ws.st) != hipSuccess)
        return ORBX_EIO;
    get(ws, o_So, S12_out, sizeof(orbx_sim3) * P);
    get(ws, o_ni, n_inliers, 4 * P);
    get(ws, o_it, iterations, 8 * P);
    get(ws, o_a, chi2_12, 8 * N);
    get(ws, o_b, chi2_21, 8 * N);
    get(ws, o_rm, removed, N);
    return ORBX_OK;
}

int orbx_optimize_sim3(int device, const orbx_sim3 *S12, const orbx_sim3_camera *cam1, const orbx_sim3_camera *cam2,
                       const orbx_sim3_corr *corr, int n, float th2, int fix_scale, orbx_sim3 *S12_out,
                       uint8_t *removed, double *chi2_12, double *chi2_21, int *n_inliers, int *iterations) {
    if (n < 0) return ORBX_EINVAL;
    const int32_t offsets[2] = {0, n}, fix = fix_scale;
    return orbx_optimize_sim3_batch(device, S12, cam1, cam2, corr, offsets, 1, &th2, &fix, S12_out, removed, chi2_12,
                                    chi2_21, n_inliers, iterations);
}

int orbx_sim3_debug_step(int device, const orbx_sim3 *S12, const orbx_sim3_camera *cam1,
                         const orbx_sim3_camera *cam2, const orbx_sim3_corr *corr, int n, float th2, int fix_scale,
                         const uint8_t *active, int robust, double lambda, double *H_out, double *b_out,
                         double *x_out, double *chi2_out, int *solved) {
    if (n < 0 || !S12 || !cam1 || !cam2 || (n && !corr) || !H_out || !b_out || !x_out || !chi2_out || !solved)
        return ORBX_EINVAL;
    if (hipSetDevice(device) != hipSuccess) return ORBX_ENODEV;
    ArenaWs &ws = sim3_ws(device);
    std::lock_guard<std::mutex> lock(ws.mu);
    const size_t N = n;
    Layout L;
    const size_t o_S = L.add(sizeof(orbx_sim3)), o_c1 = L.add(sizeof(orbx_sim3_camera));
    const size_t o_c2 = L.add(sizeof(orbx_sim3_camera)), o_corr = L.add(sizeof(orbx_sim3_corr) * (N + 1));
    const size_t o_act = L.add(N + 1), in_end = L.size;
    const size_t o_res = L.add(8 * 65), o_a = L.add(8 * (N + 1)), o_b = L.add(8 * (N + 1));
    int rc = ws_reserve(ws, L.size);
    if (rc) return rc;
    put(ws, o_S, S12, sizeof(orbx_sim3));
    put(ws, o_c1, cam1, sizeof(orbx_sim3_camera));
    put(ws, o_c2, cam2, sizeof(orbx_sim3_camera));
    put(ws, o_corr, corr, sizeof(orbx_sim3_corr) * N);
    put(ws, o_act, active, N);
    if (hipMemcpyAsync(ws.dev, ws.host, in_end, hipMemcpyHostToDevice, ws.st) != hipSuccess) return ORBX_EIO;
    uint8_t *d = ws.dev;
    hipLaunchKernelGGL(k_sim3_step, dim3(1), dim3(kSim3Lanes), 0, ws.st, at<orbx_sim3>(d, o_S),
                       at<orbx_sim3_camera>(d, o_c1), at<orbx_sim3_camera>(d, o_c2), at<orbx_sim3_corr>(d, o_corr), n,
                       th2, fix_scale, active ? static_cast<const uint8_t *>(d + o_act) : nullptr, robust, lambda,
                       at<double>(d, o_a), at<double>(d, o_b), at<double>(d, o_res));
    if (hipGetLastError() != hipSuccess) return ORBX_EIO;
    if (hipMemcpyAsync(ws.host + o_res, d + o_res, 8 * 65, hipMemcpyDeviceToHost, ws.st) != hipSuccess ||
        hipStreamSynchronize(ws.st) != hipSuccess)
        return ORBX_EIO;
    const double *res = at<double>(ws.host, o_res);
    std::memcpy(H_out, res, 8 * 49);
    std::memcpy(b_out, res + 49, 8 * 7);
    std::memcpy(x_out, res + 56, 8 * 7);
    *chi2_out = res[63];
    *solved = res[64] != 0.0;
    return ORBX_OK;
}

int orbx_sim3_debug_update(int device, const orbx_sim3 *S, const double *x, int count, int fix_scale,
                           orbx_sim3 *S_out) {
    if (count < 0) return ORBX_EINVAL;
    if (count == 0) return ORBX_OK;
    if (!S || !x || !S_out) return ORBX_EINVAL;
    if (hipSetDevice(device) != hipSuccess) return ORBX_ENODEV;
    ArenaWs &ws = sim3_ws(device);
    std::lock_guard<std::mutex> lock(ws.mu);
    const size_t C = count;
    Layout L;
    const size_t o_S = L.add(sizeof(orbx_sim3) * C), o_x = L.add(56 * C), in_end = L.size;
    const size_t o_out = L.add(sizeof(orbx_sim3) * C);
    int rc = ws_reserve(ws, L.size);
    if (rc) return rc;
    put(ws, o_S, S, sizeof(orbx_sim3) * C);
    put(ws, o_x, x, 56 * C);
    if (hipMemcpyAsync(ws.dev, ws.host, in_end, hipMemcpyHostToDevice, ws.st) != hipSuccess) return ORBX_EIO;
    uint8_t *d = ws.dev;
    hipLaunchKernelGGL(k_sim3_update, dim3(1), dim3(kSim3Lanes), 0, ws.st, at<orbx_sim3>(d, o_S), at<double>(d, o_x),
                       count, fix_scale, at<orbx_sim3>(d, o_out));
    if (hipGetLastError() != hipSuccess) return ORBX_EIO;
    if (hipMemcpyAsync(ws.host + o_out, d + o_out, sizeof(orbx_sim3) * C, hipMemcpyDeviceToHost, ws.st) !=
            hipSuccess ||
        hipStreamSynchronize(ws.st) != hipSuccess)
        return ORBX_EIO;
    get(ws, o_out, S_out, sizeof(orbx_sim3) * C);
    return ORBX_OK;
}

}  // extern "C"
