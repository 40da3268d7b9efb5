// orbx_pose.hip -- Optimizer::PoseOptimization (Optimizer.cc:265-509) on
// gfx950: g2o's Levenberg-Marquardt (optimization_algorithm_levenberg.cpp:
// 60-160) over one free VertexSE3Expmap and the frame's
// EdgeSE3ProjectXYZOnlyPose / EdgeStereoSE3ProjectXYZOnlyPose edges
// (types_six_dof_expmap.cpp:266-364) with Huber kernels, four rounds with the
// inlier / outlier classification between them.  DESIGN.md §3.13 is the
// numeric specification; tests/pyref_pose.py restates it in numpy.  This file
// holds the edges (errors, Jacobians), the rounds and the host entry points;
// the LM control, Huber, the edge's sums, the 6x6 solve and the lanes' fold are
// orbx_lm.h's with N = 6 (shared with Sim3 optimisation), which PoseWave feeds.
//
//   k_pose_optimize   one wave (one 64-thread workgroup) per problem, the
//                     whole optimisation in the one launch: lane l evaluates
//                     observations l, l + 64, ... and keeps its 28 partial
//                     sums (H's upper triangle, b, the robust chi2) in
//                     registers; the partials meet in LDS, lane f adds column
//                     f in lane order, every lane reads the totals and runs
//                     the 6x6 solve, the update and the LM control itself.
//                     The control flow of a problem is uniform over its wave
//                     and nothing waits on another workgroup or on the host;
//                     every loop bound is a constant or n.
//   k_pose_step       one linear system at a given active set and lambda
//                     (test hook), the same device functions.
// All arithmetic is FP64, unfused (-ffp-contract=off), every sum in the fixed
// order of §3.13, so a run is deterministic and equals the numpy restatement.
// The only per-observation state between trials is the chi2 array (an
// observation's last computed chi2) and the outlier flags, both outputs.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstring>
#include <mutex>
#include <vector>

#include "orbx_device.h"
#include "orbx_lm.h"
#include "orbx_se3.h"
#include "orbx_ws.h"

namespace orbx {
namespace {

constexpr int kPoseLanes = kLmLanes;
constexpr int kPoseSums = lm_sums(6);   // H(a, b) a <= b: 21, b: 6, robust chi2: 1

struct PoseCam {
    double fx, fy, cx, cy, bf;
};

using PoseLds = LmFoldLds<kPoseSums>;

// One problem as the device functions see it.  An observation is active iff
// (flag[i] != 0) == sense: the outlier flags with sense = false, or the step
// hook's active array with sense = true (flag == nullptr: all active).
struct PoseProblem {
    const orbx_pose_obs *obs;
    int n;
    const uint8_t *flag;
    bool sense;
    double *chi2;
    PoseCam cam;
};

__device__ inline bool pose_active(const PoseProblem &pr, int i) {
    return !pr.flag || ((pr.flag[i] != 0) == pr.sense);
}

// computeError of an edge at T: the camera point p, the error, and chi2 =
// sum_k err_k (omega err_k).  D = 2 monocular, 3 stereo.
template <int D>
__device__ inline double pose_obs_error(const orbx_pose_obs &o, const PoseCam &c, const Pose &T, double *p,
                                        double *err) {
    const double X[3] = {o.Xw[0], o.Xw[1], o.Xw[2]};
    se3_map(T, X, p);
    if (D == 2) {
        const double u = p[0] / p[2], v = p[1] / p[2];   // project2d
        err[0] = (double)o.u - (u * c.fx + c.cx);
        err[1] = (double)o.v - (v * c.fy + c.cy);
    } else {
        const double invz = (double)(float)(1.0 / p[2]);   // const float invz = 1.0f/trans_xyz[2]
        const double r0 = p[0] * invz * c.fx + c.cx;
        const double r1 = p[1] * invz * c.fy + c.cy;
        err[0] = (double)o.u - r0;
        err[1] = (double)o.v - r1;
        err[2] = (double)o.ur - (r0 - c.bf * invz);
    }
    const double omega = o.inv_sigma2;
    double chi2 = 0;
#pragma unroll
    for (int k = 0; k < D; ++k) chi2 = chi2 + err[k] * (omega * err[k]);
    return chi2;
}

__device__ inline double pose_obs_chi2(const orbx_pose_obs &o, const PoseCam &c, const Pose &T) {
    double p[3], err[3];
    return o.ur < 0 ? pose_obs_error<2>(o, c, T, p, err) : pose_obs_error<3>(o, c, T, p, err);
}

// Huber's delta of an edge of dimension D
template <int D>
__device__ inline double pose_delta() {
    return D == 2 ? (double)(float)sqrt(5.991) : (double)(float)sqrt(7.815);
}

// One active observation's terms added to the lane's partials; its chi2
// returned.  The Jacobians are the OnlyPose edges' own (they multiply by
// invz = 1.0 / z where local BA's edges divide by z).
template <int D>
__device__ inline double pose_obs_terms(const orbx_pose_obs &o, const PoseCam &c, const Pose &T, bool robust,
                                        double *acc) {
    double p[3], err[3];
    const double chi2 = pose_obs_error<D>(o, c, T, p, err);
    double rho0, rho1;
    lm_huber(chi2, robust, pose_delta<D>(), rho0, rho1);
    const double x = p[0], y = p[1];
    const double invz = 1.0 / p[2];
    const double invz_2 = invz * invz;
    double J[D][6];
    J[0][0] = x * y * invz_2 * c.fx;
    J[0][1] = -(1 + (x * x * invz_2)) * c.fx;
    J[0][2] = y * invz * c.fx;
    J[0][3] = -invz * c.fx;
    J[0][4] = 0;
    J[0][5] = x * invz_2 * c.fx;
    J[1][0] = (1 + y * y * invz_2) * c.fy;
    J[1][1] = -x * y * invz_2 * c.fy;
    J[1][2] = -x * invz * c.fy;
    J[1][3] = 0;
    J[1][4] = -invz * c.fy;
    J[1][5] = y * invz_2 * c.fy;
    if (D == 3) {
        J[D - 1][0] = J[0][0] - c.bf * y * invz_2;
        J[D - 1][1] = J[0][1] + c.bf * x * invz_2;
        J[D - 1][2] = J[0][2];
        J[D - 1][3] = J[0][3];
        J[D - 1][4] = 0;
        J[D - 1][5] = J[0][5] - c.bf * invz_2;
    }
    lm_edge_sums(J, err, (double)o.inv_sigma2, rho0, rho1, acc);
    return chi2;
}

// The executor of orbx_lm.h's lm_run: one wave, lane l at observations l,
// l + 64, ...  (Its methods are forced inline, so that lm_run is optimised with
// the members as values and not as loads from the executor: inlined by cost,
// k_pose_optimize takes 255 VGPRs and 2 AGPRs, more than two waves per
// SIMD leave it.)
struct PoseWave {
    PoseProblem pr;
    bool robust;
    int lane;
    PoseLds *lds;

    // computeActiveErrors + buildSystem at T: H (6x6, mirrored), b and the
    // robust chi2 over the active observations
    __device__ __forceinline__ void build(const Pose &T, double *H, double *b, double *chi) {
        double acc[kPoseSums];
#pragma unroll
        for (int f = 0; f < kPoseSums; ++f) acc[f] = 0.0;
        for (int i = lane; i < pr.n; i += kPoseLanes) {
            if (!pose_active(pr, i)) continue;
            const orbx_pose_obs o = pr.obs[i];
            pr.chi2[i] = o.ur < 0 ? pose_obs_terms<2>(o, pr.cam, T, robust, acc)
                                  : pose_obs_terms<3>(o, pr.cam, T, robust, acc);
        }
        double tot[kPoseSums];
        lm_fold<kPoseSums>(*lds, acc, lane, tot);
        lm_unpack<6>(tot, H, b, chi);
    }

    // computeActiveErrors at T: the robust chi2 over the active observations
    __device__ __forceinline__ double errors(const Pose &T) {
        double acc[1] = {0.0};
        for (int i = lane; i < pr.n; i += kPoseLanes) {
            if (!pose_active(pr, i)) continue;
            const orbx_pose_obs o = pr.obs[i];
            double p[3], err[3], rho0, rho1;
            double chi2;
            if (o.ur < 0) {
                chi2 = pose_obs_error<2>(o, pr.cam, T, p, err);
                lm_huber(chi2, robust, pose_delta<2>(), rho0, rho1);
            } else {
                chi2 = pose_obs_error<3>(o, pr.cam, T, p, err);
                lm_huber(chi2, robust, pose_delta<3>(), rho0, rho1);
            }
            pr.chi2[i] = chi2;
            acc[0] = acc[0] + rho0;
        }
        double tot[1];
        lm_fold<1>(*lds, acc, lane, tot);
        return tot[0];
    }

    __device__ __forceinline__ void update(Pose &T, const double *x) { se3_exp_update(T, x); }
};

__device__ inline PoseCam pose_cam(const orbx_pose_camera &c) {
    PoseCam r;
    r.fx = c.fx; r.fy = c.fy; r.cx = c.cx; r.cy = c.cy; r.bf = c.bf;
    return r;
}

__global__ __launch_bounds__(kPoseLanes) void k_pose_optimize(
    const float *Tcw, const orbx_pose_camera *cams, const orbx_pose_obs *obs, const int32_t *offsets, int nproblems,
    float *Tcw_out, uint8_t *outlier, double *chi2, int32_t *n_inliers, int32_t *iterations) {
    __shared__ PoseLds lds;
    const int p = blockIdx.x, lane = threadIdx.x;
    if (p >= nproblems) return;
    const int64_t o0 = offsets[p];
    const int n = (int)(offsets[p + 1] - o0);
    uint8_t *out = outlier + o0;
    int its[4] = {0, 0, 0, 0};
    for (int i = lane; i < n; i += kPoseLanes) out[i] = 0;   // (read back by this lane only)
    if (n < 3) {   // the reference returns 0 before SetPose
        for (int i = lane; i < n; i += kPoseLanes) chi2[o0 + i] = 0.0;
        if (lane < 12) Tcw_out[12 * (int64_t)p + lane] = Tcw[12 * (int64_t)p + lane];
        if (lane == 0) {
            n_inliers[p] = 0;
            if (iterations)
                for (int r = 0; r < 4; ++r) iterations[4 * (int64_t)p + r] = 0;
        }
        return;
    }
    PoseWave ex;
    ex.pr.obs = obs + o0;
    ex.pr.n = n;
    ex.pr.flag = out;
    ex.pr.sense = false;
    ex.pr.chi2 = chi2 + o0;
    ex.pr.cam = pose_cam(cams[p]);
    ex.lane = lane;
    ex.lds = &lds;
    Pose T0;
    pose_from_cv(Tcw + 12 * (int64_t)p, T0);   // toSE3Quat(pFrame->mTcw)
    T0.free_idx = 0;
    T0.pad = 0;
    Pose T = T0;
    int nbad = 0;
    for (int r = 0; r < 4; ++r) {
        T = T0;   // setEstimate(toSE3Quat(mTcw)): every round starts at the initial pose
        ex.robust = r < 3;
        if (n - nbad > 0) its[r] = lm_run<6>(ex, T, 10);   // optimize(10)
        int bad = 0;
        for (int base = 0; base < n; base += kPoseLanes) {
            const int i = base + lane;
            bool isbad = false;
            if (i < n) {
                const orbx_pose_obs o = ex.pr.obs[i];
                double c;
                if (out[i]) {   // computeError() at the round's estimate
                    c = pose_obs_chi2(o, ex.pr.cam, T);
                    ex.pr.chi2[i] = c;
                } else {
                    c = ex.pr.chi2[i];   // e->chi2() as last computed
                }
                isbad = o.ur < 0 ? (float)c > 5.991f : (float)c > 7.815f;
                out[i] = isbad;
            }
            bad += __popcll(__ballot(isbad));
        }
        nbad = bad;
        if (n < 10) break;   // optimizer.edges().size() < 10
    }
    if (lane == 0) {
        pose_to_cv(T, Tcw_out + 12 * (int64_t)p);
        n_inliers[p] = n - nbad;
        if (iterations)
            for (int r = 0; r < 4; ++r) iterations[4 * (int64_t)p + r] = its[r];
    }
}

// out: H[36], b[6], x[6], chi2, solved (as a double)
__global__ __launch_bounds__(kPoseLanes) void k_pose_step(const float *Tcw, const orbx_pose_camera *cam,
                                                          const orbx_pose_obs *obs, int n, const uint8_t *active,
                                                          int robust, double lambda, double *chi2, double *res) {
    __shared__ PoseLds lds;
    const int lane = threadIdx.x;
    PoseWave ex;
    ex.pr.obs = obs;
    ex.pr.n = n;
    ex.pr.flag = active;
    ex.pr.sense = true;
    ex.pr.chi2 = chi2;
    ex.pr.cam = pose_cam(*cam);
    ex.robust = robust != 0;
    ex.lane = lane;
    ex.lds = &lds;
    Pose T;
    pose_from_cv(Tcw, T);
    T.free_idx = 0;
    T.pad = 0;
    double H[36], b[6], chi, x[6] = {0, 0, 0, 0, 0, 0};
    ex.build(T, H, b, &chi);
    double xs[6];
    const bool ok = lm_solve<6>(H, b, lambda, xs);
    if (ok)
        for (int j = 0; j < 6; ++j) x[j] = xs[j];
    if (lane == 0) {
        for (int j = 0; j < 36; ++j) res[j] = H[j];
        for (int j = 0; j < 6; ++j) res[36 + j] = b[j];
        for (int j = 0; j < 6; ++j) res[42 + j] = x[j];
        res[48] = chi;
        res[49] = ok ? 1.0 : 0.0;
    }
}

// Per-device workspace of the host entry points, kept across calls (tracking
// calls PoseOptimization once or twice per frame)
ArenaWs &pose_ws(int device) {
    static ArenaWs ws[64];
    return ws[device & 63];
}

}  // namespace
}  // namespace orbx

using namespace orbx;

extern "C" {

int orbx_pose_optimization_batch_device(const float *d_Tcw, const orbx_pose_camera *d_cams,
                                        const orbx_pose_obs *d_obs, const int32_t *d_offsets, int nproblems,
                                        float *d_Tcw_out, uint8_t *d_outlier, double *d_chi2, int32_t *d_n_inliers,
                                        int32_t *d_iterations, void *stream) {
    if (nproblems < 0) return ORBX_EINVAL;
    if (nproblems == 0) return ORBX_OK;
    if (!d_Tcw || !d_cams || !d_obs || !d_offsets || !d_Tcw_out || !d_outlier || !d_chi2 || !d_n_inliers)
        return ORBX_EINVAL;
    hipLaunchKernelGGL(k_pose_optimize, dim3(nproblems), dim3(kPoseLanes), 0, static_cast<hipStream_t>(stream),
                       d_Tcw, d_cams, d_obs, d_offsets, nproblems, d_Tcw_out, d_outlier, d_chi2, d_n_inliers,
                       d_iterations);
    return hipGetLastError() == hipSuccess ? ORBX_OK : ORBX_EIO;
}

int orbx_pose_optimization_batch(int device, const float *Tcw, const orbx_pose_camera *cams, const orbx_pose_obs *obs,
                                 const int32_t *offsets, int nproblems, float *Tcw_out, uint8_t *outlier,
                                 double *chi2, int *n_inliers, int *iterations) {
    if (nproblems < 0) return ORBX_EINVAL;
    if (nproblems == 0) return ORBX_OK;
    if (!Tcw || !cams || !offsets || !Tcw_out || !n_inliers || offsets[0] != 0) return ORBX_EINVAL;
    for (int p = 0; p < nproblems; ++p)
        if (offsets[p + 1] < offsets[p]) return ORBX_EINVAL;
    const size_t P = nproblems, N = offsets[nproblems];
    if (N && (!obs || !outlier)) return ORBX_EINVAL;
    if (hipSetDevice(device) != hipSuccess) return ORBX_ENODEV;
    ArenaWs &ws = pose_ws(device);
    std::lock_guard<std::mutex> lock(ws.mu);
    // arena: inputs (one upload), then outputs (one download)
    Layout L;
    const size_t o_T = L.add(48 * P), o_cam = L.add(sizeof(orbx_pose_camera) * P), o_off = L.add(4 * (P + 1));
    const size_t o_obs = L.add(sizeof(orbx_pose_obs) * (N + 1)), in_end = L.size;
    const size_t o_To = L.add(48 * P), o_ni = L.add(4 * P), o_it = L.add(16 * P);
    const size_t o_chi = L.add(8 * (N + 1)), o_out = L.add(N + 1);
    int rc = ws_reserve(ws, L.size);
    if (rc) return rc;
    put(ws, o_T, Tcw, 48 * P);
    put(ws, o_cam, cams, sizeof(orbx_pose_camera) * P);
    put(ws, o_off, offsets, 4 * (P + 1));
    put(ws, o_obs, obs, sizeof(orbx_pose_obs) * N);
    if (hipMemcpyAsync(ws.dev, ws.host, in_end, hipMemcpyHostToDevice, ws.st) != hipSuccess) return ORBX_EIO;
    uint8_t *d = ws.dev;
    rc = orbx_pose_optimization_batch_device(at<float>(d, o_T), at<orbx_pose_camera>(d, o_cam),
                                             at<orbx_pose_obs>(d, o_obs), at<int32_t>(d, o_off), nproblems,
                                             at<float>(d, o_To), d + o_out, at<double>(d, o_chi),
                                             at<int32_t>(d, o_ni), at<int32_t>(d, o_it), ws.st);
    if (rc) return rc;
    if (hipMemcpyAsync(ws.host + o_To, d + o_To, L.size - o_To, hipMemcpyDeviceToHost, ws.st) != hipSuccess ||
        hipStreamSynchronize(ws.st) != hipSuccess)
        return ORBX_EIO;
    get(ws, o_To, Tcw_out, 48 * P);
    get(ws, o_ni, n_inliers, 4 * P);
    get(ws, o_it, iterations, 16 * P);
    get(ws, o_chi, chi2, 8 * N);
    get(ws, o_out, outlier, N);
    return ORBX_OK;
}

int orbx_pose_optimization(int device, const float *Tcw, const orbx_pose_camera *cam, const orbx_pose_obs *obs, int n,
                           float *Tcw_out, uint8_t *outlier, double *chi2, int *n_inliers, int *iterations) {
    if (n < 0) return ORBX_EINVAL;
    const int32_t offsets[2] = {0, n};
    return orbx_pose_optimization_batch(device, Tcw, cam, obs, offsets, 1, Tcw_out, outlier, chi2, n_inliers,
                                        iterations);
}

int orbx_pose_debug_step(int device, const float *Tcw, const orbx_pose_camera *cam, const orbx_pose_obs *obs, int n,
                         const uint8_t *active, int robust, double lambda, double *H_out, double *b_out,
                         double *x_out, double *chi2_out, int *solved) {
    if (n < 0 || !Tcw || !cam || (n && !obs) || !H_out || !b_out || !x_out || !chi2_out || !solved)
        return ORBX_EINVAL;
    if (hipSetDevice(device) != hipSuccess) return ORBX_ENODEV;
    ArenaWs &ws = pose_ws(device);
    std::lock_guard<std::mutex> lock(ws.mu);
    const size_t N = n;
    Layout L;
    const size_t o_T = L.add(48), o_cam = L.add(sizeof(orbx_pose_camera));
    const size_t o_obs = L.add(sizeof(orbx_pose_obs) * (N + 1)), o_act = L.add(N + 1), in_end = L.size;
    const size_t o_res = L.add(8 * 50), o_chi = L.add(8 * (N + 1));
    int rc = ws_reserve(ws, L.size);
    if (rc) return rc;
    put(ws, o_T, Tcw, 48);
    put(ws, o_cam, cam, sizeof(orbx_pose_camera));
    put(ws, o_obs, obs, sizeof(orbx_pose_obs) * N);
    put(ws, o_act, active, N);
    if (hipMemcpyAsync(ws.dev, ws.host, in_end, hipMemcpyHostToDevice, ws.st) != hipSuccess) return ORBX_EIO;
    uint8_t *d = ws.dev;
    hipLaunchKernelGGL(k_pose_step, dim3(1), dim3(kPoseLanes), 0, ws.st, at<float>(d, o_T),
                       at<orbx_pose_camera>(d, o_cam), at<orbx_pose_obs>(d, o_obs), n,
                       active ? static_cast<const uint8_t *>(d + o_act) : nullptr, robust, lambda,
                       at<double>(d, o_chi), at<double>(d, o_res));
    if (hipGetLastError() != hipSuccess) return ORBX_EIO;
    if (hipMemcpyAsync(ws.host + o_res, d + o_res, 8 * 50, hipMemcpyDeviceToHost, ws.st) != hipSuccess ||
        hipStreamSynchronize(ws.st) != hipSuccess)
        return ORBX_EIO;
    const double *res = at<double>(ws.host, o_res);
    std::memcpy(H_out, res, 8 * 36);
    std::memcpy(b_out, res + 36, 8 * 6);
    std::memcpy(x_out, res + 42, 8 * 6);
    *chi2_out = res[48];
    *solved = res[49] != 0.0;
    return ORBX_OK;
}

}  // extern "C"
