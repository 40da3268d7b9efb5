// orbx_pose.hip -- Optimizer::PoseOptimization (Optimizer.cc:265-509) on
// gfx950: g2o's Levenberg-Marquardt (optimization_algorithm_levenberg.cpp:
// 60-160) over one free VertexSE3Expmap and the frame's
// EdgeSE3ProjectXYZOnlyPose / EdgeStereoSE3ProjectXYZOnlyPose edges
// (types_six_dof_expmap.cpp:266-364) with Huber kernels, four rounds with the
// inlier / outlier classification between them.  DESIGN.md §3.13 is the
// numeric specification; tests/pyref_pose.py restates it in numpy.
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

#include <cfloat>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <mutex>
#include <vector>

#include "orbx_device.h"
#include "orbx_se3.h"

namespace orbx {
namespace {

constexpr int kPoseLanes = 64;
constexpr int kPoseSums = 28;   // H(a, b) a <= b: 21, b: 6, robust chi2: 1

struct PoseCam {
    double fx, fy, cx, cy, bf;
};

struct PoseLds {
    double part[kPoseLanes * kPoseSums];
    double tot[kPoseSums];
};

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

// The partials of the wave's lanes, added in lane order: tot[f] = ((P_0 + P_1) + P_2) + ... + P_63
template <int NF>
__device__ inline void pose_fold(PoseLds &s, const double *acc, int lane, double *tot) {
#pragma unroll
    for (int f = 0; f < NF; ++f) s.part[lane * kPoseSums + f] = acc[f];
    __syncthreads();
    if (lane < NF) {
        double a = s.part[lane];
        for (int l = 1; l < kPoseLanes; ++l) a = a + s.part[l * kPoseSums + lane];
        s.tot[lane] = a;
    }
    __syncthreads();
#pragma unroll
    for (int f = 0; f < NF; ++f) tot[f] = s.tot[f];
    __syncthreads();   // (the next fold writes part and tot again)
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

// RobustKernelHuber::robustify (rho0, rho1); without a kernel (chi2, 1)
template <int D>
__device__ inline void pose_huber(double chi2, bool robust, double &rho0, double &rho1) {
    rho0 = chi2;
    rho1 = 1.0;
    if (robust) {
        const double delta = D == 2 ? (double)(float)sqrt(5.991) : (double)(float)sqrt(7.815);
        const double dsqr = delta * delta;
        if (!(chi2 <= dsqr)) {
            const double s = sqrt(chi2);
            rho0 = 2 * s * delta - dsqr;
            rho1 = delta / s;
        }
    }
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
    pose_huber<D>(chi2, robust, rho0, rho1);
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
    const double omega = o.inv_sigma2;
    const double w = rho1 * omega;   // robustInformation
    double omr[D];
#pragma unroll
    for (int k = 0; k < D; ++k) omr[k] = -(omega * err[k]) * rho1;
    int idx = 0;
#pragma unroll
    for (int a = 0; a < 6; ++a)
#pragma unroll
        for (int b = a; b < 6; ++b) {
            double t = 0;
#pragma unroll
            for (int k = 0; k < D; ++k) t = t + (J[k][a] * w) * J[k][b];
            acc[idx] = acc[idx] + t;
            ++idx;
        }
#pragma unroll
    for (int a = 0; a < 6; ++a) {
        double t = 0;
#pragma unroll
        for (int k = 0; k < D; ++k) t = t + J[k][a] * omr[k];
        acc[21 + a] = acc[21 + a] + t;
    }
    acc[27] = acc[27] + rho0;
    return chi2;
}

// computeActiveErrors + buildSystem at T: H (6x6, mirrored), b and the
// robust chi2 over the active observations
__device__ inline void pose_build(const PoseProblem &pr, const Pose &T, bool robust, int lane, PoseLds &lds,
                                  double *H, double *b, double *chi) {
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
    pose_fold<kPoseSums>(lds, acc, lane, tot);
    int idx = 0;
#pragma unroll
    for (int a = 0; a < 6; ++a)
#pragma unroll
        for (int c = a; c < 6; ++c) {
            H[6 * a + c] = tot[idx];
            H[6 * c + a] = tot[idx];
            ++idx;
        }
#pragma unroll
    for (int a = 0; a < 6; ++a) b[a] = tot[21 + a];
    *chi = tot[27];
}

// computeActiveErrors at T: the robust chi2 over the active observations
__device__ inline double pose_errors(const PoseProblem &pr, const Pose &T, bool robust, int lane, PoseLds &lds) {
    double acc[1] = {0.0};
    for (int i = lane; i < pr.n; i += kPoseLanes) {
        if (!pose_active(pr, i)) continue;
        const orbx_pose_obs o = pr.obs[i];
        double p[3], err[3], rho0, rho1;
        double chi2;
        if (o.ur < 0) {
            chi2 = pose_obs_error<2>(o, pr.cam, T, p, err);
            pose_huber<2>(chi2, robust, rho0, rho1);
        } else {
            chi2 = pose_obs_error<3>(o, pr.cam, T, p, err);
            pose_huber<3>(chi2, robust, rho0, rho1);
        }
        pr.chi2[i] = chi2;
        acc[0] = acc[0] + rho0;
    }
    double tot[1];
    pose_fold<1>(lds, acc, lane, tot);
    return tot[0];
}

// (H + lambda I) x = b by a 6x6 Cholesky, k_ba_chol's conventions: L column
// by column, each entry's terms in ascending k, each its own multiply and
// subtract; false if not positive definite
__device__ inline bool pose_solve(const double *H, const double *b, double lambda, double *x) {
    double L[36];
#pragma unroll
    for (int j = 0; j < 6; ++j) {
        double d = H[6 * j + j] + lambda;
#pragma unroll
        for (int k = 0; k < j; ++k) d = d - L[6 * j + k] * L[6 * j + k];
        if (!(d > 0)) return false;
        const double diag = sqrt(d);
        L[6 * j + j] = diag;
#pragma unroll
        for (int i = j + 1; i < 6; ++i) {
            double s = H[6 * i + j];
#pragma unroll
            for (int k = 0; k < j; ++k) s = s - L[6 * i + k] * L[6 * j + k];
            L[6 * i + j] = s / diag;
        }
    }
#pragma unroll
    for (int i = 0; i < 6; ++i) {   // L y = b
        double s = b[i];
#pragma unroll
        for (int k = 0; k < i; ++k) s = s - L[6 * i + k] * x[k];
        x[i] = s / L[6 * i + i];
    }
#pragma unroll
    for (int i = 5; i >= 0; --i) {   // L^T x = y
        double s = x[i];
#pragma unroll
        for (int k = 5; k > i; --k) s = s - L[6 * k + i] * x[k];
        x[i] = s / L[6 * i + i];
    }
    return true;
}

// optimize(10) of one round: lm_optimize (orbx_ba.hip) statement for
// statement for one free vertex and no points.  Returns the iterations run.
// A NaN falls through the comparisons as it does there and runs out the
// bounded loops.
__device__ inline int pose_lm(const PoseProblem &pr, Pose &T, bool robust, int lane, PoseLds &lds) {
    double lambda = 0, ni = 2, currentChi = 0;
    int nBad = 0;
    for (int it = 0; it < 10; ++it) {
        double H[36], b[6];
        pose_build(pr, T, robust, lane, lds, H, b, &currentChi);
        if (it == 0) {
            double mx = 0.;
#pragma unroll
            for (int j = 0; j < 6; ++j) {   // std::max(fabs(H_jj), mx)
                const double a = fabs(H[7 * j]);
                mx = a < mx ? mx : a;
            }
            lambda = 1e-5 * mx;   // _tau * maxDiagonal
            ni = 2;
            nBad = 0;
        }
        const double iniChi = currentChi;
        double rho = 0;
        int qmax = 0;
        do {
            double x[6];
            const bool ok = pose_solve(H, b, lambda, x);
            Pose bk = T;
            double tempChi = DBL_MAX;
            double sc = 0.0;
            if (ok) {   // (a failed solve leaves the estimate and the errors alone)
                se3_exp_update(T, x);
                tempChi = pose_errors(pr, T, robust, lane, lds);
#pragma unroll
                for (int j = 0; j < 6; ++j) sc += x[j] * (lambda * x[j] + b[j]);   // computeScale
            }
            rho = currentChi - tempChi;
            sc += 1e-3;
            rho /= sc;
            if (rho > 0 && isfinite(tempChi)) {
                const double t = 2 * rho - 1;
                double alpha = 1. - t * t * t;
                alpha = (2. / 3.) < alpha ? (2. / 3.) : alpha;          // std::min(alpha, 2/3)
                const double scaleFactor = (1. / 3.) < alpha ? alpha : (1. / 3.);   // std::max(1/3, alpha)
                lambda *= scaleFactor;
                ni = 2;
                currentChi = tempChi;
            } else {
                lambda *= ni;
                ni *= 2;
                if (ok) T = bk;   // pop()
            }
            qmax++;
        } while (rho < 0 && qmax < 10);
        if (qmax == 10 || rho == 0) return it + 1;   // Terminate
        if ((iniChi - currentChi) * 1e3 < iniChi) nBad++;
        else nBad = 0;
        if (nBad >= 3) return it + 1;
    }
    return 10;
}

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
    PoseProblem pr;
    pr.obs = obs + o0;
    pr.n = n;
    pr.flag = out;
    pr.sense = false;
    pr.chi2 = chi2 + o0;
    pr.cam = pose_cam(cams[p]);
    Pose T0;
    pose_from_cv(Tcw + 12 * (int64_t)p, T0);   // toSE3Quat(pFrame->mTcw)
    T0.free_idx = 0;
    T0.pad = 0;
    Pose T = T0;
    int nbad = 0;
    for (int r = 0; r < 4; ++r) {
        T = T0;   // setEstimate(toSE3Quat(mTcw)): every round starts at the initial pose
        if (n - nbad > 0) its[r] = pose_lm(pr, T, r < 3, lane, lds);
        int bad = 0;
        for (int base = 0; base < n; base += kPoseLanes) {
            const int i = base + lane;
            bool isbad = false;
            if (i < n) {
                const orbx_pose_obs o = pr.obs[i];
                double c;
                if (out[i]) {   // computeError() at the round's estimate
                    c = pose_obs_chi2(o, pr.cam, T);
                    pr.chi2[i] = c;
                } else {
                    c = pr.chi2[i];   // e->chi2() as last computed
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
    PoseProblem pr;
    pr.obs = obs;
    pr.n = n;
    pr.flag = active;
    pr.sense = true;
    pr.chi2 = chi2;
    pr.cam = pose_cam(*cam);
    Pose T;
    pose_from_cv(Tcw, T);
    T.free_idx = 0;
    T.pad = 0;
    double H[36], b[6], chi, x[6] = {0, 0, 0, 0, 0, 0};
    pose_build(pr, T, robust != 0, lane, lds, H, b, &chi);
    double xs[6];
    const bool ok = pose_solve(H, b, lambda, xs);
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
// calls PoseOptimization once or twice per frame): the stream, a device arena
// and a pinned staging buffer, grown on demand.
struct PoseWs {
    std::mutex mu;
    hipStream_t st = nullptr;
    uint8_t *dev = nullptr, *host = nullptr;
    size_t cap = 0, hcap = 0;
};

PoseWs &pose_ws(int device) {
    static PoseWs ws[64];
    return ws[device & 63];
}

int pose_ws_reserve(PoseWs &ws, size_t bytes) {
    if (!ws.st && hipStreamCreateWithFlags(&ws.st, hipStreamNonBlocking) != hipSuccess) return ORBX_EIO;
    if (bytes > ws.cap) {
        if (ws.dev) (void)hipFree(ws.dev);
        ws.dev = nullptr;
        ws.cap = 0;
        if (hipMalloc(reinterpret_cast<void **>(&ws.dev), bytes) != hipSuccess) return ORBX_ENOMEM;
        ws.cap = bytes;
    }
    if (bytes > ws.hcap) {
        if (ws.host) (void)hipHostFree(ws.host);
        ws.host = nullptr;
        ws.hcap = 0;
        if (hipHostMalloc(reinterpret_cast<void **>(&ws.host), bytes, hipHostMallocDefault) != hipSuccess)
            return ORBX_ENOMEM;
        ws.hcap = bytes;
    }
    return ORBX_OK;
}

size_t pad256(size_t b) { return (b + 255) & ~size_t(255); }

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
    PoseWs &ws = pose_ws(device);
    std::lock_guard<std::mutex> lock(ws.mu);
    // arena: inputs (one upload), then outputs (one download)
    const size_t o_T = 0, o_cam = o_T + pad256(48 * P), o_off = o_cam + pad256(sizeof(orbx_pose_camera) * P);
    const size_t o_obs = o_off + pad256(4 * (P + 1)), in_end = o_obs + pad256(sizeof(orbx_pose_obs) * (N + 1));
    const size_t o_To = in_end, o_ni = o_To + pad256(48 * P), o_it = o_ni + pad256(4 * P);
    const size_t o_chi = o_it + pad256(16 * P), o_out = o_chi + pad256(8 * (N + 1)), end = o_out + pad256(N + 1);
    int rc = pose_ws_reserve(ws, end);
    if (rc) return rc;
    std::memcpy(ws.host + o_T, Tcw, 48 * P);
    std::memcpy(ws.host + o_cam, cams, sizeof(orbx_pose_camera) * P);
    std::memcpy(ws.host + o_off, offsets, 4 * (P + 1));
    if (N) std::memcpy(ws.host + o_obs, obs, sizeof(orbx_pose_obs) * N);
    if (hipMemcpyAsync(ws.dev, ws.host, in_end, hipMemcpyHostToDevice, ws.st) != hipSuccess) return ORBX_EIO;
    uint8_t *d = ws.dev;
    rc = orbx_pose_optimization_batch_device(
        reinterpret_cast<const float *>(d + o_T), reinterpret_cast<const orbx_pose_camera *>(d + o_cam),
        reinterpret_cast<const orbx_pose_obs *>(d + o_obs), reinterpret_cast<const int32_t *>(d + o_off), nproblems,
        reinterpret_cast<float *>(d + o_To), d + o_out, reinterpret_cast<double *>(d + o_chi),
        reinterpret_cast<int32_t *>(d + o_ni), reinterpret_cast<int32_t *>(d + o_it), ws.st);
    if (rc) return rc;
    if (hipMemcpyAsync(ws.host + o_To, d + o_To, end - o_To, hipMemcpyDeviceToHost, ws.st) != hipSuccess ||
        hipStreamSynchronize(ws.st) != hipSuccess)
        return ORBX_EIO;
    std::memcpy(Tcw_out, ws.host + o_To, 48 * P);
    std::memcpy(n_inliers, ws.host + o_ni, 4 * P);
    if (iterations) std::memcpy(iterations, ws.host + o_it, 16 * P);
    if (N && chi2) std::memcpy(chi2, ws.host + o_chi, 8 * N);
    if (N) std::memcpy(outlier, ws.host + o_out, N);
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
    PoseWs &ws = pose_ws(device);
    std::lock_guard<std::mutex> lock(ws.mu);
    const size_t N = n;
    const size_t o_T = 0, o_cam = o_T + 256, o_obs = o_cam + 256, o_act = o_obs + pad256(sizeof(orbx_pose_obs) * (N + 1));
    const size_t in_end = o_act + pad256(N + 1), o_res = in_end, o_chi = o_res + pad256(8 * 50);
    const size_t end = o_chi + pad256(8 * (N + 1));
    int rc = pose_ws_reserve(ws, end);
    if (rc) return rc;
    std::memcpy(ws.host + o_T, Tcw, 48);
    std::memcpy(ws.host + o_cam, cam, sizeof(orbx_pose_camera));
    if (N) std::memcpy(ws.host + o_obs, obs, sizeof(orbx_pose_obs) * N);
    if (N && active) std::memcpy(ws.host + o_act, active, N);
    if (hipMemcpyAsync(ws.dev, ws.host, in_end, hipMemcpyHostToDevice, ws.st) != hipSuccess) return ORBX_EIO;
    uint8_t *d = ws.dev;
    hipLaunchKernelGGL(k_pose_step, dim3(1), dim3(kPoseLanes), 0, ws.st, reinterpret_cast<const float *>(d + o_T),
                       reinterpret_cast<const orbx_pose_camera *>(d + o_cam),
                       reinterpret_cast<const orbx_pose_obs *>(d + o_obs), n,
                       active ? static_cast<const uint8_t *>(d + o_act) : nullptr, robust, lambda,
                       reinterpret_cast<double *>(d + o_chi), reinterpret_cast<double *>(d + o_res));
    if (hipGetLastError() != hipSuccess) return ORBX_EIO;
    if (hipMemcpyAsync(ws.host + o_res, d + o_res, 8 * 50, hipMemcpyDeviceToHost, ws.st) != hipSuccess ||
        hipStreamSynchronize(ws.st) != hipSuccess)
        return ORBX_EIO;
    const double *res = reinterpret_cast<const double *>(ws.host + o_res);
    std::memcpy(H_out, res, 8 * 36);
    std::memcpy(b_out, res + 36, 8 * 6);
    std::memcpy(x_out, res + 42, 8 * 6);
    *chi2_out = res[48];
    *solved = res[49] != 0.0;
    return ORBX_OK;
}

}  // extern "C"
