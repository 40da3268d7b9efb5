// orbx_lm.h -- g2o's Levenberg-Marquardt (optimization_algorithm_levenberg.cpp:
// 60-160) for one free vertex of N dimensions and fixed points, as DESIGN.md
// §3.13 specifies it: the one text of pose optimisation (orbx_pose.hip, N = 6),
// of Sim3 optimisation (orbx_sim3.h, N = 7) and of the latter's host compile.
// A problem keeps N (N + 1) / 2 + N + 1 sums: H's upper triangle row by row, b,
// the robust chi2.  Whatever depends on the vertex or on where the text runs is
// behind an executor X:
//   X::build(E, H, b, &chi)   the normal equations over the active set at E
//   X::errors(E)              the robust chi2 over the active set at E
//   X::update(E, x)           the vertex's oplus: E = exp(x) * E
// All arithmetic is FP64, unfused, every sum in §3.13's order with each term its
// own multiply, so every compile of this text gives the same bits.
// (orbx_ba.hip's lm_optimize is host-driven across kernels and stays its own.)
#pragma once

#include <hip/hip_runtime.h>

#include <cfloat>
#include <cmath>

namespace orbx {

constexpr int kLmLanes = 64;

constexpr int lm_sums(int n) { return n * (n + 1) / 2 + n + 1; }

// RobustKernelHuber::robustify (rho0, rho1); without a kernel (chi2, 1)
__host__ __device__ inline void lm_huber(double chi2, bool robust, double delta, double &rho0, double &rho1) {
    rho0 = chi2;
    rho1 = 1.0;
    if (robust) {
        const double dsqr = delta * delta;
        if (!(chi2 <= dsqr)) {
            const double s = sqrt(chi2);
            rho0 = 2 * s * delta - dsqr;
            rho1 = delta / s;
        }
    }
}

// buildSystem's blocks of one edge (error dimension D) added to a lane's partials
template <int N, int D>
__host__ __device__ inline void lm_edge_sums(const double (&J)[D][N], const double *err, double omega, double rho0,
                                             double rho1, double *acc) {
    const double w = rho1 * omega;   // robustInformation
    double omr[D];
#pragma unroll
    for (int k = 0; k < D; ++k) omr[k] = -(omega * err[k]) * rho1;
    int idx = 0;
#pragma unroll
    for (int a = 0; a < N; ++a)
#pragma unroll
        for (int b = a; b < N; ++b) {
            double t = 0;
#pragma unroll
            for (int k = 0; k < D; ++k) t = t + (J[k][a] * w) * J[k][b];
            acc[idx] = acc[idx] + t;
            ++idx;
        }
#pragma unroll
    for (int a = 0; a < N; ++a) {
        double t = 0;
#pragma unroll
        for (int k = 0; k < D; ++k) t = t + J[k][a] * omr[k];
        acc[idx + a] = acc[idx + a] + t;
    }
    acc[idx + N] = acc[idx + N] + rho0;
}

// The folded sums as H (N x N, mirrored), b and the robust chi2
template <int N>
__host__ __device__ inline void lm_unpack(const double *tot, double *H, double *b, double *chi) {
    int idx = 0;
#pragma unroll
    for (int i = 0; i < N; ++i)
#pragma unroll
        for (int j = i; j < N; ++j) {
            H[N * i + j] = tot[idx];
            H[N * j + i] = tot[idx];
            ++idx;
        }
#pragma unroll
    for (int i = 0; i < N; ++i) b[i] = tot[idx + i];
    *chi = tot[idx + N];
}

// (H + lambda I) x = b by an N x N Cholesky, k_ba_chol's conventions: L column
// by column, each entry's terms in ascending k, each its own multiply and
// subtract; false if not positive definite
template <int N>
__host__ __device__ inline bool lm_solve(const double *H, const double *b, double lambda, double *x) {
    double L[N * N];
#pragma unroll
    for (int j = 0; j < N; ++j) {
        double d = H[N * j + j] + lambda;
#pragma unroll
        for (int k = 0; k < j; ++k) d = d - L[N * j + k] * L[N * j + k];
        if (!(d > 0)) return false;
        const double diag = sqrt(d);
        L[N * j + j] = diag;
#pragma unroll
        for (int i = j + 1; i < N; ++i) {
            double s = H[N * i + j];
#pragma unroll
            for (int k = 0; k < j; ++k) s = s - L[N * i + k] * L[N * j + k];
            L[N * i + j] = s / diag;
        }
    }
#pragma unroll
    for (int i = 0; i < N; ++i) {   // L y = b
        double s = b[i];
#pragma unroll
        for (int k = 0; k < i; ++k) s = s - L[N * i + k] * x[k];
        x[i] = s / L[N * i + i];
    }
#pragma unroll
    for (int i = N - 1; i >= 0; --i) {   // L^T x = y
        double s = x[i];
#pragma unroll
        for (int k = N - 1; k > i; --k) s = s - L[N * k + i] * x[k];
        x[i] = s / L[N * i + i];
    }
    return true;
}

// optimize(maxit) of one round, maxit <= 10: lm_optimize (orbx_ba.hip)
// statement for statement for one free vertex and no points.  Returns the
// iterations run.  A NaN falls through the comparisons as it does there and
// runs out the bounded loops.
template <int N, class X, class E>
__host__ __device__ inline int lm_run(X &ex, E &est, int maxit) {
    double lambda = 0, ni = 2, currentChi = 0;
    int nBad = 0;
    for (int it = 0; it < 10; ++it) {
        if (it >= maxit) return maxit;
        double H[N * N], b[N];
        ex.build(est, H, b, &currentChi);
        if (it == 0) {
            double mx = 0.;
#pragma unroll
            for (int j = 0; j < N; ++j) {   // std::max(fabs(H_jj), mx)
                const double a = fabs(H[(N + 1) * j]);
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
            double x[N];
            const bool ok = lm_solve<N>(H, b, lambda, x);
            const E bk = est;
            double tempChi = DBL_MAX;
            double sc = 0.0;
            if (ok) {   // (a failed solve leaves the estimate and the errors alone)
                ex.update(est, x);
                tempChi = ex.errors(est);
#pragma unroll
                for (int j = 0; j < N; ++j) sc += x[j] * (lambda * x[j] + b[j]);   // computeScale
            }
            rho = currentChi - tempChi;
            sc += 1e-3;
            rho /= sc;
            if (rho > 0 && std::isfinite(tempChi)) {
                const double t = 2 * rho - 1;
                double alpha = 1. - t * t * t;
                alpha = (2. / 3.) < alpha ? (2. / 3.) : alpha;                      // std::min(alpha, 2/3)
                const double scaleFactor = (1. / 3.) < alpha ? alpha : (1. / 3.);   // std::max(1/3, alpha)
                lambda *= scaleFactor;
                ni = 2;
                currentChi = tempChi;
            } else {
                lambda *= ni;
                ni *= 2;
                if (ok) est = bk;   // pop()
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

#ifdef __HIPCC__
// Where the partials of a wave's lanes meet: SUMS is the executor's stride
template <int SUMS>
struct LmFoldLds {
    double part[kLmLanes * SUMS];
    double tot[SUMS];
};

// The first NF partials of the wave's lanes, added in lane order: tot[f] = ((P_0 + P_1) + P_2) + ... + P_63
template <int NF, int SUMS>
__device__ inline void lm_fold(LmFoldLds<SUMS> &s, const double *acc, int lane, double *tot) {
#pragma unroll
    for (int f = 0; f < NF; ++f) s.part[lane * SUMS + f] = acc[f];
    __syncthreads();
    if (lane < NF) {
        double a = s.part[lane];
        for (int l = 1; l < kLmLanes; ++l) a = a + s.part[l * SUMS + lane];
        s.tot[lane] = a;
    }
    __syncthreads();
#pragma unroll
    for (int f = 0; f < NF; ++f) tot[f] = s.tot[f];
    __syncthreads();   // (the next fold writes part and tot again)
}
#endif

}  // namespace orbx
