// orbx_sim3.h -- Optimizer::OptimizeSim3 (Optimizer.cc:1177-1414) as DESIGN.md
// §3.14 specifies it, in one text for the device (orbx_sim3.hip) and for a host
// compile (tools/sim3_host/sim3_host.cpp, the CPU figure and a CPU parity
// check): g2o's Sim3 (sim3.h) without its Eigen types, the two reprojection
// edges of a correspondence, their numeric Jacobians (base_binary_edge.hpp:
// 147-200, central differences with delta = 1e-9), the update and the two
// rounds.  The 7x7 system's sums, its Cholesky, Huber and the Levenberg-
// Marquardt control are orbx_lm.h's with N = 7, the text pose optimisation runs.
//
// Whatever differs between the device and the host is behind an executor X:
// orbx_lm.h's build / errors / update (update is sim3_update with the
// problem's fix_scale), and
//   X::classify(mark)         flags the active correspondences over th2
// The device's executor spreads the correspondences over the 64 lanes of a
// wave and folds the lanes' partials through LDS; the host's runs the lanes
// one after another.  Both add in §3.14's order, so they agree bit for bit.
#pragma once

#include <cmath>
#include <cstdint>

#include "orbx_lm.h"
#include "orbx_se3.h"
#include "../../include/orbx.h"

namespace orbx {

constexpr int kSim3Lanes = kLmLanes;
constexpr int kSim3Sums = lm_sums(7);   // H(a, b) a <= b: 28, b: 7, robust chi2: 1
constexpr int kSim3Table = 15;   // the estimate and its 14 perturbations

struct Sim3 {   // g2o::Sim3: r = (x, y, z, w) (never normalised), t, s
    double q[4];
    double t[3];
    double s;
};

struct Sim3Cam {
    double fx, fy, cx, cy;
};

// exp(+1e-9), exp(-1e-9): correctly rounded (glibc's values; §3.14)
constexpr double kSim3ExpPlus = 0x1.000000044b830p+0;
constexpr double kSim3ExpMinus = 0x1.fffffff768fa1p-1;
constexpr double kSim3Delta = 1e-9;

// The specification's exp (§3.14).  The device's exp and glibc's differ in the
// last bit on arguments an update reaches (exp(-0.4) is one), so the scale's
// exponential is this fixed sequence on every side: k = floor(x / ln 2 + 1/2),
// r = (x - k ln2_hi) - k ln2_lo (fdlibm's split of ln 2, |r| <= 0.347), the
// Taylor polynomial of degree 13 in Horner's form with coefficients 1 / n!
// (remainder below 4e-18 relative), scaled by 2^k.  floor and the scaling are
// exact; everything else is +, -, x, /.  Within about one unit in the last
// place of e^x, and exactly 1 at 0.
__host__ __device__ inline double sim3_exp_scalar(double x) {
    if (x != x) return x;
    if (x > 709.0) return HUGE_VAL;
    if (x < -745.0) return 0.0;
    const double kd = floor(x * 0x1.71547652b82fep+0 + 0.5);
    const double r = (x - kd * 0x1.62e42fee00000p-1) - kd * 0x1.a39ef35793c76p-33;
    const double f[14] = {1.0, 1.0, 2.0, 6.0, 24.0, 120.0, 720.0, 5040.0, 40320.0, 362880.0, 3628800.0,
                          39916800.0, 479001600.0, 6227020800.0};
    double p = 1.0 / f[13];
#pragma unroll
    for (int n = 12; n >= 0; --n) p = 1.0 / f[n] + r * p;
    return ldexp(p, (int)kd);
}

// R_to_quat's arithmetic (Eigen's Quaternion(const Matrix3&)) with the branch
// on the largest diagonal element written out, so that no index is dynamic
__host__ __device__ inline void sim3_R_to_quat(const double *m, double *q) {
    const double tr = m[0] + m[4] + m[8];
    if (tr > 0) {
        double t = sqrt(tr + 1.0);
        q[3] = 0.5 * t;
        t = 0.5 / t;
        q[0] = (m[7] - m[5]) * t;
        q[1] = (m[2] - m[6]) * t;
        q[2] = (m[3] - m[1]) * t;
        return;
    }
    int i = 0;
    if (m[4] > m[0]) i = 1;
    if (m[8] > (i == 1 ? m[4] : m[0])) i = 2;
    if (i == 0) {
        double t = sqrt(m[0] - m[4] - m[8] + 1.0);
        q[0] = 0.5 * t;
        t = 0.5 / t;
        q[3] = (m[7] - m[5]) * t;
        q[1] = (m[3] + m[1]) * t;
        q[2] = (m[6] + m[2]) * t;
    } else if (i == 1) {
        double t = sqrt(m[4] - m[8] - m[0] + 1.0);
        q[1] = 0.5 * t;
        t = 0.5 / t;
        q[3] = (m[2] - m[6]) * t;
        q[2] = (m[7] + m[5]) * t;
        q[0] = (m[1] + m[3]) * t;
    } else {
        double t = sqrt(m[8] - m[0] - m[4] + 1.0);
        q[2] = 0.5 * t;
        t = 0.5 / t;
        q[3] = (m[3] - m[1]) * t;
        q[0] = (m[2] + m[6]) * t;
        q[1] = (m[5] + m[7]) * t;
    }
}

// Sim3::map: s * (r * xyz) + t
__host__ __device__ inline void sim3_map(const Sim3 &S, const double *X, double *o) {
    double r[3];
    quat_rotate(S.q, X, r);
    for (int i = 0; i < 3; ++i) o[i] = S.s * r[i] + S.t[i];
}

// Sim3::inverse: (r.conjugate(), r.conjugate() * ((-1. / s) * t), 1. / s)
__host__ __device__ inline void sim3_inverse(const Sim3 &S, Sim3 &o) {
    const double qc[4] = {-S.q[0], -S.q[1], -S.q[2], S.q[3]};
    const double a = -1. / S.s;
    const double v[3] = {a * S.t[0], a * S.t[1], a * S.t[2]};
    double t[3];
    quat_rotate(qc, v, t);
    for (int i = 0; i < 4; ++i) o.q[i] = qc[i];
    for (int i = 0; i < 3; ++i) o.t[i] = t[i];
    o.s = 1. / S.s;
}

// Sim3::operator*: r = a.r * b.r, t = a.s * (a.r * b.t) + a.t, s = a.s * b.s
__host__ __device__ inline void sim3_mul(const Sim3 &a, const Sim3 &b, Sim3 &o) {
    double q[4], r[3];
    quat_mul(a.q, b.q, q);
    quat_rotate(a.q, b.t, r);
    const double s = a.s * b.s;
    for (int i = 0; i < 3; ++i) o.t[i] = a.s * r[i] + a.t[i];
    for (int i = 0; i < 4; ++i) o.q[i] = q[i];
    o.s = s;
}

// Sim3(const Vector7d &update) (sim3.h:70-142): u = (omega, upsilon, sigma)
__host__ __device__ inline void sim3_exp(const double *u, Sim3 &o) {
    const double w[3] = {u[0], u[1], u[2]}, ups[3] = {u[3], u[4], u[5]};
    const double sigma = u[6];
    const double theta = sqrt(w[0] * w[0] + w[1] * w[1] + w[2] * w[2]);
    const double Om[9] = {0, -w[2], w[1], w[2], 0, -w[0], -w[1], w[0], 0};
    const double s = sim3_exp_scalar(sigma);   // s = std::exp(sigma): §3.14's exp
    double O2[9];
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c) {
            double acc = 0;
            for (int k = 0; k < 3; ++k) acc = acc + Om[3 * r + k] * Om[3 * k + c];
            O2[3 * r + c] = acc;
        }
    const double eps = 0.00001;
    double A, B, C, R[9];
    const bool small = theta < eps;
    if (small) {
        for (int k = 0; k < 9; ++k) R[k] = ((k % 4 == 0) ? 1.0 : 0.0) + Om[k] + O2[k];
    } else {
        const double ra = sin(theta) / theta, rb = (1 - cos(theta)) / (theta * theta);
        for (int k = 0; k < 9; ++k) R[k] = ((k % 4 == 0) ? 1.0 : 0.0) + ra * Om[k] + rb * O2[k];
    }
    if (fabs(sigma) < eps) {
        C = 1;
        if (small) {
            A = 1. / 2.;
            B = 1. / 6.;
        } else {
            const double theta2 = theta * theta;
            A = (1 - cos(theta)) / (theta2);
            B = (theta - sin(theta)) / (theta2 * theta);
        }
    } else {
        C = (s - 1) / sigma;
        if (small) {
            const double sigma2 = sigma * sigma;
            A = ((sigma - 1) * s + 1) / sigma2;
            B = ((0.5 * sigma2 - sigma + 1) * s) / (sigma2 * sigma);
        } else {
            const double a = s * sin(theta);
            const double b = s * cos(theta);
            const double theta2 = theta * theta;
            const double sigma2 = sigma * sigma;
            const double c = theta2 + sigma2;
            A = (a * sigma + (1 - b) * theta) / (theta * c);
            B = (C - ((b - 1) * sigma + a * theta) / (c)) * 1. / (theta2);
        }
    }
    sim3_R_to_quat(R, o.q);
    double W[9];
    for (int k = 0; k < 9; ++k) W[k] = A * Om[k] + B * O2[k] + C * ((k % 4 == 0) ? 1.0 : 0.0);
    for (int r = 0; r < 3; ++r) o.t[r] = W[3 * r] * ups[0] + W[3 * r + 1] * ups[1] + W[3 * r + 2] * ups[2];
    o.s = s;
}

// VertexSim3Expmap::oplusImpl: S = Sim3(x) * S, x[6] zeroed first with a fixed scale
__host__ __device__ inline void sim3_update(Sim3 &S, const double *x, int fix_scale) {
    double u[7];
    for (int j = 0; j < 7; ++j) u[j] = x[j];
    if (fix_scale) u[6] = 0;
    Sim3 E, o;
    sim3_exp(u, E);
    sim3_mul(E, S, o);
    S = o;
}

// Entry k of the perturbation table, Sim3(+-1e-9 e_d) with k = 1 + 2 d for +,
// 2 + 2 d for -: the value sim3_exp gives there (every one in the theta < eps,
// |sigma| < eps branch), written as the constant it is.  With a fixed scale
// oplusImpl zeroes the seventh component, so both entries of d = 6 are Sim3(0).
__host__ __device__ inline void sim3_perturbation(int k, int fix_scale, Sim3 &P) {
    const int d = (k - 1) >> 1;
    const bool plus = (k & 1) != 0;
    const double h = plus ? 0.5 * kSim3Delta : -(0.5 * kSim3Delta);
    const double g = plus ? kSim3Delta : -kSim3Delta;
    P.q[0] = d == 0 ? h : 0.0;
    P.q[1] = d == 1 ? h : 0.0;
    P.q[2] = d == 2 ? h : 0.0;
    P.q[3] = 1.0;
    P.t[0] = d == 3 ? g : 0.0;
    P.t[1] = d == 4 ? g : 0.0;
    P.t[2] = d == 5 ? g : 0.0;
    P.s = (d == 6 && !fix_scale) ? (plus ? kSim3ExpPlus : kSim3ExpMinus) : 1.0;
}

// Entry k of a linearisation's table: the estimate (k = 0) or Sim3(+-delta e_d) * S, and its inverse
__host__ __device__ inline void sim3_table_entry(const Sim3 &S, int k, int fix_scale, Sim3 &Sk, Sim3 &Sk_inv) {
    if (k == 0) {
        Sk = S;
    } else {
        Sim3 P;
        sim3_perturbation(k, fix_scale, P);
        sim3_mul(P, S, Sk);
    }
    sim3_inverse(Sk, Sk_inv);
}

// computeError of either edge: obs - cam_map(project(S.map(P)))
__host__ __device__ inline void sim3_edge_error(const Sim3 &S, const double *P, const Sim3Cam &c, double u, double v,
                                                double *e) {
    double p[3];
    sim3_map(S, P, p);
    e[0] = u - (p[0] / p[2] * c.fx + c.cx);
    e[1] = v - (p[1] / p[2] * c.fy + c.cy);
}

__host__ __device__ inline double sim3_chi2(const double *e, double omega) {
    double chi2 = 0;
    for (int k = 0; k < 2; ++k) chi2 = chi2 + e[k] * (omega * e[k]);
    return chi2;
}

// One problem as the lanes see it.  A correspondence is active iff
// (flag[i] != 0) == sense: the removal flags with sense = false, or the step
// hook's active array with sense = true (flag == nullptr: all active).
struct Sim3Problem {
    const orbx_sim3_corr *corr;
    int n;
    const uint8_t *flag;
    bool sense;
    double *chi12, *chi21;
    Sim3Cam c1, c2;
    double delta;   // Huber's: (double)(float)sqrt(th2)
    double th2;
    int fix_scale;
    bool robust;
};

__host__ __device__ inline bool sim3_active(const Sim3Problem &pr, int i) {
    return !pr.flag || ((pr.flag[i] != 0) == pr.sense);
}

__host__ __device__ inline Sim3Cam sim3_cam(const orbx_sim3_camera &c) {
    Sim3Cam r;
    r.fx = c.fx; r.fy = c.fy; r.cx = c.cx; r.cy = c.cy;
    return r;
}

__host__ __device__ inline void sim3_problem_thresholds(Sim3Problem &pr, float th2) {
    pr.delta = (double)(float)sqrt((double)th2);   // const float deltaHuber = sqrt(th2)
    pr.th2 = (double)th2;
}

// A linearisation's table where it was formed once (LDS on the device, the stack on the host)
struct Sim3TableRef {
    const Sim3 *S, *Sinv;
    __host__ __device__ inline void get(int k, Sim3 &a, Sim3 &ainv) const {
        a = S[k];
        ainv = Sinv[k];
    }
};

// One edge's terms added to a lane's partials: the numeric Jacobian from the
// table, then buildSystem's blocks.  inv selects the table's inverses (e21).
template <class Table>
__host__ __device__ inline double sim3_edge_terms(const Table &tab, bool inv, const double *P, const Sim3Cam &c,
                                                  double u, double v, double omega, bool robust, double delta,
                                                  double *acc) {
    const double scalar = 1.0 / (2 * kSim3Delta);
    Sim3 a, ainv;
    double e[2], J[2][7];
    tab.get(0, a, ainv);
    sim3_edge_error(inv ? ainv : a, P, c, u, v, e);
    // (kept rolled: unrolled, the loads of all 30 table entries are scheduled ahead of the loop
    // and the kernel spills 1.2 KB a lane to scratch; rolled it needs none)
#pragma nounroll
    for (int d = 0; d < 7; ++d) {
        double ep[2], em[2];
        tab.get(1 + 2 * d, a, ainv);
        sim3_edge_error(inv ? ainv : a, P, c, u, v, ep);
        tab.get(2 + 2 * d, a, ainv);
        sim3_edge_error(inv ? ainv : a, P, c, u, v, em);
        J[0][d] = scalar * (ep[0] - em[0]);
        J[1][d] = scalar * (ep[1] - em[1]);
    }
    const double chi2 = sim3_chi2(e, omega);
    double rho0, rho1;
    lm_huber(chi2, robust, delta, rho0, rho1);
    lm_edge_sums(J, e, omega, rho0, rho1, acc);
    return chi2;
}

// A lane's share of computeActiveErrors + linearizeOplus + buildSystem:
// correspondences lane, lane + 64, ..., e12 before e21
template <class Table>
__host__ __device__ inline void sim3_lane_build(const Sim3Problem &pr, const Table &tab, int lane, double *acc) {
    for (int i = lane; i < pr.n; i += kSim3Lanes) {
        if (!sim3_active(pr, i)) continue;
        const orbx_sim3_corr c = pr.corr[i];
        const double P1[3] = {c.P1c[0], c.P1c[1], c.P1c[2]}, P2[3] = {c.P2c[0], c.P2c[1], c.P2c[2]};
        pr.chi12[i] = sim3_edge_terms(tab, false, P2, pr.c1, (double)c.u1, (double)c.v1, (double)c.inv_sigma2_1,
                                      pr.robust, pr.delta, acc);
        pr.chi21[i] = sim3_edge_terms(tab, true, P1, pr.c2, (double)c.u2, (double)c.v2, (double)c.inv_sigma2_2,
                                      pr.robust, pr.delta, acc);
    }
}

// A lane's share of computeActiveErrors: its robust chi2
__host__ __device__ inline double sim3_lane_errors(const Sim3Problem &pr, const Sim3 &S, const Sim3 &Sinv, int lane) {
    double acc = 0.0;
    for (int i = lane; i < pr.n; i += kSim3Lanes) {
        if (!sim3_active(pr, i)) continue;
        const orbx_sim3_corr c = pr.corr[i];
        const double P1[3] = {c.P1c[0], c.P1c[1], c.P1c[2]}, P2[3] = {c.P2c[0], c.P2c[1], c.P2c[2]};
        double e[2], rho0, rho1;
        sim3_edge_error(S, P2, pr.c1, (double)c.u1, (double)c.v1, e);
        const double c12 = sim3_chi2(e, (double)c.inv_sigma2_1);
        lm_huber(c12, pr.robust, pr.delta, rho0, rho1);
        acc = acc + rho0;
        sim3_edge_error(Sinv, P1, pr.c2, (double)c.u2, (double)c.v2, e);
        const double c21 = sim3_chi2(e, (double)c.inv_sigma2_2);
        lm_huber(c21, pr.robust, pr.delta, rho0, rho1);
        acc = acc + rho0;
        pr.chi12[i] = c12;
        pr.chi21[i] = c21;
    }
    return acc;
}

// Optimizer.cc:1337-1413: two rounds with the classification between them.
// Sout is S0 itself unless both rounds ran.
template <class X>
__host__ __device__ inline void sim3_optimize(X &ex, const Sim3 &S0, int n, Sim3 &Sout, int &n_inliers, int *its) {
    its[0] = 0;
    its[1] = 0;
    n_inliers = 0;
    Sout = S0;
    if (n == 0) return;
    Sim3 S = S0;
    its[0] = lm_run<7>(ex, S, 5);
    const int nBad = ex.classify(1);
    if (n - nBad < 10) return;   // :1379, before g2oS12 is written
    its[1] = lm_run<7>(ex, S, nBad > 0 ? 10 : 5);
    const int nOut = ex.classify(2);
    n_inliers = n - nBad - nOut;
    Sout = S;
}

}  // namespace orbx
