// orbx_triangulate.h -- one pair of LocalMapping::CreateNewMapPoints' inner loop
// (LocalMapping.cc:334-480) as DESIGN.md §3.16 specifies it, in one text for the
// device (orbx_triangulate.hip) and for a host compile
// (tools/triangulate_host/triangulate_host.cpp, the CPU figure and a CPU parity
// check): the ray parallax test, the linear triangulation (cv::SVD::compute of
// the float 4x4 restated as a one-sided Jacobi, of which only vt.row(3) is
// used) or KeyFrame::UnprojectStereo, the two depth tests, the two reprojection
// tests and the scale-consistency test.  Float and unfused (-ffp-contract=off)
// except where §3.16 says double.
//
// The Jacobi's pair order and the sort are fixed, so every array index below is
// a compile-time constant once the loops are unrolled: A^T, V and the four
// double norms stay in registers on the device.
#pragma once

#include <cfloat>
#include <cmath>
#include <cstdint>

#include "../../include/orbx.h"

namespace orbx {

constexpr int kTriMaxSweeps = 30;
constexpr int kTriInvalidStereo = 9;

// (a0 b0 + a1 b1) + a2 b2: every entry of a small Mat product (§3.15's rule)
__host__ __device__ inline float tri_dot3(float a0, float a1, float a2, float b0, float b1, float b2) {
    return (a0 * b0 + a1 * b1) + a2 * b2;
}

// Mat::dot of two float 3-vectors: double products summed in order from 0.0
__host__ __device__ inline double tri_dotd(float a0, float a1, float a2, float b0, float b1, float b2) {
    return ((0.0 + (double)a0 * (double)b0) + (double)a1 * (double)b1) + (double)a2 * (double)b2;
}

// cos(2 atan2(mb / 2, depth)) as the identity (d d - h h) / (d d + h h), once in double
__host__ __device__ inline float tri_cos_stereo(float mb, float depth) {
    const float hm = mb / 2.0f;
    const double h = (double)hm, d = (double)depth;
    return (float)((d * d - h * h) / (d * d + h * h));
}

// hypot as cv::SVD's Jacobi forms it: no library call
__host__ __device__ inline double tri_hypot(double a, double b) {
    a = fabs(a);
    b = fabs(b);
    if (a > b) {
        b /= a;
        return a * sqrt(1.0 + b * b);
    }
    if (b > 0.0) {
        a /= b;
        return b * sqrt(1.0 + a * a);
    }
    return 0.0;
}

// One pair (i, j) of a sweep: rows Ai, Aj of A^T, rows Vi, Vj of V, their
// squared norms wi, wj.  Returns whether it rotated.
__host__ __device__ inline bool tri_rotate(float *Ai, float *Aj, float *Vi, float *Vj, double &wi, double &wj) {
    const double a = wi, b = wj;
    double p = 0.0;
#pragma unroll
    for (int k = 0; k < 4; ++k) p += (double)Ai[k] * (double)Aj[k];
    if (fabs(p) <= (2.0 * (double)FLT_EPSILON) * sqrt(a * b)) return false;
    p *= 2.0;
    const double beta = a - b, gamma = tri_hypot(p, beta);
    float c, s;
    if (beta < 0.0) {
        const double delta = (gamma - beta) * 0.5;
        s = (float)sqrt(delta / gamma);
        c = (float)(p / ((gamma * (double)s) * 2.0));
    } else {
        c = (float)sqrt((gamma + beta) / (gamma * 2.0));
        s = (float)(p / ((gamma * (double)c) * 2.0));
    }
    double na = 0.0, nb = 0.0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const float t0 = c * Ai[k] + s * Aj[k];
        const float t1 = (-s) * Ai[k] + c * Aj[k];
        Ai[k] = t0;
        Aj[k] = t1;
        na += (double)t0 * (double)t0;
        nb += (double)t1 * (double)t1;
    }
    wi = na;
    wj = nb;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const float t0 = c * Vi[k] + s * Vj[k];
        const float t1 = (-s) * Vi[k] + c * Vj[k];
        Vi[k] = t0;
        Vj[k] = t1;
    }
    return true;
}

// vt.row(3) of cv::SVD::compute(A): A row-major 4x4.  Returns the number of
// sweeps run (the last one changed nothing unless it is kTriMaxSweeps).
__host__ __device__ inline int tri_svd_last_row(const float A[16], float out[4]) {
    float At[4][4], V[4][4];
    double W[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        double w = 0.0;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            At[i][k] = A[4 * k + i];
            V[i][k] = i == k ? 1.0f : 0.0f;
            w += (double)At[i][k] * (double)At[i][k];
        }
        W[i] = w;
    }
    int sweeps = 0;
    for (; sweeps < kTriMaxSweeps;) {
        ++sweeps;
        bool changed = false;
#pragma unroll
        for (int i = 0; i < 3; ++i)
#pragma unroll
            for (int j = i + 1; j < 4; ++j) changed |= tri_rotate(At[i], At[j], V[i], V[j], W[i], W[j]);
        if (!changed) break;
    }
    double S[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) S[i] = sqrt(W[i]);
    // selection sort, descending, the first among equals (§3.15's rule); the
    // swap partner is a run-time value, so each candidate swaps under a predicate
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        int mx = r;
        double best = S[r];
#pragma unroll
        for (int i = r + 1; i < 4; ++i)
            if (best < S[i]) {
                best = S[i];
                mx = i;
            }
#pragma unroll
        for (int i = r + 1; i < 4; ++i)
            if (mx == i) {
                const double sv = S[i];
                S[i] = S[r];
                S[r] = sv;
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const float v = V[i][k];
                    V[i][k] = V[r][k];
                    V[r][k] = v;
                }
            }
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) out[k] = V[3][k];
    return sweeps;
}

// An observation the reference could not have: a right coordinate without a
// positive depth (UnprojectStereo would return an empty Mat, :390 / :394
// dereference it)
__host__ __device__ inline bool tri_obs_invalid(const orbx_tri_obs &o) { return o.ur >= 0.0f && !(o.depth > 0.0f); }

// KeyFrame::UnprojectStereo (KeyFrame.cc:748-764) of a valid stereo observation
__host__ __device__ inline void tri_unproject(const orbx_tri_view &v, const orbx_tri_obs &o, float X[3]) {
    const float z = o.depth;
    const float x = (o.raw_u - v.cx) * z * v.invfx;
    const float y = (o.raw_v - v.cy) * z * v.invfy;
#pragma unroll
    for (int i = 0; i < 3; ++i) X[i] = tri_dot3(v.Tcw[i], v.Tcw[4 + i], v.Tcw[8 + i], x, y, z) + v.Ow[i];
}

// (float)(Rcw.row(r).dot(x3Dt) + tcw(r))
__host__ __device__ inline float tri_cam(const orbx_tri_view &v, int r, const float X[3]) {
    return (float)(tri_dotd(v.Tcw[4 * r], v.Tcw[4 * r + 1], v.Tcw[4 * r + 2], X[0], X[1], X[2]) +
                   (double)v.Tcw[4 * r + 3]);
}

// The reprojection test of one side (:410-461); mbf: the current keyframe's on
// both sides (:454).  True = rejected.
__host__ __device__ inline bool tri_reproj_fails(const orbx_tri_view &v, const orbx_tri_obs &o, float mbf, float z,
                                                 const float X[3]) {
    const float x = tri_cam(v, 0, X), y = tri_cam(v, 1, X);
    const float invz = (float)(1.0 / (double)z);
    const float u = v.fx * x * invz + v.cx;
    const float vv = v.fy * y * invz + v.cy;
    const float ex = u - o.u, ey = vv - o.v;
    if (!(o.ur >= 0.0f)) return (double)(ex * ex + ey * ey) > 5.991 * (double)o.sigma2;
    const float u_r = u - mbf * invz;
    const float er = u_r - o.ur;
    return (double)(ex * ex + ey * ey + er * er) > 7.8 * (double)o.sigma2;
}

// (float)cv::norm(X - Ow)
__host__ __device__ inline float tri_dist(const float X[3], const float Ow[3]) {
    const float n0 = X[0] - Ow[0], n1 = X[1] - Ow[1], n2 = X[2] - Ow[2];
    return (float)sqrt(tri_dotd(n0, n1, n2, n0, n1, n2));
}

// One pair.  Writes X (zero unless computed) and returns the status of
// orbx_tri_point; sweeps (optional): the Jacobi's sweep count, 0 without one.
__host__ __device__ inline int tri_pair(const orbx_tri_view &v1, const orbx_tri_view &v2, float ratio_factor,
                                        const orbx_tri_obs &o1, const orbx_tri_obs &o2, float X[3],
                                        int *sweeps = nullptr) {
    X[0] = X[1] = X[2] = 0.0f;
    if (sweeps) *sweeps = 0;
    if (tri_obs_invalid(o1) || tri_obs_invalid(o2)) return kTriInvalidStereo;
    const bool st1 = o1.ur >= 0.0f, st2 = o2.ur >= 0.0f;
    const float xn1[3] = {(o1.u - v1.cx) * v1.invfx, (o1.v - v1.cy) * v1.invfy, 1.0f};
    const float xn2[3] = {(o2.u - v2.cx) * v2.invfx, (o2.v - v2.cy) * v2.invfy, 1.0f};
    float r1[3], r2[3];   // Rwc * xn, Rwc = Rcw^T
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        r1[i] = tri_dot3(v1.Tcw[i], v1.Tcw[4 + i], v1.Tcw[8 + i], xn1[0], xn1[1], xn1[2]);
        r2[i] = tri_dot3(v2.Tcw[i], v2.Tcw[4 + i], v2.Tcw[8 + i], xn2[0], xn2[1], xn2[2]);
    }
    const double nr1 = sqrt(tri_dotd(r1[0], r1[1], r1[2], r1[0], r1[1], r1[2]));
    const double nr2 = sqrt(tri_dotd(r2[0], r2[1], r2[2], r2[0], r2[1], r2[2]));
    const float cos_rays = (float)(tri_dotd(r1[0], r1[1], r1[2], r2[0], r2[1], r2[2]) / (nr1 * nr2));
    float cs1 = cos_rays + 1.0f, cs2 = cs1;
    if (st1)
        cs1 = tri_cos_stereo(v1.mb, o1.depth);
    else if (st2)
        cs2 = tri_cos_stereo(v2.mb, o2.depth);
    const float cos_stereo = cs2 < cs1 ? cs2 : cs1;   // std::min(cs1, cs2)

    if (cos_rays < cos_stereo && cos_rays > 0.0f && (st1 || st2 || (double)cos_rays < 0.9998)) {
        float A[16];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            A[j] = xn1[0] * v1.Tcw[8 + j] - v1.Tcw[j];
            A[4 + j] = xn1[1] * v1.Tcw[8 + j] - v1.Tcw[4 + j];
            A[8 + j] = xn2[0] * v2.Tcw[8 + j] - v2.Tcw[j];
            A[12 + j] = xn2[1] * v2.Tcw[8 + j] - v2.Tcw[4 + j];
        }
        float h[4];
        const int n = tri_svd_last_row(A, h);
        if (sweeps) *sweeps = n;
        if (h[3] == 0.0f) return 2;
        const float alpha = (float)(1.0 / (double)h[3]);
#pragma unroll
        for (int i = 0; i < 3; ++i) X[i] = h[i] * alpha;
    } else if (st1 && cs1 < cs2) {
        tri_unproject(v1, o1, X);
    } else if (st2 && cs2 < cs1) {
        tri_unproject(v2, o2, X);
    } else {
        return 1;
    }

    const float z1 = tri_cam(v1, 2, X);
    if (z1 <= 0.0f) return 3;
    const float z2 = tri_cam(v2, 2, X);
    if (z2 <= 0.0f) return 4;
    if (tri_reproj_fails(v1, o1, v1.mbf, z1, X)) return 5;
    if (tri_reproj_fails(v2, o2, v1.mbf, z2, X)) return 6;
    const float d1 = tri_dist(X, v1.Ow), d2 = tri_dist(X, v2.Ow);
    if (d1 == 0.0f || d2 == 0.0f) return 7;
    const float ratio_dist = d2 / d1, ratio_octave = o1.scale / o2.scale;
    if (ratio_dist * ratio_factor < ratio_octave || ratio_dist > ratio_octave * ratio_factor) return 8;
    return 0;
}

// The problem of pair i: the last p with offsets[p] <= i (empty problems are
// passed over); offsets[0] = 0 <= i < offsets[nproblems]
__host__ __device__ inline int tri_problem_of(const int32_t *offsets, int nproblems, int i) {
    int lo = 0, hi = nproblems;   // offsets[lo] <= i < offsets[hi]
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (offsets[mid] <= i)
            lo = mid;
        else
            hi = mid;
    }
    return lo;
}

}  // namespace orbx
