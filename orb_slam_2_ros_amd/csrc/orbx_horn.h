// orbx_horn.h -- one Sim3Solver hypothesis (Sim3Solver.cc:215-364) as DESIGN.md
// §3.15 specifies it, in one text for the device (orbx_sim3_ransac.hip) and for
// a host compile (tools/sim3solver_host/sim3solver_host.cpp, the CPU figure and
// a CPU parity check): ComputeSim3, Horn's closed form on three point pairs
// with OpenCV's primitives (reduce, the small Mat products, the Jacobi of
// cv::eigen, norm, Rodrigues) each replaced by the one rule §3.15 states for
// it, and CheckInliers' test of one correspondence.  Float and unfused
// (-ffp-contract=off) except where §3.15 says double.
//
// The Jacobi's pivot indices depend on the data, so its matrices live in
// memory the caller provides (LDS on the device, element e of a lane at
// [e * stride]; a plain array with stride 1 on the host), never in registers.
#pragma once

#include <cfloat>
#include <cmath>
#include <cstdint>

#include "../../include/orbx.h"

namespace orbx {

constexpr int kHornLanes = 64;
constexpr int kJacobiMaxRotations = 4 * 4 * 30;   // cv::eigen's cap, n * n * 30
constexpr int kJacobiFloats = 36;                 // A 16, V 16, W 4

struct HornResult {
    float R[9], t[3], s;
    float T12[12], T21[12];   // [sR | t], [(1/s) R^T | -sRinv t], rows of four
};

// (a0 b0 + a1 b1) + a2 b2: every entry of a small Mat product
__host__ __device__ inline float horn_dot3(float a0, float a1, float a2, float b0, float b1, float b2) {
    return (a0 * b0 + a1 * b1) + a2 * b2;
}

// cv::eigen of a symmetric 4x4 float matrix.  m: kJacobiFloats elements at
// m[e * stride]: A (row-major, both triangles kept), then V, then W.  On
// return W holds the eigenvalues descending and V the eigenvectors as rows.
__host__ __device__ inline void horn_jacobi4(float *m, int stride) {
#define ORBX_A(r, c) m[((r) * 4 + (c)) * stride]
#define ORBX_V(r, c) m[(16 + (r) * 4 + (c)) * stride]
#define ORBX_W(r) m[(32 + (r)) * stride]
    for (int r = 0; r < 4; ++r)
        for (int c = 0; c < 4; ++c) ORBX_V(r, c) = r == c ? 1.0f : 0.0f;
    for (int it = 0; it < kJacobiMaxRotations; ++it) {
        // the largest off-diagonal element, the first in row-major order among equals
        int k = 0, l = 1;
        float mv = fabsf(ORBX_A(0, 1));
        for (int r = 0; r < 3; ++r)
            for (int c = r + 1; c < 4; ++c) {
                const float v = fabsf(ORBX_A(r, c));
                if (mv < v) {
                    mv = v;
                    k = r;
                    l = c;
                }
            }
        const float p = ORBX_A(k, l);
        if (fabsf(p) <= FLT_EPSILON) break;
        const float y = (ORBX_A(l, l) - ORBX_A(k, k)) * 0.5f;
        float t = fabsf(y) + sqrtf(p * p + y * y);
        float s = sqrtf(p * p + t * t);
        const float c = t / s;
        s = p / s;
        t = (p / t) * p;
        if (y < 0.0f) {
            s = -s;
            t = -t;
        }
        for (int i = 0; i < 4; ++i) {
            if (i == k || i == l) continue;
            const float a = ORBX_A(i, k), b = ORBX_A(i, l);
            const float nk = a * c - b * s, nl = a * s + b * c;
            ORBX_A(i, k) = nk;
            ORBX_A(k, i) = nk;
            ORBX_A(i, l) = nl;
            ORBX_A(l, i) = nl;
        }
        ORBX_A(k, k) = ORBX_A(k, k) - t;
        ORBX_A(l, l) = ORBX_A(l, l) + t;
        ORBX_A(k, l) = 0.0f;
        ORBX_A(l, k) = 0.0f;
        for (int i = 0; i < 4; ++i) {
            const float a = ORBX_V(k, i), b = ORBX_V(l, i);
            ORBX_V(k, i) = a * c - b * s;
            ORBX_V(l, i) = a * s + b * c;
        }
    }
    for (int r = 0; r < 4; ++r) ORBX_W(r) = ORBX_A(r, r);
    for (int r = 0; r < 3; ++r) {   // selection sort, descending
        int mx = r;
        for (int i = r + 1; i < 4; ++i)
            if (ORBX_W(mx) < ORBX_W(i)) mx = i;
        if (mx != r) {
            const float w = ORBX_W(mx);
            ORBX_W(mx) = ORBX_W(r);
            ORBX_W(r) = w;
            for (int i = 0; i < 4; ++i) {
                const float v = ORBX_V(mx, i);
                ORBX_V(mx, i) = ORBX_V(r, i);
                ORBX_V(r, i) = v;
            }
        }
    }
#undef ORBX_A
#undef ORBX_V
#undef ORBX_W
}

// ComputeCentroid: C = (reduce sum over the three columns) * (float)(1. / 3),
// Pr = P - C.  P, Pr: [row][point]
__host__ __device__ inline void horn_centroid(const float P[3][3], float Pr[3][3], float C[3]) {
    const float third = (float)(1.0 / 3.0);
    for (int r = 0; r < 3; ++r) {
        C[r] = ((P[r][0] + P[r][1]) + P[r][2]) * third;
        for (int i = 0; i < 3; ++i) Pr[r][i] = P[r][i] - C[r];
    }
}

// cv::Rodrigues on a float vector: double inside, R rounded to float
__host__ __device__ inline void horn_rodrigues(const float v[3], float R[9]) {
    const double rx = v[0], ry = v[1], rz = v[2];
    const double theta = sqrt((rx * rx + ry * ry) + rz * rz);
    if (theta < DBL_EPSILON) {
        for (int k = 0; k < 9; ++k) R[k] = (k & 3) == 0 ? 1.0f : 0.0f;
        return;
    }
    const double c = cos(theta), s = sin(theta), c1 = 1.0 - c, itheta = 1.0 / theta;
    const double x = rx * itheta, y = ry * itheta, z = rz * itheta;
    const double rrt[9] = {x * x, x * y, x * z, x * y, y * y, y * z, x * z, y * z, z * z};
    const double rx_[9] = {0.0, -z, y, z, 0.0, -x, -y, x, 0.0};
    for (int k = 0; k < 9; ++k) {
        const double eye = (k & 3) == 0 ? 1.0 : 0.0;
        R[k] = (float)((c * eye + c1 * rrt[k]) + s * rx_[k]);
    }
}

// ComputeSim3(P1, P2) (:226-337).  P1, P2: [row][point], the three sampled
// points of either camera.  jac: the Jacobi's memory (see above).
__host__ __device__ inline void horn_compute(const float P1[3][3], const float P2[3][3], int fix_scale, float *jac,
                                             int stride, HornResult &out) {
    float Pr1[3][3], Pr2[3][3], O1[3], O2[3];
    horn_centroid(P1, Pr1, O1);
    horn_centroid(P2, Pr2, O2);
    float M[3][3];   // Pr2 * Pr1^T
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j)
            M[i][j] = horn_dot3(Pr2[i][0], Pr2[i][1], Pr2[i][2], Pr1[j][0], Pr1[j][1], Pr1[j][2]);
    // N's ten entries in double from the float M, rounded to float
    const double m00 = M[0][0], m01 = M[0][1], m02 = M[0][2], m10 = M[1][0], m11 = M[1][1], m12 = M[1][2],
                 m20 = M[2][0], m21 = M[2][1], m22 = M[2][2];
    const float N11 = (float)((m00 + m11) + m22), N12 = (float)(m12 - m21), N13 = (float)(m20 - m02),
                N14 = (float)(m01 - m10), N22 = (float)((m00 - m11) - m22), N23 = (float)(m01 + m10),
                N24 = (float)(m20 + m02), N33 = (float)((-m00 + m11) - m22), N34 = (float)(m12 + m21),
                N44 = (float)((-m00 - m11) + m22);
    const float Nm[16] = {N11, N12, N13, N14, N12, N22, N23, N24, N13, N23, N33, N34, N14, N24, N34, N44};
    for (int e = 0; e < 16; ++e) jac[e * stride] = Nm[e];
    horn_jacobi4(jac, stride);
    const float q0 = jac[16 * stride];
    float vec[3] = {jac[17 * stride], jac[18 * stride], jac[19 * stride]};
    // norm(vec): double products summed in order, double square root
    const double v0 = vec[0], v1 = vec[1], v2 = vec[2];
    const double nrm = sqrt(((0.0 + v0 * v0) + v1 * v1) + v2 * v2);
    const double ang = atan2(nrm, (double)q0);
    // 2 * ang * vec / norm(vec): the Mat scaled by (float)((2 ang) (1 / norm))
    const float alpha = (float)((2.0 * ang) * (1.0 / nrm));
    for (int k = 0; k < 3; ++k) vec[k] = vec[k] * alpha;
    horn_rodrigues(vec, out.R);
    const float *R = out.R;
    float P3[3][3];   // R * Pr2
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j)
            P3[i][j] = horn_dot3(R[3 * i], R[3 * i + 1], R[3 * i + 2], Pr2[0][j], Pr2[1][j], Pr2[2][j]);
    if (!fix_scale) {
        double nom = 0.0, den = 0.0;   // Pr1.dot(P3); the double loop over float squares
        for (int i = 0; i < 3; ++i)
            for (int j = 0; j < 3; ++j) {
                nom += (double)Pr1[i][j] * (double)P3[i][j];
                const float sq = P3[i][j] * P3[i][j];
                den += (double)sq;
            }
        out.s = (float)(nom / den);
    } else {
        out.s = 1.0f;
    }
    const float s = out.s;
    // t = O1 - s * (R * O2)
    for (int i = 0; i < 3; ++i)
        out.t[i] = O1[i] - s * horn_dot3(R[3 * i], R[3 * i + 1], R[3 * i + 2], O2[0], O2[1], O2[2]);
    // T12 = [sR | t]; T21 = [sRinv | -(sRinv * t)], sRinv = (float)(1.0 / s) * R^T
    const float sinv = (float)(1.0 / (double)s);
    float sRinv[9];
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) {
            out.T12[4 * i + j] = s * R[3 * i + j];
            sRinv[3 * i + j] = sinv * R[3 * j + i];
        }
    for (int i = 0; i < 3; ++i) {
        out.T12[4 * i + 3] = out.t[i];
        for (int j = 0; j < 3; ++j) out.T21[4 * i + j] = sRinv[3 * i + j];
        out.T21[4 * i + 3] =
            -horn_dot3(sRinv[3 * i], sRinv[3 * i + 1], sRinv[3 * i + 2], out.t[0], out.t[1], out.t[2]);
    }
}

// FromCameraToImage of one point (:405-423)
__host__ __device__ inline void horn_own_projection(const float X[3], const orbx_sim3_camera &cam, float &u,
                                                    float &v) {
    const float invz = 1.0f / X[2];
    const float x = X[0] * invz, y = X[1] * invz;
    u = cam.fx * x + cam.cx;
    v = cam.fy * y + cam.cy;
}

// Project of one point (:382-403): T rows of four, [R | t]
template <typename TPtr>
__host__ __device__ inline void horn_project(const TPtr T, const float X[3], const orbx_sim3_camera &cam, float &u,
                                             float &v) {
    float c[3];
    for (int i = 0; i < 3; ++i) c[i] = horn_dot3(T[4 * i], T[4 * i + 1], T[4 * i + 2], X[0], X[1], X[2]) + T[4 * i + 3];
    const float invz = 1.0f / c[2];
    const float x = c[0] * invz, y = c[1] * invz;
    u = cam.fx * x + cam.cx;
    v = cam.fy * y + cam.cy;
}

// dist.dot(dist) of a 2-vector assigned to a float: double products summed
// from 0.0, rounded to float
__host__ __device__ inline float horn_err(float dx, float dy) {
    return (float)((0.0 + (double)dx * (double)dx) + (double)dy * (double)dy);
}

// CheckInliers of one correspondence (:348-363).  u1o, v1o, u2o, v2o: its own
// projections (mvP1im1, mvP2im2)
template <typename TPtr>
__host__ __device__ inline bool horn_inlier(const TPtr T12, const TPtr T21, const orbx_ransac_corr &k,
                                            const orbx_sim3_camera &cam1, const orbx_sim3_camera &cam2, float u1o,
                                            float v1o, float u2o, float v2o, float *err_out = nullptr) {
    float u21, v21, u12, v12;
    horn_project(T12, k.X2c, cam1, u21, v21);   // vP2im1
    horn_project(T21, k.X1c, cam2, u12, v12);   // vP1im2
    const float err1 = horn_err(u1o - u21, v1o - v21);
    const float err2 = horn_err(u12 - u2o, v12 - v2o);
    if (err_out) {
        err_out[0] = err1;
        err_out[1] = err2;
    }
    return err1 < k.max_err1 && err2 < k.max_err2;
}

// A triple is usable iff its indices are distinct and inside [0, n)
__host__ __device__ inline bool horn_triple_ok(const int32_t *t, int n) {
    return t[0] >= 0 && t[1] >= 0 && t[2] >= 0 && t[0] < n && t[1] < n && t[2] < n && t[0] != t[1] && t[0] != t[2] &&
           t[1] != t[2];
}

}  // namespace orbx
