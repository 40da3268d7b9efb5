// orbx_se3.h -- g2o's SE3Quat as the optimisers hold it (se3quat.h), shared by
// orbx_ba.hip (local bundle adjustment), orbx_pose.hip (pose optimisation) and
// orbx_sim3.h (the quaternion products of g2o's Sim3):
// Eigen's quaternion conversions and products in its operation order, the
// exponential update exp(dx) * T, and Converter::toSE3Quat / toCvMat.  All of
// them compile this one text, so a pose takes the same roundings in each.  The
// optimisers' Levenberg-Marquardt control and solve are orbx_lm.h's, not here.
#pragma once

#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

namespace orbx {

struct Pose {      // SE3Quat: q = (x, y, z, w), t
    double q[4];
    double t[3];
    int32_t free_idx;   // -1: fixed
    int32_t pad;
};

// Eigen's q * v (Quaternion::_transformVector): uv = 2 (q.vec x v); v + w uv + q.vec x uv
__host__ __device__ inline void quat_rotate(const double *q, const double *v, double *o) {
    double uv[3] = {q[1] * v[2] - q[2] * v[1], q[2] * v[0] - q[0] * v[2], q[0] * v[1] - q[1] * v[0]};
    for (int i = 0; i < 3; ++i) uv[i] = uv[i] + uv[i];
    const double c[3] = {q[1] * uv[2] - q[2] * uv[1], q[2] * uv[0] - q[0] * uv[2], q[0] * uv[1] - q[1] * uv[0]};
    for (int i = 0; i < 3; ++i) o[i] = v[i] + q[3] * uv[i] + c[i];
}

__host__ __device__ inline void se3_map(const Pose &T, const double *X, double *o) {
    quat_rotate(T.q, X, o);
    for (int i = 0; i < 3; ++i) o[i] = o[i] + T.t[i];
}

// Eigen's Quaternion::toRotationMatrix
__host__ __device__ inline void quat_to_R(const double *q, double *R) {
    const double tx = 2 * q[0], ty = 2 * q[1], tz = 2 * q[2];
    const double twx = tx * q[3], twy = ty * q[3], twz = tz * q[3];
    const double txx = tx * q[0], txy = ty * q[0], txz = tz * q[0];
    const double tyy = ty * q[1], tyz = tz * q[1], tzz = tz * q[2];
    R[0] = 1 - (tyy + tzz); R[1] = txy - twz; R[2] = txz + twy;
    R[3] = txy + twz; R[4] = 1 - (txx + tzz); R[5] = tyz - twx;
    R[6] = txz - twy; R[7] = tyz + twx; R[8] = 1 - (txx + tyy);
}

// Eigen's Quaternion(const Matrix3&) (quaternion_base_assign_impl)
__host__ __device__ inline void R_to_quat(const double *m, double *q) {
    const double tr = m[0] + m[4] + m[8];
    if (tr > 0) {
        double t = sqrt(tr + 1.0);
        q[3] = 0.5 * t;
        t = 0.5 / t;
        q[0] = (m[7] - m[5]) * t;
        q[1] = (m[2] - m[6]) * t;
        q[2] = (m[3] - m[1]) * t;
    } else {
        int i = 0;
        if (m[4] > m[0]) i = 1;
        if (m[8] > m[3 * i + i]) i = 2;
        const int j = (i + 1) % 3, k = (j + 1) % 3;
        double t = sqrt(m[3 * i + i] - m[3 * j + j] - m[3 * k + k] + 1.0);
        q[i] = 0.5 * t;
        t = 0.5 / t;
        q[3] = (m[3 * k + j] - m[3 * j + k]) * t;
        q[j] = (m[3 * j + i] + m[3 * i + j]) * t;
        q[k] = (m[3 * k + i] + m[3 * i + k]) * t;
    }
}

// SE3Quat::normalizeRotation: w >= 0, unit norm
__host__ __device__ inline void quat_normalize(double *q) {
    if (q[3] < 0)
        for (int i = 0; i < 4; ++i) q[i] *= -1;
    const double n = sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
    for (int i = 0; i < 4; ++i) q[i] = q[i] / n;
}

// Eigen's quaternion product a * b
__host__ __device__ inline void quat_mul(const double *a, const double *b, double *o) {
    o[3] = a[3] * b[3] - a[0] * b[0] - a[1] * b[1] - a[2] * b[2];
    o[0] = a[3] * b[0] + a[0] * b[3] + a[1] * b[2] - a[2] * b[1];
    o[1] = a[3] * b[1] + a[1] * b[3] + a[2] * b[0] - a[0] * b[2];
    o[2] = a[3] * b[2] + a[2] * b[3] + a[0] * b[1] - a[1] * b[0];
}

// T = SE3Quat::exp(u) * T (se3quat.h:223-258, :104-110); u = (w, upsilon)
__host__ __device__ inline void se3_exp_update(Pose &T, const double *u) {
    const double w[3] = {u[0], u[1], u[2]}, ups[3] = {u[3], u[4], u[5]};
    const double theta = sqrt(w[0] * w[0] + w[1] * w[1] + w[2] * w[2]);
    const double Om[9] = {0, -w[2], w[1], w[2], 0, -w[0], -w[1], w[0], 0};
    double O2[9];
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c) {
            double acc = 0;
            for (int k = 0; k < 3; ++k) acc = acc + Om[3 * r + k] * Om[3 * k + c];
            O2[3 * r + c] = acc;
        }
    double R[9], V[9];
    if (theta < 0.00001) {
        for (int k = 0; k < 9; ++k) R[k] = ((k % 4 == 0) ? 1.0 : 0.0) + Om[k] + O2[k];
        for (int k = 0; k < 9; ++k) V[k] = R[k];
    } else {
        const double a = sin(theta) / theta, b = (1 - cos(theta)) / (theta * theta);
        const double c = (theta - sin(theta)) / pow(theta, 3);
        for (int k = 0; k < 9; ++k) {
            R[k] = ((k % 4 == 0) ? 1.0 : 0.0) + a * Om[k] + b * O2[k];
            V[k] = ((k % 4 == 0) ? 1.0 : 0.0) + b * Om[k] + c * O2[k];
        }
    }
    double qe[4], te[3];
    R_to_quat(R, qe);
    for (int r = 0; r < 3; ++r) te[r] = V[3 * r] * ups[0] + V[3 * r + 1] * ups[1] + V[3 * r + 2] * ups[2];
    quat_normalize(qe);   // SE3Quat(q, t) constructor
    // (qe, te) * (T.q, T.t): t = te + qe * T.t, q = qe * T.q, normalised
    double rt[3], qn[4];
    quat_rotate(qe, T.t, rt);
    for (int k = 0; k < 3; ++k) T.t[k] = te[k] + rt[k];
    quat_mul(qe, T.q, qn);
    quat_normalize(qn);
    for (int k = 0; k < 4; ++k) T.q[k] = qn[k];
}

// Converter::toSE3Quat (Converter.cc:37-47): SE3Quat(R, t) from a float Tcw
__host__ __device__ inline void pose_from_cv(const float *T, Pose &p) {
    double R[9];
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c) R[3 * r + c] = T[4 * r + c];
    R_to_quat(R, p.q);
    quat_normalize(p.q);
    for (int r = 0; r < 3; ++r) p.t[r] = T[4 * r + 3];
}

// Converter::toCvMat(SE3Quat): rotation matrix and translation as float
__host__ __device__ inline void pose_to_cv(const Pose &p, float *T) {
    double R[9];
    quat_to_R(p.q, R);
    for (int r = 0; r < 3; ++r) {
        for (int c = 0; c < 3; ++c) T[4 * r + c] = (float)R[3 * r + c];
        T[4 * r + 3] = (float)p.t[r];
    }
}

}  // namespace orbx
