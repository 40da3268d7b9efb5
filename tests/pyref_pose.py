"""Optimizer::PoseOptimization (Optimizer.cc:265-509) restated in float64
numpy: DESIGN.md §3.13 operation for operation, independent of
orbx_pose.hip.  Per-observation arithmetic is elementwise numpy (no fused
operations); a sum over observations goes through a (k, 64) reshape, rows
added in order into 64 partials, then the partials in order; the pose, the
6x6 Cholesky and the LM control are Python floats (IEEE doubles); the
exponential uses math.sin / math.cos / math.pow (glibc's, which the device's
agree with in local BA already).

pose_step is one linear system (orbx_pose_debug_step's counterpart),
pose_optimization the whole run with per-round traces."""
from __future__ import annotations

import math

import numpy as np

DELTA_MONO = float(np.float32(math.sqrt(5.991)))
DELTA_STEREO = float(np.float32(math.sqrt(7.815)))
TH_MONO, TH_STEREO = np.float32(5.991), np.float32(7.815)
DBL_MAX = float(np.finfo(np.float64).max)


# ---- SE3Quat (orbx_se3.h's operation order) ---------------------------------
def quat_rotate(q, v0, v1, v2):
    uv0 = q[1] * v2 - q[2] * v1
    uv1 = q[2] * v0 - q[0] * v2
    uv2 = q[0] * v1 - q[1] * v0
    uv0, uv1, uv2 = uv0 + uv0, uv1 + uv1, uv2 + uv2
    c0 = q[1] * uv2 - q[2] * uv1
    c1 = q[2] * uv0 - q[0] * uv2
    c2 = q[0] * uv1 - q[1] * uv0
    return v0 + q[3] * uv0 + c0, v1 + q[3] * uv1 + c1, v2 + q[3] * uv2 + c2


def quat_to_R(q):
    tx, ty, tz = 2 * q[0], 2 * q[1], 2 * q[2]
    twx, twy, twz = tx * q[3], ty * q[3], tz * q[3]
    txx, txy, txz = tx * q[0], ty * q[0], tz * q[0]
    tyy, tyz, tzz = ty * q[1], tz * q[1], tz * q[2]
    return [1 - (tyy + tzz), txy - twz, txz + twy,
            txy + twz, 1 - (txx + tzz), tyz - twx,
            txz - twy, tyz + twx, 1 - (txx + tyy)]


def R_to_quat(m):
    q = [0.0] * 4
    tr = m[0] + m[4] + m[8]
    if tr > 0:
        t = math.sqrt(tr + 1.0)
        q[3] = 0.5 * t
        t = 0.5 / t
        q[0] = (m[7] - m[5]) * t
        q[1] = (m[2] - m[6]) * t
        q[2] = (m[3] - m[1]) * t
    else:
        i = 0
        if m[4] > m[0]:
            i = 1
        if m[8] > m[3 * i + i]:
            i = 2
        j = (i + 1) % 3
        k = (j + 1) % 3
        t = math.sqrt(m[3 * i + i] - m[3 * j + j] - m[3 * k + k] + 1.0)
        q[i] = 0.5 * t
        t = 0.5 / t
        q[3] = (m[3 * k + j] - m[3 * j + k]) * t
        q[j] = (m[3 * j + i] + m[3 * i + j]) * t
        q[k] = (m[3 * k + i] + m[3 * i + k]) * t
    return q


def quat_normalize(q):
    if q[3] < 0:
        q = [x * -1 for x in q]
    n = math.sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3])
    return [x / n for x in q]


def quat_mul(a, b):
    return [a[3] * b[0] + a[0] * b[3] + a[1] * b[2] - a[2] * b[1],
            a[3] * b[1] + a[1] * b[3] + a[2] * b[0] - a[0] * b[2],
            a[3] * b[2] + a[2] * b[3] + a[0] * b[1] - a[1] * b[0],
            a[3] * b[3] - a[0] * b[0] - a[1] * b[1] - a[2] * b[2]]


def pose_from_cv(Tcw):
    T = np.asarray(Tcw, np.float32).reshape(3, 4)
    R = [float(T[r, c]) for r in range(3) for c in range(3)]
    return quat_normalize(R_to_quat(R)), [float(T[r, 3]) for r in range(3)]


def pose_to_cv(pose):
    q, t = pose
    R = quat_to_R(q)
    with np.errstate(all="ignore"):
        return np.array([[R[3 * r], R[3 * r + 1], R[3 * r + 2], t[r]] for r in range(3)]).astype(np.float32)


def se3_exp_update(pose, u):
    """exp(u) * pose (se3quat.h:223-258, :104-110)"""
    q, t = pose
    w, ups = u[:3], u[3:]
    theta = math.sqrt(w[0] * w[0] + w[1] * w[1] + w[2] * w[2])
    Om = [0.0, -w[2], w[1], w[2], 0.0, -w[0], -w[1], w[0], 0.0]
    O2 = [0.0] * 9
    for r in range(3):
        for c in range(3):
            acc = 0.0
            for k in range(3):
                acc = acc + Om[3 * r + k] * Om[3 * k + c]
            O2[3 * r + c] = acc
    eye = [1.0 if k % 4 == 0 else 0.0 for k in range(9)]
    if theta < 0.00001:
        R = [eye[k] + Om[k] + O2[k] for k in range(9)]
        V = list(R)
    else:
        a = math.sin(theta) / theta
        b = (1 - math.cos(theta)) / (theta * theta)
        c = (theta - math.sin(theta)) / math.pow(theta, 3)
        R = [eye[k] + a * Om[k] + b * O2[k] for k in range(9)]
        V = [eye[k] + b * Om[k] + c * O2[k] for k in range(9)]
    qe = R_to_quat(R)
    te = [V[3 * r] * ups[0] + V[3 * r + 1] * ups[1] + V[3 * r + 2] * ups[2] for r in range(3)]
    qe = quat_normalize(qe)
    rt = quat_rotate(qe, t[0], t[1], t[2])
    tn = [te[k] + rt[k] for k in range(3)]
    qn = quat_normalize(quat_mul(qe, q))
    return qn, tn


# ---- observations -------------------------------------------------------------
class Problem:
    def __init__(self, cam, obs):
        cam = np.asarray(cam).reshape(-1)[0]
        self.fx, self.fy, self.cx, self.cy, self.bf = (float(np.float32(cam[k])) for k in
                                                       ("fx", "fy", "cx", "cy", "bf"))
        X = obs["Xw"].astype(np.float64).reshape(-1, 3)
        self.n = len(obs)
        self.X0, self.X1, self.X2 = X[:, 0].copy(), X[:, 1].copy(), X[:, 2].copy()
        self.u, self.v, self.ur = (obs[k].astype(np.float64) for k in ("u", "v", "ur"))
        self.w = obs["inv_sigma2"].astype(np.float64)
        self.stereo = ~(obs["ur"] < 0)            # monocular iff ur < 0
        self.delta = np.where(self.stereo, DELTA_STEREO, DELTA_MONO)


def lane_sum(terms, active):
    """§3.13's order: partial P_l = the terms of observations l, l + 64, ...
    added in order from +0.0 (inactive: +0.0), total ((P_0 + P_1) + ...) + P_63.
    terms (n,) or (n, m)."""
    t = np.asarray(terms, np.float64)
    flat = t.ndim == 1
    t = t.reshape(len(t), 1) if flat else t
    n, m = t.shape
    k = -(-n // 64)
    a = np.zeros((k * 64, m))
    a[:n] = np.where(np.asarray(active, bool)[:, None], t, 0.0)
    a = a.reshape(k, 64, m)
    P = np.zeros((64, m))
    with np.errstate(all="ignore"):
        for row in a:
            P = P + row
        tot = P[0].copy()
        for l in range(1, 64):
            tot = tot + P[l]
    return float(tot[0]) if flat else tot


def errors(pr, pose):
    """(p (3 arrays), err (3 arrays; the third 0 for mono), chi2) of every
    observation at pose"""
    q, t = pose
    with np.errstate(all="ignore"):
        p0, p1, p2 = quat_rotate(q, pr.X0, pr.X1, pr.X2)
        p0, p1, p2 = p0 + t[0], p1 + t[1], p2 + t[2]
        um, vm = p0 / p2, p1 / p2
        e0m = pr.u - (um * pr.fx + pr.cx)
        e1m = pr.v - (vm * pr.fy + pr.cy)
        invz = (1.0 / p2).astype(np.float32).astype(np.float64)
        r0 = p0 * invz * pr.fx + pr.cx
        r1 = p1 * invz * pr.fy + pr.cy
        e0s, e1s = pr.u - r0, pr.v - r1
        e2s = pr.ur - (r0 - pr.bf * invz)
        e0 = np.where(pr.stereo, e0s, e0m)
        e1 = np.where(pr.stereo, e1s, e1m)
        e2 = np.where(pr.stereo, e2s, 0.0)
        chi2 = (0.0 + e0 * (pr.w * e0)) + e1 * (pr.w * e1)
        chi2 = np.where(pr.stereo, chi2 + e2 * (pr.w * e2), chi2)
    return (p0, p1, p2), (e0, e1, e2), chi2


def huber(pr, chi2, robust):
    """(rho0, rho1) per observation"""
    if not robust:
        return chi2.copy(), np.ones_like(chi2)
    with np.errstate(all="ignore"):
        dsqr = pr.delta * pr.delta
        out = ~(chi2 <= dsqr)
        s = np.sqrt(chi2)
        rho0 = np.where(out, 2 * s * pr.delta - dsqr, chi2)
        rho1 = np.where(out, pr.delta / s, 1.0)
    return rho0, rho1


def jacobians(pr, p):
    """The OnlyPose edges' Jacobians (types_six_dof_expmap.cpp:266-288,
    335-364): J[k][a] arrays, k = 0..2 (row 2 meaningful for stereo only)"""
    x, y, z = p
    fx, fy, bf = pr.fx, pr.fy, pr.bf
    with np.errstate(all="ignore"):
        invz = 1.0 / z
        invz_2 = invz * invz
        zero = np.zeros_like(x)
        J0 = [x * y * invz_2 * fx, -(1 + (x * x * invz_2)) * fx, y * invz * fx, -invz * fx, zero, x * invz_2 * fx]
        J1 = [(1 + y * y * invz_2) * fy, -x * y * invz_2 * fy, -x * invz * fy, zero, -invz * fy, y * invz_2 * fy]
        J2 = [J0[0] - bf * y * invz_2, J0[1] + bf * x * invz_2, J0[2], J0[3], zero, J0[5] - bf * invz_2]
    return [J0, J1, J2]


def build(pr, pose, active, robust, mutate=None):
    """computeActiveErrors + buildSystem: (H (6, 6), b (6,), robust chi2 sum,
    chi2 per observation).  mutate (tests only): {"jsign": (a, s)} multiplies
    Jacobian column a by s."""
    p, err, chi2 = errors(pr, pose)
    rho0, rho1 = huber(pr, chi2, robust)
    J = jacobians(pr, p)
    if mutate and "jsign" in mutate:
        a, s = mutate["jsign"]
        for k in range(3):
            J[k][a] = J[k][a] * s
    st = pr.stereo
    with np.errstate(all="ignore"):
        w = rho1 * pr.w
        omr = [-(pr.w * err[k]) * rho1 for k in range(3)]
        cols = []
        for a in range(6):
            for b in range(a, 6):
                t = (0.0 + (J[0][a] * w) * J[0][b]) + (J[1][a] * w) * J[1][b]
                cols.append(np.where(st, t + (J[2][a] * w) * J[2][b], t))
        for a in range(6):
            t = (0.0 + J[0][a] * omr[0]) + J[1][a] * omr[1]
            cols.append(np.where(st, t + J[2][a] * omr[2], t))
        cols.append(rho0)
    tot = lane_sum(np.stack(cols, 1) if pr.n else np.zeros((0, 28)), active)
    H = np.zeros((6, 6))
    idx = 0
    for a in range(6):
        for b in range(a, 6):
            H[a, b] = H[b, a] = tot[idx]
            idx += 1
    return H, tot[21:27].copy(), float(tot[27]), chi2


def solve(H, b, lam):
    """(H + lam I) x = b by Cholesky (k_ba_chol's conventions); None if not
    positive definite"""
    L = [[0.0] * 6 for _ in range(6)]
    for j in range(6):
        d = float(H[j, j]) + lam
        for k in range(j):
            d = d - L[j][k] * L[j][k]
        if not d > 0:
            return None
        diag = math.sqrt(d)
        L[j][j] = diag
        for i in range(j + 1, 6):
            s = float(H[i, j])
            for k in range(j):
                s = s - L[i][k] * L[j][k]
            L[i][j] = s / diag
    x = [0.0] * 6
    for i in range(6):
        s = float(b[i])
        for k in range(i):
            s = s - L[i][k] * x[k]
        x[i] = s / L[i][i]
    for i in range(5, -1, -1):
        s = x[i]
        for k in range(5, i, -1):
            s = s - L[k][i] * x[k]
        x[i] = s / L[i][i]
    return x


def pose_step(Tcw, cam, obs, active=None, robust=True, lam=0.0, mutate=None):
    """(H, b, x, robust chi2, solved): orbx_pose_debug_step's counterpart"""
    pr = Problem(cam, obs)
    act = np.ones(pr.n, bool) if active is None else np.asarray(active).astype(bool)
    H, b, chi, _ = build(pr, pose_from_cv(Tcw), act, robust, mutate)
    x = solve(H, b, lam)
    return H, b, np.array(x if x is not None else [0.0] * 6), chi, x is not None


def _div(a, b):
    with np.errstate(all="ignore"):
        return float(np.float64(a) / np.float64(b))


def lm(pr, pose, active, robust, chi2_state, trace):
    """optimize(10): lm_optimize for one free vertex.  chi2_state: each
    observation's last computed chi2, updated in place.  Returns (pose,
    iterations)."""
    lam, ni, cur, nbad = 0.0, 2.0, 0.0, 0
    for it in range(10):
        H, b, cur, chi2 = build(pr, pose, active, robust)
        chi2_state[active] = chi2[active]
        if it == 0:
            mx = 0.0
            for j in range(6):
                a = abs(float(H[j, j]))
                mx = mx if a < mx else a
            lam = 1e-5 * mx
            ni, nbad = 2.0, 0
        ini = cur
        rho, q = 0.0, 0
        trials = []
        while True:
            x = solve(H, b, lam)
            bk = pose
            tmp, sc = DBL_MAX, 0.0
            if x is not None:
                pose = se3_exp_update(pose, x)
                _, _, chi2 = errors(pr, pose)
                chi2_state[active] = chi2[active]
                tmp = lane_sum(huber(pr, chi2, robust)[0], active)
                with np.errstate(all="ignore"):
                    for j in range(6):
                        sc += float(np.float64(x[j]) * (np.float64(lam) * x[j] + b[j]))
            with np.errstate(all="ignore"):
                rho = float(np.float64(cur) - np.float64(tmp))
            sc += 1e-3
            rho = _div(rho, sc)
            accepted = rho > 0 and math.isfinite(tmp)
            trials.append({"solved": x is not None, "accepted": accepted, "rho": rho, "lambda": lam})
            if accepted:
                t = 2 * rho - 1
                alpha = 1.0 - t * t * t
                alpha = (2.0 / 3.0) if (2.0 / 3.0) < alpha else alpha
                lam *= alpha if (1.0 / 3.0) < alpha else (1.0 / 3.0)
                ni = 2.0
                cur = tmp
            else:
                lam *= ni
                ni *= 2
                if x is not None:
                    pose = bk
            q += 1
            if not (rho < 0 and q < 10):
                break
        trace.append({"trials": trials, "chi": cur})
        if q == 10 or rho == 0:
            trace[-1]["end"] = "terminate"
            return pose, it + 1
        nbad = nbad + 1 if (ini - cur) * 1e3 < ini else 0
        if nbad >= 3:
            trace[-1]["end"] = "non-improving"
            return pose, it + 1
    return pose, 10


def pose_optimization(Tcw, cam, obs):
    """Returns dict: Tcw (3, 4) f32, outlier (n,) bool, chi2 (n,) f64,
    n_inliers, iterations (4,) int32, rounds: per run round {"active": count,
    "iterations": trace per LM iteration, "outlier": flags after it,
    "depth": camera z of every observation at the round's estimate}."""
    T = np.asarray(Tcw, np.float32).reshape(3, 4)
    pr = Problem(cam, obs)
    n = pr.n
    res = {"Tcw": T.copy(), "outlier": np.zeros(n, bool), "chi2": np.zeros(n), "n_inliers": 0,
           "iterations": np.zeros(4, np.int32), "rounds": []}
    if n < 3:
        return res
    pose0 = pose_from_cv(T)
    out = np.zeros(n, bool)
    chi2_state = np.zeros(n)
    pose = pose0
    for r in range(4):
        pose = pose0
        active = ~out
        trace = []
        if active.any():
            pose, res["iterations"][r] = lm(pr, pose, active, r < 3, chi2_state, trace)
        p, _, chi2 = errors(pr, pose)
        chi2_state[out] = chi2[out]               # a flagged observation: computeError() at the estimate
        with np.errstate(all="ignore"):
            c32 = chi2_state.astype(np.float32)
        out = np.where(pr.stereo, c32 > TH_STEREO, c32 > TH_MONO)
        res["rounds"].append({"active": int(active.sum()), "iterations": trace, "outlier": out.copy(),
                              "depth": p[2].copy()})
        if n < 10:
            break
    res["Tcw"] = pose_to_cv(pose)
    res["outlier"] = out
    res["chi2"] = chi2_state
    res["n_inliers"] = int(n - out.sum())
    return res
