"""Optimizer::OptimizeSim3 (Optimizer.cc:1177-1414) restated in float64 numpy:
DESIGN.md §3.14 operation for operation, independent of orbx_sim3.h.  The Sim3
algebra, the 7x7 Cholesky and the LM control are Python floats (IEEE doubles);
per-correspondence arithmetic is elementwise numpy (no fused operations); a sum
over correspondences goes through pyref_pose.lane_sum (rows of 64 added in
order into 64 partials, then the partials in order), each correspondence's e12
terms before its e21 terms.  The update's sin and cos are math.sin / math.cos
(glibc's, which the device's agree with in local BA and pose optimisation
already); its exp is §3.14's own fixed sequence (exp_spec), because the
device's exp and glibc's differ in the last bit on arguments a run reaches.

sim3_step is one linear system (orbx_sim3_debug_step's counterpart),
sim3_update one update, optimize_sim3 the whole run with per-round traces."""
from __future__ import annotations

import math

import numpy as np

from pyref_pose import DBL_MAX, R_to_quat, _div, lane_sum, quat_mul, quat_rotate

DELTA = 1e-9
SCALAR = 1.0 / (2 * DELTA)
EXP_PLUS = float.fromhex("0x1.000000044b830p+0")    # exp(+1e-9), correctly rounded
EXP_MINUS = float.fromhex("0x1.fffffff768fa1p-1")    # exp(-1e-9)
EPS = 0.00001


# ---- g2o::Sim3 (sim3.h): (q (x, y, z, w), t, s), q never normalised ------------
def sim3_from(S):
    S = np.asarray(S).reshape(-1)[0]
    return [float(v) for v in S["q"]], [float(v) for v in S["t"]], float(S["s"])


def sim3_map(S, X0, X1, X2):
    q, t, s = S
    r0, r1, r2 = quat_rotate(q, X0, X1, X2)
    return s * r0 + t[0], s * r1 + t[1], s * r2 + t[2]


def sim3_inverse(S):
    q, t, s = S
    qc = [-q[0], -q[1], -q[2], q[3]]
    a = _div(-1.0, s)
    ti = quat_rotate(qc, a * t[0], a * t[1], a * t[2])
    return qc, [ti[0], ti[1], ti[2]], _div(1.0, s)


def sim3_mul(A, B):
    qa, ta, sa = A
    qb, tb, sb = B
    r = quat_rotate(qa, tb[0], tb[1], tb[2])
    return quat_mul(qa, qb), [sa * r[k] + ta[k] for k in range(3)], sa * sb


FACT = [float(math.factorial(n)) for n in range(14)]
INV_LN2 = float.fromhex("0x1.71547652b82fep+0")
LN2_HI = float.fromhex("0x1.62e42fee00000p-1")
LN2_LO = float.fromhex("0x1.a39ef35793c76p-33")


def exp_spec(x):
    """§3.14's exp: k = floor(x / ln 2 + 1/2), r = (x - k ln2_hi) - k ln2_lo,
    the degree-13 Taylor polynomial by Horner with coefficients 1 / n!, times 2^k"""
    if x != x:
        return x
    if x > 709.0:
        return math.inf
    if x < -745.0:
        return 0.0
    kd = float(math.floor(x * INV_LN2 + 0.5))
    r = (x - kd * LN2_HI) - kd * LN2_LO
    p = 1.0 / FACT[13]
    for n in range(12, -1, -1):
        p = 1.0 / FACT[n] + r * p
    return math.ldexp(p, int(kd))


def sim3_exp(u):
    """Sim3(const Vector7d&) (sim3.h:70-142), all four branches"""
    w, ups, sigma = u[:3], u[3:6], u[6]
    theta = math.sqrt(w[0] * w[0] + w[1] * w[1] + w[2] * w[2])
    Om = [0.0, -w[2], w[1], w[2], 0.0, -w[0], -w[1], w[0], 0.0]
    s = exp_spec(sigma)
    O2 = [0.0] * 9
    for r in range(3):
        for c in range(3):
            acc = 0.0
            for k in range(3):
                acc = acc + Om[3 * r + k] * Om[3 * k + c]
            O2[3 * r + c] = acc
    eye = [1.0 if k % 4 == 0 else 0.0 for k in range(9)]
    small = theta < EPS
    if small:
        R = [eye[k] + Om[k] + O2[k] for k in range(9)]
    else:
        ra = math.sin(theta) / theta
        rb = (1 - math.cos(theta)) / (theta * theta)
        R = [eye[k] + ra * Om[k] + rb * O2[k] for k in range(9)]
    if abs(sigma) < EPS:
        C = 1.0
        if small:
            A, B = 1.0 / 2.0, 1.0 / 6.0
        else:
            theta2 = theta * theta
            A = (1 - math.cos(theta)) / theta2
            B = (theta - math.sin(theta)) / (theta2 * theta)
    else:
        C = (s - 1) / sigma
        if small:
            sigma2 = sigma * sigma
            A = ((sigma - 1) * s + 1) / sigma2
            B = ((0.5 * sigma2 - sigma + 1) * s) / (sigma2 * sigma)
        else:
            a = s * math.sin(theta)
            b = s * math.cos(theta)
            theta2 = theta * theta
            sigma2 = sigma * sigma
            c = theta2 + sigma2
            A = (a * sigma + (1 - b) * theta) / (theta * c)
            B = (C - ((b - 1) * sigma + a * theta) / c) * 1.0 / theta2
    q = R_to_quat(R)
    W = [A * Om[k] + B * O2[k] + C * eye[k] for k in range(9)]
    t = [W[3 * r] * ups[0] + W[3 * r + 1] * ups[1] + W[3 * r + 2] * ups[2] for r in range(3)]
    return q, t, s


def sim3_update(S, x, fix_scale):
    """oplusImpl: Sim3(x) * S, x[6] zeroed first with a fixed scale"""
    u = [float(v) for v in x]
    if fix_scale:
        u[6] = 0.0
    return sim3_mul(sim3_exp(u), S)


def perturbation(k, fix_scale):
    """Entry k of §3.14's table: Sim3(+1e-9 e_d) for k = 1 + 2 d, Sim3(-1e-9
    e_d) for k = 2 + 2 d, as constants"""
    d, plus = (k - 1) >> 1, (k & 1) != 0
    h = 0.5 * DELTA if plus else -(0.5 * DELTA)
    g = DELTA if plus else -DELTA
    q = [h if d == j else 0.0 for j in range(3)] + [1.0]
    t = [g if d == 3 + j else 0.0 for j in range(3)]
    s = (EXP_PLUS if plus else EXP_MINUS) if (d == 6 and not fix_scale) else 1.0
    return q, t, s


def table(S, fix_scale):
    """The estimate and its 14 perturbed estimates, each with its inverse"""
    tab = []
    for k in range(15):
        Sk = S if k == 0 else sim3_mul(perturbation(k, fix_scale), S)
        tab.append((Sk, sim3_inverse(Sk)))
    return tab


# ---- correspondences ------------------------------------------------------------
class Problem:
    def __init__(self, cam1, cam2, corr, th2):
        c1, c2 = np.asarray(cam1).reshape(-1)[0], np.asarray(cam2).reshape(-1)[0]
        self.cam = [tuple(float(np.float32(c[k])) for k in ("fx", "fy", "cx", "cy")) for c in (c1, c2)]
        self.n = len(corr)
        P1 = corr["P1c"].astype(np.float64).reshape(-1, 3)
        P2 = corr["P2c"].astype(np.float64).reshape(-1, 3)
        self.P1 = [P1[:, k].copy() for k in range(3)]
        self.P2 = [P2[:, k].copy() for k in range(3)]
        self.obs = [(corr["u1"].astype(np.float64), corr["v1"].astype(np.float64)),
                    (corr["u2"].astype(np.float64), corr["v2"].astype(np.float64))]
        self.w = [corr["inv_sigma2_1"].astype(np.float64), corr["inv_sigma2_2"].astype(np.float64)]
        th2 = np.float32(th2)
        self.th2 = float(th2)
        self.delta = float(np.float32(math.sqrt(float(th2))))


def edge_error(pr, edge, S):
    """computeError of edge 0 (e12, at S) or 1 (e21, at S's inverse, which the
    caller passes): (e0, e1, depth)"""
    P = pr.P2 if edge == 0 else pr.P1
    fx, fy, cx, cy = pr.cam[edge]
    u, v = pr.obs[edge]
    with np.errstate(all="ignore"):
        p0, p1, p2 = sim3_map(S, P[0], P[1], P[2])
        e0 = u - (p0 / p2 * fx + cx)
        e1 = v - (p1 / p2 * fy + cy)
    return e0, e1, p2


def chi2_of(e0, e1, w):
    with np.errstate(all="ignore"):
        return (0.0 + e0 * (w * e0)) + e1 * (w * e1)


def huber(pr, chi2, robust):
    if not robust:
        return chi2.copy(), np.ones_like(chi2)
    with np.errstate(all="ignore"):
        dsqr = pr.delta * pr.delta
        out = ~(chi2 <= dsqr)
        s = np.sqrt(chi2)
        rho0 = np.where(out, 2 * s * pr.delta - dsqr, chi2)
        rho1 = np.where(out, pr.delta / s, 1.0)
    return rho0, rho1


def numeric_jacobian(pr, edge, tab, mutate=None):
    """J[k][d] arrays: scalar * (e(S+_d) - e(S-_d)).  mutate (tests only):
    {"jsign": d} flips column d; {"one_sided": d} takes e(S) in the place of
    e(S-_d) and leaves the scalar 1 / (2 delta) alone (the negative step
    dropped from g2o's loop); {"forward": d} is the correctly scaled forward
    difference (e(S+_d) - e(S)) / delta."""
    J = [[None] * 7, [None] * 7]
    base = edge_error(pr, edge, tab[0][edge])
    for d in range(7):
        ep = edge_error(pr, edge, tab[1 + 2 * d][edge])
        em = edge_error(pr, edge, tab[2 + 2 * d][edge])
        with np.errstate(all="ignore"):
            for k in range(2):
                J[k][d] = SCALAR * (ep[k] - em[k])
                if mutate and mutate.get("one_sided") == d:
                    J[k][d] = SCALAR * (ep[k] - base[k])
                if mutate and mutate.get("forward") == d:
                    J[k][d] = (ep[k] - base[k]) / DELTA
                if mutate and mutate.get("jsign") == d:
                    J[k][d] = -J[k][d]
    return J


def edge_terms(pr, edge, tab, robust, mutate=None):
    """(36 term arrays, chi2) of one edge type"""
    e0, e1, _ = edge_error(pr, edge, tab[0][edge])
    J = numeric_jacobian(pr, edge, tab, mutate)
    om = pr.w[edge]
    chi2 = chi2_of(e0, e1, om)
    rho0, rho1 = huber(pr, chi2, robust)
    with np.errstate(all="ignore"):
        w = rho1 * om
        omr = [-(om * e0) * rho1, -(om * e1) * rho1]
        cols = []
        for a in range(7):
            for b in range(a, 7):
                cols.append((0.0 + (J[0][a] * w) * J[0][b]) + (J[1][a] * w) * J[1][b])
        for a in range(7):
            cols.append((0.0 + J[0][a] * omr[0]) + J[1][a] * omr[1])
        cols.append(rho0)
    return cols, chi2


def pair_sum(t12, t21, active):
    """§3.14's order: correspondence i on lane i % 64, its e12 term then its
    e21 term added to the lane's partial, partials added in lane order.
    Interleaving the two as rows 2r and 2r + 1 of lane_sum's (k, 64) layout is
    that order."""
    t12, t21 = np.asarray(t12, np.float64), np.asarray(t21, np.float64)
    flat = t12.ndim == 1
    if flat:
        t12, t21 = t12[:, None], t21[:, None]
    n, m = t12.shape
    k = -(-n // 64)
    a = np.zeros((k, 2, 64, m))
    act = np.asarray(active, bool)[:, None]
    pad = np.zeros((k * 64, m))
    pad[:n] = np.where(act, t12, 0.0)
    a[:, 0] = pad.reshape(k, 64, m)
    pad = np.zeros((k * 64, m))
    pad[:n] = np.where(act, t21, 0.0)
    a[:, 1] = pad.reshape(k, 64, m)
    tot = lane_sum(a.reshape(2 * k * 64, m), np.ones(2 * k * 64, bool)) if k else np.zeros(m)
    return float(tot[0]) if flat else tot


def build(pr, S, active, robust, fix_scale, mutate=None):
    """(H (7, 7), b (7,), robust chi2 sum, chi2_12, chi2_21, J12, J21)"""
    tab = table(S, fix_scale)
    c12, chi12 = edge_terms(pr, 0, tab, robust, mutate)
    c21, chi21 = edge_terms(pr, 1, tab, robust, mutate)
    if mutate and "drop_e21" in mutate:
        c21 = [np.where(np.arange(pr.n) == mutate["drop_e21"], 0.0, c) for c in c21]
    if pr.n:
        tot = pair_sum(np.stack(c12, 1), np.stack(c21, 1), active)
    else:
        tot = np.zeros(36)
    H = np.zeros((7, 7))
    idx = 0
    for a in range(7):
        for b in range(a, 7):
            H[a, b] = H[b, a] = tot[idx]
            idx += 1
    return H, tot[28:35].copy(), float(tot[35]), chi12, chi21


def solve(H, b, lam):
    """(H + lam I) x = b by a 7x7 Cholesky (k_ba_chol's conventions); None if
    not positive definite"""
    n = 7
    L = [[0.0] * n for _ in range(n)]
    with np.errstate(all="ignore"):
        for j in range(n):
            d = float(H[j, j]) + lam
            for k in range(j):
                d = d - L[j][k] * L[j][k]
            if not d > 0:
                return None
            diag = math.sqrt(d)
            L[j][j] = diag
            for i in range(j + 1, n):
                s = float(H[i, j])
                for k in range(j):
                    s = s - L[i][k] * L[j][k]
                L[i][j] = _div(s, diag)
        x = [0.0] * n
        for i in range(n):
            s = float(b[i])
            for k in range(i):
                s = s - L[i][k] * x[k]
            x[i] = _div(s, L[i][i])
        for i in range(n - 1, -1, -1):
            s = x[i]
            for k in range(n - 1, i, -1):
                s = s - L[k][i] * x[k]
            x[i] = _div(s, L[i][i])
    return x


def sim3_step(S, cams, corr, active=None, robust=True, lam=0.0, fix_scale=False, th2=10.0, mutate=None):
    """(H, b, x, robust chi2, solved): orbx_sim3_debug_step's counterpart.
    S: an orbx_sim3 record or a (q, t, s) triple; cams: (cam1, cam2)."""
    pr = Problem(cams[0], cams[1], corr, th2)
    S = S if isinstance(S, tuple) else sim3_from(S)
    act = np.ones(pr.n, bool) if active is None else np.asarray(active).astype(bool)
    H, b, chi, _, _ = build(pr, S, act, robust, fix_scale, mutate)
    x = solve(H, b, lam)
    return H, b, np.array(x if x is not None else [0.0] * 7), chi, x is not None


def errors(pr, S, active, robust, state):
    """computeActiveErrors at S: the robust chi2 sum; the active edges' chi2 into state"""
    e0, e1, _ = edge_error(pr, 0, S)
    c12 = chi2_of(e0, e1, pr.w[0])
    e0, e1, _ = edge_error(pr, 1, sim3_inverse(S))
    c21 = chi2_of(e0, e1, pr.w[1])
    state[0][active] = c12[active]
    state[1][active] = c21[active]
    return pair_sum(huber(pr, c12, robust)[0], huber(pr, c21, robust)[0], active)


def lm(pr, S, active, fix_scale, maxit, state, trace):
    """optimize(maxit): pyref_pose.lm with seven dimensions.  state: the two
    chi2 arrays (each edge's last computed chi2), updated in place.  Returns
    (S, iterations)."""
    lam, ni, cur, nbad = 0.0, 2.0, 0.0, 0
    for it in range(10):
        if it >= maxit:
            return S, maxit
        H, b, cur, c12, c21 = build(pr, S, active, True, fix_scale)
        state[0][active] = c12[active]
        state[1][active] = c21[active]
        if it == 0:
            mx = 0.0
            for j in range(7):
                a = abs(float(H[j, j]))
                mx = mx if a < mx else a
            lam = 1e-5 * mx
            ni, nbad = 2.0, 0
        ini = cur
        rho, q = 0.0, 0
        trials = []
        while True:
            x = solve(H, b, lam)
            bk = S
            tmp, sc = DBL_MAX, 0.0
            if x is not None:
                S = sim3_update(S, x, fix_scale)
                tmp = errors(pr, S, active, True, state)
                with np.errstate(all="ignore"):
                    for j in range(7):
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
                    S = bk
            q += 1
            if not (rho < 0 and q < 10):
                break
        trace.append({"trials": trials, "chi": cur})
        if q == 10 or rho == 0:
            trace[-1]["end"] = "terminate"
            return S, it + 1
        nbad = nbad + 1 if (ini - cur) * 1e3 < ini else 0
        if nbad >= 3:
            trace[-1]["end"] = "non-improving"
            return S, it + 1
    return S, 10


def pack(S):
    """(q, t, s) as the eight doubles of orbx_sim3"""
    return np.array(list(S[0]) + list(S[1]) + [S[2]], np.float64)


def optimize_sim3(S12, cam1, cam2, corr, th2, fix_scale):
    """Returns dict: S (8,) f64 (q, t, s), removed (n,) uint8, chi2_12, chi2_21
    (n,) f64, n_inliers, iterations (2,) int32, early (the return before
    g2oS12 is written), rounds: per run round {"active", "max_iterations",
    "iterations": trace per LM iteration, "removed": flags after its
    classification}, depth: (z of e12's point, z of e21's) under the input."""
    pr = Problem(cam1, cam2, corr, th2)
    n = pr.n
    S0 = sim3_from(S12)
    raw = np.ascontiguousarray(S12).reshape(-1)[:1].tobytes()   # (the early return hands the input back as it is)
    res = {"S": np.frombuffer(raw, np.float64).copy(), "removed": np.zeros(n, np.uint8),
           "chi2_12": np.zeros(n), "chi2_21": np.zeros(n), "n_inliers": 0, "iterations": np.zeros(2, np.int32),
           "early": True, "rounds": [],
           "depth": (edge_error(pr, 0, S0)[2], edge_error(pr, 1, sim3_inverse(S0))[2])}
    if n == 0:
        return res
    state = [res["chi2_12"], res["chi2_21"]]
    removed = res["removed"]
    S = S0
    active = np.ones(n, bool)
    trace = []
    S, res["iterations"][0] = lm(pr, S, active, fix_scale, 5, state, trace)
    bad = (state[0] > pr.th2) | (state[1] > pr.th2)              # a NaN compares false: an inlier
    removed[bad] = 1
    nbad = int(bad.sum())
    res["rounds"].append({"active": n, "max_iterations": 5, "iterations": trace, "removed": removed.copy()})
    if n - nbad < 10:
        return res
    active = ~bad
    more = 10 if nbad > 0 else 5
    trace = []
    S, res["iterations"][1] = lm(pr, S, active, fix_scale, more, state, trace)
    out = active & ((state[0] > pr.th2) | (state[1] > pr.th2))
    removed[out] = 2
    res["rounds"].append({"active": int(active.sum()), "max_iterations": more, "iterations": trace,
                          "removed": removed.copy()})
    res["n_inliers"] = int(n - nbad - out.sum())
    res["S"] = pack(S)
    res["early"] = False
    return res
