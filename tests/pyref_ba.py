"""Dense reference for local bundle adjustment (Optimizer::LocalBundleAdjustment
over g2o), independent of oracle/orbx_oracle.cpp and of orbx_ba.hip: plain
numpy, no Schur complement, no per-point inverses.

  * ba_dense_system: the full (6 nf + 3 npt)^2 normal equations of one
    Levenberg-Marquardt linearisation, in np.longdouble.  The Jacobians are
    derived here from the left perturbation p' = p + w x p + v of the camera
    point p = R X + t (they are not g2o's closed forms; test_ba_reference.py
    checks them against central differences of edge_errors).
  * ba_backward_error: the normwise backward error of a step x of
    (H + lam I) x = b.
  * local_ba_ref: the two-pass run in float64, a dense solve per LM trial.

Conventions of the reference (g2o types_six_dof_expmap, Optimizer.cc):
unknowns are the free poses (rotation w, then translation v, six each, in
camera order), then the points; the error is observation minus projection;
the stereo projection rounds 1/z to float, the mono one does not; the Huber
deltas are floats; a pose enters through Eigen's matrix -> quaternion
conversion, normalised, and back to a matrix."""
from __future__ import annotations

import numpy as np

LD = np.longdouble
CHI2_MONO, CHI2_STEREO = 5.991, 7.815
DELTA_MONO = float(np.float32(np.sqrt(5.991)))      # const float thHuberMono = sqrt(5.991)
DELTA_STEREO = float(np.float32(np.sqrt(7.815)))


def _quat_from_matrix(m):
    """Eigen's Quaternion(Matrix3) (Shepperd's branches), as (x, y, z, w)."""
    q = np.zeros(4)
    tr = m[0, 0] + m[1, 1] + m[2, 2]
    if tr > 0:
        s = np.sqrt(tr + 1.0)
        q[3] = 0.5 * s
        s = 0.5 / s
        q[0] = (m[2, 1] - m[1, 2]) * s
        q[1] = (m[0, 2] - m[2, 0]) * s
        q[2] = (m[1, 0] - m[0, 1]) * s
    else:
        i = 0
        if m[1, 1] > m[0, 0]:
            i = 1
        if m[2, 2] > m[i, i]:
            i = 2
        j, k = (i + 1) % 3, (i + 2) % 3
        s = np.sqrt(m[i, i] - m[j, j] - m[k, k] + 1.0)
        q[i] = 0.5 * s
        s = 0.5 / s
        q[3] = (m[k, j] - m[j, k]) * s
        q[j] = (m[j, i] + m[i, j]) * s
        q[k] = (m[k, i] + m[i, k]) * s
    return q


def _matrix_from_quat(q):
    x, y, z, w = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def poses_in(Tcw):
    """(ncam, 3, 4) float poses -> (R (ncam, 3, 3), t (ncam, 3)) float64, the
    rotation as the reference holds it: matrix -> quaternion, w >= 0, unit
    norm, -> matrix."""
    T = np.asarray(Tcw, np.float32).reshape(-1, 3, 4).astype(np.float64)
    R = np.empty((len(T), 3, 3))
    for c in range(len(T)):
        q = _quat_from_matrix(T[c, :, :3])
        if q[3] < 0:
            q = -q
        R[c] = _matrix_from_quat(q / np.sqrt((q * q).sum()))
    return R, T[:, :, 3].copy()


def _f(E, name, dtype):
    return E[name].astype(np.float64).astype(dtype)


def edge_errors(R, t, X, E, float_invz=True):
    """Camera points and errors of every edge at (R, t, X), in their dtype.
    Returns (p (ne, 3), r (ne, 3), stereo (ne,) bool); a mono edge's third
    error is 0.  float_invz: the stereo projection's 1/z rounded to float, as
    the reference does (off for the finite-difference check)."""
    dt = X.dtype
    cam, pt = E["cam"], E["point"]
    p = (R[cam] * X[pt][:, None, :]).sum(-1) + t[cam]
    stereo = E["ur"] >= 0
    invz = 1 / p[:, 2]
    if float_invz:
        invz = np.where(stereo, invz.astype(np.float32).astype(dt), invz)
    u = p[:, 0] * invz * _f(E, "fx", dt) + _f(E, "cx", dt)
    v = p[:, 1] * invz * _f(E, "fy", dt) + _f(E, "cy", dt)
    ur = u - _f(E, "bf", dt) * invz
    r = np.stack([_f(E, "u", dt) - u, _f(E, "v", dt) - v, np.where(stereo, _f(E, "ur", dt) - ur, 0)], 1)
    return p, r, stereo


def edge_jacobians(R, p, E):
    """d error / d (w, v) (ne, 3, 6) and d error / d X (ne, 3, 3) at camera
    points p.  With p' = p + w x p + v:  dp/dw = -[p]x, dp/dv = I, dp/dX = R,
    and the error is -projection, so J = -dproj/dp . dp/d(.)."""
    dt = p.dtype
    ne = len(E)
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    fx, fy, bf = _f(E, "fx", dt), _f(E, "fy", dt), _f(E, "bf", dt)
    stereo = E["ur"] >= 0
    dpi = np.zeros((ne, 3, 3), dt)                      # d (u, v, ur) / d p
    dpi[:, 0, 0] = fx / z
    dpi[:, 0, 2] = -fx * x / (z * z)
    dpi[:, 1, 1] = fy / z
    dpi[:, 1, 2] = -fy * y / (z * z)
    dpi[:, 2, 0] = np.where(stereo, fx / z, 0)
    dpi[:, 2, 2] = np.where(stereo, (bf - fx * x) / (z * z), 0)
    dp = np.zeros((ne, 3, 6), dt)                       # d p / d (w, v)
    dp[:, 0, 1], dp[:, 0, 2] = z, -y                    # -[p]x
    dp[:, 1, 0], dp[:, 1, 2] = -z, x
    dp[:, 2, 0], dp[:, 2, 1] = y, -x
    dp[:, 0, 3] = dp[:, 1, 4] = dp[:, 2, 5] = 1
    Jpose = -(dpi[:, :, :, None] * dp[:, None, :, :]).sum(2)
    Jpt = -(dpi[:, :, :, None] * R[E["cam"]][:, None, :, :]).sum(2)
    return Jpose, Jpt


def robust_weights(r, E, robust):
    """chi2, rho0 (the robustified cost) and rho1 (its derivative) per edge."""
    dt = r.dtype
    chi2 = _f(E, "inv_sigma2", dt) * (r * r).sum(1)
    if not robust:
        return chi2, chi2.copy(), np.ones_like(chi2)
    delta = np.where(E["ur"] >= 0, DELTA_STEREO, DELTA_MONO).astype(dt)
    out = chi2 > delta * delta
    s = np.sqrt(np.where(out, chi2, 1))
    return chi2, np.where(out, 2 * s * delta - delta * delta, chi2), np.where(out, delta / s, 1)


def _system(R, t, X, free_idx, E, active, robust):
    """(H, b, rho0 sum, chi2 per edge, p) at the state (R, t, X)."""
    dt = X.dtype
    nf, npt = int((free_idx >= 0).sum()), len(X)
    m = 6 * nf + 3 * npt
    p, r, _ = edge_errors(R, t, X, E)
    chi2, rho0, rho1 = robust_weights(r, E, robust)
    act = np.asarray(active, bool)
    H = np.zeros((m + 6, m + 6), dt)                    # (the last six: a bin for the fixed cameras' pose blocks)
    b = np.zeros(m + 6, dt)
    if act.any():
        Ea = E[act]
        Jp, Jl = edge_jacobians(R, p[act], Ea)
        J = np.concatenate([Jp, Jl], 2)                 # (na, 3, 9)
        w = (rho1[act] * _f(Ea, "inv_sigma2", dt))
        f = free_idx[Ea["cam"]]
        idx = np.concatenate([np.where(f >= 0, 6 * f, m)[:, None] + np.arange(6),
                              (6 * nf + 3 * Ea["point"])[:, None] + np.arange(3)], 1)
        He = (J[:, :, :, None] * J[:, :, None, :] * w[:, None, None, None]).sum(1)
        be = -(J * (w[:, None] * r[act])[:, :, None]).sum(1)
        np.add.at(H, (idx[:, :, None], idx[:, None, :]), He)
        np.add.at(b, idx, be)
    return H[:m, :m], b[:m], rho0[act].sum(), chi2, p


def free_index(fixed):
    fixed = np.asarray(fixed).astype(bool)
    return np.where(fixed, -1, np.cumsum(~fixed) - 1)


def ba_dense_system(Tcw, fixed, Xw, edges, active, robust):
    """(H, b, rho0_sum) in np.longdouble: H x = b is the undamped normal
    system of the linearisation at (Tcw, Xw) over the active edges, the edge
    weight rho1 * inv_sigma2; fixed cameras contribute point blocks only."""
    R, t = poses_in(Tcw)
    X = np.asarray(Xw, np.float32).reshape(-1, 3).astype(np.float64).astype(LD)
    H, b, s, _, _ = _system(R.astype(LD), t.astype(LD), X, free_index(fixed), edges, active, robust)
    return H, b, s


def ba_backward_error(H, b, lam, x):
    """eta = |b - M x|_inf / (|M|_inf |x|_inf + |b|_inf), M = H + lam I, in
    np.longdouble: the smallest relative perturbation of (M, b) that makes x
    an exact solution (Rigal-Gaches)."""
    M = np.asarray(H, LD) + LD(lam) * np.eye(len(b), dtype=LD)
    x = np.asarray(x, LD)
    r = np.asarray(b, LD) - M @ x
    return np.abs(r).max() / (np.abs(M).sum(1).max() * np.abs(x).max() + np.abs(b).max())


def _se3_exp(d):
    """(R, V) of the update d = (w, v): rotation by Rodrigues' formula and the
    matrix V with translation V v; below 1e-5 rad the reference takes
    R = V = I + [w]x + [w]x^2."""
    w = d[:3]
    th = np.sqrt(w @ w)
    K = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])
    K2 = K @ K
    if th < 1e-5:
        Rm = np.eye(3) + K + K2
        return Rm, Rm
    a, bb, c = np.sin(th) / th, (1 - np.cos(th)) / th ** 2, (th - np.sin(th)) / th ** 3
    return np.eye(3) + a * K + bb * K2, np.eye(3) + bb * K + c * K2


def local_ba_ref(Tcw, fixed, Xw, edges, iters=(5, 10), details=False):
    """The two LM passes of LocalBundleAdjustment with a dense float64 solve
    per trial: pass 1 with Huber kernels on every edge; edges with chi2 over
    5.991 (mono) / 7.815 (stereo) or non-positive depth leave; pass 2 without
    kernels; final flags by the same rule, an inactive edge keeping its last
    chi2 and the depth taken at the final estimate for every edge.  Returns
    (Tcw f32, Xw f32, outlier, (it1, it2)); details adds a dict with the
    per-edge chi2 and depth and the nearest |chi2 / threshold - 1| of the two
    decisions."""
    E = edges
    R, t = poses_in(Tcw)
    X = np.asarray(Xw, np.float32).reshape(-1, 3).astype(np.float64)
    fidx = free_index(fixed)
    free = np.nonzero(fidx >= 0)[0]
    nf, ne = len(free), len(E)
    th = np.where(E["ur"] >= 0, CHI2_STEREO, CHI2_MONO)
    chi2 = np.zeros(ne)                                  # e->chi2() as last computed while active

    def errors(act, robust):
        _, r, _ = edge_errors(R, t, X, E)
        c, rho0, _ = robust_weights(r, E, robust)
        chi2[act] = c[act]
        return rho0[act].sum()

    def lm(n_iter, act, robust):
        nonlocal R, t, X
        lam, nu, nbad = 0.0, 2.0, 0
        for it in range(n_iter):
            H, b, cur, c, _ = _system(R, t, X, fidx, E, act, robust)
            chi2[act] = c[act]
            ini = cur
            if it == 0:
                lam = 1e-5 * (np.abs(np.diag(H)).max() if len(b) else 0.0)
                nu, nbad = 2.0, 0
            rho, q = 0.0, 0
            while True:
                keep = (R, t, X)
                try:
                    x = np.linalg.solve(H + lam * np.eye(len(b)), b)
                    ok = bool(np.isfinite(x).all())
                except np.linalg.LinAlgError:
                    ok = False
                tmp = np.finfo(np.float64).max
                if ok:
                    Rn, tn = R.copy(), t.copy()
                    for k, c_ in enumerate(free):
                        Re, V = _se3_exp(x[6 * k:6 * k + 6])
                        Rn[c_] = Re @ R[c_]
                        tn[c_] = Re @ t[c_] + V @ x[6 * k + 3:6 * k + 6]
                    R, t, X = Rn, tn, X + x[6 * nf:].reshape(-1, 3)
                    tmp = errors(act, robust)
                rho = (cur - tmp) / ((x @ (lam * x + b) if ok else 0.0) + 1e-3)
                if rho > 0 and np.isfinite(tmp):
                    lam *= max(1 / 3, min(1 - (2 * rho - 1) ** 3, 2 / 3))
                    nu = 2.0
                    cur = tmp
                else:
                    lam *= nu
                    nu *= 2
                    R, t, X = keep
                q += 1
                if not (rho < 0 and q < 10):
                    break
            if q == 10 or rho == 0:
                return it + 1
            nbad = nbad + 1 if (ini - cur) * 1e3 < ini else 0
            if nbad >= 3:
                return it + 1
        return n_iter

    def depth():
        return edge_errors(R, t, X, E)[0][:, 2]

    act = np.ones(ne, bool)
    it1 = lm(iters[0], act, True)
    margin = np.inf
    it2 = 0
    if iters[1] > 0:
        if ne:
            margin = np.abs(chi2 / th - 1).min()
        act = ~((chi2 > th) | ~(depth() > 0))
        it2 = lm(iters[1], act, False)
    z = depth()
    outlier = (chi2 > th) | ~(z > 0)
    if ne:
        margin = min(margin, np.abs(chi2 / th - 1).min())
    To = np.concatenate([R, t[:, :, None]], 2).astype(np.float32)
    out = (To, X.astype(np.float32), outlier, (it1, it2))
    if details:
        out += ({"chi2": chi2.copy(), "depth": z, "margin": float(margin), "active2": act},)
    return out
