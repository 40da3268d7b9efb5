"""Sim3 optimisation without a GPU: pyref_sim3's error functions against an
independently written np.longdouble projection (rotation matrices, not
quaternion products), its numeric Jacobian against the same central difference
in longdouble and against analytic derivatives, its normal equations and solve
against the longdouble system of its own Jacobian, the constants of the
perturbation table, its classification on planted outliers, the shared cases
against what they are meant to reach, and the C API's argument checks, which
come before the device is touched."""
import ctypes
import math

import numpy as np
import pytest

import pyref_ba
import pyref_sim3
import sim3_cases
from orb_slam_2_ros_amd import _lib
from orb_slam_2_ros_amd.optimizer import optimize_sim3_batch, sim3_debug_step, sim3_debug_update
from orb_slam_2_ros_amd.synth_sim3 import SIM3_DTYPE, make_sim3_problem

LD = np.longdouble
U = 2.0 ** -53
DELTA = 1e-9
K_ROUND = 32

ERR_CASES = [(130, False), (65, True), "scale-2", "behind", "fixed-scale"]


# ---- the independent longdouble model -------------------------------------------
def rot_of(q):
    """(1 - 2 |u|^2) I + 2 u u^T + 2 w [u]x for q = (u, w) of any norm: what
    Eigen's q * v applies, as a matrix"""
    x, y, z, w = (LD(v) for v in q)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]], LD)


def affine_of(S):
    """(A, t) with map(X) = A X + t, A = s R"""
    q, t, s = S
    return LD(s) * rot_of(q), np.array(t, LD)


def ld_edge(P, edge, A, t):
    """The edge's error in longdouble at the affine map (A, t) (e12) or at its
    inverse (e21): (e (n, 2), p (n, 3), magnitude (n,)), magnitude = the sum of
    the absolute values that enter a component of p."""
    corr, cams = P["corr"], (P["cam1"][0], P["cam2"][0])
    if edge == 0:
        X = corr["P2c"].astype(LD)
        M, m = A, t
        mag = np.abs(X) @ np.abs(M).T + np.abs(m)
    else:
        X = corr["P1c"].astype(LD)
        M = np.linalg.inv(A.astype(np.float64)).astype(LD)
        for _ in range(3):                               # Newton steps to longdouble accuracy
            M = M + M @ (np.eye(3, dtype=LD) - A @ M)
        m = -(M @ t)
        mag = np.abs(X) @ np.abs(M).T + np.abs(M) @ np.abs(t)
    p = X @ M.T + m
    c = cams[edge]
    fx, fy, cx, cy = (LD(np.float32(c[k])) for k in ("fx", "fy", "cx", "cy"))
    u, v = (corr[k].astype(LD) for k in (("u1", "v1") if edge == 0 else ("u2", "v2")))
    e = np.stack([u - (p[:, 0] / p[:, 2] * fx + cx), v - (p[:, 1] / p[:, 2] * fy + cy)], 1)
    return e, p, mag.max(1), (fx, fy, cx, cy, u, v)


def error_bound(p, mag, cam):
    """E (n, 2): the forward-error bound of an edge's float64 error.

    A component of p is a sum of products of at most K roundings (the two
    cross products, the doubling, the final sums of quat_rotate: 10; s r + t:
    2; for e21 the inverse's own rotate and scalings: 12 more; under K = 32
    with slack), so |dp| <= K u mag.  The ratio x / z then carries
    (|dp_x| + |x / z| |dp_z|) / |z| + u |x / z|, the camera map multiplies by f
    and adds two roundings, the subtraction from the observation one: 4 u
    (|obs| + |f x / z| + |c|) covers those."""
    fx, fy, cx, cy, u, v = cam
    z = np.abs(p[:, 2])
    out = []
    for f, c, o, x in ((fx, cx, u, p[:, 0]), (fy, cy, v, p[:, 1])):
        r = np.abs(x) / z
        out.append(LD(U) * (K_ROUND * f * mag / z * (1 + r) + 4 * (np.abs(o) + f * r + abs(c))))
    return np.stack(out, 1)


def ld_perturbed(S, k, fix_scale):
    """Entry k of the table as an affine map in longdouble"""
    A, t = affine_of(S)
    if k == 0:
        return A, t
    Pa, Pt = affine_of(pyref_sim3.perturbation(k, fix_scale))
    return Pa @ A, Pa @ t + Pt


def ld_jacobian(P, edge, S, fix_scale):
    """The central difference of ld_edge over the table's perturbations, (n, 2, 7)"""
    cols = []
    for d in range(7):
        ep = ld_edge(P, edge, *ld_perturbed(S, 1 + 2 * d, fix_scale))[0]
        em = ld_edge(P, edge, *ld_perturbed(S, 2 + 2 * d, fix_scale))[0]
        cols.append((ep - em) / (2 * LD(DELTA)))
    return np.stack(cols, 2)


def skew(p):
    z = np.zeros(len(p), LD)
    return np.stack([np.stack([z, -p[:, 2], p[:, 1]], 1), np.stack([p[:, 2], z, -p[:, 0]], 1),
                     np.stack([-p[:, 1], p[:, 0], z], 1)], 1)


def analytic_jacobian(P, edge, S, fix_scale):
    """d e / d eps at eps = 0 of S' = Sim3(eps) S, eps = (omega, upsilon,
    sigma): for e12 p' = exp(eps) p, so dp = [-[p]x | I | p]; for e21
    p' = S^-1 exp(-eps) X, so dp = A^-1 [[X]x | -I | -X]."""
    A, t = affine_of(S)
    e, p, _, cam = ld_edge(P, edge, A, t)
    n = len(p)
    eye = np.broadcast_to(np.eye(3, dtype=LD), (n, 3, 3))
    if edge == 0:
        dp = np.concatenate([-skew(p), eye, p[:, :, None]], 2)
    else:
        X = P["corr"]["P1c"].astype(LD)
        Ai = np.linalg.inv(A.astype(np.float64)).astype(LD)
        for _ in range(3):
            Ai = Ai + Ai @ (np.eye(3, dtype=LD) - A @ Ai)
        dp = np.einsum("ij,njk->nik", Ai, np.concatenate([skew(X), -eye, -X[:, :, None]], 2))
    fx, fy = cam[0], cam[1]
    z = p[:, 2]
    zero = np.zeros(n, LD)
    Jpi = np.stack([np.stack([fx / z, zero, -fx * p[:, 0] / (z * z)], 1),
                    np.stack([zero, fy / z, -fy * p[:, 1] / (z * z)], 1)], 1)
    J = -np.einsum("nij,njk->nik", Jpi, dp)
    if fix_scale:
        J[:, :, 6] = 0
    return J


def pyref_lin(P, S, fix_scale, mutate=None):
    """pyref_sim3's errors and numeric Jacobians of both edges: [(e (n, 2), J (n, 2, 7))] * 2"""
    pr = pyref_sim3.Problem(P["cam1"], P["cam2"], P["corr"], P["th2"])
    tab = pyref_sim3.table(S, fix_scale)
    out = []
    for edge in (0, 1):
        e0, e1, _ = pyref_sim3.edge_error(pr, edge, tab[0][edge])
        J = pyref_sim3.numeric_jacobian(pr, edge, tab, mutate)
        out.append((np.stack([e0, e1], 1), np.stack([np.stack(J[k], 1) for k in range(2)], 1)))
    return out


def case(name):
    P = sim3_cases.problem(name)
    return P, pyref_sim3.sim3_from(P["S12"]), P["fix_scale"]


# ---- 1: error functions -----------------------------------------------------------
@pytest.mark.parametrize("name", ERR_CASES, ids=sim3_cases.case_id)
def test_error_functions_equal_longdouble_projection(name):
    """Both edges' float64 errors against the longdouble projection written
    with matrices, within error_bound (its docstring derives it)."""
    P, S, fix = case(name)
    A, t = affine_of(S)
    for edge, (e, _) in enumerate(pyref_lin(P, S, fix)):
        el, p, mag, cam = ld_edge(P, edge, A, t)
        E = error_bound(p, mag, cam)
        ratio = float((np.abs(e.astype(LD) - el) / E).max())
        print(f"{sim3_cases.case_id(name)} e{'12' if edge == 0 else '21'}: max error / bound {ratio:.3f}")
        assert ratio <= 1.0


# ---- 2, 3: numeric Jacobian ---------------------------------------------------------
@pytest.mark.parametrize("name", ERR_CASES, ids=sim3_cases.case_id)
def test_numeric_jacobian_float64_longdouble_analytic(name):
    """The float64 central difference carries each error's rounding divided
    by delta: |J64 - JLD| <= (E+ + E-) / (2 delta) <= E / delta with E the
    bound of test 1 at the estimate (the perturbed points differ from it by
    1e-9 relative).  The longdouble difference has 2^11 times less of it and a
    truncation error of order delta^2, so it must meet the analytic derivative
    within the same E / delta.  A column with its sign flipped, or a one-sided
    difference in the place of the central one (e- replaced by e in g2o's
    loop, its scalar 1 / (2 delta) unchanged: half the derivative), must not.
    The correctly scaled forward difference (e+ - e) / delta is printed and not
    asserted: its truncation error is of order delta (1e-9 times the second
    derivative) and its rounding noise twice the central one's, both far under
    a forward-error bound that has to cover the central difference's worst
    case, so no test at this tolerance can tell it from the central one."""
    P, S, fix = case(name)
    A, t = affine_of(S)
    lin = pyref_lin(P, S, fix)
    flipped = pyref_lin(P, S, fix, {"jsign": 1})
    one_sided = pyref_lin(P, S, fix, {"one_sided": 4})
    forward = pyref_lin(P, S, fix, {"forward": 4})
    for edge in (0, 1):
        _, p, mag, cam = ld_edge(P, edge, A, t)
        tol = (error_bound(p, mag, cam) / LD(DELTA))[:, :, None] * (1 + LD(1e-6))
        JL = ld_jacobian(P, edge, S, fix)
        JA = analytic_jacobian(P, edge, S, fix)
        r64 = float((np.abs(lin[edge][1].astype(LD) - JL) / tol).max())
        ran = float((np.abs(JL - JA) / tol).max())
        rfl = float((np.abs(flipped[edge][1].astype(LD) - JL) / tol).max())
        ros = float((np.abs(one_sided[edge][1].astype(LD) - JL) / tol).max())
        rfw = float((np.abs(forward[edge][1].astype(LD) - JL) / tol)[:, :, 4].max())
        print(f"{sim3_cases.case_id(name)} e{'12' if edge == 0 else '21'}: |J64 - JLD| / tol {r64:.3f}, "
              f"|JLD - Jan| / tol {ran:.2e}, flipped {rfl:.3g}, one-sided {ros:.3g}, "
              f"scaled forward difference (column 4) {rfw:.3g}")
        assert r64 <= 1.0
        assert ran <= 1.0
        assert rfl > 1.0
        assert ros > 1.0


# ---- 4: fixed scale -------------------------------------------------------------------
@pytest.mark.parametrize("name", [(65, True), "fixed-scale"], ids=sim3_cases.case_id)
def test_fixed_scale_zeroes_the_seventh_dimension(name):
    P, S, fix = case(name)
    assert fix
    for _, J in pyref_lin(P, S, True):
        assert not J[:, :, 6].any()
    for lam in (1e-3, 10.0):
        H, b, x, _, ok = pyref_sim3.sim3_step(S, (P["cam1"], P["cam2"]), P["corr"], None, True, lam, True, P["th2"])
        assert ok and not H[6].any() and not H[:, 6].any() and b[6] == 0 and x[6] == 0
    # the same problem with the scale free has a seventh column
    assert all(J[:, :, 6].any() for _, J in pyref_lin(P, S, False))


# ---- 5: normal equations ------------------------------------------------------------
def ld_system(P, lin, active, robust):
    """H, b in longdouble from pyref's own errors and Jacobians"""
    pr = pyref_sim3.Problem(P["cam1"], P["cam2"], P["corr"], P["th2"])
    H, b = np.zeros((7, 7), LD), np.zeros(7, LD)
    for edge, (e, J) in enumerate(lin):
        om = pr.w[edge].astype(LD)
        chi2 = (e.astype(LD) ** 2).sum(1) * om
        rho1 = np.ones(len(e), LD)
        if robust:
            out = ~(chi2 <= LD(pr.delta) ** 2)
            rho1 = np.where(out, LD(pr.delta) / np.sqrt(np.where(out, chi2, 1)), rho1)
        w = (rho1 * om)[active]
        Ja, ea = J.astype(LD)[active], e.astype(LD)[active]
        H += np.einsum("nki,n,nkj->ij", Ja, w, Ja)
        b += -np.einsum("nki,n,nk->i", Ja, w, ea)
    return H, b


def step_bound(n):
    """(2 n + 45) 2^-53: a recursive sum of 2 n edge terms carries at most
    (2 n - 1) u, each term a handful of roundings; a 7x7 Cholesky with its two
    triangular solves adds about 3 * 7 + 1 + 2 * 7 units (pose's step_bound
    with one more row)."""
    return (2 * n + 45) * U


@pytest.mark.parametrize("robust", [True, False])
@pytest.mark.parametrize("name", [(130, False), (65, False), (64, False), (20, False), "scale-2"],
                         ids=sim3_cases.case_id)
def test_step_solves_longdouble_normal_equations(name, robust):
    P, S, fix = case(name)
    n = len(P["corr"])
    lin = pyref_lin(P, S, fix)
    cams = (P["cam1"], P["cam2"])
    rng = np.random.default_rng(n + 1)
    for active in (np.ones(n, bool), rng.random(n) < 0.7):
        Hd, bd = ld_system(P, lin, active, robust)
        lam0 = 1e-5 * float(np.abs(np.diag(Hd)).max())
        for lam in (lam0, 1e3 * lam0, 1e6 * lam0):
            H, b, x, chi, ok = pyref_sim3.sim3_step(S, cams, P["corr"], active, robust, lam, fix, P["th2"])
            assert ok
            eta = float(pyref_ba.ba_backward_error(Hd, bd, lam, x))
            print(f"{sim3_cases.case_id(name)} robust={robust} lam={lam:.2e}: eta {eta:.3e}, bound {step_bound(n):.3e}")
            assert eta <= step_bound(n), eta
            k = int(np.nonzero(active)[0][len(active) // 7])
            drop = active.copy()
            drop[k] = False
            x1 = pyref_sim3.sim3_step(S, cams, P["corr"], drop, robust, lam, fix, P["th2"])[2]
            assert float(pyref_ba.ba_backward_error(Hd, bd, lam, x1)) > step_bound(n)
            x2 = pyref_sim3.sim3_step(S, cams, P["corr"], active, robust, lam, fix, P["th2"],
                                      mutate={"drop_e21": k})[2]
            assert float(pyref_ba.ba_backward_error(Hd, bd, lam, x2)) > step_bound(n)


# ---- 6: the table's constants ---------------------------------------------------------
def test_exp_literals_and_perturbation_table():
    assert pyref_sim3.EXP_PLUS == math.exp(1e-9) and pyref_sim3.EXP_MINUS == math.exp(-1e-9)
    assert LD(pyref_sim3.EXP_PLUS) == LD(np.float64(np.exp(LD(1e-9))))
    assert LD(pyref_sim3.EXP_MINUS) == LD(np.float64(np.exp(LD(-1e-9))))
    # the literals the kernel compiles are the same
    text = (_lib.LIB_PATH.parent / "csrc" / "orbx_sim3.h").read_text()
    assert float.fromhex(text.split("kSim3ExpPlus = ")[1].split(";")[0]) == pyref_sim3.EXP_PLUS
    assert float.fromhex(text.split("kSim3ExpMinus = ")[1].split(";")[0]) == pyref_sim3.EXP_MINUS
    # every entry is what Sim3(Vector7d) gives at +-1e-9 e_d, bit for bit
    for fix in (False, True):
        for k in range(1, 15):
            u = [0.0] * 7
            u[(k - 1) >> 1] = DELTA if k & 1 else -DELTA
            if fix:
                u[6] = 0.0
            assert pyref_sim3.pack(pyref_sim3.sim3_exp(u)).tobytes() == \
                pyref_sim3.pack(pyref_sim3.perturbation(k, fix)).tobytes(), (k, fix)


def test_update_reaches_all_four_branches():
    """Sim3(Vector7d)'s branches on |sigma| < 1e-5 and theta < 1e-5 against
    the closed forms in longdouble (rotation by Rodrigues, t = W upsilon with
    W the integral of the exponential).  Below 1e-5 the reference replaces
    the coefficients by their limits (C = 1, A = 1 / 2, B = 1 / 6, R = I +
    Omega + Omega^2), an error of the order of the argument, so the tolerance
    is 1e-5 |upsilon| there and stays that in the exact branch."""
    for w, sg in ((1e-7, 1e-7), (0.3, 1e-7), (1e-7, 0.2), (0.3, 0.2)):
        u = [w * 0.6, -w * 0.48, w * 0.64, 0.1, -0.2, 0.3, sg]
        q, t, s = pyref_sim3.sim3_exp(u)
        th = LD(w)
        k = np.array([0.6, -0.48, 0.64], LD)
        K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]], LD)
        R = np.eye(3, dtype=LD) + np.sin(th) * K + (1 - np.cos(th)) * K @ K
        assert float(np.abs(rot_of(q) - R).max()) < 1e-12
        assert abs(s - math.exp(sg)) <= 4 * U * s            # §3.14's exp: within about one ulp
        # W = int_0^1 exp(a (sigma I + [omega]x)) da, by Simpson's rule on 2000 panels
        a = np.linspace(0, 1, 2001).astype(LD)
        Ra = (np.eye(3, dtype=LD)[None] + np.sin(a * th)[:, None, None] * K + (1 - np.cos(a * th))[:, None, None] * (K @ K))
        f = np.exp(a * LD(sg))[:, None, None] * Ra
        wts = np.ones(2001, LD)
        wts[1:-1:2], wts[2:-1:2] = 4, 2
        W = (f * wts[:, None, None]).sum(0) / (3 * 2000)
        assert float(np.abs(W @ np.array(u[3:6], LD) - np.array(t, LD)).max()) < 1e-5 * 0.3, (w, sg)


# ---- 7: planted outliers ----------------------------------------------------------------
@pytest.mark.parametrize("fix", [False, True])
def test_planted_outliers_are_the_removed_set(fix):
    """A tenth of the correspondences moved by 50 px, no noise.  Tolerances:
    measured once on this case (the largest element of R - R_true 6.2e-9 with
    the scale free and 6.3e-9 fixed, translation 7.7e-8 / 7.9e-8 m, scale
    2.8e-7: the float32 rounding of the points and observations), written
    with a factor of about five of slack."""
    P = make_sim3_problem(200, seed=31, fix_scale=fix, outlier_frac=0.1, noise_px=0.0, outlier_px=50.0,
                          init_scale=1.0 if fix else None)
    assert 5 <= P["planted"].sum() <= 40
    r = sim3_cases.run_reference(P)
    assert np.array_equal(r["removed"] != 0, P["planted"])
    assert r["n_inliers"] == 200 - int(P["planted"].sum())
    q, t, s = r["S"][:4], r["S"][4:7], r["S"][7]
    dR = float(np.abs(rot_of(q / np.linalg.norm(q)).astype(np.float64) - P["R_true"]).max())
    dt = float(np.abs(t - P["t_true"]).max())
    print(f"fix={fix}: dR {dR:.2e}, dt {dt:.2e}, ds {abs(s - P['s_true']):.2e}")
    assert dR < 3e-8 and dt < 4e-7
    if fix:
        assert np.float64(s).tobytes() == P["S12"]["s"][0].tobytes()
    else:
        assert abs(s - P["s_true"]) < 1.5e-6


# ---- 8, 9: the cases --------------------------------------------------------------------
def test_cases_reach_what_they_are_for():
    ref, prob = sim3_cases.reference, sim3_cases.problem
    r = ref("bad-then-10")
    assert not r["early"] and (r["removed"] == 1).any() and r["rounds"][1]["max_iterations"] == 10
    assert r["rounds"][1]["active"] == len(r["removed"]) - int((r["rounds"][0]["removed"] == 1).sum())
    r = ref("clean-5")
    assert not r["early"] and not r["rounds"][0]["removed"].any() and r["rounds"][1]["max_iterations"] == 5
    assert r["iterations"][1] <= 5
    r = ref("early-return")
    n = len(r["removed"])
    assert n >= 10 and r["early"] and len(r["rounds"]) == 1 and n - int((r["removed"] == 1).sum()) < 10
    assert any(t["solved"] and not t["accepted"] for t in sim3_cases.trials(ref("rejected")))
    r = ref("behind")
    assert r["depth"][0][5] < -1.0 and r["depth"][1][5] > 1.0 and r["removed"][5] == 1
    assert (np.delete(r["depth"][0], 5) > 0).all() and (r["depth"][1] > 0).all()
    r, th2 = ref("one-sided"), prob("one-sided")["th2"]
    assert ((r["chi2_12"] <= th2) & (r["chi2_21"] > th2)).any() and ((r["chi2_21"] <= th2) & (r["chi2_12"] > th2)).any()
    P, r = prob("scale-2"), ref("scale-2")
    assert P["s_true"] == 2.0 and not P["fix_scale"] and P["S12"]["s"][0] == 1.0
    assert not r["early"] and abs(r["S"][7] - 2.0) < 0.1 and r["n_inliers"] > 50
    P, r = prob("fixed-scale"), ref("fixed-scale")
    assert P["fix_scale"] and P["S12"]["s"][0] != 1.0 and not r["early"]
    assert np.float64(r["S"][7]).tobytes() == P["S12"]["s"][0].tobytes()
    for name in sim3_cases.ALL:
        r = ref(name)
        assert np.isfinite(r["S"]).all(), name
        n = len(r["removed"])
        assert r["early"] == (n - int((r["removed"] == 1).sum()) < 10 or n == 0), name
        if n == 0:
            assert r["n_inliers"] == 0 and list(r["iterations"]) == [0, 0] and not r["rounds"]
        elif n < 10:
            assert r["early"] and r["iterations"][0] > 0 and r["iterations"][1] == 0


def test_early_return_hands_the_input_back():
    P, r = sim3_cases.problem("early-return"), sim3_cases.reference("early-return")
    assert r["S"].tobytes() == P["S12"].tobytes() and r["n_inliers"] == 0
    assert (r["removed"] == 1).sum() > 0 and not (r["removed"] == 2).any()
    assert np.array_equal(r["removed"], r["rounds"][0]["removed"])
    assert r["chi2_12"].any() and r["chi2_21"].any()   # round 0 ran


# ---- 10: argument checks ------------------------------------------------------------------
def _einval(fn, *args, **kw):
    with pytest.raises(_lib.OrbxError) as ei:
        fn(*args, **kw)
    assert ei.value.code == _lib.ORBX_EINVAL, ei.value


def test_sim3_argument_checks_precede_the_device():
    """Nulls, negative counts and offsets that do not ascend (or do not start
    at 0) are ORBX_EINVAL with or without a device (ORBX_ENODEV would mean the
    device came first)."""
    from orb_slam_2_ros_amd._lib import load, ptr
    lib = load()
    P = sim3_cases.problem((10, False))
    S, C1, C2, K = P["S12"], P["cam1"], P["cam2"], P["corr"]
    So, rem, a, b = np.zeros(2, SIM3_DTYPE), np.zeros(32, np.uint8), np.zeros(32), np.zeros(32)
    ninl, its = np.zeros(2, np.int32), np.zeros((2, 2), np.int32)
    EINVAL = _lib.ORBX_EINVAL
    one = lib.orbx_optimize_sim3
    good = [0, ptr(S), ptr(C1), ptr(C2), ptr(K), 10, 10.0, 0, ptr(So), ptr(rem), ptr(a), ptr(b), ptr(ninl), ptr(its)]
    for k in (1, 2, 3, 4, 8, 9, 12):
        args = list(good)
        args[k] = None
        assert one(*args) == EINVAL, k
    args = list(good)
    args[5] = -1
    assert one(*args) == EINVAL
    S2, C12, C22 = np.concatenate([S, S]), np.concatenate([C1, C1]), np.concatenate([C2, C2])
    th, fix = np.full(2, 10, np.float32), np.zeros(2, np.int32)
    bat = lib.orbx_optimize_sim3_batch

    def batch_args(off, nprob=2):
        return [0, ptr(S2), ptr(C12), ptr(C22), ptr(K), ptr(off), nprob, ptr(th), ptr(fix), ptr(So), ptr(rem), ptr(a),
                ptr(b), ptr(ninl), ptr(its)]
    for off in ([0, 6, 4], [1, 5, 10], [0, -1, 10]):
        assert bat(*batch_args(np.array(off, np.int32))) == EINVAL, off
    off = np.array([0, 5, 10], np.int32)
    assert bat(*batch_args(off, -1)) == EINVAL
    for k in (1, 2, 3, 4, 5, 7, 8, 9, 10, 13):
        args = batch_args(off)
        args[k] = None
        assert bat(*args) == EINVAL, k
    dev = lib.orbx_optimize_sim3_batch_device
    assert dev(*([None] * 5), 2, *([None] * 9)) == EINVAL
    assert dev(*([None] * 5), -1, *([None] * 9)) == EINVAL
    H, bb, x = np.zeros(49), np.zeros(7), np.zeros(7)
    c, ok = ctypes.c_double(0), ctypes.c_int(0)
    step = lib.orbx_sim3_debug_step
    good = [0, ptr(S), ptr(C1), ptr(C2), ptr(K), 10, 10.0, 0, None, 1, 1.0, ptr(H), ptr(bb), ptr(x), ctypes.byref(c),
            ctypes.byref(ok)]
    for k in (1, 2, 3, 4, 11, 12, 13, 14, 15):
        args = list(good)
        args[k] = None
        assert step(*args) == EINVAL, k
    args = list(good)
    args[5] = -1
    assert step(*args) == EINVAL
    upd = lib.orbx_sim3_debug_update
    X = np.zeros((1, 7))
    assert upd(0, None, ptr(X), 1, 0, ptr(So)) == EINVAL
    assert upd(0, ptr(S), None, 1, 0, ptr(So)) == EINVAL
    assert upd(0, ptr(S), ptr(X), 1, 0, None) == EINVAL
    assert upd(0, ptr(S), ptr(X), -1, 0, ptr(So)) == EINVAL
    # the Python wrappers raise the same code
    _einval(optimize_sim3_batch, S2, C12, C22, K, np.array([0, 12, 10], np.int32))
    with pytest.raises(ValueError):
        sim3_debug_step(S, C1, C2, K, active=np.ones(3, np.uint8))
    with pytest.raises(ValueError):
        sim3_debug_update(S, np.zeros((2, 7)))
    with pytest.raises(ValueError):
        optimize_sim3_batch(S2, C12, C22, K, np.array([0, 10], np.int32))
