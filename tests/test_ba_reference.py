"""Local bundle adjustment against an independent dense reference
(pyref_ba.py), without a GPU: the reference's Jacobians against central
differences of its own error function; the oracle's LM step against the
reference's full normal equations by backward error; the oracle's two-pass
run against the reference's; and the C API's argument checks, which come
before the device is touched."""
import numpy as np
import pytest

import ba_cases
import pyref_ba
from orb_slam_2_ros_amd import _lib
from orb_slam_2_ros_amd.optimizer import debug_step, local_bundle_adjustment
from orb_slam_2_ros_amd.synth_ba import make_ba_problem

LD = np.longdouble

# pyref <-> oracle distance of the full runs, measured on the CPU: float32
# ulps of the array's largest magnitude (ba_cases.ulps32), poses and points.
# Iteration counts (5, 10) and outlier flags were identical on every case.
# The tests assert twice these, and never more than 8 ulps.
FULL_ULPS = {
    "full-3": (0.0, 0.0),
    "full-5-mono": (0.0, 0.0),
    "full-7": (0.0, 0.0),
    "full-6-stereo": (0.125, 4.0),
    "degenerate": (0.03125, 3.0),
    "behind": (0.0, 0.0),
    "degenerate-unique": (0.046875, 3.0),
}


def full_bounds(name):
    return tuple(min(2 * u, 8.0) for u in FULL_ULPS[name])


def test_reference_jacobians_match_central_differences():
    """Pose and point blocks of a dozen random mono and stereo edges, in
    np.longdouble.  Central differences with step h = eps^(1/3) (the variables
    are of order 1: radians, metres at ~10 m depth) carry a truncation error
    ~h^2 and a rounding error ~eps / h, both ~eps^(2/3) = 2.3e-13 relative to
    the function's scale; the tolerance is 100 eps^(2/3) of the block's largest
    entry, ten orders below a wrong sign or a swapped term.  The differenced
    error function keeps 1/z exact: the reference's float rounding of it is
    not differentiable, and its analytic Jacobian ignores it too."""
    eps = np.finfo(LD).eps
    h = eps ** (LD(1) / 3)
    tol = 100 * eps ** (LD(2) / 3)
    P = make_ba_problem(n_local=4, n_fixed=2, n_points=30, seed=21)
    rng = np.random.default_rng(3)
    E = P["edges"]
    mono, stereo = np.nonzero(E["ur"] < 0)[0], np.nonzero(E["ur"] >= 0)[0]
    pick = np.concatenate([rng.choice(mono, 6, replace=False), rng.choice(stereo, 6, replace=False)])
    R64, t64 = pyref_ba.poses_in(P["Tcw"])
    R, t, X = R64.astype(LD), t64.astype(LD), P["Xw"].astype(np.float64).astype(LD)
    for e in pick:
        Ee = E[e:e + 1]
        cam, pt = int(Ee["cam"][0]), int(Ee["point"][0])
        p, _, _ = pyref_ba.edge_errors(R, t, X, Ee, float_invz=False)
        Jp, Jl = pyref_ba.edge_jacobians(R, p, Ee)
        rows = 3 if Ee["ur"][0] >= 0 else 2
        assert np.all(Jp[0, rows:] == 0) and np.all(Jl[0, rows:] == 0)

        def err(d_pose, d_pt):
            Re, V = pyref_ba._se3_exp(d_pose)
            R2, t2, X2 = R.copy(), t.copy(), X.copy()
            R2[cam] = Re @ R[cam]
            t2[cam] = Re @ t[cam] + V @ d_pose[3:]
            X2[pt] = X[pt] + d_pt
            return pyref_ba.edge_errors(R2, t2, X2, Ee, float_invz=False)[1][0]

        z6, z3 = np.zeros(6, LD), np.zeros(3, LD)
        for k in range(6):
            d = z6.copy()
            d[k] = h
            fd = (err(d, z3) - err(-d, z3)) / (2 * h)
            assert np.abs(fd - Jp[0, :, k]).max() <= tol * np.abs(Jp[0]).max(), (e, "pose", k)
        for k in range(3):
            d = z3.copy()
            d[k] = h
            fd = (err(z6, d) - err(z6, -d)) / (2 * h)
            assert np.abs(fd - Jl[0, :, k]).max() <= tol * np.abs(Jl[0]).max(), (e, "point", k)


@pytest.mark.parametrize("robust,lam", ba_cases.STEP_MODES)
@pytest.mark.parametrize("name", ba_cases.STEP_CASES)
def test_oracle_step_solves_dense_system(name, robust, lam, oracle_mod):
    """The oracle's Schur-complement step x must solve the reference's full
    system (H + lam I) x = b to a backward error of m 2^-53 (m unknowns; the
    c n eps bound of a backward-stable solve.  Measured at most 4.5e-16; with
    one edge left out of the oracle's Hll every case fails, the smallest eta
    3.1e-11 on max-170 against its bound of 1.5e-13), and its robust chi2 sum must
    equal the reference's to 1e-13 relative."""
    P = ba_cases.problem(name)
    H, b, chi = ba_cases.step_reference(name, robust)
    x, c, ok = oracle_mod.ba_debug_step(P["Tcw"], P["fixed"], P["Xw"], P["edges"], robust, lam)
    assert ok and len(x) == len(b)
    assert abs(c - float(chi)) <= 1e-13 * float(chi), (c, float(chi))
    eta = float(pyref_ba.ba_backward_error(H, b, lam, x))
    print(f"{name} robust={robust}: eta {eta:.3e}, bound {ba_cases.step_bound(P):.3e}")
    assert eta <= ba_cases.step_bound(P), eta


@pytest.mark.parametrize("name", ba_cases.FULL_CASES)
def test_oracle_local_ba_matches_reference(name, oracle_mod):
    P = ba_cases.problem(name)
    Tr, Xr, out_r, it_r, info = ba_cases.full_reference(name)
    To, Xo, out_o, it_o = oracle_mod.local_ba(P["Tcw"], P["fixed"], P["Xw"], P["edges"])
    assert it_o == it_r
    assert np.array_equal(out_o, out_r), np.nonzero(out_o != out_r)[0][:8]
    dT, dX = ba_cases.ulps32(To, Tr), ba_cases.ulps32(Xo, Xr)
    print(f"{name}: poses {dT} ulps, points {dX} ulps, nearest threshold margin {info['margin']:.2e}")
    bT, bX = full_bounds(name)
    assert dT <= bT and dX <= bX, (dT, dX)


def test_behind_camera_edge_is_flagged_by_depth_alone(oracle_mod):
    """The added edge of the `behind` problem fits (chi2 far under 7.815) at
    the reference's final estimate and its point stays behind the camera: the
    depth test is all that flags it, in the reference and in the oracle."""
    P = ba_cases.problem("behind")
    _, _, out_r, _, info = ba_cases.full_reference("behind")
    assert info["chi2"][-1] < 0.1 and info["depth"][-1] < -1.0
    assert out_r[-1] and not info["active2"][-1]
    out_o = oracle_mod.local_ba(P["Tcw"], P["fixed"], P["Xw"], P["edges"])[2]
    assert out_o[-1]


def _einval(fn, *args, **kw):
    with pytest.raises(_lib.OrbxError) as ei:
        fn(*args, **kw)
    assert ei.value.code == _lib.ORBX_EINVAL, ei.value


@pytest.mark.parametrize("fast", [False, True])
def test_ba_argument_checks_precede_the_device(fast):
    """171 free cameras, an edge naming camera ncam and an edge naming point
    -1 are ORBX_EINVAL from both entry points, with or without a device
    (ORBX_ENODEV would mean the device came first)."""
    P = ba_cases.problem("tiny")
    T, F, X, E = P["Tcw"], P["fixed"], P["Xw"], P["edges"]
    big_T = np.tile(T[:1], (172, 1, 1))
    big_F = np.zeros(172, np.uint8)
    big_F[0] = 1                                         # 171 free
    bad_cam, bad_pt = E.copy(), E.copy()
    bad_cam["cam"][3] = len(T)
    bad_pt["point"][5] = -1
    for args in [(big_T, big_F, X, E[:0]), (T, F, X, bad_cam), (T, F, X, bad_pt)]:
        _einval(local_bundle_adjustment, *args, fast=fast)
        _einval(debug_step, *args, fast=fast)
