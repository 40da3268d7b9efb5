"""Pose optimisation without a GPU: pyref_pose's linear step against an
independent np.longdouble system built from pyref_ba's machinery (the local-BA
edges' Jacobians, derived there from the left perturbation and checked
against central differences), its robust chi2 sum against the longdouble sum,
its classification on a problem with planted outliers, the shared cases
against what they are meant to reach, and the C API's argument checks, which
come before the device is touched."""
import numpy as np
import pytest

import pose_cases
import pyref_ba
import pyref_pose
from orb_slam_2_ros_amd import _lib
from orb_slam_2_ros_amd.optimizer import pose_debug_step, pose_optimization_batch
from orb_slam_2_ros_amd.synth_ba import BA_EDGE_DTYPE
from orb_slam_2_ros_amd.synth_pose import make_pose_problem

LD = np.longdouble
U = 2.0 ** -53

STEP_CASES = [(300, "mixed"), (130, "stereo"), (65, "mixed"), (64, "mono"), (10, "mixed")]


def ba_edges(P):
    """The problem as local-BA edges of camera 0 and one point per observation"""
    O, c = P["obs"], P["cam"][0]
    E = np.zeros(len(O), BA_EDGE_DTYPE)
    E["cam"], E["point"] = 0, np.arange(len(O))
    for k in ("u", "v", "ur", "inv_sigma2"):
        E[k] = O[k]
    for k in ("fx", "fy", "cx", "cy", "bf"):
        E[k] = c[k]
    return E


def dense_pose_system(P, active, robust):
    """(Hpp, bp, rho0 sum) in np.longdouble: the pose block of the full normal
    equations with one free camera, the points held as data"""
    H, b, s = pyref_ba.ba_dense_system(P["Tcw"][None], [0], P["obs"]["Xw"], ba_edges(P), active, robust)
    return H[:6, :6], b[:6], s


def step_bound(n):
    """(n + 40) 2^-53.  A recursive sum of n terms carries at most (n - 1) u;
    each term a handful of roundings; |dH_ab| <= gamma sqrt(H_aa H_bb) <=
    gamma |M|_inf; a 6x6 Cholesky with its two triangular solves adds at most
    about 3 * 6 + 1 + 2 * 6 units."""
    return (n + 40) * U


@pytest.mark.parametrize("robust", [True, False])
@pytest.mark.parametrize("name", STEP_CASES, ids=pose_cases.case_id)
def test_step_solves_independent_dense_system(name, robust):
    P = pose_cases.problem(name)
    n = len(P["obs"])
    rng = np.random.default_rng(n + 1)
    for active in (np.ones(n, bool), rng.random(n) < 0.7):
        Hd, bd, _ = dense_pose_system(P, active, robust)
        lam0 = 1e-5 * float(np.abs(np.diag(Hd)).max())
        for lam in (lam0, 1e3 * lam0, 1e6 * lam0):
            H, b, x, chi, ok = pyref_pose.pose_step(P["Tcw"], P["cam"], P["obs"], active, robust, lam)
            assert ok
            eta = float(pyref_ba.ba_backward_error(Hd, bd, lam, x))
            print(f"{pose_cases.case_id(name)} robust={robust} lam={lam:.2e}: eta {eta:.3e}, bound {step_bound(n):.3e}")
            assert eta <= step_bound(n), eta
            # one observation left out of the system
            drop = active.copy()
            drop[np.nonzero(active)[0][len(active) // 7]] = False
            x1 = pyref_pose.pose_step(P["Tcw"], P["cam"], P["obs"], drop, robust, lam)[2]
            assert float(pyref_ba.ba_backward_error(Hd, bd, lam, x1)) > step_bound(n)
            # the sign of one Jacobian column flipped
            x2 = pyref_pose.pose_step(P["Tcw"], P["cam"], P["obs"], active, robust, lam, mutate={"jsign": (2, -1.0)})[2]
            assert float(pyref_ba.ba_backward_error(Hd, bd, lam, x2)) > step_bound(n)


@pytest.mark.parametrize("robust", [True, False])
@pytest.mark.parametrize("name", STEP_CASES, ids=pose_cases.case_id)
def test_robust_chi2_sum_equals_longdouble_sum(name, robust):
    """The lane-ordered float64 sum of the observations' rho0 against (1) the
    robust chi2 the dense np.longdouble system forms from longdouble errors and
    (2) the np.longdouble sum of the same float64 terms: n 2^-53 relative
    each (two recursive sums of at most n / 64 + 64 non-negative terms, so the
    sum's condition is 1; (1) adds each term's own roundings).  Leaving one
    observation out exceeds both."""
    P = pose_cases.problem(name)
    n = len(P["obs"])
    pr = pyref_pose.Problem(P["cam"], P["obs"])
    pose = pyref_pose.pose_from_cv(P["Tcw"])
    active = np.random.default_rng(n + 2).random(n) < 0.8
    _, _, chi2 = pyref_pose.errors(pr, pose)
    rho0 = pyref_pose.huber(pr, chi2, robust)[0]
    chi = pyref_pose.pose_step(P["Tcw"], P["cam"], P["obs"], active, robust, 1.0)[3]
    exact = rho0[active].astype(LD).sum()
    rel = float(abs(LD(chi) - exact) / exact)
    dense = dense_pose_system(P, active, robust)[2]
    print(f"{pose_cases.case_id(name)} robust={robust}: rel {rel:.3e}, bound {n * U:.3e}; "
          f"to the longdouble-error sum {float(abs(LD(chi) - dense) / dense):.3e}")
    assert rel <= n * U
    assert float(abs(LD(chi) - dense) / dense) <= n * U
    drop = active.copy()
    drop[np.nonzero(active)[0][3]] = False
    chi1 = pyref_pose.pose_step(P["Tcw"], P["cam"], P["obs"], drop, robust, 1.0)[3]
    assert float(abs(LD(chi1) - exact) / exact) > n * U and float(abs(LD(chi1) - dense) / dense) > n * U


@pytest.mark.parametrize("kind", list(pose_cases.KINDS))
def test_planted_outliers_are_the_flagged_set(kind):
    P = make_pose_problem(200, seed=31, stereo_frac=pose_cases.KINDS[kind], outlier_frac=0.1, noise_px=0.0,
                          outlier_px=50.0)
    assert 5 <= P["planted"].sum() <= 40
    r = pyref_pose.pose_optimization(P["Tcw"], P["cam"], P["obs"])
    assert np.array_equal(r["outlier"], P["planted"])
    assert r["n_inliers"] == 200 - int(P["planted"].sum())
    assert np.abs(r["Tcw"] - P["Tcw_true"]).max() < 1e-3


def _trials(r):
    return [t for rd in r["rounds"] for it in rd["iterations"] for t in it["trials"]]


def test_cases_reach_what_they_are_for():
    ref = pose_cases.reference
    rs = ref("returns")["rounds"]
    assert any((rs[0]["outlier"] & ~rs[k]["outlier"]).any() for k in range(1, len(rs)))
    assert any(t["solved"] and not t["accepted"] for t in _trials(ref("rejected")))
    assert any(rd["iterations"][-1].get("end") == "non-improving" and len(rd["iterations"]) < 10
               for rd in ref("non-improving")["rounds"])
    r = ref("empty-round")
    assert len(r["rounds"]) == 4 and r["rounds"][1]["active"] == 0 and r["iterations"][1] == 0
    r = ref("nine")
    assert len(r["rounds"]) == 1 and r["iterations"][0] > 0 and list(r["iterations"][1:]) == [0, 0, 0]
    r = ref("two")
    P = pose_cases.problem("two")
    assert r["n_inliers"] == 0 and not r["outlier"].any() and list(r["iterations"]) == [0, 0, 0, 0]
    assert r["Tcw"].tobytes() == P["Tcw"].tobytes()
    r = ref("behind")
    assert all(rd["depth"][5] < -1.0 for rd in r["rounds"]) and r["outlier"][5]
    O = pose_cases.problem("ur-edges")["obs"]
    assert O["ur"][3] == 0.0 and O["ur"][4] == -1.0
    pr = pyref_pose.Problem(pose_cases.problem("ur-edges")["cam"], O)
    assert pr.stereo[3] and not pr.stereo[4]
    assert ref("ur-edges")["outlier"][3]                      # ur = 0 is a gross stereo error, not a mono edge
    # every size case runs to an end with a finite pose
    for name in pose_cases.ALL:
        assert np.isfinite(ref(name)["Tcw"]).all(), name


def test_empty_round_keeps_the_initial_pose():
    """All twelve observations are flagged after round 0, so rounds 1-3 run
    nothing and the result is toCvMat(toSE3Quat(Tcw)) of the input."""
    P, r = pose_cases.problem("empty-round"), pose_cases.reference("empty-round")
    assert r["rounds"][0]["outlier"].all() and r["n_inliers"] == 0
    assert np.array_equal(r["Tcw"], pyref_pose.pose_to_cv(pyref_pose.pose_from_cv(P["Tcw"])))


def _einval(fn, *args, **kw):
    with pytest.raises(_lib.OrbxError) as ei:
        fn(*args, **kw)
    assert ei.value.code == _lib.ORBX_EINVAL, ei.value


def test_pose_argument_checks_precede_the_device():
    """Nulls, negative counts and offsets that do not ascend (or do not start
    at 0) are ORBX_EINVAL with or without a device (ORBX_ENODEV would mean the
    device came first)."""
    import ctypes
    from orb_slam_2_ros_amd._lib import load, ptr
    lib = load()
    P = pose_cases.problem((10, "mixed"))
    T, C, O = P["Tcw"], P["cam"], P["obs"]
    To, out, chi2 = np.zeros((2, 3, 4), np.float32), np.zeros(32, np.uint8), np.zeros(32)
    ninl, its = np.zeros(2, np.int32), np.zeros((2, 4), np.int32)
    EINVAL = _lib.ORBX_EINVAL
    one = lib.orbx_pose_optimization
    assert one(0, None, ptr(C), ptr(O), 10, ptr(To), ptr(out), ptr(chi2), ptr(ninl), ptr(its)) == EINVAL
    assert one(0, ptr(T), None, ptr(O), 10, ptr(To), ptr(out), ptr(chi2), ptr(ninl), ptr(its)) == EINVAL
    assert one(0, ptr(T), ptr(C), None, 10, ptr(To), ptr(out), ptr(chi2), ptr(ninl), ptr(its)) == EINVAL
    assert one(0, ptr(T), ptr(C), ptr(O), -1, ptr(To), ptr(out), ptr(chi2), ptr(ninl), ptr(its)) == EINVAL
    assert one(0, ptr(T), ptr(C), ptr(O), 10, None, ptr(out), ptr(chi2), ptr(ninl), ptr(its)) == EINVAL
    assert one(0, ptr(T), ptr(C), ptr(O), 10, ptr(To), None, ptr(chi2), ptr(ninl), ptr(its)) == EINVAL
    assert one(0, ptr(T), ptr(C), ptr(O), 10, ptr(To), ptr(out), ptr(chi2), None, ptr(its)) == EINVAL
    T2, C2 = np.stack([T, T]), np.concatenate([C, C])
    bat = lib.orbx_pose_optimization_batch
    for off in ([0, 6, 4], [1, 5, 10], [0, -1, 10]):
        off = np.array(off, np.int32)
        assert bat(0, ptr(T2), ptr(C2), ptr(O), ptr(off), 2, ptr(To), ptr(out), ptr(chi2), ptr(ninl),
                   ptr(its)) == EINVAL
    off = np.array([0, 5, 10], np.int32)
    assert bat(0, ptr(T2), ptr(C2), ptr(O), ptr(off), -1, ptr(To), ptr(out), ptr(chi2), ptr(ninl), ptr(its)) == EINVAL
    assert bat(0, ptr(T2), ptr(C2), ptr(O), None, 2, ptr(To), ptr(out), ptr(chi2), ptr(ninl), ptr(its)) == EINVAL
    dev = lib.orbx_pose_optimization_batch_device
    assert dev(None, None, None, None, 2, None, None, None, None, None, None) == EINVAL
    assert dev(None, None, None, None, -1, None, None, None, None, None, None) == EINVAL
    H, b, x = np.zeros(36), np.zeros(6), np.zeros(6)
    c, ok = ctypes.c_double(0), ctypes.c_int(0)
    step = lib.orbx_pose_debug_step
    assert step(0, ptr(T), ptr(C), ptr(O), -1, None, 1, 1.0, ptr(H), ptr(b), ptr(x), ctypes.byref(c),
                ctypes.byref(ok)) == EINVAL
    assert step(0, ptr(T), ptr(C), None, 10, None, 1, 1.0, ptr(H), ptr(b), ptr(x), ctypes.byref(c),
                ctypes.byref(ok)) == EINVAL
    assert step(0, ptr(T), ptr(C), ptr(O), 10, None, 1, 1.0, None, ptr(b), ptr(x), ctypes.byref(c),
                ctypes.byref(ok)) == EINVAL
    # the Python wrappers raise the same code
    _einval(pose_optimization_batch, T2, C2, O, np.array([0, 12, 10], np.int32))
    with pytest.raises(ValueError):
        pose_debug_step(T, C, O, active=np.ones(3, np.uint8))
