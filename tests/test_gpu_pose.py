"""k_pose_optimize / k_pose_step (orbx_pose.hip) against pyref_pose.py, the
float64 numpy restatement of DESIGN.md §3.13, bit for bit: the linear step is
only +, -, x, / and sqrt in a fixed order; the full runs add the exponential's
sin / cos / pow, on whose device-versus-glibc agreement local BA's parity
(test_gpu_ba.py) already rests.  The sizes are the lane-stride edges
(pose_cases.SIZES), mixed, all-mono and all-stereo."""
import numpy as np
import pytest

import pose_cases
import pyref_pose
from orb_slam_2_ros_amd.optimizer import pose_debug_step, pose_optimization, pose_optimization_batch
from orb_slam_2_ros_amd.synth_pose import POSE_CAM_DTYPE, make_pose_problem

pytestmark = pytest.mark.gpu

SIZE_CASES = [(n, k) for n in pose_cases.SIZES for k in pose_cases.KINDS]


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def same64(a, b):
    return np.array_equal(bits(a), bits(b))


def assert_run_equal(dev, ref, what=""):
    To, out, chi2, ninl, its = dev
    assert list(its) == list(ref["iterations"]), (what, list(its), list(ref["iterations"]))
    assert np.array_equal(out, ref["outlier"]), (what, np.nonzero(out != ref["outlier"])[0][:8])
    assert int(ninl) == ref["n_inliers"], what
    assert np.array_equal(np.asarray(To, np.float32).view(np.uint32), ref["Tcw"].view(np.uint32)), \
        (what, To, ref["Tcw"])
    assert same64(chi2, ref["chi2"]), (what, np.nonzero(bits(chi2) != bits(ref["chi2"]))[0][:8])


@pytest.mark.parametrize("name", SIZE_CASES, ids=pose_cases.case_id)
def test_step_is_bit_equal(name):
    """H, b, the robust chi2 and x of one linear system: robust on and off,
    three lambdas (small, moderate, dominating H), all observations and a
    partial active set."""
    P = pose_cases.problem(name)
    n = len(P["obs"])
    rng = np.random.default_rng(n)
    partial = rng.random(n) < 0.7
    for active in (None, partial):
        for robust in (True, False):
            for lam in (1e-3, 10.0, 1e7):
                H, b, x, chi, ok = pose_debug_step(P["Tcw"], P["cam"], P["obs"], active, robust, lam)
                Hr, br, xr, chir, okr = pyref_pose.pose_step(P["Tcw"], P["cam"], P["obs"], active, robust, lam)
                what = (name, active is not None, robust, lam)
                assert ok == okr, what
                assert same64(H, Hr), (what, "H", np.abs(H - Hr).max())
                assert same64(b, br), (what, "b", np.abs(b - br).max())
                assert same64([chi], [chir]), (what, "chi2", chi, chir)
                assert same64(x, xr), (what, "x", x, xr)


def test_step_reports_a_system_that_is_not_positive_definite():
    """One observation and lambda = 0: H has rank 2 (mono) or 3 (stereo), so a
    pivot of the Cholesky is zero up to rounding.  Observations 0-2 (mono,
    stereo, mono) give a pivot <= 0 in the reference and must report solved =
    0 on the device too; observation 3's rounds to a tiny positive number, and
    there both sides must agree on solved = 1 and on x.  No observation at all
    (H = 0) is the exact case."""
    P = pose_cases.problem((10, "mixed"))
    for i in range(10):
        obs = P["obs"][i:i + 1]
        *_, x, _, ok = pose_debug_step(P["Tcw"], P["cam"], obs, None, True, 0.0)
        *_, xr, _, okr = pyref_pose.pose_step(P["Tcw"], P["cam"], obs, None, True, 0.0)
        assert ok == okr and same64(x, xr), i
        if i < 3:
            assert not ok and not okr and not x.any()
        if i == 3:
            assert ok and okr
    *_, ok = pose_debug_step(P["Tcw"], P["cam"], P["obs"][:0], None, True, 0.0)
    assert not ok and not pyref_pose.pose_step(P["Tcw"], P["cam"], P["obs"][:0], None, True, 0.0)[4]


@pytest.mark.parametrize("name", pose_cases.ALL, ids=pose_cases.case_id)
def test_full_run_is_bit_equal(name):
    P = pose_cases.problem(name)
    assert_run_equal(pose_optimization(P["Tcw"], P["cam"], P["obs"]), pose_cases.reference(name), name)


def _batch(names):
    Ps = [pose_cases.problem(nm) for nm in names]
    T = np.stack([P["Tcw"] for P in Ps])
    C = np.concatenate([P["cam"] for P in Ps])
    O = np.concatenate([P["obs"] for P in Ps])
    off = np.concatenate([[0], np.cumsum([len(P["obs"]) for P in Ps])]).astype(np.int32)
    return T, C, O, off


def _assert_batch(res, names, off):
    To, out, chi2, ninl, its = (np.asarray(a) for a in res)
    for p, nm in enumerate(names):
        s = slice(off[p], off[p + 1])
        assert_run_equal((To[p], out[s].astype(bool), chi2[s], ninl[p], its[p]), pose_cases.reference(nm), (p, nm))


BATCH_A = [(65, "mixed"), (0, "mixed"), (130, "stereo"), (2, "mono"), (300, "mixed")]
BATCH_B = [(9, "mixed"), (64, "mono"), (3, "stereo"), (63, "mixed"), (10, "mixed"), "behind"]


def test_batch_equals_single_calls():
    T, C, O, off = _batch(BATCH_A)
    res = pose_optimization_batch(T, C, O, off)
    _assert_batch(res, BATCH_A, off)
    for p, nm in enumerate(BATCH_A):
        P = pose_cases.problem(nm)
        To, out, chi2, ninl, its = pose_optimization(P["Tcw"], P["cam"], P["obs"])
        s = slice(off[p], off[p + 1])
        assert np.array_equal(To.view(np.uint32), res[0][p].view(np.uint32))
        assert np.array_equal(out, res[1][s]) and same64(chi2, res[2][s])
        assert ninl == res[3][p] and list(its) == list(res[4][p])


def _to_torch(T, C, O, off):
    import torch
    Cf = np.stack([C[k] for k in POSE_CAM_DTYPE.names], 1).astype(np.float32)
    Of = np.ascontiguousarray(O).view(np.float32).reshape(-1, 7)
    return [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in (T, Cf, Of, off)]


def test_device_entry_equals_host_batch_and_keeps_no_state():
    """The _device entry on torch tensors, then the same buffers reused for
    another batch of other sizes: each equals its own reference."""
    import torch
    args_a, args_b = _batch(BATCH_A), _batch(BATCH_B)
    cap_p = max(len(BATCH_A), len(BATCH_B))
    cap_n = max(len(args_a[2]), len(args_b[2]))
    dT = torch.zeros((cap_p, 3, 4), dtype=torch.float32, device="cuda")
    dC = torch.zeros((cap_p, 5), dtype=torch.float32, device="cuda")
    dO = torch.zeros((cap_n, 7), dtype=torch.float32, device="cuda")
    doff = torch.zeros(cap_p + 1, dtype=torch.int32, device="cuda")
    from orb_slam_2_ros_amd._lib import check, load
    dTo = torch.empty_like(dT)
    dout = torch.full((cap_n,), 7, dtype=torch.uint8, device="cuda")
    dchi = torch.full((cap_n,), float("nan"), dtype=torch.float64, device="cuda")
    dninl = torch.full((cap_p,), -1, dtype=torch.int32, device="cuda")
    dits = torch.full((cap_p, 4), -1, dtype=torch.int32, device="cuda")
    for names, args in ((BATCH_A, args_a), (BATCH_B, args_b)):
        tT, tC, tO, toff = _to_torch(*args)
        P, N = len(names), len(args[2])
        dT[:P], dC[:P], dO[:N], doff[:P + 1] = tT, tC, tO, toff
        check(load().orbx_pose_optimization_batch_device(
            dT.data_ptr(), dC.data_ptr(), dO.data_ptr(), doff.data_ptr(), P, dTo.data_ptr(), dout.data_ptr(),
            dchi.data_ptr(), dninl.data_ptr(), dits.data_ptr(), torch.cuda.current_stream().cuda_stream), "device")
        torch.cuda.synchronize()
        res = (dTo[:P].cpu().numpy(), dout[:N].cpu().numpy(), dchi[:N].cpu().numpy(), dninl[:P].cpu().numpy(),
               dits[:P].cpu().numpy())
        _assert_batch(res, names, args[3])
    # the Python wrapper on tensors
    res = pose_optimization_batch(*_to_torch(*args_a))
    torch.cuda.synchronize()
    _assert_batch([r.cpu().numpy() for r in res], BATCH_A, args_a[3])


def test_two_hundred_problems_map_to_their_workgroups():
    """200 different problems of 65 observations: problem p's results must be
    problem p's."""
    Ps = [make_pose_problem(65, seed=1000 + p) for p in range(200)]
    T = np.stack([P["Tcw"] for P in Ps])
    C = np.concatenate([P["cam"] for P in Ps])
    O = np.concatenate([P["obs"] for P in Ps])
    off = (65 * np.arange(201)).astype(np.int32)
    To, out, chi2, ninl, its = pose_optimization_batch(T, C, O, off)
    for p, P in enumerate(Ps):
        ref = pyref_pose.pose_optimization(P["Tcw"], P["cam"], P["obs"])
        s = slice(off[p], off[p + 1])
        assert_run_equal((To[p], out[s], chi2[s], ninl[p], its[p]), ref, p)
