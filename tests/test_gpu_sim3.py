"""k_sim3_optimize / k_sim3_step / k_sim3_update (orbx_sim3.hip) against
pyref_sim3.py, the float64 numpy restatement of DESIGN.md §3.14, bit for bit.
The linear step is only +, -, x, / and sqrt in a fixed order, so its equality
is unconditional; the update and the full runs add sin and cos, whose device
results have to equal glibc's on the arguments reached (as in local BA and
pose optimisation already), and §3.14's own exp, a fixed sequence of exact
operations that both sides execute (the device's exp and glibc's differ in
the last bit at exp(-0.4), which this file's update test reaches).  The sizes are
the lane-stride edges and the ten-survivor threshold (sim3_cases.SIZES), with
the scale free and fixed."""
import numpy as np
import pytest

import pyref_sim3
import sim3_cases
from orb_slam_2_ros_amd.optimizer import (optimize_sim3, optimize_sim3_batch, sim3_debug_step, sim3_debug_update,
                                          sim3_device_buffers, sim3_device_launch)
from orb_slam_2_ros_amd.synth_sim3 import SIM3_DTYPE

pytestmark = pytest.mark.gpu


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def same64(a, b):
    return np.array_equal(bits(a), bits(b))


def doubles(S):
    return np.frombuffer(np.ascontiguousarray(S, SIM3_DTYPE).tobytes(), np.float64)


def assert_run_equal(dev, ref, what=""):
    So, rem, c12, c21, ninl, its = dev
    assert list(its) == list(ref["iterations"]), (what, list(its), list(ref["iterations"]))
    assert np.array_equal(rem, ref["removed"]), (what, np.nonzero(rem != ref["removed"])[0][:8])
    assert int(ninl) == ref["n_inliers"], what
    assert same64(doubles(So), ref["S"]), (what, doubles(So), ref["S"])
    assert same64(c12, ref["chi2_12"]), (what, np.nonzero(bits(c12) != bits(ref["chi2_12"]))[0][:8])
    assert same64(c21, ref["chi2_21"]), (what, np.nonzero(bits(c21) != bits(ref["chi2_21"]))[0][:8])


@pytest.mark.parametrize("name", sim3_cases.SIZE_CASES, ids=sim3_cases.case_id)
def test_step_is_bit_equal(name):
    """H, b, the robust chi2 and x of one linear system: robust on and off,
    three lambdas (small, moderate, dominating H), all correspondences and a
    partial active set."""
    P = sim3_cases.problem(name)
    n, fix, cams = len(P["corr"]), P["fix_scale"], (P["cam1"], P["cam2"])
    partial = np.random.default_rng(n).random(n) < 0.7
    for active in (None, partial):
        for robust in (True, False):
            for lam in (1e-3, 10.0, 1e7):
                H, b, x, chi, ok = sim3_debug_step(P["S12"], *cams, P["corr"], active, robust, lam, fix, P["th2"])
                Hr, br, xr, chir, okr = pyref_sim3.sim3_step(P["S12"], cams, P["corr"], active, robust, lam, fix,
                                                             P["th2"])
                what = (name, active is not None, robust, lam)
                assert ok == okr, what
                assert same64(H, Hr), (what, "H", np.abs(H - Hr).max())
                assert same64(b, br), (what, "b", np.abs(b - br).max())
                assert same64([chi], [chir]), (what, "chi2", chi, chir)
                assert same64(x, xr), (what, "x", x, xr)


def test_step_reports_a_system_that_is_not_positive_definite():
    """One correspondence and lambda = 0: H has rank 4 at most, so a pivot of
    the Cholesky is zero up to rounding; whatever its sign comes out as, both
    sides must agree on solved and on x.  No correspondence at all (H = 0) is
    the exact case.  With a fixed scale and lambda = 0 the seventh pivot is
    exactly zero."""
    P = sim3_cases.problem((10, False))
    cams = (P["cam1"], P["cam2"])
    for i in range(10):
        K = P["corr"][i:i + 1]
        *_, x, _, ok = sim3_debug_step(P["S12"], *cams, K, None, True, 0.0, False, P["th2"])
        *_, xr, _, okr = pyref_sim3.sim3_step(P["S12"], cams, K, None, True, 0.0, False, P["th2"])
        assert ok == okr and same64(x, xr), i
    *_, ok = sim3_debug_step(P["S12"], *cams, P["corr"][:0], None, True, 0.0, False, P["th2"])
    assert not ok and not pyref_sim3.sim3_step(P["S12"], cams, P["corr"][:0], None, True, 0.0, False, P["th2"])[4]
    *_, ok = sim3_debug_step(P["S12"], *cams, P["corr"], None, True, 0.0, True, P["th2"])
    assert not ok and not pyref_sim3.sim3_step(P["S12"], cams, P["corr"], None, True, 0.0, True, P["th2"])[4]


def _updates():
    """Update vectors in all four branches of Sim3(Vector7d) (|sigma| and
    theta on either side of 1e-5, and at the thresholds), at sizes an LM run
    takes, on estimates with scales away from 1"""
    rng = np.random.default_rng(7)
    S, X = [], []
    for theta in (0.0, 3e-6, 9.999e-6, 1.0001e-5, 1e-3, 0.05, 0.7):
        for sigma in (0.0, 2e-6, -9.99e-6, 1.001e-5, -1e-3, 0.03, 0.69, -0.4):
            for _ in range(3):
                ax = rng.normal(size=3)
                w = theta * ax / np.linalg.norm(ax)
                X.append(np.concatenate([w, rng.normal(0, 0.1, 3), [sigma]]))
                P = sim3_cases.problem("scale-2" if len(X) % 2 else (65, False))
                S.append(P["S12"][0])
    return np.array(S, SIM3_DTYPE), np.array(X)


@pytest.mark.parametrize("fix", [False, True])
def test_update_is_bit_equal(fix):
    S, X = _updates()
    out = sim3_debug_update(S, X, fix)
    bad = []
    for k in range(len(S)):
        ref = pyref_sim3.pack(pyref_sim3.sim3_update(pyref_sim3.sim3_from(S[k:k + 1]), X[k], fix))
        if not same64(doubles(out[k:k + 1]), ref):
            bad.append((k, list(X[k]), list(doubles(out[k:k + 1])), list(ref)))
    assert not bad, (len(bad), bad[:3])
    if fix:
        assert np.array_equal(out["s"].view(np.uint64), S["s"].view(np.uint64))


@pytest.mark.parametrize("name", sim3_cases.ALL, ids=sim3_cases.case_id)
def test_full_run_is_bit_equal(name):
    P = sim3_cases.problem(name)
    dev = optimize_sim3(P["S12"], P["cam1"], P["cam2"], P["corr"], P["th2"], P["fix_scale"])
    assert_run_equal(dev, sim3_cases.reference(name), name)
    if sim3_cases.reference(name)["early"]:
        assert dev[0].tobytes() == P["S12"].tobytes() and dev[4] == 0


def _batch(names):
    Ps = [sim3_cases.problem(nm) for nm in names]
    S = np.concatenate([P["S12"] for P in Ps])
    C1 = np.concatenate([P["cam1"] for P in Ps])
    C2 = np.concatenate([P["cam2"] for P in Ps])
    K = np.concatenate([P["corr"] for P in Ps])
    off = np.concatenate([[0], np.cumsum([len(P["corr"]) for P in Ps])]).astype(np.int32)
    th = np.array([P["th2"] for P in Ps], np.float32)
    fix = np.array([P["fix_scale"] for P in Ps], np.int32)
    return S, C1, C2, K, off, th, fix


def _assert_batch(res, names, off):
    So, rem, c12, c21, ninl, its = (np.asarray(a) for a in res)
    for p, nm in enumerate(names):
        s = slice(off[p], off[p + 1])
        assert_run_equal((So[p:p + 1], rem[s], c12[s], c21[s], ninl[p], its[p]), sim3_cases.reference(nm), (p, nm))


EMPTY = (0, False)
BATCH_ALL = [EMPTY] + list(sim3_cases.ALL[:13]) + [EMPTY, (0, True)] + list(sim3_cases.ALL[13:]) + [EMPTY]
BATCH_SMALL = [(9, True), "early-return", EMPTY, (65, False)]


def test_batch_of_all_cases_equals_single_calls():
    """Every case in one CSR batch, empty problems first, in the middle and
    last: each problem equals its reference, which the single calls equal too
    (test_full_run_is_bit_equal); three of them are compared to their single
    calls directly."""
    args = _batch(BATCH_ALL)
    res = optimize_sim3_batch(*args)
    _assert_batch(res, BATCH_ALL, args[4])
    for p in (3, 14, len(BATCH_ALL) - 2):
        P = sim3_cases.problem(BATCH_ALL[p])
        one = optimize_sim3(P["S12"], P["cam1"], P["cam2"], P["corr"], P["th2"], P["fix_scale"])
        s = slice(args[4][p], args[4][p + 1])
        assert one[0].tobytes() == res[0][p:p + 1].tobytes() and np.array_equal(one[1], res[1][s])
        assert same64(one[2], res[2][s]) and same64(one[3], res[3][s])
        assert one[4] == res[4][p] and list(one[5]) == list(res[5][p])


def test_device_entry_on_a_side_stream_equals_the_host_batch():
    import torch
    args = _batch(BATCH_ALL)
    host = optimize_sim3_batch(*args)
    dev = optimize_sim3_batch(*args, stream=torch.cuda.Stream())
    for h, d in zip(host, dev):
        assert np.asarray(h).tobytes() == np.asarray(d).tobytes()


def test_device_buffers_reused_for_a_smaller_batch_keep_no_state():
    """The _device entry twice on the same output tensors, the large batch and
    then a small one: the small one's results are its own, and what lies
    beyond them is the large batch's, untouched."""
    import torch
    st = torch.cuda.Stream()
    big, small = _batch(BATCH_ALL), _batch(BATCH_SMALL)
    with torch.cuda.stream(st):
        ins, outs = sim3_device_buffers(*big, st.device)
        sim3_device_launch(ins, outs, len(BATCH_ALL), st)
        st.synchronize()
        first = [o.cpu().numpy().copy() for o in outs]
        ins2, _ = sim3_device_buffers(*small, st.device)
        sim3_device_launch(ins2, outs, len(BATCH_SMALL), st)
        st.synchronize()
        second = [o.cpu().numpy() for o in outs]
    P, N = len(BATCH_SMALL), len(small[3])
    So = np.frombuffer(second[0].tobytes(), SIM3_DTYPE)
    _assert_batch((So[:P], second[1][:N], second[2][:N], second[3][:N], second[4][:P], second[5][:P]), BATCH_SMALL,
                  small[4])
    assert second[0][64 * P:].tobytes() == first[0][64 * P:].tobytes()
    assert second[1][N:].tobytes() == first[1][N:].tobytes() and second[2][N:].tobytes() == first[2][N:].tobytes()
    # and the workspace of the host entry points: a smaller batch after a larger one
    _assert_batch(optimize_sim3_batch(*big), BATCH_ALL, big[4])
    _assert_batch(optimize_sim3_batch(*small), BATCH_SMALL, small[4])
