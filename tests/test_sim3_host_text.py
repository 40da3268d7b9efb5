"""orbx_sim3.h compiled for the host (tools/sim3_host: the text the kernel
compiles, its 64 lanes run one after another) against pyref_sim3.py, bit for
bit and without a GPU: the linear step, the update in all four branches, the
perturbation table's constants and the full runs of every shared case.  What
tests/test_gpu_sim3.py asserts of the device, asserted of the same text on a
CPU; the two differ only in the compiler's target and the library's sin / cos."""
import ctypes
import sys
from pathlib import Path

import numpy as np
import pytest

import pyref_sim3
import sim3_cases
from orb_slam_2_ros_amd._lib import ptr
from orb_slam_2_ros_amd.synth_sim3 import SIM3_DTYPE

sys.path.insert(0, str(Path(__file__).resolve().parents[1] / "tools" / "sim3_host"))


@pytest.fixture(scope="module")
def host():
    import sim3_host_build as host_build
    return host_build.load()


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def same64(a, b):
    return np.array_equal(bits(a), bits(b))


def test_host_step_is_bit_equal(host):
    for name in sim3_cases.SIZE_CASES:
        P = sim3_cases.problem(name)
        n, fix = len(P["corr"]), P["fix_scale"]
        act = (np.random.default_rng(n).random(n) < 0.7).astype(np.uint8)
        for active in (None, act):
            for robust in (True, False):
                for lam in (1e-3, 1e7):
                    H, b, x = np.zeros(49), np.zeros(7), np.zeros(7)
                    chi, ok = ctypes.c_double(0), ctypes.c_int(0)
                    host.sim3_host_step(ptr(P["S12"]), ptr(P["cam1"]), ptr(P["cam2"]), ptr(P["corr"]), n, P["th2"],
                                        int(fix), ptr(active) if n else None, int(robust), lam, ptr(H), ptr(b),
                                        ptr(x), ctypes.byref(chi), ctypes.byref(ok))
                    Hr, br, xr, chir, okr = pyref_sim3.sim3_step(P["S12"], (P["cam1"], P["cam2"]), P["corr"], active,
                                                                 robust, lam, fix, P["th2"])
                    what = (name, active is not None, robust, lam)
                    assert bool(ok.value) == okr, what
                    assert same64(H, Hr.reshape(-1)) and same64(b, br) and same64(x, xr), what
                    assert same64([chi.value], [chir]), what


def test_host_update_and_table_are_bit_equal(host):
    rng = np.random.default_rng(7)
    S0 = sim3_cases.problem("scale-2")["S12"]
    for theta in (0.0, 3e-6, 1.0001e-5, 1e-3, 0.7):
        for sigma in (0.0, 2e-6, 1.001e-5, -1e-3, 0.69, -0.4):
            ax = rng.normal(size=3)
            x = np.concatenate([theta * ax / np.linalg.norm(ax), rng.normal(0, 0.1, 3), [sigma]])
            for fix in (0, 1):
                out = np.zeros(1, SIM3_DTYPE)
                host.sim3_host_update(ptr(S0), ptr(x), 1, fix, ptr(out))
                ref = pyref_sim3.pack(pyref_sim3.sim3_update(pyref_sim3.sim3_from(S0), x, fix))
                assert out.tobytes() == ref.tobytes(), (theta, sigma, fix)
    for fix in (0, 1):
        for k in range(1, 15):
            tab, exp = np.zeros(1, SIM3_DTYPE), np.zeros(1, SIM3_DTYPE)
            host.sim3_host_perturbation(k, fix, ptr(tab))
            u = np.zeros(7)
            u[(k - 1) >> 1] = 1e-9 if k & 1 else -1e-9
            if fix:
                u[6] = 0.0
            host.sim3_host_exp(ptr(u), ptr(exp))
            assert tab.tobytes() == exp.tobytes() == pyref_sim3.pack(pyref_sim3.perturbation(k, fix)).tobytes(), (k, fix)


@pytest.mark.parametrize("name", sim3_cases.ALL, ids=sim3_cases.case_id)
def test_host_full_run_is_bit_equal(name, host):
    P, ref = sim3_cases.problem(name), sim3_cases.reference(name)
    n = len(P["corr"])
    So, rem = np.zeros(1, SIM3_DTYPE), np.zeros(n + 1, np.uint8)
    c12, c21 = np.zeros(n + 1), np.zeros(n + 1)
    ninl, its = ctypes.c_int(-1), np.zeros(2, np.int32)
    host.sim3_host_optimize(ptr(P["S12"]), ptr(P["cam1"]), ptr(P["cam2"]), ptr(P["corr"]), n, P["th2"],
                            int(P["fix_scale"]), ptr(So), ptr(rem), ptr(c12), ptr(c21), ctypes.byref(ninl), ptr(its))
    assert list(its) == list(ref["iterations"]) and ninl.value == ref["n_inliers"]
    assert np.array_equal(rem[:n], ref["removed"])
    assert So.tobytes() == ref["S"].tobytes()
    assert same64(c12[:n], ref["chi2_12"]) and same64(c21[:n], ref["chi2_21"])
