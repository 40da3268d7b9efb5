"""integration/Optimizer_sim3_orbx.cc, the reference-side
Optimizer::OptimizeSim3: compiled against the test stand-ins of the reference
headers (tests/cxx/sim3_mock before tests/cxx/orbslam_mock) and run by
tests/cxx/sim3_forwarder_test.cpp on two keyframes and a match list this test
writes, with every kind of entry the reference skips interleaved.  On the CPU
a recording stand-in answers orbx_optimize_sim3, so the arrays the forwarder
hands over and what it does with the answer are checked; on the GPU it links
liborbx and the results equal pyref_sim3 on the same arrays."""
import os
import subprocess
import tempfile
from pathlib import Path

import numpy as np
import pytest

import sim3_cases
from orb_slam_2_ros_amd.synth_sim3 import SIM3_CAM_DTYPE, SIM3_CORR_DTYPE, SIM3_DTYPE

ROOT = Path(__file__).resolve().parents[1]
REC = np.dtype([("match", "<i4"), ("mp1", "<i4"), ("mp2_bad", "<i4"), ("i2", "<i4"), ("X1w", "<f4", (3,)),
                ("X2w", "<f4", (3,)), ("u1", "<f4"), ("v1", "<f4"), ("octave1", "<i4"), ("u2", "<f4"), ("v2", "<f4"),
                ("octave2", "<i4")])
assert REC.itemsize == 64
INV_SIGMA2 = (1.0 / (1.2 ** np.arange(8)) ** 2).astype(np.float32)
IDENTITY = np.eye(4, dtype=np.float32)[:3]
SKIPS = ("no-match", "no-mp1", "bad-mp1", "bad-mp2", "not-in-kf2")


def build(backend):
    out = Path(tempfile.mkdtemp(prefix="orbx_sim3fwd_")) / f"sim3_forwarder_test_{backend}"
    cxx = ROOT / "tests" / "cxx"
    srcs = [ROOT / "integration" / "Optimizer_sim3_orbx.cc", cxx / "sim3_forwarder_test.cpp"]
    lib_dir = ROOT / "orb_slam_2_ros_amd"
    if backend == "record":
        srcs.append(cxx / "orbx_sim3_record_shim.cpp")
        libs = []
    else:
        libs = [f"-L{lib_dir}", "-lorbx", f"-Wl,-rpath,{lib_dir}"]
    inc = [ROOT / "integration", cxx / "sim3_mock", cxx / "orbslam_mock", cxx / "cv_mock", ROOT / "include"]
    subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Wextra", "-Werror", *[f"-I{i}" for i in inc],
                    *[str(s) for s in srcs], *libs, "-o", str(out)], check=True)
    return out


def octave_of(inv_sigma2):
    k = int(np.argmin(np.abs(INV_SIGMA2 - inv_sigma2)))
    assert INV_SIGMA2[k] == inv_sigma2
    return k


def keyframes_of(P, X1w=None, X2w=None, gap_every=3):
    """The problem's correspondences as features of KF1 with their matches,
    an entry the reference skips (each kind of SKIPS in turn) before every
    gap_every-th one and one at the end; KF2's features in a shuffled order.
    X1w, X2w: the map points' world positions (default: the camera points
    themselves, for identity poses).  Returns (records, index of each
    correspondence's feature, number of KF2 features)."""
    K = P["corr"]
    n = len(K)
    X1w = K["P1c"] if X1w is None else X1w
    X2w = K["P2c"] if X2w is None else X2w
    rng = np.random.default_rng(n)
    slots = rng.permutation(2 * n + 8)                   # KF2 feature indices: distinct, not in order
    recs, index, kinds = [], [], 0
    for k in range(n + 1):
        if k % gap_every == 0 or k == n:
            kind = SKIPS[kinds % len(SKIPS)]
            kinds += 1
            recs.append((0 if kind == "no-match" else 1, {"no-mp1": 0, "bad-mp1": 2}.get(kind, 1),
                         1 if kind == "bad-mp2" else 0, -1 if kind == "not-in-kf2" else int(slots[n + kinds % 8]),
                         tuple(rng.normal(0, 1, 3)), tuple(rng.normal(0, 1, 3)), rng.uniform(0, 600),
                         rng.uniform(0, 400), int(rng.integers(8)), rng.uniform(0, 600), rng.uniform(0, 400),
                         int(rng.integers(8))))
        if k < n:
            index.append(len(recs))
            recs.append((1, 1, 0, int(slots[k]), tuple(X1w[k]), tuple(X2w[k]), K["u1"][k], K["v1"][k],
                         octave_of(K["inv_sigma2_1"][k]), K["u2"][k], K["v2"][k], octave_of(K["inv_sigma2_2"][k])))
    return np.array(recs, REC), np.array(index, np.int64), 2 * n + 8


def run(exe, P, recs, n2, T1w=IDENTITY, T2w=IDENTITY, record=False, early=False):
    """(return value, g2oS12 as eight doubles, which matches are still set, record path)"""
    d = Path(tempfile.mkdtemp(prefix="orbx_sim3fwd_io_"))
    with open(d / "in.bin", "wb") as f:
        f.write(np.array([len(recs), n2], np.int32).tobytes())
        f.write(np.float32(P["th2"]).tobytes())
        f.write(np.int32(P["fix_scale"]).tobytes())
        f.write(P["S12"].tobytes())
        f.write(P["cam1"].tobytes())
        f.write(P["cam2"].tobytes())
        f.write(np.ascontiguousarray(T1w, np.float32).tobytes())
        f.write(np.ascontiguousarray(T2w, np.float32).tobytes())
        f.write(INV_SIGMA2.tobytes())
        f.write(recs.tobytes())
    env = dict(os.environ)
    env.pop("ORBX_SIM3_EARLY", None)
    if record:
        env["ORBX_SIM3_RECORD"] = str(d / "record.bin")
    if early:
        env["ORBX_SIM3_EARLY"] = "1"
    r = subprocess.run([str(exe), str(d / "in.bin"), str(d / "out.bin")], capture_output=True, text=True,
                       timeout=120, env=env)
    assert r.returncode == 0, r.stdout + r.stderr
    raw = (d / "out.bin").read_bytes()
    assert len(raw) == 68 + 4 * len(recs)
    ret = int(np.frombuffer(raw, np.int32, 1)[0])
    return ret, np.frombuffer(raw, np.float64, 8, 4), np.frombuffer(raw, np.int32, len(recs), 68).astype(bool), \
        d / "record.bin"


def recorded(path):
    raw = Path(path).read_bytes()
    device, n = (int(v) for v in np.frombuffer(raw, np.int32, 2))
    assert len(raw) == 112 + 48 * n + 12
    return {"device": device, "n": n, "th2": np.frombuffer(raw, np.float32, 1, 8)[0],
            "fix_scale": int(np.frombuffer(raw, np.int32, 1, 12)[0]), "S12": np.frombuffer(raw, SIM3_DTYPE, 1, 16),
            "cam1": np.frombuffer(raw, SIM3_CAM_DTYPE, 1, 80), "cam2": np.frombuffer(raw, SIM3_CAM_DTYPE, 1, 96),
            "corr": np.frombuffer(raw, SIM3_CORR_DTYPE, n, 112), "nulls": np.frombuffer(raw, np.int32, 3, 112 + 48 * n)}


def mock_transform(T, X):
    """R * X + t as the cv stand-in computes it in float: each row's products
    added in order from 0, then the translation"""
    T, X = np.asarray(T, np.float32), np.asarray(X, np.float32)
    out = np.zeros_like(X)
    for r in range(3):
        s = np.zeros(len(X), np.float32)
        for k in range(3):
            s = s + T[r, k] * X[:, k]
        out[:, r] = s + T[r, 3]
    return out


@pytest.fixture(scope="module")
def record_exe():
    return build("record")


def _poses():
    from orb_slam_2_ros_amd.synth_ba import _rot
    T1 = np.hstack([_rot([0.1, -0.2, 0.05]), [[0.3], [-0.1], [0.2]]]).astype(np.float32)
    T2 = np.hstack([_rot([-0.15, 0.1, 0.2]), [[-0.2], [0.4], [0.1]]]).astype(np.float32)
    return T1, T2


@pytest.mark.parametrize("name", [(65, False), (20, True), "one-sided", (9, False), (0, False)],
                         ids=sim3_cases.case_id)
def test_forwarder_hands_over_the_correspondences(name, record_exe):
    """Entries without a match, without a good map point on either side or
    whose matched point is not observed in KF2 are skipped; the others arrive
    in feature order with KF2's keypoint looked up by the matched point's
    index; the points arrive as R * X + t of their own keyframe computed in
    float; both cameras, th2, the scale flag and g2oS12 arrive as they are;
    the chi2 and iteration outputs are not asked for.  Of the answer, every
    removed correspondence's match is nulled (both classifications), the
    skipped entries keep theirs, g2oS12 is the answer's and the return value
    its n_inliers, unless fewer than ten survive the first classification."""
    P = sim3_cases.problem(name)
    n = len(P["corr"])
    T1, T2 = _poses()
    rng = np.random.default_rng(n + 5)
    X1w, X2w = (rng.normal(0, 3, (n, 3)).astype(np.float32) for _ in range(2))
    recs, index, n2 = keyframes_of(P, X1w, X2w)
    ret, S, still, rec_path = run(record_exe, P, recs, n2, T1, T2, record=True)
    R = recorded(rec_path)
    assert R["n"] == n and R["device"] == 0 and list(R["nulls"]) == [1, 1, 1]
    assert R["th2"] == np.float32(P["th2"]) and R["fix_scale"] == int(P["fix_scale"])
    assert R["S12"].tobytes() == P["S12"].tobytes()
    assert R["cam1"].tobytes() == P["cam1"].tobytes() and R["cam2"].tobytes() == P["cam2"].tobytes()
    want = P["corr"].copy()
    want["P1c"], want["P2c"] = mock_transform(T1, X1w), mock_transform(T2, X2w)
    assert R["corr"].tobytes() == want.tobytes()
    skipped = np.ones(len(recs), bool)
    skipped[index] = False
    assert np.array_equal(still[skipped], recs["match"][skipped] != 0)      # untouched, null or not
    assert np.array_equal(still[index], np.arange(n) % 3 == 0)
    nbad = int((np.arange(n) % 3 == 1).sum())
    if n - nbad < 10:
        assert ret == 0 and S.tobytes() == P["S12"].tobytes()
    else:
        q, t, s = P["S12"]["q"][0], P["S12"]["t"][0], P["S12"]["s"][0]
        assert ret == 1000 + n
        assert S.tobytes() == np.concatenate([q, t + [0, 0, 1.0], [2 * s]]).tobytes()


def test_forwarder_early_return_leaves_the_sim3_alone(record_exe):
    """Thirty correspondences of which the answer removes all but nine in the
    first classification: the return value is 0, g2oS12 keeps its bytes (the
    answer's differs), and the removed matches are nulled all the same."""
    P = dict(sim3_cases.problem((65, False)))
    P["corr"] = P["corr"][:30]
    recs, index, n2 = keyframes_of(P)
    ret, S, still, _ = run(record_exe, P, recs, n2, record=True, early=True)
    assert ret == 0 and S.tobytes() == P["S12"].tobytes()
    assert np.array_equal(still[index], np.arange(30) < 9)
    ret, S, _, _ = run(record_exe, P, recs, n2, record=True)
    assert ret == 1030 and S.tobytes() != P["S12"].tobytes()


def test_forwarder_links_against_liborbx():
    assert build("liborbx").exists()


@pytest.mark.gpu
@pytest.mark.parametrize("name", [(65, False), "early-return", (9, False), (0, False)], ids=sim3_cases.case_id)
def test_forwarder_on_the_gpu(name):
    """Identity keyframe poses, so the camera points are the world points and
    the arrays are the case's own"""
    P = sim3_cases.problem(name)
    ref = sim3_cases.reference(name)
    recs, index, n2 = keyframes_of(P)
    ret, S, still, _ = run(build("liborbx"), P, recs, n2)
    assert ret == ref["n_inliers"]
    assert S.tobytes() == ref["S"].tobytes()
    if ref["early"]:
        assert ret == 0 and S.tobytes() == P["S12"].tobytes()
    assert np.array_equal(still[index], ref["removed"] == 0)
    skipped = np.ones(len(recs), bool)
    skipped[index] = False
    assert np.array_equal(still[skipped], recs["match"][skipped] != 0)
