"""integration/Optimizer_pose_orbx.cc, the reference-side
Optimizer::PoseOptimization: compiled against the test stand-ins of the
reference headers (tests/cxx/pose_mock before tests/cxx/orbslam_mock) and run
by tests/cxx/pose_forwarder_test.cpp on a frame this test writes, with
features that have no map point interleaved.  On the CPU a recording stand-in
answers orbx_pose_optimization, so the arrays the forwarder hands over and
what it does with the answer are checked; on the GPU it links liborbx and the
results equal pyref_pose on the same arrays."""
import os
import subprocess
import tempfile
from pathlib import Path

import numpy as np
import pytest

import pose_cases
from orb_slam_2_ros_amd.synth_pose import POSE_CAM_DTYPE, POSE_OBS_DTYPE

ROOT = Path(__file__).resolve().parents[1]
REC = np.dtype([("has_point", "<i4"), ("Xw", "<f4", (3,)), ("u", "<f4"), ("v", "<f4"), ("ur", "<f4"),
                ("octave", "<i4"), ("outlier_before", "<i4")])
INV_SIGMA2 = (1.0 / (1.2 ** np.arange(8)) ** 2).astype(np.float32)


def build(backend):
    out = Path(tempfile.mkdtemp(prefix="orbx_posefwd_")) / f"pose_forwarder_test_{backend}"
    cxx = ROOT / "tests" / "cxx"
    srcs = [ROOT / "integration" / "Optimizer_pose_orbx.cc", cxx / "pose_mock" / "pose_mock_impl.cpp",
            cxx / "pose_forwarder_test.cpp"]
    lib_dir = ROOT / "orb_slam_2_ros_amd"
    if backend == "record":
        srcs.append(cxx / "orbx_pose_record_shim.cpp")
        libs = []
    else:
        libs = [f"-L{lib_dir}", "-lorbx", f"-Wl,-rpath,{lib_dir}"]
    inc = [ROOT / "integration", cxx / "pose_mock", cxx / "orbslam_mock", cxx / "cv_mock", ROOT / "include"]
    subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Wextra", "-Werror", *[f"-I{i}" for i in inc],
                    *[str(s) for s in srcs], *libs, "-o", str(out)], check=True)
    return out


def frame_of(P, gap_every=3):
    """The problem's observations as frame features with a feature without a
    map point (a plausible keypoint, outlier flag set) before every
    gap_every-th one and one at the end.  Returns (records, index of each
    observation's feature)."""
    O = P["obs"]
    recs, index = [], []
    rng = np.random.default_rng(len(O))
    for k in range(len(O) + 1):
        if k % gap_every == 0 or k == len(O):
            recs.append((0, (0, 0, 0), rng.uniform(0, 600), rng.uniform(0, 300), rng.choice([-1.0, 40.0]),
                         int(rng.integers(8)), int(rng.integers(2))))
        if k < len(O):
            octave = int(np.argmin(np.abs(INV_SIGMA2 - O["inv_sigma2"][k])))
            assert INV_SIGMA2[octave] == O["inv_sigma2"][k]
            index.append(len(recs))
            recs.append((1, tuple(O["Xw"][k]), O["u"][k], O["v"][k], O["ur"][k], octave, 1))
    return np.array(recs, REC), np.array(index, np.int64)


def run(exe, P, recs, record=False):
    """(return value, SetPose ran, mTcw rows, mvbOutlier, record path)"""
    d = Path(tempfile.mkdtemp(prefix="orbx_posefwd_io_"))
    with open(d / "in.bin", "wb") as f:
        f.write(np.int32(len(recs)).tobytes())
        f.write(np.ascontiguousarray(P["Tcw"], np.float32).tobytes())
        f.write(P["cam"].tobytes())
        f.write(INV_SIGMA2.tobytes())
        f.write(recs.tobytes())
    env = {**os.environ, "ORBX_POSE_RECORD": str(d / "record.bin")} if record else dict(os.environ)
    r = subprocess.run([str(exe), str(d / "in.bin"), str(d / "out.bin")], capture_output=True, text=True,
                       timeout=120, env=env)
    assert r.returncode == 0, r.stdout + r.stderr
    raw = (d / "out.bin").read_bytes()
    assert len(raw) == 56 + 4 * len(recs)
    ret, set_pose = np.frombuffer(raw, np.int32, 2)
    Tcw = np.frombuffer(raw, np.float32, 12, 8).reshape(3, 4)
    out = np.frombuffer(raw, np.int32, len(recs), 56)
    return int(ret), bool(set_pose), Tcw, out.astype(bool), d / "record.bin"


def recorded(path):
    raw = Path(path).read_bytes()
    device, n = (int(v) for v in np.frombuffer(raw, np.int32, 2))
    assert len(raw) == 76 + 28 * n + 8
    return {"device": device, "n": n, "Tcw": np.frombuffer(raw, np.float32, 12, 8).reshape(3, 4),
            "cam": np.frombuffer(raw, POSE_CAM_DTYPE, 1, 56), "obs": np.frombuffer(raw, POSE_OBS_DTYPE, n, 76),
            "nulls": np.frombuffer(raw, np.int32, 2, 76 + 28 * n)}


@pytest.fixture(scope="module")
def record_exe():
    return build("record")


@pytest.mark.parametrize("name", [(10, "mixed"), (65, "mixed"), "ur-edges", (3, "stereo"), (2, "mono"), (0, "mixed")],
                         ids=pose_cases.case_id)
def test_forwarder_hands_over_the_observations(name, record_exe):
    """Null points are skipped, feature order is kept, ur passes through (the
    mono / stereo rule is ur < 0, so ur = 0 stays a stereo observation), the
    pose and intrinsics arrive as they are; the answer's flags land on the
    observations' features, the others keep theirs, and for n < 3 neither
    SetPose nor the flags of the answer are applied and the return is 0."""
    P = pose_cases.problem(name)
    recs, index = frame_of(P)
    n = len(P["obs"])
    ret, set_pose, Tcw, out, rec_path = run(record_exe, P, recs, record=True)
    R = recorded(rec_path)
    assert R["n"] == n and R["device"] == 0 and list(R["nulls"]) == [1, 1]
    assert R["Tcw"].tobytes() == P["Tcw"].tobytes() and R["cam"].tobytes() == P["cam"].tobytes()
    assert R["obs"].tobytes() == P["obs"].tobytes()
    if name == "ur-edges":
        assert R["obs"]["ur"][3] == 0.0 and R["obs"]["ur"][4] == -1.0
    nomp = recs["has_point"] == 0
    assert np.array_equal(out[nomp], recs["outlier_before"][nomp] != 0)
    if n < 3:
        assert ret == 0 and not set_pose and Tcw.tobytes() == P["Tcw"].tobytes()
        assert not out[index].any()               # cleared during the collection, as the reference does
    else:
        want = P["Tcw"].copy()
        want[2, 3] += 1.0
        assert ret == 1000 + n and set_pose and Tcw.tobytes() == want.tobytes()
        assert np.array_equal(out[index], np.arange(n) % 2 == 1)


def test_forwarder_links_against_liborbx():
    assert build("liborbx").exists()


@pytest.mark.gpu
@pytest.mark.parametrize("name", [(65, "mixed"), "behind", (9, "mixed"), (2, "mono")], ids=pose_cases.case_id)
def test_forwarder_on_the_gpu(name):
    P = pose_cases.problem(name)
    ref = pose_cases.reference(name)
    recs, index = frame_of(P)
    ret, set_pose, Tcw, out, _ = run(build("liborbx"), P, recs)
    n = len(P["obs"])
    assert ret == ref["n_inliers"] and set_pose == (n >= 3)
    assert Tcw.tobytes() == ref["Tcw"].tobytes()
    assert np.array_equal(out[index], ref["outlier"])
    nomp = recs["has_point"] == 0
    assert np.array_equal(out[nomp], recs["outlier_before"][nomp] != 0)
