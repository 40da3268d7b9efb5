"""integration/LocalMapping_triangulate_orbx.cc, the reference-side
OrbxTriangulateBatch: compiled against the test stand-ins of the reference
headers (tests/cxx/orbslam_mock) and run by
tests/cxx/triangulate_forwarder_test.cpp on a current keyframe, neighbours and
pair lists this test writes.  On the CPU a recording stand-in answers
orbx_triangulate_batch, so the arrays the forwarder hands over and what it
does with the answer are checked; on the GPU it links liborbx and the points
equal pyref_triangulate's on the same arrays."""
import os
import subprocess
import tempfile
from pathlib import Path

import numpy as np
import pytest

import pyref_triangulate as ref
import triangulate_cases as cases
from orb_slam_2_ros_amd.synth_ba import _rot
from orb_slam_2_ros_amd.synth_triangulate import make_triangulation_problem

ROOT = Path(__file__).resolve().parents[1]
LEVELS = 8
FEAT = np.dtype([("u", "<f4"), ("v", "<f4"), ("raw_u", "<f4"), ("raw_v", "<f4"), ("ur", "<f4"), ("depth", "<f4"),
                 ("octave", "<i4")])
assert FEAT.itemsize == 28


def build(backend):
    out = Path(tempfile.mkdtemp(prefix="orbx_trifwd_")) / f"triangulate_forwarder_test_{backend}"
    cxx = ROOT / "tests" / "cxx"
    srcs = [ROOT / "integration" / "LocalMapping_triangulate_orbx.cc", cxx / "triangulate_forwarder_test.cpp"]
    lib_dir = ROOT / "orb_slam_2_ros_amd"
    if backend == "record":
        srcs.append(cxx / "orbx_triangulate_record_shim.cpp")
        libs = []
    else:
        libs = [f"-L{lib_dir}", "-lorbx", f"-Wl,-rpath,{lib_dir}"]
    inc = [ROOT / "integration", cxx / "orbslam_mock", cxx / "cv_mock", ROOT / "include"]
    subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Wextra", "-Werror", *[f"-I{i}" for i in inc],
                    *[str(s) for s in srcs], *libs, "-o", str(out)], check=True)
    return out


def tables(factor):
    """a keyframe's mvScaleFactors and mvLevelSigma2 for its own scale factor"""
    s = np.ones(LEVELS, np.float32)
    for i in range(1, LEVELS):
        s[i] = s[i - 1] * np.float32(factor)
    return s, (s * s).astype(np.float32)


def make_map(sizes, stereo, seed=0):
    """A current keyframe and len(sizes) neighbours: neighbour i has sizes[i]
    pairs (0: an empty list) and stereo[i] of its observations with a right
    coordinate; keyframe k's scale factor is 1.2 + k / 50, so a look-up in the
    wrong keyframe's table shows.  Every keyframe has more features than pairs,
    in shuffled order.  Returns (keyframes, pair lists, the expected
    orbx_triangulate_batch arguments)."""
    rng = np.random.default_rng(seed)
    pose1 = (_rot(np.array([0.05, -0.1, 0.02])), np.array([0.1, -0.2, 0.05]))
    Ps = [make_triangulation_problem(max(n, 1), seed=700 + i, stereo_frac=stereo[i], outlier_frac=0.15, pose1=pose1,
                                     mbf2=40.0 + 5 * i) for i, n in enumerate(sizes)]
    n1 = sum(sizes) + 9

    def keyframe(view, factor, N):
        feats = np.zeros(N, FEAT)   # the features no pair uses: recognisably wrong values
        feats["u"], feats["v"], feats["raw_u"], feats["raw_v"] = -1e3, -2e3, -3e3, -4e3
        feats["ur"], feats["depth"], feats["octave"] = -1, -1, rng.integers(0, LEVELS, N)
        return {"view": view, "factor": np.float32(factor), "tables": tables(factor), "feats": feats}

    def put(kf, idx, o, octave):
        f = kf["feats"]
        f["u"][idx], f["v"][idx], f["raw_u"][idx], f["raw_v"][idx] = o["u"], o["v"], o["raw_u"], o["raw_v"]
        f["ur"][idx], f["depth"][idx], f["octave"][idx] = o["ur"], o["depth"], octave

    kfs = [keyframe(Ps[0]["v1"], 1.2, n1)]
    slots1 = list(rng.permutation(n1))
    pair_lists, want_pairs = [], []
    for i, (n, P) in enumerate(zip(sizes, Ps)):
        kf2 = keyframe(P["v2"], 1.2 + (i + 1) / 50, n + 5)
        slots2 = rng.permutation(n + 5)
        pl, K = [], np.zeros(n, ref.PAIR_DTYPE)
        for k in range(n):
            idx1, idx2 = int(slots1.pop()), int(slots2[k])
            put(kfs[0], idx1, P["pairs"]["o1"][k], P["octaves"][0][k])
            put(kf2, idx2, P["pairs"]["o2"][k], P["octaves"][1][k])
            pl.append((idx1, idx2))
            K[k] = P["pairs"][k]
            K["o1"]["scale"][k], K["o1"]["sigma2"][k] = (t[P["octaves"][0][k]] for t in kfs[0]["tables"])
            K["o2"]["scale"][k], K["o2"]["sigma2"][k] = (t[P["octaves"][1][k]] for t in kf2["tables"])
        kfs.append(kf2)
        pair_lists.append(pl)
        want_pairs.append(K)
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
    want = (np.concatenate([Ps[0]["v1"]] * len(sizes)), np.concatenate([P["v2"] for P in Ps]),
            np.full(len(sizes), np.float32(1.5) * np.float32(1.2), np.float32), np.concatenate(want_pairs), off)
    return kfs, pair_lists, want


def run(exe, kfs, pair_lists, record=False):
    d = Path(tempfile.mkdtemp(prefix="orbx_trifwd_io_"))
    with open(d / "in.bin", "wb") as f:
        f.write(np.array([len(pair_lists), LEVELS], np.int32).tobytes())
        for kf in kfs:
            v = kf["view"][0]
            f.write(np.array([len(kf["feats"])], np.int32).tobytes())
            f.write(v["Tcw"].tobytes() + v["Ow"].tobytes())
            f.write(np.array([v[k] for k in ("fx", "fy", "cx", "cy", "invfx", "invfy", "mbf", "mb")] + [kf["factor"]],
                             np.float32).tobytes())
            f.write(kf["tables"][0].tobytes() + kf["tables"][1].tobytes())
            f.write(kf["feats"].tobytes())
        for pl in pair_lists:
            f.write(np.array([len(pl)], np.int32).tobytes())
            f.write(np.array(pl, np.int32).reshape(-1, 2).tobytes())
    env = dict(os.environ)
    if record:
        env["ORBX_TRI_RECORD"] = str(d / "record.bin")
    r = subprocess.run([str(exe), str(d / "in.bin"), str(d / "out.bin")], capture_output=True, text=True, timeout=120,
                       env=env)
    assert r.returncode == 0, r.stdout + r.stderr
    raw = (d / "out.bin").read_bytes()
    nk, pos, out = int(np.frombuffer(raw, np.int32, 1)[0]), 4, []
    for _ in range(nk):
        c = int(np.frombuffer(raw, np.int32, 1, pos)[0])
        out.append(np.frombuffer(raw, ref.POINT_DTYPE, c, pos + 4))
        pos += 4 + 16 * c
    assert pos == len(raw)
    return out, d / "record.bin"


def recorded(path):
    """The record shim's calls: [(device, v1, v2, ratio_factor, offsets, pairs)]"""
    raw = Path(path).read_bytes() if Path(path).exists() else b""
    pos, calls = 0, []
    while pos < len(raw):
        device, P = (int(v) for v in np.frombuffer(raw, np.int32, 2, pos))
        pos += 8
        v1 = np.frombuffer(raw, ref.VIEW_DTYPE, P, pos)
        v2 = np.frombuffer(raw, ref.VIEW_DTYPE, P, pos + 96 * P)
        pos += 192 * P
        rf = np.frombuffer(raw, np.float32, P, pos)
        off = np.frombuffer(raw, np.int32, P + 1, pos + 4 * P)
        pos += 8 * P + 4
        K = np.frombuffer(raw, ref.PAIR_DTYPE, int(off[-1]), pos)
        pos += 64 * int(off[-1])
        calls.append((device, v1, v2, rf, off, K))
    return calls


def test_forwarder_hands_over_and_returns():
    """One call for all neighbours, the empty one included; the current
    keyframe's view repeated, each neighbour's own; pairs in list order with
    mvKeysUn in u, v and mvKeys in raw_u, raw_v, mvuRight and mvDepth, and each
    observation's sigma2 and scale from its own keyframe's tables at its own
    octave; ratio_factor 1.5f * the current keyframe's mfScaleFactor; the
    answer split back per neighbour, in order."""
    sizes = [12, 0, 7, 5]
    kfs, pair_lists, want = make_map(sizes, [0.0, 0.0, 1.0, 0.5])
    out, rec = run(build("record"), kfs, pair_lists, record=True)
    calls = recorded(rec)
    assert len(calls) == 1
    device, v1, v2, rf, off, K = calls[0]
    assert device == 0 and list(off) == [0, 12, 12, 19, 24]
    assert v1.tobytes() == want[0].tobytes() and v2.tobytes() == want[1].tobytes()
    assert len({v.tobytes() for v in v2}) == 4 and len({v.tobytes() for v in v1}) == 1
    assert rf.tobytes() == want[2].tobytes() and rf[0] == np.float32(1.5) * np.float32(1.2)
    assert K.tobytes() == want[3].tobytes()
    assert np.any(K["o1"]["u"] != K["o1"]["raw_u"]) and np.any(K["o2"]["ur"] >= 0) and np.any(K["o2"]["ur"] < 0)
    # the tables differ between keyframes, so these values can only come from the right one
    assert set(np.unique(K["o2"]["scale"][12:19])) <= set(kfs[3]["tables"][0])
    others = set(np.unique(K["o2"]["scale"][12:19])) - {np.float32(1)}
    assert others and not others & set(kfs[0]["tables"][0])
    assert [len(o) for o in out] == sizes
    for p, o in enumerate(out):
        assert list(o["status"]) == [(p + i) % 9 for i in range(len(o))]
        assert o["X"].tolist() == [[p, i, 0.5] for i in range(len(o))]


def test_forwarder_without_neighbours_makes_no_call():
    kfs, _, _ = make_map([3], [0.0])
    out, rec = run(build("record"), kfs[:1], [], record=True)
    assert out == [] and recorded(rec) == []


def test_forwarder_links_against_liborbx():
    assert build("liborbx").exists()


@pytest.mark.gpu
def test_forwarder_on_the_gpu():
    """Three neighbours of about 40 pairs, a mono, a stereo and a mixed one:
    the points equal pyref_triangulate's on the arrays the forwarder is to
    build, and some are created, some rejected"""
    sizes = [40, 37, 43]
    kfs, pair_lists, want = make_map(sizes, [0.0, 1.0, 0.5], seed=1)
    out, _ = run(build("liborbx"), kfs, pair_lists)
    pts = ref.triangulate_batch(*want)
    assert [len(o) for o in out] == sizes
    cases.assert_same(np.concatenate(out), pts)
    assert (pts["status"] == 0).sum() > 60 and (pts["status"] != 0).sum() > 5
