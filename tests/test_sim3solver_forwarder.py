"""integration/Sim3Solver_orbx.cc, the reference-side Sim3Solver: compiled
against the test stand-ins of the reference headers
(tests/cxx/sim3solver_mock before tests/cxx/orbslam_mock) and run by
tests/cxx/sim3solver_forwarder_test.cpp, LoopClosing::ComputeSim3's solver
loop, on keyframe pairs and match lists this test writes, with every kind of
entry the constructor skips interleaved.  On the CPU a recording stand-in
answers orbx_sim3_ransac_batch, so the arrays the forwarder hands over and
what it does with the answer are checked; on the GPU it links liborbx and the
inlier flags, the returned T12 and the getters equal pyref_sim3solver's on
the same arrays and triples."""
import os
import subprocess
import tempfile
from pathlib import Path

import numpy as np
import pytest

import pyref_sim3solver as ref
import sim3solver_cases as cases
from orb_slam_2_ros_amd.sim3solver import RANSAC_CORR_DTYPE, draw_triples, max_error
from orb_slam_2_ros_amd.synth_sim3 import SIM3_CAM_DTYPE

ROOT = Path(__file__).resolve().parents[1]
REC = np.dtype([("match", "<i4"), ("mp1", "<i4"), ("mp2_bad", "<i4"), ("i1", "<i4"), ("i2", "<i4"),
                ("X1w", "<f4", (3,)), ("X2w", "<f4", (3,)), ("octave1", "<i4"), ("octave2", "<i4")])
assert REC.itemsize == 52
SIGMA2 = ((1.2 ** np.arange(8)).astype(np.float32) ** 2).astype(np.float32)
IDENTITY = np.eye(4, dtype=np.float32)[:3]
SKIPS = ("no-match", "no-mp1", "bad-mp1", "bad-mp2", "not-in-kf1", "not-in-kf2")
MIN_INLIERS = 20


def build(backend):
    out = Path(tempfile.mkdtemp(prefix="orbx_s3sfwd_")) / f"sim3solver_forwarder_test_{backend}"
    cxx = ROOT / "tests" / "cxx"
    srcs = [ROOT / "integration" / "Sim3Solver_orbx.cc", cxx / "sim3solver_forwarder_test.cpp"]
    lib_dir = ROOT / "orb_slam_2_ros_amd"
    if backend == "record":
        srcs.append(cxx / "orbx_sim3solver_record_shim.cpp")
        libs = []
    else:
        libs = [f"-L{lib_dir}", "-lorbx", f"-Wl,-rpath,{lib_dir}"]
    inc = [ROOT / "integration", cxx / "sim3solver_mock", cxx / "orbslam_mock", cxx / "cv_mock", ROOT / "include"]
    subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Wextra", "-Werror", *[f"-I{i}" for i in inc],
                    *[str(s) for s in srcs], *libs, "-o", str(out)], check=True)
    return out


def candidate(corr, octaves, fix, X1w=None, X2w=None, T1w=IDENTITY, T2w=IDENTITY, cam1=None, cam2=None, gap_every=3):
    """The correspondences as features of KF1 with their matches, an entry the
    constructor skips (each kind of SKIPS in turn) before every gap_every-th
    one and one at the end; both keyframes' feature indices shuffled.  Returns
    dict with the records and the index (mvnIndices1) of each correspondence."""
    n = len(corr)
    X1w = corr["X1c"] if X1w is None else X1w
    X2w = corr["X2c"] if X2w is None else X2w
    rng = np.random.default_rng(n)
    s1, s2 = rng.permutation(2 * n + 8), rng.permutation(2 * n + 8)
    recs, index, kinds = [], [], 0
    for k in range(n + 1):
        if k % gap_every == 0 or k == n:
            kind = SKIPS[kinds % len(SKIPS)]
            kinds += 1
            recs.append((0 if kind == "no-match" else 1, {"no-mp1": 0, "bad-mp1": 2}.get(kind, 1),
                         1 if kind == "bad-mp2" else 0, -1 if kind == "not-in-kf1" else int(s1[n + kinds % 8]),
                         -1 if kind == "not-in-kf2" else int(s2[n + kinds % 8]), tuple(rng.normal(0, 1, 3)),
                         tuple(rng.normal(0, 1, 3)), int(rng.integers(8)), int(rng.integers(8))))
        if k < n:
            index.append(len(recs))
            recs.append((1, 1, 0, int(s1[k]), int(s2[k]), tuple(X1w[k]), tuple(X2w[k]), int(octaves[0][k]),
                         int(octaves[1][k])))
    return {"recs": np.array(recs, REC), "index": np.array(index, np.int64), "nkeys": 2 * n + 8, "fix": int(fix),
            "T1w": np.ascontiguousarray(T1w, np.float32), "T2w": np.ascontiguousarray(T2w, np.float32),
            "cam1": cam1, "cam2": cam2}


def run(exe, cands, prepare=True, record=False):
    d = Path(tempfile.mkdtemp(prefix="orbx_s3sfwd_io_"))
    with open(d / "in.bin", "wb") as f:
        f.write(np.array([len(cands), int(prepare)], np.int32).tobytes())
        f.write(SIGMA2.tobytes())
        for c in cands:
            f.write(np.array([len(c["recs"]), c["nkeys"], c["nkeys"], c["fix"]], np.int32).tobytes())
            f.write(c["cam1"].tobytes() + c["cam2"].tobytes() + c["T1w"].tobytes() + c["T2w"].tobytes())
            f.write(c["recs"].tobytes())
    env = dict(os.environ)
    if record:
        env["ORBX_RANSAC_RECORD"] = str(d / "record.bin")
    r = subprocess.run([str(exe), str(d / "in.bin"), str(d / "out.bin")], capture_output=True, text=True, timeout=120,
                       env=env)
    assert r.returncode == 0, r.stdout + r.stderr
    raw = (d / "out.bin").read_bytes()
    calls_after_prepare = int(np.frombuffer(raw, np.int32, 1)[0])
    pos, events = 4, []
    while True:
        s = int(np.frombuffer(raw, np.int32, 1, pos)[0])
        if s < 0:
            break
        _, returned, no_more, n_inl = (int(v) for v in np.frombuffer(raw, np.int32, 4, pos))
        pos += 16
        m = len(cands[s]["recs"])
        ev = {"solver": s, "returned": bool(returned), "no_more": bool(no_more), "n_inliers": n_inl,
              "inliers": np.frombuffer(raw, np.uint8, m, pos).astype(bool)}
        pos += m
        if returned:
            fl = np.frombuffer(raw, np.float32, 29, pos)
            pos += 116
            ev.update(T12=fl[:16].reshape(4, 4), R=fl[16:25], t=fl[25:28], s=fl[28])
        events.append(ev)
    calls = int(np.frombuffer(raw, np.int32, 1, pos + 4)[0])
    assert pos + 8 == len(raw)
    return calls_after_prepare, events, calls, d / "record.bin"


def recorded(path):
    """The record shim's calls: a list of lists of problems"""
    raw = Path(path).read_bytes() if Path(path).exists() else b""
    pos, calls = 0, []
    while pos < len(raw):
        device, P = (int(v) for v in np.frombuffer(raw, np.int32, 2, pos))
        pos += 8
        probs = []
        for _ in range(P):
            cam1, cam2 = np.frombuffer(raw, SIM3_CAM_DTYPE, 2, pos)
            fix, n, h = (int(v) for v in np.frombuffer(raw, np.int32, 3, pos + 32))
            pos += 44
            corr = np.frombuffer(raw, RANSAC_CORR_DTYPE, n, pos)
            pos += 32 * n
            tri = np.frombuffer(raw, np.int32, 3 * h, pos).reshape(h, 3)
            pos += 12 * h
            probs.append({"device": device, "cam1": cam1, "cam2": cam2, "fix": fix, "corr": corr, "triples": tri})
        calls.append(probs)
    return calls


class Lcg:
    """tests/cxx/sim3solver_mock's DUtils::Random::RandomInt"""

    def __init__(self):
        self.x, self.calls = 12345, 0

    def __call__(self, lo, hi):
        self.x = (1103515245 * self.x + 12345) & 0x7fffffff
        self.calls += 1
        return lo + self.x % (hi - lo + 1)


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


def expected_triples(ns, rng):
    """Each solver's triples in list order: all of its mRansacMaxIts, none below the minimum"""
    out = []
    for n in ns:
        its = ref.ransac_iterations(n, 0.99, MIN_INLIERS, 300)
        out.append(draw_triples(n, its, rng) if n >= MIN_INLIERS else np.zeros((0, 3), np.int32))
    return out


def expected_events(cands, ns, hyps, masks):
    """The driver's loop over ref.Walk: iterate(5) round robin, the last solver's first call find()"""
    walks = [ref.Walk(n, len(c["recs"]), c["index"], hyps[s], masks[s], MIN_INLIERS,
                      ref.ransac_iterations(n, 0.99, MIN_INLIERS, 300)) for s, (c, n) in enumerate(zip(cands, ns))]
    alive, first, out = [True] * len(cands), [True] * len(cands), []
    while any(alive):
        for s, w in enumerate(walks):
            if not alive[s]:
                continue
            if s == len(cands) - 1 and first[s]:
                k, vb, ni = w.find()
                nm = False
            else:
                k, nm, vb, ni = w.iterate(5)
            first[s] = False
            out.append({"solver": s, "k": k, "no_more": nm, "n_inliers": ni, "inliers": np.array(vb, bool),
                        "best": w.best})
            alive[s] = not nm
    return out


def assert_events(events, want, hyps):
    assert [e["solver"] for e in events] == [e["solver"] for e in want]
    for e, w in zip(events, want):
        assert e["returned"] == (w["k"] is not None) and e["no_more"] == w["no_more"], (e["solver"], w)
        assert e["n_inliers"] == w["n_inliers"] and np.array_equal(e["inliers"], w["inliers"]), (e["solver"], w["k"])
        if w["k"] is not None:
            h = hyps[e["solver"]][w["k"]]
            T = np.eye(4, dtype=np.float32)
            T[:3, :3] = h["s"] * h["R"].reshape(3, 3)
            T[:3, 3] = h["t"]
            assert e["T12"].tobytes() == T.tobytes(), (e["solver"], w["k"])
            assert w["best"] == w["k"]
            assert e["R"].tobytes() == h["R"].tobytes() and e["t"].tobytes() == h["t"].tobytes() and e["s"] == h["s"]


@pytest.fixture(scope="module")
def record_exe():
    return build("record")


def _poses():
    from orb_slam_2_ros_amd.synth_ba import _rot
    T1 = np.hstack([_rot([0.1, -0.2, 0.05]), [[0.3], [-0.1], [0.2]]]).astype(np.float32)
    T2 = np.hstack([_rot([-0.15, 0.1, 0.2]), [[-0.2], [0.4], [0.1]]]).astype(np.float32)
    return T1, T2


def _record_candidates():
    T1, T2 = _poses()
    out = []
    for s, name in enumerate([(65, False), (20, True), (3, False), "z0"]):   # (3 accepted: below the minimum)
        P = cases.problem(name)
        n = len(P["corr"])
        rng = np.random.default_rng(n + 5)
        X1w, X2w = (rng.normal(0, 3, (n, 3)).astype(np.float32) for _ in range(2))
        c = candidate(P["corr"], P["octaves"], s % 2, X1w, X2w, T1, T2, P["cam1"], P["cam2"], gap_every=2 + s)
        c["want"] = P["corr"].copy()
        c["want"]["X1c"], c["want"]["X2c"] = mock_transform(T1, X1w), mock_transform(T2, X2w)
        out.append(c)
    return out


def _shim_answer(p, n, h):
    """What tests/cxx/orbx_sim3solver_record_shim.cpp answers for problem p of a call"""
    hyp = np.zeros(h, ref.HYP_DTYPE)
    mask = np.zeros((h, (n + 63) // 64), np.uint64)
    for k in range(h):
        hyp["R"][k] = [np.float32(100 * p + k) + np.float32(j / 16) for j in range(9)]
        hyp["t"][k] = [-(np.float32(k) + np.float32(j / 4)) for j in range(3)]
        hyp["s"][k] = 2 + k
        inl = np.arange(n) < 3
        if k == 7 + p:
            inl = np.arange(n) != p
        if k == 11 + p:
            inl = np.ones(n, bool)
        if k == 12 + p:
            inl = np.arange(n) >= 2
        hyp["n_inliers"][k] = inl.sum()
        mask[k] = ref.mask_words(inl)
    return hyp, mask


@pytest.mark.parametrize("prepare", [True, False], ids=["prepared", "lazy"])
def test_forwarder_hands_over_and_walks(prepare, record_exe):
    """Entries without a match, without a good map point on either side or
    whose points are not observed in their keyframes are skipped; the others
    arrive in feature order as R * X + t of their own keyframe computed in
    float, with the thresholds truncated to integers; the triples are distinct,
    all mRansacMaxIts of a solver, drawn from RandomInt in list order with the
    swap-with-last removal; prepared, the solvers (the null entry skipped) are
    one call, the one below the minimum with no hypotheses; lazy, each is its
    own call on its first iterate, and the one below the minimum none at all.
    Of the answer: vbInliers goes through mvnIndices1, T12 is [sR | t], the
    getters are the best hypothesis's, and the walk is the restatement's."""
    cands = _record_candidates()
    ns = [len(c["want"]) for c in cands]
    calls_after_prepare, events, calls, rec_path = run(record_exe, cands, prepare, record=True)
    R = recorded(rec_path)
    lcg = Lcg()
    triples = expected_triples(ns, lcg)
    if prepare:
        assert len(R) == 1 and len(R[0]) == 3
        probs = [R[0][0], R[0][1], None, R[0][2]]
        assert calls_after_prepare == lcg.calls == 3 * sum(len(t) for t in triples)
        slot = [0, 1, None, 2]
    else:
        # round robin: solver 0 iterates first, then 1; solver 2 is below the minimum; solver 3's first call is find()
        assert calls_after_prepare == 0 and [len(c) for c in R] == [1, 1, 1]
        probs = [R[0][0], R[1][0], None, R[2][0]]
        slot = [0, 0, None, 0]
    assert calls == lcg.calls
    hyps, masks = [], []
    for s, c in enumerate(cands):
        p = probs[s]
        if p is None:
            hyps.append(np.zeros(0, ref.HYP_DTYPE))
            masks.append(np.zeros((0, 1), np.uint64))
            continue
        assert p["device"] == 0 and p["fix"] == c["fix"]
        assert p["cam1"].tobytes() == c["cam1"].tobytes() and p["cam2"].tobytes() == c["cam2"].tobytes()
        assert p["corr"].tobytes() == c["want"].tobytes()
        assert np.array_equal(p["corr"]["max_err1"], np.floor(p["corr"]["max_err1"]))
        assert set(np.unique(p["corr"]["max_err1"])) <= {max_error(s2) for s2 in SIGMA2}
        assert np.array_equal(p["triples"], triples[s])
        t = p["triples"]
        assert len(t) == 0 or ((t[:, 0] != t[:, 1]) & (t[:, 0] != t[:, 2]) & (t[:, 1] != t[:, 2])).all()
        h, m = _shim_answer(slot[s], ns[s], len(t))
        hyps.append(h)
        masks.append(m)
    want = expected_events(cands, ns, hyps, masks)
    assert_events(events, want, hyps)
    # what the answers were built to reach: a result, a later and larger one, and one above the minimum below the best
    for s in (0, 3):
        got = [w["k"] for w in want if w["solver"] == s and w["k"] is not None]
        assert got == [7 + slot[s], 11 + slot[s]]
    assert [w["k"] for w in want if w["solver"] == 1] == [None]              # N == minInliers: one iteration
    assert [w["no_more"] for w in want if w["solver"] == 2] == [True]        # N < minInliers


def test_forwarder_links_against_liborbx():
    assert build("liborbx").exists()


@pytest.mark.gpu
def test_forwarder_on_the_gpu():
    """Three solvers prepared in one launch, identity keyframe poses, so the
    camera points are the world points and the arrays are the cases' own; the
    triples are the stand-in RandomInt's, replayed here."""
    names = [(65, False), "recovery", (130, True)]
    Ps = [cases.problem(nm) for nm in names]
    cands = [candidate(P["corr"], P["octaves"], P["fix_scale"], cam1=P["cam1"], cam2=P["cam2"]) for P in Ps]
    ns = [len(P["corr"]) for P in Ps]
    lcg = Lcg()
    triples = expected_triples(ns, lcg)
    hyps, masks = [], []
    for P, T in zip(Ps, triples):
        h, m = ref.ransac(P["cam1"], P["cam2"], P["fix_scale"], P["corr"], T)
        hyps.append(h)
        masks.append(m)
    calls_after_prepare, events, calls, _ = run(build("liborbx"), cands)
    assert calls_after_prepare == calls == lcg.calls
    want = expected_events(cands, ns, hyps, masks)
    assert sum(w["k"] is not None for w in want) >= 3
    assert_events(events, want, hyps)
