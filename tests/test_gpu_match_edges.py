"""The constructed matcher cases (match_cases.py) through the kernels, equal
to the oracle bit for bit: nmatches, per-query index and distance, final
keypoint ownership, both SearchByBoW directions, vbPrevMatched.
test_match_cases.py shows on the CPU that each case reaches the comparison or
capacity it is named for; the replay's capacity paths are asserted here too,
from the device's own counters (orbx_debug_counter "proj_*").

Each projection and vocabulary case runs through the single call and again
through the batch entry, in one batch that mixes every case of the variant
(and an empty problem).  orbx_mono_step_device extracts its own keypoints from
images, so it cannot carry constructed keypoints and is not run here.
"""
import numpy as np
import pytest

import match_cases as mc
from orb_slam_2_ros_amd import Frame, ORBmatcher
from orb_slam_2_ros_amd._lib import debug_counter

pytestmark = pytest.mark.gpu

CASES = mc.all_cases()
PROJ = [n for n, c in CASES.items() if c["family"] == "proj"]
BOW = [n for n, c in CASES.items() if c["family"] == "bow"]
INIT = [n for n, c in CASES.items() if c["family"] == "init"]
_ORACLE = {}


def oracle_result(c, oracle):
    """The oracle's answer, computed once per case and left unchanged."""
    if c["name"] not in _ORACLE:
        if c["family"] == "proj":
            r = oracle.search_by_projection(c["variant"], c["keys"], c["desc"], c["queries"], c["qdesc"], c["bounds"],
                                            c["uright"], c["mp_state"], c["inv_sigma2"], c["th_dist"], c["nnratio"],
                                            c["check_ori"])
        elif c["family"] == "bow":
            r = oracle.search_by_bow(c["variant"], c["A"], c["B"], c["nnratio"], c["check_ori"], c["tri"])
        elif c["family"] == "sim3":
            k1, k2 = c["kf1"], c["kf2"]
            r = oracle.search_by_sim3(k1["keys"], k1["desc"], k1["bounds"], k2["keys"], k2["desc"], k2["bounds"],
                                      c["q1"], c["qd1"], c["q2"], c["qd2"], c["th_dist"])
        else:
            r = oracle.search_for_initialization(c["k1"], c["d1"], c["k2"], c["d2"], mc.W, mc.H, c["prev"],
                                                 c["window"], c["nnratio"], c["check_ori"], bounds=c["bounds"])
        for a in r[1:]:
            a.setflags(write=False)
        _ORACLE[c["name"]] = r
    return _ORACLE[c["name"]]


def same(name, fields, got, want):
    for f, x, y in zip(fields, got, want):
        x, y = np.atleast_1d(x), np.atleast_1d(y)
        bad = np.nonzero(x != y)[0]
        assert len(bad) == 0, f"{name}: {f} differs at {bad[:6]}: gpu {x[bad[:6]]} vs oracle {y[bad[:6]]}"


PROJ_FIELDS = ("nmatches", "q_idx", "q_dist", "kp_final")
BOW_FIELDS = ("nmatches", "match_a", "match_b")


def proj_args(c):
    return dict(keys=c["keys"], desc=c["desc"], queries=c["queries"], qdesc=c["qdesc"], bounds=c["bounds"],
                uright=c["uright"], mp_state=c["mp_state"], inv_sigma2=c["inv_sigma2"])


@pytest.mark.parametrize("name", PROJ)
def test_projection_case(name, oracle_mod):
    c = CASES[name]
    g = ORBmatcher(c["nnratio"], c["check_ori"]).search_by_projection(c["variant"], th_dist=c["th_dist"],
                                                                      **proj_args(c))
    ctr = {k: debug_counter("proj_" + k) for k in ("hard", "pool_used", "rounds", "in_order", "full_list")}
    same(name, PROJ_FIELDS, g, oracle_result(c, oracle_mod))
    print(name, ctr)
    nq = len(c["queries"])
    base = name.rsplit("-", 1)[0]
    if base == "overflow":            # more claims than the `hard` list holds: everything in query order
        assert ctr["hard"] > 4 * nq + 4096 and ctr["rounds"] == 0 and ctr["in_order"] == nq, ctr
    elif base == "chain":             # one decision a round: the rounds run out
        assert ctr["rounds"] == 64 and ctr["in_order"] > 0, ctr
    elif base == "queue":             # more full-list queries in a round than its queue holds (512): each is
        # scanned once, 512 in the first round and the rest in the second
        assert ctr["full_list"] > 512 and ctr["full_list"] == nq and ctr["rounds"] == 2 and ctr["in_order"] == 0, ctr
    elif base in ("entries3", "entries4"):   # all possible takes among the 4 kept entries
        assert ctr["hard"] == 0, ctr
    elif base == "entries5":
        assert ctr["hard"] > 0, ctr
    if c["variant"] in ("fuse", "fuse_sim3"):
        assert ctr["hard"] == 0 and ctr["rounds"] == 0 and ctr["in_order"] == 0, ctr
    else:
        assert ctr["pool_used"] > 0 or g[0] == 0, ctr


def _groups(names, key):
    out = {}
    for n in names:
        out.setdefault(key(CASES[n]), []).append(n)
    return sorted(out.items(), key=lambda kv: str(kv[0]))


PROJ_GROUPS = _groups(PROJ, lambda c: (c["variant"], c["th_dist"], c["nnratio"], c["check_ori"]))
BOW_GROUPS = _groups(BOW, lambda c: (c["variant"], c["nnratio"], c["check_ori"]))


@pytest.mark.parametrize("key,names", PROJ_GROUPS, ids=[f"{k[0]}-th{k[1]}-r{k[2]}-ori{int(k[3])}" for k, _ in PROJ_GROUPS])
def test_projection_cases_batched(key, names, oracle_mod):
    variant, th, ratio, ori = key
    probs = [proj_args(CASES[n]) for n in names]
    c0 = CASES[names[0]]
    probs.insert(len(probs) // 2, dict(proj_args(c0), queries=c0["queries"][:0], qdesc=c0["qdesc"][:0]))
    res = ORBmatcher(ratio, ori).search_by_projection_batch(variant, probs, th_dist=th)
    e = res.pop(len(names) // 2)
    assert e[0] == 0 and len(e[1]) == 0 and (e[3] == -1).all()
    for n, g in zip(names, res):
        same(n + " (batch)", PROJ_FIELDS, g, oracle_result(CASES[n], oracle_mod))


@pytest.mark.parametrize("name", BOW)
def test_bow_case(name, oracle_mod):
    c = CASES[name]
    g = ORBmatcher(c["nnratio"], c["check_ori"]).search_by_bow(c["variant"], c["A"], c["B"], c["tri"])
    same(name, BOW_FIELDS, g, oracle_result(c, oracle_mod))
    want = c["expect"]
    built = want != -9
    assert (g[1][built] == want[built]).all(), (name, g[1][built], want[built])


@pytest.mark.parametrize("key,names", BOW_GROUPS, ids=[f"{k[0]}-r{k[1]}-ori{int(k[2])}" for k, _ in BOW_GROUPS])
def test_bow_cases_batched(key, names, oracle_mod):
    variant, ratio, ori = key
    probs = [dict(A=CASES[n]["A"], B=CASES[n]["B"], tri=CASES[n]["tri"]) for n in names]
    c0 = CASES[names[0]]
    empty = {k: (v[:0] if k in ("keys", "desc", "flags", "ids", "feat") else v[:1]) for k, v in c0["A"].items()}
    probs.insert(len(probs) // 2, dict(A=empty, B=c0["B"], tri=c0["tri"]))
    res = ORBmatcher(ratio, ori).search_by_bow_batch(variant, probs)
    e = res.pop(len(names) // 2)
    assert e[0] == 0 and len(e[1]) == 0 and (e[2] == -1).all()
    for n, g in zip(names, res):
        same(n + " (batch)", BOW_FIELDS, g, oracle_result(CASES[n], oracle_mod))


@pytest.mark.parametrize("name", INIT)
def test_initialization_case(name, oracle_mod):
    c = CASES[name]
    prev = c["prev"].copy()
    nm, m12 = ORBmatcher(c["nnratio"], c["check_ori"]).SearchForInitialization(
        Frame(c["k1"], c["d1"], mc.W, mc.H, bounds=c["bounds"]), Frame(c["k2"], c["d2"], mc.W, mc.H, bounds=c["bounds"]),
        prev, c["window"])
    same(name, ("nmatches", "matches12", "prev"), (nm, m12, prev), oracle_result(c, oracle_mod))
    if c["expect"] is not None:
        assert m12.tolist() == c["expect"], (name, m12, c["expect"])


def test_sim3_case(oracle_mod):
    c = CASES["sim3-agreement"]
    g = ORBmatcher(0.75, False).search_by_sim3(c["kf1"], c["kf2"], c["q1"], c["qd1"], c["q2"], c["qd2"], c["th_dist"])
    same(c["name"], ("nfound", "matches12"), g, oracle_result(c, oracle_mod))
    assert g[1].tolist() == c["expect"]


def test_fuse_octave_outside_levels():
    """Keypoint octaves outside [0, nlevels): invSigma2 counts as 0 and Fuse's
    reprojection gate passes (k_proj_search); the oracle refuses such input."""
    c = mc.proj_fuse_octave_outside()
    g = ORBmatcher(c["nnratio"], False).search_by_projection("fuse", th_dist=c["th_dist"], **proj_args(c))
    assert g[0] == len(c["expect"]) and g[1].tolist() == c["expect"] and (g[2] == 3).all(), g
