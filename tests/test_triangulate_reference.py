"""pyref_triangulate.py, the restatement every other triangulation test is
held to, pinned itself: against a float64 triangulation on numpy.linalg.svd
over seeded well-conditioned pairs (selected by geometry), against deliberate
slips, against the ground truth on noise-free pairs, and case by case against
what each named case of triangulate_cases.py says it reaches.  Also the cosine
identity of §3.16 against the float32 arctan2 / cos chain, and the walk against
a literal loop.  No GPU.

Measured here (numpy 2, x86-64): SVD against float64 max 2.26e-6 of the
point's distance over 410 pairs; the cosine identity max 194,788 float ulps from
the float32 chain over 120,000 points, at depth = mb / 2 where the cosine
crosses zero (3.4e-7 absolute); 3 ulps where |cos| > 0.5; 11.5 % differ at all."""
import functools

import numpy as np
import pytest

import pyref_triangulate as ref
import triangulate_cases as cases
from orb_slam_2_ros_amd import create_new_map_points_walk
from orb_slam_2_ros_amd.synth_triangulate import make_triangulation_problem

MEASURED_SVD = 2.26e-6           # the maximum below, as measured
SVD_BOUND = 4 * MEASURED_SVD     # §3.15's margin: float Jacobi against LAPACK rounding
MEASURED_COS_ULPS = 194788            # the maximum of the cosine sweep, as measured
COS_BOUND_ULPS = 2 * MEASURED_COS_ULPS
MEASURED_COS_ULPS_RIG = 3        # the same where |cos| > 0.5, as measured


def svd64(v1, v2, o1, o2):
    """the linear triangulation in float64 on numpy.linalg.svd, from the same float32 inputs"""
    rows = []
    for v, o in ((v1, o1), (v2, o2)):
        T = v["Tcw"].astype(np.float64).reshape(3, 4)
        x = (np.float64(o["u"]) - np.float64(v["cx"])) * np.float64(v["invfx"])
        y = (np.float64(o["v"]) - np.float64(v["cy"])) * np.float64(v["invfy"])
        rows += [x * T[2] - T[0], y * T[2] - T[1]]
    h = np.linalg.svd(np.array(rows))[2][3]
    return h[:3] / h[3]


@functools.lru_cache(maxsize=None)
def well_conditioned():
    """[(v1, v2, rf, o1, o2, X_true)]: mono pairs with parallax between 2 and 40
    degrees, depth 1 to 30 baselines, at least 1 m in front of both cameras"""
    out = []
    for seed in range(6):
        P = make_triangulation_problem(80, seed=3000 + seed, noise_px=0.5, baseline=0.5, depth=(1.2, 14.0))
        (R1, t1), (R2, t2) = P["poses"]
        C1, C2 = -R1.T @ t1, -R2.T @ t2
        for k, X in zip(P["pairs"], P["X_true"]):
            a, b = X - C1, X - C2
            par = np.degrees(np.arccos(a @ b / np.linalg.norm(a) / np.linalg.norm(b)))
            z1, z2 = (R1 @ X + t1)[2], (R2 @ X + t2)[2]
            if 2 < par < 40 and 0.5 <= z1 <= 15 and min(z1, z2) >= 1:
                out.append((P["v1"][0], P["v2"][0], P["ratio_factor"], k["o1"], k["o2"], X))
    return out


def deviations(slip=None):
    dev = []
    for v1, v2, rf, o1, o2, _ in well_conditioned():
        X, status, d = ref.pair(v1, v2, rf, o1, o2, slip=slip)
        if d["branch"] != "svd" or status in (1, 2):
            dev.append(np.inf)   # a slip that sends the pair elsewhere is as wrong as can be
            continue
        X64 = svd64(v1, v2, o1, o2)
        dev.append(np.linalg.norm(X.astype(np.float64) - X64) / np.linalg.norm(X64 - v1["Ow"].astype(np.float64)))
    return np.array(dev)


def test_restatement_against_float64_svd():
    dev = deviations()
    print(f"SVD against float64: {len(dev)} pairs, max {dev.max():.3e}, median {np.median(dev):.3e}")
    assert len(dev) >= 300
    assert dev.max() <= SVD_BOUND


@pytest.mark.parametrize("slip", ["rows-swapped", "vt-column"])
def test_deliberate_slips_exceed_the_bound(slip):
    dev = deviations(slip)
    print(f"{slip}: median {np.median(dev):.3e} = {np.median(dev) / SVD_BOUND:.0f} x the bound")
    assert np.median(dev) > 100 * SVD_BOUND


def test_rcw_for_rwc_shows_in_the_ray_cosine():
    """Rwc only feeds the parallax test, so this slip is held to the float64
    cosine of the two rays instead: the restatement stays within 1e-6 of it
    (three float roundings of 6e-8 on either ray), the slip is a hundred times
    further off"""
    ok, bad = [], []
    for v1, v2, rf, o1, o2, _ in well_conditioned():
        r = []
        for v, o in ((v1, o1), (v2, o2)):
            R = v["Tcw"].astype(np.float64).reshape(3, 4)[:, :3]
            xn = np.array([(np.float64(o["u"]) - v["cx"]) * np.float64(v["invfx"]),
                           (np.float64(o["v"]) - v["cy"]) * np.float64(v["invfy"]), 1.0])
            r.append(R.T @ xn)
        c64 = r[0] @ r[1] / np.linalg.norm(r[0]) / np.linalg.norm(r[1])
        ok.append(abs(ref.pair(v1, v2, rf, o1, o2)[2]["cos_rays"] - c64))
        bad.append(abs(ref.pair(v1, v2, rf, o1, o2, slip="rcw-for-rwc")[2]["cos_rays"] - c64))
    print(f"ray cosine: max {max(ok):.3e}; with Rcw for Rwc median {np.median(bad):.3e}")
    assert max(ok) <= 1e-6 and np.median(bad) > 1e-4


def test_noise_free_pairs_are_created_at_the_truth():
    n = 0
    for seed in range(3):
        P = make_triangulation_problem(40, seed=3100 + seed, noise_px=0.0, baseline=0.5, depth=(2.0, 10.0))
        pts = ref.triangulate(P["v1"], P["v2"], P["ratio_factor"], P["pairs"])
        (R1, t1), _ = P["poses"]
        for p, X in zip(pts, P["X_true"]):
            assert p["status"] == 0
            # the observations are float32 pixels: their rounding (2^-16 px of ~500 px focal length at a
            # parallax of at least 2 degrees) stays inside the bound's margin
            assert np.linalg.norm(p["X"] - X) / np.linalg.norm(X + R1.T @ t1) <= SVD_BOUND
            n += 1
    assert n == 120


def test_cosine_identity_against_the_float32_chain():
    rng = np.random.default_rng(11)
    mb = rng.uniform(0.05, 0.6, 120000).astype(np.float32)
    depth = np.exp(rng.uniform(np.log(0.2), np.log(80.0), 120000)).astype(np.float32)
    chain = np.cos(np.float32(2) * np.arctan2(mb / np.float32(2), depth)).astype(np.float32)
    assert chain.dtype == np.float32
    h, d = (mb / np.float32(2)).astype(np.float64), depth.astype(np.float64)
    ident = ((d * d - h * h) / (d * d + h * h)).astype(np.float32)
    ulps = np.abs(ident.view(np.int32).astype(np.int64) - chain.view(np.int32).astype(np.int64))
    worst = int(np.argmax(ulps))
    print(f"cosine identity: max {ulps.max()} ulps (mb {mb[worst]}, depth {depth[worst]}: {ident[worst]} against "
          f"{chain[worst]}), {np.count_nonzero(ulps)} of {len(ulps)} differ, max absolute "
          f"{np.abs(ident.astype(np.float64) - chain).max():.3e}; away from the zero crossing (|cos| > 0.5) max "
          f"{ulps[np.abs(ident) > 0.5].max()} ulps")
    assert ulps.max() <= COS_BOUND_ULPS
    # the zero crossing dominates that maximum; where a stereo rig works the measured maximum is 3 ulps
    assert ulps[np.abs(ident) > 0.5].max() <= 2 * MEASURED_COS_ULPS_RIG
    for k in range(0, 120000, 9973):   # and the scalar function is that expression
        assert ref.cos_stereo(mb[k], depth[k]) == ident[k]


@pytest.mark.parametrize("name", list(cases.SPECIAL))
def test_named_case_reaches_what_it_says(name):
    P = cases.problem(name)
    pts, dbg = cases.reference(name)
    want = cases.SPECIAL[name][1]
    if want is not None:
        assert list(pts["status"]) == want
    d = dbg[0]
    if name == "parallax-edge":
        assert dbg[0]["cos_rays"] < 0.9998 < dbg[1]["cos_rays"] and dbg[0]["branch"] == "svd"
    if name == "low-parallax":
        assert 0.9998 < d["cos_rays"] < 1
    if name == "cos-negative":
        assert all(x["cos_rays"] <= 0 for x in dbg)
    if name == "w-zero":
        assert d["branch"] == "svd" and list(d["h"]) == [0, 0, 1, 0] or list(d["h"]) == [0, 0, -1, 0]
    if name == "first-sweep":
        assert d["sweeps"] == 1 and d["z1"] == 0
    if name == "many-sweeps":
        assert all(x["sweeps"] > 2 for x in dbg)
    if name == "stereo1-behind-second":
        assert d["branch"] == "stereo1" and d["z1"] > 0 and d["z2"] < 0
    if name == "stereo2":
        assert d["branch"] == "stereo2" and P["pairs"]["o1"]["ur"][0] < 0
        assert np.abs(pts["X"][0] - [0.3, -0.2, 6.0]).max() < 0.01     # mvKeys is a quarter pixel off mvKeysUn
    if name == "both-stereo":
        assert d["branch"] == "stereo1" and d["cs2"] == np.float32(d["cos_rays"] + np.float32(1))
        assert ref.cos_stereo(P["v2"]["mb"][0], P["pairs"]["o2"]["depth"][0]) < d["cs1"]
    if name in ("reproj-edge-kept", "reproj-edge-rejected"):
        s = P["pairs"]["o1"]["sigma2"][0]
        kept = cases.problem("reproj-edge-kept")["pairs"]["o1"]["sigma2"][0]
        assert d["err1"] == P["edge_err"] and (s == kept) == (name == "reproj-edge-kept")
        assert np.nextafter(kept, np.float32(0)) == cases.problem("reproj-edge-rejected")["pairs"]["o1"]["sigma2"][0]
        assert (5.991 * np.float64(s) >= np.float64(d["err1"])) == (name == "reproj-edge-kept")
    if name == "mbf-slip":
        v1 = P["v1"].copy()
        v1["mbf"] = P["v2"]["mbf"]      # what :454 would read had it been written for pKF2
        k = P["pairs"][0]
        assert ref.pair(v1[0], P["v2"][0], P["ratio_factor"], k["o1"], k["o2"])[1] == 0
    if name == "identical-rays":
        assert d["cos_rays"] == 1 and d["branch"] is None
    if name == "near-rank-2":
        assert d["branch"] == "svd" and d["cos_rays"] == np.nextafter(np.float32(1), np.float32(0))
        s = np.linalg.svd(d["A"].astype(np.float64))[1]
        assert s[2] < 1e-2 * s[1]
    if name == "nan":
        assert np.all(np.isnan(pts["X"][0])) and np.isnan(P["v1"]["Tcw"][0][3])
    if name == "zero-distance":
        assert np.array_equal(P["v2"]["Ow"][0], pts["X"][0])
    if name == "scale-ratio":
        assert d["ratio_octave"] > d["ratio_dist"] * P["ratio_factor"]


def test_every_status_is_reached():
    seen = set()
    for name in cases.ALL:
        seen |= set(int(s) for s in cases.reference(name)[0]["status"])
    assert seen >= set(range(9))


def _literal_walk(pairs, status, has, stop_after=None):
    has, out = list(has), []
    for i in range(len(pairs)):
        if i > 0 and stop_after is not None and stop_after <= i:
            return out
        for k in range(len(pairs[i])):
            idx1, idx2 = pairs[i][k]
            if has[idx1]:
                continue
            if status[i][k] != 0:
                continue
            out.append((i, idx1, idx2))
            has[idx1] = True
    return out


def test_walk_against_a_literal_loop():
    pairs = [[(0, 10), (1, 11), (2, 12)], [], [(1, 20), (0, 21), (3, 22), (5, 23)], [(3, 30), (4, 31), (2, 32)]]
    status = [[0, 5, 0], [], [0, 0, 8, 0], [0, 0, 0]]
    has = [False, False, False, False, False, True]
    pts = []
    for i, s in enumerate(status):
        p = np.zeros(len(s), ref.POINT_DTYPE)
        p["status"] = s
        if len(s):
            p["X"] = [[i, k, 0.5] for k in range(len(s))]
        pts.append(p)
    got = create_new_map_points_walk(pairs, pts, has)
    # feature 0 claimed by neighbour 0 is dropped in neighbour 2; feature 1 failed in neighbour 0 (status 5) and did
    # not claim, so neighbour 2 creates it; feature 5 had a point; feature 3 failed in 2 and is created in 3
    assert [g[:3] for g in got] == [(0, 0, 10), (0, 2, 12), (2, 1, 20), (3, 3, 30), (3, 4, 31)]
    assert [g[:3] for g in got] == _literal_walk(pairs, status, has)
    assert got[2][3].tolist() == [2, 0, 0.5] and got[2][3].dtype == np.float32
    for stop in (0, 1, 2, 3, 4, None):
        a = create_new_map_points_walk(pairs, pts, has, stop_after=stop)
        assert [g[:3] for g in a] == _literal_walk(pairs, status, has, stop)
        assert [g[:3] for g in ref.walk(pairs, pts, has, stop)] == [g[:3] for g in a]
    assert len(create_new_map_points_walk(pairs, pts, has, stop_after=1)) == 2      # neighbour 0 always runs
    assert create_new_map_points_walk([], [], has) == []
    assert has == [False, False, False, False, False, True]                          # the caller's list is not edited
