"""pyref_sim3solver.py (the numpy restatement of DESIGN.md §3.15) on its own,
without a GPU: its Horn against a float64 Horn built on numpy.linalg.eigh, the
mutations that bound has to catch, that each shared case reaches what it is
named for, the recovery of a planted inlier set, and the walk against a
literal loop."""
import numpy as np
import pytest

import pyref_sim3solver as ref
import sim3solver_cases as cases
from orb_slam_2_ros_amd.synth_sim3solver import make_sim3solver_problem

# The largest deviation of the float restatement from the float64 Horn over
# the seeded triples below, as test_horn_accuracy measures it (printed there):
MEASURED = 1.48e-6
BOUND = 4 * MEASURED   # the margin: float Jacobi against eigh rounding


def horn64(P1, P2, fix_scale, mutate=None):
    """Horn 1987 in float64 on three point pairs, the eigenvector from
    numpy.linalg.eigh and the rotation straight from the quaternion.  Returns
    the 9 + 1 + 12 + 12 numbers R, s, T12, T21."""
    P1, P2 = np.asarray(P1, np.float64), np.asarray(P2, np.float64)
    O1, O2 = P1.mean(0), P2.mean(0)
    Pr1, Pr2 = (P1 - O1).T, (P2 - O2).T
    M = Pr2 @ Pr1.T
    if mutate == "M transposed":
        M = M.T
    N12 = M[1, 2] - M[2, 1]
    if mutate == "N12 sign":
        N12 = -N12
    N13, N14 = M[2, 0] - M[0, 2], M[0, 1] - M[1, 0]
    N23, N24, N34 = M[0, 1] + M[1, 0], M[2, 0] + M[0, 2], M[1, 2] + M[2, 1]
    N = np.array([[M[0, 0] + M[1, 1] + M[2, 2], N12, N13, N14],
                  [N12, M[0, 0] - M[1, 1] - M[2, 2], N23, N24],
                  [N13, N23, -M[0, 0] + M[1, 1] - M[2, 2], N34],
                  [N14, N24, N34, -M[0, 0] - M[1, 1] + M[2, 2]]])
    w, v = np.linalg.eigh(N)
    q = v[:, int(np.argmax(w))]
    a, b, c, d = q / np.linalg.norm(q)
    R = np.array([[a * a + b * b - c * c - d * d, 2 * (b * c - a * d), 2 * (b * d + a * c)],
                  [2 * (b * c + a * d), a * a - b * b + c * c - d * d, 2 * (c * d - a * b)],
                  [2 * (b * d - a * c), 2 * (c * d + a * b), a * a - b * b - c * c + d * d]])
    P3 = R @ Pr2
    den = (Pr1 * Pr1).sum() if mutate == "den from Pr1" else (P3 * P3).sum()
    s = 1.0 if fix_scale else (Pr1 * P3).sum() / den
    t = O1 - s * R @ O2
    T12 = np.concatenate([s * R, t[:, None]], 1)
    sRinv = R.T / s
    T21 = T12 if mutate == "T21 not inverted" else np.concatenate([sRinv, (-sRinv @ t)[:, None]], 1)
    return np.concatenate([R.reshape(-1), [s], T12.reshape(-1), T21.reshape(-1)])


def _well_conditioned_triples():
    """(P1, P2) float32 point triples whose smallest altitude is at least 0.2
    of the longest side in both cameras"""
    out = []
    for seed in range(12):
        P = make_sim3solver_problem(60, seed=500 + seed, scale=(0.7, 1.0, 1.3, 2.0)[seed % 4],
                                    rot_sigma=(0.1, 0.5, 1.5)[seed % 3])
        rng = np.random.default_rng(seed)
        for _ in range(40):
            idx = rng.choice(60, 3, replace=False)
            sets = P["corr"]["X1c"][idx], P["corr"]["X2c"][idx]
            ok = True
            for X in sets:
                X = X.astype(np.float64)
                sides = [np.linalg.norm(X[i] - X[j]) for i, j in ((0, 1), (1, 2), (0, 2))]
                area2 = np.linalg.norm(np.cross(X[1] - X[0], X[2] - X[0]))
                ok = ok and area2 / max(sides) >= 0.2 * max(sides)
            if ok:
                out.append(sets)
    return out


def _deviation(P1, P2, fix, mutate=None):
    """Largest difference over R, s, T12 and T21, the translations taken
    relative to the largest coordinate of the points"""
    R, t, s, T12, T21 = ref.horn(P1, P2, fix)
    got = np.array([float(x) for x in R + [s] + T12 + T21])
    want = horn64(P1, P2, fix, mutate)
    scale = np.ones(34)
    big = max(np.abs(P1).max(), np.abs(P2).max())
    scale[[13, 17, 21, 25, 29, 33]] = big
    return float(np.max(np.abs(got - want) / scale))


def test_horn_accuracy():
    """Measured: 1.48e-6 at most over 385 triples (rotations of 0.1 to
    1.5 rad sigma, scales 0.7 to 2); the bound is four times that."""
    T = _well_conditioned_triples()
    assert len(T) > 100
    worst = max(_deviation(P1, P2, fix) for P1, P2 in T for fix in (False,))
    print(f"horn deviation from float64: {worst:.3e} over {len(T)} triples (bound {BOUND:.3e})")
    assert worst <= BOUND


@pytest.mark.parametrize("mutate", ["M transposed", "N12 sign", "den from Pr1", "T21 not inverted"])
def test_mutation_exceeds_the_bound(mutate):
    """Each mistake moves the result by at least 100 bounds on every triple
    (the scale's only where the scale is not 1)"""
    T = _well_conditioned_triples()
    devs = []
    for P1, P2 in T:
        if mutate == "den from Pr1":
            r1 = np.linalg.norm(P1[0].astype(np.float64) - P1[1]) / np.linalg.norm(P2[0].astype(np.float64) - P2[1])
            if abs(r1 - 1) < 0.2:
                continue
        devs.append(_deviation(P1, P2, False, mutate))
    print(f"{mutate}: smallest deviation {min(devs):.3e} over {len(devs)} triples")
    assert len(devs) > 50 and min(devs) >= 100 * BOUND


def _bits(mask, n):
    return np.array([(int(mask[i >> 6]) >> (i & 63)) & 1 for i in range(n)], bool)


def test_nan_case():
    hyp, mask, det = cases.reference("nan")
    N = np.array(det[0]["N"], np.float32)
    assert np.all(N == 0)   # exactly diagonal
    assert det[0]["atan2"] == (0.0, 1.0) and det[0]["rotations"] == 0
    assert np.all(np.isnan(hyp["R"][0])) and np.all(np.isnan(hyp["t"][0])) and np.isnan(hyp["s"][0])
    assert hyp["n_inliers"][0] == 0 and not mask[0].any()
    assert hyp["n_inliers"][1:].max() > 6   # the others are ordinary


def test_threshold_edge_cases():
    out, inn = cases.problem("edge-out"), cases.problem("edge-in")
    e1, e2 = out["edge_err"]
    k = cases.EDGE_CORR
    assert 0 < e1 < 9 and e2 < out["corr"]["max_err2"][k] and np.isfinite(e1)
    assert out["corr"]["max_err1"][k] == e1 and inn["corr"]["max_err1"][k] == np.nextafter(e1, np.float32(np.inf))
    assert k not in list(out["triples"][cases.EDGE_HYP])
    ho, mo, _ = cases.reference("edge-out")
    hi, mi, _ = cases.reference("edge-in")
    n = len(out["corr"])
    bo, bi = _bits(mo[cases.EDGE_HYP], n), _bits(mi[cases.EDGE_HYP], n)
    assert not bo[k] and bi[k]
    assert np.array_equal(np.delete(bo, k), np.delete(bi, k))
    assert hi["n_inliers"][cases.EDGE_HYP] == ho["n_inliers"][cases.EDGE_HYP] + 1


def test_collinear_case():
    P = cases.problem("collinear")
    hyp, mask, det = cases.reference("collinear")
    for key in ("X1c", "X2c"):
        X = P["corr"][key][:3].astype(np.float64)
        assert np.linalg.norm(np.cross(X[1] - X[0], X[2] - X[0])) == 0.0
    assert tuple(P["triples"][0]) == (0, 1, 2) and det[0]["rotations"] > 0
    # whatever the Jacobi gives is a rotation about the line or NaN; it is recorded, not judged
    assert hyp["n_inliers"][0] == _bits(mask[0], len(P["corr"])).sum()


def test_z0_case():
    P = cases.problem("z0")
    hyp, mask, _ = cases.reference("z0")
    assert P["corr"]["X1c"][5][2] == 0 and P["corr"]["X2c"][6][2] == 0
    u, _ = ref.own_projection(P["corr"]["X1c"][5:6], P["cam1"][0])
    assert np.isinf(u[0]) or np.isnan(u[0])
    n = len(P["corr"])
    for k in range(len(hyp)):
        b = _bits(mask[k], n)
        assert not b[5] and not b[6]
    assert hyp["n_inliers"].max() > 20


def test_fix_scale_keeps_one():
    for name in ("fix-scale", (65, True)):
        hyp, _, _ = cases.reference(name)
        assert np.all(hyp["s"].view(np.uint32) == np.float32(1.0).view(np.uint32))
    assert not np.any(cases.reference((65, False))[0]["s"] == np.float32(1.0))


def test_recovery_of_the_unplanted_set():
    """40 % planted outliers and no noise: every triple drawn from the
    unplanted correspondences gives exactly the unplanted set"""
    P = cases.problem("recovery")
    hyp, mask, _ = cases.reference("recovery")
    n, planted = len(P["corr"]), P["planted"]
    assert 0.3 < planted.mean() < 0.5
    clean = [k for k, t in enumerate(P["triples"]) if not planted[list(t)].any()]
    assert len(clean) >= 10
    for k in clean:
        assert np.array_equal(_bits(mask[k], n), ~planted), k
        assert hyp["n_inliers"][k] == (~planted).sum()
        assert abs(float(hyp["s"][k]) - P["s_true"]) < 1e-3 and np.abs(hyp["R"][k].reshape(3, 3) - P["R_true"]).max() < 1e-3


def test_masks_and_counts_agree():
    for name in cases.ALL:
        hyp, mask, _ = cases.reference(name)
        n = len(cases.problem(name)["corr"])
        for k in range(0, len(hyp), 7):
            assert _bits(mask[k], n).sum() == hyp["n_inliers"][k]
            assert n % 64 == 0 or int(mask[k][-1]) >> (n & 63) == 0


def test_ransac_iterations():
    """SetRansacParameters with (0.99, 20, 300): N == minInliers is one
    iteration, fewer than that too (the walk never runs them), and the count
    falls as the inlier share grows"""
    assert ref.ransac_iterations(20, 0.99, 20, 300) == 1
    assert ref.ransac_iterations(10, 0.99, 20, 300) == 1
    assert ref.ransac_iterations(21, 0.99, 20, 300) == 3
    assert ref.ransac_iterations(40, 0.99, 20, 300) == 35
    assert ref.ransac_iterations(200, 0.99, 20, 300) == 300
    assert ref.ransac_iterations(0, 0.99, 20, 300) == 1


def literal_walk(counts, calls, N, min_inliers, max_its):
    """iterate() as the reference writes it (:140-207), over a list of inlier
    counts.  Returns per call (returned hypothesis or None, bNoMore, nInliers)
    and the best hypothesis at the end."""
    mnIterations, mnBestInliers, best = 0, 0, None
    out = []
    for nIterations in calls:
        bNoMore, nInliers = False, 0
        if N < min_inliers:
            out.append((None, True, 0))
            continue
        nCurrentIterations, returned = 0, None
        while mnIterations < max_its and nCurrentIterations < nIterations:
            nCurrentIterations += 1
            mnIterations += 1
            c = counts[mnIterations - 1]
            if c >= mnBestInliers:
                mnBestInliers, best = c, mnIterations - 1
                if c > min_inliers:
                    nInliers, returned = c, mnIterations - 1
                    break
        if returned is None and mnIterations >= max_its:
            bNoMore = True
        out.append((returned, bNoMore, nInliers))
    return out, best


WALKS = {
    # name: (counts, calls, N, min_inliers)
    "count == min returns nothing": ([20, 20, 20, 19, 20], [5, 5], 30, 20),
    "tie after a return": ([5, 25, 25, 3, 25, 26], [2, 2, 2, 2], 30, 20),
    "above min below best": ([28, 22, 27, 28, 21, 29], [1, 5, 5, 5], 30, 20),
    "success on the last iteration, then no more": ([3, 4, 5, 6, 25], [5, 5, 5], 30, 20),
    "N < min": ([3, 3, 3], [5, 5], 10, 20),
    "find": ([1, 2, 30, 31], [4, 4], 40, 20),
    "find without a result": ([1, 2, 20, 7], [4], 40, 20),
    "partial calls": ([0] * 12 + [21], [5, 5, 5, 5], 25, 20),
}


@pytest.mark.parametrize("name", list(WALKS))
def test_walk_equals_the_literal_loop(name):
    counts, calls, N, mn = WALKS[name]
    h = len(counts)
    hyp = np.zeros(h, ref.HYP_DTYPE)
    hyp["n_inliers"] = counts
    mask = np.zeros((h, 1), np.uint64)
    for k, c in enumerate(counts):
        mask[k, 0] = (1 << c) - 1   # the first c correspondences
    indices1 = [2 * i + 1 for i in range(N)]
    w = ref.Walk(N, 2 * N + 5, indices1, hyp, mask, mn, h)
    want, best = literal_walk(counts, calls, N, mn, h)
    for call, (ret, no_more, n_inl) in zip(calls, want):
        if name.startswith("find"):
            k, vb, ni = w.find()
            nm = no_more
        else:
            k, nm, vb, ni = w.iterate(call)
        assert (k, nm, ni) == (ret, no_more, n_inl), (name, call)
        assert len(vb) == 2 * N + 5
        on = [i for i, b in enumerate(vb) if b]
        assert on == ([] if ret is None else indices1[:counts[ret]])
    assert w.best == best


def test_walk_cases_reach_what_they_are_named_for():
    r, _ = literal_walk(*WALKS["count == min returns nothing"][:2], 30, 20, 5)
    assert r == [(None, True, 0), (None, True, 0)]
    r, best = literal_walk(*WALKS["tie after a return"][:2], 30, 20, 6)
    assert r == [(1, False, 25), (2, False, 25), (4, False, 25), (5, False, 26)] and best == 5
    r, best = literal_walk(*WALKS["above min below best"][:2], 30, 20, 6)
    assert r == [(0, False, 28), (3, False, 28), (5, False, 29), (None, True, 0)] and best == 5
    r, _ = literal_walk(*WALKS["success on the last iteration, then no more"][:2], 30, 20, 5)
    assert r == [(4, False, 25), (None, True, 0), (None, True, 0)]
    r, best = literal_walk(*WALKS["N < min"][:2], 10, 20, 3)
    assert r == [(None, True, 0), (None, True, 0)] and best is None


def test_python_mirror_walks_like_the_restatement():
    """orb_slam_2_ros_amd.Sim3Solver.iterate over injected hypotheses equals Walk"""
    from orb_slam_2_ros_amd import Sim3Solver
    P = cases.problem("recovery")
    hyp, mask, _ = cases.reference("recovery")
    n = len(P["corr"])
    indices1 = [3 * i for i in range(n)]
    s = Sim3Solver(P["cam1"], P["cam2"], P["corr"], indices1, 3 * n, P["fix_scale"])
    s.set_ransac_parameters(0.99, 20, 100)
    assert s.max_its == ref.ransac_iterations(n, 0.99, 20, 100) == 100
    s._store(P["triples"], hyp, mask)
    w = ref.Walk(n, 3 * n, indices1, hyp, mask, 20, s.max_its)
    for _ in range(s.max_its // 5 + 2):
        T, nm, vb, ni = s.iterate(5)
        k, nm2, vb2, ni2 = w.iterate(5)
        assert (T is None) == (k is None) and nm == nm2 and ni == ni2 and list(vb) == vb2
        if k is not None:
            assert np.array_equal(T[:3, 3], hyp["t"][k]) and s.best == k
            assert np.array_equal(s.get_estimated_rotation().reshape(-1), hyp["R"][k])
            assert s.get_estimated_scale() == float(hyp["s"][k])
