"""k_sim3_ransac (orbx_sim3_ransac.hip) against pyref_sim3solver.py, the numpy
restatement of DESIGN.md §3.15, bit for bit: R, t, s, the inlier counts and
the mask words.  Everything is +, -, x, / and sqrt in a fixed order except the
angle's atan2 and Rodrigues' sin and cos, which are the library's on either
side; the device's atan2 is compared with the host's here, on a sweep and on
every argument the cases reach.  The sizes are the chunk edges (64
correspondences per pass) crossed with the workgroup edges (64 hypotheses per
workgroup), scale free and fixed; a run with h hypotheses takes the first h of
the case's 300 triples, so one reference serves every h.  A NaN equals a NaN."""
import math

import numpy as np
import pytest

import sim3solver_cases as cases
from orb_slam_2_ros_amd._lib import ORBX_EINVAL, OrbxError
from orb_slam_2_ros_amd.sim3solver import (_batch_args, debug_atan2, mask_offsets, ransac_device_buffers,
                                           ransac_device_launch, sim3_ransac, sim3_ransac_batch, split_masks,
                                           RANSAC_HYP_DTYPE)

pytestmark = pytest.mark.gpu


def canon(a):
    f = np.frombuffer(np.ascontiguousarray(a).tobytes(), np.uint32).reshape(len(a), 14).copy()
    v = f[:, :13].view(np.float32)
    f[:, :13][np.isnan(v)] = 0x7fc00000
    return f


def assert_equal(hyp, mask, hyp_r, mask_r, what=""):
    a, b = canon(hyp), canon(hyp_r)
    bad = np.nonzero((a != b).any(1))[0]
    assert len(bad) == 0, (what, len(bad), bad[:5], hyp[bad[:2]], hyp_r[bad[:2]])
    assert np.array_equal(np.asarray(mask).reshape(-1), np.asarray(mask_r).reshape(-1)), what


@pytest.mark.parametrize("name", cases.SIZE_CASES, ids=cases.case_id)
def test_sizes_are_bit_equal(name):
    P = cases.problem(name)
    hyp_r, mask_r, _ = cases.reference(name)
    for h in cases.HYPS:
        hyp, mask = sim3_ransac(P["cam1"], P["cam2"], P["fix_scale"], P["corr"], P["triples"][:h])
        assert hyp.shape == (h,) and mask.shape == (h, (name[0] + 63) // 64)
        assert_equal(hyp, mask, hyp_r[:h], mask_r[:h], (name, h))


@pytest.mark.parametrize("name", list(cases.SPECIAL))
def test_named_cases_are_bit_equal(name):
    P = cases.problem(name)
    hyp_r, mask_r, _ = cases.reference(name)
    hyp, mask = sim3_ransac(P["cam1"], P["cam2"], P["fix_scale"], P["corr"], P["triples"])
    assert_equal(hyp, mask, hyp_r, mask_r, name)
    if name == "nan":
        assert np.all(np.isnan(hyp["R"][0])) and hyp["n_inliers"][0] == 0 and not mask[0].any()
    if name in ("edge-out", "edge-in"):
        bit = (int(mask[cases.EDGE_HYP][0]) >> cases.EDGE_CORR) & 1
        assert bit == (name == "edge-in")
    if name == "fix-scale":
        assert np.all(hyp["s"].view(np.uint32) == 0x3f800000)


EMPTY_H = ((20, False), 0)      # correspondences, no hypotheses
EMPTY = (None, 0)               # neither
BATCH = [EMPTY, ((3, False), 5), ((130, True), 300), ("nan", 64), EMPTY_H, ((64, False), 64), EMPTY, ("z0", 64),
         ((65, True), 65), ("recovery", 100), ((63, False), 1), EMPTY]
SMALL = [((20, True), 63), EMPTY, ("edge-in", 8)]


def _batch(items):
    Ps = [(cases.problem(nm if nm is not None else (20, False)), h, nm is None) for nm, h in items]
    K = [P["corr"][:0] if none else P["corr"] for P, h, none in Ps]
    T = [P["triples"][:h] for P, h, none in Ps]
    co = np.concatenate([[0], np.cumsum([len(k) for k in K])]).astype(np.int32)
    ho = np.concatenate([[0], np.cumsum([len(t) for t in T])]).astype(np.int32)
    return (np.concatenate([P["cam1"] for P, *_ in Ps]), np.concatenate([P["cam2"] for P, *_ in Ps]),
            np.array([P["fix_scale"] for P, *_ in Ps], np.int32), np.concatenate(K), co, np.concatenate(T), ho)


def _assert_batch(hyp, mask, items, args):
    co, ho = args[4], args[6]
    masks = split_masks(np.asarray(mask), co, ho)
    for p, (nm, h) in enumerate(items):
        if h == 0:
            assert masks[p].size == 0
            continue
        hyp_r, mask_r, _ = cases.reference(nm)
        assert_equal(hyp[ho[p]:ho[p + 1]], masks[p], hyp_r[:h], mask_r[:h], (p, nm, h))


def test_batch_with_empty_problems():
    """One CSR batch, empty problems first, in the middle and last (one with
    correspondences and no hypotheses, the others with neither)"""
    args = _batch(BATCH)
    hyp, mask = sim3_ransac_batch(*args)
    assert len(hyp) == args[6][-1] and len(mask) == mask_offsets(args[4], args[6])[-1]
    _assert_batch(hyp, mask, BATCH, args)
    none = sim3_ransac_batch(*_batch([EMPTY, EMPTY_H]))
    assert len(none[0]) == 0 and len(none[1]) == 0


def test_device_entry_on_a_side_stream_with_reused_buffers():
    """The _device entry on a side stream equals the host batch; run again on
    the same output tensors with a smaller batch, the small one's results are
    its own and what lies beyond them is the large batch's, untouched."""
    import torch
    st = torch.cuda.Stream()
    big, small = _batch(BATCH), _batch(SMALL)
    host = sim3_ransac_batch(*big)
    dev = sim3_ransac_batch(*big, stream=st)
    assert canon(host[0]).tobytes() == canon(dev[0]).tobytes() and np.array_equal(host[1], dev[1])
    with torch.cuda.stream(st):
        ins, outs = ransac_device_buffers(*_batch_args(*big), st.device)
        ransac_device_launch(ins, outs, len(BATCH), 300, st)
        st.synchronize()
        first = [o.cpu().numpy().copy() for o in outs]
        ins2, _ = ransac_device_buffers(*_batch_args(*small), st.device)
        ransac_device_launch(ins2, outs, len(SMALL), 63, st)
        st.synchronize()
        second = [o.cpu().numpy() for o in outs]
    H, W = int(small[6][-1]), int(mask_offsets(small[4], small[6])[-1])
    hyp = np.frombuffer(second[0].tobytes(), RANSAC_HYP_DTYPE)
    _assert_batch(hyp[:H], second[1].view(np.uint64)[:W], SMALL, small)
    assert second[0][56 * H:].tobytes() == first[0][56 * H:].tobytes()
    assert second[1][W:].tobytes() == first[1][W:].tobytes()
    # and the workspace of the host entry points: a smaller batch after a larger one
    _assert_batch(*sim3_ransac_batch(*small), SMALL, small)


def test_invalid_inputs_are_einval():
    P = cases.problem((20, False))
    for bad in ([0, 0, 1], [3, 4, 3], [0, 1, 20], [-1, 2, 3]):
        T = np.array([[1, 2, 3], bad, [4, 5, 6]], np.int32)
        with pytest.raises(OrbxError) as e:
            sim3_ransac(P["cam1"], P["cam2"], False, P["corr"], T)
        assert e.value.code == ORBX_EINVAL
    for n in (0, 1, 2):
        with pytest.raises(OrbxError) as e:
            sim3_ransac(P["cam1"], P["cam2"], False, P["corr"][:n], np.array([[0, 1, 2]], np.int32))
        assert e.value.code == ORBX_EINVAL
    for n in (0, 2, 20):   # no hypotheses: legal, nothing written
        hyp, mask = sim3_ransac(P["cam1"], P["cam2"], False, P["corr"][:n], np.zeros((0, 3), np.int32))
        assert len(hyp) == 0 and mask.size == 0


def test_device_atan2_equals_the_host():
    """A strided sweep of the angle's domain (y = norm >= 0, x = the
    quaternion's real part, both of a unit eigenvector) and every argument pair
    the shared cases reach.  The angle's only consumer rounds (2 ang)(1 / y)
    to float, and that float is what has to agree; how many doubles differ is
    printed.  On an MI355X: 4,217 of 32,608 doubles differ from glibc's in the
    last bit, none of the float scales."""
    th = np.arange(0, 200001, 7) * (math.pi / 200000)
    ys, xs = list(np.sin(th)), list(np.cos(th))
    for name in cases.ALL:
        for d in cases.reference(name)[2]:
            ys.append(d["atan2"][0])
            xs.append(d["atan2"][1])
    ys, xs = np.array(ys), np.array(xs)
    dev = debug_atan2(ys, xs)
    want = np.array([math.atan2(y, x) for y, x in zip(ys, xs)])
    diff = np.nonzero(dev.view(np.uint64) != want.view(np.uint64))[0]
    print(f"atan2: {len(diff)} of {len(ys)} doubles differ from the host's", [(ys[i], xs[i]) for i in diff[:5]])
    # the angle's only consumer: the float scale of the rotation vector
    with np.errstate(all="ignore"):
        fd = ((2.0 * dev) * (1.0 / ys)).astype(np.float32)
        fw = ((2.0 * want) * (1.0 / ys)).astype(np.float32)
    same = (fd.view(np.uint32) == fw.view(np.uint32)) | (np.isnan(fd) & np.isnan(fw))
    print(f"atan2: {np.count_nonzero(~same)} of {len(ys)} float scales differ")
    assert same.all(), [(ys[i], xs[i]) for i in np.nonzero(~same)[0][:5]]


def test_python_mirror_prepares_in_one_launch_and_walks():
    """orb_slam_2_ros_amd.Sim3Solver: three solvers prepared together, one
    left to launch on its first iterate; hypotheses, flags, T12 and getters
    equal the restatement's on the solver's own triples."""
    import pyref_sim3solver as ref
    from orb_slam_2_ros_amd import Sim3Solver
    solvers, names = [], [(65, False), "recovery", (20, True), (130, True)]
    for k, nm in enumerate(names):
        P = cases.problem(nm)
        n = len(P["corr"])
        rng = np.random.default_rng(k)
        s = Sim3Solver(P["cam1"], P["cam2"], P["corr"], [2 * i for i in range(n)], 2 * n, P["fix_scale"],
                       random_int=lambda lo, hi, rng=rng: int(rng.integers(lo, hi + 1)))
        s.set_ransac_parameters(0.99, 20, 300)
        solvers.append(s)
    Sim3Solver.prepare(solvers[:3])
    assert solvers[3].hyp is None and all(s.hyp is not None for s in solvers[:3])
    for s, nm in zip(solvers, names):
        P = cases.problem(nm)
        n = len(P["corr"])
        first = s.iterate(5)
        assert len(s.triples) == s.max_its == ref.ransac_iterations(n, 0.99, 20, 300)
        hyp_r, mask_r = ref.ransac(P["cam1"], P["cam2"], P["fix_scale"], P["corr"], s.triples)
        assert_equal(s.hyp, s.mask, hyp_r, mask_r, nm)
        w = ref.Walk(n, 2 * n, s.indices1, hyp_r, mask_r, 20, s.max_its)
        got, returned = first, 0
        while True:
            k, nm2, vb, ni = w.iterate(5)
            T, nm1, vb1, ni1 = got
            assert (T is None) == (k is None) and nm1 == nm2 and ni1 == ni and list(vb1) == vb
            if k is not None:
                returned += 1
                want = np.eye(4, dtype=np.float32)
                want[:3, :3] = hyp_r["s"][k] * hyp_r["R"][k].reshape(3, 3)
                want[:3, 3] = hyp_r["t"][k]
                assert T.tobytes() == want.tobytes() and s.best == k
                assert s.get_estimated_scale() == float(hyp_r["s"][k])
                assert np.array_equal(s.get_estimated_translation(), hyp_r["t"][k])
            if nm2:
                break
            got = s.iterate(5)
        assert returned >= 1 or n == 20
