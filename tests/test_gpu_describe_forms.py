"""k_describe's slot grouping: a workgroup describes kDescW consecutive output
slots of one frame (orbx_describe.hip), whatever levels they belong to and
whether or not they hold a keypoint, and each launch of the level pipeline
covers a sub-range of the slots.  kDescW is 1 now (it was 4, and 8 and 16 were
measured); the inputs are chosen for W = 4, so that a wider grouping meets them
again.  Small frames chosen so the grouping can go wrong, byte for byte against
the oracle (ORBextractor.cc:77-147, 1083-1149): level counts that are no
multiple of W, levels without a keypoint, a frame with fewer than W keypoints,
and keypoints within the patch radius of every border (the reflect-101 staging
beside interior patches).  The oracle's own counts are checked for each of
these properties first, so an input that stops exercising one fails instead of
passing silently."""
import numpy as np
import pytest

from orb_slam_2_ros_amd import ORBextractor, synth

pytestmark = pytest.mark.gpu

W = 4                      # the slot group the cases are built for (kDescW <= 4)
PATCH_R = 21               # kDescR: the staged patch's radius
WIDTH, HEIGHT, NLEVELS = 333, 250, 8
NFEATURES = [37, 100, 1000]


def _frames():
    """Three different frames: textured everywhere; flat outside one textured
    quadrant; flat but for one 3 x 3 dot (two keypoints in all)."""
    full = synth.frame(WIDTH, HEIGHT, 33)
    quad = np.full((HEIGHT, WIDTH), 128, np.uint8)
    quad[:HEIGHT // 2, :WIDTH // 2] = synth.frame(WIDTH, HEIGHT, 34)[:HEIGHT // 2, :WIDTH // 2]
    dot = np.full((HEIGHT, WIDTH), 90, np.uint8)
    dot[36:39, 36:39] = 250
    return np.ascontiguousarray(np.stack([full, quad, dot]))


@pytest.fixture(scope="module")
def cases(oracle_mod):
    """The frames and, per nfeatures, the oracle's (keypoints, descriptors) of each (computed once)."""
    frames = _frames()
    return frames, {nf: [oracle_mod.extract(f, nf) for f in frames] for nf in NFEATURES}


def _kp_equal(a, b):
    return len(a) == len(b) and all(np.array_equal(a[f], b[f]) for f in a.dtype.names)


def _check_inputs(oracle_mod, ref, nf):
    """Every property the test is about occurs in the oracle's output for these frames."""
    lw, lh, _, scale = oracle_mod.levels(WIDTH, HEIGHT, nf, 1.2, NLEVELS)
    counts = [np.bincount(k["octave"], minlength=NLEVELS) for k, _ in ref]
    totals = [int(c.sum()) for c in counts]
    assert any(c % W for cs in counts for c in cs), f"no level count off a multiple of {W}: {counts}"
    assert any(t > 0 and (cs == 0).any() for t, cs in zip(totals, counts)), f"no empty level beside a full one: {counts}"
    assert any(0 < t < W for t in totals), f"no frame with fewer than {W} keypoints: {totals}"
    assert any(t > W * NLEVELS for t in totals)
    near = np.zeros(4, bool)   # left, top, right, bottom
    for k, _ in ref:
        l = k["octave"]
        x = np.rint(k["x"] / scale[l]).astype(int)
        y = np.rint(k["y"] / scale[l]).astype(int)
        near |= [(x < PATCH_R).any(), (y < PATCH_R).any(), (x > lw[l] - 1 - PATCH_R).any(),
                 (y > lh[l] - 1 - PATCH_R).any()]
    assert near.all(), f"no keypoint within {PATCH_R} px of some border: {near}"


@pytest.mark.parametrize("nf", NFEATURES)
def test_batch_extract_mixed_groups(nf, cases, oracle_mod):
    """One unpipelined batch call: every slot of a frame in one launch."""
    import torch
    frames, refs = cases
    ref = refs[nf]
    _check_inputs(oracle_mod, ref, nf)
    B = len(frames)
    dev = torch.from_numpy(frames).cuda()
    ex = ORBextractor(nf, 1.2, NLEVELS, 20, 7)
    ex.reserve(WIDTH, HEIGHT, B)
    ex.extract_batch_device(dev.data_ptr(), WIDTH * HEIGHT, WIDTH, B)
    torch.cuda.synchronize()
    for b in range(B):
        kp, de = ex.batch_download(b)
        assert _kp_equal(kp, ref[b][0]) and np.array_equal(de, ref[b][1]), f"frame {b}"
    ex.close()


@pytest.mark.parametrize("nf", NFEATURES)
def test_step_launch_ranges(nf, cases, oracle_mod):
    """The mono step unpipelined, with the level pipeline and with the deep one:
    the describe launches then start at slots s0 > 0 and cover slot counts that
    are no multiple of W.  Identical across the three and to the oracle."""
    import torch
    frames, refs = cases
    ref = refs[nf]
    _check_inputs(oracle_mod, ref, nf)
    B = len(frames)
    dev = torch.from_numpy(frames).cuda()
    outs = []
    for pipe in (0, 1, 2):
        ex = ORBextractor(nf, 1.2, NLEVELS, 20, 7)
        ex.reserve(WIDTH, HEIGHT, B)
        ex.split(1)
        assert ex.pipeline(pipe) == pipe
        for _ in range(2):
            ex.mono_step_device(dev.data_ptr(), WIDTH * HEIGHT, WIDTH, B, 100, 0.9, True)
        torch.cuda.synchronize()
        outs.append([(ex.batch_download(b), ex.mono_matches_download(b)) for b in range(B)])
        ex.close()
    for pipe, out in enumerate(outs):
        for b in range(B):
            (kp, de), (m12, nm) = out[b]
            assert _kp_equal(kp, ref[b][0]) and np.array_equal(de, ref[b][1]), f"pipeline {pipe} frame {b} vs oracle"
            (kp0, de0), (m0, nm0) = outs[0][b]
            assert kp.tobytes() == kp0.tobytes() and np.array_equal(de, de0), f"pipeline {pipe} frame {b}"
            assert nm == nm0 and np.array_equal(m12, m0), f"pipeline {pipe} frame {b} matches"
