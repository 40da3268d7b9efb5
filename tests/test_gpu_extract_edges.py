"""The extractor's kernels against the oracle, byte for byte and stage by
stage (orientation at 0 ulp), on the inputs synth.frame never produces
(tests/extract_cases.py; test_extract_cases.py shows on the CPU that each one
reaches what it is for): pixel values at 0 and 255 against every threshold
edge (k_fast's packed saturating compares), cells with more compass survivors
than the survivor list holds (the flush in mid cell), equal scores and corners
on a cell's edges (the strict NMS), a cell at its candidate cap, patches of
ties and zero moments (k_describe), frames without a keypoint beside full ones
in a batch, every interior cell width and height the grid can make (lane
geometry, both staging paths, both patch strides), and padded or misaligned
input images through the host and the device entry points."""
import ctypes

import numpy as np
import pytest

import extract_cases as ec
from orb_slam_2_ros_amd import ORBextractor, _lib, synth
from orb_slam_2_ros_amd._lib import KEYPOINT_DTYPE

pytestmark = pytest.mark.gpu


def _first_diff(a, b):
    idx = np.nonzero(a != b)
    return tuple(int(i[0]) for i in idx) if len(idx[0]) else None


def _same_output(kg, dg, ko, do, what=""):
    assert len(kg) == len(ko), f"{what}: {len(kg)} keypoints vs the oracle's {len(ko)}"
    for f in ko.dtype.names:
        a, b = kg[f], ko[f]
        if f == "angle":   # 0 ulp: the bit patterns
            a, b = a.view(np.uint32), b.view(np.uint32)
        assert np.array_equal(a, b), f"{what}: keypoint field {f} differs at {_first_diff(a, b)}"
    assert np.array_equal(dg, do), f"{what}: descriptors differ at {_first_diff(dg, do)}"


def _check_stages(ex, img, nf, scale, nlev, ini, mn, oracle_mod, stages=(0, 1, 2, 3), frame=0):
    h, w = img.shape
    pyr = oracle_mod.pyramid(img, scale, nlev)
    _, _, quotas, _ = oracle_mod.levels(w, h, nf, scale, nlev)
    for l in range(nlev):
        if 0 in stages:
            gp = ex.debug_fetch(frame, l, 0)
            assert gp.shape == pyr[l].shape and np.array_equal(gp, pyr[l]), f"pyramid level {l} differs at {_first_diff(gp, pyr[l])}"
        if 1 in stages:
            gb, ob = ex.debug_fetch(frame, l, 1), oracle_mod.gauss7(pyr[l])
            assert np.array_equal(gb, ob), f"blur level {l} differs at {_first_diff(gb, ob)}"
        oc = oracle_mod.level_candidates(pyr[l], ini, mn)
        if 2 in stages:
            gc = ex.debug_fetch(frame, l, 2)
            assert gc.shape == oc.shape and np.array_equal(gc, oc), \
                f"FAST candidates level {l}: {len(gc)} vs {len(oc)}, first difference {_first_diff(gc, oc) if gc.shape == oc.shape else None}"
        if 3 in stages:
            gs = ex.debug_fetch(frame, l, 3)
            osel = oc[oracle_mod.distribute(oc, pyr[l].shape[1], pyr[l].shape[0], int(quotas[l]))]
            assert gs.shape == osel.shape and np.array_equal(gs, osel), f"quadtree level {l}: {len(gs)} vs {len(osel)}"


@pytest.fixture(scope="module")
def extractors():
    cache = {}

    def get(nfeat, scale, nlev, ini, mn):
        key = (nfeat, scale, nlev, ini, mn)
        if key not in cache:
            cache[key] = ORBextractor(nfeat, scale, nlev, ini, mn)
        return cache[key]
    yield get
    for ex in cache.values():
        ex.close()


# ---- every image x every threshold pair ------------------------------------------
@pytest.mark.parametrize("name", ec.IMAGE_NAMES)
@pytest.mark.parametrize("ini,mn", ec.GPU_THRESHOLDS, ids=[f"{a}-{b}" for a, b in ec.GPU_THRESHOLDS])
def test_adversarial_images(name, ini, mn, extractors, oracle_mod):
    img = ec.image(name, ini, mn)
    nf = ec.nfeatures(name)
    ex = extractors(nf, ec.SCALE, ec.NLEVELS, ini, mn)
    kg, dg = ex(img)
    _check_stages(ex, img, nf, ec.SCALE, ec.NLEVELS, ini, mn, oracle_mod)
    ko, do = ec.oracle_extract(name, ini, mn)
    _same_output(kg, dg, ko, do, f"{name} ({ini}, {mn})")


# ---- frames without a keypoint beside full ones ---------------------------------
def _expected_matches(oracle_mod, prev_kd, cur_kd, w, h):
    (k1, d1), (k2, d2) = prev_kd, cur_kd
    if len(k1) == 0 or len(k2) == 0:
        return 0, np.full(len(k1), -1, np.int32)
    prev = np.ascontiguousarray(np.stack([k1["x"], k1["y"]], 1).astype(np.float32))
    nm, m, _ = oracle_mod.search_for_initialization(k1, d1, k2, d2, w, h, prev, 100, 0.9, True)
    return nm, m


@pytest.fixture(scope="module")
def mixed_steps(oracle_mod):
    """Three steps of the mixed batch and the oracle's output of every frame.
    Step 2 shifts the streams by one, so that a stream goes empty -> empty,
    full -> empty, full -> full and empty -> full."""
    steps = [ec.mixed(0), ec.mixed(1), np.ascontiguousarray(np.roll(ec.mixed(2), 1, axis=0))]
    ref = [[oracle_mod.extract(f, ec.NFEATURES, ec.SCALE, ec.NLEVELS, 20, 7) for f in s] for s in steps]
    n = [[len(k) for k, _ in r] for r in ref]
    assert n[0][0] == 0 and n[0][3] == 0 and n[0][1] > 300 and n[0][2] > 20, n
    assert [(a > 0, b > 0) for a, b in zip(n[1], n[2])] == [(False, False), (True, False), (True, True), (False, True)], n
    return steps, ref


def test_mixed_batch_extract(mixed_steps, oracle_mod):
    import torch
    steps, ref = mixed_steps
    B = len(steps[0])
    ex = ORBextractor(ec.NFEATURES, ec.SCALE, ec.NLEVELS, 20, 7)
    ex.reserve(ec.W0, ec.H0, B)
    dev = torch.from_numpy(steps[0]).cuda()
    ex.extract_batch_device(dev.data_ptr(), ec.W0 * ec.H0, ec.W0, B)
    torch.cuda.synchronize()
    for b in range(B):
        kg, dg = ex.batch_download(b)
        _same_output(kg, dg, *ref[0][b], f"stream {b} ({ec.MIXED_NAMES[b]})")
        _check_stages(ex, steps[0][b], ec.NFEATURES, ec.SCALE, ec.NLEVELS, 20, 7, oracle_mod, stages=(2, 3), frame=b)
    ex.close()


@pytest.mark.parametrize("pipeline", [0, 1, 2])
def test_mixed_batch_mono_steps(pipeline, mixed_steps, oracle_mod):
    """An empty stream reports 0 keypoints and 0 matches with every matches12
    entry -1, whichever of its two frames is the empty one; its full
    neighbours equal the oracle, matches included."""
    import torch
    steps, ref = mixed_steps
    B = len(steps[0])
    ex = ORBextractor(ec.NFEATURES, ec.SCALE, ec.NLEVELS, 20, 7)
    ex.reserve(ec.W0, ec.H0, B)
    ex.split(1)
    assert ex.pipeline(pipeline) == pipeline
    dev = [torch.from_numpy(s).cuda() for s in steps]
    ex.mono_step_device(dev[0].data_ptr(), ec.W0 * ec.H0, ec.W0, B)
    for t in (1, 2):
        ex.mono_step_device(dev[t].data_ptr(), ec.W0 * ec.H0, ec.W0, B)
        torch.cuda.synchronize()
        for b in range(B):
            kg, dg = ex.batch_download(b)
            _same_output(kg, dg, *ref[t][b], f"step {t} stream {b}")
            nm_o, m_o = _expected_matches(oracle_mod, ref[t - 1][b], ref[t][b], ec.W0, ec.H0)
            m_g, nm_g = ex.mono_matches_download(b)
            assert nm_g == nm_o and len(m_g) == len(m_o) and np.array_equal(m_g, m_o), f"step {t} stream {b} matches"
            if len(ref[t - 1][b][0]) == 0 or len(ref[t][b][0]) == 0:
                assert nm_g == 0 and (m_g == -1).all()
    ex.close()


# ---- every cell shape -----------------------------------------------------------------
def _chunks(seq, n):
    return [tuple(seq[i:i + n]) for i in range(0, len(seq), n)]


@pytest.mark.parametrize("axis", ["width", "height"])
@pytest.mark.parametrize("sizes", _chunks(ec.sweep_sizes(), 8), ids=lambda s: f"{s[0]}-{s[-1]}")
def test_cell_shape_sweep(sizes, axis, extractors, oracle_mod):
    """One level, one row (column) of cells: FAST candidates and the final
    output for every interior cell width (height) from 1 to 53."""
    nf = 500
    ex = extractors(nf, 1.2, 1, 20, 7)
    for n in sizes:
        w, h = ec.sweep_shape(axis, n)
        img = ec.sweep_image(w, h, n)
        kg, dg = ex(img)
        _check_stages(ex, img, nf, 1.2, 1, 20, 7, oracle_mod, stages=(2,))
        ko, do = oracle_mod.extract(img, nf, 1.2, 1, 20, 7)
        assert len(ko) > 0
        _same_output(kg, dg, ko, do, f"{w} x {h}")


def test_cell_shape_sweep_two_levels(extractors, oracle_mod):
    """The 48 | 64 stride boundary with a second level in the same launch
    (the stride is chosen from the widest cell of all levels)."""
    ex = extractors(500, 1.2, 2, 20, 7)
    for w, h in [(77, 92), (78, 92), (92, 77), (92, 78), (91, 91)]:
        img = ec.sweep_image(w, h, w + h)
        kg, dg = ex(img)
        _check_stages(ex, img, 500, 1.2, 2, 20, 7, oracle_mod, stages=(0, 2, 3))
        ko, do = oracle_mod.extract(img, 500, 1.2, 2, 20, 7)
        assert (ko["octave"] == 1).any()
        _same_output(kg, dg, ko, do, f"{w} x {h}")


# ---- padded and misaligned inputs ---------------------------------------------------------
PAD_SIZES = [(152, 100), (333, 250)]
NF_PAD = 500


def _layouts(w):
    """(pitch, frame-stride slack, base offset): the odd ones are repacked
    on the device first; the multiples of 4 are read in place at the
    caller's pitch."""
    out = [(w + 1, 37, 0), (w + 5, 37, 1), (w + 64, 37, 3), (w + 1, 37, 3), (w + 64, 37, 1)]
    p4 = (w + 64 + 3) & ~3
    return out + [(p4, 40, 0), (p4, 40, 4), ((w + 3) & ~3, 0, 8)]


def _padded(frames, pitch, slack, off, fill):
    """The frames laid out at `pitch` / `pitch h + slack` from byte `off` of a buffer full of `fill`."""
    B, h, w = frames.shape
    stride = pitch * h + slack
    buf = np.full(off + B * stride + 64, fill, np.uint8)
    for b in range(B):
        v = buf[off + b * stride: off + b * stride + pitch * h].reshape(h, pitch)
        v[:, :w] = frames[b]
    return buf, stride


@pytest.fixture(scope="module")
def pad_frames(oracle_mod):
    out = {}
    for w, h in PAD_SIZES:
        L, R = synth.stereo_pair(w, h, 91, 0, 9)
        L2, R2 = synth.stereo_pair(w, h, 92, 0, 6)
        fr = np.ascontiguousarray(np.stack([L, R, ec.uniform(w, h, 5), synth.frame(w, h, 93), L2, R2]))
        out[(w, h)] = fr, [oracle_mod.extract(f, NF_PAD) for f in fr]
    return out


@pytest.mark.parametrize("w,h", PAD_SIZES)
def test_padded_host_images(w, h, pad_frames, extractors):
    fr, ref = pad_frames[(w, h)]
    ex = extractors(NF_PAD, 1.2, 8, 20, 7)
    lib = _lib.load()
    cap = NF_PAD + 16 * 8 + 64
    for pitch, slack, off in _layouts(w):
        for fill in (255, 0):
            buf, stride = _padded(fr[:2], pitch, slack, off, fill)
            for b in range(2):
                kps = np.zeros(cap, KEYPOINT_DTYPE)
                desc = np.zeros((cap, 32), np.uint8)
                n = ctypes.c_int(0)
                rc = lib.orbx_extract(ex._h, ctypes.c_void_p(buf.ctypes.data + off + b * stride), w, h,
                                      ctypes.c_size_t(pitch), _lib.ptr(kps), _lib.ptr(desc), cap, ctypes.byref(n))
                assert rc == 0
                _same_output(kps[:n.value], desc[:n.value], *ref[b], f"pitch {pitch} offset {off} fill {fill} frame {b}")
            assert (buf[:off] == fill).all()


@pytest.mark.parametrize("w,h", PAD_SIZES)
@pytest.mark.parametrize("entry", ["extract", "mono", "stereo"])
def test_padded_device_images(entry, w, h, pad_frames, oracle_mod):
    """B = 3 frames (stereo: 3 pairs) at every layout, the padding full of 255
    and then of 0: the results equal the tightly packed run's and the oracle's."""
    import torch
    fr, ref = pad_frames[(w, h)]
    B = 6 if entry == "stereo" else 3
    frames = fr[:B] if entry == "stereo" else fr[1:4]
    refs = ref[:B] if entry == "stereo" else ref[1:4]
    bf, mb = 40.0, float(np.float32(40.0) / np.float32(300.0))
    ex = ORBextractor(NF_PAD, 1.2, 8, 20, 7)
    ex.reserve(w, h, B)

    def run(d_ptr, stride, pitch):
        if entry == "extract":
            ex.extract_batch_device(d_ptr, stride, pitch, B)
        elif entry == "mono":
            for _ in range(2):
                ex.mono_step_device(d_ptr, stride, pitch, B)
        else:
            ex.stereo_step_device(d_ptr, stride, pitch, B // 2, bf, mb)
        torch.cuda.synchronize()
        out = [ex.batch_download(b) for b in range(B)]
        if entry == "mono":
            out += [ex.mono_matches_download(b) for b in range(B)]
        if entry == "stereo":
            out += [ex.depth_download(p) for p in range(B // 2)]
        return out

    tight = torch.from_numpy(frames).cuda()
    base = run(tight.data_ptr(), w * h, w)
    for b in range(B):
        _same_output(*base[b], *refs[b], f"packed frame {b}")
    if entry == "mono":
        for b in range(B):
            k, d = refs[b]
            prev = np.ascontiguousarray(np.stack([k["x"], k["y"]], 1).astype(np.float32))
            nm, m, _ = oracle_mod.search_for_initialization(k, d, k, d, w, h, prev, 100, 0.9, True)
            assert base[B + b][1] == nm and np.array_equal(base[B + b][0], m)
    if entry == "stereo":
        for p in range(B // 2):
            (kl, dl), (kr, dr) = refs[2 * p], refs[2 * p + 1]
            our, odp, okept = oracle_mod.compute_stereo_matches(oracle_mod.pyramid(frames[2 * p]),
                                                                oracle_mod.pyramid(frames[2 * p + 1]), kl, dl, kr, dr, bf, mb)
            ur, dp, kept = base[B + p]
            assert kept == okept and (kept > 0 or p == 1)   # (pair 1 is two unrelated frames)
            assert np.array_equal(ur.view(np.uint32), our.view(np.uint32)) and np.array_equal(dp.view(np.uint32), odp.view(np.uint32))
    for pitch, slack, off in _layouts(w):
        for fill in (255, 0):
            buf, stride = _padded(frames, pitch, slack, off, fill)
            dev = torch.from_numpy(buf).cuda()
            got = run(dev.data_ptr() + off, stride, pitch)
            what = f"{entry} pitch {pitch} stride {stride} offset {off} fill {fill}"
            for b in range(B):
                _same_output(*got[b], *base[b], f"{what} frame {b}")
            for g, t in zip(got[B:], base[B:]):
                assert all(np.array_equal(np.asarray(x).view(np.uint32) if np.asarray(x).dtype == np.float32 else x,
                                          np.asarray(y).view(np.uint32) if np.asarray(y).dtype == np.float32 else y)
                           for x, y in zip(g, t)), what
            assert torch.equal(dev.cpu(), torch.from_numpy(buf)), f"{what}: the input buffer was written"
    ex.close()
