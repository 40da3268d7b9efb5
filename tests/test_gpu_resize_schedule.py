"""k_resize_d's two row schedules against the oracle's pyramid, byte for byte.

A row of wave tiles is phase-uniform when every lane group's 10 rows lie inside
the level, no source row is clamped and the groups' source rows advance by one
shared sequence (orbx_plan.h, ResizeTileRow); such tiles take the row schedule
as scalars, every other tile keeps the per-lane schedule, and
ORBX_RESIZE_UNIFORM=0 keeps it for all.  The classes each size must give are
recomputed here from cv::resize's row arithmetic and compared with the plan's
counters, so a run cannot pass by not reaching a path."""
import numpy as np
import pytest

import extract_cases as ec
from orb_slam_2_ros_amd import ORBextractor, synth
from orb_slam_2_ros_amd._lib import debug_counter

pytestmark = pytest.mark.gpu

K = 10   # kResizeK: output rows per lane


def _first_diff(a, b):
    idx = np.nonzero(a != b)
    return tuple(int(i[0]) for i in idx) if len(idx[0]) else None


def _src_rows(hs, hd):
    """First source row of every output row (cv::resize INTER_LINEAR, before clamping)."""
    scale = 1.0 / (hd / hs)
    return np.floor(((np.arange(hd) + 0.5) * scale - 0.5).astype(np.float32)).astype(np.int64)


def _tile_shape(w):
    """(tile width, tile height): the column count in {256, 128, 64} wasting the fewest columns, wider on ties."""
    best = None
    for sh in (6, 5, 4):
        cols = 4 << sh
        n = -(-w // cols)
        if best is None or n * cols < best[0]:
            best = (n * cols, sh)
    return 4 << best[1], (64 >> best[1]) * K


def _classes(sizes):
    """Per level >= 1: (tiles a row, [tile row is phase-uniform], tail column groups?, partial last tile row?)."""
    out = []
    for (ws, hs), (w, h) in zip(sizes[:-1], sizes[1:]):
        tw, th = _tile_shape(w)
        src = _src_rows(hs, h)
        rows = []
        for y0 in range(0, h, th):
            uni = y0 + th <= h
            if uni:
                s = src[y0:y0 + th]
                uni = s.min() >= 0 and s.max() + 1 <= hs - 1
                rel = (s.reshape(-1, K) - s.reshape(-1, K)[:, :1])
                uni = uni and (rel == rel[0]).all() and (np.diff(rel[0]) >= 1).all()
            rows.append(bool(uni))
        out.append((-(-w // tw), rows, w % 16 != 0, h % th != 0))
    return out


def _expected(sizes):
    cl = _classes(sizes)
    return (sum(ntx * sum(rows) for ntx, rows, _, _ in cl), sum(ntx * (len(rows) - sum(rows)) for ntx, rows, _, _ in cl))


def _sizes(oracle_mod, w, h, nlev):
    lw, lh, _, _ = oracle_mod.levels(w, h, 500, 1.2, nlev)
    return [(int(a), int(b)) for a, b in zip(lw, lh)]


def _frames(w, h, B, seed):
    # synthetic texture, then uniform noise: every byte value next to every other
    fr = [synth.frame(w, h, seed + b) if b % 2 == 0 else ec.uniform(w, h, seed + b) for b in range(B)]
    return np.ascontiguousarray(np.stack(fr))


@pytest.fixture(scope="module")
def refs(oracle_mod):
    """The oracle's pyramids, once per (size, batch, levels)."""
    cache = {}

    def get(w, h, B, nlev, seed):
        key = (w, h, B, nlev, seed)
        if key not in cache:
            fr = _frames(w, h, B, seed)
            cache[key] = fr, [oracle_mod.pyramid(f, 1.2, nlev) for f in fr]
        return cache[key]
    return get


def _check_levels(ex, pyrs, nlev, what):
    for b, pyr in enumerate(pyrs):
        for l in range(nlev):
            gp = ex.debug_fetch(b, l, 0)
            assert gp.shape == pyr[l].shape and np.array_equal(gp, pyr[l]), \
                f"{what}: frame {b} pyramid level {l} differs at {_first_diff(gp, pyr[l])}"


def _extractor(monkeypatch, nlev, forced):
    monkeypatch.setenv("ORBX_PYR_RGN", "0")   # the per-level kernels at every batch
    if forced:
        monkeypatch.setenv("ORBX_RESIZE_UNIFORM", "0")
    else:
        monkeypatch.delenv("ORBX_RESIZE_UNIFORM", raising=False)
    return ORBextractor(500, 1.2, nlev, 20, 7)


def _check_counters(sizes, forced, what):
    uni, fb = _expected(sizes)
    got = debug_counter("resize_uniform_tiles"), debug_counter("resize_fallback_tiles")
    assert got == ((0, uni + fb) if forced else (uni, fb)), f"{what}: tiles (uniform, fallback) {got}, expected from the row arithmetic {(uni, fb)}"


# (w, h, B, nlevels, what the size is here for)
CASES = [
    (640, 480, 3, 8, "mixed"),
    (333, 250, 2, 8, "mixed partial"),
    (752, 480, 2, 8, "mixed"),
    (752, 480, 2, 3, "mixed"),
    (400, 300, 2, 8, "tail64"),      # level 1 is 333 wide: 13 columns past column 320
    (384, 288, 2, 2, "notail"),      # level 1 is 320 x 240: no scalar-tail column
    (640, 480, 2, 2, "all"),         # level 1 alone: 480 / 400 = 1.2 exactly
]


@pytest.mark.parametrize("forced", [False, True], ids=["default", "fallback"])
@pytest.mark.parametrize("w,h,B,nlev,kind", CASES, ids=[f"{c[0]}x{c[1]}-{c[3]}-{c[4].replace(' ', '_')}" for c in CASES])
def test_resize_schedule_sizes(w, h, B, nlev, kind, forced, refs, oracle_mod, monkeypatch):
    import torch
    sizes = _sizes(oracle_mod, w, h, nlev)
    cl = _classes(sizes)
    uni, fb = _expected(sizes)
    # the size holds what it is here for
    if "mixed" in kind:
        assert uni > 0 and fb > 0, (uni, fb)
    if "partial" in kind:
        assert any(part for _, _, _, part in cl), cl
    if kind == "tail64":
        assert any(1 <= sw % 64 <= 15 and tail for (sw, _), (_, _, tail, _) in zip(sizes[1:], cl)), sizes
    if kind == "notail":
        assert not any(tail for _, _, tail, _ in cl) and uni > 0, (sizes, cl)
    if kind == "all":
        assert fb == 0 and all(cl[0][1]) and uni == cl[0][0] * len(cl[0][1]), cl
    if (w, h, nlev) == (640, 480, 8):
        assert all(cl[0][1]), "every level-1 tile row of 640 x 480 is phase-uniform"
    fr, pyrs = refs(w, h, B, nlev, 700 + w)
    ex = _extractor(monkeypatch, nlev, forced)
    ex.reserve(w, h, B)
    _check_counters(sizes, forced, f"{w} x {h}")
    dev = torch.from_numpy(fr).cuda()
    ex.extract_batch_device(dev.data_ptr(), w * h, w, B)
    torch.cuda.synchronize()
    _check_levels(ex, pyrs, nlev, f"{w} x {h} {'fallback' if forced else 'default'}")
    ex.close()


@pytest.mark.parametrize("forced", [False, True], ids=["default", "fallback"])
def test_resize_schedule_padded(forced, refs, oracle_mod, monkeypatch):
    """333 x 250 at an odd pitch (repacked on the device) and at a padded
    pitch of a multiple of 4 from an offset base (read in place: level 1's
    source pitch is then the caller's), the padding full of 255."""
    import torch
    w, h, B, nlev = 333, 250, 2, 8
    fr, pyrs = refs(w, h, B, nlev, 700 + w)
    sizes = _sizes(oracle_mod, w, h, nlev)
    ex = _extractor(monkeypatch, nlev, forced)
    ex.reserve(w, h, B)
    _check_counters(sizes, forced, "padded")
    for pitch, slack, off in [(w + 1, 37, 0), ((w + 64 + 3) & ~3, 40, 4)]:
        stride = pitch * h + slack
        buf = np.full(off + B * stride + 64, 255, np.uint8)
        for b in range(B):
            buf[off + b * stride: off + b * stride + pitch * h].reshape(h, pitch)[:, :w] = fr[b]
        dev = torch.from_numpy(buf).cuda()
        ex.extract_batch_device(dev.data_ptr() + off, stride, pitch, B)
        torch.cuda.synchronize()
        _check_levels(ex, pyrs, nlev, f"pitch {pitch} offset {off}")
    ex.close()


@pytest.mark.parametrize("forced", [False, True], ids=["default", "fallback"])
@pytest.mark.parametrize("pipeline", [0, 2])
def test_resize_schedule_mono_step(pipeline, forced, refs, oracle_mod, monkeypatch):
    """The batched mono step launches the same kernel per level, in one
    stream (pipeline 0) or level-pipelined on internal streams (2)."""
    import torch
    w, h, B, nlev = 333, 250, 2, 8
    fr, pyrs = refs(w, h, B, nlev, 700 + w)
    sizes = _sizes(oracle_mod, w, h, nlev)
    ex = _extractor(monkeypatch, nlev, forced)
    ex.reserve(w, h, B)
    ex.split(1)
    assert ex.pipeline(pipeline) == pipeline
    _check_counters(sizes, forced, "mono step")
    dev = torch.from_numpy(fr).cuda()
    for _ in range(2):
        ex.mono_step_device(dev.data_ptr(), w * h, w, B)
    torch.cuda.synchronize()
    _check_levels(ex, pyrs, nlev, f"mono step, pipeline {pipeline}")
    ex.close()
