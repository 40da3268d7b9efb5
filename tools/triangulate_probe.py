"""CreateNewMapPoints triangulation timing probe (k_triangulate, orbx_triangulate.hip):

  host-20x150       one keyframe: 20 neighbours of about 150 pairs through
                    orbx_triangulate_batch from Python, host arrays in and out
  device-PxN        orbx_triangulate_batch_device on resident tensors, P in
                    {20, 160, 1280} problems of about N = 150 pairs
  cpu-20x150        the same text compiled for the host (tools/triangulate_host,
                    -O3 -ffp-contract=off), one thread: the project's
                    restatement, not OpenCV's cv::Mat code

The device entries are timed with events around `inner` back-to-back launches
(no synchronisation inside), the host call and the CPU figure with a host
clock.  Each shape is warmed up, then `reps` windows are timed; min / median /
max are reported.  One JSON line per shape; the last line repeats them as one
record.

    python tools/triangulate_probe.py [reps] [--out FILE] [--case NAME]"""
import json
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tools" / "triangulate_host"))
from orb_slam_2_ros_amd._lib import ptr  # noqa: E402
from orb_slam_2_ros_amd.synth_triangulate import make_triangulation_problem  # noqa: E402
from orb_slam_2_ros_amd.triangulate import (TRI_POINT_DTYPE, _batch_args, triangulate_batch,  # noqa: E402
                                            triangulate_device_buffers, triangulate_device_launch)

PAIRS = 150


def batch(nproblems, distinct=20):
    """nproblems neighbours of PAIRS +- 10 % pairs, cycled from `distinct` synthetic ones (a third stereo)"""
    rng = np.random.default_rng(1)
    base = [make_triangulation_problem(int(PAIRS * rng.uniform(0.9, 1.1)), seed=800 + k, stereo_frac=0.3 * (k % 3 == 0),
                                       outlier_frac=0.2) for k in range(distinct)]
    Ps = [base[p % distinct] for p in range(nproblems)]
    off = np.concatenate([[0], np.cumsum([len(P["pairs"]) for P in Ps])]).astype(np.int32)
    return _batch_args(np.concatenate([P["v1"] for P in Ps]), np.concatenate([P["v2"] for P in Ps]),
                       np.array([P["ratio_factor"] for P in Ps], np.float32),
                       np.concatenate([P["pairs"] for P in Ps]), off)


def stats(ms):
    ms = sorted(ms)
    return {"min_ms": round(ms[0], 4), "median_ms": round(ms[len(ms) // 2], 4), "max_ms": round(ms[-1], 4)}


def device_case(name, nproblems, reps, inner, warmup=3):
    import torch
    args = batch(nproblems)
    N = len(args[3])
    st = torch.cuda.current_stream()
    ins, out = triangulate_device_buffers(*args, st.device)
    for _ in range(warmup):
        triangulate_device_launch(ins, out, nproblems, N, st)
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(inner):
            triangulate_device_launch(ins, out, nproblems, N, st)
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1) / inner)
    pts = np.frombuffer(out.cpu().numpy().tobytes(), TRI_POINT_DTYPE)[:N]
    r = {"case": name, "problems": nproblems, "pairs": N, "launches_per_window": inner, "windows": reps,
         "created": int((pts["status"] == 0).sum()), **stats(ms)}
    r["ns_per_pair"] = round(1e6 * r["median_ms"] / N, 2)
    return r


def host_case(name, nproblems, reps, inner, warmup=5):
    args = batch(nproblems)
    for _ in range(warmup):
        triangulate_batch(*args)
    ms = []
    for _ in range(reps):
        t0 = time.perf_counter()
        for _ in range(inner):
            triangulate_batch(*args)
        ms.append(1e3 * (time.perf_counter() - t0) / inner)
    return {"case": name, "problems": nproblems, "pairs": len(args[3]), "launches_per_window": inner,
            "windows": reps, **stats(ms)}


def cpu_case(name, nproblems, reps, inner, lib):
    V1, V2, rf, K, off = batch(nproblems)
    out = np.zeros(len(K), TRI_POINT_DTYPE)

    def sweep():
        lib.triangulate_host_batch(ptr(V1), ptr(V2), ptr(rf), ptr(K), ptr(off), nproblems, ptr(out), None)
    sweep()
    ms = []
    for _ in range(reps):
        t0 = time.perf_counter()
        for _ in range(inner):
            sweep()
        ms.append(1e3 * (time.perf_counter() - t0) / inner)
    r = {"case": name, "problems": nproblems, "pairs": len(K), "threads": 1,
         "what": "orbx_triangulate.h compiled for the host: the project's restatement, not OpenCV",
         "windows": reps, "created": int((out["status"] == 0).sum()), **stats(ms)}
    r["ns_per_pair"] = round(1e6 * r["median_ms"] / len(K), 2)
    return r


def main():
    args = [a for a in sys.argv[1:]]
    opts = {}
    for flag in ("--out", "--case"):
        if flag in args:
            i = args.index(flag)
            opts[flag] = args[i + 1]
            del args[i:i + 2]
    reps = int(args[0]) if args else 9
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("triangulate_probe: no GPU (timings are taken on the device only)")
    import triangulate_host_build as host_build
    lib = host_build.load()
    cases = {"host-20x150": lambda: host_case("host-20x150", 20, reps, inner=50)}
    for P in (20, 160, 1280):
        cases[f"device-{P}x150"] = lambda P=P: device_case(f"device-{P}x150", P, reps, inner=20)
    cases["cpu-20x150"] = lambda: cpu_case("cpu-20x150", 20, reps, 5, lib)
    only = opts.get("--case")
    if only is not None and only not in cases:
        raise SystemExit(f"triangulate_probe: --case is one of {list(cases)}")
    res = [run() for name, run in cases.items() if only in (None, name)]
    lines = [json.dumps(r) for r in res] + [json.dumps({"triangulate_probe": res,
                                                        "device": torch.cuda.get_device_name(0)})]
    print("\n".join(lines))
    if "--out" in opts:
        out = Path(opts["--out"])
        out.parent.mkdir(parents=True, exist_ok=True)
        out.write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
