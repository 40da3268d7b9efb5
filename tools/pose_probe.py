"""Pose-optimisation timing probe (k_pose_optimize, orbx_pose.hip):

  device-3072x300   orbx_pose_optimization_batch_device on resident tensors,
                    3072 problems of ~300 observations (the tracking batch)
  device-128x1000   the same, 128 problems of ~1000 observations
  host-1x300        orbx_pose_optimization from Python, host arrays in and out

The device entries are timed with events around `inner` back-to-back launches
(no synchronisation inside), the host call with a host clock (it ends in a
stream synchronise).  Each shape is warmed up, then `reps` windows are timed;
min / median / max are reported.  One JSON line per shape; the last line
repeats them as one record.

    python tools/pose_probe.py [reps] [--out FILE] [--case NAME]

--case runs one shape alone (a counter pass under rocprofv3 --pmc, read with
tools/pmc_table.py)."""
import json
import sys
import time
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
from orb_slam_2_ros_amd._lib import check, load  # noqa: E402
from orb_slam_2_ros_amd.optimizer import pose_optimization  # noqa: E402
from orb_slam_2_ros_amd.synth_pose import POSE_CAM_DTYPE, make_pose_problem  # noqa: E402


def batch(nproblems, nobs, distinct=16):
    """nproblems problems of nobs +- 10 % observations, cycled from `distinct` synthetic frames"""
    rng = np.random.default_rng(nproblems)
    base = [make_pose_problem(int(nobs * rng.uniform(0.9, 1.1)), seed=500 + k) for k in range(distinct)]
    Ps = [base[p % distinct] for p in range(nproblems)]
    T = np.stack([P["Tcw"] for P in Ps])
    C = np.concatenate([P["cam"] for P in Ps])
    O = np.concatenate([P["obs"] for P in Ps])
    off = np.concatenate([[0], np.cumsum([len(P["obs"]) for P in Ps])]).astype(np.int32)
    return T, C, O, off


def stats(ms):
    ms = sorted(ms)
    return {"min_ms": round(ms[0], 4), "median_ms": round(ms[len(ms) // 2], 4), "max_ms": round(ms[-1], 4)}


def device_case(name, nproblems, nobs, reps, inner, warmup=3):
    import torch
    T, C, O, off = batch(nproblems, nobs)
    Cf = np.stack([C[k] for k in POSE_CAM_DTYPE.names], 1).astype(np.float32)
    Of = np.ascontiguousarray(O).view(np.float32).reshape(-1, 7)
    dT, dC, dO, doff = (torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in (T, Cf, Of, off))
    P, N = len(T), len(O)
    dTo = torch.empty_like(dT)
    dout = torch.empty(N, dtype=torch.uint8, device="cuda")
    dchi = torch.empty(N, dtype=torch.float64, device="cuda")
    dn = torch.empty(P, dtype=torch.int32, device="cuda")
    dit = torch.empty((P, 4), dtype=torch.int32, device="cuda")
    fn = load().orbx_pose_optimization_batch_device
    st = torch.cuda.current_stream().cuda_stream

    def launch():
        check(fn(dT.data_ptr(), dC.data_ptr(), dO.data_ptr(), doff.data_ptr(), P, dTo.data_ptr(), dout.data_ptr(),
                 dchi.data_ptr(), dn.data_ptr(), dit.data_ptr(), st), name)

    for _ in range(warmup):
        launch()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(inner):
            launch()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1) / inner)
    its = dit.cpu().numpy()
    r = {"case": name, "problems": P, "observations": N, "launches_per_window": inner, "windows": reps,
         "lm_iterations_mean": round(float(its.sum(1).mean()), 2), "inliers_mean": round(float(dn.float().mean()), 1),
         **stats(ms)}
    r["us_per_problem"] = round(1e3 * r["median_ms"] / P, 3)
    return r


def host_case(name, nobs, reps, inner, warmup=5):
    P = make_pose_problem(nobs, seed=77)
    for _ in range(warmup):
        pose_optimization(P["Tcw"], P["cam"], P["obs"])
    ms = []
    for _ in range(reps):
        t0 = time.perf_counter()
        for _ in range(inner):
            pose_optimization(P["Tcw"], P["cam"], P["obs"])
        ms.append(1e3 * (time.perf_counter() - t0) / inner)
    return {"case": name, "problems": 1, "observations": nobs, "launches_per_window": inner, "windows": reps,
            **stats(ms)}


def main():
    args = [a for a in sys.argv[1:]]
    out = None
    if "--out" in args:
        i = args.index("--out")
        out = Path(args[i + 1])
        del args[i:i + 2]
    only = None
    if "--case" in args:
        i = args.index("--case")
        only = args[i + 1]
        del args[i:i + 2]
    reps = int(args[0]) if args else 9
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("pose_probe: no GPU (timings are taken on the device only)")
    cases = {"device-3072x300": lambda: device_case("device-3072x300", 3072, 300, reps, inner=20),
             "device-128x1000": lambda: device_case("device-128x1000", 128, 1000, reps, inner=20),
             "host-1x300": lambda: host_case("host-1x300", 300, reps, inner=50)}
    if only is not None and only not in cases:
        raise SystemExit(f"pose_probe: --case is one of {list(cases)}")
    res = [run() for name, run in cases.items() if only in (None, name)]
    lines = [json.dumps(r) for r in res] + [json.dumps({"pose_probe": res, "device": torch.cuda.get_device_name(0)})]
    print("\n".join(lines))
    if out:
        out.parent.mkdir(parents=True, exist_ok=True)
        out.write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
