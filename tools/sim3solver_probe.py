"""Sim3Solver timing probe (k_sim3_ransac, orbx_sim3_ransac.hip):

  host-1xN          orbx_sim3_ransac from Python, host arrays in and out
  device-PxN        orbx_sim3_ransac_batch_device on resident tensors, P in
                    {1, 8, 64} solvers of about N correspondences
  cpu-1xN           the same text compiled for the host (tools/sim3solver_host,
                    -O3 -ffp-contract=off), one thread, per solver: the
                    project's restatement, not OpenCV's cv::Mat code

for N about 40 and about 150, 300 hypotheses per solver.  The device entries
are timed with events around `inner` back-to-back launches (no synchronisation
inside), the host call and the CPU figure with a host clock.  Each shape is
warmed up, then `reps` windows are timed; min / median / max are reported.
One JSON line per shape; the last line repeats them as one record.

    python tools/sim3solver_probe.py [reps] [--out FILE] [--case NAME]"""
import json
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tools" / "sim3solver_host"))
from orb_slam_2_ros_amd._lib import ptr  # noqa: E402
from orb_slam_2_ros_amd.sim3solver import (RANSAC_HYP_DTYPE, _batch_args, draw_triples, ransac_device_buffers,  # noqa: E402
                                           ransac_device_launch, sim3_ransac)
from orb_slam_2_ros_amd.synth_sim3solver import make_sim3solver_problem  # noqa: E402

HYPS = 300


def problem(ncorr, seed):
    rng = np.random.default_rng(seed)
    P = make_sim3solver_problem(int(ncorr * rng.uniform(0.9, 1.1)), seed=seed, outlier_frac=0.3, noise_m=0.002,
                                scale=1.1, fix_scale=bool(seed % 2))
    P["triples"] = draw_triples(len(P["corr"]), HYPS, lambda lo, hi: int(rng.integers(lo, hi + 1)))
    return P


def batch(nproblems, ncorr, distinct=8):
    """nproblems solvers of ncorr +- 10 % correspondences, cycled from `distinct` synthetic candidates"""
    base = [problem(ncorr, 700 + k) for k in range(distinct)]
    Ps = [base[p % distinct] for p in range(nproblems)]
    co = np.concatenate([[0], np.cumsum([len(P["corr"]) for P in Ps])]).astype(np.int32)
    ho = (HYPS * np.arange(nproblems + 1)).astype(np.int32)
    return _batch_args(np.concatenate([P["cam1"] for P in Ps]), np.concatenate([P["cam2"] for P in Ps]),
                       np.array([P["fix_scale"] for P in Ps], np.int32), np.concatenate([P["corr"] for P in Ps]), co,
                       np.concatenate([P["triples"] for P in Ps]), ho)


def stats(ms):
    ms = sorted(ms)
    return {"min_ms": round(ms[0], 4), "median_ms": round(ms[len(ms) // 2], 4), "max_ms": round(ms[-1], 4)}


def device_case(name, nproblems, ncorr, reps, inner, warmup=3):
    import torch
    args = batch(nproblems, ncorr)
    st = torch.cuda.current_stream()
    ins, outs = ransac_device_buffers(*args, st.device)
    for _ in range(warmup):
        ransac_device_launch(ins, outs, nproblems, HYPS, st)
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(inner):
            ransac_device_launch(ins, outs, nproblems, HYPS, st)
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1) / inner)
    hyp = np.frombuffer(outs[0].cpu().numpy().tobytes(), RANSAC_HYP_DTYPE)[:HYPS * nproblems]
    r = {"case": name, "problems": nproblems, "correspondences": len(args[3]), "hypotheses": HYPS * nproblems,
         "launches_per_window": inner, "windows": reps, "best_inliers_mean":
         round(float(hyp["n_inliers"].reshape(nproblems, HYPS).max(1).mean()), 1), **stats(ms)}
    r["us_per_problem"] = round(1e3 * r["median_ms"] / nproblems, 3)
    r["ns_per_hypothesis"] = round(1e6 * r["median_ms"] / (HYPS * nproblems), 2)
    return r


def host_case(name, ncorr, reps, inner, warmup=5):
    P = problem(ncorr, 77)
    call = lambda: sim3_ransac(P["cam1"], P["cam2"], P["fix_scale"], P["corr"], P["triples"])  # noqa: E731
    for _ in range(warmup):
        call()
    ms = []
    for _ in range(reps):
        t0 = time.perf_counter()
        for _ in range(inner):
            call()
        ms.append(1e3 * (time.perf_counter() - t0) / inner)
    return {"case": name, "problems": 1, "correspondences": len(P["corr"]), "hypotheses": HYPS,
            "launches_per_window": inner, "windows": reps, **stats(ms)}


def cpu_case(name, ncorr, reps, inner, lib):
    """The host compile of orbx_horn.h on one thread, over the device batch's 8 distinct solvers"""
    Ps = [problem(ncorr, 700 + k) for k in range(8)]
    n_max = max(len(P["corr"]) for P in Ps)
    hyp, mask = np.zeros(HYPS, RANSAC_HYP_DTYPE), np.zeros(HYPS * ((n_max + 63) // 64), np.uint64)

    def sweep():
        for P in Ps:
            lib.sim3solver_host_ransac(ptr(P["cam1"]), ptr(P["cam2"]), int(P["fix_scale"]), ptr(P["corr"]),
                                       len(P["corr"]), ptr(P["triples"]), HYPS, ptr(hyp), ptr(mask))
    sweep()
    ms = []
    for _ in range(reps):
        t0 = time.perf_counter()
        for _ in range(inner):
            sweep()
        ms.append(1e3 * (time.perf_counter() - t0) / (8 * inner))
    r = {"case": name, "problems": 1, "correspondences": int(sum(len(P["corr"]) for P in Ps) / 8), "hypotheses": HYPS,
         "threads": 1, "what": "orbx_horn.h compiled for the host: the project's restatement, not OpenCV",
         "windows": reps, **stats(ms)}
    r["us_per_problem"] = round(1e3 * r["median_ms"], 3)
    r["ns_per_hypothesis"] = round(1e6 * r["median_ms"] / HYPS, 2)
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
        raise SystemExit("sim3solver_probe: no GPU (timings are taken on the device only)")
    import sim3solver_host_build as host_build
    lib = host_build.load()
    cases = {}
    for n in (40, 150):
        cases[f"host-1x{n}"] = lambda n=n: host_case(f"host-1x{n}", n, reps, inner=50)
        for P in (1, 8, 64):
            cases[f"device-{P}x{n}"] = lambda n=n, P=P: device_case(f"device-{P}x{n}", P, n, reps, inner=20)
        cases[f"cpu-1x{n}"] = lambda n=n: cpu_case(f"cpu-1x{n}", n, reps, 5, lib)
    only = opts.get("--case")
    if only is not None and only not in cases:
        raise SystemExit(f"sim3solver_probe: --case is one of {list(cases)}")
    res = [run() for name, run in cases.items() if only in (None, name)]
    lines = [json.dumps(r) for r in res] + [json.dumps({"sim3solver_probe": res,
                                                        "device": torch.cuda.get_device_name(0)})]
    print("\n".join(lines))
    if "--out" in opts:
        out = Path(opts["--out"])
        out.parent.mkdir(parents=True, exist_ok=True)
        out.write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
