"""Sim3-optimisation timing probe (k_sim3_optimize, orbx_sim3.hip):

  host-1xN          orbx_optimize_sim3 from Python, host arrays in and out
  device-PxN        orbx_optimize_sim3_batch_device on resident tensors, P in
                    {1, 64, 1024, 8192} problems of about N correspondences
  cpu-1xN           the same text compiled for the host (tools/sim3_host), one
                    thread, per problem: the project's restatement, not g2o

for N about 40 and about 150.  The device entries are timed with events around
`inner` back-to-back launches (no synchronisation inside), the host call and
the CPU figure with a host clock.  Each shape is warmed up, then `reps` windows
are timed; min / median / max are reported.  One JSON line per shape; the last
line repeats them as one record.

    python tools/sim3_probe.py [reps] [--out FILE] [--case NAME] [--label TEXT]

--label is copied into every line (which build of the library ORBX_LIB names,
for an A/B)."""
import ctypes
import json
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tools" / "sim3_host"))
from orb_slam_2_ros_amd._lib import ptr  # noqa: E402
from orb_slam_2_ros_amd.optimizer import (_sim3_batch_args, optimize_sim3, sim3_device_buffers,  # noqa: E402
                                          sim3_device_launch)
from orb_slam_2_ros_amd.synth_sim3 import SIM3_DTYPE, make_sim3_problem  # noqa: E402


def batch(nproblems, ncorr, distinct=16):
    """nproblems problems of ncorr +- 10 % correspondences, cycled from `distinct` synthetic candidates"""
    rng = np.random.default_rng(nproblems)
    base = [make_sim3_problem(int(ncorr * rng.uniform(0.9, 1.1)), seed=500 + k, outlier_frac=0.1,
                              fix_scale=bool(k % 2)) for k in range(distinct)]
    Ps = [base[p % distinct] for p in range(nproblems)]
    off = np.concatenate([[0], np.cumsum([len(P["corr"]) for P in Ps])]).astype(np.int32)
    return _sim3_batch_args(np.concatenate([P["S12"] for P in Ps]), np.concatenate([P["cam1"] for P in Ps]),
                            np.concatenate([P["cam2"] for P in Ps]), np.concatenate([P["corr"] for P in Ps]), off,
                            np.array([P["th2"] for P in Ps], np.float32),
                            np.array([P["fix_scale"] for P in Ps], np.int32))


def stats(ms):
    ms = sorted(ms)
    return {"min_ms": round(ms[0], 4), "median_ms": round(ms[len(ms) // 2], 4), "max_ms": round(ms[-1], 4)}


def device_case(name, nproblems, ncorr, reps, inner, warmup=3):
    import torch
    args = batch(nproblems, ncorr)
    st = torch.cuda.current_stream()
    ins, outs = sim3_device_buffers(*args, st.device)
    P, N = nproblems, len(args[3])
    for _ in range(warmup):
        sim3_device_launch(ins, outs, P, st)
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(inner):
            sim3_device_launch(ins, outs, P, st)
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1) / inner)
    its = outs[5].cpu().numpy()[:P]
    r = {"case": name, "problems": P, "correspondences": N, "launches_per_window": inner, "windows": reps,
         "lm_iterations_mean": round(float(its.sum(1).mean()), 2),
         "inliers_mean": round(float(outs[4][:P].float().mean()), 1), **stats(ms)}
    r["us_per_problem"] = round(1e3 * r["median_ms"] / P, 3)
    return r


def host_case(name, ncorr, reps, inner, warmup=5):
    P = make_sim3_problem(ncorr, seed=77, outlier_frac=0.1)
    call = lambda: optimize_sim3(P["S12"], P["cam1"], P["cam2"], P["corr"], P["th2"], P["fix_scale"])  # noqa: E731
    for _ in range(warmup):
        call()
    ms = []
    for _ in range(reps):
        t0 = time.perf_counter()
        for _ in range(inner):
            call()
        ms.append(1e3 * (time.perf_counter() - t0) / inner)
    return {"case": name, "problems": 1, "correspondences": ncorr, "launches_per_window": inner, "windows": reps,
            **stats(ms)}


def cpu_case(name, ncorr, reps, inner, lib):
    """The host compile of orbx_sim3.h on one thread, over the device batch's 16 distinct problems"""
    S, C1, C2, K, off, th, fix = batch(16, ncorr)
    So = np.zeros(1, SIM3_DTYPE)
    n_max = int(np.diff(off).max())
    rem, a, b = np.zeros(n_max + 1, np.uint8), np.zeros(n_max + 1), np.zeros(n_max + 1)
    ninl, its = ctypes.c_int(0), np.zeros(2, np.int32)

    def sweep():
        for p in range(16):
            lib.sim3_host_optimize(ptr(S[p:p + 1]), ptr(C1[p:p + 1]), ptr(C2[p:p + 1]), ptr(K[off[p]:off[p + 1]]),
                                   int(off[p + 1] - off[p]), float(th[p]), int(fix[p]), ptr(So), ptr(rem), ptr(a),
                                   ptr(b), ctypes.byref(ninl), ptr(its))
    sweep()
    ms = []
    for _ in range(reps):
        t0 = time.perf_counter()
        for _ in range(inner):
            sweep()
        ms.append(1e3 * (time.perf_counter() - t0) / (16 * inner))
    r = {"case": name, "problems": 1, "correspondences": int(len(K) / 16), "threads": 1,
         "what": "orbx_sim3.h compiled for the host: the project's restatement, not g2o", "windows": reps,
         **stats(ms)}
    r["us_per_problem"] = round(1e3 * r["median_ms"], 3)
    return r


def main():
    args = [a for a in sys.argv[1:]]
    opts = {}
    for flag in ("--out", "--case", "--label"):
        if flag in args:
            i = args.index(flag)
            opts[flag] = args[i + 1]
            del args[i:i + 2]
    reps = int(args[0]) if args else 9
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("sim3_probe: no GPU (timings are taken on the device only)")
    import sim3_host_build as host_build
    lib = host_build.load()
    cases = {}
    for n in (40, 150):
        cases[f"host-1x{n}"] = lambda n=n: host_case(f"host-1x{n}", n, reps, inner=50)
        for P in (1, 64, 1024, 8192):
            cases[f"device-{P}x{n}"] = lambda n=n, P=P: device_case(f"device-{P}x{n}", P, n, reps,
                                                                    inner=20 if P < 8192 else 5)
        cases[f"cpu-1x{n}"] = lambda n=n: cpu_case(f"cpu-1x{n}", n, reps, 3, lib)
    only = opts.get("--case")
    if only is not None and only not in cases:
        raise SystemExit(f"sim3_probe: --case is one of {list(cases)}")
    res = [run() for name, run in cases.items() if only in (None, name)]
    if "--label" in opts:
        res = [{"build": opts["--label"], **r} for r in res]
    lines = [json.dumps(r) for r in res] + [json.dumps({"sim3_probe": res, "device": torch.cuda.get_device_name(0)})]
    print("\n".join(lines))
    if "--out" in opts:
        out = Path(opts["--out"])
        out.parent.mkdir(parents=True, exist_ok=True)
        out.write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
