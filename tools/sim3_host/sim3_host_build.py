"""Builds tools/sim3_host/sim3_host.cpp (orbx_sim3.h's host path) as a shared
library and binds it with ctypes.  No device code is compiled and none runs."""
import ctypes
import os
import subprocess
import tempfile
from pathlib import Path

ROOT = Path(__file__).resolve().parents[2]
P, I32, F32, F64 = ctypes.c_void_p, ctypes.c_int, ctypes.c_float, ctypes.c_double


def build(out: Path = None) -> Path:
    out = Path(out) if out is not None else Path(tempfile.mkdtemp(prefix="orbx_sim3host_")) / "libsim3_host.so"
    out.parent.mkdir(parents=True, exist_ok=True)
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    subprocess.run([hipcc, "-x", "hip", "--offload-host-only", "-O3", "-std=c++17", "-ffp-contract=off", "-fPIC",
                    "-shared", "-Wall", f"-I{ROOT / 'orb_slam_2_ros_amd' / 'csrc'}",
                    str(ROOT / "tools" / "sim3_host" / "sim3_host.cpp"), "-o", str(out)], check=True)
    return out


def load(path: Path = None) -> ctypes.CDLL:
    lib = ctypes.CDLL(str(path if path is not None else build()))
    lib.sim3_host_optimize.argtypes = [P, P, P, P, I32, F32, I32, P, P, P, P, P, P]
    lib.sim3_host_step.argtypes = [P, P, P, P, I32, F32, I32, P, I32, F64, P, P, P, P, P]
    lib.sim3_host_update.argtypes = [P, P, I32, I32, P]
    lib.sim3_host_exp.argtypes = [P, P]
    lib.sim3_host_perturbation.argtypes = [I32, I32, P]
    for f in (lib.sim3_host_optimize, lib.sim3_host_step, lib.sim3_host_update):
        f.restype = I32
    lib.sim3_host_exp.restype = None
    lib.sim3_host_perturbation.restype = None
    return lib
