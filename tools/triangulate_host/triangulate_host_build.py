"""Builds tools/triangulate_host/triangulate_host.cpp (orbx_triangulate.h's host
path) as a shared library and binds it with ctypes.  No device code is compiled
and none runs."""
import ctypes
import os
import subprocess
import tempfile
from pathlib import Path

ROOT = Path(__file__).resolve().parents[2]
P, I32 = ctypes.c_void_p, ctypes.c_int


def build(out: Path = None) -> Path:
    out = Path(out) if out is not None else Path(tempfile.mkdtemp(prefix="orbx_trihost_")) / "libtriangulate_host.so"
    out.parent.mkdir(parents=True, exist_ok=True)
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    subprocess.run([hipcc, "-x", "hip", "--offload-host-only", "-O3", "-std=c++17", "-ffp-contract=off", "-fPIC",
                    "-shared", "-Wall", f"-I{ROOT / 'orb_slam_2_ros_amd' / 'csrc'}",
                    str(ROOT / "tools" / "triangulate_host" / "triangulate_host.cpp"), "-o", str(out)], check=True)
    return out


def load(path: Path = None) -> ctypes.CDLL:
    lib = ctypes.CDLL(str(path if path is not None else build()))
    lib.triangulate_host_batch.argtypes = [P, P, P, P, P, I32, P, P]
    lib.triangulate_host_batch.restype = I32
    lib.triangulate_host_batch_unchecked.argtypes = [P, P, P, P, P, I32, I32, P]
    lib.triangulate_host_batch_unchecked.restype = I32
    lib.triangulate_host_svd.argtypes = [P, P]
    lib.triangulate_host_svd.restype = I32
    return lib
