"""ASan + UBSan on the host validation of orbx_triangulate(_batch), no GPU
needed and none used: orbx_triangulate.hip compiled with -Xarch_host
-fsanitize=address,undefined (the Makefile's sanitize object, device code
unchanged) and linked into a stand-alone program with its own main
(tests/cxx/san_triangulate_test.cpp), whose calls all return before the library
touches a device.  A sanitizer report makes the program exit non-zero."""
import os
import subprocess
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
HIPCC = "/opt/rocm/bin/hipcc"
ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:halt_on_error=1",
           UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")


def test_triangulate_validation_under_asan_ubsan(tmp_path):
    csrc = ROOT / "orb_slam_2_ros_amd" / "csrc"
    subprocess.run(["make", "-s", "-C", str(csrc), "_san/orbx_triangulate.o"], check=True, timeout=900)
    exe = tmp_path / "san_triangulate_test"
    subprocess.run([HIPCC, "--offload-arch=gfx950", "-O1", "-g", "-std=c++17", "-x", "c++", f"-I{ROOT / 'include'}",
                    "-Xarch_host", "-fsanitize=address", "-Xarch_host", "-fsanitize=undefined",
                    str(ROOT / "tests" / "cxx" / "san_triangulate_test.cpp"), "-x", "none",
                    str(csrc / "_san" / "orbx_triangulate.o"), "-o", str(exe)], check=True, timeout=600)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300, env=ENV)
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    assert "sanitize triangulate ok" in r.stdout and "runtime error" not in r.stderr
