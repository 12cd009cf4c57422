"""CPU: the Y path's geometry header under AddressSanitizer + UBSan.

tests/host/y_path_geom_sanitize.cpp is a stand-alone program (its own main, no GPU, no HIP) that drives
csrc/srcnn_y_path_geom.hpp -- the halo of an output range, the source span of a range of a resampled axis, the size limits and the
band decision that every frame, rect, rect-list and delta entry point goes through.  It holds y_path_halo against set dilation for
every range of every axis up to 24 long, taps_span against a literal min / max over the tables of all five filters (up-scales, a
down-scale, an axis that keeps its size), y_path_band_rows against the rule as the call sites used to spell it (the exact fit, one
byte short, the 16-row floor, the fused tier, fewer rows than the band, and a sweep of budgets around each), and y_path_fits at
every limit and one past it.  It is built here exactly as tests/test_delta_sanitizer.py builds its program and run as a process of
its own; nothing of it is loaded into Python."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_y_path_geometry_under_asan_and_ubsan(tmp_path):
    if not shutil.which("g++"):
        pytest.skip("no host toolchain")
    exe = str(tmp_path / "y_path_geom_asan")
    r = subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                        "-fno-omit-frame-pointer", os.path.join(ROOT, "tests", "host", "y_path_geom_sanitize.cpp"), "-lm", "-o", exe],
                       capture_output=True, text=True, timeout=600)
    if r.returncode != 0 and ("cannot find -lasan" in r.stderr or "libasan" in r.stderr and "No such file" in r.stderr):
        pytest.skip("sanitizer runtime not installed: " + r.stderr[-200:])
    assert r.returncode == 0, r.stderr[-4000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:alloc_dealloc_mismatch=1:strict_string_checks=1", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "all checks passed" in r.stdout
