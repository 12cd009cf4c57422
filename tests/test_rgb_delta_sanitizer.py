"""CPU: the host half of the RGB(A) delta call under AddressSanitizer + UBSan.

tests/host/rgb_delta_sanitize.cpp is a stand-alone program (its own main, no GPU, no HIP) that drives csrc/srcnn_rgb_delta.hpp --
the span tables of an RGB(A) tile grid and the items that srcnn_rgb_delta_flags_dev, srcnn_rgb_delta_rects and
srcnn_rgb_upscale_delta_dev run -- over the grid, the coalescer and the monotonicity gate of csrc/srcnn_delta.hpp.  It asserts that
every tile's span, built from one pair of tables per axis, is the union srcnn_rgb_rect_source computes for that tile alone (all five
filters; 2x, 2.5x, 1.5x, the identity size, one axis that keeps its size, a down-scale), that the spans are monotone and the
kernel's bisection over them finds exactly the tiles whose span holds a source pixel, and that the items point at pixel (x0, y0) of
the full-size image for every bytes-per-pixel class.  It is built here exactly as tests/test_delta_sanitizer.py builds its program
and run as a process of its own; nothing of it is loaded into Python."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_rgb_delta_host_code_under_asan_and_ubsan(tmp_path):
    if not shutil.which("g++"):
        pytest.skip("no host toolchain")
    exe = str(tmp_path / "rgb_delta_asan")
    r = subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                        "-fno-omit-frame-pointer", os.path.join(ROOT, "tests", "host", "rgb_delta_sanitize.cpp"), "-lm", "-o", exe],
                       capture_output=True, text=True, timeout=600)
    if r.returncode != 0 and ("cannot find -lasan" in r.stderr or "libasan" in r.stderr and "No such file" in r.stderr):
        pytest.skip("sanitizer runtime not installed: " + r.stderr[-200:])
    assert r.returncode == 0, r.stderr[-4000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:alloc_dealloc_mismatch=1:strict_string_checks=1", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "all checks passed" in r.stdout
