"""CPU: the host half of the delta call under AddressSanitizer + UBSan.

tests/host/delta_sanitize.cpp is a stand-alone program (its own main, no GPU, no HIP) that drives csrc/srcnn_delta.hpp -- the grid,
the span-table builder, the coalescer and the whole-frame rule that srcnn_y_path_delta_grid, srcnn_y_path_delta_flags_dev,
srcnn_y_path_delta_rects and srcnn_y_path_delta_f32_dev all run.  It asserts that every tile's span, built from one table per axis,
is the rectangle y_path_rect_source_span gives for that tile alone (all five filters; the grids of the issue, a 2.5x frame, axes
that keep their size, a down-scale, a steep up-scale), that the spans are monotone and the kernel's bisection over them finds
exactly the tiles whose span holds a source sample, that the coalescer's rects are disjoint, cover exactly the dirty tiles clipped
to the frame and follow the one rule (hand cases, seeded grids, degenerate grids: 1 x 1, a 1-tile column, a 1-tile row), that a
capacity one short writes no item, and every clause of the whole-frame rule.  It is built here exactly as
tests/test_yuv_rect_list_sanitizer.py builds its program and run as a process of its own; nothing of it is loaded into Python."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_delta_host_code_under_asan_and_ubsan(tmp_path):
    if not shutil.which("g++"):
        pytest.skip("no host toolchain")
    exe = str(tmp_path / "delta_asan")
    r = subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                        "-fno-omit-frame-pointer", os.path.join(ROOT, "tests", "host", "delta_sanitize.cpp"), "-lm", "-o", exe],
                       capture_output=True, text=True, timeout=600)
    if r.returncode != 0 and ("cannot find -lasan" in r.stderr or "libasan" in r.stderr and "No such file" in r.stderr):
        pytest.skip("sanitizer runtime not installed: " + r.stderr[-200:])
    assert r.returncode == 0, r.stderr[-4000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:alloc_dealloc_mismatch=1:strict_string_checks=1", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "all checks passed" in r.stdout
