"""CPU: the host half of the rect list call under AddressSanitizer + UBSan.

tests/host/rect_list_sanitize.cpp is a stand-alone program (its own main, no GPU, no HIP) that drives the router, the shelf
packer and the descriptor tables of csrc/srcnn_rect_atlas.hpp -- the code srcnn_y_path_rect_list_plan and
srcnn_y_path_rect_list_f32_dev both run -- over seeded lists: n = 1, 65536 one-sample rects, a frame-sized rect among small ones,
strips, and workspace caps that force many atlases.  It asserts that cells lie inside their atlas and are pairwise disjoint, that
every item is placed exactly once and that the tile prefix sums are consistent.  It is built here exactly as
tests/test_yuv_rect_sanitizer.py builds its program and run as a process of its own; nothing of it is loaded into Python."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_rect_list_host_code_under_asan_and_ubsan(tmp_path):
    if not shutil.which("g++"):
        pytest.skip("no host toolchain")
    exe = str(tmp_path / "rect_list_asan")
    r = subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                        "-fno-omit-frame-pointer", os.path.join(ROOT, "tests", "host", "rect_list_sanitize.cpp"), "-lm", "-o", exe],
                       capture_output=True, text=True, timeout=600)
    if r.returncode != 0 and ("cannot find -lasan" in r.stderr or "libasan" in r.stderr and "No such file" in r.stderr):
        pytest.skip("sanitizer runtime not installed: " + r.stderr[-200:])
    assert r.returncode == 0, r.stderr[-4000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:alloc_dealloc_mismatch=1:strict_string_checks=1", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "all checks passed" in r.stdout
