"""CPU: the host half of the packed YUV rect call under AddressSanitizer + UBSan.

tests/host/yuv_packed_rect_sanitize.cpp is a stand-alone program (its own main, no GPU, no HIP) that drives the bodies of
srcnn_yuv_packed_span_bytes and srcnn_yuv_packed_rect_source (csrc/srcnn_rect_source.hpp) and the argument validation of
srcnn_yuv_packed_upscale_rect_dev (check_yuv_packed_rect_args in csrc/srcnn_frame_args.hpp) across the shapes of
tests/test_yuv_packed_rect_abi.py, and holds yuvp_window_fits, the predicate that picks k_yuvp_window_merge or the plane route
for a rect, to its answers on tables from build_axis_table, v210's tile width of 60 included -- both routes give the same bytes,
so no other test would notice it refusing everything.  It is built here the way `make asan` builds tests/host/host_sanitize.cpp
and run as a process of its own; nothing of it is loaded into Python."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_yuv_packed_rect_host_code_under_asan_and_ubsan(tmp_path):
    if not shutil.which("g++"):
        pytest.skip("no host toolchain")
    exe = str(tmp_path / "yuv_packed_rect_asan")
    r = subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                        "-fno-omit-frame-pointer", os.path.join(ROOT, "tests", "host", "yuv_packed_rect_sanitize.cpp"), "-lm", "-o", exe],
                       capture_output=True, text=True, timeout=600)
    if r.returncode != 0 and ("cannot find -lasan" in r.stderr or "libasan" in r.stderr and "No such file" in r.stderr):
        pytest.skip("sanitizer runtime not installed: " + r.stderr[-200:])
    assert r.returncode == 0, r.stderr[-4000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:alloc_dealloc_mismatch=1:strict_string_checks=1", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "all checks passed" in r.stdout
