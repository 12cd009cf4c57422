"""CPU: the host half of the packed YUV rect list call under AddressSanitizer + UBSan.

tests/host/yuv_packed_rect_list_sanitize.cpp is a stand-alone program (its own main, no GPU, no HIP) that drives the router with
the chroma condition and the destination table of csrc/srcnn_yuv_packed_rect_atlas.hpp -- the code
srcnn_yuv_packed_upscale_rect_list_plan and srcnn_yuv_packed_upscale_rect_list_dev both run -- over seeded lists in all six kinds
(YUY2, Y210, VUYA, Y410, Y416, v210).  It asserts that every destination entry belongs to exactly one batched item, that the
tile prefix counts each item's tiles once (at 60 columns for v210) and ends at the closing entry's total, that the bytes an entry
lets the merge kernel write -- recomputed from the descriptors alone -- are the item's rh row segments of n bytes at its pitch,
v210's padding groups included only at the right border, that [blo, bhi) lies inside the span of the item's reported source
rectangle, that the vector store path is flagged only where base and pitch are multiples of 16, that an item whose chroma window
does not fit is routed single, and that a frame whose chroma width keeps its size routes every item single.  It is built here
exactly as tests/test_yuv_rect_list_sanitizer.py builds its program and run as a process of its own; nothing of it is loaded into
Python."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_yuv_packed_rect_list_host_code_under_asan_and_ubsan(tmp_path):
    if not shutil.which("g++"):
        pytest.skip("no host toolchain")
    exe = str(tmp_path / "yuv_packed_rect_list_asan")
    r = subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                        "-fno-omit-frame-pointer", os.path.join(ROOT, "tests", "host", "yuv_packed_rect_list_sanitize.cpp"), "-lm", "-o", exe],
                       capture_output=True, text=True, timeout=600)
    if r.returncode != 0 and ("cannot find -lasan" in r.stderr or "libasan" in r.stderr and "No such file" in r.stderr):
        pytest.skip("sanitizer runtime not installed: " + r.stderr[-200:])
    assert r.returncode == 0, r.stderr[-4000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:alloc_dealloc_mismatch=1:strict_string_checks=1", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "all checks passed" in r.stdout
