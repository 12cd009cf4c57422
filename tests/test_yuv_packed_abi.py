"""CPU: the packed YUV extension (include/srcnn_amd_yuv_packed.h) -- its declared functions, committed list, binding and export
table agree (full and strict-only builds), the header compiles as C99, srcnn_yuv_packed_row_bytes matches a restatement, and
every argument rule of srcnn_yuv_packed_upscale_dev returns its code before any device lookup."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from test_abi import HANDLE_ONLY_HOOKS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_ARG, E_SCALE, E_NODEVICE, E_UNSUPPORTED = -1, -2, -200, -203
YUY2, UYVY, YVYU, Y210, Y212, Y216, VUYA, Y410, Y416, V210 = range(10)
FORMATS = {"yuy2": YUY2, "uyvy": UYVY, "yvyu": YVYU, "y210": Y210, "y212": Y212, "y216": Y216, "vuya": VUYA, "y410": Y410,
           "y416": Y416, "v210": V210}
OTHER_HEADERS = ("srcnn_amd.h", "srcnn_amd_yuv.h", "srcnn_amd_yuv_ex.h", "srcnn_amd_rgb.h")


@pytest.fixture(scope="module")
def S():
    import libsrcnn_amd as S
    from libsrcnn_amd import build
    if build.stale():
        build.build(verbose=False)
    return S


def _declared(header):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", header)).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(srcnn_[a-z0-9_]+)\s*\(", text)))


def _exported(path):
    out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
    return sorted(line.split()[-1] for line in out.splitlines() if line.strip())


def test_header_list_binding_and_exports_agree(S):
    names = _declared("srcnn_amd_yuv_packed.h")
    listed = [ln.strip() for ln in open(os.path.join(ROOT, "include", "srcnn_amd_yuv_packed.abi")) if ln.strip() and not ln.startswith("#")]
    assert listed == sorted(listed) and len(set(listed)) == len(listed)
    assert names == listed == sorted(S.YUV_PACKED_SYMBOLS)
    assert set(S.YUV_PACKED_SYMBOLS) <= set(S.C_ABI_SYMBOLS)
    for other in OTHER_HEADERS:
        assert not set(names) & set(_declared(other)), "the extension must not touch " + other
        text = open(os.path.join(ROOT, "include", other)).read()
        assert not any(n in text for n in names) and "yuv_packed" not in text.lower() and "YUVP" not in text, other
    header = open(os.path.join(ROOT, "include", "srcnn_amd_yuv_packed.h")).read()
    assert "#define SRCNN_AMD_YUV_PACKED_VERSION 1" in header and '#include "srcnn_amd.h"' in header
    for name, value in FORMATS.items():
        assert re.search(r"#define SRCNN_YUVP_%s +%d\b" % (name.upper(), value), header), name
    assert "#define SRCNN_AMD_ABI_VERSION 5" in open(os.path.join(ROOT, "include", "srcnn_amd.h")).read()
    exported = _exported(S.LIB_PATH)
    assert set(names) <= set(exported)
    assert exported == sorted(S.C_ABI_SYMBOLS + S.CXX_SYMBOLS + HANDLE_ONLY_HOOKS)
    assert S.lib().srcnn_yuv_packed_abi_version() == 1


def test_strict_only_build_exports_the_same_set(S):
    from libsrcnn_amd import build
    strict, _ = build.build_strict_only(verbose=False)
    assert _exported(strict) == _exported(S.LIB_PATH)
    assert set(S.YUV_PACKED_SYMBOLS) <= set(_exported(strict))


def test_header_compiles_as_c99(tmp_path):
    src = tmp_path / "use.c"
    src.write_text('#include "srcnn_amd_yuv_packed.h"\n'
                   "int f(const void* s, void* d) { size_t b; unsigned a;\n"
                   "  return srcnn_yuv_packed_abi_version() + srcnn_yuv_packed_row_bytes(SRCNN_YUVP_V210, 49, &b, &a)\n"
                   "  + srcnn_yuv_packed_upscale_dev(SRCNN_YUVP_YUY2, 4, 4, 2.0f, SRCNN_FILTER_BICUBIC, s, 0, d, 0, 0)\n"
                   "  + SRCNN_YUVP_UYVY + SRCNN_YUVP_YVYU + SRCNN_YUVP_Y210 + SRCNN_YUVP_Y212 + SRCNN_YUVP_Y216 + SRCNN_YUVP_VUYA\n"
                   "  + SRCNN_YUVP_Y410 + SRCNN_YUVP_Y416 + SRCNN_AMD_YUV_PACKED_VERSION; }\n")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-c", str(src), "-I" + os.path.join(ROOT, "include"),
                           "-o", str(tmp_path / "use.o")])


# ---- srcnn_yuv_packed_row_bytes ----
def row_bytes(fmt, w):
    """The restatement: (tight row bytes, alignment)."""
    if fmt in (YUY2, UYVY, YVYU):
        return 4 * ((w + 1) // 2), 1
    if fmt in (Y210, Y212, Y216):
        return 8 * ((w + 1) // 2), 2
    if fmt == VUYA:
        return 4 * w, 1
    if fmt == Y410:
        return 4 * w, 4
    if fmt == Y416:
        return 8 * w, 2
    assert fmt == V210
    return 128 * ((w + 47) // 48), 4


@pytest.mark.parametrize("name", list(FORMATS))
def test_row_bytes(S, name):
    fmt = FORMATS[name]
    widths = list(range(1, 101)) + [1920, 3840, 3841]
    assert {47, 48, 49} <= set(widths)
    for w in widths:
        assert S.yuv_packed_row_bytes(fmt, w) == row_bytes(fmt, w), (name, w)
        assert S.yuv_packed_row_bytes(name, w) == row_bytes(fmt, w), (name, w)
    assert [row_bytes(V210, w)[0] for w in (1, 47, 48, 49, 96, 97)] == [128, 128, 128, 256, 256, 384]


def test_row_bytes_errors(S):
    L = S.lib()
    b, a = C.c_size_t(), C.c_uint()
    assert L.srcnn_yuv_packed_row_bytes(YUY2, 4, C.byref(b), C.byref(a)) == 0 and (b.value, a.value) == (8, 1)
    assert L.srcnn_yuv_packed_row_bytes(V210, 4, None, None) == 0
    assert L.srcnn_yuv_packed_row_bytes(Y410, 4, None, C.byref(a)) == 0 and a.value == 4
    for fmt in (-1, 10, 99):
        assert L.srcnn_yuv_packed_row_bytes(fmt, 4, C.byref(b), C.byref(a)) == E_ARG
    assert L.srcnn_yuv_packed_row_bytes(YUY2, 0, C.byref(b), C.byref(a)) == E_ARG


# ---- argument rules: host buffers stand in for device frames, which is safe because every call below is refused before
# the device is looked up ----
class Frame:
    """Host memory laid out like an input and an output frame: tight unless pitches are given, both on 64-byte boundaries."""

    def __init__(self, S, fmt=YUY2, w=9, h=7, mul=2.0, src_pitch=0, dst_pitch=0):
        self.fmt, self.w, self.h, self.mul = fmt, w, h, mul
        self.dw, self.dh = S.output_size(w, h, mul)
        self.src_row, self.align = row_bytes(fmt, w)
        self.dst_row = row_bytes(fmt, self.dw)[0]
        up = lambda n: (n + 63) // 64 * 64   # noqa: E731
        self.src_size = max(src_pitch, self.src_row) * h
        self.dst_size = max(dst_pitch, self.dst_row) * self.dh
        self.buf = np.zeros(up(self.src_size) + up(self.dst_size) + 192, np.uint8)
        base = (self.buf.ctypes.data + 63) // 64 * 64
        self.src, self.dst = base, base + up(self.src_size) + 64
        self.src_pitch, self.dst_pitch = src_pitch, dst_pitch

    def call(self, S, **kw):
        a = dict(fmt=self.fmt, w=self.w, h=self.h, multiply=self.mul, filt=2, src=self.src, src_pitch=self.src_pitch,
                 dst=self.dst, dst_pitch=self.dst_pitch)
        a.update(kw)
        try:
            S.yuv_packed_upscale_dev(a["fmt"], a["w"], a["h"], a["multiply"], a["filt"], a["src"], a["src_pitch"], a["dst"], a["dst_pitch"])
        except S.SrcnnError as e:
            return e.code
        return 0


def test_format_and_filter_rules(S):
    f = Frame(S)
    for fmt in (-1, 10, 11, 99, 1 << 20):
        assert f.call(S, fmt=fmt) == E_ARG, fmt
    assert f.call(S, fmt="nv12") == E_ARG
    for filt in (-1, 5, 100):
        assert f.call(S, filt=filt) == E_ARG


@pytest.mark.parametrize("name", list(FORMATS))
def test_null_pointers_and_zero_sizes(S, name):
    f = Frame(S, FORMATS[name])
    assert f.call(S, src=None) == E_ARG and f.call(S, dst=None) == E_ARG
    assert f.call(S, w=0) == E_ARG and f.call(S, h=0) == E_ARG


@pytest.mark.parametrize("name", list(FORMATS))
def test_short_pitches(S, name):
    fmt = FORMATS[name]
    big = Frame(S, fmt, src_pitch=512, dst_pitch=512)
    step = big.align                                      # keep the pitch aligned: a misaligned one is refused for itself
    assert big.call(S, src_pitch=big.src_row - step) == E_ARG
    assert big.call(S, dst_pitch=big.dst_row - step) == E_ARG
    if big.src_row < big.dst_row:                         # the input's row length is not the output's (v210: one block both)
        assert big.call(S, dst_pitch=big.src_row) == E_ARG
    if S.device_count() == 0:
        assert big.call(S, src_pitch=big.src_row, dst_pitch=big.dst_row) == E_NODEVICE
        assert big.call(S, src_pitch=0, dst_pitch=0) == E_NODEVICE
        assert big.call(S) == E_NODEVICE


@pytest.mark.parametrize("name", list(FORMATS))
def test_misaligned_addresses_and_pitches(S, name):
    fmt = FORMATS[name]
    f = Frame(S, fmt, src_pitch=512, dst_pitch=512)
    for off in range(1, f.align):
        assert f.call(S, src=f.src + off) == E_ARG, ("src", off)
        assert f.call(S, dst=f.dst + off) == E_ARG, ("dst", off)
        assert f.call(S, src_pitch=512 + off) == E_ARG, ("src pitch", off)
        assert f.call(S, dst_pitch=512 - off) == E_ARG, ("dst pitch", off)
    if S.device_count() == 0:                             # the alignment itself is enough
        g = Frame(S, fmt, src_pitch=512 + f.align, dst_pitch=512 + 3 * f.align)
        assert g.call(S, src=g.src + f.align, dst=g.dst + f.align) == E_NODEVICE


def test_multiply_and_size_limits(S):
    f = Frame(S)
    for mul in (0.0, -1.0, 0.1, 0.05, float("nan")):
        assert f.call(S, multiply=mul) == E_SCALE, mul
    assert f.call(S, w=1 << 22, h=2, multiply=4.0) == E_UNSUPPORTED
    assert f.call(S, w=2, h=1 << 20, multiply=2.0) == E_UNSUPPORTED
    assert f.call(S, w=60000, h=60000, multiply=2.0) == E_UNSUPPORTED
    assert f.call(S, multiply=float("inf")) == E_UNSUPPORTED


@pytest.mark.parametrize("name", ["yuy2", "y210", "y410", "y416", "v210"])
def test_overlapping_frames(S, name):
    f = Frame(S, FORMATS[name])
    assert f.call(S, dst=f.src) == E_ARG                                   # same start
    assert f.call(S, dst=f.src + f.src_size - 4) == E_ARG                  # output starts on the input's last dword
    assert f.call(S, dst=f.src - f.dst_size + 4) == E_ARG                  # output ends on the input's first dword
    p = Frame(S, FORMATS[name], src_pitch=512, dst_pitch=1024)
    assert p.call(S, dst=p.src + 512 * (p.h - 1)) == E_ARG                 # ... also with pitches: the input's last row
    if S.device_count() == 0:
        assert f.call(S, dst=f.src + f.src_size) == E_NODEVICE             # adjacent is not overlapping
        assert f.call(S, dst=f.dst, src=f.dst + f.dst_size) == E_NODEVICE


def test_valid_calls_without_a_device(S):
    if S.device_count() > 0:
        pytest.skip("a device is present: a valid call would run on host memory")
    for fmt in FORMATS.values():
        for (w, h, mul) in ((9, 7, 2.0), (1, 1, 3.0), (16, 8, 0.75), (49, 2, 1.0)):
            assert Frame(S, fmt, w, h, mul).call(S) == E_NODEVICE, (fmt, w, h, mul)
