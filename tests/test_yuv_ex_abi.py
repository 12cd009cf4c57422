"""CPU: the high-bit-depth / 4:2:2 / 4:4:4 YUV extension (include/srcnn_amd_yuv_ex.h) -- its declared functions, committed list,
binding and export table agree (full and strict-only builds), srcnn_yuv_plane_size matches a restatement, every argument rule
of srcnn_yuv_upscale_dev returns its code before any device lookup, and `srcnnyuv --all-formats` refuses what it does not
handle with status 2 without touching a device."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from test_abi import HANDLE_ONLY_HOOKS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_ARG, E_SCALE, E_NODEVICE, E_UNSUPPORTED = -1, -2, -200, -203
PLANAR, SEMI = 0, 1
C420, C422, C444 = 0, 1, 2
DEPTHS = (8, 10, 12, 14, 16)


@pytest.fixture(scope="module")
def S():
    import libsrcnn_amd as S
    from libsrcnn_amd import build
    if build.stale() or not os.path.exists(os.path.join(ROOT, "libsrcnn_amd", "bin", "srcnnyuv")):
        build.build(verbose=False)
    return S


def _declared(header):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", header)).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(srcnn_[a-z0-9_]+)\s*\(", text)))


def _exported(path):
    out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
    return sorted(line.split()[-1] for line in out.splitlines() if line.strip())


def test_header_list_binding_and_exports_agree(S):
    names = _declared("srcnn_amd_yuv_ex.h")
    listed = [ln.strip() for ln in open(os.path.join(ROOT, "include", "srcnn_amd_yuv_ex.abi")) if ln.strip() and not ln.startswith("#")]
    assert listed == sorted(listed) and len(set(listed)) == len(listed)
    assert names == listed == sorted(S.YUV_EX_SYMBOLS)
    assert set(S.YUV_EX_SYMBOLS) <= set(S.C_ABI_SYMBOLS)
    for other in ("srcnn_amd.h", "srcnn_amd_yuv.h"):
        assert not set(names) & set(_declared(other)), "the extension must not touch " + other
        text = open(os.path.join(ROOT, "include", other)).read()
        assert not any(n in text for n in names) and "yuv_ex" not in text.lower(), other
    header = open(os.path.join(ROOT, "include", "srcnn_amd_yuv_ex.h")).read()
    assert "#define SRCNN_AMD_YUV_EX_VERSION 1" in header and '#include "srcnn_amd.h"' in header
    for line in ("#define SRCNN_YUV_PLANAR     0", "#define SRCNN_YUV_SEMIPLANAR 1", "#define SRCNN_YUV_420 0",
                 "#define SRCNN_YUV_422 1", "#define SRCNN_YUV_444 2"):
        assert line in header, line
    exported = _exported(S.LIB_PATH)
    assert set(names) <= set(exported)
    assert exported == sorted(S.C_ABI_SYMBOLS + S.CXX_SYMBOLS + HANDLE_ONLY_HOOKS)
    assert S.lib().srcnn_yuv_ex_abi_version() == 1


def test_strict_only_build_exports_the_same_set(S):
    from libsrcnn_amd import build
    strict, _ = build.build_strict_only(verbose=False)
    assert _exported(strict) == _exported(S.LIB_PATH)
    assert set(S.YUV_EX_SYMBOLS) <= set(_exported(strict))


def test_header_compiles_as_c99(tmp_path):
    src = tmp_path / "use.c"
    src.write_text('#include "srcnn_amd_yuv_ex.h"\n'
                   "int f(void) { srcnn_yuv_format x = {sizeof(srcnn_yuv_format), SRCNN_YUV_SEMIPLANAR, SRCNN_YUV_422, 10, 1};\n"
                   "  unsigned c, r; size_t b; return srcnn_yuv_ex_abi_version() + srcnn_yuv_plane_size(&x, 4, 4, 1, &c, &r, &b)\n"
                   "  + SRCNN_YUV_PLANAR + SRCNN_YUV_420 + SRCNN_YUV_444 + SRCNN_AMD_YUV_EX_VERSION; }\n")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-c", str(src), "-I" + os.path.join(ROOT, "include"),
                           "-o", str(tmp_path / "use.o")])


# ---- srcnn_yuv_plane_size ----
def plane_size(layout, chroma, depth, w, h, plane):
    """The restatement: (cols, rows, tight row bytes)."""
    if plane == 0:
        return w, h, w * (1 if depth == 8 else 2)
    if layout == SEMI and plane == 2:
        return 0, 0, 0
    cols, rows = (w if chroma == C444 else (w + 1) // 2), ((h + 1) // 2 if chroma == C420 else h)
    return cols, rows, cols * (1 if depth == 8 else 2) * (2 if layout == SEMI else 1)


@pytest.mark.parametrize("layout", [PLANAR, SEMI])
@pytest.mark.parametrize("chroma", [C420, C422, C444])
def test_plane_size(S, layout, chroma):
    for depth in DEPTHS:
        for msb in ((0,) if depth == 8 else (0, 1)):
            fmt = S.yuv_format(layout, chroma, depth, msb)
            for (w, h) in ((1, 1), (2, 2), (9, 7), (8, 6), (1, 5), (17, 2), (1920, 1080), (3841, 2161)):
                for plane in range(3):
                    assert S.yuv_plane_size(fmt, w, h, plane) == plane_size(layout, chroma, depth, w, h, plane), (depth, w, h, plane)


def test_plane_size_errors(S):
    L = S.lib()
    fmt = S.yuv_format(PLANAR, C420, 10, 0)
    c, r, b = C.c_uint(), C.c_uint(), C.c_size_t()
    ok = lambda f, w, h, p: L.srcnn_yuv_plane_size(f, w, h, p, C.byref(c), C.byref(r), C.byref(b))   # noqa: E731
    assert ok(C.byref(fmt), 4, 4, 0) == 0
    assert L.srcnn_yuv_plane_size(C.byref(fmt), 4, 4, 1, None, None, None) == 0
    assert ok(None, 4, 4, 0) == E_ARG
    assert ok(C.byref(fmt), 0, 4, 0) == E_ARG and ok(C.byref(fmt), 4, 0, 0) == E_ARG
    assert ok(C.byref(fmt), 4, 4, 3) == E_ARG and ok(C.byref(fmt), 4, 4, -1) == E_ARG
    bad = S.yuv_format(PLANAR, C420, 9, 0)
    assert ok(C.byref(bad), 4, 4, 0) == E_ARG


# ---- argument rules: host buffers stand in for device planes, which is safe because every call below is refused before
# the device is looked up ----
class Frame:
    """Host memory laid out like one frame's planes: tight unless pitches are given; every plane starts on an even address."""

    def __init__(self, S, layout=PLANAR, chroma=C420, depth=10, msb=0, w=9, h=7, mul=2.0, src_pitch=None, dst_pitch=None):
        self.fmt = S.yuv_format(layout, chroma, depth, msb)
        self.w, self.h, self.mul = w, h, mul
        self.np = 2 if layout == SEMI else 3
        (self.dw, self.dh), self.src_planes, self.dst_planes = S.yuv_plane_sizes(self.fmt, w, h, mul)
        sp = src_pitch or [0, 0, 0]
        dp = dst_pitch or [0, 0, 0]
        even = lambda n: (n + 1) & ~1   # noqa: E731
        self.src_sizes = [even(max(sp[k], rb) * r) for k, (_c, r, rb) in enumerate(self.src_planes)]
        self.dst_sizes = [even(max(dp[k], rb) * r) for k, (_c, r, rb) in enumerate(self.dst_planes)]
        self.buf = np.zeros(sum(self.src_sizes) + sum(self.dst_sizes) + 64, np.uint16)
        base = self.buf.ctypes.data
        offs = np.cumsum([0] + self.src_sizes + self.dst_sizes)
        self.src = [base + int(o) for o in offs[:self.np]] + [None] * (3 - self.np)
        self.dst = [base + int(o) for o in offs[self.np:2 * self.np]] + [None] * (3 - self.np)
        self.src_pitch, self.dst_pitch = src_pitch, dst_pitch

    def call(self, S, **kw):
        a = dict(fmt=self.fmt, w=self.w, h=self.h, multiply=self.mul, filt=2, src=self.src, src_pitch=self.src_pitch,
                 dst=self.dst, dst_pitch=self.dst_pitch)
        a.update(kw)
        try:
            S.yuv_upscale_dev(a["fmt"], a["w"], a["h"], a["multiply"], a["filt"], a["src"], a["src_pitch"], a["dst"], a["dst_pitch"])
        except S.SrcnnError as e:
            return e.code
        return 0


def test_format_rules(S):
    f = Frame(S)
    assert f.call(S, fmt=None) == E_ARG
    for size in (0, 4, 19, 21, 24):
        fmt = S.yuv_format(PLANAR, C420, 10, 0)
        fmt.struct_size = size
        assert f.call(S, fmt=fmt) == E_ARG, size
    for layout in (-1, 2, 99):
        assert f.call(S, fmt=S.yuv_format(layout, C420, 10, 0)) == E_ARG
    for chroma in (-1, 3, 99):
        assert f.call(S, fmt=S.yuv_format(PLANAR, chroma, 10, 0)) == E_ARG
    for depth in (0, 7, 9, 11, 13, 15, 17, 32, -10):
        assert f.call(S, fmt=S.yuv_format(PLANAR, C420, depth, 0)) == E_ARG, depth
    for msb in (-1, 2):
        assert f.call(S, fmt=S.yuv_format(PLANAR, C420, 10, msb)) == E_ARG
    assert Frame(S, depth=8).call(S, fmt=S.yuv_format(PLANAR, C420, 8, 1)) == E_ARG
    for filt in (-1, 5, 100):
        assert f.call(S, filt=filt) == E_ARG


@pytest.mark.parametrize("layout", [PLANAR, SEMI])
@pytest.mark.parametrize("depth", [8, 10, 16])
def test_null_planes_and_zero_sizes(S, layout, depth):
    f = Frame(S, layout=layout, depth=depth)
    for k in range(f.np):
        src = list(f.src); src[k] = None
        assert f.call(S, src=src) == E_ARG
        dst = list(f.dst); dst[k] = None
        assert f.call(S, dst=dst) == E_ARG
    assert f.call(S, src=None) == E_ARG and f.call(S, dst=None) == E_ARG
    assert f.call(S, w=0) == E_ARG and f.call(S, h=0) == E_ARG


@pytest.mark.parametrize("layout", [PLANAR, SEMI])
@pytest.mark.parametrize("chroma", [C420, C422, C444])
@pytest.mark.parametrize("depth", [8, 12])
def test_short_pitches(S, layout, chroma, depth):
    big = Frame(S, layout=layout, chroma=chroma, depth=depth, src_pitch=[256, 256, 256], dst_pitch=[256, 256, 256])
    n = big.np
    step = 1 if depth == 8 else 2                        # at depth > 8 keep the pitch even: an odd one is refused for itself
    for k in range(n):
        sp = [0, 0, 0]; sp[k] = big.src_planes[k][2] - step
        assert big.call(S, src_pitch=sp) == E_ARG, ("src", k)
        dp = [0, 0, 0]; dp[k] = big.dst_planes[k][2] - step
        assert big.call(S, dst_pitch=dp) == E_ARG, ("dst", k)
    if layout == SEMI:                                   # the byte length of a planar chroma row is not a UV row
        assert big.call(S, src_pitch=[0, big.src_planes[1][2] // 2, 0]) == E_ARG
    if depth > 8:                                        # one byte per sample is not a 16-bit row
        assert big.call(S, dst_pitch=[big.dw, 0, 0]) == E_ARG
    if S.device_count() == 0:
        exact_s = [p[2] for p in big.src_planes] + [0] * (3 - n)
        exact_d = [p[2] for p in big.dst_planes] + [0] * (3 - n)
        assert big.call(S, src_pitch=exact_s, dst_pitch=exact_d) == E_NODEVICE
        assert big.call(S, src_pitch=[0, 0, 0], dst_pitch=None) == E_NODEVICE


@pytest.mark.parametrize("layout", [PLANAR, SEMI])
def test_odd_addresses_and_pitches_above_8_bits(S, layout):
    f = Frame(S, layout=layout, depth=10, src_pitch=[64, 64, 64], dst_pitch=[64, 64, 64])
    for k in range(f.np):
        src = list(f.src); src[k] += 1
        assert f.call(S, src=src) == E_ARG, ("src", k)
        dst = list(f.dst); dst[k] += 1
        assert f.call(S, dst=dst) == E_ARG, ("dst", k)
        sp = [64, 64, 64]; sp[k] = 65
        assert f.call(S, src_pitch=sp) == E_ARG
        dp = [64, 64, 64]; dp[k] = 63
        assert f.call(S, dst_pitch=dp) == E_ARG
    if S.device_count() == 0:
        g = Frame(S, layout=layout, depth=8, src_pitch=[65, 65, 65], dst_pitch=[63, 63, 63])     # depth 8: no alignment rule
        src = list(g.src); src[0] += 1
        assert g.call(S, src=src) == E_NODEVICE


def test_multiply_and_size_limits(S):
    f = Frame(S)
    for mul in (0.0, -1.0, 0.1, 0.05, float("nan")):
        assert f.call(S, multiply=mul) == E_SCALE, mul
    assert f.call(S, w=1 << 22, h=2, multiply=4.0) == E_UNSUPPORTED
    assert f.call(S, w=2, h=1 << 20, multiply=2.0) == E_UNSUPPORTED
    assert f.call(S, w=60000, h=60000, multiply=2.0) == E_UNSUPPORTED
    assert f.call(S, multiply=float("inf")) == E_UNSUPPORTED


@pytest.mark.parametrize("layout", [PLANAR, SEMI])
@pytest.mark.parametrize("depth", [8, 10])
def test_overlapping_planes(S, layout, depth):
    f = Frame(S, layout=layout, chroma=C422, depth=depth)
    for a in range(f.np):
        for b in range(f.np):
            dst = list(f.dst); dst[b] = f.src[a]                        # same start
            assert f.call(S, dst=dst) == E_ARG, (a, b)
            dst = list(f.dst); dst[b] = f.src[a] + f.src_sizes[a] - 2  # output starts on the input's last sample
            assert f.call(S, dst=dst) == E_ARG, (a, b)
    dst = list(f.dst); dst[0] = f.src[0] - f.dst_sizes[0] + 2           # an output that ends on the first sample of an input
    assert f.call(S, dst=dst) == E_ARG


def test_valid_calls_without_a_device(S):
    if S.device_count() > 0:
        pytest.skip("a device is present: a valid call would run on host memory")
    for layout in (PLANAR, SEMI):
        for chroma in (C420, C422, C444):
            for depth in DEPTHS:
                for msb in ((0,) if depth == 8 else (0, 1)):
                    for (w, h, mul) in ((9, 7, 2.0), (1, 1, 3.0), (16, 8, 0.75)):
                        assert Frame(S, layout, chroma, depth, msb, w, h, mul).call(S) == E_NODEVICE
    f = Frame(S, layout=SEMI)
    assert f.call(S, src=[f.src[0], f.src[1], None], dst=[f.dst[0], f.dst[1], None]) == E_NODEVICE   # plane[2] ignored


# ---- tools/srcnnyuv --all-formats ----
def _srcnnyuv():
    return os.path.join(ROOT, "libsrcnn_amd", "bin", "srcnnyuv")


_HIDDEN = dict(HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1")


@pytest.mark.parametrize("tags", ["Cmono", "C444alpha", "It", "C420p9", "C411", "C420p10 Ib", "Cmono16"])
def test_srcnnyuv_all_formats_still_refuses(S, tmp_path, tags):
    src = tmp_path / "in.y4m"
    src.write_bytes(b"YUV4MPEG2 W8 H6 F25:1 " + tags.encode() + b"\nFRAME\n" + bytes(8 * 6 * 6))
    r = subprocess.run([_srcnnyuv(), "--all-formats", str(src), str(tmp_path / "out.y4m")], capture_output=True, text=True,
                       timeout=60, env=dict(os.environ, **_HIDDEN))
    assert r.returncode == 2, (r.returncode, r.stderr)
    assert len(r.stderr.strip().splitlines()) == 1 and "srcnnyuv:" in r.stderr
    assert not (tmp_path / "out.y4m").exists()


@pytest.mark.parametrize("tag,bytes_per_frame", [("C420p10", (9 * 7 + 2 * 5 * 4) * 2), ("C422", 9 * 7 + 2 * 5 * 7),
                                                 ("C444p16", 9 * 7 * 3 * 2)])
def test_srcnnyuv_all_formats_gets_past_the_header(S, tmp_path, tag, bytes_per_frame):
    src = tmp_path / "in.y4m"
    src.write_bytes(b"YUV4MPEG2 W9 H7 F25:1 Ip " + tag.encode() + b"\nFRAME\n" + bytes(bytes_per_frame))
    r = subprocess.run([_srcnnyuv(), "--all-formats", str(src), "-"], capture_output=True, timeout=60, env=dict(os.environ, **_HIDDEN))
    assert r.returncode == 1, (r.returncode, r.stderr)     # the missing device, not the header
    # and the same stream without the option keeps today's refusal
    r = subprocess.run([_srcnnyuv(), str(src), "-"], capture_output=True, timeout=60, env=dict(os.environ, **_HIDDEN))
    assert r.returncode == 2
