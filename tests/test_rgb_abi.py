"""CPU: the device-resident RGB(A) extension (include/srcnn_amd_rgb.h) -- its declared functions, committed list, binding and
export table agree (full and strict-only builds), the header is C99, srcnn_rgb_plane_size matches a restatement, and every
argument rule of srcnn_rgb_upscale_dev returns its code before any device lookup (host buffers stand in for device planes)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from test_abi import HANDLE_ONLY_HOOKS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_ARG, E_SCALE, E_NODEVICE, E_UNSUPPORTED = -1, -2, -200, -203
INTER, PLANAR = 0, 1
RGB, BGR = 0, 1
DEPTHS = (8, 10, 12, 14, 16)


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
    names = _declared("srcnn_amd_rgb.h")
    listed = [ln.strip() for ln in open(os.path.join(ROOT, "include", "srcnn_amd_rgb.abi")) if ln.strip() and not ln.startswith("#")]
    assert listed == sorted(listed) and len(set(listed)) == len(listed)
    assert names == listed == sorted(S.RGB_SYMBOLS)
    assert set(S.RGB_SYMBOLS) <= set(S.C_ABI_SYMBOLS)
    for other in ("srcnn_amd.h", "srcnn_amd_yuv.h", "srcnn_amd_yuv_ex.h"):
        assert not set(names) & set(_declared(other)), "the extension must not touch " + other
        text = open(os.path.join(ROOT, "include", other)).read()
        assert not any(n in text for n in names) and "srcnn_amd_rgb" not in text.lower(), other
    header = open(os.path.join(ROOT, "include", "srcnn_amd_rgb.h")).read()
    assert "#define SRCNN_AMD_RGB_VERSION 1" in header and '#include "srcnn_amd.h"' in header
    for line in ("#define SRCNN_RGB_INTERLEAVED 0", "#define SRCNN_RGB_PLANAR      1", "#define SRCNN_RGB_ORDER_RGB   0",
                 "#define SRCNN_RGB_ORDER_BGR   1"):
        assert line in header, line
    exported = _exported(S.LIB_PATH)
    assert set(names) <= set(exported)
    assert exported == sorted(S.C_ABI_SYMBOLS + S.CXX_SYMBOLS + HANDLE_ONLY_HOOKS)
    assert S.lib().srcnn_rgb_abi_version() == 1
    assert C.sizeof(S.RgbFormat) == 20


def test_strict_only_build_exports_the_same_set(S):
    from libsrcnn_amd import build
    strict, _ = build.build_strict_only(verbose=False)
    assert _exported(strict) == _exported(S.LIB_PATH)
    assert set(S.RGB_SYMBOLS) <= set(_exported(strict))


def test_header_compiles_as_c99(tmp_path):
    src = tmp_path / "use.c"
    src.write_text('#include "srcnn_amd_rgb.h"\n'
                   "int f(void) { srcnn_rgb_format x = {sizeof(srcnn_rgb_format), SRCNN_RGB_PLANAR, SRCNN_RGB_ORDER_BGR, 1, 10};\n"
                   "  unsigned c, r; size_t b; const void* s[4] = {0, 0, 0, 0}; void* d[4] = {0, 0, 0, 0};\n"
                   "  return srcnn_rgb_abi_version() + srcnn_rgb_plane_size(&x, 4, 4, 1, &c, &r, &b)\n"
                   "  + srcnn_rgb_upscale_dev(&x, 4, 4, 2.0f, SRCNN_FILTER_BICUBIC, s, 0, d, 0, 0, 0, 0)\n"
                   "  + SRCNN_RGB_INTERLEAVED + SRCNN_RGB_ORDER_RGB + SRCNN_AMD_RGB_VERSION; }\n")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-c", str(src), "-I" + os.path.join(ROOT, "include"),
                           "-o", str(tmp_path / "use.o")])


# ---- srcnn_rgb_plane_size ----
def plane_size(layout, alpha, depth, w, h, plane):
    """The restatement: (cols, rows, tight row bytes)."""
    bps = 1 if depth == 8 else 2
    if layout == INTER:
        return (w, h, w * (3 + alpha) * bps) if plane == 0 else (0, 0, 0)
    return (w, h, w * bps) if plane < 3 + alpha else (0, 0, 0)


@pytest.mark.parametrize("layout", [INTER, PLANAR])
@pytest.mark.parametrize("alpha", [0, 1])
def test_plane_size(S, layout, alpha):
    for depth in DEPTHS:
        for order in (RGB, BGR):
            fmt = S.rgb_format(layout, order, alpha, depth)
            for (w, h) in ((1, 1), (2, 2), (9, 7), (8, 6), (1, 5), (17, 2), (1920, 1080), (3841, 2161)):
                for plane in range(4):
                    assert S.rgb_plane_size(fmt, w, h, plane) == plane_size(layout, alpha, depth, w, h, plane), (depth, w, h, plane)


def test_plane_size_errors(S):
    L = S.lib()
    fmt = S.rgb_format(PLANAR, RGB, 1, 10)
    c, r, b = C.c_uint(), C.c_uint(), C.c_size_t()
    ok = lambda f, w, h, p: L.srcnn_rgb_plane_size(f, w, h, p, C.byref(c), C.byref(r), C.byref(b))   # noqa: E731
    assert ok(C.byref(fmt), 4, 4, 0) == 0
    assert L.srcnn_rgb_plane_size(C.byref(fmt), 4, 4, 3, None, None, None) == 0
    assert ok(None, 4, 4, 0) == E_ARG
    assert ok(C.byref(fmt), 0, 4, 0) == E_ARG and ok(C.byref(fmt), 4, 0, 0) == E_ARG
    assert ok(C.byref(fmt), 4, 4, 4) == E_ARG and ok(C.byref(fmt), 4, 4, -1) == E_ARG
    bad = S.rgb_format(PLANAR, RGB, 0, 9)
    assert ok(C.byref(bad), 4, 4, 0) == E_ARG


# ---- argument rules: host buffers stand in for device planes, which is safe because every call below is refused before
# the device is looked up ----
class Image:
    """Host memory laid out like one image's planes and the result's, dst_conv last: tight unless pitches are given; every
    plane starts on an even address."""

    def __init__(self, S, layout=INTER, order=RGB, alpha=0, depth=10, w=9, h=7, mul=2.0, src_pitch=None, dst_pitch=None,
                 conv=True, conv_pitch=0):
        self.fmt = S.rgb_format(layout, order, alpha, depth)
        self.w, self.h, self.mul = w, h, mul
        self.np = (3 + alpha) if layout == PLANAR else 1
        self.dw, self.dh = S.output_size(w, h, mul)
        self.src_planes = [S.rgb_plane_size(self.fmt, w, h, k) for k in range(self.np)]
        self.dst_planes = [S.rgb_plane_size(self.fmt, self.dw, self.dh, k) for k in range(self.np)]
        self.conv_row = self.dw * (1 if depth == 8 else 2)
        sp = src_pitch or [0, 0, 0, 0]
        dp = dst_pitch or [0, 0, 0, 0]
        even = lambda n: (n + 1) & ~1   # noqa: E731
        self.src_sizes = [even(max(sp[k], rb) * r) for k, (_c, r, rb) in enumerate(self.src_planes)]
        self.dst_sizes = [even(max(dp[k], rb) * r) for k, (_c, r, rb) in enumerate(self.dst_planes)]
        self.conv_size = even(max(conv_pitch, self.conv_row) * self.dh)
        self.buf = np.zeros(sum(self.src_sizes) + sum(self.dst_sizes) + self.conv_size + 64, np.uint16)
        base = self.buf.ctypes.data
        offs = np.cumsum([0] + self.src_sizes + self.dst_sizes)
        self.src = [base + int(o) for o in offs[:self.np]] + [None] * (4 - self.np)
        self.dst = [base + int(o) for o in offs[self.np:2 * self.np]] + [None] * (4 - self.np)
        self.conv = base + int(offs[2 * self.np]) if conv else None
        self.src_pitch, self.dst_pitch, self.conv_pitch = src_pitch, dst_pitch, conv_pitch

    def call(self, S, **kw):
        a = dict(fmt=self.fmt, w=self.w, h=self.h, multiply=self.mul, filt=2, src=self.src, src_pitch=self.src_pitch,
                 dst=self.dst, dst_pitch=self.dst_pitch, conv=self.conv, conv_pitch=self.conv_pitch)
        a.update(kw)
        try:
            S.rgb_upscale_dev(a["fmt"], a["w"], a["h"], a["multiply"], a["filt"], a["src"], a["src_pitch"], a["dst"], a["dst_pitch"],
                              a["conv"], a["conv_pitch"])
        except S.SrcnnError as e:
            return e.code
        return 0


def test_format_rules(S):
    f = Image(S)
    assert f.call(S, fmt=None) == E_ARG
    for size in (0, 4, 19, 21, 24):
        fmt = S.rgb_format(INTER, RGB, 0, 10)
        fmt.struct_size = size
        assert f.call(S, fmt=fmt) == E_ARG, size
    for layout in (-1, 2, 99):
        assert f.call(S, fmt=S.rgb_format(layout, RGB, 0, 10)) == E_ARG
    for order in (-1, 2, 99):
        assert f.call(S, fmt=S.rgb_format(INTER, order, 0, 10)) == E_ARG
    for alpha in (-1, 2, 4):
        assert f.call(S, fmt=S.rgb_format(INTER, RGB, alpha, 10)) == E_ARG
    for depth in (0, 7, 9, 11, 13, 15, 17, 32, -10):
        assert f.call(S, fmt=S.rgb_format(INTER, RGB, 0, depth)) == E_ARG, depth
    for filt in (-1, 5, 100):
        assert f.call(S, filt=filt) == E_ARG


@pytest.mark.parametrize("layout", [INTER, PLANAR])
@pytest.mark.parametrize("alpha", [0, 1])
@pytest.mark.parametrize("depth", [8, 10, 16])
def test_null_planes_and_zero_sizes(S, layout, alpha, depth):
    f = Image(S, layout=layout, alpha=alpha, depth=depth)
    for k in range(f.np):
        src = list(f.src); src[k] = None
        assert f.call(S, src=src) == E_ARG
        dst = list(f.dst); dst[k] = None
        assert f.call(S, dst=dst) == E_ARG
    assert f.call(S, src=None) == E_ARG and f.call(S, dst=None) == E_ARG
    assert f.call(S, w=0) == E_ARG and f.call(S, h=0) == E_ARG
    if S.device_count() == 0:
        # planes the format does not use are ignored: 1..3 when interleaved, 3 without alpha when planar; dst_conv is optional
        junk = 1 if depth == 8 else 2
        src = list(f.src); dst = list(f.dst)
        for k in range(f.np, 4):
            src[k] = junk * (k + 1); dst[k] = junk * (k + 1)
        assert f.call(S, src=src, dst=dst) == E_NODEVICE
        assert f.call(S, conv=None) == E_NODEVICE


@pytest.mark.parametrize("layout", [INTER, PLANAR])
@pytest.mark.parametrize("alpha", [0, 1])
@pytest.mark.parametrize("depth", [8, 12])
def test_short_pitches(S, layout, alpha, depth):
    big = Image(S, layout=layout, alpha=alpha, depth=depth, src_pitch=[512] * 4, dst_pitch=[512] * 4, conv_pitch=512)
    n = big.np
    step = 1 if depth == 8 else 2                        # at depth > 8 keep the pitch even: an odd one is refused for itself
    for k in range(n):
        sp = [0] * 4; sp[k] = big.src_planes[k][2] - step
        assert big.call(S, src_pitch=sp) == E_ARG, ("src", k)
        dp = [0] * 4; dp[k] = big.dst_planes[k][2] - step
        assert big.call(S, dst_pitch=dp) == E_ARG, ("dst", k)
    assert big.call(S, conv_pitch=big.conv_row - step) == E_ARG
    if layout == INTER:                                  # the byte length of one channel's row is not a row of pixels
        assert big.call(S, src_pitch=[big.src_planes[0][2] // (3 + alpha), 0, 0, 0]) == E_ARG
    if depth > 8:                                        # one byte per sample is not a 16-bit row
        assert big.call(S, conv_pitch=big.dw) == E_ARG
    if S.device_count() == 0:
        exact_s = [p[2] for p in big.src_planes] + [0] * (4 - n)
        exact_d = [p[2] for p in big.dst_planes] + [0] * (4 - n)
        assert big.call(S, src_pitch=exact_s, dst_pitch=exact_d, conv_pitch=big.conv_row) == E_NODEVICE
        assert big.call(S, src_pitch=[0] * 4, dst_pitch=None, conv_pitch=0) == E_NODEVICE


@pytest.mark.parametrize("layout", [INTER, PLANAR])
def test_odd_addresses_and_pitches_above_8_bits(S, layout):
    f = Image(S, layout=layout, alpha=1, depth=10, src_pitch=[256] * 4, dst_pitch=[256] * 4, conv_pitch=256)
    for k in range(f.np):
        src = list(f.src); src[k] += 1
        assert f.call(S, src=src) == E_ARG, ("src", k)
        dst = list(f.dst); dst[k] += 1
        assert f.call(S, dst=dst) == E_ARG, ("dst", k)
        sp = [256] * 4; sp[k] = 257
        assert f.call(S, src_pitch=sp) == E_ARG
        dp = [256] * 4; dp[k] = 255
        assert f.call(S, dst_pitch=dp) == E_ARG
    assert f.call(S, conv=f.conv + 1) == E_ARG
    assert f.call(S, conv_pitch=257) == E_ARG
    if S.device_count() == 0:
        g = Image(S, layout=layout, alpha=1, depth=8, src_pitch=[257] * 4, dst_pitch=[255] * 4, conv_pitch=63)   # depth 8: no alignment rule
        src = list(g.src); src[0] += 1
        assert g.call(S, src=src, conv=g.conv + 1) == E_NODEVICE


def test_multiply_and_size_limits(S):
    f = Image(S)
    for mul in (0.0, -1.0, 0.1, 0.05, float("nan")):
        assert f.call(S, multiply=mul) == E_SCALE, mul
    assert f.call(S, w=1 << 22, h=2, multiply=4.0) == E_UNSUPPORTED
    assert f.call(S, w=2, h=1 << 20, multiply=2.0) == E_UNSUPPORTED
    assert f.call(S, w=60000, h=60000, multiply=2.0) == E_UNSUPPORTED
    assert f.call(S, multiply=float("inf")) == E_UNSUPPORTED


@pytest.mark.parametrize("layout", [INTER, PLANAR])
@pytest.mark.parametrize("depth", [8, 10])
def test_overlapping_planes(S, layout, depth):
    f = Image(S, layout=layout, alpha=1, depth=depth)
    outs = [("dst", b) for b in range(f.np)] + [("conv", 0)]

    def moved(which, b, addr):
        dst, conv = list(f.dst), f.conv
        if which == "dst":
            dst[b] = addr
        else:
            conv = addr
        return dict(dst=dst, conv=conv)
    for a in range(f.np):                                 # every input plane against every output plane, dst_conv included
        for (which, b) in outs:
            assert f.call(S, **moved(which, b, f.src[a])) == E_ARG, (a, which, b)                        # same start
            assert f.call(S, **moved(which, b, f.src[a] + f.src_sizes[a] - 2)) == E_ARG, (a, which, b)   # starts on the input's last sample
    # an output that ends on the first sample of an input
    assert f.call(S, **moved("dst", 0, f.src[0] - f.dst_sizes[0] + 2)) == E_ARG
    # two output planes over each other
    for i, (wa, a) in enumerate(outs):
        for (wb, b) in outs[i + 1:]:
            addr = f.dst[a] if wa == "dst" else f.conv
            size = f.dst_sizes[a] if wa == "dst" else f.conv_size
            assert f.call(S, **moved(wb, b, addr)) == E_ARG, (wa, a, wb, b)
            assert f.call(S, **moved(wb, b, addr + size - 2)) == E_ARG, (wa, a, wb, b)


def test_valid_calls_without_a_device(S):
    if S.device_count() > 0:
        pytest.skip("a device is present: a valid call would run on host memory")
    for layout in (INTER, PLANAR):
        for order in (RGB, BGR):
            for alpha in (0, 1):
                for depth in DEPTHS:
                    for (w, h, mul) in ((9, 7, 2.0), (1, 1, 3.0), (16, 8, 0.75), (5, 5, 1.0)):
                        assert Image(S, layout, order, alpha, depth, w, h, mul).call(S) == E_NODEVICE
