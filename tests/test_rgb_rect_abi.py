"""CPU: the RGB(A) rect extension (include/srcnn_amd_rgb_rect.h) -- its declared functions, committed list, binding and export
table agree (full and strict-only builds), the header is C99, no older header knows the names, srcnn_rgb_rect_source matches
a restatement built on the oracle's contribution tables (the Y rule of tests/test_rect_abi.py united with the chroma filter's
first and last tap), every argument rule of srcnn_rgb_upscale_rect_dev returns its code before any device lookup (host buffers
stand in for device planes), and the layer kernels' fingerprints are still the ones tests/test_rect_abi.py pins."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from test_abi import HANDLE_ONLY_HOOKS

import test_rect_abi as RA
from test_rect_abi import _declared, _exported, axis_span, edges

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_ARG, E_SCALE, E_NODEVICE, E_UNSUPPORTED = -1, -2, -200, -203
OLDER = RA.OLDER + ("srcnn_amd_rect.h",)
NAMES = ["srcnn_rgb_rect_abi_version", "srcnn_rgb_rect_source", "srcnn_rgb_upscale_rect_dev"]
INTER, PLANAR, RGB, BGR = 0, 1, 0, 1


@pytest.fixture(scope="module")
def S():
    import libsrcnn_amd as S
    from libsrcnn_amd import build
    if build.stale():
        build.build(verbose=False)
    return S


def test_header_list_binding_and_exports_agree(S):
    names = _declared("srcnn_amd_rgb_rect.h")
    listed = [ln.strip() for ln in open(os.path.join(ROOT, "include", "srcnn_amd_rgb_rect.abi")) if ln.strip() and not ln.startswith("#")]
    assert listed == sorted(listed) and len(set(listed)) == len(listed)
    assert names == listed == sorted(S.RGB_RECT_SYMBOLS) == sorted(NAMES)
    assert set(S.RGB_RECT_SYMBOLS) <= set(S.C_ABI_SYMBOLS)
    header = open(os.path.join(ROOT, "include", "srcnn_amd_rgb_rect.h")).read()
    assert "#define SRCNN_AMD_RGB_RECT_VERSION 1" in header and '#include "srcnn_amd_rgb.h"' in header
    exported = _exported(S.LIB_PATH)
    assert set(names) <= set(exported)
    assert exported == sorted(S.C_ABI_SYMBOLS + S.CXX_SYMBOLS + HANDLE_ONLY_HOOKS)
    assert S.lib().srcnn_rgb_rect_abi_version() == 1


def test_no_older_header_mentions_the_new_names():
    for other in OLDER:
        text = open(os.path.join(ROOT, "include", other)).read()
        assert not set(NAMES) & set(_declared(other)), other
        assert not any(n in text for n in NAMES) and "srcnn_amd_rgb_rect" not in text.lower(), other


def test_header_is_not_installed_by_make_install():
    mk = open(os.path.join(ROOT, "Makefile")).read()
    install = re.search(r"^install: all\n((?:\t.*\n)+)", mk, flags=re.M).group(1)
    assert "rgb_rect" not in install


def test_strict_only_build_exports_the_same_set(S):
    from libsrcnn_amd import build
    strict, _ = build.build_strict_only(verbose=False)
    assert _exported(strict) == _exported(S.LIB_PATH)
    assert set(NAMES) <= set(_exported(strict))


def test_header_compiles_as_c99(tmp_path):
    src = tmp_path / "use.c"
    src.write_text('#include "srcnn_amd_rgb_rect.h"\n'
                   "int f(const void* const s[4], void* const d[4], const size_t p[4]) { unsigned a, b, c, e;\n"
                   "  srcnn_rgb_format fmt = {sizeof(srcnn_rgb_format), SRCNN_RGB_INTERLEAVED, SRCNN_RGB_ORDER_RGB, 0, 8};\n"
                   "  return srcnn_rgb_rect_abi_version() + srcnn_rgb_rect_source(8, 8, 2.f, SRCNN_FILTER_BICUBIC, 1, 2, 3, 4, &a, &b, &c, &e)\n"
                   "  + srcnn_rgb_upscale_rect_dev(&fmt, 8, 8, 2.f, SRCNN_FILTER_BICUBIC, s, p, 1, 2, 3, 4, d, p, 0, 0, 0)\n"
                   "  + SRCNN_AMD_RGB_RECT_VERSION; }\n")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-c", str(src), "-I" + os.path.join(ROOT, "include"),
                           "-o", str(tmp_path / "use.o")])


def test_settings_table_has_the_switch(S):
    assert "SRCNN_RGB_RECT_UNFUSED=0" in S.debug_settings()


# ---- srcnn_rgb_rect_source ----
SHAPES = [(70, 40, 2.0), (40, 31, 1.5), (50, 30, 0.75), (24, 24, 1.0), (1, 17, 2.0)]


def chroma_span(tables, filt, dst, src, a, b):
    """First and last tap of the chroma filter (box for nearest, bilinear otherwise) over [a, b); a kept size is copied."""
    if dst == src:
        return a, b - a
    left, right = tables(0 if filt == 0 else 1, dst, src)
    lo, hi = int(left[a:b].min()), int(right[a:b].max()) + 1
    return lo, hi - lo


def union(p, q):
    lo = min(p[0], q[0])
    return lo, max(p[0] + p[1], q[0] + q[1]) - lo


@pytest.mark.parametrize("filt", range(5))
def test_source_rect_matches_the_restatement(S, oracle_lib, filt):
    cache = {}

    def tables(f, dst, src):
        if (f, dst, src) not in cache:
            cache[(f, dst, src)] = oracle_lib.axis_table(dst, src, f)[:2]
        return cache[(f, dst, src)]
    rng = np.random.default_rng(4321 + filt)
    n = 0
    for (w, h, mul) in SHAPES:
        dw, dh = S.output_size(w, h, mul)
        ex, ey = edges(dw), edges(dh)
        xs = [(a, b) for a in ex for b in ex if a < b]
        ys = [(a, b) for a in ey for b in ey if a < b]
        rects = [(x, ys[rng.integers(len(ys))]) for x in xs] + [(xs[rng.integers(len(xs))], y) for y in ys]
        rects += [((0, dw), (0, dh)), ((dw // 2, dw // 2 + 1), (dh // 2, dh // 2 + 1))]
        for (x0, x1), (y0, y1) in rects:
            sx0, sw = union(axis_span(tables, filt, dw, w, x0, x1), chroma_span(tables, filt, dw, w, x0, x1))
            sy0, sh = union(axis_span(tables, filt, dh, h, y0, y1), chroma_span(tables, filt, dh, h, y0, y1))
            got = S.rgb_rect_source(w, h, mul, filt, x0, y0, x1 - x0, y1 - y0)
            assert got == (sx0, sy0, sw, sh), ((w, h, mul), filt, (x0, x1, y0, y1), got, (sx0, sy0, sw, sh))
            assert sx0 + sw <= w and sy0 + sh <= h and sw > 0 and sh > 0
            ysrc = S.y_path_rect_source(w, h, dw, dh, filt, x0, y0, x1 - x0, y1 - y0)
            assert sx0 <= ysrc[0] and ysrc[0] + ysrc[2] <= sx0 + sw and sy0 <= ysrc[1] and ysrc[1] + ysrc[3] <= sy0 + sh
            n += 1
    assert n > 300


def test_source_rect_errors_and_null_results(S):
    L = S.lib()
    u = [C.c_uint() for _ in range(4)]
    call = lambda *a: L.srcnn_rgb_rect_source(*a, *[C.byref(v) for v in u])   # noqa: E731
    assert call(8, 8, 2.0, 2, 1, 2, 3, 4) == 0
    assert L.srcnn_rgb_rect_source(8, 8, 2.0, 2, 1, 2, 3, 4, None, None, None, None) == 0
    assert call(0, 8, 2.0, 2, 0, 0, 1, 1) == E_ARG and call(8, 0, 2.0, 2, 0, 0, 1, 1) == E_ARG
    assert call(8, 8, 2.0, 2, 0, 0, 0, 1) == E_ARG and call(8, 8, 2.0, 2, 0, 0, 1, 0) == E_ARG
    assert call(8, 8, 0.0, 2, 0, 0, 1, 1) == E_SCALE and call(8, 8, 0.05, 2, 0, 0, 1, 1) == E_SCALE
    assert call(8, 8, 2.0, 5, 0, 0, 1, 1) == E_ARG and call(8, 8, 2.0, -1, 0, 0, 1, 1) == E_ARG
    assert call(8, 8, 2.0, 2, 14, 0, 3, 1) == E_ARG and call(8, 8, 2.0, 2, 0, 16, 1, 1) == E_ARG
    assert call(8, 8, 2.0, 2, 0xffffffff, 0, 2, 1) == E_ARG
    assert call(8, (1 << 20) + 1, 2.0, 2, 0, 0, 1, 1) == E_UNSUPPORTED


# ---- argument rules: host buffers stand in for device planes, which is safe because every call below is refused before the
# device is looked up ----
class Image:
    """Host memory laid out like one image's planes and the rect's, dst_conv last: tight unless pitches are given; every plane
    starts on an even address."""

    def __init__(self, S, layout=INTER, order=RGB, alpha=0, depth=10, w=9, h=7, mul=2.0, rect=(3, 2, 8, 6), src_pitch=None,
                 dst_pitch=None, conv=True, conv_pitch=0):
        self.fmt = S.rgb_format(layout, order, alpha, depth)
        self.w, self.h, self.mul, self.rect = w, h, mul, rect
        self.np = (3 + alpha) if layout == PLANAR else 1
        self.dw, self.dh = S.output_size(w, h, mul)
        rw, rh = rect[2], rect[3]
        self.src_planes = [S.rgb_plane_size(self.fmt, w, h, k) for k in range(self.np)]
        self.dst_planes = [S.rgb_plane_size(self.fmt, rw, rh, k) for k in range(self.np)]
        self.conv_row = rw * (1 if depth == 8 else 2)
        sp = src_pitch or [0, 0, 0, 0]
        dp = dst_pitch or [0, 0, 0, 0]
        even = lambda n: (n + 1) & ~1   # noqa: E731
        self.src_sizes = [even(max(sp[k], rb) * r) for k, (_c, r, rb) in enumerate(self.src_planes)]
        self.dst_sizes = [even(max(dp[k], rb) * r) for k, (_c, r, rb) in enumerate(self.dst_planes)]
        self.conv_size = even(max(conv_pitch, self.conv_row) * rh)
        self.buf = np.zeros(sum(self.src_sizes) + sum(self.dst_sizes) + self.conv_size + 64, np.uint16)
        base = self.buf.ctypes.data
        offs = np.cumsum([0] + self.src_sizes + self.dst_sizes)
        self.src = [base + int(o) for o in offs[:self.np]] + [None] * (4 - self.np)
        self.dst = [base + int(o) for o in offs[self.np:2 * self.np]] + [None] * (4 - self.np)
        self.conv = base + int(offs[2 * self.np]) if conv else None
        self.src_pitch, self.dst_pitch, self.conv_pitch = src_pitch, dst_pitch, conv_pitch

    def call(self, S, **kw):
        a = dict(fmt=self.fmt, w=self.w, h=self.h, multiply=self.mul, filt=2, src=self.src, src_pitch=self.src_pitch,
                 x0=self.rect[0], y0=self.rect[1], rw=self.rect[2], rh=self.rect[3],
                 dst=self.dst, dst_pitch=self.dst_pitch, conv=self.conv, conv_pitch=self.conv_pitch)
        a.update(kw)
        try:
            S.rgb_upscale_rect_dev(a["fmt"], a["w"], a["h"], a["multiply"], a["filt"], a["src"], a["src_pitch"], a["x0"], a["y0"],
                                   a["rw"], a["rh"], a["dst"], a["dst_pitch"], a["conv"], a["conv_pitch"])
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
    for k in ("w", "h", "rw", "rh"):
        assert f.call(S, **{k: 0}) == E_ARG, k
    if S.device_count() == 0:
        junk = 1 if depth == 8 else 2
        src = list(f.src); dst = list(f.dst)
        for k in range(f.np, 4):
            src[k] = junk * (k + 1); dst[k] = junk * (k + 1)
        assert f.call(S, src=src, dst=dst) == E_NODEVICE
        assert f.call(S, conv=None) == E_NODEVICE


def test_rect_rules(S):
    f = Image(S)                                         # 9 x 7 -> 18 x 14, rect 8 x 6 at (3, 2)
    assert (f.dw, f.dh) == (18, 14)
    assert f.call(S, x0=11) == E_ARG                      # 11 + 8 > 18
    assert f.call(S, y0=9) == E_ARG                       # 9 + 6 > 14
    assert f.call(S, x0=18, rw=1) == E_ARG and f.call(S, y0=14, rh=1) == E_ARG
    assert f.call(S, x0=0xfffffffe, rw=4) == E_ARG        # the sum wraps in 32 bits
    assert f.call(S, y0=0xfffffffd, rh=6) == E_ARG
    assert f.call(S, rw=0, multiply=0.0) == E_ARG         # the order of the header: an empty rect before the scale
    assert f.call(S, x0=11, multiply=0.0) == E_SCALE      # ... and the scale before the rect's place in the output
    big = Image(S, rect=(0, 0, 18, 14))
    assert big.call(S, rw=19) == E_ARG and big.call(S, rh=15) == E_ARG
    if S.device_count() == 0:
        assert big.call(S) == E_NODEVICE
        assert Image(S, rect=(17, 13, 1, 1)).call(S) == E_NODEVICE


@pytest.mark.parametrize("layout", [INTER, PLANAR])
@pytest.mark.parametrize("alpha", [0, 1])
@pytest.mark.parametrize("depth", [8, 12])
def test_short_pitches(S, layout, alpha, depth):
    big = Image(S, layout=layout, alpha=alpha, depth=depth, src_pitch=[512] * 4, dst_pitch=[512] * 4, conv_pitch=512)
    n = big.np
    step = 1 if depth == 8 else 2
    for k in range(n):
        sp = [0] * 4; sp[k] = big.src_planes[k][2] - step
        assert big.call(S, src_pitch=sp) == E_ARG, ("src", k)
        dp = [0] * 4; dp[k] = big.dst_planes[k][2] - step                  # destination rows are rw pixels
        assert big.call(S, dst_pitch=dp) == E_ARG, ("dst", k)
    assert big.call(S, conv_pitch=big.conv_row - step) == E_ARG
    if S.device_count() == 0:
        exact_s = [p[2] for p in big.src_planes] + [0] * (4 - n)
        exact_d = [p[2] for p in big.dst_planes] + [0] * (4 - n)           # the row of rw pixels is enough: not the dw-pixel row
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
        dst = list(g.dst); dst[0] += 1
        assert g.call(S, src=src, dst=dst, conv=g.conv + 1) == E_NODEVICE


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
    for a in range(f.np):                                 # every WHOLE input plane against every plane of the rect, dst_conv included
        for (which, b) in outs:
            assert f.call(S, **moved(which, b, f.src[a])) == E_ARG, (a, which, b)
            assert f.call(S, **moved(which, b, f.src[a] + f.src_sizes[a] - 2)) == E_ARG, (a, which, b)
    assert f.call(S, **moved("dst", 0, f.src[0] - f.dst_sizes[0] + 2)) == E_ARG     # ends on the first sample of an input
    for i, (wa, a) in enumerate(outs):                    # two planes of the rect over each other
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
                for depth in (8, 10, 12, 14, 16):
                    for (w, h, mul) in ((9, 7, 2.0), (1, 1, 3.0), (16, 8, 0.75), (5, 5, 1.0)):
                        dw, dh = S.output_size(w, h, mul)
                        for rect in ((0, 0, dw, dh), (dw - 1, dh - 1, 1, 1), (dw // 2, 0, dw - dw // 2, dh)):
                            f = Image(S, layout=layout, order=order, alpha=alpha, depth=depth, w=w, h=h, mul=mul, rect=rect)
                            assert f.call(S) == E_NODEVICE, (layout, order, alpha, depth, w, h, mul, rect)
    # a rect inside a full-size image: the address of pixel (x0, y0) and the image's pitch; it ends right before the source
    f = Image(S, depth=8, rect=(3, 2, 8, 6))
    pitch = 3 * f.dw
    full = np.zeros(pitch * f.dh + f.src_sizes[0], np.uint8)
    base = full.ctypes.data
    assert f.call(S, src=[base + pitch * f.dh] + [None] * 3, dst=[base + 2 * pitch + 3 * 3] + [None] * 3, dst_pitch=[pitch, 0, 0, 0],
                  conv=None) == E_NODEVICE


def test_layer_kernel_fingerprints_are_the_parents():
    """The colour shell over a window adds kernels and leaves the layer kernels' text alone: the fingerprints are the values
    tests/test_rect_abi.py pins."""
    import inspect
    from libsrcnn_amd import build
    pinned = dict(re.findall(r'kernel_source_sha\("(\w+)"\) == "([0-9a-f]{64})"', inspect.getsource(RA.test_layer_kernel_fingerprints_are_the_parents)))
    assert sorted(pinned) == ["k_conv12_mfma", "k_conv3", "k_rs2d_dma"]
    for name, sha in pinned.items():
        assert build.kernel_source_sha(name) == sha, name
    RA.test_layer_kernel_fingerprints_are_the_parents()
