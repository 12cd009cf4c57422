"""CPU: the YUV rect extension (include/srcnn_amd_yuv_rect.h) -- its declared functions, committed list, binding and export
table agree (full and strict-only builds), the header is C99, no older header knows the names, srcnn_yuv_rect_source matches
a restatement built on the oracle's contribution tables (plane 0: the Y rule of tests/test_rect_abi.py; chroma planes: the
chroma filter's first and last tap on the chroma grid), every argument rule of srcnn_yuv_upscale_rect_dev returns its code
before any device lookup (host buffers stand in for device planes), and the layer kernels' fingerprints are still the ones
tests/test_rect_abi.py pins."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from test_abi import HANDLE_ONLY_HOOKS

import test_rect_abi as RA
from test_rect_abi import _declared, _exported, axis_span, edges
from test_rgb_rect_abi import chroma_span

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_ARG, E_SCALE, E_NODEVICE, E_UNSUPPORTED = -1, -2, -200, -203
OLDER = RA.OLDER + ("srcnn_amd_rect.h", "srcnn_amd_rgb_rect.h")
NAMES = ["srcnn_yuv_rect_abi_version", "srcnn_yuv_rect_source", "srcnn_yuv_upscale_rect_dev"]
PLANAR, SEMI = 0, 1
CHROMAS = ("420", "422", "444")


@pytest.fixture(scope="module")
def S():
    import libsrcnn_amd as S
    from libsrcnn_amd import build
    if build.stale():
        build.build(verbose=False)
    return S


def test_header_list_binding_and_exports_agree(S):
    names = _declared("srcnn_amd_yuv_rect.h")
    listed = [ln.strip() for ln in open(os.path.join(ROOT, "include", "srcnn_amd_yuv_rect.abi")) if ln.strip() and not ln.startswith("#")]
    assert listed == sorted(listed) and len(set(listed)) == len(listed)
    assert names == listed == sorted(S.YUV_RECT_SYMBOLS) == sorted(NAMES)
    assert set(S.YUV_RECT_SYMBOLS) <= set(S.C_ABI_SYMBOLS)
    header = open(os.path.join(ROOT, "include", "srcnn_amd_yuv_rect.h")).read()
    assert "#define SRCNN_AMD_YUV_RECT_VERSION 1" in header and '#include "srcnn_amd_yuv_ex.h"' in header
    exported = _exported(S.LIB_PATH)
    assert set(names) <= set(exported)
    assert exported == sorted(S.C_ABI_SYMBOLS + S.CXX_SYMBOLS + HANDLE_ONLY_HOOKS)
    assert S.lib().srcnn_yuv_rect_abi_version() == 1


def test_no_older_header_mentions_the_new_names():
    for other in OLDER:
        text = open(os.path.join(ROOT, "include", other)).read()
        assert not set(NAMES) & set(_declared(other)), other
        assert not any(n in text for n in NAMES) and "srcnn_amd_yuv_rect" not in text.lower(), other


def test_header_is_not_installed_by_make_install():
    mk = open(os.path.join(ROOT, "Makefile")).read()
    for target in ("install", "install-yuv", "install-rgb", "install-rect"):
        recipe = re.search(r"^%s: \w+\n((?:\t.*\n)+)" % target, mk, flags=re.M).group(1)
        assert "yuv_rect" not in recipe, target


def test_strict_only_build_exports_the_same_set(S):
    from libsrcnn_amd import build
    strict, _ = build.build_strict_only(verbose=False)
    assert _exported(strict) == _exported(S.LIB_PATH)
    assert set(NAMES) <= set(_exported(strict))


def test_header_compiles_as_c99(tmp_path):
    src = tmp_path / "use.c"
    src.write_text('#include "srcnn_amd_yuv_rect.h"\n'
                   "int f(const void* const s[3], void* const d[3], const size_t p[3]) { unsigned a, b, c, e;\n"
                   "  srcnn_yuv_format fmt = {sizeof(srcnn_yuv_format), SRCNN_YUV_SEMIPLANAR, SRCNN_YUV_420, 10, 1};\n"
                   "  return srcnn_yuv_rect_abi_version() + srcnn_yuv_rect_source(&fmt, 8, 8, 2.f, SRCNN_FILTER_BICUBIC, 2, 2, 3, 4, 1, &a, &b, &c, &e)\n"
                   "  + srcnn_yuv_upscale_rect_dev(&fmt, 8, 8, 2.f, SRCNN_FILTER_BICUBIC, s, p, 2, 2, 3, 4, d, p, 0)\n"
                   "  + SRCNN_AMD_YUV_RECT_VERSION; }\n")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-c", str(src), "-I" + os.path.join(ROOT, "include"),
                           "-o", str(tmp_path / "use.o")])


def test_settings_table_has_the_switch(S):
    assert "SRCNN_YUV_RECT_UNFUSED=0" in S.debug_settings()


# ---- srcnn_yuv_rect_source ----
# odd w, h, dw and dh among them: 35 x 21 x 1.5 -> 52 x 31, x 2.5 -> 87 x 52, x 3 -> 105 x 63; 50 x 30 x 0.75 -> 37 x 22
SIZES = [(70, 40), (35, 21), (50, 30), (1, 17)]
MULS = (0.75, 1.0, 1.5, 2.0, 2.5, 3.0)


def out_size(w, h, mul):
    """srcnn_output_size, restated: the float32 products, truncated (a zero size is a scale error there)."""
    m = np.float32(mul)
    return int(np.float32(w) * m), int(np.float32(h) * m)


def chroma_size(w, h, chroma):
    return (w if chroma == "444" else (w + 1) // 2), ((h + 1) // 2 if chroma == "420" else h)


def snap(rect, chroma):
    """Origins snapped down to even where the format demands it, the far edge kept."""
    (x0, x1), (y0, y1) = rect
    if chroma != "444":
        x0 -= x0 & 1
    if chroma == "420":
        y0 -= y0 & 1
    return (x0, x1), (y0, y1)


def chroma_rect(x0, x1, y0, y1, chroma):
    cx = (x0, x1) if chroma == "444" else (x0 // 2, (x1 + 1) // 2)
    cy = (y0 // 2, (y1 + 1) // 2) if chroma == "420" else (y0, y1)
    return cx, cy


def test_the_sizes_are_odd_in_every_place(S):
    shapes = [(w, h) + out_size(w, h, m) for (w, h) in SIZES for m in MULS if all(out_size(w, h, m))]
    for k in range(4):
        assert any(s[k] % 2 for s in shapes) and any(s[k] % 2 == 0 for s in shapes), k


@pytest.mark.parametrize("filt", range(5))
@pytest.mark.parametrize("chroma", CHROMAS)
def test_source_rect_matches_the_restatement(S, oracle_lib, chroma, filt):
    cache = {}

    def tables(f, dst, src):
        if (f, dst, src) not in cache:
            cache[(f, dst, src)] = oracle_lib.axis_table(dst, src, f)[:2]
        return cache[(f, dst, src)]
    rng = np.random.default_rng(8765 + filt)
    n = 0
    for k, (w, h) in enumerate(SIZES):
        for j, mul in enumerate(MULS):
            dw, dh = out_size(w, h, mul)
            if not (dw and dh):
                continue
            assert (dw, dh) == S.output_size(w, h, mul)
            layout = (k + j) % 2
            fmt = S.yuv_format(layout, chroma, (8, 10, 16)[(k + j) % 3], (k + j) % 3 == 1)
            (cw, ch), (dcw, dch) = chroma_size(w, h, chroma), chroma_size(dw, dh, chroma)
            ex, ey = edges(dw), edges(dh)
            xs = [(a, b) for a in ex for b in ex if a < b]
            ys = [(a, b) for a in ey for b in ey if a < b]
            pick = lambda ps: [ps[i] for i in rng.choice(len(ps), min(len(ps), 40), replace=False)]   # noqa: E731
            rects = [(x, ys[rng.integers(len(ys))]) for x in pick(xs)] + [(xs[rng.integers(len(xs))], y) for y in pick(ys)]
            rects += [((0, dw), (0, dh)), ((dw // 2, dw // 2 + 1), (dh // 2, dh // 2 + 1)), ((dw - 1, dw), (dh - 1, dh))]
            for (x0, x1), (y0, y1) in {snap(r, chroma) for r in rects}:
                args = (fmt, w, h, mul, filt, x0, y0, x1 - x0, y1 - y0)
                sx0, sw = axis_span(tables, filt, dw, w, x0, x1)
                sy0, sh = axis_span(tables, filt, dh, h, y0, y1)
                assert S.yuv_rect_source(*args, 0) == (sx0, sy0, sw, sh) == S.y_path_rect_source(w, h, dw, dh, filt, x0, y0, x1 - x0, y1 - y0)
                (cx0, cx1), (cy0, cy1) = chroma_rect(x0, x1, y0, y1, chroma)
                assert (cx1 - cx0, cy1 - cy0) == chroma_size(x1 - x0, y1 - y0, chroma) and cx1 <= dcw and cy1 <= dch
                ux0, uw = chroma_span(tables, filt, dcw, cw, cx0, cx1)
                uy0, uh = chroma_span(tables, filt, dch, ch, cy0, cy1)
                want = (ux0, uy0, uw, uh)
                got = S.yuv_rect_source(*args, 1)
                assert got == want, ((w, h, mul), chroma, filt, (x0, x1, y0, y1), got, want)
                assert ux0 + uw <= cw and uy0 + uh <= ch and uw > 0 and uh > 0
                assert S.yuv_rect_source(*args, 2) == ((0, 0, 0, 0) if layout == SEMI else want)
                n += 1
    assert n > 1000


def test_source_rect_errors_and_null_results(S):
    L = S.lib()
    u = [C.c_uint() for _ in range(4)]
    f420, f422, f444 = (S.yuv_format(PLANAR, c, 8, 0) for c in CHROMAS)

    def call(fmt, *a):
        return L.srcnn_yuv_rect_source(C.byref(fmt) if fmt is not None else None, *a, *[C.byref(v) for v in u])
    assert call(f420, 8, 8, 2.0, 2, 2, 2, 3, 4, 0) == 0
    assert L.srcnn_yuv_rect_source(C.byref(f420), 8, 8, 2.0, 2, 2, 2, 3, 4, 1, None, None, None, None) == 0
    assert call(None, 8, 8, 2.0, 2, 0, 0, 1, 1, 0) == E_ARG
    bad = S.yuv_format(PLANAR, "420", 9, 0)
    assert call(bad, 8, 8, 2.0, 2, 0, 0, 1, 1, 0) == E_ARG
    assert call(S.yuv_format(PLANAR, "420", 8, 1), 8, 8, 2.0, 2, 0, 0, 1, 1, 0) == E_ARG
    assert call(f420, 8, 8, 2.0, 2, 0, 0, 1, 1, 3) == E_ARG and call(f420, 8, 8, 2.0, 2, 0, 0, 1, 1, -1) == E_ARG
    assert call(f420, 0, 8, 2.0, 2, 0, 0, 1, 1, 0) == E_ARG and call(f420, 8, 0, 2.0, 2, 0, 0, 1, 1, 0) == E_ARG
    assert call(f420, 8, 8, 2.0, 2, 0, 0, 0, 1, 0) == E_ARG and call(f420, 8, 8, 2.0, 2, 0, 0, 1, 0, 0) == E_ARG
    assert call(f420, 8, 8, 0.0, 2, 0, 0, 1, 1, 0) == E_SCALE and call(f420, 8, 8, 0.05, 2, 0, 0, 1, 1, 0) == E_SCALE
    assert call(f420, 8, 8, 2.0, 5, 0, 0, 1, 1, 0) == E_ARG and call(f420, 8, 8, 2.0, -1, 0, 0, 1, 1, 0) == E_ARG
    assert call(f420, 8, 8, 2.0, 2, 14, 0, 3, 1, 0) == E_ARG and call(f420, 8, 8, 2.0, 2, 0, 16, 1, 1, 0) == E_ARG
    assert call(f420, 8, 8, 2.0, 2, 0xfffffffe, 0, 4, 1, 0) == E_ARG
    assert call(f420, 8, (1 << 20) + 1, 2.0, 2, 0, 0, 1, 1, 0) == E_UNSUPPORTED
    for plane in range(3):
        assert call(f420, 8, 8, 2.0, 2, 1, 0, 1, 1, plane) == E_ARG and call(f420, 8, 8, 2.0, 2, 0, 1, 1, 1, plane) == E_ARG
        assert call(f422, 8, 8, 2.0, 2, 1, 0, 1, 1, plane) == E_ARG and call(f422, 8, 8, 2.0, 2, 0, 1, 1, 1, plane) == 0
        assert call(f444, 8, 8, 2.0, 2, 1, 1, 1, 1, plane) == 0
    assert call(f420, 8, 8, 0.0, 2, 1, 0, 1, 1, 0) == E_SCALE          # the scale before the rect's place and parity


# ---- argument rules: host buffers stand in for device planes, which is safe because every call below is refused before the
# device is looked up ----
class Frame:
    """Host memory laid out like one frame's planes and the rect's: tight unless pitches are given; every plane starts on an
    even address."""

    def __init__(self, S, layout=PLANAR, chroma="420", depth=10, msb=0, w=9, h=7, mul=2.0, rect=(2, 2, 9, 7), src_pitch=None, dst_pitch=None):
        self.fmt = S.yuv_format(layout, chroma, depth, msb)
        self.w, self.h, self.mul, self.rect = w, h, mul, rect
        self.np = 2 if layout == SEMI else 3
        self.dw, self.dh = S.output_size(w, h, mul)
        self.src_planes = [S.yuv_plane_size(self.fmt, w, h, k) for k in range(self.np)]
        self.dst_planes = [S.yuv_plane_size(self.fmt, rect[2], rect[3], k) for k in range(self.np)]
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
                 x0=self.rect[0], y0=self.rect[1], rw=self.rect[2], rh=self.rect[3], dst=self.dst, dst_pitch=self.dst_pitch)
        a.update(kw)
        try:
            S.yuv_upscale_rect_dev(a["fmt"], a["w"], a["h"], a["multiply"], a["filt"], a["src"], a["src_pitch"], a["x0"], a["y0"],
                                   a["rw"], a["rh"], a["dst"], a["dst_pitch"])
        except S.SrcnnError as e:
            return e.code
        return 0


def test_format_rules(S):
    f = Frame(S)
    assert f.call(S, fmt=None) == E_ARG
    for size in (0, 4, 19, 21, 24):
        fmt = S.yuv_format(PLANAR, "420", 10, 0)
        fmt.struct_size = size
        assert f.call(S, fmt=fmt) == E_ARG, size
    for layout in (-1, 2, 99):
        assert f.call(S, fmt=S.yuv_format(layout, "420", 10, 0)) == E_ARG
    for chroma in (-1, 3, 99):
        assert f.call(S, fmt=S.yuv_format(PLANAR, chroma, 10, 0)) == E_ARG
    for depth in (0, 7, 9, 11, 13, 15, 17, 32, -10):
        assert f.call(S, fmt=S.yuv_format(PLANAR, "420", depth, 0)) == E_ARG, depth
    for msb in (-1, 2):
        assert f.call(S, fmt=S.yuv_format(PLANAR, "420", 10, msb)) == E_ARG
    assert f.call(S, fmt=S.yuv_format(PLANAR, "420", 8, 1)) == E_ARG
    for filt in (-1, 5, 100):
        assert f.call(S, filt=filt) == E_ARG
    assert f.call(S, fmt=None, multiply=0.0) == E_ARG            # the format before everything else


@pytest.mark.parametrize("layout", [PLANAR, SEMI])
@pytest.mark.parametrize("chroma", CHROMAS)
@pytest.mark.parametrize("depth", [8, 10, 16])
def test_null_planes_and_zero_sizes(S, layout, chroma, depth):
    f = Frame(S, layout=layout, chroma=chroma, depth=depth)
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
        for k in range(f.np, 3):
            src[k] = junk * (k + 1); dst[k] = junk * (k + 1)          # the third plane of a semi-planar frame is ignored
        assert f.call(S, src=src, dst=dst) == E_NODEVICE


def test_rect_rules(S):
    f = Frame(S)                                         # 9 x 7 -> 18 x 14, rect 9 x 7 at (2, 2)
    assert (f.dw, f.dh) == (18, 14)
    assert f.call(S, x0=10) == E_ARG                      # 10 + 9 > 18
    assert f.call(S, y0=8) == E_ARG                       # 8 + 7 > 14
    assert f.call(S, x0=18, rw=1) == E_ARG and f.call(S, y0=14, rh=1) == E_ARG
    assert f.call(S, x0=0xfffffffe, rw=4) == E_ARG        # the sum wraps in 32 bits
    assert f.call(S, y0=0xfffffffc, rh=6) == E_ARG
    assert f.call(S, rw=0, multiply=0.0) == E_ARG         # the order of the header: an empty rect before the scale
    assert f.call(S, x0=10, multiply=0.0) == E_SCALE      # ... the scale before the rect's place in the output
    assert f.call(S, x0=3, multiply=0.0) == E_SCALE       # ... and before its parity
    assert f.call(S, x0=11, src_pitch=[1, 0, 0]) == E_ARG and f.call(S, x0=3, src_pitch=[1, 0, 0]) == E_ARG
    big = Frame(S, rect=(0, 0, 18, 14))
    assert big.call(S, rw=19) == E_ARG and big.call(S, rh=15) == E_ARG
    if S.device_count() == 0:
        assert big.call(S) == E_NODEVICE
        assert Frame(S, rect=(16, 12, 2, 2)).call(S) == E_NODEVICE
        assert Frame(S, chroma="444", rect=(17, 13, 1, 1)).call(S) == E_NODEVICE


@pytest.mark.parametrize("layout", [PLANAR, SEMI])
@pytest.mark.parametrize("depth", [8, 12])
def test_odd_origins(S, layout, depth):
    """Odd x0 is refused where chroma is subsampled horizontally (4:2:0, 4:2:2), odd y0 for 4:2:0 only."""
    ok = E_NODEVICE if S.device_count() == 0 else None
    for chroma, odd_x, odd_y in (("420", E_ARG, E_ARG), ("422", E_ARG, ok), ("444", ok, ok)):
        f = Frame(S, layout=layout, chroma=chroma, depth=depth, rect=(2, 2, 5, 5))
        for (x0, y0, want) in ((3, 2, odd_x), (2, 3, odd_y), (3, 3, odd_x or odd_y), (2, 2, ok), (1, 4, odd_x), (4, 1, odd_y)):
            if want is not None:
                assert f.call(S, x0=x0, y0=y0) == want, (chroma, x0, y0)
        # the geometry function gives the same verdicts without a device
        for (x0, y0, want) in ((3, 2, odd_x), (2, 3, odd_y), (3, 3, odd_x or odd_y), (2, 2, None)):
            try:
                S.yuv_rect_source(f.fmt, f.w, f.h, f.mul, 2, x0, y0, 5, 5, 1)
                code = None
            except S.SrcnnError as e:
                code = e.code
            assert code == (want if want == E_ARG else None), (chroma, x0, y0)


@pytest.mark.parametrize("layout", [PLANAR, SEMI])
@pytest.mark.parametrize("chroma", CHROMAS)
@pytest.mark.parametrize("depth", [8, 12])
def test_short_pitches(S, layout, chroma, depth):
    big = Frame(S, layout=layout, chroma=chroma, depth=depth, src_pitch=[512] * 3, dst_pitch=[512] * 3)
    n = big.np
    step = 1 if depth == 8 else 2
    for k in range(n):
        sp = [0] * 3; sp[k] = big.src_planes[k][2] - step
        assert big.call(S, src_pitch=sp) == E_ARG, ("src", k)
        dp = [0] * 3; dp[k] = big.dst_planes[k][2] - step                  # destination rows are those of an rw x rh frame
        assert big.call(S, dst_pitch=dp) == E_ARG, ("dst", k)
    if S.device_count() == 0:
        exact_s = [p[2] for p in big.src_planes] + [0] * (3 - n)
        exact_d = [p[2] for p in big.dst_planes] + [0] * (3 - n)           # the rect's row is enough: not the dw-sample row
        assert big.call(S, src_pitch=exact_s, dst_pitch=exact_d) == E_NODEVICE
        assert big.call(S, src_pitch=[0] * 3, dst_pitch=None) == E_NODEVICE


@pytest.mark.parametrize("layout", [PLANAR, SEMI])
def test_odd_addresses_and_pitches_above_8_bits(S, layout):
    f = Frame(S, layout=layout, depth=10, msb=1, src_pitch=[256] * 3, dst_pitch=[256] * 3)
    for k in range(f.np):
        src = list(f.src); src[k] += 1
        assert f.call(S, src=src) == E_ARG, ("src", k)
        dst = list(f.dst); dst[k] += 1
        assert f.call(S, dst=dst) == E_ARG, ("dst", k)
        sp = [256] * 3; sp[k] = 257
        assert f.call(S, src_pitch=sp) == E_ARG
        dp = [256] * 3; dp[k] = 255
        assert f.call(S, dst_pitch=dp) == E_ARG
    if S.device_count() == 0:
        g = Frame(S, layout=layout, depth=8, src_pitch=[257] * 3, dst_pitch=[255] * 3)   # depth 8: no alignment rule
        src = list(g.src); src[0] += 1
        dst = list(g.dst); dst[1] += 1
        assert g.call(S, src=src, dst=dst) == E_NODEVICE


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
    f = Frame(S, layout=layout, depth=depth)

    def moved(b, addr):
        dst = list(f.dst)
        dst[b] = addr
        return dict(dst=dst)
    for a in range(f.np):                                 # every WHOLE input plane against every plane of the rect
        for b in range(f.np):
            assert f.call(S, **moved(b, f.src[a])) == E_ARG, (a, b)
            assert f.call(S, **moved(b, f.src[a] + f.src_sizes[a] - 2)) == E_ARG, (a, b)
    assert f.call(S, **moved(0, f.src[0] - f.dst_sizes[0] + 2)) == E_ARG      # ends on the first sample of an input
    for a in range(f.np):                                 # two planes of the rect over each other
        for b in range(a + 1, f.np):
            assert f.call(S, **moved(b, f.dst[a])) == E_ARG, (a, b)
            assert f.call(S, **moved(b, f.dst[a] + f.dst_sizes[a] - 2)) == E_ARG, (a, b)


@pytest.mark.parametrize("layout,depth", [(SEMI, 8), (SEMI, 10), (PLANAR, 8)])
def test_a_destination_inside_the_source_surface_is_refused(S, layout, depth):
    """Repainting a rect of the surface the source frame lives in: the rect's row segments overlap the source plane's byte range,
    whatever the pitch; a surface of its own right behind the source is fine."""
    f = Frame(S, layout=layout, depth=depth, w=16, h=12, mul=1.0, rect=(4, 2, 6, 4))
    bps = 1 if depth == 8 else 2
    pitches = [rb for (_c, _r, rb) in f.src_planes] + [0] * (3 - f.np)
    spp = 2 if layout == SEMI else 1
    inside = [f.src[0] + 2 * pitches[0] + 4 * bps] + [f.src[k] + 1 * pitches[k] + 2 * bps * spp for k in range(1, f.np)] + [None] * (3 - f.np)
    assert f.call(S, dst=inside, dst_pitch=pitches) == E_ARG
    for k in range(f.np):                                 # one plane inside the source is enough
        dst = list(f.dst); dst[k] = inside[k]
        dp = [0, 0, 0]; dp[k] = pitches[k]
        assert f.call(S, dst=dst, dst_pitch=dp) == E_ARG, k
    if S.device_count() == 0:
        assert f.call(S) == E_NODEVICE


def test_valid_calls_without_a_device(S):
    if S.device_count() > 0:
        pytest.skip("a device is present: a valid call would run on host memory")
    for layout in (PLANAR, SEMI):
        for chroma in CHROMAS:
            for (depth, msb) in ((8, 0), (10, 1), (12, 0), (14, 1), (16, 0)):
                for (w, h, mul) in ((9, 7, 2.0), (1, 1, 3.0), (16, 8, 0.75), (5, 5, 1.0)):
                    dw, dh = S.output_size(w, h, mul)
                    for rect in ((0, 0, dw, dh), (dw - 1 - (dw - 1) % 2, dh - 1 - (dh - 1) % 2, 1 + (dw - 1) % 2, 1 + (dh - 1) % 2),
                                 (dw // 2 - (dw // 2) % 2, 0, dw - dw // 2 + (dw // 2) % 2, dh)):
                        f = Frame(S, layout=layout, chroma=chroma, depth=depth, msb=msb, w=w, h=h, mul=mul, rect=rect)
                        assert f.call(S) == E_NODEVICE, (layout, chroma, depth, w, h, mul, rect)
    # a rect inside a full-size NV12 surface: the addresses of luma sample (x0, y0) and of its U, V pair, the surface's pitches,
    # at odd byte offsets of the planes
    f = Frame(S, layout=SEMI, depth=8, rect=(6, 2, 7, 5))
    pitch = f.dw + 3
    full = np.zeros(pitch * (f.dh + (f.dh + 1) // 2) + 8, np.uint8)
    base = full.ctypes.data + 1
    assert f.call(S, dst=[base + 2 * pitch + 6, base + f.dh * pitch + 1 * pitch + 6, None], dst_pitch=[pitch, pitch, 0]) == E_NODEVICE


def test_layer_kernel_fingerprints_are_the_parents():
    """The chroma kernel over a window leaves the layer and resampler kernels' text alone: the fingerprints are the values
    tests/test_rect_abi.py pins."""
    import inspect
    from libsrcnn_amd import build
    pinned = dict(re.findall(r'kernel_source_sha\("(\w+)"\) == "([0-9a-f]{64})"', inspect.getsource(RA.test_layer_kernel_fingerprints_are_the_parents)))
    assert sorted(pinned) == ["k_conv12_mfma", "k_conv3", "k_rs2d_dma"]
    for name, sha in pinned.items():
        assert build.kernel_source_sha(name) == sha, name
    RA.test_layer_kernel_fingerprints_are_the_parents()
