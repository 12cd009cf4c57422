"""CPU: the packed YUV rect extension (include/srcnn_amd_yuv_packed_rect.h) -- its declared functions, committed list, binding and
export table agree (full and strict-only builds), the header is C99, no older header knows the names,
srcnn_yuv_packed_span_bytes matches the numpy restatement of the ten layouts (row_bytes / pack of tests/test_gpu_yuv_packed.py),
srcnn_yuv_packed_rect_source matches a restatement built on the oracle's contribution tables, and every argument rule of
srcnn_yuv_packed_upscale_rect_dev returns its code, in the header's order, before any device lookup (host buffers stand in for
device frames)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from test_abi import HANDLE_ONLY_HOOKS

import test_yuv_rect_abi as YA
from test_gpu_yuv_packed import FORMATS, NAMES, frame_planes, pack, row_bytes
from test_rect_abi import _declared, _exported, axis_span
from test_rgb_rect_abi import chroma_span
from yuv_packed_rect_worker import UNIT, UNIT_BYTES, span

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_ARG, E_SCALE, E_NODEVICE, E_UNSUPPORTED = -1, -2, -200, -203
OLDER = YA.OLDER + ("srcnn_amd_yuv_rect.h",)
SYMBOLS = ["srcnn_yuv_packed_rect_abi_version", "srcnn_yuv_packed_rect_source", "srcnn_yuv_packed_span_bytes", "srcnn_yuv_packed_upscale_rect_dev"]


@pytest.fixture(scope="module")
def S():
    import libsrcnn_amd as S
    from libsrcnn_amd import build
    if build.stale():
        build.build(verbose=False)
    return S


def test_header_list_binding_and_exports_agree(S):
    names = _declared("srcnn_amd_yuv_packed_rect.h")
    listed = [ln.strip() for ln in open(os.path.join(ROOT, "include", "srcnn_amd_yuv_packed_rect.abi")) if ln.strip() and not ln.startswith("#")]
    assert listed == sorted(listed) and len(set(listed)) == len(listed)
    assert names == listed == sorted(S.YUV_PACKED_RECT_SYMBOLS) == sorted(SYMBOLS)
    assert set(S.YUV_PACKED_RECT_SYMBOLS) <= set(S.C_ABI_SYMBOLS)
    header = open(os.path.join(ROOT, "include", "srcnn_amd_yuv_packed_rect.h")).read()
    assert "#define SRCNN_AMD_YUV_PACKED_RECT_VERSION 1" in header and '#include "srcnn_amd_yuv_packed.h"' in header
    exported = _exported(S.LIB_PATH)
    assert set(names) <= set(exported)
    assert exported == sorted(S.C_ABI_SYMBOLS + S.CXX_SYMBOLS + HANDLE_ONLY_HOOKS)
    assert S.lib().srcnn_yuv_packed_rect_abi_version() == 1


def test_no_older_header_mentions_the_new_names():
    for other in OLDER:
        text = open(os.path.join(ROOT, "include", other)).read()
        assert not set(SYMBOLS) & set(_declared(other)), other
        assert not any(n in text for n in SYMBOLS) and "srcnn_amd_yuv_packed_rect" not in text.lower(), other


def test_strict_only_build_exports_the_same_set(S):
    from libsrcnn_amd import build
    strict, _ = build.build_strict_only(verbose=False)
    assert _exported(strict) == _exported(S.LIB_PATH)
    assert set(SYMBOLS) <= set(_exported(strict))


def test_header_compiles_as_c99(tmp_path):
    src = tmp_path / "use.c"
    src.write_text('#include "srcnn_amd_yuv_packed_rect.h"\n'
                   "int f(const void* s, void* d) { unsigned a, b, c, e; size_t o, n;\n"
                   "  return srcnn_yuv_packed_rect_abi_version() + srcnn_yuv_packed_span_bytes(SRCNN_YUVP_V210, 140, 6, 12, &a, &o, &n)\n"
                   "  + srcnn_yuv_packed_rect_source(SRCNN_YUVP_Y410, 8, 8, 2.f, SRCNN_FILTER_BICUBIC, 2, 2, 3, 4, &a, &b, &c, &e)\n"
                   "  + srcnn_yuv_packed_upscale_rect_dev(SRCNN_YUVP_YUY2, 8, 8, 2.f, SRCNN_FILTER_BICUBIC, s, 0, 2, 2, 4, 4, d, 0, 0)\n"
                   "  + SRCNN_AMD_YUV_PACKED_RECT_VERSION; }\n")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-c", str(src), "-I" + os.path.join(ROOT, "include"),
                           "-o", str(tmp_path / "use.o")])


def test_settings_table_has_the_switch(S):
    assert "SRCNN_YUV_PACKED_RECT_UNFUSED=0" in S.debug_settings()


# ---- srcnn_yuv_packed_span_bytes ----
WIDTHS = {name: sorted(set(range(1, 3 * UNIT[name] + 2)) | {47, 48, 49, 97, 140}) for name in NAMES}


@pytest.mark.parametrize("name", NAMES)
def test_span_bytes_matches_the_restated_layouts(S, name):
    """The unit, offset and length against the arithmetic restated in tests/yuv_packed_rect_worker.py, and against the bytes
    themselves: pack() a row whose every pixel is distinct, and the span of pixels [x, x + n) is exactly the bytes that change
    when those pixels (and the chroma samples that cover them) change -- plus, at the row's end, the slots without a sample."""
    u = UNIT[name]
    assert {w % u for w in WIDTHS[name]} == set(range(u)) and {47, 48, 49, 97} <= set(WIDTHS[name])
    _id, chroma, depth, adepth, _al = FORMATS[name]
    step = 2 if chroma == "422" else 1
    for width in WIDTHS[name]:
        assert S.yuv_packed_span_bytes(name, width, 0, width) == (u, 0, row_bytes(name, width)) == (u,) + span(name, width, 0, width)
        Y, U, V, A = frame_planes(name, width, 1, 31 * width)
        base = pack(name, Y, U, V, A)
        for x in range(0, width, u):
            for n in sorted({u, 2 * u, 3 * u, width - x}):
                if x + n > width or (n % u and x + n != width):
                    continue
                got = S.yuv_packed_span_bytes(name, width, x, n)
                off, nb = span(name, width, x, n)
                assert got == (u, off, nb), (name, width, x, n, got)
                assert off == x // u * UNIT_BYTES[name] and off + nb <= row_bytes(name, width)
                # flip every bit of the samples of those pixels: every changed byte lies inside the span, and the span's bytes that
                # carry a sample all change
                Y2, U2, V2 = Y.copy(), U.copy(), V.copy()
                A2 = A.copy() if A is not None else None
                maxv = (1 << depth) - 1
                Y2[:, x:x + n] ^= maxv
                cx0, cx1 = x // step, (x + n + step - 1) // step
                U2[:, cx0:cx1] ^= maxv
                V2[:, cx0:cx1] ^= maxv
                if A2 is not None:
                    A2[:, x:x + n] ^= (1 << adepth) - 1
                changed = np.flatnonzero(pack(name, Y2, U2, V2, A2)[0] != base[0])
                assert changed.min() >= off and changed.max() < off + nb, (name, width, x, n)
                assert changed.min() < off + UNIT_BYTES[name] and (x + n == width or changed.max() >= off + nb - UNIT_BYTES[name]), (name, width, x, n)
                if x + n == width:
                    assert off + nb == row_bytes(name, width)
        # the unit rule, and the place in the row
        for (x, n) in ((1, u), (0, u + 1), (u, 1), (0, width + 1), (width, 1), (0, 0), (0xfffffffe, 4)):
            ok = x % u == 0 and 0 < n and x + n <= width and (n % u == 0 or x + n == width)
            if ok:
                continue
            with pytest.raises(S.SrcnnError) as e:
                S.yuv_packed_span_bytes(name, width, x, n)
            assert e.value.code == E_ARG, (name, width, x, n)


def test_span_bytes_v210_rows_and_null_results(S):
    L = S.lib()
    for dw, blocks in ((47, 1), (48, 1), (49, 2), (97, 3), (140, 3)):
        assert S.yuv_packed_span_bytes("v210", dw, 0, dw) == (6, 0, 128 * blocks)
        last = (dw - 1) // 6 * 6
        assert S.yuv_packed_span_bytes("v210", dw, last, dw - last) == (6, last // 6 * 16, 128 * blocks - last // 6 * 16)   # the padding groups
        assert S.yuv_packed_span_bytes("v210", dw, 0, 6) == (6, 0, 16)
    assert S.yuv_packed_span_bytes("yuy2", 5, 4, 1) == (2, 8, 4) and S.yuv_packed_span_bytes("y216", 5, 4, 1) == (2, 16, 8)   # the empty second-Y slot
    assert L.srcnn_yuv_packed_span_bytes(0, 8, 0, 8, None, None, None) == 0
    assert L.srcnn_yuv_packed_span_bytes(-1, 8, 0, 8, None, None, None) == E_ARG and L.srcnn_yuv_packed_span_bytes(10, 8, 0, 8, None, None, None) == E_ARG
    assert L.srcnn_yuv_packed_span_bytes(0, 0, 0, 1, None, None, None) == E_ARG


# ---- srcnn_yuv_packed_rect_source ----
def out_size(w, h, mul):
    m = np.float32(mul)
    return int(np.float32(w) * m), int(np.float32(h) * m)


def snap_x(name, dw, x0, x1):
    u = UNIT[name]
    return x0 - x0 % u, min(dw, -(-x1 // u) * u)


@pytest.mark.parametrize("filt", range(5))
@pytest.mark.parametrize("name", ["uyvy", "y212", "vuya", "y410", "y416", "v210"])
def test_source_rect_matches_the_restatement(S, oracle_lib, name, filt):
    cache = {}

    def tables(f, dst, src):
        if (f, dst, src) not in cache:
            cache[(f, dst, src)] = oracle_lib.axis_table(dst, src, f)[:2]
        return cache[(f, dst, src)]
    rng = np.random.default_rng(4321 + filt)
    u = UNIT[name]
    step = 2 if FORMATS[name][1] == "422" else 1
    n = whole = small = 0
    for (w, h) in YA.SIZES:
        for mul in YA.MULS:
            dw, dh = out_size(w, h, mul)
            if not (dw and dh):
                continue
            cw, dcw = (w + step - 1) // step, (dw + step - 1) // step
            ex, ey = YA.edges(dw), YA.edges(dh)
            xs = [(a, b) for a in ex for b in ex if a < b]
            ys = [(a, b) for a in ey for b in ey if a < b]
            pick = lambda ps: [ps[i] for i in rng.choice(len(ps), min(len(ps), 25), replace=False)]   # noqa: E731
            rects = [(x, ys[rng.integers(len(ys))]) for x in pick(xs)] + [(xs[rng.integers(len(xs))], y) for y in pick(ys)]
            rects += [((0, dw), (0, dh)), ((dw // 2, dw // 2 + 1), (dh // 2, dh // 2 + 1)), ((dw - 1, dw), (dh - 1, dh))]
            for (x0, x1), (y0, y1) in {(snap_x(name, dw, *x), y) for x, y in rects}:
                sx0, sw = axis_span(tables, filt, dw, w, x0, x1)
                sy0, sh = axis_span(tables, filt, dh, h, y0, y1)
                cx0, cx1 = x0 // step, (x1 + step - 1) // step
                ux0, uw = chroma_span(tables, filt, dcw, cw, cx0, cx1)
                uy0, uh = chroma_span(tables, filt, dh, h, y0, y1)
                lx, hx = min(sx0, ux0 * step), max(sx0 + sw, min((ux0 + uw) * step, w))
                lx, hx = lx - lx % u, min(w, -(-hx // u) * u)
                ly, hy = min(sy0, uy0), max(sy0 + sh, uy0 + uh)
                got = S.yuv_packed_rect_source(name, w, h, mul, filt, x0, y0, x1 - x0, y1 - y0)
                assert got == (lx, ly, hx - lx, hy - ly), ((w, h, mul), name, filt, (x0, x1, y0, y1), got, (lx, ly, hx - lx, hy - ly))
                assert lx % u == 0 and ((hx - lx) % u == 0 or hx == w) and hx <= w and hy <= h
                S.yuv_packed_span_bytes(name, w, got[0], got[2])          # the reported rectangle is itself a legal span
                if (x0, x1, y0, y1) == (0, dw, 0, dh):
                    assert got == (0, 0, w, h)                            # a whole-frame rect depends on the whole frame
                    whole += 1
                if x1 - x0 <= u and y1 - y0 == 1 and w * h > 600 and mul >= 1.5:
                    assert got[2] * got[3] < w * h                        # a rect of one unit of an up-scale on a smaller part
                    small += 1
                n += 1
    assert n > 500 and whole >= 15 and small >= 10, (n, whole, small)


def test_source_rect_errors_and_null_results(S):
    L = S.lib()
    u = [C.c_uint() for _ in range(4)]

    def call(fmt, *a):
        return L.srcnn_yuv_packed_rect_source(fmt, *a, *[C.byref(v) for v in u])
    assert call(0, 8, 8, 2.0, 2, 2, 2, 4, 4) == 0
    assert L.srcnn_yuv_packed_rect_source(9, 12, 8, 2.0, 2, 6, 2, 12, 4, None, None, None, None) == 0
    assert call(-1, 8, 8, 2.0, 2, 0, 0, 2, 1) == E_ARG and call(10, 8, 8, 2.0, 2, 0, 0, 2, 1) == E_ARG
    assert call(0, 0, 8, 2.0, 2, 0, 0, 2, 1) == E_ARG and call(0, 8, 0, 2.0, 2, 0, 0, 2, 1) == E_ARG
    assert call(0, 8, 8, 2.0, 2, 0, 0, 0, 1) == E_ARG and call(0, 8, 8, 2.0, 2, 0, 0, 2, 0) == E_ARG
    assert call(0, 8, 8, 0.0, 2, 0, 0, 2, 1) == E_SCALE and call(0, 8, 8, 0.05, 2, 0, 0, 2, 1) == E_SCALE
    assert call(0, 8, 8, 2.0, 5, 0, 0, 2, 1) == E_ARG and call(0, 8, 8, 2.0, -1, 0, 0, 2, 1) == E_ARG
    assert call(0, 8, 8, 2.0, 2, 14, 0, 4, 1) == E_ARG and call(0, 8, 8, 2.0, 2, 0, 16, 2, 1) == E_ARG
    assert call(0, 8, 8, 2.0, 2, 0xfffffffe, 0, 4, 1) == E_ARG
    assert call(0, 8, (1 << 20) + 1, 2.0, 2, 0, 0, 2, 1) == E_UNSUPPORTED
    assert call(0, 8, 8, 2.0, 2, 1, 0, 2, 1) == E_ARG and call(0, 8, 8, 2.0, 2, 0, 0, 3, 1) == E_ARG        # the unit rule: YUY2, 2
    assert call(0, 8, 8, 2.0, 2, 14, 0, 2, 1) == 0 and call(3, 9, 8, 1.0, 2, 8, 0, 1, 1) == 0                # ... the row's end at a partial unit
    assert call(7, 8, 8, 2.0, 2, 1, 1, 1, 1) == 0                                                            # Y410: 1
    assert call(9, 12, 8, 2.0, 2, 2, 0, 6, 1) == E_ARG and call(9, 12, 8, 2.0, 2, 6, 0, 4, 1) == E_ARG       # v210: 6
    assert call(9, 12, 8, 2.0, 2, 18, 0, 6, 1) == 0 and call(9, 10, 8, 2.0, 2, 18, 0, 2, 1) == 0
    assert call(0, 8, 8, 0.0, 2, 1, 0, 2, 1) == E_SCALE             # the scale before the rect's place and the unit rule
    assert call(0, 8, 8, 2.0, 2, 15, 0, 2, 1) == E_ARG              # not inside (and odd: the place comes first, both E_ARG)


# ---- argument rules: host buffers stand in for device frames, which is safe because every call below is refused before the
# device is looked up ----
class Frame:
    """Host memory laid out like one packed frame and the rect's row segments: tight unless pitches are given; both 16-aligned."""

    def __init__(self, S, name="y210", w=9, h=7, mul=2.0, rect=(2, 2, 8, 7), src_pitch=0, dst_pitch=0):
        self.name, self.w, self.h, self.mul, self.rect = name, w, h, mul, rect
        self.dw, self.dh = S.output_size(w, h, mul)
        self.src_rb = row_bytes(name, w)
        self.n = span(name, self.dw, rect[0], rect[2])[1]
        self.src_size = (max(src_pitch, self.src_rb) * h + 15) & ~15
        self.dst_size = (max(dst_pitch, self.n) * rect[3] + 15) & ~15
        self.buf = np.zeros(self.src_size + self.dst_size + 64, np.uint8)
        base = (self.buf.ctypes.data + 15) & ~15
        self.src, self.dst = base, base + self.src_size
        self.src_pitch, self.dst_pitch = src_pitch, dst_pitch

    def call(self, S, **kw):
        a = dict(name=self.name, w=self.w, h=self.h, multiply=self.mul, filt=2, src=self.src, src_pitch=self.src_pitch,
                 x0=self.rect[0], y0=self.rect[1], rw=self.rect[2], rh=self.rect[3], dst=self.dst, dst_pitch=self.dst_pitch)
        a.update(kw)
        try:
            S.yuv_packed_upscale_rect_dev(a["name"], a["w"], a["h"], a["multiply"], a["filt"], a["src"], a["src_pitch"], a["x0"], a["y0"],
                                          a["rw"], a["rh"], a["dst"], a["dst_pitch"])
        except S.SrcnnError as e:
            return e.code
        return 0


def test_the_error_order_case_by_case(S):
    f = Frame(S)                                          # Y210 9 x 7 -> 18 x 14, rect 8 x 7 at (2, 2)
    assert (f.dw, f.dh) == (18, 14)
    ok = E_NODEVICE if S.device_count() == 0 else None
    # format / NULL / zero size / filter
    assert f.call(S, name=-1) == E_ARG and f.call(S, name=10) == E_ARG and f.call(S, name="nv12") == E_ARG
    assert f.call(S, name=-1, multiply=0.0) == E_ARG      # the format before everything else
    assert f.call(S, src=None) == E_ARG and f.call(S, dst=None) == E_ARG
    for k in ("w", "h", "rw", "rh"):
        assert f.call(S, **{k: 0}) == E_ARG, k
    for filt in (-1, 5, 100):
        assert f.call(S, filt=filt) == E_ARG
    assert f.call(S, rw=0, multiply=0.0) == E_ARG and f.call(S, filt=7, multiply=0.0) == E_ARG    # ... before the scale
    # the scale, then the limits
    for mul in (0.0, -1.0, 0.1, 0.05, float("nan")):
        assert f.call(S, multiply=mul) == E_SCALE, mul
    assert f.call(S, w=1 << 22, h=2, multiply=4.0) == E_UNSUPPORTED and f.call(S, w=2, h=1 << 20, multiply=2.0) == E_UNSUPPORTED
    assert f.call(S, w=60000, h=60000, multiply=2.0) == E_UNSUPPORTED and f.call(S, multiply=float("inf")) == E_UNSUPPORTED
    assert f.call(S, x0=12, multiply=0.0) == E_SCALE and f.call(S, x0=3, multiply=0.0) == E_SCALE and f.call(S, src_pitch=2, multiply=0.0) == E_SCALE
    assert f.call(S, x0=12, w=2, h=1 << 20) == E_UNSUPPORTED
    # 1. the rect's place (without 32-bit wrap)
    assert f.call(S, x0=12) == E_ARG and f.call(S, y0=8) == E_ARG and f.call(S, x0=18, rw=2) == E_ARG and f.call(S, y0=14, rh=1) == E_ARG
    assert f.call(S, x0=0xfffffffe, rw=4) == E_ARG and f.call(S, y0=0xfffffffc, rh=6) == E_ARG
    # 2. the unit rule
    assert f.call(S, x0=3) == E_ARG and f.call(S, rw=7) == E_ARG and f.call(S, x0=1, rw=17) == E_ARG
    for name, bad, good in (("yuy2", (1, 2), (16, 2)), ("y216", (2, 3), (2, 16)), ("vuya", None, (3, 5)), ("y410", None, (17, 1)), ("y416", None, (1, 1)),
                            ("v210", (2, 6), (6, 12)), ("v210", (6, 8), (12, 6)), ("v210", (3, 15), (0, 18))):
        g = Frame(S, name=name, rect=(good[0], 2, good[1], 7))
        if ok is not None:                                # (with a device present a valid call would run on host memory)
            assert g.call(S) == ok, (name, good)
        if bad:
            assert g.call(S, x0=bad[0], rw=bad[1]) == E_ARG, (name, bad)
    # 3. pitch and alignment
    assert f.call(S, src_pitch=f.src_rb - 2) == E_ARG and f.call(S, dst_pitch=f.n - 2) == E_ARG
    assert f.call(S, src=f.src + 1) == E_ARG and f.call(S, dst=f.dst + 1) == E_ARG and f.call(S, src_pitch=f.src_rb + 1) == E_ARG and f.call(S, dst_pitch=f.n + 1) == E_ARG
    v = Frame(S, name="v210", rect=(6, 2, 6, 7))
    assert v.n == 16 and v.call(S, dst=v.dst + 2) == E_ARG and v.call(S, dst_pitch=18) == E_ARG and v.call(S, dst_pitch=12) == E_ARG
    y = Frame(S, name="yuy2", rect=(2, 2, 8, 7), src_pitch=41, dst_pitch=17)            # alignment 1: anything goes
    if ok is not None:
        assert y.call(S, src=y.src + 1, dst=y.dst + 3) == ok
        assert f.call(S, src_pitch=f.src_rb, dst_pitch=f.n) == ok and f.call(S) == ok     # the rect's span is enough: not the dw-pixel row
    assert f.n == 32 and f.n < row_bytes("y210", 18)


def test_the_overlap_rule(S):
    f = Frame(S)
    assert f.call(S, dst=f.src) == E_ARG                                        # the first byte of the source
    assert f.call(S, dst=f.src + f.src_rb * f.h - 2) == E_ARG                   # its last word
    assert f.call(S, dst=f.src - (f.n * f.rect[3]) + 2) == E_ARG                # ends on the source's first word
    # repainting a rect of the surface the source frame lives in, whatever the pitch
    g = Frame(S, name="yuy2", w=16, h=12, mul=1.0, rect=(4, 2, 6, 4))
    assert g.call(S, dst=g.src + 2 * g.src_rb + span("yuy2", 16, 4, 6)[0], dst_pitch=g.src_rb) == E_ARG
    if S.device_count() == 0:
        assert f.call(S, dst=f.src + f.src_rb * f.h) == E_NODEVICE              # right behind the source is fine
        assert g.call(S) == E_NODEVICE


def test_valid_calls_without_a_device(S):
    if S.device_count() > 0:
        pytest.skip("a device is present: a valid call would run on host memory")
    for name in NAMES:
        u = UNIT[name]
        for (w, h, mul) in ((9, 7, 2.0), (1, 1, 3.0), (16, 8, 0.75), (5, 5, 1.0), (35, 20, 2.5)):
            dw, dh = S.output_size(w, h, mul)
            last = (dw - 1) // u * u
            for rect in ((0, 0, dw, dh), (last, dh - 1, dw - last, 1), (0, 0, min(dw, u), dh)):
                assert Frame(S, name=name, w=w, h=h, mul=mul, rect=rect).call(S) == E_NODEVICE, (name, w, h, mul, rect)
