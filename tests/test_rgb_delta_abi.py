"""CPU: the RGB(A) delta extension (include/srcnn_amd_rgb_delta.h) -- its declared functions, committed list, binding and export
table agree (full and strict-only builds), the header is C99, no older header mentions the new names, every argument rule of the
two device calls returns its code before any device lookup and in the header's order (host buffers stand in for device planes),
srcnn_rgb_delta_grid follows its arithmetic up to the limits, and srcnn_rgb_delta_rects follows the coalescer's one rule (a Python
restatement) with every item pointing at pixel (x0, y0) of the full-size image, for every layout x depth class."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from test_abi import HANDLE_ONLY_HOOKS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
E_ARG, E_SCALE, E_NODEVICE, E_UNSUPPORTED = -1, -2, -200, -203
OLDER = ("srcnn_amd.h", "srcnn_amd_debug.h", "srcnn_amd_yuv.h", "srcnn_amd_yuv_ex.h", "srcnn_amd_yuv_packed.h", "srcnn_amd_rgb.h",
         "srcnn_amd_rect.h", "srcnn_amd_rgb_rect.h", "srcnn_amd_yuv_rect.h", "srcnn_amd_yuv_packed_rect.h", "srcnn_amd_rect_list.h",
         "srcnn_amd_rgb_rect_list.h", "srcnn_amd_yuv_rect_list.h", "srcnn_amd_yuv_packed_rect_list.h", "srcnn_amd_delta.h", "libsrcnn_dropin.h")
HEADER = "srcnn_amd_rgb_delta.h"
# layout, alpha, depth -> bytes of a pixel in one plane's row: every class the kernel and the items know
CLASSES = [("interleaved", 0, 8, 3), ("interleaved", 1, 8, 4), ("interleaved", 0, 12, 6), ("interleaved", 1, 16, 8), ("planar", 0, 8, 1),
           ("planar", 1, 8, 1), ("planar", 0, 10, 2), ("planar", 1, 12, 2)]


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


def _code(S, fn):
    try:
        fn()
    except S.SrcnnError as e:
        return e.code
    return 0


def _why(S):
    return S.lib().srcnn_last_error().decode()


def test_header_list_binding_and_exports_agree(S):
    names = _declared(HEADER)
    listed = [ln.strip() for ln in open(os.path.join(ROOT, "include", "srcnn_amd_rgb_delta.abi")) if ln.strip() and not ln.startswith("#")]
    assert listed == sorted(listed) and len(set(listed)) == len(listed)
    assert names == listed == sorted(S.RGB_DELTA_SYMBOLS) and len(names) == 5
    assert set(S.RGB_DELTA_SYMBOLS) <= set(S.C_ABI_SYMBOLS)
    header = open(os.path.join(ROOT, "include", HEADER)).read()
    assert "#define SRCNN_AMD_RGB_DELTA_VERSION 1" in header
    assert '#include "srcnn_amd_delta.h"' in header and '#include "srcnn_amd_rgb_rect_list.h"' in header
    exported = _exported(S.LIB_PATH)
    assert set(names) <= set(exported)
    assert exported == sorted(S.C_ABI_SYMBOLS + S.CXX_SYMBOLS + HANDLE_ONLY_HOOKS)
    assert S.lib().srcnn_rgb_delta_abi_version() == 1
    assert C.sizeof(S.DeltaStats) == 32 and C.sizeof(S.RgbRectItem) == 96          # the structs of the binding are the headers'
    emap = open(os.path.join(ROOT, "libsrcnn_amd", "csrc", "exports.map")).read()
    assert "srcnn_*;" in emap and all(name in emap for name in names)              # exported by the pattern, and named in its comment
    for lst in ("build.py", os.path.join("..", "Makefile")):                       # both source lists carry the new files
        text = open(os.path.join(ROOT, "libsrcnn_amd", lst)).read()
        assert "srcnn_rgb_delta_call.cpp" in text and "srcnn_rgb_delta.hpp" in text and "srcnn_amd_rgb_delta.h" in text, lst


def test_no_older_header_or_list_mentions_the_new_names():
    names = _declared(HEADER)
    assert len(names) == 5
    for other in OLDER:
        text = open(os.path.join(ROOT, "include", other)).read()
        assert not set(names) & set(_declared(other)), other
        assert not any(n in text for n in names) and "srcnn_amd_rgb_delta" not in text.lower(), other
    for lst in os.listdir(os.path.join(ROOT, "include")):
        if lst.endswith(".abi") and lst != "srcnn_amd_rgb_delta.abi":
            assert not set(names) & set(open(os.path.join(ROOT, "include", lst)).read().split()), lst


def test_strict_only_build_exports_the_same_set(S):
    from libsrcnn_amd import build
    strict, _ = build.build_strict_only(verbose=False)
    assert _exported(strict) == _exported(S.LIB_PATH)
    assert set(S.RGB_DELTA_SYMBOLS) <= set(_exported(strict))


def test_header_compiles_as_c99_and_struct_sizes_match(S, tmp_path):
    src = tmp_path / "use.c"
    src.write_text('#include "srcnn_amd_rgb_delta.h"\n'
                   "int f(const void* const a[4], const void* const b[4], void* const out[4], unsigned char* fl) {\n"
                   "  srcnn_delta_stats st; srcnn_rgb_rect_item it[2]; srcnn_rgb_format fmt; unsigned dw, dh, c, r, n;\n"
                   "  fmt.struct_size = (unsigned)sizeof fmt; fmt.layout = SRCNN_RGB_INTERLEAVED; fmt.order = SRCNN_RGB_ORDER_RGB; fmt.alpha = 0; fmt.depth = 8;\n"
                   "  st.struct_size = (unsigned)sizeof st;\n"
                   "  return srcnn_rgb_delta_abi_version() + srcnn_rgb_delta_grid(8, 8, 2.0f, SRCNN_FILTER_BICUBIC, 0, 0, &dw, &dh, &c, &r)\n"
                   "  + srcnn_rgb_delta_flags_dev(&fmt, 8, 8, 2.0f, SRCNN_FILTER_BICUBIC, a, 0, b, 0, 0, 0, fl, 0)\n"
                   "  + srcnn_rgb_delta_rects(fl, c, r, 64, 64, &fmt, dw, dh, out, 0, 0, 0, it, 2, (unsigned)sizeof it[0], &n)\n"
                   "  + srcnn_rgb_upscale_delta_dev(&fmt, 8, 8, 2.0f, SRCNN_FILTER_BICUBIC, a, 0, b, 0, 0, 0, out, 0, 0, 0, 0, &st)\n"
                   "  + (int)st.cell_samples + SRCNN_AMD_RGB_DELTA_VERSION; }\n")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-c", str(src), "-I" + os.path.join(ROOT, "include"), "-o", str(tmp_path / "use.o")])
    main = tmp_path / "sizes.c"
    main.write_text('#include <stdio.h>\n#include "srcnn_amd_rgb_delta.h"\n'
                    'int main(void) { printf("%u %u %u\\n", (unsigned)sizeof(srcnn_delta_stats), (unsigned)sizeof(srcnn_rgb_rect_item), (unsigned)sizeof(srcnn_rgb_format)); return 0; }\n')
    exe = str(tmp_path / "sizes")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", str(main), "-I" + os.path.join(ROOT, "include"), "-o", exe])
    sizes = subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split()
    assert [int(v) for v in sizes] == [C.sizeof(S.DeltaStats), C.sizeof(S.RgbRectItem), C.sizeof(S.RgbFormat)]


# ---- the grid ----
def test_grid_against_its_arithmetic(S):
    for (w, h, mul, tile) in ((96, 56, 2.0, (32, 16)), (96, 56, 2.0, (40, 24)), (37, 23, 2.0, (16, 16)), (96, 56, 2.5, (64, 64)), (96, 56, 2.5, (0, 0)),
                              (96, 56, 2.5, (0, 8)), (40, 31, 1.5, (8, 9)), (50, 30, 0.75, (8, 8)), (24, 24, 1.0, (65535, 8)), (3840, 2160, 2.0, (0, 0))):
        dw, dh = S.output_size(w, h, mul)
        tw, th = tile[0] or 64, tile[1] or 64
        assert S.rgb_delta_grid(w, h, mul, 2, tile) == (dw, dh, -(-dw // tw), -(-dh // th)), (w, h, mul, tile)
    assert S.rgb_delta_grid(96, 56, 2.0, 2, (32, 16)) == (192, 112, 6, 7)
    assert S.rgb_delta_grid(3840, 2160, 2.0, 2) == (7680, 4320, 120, 68)


def test_grid_limits_and_argument_rules(S):
    g = lambda *a, **kw: _code(S, lambda: S.rgb_delta_grid(*a, **kw))   # noqa: E731
    assert g(0, 56, 2.0, 2) == E_ARG and g(96, 0, 2.0, 2) == E_ARG
    assert g(96, 56, 0.0, 2) == E_SCALE and g(96, 56, -1.0, 2) == E_SCALE and g(1, 1, 0.25, 2) == E_SCALE
    assert g(96, 56, 2.0, -1) == E_ARG and g(96, 56, 2.0, 5) == E_ARG
    # the tile: 0 = 64, else 8 ... 65535
    for t in (1, 7, 65536, 1 << 20):
        assert g(96, 56, 2.0, 2, (t, 16)) == E_ARG and g(96, 56, 2.0, 2, (16, t)) == E_ARG, t
    for t in (8, 65535):
        assert g(96, 56, 2.0, 2, (t, 16)) == 0 and g(96, 56, 2.0, 2, (16, t)) == 0, t
    assert S.rgb_delta_grid(96, 56, 2.0, 2, (65535, 8)) == (192, 112, 1, 14)
    # the stated limit: 2048 tile columns or rows
    assert S.rgb_delta_grid(8192, 4, 2.0, 2, (8, 8))[2:] == (2048, 1) and g(8193, 4, 2.0, 2, (8, 8)) == E_UNSUPPORTED
    assert "2048" in _why(S)
    assert S.rgb_delta_grid(4, 8192, 2.0, 2, (8, 8))[2:] == (1, 2048) and g(4, 8193, 2.0, 2, (8, 8)) == E_UNSUPPORTED
    assert g(96, (1 << 20) + 1, 1.0, 2) == E_UNSUPPORTED and g(1 << 22, 4, 2.0, 2) == E_UNSUPPORTED          # the Y path's limits, from check_scale
    # the order: geometry and scale before the tile
    assert g(96, 56, 0.0, 2, (7, 7)) == E_SCALE and g(96, 56, 2.0, 9, (7, 7)) == E_ARG and "filter" in _why(S)
    # any result may be NULL
    c = C.c_uint(0)
    assert S.lib().srcnn_rgb_delta_grid(96, 56, 2.0, 2, 32, 16, None, None, C.byref(c), None) == 0 and c.value == 6
    assert S.lib().srcnn_rgb_delta_grid(96, 56, 2.0, 2, 32, 16, None, None, None, None) == 0


# ---- argument rules of the device calls: host buffers stand in for device planes, which is safe because every call below is
# refused before the device is looked up ----
class Image:
    """Two w x h sources, a dw x dh destination with its conv plane and a flag array in one host array, for one format."""

    def __init__(self, S, layout="interleaved", alpha=0, depth=8, w=9, h=7, mul=2.0, pitch=0, out_pitch=0):
        self.S, self.w, self.h, self.mul = S, w, h, mul
        self.fmt = S.rgb_format(layout, "rgb", alpha, depth)
        self.np = (3 + alpha) if layout == "planar" else 1
        self.bps = 1 if depth == 8 else 2
        self.bpp = self.bps * (1 if layout == "planar" else 3 + alpha)
        self.dw, self.dh = S.output_size(w, h, mul)
        self.row, self.orow = self.bpp * w, self.bpp * self.dw
        self.pitch, self.out_pitch = pitch, out_pitch
        in_plane = -(-max(pitch, self.row) * h // 64) * 64
        out_plane = -(-max(out_pitch, self.orow) * self.dh // 64) * 64
        self.in_plane, self.out_plane = in_plane, out_plane
        self.buf = np.zeros(2 * self.np * in_plane + (self.np + 1) * out_plane + 4096, np.uint8)
        base = -(-self.buf.ctypes.data // 64) * 64
        self.prev = [base + k * in_plane for k in range(self.np)]
        self.cur = [base + (self.np + k) * in_plane for k in range(self.np)]
        self.dst = [base + 2 * self.np * in_plane + k * out_plane for k in range(self.np)]
        self.conv = self.dst[-1] + out_plane
        self.flags = self.conv + out_plane

    def args(self, kw):
        a = dict(fmt=self.fmt, w=self.w, h=self.h, mul=self.mul, filt=2, prev=self.prev, prev_pitch=[self.pitch] * self.np, cur=self.cur,
                 cur_pitch=[self.pitch] * self.np, tile=(0, 0), dst=self.dst, dst_pitch=[self.out_pitch] * self.np, conv=self.conv, conv_pitch=0,
                 flags=self.flags, struct_size=None, stats=True)
        a.update(kw)
        return a

    def delta(self, **kw):
        a, S = self.args(kw), self.S
        return _code(S, lambda: S.rgb_upscale_delta_dev(a["fmt"], a["w"], a["h"], a["mul"], a["filt"], a["prev"], a["prev_pitch"], a["cur"], a["cur_pitch"],
                                                        a["tile"], a["dst"], a["dst_pitch"], a["conv"], a["conv_pitch"], None, a["stats"], a["struct_size"]))

    def flag(self, **kw):
        a, S = self.args(kw), self.S
        return _code(S, lambda: S.rgb_delta_flags_dev(a["fmt"], a["w"], a["h"], a["mul"], a["filt"], a["prev"], a["prev_pitch"], a["cur"], a["cur_pitch"],
                                                      a["tile"], a["flags"]))


def with_one(xs, k, v):
    xs = list(xs)
    xs[k] = v
    return xs


@pytest.mark.parametrize("layout,alpha,depth", [("interleaved", 0, 8), ("planar", 1, 12)], ids=["rgb8", "planar-rgba12"])
def test_argument_rules_of_both_device_calls(S, layout, alpha, depth):
    p = Image(S, layout, alpha, depth)
    last = p.np - 1
    for call in (p.delta, p.flag):
        # format
        assert call(fmt=None) == E_ARG
        for bad in (dict(layout=2), dict(order=2), dict(alpha=2), dict(depth=9), dict(struct_size=4)):
            f = S.rgb_format(layout, "rgb", alpha, depth)
            for k, v in bad.items():
                setattr(f, k, v)
            assert call(fmt=f) == E_ARG, bad
        # geometry and scale
        assert call(w=0) == E_ARG and call(h=0) == E_ARG
        for filt in (-1, 5, 100):
            assert call(filt=filt) == E_ARG
        assert call(mul=0.0) == E_SCALE and call(mul=-2.0) == E_SCALE and call(mul=0.01) == E_SCALE
        assert call(h=(1 << 20) + 1, mul=1.0) == E_UNSUPPORTED and call(w=1 << 22) == E_UNSUPPORTED
        # tile and grid
        assert call(tile=(7, 0)) == E_ARG and call(tile=(0, 65536)) == E_ARG
        assert call(w=8193, tile=(8, 8)) == E_UNSUPPORTED and "2048" in _why(S)
        # the source planes of both images
        assert call(cur=None) == E_ARG
        for which in ("prev", "cur"):
            planes = getattr(p, which)
            assert call(**{which: with_one(planes, last, None)}) == E_ARG, which
            assert call(**{which + "_pitch": with_one([0] * p.np, last, p.row - 1)}) == E_ARG and "pitch" in _why(S), which
            if depth > 8:                    # (depth 8 takes any base and any pitch: test_valid_calls_without_a_device)
                assert call(**{which: with_one(planes, last, planes[last] + 1)}) == E_ARG and "multiples of 2" in _why(S), which
                assert call(**{which + "_pitch": with_one([0] * p.np, last, p.row + 1)}) == E_ARG and "multiples of 2" in _why(S), which
    assert p.flag(flags=None) == E_ARG
    # the destination of the whole operation: a dw x dh image under the rules of the RGB(A) calls
    assert p.delta(dst=None) == E_ARG and p.delta(dst=with_one(p.dst, last, None)) == E_ARG
    assert p.delta(dst_pitch=with_one([0] * p.np, last, p.orow - 1)) == E_ARG and "output pitch" in _why(S)
    assert p.delta(conv_pitch=p.bps * p.dw - 1) == E_ARG and "dst_conv" in _why(S)
    if depth > 8:
        assert p.delta(dst=with_one(p.dst, last, p.dst[last] + 1)) == E_ARG and p.delta(dst_pitch=with_one([0] * p.np, last, p.orow + 1)) == E_ARG
        assert p.delta(conv=p.conv + 1) == E_ARG and p.delta(conv_pitch=p.bps * p.dw + 1) == E_ARG
    # a source plane of either image against a destination plane or dst_conv
    for which in ("prev", "cur"):
        planes = getattr(p, which)
        assert p.delta(dst=with_one(p.dst, last, planes[0])) == E_ARG and "input plane 0 overlaps output plane %d" % last in _why(S), which
        assert p.delta(dst=with_one(p.dst, 0, planes[last] + p.row * p.h - 2)) == E_ARG and "overlaps" in _why(S), which          # the last bytes only
        assert p.delta(conv=planes[last]) == E_ARG and "input plane %d overlaps output plane %d" % (last, p.np) in _why(S), which
    # two destination planes
    assert p.delta(conv=p.dst[0]) == E_ARG and "output planes 0 and %d overlap" % p.np in _why(S)
    if p.np > 1:
        assert p.delta(dst=with_one(p.dst, 1, p.dst[0] + 2)) == E_ARG and "output planes 0 and 1 overlap" in _why(S)
    # stats
    assert p.delta(struct_size=0) == E_ARG and p.delta(struct_size=C.sizeof(S.DeltaStats) + 8) == E_ARG and "struct_size" in _why(S)


def test_the_order_of_the_errors(S):
    p = Image(S)
    bad_fmt = S.rgb_format("interleaved", "rgb", 0, 9)
    for call in (p.delta, p.flag):
        assert call(fmt=bad_fmt, mul=0.0) == E_ARG                                              # format before scale
        assert call(mul=0.0, tile=(7, 7)) == E_SCALE                                             # scale before the tile
        assert call(w=8193, tile=(8, 8), cur=None) == E_UNSUPPORTED                              # the grid before the sources
        assert call(prev_pitch=[1], cur_pitch=[2]) == E_ARG and "previous" in _why(S)            # prev before cur
    assert p.delta(w=8193, tile=(8, 8), struct_size=0) == E_UNSUPPORTED                          # the grid before stats
    assert p.delta(struct_size=0, cur_pitch=[1]) == E_ARG and "struct_size" in _why(S)           # stats before the sources
    assert p.delta(cur_pitch=[1], dst_pitch=[1]) == E_ARG and "current" in _why(S)               # sources before the destination
    assert p.delta(dst_pitch=[1], conv=p.cur[0]) == E_ARG and "output pitch" in _why(S)          # the destination's planes before the overlaps
    assert p.delta(dst=[p.cur[0]], conv=p.cur[0]) == E_ARG and "input plane" in _why(S)          # source / destination before destination / destination


def test_valid_calls_without_a_device(S):
    if S.device_count() > 0:
        pytest.skip("a device is present: a valid call would run on host memory")
    for p in (Image(S), Image(S, pitch=64, out_pitch=128), Image(S, "planar", 1, 12, pitch=40, out_pitch=64), Image(S, "interleaved", 1, 16, 50, 30, 0.75),
              Image(S, "interleaved", 0, 8, pitch=29, out_pitch=55)):
        assert p.delta() == E_NODEVICE and p.flag() == E_NODEVICE, _why(S)
        assert p.delta(stats=False) == E_NODEVICE and p.delta(prev=None) == E_NODEVICE and p.flag(prev=None) == E_NODEVICE
        assert p.delta(conv=None) == E_NODEVICE and p.delta(prev_pitch=None, cur_pitch=None, dst_pitch=None) == E_NODEVICE
    q = Image(S)
    assert q.delta(prev=q.cur) == E_NODEVICE          # the two sources may be one image
    # depth 8: no base and no pitch needs an alignment
    assert q.delta(prev=[q.prev[0] + 1], cur=[q.cur[0] + 3], dst=[q.dst[0] + 1], conv=q.conv + 1, conv_pitch=q.dw + 3) == E_NODEVICE
    assert q.flag(cur=[q.cur[0] + 1], prev_pitch=[q.row + 3]) == E_NODEVICE


# ---- the coalescer and its items ----
def coalesce(flags, tile, dw, dh):
    """The rule, restated: tile rows top to bottom, the maximal runs of each; a run continues the open rect of the previous row
    when its [c0, c1) is identical, otherwise it opens a new rect.  Rects in the order they were opened."""
    tw, th = tile
    rows, cols = flags.shape
    rects, open_ = [], {}
    for r in range(rows):
        runs, c = [], 0
        while c < cols:
            if flags[r, c]:
                c0 = c
                while c < cols and flags[r, c]:
                    c += 1
                runs.append((c0, c))
            else:
                c += 1
        now = {}
        for run in runs:
            if run in open_:
                k = open_[run]
                rects[k][3] = min(dh, (r + 1) * th) - rects[k][1]
            else:
                k = len(rects)
                rects.append([run[0] * tw, r * th, min(dw, run[1] * tw) - run[0] * tw, min(dh, (r + 1) * th) - r * th])
            now[run] = k
        open_ = now
    return [tuple(r) for r in rects]


@pytest.mark.parametrize("layout,alpha,depth,bpp", CLASSES, ids=["%s-a%d-%d" % c[:3] for c in CLASSES])
def test_rects_and_items_for_every_layout_and_depth(S, layout, alpha, depth, bpp):
    fmt = S.rgb_format(layout, "bgr", alpha, depth)
    nplanes = (3 + alpha) if layout == "planar" else 1
    bps = 1 if depth == 8 else 2
    assert S.rgb_plane_size(fmt, 1, 1, 0)[2] == bpp                      # the class is the format's, not this test's
    rng = np.random.default_rng(8100 + bpp + 10 * nplanes)
    for tile, dw, dh in (((32, 16), 192, 112), ((40, 24), 192, 112), ((8, 8), 333, 95), ((64, 64), 20, 9)):
        cols, rows = -(-dw // tile[0]), -(-dh // tile[1])
        tight = S.rgb_plane_size(fmt, dw, dh, 0)[2]
        assert tight == bpp * dw
        for density in (0.0, 0.15, 0.6, 1.0):
            flags = ((rng.random((rows, cols)) < density) * int(rng.integers(1, 256))).astype(np.uint8)
            want = coalesce(flags, tile, dw, dh)
            bases = [0x100000 * (k + 1) + 2 * k for k in range(nplanes)]
            pitches = [tight + 2 * (k + 1) for k in range(nplanes)]
            conv, conv_pitch = 0x900000, bps * dw + 4
            got = S.rgb_delta_rects(flags, tile, fmt, dw, dh, bases, pitches, conv, conv_pitch)
            assert [g[:4] for g in got] == want
            for (x0, y0, _, _, dst, dpitch, dconv, dconv_pitch) in got:
                assert dst[:nplanes] == [bases[k] + y0 * pitches[k] + x0 * bpp for k in range(nplanes)]
                assert dst[nplanes:] == [None] * (4 - nplanes) and dpitch == pitches + [0] * (4 - nplanes)
                assert (dconv, dconv_pitch) == (conv + y0 * conv_pitch + x0 * bps, conv_pitch)
            # tight rows (pitch 0 and a NULL pitch array), no conv plane
            for arg in ([0] * nplanes, None):
                for (x0, y0, _, _, dst, dpitch, dconv, dconv_pitch) in S.rgb_delta_rects(flags, tile, fmt, dw, dh, bases, arg):
                    assert dst[:nplanes] == [bases[k] + y0 * tight + x0 * bpp for k in range(nplanes)] and dpitch[:nplanes] == [tight] * nplanes
                    assert dconv is None and dconv_pitch == 0
            # no image at all: NULL destinations; and the count-only form
            assert all(g[4] == [None] * 4 and g[6] is None for g in S.rgb_delta_rects(flags, tile, fmt, dw, dh))
            assert S.rgb_delta_rects(flags, tile, fmt, dw, dh, cap=0) == len(want)
            # a capacity that is one short: the code, the count, and not one item written
            if want:
                n = C.c_uint(0)
                items = (S.RgbRectItem * len(want))()
                C.memset(items, 0xEE, C.sizeof(items))
                f = np.ascontiguousarray(flags)
                rc = S.lib().srcnn_rgb_delta_rects(f.ctypes.data, cols, rows, tile[0], tile[1], C.byref(fmt), dw, dh, None, None, None, 0,
                                                   C.cast(items, C.c_void_p), len(want) - 1, C.sizeof(S.RgbRectItem), C.byref(n))
                assert rc == E_ARG and n.value == len(want) and bytes(items) == b"\xee" * C.sizeof(items)


def test_rects_argument_rules(S):
    flags = np.zeros((7, 6), np.uint8); flags[2:5, 2:4] = 1; flags[6, 5] = 1
    fmt = S.rgb_format("interleaved", "rgb", 0, 12)
    L, n, f, size = S.lib(), C.c_uint(99), flags.ctypes.data, C.sizeof(S.RgbRectItem)
    items = (S.RgbRectItem * 2)()
    it = C.cast(items, C.c_void_p)
    base = (C.c_void_p * 4)(0x10000, None, None, None)
    pitch = lambda v: (C.c_size_t * 4)(v, 0, 0, 0)   # noqa: E731
    ok = lambda *a: L.srcnn_rgb_delta_rects(*a)   # noqa: E731
    assert ok(f, 6, 7, 32, 16, C.byref(fmt), 192, 112, None, None, None, 0, it, 2, size, C.byref(n)) == 0 and n.value == 2
    assert ok(f, 6, 7, 32, 16, C.byref(fmt), 192, 112, None, None, None, 0, it, 1, size, C.byref(n)) == E_ARG and n.value == 2       # cap one short
    assert ok(f, 6, 7, 32, 16, C.byref(fmt), 192, 112, None, None, None, 0, None, 2, size, C.byref(n)) == E_ARG
    assert ok(f, 6, 7, 32, 16, C.byref(fmt), 192, 112, None, None, None, 0, None, 0, size, None) == E_ARG
    assert ok(None, 6, 7, 32, 16, C.byref(fmt), 192, 112, None, None, None, 0, None, 0, size, C.byref(n)) == E_ARG
    assert ok(f, 6, 7, 32, 16, None, 192, 112, None, None, None, 0, None, 0, size, C.byref(n)) == E_ARG
    assert ok(f, 5, 7, 32, 16, C.byref(fmt), 192, 112, None, None, None, 0, None, 0, size, C.byref(n)) == E_ARG          # not the grid of 192 x 112
    assert ok(f, 6, 7, 0, 16, C.byref(fmt), 192, 112, None, None, None, 0, None, 0, size, C.byref(n)) == E_ARG           # the tile is given here
    assert ok(f, 6, 7, 32, 16, C.byref(fmt), 0, 112, None, None, None, 0, None, 0, size, C.byref(n)) == E_SCALE
    assert ok(f, 6, 7, 32, 16, C.byref(fmt), 192, 112, None, None, None, 0, it, 2, size - 8, C.byref(n)) == E_ARG and "item_size" in _why(S)
    assert ok(f, 6, 7, 32, 16, C.byref(fmt), 192, 112, base, pitch(6 * 192 - 2), None, 0, None, 0, size, C.byref(n)) == E_ARG       # pitch below the row
    assert ok(f, 6, 7, 32, 16, C.byref(fmt), 192, 112, base, pitch(6 * 192 + 1), None, 0, None, 0, size, C.byref(n)) == E_ARG       # odd pitch at depth 12
    assert ok(f, 6, 7, 32, 16, C.byref(fmt), 192, 112, (C.c_void_p * 4)(0x10001, None, None, None), None, None, 0, None, 0, size, C.byref(n)) == E_ARG
    assert ok(f, 6, 7, 32, 16, C.byref(fmt), 192, 112, base, None, 0x90001, 0, None, 0, size, C.byref(n)) == E_ARG and "dst_conv" in _why(S)
    assert ok(f, 6, 7, 32, 16, C.byref(fmt), 192, 112, (C.c_void_p * 4)(), None, None, 0, None, 0, size, C.byref(n)) == E_ARG       # an image without its plane
    assert ok(f, 6, 7, 32, 16, C.byref(fmt), 192, 112, base, pitch(6 * 192 + 2), 0x90000, 2 * 192, it, 2, size, C.byref(n)) == 0 and n.value == 2
    assert (items[0].x0, items[0].y0, items[0].rw, items[0].rh) == (64, 32, 64, 48) and items[0].dst[0] == 0x10000 + 32 * (6 * 192 + 2) + 6 * 64


def test_the_whole_frame_setting_is_the_y_calls(S):
    """No RGB-specific setting unless the probe measures a crossover more than 50 permille away (DESIGN 4.16 says what it measured)."""
    rows = [ln for ln in S.debug_settings(markdown=True).splitlines() if "WHOLE_PERMILLE" in ln]
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert rows and all(r in design for r in rows)
    # no row is cut: the library formats every switch into a line of fixed size
    table = S.debug_settings(markdown=True)
    assert table.endswith(" |\n") and all(ln.startswith("| `SRCNN_") and ln.endswith(" |") for ln in table.splitlines())
    text = S.debug_settings()
    assert text.endswith("\n") and len(text.splitlines()) == len(table.splitlines()) and all(re.match(r"SRCNN_\w+=", ln) for ln in text.splitlines())
    assert rows[0].rstrip().endswith("Either route gives the same bits |")
    assert any("SRCNN_DELTA_WHOLE_PERMILLE" in r and "srcnn_rgb_upscale_delta_dev" in r for r in rows) or any("SRCNN_RGB_DELTA_WHOLE_PERMILLE" in r for r in rows)
