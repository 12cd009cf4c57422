"""CPU: the planar / semi-planar YUV rect list extension (include/srcnn_amd_yuv_rect_list.h) -- its declared functions, committed
list, binding and export table agree (full and strict-only builds), the header is C99, no older header mentions the new names,
every list rule, frame rule and item rule of srcnn_yuv_upscale_rect_list_dev returns its code before any device lookup, in the
order the header states (host buffers stand in for device planes), and srcnn_yuv_upscale_rect_list_plan, which runs the call's
own routing and packing without a device, reports what the header states."""
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
         "srcnn_amd_rgb_rect_list.h", "libsrcnn_dropin.h")
HEADER = "srcnn_amd_yuv_rect_list.h"
PLANAR, SEMI = 0, 1


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
    names = _declared(HEADER)
    listed = [ln.strip() for ln in open(os.path.join(ROOT, "include", "srcnn_amd_yuv_rect_list.abi")) if ln.strip() and not ln.startswith("#")]
    assert listed == sorted(listed) and len(set(listed)) == len(listed)
    assert names == listed == sorted(S.YUV_RECT_LIST_SYMBOLS) and len(names) == 3
    assert set(S.YUV_RECT_LIST_SYMBOLS) <= set(S.C_ABI_SYMBOLS)
    header = open(os.path.join(ROOT, "include", HEADER)).read()
    assert "#define SRCNN_AMD_YUV_RECT_LIST_VERSION 1" in header
    assert '#include "srcnn_amd_yuv_rect.h"' in header and '#include "srcnn_amd_rect_list.h"' in header
    exported = _exported(S.LIB_PATH)
    assert set(names) <= set(exported)
    assert exported == sorted(S.C_ABI_SYMBOLS + S.CXX_SYMBOLS + HANDLE_ONLY_HOOKS)
    version = int(re.search(r"#define SRCNN_AMD_YUV_RECT_LIST_VERSION (\d+)", header).group(1))
    assert S.lib().srcnn_yuv_rect_list_abi_version() == version == 1
    # the structs of the binding are the header's
    assert C.sizeof(S.YuvRectItem) == 64 and C.sizeof(S.RectListPlan) == 40
    emap = open(os.path.join(ROOT, "libsrcnn_amd", "csrc", "exports.map")).read()
    assert "srcnn_*;" in emap and all(name in emap for name in names)          # exported by the pattern, and named in its comment
    assert "SRCNN_YUV_RECT_LIST_UNFUSED=0" in S.debug_settings()


def test_no_older_header_mentions_the_new_names():
    names = _declared(HEADER)
    assert len(names) == 3
    for other in OLDER:
        text = open(os.path.join(ROOT, "include", other)).read()
        assert not set(names) & set(_declared(other)), other
        assert not any(n in text for n in names) and "srcnn_amd_yuv_rect_list" not in text.lower() and "srcnn_yuv_rect_item" not in text, other


def test_strict_only_build_exports_the_same_set(S):
    from libsrcnn_amd import build
    strict, _ = build.build_strict_only(verbose=False)
    assert _exported(strict) == _exported(S.LIB_PATH)
    assert set(S.YUV_RECT_LIST_SYMBOLS) <= set(_exported(strict))


def test_header_compiles_as_c99_and_the_item_is_64_bytes(tmp_path):
    src = tmp_path / "use.c"
    src.write_text('#include "srcnn_amd_yuv_rect_list.h"\n'
                   "typedef char item_is_64_bytes[sizeof(srcnn_yuv_rect_item) == 64 ? 1 : -1];\n"
                   "int f(const void* const src[3], void* out) { srcnn_yuv_rect_item it[2]; srcnn_rect_list_plan p; srcnn_yuv_format fmt;\n"
                   "  int k; fmt.struct_size = (unsigned)sizeof fmt; fmt.layout = SRCNN_YUV_SEMIPLANAR; fmt.chroma = SRCNN_YUV_420; fmt.depth = 10; fmt.msb_aligned = 1;\n"
                   "  it[0].x0 = 2; it[0].y0 = 2; it[0].rw = 3; it[0].rh = 4;\n"
                   "  for (k = 0; k < 3; ++k) { it[0].dst[k] = k == 2 ? 0 : out; it[0].dst_pitch[k] = 0; }\n"
                   "  it[1] = it[0]; p.struct_size = (unsigned)sizeof p;\n"
                   "  return srcnn_yuv_rect_list_abi_version()\n"
                   "  + srcnn_yuv_upscale_rect_list_plan(&fmt, 8, 8, 2.0f, SRCNN_FILTER_BICUBIC, it, 2, (unsigned)sizeof it[0], &p)\n"
                   "  + srcnn_yuv_upscale_rect_list_dev(&fmt, 8, 8, 2.0f, SRCNN_FILTER_BICUBIC, src, 0, it, 2, (unsigned)sizeof it[0], 0)\n"
                   "  + (int)p.atlases + SRCNN_AMD_YUV_RECT_LIST_VERSION; }\n")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-c", str(src), "-I" + os.path.join(ROOT, "include"),
                           "-o", str(tmp_path / "use.o")])


# ---- argument rules: host buffers stand in for device planes, which is safe because every call below is refused before the
# device is looked up ----
def chroma_cols_rows(w, h, chroma):
    return (w if chroma == "444" else (w + 1) // 2), ((h + 1) // 2 if chroma == "420" else h)


class Planes:
    """A 9 x 7 source frame and room for three rects of the 18 x 14 output, in one host array; every plane starts on an even
    address."""

    def __init__(self, S, layout=PLANAR, chroma="420", depth=10, w=9, h=7, mul=2.0, src_pitch=None,
                 rects=((2, 2, 9, 6), (0, 0, 18, 14), (14, 10, 4, 4)), dst_pitch=0):
        self.S, self.fmt = S, S.yuv_format(layout, chroma, depth, 0)
        self.w, self.h, self.mul, self.src_pitch = w, h, mul, src_pitch
        self.np = 2 if layout == SEMI else 3
        self.bps = 1 if depth == 8 else 2
        spp = 2 if layout == SEMI else 1
        even = lambda n: (n + 1) & ~1   # noqa: E731

        def shapes(pw, ph):              # per plane: (row bytes, rows)
            cw, ch = chroma_cols_rows(pw, ph, chroma)
            return [(pw * self.bps, ph)] + [(cw * spp * self.bps, ch)] * (self.np - 1)
        self.src_rows = [rb for rb, _ in shapes(w, h)]
        sizes = [even(max((src_pitch or [0] * 3)[k], rb) * r) for k, (rb, r) in enumerate(shapes(w, h))]
        total = sum(sizes)
        per_item = []
        for (_, _, rw, rh) in rects:
            sh = shapes(rw, rh)
            per_item.append((sh, [even(max(dst_pitch, rb) * r) for rb, r in sh]))
            total += sum(per_item[-1][1])
        self.buf = np.zeros(total // 2 + 64, np.uint16)
        base = self.buf.ctypes.data
        self.src, pos = [], base
        for sz in sizes:
            self.src.append(pos)
            pos += sz
        self.src += [None] * (3 - self.np)
        self.src_end = pos
        self.items, self.dst_rows = [], []
        for r, (sh, psizes) in zip(rects, per_item):
            dst = []
            for sz in psizes:
                dst.append(pos)
                pos += sz
            self.dst_rows.append([rb for rb, _ in sh])
            self.items.append(dict(x0=r[0], y0=r[1], rw=r[2], rh=r[3], dst=dst, pitch=[dst_pitch] * self.np))

    def call(self, at=None, n=None, item_size=None, items="given", **kw):
        """The list call with frame arguments overridden by kw, or -- with at=k -- item k's fields."""
        S = self.S
        a = dict(fmt=self.fmt, w=self.w, h=self.h, multiply=self.mul, filt=2, src=self.src, src_pitch=self.src_pitch)
        its = [dict(i) for i in self.items]
        if at is None:
            a.update(kw)
        else:
            its[at].update(kw)
        arr = [(i["x0"], i["y0"], i["rw"], i["rh"], i["dst"], i["pitch"]) for i in its] if items == "given" else items
        try:
            S.yuv_upscale_rect_list_dev(a["fmt"], a["w"], a["h"], a["multiply"], a["filt"], a["src"], a["src_pitch"], arr, None, n=n, item_size=item_size)
        except S.SrcnnError as e:
            self.message = str(e)
            return e.code
        return 0


def test_list_rules_and_frame_rules(S):
    p = Planes(S)
    # 1. the list itself
    assert p.call(item_size=C.sizeof(S.YuvRectItem) - 8) == E_ARG and p.call(item_size=0) == E_ARG and p.call(item_size=96) == E_ARG
    assert p.call(items=None, n=3) == E_ARG                     # NULL items with n > 0
    assert p.call(n=0) == 0 and p.call(items=None, n=0) == 0           # nothing to do: SRCNN_OK, even without a device
    assert p.call(n=0, fmt=None, src=None, w=0) == 0                   # ... with nothing else looked at
    assert S.lib().srcnn_yuv_upscale_rect_list_dev(None, 0, 0, 0.0, 9, None, None, None, 0, C.sizeof(S.YuvRectItem), None) == 0
    assert p.call(n=0, item_size=8) == E_ARG                    # (the item size is checked first)
    big = (S.YuvRectItem * 65537)()
    assert p.call(items=big, n=65537) == E_UNSUPPORTED
    assert p.call(items=big, n=65536) == E_ARG and "item 0:" in p.message      # 65536 are allowed: its first (all-zero) item is refused
    # the list comes before the frame
    assert p.call(fmt=None, item_size=8) == E_ARG and "item_size" in p.message
    assert p.call(fmt=None, items=big, n=65537) == E_UNSUPPORTED
    # 2. the frame, with the codes and the order of srcnn_yuv_upscale_rect_dev; no item is named
    assert p.call(fmt=None) == E_ARG and "item" not in p.message
    for size in (0, 4, 19, 24):
        fmt = S.yuv_format(PLANAR, "420", 10, 0)
        fmt.struct_size = size
        assert p.call(fmt=fmt) == E_ARG, size
    assert p.call(fmt=S.yuv_format(2, "420", 10, 0)) == E_ARG and p.call(fmt=S.yuv_format(PLANAR, 3, 10, 0)) == E_ARG
    assert p.call(fmt=S.yuv_format(PLANAR, "420", 9, 0)) == E_ARG and p.call(fmt=S.yuv_format(PLANAR, "420", 8, 1)) == E_ARG
    assert p.call(src=None) == E_ARG and "item" not in p.message
    for k in range(3):
        src = list(p.src); src[k] = None
        assert p.call(src=src) == E_ARG and ("NULL plane %d" % k) in p.message and "item" not in p.message, k
    semi = Planes(S, layout=SEMI)
    assert semi.call(src=[semi.src[0], None, None]) == E_ARG
    if S.device_count() == 0:
        assert semi.call() == E_NODEVICE                         # plane 2 of a semi-planar frame is not looked at
    for filt in (-1, 5, 100):
        assert p.call(filt=filt) == E_ARG
    assert p.call(w=0) == E_ARG and p.call(h=0) == E_ARG
    assert p.call(multiply=0.0) == E_SCALE and p.call(multiply=0.05) == E_SCALE
    assert p.call(h=(1 << 20) + 1) == E_UNSUPPORTED
    for k in range(3):
        pitch = [0, 0, 0]; pitch[k] = p.src_rows[k] - 2
        assert p.call(src_pitch=pitch) == E_ARG and "input pitch" in p.message and "item" not in p.message      # a source pitch below its row
        pitch[k] = p.src_rows[k] + 1
        assert p.call(src_pitch=pitch) == E_ARG and "item" not in p.message                                      # odd above 8 bits
        src = list(p.src); src[k] += 1
        assert p.call(src=src) == E_ARG and "item" not in p.message
    # the order inside the frame: NULL source plane < filter < zero size < scale < limits < pitch
    assert p.call(src=[None] * 3, filt=9) == E_ARG and "NULL plane" in p.message
    assert p.call(filt=9, w=0) == E_ARG and "filter" in p.message
    assert p.call(w=0, multiply=0.0) == E_ARG
    assert p.call(multiply=0.0, src_pitch=[2, 0, 0]) == E_SCALE
    assert p.call(h=(1 << 20) + 1, src_pitch=[2, 0, 0]) == E_UNSUPPORTED
    # 3. the frame comes before the items
    assert p.call(at=0, rw=0) == E_ARG and "item 0:" in p.message
    q = Planes(S)
    q.items[0]["rw"] = 0
    assert q.call(filt=7) == E_ARG and "item" not in q.message
    assert q.call(src_pitch=[2, 0, 0]) == E_ARG and "item" not in q.message


@pytest.mark.parametrize("at", [0, 2])
@pytest.mark.parametrize("layout", [PLANAR, SEMI])
def test_item_rules_name_the_first_offender(S, at, layout):
    p = Planes(S, layout=layout, dst_pitch=256)
    it = p.items[at]
    rows = p.dst_rows[at]

    def planes(k, v):
        d = list(it["dst"]); d[k] = v
        return d

    def pitches(k, v):
        d = list(it["pitch"]); d[k] = v
        return d
    bad = [dict(rw=0), dict(rh=0), dict(x0=18, rw=1), dict(y0=14, rh=1), dict(x0=0xfffffffe, rw=4), dict(y0=0xfffffffc, rh=6), dict(rw=19, x0=0),
           dict(x0=it["x0"] + 1, rw=1), dict(y0=it["y0"] + 1, rh=1)]                              # ... an odd origin under 4:2:0
    for k in range(p.np):
        bad += [dict(dst=planes(k, None)), dict(pitch=pitches(k, rows[k] - 2)), dict(pitch=pitches(k, 257)), dict(dst=planes(k, it["dst"][k] + 1)),
                dict(dst=planes(k, p.src[0])), dict(dst=planes(k, p.src_end - 2))]
    bad += [dict(dst=planes(1, it["dst"][0]))]                                                    # two destination planes of the item overlap
    if p.np == 3:
        bad += [dict(dst=planes(2, it["dst"][1] + 2))]
    for kw in bad:
        assert p.call(at=at, **kw) == E_ARG, kw
        assert ("item %d:" % at) in p.message, (kw, p.message)
    # the order inside an item: NULL plane < empty < inside < odd origin < pitch < alignment < source overlap < destination overlap
    order = [(dict(dst=planes(0, None), rw=0), "NULL plane 0"), (dict(rw=0, x0=19), "empty rect"), (dict(x0=17, rw=2), "not inside"),
             (dict(x0=1, rw=2, pitch=pitches(0, 2)), "origin"), (dict(pitch=pitches(0, rows[0] - 2), dst=planes(0, it["dst"][0] + 1)), "pitch"),
             (dict(dst=planes(0, it["dst"][0] + 1), pitch=pitches(1, 257)), "output plane 0"),
             (dict(dst=[p.src[0]] + [it["dst"][0]] * (p.np - 1)), "input plane 0 overlaps"), (dict(dst=planes(1, it["dst"][0])), "output planes 0 and 1 overlap")]
    for kw, text in order:
        assert p.call(at=at, **kw) == E_ARG and text in p.message and ("item %d:" % at) in p.message, (kw, text, p.message)
    # the message after the prefix is the single call's
    try:
        S.yuv_upscale_rect_dev(p.fmt, p.w, p.h, p.mul, 2, p.src, None, 1, it["y0"], 2, it["rh"], it["dst"] + [None] * (3 - p.np), it["pitch"] + [0] * (3 - p.np))
        single = None
    except S.SrcnnError as e:
        single = str(e)
    assert p.call(at=at, x0=1, rw=2) == E_ARG
    assert single and p.message == single.replace(": ", ": item %d: " % at, 1), (single, p.message)
    # an earlier offender wins
    q = Planes(S, layout=layout)
    q.items[1]["rw"] = 0
    assert q.call(at=2, rh=0) == E_ARG and "item 1:" in q.message


def test_depth_8_needs_no_alignment_and_items_may_share_memory(S):
    if S.device_count() > 0:
        pytest.skip("a device is present: a valid call would run on host memory")
    p = Planes(S, depth=8, dst_pitch=64)
    assert p.call() == E_NODEVICE
    assert p.call(at=1, dst=[p.items[1]["dst"][0] + 1] + p.items[1]["dst"][1:], pitch=[63, 64, 64]) == E_NODEVICE      # odd base, odd pitch
    assert Planes(S, layout=SEMI, chroma="422", depth=12, src_pitch=[64] * 3, dst_pitch=128).call() == E_NODEVICE
    assert Planes(S, w=50, h=30, mul=0.75, rects=((0, 0, 37, 22), (36, 20, 1, 2))).call() == E_NODEVICE
    assert Planes(S, chroma="444", rects=((3, 3, 8, 6), (0, 0, 18, 14), (17, 13, 1, 1))).call() == E_NODEVICE          # odd origins are fine in 4:4:4
    q = Planes(S, rects=((2, 2, 9, 6), (4, 6, 9, 6), (14, 10, 4, 4)))
    q.items[1]["dst"] = q.items[0]["dst"]                          # destinations of DIFFERENT items that overlap are the caller's business
    assert q.call() == E_NODEVICE


# ---- the plan ----
def plan_tuple(p):
    return p.batched_items, p.single_items, p.atlases


def _code(S, fn):
    try:
        fn()
    except S.SrcnnError as e:
        return e.code
    return 0


def test_plan_struct_and_argument_rules(S):
    fmt = S.yuv_format()
    items = [(2, 2, 9, 6), (0, 0, 18, 14)]
    code = lambda **kw: _code(S, lambda: S.yuv_upscale_rect_list_plan(fmt, 9, 7, 2.0, 2, items, **kw))   # noqa: E731
    assert code() == 0
    assert code(struct_size=0) == E_ARG and code(struct_size=C.sizeof(S.RectListPlan) + 8) == E_ARG
    assert code(item_size=96) == E_ARG
    assert _code(S, lambda: S.yuv_upscale_rect_list_plan(fmt, 9, 7, 2.0, 2, None, n=2)) == E_ARG
    assert _code(S, lambda: S.yuv_upscale_rect_list_plan(fmt, 9, 7, 2.0, 2, (S.YuvRectItem * 65537)(), n=65537)) == E_UNSUPPORTED
    assert _code(S, lambda: S.yuv_upscale_rect_list_plan(None, 9, 7, 2.0, 2, items)) == E_ARG
    assert _code(S, lambda: S.yuv_upscale_rect_list_plan(fmt, 9, 7, 0.0, 2, items)) == E_SCALE
    assert _code(S, lambda: S.yuv_upscale_rect_list_plan(fmt, 9, 7, 2.0, 7, items)) == E_ARG
    assert _code(S, lambda: S.yuv_upscale_rect_list_plan(fmt, 9, 7, 2.0, 2, items + [(16, 0, 3, 1)])) == E_ARG
    assert "item 2:" in S.lib().srcnn_last_error().decode()
    assert _code(S, lambda: S.yuv_upscale_rect_list_plan(fmt, 9, 7, 2.0, 2, items + [(0, 0, 2, 2), (3, 0, 1, 1)])) == E_ARG       # an odd origin
    assert "item 3:" in S.lib().srcnn_last_error().decode() and "origin" in S.lib().srcnn_last_error().decode()
    assert _code(S, lambda: S.yuv_upscale_rect_list_plan(S.yuv_format("planar", "444"), 9, 7, 2.0, 2, [(3, 1, 1, 1)])) == 0
    # no plane address and no pitch is looked at: NULL planes and absurd pitches plan like any others
    assert plan_tuple(S.yuv_upscale_rect_list_plan(fmt, 9, 7, 2.0, 2, [(2, 2, 9, 6, [None, 1, 3], [1, 1, 1])])) == (1, 0, 1)
    assert S.lib().srcnn_yuv_upscale_rect_list_plan(C.byref(fmt), 9, 7, 2.0, 2, None, 0, C.sizeof(S.YuvRectItem), None) == E_ARG
    p = S.yuv_upscale_rect_list_plan(fmt, 9, 7, 2.0, 2, [])
    assert plan_tuple(p) == (0, 0, 0) and p.cell_samples == p.atlas_samples == p.scratch_bytes == 0
    p = S.yuv_upscale_rect_list_plan(None, 0, 0, 0.0, 9, [])                     # n == 0: nothing else is looked at
    assert plan_tuple(p) == (0, 0, 0)


def small_rects(seed=64001, n=64, chroma="420"):
    from rect_list_worker import seeded_rects
    from yuv_rect_worker import snap
    return [snap(r, chroma) for r in seeded_rects(seed, n)]           # 96 x 56 -> 192 x 112, 1 ... 41 samples a side


@pytest.mark.parametrize("cell", [(PLANAR, "420", 8), (SEMI, "420", 10), (SEMI, "422", 12), (PLANAR, "444", 16)])
def test_plan_packs_as_the_y_list_and_states_the_headers_scratch(S, cell):
    rects = small_rects(chroma=cell[1])
    fmt = S.yuv_format(cell[0], cell[1], cell[2], 0)
    p = S.yuv_upscale_rect_list_plan(fmt, 96, 56, 2.0, 2, rects)
    assert plan_tuple(p) == (64, 0, 1)
    y = S.y_path_rect_list_plan(96, 56, 192, 112, 2, rects)        # the packer is the same
    assert (p.cell_samples, p.atlas_samples) == (y.cell_samples, y.atlas_samples)
    assert p.cell_samples == sum((rw + 12) * (rh + 12) for (_, _, rw, rh) in rects)
    # the header: 136 B per sample of the largest atlas, 160 B per batched item, 160 B per atlas
    assert p.scratch_bytes == 136 * p.atlas_samples + 160 * 64 + 160 * 1
    header = open(os.path.join(ROOT, "include", HEADER)).read()
    assert "136 B per sample" in header and "160 B per batched item" in header and "160 B per atlas" in header


def test_plan_sends_everything_else_the_single_way(S):
    from rect_list_worker import seeded_rects
    from yuv_rect_worker import snap
    fmt = S.yuv_format()                     # planar 4:2:0, 8 bits
    snapped = lambda rects: [snap(r, "420") for r in rects]   # noqa: E731
    assert plan_tuple(S.yuv_upscale_rect_list_plan(fmt, 50, 30, 0.75, 2, snapped(seeded_rects(5, 20, 37, 22, hi=15)))) == (0, 20, 0)      # a down-scale
    assert S.output_size(50, 30, 0.75) == (37, 22)
    assert plan_tuple(S.yuv_upscale_rect_list_plan(fmt, 24, 24, 1.0, 2, snapped(seeded_rects(7, 20, 24, 24, hi=15)))) == (0, 20, 0)       # the identity size
    # a luma axis that keeps its size while the other grows: 30 x 1 at x1.5 is 45 x 1
    assert S.output_size(30, 1, 1.5) == (45, 1)
    assert plan_tuple(S.yuv_upscale_rect_list_plan(fmt, 30, 1, 1.5, 2, snapped(seeded_rects(6, 20, 45, 1, hi=15)))) == (0, 20, 0)
    # a CHROMA axis that keeps its size while luma grows in both: 1 x 9 at x2 is 2 x 18, one chroma column before and after
    assert S.output_size(1, 9, 2.0) == (2, 18)
    rects = snapped(seeded_rects(8, 20, 2, 18, hi=15))
    assert plan_tuple(S.yuv_upscale_rect_list_plan(fmt, 1, 9, 2.0, 2, rects)) == (0, 20, 0)
    assert plan_tuple(S.y_path_rect_list_plan(1, 9, 2, 18, 2, rects)) == (20, 0, 1)                     # (the Y list batches them)
    assert plan_tuple(S.yuv_upscale_rect_list_plan(S.yuv_format("planar", "444"), 1, 9, 2.0, 2, rects)) == (20, 0, 1)      # (and 4:4:4 has no such axis)
    # ... and 4:2:0 with w = 3 at 4/3: dw = 4, two chroma columns before and after
    mul = float(np.float32(4.0 / 3.0)) + 1e-6
    assert S.output_size(3, 30, mul) == (4, 40)
    rects = snapped(seeded_rects(9, 12, 4, 40, hi=15))
    assert plan_tuple(S.yuv_upscale_rect_list_plan(fmt, 3, 30, mul, 2, rects)) == (0, 12, 0)
    # the switches are read when the library loads: processes of their own
    code = ("import libsrcnn_amd as S, sys; sys.path.insert(0, %r); from rect_list_worker import seeded_rects; from yuv_rect_worker import snap;"
            "rects = [snap(r, '420') for r in seeded_rects(64001, 64)];"
            "p = S.yuv_upscale_rect_list_plan(S.yuv_format(), 96, 56, 2.0, 2, rects);"
            "y = S.y_path_rect_list_plan(96, 56, 192, 112, 2, rects);"
            "print('PLAN', p.batched_items, p.single_items, p.atlases, 'Y', y.batched_items)" % os.path.join(ROOT, "tests"))
    r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, SRCNN_YUV_RECT_LIST_UNFUSED="1"), cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "PLAN 0 64 0 Y 64" in r.stdout, r.stdout[-500:] + r.stderr[-1500:]      # (the Y list has a switch of its own)
    r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, SRCNN_RECT_LIST_SINGLE_SAMPLES="1000"), cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-1500:]
    nb = sum((rw + 12) * (rh + 12) < 1000 for (_, _, rw, rh) in small_rects())
    assert 0 < nb < 64 and ("PLAN %d %d 1 Y %d" % (nb, 64 - nb, nb)) in r.stdout, r.stdout          # the shared threshold, on the cell's samples


def test_plan_in_a_non_parity_mode_is_all_single(S):
    prev = S.set_mode(S.MODE_FAST)           # (a strict-only build refuses: conftest turns that into a skip)
    try:
        p = S.yuv_upscale_rect_list_plan(S.yuv_format(), 96, 56, 2.0, 2, small_rects())
    finally:
        S.set_mode(prev)
    assert plan_tuple(p) == (0, 64, 0) and p.scratch_bytes == 0
    assert plan_tuple(S.yuv_upscale_rect_list_plan(S.yuv_format(), 96, 56, 2.0, 2, small_rects())) == (64, 0, 1)


def test_plan_lower_workspace_limit_raises_atlases(S):
    rects = small_rects()
    fmt = S.yuv_format("semiplanar", "420", 10, 1)
    one = S.yuv_upscale_rect_list_plan(fmt, 96, 56, 2.0, 2, rects)
    prev = S.lib().srcnn_set_workspace_limit(1 << 20)
    try:
        p = S.yuv_upscale_rect_list_plan(fmt, 96, 56, 2.0, 2, rects)
    finally:
        S.lib().srcnn_set_workspace_limit(prev)
    assert one.atlases == 1 and p.atlases >= 3 and p.batched_items == 64
    assert 128 * p.atlas_samples <= p.atlases << 20               # every atlas obeys the cap
    assert p.scratch_bytes < one.scratch_bytes                    # scratch is the LARGEST atlas, not their sum
    assert S.yuv_upscale_rect_list_plan(fmt, 96, 56, 2.0, 2, rects).atlases == 1
