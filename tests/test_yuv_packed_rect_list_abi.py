"""CPU: the packed YUV rect list extension (include/srcnn_amd_yuv_packed_rect_list.h) -- its declared functions, committed list,
binding and export table agree (full and strict-only builds), the header is C99, no older header mentions the new names, every
list rule, frame rule and item rule of srcnn_yuv_packed_upscale_rect_list_dev returns its code before any device lookup, in the
order the header states (host buffers stand in for device memory), and srcnn_yuv_packed_upscale_rect_list_plan, which runs the
call's own routing and packing without a device, reports what the header states."""
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
         "srcnn_amd_rgb_rect_list.h", "srcnn_amd_yuv_rect_list.h", "libsrcnn_dropin.h")
HEADER = "srcnn_amd_yuv_packed_rect_list.h"
NAMES = ("yuy2", "uyvy", "yvyu", "y210", "y212", "y216", "vuya", "y410", "y416", "v210")
_422 = NAMES[:6]
UNIT = {n: (6 if n == "v210" else 2 if n in _422 else 1) for n in NAMES}
ALIGN = {"yuy2": 1, "uyvy": 1, "yvyu": 1, "y210": 2, "y212": 2, "y216": 2, "vuya": 1, "y410": 4, "y416": 2, "v210": 4}


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
    listed = [ln.strip() for ln in open(os.path.join(ROOT, "include", "srcnn_amd_yuv_packed_rect_list.abi")) if ln.strip() and not ln.startswith("#")]
    assert listed == sorted(listed) and len(set(listed)) == len(listed)
    assert names == listed == sorted(S.YUV_PACKED_RECT_LIST_SYMBOLS) and len(names) == 3
    assert set(S.YUV_PACKED_RECT_LIST_SYMBOLS) <= set(S.C_ABI_SYMBOLS)
    header = open(os.path.join(ROOT, "include", HEADER)).read()
    assert "#define SRCNN_AMD_YUV_PACKED_RECT_LIST_VERSION 1" in header
    assert '#include "srcnn_amd_yuv_packed_rect.h"' in header and '#include "srcnn_amd_rect_list.h"' in header
    for section in ("Result.", "How.", "Memory.", "Overlap.", "Source rectangle.", "Stream.", "Scratch ", "Errors."):
        assert ("\n * " + section) in header, section
    exported = _exported(S.LIB_PATH)
    assert set(names) <= set(exported)
    assert exported == sorted(S.C_ABI_SYMBOLS + S.CXX_SYMBOLS + HANDLE_ONLY_HOOKS)
    version = int(re.search(r"#define SRCNN_AMD_YUV_PACKED_RECT_LIST_VERSION (\d+)", header).group(1))
    assert S.lib().srcnn_yuv_packed_rect_list_abi_version() == version == 1
    # the structs of the binding are the header's
    assert C.sizeof(S.YuvPackedRectItem) == 32 and C.sizeof(S.RectListPlan) == 40
    emap = open(os.path.join(ROOT, "libsrcnn_amd", "csrc", "exports.map")).read()
    assert "srcnn_*;" in emap and all(name in emap for name in names)          # exported by the pattern, and named in its comment
    assert "SRCNN_YUV_PACKED_RECT_LIST_UNFUSED=0" in S.debug_settings()


def test_no_older_header_mentions_the_new_names():
    names = _declared(HEADER)
    assert len(names) == 3
    for other in OLDER:
        text = open(os.path.join(ROOT, "include", other)).read()
        assert not set(names) & set(_declared(other)), other
        assert not any(n in text for n in names) and "srcnn_amd_yuv_packed_rect_list" not in text.lower() and "srcnn_yuv_packed_rect_item" not in text, other


def test_strict_only_build_exports_the_same_set(S):
    from libsrcnn_amd import build
    strict, _ = build.build_strict_only(verbose=False)
    assert _exported(strict) == _exported(S.LIB_PATH)
    assert set(S.YUV_PACKED_RECT_LIST_SYMBOLS) <= set(_exported(strict))


def test_header_compiles_as_c99_and_the_item_is_32_bytes(tmp_path):
    src = tmp_path / "use.c"
    src.write_text('#include "srcnn_amd_yuv_packed_rect_list.h"\n'
                   "typedef char item_is_32_bytes[sizeof(srcnn_yuv_packed_rect_item) == 32 ? 1 : -1];\n"
                   "int f(const void* src, void* out) { srcnn_yuv_packed_rect_item it[2]; srcnn_rect_list_plan p;\n"
                   "  it[0].x0 = 6; it[0].y0 = 2; it[0].rw = 6; it[0].rh = 4; it[0].dst = out; it[0].dst_pitch = 0;\n"
                   "  it[1] = it[0]; p.struct_size = (unsigned)sizeof p;\n"
                   "  return srcnn_yuv_packed_rect_list_abi_version()\n"
                   "  + srcnn_yuv_packed_upscale_rect_list_plan(SRCNN_YUVP_V210, 8, 8, 2.0f, SRCNN_FILTER_BICUBIC, it, 2, (unsigned)sizeof it[0], &p)\n"
                   "  + srcnn_yuv_packed_upscale_rect_list_dev(SRCNN_YUVP_V210, 8, 8, 2.0f, SRCNN_FILTER_BICUBIC, src, 0, it, 2, (unsigned)sizeof it[0], 0)\n"
                   "  + (int)p.atlases + SRCNN_AMD_YUV_PACKED_RECT_LIST_VERSION; }\n")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-c", str(src), "-I" + os.path.join(ROOT, "include"),
                           "-o", str(tmp_path / "use.o")])


# ---- argument rules: host buffers stand in for device memory, which is safe because every call below is refused before the
# device is looked up ----
def row_bytes(name, w):
    if name in ("yuy2", "uyvy", "yvyu"):
        return 4 * ((w + 1) // 2)
    if name in ("y210", "y212", "y216"):
        return 8 * ((w + 1) // 2)
    if name in ("vuya", "y410"):
        return 4 * w
    return 8 * w if name == "y416" else 128 * ((w + 47) // 48)


class Frame:
    """A 12 x 7 source frame and room for three rects of the 24 x 14 output, in one host array; everything starts on a multiple
    of 16."""

    def __init__(self, S, name="y210", w=12, h=7, mul=2.0, src_pitch=0, rects=((6, 2, 12, 6), (0, 0, 24, 14), (18, 10, 6, 4)), dst_pitch=0):
        self.S, self.name, self.w, self.h, self.mul, self.src_pitch = S, name, w, h, mul, src_pitch
        dw, _dh = S.output_size(w, h, mul)
        self.src_row = row_bytes(name, w)
        up = lambda n: (n + 15) & ~15   # noqa: E731
        size = up(max(src_pitch, self.src_row) * h)
        self.spans = [S.yuv_packed_span_bytes(name, dw, r[0], r[2])[2] for r in rects]
        sizes = [up(max(dst_pitch, n) * r[3]) for r, n in zip(rects, self.spans)]
        self.buf = np.zeros(size + sum(sizes) + 64, np.uint8)
        base = (self.buf.ctypes.data + 15) & ~15
        self.src, self.src_end = base, base + size
        self.src_last = base + max(src_pitch, self.src_row) * (h - 1) + self.src_row          # one past the frame's last byte
        pos = self.src_end
        self.items = []
        for r, sz in zip(rects, sizes):
            self.items.append(dict(x0=r[0], y0=r[1], rw=r[2], rh=r[3], dst=pos, pitch=dst_pitch))
            pos += sz

    def call(self, at=None, n=None, item_size=None, items="given", **kw):
        """The list call with frame arguments overridden by kw, or -- with at=k -- item k's fields."""
        S = self.S
        a = dict(fmt=self.name, w=self.w, h=self.h, multiply=self.mul, filt=2, src=self.src, src_pitch=self.src_pitch)
        its = [dict(i) for i in self.items]
        if at is None:
            a.update(kw)
        else:
            its[at].update(kw)
        arr = [(i["x0"], i["y0"], i["rw"], i["rh"], i["dst"], i["pitch"]) for i in its] if items == "given" else items
        try:
            S.yuv_packed_upscale_rect_list_dev(a["fmt"], a["w"], a["h"], a["multiply"], a["filt"], a["src"], a["src_pitch"], arr, None, n=n, item_size=item_size)
        except S.SrcnnError as e:
            self.message = str(e)
            return e.code
        return 0


def test_list_rules_and_frame_rules(S):
    p = Frame(S)
    # 1. the list itself
    assert p.call(item_size=C.sizeof(S.YuvPackedRectItem) - 8) == E_ARG and p.call(item_size=0) == E_ARG and p.call(item_size=64) == E_ARG
    assert p.call(items=None, n=3) == E_ARG                     # NULL items with n > 0
    assert p.call(n=0) == 0 and p.call(items=None, n=0) == 0           # nothing to do: SRCNN_OK, even without a device
    assert p.call(n=0, fmt=99, src=None, w=0) == 0                     # ... with nothing else looked at
    assert S.lib().srcnn_yuv_packed_upscale_rect_list_dev(-1, 0, 0, 0.0, 9, None, 0, None, 0, C.sizeof(S.YuvPackedRectItem), None) == 0
    assert p.call(n=0, item_size=8) == E_ARG                    # (the item size is checked first)
    big = (S.YuvPackedRectItem * 65537)()
    assert p.call(items=big, n=65537) == E_UNSUPPORTED
    assert p.call(items=big, n=65536) == E_ARG and "item 0:" in p.message      # 65536 are allowed: its first (all-zero) item is refused
    # the list comes before the frame
    assert p.call(fmt=99, item_size=8) == E_ARG and "item_size" in p.message
    assert p.call(fmt=99, items=big, n=65537) == E_UNSUPPORTED
    # 2. the frame, with the codes and the order of srcnn_yuv_packed_upscale_rect_dev; no item is named
    for fmt in (-1, 10, 99):
        assert p.call(fmt=fmt) == E_ARG and "format" in p.message and "item" not in p.message
    assert p.call(src=None) == E_ARG and "NULL frame" in p.message and "item" not in p.message
    for filt in (-1, 5, 100):
        assert p.call(filt=filt) == E_ARG
    assert p.call(w=0) == E_ARG and p.call(h=0) == E_ARG
    assert p.call(multiply=0.0) == E_SCALE and p.call(multiply=0.05) == E_SCALE
    assert p.call(h=(1 << 20) + 1) == E_UNSUPPORTED
    assert p.call(src_pitch=p.src_row - 2) == E_ARG and "input pitch" in p.message and "item" not in p.message      # a source pitch below its row
    assert p.call(src_pitch=p.src_row + 1) == E_ARG and "item" not in p.message                                      # not a multiple of the alignment (2)
    assert p.call(src=p.src + 1) == E_ARG and "item" not in p.message
    # the order inside the frame: format < NULL source < filter < zero size < scale < limits < pitch
    assert p.call(fmt=99, src=None) == E_ARG and "format" in p.message
    assert p.call(src=None, filt=9) == E_ARG and "NULL frame" in p.message
    assert p.call(filt=9, w=0) == E_ARG and "filter" in p.message
    assert p.call(w=0, multiply=0.0) == E_ARG
    assert p.call(multiply=0.0, src_pitch=2) == E_SCALE
    assert p.call(h=(1 << 20) + 1, src_pitch=2) == E_UNSUPPORTED
    # 3. the frame comes before the items
    assert p.call(at=0, rw=0) == E_ARG and "item 0:" in p.message
    q = Frame(S)
    q.items[0]["rw"] = 0
    assert q.call(filt=7) == E_ARG and "item" not in q.message
    assert q.call(src_pitch=2) == E_ARG and "item" not in q.message


@pytest.mark.parametrize("at", [0, 2])
@pytest.mark.parametrize("name", ["yuy2", "y210", "y410", "v210"])
def test_item_rules_name_the_first_offender(S, at, name):
    u, al = UNIT[name], ALIGN[name]
    p = Frame(S, name=name, dst_pitch=256)
    it = p.items[at]
    n = p.spans[at]
    bad = [dict(dst=None), dict(rw=0), dict(rh=0), dict(x0=24, rw=1), dict(y0=14, rh=1), dict(x0=0xfffffffa, rw=12), dict(y0=0xfffffffc, rh=6),
           dict(rw=30, x0=0), dict(pitch=n - al), dict(dst=p.src), dict(dst=p.src_last - al)]
    if u > 1:
        bad += [dict(x0=it["x0"] + 1, rw=u), dict(x0=0, rw=u + 1)]                       # the unit rule: the origin, the count
    if al > 1:
        bad += [dict(pitch=257), dict(dst=it["dst"] + 1)]
    for kw in bad:
        assert p.call(at=at, **kw) == E_ARG, kw
        assert ("item %d:" % at) in p.message, (kw, p.message)
    # the order inside an item: NULL dst < empty < inside < unit rule < pitch < alignment < overlap
    order = [(dict(dst=None, rw=0), "NULL frame"), (dict(rw=0, x0=25), "empty rect"), (dict(x0=24 - u, rw=2 * u, pitch=2), "not inside"),
             (dict(pitch=n - al, dst=p.src), "output pitch"), (dict(dst=p.src), "overlap")]
    if u > 1:
        order.insert(3, (dict(x0=0, rw=u + 1, pitch=2), "multiple of %d" % u))
    if al > 1:
        order.insert(len(order) - 1, (dict(dst=p.src + 1), "output"))
    for kw, text in order:
        assert p.call(at=at, **kw) == E_ARG and text in p.message and ("item %d:" % at) in p.message, (kw, text, p.message)
    # the message after the prefix is the single call's
    kw = dict(x0=0, rw=u + 1) if u > 1 else dict(pitch=n - 1)
    one = dict(it, **kw)
    try:
        S.yuv_packed_upscale_rect_dev(name, p.w, p.h, p.mul, 2, p.src, 0, one["x0"], one["y0"], one["rw"], one["rh"], one["dst"], one["pitch"])
        single = None
    except S.SrcnnError as e:
        single = str(e)
    assert p.call(at=at, **kw) == E_ARG
    assert single and p.message == single.replace(": ", ": item %d: " % at, 1), (single, p.message)
    # an earlier offender wins
    q = Frame(S, name=name)
    q.items[1]["rw"] = 0
    assert q.call(at=2, rh=0) == E_ARG and "item 1:" in q.message


def test_valid_lists_reach_the_device_lookup_and_items_may_share_memory(S):
    if S.device_count() > 0:
        pytest.skip("a device is present: a valid call would run on host memory")
    for name in NAMES:
        assert Frame(S, name=name).call() == E_NODEVICE, name
        assert Frame(S, name=name, src_pitch=512, dst_pitch=256).call() == E_NODEVICE, name
    p = Frame(S, name="yuy2", dst_pitch=65)                        # alignment 1: odd bases and odd pitches are fine
    assert p.call(at=1, dst=p.items[1]["dst"] + 1) == E_NODEVICE
    assert Frame(S, name="v210", w=50, h=30, mul=0.75, rects=((0, 0, 37, 22), (36, 20, 1, 2))).call() == E_NODEVICE       # a rect that ends the row
    q = Frame(S, rects=((6, 2, 12, 6), (6, 4, 12, 6), (18, 10, 6, 4)))
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
    items = [(6, 2, 12, 6), (0, 0, 24, 14)]
    plan = S.yuv_packed_upscale_rect_list_plan
    code = lambda **kw: _code(S, lambda: plan("v210", 12, 7, 2.0, 2, items, **kw))   # noqa: E731
    assert code() == 0
    assert code(struct_size=0) == E_ARG and code(struct_size=C.sizeof(S.RectListPlan) + 8) == E_ARG
    assert code(item_size=64) == E_ARG
    assert _code(S, lambda: plan("v210", 12, 7, 2.0, 2, None, n=2)) == E_ARG
    assert _code(S, lambda: plan("v210", 12, 7, 2.0, 2, (S.YuvPackedRectItem * 65537)(), n=65537)) == E_UNSUPPORTED
    assert _code(S, lambda: plan(99, 12, 7, 2.0, 2, items)) == E_ARG
    assert _code(S, lambda: plan("v210", 12, 7, 0.0, 2, items)) == E_SCALE
    assert _code(S, lambda: plan("v210", 12, 7, 2.0, 7, items)) == E_ARG
    assert _code(S, lambda: plan("v210", 12, 7, 2.0, 2, items + [(18, 0, 12, 1)])) == E_ARG
    assert "item 2:" in S.lib().srcnn_last_error().decode()
    assert _code(S, lambda: plan("v210", 12, 7, 2.0, 2, items + [(0, 0, 6, 2), (3, 0, 6, 1)])) == E_ARG       # the unit rule
    assert "item 3:" in S.lib().srcnn_last_error().decode() and "multiple of 6" in S.lib().srcnn_last_error().decode()
    assert _code(S, lambda: plan("y410", 12, 7, 2.0, 2, [(3, 1, 1, 1)])) == 0
    # no address and no pitch is looked at: a NULL dst and an absurd pitch plan like any others
    assert plan_tuple(plan("v210", 12, 7, 2.0, 2, [(6, 2, 12, 6, None, 1)])) == (1, 0, 1)
    assert S.lib().srcnn_yuv_packed_upscale_rect_list_plan(9, 12, 7, 2.0, 2, None, 0, C.sizeof(S.YuvPackedRectItem), None) == E_ARG
    p = plan("v210", 12, 7, 2.0, 2, [])
    assert plan_tuple(p) == (0, 0, 0) and p.cell_samples == p.atlas_samples == p.scratch_bytes == 0
    p = plan(99, 0, 0, 0.0, 9, [])                     # n == 0: nothing else is looked at
    assert plan_tuple(p) == (0, 0, 0)


def small_rects(name, seed=64001, n=64, dw=192, dh=112, hi=40):
    from rect_list_worker import seeded_rects
    from yuv_packed_rect_worker import snap
    return [snap(r, name, dw) for r in seeded_rects(seed, n, dw, dh, hi=hi)]           # 96 x 56 -> 192 x 112 unless said otherwise


@pytest.mark.parametrize("name", NAMES)
def test_plan_batches_small_rects_and_states_the_headers_scratch(S, name):
    rects = small_rects(name)
    p = S.yuv_packed_upscale_rect_list_plan(name, 96, 56, 2.0, 2, rects)
    assert plan_tuple(p) == (64, 0, 1)
    y = S.y_path_rect_list_plan(96, 56, 192, 112, 2, rects)        # the packer is the same
    assert (p.cell_samples, p.atlas_samples) == (y.cell_samples, y.atlas_samples)
    assert p.cell_samples == sum((rw + 12) * (rh + 12) for (_, _, rw, rh) in rects)
    # the header: 136 B per sample of the largest atlas, 144 B per batched item, 144 B per atlas
    assert p.scratch_bytes == 136 * p.atlas_samples + 144 * 64 + 144 * 1
    header = open(os.path.join(ROOT, "include", HEADER)).read()
    assert "136 B per sample" in header and "144 B per batched item" in header and "144 B per atlas" in header


@pytest.mark.parametrize("name", NAMES)
def test_plan_sends_everything_else_the_single_way(S, name):
    plan = S.yuv_packed_upscale_rect_list_plan
    assert S.output_size(50, 30, 0.75) == (37, 22)
    assert plan_tuple(plan(name, 50, 30, 0.75, 2, small_rects(name, 5, 20, 37, 22, hi=15))) == (0, 20, 0)      # a down-scale
    assert plan_tuple(plan(name, 24, 24, 1.0, 2, small_rects(name, 7, 20, 24, 24, hi=15))) == (0, 20, 0)       # the identity size
    # a mixed-axis scale: 30 x 1 at x1.5 is 45 x 1, the rows keep their number
    assert S.output_size(30, 1, 1.5) == (45, 1)
    assert plan_tuple(plan(name, 30, 1, 1.5, 2, small_rects(name, 6, 20, 45, 1, hi=15))) == (0, 20, 0)
    # a CHROMA axis that keeps its size while luma grows in both: 1 x 9 at x2 is 2 x 18, one 4:2:2 chroma column before and after
    assert S.output_size(1, 9, 2.0) == (2, 18)
    rects = small_rects(name, 8, 20, 2, 18, hi=15)
    assert plan_tuple(S.y_path_rect_list_plan(1, 9, 2, 18, 2, rects)) == (20, 0, 1)                     # (the Y list batches them)
    assert plan_tuple(plan(name, 1, 9, 2.0, 2, rects)) == ((20, 0, 1) if UNIT[name] == 1 else (0, 20, 0))  # (4:4:4 has no such axis)
    # an item at or above SRCNN_RECT_LIST_SINGLE_SAMPLES = 2^21 samples of its cell is single, one just below is batched
    at, below = (0, 0, 2040, 1020), (0, 0, 2040, 1008)
    assert (at[2] + 12) * (at[3] + 12) >= 1 << 21 > (below[2] + 12) * (below[3] + 12)
    p = plan(name, 1020, 510, 2.0, 2, [at, below, (6, 6, 30, 30)])
    assert plan_tuple(p) == (2, 1, 1)


def test_plan_follows_the_y_list_exactly_where_the_chroma_grid_grows(S):
    """The chroma filter has at most 2 taps, so on a growing chroma grid a tile of 64 (60) x 16 chroma samples never reads more
    than the 72 x 24 source samples the tile resampler stages: yuvp_window_fits refuses no shape a real table produces (synthetic
    tables that it must refuse are driven through the router by tests/host/yuv_packed_rect_list_sanitize.cpp).  So the plan
    batches exactly what the Y list batches where the chroma grid grows in both axes, and nothing where it does not."""
    plan = S.yuv_packed_upscale_rect_list_plan
    grew = set()
    for name in ("yuy2", "y410", "v210"):
        for (w, h, mul) in ((96, 56, 2.0), (40, 31, 1.5), (63, 40, 1.02), (250, 40, 1.01), (3, 40, 1.5)):
            dw, dh = S.output_size(w, h, mul)
            cc = (lambda v: v) if UNIT[name] == 1 else (lambda v: (v + 1) // 2)
            grows = cc(dw) > cc(w) and dh > h
            grew.add(grows)
            rects = small_rects(name, 11, 24, dw, dh, hi=80) + [(0, 0, dw, dh)]
            for r in rects:
                yb = S.y_path_rect_list_plan(w, h, dw, dh, 2, [r]).batched_items
                assert plan(name, w, h, mul, 2, [r]).batched_items == (yb if grows else 0), (name, w, h, mul, r)
    assert grew == {True, False}


def test_plan_with_the_switch_set_is_all_single(S):
    # the switches are read when the library loads: processes of their own
    code = ("import libsrcnn_amd as S, sys; sys.path.insert(0, %r); from rect_list_worker import seeded_rects; from yuv_packed_rect_worker import snap;"
            "rects = [snap(r, 'v210', 192) for r in seeded_rects(64001, 64)];"
            "p = S.yuv_packed_upscale_rect_list_plan('v210', 96, 56, 2.0, 2, rects);"
            "y = S.y_path_rect_list_plan(96, 56, 192, 112, 2, rects);"
            "print('PLAN', p.batched_items, p.single_items, p.atlases, 'Y', y.batched_items)" % os.path.join(ROOT, "tests"))
    r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, SRCNN_YUV_PACKED_RECT_LIST_UNFUSED="1"), cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "PLAN 0 64 0 Y 64" in r.stdout, r.stdout[-500:] + r.stderr[-1500:]      # (the Y list has a switch of its own)
    r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, SRCNN_RECT_LIST_SINGLE_SAMPLES="1000"), cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-1500:]
    nb = sum((rw + 12) * (rh + 12) < 1000 for (_, _, rw, rh) in small_rects("v210"))
    assert 0 < nb < 64 and ("PLAN %d %d 1 Y %d" % (nb, 64 - nb, nb)) in r.stdout, r.stdout          # the shared threshold, on the cell's samples


def test_plan_in_a_non_parity_mode_is_all_single(S):
    prev = S.set_mode(S.MODE_FAST)           # (a strict-only build refuses: conftest turns that into a skip)
    try:
        p = S.yuv_packed_upscale_rect_list_plan("y416", 96, 56, 2.0, 2, small_rects("y416"))
    finally:
        S.set_mode(prev)
    assert plan_tuple(p) == (0, 64, 0) and p.scratch_bytes == 0
    assert plan_tuple(S.yuv_packed_upscale_rect_list_plan("y416", 96, 56, 2.0, 2, small_rects("y416"))) == (64, 0, 1)


def test_plan_lower_workspace_limit_raises_atlases(S):
    for name in ("uyvy", "v210"):
        rects = small_rects(name)
        one = S.yuv_packed_upscale_rect_list_plan(name, 96, 56, 2.0, 2, rects)
        prev = S.lib().srcnn_set_workspace_limit(1 << 20)
        try:
            p = S.yuv_packed_upscale_rect_list_plan(name, 96, 56, 2.0, 2, rects)
        finally:
            S.lib().srcnn_set_workspace_limit(prev)
        assert one.atlases == 1 and p.atlases >= 2 and p.batched_items == 64
        assert 128 * p.atlas_samples <= p.atlases << 20               # every atlas obeys the cap
        assert p.scratch_bytes < one.scratch_bytes                    # scratch is the LARGEST atlas, not their sum
        assert p.scratch_bytes == 136 * max_atlas(S, name, rects, 1 << 20) + 144 * (64 + p.atlases)
        assert S.yuv_packed_upscale_rect_list_plan(name, 96, 56, 2.0, 2, rects).atlases == 1


def max_atlas(S, name, rects, limit):
    """Samples of the largest atlas under `limit`, from the header's formula solved for it with the Y list's plan: the packer
    is shared, and the Y list states 136 B per sample and 80 B per entry."""
    prev = S.lib().srcnn_set_workspace_limit(limit)
    try:
        y = S.y_path_rect_list_plan(96, 56, 192, 112, 2, rects)
    finally:
        S.lib().srcnn_set_workspace_limit(prev)
    rest = y.scratch_bytes - 80 * (y.batched_items + y.atlases)
    assert rest % 136 == 0
    return rest // 136
