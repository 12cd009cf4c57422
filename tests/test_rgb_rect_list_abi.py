"""CPU: the RGB(A) rect list extension (include/srcnn_amd_rgb_rect_list.h) -- its declared functions, committed list, binding
and export table agree (full and strict-only builds), the header is C99, no older header mentions the new names, every frame
rule and every item rule of srcnn_rgb_upscale_rect_list_dev returns its code before any device lookup (host buffers stand in for
device planes), and srcnn_rgb_upscale_rect_list_plan, which runs the call's own routing and packing without a device, reports
what the header states."""
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
         "libsrcnn_dropin.h")
HEADER = "srcnn_amd_rgb_rect_list.h"
INTER, PLANAR = 0, 1


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
    listed = [ln.strip() for ln in open(os.path.join(ROOT, "include", "srcnn_amd_rgb_rect_list.abi")) if ln.strip() and not ln.startswith("#")]
    assert listed == sorted(listed) and len(set(listed)) == len(listed)
    assert names == listed == sorted(S.RGB_RECT_LIST_SYMBOLS) and len(names) == 3
    assert set(S.RGB_RECT_LIST_SYMBOLS) <= set(S.C_ABI_SYMBOLS)
    header = open(os.path.join(ROOT, "include", HEADER)).read()
    assert "#define SRCNN_AMD_RGB_RECT_LIST_VERSION 1" in header
    assert '#include "srcnn_amd_rgb_rect.h"' in header and '#include "srcnn_amd_rect_list.h"' in header
    exported = _exported(S.LIB_PATH)
    assert set(names) <= set(exported)
    assert exported == sorted(S.C_ABI_SYMBOLS + S.CXX_SYMBOLS + HANDLE_ONLY_HOOKS)
    assert S.lib().srcnn_rgb_rect_list_abi_version() == 1
    # the structs of the binding are the header's
    assert C.sizeof(S.RgbRectItem) == 96 and C.sizeof(S.RectListPlan) == 40
    emap = open(os.path.join(ROOT, "libsrcnn_amd", "csrc", "exports.map")).read()
    assert "srcnn_*;" in emap and all(name in emap for name in names)          # exported by the pattern, and named in its comment
    assert "SRCNN_RGB_RECT_LIST_UNFUSED=0" in S.debug_settings()


def test_no_older_header_mentions_the_new_names():
    names = _declared(HEADER)
    assert len(names) == 3
    for other in OLDER:
        text = open(os.path.join(ROOT, "include", other)).read()
        assert not set(names) & set(_declared(other)), other
        assert not any(n in text for n in names) and "srcnn_amd_rgb_rect_list" not in text.lower() and "srcnn_rgb_rect_item" not in text, other


def test_strict_only_build_exports_the_same_set(S):
    from libsrcnn_amd import build
    strict, _ = build.build_strict_only(verbose=False)
    assert _exported(strict) == _exported(S.LIB_PATH)
    assert set(S.RGB_RECT_LIST_SYMBOLS) <= set(_exported(strict))


def test_header_compiles_as_c99_and_the_item_is_96_bytes(tmp_path):
    src = tmp_path / "use.c"
    src.write_text('#include "srcnn_amd_rgb_rect_list.h"\n'
                   "typedef char item_is_96_bytes[sizeof(srcnn_rgb_rect_item) == 96 ? 1 : -1];\n"
                   "int f(const void* const src[4], void* out) { srcnn_rgb_rect_item it[2]; srcnn_rect_list_plan p; srcnn_rgb_format fmt;\n"
                   "  int k; fmt.struct_size = (unsigned)sizeof fmt; fmt.layout = SRCNN_RGB_INTERLEAVED; fmt.order = SRCNN_RGB_ORDER_RGB; fmt.alpha = 0; fmt.depth = 8;\n"
                   "  it[0].x0 = 1; it[0].y0 = 2; it[0].rw = 3; it[0].rh = 4; it[0].dst_conv = 0; it[0].dst_conv_pitch = 0;\n"
                   "  for (k = 0; k < 4; ++k) { it[0].dst[k] = k ? 0 : out; it[0].dst_pitch[k] = 0; }\n"
                   "  it[1] = it[0]; p.struct_size = (unsigned)sizeof p;\n"
                   "  return srcnn_rgb_rect_list_abi_version()\n"
                   "  + srcnn_rgb_upscale_rect_list_plan(&fmt, 8, 8, 2.0f, SRCNN_FILTER_BICUBIC, it, 2, (unsigned)sizeof it[0], &p)\n"
                   "  + srcnn_rgb_upscale_rect_list_dev(&fmt, 8, 8, 2.0f, SRCNN_FILTER_BICUBIC, src, 0, it, 2, (unsigned)sizeof it[0], 0)\n"
                   "  + (int)p.atlases + SRCNN_AMD_RGB_RECT_LIST_VERSION; }\n")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-c", str(src), "-I" + os.path.join(ROOT, "include"),
                           "-o", str(tmp_path / "use.o")])


# ---- argument rules: host buffers stand in for device planes, which is safe because every call below is refused before the
# device is looked up ----
class Planes:
    """A 9 x 7 source image and room for three rects of the 18 x 14 output (and their dst_conv planes), in one host array; every
    plane starts on an even address."""

    def __init__(self, S, layout=INTER, alpha=0, depth=10, w=9, h=7, mul=2.0, src_pitch=None,
                 rects=((3, 2, 8, 6), (0, 0, 18, 14), (16, 13, 2, 1)), dst_pitch=0, conv_pitch=0):
        self.S, self.fmt = S, S.rgb_format(layout, 0, alpha, depth)
        self.w, self.h, self.mul, self.src_pitch = w, h, mul, src_pitch
        self.np = (3 + alpha) if layout == PLANAR else 1
        self.bps = 1 if depth == 8 else 2
        spp = 1 if layout == PLANAR else 3 + alpha
        even = lambda n: (n + 1) & ~1   # noqa: E731
        self.src_row = w * spp * self.bps
        self.src_size = even(max((src_pitch or [0])[0], self.src_row) * h)
        total = self.np * self.src_size
        self.dst_rows, sizes = [], []
        for (_, _, rw, rh) in rects:
            row = rw * spp * self.bps
            self.dst_rows.append(row)
            sizes.append((even(max(dst_pitch, row) * rh), even(max(conv_pitch, rw * self.bps) * rh)))
            total += self.np * sizes[-1][0] + sizes[-1][1]
        self.buf = np.zeros(total // 2 + 64, np.uint16)
        base = self.buf.ctypes.data
        self.src = [base + k * self.src_size for k in range(self.np)] + [None] * (4 - self.np)
        self.src_end = base + self.np * self.src_size
        pos = self.src_end
        self.items = []
        for r, (psize, csize) in zip(rects, sizes):
            dst = [pos + k * psize for k in range(self.np)]
            pos += self.np * psize
            self.items.append(dict(x0=r[0], y0=r[1], rw=r[2], rh=r[3], dst=dst, pitch=[dst_pitch] * self.np, conv=pos, conv_pitch=conv_pitch))
            pos += csize

    def call(self, at=None, n=None, item_size=None, items="given", **kw):
        """The list call with frame arguments overridden by kw, or -- with at=k -- item k's fields."""
        S = self.S
        a = dict(fmt=self.fmt, w=self.w, h=self.h, multiply=self.mul, filt=2, src=self.src, src_pitch=self.src_pitch)
        its = [dict(i) for i in self.items]
        if at is None:
            a.update(kw)
        else:
            its[at].update(kw)
        arr = [(i["x0"], i["y0"], i["rw"], i["rh"], i["dst"], i["pitch"], i["conv"], i["conv_pitch"]) for i in its] if items == "given" else items
        try:
            S.rgb_upscale_rect_list_dev(a["fmt"], a["w"], a["h"], a["multiply"], a["filt"], a["src"], a["src_pitch"], arr, None, n=n, item_size=item_size)
        except S.SrcnnError as e:
            self.message = str(e)
            return e.code
        return 0


def test_list_rules_and_frame_rules(S):
    p = Planes(S)
    # the list itself
    assert p.call(item_size=C.sizeof(S.RgbRectItem) - 8) == E_ARG and p.call(item_size=0) == E_ARG and p.call(item_size=32) == E_ARG
    assert p.call(items=None, n=3) == E_ARG                     # NULL items with n > 0
    assert p.call(n=0) == 0 and p.call(items=None, n=0) == 0           # nothing to do: SRCNN_OK, even without a device
    assert p.call(n=0, item_size=8) == E_ARG                    # (the item size is checked first)
    big = (S.RgbRectItem * 65537)()
    assert p.call(items=big, n=65537) == E_UNSUPPORTED
    assert p.call(items=big, n=65536) == E_ARG and "item 0:" in p.message      # 65536 are allowed: its first (all-zero) item is refused
    # the frame, with the codes of srcnn_rgb_upscale_rect_dev; no item is named
    assert p.call(fmt=None) == E_ARG and "item" not in p.message
    for size in (0, 4, 19, 24):
        fmt = S.rgb_format(INTER, 0, 0, 10)
        fmt.struct_size = size
        assert p.call(fmt=fmt) == E_ARG, size
    assert p.call(fmt=S.rgb_format(2, 0, 0, 10)) == E_ARG and p.call(fmt=S.rgb_format(INTER, 2, 0, 10)) == E_ARG
    assert p.call(fmt=S.rgb_format(INTER, 0, 2, 10)) == E_ARG and p.call(fmt=S.rgb_format(INTER, 0, 0, 9)) == E_ARG
    assert p.call(src=None) == E_ARG and p.call(src=[None]) == E_ARG
    for filt in (-1, 5, 100):
        assert p.call(filt=filt) == E_ARG
    assert p.call(w=0) == E_ARG and p.call(h=0) == E_ARG
    assert p.call(multiply=0.0) == E_SCALE and p.call(multiply=0.05) == E_SCALE
    assert p.call(h=(1 << 20) + 1) == E_UNSUPPORTED
    assert p.call(src_pitch=[p.src_row - 2]) == E_ARG and "item" not in p.message            # a source pitch below its row
    assert p.call(src_pitch=[p.src_row + 1]) == E_ARG and p.call(src=[p.src[0] + 1]) == E_ARG     # odd above 8 bits
    # the frame comes before the items
    assert p.call(at=0, rw=0) == E_ARG and "item 0:" in p.message
    q = Planes(S)
    q.items[0]["rw"] = 0
    assert q.call(filt=7) == E_ARG and "item" not in q.message
    planar = Planes(S, layout=PLANAR, alpha=1)
    for k in range(4):
        src = list(planar.src); src[k] = None
        assert planar.call(src=src) == E_ARG and "item" not in planar.message, k


@pytest.mark.parametrize("at", [0, 2])
@pytest.mark.parametrize("layout", [INTER, PLANAR])
def test_item_rules_name_the_first_offender(S, at, layout):
    p = Planes(S, layout=layout, alpha=1, dst_pitch=256, conv_pitch=128)
    it = p.items[at]
    row = p.dst_rows[at]

    def planes(k, v):
        d = list(it["dst"]); d[k] = v
        return d

    def pitches(k, v):
        d = list(it["pitch"]); d[k] = v
        return d
    bad = [dict(rw=0), dict(rh=0), dict(x0=18, rw=1), dict(y0=14, rh=1), dict(x0=0xfffffffe, rw=4), dict(y0=0xfffffffd, rh=6), dict(rw=19, x0=0),
           dict(conv_pitch=it["rw"] * 2 - 2), dict(conv=it["conv"] + 1), dict(conv_pitch=129),
           dict(conv=p.src[0]), dict(conv=p.src_end - 2), dict(conv=it["dst"][0])]
    for k in range(p.np):
        bad += [dict(dst=planes(k, None)), dict(pitch=pitches(k, row - 2)), dict(pitch=pitches(k, 257)), dict(dst=planes(k, it["dst"][k] + 1)),
                dict(dst=planes(k, p.src[0])), dict(dst=planes(k, p.src_end - 2))]
    if p.np > 1:
        bad += [dict(dst=planes(1, it["dst"][0])), dict(dst=planes(3, it["dst"][2] + 2))]          # two destination planes of the item overlap
    for kw in bad:
        assert p.call(at=at, **kw) == E_ARG, kw
        assert ("item %d:" % at) in p.message, (kw, p.message)
    # an earlier offender wins
    q = Planes(S, layout=layout)
    q.items[1]["rw"] = 0
    assert q.call(at=2, rh=0) == E_ARG and "item 1:" in q.message


def test_depth_8_needs_no_alignment_and_items_may_share_memory(S):
    if S.device_count() > 0:
        pytest.skip("a device is present: a valid call would run on host memory")
    p = Planes(S, depth=8)
    assert p.call() == E_NODEVICE
    assert p.call(at=1, dst=[p.items[1]["dst"][0] + 1], pitch=[55], conv=None) == E_NODEVICE      # odd base, odd pitch >= 54 (over its unused conv plane)
    assert Planes(S, layout=PLANAR, alpha=1, depth=12, src_pitch=[64] * 4, dst_pitch=128, conv_pitch=64).call() == E_NODEVICE
    assert Planes(S, w=50, h=30, mul=0.75, rects=((0, 0, 37, 22), (36, 21, 1, 1))).call() == E_NODEVICE
    assert p.call(at=0, conv=None) == E_NODEVICE                   # dst_conv is per item
    q = Planes(S)
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
    fmt = S.rgb_format()
    items = [(3, 2, 8, 6), (0, 0, 18, 14)]
    code = lambda **kw: _code(S, lambda: S.rgb_upscale_rect_list_plan(fmt, 9, 7, 2.0, 2, items, **kw))   # noqa: E731
    assert code() == 0
    assert code(struct_size=0) == E_ARG and code(struct_size=C.sizeof(S.RectListPlan) + 8) == E_ARG
    assert code(item_size=32) == E_ARG
    assert _code(S, lambda: S.rgb_upscale_rect_list_plan(fmt, 9, 7, 2.0, 2, None, n=2)) == E_ARG
    assert _code(S, lambda: S.rgb_upscale_rect_list_plan(fmt, 9, 7, 2.0, 2, (S.RgbRectItem * 65537)(), n=65537)) == E_UNSUPPORTED
    assert _code(S, lambda: S.rgb_upscale_rect_list_plan(None, 9, 7, 2.0, 2, items)) == E_ARG
    assert _code(S, lambda: S.rgb_upscale_rect_list_plan(fmt, 9, 7, 0.0, 2, items)) == E_SCALE
    assert _code(S, lambda: S.rgb_upscale_rect_list_plan(fmt, 9, 7, 2.0, 7, items)) == E_ARG
    assert _code(S, lambda: S.rgb_upscale_rect_list_plan(fmt, 9, 7, 2.0, 2, items + [(17, 0, 2, 1)])) == E_ARG
    assert "item 2:" in S.lib().srcnn_last_error().decode()
    assert S.lib().srcnn_rgb_upscale_rect_list_plan(C.byref(fmt), 9, 7, 2.0, 2, None, 0, C.sizeof(S.RgbRectItem), None) == E_ARG
    p = S.rgb_upscale_rect_list_plan(fmt, 9, 7, 2.0, 2, [])
    assert plan_tuple(p) == (0, 0, 0) and p.cell_samples == p.atlas_samples == p.scratch_bytes == 0


@pytest.mark.parametrize("cell", [(INTER, 0, 8), (PLANAR, 1, 12)])
def test_plan_packs_as_the_y_list_and_states_the_headers_scratch(S, cell):
    from rect_list_worker import seeded_rects
    rects = seeded_rects(64001, 64)                                # 96 x 56 -> 192 x 112, 1 ... 40 samples a side
    fmt = S.rgb_format(cell[0], 0, cell[1], cell[2])
    p = S.rgb_upscale_rect_list_plan(fmt, 96, 56, 2.0, 2, rects)
    assert plan_tuple(p) == (64, 0, 1)
    y = S.y_path_rect_list_plan(96, 56, 192, 112, 2, rects)        # the packer is the same
    assert (p.cell_samples, p.atlas_samples) == (y.cell_samples, y.atlas_samples)
    assert p.cell_samples == sum((rw + 12) * (rh + 12) for (_, _, rw, rh) in rects)
    # the header: 136 B per sample of the largest atlas, 168 B per batched item, 80 B per atlas
    assert p.scratch_bytes == 136 * p.atlas_samples + 168 * 64 + 80 * 1
    header = open(os.path.join(ROOT, "include", HEADER)).read()
    assert "136 B per sample" in header and "168 B per batched item" in header and "80 B per atlas" in header


def test_plan_sends_everything_else_the_single_way(S):
    from rect_list_worker import seeded_rects
    fmt = S.rgb_format()
    assert plan_tuple(S.rgb_upscale_rect_list_plan(fmt, 50, 30, 0.75, 2, seeded_rects(5, 20, 37, 22, hi=15))) == (0, 20, 0)      # a down-scale
    assert S.output_size(50, 30, 0.75) == (37, 22)
    assert plan_tuple(S.rgb_upscale_rect_list_plan(fmt, 24, 24, 1.0, 2, seeded_rects(7, 20, 24, 24, hi=15))) == (0, 20, 0)       # the identity size
    # an axis that keeps its size while the other grows: 30 x 1 at x1.5 is 45 x 1
    assert S.output_size(30, 1, 1.5) == (45, 1)
    assert plan_tuple(S.rgb_upscale_rect_list_plan(fmt, 30, 1, 1.5, 2, seeded_rects(6, 20, 45, 1, hi=15))) == (0, 20, 0)
    # the switches are read when the library loads: processes of their own
    code = ("import libsrcnn_amd as S, sys; sys.path.insert(0, %r); from rect_list_worker import seeded_rects;"
            "p = S.rgb_upscale_rect_list_plan(S.rgb_format(), 96, 56, 2.0, 2, seeded_rects(64001, 64));"
            "y = S.y_path_rect_list_plan(96, 56, 192, 112, 2, seeded_rects(64001, 64));"
            "print('PLAN', p.batched_items, p.single_items, p.atlases, 'Y', y.batched_items)" % os.path.join(ROOT, "tests"))
    r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, SRCNN_RGB_RECT_LIST_UNFUSED="1"), cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "PLAN 0 64 0 Y 64" in r.stdout, r.stdout[-500:] + r.stderr[-1500:]      # (the Y list has a switch of its own)
    r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, SRCNN_RECT_LIST_SINGLE_SAMPLES="1000"), cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-1500:]
    nb = sum((rw + 12) * (rh + 12) < 1000 for (_, _, rw, rh) in seeded_rects(64001, 64))
    assert 0 < nb < 64 and ("PLAN %d %d 1 Y %d" % (nb, 64 - nb, nb)) in r.stdout, r.stdout          # the shared threshold, on the cell's samples


def test_plan_lower_workspace_limit_raises_atlases(S):
    from rect_list_worker import seeded_rects
    rects = seeded_rects(64001, 64)
    fmt = S.rgb_format()
    one = S.rgb_upscale_rect_list_plan(fmt, 96, 56, 2.0, 2, rects)
    prev = S.lib().srcnn_set_workspace_limit(1 << 20)
    try:
        p = S.rgb_upscale_rect_list_plan(fmt, 96, 56, 2.0, 2, rects)
    finally:
        S.lib().srcnn_set_workspace_limit(prev)
    assert one.atlases == 1 and p.atlases >= 3 and p.batched_items == 64
    assert 128 * p.atlas_samples <= p.atlases << 20               # every atlas obeys the cap
    assert p.scratch_bytes < one.scratch_bytes                    # scratch is the LARGEST atlas, not their sum
    assert S.rgb_upscale_rect_list_plan(fmt, 96, 56, 2.0, 2, rects).atlases == 1
