"""CPU: the rect list extension (include/srcnn_amd_rect_list.h) -- its declared functions, committed list, binding and export
table agree (full and strict-only builds), the header is C99, no older header mentions the new names, every argument rule of
srcnn_y_path_rect_list_f32_dev returns its code before any device lookup (host buffers stand in for device planes), and
srcnn_y_path_rect_list_plan, which runs the call's own routing and packing without a device, reports what the issue demands."""
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
         "srcnn_amd_rect.h", "srcnn_amd_rgb_rect.h", "srcnn_amd_yuv_rect.h", "srcnn_amd_yuv_packed_rect.h", "libsrcnn_dropin.h")
HEADER = "srcnn_amd_rect_list.h"


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
    listed = [ln.strip() for ln in open(os.path.join(ROOT, "include", "srcnn_amd_rect_list.abi")) if ln.strip() and not ln.startswith("#")]
    assert listed == sorted(listed) and len(set(listed)) == len(listed)
    assert names == listed == sorted(S.RECT_LIST_SYMBOLS) and len(names) == 3
    assert set(S.RECT_LIST_SYMBOLS) <= set(S.C_ABI_SYMBOLS)
    header = open(os.path.join(ROOT, "include", HEADER)).read()
    assert "#define SRCNN_AMD_RECT_LIST_VERSION 1" in header and '#include "srcnn_amd.h"' in header
    exported = _exported(S.LIB_PATH)
    assert set(names) <= set(exported)
    assert exported == sorted(S.C_ABI_SYMBOLS + S.CXX_SYMBOLS + HANDLE_ONLY_HOOKS)
    assert S.lib().srcnn_rect_list_abi_version() == 1
    # the structs of the binding are the header's
    assert C.sizeof(S.RectItem) == 32 and C.sizeof(S.RectListPlan) == 40
    emap = open(os.path.join(ROOT, "libsrcnn_amd", "csrc", "exports.map")).read()
    assert "srcnn_*;" in emap and all(name in emap for name in names)          # exported by the pattern, and named in its comment


def test_no_older_header_mentions_the_new_names():
    names = _declared(HEADER)
    assert len(names) == 3
    for other in OLDER:
        text = open(os.path.join(ROOT, "include", other)).read()
        assert not set(names) & set(_declared(other)), other
        assert not any(n in text for n in names) and "srcnn_amd_rect_list" not in text.lower() and "srcnn_rect_item" not in text, other


def test_strict_only_build_exports_the_same_set(S):
    from libsrcnn_amd import build
    strict, _ = build.build_strict_only(verbose=False)
    assert _exported(strict) == _exported(S.LIB_PATH)
    assert set(S.RECT_LIST_SYMBOLS) <= set(_exported(strict))


def test_header_compiles_as_c99(tmp_path):
    src = tmp_path / "use.c"
    src.write_text('#include "srcnn_amd_rect_list.h"\n'
                   "int f(const float* in, float* out) { srcnn_rect_item it[2]; srcnn_rect_list_plan p;\n"
                   "  it[0].x0 = 1; it[0].y0 = 2; it[0].rw = 3; it[0].rh = 4; it[0].d_out = out; it[0].out_pitch = 0; it[1] = it[0];\n"
                   "  p.struct_size = (unsigned)sizeof p;\n"
                   "  return srcnn_rect_list_abi_version() + srcnn_y_path_rect_list_plan(8, 8, 16, 16, SRCNN_FILTER_BICUBIC, it, 2, (unsigned)sizeof it[0], &p)\n"
                   "  + srcnn_y_path_rect_list_f32_dev(in, 0, 8, 8, 16, 16, SRCNN_FILTER_BICUBIC, it, 2, (unsigned)sizeof it[0], 0)\n"
                   "  + (int)p.atlases + SRCNN_AMD_RECT_LIST_VERSION; }\n")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-c", str(src), "-I" + os.path.join(ROOT, "include"),
                           "-o", str(tmp_path / "use.o")])


# ---- argument rules: host buffers stand in for device planes, which is safe because every call below is refused before the
# device is looked up ----
class Planes:
    """A 9 x 7 source and room for three rects of the 18 x 14 output, in one host array."""

    def __init__(self, w=9, h=7, dw=18, dh=14, in_pitch=0, rects=((3, 2, 8, 6), (0, 0, 18, 14), (16, 13, 2, 1)), out_pitch=0):
        self.w, self.h, self.dw, self.dh, self.in_pitch = w, h, dw, dh, in_pitch
        self.in_bytes = max(in_pitch, 4 * w) * h
        sizes = [max(out_pitch, 4 * r[2]) * r[3] for r in rects]
        self.buf = np.zeros((self.in_bytes + sum(sizes)) // 4 + 64, np.float32)
        self.src = self.buf.ctypes.data
        self.items, pos = [], self.src + self.in_bytes
        for r, n in zip(rects, sizes):
            self.items.append(dict(x0=r[0], y0=r[1], rw=r[2], rh=r[3], dst=pos, pitch=out_pitch))
            pos += n

    def call(self, S, at=None, n=None, item_size=None, items="given", **kw):
        """The list call with frame arguments overridden by kw, or -- with at=k -- item k's fields."""
        a = dict(src=self.src, in_pitch=self.in_pitch, w=self.w, h=self.h, dw=self.dw, dh=self.dh, filt=2)
        its = [dict(i) for i in self.items]
        if at is None:
            a.update(kw)
        else:
            its[at].update(kw)
        arr = [(i["x0"], i["y0"], i["rw"], i["rh"], i["dst"], i["pitch"]) for i in its] if items == "given" else items
        try:
            S.y_path_rect_list_dev(a["src"], a["in_pitch"], a["w"], a["h"], a["dw"], a["dh"], a["filt"], arr, None, n=n, item_size=item_size)
        except S.SrcnnError as e:
            self.message = str(e)
            return e.code
        return 0


def test_frame_rules_and_list_rules(S):
    p = Planes()
    assert p.call(S, src=None) == E_ARG
    assert p.call(S, w=0) == E_ARG and p.call(S, h=0) == E_ARG
    assert p.call(S, dw=0) == E_SCALE and p.call(S, dh=0) == E_SCALE
    for filt in (-1, 5, 100):
        assert p.call(S, filt=filt) == E_ARG
    assert p.call(S, in_pitch=4 * p.w - 4) == E_ARG and p.call(S, in_pitch=65) == E_ARG and p.call(S, src=p.src + 2) == E_ARG
    assert p.call(S, h=(1 << 20) + 1) == E_UNSUPPORTED and p.call(S, dw=1 << 23) == E_UNSUPPORTED
    # the list itself
    assert p.call(S, item_size=C.sizeof(S.RectItem) - 8) == E_ARG and p.call(S, item_size=0) == E_ARG and p.call(S, item_size=64) == E_ARG
    assert p.call(S, items=None, n=3) == E_ARG                     # NULL items with n > 0
    assert p.call(S, n=0) == 0 and p.call(S, items=None, n=0) == 0          # nothing to do: SRCNN_OK, even without a device
    assert p.call(S, n=0, item_size=8) == E_ARG                    # (the item size is checked first)
    big = (S.RectItem * 65537)()
    assert p.call(S, items=big, n=65537) == E_UNSUPPORTED
    assert p.call(S, items=big, n=65536) == E_ARG and "item 0:" in p.message      # 65536 are allowed: its first (empty) item is refused


@pytest.mark.parametrize("at", [0, 2])
def test_item_rules_name_the_first_offender(S, at):
    p = Planes(out_pitch=128)
    bad = [dict(dst=None), dict(rw=0), dict(rh=0), dict(x0=18, rw=1), dict(y0=14, rh=1), dict(x0=0xfffffffe, rw=4), dict(rw=19, x0=0),
           dict(pitch=4 * p.items[at]["rw"] - 4), dict(pitch=130), dict(dst=p.items[at]["dst"] + 2), dict(dst=p.src), dict(dst=p.src + p.in_bytes - 4)]
    for kw in bad:
        assert p.call(S, at=at, **kw) == E_ARG, kw
        assert ("item %d:" % at) in p.message, (kw, p.message)
    assert Planes(rects=((3, 2, 8, 6),) * 3).call(S, at=at, rh=65535 * 16 + 1, y0=0) == E_ARG      # (outside 18 x 14 first)
    # an earlier offender wins
    q = Planes()
    q.items[1]["rw"] = 0
    assert q.call(S, at=2, rh=0) == E_ARG and "item 1:" in q.message


def test_valid_lists_without_a_device(S):
    if S.device_count() > 0:
        pytest.skip("a device is present: a valid call would run on host memory")
    assert Planes().call(S) == E_NODEVICE
    assert Planes(in_pitch=64, out_pitch=128).call(S) == E_NODEVICE
    assert Planes(50, 30, 37, 20, rects=((0, 0, 37, 20), (36, 19, 1, 1))).call(S) == E_NODEVICE
    p = Planes()
    p.items[1]["dst"] = p.items[0]["dst"]                          # destinations that overlap are the caller's business
    assert p.call(S) == E_NODEVICE


# ---- the plan ----
def plan_tuple(p):
    return p.batched_items, p.single_items, p.atlases


def test_plan_struct_and_argument_rules(S):
    items = [(3, 2, 8, 6), (0, 0, 18, 14)]
    code = lambda **kw: _code(S, lambda: S.y_path_rect_list_plan(9, 7, 18, 14, 2, items, **kw))   # noqa: E731
    assert code() == 0
    assert code(struct_size=0) == E_ARG and code(struct_size=C.sizeof(S.RectListPlan) + 8) == E_ARG
    assert code(item_size=24) == E_ARG
    assert _code(S, lambda: S.y_path_rect_list_plan(9, 7, 18, 14, 2, None, n=2)) == E_ARG
    assert _code(S, lambda: S.y_path_rect_list_plan(9, 7, 18, 14, 2, (S.RectItem * 65537)(), n=65537)) == E_UNSUPPORTED
    assert _code(S, lambda: S.y_path_rect_list_plan(9, 7, 0, 14, 2, items)) == E_SCALE
    assert _code(S, lambda: S.y_path_rect_list_plan(9, 7, 18, 14, 7, items)) == E_ARG
    assert _code(S, lambda: S.y_path_rect_list_plan(9, 7, 18, 14, 2, items + [(17, 0, 2, 1)])) == E_ARG
    assert "item 2:" in S.lib().srcnn_last_error().decode()
    assert S.lib().srcnn_y_path_rect_list_plan(9, 7, 18, 14, 2, None, 0, C.sizeof(S.RectItem), None) == E_ARG
    p = S.y_path_rect_list_plan(9, 7, 18, 14, 2, [])
    assert plan_tuple(p) == (0, 0, 0) and p.cell_samples == p.atlas_samples == p.scratch_bytes == 0


def _code(S, fn):
    try:
        fn()
    except S.SrcnnError as e:
        return e.code
    return 0


def test_plan_batches_small_rects_of_an_upscale_under_the_cap(S):
    from rect_list_worker import seeded_rects
    rects = seeded_rects(64001, 64)                                # 96 x 56 -> 192 x 112, 1 ... 40 samples a side
    assert all(1 <= r[2] <= 40 and 1 <= r[3] <= 40 for r in rects)
    p = S.y_path_rect_list_plan(96, 56, 192, 112, 2, rects)
    assert plan_tuple(p) == (64, 0, 1)
    assert p.cell_samples == sum((rw + 12) * (rh + 12) for (_, _, rw, rh) in rects)
    assert p.cell_samples <= p.atlas_samples <= 2 * p.cell_samples
    assert p.scratch_bytes == 136 * p.atlas_samples + 80 * (64 + 1)
    # a plan is a function of the list
    q = S.y_path_rect_list_plan(96, 56, 192, 112, 2, rects)
    assert (q.atlas_samples, q.scratch_bytes) == (p.atlas_samples, p.scratch_bytes)


@pytest.mark.parametrize("n", [16, 17, 23, 26, 37, 64, 101])
@pytest.mark.parametrize("side", [1, 20, 52])
def test_plan_equal_cells_stay_under_the_cap_on_waste(S, n, side):
    rects = [((7 * k) % (192 - side), (5 * k) % (112 - side), side, side) for k in range(n)]
    p = S.y_path_rect_list_plan(96, 56, 192, 112, 2, rects)
    assert plan_tuple(p) == (n, 0, 1) and p.cell_samples == n * (side + 12) ** 2
    assert p.atlas_samples <= 2 * p.cell_samples                   # the cap of the issue
    assert 2 * p.atlas_samples <= 3 * p.cell_samples               # what a shelf packing of equal cells gives by hand: under 1.5


def test_plan_sends_everything_else_the_single_way(S):
    from rect_list_worker import seeded_rects
    down = seeded_rects(5, 20, 37, 20, hi=15)
    assert plan_tuple(S.y_path_rect_list_plan(50, 30, 37, 20, 2, down)) == (0, 20, 0)
    ident = seeded_rects(6, 20, 30, 40, hi=15)
    assert plan_tuple(S.y_path_rect_list_plan(30, 20, 30, 40, 2, ident)) == (0, 20, 0)      # the columns keep their size
    assert plan_tuple(S.y_path_rect_list_plan(24, 24, 24, 24, 2, seeded_rects(7, 20, 24, 24, hi=15))) == (0, 20, 0)
    # SRCNN_RECT_LIST_UNFUSED=1 is read when the library loads: a process of its own
    code = ("import libsrcnn_amd as S, sys; sys.path.insert(0, %r); from rect_list_worker import seeded_rects;"
            "p = S.y_path_rect_list_plan(96, 56, 192, 112, 2, seeded_rects(64001, 64)); print('PLAN', p.batched_items, p.single_items, p.atlases)"
            % os.path.join(ROOT, "tests"))
    r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, SRCNN_RECT_LIST_UNFUSED="1"), cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "PLAN 0 64 0" in r.stdout, r.stdout[-500:] + r.stderr[-1500:]
    r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, SRCNN_RECT_LIST_SINGLE_SAMPLES="1000"), cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-1500:]
    nb = sum((rw + 12) * (rh + 12) < 1000 for (_, _, rw, rh) in seeded_rects(64001, 64))
    assert 0 < nb < 64 and ("PLAN %d %d 1" % (nb, 64 - nb)) in r.stdout, r.stdout          # the threshold is on the cell's samples


def test_plan_lower_workspace_limit_raises_atlases(S):
    from rect_list_worker import seeded_rects
    rects = seeded_rects(64001, 64)
    one = S.y_path_rect_list_plan(96, 56, 192, 112, 2, rects)
    prev = S.lib().srcnn_set_workspace_limit(1 << 20)
    try:
        p = S.y_path_rect_list_plan(96, 56, 192, 112, 2, rects)
    finally:
        S.lib().srcnn_set_workspace_limit(prev)
    assert one.atlases == 1 and p.atlases >= 3 and p.batched_items == 64
    assert 128 * p.atlas_samples <= p.atlases << 20               # every atlas obeys the cap
    assert S.y_path_rect_list_plan(96, 56, 192, 112, 2, rects).atlases == 1
