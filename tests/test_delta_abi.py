"""CPU: the delta extension (include/srcnn_amd_delta.h) -- its declared functions, committed list, binding and export table agree
(full and strict-only builds), the header is C99, no older header mentions the new names, every argument rule of the two device
calls returns its code before any device lookup (host buffers stand in for device planes), srcnn_y_path_delta_grid reports the
grids of the issue, the coalescer srcnn_y_path_delta_rects follows its one rule (a Python restatement, seeded grids and hand
cases), and the whole-frame rule and its settings row are what the header states."""
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
         "srcnn_amd_rgb_rect_list.h", "srcnn_amd_yuv_rect_list.h", "srcnn_amd_yuv_packed_rect_list.h", "libsrcnn_dropin.h")
HEADER = "srcnn_amd_delta.h"


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


def test_header_list_binding_and_exports_agree(S):
    names = _declared(HEADER)
    listed = [ln.strip() for ln in open(os.path.join(ROOT, "include", "srcnn_amd_delta.abi")) if ln.strip() and not ln.startswith("#")]
    assert listed == sorted(listed) and len(set(listed)) == len(listed)
    assert names == listed == sorted(S.DELTA_SYMBOLS) and len(names) == 5
    assert set(S.DELTA_SYMBOLS) <= set(S.C_ABI_SYMBOLS)
    header = open(os.path.join(ROOT, "include", HEADER)).read()
    assert "#define SRCNN_AMD_DELTA_VERSION 1" in header and '#include "srcnn_amd_rect_list.h"' in header
    exported = _exported(S.LIB_PATH)
    assert set(names) <= set(exported)
    assert exported == sorted(S.C_ABI_SYMBOLS + S.CXX_SYMBOLS + HANDLE_ONLY_HOOKS)
    assert S.lib().srcnn_delta_abi_version() == 1
    assert C.sizeof(S.DeltaStats) == 32 and C.sizeof(S.RectItem) == 32          # the structs of the binding are the header's
    emap = open(os.path.join(ROOT, "libsrcnn_amd", "csrc", "exports.map")).read()
    assert "srcnn_*;" in emap and all(name in emap for name in names)          # exported by the pattern, and named in its comment


def test_no_older_header_mentions_the_new_names():
    names = _declared(HEADER)
    assert len(names) == 5
    for other in OLDER:
        text = open(os.path.join(ROOT, "include", other)).read()
        assert not set(names) & set(_declared(other)), other
        assert not any(n in text for n in names) and "srcnn_amd_delta" not in text.lower() and "srcnn_delta_stats" not in text, other


def test_strict_only_build_exports_the_same_set(S):
    from libsrcnn_amd import build
    strict, _ = build.build_strict_only(verbose=False)
    assert _exported(strict) == _exported(S.LIB_PATH)
    assert set(S.DELTA_SYMBOLS) <= set(_exported(strict))


def test_header_compiles_as_c99_and_struct_sizes_match(S, tmp_path):
    src = tmp_path / "use.c"
    src.write_text('#include "srcnn_amd_delta.h"\n'
                   "int f(const float* a, const float* b, float* out, unsigned char* fl) { srcnn_delta_stats st; srcnn_rect_item it[2]; unsigned c, r, n;\n"
                   "  st.struct_size = (unsigned)sizeof st;\n"
                   "  return srcnn_delta_abi_version() + srcnn_y_path_delta_grid(8, 8, 16, 16, SRCNN_FILTER_BICUBIC, 0, 0, &c, &r)\n"
                   "  + srcnn_y_path_delta_flags_dev(a, 0, b, 0, 8, 8, 16, 16, SRCNN_FILTER_BICUBIC, 0, 0, fl, 0)\n"
                   "  + srcnn_y_path_delta_rects(fl, c, r, 64, 64, 16, 16, out, 0, it, 2, &n)\n"
                   "  + srcnn_y_path_delta_f32_dev(a, 0, b, 0, 8, 8, 16, 16, SRCNN_FILTER_BICUBIC, 0, 0, out, 0, 0, &st)\n"
                   "  + (int)st.cell_samples + SRCNN_AMD_DELTA_VERSION; }\n"
                   )
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-c", str(src), "-I" + os.path.join(ROOT, "include"), "-o", str(tmp_path / "use.o")])
    main = tmp_path / "sizes.c"
    main.write_text('#include <stdio.h>\n#include "srcnn_amd_delta.h"\n'
                    'int main(void) { printf("%u %u\\n", (unsigned)sizeof(srcnn_delta_stats), (unsigned)sizeof(srcnn_rect_item)); return 0; }\n')
    exe = str(tmp_path / "sizes")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", str(main), "-I" + os.path.join(ROOT, "include"), "-o", exe])
    sizes = subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split()
    assert [int(v) for v in sizes] == [C.sizeof(S.DeltaStats), C.sizeof(S.RectItem)]


# ---- the grid ----
def test_grid_of_the_issue(S):
    assert S.y_path_delta_grid(96, 56, 192, 112, 2, (32, 16)) == (6, 7)
    assert S.y_path_delta_grid(96, 56, 192, 112, 2, (40, 24)) == (5, 5)          # last tiles partial: 192 = 4 * 40 + 32, 112 = 4 * 24 + 16
    assert S.y_path_delta_grid(37, 23, 74, 46, 2, (16, 16)) == (5, 3)
    assert S.y_path_delta_grid(96, 56, 240, 140, 3, (64, 64)) == (4, 3)
    assert S.y_path_delta_grid(96, 56, 240, 140, 3, (0, 0)) == (4, 3)             # 0 = the default 64
    assert S.y_path_delta_grid(96, 56, 240, 140, 3, (0, 8)) == (4, 18)
    assert S.y_path_delta_grid(3840, 2160, 7680, 4320, 2) == (120, 68)


def test_grid_argument_rules(S):
    g = lambda *a, **kw: _code(S, lambda: S.y_path_delta_grid(*a, **kw))   # noqa: E731
    assert g(0, 56, 192, 112, 2) == E_ARG and g(96, 0, 192, 112, 2) == E_ARG
    assert g(96, 56, 0, 112, 2) == E_SCALE and g(96, 56, 192, 0, 2) == E_SCALE
    assert g(96, 56, 192, 112, -1) == E_ARG and g(96, 56, 192, 112, 5) == E_ARG
    for t in (1, 7, 65536, 1 << 20):
        assert g(96, 56, 192, 112, 2, (t, 16)) == E_ARG and g(96, 56, 192, 112, 2, (16, t)) == E_ARG, t
    assert g(96, 56, 192, 112, 2, (8, 65535)) == 0
    assert g(96, (1 << 20) + 1, 192, 112, 2) == E_UNSUPPORTED and g(96, 56, 1 << 23, 112, 2) == E_UNSUPPORTED
    # the stated limit: 2048 tile columns or rows
    assert g(96, 56, 2048 * 8, 112, 2, (8, 8)) == 0 and g(96, 56, 2048 * 8 + 1, 112, 2, (8, 8)) == E_UNSUPPORTED
    assert g(96, 56, 192, 2048 * 8, 2, (8, 8)) == 0 and g(96, 56, 192, 2048 * 8 + 1, 2, (8, 8)) == E_UNSUPPORTED
    assert "2048" in S.lib().srcnn_last_error().decode()
    c, r = C.c_uint(0), C.c_uint(0)
    assert S.lib().srcnn_y_path_delta_grid(96, 56, 192, 112, 2, 0, 0, None, C.byref(r)) == E_ARG
    assert S.lib().srcnn_y_path_delta_grid(96, 56, 192, 112, 2, 0, 0, C.byref(c), None) == E_ARG


# ---- argument rules of the device calls: host buffers stand in for device planes, which is safe because every call below is
# refused before the device is looked up ----
class Planes:
    """Two 9 x 7 sources, an 18 x 14 output and a flag array, in one host array."""

    def __init__(self, w=9, h=7, dw=18, dh=14, pitch=0, out_pitch=0):
        self.w, self.h, self.dw, self.dh, self.pitch, self.out_pitch = w, h, dw, dh, pitch, out_pitch
        self.in_bytes = max(pitch, 4 * w) * h
        self.out_bytes = max(out_pitch, 4 * dw) * dh
        self.buf = np.zeros((2 * self.in_bytes + self.out_bytes) // 4 + 1024, np.float32)
        self.prev = self.buf.ctypes.data
        self.cur = self.prev + self.in_bytes
        self.out = self.cur + self.in_bytes
        self.flags = self.out + self.out_bytes

    def args(self, kw):
        a = dict(prev=self.prev, prev_pitch=self.pitch, cur=self.cur, cur_pitch=self.pitch, w=self.w, h=self.h, dw=self.dw, dh=self.dh, filt=2,
                 tile=(0, 0), out=self.out, out_pitch=self.out_pitch, flags=self.flags, struct_size=None, stats=True)
        a.update(kw)
        return a

    def delta(self, S, **kw):
        a = self.args(kw)
        return _code(S, lambda: S.y_path_delta_dev(a["prev"], a["prev_pitch"], a["cur"], a["cur_pitch"], a["w"], a["h"], a["dw"], a["dh"], a["filt"],
                                                   a["tile"], a["out"], a["out_pitch"], None, a["stats"], a["struct_size"]))

    def flag(self, S, **kw):
        a = self.args(kw)
        return _code(S, lambda: S.y_path_delta_flags_dev(a["prev"], a["prev_pitch"], a["cur"], a["cur_pitch"], a["w"], a["h"], a["dw"], a["dh"],
                                                         a["filt"], a["tile"], a["flags"]))


def test_argument_rules_of_both_device_calls(S):
    p = Planes()
    for call in (p.delta, p.flag):
        assert call(S, cur=None) == E_ARG
        assert call(S, w=0) == E_ARG and call(S, h=0) == E_ARG
        assert call(S, dw=0) == E_SCALE and call(S, dh=0) == E_SCALE
        for filt in (-1, 5, 100):
            assert call(S, filt=filt) == E_ARG
        assert call(S, tile=(7, 0)) == E_ARG and call(S, tile=(0, 65536)) == E_ARG
        for which in ("prev", "cur"):
            assert call(S, **{which + "_pitch": 4 * p.w - 4}) == E_ARG, which
            assert call(S, **{which + "_pitch": 4 * p.w + 2}) == E_ARG, which
            assert call(S, **{which: getattr(p, which) + 2}) == E_ARG, which
        assert call(S, h=(1 << 20) + 1) == E_UNSUPPORTED and call(S, dw=1 << 23) == E_UNSUPPORTED
        assert call(S, dw=2048 * 8 + 1, tile=(8, 8)) == E_UNSUPPORTED
    assert p.flag(S, flags=None) == E_ARG
    # the output plane of the whole operation: a dw x dh plane under the rect call's rules, clear of both sources
    assert p.delta(S, out=None) == E_ARG
    assert p.delta(S, out_pitch=4 * p.dw - 4) == E_ARG and p.delta(S, out_pitch=4 * p.dw + 2) == E_ARG and p.delta(S, out=p.out + 2) == E_ARG
    assert p.delta(S, out=p.prev) == E_ARG and p.delta(S, out=p.cur) == E_ARG
    assert p.delta(S, out=p.cur + p.in_bytes - 4) == E_ARG and p.delta(S, out=p.prev + p.in_bytes - 4) == E_ARG
    assert "overlaps" in S.lib().srcnn_last_error().decode()
    assert p.delta(S, struct_size=0) == E_ARG and p.delta(S, struct_size=C.sizeof(S.DeltaStats) + 8) == E_ARG
    assert "struct_size" in S.lib().srcnn_last_error().decode()


def test_valid_calls_without_a_device(S):
    if S.device_count() > 0:
        pytest.skip("a device is present: a valid call would run on host memory")
    for p in (Planes(), Planes(pitch=64, out_pitch=128), Planes(50, 30, 37, 20)):
        assert p.delta(S) == E_NODEVICE and p.flag(S) == E_NODEVICE
        assert p.delta(S, stats=False) == E_NODEVICE and p.delta(S, prev=None) == E_NODEVICE and p.flag(S, prev=None) == E_NODEVICE
    q = Planes()
    assert q.delta(S, prev=q.cur) == E_NODEVICE          # the two sources may be one plane


# ---- the coalescer ----
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


def check_cover(rects, flags, tile, dw, dh):
    """Pairwise disjoint, union exactly the dirty tiles clipped to dw x dh, no clean tile covered."""
    tw, th = tile
    rows, cols = flags.shape
    paint = np.zeros((dh, dw), np.int32)
    for (x0, y0, rw, rh) in rects:
        assert rw > 0 and rh > 0 and x0 + rw <= dw and y0 + rh <= dh, (x0, y0, rw, rh)
        assert x0 % tw == 0 and y0 % th == 0 and ((x0 + rw) % tw == 0 or x0 + rw == dw) and ((y0 + rh) % th == 0 or y0 + rh == dh)
        paint[y0:y0 + rh, x0:x0 + rw] += 1
    want = np.kron((flags != 0).astype(np.int32), np.ones((th, tw), np.int32))[:dh, :dw]
    assert np.array_equal(paint, want)


def run_coalescer(S, flags, tile, dw, dh):
    flags = np.asarray(flags, np.uint8)
    got = S.y_path_delta_rects(flags, tile, dw, dh)
    rects = [g[:4] for g in got]
    assert rects == coalesce(flags, tile, dw, dh)
    assert S.y_path_delta_rects(flags, tile, dw, dh, cap=0) == len(rects)
    check_cover(rects, flags, tile, dw, dh)
    return rects


def test_coalescer_hand_cases(S):
    tile, dw, dh = (32, 16), 192, 112                    # 6 x 7
    z = np.zeros((7, 6), np.uint8)
    assert run_coalescer(S, z, tile, dw, dh) == []                                                   # empty
    assert run_coalescer(S, z + 1, tile, dw, dh) == [(0, 0, 192, 112)]                               # full
    assert run_coalescer(S, z + 0x80, tile, dw, dh) == [(0, 0, 192, 112)]                            # (any non-zero byte is dirty)
    one = z.copy(); one[3, 2] = 1
    assert run_coalescer(S, one, tile, dw, dh) == [(64, 48, 32, 16)]
    ell = z.copy(); ell[1:5, 1] = 1; ell[4, 1:4] = 1                                                 # an L: the foot is a run of its own
    assert run_coalescer(S, ell, tile, dw, dh) == [(32, 16, 32, 48), (32, 64, 96, 16)]
    chk = np.indices((7, 6)).sum(0) % 2
    assert len(run_coalescer(S, chk, tile, dw, dh)) == 21                                            # a checkerboard: every tile alone
    two = z.copy(); two[2, 0:2] = 1; two[2, 3:6] = 1; two[3, 0:2] = 1; two[3, 3:5] = 1               # two runs; the first continues
    assert run_coalescer(S, two, tile, dw, dh) == [(0, 32, 64, 32), (96, 32, 96, 16), (96, 48, 64, 16)]
    gap = z.copy(); gap[0, 1:3] = 1; gap[2, 1:3] = 1                                                 # the same run after a clean row: a new rect
    assert run_coalescer(S, gap, tile, dw, dh) == [(32, 0, 64, 16), (32, 32, 64, 16)]
    # partial last tiles are clipped: 40 x 24 tiles over 192 x 112
    full = np.ones((5, 5), np.uint8)
    assert run_coalescer(S, full, (40, 24), dw, dh) == [(0, 0, 192, 112)]
    edge = np.zeros((5, 5), np.uint8); edge[4, 4] = 1
    assert run_coalescer(S, edge, (40, 24), dw, dh) == [(160, 96, 32, 16)]
    # degenerate grids
    assert run_coalescer(S, [[1]], (64, 64), 20, 9) == [(0, 0, 20, 9)]
    assert run_coalescer(S, [[1], [0], [1], [1]], (64, 8), 10, 30) == [(0, 0, 10, 8), (0, 16, 10, 14)]


@pytest.mark.parametrize("seed", range(6))
def test_coalescer_seeded_grids(S, seed):
    rng = np.random.default_rng(7100 + seed)
    for tile, dw, dh in (((32, 16), 192, 112), ((40, 24), 192, 112), ((16, 16), 74, 46), ((64, 64), 240, 140), ((8, 8), 333, 95)):
        cols, rows = -(-dw // tile[0]), -(-dh // tile[1])
        for density in (0.1, 0.5, 0.9):
            run_coalescer(S, rng.random((rows, cols)) < density, tile, dw, dh)


def test_coalescer_items_and_argument_rules(S):
    flags = np.zeros((7, 6), np.uint8); flags[2:5, 2:4] = 1; flags[6, 5] = 1
    base = 0x10000
    got = S.y_path_delta_rects(flags, (32, 16), 192, 112, out=base, out_pitch=1024)
    assert got == [(64, 32, 64, 48, base + 32 * 1024 + 4 * 64, 1024), (160, 96, 32, 16, base + 96 * 1024 + 4 * 160, 1024)]
    tight = S.y_path_delta_rects(flags, (32, 16), 192, 112, out=base)
    assert [t[4:] for t in tight] == [(base + 32 * 768 + 4 * 64, 768), (base + 96 * 768 + 4 * 160, 768)]
    assert [t[4] for t in S.y_path_delta_rects(flags, (32, 16), 192, 112)] == [None, None]
    L, n = S.lib(), C.c_uint(99)
    f = flags.ctypes.data
    items = (S.RectItem * 2)()
    assert L.srcnn_y_path_delta_rects(f, 6, 7, 32, 16, 192, 112, None, 0, C.cast(items, C.c_void_p), 1, C.byref(n)) == E_ARG and n.value == 2   # cap one short
    assert L.srcnn_y_path_delta_rects(f, 6, 7, 32, 16, 192, 112, None, 0, C.cast(items, C.c_void_p), 2, C.byref(n)) == 0 and n.value == 2
    assert L.srcnn_y_path_delta_rects(f, 6, 7, 32, 16, 192, 112, None, 0, None, 2, C.byref(n)) == E_ARG
    assert L.srcnn_y_path_delta_rects(f, 6, 7, 32, 16, 192, 112, None, 0, None, 0, None) == E_ARG
    assert L.srcnn_y_path_delta_rects(None, 6, 7, 32, 16, 192, 112, None, 0, None, 0, C.byref(n)) == E_ARG
    assert L.srcnn_y_path_delta_rects(f, 5, 7, 32, 16, 192, 112, None, 0, None, 0, C.byref(n)) == E_ARG          # not the grid of 192 x 112
    assert L.srcnn_y_path_delta_rects(f, 6, 7, 0, 16, 192, 112, None, 0, None, 0, C.byref(n)) == E_ARG           # the tile is given here
    assert L.srcnn_y_path_delta_rects(f, 6, 7, 32, 16, 0, 112, None, 0, None, 0, C.byref(n)) == E_SCALE
    assert L.srcnn_y_path_delta_rects(f, 6, 7, 32, 16, 192, 112, base, 764, None, 0, C.byref(n)) == E_ARG        # pitch below the row
    assert L.srcnn_y_path_delta_rects(f, 6, 7, 32, 16, 192, 112, base + 2, 0, None, 0, C.byref(n)) == E_ARG


# ---- the whole-frame rule and its switch ----
def test_whole_frame_rule_and_settings_row(S):
    text = S.debug_settings()
    assert "SRCNN_DELTA_WHOLE_PERMILLE=" in text
    row = [ln for ln in S.debug_settings(markdown=True).splitlines() if "SRCNN_DELTA_WHOLE_PERMILLE" in ln]
    assert len(row) == 1
    default = int(re.search(r"\*\*(\d+)\*\*", row[0]).group(1))
    assert 500 <= default <= 1000                                       # 1000 until measured; the measured crossover, never below 500
    assert row[0] in open(os.path.join(ROOT, "DESIGN.md")).read()
    settings = open(os.path.join(ROOT, "libsrcnn_amd", "csrc", "srcnn_settings.hpp")).read()
    assert re.search(r'X\(I,\s*delta_whole_permille,\s*"SRCNN_DELTA_WHOLE_PERMILLE",\s*%d,' % default, settings)
    # the rule itself is host code: tests/host/delta_sanitize.cpp drives delta_whole_frame with every clause; here, that the
    # switch reaches a process that sets it
    r = subprocess.run([sys.executable, "-c", "import libsrcnn_amd as S; print(S.debug_settings())"], env=dict(os.environ, SRCNN_DELTA_WHOLE_PERMILLE="650"),
                       cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "SRCNN_DELTA_WHOLE_PERMILLE=650" in r.stdout, r.stdout[-500:] + r.stderr[-1500:]
