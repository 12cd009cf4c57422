"""CPU: the rect extension (include/srcnn_amd_rect.h) -- its declared functions, committed list, binding and export table agree
(full and strict-only builds), the header is C99, srcnn_y_path_rect_source matches a restatement built on the oracle's
contribution tables, every argument rule of srcnn_y_path_rect_f32_dev returns its code before any device lookup (host buffers
stand in for device planes), and the layer kernels' fingerprints are the ones the traffic records were taken with."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from test_abi import HANDLE_ONLY_HOOKS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_ARG, E_SCALE, E_NODEVICE, E_UNSUPPORTED = -1, -2, -200, -203
OLDER = ("srcnn_amd.h", "srcnn_amd_debug.h", "srcnn_amd_yuv.h", "srcnn_amd_yuv_ex.h", "srcnn_amd_yuv_packed.h", "srcnn_amd_rgb.h",
         "libsrcnn_dropin.h")


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
    names = _declared("srcnn_amd_rect.h")
    listed = [ln.strip() for ln in open(os.path.join(ROOT, "include", "srcnn_amd_rect.abi")) if ln.strip() and not ln.startswith("#")]
    assert listed == sorted(listed) and len(set(listed)) == len(listed)
    assert names == listed == sorted(S.RECT_SYMBOLS)
    assert set(S.RECT_SYMBOLS) <= set(S.C_ABI_SYMBOLS)
    header = open(os.path.join(ROOT, "include", "srcnn_amd_rect.h")).read()
    assert "#define SRCNN_AMD_RECT_VERSION 1" in header and '#include "srcnn_amd.h"' in header
    exported = _exported(S.LIB_PATH)
    assert set(names) <= set(exported)
    assert exported == sorted(S.C_ABI_SYMBOLS + S.CXX_SYMBOLS + HANDLE_ONLY_HOOKS)
    assert S.lib().srcnn_rect_abi_version() == 1


def test_no_older_header_mentions_the_new_names():
    names = _declared("srcnn_amd_rect.h")
    assert len(names) == 3
    for other in OLDER:
        text = open(os.path.join(ROOT, "include", other)).read()
        assert not set(names) & set(_declared(other)), other
        assert not any(n in text for n in names) and "srcnn_amd_rect" not in text.lower(), other


def test_strict_only_build_exports_the_same_set(S):
    from libsrcnn_amd import build
    strict, _ = build.build_strict_only(verbose=False)
    assert _exported(strict) == _exported(S.LIB_PATH)
    assert set(S.RECT_SYMBOLS) <= set(_exported(strict))


def test_header_compiles_as_c99(tmp_path):
    src = tmp_path / "use.c"
    src.write_text('#include "srcnn_amd_rect.h"\n'
                   "int f(const float* in, float* out) { unsigned a, b, c, d;\n"
                   "  return srcnn_rect_abi_version() + srcnn_y_path_rect_source(8, 8, 16, 16, SRCNN_FILTER_BICUBIC, 1, 2, 3, 4, &a, &b, &c, &d)\n"
                   "  + srcnn_y_path_rect_f32_dev(in, 0, 8, 8, 16, 16, SRCNN_FILTER_BICUBIC, 1, 2, 3, 4, out, 64, 0)\n"
                   "  + SRCNN_AMD_RECT_VERSION; }\n")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-c", str(src), "-I" + os.path.join(ROOT, "include"),
                           "-o", str(tmp_path / "use.o")])


# ---- srcnn_y_path_rect_source ----
SHAPES = [(70, 40, 140, 80), (40, 31, 60, 46), (50, 30, 37, 20), (33, 20, 66, 15), (24, 24, 24, 24), (1, 17, 2, 34)]


def edges(n):
    """Rect edges of one axis: at and near both borders, around the halo (6) and the tile sizes, and in the middle."""
    e = {0, 1, 2, 5, 6, 7, 8, 15, 16, 17, 63, 64, 65, n - 8, n - 7, n - 6, n - 5, n - 2, n - 1, n, n // 2}
    return sorted(v for v in e if 0 <= v <= n)


def axis_span(tables, filt, dst, src, a, b):
    """The restatement of one axis: +-2 (layer 3) and +-4 (layer 1) cut at the borders, then the first and the last tap of
    that range; an axis that keeps its size is copied."""
    ca, cb = max(0, a - 2), min(dst, b + 2)
    ua, ub = max(0, ca - 4), min(dst, cb + 4)
    if dst == src:
        return ua, ub - ua
    left, right = tables(filt, dst, src)
    lo, hi = int(left[ua:ub].min()), int(right[ua:ub].max()) + 1
    return lo, hi - lo


@pytest.mark.parametrize("filt", range(5))
def test_source_rect_matches_the_restatement(S, oracle_lib, filt):
    cache = {}

    def tables(f, dst, src):
        if (f, dst, src) not in cache:
            cache[(f, dst, src)] = oracle_lib.axis_table(dst, src, f)[:2]
        return cache[(f, dst, src)]
    rng = np.random.default_rng(1234 + filt)
    n = 0
    for (w, h, dw, dh) in SHAPES:
        ex, ey = edges(dw), edges(dh)
        xs = [(a, b) for a in ex for b in ex if a < b]
        ys = [(a, b) for a in ey for b in ey if a < b]
        rects = [(x, ys[rng.integers(len(ys))]) for x in xs] + [(xs[rng.integers(len(xs))], y) for y in ys]
        rects += [((0, dw), (0, dh)), ((dw // 2, dw // 2 + 1), (dh // 2, dh // 2 + 1))]      # every border, and none (1 x 1 inside)
        for (x0, x1), (y0, y1) in rects:
            sx0, sw = axis_span(tables, filt, dw, w, x0, x1)
            sy0, sh = axis_span(tables, filt, dh, h, y0, y1)
            got = S.y_path_rect_source(w, h, dw, dh, filt, x0, y0, x1 - x0, y1 - y0)
            assert got == (sx0, sy0, sw, sh), ((w, h, dw, dh), filt, (x0, x1, y0, y1), got, (sx0, sy0, sw, sh))
            assert sx0 + sw <= w and sy0 + sh <= h and sw > 0 and sh > 0
            n += 1
    assert n > 300


def test_source_rect_errors_and_null_results(S):
    L = S.lib()
    u = [C.c_uint() for _ in range(4)]
    call = lambda *a: L.srcnn_y_path_rect_source(*a, *[C.byref(v) for v in u])   # noqa: E731
    assert call(8, 8, 16, 16, 2, 1, 2, 3, 4) == 0
    assert L.srcnn_y_path_rect_source(8, 8, 16, 16, 2, 1, 2, 3, 4, None, None, None, None) == 0
    assert call(0, 8, 16, 16, 2, 0, 0, 1, 1) == E_ARG and call(8, 0, 16, 16, 2, 0, 0, 1, 1) == E_ARG
    assert call(8, 8, 16, 16, 2, 0, 0, 0, 1) == E_ARG and call(8, 8, 16, 16, 2, 0, 0, 1, 0) == E_ARG
    assert call(8, 8, 0, 16, 2, 0, 0, 1, 1) == E_SCALE and call(8, 8, 16, 0, 2, 0, 0, 1, 1) == E_SCALE
    assert call(8, 8, 16, 16, 5, 0, 0, 1, 1) == E_ARG and call(8, 8, 16, 16, -1, 0, 0, 1, 1) == E_ARG
    assert call(8, 8, 16, 16, 2, 14, 0, 3, 1) == E_ARG and call(8, 8, 16, 16, 2, 0, 16, 1, 1) == E_ARG
    assert call(8, 8, 16, 16, 2, 0xffffffff, 0, 2, 1) == E_ARG
    assert call(8, (1 << 20) + 1, 16, 16, 2, 0, 0, 1, 1) == E_UNSUPPORTED


# ---- argument rules: host buffers stand in for device planes, which is safe because every call below is refused before the
# device is looked up ----
class Planes:
    def __init__(self, w=9, h=7, dw=18, dh=14, in_pitch=0, out_pitch=0, rect=(3, 2, 8, 6)):
        self.w, self.h, self.dw, self.dh, self.rect = w, h, dw, dh, rect
        self.in_pitch, self.out_pitch = in_pitch, out_pitch
        self.in_bytes = max(in_pitch, 4 * w) * h
        self.out_bytes = max(out_pitch, 4 * rect[2]) * rect[3]
        self.buf = np.zeros((self.in_bytes + self.out_bytes) // 4 + 64, np.float32)
        self.src = self.buf.ctypes.data
        self.dst = self.src + self.in_bytes

    def call(self, S, **kw):
        a = dict(src=self.src, in_pitch=self.in_pitch, w=self.w, h=self.h, dw=self.dw, dh=self.dh, filt=2, x0=self.rect[0],
                 y0=self.rect[1], rw=self.rect[2], rh=self.rect[3], dst=self.dst, out_pitch=self.out_pitch)
        a.update(kw)
        try:
            S.y_path_rect_dev(a["src"], a["in_pitch"], a["w"], a["h"], a["dw"], a["dh"], a["filt"], a["x0"], a["y0"], a["rw"], a["rh"],
                              a["dst"], a["out_pitch"])
        except S.SrcnnError as e:
            return e.code
        return 0


def test_null_zero_scale_filter_and_rect_rules(S):
    p = Planes()
    assert p.call(S, src=None) == E_ARG and p.call(S, dst=None) == E_ARG
    for k in ("w", "h", "rw", "rh"):
        assert p.call(S, **{k: 0}) == E_ARG, k
    assert p.call(S, dw=0) == E_SCALE and p.call(S, dh=0) == E_SCALE
    for filt in (-1, 5, 100):
        assert p.call(S, filt=filt) == E_ARG
    assert p.call(S, x0=11) == E_ARG                      # 11 + 8 > 18
    assert p.call(S, y0=9) == E_ARG                       # 9 + 6 > 14
    assert p.call(S, x0=18, rw=1) == E_ARG and p.call(S, y0=14, rh=1) == E_ARG
    assert p.call(S, x0=0xfffffffe, rw=4) == E_ARG        # the sum wraps in 32 bits
    assert p.call(S, rw=19, x0=0) == E_ARG and p.call(S, rh=15, y0=0) == E_ARG


def test_pitch_and_alignment_rules(S):
    p = Planes(in_pitch=64, out_pitch=64)
    assert p.call(S, in_pitch=4 * p.w - 4) == E_ARG and p.call(S, out_pitch=4 * p.rect[2] - 4) == E_ARG
    for bad in (65, 66, 67):
        assert p.call(S, in_pitch=bad) == E_ARG and p.call(S, out_pitch=bad) == E_ARG
    for off in (1, 2, 3):
        assert p.call(S, src=p.src + off) == E_ARG and p.call(S, dst=p.dst + off) == E_ARG


def test_size_limits(S):
    p = Planes()
    assert p.call(S, h=(1 << 20) + 1) == E_UNSUPPORTED
    assert p.call(S, dh=(1 << 20) + 1) == E_UNSUPPORTED
    assert p.call(S, dw=1 << 23) == E_UNSUPPORTED
    assert p.call(S, w=60000, h=60000, in_pitch=0) == E_UNSUPPORTED


def test_overlapping_input_and_output(S):
    p = Planes(in_pitch=64, out_pitch=64)
    assert p.call(S, dst=p.src) == E_ARG                                   # same start
    assert p.call(S, dst=p.src + p.in_bytes - 64 + 4 * p.w - 4) == E_ARG   # starts on the input's last sample
    assert p.call(S, dst=p.src - 64 * (p.rect[3] - 1) - 4 * p.rect[2] + 4) == E_ARG    # ends on the input's first sample
    assert p.call(S, src=p.dst + 4) == E_ARG


def test_valid_calls_without_a_device(S):
    if S.device_count() > 0:
        pytest.skip("a device is present: a valid call would run on host memory")
    assert Planes().call(S) == E_NODEVICE
    assert Planes(in_pitch=64, out_pitch=128).call(S) == E_NODEVICE
    p = Planes(in_pitch=64, out_pitch=64)
    assert p.call(S, dst=p.src + p.in_bytes - 64 + 4 * p.w) == E_NODEVICE          # starts right after the input's last sample
    for (w, h, dw, dh) in SHAPES:
        assert Planes(w, h, dw, dh, rect=(0, 0, dw, dh)).call(S) == E_NODEVICE
        assert Planes(w, h, dw, dh, rect=(dw - 1, dh - 1, 1, 1)).call(S) == E_NODEVICE


def test_layer_kernel_fingerprints_are_the_parents():
    """The rect call reuses the layer kernels and their launchers untouched: their fingerprints (build.kernel_source_sha) are
    the recorded ones, so bench.py keeps quoting roofline.traffic.  k_rs2d_dma's is the value of the commit before the rect
    call; k_conv12_mfma's moved once since, on purpose, when the nested-tiers kernel was folded into it instruction for
    instruction (profiles/conv12_fold_isa.txt), and k_conv3's moved once, on purpose, when the written-out copy of its skip instance was folded into
    it in the same way (profiles/conv3_fold_isa.txt); each time the traffic record was re-measured."""
    from libsrcnn_amd import build
    assert build.kernel_source_sha("k_conv12_mfma") == "94857eddbb2a8296a76ec6a18246f0288de6590de38bfd8a5f647015ee1ee39a"
    assert build.kernel_source_sha("k_conv3") == "4d4511830f635b4324fe30ab3cc2c5f8861b2dac0d85fb0c7ac48db46b7fa46d"
    assert build.kernel_source_sha("k_rs2d_dma") == "adef7f27470d21d8aa7396a314ed8a758b2707fa87b705cbb289ae66fd085030"
