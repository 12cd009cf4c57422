"""srcnn_rgb_upscale_rect_dev (include/srcnn_amd_rgb_rect.h) byte for byte against crops of the whole image (GPU).

A rect is a crop of what srcnn_rgb_upscale_dev writes, so every expectation is a crop of the whole-image expectation of
tests/test_gpu_rgb.py -- oracle.process at depth 8, the numpy restatement of tests/test_rgb_restatement.py above it -- computed
once per image, and, where the contract names it, a crop of the library's own whole-image call.  Never the call under test.
Rect edges sit at and next to both borders, around the 6-sample halo and the 16 / 64 tile sizes; small shapes throughout; the
positions the edge rule leaves open rotate with the session seed.  Every process these tests start runs under a timeout of
its own and nothing is tried twice.
"""
import json
import os
import subprocess
import sys
import threading

import numpy as np
import pytest

from conftest import assert_bit_equal, rotating_seed
from test_gpu_rect import edge_rects
from test_gpu_rgb import arrange, canonical, first_difference, layout_bases, run
from test_gpu_yuv import FILTER_NAMES, FILTERS, out_size
from test_rgb_restatement import CELLS, DEPTHS, LAYOUTS, ORDERS, cases_for, dtype_of, image, restatement, seed_of, want_for

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORKER = os.path.join(ROOT, "tests", "rgb_rect_worker.py")
CANARY = 0xA5
F = np.float32


def seed():
    return rotating_seed("rect positions of tests/test_gpu_rgb_rect.py")


def crop(pair, rect):
    x0, y0, rw, rh = rect
    return pair[0][y0:y0 + rh, x0:x0 + rw], pair[1][y0:y0 + rh, x0:x0 + rw]


def assert_rect(got, want, what):
    for name, g, e in zip(("out", "conv"), got, want):
        assert g.shape == e.shape and g.dtype == e.dtype, (what, name, g.shape, e.shape, g.dtype, e.dtype)
        assert np.array_equal(g, e), "%s %s: %s" % (what, name, first_difference(g, e))


def whole_want(oracle_lib, img, depth, mul, filt):
    return oracle_lib.process(img, mul, filt) if depth == 8 else restatement(oracle_lib, img, depth, mul, filt)


class Rig:
    """One source image in device memory (tight) in a format, and result buffers; rect() runs one call and returns (out, conv)
    in R, G, B[, A] order."""

    def __init__(self, S, img, layout, order, depth, mul, filt):
        self.S, self.layout, self.order, self.depth, self.mul, self.filt = S, layout, order, depth, mul, filt
        self.h, self.w, self.c = img.shape
        self.planar = layout == "planar"
        self.dt = dtype_of(depth)
        self.bps = np.dtype(self.dt).itemsize
        self.dw, self.dh = out_size(self.w, self.h, mul)
        self.fmt = S.rgb_format(layout, order, self.c == 4, depth)
        self.din = S.DeviceBuffer.from_numpy(arrange(img, layout, order))
        self.dout = S.DeviceBuffer(max(1, self.dw * self.dh * self.c * self.bps))
        self.dconv = S.DeviceBuffer(max(1, self.dw * self.dh * self.bps))
        self.src = [(self.din, k * self.w * self.h * self.bps) for k in range(self.c)] if self.planar else [self.din]

    def rect(self, x0, y0, rw, rh, stream=None):
        S = self.S
        dst = [(self.dout, k * rw * rh * self.bps) for k in range(self.c)] if self.planar else [self.dout]
        S.rgb_upscale_rect_dev(self.fmt, self.w, self.h, self.mul, self.filt, self.src, None, x0, y0, rw, rh, dst, None, self.dconv, 0, stream)
        S.sync()
        out = self.dout.to_numpy(self.dt, (self.c, rh, rw) if self.planar else (rh, rw, self.c))
        return canonical(out, self.layout, self.order), self.dconv.to_numpy(self.dt, (rh, rw))

    def check(self, want, rects, what):
        for r in rects:
            assert_rect(self.rect(*r), crop(want, r), "%s rect %dx%d at (%d,%d)" % ((what,) + (r[2], r[3], r[0], r[1])))


# ---- edges: 70 x 40 -> 140 x 80, 2x bicubic ----
def edge_case_rects(rng):
    rects = edge_rects(140, 80, rng)
    rects += [(77, 41, 1, 1), (0, 0, 140, 80)]
    rects += [(7, 9, ww - 12, 30) for ww in (63, 64, 65, 127, 128, 129)]      # windows of 63 ... 129 columns: rect + 6 on both sides
    return rects


@pytest.mark.parametrize("layout,order,alpha,depth", [("interleaved", "rgb", 0, 8), ("planar", "bgr", 1, 12)], ids=["rgb8", "planar-bgra12"])
def test_edges_vs_oracle_and_whole_image(srcnn, oracle_lib, layout, order, alpha, depth):
    img = image(70, 40, alpha, depth, 7040 + depth)
    want = whole_want(oracle_lib, img, depth, 2.0, 2)
    whole = run(srcnn, img, layout, order, depth, 2.0, 2)
    assert_rect(whole, want, "whole image vs oracle")
    rig = Rig(srcnn, img, layout, order, depth, 2.0, 2)
    rects = edge_case_rects(np.random.default_rng(seed()))
    assert len(rects) >= 380
    for r in rects:
        got = rig.rect(*r)
        what = "rect %dx%d at (%d,%d)" % (r[2], r[3], r[0], r[1])
        assert_rect(got, crop(want, r), what + " vs oracle")
        assert_rect(got, crop(whole, r), what + " vs the library's whole image")


# ---- the matrix: one case per format cell, rotating through the cell's cases ----
def matrix_case(cell):
    cases = list(cases_for(*cell))
    return cases[(5 * CELLS.index(cell) + 2) % len(cases)]


MATRIX = [(cell, matrix_case(cell)) for cell in CELLS]
assert len(MATRIX) == 40 and {c[1][2] for c in MATRIX} == set(FILTERS)
_SHAPES = [(w, h) + out_size(w, h, m) for (_cell, (w, h, _f, m)) in MATRIX]
assert any(dw > w and dh > h for (w, h, dw, dh) in _SHAPES), "no up-scale in both axes"
assert any(dw < w and dh < h for (w, h, dw, dh) in _SHAPES), "no down-scale"
assert any((dw == w) != (dh == h) for (w, h, dw, dh) in _SHAPES), "no case with one axis kept and the other resampled"
assert {m for (_cell, (_w, _h, _f, m)) in MATRIX} >= {0.75, 1.5, 2.0, 2.5, 3.0}


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("alpha", [0, 1], ids=["rgb", "rgba"])
@pytest.mark.parametrize("depth", DEPTHS)
def test_matrix_vs_oracle(srcnn, oracle_lib, layout, order, alpha, depth):
    cell = (layout, order, alpha, depth)
    case = matrix_case(cell)
    w, h, filt, mul = case
    dw, dh = out_size(w, h, mul)
    rng = np.random.default_rng(seed() + CELLS.index(cell))
    rects = edge_rects(dw, dh, rng, limit=8) + [(0, 0, dw, dh), (dw - 1, dh - 1, 1, 1), (dw // 2, dh // 2, 1, 1), (0, dh - 1, dw, 1), (dw - 1, 0, 1, dh)]
    assert len(rects) >= 12, (cell, case, len(rects))
    img = image(w, h, alpha, depth, seed_of(w, h))
    Rig(srcnn, img, layout, order, depth, mul, filt).check(want_for(oracle_lib, alpha, depth, case), rects,
                                                           "%s %s alpha=%d %d-bit %dx%d %s x%g" % (layout, order, alpha, depth, w, h, FILTER_NAMES[filt], mul))


# ---- the identity size: crops of srcnn_process_u8 (the library's pinned deviation from the reference) ----
@pytest.mark.parametrize("alpha", [0, 1], ids=["rgb", "rgba"])
def test_identity_size_gives_crops_of_process_u8(srcnn, alpha):
    S = srcnn
    rng = np.random.default_rng(seed() + 31)
    for k, (w, h) in enumerate(((23, 17), (64, 40), (9, 7), (1, 5), (130, 66))):
        filt = FILTERS[k % 5]
        img = image(w, h, alpha, 8, 3 * w + h)
        want = S.process_u8(img, 1.0, filt, want_conv=True)
        rects = edge_rects(w, h, rng, limit=3) + [(0, 0, w, h), (w - 1, h - 1, 1, 1), (w // 2, h // 2, 1, 1)]
        for layout in LAYOUTS:
            for order in ORDERS:
                Rig(S, img, layout, order, 8, 1.0, filt).check(want, rects, "identity %s %s %dx%d f%d" % (layout, order, w, h, filt))


# ---- both routes: k_rgb_window_merge and the plane route over the window give the same bytes ----
def child(mode, env=None, timeout=600):
    r = subprocess.run([sys.executable, WORKER, mode], env=dict(os.environ, **(env or {})), capture_output=True, text=True, timeout=timeout)
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")]
    assert r.returncode == 0 and line, "rgb_rect_worker %s: exit %d\n%s\n%s" % (mode, r.returncode, r.stdout[-600:], r.stderr[-1500:])
    return json.loads(line[0][7:])


def test_forced_plane_route_gives_the_same_bytes(srcnn, oracle_lib):
    """SRCNN_RGB_RECT_UNFUSED=1 (read when the library loads) sends up-scales down the plane route as well; here the default
    route's bytes are first held to the oracle, and one rect is one launch of the layer-1+2 kernel."""
    S = srcnn
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import rgb_rect_worker as W
    assert "SRCNN_RGB_RECT_UNFUSED=0" in S.debug_settings()
    cases = W.route_cases()
    assert len({(c[2], c[3], c[4]) for c in cases}) == 4 and all(out_size(c[1].shape[1], c[1].shape[0], c[5])[0] > c[1].shape[1] for c in cases)
    fast = W.run_routes(S)
    for (name, img, layout, order, depth, mul, filt, rects) in cases:
        want = whole_want(oracle_lib, img, depth, mul, filt)
        parts = []
        for r in rects:
            o, c = crop(want, r)
            parts += [arrange(o, layout, order), c]
        assert fast[name] == W.digest(*parts), "default route vs oracle: " + name
    S.profile_enable(True)
    try:
        S.profile_reset()
        name, img, layout, order, depth, mul, filt, rects = cases[0]
        S.rgb_upscale_rect(arrange(img, layout, order), rects[1], multiply=mul, filt=filt, layout=layout, order=order, depth=depth)
        assert S.profile_read()["conv12"][1] == 1
    finally:
        S.profile_enable(False)
    assert child("unfused", env={"SRCNN_RGB_RECT_UNFUSED": "1"}) == fast


# ---- pitches and guards: everything in one device buffer filled with a canary ----
PITCH_CASES = [(9, 7, 2, 2.0, "rgb", 0, 8), (23, 17, 3, 1.5, "bgr", 1, 8), (30, 11, 0, 2.5, "bgr", 0, 16), (33, 20, 4, 0.75, "rgb", 1, 10)]
_PITCH_WANT = {}


def pitch_rects(dw, dh):
    """Odd and even origins, widths 1, 3, 4, 5 and wider, the right and bottom borders."""
    rects = [(1, 1, 1, 1), (3, 2, 3, 2), (2, 1, 4, 3), (5, 0, 5, dh), (1, 3, dw - 1, dh - 3), (0, 0, dw, dh), (dw - 4, dh - 1, 4, 1)]
    return [r for r in rects if r[0] + r[2] <= dw and r[1] + r[3] <= dh and r[2] > 0 and r[3] > 0]


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("offset,pad", [(1, 1), (3, 7), (2, 2), (6, 14), (2, 64), (0, 0), (0, 16)])
@pytest.mark.parametrize("w,h,filt,mul,order,alpha,depth", PITCH_CASES)
def test_pitched_misaligned_and_in_place_vs_oracle(srcnn, oracle_lib, layout, offset, pad, w, h, filt, mul, order, alpha, depth):
    """Two destinations per rect: the rect's own planes at odd base offsets with padded rows, and the address of pixel (x0, y0)
    inside a full-size canary image with that image's pitch.  The rect's bytes are the oracle's, every other byte -- padding
    of the planes and of dst_conv, the rest of the full-size image, the guards -- is still the canary."""
    S = srcnn
    if depth > 8 and (offset % 2 or pad % 2):
        offset, pad = offset + 1, pad + 1                 # 16-bit planes: even addresses and pitches (still not dword aligned)
    key = (w, h, filt, mul, alpha, depth)
    if key not in _PITCH_WANT:
        _PITCH_WANT[key] = whole_want(oracle_lib, image(w, h, alpha, depth, 7 * w + h), depth, mul, filt)
    img, want = image(w, h, alpha, depth, 7 * w + h), _PITCH_WANT[key]
    dw, dh = out_size(w, h, mul)
    c, bps = 3 + alpha, (1 if depth == 8 else 2)
    as_rows = lambda a: [np.ascontiguousarray(p).reshape(p.shape[0], -1).view(np.uint8) for p in (a if layout == "planar" else [a])]   # noqa: E731
    src_planes = as_rows(arrange(img, layout, order))
    n = len(src_planes)
    spp = 1 if layout == "planar" else c
    fmt = S.rgb_format(layout, order, alpha, depth)
    for (x0, y0, rw, rh) in pitch_rects(dw, dh):
        o, cv = crop(want, (x0, y0, rw, rh))
        out_planes = as_rows(arrange(o, layout, order)) + [np.ascontiguousarray(cv).view(np.uint8)]
        for in_place in (False, True):
            # destination planes: the rect's own rows, or the rows of a full-size image in which the rect sits at (x0, y0)
            prow = [(dw if in_place else rw) * bps * (spp if k < n else 1) for k in range(n + 1)]
            rows = [p.shape[0] for p in src_planes] + [dh if in_place else rh] * (n + 1)
            widths = [p.shape[1] for p in src_planes] + prow
            pitches = [wd + (pad + 16 * k if pad % 16 == 0 else pad + 4 * k) if pad else wd for k, wd in enumerate(widths)]
            bases, total = layout_bases(rows, pitches, offset)
            host = np.full(total, CANARY, np.uint8)
            for p, b, pt in zip(src_planes, bases, pitches):
                for r in range(p.shape[0]):
                    host[b + r * pt: b + r * pt + p.shape[1]] = p[r]
            first = [b + ((y0 * pt + x0 * bps * (spp if k < n else 1)) if in_place else 0)
                     for k, (b, pt) in enumerate(zip(bases[n:], pitches[n:]))]           # the byte of pixel (x0, y0) of every plane
            buf = S.DeviceBuffer.from_numpy(host)
            S.rgb_upscale_rect_dev(fmt, w, h, mul, filt, [(buf, b) for b in bases[:n]], pitches[:n], x0, y0, rw, rh,
                                   [(buf, a) for a in first[:n]], pitches[n:2 * n], (buf, first[n]), pitches[2 * n])
            S.sync()
            back = buf.to_numpy(np.uint8, (total,))
            expect = host.copy()
            for p, a, pt in zip(out_planes, first, pitches[n:]):
                for r in range(p.shape[0]):
                    expect[a + r * pt: a + r * pt + p.shape[1]] = p[r]
            if not np.array_equal(back, expect):
                bad = np.flatnonzero(back != expect)
                where = ["plane %d" % k for k, b in enumerate(bases) if b <= bad[0] < b + pitches[k] * rows[k]] or ["guard"]
                raise AssertionError("rect %r %s: %d bytes differ, first at byte %d (%s): got %d want %d" %
                                     ((x0, y0, rw, rh), "in a full-size image" if in_place else "own planes", len(bad), bad[0], where[0],
                                      back[bad[0]], expect[bad[0]]))


def test_no_conv_plane_and_tight_defaults(srcnn, oracle_lib):
    S = srcnn
    img = image(23, 17, 1, 8, 5)
    want, _ = oracle_lib.process(img, 2.0, 2)
    for layout in LAYOUTS:
        out, conv = S.rgb_upscale_rect(arrange(img, layout, "rgb"), (3, 5, 40, 20), multiply=2.0, filt=2, layout=layout, want_conv=False)
        assert conv is None and np.array_equal(canonical(out, layout, "rgb"), want[5:25, 3:43]), layout


# ---- source locality ----
@pytest.mark.parametrize("w,h,mul,filt,layout,order,alpha,depth", [(70, 40, 2.0, 2, "interleaved", "rgb", 0, 8),
                                                                   (40, 31, 1.5, 3, "planar", "bgr", 1, 12),
                                                                   (50, 30, 0.75, 2, "interleaved", "bgr", 1, 16)],
                         ids=["2x-bicubic", "1.5x-lanczos3", "downscale"])
def test_nothing_outside_the_source_rectangle_is_used(srcnn, oracle_lib, w, h, mul, filt, layout, order, alpha, depth):
    S = srcnn
    dw, dh = out_size(w, h, mul)
    rng = np.random.default_rng(seed() + 77)
    img = image(w, h, alpha, depth, 9 * w + h)
    want = whole_want(oracle_lib, img, depth, mul, filt)
    rects = edge_rects(dw, dh, rng, limit=5) + [(dw // 2, dh // 2, 1, 1), (0, 0, 9, 9), (dw - 9, dh - 9, 9, 9)]
    assert len(rects) >= 12
    shrunk = 0
    for r in rects:
        sx0, sy0, sw, sh = S.rgb_rect_source(w, h, mul, filt, *r)
        other = rng.integers(0, 1 << depth, img.shape).astype(img.dtype)          # (integers cannot carry NaN: fresh noise instead)
        other[sy0:sy0 + sh, sx0:sx0 + sw] = img[sy0:sy0 + sh, sx0:sx0 + sw]
        shrunk += int(sw * sh < w * h)
        assert_rect(Rig(S, other, layout, order, depth, mul, filt).rect(*r), crop(want, r),
                    "source replaced outside %dx%d at (%d,%d), rect %r" % (sw, sh, sx0, sy0, r))
    assert shrunk >= 3          # the test has teeth: most source rectangles are smaller than the image


# ---- banding ----
@pytest.mark.parametrize("layout,order,alpha,depth", [("interleaved", "rgb", 0, 8), ("planar", "bgr", 1, 12)], ids=["rgb8", "planar-bgra12"])
def test_banded_rect_gives_the_same_bytes(srcnn, oracle_lib, layout, order, alpha, depth):
    S = srcnn
    L = S.lib()
    img = image(70, 40, alpha, depth, 7040 + depth)
    want = whole_want(oracle_lib, img, depth, 2.0, 2)
    rig = Rig(S, img, layout, order, depth, 2.0, 2)
    limit = 1 << 20
    # the window of these rects is all 140 columns: 32 planes x 4 B x 140 x (80 + 4) rows do not fit 1 MB, 54-row bands do
    assert 32 * 4 * 140 * (80 + 4) > limit
    band_rows = limit // (32 * 4 * 140) - 4
    bands = -(-80 // band_rows)
    assert bands >= 2
    rects = [(3, 0, 134, 80), (0, 0, 139, 80), (0, 0, 140, 80)]
    unbanded = [rig.rect(*r) for r in rects]
    prev = L.srcnn_set_workspace_limit(limit)
    S.profile_enable(True)
    try:
        for r, ref in zip(rects, unbanded):
            S.profile_reset()
            got = rig.rect(*r)
            launches = S.profile_read()["conv12"][1]
            assert launches == bands, (r, launches, bands)
            assert_rect(got, ref, "banded vs unbanded rect %r" % (r,))
            assert_rect(got, crop(want, r), "banded rect %r vs oracle" % (r,))
    finally:
        S.profile_enable(False)
        L.srcnn_set_workspace_limit(prev)


# ---- non-parity modes: Y' is the mode's own y_path_rect, every other step is the contract's ----
def merge_restated(oracle_lib, img, depth, mul, filt, rect, yp):
    """The restatement of tests/test_rgb_restatement.py for one rect, with Y' given (float32, rh x rw)."""
    h, w, c = img.shape
    dw, dh = out_size(w, h, mul)
    x0, y0, rw, rh = rect
    s, maxv, dt = depth - 8, (1 << depth) - 1, dtype_of(depth)
    down, up = F(2.0 ** -s), F(2.0 ** s)
    ch = [(img[..., k].astype(np.uint32) & maxv).astype(F) * down for k in range(c)]
    r, g, b = ch[:3]
    cb = F(128) - (F(0.1687) * r) - (F(0.3313) * g) + (F(0.5) * b)
    cr = F(128) + (F(0.5) * r) - (F(0.4187) * g) - (F(0.0813) * b)
    cfilt = 0 if filt == 0 else 1
    win = lambda p: oracle_lib.resample(p, dw, dh, cfilt)[y0:y0 + rh, x0:x0 + rw]   # noqa: E731
    cb, cr = win(cb) - F(128), win(cr) - F(128)
    outs = [yp + F(45) * cr / F(32), yp - (F(11) * cb + F(23) * cr) / F(32), yp + F(113) * cb / F(64)]
    if c == 4:
        outs.append(win(ch[3]))

    def code(v):
        assert v.dtype == F
        v = np.where(F(255) < v, F(255), v)
        v = np.where(F(0) > v, F(0), v)
        return (v * up).astype(np.uint32).astype(dt)
    return np.stack([code(v) for v in outs], axis=-1), (yp * up).astype(np.uint32).astype(dt)


def y_plane_of(img, depth):
    s, maxv = depth - 8, (1 << depth) - 1
    r, g, b = [(img[..., k].astype(np.uint32) & maxv).astype(F) * F(2.0 ** -s) for k in range(3)]
    return (F(0.299) * r) + (F(0.587) * g) + (F(0.114) * b)


def test_merge_restated_is_the_restatement_in_strict_mode(srcnn, oracle_lib):
    """The helper of the next test, held to the module's references first: with the oracle's Y' it is the crop of the restatement."""
    img = image(40, 31, 1, 12, 4031)
    want = restatement(oracle_lib, img, 12, 1.5, 3)
    yp = oracle_lib.y_path(y_plane_of(img, 12), 60, 46, 3)
    for rect in ((0, 0, 60, 46), (7, 5, 33, 20)):
        x0, y0, rw, rh = rect
        assert_rect(merge_restated(oracle_lib, img, 12, 1.5, 3, rect, yp[y0:y0 + rh, x0:x0 + rw]), crop(want, rect), "rect %r" % (rect,))
        got = srcnn.y_path_rect(y_plane_of(img, 12), 60, 46, 3, *rect)
        assert_bit_equal(got, yp[y0:y0 + rh, x0:x0 + rw], "strict y_path_rect %r" % (rect,))


@pytest.mark.parametrize("mode_name", ["MODE_FAST", "MODE_FAST_F16"])
def test_non_parity_modes_are_exact_around_their_y(srcnn, oracle_lib, mode_name):
    S = srcnn
    rng = np.random.default_rng(seed() + 5)
    prev = S.set_mode(getattr(S, mode_name))        # (a strict-only build refuses: conftest turns that into a skip)
    try:
        for (w, h, mul, filt, layout, order, alpha, depth) in ((70, 40, 2.0, 2, "interleaved", "rgb", 0, 8), (40, 31, 1.5, 3, "planar", "bgr", 1, 12),
                                                               (50, 30, 0.75, 1, "interleaved", "bgr", 1, 10)):
            dw, dh = out_size(w, h, mul)
            img = image(w, h, alpha, depth, 13 * w + h)
            yf = y_plane_of(img, depth)
            rig = Rig(S, img, layout, order, depth, mul, filt)
            for rect in edge_rects(dw, dh, rng, limit=4) + [(0, 0, dw, dh), (dw // 2, dh // 2, 1, 1)]:
                yp = S.y_path_rect(yf, dw, dh, filt, *rect)
                assert_rect(rig.rect(*rect), merge_restated(oracle_lib, img, depth, mul, filt, rect, yp),
                            "%s %dx%d x%g %s rect %r" % (mode_name, w, h, mul, layout, rect))
    finally:
        S.set_mode(prev)


# ---- two host threads on two streams, mixed formats; a second context ----
def test_two_threads_two_streams(srcnn):
    S = srcnn
    cases = [(LAYOUTS[k % 2], ORDERS[(k // 2) % 2], k % 3 == 0, DEPTHS[k % 5], 2.0 if k % 3 else 1.5, FILTERS[k % 5]) for k in range(8)]
    images = [arrange(image(97, 61, int(c[2]), c[3], 500 + k), c[0], c[1]) for k, c in enumerate(cases)]
    rects = [(3 + 5 * k, 2 + 3 * k, 50 + 7 * k, 31 + 4 * k) for k in range(8)]          # inside the smallest output, 145 x 91

    def call(k, st=None):
        c = cases[k]
        return S.rgb_upscale_rect(images[k], rects[k], multiply=c[4], filt=c[5], layout=c[0], order=c[1], depth=c[3], want_conv=True, stream=st)
    single = [call(k) for k in range(8)]
    results, errors = [None] * 8, []

    def worker(t):
        st = S.Stream()
        try:
            for k in range(t, 8, 2):
                results[k] = call(k, st)
        except Exception as e:          # noqa: BLE001
            errors.append(e)
        finally:
            st.destroy()
    threads = [threading.Thread(target=worker, args=(t,)) for t in range(2)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors
    for k in range(8):
        assert_rect(results[k], single[k], "image %d on thread %d" % (k, k % 2))


def test_second_context_through_its_own_stream(srcnn, oracle_lib):
    import rgb_rect_worker as W
    res = child("second_context")
    rect = (33, 21, 101, 47)
    for k, (alpha, depth, layout, order) in enumerate(((0, 8, "interleaved", "rgb"), (1, 12, "planar", "bgr"))):
        img = image(97, 61, alpha, depth, 300 + k)
        out, conv = crop(whole_want(oracle_lib, img, depth, 2.0, 2), rect)
        want = W.digest(arrange(out, layout, order), conv)
        assert res["case%d" % k] == [want, want], (k, layout, order)


# ---- torch tensors ----
def test_torch_tensors_vs_oracle(oracle_lib):
    import rgb_rect_worker as W
    res = child("torch")
    if "skip" in res:
        pytest.skip(res["skip"])
    img = image(37, 21, 0, 8, 11)
    rect = (5, 3, 41, 20)
    out, conv = crop(oracle_lib.process(img, 2.0, 2), rect)
    assert res["new"]["sha"] == W.digest(out, conv), "(H, W, 3) uint8, out=None"
    assert res["new"]["device"] == res["device"] and res["new"]["shape"] == [20, 41, 3] and res["new"]["contig"]
    assert res["inplace"]["sha"] == res["inplace"]["inside_sha"] == W.digest(out, conv), "in place into a full-size image"
    assert res["inplace"]["same_memory"] and res["inplace"]["rest_untouched"] and res["inplace"]["shape"] == [20, 41, 3]
    assert res["padded"]["inside_sha"] == W.digest(out) and res["padded"]["rest_untouched"], "in place into a row-padded image"
    img = image(30, 11, 1, 12, 12)
    rect = (7, 2, 33, 19)
    out, conv = crop(restatement(oracle_lib, img, 12, 2.5, 3), rect)
    assert res["chw4"]["sha"] == W.digest(out, conv), "(4, H, W) 12-bit BGR"
    assert res["chw4"]["device"] == res["device"] and res["chw4"]["shape"] == [4, 19, 33] and res["chw4"]["view_shape"] == [4, 19, 33]
    assert res["chw4"]["inside_sha"] == W.digest(out) and res["chw4"]["rest_untouched"], "(4, H, W) in place"
    assert res["refused"] == [True] * 5


# ---- one real size ----
def test_1080p_to_4k_interior_and_corner(srcnn):
    S = srcnn
    w, h = 1920, 1080
    img = image(w, h, 0, 8, 1080)
    whole = run(S, img, "interleaved", "rgb", 8, 2.0, 2)          # (held to the oracle by tests/test_gpu_rgb.py and the shell tests)
    rig = Rig(S, img, "interleaved", "rgb", 8, 2.0, 2)
    for (x0, y0) in ((1601, 903), (3840 - 640, 2160 - 360)):
        assert_rect(rig.rect(x0, y0, 640, 360), crop(whole, (x0, y0, 640, 360)), "640x360 rect at (%d,%d) of 3840x2160" % (x0, y0))
