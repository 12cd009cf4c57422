"""srcnn_yuv_upscale_rect_list_dev (include/srcnn_amd_yuv_rect_list.h) byte for byte against crops of the whole frame (GPU).

Every item of a list is a crop of what srcnn_yuv_upscale_dev writes -- the luma rect and the chroma samples that cover it -- so
every expectation is a crop of the whole-frame expectation of tests/test_gpu_yuv_ex.py (frame(), expected(): the oracle
composition), computed once per frame and never by the call under test; where the contract names it, results are also compared
with the loop of srcnn_yuv_upscale_rect_dev.  The frame is 96 x 56 -> 192 x 112, 2x bicubic, unless said otherwise: the frame of
tests/test_gpu_rect_list.py, whose cells straddle the tile seams of the layer kernels.  Lists are seeded and snapped to the
format's origin rule.  Every child process runs under a timeout of its own and nothing is tried twice.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import yuv_rect_list_worker as LW
from rect_list_worker import DH, DW, H, W, border_rects, seeded_rects
from test_gpu_yuv import first_difference
from test_gpu_yuv_ex import LAYOUTS, expected, frame, run, to_words
from yuv_rect_list_worker import YuvListRig, snapped
from yuv_rect_worker import chroma_rect, interleave, snap

pytestmark = pytest.mark.gpu

FILTER_NAMES = ("nearest", "bilinear", "bicubic", "lanczos3", "bspline")
CANARY = 0xA5
GUARD = 1024
WORKER = os.path.join(os.path.dirname(os.path.abspath(__file__)), "yuv_rect_list_worker.py")
SEED = LW.FRAME_SEED
_WANT = {}
_DIGEST = {}


def whole(oracle_lib, chroma, depth, seed=SEED, mul=2.0, filt=2, w=W, h=H):
    """((Y, U, V), (Y', U', V') of the whole frame) as values: computed once, read-only."""
    key = (chroma, depth, seed, mul, filt, w, h)
    if key not in _WANT:
        src = frame(w, h, chroma, depth, seed)
        want = expected(oracle_lib, *src, chroma, depth, mul, filt)
        for a in tuple(src) + tuple(want):
            a.setflags(write=False)
        _WANT[key] = (src, tuple(want))
    return _WANT[key]


def crop(planes, rect, chroma):
    """The rect of a whole frame's (Y', U', V'): the luma rect and the chroma samples that cover it."""
    x0, y0, rw, rh = rect
    cx0, cy0, crw, crh = chroma_rect(rect, chroma)
    return (planes[0][y0:y0 + rh, x0:x0 + rw], planes[1][cy0:cy0 + crh, cx0:cx0 + crw], planes[2][cy0:cy0 + crh, cx0:cx0 + crw])


def assert_item(got, want, what):
    assert len(got) == len(want), (what, len(got), len(want))
    for name, g, e in zip("YUV", got, want):
        assert g.shape == e.shape and g.dtype == e.dtype, (what, name, g.shape, e.shape, g.dtype, e.dtype)
        assert np.array_equal(g, e), "%s %s': %s" % (what, name, first_difference(g, e))


def check_list(got, want, rects, chroma, what):
    assert len(got) == len(rects)
    for k, (g, r) in enumerate(zip(got, rects)):
        assert_item(g, crop(want, r, chroma), "%s: item %d, rect %dx%d at (%d,%d)" % (what, k, r[2], r[3], r[0], r[1]))


def all_batched(rig, rects, atlases=None):
    p = rig.plan(rects)
    assert p.batched_items == len(rects) and p.single_items == 0, (p.batched_items, p.single_items)
    assert atlases is None or p.atlases == atlases


def rig_for(S, src, layout, chroma, depth, msb, mul=2.0, filt=2):
    return YuvListRig(S, *src, layout, chroma, depth, msb, mul, filt)


# ---- 1. borders ----
@pytest.mark.parametrize("cell", LW.BORDER_CELLS, ids=["i420", "p210-422", "planar444-16"])
def test_borders_vs_oracle_and_the_loop_of_single_calls(srcnn, oracle_lib, cell):
    layout, chroma, depth, msb = cell
    src, want = whole(oracle_lib, chroma, depth)
    rig = rig_for(srcnn, src, *cell)
    rects = snapped(border_rects(), chroma)
    all_batched(rig, rects, atlases=1)
    raw = rig.raw_run(rects)
    _DIGEST[cell] = LW.digest(raw)
    check_list([rig.to_values(one) for one in raw], want, rects, chroma, "borders vs the whole frame")
    for k, (g, s) in enumerate(zip(raw, rig.raw_loop(rects))):
        assert_item(g, s, "borders: item %d vs the single call (raw words)" % k)


# ---- 2. every kernel instantiation on the batched route ----
CELLS = [(layout, chroma, depth, msb) for layout in ("planar", "semiplanar") for chroma in ("420", "422", "444")
         for (depth, msb) in ((8, 0), (10, 0), (10, 1), (16, 0))]
assert len(CELLS) == 24


@pytest.mark.parametrize("layout,chroma,depth,msb", CELLS, ids=["%s-%s-%d%s" % (c[0], c[1], c[2], "msb" if c[3] else "") for c in CELLS])
def test_every_format_cell_on_the_batched_route(srcnn, oracle_lib, layout, chroma, depth, msb):
    src, want = whole(oracle_lib, chroma, depth)
    rig = rig_for(srcnn, src, layout, chroma, depth, msb)
    rects = snapped(seeded_rects(200 + CELLS.index((layout, chroma, depth, msb)), 32) + [(0, 0, DW, DH)], chroma)
    all_batched(rig, rects)
    check_list(rig.run(rects), want, rects, chroma, "%s %s %d-bit msb=%d" % (layout, chroma, depth, msb))


# ---- 3. many small rects repainted in place ----
class Surface:
    """A full-size dw x dh frame of canary bytes in one device buffer, every plane from a 256-byte boundary, tight pitches."""

    def __init__(self, S, layout, chroma, depth, dw=DW, dh=DH):
        self.S, self.chroma, self.semi = S, chroma, layout == "semiplanar"
        self.bps = 1 if depth == 8 else 2
        fmt = S.yuv_format(layout, chroma, depth, 0)
        self.n = 2 if self.semi else 3
        sizes = [S.yuv_plane_size(fmt, dw, dh, k) for k in range(self.n)]
        self.rows = [r for (_c, r, _rb) in sizes]
        self.pitch = [rb for (_c, _r, rb) in sizes]
        self.off, pos = [], 0
        for r, rb in zip(self.rows, self.pitch):
            self.off.append(pos)
            pos += (r * rb + 255) & ~255
        self.total = pos
        self.buf = S.DeviceBuffer.from_numpy(np.full(self.total, CANARY, np.uint8))

    def first(self, rect):
        """Per plane: the byte offset of the rect's first sample (luma (x0, y0), chroma (cx0, cy0))."""
        x0, y0, _, _ = rect
        cx0, cy0, _, _ = chroma_rect(rect, self.chroma)
        spp = 2 if self.semi else 1
        return [self.off[0] + y0 * self.pitch[0] + x0 * self.bps] + [self.off[k] + cy0 * self.pitch[k] + cx0 * spp * self.bps for k in range(1, self.n)]

    def item(self, rect):
        return tuple(rect) + ([(self.buf, o) for o in self.first(rect)], list(self.pitch))

    def planes(self):
        """The surface back on the host, as bytes per plane."""
        flat = self.buf.to_numpy(np.uint8, (self.total,))
        return [flat[o:o + r * p].reshape(r, p) for o, r, p in zip(self.off, self.rows, self.pitch)]

    def expect(self, want, depth, msb, rects):
        """(bytes per plane, painted fraction of luma): canary everywhere but on the rects' samples, which hold `want`."""
        words = [to_words(np.asarray(P), depth, msb) for P in want]
        full = [words[0], interleave(words[1], words[2])] if self.semi else words
        full = [np.ascontiguousarray(p).view(np.uint8) for p in full]
        mask_y = np.zeros(want[0].shape, bool)
        mask_c = np.zeros(want[1].shape, bool)
        for r in rects:
            x0, y0, rw, rh = r
            cx0, cy0, crw, crh = chroma_rect(r, self.chroma)
            mask_y[y0:y0 + rh, x0:x0 + rw] = True
            mask_c[cy0:cy0 + crh, cx0:cx0 + crw] = True
        out = []
        for k, p in enumerate(full):
            m = mask_y if k == 0 else mask_c
            m = np.repeat(m, self.bps * (2 if self.semi and k else 1), axis=1)
            e = np.full(p.shape, CANARY, np.uint8)
            e[m] = p[m]
            out.append(e)
        return out, float(mask_y.mean())


@pytest.mark.parametrize("layout,depth,msb", [("semiplanar", 8, 0), ("semiplanar", 10, 1), ("planar", 8, 0)], ids=["nv12", "p010", "i420"])
def test_repaint_inside_one_full_size_surface(srcnn, oracle_lib, layout, depth, msb):
    S = srcnn
    src, want = whole(oracle_lib, "420", depth)
    rig = rig_for(S, src, layout, "420", depth, msb)
    rects = snapped(seeded_rects(64001, 64), "420")
    all_batched(rig, rects)
    sf = Surface(S, layout, "420", depth)
    bps, semi = sf.bps, layout == "semiplanar"
    luma_store, chroma_store = 4 * bps, 4 * bps * (2 if semi else 1)
    firsts = [sf.first(r) for r in rects]
    assert sf.buf.ptr % 256 == 0 and sf.pitch[0] % luma_store == 0 and all(p % chroma_store == 0 for p in sf.pitch[1:])
    luma = {(sf.buf.ptr + f[0]) % luma_store == 0 for f in firsts}
    chroma = {all((sf.buf.ptr + o) % chroma_store == 0 for o in f[1:]) for f in firsts}
    assert luma == {True, False} and chroma == {True, False}, "both store paths must run for luma and for chroma"
    S.yuv_upscale_rect_list_dev(rig.fmt, W, H, 2.0, 2, rig.din + rig.pad, None, [sf.item(r) for r in rects])
    S.sync()
    expect, painted = sf.expect(want, depth, msb, rects)
    assert 0.2 < painted < 1.0                              # overlaps happen, and so does untouched ground
    for k, (g, e) in enumerate(zip(sf.planes(), expect)):
        assert np.array_equal(g, e), "plane %d: %s" % (k, first_difference(g, e))


# ---- 4. pitches and guard bands ----
@pytest.mark.parametrize("layout,depth,msb", [("planar", 8, 0), ("semiplanar", 10, 1)], ids=["i420", "p010"])
def test_pitched_guarded_destinations(srcnn, oracle_lib, layout, depth, msb):
    S = srcnn
    chroma = "420"
    src, want = whole(oracle_lib, chroma, depth)
    rig = rig_for(S, src, layout, chroma, depth, msb)
    # 1 x 1, 3 x 5, 64 x 16, a full-width strip, an odd-width rect ending mid-frame, and three more
    rects = [(64, 32, 1, 1), (50, 20, 3, 5), (20, 16, 64, 16), (0, 40, DW, 9), (8, 6, 37, 11), (DW - 10, DH - 10, 10, 10), (0, 0, 8, 8), (100, 0, 12, 40)]
    assert rects == snapped(rects, chroma) and len(rects) == 8
    all_batched(rig, rects)
    bps, n, spp = rig.bps, rig.n, (2 if layout == "semiplanar" else 1)
    pos, spans = 0, []
    for k, r in enumerate(rects):
        one = []
        for p in range(n):
            cols, prow = (r[2], r[3]) if p == 0 else chroma_rect(r, chroma)[2:]
            row = cols * bps * (1 if p == 0 else spp)
            pitch = (row + 3) // 4 * 4 + 8 if (k + p) % 2 == 0 else row + bps + (bps if (row + bps) % 4 == 0 else 0)     # a multiple of 4, or not
            assert pitch > row and pitch % bps == 0 and ((k + p) % 2 == 0) == (pitch % 4 == 0)
            off = 2 if bps == 2 else (1, 2, 3)[k % 3]                                                            # even bases at depth > 8
            start = (pos + GUARD + 3) // 4 * 4 + off * ((k // 2) % 2)                                            # 4-byte aligned, or not
            pos = start + pitch * (prow - 1) + row
            one.append((start, pitch, row, prow))
        spans.append(one)
    total = pos + GUARD
    buf = S.DeviceBuffer.from_numpy(np.full(total, CANARY, np.uint8))
    items = [tuple(r) + ([(buf, s) for (s, _, _, _) in one], [pt for (_, pt, _, _) in one]) for r, one in zip(rects, spans)]
    S.yuv_upscale_rect_list_dev(rig.fmt, W, H, 2.0, 2, rig.din + rig.pad, None, items)
    S.sync()
    raw = buf.to_numpy(np.uint8, (total,))

    def take(start, pitch, row, prow):
        got = np.empty((prow, row), np.uint8)
        for y in range(prow):
            a = start + y * pitch
            got[y] = raw[a:a + row]
            raw[a:a + row] = CANARY
        return np.ascontiguousarray(got).view(rig.dt)
    for k, (r, one) in enumerate(zip(rects, spans)):
        got = rig.to_values([take(*sp) for sp in one])
        assert_item(got, crop(want, r, chroma), "pitched item %d" % k)
    touched = np.flatnonzero(raw != CANARY)
    assert touched.size == 0, "%d padding / guard bytes written, first at %d" % (touched.size, int(touched[0]))


# ---- 5. neighbouring rects that share a chroma column ----
@pytest.mark.parametrize("layout", ["planar", "semiplanar"], ids=["i420", "nv12"])
def test_shared_chroma_column(srcnn, oracle_lib, layout):
    S = srcnn
    src, want = whole(oracle_lib, "420", 8)
    rig = rig_for(S, src, layout, "420", 8, 0)
    x, y = 30, 20
    first = [(x, y, 5, 7), (x + 6, y, 4, 7)]                  # adjacent: chroma columns [15, 18) and [18, 20)
    second = [(x + 60, y + 40, 5, 6), (x + 64, y + 40, 6, 6)]       # chroma column 47 is written by both
    a, b = chroma_rect(second[0], "420"), chroma_rect(second[1], "420")
    assert a[0] + a[2] - 1 == b[0] == 47 and chroma_rect(first[0], "420")[0] + chroma_rect(first[0], "420")[2] == chroma_rect(first[1], "420")[0]
    rects = first + second
    all_batched(rig, rects)
    sf = Surface(S, layout, "420", 8)
    S.yuv_upscale_rect_list_dev(rig.fmt, W, H, 2.0, 2, rig.din + rig.pad, None, [sf.item(r) for r in rects])
    S.sync()
    expect, _ = sf.expect(want, 8, 0, rects)
    for k, (g, e) in enumerate(zip(sf.planes(), expect)):
        assert np.array_equal(g, e), "plane %d: %s" % (k, first_difference(g, e))


# ---- 6. source rectangle ----
@pytest.mark.parametrize("layout,depth,msb", [("planar", 8, 0), ("semiplanar", 10, 1)], ids=["i420", "p010"])
def test_nothing_outside_the_union_of_the_source_rectangles_is_read(srcnn, oracle_lib, layout, depth, msb):
    S = srcnn
    chroma = "420"
    src, want = whole(oracle_lib, chroma, depth)
    rects = snapped([(0, 0, 9, 9), (DW - 9, DH - 9, 9, 9), (90, 50, 1, 1), (40, 0, 30, 12), (0, 70, 7, 20)] + seeded_rects(77, 6, hi=20), chroma)
    fmt = S.yuv_format(layout, chroma, depth, msb)
    rng = np.random.default_rng(31337)
    other = []
    for k, P in enumerate(src):
        keep = np.zeros(P.shape, bool)
        for r in rects:
            sx0, sy0, sw, sh = S.yuv_rect_source(fmt, W, H, 2.0, 2, *r, min(k, 1) if layout == "semiplanar" else k)
            keep[sy0:sy0 + sh, sx0:sx0 + sw] = True
        Q = (P ^ rng.integers(1, 256, P.shape).astype(P.dtype)) & ((1 << depth) - 1)       # other values: every sample differs
        Q[keep] = P[keep]
        assert (Q != P).mean() > 0.2, "plane %d"  % k                                      # the test has teeth
        other.append(Q)
    rig = rig_for(S, other, layout, chroma, depth, msb)
    all_batched(rig, rects)
    check_list(rig.run(rects), want, rects, chroma, "altered source")


# ---- 7. several atlases ----
def test_split_atlas_is_byte_identical(srcnn, oracle_lib):
    S = srcnn
    src, want = whole(oracle_lib, "420", 10)
    rig = rig_for(S, src, "semiplanar", "420", 10, 1)
    rects = snapped(seeded_rects(64001, 64) + [(0, 0, 60, 50), (DW - 70, DH - 30, 70, 30)], "420")
    one = rig.raw_run(rects)
    check_list([rig.to_values(o) for o in one], want, rects, "420", "one atlas")
    prev = S.lib().srcnn_set_workspace_limit(1 << 20)
    try:
        p = rig.plan(rects)
        assert p.atlases >= 3 and p.batched_items + p.single_items == len(rects), (p.atlases, p.batched_items, p.single_items)
        split = rig.raw_run(rects)
    finally:
        S.lib().srcnn_set_workspace_limit(prev)
    for k, (a, b) in enumerate(zip(split, one)):
        assert_item(a, b, "split atlas, item %d" % k)


# ---- 8. calls back to back ----
def test_three_lists_back_to_back_on_one_stream(srcnn, oracle_lib):
    S = srcnn
    src, want = whole(oracle_lib, "420", 8)
    rig = rig_for(S, src, "semiplanar", "420", 8, 0)
    a = snapped(seeded_rects(71, 48), "420")
    b = snapped(border_rects()[:30] + seeded_rects(72, 9, hi=25), "420")
    st = S.Stream()
    try:
        qa = rig.queue(a, st)
        qb = rig.queue(b, st)              # (no sync in between: each call has its own descriptor slot)
        qc = rig.queue(a[::-1], st)
        st.sync()
        check_list(rig.fetch(*qa), want, a, "420", "first of three calls")
        check_list(rig.fetch(*qb), want, b, "420", "second of three calls")
        check_list(rig.fetch(*qc), want, a[::-1], "420", "third of three calls")
    finally:
        st.destroy()


# ---- 9. every filter at 2x, NV12 ----
@pytest.mark.parametrize("filt", range(5), ids=FILTER_NAMES)
def test_every_filter(srcnn, oracle_lib, filt):
    src, want = whole(oracle_lib, "420", 8, filt=filt)
    rig = rig_for(srcnn, src, "semiplanar", "420", 8, 0, filt=filt)
    rects = snapped(border_rects()[:12] + seeded_rects(80 + filt, 8) + [(0, 0, DW, DH)], "420")
    all_batched(rig, rects)
    check_list(rig.run(rects), want, rects, "420", FILTER_NAMES[filt])


# ---- 10. other ratios: whichever route the plan reports ----
@pytest.mark.parametrize("w,h,mul", [(40, 31, 1.5), (50, 30, 0.75), (24, 24, 1.0), (30, 1, 1.5), (1, 9, 2.0)],
                         ids=["x1.5", "downscale", "identity", "kept-rows", "kept-chroma-columns"])
def test_other_ratios(srcnn, oracle_lib, w, h, mul):
    S = srcnn
    dw, dh = S.output_size(w, h, mul)
    chroma = "420"
    layout, depth, msb = ("semiplanar", 8, 0) if w % 20 else ("planar", 10, 1)
    up, down = dw > w and dh > h, dw < w and dh < h
    cw, ch, dcw, dch = (w + 1) // 2, (h + 1) // 2, (dw + 1) // 2, (dh + 1) // 2
    chroma_up = dcw > cw and dch > ch
    if (up and chroma_up) or (down and dcw < cw and dch < ch):
        src, want = whole(oracle_lib, chroma, depth, 520 + w, mul=mul, w=w, h=h)
    else:                                  # the identity size and kept axes: the library's own whole frame (srcnn_yuv_upscale_dev)
        src = frame(w, h, chroma, depth, 520 + w)
        want = run(S, LAYOUTS[layout], chroma, depth, msb, *src, mul, 2)
    rig = rig_for(S, src, layout, chroma, depth, msb, mul=mul)
    rects = snapped(seeded_rects(90 + w, 24, dw, dh, hi=30) + [(0, 0, 1, 1), (dw - 1, dh - 1, 1, 1), (0, 0, dw, dh), (0, dh // 2, dw, 1), (dw // 2, 0, 1, dh)],
                    chroma)
    p = rig.plan(rects)
    if up and chroma_up:
        assert (w, h, mul) == (40, 31, 1.5) and p.batched_items == len(rects)
    else:
        assert p.single_items == len(rects) and p.atlases == 0
    assert (w, h) != (1, 9) or (up and not chroma_up)        # luma grows, the chroma columns keep their number
    check_list(rig.run(rects), want, rects, chroma, "%dx%d x%g" % (w, h, mul))


# ---- 11. the forced single route ----
def child(mode, env=None, timeout=600):
    r = subprocess.run([sys.executable, WORKER, mode], env=dict(os.environ, **(env or {})), capture_output=True, text=True, timeout=timeout)
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")]
    assert r.returncode == 0 and line, "yuv_rect_list_worker %s: exit %d\n%s\n%s" % (mode, r.returncode, r.stdout[-600:], r.stderr[-1500:])
    return json.loads(line[0][7:])


def test_unfused_child_gives_the_same_bytes(srcnn):
    S = srcnn
    assert "SRCNN_YUV_RECT_LIST_UNFUSED=0" in S.debug_settings()
    fast = {"/".join(str(v) for v in cell): _DIGEST.get(cell) or LW.border_digest(S, cell) for cell in LW.BORDER_CELLS}
    assert child("unfused", {"SRCNN_YUV_RECT_LIST_UNFUSED": "1"}) == fast


# ---- 12. a non-parity mode: the list is the loop ----
def test_fast_mode_equals_the_loop_of_single_calls(srcnn):
    S = srcnn
    prev = S.set_mode(S.MODE_FAST)        # (a strict-only build refuses: conftest turns that into a skip)
    try:
        rig = rig_for(S, frame(W, H, "420", 10, 1212), "semiplanar", "420", 10, 1)
        rects = snapped(border_rects()[:20] + seeded_rects(99, 12), "420")
        p = rig.plan(rects)
        assert p.single_items == len(rects) and p.batched_items == 0 and p.atlases == 0
        for k, (a, b) in enumerate(zip(rig.raw_run(rects), rig.raw_loop(rects))):
            assert_item(a, b, "MODE_FAST, item %d vs the single call" % k)
    finally:
        S.set_mode(prev)


# ---- 13. the convenience call ----
def test_numpy_convenience(srcnn, oracle_lib):
    S = srcnn
    rects = [snap(r, "420") for r in [(0, 0, 1, 1), (33, 21, 70, 40), (DW - 5, 3, 5, 100), (100, 60, 17, 3)]]
    src, want = whole(oracle_lib, "420", 8)
    got = S.yuv_upscale_rects(src, rects)                                          # I420
    assert all(isinstance(p, np.ndarray) and p.dtype == np.uint8 for it in got for p in it)
    check_list(got, want, rects, "420", "yuv_upscale_rects, I420")
    src, want = whole(oracle_lib, "420", 10)
    words = [to_words(np.asarray(P), 10, 1) for P in src]
    got = S.yuv_upscale_rects([words[0], interleave(words[1], words[2])], rects, layout="semiplanar", depth=10, msb_aligned=True)      # P010
    assert all(len(it) == 2 for it in got)
    vals = [(yp >> 6, np.ascontiguousarray(uv[:, 0::2]) >> 6, np.ascontiguousarray(uv[:, 1::2]) >> 6) for (yp, uv) in got]
    assert not any(np.any(p & 63) for it in got for p in it)
    check_list(vals, want, rects, "420", "yuv_upscale_rects, P010")
    assert S.yuv_upscale_rects(src, []) == []
    S.yuv_upscale_rect_list_dev(S.yuv_format(), W, H, 2.0, 2, None, None, [])       # n == 0: nothing is looked at
