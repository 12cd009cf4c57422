"""srcnn_yuv_packed_upscale_rect_list_dev (include/srcnn_amd_yuv_packed_rect_list.h) byte for byte against crops of the whole
frame (GPU).

Every item of a list is a crop, by span, of what srcnn_yuv_packed_upscale_dev writes, so every expectation is a crop
(yuv_packed_rect_worker.crop) of the packed oracle composition of the whole frame (want_for / pack of tests/test_gpu_yuv_packed.py),
computed once per frame and never by the call under test; where the contract names it, results are also compared with the loop
of srcnn_yuv_packed_upscale_rect_dev.  The frame is 96 x 56 -> 192 x 112, 2x bicubic, unless said otherwise: the frame of
tests/rect_list_worker.py, whose cells straddle the tile seams of the layer kernels; the two EDGE_SHAPES of the packed rect tests
add v210's padding groups (140 is no multiple of 6) and the empty slot of an odd 4:2:2 width (87).  Lists are seeded and snapped
to the format's unit.  Every child process runs under a timeout of its own and nothing is tried twice.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import yuv_packed_rect_list_worker as LW
from rect_list_worker import DH, DW, H, W, seeded_rects
from test_gpu_yuv import first_difference
from test_gpu_yuv_packed import frame_planes, pack, want_for
from yuv_packed_rect_list_worker import MAIN, PackedListRig, main_rects, snapped, source
from yuv_packed_rect_worker import EDGE_SHAPES, NAMES, UNIT, crop, out_size, row_bytes, span

pytestmark = pytest.mark.gpu

FILTER_NAMES = ("nearest", "bilinear", "bicubic", "lanczos3", "bspline")
CANARY = 0xA5
GUARD = 1024
WORKER = os.path.join(os.path.dirname(os.path.abspath(__file__)), "yuv_packed_rect_list_worker.py")
_WHOLE = {}
_DIGEST = {}


def whole(oracle_lib, name, case=MAIN):
    """The packed oracle composition of the whole output frame: (dh, row bytes) uint8, computed once, read-only."""
    key = (name, case)
    if key not in _WHOLE:
        a = pack(name, *want_for(oracle_lib, name, case))
        a.setflags(write=False)
        _WHOLE[key] = a
    return _WHOLE[key]


def assert_bytes(got, want, what):
    assert got.dtype == np.uint8 and got.shape == want.shape, (what, got.shape, want.shape)
    assert np.array_equal(got, want), "%s: %s" % (what, first_difference(got, want))


def check_list(got, want, rects, name, dw, what):
    assert len(got) == len(rects)
    for k, (g, r) in enumerate(zip(got, rects)):
        assert_bytes(g, crop(want, r, name, dw), "%s %s: item %d, rect %dx%d at (%d,%d)" % (what, name, k, r[2], r[3], r[0], r[1]))


def all_batched(rig, rects, atlases=None):
    p = rig.plan(rects)
    assert p.batched_items == len(rects) and p.single_items == 0, (p.batched_items, p.single_items)
    assert atlases is None or p.atlases == atlases
    return p


def rig_for(S, name, case=MAIN, src=None):
    w, _h, filt, mul = case
    return PackedListRig(S, name, source(name, case) if src is None else src, w, mul, filt)


# ---- 1. all ten formats on the batched route ----
@pytest.mark.parametrize("name", NAMES)
def test_every_format_on_the_batched_route(srcnn, oracle_lib, name):
    want = whole(oracle_lib, name)
    rig = rig_for(srcnn, name)
    rects = main_rects(name, NAMES.index(name))
    assert (0, 0, DW, DH) in rects and len(rects) >= 25
    all_batched(rig, rects)
    got = rig.run(rects)
    _DIGEST[name] = LW.digest(got)
    check_list(got, want, rects, name, DW, "batched vs the whole frame")
    for k, (g, s) in enumerate(zip(got, rig.fetch(*rig.loop(rects)))):
        assert_bytes(g, s, "%s item %d vs the single call (raw bytes)" % (name, k))


# ---- 2. the edge shapes: padding groups and the empty slot ----
def edge_case(shape):
    w, h, mul, filt = shape
    return (w, h, filt, mul)


def border_list(name, dw, dh, seed):
    """Rects at and next to all four borders, then seeded ones: at least 5 end at dw and at least 5 stop short of it."""
    u = UNIT[name]
    r = [(0, 0, dw, dh), (0, 0, u, 1), (0, dh - 1, u, 1), (dw - 1, 0, 1, 1), (dw - 1, dh - 1, 1, 1),
         (0, 3, 3 * u, 9), (u, 0, 4 * u, 5), (2 * u, dh - 7, 5 * u, 7), (dw - 7, 5, 7, 11), (dw - 13, dh - 9, 13, 9), (dw - 30, 0, 30, 3),
         (dw - 2 * u - 9, 7, 9, 8), (dw - 3 * u - 20, dh - 4, 20, 3), (dw - 40, 20, 40 - 6, 10), (6, 6, dw - 18, dh - 12), (0, dh // 2, dw, 1),
         (0, 0, 66, 17), (60, 1, 72, 16)]
    r = [q for q in r if q[0] >= 0 and q[0] + q[2] <= dw]
    return snapped(r + seeded_rects(seed, 12, dw, dh, hi=30), name, dw)


@pytest.mark.parametrize("shape", EDGE_SHAPES, ids=["140x80", "87x50"])
@pytest.mark.parametrize("name", NAMES)
def test_edge_shapes_at_the_borders(srcnn, oracle_lib, name, shape):
    case = edge_case(shape)
    dw, dh = out_size(case[0], case[1], case[3])
    assert (dw, dh) in ((140, 80), (87, 50))
    want = whole(oracle_lib, name, case)
    rig = rig_for(srcnn, name, case)
    rects = border_list(name, dw, dh, 400 + NAMES.index(name))
    assert len(set(rects)) == len(rects)
    assert sum(1 for r in rects if r[0] + r[2] == dw) >= 5 and sum(1 for r in rects if r[0] + r[2] < dw) >= 5
    assert any(r[0] == 0 for r in rects) and any(r[1] == 0 for r in rects) and any(r[1] + r[3] == dh for r in rects)
    all_batched(rig, rects)
    got = rig.run(rects)
    check_list(got, want, rects, name, dw, "edge shape %dx%d" % (dw, dh))
    for k, (g, s) in enumerate(zip(got, rig.fetch(*rig.loop(rects)))):
        assert_bytes(g, s, "%s edge item %d vs the single call" % (name, k))


# ---- 3. many small rects repainted inside one full-size surface ----
@pytest.mark.parametrize("name", ["yuy2", "y210", "y410", "v210"])
def test_repaint_inside_one_full_size_surface(srcnn, oracle_lib, name):
    S = srcnn
    want = whole(oracle_lib, name)
    rig = rig_for(S, name)
    rects = snapped(seeded_rects(64001, 64), name, DW)
    all_batched(rig, rects)
    pitch = row_bytes(name, DW)
    assert pitch % 16 == 0
    # An item's store path is io_of(its first byte, the pitch).  A v210 span starts on a 16-byte group, so inside ONE surface all
    # its items share a path: v210 is painted twice, into a surface on a 16-byte boundary and into one 4 bytes past it.
    paths = set()
    for base in ((0, 4) if name == "v210" else (0,)):
        buf = S.DeviceBuffer.from_numpy(np.full(DH * pitch + 16, CANARY, np.uint8))
        assert buf.ptr % 16 == 0
        firsts = [base + y0 * pitch + span(name, DW, x0, rw)[0] for (x0, y0, rw, _rh) in rects]
        paths |= {f % 16 == 0 for f in firsts}
        S.yuv_packed_upscale_rect_list_dev(name, W, H, 2.0, 2, rig.din, 0, [tuple(r) + ((buf, f), pitch) for r, f in zip(rects, firsts)])
        S.sync()
        flat = buf.to_numpy(np.uint8, (DH * pitch + 16,))
        assert np.all(flat[:base] == CANARY) and np.all(flat[base + DH * pitch:] == CANARY)
        got = flat[base:base + DH * pitch].reshape(DH, pitch)
        mask = np.zeros((DH, pitch), bool)
        count = np.zeros((DH, pitch), np.int32)
        for (x0, y0, rw, rh) in rects:
            off, n = span(name, DW, x0, rw)
            mask[y0:y0 + rh, off:off + n] = True
            count[y0:y0 + rh, off:off + n] += 1
        assert count.max() >= 2, "overlaps must happen"
        assert 0.2 < float(mask.mean()) < 1.0                 # ... and so does untouched ground
        assert_bytes(got, np.where(mask, want, np.uint8(CANARY)), "%s repainted surface at +%d" % (name, base))
    assert paths == {True, False}, "both store paths must run"


# ---- 4. pitches and guard bands ----
@pytest.mark.parametrize("name", ["uyvy", "y216", "vuya", "y416", "v210"])
def test_pitched_guarded_destinations(srcnn, oracle_lib, name):
    S = srcnn
    want = whole(oracle_lib, name)
    rig = rig_for(S, name)
    u = UNIT[name]
    align = S.yuv_packed_row_bytes(name, DW)[1]
    # the smallest rect the unit allows (mid-frame and in the last unit of a row), a full-width strip, a rect ending mid-frame, more
    rects = [(66, 32, u, 1), (DW - u, 0, u, 1), (0, 40, DW, 1), (0, 41, DW, 9), (12, 6, 36, 11), (DW - 12, DH - 10, 12, 10), (0, 0, 6, 8), (102, 0, 12, 40)]
    assert rects == snapped(rects, name, DW) and len(rects) == 8
    assert (u, 1) == {"uyvy": (2, 1), "y216": (2, 1), "vuya": (1, 1), "y416": (1, 1), "v210": (6, 1)}[name]
    all_batched(rig, rects)
    pos, spans = 0, []
    for k, (x0, _y0, rw, rh) in enumerate(rects):
        n = span(name, DW, x0, rw)[1]
        pitch = (n + 15) // 16 * 16 + 16 if k % 2 == 0 else n + align * (1 + k)         # a multiple of 16, or the alignment only
        start = (pos + GUARD + 15) // 16 * 16 + align * ((k // 2) % 2)                  # 16-byte aligned, or the alignment only
        assert pitch >= n and pitch % align == 0 and start % align == 0
        pos = start + pitch * (rh - 1) + n
        spans.append((start, pitch, n, rh))
    total = pos + GUARD
    buf = S.DeviceBuffer.from_numpy(np.full(total, CANARY, np.uint8))
    assert buf.ptr % 16 == 0
    S.yuv_packed_upscale_rect_list_dev(name, W, H, 2.0, 2, rig.din, 0, [tuple(r) + ((buf, s), p) for r, (s, p, _n, _rh) in zip(rects, spans)])
    S.sync()
    raw = buf.to_numpy(np.uint8, (total,))
    for k, (r, (start, pitch, n, rh)) in enumerate(zip(rects, spans)):
        got = np.empty((rh, n), np.uint8)
        for y in range(rh):
            a = start + y * pitch
            got[y] = raw[a:a + n]
            raw[a:a + n] = CANARY
        assert_bytes(got, crop(want, r, name, DW), "%s pitched item %d" % (name, k))
    touched = np.flatnonzero(raw != CANARY)
    assert touched.size == 0, "%d padding / guard bytes written, first at %d" % (touched.size, int(touched[0]))


# ---- 5. source rectangle ----
@pytest.mark.parametrize("name", ["yuy2", "y212", "y410", "v210"])
def test_nothing_outside_the_union_of_the_source_rectangles_is_read(srcnn, oracle_lib, name):
    S = srcnn
    want = whole(oracle_lib, name)
    rects = snapped([(0, 0, 12, 9), (18, 4, 24, 20), (6, 30, 30, 6), (48, 0, 6, 1)] + seeded_rects(77, 8, 72, 48, hi=20), name, DW)     # one corner
    src = source(name, MAIN)
    keep = np.zeros(src.shape, bool)
    for r in rects:
        sx0, sy0, sw, sh = S.yuv_packed_rect_source(name, W, H, 2.0, 2, *r)
        off, n = span(name, W, sx0, sw)
        keep[sy0:sy0 + sh, off:off + n] = True
    assert 0.05 < keep.mean() < 0.8, "the union must be a proper subset of the frame"
    rng = np.random.default_rng(31337)
    planes = frame_planes(name, W, H, 4242)
    other = pack(name, *planes, junk=rng) if name in ("y212", "v210") else pack(name, *planes)           # other values, stray bits among them
    other = np.where(keep, src, other)
    assert (other != src).mean() > 0.1
    a = rig_for(S, name)
    b = rig_for(S, name, src=other)
    all_batched(b, rects)
    first, second = a.run(rects), b.run(rects)
    check_list(first, want, rects, name, DW, "source")
    for k, (x, y) in enumerate(zip(first, second)):
        assert_bytes(y, x, "%s item %d with every byte outside the union replaced" % (name, k))


# ---- 6. several atlases ----
@pytest.mark.parametrize("name", ["y210", "v210"])
def test_split_atlas_is_byte_identical(srcnn, oracle_lib, name):
    S = srcnn
    want = whole(oracle_lib, name)
    rig = rig_for(S, name)
    rects = snapped(seeded_rects(64001, 64) + [(0, 0, 60, 50), (DW - 72, DH - 30, 72, 30)], name, DW)
    one = rig.run(rects)
    check_list(one, want, rects, name, DW, "one atlas")
    prev = S.lib().srcnn_set_workspace_limit(1 << 20)
    try:
        p = rig.plan(rects)
        assert p.atlases >= 2 and p.batched_items + p.single_items == len(rects), (p.atlases, p.batched_items, p.single_items)
        split = rig.run(rects)
    finally:
        S.lib().srcnn_set_workspace_limit(prev)
    for k, (a, b) in enumerate(zip(split, one)):
        assert_bytes(a, b, "%s split atlas, item %d" % (name, k))


# ---- 7. calls back to back ----
def test_three_lists_back_to_back_on_one_stream(srcnn, oracle_lib):
    S = srcnn
    name = "y416"
    want = whole(oracle_lib, name)
    rig = rig_for(S, name)
    a = snapped(seeded_rects(71, 48), name, DW)
    b = snapped(seeded_rects(72, 30, hi=25) + [(0, 0, DW, 5), (DW - 9, 0, 9, DH)], name, DW)
    st = S.Stream()
    try:
        qa = rig.queue(a, st)
        qb = rig.queue(b, st)              # (no sync in between: each call has its own descriptor slot)
        qc = rig.queue(a[::-1], st)
        st.sync()
        check_list(rig.fetch(*qa), want, a, name, DW, "first of three calls")
        check_list(rig.fetch(*qb), want, b, name, DW, "second of three calls")
        check_list(rig.fetch(*qc), want, a[::-1], name, DW, "third of three calls")
    finally:
        st.destroy()


# ---- 8. every filter at 2x, and other ratios: whichever route the plan reports ----
@pytest.mark.parametrize("filt", range(5), ids=FILTER_NAMES)
def test_every_filter(srcnn, oracle_lib, filt):
    name = NAMES[2 * filt + 1]             # uyvy, y210, y216, y410, v210
    case = (W, H, filt, 2.0)
    want = whole(oracle_lib, name, case)
    rig = rig_for(srcnn, name, case)
    rects = snapped(seeded_rects(80 + filt, 16) + [(0, 0, DW, DH), (0, 0, 6, 1), (DW - 6, DH - 1, 6, 1)], name, DW)
    all_batched(rig, rects)
    check_list(rig.run(rects), want, rects, name, DW, FILTER_NAMES[filt])


@pytest.mark.parametrize("w,h,mul", [(40, 31, 1.5), (50, 30, 0.75), (24, 24, 1.0), (30, 1, 1.5), (1, 9, 2.0)],
                         ids=["x1.5", "downscale", "identity", "kept-rows", "kept-chroma-columns"])
def test_other_ratios(srcnn, oracle_lib, w, h, mul):
    S = srcnn
    dw, dh = S.output_size(w, h, mul)
    for name in ("yuy2", "y410", "v210") if w % 20 else ("y212", "vuya", "v210"):
        cw, dcw = S_ccols(name, w), S_ccols(name, dw)
        up, down = dw > w and dh > h, dw < w and dh < h
        chroma_up = dcw > cw and dh > h
        src = pack(name, *frame_planes(name, w, h, 100 * w + h))
        if (up and chroma_up) or (down and dcw < cw):
            want = whole(oracle_lib, name, (w, h, 2, mul))
        else:                              # the identity size and kept axes: the library's own whole frame (srcnn_yuv_packed_upscale_dev)
            want = S.yuv_packed_upscale(src, name, w, multiply=mul, filt=2)
        rig = rig_for(S, name, (w, h, 2, mul), src=src)
        rects = snapped(seeded_rects(90 + w, 24, dw, dh, hi=30) + [(0, 0, 1, 1), (dw - 1, dh - 1, 1, 1), (0, 0, dw, dh), (0, dh // 2, dw, 1), (dw // 2, 0, 1, dh)],
                        name, dw)
        p = rig.plan(rects)
        if up and chroma_up:
            assert (w, h, mul) == (40, 31, 1.5) or UNIT[name] == 1
            assert p.batched_items == len(rects), (name, p.batched_items, p.single_items)
        else:
            assert p.single_items == len(rects) and p.atlases == 0, name
        if (w, h) == (1, 9):
            assert up and (chroma_up == (UNIT[name] == 1))        # luma grows; the 4:2:2 chroma columns keep their number
        check_list(rig.run(rects), want, rects, name, dw, "%dx%d x%g" % (w, h, mul))


def S_ccols(name, w):
    return w if UNIT[name] == 1 else (w + 1) // 2


# ---- 9. mixed routes in one list ----
def find_refused_shape(S, name, w, h, mul, filt, dw, dh):
    """A small rect the Y list batches and the chroma tile predicate refuses, if a seeded search over this frame finds one."""
    for r in snapped(seeded_rects(4711, 200, dw, dh, hi=60), name, dw):
        if S.yuv_packed_upscale_rect_list_plan(name, w, h, mul, filt, [r]).single_items == 1 and \
                S.y_path_rect_list_plan(w, h, dw, dh, filt, [r[:4]]).batched_items == 1:
            return r
    return None


@pytest.mark.parametrize("name", ["yuy2", "v210"])
def test_mixed_routes_in_one_list(srcnn, oracle_lib, name):
    S = srcnn
    case = (1020, 510, 2, 2.0)             # -> 2040 x 1020: the smallest frame that holds a cell at the threshold
    w, h, filt, mul = case
    dw, dh = S.output_size(w, h, mul)
    big = (0, 0, dw, dh)                   # (2040 + 12) x (1020 + 12) = 2 117 664 samples: at or above SRCNN_RECT_LIST_SINGLE_SAMPLES = 2^21
    assert (dw, dh) == (2040, 1020) and (big[2] + 12) * (big[3] + 12) >= 2097152 and big == snapped([big], name, dw)[0]
    small = snapped(seeded_rects(5150, 12, dw, dh, hi=40) + [(dw - 6, dh - 1, 6, 1)], name, dw)
    refused = find_refused_shape(S, name, w, h, mul, filt, dw, dh)
    # (at 2x bilinear / box chroma tables every tile's patch fits: the search finds nothing, and the refused shape is covered by
    # tests/test_yuv_packed_rect_list_abi.py and tests/host/yuv_packed_rect_list_sanitize.cpp on the CPU)
    rects = small + [big] + ([refused] if refused else [])
    rig = rig_for(S, name, case)
    p = rig.plan(rects)
    assert p.batched_items == len(small) and p.single_items == len(rects) - len(small) >= 1, (p.batched_items, p.single_items)
    want = whole(oracle_lib, name, case)
    check_list(rig.run(rects), want, rects, name, dw, "mixed routes")


# ---- 10. children: the forced single route, a non-parity mode, a list under the caller's capture ----
def child(mode, env=None, timeout=600):
    r = subprocess.run([sys.executable, WORKER, mode], env=dict(os.environ, **(env or {})), capture_output=True, text=True, timeout=timeout)
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")]
    assert r.returncode == 0 and line, "yuv_packed_rect_list_worker %s: exit %d\n%s\n%s" % (mode, r.returncode, r.stdout[-600:], r.stderr[-1500:])
    return json.loads(line[0][7:])


def test_unfused_child_gives_the_same_bytes(srcnn):
    S = srcnn
    assert "SRCNN_YUV_PACKED_RECT_LIST_UNFUSED=0" in S.debug_settings()
    fast = {name: _DIGEST.get(name) or LW.main_digest(S, name) for name in NAMES}
    assert child("unfused", {"SRCNN_YUV_PACKED_RECT_LIST_UNFUSED": "1"}) == fast


def test_fast_mode_equals_the_loop_of_single_calls(srcnn):
    S = srcnn
    prev = S.set_mode(S.MODE_FAST)        # (a strict-only build refuses: conftest turns that into a skip)
    try:
        for name in ("yvyu", "y410", "v210"):
            rig = rig_for(S, name)
            rects = main_rects(name, 7)[:24]
            p = rig.plan(rects)
            assert p.single_items == len(rects) and p.batched_items == 0 and p.atlases == 0
            for k, (a, b) in enumerate(zip(rig.run(rects), rig.fetch(*rig.loop(rects)))):
                assert_bytes(a, b, "MODE_FAST %s, item %d vs the single call" % (name, k))
    finally:
        S.set_mode(prev)


def test_list_under_the_callers_capture_equals_the_loop_after_replay(srcnn):
    assert child("capture") == {name: True for name in LW.CAPTURE_NAMES}


# ---- 11. the convenience call ----
@pytest.mark.parametrize("name", ["uyvy", "y212", "y416", "v210"])
def test_numpy_convenience(srcnn, oracle_lib, name):
    S = srcnn
    want = whole(oracle_lib, name)
    rects = snapped([(0, 0, 6, 1), (36, 21, 72, 40), (DW - 6, 3, 6, 100), (102, 60, 18, 3)], name, DW)
    got = S.yuv_packed_upscale_rects(source(name, MAIN), name, W, rects)
    assert all(isinstance(a, np.ndarray) and a.dtype == np.uint8 for a in got)
    check_list(got, want, rects, name, DW, "yuv_packed_upscale_rects")
    assert S.yuv_packed_upscale_rects(source(name, MAIN), name, W, []) == []
    S.yuv_packed_upscale_rect_list_dev(name, W, H, 2.0, 2, None, 0, [])          # n == 0: nothing is looked at
