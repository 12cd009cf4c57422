"""srcnn_y_path_rect_list_f32_dev (include/srcnn_amd_rect_list.h) bit for bit against the oracle's whole frame (GPU).

Every item of a list is a crop of the whole-frame result, so every expectation is a crop of oracle.y_path of the whole frame,
computed once per frame -- and, where the contract says so, the loop of single rect calls.  The frame is 96 x 56 -> 192 x 112,
2x bicubic, unless said otherwise: three tile columns and seven tile rows of the layer kernels, so the cells of an atlas straddle
the tile seams of both.  Lists are seeded (fixed seeds: the plan test on the CPU uses the same lists).
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import rect_list_worker as RW
from conftest import assert_bit_equal
from libsrcnn_amd import synth
from rect_list_worker import DH, DW, H, W, ListRig, border_rects, seeded_rects

pytestmark = pytest.mark.gpu

FILTER_NAMES = ("nearest", "bilinear", "bicubic", "lanczos3", "bspline")
CANARY = 0xA5
GUARD = 4096
WORKER = os.path.join(os.path.dirname(os.path.abspath(__file__)), "rect_list_worker.py")
_DIGEST = {}


@pytest.fixture(scope="module")
def frame(srcnn, oracle_lib):
    class F:
        y = RW.frame_plane()
        want = oracle_lib.y_path(y)
    assert F.want.shape == (DH, DW)
    F.want.setflags(write=False)
    return F


def crop(want, r):
    x0, y0, rw, rh = r
    return want[y0:y0 + rh, x0:x0 + rw]


def check_list(got, want, rects, what):
    assert len(got) == len(rects)
    for k, (g, r) in enumerate(zip(got, rects)):
        assert_bit_equal(g, crop(want, r), "%s: item %d, rect %dx%d at (%d,%d)" % (what, k, r[2], r[3], r[0], r[1]))


# ---- borders ----
def test_borders_vs_oracle_and_the_loop_of_single_calls(srcnn, frame):
    rig = ListRig(srcnn, frame.y, DW, DH)
    rects = border_rects()
    p = rig.plan(rects)
    assert p.batched_items == len(rects) and p.single_items == 0 and p.atlases == 1
    got = rig.run(rects)
    _DIGEST["borders"] = RW.digest(got)
    check_list(got, frame.want, rects, "borders vs oracle")
    for k, (g, s) in enumerate(zip(got, rig.loop(rects))):
        assert_bit_equal(g, s, "borders: item %d vs the single call" % k)


# ---- many small rects repainted in place ----
def test_many_small_rects_repaint_one_plane(srcnn, frame):
    S = srcnn
    rig = ListRig(S, frame.y, DW, DH)
    rects = seeded_rects(64001, 64)
    assert rig.plan(rects).batched_items == 64
    plane = S.DeviceBuffer.from_numpy(np.full(4 * DW * DH, CANARY, np.uint8))
    S.y_path_rect_list_dev(rig.din, 0, W, H, DW, DH, 2, [(x0, y0, rw, rh, (plane, 4 * (y0 * DW + x0)), 4 * DW) for (x0, y0, rw, rh) in rects])
    S.sync()
    raw = plane.to_numpy(np.uint8, (DH, 4 * DW))
    painted = np.zeros((DH, DW), bool)
    for (x0, y0, rw, rh) in rects:
        painted[y0:y0 + rh, x0:x0 + rw] = True
    assert 0.2 < painted.mean() < 1.0                      # overlaps happen, and so does untouched ground
    got = raw.view(np.float32)
    assert np.array_equal(got.view(np.uint32)[painted], np.ascontiguousarray(frame.want).view(np.uint32)[painted]), "painted samples differ from the whole frame"
    rest = raw.reshape(DH, DW, 4)[~painted]
    assert np.all(rest == CANARY), "%d bytes outside the rects were written" % int(np.count_nonzero(rest != CANARY))


# ---- pitches and guard bands ----
def test_pitched_source_and_guarded_pitched_destinations(srcnn, frame):
    S = srcnn
    rig = ListRig(S, frame.y, DW, DH, pad_cols=5)
    rects = [(9, 7, 37, 11), (0, 0, DW, 9), (DW - 9, DH - 10, 9, 10), (50, 20, 3, 5), (64, 33, 1, 4), (20, 16, 64, 16), (0, 40, 8, 8), (100, 0, 12, 40)]
    items, spans, pos = [], [], 0
    for k, (x0, y0, rw, rh) in enumerate(rects):
        base_off = 4 * (k % 4)                                 # 16-byte aligned, and only 4-byte aligned in three ways
        pitch = (4 * rw + 15) // 16 * 16 + 32 if k % 2 == 0 else 4 * (rw + 1) + (4 - 4 * (rw + 1)) % 16      # rows equally aligned / rotating
        assert pitch > 4 * rw and pitch % 4 == 0
        start = pos + GUARD + base_off
        items.append((x0, y0, rw, rh, start, pitch))
        spans.append((start, pitch))
        pos = (start + pitch * (rh - 1) + 4 * rw + 15) & ~15
    total = pos + GUARD
    buf = S.DeviceBuffer.from_numpy(np.full(total, CANARY, np.uint8))
    S.y_path_rect_list_dev(rig.din, rig.in_pitch, W, H, DW, DH, 2, [(x0, y0, rw, rh, (buf, o), p) for (x0, y0, rw, rh, o, p) in items])
    S.sync()
    raw = buf.to_numpy(np.uint8, (total,))
    for k, ((x0, y0, rw, rh), (start, pitch)) in enumerate(zip(rects, spans)):
        got = np.empty((rh, rw), np.float32)
        for r in range(rh):
            a = start + r * pitch
            got[r] = raw[a:a + 4 * rw].view(np.float32)
            raw[a:a + 4 * rw] = CANARY
        assert_bit_equal(got, crop(frame.want, rects[k]), "pitched item %d (pitch %d, base +%d)" % (k, pitch, start % 16))
    touched = np.flatnonzero(raw != CANARY)
    assert touched.size == 0, "%d padding / guard bytes written, first at %d" % (touched.size, int(touched[0]))


# ---- n = 1 ----
def test_a_list_of_one_equals_the_single_call(srcnn, frame):
    rig = ListRig(srcnn, frame.y, DW, DH)
    for r in ((33, 21, 70, 40), (0, 0, 1, 1), (DW - 5, 3, 5, 100), (0, 0, DW, DH)):
        got, single = rig.run([r]), rig.loop([r])
        assert_bit_equal(got[0], single[0], "n = 1, rect %r vs the single call" % (r,))
        assert_bit_equal(got[0], crop(frame.want, r), "n = 1, rect %r vs oracle" % (r,))


def test_numpy_convenience(srcnn, frame):
    rects = [(0, 0, 1, 1), (33, 21, 70, 40), (DW - 5, 3, 5, 100), (100, 60, 17, 3)]
    check_list(srcnn.y_path_rects(frame.y, DW, DH, 2, rects), frame.want, rects, "y_path_rects")
    assert srcnn.y_path_rects(frame.y, DW, DH, 2, []) == []


# ---- source rectangle ----
def test_nothing_outside_the_union_of_the_source_rectangles_is_read(srcnn, frame):
    S = srcnn
    rects = [(0, 0, 9, 9), (DW - 9, DH - 9, 9, 9), (90, 50, 1, 1), (40, 0, 30, 12), (0, 70, 7, 20)] + seeded_rects(77, 6, hi=20)
    poisoned = np.full_like(frame.y, np.nan)
    for r in rects:
        sx0, sy0, sw, sh = S.y_path_rect_source(W, H, DW, DH, 2, *r)
        poisoned[sy0:sy0 + sh, sx0:sx0 + sw] = frame.y[sy0:sy0 + sh, sx0:sx0 + sw]
    assert np.isnan(poisoned).mean() > 0.2                 # the test has teeth: a good part of the plane is poison
    rig = ListRig(S, poisoned, DW, DH)
    assert rig.plan(rects).batched_items == len(rects)
    check_list(rig.run(rects), frame.want, rects, "poisoned source")


# ---- several atlases ----
def test_split_atlas_is_bit_identical(srcnn, frame):
    S = srcnn
    rig = ListRig(S, frame.y, DW, DH)
    rects = seeded_rects(64001, 64) + [(0, 0, 60, 50), (DW - 70, DH - 30, 70, 30)]
    whole = rig.run(rects)
    check_list(whole, frame.want, rects, "one atlas")
    prev = S.lib().srcnn_set_workspace_limit(1 << 20)
    try:
        p = rig.plan(rects)
        assert p.atlases >= 3 and p.batched_items + p.single_items == len(rects), (p.atlases, p.batched_items, p.single_items)
        split = rig.run(rects)
    finally:
        S.lib().srcnn_set_workspace_limit(prev)
    for k, (a, b) in enumerate(zip(split, whole)):
        assert_bit_equal(a, b, "split atlas, item %d" % k)


# ---- two calls back to back ----
def test_two_lists_back_to_back_on_one_stream(srcnn, frame):
    S = srcnn
    rig = ListRig(S, frame.y, DW, DH)
    a, b = seeded_rects(71, 48), border_rects()[:30] + seeded_rects(72, 9, hi=25)
    st = S.Stream()
    try:
        qa = rig.queue(a, st)
        qb = rig.queue(b, st)              # (no sync in between: each call has its own descriptor slot)
        qc = rig.queue(a[::-1], st)
        st.sync()
        check_list(rig.fetch(a, *qa), frame.want, a, "first of three calls")
        check_list(rig.fetch(b, *qb), frame.want, b, "second of three calls")
        check_list(rig.fetch(a[::-1], *qc), frame.want, a[::-1], "third of three calls")
    finally:
        st.destroy()


# ---- six calls of the four surfaces back to back: the staging ring of the stream wraps ----
RING_FRAME = (48, 36, 96, 72)


def ring_rects(k):
    """The list of call k: a rect at the origin corner, one that touches the far corner and an interior one, none larger than
    24 x 16, origins and widths even (YUY2's unit, 4:2:0's origin rule), different for every k."""
    _w, _h, dw, dh = RING_FRAME
    return [(0, 0, 24 - 2 * k, 16 - 2 * k),
            (dw - 8 - 2 * k, dh - 6 - 2 * k, 8 + 2 * k, 6 + 2 * k),
            (20 + 4 * k, 10 + 2 * k, 12 + 2 * k, 15 - k)]


def ring_surfaces(S):
    """Per surface: (rig, layout(rects) -> (lay, bytes), submit(rects, buf, lay, stream), fetch(rects, buf, lay), loop(rects));
    fetch and loop give one entry per item.  The destination buffers are the caller's, so that nothing but the list calls
    themselves happens between the first and the last of them."""
    from rgb_rect_list_worker import RgbListRig
    from test_gpu_yuv_ex import frame as yuv_frame
    from test_rgb_restatement import image
    from yuv_packed_rect_list_worker import PackedListRig, source
    from yuv_rect_list_worker import YuvListRig
    w, h, dw, dh = RING_FRAME
    y = ListRig(S, synth.plane(h, w, synth.SEED0 + 540, "noise"), dw, dh)
    rgb = RgbListRig(S, image(w, h, 0, 8, 541), "interleaved", "rgb", 8)
    yuv = YuvListRig(S, *yuv_frame(w, h, "420", 8, 542), "planar", "420", 8, 0, 2.0, 2)
    pk = PackedListRig(S, "yuy2", source("yuy2", (w, h, 2, 2.0)), w)
    assert (rgb.dw, rgb.dh) == (dw, dh) and (pk.dw, pk.dh) == (dw, dh)

    def y_submit(rects, buf, offs, st):
        S.y_path_rect_list_dev(y.din, y.in_pitch, w, h, dw, dh, 2, [(x0, y0, rw, rh, (buf, o), 0) for (x0, y0, rw, rh), o in zip(rects, offs)], st)

    def rgb_submit(rects, buf, offs, st):
        items = [(x0, y0, rw, rh, rgb.dst_of(buf, oi, rw, rh), None, (buf, oc), 0) for (x0, y0, rw, rh), (oi, oc) in zip(rects, offs)]
        S.rgb_upscale_rect_list_dev(rgb.fmt, w, h, 2.0, 2, rgb.src, None, items, st)

    def yuv_submit(rects, buf, lay, st):
        items = [(x0, y0, rw, rh, [(buf, o) for o, _ in one], None) for (x0, y0, rw, rh), one in zip(rects, lay)]
        S.yuv_upscale_rect_list_dev(yuv.fmt, w, h, 2.0, 2, yuv.din + yuv.pad, None, items, st)

    def pk_submit(rects, buf, offs, st):
        S.yuv_packed_upscale_rect_list_dev("yuy2", w, h, 2.0, 2, pk.din, 0, pk.items(rects, buf, offs), st)

    return {"y": (y, y.layout, y_submit, y.fetch, y.loop),
            "rgb": (rgb, rgb.layout_of, rgb_submit, rgb.fetch, rgb.loop),
            "i420": (yuv, yuv.layout_of, yuv_submit, lambda rects, buf, lay: yuv.fetch_raw(buf, lay), yuv.raw_loop),
            "yuy2": (pk, pk.layout, pk_submit, pk.fetch, lambda rects: pk.fetch(*pk.loop(rects)))}


def test_six_lists_of_four_surfaces_back_to_back_wrap_the_staging_ring(srcnn):
    """Y, RGB, I420, YUY2, Y, RGB on one stream without a synchronisation in between: the lists share the stream's descriptor
    table and its ring of four staging slots, so the fifth call takes the first call's slot again and waits for its event.
    Every item equals the single rect call run afterwards, byte for byte, and every item went the batched route."""
    S = srcnn
    prev = S.set_mode(S.MODE_STRICT)
    st = S.Stream()
    try:
        surf = ring_surfaces(S)
        calls = []
        for k, name in enumerate(("y", "rgb", "i420", "yuy2", "y", "rgb")):
            rig, layout, submit, fetch, loop = surf[name]
            rects = ring_rects(k)
            assert all(rw <= 24 and rh <= 16 and x0 % 2 == 0 and y0 % 2 == 0 and rw % 2 == 0 for (x0, y0, rw, rh) in rects)
            p = rig.plan(rects)
            assert p.batched_items == len(rects) and p.single_items == 0, (k, name, p.batched_items, p.single_items)
            lay, total = layout(rects)
            calls.append((name, rects, S.DeviceBuffer.from_numpy(np.full(total, CANARY, np.uint8)), lay))
        for name, rects, buf, lay in calls:
            surf[name][2](rects, buf, lay, st)
        st.sync()
        for k, (name, rects, buf, lay) in enumerate(calls):
            _rig, _layout, _submit, fetch, loop = surf[name]
            got, want = fetch(rects, buf, lay), loop(rects)
            assert len(got) == len(want) == len(rects)
            for j, (g, s) in enumerate(zip(got, want)):
                gs, ss = (g, s) if isinstance(g, (list, tuple)) else ((g,), (s,))
                assert len(gs) == len(ss)
                for a, b in zip(gs, ss):
                    assert a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes(), \
                        "call %d (%s), item %d, rect %r: the list and the single call differ" % (k, name, j, rects[j])
    finally:
        st.destroy()
        S.set_mode(prev)


# ---- every filter at 2x ----
@pytest.mark.parametrize("filt", range(5), ids=FILTER_NAMES)
def test_every_filter(srcnn, oracle_lib, frame, filt):
    want = frame.want if filt == 2 else oracle_lib.y_path(frame.y, DW, DH, filt)
    rig = ListRig(srcnn, frame.y, DW, DH, filt)
    rects = border_rects()[:12] + seeded_rects(80 + filt, 20) + [(0, 0, DW, DH)]
    assert rig.plan(rects).batched_items == len(rects)
    check_list(rig.run(rects), want, rects, FILTER_NAMES[filt])


# ---- other ratios: whichever route the plan reports ----
@pytest.mark.parametrize("shape", [(40, 31, 60, 46), (50, 30, 37, 20), (24, 24, 24, 24), (30, 20, 30, 40)], ids=["x1.5", "downscale", "identity", "identity-axis"])
def test_other_ratios(srcnn, oracle_lib, shape):
    from test_gpu_rect import oracle_whole
    w, h, dw, dh = shape
    y = synth.plane(h, w, synth.SEED0 + 520 + w, "noise")
    want = oracle_whole(oracle_lib, y, dw, dh, 2)
    rig = ListRig(srcnn, y, dw, dh)
    rects = seeded_rects(90 + w, 24, dw, dh, hi=30) + [(0, 0, 1, 1), (dw - 1, dh - 1, 1, 1), (0, 0, dw, dh), (0, dh // 2, dw, 1), (dw // 2, 0, 1, dh)]
    p = rig.plan(rects)
    if dw > w and dh > h:
        assert p.batched_items == len(rects)
    else:
        assert p.single_items == len(rects) and p.atlases == 0
    check_list(rig.run(rects), want, rects, "%dx%d -> %dx%d" % shape)


# ---- the forced single route ----
def test_unfused_child_gives_the_same_bytes(srcnn, frame):
    S = srcnn
    assert "SRCNN_RECT_LIST_UNFUSED=0" in S.debug_settings()
    fast = _DIGEST.get("borders") or RW.border_digest(S)
    r = subprocess.run([sys.executable, WORKER, "unfused"], env=dict(os.environ, SRCNN_RECT_LIST_UNFUSED="1"), capture_output=True, text=True, timeout=600)
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")]
    assert r.returncode == 0 and line, "rect_list_worker unfused: exit %d\n%s\n%s" % (r.returncode, r.stdout[-600:], r.stderr[-1500:])
    assert json.loads(line[0][7:]) == {"borders": fast}


# ---- a non-parity mode: the list is the loop ----
def test_fast_mode_equals_the_loop_of_single_calls(srcnn, frame):
    S = srcnn
    prev = S.set_mode(S.MODE_FAST)        # (a strict-only build refuses: conftest turns that into a skip)
    try:
        rig = ListRig(S, frame.y, DW, DH)
        rects = border_rects()[:20] + seeded_rects(99, 12)
        p = rig.plan(rects)
        assert p.single_items == len(rects) and p.atlases == 0
        for k, (a, b) in enumerate(zip(rig.run(rects), rig.loop(rects))):
            assert_bit_equal(a, b, "MODE_FAST, item %d vs the single call" % k)
    finally:
        S.set_mode(prev)
