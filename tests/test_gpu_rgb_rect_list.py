"""srcnn_rgb_upscale_rect_list_dev (include/srcnn_amd_rgb_rect_list.h) byte for byte against crops of the whole image (GPU).

Every item of a list is a crop of what srcnn_rgb_upscale_dev writes, so every expectation is a crop of the whole-image
expectation -- oracle.process at depth 8, the numpy restatement of tests/test_rgb_restatement.py above it -- computed once per
image and never by the call under test; where the contract names it, results are also compared with the loop of
srcnn_rgb_upscale_rect_dev.  The image is 96 x 56 -> 192 x 112, 2x bicubic, unless said otherwise: the frame of
tests/test_gpu_rect_list.py, whose cells straddle the tile seams of the layer kernels.  Lists are seeded.  Every child process runs
under a timeout of its own and nothing is tried twice.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import rgb_rect_list_worker as RW
from rect_list_worker import DH, DW, H, W, border_rects, seeded_rects
from rgb_rect_list_worker import RgbListRig
from test_gpu_rgb import first_difference, run
from test_rgb_restatement import image, restatement

pytestmark = pytest.mark.gpu

FILTER_NAMES = ("nearest", "bilinear", "bicubic", "lanczos3", "bspline")
CANARY = 0xA5
GUARD = 1024
WORKER = os.path.join(os.path.dirname(os.path.abspath(__file__)), "rgb_rect_list_worker.py")
_WANT = {}
_DIGEST = {}


def whole(oracle_lib, alpha, depth, seed, mul=2.0, filt=2, w=W, h=H):
    """(image, (out, conv) of the whole image) in R, G, B[, A] order: computed once, read-only."""
    key = (alpha, depth, seed, mul, filt, w, h)
    if key not in _WANT:
        img = image(w, h, alpha, depth, seed)
        want = oracle_lib.process(img, mul, filt) if depth == 8 else restatement(oracle_lib, img, depth, mul, filt)
        for a in (img,) + tuple(want):
            a.setflags(write=False)
        _WANT[key] = (img, tuple(want))
    return _WANT[key]


def crop(pair, r):
    x0, y0, rw, rh = r
    return pair[0][y0:y0 + rh, x0:x0 + rw], pair[1][y0:y0 + rh, x0:x0 + rw]


def assert_pair(got, want, what):
    for name, g, e in zip(("out", "conv"), got, want):
        assert g.shape == e.shape and g.dtype == e.dtype, (what, name, g.shape, e.shape, g.dtype, e.dtype)
        assert np.array_equal(g, e), "%s %s: %s" % (what, name, first_difference(g, e))


def check_list(got, want, rects, what):
    assert len(got) == len(rects)
    for k, (g, r) in enumerate(zip(got, rects)):
        assert_pair(g, crop(want, r), "%s: item %d, rect %dx%d at (%d,%d)" % (what, k, r[2], r[3], r[0], r[1]))


def all_batched(rig, rects, atlases=None):
    p = rig.plan(rects)
    assert p.batched_items == len(rects) and p.single_items == 0, (p.batched_items, p.single_items)
    assert atlases is None or p.atlases == atlases


# ---- 1. borders ----
@pytest.mark.parametrize("layout,order,alpha,depth", [RW.BORDER_CELL, ("planar", "bgr", 1, 12)], ids=["rgb8", "planar-bgra12"])
def test_borders_vs_oracle_and_the_loop_of_single_calls(srcnn, oracle_lib, layout, order, alpha, depth):
    img, want = whole(oracle_lib, alpha, depth, RW.BORDER_SEED)
    rig = RgbListRig(srcnn, img, layout, order, depth)
    rects = border_rects()
    all_batched(rig, rects, atlases=1)
    got = rig.run(rects)
    if (layout, order, alpha, depth) == RW.BORDER_CELL:
        _DIGEST["borders"] = RW.digest(got)
    check_list(got, want, rects, "borders vs the whole image")
    for k, (g, s) in enumerate(zip(got, rig.loop(rects))):
        assert_pair(g, s, "borders: item %d vs the single call" % k)


# ---- 2. every kernel instantiation on the batched route ----
CELLS = [(layout, ("rgb", "bgr")[k % 2], alpha, depth)
         for k, (layout, alpha, depth) in enumerate((lay, a, d) for lay in ("interleaved", "planar") for a in (0, 1) for d in (8, 12))]
CELLS += [("interleaved", "bgr", 0, 10), ("planar", "rgb", 1, 16)]
assert len({(c[0], c[2], c[3] == 8) for c in CELLS[:8]}) == 8 and {c[1] for c in CELLS} == {"rgb", "bgr"}


@pytest.mark.parametrize("layout,order,alpha,depth", CELLS, ids=["%s-%s-a%d-%d" % c for c in CELLS])
def test_every_format_cell_on_the_batched_route(srcnn, oracle_lib, layout, order, alpha, depth):
    img, want = whole(oracle_lib, alpha, depth, 100 + depth)
    rig = RgbListRig(srcnn, img, layout, order, depth)
    rects = seeded_rects(200 + CELLS.index((layout, order, alpha, depth)), 32) + [(0, 0, DW, DH)]
    all_batched(rig, rects)
    check_list(rig.run(rects), want, rects, "%s %s alpha=%d %d-bit" % (layout, order, alpha, depth))


# ---- 3. many small rects repainted in place ----
def test_repaint_inside_one_full_size_image(srcnn, oracle_lib):
    S = srcnn
    img, want = whole(oracle_lib, 0, 8, RW.BORDER_SEED)
    rig = RgbListRig(S, img, "interleaved", "rgb", 8)
    rects = seeded_rects(64001, 64)
    all_batched(rig, rects)
    full = S.DeviceBuffer.from_numpy(np.full(3 * DW * DH, CANARY, np.uint8))
    conv = S.DeviceBuffer.from_numpy(np.full(DW * DH, CANARY, np.uint8))
    bases = [full.ptr + 3 * (y0 * DW + x0) for (x0, y0, _, _) in rects]
    assert any(b % 4 == 0 for b in bases) and any(b % 4 for b in bases)        # both store paths run
    assert {b % 4 for b in bases} == {0, 1, 2, 3}
    S.rgb_upscale_rect_list_dev(rig.fmt, W, H, 2.0, 2, rig.src, None,
                                [(x0, y0, rw, rh, [(full, 3 * (y0 * DW + x0))], [3 * DW], (conv, y0 * DW + x0), DW) for (x0, y0, rw, rh) in rects])
    S.sync()
    got, got_conv = full.to_numpy(np.uint8, (DH, DW, 3)), conv.to_numpy(np.uint8, (DH, DW))
    painted = np.zeros((DH, DW), bool)
    for (x0, y0, rw, rh) in rects:
        painted[y0:y0 + rh, x0:x0 + rw] = True
    assert 0.2 < painted.mean() < 1.0                      # overlaps happen, and so does untouched ground
    assert np.array_equal(got[painted], want[0][painted]), "painted pixels differ from the whole image"
    assert np.array_equal(got_conv[painted], want[1][painted]), "painted Y' samples differ from the whole image"
    assert np.all(got[~painted] == CANARY) and np.all(got_conv[~painted] == CANARY), "bytes outside the rects were written"


# ---- 4. pitches and guard bands ----
def test_pitched_guarded_destinations_and_optional_conv(srcnn, oracle_lib):
    S = srcnn
    img, want = whole(oracle_lib, 1, 12, RW.BORDER_SEED)
    rig = RgbListRig(S, img, "planar", "bgr", 12)
    rects = [(9, 7, 37, 11), (0, 0, DW, 9), (DW - 9, DH - 10, 9, 10), (50, 20, 3, 5), (64, 33, 1, 4), (20, 16, 64, 16), (0, 40, 8, 8), (100, 0, 12, 40)]
    all_batched(rig, rects)
    items, spans, pos = [], [], 0

    def place(k, rw, rh):
        nonlocal pos
        row = 2 * rw
        pitch = (row + 3) // 4 * 4 + 8 if k % 2 == 0 else row + 2 + (2 if (row + 2) % 4 == 0 else 0)     # rows equally aligned / rotating
        assert pitch > row and pitch % 2 == 0 and (k % 2 == 0) == (pitch % 4 == 0)
        start = (pos + GUARD + 3) // 4 * 4 + 2 * ((k // 2) % 2)                                        # 4-byte aligned, or only 2-byte aligned
        pos = start + pitch * (rh - 1) + row
        return start, pitch
    for k, (x0, y0, rw, rh) in enumerate(rects):
        planes = [place(k, rw, rh) for _ in range(4)]
        cv = place(k, rw, rh) if k % 2 == 0 else None                                                  # dst_conv is NULL for every other item
        spans.append((planes, cv))
    total = pos + GUARD
    buf = S.DeviceBuffer.from_numpy(np.full(total, CANARY, np.uint8))
    for (x0, y0, rw, rh), (planes, cv) in zip(rects, spans):
        items.append((x0, y0, rw, rh, [(buf, s) for (s, _) in planes], [p for (_, p) in planes], (buf, cv[0]) if cv else None, cv[1] if cv else 0))
    S.rgb_upscale_rect_list_dev(rig.fmt, W, H, 2.0, 2, rig.src, None, items)
    S.sync()
    raw = buf.to_numpy(np.uint8, (total,))

    def take(start, pitch, rw, rh):
        got = np.empty((rh, rw), np.uint16)
        for r in range(rh):
            a = start + r * pitch
            got[r] = raw[a:a + 2 * rw].view(np.uint16)
            raw[a:a + 2 * rw] = CANARY
        return got
    for k, ((x0, y0, rw, rh), (planes, cv)) in enumerate(zip(rects, spans)):
        out = RW.canonical(np.stack([take(s, p, rw, rh) for (s, p) in planes]), "planar", "bgr")
        e_out, e_conv = crop(want, rects[k])
        assert np.array_equal(out, e_out), "pitched item %d: %s" % (k, first_difference(out, e_out))
        if cv:
            assert np.array_equal(take(cv[0], cv[1], rw, rh), e_conv), "pitched item %d, conv" % k
    touched = np.flatnonzero(raw != CANARY)          # (an item without dst_conv has no conv region at all: anything it wrote there shows here)
    assert touched.size == 0, "%d padding / guard bytes written, first at %d" % (touched.size, int(touched[0]))


# ---- 5. source rectangle ----
@pytest.mark.parametrize("layout,order,alpha,depth", [("interleaved", "rgb", 0, 8), ("planar", "bgr", 1, 12)], ids=["rgb8", "planar-bgra12"])
def test_nothing_outside_the_union_of_the_source_rectangles_is_read(srcnn, oracle_lib, layout, order, alpha, depth):
    S = srcnn
    img, want = whole(oracle_lib, alpha, depth, RW.BORDER_SEED)
    rects = [(0, 0, 9, 9), (DW - 9, DH - 9, 9, 9), (90, 50, 1, 1), (40, 0, 30, 12), (0, 70, 7, 20)] + seeded_rects(77, 6, hi=20)
    other = img ^ np.random.default_rng(31337).integers(1, 256, img.shape).astype(img.dtype)      # other random values: every sample differs
    keep = np.zeros((H, W), bool)
    for r in rects:
        sx0, sy0, sw, sh = S.rgb_rect_source(W, H, 2.0, 2, *r)
        keep[sy0:sy0 + sh, sx0:sx0 + sw] = True
    other[keep] = img[keep]
    assert np.any(other != img, axis=2).mean() > 0.2          # the test has teeth: a good part of the image is something else
    rig = RgbListRig(S, other, layout, order, depth)
    all_batched(rig, rects)
    check_list(rig.run(rects), want, rects, "altered source")


# ---- 6. several atlases ----
def test_split_atlas_is_byte_identical(srcnn, oracle_lib):
    S = srcnn
    img, want = whole(oracle_lib, 1, 8, 640)
    rig = RgbListRig(S, img, "interleaved", "bgr", 8)
    rects = seeded_rects(64001, 64) + [(0, 0, 60, 50), (DW - 70, DH - 30, 70, 30)]
    one = rig.run(rects)
    check_list(one, want, rects, "one atlas")
    prev = S.lib().srcnn_set_workspace_limit(1 << 20)
    try:
        p = rig.plan(rects)
        assert p.atlases >= 3 and p.batched_items + p.single_items == len(rects), (p.atlases, p.batched_items, p.single_items)
        split = rig.run(rects)
    finally:
        S.lib().srcnn_set_workspace_limit(prev)
    for k, (a, b) in enumerate(zip(split, one)):
        assert_pair(a, b, "split atlas, item %d" % k)


# ---- 7. calls back to back ----
def test_three_lists_back_to_back_on_one_stream(srcnn, oracle_lib):
    S = srcnn
    img, want = whole(oracle_lib, 0, 8, RW.BORDER_SEED)
    rig = RgbListRig(S, img, "interleaved", "rgb", 8)
    a, b = seeded_rects(71, 48), border_rects()[:30] + seeded_rects(72, 9, hi=25)
    st = S.Stream()
    try:
        qa = rig.queue(a, st)
        qb = rig.queue(b, st)              # (no sync in between: each call has its own descriptor slot)
        qc = rig.queue(a[::-1], st)
        st.sync()
        check_list(rig.fetch(a, *qa), want, a, "first of three calls")
        check_list(rig.fetch(b, *qb), want, b, "second of three calls")
        check_list(rig.fetch(a[::-1], *qc), want, a[::-1], "third of three calls")
    finally:
        st.destroy()


# ---- 8. every filter at 2x ----
@pytest.mark.parametrize("filt", range(5), ids=FILTER_NAMES)
def test_every_filter(srcnn, oracle_lib, filt):
    img, want = whole(oracle_lib, 1, 8, 880, filt=filt)
    rig = RgbListRig(srcnn, img, "planar", "rgb", 8, filt=filt)
    rects = border_rects()[:12] + seeded_rects(80 + filt, 8) + [(0, 0, DW, DH)]
    all_batched(rig, rects)
    check_list(rig.run(rects), want, rects, FILTER_NAMES[filt])


# ---- 9. other ratios: whichever route the plan reports ----
# the source shapes of test_other_ratios in tests/test_gpu_rect_list.py; one multiplier serves both axes here, so the axis that
# keeps its size is one of a single row (30 x 1 -> 45 x 1)
@pytest.mark.parametrize("w,h,mul", [(40, 31, 1.5), (50, 30, 0.75), (24, 24, 1.0), (30, 1, 1.5)], ids=["x1.5", "downscale", "identity", "identity-axis"])
def test_other_ratios(srcnn, oracle_lib, w, h, mul):
    S = srcnn
    dw, dh = S.output_size(w, h, mul)
    layout, order, alpha, depth = ("interleaved", "bgr", 1, 8) if w % 20 else ("planar", "rgb", 0, 12)
    if dw > w and dh > h or (dw < w and dh < h):
        img, want = whole(oracle_lib, alpha, depth, 520 + w, mul=mul, w=w, h=h)
    else:                                  # the identity size and kept axes: the library's own whole image (srcnn_rgb_upscale_dev)
        img = image(w, h, alpha, depth, 520 + w)
        want = run(S, img, layout, order, depth, mul, 2)
    rig = RgbListRig(S, img, layout, order, depth, mul=mul)
    rects = seeded_rects(90 + w, 24, dw, dh, hi=30) + [(0, 0, 1, 1), (dw - 1, dh - 1, 1, 1), (0, 0, dw, dh), (0, dh // 2, dw, 1), (dw // 2, 0, 1, dh)]
    p = rig.plan(rects)
    if dw > w and dh > h:
        assert p.batched_items == len(rects)
    else:
        assert p.single_items == len(rects) and p.atlases == 0
    check_list(rig.run(rects), want, rects, "%dx%d x%g" % (w, h, mul))


# ---- 10. the forced single route ----
def child(mode, env=None, timeout=600):
    r = subprocess.run([sys.executable, WORKER, mode], env=dict(os.environ, **(env or {})), capture_output=True, text=True, timeout=timeout)
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")]
    assert r.returncode == 0 and line, "rgb_rect_list_worker %s: exit %d\n%s\n%s" % (mode, r.returncode, r.stdout[-600:], r.stderr[-1500:])
    return json.loads(line[0][7:])


def test_unfused_child_gives_the_same_bytes(srcnn):
    S = srcnn
    assert "SRCNN_RGB_RECT_LIST_UNFUSED=0" in S.debug_settings()
    fast = _DIGEST.get("borders") or RW.border_digest(S)
    assert child("unfused", {"SRCNN_RGB_RECT_LIST_UNFUSED": "1"}) == {"borders": fast}


# ---- 11. a non-parity mode: the list is the loop ----
def test_fast_mode_equals_the_loop_of_single_calls(srcnn):
    S = srcnn
    prev = S.set_mode(S.MODE_FAST)        # (a strict-only build refuses: conftest turns that into a skip)
    try:
        rig = RgbListRig(S, image(W, H, 1, 12, 1212), "planar", "bgr", 12)
        rects = border_rects()[:20] + seeded_rects(99, 12)
        p = rig.plan(rects)
        assert p.single_items == len(rects) and p.batched_items == 0 and p.atlases == 0
        for k, (a, b) in enumerate(zip(rig.run(rects), rig.loop(rects))):
            assert_pair(a, b, "MODE_FAST, item %d vs the single call" % k)
    finally:
        S.set_mode(prev)


# ---- 12. the convenience calls ----
def test_numpy_convenience(srcnn, oracle_lib):
    S = srcnn
    rects = [(0, 0, 1, 1), (33, 21, 70, 40), (DW - 5, 3, 5, 100), (100, 60, 17, 3)]
    img, want = whole(oracle_lib, 0, 8, RW.BORDER_SEED)
    got = S.rgb_upscale_rects(img, rects, want_conv=True)
    check_list(got, want, rects, "rgb_upscale_rects, (h, w, 3) uint8")
    for g, r in zip(S.rgb_upscale_rects(img, rects), rects):
        assert isinstance(g, np.ndarray) and np.array_equal(g, crop(want, r)[0])
    img, want = whole(oracle_lib, 1, 12, RW.BORDER_SEED)
    got = S.rgb_upscale_rects(RW.arrange(img, "planar", "bgr"), rects, layout="planar", order="bgr", depth=12, want_conv=True)
    check_list([(RW.canonical(o, "planar", "bgr"), c) for (o, c) in got], want, rects, "rgb_upscale_rects, (4, h, w) 12-bit BGRA")
    assert S.rgb_upscale_rects(img, []) == []
    S.rgb_upscale_rect_list_dev(S.rgb_format(), W, H, 2.0, 2, None, None, [])          # n == 0: nothing is looked at


def test_torch_repaint_vs_oracle(oracle_lib):
    res = child("torch")
    if "skip" in res:
        pytest.skip(res["skip"])
    rects = RW.torch_rects()
    painted = np.zeros((DH, DW), bool)
    for (x0, y0, rw, rh) in rects:
        painted[y0:y0 + rh, x0:x0 + rw] = True
    assert 0 < painted.mean() < 1
    _, want = whole(oracle_lib, 0, 8, 31)
    full = np.full((DH, DW, 3), CANARY, np.uint8)
    full[painted] = want[0][painted]
    assert res["hwc"]["same"] and res["hwc"]["sha"] == RW.digest([(full,)]), "(H, W, 3) uint8: rects repainted, the rest untouched"
    _, want = whole(oracle_lib, 1, 12, 32)
    wide = np.full((4, DH, DW + 6), 0x5A5A, np.uint16)
    bgra = want[0][..., [2, 1, 0, 3]].transpose(2, 0, 1)
    wide[:, :, :DW][:, painted] = bgra[:, painted]
    assert res["chw"]["sha"] == RW.digest([(wide,)]), "(4, H, W) 12-bit BGRA in a row-padded image"
    assert res["empty"]["sha"] == res["chw"]["sha"], "n == 0 touched the image"
    assert res["refused"] == [True, True, True]
