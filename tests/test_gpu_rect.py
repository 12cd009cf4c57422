"""srcnn_y_path_rect_f32_dev (include/srcnn_amd_rect.h) bit for bit against the oracle's whole frame (GPU).

A rect is a crop of the whole-frame result, so every expectation is a crop of oracle.y_path of the whole frame (computed once
per frame) -- and, where the contract says so, of the library's own whole-frame or band call.  Rect edges sit at and next to
both borders, around the 6-sample halo and around the 16 / 64 tile sizes of the layer kernels.  Small shapes throughout; the
positions not fixed by the edge rule rotate with the session seed (conftest.rotating_seed).
"""
import numpy as np
import pytest

from conftest import assert_bit_equal, bits, rotating_seed
from libsrcnn_amd import synth

pytestmark = pytest.mark.gpu

FILTER_NAMES = ("nearest", "bilinear", "bicubic", "lanczos3", "bspline")
CANARY = 0xA5
GUARD = 4096


def seed():
    return rotating_seed("rect positions of tests/test_gpu_rect.py")


def edges(n):
    e = {0, 1, 2, 5, 6, 7, 8, 15, 16, 17, 63, 64, 65, n - 8, n - 7, n - 6, n - 5, n - 2, n - 1, n}
    return sorted(v for v in e if 0 <= v <= n)


def pairs(n):
    e = edges(n)
    return [(a, b) for a in e for b in e if a < b]


def edge_rects(dw, dh, rng, limit=None):
    """Every pair of x edges with a random pair of y edges, every pair of y edges with a random pair of x edges -- or `limit`
    of each, drawn at random.  (x0, y0, rw, rh)."""
    xs, ys = pairs(dw), pairs(dh)
    pick = lambda ps: ps if limit is None or len(ps) <= limit else [ps[k] for k in rng.choice(len(ps), limit, replace=False)]   # noqa: E731
    out = [(x, ys[rng.integers(len(ys))]) for x in pick(xs)] + [(xs[rng.integers(len(xs))], y) for y in pick(ys)]
    return [(x0, y0, x1 - x0, y1 - y0) for (x0, x1), (y0, y1) in out]


class Rig:
    """One source plane in device memory (tight, or pitched with NaN padding) and a result buffer; rect() runs one call."""

    def __init__(self, S, y, dw, dh, filt=2, pad_cols=0):
        self.S, self.dw, self.dh, self.filt = S, dw, dh, filt
        self.h, self.w = y.shape
        src = np.full((self.h, self.w + pad_cols), np.nan, np.float32)
        src[:, :self.w] = y
        self.in_pitch = 4 * (self.w + pad_cols) if pad_cols else 0
        self.din = S.DeviceBuffer.from_numpy(src)
        self.dout = S.DeviceBuffer(4 * dw * dh)

    def rect(self, x0, y0, rw, rh):
        self.S.y_path_rect_dev(self.din, self.in_pitch, self.w, self.h, self.dw, self.dh, self.filt, x0, y0, rw, rh, self.dout, 0)
        self.S.sync()
        return self.dout.to_numpy(np.float32, (rh, rw))

    def check(self, want, rects, what):
        for (x0, y0, rw, rh) in rects:
            assert_bit_equal(self.rect(x0, y0, rw, rh), want[y0:y0 + rh, x0:x0 + rw], "%s rect %dx%d at (%d,%d)" % (what, rw, rh, x0, y0))


# ---- the frame of cases 1, 5, 6 and 7: 70 x 40 -> 140 x 80, 2x bicubic; oracle and library whole frames computed once ----
@pytest.fixture(scope="module")
def frame(srcnn, oracle_lib):
    class F:
        w, h, dw, dh = 70, 40, 140, 80
        y = synth.plane(40, 70, synth.SEED0 + 401, "noise")
        want = oracle_lib.y_path(y)
        whole = srcnn.y_upscale2x(y)
    assert_bit_equal(F.whole, F.want, "whole frame vs oracle")
    F.want.setflags(write=False)
    F.whole.setflags(write=False)
    return F


def case1_rects(rng):
    rects = edge_rects(140, 80, rng)
    rects += [(77, 41, 1, 1), (0, 0, 140, 80)]
    # windows of 63, 64, 65, 127, 128, 129 columns (rect + 6 on both sides): around the 64-column tiles of both layer kernels
    rects += [(7, 9, ww - 12, 30) for ww in (63, 64, 65, 127, 128, 129)]
    # ... and cut by the left / right border (rect + 6 on one side only)
    rects += [(0, 3, ww - 6, 20) for ww in (63, 64, 65)] + [(140 - (ww - 6), 50, ww - 6, 30) for ww in (127, 128, 129)]
    return rects


def test_edges_vs_oracle_and_whole_frame(srcnn, frame):
    rng = np.random.default_rng(seed())
    rig = Rig(srcnn, frame.y, frame.dw, frame.dh)
    rects = case1_rects(rng)
    assert len(rects) >= 380
    for (x0, y0, rw, rh) in rects:
        got = rig.rect(x0, y0, rw, rh)
        what = "rect %dx%d at (%d,%d)" % (rw, rh, x0, y0)
        assert_bit_equal(got, frame.want[y0:y0 + rh, x0:x0 + rw], what + " vs oracle")
        assert_bit_equal(got, frame.whole[y0:y0 + rh, x0:x0 + rw], what + " vs the library's whole frame")


# ---- every pass order and filter ----
def oracle_whole(oracle_lib, y, dw, dh, filt):
    """The oracle's whole frame.  At the identity size the library copies the plane where the reference copies half of it
    (the one deliberate deviation, pinned by tests/test_gpu_parity.py::test_identity_size_deviation_is_pinned): there the
    expectation is the oracle's three layers on the plane itself, as in that test."""
    if (dh, dw) == y.shape:
        return oracle_lib.conv3(oracle_lib.conv2(oracle_lib.conv1(y)))
    return oracle_lib.y_path(y, dw, dh, filt)


SHAPES = [(40, 31, 60, 46), (50, 30, 37, 20), (33, 20, 66, 15), (20, 33, 15, 66), (24, 24, 24, 24), (30, 20, 30, 40), (1, 17, 2, 34),
          (17, 1, 34, 2)]


@pytest.mark.parametrize("filt", range(5), ids=FILTER_NAMES)
def test_pass_orders_and_filters(srcnn, oracle_lib, filt):
    rng = np.random.default_rng(seed() + filt)
    for k, (w, h, dw, dh) in enumerate(SHAPES):
        y = synth.plane(h, w, synth.SEED0 + 420 + k, "noise")
        want = oracle_whole(oracle_lib, y, dw, dh, filt)
        rects = edge_rects(dw, dh, rng, limit=20) + [(0, 0, dw, dh), (dw - 1, dh - 1, 1, 1)]
        Rig(srcnn, y, dw, dh, filt).check(want, rects, "%dx%d -> %dx%d %s" % (w, h, dw, dh, FILTER_NAMES[filt]))


# ---- pitches and guard bands ----
def pitched_rect(S, rig, x0, y0, rw, rh, pitch, base_off):
    """One call into a buffer of CANARY bytes: guard | rows of `pitch` bytes starting base_off bytes in | guard.  Returns the
    rect and the whole buffer's bytes with the rect's own bytes set back to CANARY."""
    body = base_off + pitch * (rh - 1) + 4 * rw
    total = GUARD + body + 16 + GUARD
    buf = S.DeviceBuffer.from_numpy(np.full(total, CANARY, np.uint8))
    S.y_path_rect_dev(rig.din, rig.in_pitch, rig.w, rig.h, rig.dw, rig.dh, rig.filt, x0, y0, rw, rh, (buf, GUARD + base_off), pitch)
    S.sync()
    raw = buf.to_numpy(np.uint8, (total,))
    got = np.empty((rh, rw), np.float32)
    for r in range(rh):
        a = GUARD + base_off + r * pitch
        got[r] = raw[a:a + 4 * rw].view(np.float32)
        raw[a:a + 4 * rw] = CANARY
    return got, raw


def test_pitches_padding_and_guard_bands(srcnn, frame):
    rig = Rig(srcnn, frame.y, frame.dw, frame.dh, pad_cols=5)
    cases = []
    for base_off in (0, 4, 8, 12):                       # 16-byte aligned, and only 4-byte aligned in three ways
        for (x0, y0, rw, rh) in ((9, 7, 37, 11), (0, 0, 140, 9), (131, 70, 9, 10), (50, 20, 3, 5), (64, 33, 1, 4), (20, 16, 64, 16)):
            p16 = (4 * rw + 15) // 16 * 16 + 32          # a multiple of 16 above the row: every row equally aligned
            p4 = 4 * (rw + 1) + (4 - 4 * (rw + 1)) % 16     # = 4 mod 16: the rows' alignment rotates
            assert p16 % 16 == 0 and p4 % 16 == 4 and p4 > 4 * rw
            for pitch in (p16, p4):
                cases.append((x0, y0, rw, rh, pitch, base_off))
    for (x0, y0, rw, rh, pitch, base_off) in cases:
        got, rest = pitched_rect(srcnn, rig, x0, y0, rw, rh, pitch, base_off)
        what = "rect %dx%d at (%d,%d) pitch %d base+%d" % (rw, rh, x0, y0, pitch, base_off)
        assert_bit_equal(got, frame.want[y0:y0 + rh, x0:x0 + rw], what)
        touched = np.flatnonzero(rest != CANARY)
        assert touched.size == 0, "%s: %d padding / guard bytes written, first at %d" % (what, touched.size, int(touched[0]))


# ---- source rectangle ----
@pytest.mark.parametrize("shape,filt", [((70, 40, 140, 80), 2), ((40, 31, 60, 46), 3), ((50, 30, 37, 20), 2)],
                         ids=["2x-bicubic", "lanczos3", "downscale"])
def test_nothing_outside_the_source_rectangle_is_used(srcnn, oracle_lib, shape, filt):
    S = srcnn
    w, h, dw, dh = shape
    rng = np.random.default_rng(seed() + 77)
    y = synth.plane(h, w, synth.SEED0 + 440 + filt, "noise")
    want = oracle_lib.y_path(y, dw, dh, filt)
    rects = edge_rects(dw, dh, rng, limit=6) + [(dw // 2, dh // 2, 1, 1), (0, 0, 9, 9), (dw - 9, dh - 9, 9, 9)]
    shrunk = 0
    for (x0, y0, rw, rh) in rects:
        sx0, sy0, sw, sh = S.y_path_rect_source(w, h, dw, dh, filt, x0, y0, rw, rh)
        poisoned = np.full_like(y, np.nan)
        poisoned[sy0:sy0 + sh, sx0:sx0 + sw] = y[sy0:sy0 + sh, sx0:sx0 + sw]
        shrunk += int(sw * sh < w * h)
        got = Rig(S, poisoned, dw, dh, filt).rect(x0, y0, rw, rh)
        assert_bit_equal(got, want[y0:y0 + rh, x0:x0 + rw], "poisoned source, rect %dx%d at (%d,%d), source %dx%d at (%d,%d)" %
                         (rw, rh, x0, y0, sw, sh, sx0, sy0))
    assert shrunk >= 3          # the test has teeth: most source rectangles are smaller than the plane


# ---- banding ----
def test_banded_rect_is_bit_identical(srcnn, frame):
    S = srcnn
    L = S.lib()
    rig = Rig(S, frame.y, frame.dw, frame.dh)
    limit = 1 << 20
    # the window of both rects is all 140 columns: 32 planes x 4 B x 140 x (80 + 4) rows do not fit 1 MB, 54-row bands do
    assert 32 * 4 * 140 * (80 + 4) > limit
    band_rows = limit // (32 * 4 * 140) - 4
    bands = -(-80 // band_rows)
    assert bands >= 2
    rects = [(3, 0, 134, 80), (0, 0, 139, 80)]
    unbanded = [rig.rect(*r) for r in rects]
    prev = L.srcnn_set_workspace_limit(limit)
    S.profile_enable(True)
    try:
        for r, ref in zip(rects, unbanded):
            S.profile_reset()
            got = rig.rect(*r)
            launches = S.profile_read()["conv12"][1]
            assert launches == bands, (r, launches, bands)
            assert_bit_equal(got, ref, "banded vs unbanded rect %r" % (r,))
            assert_bit_equal(got, frame.want[r[1]:r[1] + r[3], r[0]:r[0] + r[2]], "banded rect %r vs oracle" % (r,))
    finally:
        S.profile_enable(False)
        L.srcnn_set_workspace_limit(prev)


# ---- band equivalence ----
def test_full_width_rect_equals_the_band_call(srcnn, frame):
    S = srcnn
    rig = Rig(S, frame.y, frame.dw, frame.dh)
    for (row0, rows) in ((0, 80), (0, 1), (79, 1), (5, 17), (16, 48), (63, 17)):
        band = S.y_upscale2x_band(frame.y, row0, rows)
        assert_bit_equal(rig.rect(0, row0, 140, rows), band, "full-width rect rows [%d,+%d) vs band call" % (row0, rows))
        # the same rows through the window route (a padded destination keeps the rect off the band path)
        got, rest = pitched_rect(S, rig, 0, row0, 140, rows, 4 * 144, 0)
        assert_bit_equal(got, band, "full-width pitched rect rows [%d,+%d) vs band call" % (row0, rows))
        assert not np.any(rest != CANARY)


# ---- non-parity modes ----
@pytest.mark.parametrize("mode_name", ["MODE_FAST", "MODE_FAST_F16"])
def test_non_parity_modes_keep_their_tolerance(srcnn, frame, mode_name):
    from test_gpu_configs import TOL
    S = srcnn
    prev = S.set_mode(getattr(S, mode_name))        # (a strict-only build refuses: conftest turns that into a skip)
    try:
        whole = S.y_upscale2x(frame.y)
        rig = Rig(S, frame.y, frame.dw, frame.dh)
        rects = case1_rects(np.random.default_rng(seed() + 5))
        worst, same = 0.0, 0
        for (x0, y0, rw, rh) in rects:
            got = rig.rect(x0, y0, rw, rh)
            err = float(np.max(np.abs(got.astype(np.float64) - frame.want[y0:y0 + rh, x0:x0 + rw])))
            worst = max(worst, err)
            same += int(np.array_equal(bits(got), bits(whole[y0:y0 + rh, x0:x0 + rw])))
            assert err <= TOL[mode_name], (mode_name, (x0, y0, rw, rh), err)
        print("%s: %d rects, max |d| vs oracle %.3g (bound %.3g); %d of them bit-equal to the mode's whole-frame call"
              % (mode_name, len(rects), worst, TOL[mode_name], same))
    finally:
        S.set_mode(prev)


# ---- one real size ----
def test_1080p_to_4k_interior_and_corner(srcnn):
    S = srcnn
    h, w = 1080, 1920
    y = synth.plane(h, w, synth.SEED0 + 460, "smooth")
    whole = S.y_upscale2x(y)             # (held to the compiled reference by the existing suite)
    rig = Rig(S, y, 2 * w, 2 * h)
    for (x0, y0) in ((1601, 903), (3840 - 640, 2160 - 360)):
        assert_bit_equal(rig.rect(x0, y0, 640, 360), whole[y0:y0 + 360, x0:x0 + 640], "640x360 rect at (%d,%d) of 3840x2160" % (x0, y0))
