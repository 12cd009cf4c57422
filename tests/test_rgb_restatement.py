"""CPU: the numpy restatement of srcnn_rgb_upscale_dev (include/srcnn_amd_rgb.h) and the case matrix of tests/test_gpu_rgb.py.

The restatement composes the contract from the oracle's stages: samples & maxv as floats times 2^-s, the reference's colour
split in float32 (every product and sum rounded on its own), oracle.y_path for Y and oracle.resample for Cb, Cr and A (box for
nearest, bilinear for every other filter), the reference's merge, MIN(255) / MAX(0), times 2^s, truncation.  At depth 8 it must
equal oracle.process -- the whole pass in C -- byte for byte, RGB and RGBA, over the matrix the GPU tests run: that pins the
values the 16-bit GPU tests expect to the oracle, not to the library under test.
"""
import numpy as np
import pytest

from test_gpu_yuv import FILTER_NAMES, FILTERS, MULS, SIZES, first_difference, out_size
from test_gpu_yuv_ex import plane

F = np.float32
LAYOUTS = ("interleaved", "planar")
ORDERS = ("rgb", "bgr")
DEPTHS = (8, 10, 12, 14, 16)
# the 8-bit YUV suite's sizes never give an output width of 7 mod 8 with its multipliers; 21 does (15, 31, 63)
SIZES_RGB = SIZES + [(21, 5)]


def dtype_of(depth):
    return np.uint8 if depth == 8 else np.uint16


def image(w, h, alpha, depth, seed):
    """(h, w, 3 + alpha) in R, G, B[, A] order: per channel noise beside saturated blocks of 0 and maxv."""
    return np.stack([plane(h, w, seed + k, depth) for k in range(3 + alpha)], axis=-1)


def restatement(oracle_lib, img, depth, mul, filt):
    """img: (h, w, c) unsigned samples in R, G, B[, A] order (stray bits above `depth` allowed).  Returns (out (dh, dw, c),
    conv (dh, dw)) as the contract defines them.  The identity size is not restated (the contract defers to srcnn_process_u8)."""
    h, w, c = img.shape
    dw, dh = out_size(w, h, mul)
    assert dw and dh and (dw, dh) != (w, h)
    s, maxv, dt = depth - 8, (1 << depth) - 1, dtype_of(depth)
    down, up = F(2.0 ** -s), F(2.0 ** s)
    ch = [(img[..., k].astype(np.uint32) & maxv).astype(F) * down for k in range(c)]
    r, g, b = ch[:3]
    y = (F(0.299) * r) + (F(0.587) * g) + (F(0.114) * b)
    cb = F(128) - (F(0.1687) * r) - (F(0.3313) * g) + (F(0.5) * b)
    cr = F(128) + (F(0.5) * r) - (F(0.4187) * g) - (F(0.0813) * b)
    assert y.dtype == cb.dtype == cr.dtype == F
    cfilt = 0 if filt == 0 else 1
    yp = oracle_lib.y_path(y, dw, dh, filt)
    cb = oracle_lib.resample(cb, dw, dh, cfilt) - F(128)
    cr = oracle_lib.resample(cr, dw, dh, cfilt) - F(128)
    outs = [yp + F(45) * cr / F(32), yp - (F(11) * cb + F(23) * cr) / F(32), yp + F(113) * cb / F(64)]
    if c == 4:
        outs.append(oracle_lib.resample(ch[3], dw, dh, cfilt))

    def code(v):
        assert v.dtype == F
        v = np.where(F(255) < v, F(255), v)
        v = np.where(F(0) > v, F(0), v)
        return (v * up).astype(np.uint32).astype(dt)
    return np.stack([code(v) for v in outs], axis=-1), (yp * up).astype(np.uint32).astype(dt)


# ---- the case matrix: {interleaved, planar} x {RGB, BGR} x {no alpha, alpha} x depth; filter and multiplier rotate across the
# format cells, every size with two multipliers and one filter per cell; cases whose output size equals the input size are left
# out (the identity size has a test of its own) ----
CELLS = [(l, o, a, d) for l in LAYOUTS for o in ORDERS for a in (0, 1) for d in DEPTHS]


def cases_for(layout, order, alpha, depth):
    base = LAYOUTS.index(layout) + 2 * ORDERS.index(order) + 3 * alpha + 2 * DEPTHS.index(depth)
    for k, (w, h) in enumerate(SIZES_RGB):
        for j in (0, 2):
            filt, mul = FILTERS[(base + k) % 5], MULS[(base + 2 * k + j) % 5]
            dw, dh = out_size(w, h, mul)
            if dw and dh and (dw, dh) != (w, h):
                yield w, h, filt, mul


ALL = [(cell, case) for cell in CELLS for case in cases_for(*cell)]
assert {c[1][2] for c in ALL} == set(FILTERS) and {c[1][3] for c in ALL} == set(MULS) and {c[1][:2] for c in ALL} == set(SIZES_RGB)
for _d in DEPTHS:   # within every depth the output widths take every residue mod 8
    assert {out_size(w, h, m)[0] % 8 for (cell, (w, h, _f, m)) in ALL if cell[3] == _d} == set(range(8)), _d
_WANT = {}


def seed_of(w, h):
    return 100 * w + h


def want_for(oracle_lib, alpha, depth, case):
    """Expected (out, conv) of a matrix case in R, G, B[, A] order: oracle.process at depth 8, the restatement above it."""
    key = (alpha, depth, case)
    if key not in _WANT:
        w, h, filt, mul = case
        img = image(w, h, alpha, depth, seed_of(w, h))
        _WANT[key] = oracle_lib.process(img, mul, filt) if depth == 8 else restatement(oracle_lib, img, depth, mul, filt)
    return _WANT[key]


@pytest.mark.parametrize("alpha", [0, 1], ids=["rgb", "rgba"])
def test_restatement_equals_oracle_process_at_depth_8(oracle_lib, alpha):
    cases = sorted({case for (cell, case) in ALL if cell[2] == alpha and cell[3] == 8})
    assert len(cases) >= 40
    assert {c[2] for c in cases} == set(FILTERS) and {c[3] for c in cases} == set(MULS) and {c[:2] for c in cases} == set(SIZES_RGB)
    for (w, h, filt, mul) in cases:
        img = image(w, h, alpha, 8, seed_of(w, h))
        want_out, want_conv = oracle_lib.process(img, mul, filt)
        got_out, got_conv = restatement(oracle_lib, img, 8, mul, filt)
        what = "%dx%dx%d %s x%g" % (w, h, 3 + alpha, FILTER_NAMES[filt], mul)
        assert got_out.shape == want_out.shape and got_out.dtype == np.uint8, what
        assert np.array_equal(got_out, want_out), what + ": " + first_difference(got_out, want_out)
        assert np.array_equal(got_conv, want_conv), what + " conv: " + first_difference(got_conv, want_conv)


def test_restatement_clips_at_both_ends_and_ignores_stray_bits(oracle_lib):
    """The matrix content reaches both clamps of the merge, and bits above `depth` do not change the restated result."""
    w, h, filt, mul = 23, 17, 2, 2.0
    for depth in (8, 10, 16):
        img = image(w, h, 1, depth, seed_of(w, h))
        out, _ = restatement(oracle_lib, img, depth, mul, filt)
        assert out.min() == 0 and out.max() == 255 << (depth - 8), (depth, out.min(), out.max())
    img = image(w, h, 0, 10, 5)
    dirty = img | (np.random.default_rng(1).integers(0, 64, img.shape).astype(np.uint16) << 10)
    assert np.any(dirty != img)
    for a, b in zip(restatement(oracle_lib, img, 10, mul, filt), restatement(oracle_lib, dirty, 10, mul, filt)):
        assert np.array_equal(a, b)


def test_depth_scaling_is_exact(oracle_lib):
    """An 8-bit image shifted left by s is, at depth 8 + s, the same float planes: the outputs are the 8-bit outputs times 2^s
    only where the clamp result is an integer -- in general they carry s more bits of the same float.  Checked: >> s gives the
    8-bit bytes."""
    w, h, filt, mul = 30, 11, 3, 1.5
    img8 = image(w, h, 1, 8, 77)
    out8, conv8 = restatement(oracle_lib, img8, 8, mul, filt)
    for depth in (10, 12, 16):
        s = depth - 8
        out, conv = restatement(oracle_lib, img8.astype(np.uint16) << s, depth, mul, filt)
        assert np.array_equal(out >> s, out8) and np.array_equal(conv >> s, conv8), depth
