"""GPU: the RGB(A) delta call (include/srcnn_amd_rgb_delta.h).  The flags of k_delta_flags_bytes are compared FOR EQUALITY with a
numpy restatement of the contract -- tile (c, r) is dirty iff a pixel of srcnn_rgb_rect_source(<tile c,r>) has a differing byte in
any plane -- built from S.rgb_rect_source per tile column and row and the byte planes of the two images.  End to end, in strict
mode, the repainted image is compared byte for byte with the oracle's whole image, and every byte outside the dirty tiles with
the canary it held before.  No tolerances anywhere."""
import ctypes as C
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import rgb_delta_worker as DWK  # noqa: E402
import test_gpu_delta as YD  # noqa: E402
from rect_list_worker import DH, DW, H, W  # noqa: E402
from rgb_rect_list_worker import arrange, canonical  # noqa: E402
from test_gpu_rgb import first_difference  # noqa: E402
from test_rgb_delta_abi import coalesce  # noqa: E402
from test_rgb_restatement import image, restatement  # noqa: E402

pytestmark = pytest.mark.gpu

CANARY = 0xA5
GUARD = 4096
E_UNSUPPORTED = -203
TILES = [(32, 16), (40, 24)]
WORKER = os.path.join(os.path.dirname(os.path.abspath(__file__)), "rgb_delta_worker.py")
# layout, order, alpha, depth: every bytes-per-pixel class of the kernel (3, 4, 6, 8 interleaved; 1, 2 planar), and a 10-bit one
CLASSES = [("interleaved", "rgb", 0, 8), ("interleaved", "bgr", 1, 8), ("interleaved", "rgb", 0, 12), ("interleaved", "rgb", 1, 16),
           ("planar", "rgb", 0, 8), ("planar", "bgr", 1, 12), ("interleaved", "bgr", 0, 10)]


def byte_planes(arr, layout):
    """The format's array ((h, w, c) interleaved, (c, h, w) planar; uint8 or uint16) as the (h, row_bytes) byte matrix of every plane."""
    arr = np.ascontiguousarray(arr)
    if layout == "planar":
        return [arr[k].view(np.uint8).reshape(arr.shape[1], -1) for k in range(arr.shape[0])]
    return [arr.view(np.uint8).reshape(arr.shape[0], -1)]


class Geo:
    """An image geometry with its tile grid and the two span tables, from the library's per-rect answers."""

    def __init__(self, S, w=W, h=H, mul=2.0, filt=2, tile=(32, 16)):
        self.S, self.w, self.h, self.mul, self.filt, self.tile = S, w, h, mul, filt, tile
        self.tw, self.th = tile[0] or 64, tile[1] or 64
        self.dw, self.dh, self.cols, self.rows = S.rgb_delta_grid(w, h, mul, filt, tile)
        assert (self.dw, self.dh) == S.output_size(w, h, mul) and (self.cols, self.rows) == (-(-self.dw // self.tw), -(-self.dh // self.th))
        self.xs, self.ys = [], []
        for c in range(self.cols):
            sx0, _, sw, _ = S.rgb_rect_source(w, h, mul, filt, c * self.tw, 0, min(self.tw, self.dw - c * self.tw), min(self.th, self.dh))
            self.xs.append((sx0, sx0 + sw))
        for r in range(self.rows):
            _, sy0, _, sh = S.rgb_rect_source(w, h, mul, filt, 0, r * self.th, min(self.tw, self.dw), min(self.th, self.dh - r * self.th))
            self.ys.append((sy0, sy0 + sh))

    def expected(self, prev, cur, layout):
        """The contract, restated: prev / cur are the format's arrays."""
        diff = np.zeros((self.h, self.w), bool)
        for p, q in zip(byte_planes(prev, layout), byte_planes(cur, layout)):
            diff |= (p != q).reshape(self.h, self.w, -1).any(axis=2)
        out = np.zeros((self.rows, self.cols), np.uint8)
        for r, (ly, hy) in enumerate(self.ys):
            for c, (lx, hx) in enumerate(self.xs):
                out[r, c] = diff[ly:hy, lx:hx].any()
        return out

    def rows_of(self, y):
        return {r for r, (ly, hy) in enumerate(self.ys) if ly <= y < hy}

    def cols_of(self, x):
        return {c for c, (lx, hx) in enumerate(self.xs) if lx <= x < hx}

    def of_pixel(self, x, y):
        out = np.zeros((self.rows, self.cols), np.uint8)
        for r in self.rows_of(y):
            for c in self.cols_of(x):
                out[r, c] = 1
        return out


def upload(S, arr, layout, pad=0, base_off=0, fill=0):
    """The image in device memory, every plane in a buffer of its own with `pad` bytes of garbage after every row and `base_off`
    bytes in front: (plane arguments, pitches in bytes or None).  The garbage is seeded by `fill`, so that two images never share it."""
    planes, pitches = [], []
    for k, m in enumerate(byte_planes(arr, layout)):
        h, row = m.shape
        rng = np.random.default_rng(9000 + 16 * fill + k)
        host = rng.integers(0, 256, size=(h, row + pad), dtype=np.uint8)
        host[:, :row] = m
        buf = S.DeviceBuffer.from_numpy(np.concatenate([np.full(base_off, fill & 0xff, np.uint8), host.reshape(-1)]))
        assert buf.ptr % 16 == 0
        planes.append((buf, base_off))
        pitches.append(row + pad)
    return planes, (pitches if pad else None)


def run_flags(geo, fmt, layout, prev, cur, prev_layout=(0, 0), cur_layout=(0, 0)):
    """One srcnn_rgb_delta_flags_dev call into a guarded, canary-filled buffer: every flag byte is 0 or 1, no guard byte is
    touched.  prev None: no previous image.  *_layout: (pad bytes per row, base offset in bytes).  Returns the (rows, cols) flags."""
    S = geo.S
    n = geo.cols * geo.rows
    fbuf = S.DeviceBuffer.from_numpy(np.full(n + 2 * GUARD, CANARY, np.uint8))
    dprev, ppitch = upload(S, prev, layout, prev_layout[0], prev_layout[1], fill=1) if prev is not None else (None, None)
    dcur, cpitch = upload(S, cur, layout, cur_layout[0], cur_layout[1], fill=2)
    S.rgb_delta_flags_dev(fmt, geo.w, geo.h, geo.mul, geo.filt, dprev, ppitch, dcur, cpitch, geo.tile, (fbuf, GUARD))
    S.sync()
    raw = fbuf.to_numpy(np.uint8, (n + 2 * GUARD,))
    assert np.all(raw[:GUARD] == CANARY) and np.all(raw[GUARD + n:] == CANARY), "a guard byte of the flag buffer was written"
    flags = raw[GUARD:GUARD + n].reshape(geo.rows, geo.cols)
    assert np.all(flags <= 1), "a flag byte is neither 0 nor 1"
    return flags


class Rig:
    """A format with a source image in it and the checks of one launch."""

    def __init__(self, S, layout="interleaved", order="rgb", alpha=0, depth=8, w=W, h=H, mul=2.0, filt=2, tile=(32, 16), seed=77):
        self.S, self.layout, self.order, self.alpha, self.depth = S, layout, order, alpha, depth
        self.geo = Geo(S, w, h, mul, filt, tile)
        self.fmt = S.rgb_format(layout, order, alpha, depth)
        self.prev = arrange(image(w, h, alpha, depth, seed), layout, order)
        self.prev.setflags(write=False)
        self.bps = 1 if depth == 8 else 2
        self.bpp = self.bps * (1 if layout == "planar" else 3 + alpha)          # bytes of a pixel in one plane's row
        self.nplanes = (3 + alpha) if layout == "planar" else 1

    def changed(self, points):
        """The image with one bit flipped in byte `b` of pixel (x, y) of plane `p`, for every (x, y, p, b) of `points`."""
        out = np.array(self.prev, copy=True)
        planes = byte_planes(out, self.layout)
        for (x, y, p, b) in points:
            planes[p][y, x * self.bpp + b] ^= 0x10
        return out

    def check(self, cur, what, prev="own", **lay):
        prev = self.prev if isinstance(prev, str) else prev
        got = run_flags(self.geo, self.fmt, self.layout, prev, cur, **lay)
        want = self.geo.expected(prev, cur, self.layout)
        assert np.array_equal(got, want), "%s\ngot\n%s\nwant\n%s" % (what, got, want)
        return got


# ---- flags, exact ----
@pytest.mark.parametrize("tile", TILES)
def test_identical_images_all_zero(srcnn, tile):
    rig = Rig(srcnn, tile=tile)
    assert not rig.check(rig.prev.copy(), "identical images").any()


def disjoint_batches(items, sets_of):
    """items into batches in which the tile sets sets_of(item) are pairwise disjoint: every change of a batch can be judged alone."""
    batches = []
    for it in items:
        for b in batches:
            if all(not (sets_of(it) & sets_of(o)) for o in b):
                b.append(it)
                break
        else:
            batches.append([it])
    return batches


@pytest.mark.parametrize("tile", TILES)
def test_span_edges_of_every_tile_column_and_row(srcnn, tile):
    """One changed byte at both edges of every span.  Inside the span it is the byte next to the outside pixel (the last byte of
    pixel hx - 1 shares a 32-bit word with pixel hx at 3 bytes a pixel), outside it is the byte next to the span: a kernel that
    marked pixels by the word or the chunk would flag a neighbouring tile column."""
    rig = Rig(srcnn, tile=tile)
    geo, last = rig.geo, rig.bpp - 1
    launches = 0
    ycands = disjoint_batches(list(range(geo.h)), geo.rows_of)[0]          # source rows with pairwise disjoint tile rows
    assert len(ycands) >= 2
    cases = []                                                             # (x, byte of the pixel, tile column, flagged?)
    for c, (lx, hx) in enumerate(geo.xs):
        cases += [(lx, 0, c, True), (hx - 1, last, c, True)]
        if lx > 0:
            cases.append((lx - 1, last, c, False))
        if hx < geo.w:
            cases.append((hx, 0, c, False))
    assert any(not f for (_, _, _, f) in cases)
    for k in range(0, len(cases), len(ycands)):
        batch = list(zip(cases[k:k + len(ycands)], ycands))
        got = rig.check(rig.changed([(x, y, 0, b) for ((x, b, _, _), y) in batch]), "column edges %r" % (batch,))
        launches += 1
        for ((x, _, c, flagged), y) in batch:
            rows = sorted(geo.rows_of(y))
            assert rows and all(bool(got[r, c]) == flagged for r in rows), "x = %d, tile column %d (span %r): %r" % (x, c, geo.xs[c], got[rows, c])
            assert all((got[r, :] != 0).tolist() == [cc in geo.cols_of(x) for cc in range(geo.cols)] for r in rows)
    xcands = disjoint_batches(list(range(geo.w)), geo.cols_of)[0]
    assert len(xcands) >= 2
    cases = []
    for r, (ly, hy) in enumerate(geo.ys):
        cases += [(ly, r, True), (hy - 1, r, True)]
        if ly > 0:
            cases.append((ly - 1, r, False))
        if hy < geo.h:
            cases.append((hy, r, False))
    for k in range(0, len(cases), len(xcands)):
        batch = list(zip(cases[k:k + len(xcands)], xcands))
        got = rig.check(rig.changed([(x, y, 0, (x + y) % rig.bpp) for ((y, _, _), x) in batch]), "row edges %r" % (batch,))
        launches += 1
        for ((y, r, flagged), x) in batch:
            cols = sorted(geo.cols_of(x))
            assert cols and all(bool(got[r, c]) == flagged for c in cols), "y = %d, tile row %d (span %r): %r" % (y, r, geo.ys[r], got[r, cols])
    assert launches <= 40


@pytest.mark.parametrize("tile", TILES)
def test_corners_seeded_sets_everything_and_no_previous_image(srcnn, tile):
    rig = Rig(srcnn, tile=tile)
    geo = rig.geo
    corners = [(0, 0, 0, 0), (W - 1, 0, 0, 2), (0, H - 1, 0, 1), (W - 1, H - 1, 0, 2)]
    for p in corners:
        got = rig.check(rig.changed([p]), "corner %r" % (p,))
        assert got.sum() == len(geo.rows_of(p[1])) * len(geo.cols_of(p[0])) > 0
    rig.check(rig.changed(corners), "the four corners")
    rng = np.random.default_rng(424242)
    for n in (1, 3, 20):
        pts = [(int(rng.integers(0, W)), int(rng.integers(0, H)), 0, int(rng.integers(0, 3))) for _ in range(n)]
        assert rig.check(rig.changed(pts), "%d seeded bytes %r" % (n, pts)).any()
    every = (rig.prev ^ 0xff).astype(rig.prev.dtype)
    assert rig.check(every, "every byte changed").all()
    assert run_flags(geo, rig.fmt, rig.layout, None, rig.prev).all(), "no previous image: all ones"


@pytest.mark.parametrize("layout,order,alpha,depth", CLASSES, ids=["%s-%s-a%d-%d" % c for c in CLASSES])
def test_every_byte_of_a_pixel_in_every_format_class(srcnn, layout, order, alpha, depth):
    """A single byte of a single sample at a time: the alpha byte alone, the high byte of a 10 / 12-bit sample alone (bits the
    value formula ignores), each plane of a planar image alone.  The flags are the pixel's, whichever byte it was."""
    rig = Rig(srcnn, layout, order, alpha, depth, seed=300 + depth + alpha)
    assert rig.bpp == srcnn.rgb_plane_size(rig.fmt, 1, 1, 0)[2]
    geo = rig.geo
    seen = 0
    for (x, y) in ((41, 23), (W - 1, 5)):
        want = geo.of_pixel(x, y)
        assert want.any()
        for p in range(rig.nplanes):
            for b in range(rig.bpp):
                got = rig.check(rig.changed([(x, y, p, b)]), "%s %s alpha=%d %d-bit: pixel (%d, %d), plane %d, byte %d" % (layout, order, alpha, depth, x, y, p, b))
                assert np.array_equal(got, want)
                seen += 1
    assert seen == 2 * rig.nplanes * rig.bpp
    if depth > 8:            # the unused high bits of a word count: the rule is about bytes, not values
        cur = np.array(rig.prev, copy=True)
        planes = byte_planes(cur, layout)
        planes[0][9, 7 * rig.bpp + 1] ^= 0x80
        assert np.array_equal((np.asarray(cur) & ((1 << depth) - 1)), (np.asarray(rig.prev) & ((1 << depth) - 1))) or depth == 16
        assert np.array_equal(rig.check(cur, "bit 15 of a sample"), geo.of_pixel(7, 9))
    assert not rig.check(rig.prev.copy(), "identical").any()


# ---- alignment and pitch ----
def test_vector_route_and_fallback_give_the_same_flags(srcnn):
    for (layout, order, alpha, depth, offs) in (("interleaved", "rgb", 0, 8, (1, 3, 5)), ("interleaved", "rgb", 1, 16, (2, 6, 2)), ("planar", "bgr", 1, 8, (1, 7, 9))):
        rig = Rig(srcnn, layout, order, alpha, depth)
        row = rig.bpp * W
        assert row % 16 == 0                   # 96 pixels: a tight image on 16-byte aligned bases takes the vector route
        rng = np.random.default_rng(31337 + depth)
        pts = [(int(rng.integers(0, W)), int(rng.integers(0, H)), int(rng.integers(0, rig.nplanes)), int(rng.integers(0, rig.bpp))) for _ in range(6)]
        pts += [(0, 0, 0, 0), (W - 1, H - 1, rig.nplanes - 1, rig.bpp - 1), (3, 17, 0, rig.bpp - 1), (4, 17, 0, 0), (W - 4, 30, 0, 0), (W - 5, 31, 0, rig.bpp - 1)]
        cur, same = rig.changed(pts), rig.prev.copy()
        odd = offs[1] if depth == 8 else 2 * offs[1]          # above depth 8 a pitch is even
        layouts = {"tight, 16-byte aligned (vector)": dict(),
                   "prev at +%d bytes (fallback)" % offs[0]: dict(prev_layout=(0, offs[0])),
                   "cur at +%d bytes (fallback)" % offs[2]: dict(cur_layout=(0, offs[2])),
                   "pitches of 16 n, different (vector)": dict(prev_layout=(16, 0), cur_layout=(48, 0)),
                   "a pitch that is no multiple of 16 (fallback)": dict(prev_layout=(odd, 0), cur_layout=(32, 0)),
                   "both at +16 bytes, pitched (vector)": dict(prev_layout=(32, 16), cur_layout=(16, 16)),
                   "both unaligned and pitched (fallback)": dict(prev_layout=(odd, offs[0]), cur_layout=(odd + 2, offs[2]))}
        got = {name: rig.check(cur, "%s: %s" % (layout, name), **lay) for name, lay in layouts.items()}
        first = got["tight, 16-byte aligned (vector)"]
        assert first.any() and not first.all()
        for name, g in got.items():
            assert np.array_equal(g, first), name
        # pitch padding holds different garbage in the two images (upload seeds it per image) and must not flag
        for name, lay in layouts.items():
            assert not rig.check(same, name + ", identical", **lay).any(), name


# ---- chunk, word and piece edges ----
def test_rows_that_are_no_multiple_of_4_or_16_bytes(srcnn):
    w, h = 37, 23                              # RGB8: rows of 111 bytes
    rig = Rig(srcnn, w=w, h=h, tile=(16, 16), seed=78)
    assert (rig.geo.cols, rig.geo.rows) == (5, 3)
    cases = ([(36, 0, 0, 2)], [(36, 22, 0, 0)], [(35, 11, 0, 1)], [(32, 5, 0, 0), (36, 6, 0, 2)], [(0, 0, 0, 0), (31, 9, 0, 2), (32, 9, 0, 0), (36, 20, 0, 1)],
             [(5, 3, 0, 0)], [(5, 3, 0, 1)], [(5, 3, 0, 2)], [])
    for pts in cases:
        cur = rig.changed(pts)
        tight = rig.check(cur, "37 x 23 tight (pitch 111: fallback) %r" % (pts,))
        padded = rig.check(cur, "37 x 23, pitch 112 (vector, 15 bytes of row tail) %r" % (pts,), prev_layout=(1, 0), cur_layout=(1, 0))
        mixed = rig.check(cur, "37 x 23, pitches 128 and 144 %r" % (pts,), prev_layout=(17, 0), cur_layout=(33, 0))
        assert np.array_equal(tight, padded) and np.array_equal(tight, mixed) and tight.any() == bool(pts)
    # every byte of the row tail (bytes 96 ... 110: three words and three bytes for the lane that reads it), one at a time
    for b in range(96, 111):
        got = rig.check(rig.changed([(b // 3, 7, 0, b % 3)]), "tail byte %d" % b, prev_layout=(1, 0), cur_layout=(17, 0))
        assert np.array_equal(got, rig.geo.of_pixel(b // 3, 7))
    assert rig.check((rig.prev ^ 0xff).astype(np.uint8), "37 x 23, every byte", prev_layout=(1, 0), cur_layout=(1, 0)).all()


def test_an_image_of_one_row_takes_the_vector_route_at_any_pitch(srcnn):
    """With one row the pitch places nothing: 16-byte aligned bases are enough for the vector route, whatever pitch the caller
    states, and the fallback (an odd base) gives the same flags."""
    rig = Rig(srcnn, w=37, h=1, tile=(16, 16), seed=81)
    for pts in ([(36, 0, 0, 2)], [(0, 0, 0, 0), (31, 0, 0, 2), (32, 0, 0, 1)], [(5, 0, 0, 1)], []):
        cur = rig.changed(pts)
        got = [rig.check(cur, "37 x 1, %s %r" % (name, pts), **lay) for name, lay in
               (("tight (pitch 111)", dict()), ("pitches 116 and 113", dict(prev_layout=(5, 0), cur_layout=(2, 0))), ("an odd base", dict(cur_layout=(0, 3))))]
        assert all(np.array_equal(g, got[0]) for g in got) and got[0].any() == bool(pts)


# rows that cross a piece, 8 rows high so that only flags cost anything.  A piece is 256 * U chunks of 16 bytes with the U of
# 1 ... 4 the launcher picks for the row: 5501 RGB8 pixels -> 1032 chunks -> U = 1 (five pieces of 4096 B), 6150 RGB12 pixels ->
# 2307 chunks -> U = 2 (8192 B), 8000 RGB8 -> 1500 chunks -> U = 3 (12288 B), 9600 RGB8 -> 1800 chunks -> U = 4 (16384 B);
# 2760 RGB12 pixels -> U = 1.
# Every multiple of 4096 B inside the row is a boundary of one of those pieces or of a lane's chunk group.
@pytest.mark.parametrize("w,depth", [(4096 // 3 + 40 + 4096, 8), (6150, 12), (8000, 8), (9600, 8), (2760, 12)], ids=["U1", "U2-rgb12", "U3", "U4", "U1-rgb12"])
def test_pixels_that_straddle_a_piece_a_chunk_and_a_word(srcnn, w, depth):
    rig = Rig(srcnn, depth=depth, w=w, h=8, tile=(32, 16), seed=79)
    bpp, row = rig.bpp, rig.bpp * w
    bounds = list(range(4096, row, 4096)) + [16 * 101, 1004]          # pieces; a 16-byte boundary; a 4-byte boundary that is not one
    p16 = -row % 16                                                    # pitches of 16 n, different in the two images: the vector route
    vec = dict(prev_layout=(p16, 0), cur_layout=(p16 + 16, 0))
    assert any(b % bpp for b in bounds[:-2]) and 1616 % bpp and 1004 % bpp and 1004 % 16
    for k, at in enumerate(bounds):
        px, y = at // bpp, k % 8                                        # the pixel that owns byte `at`: it straddles when at % bpp != 0
        for b in range(bpp):
            got = rig.check(rig.changed([(px, y, 0, b)]), "byte %d of pixel %d, which holds byte %d of the row" % (b, px, at), **vec)
            assert np.array_equal(got, rig.geo.of_pixel(px, y))
        for (x, b) in ((px - 1, bpp - 1), (px + 1, 0)):                 # the neighbours' bytes next to it
            got = rig.check(rig.changed([(x, y, 0, b)]), "byte %d of pixel %d, next to the pixel of byte %d" % (b, x, at), **vec)
            assert np.array_equal(got, rig.geo.of_pixel(x, y))
    # the same on the fallback (an odd base) for the first piece boundary, and the last pixel of the row on both routes
    px = 4096 // bpp
    off = 1 if depth == 8 else 2
    for pts in ([(px, 3, 0, 0)], [(px, 3, 0, bpp - 1)], [(w - 1, 7, 0, bpp - 1)], [(0, 0, 0, 0), (w - 1, 0, 0, 0)]):
        a = rig.check(rig.changed(pts), "%r" % (pts,), **vec)
        assert np.array_equal(a, rig.check(rig.changed(pts), "%r on the fallback" % (pts,), prev_layout=(p16, off), cur_layout=(p16, 0)))
    assert not rig.check(rig.prev.copy(), "identical", **vec).any()


# ---- other geometry ----
@pytest.mark.parametrize("w,h,mul,filt,tile", [(96, 56, 2.5, 3, (0, 0)), (40, 31, 1.5, 2, (16, 8)), (50, 30, 0.75, 2, (8, 8)), (24, 24, 1.0, 2, (8, 8)),
                                               (30, 1, 1.5, 1, (8, 8)), (96, 56, 2.0, 0, (8, 8))],
                         ids=["2.5x-lanczos3-default-tiles", "x1.5", "down-scale", "identity", "identity-axis", "nearest-8x8"])
def test_other_geometry(srcnn, w, h, mul, filt, tile):
    layout, order, alpha, depth = ("interleaved", "bgr", 1, 8) if w % 20 else ("planar", "rgb", 0, 12)
    rig = Rig(srcnn, layout, order, alpha, depth, w, h, mul, filt, tile, seed=80)
    rng = np.random.default_rng(555 + w)
    assert not rig.check(rig.prev.copy(), "identical").any()
    rnd = lambda: (int(rng.integers(0, w)), int(rng.integers(0, h)), int(rng.integers(0, rig.nplanes)), int(rng.integers(0, rig.bpp)))   # noqa: E731
    for n in (1, 4, 25):
        pts = [rnd() for _ in range(n)]
        rig.check(rig.changed(pts), "%d bytes %r" % (n, pts))
    for (x, y) in ((0, 0), (w - 1, h - 1), (w // 2, h // 2)):
        got = rig.check(rig.changed([(x, y, rig.nplanes - 1, rig.bpp - 1)]), "%r" % ((x, y),))
        assert np.array_equal(got, rig.geo.of_pixel(x, y))
    assert rig.check((rig.prev ^ 0x01).astype(rig.prev.dtype), "every sample").all()


# ---- the span tables both delta calls keep in one place ----
def test_y_and_rgb_flags_back_to_back_on_one_stream(srcnn):
    """srcnn_y_path_delta_flags_dev, srcnn_rgb_delta_flags_dev and srcnn_y_path_delta_flags_dev again, queued on one stream with
    nothing between them, each into a flag buffer of its own and each compared with its restatement.  The two calls keep their
    span tables in the same buffer of the stream's workspace, so each call here invalidates the tables of the one before and
    uploads its own while that one's kernel may still be reading: first with the RGB(A) image at the Y plane's geometry, then at
    another.  This guards the order of invalidate, upload and launch.  It cannot tell whose tables a call used: for these
    geometries both rules give the same tables."""
    S = srcnn
    bicubic = S.SRCNNF_Bicubic
    ygeo = YD.Geo(S, filt=bicubic, tile=(16, 16))
    plane = YD.RW.frame_plane()
    ycurs = [YD.changed(plane, [(5, 3), (70, 40)]), YD.changed(plane, [(90, 55), (33, 20)])]
    ywants = [ygeo.expected(plane, c) for c in ycurs]
    assert ywants[0].any() and not np.array_equal(ywants[0], ywants[1])
    for kw in (dict(tile=(16, 16)), dict(w=40, h=31, mul=1.5, tile=(16, 8))):
        rig = Rig(S, filt=bicubic, **kw)
        rgeo = rig.geo
        rcur = rig.changed([(7, 9, 0, 1), (rgeo.w - 1, rgeo.h - 1, 0, 0)])
        wants = [ywants[0], rgeo.expected(rig.prev, rcur, rig.layout), ywants[1]]
        assert wants[1].any() and not wants[1].all()
        dplane = YD.upload(S, plane, fill=1)[0]
        dycurs = [YD.upload(S, c, fill=2 + k)[0] for k, c in enumerate(ycurs)]
        dprev = upload(S, rig.prev, rig.layout, fill=1)[0]
        dcur = upload(S, rcur, rig.layout, fill=2)[0]
        fbufs = [S.DeviceBuffer.from_numpy(np.full(want.size + 2 * GUARD, CANARY, np.uint8)) for want in wants]
        S.sync()
        S.y_path_delta_flags_dev(dplane, 0, dycurs[0], 0, ygeo.w, ygeo.h, ygeo.dw, ygeo.dh, bicubic, ygeo.tile, (fbufs[0], GUARD))
        S.rgb_delta_flags_dev(rig.fmt, rgeo.w, rgeo.h, rgeo.mul, bicubic, dprev, None, dcur, None, rgeo.tile, (fbufs[1], GUARD))
        S.y_path_delta_flags_dev(dplane, 0, dycurs[1], 0, ygeo.w, ygeo.h, ygeo.dw, ygeo.dh, bicubic, ygeo.tile, (fbufs[2], GUARD))
        S.sync()
        for k, (fbuf, want) in enumerate(zip(fbufs, wants)):
            raw = fbuf.to_numpy(np.uint8, (want.size + 2 * GUARD,))
            assert np.all(raw[:GUARD] == CANARY) and np.all(raw[GUARD + want.size:] == CANARY), "call %d wrote a guard byte of its flag buffer" % k
            got = raw[GUARD:GUARD + want.size].reshape(want.shape)
            assert np.array_equal(got, want), "call %d of the sequence, RGB(A) at %r\ngot\n%s\nwant\n%s" % (k, kw, got, want)


# ---- end to end, strict ----
_WANT = {}


def oracle_of(oracle_lib, img, depth, mul=2.0, filt=2):
    """(out, conv) of the whole image `img` ((h, w, c) in R, G, B[, A] order): computed once per image, read-only."""
    key = (img.tobytes(), img.shape, depth, mul, filt)
    if key not in _WANT:
        want = oracle_lib.process(img, mul, filt) if depth == 8 else restatement(oracle_lib, img, depth, mul, filt)
        for a in want:
            a.setflags(write=False)
        _WANT[key] = tuple(want)
    return _WANT[key]


E2E = [("interleaved", "rgb", 0, 8), ("planar", "bgr", 1, 12)]
E2E_IDS = ["rgb8", "planar-bgra12"]


class OutImage:
    """A dw x dh destination image and its conv plane in device memory, every plane with `pad` bytes after each row and a guard
    on each side, canary-filled or holding `init` = (out, conv) in R, G, B[, A] order."""

    def __init__(self, S, layout, order, alpha, depth, dw=DW, dh=DH, pad=0, init=None):
        self.S, self.layout, self.order, self.dw, self.dh, self.pad = S, layout, order, dw, dh, pad
        self.dt = np.uint8 if depth == 8 else np.uint16
        self.c = 3 + alpha
        bps = np.dtype(self.dt).itemsize
        self.rows = [bps * dw * (1 if layout == "planar" else self.c)] * (self.c if layout == "planar" else 1) + [bps * dw]     # planes, then conv
        mats = [None] * len(self.rows)
        if init is not None:
            mats = byte_planes(arrange(init[0], layout, order), layout) + [np.ascontiguousarray(init[1]).view(np.uint8).reshape(dh, -1)]
        self.bufs = []
        for row, m in zip(self.rows, mats):
            body = np.full((dh, row + pad), CANARY, np.uint8)
            if m is not None:
                body[:, :row] = m
            self.bufs.append(S.DeviceBuffer.from_numpy(np.concatenate([np.full(GUARD, CANARY, np.uint8), body.reshape(-1), np.full(GUARD, CANARY, np.uint8)])))
        self.dst = [(b, GUARD) for b in self.bufs[:-1]]
        self.dst_pitch = [r + pad for r in self.rows[:-1]] if pad else None
        self.conv = (self.bufs[-1], GUARD)
        self.conv_pitch = self.rows[-1] + pad if pad else 0

    def fetch(self):
        """((out, conv) in R, G, B[, A] order, every other byte: guards and pitch padding)"""
        mats, rest = [], []
        for row, b in zip(self.rows, self.bufs):
            raw = b.to_numpy(np.uint8, (b.nbytes,))
            body = raw[GUARD:GUARD + (row + self.pad) * self.dh].reshape(self.dh, row + self.pad)
            rest += [raw[:GUARD], raw[GUARD + (row + self.pad) * self.dh:], np.ascontiguousarray(body[:, row:]).reshape(-1)]
            mats.append(np.ascontiguousarray(body[:, :row]))
        if self.layout == "planar":
            arr = np.stack([m.view(self.dt) for m in mats[:-1]])
        else:
            arr = mats[0].view(self.dt).reshape(self.dh, self.dw, self.c)
        return (canonical(arr, self.layout, self.order), mats[-1].view(self.dt).reshape(self.dh, self.dw)), np.concatenate(rest)


def delta(S, fmt, layout, order, prev, cur, out, tile=(32, 16), mul=2.0, filt=2, stream=None):
    """prev / cur: (h, w, c) in R, G, B[, A] order (prev None: no previous image)."""
    h, w = cur.shape[:2]
    dprev, _ = upload(S, arrange(prev, layout, order), layout, fill=1) if prev is not None else (None, None)
    dcur, _ = upload(S, arrange(cur, layout, order), layout, fill=2)
    st = S.rgb_upscale_delta_dev(fmt, w, h, mul, filt, dprev, None, dcur, None, tile, out.dst, out.dst_pitch, out.conv, out.conv_pitch, stream)
    S.sync()
    return st


def restated_stats(geo, prev, cur, layout, order):
    """(tiles, dirty_tiles, rects, whole_frame, cell_samples) and the rects, from the restated flags and the restated coalescer
    (the whole-frame rule: every tile dirty, or the cells reach the setting's share of dw x dh)."""
    e = geo.expected(arrange(prev, layout, order), arrange(cur, layout, order), layout)
    rects = coalesce(e, (geo.tw, geo.th), geo.dw, geo.dh)
    cells = sum((rw + 12) * (rh + 12) for (_, _, rw, rh) in rects)
    permille = int(re.search(r"SRCNN_DELTA_WHOLE_PERMILLE=(\d+)", geo.S.debug_settings()).group(1))
    whole = bool(rects) and (bool(e.all()) or len(rects) > 65536 or cells * 1000 >= permille * geo.dw * geo.dh)
    return (geo.cols * geo.rows, int(e.sum()), len(rects), int(whole), cells), rects


def stats_tuple(st):
    return st.tiles, st.dirty_tiles, st.rects, st.whole_frame, st.cell_samples


def assert_pair(got, want, what):
    for name, g, e in zip(("out", "conv"), got, want):
        assert g.shape == e.shape and g.dtype == e.dtype, (what, name, g.shape, e.shape, g.dtype, e.dtype)
        assert np.array_equal(g, e), "%s %s: %s" % (what, name, first_difference(g, e))


def with_pixel(img, x, y, k, depth):
    out = np.array(img, copy=True)
    out[y, x, k] ^= 1 << (depth - 2)
    return out


@pytest.mark.parametrize("layout,order,alpha,depth", E2E, ids=E2E_IDS)
@pytest.mark.parametrize("pad", [0, 6], ids=["tight", "pitched"])
def test_canary_repaint(srcnn, oracle_lib, layout, order, alpha, depth, pad):
    S = srcnn
    assert S.lib().srcnn_get_mode() == S.MODE_STRICT
    prev = image(W, H, alpha, depth, 9656)
    cur = with_pixel(prev, 48, 28, 1, depth)
    geo = Geo(S)
    want_stats, rects = restated_stats(geo, prev, cur, layout, order)
    assert len(rects) == 1 and want_stats[3] == 0 and want_stats[4] * 4 < DW * DH          # one rect, on the list route
    out = OutImage(S, layout, order, alpha, depth, pad=pad)
    st = delta(S, S.rgb_format(layout, order, alpha, depth), layout, order, prev, cur, out)
    assert st.struct_size == C.sizeof(S.DeltaStats) and stats_tuple(st) == want_stats
    got, rest = out.fetch()
    x0, y0, rw, rh = rects[0]
    want = oracle_of(oracle_lib, cur, depth)
    assert_pair([g[y0:y0 + rh, x0:x0 + rw] for g in got], [e[y0:y0 + rh, x0:x0 + rw] for e in want], "the dirty tiles of a change at (48, 28)")
    mask = np.ones((DH, DW), bool)
    mask[y0:y0 + rh, x0:x0 + rw] = False
    for g in got:
        assert np.all(np.ascontiguousarray(g[mask]).view(np.uint8) == CANARY), "a pixel of a clean tile was written"
    assert np.all(rest == CANARY), "a guard or padding byte was written"


@pytest.mark.parametrize("layout,order,alpha,depth", E2E, ids=E2E_IDS)
def test_sequence_of_frames(srcnn, oracle_lib, layout, order, alpha, depth):
    S = srcnn
    base = image(W, H, alpha, depth, 9656)

    def with_block(x, y):
        f = np.array(base, copy=True)
        f[y:y + 5, x:x + 5, :3] ^= 1 << (depth - 1)
        return f
    frames = [base, with_block(10, 8), with_block(10, 8), with_block(60, 30)]          # the block appears, stays, moves
    fmt = S.rgb_format(layout, order, alpha, depth)
    first = S.rgb_upscale(arrange(frames[0], layout, order), 2.0, 2, layout=layout, order=order, depth=depth, want_conv=True)
    init = (canonical(first[0], layout, order), first[1])
    assert_pair(init, oracle_of(oracle_lib, frames[0], depth), "srcnn_rgb_upscale_dev of frame 0")
    out = OutImage(S, layout, order, alpha, depth, pad=2, init=init)
    geo = Geo(S)
    for k in (1, 2, 3):
        st = delta(S, fmt, layout, order, frames[k - 1], frames[k], out)
        got, rest = out.fetch()
        assert_pair(got, oracle_of(oracle_lib, frames[k], depth), "frame %d" % k)
        assert np.all(rest == CANARY)
        assert stats_tuple(st) == restated_stats(geo, frames[k - 1], frames[k], layout, order)[0]
        assert (st.rects == 0 and st.dirty_tiles == 0) if k == 2 else (1 <= st.rects <= st.dirty_tiles)
    # the numpy convenience gives the same image
    want2, want3 = oracle_of(oracle_lib, frames[2], depth), oracle_of(oracle_lib, frames[3], depth)
    res, conv, st = S.rgb_upscale_delta(arrange(frames[2], layout, order), arrange(frames[3], layout, order), arrange(want2[0], layout, order), 2.0, 2,
                                        layout=layout, order=order, depth=depth, tile=(32, 16), conv=want2[1])
    assert_pair((canonical(res, layout, order), conv), want3, "rgb_upscale_delta")
    assert st.rects >= 1 and st.whole_frame == 0
    res, st = S.rgb_upscale_delta(None, arrange(frames[3], layout, order), np.zeros_like(arrange(want3[0], layout, order)), layout=layout, order=order, depth=depth)
    assert np.array_equal(canonical(res, layout, order), want3[0]) and st.whole_frame == 1


@pytest.mark.parametrize("layout,order,alpha,depth", E2E, ids=E2E_IDS)
def test_every_pixel_changed_takes_the_whole_frame(srcnn, oracle_lib, layout, order, alpha, depth):
    S = srcnn
    prev = image(W, H, alpha, depth, 9656)
    cur = prev ^ 1
    want = oracle_of(oracle_lib, cur, depth)
    for p in (prev, None):                               # every tile dirty; no previous image
        out = OutImage(S, layout, order, alpha, depth, pad=4)
        st = delta(S, S.rgb_format(layout, order, alpha, depth), layout, order, p, cur, out, tile=(0, 0))
        assert st.whole_frame == 1 and st.tiles == st.dirty_tiles == 6 and st.rects == 1 and st.cell_samples == (DW + 12) * (DH + 12)
        got, rest = out.fetch()
        assert_pair(got, want, "whole frame")
        assert np.all(rest == CANARY)


def test_a_change_in_alpha_only_repaints_alpha(srcnn, oracle_lib):
    S = srcnn
    layout, order, alpha, depth = E2E[1]
    prev = image(W, H, alpha, depth, 9656)
    cur = with_pixel(prev, 70, 40, 3, depth)
    assert np.array_equal(prev[..., :3], cur[..., :3])
    before, after = oracle_of(oracle_lib, prev, depth), oracle_of(oracle_lib, cur, depth)
    assert np.array_equal(before[0][..., :3], after[0][..., :3]) and not np.array_equal(before[0][..., 3], after[0][..., 3])
    out = OutImage(S, layout, order, alpha, depth, init=before)
    st = delta(S, S.rgb_format(layout, order, alpha, depth), layout, order, prev, cur, out)
    assert stats_tuple(st) == restated_stats(Geo(S), prev, cur, layout, order)[0] and st.dirty_tiles > 0 and st.whole_frame == 0
    got, rest = out.fetch()
    assert_pair(got, after, "alpha changed")
    assert np.all(rest == CANARY)


# ---- capture ----
def test_a_stream_under_the_callers_capture_is_refused(srcnn):
    S = srcnn
    hip = None
    for name in ("libamdhip64.so.7", "libamdhip64.so", "/opt/rocm/lib/libamdhip64.so"):
        try:
            hip = C.CDLL(name)
            break
        except OSError:
            continue
    assert hip is not None, "no libamdhip64 to capture a stream with"
    vp = C.c_void_p
    hip.hipStreamBeginCapture.argtypes = [vp, C.c_int]
    hip.hipStreamEndCapture.argtypes = [vp, C.POINTER(vp)]
    hip.hipGraphGetNodes.argtypes = [vp, vp, C.POINTER(C.c_size_t)]
    hip.hipGraphDestroy.argtypes = [vp]
    hip.hipStreamDestroy.argtypes = [vp]
    hip.hipStreamSynchronize.argtypes = [vp]
    layout, order, alpha, depth = E2E[0]
    fmt = S.rgb_format(layout, order, alpha, depth)
    prev = image(W, H, alpha, depth, 9656)
    cur = with_pixel(prev, 48, 28, 1, depth)
    dprev, _ = upload(S, arrange(prev, layout, order), layout, fill=1)
    dcur, _ = upload(S, arrange(cur, layout, order), layout, fill=2)
    out = OutImage(S, layout, order, alpha, depth)
    call = lambda o, s: S.rgb_upscale_delta_dev(fmt, W, H, 2.0, 2, dprev, None, dcur, None, (32, 16), o.dst, o.dst_pitch, o.conv, o.conv_pitch, s)   # noqa: E731
    raw = vp()
    assert hip.hipStreamCreateWithFlags(C.byref(raw), 1) == 0          # hipStreamNonBlocking
    try:
        # once eagerly on this stream: whatever the call keeps per stream exists before the capture begins
        st = call(out, raw.value)
        assert hip.hipStreamSynchronize(raw) == 0 and st.rects == 1
        out = OutImage(S, layout, order, alpha, depth)
        graph = vp()
        assert hip.hipStreamBeginCapture(raw, 2) == 0                  # hipStreamCaptureModeRelaxed
        try:
            with pytest.raises(S.SrcnnError) as e:
                call(out, raw.value)
        finally:
            rc = hip.hipStreamEndCapture(raw, C.byref(graph))
        assert e.value.code == E_UNSUPPORTED
        assert rc == 0 and graph.value, "the capture did not end cleanly (%d)" % rc
        n = C.c_size_t(99)
        assert hip.hipGraphGetNodes(graph, None, C.byref(n)) == 0 and n.value == 0, "%d nodes were captured" % n.value
        hip.hipGraphDestroy(graph)
        assert hip.hipStreamSynchronize(raw) == 0
        got, rest = out.fetch()
        assert all(np.all(np.ascontiguousarray(g).view(np.uint8) == CANARY) for g in got) and np.all(rest == CANARY)
    finally:
        hip.hipStreamDestroy(raw)


# ---- torch ----
def test_torch_uint8_hwc_vs_oracle(oracle_lib):
    r = subprocess.run([sys.executable, WORKER, "torch"], capture_output=True, text=True, timeout=600)
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")]
    assert r.returncode == 0 and line, "rgb_delta_worker torch: exit %d\n%s\n%s" % (r.returncode, r.stdout[-600:], r.stderr[-1500:])
    res = json.loads(line[0][7:])
    if "skip" in res:
        pytest.skip(res["skip"])
    frames = DWK.torch_frames()
    want = [oracle_of(oracle_lib, f, 8)[0] for f in frames]
    assert res["first"]["sha"] == DWK.digest(want[0]) and res["first"]["whole_frame"] == 1, "prev=None: the whole image"
    assert res["second"]["sha"] == DWK.digest(want[1]) and res["second"]["whole_frame"] == 0 and 1 <= res["second"]["rects"] <= res["second"]["dirty_tiles"] < res["second"]["tiles"]
    # a row-padded out tensor: the padding keeps its bytes
    wide = np.full((DH, DW + 5, 3), 0x5A, np.uint8)
    wide[:, :DW] = want[1]
    assert res["padded"]["sha"] == DWK.digest(wide)
    assert res["unchanged"] == {"sha": DWK.digest(want[1]), "rects": 0, "dirty_tiles": 0}
    assert res["refused"] == [True, True, True]


# ---- a non-parity mode ----
def test_fast_mode_repaints_what_the_rect_call_gives(srcnn):
    S = srcnn
    layout, order, alpha, depth = E2E[1]
    fmt = S.rgb_format(layout, order, alpha, depth)
    prev = image(W, H, alpha, depth, 1212)
    cur = with_pixel(with_pixel(prev, 48, 28, 0, depth), 150 // 2, 10, 2, depth)
    geo = Geo(S)
    _, rects = restated_stats(geo, prev, cur, layout, order)
    assert len(rects) == 2
    was = S.set_mode(S.MODE_FAST)         # (a strict-only build refuses: conftest turns that into a skip)
    try:
        out = OutImage(S, layout, order, alpha, depth, pad=2)
        st = delta(S, fmt, layout, order, prev, cur, out)
        assert st.rects == 2 and st.whole_frame == 0
        got, rest = out.fetch()
        dcur, _ = upload(S, arrange(cur, layout, order), layout, fill=2)
        painted = np.zeros((DH, DW), bool)
        for (x0, y0, rw, rh) in rects:
            single = OutImage(S, layout, order, alpha, depth, dw=rw, dh=rh)
            S.rgb_upscale_rect_dev(fmt, W, H, 2.0, 2, dcur, None, x0, y0, rw, rh, single.dst, None, single.conv, 0)
            S.sync()
            assert_pair([g[y0:y0 + rh, x0:x0 + rw] for g in got], single.fetch()[0], "MODE_FAST: rect %r vs srcnn_rgb_upscale_rect_dev" % ((x0, y0, rw, rh),))
            painted[y0:y0 + rh, x0:x0 + rw] = True
        for g in got:
            assert np.all(np.ascontiguousarray(g[~painted]).view(np.uint8) == CANARY), "an untouched pixel lost its bytes"
        assert np.all(rest == CANARY)
    finally:
        S.set_mode(was)
