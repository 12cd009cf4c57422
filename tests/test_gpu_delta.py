"""GPU: the delta call (include/srcnn_amd_delta.h).  The flags of k_delta_flags are compared FOR EQUALITY with a numpy restatement
of the contract -- tile (c, r) is dirty iff a sample of srcnn_y_path_rect_source(<tile c,r>) differs in its 32 bits -- built from
S.y_path_rect_source per tile column and row and the positions where the planes' uint32 views differ.  End to end, in strict mode,
the repainted plane is compared bit for bit with the oracle's whole frame, and every byte outside the dirty tiles with the canary
it held before."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import rect_list_worker as RW  # noqa: E402
from conftest import assert_bit_equal  # noqa: E402
from rect_list_worker import DH, DW, H, W  # noqa: E402

pytestmark = pytest.mark.gpu

CANARY = 0xA5
GUARD = 4096
E_UNSUPPORTED = -203
TILES = [(32, 16), (40, 24)]


class Geo:
    """A frame geometry with its tile grid and the two span tables, from the library's per-rect answers."""

    def __init__(self, S, w=W, h=H, dw=DW, dh=DH, filt=2, tile=(32, 16)):
        self.S, self.w, self.h, self.dw, self.dh, self.filt, self.tile = S, w, h, dw, dh, filt, tile
        self.tw, self.th = tile[0] or 64, tile[1] or 64
        self.cols, self.rows = S.y_path_delta_grid(w, h, dw, dh, filt, tile)
        assert (self.cols, self.rows) == (-(-dw // self.tw), -(-dh // self.th))
        self.xs, self.ys = [], []
        for c in range(self.cols):
            sx0, _, sw, _ = S.y_path_rect_source(w, h, dw, dh, filt, c * self.tw, 0, min(self.tw, dw - c * self.tw), min(self.th, dh))
            self.xs.append((sx0, sx0 + sw))
        for r in range(self.rows):
            _, sy0, _, sh = S.y_path_rect_source(w, h, dw, dh, filt, 0, r * self.th, min(self.tw, dw), min(self.th, dh - r * self.th))
            self.ys.append((sy0, sy0 + sh))

    def expected(self, prev, cur):
        """The contract, restated."""
        diff = np.ascontiguousarray(prev, np.float32).view(np.uint32) != np.ascontiguousarray(cur, np.float32).view(np.uint32)
        out = np.zeros((self.rows, self.cols), np.uint8)
        for r, (ly, hy) in enumerate(self.ys):
            for c, (lx, hx) in enumerate(self.xs):
                out[r, c] = diff[ly:hy, lx:hx].any()
        return out

    def rows_of(self, y):
        return {r for r, (ly, hy) in enumerate(self.ys) if ly <= y < hy}

    def cols_of(self, x):
        return {c for c, (lx, hx) in enumerate(self.xs) if lx <= x < hx}


def upload(S, plane, pad=0, base_off=0, fill=0):
    """The plane in device memory with `pad` floats of garbage after every row and `base_off` bytes in front: (plane argument,
    pitch in bytes or 0).  The garbage is seeded by `fill`, so that two planes never share it."""
    h, w = plane.shape
    rng = np.random.default_rng(9000 + fill)
    host = rng.integers(0, 2 ** 32, size=(h, w + pad), dtype=np.uint64).astype(np.uint32)
    host[:, :w] = np.ascontiguousarray(plane, np.float32).view(np.uint32)
    raw = np.concatenate([np.full(base_off, fill & 0xff, np.uint8), host.reshape(-1).view(np.uint8)])
    buf = S.DeviceBuffer.from_numpy(raw)
    return (buf, base_off), (4 * (w + pad) if pad else 0)


def run_flags(geo, prev, cur, prev_layout=(0, 0), cur_layout=(0, 0)):
    """One srcnn_y_path_delta_flags_dev call into a guarded, canary-filled buffer: every flag byte is 0 or 1, no guard byte is
    touched.  prev None: no previous frame.  layout: (pad floats per row, base offset in bytes).  Returns the (rows, cols) flags."""
    S = geo.S
    n = geo.cols * geo.rows
    fbuf = S.DeviceBuffer.from_numpy(np.full(n + 2 * GUARD, CANARY, np.uint8))
    dprev, ppitch = upload(S, prev, prev_layout[0], prev_layout[1], fill=1) if prev is not None else (None, 0)
    dcur, cpitch = upload(S, cur, cur_layout[0], cur_layout[1], fill=2)
    S.y_path_delta_flags_dev(dprev, ppitch, dcur, cpitch, geo.w, geo.h, geo.dw, geo.dh, geo.filt, geo.tile, (fbuf, GUARD))
    S.sync()
    raw = fbuf.to_numpy(np.uint8, (n + 2 * GUARD,))
    assert np.all(raw[:GUARD] == CANARY) and np.all(raw[GUARD + n:] == CANARY), "a guard byte of the flag buffer was written"
    flags = raw[GUARD:GUARD + n].reshape(geo.rows, geo.cols)
    assert np.all(flags <= 1), "a flag byte is neither 0 nor 1"
    return flags


def changed(plane, points):
    """The plane with the lowest mantissa bit of every (x, y) of `points` flipped."""
    out = np.array(plane, np.float32, copy=True)
    v = out.view(np.uint32)
    for (x, y) in points:
        v[y, x] ^= 1
    return out


def check(geo, prev, cur, what, **layout):
    got = run_flags(geo, prev, cur, **layout)
    want = geo.expected(prev, cur)
    assert np.array_equal(got, want), "%s\ngot\n%s\nwant\n%s" % (what, got, want)
    return got


@pytest.fixture(scope="module")
def plane(srcnn):
    y = RW.frame_plane()
    y.setflags(write=False)
    return y


# ---- flags, exact ----
@pytest.mark.parametrize("tile", TILES)
def test_identical_planes_all_zero(srcnn, plane, tile):
    geo = Geo(srcnn, tile=tile)
    got = check(geo, plane, plane.copy(), "identical planes")
    assert not got.any()


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
def test_span_edges_of_every_tile_column_and_row(srcnn, plane, tile):
    geo = Geo(srcnn, tile=tile)
    launches = 0
    # columns: a change at lx, hx - 1 (inside: flags c), lx - 1, hx (outside: do not flag c), each in a source row of its own
    # whose tile rows no other change of the launch touches
    ycands = disjoint_batches(list(range(geo.h)), geo.rows_of)[0]          # source rows with pairwise disjoint tile rows
    assert len(ycands) >= 2
    cases = []                                                             # (x, tile column, flagged?)
    for c, (lx, hx) in enumerate(geo.xs):
        cases += [(lx, c, True), (hx - 1, c, True)]
        if lx > 0:
            cases.append((lx - 1, c, False))
        if hx < geo.w:
            cases.append((hx, c, False))
    assert any(not f for (_, _, f) in cases)
    for k in range(0, len(cases), len(ycands)):
        batch = list(zip(cases[k:k + len(ycands)], ycands))
        got = check(geo, plane, changed(plane, [(x, y) for ((x, _, _), y) in batch]), "column edges %r" % (batch,))
        launches += 1
        for ((x, c, flagged), y) in batch:
            rows = sorted(geo.rows_of(y))
            assert rows and all(bool(got[r, c]) == flagged for r in rows), "x = %d, tile column %d (span %r): %r" % (x, c, geo.xs[c], got[rows, c])
            assert all((got[r, :] != 0).tolist() == [cc in geo.cols_of(x) for cc in range(geo.cols)] for r in rows)
    # rows, the same way
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
        got = check(geo, plane, changed(plane, [(x, y) for ((y, _, _), x) in batch]), "row edges %r" % (batch,))
        launches += 1
        for ((y, r, flagged), x) in batch:
            cols = sorted(geo.cols_of(x))
            assert cols and all(bool(got[r, c]) == flagged for c in cols), "y = %d, tile row %d (span %r): %r" % (y, r, geo.ys[r], got[r, cols])
    assert launches <= 40


@pytest.mark.parametrize("tile", TILES)
def test_corners_seeded_sets_everything_and_no_previous_frame(srcnn, plane, tile):
    geo = Geo(srcnn, tile=tile)
    corners = [(0, 0), (W - 1, 0), (0, H - 1), (W - 1, H - 1)]
    for p in corners:
        got = check(geo, plane, changed(plane, [p]), "corner %r" % (p,))
        assert got.sum() == len(geo.rows_of(p[1])) * len(geo.cols_of(p[0])) > 0
    check(geo, plane, changed(plane, corners), "the four corners")
    rng = np.random.default_rng(424242)
    for n in (1, 3, 20):
        pts = [(int(rng.integers(0, W)), int(rng.integers(0, H))) for _ in range(n)]
        got = check(geo, plane, changed(plane, pts), "%d seeded samples %r" % (n, pts))
        assert got.any()
    every = changed(plane, [(x, y) for y in range(H) for x in range(W)])
    assert check(geo, plane, every, "every sample changed").all()
    assert run_flags(geo, None, plane).all(), "no previous frame: all ones"


def test_bit_patterns(srcnn, plane):
    geo = Geo(srcnn)
    prev = np.array(plane, np.float32, copy=True)
    cur = prev.copy()
    pv, cv = prev.view(np.uint32), cur.view(np.uint32)
    pv[5, 7], cv[5, 7] = 0x00000000, 0x80000000          # +0.0 against -0.0: equal as floats, different bits
    assert prev[5, 7] == cur[5, 7]
    got = check(geo, prev, cur, "+0.0 against -0.0")
    assert got.any()
    pv[5, 7] = cv[5, 7] = 0x7fc00001                     # the same NaN in both: unequal as floats, equal bits
    pv[40, 90] = cv[40, 90] = 0xffc12345
    assert prev[5, 7] != cur[5, 7]
    got = check(geo, prev, cur, "NaNs with equal bits")
    assert not got.any()
    cv[40, 90] = 0xffc12346                              # NaNs with different payloads
    got = check(geo, prev, cur, "NaNs with different payloads")
    assert got.sum() == len(geo.rows_of(40)) * len(geo.cols_of(90)) > 0


# ---- alignment and pitch ----
def test_vector_and_scalar_routes_give_the_same_flags(srcnn, plane):
    geo = Geo(srcnn)
    rng = np.random.default_rng(31337)
    pts = [(int(rng.integers(0, W)), int(rng.integers(0, H))) for _ in range(6)] + [(0, 0), (W - 1, H - 1), (3, 17), (4, 17), (W - 4, 30), (W - 5, 31)]
    cur = changed(plane, pts)
    same = plane.copy()
    layouts = {"tight, 16-byte aligned (vector)": dict(),
               "prev at +4 bytes (scalar)": dict(prev_layout=(0, 4)),
               "cur at +8 bytes (scalar)": dict(cur_layout=(0, 8)),
               "pitches of 16 n, different (vector)": dict(prev_layout=(4, 0), cur_layout=(12, 0)),
               "pitches of 4 n, different (scalar)": dict(prev_layout=(1, 0), cur_layout=(3, 0)),
               "both at +16 bytes, pitched (vector)": dict(prev_layout=(8, 16), cur_layout=(4, 16))}
    got = {name: check(geo, plane, cur, name, **lay) for name, lay in layouts.items()}
    first = got["tight, 16-byte aligned (vector)"]
    assert first.any() and not first.all()
    for name, g in got.items():
        assert np.array_equal(g, first), name
    # pitch padding holds different garbage in the two planes (upload seeds it per plane) and must not flag
    for name, lay in layouts.items():
        assert not check(geo, plane, same, name + ", identical", **lay).any(), name


def test_row_tails_where_w_is_no_multiple_of_4(srcnn):
    from libsrcnn_amd import synth
    w, h = 37, 23
    geo = Geo(srcnn, w, h, 74, 46, 2, (16, 16))
    assert (geo.cols, geo.rows) == (5, 3)
    prev = synth.plane(h, w, synth.SEED0 + 77, "noise")
    for pts in ([(36, 0)], [(36, 22)], [(35, 11)], [(32, 5), (36, 6)], [(0, 0), (33, 9), (34, 9), (36, 20)], []):
        cur = changed(prev, pts)
        tight = check(geo, prev, cur, "37 x 23 tight (pitch 148: scalar) %r" % (pts,))
        padded = check(geo, prev, cur, "37 x 23, pitch 160 (vector, with a row tail) %r" % (pts,), prev_layout=(3, 0), cur_layout=(3, 0))
        mixed = check(geo, prev, cur, "37 x 23, pitches 160 and 176 %r" % (pts,), prev_layout=(3, 0), cur_layout=(7, 0))
        assert np.array_equal(tight, padded) and np.array_equal(tight, mixed) and tight.any() == bool(pts)
    every = changed(prev, [(x, y) for y in range(h) for x in range(w)])
    assert check(geo, prev, every, "37 x 23, every sample", prev_layout=(3, 0), cur_layout=(3, 0)).all()


# ---- other geometry ----
@pytest.mark.parametrize("shape", [(96, 56, 240, 140, 3, (0, 0)), (96, 56, 96, 112, 2, (32, 16)), (96, 56, 192, 112, 0, (8, 8)), (50, 30, 37, 20, 2, (8, 8))],
                         ids=["2.5x-lanczos3-default-tiles", "columns-keep-their-size", "nearest-8x8", "down-scale"])
def test_other_geometry(srcnn, shape):
    from libsrcnn_amd import synth
    w, h, dw, dh, filt, tile = shape
    geo = Geo(srcnn, w, h, dw, dh, filt, tile)
    prev = synth.plane(h, w, synth.SEED0 + 78, "noise")
    rng = np.random.default_rng(555 + dw)
    assert not check(geo, prev, prev.copy(), "identical").any()
    for n in (1, 4, 25):
        pts = [(int(rng.integers(0, w)), int(rng.integers(0, h))) for _ in range(n)]
        check(geo, prev, changed(prev, pts), "%r: %d samples %r" % (shape, n, pts))
    for p in ((0, 0), (w - 1, h - 1), (w // 2, h // 2)):
        check(geo, prev, changed(prev, [p]), "%r: %r" % (shape, p))
    assert check(geo, prev, changed(prev, [(x, y) for y in range(h) for x in range(w)]), "every sample").all()


# ---- end to end, strict ----
class OutPlane:
    """A dw x dh output plane in device memory with `pad` floats after every row and a guard on each side, canary-filled or
    holding `init`."""

    def __init__(self, S, dw, dh, pad=0, init=None):
        self.S, self.dw, self.dh, self.stride = S, dw, dh, dw + pad
        self.pitch = 4 * self.stride if pad else 0
        body = np.full((dh, self.stride), np.frombuffer(bytes([CANARY] * 4), np.float32)[0], np.float32)
        if init is not None:
            body[:, :dw] = init
        raw = np.concatenate([np.full(GUARD, CANARY, np.uint8), body.reshape(-1).view(np.uint8), np.full(GUARD, CANARY, np.uint8)])
        self.buf = S.DeviceBuffer.from_numpy(raw)
        self.arg = (self.buf, GUARD)

    def fetch(self):
        """(plane, everything else as bytes)"""
        raw = self.buf.to_numpy(np.uint8, (self.buf.nbytes,))
        body = raw[GUARD:GUARD + 4 * self.stride * self.dh].view(np.float32).reshape(self.dh, self.stride)
        rest = np.concatenate([raw[:GUARD], raw[GUARD + 4 * self.stride * self.dh:], np.ascontiguousarray(body[:, self.dw:]).reshape(-1).view(np.uint8)])
        return body[:, :self.dw].copy(), rest


def delta(S, prev, cur, out, tile=(32, 16), filt=2, dw=DW, dh=DH):
    h, w = cur.shape
    dprev = S.DeviceBuffer.from_numpy(np.ascontiguousarray(prev, np.float32)) if prev is not None else None
    dcur = S.DeviceBuffer.from_numpy(np.ascontiguousarray(cur, np.float32))
    st = S.y_path_delta_dev(dprev, 0, dcur, 0, w, h, dw, dh, filt, tile, out.arg, out.pitch)
    S.sync()
    return st


def stats_tuple(st):
    return st.tiles, st.dirty_tiles, st.rects, st.whole_frame, st.cell_samples


@pytest.mark.parametrize("point, want_stats, rect", [((48, 28), (42, 6, 1, 0, 4560), (64, 32, 64, 48)), ((20, 10), (42, 4, 1, 0, 3344), (0, 0, 64, 32))])
@pytest.mark.parametrize("pad", [0, 8], ids=["tight", "pitched"])
def test_canary_repaint(srcnn, oracle_lib, plane, point, want_stats, rect, pad):
    S = srcnn
    assert S.lib().srcnn_get_mode() == S.MODE_STRICT
    cur = changed(plane, [point])
    out = OutPlane(S, DW, DH, pad=pad)
    st = delta(S, plane, cur, out)
    assert st.struct_size == C.sizeof(S.DeltaStats)
    assert stats_tuple(st) == want_stats                  # (the route is asserted here: the cells are under a quarter of dw * dh)
    assert st.cell_samples * 4 < DW * DH
    got, rest = out.fetch()
    x0, y0, rw, rh = rect
    want = oracle_lib.y_path(cur)
    assert_bit_equal(got[y0:y0 + rh, x0:x0 + rw], want[y0:y0 + rh, x0:x0 + rw], "the dirty tiles of a change at %r" % (point,))
    mask = np.ones((DH, DW), bool)
    mask[y0:y0 + rh, x0:x0 + rw] = False
    assert np.all(got.view(np.uint8).reshape(DH, DW, 4)[mask] == CANARY), "a sample of a clean tile was written"
    assert np.all(rest == CANARY), "a guard or padding byte was written"
    # the dirty tiles are exactly the restatement's
    geo = Geo(S)
    e = geo.expected(plane, cur)
    assert e.sum() == want_stats[1] and e[y0 // 16:(y0 + rh) // 16, x0 // 32:(x0 + rw) // 32].all()


def test_sequence_of_frames(srcnn, oracle_lib, plane):
    S = srcnn
    frames = [np.array(plane, np.float32, copy=True)]

    def with_block(x, y):
        f = np.array(plane, np.float32, copy=True)
        f[y:y + 5, x:x + 5] = 1.0 - f[y:y + 5, x:x + 5]
        return f
    frames += [with_block(10, 8), with_block(10, 8), with_block(60, 30)]          # the block appears, stays, moves
    want = {}
    out = OutPlane(S, DW, DH, init=oracle_lib.y_path(frames[0]))
    for k in (1, 2, 3):
        st = delta(S, frames[k - 1], frames[k], out)
        key = frames[k].tobytes()
        if key not in want:
            want[key] = oracle_lib.y_path(frames[k])
        got, rest = out.fetch()
        assert_bit_equal(got, want[key], "frame %d" % k)
        assert np.all(rest == CANARY)
        e = Geo(S).expected(frames[k - 1], frames[k])
        assert st.dirty_tiles == e.sum() and st.tiles == 42
        if k == 2:
            assert st.rects == 0 and st.dirty_tiles == 0 and st.whole_frame == 0 and st.cell_samples == 0
        else:
            assert 1 <= st.rects <= st.dirty_tiles
    # the numpy convenience gives the same plane
    got, st = S.y_path_delta(frames[2], frames[3], want[frames[2].tobytes()], DW, DH, 2, (32, 16))
    assert_bit_equal(got, want[frames[3].tobytes()], "y_path_delta")
    assert st.rects >= 1


def test_every_sample_changed_takes_the_whole_frame(srcnn, oracle_lib, plane):
    S = srcnn
    cur = changed(plane, [(x, y) for y in range(H) for x in range(W)])
    want = oracle_lib.y_path(cur)
    for prev in (plane, None):                           # every tile dirty; no previous frame
        out = OutPlane(S, DW, DH, pad=4)
        st = delta(S, prev, cur, out, tile=(0, 0))
        assert st.whole_frame == 1 and st.tiles == st.dirty_tiles == 6 and st.rects == 1 and st.cell_samples == (DW + 12) * (DH + 12)
        got, rest = out.fetch()
        assert_bit_equal(got, want, "whole frame")
        assert np.all(rest == CANARY)


# ---- capture ----
def test_a_stream_under_the_callers_capture_is_refused(srcnn, plane):
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
    cur = changed(plane, [(48, 28)])
    dprev = S.DeviceBuffer.from_numpy(np.ascontiguousarray(plane))
    dcur = S.DeviceBuffer.from_numpy(cur)
    out = OutPlane(S, DW, DH)
    raw = vp()
    assert hip.hipStreamCreateWithFlags(C.byref(raw), 1) == 0          # hipStreamNonBlocking
    try:
        # once eagerly on this stream: whatever the call keeps per stream exists before the capture begins
        st = S.y_path_delta_dev(dprev, 0, dcur, 0, W, H, DW, DH, 2, (32, 16), out.arg, out.pitch, raw.value)
        assert hip.hipStreamSynchronize(raw) == 0 and st.rects == 1
        out = OutPlane(S, DW, DH)
        graph = vp()
        assert hip.hipStreamBeginCapture(raw, 2) == 0                  # hipStreamCaptureModeRelaxed
        try:
            with pytest.raises(S.SrcnnError) as e:
                S.y_path_delta_dev(dprev, 0, dcur, 0, W, H, DW, DH, 2, (32, 16), out.arg, out.pitch, raw.value)
        finally:
            rc = hip.hipStreamEndCapture(raw, C.byref(graph))
        assert e.value.code == E_UNSUPPORTED
        assert rc == 0 and graph.value, "the capture did not end cleanly (%d)" % rc
        n = C.c_size_t(99)
        assert hip.hipGraphGetNodes(graph, None, C.byref(n)) == 0 and n.value == 0, "%d nodes were captured" % n.value
        hip.hipGraphDestroy(graph)
        assert hip.hipStreamSynchronize(raw) == 0
        got, rest = out.fetch()
        assert np.all(got.view(np.uint8) == CANARY) and np.all(rest == CANARY)
    finally:
        hip.hipStreamDestroy(raw)
