"""srcnn_yuv_packed_upscale_rect_dev (include/srcnn_amd_yuv_packed_rect.h) byte for byte against crops of the whole frame (GPU).

A rect is rh row segments of what srcnn_yuv_packed_upscale_dev writes -- the bytes srcnn_yuv_packed_span_bytes gives for its
columns -- so every expectation is a crop of the whole-frame expectation of tests/test_gpu_yuv_packed.py (want_for() / pack(): the
oracle composition), computed once per frame, and of the library's own whole-frame call.  Never the call under test.  Rect edges
sit at and next to both borders, around the 6-sample halo and the 16 / 64 / 128 tile edges; origins are snapped down to the
format's unit and the far edge up to the unit or to the right border; small shapes throughout; the positions the edge rule leaves
open rotate with the session seed.  Every process these tests start runs under a timeout of its own and nothing is tried twice.
"""
import hashlib
import json
import os
import subprocess
import sys
import threading

import numpy as np
import pytest

import yuv_packed_rect_worker as W
from conftest import rotating_seed
from test_gpu_rect import edge_rects
from test_gpu_yuv import FILTER_NAMES, FILTERS, first_difference, out_size
from test_gpu_yuv_ex import expected
from test_gpu_yuv_packed import FORMATS, NAMES, alpha_expected, cases_for, frame_planes, pack, row_bytes, unpack, want_for
from yuv_packed_rect_worker import EDGE_SHAPES, UNIT, Rig, crop, snap, span

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORKER = os.path.join(ROOT, "tests", "yuv_packed_rect_worker.py")
CANARY = 0xA5
GUARD = 256


def seed():
    return rotating_seed("rect positions of tests/test_gpu_yuv_packed_rect.py")


def assert_bytes(got, want, what):
    assert got.dtype == np.uint8 and got.shape == want.shape, (what, got.shape, want.shape)
    assert np.array_equal(got, want), "%s: %s" % (what, first_difference(got, want))


def name_of(r):
    return "rect %dx%d at (%d,%d)" % (r[2], r[3], r[0], r[1])


_ORACLE = {}


def oracle_frame(oracle_lib, name, planes, mul, filt, key):
    """pack() of the oracle composition for one frame, computed once per (chroma, depth, alpha depth, key) and packed per format."""
    _id, chroma, depth, adepth, _al = FORMATS[name]
    k = (chroma, depth, adepth, key)
    if k not in _ORACLE:
        Y, U, V, A = planes
        yuv = expected(oracle_lib, Y, U, V, chroma, depth, mul, filt)
        _ORACLE[k] = tuple(yuv) + ((alpha_expected(oracle_lib, A, adepth, mul, filt),) if adepth else (None,))
    return pack(name, *_ORACLE[k])


def test_the_restated_span_is_the_librarys(srcnn):
    for name in NAMES:
        for width in (1, 2, 5, 6, 7, 47, 48, 49, 87, 97, 140):
            u = UNIT[name]
            for x in range(0, width, u):
                for n in {u, 2 * u, width - x}:
                    if x + n <= width and (n % u == 0 or x + n == width):
                        assert srcnn.yuv_packed_span_bytes(name, width, x, n) == (u,) + span(name, width, x, n), (name, width, x, n)
            assert span(name, width, 0, width) == (0, row_bytes(name, width))


# ---- edges: 70 x 40 -> 140 x 80 (2x) and 35 x 20 -> 87 x 50 (2.5x), bicubic ----
_EDGE_DIGEST = {}


@pytest.mark.parametrize("shape", EDGE_SHAPES, ids=["140x80", "87x50"])
@pytest.mark.parametrize("name", NAMES)
def test_edges_vs_oracle_and_whole_frame(srcnn, oracle_lib, name, shape):
    w, h, mul, filt = shape
    dw, dh = out_size(w, h, mul)
    assert (dw, dh) == ((140, 80) if w == 70 else (87, 50)) and 140 % 6 and row_bytes("v210", 140) == 3 * 128
    planes = frame_planes(name, w, h, 7040 + w)
    want = oracle_frame(oracle_lib, name, planes, mul, filt, ("edge", w))
    src = W.edge_source(name, shape)
    assert np.array_equal(src, pack(name, *planes))
    whole = srcnn.yuv_packed_upscale(src, name, w, multiply=mul, filt=filt)
    assert_bytes(whole, want, "whole frame vs oracle")
    rig = Rig(srcnn, name, src, w, mul, filt)
    rects = W.edge_case_rects(seed(), name, dw, dh)
    assert len(set(rects)) == len(rects) >= 150, len(rects)
    assert sum(1 for r in rects if r[0] + r[2] == dw) >= 20
    assert sum(1 for r in rects if r[0] + r[2] < dw) >= 100
    sha = hashlib.sha256()
    for r in rects:
        got = rig.raw(*r)
        sha.update(got.tobytes())
        assert_bytes(got, crop(want, r, name, dw), "%s %s vs oracle" % (name, name_of(r)))
        assert_bytes(got, crop(whole, r, name, dw), "%s %s vs the library's whole frame" % (name, name_of(r)))
    _EDGE_DIGEST[W.digest_key(name, shape)] = sha.hexdigest()


# ---- the matrix: one rotating case per format ----
def matrix_case(name):
    cases = list(cases_for(name))
    return cases[(2 * FORMATS[name][0] + 5) % len(cases)]


MATRIX = {name: matrix_case(name) for name in NAMES}
_SHAPES = [(w, h) + out_size(w, h, m) for (w, h, _f, m) in MATRIX.values()]
assert {c[2] for c in MATRIX.values()} == set(FILTERS), "not all five filters"
assert any(dw > w and dh > h for (w, h, dw, dh) in _SHAPES), "no up-scale in both axes"
assert any(dw < w and dh < h for (w, h, dw, dh) in _SHAPES), "no down-scale"
assert any((dw == w) != (dh == h) for (w, h, dw, dh) in _SHAPES), "no case with one axis kept and the other resampled"


def matrix_rects(name, dw, dh, rng):
    limit = 8 if min(dw, dh) > 8 else None               # (a one-pixel-wide output has one pair of x edges: all pairs of the other axis then)
    rects = edge_rects(dw, dh, rng, limit=limit) + [(0, 0, dw, dh), (dw - 1, dh - 1, 1, 1), (dw // 2, dh // 2, 1, 1), (0, dh - 1, dw, 1), (dw - 1, 0, 1, dh)]
    return sorted({snap(r, name, dw) for r in rects})


@pytest.mark.parametrize("name", NAMES)
def test_matrix_vs_oracle(srcnn, oracle_lib, name):
    case = MATRIX[name]
    w, h, filt, mul = case
    dw, dh = out_size(w, h, mul)
    rects = matrix_rects(name, dw, dh, np.random.default_rng(seed() + FORMATS[name][0]))
    assert len(rects) >= 12, (name, case, len(rects))
    want = pack(name, *want_for(oracle_lib, name, case))
    rig = Rig(srcnn, name, pack(name, *frame_planes(name, w, h, 100 * w + h)), w, mul, filt)
    for r in rects:
        assert_bytes(rig.raw(*r), crop(want, r, name, dw), "%s %dx%d %s x%g %s" % (name, w, h, FILTER_NAMES[filt], mul, name_of(r)))


# ---- the identity size: chroma and alpha are copied; crops of the library's whole-frame call ----
@pytest.mark.parametrize("name", NAMES)
def test_identity_size_gives_crops_of_the_whole_frame_call(srcnn, name):
    S = srcnn
    rng = np.random.default_rng(seed() + 31)
    for k, (w, h) in enumerate(((23, 17), (64, 40), (9, 7), (1, 5), (130, 66))):
        filt = FILTERS[(k + FORMATS[name][0]) % 5]
        src = pack(name, *frame_planes(name, w, h, 3 * w + h))
        whole = S.yuv_packed_upscale(src, name, w, multiply=1.0, filt=filt)
        for a, b in zip(unpack(name, whole, w)[1:], unpack(name, src, w)[1:]):      # chroma and alpha are copied at the identity size
            assert (a is None and b is None) or np.array_equal(a, b)
        rig = Rig(S, name, src, w, 1.0, filt)
        rects = edge_rects(w, h, rng, limit=3) + [(0, 0, w, h), (w - 1, h - 1, 1, 1), (w // 2, h // 2, 1, 1)]
        for r in sorted({snap(r, name, w) for r in rects}):
            assert_bytes(rig.raw(*r), crop(whole, r, name, w), "identity %s %dx%d f%d %s" % (name, w, h, filt, name_of(r)))


# ---- repaint in place: the rect inside a full-size packed frame filled with a canary ----
REPAINT_CASES = [(23, 17, 2, 2.0), (30, 11, 3, 1.5), (33, 20, 4, 0.75), (52, 9, 2, 2.0)]


def repaint_rects(name, dw, dh):
    """One unit, the right border at a partial unit, the bottom row, the whole frame, interior rects that stop short of dw (for
    v210: inside a 128-byte block, so that the groups up to the block's end must keep the canary)."""
    u = UNIT[name]
    rects = [(u, 1, u, 1), (0, 0, u, dh), (dw - 1, 2, 1, 3), (0, dh - 1, dw, 1), (0, 0, dw, dh), (u, 2, 2 * u, 3), (2 * u, 0, dw - 2 * u, dh),
             (3, 1, 7, 5), (6, 3, 12, 2)]
    return sorted({snap(r, name, dw) for r in rects if r[0] + r[2] <= dw and r[1] + r[3] <= dh and r[2] > 0 and r[3] > 0})


@pytest.mark.parametrize("name", ["yuy2", "y212", "vuya", "y410", "v210"])
@pytest.mark.parametrize("offset,pad", [(1, 1), (3, 7), (6, 14), (0, 0), (0, 16)])
@pytest.mark.parametrize("w,h,filt,mul", REPAINT_CASES)
def test_repaint_in_place_vs_oracle(srcnn, oracle_lib, name, offset, pad, w, h, filt, mul):
    """The destination is a full-size dw x dh packed frame of canary bytes between guards; the call gets the address of the rect's
    first byte and the frame's pitch.  The row segments hold the oracle's crop; every other byte -- the rest of the frame, the row
    padding, the guards, the source -- is unchanged."""
    S = srcnn
    align = FORMATS[name][4]
    offset, pad = align * offset, align * pad              # the pairs of the planar repaint test, raised to the format's alignment
    planes = frame_planes(name, w, h, 7 * w + h)
    src = pack(name, *planes)
    want = oracle_frame(oracle_lib, name, planes, mul, filt, ("repaint", w, h, filt, mul))
    dw, dh = out_size(w, h, mul)
    rbs = [src.shape[1], want.shape[1]]
    rows = [h, dh]
    pitches = [rb + (pad + 4 * align * k if pad else 0) for k, rb in enumerate(rbs)]
    pos, bases = 0, []
    for r, p in zip(rows, pitches):
        pos = (pos + GUARD + 63) // 64 * 64 + offset
        bases.append(pos)
        pos += p * r
    total = pos + GUARD
    host = np.full(total, CANARY, np.uint8)
    for r in range(h):
        host[bases[0] + r * pitches[0]: bases[0] + r * pitches[0] + rbs[0]] = src[r]
    rects = repaint_rects(name, dw, dh)
    assert any(r[2] == UNIT[name] for r in rects) and any(r[0] + r[2] == dw and r[2] <= UNIT[name] for r in rects) and any(r[1] + r[3] == dh and r[3] == 1 for r in rects)
    short = 0
    for rect in rects:
        x0, y0, rw, rh = rect
        off, n = span(name, dw, x0, rw)
        first = bases[1] + y0 * pitches[1] + off
        buf = S.DeviceBuffer.from_numpy(host)
        S.yuv_packed_upscale_rect_dev(name, w, h, mul, filt, (buf, bases[0]), pitches[0], x0, y0, rw, rh, (buf, first), pitches[1])
        S.sync()
        back = buf.to_numpy(np.uint8, (total,))
        expect = host.copy()
        for r in range(rh):
            expect[first + r * pitches[1]: first + r * pitches[1] + n] = want[y0 + r, off:off + n]
        if not np.array_equal(back, expect):
            bad = np.flatnonzero(back != expect)
            where = "output frame" if bases[1] <= bad[0] < bases[1] + pitches[1] * dh else "input frame or guard"
            raise AssertionError("%s %s: %d bytes differ, first at byte %d (%s, byte %d of its row): got %d want %d" %
                                 (name, name_of(rect), len(bad), bad[0], where, (bad[0] - bases[1]) % pitches[1], back[bad[0]], expect[bad[0]]))
        if name == "v210" and x0 + rw < dw and (off + n) % 128:
            short += 1                                      # the groups between the rect's last one and the block's end kept the canary
            assert np.all(back[first + n: first - off + (off + n + 127) // 128 * 128] == CANARY)
    assert name != "v210" or short >= 2


# ---- source locality ----
@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("w,h,mul,filt", [(70, 40, 2.0, 2), (40, 31, 1.5, 3), (50, 30, 0.75, 2), (3, 40, 1.5, 2)],
                         ids=["2x-bicubic", "1.5x-lanczos3", "downscale-bicubic", "w3-mixed"])
def test_nothing_outside_the_source_rectangle_is_used(srcnn, oracle_lib, name, w, h, mul, filt):
    """Two source frames that agree on the bytes srcnn_yuv_packed_span_bytes gives for the rectangle srcnn_yuv_packed_rect_source
    reports and differ in every other byte give the same bytes: the crop.  (3 x 40 x 1.5 -> 4 x 60: the 4:2:2 formats keep their 2
    chroma columns while the rows are resampled.)"""
    S = srcnn
    dw, dh = out_size(w, h, mul)
    if w == 3 and FORMATS[name][1] == "422":
        assert (w + 1) // 2 == (dw + 1) // 2 and h != dh
    rng = np.random.default_rng(seed() + 77)
    planes = frame_planes(name, w, h, 9 * w + h)
    src = pack(name, *planes)
    want = oracle_frame(oracle_lib, name, planes, mul, filt, ("local", w, h, mul, filt))
    rects = edge_rects(dw, dh, rng, limit=5) + [(dw // 2, dh // 2, 1, 1), (0, 0, min(9, dw), 9), (max(0, dw - 9), dh - 9, min(9, dw), 9)]
    rects = sorted({snap(r, name, dw) for r in rects})
    assert len(rects) >= 9
    need = 9 if w > 3 else 5

    def smaller_than_the_frame(r):
        _sx0, _sy0, sw_, sh_ = S.yuv_packed_rect_source(name, w, h, mul, filt, *r)
        return S.yuv_packed_span_bytes(name, w, _sx0, sw_)[2] * sh_ < src.size

    # The drawn edge pairs may span the frame (both lists hold 0 and the far border; a wide filter or a down-scale reaches the
    # rest), and such a rect proves nothing here: one session seed in about 250 drew too few of the others for a case.  More rects
    # are drawn, never fewer, until the count below can hold; the bound itself stays.
    for _ in range(8):
        if sum(smaller_than_the_frame(r) for r in rects) >= need:
            break
        rects = sorted(set(rects) | {snap(r, name, dw) for r in edge_rects(dw, dh, rng, limit=5)})
    shrunk = 0
    a_rig = Rig(S, name, src, w, mul, filt)
    for r in rects:
        sx0, sy0, sw, sh = S.yuv_packed_rect_source(name, w, h, mul, filt, *r)
        assert sx0 + sw <= w and sy0 + sh <= h and sw and sh
        _u, off, n = S.yuv_packed_span_bytes(name, w, sx0, sw)
        other = rng.integers(0, 256, src.shape).astype(np.uint8)
        other[sy0:sy0 + sh, off:off + n] = src[sy0:sy0 + sh, off:off + n]
        shrunk += int(n * sh < src.size)
        a = a_rig.raw(*r)
        b = Rig(S, name, other, w, mul, filt).raw(*r)
        assert_bytes(b, a, "%s source replaced outside its rectangle, %s" % (name, name_of(r)))
        assert_bytes(a, crop(want, r, name, dw), "%s %s" % (name, name_of(r)))
    assert shrunk >= need                         # the test has teeth: most source rectangles are smaller than the frame (w = 3: in rows only)


# ---- both routes: k_yuvp_window_merge and the plane route over the window give the same bytes ----
def child(mode, arg, env=None, timeout=600):
    r = subprocess.run([sys.executable, WORKER, mode, str(arg)], env=dict(os.environ, **(env or {})), capture_output=True, text=True, timeout=timeout)
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")]
    assert r.returncode == 0 and line, "yuv_packed_rect_worker %s: exit %d\n%s\n%s" % (mode, r.returncode, r.stdout[-600:], r.stderr[-1500:])
    return json.loads(line[0][7:])


def test_forced_plane_route_gives_the_same_bytes(srcnn):
    """SRCNN_YUV_PACKED_RECT_UNFUSED=1 (read when the library loads) sends up-scales down the plane route as well.  The default
    route's bytes of the same rects are held to the oracle by test_edges_vs_oracle_and_whole_frame, whose digests are reused when
    it ran in this session."""
    S = srcnn
    assert "SRCNN_YUV_PACKED_RECT_UNFUSED=0" in S.debug_settings()
    fast = {}
    for name in NAMES:
        for shape in EDGE_SHAPES:
            key = W.digest_key(name, shape)
            fast[key] = _EDGE_DIGEST.get(key) or W.edge_digest(S, seed(), name, shape)
    assert child("unfused", seed(), env={"SRCNN_YUV_PACKED_RECT_UNFUSED": "1"}) == fast


# ---- banding ----
@pytest.mark.parametrize("name", ["yuy2", "y416", "v210"])
def test_banded_rect_gives_the_same_bytes(srcnn, oracle_lib, name):
    S = srcnn
    L = S.lib()
    shape = EDGE_SHAPES[0]
    w, h, mul, filt = shape
    want = oracle_frame(oracle_lib, name, frame_planes(name, w, h, 7040 + w), mul, filt, ("edge", w))
    rig = W.edge_rig(S, name, shape)
    limit = 1 << 20
    # the window of these rects is all 140 columns: 32 planes x 4 B x 140 x (80 + 4) rows do not fit 1 MB, 54-row bands do
    assert 32 * 4 * 140 * (80 + 4) > limit
    band_rows = limit // (32 * 4 * 140) - 4
    bands = -(-80 // band_rows)
    assert bands >= 2
    rects = [(0, 0, 140, 80), (6, 0, 134, 80), (0, 0, 138, 80)]
    unbanded = [rig.raw(*r) for r in rects]
    prev = L.srcnn_set_workspace_limit(limit)
    S.profile_enable(True)
    try:
        for r, ref in zip(rects, unbanded):
            S.profile_reset()
            got = rig.raw(*r)
            launches = S.profile_read()["conv12"][1]
            assert launches == bands, (r, launches, bands)
            assert_bytes(got, ref, "banded vs unbanded %s" % name_of(r))
            assert_bytes(got, crop(want, r, name, 140), "banded %s vs oracle" % name_of(r))
    finally:
        S.profile_enable(False)
        L.srcnn_set_workspace_limit(prev)


# ---- non-parity modes: Y' is the integer conversion of the mode's own y_path_rect, everything else is the strict bytes ----
@pytest.mark.parametrize("mode_name", ["MODE_FAST", "MODE_FAST_F16", "MODE_RELAXED"])
def test_non_parity_modes_are_exact_around_their_y(srcnn, oracle_lib, mode_name):
    S = srcnn
    rng = np.random.default_rng(seed() + 5)
    prev = S.set_mode(getattr(S, mode_name))        # (a strict-only build refuses: conftest turns that into a skip)
    try:
        for (name, w, h, mul, filt) in (("yuy2", 70, 40, 2.0, 2), ("y212", 40, 31, 1.5, 3), ("y410", 50, 30, 0.75, 1), ("v210", 70, 40, 2.0, 2)):
            _id, _chroma, depth, _adepth, _al = FORMATS[name]
            dw, dh = out_size(w, h, mul)
            planes = frame_planes(name, w, h, 13 * w + h)
            strict = oracle_frame(oracle_lib, name, planes, mul, filt, ("modes", w, h, mul, filt))
            _sy, su, sv, sa = unpack(name, strict, dw)
            s = depth - 8
            yf = planes[0].astype(np.float32) * np.float32(2.0 ** -s)
            rig = Rig(S, name, pack(name, *planes), w, mul, filt)
            for r in sorted({snap(r, name, dw) for r in edge_rects(dw, dh, rng, limit=4) + [(0, 0, dw, dh), (dw // 2, dh // 2, 1, 1)]}):
                x0, y0, rw, rh = r
                yp = np.zeros((dh, dw), planes[0].dtype)
                yp[y0:y0 + rh, x0:x0 + rw] = (S.y_path_rect(yf, dw, dh, filt, *r) * np.float32(2.0 ** s)).astype(np.uint32).astype(planes[0].dtype)
                want = pack(name, yp, su, sv, sa)
                assert_bytes(rig.raw(*r), crop(want, r, name, dw), "%s %s %dx%d x%g %s" % (mode_name, name, w, h, mul, name_of(r)))
    finally:
        S.set_mode(prev)


# ---- stray bits ----
@pytest.mark.parametrize("name", ["yuy2", "y210", "y216", "v210"])
def test_stray_bits_do_not_change_a_rect(srcnn, name):
    S = srcnn
    w, h, mul, filt = 37, 12, 2.0, 2
    dw, dh = out_size(w, h, mul)
    planes = frame_planes(name, w, h, 77)
    clean = pack(name, *planes)
    dirty = pack(name, *planes, junk=np.random.default_rng(9))
    assert not np.array_equal(clean, dirty)
    a, b = Rig(S, name, clean, w, mul, filt), Rig(S, name, dirty, w, mul, filt)
    for r in sorted({snap(r, name, dw) for r in ((0, 0, dw, dh), (6, 2, 30, 9), (dw - 5, dh - 3, 5, 3), (60, 0, 14, dh))}):
        assert_bytes(b.raw(*r), a.raw(*r), "%s %s" % (name, name_of(r)))


# ---- the numpy convenience of the binding ----
@pytest.mark.parametrize("name", ["uyvy", "y210", "y416", "v210"])
def test_numpy_convenience_returns_the_rects_row_segments(srcnn, name):
    S = srcnn
    w, h, mul, filt = 37, 21, 2.5, 3
    src = pack(name, *frame_planes(name, w, h, 77))
    whole = S.yuv_packed_upscale(src, name, w, multiply=mul, filt=filt)
    assert whole.shape == (52, row_bytes(name, 92))
    for rect in ((0, 0, 92, 52), (6, 4, 42, 23), (90, 50, 2, 2)):
        got = S.yuv_packed_upscale_rect(src, name, w, rect, multiply=mul, filt=filt)
        want = crop(whole, rect, name, 92)
        assert got.dtype == np.uint8 and got.shape == want.shape == (rect[3], span(name, 92, rect[0], rect[2])[1]) and np.array_equal(got, want), (name, rect)
    with pytest.raises(S.SrcnnError):
        S.yuv_packed_upscale_rect(src, name, w, (0, 0, 0, 5), multiply=mul, filt=filt)
    if UNIT[name] > 1:
        with pytest.raises(S.SrcnnError):
            S.yuv_packed_upscale_rect(src, name, w, (1, 0, UNIT[name], 5), multiply=mul, filt=filt)
    with pytest.raises(ValueError):
        S.yuv_packed_upscale_rect(src[:, :-4], name, w, (0, 0, 2, 2), multiply=mul, filt=filt)


# ---- two host threads on two streams, different rects of different formats ----
def test_two_threads_two_streams(srcnn):
    S = srcnn
    cases = [(NAMES[k], 2.0 if k % 3 else 1.5, FILTERS[k % 5]) for k in range(10)]
    frames = [pack(c[0], *frame_planes(c[0], 97, 61, 500 + k)) for k, c in enumerate(cases)]
    rigs = [Rig(S, c[0], frames[k], 97, c[1], c[2]) for k, c in enumerate(cases)]
    rects = [snap((3 + 4 * k, 2 + 3 * k, 50 + 5 * k, 31 + 3 * k), cases[k][0], rigs[k].dw) for k in range(10)]     # inside the smallest output, 145 x 91
    whole = [S.yuv_packed_upscale(frames[k], c[0], 97, multiply=c[1], filt=c[2]) for k, c in enumerate(cases)]
    results, errors = [None] * 10, []

    def worker(t):
        st = S.Stream()
        try:
            for k in range(t, 10, 2):
                results[k] = rigs[k].raw(*rects[k], stream=st)
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
    assert all(r[0] + r[2] <= 145 and r[1] + r[3] <= 91 for r in rects)
    for k in range(10):
        assert_bytes(results[k], crop(whole[k], rects[k], cases[k][0], rigs[k].dw), "%s frame %d on thread %d, %s" % (cases[k][0], k, k % 2, name_of(rects[k])))


# ---- one real size ----
@pytest.mark.parametrize("name", ["v210", "y410"])
def test_1080p_to_4k_interior_and_corner(srcnn, name):
    """1920 x 1080 -> 3840 x 2160: an interior 258 x 128 rect, an interior rect that ends at a partial tile, and the bottom-right
    255 x 127 samples with the origin snapped down to the unit.  Crops of the library's whole-frame call (held to the planar
    call, and through it to the oracle, by tests/test_gpu_yuv_packed.py)."""
    S = srcnn
    w, h = 1920, 1080
    src = pack(name, *frame_planes(name, w, h, 4242))
    whole = S.yuv_packed_upscale(src, name, w, multiply=2.0, filt=2)
    rig = Rig(S, name, src, w, 2.0, 2)
    if UNIT[name] > 1:
        with pytest.raises(S.SrcnnError):
            rig.raw(3840 - 255, 2160 - 127, 255, 127)
    for r in ((1602, 902, 258, 128), snap((1602, 904, 255 + 61, 127 + 9), name, 3840), snap((3840 - 255, 2160 - 127, 255, 127), name, 3840)):
        assert_bytes(rig.raw(*r), crop(whole, r, name, 3840), "%s %s of 3840x2160" % (name, name_of(r)))
