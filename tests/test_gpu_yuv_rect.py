"""srcnn_yuv_upscale_rect_dev (include/srcnn_amd_yuv_rect.h) byte for byte against crops of the whole frame (GPU).

A rect is a crop of what srcnn_yuv_upscale_dev writes -- the luma rect, and the chroma samples that cover it -- so every
expectation is a crop of the whole-frame expectation of tests/test_gpu_yuv_ex.py (expected() / want_for(): the oracle
composition), computed once per frame, and, where the contract names it, a crop of the library's own whole-frame call.  Never
the call under test.  Rect edges sit at and next to both borders, around the 6-sample halo and the 16 / 64 tile sizes; origins
are snapped down to even where the format demands it and the far edge is kept; small shapes throughout; the positions the
edge rule leaves open rotate with the session seed.  Every process these tests start runs under a timeout of its own and
nothing is tried twice.
"""
import json
import os
import subprocess
import sys
import threading

import numpy as np
import pytest

import yuv_rect_worker as W
from conftest import rotating_seed
from test_gpu_rect import edge_rects
from test_gpu_yuv import FILTER_NAMES, FILTERS, first_difference, out_size
from test_gpu_yuv_ex import (CHROMAS, LAYOUTS, WORDS, cases_for, chroma_size, expected, frame, layout_bases, run, to_words,
                             want_for)
from yuv_rect_worker import EDGE_CELLS, Rig, chroma_rect, snap

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORKER = os.path.join(ROOT, "tests", "yuv_rect_worker.py")
CANARY = 0xA5


def seed():
    return rotating_seed("rect positions of tests/test_gpu_yuv_rect.py")


def crop(planes, rect, chroma):
    """The rect of a whole frame's (Y', U', V'): the luma rect and the chroma samples that cover it."""
    x0, y0, rw, rh = rect
    cx0, cy0, crw, crh = chroma_rect(rect, chroma)
    return (planes[0][y0:y0 + rh, x0:x0 + rw], planes[1][cy0:cy0 + crh, cx0:cx0 + crw], planes[2][cy0:cy0 + crh, cx0:cx0 + crw])


def assert_rect(got, want, what):
    for name, g, e in zip("YUV", got, want):
        assert g.shape == e.shape and g.dtype == e.dtype, (what, name, g.shape, e.shape, g.dtype, e.dtype)
        assert np.array_equal(g, e), "%s %s': %s" % (what, name, first_difference(g, e))


def name_of(r):
    return "rect %dx%d at (%d,%d)" % (r[2], r[3], r[0], r[1])


# ---- edges: 70 x 40 -> 140 x 80, 2x bicubic ----
_EDGE_DIGEST = {}


@pytest.mark.parametrize("cell", EDGE_CELLS, ids=["i420", "p210-422", "planar444-16"])
def test_edges_vs_oracle_and_whole_frame(srcnn, oracle_lib, cell):
    import hashlib
    layout, chroma, depth, msb = cell
    w, h, mul, filt = W.EDGE_SHAPE
    Y, U, V = frame(w, h, chroma, depth, 7040 + depth)
    want = expected(oracle_lib, Y, U, V, chroma, depth, mul, filt)
    whole = run(srcnn, LAYOUTS[layout], chroma, depth, msb, Y, U, V, mul, filt)
    assert_rect(whole, want, "whole frame vs oracle")
    rig = W.edge_rig(srcnn, cell)
    rects = W.edge_case_rects(seed(), chroma)
    assert len(set(rects)) == len(rects) >= 370, len(rects)
    assert sum(1 for r in rects if r[2] % 2 or r[3] % 2) >= 250
    sha = hashlib.sha256()
    for r in rects:
        raw = rig.raw(*r)
        for p in raw:
            sha.update(np.ascontiguousarray(p).tobytes())
        got = rig.to_values(raw)
        assert_rect(got, crop(want, r, chroma), name_of(r) + " vs oracle")
        assert_rect(got, crop(whole, r, chroma), name_of(r) + " vs the library's whole frame")
    _EDGE_DIGEST[cell] = sha.hexdigest()


# ---- the matrix: one case per format cell, rotating through the cell's cases ----
CELLS = [(l, c, wd) for l in LAYOUTS for c in CHROMAS for wd in WORDS]


def matrix_case(cell):
    cases = list(cases_for(*cell))
    return cases[(3 * CELLS.index(cell) + 1) % len(cases)]


MATRIX = [(cell, matrix_case(cell)) for cell in CELLS]
assert len(MATRIX) == 54 and {c[1][2] for c in MATRIX} == set(FILTERS)
_SHAPES = [(cell[1], w, h) + out_size(w, h, m) for (cell, (w, h, _f, m)) in MATRIX]
assert any(dw > w and dh > h for (_c, w, h, dw, dh) in _SHAPES), "no up-scale in both axes"
assert any(dw < w and dh < h for (_c, w, h, dw, dh) in _SHAPES), "no down-scale"
assert any((dw == w) != (dh == h) for (_c, w, h, dw, dh) in _SHAPES), "no case with one axis kept and the other resampled"
assert {m for (_cell, (_w, _h, _f, m)) in MATRIX} >= {0.75, 1.5, 2.0, 2.5, 3.0}
assert any(c != "444" and ((dw + 1) // 2) % 2 for (c, _w, _h, dw, _dh) in _SHAPES), "no output width whose chroma rect width is odd"


def matrix_rects(dw, dh, chroma, rng):
    rects = edge_rects(dw, dh, rng, limit=8) + [(0, 0, dw, dh), (dw - 1, dh - 1, 1, 1), (dw // 2, dh // 2, 1, 1), (0, dh - 1, dw, 1), (dw - 1, 0, 1, dh)]
    return [snap(r, chroma) for r in rects]


@pytest.mark.parametrize("layout", list(LAYOUTS))
@pytest.mark.parametrize("chroma", CHROMAS)
@pytest.mark.parametrize("word", WORDS, ids=["%d%s" % (d, "msb" if m else "") for d, m in WORDS])
def test_matrix_vs_oracle(srcnn, oracle_lib, layout, chroma, word):
    cell = (layout, chroma, word)
    depth, msb = word
    case = matrix_case(cell)
    w, h, filt, mul = case
    dw, dh = out_size(w, h, mul)
    rects = matrix_rects(dw, dh, chroma, np.random.default_rng(seed() + CELLS.index(cell)))
    assert len(rects) >= 12, (cell, case, len(rects))
    want = want_for(oracle_lib, chroma, depth, case)
    rig = Rig(srcnn, *frame(w, h, chroma, depth, 100 * w + h), layout, chroma, depth, msb, mul, filt)
    for r in rects:
        assert_rect(rig.values(*r), crop(want, r, chroma),
                    "%s %s %d-bit msb=%d %dx%d %s x%g %s" % (layout, chroma, depth, msb, w, h, FILTER_NAMES[filt], mul, name_of(r)))


# ---- the identity size: chroma is copied; crops of the library's whole-frame call ----
@pytest.mark.parametrize("chroma", ["420", "444"])
def test_identity_size_gives_crops_of_the_whole_frame_call(srcnn, chroma):
    S = srcnn
    rng = np.random.default_rng(seed() + 31)
    for k, (w, h) in enumerate(((23, 17), (64, 40), (9, 7), (1, 5), (130, 66))):
        filt = FILTERS[k % 5]
        layout, (depth, msb) = ("planar", "semiplanar")[k % 2], WORDS[(2 * k + 1) % 9]
        Y, U, V = frame(w, h, chroma, depth, 3 * w + h)
        whole = run(S, LAYOUTS[layout], chroma, depth, msb, Y, U, V, 1.0, filt)
        assert np.array_equal(whole[1], U) and np.array_equal(whole[2], V)        # chroma is copied at the identity size
        rig = Rig(S, Y, U, V, layout, chroma, depth, msb, 1.0, filt)
        rects = edge_rects(w, h, rng, limit=3) + [(0, 0, w, h), (w - 1, h - 1, 1, 1), (w // 2, h // 2, 1, 1)]
        for r in (snap(r, chroma) for r in rects):
            assert_rect(rig.values(*r), crop(whole, r, chroma), "identity %s %s %d-bit %dx%d f%d %s" % (layout, chroma, depth, w, h, filt, name_of(r)))


# ---- repaint in place: the rect inside a full-size frame filled with a canary ----
REPAINT_CASES = [(23, 17, 2, 2.0, "420", 8, 0), (30, 11, 3, 1.5, "422", 8, 0), (9, 7, 1, 2.5, "444", 10, 1), (33, 20, 4, 0.75, "420", 10, 0),
                 (40, 24, 2, 2.0, "420", 10, 1)]
_REPAINT_WANT = {}


def repaint_rects(dw, dh, chroma):
    """Odd and even origins and sizes, one sample, the right and bottom borders, an odd width that stops short of the border."""
    rects = [(1, 1, 1, 1), (3, 2, 3, 2), (2, 1, 4, 3), (5, 0, 5, dh), (1, 3, dw - 1, dh - 3), (0, 0, dw, dh), (dw - 4, dh - 1, 4, 1), (4, 2, 7, 5)]
    rects = [r for r in rects if r[0] + r[2] <= dw and r[1] + r[3] <= dh and r[2] > 0 and r[3] > 0]
    return sorted({snap(r, chroma) for r in rects})


@pytest.mark.parametrize("layout", list(LAYOUTS))
@pytest.mark.parametrize("offset,pad", [(1, 1), (3, 7), (6, 14), (0, 0), (0, 16)])
@pytest.mark.parametrize("w,h,filt,mul,chroma,depth,msb", REPAINT_CASES)
def test_repaint_in_place_vs_oracle(srcnn, oracle_lib, layout, offset, pad, w, h, filt, mul, chroma, depth, msb):
    """The destination is a full-size dw x dh frame of canary bytes; the call gets the addresses of luma sample (x0, y0) and of
    the chroma sample that covers it, and the frame's pitches.  The bytes of the rect's row segments are the oracle's crop;
    every other byte -- the rest of the frame, the row padding, the guards, the source -- is unchanged."""
    S = srcnn
    if depth > 8 and (offset % 2 or pad % 2):
        offset, pad = offset + 1, pad + 1                 # 16-bit planes: even addresses and pitches (still not dword aligned)
    semi = layout == "semiplanar"
    key = (w, h, filt, mul, chroma, depth)
    Y, U, V = frame(w, h, chroma, depth, 7 * w + h)
    if key not in _REPAINT_WANT:
        _REPAINT_WANT[key] = expected(oracle_lib, Y, U, V, chroma, depth, mul, filt)
    want = [to_words(P, depth, msb) for P in _REPAINT_WANT[key]]
    dw, dh = out_size(w, h, mul)
    bps = 1 if depth == 8 else 2
    ins = [to_words(P, depth, msb) for P in (Y, U, V)]
    as_bytes = lambda ps: [np.ascontiguousarray(p).view(np.uint8) for p in ([ps[0], W.interleave(ps[1], ps[2])] if semi else ps)]   # noqa: E731
    src_planes, full_planes = as_bytes(ins), as_bytes(want)
    n = len(src_planes)
    spp = [1] + [2 if semi else 1] * (n - 1)              # samples per column of each plane
    fmt = S.yuv_format(layout, chroma, depth, msb)
    allp = src_planes + full_planes
    rows = [p.shape[0] for p in allp]
    pitches = [p.shape[1] + (pad + 16 * k if pad % 16 == 0 else pad + 4 * k) if pad else p.shape[1] for k, p in enumerate(allp)]
    bases, total = layout_bases(rows, pitches, offset)
    host = np.full(total, CANARY, np.uint8)
    for p, b, pt in zip(src_planes, bases, pitches):
        for r in range(p.shape[0]):
            host[b + r * pt: b + r * pt + p.shape[1]] = p[r]
    for rect in repaint_rects(dw, dh, chroma):
        x0, y0, rw, rh = rect
        cx0, cy0, crw, crh = chroma_rect(rect, chroma)
        org = [(x0, y0, rw, rh)] + [(cx0, cy0, crw, crh)] * (n - 1)         # per plane: first column, first row, columns, rows
        first = [b + oy * pt + ox * bps * s for b, pt, s, (ox, oy, _w, _h) in zip(bases[n:], pitches[n:], spp, org)]
        buf = S.DeviceBuffer.from_numpy(host)
        S.yuv_upscale_rect_dev(fmt, w, h, mul, filt, [(buf, b) for b in bases[:n]] + [None] * (3 - n), pitches[:n] + [0] * (3 - n),
                               x0, y0, rw, rh, [(buf, a) for a in first] + [None] * (3 - n), pitches[n:] + [0] * (3 - n))
        S.sync()
        back = buf.to_numpy(np.uint8, (total,))
        expect = host.copy()
        for p, a, pt, s, (ox, oy, ow, oh) in zip(full_planes, first, pitches[n:], spp, org):
            for r in range(oh):
                expect[a + r * pt: a + r * pt + ow * bps * s] = p[oy + r, ox * bps * s:(ox + ow) * bps * s]
        if not np.array_equal(back, expect):
            bad = np.flatnonzero(back != expect)
            where = ["plane %d" % k for k, b in enumerate(bases) if b <= bad[0] < b + pitches[k] * rows[k]] or ["guard"]
            raise AssertionError("%s: %d bytes differ, first at byte %d (%s): got %d want %d" %
                                 (name_of(rect), len(bad), bad[0], where[0], back[bad[0]], expect[bad[0]]))


# ---- source locality ----
@pytest.mark.parametrize("w,h,mul,filt,layout,chroma,depth,msb", [(70, 40, 2.0, 2, "semiplanar", "420", 8, 0),
                                                                  (40, 31, 1.5, 3, "planar", "422", 12, 1),
                                                                  (50, 30, 0.75, 2, "semiplanar", "420", 10, 1),
                                                                  (50, 30, 0.75, 3, "planar", "444", 16, 0),
                                                                  (3, 40, 1.5, 2, "planar", "420", 8, 0),
                                                                  (3, 40, 1.5, 3, "semiplanar", "422", 10, 0)],
                         ids=["2x-bicubic", "1.5x-lanczos3", "downscale-bicubic", "downscale-lanczos3", "mixed-bicubic", "mixed-lanczos3"])
def test_nothing_outside_the_source_rectangles_is_used(srcnn, oracle_lib, w, h, mul, filt, layout, chroma, depth, msb):
    """Two source frames that agree inside the per-plane rectangles srcnn_yuv_rect_source reports and differ everywhere else
    give the same bytes: the crop.  (3 x 40 x 1.5 -> 4 x 60: chroma keeps its 2 columns while its rows are resampled.)"""
    S = srcnn
    dw, dh = out_size(w, h, mul)
    (cw, ch), (dcw, dch) = chroma_size(w, h, chroma), chroma_size(dw, dh, chroma)
    if w == 3:
        assert cw == dcw and ch != dch
    rng = np.random.default_rng(seed() + 77)
    planes = frame(w, h, chroma, depth, 9 * w + h)
    want = expected(oracle_lib, *planes, chroma, depth, mul, filt)
    fmt = S.yuv_format(layout, chroma, depth, msb)
    rects = edge_rects(dw, dh, rng, limit=5) + [(dw // 2, dh // 2, 1, 1), (0, 0, min(9, dw), 9), (max(0, dw - 9), dh - 9, min(9, dw), 9)]
    assert len(rects) >= 9
    shrunk = 0
    for r in (snap(r, chroma) for r in rects):
        others = []
        for k, P in enumerate(planes):
            sx0, sy0, sw, sh = S.yuv_rect_source(fmt, w, h, mul, filt, *r, 1 if (k and layout == "semiplanar") else k)
            assert sx0 + sw <= P.shape[1] and sy0 + sh <= P.shape[0] and sw and sh
            other = rng.integers(0, 1 << depth, P.shape).astype(P.dtype)           # (integers cannot carry NaN: fresh noise instead)
            other[sy0:sy0 + sh, sx0:sx0 + sw] = P[sy0:sy0 + sh, sx0:sx0 + sw]
            shrunk += int(sw * sh < P.size)
            others.append(other)
        if layout == "semiplanar":
            assert S.yuv_rect_source(fmt, w, h, mul, filt, *r, 2) == (0, 0, 0, 0)
        a = Rig(S, *planes, layout, chroma, depth, msb, mul, filt).values(*r)
        b = Rig(S, *others, layout, chroma, depth, msb, mul, filt).values(*r)
        assert_rect(b, a, "source replaced outside its rectangles, %s" % name_of(r))
        assert_rect(a, crop(want, r, chroma), name_of(r))
    assert shrunk >= 9          # the test has teeth: most source rectangles are smaller than their planes


# ---- both routes: k_yuv_window_chroma and the plane route over the window give the same bytes ----
def child(mode, arg, env=None, timeout=600):
    r = subprocess.run([sys.executable, WORKER, mode, str(arg)], env=dict(os.environ, **(env or {})), capture_output=True, text=True, timeout=timeout)
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")]
    assert r.returncode == 0 and line, "yuv_rect_worker %s: exit %d\n%s\n%s" % (mode, r.returncode, r.stdout[-600:], r.stderr[-1500:])
    return json.loads(line[0][7:])


def test_forced_plane_route_gives_the_same_bytes(srcnn):
    """SRCNN_YUV_RECT_UNFUSED=1 (read when the library loads) sends chroma up-scales down the plane route as well.  The default
    route's bytes of the same rects are held to the oracle by test_edges_vs_oracle_and_whole_frame, whose digests are reused
    when it ran in this session."""
    S = srcnn
    assert "SRCNN_YUV_RECT_UNFUSED=0" in S.debug_settings()
    fast = {"/".join(str(v) for v in cell): _EDGE_DIGEST.get(cell) or W.edge_digest(S, seed(), cell) for cell in EDGE_CELLS}
    assert child("unfused", seed(), env={"SRCNN_YUV_RECT_UNFUSED": "1"}) == fast


# ---- banding ----
@pytest.mark.parametrize("cell", EDGE_CELLS, ids=["i420", "p210-422", "planar444-16"])
def test_banded_rect_gives_the_same_bytes(srcnn, oracle_lib, cell):
    S = srcnn
    L = S.lib()
    layout, chroma, depth, msb = cell
    w, h, mul, filt = W.EDGE_SHAPE
    want = expected(oracle_lib, *frame(w, h, chroma, depth, 7040 + depth), chroma, depth, mul, filt)
    rig = W.edge_rig(S, cell)
    limit = 1 << 20
    # the window of these rects is all 140 columns: 32 planes x 4 B x 140 x (80 + 4) rows do not fit 1 MB, 54-row bands do
    assert 32 * 4 * 140 * (80 + 4) > limit
    band_rows = limit // (32 * 4 * 140) - 4
    bands = -(-80 // band_rows)
    assert bands >= 2
    rects = [(0, 0, 140, 80), (2, 0, 135, 80), (0, 0, 139, 80)]
    unbanded = [rig.values(*r) for r in rects]
    prev = L.srcnn_set_workspace_limit(limit)
    S.profile_enable(True)
    try:
        for r, ref in zip(rects, unbanded):
            S.profile_reset()
            got = rig.values(*r)
            launches = S.profile_read()["conv12"][1]
            assert launches == bands, (r, launches, bands)
            assert_rect(got, ref, "banded vs unbanded %s" % name_of(r))
            assert_rect(got, crop(want, r, chroma), "banded %s vs oracle" % name_of(r))
    finally:
        S.profile_enable(False)
        L.srcnn_set_workspace_limit(prev)


# ---- non-parity modes: Y' is the integer conversion of the mode's own y_path_rect, chroma is the strict bytes ----
@pytest.mark.parametrize("mode_name", ["MODE_FAST", "MODE_FAST_F16", "MODE_RELAXED"])
def test_non_parity_modes_are_exact_around_their_y(srcnn, oracle_lib, mode_name):
    S = srcnn
    rng = np.random.default_rng(seed() + 5)
    prev = S.set_mode(getattr(S, mode_name))        # (a strict-only build refuses: conftest turns that into a skip)
    try:
        for (w, h, mul, filt, layout, chroma, depth, msb) in ((70, 40, 2.0, 2, "semiplanar", "420", 8, 0), (40, 31, 1.5, 3, "planar", "422", 12, 1),
                                                              (50, 30, 0.75, 1, "semiplanar", "444", 10, 0)):
            dw, dh = out_size(w, h, mul)
            Y, U, V = frame(w, h, chroma, depth, 13 * w + h)
            strict = expected(oracle_lib, Y, U, V, chroma, depth, mul, filt)
            s = depth - 8
            yf = Y.astype(np.float32) * np.float32(2.0 ** -s)
            rig = Rig(S, Y, U, V, layout, chroma, depth, msb, mul, filt)
            for r in (snap(r, chroma) for r in edge_rects(dw, dh, rng, limit=4) + [(0, 0, dw, dh), (dw // 2, dh // 2, 1, 1)]):
                yp = (S.y_path_rect(yf, dw, dh, filt, *r) * np.float32(2.0 ** s)).astype(np.uint32).astype(Y.dtype)
                _, cu, cv = crop(strict, r, chroma)
                assert_rect(rig.values(*r), (yp, cu, cv), "%s %dx%d x%g %s %s" % (mode_name, w, h, mul, layout, name_of(r)))
    finally:
        S.set_mode(prev)


# ---- the numpy convenience of the binding ----
@pytest.mark.parametrize("layout,chroma,depth,msb", [("planar", "420", 8, 0), ("semiplanar", "420", 10, 1), ("semiplanar", "444", 12, 0)])
def test_numpy_convenience_returns_the_rects_planes(srcnn, layout, chroma, depth, msb):
    S = srcnn
    w, h, mul, filt = 37, 21, 2.5, 3
    Y, U, V = frame(w, h, chroma, depth, 77)
    whole = [to_words(P, depth, msb) for P in run(S, LAYOUTS[layout], chroma, depth, msb, Y, U, V, mul, filt)]
    ins = [to_words(P, depth, msb) for P in (Y, U, V)]
    planes = [ins[0], W.interleave(ins[1], ins[2])] if layout == "semiplanar" else ins
    for rect in ((0, 0, 92, 52), (6, 4, 41, 23), (90, 50, 2, 2)):
        got = S.yuv_upscale_rect(planes, rect, layout=layout, chroma=chroma, depth=depth, msb_aligned=msb, multiply=mul, filt=filt)
        y, u, v = crop(whole, rect, chroma)
        want = [y, W.interleave(u, v)] if layout == "semiplanar" else [y, u, v]
        assert len(got) == len(want)
        for g, e in zip(got, want):
            assert g.dtype == e.dtype and g.shape == e.shape and np.array_equal(g, e), (layout, chroma, depth, rect)
    with pytest.raises(S.SrcnnError):
        S.yuv_upscale_rect(planes, (0, 0, 0, 5), layout=layout, chroma=chroma, depth=depth, msb_aligned=msb, multiply=mul, filt=filt)


# ---- two host threads on two streams, different rects of different formats ----
def test_two_threads_two_streams(srcnn):
    S = srcnn
    cases = [(("semiplanar", "planar")[k % 2], CHROMAS[k % 3], WORDS[(2 * k + 1) % 9], 2.0 if k % 3 else 1.5, FILTERS[k % 5]) for k in range(8)]
    rigs = [Rig(S, *frame(97, 61, c[1], c[2][0], 500 + k), c[0], c[1], c[2][0], c[2][1], c[3], c[4]) for k, c in enumerate(cases)]
    rects = [snap((3 + 5 * k, 2 + 3 * k, 50 + 7 * k, 31 + 4 * k), cases[k][1]) for k in range(8)]          # inside the smallest output, 145 x 91
    whole = [run(S, LAYOUTS[c[0]], c[1], c[2][0], c[2][1], *frame(97, 61, c[1], c[2][0], 500 + k), c[3], c[4]) for k, c in enumerate(cases)]
    results, errors = [None] * 8, []

    def worker(t):
        st = S.Stream()
        try:
            for k in range(t, 8, 2):
                results[k] = rigs[k].values(*rects[k], stream=st)
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
        assert_rect(results[k], crop(whole[k], rects[k], cases[k][1]), "frame %d on thread %d, %s" % (k, k % 2, name_of(rects[k])))


# ---- one real size ----
def test_1080p_p010_to_4k_interior_and_corner(srcnn):
    """1920 x 1080 P010 -> 3840 x 2160: an interior 256 x 128 rect, an interior 255 x 127 rect (its last chroma column and row cover
    a luma column and row outside it) and the bottom-right 255 x 127 samples -- whose origin (3585, 2033) 4:2:0 does not allow,
    so, by the rule of this file, it is snapped down to (3584, 2032) and the far edge kept."""
    S = srcnn
    w, h = 1920, 1080
    Y, U, V = frame(w, h, "420", 10, 4242)
    whole = run(S, LAYOUTS["semiplanar"], "420", 10, 1, Y, U, V, 2.0, 2)      # (held to the oracle by tests/test_gpu_yuv_ex.py)
    rig = Rig(S, Y, U, V, "semiplanar", "420", 10, 1, 2.0, 2)
    with pytest.raises(S.SrcnnError):
        rig.values(3840 - 255, 2160 - 127, 255, 127)
    for r in ((1600, 902, 256, 128), (1602, 904, 255, 127), snap((3840 - 255, 2160 - 127, 255, 127), "420")):
        assert_rect(rig.values(*r), crop(whole, r, "420"), "%s of 3840x2160" % name_of(r))
