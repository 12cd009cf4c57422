"""srcnn_yuv_packed_upscale_dev (include/srcnn_amd_yuv_packed.h) byte for byte against the oracle composition and against the
library's own planar call (GPU), with a numpy restatement of the ten packed layouts that is itself checked on the CPU.

The Y, U and V samples of a packed result are those of srcnn_yuv_upscale_dev for the planar frame of the same chroma format and
depth (tests/test_gpu_yuv_ex.py states that composition: plane() and expected() come from there); alpha goes through the chroma
filter on its own scale.  All bytes of the tight output rows are compared, so the slots that carry no sample -- the second Y of
the last pair at odd width, v210's fields past the row, bits 30-31 of v210 words, the low bits of Y21x words -- must be zero.
"""
import threading

import numpy as np
import pytest

from test_gpu_yuv import FILTER_NAMES, FILTERS, MULS, first_difference, out_size
from test_gpu_yuv_ex import SIZES_EX, expected, plane

gpu = pytest.mark.gpu

CANARY = 0xA5
# name -> (SRCNN_YUVP_* value, chroma, depth of Y / U / V, depth of alpha or 0, alignment of base and pitch)
FORMATS = {
    "yuy2": (0, "422", 8, 0, 1), "uyvy": (1, "422", 8, 0, 1), "yvyu": (2, "422", 8, 0, 1),
    "y210": (3, "422", 10, 0, 2), "y212": (4, "422", 12, 0, 2), "y216": (5, "422", 16, 0, 2),
    "vuya": (6, "444", 8, 8, 1), "y410": (7, "444", 10, 2, 4), "y416": (8, "444", 16, 16, 2),
    "v210": (9, "422", 10, 0, 4),
}
NAMES = list(FORMATS)
# byte index inside a pixel pair of (Y0, U, Y1, V)
POS422 = {"yuy2": (0, 1, 2, 3), "uyvy": (1, 0, 3, 2), "yvyu": (0, 3, 2, 1)}


# ---- the numpy restatement -------------------------------------------------------------------------------------------------
def ccols(name, w):
    return (w + 1) // 2 if FORMATS[name][1] == "422" else w


def row_bytes(name, w):
    if name in POS422:
        return 4 * ((w + 1) // 2)
    if name in ("y210", "y212", "y216"):
        return 8 * ((w + 1) // 2)
    if name in ("vuya", "y410"):
        return 4 * w
    if name == "y416":
        return 8 * w
    return 128 * ((w + 47) // 48)


def _padded(P, cols, junk, maxv):
    """P widened to `cols` columns: zeros, or random values of the field's range where a generator is given."""
    h, w = P.shape
    out = np.zeros((h, cols), np.uint32)
    if junk is not None:
        out[:] = junk.integers(0, maxv + 1, (h, cols))
    out[:, :w] = P
    return out


def pack(name, Y, U, V, A=None, junk=None):
    """Planes of sample values -> (h, row_bytes) uint8.  junk: a numpy Generator that fills everything the format ignores on
    input (slots without a sample, bits beside the fields) with random bits instead of zeros."""
    _id, chroma, depth, adepth, _al = FORMATS[name]
    h, w = Y.shape
    maxv = (1 << depth) - 1
    assert U.shape == V.shape == (h, ccols(name, w)) and (A is None) == (adepth == 0)
    if chroma == "422" and name != "v210":
        n = (w + 1) // 2
        Yp = _padded(Y, 2 * n, junk, maxv)
        fields = [Yp[:, 0::2], U.astype(np.uint32), Yp[:, 1::2], V.astype(np.uint32)]
        if name in POS422:
            out = np.zeros((h, n, 4), np.uint8)
            for f, pos in zip(fields, POS422[name]):
                out[:, :, pos] = f
            return out.reshape(h, 4 * n)
        shift = 16 - depth
        words = np.stack(fields, -1) << shift
        if junk is not None and shift:
            words |= junk.integers(0, 1 << shift, words.shape).astype(np.uint32)
        return np.ascontiguousarray(words.astype("<u2")).view(np.uint8).reshape(h, 8 * n)
    if name == "vuya":
        return np.stack([V, U, Y, A], -1).astype(np.uint8).reshape(h, 4 * w)
    if name == "y410":
        u32 = lambda P: P.astype(np.uint32)   # noqa: E731
        words = u32(U) | (u32(Y) << 10) | (u32(V) << 20) | (u32(A) << 30)
        return np.ascontiguousarray(words.astype("<u4")).view(np.uint8).reshape(h, 4 * w)
    if name == "y416":
        return np.ascontiguousarray(np.stack([U, Y, V, A], -1).astype("<u2")).view(np.uint8).reshape(h, 8 * w)
    assert name == "v210"
    g = 8 * ((w + 47) // 48)                                     # groups of 6 pixels per row, whole 128-byte blocks
    y = _padded(Y, 6 * g, junk, maxv).reshape(h, g, 6)
    u = _padded(U, 3 * g, junk, maxv).reshape(h, g, 3)
    v = _padded(V, 3 * g, junk, maxv).reshape(h, g, 3)
    words = np.stack([u[..., 0] | (y[..., 0] << 10) | (v[..., 0] << 20), y[..., 1] | (u[..., 1] << 10) | (y[..., 2] << 20),
                      v[..., 1] | (y[..., 3] << 10) | (u[..., 2] << 20), y[..., 4] | (v[..., 2] << 10) | (y[..., 5] << 20)], -1)
    if junk is not None:
        words |= junk.integers(0, 4, words.shape).astype(np.uint32) << 30
    return np.ascontiguousarray(words.astype("<u4")).view(np.uint8).reshape(h, 16 * g)


def unpack(name, frame, w):
    """(h, row_bytes) uint8 -> (Y, U, V, A | None) as sample values, by the read rule: bits beside a field are ignored."""
    _id, chroma, depth, adepth, _al = FORMATS[name]
    frame = np.ascontiguousarray(frame, np.uint8)
    h = frame.shape[0]
    assert frame.shape == (h, row_bytes(name, w)), (frame.shape, row_bytes(name, w))
    cw = ccols(name, w)
    dt = np.uint8 if depth == 8 else np.uint16
    if name in POS422:
        px = frame.reshape(h, -1, 4)
        y0, u, y1, v = (px[:, :, p] for p in POS422[name])
        return np.stack([y0, y1], -1).reshape(h, -1)[:, :w].copy(), u[:, :cw].copy(), v[:, :cw].copy(), None
    if name in ("y210", "y212", "y216"):
        px = (frame.view("<u2").reshape(h, -1, 4) >> (16 - depth)).astype(dt)
        return np.stack([px[..., 0], px[..., 2]], -1).reshape(h, -1)[:, :w].copy(), px[:, :cw, 1].copy(), px[:, :cw, 3].copy(), None
    if name == "vuya":
        px = frame.reshape(h, w, 4)
        return px[..., 2].copy(), px[..., 1].copy(), px[..., 0].copy(), px[..., 3].copy()
    if name == "y410":
        q = frame.view("<u4").reshape(h, w).astype(np.uint32)
        return ((q >> 10) & 1023).astype(dt), (q & 1023).astype(dt), ((q >> 20) & 1023).astype(dt), (q >> 30).astype(dt)
    if name == "y416":
        px = frame.view("<u2").reshape(h, w, 4).astype(dt)
        return px[..., 1].copy(), px[..., 0].copy(), px[..., 2].copy(), px[..., 3].copy()
    q = frame.view("<u4").reshape(h, -1, 4).astype(np.uint32)
    f = lambda k, s: ((q[..., k] >> s) & 1023).astype(dt)   # noqa: E731
    y = np.stack([f(0, 10), f(1, 0), f(1, 20), f(2, 10), f(3, 0), f(3, 20)], -1).reshape(h, -1)
    u = np.stack([f(0, 0), f(1, 10), f(2, 20)], -1).reshape(h, -1)
    v = np.stack([f(0, 20), f(2, 0), f(3, 10)], -1).reshape(h, -1)
    return y[:, :w].copy(), u[:, :cw].copy(), v[:, :cw].copy(), None


def frame_planes(name, w, h, seed):
    """Noise beside saturated blocks (plane() of the planar suite), alpha from the same generator at alpha's own depth."""
    _id, _chroma, depth, adepth, _al = FORMATS[name]
    cw = ccols(name, w)
    A = plane(h, w, seed + 3, adepth) if adepth else None
    return plane(h, w, seed, depth), plane(h, cw, seed + 1, depth), plane(h, cw, seed + 2, depth), A


# ---- the restatement, checked without a device -------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_restatement_round_trips(name):
    rng = np.random.default_rng(5)
    for (w, h) in ((1, 1), (2, 3), (7, 2), (47, 2), (48, 1), (49, 3), (96, 2), (101, 2)):
        Y, U, V, A = frame_planes(name, w, h, 11 * w + h)
        clean = pack(name, Y, U, V, A)
        assert clean.dtype == np.uint8 and clean.shape == (h, row_bytes(name, w))
        for packed in (clean, pack(name, Y, U, V, A, junk=rng)):
            got = unpack(name, packed, w)
            for want, g in zip((Y, U, V, A), got):
                assert (want is None and g is None) or (g.shape == want.shape and np.array_equal(g, want)), (name, w, h)
            assert np.array_equal(pack(name, *got), clean), (name, w, h)        # and back: the padding slots come out as zero


def test_restatement_handwritten_v210_group_and_y410_word():
    # one v210 group: Y = 64 .. 69, Cb = 512, 513, 514, Cr = 940, 941, 942
    Y = np.array([[64, 65, 66, 67, 68, 69]], np.uint16)
    U = np.array([[512, 513, 514]], np.uint16)
    V = np.array([[940, 941, 942]], np.uint16)
    words = [512 | (64 << 10) | (940 << 20), 65 | (513 << 10) | (66 << 20), 941 | (67 << 10) | (514 << 20), 68 | (942 << 10) | (69 << 20)]
    want = b"".join(int(x).to_bytes(4, "little") for x in words) + bytes(112)
    assert want[:4] == bytes([0x00, 0x02, 0xC1, 0x3A])            # 0x3AC10200: Cb0 = 0x200, Y0 = 0x040, Cr0 = 0x3AC
    got = pack("v210", Y, U, V)
    assert got.shape == (1, 128) and got.tobytes() == want
    y, u, v, a = unpack("v210", got, 6)
    assert a is None and np.array_equal(y, Y) and np.array_equal(u, U) and np.array_equal(v, V)
    # one Y410 word: U = 0x155, Y = 0x2AA, V = 0x3FF, A = 2 -> 0x155 | 0x2AA << 10 | 0x3FF << 20 | 2 << 30 = 0xBFFAA955
    one = lambda x: np.array([[x]], np.uint16)   # noqa: E731
    got = pack("y410", one(0x2AA), one(0x155), one(0x3FF), one(2))
    assert got.tobytes() == bytes([0x55, 0xA9, 0xFA, 0xBF])
    y, u, v, a = unpack("y410", got, 1)
    assert (int(y[0, 0]), int(u[0, 0]), int(v[0, 0]), int(a[0, 0])) == (0x2AA, 0x155, 0x3FF, 2)
    # and the byte formats, one pixel pair / pixel each: Y0 = 1, U = 2, Y1 = 3, V = 4 (A = 5)
    two = np.array([[1, 3]], np.uint8)
    assert pack("yuy2", two, one(2), one(4)).tobytes() == bytes([1, 2, 3, 4])
    assert pack("uyvy", two, one(2), one(4)).tobytes() == bytes([2, 1, 4, 3])
    assert pack("yvyu", two, one(2), one(4)).tobytes() == bytes([1, 4, 3, 2])
    assert pack("y210", two, one(2), one(4)).tobytes() == bytes([0x40, 0, 0x80, 0, 0xC0, 0, 0, 1])
    assert pack("vuya", one(1), one(2), one(4), one(5)).tobytes() == bytes([4, 2, 1, 5])
    assert pack("y416", one(1), one(2), one(4), one(5)).tobytes() == bytes([2, 0, 1, 0, 4, 0, 5, 0])


# ---- 1. the matrix against the oracle ------------------------------------------------------------------------------------------
SIZES_PACKED = SIZES_EX + [(47, 3), (49, 2), (16, 4), (6, 2)]


def cases_for(name):
    """Filter and multiplier rotate across the formats: every size with two multipliers and one filter per format."""
    base = FORMATS[name][0]
    for k, (w, h) in enumerate(SIZES_PACKED):
        for j in (0, 2):
            filt, mul = FILTERS[(base + k) % 5], MULS[(base + 2 * k + j) % 5]
            dw, dh = out_size(w, h, mul)
            if dw and dh and (dw, dh) != (w, h):
                yield w, h, filt, mul


ALL = [(name, case) for name in NAMES for case in cases_for(name)]
assert {c[2] for _n, c in ALL} == set(FILTERS) and {c[3] for _n, c in ALL} == set(MULS) and {c[:2] for _n, c in ALL} == set(SIZES_PACKED)
for _name in NAMES:
    _dws = {out_size(w, h, m)[0] for n, (w, h, _f, m) in ALL if n == _name}
    if _name == "v210":
        assert {d % 6 for d in _dws} == set(range(6)), sorted(_dws)
        assert min(_dws) < 48 < max(_dws) and any(48 < d <= 96 for d in _dws) and any(d > 96 for d in _dws), sorted(_dws)
    else:
        assert {d % 8 for d in _dws} == set(range(8)), (_name, sorted(_dws))
    if FORMATS[_name][1] == "422":
        assert {d % 2 for d in _dws} == {0, 1} and {w % 2 for n, (w, _h, _f, _m) in ALL if n == _name} == {0, 1}, _name
_WANT = {}


def alpha_expected(oracle_lib, A, adepth, mul, filt):
    h, w = A.shape
    dw, dh = out_size(w, h, mul)
    r = A.astype(np.float32) if (dw, dh) == (w, h) else oracle_lib.resample(A.astype(np.float32), dw, dh, 0 if filt == 0 else 1)
    return np.maximum(np.minimum(r, np.float32((1 << adepth) - 1)), np.float32(0)).astype(np.uint32).astype(A.dtype)


def want_for(oracle_lib, name, case):
    """The expected planes, computed once per (chroma, depth, alpha depth, case) and shared by the formats that differ only in
    their byte order."""
    _id, chroma, depth, adepth, _al = FORMATS[name]
    key = (chroma, depth, adepth, case)
    if key not in _WANT:
        w, h, filt, mul = case
        Y, U, V, A = frame_planes(name, w, h, 100 * w + h)
        yuv = expected(oracle_lib, Y, U, V, chroma, depth, mul, filt)
        _WANT[key] = tuple(yuv) + ((alpha_expected(oracle_lib, A, adepth, mul, filt),) if adepth else (None,))
    return _WANT[key]


def assert_bytes(got, want, what):
    assert got.dtype == np.uint8 and got.shape == want.shape, (what, got.shape, want.shape)
    assert np.array_equal(got, want), "%s: %s" % (what, first_difference(got, want))


@gpu
@pytest.mark.parametrize("name", NAMES)
def test_matrix_vs_oracle(srcnn, oracle_lib, name):
    """Every input carries random bits wherever the format ignores them; the expectation is built from the clean planes."""
    rng = np.random.default_rng(FORMATS[name][0])
    dirtied = 0
    for case in cases_for(name):
        w, h, filt, mul = case
        dw, _dh = out_size(w, h, mul)
        planes = frame_planes(name, w, h, 100 * w + h)
        src = pack(name, *planes, junk=rng)
        dirtied += int(not np.array_equal(src, pack(name, *planes)))
        got = srcnn.yuv_packed_upscale(src, name, w, multiply=mul, filt=filt)
        assert_bytes(got, pack(name, *want_for(oracle_lib, name, case)),
                     "%s %dx%d -> width %d %s x%g" % (name, w, h, dw, FILTER_NAMES[filt], mul))
    if name in ("y210", "y212", "v210") or FORMATS[name][1] == "422":
        assert dirtied, "no input of %s carried a stray bit" % name


@gpu
@pytest.mark.parametrize("name", ["yuy2", "y210", "y216", "v210"])
def test_stray_bits_do_not_change_the_result(srcnn, name):
    S = srcnn
    w, h, mul, filt = 37, 5, 2.0, 2
    planes = frame_planes(name, w, h, 77)
    clean = pack(name, *planes)
    dirty = pack(name, *planes, junk=np.random.default_rng(9))
    assert (name == "y216" and w % 2 == 0) or not np.array_equal(clean, dirty)
    assert_bytes(S.yuv_packed_upscale(dirty, name, w, multiply=mul, filt=filt), S.yuv_packed_upscale(clean, name, w, multiply=mul, filt=filt), name)


# ---- 2. against the library's own planar call ----------------------------------------------------------------------------------
def through_planar(S, name, src, w, mul, filt):
    """pack(yuv_upscale(unpack(x))): the planar call on the same samples (Y21x words MSB-aligned, as the packed words are), alpha
    through the library's float resampler with the conversion restated."""
    _id, chroma, depth, adepth, _al = FORMATS[name]
    Y, U, V, A = unpack(name, src, w)
    msb = name in ("y210", "y212", "y216") and depth < 16
    shift = 16 - depth if msb else 0
    outs = S.yuv_upscale([P << shift for P in (Y, U, V)] if shift else [Y, U, V], layout="planar", chroma=chroma, depth=depth,
                         msb_aligned=msb, multiply=mul, filt=filt)
    outs = [o >> shift for o in outs] if shift else list(outs)
    Ap = None
    if adepth:
        h = Y.shape[0]
        dw, dh = out_size(w, h, mul)
        r = A.astype(np.float32) if (dw, dh) == (w, h) else S.resample(A.astype(np.float32), dw, dh, 0 if filt == 0 else 1)
        Ap = np.maximum(np.minimum(r, np.float32((1 << adepth) - 1)), np.float32(0)).astype(np.uint32).astype(A.dtype)
    return pack(name, outs[0], outs[1], outs[2], Ap)


PLANAR_CASES = [(23, 17, 2, 1.0), (16, 6, 0, 1.0), (33, 20, 1, 0.75), (50, 7, 4, 0.5), (9, 7, 3, 2.0), (48, 4, 2, 2.5)]


@gpu
@pytest.mark.parametrize("name", NAMES)
def test_equals_the_planar_call(srcnn, name):
    """Identity size (multiply 1.0: Y still goes through SRCNN, chroma and alpha are copied), down-scales and up-scales."""
    for (w, h, filt, mul) in PLANAR_CASES:
        src = pack(name, *frame_planes(name, w, h, 31 * w + h))
        got = srcnn.yuv_packed_upscale(src, name, w, multiply=mul, filt=filt)
        assert_bytes(got, through_planar(srcnn, name, src, w, mul, filt), "%s %dx%d x%g" % (name, w, h, mul))
        if mul == 1.0:                                               # chroma (and alpha) of an identity-size call: the input's
            for a, b in zip(unpack(name, got, w)[1:], unpack(name, src, w)[1:]):
                assert (a is None and b is None) or np.array_equal(a, b), name


@gpu
@pytest.mark.parametrize("mode", ["MODE_STRICT", "MODE_FAST", "MODE_FAST_F16", "MODE_RELAXED"])
def test_equals_the_planar_call_in_every_mode(srcnn, mode):
    """One case per format in each numerics mode (a strict-only build refuses the others: that mode is skipped there)."""
    S = srcnn
    prev = S.set_mode(getattr(S, mode))
    try:
        for k, name in enumerate(NAMES):
            w, h, filt, mul = 40 + k, 12, FILTERS[k % 5], 2.0
            src = pack(name, *frame_planes(name, w, h, 900 + k))
            assert_bytes(S.yuv_packed_upscale(src, name, w, multiply=mul, filt=filt), through_planar(S, name, src, w, mul, filt),
                         "%s in %s" % (name, mode))
    finally:
        S.set_mode(prev)


# ---- 3. pitched and misaligned frames -------------------------------------------------------------------------------------------
GUARD = 256


@gpu
@pytest.mark.parametrize("name", NAMES)
# base = a 64-byte boundary + offset.  (0, 0) and (0, 32): 16-byte vectors with tight and padded rows; the others offset the
# base by one, two and three times the format's alignment with pads that break the 16-byte alignment of the rows as well
@pytest.mark.parametrize("offset,pad", [(1, 1), (2, 5), (3, 12), (0, 0), (0, 32)])
def test_pitched_and_misaligned_equal_the_tight_run(srcnn, name, offset, pad):
    S = srcnn
    align = FORMATS[name][4]
    for (w, h, filt, mul) in ((23, 5, 2, 2.0), (32, 4, 1, 1.5)):
        dw, dh = out_size(w, h, mul)
        src = pack(name, *frame_planes(name, w, h, 7 * w + h))
        tight = S.yuv_packed_upscale(src, name, w, multiply=mul, filt=filt)
        rows = [h, dh]
        rbs = [src.shape[1], tight.shape[1]]
        pitches = [rb + align * (pad + 4 * k) for k, rb in enumerate(rbs)]
        pos, bases = 0, []
        for r, p in zip(rows, pitches):
            pos = (pos + GUARD + 63) // 64 * 64 + align * offset
            bases.append(pos)
            pos += p * r
        total = pos + GUARD
        host = np.full(total, CANARY, np.uint8)
        for r in range(h):
            host[bases[0] + r * pitches[0]: bases[0] + r * pitches[0] + rbs[0]] = src[r]
        buf = S.DeviceBuffer.from_numpy(host)
        S.yuv_packed_upscale_dev(name, w, h, mul, filt, (buf, bases[0]), pitches[0], (buf, bases[1]), pitches[1])
        S.sync()
        back = buf.to_numpy(np.uint8, (total,))
        expect = host.copy()
        for r in range(dh):
            expect[bases[1] + r * pitches[1]: bases[1] + r * pitches[1] + rbs[1]] = tight[r]
        if not np.array_equal(back, expect):
            bad = np.flatnonzero(back != expect)
            where = "output frame" if bases[1] <= bad[0] < bases[1] + pitches[1] * dh else "input frame or guard"
            raise AssertionError("%s %dx%d: %d bytes differ, first at byte %d (%s): got %d want %d" %
                                 (name, w, h, len(bad), bad[0], where, back[bad[0]], expect[bad[0]]))
        if align > 1:                                                # one byte (or two) off the alignment: refused, nothing written
            for kw in (dict(src=(buf, bases[0] + align // 2)), dict(dst=(buf, bases[1] + align // 2)),
                       dict(src_pitch=pitches[0] + align // 2), dict(dst_pitch=pitches[1] + align // 2)):
                a = dict(src=(buf, bases[0]), src_pitch=pitches[0], dst=(buf, bases[1]), dst_pitch=pitches[1])
                a.update(kw)
                with pytest.raises(S.SrcnnError) as e:
                    S.yuv_packed_upscale_dev(name, w, h, mul, filt, a["src"], a["src_pitch"], a["dst"], a["dst_pitch"])
                assert e.value.code == -1, kw


# ---- 4. one real frame --------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("name", ["v210", "yuy2"])
def test_1080p_to_4k_and_banded(srcnn, name):
    """No CPU oracle at this size: the planar call's bytes, and the same bytes again when Y is produced in several bands."""
    S = srcnn
    w, h = 1920, 1080
    src = pack(name, *frame_planes(name, w, h, 4242))
    got = S.yuv_packed_upscale(src, name, w, multiply=2.0, filt=2)
    assert_bytes(got, through_planar(S, name, src, w, 2.0, 2), "1920x1080 %s x2" % name)
    limit = 64 << 20
    band = max(16, limit // (32 * 3840 * 4) - 4)
    assert -(-2160 // band) >= 4
    prev = S.lib().srcnn_set_workspace_limit(limit)
    try:
        banded = S.yuv_packed_upscale(src, name, w, multiply=2.0, filt=2)
    finally:
        S.lib().srcnn_set_workspace_limit(prev)
    assert_bytes(banded, got, "1920x1080 %s x2 in %d-row bands" % (name, band))


# ---- 5. two host threads on two streams, mixed formats --------------------------------------------------------------------------
@gpu
def test_two_threads_two_streams(srcnn):
    S = srcnn
    cases = [(NAMES[k], 2.0 if k % 3 else 1.5, FILTERS[k % 5]) for k in range(10)]
    frames = [pack(c[0], *frame_planes(c[0], 97, 61, 500 + k)) for k, c in enumerate(cases)]
    call = lambda k, st=None: S.yuv_packed_upscale(frames[k], cases[k][0], 97, multiply=cases[k][1], filt=cases[k][2], stream=st)   # noqa: E731
    single = [call(k) for k in range(10)]
    results, errors = [None] * 10, []

    def worker(t):
        st = S.Stream()
        try:
            for k in range(t, 10, 2):
                results[k] = call(k, st)
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
    for k in range(10):
        assert_bytes(results[k], single[k], "%s frame %d on thread %d" % (cases[k][0], k, k % 2))
