"""srcnn_yuv_upscale_dev (include/srcnn_amd_yuv_ex.h) byte for byte against the oracle composition (GPU).

With s = depth - 8 and maxv = 2^depth - 1:  Y' = (unsigned)(oracle.y_path((float)Y * 2^-s, dw, dh, filter) * 2^s);
U', V' = oracle.resample((float)U, dcw, dch, chroma filter) on the native scale, clipped to [0, maxv] and truncated -- box for
nearest, bilinear for every other filter.  A chroma plane whose size does not change is copied.  16-bit words carry the value in
their low bits, or shifted left by 16 - depth when msb_aligned.  Content is noise beside saturated blocks of 0 and maxv, so the
chroma conversion clips at both ends.
"""
import os
import subprocess
import threading

import numpy as np
import pytest

from test_gpu_yuv import FILTER_NAMES, FILTERS, MULS, SIZES, first_difference, out_size

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PLANAR, SEMI = 0, 1
LAYOUTS = {"planar": PLANAR, "semiplanar": SEMI}
CHROMAS = ("420", "422", "444")
# (depth, msb_aligned): both alignments above 8 bits
WORDS = [(8, 0), (10, 0), (10, 1), (12, 0), (12, 1), (14, 0), (14, 1), (16, 0), (16, 1)]
CANARY = 0xA5
# the 8-bit suite's sizes never give an output width of 7 mod 8 with its multipliers; 21 does (15, 31, 63)
SIZES_EX = SIZES + [(21, 5)]


def chroma_size(w, h, chroma):
    return (w if chroma == "444" else (w + 1) // 2), ((h + 1) // 2 if chroma == "420" else h)


def dtype_of(depth):
    return np.uint8 if depth == 8 else np.uint16


def plane(h, w, seed, depth):
    """Noise with saturated blocks of 0 and maxv."""
    maxv = (1 << depth) - 1
    rng = np.random.default_rng(seed)
    p = rng.integers(0, maxv + 1, (h, w)).astype(dtype_of(depth))
    yy, xx = np.mgrid[0:h, 0:w]
    block = ((yy // 3 + xx // 2) % 3 == 0)
    p[block] = np.where(((yy // 3 + xx // 5) % 2 == 0)[block], 0, maxv).astype(p.dtype)
    return p


def frame(w, h, chroma, depth, seed):
    cw, ch = chroma_size(w, h, chroma)
    return plane(h, w, seed, depth), plane(ch, cw, seed + 1, depth), plane(ch, cw, seed + 2, depth)


def expected(oracle_lib, Y, U, V, chroma, depth, mul, filt):
    h, w = Y.shape
    dw, dh = out_size(w, h, mul)
    (cw, ch), (dcw, dch) = chroma_size(w, h, chroma), chroma_size(dw, dh, chroma)
    s, maxv, dt = depth - 8, (1 << depth) - 1, dtype_of(depth)
    down, up = np.float32(2.0 ** -s), np.float32(2.0 ** s)
    yp = (oracle_lib.y_path(Y.astype(np.float32) * down, dw, dh, filt) * up).astype(np.uint32).astype(dt)

    def conv(P):
        r = P.astype(np.float32) if (dcw, dch) == (cw, ch) else oracle_lib.resample(P.astype(np.float32), dcw, dch, 0 if filt == 0 else 1)
        return np.maximum(np.minimum(r, np.float32(maxv)), np.float32(0)).astype(np.uint32).astype(dt)
    return yp, conv(U), conv(V)


def to_words(P, depth, msb):
    return P << (16 - depth) if msb else P


def run(S, layout, chroma, depth, msb, Y, U, V, mul, filt, stream=None, raw=False):
    """The library's result as values (Y', U', V'), whatever the layout and alignment; the bits beside the value must be zero."""
    ins = [to_words(P, depth, msb) for P in (Y, U, V)] if not raw else [Y, U, V]
    if layout == SEMI:
        uv = np.stack([ins[1], ins[2]], axis=-1).reshape(U.shape[0], 2 * U.shape[1])
        yp, uvp = S.yuv_upscale([ins[0], uv], layout="semiplanar", chroma=chroma, depth=depth, msb_aligned=msb, multiply=mul,
                                filt=filt, stream=stream)
        outs = [yp, np.ascontiguousarray(uvp[:, 0::2]), np.ascontiguousarray(uvp[:, 1::2])]
    else:
        outs = list(S.yuv_upscale(ins, layout="planar", chroma=chroma, depth=depth, msb_aligned=msb, multiply=mul, filt=filt,
                                  stream=stream))
    if depth > 8:
        shift = 16 - depth
        for name, o in zip("YUV", outs):
            assert o.dtype == np.uint16
            if msb:
                assert not np.any(o & ((1 << shift) - 1)), "%s': low bits set in MSB-aligned output" % name
            else:
                assert not np.any(o >> depth), "%s': high bits set in LSB-aligned output" % name
        if msb:
            outs = [o >> shift for o in outs]
    return tuple(outs)


def assert_planes(got, want, what):
    for name, g, e in zip("YUV", got, want):
        assert g.shape == e.shape, (what, name, g.shape, e.shape)
        assert np.array_equal(g, e), "%s %s': %s" % (what, name, first_difference(g, e))


def cases_for(layout, chroma, word):
    """Filter and multiplier rotate across the format axes: every size with two multipliers and one filter per format cell."""
    base = 3 * LAYOUTS[layout] + CHROMAS.index(chroma) + 2 * WORDS.index(word)
    for k, (w, h) in enumerate(SIZES_EX):
        for j in (0, 2):
            filt, mul = FILTERS[(base + k) % 5], MULS[(base + 2 * k + j) % 5]
            dw, dh = out_size(w, h, mul)
            if dw and dh and (dw, dh) != (w, h):
                yield w, h, filt, mul


ALL = [(l, c, wd, case) for l in LAYOUTS for c in CHROMAS for wd in WORDS for case in cases_for(l, c, wd)]
assert {c[3][2] for c in ALL} == set(FILTERS) and {c[3][3] for c in ALL} == set(MULS) and {c[3][:2] for c in ALL} == set(SIZES_EX)
assert {out_size(w, h, m)[0] % 8 for (_l, _c, wd, (w, h, _f, m)) in ALL if wd[0] > 8} == set(range(8))
for _wd in WORDS:   # ... and within every word format as well
    assert {out_size(w, h, m)[0] % 8 for (_l, _c, wd, (w, h, _f, m)) in ALL if wd == _wd} == set(range(8)), _wd
_WANT = {}


def want_for(oracle_lib, chroma, depth, case):
    key = (chroma, depth, case)
    if key not in _WANT:
        w, h, filt, mul = case
        _WANT[key] = expected(oracle_lib, *frame(w, h, chroma, depth, 100 * w + h), chroma, depth, mul, filt)
    return _WANT[key]


@pytest.mark.parametrize("layout", list(LAYOUTS))
@pytest.mark.parametrize("chroma", CHROMAS)
@pytest.mark.parametrize("word", WORDS, ids=["%d%s" % (d, "msb" if m else "") for d, m in WORDS])
def test_matrix_vs_oracle(srcnn, oracle_lib, layout, chroma, word):
    depth, msb = word
    for case in cases_for(layout, chroma, word):
        w, h, filt, mul = case
        Y, U, V = frame(w, h, chroma, depth, 100 * w + h)
        assert_planes(run(srcnn, LAYOUTS[layout], chroma, depth, msb, Y, U, V, mul, filt), want_for(oracle_lib, chroma, depth, case),
                      "%s %s %d-bit msb=%d %dx%d %s x%g" % (layout, chroma, depth, msb, w, h, FILTER_NAMES[filt], mul))


@pytest.mark.parametrize("layout", list(LAYOUTS))
def test_depth8_420_equals_the_yuv420_call(srcnn, layout):
    S = srcnn
    for (w, h, filt, mul) in ((9, 7, 2, 2.0), (23, 17, 0, 1.5), (30, 11, 3, 2.5), (32, 12, 1, 0.75)):
        Y, U, V = frame(w, h, "420", 8, 31 * w + h)
        got = run(S, LAYOUTS[layout], "420", 8, 0, Y, U, V, mul, filt)
        if layout == "semiplanar":
            uv = np.stack([U, V], -1).reshape(U.shape[0], 2 * U.shape[1])
            yp, uvp = S.yuv420_upscale(Y, uv, multiply=mul, filt=filt, fmt="nv12")
            old = (yp, np.ascontiguousarray(uvp[:, 0::2]), np.ascontiguousarray(uvp[:, 1::2]))
        else:
            old = S.yuv420_upscale(Y, U, V, multiply=mul, filt=filt, fmt="i420")
        assert_planes(got, old, "%s %dx%d x%g" % (layout, w, h, mul))


@pytest.mark.parametrize("layout", list(LAYOUTS))
@pytest.mark.parametrize("depth", [10, 12, 14])
def test_stray_bits_are_ignored(srcnn, layout, depth):
    """LSB-aligned input with random bits above `depth`, MSB-aligned input with random bits below it: the clean frame's output."""
    S = srcnn
    w, h, mul, filt = 37, 21, 2.0, 2
    Y, U, V = frame(w, h, "420", depth, 77)
    rng = np.random.default_rng(depth)
    shift = 16 - depth
    for msb in (0, 1):
        clean = run(S, LAYOUTS[layout], "420", depth, msb, Y, U, V, mul, filt)
        dirty = []
        for P in (Y, U, V):
            junk = rng.integers(0, 1 << shift, P.shape).astype(np.uint16)
            dirty.append((P << shift) | junk if msb else P | (junk << depth))
        assert any(np.any(d != to_words(P, depth, msb)) for d, P in zip(dirty, (Y, U, V)))
        assert_planes(run(S, LAYOUTS[layout], "420", depth, msb, *dirty, mul, filt, raw=True), clean, "stray bits, msb=%d" % msb)


@pytest.mark.parametrize("depth", [10, 12, 16])
def test_cross_depth_luma(srcnn, depth):
    """A frame whose luma samples are all multiples of 2^s has Y' >> s equal to the 8-bit call's Y' on Y >> s (the definition:
    the float plane that enters the Y path is the same).  The same holds for chroma because the resampler is exactly
    scale-invariant under powers of two (checked on the CPU oracle: oracle.resample(4 x) == 4 oracle.resample(x) bit for bit,
    box and bilinear, up and down), and floor(min(maxv, 2^s x)) >> s == floor(min(255, x))."""
    S = srcnn
    s = depth - 8
    for (w, h, filt, mul, chroma) in ((23, 17, 2, 2.0, "420"), (30, 11, 0, 1.5, "422"), (9, 7, 4, 2.5, "444"), (33, 20, 1, 0.75, "420")):
        Y8, U8, V8 = frame(w, h, chroma, 8, 5 * w + h)
        hi = [P.astype(np.uint16) << s for P in (Y8, U8, V8)]
        got = run(S, PLANAR, chroma, depth, 0, *hi, mul, filt)
        low = run(S, PLANAR, chroma, 8, 0, Y8, U8, V8, mul, filt)
        assert_planes([g >> s for g in got], [p.astype(np.uint16) for p in low], "%d-bit vs 8-bit %s %dx%d" % (depth, chroma, w, h))


# ---- pitched and misaligned layouts: all planes in one device buffer filled with a canary ----
GUARD = 256


def layout_bases(rows, pitches, offset):
    pos, bases = 0, []
    for r, p in zip(rows, pitches):
        pos += GUARD
        pos = (pos + 63) // 64 * 64 + offset
        bases.append(pos)
        pos += p * r
    return bases, pos + GUARD


@pytest.mark.parametrize("layout", list(LAYOUTS))
# even offsets past a 64-byte boundary with pads that break 16-byte alignment, and the fully aligned case (offset 0, pads that
# are multiples of 16 on widths that are multiples of 8): both forms of the conversion kernels
@pytest.mark.parametrize("offset,pad", [(2, 2), (6, 14), (14, 34), (2, 64), (0, 0), (0, 16)])
@pytest.mark.parametrize("w,h,filt,mul,chroma,depth,msb", [(9, 7, 2, 2.0, "420", 10, 1), (23, 17, 3, 1.5, "422", 12, 0),
                                                           (30, 11, 0, 2.5, "444", 16, 0), (33, 20, 4, 0.75, "420", 14, 1),
                                                           (32, 16, 2, 2.0, "420", 10, 1), (32, 16, 1, 2.0, "444", 12, 0),
                                                           # output luma rows of 12 samples: float4 accesses on the float side
                                                           # while the last 8-sample chunk of every row is partial
                                                           (6, 5, 2, 2.0, "420", 10, 1)])
def test_pitched_and_misaligned_vs_oracle(srcnn, oracle_lib, layout, offset, pad, w, h, filt, mul, chroma, depth, msb):
    S = srcnn
    semi = layout == "semiplanar"
    Y, U, V = frame(w, h, chroma, depth, 7 * w + h)
    want = [to_words(P, depth, msb) for P in expected(oracle_lib, Y, U, V, chroma, depth, mul, filt)]
    ins = [to_words(P, depth, msb) for P in (Y, U, V)]
    il = lambda a, b: np.stack([a, b], -1).reshape(a.shape[0], 2 * a.shape[1])   # noqa: E731
    src_planes = [ins[0], il(ins[1], ins[2])] if semi else ins
    outs = [want[0], il(want[1], want[2])] if semi else want
    n = len(src_planes)
    allp = [np.ascontiguousarray(p).view(np.uint8) for p in src_planes + outs]       # rows of bytes
    rows = [p.shape[0] for p in allp]
    pitches = [p.shape[1] + (pad + 16 * k if pad % 16 == 0 else pad + 4 * k) if pad else p.shape[1] for k, p in enumerate(allp)]
    bases, total = layout_bases(rows, pitches, offset)
    host = np.full(total, CANARY, np.uint8)
    for p, b, pt in zip(allp[:n], bases, pitches):
        for r in range(p.shape[0]):
            host[b + r * pt: b + r * pt + p.shape[1]] = p[r]
    buf = S.DeviceBuffer.from_numpy(host)
    src = [(buf, b) for b in bases[:n]] + [None] * (3 - n)
    dst = [(buf, b) for b in bases[n:]] + [None] * (3 - n)
    S.yuv_upscale_dev(S.yuv_format(layout, chroma, depth, msb), w, h, mul, filt, src, pitches[:n] + [0] * (3 - n), dst,
                      pitches[n:] + [0] * (3 - n))
    S.sync()
    back = buf.to_numpy(np.uint8, (total,))
    expect = host.copy()
    for p, b, pt in zip(allp[n:], bases[n:], pitches[n:]):
        for r in range(p.shape[0]):
            expect[b + r * pt: b + r * pt + p.shape[1]] = p[r]
    if not np.array_equal(back, expect):
        bad = np.flatnonzero(back != expect)
        where = ["plane %d" % k for k, b in enumerate(bases) if b <= bad[0] < b + pitches[k] * rows[k]] or ["guard"]
        raise AssertionError("%d bytes differ, first at byte %d (%s): got %d want %d" % (len(bad), bad[0], where[0], back[bad[0]], expect[bad[0]]))


# ---- frames of the sizes the library is for ----
def test_1080p_p010_to_4k_and_banded(srcnn, oracle_lib):
    S = srcnn
    w, h = 1920, 1080
    Y, U, V = frame(w, h, "420", 10, 4242)
    want = expected(oracle_lib, Y, U, V, "420", 10, 2.0, 2)
    got = run(S, SEMI, "420", 10, 1, Y, U, V, 2.0, 2)
    assert_planes(got, want, "1920x1080 P010 x2")
    limit = 64 << 20
    band = max(16, limit // (32 * 3840 * 4) - 4)
    assert -(-2160 // band) >= 4
    prev = S.lib().srcnn_set_workspace_limit(limit)
    try:
        banded = run(S, SEMI, "420", 10, 1, Y, U, V, 2.0, 2)
    finally:
        S.lib().srcnn_set_workspace_limit(prev)
    assert_planes(banded, got, "1920x1080 P010 x2 in %d-row bands" % band)


@pytest.mark.parametrize("w,h,chroma,depth", [(3840, 2160, "420", 10), (1920, 1080, "444", 12)])
def test_large_planar_vs_library_float_path(srcnn, w, h, chroma, depth):
    """The CPU oracle takes too long on these: the library's float Y path and float resampler (both pinned to the oracle
    elsewhere) with the conversion restated in numpy."""
    S = srcnn
    Y, U, V = frame(w, h, chroma, depth, 8080)
    got = run(S, PLANAR, chroma, depth, 0, Y, U, V, 2.0, 2)
    dw, dh = 2 * w, 2 * h
    dcw, dch = chroma_size(dw, dh, chroma)
    s, maxv = depth - 8, (1 << depth) - 1
    din = S.DeviceBuffer.from_numpy(Y.astype(np.float32) * np.float32(2.0 ** -s))
    dout = S.DeviceBuffer(dw * dh * 4)
    S.check(S.lib().srcnn_y_path_f32_dev(din.ptr, w, h, dw, dh, 2, dout.ptr, None))
    S.sync()
    want_y = (dout.to_numpy(np.float32, (dh, dw)) * np.float32(2.0 ** s)).astype(np.uint32).astype(np.uint16)
    del din, dout
    want_c = [np.clip(S.resample(P.astype(np.float32), dcw, dch, 1), 0, maxv).astype(np.uint32).astype(np.uint16) for P in (U, V)]
    assert_planes(got, [want_y] + want_c, "%dx%d %s %d-bit x2" % (w, h, chroma, depth))


# ---- two host threads on two streams, mixed formats ----
def test_two_threads_two_streams(srcnn):
    S = srcnn
    cases = [(SEMI if k % 2 else PLANAR, CHROMAS[k % 3], WORDS[(2 * k + 1) % 9], 2.0 if k % 3 else 1.5, FILTERS[k % 5]) for k in range(8)]
    frames = [frame(97, 61, c[1], c[2][0], 500 + k) for k, c in enumerate(cases)]
    call = lambda k, st=None: run(S, cases[k][0], cases[k][1], cases[k][2][0], cases[k][2][1], *frames[k], cases[k][3], cases[k][4], stream=st)   # noqa: E731
    single = [call(k) for k in range(8)]
    results, errors = [None] * 8, []

    def worker(t):
        st = S.Stream()
        try:
            for k in range(t, 8, 2):
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
    for k in range(8):
        assert_planes(results[k], single[k], "frame %d on thread %d" % (k, k % 2))


# ---- tools/srcnnyuv --all-formats ----
@pytest.mark.parametrize("tag,chroma,depth", [("C420p10", "420", 10), ("C422", "422", 8), ("C444p12", "444", 12)])
def test_srcnnyuv_all_formats_vs_oracle(srcnn, oracle_lib, tmp_path, tag, chroma, depth):
    w, h, mul, filt = 37, 21, 2.5, 3
    dw, dh = out_size(w, h, mul)
    tags_in = "YUV4MPEG2 W%d H%d F30000:1001 Ip A1:1 %s XYSCSS=FOO" % (w, h, tag)
    params = ["", " Ixyz", " XFOO=1"]
    frames = [frame(w, h, chroma, depth, 900 + k) for k in range(3)]
    data = tags_in.encode() + b"\n"
    for p, planes in zip(params, frames):
        data += b"FRAME" + p.encode() + b"\n" + b"".join(P.astype("<u2" if depth > 8 else np.uint8).tobytes() for P in planes)
    (tmp_path / "in.y4m").write_bytes(data)
    exe = os.path.join(ROOT, "libsrcnn_amd", "bin", "srcnnyuv")
    r = subprocess.run([exe, "--all-formats", "--scale", "2.5", "--filter", "lanczos3", str(tmp_path / "in.y4m"), "-"],
                       capture_output=True, timeout=300)
    assert r.returncode == 0, r.stderr[-800:]
    header, rest = r.stdout.split(b"\n", 1)
    assert header.decode() == tags_in.replace("W%d H%d" % (w, h), "W%d H%d" % (dw, dh))
    dcw, dch = chroma_size(dw, dh, chroma)
    dt = "<u2" if depth > 8 else np.uint8
    bps = 2 if depth > 8 else 1
    for p, (Y, U, V) in zip(params, frames):
        line, rest = rest.split(b"\n", 1)
        assert line.decode() == "FRAME" + p
        ny, nc = dw * dh * bps, dcw * dch * bps
        body, rest = rest[:ny + 2 * nc], rest[ny + 2 * nc:]
        got = (np.frombuffer(body[:ny], dt).reshape(dh, dw), np.frombuffer(body[ny:ny + nc], dt).reshape(dch, dcw),
               np.frombuffer(body[ny + nc:], dt).reshape(dch, dcw))
        assert_planes(got, expected(oracle_lib, Y, U, V, chroma, depth, mul, filt), "srcnnyuv %s frame%s" % (tag, p))
    assert rest == b""
