"""srcnn_yuv420_upscale_dev (include/srcnn_amd_yuv.h) byte for byte against the oracle composition (GPU).

Y' = oracle.y_path((float)Y, dw, dh, filter) truncated to u8; U', V' = oracle.resample((float)U, dcw, dch, chroma filter)
clipped to [0, 255] and truncated -- box for nearest, bilinear for every other filter (the colour shell's chroma filter).
A chroma plane whose size does not change is copied (the library's identity-size deviation; the oracle half-copies there).
Content is noise beside saturated 0 / 255 blocks, so the chroma conversion clips at both ends.
"""
import hashlib
import json
import os
import subprocess
import sys
import threading

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
I420, NV12 = 0, 1
FORMATS = {"i420": I420, "nv12": NV12}
FILTERS = (0, 1, 2, 3, 4)
FILTER_NAMES = ("nearest", "bilinear", "bicubic", "lanczos3", "bspline")
MULS = (0.75, 1.5, 2.0, 2.5, 3.0)
# odd and even sizes, 1-sample-wide and 1-sample-tall chroma planes; with MULS the output widths take every residue mod 4
SIZES = [(9, 7), (8, 6), (1, 5), (2, 9), (23, 17), (30, 11), (17, 2)]
CANARY = 0xA5


def out_size(w, h, mul):
    m = np.float32(mul)
    return int(np.float32(w) * m), int(np.float32(h) * m)


def chroma_size(w, h):
    return (w + 1) // 2, (h + 1) // 2


def plane(h, w, seed):
    """Noise with saturated blocks of 0 and 255."""
    rng = np.random.default_rng(seed)
    p = rng.integers(0, 256, (h, w), dtype=np.uint8)
    yy, xx = np.mgrid[0:h, 0:w]
    block = ((yy // 3 + xx // 2) % 3 == 0)
    p[block] = np.where(((yy // 3 + xx // 5) % 2 == 0)[block], 0, 255).astype(np.uint8)
    return p


def frame(w, h, seed):
    cw, ch = chroma_size(w, h)
    return plane(h, w, seed), plane(ch, cw, seed + 1), plane(ch, cw, seed + 2)


def chroma_filter(filt):
    return 0 if filt == 0 else 1


def expected(oracle_lib, Y, U, V, mul, filt):
    h, w = Y.shape
    dw, dh = out_size(w, h, mul)
    (cw, ch), (dcw, dch) = chroma_size(w, h), chroma_size(dw, dh)
    yp = oracle_lib.y_path(Y.astype(np.float32), dw, dh, filt).astype(np.uint8)

    def chroma(P):
        r = P.astype(np.float32) if (dcw, dch) == (cw, ch) else oracle_lib.resample(P.astype(np.float32), dcw, dch, chroma_filter(filt))
        return np.clip(r, 0, 255).astype(np.uint8)
    return yp, chroma(U), chroma(V)


def run(S, fmt, Y, U, V, mul, filt, stream=None):
    """The library's result as (Y', U', V'), whatever the format."""
    if fmt == NV12:
        uv = np.stack([U, V], axis=-1).reshape(U.shape[0], 2 * U.shape[1])
        yp, uvp = S.yuv420_upscale(Y, uv, multiply=mul, filt=filt, fmt="nv12", stream=stream)
        return yp, np.ascontiguousarray(uvp[:, 0::2]), np.ascontiguousarray(uvp[:, 1::2])
    return S.yuv420_upscale(Y, U, V, multiply=mul, filt=filt, fmt="i420", stream=stream)


def first_difference(got, want):
    bad = np.argwhere(got != want)
    i = tuple(bad[0])
    return "%d bytes differ, first at %s: got %d want %d" % (len(bad), i, got[i], want[i])


def assert_planes(got, want, what):
    for name, g, e in zip("YUV", got, want):
        assert g.shape == e.shape, (what, name, g.shape, e.shape)
        assert np.array_equal(g, e), "%s %s': %s" % (what, name, first_difference(g, e))


def matrix():
    for (w, h) in SIZES:
        for filt in FILTERS:
            for mul in MULS:
                dw, dh = out_size(w, h, mul)
                if dw and dh and (dw, dh) != (w, h):
                    yield w, h, filt, mul


CASES = list(matrix())
assert {out_size(w, h, m)[0] % 4 for (w, h, _f, m) in CASES} == {0, 1, 2, 3}
_WANT = {}


def want_for(oracle_lib, case):
    if case not in _WANT:
        w, h, filt, mul = case
        Y, U, V = frame(w, h, 100 * w + h)
        _WANT[case] = expected(oracle_lib, Y, U, V, mul, filt)
    return _WANT[case]


def digest(planes):
    return hashlib.sha256(b"".join(p.tobytes() for p in planes)).hexdigest()


@pytest.mark.parametrize("fmt", ["i420", "nv12"])
@pytest.mark.parametrize("w,h", SIZES)
@pytest.mark.parametrize("filt", FILTERS, ids=FILTER_NAMES)
def test_matrix_vs_oracle(srcnn, oracle_lib, fmt, w, h, filt):
    for mul in MULS:
        case = (w, h, filt, mul)
        if case not in CASES:
            continue
        Y, U, V = frame(w, h, 100 * w + h)
        assert_planes(run(srcnn, FORMATS[fmt], Y, U, V, mul, filt), want_for(oracle_lib, case),
                      "%s %dx%d %s x%g" % (fmt, w, h, FILTER_NAMES[filt], mul))


def test_zero_output_size_is_refused(srcnn):
    Y, U, V = frame(1, 5, 1)
    with pytest.raises(srcnn.SrcnnError) as e:
        srcnn.yuv420_upscale(Y, U, V, multiply=0.75)
    assert e.value.code == -2


# ---- pitched and misaligned layouts: all planes in one device buffer filled with a canary ----
GUARD = 256


def layout(rows_bytes, pitches, offset):
    """Byte offsets of planes with the given (rows, row bytes) and pitches inside one buffer: GUARD bytes before and after
    every plane, each plane base at `offset` past a 64-byte boundary."""
    pos, bases = 0, []
    for (rows, _rb), p in zip(rows_bytes, pitches):
        pos += GUARD
        pos = (pos + 63) // 64 * 64 + offset
        bases.append(pos)
        pos += p * rows
    return bases, pos + GUARD


@pytest.mark.parametrize("fmt", ["i420", "nv12"])
# (offset 0 with pitches padded by multiples of 8 on a 32-wide frame: the dword / float4 forms of the conversion kernels)
@pytest.mark.parametrize("offset,pad", [(1, 1), (3, 7), (1, 64), (3, 33), (0, 0), (0, 8)])
@pytest.mark.parametrize("w,h,filt,mul", [(9, 7, 2, 2.0), (23, 17, 3, 1.5), (30, 11, 0, 2.5), (33, 20, 4, 0.75), (32, 12, 2, 2.0)])
def test_pitched_and_misaligned_vs_oracle(srcnn, oracle_lib, fmt, offset, pad, w, h, filt, mul):
    S = srcnn
    nv12 = fmt == "nv12"
    Y, U, V = frame(w, h, 7 * w + h)
    want = expected(oracle_lib, Y, U, V, mul, filt)
    dw, dh = out_size(w, h, mul)
    (cw, ch), (dcw, dch) = chroma_size(w, h), chroma_size(dw, dh)
    if nv12:
        src_planes = [Y, np.stack([U, V], -1).reshape(ch, 2 * cw)]
        dst_shapes = [(dh, dw), (dch, 2 * dcw)]
    else:
        src_planes = [Y, U, V]
        dst_shapes = [(dh, dw), (dch, dcw), (dch, dcw)]
    rb = [(p.shape[0], p.shape[1]) for p in src_planes] + list(dst_shapes)
    pitches = [r[1] + (pad + 8 * k - 1) % 64 + 1 if pad else r[1] for k, r in enumerate(rb)]     # padded by 1..64 bytes
    bases, total = layout(rb, pitches, offset)
    host = np.full(total, CANARY, np.uint8)
    for p, b, pt in zip(src_planes, bases, pitches):
        for r in range(p.shape[0]):
            host[b + r * pt: b + r * pt + p.shape[1]] = p[r]
    buf = S.DeviceBuffer.from_numpy(host)
    n = len(src_planes)
    src = [(buf, b) for b in bases[:n]] + [None] * (3 - n)
    dst = [(buf, b) for b in bases[n:]] + [None] * (3 - n)
    S.yuv420_upscale_dev(FORMATS[fmt], w, h, mul, filt, src, pitches[:n] + [0] * (3 - n), dst, pitches[n:] + [0] * (3 - n))
    S.sync()
    back = buf.to_numpy(np.uint8, (total,))
    expect = host.copy()
    outs = [want[0], np.stack([want[1], want[2]], -1).reshape(dch, 2 * dcw)] if nv12 else list(want)
    for p, b, pt in zip(outs, bases[n:], pitches[n:]):
        for r in range(p.shape[0]):
            expect[b + r * pt: b + r * pt + p.shape[1]] = p[r]
    if not np.array_equal(back, expect):
        bad = np.flatnonzero(back != expect)
        where = ["plane %d" % k for k, b in enumerate(bases) if b <= bad[0] < b + pitches[k] * rb[k][0]] or ["guard"]
        raise AssertionError("%d bytes differ, first at byte %d (%s): got %d want %d" % (len(bad), bad[0], where[0], back[bad[0]], expect[bad[0]]))


# ---- frames of the sizes the library is for ----
def test_1080p_nv12_to_4k_and_banded(srcnn, oracle_lib):
    S = srcnn
    w, h = 1920, 1080
    Y, U, V = frame(w, h, 4242)
    want = expected(oracle_lib, Y, U, V, 2.0, 2)
    got = run(S, NV12, Y, U, V, 2.0, 2)
    assert_planes(got, want, "1920x1080 nv12 x2")
    limit = 64 << 20
    band = max(16, limit // (32 * 3840 * 4) - 4)
    assert -(-2160 // band) >= 4
    prev = S.lib().srcnn_set_workspace_limit(limit)
    try:
        banded = run(S, NV12, Y, U, V, 2.0, 2)
    finally:
        S.lib().srcnn_set_workspace_limit(prev)
    assert_planes(banded, got, "1920x1080 nv12 x2 in %d-row bands" % band)


def test_4k_i420_to_8k_vs_library_float_path(srcnn):
    S = srcnn
    w, h = 3840, 2160
    Y, U, V = frame(w, h, 8080)
    got = run(S, I420, Y, U, V, 2.0, 2)
    dw, dh = 2 * w, 2 * h
    (cw, ch), (dcw, dch) = chroma_size(w, h), chroma_size(dw, dh)
    din = S.DeviceBuffer.from_numpy(Y.astype(np.float32))
    dout = S.DeviceBuffer(dw * dh * 4)
    S.check(S.lib().srcnn_y_path_f32_dev(din.ptr, w, h, dw, dh, 2, dout.ptr, None))
    S.sync()
    want_y = dout.to_numpy(np.float32, (dh, dw)).astype(np.uint8)
    del din, dout
    want_c = [np.clip(S.resample(P.astype(np.float32), dcw, dch, 1), 0, 255).astype(np.uint8) for P in (U, V)]
    assert_planes(got, [want_y] + want_c, "3840x2160 i420 x2")


# ---- SRCNN_RESAMPLE_2PASS=1 (read when the library loads): the small matrix in a child process ----
_CHILD = r"""
import json, sys
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + "/tests")
import libsrcnn_amd as S
import test_gpu_yuv as T
S.init(0)
assert "SRCNN_RESAMPLE_2PASS=1" in S.debug_settings()
out = {}
for fmt in (T.I420, T.NV12):
    for case in T.CASES:
        w, h, filt, mul = case
        Y, U, V = T.frame(w, h, 100 * w + h)
        out["%d/%r" % (fmt, case)] = T.digest(T.run(S, fmt, Y, U, V, mul, filt))
print("DIGESTS " + json.dumps(out))
"""


def test_resample_2pass_variant_vs_oracle(srcnn, oracle_lib):
    r = subprocess.run([sys.executable, "-c", _CHILD, ROOT], env=dict(os.environ, SRCNN_RESAMPLE_2PASS="1"),
                       capture_output=True, text=True, timeout=600)
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("DIGESTS ")]
    assert r.returncode == 0 and line, r.stdout[-400:] + r.stderr[-800:]
    got = json.loads(line[0][8:])
    bad = [(fmt, case) for fmt in (I420, NV12) for case in CASES
           if got["%d/%r" % (fmt, case)] != digest(want_for(oracle_lib, case))]
    assert not bad, "%d cases differ from the oracle under SRCNN_RESAMPLE_2PASS=1: %s" % (len(bad), bad[:10])


# ---- two host threads on two streams ----
def test_two_threads_two_streams(srcnn):
    S = srcnn
    frames = [frame(97, 61, 500 + k) for k in range(8)]
    cases = [(NV12 if k % 2 else I420, 2.0 if k % 3 else 1.5, FILTERS[k % 5]) for k in range(8)]
    single = [run(S, fmt, *fr, mul, filt) for fr, (fmt, mul, filt) in zip(frames, cases)]
    results, errors = [None] * 8, []

    def worker(t):
        st = S.Stream()
        try:
            for k in range(t, 8, 2):
                fmt, mul, filt = cases[k]
                results[k] = run(S, fmt, *frames[k], mul, filt, stream=st)
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


# ---- tools/srcnnyuv ----
def test_srcnnyuv_y4m_vs_oracle(srcnn, oracle_lib, tmp_path):
    w, h, mul, filt = 37, 21, 2.5, 3
    dw, dh = out_size(w, h, mul)
    tags_in = "YUV4MPEG2 W%d H%d F30000:1001 Ip A1:1 C420jpeg XYSCSS=420JPEG" % (w, h)
    params = ["", " Ixyz", " XFOO=1"]
    frames = [frame(w, h, 900 + k) for k in range(3)]
    data = tags_in.encode() + b"\n"
    for p, (Y, U, V) in zip(params, frames):
        data += b"FRAME" + p.encode() + b"\n" + Y.tobytes() + U.tobytes() + V.tobytes()
    (tmp_path / "in.y4m").write_bytes(data)
    exe = os.path.join(ROOT, "libsrcnn_amd", "bin", "srcnnyuv")
    r = subprocess.run([exe, "--scale", "2.5", "--filter", "lanczos3", str(tmp_path / "in.y4m"), "-"], capture_output=True,
                       timeout=300)
    assert r.returncode == 0, r.stderr[-800:]
    out = r.stdout
    header, rest = out.split(b"\n", 1)
    assert header.decode() == tags_in.replace("W%d H%d" % (w, h), "W%d H%d" % (dw, dh))
    (dcw, dch) = chroma_size(dw, dh)
    for p, (Y, U, V) in zip(params, frames):
        line, rest = rest.split(b"\n", 1)
        assert line.decode() == "FRAME" + p
        n = dw * dh + 2 * dcw * dch
        body, rest = rest[:n], rest[n:]
        got = (np.frombuffer(body[:dw * dh], np.uint8).reshape(dh, dw),
               np.frombuffer(body[dw * dh:dw * dh + dcw * dch], np.uint8).reshape(dch, dcw),
               np.frombuffer(body[dw * dh + dcw * dch:], np.uint8).reshape(dch, dcw))
        assert_planes(got, expected(oracle_lib, Y, U, V, mul, filt), "srcnnyuv frame" + p)
    assert rest == b""
