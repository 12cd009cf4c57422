"""srcnn_rgb_upscale_dev (include/srcnn_amd_rgb.h) byte for byte against the oracle (GPU).

Expected RGB(A) and dst_conv come from oracle.process at depth 8 and from the numpy restatement of tests/test_rgb_restatement.py
above that (pinned to oracle.process by that module's CPU tests) -- never from the library itself, except where the contract
says "the bytes of srcnn_process_u8" (the identity size).  Content is noise beside saturated blocks of 0 and maxv, so the merge
clips at both ends.  Every process these tests start runs under a timeout of its own and nothing is tried twice.
"""
import json
import os
import subprocess
import sys
import threading

import numpy as np
import pytest

from test_gpu_yuv import FILTER_NAMES, FILTERS, first_difference, out_size
from test_rgb_restatement import DEPTHS, LAYOUTS, ORDERS, cases_for, dtype_of, image, restatement, seed_of, want_for

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORKER = os.path.join(ROOT, "tests", "rgb_worker.py")
CANARY = 0xA5
GUARD = 256


def arrange(img, layout, order):
    """(h, w, c) in R, G, B[, A] order -> the array the format holds: channels reordered, (c, h, w) when planar."""
    c = img.shape[2]
    idx = ([2, 1, 0] if order == "bgr" else [0, 1, 2]) + ([3] if c == 4 else [])
    a = img[..., idx]
    return np.ascontiguousarray(a.transpose(2, 0, 1) if layout == "planar" else a)


def canonical(arr, layout, order):
    """The inverse of arrange."""
    a = arr.transpose(1, 2, 0) if layout == "planar" else arr
    c = a.shape[2]
    idx = ([2, 1, 0] if order == "bgr" else [0, 1, 2]) + ([3] if c == 4 else [])
    return np.ascontiguousarray(a[..., idx])


def run(S, img, layout, order, depth, mul, filt, stream=None, raw=None):
    """The library's (out, conv) for an R, G, B[, A] image, back in that order, whatever the format."""
    src = arrange(img if raw is None else raw, layout, order)
    out, conv = S.rgb_upscale(src, multiply=mul, filt=filt, layout=layout, order=order, depth=depth, want_conv=True, stream=stream)
    assert out.dtype == conv.dtype == dtype_of(depth)
    if depth > 8:       # high bits of outputs are zero: nothing above the ceiling 255 * 2^s
        assert int(out.max()) <= 255 << (depth - 8) and int(conv.max()) <= 255 << (depth - 8)
    return canonical(out, layout, order), conv


def assert_same(got, want, what):
    for name, g, e in zip(("out", "conv"), got, want):
        assert g.shape == e.shape and g.dtype == e.dtype, (what, name, g.shape, e.shape, g.dtype, e.dtype)
        assert np.array_equal(g, e), "%s %s: %s" % (what, name, first_difference(g, e))


# ---- the matrix ----
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("alpha", [0, 1], ids=["rgb", "rgba"])
@pytest.mark.parametrize("depth", DEPTHS)
def test_matrix_vs_oracle(srcnn, oracle_lib, layout, order, alpha, depth):
    for case in cases_for(layout, order, alpha, depth):
        w, h, filt, mul = case
        img = image(w, h, alpha, depth, seed_of(w, h))
        assert_same(run(srcnn, img, layout, order, depth, mul, filt), want_for(oracle_lib, alpha, depth, case),
                    "%s %s alpha=%d %d-bit %dx%d %s x%g" % (layout, order, alpha, depth, w, h, FILTER_NAMES[filt], mul))


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("depth", [10, 12, 14])
def test_stray_high_bits_are_ignored(srcnn, oracle_lib, layout, depth):
    w, h, mul, filt = 37, 21, 2.0, 2
    img = image(w, h, 1, depth, 77)
    junk = np.random.default_rng(depth).integers(0, 1 << (16 - depth), img.shape).astype(np.uint16) << depth
    assert np.any(junk)
    want = restatement(oracle_lib, img, depth, mul, filt)
    assert_same(run(srcnn, img, layout, "rgb", depth, mul, filt), want, "clean")
    assert_same(run(srcnn, img, layout, "rgb", depth, mul, filt, raw=img | junk), want, "stray bits")


def test_zero_output_size_is_refused(srcnn):
    with pytest.raises(srcnn.SrcnnError) as e:
        srcnn.rgb_upscale(image(1, 5, 0, 8, 1), multiply=0.75)
    assert e.value.code == -2


# ---- the identity size: the bytes of srcnn_process_u8 (the library's pinned deviation from the reference) ----
@pytest.mark.parametrize("alpha", [0, 1], ids=["rgb", "rgba"])
def test_identity_size_gives_the_bytes_of_process_u8(srcnn, alpha):
    S = srcnn
    for k, (w, h) in enumerate(((23, 17), (64, 40), (9, 7), (1, 5), (130, 66))):
        filt = FILTERS[k % 5]
        img = image(w, h, alpha, 8, 3 * w + h)
        want = S.process_u8(img, 1.0, filt, want_conv=True)
        assert want[0].shape == img.shape
        for layout in LAYOUTS:
            for order in ORDERS:
                assert_same(run(S, img, layout, order, 8, 1.0, filt), want, "identity %s %s %dx%d f%d" % (layout, order, w, h, filt))


# ---- pitched and misaligned layouts: all planes in one device buffer filled with a canary ----
def layout_bases(rows, pitches, offset):
    pos, bases = 0, []
    for r, p in zip(rows, pitches):
        pos += GUARD
        pos = (pos + 63) // 64 * 64 + offset
        bases.append(pos)
        pos += p * r
    return bases, pos + GUARD


@pytest.mark.parametrize("layout", LAYOUTS)
# odd offsets past a 64-byte boundary with pads that break dword alignment (depth 8 only: above it offsets and pads are even),
# and the fully aligned case: both forms of the conversion kernels.  Every plane gets a pitch of its own.
@pytest.mark.parametrize("offset,pad", [(1, 1), (3, 7), (2, 2), (6, 14), (2, 64), (0, 0), (0, 16)])
@pytest.mark.parametrize("w,h,filt,mul,order,alpha,depth", [(9, 7, 2, 2.0, "rgb", 0, 8), (23, 17, 3, 1.5, "bgr", 1, 8),
                                                            (30, 11, 0, 2.5, "bgr", 0, 16), (33, 20, 4, 0.75, "rgb", 1, 10),
                                                            (32, 16, 2, 2.0, "rgb", 0, 8), (32, 16, 1, 2.0, "bgr", 1, 12),
                                                            (16, 8, 2, 1.0, "rgb", 1, 8)])
def test_pitched_and_misaligned_vs_oracle(srcnn, oracle_lib, layout, offset, pad, w, h, filt, mul, order, alpha, depth):
    S = srcnn
    if depth > 8 and (offset % 2 or pad % 2):
        offset, pad = offset + 1, pad + 1                 # 16-bit planes: even addresses and pitches (still not dword aligned)
    img = image(w, h, alpha, depth, 7 * w + h)
    if mul == 1.0:
        want = S.process_u8(img, 1.0, filt, want_conv=True)            # the identity size: the contract names the host call
    else:
        want = oracle_lib.process(img, mul, filt) if depth == 8 else restatement(oracle_lib, img, depth, mul, filt)
    src, out = arrange(img, layout, order), arrange(want[0], layout, order)
    as_rows = lambda a: [np.ascontiguousarray(p).reshape(p.shape[0], -1).view(np.uint8) for p in (a if layout == "planar" else [a])]   # noqa: E731
    src_planes, out_planes = as_rows(src), as_rows(out) + [np.ascontiguousarray(want[1]).view(np.uint8)]
    n = len(src_planes)
    allp = src_planes + out_planes
    rows = [p.shape[0] for p in allp]
    pitches = [p.shape[1] + (pad + 16 * k if pad % 16 == 0 else pad + 4 * k) if pad else p.shape[1] for k, p in enumerate(allp)]
    bases, total = layout_bases(rows, pitches, offset)
    host = np.full(total, CANARY, np.uint8)
    for p, b, pt in zip(src_planes, bases, pitches):
        for r in range(p.shape[0]):
            host[b + r * pt: b + r * pt + p.shape[1]] = p[r]
    buf = S.DeviceBuffer.from_numpy(host)
    S.rgb_upscale_dev(S.rgb_format(layout, order, alpha, depth), w, h, mul, filt, [(buf, b) for b in bases[:n]], pitches[:n],
                      [(buf, b) for b in bases[n:2 * n]], pitches[n:2 * n], (buf, bases[2 * n]), pitches[2 * n])
    S.sync()
    back = buf.to_numpy(np.uint8, (total,))
    expect = host.copy()
    for p, b, pt in zip(out_planes, bases[n:], pitches[n:]):
        for r in range(p.shape[0]):
            expect[b + r * pt: b + r * pt + p.shape[1]] = p[r]
    if not np.array_equal(back, expect):
        bad = np.flatnonzero(back != expect)
        where = ["plane %d" % k for k, b in enumerate(bases) if b <= bad[0] < b + pitches[k] * rows[k]] or ["guard"]
        raise AssertionError("%d bytes differ, first at byte %d (%s): got %d want %d" % (len(bad), bad[0], where[0], back[bad[0]], expect[bad[0]]))


def test_no_conv_plane_and_tight_defaults(srcnn, oracle_lib):
    """dst_conv = NULL, NULL pitch arrays: the image alone, same bytes."""
    S = srcnn
    img = image(23, 17, 1, 8, 5)
    want, _ = oracle_lib.process(img, 2.0, 2)
    for layout in LAYOUTS:
        out, conv = S.rgb_upscale(arrange(img, layout, "rgb"), multiply=2.0, filt=2, layout=layout, want_conv=False)
        assert conv is None and np.array_equal(canonical(out, layout, "rgb"), want), layout


# ---- the fused shell (8-bit interleaved RGB, tight) and the plane shell (everything else) give the same bytes ----
def shell_results(S):
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import rgb_worker
    return rgb_worker.shell_cases(), rgb_worker.run_shell(S)


def test_fast_path_and_general_path_agree(srcnn, oracle_lib):
    S = srcnn
    import rgb_worker
    cases, fast = shell_results(S)
    assert any(img.shape[1] >= 512 and img.shape[0] >= 300 and mul == 2.0 for (_n, img, mul, _f) in cases)
    for (name, img, mul, filt) in cases:
        h, w, c = img.shape
        dw, dh = out_size(w, h, mul)
        want = oracle_lib.process(img, mul, filt)
        assert fast[name] == rgb_worker.digest(*want), "tight interleaved RGB (fused shell) vs oracle: " + name
        assert_same(S.process_u8(img, mul, filt, want_conv=True), want, "srcnn_process_u8 " + name)
        # the plane shell: BGR order, and a pitched RGB destination
        assert_same(run(S, img, "interleaved", "bgr", 8, mul, filt), want, "BGR " + name)
        assert_same(run(S, img, "planar", "rgb", 8, mul, filt), want, "planar " + name)
        src = S.DeviceBuffer.from_numpy(img)
        pitch = dw * c + 20
        dst, conv = S.DeviceBuffer(pitch * dh), S.DeviceBuffer(dw * dh)
        S.rgb_upscale_dev(S.rgb_format("interleaved", "rgb", c == 4, 8), w, h, mul, filt, [src], None, [dst], [pitch], conv, 0)
        S.sync()
        got = dst.to_numpy(np.uint8, (dh, pitch))[:, :dw * c].reshape(dh, dw, c)
        assert_same((got, conv.to_numpy(np.uint8, (dh, dw))), want, "pitched destination " + name)


def child(mode, env=None, timeout=600):
    r = subprocess.run([sys.executable, WORKER, mode], env=dict(os.environ, **(env or {})), capture_output=True, text=True, timeout=timeout)
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")]
    assert r.returncode == 0 and line, "rgb_worker %s: exit %d\n%s\n%s" % (mode, r.returncode, r.stdout[-600:], r.stderr[-1500:])
    return json.loads(line[0][7:])


def test_forced_plane_shell_gives_the_same_bytes(srcnn):
    """SRCNN_SHELL_UNFUSED=1 (read when the library loads) sends the tight 8-bit RGB call down the general path."""
    _cases, fast = shell_results(srcnn)
    assert child("unfused", env={"SRCNN_SHELL_UNFUSED": "1"}) == fast


# ---- the workspace cap ----
@pytest.mark.parametrize("order", ORDERS, ids=["fused-shell", "plane-shell"])
def test_workspace_cap_bands_give_the_same_bytes(srcnn, order):
    S = srcnn
    w, h = 1280, 720
    img = image(w, h, 0, 8, 4242)
    whole = run(S, img, "interleaved", order, 8, 2.0, 2)
    limit = 48 << 20
    band = max(16, limit // (32 * 2 * w * 4) - 4)
    assert -(-2 * h // band) >= 3
    prev = S.lib().srcnn_set_workspace_limit(limit)
    try:
        banded = run(S, img, "interleaved", order, 8, 2.0, 2)
    finally:
        S.lib().srcnn_set_workspace_limit(prev)
    assert_same(banded, whole, "1280x720 x2 in %d-row bands" % band)
    assert_same(whole, S.process_u8(img, 2.0, 2, want_conv=True), "1280x720 x2 vs srcnn_process_u8")


# ---- two host threads on two streams, mixed formats; a second context ----
def test_two_threads_two_streams(srcnn):
    S = srcnn
    cases = [(LAYOUTS[k % 2], ORDERS[(k // 2) % 2], k % 3 == 0, DEPTHS[k % 5], 2.0 if k % 3 else 1.5, FILTERS[k % 5]) for k in range(8)]
    images = [image(97, 61, int(c[2]), c[3], 500 + k) for k, c in enumerate(cases)]
    call = lambda k, st=None: run(S, images[k], cases[k][0], cases[k][1], cases[k][3], cases[k][4], cases[k][5], stream=st)   # noqa: E731
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
        assert_same(results[k], single[k], "image %d on thread %d" % (k, k % 2))


def test_second_context_through_its_own_stream(srcnn, oracle_lib):
    import rgb_worker
    res = child("second_context")
    for k, (alpha, depth, layout, order) in enumerate(((0, 8, "interleaved", "rgb"), (1, 12, "planar", "bgr"))):
        img = image(97, 61, alpha, depth, 300 + k)
        out, conv = oracle_lib.process(img, 2.0, 2) if depth == 8 else restatement(oracle_lib, img, depth, 2.0, 2)
        want = rgb_worker.digest(arrange(out, layout, order), conv)
        assert res["case%d" % k] == [want, want], (k, layout, order)


# ---- torch tensors ----
def test_torch_tensors_vs_oracle(oracle_lib):
    import rgb_worker
    res = child("torch")
    if "skip" in res:
        pytest.skip(res["skip"])
    img = image(37, 21, 0, 8, 11)
    assert res["hwc3"]["sha"] == rgb_worker.digest(*oracle_lib.process(img, 2.0, 2)), "(H, W, 3) uint8"
    assert res["hwc3"]["device"] == res["device"] and res["hwc3"]["shape"] == [42, 74, 3] and res["hwc3"]["contig"]
    img = image(30, 11, 1, 12, 12)
    assert res["chw4"]["sha"] == rgb_worker.digest(*restatement(oracle_lib, img, 12, 2.5, 3)), "(4, H, W) 12-bit BGR"
    assert res["chw4"]["device"] == res["device"] and res["chw4"]["shape"] == [4, 27, 75]
    wide = image(48, 19, 0, 8, 13)
    assert res["strided"]["sha"] == rgb_worker.digest(*oracle_lib.process(np.ascontiguousarray(wide[:, 3:40, :]), 1.5, 1)), "row-strided view"
    assert res["strided"]["device"] == res["device"] and res["strided"]["shape"] == [28, 55, 3]
    assert res["permuted"]["sha"] == rgb_worker.digest(oracle_lib.process(wide, 2.0, 2)[0]) and res["permuted"]["shape"] == [38, 96, 3]
    assert res["permuted"]["strides"] == [96, 1, 38 * 96]
    assert res["refused"] == [True] * 5
