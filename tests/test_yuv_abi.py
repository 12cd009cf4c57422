"""CPU: the YUV 4:2:0 extension (include/srcnn_amd_yuv.h) -- its declared functions, committed list, binding and export table
agree (full and strict-only builds), every argument rule of srcnn_yuv420_upscale_dev returns its code before any device
lookup, and tools/srcnnyuv refuses the YUV4MPEG2 streams it does not handle with status 2 without touching a device."""
import os
import re
import subprocess

import numpy as np
import pytest

from test_abi import HANDLE_ONLY_HOOKS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_ARG, E_SCALE, E_NODEVICE, E_UNSUPPORTED = -1, -2, -200, -203
I420, NV12 = 0, 1


@pytest.fixture(scope="module")
def S():
    import libsrcnn_amd as S
    from libsrcnn_amd import build
    if build.stale() or not os.path.exists(os.path.join(ROOT, "libsrcnn_amd", "bin", "srcnnyuv")):
        build.build(verbose=False)
    return S


def _declared(header):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", header)).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(srcnn_[a-z0-9_]+)\s*\(", text)))


def _exported(path):
    out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
    return sorted(line.split()[-1] for line in out.splitlines() if line.strip())


def test_yuv_header_list_binding_and_exports_agree(S):
    names = _declared("srcnn_amd_yuv.h")
    listed = [ln.strip() for ln in open(os.path.join(ROOT, "include", "srcnn_amd_yuv.abi")) if ln.strip() and not ln.startswith("#")]
    assert listed == sorted(listed) and len(set(listed)) == len(listed)
    assert names == listed == sorted(S.YUV_SYMBOLS)
    assert set(S.YUV_SYMBOLS) <= set(S.C_ABI_SYMBOLS)
    assert not set(names) & set(_declared("srcnn_amd.h")), "the extension must not touch the frozen header"
    header = open(os.path.join(ROOT, "include", "srcnn_amd_yuv.h")).read()
    assert "#define SRCNN_AMD_YUV_VERSION 1" in header and '#include "srcnn_amd.h"' in header
    assert "#define SRCNN_YUV_I420 0" in header and "#define SRCNN_YUV_NV12 1" in header
    exported = _exported(S.LIB_PATH)
    assert set(names) <= set(exported)
    assert exported == sorted(S.C_ABI_SYMBOLS + S.CXX_SYMBOLS + HANDLE_ONLY_HOOKS)
    assert S.lib().srcnn_yuv_abi_version() == 1


def test_strict_only_build_exports_the_yuv_call(S):
    from libsrcnn_amd import build
    strict, _ = build.build_strict_only(verbose=False)
    assert _exported(strict) == _exported(S.LIB_PATH)
    assert set(S.YUV_SYMBOLS) <= set(_exported(strict))


def test_yuv_header_compiles_as_c(tmp_path):
    src = tmp_path / "use.c"
    src.write_text('#include "srcnn_amd_yuv.h"\nint f(void) { return srcnn_yuv_abi_version() + SRCNN_YUV_NV12; }\n')
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-c", str(src), "-I" + os.path.join(ROOT, "include"),
                           "-o", str(tmp_path / "use.o")])


# ---- argument rules: host buffers stand in for device planes, which is safe because every call below is refused before
# the device is looked up ----
class Frame:
    """Host memory laid out like one frame's planes (fmt, w, h, multiply): tight unless pitches are given."""

    def __init__(self, S, fmt, w, h, mul=2.0, src_pitch=None, dst_pitch=None):
        (dw, dh), (cw, ch), (dcw, dch) = S.yuv420_sizes(w, h, mul)
        self.fmt, self.w, self.h, self.mul = fmt, w, h, mul
        cb = 2 * cw if fmt == NV12 else cw
        dcb = 2 * dcw if fmt == NV12 else dcw
        sp = src_pitch or [0, 0, 0]
        dp = dst_pitch or [0, 0, 0]
        self.src_sizes = [max(sp[0], w) * h, max(sp[1], cb) * ch, max(sp[2], cb) * ch]
        self.dst_sizes = [max(dp[0], dw) * dh, max(dp[1], dcb) * dch, max(dp[2], dcb) * dch]
        self.buf = np.zeros(sum(self.src_sizes) + sum(self.dst_sizes) + 64, np.uint8)
        base = self.buf.ctypes.data
        offs = np.cumsum([0] + self.src_sizes + self.dst_sizes)
        self.src = [base + int(o) for o in offs[:3]]
        self.dst = [base + int(o) for o in offs[3:6]]
        self.src_pitch, self.dst_pitch = src_pitch, dst_pitch

    def call(self, S, **kw):
        a = dict(fmt=self.fmt, w=self.w, h=self.h, multiply=self.mul, filt=2, src=self.src, src_pitch=self.src_pitch,
                 dst=self.dst, dst_pitch=self.dst_pitch)
        a.update(kw)
        try:
            S.yuv420_upscale_dev(a["fmt"], a["w"], a["h"], a["multiply"], a["filt"], a["src"], a["src_pitch"], a["dst"],
                                 a["dst_pitch"])
        except S.SrcnnError as e:
            return e.code
        return 0


def _raw(S, fmt, w, h, mul, filt, src, sp, dst, dp):
    return S.lib().srcnn_yuv420_upscale_dev(fmt, w, h, float(mul), filt, src, sp, dst, dp, None)


@pytest.mark.parametrize("fmt", [I420, NV12])
def test_null_planes_and_zero_sizes(S, fmt):
    f = Frame(S, fmt, 9, 7)
    for k in range(2 if fmt == NV12 else 3):
        src = list(f.src); src[k] = None
        assert f.call(S, src=src) == E_ARG
        dst = list(f.dst); dst[k] = None
        assert f.call(S, dst=dst) == E_ARG
    assert _raw(S, fmt, 9, 7, 2.0, 2, None, None, None, None) == E_ARG
    assert f.call(S, w=0) == E_ARG and f.call(S, h=0) == E_ARG


def test_format_and_filter(S):
    f = Frame(S, I420, 9, 7)
    for fmt in (2, -1, 99):
        assert f.call(S, fmt=fmt) == E_ARG
    for filt in (-1, 5, 100):
        assert f.call(S, filt=filt) == E_ARG


def test_nv12_ignores_the_third_plane(S):
    if S.device_count() > 0:
        pytest.skip("a device is present: a valid call would run on host memory")
    f = Frame(S, NV12, 9, 7)
    assert f.call(S, src=[f.src[0], f.src[1], None], dst=[f.dst[0], f.dst[1], None]) == E_NODEVICE


@pytest.mark.parametrize("fmt", [I420, NV12])
def test_short_pitches(S, fmt):
    w, h = 9, 7                     # chroma rows of ceil(9/2) = 5 samples: 5 bytes (I420), 10 bytes (NV12)
    (dw, _), _, (dcw, _) = S.yuv420_sizes(w, h, 2.0)
    cb, dcb = (10, 2 * dcw) if fmt == NV12 else (5, dcw)
    big = Frame(S, fmt, w, h, src_pitch=[64, 64, 64], dst_pitch=[64, 64, 64])
    assert big.call(S, src_pitch=[w - 1, 0, 0]) == E_ARG
    assert big.call(S, src_pitch=[0, cb - 1, 0]) == E_ARG
    assert big.call(S, dst_pitch=[dw - 1, 0, 0]) == E_ARG
    assert big.call(S, dst_pitch=[0, dcb - 1, 0]) == E_ARG
    if fmt == NV12:
        assert big.call(S, src_pitch=[0, 5, 0]) == E_ARG            # ceil(w/2): one byte per pair is not a UV row
        assert big.call(S, dst_pitch=[0, dcw, 0]) == E_ARG
    else:
        assert big.call(S, src_pitch=[0, 0, cb - 1]) == E_ARG
        assert big.call(S, dst_pitch=[0, 0, dcb - 1]) == E_ARG
    if S.device_count() == 0:
        # exactly the row length, and 0 (= tight), are valid
        assert big.call(S, src_pitch=[w, cb, cb], dst_pitch=[dw, dcb, dcb]) == E_NODEVICE
        assert big.call(S, src_pitch=[0, 0, 0], dst_pitch=None) == E_NODEVICE


def test_multiply_giving_zero_size(S):
    f = Frame(S, I420, 9, 7)
    for mul in (0.0, -1.0, 0.1, 0.05, float("nan")):
        assert f.call(S, multiply=mul) == E_SCALE, mul


def test_sizes_beyond_the_y_path(S):
    f = Frame(S, I420, 9, 7)
    assert f.call(S, w=1 << 22, h=2, multiply=4.0) == E_UNSUPPORTED
    assert f.call(S, w=2, h=1 << 20, multiply=2.0) == E_UNSUPPORTED
    assert f.call(S, w=60000, h=60000, multiply=2.0) == E_UNSUPPORTED
    assert f.call(S, multiply=float("inf")) == E_UNSUPPORTED


@pytest.mark.parametrize("fmt", [I420, NV12])
def test_overlapping_planes(S, fmt):
    f = Frame(S, fmt, 9, 7)
    np_ = 2 if fmt == NV12 else 3
    for a in range(np_):
        for b in range(np_):
            dst = list(f.dst); dst[b] = f.src[a]                        # same start
            assert f.call(S, dst=dst) == E_ARG, (a, b)
            dst = list(f.dst); dst[b] = f.src[a] + f.src_sizes[a] - 1  # output starts on the input's last byte
            assert f.call(S, dst=dst) == E_ARG, (a, b)
    # an output that ends on the first byte of an input
    dst = list(f.dst); dst[0] = f.src[0] - f.dst_sizes[0] + 1
    assert f.call(S, dst=dst) == E_ARG
    # the padding bytes of a pitched input row count: an output inside the last row's padding is fine, one inside an
    # earlier row's padding is not
    g = Frame(S, fmt, 9, 7, src_pitch=[32, 32, 32])
    dst = list(g.dst); dst[1] = g.src[0] + 32 * 6 - 16
    assert g.call(S, dst=dst) == E_ARG


def test_valid_call_without_a_device(S):
    if S.device_count() > 0:
        pytest.skip("a device is present")
    for fmt in (I420, NV12):
        for (w, h, mul) in ((9, 7, 2.0), (1, 1, 3.0), (16, 8, 0.75)):
            assert Frame(S, fmt, w, h, mul).call(S) == E_NODEVICE


# ---- tools/srcnnyuv ----
def _srcnnyuv():
    return os.path.join(ROOT, "libsrcnn_amd", "bin", "srcnnyuv")


@pytest.mark.parametrize("tags", ["C422", "C444", "C420p10", "C420p12", "Cmono", "C444alpha", "It", "Ib", "Im",
                                  "C420jpeg It"])
def test_srcnnyuv_refuses_before_touching_the_device(S, tmp_path, tags):
    src = tmp_path / "in.y4m"
    src.write_bytes(b"YUV4MPEG2 W8 H6 F25:1 " + tags.encode() + b"\nFRAME\n" + bytes(8 * 6 * 3))
    # HIP_VISIBLE_DEVICES=-1 hides every device: a refusal that touched one would fail differently (or not at all)
    r = subprocess.run([_srcnnyuv(), str(src), str(tmp_path / "out.y4m")], capture_output=True, text=True, timeout=60,
                       env=dict(os.environ, HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1"))
    assert r.returncode == 2, (r.returncode, r.stderr)
    assert len(r.stderr.strip().splitlines()) == 1 and "srcnnyuv:" in r.stderr
    assert not (tmp_path / "out.y4m").exists()


def test_srcnnyuv_usage_errors(S, tmp_path):
    for args in ([], ["--filter", "sinc", "-", "-"], ["--scale", "x", "-", "-"], ["a"]):
        r = subprocess.run([_srcnnyuv()] + args, capture_output=True, text=True, timeout=60, stdin=subprocess.DEVNULL)
        assert r.returncode == 2, (args, r.returncode)
    r = subprocess.run([_srcnnyuv(), "-", "-"], input=b"P6 4 4 255\n", capture_output=True, timeout=60)
    assert r.returncode == 2
