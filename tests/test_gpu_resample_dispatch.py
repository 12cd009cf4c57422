"""Every plane-resample kernel cell, bit for bit against the oracle (GPU).

srcnn_resample_f32_dev and srcnn_y_path_f32 pick a kernel by ratio, filter, width and destination alignment
(tests/resample_dispatch.py names the cell; tests/test_resample_dispatch_model.py checks on the CPU that PLANE_CASES reach
every reachable cell for every filter).  Each case runs for all five filters; the destination sits between guard bands, and
the cases whose width is a multiple of 4 run a second time with the destination 4 bytes into a larger buffer (scalar stores
instead of 16-byte ones).  SRCNN_RS_DMA=0 and SRCNN_RESAMPLE_2PASS=1 are read when the library loads: those runs repeat the
plane resamples in a subprocess each, which prints digests that are compared with the oracle's here.
"""
import ctypes as C
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import assert_bit_equal
from libsrcnn_amd import synth
import resample_dispatch as M

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GUARD = 4096

# (sh, sw, dh, dw).  Ratios just above 1, between 1 and 2, 2, above 2, down-scales, mixed axes in both orders, one axis
# unchanged, the identity, every dw % 4, tiny sources (3- and 5-tap tables of the long filters), short tall planes (the
# LDS-DMA form with wide LDS rows) and plain planes of more than 65 535 rows for the two generic passes.
PLANE_CASES = [
    (24, 40, 48, 80),          # x2, dw % 4 == 0
    (24, 41, 48, 82),          # x2, dw % 4 == 2
    (25, 37, 62, 92),          # x2.5
    (25, 38, 62, 95),          # x2.5, dw % 4 == 3
    (30, 23, 150, 115),        # x5, dw % 4 == 3
    (20, 30, 160, 240),        # x8
    (100, 200, 101, 202),      # x1.01 (wide LDS rows)
    (48, 160, 60, 200),        # x1.25
    (20, 150, 30, 225),        # x1.5, dw % 4 == 1
    (6, 152, 12, 228),         # x1.5 wide x2 tall on a short plane: LDS-DMA with wide rows
    (4, 150, 8, 225),          # the same, dw % 4 == 1
    (5, 160, 10, 200),         # x1.25 wide x2 tall: monotone Mitchell tables (x1.5 ones are not)
    (4, 200, 8, 250),          # the same, dw % 4 == 2
    (3, 3, 9, 12),             # 3-sample axes: 3-tap tables for every filter
    (2, 3, 6, 9),
    (5, 4, 15, 12),            # 4/5-sample axes: 5-tap tables for Lanczos3
    (4, 5, 12, 15),
    (9, 13, 27, 39),           # x3: non-monotone Mitchell / B-spline tables (two-pass, vertical first)
    (40, 60, 20, 30),          # x0.5
    (40, 60, 30, 45),          # x0.75
    (50, 70, 15, 21),          # x0.3
    (40, 30, 20, 60),          # up-w, down-h: vertical first
    (30, 40, 60, 20),          # down-w, up-h: horizontal first
    (30, 40, 30, 80),          # rows only, up
    (30, 40, 30, 21),          # rows only, down
    (30, 40, 60, 40),          # cols only, up
    (30, 40, 13, 40),          # cols only, down
    (30, 40, 30, 40),          # identity
]
# two-pass launches of more than 65 535 rows (the kernels' grid is capped there and strides over the rest)
TALL_CASES = [
    (50000, 3, 100000, 2),     # horizontal first, then a vertical pass of 100 000 rows
    (70000, 2, 70000, 3),      # rows only, 70 000 rows
    (140000, 2, 70000, 3),     # vertical first (down-h, up-w), 70 000 rows in both passes
]
SPECIAL_CASE = 0               # this case also runs on a plane with step edges and special values


def plane_input(i, sh, sw):
    return synth.plane(sh, sw, synth.SEED0 + 500 + i, "noise" if i & 1 else "smooth")


def special_plane(sh, sw):
    """Step edges (0 / 255 blocks), then the special values of test_special_values_match_reference_semantics."""
    y = np.zeros((sh, sw), np.float32)
    y[:, sw // 3: 2 * sw // 3] = 255.0
    y[sh // 2:, :] = 255.0 - y[sh // 2:, :]
    y[2, 3] = 1e-40
    y[2, 4] = -1e-42
    y[5, 7] = -0.0
    y[9, 9] = 3e30
    y[9, 30] = -3e30
    y[15, 20] = np.inf
    y[18, 5] = -np.inf
    y[21, 33] = np.nan
    return y


def offsets(dw):
    return (0, 4) if dw % 4 == 0 else (0,)


def case_id(c):
    return "%dx%d-to-%dx%d" % (c[1], c[0], c[3], c[2])


def same_values(got, want, what):
    """NaN-ness first, then bits everywhere else (NaN payloads are not part of the contract)."""
    assert got.shape == want.shape, (what, got.shape, want.shape)
    assert np.array_equal(np.isnan(got), np.isnan(want)), what + ": NaN positions differ"
    ok = ~np.isnan(want)
    assert_bit_equal(np.where(ok, got, 0), np.where(ok, want, 0), what)


def guarded_resample(S, y, dw, dh, filt, off):
    """srcnn_resample_f32_dev into a destination `off` bytes into a buffer with GUARD bytes of 0xA5 on either side."""
    L = S.lib()
    sh, sw = y.shape
    nbytes = dw * dh * 4
    src = S.DeviceBuffer.from_numpy(y)
    buf = S.DeviceBuffer(nbytes + 2 * GUARD + off)
    S.check(L.srcnn_memset_dev(buf.ptr, 0xA5, buf.nbytes, None))
    S.check(L.srcnn_resample_f32_dev(src.ptr, sw, sh, dw, dh, filt, buf.ptr + GUARD + off, None))
    S.sync()
    raw = buf.to_numpy(np.uint8, (buf.nbytes,))
    intact = bool((raw[:GUARD + off] == 0xA5).all() and (raw[GUARD + off + nbytes:] == 0xA5).all())
    out = raw[GUARD + off: GUARD + off + nbytes].view(np.float32).reshape(dh, dw).copy()
    return out, intact


def expected_resample(oracle_lib, y, dw, dh, filt):
    sh, sw = y.shape
    if (sw, sh) == (dw, dh):
        return y.copy()     # the identity copies the whole plane (test_identity_size_deviation_is_pinned)
    return oracle_lib.resample(y, dw, dh, filt)


def cell(filt, c, off=0, settings=M.DEFAULT):
    sh, sw, dh, dw = c
    return M.plane_cell(filt, sw, sh, dw, dh, settings, dst_aligned16=off % 16 == 0)


@pytest.mark.parametrize("filt", M.FILTERS, ids=M.FILTER_NAMES)
def test_plane_resample_every_cell_vs_oracle(srcnn, oracle_lib, filt):
    for i, c in enumerate(PLANE_CASES):
        sh, sw, dh, dw = c
        inputs = [plane_input(i, sh, sw)] + ([special_plane(sh, sw)] if i == SPECIAL_CASE else [])
        for k, y in enumerate(inputs):
            want = expected_resample(oracle_lib, y, dw, dh, filt)
            for off in offsets(dw):
                what = "%s %s input %d +%d B [%s]" % (M.FILTER_NAMES[filt], case_id(c), k, off, cell(filt, c, off))
                got, intact = guarded_resample(srcnn, y, dw, dh, filt, off)
                assert intact, what + ": wrote outside its destination"
                same_values(got, want, what)


def test_plane_resample_tall_two_pass_vs_oracle(srcnn, oracle_lib):
    for filt in M.FILTERS:
        for i, c in enumerate(TALL_CASES):
            sh, sw, dh, dw = c
            assert cell(filt, c) in ("h-first", "v-first", "rows-only") and max(dh, sh) > 65535
            y = plane_input(i, sh, sw)
            got, intact = guarded_resample(srcnn, y, dw, dh, filt, 0)
            what = "%s %s [%s]" % (M.FILTER_NAMES[filt], case_id(c), cell(filt, c))
            assert intact, what
            assert_bit_equal(got, oracle_lib.resample(y, dw, dh, filt), what)


@pytest.mark.parametrize("filt", M.FILTERS, ids=M.FILTER_NAMES)
def test_y_path_every_cell_vs_oracle(srcnn, oracle_lib, filt):
    for i, c in enumerate(PLANE_CASES):
        sh, sw, dh, dw = c
        if (sw, sh) == (dw, dh):
            continue        # the identity-size Y path is pinned by test_identity_size_deviation_is_pinned
        inputs = [plane_input(i, sh, sw)] + ([special_plane(sh, sw)] if i == SPECIAL_CASE else [])
        for k, y in enumerate(inputs):
            what = "%s %s input %d [%s]" % (M.FILTER_NAMES[filt], case_id(c), k, cell(filt, c))
            same_values(srcnn.y_path(y, dw, dh, filt), oracle_lib.y_path(y, dw, dh, filt), what)


def test_y_path_tall_two_pass_vs_oracle(srcnn, oracle_lib):
    sh, sw, dh, dw = TALL_CASES[0]
    y = plane_input(0, sh, sw)
    assert_bit_equal(srcnn.y_path(y, dw, dh, 2), oracle_lib.y_path(y, dw, dh, 2), "y_path " + case_id(TALL_CASES[0]))


_CHILD = r"""
import hashlib, json, sys
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + "/tests")
import libsrcnn_amd as S
import test_gpu_resample_dispatch as T
S.init(0)
out = {}
for filt in range(5):
    for i, c in enumerate(T.PLANE_CASES + T.TALL_CASES):
        sh, sw, dh, dw = c
        y = T.plane_input(i, sh, sw) if i < len(T.PLANE_CASES) else T.plane_input(i - len(T.PLANE_CASES), sh, sw)
        for off in T.offsets(dw):
            got, intact = T.guarded_resample(S, y, dw, dh, filt, off)
            out["%d/%d/%d" % (filt, i, off)] = [hashlib.sha256(got.tobytes()).hexdigest(), intact]
print("DIGESTS " + json.dumps(out))
"""


def run_child(env):
    r = subprocess.run([sys.executable, "-c", _CHILD, ROOT], env=dict(os.environ, **env), capture_output=True, text=True,
                       timeout=600)
    line = [l for l in r.stdout.splitlines() if l.startswith("DIGESTS ")]
    assert r.returncode == 0 and line, r.stdout[-400:] + r.stderr[-800:]
    return json.loads(line[0][8:])


@pytest.mark.parametrize("env_name", ["rs_dma0", "2pass"])
def test_plane_resample_switch_variants_vs_oracle(srcnn, oracle_lib, env_name):
    env, settings = M.ENVS[env_name]
    got = run_child(env)
    bad = []
    for filt in M.FILTERS:
        for i, c in enumerate(PLANE_CASES + TALL_CASES):
            sh, sw, dh, dw = c
            y = plane_input(i, sh, sw) if i < len(PLANE_CASES) else plane_input(i - len(PLANE_CASES), sh, sw)
            want = hashlib.sha256(expected_resample(oracle_lib, y, dw, dh, filt).tobytes()).hexdigest()
            for off in offsets(dw):
                digest, intact = got["%d/%d/%d" % (filt, i, off)]
                if digest != want or not intact:
                    bad.append("%s %s +%d B [%s]%s" % (M.FILTER_NAMES[filt], case_id(c), off, cell(filt, c, off, settings),
                                                         "" if intact else " (wrote outside)"))
    assert not bad, "%s: %d cases differ from the oracle: %s" % (env, len(bad), bad)
