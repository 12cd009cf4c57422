"""The colour shell of srcnn_process_u8 / ProcessSRCNN, byte for byte against the oracle, in every form it takes (GPU).

The shell is either fused into the resampler (Y from the interleaved source, chroma resampled and merged in the same kernel)
or the plane form (split, plane resamples, merge; down-scales, shapes rs2d refuses, SRCNN_SHELL_UNFUSED).  The test ids
carry what tests/resample_dispatch.py says the case takes.  Images: fewer than 1024 pixels, just above 1024 with
w*h % 4 != 0, and shapes for the wide-LDS-row and the refused cells; output widths of every residue mod 4.  Content has
saturated colours (pure primaries, black, white, alpha 0 and 255), so the u8 conversions clip at both ends and Y' leaves
[0, 255].  SRCNN_SHELL_UNFUSED=1 and SRCNN_RESAMPLE_2PASS=1 are read when the library loads: the whole matrix runs once
more in a subprocess for each, whose digests are compared with the oracle's here.
"""
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import resample_dispatch as M

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CANARY = 4096
MULS = (0.5, 0.75, 1.25, 1.5, 2.0, 2.5, 3.0, 5.0)
# (h, w): 667 px; 1073 px (% 4 == 1); 1280 px (% 4 == 0: the 4-pixel split / merge and the fused 16-byte stores for RGB);
# short wide images (wide LDS rows; chroma patches too large for the fused merge; x1.5 Mitchell / B-spline tables are not
# monotone); 2-5 sample axes (3- and 5-tap tables of the long filters); 1 wide
IMAGES = [(23, 29), (29, 37), (32, 40), (4, 160), (4, 150), (5, 161), (9, 160), (8, 150), (3, 2), (5, 4), (9, 1)]
LARGE_CASE = (584, 600, 4, 3, 2.5)    # (h, w, d, filter, multiply): output above 8 MB, the banded and pipelined path


def image(h, w, d, seed):
    """Saturated blocks (pure primaries, black, white) beside noise; alpha alternates 0 / 255 blocks and noise."""
    rng = np.random.default_rng(seed)
    img = rng.integers(0, 256, (h, w, d), dtype=np.uint8)
    palette = np.array([[255, 0, 0, 0], [0, 255, 0, 255], [0, 0, 255, 0], [0, 0, 0, 255], [255, 255, 255, 0],
                        [255, 255, 0, 255], [0, 255, 255, 0], [255, 0, 255, 255]], np.uint8)[:, :d]
    yy, xx = np.mgrid[0:h, 0:w]
    block = (yy // 3 + xx // 4) % len(palette)
    sat = (xx < (w + 1) // 2) | (yy % 7 < 2)
    img[sat] = palette[block[sat]]
    return img


def matrix():
    for (h, w) in IMAGES:
        for d in (3, 4):
            for filt in M.FILTERS:
                for mul in MULS:
                    dw, dh = M.out_size(w, h, mul)
                    # (the identity size is pinned by test_identity_size_deviation_is_pinned: the oracle half-copies there)
                    if dw and dh and (dw, dh) != (w, h):
                        yield h, w, d, filt, mul


def case_id(c):
    h, w, d, filt, mul = c
    shell, _ = M.shell_cells(filt, w, h, d, mul)
    return "%s-%dx%dx%d-%s-x%g" % (shell.replace(":", "-"), w, h, d, M.FILTER_NAMES[filt], mul)


CASES = list(matrix())


def run_process_u8(S, img, mul, filt, conv):
    """srcnn_process_u8 into host buffers with CANARY bytes of 0xA5 on either side; returns (rgb, conv|None)."""
    h, w, d = img.shape
    dw, dh = M.out_size(w, h, mul)
    out = np.full(dh * dw * d + 2 * CANARY, 0xA5, np.uint8)
    cv = np.full(dh * dw + 2 * CANARY, 0xA5, np.uint8)
    S.check(S.lib().srcnn_process_u8(img.ctypes.data, w, h, d, float(np.float32(mul)), filt, out.ctypes.data + CANARY,
                                     cv.ctypes.data + CANARY if conv else None))
    for buf in (out, cv):
        assert (buf[:CANARY] == 0xA5).all() and (buf[-CANARY:] == 0xA5).all(), "wrote outside the caller's buffers"
    if not conv:
        assert (cv == 0xA5).all()
    return out[CANARY:-CANARY].reshape(dh, dw, d), (cv[CANARY:-CANARY].reshape(dh, dw) if conv else None)


_WANT = {}      # case -> oracle digests (conv on, conv off): the switch variants compare with them


def digest(rgb, conv):
    return hashlib.sha256(rgb.tobytes() + (conv.tobytes() if conv is not None else b"")).hexdigest()


def oracle_case(oracle_lib, case, seed):
    h, w, d, filt, mul = case
    img = image(h, w, d, seed)
    want_rgb, want_conv = oracle_lib.process(img, mul, filt)
    _WANT[case] = (digest(want_rgb, want_conv), digest(want_rgb, None))
    return img, want_rgb, want_conv


def first_difference(got, want):
    bad = np.argwhere(got != want)
    i = tuple(bad[0])
    return "%d bytes differ, first at %s: got %d want %d" % (len(bad), i, got[i], want[i])


@pytest.mark.parametrize("case", CASES, ids=[case_id(c) for c in CASES])
def test_colour_shell_vs_oracle(srcnn, oracle_lib, case):
    S = srcnn
    h, w, d, filt, mul = case
    img, want_rgb, want_conv = oracle_case(oracle_lib, case, 1000 * h + w)
    for conv in (True, False):
        got_rgb, got_conv = run_process_u8(S, img, mul, filt, conv)
        assert np.array_equal(got_rgb, want_rgb), "srcnn_process_u8 conv=%d: rgb %s" % (conv, first_difference(got_rgb, want_rgb))
        if conv:
            assert np.array_equal(got_conv, want_conv), "srcnn_process_u8: conv " + first_difference(got_conv, want_conv)
    S.ConfigureFilterSRCNN(filt, False)
    for conv in (True, False):
        rc, out, cv = S.ProcessSRCNN(img, w, h, d, mul, want_conv=conv)
        assert rc == 0
        assert np.array_equal(out.reshape(want_rgb.shape), want_rgb), "ProcessSRCNN conv=%d: rgb" % conv
        assert (cv is None) if not conv else np.array_equal(cv.reshape(want_conv.shape), want_conv), "ProcessSRCNN conv"


def test_colour_shell_large_banded_vs_oracle(srcnn, oracle_lib):
    h, w, d, filt, mul = LARGE_CASE
    img, want_rgb, want_conv = oracle_case(oracle_lib, LARGE_CASE, 77)
    assert want_rgb.nbytes > (8 << 20)
    got_rgb, got_conv = run_process_u8(srcnn, img, mul, filt, True)
    assert np.array_equal(got_rgb, want_rgb), "rgb " + first_difference(got_rgb, want_rgb)
    assert np.array_equal(got_conv, want_conv), "conv " + first_difference(got_conv, want_conv)


_CHILD = r"""
import hashlib, json, sys
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + "/tests")
import libsrcnn_amd as S
import test_gpu_colour_shell as T
S.init(0)
out = {}
for k, (h, w, d, filt, mul) in enumerate(T.CASES + [T.LARGE_CASE]):
    img = T.image(h, w, d, 77 if k == len(T.CASES) else 1000 * h + w)
    for conv in (True, False):
        rgb, cv = T.run_process_u8(S, img, mul, filt, conv)
        out["%d/%d" % (k, conv)] = T.digest(rgb, cv)
print("DIGESTS " + json.dumps(out))
"""


@pytest.mark.parametrize("env_name", ["unfused", "2pass"])
def test_colour_shell_switch_variants_vs_oracle(srcnn, oracle_lib, env_name):
    env, settings = M.ENVS[env_name]
    r = subprocess.run([sys.executable, "-c", _CHILD, ROOT], env=dict(os.environ, **env), capture_output=True, text=True,
                       timeout=900)
    line = [l for l in r.stdout.splitlines() if l.startswith("DIGESTS ")]
    assert r.returncode == 0 and line, r.stdout[-400:] + r.stderr[-800:]
    got = json.loads(line[0][8:])
    bad = []
    for k, case in enumerate(CASES + [LARGE_CASE]):
        h, w, d, filt, mul = case
        if case not in _WANT:
            oracle_case(oracle_lib, case, 77 if k == len(CASES) else 1000 * h + w)
        for conv in (True, False):
            if got["%d/%d" % (k, conv)] != _WANT[case][0 if conv else 1]:
                shell, cells = M.shell_cells(filt, w, h, d, mul, conv, settings)
                bad.append("%dx%dx%d %s x%g conv=%d [%s %s]" % (w, h, d, M.FILTER_NAMES[filt], mul, conv, shell, sorted(cells)))
    assert not bad, "%s: %d cases differ from the oracle: %s" % (env, len(bad), bad[:20])
