"""The production strict layer-3 kernel (k_conv3<true, false, false, true, SKIP = true>) lets a wave skip a layer-2 channel of
C3_SPARSE (in srcnn_kernels.hip) whose activations it has just read as all +-0 over its 68 x 8 window; SRCNN_CONV3_SKIP=0 runs
the instance with SKIP = false, which never skips.  The
result must stay the oracle's bit for bit whether a wave skips or not, so the planes below are built -- through the
stage-level conv3 call on caller-provided planes -- to put every candidate channel on both sides of that decision for waves
in the interior, on tile seams, in the ragged right / bottom tiles and at the clamped image border.

Geometry (srcnn_kernels.hip): 64 x 16 tiles, four waves of 64 columns x 4 rows each; a wave reads its rectangle plus a
2-sample halo, clamped to the image.
"""
import hashlib
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from conftest import assert_bit_equal
from libsrcnn_amd import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
C3_SPARSE = 0x24002002          # duplicate of the kernel's literal: layer-2 channels 1, 13, 26, 29 (checked against the source below)
CANDIDATES = [m for m in range(32) if (C3_SPARSE >> m) & 1]
SHAPES = [(20, 130), (9, 70)]   # (h, w): three tiles wide and two high, ragged right and bottom; two tiles wide, one high
SEED = 3107
# One sample of this size moves a pre-clamp sum (within about +-200 for these planes) by at least 1000 through the smallest
# nonzero layer-3 weight of a candidate (1e-4), so with both signs tried a missed sample cannot hide behind the [0, 255] clamp.
SAMPLE = np.float32(1e7)


def noise_planes(h, w, zero=CANDIDATES, zero_value=0.0):
    """32 planes of seeded noise in [0, 300], the channels of `zero` filled with zero_value (+0.0 or -0.0)."""
    rng = np.random.default_rng(SEED + 1000 * h + w)
    c2 = rng.uniform(0.0, 300.0, (32, h, w)).astype(np.float32)
    for m in zero:
        c2[m] = np.float32(zero_value)
    return c2


def wave_windows(h, w):
    """[(body rows, body cols, window rows, window cols)] of every wave with a pixel inside the image; windows clamped, as
    half-open ranges."""
    out = []
    for y0 in range(0, h, 4):
        for x0 in range(0, w, 64):
            out.append(((y0, min(y0 + 4, h)), (x0, min(x0 + 64, w)),
                        (max(y0 - 2, 0), min(y0 + 6, h)), (max(x0 - 2, 0), min(x0 + 66, w))))
    return out


def halo_positions(h, w):
    """Every image position that is a corner, or the middle of the first / last column or row, of some wave's UNCLAMPED 68 x 8
    window, clamped into the image as the kernel's staging clamps it: window corners, columns 0 and 67, rows 0 and 7; among
    them positions across a tile seam (rows 14, 17, 21 -> 19; columns 62, 65, 126, 129) and on the clamped border."""
    pos = set()
    for y0 in range(0, h, 4):
        for x0 in range(0, w, 64):
            rows = (y0 - 2, y0 + 1, y0 + 5)
            cols = (x0 - 2, x0 + 31, x0 + 65)
            for r in rows:
                for c in cols:
                    if (r, c) != (rows[1], cols[1]):
                        pos.add((min(max(r, 0), h - 1), min(max(c, 0), w - 1)))
    return sorted(pos)


@pytest.fixture(scope="module")
def base(oracle_lib):
    """Per shape: the planes with every candidate all +0 and the oracle's result for them (computed once, never modified)."""
    out = {}
    for (h, w) in SHAPES:
        c2 = noise_planes(h, w)
        want = oracle_lib.conv3(c2)
        c2.setflags(write=False)
        want.setflags(write=False)
        out[(h, w)] = (c2, want)
    return out


def test_mask_matches_the_source_and_the_committed_count_and_layer3_weights_are_finite(golden):
    """CPU: the literal above is the kernel's; it is the set tools/conv3_zero_windows.py found (profiles/conv3_zero_windows.txt:
    every channel all zero on at least 25 % of the wave windows of some input); every layer-3 weight is finite, which the
    kernel's exactness argument needs ((+-0) x a finite weight = +-0)."""
    src = open(os.path.join(ROOT, "libsrcnn_amd", "csrc", "srcnn_kernels.hip")).read()
    m = re.search(r"constexpr unsigned C3_SPARSE = (0x[0-9a-fA-F]+)u;", src)
    assert m, "C3_SPARSE not found"
    assert int(m.group(1), 16) == C3_SPARSE
    txt = open(os.path.join(ROOT, "profiles", "conv3_zero_windows.txt")).read()
    t = re.search(r"^C3_SPARSE = (0x[0-9a-fA-F]+)$", txt, re.M)
    assert t, "no C3_SPARSE line in profiles/conv3_zero_windows.txt"
    assert int(t.group(1), 16) == C3_SPARSE
    assert CANDIDATES == [1, 13, 26, 29]
    w3 = golden.weights[-800:]                     # blob order b1, W1, b2, W2, b3, W3: the last 32 x 25 values
    assert golden.weights.size == 8129 and np.all(np.isfinite(w3))
    assert np.isfinite(golden.weights[-801])       # b3


def test_both_layer3_kernels_are_in_both_builds():
    """CPU: the skipping instance of k_conv3 and the one SRCNN_CONV3_SKIP=0 runs are compiled into the full and the strict-only
    library; the written-out copy of the former (see the last line) is in neither."""
    import libsrcnn_amd as S
    from libsrcnn_amd import build
    strict, _ = build.build_strict_only(verbose=False)
    for path in (S.LIB_PATH, strict):
        blob = open(path, "rb").read()
        assert b"k_conv3ILb1ELb0ELb0ELb1ELb1E" in blob and b"k_conv3ILb1ELb0ELb0ELb1ELb0E" in blob, path
        assert b"k_conv3_sparse" not in blob, path


@pytest.mark.gpu
@pytest.mark.parametrize("zero_value", [0.0, -0.0], ids=["plus0", "minus0"])
def test_all_candidates_zero(srcnn, oracle_lib, base, zero_value):
    """Every candidate channel all +0, then all -0: every wave skips all four."""
    for (h, w) in SHAPES:
        c2 = noise_planes(h, w, zero_value=zero_value)
        assert np.all(c2[CANDIDATES] == 0) and np.all(np.signbit(c2[CANDIDATES]) == np.signbit(np.float32(zero_value)))
        want = oracle_lib.conv3(c2)
        assert_bit_equal(want, base[(h, w)][1], "the oracle itself: -0 channels add nothing")
        assert_bit_equal(srcnn.conv3(c2), want, "candidates all %r, %dx%d" % (zero_value, w, h))


@pytest.mark.gpu
@pytest.mark.parametrize("m", CANDIDATES)
def test_one_sample_where_a_wave_sees_it_only_through_its_halo(srcnn, oracle_lib, base, golden, m):
    """One nonzero sample in candidate m (the others all zero), in turn at every corner and edge middle of every wave's
    window: each wave that sees the sample -- its owner and up to three neighbours that see it in their halo alone -- must run
    the channel.  Both signs, so that the [0, 255] clamp cannot hide a missed sample; for channels whose 25 weights are all
    nonzero the oracle's own results show that every such wave's output depends on the sample."""
    w3m = golden.weights[-800:].reshape(32, 25)[m]
    all_taps = bool(np.all(w3m != 0))              # channel 26 has one nonzero tap: a finite halo sample adds +-0 there anyway
    for (h, w) in SHAPES:
        c2_0, want_0 = base[(h, w)]
        waves = wave_windows(h, w)
        for (r, c) in halo_positions(h, w):
            moved = np.zeros((h, w), bool)
            for v in (SAMPLE, -SAMPLE):
                c2 = c2_0.copy()
                c2[m, r, c] = v
                want = oracle_lib.conv3(c2)
                moved |= want.view(np.uint32) != want_0.view(np.uint32)
                assert_bit_equal(srcnn.conv3(c2), want, "channel %d, sample %g at (%d, %d), %dx%d" % (m, v, r, c, w, h))
            if all_taps:
                for (br, bc, wr, wc) in waves:
                    if wr[0] <= r < wr[1] and wc[0] <= c < wc[1]:
                        assert moved[br[0]:br[1], bc[0]:bc[1]].any(), ("insensitive case", m, r, c, br, bc)


@pytest.mark.gpu
@pytest.mark.parametrize("value", [np.float32(1e-42), np.float32(np.nan), np.float32(np.inf)], ids=["denormal", "nan", "inf"])
def test_denormal_nan_inf_are_not_zero(srcnn, oracle_lib, base, value):
    """A denormal, a NaN, a +Inf in a candidate channel: magnitude bits are set, so no wave that sees it may skip.  In a
    window corner, so that one wave sees it through its halo alone; the NaN positions and all other bits are the oracle's."""
    for (h, w) in SHAPES:
        c2_0, _ = base[(h, w)]
        for m in CANDIDATES:
            for (r, c) in ((2, 62), (min(9, h - 1), 65), (0, 0), (h - 1, w - 1)):
                c2 = c2_0.copy()
                c2[m, r, c] = value
                want = oracle_lib.conv3(c2)
                got = srcnn.conv3(c2)
                assert np.array_equal(np.isnan(got), np.isnan(want)), (m, r, c)
                ok = ~np.isnan(want)
                assert np.array_equal(got.view(np.uint32)[ok], want.view(np.uint32)[ok]), (m, r, c)


@pytest.mark.gpu
def test_inf_at_every_halo_position_of_channels_with_zero_taps(srcnn, oracle_lib, golden):
    """Channel 26 has one nonzero tap (the centre), so a finite sample in a wave's halo adds +-0 there whether the wave runs the
    channel or not, and the one-sample test above cannot see a wrong skip.  +Inf can: (+-0) x Inf = NaN, which the final clamp
    turns into 0.  So: one +Inf at every halo position, on planes whose oracle result is nowhere 0 (the noise of the channels
    with a negative weight sum is scaled down to [0, 15], that of the others moved to [150, 300]: still inside [0, 300]); the oracle's own results show that every wave
    that sees the sample has an output pixel that depends on it."""
    w3 = golden.weights[-800:].reshape(32, 25)
    sparse_taps = [m for m in CANDIDATES if np.any(w3[m] == 0)]
    assert sparse_taps == [26]
    for (h, w) in SHAPES:
        c2_0 = noise_planes(h, w)
        neg = w3.sum(axis=1) <= 0
        c2_0[neg] *= np.float32(0.05)
        c2_0[~neg] = np.float32(150.0) + c2_0[~neg] * np.float32(0.5)
        c2_0[CANDIDATES] = 0
        want_0 = oracle_lib.conv3(c2_0)
        assert want_0.min() > 0, "the base result must be nowhere 0 for a NaN (clamped to 0) to show"
        waves = wave_windows(h, w)
        for m in sparse_taps:
            for (r, c) in halo_positions(h, w):
                c2 = c2_0.copy()
                c2[m, r, c] = np.float32(np.inf)
                want = oracle_lib.conv3(c2)
                assert not np.isnan(want).any()
                assert_bit_equal(srcnn.conv3(c2), want, "channel %d, +Inf at (%d, %d), %dx%d" % (m, r, c, w, h))
                moved = want.view(np.uint32) != want_0.view(np.uint32)
                for (br, bc, wr, wc) in waves:
                    if wr[0] <= r < wr[1] and wc[0] <= c < wc[1]:
                        assert moved[br[0]:br[1], bc[0]:bc[1]].any(), ("insensitive case", m, r, c, br, bc)


@pytest.mark.gpu
def test_non_candidate_channel_all_zero(srcnn, oracle_lib):
    """A channel outside the set all zero (never tested, never skipped), with the candidates all zero (skipped) and with
    the candidates noise (tested, not skipped): the oracle's result each time."""
    for (h, w) in SHAPES:
        for zero in ([0, 7, 31] + CANDIDATES, [0, 7, 31]):
            c2 = noise_planes(h, w, zero=zero)
            assert_bit_equal(srcnn.conv3(c2), oracle_lib.conv3(c2), "channels %s zero, %dx%d" % (zero, w, h))


_CHILD = """
import sys, hashlib
sys.path.insert(0, %(root)r)
sys.path.insert(0, %(tests)r)
import numpy as np, libsrcnn_amd as S
from libsrcnn_amd import synth
import test_gpu_conv3_skip as T
S.init(0)
assert ('SRCNN_CONV3_SKIP=%%s ' %% sys.argv[1]) in S.debug_settings(), S.debug_settings()
sha = lambda a: hashlib.sha256(np.ascontiguousarray(a, np.float32).tobytes()).hexdigest()
for (h, w) in T.SHAPES:
    print('SHA conv3 %%dx%%d' %% (w, h), sha(S.conv3(T.noise_planes(h, w))))
print('SHA y_path', sha(S.y_upscale2x(synth.plane(272, 480, synth.SEED0, 'smooth'))))
"""


@pytest.mark.gpu
def test_switch_off_and_on_give_the_oracles_bytes(oracle_lib, base):
    """SRCNN_CONV3_SKIP=0 and =1, each in a fresh process (the switches are read when the library is loaded): the planes with
    every candidate all +0 through the conv3 stage call, and a 272x480 `smooth` frame (where the kernel meets skippable
    windows of every candidate, profiles/conv3_zero_windows.txt) through y_upscale2x -- all equal to the oracle's."""
    sha = lambda a: hashlib.sha256(np.ascontiguousarray(a, np.float32).tobytes()).hexdigest()
    want = {"conv3 %dx%d" % (w, h): sha(base[(h, w)][1]) for (h, w) in SHAPES}
    want["y_path"] = sha(oracle_lib.y_path(synth.plane(272, 480, synth.SEED0, "smooth")))
    code = _CHILD % {"root": ROOT, "tests": os.path.join(ROOT, "tests")}
    for skip in ("0", "1"):
        r = subprocess.run([sys.executable, "-c", code, skip], env=dict(os.environ, SRCNN_CONV3_SKIP=skip),
                           capture_output=True, text=True, timeout=300)
        got = dict(re.findall(r"^SHA (.+) ([0-9a-f]{64})$", r.stdout, re.M))
        assert r.returncode == 0 and got == want, (skip, r.stdout + r.stderr)
