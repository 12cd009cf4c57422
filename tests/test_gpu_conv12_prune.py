"""Strict layer 2 of k_conv12_mfma skips the near-dead layer-1 channels (M_DEAD in srcnn_kernels.hip) in every 32-pixel
segment where the kernel has just seen them all zero (SRCNN_CONV12_PRUNE, default 1).  The result must stay the oracle's bit
for bit whichever body a segment takes, so the planes below are chosen -- and checked on the CPU, from the oracle's layer-1
activations -- to drive segments through both bodies of both MFMA blocks.

The CPU classification looks at whole segments only (32 output pixels inside the image); what the kernel decides for a
segment the right edge cuts depends on pixels the oracle does not compute, and either decision is exact.
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
DEAD_SUM = 0.2                  # a channel is near-dead when its 81 absolute layer-1 weights sum to less than this
SEED = synth.SEED0 + 701        # the oracle confirms all four kinds of segment for this seed (asserted below)
SHAPE = (48, 78)                # -> 96 output rows x (4 whole segments + one cut by the right edge): a quarter-tile launch


def dead_set(weights):
    """{f : sum |w1[f][.]| < 0.2} from the weight blob (order b1, W1, b2, W2, b3, W3)."""
    w1 = weights[64:64 + 64 * 81].reshape(64, 81).astype(np.float64)
    return [f for f in range(64) if np.abs(w1[f]).sum() < DEAD_SUM]


def kernel_mask():
    src = open(os.path.join(ROOT, "libsrcnn_amd", "csrc", "srcnn_kernels.hip")).read()
    m = re.search(r"constexpr unsigned long long M_DEAD = (0x[0-9a-fA-F]+)ull;", src)
    assert m, "M_DEAD not found"
    return int(m.group(1), 16)


def segment_kinds(oracle_lib, y, dead):
    """Count the whole 32-pixel segments of the 2x plane by kind: index 2*(block 0 pruned) + (block 1 pruned), where a block
    is pruned iff every near-dead channel of it is +-0 on all 32 pixels.  Returns (counts[4], oracle output)."""
    out, _up, c1, _c2 = oracle_lib.y_path(y, taps=True)
    h, w = out.shape
    nseg = w // 32
    pruned = []
    for blk in range(2):
        members = [f for f in dead if f // 32 == blk]
        zero = (np.abs(c1[members]) == 0).all(axis=0)            # -0 counts as zero, NaN does not
        pruned.append(zero[:, :nseg * 32].reshape(h, nseg, 32).all(axis=2))
    kind = 2 * pruned[0].astype(int) + pruned[1].astype(int)
    return [int((kind == k).sum()) for k in range(4)], out


@pytest.fixture(scope="module")
def dead(golden):
    return dead_set(golden.weights)


@pytest.fixture(scope="module")
def noise_case(oracle_lib, dead):
    y = synth.plane(SHAPE[0], SHAPE[1], SEED, "noise")
    counts, want = segment_kinds(oracle_lib, y, dead)
    return y, counts, want


def test_mask_is_the_near_dead_set_and_no_layer2_bias_is_zero(golden):
    """CPU: the kernel's mask is {f : sum|w1[f]| < 0.2} of the golden weight blob (the next sum is far away, so the set is a
    property of the table), and no layer-2 bias is +-0 -- the bias add is what erases the sign of a zero accumulator."""
    w = golden.weights
    dead = dead_set(w)
    assert kernel_mask() == sum(1 << f for f in dead)
    assert dead == [18, 21, 22, 23, 24, 25, 26, 28, 30, 35, 41, 42, 43, 46, 50]
    sums = np.sort(np.abs(w[64:64 + 64 * 81].reshape(64, 81).astype(np.float64)).sum(axis=1))
    assert sums[len(dead) - 1] < 0.1 and sums[len(dead)] > 2.7
    b2 = w[64 + 64 * 81:64 + 64 * 81 + 32]
    assert np.all(np.abs(b2) > 0) and float(np.abs(b2).min()) >= 0.05
    assert np.all(np.isfinite(w))


@pytest.mark.gpu
def test_mixed_paths_noise(srcnn, noise_case):
    """Segments of all four kinds (block 0 pruned or not x block 1 pruned or not) in one launch."""
    y, counts, want = noise_case
    print("segment kinds [none, blk1, blk0, both]:", counts)
    assert all(c >= 1 for c in counts), counts
    assert_bit_equal(srcnn.y_upscale2x(y), want, "noise %dx%d" % SHAPE)


@pytest.mark.gpu
def test_all_hit_smooth(srcnn, oracle_lib, dead):
    y = synth.plane(SHAPE[0], SHAPE[1], SEED, "smooth")
    counts, want = segment_kinds(oracle_lib, y, dead)
    assert counts[:3] == [0, 0, 0] and counts[3] > 0, counts
    assert_bit_equal(srcnn.y_upscale2x(y), want, "smooth %dx%d" % SHAPE)


@pytest.mark.gpu
@pytest.mark.parametrize("scale", [1000.0, -1000.0])
def test_scaled_noise_and_all_miss(srcnn, oracle_lib, dead, noise_case, scale):
    """The noise plane x1000, and negated.  Every near-dead channel has a NEGATIVE weight sum (and a bias <= 0.002), so a
    larger positive input pushes it further below zero: x1000 does not wake the channels (the oracle counts about as many
    pruned segments as at x1; the plane stays a mixed case with 1000 times larger values).  The negated plane does: the
    oracle finds no pruned block in any segment, which is asserted -- the all-miss case."""
    y = noise_case[0] * np.float32(scale)
    counts, want = segment_kinds(oracle_lib, y, dead)
    print("scale %g: segment kinds [none, blk1, blk0, both]:" % scale, counts)
    if scale < 0:
        assert counts[0] > 0 and counts[1:] == [0, 0, 0], counts
    else:
        assert all(c >= 1 for c in counts), counts
    assert_bit_equal(srcnn.y_upscale2x(y), want, "noise x %g" % scale)


@pytest.mark.gpu
def test_odd_shape_quarter_tiles(srcnn, oracle_lib, dead):
    """Width no multiple of 64, height no multiple of 16, fewer tiles than resident workgroups."""
    y = synth.plane(37, 53, SEED + 10, "noise")
    counts, want = segment_kinds(oracle_lib, y, dead)
    assert counts[0] >= 1 and counts[3] >= 1, counts
    assert_bit_equal(srcnn.y_upscale2x(y), want, "noise 37x53")


@pytest.mark.gpu
def test_special_values(srcnn, oracle_lib):
    """NaN, +-Inf, -0.0, denormal and negative inputs: a NaN or an Inf in a near-dead channel is not zero and must take the
    full body; the values and the NaN positions are the oracle's."""
    y = synth.plane(24, 40, synth.SEED0 + 77, "noise")
    y[2, 3] = 1e-40
    y[5, 7] = -0.0
    y[7, 20:30] = -y[7, 20:30]
    y[9, 9] = 3e30
    y[9, 30] = -3e30
    y[15, 20] = np.inf
    y[18, 5] = -np.inf
    y[21, 33] = np.nan
    want = oracle_lib.y_path(y)
    got = srcnn.y_upscale2x(y)
    assert np.array_equal(np.isnan(got), np.isnan(want))
    ok = ~np.isnan(want)
    assert np.array_equal(got.view(np.uint32)[ok], want.view(np.uint32)[ok])


@pytest.mark.gpu
def test_switch_gives_identical_bytes(noise_case):
    """SRCNN_CONV12_PRUNE=0 and =1, with either SRCNN_CONV12_DMA setting, each in a fresh process (the switches are read
    when the library is loaded): byte-identical output on the mixed-path noise plane, equal to the oracle's."""
    y, _counts, want = noise_case
    code = ("import sys, hashlib; sys.path.insert(0, %r); import numpy as np, libsrcnn_amd as S; from libsrcnn_amd import synth;"
            "S.init(0); y = synth.plane(%d, %d, %d, 'noise');"
            "assert ('SRCNN_CONV12_PRUNE=%%s ' %% sys.argv[1]) in S.debug_settings(), S.debug_settings();"
            "print('SHA', hashlib.sha256(np.ascontiguousarray(S.y_upscale2x(y)).tobytes()).hexdigest())") % (ROOT, SHAPE[0], SHAPE[1], SEED)
    shas = {}
    for prune in ("0", "1"):
        for dma in ("0", "1"):
            r = subprocess.run([sys.executable, "-c", code, prune], env=dict(os.environ, SRCNN_CONV12_PRUNE=prune, SRCNN_CONV12_DMA=dma),
                               capture_output=True, text=True, timeout=300)
            m = re.search(r"SHA ([0-9a-f]{64})", r.stdout)
            assert r.returncode == 0 and m, r.stdout + r.stderr
            shas[(prune, dma)] = m.group(1)
    assert set(shas.values()) == {hashlib.sha256(np.ascontiguousarray(want, np.float32).tobytes()).hexdigest()}, shas
