"""The nested-tiers instance of k_conv12_mfma, the production strict layer-1+2 kernel, chooses per 32-channel block and 32-pixel
segment between the full layer-2 body and one body per zero tier (MT_TIER in srcnn_kernels.hip: T1 = M_DEAD, T2 = T1 +
often-zero channels).  Whatever body a segment takes, the 32 layer-2 planes must be the oracle's conv2(conv1(.)) bit for bit; so
must those of the instance without the tiers, which SRCNN_CONV12_TIERS=0 runs with the M_DEAD body and SRCNN_CONV12_PRUNE=0 with
the full body only.  All three go through the
stage-level layers-1+2 call (srcnn_conv12_f32_dev) on the same upscaled-Y planes.

The planes are built so that every body of every block is taken, which is checked on the CPU from the oracle's layer-1
planes (whole 32-pixel segments only: what the kernel decides for a segment the right edge cuts depends on pixels the oracle
does not compute, and either decision is exact): every (block, body) must occur in at least MIN_SEGMENTS segments over the
input set.  That is a condition on the inputs; if it fails the test fails.  The tolerance is 0: bit patterns are compared,
except that where the oracle has a NaN the kernel must have a NaN (payloads are the adder's, not the network's).
"""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from libsrcnn_amd import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(48, 78), (70, 130), (1, 33), (33, 1)]        # (h, w) of the upscaled-Y plane
SEED = synth.SEED0 + 1201
MIN_SEGMENTS = 8
FLAT = np.float32(96.0)


def kernel_tiers():
    import test_conv12_tiers_cpu
    return test_conv12_tiers_cpu.kernel_tiers()[1]


def planes(h, w):
    """[(name, plane)] for one shape.  `mix` puts a constant region, a smooth crop and a noise crop side by side with one
    seam on a segment boundary (column 32) and one inside a segment (column 45, and column 77 / 109 where the plane is that
    wide); rows change regions at h / 2, inside a 16-row tile."""
    big = (max(h + 7, 80), max(w + 11, 160))        # room for the crops below (the shapes of this file: 80 x 160, as ever)
    smooth = synth.plane(big[0], big[1], SEED, "smooth")[7:7 + h, 11:11 + w].copy()
    noise = synth.plane(big[0], big[1], SEED + 1, "noise")[3:3 + h, 5:5 + w].copy()
    flat = np.full((h, w), FLAT, np.float32)
    mix = flat.copy()
    hh = (h + 1) // 2
    mix[:hh, 32:] = smooth[:hh, 32:]                 # seam on a segment boundary
    mix[hh:, :45] = noise[hh:, :45]                  # seam inside segment 1
    mix[hh:, 77:] = smooth[hh:, 77:]                 # ... and inside segment 2
    mix[:hh, 109:] = noise[:hh, 109:]                # ... and inside segment 3
    special = flat.copy()
    special[h // 2:, :] = smooth[h // 2:, :]
    for i, v in enumerate((np.nan, np.inf, -np.inf, 1e-40, -0.0, -1e-40, 3e30, -3e30)):
        # spread over rows and columns so that each value sits in the 9x9 window of pixels of a whole segment that would
        # take a tier without it
        y, x = (5 * i + 2) % h, (13 * i + 6) % w
        special[y, x] = np.float32(v)
    # the smooth crop at a half and a quarter of its contrast about the flat level: T1 and T2 segments mixed by the content itself
    gentle = [("smooth / %d" % d, FLAT + (smooth - np.float32(smooth.mean())) * np.float32(1.0 / d)) for d in (2, 4)]
    return gentle + [("flat", flat), ("smooth", smooth), ("mix", mix), ("noise", noise), ("noise x1000", noise * np.float32(1000)),
            ("-smooth", -smooth), ("-noise", -noise), ("-mix", -mix), ("special", special)]


def cases():
    return [("%s %dx%d" % (name, w, h), p) for (h, w) in SHAPES for name, p in planes(h, w)]


def body_counts(c1, tiers):
    """c1: (64, h, w) oracle layer-1 planes.  counts[blk][body] over the whole segments: body = number of the largest tier
    whose members of the block are all +-0 on the segment's 32 pixels (0 = the full body).  -0 is zero; NaN, Inf and
    denormals are not."""
    _, h, w = c1.shape
    n = w // 32
    counts = np.zeros((2, len(tiers) + 1), np.int64)
    if n == 0:
        return counts
    z = (c1[:, :, :n * 32].view(np.uint32) & 0x7fffffff) == 0
    z = z.reshape(64, h, n, 32).all(axis=3)
    for blk in range(2):
        body = np.zeros((h, n), np.int64)
        for t, mask in enumerate(tiers):
            members = [f for f in range(32 * blk, 32 * blk + 32) if (mask >> f) & 1]
            body[z[members].all(axis=0)] = t + 1           # nested: a larger tier all zero implies the smaller ones
        for b in range(len(tiers) + 1):
            counts[blk, b] += int((body == b).sum())
    return counts


@pytest.fixture(scope="module")
def reference(oracle_lib):
    """{name: (plane, oracle conv2(conv1(plane)))} and the body counts over the whole set, computed once."""
    tiers = kernel_tiers()
    ref = {}
    total = np.zeros((2, len(tiers) + 1), np.int64)
    for name, p in cases():
        c1 = oracle_lib.conv1(p)
        total += body_counts(c1, tiers)
        want = oracle_lib.conv2(c1)
        want.setflags(write=False)
        ref[name] = (p, want)
    return ref, total


def check(got, want, what):
    got = np.ascontiguousarray(got, np.float32)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan), what + ": NaN positions differ"
    bad = (got.view(np.uint32) != want.view(np.uint32)) & ~nan
    assert not bad.any(), "%s: %d of %d elements differ, first at %s" % (what, int(bad.sum()), bad.size, tuple(np.argwhere(bad)[0]))


def test_inputs_take_every_body_of_every_block(reference):
    """CPU: the condition on the inputs.  Every body (full, T1, T2, ...) of both blocks in at least MIN_SEGMENTS segments."""
    _ref, total = reference
    print("segments by body [full, T1, T2, ...]: block 0 %s, block 1 %s" % (total[0].tolist(), total[1].tolist()))
    assert (total >= MIN_SEGMENTS).all(), total.tolist()


@pytest.mark.gpu
def test_tiers_kernel_matches_the_oracle(srcnn, reference):
    """The library as loaded (SRCNN_CONV12_TIERS default 1 -> the nested-tiers instance; under another setting, what that setting runs)."""
    ref, total = reference
    assert (total >= MIN_SEGMENTS).all(), total.tolist()
    for name, (p, want) in ref.items():
        check(srcnn.conv12(p), want, name)


_CHILD = """
import sys
sys.path.insert(0, %(root)r)
sys.path.insert(0, %(tests)r)
import numpy as np, libsrcnn_amd as S
import test_gpu_conv12_tiers as T
S.init(0)
for kv in sys.argv[2:]:
    assert (kv + ' ') in S.debug_settings(), (kv, S.debug_settings())
np.savez(sys.argv[1], **{'p%%d' %% i: S.conv12(p) for i, (_name, p) in enumerate(T.cases())})
print('DONE')
"""


@pytest.mark.gpu
@pytest.mark.parametrize("switch", ["SRCNN_CONV12_TIERS=1", "SRCNN_CONV12_TIERS=0", "SRCNN_CONV12_PRUNE=0"])
def test_switches_match_the_oracle(reference, tmp_path, switch):
    """Each switch in a fresh process (the switches are read when the library is loaded): the nested-tiers instance of
    k_conv12_mfma, the instance without the tiers with its M_DEAD body (TIERS=0) and with the full body only (PRUNE=0), all on the
    same planes."""
    ref, _total = reference
    out = str(tmp_path / "planes.npz")
    code = _CHILD % {"root": ROOT, "tests": os.path.join(ROOT, "tests")}
    k, v = switch.split("=")
    r = subprocess.run([sys.executable, "-c", code, out, switch], env=dict(os.environ, **{k: v}), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "DONE" in r.stdout, r.stdout + r.stderr
    got = np.load(out)
    for i, (name, (_p, want)) in enumerate(ref.items()):
        check(got["p%d" % i], want, "%s, %s" % (switch, name))

