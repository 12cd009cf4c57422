"""CPU checks of k_conv12_tiers' premises (the GPU side is tests/test_gpu_conv12_tiers.py): the tier masks in the kernel source
are a nested chain that starts at M_DEAD and are the ones tools/conv12_zero_segments.py printed; the exactness argument's two
facts about the weight table hold (no layer-2 bias is +-0, every layer-2 weight is finite); the three pinned kernel
fingerprints did not move; the new kernel has a fingerprint of its own."""
import os
import re

import numpy as np

from libsrcnn_amd import build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PINNED = {
    "k_conv12_mfma": "e6fcc3897416918d97488400ce07d743bd3884e49cc6b4b95059ed52ca0d14db",
    "k_conv3": "8f0b7e652c0cb756f84cfcb4c4c087ecf194afc30c362529bc70a23bf8764bd9",
    "k_rs2d_dma": "adef7f27470d21d8aa7396a314ed8a758b2707fa87b705cbb289ae66fd085030",
}


def kernel_tiers():
    """[T1, T2, ...] as 64-bit masks, from the MT_TIER initialiser of srcnn_kernels.hip (M_DEAD resolved)."""
    src = open(os.path.join(ROOT, "libsrcnn_amd", "csrc", "srcnn_kernels.hip")).read()
    dead = int(re.search(r"constexpr unsigned long long M_DEAD = (0x[0-9a-fA-F]+)ull;", src).group(1), 16)
    n = int(re.search(r"constexpr int MT_TIERS = (\d+);", src).group(1))
    m = re.search(r"constexpr unsigned long long MT_TIER\[MT_TIERS\] = \{(.*?)\n\};", src, re.S)
    assert m, "MT_TIER not found"
    body = re.sub(r"//[^\n]*", "", m.group(1))
    tiers = [dead if t.strip() == "M_DEAD" else int(t.strip().rstrip("ul"), 16) for t in body.split(",") if t.strip()]
    assert len(tiers) == n, (tiers, n)
    return dead, tiers


def test_tier_masks_are_nested_and_start_at_m_dead():
    dead, tiers = kernel_tiers()
    assert tiers[0] == dead
    assert 1 <= len(tiers) <= 3
    for below, above in zip(tiers, tiers[1:]):
        assert above & below == below and above != below, (hex(below), hex(above))
        for blk in range(2):
            lo, hi = (below >> 32 * blk) & 0xffffffff, (above >> 32 * blk) & 0xffffffff
            assert hi & lo == lo, "nested per block"
    for t in tiers:                                   # two pairs per block are fetched ahead
        for blk in range(2):
            assert 32 - bin((t >> 32 * blk) & 0xffffffff).count("1") >= 4
        assert t & dead == dead


def test_tier_masks_are_the_tools_choice():
    """profiles/conv12_zero_segments.txt is tools/conv12_zero_segments.py's output; the kernel carries the sets it prints.  Where
    the tool keeps fewer tiers than it has lines for, it repeats the last mask."""
    _dead, tiers = kernel_tiers()
    txt = open(os.path.join(ROOT, "profiles", "conv12_zero_segments.txt")).read()
    printed = [int(re.search(r"^MT_TIER%d = (0x[0-9a-f]{16})" % i, txt, re.M).group(1), 16) for i in (1, 2, 3)]
    chain = [printed[0]] + [p for q, p in zip(printed, printed[1:]) if p != q]
    assert tiers == chain, ([hex(t) for t in tiers], [hex(p) for p in chain])


def test_no_layer2_bias_is_zero_and_layer2_weights_are_finite(golden):
    """Skipping a channel whose activations are +-0 can change only the SIGN of a zero accumulator, which the bias add erases
    unless the bias is +-0; and 0 x w is +-0 only for finite w."""
    w = golden.weights                               # order b1, W1, b2, W2, b3, W3
    o = 64 + 64 * 81
    b2, w2 = w[o:o + 32], w[o + 32:o + 32 + 32 * 64]
    assert np.all(np.abs(b2) > 0)
    assert np.all(np.isfinite(w2)) and np.all(np.isfinite(b2))


def test_pinned_fingerprints_are_unchanged():
    for name, sha in PINNED.items():
        assert build.kernel_source_sha(name) == sha, name


def test_new_kernel_has_its_own_fingerprint():
    sha = build.kernel_source_sha("k_conv12_tiers")
    assert sha is not None and re.fullmatch(r"[0-9a-f]{64}", sha)
    others = [build.kernel_source_sha(n) for n in ("k_conv12_mfma", "k_conv3", "k_conv3_sparse", "k_rs2d_dma")]
    assert sha not in others
