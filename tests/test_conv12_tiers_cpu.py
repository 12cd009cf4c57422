"""CPU checks of the premises of k_conv12_mfma's nested zero tiers (the GPU side is tests/test_gpu_conv12_tiers.py): the tier
masks in the kernel source are a nested chain that starts at M_DEAD and are the ones tools/conv12_zero_segments.py printed; the
exactness argument's two facts about the weight table hold (no layer-2 bias is +-0, every layer-2 weight is finite); the three
pinned kernel fingerprints are the recorded ones, k_conv12_mfma's covers the tiers and run_conv12, k_conv3's covers C3_SPARSE and
launch_conv3, and the committed traffic record was measured on this text.  k_conv3's pin moved once, on purpose, when
the written-out copy of its
skip instance was folded into the template instruction for instruction (profiles/conv3_fold_isa.txt)."""
import json
import os
import re

import numpy as np

from libsrcnn_amd import build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PINNED = {
    "k_conv12_mfma": "94857eddbb2a8296a76ec6a18246f0288de6590de38bfd8a5f647015ee1ee39a",
    "k_conv3": "4d4511830f635b4324fe30ab3cc2c5f8861b2dac0d85fb0c7ac48db46b7fa46d",
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


def _sha_of_modified_copy(monkeypatch, tmp_path, file, old, new, name="k_conv12_mfma"):
    """kernel_source_sha(name) of a copy of the sources in which `old` (which occurs once) reads `new`"""
    for f in ("srcnn_kernels.hip", "srcnn_capi.cpp"):
        text = open(os.path.join(build.CSRC, f)).read()
        if f == file:
            assert text.count(old) == 1, old
            text = text.replace(old, new)
        (tmp_path / f).write_text(text)
    monkeypatch.setattr(build, "CSRC", str(tmp_path))
    return build.kernel_source_sha(name)


def test_one_fingerprint_covers_the_tiers_and_run_conv12(monkeypatch, tmp_path):
    """The nested-tiers instance is k_conv12_mfma's: there is no second kernel and no second fingerprint, and the one
    fingerprint moves with the tier masks and with the host function that picks the instance."""
    assert build.kernel_source_sha("k_conv12_tiers") is None
    sha = build.kernel_source_sha("k_conv12_mfma")
    _dead, tiers = kernel_tiers()
    t2 = "0x%016xull" % tiers[-1]
    assert _sha_of_modified_copy(monkeypatch, tmp_path, "srcnn_kernels.hip", t2, "0x%016xull" % (tiers[-1] | 1)) not in (None, sha)
    monkeypatch.undo()
    assert _sha_of_modified_copy(monkeypatch, tmp_path, "srcnn_capi.cpp", "const bool tiers = c.relax() == 0 &&", "const bool tiers = c.relax() != 0 &&") not in (None, sha)
    monkeypatch.undo()
    assert build.kernel_source_sha("k_conv12_mfma") == sha


def test_one_fingerprint_covers_the_skip_instance_and_launch_conv3(monkeypatch, tmp_path):
    """The instance that skips all-zero channel windows is k_conv3's: there is no second kernel and no second fingerprint, and
    the one fingerprint moves with the candidate set and with the launcher that picks the instance."""
    assert build.kernel_source_sha("k_conv3_sparse") is None
    sha = build.kernel_source_sha("k_conv3")
    assert _sha_of_modified_copy(monkeypatch, tmp_path, "srcnn_kernels.hip", "C3_SPARSE = 0x24002002u;", "C3_SPARSE = 0x24002003u;",
                                 "k_conv3") not in (None, sha)
    monkeypatch.undo()
    assert _sha_of_modified_copy(monkeypatch, tmp_path, "srcnn_kernels.hip", "if (settings().conv3_skip) CONV3_GO(",
                                 "if (!settings().conv3_skip) CONV3_GO(", "k_conv3") not in (None, sha)
    monkeypatch.undo()
    assert build.kernel_source_sha("k_conv3") == sha


def test_traffic_record_carries_the_trees_fingerprints():
    """bench.py quotes roofline.traffic and whole_path only from a record taken on this text: profiles/r06_pmc_conv12.json must
    carry the tree's fingerprints, at top level (k_conv12_mfma) and for every kernel of `path`."""
    rec = json.load(open(os.path.join(ROOT, "profiles", "r06_pmc_conv12.json")))
    assert rec["kernel"] == "k_conv12_mfma" and rec["kernel_source_sha256"] == build.kernel_source_sha("k_conv12_mfma")
    assert set(rec["path"]) == {"k_conv12_mfma", "k_conv3", "k_rs2d_dma"}
    for name, entry in rec["path"].items():
        assert entry["kernel_source_sha256"] == build.kernel_source_sha(name), name
