#!/usr/bin/env python3
"""How often is a layer-1 channel all zero over one wave segment of the layer-1+2 kernel, and which channels are zero together?

k_conv12_mfma computes one image row x 32 columns per wave step (a segment) and hands the 64 layer-1 activations
of those 32 pixels to layer 2 one 32-channel MFMA block at a time.  Strict layer 2 may leave out every channel it has just
seen all +-0 over the segment.  The kernel decides once per block between a few fully unrolled bodies, so what it needs is
a short chain of NESTED channel sets per block, T1 = M_DEAD's members of the block, T1 < T2 < T3, each as large and as
often jointly zero as possible.  This tool counts, on the CPU and through the oracle, on the butterfly golden image and on
synth frames:

  * for every layer-1 channel, the share of segments on which it is +-0;
  * per block, the greedy chain from T1 (grow by the channel that keeps the joint-zero share highest) and the tiers taken from it.

Score of a set over the tier below: (channels it adds) x (share of segments on which all its members are zero) -- the expected
number of channels saved per segment.  The measure is the mean of the `smooth` share (mean of three seeds) and the butterfly
share.  T2 is the best-scoring set of the chain, T3 the best-scoring strict superset of T2 (scored over T2); a tier is kept only
if it scores at least 1.0, one channel per segment.  `noise` is listed for the record and takes no part in the choice.

    python tools/conv12_zero_segments.py > profiles/conv12_zero_segments.txt

No GPU is needed.  tests/test_conv12_tiers_cpu.py reads the `MT_TIER2` / `MT_TIER3` lines of the committed output.
"""
import os
import re
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import oracle                              # noqa: E402
from libsrcnn_amd import synth             # noqa: E402

SEG = 32
MIN_GAIN = 1.0


def m_dead():
    src = open(os.path.join(ROOT, "libsrcnn_amd", "csrc", "srcnn_kernels.hip")).read()
    return int(re.search(r"constexpr unsigned long long M_DEAD = (0x[0-9a-fA-F]+)ull;", src).group(1), 16)


def segment_zero(c1):
    """c1: (64, H, W) layer-1 activations -> bool (64, H * (W // 32)): channel f is +-0 on all 32 pixels of the segment.
    Whole segments only; NaN counts as not zero, -0 as zero."""
    _, h, w = c1.shape
    n = w // SEG
    z = np.abs(c1[:, :, :n * SEG]) == 0
    return z.reshape(64, h, n, SEG).all(axis=3).reshape(64, h * n)


def inputs():
    g = np.load(os.path.join(ROOT, "tests", "golden", "butterfly.npz"))
    f = g["rgb_in"].astype(np.float32)
    F = np.float32
    yield "butterfly", "butterfly 256x256 (luma of tests/golden/butterfly.npz)", (F(0.299) * f[..., 0]) + (F(0.587) * f[..., 1]) + (F(0.114) * f[..., 2])
    for kind in ("smooth", "noise"):
        for k in range(3):
            yield kind, "synth %s 480x270 seed SEED0+%d" % (kind, k), synth.plane(270, 480, synth.SEED0 + k, kind)


def fmt(s):
    return "{" + ", ".join(map(str, sorted(s))) + "}"


def main():
    orc = oracle.Oracle()
    dead = m_dead()
    zs = []                                     # (kind, name, zero[64, nseg])
    print("share of 32-pixel segments (one row x 32 columns of the 2x plane) on which a layer-1 channel is all +-0; oracle activations")
    for kind, name, y in inputs():
        _out, _up, c1, _c2 = orc.y_path(y, taps=True)
        z = segment_zero(c1)
        zs.append((kind, name, z))
        print("%s: %d segments" % (name, z.shape[1]))
        share = z.mean(axis=1)
        for b in range(2):
            print("  block %d: " % b + " ".join("%d:%.2f" % (f, share[f]) for f in range(32 * b, 32 * b + 32)))

    def joint(s, kind):
        """share of segments where every member of s is zero: one figure per input of that kind"""
        m = sorted(s)
        return [float(z[m].all(axis=0).mean()) for k, _n, z in zs if k == kind]

    def measure(s):
        return 0.5 * (float(np.mean(joint(s, "smooth"))) + joint(s, "butterfly")[0])

    masks = [dead, dead, dead]
    for b in range(2):
        t1 = {f for f in range(32 * b, 32 * b + 32) if (dead >> f) & 1}
        print("\nblock %d: T1 = M_DEAD's members %s, jointly zero: smooth %s, butterfly %.3f, noise %s" % (
            b, fmt(t1), "/".join("%.3f" % v for v in joint(t1, "smooth")), joint(t1, "butterfly")[0],
            "/".join("%.3f" % v for v in joint(t1, "noise"))))
        chain = [set(t1)]
        rest = set(range(32 * b, 32 * b + 32)) - t1
        print("  greedy chain (added channel, set size, joint share: mean | smooth x3 | butterfly | noise x3, score over T1):")
        while rest:
            f = max(sorted(rest), key=lambda c: measure(chain[-1] | {c}))
            if measure(chain[-1] | {f}) < 0.005:
                break
            rest.discard(f)
            chain.append(chain[-1] | {f})
            s = chain[-1]
            print("    +%-2d  %2d  %.3f | %s | %.3f | %s   %.2f" % (
                f, len(s), measure(s), " ".join("%.3f" % v for v in joint(s, "smooth")), joint(s, "butterfly")[0],
                " ".join("%.3f" % v for v in joint(s, "noise")), (len(s) - len(t1)) * measure(s)))
        tiers = [t1]
        for _ in range(2):
            below = tiers[-1]
            cands = [s for s in chain if len(s) > len(below)]
            if not cands:
                break
            best = max(cands, key=lambda s: (len(s) - len(below)) * measure(s))
            gain = (len(best) - len(below)) * measure(best)
            if gain < MIN_GAIN:
                print("  T%d: best candidate %s scores %.2f < %.1f over T%d: not kept" % (len(tiers) + 1, fmt(best - below), gain, MIN_GAIN, len(tiers)))
                break
            tiers.append(best)
            print("  T%d = T%d + %s  (%d channels; jointly zero: mean %.3f, smooth %s, butterfly %.3f, noise %s; score over T%d %.2f)" % (
                len(tiers), len(tiers) - 1, fmt(best - below), len(best), measure(best), "/".join("%.3f" % v for v in joint(best, "smooth")),
                joint(best, "butterfly")[0], "/".join("%.3f" % v for v in joint(best, "noise")), len(tiers) - 1, gain))
        for i in (1, 2):
            t = tiers[min(i, len(tiers) - 1)]
            masks[i] |= sum(1 << f for f in t)
        live = [32 - len(t) for t in tiers]
        print("  MFMAs per body (full 16): " + ", ".join("T%d %d" % (i + 1, (n + 1) // 2) for i, n in enumerate(live)))
    print()
    print("MT_TIER1 = 0x%016x   (M_DEAD)" % masks[0])
    print("MT_TIER2 = 0x%016x" % masks[1])
    print("MT_TIER3 = 0x%016x" % masks[2])


if __name__ == "__main__":
    main()
