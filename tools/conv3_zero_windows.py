#!/usr/bin/env python3
"""How often is a layer-2 channel all zero over everything one wave of the strict layer-3 kernel reads?

k_conv3 works on 64 x 16 tiles; each of a workgroup's four waves owns 64 columns x 4 rows and reads, per channel, that
rectangle plus a 2-sample halo, clamped to the image: a 68 x 8 window.  A wave may skip a channel whose window is all +-0
(C3_SPARSE in srcnn_kernels.hip names the channels it tests).  This tool counts, on the CPU and through the oracle, the
share of such windows per channel for the butterfly golden image and for synth frames of both generators, and prints the
candidate set: every channel that is all zero on at least 25 % of the windows of some input.

    python tools/conv3_zero_windows.py > profiles/conv3_zero_windows.txt

No GPU is needed.  tests/test_gpu_conv3_skip.py reads the `C3_SPARSE` line of the committed output.
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import oracle                              # noqa: E402
from libsrcnn_amd import synth             # noqa: E402

TW, TH, WAVE_ROWS, HALO = 64, 16, 4, 2
KEEP = 0.25


def zero_window_share(c2):
    """c2: (32, H, W) layer-2 activations.  Returns (share[32], windows): per channel, the share of wave windows (waves with
    at least one row and one column inside the image) whose clamped 68 x 8 window holds nothing but +-0."""
    nz = np.abs(c2) != 0                                  # NaN counts as not zero, -0 as zero
    _, h, w = c2.shape
    hits = np.zeros(32, np.int64)
    n = 0
    for y0 in range(0, h, WAVE_ROWS):
        ra, rb = max(y0 - HALO, 0), min(y0 + WAVE_ROWS + HALO, h)
        for x0 in range(0, w, TW):
            ca, cb = max(x0 - HALO, 0), min(x0 + TW + HALO, w)
            hits += ~nz[:, ra:rb, ca:cb].any(axis=(1, 2))
            n += 1
    return hits / float(n), n


def inputs():
    g = np.load(os.path.join(ROOT, "tests", "golden", "butterfly.npz"))
    f = g["rgb_in"].astype(np.float32)
    F = np.float32
    yield "butterfly 256x256 (luma of tests/golden/butterfly.npz)", (F(0.299) * f[..., 0]) + (F(0.587) * f[..., 1]) + (F(0.114) * f[..., 2])
    for kind in ("smooth", "noise"):
        for (h, w) in ((272, 480), (540, 960)):
            for seed in (synth.SEED0, synth.SEED0 + 3):
                yield "synth %s %dx%d seed SEED0+%d" % (kind, w, h, seed - synth.SEED0), synth.plane(h, w, seed, kind)


def main():
    orc = oracle.Oracle()
    best = np.zeros(32)
    print("share of all-zero 68x8 wave windows per layer-2 channel (2x upscale, oracle activations); channels below 0.005 omitted")
    for name, y in inputs():
        _out, _up, _c1, c2 = orc.y_path(y, taps=True)
        share, n = zero_window_share(c2)
        best = np.maximum(best, share)
        shown = "  ".join("%d:%.2f" % (m, share[m]) for m in range(32) if share[m] >= 0.005)
        print("%-58s %5d windows  mean skippable %.3f  | %s" % (name, n, share.mean(), shown or "-"))
    keep = [m for m in range(32) if best[m] >= KEEP]
    print("best share per channel over the inputs: " + "  ".join("%d:%.2f" % (m, best[m]) for m in range(32) if best[m] >= 0.005))
    print("kept (all zero on >= %d %% of the windows of some input): %s" % (int(KEEP * 100), " ".join(map(str, keep))))
    print("C3_SPARSE = 0x%08x" % sum(1 << m for m in keep))


if __name__ == "__main__":
    main()
