#!/usr/bin/env python3
"""Layers 1+2 by kernel, A/B of two builds and the SRCNN_CONV12_TIERS switch on one box:

    python tools/conv12_ab_probe.py PARENT.so [rounds]

Three arms, alternating, a fresh child process per measurement: the parent build (SRCNN_AMD_LIB=PARENT.so), this tree's
build, and this tree's build with SRCNN_CONV12_TIERS=0.  Each child takes one 3840x2160 -> 7680x4320 frame of each generator
(`smooth`, `noise`), times the layers-1+2 stage call alone and the whole strict path with HIP events (8 calls per timing, 6
repeats: min and median) and prints a checksum of the layer-2 planes and of the result, so that arms that disagree are visible
at once.

On `noise` nothing beyond M_DEAD is ever zero, so the nested-tiers instance of k_conv12_mfma only pays its extra compares there; bench.py's
`generators.noise` is a 3-step figure whose run-to-run spread (1.4 %) is larger than that.  This is the instrument behind the
`noise` lines of profiles/conv12_tiers_ab.txt (tools/conv3_ab_probe.py is its layer-3 twin).  A child that fails or runs past
its limit ends the probe: nothing more is started on the device after it."""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHILD = r'''
import sys, hashlib
sys.path.insert(0, %r)
import numpy as np, libsrcnn_amd as S
from libsrcnn_amd import synth
S.init(0); L = S.lib()
h, w = 2160, 3840; H, W = 2*h, 2*w
for kind in ("smooth", "noise"):
    din = S.DeviceBuffer.from_numpy(synth.plane(h, w, synth.SEED0, kind))
    up = S.DeviceBuffer(H*W*4); c2 = S.DeviceBuffer(32*H*W*4); out = S.DeviceBuffer(H*W*4)
    S.check(L.srcnn_resample_f32_dev(din.ptr, w, h, W, H, 2, up.ptr, None)); S.sync()
    def t(fn, reps=6, n=8):
        fn(); S.sync(); ts = []
        for _ in range(reps):
            e0, e1 = S.Event(), S.Event(); e0.record()
            for _ in range(n): fn()
            e1.record(); S.sync(); ts.append(e0.elapsed_ms(e1)/n)
        return min(ts), sorted(ts)[len(ts)//2]
    c12 = t(lambda: S.check(L.srcnn_conv12_f32_dev(up.ptr, W, H, c2.ptr, None)))
    sha2 = hashlib.sha256(c2.to_numpy(np.float32, (8, H, W)).tobytes()).hexdigest()[:12]      # the first 8 planes
    whole = t(lambda: S.check(L.srcnn_y_upscale2x_f32_dev(din.ptr, w, h, out.ptr, None)))
    sha = hashlib.sha256(out.to_numpy(np.float32, (H, W)).tobytes()).hexdigest()[:12]
    print("%%-8s %%-6s conv12 min %%.4f med %%.4f ms   whole min %%.4f med %%.4f ms   sha c2 %%s out %%s" %% (sys.argv[1], kind, c12[0], c12[1], whole[0], whole[1], sha2, sha), flush=True)
    del din, up, c2, out
''' % ROOT


def main():
    if len(sys.argv) < 2:
        sys.exit(__doc__)
    parent = os.path.abspath(sys.argv[1])
    rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 3
    arms = [("parent", {"SRCNN_AMD_LIB": parent}), ("new", {}), ("off", {"SRCNN_CONV12_TIERS": "0"})]
    for _ in range(rounds):
        for name, env in arms:
            try:
                rc = subprocess.call([sys.executable, "-c", CHILD, name], env=dict(os.environ, **env), timeout=150)
            except subprocess.TimeoutExpired:
                rc = 124
            if rc != 0:
                print("FAILED", name, rc, flush=True)
                sys.exit(rc)


if __name__ == "__main__":
    main()
