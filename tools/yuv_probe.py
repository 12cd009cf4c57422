#!/usr/bin/env python3
"""What the 8-bit YUV 4:2:0 call costs over the float Y path it is built on: 3840x2160 -> 7680x4320 NV12 frames through
srcnn_yuv420_upscale_dev against srcnn_y_upscale2x_f32_dev on the same Y plane (as float), alternating the two call by call
on one stream, each timed with device events.  The extra work of the YUV call (u8 <-> float conversions, two chroma
resamples) is also given in bytes, computed from the shapes.

Usage: python tools/yuv_probe.py [--frames N] [--out FILE]      (profiles/yuv_probe.txt is its output)
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import libsrcnn_amd as S
from libsrcnn_amd import synth


def extra_bytes(w, h, dw, dh):
    """HBM bytes the YUV call moves beyond the Y path, from the shapes (every access counted once)."""
    cw, ch, dcw, dch = (w + 1) // 2, (h + 1) // 2, (dw + 1) // 2, (dh + 1) // 2
    unpack = (w * h + 2 * cw * ch) * (1 + 4)                 # u8 in, float out
    chroma = 2 * (cw * ch + dcw * dch) * 4                   # two plane resamples, float in and out
    pack = (dw * dh + 2 * dcw * dch) * (4 + 1)               # float in, u8 out
    return unpack, chroma, pack


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    S.init(0)
    L = S.lib()
    w, h = 3840, 2160
    (dw, dh), (cw, ch), (dcw, dch) = S.yuv420_sizes(w, h, 2.0)
    y = np.clip(synth.plane(h, w, synth.SEED0, "smooth"), 0, 255).astype(np.uint8)
    uv = np.random.default_rng(7).integers(0, 256, (ch, 2 * cw), dtype=np.uint8)
    d_y, d_uv = S.DeviceBuffer.from_numpy(y), S.DeviceBuffer.from_numpy(uv)
    d_yo, d_uvo = S.DeviceBuffer(dw * dh), S.DeviceBuffer(dch * 2 * dcw)
    d_yf = S.DeviceBuffer.from_numpy(y.astype(np.float32))
    d_out = S.DeviceBuffer(dw * dh * 4)
    st = S.Stream()
    ev = [S.Event() for _ in range(4)]

    def yuv():
        S.yuv420_upscale_dev(S.YUV_NV12, w, h, 2.0, S.SRCNNF_Bicubic, [d_y, d_uv, None], None, [d_yo, d_uvo, None], None, st)

    def fy():
        S.check(L.srcnn_y_upscale2x_f32_dev(d_yf.ptr, w, h, d_out.ptr, st.handle))

    for _ in range(3):
        yuv()
        fy()
    st.sync()
    t_yuv, t_f = [], []
    for k in range(a.frames):
        order = ((yuv, t_yuv, 0), (fy, t_f, 2)) if k % 2 == 0 else ((fy, t_f, 2), (yuv, t_yuv, 0))
        for fn, _, e in order:
            ev[e].record(st)
            fn()
            ev[e + 1].record(st)
        st.sync()
        for _, acc, e in order:
            acc.append(ev[e].elapsed_ms(ev[e + 1]))
    # the Y' bytes equal the truncated float path (a spot check of the frame that was timed)
    got = d_yo.to_numpy(np.uint8, (dh, dw))
    want = d_out.to_numpy(np.float32, (dh, dw)).astype(np.uint8)
    same = bool(np.array_equal(got, want))
    unpack, chroma, pack = extra_bytes(w, h, dw, dh)
    med_yuv, med_f = float(np.median(t_yuv)), float(np.median(t_f))
    lines = [
        "yuv_probe: %s, %d frames %dx%d -> %dx%d, NV12 bicubic, alternating with srcnn_y_upscale2x_f32_dev on one stream"
        % (S.device_name(), a.frames, w, h, dw, dh),
        "device-event ms per frame      median    mean     min     max",
        "  srcnn_yuv420_upscale_dev   %7.3f %7.3f %7.3f %7.3f" % (med_yuv, np.mean(t_yuv), np.min(t_yuv), np.max(t_yuv)),
        "  srcnn_y_upscale2x_f32_dev  %7.3f %7.3f %7.3f %7.3f" % (med_f, np.mean(t_f), np.min(t_f), np.max(t_f)),
        "overhead of the YUV call (medians): %+.3f ms = %+.2f %%" % (med_yuv - med_f, 100.0 * (med_yuv - med_f) / med_f),
        "extra traffic from the shapes: unpack %.1f MB, chroma resamples %.1f MB, pack %.1f MB, total %.1f MB"
        % (unpack / 1e6, chroma / 1e6, pack / 1e6, (unpack + chroma + pack) / 1e6),
        "Y' equals the truncated float path: %s" % same,
    ]
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)
    st.destroy()
    return 0 if same else 1


if __name__ == "__main__":
    sys.exit(main())
