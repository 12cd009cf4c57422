#!/usr/bin/env python3
"""What a 10-bit frame costs: 3840x2160 -> 7680x4320 P010 frames through srcnn_yuv_upscale_dev against (a) the 8-bit NV12 call
(srcnn_yuv420_upscale_dev) on the same frame >> 2 and (b) srcnn_y_upscale2x_f32_dev on the same Y plane as float, the three
calls rotated call by call on one stream, each timed with device events (the method of tools/yuv_probe.py).  The traffic the
16-bit call adds over the 8-bit one is also given in bytes, computed from the shapes.

Usage: python tools/yuv_ex_probe.py [--frames N] [--out FILE]      (profiles/yuv_ex_probe.txt is its output)
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import libsrcnn_amd as S
from libsrcnn_amd import synth


def integer_side_bytes(w, h, dw, dh, bps):
    """HBM bytes on the integer side of unpack and pack for a 4:2:0 frame with `bps` bytes per sample."""
    cw, ch, dcw, dch = (w + 1) // 2, (h + 1) // 2, (dw + 1) // 2, (dh + 1) // 2
    return bps * (w * h + 2 * cw * ch + dw * dh + 2 * dcw * dch)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    S.init(0)
    L = S.lib()
    w, h = 3840, 2160
    (dw, dh), (cw, ch), (dcw, dch) = S.yuv420_sizes(w, h, 2.0)
    y8 = np.clip(synth.plane(h, w, synth.SEED0, "smooth"), 0, 255).astype(np.uint8)
    rng = np.random.default_rng(7)
    y10 = (y8.astype(np.uint16) << 2) | rng.integers(0, 4, (h, w)).astype(np.uint16)
    uv10 = rng.integers(0, 1024, (ch, 2 * cw)).astype(np.uint16)
    p010 = S.yuv_format("semiplanar", "420", 10, True)
    d_y10, d_uv10 = S.DeviceBuffer.from_numpy(y10 << 6), S.DeviceBuffer.from_numpy(uv10 << 6)
    d_y10o, d_uv10o = S.DeviceBuffer(dw * dh * 2), S.DeviceBuffer(dch * 2 * dcw * 2)
    d_y8, d_uv8 = S.DeviceBuffer.from_numpy((y10 >> 2).astype(np.uint8)), S.DeviceBuffer.from_numpy((uv10 >> 2).astype(np.uint8))
    d_y8o, d_uv8o = S.DeviceBuffer(dw * dh), S.DeviceBuffer(dch * 2 * dcw)
    yf = y10.astype(np.float32) * np.float32(0.25)
    d_yf = S.DeviceBuffer.from_numpy(yf)
    d_out = S.DeviceBuffer(dw * dh * 4)
    st = S.Stream()
    ev = [S.Event() for _ in range(6)]

    def p010_call():
        S.yuv_upscale_dev(p010, w, h, 2.0, S.SRCNNF_Bicubic, [d_y10, d_uv10, None], None, [d_y10o, d_uv10o, None], None, st)

    def nv12_call():
        S.yuv420_upscale_dev(S.YUV_NV12, w, h, 2.0, S.SRCNNF_Bicubic, [d_y8, d_uv8, None], None, [d_y8o, d_uv8o, None], None, st)

    def fy():
        S.check(L.srcnn_y_upscale2x_f32_dev(d_yf.ptr, w, h, d_out.ptr, st.handle))

    calls = [(p010_call, [], 0), (nv12_call, [], 2), (fy, [], 4)]
    for _ in range(3):
        for fn, _, _ in calls:
            fn()
    st.sync()
    for k in range(a.frames):
        order = calls[k % 3:] + calls[:k % 3]
        for fn, _, e in order:
            ev[e].record(st)
            fn()
            ev[e + 1].record(st)
        st.sync()
        for _, acc, e in order:
            acc.append(ev[e].elapsed_ms(ev[e + 1]))
    # the P010 Y' equals the float path scaled and truncated (a spot check of the frame that was timed)
    got = d_y10o.to_numpy(np.uint16, (dh, dw))
    want = ((d_out.to_numpy(np.float32, (dh, dw)) * np.float32(4.0)).astype(np.uint32) << 6).astype(np.uint16)
    same = bool(np.array_equal(got, want))
    t_p, t_n, t_f = (np.array(c[1]) for c in calls)
    m_p, m_n, m_f = float(np.median(t_p)), float(np.median(t_n)), float(np.median(t_f))
    extra = integer_side_bytes(w, h, dw, dh, 2) - integer_side_bytes(w, h, dw, dh, 1)
    lines = [
        "yuv_ex_probe: %s, %d frames %dx%d -> %dx%d, bicubic, P010 / NV12 (same frame >> 2) / srcnn_y_upscale2x_f32_dev rotated on one stream"
        % (S.device_name(), a.frames, w, h, dw, dh),
        "device-event ms per frame           median    mean     min     max",
        "  srcnn_yuv_upscale_dev (P010)    %7.3f %7.3f %7.3f %7.3f" % (m_p, t_p.mean(), t_p.min(), t_p.max()),
        "  srcnn_yuv420_upscale_dev (NV12) %7.3f %7.3f %7.3f %7.3f" % (m_n, t_n.mean(), t_n.min(), t_n.max()),
        "  srcnn_y_upscale2x_f32_dev       %7.3f %7.3f %7.3f %7.3f" % (m_f, t_f.mean(), t_f.min(), t_f.max()),
        "P010 over NV12 (medians): %+.3f ms = %+.2f %%" % (m_p - m_n, 100.0 * (m_p - m_n) / m_n),
        "P010 over the float Y path (medians): %+.3f ms = %+.2f %%" % (m_p - m_f, 100.0 * (m_p - m_f) / m_f),
        "NV12 over the float Y path (medians): %+.3f ms = %+.2f %%" % (m_n - m_f, 100.0 * (m_n - m_f) / m_f),
        "extra traffic of the 16-bit call over the 8-bit one, from the shapes (integer side of unpack and pack): %.1f MB" % (extra / 1e6),
        "P010 Y' equals the scaled, truncated float path: %s" % same,
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
