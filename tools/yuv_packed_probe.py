#!/usr/bin/env python3
"""What a packed frame costs beside the planar frame of the same samples: 1920x1080 -> 3840x2160, bicubic, strict mode, three
pairs -- YUY2 against planar 8-bit 4:2:2, v210 against planar 10-bit 4:2:2, Y410 against planar 10-bit 4:4:4 (Y410 also carries
a 2-bit alpha plane, which the planar frame has no place for).  Both calls of a pair run in this process on one stream,
alternating call by call, each timed with device events after a warm-up.  The yardstick is the planar call of the same run.

Usage: python tools/yuv_packed_probe.py [--frames N] [--out FILE]      (profiles/yuv_packed.txt is its output)
Kernel times of the unpack and pack kernels come from a run of their own under
`rocprofv3 --kernel-trace --stats -- python tools/yuv_packed_probe.py --frames 3` (k_yuvp_* against k_plane_*).
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import libsrcnn_amd as S

W, H, MUL = 1920, 1080, 2.0
# packed format, planar chroma, depth, alpha bits
PAIRS = [("yuy2", "422", 8, 0), ("v210", "422", 10, 0), ("y410", "444", 10, 2)]


def packed_frame(name, rng, depth, abits):
    """Random samples in the packed layout; the planar planes of the same samples."""
    cw = (W + 1) // 2 if name != "y410" else W
    dt = np.uint8 if depth == 8 else np.uint16
    Y = rng.integers(0, 1 << depth, (H, W)).astype(dt)
    U = rng.integers(0, 1 << depth, (H, cw)).astype(dt)
    V = rng.integers(0, 1 << depth, (H, cw)).astype(dt)
    u32 = lambda P: P.astype(np.uint32)   # noqa: E731
    if name == "yuy2":
        px = np.stack([Y[:, 0::2], U, Y[:, 1::2], V], -1)
        return np.ascontiguousarray(px).reshape(H, -1).view(np.uint8), (Y, U, V)
    if name == "y410":
        A = rng.integers(0, 1 << abits, (H, W))
        q = u32(U) | (u32(Y) << 10) | (u32(V) << 20) | (u32(A) << 30)
        return np.ascontiguousarray(q.astype("<u4")).view(np.uint8).reshape(H, 4 * W), (Y, U, V)
    g = 8 * ((W + 47) // 48)
    y, u, v = np.zeros((H, 6 * g), np.uint32), np.zeros((H, 3 * g), np.uint32), np.zeros((H, 3 * g), np.uint32)
    y[:, :W], u[:, :cw], v[:, :cw] = Y, U, V
    y, u, v = y.reshape(H, g, 6), u.reshape(H, g, 3), v.reshape(H, g, 3)
    q = np.stack([u[..., 0] | (y[..., 0] << 10) | (v[..., 0] << 20), y[..., 1] | (u[..., 1] << 10) | (y[..., 2] << 20),
                  v[..., 1] | (y[..., 3] << 10) | (u[..., 2] << 20), y[..., 4] | (v[..., 2] << 10) | (y[..., 5] << 20)], -1)
    return np.ascontiguousarray(q.astype("<u4")).view(np.uint8).reshape(H, 16 * g), (Y, U, V)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=12, help="timed repetitions of each call (at least 10 for a report)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    S.init(0)
    prev_mode = S.set_mode(S.MODE_STRICT)
    dw, dh = S.output_size(W, H, MUL)
    st = S.Stream()
    ev = [S.Event() for _ in range(4)]
    rng = np.random.default_rng(7)
    lines = ["yuv_packed_probe: %s, %dx%d -> %dx%d, bicubic, strict mode, %d timed repetitions per call after 3 warm-up rounds; packed and "
             "planar call of a pair alternate on one stream" % (S.device_name(), W, H, dw, dh, a.frames),
             "device-event ms per frame                     median     min     max   spread (max - min)"]
    notes = []
    for name, chroma, depth, abits in PAIRS:
        frame, planes = packed_frame(name, rng, depth, abits)
        rb, _ = S.yuv_packed_row_bytes(name, W)
        drb, _ = S.yuv_packed_row_bytes(name, dw)
        assert frame.shape == (H, rb)
        d_in, d_out = S.DeviceBuffer.from_numpy(frame), S.DeviceBuffer(dh * drb)
        fmt = S.yuv_format("planar", chroma, depth, False)
        _, _src_sizes, dst_sizes = S.yuv_plane_sizes(fmt, W, H, MUL)
        p_in = [S.DeviceBuffer.from_numpy(p) for p in planes]
        p_out = [S.DeviceBuffer(r * b) for (_c, r, b) in dst_sizes]

        def packed_call():
            S.yuv_packed_upscale_dev(name, W, H, MUL, S.SRCNNF_Bicubic, d_in, 0, d_out, 0, st)

        def planar_call():
            S.yuv_upscale_dev(fmt, W, H, MUL, S.SRCNNF_Bicubic, p_in, None, p_out, None, st)

        calls = [(packed_call, [], 0), (planar_call, [], 2)]
        for _ in range(3):
            for fn, _acc, _e in calls:
                fn()
        st.sync()
        for k in range(a.frames):
            order = calls[k % 2:] + calls[:k % 2]
            for fn, _acc, e in order:
                ev[e].record(st)
                fn()
                ev[e + 1].record(st)
            st.sync()
            for _fn, acc, e in order:
                acc.append(ev[e].elapsed_ms(ev[e + 1]))
        t_p, t_n = np.array(calls[0][1]), np.array(calls[1][1])
        m_p, m_n = float(np.median(t_p)), float(np.median(t_n))
        lines.append("  srcnn_yuv_packed_upscale_dev %-5s         %7.3f %7.3f %7.3f %7.3f" % (name, m_p, t_p.min(), t_p.max(), t_p.max() - t_p.min()))
        lines.append("  srcnn_yuv_upscale_dev planar %s %2d-bit   %7.3f %7.3f %7.3f %7.3f" % (chroma, depth, m_n, t_n.min(), t_n.max(), t_n.max() - t_n.min()))
        spread = float(t_n.max() - t_n.min())
        verdict = "within" if m_p - m_n <= spread else "ABOVE"
        lines.append("    packed - planar (medians): %+.3f ms = %+.2f %%; %s the planar call's own spread of %.3f ms" %
                     (m_p - m_n, 100.0 * (m_p - m_n) / m_n, verdict, spread))
        # the frame that was timed: the packed result holds the planar result's luma
        got = d_out.to_numpy(np.uint8, (dh, drb))
        want_y = p_out[0].to_numpy(np.uint8 if depth == 8 else np.uint16, (dh, dw))
        if name == "yuy2":
            got_y = got.reshape(dh, -1, 2)[:, :, 0][:, :dw]
        elif name == "y410":
            got_y = ((got.view("<u4").reshape(dh, dw) >> 10) & 1023).astype(np.uint16)
        else:
            q = got.view("<u4").reshape(dh, -1, 4)
            f = lambda k, s: (q[..., k] >> s) & 1023   # noqa: E731
            got_y = np.stack([f(0, 10), f(1, 0), f(1, 20), f(2, 10), f(3, 0), f(3, 20)], -1).reshape(dh, -1)[:, :dw].astype(np.uint16)
        same = bool(np.array_equal(got_y, want_y))
        notes.append("%s Y' equals the planar call's Y': %s" % (name, same))
        if not same:
            notes.append("MISMATCH in %s" % name)
        for b in [d_in, d_out] + p_in + p_out:
            b.free()
    lines += notes
    lines.append("y410 also resamples and packs a 2-bit alpha plane of full size, which its planar yardstick does not have.")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)
    st.destroy()
    S.set_mode(prev_mode)
    return 1 if any("MISMATCH" in n for n in notes) else 0


if __name__ == "__main__":
    sys.exit(main())
