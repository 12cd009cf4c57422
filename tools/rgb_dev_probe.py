#!/usr/bin/env python3
"""What an RGB image that already sits in device memory costs: 3840x2160 RGB -> 7680x4320, bicubic, strict mode.

  (a) srcnn_rgb_upscale_dev, tight interleaved 8-bit RGB   -- the fused colour shell (the fast path)
  (b) srcnn_rgb_upscale_dev, the same image as BGR         -- unpack / plane resamples / pack (the general path)
  (c) srcnn_process_u8 with page-locked buffers            -- the host-pointer call: the same device work + both PCIe copies
  (d) srcnn_y_upscale2x_f32_dev on one float plane         -- the Y path alone

All four run in one process, rotated call by call, after 3 warm-up rounds.  (a), (b) and (d) are timed twice per call: with
device events around the call on its stream, and with the host clock from the call to the end of a stream synchronise; (c) is a
blocking host call and has the host clock only.  (a) and (c) are compared on the host clock, the colour shell's cost over the Y
path on device events.  The spread given is each series' interquartile range and min .. max: a difference of medians inside it
is reported as such, not as a win.

Usage: python tools/rgb_dev_probe.py [--calls N] [--out FILE]      (profiles/rgb_dev.txt is its output)
"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import libsrcnn_amd as S
from libsrcnn_amd import synth


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.calls < 10:
        ap.error("--calls: at least 10 timed calls")
    S.init(0)
    S.set_mode(S.MODE_STRICT)
    L = S.lib()
    w, h = 3840, 2160
    dw, dh = S.output_size(w, h, 2.0)
    rgb = np.stack([np.clip(synth.plane(h, w, synth.SEED0 + k, "smooth"), 0, 255).astype(np.uint8) for k in range(3)], axis=-1)
    rgb[::7, ::5] = np.random.default_rng(3).integers(0, 256, rgb[::7, ::5].shape, dtype=np.uint8)
    fmt_rgb, fmt_bgr = S.rgb_format("interleaved", "rgb", False, 8), S.rgb_format("interleaved", "bgr", False, 8)
    d_rgb = S.DeviceBuffer.from_numpy(rgb)
    d_bgr = S.DeviceBuffer.from_numpy(rgb[..., ::-1])
    d_out_a, d_conv_a = S.DeviceBuffer(dw * dh * 3), S.DeviceBuffer(dw * dh)
    d_out_b, d_conv_b = S.DeviceBuffer(dw * dh * 3), S.DeviceBuffer(dw * dh)
    p_in, p_out, p_conv = S.PinnedArray((h, w, 3)), S.PinnedArray((dh, dw, 3)), S.PinnedArray((dh, dw))
    p_in.array[...] = rgb
    d_y = S.DeviceBuffer.from_numpy(np.ascontiguousarray(rgb[..., 1], np.float32))
    d_yo = S.DeviceBuffer(dw * dh * 4)
    st = S.Stream()
    ev = [S.Event(), S.Event()]

    def call_a():
        S.rgb_upscale_dev(fmt_rgb, w, h, 2.0, S.SRCNNF_Bicubic, [d_rgb], None, [d_out_a], None, d_conv_a, 0, st)

    def call_b():
        S.rgb_upscale_dev(fmt_bgr, w, h, 2.0, S.SRCNNF_Bicubic, [d_bgr], None, [d_out_b], None, d_conv_b, 0, st)

    def call_c():
        S.check(L.srcnn_process_u8(p_in.ptr, w, h, 3, 2.0, S.SRCNNF_Bicubic, p_out.ptr, p_conv.ptr))

    def call_d():
        S.check(L.srcnn_y_upscale2x_f32_dev(d_y.ptr, w, h, d_yo.ptr, st.handle))

    series = {"a": ([], []), "b": ([], []), "c": ([], []), "d": ([], [])}       # (device-event ms, host-clock ms)
    calls = [("a", call_a), ("b", call_b), ("c", call_c), ("d", call_d)]

    def timed(name, fn, keep):
        st.sync()
        t0 = time.perf_counter()
        if name == "c":
            fn()
            wall, dev = (time.perf_counter() - t0) * 1e3, None
        else:
            ev[0].record(st)
            fn()
            ev[1].record(st)
            st.sync()
            wall, dev = (time.perf_counter() - t0) * 1e3, ev[0].elapsed_ms(ev[1])
        if keep:
            series[name][1].append(wall)
            if dev is not None:
                series[name][0].append(dev)

    for _ in range(3):
        for name, fn in calls:
            timed(name, fn, False)
    for k in range(a.calls):
        for name, fn in calls[k % 4:] + calls[:k % 4]:
            timed(name, fn, True)

    # the frames that were timed: all three colour calls gave the same bytes
    out_a, conv_a = d_out_a.to_numpy(np.uint8, (dh, dw, 3)), d_conv_a.to_numpy(np.uint8, (dh, dw))
    out_b, conv_b = d_out_b.to_numpy(np.uint8, (dh, dw, 3))[..., ::-1], d_conv_b.to_numpy(np.uint8, (dh, dw))
    same = bool(np.array_equal(out_a, p_out.array) and np.array_equal(conv_a, p_conv.array) and
                np.array_equal(out_b, p_out.array) and np.array_equal(conv_b, p_conv.array))

    def stats(v):
        v = np.array(v)
        return float(np.median(v)), float(np.percentile(v, 75) - np.percentile(v, 25)), float(v.min()), float(v.max())

    names = {"a": "(a) srcnn_rgb_upscale_dev RGB, fused shell", "b": "(b) srcnn_rgb_upscale_dev BGR, plane shell",
             "c": "(c) srcnn_process_u8, page-locked buffers", "d": "(d) srcnn_y_upscale2x_f32_dev"}
    lines = ["rgb_dev_probe: %s, strict mode, %d timed calls each after 3 warm-up rounds, %dx%d RGB -> %dx%d, bicubic, rotated in one process"
             % (S.device_name(), a.calls, w, h, dw, dh),
             "ms per call                                      median     IQR     min     max"]
    dev, wall = {}, {}
    for k in "abd":
        dev[k] = stats(series[k][0])
        lines.append("  device events  %-32s %7.3f %7.3f %7.3f %7.3f" % (names[k], *dev[k]))
    for k in "abcd":
        wall[k] = stats(series[k][1])
        lines.append("  host clock     %-32s %7.3f %7.3f %7.3f %7.3f" % (names[k], *wall[k]))
    diff = wall["a"][0] - wall["c"][0]
    spread = max(wall["a"][1], wall["c"][1])
    verdict = ("inside the run-to-run spread (IQR %.3f ms): neither is faster" % spread) if abs(diff) <= spread else \
              ("(a) is faster" if diff < 0 else "(a) is SLOWER")
    lines += ["(a) - (c), host clock medians: %+.3f ms = %+.1f %% -- %s" % (diff, 100.0 * diff / wall["c"][0], verdict),
              "colour shell over the Y path, device-event medians: fused shell (a) - (d) = %+.3f ms, plane shell (b) - (d) = %+.3f ms"
              % (dev["a"][0] - dev["d"][0], dev["b"][0] - dev["d"][0]),
              "(a), (b) and (c) gave the same bytes: %s" % same]
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)
    st.destroy()
    for p in (p_in, p_out, p_conv):
        p.free()
    return 0 if same else 1


if __name__ == "__main__":
    sys.exit(main())
