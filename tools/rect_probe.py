#!/usr/bin/env python3
"""What one rectangle of the output costs: 3840x2160 -> 7680x4320, bicubic, strict mode, srcnn_y_path_rect_f32_dev.

  whole     srcnn_y_upscale2x_f32_dev, the whole frame
  band512   srcnn_y_upscale2x_f32_band_dev, 512 full-width rows -- what a caller had to pay for any rect 512 rows high before
  rects     64x64, 512x512 (interior and bottom-right corner), 960x512, 1920x1080, 3840x512

All calls run in one process on one stream, rotated call by call, after 3 warm-up rounds; each is timed with device events
around the call (median of --calls).  A second pass with srcnn_profile_enable gives the mean time of each stage of a call
(resample / layers 1+2 / layer 3); what the stages leave of the call's median is the window store and the launch gaps.

Condition (stated before measuring): the 960x512 rect takes less than half the median device time of the 512-row band -- the
band is 120 x 33 tiles of the persistent layer-1+2 grid (8 rounds of 512 workgroups), the rect 16 x 33 (2 rounds), layer 3
scales by the same column ratio, and the factor 2 over that 0.25 covers launches, the generic resampler and the store.  Every
other number is reported, not gated.

Usage: python tools/rect_probe.py [--calls N] [--commit TEXT] [--out FILE]      (profiles/rect_probe.txt is its output)
"""
import argparse
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import libsrcnn_amd as S
from libsrcnn_amd import build, synth


def commit_text(given):
    if given:
        return given
    try:
        return subprocess.run(["git", "-C", ROOT, "rev-parse", "HEAD"], capture_output=True, text=True, check=True).stdout.strip()
    except (OSError, subprocess.CalledProcessError):
        return "unknown (no git here)"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--commit", default=None, help="what to record as the commit (default: git rev-parse HEAD)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.calls < 10:
        ap.error("--calls: at least 10 timed calls")
    S.init(0)
    S.set_mode(S.MODE_STRICT)
    L = S.lib()
    w, h = 3840, 2160
    dw, dh = 2 * w, 2 * h
    y = synth.plane(h, w, synth.SEED0 + 3, "smooth")
    d_in = S.DeviceBuffer.from_numpy(y)
    d_whole = S.DeviceBuffer(4 * dw * dh)
    d_band = S.DeviceBuffer(4 * dw * 512)
    st = S.Stream()
    ev = [S.Event(), S.Event()]

    rects = [("rect 64x64 interior", 3808, 2128, 64, 64), ("rect 512x512 interior", 3584, 1904, 512, 512),
             ("rect 512x512 corner", dw - 512, dh - 512, 512, 512), ("rect 960x512 interior", 3360, 1904, 960, 512),
             ("rect 1920x1080 interior", 2880, 1620, 1920, 1080), ("rect 3840x512 interior", 1920, 1904, 3840, 512)]
    d_rect = {name: S.DeviceBuffer(4 * rw * rh) for (name, _x, _y, rw, rh) in rects}

    def whole():
        S.check(L.srcnn_y_upscale2x_f32_dev(d_in.ptr, w, h, d_whole.ptr, st.handle))

    def band():
        S.check(L.srcnn_y_upscale2x_f32_band_dev(d_in.ptr, w, h, 1904, 512, d_band.ptr, st.handle))

    def rect_call(name, x0, y0, rw, rh):
        return lambda: S.y_path_rect_dev(d_in, 0, w, h, dw, dh, S.SRCNNF_Bicubic, x0, y0, rw, rh, d_rect[name], 0, st)

    calls = [("whole frame 7680x4320", whole), ("band 512 rows x 7680", band)] + [(r[0], rect_call(*r)) for r in rects]
    pixels = {"whole frame 7680x4320": dw * dh, "band 512 rows x 7680": dw * 512}
    pixels.update({r[0]: r[3] * r[4] for r in rects})
    series = {name: [] for name, _ in calls}

    def timed(name, fn, keep):
        st.sync()
        ev[0].record(st)
        fn()
        ev[1].record(st)
        st.sync()
        if keep:
            series[name].append(ev[0].elapsed_ms(ev[1]))

    for _ in range(3):
        for name, fn in calls:
            timed(name, fn, False)
    n = len(calls)
    for k in range(a.calls):
        for name, fn in calls[k % n:] + calls[:k % n]:
            timed(name, fn, True)

    # per-stage means: a pass of its own, because the stage timers put event pairs inside the call
    stages = {}
    S.profile_enable(True)
    try:
        for name, fn in calls:
            st.sync()
            S.profile_reset()
            for _ in range(a.calls):
                fn()
            st.sync()
            prof = S.profile_read()
            stages[name] = {k: prof[k][0] / a.calls for k in S.STAGES}
    finally:
        S.profile_enable(False)

    # the rects that were timed are the whole frame's samples
    frame = d_whole.to_numpy(np.float32, (dh, dw))
    same = all(np.array_equal(d_rect[name].to_numpy(np.float32, (rh, rw)).view(np.uint32), frame[y0:y0 + rh, x0:x0 + rw].view(np.uint32))
               for (name, x0, y0, rw, rh) in rects)
    same = same and np.array_equal(d_band.to_numpy(np.float32, (512, dw)).view(np.uint32), frame[1904:1904 + 512].view(np.uint32))

    def stats(v):
        v = np.array(v)
        return float(np.median(v)), float(np.percentile(v, 75) - np.percentile(v, 25)), float(v.min()), float(v.max())

    lines = ["rect_probe: %s, strict mode, %d timed calls each after 3 warm-up rounds, %dx%d -> %dx%d, bicubic, rotated on one stream"
             % (S.device_name(), a.calls, w, h, dw, dh),
             "commit: %s    source digest: %s" % (commit_text(a.commit), build.source_digest()[:16]),
             "device events, ms per call            median     IQR     min     max   ns/pixel | stage means: resample  conv12   conv3   rest | resample share"]
    med = {}
    for name, _ in calls:
        m, iqr, lo, hi = stats(series[name])
        med[name] = (m, iqr)
        sg = stages[name]
        rest = m - sum(sg.values())
        lines.append("  %-32s %9.4f %7.4f %7.4f %7.4f %9.3f | %20.4f %7.4f %7.4f %6.4f | %5.1f %%"
                     % (name, m, iqr, lo, hi, 1e6 * m / pixels[name], sg["resample"], sg["conv12"], sg["conv3"], rest, 100.0 * sg["resample"] / m))
    b, r = med["band 512 rows x 7680"], med["rect 960x512 interior"]
    ratio = r[0] / b[0]
    lines += ["condition: rect 960x512 < 0.5 x band 512 rows: %.4f ms vs %.4f ms, ratio %.3f (IQRs %.4f / %.4f ms) -- %s"
              % (r[0], b[0], ratio, r[1], b[1], "MET" if ratio < 0.5 else "NOT MET by %.0f %%" % (100.0 * (ratio / 0.5 - 1.0))),
              "every timed rect and the band hold the whole frame's bits: %s" % same]
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
