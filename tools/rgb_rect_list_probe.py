#!/usr/bin/env python
"""What a LIST of rectangles of an RGB(A) image costs: 3840x2160 -> 7680x4320, 8-bit interleaved RGB, bicubic, strict mode,
srcnn_rgb_upscale_rect_list_dev (include/srcnn_amd_rgb_rect_list.h) against the loop of srcnn_rgb_upscale_rect_dev over the same
rects and against srcnn_y_path_rect_list_f32_dev over the same rects of a float Y plane.

  the lists   256 rects of 32x32, 64 of 64x64, 16 of 256x256, 4 of 960x512 (the lists of tools/rect_list_probe.py: seeded
              positions, every eighth on a border).  Per list:
                (a) list    one srcnn_rgb_upscale_rect_list_dev call, every item with a tight destination of its own
                (b) loop    n srcnn_rgb_upscale_rect_dev calls into the same destinations
                (c) Y list  one srcnn_y_path_rect_list_f32_dev call over the float Y plane of the image
              reported: (b) / (a), and the colour cost ((a) - (c)) / (c)

Before anything is timed every item of (a) is compared with (b), byte for byte; a difference ends the probe with exit code 1.
Device-event medians of N calls (default 20) after 3 warm-up rounds, the candidates rotated on one stream so that a clock
drift hits all alike; the IQR beside every median.

Usage: python tools/rgb_rect_list_probe.py [--calls N] [--commit TEXT] [--out FILE]   (profiles/rgb_rect_list_probe.txt is its output)
"""
import argparse
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import libsrcnn_amd as S
from libsrcnn_amd import build
from rect_list_probe import DH, DW, H, LISTS, W, commit_text, positions, stats


class Bench:
    def __init__(self, calls):
        S.init(0)
        S.set_mode(S.MODE_STRICT)
        self.calls = calls
        rng = np.random.default_rng(20240612)
        # smooth content with noise on top, as a UI surface is neither flat nor white noise
        yy, xx = np.mgrid[0:H, 0:W].astype(np.float32)
        base = np.stack([127 + 100 * np.sin(xx / 97 + k) * np.cos(yy / 61 - k) for k in range(3)], axis=-1)
        img = np.clip(base + rng.integers(-20, 21, base.shape), 0, 255).astype(np.uint8)
        self.fmt = S.rgb_format("interleaved", "rgb", False, 8)
        self.d_img = S.DeviceBuffer.from_numpy(img)
        f = img.astype(np.float32)
        y = (np.float32(0.299) * f[..., 0]) + (np.float32(0.587) * f[..., 1]) + (np.float32(0.114) * f[..., 2])
        self.d_y = S.DeviceBuffer.from_numpy(np.ascontiguousarray(y, np.float32))
        self.st = S.Stream()
        self.ev = [S.Event(), S.Event()]
        self.bufs = {}

    def layout(self, key, rects, bytes_per_pixel):
        offs, total = [], 0
        for (_, _, rw, rh) in rects:
            offs.append(total)
            total += (bytes_per_pixel * rw * rh + 15) & ~15
        return self.bufs.setdefault(key, S.DeviceBuffer(total)), offs

    def list_call(self, name, rects):
        buf, offs = self.layout(name + "/list", rects, 3)
        arr, _ = S.rgb_rect_items([(x0, y0, rw, rh, [(buf, o)], None) for (x0, y0, rw, rh), o in zip(rects, offs)])
        return lambda: S.rgb_upscale_rect_list_dev(self.fmt, W, H, 2.0, S.SRCNNF_Bicubic, [self.d_img], None, arr, self.st)

    def loop_call(self, name, rects):
        buf, offs = self.layout(name + "/loop", rects, 3)

        def run():
            for (x0, y0, rw, rh), o in zip(rects, offs):
                S.rgb_upscale_rect_dev(self.fmt, W, H, 2.0, S.SRCNNF_Bicubic, [self.d_img], None, x0, y0, rw, rh, [(buf, o)], None, None, 0, self.st)
        return run

    def y_list_call(self, name, rects):
        buf, offs = self.layout(name + "/ylist", rects, 4)
        arr, _ = S.rect_items([(x0, y0, rw, rh, (buf, o), 0) for (x0, y0, rw, rh), o in zip(rects, offs)])
        return lambda: S.y_path_rect_list_dev(self.d_y, 0, W, H, DW, DH, S.SRCNNF_Bicubic, arr, self.st)

    def same_bytes(self, name, rects):
        """every item of the list call against the loop of single calls, byte for byte"""
        self.list_call(name, rects)()
        self.loop_call(name, rects)()
        self.st.sync()
        (a, offs), (b, _) = self.layout(name + "/list", rects, 3), self.layout(name + "/loop", rects, 3)
        fa, fb = a.to_numpy(np.uint8, (a.nbytes,)), b.to_numpy(np.uint8, (b.nbytes,))
        return all(np.array_equal(fa[o:o + 3 * rw * rh], fb[o:o + 3 * rw * rh]) for (_, _, rw, rh), o in zip(rects, offs))

    def measure(self, calls):
        """calls: [(key, fn)].  Returns {key: [ms, ...]}."""
        series = {k: [] for k, _ in calls}

        def timed(key, fn, keep):
            self.st.sync()
            self.ev[0].record(self.st)
            fn()
            self.ev[1].record(self.st)
            self.st.sync()
            if keep:
                series[key].append(self.ev[0].elapsed_ms(self.ev[1]))
        for _ in range(3):
            for key, fn in calls:
                timed(key, fn, False)
        n = len(calls)
        for k in range(self.calls):
            for key, fn in calls[k % n:] + calls[:k % n]:
                timed(key, fn, True)
        return series


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--commit", default=None, help="what to record as the commit (default: git rev-parse HEAD)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.calls < 10:
        ap.error("--calls: at least 10 timed calls")
    b = Bench(a.calls)
    lists = [(name, positions(1000 + k, n, rw, rh)) for k, (name, n, rw, rh) in enumerate(LISTS)]
    same = {name: b.same_bytes(name, rects) for name, rects in lists}
    if not all(same.values()):
        print("the list call and the loop of single calls differ: %r" % same)
        return 1
    calls = []
    for name, rects in lists:
        calls += [(name + "/list", b.list_call(name, rects)), (name + "/loop", b.loop_call(name, rects)), (name + "/ylist", b.y_list_call(name, rects))]
    med = {k: stats(v) for k, v in b.measure(calls).items()}
    plans = {name: S.rgb_upscale_rect_list_plan(b.fmt, W, H, 2.0, S.SRCNNF_Bicubic, rects) for name, rects in lists}
    b.st.destroy()
    lines = ["rgb_rect_list_probe: %s, strict mode, %d timed calls each after 3 warm-up rounds, %dx%d -> %dx%d, 8-bit interleaved RGB, bicubic, rotated on one stream"
             % (S.device_name(), a.calls, W, H, DW, DH),
             "commit: %s    source digest: %s" % (commit_text(a.commit), build.source_digest()[:16]),
             "every item of every list call equals the loop of single calls, byte for byte (checked before timing): True",
             "device events, ms per call      (a) list median  IQR | (b) loop median     IQR | (b) / (a) | (c) Y list median  IQR | colour cost ((a) - (c)) / (c) | batched single atlases"]
    for name, _ in lists:
        p = plans[name]
        (lm, li), (om, oi), (ym, yi) = med[name + "/list"], med[name + "/loop"], med[name + "/ylist"]
        lines.append("  %-28s %12.4f %7.4f | %15.4f %7.4f | %9.2f | %17.4f %7.4f | %28.1f %% | %7d %6d %7d"
                     % (name, lm, li, om, oi, om / lm, ym, yi, 100.0 * (lm - ym) / ym, p.batched_items, p.single_items, p.atlases))
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
