#!/usr/bin/env python
"""What a LIST of rectangles of a planar / semi-planar YUV frame costs: 3840x2160 -> 7680x4320, NV12 and P010, bicubic, strict
mode, srcnn_yuv_upscale_rect_list_dev (include/srcnn_amd_yuv_rect_list.h) against the loop of srcnn_yuv_upscale_rect_dev over the
same rects and against srcnn_y_path_rect_list_f32_dev over the same rects of a float Y plane.

  the lists   256 rects of 32x32, 64 of 64x64, 16 of 256x256, 4 of 960x512 (the lists of tools/rect_list_probe.py: seeded
              positions, every eighth on a border; origins moved down to even, as 4:2:0 demands, sizes kept).  Per list and format:
                (a) list    one srcnn_yuv_upscale_rect_list_dev call, every item with tight destination planes of its own
                (b) loop    n srcnn_yuv_upscale_rect_dev calls into the same destinations
                (c) Y list  one srcnn_y_path_rect_list_f32_dev call over the float Y plane of the frame
              reported: (b) / (a), and the colour cost ((a) - (c)) / (c)

Before anything is timed every item of (a) is compared with (b), byte for byte; a difference ends the probe with exit code 1.
Device-event medians of N calls (default 20) after 3 warm-up rounds, the candidates rotated on one stream so that a clock
drift hits all alike; the IQR beside every median.

Usage: python tools/yuv_rect_list_probe.py [--calls N] [--commit TEXT] [--out FILE]   (profiles/yuv_rect_list_probe.txt is its output)
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import libsrcnn_amd as S
from libsrcnn_amd import build
from rect_list_probe import DH, DW, H, LISTS, W, commit_text, positions, stats

FORMATS = [("NV12", 8, 0), ("P010", 10, 1)]          # semi-planar 4:2:0: name, depth, msb_aligned


class Bench:
    def __init__(self, calls):
        S.init(0)
        S.set_mode(S.MODE_STRICT)
        self.calls = calls
        rng = np.random.default_rng(20240917)
        # smooth content with noise on top, as video is neither flat nor white noise
        yy, xx = np.mgrid[0:H, 0:W].astype(np.float32)
        y8 = np.clip(127 + 100 * np.sin(xx / 97) * np.cos(yy / 61) + rng.integers(-20, 21, (H, W)), 0, 255).astype(np.uint16)
        cy, cx = np.mgrid[0:H // 2, 0:W // 2].astype(np.float32)
        uv8 = np.stack([np.clip(128 + 90 * np.sin(cx / 53 + k) * np.cos(cy / 41 - k) + rng.integers(-10, 11, (H // 2, W // 2)), 0, 255) for k in (0, 1)],
                       axis=-1).astype(np.uint16).reshape(H // 2, W)
        self.fmt, self.src, self.bps = {}, {}, {}
        for name, depth, msb in FORMATS:
            dt, shift = (np.uint8, 0) if depth == 8 else (np.uint16, (depth - 8) + (16 - depth if msb else 0))
            self.fmt[name] = S.yuv_format("semiplanar", "420", depth, msb)
            self.src[name] = [S.DeviceBuffer.from_numpy(np.ascontiguousarray((p << shift).astype(dt))) for p in (y8, uv8)] + [None]
            self.bps[name] = np.dtype(dt).itemsize
        self.d_y = S.DeviceBuffer.from_numpy(np.ascontiguousarray(y8, np.float32))
        self.st = S.Stream()
        self.ev = [S.Event(), S.Event()]
        self.bufs = {}

    def layout(self, key, rects, bps):
        """Per item (luma offset, chroma offset) in one buffer; bps == 0: one float plane per item."""
        offs, total = [], 0
        for (_, _, rw, rh) in rects:
            o_y = total
            total += ((bps or 4) * rw * rh + 15) & ~15
            o_c = total
            if bps:
                total += (bps * 2 * ((rw + 1) // 2) * ((rh + 1) // 2) + 15) & ~15
            offs.append((o_y, o_c))
        return self.bufs.setdefault(key, S.DeviceBuffer(total)), offs

    def list_call(self, f, name, rects):
        buf, offs = self.layout("%s/%s/list" % (f, name), rects, self.bps[f])
        arr, _ = S.yuv_rect_items([(x0, y0, rw, rh, [(buf, oy), (buf, oc)], None) for (x0, y0, rw, rh), (oy, oc) in zip(rects, offs)])
        return lambda: S.yuv_upscale_rect_list_dev(self.fmt[f], W, H, 2.0, S.SRCNNF_Bicubic, self.src[f], None, arr, self.st)

    def loop_call(self, f, name, rects):
        buf, offs = self.layout("%s/%s/loop" % (f, name), rects, self.bps[f])

        def run():
            for (x0, y0, rw, rh), (oy, oc) in zip(rects, offs):
                S.yuv_upscale_rect_dev(self.fmt[f], W, H, 2.0, S.SRCNNF_Bicubic, self.src[f], None, x0, y0, rw, rh, [(buf, oy), (buf, oc), None], None, self.st)
        return run

    def y_list_call(self, name, rects):
        buf, offs = self.layout(name + "/ylist", rects, 0)
        arr, _ = S.rect_items([(x0, y0, rw, rh, (buf, o), 0) for (x0, y0, rw, rh), (o, _) in zip(rects, offs)])
        return lambda: S.y_path_rect_list_dev(self.d_y, 0, W, H, DW, DH, S.SRCNNF_Bicubic, arr, self.st)

    def same_bytes(self, f, name, rects):
        """every item of the list call against the loop of single calls, byte for byte (the gaps between items hold nothing)"""
        self.list_call(f, name, rects)()
        self.loop_call(f, name, rects)()
        self.st.sync()
        bps = self.bps[f]
        (a, offs), (b, _) = self.layout("%s/%s/list" % (f, name), rects, bps), self.layout("%s/%s/loop" % (f, name), rects, bps)
        fa, fb = a.to_numpy(np.uint8, (a.nbytes,)), b.to_numpy(np.uint8, (b.nbytes,))
        ok = True
        for (_, _, rw, rh), (oy, oc) in zip(rects, offs):
            ny, nc = bps * rw * rh, bps * 2 * ((rw + 1) // 2) * ((rh + 1) // 2)
            ok = ok and np.array_equal(fa[oy:oy + ny], fb[oy:oy + ny]) and np.array_equal(fa[oc:oc + nc], fb[oc:oc + nc])
        return bool(ok)

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
    lists = [(name, [(x0 & ~1, y0 & ~1, rw, rh) for (x0, y0, rw, rh) in positions(1000 + k, n, rw, rh)]) for k, (name, n, rw, rh) in enumerate(LISTS)]
    names = [f for f, _, _ in FORMATS]
    same = {(f, name): b.same_bytes(f, name, rects) for f in names for name, rects in lists}
    if not all(same.values()):
        print("the list call and the loop of single calls differ: %r" % same)
        return 1
    calls = []
    for name, rects in lists:
        for f in names:
            calls += [("%s/%s/list" % (f, name), b.list_call(f, name, rects)), ("%s/%s/loop" % (f, name), b.loop_call(f, name, rects))]
        calls += [(name + "/ylist", b.y_list_call(name, rects))]
    med = {k: stats(v) for k, v in b.measure(calls).items()}
    plans = {(f, name): S.yuv_upscale_rect_list_plan(b.fmt[f], W, H, 2.0, S.SRCNNF_Bicubic, rects) for f in names for name, rects in lists}
    b.st.destroy()
    lines = ["yuv_rect_list_probe: %s, strict mode, %d timed calls each after 3 warm-up rounds, %dx%d -> %dx%d, NV12 and P010, bicubic, rotated on one stream"
             % (S.device_name(), a.calls, W, H, DW, DH),
             "commit: %s    source digest: %s" % (commit_text(a.commit), build.source_digest()[:16]),
             "every item of every list call equals the loop of single calls, byte for byte (checked before timing): True",
             "device events, ms per call           (a) list median  IQR | (b) loop median     IQR | (b) / (a) | (c) Y list median  IQR | colour cost ((a) - (c)) / (c) | batched single atlases"]
    for name, _ in lists:
        for f in names:
            p = plans[(f, name)]
            (lm, li), (om, oi), (ym, yi) = med["%s/%s/list" % (f, name)], med["%s/%s/loop" % (f, name)], med[name + "/ylist"]
            lines.append("  %-4s %-28s %12.4f %7.4f | %15.4f %7.4f | %9.2f | %17.4f %7.4f | %28.1f %% | %7d %6d %7d"
                         % (f, name, lm, li, om, oi, om / lm, ym, yi, 100.0 * (lm - ym) / ym, p.batched_items, p.single_items, p.atlases))
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
