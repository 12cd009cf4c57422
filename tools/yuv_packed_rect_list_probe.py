#!/usr/bin/env python
"""What a LIST of rectangles of a packed YUV frame costs: 3840x2160 -> 7680x4320, YUY2, Y210, Y410 and v210, bicubic, strict mode,
srcnn_yuv_packed_upscale_rect_list_dev (include/srcnn_amd_yuv_packed_rect_list.h) against the loop of
srcnn_yuv_packed_upscale_rect_dev over the same rects and against srcnn_y_path_rect_list_f32_dev over the same rects of a float
Y plane.

  the lists   256 rects of 32x32, 64 of 64x64, 16 of 256x256, 4 of 960x512 (the lists of tools/rect_list_probe.py: seeded
              positions, every eighth on a border; origins moved down to a multiple of 6, which is unit-aligned in every format;
              for v210 the width is rounded up to its unit of 6 pixels -- 36, 66, 258, 960 -- and the Y list of column (c) runs
              those rects).  Per list and format:
                (a) list    one srcnn_yuv_packed_upscale_rect_list_dev call, every item with tight row segments of its own
                (b) loop    n srcnn_yuv_packed_upscale_rect_dev calls into the same destinations
                (c) Y list  one srcnn_y_path_rect_list_f32_dev call over the float Y plane of the frame
              reported: (b) / (a), and the cost of the colour shell ((a) - (c)) / (c)

Before anything is timed every item of (a) is compared with (b), byte for byte; a difference ends the probe with exit code 1.
Device-event medians of N calls (default 20) after 3 warm-up rounds, the candidates rotated on one stream so that a clock
drift hits all alike; the IQR beside every median.  Acceptance: for 256 x 32x32, (a) is below (b) by more than the sum of their
IQRs in every format; for 4 x 960x512, (a) is not above (b) by more than that sum.

Usage: python tools/yuv_packed_rect_list_probe.py [--calls N] [--commit TEXT] [--out FILE]   (profiles/yuv_packed_rect_list_probe.txt is its output)
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

FORMATS = ["yuy2", "y210", "y410", "v210"]


def pack(name, y, u, v):
    """8-bit planes (y: H x W; u, v: H x W/2 for the 4:2:2 formats, H x W for y410) -> the packed frame, H x row bytes uint8."""
    h, w = y.shape
    if name == "yuy2":
        f = np.empty((h, w // 2, 4), np.uint8)
        f[..., 0], f[..., 1], f[..., 2], f[..., 3] = y[:, 0::2], u, y[:, 1::2], v
    elif name == "y210":
        f = np.empty((h, w // 2, 4), np.uint16)
        f[..., 0], f[..., 1], f[..., 2], f[..., 3] = y[:, 0::2], u, y[:, 1::2], v
        f <<= 8                                              # 10 significant bits in the high bits of the word: (v8 << 2) << 6
    elif name == "y410":
        a = np.uint32(3)
        f = (u.astype(np.uint32) << 2) | (y.astype(np.uint32) << 12) | (v.astype(np.uint32) << 22) | (a << 30)
    else:                                                    # v210: Cb0 Y0 Cr0 | Y1 Cb1 Y2 | Cr1 Y3 Cb2 | Y4 Cr2 Y5, 10-bit fields
        assert w % 48 == 0
        Y = (y.astype(np.uint32) << 2).reshape(h, w // 6, 6)
        U = (u.astype(np.uint32) << 2).reshape(h, w // 6, 3)
        V = (v.astype(np.uint32) << 2).reshape(h, w // 6, 3)
        f = np.stack([U[..., 0] | (Y[..., 0] << 10) | (V[..., 0] << 20), Y[..., 1] | (U[..., 1] << 10) | (Y[..., 2] << 20),
                      V[..., 1] | (Y[..., 3] << 10) | (U[..., 2] << 20), Y[..., 4] | (V[..., 2] << 10) | (Y[..., 5] << 20)], axis=-1)
    return np.ascontiguousarray(f).view(np.uint8).reshape(h, -1)


def rects_for(name, k, n, rw, rh):
    """The list's rects under the format's unit rule: origins on a multiple of 6; v210: the width rounded up to 6."""
    if name == "v210":
        rw = -(-rw // 6) * 6
    out = []
    for (x0, y0, _rw, _rh) in positions(1000 + k, n, rw, rh):
        x0 = min(x0, DW - rw)
        out.append((x0 - x0 % 6, y0, rw, rh))
    return out


class Bench:
    def __init__(self, calls):
        S.init(0)
        S.set_mode(S.MODE_STRICT)
        self.calls = calls
        rng = np.random.default_rng(20241020)
        # smooth content with noise on top, as video is neither flat nor white noise
        yy, xx = np.mgrid[0:H, 0:W].astype(np.float32)
        y8 = np.clip(127 + 100 * np.sin(xx / 97) * np.cos(yy / 61) + rng.integers(-20, 21, (H, W)), 0, 255).astype(np.uint8)

        def chroma(cw):
            cy, cx = np.mgrid[0:H, 0:cw].astype(np.float32)
            return [np.clip(128 + 90 * np.sin(cx / 53 + k) * np.cos(cy / 41 - k) + rng.integers(-10, 11, (H, cw)), 0, 255).astype(np.uint8) for k in (0, 1)]
        half, full = chroma(W // 2), chroma(W)
        self.src = {}
        for name in FORMATS:
            u, v = full if name == "y410" else half
            frame = pack(name, y8, u, v)
            assert frame.shape == (H, S.yuv_packed_row_bytes(name, W)[0]), (name, frame.shape)
            self.src[name] = S.DeviceBuffer.from_numpy(frame)
        self.d_y = S.DeviceBuffer.from_numpy(np.ascontiguousarray(y8, np.float32))
        self.st = S.Stream()
        self.ev = [S.Event(), S.Event()]
        self.bufs = {}

    def layout(self, key, rects, name):
        """Per item its byte offset and the bytes of a row segment in one buffer; name None: one float plane per item."""
        offs, total = [], 0
        for (x0, _y0, rw, rh) in rects:
            n = 4 * rw if name is None else S.yuv_packed_span_bytes(name, DW, x0, rw)[2]
            offs.append((total, n))
            total += (n * rh + 15) & ~15
        return self.bufs.setdefault(key, S.DeviceBuffer(total)), offs

    def list_call(self, f, name, rects):
        buf, offs = self.layout("%s/%s/list" % (f, name), rects, f)
        arr, _ = S.yuv_packed_rect_items([(x0, y0, rw, rh, (buf, o), 0) for (x0, y0, rw, rh), (o, _n) in zip(rects, offs)])
        return lambda: S.yuv_packed_upscale_rect_list_dev(f, W, H, 2.0, S.SRCNNF_Bicubic, self.src[f], 0, arr, self.st)

    def loop_call(self, f, name, rects):
        buf, offs = self.layout("%s/%s/loop" % (f, name), rects, f)

        def run():
            for (x0, y0, rw, rh), (o, _n) in zip(rects, offs):
                S.yuv_packed_upscale_rect_dev(f, W, H, 2.0, S.SRCNNF_Bicubic, self.src[f], 0, x0, y0, rw, rh, (buf, o), 0, self.st)
        return run

    def y_list_call(self, key, rects):
        buf, offs = self.layout(key, rects, None)
        arr, _ = S.rect_items([(x0, y0, rw, rh, (buf, o), 0) for (x0, y0, rw, rh), (o, _n) in zip(rects, offs)])
        return lambda: S.y_path_rect_list_dev(self.d_y, 0, W, H, DW, DH, S.SRCNNF_Bicubic, arr, self.st)

    def same_bytes(self, f, name, rects):
        """every item of the list call against the loop of single calls, byte for byte (the gaps between items hold nothing)"""
        self.list_call(f, name, rects)()
        self.loop_call(f, name, rects)()
        self.st.sync()
        (a, offs), (b, _) = self.layout("%s/%s/list" % (f, name), rects, f), self.layout("%s/%s/loop" % (f, name), rects, f)
        fa, fb = a.to_numpy(np.uint8, (a.nbytes,)), b.to_numpy(np.uint8, (b.nbytes,))
        return bool(all(np.array_equal(fa[o:o + n * rh], fb[o:o + n * rh]) for (_, _, _, rh), (o, n) in zip(rects, offs)))

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
    lists = {f: [(name, rects_for(f, k, n, rw, rh)) for k, (name, n, rw, rh) in enumerate(LISTS)] for f in FORMATS}
    same = {(f, name): b.same_bytes(f, name, rects) for f in FORMATS for name, rects in lists[f]}
    if not all(same.values()):
        print("the list call and the loop of single calls differ: %r" % same)
        return 1
    calls = []
    for k, (name, _n, _rw, _rh) in enumerate(LISTS):
        for f in FORMATS:
            rects = lists[f][k][1]
            calls += [("%s/%s/list" % (f, name), b.list_call(f, name, rects)), ("%s/%s/loop" % (f, name), b.loop_call(f, name, rects))]
        calls += [("exact/%s/ylist" % name, b.y_list_call("exact/%s/ylist" % name, lists["yuy2"][k][1])),
                  ("v210/%s/ylist" % name, b.y_list_call("v210/%s/ylist" % name, lists["v210"][k][1]))]
    med = {k: stats(v) for k, v in b.measure(calls).items()}
    plans = {(f, name): S.yuv_packed_upscale_rect_list_plan(f, W, H, 2.0, S.SRCNNF_Bicubic, rects) for f in FORMATS for name, rects in lists[f]}
    b.st.destroy()
    lines = ["yuv_packed_rect_list_probe: %s, strict mode, %d timed calls each after 3 warm-up rounds, %dx%d -> %dx%d, YUY2 / Y210 / Y410 / v210, bicubic, rotated on one stream"
             % (S.device_name(), a.calls, W, H, DW, DH),
             "commit: %s    source digest: %s" % (commit_text(a.commit), build.source_digest()[:16]),
             "every item of every list call equals the loop of single calls, byte for byte (checked before timing): True",
             "origins on multiples of 6; v210 rects are 36, 66, 258 and 960 wide (its unit is 6 pixels), and its Y list runs those rects",
             "device events, ms per call           (a) list median  IQR | (b) loop median     IQR | (b) / (a) | (c) Y list median  IQR | colour shell ((a) - (c)) / (c) | batched single atlases"]
    verdict = []
    for name, _n, _rw, _rh in LISTS:
        for f in FORMATS:
            p = plans[(f, name)]
            (lm, li), (om, oi) = med["%s/%s/list" % (f, name)], med["%s/%s/loop" % (f, name)]
            ym, yi = med["%s/%s/ylist" % ("v210" if f == "v210" else "exact", name)]
            lines.append("  %-4s %-28s %12.4f %7.4f | %15.4f %7.4f | %9.2f | %17.4f %7.4f | %29.1f %% | %7d %6d %7d"
                         % (f, name, lm, li, om, oi, om / lm, ym, yi, 100.0 * (lm - ym) / ym, p.batched_items, p.single_items, p.atlases))
            if name == LISTS[0][0]:
                verdict.append(("%s %s: list below loop by more than the sum of the IQRs" % (f, name), om - lm > li + oi))
            if name == LISTS[-1][0]:
                verdict.append(("%s %s: list not above loop by more than the sum of the IQRs" % (f, name), lm - om <= li + oi))
    lines += ["acceptance: " + ("; ".join("%s: %s" % (t, "yes" if ok else "NO") for t, ok in verdict))]
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)
    return 0 if all(ok for _t, ok in verdict) else 2


if __name__ == "__main__":
    sys.exit(main())
