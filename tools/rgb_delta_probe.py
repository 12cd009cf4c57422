#!/usr/bin/env python3
"""What upscaling ONLY WHAT CHANGED costs for RGB(A) images: 3840x2160 -> 7680x4320, bicubic, strict mode,
srcnn_rgb_upscale_delta_dev (default 64x64 tiles, SRCNN_DELTA_WHOLE_PERMILLE=1000) against the whole-image call
srcnn_rgb_upscale_dev on the same images in the same run, for 8-bit interleaved RGB and 8-bit interleaved BGRA.  The protocol is
that of tools/delta_probe.py.

  kernel    k_delta_flags_bytes alone (srcnn_rgb_delta_flags_dev), device events: nothing changed and 256 scattered pixels
            changed, each timed round one launch on each of 8 different pairs of images (every case its own buffers: from HBM, not from the
            Infinity Cache),
            divided by 8; the same pair over and over (cache-warm), every byte changed.  k_delta_flags on 8 pairs of float planes
            of the same size runs in the same rotation: the byte kernel's floor is the bytes of both images at the bandwidth the
            float kernel reaches there.  The ratio is reported, it is not a pass mark.
  cases     the whole delta call on the HOST clock, from the call to the end of a stream synchronise: nothing changed (the fixed
            cost), one 32x32 block changed, 256 scattered pixels changed; the whole-image call and srcnn_y_path_delta_f32_dev on the
            float Y plane of the same images in the same rotation.  THE PASS MARK: the RGB8 call on an unchanged image takes at
            most 2 x the Y call on an unchanged plane.
  crossover 10 ... 100 % of the tiles dirty, as a seeded random tile set and as one contiguous block (the centre pixel of every
            chosen tile is changed), the delta call against the whole image; the share that tools/delta_probe.py's rule gives.
  bytes     for every case a digest of dst after the delta route (from the previous image's result) against a digest after the
            whole-image route.

Usage: python tools/rgb_delta_probe.py [--calls N] [--commit TEXT] [--out FILE]      (profiles/rgb_delta_probe.txt is its output)
"""
import argparse
import os
import sys

import numpy as np

os.environ["SRCNN_DELTA_WHOLE_PERMILLE"] = "1000"      # read when the library loads: the probe measures the list route up to the frame

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import delta_probe as DP  # noqa: E402  (Bench, stats, digest, tile_centres, commit_text: one protocol)
import libsrcnn_amd as S  # noqa: E402
from libsrcnn_amd import build, synth  # noqa: E402

W, H, DW, DH, TILE, PAIRS, FRACTIONS = DP.W, DP.H, DP.DW, DP.DH, DP.TILE, DP.PAIRS, DP.FRACTIONS
FORMATS = [("RGB8", "rgb", 0), ("BGRA8", "bgr", 1)]


def base_image(c):
    """(H, W, c) uint8, image-like: one smooth synthetic plane per channel."""
    return np.stack([synth.plane(H, W, synth.SEED0 + 40 + k, "smooth").astype(np.uint8) for k in range(c)], axis=-1)


def luma(img):
    f = img[..., :3].astype(np.float32)
    return np.ascontiguousarray(np.float32(0.299) * f[..., 0] + np.float32(0.587) * f[..., 1] + np.float32(0.114) * f[..., 2])


def flip(img, xs, ys):
    out = img.copy()
    out[ys, xs, 1] ^= 0x20          # (G: the luma plane of the comparison changes with it)
    return out


def cases(base, cols, rows):
    """[(group, name, cur image)]"""
    rng = np.random.default_rng(20261)
    out = [("cases", "nothing changed", base.copy())]
    blk = base.copy()
    blk[1000:1032, 2000:2032, 1] ^= 0x20
    out.append(("cases", "one 32x32 block", blk))
    out.append(("cases", "256 scattered pixels", flip(base, rng.integers(0, W, 256), rng.integers(0, H, 256))))
    n = cols * rows
    for f in FRACTIONS:
        k = n if f == 100 else int(round(n * f / 100.0))
        out.append(("crossover", "%3d %% random tiles" % f, flip(base, *DP.tile_centres(rng.permutation(n)[:k], cols))))
        bc, br = max(1, int(round(cols * (f / 100.0) ** 0.5))), max(1, int(round(rows * (f / 100.0) ** 0.5)))
        if f == 100:
            bc, br = cols, rows
        c0, r0 = (cols - bc) // 2, (rows - br) // 2
        block = [(r0 + r) * cols + (c0 + c) for r in range(br) for c in range(bc)]
        out.append(("crossover", "%3d %% one block" % f, flip(base, *DP.tile_centres(block, cols))))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--commit", default=None, help="what to record as the commit (default: git rev-parse HEAD)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.calls < 10:
        ap.error("--calls: at least 10 timed calls")
    b = DP.Bench(a.calls)
    filt = S.SRCNNF_Bicubic
    dw, dh, cols, rows = S.rgb_delta_grid(W, H, 2.0, filt)
    assert (dw, dh) == (DW, DH)
    lines = ["rgb_delta_probe: %s, strict mode, %d timed calls each after 3 warm-up rounds, %dx%d -> %dx%d, bicubic, %dx%d tiles (%d x %d), rotated on one stream"
             % (S.device_name(), a.calls, W, H, DW, DH, TILE, TILE, cols, rows),
             "commit: %s    source digest: %s    SRCNN_DELTA_WHOLE_PERMILLE=1000" % (DP.commit_text(a.commit), build.source_digest()[:16])]
    ok, mark = True, None
    d_flags = S.DeviceBuffer(cols * rows)
    frame = float(DW) * DH

    for fname, order, alpha in FORMATS:
        c = 3 + alpha
        fmt = S.rgb_format("interleaved", order, alpha, 8)
        nbytes = 2.0 * c * W * H
        # ---- the kernel alone, with the float kernel on planes of the same size in the same rotation ----
        rng = np.random.default_rng(20262 + c)
        same, scat, fl = [], [], []
        for k in range(PAIRS):
            p = rng.integers(0, 256, (H, W, c), dtype=np.uint8)
            dp = S.DeviceBuffer.from_numpy(p)
            same.append((dp, S.DeviceBuffer.from_numpy(p)))
            scat.append((S.DeviceBuffer.from_numpy(p), S.DeviceBuffer.from_numpy(flip(p, rng.integers(0, W, 256), rng.integers(0, H, 256)))))
            y = synth.plane(H, W, synth.SEED0 + 100 + k, "noise")
            fl.append((S.DeviceBuffer.from_numpy(y), S.DeviceBuffer.from_numpy(y)))
        every = [(same[0][0], S.DeviceBuffer.from_numpy(same[0][0].to_numpy(np.uint8, (H, W, c)) ^ 0xff))]

        def bytes_call(plist):
            def run():
                for (p, q) in plist:
                    S.rgb_delta_flags_dev(fmt, W, H, 2.0, filt, [p], None, [q], None, (0, 0), d_flags, b.st)
            return run

        def float_call(plist):
            def run():
                for (p, q) in plist:
                    S.y_path_delta_flags_dev(p, 0, q, 0, W, H, DW, DH, filt, (0, 0), d_flags, b.st)
            return run
        kcalls = [("float plane (k_delta_flags), nothing changed / 8 pairs", float_call(fl)),
                  ("nothing changed / 8 pairs", bytes_call(same)), ("256 scattered pixels / 8 pairs", bytes_call(scat)),
                  ("nothing changed / warm", bytes_call(same[:1] * PAIRS)), ("256 scattered pixels / warm", bytes_call(scat[:1] * PAIRS)),
                  ("every byte changed / warm", bytes_call(every * PAIRS))]
        print("%s: the kernel alone ..." % fname, file=sys.stderr, flush=True)
        kmed = b.rotate(kcalls, b.device_ms)
        f_us = kmed[kcalls[0][0]][0] * 1e3 / PAIRS
        f_rate = 8.0 * W * H / (f_us * 1e-6)
        floor_us = nbytes / f_rate * 1e6
        lines.append("%s: k_delta_flags_bytes alone, device events around %d launches, per launch; k_delta_flags on float planes in the same rotation: %.2f us, %.2f TB/s;"
                     " floor: %.1f MB at that rate = %.2f us" % (fname, PAIRS, f_us, f_rate / 1e12, nbytes / 1e6, floor_us))
        lines.append("  %-56s %10s %8s %10s %14s" % ("", "median us", "IQR us", "TB/s", "time / floor"))
        for key, _ in kcalls:
            m, i = kmed[key]
            us = m * 1e3 / PAIRS
            nb = 8.0 * W * H if key.startswith("float") else nbytes
            lines.append("  %-56s %10.2f %8.2f %10.2f %14.2f" % (key, us, i * 1e3 / PAIRS, nb / (us * 1e-6) / 1e12, us / (nb / f_rate * 1e6)))
        del same, scat, fl, every

        # ---- the whole call ----
        base = base_image(c)
        todo = cases(base, cols, rows)
        d_prev = S.DeviceBuffer.from_numpy(base)
        d_cur = {name: S.DeviceBuffer.from_numpy(cur) for _, name, cur in todo}
        d_out, d_whole = S.DeviceBuffer(c * DW * DH), S.DeviceBuffer(c * DW * DH)
        y_prev = S.DeviceBuffer.from_numpy(luma(base))
        y_cur = {name: S.DeviceBuffer.from_numpy(luma(cur)) for g, name, cur in todo if g == "cases"}
        y_out = S.DeviceBuffer(4 * DW * DH)
        st_of = {}

        def delta_call(name):
            def run():
                st_of[name] = S.rgb_upscale_delta_dev(fmt, W, H, 2.0, filt, [d_prev], None, [d_cur[name]], None, (0, 0), [d_out], None, None, 0, b.st)
            return run

        def y_call(name):
            def run():
                st_of["Y: " + name] = S.y_path_delta_dev(y_prev, 0, y_cur[name], 0, W, H, DW, DH, filt, (0, 0), y_out, 0, b.st)
            return run

        def whole_call(name, dst):
            return lambda: S.rgb_upscale_dev(fmt, W, H, 2.0, filt, [d_cur[name]], None, [dst], None, None, 0, b.st)
        S.rgb_upscale_dev(fmt, W, H, 2.0, filt, [d_prev], None, [d_out], None, None, 0, b.st)
        S.check(S.lib().srcnn_y_upscale2x_f32_dev(y_prev.ptr, W, H, y_out.ptr, b.st.handle))
        b.st.sync()
        med = {}
        for group in ("cases", "crossover"):
            names = [name for g, name, _ in todo if g == group]
            calls = [("whole", whole_call(names[0], d_whole))]
            for name in names:
                calls.append((name, delta_call(name)))
                if group == "cases":
                    calls.append(("Y: " + name, y_call(name)))
            print("%s: %s ..." % (fname, group), file=sys.stderr, flush=True)
            m = b.rotate(calls, b.host_ms)
            med[group + "/whole"] = m.pop("whole")
            med.update(m)

        # ---- bytes: the delta route from the previous image's result against the whole-image route, case by case ----
        same_bytes = {}
        for _, name, _ in todo:
            S.rgb_upscale_dev(fmt, W, H, 2.0, filt, [d_prev], None, [d_out], None, None, 0, b.st)
            b.st.sync()
            delta_call(name)()
            whole_call(name, d_whole)()
            b.st.sync()
            same_bytes[name] = DP.digest(d_out) == DP.digest(d_whole)

        for group in ("cases", "crossover"):
            wm, wi = med[group + "/whole"]
            lines.append("%s: %s, host clock from the call to the end of a stream synchronise, ms; whole image (srcnn_rgb_upscale_dev) in the same rotation: median %.4f, IQR %.4f"
                         % (fname, group, wm, wi))
            lines.append("  %-30s %10s %8s %9s %7s %7s %6s %6s %13s %8s %6s" % ("", "median", "IQR", "whole/it", "tiles", "dirty", "rects", "whole", "cell_samples", "/ dw*dh", "bytes"))
            for g, name, _ in todo:
                if g != group:
                    continue
                for key in ([name, "Y: " + name] if group == "cases" else [name]):
                    m, i = med[key]
                    s = st_of[key]
                    lines.append("  %-30s %10.4f %8.4f %9.2f %7d %7d %6d %6d %13d %8.3f %6s"
                                 % (key, m, i, wm / m, s.tiles, s.dirty_tiles, s.rects, s.whole_frame, s.cell_samples, s.cell_samples / frame,
                                    "-" if key.startswith("Y: ") else ("same" if same_bytes[name] else "DIFFER")))
        rgb0, y0 = med["nothing changed"][0], med["Y: nothing changed"][0]
        lines.append("%s: unchanged image %.4f ms, unchanged float Y plane %.4f ms in the same rotation: %.2f x" % (fname, rgb0, y0, rgb0 / y0))
        if fname == "RGB8":
            mark = rgb0 <= 2.0 * y0
            lines.append("pass mark (the RGB8 call on an unchanged image takes at most 2 x the Y call on an unchanged plane): %s" % ("met" if mark else "MISSED"))
        wm, wi = med["crossover/whole"]
        best = None
        for g, name, _ in todo:
            s = st_of[name]
            if g == "crossover" and not s.whole_frame and wm - med[name][0] > wi + med[name][1]:
                best = max(best or 0.0, s.cell_samples / frame)
        if best is None:
            lines.append("%s: crossover: the list route beat the whole image by more than both IQRs in no measured case" % fname)
        else:
            lines.append("%s: crossover: the list route still beats the whole image by more than both IQRs at cell_samples / (dw * dh) = %.3f: "
                         "%d permille (rounded down to 50, never below 500, at most 1000)" % (fname, best, min(1000, max(500, int(best * 1000) // 50 * 50))))
        ok = ok and all(same_bytes.values())
        del d_cur, d_out, d_whole, y_cur
    lines.append("every delta route holds the whole-image route's bytes: %s" % ok)
    b.st.destroy()
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
