#!/usr/bin/env python3
"""What upscaling ONLY WHAT CHANGED costs: 3840x2160 -> 7680x4320, bicubic, strict mode, srcnn_y_path_delta_f32_dev (default
64x64 tiles, SRCNN_DELTA_WHOLE_PERMILLE=1000) against the whole-frame call on the same frames in the same run.

  kernel    k_delta_flags alone (srcnn_y_path_delta_flags_dev), device events: nothing changed, 256 scattered samples changed,
            every sample changed.  Each timed round is one launch on each of 8 different pairs of planes (531 MB, twice the
            Infinity Cache, so the planes come from HBM), divided by 8; and, stated apart, the same pair over and over (cache-warm).
            Its floor is 8 * w * h bytes at the 5.2 - 5.5 TB/s the project's conversion kernels reach
            (profiles/yuv_kernel_trace.txt); the ratio is reported, it is not a pass mark.
  cases     the whole delta call on the HOST clock, from the call to the end of a stream synchronise (the call itself waits for
            the flags): nothing changed (the fixed cost: kernel, copy, one synchronise), one 32x32 source block changed, 256
            scattered samples changed; the whole-frame call in the same rotation.
  crossover 10, 25, 40, 55, 70, 85 and 100 % of the tiles dirty, as a seeded random tile set and as one contiguous block (the
            centre source sample of every chosen tile is changed: it lies in that tile's source rectangle alone), the delta call
            against the whole frame.  The default of SRCNN_DELTA_WHOLE_PERMILLE is the largest measured cell_samples / (dw * dh)
            at which the list route still beats the whole frame by more than the two IQRs together, rounded down to 50 permille,
            never below 500.
  bits      for every case a digest of the output plane after the delta route (from the previous frame's Y path) against a digest
            after the whole-frame route.

All calls of a group run on one stream, rotated call by call, after 3 warm-up rounds (median and IQR of --calls).

Usage: python tools/delta_probe.py [--calls N] [--commit TEXT] [--out FILE]      (profiles/delta_probe.txt is its output)
"""
import argparse
import hashlib
import os
import subprocess
import sys
import time

import numpy as np

os.environ["SRCNN_DELTA_WHOLE_PERMILLE"] = "1000"      # read when the library loads: the probe measures the list route up to the frame

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import libsrcnn_amd as S  # noqa: E402
from libsrcnn_amd import build, synth  # noqa: E402

W, H = 3840, 2160
DW, DH = 2 * W, 2 * H
TILE = 64
FRACTIONS = [10, 25, 40, 55, 70, 85, 100]
FLOOR_RATES = (5.2e12, 5.5e12)
PAIRS = 8


def commit_text(given):
    if given:
        return given
    try:
        return subprocess.run(["git", "-C", ROOT, "rev-parse", "HEAD"], capture_output=True, text=True, check=True).stdout.strip()
    except (OSError, subprocess.CalledProcessError):
        return "unknown (no git here)"


def stats(v):
    v = np.array(v)
    return float(np.median(v)), float(np.percentile(v, 75) - np.percentile(v, 25))


def flip(plane, xs, ys):
    out = plane.copy()
    out.view(np.uint32)[ys, xs] ^= 1
    return out


def tile_centres(tiles, cols):
    """The source sample in the middle of output tile k = r * cols + c (2x, 64x64 tiles): in that tile's source rectangle alone."""
    t = np.asarray(tiles)
    c, r = t % cols, t // cols
    return np.minimum(c * (TILE // 2) + TILE // 4, W - 1), np.minimum(r * (TILE // 2) + TILE // 4, H - 1)


def cases(base, cols, rows):
    """[(group, name, cur plane)]"""
    rng = np.random.default_rng(20261)
    out = [("cases", "nothing changed", base.copy())]
    blk = base.copy()
    blk.view(np.uint32)[1000:1032, 2000:2032] ^= 1
    out.append(("cases", "one 32x32 source block", blk))
    out.append(("cases", "256 scattered samples", flip(base, rng.integers(0, W, 256), rng.integers(0, H, 256))))
    n = cols * rows
    for f in FRACTIONS:
        k = n if f == 100 else int(round(n * f / 100.0))
        out.append(("crossover", "%3d %% random tiles" % f, flip(base, *tile_centres(rng.permutation(n)[:k], cols))))
        bc, br = max(1, int(round(cols * (f / 100.0) ** 0.5))), max(1, int(round(rows * (f / 100.0) ** 0.5)))
        if f == 100:
            bc, br = cols, rows
        c0, r0 = (cols - bc) // 2, (rows - br) // 2
        block = [(r0 + r) * cols + (c0 + c) for r in range(br) for c in range(bc)]
        out.append(("crossover", "%3d %% one block" % f, flip(base, *tile_centres(block, cols))))
    return out


class Bench:
    def __init__(self, calls):
        S.init(0)
        S.set_mode(S.MODE_STRICT)
        assert "SRCNN_DELTA_WHOLE_PERMILLE=1000" in S.debug_settings()
        self.calls = calls
        self.st = S.Stream()
        self.ev = [S.Event(), S.Event()]

    def rotate(self, calls, timed):
        series = {k: [] for k, _ in calls}
        for _ in range(3):
            for key, fn in calls:
                timed(fn)
        n = len(calls)
        for k in range(self.calls):
            for key, fn in calls[k % n:] + calls[:k % n]:
                series[key].append(timed(fn))
        return {k: stats(v) for k, v in series.items()}

    def device_ms(self, fn):
        self.st.sync()
        self.ev[0].record(self.st)
        fn()
        self.ev[1].record(self.st)
        self.st.sync()
        return self.ev[0].elapsed_ms(self.ev[1])

    def host_ms(self, fn):
        self.st.sync()
        t0 = time.perf_counter()
        fn()
        self.st.sync()
        return (time.perf_counter() - t0) * 1e3


def digest(buf):
    return hashlib.sha256(buf.to_numpy(np.uint8, (buf.nbytes,)).tobytes()).hexdigest()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--commit", default=None, help="what to record as the commit (default: git rev-parse HEAD)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.calls < 10:
        ap.error("--calls: at least 10 timed calls")
    b = Bench(a.calls)
    L = S.lib()
    cols, rows = S.y_path_delta_grid(W, H, DW, DH, S.SRCNNF_Bicubic)
    base = synth.plane(H, W, synth.SEED0 + 3, "smooth")
    d_prev = S.DeviceBuffer.from_numpy(base)
    d_out = S.DeviceBuffer(4 * DW * DH)
    d_whole = S.DeviceBuffer(4 * DW * DH)
    lines = ["delta_probe: %s, strict mode, %d timed calls each after 3 warm-up rounds, %dx%d -> %dx%d, bicubic, %dx%d tiles (%d x %d), rotated on one stream"
             % (S.device_name(), a.calls, W, H, DW, DH, TILE, TILE, cols, rows),
             "commit: %s    source digest: %s    SRCNN_DELTA_WHOLE_PERMILLE=1000" % (commit_text(a.commit), build.source_digest()[:16])]

    # ---- the kernel alone ----
    rng = np.random.default_rng(20262)
    d_flags = S.DeviceBuffer(cols * rows)
    kinds = [("nothing changed", lambda p: p.copy()),
             ("256 scattered samples", lambda p: flip(p, rng.integers(0, W, 256), rng.integers(0, H, 256))),
             ("every sample changed", lambda p: (p.view(np.uint32) ^ 1).view(np.float32))]
    pairs = {name: [] for name, _ in kinds}
    prevs = []
    for k in range(PAIRS):
        p = synth.plane(H, W, synth.SEED0 + 100 + k, "smooth")
        prevs.append(S.DeviceBuffer.from_numpy(p))
        for name, make in kinds[:2]:
            pairs[name].append((prevs[k], S.DeviceBuffer.from_numpy(make(p))))
    every = S.DeviceBuffer.from_numpy(kinds[2][1](base))
    pairs["every sample changed"] = [(d_prev, every)]                 # (one pair: cache-warm only)

    def flags_call(plist):
        def run():
            for (p, c) in plist:
                S.y_path_delta_flags_dev(p, 0, c, 0, W, H, DW, DH, S.SRCNNF_Bicubic, (0, 0), d_flags, b.st)
        return run
    kcalls = [(name + " / 8 pairs", flags_call(pairs[name])) for name, _ in kinds[:2]]
    kcalls += [(name + " / warm", flags_call(pairs[name][:1] * PAIRS)) for name, _ in kinds]
    kmed = b.rotate(kcalls, b.device_ms)
    nbytes = 8.0 * W * H
    floor_us = [nbytes / r * 1e6 for r in FLOOR_RATES]
    lines.append("k_delta_flags alone, device events around %d launches, per launch; floor: %.1f MB at %.1f - %.1f TB/s = %.1f - %.1f us"
                 % (PAIRS, nbytes / 1e6, FLOOR_RATES[0] / 1e12, FLOOR_RATES[1] / 1e12, floor_us[0], floor_us[1]))
    lines.append("  %-44s %10s %8s %10s %14s" % ("", "median us", "IQR us", "TB/s", "time / floor"))
    for key, _ in kcalls:
        m, i = kmed[key]
        us = m * 1e3 / PAIRS
        lines.append("  %-44s %10.2f %8.2f %10.2f %8.2f - %.2f" % (key, us, i * 1e3 / PAIRS, nbytes / (us * 1e-6) / 1e12, us / floor_us[0], us / floor_us[1]))
    del pairs, prevs, every

    # ---- the whole call ----
    todo = cases(base, cols, rows)
    d_cur = {name: S.DeviceBuffer.from_numpy(cur) for _, name, cur in todo}
    st_of = {}

    def delta_call(name):
        def run():
            st_of[name] = S.y_path_delta_dev(d_prev, 0, d_cur[name], 0, W, H, DW, DH, S.SRCNNF_Bicubic, (0, 0), d_out, 0, b.st)
        return run

    def whole_call(name):
        return lambda: S.check(L.srcnn_y_upscale2x_f32_dev(d_cur[name].ptr, W, H, d_whole.ptr, b.st.handle))
    S.check(L.srcnn_y_upscale2x_f32_dev(d_prev.ptr, W, H, d_out.ptr, b.st.handle))
    b.st.sync()
    med = {}
    for group in ("cases", "crossover"):
        names = [name for g, name, _ in todo if g == group]
        calls = [("whole", whole_call(names[0]))]
        for name in names:
            calls.append((name, delta_call(name)))
        m = b.rotate(calls, b.host_ms)
        med[group + "/whole"] = m.pop("whole")
        med.update(m)

    # ---- bits: the delta route from Y(prev) against the whole-frame route, case by case ----
    same = {}
    for _, name, _ in todo:
        S.check(L.srcnn_y_upscale2x_f32_dev(d_prev.ptr, W, H, d_out.ptr, b.st.handle))
        b.st.sync()
        delta_call(name)()
        whole_call(name)()
        b.st.sync()
        same[name] = digest(d_out) == digest(d_whole)

    frame = float(DW) * DH
    for group in ("cases", "crossover"):
        wm, wi = med[group + "/whole"]
        lines.append("%s, host clock from the call to the end of a stream synchronise, ms; whole frame in the same rotation: median %.4f, IQR %.4f"
                     % (group, wm, wi))
        lines.append("  %-26s %10s %8s %9s %7s %7s %6s %6s %13s %8s %6s" % ("", "median", "IQR", "whole/it", "tiles", "dirty", "rects", "whole", "cell_samples", "/ dw*dh", "bits"))
        for g, name, _ in todo:
            if g != group:
                continue
            m, i = med[name]
            s = st_of[name]
            lines.append("  %-26s %10.4f %8.4f %9.2f %7d %7d %6d %6d %13d %8.3f %6s"
                         % (name, m, i, wm / m, s.tiles, s.dirty_tiles, s.rects, s.whole_frame, s.cell_samples, s.cell_samples / frame, "same" if same[name] else "DIFFER"))
    wm, wi = med["crossover/whole"]
    best = None
    for g, name, _ in todo:
        s = st_of[name]
        if g == "crossover" and not s.whole_frame and wm - med[name][0] > wi + med[name][1]:
            best = max(best or 0.0, s.cell_samples / frame)
    if best is None:
        lines.append("crossover: the list route beat the whole frame by more than both IQRs in no measured case: SRCNN_DELTA_WHOLE_PERMILLE stays at 1000")
    else:
        lines.append("crossover: the list route still beats the whole frame by more than both IQRs at cell_samples / (dw * dh) = %.3f: "
                     "SRCNN_DELTA_WHOLE_PERMILLE = %d (rounded down to 50, never below 500, at most 1000)" % (best, min(1000, max(500, int(best * 1000) // 50 * 50))))
    ok = all(same.values())
    lines.append("every delta route holds the whole-frame route's bits: %s" % ok)
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
