#!/usr/bin/env python3
"""What a LIST of rectangles of the output costs: 3840x2160 -> 7680x4320, bicubic, strict mode, srcnn_y_path_rect_list_f32_dev
against the loop of srcnn_y_path_rect_f32_dev over the same items in the same run.

  whole     srcnn_y_upscale2x_f32_dev, the whole frame
  lists     256 rects of 32x32, 64 of 64x64, 16 of 256x256, 4 of 960x512; positions seeded, a few on the borders
            list     one srcnn_y_path_rect_list_f32_dev call
            loop     srcnn_y_path_rect_f32_dev item by item: the yardstick, what a caller had to do before
            unfused  the list call under SRCNN_RECT_LIST_UNFUSED=1 (a child process: the switch is read when the library loads)
  sweep     16 rects of one size, 32x32 ... 1436x1436 (a cell just below 2^21 samples): the loop, the list call as routed by default, and the list call with the
            single-route threshold lifted (SRCNN_RECT_LIST_SINGLE_SAMPLES = 2^40, a child process) -- where the batched route
            stops paying is where SRCNN_RECT_LIST_SINGLE_SAMPLES belongs

All calls of a process run on one stream, rotated call by call, after 3 warm-up rounds; each is timed with device events around
the call (median and IQR of --calls).  The plan's cell_samples and atlas_samples are recorded per list.

Conditions (stated before measuring): for the 256 x (32x32) and the 64 x (64x64) list the list call is faster than the loop by
more than the two IQRs together; for 16 x (256x256) and 4 x (960x512) it is not slower than the loop by more than the loop's IQR,
whichever route the threshold sends them.  Every other number is reported, not gated.

Usage: python tools/rect_list_probe.py [--calls N] [--commit TEXT] [--out FILE]      (profiles/rect_list_probe.txt is its output)
"""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import libsrcnn_amd as S
from libsrcnn_amd import build, synth

W, H = 3840, 2160
DW, DH = 2 * W, 2 * H
LISTS = [("256 x 32x32", 256, 32, 32), ("64 x 64x64", 64, 64, 64), ("16 x 256x256", 16, 256, 256), ("4 x 960x512", 4, 960, 512)]
SWEEP = [32, 64, 128, 256, 384, 512, 768, 1024, 1280, 1436]


def commit_text(given):
    if given:
        return given
    try:
        return subprocess.run(["git", "-C", ROOT, "rev-parse", "HEAD"], capture_output=True, text=True, check=True).stdout.strip()
    except (OSError, subprocess.CalledProcessError):
        return "unknown (no git here)"


def positions(seed, n, rw, rh):
    """n seeded rects of rw x rh; every eighth lies on a border (left, top, right, bottom in turn)."""
    rng = np.random.default_rng(seed)
    out = []
    for k in range(n):
        x0, y0 = int(rng.integers(0, DW - rw + 1)), int(rng.integers(0, DH - rh + 1))
        if k % 8 == 0:
            x0, y0 = ((0, y0), (x0, 0), (DW - rw, y0), (x0, DH - rh))[(k // 8) % 4]
        out.append((x0, y0, rw, rh))
    return out


def all_lists():
    lists = [(name, positions(1000 + k, n, rw, rh)) for k, (name, n, rw, rh) in enumerate(LISTS)]
    sweep = [("sweep 16 x %dx%d" % (s, s), positions(2000 + s, 16, s, s)) for s in SWEEP]
    return lists, sweep


class Bench:
    def __init__(self, calls):
        S.init(0)
        S.set_mode(S.MODE_STRICT)
        self.calls = calls
        self.d_in = S.DeviceBuffer.from_numpy(synth.plane(H, W, synth.SEED0 + 3, "smooth"))
        self.st = S.Stream()
        self.ev = [S.Event(), S.Event()]
        self.bufs = {}

    def items(self, name, rects):
        offs, total = [], 0
        for (_, _, rw, rh) in rects:
            offs.append(total)
            total += 4 * rw * rh
        buf = self.bufs.setdefault(name, S.DeviceBuffer(total))
        arr, _ = S.rect_items([(x0, y0, rw, rh, (buf, o), 0) for (x0, y0, rw, rh), o in zip(rects, offs)])
        return arr, buf, offs

    def list_call(self, name, rects):
        arr, _, _ = self.items(name, rects)
        return lambda: S.y_path_rect_list_dev(self.d_in, 0, W, H, DW, DH, S.SRCNNF_Bicubic, arr, self.st)

    def loop_call(self, name, rects):
        _, buf, offs = self.items(name, rects)
        def run():
            for (x0, y0, rw, rh), o in zip(rects, offs):
                S.y_path_rect_dev(self.d_in, 0, W, H, DW, DH, S.SRCNNF_Bicubic, x0, y0, rw, rh, (buf, o), 0, self.st)
        return run

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


def stats(v):
    v = np.array(v)
    return float(np.median(v)), float(np.percentile(v, 75) - np.percentile(v, 25))


def child(mode, calls, env):
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", mode, "--calls", str(calls)], env=dict(os.environ, **env),
                       capture_output=True, text=True, timeout=900)
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")]
    if r.returncode != 0 or not line:
        raise SystemExit("child %s failed (exit %d)\n%s\n%s" % (mode, r.returncode, r.stdout[-800:], r.stderr[-2000:]))
    return json.loads(line[0][7:])


def run_child(mode, calls):
    """unfused: the four lists under SRCNN_RECT_LIST_UNFUSED=1; lifted: the sweep with the threshold lifted.  {name: [median, iqr]}"""
    b = Bench(calls)
    lists, sweep = all_lists()
    if mode == "unfused":
        assert "SRCNN_RECT_LIST_UNFUSED=1" in S.debug_settings()
        todo = lists
    else:
        todo = sweep
    series = b.measure([(name, b.list_call(name, rects)) for name, rects in todo])
    routes = {name: S.y_path_rect_list_plan(W, H, DW, DH, S.SRCNNF_Bicubic, rects).batched_items for name, rects in todo}
    print("RESULT " + json.dumps({name: list(stats(series[name])) + [routes[name]] for name, _ in todo}))
    b.st.destroy()
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--commit", default=None, help="what to record as the commit (default: git rev-parse HEAD)")
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.calls < 10:
        ap.error("--calls: at least 10 timed calls")
    if a.child:
        return run_child(a.child, a.calls)
    b = Bench(a.calls)
    L = S.lib()
    d_whole = S.DeviceBuffer(4 * DW * DH)
    lists, sweep = all_lists()
    calls = [("whole", lambda: S.check(L.srcnn_y_upscale2x_f32_dev(b.d_in.ptr, W, H, d_whole.ptr, b.st.handle)))]
    for name, rects in lists + sweep:
        calls += [(name + "/list", b.list_call(name, rects)), (name + "/loop", b.loop_call(name + " (loop)", rects))]
    series = b.measure(calls)
    med = {k: stats(v) for k, v in series.items()}
    plans = {name: S.y_path_rect_list_plan(W, H, DW, DH, S.SRCNNF_Bicubic, rects) for name, rects in lists + sweep}

    # what was timed last holds the whole frame's bits: the list's buffers and the loop's
    frame = d_whole.to_numpy(np.float32, (DH, DW))
    same = True
    for name, rects in lists + sweep:
        for key in (name, name + " (loop)"):
            _, buf, offs = b.items(key, rects)
            flat = buf.to_numpy(np.uint8, (buf.nbytes,))
            for (x0, y0, rw, rh), o in zip(rects, offs):
                got = flat[o:o + 4 * rw * rh].view(np.uint32).reshape(rh, rw)
                same = same and np.array_equal(got, frame[y0:y0 + rh, x0:x0 + rw].view(np.uint32))
    b.st.destroy()
    unfused = child("unfused", a.calls, {"SRCNN_RECT_LIST_UNFUSED": "1"})
    lifted = child("lifted", a.calls, {"SRCNN_RECT_LIST_SINGLE_SAMPLES": str(1 << 40)})

    lines = ["rect_list_probe: %s, strict mode, %d timed calls each after 3 warm-up rounds, %dx%d -> %dx%d, bicubic, rotated on one stream"
             % (S.device_name(), a.calls, W, H, DW, DH),
             "commit: %s    source digest: %s" % (commit_text(a.commit), build.source_digest()[:16]),
             "whole frame 7680x4320: median %.4f ms, IQR %.4f ms" % med["whole"],
             "device events, ms per call      list median     IQR | loop median     IQR | loop / list | unfused median     IQR | batched single atlases  cell_samples atlas_samples"]
    for name, _ in lists:
        p = plans[name]
        (lm, li), (om, oi) = med[name + "/list"], med[name + "/loop"]
        lines.append("  %-28s %12.4f %7.4f | %11.4f %7.4f | %11.2f | %14.4f %7.4f | %7d %6d %7d %13d %13d"
                     % (name, lm, li, om, oi, om / lm, unfused[name][0], unfused[name][1], p.batched_items, p.single_items, p.atlases, p.cell_samples, p.atlas_samples))
    lines.append("sweep, 16 rects of one size        list median     IQR | loop median     IQR | loop / list | threshold lifted   IQR | batched by default / lifted")
    for name, _ in sweep:
        p = plans[name]
        (lm, li), (om, oi) = med[name + "/list"], med[name + "/loop"]
        lines.append("  %-28s %15.4f %7.4f | %11.4f %7.4f | %11.2f | %16.4f %7.4f | %7d / %d" % (name, lm, li, om, oi, om / lm, lifted[name][0], lifted[name][1], p.batched_items, lifted[name][2]))
    ok = same
    for name, _ in lists[:2]:
        (lm, li), (om, oi) = med[name + "/list"], med[name + "/loop"]
        met = om - lm > li + oi
        ok = ok and met
        lines.append("condition: %s, list faster than the loop by more than both IQRs: %.4f ms vs %.4f ms, ratio %.2f (IQRs %.4f + %.4f ms) -- %s"
                     % (name, lm, om, om / lm, li, oi, "MET" if met else "NOT MET"))
    for name, _ in lists[2:]:
        (lm, li), (om, oi) = med[name + "/list"], med[name + "/loop"]
        met = lm - om <= oi
        ok = ok and met
        lines.append("condition: %s, list not slower than the loop by more than the loop's IQR: %.4f ms vs %.4f ms (IQR %.4f ms) -- %s"
                     % (name, lm, om, oi, "MET" if met else "NOT MET"))
    lines.append("every timed list and loop holds the whole frame's bits: %s" % same)
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
