#!/usr/bin/env python3
"""What one rectangle of a YUV frame costs: 3840x2160 -> 7680x4320, 4:2:0 semi-planar, bicubic, strict mode, a 960x512 interior
rect, in NV12 (8-bit) and in P010 (10 bits in the high end of a 16-bit word).

  (a)  srcnn_yuv_upscale_rect_dev                      the rect, chroma included
  (b)  srcnn_y_path_rect_f32_dev                       the same rect of the float Y plane alone: the floor of (a)
  (c)  srcnn_yuv_upscale_dev                           the whole frame -- what a caller paid for any region before
  (d)  (a) with SRCNN_YUV_RECT_UNFUSED=1               chroma by the plane route over the window, in a child process (the switch
                                                       is read when the library loads)

(a), (b) and (c) run in one process on one stream, rotated call by call, after 3 warm-up rounds; each call is timed with device
events around it (median of --calls, with the inter-quartile range as the spread).  The child runs under a time limit of its
own.  No threshold is fixed: the file states what was measured, and says whether (a) is slower than (d) by more than the
larger of the two spreads -- the bar for keeping k_yuv_window_chroma as the default route.

Usage: python tools/yuv_rect_probe.py [--calls N] [--commit TEXT] [--out FILE]      (profiles/yuv_rect_probe.txt is its output)
"""
import argparse
import hashlib
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import libsrcnn_amd as S
from libsrcnn_amd import build

W, H, MUL = 3840, 2160, 2.0
RECT = (3360, 1904, 960, 512)
FORMATS = (("NV12", 8, 0), ("P010", 10, 1))


def commit_text(given):
    if given:
        return given
    try:
        return subprocess.run(["git", "-C", ROOT, "rev-parse", "HEAD"], capture_output=True, text=True, check=True).stdout.strip()
    except (OSError, subprocess.CalledProcessError):
        return "unknown (no git here)"


def picture(depth):
    """Smooth planes with texture: a deterministic 4:2:0 frame, (Y, UV) as values of `depth` bits."""
    rng = np.random.default_rng(20240)
    top = (1 << depth) - 1

    def plane(h, w, k):
        yy, xx = np.mgrid[0:h, 0:w].astype(np.float32)
        v = 0.5 + 0.4 * np.sin(xx / (37.0 + 11 * k) + k) * np.cos(yy / (29.0 + 7 * k)) + rng.normal(0.0, 0.02, (h, w))
        return np.clip(v * top, 0, top).astype(np.uint8 if depth == 8 else np.uint16)
    y, u, v = plane(H, W, 0), plane(H // 2, W // 2, 1), plane(H // 2, W // 2, 2)
    return y, np.stack([u, v], axis=-1).reshape(H // 2, W)


def stats(v):
    v = np.array(v)
    return float(np.median(v)), float(np.percentile(v, 75) - np.percentile(v, 25)), float(v.min()), float(v.max())


def measure(calls_n, with_rest):
    """Per format: medians of the rect call (and, with_rest, of the Y rect and the whole frame) in this process."""
    S.init(0)
    S.set_mode(S.MODE_STRICT)
    dw, dh = S.output_size(W, H, MUL)
    x0, y0, rw, rh = RECT
    res = {"settings": S.debug_settings(), "formats": {}}
    for name, depth, msb in FORMATS:
        fmt = S.yuv_format("semiplanar", "420", depth, msb)
        dt = np.uint8 if depth == 8 else np.uint16
        bps = np.dtype(dt).itemsize
        y, uv = picture(depth)
        shift = 16 - depth if msb else 0
        d_y, d_uv = S.DeviceBuffer.from_numpy(y << shift), S.DeviceBuffer.from_numpy(uv << shift)
        d_ry, d_ruv = S.DeviceBuffer(rw * rh * bps), S.DeviceBuffer(rw * (rh // 2) * bps)
        st = S.Stream()
        ev = [S.Event(), S.Event()]
        calls = [("a", lambda: S.yuv_upscale_rect_dev(fmt, W, H, MUL, S.SRCNNF_Bicubic, [d_y, d_uv, None], None, x0, y0, rw, rh,
                                                      [d_ry, d_ruv, None], None, st))]
        if with_rest:
            d_f = S.DeviceBuffer.from_numpy(y.astype(np.float32) * np.float32(2.0 ** -(depth - 8)))
            d_frect = S.DeviceBuffer(4 * rw * rh)
            d_wy, d_wuv = S.DeviceBuffer(dw * dh * bps), S.DeviceBuffer(dw * (dh // 2) * bps)
            calls += [("b", lambda: S.y_path_rect_dev(d_f, 0, W, H, dw, dh, S.SRCNNF_Bicubic, x0, y0, rw, rh, d_frect, 0, st)),
                      ("c", lambda: S.yuv_upscale_dev(fmt, W, H, MUL, S.SRCNNF_Bicubic, [d_y, d_uv, None], None, [d_wy, d_wuv, None], None, st))]
        series = {k: [] for k, _ in calls}

        def timed(key, fn, keep):
            st.sync()
            ev[0].record(st)
            fn()
            ev[1].record(st)
            st.sync()
            if keep:
                series[key].append(ev[0].elapsed_ms(ev[1]))
        for _ in range(3):
            for key, fn in calls:
                timed(key, fn, False)
        n = len(calls)
        for k in range(calls_n):
            for key, fn in calls[k % n:] + calls[:k % n]:
                timed(key, fn, True)
        ry, ruv = d_ry.to_numpy(dt, (rh, rw)), d_ruv.to_numpy(dt, (rh // 2, rw))
        one = {"median": {k: stats(v) for k, v in series.items()}, "rect_sha": hashlib.sha256(ry.tobytes() + ruv.tobytes()).hexdigest()}
        if with_rest:
            wy = d_wy.to_numpy(dt, (dh, dw))[y0:y0 + rh, x0:x0 + rw]
            wuv = d_wuv.to_numpy(dt, (dh // 2, dw))[y0 // 2:(y0 + rh) // 2, x0:x0 + rw]
            one["same"] = bool(np.array_equal(ry, wy) and np.array_equal(ruv, wuv))
        res["formats"][name] = one
        st.destroy()
        del calls
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--commit", default=None, help="what to record as the commit (default: git rev-parse HEAD)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "yuv_rect_probe.txt"))
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.calls < 10:
        ap.error("--calls: at least 10 timed calls")
    if a.child:
        print("RESULT " + json.dumps(measure(a.calls, False)))
        return 0
    res = measure(a.calls, True)
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--calls", str(a.calls)], capture_output=True, text=True,
                       env=dict(os.environ, SRCNN_YUV_RECT_UNFUSED="1"), timeout=300)
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")]
    if r.returncode != 0 or not line:
        sys.stderr.write(r.stdout[-1000:] + r.stderr[-2000:])
        return 1
    unf = json.loads(line[0][7:])
    assert "SRCNN_YUV_RECT_UNFUSED=1" in unf["settings"] and "SRCNN_YUV_RECT_UNFUSED=0" in res["settings"]
    dw, dh = S.output_size(W, H, MUL)
    lines = ["yuv_rect_probe: %s, strict mode, %d timed calls each after 3 warm-up rounds, %dx%d -> %dx%d, 4:2:0 semi-planar, bicubic, rect %dx%d at (%d,%d)"
             % (S.device_name(), a.calls, W, H, dw, dh, RECT[2], RECT[3], RECT[0], RECT[1]),
             "commit: %s    source digest: %s" % (commit_text(a.commit), build.source_digest()[:16]),
             "device events, ms per call                       median     IQR     min     max   ns/pixel"]
    ok = True
    for name, _depth, _msb in FORMATS:
        f, u = res["formats"][name], unf["formats"][name]
        rows = [("(a) yuv rect", f["median"]["a"], RECT[2] * RECT[3]), ("(b) y_path rect, same rect", f["median"]["b"], RECT[2] * RECT[3]),
                ("(c) whole frame %dx%d" % (dw, dh), f["median"]["c"], dw * dh), ("(d) yuv rect, SRCNN_YUV_RECT_UNFUSED=1", u["median"]["a"], RECT[2] * RECT[3])]
        for what, (m, iqr, lo, hi), px in rows:
            lines.append("  %-5s %-38s %9.4f %7.4f %7.4f %7.4f %9.3f" % (name, what, m, iqr, lo, hi, 1e6 * m / px))
        (ma, sa), mb, mc, (md, sd) = f["median"]["a"][:2], f["median"]["b"][0], f["median"]["c"][0], u["median"]["a"][:2]
        spread = max(sa, sd)
        verdict = "SLOWER than (d) by more than the spread" if ma - md > spread else "not slower than (d) by more than the spread"
        same = f["same"] and f["rect_sha"] == u["rect_sha"]
        ok = ok and same
        lines += ["  %-5s colour work, (a) - (b): %.4f ms = %.2f x the Y rect (b); (a) is %.1f x cheaper than the whole frame (c)"
                  % (name, ma - mb, (ma - mb) / mb, mc / ma),
                  "  %-5s (a) - (d) = %+.4f ms, spread (larger IQR of the two) %.4f ms: (a) is %s" % (name, ma - md, spread, verdict),
                  "  %-5s the timed rect holds the whole frame's bytes, and both routes give the same bytes: %s" % (name, same)]
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
