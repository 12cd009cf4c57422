#!/usr/bin/env python3
"""What one rectangle of a PACKED YUV frame costs: 3840x2160 -> 7680x4320, bicubic, strict mode, a 960x512 rect at a unit-aligned
interior origin, in YUY2, Y210, Y410 and v210.

  (a)   srcnn_yuv_packed_upscale_rect_dev                   the rect, chroma (and alpha) included: k_yuvp_window_merge
  (b)   srcnn_y_path_rect_f32_dev                           the same rect of the float Y plane alone: the floor of (a)
  (c)   srcnn_yuv_packed_upscale_dev                        the whole frame -- what a caller paid for any region before
  (a')  (a) with SRCNN_YUV_PACKED_RECT_UNFUSED=1            the plane route over the window (the switch is read when the library
                                                            loads)

Two child processes, each under a time limit of its own: one with the default settings measures (a), (b) and (c) on one stream,
rotated call by call, after 3 warm-up rounds; one with the switch set measures (a').  Each call is timed with device events
around it (median of --calls, with the inter-quartile range as the spread).  The probe also asserts that (a), (a') and the crop
of (c) are the same bytes.  No time is fixed: the yardstick is (a') of the same run, and a format stays on the fused route by
default only if its (a) is not slower than (a') by more than the larger IQR of the two.

Usage: python tools/yuv_packed_rect_probe.py [--calls N] [--commit TEXT] [--out FILE]
profiles/yuv_packed_rect_probe.txt is its output; what that file holds below the line that starts with "==== kernel resources" (the
resource table of the new kernels, the disassembly comparison, the kernel trace) is kept as it is.
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
RECT = (3360, 1904, 960, 512)          # 3360 and 960 are multiples of 6: legal in every format
# name, depth, alpha bits
FORMATS = (("yuy2", 8, 0), ("y210", 10, 0), ("y410", 10, 2), ("v210", 10, 0))
KEEP = "==== kernel resources"


def commit_text(given):
    if given:
        return given
    try:
        return subprocess.run(["git", "-C", ROOT, "rev-parse", "HEAD"], capture_output=True, text=True, check=True).stdout.strip()
    except (OSError, subprocess.CalledProcessError):
        return "unknown (no git here)"


def picture(name, depth, abits):
    """Smooth planes with texture, deterministic: (the packed frame, its Y plane as values of `depth` bits)."""
    rng = np.random.default_rng(20240)
    top = (1 << depth) - 1
    cw = W if name == "y410" else W // 2

    def plane(h, w, k, t=top):
        yy, xx = np.mgrid[0:h, 0:w].astype(np.float32)
        v = 0.5 + 0.4 * np.sin(xx / (37.0 + 11 * k) + k) * np.cos(yy / (29.0 + 7 * k)) + rng.normal(0.0, 0.02, (h, w))
        return np.clip(v * t, 0, t).astype(np.uint32)
    Y, U, V = plane(H, W, 0), plane(H, cw, 1), plane(H, cw, 2)
    if name == "yuy2":
        px = np.stack([Y[:, 0::2], U, Y[:, 1::2], V], -1).astype(np.uint8)
        return np.ascontiguousarray(px).reshape(H, 2 * W), Y
    if name == "y210":
        px = (np.stack([Y[:, 0::2], U, Y[:, 1::2], V], -1) << 6).astype("<u2")
        return np.ascontiguousarray(px).view(np.uint8).reshape(H, 4 * W), Y
    if name == "y410":
        A = plane(H, W, 3, (1 << abits) - 1)
        q = U | (Y << 10) | (V << 20) | (A << 30)
        return np.ascontiguousarray(q.astype("<u4")).view(np.uint8).reshape(H, 4 * W), Y
    g = W // 6                                               # v210: 3840 = 640 groups = 80 blocks, no padding
    y, u, v = Y.reshape(H, g, 6), U.reshape(H, g, 3), V.reshape(H, g, 3)
    q = np.stack([u[..., 0] | (y[..., 0] << 10) | (v[..., 0] << 20), y[..., 1] | (u[..., 1] << 10) | (y[..., 2] << 20),
                  v[..., 1] | (y[..., 3] << 10) | (u[..., 2] << 20), y[..., 4] | (v[..., 2] << 10) | (y[..., 5] << 20)], -1)
    return np.ascontiguousarray(q.astype("<u4")).view(np.uint8).reshape(H, 16 * g), Y


def stats(v):
    v = np.array(v)
    return float(np.median(v)), float(np.percentile(v, 75) - np.percentile(v, 25)), float(v.min()), float(v.max())


def measure(calls_n, with_rest):
    """Per format: medians of the rect call (and, with_rest, of the Y rect and the whole frame) in this process."""
    S.init(0)
    S.set_mode(S.MODE_STRICT)
    dw, dh = S.output_size(W, H, MUL)
    x0, y0, rw, rh = RECT
    res = {"settings": S.debug_settings(), "device": S.device_name(), "formats": {}}
    for name, depth, abits in FORMATS:
        frame, Y = picture(name, depth, abits)
        rb, _ = S.yuv_packed_row_bytes(name, W)
        drb, _ = S.yuv_packed_row_bytes(name, dw)
        _unit, off, n = S.yuv_packed_span_bytes(name, dw, x0, rw)
        assert frame.shape == (H, rb)
        d_in, d_rect = S.DeviceBuffer.from_numpy(frame), S.DeviceBuffer(rh * n)
        st = S.Stream()
        ev = [S.Event(), S.Event()]
        calls = [("a", lambda: S.yuv_packed_upscale_rect_dev(name, W, H, MUL, S.SRCNNF_Bicubic, d_in, 0, x0, y0, rw, rh, d_rect, 0, st))]
        if with_rest:
            d_f = S.DeviceBuffer.from_numpy(Y.astype(np.float32) * np.float32(2.0 ** -(depth - 8)))
            d_frect = S.DeviceBuffer(4 * rw * rh)
            d_whole = S.DeviceBuffer(dh * drb)
            calls += [("b", lambda: S.y_path_rect_dev(d_f, 0, W, H, dw, dh, S.SRCNNF_Bicubic, x0, y0, rw, rh, d_frect, 0, st)),
                      ("c", lambda: S.yuv_packed_upscale_dev(name, W, H, MUL, S.SRCNNF_Bicubic, d_in, 0, d_whole, 0, st))]
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
        k_n = len(calls)
        for k in range(calls_n):
            for key, fn in calls[k % k_n:] + calls[:k % k_n]:
                timed(key, fn, True)
        rect = d_rect.to_numpy(np.uint8, (rh, n))
        one = {"median": {k: stats(v) for k, v in series.items()}, "rect_sha": hashlib.sha256(rect.tobytes()).hexdigest()}
        if with_rest:
            one["same"] = bool(np.array_equal(rect, d_whole.to_numpy(np.uint8, (dh, drb))[y0:y0 + rh, off:off + n]))
        res["formats"][name] = one
        st.destroy()
        del calls
    return res


def child(calls_n, unfused, limit):
    args = [sys.executable, os.path.abspath(__file__), "--child", "rect" if unfused else "all", "--calls", str(calls_n)]
    env = dict(os.environ, SRCNN_YUV_PACKED_RECT_UNFUSED="1" if unfused else "0")
    r = subprocess.run(args, capture_output=True, text=True, env=env, timeout=limit)
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")]
    if r.returncode != 0 or not line:
        sys.stderr.write(r.stdout[-1000:] + r.stderr[-2000:])
        raise SystemExit(1)
    return json.loads(line[0][7:])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--commit", default=None, help="what to record as the commit (default: git rev-parse HEAD)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "yuv_packed_rect_probe.txt"))
    ap.add_argument("--limit", type=int, default=240, help="time limit of each child process, seconds")
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.calls < 10:
        ap.error("--calls: at least 10 timed calls")
    if a.child:
        print("RESULT " + json.dumps(measure(a.calls, a.child == "all")))
        return 0
    res = child(a.calls, False, a.limit)
    unf = child(a.calls, True, a.limit)
    assert "SRCNN_YUV_PACKED_RECT_UNFUSED=1" in unf["settings"] and "SRCNN_YUV_PACKED_RECT_UNFUSED=0" in res["settings"]
    dw, dh = int(W * MUL), int(H * MUL)
    px = RECT[2] * RECT[3]
    lines = ["yuv_packed_rect_probe: %s, strict mode, %d timed calls each after 3 warm-up rounds, %dx%d -> %dx%d, bicubic, rect %dx%d at (%d,%d)"
             % (res["device"], a.calls, W, H, dw, dh, RECT[2], RECT[3], RECT[0], RECT[1]),
             "commit: %s    source digest: %s" % (commit_text(a.commit), build.source_digest()[:16]),
             "device events, ms per call                                median     IQR     min     max   ns/pixel"]
    ok = True
    fused, plane = [], []
    for name, _depth, _abits in FORMATS:
        f, u = res["formats"][name], unf["formats"][name]
        rows = [("(a)  packed rect", f["median"]["a"], px), ("(b)  y_path rect, same rect", f["median"]["b"], px),
                ("(c)  whole frame %dx%d" % (dw, dh), f["median"]["c"], dw * dh),
                ("(a') packed rect, SRCNN_YUV_PACKED_RECT_UNFUSED=1", u["median"]["a"], px)]
        for what, (m, iqr, lo, hi), n in rows:
            lines.append("  %-5s %-47s %9.4f %7.4f %7.4f %7.4f %9.3f" % (name, what, m, iqr, lo, hi, 1e6 * m / n))
        (ma, sa), mb, mc, (md, sd) = f["median"]["a"][:2], f["median"]["b"][0], f["median"]["c"][0], u["median"]["a"][:2]
        spread = max(sa, sd)
        slower = ma - md > spread
        (plane if slower else fused).append(name)
        same = f["same"] and f["rect_sha"] == u["rect_sha"]
        ok = ok and same
        lines += ["  %-5s colour work, (a) - (b): %.4f ms = %.2f x the Y rect (b) (NV12 rect: 0.09 x, profiles/yuv_rect_probe.txt); (a) is %.1f x cheaper than the whole frame (c)"
                  % (name, ma - mb, (ma - mb) / mb, mc / ma),
                  "  %-5s (a) - (a') = %+.4f ms, spread (larger IQR of the two) %.4f ms: (a) is %s" %
                  (name, ma - md, spread, "SLOWER than (a') by more than the spread" if slower else "not slower than (a') by more than the spread"),
                  "  %-5s (a), (a') and the crop of (c) are the same bytes: %s" % (name, same)]
    lines.append("route decision by the rule above: fused route (k_yuvp_window_merge) for %s; plane route for %s" %
                 (", ".join(fused) or "none", ", ".join(plane) or "none"))
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if a.out:
        kept = ""
        if os.path.exists(a.out):
            old = open(a.out).read()
            if KEEP in old:
                kept = "\n" + old[old.index(KEEP):]
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + kept)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
