#!/usr/bin/env python3
"""What one rectangle of an RGB image costs: 3840x2160 -> 7680x4320, 8-bit interleaved RGB, bicubic, strict mode, a 960x512
interior rect.

  (a)  srcnn_rgb_upscale_rect_dev                      the rect, colour included
  (b)  srcnn_y_path_rect_f32_dev                       the same rect of the Y plane alone: the floor of (a)
  (c)  srcnn_rgb_upscale_dev                           the whole image -- what a caller paid for any region before
  (a') (a) with SRCNN_RGB_RECT_UNFUSED=1               the plane route over the window, in a child process (the switch is read
                                                       when the library loads)

(a), (b) and (c) run in one process on one stream, rotated call by call, after 3 warm-up rounds; each call is timed with device
events around it (median of --calls).  A second pass with srcnn_profile_enable gives the mean time of the Y path's stages inside
(a) and (b); what they leave of (a)'s median is the colour shell (k_rgb_window_y, k_rgb_window_merge), the window store and the
launch gaps.  No threshold is fixed: the file states what was measured, and says so when the shell, (a) - (b), costs more than
the Y rect (b) itself.

Usage: python tools/rgb_rect_probe.py [--calls N] [--commit TEXT] [--out FILE]      (profiles/rgb_rect_probe.txt is its output)
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
from libsrcnn_amd import build

W, H, MUL = 3840, 2160, 2.0
RECT = (3360, 1904, 960, 512)


def commit_text(given):
    if given:
        return given
    try:
        return subprocess.run(["git", "-C", ROOT, "rev-parse", "HEAD"], capture_output=True, text=True, check=True).stdout.strip()
    except (OSError, subprocess.CalledProcessError):
        return "unknown (no git here)"


def picture():
    """Smooth colour with texture: a deterministic 8-bit RGB image."""
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float32)
    rng = np.random.default_rng(20240)
    chans = [127.5 + 100.0 * np.sin(xx / (37.0 + 11 * k) + k) * np.cos(yy / (29.0 + 7 * k)) + rng.normal(0.0, 6.0, (H, W)) for k in range(3)]
    return np.clip(np.stack(chans, axis=-1), 0, 255).astype(np.uint8)


def stats(v):
    v = np.array(v)
    return float(np.median(v)), float(np.percentile(v, 75) - np.percentile(v, 25)), float(v.min()), float(v.max())


def measure(calls_n, with_rest):
    """Medians of the rect call (and, with_rest, of the Y rect and the whole image) in this process."""
    S.init(0)
    S.set_mode(S.MODE_STRICT)
    dw, dh = S.output_size(W, H, MUL)
    x0, y0, rw, rh = RECT
    img = picture()
    fmt = S.rgb_format("interleaved", "rgb", False, 8)
    d_img = S.DeviceBuffer.from_numpy(img)
    d_rect, d_rconv = S.DeviceBuffer(3 * rw * rh), S.DeviceBuffer(rw * rh)
    st = S.Stream()
    ev = [S.Event(), S.Event()]
    calls = [("a", lambda: S.rgb_upscale_rect_dev(fmt, W, H, MUL, S.SRCNNF_Bicubic, [d_img], None, x0, y0, rw, rh, [d_rect], None, d_rconv, 0, st))]
    if with_rest:
        f = img.astype(np.float32)
        yplane = (np.float32(0.299) * f[..., 0]) + (np.float32(0.587) * f[..., 1]) + (np.float32(0.114) * f[..., 2])
        d_y = S.DeviceBuffer.from_numpy(yplane)
        d_yrect = S.DeviceBuffer(4 * rw * rh)
        d_whole, d_wconv = S.DeviceBuffer(3 * dw * dh), S.DeviceBuffer(dw * dh)
        calls += [("b", lambda: S.y_path_rect_dev(d_y, 0, W, H, dw, dh, S.SRCNNF_Bicubic, x0, y0, rw, rh, d_yrect, 0, st)),
                  ("c", lambda: S.rgb_upscale_dev(fmt, W, H, MUL, S.SRCNNF_Bicubic, [d_img], None, [d_whole], None, d_wconv, 0, st))]
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
    for k in range(calls_n):
        for name, fn in calls[k % n:] + calls[:k % n]:
            timed(name, fn, True)
    stages = {}
    S.profile_enable(True)
    try:
        for name, fn in calls:
            st.sync()
            S.profile_reset()
            for _ in range(calls_n):
                fn()
            st.sync()
            prof = S.profile_read()
            stages[name] = {k: prof[k][0] / calls_n for k in S.STAGES}
    finally:
        S.profile_enable(False)
    res = {"median": {k: stats(v) for k, v in series.items()}, "stages": stages, "settings": S.debug_settings(),
           "rect_sha": __import__("hashlib").sha256(d_rect.to_numpy(np.uint8, (rh, rw, 3)).tobytes() + d_rconv.to_numpy(np.uint8, (rh, rw)).tobytes()).hexdigest()}
    if with_rest:
        whole = d_whole.to_numpy(np.uint8, (dh, dw, 3))[y0:y0 + rh, x0:x0 + rw]
        wconv = d_wconv.to_numpy(np.uint8, (dh, dw))[y0:y0 + rh, x0:x0 + rw]
        res["same"] = bool(np.array_equal(d_rect.to_numpy(np.uint8, (rh, rw, 3)), whole) and np.array_equal(d_rconv.to_numpy(np.uint8, (rh, rw)), wconv))
    st.destroy()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--commit", default=None, help="what to record as the commit (default: git rev-parse HEAD)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rgb_rect_probe.txt"))
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.calls < 10:
        ap.error("--calls: at least 10 timed calls")
    if a.child:
        print("RESULT " + json.dumps(measure(a.calls, False)))
        return 0
    res = measure(a.calls, True)
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--calls", str(a.calls)], capture_output=True, text=True,
                       env=dict(os.environ, SRCNN_RGB_RECT_UNFUSED="1"), timeout=300)
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")]
    if r.returncode != 0 or not line:
        sys.stderr.write(r.stdout[-1000:] + r.stderr[-2000:])
        return 1
    unf = json.loads(line[0][7:])
    assert "SRCNN_RGB_RECT_UNFUSED=1" in unf["settings"]
    dw, dh = S.output_size(W, H, MUL)
    rows = [("(a)  rgb rect %dx%d at (%d,%d)" % (RECT[2], RECT[3], RECT[0], RECT[1]), res["median"]["a"], res["stages"]["a"], RECT[2] * RECT[3]),
            ("(b)  y_path rect, same rect", res["median"]["b"], res["stages"]["b"], RECT[2] * RECT[3]),
            ("(c)  whole image %dx%d" % (dw, dh), res["median"]["c"], res["stages"]["c"], dw * dh),
            ("(a') rgb rect, SRCNN_RGB_RECT_UNFUSED=1", unf["median"]["a"], unf["stages"]["a"], RECT[2] * RECT[3])]
    lines = ["rgb_rect_probe: %s, strict mode, %d timed calls each after 3 warm-up rounds, %dx%d -> %dx%d, 8-bit interleaved RGB, bicubic"
             % (S.device_name(), a.calls, W, H, dw, dh),
             "commit: %s    source digest: %s" % (commit_text(a.commit), build.source_digest()[:16]),
             "device events, ms per call                  median     IQR     min     max   ns/pixel | stage means: resample  conv12   conv3   rest"]
    for name, (m, iqr, lo, hi), sg, px in rows:
        lines.append("  %-38s %9.4f %7.4f %7.4f %7.4f %9.3f | %20.4f %7.4f %7.4f %6.4f"
                     % (name, m, iqr, lo, hi, 1e6 * m / px, sg["resample"], sg["conv12"], sg["conv3"], m - sum(sg.values())))
    ma, mb, mc, mu = res["median"]["a"][0], res["median"]["b"][0], res["median"]["c"][0], unf["median"]["a"][0]
    shell = ma - mb
    lines += ["colour shell of the rect, (a) - (b): %.4f ms = %.2f x the Y rect (b) -- %s" %
              (shell, shell / mb, "MORE than the Y rect itself" if shell > mb else "less than the Y rect itself"),
              "(a) is %.1f x cheaper than the whole image (c); the plane route (a') costs %.2f x (a)" % (mc / ma, mu / ma),
              "the timed rect holds the whole image's bytes (out and conv): %s; both routes give the same bytes: %s"
              % (res["same"], res["rect_sha"] == unf["rect_sha"])]
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)
    return 0 if res["same"] and res["rect_sha"] == unf["rect_sha"] else 1


if __name__ == "__main__":
    sys.exit(main())
