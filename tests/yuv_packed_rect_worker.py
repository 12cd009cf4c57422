"""What tests/test_gpu_yuv_packed_rect.py shares with its child processes, and the children themselves: things that need a process
of their own -- a switch the library reads when it loads.  Usage: python tests/yuv_packed_rect_worker.py MODE SEED; prints one
line "RESULT <json>".
"""
import hashlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
# the edge cases, 2x bicubic and 2.5x bicubic: 70 x 40 -> 140 x 80 (140 is no multiple of 6: v210's last group is partial, and the
# row is three 128-byte blocks wide) and 35 x 20 -> 87 x 50 (an odd output width: the last pixel pair of a 4:2:2 row is half empty)
EDGE_SHAPES = ((70, 40, 2.0, 2), (35, 20, 2.5, 2))
NAMES = ("yuy2", "uyvy", "yvyu", "y210", "y212", "y216", "vuya", "y410", "y416", "v210")
_422 = ("yuy2", "uyvy", "yvyu", "y210", "y212", "y216")
UNIT = {n: (6 if n == "v210" else 2 if n in _422 else 1) for n in NAMES}
UNIT_BYTES = {"yuy2": 4, "uyvy": 4, "yvyu": 4, "y210": 8, "y212": 8, "y216": 8, "vuya": 4, "y410": 4, "y416": 8, "v210": 16}


def out_size(w, h, mul):
    m = np.float32(mul)
    return int(np.float32(w) * m), int(np.float32(h) * m)


def row_bytes(name, w):
    if name in ("yuy2", "uyvy", "yvyu"):
        return 4 * ((w + 1) // 2)
    if name in ("y210", "y212", "y216"):
        return 8 * ((w + 1) // 2)
    if name in ("vuya", "y410"):
        return 4 * w
    if name == "y416":
        return 8 * w
    return 128 * ((w + 47) // 48)


def span(name, width, x, n):
    """(byte offset, byte length) of pixels [x, x + n) of a width-pixel row, restated: whole units, and the rest of the tight row
    when the pixels end it."""
    u, ub = UNIT[name], UNIT_BYTES[name]
    assert x % u == 0 and (n % u == 0 or x + n == width) and 0 < n and x + n <= width, (name, width, x, n)
    off = x // u * ub
    end = row_bytes(name, width) if x + n == width else (x + n) // u * ub
    return off, end - off


def snap(rect, name, dw):
    """The origin snapped down to the unit; the far edge up to the unit, or to dw."""
    x0, y0, rw, rh = (int(v) for v in rect)
    u = UNIT[name]
    x1 = min(dw, -(-(x0 + rw) // u) * u)
    x0 -= x0 % u
    return x0, y0, x1 - x0, rh


def crop(whole, rect, name, dw):
    """The rect's row segments of a whole packed frame (dh x row_bytes(dw) uint8)."""
    x0, y0, rw, rh = rect
    off, n = span(name, dw, x0, rw)
    return whole[y0:y0 + rh, off:off + n]


def edge_case_rects(seed, name, dw, dh):
    """The rects of an edge case for one format, snapped, without repeats, in a fixed order: every pair of x edges with a random
    pair of y edges and the other way round (edge_rects), the whole output, windows of 63 ... 129 columns, and every pair of
    unit-aligned columns next to the 64 / 128 tile edges and the right border with a random pair of y edges."""
    from test_gpu_rect import edge_rects, pairs
    rng = np.random.default_rng(seed)
    rects = edge_rects(dw, dh, rng)
    rects += [(0, 0, dw, dh)]
    rects += [(8, 10, ww - 12, min(30, dh - 10)) for ww in (63, 64, 65, 127, 128, 129) if 8 + ww - 12 <= dw]
    u = UNIT[name]
    cols = sorted({c for e in (0, 6, 12, 48, 60, 64, 66, 96, 120, 126, 128, dw - 12, dw - 6, dw) for c in (e - e % u, min(dw, -(-e // u) * u))
                   if 0 <= e <= dw})
    ys = pairs(dh)
    for a in cols:
        for b in cols:
            if a < b:
                y0, y1 = ys[rng.integers(len(ys))]
                rects.append((a, y0, b - a, y1 - y0))
    out, seen = [], set()
    for r in rects:
        r = snap(r, name, dw)
        if r not in seen:
            seen.add(r)
            out.append(r)
    return out


class Rig:
    """One packed source frame in device memory (tight) and a result buffer; raw() runs one rect call and returns the (rh, bytes)
    uint8 array of its row segments."""

    def __init__(self, S, name, src, w, mul, filt):
        self.S, self.name, self.w, self.mul, self.filt = S, name, w, mul, filt
        self.h = src.shape[0]
        self.dw, self.dh = S.output_size(w, self.h, mul)
        self.din = S.DeviceBuffer.from_numpy(np.ascontiguousarray(src, np.uint8))
        self.dout = S.DeviceBuffer(max(1, self.dh * row_bytes(name, self.dw)))

    def raw(self, x0, y0, rw, rh, stream=None):
        S = self.S
        S.yuv_packed_upscale_rect_dev(self.name, self.w, self.h, self.mul, self.filt, self.din, 0, x0, y0, rw, rh, self.dout, 0, stream)
        if stream is not None:
            stream.sync()
        else:
            S.sync()
        _off, n = span(self.name, self.dw, x0, rw)
        return self.dout.to_numpy(np.uint8, (rh, n))


def edge_source(name, shape):
    from test_gpu_yuv_packed import frame_planes, pack
    w, h, _mul, _filt = shape
    return pack(name, *frame_planes(name, w, h, 7040 + w))


def edge_rig(S, name, shape):
    w, _h, mul, filt = shape
    return Rig(S, name, edge_source(name, shape), w, mul, filt)


def edge_digest(S, seed, name, shape):
    """sha256 over the row segments of every rect of an edge case in one format."""
    rig = edge_rig(S, name, shape)
    h = hashlib.sha256()
    for r in edge_case_rects(seed, name, rig.dw, rig.dh):
        h.update(rig.raw(*r).tobytes())
    return h.hexdigest()


def digest_key(name, shape):
    return "%s/%dx%d" % (name, shape[0], shape[1])


def mode_unfused(seed):
    import libsrcnn_amd as S
    S.init(0)
    assert "SRCNN_YUV_PACKED_RECT_UNFUSED=1" in S.debug_settings()
    return {digest_key(name, shape): edge_digest(S, seed, name, shape) for name in NAMES for shape in EDGE_SHAPES}


if __name__ == "__main__":
    result = {"unfused": mode_unfused}[sys.argv[1]](int(sys.argv[2]))
    print("RESULT " + json.dumps(result))
