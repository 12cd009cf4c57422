"""What tests/test_gpu_yuv_rect.py shares with its child processes, and the children themselves: things that need a process of
their own -- a switch the library reads when it loads.  Usage: python tests/yuv_rect_worker.py MODE SEED; prints one line
"RESULT <json>".
"""
import hashlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
PLANAR, SEMI = 0, 1
# the edge case: 70 x 40 -> 140 x 80, 2x bicubic, in three format cells (layout, chroma, depth, msb_aligned)
EDGE_CELLS = (("planar", "420", 8, 0), ("semiplanar", "422", 10, 1), ("planar", "444", 16, 0))
EDGE_SHAPE = (70, 40, 2.0, 2)


def digest(*arrays):
    return hashlib.sha256(b"".join(np.ascontiguousarray(a).tobytes() for a in arrays)).hexdigest()


def snap(rect, chroma):
    """The origin snapped down to even where the format demands it; the far edge is kept."""
    x0, y0, rw, rh = (int(v) for v in rect)
    if chroma != "444":
        rw, x0 = rw + (x0 & 1), x0 - (x0 & 1)
    if chroma == "420":
        rh, y0 = rh + (y0 & 1), y0 - (y0 & 1)
    return x0, y0, rw, rh


def chroma_rect(rect, chroma):
    """(cx0, cy0, crw, crh): the chroma samples that cover a (snapped) luma rect."""
    x0, y0, rw, rh = rect
    cx0, cx1 = (x0, x0 + rw) if chroma == "444" else (x0 // 2, (x0 + rw + 1) // 2)
    cy0, cy1 = (y0 // 2, (y0 + rh + 1) // 2) if chroma == "420" else (y0, y0 + rh)
    return cx0, cy0, cx1 - cx0, cy1 - cy0


def edge_case_rects(seed, chroma):
    """The rects of the edge case for one chroma format, snapped, without repeats, in a fixed order."""
    from test_gpu_rect import edge_rects
    rects = edge_rects(140, 80, np.random.default_rng(seed))
    rects += [(0, 0, 140, 80)]
    rects += [(8, 10, ww - 12, 30) for ww in (63, 64, 65, 127, 128, 129)]     # windows of 63 ... 129 columns: rect + 6 on both sides
    out, seen = [], set()
    for r in rects:
        r = snap(r, chroma)
        if r not in seen:
            seen.add(r)
            out.append(r)
    return out


def interleave(a, b):
    return np.stack([a, b], axis=-1).reshape(a.shape[0], 2 * a.shape[1])


class Rig:
    """One source frame in device memory (tight) in a format, and result buffers; raw() runs one call and returns the rect's
    planes as the words the library wrote (semi-planar: Y', UV'), values() the same as values (Y', U', V') after checking
    that the bits beside the value are zero."""

    def __init__(self, S, Y, U, V, layout, chroma, depth, msb, mul, filt):
        self.S, self.chroma, self.depth, self.msb, self.mul, self.filt = S, chroma, depth, msb, mul, filt
        self.semi = layout in ("semiplanar", SEMI)
        self.h, self.w = Y.shape
        self.dt = np.uint8 if depth == 8 else np.uint16
        self.bps = np.dtype(self.dt).itemsize
        self.fmt = S.yuv_format(SEMI if self.semi else PLANAR, chroma, depth, msb)
        words = [(P.astype(self.dt) << (16 - depth)) if msb else P.astype(self.dt) for P in (Y, U, V)]
        planes = [words[0], interleave(words[1], words[2])] if self.semi else words
        self.n = len(planes)
        self.din = [S.DeviceBuffer.from_numpy(np.ascontiguousarray(p)) for p in planes]
        self.dw, self.dh = S.output_size(self.w, self.h, mul)
        sizes = [S.yuv_plane_size(self.fmt, self.dw, self.dh, k) for k in range(self.n)]
        self.dout = [S.DeviceBuffer(max(1, r * rb)) for (_c, r, rb) in sizes]
        self.pad = [None] * (3 - self.n)

    def raw(self, x0, y0, rw, rh, stream=None):
        S = self.S
        S.yuv_upscale_rect_dev(self.fmt, self.w, self.h, self.mul, self.filt, self.din + self.pad, None, x0, y0, rw, rh,
                               self.dout + self.pad, None, stream)
        if stream is not None:
            stream.sync()
        else:
            S.sync()
        shapes = [(r, rb // self.bps) for (_c, r, rb) in (S.yuv_plane_size(self.fmt, rw, rh, k) for k in range(self.n))]
        return [b.to_numpy(self.dt, s) for b, s in zip(self.dout, shapes)]

    def values(self, x0, y0, rw, rh, stream=None):
        return self.to_values(self.raw(x0, y0, rw, rh, stream))

    def to_values(self, outs):
        if self.semi:
            outs = [outs[0], np.ascontiguousarray(outs[1][:, 0::2]), np.ascontiguousarray(outs[1][:, 1::2])]
        if self.depth > 8:
            shift = 16 - self.depth
            for name, o in zip("YUV", outs):
                if self.msb:
                    assert not np.any(o & ((1 << shift) - 1)), "%s': low bits set in MSB-aligned output" % name
                else:
                    assert not np.any(o >> self.depth), "%s': high bits set in LSB-aligned output" % name
            if self.msb:
                outs = [o >> shift for o in outs]
        return tuple(outs)


def edge_rig(S, cell):
    from test_gpu_yuv_ex import frame
    layout, chroma, depth, msb = cell
    w, h, mul, filt = EDGE_SHAPE
    return Rig(S, *frame(w, h, chroma, depth, 7040 + depth), layout, chroma, depth, msb, mul, filt)


def edge_digest(S, seed, cell):
    """sha256 over the raw planes of every rect of the edge case in one format cell."""
    rig = edge_rig(S, cell)
    h = hashlib.sha256()
    for r in edge_case_rects(seed, cell[1]):
        for p in rig.raw(*r):
            h.update(np.ascontiguousarray(p).tobytes())
    return h.hexdigest()


def mode_unfused(seed):
    import libsrcnn_amd as S
    S.init(0)
    assert "SRCNN_YUV_RECT_UNFUSED=1" in S.debug_settings()
    return {"/".join(str(v) for v in cell): edge_digest(S, seed, cell) for cell in EDGE_CELLS}


if __name__ == "__main__":
    result = {"unfused": mode_unfused}[sys.argv[1]](int(sys.argv[2]))
    print("RESULT " + json.dumps(result))
