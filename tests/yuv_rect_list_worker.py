"""What tests/test_gpu_yuv_rect_list.py shares with its child process, and the child itself: SRCNN_YUV_RECT_LIST_UNFUSED is read
when the library loads, so the forced single route needs a process of its own.  Usage: python tests/yuv_rect_list_worker.py MODE;
prints one line "RESULT <json>".
"""
import hashlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from rect_list_worker import DH, DW, H, W, border_rects, seeded_rects      # noqa: E402,F401  (the Y list's frame and lists)
from yuv_rect_worker import Rig, chroma_rect, snap                          # noqa: E402,F401

CANARY = 0xA5
# the border case: (layout, chroma, depth, msb_aligned)
BORDER_CELLS = (("planar", "420", 8, 0), ("semiplanar", "422", 10, 1), ("planar", "444", 16, 0))
FRAME_SEED = 9656


def snapped(rects, chroma):
    """The rects snapped to the format's origin rule, without repeats, in their order."""
    out, seen = [], set()
    for r in rects:
        r = snap(r, chroma)
        if r not in seen:
            seen.add(r)
            out.append(r)
    return out


def digest(items):
    return hashlib.sha256(b"".join(np.ascontiguousarray(p).tobytes() for it in items for p in it)).hexdigest()


class YuvListRig(Rig):
    """Rig of tests/yuv_rect_worker.py (one source frame in device memory, tight) with the list call: raw_run() is one list call
    with the planes of every rect in tight regions of their own and returns, per item, the words the library wrote (semi-planar:
    Y', UV'); run() the same as values (Y', U', V'); loop() the same rects through single calls into the same layout."""

    def layout_of(self, rects):
        S, items, total = self.S, [], 0
        for (_, _, rw, rh) in rects:
            one = []
            for k in range(self.n):
                _c, r, rb = S.yuv_plane_size(self.fmt, rw, rh, k)
                one.append((total, (r, rb // self.bps)))
                total += (r * rb + 15) & ~15
            items.append(one)
        return items, max(16, total)

    def queue(self, rects, stream=None):
        """Queues one list call; returns (buffer, layout)."""
        lay, total = self.layout_of(rects)
        buf = self.S.DeviceBuffer(total)
        items = [(x0, y0, rw, rh, [(buf, o) for o, _ in one], None) for (x0, y0, rw, rh), one in zip(rects, lay)]
        self.S.yuv_upscale_rect_list_dev(self.fmt, self.w, self.h, self.mul, self.filt, self.din + self.pad, None, items, stream)
        return buf, lay

    def fetch_raw(self, buf, lay):
        flat = buf.to_numpy(np.uint8, (buf.nbytes,))
        return [[flat[o:o + sh[0] * sh[1] * self.bps].view(self.dt).reshape(sh).copy() for o, sh in one] for one in lay]

    def fetch(self, buf, lay):
        return [self.to_values(one) for one in self.fetch_raw(buf, lay)]

    def raw_run(self, rects):
        buf, lay = self.queue(rects)
        self.S.sync()
        return self.fetch_raw(buf, lay)

    def run(self, rects):
        return [self.to_values(one) for one in self.raw_run(rects)]

    def raw_loop(self, rects):
        lay, total = self.layout_of(rects)
        buf = self.S.DeviceBuffer(total)
        for (x0, y0, rw, rh), one in zip(rects, lay):
            self.S.yuv_upscale_rect_dev(self.fmt, self.w, self.h, self.mul, self.filt, self.din + self.pad, None, x0, y0, rw, rh,
                                        [(buf, o) for o, _ in one] + self.pad, None)
        self.S.sync()
        return self.fetch_raw(buf, lay)

    def plan(self, rects):
        return self.S.yuv_upscale_rect_list_plan(self.fmt, self.w, self.h, self.mul, self.filt, rects)


def border_rig(S, cell):
    from test_gpu_yuv_ex import frame
    layout, chroma, depth, msb = cell
    return YuvListRig(S, *frame(W, H, chroma, depth, FRAME_SEED), layout, chroma, depth, msb, 2.0, 2)


def border_digest(S, cell):
    return digest(border_rig(S, cell).raw_run(snapped(border_rects(), cell[1])))


def mode_unfused():
    import libsrcnn_amd as S
    S.init(0)
    assert "SRCNN_YUV_RECT_LIST_UNFUSED=1" in S.debug_settings()
    res = {}
    for cell in BORDER_CELLS:
        rects = snapped(border_rects(), cell[1])
        p = border_rig(S, cell).plan(rects)
        assert p.batched_items == 0 and p.single_items == len(rects) and p.atlases == 0
        res["/".join(str(v) for v in cell)] = border_digest(S, cell)
    return res


if __name__ == "__main__":
    result = {"unfused": mode_unfused}[sys.argv[1]]()
    print("RESULT " + json.dumps(result))
