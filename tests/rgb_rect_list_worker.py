"""What tests/test_gpu_rgb_rect_list.py shares with its child processes, and the children themselves: a switch the library reads
when it loads and torch on the GPU need processes of their own.  Usage: python tests/rgb_rect_list_worker.py MODE; prints one
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

from rect_list_worker import DH, DW, H, W, border_rects, seeded_rects      # noqa: E402  (the Y list's frame and lists)

CANARY = 0xA5
BORDER_CELL = ("interleaved", "rgb", 0, 8)
BORDER_SEED = 9656


def arrange(img, layout, order):
    """(h, w, c) in R, G, B[, A] order -> the array the format holds: channels reordered, (c, h, w) when planar."""
    c = img.shape[2]
    a = img[..., ([2, 1, 0] if order == "bgr" else [0, 1, 2]) + ([3] if c == 4 else [])]
    return np.ascontiguousarray(a.transpose(2, 0, 1) if layout == "planar" else a)


def canonical(arr, layout, order):
    """The inverse of arrange."""
    a = arr.transpose(1, 2, 0) if layout == "planar" else arr
    c = a.shape[2]
    return np.ascontiguousarray(a[..., ([2, 1, 0] if order == "bgr" else [0, 1, 2]) + ([3] if c == 4 else [])])


def digest(pairs):
    return hashlib.sha256(b"".join(np.ascontiguousarray(a).tobytes() for p in pairs for a in p)).hexdigest()


class RgbListRig:
    """One source image in device memory (tight) in a format; run() is one list call with every rect (and its dst_conv) in a
    tight region of its own, loop() the same rects through single calls into the same layout.  Results come back as
    (out, conv) pairs, out in R, G, B[, A] order shaped (rh, rw, c)."""

    def __init__(self, S, img, layout, order, depth, mul=2.0, filt=2):
        self.S, self.layout, self.order, self.depth, self.mul, self.filt = S, layout, order, depth, mul, filt
        self.h, self.w, self.c = img.shape
        self.planar = layout == "planar"
        self.dt = np.uint8 if depth == 8 else np.uint16
        self.bps = np.dtype(self.dt).itemsize
        self.dw, self.dh = S.output_size(self.w, self.h, mul)
        self.fmt = S.rgb_format(layout, order, self.c == 4, depth)
        self.din = S.DeviceBuffer.from_numpy(arrange(img, layout, order))
        self.src = [(self.din, k * self.w * self.h * self.bps) for k in range(self.c)] if self.planar else [self.din]

    def layout_of(self, rects):
        offs, total = [], 0
        for (_, _, rw, rh) in rects:
            o_img = total
            total += (rw * rh * self.c * self.bps + 15) & ~15
            offs.append((o_img, total))
            total += (rw * rh * self.bps + 15) & ~15
        return offs, max(16, total)

    def dst_of(self, buf, o_img, rw, rh):
        return [(buf, o_img + k * rw * rh * self.bps) for k in range(self.c)] if self.planar else [(buf, o_img)]

    def queue(self, rects, stream=None):
        """Queues one list call; returns (buffer, offsets)."""
        offs, total = self.layout_of(rects)
        buf = self.S.DeviceBuffer(total)
        items = [(x0, y0, rw, rh, self.dst_of(buf, oi, rw, rh), None, (buf, oc), 0) for (x0, y0, rw, rh), (oi, oc) in zip(rects, offs)]
        self.S.rgb_upscale_rect_list_dev(self.fmt, self.w, self.h, self.mul, self.filt, self.src, None, items, stream)
        return buf, offs

    def fetch(self, rects, buf, offs):
        flat = buf.to_numpy(np.uint8, (buf.nbytes,))
        res = []
        for (_, _, rw, rh), (oi, oc) in zip(rects, offs):
            out = flat[oi:oi + rw * rh * self.c * self.bps].view(self.dt).reshape((self.c, rh, rw) if self.planar else (rh, rw, self.c))
            res.append((canonical(out, self.layout, self.order), flat[oc:oc + rw * rh * self.bps].view(self.dt).reshape(rh, rw).copy()))
        return res

    def run(self, rects):
        buf, offs = self.queue(rects)
        self.S.sync()
        return self.fetch(rects, buf, offs)

    def loop(self, rects):
        offs, total = self.layout_of(rects)
        buf = self.S.DeviceBuffer(total)
        for (x0, y0, rw, rh), (oi, oc) in zip(rects, offs):
            self.S.rgb_upscale_rect_dev(self.fmt, self.w, self.h, self.mul, self.filt, self.src, None, x0, y0, rw, rh, self.dst_of(buf, oi, rw, rh), None,
                                        (buf, oc), 0)
        self.S.sync()
        return self.fetch(rects, buf, offs)

    def plan(self, rects):
        return self.S.rgb_upscale_rect_list_plan(self.fmt, self.w, self.h, self.mul, self.filt, rects)


def border_image():
    import test_rgb_restatement as R
    return R.image(W, H, BORDER_CELL[2], BORDER_CELL[3], BORDER_SEED)


def border_digest(S):
    return digest(RgbListRig(S, border_image(), *BORDER_CELL[:2], BORDER_CELL[3]).run(border_rects()))


def mode_unfused():
    import libsrcnn_amd as S
    S.init(0)
    assert "SRCNN_RGB_RECT_LIST_UNFUSED=1" in S.debug_settings()
    rig = RgbListRig(S, border_image(), *BORDER_CELL[:2], BORDER_CELL[3])
    p = rig.plan(border_rects())
    assert p.batched_items == 0 and p.single_items == len(border_rects()) and p.atlases == 0
    return {"borders": border_digest(S)}


def torch_rects():
    return seeded_rects(4242, 12) + [(0, 0, 1, 1), (DW - 1, DH - 1, 1, 1), (130, 40, 62, 72)]


def mode_torch():
    import torch                      # before the library: both then share torch's HIP runtime
    if not torch.cuda.is_available():
        return {"skip": "torch sees no GPU"}
    import libsrcnn_amd as S
    import test_rgb_restatement as R
    dev = torch.device("cuda", 0)
    rects = torch_rects()
    res = {"device": str(dev)}
    # (H, W, 3) uint8 into a canary-filled full-size (dh, dw, 3) image
    t = torch.from_numpy(R.image(W, H, 0, 8, 31)).to(dev)
    full = torch.full((DH, DW, 3), CANARY, dtype=torch.uint8, device=dev)
    back = S.rgb_upscale_rect_list_torch(t, rects, full)
    torch.cuda.synchronize()
    res["hwc"] = {"sha": digest([(full.cpu().numpy(),)]), "same": back is full}
    # (4, H, W) 16-bit words at depth 12, BGR order, into a row-padded full-size CHW image (a view of a wider tensor)
    chw = np.ascontiguousarray(R.image(W, H, 1, 12, 32)[..., [2, 1, 0, 3]].transpose(2, 0, 1)).astype(np.int16)
    t = torch.from_numpy(chw).to(dev)
    wide = torch.full((4, DH, DW + 6), 0x5A5A, dtype=torch.int16, device=dev)
    S.rgb_upscale_rect_list_torch(t, rects, wide[:, :, :DW], order="bgr", depth=12)
    torch.cuda.synchronize()
    res["chw"] = {"sha": digest([(wide.cpu().numpy().astype(np.uint16),)])}
    # n == 0: nothing is touched
    S.rgb_upscale_rect_list_torch(t, [], wide[:, :, :DW], order="bgr", depth=12)
    torch.cuda.synchronize()
    res["empty"] = {"sha": digest([(wide.cpu().numpy().astype(np.uint16),)])}
    refused = []
    for kw in (dict(rects=[(190, 0, 5, 5)], out=full), dict(rects=[(0, 0, 5, 5)], out=torch.zeros((DH, DW - 1, 3), dtype=torch.uint8, device=dev)),
               dict(rects=[(0, 0, 5, 5)], out=torch.zeros((3, DH, DW), dtype=torch.uint8, device=dev))):
        try:
            S.rgb_upscale_rect_list_torch(torch.from_numpy(R.image(W, H, 0, 8, 31)).to(dev), kw["rects"], kw["out"])
            refused.append(False)
        except ValueError:
            refused.append(True)
    res["refused"] = refused
    return res


if __name__ == "__main__":
    result = {"unfused": mode_unfused, "torch": mode_torch}[sys.argv[1]]()
    print("RESULT " + json.dumps(result))
