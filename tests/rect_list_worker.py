"""What tests/test_gpu_rect_list.py shares with its child process, and the child itself: SRCNN_RECT_LIST_UNFUSED is read when
the library loads, so the forced single route needs a process of its own.  Usage: python tests/rect_list_worker.py MODE; prints
one line "RESULT <json>".
"""
import hashlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

W, H, DW, DH = 96, 56, 192, 112          # the frame of most cases: 3 tile columns x 7 tile rows of the layer kernels
FRAME_SEED_OFFSET = 501


def frame_plane():
    from libsrcnn_amd import synth
    return synth.plane(H, W, synth.SEED0 + FRAME_SEED_OFFSET, "noise")


def border_rects(dw=DW, dh=DH):
    """The border list of the issue: the four 1 x 1 corners; rects that touch one edge with their other edges 1, 5, 6 and 7
    samples from a border; an interior 1 x 1; cells of 63, 64, 65 and 129 columns; the full frame.  (x0, y0, rw, rh)."""
    r = [(0, 0, 1, 1), (dw - 1, 0, 1, 1), (0, dh - 1, 1, 1), (dw - 1, dh - 1, 1, 1)]
    for d in (1, 5, 6, 7):
        r += [(0, d, dw - d, dh - 2 * d),            # left edge
              (d, d, dw - d, dh - 2 * d),            # right edge
              (d, 0, dw - 2 * d, dh - d),            # top edge
              (d, d, dw - 2 * d, dh - d)]            # bottom edge
        r += [(0, d, 3 + d, 9), (dw - 3 - d, dh - 9 - d, 3 + d, 9), (d, 0, 9, 3 + d), (dw - 9 - d, dh - 3 - d, 9, 3 + d)]    # the same, small
    r += [(97, 55, 1, 1)]
    r += [(20 + k, 30 + k, cw - 12, 10 + k) for k, cw in enumerate((63, 64, 65, 129))]
    r += [(0, 0, dw, dh)]
    return r


def seeded_rects(seed, n, dw=DW, dh=DH, lo=1, hi=40):
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(n):
        rw, rh = int(rng.integers(lo, min(hi, dw) + 1)), int(rng.integers(lo, min(hi, dh) + 1))
        out.append((int(rng.integers(0, dw - rw + 1)), int(rng.integers(0, dh - rh + 1)), rw, rh))
    return out


class ListRig:
    """One source plane in device memory (tight, or pitched with NaN padding); run() is one list call with every rect in a
    tight region of its own, loop() the same rects through single calls."""

    def __init__(self, S, y, dw, dh, filt=2, pad_cols=0):
        self.S, self.dw, self.dh, self.filt = S, dw, dh, filt
        self.h, self.w = y.shape
        src = np.full((self.h, self.w + pad_cols), np.nan, np.float32)
        src[:, :self.w] = y
        self.in_pitch = 4 * (self.w + pad_cols) if pad_cols else 0
        self.din = S.DeviceBuffer.from_numpy(src)

    def layout(self, rects):
        offs, total = [], 0
        for (_, _, rw, rh) in rects:
            offs.append(total)
            total += (4 * rw * rh + 15) & ~15
        return offs, max(16, total)

    def queue(self, rects, stream=None):
        """Queues one list call; returns (buffer, offsets)."""
        offs, total = self.layout(rects)
        buf = self.S.DeviceBuffer(total)
        self.S.y_path_rect_list_dev(self.din, self.in_pitch, self.w, self.h, self.dw, self.dh, self.filt,
                                    [(x0, y0, rw, rh, (buf, o), 0) for (x0, y0, rw, rh), o in zip(rects, offs)], stream)
        return buf, offs

    def fetch(self, rects, buf, offs):
        flat = buf.to_numpy(np.uint8, (buf.nbytes,))
        return [flat[o:o + 4 * rw * rh].view(np.float32).reshape(rh, rw).copy() for (_, _, rw, rh), o in zip(rects, offs)]

    def run(self, rects):
        buf, offs = self.queue(rects)
        self.S.sync()
        return self.fetch(rects, buf, offs)

    def loop(self, rects):
        offs, total = self.layout(rects)
        buf = self.S.DeviceBuffer(total)
        for (x0, y0, rw, rh), o in zip(rects, offs):
            self.S.y_path_rect_dev(self.din, self.in_pitch, self.w, self.h, self.dw, self.dh, self.filt, x0, y0, rw, rh, (buf, o), 0)
        self.S.sync()
        return self.fetch(rects, buf, offs)

    def plan(self, rects):
        return self.S.y_path_rect_list_plan(self.w, self.h, self.dw, self.dh, self.filt, rects)


def digest(arrays):
    return hashlib.sha256(b"".join(np.ascontiguousarray(a).tobytes() for a in arrays)).hexdigest()


def border_digest(S):
    return digest(ListRig(S, frame_plane(), DW, DH).run(border_rects()))


def main():
    import libsrcnn_amd as S
    mode = sys.argv[1]
    S.init(0)
    if mode == "unfused":
        assert "SRCNN_RECT_LIST_UNFUSED=1" in S.debug_settings()
        rig = ListRig(S, frame_plane(), DW, DH)
        p = rig.plan(border_rects())
        assert p.batched_items == 0 and p.single_items == len(border_rects()) and p.atlases == 0
        print("RESULT " + json.dumps({"borders": border_digest(S)}))
    else:
        raise SystemExit("unknown mode " + mode)


if __name__ == "__main__":
    main()
