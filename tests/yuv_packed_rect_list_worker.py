"""What tests/test_gpu_yuv_packed_rect_list.py shares with its child processes, and the children themselves: things that need a
process of their own -- SRCNN_YUV_PACKED_RECT_LIST_UNFUSED is read when the library loads, and a stream capture of the caller's
is kept away from the suite's process.  Usage: python tests/yuv_packed_rect_list_worker.py MODE; prints one line "RESULT <json>".
"""
import ctypes as C
import hashlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from rect_list_worker import DH, DW, H, W, seeded_rects  # noqa: E402
from yuv_packed_rect_worker import NAMES, snap, span  # noqa: E402

MAIN = (W, H, 2, 2.0)                    # (w, h, filter, multiply): 96 x 56 -> 192 x 112, 2x bicubic, the frame of tests/rect_list_worker.py
CAPTURE_NAMES = ("yuy2", "y410", "v210")


def source(name, case):
    """The packed source frame whose expectation test_gpu_yuv_packed.want_for(oracle_lib, name, case) holds."""
    from test_gpu_yuv_packed import frame_planes, pack
    w, h, _filt, _mul = case
    return pack(name, *frame_planes(name, w, h, 100 * w + h))


def snapped(rects, name, dw):
    """Every rect under the unit rule, without repeats, in order."""
    out, seen = [], set()
    for r in rects:
        r = snap(r, name, dw)
        if r not in seen:
            seen.add(r)
            out.append(r)
    return out


def main_rects(name, k=0):
    return snapped(seeded_rects(300 + k, 32) + [(0, 0, DW, DH)], name, DW)


class PackedListRig:
    """One packed source frame in device memory (tight); run() is one list call with every rect's row segments in a tight region
    of its own, loop() the same rects through single calls."""

    def __init__(self, S, name, src, w, mul=2.0, filt=2):
        self.S, self.name, self.w, self.mul, self.filt = S, name, w, mul, filt
        self.h = src.shape[0]
        self.dw, self.dh = S.output_size(w, self.h, mul)
        self.din = S.DeviceBuffer.from_numpy(np.ascontiguousarray(src, np.uint8))

    def layout(self, rects):
        offs, total = [], 0
        for (x0, _y0, rw, rh) in rects:
            offs.append(total)
            total += (rh * span(self.name, self.dw, x0, rw)[1] + 15) & ~15
        return offs, max(16, total)

    def items(self, rects, buf, offs):
        return [(x0, y0, rw, rh, (buf, o), 0) for (x0, y0, rw, rh), o in zip(rects, offs)]

    def queue(self, rects, stream=None):
        """Queues one list call; returns (rects, buffer, offsets)."""
        offs, total = self.layout(rects)
        buf = self.S.DeviceBuffer.from_numpy(np.full(total, 0x5A, np.uint8))
        self.S.yuv_packed_upscale_rect_list_dev(self.name, self.w, self.h, self.mul, self.filt, self.din, 0, self.items(rects, buf, offs), stream)
        return rects, buf, offs

    def fetch(self, rects, buf, offs):
        flat = buf.to_numpy(np.uint8, (buf.nbytes,))
        out = []
        for (x0, _y0, rw, rh), o in zip(rects, offs):
            n = span(self.name, self.dw, x0, rw)[1]
            out.append(flat[o:o + rh * n].reshape(rh, n).copy())
        return out

    def run(self, rects):
        q = self.queue(rects)
        self.S.sync()
        return self.fetch(*q)

    def loop(self, rects, stream=None):
        offs, total = self.layout(rects)
        buf = self.S.DeviceBuffer.from_numpy(np.full(total, 0x5A, np.uint8))
        for (x0, y0, rw, rh), o in zip(rects, offs):
            self.S.yuv_packed_upscale_rect_dev(self.name, self.w, self.h, self.mul, self.filt, self.din, 0, x0, y0, rw, rh, (buf, o), 0, stream)
        if stream is None:
            self.S.sync()
        return rects, buf, offs

    def plan(self, rects):
        return self.S.yuv_packed_upscale_rect_list_plan(self.name, self.w, self.h, self.mul, self.filt, rects)


def digest(arrays):
    return hashlib.sha256(b"".join(np.ascontiguousarray(a).tobytes() for a in arrays)).hexdigest()


def main_digest(S, name):
    return digest(PackedListRig(S, name, source(name, MAIN), W).run(main_rects(name, NAMES.index(name))))


def mode_unfused(S):
    assert "SRCNN_YUV_PACKED_RECT_LIST_UNFUSED=1" in S.debug_settings()
    for name in NAMES:
        rects = main_rects(name, NAMES.index(name))
        p = PackedListRig(S, name, source(name, MAIN), W).plan(rects)
        assert p.batched_items == 0 and p.single_items == len(rects) and p.atlases == 0, name
    return {name: main_digest(S, name) for name in NAMES}


def mode_capture(S):
    """A list issued while the CALLER captures its stream runs every item the single way, is recorded, and gives the loop's bytes
    when the graph is replayed."""
    hip = None
    for lib in ("libamdhip64.so.7", "libamdhip64.so", "/opt/rocm/lib/libamdhip64.so"):
        try:
            hip = C.CDLL(lib)
            break
        except OSError:
            continue
    assert hip is not None, "no libamdhip64 to capture a stream with"
    vp = C.c_void_p
    hip.hipStreamBeginCapture.argtypes = [vp, C.c_int]
    hip.hipStreamEndCapture.argtypes = [vp, C.POINTER(vp)]
    hip.hipGraphInstantiate.argtypes = [C.POINTER(vp), vp, vp, vp, C.c_size_t]
    hip.hipGraphLaunch.argtypes = [vp, vp]
    hip.hipStreamSynchronize.argtypes = [vp]
    hip.hipGraphExecDestroy.argtypes = [vp]
    hip.hipGraphDestroy.argtypes = [vp]
    hip.hipStreamDestroy.argtypes = [vp]
    out = {}
    for name in CAPTURE_NAMES:
        rig = PackedListRig(S, name, source(name, MAIN), W)
        rects = main_rects(name, NAMES.index(name))[:12]
        raw = vp()
        assert hip.hipStreamCreateWithFlags(C.byref(raw), 1) == 0          # hipStreamNonBlocking
        try:
            # the loop first, eagerly on the same stream: the expectation, and every table and scratch block the capture needs
            want_q = rig.loop(rects, raw)
            assert hip.hipStreamSynchronize(raw) == 0
            want = rig.fetch(*want_q)
            offs, total = rig.layout(rects)
            buf = S.DeviceBuffer.from_numpy(np.full(total, 0x5A, np.uint8))
            graph, ex = vp(), vp()
            assert hip.hipStreamBeginCapture(raw, 2) == 0                  # hipStreamCaptureModeRelaxed
            try:
                S.yuv_packed_upscale_rect_list_dev(name, rig.w, rig.h, rig.mul, rig.filt, rig.din, 0, rig.items(rects, buf, offs), raw.value)
            finally:
                rc = hip.hipStreamEndCapture(raw, C.byref(graph))
            assert rc == 0 and graph.value, rc
            before = rig.fetch(rects, buf, offs)
            assert all(np.all(b == 0x5A) for b in before), "the captured call must not have run yet"
            assert hip.hipGraphInstantiate(C.byref(ex), graph, None, None, 0) == 0
            assert hip.hipGraphLaunch(ex, raw) == 0
            assert hip.hipStreamSynchronize(raw) == 0
            got = rig.fetch(rects, buf, offs)
            out[name] = bool(all(np.array_equal(g, e) for g, e in zip(got, want)))
            hip.hipGraphExecDestroy(ex)
            hip.hipGraphDestroy(graph)
        finally:
            hip.hipStreamDestroy(raw)
    return out


if __name__ == "__main__":
    import libsrcnn_amd as S
    S.init(0)
    print("RESULT " + json.dumps({"unfused": mode_unfused, "capture": mode_capture}[sys.argv[1]](S)))
