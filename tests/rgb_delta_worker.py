"""What tests/test_gpu_rgb_delta.py shares with its child process, and the child itself: torch on the GPU needs a process of its
own (torch is imported before the library, so that both share torch's HIP runtime).  Usage: python tests/rgb_delta_worker.py torch;
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

from rect_list_worker import DH, DW, H, W      # noqa: E402  (the Y list's frame)


def digest(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def torch_frames():
    """Two (H, W, 3) uint8 images in R, G, B order: the second has a 7 x 4 block and one far pixel changed."""
    import test_rgb_restatement as R
    a = R.image(W, H, 0, 8, 31)
    b = np.array(a, copy=True)
    b[20:24, 30:37] ^= 0x40
    b[50, 90, 2] ^= 1
    return a, b


def mode_torch():
    import torch                      # before the library: both then share torch's HIP runtime
    if not torch.cuda.is_available():
        return {"skip": "torch sees no GPU"}
    import libsrcnn_amd as S
    dev = torch.device("cuda", 0)
    a, b = torch_frames()
    ta, tb = torch.from_numpy(a).to(dev), torch.from_numpy(b).to(dev)
    res = {"device": str(dev)}
    stats = lambda st: {"tiles": st.tiles, "dirty_tiles": st.dirty_tiles, "rects": st.rects, "whole_frame": st.whole_frame}   # noqa: E731
    # no previous image: the whole image, into a tensor of garbage
    out = torch.full((DH, DW, 3), 0xA5, dtype=torch.uint8, device=dev)
    st = S.rgb_upscale_delta_torch(None, ta, out, tile=(32, 16))
    torch.cuda.synchronize()
    res["first"] = dict(stats(st), sha=digest(out.cpu().numpy()))
    # the next frame: only what changed, in place
    st = S.rgb_upscale_delta_torch(ta, tb, out, tile=(32, 16))
    torch.cuda.synchronize()
    res["second"] = dict(stats(st), sha=digest(out.cpu().numpy()))
    # the same step into a row-padded image (a view of a wider tensor) that holds frame a's result
    wide = torch.full((DH, DW + 5, 3), 0x5A, dtype=torch.uint8, device=dev)
    S.rgb_upscale_delta_torch(None, ta, wide[:, :DW])
    S.rgb_upscale_delta_torch(ta, tb, wide[:, :DW], tile=(32, 16))
    torch.cuda.synchronize()
    res["padded"] = {"sha": digest(wide.cpu().numpy())}
    # nothing changed: nothing is queued, nothing is touched
    st = S.rgb_upscale_delta_torch(tb, tb.clone(), out)
    torch.cuda.synchronize()
    res["unchanged"] = {"sha": digest(out.cpu().numpy()), "rects": st.rects, "dirty_tiles": st.dirty_tiles}
    refused = []
    for kw in (dict(prev=ta[:, :W - 1], out=out), dict(prev=ta, out=torch.zeros((DH, DW - 1, 3), dtype=torch.uint8, device=dev)),
               dict(prev=ta, out=torch.zeros((3, DH, DW), dtype=torch.uint8, device=dev))):
        try:
            S.rgb_upscale_delta_torch(kw["prev"], tb, kw["out"])
            refused.append(False)
        except ValueError:
            refused.append(True)
    res["refused"] = refused
    return res


if __name__ == "__main__":
    result = {"torch": mode_torch}[sys.argv[1]]()
    print("RESULT " + json.dumps(result))
