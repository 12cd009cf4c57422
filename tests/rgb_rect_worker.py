"""Child processes of tests/test_gpu_rgb_rect.py: things that need a process of their own -- a switch the library reads when it
loads, a second context, torch on the GPU.  Usage: python tests/rgb_rect_worker.py MODE; prints one line "RESULT <json>".
"""
import hashlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
CANARY = 0xA5


def digest(*arrays):
    return hashlib.sha256(b"".join(np.ascontiguousarray(a).tobytes() for a in arrays)).hexdigest()


def arranged(img, layout, order):
    c = img.shape[2]
    a = img[..., ([2, 1, 0] if order == "bgr" else [0, 1, 2]) + ([3] if c == 4 else [])]
    return np.ascontiguousarray(a.transpose(2, 0, 1) if layout == "planar" else a)


def out_size(w, h, mul):
    m = np.float32(mul)
    return int(np.float32(w) * m), int(np.float32(h) * m)


def route_cases():
    """(name, image, layout, order, depth, multiply, filter, rects): up-scales in four format cells, rects at the borders, inside,
    one pixel, and wider than one tile."""
    import test_rgb_restatement as R
    out = []
    cells = (("interleaved", "rgb", 0, 8), ("planar", "bgr", 1, 12), ("interleaved", "bgr", 1, 16), ("planar", "rgb", 0, 10))
    shapes = ((70, 40, 2.0, 2), (37, 21, 2.5, 0), (64, 40, 3.0, 3), (40, 31, 1.5, 1))
    for k, (layout, order, alpha, depth) in enumerate(cells):
        for j in (0, 1):
            w, h, mul, filt = shapes[(k + 2 * j) % 4]
            dw, dh = out_size(w, h, mul)
            rects = [(0, 0, dw, dh), (5, 3, dw - 9, dh - 7), (dw // 2, dh // 2, 1, 1), (dw - 13, 0, 13, dh), (1, dh - 17, min(67, dw - 1), 17)]
            out.append(("%s %s a%d %d-bit %dx%d x%g f%d" % (layout, order, alpha, depth, w, h, mul, filt),
                        R.image(w, h, alpha, depth, 11 * w + h + k), layout, order, depth, mul, filt, rects))
    return out


def run_routes(S):
    """sha256 of (out, conv) over the rects of every route case, in the format's own sample order."""
    res = {}
    for (name, img, layout, order, depth, mul, filt, rects) in route_cases():
        parts = []
        for rect in rects:
            parts += list(S.rgb_upscale_rect(arranged(img, layout, order), rect, multiply=mul, filt=filt, layout=layout, order=order,
                                             depth=depth, want_conv=True))
        res[name] = digest(*parts)
    return res


def mode_unfused():
    import libsrcnn_amd as S
    S.init(0)
    assert "SRCNN_RGB_RECT_UNFUSED=1" in S.debug_settings()
    return run_routes(S)


def mode_second_context():
    """Two virtual contexts on device 0: the same rect through the NULL stream of context 0 and through a stream of context 1
    (made while context 1 is current), from the thread whose current context is 0 again."""
    import libsrcnn_amd as S
    import test_rgb_restatement as R
    assert S.init_devices([0, 0]) == 2
    res = {}
    for k, (alpha, depth, layout, order) in enumerate(((0, 8, "interleaved", "rgb"), (1, 12, "planar", "bgr"))):
        arr = arranged(R.image(97, 61, alpha, depth, 300 + k), layout, order)
        rect = (33, 21, 101, 47)
        S.set_context(0)
        a = S.rgb_upscale_rect(arr, rect, multiply=2.0, filt=2, layout=layout, order=order, depth=depth, want_conv=True)
        S.set_context(1)
        st = S.Stream()
        S.set_context(0)
        b = S.rgb_upscale_rect(arr, rect, multiply=2.0, filt=2, layout=layout, order=order, depth=depth, want_conv=True, stream=st)
        st.destroy()
        res["case%d" % k] = [digest(*a), digest(*b)]
    return res


def mode_torch():
    import torch                      # before the library: both then share torch's HIP runtime
    if not torch.cuda.is_available():
        return {"skip": "torch sees no GPU"}
    import libsrcnn_amd as S
    import test_rgb_restatement as R
    dev = torch.device("cuda", 0)
    res = {"device": str(dev)}
    # (H, W, 3) uint8, out=None: a new rw x rh tensor
    img = R.image(37, 21, 0, 8, 11)
    t = torch.from_numpy(img).to(dev)
    rect = (5, 3, 41, 20)
    out, conv = S.rgb_upscale_rect_torch(t, rect, 2.0, S.SRCNNF_Bicubic, want_conv=True)
    res["new"] = {"sha": digest(out.cpu().numpy(), conv.cpu().numpy()), "device": str(out.device), "shape": list(out.shape),
                  "contig": bool(out.is_contiguous())}
    # in place into a full-size (dh, dw, 3) image filled with a canary: the view of the rect comes back, the rest stays
    full = torch.full((42, 74, 3), CANARY, dtype=torch.uint8, device=dev)
    view, conv = S.rgb_upscale_rect_torch(t, rect, 2.0, S.SRCNNF_Bicubic, want_conv=True, out=full)
    torch.cuda.synchronize()
    host = full.cpu().numpy()
    inside = host[3:23, 5:46].copy()
    host[3:23, 5:46] = CANARY
    res["inplace"] = {"sha": digest(view.cpu().numpy(), conv.cpu().numpy()), "same_memory": view.data_ptr() == full[3:23, 5:46].data_ptr(),
                      "inside_sha": digest(inside, conv.cpu().numpy()), "rest_untouched": bool(np.all(host == CANARY)),
                      "shape": list(view.shape)}
    # ... and into a row-padded full-size image (a view of a wider tensor)
    wide = torch.full((42, 80, 3), CANARY, dtype=torch.uint8, device=dev)
    view, _ = S.rgb_upscale_rect_torch(t, rect, 2.0, S.SRCNNF_Bicubic, out=wide[:, :74, :])
    torch.cuda.synchronize()
    host = wide.cpu().numpy()
    inside = host[3:23, 5:46].copy()
    host[3:23, 5:46] = CANARY
    res["padded"] = {"inside_sha": digest(inside), "rest_untouched": bool(np.all(host == CANARY))}
    # (4, H, W) 16-bit words at depth 12, BGR order, on a side stream; new tensor and in place
    img = R.image(30, 11, 1, 12, 12)
    chw = np.ascontiguousarray(img[..., [2, 1, 0, 3]].transpose(2, 0, 1)).astype(np.int16)
    t = torch.from_numpy(chw).to(dev)
    rect = (7, 2, 33, 19)
    side = torch.cuda.Stream(dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    full = torch.full((4, 27, 75), 0x5A5A, dtype=torch.int16, device=dev)
    with torch.cuda.stream(side):
        out, conv = S.rgb_upscale_rect_torch(t, rect, 2.5, S.SRCNNF_Lanczos3, want_conv=True, order="bgr", depth=12)
        view, _ = S.rgb_upscale_rect_torch(t, rect, 2.5, S.SRCNNF_Lanczos3, order="bgr", depth=12, out=full)
    side.synchronize()
    o = out.cpu().numpy().astype(np.uint16).transpose(1, 2, 0)[..., [2, 1, 0, 3]]
    host = full.cpu().numpy()
    inside = host[:, 2:21, 7:40].astype(np.uint16).transpose(1, 2, 0)[..., [2, 1, 0, 3]]
    host[:, 2:21, 7:40] = 0x5A5A
    res["chw4"] = {"sha": digest(o, conv.cpu().numpy().astype(np.uint16)), "device": str(out.device), "shape": list(out.shape),
                   "inside_sha": digest(inside), "rest_untouched": bool(np.all(host == 0x5A5A)), "view_shape": list(view.shape)}
    # what the call cannot do
    refused = []
    img8 = torch.from_numpy(R.image(37, 21, 0, 8, 11)).to(dev)
    for kw in (dict(rect=(70, 0, 5, 5)), dict(rect=(0, 0, 0, 5)), dict(rect=(0, 0, 5, 5), out=torch.zeros((42, 73, 3), dtype=torch.uint8, device=dev)),
               dict(rect=(0, 0, 5, 5), out=torch.zeros((3, 42, 74), dtype=torch.uint8, device=dev)),
               dict(rect=(0, 0, 5, 5), out=torch.zeros((42, 74, 3), dtype=torch.int16, device=dev))):
        try:
            S.rgb_upscale_rect_torch(img8, kw.pop("rect"), 2.0, S.SRCNNF_Bicubic, **kw)
            refused.append(False)
        except ValueError:
            refused.append(True)
    res["refused"] = refused
    return res


if __name__ == "__main__":
    result = {"unfused": mode_unfused, "second_context": mode_second_context, "torch": mode_torch}[sys.argv[1]]()
    print("RESULT " + json.dumps(result))
