"""Child processes of tests/test_gpu_rgb.py: things that need a process of their own -- a switch the library reads when it
loads, a second context, torch on the GPU.  Usage: python tests/rgb_worker.py MODE; prints one line "RESULT <json>".
"""
import hashlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def digest(*arrays):
    return hashlib.sha256(b"".join(np.ascontiguousarray(a).tobytes() for a in arrays)).hexdigest()


def shell_cases():
    """(name, image, multiply, filter) of the fast-path / general-path comparison: small sizes and one the fused shell
    certainly takes."""
    import test_rgb_restatement as R
    out = []
    for (w, h, mul, filt) in ((23, 17, 2.0, 2), (64, 40, 3.0, 3), (37, 21, 2.5, 0), (512, 300, 2.0, 2), (640, 360, 1.5, 1)):
        for alpha in (0, 1):
            out.append(("%dx%dx%d x%g f%d" % (w, h, 3 + alpha, mul, filt), R.image(w, h, alpha, 8, 7 * w + h), mul, filt))
    return out


def run_shell(S):
    """sha256 of (out, conv) of every shell case through the tight interleaved RGB call."""
    return {name: digest(*S.rgb_upscale(img, multiply=mul, filt=filt, want_conv=True)) for (name, img, mul, filt) in shell_cases()}


def mode_unfused():
    import libsrcnn_amd as S
    S.init(0)
    assert "SRCNN_SHELL_UNFUSED=1" in S.debug_settings()
    return run_shell(S)


def mode_second_context():
    """Two virtual contexts on device 0: the same image through the NULL stream of context 0 and through a stream of context 1
    (made while context 1 is current), from the thread whose current context is 0 again."""
    import libsrcnn_amd as S
    import test_rgb_restatement as R
    assert S.init_devices([0, 0]) == 2
    res = {}
    for k, (alpha, depth, layout, order) in enumerate(((0, 8, "interleaved", "rgb"), (1, 12, "planar", "bgr"))):
        img = R.image(97, 61, alpha, depth, 300 + k)
        arr = img if order == "rgb" else img[..., [2, 1, 0, 3][:3 + alpha]]
        arr = np.ascontiguousarray(arr if layout == "interleaved" else arr.transpose(2, 0, 1))
        S.set_context(0)
        a = S.rgb_upscale(arr, multiply=2.0, filt=2, layout=layout, order=order, depth=depth, want_conv=True)
        S.set_context(1)
        st = S.Stream()
        S.set_context(0)
        b = S.rgb_upscale(arr, multiply=2.0, filt=2, layout=layout, order=order, depth=depth, want_conv=True, stream=st)
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
    # (H, W, 3) uint8
    img = R.image(37, 21, 0, 8, 11)
    t = torch.from_numpy(img).to(dev)
    out, conv = S.rgb_upscale_torch(t, 2.0, S.SRCNNF_Bicubic, want_conv=True)
    res["hwc3"] = {"sha": digest(out.cpu().numpy(), conv.cpu().numpy()), "device": str(out.device), "shape": list(out.shape),
                   "contig": bool(out.is_contiguous())}
    # (4, H, W) 16-bit words at depth 12, BGR order, on a side stream
    img = R.image(30, 11, 1, 12, 12)
    chw = np.ascontiguousarray(img[..., [2, 1, 0, 3]].transpose(2, 0, 1)).astype(np.int16)
    t = torch.from_numpy(chw).to(dev)
    side = torch.cuda.Stream(dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        out, conv = S.rgb_upscale_torch(t, 2.5, S.SRCNNF_Lanczos3, want_conv=True, order="bgr", depth=12)
    side.synchronize()
    o = out.cpu().numpy().astype(np.uint16).transpose(1, 2, 0)[..., [2, 1, 0, 3]]
    res["chw4"] = {"sha": digest(o, conv.cpu().numpy().astype(np.uint16)), "device": str(out.device), "shape": list(out.shape)}
    # a row-strided view: columns 3..40 of a wider (H, W, 3) image
    wide = R.image(48, 19, 0, 8, 13)
    view = torch.from_numpy(wide).to(dev)[:, 3:40, :]
    assert not view.is_contiguous()
    out, conv = S.rgb_upscale_torch(view, 1.5, S.SRCNNF_Bilinear, want_conv=True)
    res["strided"] = {"sha": digest(out.cpu().numpy(), conv.cpu().numpy()), "device": str(out.device), "shape": list(out.shape)}
    # a permuted CHW tensor is planar memory behind an (H, W, C) shape
    t = torch.from_numpy(np.ascontiguousarray(wide.transpose(2, 0, 1))).to(dev).permute(1, 2, 0)
    out, _ = S.rgb_upscale_torch(t, 2.0, S.SRCNNF_Bicubic)
    res["permuted"] = {"sha": digest(out.cpu().numpy()), "shape": list(out.shape), "strides": list(out.stride())}
    # layouts the format cannot express
    refused = []
    for bad in (torch.from_numpy(wide).to(dev)[:, ::2, :], torch.from_numpy(wide).to(dev).float(), torch.from_numpy(wide),
                torch.zeros((5, 7, 9), dtype=torch.uint8, device=dev), torch.from_numpy(wide).to(dev)[..., :2]):
        try:
            S.rgb_upscale_torch(bad)
            refused.append(False)
        except ValueError:
            refused.append(True)
    res["refused"] = refused
    return res


if __name__ == "__main__":
    result = {"unfused": mode_unfused, "second_context": mode_second_context, "torch": mode_torch}[sys.argv[1]]()
    print("RESULT " + json.dumps(result))
