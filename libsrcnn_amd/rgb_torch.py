"""The RGB(A) calls on torch tensors that live on a GPU: no copies, queued on torch's current stream.  torch is imported by the
calls, never by importing this module."""
import collections
import os

from .abi import SRCNNF_Bicubic
from .core import init, lib, output_size
from .rgb import RGB_INTERLEAVED, RGB_PLANAR, rgb_format, rgb_upscale_delta_dev, rgb_upscale_dev, rgb_upscale_rect_dev, rgb_upscale_rect_list_dev

__all__ = ["rgb_upscale_torch", "rgb_upscale_rect_torch", "rgb_upscale_rect_list_torch", "rgb_upscale_delta_torch"]


def _one_hip_runtime():
    """torch wheels carry a HIP runtime of their own.  When torch is imported first this library binds to that copy and both
    share one runtime; the other way round the process holds two, and memory of one is unknown to the other."""
    seen = set()
    try:
        with open("/proc/self/maps") as f:
            for line in f:
                path = line.rsplit(None, 1)[-1]
                if "/libamdhip64.so" in path:
                    seen.add(os.path.realpath(path))
    except OSError:
        return
    if len(seen) > 1:
        raise RuntimeError("two HIP runtimes are loaded (%s): import torch before the first libsrcnn_amd call so that both use "
                           "the same one" % ", ".join(sorted(seen)))


# W, H, C, bytes per sample, depth, channels-last shape?, SRCNN_RGB_* layout, row stride, channel stride -- strides in samples
_TorchImage = collections.namedtuple("_TorchImage", "W H Cn bps depth hwc layout sh sc")


def _rgb_torch_layout(t, depth, who):
    """What the RGB(A) torch calls read off a tensor, as a _TorchImage; ValueError for anything that is not an RGB(A) image in
    GPU memory."""
    import torch
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise ValueError("%s needs a torch tensor on a GPU" % who)
    sixteen = [torch.int16] + ([torch.uint16] if hasattr(torch, "uint16") else [])
    if t.dtype != torch.uint8 and t.dtype not in sixteen:
        raise ValueError("dtype %s: torch.uint8 or a 16-bit integer type" % (t.dtype,))
    bps = 1 if t.dtype == torch.uint8 else 2
    if depth is None:
        depth = 8 if bps == 1 else 16
    if (depth == 8) != (bps == 1):
        raise ValueError("depth %d does not go with %s" % (depth, t.dtype))
    if t.dim() != 3 or 0 in t.shape:
        raise ValueError("an RGB(A) image is (H, W, C) or (C, H, W), not %r" % (tuple(t.shape),))
    for hwc in (True, False):            # which axis carries the channels, and what the strides say about the memory
        (H, W, Cn) = tuple(t.shape) if hwc else (t.shape[1], t.shape[2], t.shape[0])
        (sh, sw, sc) = t.stride() if hwc else (t.stride(1), t.stride(2), t.stride(0))
        if Cn not in (3, 4):
            continue
        if sc == 1 and sw == Cn and sh >= W * Cn:
            return _TorchImage(W, H, Cn, bps, depth, hwc, RGB_INTERLEAVED, sh, sc)
        if sw == 1 and sh >= W and sc >= 1:
            return _TorchImage(W, H, Cn, bps, depth, hwc, RGB_PLANAR, sh, sc)
    raise ValueError("shape %r with strides %r is neither interleaved pixels nor one plane per channel" % (tuple(t.shape), t.stride()))


def _rgb_torch_context(t):
    """Load the library beside torch's HIP runtime and make sure the current srcnn context is on the tensor's device."""
    import torch
    lib()
    _one_hip_runtime()
    dev = t.device.index if t.device.index is not None else torch.cuda.current_device()
    if lib().srcnn_context_count() == 0:
        init(dev)
    have = lib().srcnn_context_device(lib().srcnn_get_context())
    if have != dev:
        raise ValueError("the tensor lives on device %d, the current srcnn context on device %d (set_context)" % (dev, have))
    return dev


def _planes_of(t, im, x0=0, y0=0):
    """(plane pointers, pitches) of pixel (x0, y0) onwards of tensor t, whose memory _TorchImage im describes."""
    if im.layout == RGB_INTERLEAVED:
        ptrs = [t.data_ptr() + (y0 * im.sh + x0 * im.Cn) * im.bps]
    else:
        ptrs = [t.data_ptr() + (k * im.sc + y0 * im.sh + x0) * im.bps for k in range(im.Cn)]
    return ptrs, [im.sh * im.bps] * len(ptrs)


def _new_like(t, im, w, h):
    """(a new w x h image tensor in the memory layout of t, its plane pointers, the view of it in the shape order of t)."""
    import torch
    if im.layout == RGB_INTERLEAVED:
        buf = torch.empty((h, w, im.Cn), dtype=t.dtype, device=t.device)
        return buf, [buf.data_ptr()], (buf if im.hwc else buf.permute(2, 0, 1))
    buf = torch.empty((im.Cn, h, w), dtype=t.dtype, device=t.device)
    return buf, [buf.data_ptr() + k * h * w * im.bps for k in range(im.Cn)], (buf.permute(1, 2, 0) if im.hwc else buf)


def _checked_out(out, t, im, dw, dh, who, like="t"):
    """The _TorchImage of `out`, which must be a dw x dh image tensor of t's dtype, device, shape order and memory layout."""
    import torch
    if not isinstance(out, torch.Tensor) or out.device != t.device or out.dtype != t.dtype:
        raise ValueError("out must be a tensor of %s on %s" % (t.dtype, t.device))
    o = _rgb_torch_layout(out, im.depth, who)
    if (o.W, o.H, o.Cn, o.hwc, o.layout) != (dw, dh, im.Cn, im.hwc, im.layout):
        raise ValueError("out is %d x %d x %d (%s), the output image %d x %d x %d in the layout of %s" %
                         (o.W, o.H, o.Cn, "interleaved" if o.layout == RGB_INTERLEAVED else "planar", dw, dh, im.Cn, like))
    return o


def _inside(rect, dw, dh):
    x0, y0, rw, rh = (int(v) for v in rect)
    if rw <= 0 or rh <= 0 or x0 < 0 or y0 < 0 or x0 + rw > dw or y0 + rh > dh:
        raise ValueError("rect %r is not inside the %d x %d output" % ((x0, y0, rw, rh), dw, dh))
    return x0, y0, rw, rh


def _stream_of(t):
    import torch
    return torch.cuda.current_stream(t.device).cuda_stream or None


def rgb_upscale_torch(t, multiply=2.0, filt=SRCNNF_Bicubic, want_conv=False, order="rgb", depth=None):
    """srcnn_rgb_upscale_dev on a torch tensor that lives on a GPU: t is torch.uint8 (depth 8) or a 16-bit integer tensor
    (depth 16 unless `depth` says 10 / 12 / 14), shaped (H, W, C) or (C, H, W) with C in (3, 4).  The memory behind it must be
    interleaved pixels (channel stride 1, column stride C) or one plane per channel (column stride 1); rows may be padded --
    the pitch is taken from the strides -- and anything else raises ValueError.  The output tensor (and the truncated Y'
    plane with want_conv) is allocated by torch on the same device, in the same layout; the call is queued on
    torch.cuda.current_stream() and neither copies to the host nor synchronises.  Returns (out, conv | None).
    The tensor's device must be the device of the calling thread's current srcnn context."""
    im = _rgb_torch_layout(t, depth, "rgb_upscale_torch")
    import torch
    _rgb_torch_context(t)
    dw, dh = output_size(im.W, im.H, multiply)
    _out, dst, result = _new_like(t, im, dw, dh)
    src, pitch = _planes_of(t, im)
    conv = torch.empty((dh, dw), dtype=t.dtype, device=t.device) if want_conv else None
    rgb_upscale_dev(rgb_format(im.layout, order, im.Cn == 4, im.depth), im.W, im.H, multiply, filt, src, pitch, dst, None,
                    conv.data_ptr() if want_conv else None, 0, _stream_of(t))
    return result, conv


def rgb_upscale_rect_torch(t, rect, multiply=2.0, filt=SRCNNF_Bicubic, want_conv=False, order="rgb", depth=None, out=None):
    """srcnn_rgb_upscale_rect_dev on a torch tensor that lives on a GPU: pixels rect = (x0, y0, rw, rh) of what
    rgb_upscale_torch(t, ...) returns, at the cost of the rect.  t as for rgb_upscale_torch.  out=None: a new tensor of rw x rh
    pixels in t's layout.  out = a full-size dw x dh image tensor of t's dtype, shape order and memory layout (rows may be
    padded): the rect is written in place through its strides, nothing else of it is touched, and the view of the rect is
    returned.  Queued on torch.cuda.current_stream(); returns (rect tensor, conv | None), conv a new rh x rw tensor."""
    im = _rgb_torch_layout(t, depth, "rgb_upscale_rect_torch")
    import torch
    _rgb_torch_context(t)
    dw, dh = output_size(im.W, im.H, multiply)
    x0, y0, rw, rh = _inside(rect, dw, dh)
    src, pitch = _planes_of(t, im)
    if out is None:
        _buf, dst, result = _new_like(t, im, rw, rh)
        dpitch = None
    else:
        dst, dpitch = _planes_of(out, _checked_out(out, t, im, dw, dh, "rgb_upscale_rect_torch(out=)"), x0, y0)
        result = out[y0:y0 + rh, x0:x0 + rw, :] if im.hwc else out[:, y0:y0 + rh, x0:x0 + rw]
    conv = torch.empty((rh, rw), dtype=t.dtype, device=t.device) if want_conv else None
    rgb_upscale_rect_dev(rgb_format(im.layout, order, im.Cn == 4, im.depth), im.W, im.H, multiply, filt, src, pitch, x0, y0, rw, rh,
                         dst, dpitch, conv.data_ptr() if want_conv else None, 0, _stream_of(t))
    return result, conv


def rgb_upscale_rect_list_torch(t, rects, out, multiply=2.0, filt=SRCNNF_Bicubic, order="rgb", depth=None):
    """srcnn_rgb_upscale_rect_list_dev on torch tensors that live on a GPU: repaints every (x0, y0, rw, rh) of `rects` inside
    `out`, in place and in ONE call.  t as for rgb_upscale_torch; out is a full-size dw x dh image tensor of t's dtype, shape
    order and memory layout (rows may be padded): the rects are written through its strides and nothing else of it is touched.
    Queued on torch.cuda.current_stream(); returns out."""
    im = _rgb_torch_layout(t, depth, "rgb_upscale_rect_list_torch")
    _rgb_torch_context(t)
    dw, dh = output_size(im.W, im.H, multiply)
    o = _checked_out(out, t, im, dw, dh, "rgb_upscale_rect_list_torch(out)")
    items = []
    for r in rects:
        x0, y0, rw, rh = _inside(r, dw, dh)
        items.append((x0, y0, rw, rh) + _planes_of(out, o, x0, y0))
    src, pitch = _planes_of(t, im)
    rgb_upscale_rect_list_dev(rgb_format(im.layout, order, im.Cn == 4, im.depth), im.W, im.H, multiply, filt, src, pitch, items, _stream_of(t))
    return out


def rgb_upscale_delta_torch(prev, cur, out, multiply=2.0, filt=SRCNNF_Bicubic, order="rgb", depth=None, tile=(0, 0)):
    """srcnn_rgb_upscale_delta_dev on torch tensors that live on a GPU: `out`, which holds rgb_upscale_torch(prev, ...), is updated
    in place to rgb_upscale_torch(cur, ...) by repainting only the tiles that can differ.  cur as for rgb_upscale_torch; prev is
    None (no previous image: everything is repainted) or a tensor of cur's shape, dtype, device and memory layout (its row
    padding may differ); out is a full-size dw x dh image tensor of cur's dtype, shape order and memory layout (rows may be
    padded): it is written through its strides and nothing of a clean tile is touched.  The call waits once, for the tile flags,
    on torch.cuda.current_stream(), and queues the repaint there.  Returns the DeltaStats."""
    im = _rgb_torch_layout(cur, depth, "rgb_upscale_delta_torch")
    import torch
    _rgb_torch_context(cur)
    dw, dh = output_size(im.W, im.H, multiply)
    p_src = p_pitch = None
    if prev is not None:
        if not isinstance(prev, torch.Tensor) or prev.device != cur.device or prev.dtype != cur.dtype:
            raise ValueError("prev must be a tensor of %s on %s" % (cur.dtype, cur.device))
        p = _rgb_torch_layout(prev, im.depth, "rgb_upscale_delta_torch(prev)")
        if (p.W, p.H, p.Cn, p.hwc, p.layout) != (im.W, im.H, im.Cn, im.hwc, im.layout):
            raise ValueError("prev is %d x %d x %d, cur %d x %d x %d in another layout or shape order" % (p.W, p.H, p.Cn, im.W, im.H, im.Cn))
        p_src, p_pitch = _planes_of(prev, p)
    dst, dpitch = _planes_of(out, _checked_out(out, cur, im, dw, dh, "rgb_upscale_delta_torch(out)", like="cur"))
    src, pitch = _planes_of(cur, im)
    return rgb_upscale_delta_dev(rgb_format(im.layout, order, im.Cn == 4, im.depth), im.W, im.H, multiply, filt, p_src, p_pitch, src, pitch, tile,
                                 dst, dpitch, None, 0, _stream_of(cur))
