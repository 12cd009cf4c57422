"""Packed YUV frames -- YUY2, UYVY, Y210, Y410, v210 ... (include/srcnn_amd_yuv_packed.h, _yuv_packed_rect.h,
_yuv_packed_rect_list.h): frame, one rect, a list of rects."""
import ctypes as C

import numpy as np

from .abi import SRCNNF_Bicubic, YuvPackedRectItem
from .core import DeviceBuffer, SrcnnError, _addr, _f32, _handle, _items, _list_dev, _list_plan, _Regions, _uints, _wait, check, lib, output_size, sync

__all__ = ["YUVP_YUY2", "YUVP_UYVY", "YUVP_YVYU", "YUVP_Y210", "YUVP_Y212", "YUVP_Y216", "YUVP_VUYA", "YUVP_Y410", "YUVP_Y416", "YUVP_V210",
           "yuv_packed_row_bytes", "yuv_packed_upscale_dev", "yuv_packed_upscale", "yuv_packed_span_bytes", "yuv_packed_rect_source",
           "yuv_packed_upscale_rect_dev", "yuv_packed_upscale_rect", "yuv_packed_rect_items", "yuv_packed_upscale_rect_list_plan",
           "yuv_packed_upscale_rect_list_dev", "yuv_packed_upscale_rects"]

(YUVP_YUY2, YUVP_UYVY, YUVP_YVYU, YUVP_Y210, YUVP_Y212, YUVP_Y216, YUVP_VUYA, YUVP_Y410, YUVP_Y416, YUVP_V210) = range(10)
_YUVP_FORMATS = {"yuy2": YUVP_YUY2, "uyvy": YUVP_UYVY, "yvyu": YUVP_YVYU, "y210": YUVP_Y210, "y212": YUVP_Y212, "y216": YUVP_Y216,
                 "vuya": YUVP_VUYA, "ayuv": YUVP_VUYA, "y410": YUVP_Y410, "y416": YUVP_Y416, "v210": YUVP_V210}


def _yuvp_format(fmt):
    return int(_YUVP_FORMATS.get(fmt.lower(), -1) if isinstance(fmt, str) else fmt)


def _frame(fmt, w, h, multiply, filt):
    return (_yuvp_format(fmt), int(w), int(h), _f32(multiply), int(filt))


def yuv_packed_row_bytes(fmt, w):
    """(tight row bytes, alignment of base and pitch) of a w-pixel row of a packed format: a YUVP_* value or its name
    ("yuy2", "v210" ...; srcnn_yuv_packed_row_bytes; no device)."""
    rb, al = C.c_size_t(0), C.c_uint(0)
    check(lib().srcnn_yuv_packed_row_bytes(_yuvp_format(fmt), int(w), C.byref(rb), C.byref(al)))
    return rb.value, al.value


def yuv_packed_upscale_dev(fmt, w, h, multiply, filt, src, src_pitch, dst, dst_pitch, stream=None):
    """srcnn_yuv_packed_upscale_dev on device memory, as given: src / dst one frame argument each (see _addr), pitches in
    bytes (0 = tight).  Asynchronous on `stream` (a Stream, a raw handle or None); raises SrcnnError with the library's code."""
    check(lib().srcnn_yuv_packed_upscale_dev(*_frame(fmt, w, h, multiply, filt), _addr(src), int(src_pitch or 0), _addr(dst), int(dst_pitch or 0),
                                             _handle(stream)))


def _whole_frame(frame, fmt, w):
    """The packed frame as a (h, row bytes of w pixels) uint8 array, or ValueError."""
    frame = np.ascontiguousarray(frame, np.uint8)
    rb, _ = yuv_packed_row_bytes(fmt, w)
    if frame.ndim != 2 or frame.shape[1] != rb:
        raise ValueError("a %d-pixel row of this format has %d bytes: the frame is %r" % (w, rb, frame.shape))
    return frame


def _span(fmt, dw, x0, rw, rh):
    """Bytes per row segment of an rw-pixel rect at x0 of a dw-pixel output row; 0 for what the library is to refuse."""
    if rw <= 0 or rh <= 0:
        return 0
    try:
        return yuv_packed_span_bytes(fmt, dw, x0, rw)[2]
    except SrcnnError:
        return 0                             # (for the upscale call to refuse, with its own message)


def yuv_packed_upscale(frame, fmt, w, multiply=2.0, filt=SRCNNF_Bicubic, stream=None):
    """One packed YUV frame through srcnn_yuv_packed_upscale_dev: a 2-D uint8 array of h x row_bytes(w) in, one of
    dh x row_bytes(dw) out (tight rows; `w` says how many pixels a row holds)."""
    frame = _whole_frame(frame, fmt, w)
    h = frame.shape[0]
    dw, dh = output_size(w, h, multiply)
    drb, _ = yuv_packed_row_bytes(fmt, dw)
    din = DeviceBuffer.from_numpy(frame)
    dout = DeviceBuffer(max(1, dh * drb))
    yuv_packed_upscale_dev(fmt, w, h, multiply, filt, din, 0, dout, 0, stream)
    _wait(stream)
    return dout.to_numpy(np.uint8, (dh, drb))


def yuv_packed_span_bytes(fmt, width, x, n):
    """(unit in pixels, byte offset, byte length) of pixels [x, x + n) of a `width`-pixel row of a packed format
    (srcnn_yuv_packed_span_bytes; no device): x a multiple of the unit, n one or x + n == width, where the length runs to the
    end of the tight row."""
    unit, off, nb = C.c_uint(0), C.c_size_t(0), C.c_size_t(0)
    check(lib().srcnn_yuv_packed_span_bytes(_yuvp_format(fmt), int(width), int(x), int(n), C.byref(unit), C.byref(off), C.byref(nb)))
    return unit.value, off.value, nb.value


def yuv_packed_rect_source(fmt, w, h, multiply, filt, x0, y0, rw, rh):
    """(sx0, sy0, sw, sh): the rectangle of the w x h packed source frame, in luma pixels, that output rect
    [x0, x0 + rw) x [y0, y0 + rh) of yuv_packed_upscale_dev(fmt, ..., multiply, filt) depends on
    (srcnn_yuv_packed_rect_source; no device)."""
    return _uints(lib().srcnn_yuv_packed_rect_source, *_frame(fmt, w, h, multiply, filt), int(x0), int(y0), int(rw), int(rh))


def yuv_packed_upscale_rect_dev(fmt, w, h, multiply, filt, src, src_pitch, x0, y0, rw, rh, dst, dst_pitch, stream=None):
    """srcnn_yuv_packed_upscale_rect_dev on device memory, as given: the arguments of yuv_packed_upscale_dev with the rect
    (x0, y0, rw, rh) in luma output coordinates; src is the whole frame, dst the rect's row segments (or the address of the
    rect's first byte inside a full-size frame, with that frame's pitch).  Frame arguments: a DeviceBuffer, an address, or
    (DeviceBuffer, byte offset).  Asynchronous on `stream`; raises SrcnnError with the library's code."""
    check(lib().srcnn_yuv_packed_upscale_rect_dev(*_frame(fmt, w, h, multiply, filt), _addr(src), int(src_pitch or 0), int(x0), int(y0), int(rw),
                                                  int(rh), _addr(dst), int(dst_pitch or 0), _handle(stream)))


def yuv_packed_upscale_rect(frame, fmt, w, rect, multiply=2.0, filt=SRCNNF_Bicubic, stream=None):
    """Rect = (x0, y0, rw, rh) (luma output coordinates, under the format's unit rule) of yuv_packed_upscale(frame, fmt, w, ...)
    through srcnn_yuv_packed_upscale_rect_dev: the whole packed frame in, the (rh, bytes) uint8 array of the rect's row segments
    out, bytes as yuv_packed_span_bytes(fmt, dw, x0, rw) gives them."""
    frame = _whole_frame(frame, fmt, w)
    h = frame.shape[0]
    x0, y0, rw, rh = (int(v) for v in rect)
    din = DeviceBuffer.from_numpy(frame)
    nb = _span(fmt, output_size(w, h, multiply)[0], x0, rw, rh) if rw > 0 and rh > 0 else 0
    dout = DeviceBuffer(max(1, rh * nb))
    yuv_packed_upscale_rect_dev(fmt, w, h, multiply, filt, din, 0, x0, y0, rw, rh, dout, 0, stream)
    _wait(stream)
    return dout.to_numpy(np.uint8, (rh, nb))


def yuv_packed_rect_items(items):
    """A ctypes array of srcnn_yuv_packed_rect_item from (x0, y0, rw, rh[, dst[, dst_pitch]]) tuples, or `items` itself when it
    already is such an array.  dst: a DeviceBuffer, a (DeviceBuffer, byte offset) pair or an address; dst_pitch: bytes or None
    (tight).  Returns (array or None, n)."""
    return _items(YuvPackedRectItem, items)


def yuv_packed_upscale_rect_list_plan(fmt, w, h, multiply, filt, items, n=None, item_size=None, struct_size=None):
    """srcnn_yuv_packed_upscale_rect_list_plan (no device): how the packed YUV list call routes and packs `items` (see
    yuv_packed_rect_items) at the current mode, workspace limit and switches.  Returns the RectListPlan.  n / item_size /
    struct_size override what is passed (tests)."""
    return _list_plan("srcnn_yuv_packed_upscale_rect_list_plan", _frame(fmt, w, h, multiply, filt), YuvPackedRectItem, items, n, item_size,
                      struct_size)


def yuv_packed_upscale_rect_list_dev(fmt, w, h, multiply, filt, src, src_pitch, items, stream=None, n=None, item_size=None):
    """srcnn_yuv_packed_upscale_rect_list_dev on device memory, as given: fmt, src and src_pitch as for
    yuv_packed_upscale_rect_dev (the whole frame), items the rects with their destinations (see yuv_packed_rect_items).
    Asynchronous on `stream` (a Stream, a raw handle or None); the item array is read before the call returns.  Raises SrcnnError
    with the library's code."""
    _list_dev("srcnn_yuv_packed_upscale_rect_list_dev", _frame(fmt, w, h, multiply, filt) + (_addr(src), int(src_pitch or 0)), YuvPackedRectItem,
              items, n, item_size, stream)


def yuv_packed_upscale_rects(src, name, w, rects, multiply=2.0, filt=SRCNNF_Bicubic):
    """The row segments of yuv_packed_upscale_rect(src, name, w, rect, ...) for every rect (x0, y0, rw, rh) of `rects`, through
    ONE srcnn_yuv_packed_upscale_rect_list_dev call: the whole packed frame in (a (h, row bytes) uint8 array of format `name`), a
    list of (rh, bytes) uint8 arrays out, bytes as yuv_packed_span_bytes(name, dw, x0, rw) gives them."""
    rects = [tuple(int(v) for v in r) for r in rects]
    if not rects:
        return []
    frame = _whole_frame(src, name, w)
    h = frame.shape[0]
    dw, _dh = output_size(w, h, multiply)
    din = DeviceBuffer.from_numpy(frame)
    regions, layouts = _Regions(), []               # per item: (byte offset, (rows, bytes))
    for (x0, y0, rw, rh) in rects:
        nb = _span(name, dw, x0, rw, rh)
        layouts.append((regions.add(max(rh, 0) * nb), (max(rh, 0) if nb else 0, nb)))
    dout = regions.alloc()
    items = [(x0, y0, rw, rh, (dout, o), 0) for (x0, y0, rw, rh), (o, _sh) in zip(rects, layouts)]
    yuv_packed_upscale_rect_list_dev(name, w, h, multiply, filt, din, 0, items)
    sync()
    regions.download()
    return [regions.take(o, np.uint8, sh) for o, sh in layouts]
