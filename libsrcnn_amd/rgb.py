"""RGB(A) images (include/srcnn_amd_rgb.h, _rgb_rect.h, _rgb_rect_list.h, _rgb_delta.h): frame, one rect, a list of rects and the
delta between two images in device memory; and the host-image calls of include/srcnn_amd.h -- srcnn_process_u8, ProcessJob and
the reference's two public names."""
import ctypes as C

import numpy as np

from .abi import CXX_SYMBOLS, RgbFormat, RgbRectItem, SRCNNF_Bicubic
from .core import (DeviceBuffer, _addr, _delta_rects, _delta_stats, _f32, _handle, _items, _list_dev, _list_plan, _pitches, _planes, _ref, _Regions,
                   _uints, _wait, check, lib, output_size, sync)

__all__ = ["process_u8", "RGB_INTERLEAVED", "RGB_PLANAR", "RGB_ORDER_RGB", "RGB_ORDER_BGR", "rgb_format", "rgb_plane_size", "rgb_upscale_dev",
           "rgb_upscale", "rgb_rect_source", "rgb_upscale_rect_dev", "rgb_upscale_rect", "rgb_rect_items", "rgb_upscale_rect_list_plan",
           "rgb_upscale_rect_list_dev", "rgb_upscale_rects", "rgb_delta_grid", "rgb_delta_flags_dev", "rgb_delta_rects", "rgb_upscale_delta_dev",
           "rgb_upscale_delta", "ProcessJob", "ConfigureFilterSRCNN", "ProcessSRCNN"]


def process_u8(rgb, multiply=2.0, filt=SRCNNF_Bicubic, want_conv=True):
    """srcnn_process_u8: one doSRCNN pass, interleaved u8 (h,w,d) in, (rgb_out, conv_y|None) out."""
    rgb = np.ascontiguousarray(rgb, np.uint8)
    h, w, d = rgb.shape
    m = np.float32(multiply)
    dw, dh = int(np.float32(w) * m), int(np.float32(h) * m)
    out = np.empty((dh, dw, d), np.uint8)
    conv = np.empty((dh, dw), np.uint8) if want_conv else None
    check(lib().srcnn_process_u8(rgb.ctypes.data, w, h, d, float(m), filt, out.ctypes.data,
                                 conv.ctypes.data if want_conv else None))
    return out, conv


RGB_INTERLEAVED, RGB_PLANAR = 0, 1
RGB_ORDER_RGB, RGB_ORDER_BGR = 0, 1
_RGB_LAYOUTS = {"interleaved": RGB_INTERLEAVED, "hwc": RGB_INTERLEAVED, "planar": RGB_PLANAR, "chw": RGB_PLANAR}
_RGB_ORDERS = {"rgb": RGB_ORDER_RGB, "rgba": RGB_ORDER_RGB, "bgr": RGB_ORDER_BGR, "bgra": RGB_ORDER_BGR}


def rgb_format(layout="interleaved", order="rgb", alpha=False, depth=8):
    """A srcnn_rgb_format: layout "interleaved" | "planar", order "rgb" | "bgr" (or the SRCNN_RGB_* values), alpha for a
    fourth channel, depth 8 / 10 / 12 / 14 / 16.  Unknown values are passed on for the library to refuse."""
    layout = layout.lower() if isinstance(layout, str) else layout
    order = order.lower() if isinstance(order, str) else order
    return RgbFormat(C.sizeof(RgbFormat), int(_RGB_LAYOUTS.get(layout, layout)), int(_RGB_ORDERS.get(order, order)), int(alpha), int(depth))


def rgb_plane_size(fmt, w, h, plane):
    """(cols, rows, row_bytes) of one plane of a w x h image (srcnn_rgb_plane_size; no device)."""
    c, r, b = C.c_uint(0), C.c_uint(0), C.c_size_t(0)
    check(lib().srcnn_rgb_plane_size(C.byref(fmt), int(w), int(h), int(plane), C.byref(c), C.byref(r), C.byref(b)))
    return c.value, r.value, b.value


def _frame(fmt, w, h, multiply, filt):
    return (_ref(fmt), int(w), int(h), _f32(multiply), int(filt))


def _image(planes, pitch):
    """The two arguments of an image: void *[4] and size_t[4]."""
    return (_planes(planes, 4), _pitches(pitch, 4))


def rgb_upscale_dev(fmt, w, h, multiply, filt, src, src_pitch, dst, dst_pitch, dst_conv=None, dst_conv_pitch=0, stream=None):
    """srcnn_rgb_upscale_dev on device memory, as given: fmt an RgbFormat (rgb_format(...)) or None, src / dst up to 4 plane
    arguments (see _addr; interleaved uses the first only), pitches byte counts (0 = tight) or None, dst_conv a plane
    argument for the truncated Y' or None.  Asynchronous on `stream` (a Stream, a raw handle or None); raises SrcnnError with
    the library's code."""
    check(lib().srcnn_rgb_upscale_dev(*_frame(fmt, w, h, multiply, filt), *_image(src, src_pitch), *_image(dst, dst_pitch), _addr(dst_conv),
                                      int(dst_conv_pitch), _handle(stream)))


class _RgbImage:
    """What the numpy conveniences read off their image: (h, w, c) (interleaved) or (c, h, w) (planar) with c = 3 or 4; layout
    decides where both fit (default: interleaved when the last axis is 3 or 4), depth defaults to 8 for uint8 and 16 otherwise."""

    def __init__(self, image, layout, order, depth):
        image = np.asarray(image)
        if image.ndim != 3:
            raise ValueError("an RGB(A) image is (h, w, c) or (c, h, w), not %r" % (image.shape,))
        if layout is None:
            layout = "interleaved" if image.shape[2] in (3, 4) else "planar"
        self.planar = _RGB_LAYOUTS.get(layout.lower() if isinstance(layout, str) else layout, layout) == RGB_PLANAR
        if depth is None:
            depth = 8 if image.dtype == np.uint8 else 16
        self.dt = np.uint8 if depth == 8 else np.uint16
        self.bps = np.dtype(self.dt).itemsize
        self.array = image = np.ascontiguousarray(image, self.dt)
        (self.c, self.h, self.w) = image.shape if self.planar else (image.shape[2], image.shape[0], image.shape[1])
        if self.c not in (3, 4):
            raise ValueError("%d channels: an RGB(A) image has 3 or 4" % self.c)
        self.fmt = rgb_format(RGB_PLANAR if self.planar else RGB_INTERLEAVED, order, self.c == 4, depth)

    def shape(self, w, h):
        """The array shape of a w x h image in the layout of this one."""
        return (self.c, h, w) if self.planar else (h, w, self.c)

    def planes(self, buf, w, h, at=0):
        """The plane arguments of a tight w x h image that starts `at` bytes into DeviceBuffer buf."""
        return [(buf, at + k * w * h * self.bps) for k in range(self.c)] if self.planar else [(buf, at)]


def rgb_upscale(image, multiply=2.0, filt=SRCNNF_Bicubic, layout=None, order="rgb", depth=None, want_conv=False, stream=None):
    """One RGB(A) image through srcnn_rgb_upscale_dev: numpy in, numpy out, uint8 at depth 8 and uint16 above.  image is
    (h, w, c) (interleaved) or (c, h, w) (planar) with c = 3 or 4; layout = "interleaved" / "planar" decides where both fit
    (default: interleaved when the last axis is 3 or 4).  depth defaults to 8 for uint8 and 16 otherwise.
    Returns (out, conv | None) with out shaped like the input."""
    im = _RgbImage(image, layout, order, depth)
    dw, dh = output_size(im.w, im.h, multiply)
    din = DeviceBuffer.from_numpy(im.array)
    dout = DeviceBuffer(max(1, dw * dh * im.c * im.bps))
    dconv = DeviceBuffer(max(1, dw * dh * im.bps)) if want_conv else None
    rgb_upscale_dev(im.fmt, im.w, im.h, multiply, filt, im.planes(din, im.w, im.h), None, im.planes(dout, dw, dh), None, dconv, 0, stream)
    _wait(stream)
    return dout.to_numpy(im.dt, im.shape(dw, dh)), (dconv.to_numpy(im.dt, (dh, dw)) if want_conv else None)


def rgb_rect_source(w, h, multiply, filt, x0, y0, rw, rh):
    """(sx0, sy0, sw, sh): the rectangle of the w x h source image that output rect [x0, x0 + rw) x [y0, y0 + rh) of
    rgb_upscale_dev(..., multiply, filt) depends on (srcnn_rgb_rect_source; no device)."""
    return _uints(lib().srcnn_rgb_rect_source, int(w), int(h), _f32(multiply), int(filt), int(x0), int(y0), int(rw), int(rh))


def rgb_upscale_rect_dev(fmt, w, h, multiply, filt, src, src_pitch, x0, y0, rw, rh, dst, dst_pitch, dst_conv=None, dst_conv_pitch=0,
                         stream=None):
    """srcnn_rgb_upscale_rect_dev on device memory, as given: the arguments of rgb_upscale_dev with the rect (x0, y0, rw, rh)
    in output coordinates; src is the whole image, dst / dst_conv are rw x rh images (or the address of pixel (x0, y0) of a
    full-size image with that image's pitch).  Asynchronous on `stream`; raises SrcnnError with the library's code."""
    check(lib().srcnn_rgb_upscale_rect_dev(*_frame(fmt, w, h, multiply, filt), *_image(src, src_pitch), int(x0), int(y0), int(rw), int(rh),
                                           *_image(dst, dst_pitch), _addr(dst_conv), int(dst_conv_pitch), _handle(stream)))


def rgb_upscale_rect(image, rect, multiply=2.0, filt=SRCNNF_Bicubic, layout=None, order="rgb", depth=None, want_conv=False,
                     stream=None):
    """Pixels rect = (x0, y0, rw, rh) of rgb_upscale(image, ...) through srcnn_rgb_upscale_rect_dev: numpy in, numpy out.
    Returns (out, conv | None), out shaped (rh, rw, c) or (c, rh, rw) like the input."""
    im = _RgbImage(image, layout, order, depth)
    x0, y0, rw, rh = (int(v) for v in rect)
    din = DeviceBuffer.from_numpy(im.array)
    dout = DeviceBuffer(max(1, rw * rh * im.c * im.bps))
    dconv = DeviceBuffer(max(1, rw * rh * im.bps)) if want_conv else None
    rgb_upscale_rect_dev(im.fmt, im.w, im.h, multiply, filt, im.planes(din, im.w, im.h), None, x0, y0, rw, rh, im.planes(dout, rw, rh), None,
                         dconv, 0, stream)
    _wait(stream)
    return dout.to_numpy(im.dt, im.shape(rw, rh)), (dconv.to_numpy(im.dt, (rh, rw)) if want_conv else None)


def rgb_rect_items(items):
    """A ctypes array of srcnn_rgb_rect_item from (x0, y0, rw, rh[, dst[, dst_pitch[, dst_conv[, dst_conv_pitch]]]]) tuples, or
    `items` itself when it already is such an array.  dst: up to 4 plane arguments (each a DeviceBuffer, a (DeviceBuffer, byte
    offset) pair or an address; interleaved uses the first only), dst_pitch: up to 4 byte counts or None (tight), dst_conv: a
    plane argument or None.  Returns (array or None, n)."""
    return _items(RgbRectItem, items)


def rgb_upscale_rect_list_plan(fmt, w, h, multiply, filt, items, n=None, item_size=None, struct_size=None):
    """srcnn_rgb_upscale_rect_list_plan (no device): how the RGB(A) list call routes and packs `items` (see rgb_rect_items) at
    the current mode, workspace limit and switches.  Returns the RectListPlan.  n / item_size / struct_size override what is
    passed (tests)."""
    return _list_plan("srcnn_rgb_upscale_rect_list_plan", _frame(fmt, w, h, multiply, filt), RgbRectItem, items, n, item_size, struct_size)


def rgb_upscale_rect_list_dev(fmt, w, h, multiply, filt, src, src_pitch, items, stream=None, n=None, item_size=None):
    """srcnn_rgb_upscale_rect_list_dev on device memory, as given: fmt, src and src_pitch as for rgb_upscale_rect_dev (the whole
    image), items the rects with their destinations (see rgb_rect_items).  Asynchronous on `stream` (a Stream, a raw handle or
    None); the item array is read before the call returns.  Raises SrcnnError with the library's code."""
    _list_dev("srcnn_rgb_upscale_rect_list_dev", _frame(fmt, w, h, multiply, filt) + _image(src, src_pitch), RgbRectItem, items, n, item_size,
              stream)


def rgb_upscale_rects(image, rects, multiply=2.0, filt=SRCNNF_Bicubic, layout=None, order="rgb", depth=None, want_conv=False):
    """Pixels (x0, y0, rw, rh) of rgb_upscale(image, ...) for every rect of `rects`, through ONE srcnn_rgb_upscale_rect_list_dev
    call: numpy in, a list of numpy arrays out -- each shaped (rh, rw, c) or (c, rh, rw) like the input -- or, with want_conv,
    a list of (out, conv) pairs."""
    im = _RgbImage(image, layout, order, depth)
    rects = [tuple(int(v) for v in r) for r in rects]
    if not rects:
        return []
    din = DeviceBuffer.from_numpy(im.array)
    regions = _Regions()                          # per item: the image, then the conv plane
    offs = [(regions.add(rw * rh * im.c * im.bps), regions.add(rw * rh * im.bps if want_conv else 0)) for (_, _, rw, rh) in rects]
    dout = regions.alloc()
    items = [(x0, y0, rw, rh, im.planes(dout, rw, rh, o_img), None, (dout, o_conv) if want_conv else None, 0)
             for (x0, y0, rw, rh), (o_img, o_conv) in zip(rects, offs)]
    rgb_upscale_rect_list_dev(im.fmt, im.w, im.h, multiply, filt, im.planes(din, im.w, im.h), None, items)
    sync()
    regions.download()
    res = []
    for (_, _, rw, rh), (o_img, o_conv) in zip(rects, offs):
        out = regions.take(o_img, im.dt, im.shape(rw, rh))
        res.append((out, regions.take(o_conv, im.dt, (rh, rw))) if want_conv else out)
    return res


def rgb_delta_grid(w, h, multiply, filt, tile=(0, 0)):
    """(dw, dh, cols, rows): the output size and the tile grid of the RGB(A) delta call (srcnn_rgb_delta_grid; no device).
    tile: (tile_w, tile_h), 0 = the default 64."""
    return _uints(lib().srcnn_rgb_delta_grid, int(w), int(h), _f32(multiply), int(filt), int(tile[0]), int(tile[1]))


def rgb_delta_flags_dev(fmt, w, h, multiply, filt, prev, prev_pitch, cur, cur_pitch, tile, flags, stream=None):
    """srcnn_rgb_delta_flags_dev on device memory, as given: prev (None = no previous image) / cur are up to 4 plane arguments of
    whole source images (see _addr), pitches byte counts or None (tight), flags receives cols x rows bytes.  Asynchronous on
    `stream`."""
    check(lib().srcnn_rgb_delta_flags_dev(*_frame(fmt, w, h, multiply, filt), *_image(prev, prev_pitch), *_image(cur, cur_pitch), int(tile[0]),
                                          int(tile[1]), _addr(flags), _handle(stream)))


def rgb_delta_rects(flags, tile, fmt, dw, dh, dst=None, dst_pitch=None, dst_conv=None, dst_conv_pitch=0, cap=None, item_size=None):
    """srcnn_rgb_delta_rects (pure host): the coalescer over a (rows, cols) uint8 array of flags of tile[0] x tile[1] tiles, as
    items that point into the full-size image dst / dst_conv (plane arguments, or None).  Returns
    [(x0, y0, rw, rh, [dst 0..3], [dst_pitch 0..3], dst_conv, dst_conv_pitch)].  cap: None = as many items as needed; 0 = count
    only (returns the number); anything else is the capacity handed to the call (tests)."""
    flags = np.ascontiguousarray(flags, np.uint8)
    rows, cols = flags.shape
    size = C.sizeof(RgbRectItem) if item_size is None else int(item_size)
    head = (flags.ctypes.data, cols, rows, int(tile[0]), int(tile[1]), _ref(fmt), int(dw), int(dh), *_image(dst, dst_pitch), _addr(dst_conv),
            int(dst_conv_pitch or 0))
    got = _delta_rects("srcnn_rgb_delta_rects", head, RgbRectItem, cap, (size,))
    if cap == 0:
        return got
    arr, n = got
    return [(a.x0, a.y0, a.rw, a.rh, list(a.dst), list(a.dst_pitch), a.dst_conv, a.dst_conv_pitch) for a in arr[:n]]


def rgb_upscale_delta_dev(fmt, w, h, multiply, filt, prev, prev_pitch, cur, cur_pitch, tile, dst, dst_pitch, dst_conv=None, dst_conv_pitch=0,
                          stream=None, stats=True, struct_size=None):
    """srcnn_rgb_upscale_delta_dev on device memory, as given: repaints inside the full-size image dst (and dst_conv) what can
    differ between prev (None = no previous image) and cur.  Blocks until the flags have arrived; the upscale is asynchronous on
    `stream`.  Returns the DeltaStats (None with stats=False)."""
    st = _delta_stats(stats, struct_size)
    check(lib().srcnn_rgb_upscale_delta_dev(*_frame(fmt, w, h, multiply, filt), *_image(prev, prev_pitch), *_image(cur, cur_pitch), int(tile[0]),
                                            int(tile[1]), *_image(dst, dst_pitch), _addr(dst_conv), int(dst_conv_pitch or 0), _handle(stream),
                                            _ref(st)))
    return st


def rgb_upscale_delta(prev, cur, out, multiply=2.0, filt=SRCNNF_Bicubic, layout=None, order="rgb", depth=None, tile=(0, 0), conv=None):
    """numpy convenience over srcnn_rgb_upscale_delta_dev: `out` (rgb_upscale of `prev`; prev None = anything) is updated to
    rgb_upscale of `cur`, and so is `conv` (the truncated Y' plane) when given.  Images as for rgb_upscale.  Returns
    (out, stats), or (out, conv, stats) with conv -- new arrays; what the call did not repaint is copied from `out` / `conv`."""
    im = _RgbImage(cur, layout, order, depth)
    w, h = im.w, im.h
    dw, dh = output_size(w, h, multiply)
    o = np.ascontiguousarray(out, im.dt)
    if o.shape != im.shape(dw, dh):
        raise ValueError("out is %r, the output image %r" % (o.shape, im.shape(dw, dh)))
    if prev is not None and np.asarray(prev).shape != im.array.shape:
        raise ValueError("prev is %r, cur %r" % (np.asarray(prev).shape, im.array.shape))
    dprev = DeviceBuffer.from_numpy(np.ascontiguousarray(prev, im.dt)) if prev is not None else None
    dcur = DeviceBuffer.from_numpy(im.array)
    dout = DeviceBuffer.from_numpy(o)
    dconv = DeviceBuffer.from_numpy(np.ascontiguousarray(conv, im.dt).reshape(dh, dw)) if conv is not None else None
    st = rgb_upscale_delta_dev(im.fmt, w, h, multiply, filt, im.planes(dprev, w, h) if dprev is not None else None, None, im.planes(dcur, w, h),
                               None, tile, im.planes(dout, dw, dh), None, dconv, 0)
    sync()
    res = dout.to_numpy(im.dt, o.shape)
    return (res, dconv.to_numpy(im.dt, (dh, dw)), st) if conv is not None else (res, st)


class ProcessJob:
    """srcnn_process_u8_begin / _wait: the image is being produced; result() blocks and returns (rgb_out, conv_y|None).

    The object owns the buffers a native worker thread reads and writes, so it must never be reclaimed while that thread is
    still running: result(), leaving a `with` block and the finaliser all end in srcnn_process_u8_wait (the finaliser is what
    covers a job dropped without result() -- e.g. the second constructor of `[ProcessJob(a), ProcessJob(b)]` raising)."""

    def __init__(self, rgb, multiply=2.0, filt=SRCNNF_Bicubic, want_conv=True, out=None, conv=None):
        self.job = None
        self.rgb = np.ascontiguousarray(rgb, np.uint8)          # kept alive until the job is done
        h, w, d = self.rgb.shape
        m = np.float32(multiply)
        dw, dh = int(np.float32(w) * m), int(np.float32(h) * m)
        self.out = out if out is not None else np.empty((dh, dw, d), np.uint8)
        self.conv = (conv if conv is not None else np.empty((dh, dw), np.uint8)) if want_conv else None
        job = C.c_void_p()
        check(lib().srcnn_process_u8_begin(self.rgb.ctypes.data, w, h, d, float(m), filt, self.out.ctypes.data,
                                           self.conv.ctypes.data if want_conv else None, C.byref(job)))
        self.job = job

    def _wait(self):
        """Join the native job (idempotent); returns its code."""
        if self.job is None:
            return 0
        job, self.job = self.job, None
        return lib().srcnn_process_u8_wait(job)

    def result(self):
        check(self._wait())
        return self.out, self.conv

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self._wait()
        return False

    def __del__(self):
        try:
            self._wait()          # the worker thread must be done with rgb / out / conv before they are freed
        except Exception:
            pass


# ------------------------------------------------------------------------------------------------
# The reference's public API, same names and argument meaning (src/libsrcnn.h:46-54), called through
# the exported C++ symbols.
# ------------------------------------------------------------------------------------------------
def ConfigureFilterSRCNN(ftype, stepscale=False):
    getattr(lib(), CXX_SYMBOLS[0])(int(ftype), bool(stepscale))


def ProcessSRCNN(refbuff, w, h, d, multiply, want_conv=True):
    """Returns (retcode, outbuff ndarray|None, convbuff ndarray|None) -- the reference's out-params."""
    L = lib()
    if refbuff is not None:
        refbuff = np.ascontiguousarray(refbuff, np.uint8)
    out, outsz = C.c_void_p(), C.c_uint(0)
    conv, convsz = C.c_void_p(), C.c_uint(0)
    rc = getattr(L, CXX_SYMBOLS[1])(refbuff.ctypes.data if refbuff is not None else None, w, h, d, _f32(multiply), C.byref(out), C.byref(outsz),
                                    C.byref(conv) if want_conv else None, C.byref(convsz) if want_conv else None)
    o = c = None
    if rc == 0:
        o = np.ctypeslib.as_array(C.cast(out, C.POINTER(C.c_ubyte)), (outsz.value,)).copy()
        L.srcnn_delete_array(out)
        if want_conv and conv.value:
            c = np.ctypeslib.as_array(C.cast(conv, C.POINTER(C.c_ubyte)), (convsz.value,)).copy()
            L.srcnn_delete_array(conv)
    return rc, o, c
