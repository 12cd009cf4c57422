"""Planar and semi-planar YUV frames (include/srcnn_amd_yuv.h, _yuv_ex.h, _yuv_rect.h, _yuv_rect_list.h): the 8-bit 4:2:0 call and
the calls that take a srcnn_yuv_format -- frame, one rect, a list of rects."""
import ctypes as C

import numpy as np

from .abi import SRCNNF_Bicubic, YuvFormat, YuvRectItem
from .core import DeviceBuffer, _f32, _handle, _items, _list_dev, _list_plan, _pitches, _planes, _ref, _Regions, _uints, _wait, check, lib, output_size, sync

__all__ = ["YUV_I420", "YUV_NV12", "yuv420_sizes", "yuv420_upscale_dev", "yuv420_upscale", "YUV_PLANAR", "YUV_SEMIPLANAR", "YUV_420", "YUV_422",
           "YUV_444", "yuv_format", "yuv_plane_size", "yuv_plane_sizes", "yuv_upscale_dev", "yuv_upscale", "yuv_rect_source",
           "yuv_upscale_rect_dev", "yuv_upscale_rect", "yuv_rect_items", "yuv_upscale_rect_list_plan", "yuv_upscale_rect_list_dev",
           "yuv_upscale_rects"]

YUV_I420, YUV_NV12 = 0, 1
_YUV_FORMATS = {"i420": YUV_I420, "nv12": YUV_NV12, YUV_I420: YUV_I420, YUV_NV12: YUV_NV12}


def yuv420_sizes(w, h, multiply):
    """((dw, dh), (cw, ch), (dcw, dch)): luma output and chroma input / output sizes of srcnn_yuv420_upscale_dev."""
    dw, dh = output_size(w, h, multiply)
    return (dw, dh), ((w + 1) // 2, (h + 1) // 2), ((dw + 1) // 2, (dh + 1) // 2)


def yuv420_upscale_dev(fmt, w, h, multiply, filt, src, src_pitch, dst, dst_pitch, stream=None):
    """srcnn_yuv420_upscale_dev on device memory, as given: src / dst are 3 plane arguments (see _addr; NV12 ignores the
    third), pitches 3 byte counts (0 = tight) or None.  Asynchronous on `stream` (a Stream, a raw handle or None);
    raises SrcnnError with the library's code."""
    check(lib().srcnn_yuv420_upscale_dev(int(_YUV_FORMATS.get(fmt, fmt)), int(w), int(h), _f32(multiply), int(filt), _planes(src, 3),
                                         _pitches(src_pitch, 3), _planes(dst, 3), _pitches(dst_pitch, 3), _handle(stream)))


def yuv420_upscale(y, u, v=None, multiply=2.0, filt=SRCNNF_Bicubic, fmt="i420", stream=None):
    """One 8-bit YUV 4:2:0 frame through srcnn_yuv420_upscale_dev: numpy u8 planes in, numpy u8 planes out.
    I420: y (h, w), u and v (ceil(h/2), ceil(w/2)) -> (y', u', v').  NV12: y, and u = the interleaved UV plane
    (ceil(h/2), 2 ceil(w/2)) or (ceil(h/2), ceil(w/2), 2); v unused -> (y', uv') with uv' (ceil(dh/2), 2 ceil(dw/2))."""
    fmt = _YUV_FORMATS[fmt.lower() if isinstance(fmt, str) else fmt]
    y = np.ascontiguousarray(y, np.uint8)
    h, w = y.shape
    (dw, dh), (cw, ch), (dcw, dch) = yuv420_sizes(w, h, multiply)
    if fmt == YUV_NV12:
        planes = [y, np.ascontiguousarray(u, np.uint8).reshape(ch, 2 * cw)]
        shapes = [(dh, dw), (dch, 2 * dcw)]
    else:
        planes = [y, np.ascontiguousarray(u, np.uint8), np.ascontiguousarray(v, np.uint8)]
        assert planes[1].shape == planes[2].shape == (ch, cw), (planes[1].shape, planes[2].shape, (ch, cw))
        shapes = [(dh, dw), (dch, dcw), (dch, dcw)]
    din = [DeviceBuffer.from_numpy(p) for p in planes]
    dout = [DeviceBuffer(int(np.prod(s))) for s in shapes]
    yuv420_upscale_dev(fmt, w, h, multiply, filt, din, None, dout, None, stream)
    _wait(stream)
    return tuple(b.to_numpy(np.uint8, s) for b, s in zip(dout, shapes))


YUV_PLANAR, YUV_SEMIPLANAR = 0, 1
YUV_420, YUV_422, YUV_444 = 0, 1, 2
_YUV_LAYOUTS = {"planar": YUV_PLANAR, "semiplanar": YUV_SEMIPLANAR, YUV_PLANAR: YUV_PLANAR, YUV_SEMIPLANAR: YUV_SEMIPLANAR}
_YUV_CHROMAS = {"420": YUV_420, "422": YUV_422, "444": YUV_444, 420: YUV_420, 422: YUV_422, 444: YUV_444,
                YUV_420: YUV_420, YUV_422: YUV_422, YUV_444: YUV_444}


def yuv_format(layout="planar", chroma="420", depth=8, msb_aligned=False):
    """A srcnn_yuv_format: layout "planar" | "semiplanar", chroma "420" | "422" | "444" (or the SRCNN_YUV_* values), depth
    8 / 10 / 12 / 14 / 16, msb_aligned for P010-style words.  Unknown values are passed on for the library to refuse."""
    layout = layout.lower() if isinstance(layout, str) else layout
    return YuvFormat(C.sizeof(YuvFormat), int(_YUV_LAYOUTS.get(layout, layout)), int(_YUV_CHROMAS.get(chroma, chroma)), int(depth),
                     int(msb_aligned))


def yuv_plane_size(fmt, w, h, plane):
    """(cols, rows, row_bytes) of one plane of a w x h frame (srcnn_yuv_plane_size; no device)."""
    c, r, b = C.c_uint(0), C.c_uint(0), C.c_size_t(0)
    check(lib().srcnn_yuv_plane_size(C.byref(fmt), int(w), int(h), int(plane), C.byref(c), C.byref(r), C.byref(b)))
    return c.value, r.value, b.value


def _plane_count(fmt):
    return 2 if fmt.layout == YUV_SEMIPLANAR else 3


def yuv_plane_sizes(fmt, w, h, multiply):
    """((dw, dh), src_planes, dst_planes): the output size and, per plane of the format (2 for semi-planar, else 3),
    (cols, rows, row_bytes) of the input and of the output frame of srcnn_yuv_upscale_dev."""
    dw, dh = output_size(w, h, multiply)
    n = _plane_count(fmt)
    return ((dw, dh), [yuv_plane_size(fmt, w, h, k) for k in range(n)], [yuv_plane_size(fmt, dw, dh, k) for k in range(n)])


def _frame(fmt, w, h, multiply, filt):
    return (_ref(fmt), int(w), int(h), _f32(multiply), int(filt))


def yuv_upscale_dev(fmt, w, h, multiply, filt, src, src_pitch, dst, dst_pitch, stream=None):
    """srcnn_yuv_upscale_dev on device memory, as given: fmt a YuvFormat (yuv_format(...)) or None, src / dst 3 plane
    arguments (see _addr; semi-planar ignores the third), pitches 3 byte counts (0 = tight) or None.  Asynchronous on
    `stream` (a Stream, a raw handle or None); raises SrcnnError with the library's code."""
    check(lib().srcnn_yuv_upscale_dev(*_frame(fmt, w, h, multiply, filt), _planes(src, 3), _pitches(src_pitch, 3), _planes(dst, 3),
                                      _pitches(dst_pitch, 3), _handle(stream)))


class _YuvFrame:
    """What the numpy conveniences read off their input: the format, the sample type, and the planes of the w x h frame shaped
    as the format lays them out (semi-planar: (y, uv) with uv (rows, 2 * cols) or (rows, cols, 2))."""

    def __init__(self, planes, layout, chroma, depth, msb_aligned):
        self.fmt = yuv_format(layout, chroma, depth, msb_aligned)
        self.dt = np.uint8 if depth == 8 else np.uint16
        self.bps = np.dtype(self.dt).itemsize
        y = np.ascontiguousarray(planes[0], self.dt)
        self.h, self.w = y.shape
        self.n = _plane_count(self.fmt)
        sizes = [yuv_plane_size(self.fmt, self.w, self.h, k) for k in range(self.n)]
        self.ins = [y] + [np.ascontiguousarray(p, self.dt).reshape(r, rb // self.bps) for p, (_c, r, rb) in zip(planes[1:], sizes[1:])]
        assert len(self.ins) == self.n, "%d planes given, the format has %d" % (len(self.ins), self.n)

    def shapes(self, w, h):
        """The array shape of every plane of a w x h frame of the format."""
        return [(r, rb // self.bps) for (_c, r, rb) in (yuv_plane_size(self.fmt, w, h, k) for k in range(self.n))]


def yuv_upscale(planes, layout="planar", chroma="420", depth=8, msb_aligned=False, multiply=2.0, filt=SRCNNF_Bicubic, stream=None):
    """One YUV frame through srcnn_yuv_upscale_dev: numpy planes in, numpy planes out, uint8 at depth 8 and uint16 above.
    planar: (y, u, v) -> (y', u', v'); semi-planar: (y, uv) with uv (rows, 2 * cols) or (rows, cols, 2) -> (y', uv') with
    uv' (rows, 2 * cols)."""
    f = _YuvFrame(planes, layout, chroma, depth, msb_aligned)
    shapes = f.shapes(*output_size(f.w, f.h, multiply))
    din = [DeviceBuffer.from_numpy(p) for p in f.ins]
    dout = [DeviceBuffer(max(1, int(np.prod(s)) * f.bps)) for s in shapes]
    yuv_upscale_dev(f.fmt, f.w, f.h, multiply, filt, din, None, dout, None, stream)
    _wait(stream)
    return tuple(b.to_numpy(f.dt, s) for b, s in zip(dout, shapes))


def yuv_rect_source(fmt, w, h, multiply, filt, x0, y0, rw, rh, plane):
    """(sx0, sy0, sw, sh): the rectangle of plane `plane` (0..2) of the w x h source frame, in that plane's own sample
    coordinates (a UV plane: one column per pair), that output rect [x0, x0 + rw) x [y0, y0 + rh) of
    yuv_upscale_dev(fmt, ..., multiply, filt) depends on (srcnn_yuv_rect_source; no device)."""
    return _uints(lib().srcnn_yuv_rect_source, *_frame(fmt, w, h, multiply, filt), int(x0), int(y0), int(rw), int(rh), int(plane))


def yuv_upscale_rect_dev(fmt, w, h, multiply, filt, src, src_pitch, x0, y0, rw, rh, dst, dst_pitch, stream=None):
    """srcnn_yuv_upscale_rect_dev on device memory, as given: the arguments of yuv_upscale_dev with the rect (x0, y0, rw, rh) in
    luma output coordinates; src is the whole frame, dst the planes of an rw x rh frame (or the addresses of luma sample
    (x0, y0) and of the chroma sample that covers it inside a full-size frame, with that frame's pitches).  Plane arguments as
    for yuv_upscale_dev: a DeviceBuffer, an address, or (DeviceBuffer, byte offset).  Asynchronous on `stream`; raises
    SrcnnError with the library's code."""
    check(lib().srcnn_yuv_upscale_rect_dev(*_frame(fmt, w, h, multiply, filt), _planes(src, 3), _pitches(src_pitch, 3), int(x0), int(y0), int(rw),
                                           int(rh), _planes(dst, 3), _pitches(dst_pitch, 3), _handle(stream)))


def yuv_upscale_rect(planes, rect, layout="planar", chroma="420", depth=8, msb_aligned=False, multiply=2.0, filt=SRCNNF_Bicubic,
                     stream=None):
    """Rect = (x0, y0, rw, rh) (luma output coordinates) of yuv_upscale(planes, ...) through srcnn_yuv_upscale_rect_dev: numpy
    planes of the whole frame in, the planes of the rw x rh rect out (the chroma samples that cover it), shaped as
    yuv_upscale shapes the planes of an rw x rh frame."""
    f = _YuvFrame(planes, layout, chroma, depth, msb_aligned)
    x0, y0, rw, rh = (int(v) for v in rect)
    din = [DeviceBuffer.from_numpy(p) for p in f.ins]
    if rw <= 0 or rh <= 0:
        shapes, dout = [], [DeviceBuffer(1) for _ in range(f.n)]        # (for the library to refuse)
    else:
        shapes = f.shapes(rw, rh)
        dout = [DeviceBuffer(max(1, int(np.prod(s)) * f.bps)) for s in shapes]
    yuv_upscale_rect_dev(f.fmt, f.w, f.h, multiply, filt, din, None, x0, y0, rw, rh, dout, None, stream)
    _wait(stream)
    return tuple(b.to_numpy(f.dt, s) for b, s in zip(dout, shapes))


def yuv_rect_items(items):
    """A ctypes array of srcnn_yuv_rect_item from (x0, y0, rw, rh[, dst[, dst_pitch]]) tuples, or `items` itself when it already
    is such an array.  dst: up to 3 plane arguments (each a DeviceBuffer, a (DeviceBuffer, byte offset) pair or an address;
    semi-planar uses the first two), dst_pitch: up to 3 byte counts or None (tight).  Returns (array or None, n)."""
    return _items(YuvRectItem, items)


def yuv_upscale_rect_list_plan(fmt, w, h, multiply, filt, items, n=None, item_size=None, struct_size=None):
    """srcnn_yuv_upscale_rect_list_plan (no device): how the YUV list call routes and packs `items` (see yuv_rect_items) at the
    current mode, workspace limit and switches.  Returns the RectListPlan.  n / item_size / struct_size override what is passed
    (tests)."""
    return _list_plan("srcnn_yuv_upscale_rect_list_plan", _frame(fmt, w, h, multiply, filt), YuvRectItem, items, n, item_size, struct_size)


def yuv_upscale_rect_list_dev(fmt, w, h, multiply, filt, src, src_pitch, items, stream=None, n=None, item_size=None):
    """srcnn_yuv_upscale_rect_list_dev on device memory, as given: fmt, src and src_pitch as for yuv_upscale_rect_dev (the whole
    frame), items the rects with their destinations (see yuv_rect_items).  Asynchronous on `stream` (a Stream, a raw handle or
    None); the item array is read before the call returns.  Raises SrcnnError with the library's code."""
    _list_dev("srcnn_yuv_upscale_rect_list_dev", _frame(fmt, w, h, multiply, filt) + (_planes(src, 3), _pitches(src_pitch, 3)), YuvRectItem,
              items, n, item_size, stream)


def yuv_upscale_rects(planes, rects, layout="planar", chroma="420", depth=8, msb_aligned=False, multiply=2.0, filt=SRCNNF_Bicubic):
    """The planes of yuv_upscale_rect(planes, rect, ...) for every rect (x0, y0, rw, rh) of `rects`, through ONE
    srcnn_yuv_upscale_rect_list_dev call: numpy planes of the whole frame in, a list of (Y', U', V') tuples out -- (Y', UV') for a
    semi-planar format -- each shaped as yuv_upscale shapes the planes of an rw x rh frame."""
    rects = [tuple(int(v) for v in r) for r in rects]
    if not rects:
        return []
    f = _YuvFrame(planes, layout, chroma, depth, msb_aligned)
    din = [DeviceBuffer.from_numpy(p) for p in f.ins]
    regions, layouts = _Regions(), []               # per item and plane: (byte offset, shape)
    for (_, _, rw, rh) in rects:
        shapes = f.shapes(rw, rh) if rw > 0 and rh > 0 else [(0, 0)] * f.n       # (an empty rect: for the library to refuse)
        layouts.append([(regions.add(s[0] * s[1] * f.bps), s) for s in shapes])
    dout = regions.alloc()
    items = [(x0, y0, rw, rh, [(dout, o) for o, _ in one], None) for (x0, y0, rw, rh), one in zip(rects, layouts)]
    yuv_upscale_rect_list_dev(f.fmt, f.w, f.h, multiply, filt, din, None, items)
    sync()
    regions.download()
    return [tuple(regions.take(o, f.dt, sh) for o, sh in one) for one in layouts]
