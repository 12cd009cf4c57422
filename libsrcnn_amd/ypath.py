"""The Y path (include/srcnn_amd.h, _rect.h, _rect_list.h, _delta.h and the stage hooks of _debug.h): frame, band, batch, stream,
the single stages, one rect, a list of rects, and the delta between two frames."""
import ctypes as C

import numpy as np

from .abi import RectItem, SRCNNF_Bicubic
from .core import (DeviceBuffer, _addr, _delta_rects, _delta_stats, _handle, _items, _list_dev, _list_plan, _previous, _ref, _Regions, _uints,
                   check, lib, sync)

__all__ = ["y_upscale2x", "y_upscale2x_batch", "y_upscale2x_stream", "stream_mode", "y_path", "y_upscale2x_band", "y_path_rect_source",
           "y_path_rect_dev", "y_path_rect", "rect_items", "y_path_rect_list_plan", "y_path_rect_list_dev", "y_path_delta_grid",
           "y_path_delta_flags_dev", "y_path_delta_rects", "y_path_delta_dev", "y_path_delta", "y_path_rects", "resample", "conv1", "conv2",
           "conv3", "conv12", "axis_table"]


# ------------------------------------------------------------------------------------------------
# numpy-level helpers over the C ABI (host arrays in, host arrays out)
# ------------------------------------------------------------------------------------------------
def _plane(a):
    a = np.ascontiguousarray(a, np.float32)
    assert a.ndim == 2, a.shape
    return a


def y_upscale2x(y):
    """srcnn_y_upscale2x_f32: 2x Mitchell upscale + the three convolutions of one float Y plane."""
    y = _plane(y)
    h, w = y.shape
    out = np.empty((2 * h, 2 * w), np.float32)
    check(lib().srcnn_y_upscale2x_f32(y.ctypes.data, w, h, out.ctypes.data))
    return out


def y_upscale2x_batch(frames):
    frames = np.ascontiguousarray(frames, np.float32)
    n, h, w = frames.shape
    out = np.empty((n, 2 * h, 2 * w), np.float32)
    check(lib().srcnn_y_upscale2x_f32_batch(frames.ctypes.data, w, h, n, out.ctypes.data))
    return out


def y_upscale2x_stream(frames, use_graph=True):
    """srcnn_y_upscale2x_f32_stream.  use_graph: False / 0 = plain launches, True / 2 = hipGraph replay whatever it costs,
    "auto" / 1 = replay kept only while it is cheap in host CPU (stream_mode() says what ran)."""
    frames = np.ascontiguousarray(frames, np.float32)
    n, h, w = frames.shape
    out = np.empty((n, 2 * h, 2 * w), np.float32)
    g = 1 if use_graph == "auto" else (int(use_graph) if isinstance(use_graph, int) and not isinstance(use_graph, bool) else (2 if use_graph else 0))
    check(lib().srcnn_y_upscale2x_f32_stream(frames.ctypes.data, w, h, n, out.ctypes.data, g))
    return out


def stream_mode():
    """(frames replayed from a hipGraph, frames launched plainly, fell back?) of the process's last stream call."""
    g, p, f = C.c_uint(0), C.c_uint(0), C.c_int(0)
    check(lib().srcnn_debug_stream_mode(C.byref(g), C.byref(p), C.byref(f)))
    return g.value, p.value, bool(f.value)


def y_path(y, dw, dh, filt=SRCNNF_Bicubic):
    y = _plane(y)
    h, w = y.shape
    out = np.empty((dh, dw), np.float32)
    check(lib().srcnn_y_path_f32(y.ctypes.data, w, h, dw, dh, filt, out.ctypes.data))
    return out


def y_upscale2x_band(y, row0, rows):
    y = _plane(y)
    h, w = y.shape
    return _stage(lib().srcnn_y_upscale2x_f32_band_dev, y, (rows, 2 * w), w, h, row0, rows)


def y_path_rect_source(w, h, dw, dh, filt, x0, y0, rw, rh):
    """(sx0, sy0, sw, sh): the source rectangle output rect [x0, x0 + rw) x [y0, y0 + rh) of the dw x dh Y path depends on
    (srcnn_y_path_rect_source; no device)."""
    return _uints(lib().srcnn_y_path_rect_source, int(w), int(h), int(dw), int(dh), int(filt), int(x0), int(y0), int(rw), int(rh))


def y_path_rect_dev(src, in_pitch, w, h, dw, dh, filt, x0, y0, rw, rh, dst, out_pitch, stream=None):
    """srcnn_y_path_rect_f32_dev on device memory, as given: src / dst plane arguments (see _addr), pitches in bytes (0 =
    tight).  Asynchronous on `stream` (a Stream, a raw handle or None); raises SrcnnError with the library's code."""
    check(lib().srcnn_y_path_rect_f32_dev(_addr(src), int(in_pitch or 0), int(w), int(h), int(dw), int(dh), int(filt), int(x0), int(y0),
                                          int(rw), int(rh), _addr(dst), int(out_pitch or 0), _handle(stream)))


def y_path_rect(plane, dw, dh, filt, x0, y0, rw, rh):
    """Samples [x0, x0 + rw) x [y0, y0 + rh) of y_path(plane, dw, dh, filt) through srcnn_y_path_rect_f32_dev: numpy in, numpy out."""
    y = _plane(plane)
    h, w = y.shape
    din = DeviceBuffer.from_numpy(y)
    dout = DeviceBuffer(max(1, rw * rh * 4))
    y_path_rect_dev(din, 0, w, h, dw, dh, filt, x0, y0, rw, rh, dout, 0)
    sync()
    return dout.to_numpy(np.float32, (rh, rw))


def rect_items(items):
    """A ctypes array of srcnn_rect_item from (x0, y0, rw, rh[, dst[, out_pitch]]) tuples (dst: a DeviceBuffer, an address or
    None), or `items` itself when it already is such an array.  Returns (array or None, n)."""
    return _items(RectItem, items)


def _frame(src, in_pitch, w, h, dw, dh, filt):
    return (_addr(src), int(in_pitch or 0), int(w), int(h), int(dw), int(dh), int(filt))


def y_path_rect_list_plan(w, h, dw, dh, filt, items, n=None, item_size=None, struct_size=None):
    """srcnn_y_path_rect_list_plan (no device): how the list call routes and packs `items` (see rect_items) at the current mode,
    workspace limit and switches.  Returns the RectListPlan.  n / item_size / struct_size override what is passed (tests)."""
    return _list_plan("srcnn_y_path_rect_list_plan", (int(w), int(h), int(dw), int(dh), int(filt)), RectItem, items, n, item_size, struct_size)


def y_path_rect_list_dev(src, in_pitch, w, h, dw, dh, filt, items, stream=None, n=None, item_size=None):
    """srcnn_y_path_rect_list_f32_dev on device memory, as given: src is the whole source plane (see _addr), items the rects with
    their destinations (see rect_items).  Asynchronous on `stream` (a Stream, a raw handle or None); the item array is read
    before the call returns.  Raises SrcnnError with the library's code."""
    _list_dev("srcnn_y_path_rect_list_f32_dev", _frame(src, in_pitch, w, h, dw, dh, filt), RectItem, items, n, item_size, stream)


def y_path_delta_grid(w, h, dw, dh, filt, tile=(0, 0)):
    """(cols, rows) of the delta call's tile grid (srcnn_y_path_delta_grid; no device).  tile: (tile_w, tile_h), 0 = the default 64."""
    return _uints(lib().srcnn_y_path_delta_grid, int(w), int(h), int(dw), int(dh), int(filt), int(tile[0]), int(tile[1]), n=2)


def _pair(prev, prev_pitch, cur, cur_pitch, w, h, dw, dh, filt, tile):
    return (_addr(prev), int(prev_pitch or 0)) + _frame(cur, cur_pitch, w, h, dw, dh, filt) + (int(tile[0]), int(tile[1]))


def y_path_delta_flags_dev(prev, prev_pitch, cur, cur_pitch, w, h, dw, dh, filt, tile, flags, stream=None):
    """srcnn_y_path_delta_flags_dev on device memory, as given: prev (None = no previous frame) / cur are whole source planes and
    flags receives cols x rows bytes (see _addr), pitches in bytes (0 = tight).  Asynchronous on `stream`."""
    check(lib().srcnn_y_path_delta_flags_dev(*_pair(prev, prev_pitch, cur, cur_pitch, w, h, dw, dh, filt, tile), _addr(flags), _handle(stream)))


def y_path_delta_rects(flags, tile, dw, dh, out=None, out_pitch=0, cap=None):
    """srcnn_y_path_delta_rects (pure host): the coalescer over a (rows, cols) uint8 array of flags of tile[0] x tile[1] tiles.
    Returns [(x0, y0, rw, rh, d_out, out_pitch)].  cap: None = as many items as needed; 0 = count only (returns the number);
    anything else is the capacity handed to the call (tests)."""
    flags = np.ascontiguousarray(flags, np.uint8)
    rows, cols = flags.shape
    head = (flags.ctypes.data, cols, rows, int(tile[0]), int(tile[1]), int(dw), int(dh), _addr(out), int(out_pitch or 0))
    got = _delta_rects("srcnn_y_path_delta_rects", head, RectItem, cap)
    if cap == 0:
        return got
    arr, n = got
    return [(arr[k].x0, arr[k].y0, arr[k].rw, arr[k].rh, arr[k].d_out, arr[k].out_pitch) for k in range(n)]


def y_path_delta_dev(prev, prev_pitch, cur, cur_pitch, w, h, dw, dh, filt, tile, out, out_pitch, stream=None, stats=True, struct_size=None):
    """srcnn_y_path_delta_f32_dev on device memory, as given: repaints inside the full-size plane `out` what can differ between
    prev (None = no previous frame) and cur.  Blocks until the flags have arrived; the upscale is asynchronous on `stream`.
    Returns the DeltaStats (None with stats=False)."""
    st = _delta_stats(stats, struct_size)
    check(lib().srcnn_y_path_delta_f32_dev(*_pair(prev, prev_pitch, cur, cur_pitch, w, h, dw, dh, filt, tile), _addr(out), int(out_pitch or 0),
                                           _handle(stream), _ref(st)))
    return st


def y_path_delta(prev, cur, out, dw, dh, filt=SRCNNF_Bicubic, tile=(0, 0)):
    """numpy convenience over srcnn_y_path_delta_f32_dev: `out` (dh x dw float32, the Y path of `prev`; prev None = anything) is
    updated to the Y path of `cur`.  Returns (out, stats) -- a new array; what the call did not repaint is copied from `out`."""
    y = _plane(cur)
    h, w = y.shape
    o = np.ascontiguousarray(out, np.float32)
    assert o.shape == (dh, dw), o.shape
    dprev = DeviceBuffer.from_numpy(_plane(prev)) if prev is not None else None
    assert prev is None or _plane(prev).shape == y.shape
    dcur = DeviceBuffer.from_numpy(y)
    dout = DeviceBuffer.from_numpy(o)
    st = y_path_delta_dev(dprev, 0, dcur, 0, w, h, dw, dh, filt, tile, dout, 0)
    sync()
    return dout.to_numpy(np.float32, (dh, dw)), st


def y_path_rects(plane, dw, dh, filt, rects):
    """Samples [x0, x0 + rw) x [y0, y0 + rh) of y_path(plane, dw, dh, filt) for every (x0, y0, rw, rh) of `rects`, through ONE
    srcnn_y_path_rect_list_f32_dev call: numpy in, a list of numpy arrays out."""
    y = _plane(plane)
    h, w = y.shape
    rects = [tuple(int(v) for v in r) for r in rects]
    din = DeviceBuffer.from_numpy(y)
    regions = _Regions()
    offs = [regions.add(rw * rh * 4) for (_, _, rw, rh) in rects]
    dout = regions.alloc()
    y_path_rect_list_dev(din, 0, w, h, dw, dh, filt, [(x0, y0, rw, rh, dout.ptr + o, 0) for (x0, y0, rw, rh), o in zip(rects, offs)])
    sync()
    regions.download()
    return [regions.take(o, np.float32, (rh, rw)) for (_, _, rw, rh), o in zip(rects, offs)]


def _stage(fn, src, out_shape, *dims):
    src = np.ascontiguousarray(src, np.float32)
    din = DeviceBuffer.from_numpy(src)
    dout = DeviceBuffer(int(np.prod(out_shape)) * 4)
    check(fn(din.ptr, *dims, dout.ptr, None))
    sync()
    return dout.to_numpy(np.float32, out_shape)


def resample(y, dw, dh, filt=SRCNNF_Bicubic):
    y = _plane(y)
    h, w = y.shape
    return _stage(lib().srcnn_resample_f32_dev, y, (dh, dw), w, h, dw, dh, filt)


def conv1(y):
    y = _plane(y)
    h, w = y.shape
    return _stage(lib().srcnn_conv1_f32_dev, y, (64, h, w), w, h)


def conv2(c1):
    _, h, w = c1.shape
    return _stage(lib().srcnn_conv2_f32_dev, c1, (32, h, w), w, h)


def conv3(c2):
    _, h, w = c2.shape
    return _stage(lib().srcnn_conv3_f32_dev, c2, (h, w), w, h)


def conv12(y):
    y = _plane(y)
    h, w = y.shape
    return _stage(lib().srcnn_conv12_f32_dev, y, (32, h, w), w, h)


def axis_table(dst_len, src_len, filt=SRCNNF_Bicubic):
    win = _previous(lib().srcnn_axis_table(filt, dst_len, src_len, None, None, None))
    left = np.zeros(dst_len, np.int32)
    right = np.zeros(dst_len, np.int32)
    w = np.zeros((dst_len, win + 1), np.float64)
    lib().srcnn_axis_table(filt, dst_len, src_len, left.ctypes.data, right.ctypes.data, w.ctypes.data)
    return left, right, w
