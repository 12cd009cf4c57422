#!/usr/bin/env python3
"""What the ctypes binding looks like from outside, as plain data: tests/test_binding_surface.py holds the package to it.

  surface(S)  every public name of the package: kind, signature, Structure fields and size, value of a constant
  record(S)   what reaches the library: a recorder stands in for the loaded shared object while every thin wrapper is driven
              with a full and a minimal argument set; each C call is kept as (symbol, normalised arguments)

Neither needs the shared object or a device.  Run in a checkout of the commit whose binding is the yardstick,

  python tools/binding_snapshot.py

writes tests/binding_surface.json and tests/binding_record.json.  The committed files come from the last commit that had the
binding in one flat module; regenerating them from a later tree only makes the test compare the binding with itself.
"""
import ctypes as C
import gc
import inspect
import json
import os
import sys
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SKIP = ("C", "np", "os")


# ---- surface ------------------------------------------------------------------------------------------------------------
def public_names(S):
    return sorted(n for n, v in vars(S).items() if not n.startswith("_") and n not in SKIP and not isinstance(v, types.ModuleType))


def _value(S, v):
    if isinstance(v, str) and v.startswith(os.path.dirname(os.path.abspath(S.__file__))):
        return "<package>" + v[len(os.path.dirname(os.path.abspath(S.__file__))):]
    return list(v) if isinstance(v, tuple) else v


def _callables(cls):
    out = {}
    for n, f in sorted(vars(cls).items()):
        f = f.__func__ if isinstance(f, (classmethod, staticmethod)) else f
        if inspect.isfunction(f):
            out[n] = {"signature": str(inspect.signature(f)), "doc": bool(f.__doc__)}
    return out


def surface(S):
    out = {}
    for name in public_names(S):
        v = getattr(S, name)
        if inspect.isclass(v) and issubclass(v, C.Structure):
            out[name] = {"kind": "structure", "fields": [[f, t.__name__] for f, t in v._fields_], "sizeof": C.sizeof(v), "doc": bool(v.__doc__)}
        elif inspect.isclass(v):
            out[name] = {"kind": "class", "bases": [b.__name__ for b in v.__bases__], "methods": _callables(v), "doc": bool(v.__doc__)}
        elif inspect.isfunction(v):
            out[name] = {"kind": "function", "signature": str(inspect.signature(v)), "doc": bool(v.__doc__)}
        else:
            out[name] = {"kind": type(v).__name__, "value": _value(S, v)}
    return out


# ---- marshalling record -------------------------------------------------------------------------------------------------
def _plain(v):
    """ctypes and numpy values as JSON data; bool and float tagged, so that True / 1 / 1.0 stay three different things."""
    if isinstance(v, (bool, np.bool_)):
        return "b:%s" % bool(v)
    if isinstance(v, (float, np.floating)):
        return "f:" + float(v).hex()
    if v is None or isinstance(v, str):
        return v
    if isinstance(v, (int, np.integer)):
        return int(v)
    if isinstance(v, bytes):
        return "x:" + v.hex()
    if isinstance(v, C.Structure):
        return {f: _plain(getattr(v, f)) for f, _t in v._fields_}
    if isinstance(v, C.Array):
        if v._type_ is C.c_char:
            return {"char_buffer": len(v)}
        if issubclass(v._type_, C.Structure):
            return "x:" + bytes(v).hex()
        return [_plain(x) for x in v]
    if isinstance(v, C._SimpleCData):
        return {type(v).__name__: _plain(v.value)}
    if type(v).__name__ == "CArgObject":
        return {"byref": _plain(v._obj)}
    if isinstance(v, np.ndarray):
        return {"ndarray": list(v.shape), "dtype": str(v.dtype)}
    if isinstance(v, (tuple, list)):
        return [_plain(x) for x in v]
    if isinstance(v, dict):
        return {str(k): _plain(x) for k, x in v.items()}
    return {"object": type(v).__name__}


# item arrays arrive as c_void_p: symbol -> (index of the array, of n, of item_size); their n * item_size bytes are the record
ITEMS = {"srcnn_y_path_rect_list_plan": (5, 6, 7), "srcnn_y_path_rect_list_f32_dev": (7, 8, 9),
         "srcnn_rgb_upscale_rect_list_plan": (5, 6, 7), "srcnn_rgb_upscale_rect_list_dev": (7, 8, 9),
         "srcnn_yuv_upscale_rect_list_plan": (5, 6, 7), "srcnn_yuv_upscale_rect_list_dev": (7, 8, 9),
         "srcnn_yuv_packed_upscale_rect_list_plan": (5, 6, 7), "srcnn_yuv_packed_upscale_rect_list_dev": (7, 8, 9)}
# addresses of numpy arrays change from run to run: symbol -> {index: bytes behind it given the arguments, or None = "host"}
HOST = {"srcnn_memcpy_h2d": {1: lambda a: a[2]}, "srcnn_memcpy_d2h": {0: None}, "srcnn_axis_table": {3: None, 4: None, 5: None},
        "srcnn_y_path_delta_rects": {0: lambda a: a[1] * a[2]}, "srcnn_rgb_delta_rects": {0: lambda a: a[1] * a[2]}}


class Recorder:
    """Stands in for the CDLL: every attribute is a function that records its call and returns 0 (srcnn_dev_alloc: addresses)."""

    def __init__(self):
        self.calls = []
        self.next_alloc = 0x7e0000000000

    def __getattr__(self, symbol):
        def call(*args):
            norm = []
            for k, a in enumerate(args):
                if symbol in ITEMS and k == ITEMS[symbol][0] and isinstance(a, C.c_void_p):
                    nbytes = int(args[ITEMS[symbol][1]]) * int(args[ITEMS[symbol][2]])
                    norm.append("x:" + C.string_at(a.value, nbytes).hex() if a.value and 0 <= nbytes <= 4096 else {"items": a.value and "unread", "bytes": nbytes})
                elif symbol in HOST and k in HOST[symbol] and a is not None:
                    size = HOST[symbol][k]
                    norm.append("x:" + C.string_at(int(a), int(size(args))).hex() if size else "host")
                elif isinstance(a, C.c_void_p):
                    norm.append("pointer" if a.value else None)
                else:
                    norm.append(_plain(a))
            if symbol == "srcnn_dev_free":       # when a buffer is collected is not the wrapper's doing
                return None
            self.calls.append([symbol, norm])
            if symbol == "srcnn_dev_alloc":
                self.next_alloc += 0x100000
                return self.next_alloc
            return 0
        return call


def _cases(S):
    """[(name, thunk)]: every thin wrapper with a full and a minimal argument set."""
    P1, P2, P3, P4 = 0x7f0000001000, (0x7f0000002000, 48), 0x7f0000003000, (0x7f0000004000, 16)
    Q1, Q2, Q3, Q4 = (0x7f1000001000, 32), 0x7f1000002000, (0x7f1000003000, 0), 0x7f1000004000
    STREAM, M = 0x5550000, 1.7
    yf = lambda: S.yuv_format("semiplanar", "422", 10, True)      # noqa: E731
    rf = lambda: S.rgb_format("planar", "bgr", True, 12)          # noqa: E731
    flags = np.array([[1, 0, 1], [0, 1, 1]], np.uint8)
    small = np.arange(6, dtype=np.float32).reshape(2, 3)

    def stream_object():
        s = S.Stream()
        s.handle = 0x7770000
        return s

    def array_of(kind, rows):
        arr = (kind * len(rows))()
        for a, r in zip(arr, rows):
            a.x0, a.y0, a.rw, a.rh = r
        return arr

    y_items = [(3, 2, 8, 6), (0, 0, 18, 14, P2), (16, 13, 2, 1, P1, 256), (1, 1, 2, 2, None, None)]
    rgb_items = [(3, 2, 8, 6), (0, 0, 18, 14, [P1, P2, P3, P4]), (1, 1, 4, 4, [P1], [96]), (2, 2, 4, 4, [P1, P2, P3], [64, None, 32], P4),
                 (4, 4, 2, 2, None, None, Q2, 128), (5, 5, 1, 1, [Q1, Q2, Q3, Q4], [1, 2, 3, 4], Q1, None)]
    yuv_items = [(3, 2, 8, 6), (0, 0, 18, 14, [P1, P2, P3]), (2, 2, 4, 4, [P1, P2], [64, None]), (4, 4, 2, 2, None, None),
                 (6, 6, 2, 2, [Q1, Q2, Q3], [128, 64, 64])]
    yp_items = [(4, 2, 8, 6), (0, 0, 18, 14, P2), (16, 12, 2, 2, P1, 256), (2, 2, 2, 2, None, None)]
    families = [("y", S.RectItem, y_items, S.rect_items), ("rgb", S.RgbRectItem, rgb_items, S.rgb_rect_items),
                ("yuv", S.YuvRectItem, yuv_items, S.yuv_rect_items), ("yuv_packed", S.YuvPackedRectItem, yp_items, S.yuv_packed_rect_items)]
    cases = []
    add = lambda name, fn: cases.append((name, fn))               # noqa: E731

    # core
    add("output_size", lambda: S.output_size(9, 7, M, True))
    add("output_size min", lambda: S.output_size(9, 7, 2))
    add("init", lambda: S.init(1))
    add("init_devices", lambda: (S.init_devices(None), S.init_devices([0, 0, 1])))
    add("contexts and modes", lambda: (S.context_count(), S.set_context(1), S.set_mode(S.MODE_FAST), S.set_relaxation(5), S.device_count()))
    add("profile and clock", lambda: (S.profile_enable(), S.profile_enable(False), S.profile_reset(), S.clock_probe(), S.profile_read(),
                                      S.profile_read_context(1), S.stream_mode()))
    add("sync shutdown", lambda: (S.sync(), S.shutdown()))
    add("device buffer", lambda: (lambda b: (b.upload(small, 8), b.nbytes, b.free(), b.ptr))(S.DeviceBuffer(64)))
    add("stream and event", lambda: (lambda s, e: (s.sync(), e.record(s), e.record(), e.elapsed_ms(e), s.destroy()))(stream_object(), S.Event()))

    # item builders, list plans and list calls of the four families
    for fam, kind, items, build in families:
        ready = array_of(kind, [(1, 2, 3, 4), (5, 6, 7, 8)])
        add(fam + " items tuples", lambda build=build, items=items: build(items))
        add(fam + " items generator", lambda build=build, items=items: build(tuple(i) for i in items[:2]))
        add(fam + " items array", lambda build=build, ready=ready: (lambda r: (r[0] is ready, r[1]))(build(ready)))
        add(fam + " items empty", lambda build=build: build([]))
    add("y list plan full", lambda: S.y_path_rect_list_plan(9, 7, 18, 14, 2, y_items, n=3, item_size=24, struct_size=40))
    add("y list plan", lambda: S.y_path_rect_list_plan(9, 7, 18, 14, 2, y_items))
    add("y list plan array", lambda: S.y_path_rect_list_plan(9, 7, 18, 14, 2, array_of(S.RectItem, [(1, 2, 3, 4)]), n=1))
    add("y list plan min", lambda: (S.y_path_rect_list_plan(9, 7, 18, 14, 2, None), S.y_path_rect_list_plan(9, 7, 18, 14, 2, []),
                                    S.y_path_rect_list_plan(9, 7, 18, 14, 2, None, n=2, item_size=0)))
    add("y list dev full", lambda: S.y_path_rect_list_dev(P2, 64, 9, 7, 18, 14, 2, y_items, STREAM, n=2, item_size=40))
    add("y list dev stream object", lambda: S.y_path_rect_list_dev(S.DeviceBuffer(252), 0, 9, 7, 18, 14, 2, y_items, stream_object()))
    add("y list dev array", lambda: S.y_path_rect_list_dev(P1, 64, 9, 7, 18, 14, 2, array_of(S.RectItem, [(1, 2, 3, 4), (5, 6, 7, 8)])))
    add("y list dev min", lambda: (S.y_path_rect_list_dev(None, None, 9, 7, 18, 14, 2, None), S.y_path_rect_list_dev(P1, None, 9, 7, 18, 14, 2, [])))
    for fam, kind, items, fmt, plan, dev, src, pitch in (
            ("rgb", S.RgbRectItem, rgb_items, rf, S.rgb_upscale_rect_list_plan, S.rgb_upscale_rect_list_dev, [P1, P2, P3, P4], [64, 64, 32, 16]),
            ("yuv", S.YuvRectItem, yuv_items, yf, S.yuv_upscale_rect_list_plan, S.yuv_upscale_rect_list_dev, [P1, P2, P3], [64, 32, 16]),
            ("yuv_packed", S.YuvPackedRectItem, yp_items, lambda: "y210", S.yuv_packed_upscale_rect_list_plan, S.yuv_packed_upscale_rect_list_dev, P2, 48)):
        short = src[:1] if isinstance(src, list) else src
        none_pitch = None
        add(fam + " list plan full", lambda plan=plan, fmt=fmt, items=items: plan(fmt(), 9, 7, M, 2, items, n=3, item_size=24, struct_size=40))
        add(fam + " list plan", lambda plan=plan, fmt=fmt, items=items: plan(fmt(), 9, 7, 2.0, 2, items))
        add(fam + " list plan array", lambda plan=plan, fmt=fmt, kind=kind: plan(fmt(), 9, 7, M, 2, array_of(kind, [(1, 2, 3, 4)]), n=1))
        add(fam + " list plan min", lambda plan=plan, fam=fam: (plan(None if fam != "yuv_packed" else S.YUVP_V210, 9, 7, 2, 2, None),
                                                              plan(None if fam != "yuv_packed" else "nope", 9, 7, 2, 2, []),
                                                              plan(None if fam != "yuv_packed" else 3, 9, 7, 2, 2, None, n=2, item_size=0)))
        add(fam + " list dev full", lambda dev=dev, fmt=fmt, items=items, src=src, pitch=pitch:
            dev(fmt(), 9, 7, M, 2, src, pitch, items, STREAM, n=2, item_size=40))
        add(fam + " list dev stream object", lambda dev=dev, fmt=fmt, items=items, src=src, pitch=pitch:
            dev(fmt(), 9, 7, M, 2, src, pitch, items, stream_object()))
        add(fam + " list dev array", lambda dev=dev, fmt=fmt, kind=kind, src=src, pitch=pitch:
            dev(fmt(), 9, 7, M, 2, src, pitch, array_of(kind, [(1, 2, 3, 4), (5, 6, 7, 8)])))
        add(fam + " list dev short", lambda dev=dev, fmt=fmt, short=short, none_pitch=none_pitch: dev(fmt(), 9, 7, 2, 2, short, none_pitch, []))
        add(fam + " list dev min", lambda dev=dev, fam=fam, none_pitch=none_pitch:
            dev(None if fam != "yuv_packed" else S.YUVP_UYVY, 9, 7, 2, 2, None, none_pitch, None))

    # Y path: rect, delta, stages
    add("y rect source", lambda: S.y_path_rect_source(9, 7, 18, 14, 2, 3, 2, 8, 6))
    add("y rect dev full", lambda: S.y_path_rect_dev(P2, 64, 9, 7, 18, 14, 2, 3, 2, 8, 6, Q1, 128, STREAM))
    add("y rect dev min", lambda: S.y_path_rect_dev(P1, None, 9, 7, 18, 14, 2, 3, 2, 8, 6, None, None))
    add("y rect dev buffers", lambda: S.y_path_rect_dev(S.DeviceBuffer(252), 0, 9, 7, 18, 14, 2, 3, 2, 8, 6, (S.DeviceBuffer(192), 16), 0, stream_object()))
    add("y delta grid", lambda: (S.y_path_delta_grid(9, 7, 18, 14, 2, (32, 16)), S.y_path_delta_grid(9, 7, 18, 14, 2)))
    add("y delta flags full", lambda: S.y_path_delta_flags_dev(P2, 64, Q1, 48, 9, 7, 18, 14, 2, (32, 16), P3, STREAM))
    add("y delta flags min", lambda: S.y_path_delta_flags_dev(None, None, P1, None, 9, 7, 18, 14, 2, (0, 0), Q2))
    for cap in (None, 0, 3):
        add("y delta rects cap %r" % (cap,), lambda cap=cap: S.y_path_delta_rects(flags, (32, 16), 80, 30, P2, 256, cap))
        add("y delta rects min cap %r" % (cap,), lambda cap=cap: S.y_path_delta_rects(flags, (32, 16), 80, 30, cap=cap))
    add("y delta dev full", lambda: S.y_path_delta_dev(P2, 64, Q1, 48, 9, 7, 18, 14, 2, (32, 16), P4, 128, STREAM, True, 24))
    add("y delta dev", lambda: S.y_path_delta_dev(P1, 0, Q2, 0, 9, 7, 18, 14, 2, (0, 0), P3, 0, stream_object()))
    add("y delta dev min", lambda: S.y_path_delta_dev(None, None, P1, None, 9, 7, 18, 14, 2, (0, 0), P3, None, stats=False))
    add("stages", lambda: [S.conv1(small), S.conv12(small), S.conv2(np.zeros((64, 2, 3), np.float32)), S.conv3(np.zeros((32, 2, 3), np.float32)),
                           S.resample(small, 5, 4, S.SRCNNF_Lanczos3), S.y_upscale2x_band(small, 1, 1)])
    add("axis table", lambda: S.axis_table(6, 3, S.SRCNNF_Bilinear))
    add("y conveniences", lambda: [S.y_path_rect(small, 6, 4, 2, 1, 1, 3, 2), S.y_path_rects(small, 6, 4, 2, [(1, 1, 3, 2), (0, 0, 6, 4)]),
                                   S.y_path_delta(small, small + 1, np.zeros((4, 6), np.float32), 6, 4, 2, (32, 16))[0],
                                   S.y_path_delta(None, small, np.zeros((4, 6), np.float32), 6, 4)[0]])

    # YUV planar / semi-planar
    add("yuv formats", lambda: [S.yuv_format(), yf(), S.yuv_format("PLANAR", 444, 16), S.yuv_format(7, "9", 12, 1), S.yuv_format(S.YUV_SEMIPLANAR, S.YUV_422)])
    add("yuv420 sizes", lambda: S.yuv420_sizes(9, 7, M))
    add("yuv420 dev full", lambda: S.yuv420_upscale_dev("nv12", 9, 7, M, 2, [P1, P2, P3], [64, 32, 16], [Q1, Q2, Q3], [128, 64, 32], STREAM))
    add("yuv420 dev min", lambda: S.yuv420_upscale_dev(S.YUV_I420, 9, 7, 2, 2, [P1, None, P3], None, [Q1, Q2], None))
    add("yuv420 dev short", lambda: S.yuv420_upscale_dev("i420", 9, 7, 2, 2, [P1, P2], [64, 32], [Q2], [128], stream_object()))
    add("yuv420 dev unknown format", lambda: S.yuv420_upscale_dev(9, 9, 7, 2, 2, [P1, P2, P3], None, [Q1, Q2, Q3], None))
    add("yuv plane size", lambda: (S.yuv_plane_size(yf(), 9, 7, 1), S.yuv_plane_sizes(yf(), 9, 7, M), S.yuv_plane_sizes(S.yuv_format(), 9, 7, 2)))
    add("yuv dev full", lambda: S.yuv_upscale_dev(yf(), 9, 7, M, 2, [P1, P2, P3], [64, 32, 16], [Q1, Q2, Q3], [128, 64, 32], STREAM))
    add("yuv dev short", lambda: S.yuv_upscale_dev(yf(), 9, 7, 2, 2, [P1, P2], [64, 32], [Q1, None], [128], stream_object()))
    add("yuv dev min", lambda: S.yuv_upscale_dev(None, 9, 7, 2, 2, None, None, None, None))
    add("yuv rect source", lambda: (S.yuv_rect_source(yf(), 9, 7, M, 2, 2, 2, 9, 7, 1), S.yuv_rect_source(None, 9, 7, 2, 2, 2, 2, 9, 7, 0)))
    add("yuv rect dev full", lambda: S.yuv_upscale_rect_dev(yf(), 9, 7, M, 2, [P1, P2, P3], [64, 32, 16], 2, 2, 8, 6, [Q1, Q2, Q3], [128, 64, 32], STREAM))
    add("yuv rect dev short", lambda: S.yuv_upscale_rect_dev(yf(), 9, 7, 2, 2, [P1, P2], [64], 2, 2, 8, 6, [Q1, None], [128, 64], stream_object()))
    add("yuv rect dev min", lambda: S.yuv_upscale_rect_dev(None, 9, 7, 2, 2, None, None, 2, 2, 8, 6, None, None))

    # packed YUV
    add("packed row bytes", lambda: [S.yuv_packed_row_bytes("yuy2", 9), S.yuv_packed_row_bytes("V210", 9), S.yuv_packed_row_bytes(S.YUVP_Y410, 9),
                                     S.yuv_packed_row_bytes("nope", 9), S.yuv_packed_row_bytes("ayuv", 9)])
    add("packed span bytes", lambda: [S.yuv_packed_span_bytes("v210", 18, 6, 12), S.yuv_packed_span_bytes(S.YUVP_UYVY, 18, 0, 18)])
    add("packed dev full", lambda: S.yuv_packed_upscale_dev("y210", 9, 7, M, 2, P2, 48, Q1, 96, STREAM))
    add("packed dev min", lambda: S.yuv_packed_upscale_dev(S.YUVP_YUY2, 9, 7, 2, 2, None, None, None, None))
    add("packed dev buffers", lambda: S.yuv_packed_upscale_dev("uyvy", 9, 7, 2, 2, S.DeviceBuffer(140), 0, (S.DeviceBuffer(560), 8), 0, stream_object()))
    add("packed rect source", lambda: (S.yuv_packed_rect_source("y416", 9, 7, M, 2, 2, 2, 8, 6), S.yuv_packed_rect_source(S.YUVP_VUYA, 9, 7, 2, 2, 2, 2, 8, 6)))
    add("packed rect dev full", lambda: S.yuv_packed_upscale_rect_dev("y212", 9, 7, M, 2, P2, 48, 2, 2, 8, 6, Q1, 96, STREAM))
    add("packed rect dev min", lambda: S.yuv_packed_upscale_rect_dev(S.YUVP_YVYU, 9, 7, 2, 2, None, None, 2, 2, 8, 6, None, None))

    # RGB(A)
    add("rgb formats", lambda: [S.rgb_format(), rf(), S.rgb_format("CHW", "BGRA", 1, 16), S.rgb_format("hwc", "rgba"), S.rgb_format(5, 7, 2, 9),
                                S.rgb_format(S.RGB_PLANAR, S.RGB_ORDER_BGR)])
    add("rgb plane size", lambda: S.rgb_plane_size(rf(), 9, 7, 3))
    add("rgb dev full", lambda: S.rgb_upscale_dev(rf(), 9, 7, M, 2, [P1, P2, P3, P4], [64, 64, 32, 16], [Q1, Q2, Q3, Q4], [128, 128, 64, 32], P4, 96, STREAM))
    add("rgb dev short", lambda: S.rgb_upscale_dev(rf(), 9, 7, 2, 2, [P1], [64], [Q1, None, Q3], [128, 0], None, 0, stream_object()))
    add("rgb dev min", lambda: S.rgb_upscale_dev(None, 9, 7, 2, 2, None, None, None, None))
    add("rgb rect source", lambda: (S.rgb_rect_source(9, 7, M, 2, 3, 2, 8, 6), S.rgb_rect_source(9, 7, 2, 0, 0, 0, 18, 14)))
    add("rgb rect dev full", lambda: S.rgb_upscale_rect_dev(rf(), 9, 7, M, 2, [P1, P2, P3, P4], [64, 64, 32, 16], 3, 2, 8, 6, [Q1, Q2, Q3, Q4],
                                                         [128, 128, 64, 32], P4, 96, STREAM))
    add("rgb rect dev short", lambda: S.rgb_upscale_rect_dev(rf(), 9, 7, 2, 2, [P1, P2], [64], 3, 2, 8, 6, [Q1], [128, 64, 32], Q2, 0, stream_object()))
    add("rgb rect dev min", lambda: S.rgb_upscale_rect_dev(None, 9, 7, 2, 2, None, None, 3, 2, 8, 6, None, None))
    add("rgb delta grid", lambda: (S.rgb_delta_grid(9, 7, M, 2, (32, 16)), S.rgb_delta_grid(9, 7, 2, 2)))
    add("rgb delta flags full", lambda: S.rgb_delta_flags_dev(rf(), 9, 7, M, 2, [P1, P2, P3, P4], [64, 64, 32, 16], [Q1, Q2, Q3, Q4], [128, 128, 64, 32],
                                                            (32, 16), P3, STREAM))
    add("rgb delta flags short", lambda: S.rgb_delta_flags_dev(rf(), 9, 7, 2, 2, [P1], [64, None], [Q1, None, Q3], [None], (0, 0), P3, stream_object()))
    add("rgb delta flags min", lambda: S.rgb_delta_flags_dev(None, 9, 7, 2, 2, None, None, [Q2], None, (0, 0), None))
    for cap in (None, 0, 3):
        add("rgb delta rects cap %r" % (cap,), lambda cap=cap: S.rgb_delta_rects(flags, (32, 16), rf(), 80, 30, [P1, P2, P3, P4], [256, 256, 128, 64], Q1, 96,
                                                                                 cap, item_size=104))
        add("rgb delta rects min cap %r" % (cap,), lambda cap=cap: S.rgb_delta_rects(flags, (32, 16), None, 80, 30, cap=cap))
    add("rgb delta rects short", lambda: S.rgb_delta_rects(flags, (32, 16), rf(), 80, 30, [P2], [None, 64], None, None, 2))
    add("rgb delta dev full", lambda: S.rgb_upscale_delta_dev(rf(), 9, 7, M, 2, [P1, P2, P3, P4], [64, 64, 32, 16], [Q1, Q2, Q3, Q4], [128, 128, 64, 32],
                                                            (32, 16), [P4, P3, P2, P1], [256, 256, 128, 64], Q4, 96, STREAM, True, 24))
    add("rgb delta dev short", lambda: S.rgb_upscale_delta_dev(rf(), 9, 7, 2, 2, [P1], [None], [Q1, Q2], [64], (0, 0), [P4], [256, None], None, None,
                                                             stream_object()))
    add("rgb delta dev min", lambda: S.rgb_upscale_delta_dev(None, 9, 7, 2, 2, None, None, [Q2], None, (0, 0), None, None, stats=False))
    return cases


def lib_holder(S):
    """The module whose global `_lib` lib() caches the loaded library in."""
    return sys.modules[S.lib.__module__]


def record(S):
    """{case: {"calls": [[symbol, args]], "result" | "raises": ...}} with a Recorder in place of the library."""
    holder = lib_holder(S)
    saved = holder._lib
    out = {}
    try:
        for name, thunk in _cases(S):
            rec = holder._lib = Recorder()
            assert name not in out, name
            try:
                out[name] = {"result": _plain(thunk())}
            except Exception as e:           # what a wrapper refuses in Python is part of its behaviour
                out[name] = {"raises": [type(e).__name__, str(e)]}
            out[name]["calls"] = rec.calls
        gc.collect()                         # no DeviceBuffer of a case lives on to free its made-up address in a real library
    finally:
        holder._lib = saved
    return out


def main():
    sys.path.insert(0, ROOT)
    import libsrcnn_amd as S
    for name, data in (("binding_surface.json", surface(S)), ("binding_record.json", record(S))):
        with open(os.path.join(ROOT, "tests", name), "w") as f:
            json.dump(data, f, indent=1, sort_keys=True)
            f.write("\n")
        print("wrote tests/%s (%d entries)" % (name, len(data)))


if __name__ == "__main__":
    main()
