"""The core of the binding: loading the library, errors, contexts / modes / profile / clock, device buffers, streams, events and
pinned arrays, and the marshalling helpers every call family is written with.  Each helper exists once."""
import ctypes as C
import os

import numpy as np

from . import abi
from .abi import DeltaStats, RectListPlan

__all__ = ["LIB_PATH", "SrcnnError", "lib", "check", "init", "init_devices", "context_count", "set_context", "shutdown", "device_count",
           "device_name", "set_mode", "set_relaxation", "sync", "STAGES", "profile_enable", "profile_reset", "clock_probe", "clock_read",
           "profile_read_context", "profile_read", "DeviceBuffer", "Stream", "Event", "PinnedArray", "output_size", "debug_settings"]

_HERE = os.path.dirname(os.path.abspath(__file__))
# SRCNN_AMD_LIB: another build of the same library (A/B runs of two kernel versions on one box: tools/lib_ab.py)
LIB_PATH = os.environ.get("SRCNN_AMD_LIB") or os.path.join(_HERE, "lib", "libsrcnn_amd.so")


class SrcnnError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__("libsrcnn_amd error %d: %s" % (code, msg))
        self.code = code


_lib = None


def lib():
    """Load the shared object (never builds, never falls back)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise ImportError("%s is missing -- run `python -m libsrcnn_amd.build` (hipcc, gfx950). "
                              "There is no CPU fallback." % LIB_PATH)
        L = C.CDLL(LIB_PATH)
        abi.declare(L, older_build=bool(os.environ.get("SRCNN_AMD_LIB")))
        _lib = L
    return _lib


def check(rc):
    if rc != 0:
        raise SrcnnError(rc, lib().srcnn_last_error().decode("utf-8", "replace"))


def _previous(prev):
    """The tail of the set_* calls: the previous value, or the library's error for a negative one."""
    if prev < 0:
        raise SrcnnError(prev, lib().srcnn_last_error().decode())
    return prev


def init(device=0):
    check(lib().srcnn_init(int(device)))


def init_devices(devices=None):
    """One context per entry of `devices` (HIP device ids; an id may repeat = virtual contexts); None = every visible device."""
    if devices is None:
        check(lib().srcnn_init_devices(None, 0))
    else:
        arr = (C.c_int * len(devices))(*devices)
        check(lib().srcnn_init_devices(arr, len(devices)))
    return lib().srcnn_context_count()


def context_count():
    return lib().srcnn_context_count()


def set_context(k):
    return _previous(lib().srcnn_set_context(int(k)))


def shutdown():
    lib().srcnn_shutdown()


def device_count():
    return lib().srcnn_device_count()


def device_name():
    buf = C.create_string_buffer(256)
    check(lib().srcnn_device_name(buf, 256))
    return buf.value.decode()


def set_mode(mode):
    return _previous(lib().srcnn_set_mode(int(mode)))


def set_relaxation(mask):
    """Which roundings MODE_RELAXED gives up (RELAX_* bits); returns the previous mask."""
    return _previous(lib().srcnn_set_relaxation(int(mask)))


def sync():
    check(lib().srcnn_device_sync())


STAGES = ("resample", "conv12", "conv3")


def profile_enable(on=True):
    return lib().srcnn_profile_enable(1 if on else 0)


def profile_reset():
    check(lib().srcnn_profile_reset())


def clock_probe(on=True):
    return lib().srcnn_debug_clock_probe(1 if on else 0)


def clock_read(context=0, cap=8192):
    """[(MHz, microseconds)] of every layer-1+2 launch since clock_probe(True), in launch order."""
    cyc = np.zeros(cap, np.uint64); tk = np.zeros(cap, np.uint64)
    n = min(_previous(lib().srcnn_debug_clock_read(int(context), cyc.ctypes.data, tk.ctypes.data, cap)), cap)
    t = np.maximum(tk[:n].astype(np.float64), 1.0)
    return [(float(c) / float(x) * 100.0, float(x) / 100.0) for c, x in zip(cyc[:n].astype(np.float64), t)]


def profile_read_context(k):
    """The same for context k alone (which device of a node-level call is the straggler)."""
    out = {}
    for st, name in enumerate(STAGES):
        ms, n = C.c_double(), C.c_ulonglong()
        check(lib().srcnn_profile_read_context(int(k), st, C.byref(ms), C.byref(n)))
        out[name] = (ms.value, n.value)
    return out


def profile_read():
    """{stage: (total_ms, launches)} accumulated by HIP events on the launch stream since the last reset."""
    out = {}
    for k, name in enumerate(STAGES):
        ms, n = C.c_double(0), C.c_ulonglong(0)
        check(lib().srcnn_profile_read(k, C.byref(ms), C.byref(n)))
        out[name] = (ms.value, n.value)
    return out


# ------------------------------------------------------------------------------------------------
# device buffers / streams / events: thin RAII over the C ABI (no torch needed)
# ------------------------------------------------------------------------------------------------
class DeviceBuffer:
    def __init__(self, nbytes):
        self.nbytes = int(nbytes)
        self.ptr = lib().srcnn_dev_alloc(self.nbytes)
        if not self.ptr:
            raise SrcnnError(-202, lib().srcnn_last_error().decode())

    @classmethod
    def from_numpy(cls, arr):
        arr = np.ascontiguousarray(arr)
        b = cls(arr.nbytes)
        check(lib().srcnn_memcpy_h2d(b.ptr, arr.ctypes.data, arr.nbytes, None))
        return b

    def upload(self, arr, offset=0):
        arr = np.ascontiguousarray(arr)
        assert offset + arr.nbytes <= self.nbytes
        check(lib().srcnn_memcpy_h2d(self.ptr + offset, arr.ctypes.data, arr.nbytes, None))

    def to_numpy(self, dtype, shape, offset=0):
        out = np.empty(shape, dtype)
        assert offset + out.nbytes <= self.nbytes
        check(lib().srcnn_memcpy_d2h(out.ctypes.data, self.ptr + offset, out.nbytes, None))
        return out

    def free(self):
        if self.ptr:
            lib().srcnn_dev_free(self.ptr)
            self.ptr = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class Stream:
    def __init__(self):
        h = C.c_void_p()
        check(lib().srcnn_stream_create(C.byref(h)))
        self.handle = h.value

    def sync(self):
        check(lib().srcnn_stream_sync(self.handle))

    def destroy(self):
        if self.handle:
            check(lib().srcnn_stream_destroy(self.handle))
            self.handle = None


class Event:
    def __init__(self):
        h = C.c_void_p()
        check(lib().srcnn_event_create(C.byref(h)))
        self.handle = h.value

    def record(self, stream=None):
        check(lib().srcnn_event_record(self.handle, stream.handle if stream else None))

    def elapsed_ms(self, stop):
        ms = C.c_float()
        check(lib().srcnn_event_elapsed_ms(self.handle, stop.handle, C.byref(ms)))
        return ms.value


class PinnedArray:
    """A numpy array on page-locked host memory from srcnn_host_alloc_pinned: srcnn_process_u8 / ProcessJob move such buffers
    to and from the device without staging copies.  Keep the object alive while the array is in use; free() when done."""

    def __init__(self, shape, dtype=np.uint8):
        self.shape, self.dtype = tuple(shape), np.dtype(dtype)
        self.nbytes = int(np.prod(self.shape)) * self.dtype.itemsize
        self.ptr = lib().srcnn_host_alloc_pinned(max(1, self.nbytes))
        if not self.ptr:
            raise SrcnnError(-202, lib().srcnn_last_error().decode())
        raw = (C.c_ubyte * max(1, self.nbytes)).from_address(self.ptr)
        self.array = np.frombuffer(raw, dtype=self.dtype, count=int(np.prod(self.shape))).reshape(self.shape)

    def free(self):
        if self.ptr:
            self.array = None
            lib().srcnn_host_free_pinned(self.ptr)
            self.ptr = None


def output_size(w, h, multiply, stepscale=False):
    ow, oh = C.c_uint(0), C.c_uint(0)
    rc = lib().srcnn_output_size(w, h, _f32(multiply), 1 if stepscale else 0, C.byref(ow), C.byref(oh))
    if rc != 0:
        raise SrcnnError(rc, "srcnn_output_size")
    return ow.value, oh.value


def debug_settings(markdown=False):
    """The SRCNN_* switches this process runs with (srcnn_debug_settings): text, one line per switch.  No device needed."""
    n = lib().srcnn_debug_settings(None, 0, 1 if markdown else 0)
    buf = C.create_string_buffer(n + 1)
    lib().srcnn_debug_settings(buf, n + 1, 1 if markdown else 0)
    return buf.value.decode()


# ------------------------------------------------------------------------------------------------
# marshalling: how the arguments of the wrappers become the arguments of the C calls
# ------------------------------------------------------------------------------------------------
def _addr(p):
    """A plane argument of the *_dev calls: None, an address, a DeviceBuffer, or (DeviceBuffer | address, byte offset)."""
    if p is None:
        return None
    if isinstance(p, tuple):
        base, off = p
        return _addr(base) + int(off)
    return p.ptr if isinstance(p, DeviceBuffer) else int(p)


def _handle(stream):
    """The stream argument of the *_dev calls: a Stream, a raw handle or None."""
    return stream.handle if isinstance(stream, Stream) else stream


def _wait(stream):
    """Block until what was queued on a stream argument is done."""
    if isinstance(stream, Stream):
        stream.sync()
    else:
        check(lib().srcnn_stream_sync(stream))


def _planes(xs, n):
    """void *[n] of up to n plane arguments (see _addr), the rest NULL; NULL for None."""
    return None if xs is None else (C.c_void_p * n)(*[_addr(x) for x in xs])


def _pitches(xs, n):
    """size_t[n] of up to n pitches in bytes (None or 0 = tight), the rest 0; NULL for None."""
    return None if xs is None else (C.c_size_t * n)(*[int(x or 0) for x in xs])


def _ref(struct):
    return C.byref(struct) if struct is not None else None


def _uints(fn, *args, n=4):
    """fn(*args, &out[0] .. &out[n - 1]) for the (no device) queries that answer in n unsigned out-parameters: the n values."""
    r = [C.c_uint(0) for _ in range(n)]
    check(fn(*args, *[C.byref(v) for v in r]))
    return tuple(v.value for v in r)


def _f32(multiply):
    """The library takes the factor as a float: what it will see, as the Python float that is passed."""
    return float(np.float32(multiply))


def _items(kind, items):
    """A ctypes array of the item struct `kind` from (x0, y0, rw, rh[, dst[, pitch[, dst_conv[, dst_conv_pitch]]]]) tuples, or
    `items` itself when it already is a ctypes array.  The struct says what a destination is: one plane argument and one pitch
    (RectItem, YuvPackedRectItem) or up to N of each (dst[N] / dst_pitch[N]), and whether there is a dst_conv.  What a tuple
    leaves out stays NULL / 0.  Returns (array or None, n)."""
    if isinstance(items, C.Array):
        return items, len(items)
    items = list(items)
    if not items:
        return None, 0
    (dst, dst_type), (pitch, _) = kind._fields_[4:6]
    arr = (kind * len(items))()
    for a, it in zip(arr, items):
        it = tuple(it)
        a.x0, a.y0, a.rw, a.rh = (int(v) for v in it[:4])
        to, to_pitch, conv, conv_pitch = (it[4:8] + (None,) * 4)[:4]
        if issubclass(dst_type, C.Array):
            for p, plane in enumerate(to or ()):
                getattr(a, dst)[p] = _addr(plane)
            for p, v in enumerate(to_pitch or ()):
                getattr(a, pitch)[p] = int(v or 0)
        else:
            setattr(a, dst, _addr(to))
            setattr(a, pitch, int(to_pitch or 0))
        if hasattr(kind, "dst_conv"):
            a.dst_conv, a.dst_conv_pitch = _addr(conv), int(conv_pitch or 0)
    return arr, len(items)


def _item_args(kind, items, n, item_size):
    """(items, n, item_size) as the list calls take them; n / item_size override what is passed (tests)."""
    arr, count = _items(kind, items) if items is not None else (None, 0)
    return (C.cast(arr, C.c_void_p) if arr is not None else None, count if n is None else int(n),
            C.sizeof(kind) if item_size is None else int(item_size))


def _list_plan(symbol, frame, kind, items, n, item_size, struct_size):
    """The *_rect_list_plan calls: `frame` are the marshalled arguments in front of the items."""
    plan = RectListPlan()
    plan.struct_size = C.sizeof(RectListPlan) if struct_size is None else int(struct_size)
    check(getattr(lib(), symbol)(*frame, *_item_args(kind, items, n, item_size), C.byref(plan)))
    return plan


def _list_dev(symbol, frame, kind, items, n, item_size, stream):
    """The *_rect_list_dev calls: `frame` are the marshalled arguments in front of the items."""
    check(getattr(lib(), symbol)(*frame, *_item_args(kind, items, n, item_size), _handle(stream)))


def _delta_rects(symbol, head, kind, cap, tail=()):
    """The *_delta_rects calls, count then fill: (item array, n), or n alone for cap == 0.  cap: None = as many items as
    needed; anything else is the capacity handed to the call (tests).  head / tail: the arguments around (items, cap)."""
    fn, n = getattr(lib(), symbol), C.c_uint(0)
    if cap is None or cap == 0:
        check(fn(*head, None, 0, *tail, C.byref(n)))
        if cap == 0:
            return n.value
        cap = n.value
    arr = (kind * max(1, int(cap)))()
    check(fn(*head, C.cast(arr, C.c_void_p), int(cap), *tail, C.byref(n)))
    return arr, n.value


def _delta_stats(stats, struct_size):
    """The DeltaStats a delta call fills (None with stats=False); struct_size overrides what it says of itself (tests)."""
    if not stats:
        return None
    st = DeltaStats()
    st.struct_size = C.sizeof(DeltaStats) if struct_size is None else int(struct_size)
    return st


class _Regions:
    """The outputs of a *_rects convenience as regions of ONE device buffer, each from a 16-byte boundary: add() while laying
    out, alloc() the buffer, and after the call download() once and take() every region back out."""

    def __init__(self):
        self.total = 0

    def add(self, nbytes):
        at = self.total
        self.total += (nbytes + 15) & ~15
        return at

    def alloc(self):
        self.buf = DeviceBuffer(max(16, self.total))
        return self.buf

    def download(self):
        self.flat = self.buf.to_numpy(np.uint8, (max(16, self.total),))

    def take(self, at, dtype, shape):
        return self.flat[at:at + int(np.prod(shape)) * np.dtype(dtype).itemsize].view(dtype).reshape(shape).copy()
