"""libsrcnn_amd -- MI355X-native SRCNN Y-channel path behind the rageworx/libsrcnn interface.

The product is libsrcnn_amd/lib/libsrcnn_amd.so (hand-written gfx950 kernels + C ABI
include/srcnn_amd.h + the C++ drop-in symbols ProcessSRCNN / ConfigureFilterSRCNN).  This module
is only the ctypes binding used by tests/, bench.py and __graft_entry__.py; it mirrors the
reference's two public calls (src/libsrcnn.h:46-54) and exposes the planar-float Y entry points.

There is no CPU compute path here: if the shared object is missing, or no gfx950 device is
visible, calls raise.
"""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
# SRCNN_AMD_LIB: another build of the same library (A/B runs of two kernel versions on one box: tools/lib_ab.py)
LIB_PATH = os.environ.get("SRCNN_AMD_LIB") or os.path.join(_HERE, "lib", "libsrcnn_amd.so")

SRCNNF_Nearest, SRCNNF_Bilinear, SRCNNF_Bicubic, SRCNNF_Lanczos3, SRCNNF_Bspline = range(5)
MODE_STRICT, MODE_FAST, MODE_FAST_F16, MODE_RELAXED = 0, 1, 2, 3
RELAX_L1, RELAX_L2, RELAX_L3_X64, RELAX_L3_F32 = 1, 2, 4, 8

# The STABLE C ABI: every function include/srcnn_amd.h declares, frozen at ABI 5 (include/srcnn_amd.abi is the committed list;
# tests/test_abi.py holds header, list, this binding and the library's export table to each other)
STABLE_ABI_SYMBOLS = [
    "srcnn_abi_version", "srcnn_device_count", "srcnn_init", "srcnn_init_devices", "srcnn_context_count",
    "srcnn_context_device", "srcnn_set_context", "srcnn_get_context", "srcnn_shutdown", "srcnn_trim",
    "srcnn_last_error", "srcnn_set_mode", "srcnn_get_mode", "srcnn_device_name", "srcnn_set_workspace_limit",
    "srcnn_dev_alloc", "srcnn_dev_free", "srcnn_host_alloc_pinned", "srcnn_host_free_pinned", "srcnn_memcpy_h2d",
    "srcnn_memcpy_d2h", "srcnn_memset_dev", "srcnn_stream_create", "srcnn_stream_destroy", "srcnn_stream_sync",
    "srcnn_device_sync", "srcnn_event_create", "srcnn_event_destroy", "srcnn_event_record",
    "srcnn_stream_wait_event", "srcnn_event_elapsed_ms", "srcnn_profile_enable", "srcnn_profile_reset",
    "srcnn_profile_read", "srcnn_profile_read_context", "srcnn_y_upscale2x_f32_dev",
    "srcnn_y_upscale2x_f32_batch_dev", "srcnn_y_upscale2x_f32_band_dev", "srcnn_y_upscale2x_f32_node_dev",
    "srcnn_batch_graph_create", "srcnn_batch_graph_launch", "srcnn_batch_graph_destroy", "srcnn_y_path_f32_dev",
    "srcnn_resample_f32_dev", "srcnn_conv1_f32_dev", "srcnn_conv2_f32_dev", "srcnn_conv3_f32_dev",
    "srcnn_conv12_f32_dev", "srcnn_y_upscale2x_f32", "srcnn_y_upscale2x_f32_batch", "srcnn_y_upscale2x_f32_stream",
    "srcnn_y_path_f32", "srcnn_process_u8", "srcnn_process_u8_begin", "srcnn_process_u8_wait", "srcnn_delete_array",
    "srcnn_output_size", "srcnn_comm_unique_id", "srcnn_comm_init", "srcnn_comm_destroy", "srcnn_comm_rank",
    "srcnn_comm_gather_f32", "srcnn_comm_gatherv_f32", "srcnn_comm_gatherv_at_f32",
    "srcnn_comm_tiled_y_upscale2x_f32_dev", "srcnn_band_rows", "srcnn_tiled_piece", "srcnn_comm_allgather_f32",
    "srcnn_comm_barrier", "srcnn_comm_wait", "srcnn_comm_set_timeout_ms",
]
# instruments (include/srcnn_amd_debug.h): test hooks, diagnostics, the relaxation experiment -- no compatibility promise
DEBUG_SYMBOLS = [
    "srcnn_set_relaxation", "srcnn_axis_table", "srcnn_fused_diag", "srcnn_debug_counts", "srcnn_debug_settings",
    "srcnn_debug_clock_probe", "srcnn_debug_clock_read", "srcnn_debug_band_plan", "srcnn_debug_process_phases", "srcnn_debug_stream_mode",
]
# the YUV 4:2:0 extension (include/srcnn_amd_yuv.h, listed in include/srcnn_amd_yuv.abi; versioned on its own)
YUV_SYMBOLS = ["srcnn_yuv_abi_version", "srcnn_yuv420_upscale_dev"]
# the high-bit-depth / 4:2:2 / 4:4:4 YUV extension (include/srcnn_amd_yuv_ex.h, listed in include/srcnn_amd_yuv_ex.abi; its own version)
YUV_EX_SYMBOLS = ["srcnn_yuv_ex_abi_version", "srcnn_yuv_plane_size", "srcnn_yuv_upscale_dev"]
# RGB(A) images already in device memory (include/srcnn_amd_rgb.h, listed in include/srcnn_amd_rgb.abi; its own version)
RGB_SYMBOLS = ["srcnn_rgb_abi_version", "srcnn_rgb_plane_size", "srcnn_rgb_upscale_dev"]
# packed YUV frames (include/srcnn_amd_yuv_packed.h, listed in include/srcnn_amd_yuv_packed.abi; its own version)
YUV_PACKED_SYMBOLS = ["srcnn_yuv_packed_abi_version", "srcnn_yuv_packed_row_bytes", "srcnn_yuv_packed_upscale_dev"]
# one rectangle of the Y path's output (include/srcnn_amd_rect.h, listed in include/srcnn_amd_rect.abi; its own version)
RECT_SYMBOLS = ["srcnn_rect_abi_version", "srcnn_y_path_rect_source", "srcnn_y_path_rect_f32_dev"]
# one rectangle of an RGB(A) image (include/srcnn_amd_rgb_rect.h, listed in include/srcnn_amd_rgb_rect.abi; its own version)
RGB_RECT_SYMBOLS = ["srcnn_rgb_rect_abi_version", "srcnn_rgb_rect_source", "srcnn_rgb_upscale_rect_dev"]
# one rectangle of a planar / semi-planar YUV frame (include/srcnn_amd_yuv_rect.h, listed in include/srcnn_amd_yuv_rect.abi; its own version)
YUV_RECT_SYMBOLS = ["srcnn_yuv_rect_abi_version", "srcnn_yuv_rect_source", "srcnn_yuv_upscale_rect_dev"]
# one rectangle of a packed YUV frame (include/srcnn_amd_yuv_packed_rect.h, listed in include/srcnn_amd_yuv_packed_rect.abi; its own version)
YUV_PACKED_RECT_SYMBOLS = ["srcnn_yuv_packed_rect_abi_version", "srcnn_yuv_packed_span_bytes", "srcnn_yuv_packed_rect_source",
                           "srcnn_yuv_packed_upscale_rect_dev"]
# a list of rectangles of the Y path's output (include/srcnn_amd_rect_list.h, listed in include/srcnn_amd_rect_list.abi; its own version)
RECT_LIST_SYMBOLS = ["srcnn_rect_list_abi_version", "srcnn_y_path_rect_list_plan", "srcnn_y_path_rect_list_f32_dev"]
# a list of rectangles of an RGB(A) image (include/srcnn_amd_rgb_rect_list.h, listed in include/srcnn_amd_rgb_rect_list.abi; its own version)
RGB_RECT_LIST_SYMBOLS = ["srcnn_rgb_rect_list_abi_version", "srcnn_rgb_upscale_rect_list_plan", "srcnn_rgb_upscale_rect_list_dev"]
# a list of rectangles of a planar / semi-planar YUV frame (include/srcnn_amd_yuv_rect_list.h, listed in include/srcnn_amd_yuv_rect_list.abi; its own version)
YUV_RECT_LIST_SYMBOLS = ["srcnn_yuv_rect_list_abi_version", "srcnn_yuv_upscale_rect_list_plan", "srcnn_yuv_upscale_rect_list_dev"]
# a list of rectangles of a packed YUV frame (include/srcnn_amd_yuv_packed_rect_list.h, listed in include/srcnn_amd_yuv_packed_rect_list.abi; its own version)
YUV_PACKED_RECT_LIST_SYMBOLS = ["srcnn_yuv_packed_rect_list_abi_version", "srcnn_yuv_packed_upscale_rect_list_plan",
                                "srcnn_yuv_packed_upscale_rect_list_dev"]
# only what changed between two Y frames (include/srcnn_amd_delta.h, listed in include/srcnn_amd_delta.abi; its own version)
DELTA_SYMBOLS = ["srcnn_delta_abi_version", "srcnn_y_path_delta_grid", "srcnn_y_path_delta_flags_dev", "srcnn_y_path_delta_rects",
                 "srcnn_y_path_delta_f32_dev"]
# only what changed between two RGB(A) images (include/srcnn_amd_rgb_delta.h, listed in include/srcnn_amd_rgb_delta.abi; its own version)
RGB_DELTA_SYMBOLS = ["srcnn_rgb_delta_abi_version", "srcnn_rgb_delta_grid", "srcnn_rgb_delta_flags_dev", "srcnn_rgb_delta_rects",
                     "srcnn_rgb_upscale_delta_dev"]
C_ABI_SYMBOLS = STABLE_ABI_SYMBOLS + DEBUG_SYMBOLS + YUV_SYMBOLS + YUV_EX_SYMBOLS + RGB_SYMBOLS + YUV_PACKED_SYMBOLS + RECT_SYMBOLS + RGB_RECT_SYMBOLS + YUV_RECT_SYMBOLS + YUV_PACKED_RECT_SYMBOLS + RECT_LIST_SYMBOLS + RGB_RECT_LIST_SYMBOLS + YUV_RECT_LIST_SYMBOLS + YUV_PACKED_RECT_LIST_SYMBOLS + DELTA_SYMBOLS + RGB_DELTA_SYMBOLS   # everything the library exports besides the two C++ symbols
CXX_SYMBOLS = ["_Z20ConfigureFilterSRCNN15SRCNNFilterTypeb", "_Z12ProcessSRCNNPKhjjjfRPhRjPS1_Pj"]


class YuvFormat(C.Structure):
    """srcnn_yuv_format (include/srcnn_amd_yuv_ex.h)."""
    _fields_ = [("struct_size", C.c_uint), ("layout", C.c_int), ("chroma", C.c_int), ("depth", C.c_int), ("msb_aligned", C.c_int)]


class RgbFormat(C.Structure):
    """srcnn_rgb_format (include/srcnn_amd_rgb.h)."""
    _fields_ = [("struct_size", C.c_uint), ("layout", C.c_int), ("order", C.c_int), ("alpha", C.c_int), ("depth", C.c_int)]


class RectItem(C.Structure):
    """srcnn_rect_item (include/srcnn_amd_rect_list.h)."""
    _fields_ = [("x0", C.c_uint), ("y0", C.c_uint), ("rw", C.c_uint), ("rh", C.c_uint), ("d_out", C.c_void_p), ("out_pitch", C.c_size_t)]


class RgbRectItem(C.Structure):
    """srcnn_rgb_rect_item (include/srcnn_amd_rgb_rect_list.h)."""
    _fields_ = [("x0", C.c_uint), ("y0", C.c_uint), ("rw", C.c_uint), ("rh", C.c_uint), ("dst", C.c_void_p * 4), ("dst_pitch", C.c_size_t * 4),
                ("dst_conv", C.c_void_p), ("dst_conv_pitch", C.c_size_t)]


class YuvRectItem(C.Structure):
    """srcnn_yuv_rect_item (include/srcnn_amd_yuv_rect_list.h)."""
    _fields_ = [("x0", C.c_uint), ("y0", C.c_uint), ("rw", C.c_uint), ("rh", C.c_uint), ("dst", C.c_void_p * 3), ("dst_pitch", C.c_size_t * 3)]


class YuvPackedRectItem(C.Structure):
    """srcnn_yuv_packed_rect_item (include/srcnn_amd_yuv_packed_rect_list.h)."""
    _fields_ = [("x0", C.c_uint), ("y0", C.c_uint), ("rw", C.c_uint), ("rh", C.c_uint), ("dst", C.c_void_p), ("dst_pitch", C.c_size_t)]


class RectListPlan(C.Structure):
    """srcnn_rect_list_plan (include/srcnn_amd_rect_list.h)."""
    _fields_ = [("struct_size", C.c_uint), ("batched_items", C.c_uint), ("single_items", C.c_uint), ("atlases", C.c_uint),
                ("cell_samples", C.c_ulonglong), ("atlas_samples", C.c_ulonglong), ("scratch_bytes", C.c_ulonglong)]


class DeltaStats(C.Structure):
    """srcnn_delta_stats (include/srcnn_amd_delta.h)."""
    _fields_ = [("struct_size", C.c_uint), ("tiles", C.c_uint), ("dirty_tiles", C.c_uint), ("rects", C.c_uint), ("whole_frame", C.c_uint),
                ("cell_samples", C.c_ulonglong)]


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
        vp, u, f, sz, i = C.c_void_p, C.c_uint, C.c_float, C.c_size_t, C.c_int
        sig = {
            "srcnn_abi_version": (i, []), "srcnn_device_count": (i, []), "srcnn_init": (i, [i]),
            "srcnn_init_devices": (i, [C.POINTER(i), i]), "srcnn_context_count": (i, []), "srcnn_context_device": (i, [i]),
            "srcnn_set_context": (i, [i]), "srcnn_get_context": (i, []), "srcnn_trim": (i, []),
            "srcnn_y_upscale2x_f32_node_dev": (i, [vp, u, u, vp, i]),
            "srcnn_comm_gatherv_at_f32": (i, [vp, C.POINTER(sz), C.POINTER(sz), vp, i, vp]),
            "srcnn_comm_tiled_y_upscale2x_f32_dev": (i, [vp, u, u, vp, vp, i, i, vp]),
            "srcnn_band_rows": (i, [u, i, i, C.POINTER(u), C.POINTER(u)]),
            "srcnn_tiled_piece": (i, [u, u, i, i, i, i, C.POINTER(u), C.POINTER(u)]),
            "srcnn_debug_band_plan": (i, [u, u, u, i, C.POINTER(u), i]),
            "srcnn_shutdown": (None, []), "srcnn_last_error": (C.c_char_p, []), "srcnn_set_mode": (i, [i]),
            "srcnn_get_mode": (i, []), "srcnn_set_relaxation": (i, [u]), "srcnn_device_name": (i, [C.c_char_p, sz]),
            "srcnn_set_workspace_limit": (sz, [sz]),
            "srcnn_dev_alloc": (vp, [sz]), "srcnn_dev_free": (None, [vp]),
            "srcnn_host_alloc_pinned": (vp, [sz]), "srcnn_host_free_pinned": (None, [vp]),
            "srcnn_memcpy_h2d": (i, [vp, vp, sz, vp]), "srcnn_memcpy_d2h": (i, [vp, vp, sz, vp]),
            "srcnn_memset_dev": (i, [vp, i, sz, vp]),
            "srcnn_stream_create": (i, [C.POINTER(vp)]), "srcnn_stream_destroy": (i, [vp]),
            "srcnn_stream_sync": (i, [vp]), "srcnn_device_sync": (i, []),
            "srcnn_event_create": (i, [C.POINTER(vp)]), "srcnn_event_destroy": (i, [vp]),
            "srcnn_event_record": (i, [vp, vp]), "srcnn_event_elapsed_ms": (i, [vp, vp, C.POINTER(f)]),
            "srcnn_stream_wait_event": (i, [vp, vp]),
            "srcnn_profile_enable": (i, [i]), "srcnn_profile_reset": (i, []),
            "srcnn_profile_read": (i, [i, C.POINTER(C.c_double), C.POINTER(C.c_ulonglong)]),
            "srcnn_profile_read_context": (i, [i, i, C.POINTER(C.c_double), C.POINTER(C.c_ulonglong)]),
            "srcnn_y_upscale2x_f32_dev": (i, [vp, u, u, vp, vp]),
            "srcnn_y_upscale2x_f32_batch_dev": (i, [vp, u, u, u, vp, vp]),
            "srcnn_y_upscale2x_f32_band_dev": (i, [vp, u, u, u, u, vp, vp]),
            "srcnn_batch_graph_create": (i, [vp, u, u, u, vp, vp, C.POINTER(vp)]),
            "srcnn_batch_graph_launch": (i, [vp]), "srcnn_batch_graph_destroy": (i, [vp]),
            "srcnn_y_path_f32_dev": (i, [vp, u, u, u, u, i, vp, vp]),
            "srcnn_resample_f32_dev": (i, [vp, u, u, u, u, i, vp, vp]),
            "srcnn_conv1_f32_dev": (i, [vp, u, u, vp, vp]), "srcnn_conv2_f32_dev": (i, [vp, u, u, vp, vp]),
            "srcnn_conv3_f32_dev": (i, [vp, u, u, vp, vp]), "srcnn_conv12_f32_dev": (i, [vp, u, u, vp, vp]),
            "srcnn_y_upscale2x_f32": (i, [vp, u, u, vp]), "srcnn_y_upscale2x_f32_batch": (i, [vp, u, u, u, vp]),
            "srcnn_y_path_f32": (i, [vp, u, u, u, u, i, vp]),
            "srcnn_y_upscale2x_f32_stream": (i, [vp, u, u, u, vp, i]),
            "srcnn_process_u8": (i, [vp, u, u, u, f, i, vp, vp]),
            "srcnn_process_u8_begin": (i, [vp, u, u, u, f, i, vp, vp, C.POINTER(vp)]), "srcnn_process_u8_wait": (i, [vp]),
            "srcnn_delete_array": (None, [vp]),
            "srcnn_output_size": (i, [u, u, f, i, C.POINTER(u), C.POINTER(u)]),
            "srcnn_axis_table": (i, [i, u, u, vp, vp, vp]),
            "srcnn_comm_unique_id": (i, [vp]), "srcnn_comm_init": (i, [vp, i, i]), "srcnn_comm_destroy": (i, []),
            "srcnn_comm_gather_f32": (i, [vp, sz, vp, i, vp]), "srcnn_comm_allgather_f32": (i, [vp, sz, vp, vp]),
            "srcnn_comm_gatherv_f32": (i, [vp, C.POINTER(sz), vp, i, vp]),
            "srcnn_comm_rank": (i, [C.POINTER(i), C.POINTER(i)]),
            "srcnn_debug_counts": (i, [C.POINTER(i), C.POINTER(i)]),
            "srcnn_fused_diag": (i, [vp, u, u, vp, vp, vp]),
            "srcnn_debug_clock_probe": (i, [i]), "srcnn_debug_clock_read": (i, [i, vp, vp, i]),
            "srcnn_debug_settings": (i, [C.c_char_p, sz, i]),
            "srcnn_debug_process_phases": (i, [C.POINTER(C.c_double), i]),
            "srcnn_debug_stream_mode": (i, [C.POINTER(u), C.POINTER(u), C.POINTER(i)]),
            "srcnn_comm_barrier": (i, [vp]), "srcnn_comm_wait": (i, [vp]), "srcnn_comm_set_timeout_ms": (i, [i]),
            "srcnn_yuv_abi_version": (i, []),
            "srcnn_yuv420_upscale_dev": (i, [i, u, u, f, i, C.POINTER(vp), C.POINTER(sz), C.POINTER(vp), C.POINTER(sz), vp]),
            "srcnn_yuv_ex_abi_version": (i, []),
            "srcnn_yuv_plane_size": (i, [C.POINTER(YuvFormat), u, u, i, C.POINTER(u), C.POINTER(u), C.POINTER(sz)]),
            "srcnn_yuv_upscale_dev": (i, [C.POINTER(YuvFormat), u, u, f, i, C.POINTER(vp), C.POINTER(sz), C.POINTER(vp), C.POINTER(sz), vp]),
            "srcnn_rgb_abi_version": (i, []),
            "srcnn_rgb_plane_size": (i, [C.POINTER(RgbFormat), u, u, i, C.POINTER(u), C.POINTER(u), C.POINTER(sz)]),
            "srcnn_rgb_upscale_dev": (i, [C.POINTER(RgbFormat), u, u, f, i, C.POINTER(vp), C.POINTER(sz), C.POINTER(vp), C.POINTER(sz), vp, sz, vp]),
            "srcnn_yuv_packed_abi_version": (i, []),
            "srcnn_yuv_packed_row_bytes": (i, [i, u, C.POINTER(sz), C.POINTER(u)]),
            "srcnn_yuv_packed_upscale_dev": (i, [i, u, u, f, i, vp, sz, vp, sz, vp]),
            "srcnn_rect_abi_version": (i, []),
            "srcnn_y_path_rect_source": (i, [u, u, u, u, i, u, u, u, u, C.POINTER(u), C.POINTER(u), C.POINTER(u), C.POINTER(u)]),
            "srcnn_y_path_rect_f32_dev": (i, [vp, sz, u, u, u, u, i, u, u, u, u, vp, sz, vp]),
            "srcnn_rgb_rect_abi_version": (i, []),
            "srcnn_rgb_rect_source": (i, [u, u, f, i, u, u, u, u, C.POINTER(u), C.POINTER(u), C.POINTER(u), C.POINTER(u)]),
            "srcnn_rgb_upscale_rect_dev": (i, [C.POINTER(RgbFormat), u, u, f, i, C.POINTER(vp), C.POINTER(sz), u, u, u, u,
                                               C.POINTER(vp), C.POINTER(sz), vp, sz, vp]),
            "srcnn_yuv_rect_abi_version": (i, []),
            "srcnn_yuv_rect_source": (i, [C.POINTER(YuvFormat), u, u, f, i, u, u, u, u, i, C.POINTER(u), C.POINTER(u), C.POINTER(u), C.POINTER(u)]),
            "srcnn_yuv_upscale_rect_dev": (i, [C.POINTER(YuvFormat), u, u, f, i, C.POINTER(vp), C.POINTER(sz), u, u, u, u,
                                               C.POINTER(vp), C.POINTER(sz), vp]),
            "srcnn_yuv_packed_rect_abi_version": (i, []),
            "srcnn_yuv_packed_span_bytes": (i, [i, u, u, u, C.POINTER(u), C.POINTER(sz), C.POINTER(sz)]),
            "srcnn_yuv_packed_rect_source": (i, [i, u, u, f, i, u, u, u, u, C.POINTER(u), C.POINTER(u), C.POINTER(u), C.POINTER(u)]),
            "srcnn_yuv_packed_upscale_rect_dev": (i, [i, u, u, f, i, vp, sz, u, u, u, u, vp, sz, vp]),
            "srcnn_rect_list_abi_version": (i, []),
            "srcnn_y_path_rect_list_plan": (i, [u, u, u, u, i, vp, u, u, C.POINTER(RectListPlan)]),
            "srcnn_y_path_rect_list_f32_dev": (i, [vp, sz, u, u, u, u, i, vp, u, u, vp]),
            "srcnn_rgb_rect_list_abi_version": (i, []),
            "srcnn_rgb_upscale_rect_list_plan": (i, [C.POINTER(RgbFormat), u, u, f, i, vp, u, u, C.POINTER(RectListPlan)]),
            "srcnn_rgb_upscale_rect_list_dev": (i, [C.POINTER(RgbFormat), u, u, f, i, C.POINTER(vp), C.POINTER(sz), vp, u, u, vp]),
            "srcnn_yuv_rect_list_abi_version": (i, []),
            "srcnn_yuv_upscale_rect_list_plan": (i, [C.POINTER(YuvFormat), u, u, f, i, vp, u, u, C.POINTER(RectListPlan)]),
            "srcnn_yuv_upscale_rect_list_dev": (i, [C.POINTER(YuvFormat), u, u, f, i, C.POINTER(vp), C.POINTER(sz), vp, u, u, vp]),
            "srcnn_yuv_packed_rect_list_abi_version": (i, []),
            "srcnn_yuv_packed_upscale_rect_list_plan": (i, [i, u, u, f, i, vp, u, u, C.POINTER(RectListPlan)]),
            "srcnn_yuv_packed_upscale_rect_list_dev": (i, [i, u, u, f, i, vp, sz, vp, u, u, vp]),
            "srcnn_delta_abi_version": (i, []),
            "srcnn_y_path_delta_grid": (i, [u, u, u, u, i, u, u, C.POINTER(u), C.POINTER(u)]),
            "srcnn_y_path_delta_flags_dev": (i, [vp, sz, vp, sz, u, u, u, u, i, u, u, vp, vp]),
            "srcnn_y_path_delta_rects": (i, [vp, u, u, u, u, u, u, vp, sz, vp, u, C.POINTER(u)]),
            "srcnn_y_path_delta_f32_dev": (i, [vp, sz, vp, sz, u, u, u, u, i, u, u, vp, sz, vp, C.POINTER(DeltaStats)]),
            "srcnn_rgb_delta_abi_version": (i, []),
            "srcnn_rgb_delta_grid": (i, [u, u, f, i, u, u, C.POINTER(u), C.POINTER(u), C.POINTER(u), C.POINTER(u)]),
            "srcnn_rgb_delta_flags_dev": (i, [C.POINTER(RgbFormat), u, u, f, i, C.POINTER(vp), C.POINTER(sz), C.POINTER(vp), C.POINTER(sz), u, u, vp, vp]),
            "srcnn_rgb_delta_rects": (i, [vp, u, u, u, u, C.POINTER(RgbFormat), u, u, C.POINTER(vp), C.POINTER(sz), vp, sz, vp, u, u, C.POINTER(u)]),
            "srcnn_rgb_upscale_delta_dev": (i, [C.POINTER(RgbFormat), u, u, f, i, C.POINTER(vp), C.POINTER(sz), C.POINTER(vp), C.POINTER(sz), u, u,
                                                C.POINTER(vp), C.POINTER(sz), vp, sz, vp, C.POINTER(DeltaStats)]),
        }
        for name, (res, args) in sig.items():
            if name in DEBUG_SYMBOLS + YUV_SYMBOLS + YUV_EX_SYMBOLS + RGB_SYMBOLS + YUV_PACKED_SYMBOLS + RECT_SYMBOLS + RGB_RECT_SYMBOLS + YUV_RECT_SYMBOLS + YUV_PACKED_RECT_SYMBOLS + RECT_LIST_SYMBOLS + RGB_RECT_LIST_SYMBOLS + YUV_RECT_LIST_SYMBOLS + YUV_PACKED_RECT_LIST_SYMBOLS + DELTA_SYMBOLS + RGB_DELTA_SYMBOLS and not hasattr(L, name) and os.environ.get("SRCNN_AMD_LIB"):
                continue                  # an older build loaded for an A/B run (tools/lib_ab.py): it may lack newer entry points
            fn = getattr(L, name)
            fn.restype, fn.argtypes = res, args
        cfg = getattr(L, CXX_SYMBOLS[0])
        cfg.restype, cfg.argtypes = None, [i, C.c_bool]
        prc = getattr(L, CXX_SYMBOLS[1])
        # references are passed as pointers in the Itanium C++ ABI
        prc.restype = i
        prc.argtypes = [vp, u, u, u, f, C.POINTER(vp), C.POINTER(u), C.POINTER(vp), C.POINTER(u)]
        _lib = L
    return _lib


def check(rc):
    if rc != 0:
        raise SrcnnError(rc, lib().srcnn_last_error().decode("utf-8", "replace"))


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
    prev = lib().srcnn_set_context(int(k))
    if prev < 0:
        raise SrcnnError(prev, lib().srcnn_last_error().decode())
    return prev


def shutdown():
    lib().srcnn_shutdown()


def device_count():
    return lib().srcnn_device_count()


def device_name():
    buf = C.create_string_buffer(256)
    check(lib().srcnn_device_name(buf, 256))
    return buf.value.decode()


def set_mode(mode):
    prev = lib().srcnn_set_mode(int(mode))
    if prev < 0:
        raise SrcnnError(prev, lib().srcnn_last_error().decode())
    return prev


def set_relaxation(mask):
    """Which roundings MODE_RELAXED gives up (RELAX_* bits); returns the previous mask."""
    prev = lib().srcnn_set_relaxation(int(mask))
    if prev < 0:
        raise SrcnnError(prev, lib().srcnn_last_error().decode())
    return prev


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
    n = lib().srcnn_debug_clock_read(int(context), cyc.ctypes.data, tk.ctypes.data, cap)
    if n < 0:
        raise SrcnnError(n, lib().srcnn_last_error().decode())
    n = min(n, cap)
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
    din = DeviceBuffer.from_numpy(y)
    dout = DeviceBuffer(rows * 2 * w * 4)
    check(lib().srcnn_y_upscale2x_f32_band_dev(din.ptr, w, h, row0, rows, dout.ptr, None))
    sync()
    return dout.to_numpy(np.float32, (rows, 2 * w))


def y_path_rect_source(w, h, dw, dh, filt, x0, y0, rw, rh):
    """(sx0, sy0, sw, sh): the source rectangle output rect [x0, x0 + rw) x [y0, y0 + rh) of the dw x dh Y path depends on
    (srcnn_y_path_rect_source; no device)."""
    r = [C.c_uint(0) for _ in range(4)]
    check(lib().srcnn_y_path_rect_source(int(w), int(h), int(dw), int(dh), int(filt), int(x0), int(y0), int(rw), int(rh),
                                         *[C.byref(v) for v in r]))
    return tuple(v.value for v in r)


def y_path_rect_dev(src, in_pitch, w, h, dw, dh, filt, x0, y0, rw, rh, dst, out_pitch, stream=None):
    """srcnn_y_path_rect_f32_dev on device memory, as given: src / dst plane arguments (see _addr), pitches in bytes (0 =
    tight).  Asynchronous on `stream` (a Stream, a raw handle or None); raises SrcnnError with the library's code."""
    handle = stream.handle if isinstance(stream, Stream) else stream
    check(lib().srcnn_y_path_rect_f32_dev(_addr(src), int(in_pitch or 0), int(w), int(h), int(dw), int(dh), int(filt), int(x0), int(y0),
                                          int(rw), int(rh), _addr(dst), int(out_pitch or 0), handle))


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
    if isinstance(items, C.Array):
        return items, len(items)
    items = list(items)
    if not items:
        return None, 0
    arr = (RectItem * len(items))()
    for k, it in enumerate(items):
        it = tuple(it)
        arr[k].x0, arr[k].y0, arr[k].rw, arr[k].rh = (int(v) for v in it[:4])
        arr[k].d_out = _addr(it[4]) if len(it) > 4 else None
        arr[k].out_pitch = int(it[5] or 0) if len(it) > 5 else 0
    return arr, len(items)


def y_path_rect_list_plan(w, h, dw, dh, filt, items, n=None, item_size=None, struct_size=None):
    """srcnn_y_path_rect_list_plan (no device): how the list call routes and packs `items` (see rect_items) at the current mode,
    workspace limit and switches.  Returns the RectListPlan.  n / item_size / struct_size override what is passed (tests)."""
    arr, count = rect_items(items) if items is not None else (None, 0)
    plan = RectListPlan()
    plan.struct_size = C.sizeof(RectListPlan) if struct_size is None else int(struct_size)
    check(lib().srcnn_y_path_rect_list_plan(int(w), int(h), int(dw), int(dh), int(filt), C.cast(arr, C.c_void_p) if arr is not None else None,
                                            count if n is None else int(n), C.sizeof(RectItem) if item_size is None else int(item_size),
                                            C.byref(plan)))
    return plan


def y_path_rect_list_dev(src, in_pitch, w, h, dw, dh, filt, items, stream=None, n=None, item_size=None):
    """srcnn_y_path_rect_list_f32_dev on device memory, as given: src is the whole source plane (see _addr), items the rects with
    their destinations (see rect_items).  Asynchronous on `stream` (a Stream, a raw handle or None); the item array is read
    before the call returns.  Raises SrcnnError with the library's code."""
    handle = stream.handle if isinstance(stream, Stream) else stream
    arr, count = rect_items(items) if items is not None else (None, 0)
    check(lib().srcnn_y_path_rect_list_f32_dev(_addr(src), int(in_pitch or 0), int(w), int(h), int(dw), int(dh), int(filt),
                                               C.cast(arr, C.c_void_p) if arr is not None else None, count if n is None else int(n),
                                               C.sizeof(RectItem) if item_size is None else int(item_size), handle))


def y_path_delta_grid(w, h, dw, dh, filt, tile=(0, 0)):
    """(cols, rows) of the delta call's tile grid (srcnn_y_path_delta_grid; no device).  tile: (tile_w, tile_h), 0 = the default 64."""
    cols, rows = C.c_uint(0), C.c_uint(0)
    check(lib().srcnn_y_path_delta_grid(int(w), int(h), int(dw), int(dh), int(filt), int(tile[0]), int(tile[1]), C.byref(cols), C.byref(rows)))
    return cols.value, rows.value


def y_path_delta_flags_dev(prev, prev_pitch, cur, cur_pitch, w, h, dw, dh, filt, tile, flags, stream=None):
    """srcnn_y_path_delta_flags_dev on device memory, as given: prev (None = no previous frame) / cur are whole source planes and
    flags receives cols x rows bytes (see _addr), pitches in bytes (0 = tight).  Asynchronous on `stream`."""
    handle = stream.handle if isinstance(stream, Stream) else stream
    check(lib().srcnn_y_path_delta_flags_dev(_addr(prev), int(prev_pitch or 0), _addr(cur), int(cur_pitch or 0), int(w), int(h), int(dw), int(dh),
                                             int(filt), int(tile[0]), int(tile[1]), _addr(flags), handle))


def y_path_delta_rects(flags, tile, dw, dh, out=None, out_pitch=0, cap=None):
    """srcnn_y_path_delta_rects (pure host): the coalescer over a (rows, cols) uint8 array of flags of tile[0] x tile[1] tiles.
    Returns [(x0, y0, rw, rh, d_out, out_pitch)].  cap: None = as many items as needed; 0 = count only (returns the number);
    anything else is the capacity handed to the call (tests)."""
    flags = np.ascontiguousarray(flags, np.uint8)
    rows, cols = flags.shape
    n = C.c_uint(0)
    args = (flags.ctypes.data, cols, rows, int(tile[0]), int(tile[1]), int(dw), int(dh), _addr(out), int(out_pitch or 0))
    if cap is None or cap == 0:
        check(lib().srcnn_y_path_delta_rects(*args, None, 0, C.byref(n)))
        if cap == 0:
            return n.value
        cap = n.value
    arr = (RectItem * max(1, int(cap)))()
    check(lib().srcnn_y_path_delta_rects(*args, C.cast(arr, C.c_void_p), int(cap), C.byref(n)))
    return [(arr[k].x0, arr[k].y0, arr[k].rw, arr[k].rh, arr[k].d_out, arr[k].out_pitch) for k in range(n.value)]


def y_path_delta_dev(prev, prev_pitch, cur, cur_pitch, w, h, dw, dh, filt, tile, out, out_pitch, stream=None, stats=True, struct_size=None):
    """srcnn_y_path_delta_f32_dev on device memory, as given: repaints inside the full-size plane `out` what can differ between
    prev (None = no previous frame) and cur.  Blocks until the flags have arrived; the upscale is asynchronous on `stream`.
    Returns the DeltaStats (None with stats=False)."""
    handle = stream.handle if isinstance(stream, Stream) else stream
    st = None
    if stats:
        st = DeltaStats()
        st.struct_size = C.sizeof(DeltaStats) if struct_size is None else int(struct_size)
    check(lib().srcnn_y_path_delta_f32_dev(_addr(prev), int(prev_pitch or 0), _addr(cur), int(cur_pitch or 0), int(w), int(h), int(dw), int(dh),
                                           int(filt), int(tile[0]), int(tile[1]), _addr(out), int(out_pitch or 0), handle,
                                           C.byref(st) if st is not None else None))
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
    offs, total = [], 0
    for (_, _, rw, rh) in rects:
        offs.append(total)
        total += (rw * rh * 4 + 15) & ~15
    dout = DeviceBuffer(max(16, total))
    y_path_rect_list_dev(din, 0, w, h, dw, dh, filt, [(x0, y0, rw, rh, dout.ptr + o, 0) for (x0, y0, rw, rh), o in zip(rects, offs)])
    sync()
    flat = dout.to_numpy(np.uint8, (max(16, total),))
    return [flat[o:o + rw * rh * 4].view(np.float32).reshape(rh, rw).copy() for (_, _, rw, rh), o in zip(rects, offs)]


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
    src = DeviceBuffer.from_numpy(y)
    dst = DeviceBuffer(dw * dh * 4)
    check(lib().srcnn_resample_f32_dev(src.ptr, w, h, dw, dh, filt, dst.ptr, None))
    sync()
    return dst.to_numpy(np.float32, (dh, dw))


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
    win = lib().srcnn_axis_table(filt, dst_len, src_len, None, None, None)
    if win < 0:
        raise SrcnnError(win, lib().srcnn_last_error().decode())
    left = np.zeros(dst_len, np.int32)
    right = np.zeros(dst_len, np.int32)
    w = np.zeros((dst_len, win + 1), np.float64)
    lib().srcnn_axis_table(filt, dst_len, src_len, left.ctypes.data, right.ctypes.data, w.ctypes.data)
    return left, right, w


def output_size(w, h, multiply, stepscale=False):
    ow, oh = C.c_uint(0), C.c_uint(0)
    rc = lib().srcnn_output_size(w, h, float(np.float32(multiply)), 1 if stepscale else 0, C.byref(ow), C.byref(oh))
    if rc != 0:
        raise SrcnnError(rc, "srcnn_output_size")
    return ow.value, oh.value


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


YUV_I420, YUV_NV12 = 0, 1
_YUV_FORMATS = {"i420": YUV_I420, "nv12": YUV_NV12, YUV_I420: YUV_I420, YUV_NV12: YUV_NV12}


def yuv420_sizes(w, h, multiply):
    """((dw, dh), (cw, ch), (dcw, dch)): luma output and chroma input / output sizes of srcnn_yuv420_upscale_dev."""
    dw, dh = output_size(w, h, multiply)
    return (dw, dh), ((w + 1) // 2, (h + 1) // 2), ((dw + 1) // 2, (dh + 1) // 2)


def _addr(p):
    """A plane argument of yuv420_upscale_dev: None, an address, a DeviceBuffer, or (DeviceBuffer | address, byte offset)."""
    if p is None:
        return None
    if isinstance(p, tuple):
        base, off = p
        return _addr(base) + int(off)
    return p.ptr if isinstance(p, DeviceBuffer) else int(p)


def yuv420_upscale_dev(fmt, w, h, multiply, filt, src, src_pitch, dst, dst_pitch, stream=None):
    """srcnn_yuv420_upscale_dev on device memory, as given: src / dst are 3 plane arguments (see _addr; NV12 ignores the
    third), pitches 3 byte counts (0 = tight) or None.  Asynchronous on `stream` (a Stream, a raw handle or None);
    raises SrcnnError with the library's code."""
    vp, sz = C.c_void_p, C.c_size_t
    s = (vp * 3)(*[_addr(p) for p in src])
    d = (vp * 3)(*[_addr(p) for p in dst])
    sp = (sz * 3)(*src_pitch) if src_pitch is not None else None
    dp = (sz * 3)(*dst_pitch) if dst_pitch is not None else None
    handle = stream.handle if isinstance(stream, Stream) else stream
    check(lib().srcnn_yuv420_upscale_dev(int(_YUV_FORMATS.get(fmt, fmt)), int(w), int(h), float(np.float32(multiply)), int(filt), s, sp,
                                         d, dp, handle))


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
    pad = [None] * (3 - len(planes))
    yuv420_upscale_dev(fmt, w, h, multiply, filt, din + pad, None, dout + pad, None, stream)
    if isinstance(stream, Stream):
        stream.sync()
    else:
        check(lib().srcnn_stream_sync(stream))
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


def yuv_plane_sizes(fmt, w, h, multiply):
    """((dw, dh), src_planes, dst_planes): the output size and, per plane of the format (2 for semi-planar, else 3),
    (cols, rows, row_bytes) of the input and of the output frame of srcnn_yuv_upscale_dev."""
    dw, dh = output_size(w, h, multiply)
    n = 2 if fmt.layout == YUV_SEMIPLANAR else 3
    return ((dw, dh), [yuv_plane_size(fmt, w, h, k) for k in range(n)], [yuv_plane_size(fmt, dw, dh, k) for k in range(n)])


def yuv_upscale_dev(fmt, w, h, multiply, filt, src, src_pitch, dst, dst_pitch, stream=None):
    """srcnn_yuv_upscale_dev on device memory, as given: fmt a YuvFormat (yuv_format(...)) or None, src / dst 3 plane
    arguments (see _addr; semi-planar ignores the third), pitches 3 byte counts (0 = tight) or None.  Asynchronous on
    `stream` (a Stream, a raw handle or None); raises SrcnnError with the library's code."""
    vp, sz = C.c_void_p, C.c_size_t
    s = (vp * 3)(*[_addr(p) for p in src]) if src is not None else None
    d = (vp * 3)(*[_addr(p) for p in dst]) if dst is not None else None
    sp = (sz * 3)(*src_pitch) if src_pitch is not None else None
    dp = (sz * 3)(*dst_pitch) if dst_pitch is not None else None
    handle = stream.handle if isinstance(stream, Stream) else stream
    check(lib().srcnn_yuv_upscale_dev(C.byref(fmt) if fmt is not None else None, int(w), int(h), float(np.float32(multiply)),
                                      int(filt), s, sp, d, dp, handle))


def yuv_upscale(planes, layout="planar", chroma="420", depth=8, msb_aligned=False, multiply=2.0, filt=SRCNNF_Bicubic, stream=None):
    """One YUV frame through srcnn_yuv_upscale_dev: numpy planes in, numpy planes out, uint8 at depth 8 and uint16 above.
    planar: (y, u, v) -> (y', u', v'); semi-planar: (y, uv) with uv (rows, 2 * cols) or (rows, cols, 2) -> (y', uv') with
    uv' (rows, 2 * cols)."""
    fmt = yuv_format(layout, chroma, depth, msb_aligned)
    dt = np.uint8 if depth == 8 else np.uint16
    y = np.ascontiguousarray(planes[0], dt)
    h, w = y.shape
    _, src_sizes, dst_sizes = yuv_plane_sizes(fmt, w, h, multiply)
    bps = np.dtype(dt).itemsize
    ins = [y] + [np.ascontiguousarray(p, dt).reshape(r, rb // bps) for p, (_c, r, rb) in zip(planes[1:], src_sizes[1:])]
    assert len(ins) == len(src_sizes), "%d planes given, the format has %d" % (len(ins), len(src_sizes))
    shapes = [(r, rb // bps) for (_c, r, rb) in dst_sizes]
    din = [DeviceBuffer.from_numpy(p) for p in ins]
    dout = [DeviceBuffer(max(1, int(np.prod(s)) * bps)) for s in shapes]
    pad = [None] * (3 - len(ins))
    yuv_upscale_dev(fmt, w, h, multiply, filt, din + pad, None, dout + pad, None, stream)
    if isinstance(stream, Stream):
        stream.sync()
    else:
        check(lib().srcnn_stream_sync(stream))
    return tuple(b.to_numpy(dt, s) for b, s in zip(dout, shapes))


def yuv_rect_source(fmt, w, h, multiply, filt, x0, y0, rw, rh, plane):
    """(sx0, sy0, sw, sh): the rectangle of plane `plane` (0..2) of the w x h source frame, in that plane's own sample
    coordinates (a UV plane: one column per pair), that output rect [x0, x0 + rw) x [y0, y0 + rh) of
    yuv_upscale_dev(fmt, ..., multiply, filt) depends on (srcnn_yuv_rect_source; no device)."""
    r = [C.c_uint(0) for _ in range(4)]
    check(lib().srcnn_yuv_rect_source(C.byref(fmt) if fmt is not None else None, int(w), int(h), float(np.float32(multiply)), int(filt),
                                      int(x0), int(y0), int(rw), int(rh), int(plane), *[C.byref(v) for v in r]))
    return tuple(v.value for v in r)


def yuv_upscale_rect_dev(fmt, w, h, multiply, filt, src, src_pitch, x0, y0, rw, rh, dst, dst_pitch, stream=None):
    """srcnn_yuv_upscale_rect_dev on device memory, as given: the arguments of yuv_upscale_dev with the rect (x0, y0, rw, rh) in
    luma output coordinates; src is the whole frame, dst the planes of an rw x rh frame (or the addresses of luma sample
    (x0, y0) and of the chroma sample that covers it inside a full-size frame, with that frame's pitches).  Plane arguments as
    for yuv_upscale_dev: a DeviceBuffer, an address, or (DeviceBuffer, byte offset).  Asynchronous on `stream`; raises
    SrcnnError with the library's code."""
    vp, sz = C.c_void_p, C.c_size_t
    s = (vp * 3)(*[_addr(p) for p in src]) if src is not None else None
    d = (vp * 3)(*[_addr(p) for p in dst]) if dst is not None else None
    sp = (sz * 3)(*src_pitch) if src_pitch is not None else None
    dp = (sz * 3)(*dst_pitch) if dst_pitch is not None else None
    handle = stream.handle if isinstance(stream, Stream) else stream
    check(lib().srcnn_yuv_upscale_rect_dev(C.byref(fmt) if fmt is not None else None, int(w), int(h), float(np.float32(multiply)),
                                           int(filt), s, sp, int(x0), int(y0), int(rw), int(rh), d, dp, handle))


def yuv_upscale_rect(planes, rect, layout="planar", chroma="420", depth=8, msb_aligned=False, multiply=2.0, filt=SRCNNF_Bicubic,
                     stream=None):
    """Rect = (x0, y0, rw, rh) (luma output coordinates) of yuv_upscale(planes, ...) through srcnn_yuv_upscale_rect_dev: numpy
    planes of the whole frame in, the planes of the rw x rh rect out (the chroma samples that cover it), shaped as
    yuv_upscale shapes the planes of an rw x rh frame."""
    fmt = yuv_format(layout, chroma, depth, msb_aligned)
    dt = np.uint8 if depth == 8 else np.uint16
    y = np.ascontiguousarray(planes[0], dt)
    h, w = y.shape
    x0, y0, rw, rh = (int(v) for v in rect)
    n = 2 if fmt.layout == YUV_SEMIPLANAR else 3
    src_sizes = [yuv_plane_size(fmt, w, h, k) for k in range(n)]
    bps = np.dtype(dt).itemsize
    ins = [y] + [np.ascontiguousarray(p, dt).reshape(r, rb // bps) for p, (_c, r, rb) in zip(planes[1:], src_sizes[1:])]
    assert len(ins) == n, "%d planes given, the format has %d" % (len(ins), n)
    din = [DeviceBuffer.from_numpy(p) for p in ins]
    pad = [None] * (3 - n)
    if rw <= 0 or rh <= 0:
        shapes, dout = [], [DeviceBuffer(1) for _ in range(n)]        # (for the library to refuse)
    else:
        shapes = [(r, rb // bps) for (_c, r, rb) in (yuv_plane_size(fmt, rw, rh, k) for k in range(n))]
        dout = [DeviceBuffer(max(1, int(np.prod(s)) * bps)) for s in shapes]
    yuv_upscale_rect_dev(fmt, w, h, multiply, filt, din + pad, None, x0, y0, rw, rh, dout + pad, None, stream)
    if isinstance(stream, Stream):
        stream.sync()
    else:
        check(lib().srcnn_stream_sync(stream))
    return tuple(b.to_numpy(dt, s) for b, s in zip(dout, shapes))


(YUVP_YUY2, YUVP_UYVY, YUVP_YVYU, YUVP_Y210, YUVP_Y212, YUVP_Y216, YUVP_VUYA, YUVP_Y410, YUVP_Y416, YUVP_V210) = range(10)
_YUVP_FORMATS = {"yuy2": YUVP_YUY2, "uyvy": YUVP_UYVY, "yvyu": YUVP_YVYU, "y210": YUVP_Y210, "y212": YUVP_Y212, "y216": YUVP_Y216,
                 "vuya": YUVP_VUYA, "ayuv": YUVP_VUYA, "y410": YUVP_Y410, "y416": YUVP_Y416, "v210": YUVP_V210}


def _yuvp_format(fmt):
    return int(_YUVP_FORMATS.get(fmt.lower(), -1) if isinstance(fmt, str) else fmt)


def yuv_packed_row_bytes(fmt, w):
    """(tight row bytes, alignment of base and pitch) of a w-pixel row of a packed format: a YUVP_* value or its name
    ("yuy2", "v210" ...; srcnn_yuv_packed_row_bytes; no device)."""
    rb, al = C.c_size_t(0), C.c_uint(0)
    check(lib().srcnn_yuv_packed_row_bytes(_yuvp_format(fmt), int(w), C.byref(rb), C.byref(al)))
    return rb.value, al.value


def yuv_packed_upscale_dev(fmt, w, h, multiply, filt, src, src_pitch, dst, dst_pitch, stream=None):
    """srcnn_yuv_packed_upscale_dev on device memory, as given: src / dst one frame argument each (see _addr), pitches in
    bytes (0 = tight).  Asynchronous on `stream` (a Stream, a raw handle or None); raises SrcnnError with the library's code."""
    handle = stream.handle if isinstance(stream, Stream) else stream
    check(lib().srcnn_yuv_packed_upscale_dev(_yuvp_format(fmt), int(w), int(h), float(np.float32(multiply)), int(filt), _addr(src),
                                             int(src_pitch or 0), _addr(dst), int(dst_pitch or 0), handle))


def yuv_packed_upscale(frame, fmt, w, multiply=2.0, filt=SRCNNF_Bicubic, stream=None):
    """One packed YUV frame through srcnn_yuv_packed_upscale_dev: a 2-D uint8 array of h x row_bytes(w) in, one of
    dh x row_bytes(dw) out (tight rows; `w` says how many pixels a row holds)."""
    frame = np.ascontiguousarray(frame, np.uint8)
    rb, _ = yuv_packed_row_bytes(fmt, w)
    if frame.ndim != 2 or frame.shape[1] != rb:
        raise ValueError("a %d-pixel row of this format has %d bytes: the frame is %r" % (w, rb, frame.shape))
    h = frame.shape[0]
    dw, dh = output_size(w, h, multiply)
    drb, _ = yuv_packed_row_bytes(fmt, dw)
    din = DeviceBuffer.from_numpy(frame)
    dout = DeviceBuffer(max(1, dh * drb))
    yuv_packed_upscale_dev(fmt, w, h, multiply, filt, din, 0, dout, 0, stream)
    if isinstance(stream, Stream):
        stream.sync()
    else:
        check(lib().srcnn_stream_sync(stream))
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
    r = [C.c_uint(0) for _ in range(4)]
    check(lib().srcnn_yuv_packed_rect_source(_yuvp_format(fmt), int(w), int(h), float(np.float32(multiply)), int(filt), int(x0), int(y0),
                                             int(rw), int(rh), *[C.byref(v) for v in r]))
    return tuple(v.value for v in r)


def yuv_packed_upscale_rect_dev(fmt, w, h, multiply, filt, src, src_pitch, x0, y0, rw, rh, dst, dst_pitch, stream=None):
    """srcnn_yuv_packed_upscale_rect_dev on device memory, as given: the arguments of yuv_packed_upscale_dev with the rect
    (x0, y0, rw, rh) in luma output coordinates; src is the whole frame, dst the rect's row segments (or the address of the
    rect's first byte inside a full-size frame, with that frame's pitch).  Frame arguments: a DeviceBuffer, an address, or
    (DeviceBuffer, byte offset).  Asynchronous on `stream`; raises SrcnnError with the library's code."""
    handle = stream.handle if isinstance(stream, Stream) else stream
    check(lib().srcnn_yuv_packed_upscale_rect_dev(_yuvp_format(fmt), int(w), int(h), float(np.float32(multiply)), int(filt), _addr(src),
                                                  int(src_pitch or 0), int(x0), int(y0), int(rw), int(rh), _addr(dst), int(dst_pitch or 0),
                                                  handle))


def yuv_packed_upscale_rect(frame, fmt, w, rect, multiply=2.0, filt=SRCNNF_Bicubic, stream=None):
    """Rect = (x0, y0, rw, rh) (luma output coordinates, under the format's unit rule) of yuv_packed_upscale(frame, fmt, w, ...)
    through srcnn_yuv_packed_upscale_rect_dev: the whole packed frame in, the (rh, bytes) uint8 array of the rect's row segments
    out, bytes as yuv_packed_span_bytes(fmt, dw, x0, rw) gives them."""
    frame = np.ascontiguousarray(frame, np.uint8)
    rb, _ = yuv_packed_row_bytes(fmt, w)
    if frame.ndim != 2 or frame.shape[1] != rb:
        raise ValueError("a %d-pixel row of this format has %d bytes: the frame is %r" % (w, rb, frame.shape))
    h = frame.shape[0]
    x0, y0, rw, rh = (int(v) for v in rect)
    din = DeviceBuffer.from_numpy(frame)
    nb = 0
    if rw > 0 and rh > 0:
        dw, _dh = output_size(w, h, multiply)
        try:
            _unit, _off, nb = yuv_packed_span_bytes(fmt, dw, x0, rw)
        except SrcnnError:
            nb = 0                           # (for the call below to refuse, with its own message)
    dout = DeviceBuffer(max(1, rh * nb))
    yuv_packed_upscale_rect_dev(fmt, w, h, multiply, filt, din, 0, x0, y0, rw, rh, dout, 0, stream)
    if isinstance(stream, Stream):
        stream.sync()
    else:
        check(lib().srcnn_stream_sync(stream))
    return dout.to_numpy(np.uint8, (rh, nb))


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


def rgb_upscale_dev(fmt, w, h, multiply, filt, src, src_pitch, dst, dst_pitch, dst_conv=None, dst_conv_pitch=0, stream=None):
    """srcnn_rgb_upscale_dev on device memory, as given: fmt an RgbFormat (rgb_format(...)) or None, src / dst up to 4 plane
    arguments (see _addr; interleaved uses the first only), pitches byte counts (0 = tight) or None, dst_conv a plane
    argument for the truncated Y' or None.  Asynchronous on `stream` (a Stream, a raw handle or None); raises SrcnnError with
    the library's code."""
    vp, sz = C.c_void_p, C.c_size_t
    four = lambda xs, fill: list(xs) + [fill] * (4 - len(xs))   # noqa: E731
    s = (vp * 4)(*[_addr(p) for p in four(src, None)]) if src is not None else None
    d = (vp * 4)(*[_addr(p) for p in four(dst, None)]) if dst is not None else None
    sp = (sz * 4)(*four(src_pitch, 0)) if src_pitch is not None else None
    dp = (sz * 4)(*four(dst_pitch, 0)) if dst_pitch is not None else None
    handle = stream.handle if isinstance(stream, Stream) else stream
    check(lib().srcnn_rgb_upscale_dev(C.byref(fmt) if fmt is not None else None, int(w), int(h), float(np.float32(multiply)),
                                      int(filt), s, sp, d, dp, _addr(dst_conv), int(dst_conv_pitch), handle))


def rgb_upscale(image, multiply=2.0, filt=SRCNNF_Bicubic, layout=None, order="rgb", depth=None, want_conv=False, stream=None):
    """One RGB(A) image through srcnn_rgb_upscale_dev: numpy in, numpy out, uint8 at depth 8 and uint16 above.  image is
    (h, w, c) (interleaved) or (c, h, w) (planar) with c = 3 or 4; layout = "interleaved" / "planar" decides where both fit
    (default: interleaved when the last axis is 3 or 4).  depth defaults to 8 for uint8 and 16 otherwise.
    Returns (out, conv | None) with out shaped like the input."""
    image = np.asarray(image)
    if image.ndim != 3:
        raise ValueError("an RGB(A) image is (h, w, c) or (c, h, w), not %r" % (image.shape,))
    if layout is None:
        layout = "interleaved" if image.shape[2] in (3, 4) else "planar"
    planar = _RGB_LAYOUTS.get(layout.lower() if isinstance(layout, str) else layout, layout) == RGB_PLANAR
    if depth is None:
        depth = 8 if image.dtype == np.uint8 else 16
    dt = np.uint8 if depth == 8 else np.uint16
    image = np.ascontiguousarray(image, dt)
    (c, h, w) = image.shape if planar else (image.shape[2], image.shape[0], image.shape[1])
    if c not in (3, 4):
        raise ValueError("%d channels: an RGB(A) image has 3 or 4" % c)
    fmt = rgb_format(RGB_PLANAR if planar else RGB_INTERLEAVED, order, c == 4, depth)
    dw, dh = output_size(w, h, multiply)
    bps = np.dtype(dt).itemsize
    din = DeviceBuffer.from_numpy(image)
    dout = DeviceBuffer(max(1, dw * dh * c * bps))
    dconv = DeviceBuffer(max(1, dw * dh * bps)) if want_conv else None
    if planar:
        src = [(din, k * w * h * bps) for k in range(c)]
        dst = [(dout, k * dw * dh * bps) for k in range(c)]
    else:
        src, dst = [din], [dout]
    rgb_upscale_dev(fmt, w, h, multiply, filt, src, None, dst, None, dconv, 0, stream)
    if isinstance(stream, Stream):
        stream.sync()
    else:
        check(lib().srcnn_stream_sync(stream))
    out = dout.to_numpy(dt, (c, dh, dw) if planar else (dh, dw, c))
    return out, (dconv.to_numpy(dt, (dh, dw)) if want_conv else None)


def rgb_rect_source(w, h, multiply, filt, x0, y0, rw, rh):
    """(sx0, sy0, sw, sh): the rectangle of the w x h source image that output rect [x0, x0 + rw) x [y0, y0 + rh) of
    rgb_upscale_dev(..., multiply, filt) depends on (srcnn_rgb_rect_source; no device)."""
    r = [C.c_uint(0) for _ in range(4)]
    check(lib().srcnn_rgb_rect_source(int(w), int(h), float(np.float32(multiply)), int(filt), int(x0), int(y0), int(rw), int(rh),
                                      *[C.byref(v) for v in r]))
    return tuple(v.value for v in r)


def rgb_upscale_rect_dev(fmt, w, h, multiply, filt, src, src_pitch, x0, y0, rw, rh, dst, dst_pitch, dst_conv=None, dst_conv_pitch=0,
                         stream=None):
    """srcnn_rgb_upscale_rect_dev on device memory, as given: the arguments of rgb_upscale_dev with the rect (x0, y0, rw, rh)
    in output coordinates; src is the whole image, dst / dst_conv are rw x rh images (or the address of pixel (x0, y0) of a
    full-size image with that image's pitch).  Asynchronous on `stream`; raises SrcnnError with the library's code."""
    vp, sz = C.c_void_p, C.c_size_t
    four = lambda xs, fill: list(xs) + [fill] * (4 - len(xs))   # noqa: E731
    s = (vp * 4)(*[_addr(p) for p in four(src, None)]) if src is not None else None
    d = (vp * 4)(*[_addr(p) for p in four(dst, None)]) if dst is not None else None
    sp = (sz * 4)(*four(src_pitch, 0)) if src_pitch is not None else None
    dp = (sz * 4)(*four(dst_pitch, 0)) if dst_pitch is not None else None
    handle = stream.handle if isinstance(stream, Stream) else stream
    check(lib().srcnn_rgb_upscale_rect_dev(C.byref(fmt) if fmt is not None else None, int(w), int(h), float(np.float32(multiply)),
                                           int(filt), s, sp, int(x0), int(y0), int(rw), int(rh), d, dp, _addr(dst_conv),
                                           int(dst_conv_pitch), handle))


def rgb_upscale_rect(image, rect, multiply=2.0, filt=SRCNNF_Bicubic, layout=None, order="rgb", depth=None, want_conv=False,
                     stream=None):
    """Pixels rect = (x0, y0, rw, rh) of rgb_upscale(image, ...) through srcnn_rgb_upscale_rect_dev: numpy in, numpy out.
    Returns (out, conv | None), out shaped (rh, rw, c) or (c, rh, rw) like the input."""
    image = np.asarray(image)
    if image.ndim != 3:
        raise ValueError("an RGB(A) image is (h, w, c) or (c, h, w), not %r" % (image.shape,))
    if layout is None:
        layout = "interleaved" if image.shape[2] in (3, 4) else "planar"
    planar = _RGB_LAYOUTS.get(layout.lower() if isinstance(layout, str) else layout, layout) == RGB_PLANAR
    if depth is None:
        depth = 8 if image.dtype == np.uint8 else 16
    dt = np.uint8 if depth == 8 else np.uint16
    image = np.ascontiguousarray(image, dt)
    (c, h, w) = image.shape if planar else (image.shape[2], image.shape[0], image.shape[1])
    if c not in (3, 4):
        raise ValueError("%d channels: an RGB(A) image has 3 or 4" % c)
    x0, y0, rw, rh = (int(v) for v in rect)
    fmt = rgb_format(RGB_PLANAR if planar else RGB_INTERLEAVED, order, c == 4, depth)
    bps = np.dtype(dt).itemsize
    din = DeviceBuffer.from_numpy(image)
    dout = DeviceBuffer(max(1, rw * rh * c * bps))
    dconv = DeviceBuffer(max(1, rw * rh * bps)) if want_conv else None
    if planar:
        src = [(din, k * w * h * bps) for k in range(c)]
        dst = [(dout, k * rw * rh * bps) for k in range(c)]
    else:
        src, dst = [din], [dout]
    rgb_upscale_rect_dev(fmt, w, h, multiply, filt, src, None, x0, y0, rw, rh, dst, None, dconv, 0, stream)
    if isinstance(stream, Stream):
        stream.sync()
    else:
        check(lib().srcnn_stream_sync(stream))
    out = dout.to_numpy(dt, (c, rh, rw) if planar else (rh, rw, c))
    return out, (dconv.to_numpy(dt, (rh, rw)) if want_conv else None)


def rgb_rect_items(items):
    """A ctypes array of srcnn_rgb_rect_item from (x0, y0, rw, rh[, dst[, dst_pitch[, dst_conv[, dst_conv_pitch]]]]) tuples, or
    `items` itself when it already is such an array.  dst: up to 4 plane arguments (each a DeviceBuffer, a (DeviceBuffer, byte
    offset) pair or an address; interleaved uses the first only), dst_pitch: up to 4 byte counts or None (tight), dst_conv: a
    plane argument or None.  Returns (array or None, n)."""
    if isinstance(items, C.Array):
        return items, len(items)
    items = list(items)
    if not items:
        return None, 0
    arr = (RgbRectItem * len(items))()
    for k, it in enumerate(items):
        it = tuple(it)
        arr[k].x0, arr[k].y0, arr[k].rw, arr[k].rh = (int(v) for v in it[:4])
        for p, plane in enumerate(it[4] if len(it) > 4 and it[4] is not None else ()):
            arr[k].dst[p] = _addr(plane)
        for p, pitch in enumerate(it[5] if len(it) > 5 and it[5] is not None else ()):
            arr[k].dst_pitch[p] = int(pitch or 0)
        arr[k].dst_conv = _addr(it[6]) if len(it) > 6 else None
        arr[k].dst_conv_pitch = int(it[7] or 0) if len(it) > 7 else 0
    return arr, len(items)


def rgb_upscale_rect_list_plan(fmt, w, h, multiply, filt, items, n=None, item_size=None, struct_size=None):
    """srcnn_rgb_upscale_rect_list_plan (no device): how the RGB(A) list call routes and packs `items` (see rgb_rect_items) at
    the current mode, workspace limit and switches.  Returns the RectListPlan.  n / item_size / struct_size override what is
    passed (tests)."""
    arr, count = rgb_rect_items(items) if items is not None else (None, 0)
    plan = RectListPlan()
    plan.struct_size = C.sizeof(RectListPlan) if struct_size is None else int(struct_size)
    check(lib().srcnn_rgb_upscale_rect_list_plan(C.byref(fmt) if fmt is not None else None, int(w), int(h), float(np.float32(multiply)), int(filt),
                                                 C.cast(arr, C.c_void_p) if arr is not None else None, count if n is None else int(n),
                                                 C.sizeof(RgbRectItem) if item_size is None else int(item_size), C.byref(plan)))
    return plan


def rgb_upscale_rect_list_dev(fmt, w, h, multiply, filt, src, src_pitch, items, stream=None, n=None, item_size=None):
    """srcnn_rgb_upscale_rect_list_dev on device memory, as given: fmt, src and src_pitch as for rgb_upscale_rect_dev (the whole
    image), items the rects with their destinations (see rgb_rect_items).  Asynchronous on `stream` (a Stream, a raw handle or
    None); the item array is read before the call returns.  Raises SrcnnError with the library's code."""
    vp, sz = C.c_void_p, C.c_size_t
    four = lambda xs, fill: list(xs) + [fill] * (4 - len(xs))   # noqa: E731
    s = (vp * 4)(*[_addr(p) for p in four(src, None)]) if src is not None else None
    sp = (sz * 4)(*four(src_pitch, 0)) if src_pitch is not None else None
    handle = stream.handle if isinstance(stream, Stream) else stream
    arr, count = rgb_rect_items(items) if items is not None else (None, 0)
    check(lib().srcnn_rgb_upscale_rect_list_dev(C.byref(fmt) if fmt is not None else None, int(w), int(h), float(np.float32(multiply)), int(filt),
                                                s, sp, C.cast(arr, C.c_void_p) if arr is not None else None, count if n is None else int(n),
                                                C.sizeof(RgbRectItem) if item_size is None else int(item_size), handle))


def rgb_upscale_rects(image, rects, multiply=2.0, filt=SRCNNF_Bicubic, layout=None, order="rgb", depth=None, want_conv=False):
    """Pixels (x0, y0, rw, rh) of rgb_upscale(image, ...) for every rect of `rects`, through ONE srcnn_rgb_upscale_rect_list_dev
    call: numpy in, a list of numpy arrays out -- each shaped (rh, rw, c) or (c, rh, rw) like the input -- or, with want_conv,
    a list of (out, conv) pairs."""
    image = np.asarray(image)
    if image.ndim != 3:
        raise ValueError("an RGB(A) image is (h, w, c) or (c, h, w), not %r" % (image.shape,))
    if layout is None:
        layout = "interleaved" if image.shape[2] in (3, 4) else "planar"
    planar = _RGB_LAYOUTS.get(layout.lower() if isinstance(layout, str) else layout, layout) == RGB_PLANAR
    if depth is None:
        depth = 8 if image.dtype == np.uint8 else 16
    dt = np.uint8 if depth == 8 else np.uint16
    image = np.ascontiguousarray(image, dt)
    (c, h, w) = image.shape if planar else (image.shape[2], image.shape[0], image.shape[1])
    if c not in (3, 4):
        raise ValueError("%d channels: an RGB(A) image has 3 or 4" % c)
    rects = [tuple(int(v) for v in r) for r in rects]
    if not rects:
        return []
    fmt = rgb_format(RGB_PLANAR if planar else RGB_INTERLEAVED, order, c == 4, depth)
    bps = np.dtype(dt).itemsize
    din = DeviceBuffer.from_numpy(image)
    offs, total = [], 0
    for (_, _, rw, rh) in rects:                  # per item: the image, then the conv plane, each from a 16-byte boundary
        o_img = total
        total += (rw * rh * c * bps + 15) & ~15
        o_conv = total
        total += ((rw * rh * bps + 15) & ~15) if want_conv else 0
        offs.append((o_img, o_conv))
    dout = DeviceBuffer(max(16, total))
    items = []
    for (x0, y0, rw, rh), (o_img, o_conv) in zip(rects, offs):
        dst = [(dout, o_img + k * rw * rh * bps) for k in range(c)] if planar else [(dout, o_img)]
        items.append((x0, y0, rw, rh, dst, None, (dout, o_conv) if want_conv else None, 0))
    src = [(din, k * w * h * bps) for k in range(c)] if planar else [din]
    rgb_upscale_rect_list_dev(fmt, w, h, multiply, filt, src, None, items)
    sync()
    flat = dout.to_numpy(np.uint8, (max(16, total),))
    res = []
    for (_, _, rw, rh), (o_img, o_conv) in zip(rects, offs):
        out = flat[o_img:o_img + rw * rh * c * bps].view(dt).reshape((c, rh, rw) if planar else (rh, rw, c)).copy()
        res.append((out, flat[o_conv:o_conv + rw * rh * bps].view(dt).reshape(rh, rw).copy()) if want_conv else out)
    return res


def _four(xs, kind, fill):
    """A ctypes array of 4 plane arguments (kind c_void_p, see _addr) or pitches (kind c_size_t), or None for None."""
    if xs is None:
        return None
    xs = list(xs) + [fill] * (4 - len(xs))
    return (kind * 4)(*[(_addr(x) if kind is C.c_void_p else int(x or 0)) for x in xs])


def rgb_delta_grid(w, h, multiply, filt, tile=(0, 0)):
    """(dw, dh, cols, rows): the output size and the tile grid of the RGB(A) delta call (srcnn_rgb_delta_grid; no device).
    tile: (tile_w, tile_h), 0 = the default 64."""
    r = [C.c_uint(0) for _ in range(4)]
    check(lib().srcnn_rgb_delta_grid(int(w), int(h), float(np.float32(multiply)), int(filt), int(tile[0]), int(tile[1]), *[C.byref(v) for v in r]))
    return tuple(v.value for v in r)


def rgb_delta_flags_dev(fmt, w, h, multiply, filt, prev, prev_pitch, cur, cur_pitch, tile, flags, stream=None):
    """srcnn_rgb_delta_flags_dev on device memory, as given: prev (None = no previous image) / cur are up to 4 plane arguments of
    whole source images (see _addr), pitches byte counts or None (tight), flags receives cols x rows bytes.  Asynchronous on
    `stream`."""
    handle = stream.handle if isinstance(stream, Stream) else stream
    check(lib().srcnn_rgb_delta_flags_dev(C.byref(fmt) if fmt is not None else None, int(w), int(h), float(np.float32(multiply)), int(filt),
                                          _four(prev, C.c_void_p, None), _four(prev_pitch, C.c_size_t, 0), _four(cur, C.c_void_p, None),
                                          _four(cur_pitch, C.c_size_t, 0), int(tile[0]), int(tile[1]), _addr(flags), handle))


def rgb_delta_rects(flags, tile, fmt, dw, dh, dst=None, dst_pitch=None, dst_conv=None, dst_conv_pitch=0, cap=None, item_size=None):
    """srcnn_rgb_delta_rects (pure host): the coalescer over a (rows, cols) uint8 array of flags of tile[0] x tile[1] tiles, as
    items that point into the full-size image dst / dst_conv (plane arguments, or None).  Returns
    [(x0, y0, rw, rh, [dst 0..3], [dst_pitch 0..3], dst_conv, dst_conv_pitch)].  cap: None = as many items as needed; 0 = count
    only (returns the number); anything else is the capacity handed to the call (tests)."""
    flags = np.ascontiguousarray(flags, np.uint8)
    rows, cols = flags.shape
    n = C.c_uint(0)
    size = C.sizeof(RgbRectItem) if item_size is None else int(item_size)
    args = (flags.ctypes.data, cols, rows, int(tile[0]), int(tile[1]), C.byref(fmt) if fmt is not None else None, int(dw), int(dh),
            _four(dst, C.c_void_p, None), _four(dst_pitch, C.c_size_t, 0), _addr(dst_conv), int(dst_conv_pitch or 0))
    if cap is None or cap == 0:
        check(lib().srcnn_rgb_delta_rects(*args, None, 0, size, C.byref(n)))
        if cap == 0:
            return n.value
        cap = n.value
    arr = (RgbRectItem * max(1, int(cap)))()
    check(lib().srcnn_rgb_delta_rects(*args, C.cast(arr, C.c_void_p), int(cap), size, C.byref(n)))
    return [(a.x0, a.y0, a.rw, a.rh, list(a.dst), list(a.dst_pitch), a.dst_conv, a.dst_conv_pitch) for a in arr[:n.value]]


def rgb_upscale_delta_dev(fmt, w, h, multiply, filt, prev, prev_pitch, cur, cur_pitch, tile, dst, dst_pitch, dst_conv=None, dst_conv_pitch=0,
                          stream=None, stats=True, struct_size=None):
    """srcnn_rgb_upscale_delta_dev on device memory, as given: repaints inside the full-size image dst (and dst_conv) what can
    differ between prev (None = no previous image) and cur.  Blocks until the flags have arrived; the upscale is asynchronous on
    `stream`.  Returns the DeltaStats (None with stats=False)."""
    handle = stream.handle if isinstance(stream, Stream) else stream
    st = None
    if stats:
        st = DeltaStats()
        st.struct_size = C.sizeof(DeltaStats) if struct_size is None else int(struct_size)
    check(lib().srcnn_rgb_upscale_delta_dev(C.byref(fmt) if fmt is not None else None, int(w), int(h), float(np.float32(multiply)), int(filt),
                                            _four(prev, C.c_void_p, None), _four(prev_pitch, C.c_size_t, 0), _four(cur, C.c_void_p, None),
                                            _four(cur_pitch, C.c_size_t, 0), int(tile[0]), int(tile[1]), _four(dst, C.c_void_p, None),
                                            _four(dst_pitch, C.c_size_t, 0), _addr(dst_conv), int(dst_conv_pitch or 0), handle,
                                            C.byref(st) if st is not None else None))
    return st


def rgb_upscale_delta(prev, cur, out, multiply=2.0, filt=SRCNNF_Bicubic, layout=None, order="rgb", depth=None, tile=(0, 0), conv=None):
    """numpy convenience over srcnn_rgb_upscale_delta_dev: `out` (rgb_upscale of `prev`; prev None = anything) is updated to
    rgb_upscale of `cur`, and so is `conv` (the truncated Y' plane) when given.  Images as for rgb_upscale.  Returns
    (out, stats), or (out, conv, stats) with conv -- new arrays; what the call did not repaint is copied from `out` / `conv`."""
    image = np.asarray(cur)
    if image.ndim != 3:
        raise ValueError("an RGB(A) image is (h, w, c) or (c, h, w), not %r" % (image.shape,))
    if layout is None:
        layout = "interleaved" if image.shape[2] in (3, 4) else "planar"
    planar = _RGB_LAYOUTS.get(layout.lower() if isinstance(layout, str) else layout, layout) == RGB_PLANAR
    if depth is None:
        depth = 8 if image.dtype == np.uint8 else 16
    dt = np.uint8 if depth == 8 else np.uint16
    image = np.ascontiguousarray(image, dt)
    (c, h, w) = image.shape if planar else (image.shape[2], image.shape[0], image.shape[1])
    if c not in (3, 4):
        raise ValueError("%d channels: an RGB(A) image has 3 or 4" % c)
    dw, dh = output_size(w, h, multiply)
    o = np.ascontiguousarray(out, dt)
    if o.shape != ((c, dh, dw) if planar else (dh, dw, c)):
        raise ValueError("out is %r, the output image %r" % (o.shape, (c, dh, dw) if planar else (dh, dw, c)))
    if prev is not None and np.asarray(prev).shape != image.shape:
        raise ValueError("prev is %r, cur %r" % (np.asarray(prev).shape, image.shape))
    fmt = rgb_format(RGB_PLANAR if planar else RGB_INTERLEAVED, order, c == 4, depth)
    bps = np.dtype(dt).itemsize
    planes = lambda buf, pw, ph: [(buf, k * pw * ph * bps) for k in range(c)] if planar else [buf]   # noqa: E731
    dprev = DeviceBuffer.from_numpy(np.ascontiguousarray(prev, dt)) if prev is not None else None
    dcur = DeviceBuffer.from_numpy(image)
    dout = DeviceBuffer.from_numpy(o)
    dconv = DeviceBuffer.from_numpy(np.ascontiguousarray(conv, dt).reshape(dh, dw)) if conv is not None else None
    st = rgb_upscale_delta_dev(fmt, w, h, multiply, filt, planes(dprev, w, h) if dprev is not None else None, None, planes(dcur, w, h), None,
                               tile, planes(dout, dw, dh), None, dconv, 0)
    sync()
    res = dout.to_numpy(dt, o.shape)
    return (res, dconv.to_numpy(dt, (dh, dw)), st) if conv is not None else (res, st)


def yuv_rect_items(items):
    """A ctypes array of srcnn_yuv_rect_item from (x0, y0, rw, rh[, dst[, dst_pitch]]) tuples, or `items` itself when it already
    is such an array.  dst: up to 3 plane arguments (each a DeviceBuffer, a (DeviceBuffer, byte offset) pair or an address;
    semi-planar uses the first two), dst_pitch: up to 3 byte counts or None (tight).  Returns (array or None, n)."""
    if isinstance(items, C.Array):
        return items, len(items)
    items = list(items)
    if not items:
        return None, 0
    arr = (YuvRectItem * len(items))()
    for k, it in enumerate(items):
        it = tuple(it)
        arr[k].x0, arr[k].y0, arr[k].rw, arr[k].rh = (int(v) for v in it[:4])
        for p, plane in enumerate(it[4] if len(it) > 4 and it[4] is not None else ()):
            arr[k].dst[p] = _addr(plane)
        for p, pitch in enumerate(it[5] if len(it) > 5 and it[5] is not None else ()):
            arr[k].dst_pitch[p] = int(pitch or 0)
    return arr, len(items)


def yuv_upscale_rect_list_plan(fmt, w, h, multiply, filt, items, n=None, item_size=None, struct_size=None):
    """srcnn_yuv_upscale_rect_list_plan (no device): how the YUV list call routes and packs `items` (see yuv_rect_items) at the
    current mode, workspace limit and switches.  Returns the RectListPlan.  n / item_size / struct_size override what is passed
    (tests)."""
    arr, count = yuv_rect_items(items) if items is not None else (None, 0)
    plan = RectListPlan()
    plan.struct_size = C.sizeof(RectListPlan) if struct_size is None else int(struct_size)
    check(lib().srcnn_yuv_upscale_rect_list_plan(C.byref(fmt) if fmt is not None else None, int(w), int(h), float(np.float32(multiply)), int(filt),
                                                 C.cast(arr, C.c_void_p) if arr is not None else None, count if n is None else int(n),
                                                 C.sizeof(YuvRectItem) if item_size is None else int(item_size), C.byref(plan)))
    return plan


def yuv_upscale_rect_list_dev(fmt, w, h, multiply, filt, src, src_pitch, items, stream=None, n=None, item_size=None):
    """srcnn_yuv_upscale_rect_list_dev on device memory, as given: fmt, src and src_pitch as for yuv_upscale_rect_dev (the whole
    frame), items the rects with their destinations (see yuv_rect_items).  Asynchronous on `stream` (a Stream, a raw handle or
    None); the item array is read before the call returns.  Raises SrcnnError with the library's code."""
    vp, sz = C.c_void_p, C.c_size_t
    three = lambda xs, fill: list(xs) + [fill] * (3 - len(xs))   # noqa: E731
    s = (vp * 3)(*[_addr(p) for p in three(src, None)]) if src is not None else None
    sp = (sz * 3)(*three(src_pitch, 0)) if src_pitch is not None else None
    handle = stream.handle if isinstance(stream, Stream) else stream
    arr, count = yuv_rect_items(items) if items is not None else (None, 0)
    check(lib().srcnn_yuv_upscale_rect_list_dev(C.byref(fmt) if fmt is not None else None, int(w), int(h), float(np.float32(multiply)), int(filt),
                                                s, sp, C.cast(arr, C.c_void_p) if arr is not None else None, count if n is None else int(n),
                                                C.sizeof(YuvRectItem) if item_size is None else int(item_size), handle))


def yuv_upscale_rects(planes, rects, layout="planar", chroma="420", depth=8, msb_aligned=False, multiply=2.0, filt=SRCNNF_Bicubic):
    """The planes of yuv_upscale_rect(planes, rect, ...) for every rect (x0, y0, rw, rh) of `rects`, through ONE
    srcnn_yuv_upscale_rect_list_dev call: numpy planes of the whole frame in, a list of (Y', U', V') tuples out -- (Y', UV') for a
    semi-planar format -- each shaped as yuv_upscale shapes the planes of an rw x rh frame."""
    rects = [tuple(int(v) for v in r) for r in rects]
    if not rects:
        return []
    fmt = yuv_format(layout, chroma, depth, msb_aligned)
    dt = np.uint8 if depth == 8 else np.uint16
    y = np.ascontiguousarray(planes[0], dt)
    h, w = y.shape
    n = 2 if fmt.layout == YUV_SEMIPLANAR else 3
    src_sizes = [yuv_plane_size(fmt, w, h, k) for k in range(n)]
    bps = np.dtype(dt).itemsize
    ins = [y] + [np.ascontiguousarray(p, dt).reshape(r, rb // bps) for p, (_c, r, rb) in zip(planes[1:], src_sizes[1:])]
    assert len(ins) == n, "%d planes given, the format has %d" % (len(ins), n)
    din = [DeviceBuffer.from_numpy(p) for p in ins]
    layouts, total = [], 0                       # per item and plane: (byte offset, shape), each plane from a 16-byte boundary
    for (_, _, rw, rh) in rects:
        one = []
        for k in range(n):
            if rw <= 0 or rh <= 0:
                one.append((total, (0, 0)))      # (for the library to refuse)
                continue
            _c, r, rb = yuv_plane_size(fmt, rw, rh, k)
            one.append((total, (r, rb // bps)))
            total += (r * rb + 15) & ~15
        layouts.append(one)
    dout = DeviceBuffer(max(16, total))
    items = [(x0, y0, rw, rh, [(dout, o) for o, _ in one], None) for (x0, y0, rw, rh), one in zip(rects, layouts)]
    yuv_upscale_rect_list_dev(fmt, w, h, multiply, filt, din, None, items)
    sync()
    flat = dout.to_numpy(np.uint8, (max(16, total),))
    return [tuple(flat[o:o + sh[0] * sh[1] * bps].view(dt).reshape(sh).copy() for o, sh in one) for one in layouts]


def yuv_packed_rect_items(items):
    """A ctypes array of srcnn_yuv_packed_rect_item from (x0, y0, rw, rh[, dst[, dst_pitch]]) tuples, or `items` itself when it
    already is such an array.  dst: a DeviceBuffer, a (DeviceBuffer, byte offset) pair or an address; dst_pitch: bytes or None
    (tight).  Returns (array or None, n)."""
    if isinstance(items, C.Array):
        return items, len(items)
    items = list(items)
    if not items:
        return None, 0
    arr = (YuvPackedRectItem * len(items))()
    for k, it in enumerate(items):
        it = tuple(it)
        arr[k].x0, arr[k].y0, arr[k].rw, arr[k].rh = (int(v) for v in it[:4])
        if len(it) > 4 and it[4] is not None:
            arr[k].dst = _addr(it[4])
        arr[k].dst_pitch = int(it[5] or 0) if len(it) > 5 else 0
    return arr, len(items)


def yuv_packed_upscale_rect_list_plan(fmt, w, h, multiply, filt, items, n=None, item_size=None, struct_size=None):
    """srcnn_yuv_packed_upscale_rect_list_plan (no device): how the packed YUV list call routes and packs `items` (see
    yuv_packed_rect_items) at the current mode, workspace limit and switches.  Returns the RectListPlan.  n / item_size /
    struct_size override what is passed (tests)."""
    arr, count = yuv_packed_rect_items(items) if items is not None else (None, 0)
    plan = RectListPlan()
    plan.struct_size = C.sizeof(RectListPlan) if struct_size is None else int(struct_size)
    check(lib().srcnn_yuv_packed_upscale_rect_list_plan(_yuvp_format(fmt), int(w), int(h), float(np.float32(multiply)), int(filt),
                                                        C.cast(arr, C.c_void_p) if arr is not None else None, count if n is None else int(n),
                                                        C.sizeof(YuvPackedRectItem) if item_size is None else int(item_size), C.byref(plan)))
    return plan


def yuv_packed_upscale_rect_list_dev(fmt, w, h, multiply, filt, src, src_pitch, items, stream=None, n=None, item_size=None):
    """srcnn_yuv_packed_upscale_rect_list_dev on device memory, as given: fmt, src and src_pitch as for
    yuv_packed_upscale_rect_dev (the whole frame), items the rects with their destinations (see yuv_packed_rect_items).
    Asynchronous on `stream` (a Stream, a raw handle or None); the item array is read before the call returns.  Raises SrcnnError
    with the library's code."""
    handle = stream.handle if isinstance(stream, Stream) else stream
    arr, count = yuv_packed_rect_items(items) if items is not None else (None, 0)
    check(lib().srcnn_yuv_packed_upscale_rect_list_dev(_yuvp_format(fmt), int(w), int(h), float(np.float32(multiply)), int(filt),
                                                       _addr(src) if src is not None else None, int(src_pitch or 0),
                                                       C.cast(arr, C.c_void_p) if arr is not None else None, count if n is None else int(n),
                                                       C.sizeof(YuvPackedRectItem) if item_size is None else int(item_size), handle))


def yuv_packed_upscale_rects(src, name, w, rects, multiply=2.0, filt=SRCNNF_Bicubic):
    """The row segments of yuv_packed_upscale_rect(src, name, w, rect, ...) for every rect (x0, y0, rw, rh) of `rects`, through
    ONE srcnn_yuv_packed_upscale_rect_list_dev call: the whole packed frame in (a (h, row bytes) uint8 array of format `name`), a
    list of (rh, bytes) uint8 arrays out, bytes as yuv_packed_span_bytes(name, dw, x0, rw) gives them."""
    rects = [tuple(int(v) for v in r) for r in rects]
    if not rects:
        return []
    frame = np.ascontiguousarray(src, np.uint8)
    rb, _ = yuv_packed_row_bytes(name, w)
    if frame.ndim != 2 or frame.shape[1] != rb:
        raise ValueError("a %d-pixel row of this format has %d bytes: the frame is %r" % (w, rb, frame.shape))
    h = frame.shape[0]
    dw, _dh = output_size(w, h, multiply)
    din = DeviceBuffer.from_numpy(frame)
    layouts, total = [], 0                       # per item: (byte offset, (rows, bytes)), each from a 16-byte boundary
    for (x0, y0, rw, rh) in rects:
        nb = 0
        if rw > 0 and rh > 0:
            try:
                _unit, _off, nb = yuv_packed_span_bytes(name, dw, x0, rw)
            except SrcnnError:
                nb = 0                           # (for the call below to refuse, with its own message)
        layouts.append((total, (max(rh, 0) if nb else 0, nb)))
        total += (max(rh, 0) * nb + 15) & ~15
    dout = DeviceBuffer(max(16, total))
    items = [(x0, y0, rw, rh, (dout, o), 0) for (x0, y0, rw, rh), (o, _sh) in zip(rects, layouts)]
    yuv_packed_upscale_rect_list_dev(name, w, h, multiply, filt, din, 0, items)
    sync()
    flat = dout.to_numpy(np.uint8, (max(16, total),))
    return [flat[o:o + sh[0] * sh[1]].reshape(sh).copy() for o, sh in layouts]


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


def rgb_upscale_torch(t, multiply=2.0, filt=SRCNNF_Bicubic, want_conv=False, order="rgb", depth=None):
    """srcnn_rgb_upscale_dev on a torch tensor that lives on a GPU: t is torch.uint8 (depth 8) or a 16-bit integer tensor
    (depth 16 unless `depth` says 10 / 12 / 14), shaped (H, W, C) or (C, H, W) with C in (3, 4).  The memory behind it must be
    interleaved pixels (channel stride 1, column stride C) or one plane per channel (column stride 1); rows may be padded --
    the pitch is taken from the strides -- and anything else raises ValueError.  The output tensor (and the truncated Y'
    plane with want_conv) is allocated by torch on the same device, in the same layout; the call is queued on
    torch.cuda.current_stream() and neither copies to the host nor synchronises.  Returns (out, conv | None).
    The tensor's device must be the device of the calling thread's current srcnn context."""
    W, H, Cn, bps, depth, hwc, layout, sh, sc = _rgb_torch_layout(t, depth, "rgb_upscale_torch")
    import torch
    _rgb_torch_context(t)
    dw, dh = output_size(W, H, multiply)
    if layout == RGB_INTERLEAVED:
        out = torch.empty((dh, dw, Cn), dtype=t.dtype, device=t.device)
        src, dst = [t.data_ptr()], [out.data_ptr()]
        result = out if hwc else out.permute(2, 0, 1)
    else:
        out = torch.empty((Cn, dh, dw), dtype=t.dtype, device=t.device)
        src = [t.data_ptr() + k * sc * bps for k in range(Cn)]
        dst = [out.data_ptr() + k * dh * dw * bps for k in range(Cn)]
        result = out.permute(1, 2, 0) if hwc else out
    conv = torch.empty((dh, dw), dtype=t.dtype, device=t.device) if want_conv else None
    stream = torch.cuda.current_stream(t.device).cuda_stream
    rgb_upscale_dev(rgb_format(layout, order, Cn == 4, depth), W, H, multiply, filt, src, [sh * bps] * len(src), dst, None,
                    conv.data_ptr() if want_conv else None, 0, stream or None)
    return result, conv


def _rgb_torch_layout(t, depth, who):
    """What the RGB(A) torch calls read off a tensor: (W, H, C, bytes per sample, depth, channels-last shape?, SRCNN_RGB_* layout,
    row stride, channel stride), strides in samples; ValueError for anything that is not an RGB(A) image in GPU memory."""
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
    lay = None
    for hwc in (True, False):            # which axis carries the channels, and what the strides say about the memory
        (H, W, Cn) = tuple(t.shape) if hwc else (t.shape[1], t.shape[2], t.shape[0])
        (sh, sw, sc) = t.stride() if hwc else (t.stride(1), t.stride(2), t.stride(0))
        if Cn not in (3, 4):
            continue
        if sc == 1 and sw == Cn and sh >= W * Cn:
            lay = (hwc, RGB_INTERLEAVED, H, W, Cn, sh, sc)
        elif sw == 1 and sh >= W and sc >= 1:
            lay = (hwc, RGB_PLANAR, H, W, Cn, sh, sc)
        if lay:
            break
    if lay is None:
        raise ValueError("shape %r with strides %r is neither interleaved pixels nor one plane per channel" % (tuple(t.shape), t.stride()))
    hwc, layout, H, W, Cn, sh, sc = lay
    return W, H, Cn, bps, depth, hwc, layout, sh, sc


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


def rgb_upscale_rect_torch(t, rect, multiply=2.0, filt=SRCNNF_Bicubic, want_conv=False, order="rgb", depth=None, out=None):
    """srcnn_rgb_upscale_rect_dev on a torch tensor that lives on a GPU: pixels rect = (x0, y0, rw, rh) of what
    rgb_upscale_torch(t, ...) returns, at the cost of the rect.  t as for rgb_upscale_torch.  out=None: a new tensor of rw x rh
    pixels in t's layout.  out = a full-size dw x dh image tensor of t's dtype, shape order and memory layout (rows may be
    padded): the rect is written in place through its strides, nothing else of it is touched, and the view of the rect is
    returned.  Queued on torch.cuda.current_stream(); returns (rect tensor, conv | None), conv a new rh x rw tensor."""
    W, H, Cn, bps, depth, hwc, layout, sh, sc = _rgb_torch_layout(t, depth, "rgb_upscale_rect_torch")
    import torch
    _rgb_torch_context(t)
    x0, y0, rw, rh = (int(v) for v in rect)
    dw, dh = output_size(W, H, multiply)
    if rw <= 0 or rh <= 0 or x0 < 0 or y0 < 0 or x0 + rw > dw or y0 + rh > dh:
        raise ValueError("rect %r is not inside the %d x %d output" % ((x0, y0, rw, rh), dw, dh))
    src = [t.data_ptr()] if layout == RGB_INTERLEAVED else [t.data_ptr() + k * sc * bps for k in range(Cn)]
    if out is None:
        if layout == RGB_INTERLEAVED:
            buf = torch.empty((rh, rw, Cn), dtype=t.dtype, device=t.device)
            dst, dpitch = [buf.data_ptr()], None
            result = buf if hwc else buf.permute(2, 0, 1)
        else:
            buf = torch.empty((Cn, rh, rw), dtype=t.dtype, device=t.device)
            dst, dpitch = [buf.data_ptr() + k * rh * rw * bps for k in range(Cn)], None
            result = buf.permute(1, 2, 0) if hwc else buf
    else:
        if not isinstance(out, torch.Tensor) or out.device != t.device or out.dtype != t.dtype:
            raise ValueError("out must be a tensor of %s on %s" % (t.dtype, t.device))
        oW, oH, oC, _, _, ohwc, olayout, osh, osc = _rgb_torch_layout(out, depth, "rgb_upscale_rect_torch(out=)")
        if (oW, oH, oC, ohwc, olayout) != (dw, dh, Cn, hwc, layout):
            raise ValueError("out is %d x %d x %d (%s), the output image %d x %d x %d in the layout of t" %
                             (oW, oH, oC, "interleaved" if olayout == RGB_INTERLEAVED else "planar", dw, dh, Cn))
        if layout == RGB_INTERLEAVED:
            dst = [out.data_ptr() + (y0 * osh + x0 * Cn) * bps]
        else:
            dst = [out.data_ptr() + (k * osc + y0 * osh + x0) * bps for k in range(Cn)]
        dpitch = [osh * bps] * len(dst)
        result = out[y0:y0 + rh, x0:x0 + rw, :] if hwc else out[:, y0:y0 + rh, x0:x0 + rw]
    conv = torch.empty((rh, rw), dtype=t.dtype, device=t.device) if want_conv else None
    stream = torch.cuda.current_stream(t.device).cuda_stream
    rgb_upscale_rect_dev(rgb_format(layout, order, Cn == 4, depth), W, H, multiply, filt, src, [sh * bps] * len(src), x0, y0, rw, rh,
                         dst, dpitch, conv.data_ptr() if want_conv else None, 0, stream or None)
    return result, conv


def rgb_upscale_rect_list_torch(t, rects, out, multiply=2.0, filt=SRCNNF_Bicubic, order="rgb", depth=None):
    """srcnn_rgb_upscale_rect_list_dev on torch tensors that live on a GPU: repaints every (x0, y0, rw, rh) of `rects` inside
    `out`, in place and in ONE call.  t as for rgb_upscale_torch; out is a full-size dw x dh image tensor of t's dtype, shape
    order and memory layout (rows may be padded): the rects are written through its strides and nothing else of it is touched.
    Queued on torch.cuda.current_stream(); returns out."""
    W, H, Cn, bps, depth, hwc, layout, sh, sc = _rgb_torch_layout(t, depth, "rgb_upscale_rect_list_torch")
    import torch
    _rgb_torch_context(t)
    dw, dh = output_size(W, H, multiply)
    if not isinstance(out, torch.Tensor) or out.device != t.device or out.dtype != t.dtype:
        raise ValueError("out must be a tensor of %s on %s" % (t.dtype, t.device))
    oW, oH, oC, _, _, ohwc, olayout, osh, osc = _rgb_torch_layout(out, depth, "rgb_upscale_rect_list_torch(out)")
    if (oW, oH, oC, ohwc, olayout) != (dw, dh, Cn, hwc, layout):
        raise ValueError("out is %d x %d x %d (%s), the output image %d x %d x %d in the layout of t" %
                         (oW, oH, oC, "interleaved" if olayout == RGB_INTERLEAVED else "planar", dw, dh, Cn))
    items = []
    for r in rects:
        x0, y0, rw, rh = (int(v) for v in r)
        if rw <= 0 or rh <= 0 or x0 < 0 or y0 < 0 or x0 + rw > dw or y0 + rh > dh:
            raise ValueError("rect %r is not inside the %d x %d output" % ((x0, y0, rw, rh), dw, dh))
        if layout == RGB_INTERLEAVED:
            dst = [out.data_ptr() + (y0 * osh + x0 * Cn) * bps]
        else:
            dst = [out.data_ptr() + (k * osc + y0 * osh + x0) * bps for k in range(Cn)]
        items.append((x0, y0, rw, rh, dst, [osh * bps] * len(dst)))
    src = [t.data_ptr()] if layout == RGB_INTERLEAVED else [t.data_ptr() + k * sc * bps for k in range(Cn)]
    stream = torch.cuda.current_stream(t.device).cuda_stream
    rgb_upscale_rect_list_dev(rgb_format(layout, order, Cn == 4, depth), W, H, multiply, filt, src, [sh * bps] * len(src), items, stream or None)
    return out


def rgb_upscale_delta_torch(prev, cur, out, multiply=2.0, filt=SRCNNF_Bicubic, order="rgb", depth=None, tile=(0, 0)):
    """srcnn_rgb_upscale_delta_dev on torch tensors that live on a GPU: `out`, which holds rgb_upscale_torch(prev, ...), is updated
    in place to rgb_upscale_torch(cur, ...) by repainting only the tiles that can differ.  cur as for rgb_upscale_torch; prev is
    None (no previous image: everything is repainted) or a tensor of cur's shape, dtype, device and memory layout (its row
    padding may differ); out is a full-size dw x dh image tensor of cur's dtype, shape order and memory layout (rows may be
    padded): it is written through its strides and nothing of a clean tile is touched.  The call waits once, for the tile flags,
    on torch.cuda.current_stream(), and queues the repaint there.  Returns the DeltaStats."""
    W, H, Cn, bps, depth, hwc, layout, sh, sc = _rgb_torch_layout(cur, depth, "rgb_upscale_delta_torch")
    import torch
    _rgb_torch_context(cur)
    dw, dh = output_size(W, H, multiply)
    planes = lambda t, chan: [t.data_ptr()] if layout == RGB_INTERLEAVED else [t.data_ptr() + k * chan * bps for k in range(Cn)]   # noqa: E731
    p_src = p_pitch = None
    if prev is not None:
        if not isinstance(prev, torch.Tensor) or prev.device != cur.device or prev.dtype != cur.dtype:
            raise ValueError("prev must be a tensor of %s on %s" % (cur.dtype, cur.device))
        pW, pH, pC, _, _, phwc, playout, psh, psc = _rgb_torch_layout(prev, depth, "rgb_upscale_delta_torch(prev)")
        if (pW, pH, pC, phwc, playout) != (W, H, Cn, hwc, layout):
            raise ValueError("prev is %d x %d x %d, cur %d x %d x %d in another layout or shape order" % (pW, pH, pC, W, H, Cn))
        p_src = planes(prev, psc)
        p_pitch = [psh * bps] * len(p_src)
    if not isinstance(out, torch.Tensor) or out.device != cur.device or out.dtype != cur.dtype:
        raise ValueError("out must be a tensor of %s on %s" % (cur.dtype, cur.device))
    oW, oH, oC, _, _, ohwc, olayout, osh, osc = _rgb_torch_layout(out, depth, "rgb_upscale_delta_torch(out)")
    if (oW, oH, oC, ohwc, olayout) != (dw, dh, Cn, hwc, layout):
        raise ValueError("out is %d x %d x %d (%s), the output image %d x %d x %d in the layout of cur" %
                         (oW, oH, oC, "interleaved" if olayout == RGB_INTERLEAVED else "planar", dw, dh, Cn))
    src, dst = planes(cur, sc), planes(out, osc)
    stream = torch.cuda.current_stream(cur.device).cuda_stream
    return rgb_upscale_delta_dev(rgb_format(layout, order, Cn == 4, depth), W, H, multiply, filt, p_src, p_pitch, src, [sh * bps] * len(src), tile,
                                 dst, [osh * bps] * len(dst), None, 0, stream or None)


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


def debug_settings(markdown=False):
    """The SRCNN_* switches this process runs with (srcnn_debug_settings): text, one line per switch.  No device needed."""
    n = lib().srcnn_debug_settings(None, 0, 1 if markdown else 0)
    buf = C.create_string_buffer(n + 1)
    lib().srcnn_debug_settings(buf, n + 1, 1 if markdown else 0)
    return buf.value.decode()


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
    rc = getattr(L, CXX_SYMBOLS[1])(refbuff.ctypes.data if refbuff is not None else None, w, h, d,
                                    float(np.float32(multiply)), C.byref(out), C.byref(outsz),
                                    C.byref(conv) if want_conv else None, C.byref(convsz) if want_conv else None)
    o = c = None
    if rc == 0:
        o = np.ctypeslib.as_array(C.cast(out, C.POINTER(C.c_ubyte)), (outsz.value,)).copy()
        L.srcnn_delete_array(out)
        if want_conv and conv.value:
            c = np.ctypeslib.as_array(C.cast(conv, C.POINTER(C.c_ubyte)), (convsz.value,)).copy()
            L.srcnn_delete_array(conv)
    return rc, o, c
