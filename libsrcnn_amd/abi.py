"""The ABI table of the binding: the constants and structs of the headers under include/, and ONE table of every C function the
library exports -- (header group, symbol, restype, argtypes).  The *_SYMBOLS lists and the argtypes that declare() assigns are
both read off that table, so a function cannot be listed without a signature (it would be called with ctypes' default int
arguments, and its pointers truncated silently)."""
import ctypes as C

__all__ = ["SRCNNF_Nearest", "SRCNNF_Bilinear", "SRCNNF_Bicubic", "SRCNNF_Lanczos3", "SRCNNF_Bspline", "MODE_STRICT", "MODE_FAST",
           "MODE_FAST_F16", "MODE_RELAXED", "RELAX_L1", "RELAX_L2", "RELAX_L3_X64", "RELAX_L3_F32", "YuvFormat", "RgbFormat", "RectItem",
           "RgbRectItem", "YuvRectItem", "YuvPackedRectItem", "RectListPlan", "DeltaStats", "STABLE_ABI_SYMBOLS", "DEBUG_SYMBOLS",
           "YUV_SYMBOLS", "YUV_EX_SYMBOLS", "RGB_SYMBOLS", "YUV_PACKED_SYMBOLS", "RECT_SYMBOLS", "RGB_RECT_SYMBOLS", "YUV_RECT_SYMBOLS",
           "YUV_PACKED_RECT_SYMBOLS", "RECT_LIST_SYMBOLS", "RGB_RECT_LIST_SYMBOLS", "YUV_RECT_LIST_SYMBOLS",
           "YUV_PACKED_RECT_LIST_SYMBOLS", "DELTA_SYMBOLS", "RGB_DELTA_SYMBOLS", "C_ABI_SYMBOLS", "CXX_SYMBOLS"]

SRCNNF_Nearest, SRCNNF_Bilinear, SRCNNF_Bicubic, SRCNNF_Lanczos3, SRCNNF_Bspline = range(5)
MODE_STRICT, MODE_FAST, MODE_FAST_F16, MODE_RELAXED = 0, 1, 2, 3
RELAX_L1, RELAX_L2, RELAX_L3_X64, RELAX_L3_F32 = 1, 2, 4, 8


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


vp, u, f, sz, i, P = C.c_void_p, C.c_uint, C.c_float, C.c_size_t, C.c_int, C.POINTER
pvp, psz, pu, pi, pd, pull = P(vp), P(sz), P(u), P(i), P(C.c_double), P(C.c_ulonglong)
yfmt, rfmt, plan, stats = P(YuvFormat), P(RgbFormat), P(RectListPlan), P(DeltaStats)

# One block per header, in the order C_ABI_SYMBOLS lists them; rows in the order of the header's committed .abi list.
_BY_HEADER = [
    # The STABLE C ABI: every function include/srcnn_amd.h declares, frozen at ABI 5 (include/srcnn_amd.abi is the committed list;
    # tests/test_abi.py holds header, list, this binding and the library's export table to each other)
    ("stable", [
        ("srcnn_abi_version", i, []), ("srcnn_device_count", i, []), ("srcnn_init", i, [i]), ("srcnn_init_devices", i, [pi, i]),
        ("srcnn_context_count", i, []), ("srcnn_context_device", i, [i]), ("srcnn_set_context", i, [i]), ("srcnn_get_context", i, []),
        ("srcnn_shutdown", None, []), ("srcnn_trim", i, []), ("srcnn_last_error", C.c_char_p, []), ("srcnn_set_mode", i, [i]),
        ("srcnn_get_mode", i, []), ("srcnn_device_name", i, [C.c_char_p, sz]), ("srcnn_set_workspace_limit", sz, [sz]),
        ("srcnn_dev_alloc", vp, [sz]), ("srcnn_dev_free", None, [vp]), ("srcnn_host_alloc_pinned", vp, [sz]),
        ("srcnn_host_free_pinned", None, [vp]), ("srcnn_memcpy_h2d", i, [vp, vp, sz, vp]), ("srcnn_memcpy_d2h", i, [vp, vp, sz, vp]),
        ("srcnn_memset_dev", i, [vp, i, sz, vp]), ("srcnn_stream_create", i, [pvp]), ("srcnn_stream_destroy", i, [vp]),
        ("srcnn_stream_sync", i, [vp]), ("srcnn_device_sync", i, []), ("srcnn_event_create", i, [pvp]), ("srcnn_event_destroy", i, [vp]),
        ("srcnn_event_record", i, [vp, vp]), ("srcnn_stream_wait_event", i, [vp, vp]), ("srcnn_event_elapsed_ms", i, [vp, vp, P(f)]),
        ("srcnn_profile_enable", i, [i]), ("srcnn_profile_reset", i, []), ("srcnn_profile_read", i, [i, pd, pull]),
        ("srcnn_profile_read_context", i, [i, i, pd, pull]), ("srcnn_y_upscale2x_f32_dev", i, [vp, u, u, vp, vp]),
        ("srcnn_y_upscale2x_f32_batch_dev", i, [vp, u, u, u, vp, vp]), ("srcnn_y_upscale2x_f32_band_dev", i, [vp, u, u, u, u, vp, vp]),
        ("srcnn_y_upscale2x_f32_node_dev", i, [vp, u, u, vp, i]), ("srcnn_batch_graph_create", i, [vp, u, u, u, vp, vp, pvp]),
        ("srcnn_batch_graph_launch", i, [vp]), ("srcnn_batch_graph_destroy", i, [vp]), ("srcnn_y_path_f32_dev", i, [vp, u, u, u, u, i, vp, vp]),
        ("srcnn_resample_f32_dev", i, [vp, u, u, u, u, i, vp, vp]), ("srcnn_conv1_f32_dev", i, [vp, u, u, vp, vp]),
        ("srcnn_conv2_f32_dev", i, [vp, u, u, vp, vp]), ("srcnn_conv3_f32_dev", i, [vp, u, u, vp, vp]), ("srcnn_conv12_f32_dev", i, [vp, u, u, vp, vp]),
        ("srcnn_y_upscale2x_f32", i, [vp, u, u, vp]), ("srcnn_y_upscale2x_f32_batch", i, [vp, u, u, u, vp]),
        ("srcnn_y_upscale2x_f32_stream", i, [vp, u, u, u, vp, i]), ("srcnn_y_path_f32", i, [vp, u, u, u, u, i, vp]),
        ("srcnn_process_u8", i, [vp, u, u, u, f, i, vp, vp]), ("srcnn_process_u8_begin", i, [vp, u, u, u, f, i, vp, vp, pvp]),
        ("srcnn_process_u8_wait", i, [vp]), ("srcnn_delete_array", None, [vp]), ("srcnn_output_size", i, [u, u, f, i, pu, pu]),
        ("srcnn_comm_unique_id", i, [vp]), ("srcnn_comm_init", i, [vp, i, i]), ("srcnn_comm_destroy", i, []), ("srcnn_comm_rank", i, [pi, pi]),
        ("srcnn_comm_gather_f32", i, [vp, sz, vp, i, vp]), ("srcnn_comm_gatherv_f32", i, [vp, psz, vp, i, vp]),
        ("srcnn_comm_gatherv_at_f32", i, [vp, psz, psz, vp, i, vp]), ("srcnn_comm_tiled_y_upscale2x_f32_dev", i, [vp, u, u, vp, vp, i, i, vp]),
        ("srcnn_band_rows", i, [u, i, i, pu, pu]), ("srcnn_tiled_piece", i, [u, u, i, i, i, i, pu, pu]),
        ("srcnn_comm_allgather_f32", i, [vp, sz, vp, vp]), ("srcnn_comm_barrier", i, [vp]), ("srcnn_comm_wait", i, [vp]),
        ("srcnn_comm_set_timeout_ms", i, [i])]),
    # instruments (include/srcnn_amd_debug.h): test hooks, diagnostics, the relaxation experiment -- no compatibility promise
    ("debug", [
        ("srcnn_set_relaxation", i, [u]), ("srcnn_axis_table", i, [i, u, u, vp, vp, vp]), ("srcnn_fused_diag", i, [vp, u, u, vp, vp, vp]),
        ("srcnn_debug_counts", i, [pi, pi]), ("srcnn_debug_settings", i, [C.c_char_p, sz, i]), ("srcnn_debug_clock_probe", i, [i]),
        ("srcnn_debug_clock_read", i, [i, vp, vp, i]), ("srcnn_debug_band_plan", i, [u, u, u, i, pu, i]),
        ("srcnn_debug_process_phases", i, [pd, i]), ("srcnn_debug_stream_mode", i, [pu, pu, pi])]),
    # Each extension below has a header include/srcnn_amd_<group>.h, a committed list include/srcnn_amd_<group>.abi and a version of
    # its own.  yuv: the 8-bit YUV 4:2:0 call
    ("yuv", [
        ("srcnn_yuv_abi_version", i, []), ("srcnn_yuv420_upscale_dev", i, [i, u, u, f, i, pvp, psz, pvp, psz, vp])]),
    # high-bit-depth / 4:2:2 / 4:4:4 YUV frames
    ("yuv_ex", [
        ("srcnn_yuv_ex_abi_version", i, []), ("srcnn_yuv_plane_size", i, [yfmt, u, u, i, pu, pu, psz]),
        ("srcnn_yuv_upscale_dev", i, [yfmt, u, u, f, i, pvp, psz, pvp, psz, vp])]),
    # RGB(A) images already in device memory
    ("rgb", [
        ("srcnn_rgb_abi_version", i, []), ("srcnn_rgb_plane_size", i, [rfmt, u, u, i, pu, pu, psz]),
        ("srcnn_rgb_upscale_dev", i, [rfmt, u, u, f, i, pvp, psz, pvp, psz, vp, sz, vp])]),
    # packed YUV frames
    ("yuv_packed", [
        ("srcnn_yuv_packed_abi_version", i, []), ("srcnn_yuv_packed_row_bytes", i, [i, u, psz, pu]),
        ("srcnn_yuv_packed_upscale_dev", i, [i, u, u, f, i, vp, sz, vp, sz, vp])]),
    # one rectangle of the Y path's output
    ("rect", [
        ("srcnn_rect_abi_version", i, []), ("srcnn_y_path_rect_source", i, [u, u, u, u, i, u, u, u, u, pu, pu, pu, pu]),
        ("srcnn_y_path_rect_f32_dev", i, [vp, sz, u, u, u, u, i, u, u, u, u, vp, sz, vp])]),
    # one rectangle of an RGB(A) image
    ("rgb_rect", [
        ("srcnn_rgb_rect_abi_version", i, []), ("srcnn_rgb_rect_source", i, [u, u, f, i, u, u, u, u, pu, pu, pu, pu]),
        ("srcnn_rgb_upscale_rect_dev", i, [rfmt, u, u, f, i, pvp, psz, u, u, u, u, pvp, psz, vp, sz, vp])]),
    # one rectangle of a planar / semi-planar YUV frame
    ("yuv_rect", [
        ("srcnn_yuv_rect_abi_version", i, []), ("srcnn_yuv_rect_source", i, [yfmt, u, u, f, i, u, u, u, u, i, pu, pu, pu, pu]),
        ("srcnn_yuv_upscale_rect_dev", i, [yfmt, u, u, f, i, pvp, psz, u, u, u, u, pvp, psz, vp])]),
    # one rectangle of a packed YUV frame
    ("yuv_packed_rect", [
        ("srcnn_yuv_packed_rect_abi_version", i, []), ("srcnn_yuv_packed_span_bytes", i, [i, u, u, u, pu, psz, psz]),
        ("srcnn_yuv_packed_rect_source", i, [i, u, u, f, i, u, u, u, u, pu, pu, pu, pu]),
        ("srcnn_yuv_packed_upscale_rect_dev", i, [i, u, u, f, i, vp, sz, u, u, u, u, vp, sz, vp])]),
    # a list of rectangles of the Y path's output
    ("rect_list", [
        ("srcnn_rect_list_abi_version", i, []), ("srcnn_y_path_rect_list_plan", i, [u, u, u, u, i, vp, u, u, plan]),
        ("srcnn_y_path_rect_list_f32_dev", i, [vp, sz, u, u, u, u, i, vp, u, u, vp])]),
    # a list of rectangles of an RGB(A) image
    ("rgb_rect_list", [
        ("srcnn_rgb_rect_list_abi_version", i, []), ("srcnn_rgb_upscale_rect_list_plan", i, [rfmt, u, u, f, i, vp, u, u, plan]),
        ("srcnn_rgb_upscale_rect_list_dev", i, [rfmt, u, u, f, i, pvp, psz, vp, u, u, vp])]),
    # a list of rectangles of a planar / semi-planar YUV frame
    ("yuv_rect_list", [
        ("srcnn_yuv_rect_list_abi_version", i, []), ("srcnn_yuv_upscale_rect_list_plan", i, [yfmt, u, u, f, i, vp, u, u, plan]),
        ("srcnn_yuv_upscale_rect_list_dev", i, [yfmt, u, u, f, i, pvp, psz, vp, u, u, vp])]),
    # a list of rectangles of a packed YUV frame
    ("yuv_packed_rect_list", [
        ("srcnn_yuv_packed_rect_list_abi_version", i, []), ("srcnn_yuv_packed_upscale_rect_list_plan", i, [i, u, u, f, i, vp, u, u, plan]),
        ("srcnn_yuv_packed_upscale_rect_list_dev", i, [i, u, u, f, i, vp, sz, vp, u, u, vp])]),
    # only what changed between two Y frames
    ("delta", [
        ("srcnn_delta_abi_version", i, []), ("srcnn_y_path_delta_grid", i, [u, u, u, u, i, u, u, pu, pu]),
        ("srcnn_y_path_delta_flags_dev", i, [vp, sz, vp, sz, u, u, u, u, i, u, u, vp, vp]),
        ("srcnn_y_path_delta_rects", i, [vp, u, u, u, u, u, u, vp, sz, vp, u, pu]),
        ("srcnn_y_path_delta_f32_dev", i, [vp, sz, vp, sz, u, u, u, u, i, u, u, vp, sz, vp, stats])]),
    # only what changed between two RGB(A) images
    ("rgb_delta", [
        ("srcnn_rgb_delta_abi_version", i, []), ("srcnn_rgb_delta_grid", i, [u, u, f, i, u, u, pu, pu, pu, pu]),
        ("srcnn_rgb_delta_flags_dev", i, [rfmt, u, u, f, i, pvp, psz, pvp, psz, u, u, vp, vp]),
        ("srcnn_rgb_delta_rects", i, [vp, u, u, u, u, rfmt, u, u, pvp, psz, vp, sz, vp, u, u, pu]),
        ("srcnn_rgb_upscale_delta_dev", i, [rfmt, u, u, f, i, pvp, psz, pvp, psz, u, u, pvp, psz, vp, sz, vp, stats])]),
]
ABI_TABLE = [(group, symbol, res, args) for group, rows in _BY_HEADER for symbol, res, args in rows]


def _symbols(group):
    return [symbol for g, symbol, _res, _args in ABI_TABLE if g == group]


STABLE_ABI_SYMBOLS = _symbols("stable")
DEBUG_SYMBOLS = _symbols("debug")
YUV_SYMBOLS = _symbols("yuv")
YUV_EX_SYMBOLS = _symbols("yuv_ex")
RGB_SYMBOLS = _symbols("rgb")
YUV_PACKED_SYMBOLS = _symbols("yuv_packed")
RECT_SYMBOLS = _symbols("rect")
RGB_RECT_SYMBOLS = _symbols("rgb_rect")
YUV_RECT_SYMBOLS = _symbols("yuv_rect")
YUV_PACKED_RECT_SYMBOLS = _symbols("yuv_packed_rect")
RECT_LIST_SYMBOLS = _symbols("rect_list")
RGB_RECT_LIST_SYMBOLS = _symbols("rgb_rect_list")
YUV_RECT_LIST_SYMBOLS = _symbols("yuv_rect_list")
YUV_PACKED_RECT_LIST_SYMBOLS = _symbols("yuv_packed_rect_list")
DELTA_SYMBOLS = _symbols("delta")
RGB_DELTA_SYMBOLS = _symbols("rgb_delta")
C_ABI_SYMBOLS = [symbol for _g, symbol, _res, _args in ABI_TABLE]   # everything the library exports besides the two C++ symbols
CXX_SYMBOLS = ["_Z20ConfigureFilterSRCNN15SRCNNFilterTypeb", "_Z12ProcessSRCNNPKhjjjfRPhRjPS1_Pj"]


def declare(L, older_build):
    """Give every function of the table its restype and argtypes on the loaded library L.  older_build: L is another build loaded
    for an A/B run (tools/lib_ab.py) and may lack the entry points of the extensions; the stable ABI it must have."""
    for group, symbol, res, args in ABI_TABLE:
        if group != "stable" and older_build and not hasattr(L, symbol):
            continue
        fn = getattr(L, symbol)
        fn.restype, fn.argtypes = res, args
    cfg = getattr(L, CXX_SYMBOLS[0])
    cfg.restype, cfg.argtypes = None, [i, C.c_bool]
    prc = getattr(L, CXX_SYMBOLS[1])
    # references are passed as pointers in the Itanium C++ ABI
    prc.restype = i
    prc.argtypes = [vp, u, u, u, f, pvp, pu, pvp, pu]
