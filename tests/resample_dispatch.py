"""Which resampler / colour-shell kernel a call lands in -- a model of the library's launch decisions, for the tests only.

The model decides COVERAGE, never correctness: the case lists of tests/test_gpu_resample_dispatch.py and
tests/test_gpu_colour_shell.py are checked against it on the CPU (tests/test_resample_dispatch_model.py), and every GPU
result is compared with the oracle bit for bit.  It reads the product's own axis tables through srcnn_axis_table (host code:
no device needed) and mirrors, line for line:

  resample_src_rows       libsrcnn_amd/csrc/srcnn_capi.cpp (resample_src_rows)   the plane-resample branches
  rs2d_plan               libsrcnn_amd/csrc/srcnn_kernels.hip:1398-1427 MAXT, LW, patch rows, LDS, grid
  rs2d_fits               libsrcnn_amd/csrc/srcnn_kernels.hip:1467-1472
  launch_rs2d             libsrcnn_amd/csrc/srcnn_kernels.hip:1474-1501 DMA form, vec flag
  launch_merge_fused      libsrcnn_amd/csrc/srcnn_kernels.hip:1503-1521
  get_table (monotone)    libsrcnn_amd/csrc/srcnn_capi.cpp (get_table)
  process_share           libsrcnn_amd/csrc/srcnn_pipeline.cpp:389-436  fused or plane shell, buffer offsets
  launch_rgb_split / launch_ycc_merge   srcnn_kernels.hip:1699-1747   4-pixel forms and scalar tails

Only the single-band form of the colour shell is modelled (outputs below 8 MB on one context): the band cuts of larger
images depend on the device's persistent-grid size.  If a launcher changes, this file changes with it.
"""
import functools

import numpy as np

RS_TH = 16                    # tile rows                                   srcnn_kernels.hip:155
RS_MAX_TPB = 16               #                                             srcnn_kernels.hip:156
RS_LDS_LIMIT = 96 * 1024      # dynamic LDS a k_rs2d launch may ask for     srcnn_kernels.hip:1392
DMA_LDS_LIMIT = 64 * 1024     # k_rs2d_dma: M0's 16-bit LDS address         srcnn_kernels.hip:1490

FILTERS = (0, 1, 2, 3, 4)
FILTER_NAMES = ("nearest", "bilinear", "bicubic", "lanczos3", "bspline")

# library settings a case runs under (read at load: one subprocess per non-default set)
DEFAULT = {"rs_dma": True, "resample_2pass": False, "shell_unfused": False}
ENVS = {
    "default": ({}, DEFAULT),
    "rs_dma0": ({"SRCNN_RS_DMA": "0"}, dict(DEFAULT, rs_dma=False)),
    "2pass": ({"SRCNN_RESAMPLE_2PASS": "1"}, dict(DEFAULT, resample_2pass=True)),
    "unfused": ({"SRCNN_SHELL_UNFUSED": "1"}, dict(DEFAULT, shell_unfused=True)),
}


def chroma_filter(filt):
    """Cb / Cr / A are resampled with box when nearest is configured, else bilinear (srcnn_pipeline.cpp:865)."""
    return 0 if filt == 0 else 1


def cdiv(a, b):
    return (a + b - 1) // b


class Table:
    """An axis table as the launchers see it (DeviceTable: first, taps, max_taps, monotone)."""

    def __init__(self, filt, dst_len, src_len):
        import libsrcnn_amd as S
        left, right, w = S.axis_table(dst_len, src_len, filt)
        window = w.shape[1] - 1
        self.first = left.astype(np.int64)
        self.taps = np.minimum(right.astype(np.int64) - left + 1, window)           # resample_table.hpp:126-129
        self.end = self.first + self.taps
        self.max_taps = int(self.taps.max())
        self.monotone = bool(np.all(np.diff(self.first) >= 0) and np.all(np.diff(self.end) >= 0))   # get_table, srcnn_capi.cpp


@functools.lru_cache(maxsize=None)
def table(filt, dst_len, src_len):
    return Table(filt, dst_len, src_len)


def rs_lds_bytes(np_, maxt, sr, lw):                                              # srcnn_kernels.hip:157-161
    return 2 * (RS_TH * maxt * 8 + RS_TH * 2 * 4) + np_ * (2 * sr + RS_TH) * lw * 4


class Plan:
    ok = False
    maxt = lw = sr = lds = 0


def rs2d_plan(np_, dst_w, dst_row0, dst_rows, tv, th, sliding=False):
    """srcnn_kernels.hip:1398-1427 (tpb from the default SRCNN_RS_TPB = 0)."""
    p = Plan()
    if dst_rows <= 0 or dst_w <= 0 or not tv.monotone or not th.monotone:
        return p
    m = max(tv.max_taps, th.max_taps)
    if m > 8:
        return p
    p.maxt = 3 if m <= 3 else (5 if m <= 5 else 8)
    x0 = np.arange(0, dst_w, 256)
    xl = np.minimum(x0 + 256, dst_w) - 1
    span = int((th.end[xl] - th.first[x0]).max())
    p.lw = 136 if span + 1 <= 136 else (272 if span + 1 <= 272 else 0)
    r = np.arange(0, dst_rows, 1 if sliding else RS_TH)
    y0 = dst_row0 + r
    yl = dst_row0 + np.minimum(r + RS_TH, dst_rows) - 1
    p.sr = int((tv.end[yl] - tv.first[y0]).max())
    p.lds = rs_lds_bytes(np_, p.maxt, p.sr, p.lw)
    tiles_y = cdiv(dst_rows, RS_TH)
    gx = cdiv(dst_w, 256)
    tpb = max(1, min(RS_MAX_TPB, cdiv(gx * tiles_y, 1024)))
    gy = cdiv(tiles_y, tpb)
    p.ok = p.lw > 0 and p.sr > 0 and p.lds <= RS_LDS_LIMIT and gy <= 65535
    return p


def rs2d_fits(np_, sw, sh, dw, dh, r0, r1, tv, th):                               # srcnn_kernels.hip:1467-1472
    if dw < sw or dh < sh or r1 <= r0:
        return False
    p = rs2d_plan(np_, dw, r0, r1 - r0, tv, th, True)
    return p.lw > 0 and p.sr > 0 and p.maxt > 0 and p.lds <= RS_LDS_LIMIT


def rs2d_cell(p, dma, vec):
    return "rs2d(MAXT=%d,LW=%d,%s,%s)" % (p.maxt, p.lw, "dma" if dma else "nodma", "vec" if vec else "scalar")


def plane_cell(filt, sw, sh, dw, dh, settings=DEFAULT, dst_aligned16=True, r0=0, r1=None):
    """The kernel(s) srcnn_resample_f32_dev / the Y path's resample of a float plane runs for destination rows [r0, r1)
    (resample_src_rows of srcnn_capi.cpp).  dst_aligned16: the destination pointer is 16-byte aligned."""
    r1 = dh if r1 is None else r1
    if sw == dw and sh == dh:
        return "identity"
    if dw > sw and sh != dh and not settings["resample_2pass"] and dh >= sh:
        th, tv = table(filt, dw, sw), table(filt, dh, sh)
        p = rs2d_plan(1, dw, r0, r1 - r0, tv, th)                               # launch_rs2d, srcnn_kernels.hip:1474-1501
        if p.ok:
            vec = dw % 4 == 0 and dst_aligned16
            dma = settings["rs_dma"] and p.lds + RS_TH * p.lw * 4 <= DMA_LDS_LIMIT
            return rs2d_cell(p, dma, vec)
    if dw <= sw:
        if sw != dw:
            return "h-first" if sh != dh else "rows-only"
        return "cols-only"
    return "v-first" if sh != dh else "rows-only"


def out_size(w, h, mul):
    """int(w * (float)mul), as srcnn_output_size / the oracle compute it."""
    m = np.float32(mul)
    return int(np.float32(w) * m), int(np.float32(h) * m)


def shell_cells(filt, w, h, d, mul, conv=True, settings=DEFAULT):
    """(shell, cells) for a single-band srcnn_process_u8 / ProcessSRCNN call (process_share, srcnn_pipeline.cpp:389-600).
    shell is "fused" or "plane:<reason>"; cells is the set of kernel cells the call runs."""
    dw, dh = out_size(w, h, mul)
    n, share_px = w * h, dw * dh
    cf = chroma_filter(filt)
    identity = dw == w and dh == h
    cells = set()
    reason = None
    if identity:
        reason = "identity"
    elif settings["shell_unfused"]:
        reason = "SRCNN_SHELL_UNFUSED"
    elif settings["resample_2pass"]:
        reason = "SRCNN_RESAMPLE_2PASS"
    elif not (dw > w and dh > h):
        reason = "not-up-both"
    else:
        yv, yh = table(filt, dh, h), table(filt, dw, w)
        cv, ch = table(cf, dh, h), table(cf, dw, w)
        if not rs2d_fits(1, w, h, dw, dh, 0, dh, yv, yh):
            reason = "rs2d-refuses-Y"
        elif not rs2d_fits(d - 1, w, h, dw, dh, 0, dh, cv, ch):
            reason = "rs2d-refuses-chroma"
        else:
            # Y from the interleaved source: KIND 1 into ws.up (hipMalloc'd, so vec = dw % 4 == 0)
            p = rs2d_plan(1, dw, 0, dh, yv, yh)
            assert p.ok
            cells.add("K1(D=%d,MAXT=%d,LW=%d,%s)" % (d, p.maxt, p.lw, "vec" if dw % 4 == 0 else "scalar"))
            # merge: Yp = ws.planes, out = ws.bytes + n*d, conv = out + share_px*d (srcnn_pipeline.cpp:419-423)
            p = rs2d_plan(d - 1, dw, 0, dh, cv, ch)
            assert p.ok
            vec = dw % 4 == 0 and (n * d) % 4 == 0 and (not conv or (n * d + share_px * d) % 4 == 0)
            cells.add("K2(D=%d,CONV=%d,MAXT=%d,LW=%d,%s)" % (d, int(conv), p.maxt, p.lw, "vec" if vec else "scalar"))
            return "fused", cells
    # plane shell.  planes = [Y' share_px][Y Cb Cr A: 4 x n][Cb' Cr' A': 3 x share_px] floats (srcnn_pipeline.cpp:426-434);
    # bytes = [source n*d][out share_px*d][conv share_px]
    a16 = lambda floats: floats % 4 == 0
    split_aligned = all(a16(share_px + k * n) for k in range(d))
    form = lambda count, aligned: ("4" if count % 4 == 0 else "4+tail") if count >= 1024 and aligned else "scalar"
    cells.add("split-" + form(n, split_aligned))
    merge_aligned = (all(a16(x) for x in [0] + [share_px + 4 * n + k * share_px for k in range(d - 1)])
                     and (n * d) % 4 == 0 and (not conv or (n * d + share_px * d) % 4 == 0))
    cells.add("merge%d-%s" % (d, form(share_px, merge_aligned)))
    if not identity:
        cells.add("Y:" + plane_cell(filt, w, h, dw, dh, settings))
        cells.add("C:" + plane_cell(cf, w, h, dw, dh, settings))
    return "plane:" + reason, cells


# ---- the cells a plane resample can name, per filter ----
def plane_universe():
    u = {"identity", "rows-only", "cols-only", "h-first", "v-first"}
    for maxt in (3, 5, 8):
        for lw in (136, 272):
            for dma in ("dma", "nodma"):
                for vec in ("vec", "scalar"):
                    u.add("rs2d(MAXT=%d,LW=%d,%s,%s)" % (maxt, lw, dma, vec))
    return u


def shell_universe():
    u = set()
    for reason in ("identity", "SRCNN_SHELL_UNFUSED", "SRCNN_RESAMPLE_2PASS", "not-up-both", "rs2d-refuses-Y",
                   "rs2d-refuses-chroma"):
        u.add("plane:" + reason)
    for form in ("4", "4+tail", "scalar"):
        u.add("split-" + form)
        for d in (3, 4):
            u.add("merge%d-%s" % (d, form))
    for d in (3, 4):
        for maxt in (3, 5, 8):
            for lw in (136, 272):
                for vec in ("vec", "scalar"):
                    u.add("K1(D=%d,MAXT=%d,LW=%d,%s)" % (d, maxt, lw, vec))
                    for conv in (0, 1):
                        u.add("K2(D=%d,CONV=%d,MAXT=%d,LW=%d,%s)" % (d, conv, maxt, lw, vec))
    return u
