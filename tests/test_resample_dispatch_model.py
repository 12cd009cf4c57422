"""The GPU case lists of the resampler and the colour shell reach every kernel cell that can be reached (CPU only).

tests/resample_dispatch.py names the cell a call lands in from the product's host-side axis tables.  For every filter, the
cells the case lists of tests/test_gpu_resample_dispatch.py and tests/test_gpu_colour_shell.py reach (under every switch
set they run with) must be all the cells the model can name, except the ones listed below as unreachable.  A broad sweep
of shapes backs each unreachable entry: if the sweep reaches one, the entry is wrong.
"""
import pytest

import resample_dispatch as M
import test_gpu_colour_shell as SHELL
import test_gpu_resample_dispatch as PLANE

NARROW = (0, 1)          # nearest, bilinear: support <= 1, window 3
MITCHELL_LIKE = (2, 4)   # bicubic, bspline: support 2, window 5
LANCZOS = (3,)           # support 3, window 7


def plane_unreachable(filt):
    """{cell: reason} of the plane-resample cells filter `filt` can never reach."""
    out = {}
    for lw in (136, 272):
        for dma in ("dma", "nodma"):
            for vec in ("vec", "scalar"):
                name = lambda maxt: "rs2d(MAXT=%d,LW=%d,%s,%s)" % (maxt, lw, dma, vec)
                if filt in NARROW:
                    for maxt in (5, 8):
                        out[name(maxt)] = ("window of 3 taps: an up-scale row has at most 3 taps (longer rows only occur in "
                                           "down-scales, which rs2d refuses)")
                if filt in MITCHELL_LIKE:
                    out[name(8)] = ("window of 5 taps: an up-scale row has at most 5 taps (longer rows only occur in "
                                    "down-scales, which rs2d refuses)")
                if filt not in NARROW and lw == 272:
                    out[name(3)] = ("MAXT 3 needs a source width of at most 3 samples (every row <= 3 taps), so a tile "
                                    "spans at most 4 LDS columns")
                if filt in LANCZOS and lw == 272:
                    out[name(5)] = "MAXT 5 needs a source width of at most 5 samples, so a tile spans at most 6 LDS columns"
    return out


def shell_unreachable(filt):
    """{cell: reason} of the colour-shell cells filter `filt` can never reach (single-band calls)."""
    out = {
        "split-4+tail": "the source planes follow each other in one buffer, so w*h % 4 != 0 misaligns the Cb plane and the "
                        "whole split runs scalar",
        "merge3-4+tail": "likewise dw*dh % 4 != 0 misaligns the resampled Cb' plane: the whole merge runs scalar",
        "merge4-4+tail": "likewise dw*dh % 4 != 0 misaligns the resampled Cb' plane: the whole merge runs scalar",
        "plane:identity": "multiply 1.0: the identity-size deviation of the Y path is pinned by "
                          "test_gpu_parity.py::test_identity_size_deviation_is_pinned, not compared with the oracle",
    }
    if filt not in MITCHELL_LIKE:
        out["plane:rs2d-refuses-Y"] = ("this filter's up-scale tables are monotone and one plane's patch always fits the "
                                       "LDS, so rs2d_fits(1, ...) never refuses the Y plane")
    for d in (3, 4):
        for lw in (136, 272):
            for vec in ("vec", "scalar"):
                for maxt in (5, 8):
                    for conv in (0, 1):
                        out["K2(D=%d,CONV=%d,MAXT=%d,LW=%d,%s)" % (d, conv, maxt, lw, vec)] = (
                            "the chroma and alpha planes are resampled with box or bilinear (window 3): MAXT is 3")
                for maxt in (3, 5, 8):
                    k1 = "K1(D=%d,MAXT=%d,LW=%d,%s)" % (d, maxt, lw, vec)
                    if filt in NARROW and maxt > 3:
                        out[k1] = "window of 3 taps"
                    if filt in MITCHELL_LIKE and maxt == 8:
                        out[k1] = "window of 5 taps"
                    if filt not in NARROW and maxt == 3 and lw == 272:
                        out[k1] = "MAXT 3 needs a source width of at most 3 samples"
                    if filt in LANCZOS and maxt == 5 and lw == 272:
                        out[k1] = "MAXT 5 needs a source width of at most 5 samples"
    return out


def plane_reached(filt):
    got = {}
    for env in ("default", "rs_dma0", "2pass"):
        settings = M.ENVS[env][1]
        for c in PLANE.PLANE_CASES + PLANE.TALL_CASES:
            sh, sw, dh, dw = c
            offs = PLANE.offsets(dw) if env != "default" or c not in PLANE.TALL_CASES else (0,)
            for off in offs:
                got.setdefault(M.plane_cell(filt, sw, sh, dw, dh, settings, dst_aligned16=off % 16 == 0), (c, off, env))
    return got


def shell_reached(filt):
    got = {}
    for env in ("default", "unfused", "2pass"):
        settings = M.ENVS[env][1]
        for (h, w, d, f, mul) in SHELL.CASES:
            if f != filt:
                continue
            for conv in (True, False):
                shell, cells = M.shell_cells(filt, w, h, d, mul, conv, settings)
                for c in cells | {shell}:
                    got.setdefault(c, ((w, h, d, mul, conv), env))
    return got


@pytest.mark.parametrize("filt", M.FILTERS, ids=M.FILTER_NAMES)
def test_plane_cases_reach_every_reachable_cell(filt):
    unreachable = plane_unreachable(filt)
    missing = sorted(M.plane_universe() - set(plane_reached(filt)) - set(unreachable))
    assert not missing, "%s: no plane-resample case reaches %s" % (M.FILTER_NAMES[filt], missing)


@pytest.mark.parametrize("filt", M.FILTERS, ids=M.FILTER_NAMES)
def test_shell_cases_reach_every_reachable_cell(filt):
    unreachable = shell_unreachable(filt)
    missing = sorted(M.shell_universe() - set(shell_reached(filt)) - set(unreachable))
    assert not missing, "%s: no colour-shell case reaches %s" % (M.FILTER_NAMES[filt], missing)


def test_shell_cases_take_both_shells_and_every_output_width_residue():
    for filt in M.FILTERS:
        seen = set()
        for (h, w, d, f, mul) in SHELL.CASES:
            if f == filt:
                shell, _ = M.shell_cells(filt, w, h, d, mul)
                seen.add((shell.split(":")[0], d, M.out_size(w, h, mul)[0] % 4))
        want = {(s, d, r) for s in ("fused", "plane") for d in (3, 4) for r in range(4)}
        assert want <= seen, (M.FILTER_NAMES[filt], sorted(want - seen))


# ---- the unreachable entries hold over a broad sweep ----
SWEEP_LENS = (1, 2, 3, 4, 5, 6, 7, 9, 13, 17, 29, 40, 64, 100, 131, 150, 200, 260, 333)
SWEEP_HEIGHTS = (1, 2, 3, 4, 5, 9, 17, 40, 100)
SWEEP_RATIOS = (0.3, 0.5, 0.75, 1.0, 1.01, 1.25, 1.5, 1.9, 2.0, 2.5, 3.0, 5.0, 8.0)


@pytest.mark.parametrize("filt", M.FILTERS, ids=M.FILTER_NAMES)
def test_plane_unreachable_cells_stay_unreached(filt):
    unreachable = plane_unreachable(filt)
    hit = {}
    for sw in SWEEP_LENS:
        for sh in SWEEP_HEIGHTS:
            for rw in SWEEP_RATIOS:
                for rh in SWEEP_RATIOS:
                    dw, dh = max(1, int(sw * rw)), max(1, int(sh * rh))
                    for env in ("default", "rs_dma0"):
                        for aligned in (True, False):
                            c = M.plane_cell(filt, sw, sh, dw, dh, M.ENVS[env][1], aligned)
                            if c in unreachable:
                                hit.setdefault(c, (sw, sh, dw, dh, env))
    assert not hit, "%s: cells listed as unreachable are reached: %s" % (M.FILTER_NAMES[filt], hit)


@pytest.mark.parametrize("filt", M.FILTERS, ids=M.FILTER_NAMES)
def test_shell_unreachable_cells_stay_unreached(filt):
    unreachable = set(shell_unreachable(filt)) - {"plane:identity"}
    hit = {}
    for w in SWEEP_LENS:
        for h in SWEEP_HEIGHTS:
            for mul in (0.5, 0.75, 1.01, 1.25, 1.5, 1.9, 2.0, 2.5, 3.0, 5.0):
                dw, dh = M.out_size(w, h, mul)
                if not (dw and dh):
                    continue
                for d in (3, 4):
                    for conv in (True, False):
                        shell, cells = M.shell_cells(filt, w, h, d, mul, conv)
                        for c in (cells | {shell}) & unreachable:
                            hit.setdefault(c, (w, h, d, mul, conv))
    assert not hit, "%s: cells listed as unreachable are reached: %s" % (M.FILTER_NAMES[filt], hit)
