"""The fused fp16 kernel (k_fused_f16, SRCNN_MODE_FAST_F16) and its host packer at tolerance 0, on exactly summable inputs.

Everywhere else the suite judges this tier by max|dY| <= TOL_FAST_F16 = 6e-4 against the strict oracle, behind the resampler: no
statement fixes the order inside its 16-deep fp16 MFMA, so with the trained weights no bit-exact expectation exists.  That bound
cannot see a lo piece dropped on one fragment, two taps or channels with similar weights exchanged, or a border sample taken one
position off (1e-5 to 1e-4 on natural content).  The order of a sum matters only where the sum rounds, though.  With chosen
weights -- small integers and dyadic fractions -- every sum of the kernel is exact in fp32 in any order, and its output is fixed
bit for bit by the statement of DESIGN.md section 3, which tests/fused_f16_model.py restates in numpy.  The kernel runs on such
weights through the test hook srcnn_debug_fused_f16 (include/srcnn_amd_debug.h): the product's two packers, the product's launcher.
The hook is driven through the loaded library handle; the binding does not carry it.

CPU part (no gpu mark): the conditions under which a match means something, (a) to (g) below, each asserted.
GPU part: every case at every shape, bands with the whole plane and with exactly the halo staged, the hook against the product
path, the argument checks.
"""
import ctypes as C

import numpy as np
import pytest

import fused_f16_model as M
from libsrcnn_amd import synth
from test_gpu_configs import TOL_FAST_F16
from test_gpu_conv12_tiers import check
from test_gpu_tiers_exact import MAX_CLAMPED, MIN_CHANGED, differing, frozen, tier

MIN_LO = 0.25                                   # (c): share of a wide set's operands X whose lo piece is non-zero
BORDER = 6                                      # the border mutations are counted within this frame (layer 3's 2 + layer 1's 4)
BANDS = [(0, 1), (65, 1), (3, 7), (15, 18), (60, 6)]            # (first row, rows) of the dense plane at M.BAND_SHAPE
PRODUCT_SHAPES = [(37, 29), (100, 245)]         # source (h, w), of test_fused_f16_bands_tiles_and_chunks: one strip; two workgroup strips
CANARY = 0xDEADBEEF                             # bit pattern of the guard rows around d_out (a NaN no kernel writes)
GUARD_ROWS = 3
E_ARG = -1
# which sets a mutation of the model is looked for in, in this order (condition (g): at least one case shows it)
MUTATION_SETS = {"yl": ["wide-Y"], "w1l": ["wide-W1"], "c1l": ["wide-c1/W2"], "w2l": ["wide-c1/W2"], "c2l": ["wide-c2/W3"],
                 "w3l": ["wide-c2/W3"]}


@pytest.fixture(scope="module")
def expected():
    """{case: (blob, up, Y', report, X, budget)}, computed once: model() with the exactness check on."""
    ref = {}
    for name, blob, up, x, budget in M.cases():
        out, report = M.model(up, blob)
        ref[name] = (blob, up, frozen(out), report, x, budget)
    return ref


def of_set(expected, which):
    return {name: e for name, e in expected.items() if name.rsplit(" ", 1)[0] == which}


# ---- CPU: the conditions ---------------------------------------------------------------------------------------------------
def test_cases_are_exactly_summable_and_mean_something(expected):
    """Per case, printed and asserted:
    (a) every sum's (sum|terms| + |C|) / q is within the set's budget (2^21 for every set: fp32's 24 bits less three guard bits),
        every sum is exactly representable in fp32 (model() raises otherwise) and so is the result of the last fmaf, so no low
        bit of a sum is rounded away before it is stored;
    (b) no piece is a non-zero fp16 subnormal;
    (c) in a wide-X set the lo piece of X is non-zero on at least MIN_LO of X's operands (activations and Y: of all samples;
        weights: of the non-zero weights), and in dense every weight and Y is narrow;
    (d) at most MAX_CLAMPED of the expected samples lie on 0 or 255;
    (e) for dense, model == plain bit for bit."""
    assert sorted({name.rsplit(" ", 1)[0] for name in expected}) == sorted(["dense", "wide-Y", "wide-W1", "wide-c1/W2", "wide-c2/W3"])
    assert len(of_set(expected, "dense")) == len(M.SHAPES) + 1 and all(len(of_set(expected, s)) == 3 for s in ("wide-Y", "wide-W1"))
    for name, (blob, up, out, r, x, budget) in expected.items():
        sums = ("l1", "l2", "p", "gather")
        print("%-22s budget/2^21 %s | lo != 0 %s | on the clamp %.3f" % (
            name, " ".join("%s %.4f" % (k, r[k]["budget"] / 2.0 ** 21) for k in sums),
            " ".join("%s %.2f" % (k, v) for k, v in r["lo"].items()), r["clamped"]))
        assert budget <= 2.0 ** 21 if name.startswith("dense") else budget <= 2.0 ** 23
        for k in sums:
            assert r[k]["budget"] <= budget and r[k]["inexact"] == 0, (name, k, r[k])
        assert r["final_inexact"] == 0, (name, r["final_inexact"])
        assert r["subnormal"] == 0, (name, r["subnormal"])
        for operand in x:
            assert r["lo"][operand] >= MIN_LO, (name, operand, r["lo"])
        assert r["clamped"] <= MAX_CLAMPED, (name, r["clamped"])
        if name.startswith("dense"):
            assert r["lo"]["Y"] == r["lo"]["W1"] == r["lo"]["W2"] == r["lo"]["W3"] == 0, (name, r["lo"])
            check(M.plain(up, blob), out, "plain against model, " + name)
            b1, w1, b2, w2, b3, w3 = M.unpack(blob)
            assert w1.all() and w2.all() and w3.all()


def test_model_and_plain_meet_the_oracle_on_the_products_weights(oracle_lib, golden):
    """(f) With the product's weights on an oracle-resampled noise plane, plain and model (exactness check off) stay within
    TOL_FAST_F16 of oracle conv3(conv2(conv1)): the blob layout and the W3 transposition are the trusted checker's."""
    assert np.array_equal(golden.weights, oracle_lib.weights())
    y = synth.plane(13, 19, synth.SEED0 + 1501, "noise")
    up = oracle_lib.resample(y, 38, 26)
    want = oracle_lib.conv3(oracle_lib.conv2(oracle_lib.conv1(up))).astype(np.float64)
    got, report = M.model(up, golden.weights, exact=False)
    for what, g in (("plain", M.plain(up, golden.weights)), ("model", got)):
        d = float(np.abs(g - want).max())
        print("%s: max|dY| %.3g against the oracle" % (what, d))
        assert d <= TOL_FAST_F16, (what, d)
    assert report["l1"]["inexact"] > 0                      # real weights: the sums do round, which is why they pin no bits
    with pytest.raises(M.Inexact):
        M.model(up, golden.weights)


@pytest.mark.parametrize("mutation", M.MUTATIONS)
def test_a_mutated_model_changes_the_expected_bits(expected, mutation):
    """(g) Mutations of the MODEL: each changes at least MIN_CHANGED of the stored, clamped output samples of at least one case
    (the two border mutations: of the samples within BORDER of an edge).  A kernel or packer with that defect cannot match."""
    best = 0.0
    for which in MUTATION_SETS.get(mutation, ["dense"]):
        for name, (blob, up, out, _r, _x, _b) in of_set(expected, which).items():
            if up.size > 40 * 140:
                continue                                    # the small shapes decide
            mutated, _ = M.model(up, blob, drop=mutation, exact=False)
            diff = mutated.view(np.uint32) != out.view(np.uint32)
            if mutation in M.BORDER_MUTATIONS:
                frame = np.ones(out.shape, bool)
                frame[BORDER:-BORDER, BORDER:-BORDER] = False
                share = float(diff[frame].mean())
            else:
                share = float(diff.mean())
            print("%-13s %-22s changes %5.1f %% of the samples" % (mutation, name, 100.0 * share))
            best = max(best, share)
    assert best >= MIN_CHANGED, (mutation, best)


# ---- GPU: the kernel against the model, tolerance 0 ------------------------------------------------------------------------
def fused(S, blob, staged, h, up_row0, out_row0, out_rows, expect=0):
    """srcnn_debug_fused_f16 through the library handle: `staged` holds rows [up_row0, ...) of the upscaled plane of h rows; returns
    output rows [out_row0, +out_rows).  d_out sits between GUARD_ROWS canary rows, which must come back untouched; expect != 0:
    the call must return that code and leave d_out untouched too."""
    fn = S.lib().srcnn_debug_fused_f16
    fn.restype = C.c_int
    fn.argtypes = [C.c_void_p, C.c_void_p, C.c_uint, C.c_uint, C.c_uint, C.c_uint, C.c_void_p, C.c_uint, C.c_uint, C.c_void_p]
    staged = np.ascontiguousarray(staged, np.float32)
    w = staged.shape[1]
    rows = max(out_rows, 1)
    canvas = np.full((GUARD_ROWS + rows + GUARD_ROWS, max(w, 1)), CANARY, np.uint32)
    d_up = S.DeviceBuffer.from_numpy(staged if staged.size else np.zeros(1, np.float32))
    d_out = S.DeviceBuffer.from_numpy(canvas)
    try:
        weights = None if blob is None else np.ascontiguousarray(blob, np.float32)
        rc = fn(None if weights is None else weights.ctypes.data, d_up.ptr, w, h, up_row0, staged.shape[0],
                d_out.ptr + 4 * GUARD_ROWS * max(w, 1), out_row0, out_rows, None)
        got = d_out.to_numpy(np.uint32, canvas.shape)
    finally:
        d_up.free()
        d_out.free()
    if expect:
        assert rc == expect, (rc, expect)
        assert (got == CANARY).all(), "a refused call wrote to d_out"
        return None
    S.check(rc)
    assert (got[:GUARD_ROWS] == CANARY).all() and (got[GUARD_ROWS + rows:] == CANARY).all(), "canary rows around d_out overwritten"
    return got[GUARD_ROWS:GUARD_ROWS + rows].view(np.float32)


def halo(h, r0, n):
    """y_path_halo of srcnn_y_path_geom.hpp: the rows of upscaled Y that output rows [r0, r0 + n) of an h-row plane depend on."""
    return max(r0 - 6, 0), min(h, r0 + n + 6)


@pytest.mark.gpu
@pytest.mark.parametrize("which", ["dense", "wide-Y", "wide-W1", "wide-c1/W2", "wide-c2/W3"])
def test_kernel_matches_the_model_bit_for_bit(srcnn, expected, which):
    """Every case of the set at every shape: the hook on the whole plane == model, twice with equal bits."""
    S = srcnn
    compared = 0
    for name, (blob, up, want, _r, _x, _b) in of_set(expected, which).items():
        h = up.shape[0]
        got = fused(S, blob, up, h, 0, 0, h)
        check(got, want, name)
        assert differing(fused(S, blob, up, h, 0, 0, h), got) == 0, name + ": two runs differ"
        compared += got.size
    print("%s: %d samples compared at tolerance 0" % (which, compared))


@pytest.mark.gpu
def test_bands_match_the_model_bit_for_bit(srcnn, expected):
    """Bands of the dense plane at M.BAND_SHAPE (the first row, the last row, rows inside the first ring stage, rows across a
    16-row chunk boundary, the last rows), each with the whole plane staged and with exactly its halo staged -- the route the
    production band path takes, up_row0 > 0 but for the first band: the same rows of the model."""
    S = srcnn
    h, w = M.BAND_SHAPE
    blob, up, want, _r, _x, _b = expected["dense %dx%d" % (w, h)]
    for r0, n in BANDS:
        check(fused(S, blob, up, h, 0, r0, n), want[r0:r0 + n], "band %d+%d, whole plane staged" % (r0, n))
        a, b = halo(h, r0, n)
        assert (a > 0) == (r0 > 6)
        check(fused(S, blob, up[a:b], h, a, r0, n), want[r0:r0 + n], "band %d+%d, rows [%d,%d) staged" % (r0, n, a, b))


@pytest.mark.gpu
def test_the_hook_is_the_product(srcnn, golden):
    """With weights = NULL on the product's own resampled plane the hook gives the bits of srcnn_y_upscale2x_f32 under
    SRCNN_MODE_FAST_F16 (and of one srcnn_y_upscale2x_f32_band_dev band); with the product's blob passed as weights, the same bits:
    the hook's packers and launcher are the product's."""
    S = srcnn
    for i, (h, w) in enumerate(PRODUCT_SHAPES):
        y = synth.plane(h, w, synth.SEED0 + 7 * h + w, "noise")
        up = S.resample(y, 2 * w, 2 * h)
        with tier(S, S.MODE_FAST_F16):
            frame = S.y_upscale2x(y)
            band = S.y_upscale2x_band(y, 11, 23) if i == 0 else None
        got = fused(S, None, up, 2 * h, 0, 0, 2 * h)
        check(got, frame, "hook with the product's image against y_upscale2x, %dx%d" % (w, h))
        check(fused(S, golden.weights, up, 2 * h, 0, 0, 2 * h), frame, "hook with the product's blob against y_upscale2x, %dx%d" % (w, h))
        if band is not None:
            a, b = halo(2 * h, 11, 23)
            check(fused(S, None, up[a:b], 2 * h, a, 11, 23), band, "hook band against y_upscale2x_band")


@pytest.mark.gpu
def test_argument_checks_launch_nothing(srcnn, expected):
    """A staged span that does not cover the halo, and a zero size, give SRCNN_E_ARG and leave d_out untouched."""
    S = srcnn
    h, w = M.BAND_SHAPE
    blob, up, _want, _r, _x, _b = expected["dense %dx%d" % (w, h)]
    a, b = halo(h, 15, 18)                                                  # rows [9, 39)
    fused(S, blob, up[a + 1:b], h, a + 1, 15, 18, expect=E_ARG)             # one row short at the top
    fused(S, blob, up[a:b - 1], h, a, 15, 18, expect=E_ARG)                 # ... at the bottom
    fused(S, blob, up[a:b], h, a, 14, 18, expect=E_ARG)                     # the band moved up by one row
    fused(S, blob, up, h, 0, 60, 7, expect=E_ARG)                           # output rows past the plane
    fused(S, blob, up, h, 0, 15, 0, expect=E_ARG)                           # no output rows
    fused(S, blob, up[:0], h, 0, 0, 1, expect=E_ARG)                        # no staged rows
    fused(S, blob, up[:, :0], h, 0, 0, 1, expect=E_ARG)                     # no columns
    fused(S, blob, up, 0, 0, 0, 1, expect=E_ARG)                            # no plane rows
    check(fused(S, blob, up[a:b], h, a, 15, 18), expected["dense %dx%d" % (w, h)][2][15:33], "the same band, accepted")
