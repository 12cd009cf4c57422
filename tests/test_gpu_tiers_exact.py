"""The fp32 non-parity tiers (SRCNN_MODE_RELAXED bits 1, 2, 4, 8 and SRCNN_MODE_FAST = 1 | 2 | 8) at tolerance 0.

Everywhere else the suite judges these tiers by max|dY| against the STRICT oracle (RELAX_BOUND, TOL_FAST), whose own distance
from them is about as large as the bound: arithmetic that is wrong the same way everywhere hides in that slack.  Each
relaxation has an exactly stated arithmetic, though (include/srcnn_amd_debug.h), and oracle/srcnn_tiers.c
restates it on the CPU with explicit fmaf / fma calls.  Here the kernels are compared with that restatement bit for bit,
through check() of test_gpu_conv12_tiers.py, at stage level (layers 1+2, layer 3) and over the whole Y path.

CPU part (no gpu mark): with nothing relaxed the restatement IS the oracle, stage by stage and over the whole path (this pins
its padding, tap, channel and weight order to the checker the suite trusts); relaxed, it stays inside the existing bounds of
the strict oracle and differs from it; and the inputs are such that a match means something (conditions below).

Layer 2 (bit 2) runs v_mfma_f32_32x32x2f32 with C = acc2.  How the two products of one K=2 step are rounded is decided on the
device by test_k2_probe: of the three models oracle/srcnn_tiers.c offers, K2_MODEL is the one the hardware follows.

Special values (NaN, Inf, denormals, -0 inputs) are left out: the tiers' statements say nothing about them.
SRCNN_MODE_FAST_F16 is no part of this: no statement fixes the order inside its 16-deep fp16 MFMA.  It is held bit for bit
where that order cannot show, on exactly summable inputs, in tests/test_gpu_fused_f16_exact.py.
"""
import contextlib

import numpy as np
import pytest

from libsrcnn_amd import synth
from test_gpu_conv12_tiers import check, cases, planes
from test_gpu_round4 import RELAX_BOUND

# upscaled-Y shapes (h, w) of the stage-level cases: ragged 32-pixel segments and 64 x 16 tiles, one row, one column, five
# tile columns of layers 1+2 / three 128-column tiles of k_conv3_fast with a 3-column ragged one; (20, 130): two tile rows
SHAPES = [(48, 78), (20, 130), (1, 33), (33, 1), (17, 259)]
CONTENTS = ("noise", "smooth", "mix", "-noise", "noise x1000")
PATH_SHAPES = [(24, 39), (10, 65), (37, 53)]            # source (h, w) of the whole-path cases
PATH_SEED = synth.SEED0 + 1301
BAND_CASE = "noise 53x37"
MIN_CHANGED = 0.05                                      # every relaxation / model pair: share of samples that must differ
MAX_CLAMPED = 0.15                                      # share of expected samples on 0 or 255

L1, L2, L3_X64, L3_F32 = 1, 2, 4, 8                     # SRCNN_RELAX_*
FAST = L1 | L2 | L3_F32                                 # SRCNN_MODE_FAST
K2_MODEL = 1                                            # Tiers.K2_A: the contract for bit 2 (test_k2_probe)


def stage_cases():
    return [("%s %dx%d" % (name, w, h), p) for (h, w) in SHAPES for name, p in planes(h, w) if name in CONTENTS]


def path_cases():
    return [("%s %dx%d" % (kind, w, h), synth.plane(h, w, PATH_SEED + i, kind))
            for i, (h, w) in enumerate(PATH_SHAPES) for kind in ("noise", "smooth")]


def frozen(a):
    a.setflags(write=False)
    return a


def differing(a, b):
    return int((a.view(np.uint32) != b.view(np.uint32)).sum())


def on_clamp(a):
    return int(((a == 0) | (a == 255)).sum())


@pytest.fixture(scope="module")
def tiers(oracle_lib):
    import oracle
    return oracle.Tiers(oracle_lib)


@pytest.fixture(scope="module")
def stage(oracle_lib, tiers):
    """{name: expectations} for the stage-level cases, computed once.  c12[mask]: layers 1+2 under mask 0..3 (bit 2 under
    K2_MODEL); c3[kind]: layer 3 of the ORACLE's layer-2 planes, strict / x64 / f32."""
    T = tiers
    ref = {}
    for name, p in stage_cases():
        c1 = [oracle_lib.conv1(p), T.conv1(p, fma=True)]
        c12 = {m: frozen(T.conv2(c1[m & 1], K2_MODEL if m & 2 else T.K2_STRICT)) for m in (1, 2, 3)}
        c12[0] = frozen(oracle_lib.conv2(c1[0]))
        c3 = {k: frozen(T.conv3(c12[0], k)) for k in (T.L3_X64, T.L3_F32)}
        c3[T.L3_STRICT] = frozen(oracle_lib.conv3(c12[0]))
        ref[name] = dict(p=p, c1=[frozen(c) for c in c1], c12=c12, c3=c3)
    return ref


@pytest.fixture(scope="module")
def k2(tiers, stage):
    """{name: {model: layers 1+2 with strict layer 1 and layer 2 under that K=2 model}}: what mask 2 may compute."""
    T = tiers
    return {name: {m: frozen(T.conv2(r["c1"][0], m)) for m in (T.K2_A, T.K2_B, T.K2_C)} for name, r in stage.items()}


@pytest.fixture(scope="module")
def path(oracle_lib, tiers):
    """{name: (y, {mask: restated 2x frame})} for the whole-path cases; mask 0 is the oracle's own frame."""
    ref = {}
    for name, y in path_cases():
        want = {m: frozen(tiers.y_path(y, mask=m, model=K2_MODEL)) for m in (1, 2, 4, 8, 7, 11)}
        want[0] = frozen(oracle_lib.y_path(y))
        ref[name] = (y, want)
    return ref


# ---- CPU: the restatement itself ----------------------------------------------------------------------------------------
def test_unrelaxed_restatement_is_the_oracle(oracle_lib, tiers, path):
    """Every restated stage with its relaxation off, on the planes of test_gpu_conv12_tiers.cases() (special values apart),
    and the whole path with mask 0: the oracle's bits."""
    T = tiers
    for name, p in cases():
        if name.startswith("special"):
            continue
        c1 = oracle_lib.conv1(p)
        check(T.conv1(p, fma=False), c1, "conv1, " + name)
        c2 = oracle_lib.conv2(c1)
        check(T.conv2(c1, T.K2_STRICT), c2, "conv2, " + name)
        check(T.conv3(c2, T.L3_STRICT), oracle_lib.conv3(c2), "conv3, " + name)
    for name in ("noise 39x24", "smooth 53x37"):
        y, want = path[name]
        check(T.y_path(y, mask=0), want[0], "y_path, " + name)
    y = synth.plane(21, 30, PATH_SEED + 9, "smooth")                      # not 2x, another filter
    check(T.y_path(y, 71, 47, filt=3, mask=0), oracle_lib.y_path(y, 71, 47, filt=3), "y_path 30x21 -> 71x47, lanczos3")
    with pytest.raises(ValueError):
        T.y_path(y, mask=L3_X64 | L3_F32)


@pytest.mark.parametrize("mask", [1, 2, 4, 8, 11])
def test_restated_tier_stays_within_its_bound_of_the_oracle(path, mask):
    """The restated whole path under each mask is a different result from the strict oracle's, within the bound the GPU tests
    of that mask already use (RELAX_BOUND of test_gpu_round4.py)."""
    for name, (_y, want) in path.items():
        d = np.abs(want[mask].astype(np.float64) - want[0])
        print("mask %2d, %-14s max|dY| %.3g, %.1f %% of the samples differ" % (mask, name, d.max(), 100.0 * (d > 0).mean()))
        assert 0 < d.max() <= RELAX_BOUND[mask], (mask, name, d.max())


def test_inputs_make_a_match_mean_something(tiers, stage, k2, path):
    """Conditions on the inputs; a failing condition fails the test.
    (1) Over the stage-level set, and over every shape of it alone, each relaxation changes at least MIN_CHANGED of the samples
        of its stage's output against strict.
    (2) The K=2 models A, B and C differ pairwise on at least MIN_CHANGED of the layer-2 samples.
    (3) At most MAX_CLAMPED of the expected whole-path samples lie on 0 or 255, under every mask.
    The stage-level layer-3 planes are NOT held to (3): they are layer 2 of planes taken as the upscaled Y directly, and such
    noise is far harsher than a resampled frame.  Of their strict layer-3 samples 39 % lie on the clamp (smooth 0 %, mix 9 %,
    noise 25 %, -noise 62 %, noise x1000 99.9 %).  What (3) is for -- the clamp must not hide a difference -- is asserted for
    them by (1) instead, which counts differences in the stored, clamped samples, shape by shape."""
    T = tiers
    n1 = n2 = n3 = 0
    changed = {}
    pairs = {(a, b): 0 for a, b in ((T.K2_A, T.K2_B), (T.K2_A, T.K2_C), (T.K2_B, T.K2_C))}
    for name, r in stage.items():
        shape = name.rsplit(" ", 1)[1]
        c1, c12, c3 = r["c1"], r["c12"], r["c3"]
        for what, n, a, b in (("L1", c1[0].size, c1[0], c1[1]), ("L2", c12[0].size, c12[0], k2[name][K2_MODEL]),
                              ("L3_X64", c3[0].size, c3[0], c3[T.L3_X64]), ("L3_F32", c3[0].size, c3[0], c3[T.L3_F32])):
            for key in ((what, "all"), (what, shape)):
                d = changed.setdefault(key, [0, 0])
                d[0] += differing(a, b)
                d[1] += n
        for a, b in pairs:
            pairs[(a, b)] += differing(k2[name][a], k2[name][b])
        n1 += c1[0].size; n2 += c12[0].size; n3 += c3[0].size
    for (what, where), (d, n) in sorted(changed.items()):
        print("%-6s %-8s differs from strict on %5.1f %% of %d samples" % (what, where, 100.0 * d / n, n))
        assert d >= MIN_CHANGED * n, (what, where, d, n)
    for (a, b), d in pairs.items():
        print("K=2 models %d and %d differ on %.1f %% of the layer-2 samples" % (a, b, 100.0 * d / n2))
        assert d >= MIN_CHANGED * n2, (a, b, d, n2)
    clamped = sum(on_clamp(r["c3"][0]) for r in stage.values())
    print("stage-level layer 3: %.1f %% of the strict samples on 0 or 255 (not asserted, see above)" % (100.0 * clamped / n3))
    for mask in (0, 1, 2, 4, 8, 7, 11):
        c = sum(on_clamp(want[mask]) for _y, want in path.values())
        n = sum(want[mask].size for _y, want in path.values())
        print("whole path, mask %2d: %.1f %% of the expected samples on 0 or 255" % (mask, 100.0 * c / n))
        assert c <= MAX_CLAMPED * n, (mask, c, n)
        for name, (_y, want) in path.items():
            assert on_clamp(want[mask]) <= MAX_CLAMPED * want[mask].size, (mask, name)


# ---- GPU: the kernels against the restatement, tolerance 0 ---------------------------------------------------------------
@contextlib.contextmanager
def tier(S, mode, mask=None):
    """The mode (and for MODE_RELAXED the mask) for the calls inside, restored afterwards whatever happens.  A strict-only
    build refuses the mode: conftest turns that error into a skip."""
    prev_mask = None if mask is None else S.set_relaxation(mask)
    try:
        prev = S.set_mode(mode)
        try:
            yield
        finally:
            S.set_mode(prev)
    finally:
        if prev_mask is not None:
            S.set_relaxation(prev_mask)


def tier_of(S, which):
    return tier(S, S.MODE_FAST) if which == "FAST" else tier(S, S.MODE_RELAXED, which)


@pytest.mark.gpu
def test_k2_probe(srcnn, stage, k2):
    """Bit 2 alone (strict layer 1, layer 2 as 32 chained K=2 MFMAs) against each model of the K=2 step: exactly one model gives
    the kernel's bits on every plane, and it is K2_MODEL."""
    S = srcnn
    counts = dict.fromkeys(next(iter(k2.values())), 0)
    total = 0
    with tier(S, S.MODE_RELAXED, L2):
        got = {name: S.conv12(r["p"]) for name, r in stage.items()}
    for name, g in got.items():
        total += g.size
        for model, want in k2[name].items():
            assert g.shape == want.shape
            counts[model] += differing(np.ascontiguousarray(g, np.float32), want)
    from oracle import Tiers
    for model, n in sorted(counts.items()):
        print("K=2 model %s: %d of %d samples differ" % (Tiers.K2_NAMES[model], n, total))
    assert [m for m, n in counts.items() if n == 0] == [K2_MODEL], counts


@pytest.mark.gpu
@pytest.mark.parametrize("which", [1, 2, 3, "FAST"])
def test_stage_layers_1_and_2(srcnn, stage, which):
    """srcnn_conv12_f32_dev under masks 1, 2, 3 and SRCNN_MODE_FAST == conv2(conv1(plane, fma), model) of the restatement."""
    S = srcnn
    mask = FAST & 3 if which == "FAST" else which
    with tier_of(S, which):
        got = {name: S.conv12(r["p"]) for name, r in stage.items()}
    for name, r in stage.items():
        check(got[name], r["c12"][mask], "conv12 under %s, %s" % (which, name))
    name, r = next(iter(stage.items()))
    check(S.conv12(r["p"]), r["c12"][0], "strict conv12 afterwards, " + name)


@pytest.mark.gpu
@pytest.mark.parametrize("mask", [L3_X64, L3_F32])
def test_stage_layer_3(srcnn, stage, tiers, mask):
    """srcnn_conv3_f32_dev under mask 4 (k_conv3<..., X64>) and mask 8 (k_conv3_fast) on the oracle's layer-2 planes == conv3(c2,
    kind) of the restatement."""
    S = srcnn
    kind = tiers.L3_X64 if mask == L3_X64 else tiers.L3_F32
    with tier(S, S.MODE_RELAXED, mask):
        got = {name: S.conv3(r["c12"][0]) for name, r in stage.items()}
    for name, r in stage.items():
        check(got[name], r["c3"][kind], "conv3 under mask %d, %s" % (mask, name))
    name, r = next(iter(stage.items()))
    check(S.conv3(r["c12"][0]), r["c3"][0], "strict conv3 afterwards, " + name)


@pytest.mark.gpu
@pytest.mark.parametrize("which", ["FAST", 7, 11])
def test_whole_path(srcnn, path, which):
    """srcnn_y_upscale2x_f32 under SRCNN_MODE_FAST and masks 7 and 11 == the restated y_path (strict resample, then the layers)."""
    S = srcnn
    mask = FAST if which == "FAST" else which
    with tier_of(S, which):
        got = {name: S.y_upscale2x(y) for name, (y, _want) in path.items()}
    for name, (_y, want) in path.items():
        check(got[name], want[mask], "y_upscale2x under %s, %s" % (which, name))
    name, (y, want) = next(iter(path.items()))
    check(S.y_upscale2x(y), want[0], "strict y_upscale2x afterwards, " + name)


@pytest.mark.gpu
@pytest.mark.parametrize("which", ["FAST", 7])
def test_whole_path_bands(srcnn, path, which):
    """Bands of one frame (the first rows, rows that start and end inside a tile, the last two rows) == the same rows of the
    restated frame."""
    S = srcnn
    y, want = path[BAND_CASE]
    mask = FAST if which == "FAST" else which
    dh = want[0].shape[0]
    bands = [(0, 11), (11, 23), (dh - 2, 2)]
    with tier_of(S, which):
        got = [S.y_upscale2x_band(y, r0, n) for r0, n in bands]
    for (r0, n), g in zip(bands, got):
        check(g, want[mask][r0:r0 + n], "band rows %d+%d under %s" % (r0, n, which))
    check(S.y_upscale2x_band(y, 11, 23), want[0][11:34], "strict band afterwards")
