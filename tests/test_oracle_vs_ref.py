"""CPU: the oracle against the real reference compiled from its own sources (oracle/_ref).

oracle/_ref/libsrcnn_ref.so exists only where `make -C oracle ref` could compile the reference's sources.  Every case is
also pinned by the sha256 of the reference's own output bytes for it, recorded in tests/golden/reference_digests.json
(`python tests/test_oracle_vs_ref.py --record`, with oracle/_ref built).  With the reference present a case is held bit for
bit against it and the reference against its recorded digest; without it, the oracle's output is held against the recorded
digest alone -- the same bits either way.
"""
import hashlib
import json
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)
import oracle  # noqa: E402
from conftest import assert_bit_equal  # noqa: E402

DIGESTS = os.path.join(ROOT, "tests", "golden", "reference_digests.json")
STAGEWISE = [((24, 40), 0), ((31, 17), 1), ((1, 9), 2), ((9, 1), 3), ((2, 2), 4), ((48, 6), 5)]
FILTERS = range(5)
DSTS = [(46, 38), (30, 20), (23, 40), (40, 19), (8, 7)]


def digest(arrays):
    h = hashlib.sha256()
    for a in arrays:
        a = np.ascontiguousarray(a)
        h.update(("%s%s" % (a.dtype.str, a.shape)).encode())
        h.update(a.tobytes())
    return h.hexdigest()


# ---- the cases: each returns the arrays an engine (oracle.Oracle or oracle.Reference) produces for it ----------------------
def case_weights(eng):
    return [eng.weights()]


def case_stagewise(eng, shape, seed):
    rng = np.random.default_rng(seed)
    y = (rng.random(shape) * 255).astype(np.float32)
    return list(eng.y_path(y, taps=True))


def case_layers(eng):
    rng = np.random.default_rng(7)
    y = (rng.random((14, 22)) * 255).astype(np.float32)
    c1 = (rng.random((64, 10, 12)) * 300 - 20).astype(np.float32)
    c2 = (rng.random((32, 11, 13)) * 200).astype(np.float32)
    return [eng.conv1(y), eng.conv2(c1), eng.conv3(c2)]


def case_resampler(eng, filt, dst):
    rng = np.random.default_rng(filt)
    y = (rng.random((19, 23)) * 255).astype(np.float32)
    return [eng.resample(y, dst[0], dst[1], filt)]


def case_process(eng):
    rng = np.random.default_rng(11)
    out = []
    for d in (3, 4):
        img = rng.integers(0, 256, (17, 21, d), dtype=np.uint8)
        for m, f in ((2.0, 2), (1.5, 2), (2.0, 1), (2.0, 0), (2.5, 3)):
            out.extend(eng.process(img, m, f))
    return out


def all_cases():
    cases = {"weights": (case_weights, ()), "layers": (case_layers, ()), "process": (case_process, ())}
    for shape, seed in STAGEWISE:
        cases["stagewise/%dx%d/%d" % (shape + (seed,))] = (case_stagewise, (shape, seed))
    for filt in FILTERS:
        for dst in DSTS:
            cases["resample/%d/%dx%d" % ((filt,) + dst)] = (case_resampler, (filt, dst))
    return cases


@pytest.fixture(scope="module")
def ref():
    return oracle.Reference() if oracle.have_reference() else None


@pytest.fixture(scope="module")
def recorded():
    with open(DIGESTS) as f:
        return json.load(f)


def pinned(recorded, key, got, want):
    """`want` is the live reference's output (None where oracle/_ref is absent): it must still be what was recorded, and
    the oracle's output must carry the recorded digest."""
    if want is not None:
        assert digest(want) == recorded[key], "%s: the reference's output no longer matches its recorded digest" % key
    assert digest(got) == recorded[key], "%s: the oracle's output differs from the reference's (recorded digest)" % key


def test_weights_identical(ref, recorded, oracle_lib):
    got = case_weights(oracle_lib)
    want = case_weights(ref) if ref is not None else None
    if want is not None:
        assert np.array_equal(want[0].view(np.uint32), got[0].view(np.uint32))
    pinned(recorded, "weights", got, want)


@pytest.mark.parametrize("shape,seed", STAGEWISE)
def test_stagewise_bit_identical(ref, recorded, oracle_lib, shape, seed):
    got = case_stagewise(oracle_lib, shape, seed)
    want = case_stagewise(ref, shape, seed) if ref is not None else None
    if want is not None:
        for g, w, what in zip(got, want, ("out", "upscaled", "layer-1", "layer-2")):
            assert_bit_equal(g, w, what)
    pinned(recorded, "stagewise/%dx%d/%d" % (shape + (seed,)), got, want)


def test_layers_fed_independently(ref, recorded, oracle_lib):
    got = case_layers(oracle_lib)
    want = case_layers(ref) if ref is not None else None
    if want is not None:
        for g, w, what in zip(got, want, ("conv1", "conv2", "conv3")):
            assert_bit_equal(g, w, what)
    pinned(recorded, "layers", got, want)


@pytest.mark.parametrize("filt", FILTERS)
@pytest.mark.parametrize("dst", DSTS)
def test_resampler(ref, recorded, oracle_lib, filt, dst):
    got = case_resampler(oracle_lib, filt, dst)
    want = case_resampler(ref, filt, dst) if ref is not None else None
    if want is not None:
        assert_bit_equal(got[0], want[0])
    pinned(recorded, "resample/%d/%dx%d" % ((filt,) + dst), got, want)


def test_process_rgb_rgba(ref, recorded, oracle_lib):
    got = case_process(oracle_lib)
    want = case_process(ref) if ref is not None else None
    if want is not None:
        for i, (a, b) in enumerate(zip(got, want)):
            assert np.array_equal(a, b), i
    pinned(recorded, "process", got, want)


if __name__ == "__main__":
    # --record: rewrite tests/golden/reference_digests.json from the compiled reference (oracle/_ref must exist)
    if sys.argv[1:] != ["--record"]:
        sys.exit("usage: python tests/test_oracle_vs_ref.py --record")
    eng = oracle.Reference()
    rec = {key: digest(fn(eng, *a)) for key, (fn, a) in sorted(all_cases().items())}
    with open(DIGESTS, "w") as f:
        json.dump(rec, f, indent=1, sort_keys=True)
        f.write("\n")
    print("recorded %d digests of the reference's outputs in %s" % (len(rec), DIGESTS))
