"""The tile loop of k_conv12_mfma beyond one item per workgroup, in every instance of the kernel.

The kernel is persistent.  With G = M_BPC x CUs resident workgroups (2 per CU) launch_conv12_mfma sizes the grid (G when there are at
least G tiles, else min(4 x tiles, G) with SRCNN_CONV12_SPREAD and the tile count without), the kernel takes the tiles that fill
whole rounds of the grid whole and deals the rest as quarter items, and a workgroup that runs a SECOND item draws it from the
tile queue through the two-slot LDS mailbox and the other Y buffer (or walks on with the static stride), and the last workgroup
out resets the queue's counters.  deal() restates that dealing; every case below is chosen by its tile count relative to G, read
from the device, and asserts from deal() which of those states it drives, so that on a part with another CU count the shapes
re-derive themselves or the test fails.

Everything goes through the stage call srcnn_conv12_f32_dev (one upscaled-Y plane in, 32 planes out) into a destination this
file allocates and fills with 0xFF bytes on the launch stream, followed by 4 KiB of slack that must stay 0xFF.  The stage call
runs on the workspace of its stream, so it draws from that workspace's tile queue as the path does (it used to run without a
workspace and therefore with the static stride under every setting: a kernel that never reset the queue passed this file's
stage-level tests).  The planes
are compared with the oracle's conv2(conv1(plane)) bit for bit (tolerance 0, check() of test_gpu_conv12_tiers.py: a NaN must meet
a NaN).  The oracle's planes hold no NaN for these inputs, so surviving poison is an unwritten sample, and no two 64 x 16 tiles of
a case's planes are equal, so a tile written to the wrong place cannot pass; both are conditions on the inputs, checked on the CPU.

The instances behind the SRCNN_CONV12_* switches are read at load, so each runs in a fresh process that regenerates the
inputs from the seeds, memory-maps the oracle's planes the parent wrote, and prints one JSON line of counts.
"""
import ctypes
import hashlib
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from libsrcnn_amd import synth
from test_gpu_conv12_tiers import FLAT, body_counts, check, kernel_tiers

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TILE_W, TILE_H = 64, 16                 # M_TW, M_TH of srcnn_kernels.hip
BPC = 2                                 # M_BPC: resident workgroups per CU
G_MI355X = 2 * 256                      # what the CPU-side checks assume where no device is visible
SEED = synth.SEED0 + 1301
BAND = 23                               # rows per content band: the seams fall everywhere inside the 16-row tiles
SLACK = 4096
POISON = 0xFFFFFFFF
MIN_SEGMENTS = 8
HIP_ATTR_MULTIPROCESSOR_COUNT = 63      # hipDeviceAttributeMultiprocessorCount (hip_runtime_api.h; cross-checked in device_G)


def deal(ntiles, G, spread):
    """(grid, full, nitems) of one launch: the grid launch_conv12_mfma chooses for `ntiles` tiles on G resident workgroups, the
    tiles k_conv12_mfma takes whole and the number of items it deals (whole tiles + four quarters per leftover tile)."""
    grid = G if ntiles >= G else (min(4 * ntiles, G) if spread else ntiles)
    full = (ntiles // grid) * grid
    nitems = full + 4 * (ntiles - full)
    return grid, full, nitems


# name: (tile count, what deal() must say with SRCNN_CONV12_SPREAD on, ragged width r of the last tile column, rows q missing
# from the last tile row).  The last item of a launch, the one `nitems` decides, is the last tile's fourth quarter: its odd rows,
# columns 32-63.  So r > 32 and q <= 14 everywhere, or a loop that ends one item early would lose nothing that is stored.
CASES = {
    "A": (lambda G: G // 4 + 1, lambda G, n: (G, 0, G + 4), 37, 5),            # first draw from the queue: four workgroups take a second quarter
    "B": (lambda G: G - 1, lambda G, n: (G, 0, 4 * (G - 1)), 37, 11),         # four rounds of quarter items
    "C": (lambda G: G, lambda G, n: (G, G, G), 50, 1),                        # every draw returns >= nitems: nobody loops; leaver reset
    "D": (lambda G: G + 1, lambda G, n: (G, G, G + 4), 37, 14),               # whole -> quarter inside one workgroup; the buffer flip it & 1
    "E": (lambda G: 2 * G - 1, lambda G, n: (G, G, G + 4 * (G - 1)), 33, 7),  # whole, then several quarter rounds
    "F": (lambda G: 2 * G, lambda G, n: (G, 2 * G, 2 * G), 64, 0),            # whole -> whole, no quarters; nothing ragged
    "H": (lambda G: 2 * G + 1, lambda G, n: (G, 2 * G, 2 * G + 4), 37, 3),    # whole -> whole -> quarter
    # the two small launches of the back-to-back list: fewer workgroups than G, one item each
    "n3": (lambda G: 3, lambda G, n: (12, 0, 12), 37, 5),
    "n1": (lambda G: 1, lambda G, n: (4, 0, 4), 37, 7),
}
MAIN = ["A", "B", "C", "D", "E", "F", "H"]
B2B = ["D", "A", "n3", "H", "n1", "C"]          # G+1, G/4+1, 3, 2G+1, 1, G tiles: the grid changes from launch to launch
SWITCH_CASES = ["A", "D", "H"]
SPREAD0_CASES = ["B", "D"]


def tiles_x_for(n):
    return next(t for t in (5, 3, 2, 1) if n % t == 0)


def shape_of(name, G):
    """(h, w, ntiles) of a case's upscaled-Y plane: tiles_x columns of tiles, the last r wide, the last tile row q rows short."""
    target, _cls, r, q = CASES[name]
    n = target(G)
    tx = tiles_x_for(n)
    w, h = TILE_W * (tx - 1) + r, TILE_H * (n // tx) - q
    assert h > 0 and -(-w // TILE_W) * -(-h // TILE_H) == n, (name, G, n, w, h)
    return h, w, n


def classify(name, G, spread=True):
    """deal() of the case, with the assertion that it is in the class the case is named for."""
    _h, _w, n = shape_of(name, G)
    got = deal(n, G, spread)
    if spread or n >= G:
        want = CASES[name][1](G, n)
    else:
        want = (n, n, n)                    # SPREAD=0 below G tiles: one whole tile per workgroup, no loop
    assert got == want, "case %s with G = %d: %d tiles deal as (grid, full, nitems) = %s, the case needs %s" % (name, G, n, got, want)
    return (n,) + got


def content(h, w, seed):
    """Noise, smooth and gentle smooth (FLAT + (smooth - mean) / 4: the T1 / T2 bodies of layer 2) in bands of BAND rows stacked
    down the plane.  No constant regions: every band carries per-sample noise."""
    noise = synth.plane(h, w, seed, "noise")
    smooth = synth.plane(h, w, seed + 1, "smooth")
    gentle = FLAT + (smooth - np.float32(smooth.mean())) * np.float32(0.25)
    kind = ((np.arange(h) // BAND) % 3)[:, None]
    return np.ascontiguousarray(np.where(kind == 0, noise, np.where(kind == 1, smooth, gentle)), np.float32)


def case_plane(name, G):
    h, w, _n = shape_of(name, G)
    return content(h, w, SEED + 16 * list(CASES).index(name))


def tile_digests(planes):
    """One digest per 64 x 16 tile of (32, h, w) planes (a ragged tile's shape is part of it)."""
    _, h, w = planes.shape
    out = []
    for y0 in range(0, h, TILE_H):
        for x0 in range(0, w, TILE_W):
            blk = np.ascontiguousarray(planes[:, y0:y0 + TILE_H, x0:x0 + TILE_W])
            out.append(hashlib.blake2b(blk.tobytes(), digest_size=16, person=b"%dx%d" % blk.shape[1:]).digest())
    return out


# ---- G -------------------------------------------------------------------------------------------------------------------
def device_G(S):
    """BPC x the CU count of the device behind context 0: hipDeviceGetAttribute(hipDeviceAttributeMultiprocessorCount) on the HIP
    runtime the library has bound, the number srcnn_capi.cpp puts in cx->num_cus (hipDeviceProp_t::multiProcessorCount; the same
    field is in srcnn_device_name's text, which guards the attribute's number)."""
    S.init(0)
    hip_path = next(line.split()[-1] for line in open("/proc/self/maps") if "libamdhip64" in line)
    hip = ctypes.CDLL(hip_path)
    v = ctypes.c_int(0)
    rc = hip.hipDeviceGetAttribute(ctypes.byref(v), HIP_ATTR_MULTIPROCESSOR_COUNT, S.lib().srcnn_context_device(0))
    assert rc == 0 and v.value > 0, (rc, v.value)
    named = int(re.search(r"(\d+) CUs\)", S.device_name()).group(1))
    assert v.value == named, (v.value, S.device_name())
    return BPC * v.value


_G = {}


def current_G():
    """(G, from the device?) once per process.  Without a visible device the CPU-side conditions are checked for an MI355X."""
    if not _G:
        import libsrcnn_amd as S
        try:
            have = S.lib().srcnn_device_count() > 0
        except Exception:                                   # noqa: BLE001 -- no library, no runtime: no device
            have = False
        _G["v"] = (device_G(S), True) if have else (G_MI355X, False)
        print("G = %d resident workgroups (%s)" % (_G["v"][0], "from the device" if _G["v"][1] else "no device visible: an MI355X's 256 CUs assumed"))
    return _G["v"]


# ---- running a case --------------------------------------------------------------------------------------------------------
def stage(S, p):
    """(source buffer, destination buffer with SLACK bytes behind the 32 planes) for one plane; nothing queued yet."""
    h, w = p.shape
    return S.DeviceBuffer.from_numpy(p), S.DeviceBuffer(32 * h * w * 4 + SLACK)


def fire(S, din, dout, h, w, stream):
    """Poison the whole destination and launch layers 1+2 behind it, both on `stream` (None = the null stream); no host sync."""
    hs = stream.handle if stream is not None else None
    S.check(S.lib().srcnn_memset_dev(dout.ptr, 0xFF, dout.nbytes, hs))
    S.check(S.lib().srcnn_conv12_f32_dev(din.ptr, w, h, dout.ptr, hs))


def collect(dout, h, w):
    return dout.to_numpy(np.float32, (32, h, w)), dout.to_numpy(np.uint8, (SLACK,), offset=32 * h * w * 4)


def compare(got, slack, want):
    """Counts, as the children report them: elements that differ under check()'s rule, the first of them, surviving poison, slack
    bytes that changed."""
    gb, wb = got.view(np.uint32), np.asarray(want).view(np.uint32)
    nan = np.isnan(want)
    bad = (np.isnan(got) != nan) | ((gb != wb) & ~nan)
    n = int(bad.sum())
    return {"differ": n, "first": [int(v) for v in np.argwhere(bad)[0]] if n else None, "of": int(bad.size),
            "poison": int((gb == POISON).sum()), "slack_changed": int((slack != 0xFF).sum())}


def clean(res):
    return res["differ"] == 0 and res["poison"] == 0 and res["slack_changed"] == 0


def run_one(S, p, want, stream=None):
    h, w = p.shape
    din, dout = stage(S, p)
    fire(S, din, dout, h, w, stream)
    stream.sync() if stream is not None else S.sync()
    got, slack = collect(dout, h, w)
    return compare(got, slack, want)


def run_back_to_back(S, planes, wants, stream, times=2):
    """`times` x: every plane's launch queued on `stream`, each into its own poisoned buffer, no host sync between them; one sync;
    then all are compared.  The queue's two counters have to come back to zero under a grid that changes from launch to launch."""
    out = []
    for _ in range(times):
        bufs = [stage(S, p) for p in planes]                 # allocation may drain the device: all of it before the first launch
        for p, (din, dout) in zip(planes, bufs):
            fire(S, din, dout, p.shape[0], p.shape[1], stream)
        stream.sync()
        out.append([compare(*collect(dout, p.shape[0], p.shape[1]), want) for p, (_din, dout), want in zip(planes, bufs, wants)])
    return out


# ---- CPU: the model and the conditions on the inputs ---------------------------------------------------------------------
def test_deal_model_for_an_mi355x():
    """deal() at G = 512 against the numbers the cases are named for, the three grid rules, and the 8K figure of the kernel's
    comment ("an 8K frame's 144 leftover tiles ... on 512 workgroups"): 7680 x 4320 is 120 x 270 = 32 400 tiles, 63 whole rounds
    of 512 leave 144 tiles = 576 quarter items."""
    G = 512
    assert deal(129, G, True) == (512, 0, 516)
    assert deal(511, G, True) == (512, 0, 2044) and deal(511, G, False) == (511, 511, 511)
    assert deal(512, G, True) == (512, 512, 512) == deal(512, G, False)
    assert deal(513, G, True) == (512, 512, 516) == deal(513, G, False)
    assert deal(1023, G, True) == (512, 512, 2556)
    assert deal(1024, G, True) == (512, 1024, 1024)
    assert deal(1025, G, True) == (512, 1024, 1028)
    assert deal(15, G, True) == (60, 0, 60)                 # the 70 x 130 planes of the directed tests: one item per workgroup
    assert deal(128, G, True) == (512, 0, 512)              # G / 4 tiles: the last count at which nobody runs a second item
    assert deal(3, G, True) == (12, 0, 12) and deal(1, G, True) == (4, 0, 4) and deal(3, G, False) == (3, 3, 3)
    n8k = (7680 // TILE_W) * (4320 // TILE_H)
    assert n8k == 32400
    grid, full, nitems = deal(n8k, G, True)
    assert (grid, n8k - full, nitems - full) == (512, 144, 576)
    src = open(os.path.join(ROOT, "libsrcnn_amd", "csrc", "srcnn_kernels.hip")).read()
    assert "an 8K frame's 144 leftover tiles" in src and "on 512 workgroups" in src
    assert re.search(r"constexpr int M_TW = %d, M_TH = 2 \* M_NW;" % TILE_W, src) and re.search(r"constexpr int M_NW = %d;" % (TILE_H // 2), src)
    assert re.search(r"constexpr int M_BPC = %d;" % BPC, src)


@pytest.mark.parametrize("g", [512, 2 * 304, 2 * 64])
def test_shapes_hit_their_class(g):
    """Every case's shape has the tile count it is chosen for and deals as its class says, at an MI355X's G and at two others."""
    G = g
    for name in CASES:
        h, w, n = shape_of(name, G)
        assert classify(name, G)[0] == n
        assert G != 512 or w * h <= 1.05e6, (name, w, h)
        assert (w - 1) % TILE_W >= 32 and (h - 1) % TILE_H >= 1, (name, w, h)      # the last quarter item stores something
    for name in SPREAD0_CASES:
        classify(name, G, spread=False)
    assert classify("B", G, spread=False)[1:] == (G - 1, G - 1, G - 1)
    tx = {tiles_x_for(shape_of(name, G)[2]) for name in MAIN}
    if G == 512:
        assert len(tx - {1}) >= 2 and 1 in tx, tx       # one, two, three and five tile columns over the set
        assert [shape_of(n, G)[:2] for n in ("F", "H")] == [(8192, 128), (3277, 293)]


@pytest.fixture(scope="module")
def G():
    return current_G()[0]


@pytest.fixture(scope="module")
def reference(oracle_lib, G):
    """{case: (plane, oracle conv2(conv1(plane)))}, the layer-2 body counts over the set and, per case, whether a tile repeats;
    computed once."""
    tiers = kernel_tiers()
    ref, repeats = {}, {}
    total = np.zeros((2, len(tiers) + 1), np.int64)
    for name in CASES:
        p = case_plane(name, G)
        c1 = oracle_lib.conv1(p)
        total += body_counts(c1, tiers)
        want = oracle_lib.conv2(c1)
        del c1
        want.setflags(write=False)
        p.setflags(write=False)
        d = tile_digests(want)
        repeats[name] = (len(d) - len(set(d)), len(d), bool(np.isnan(want).any()))
        ref[name] = (p, want)
    return ref, total, repeats


def test_inputs_distinguish_every_tile(reference, G):
    """CPU: the conditions on the inputs.  No two 64 x 16 tiles of a case's oracle planes are equal, the planes hold no NaN (so
    poison that survives is an unwritten sample), each case has as many tiles as its class needs, and layer 2 takes every body
    (full, T1, T2) of both blocks while the kernel loops."""
    _ref, total, repeats = reference
    for name, (rep, tiles, has_nan) in repeats.items():
        assert tiles == shape_of(name, G)[2], (name, tiles)
        assert rep == 0, "case %s: %d of %d tiles repeat another tile" % (name, rep, tiles)
        assert not has_nan, name
    print("segments by body [full, T1, T2, ...]: block 0 %s, block 1 %s" % (total[0].tolist(), total[1].tolist()))
    assert (total >= MIN_SEGMENTS).all(), total.tolist()


def test_compare_sees_poison_and_slack():
    """CPU: the counting the GPU tests and their children rely on."""
    want = np.arange(32 * 6, dtype=np.float32).reshape(32, 2, 3)
    slack = np.full(SLACK, 0xFF, np.uint8)
    assert clean(compare(want.copy(), slack, want))
    got = want.copy()
    got.view(np.uint32)[3, 1, 2] = POISON
    res = compare(got, slack, want)
    assert (res["differ"], res["first"], res["poison"]) == (1, [3, 1, 2], 1) and not clean(res)
    got = want.copy()
    got[0, 0, 0] = -0.0                                         # +0 expected: a sign alone is a difference
    assert compare(got, slack, want)["differ"] == 1
    slack[7] = 0
    assert compare(want.copy(), slack, want)["slack_changed"] == 1


# ---- GPU -------------------------------------------------------------------------------------------------------------------
def describe(names, G, spread=True):
    return "; ".join("%s (ntiles, grid, full, nitems) = %s" % (n, classify(n, G, spread)) for n in names)


def assert_clean(res, what):
    assert clean(res), "%s: %d of %d elements differ, first at %s; %d still poison; %d slack bytes changed" % (
        what, res["differ"], res["of"], res["first"], res["poison"], res["slack_changed"])


@pytest.fixture(scope="module")
def device(srcnn):
    """(G, from the device): the GPU tests refuse a G that was assumed."""
    g, from_device = current_G()
    assert from_device
    return g


@pytest.mark.gpu
@pytest.mark.parametrize("name", MAIN)
def test_default_instance_loops(srcnn, reference, device, name):
    """The library as loaded (by default the nested-tiers instance <0, true, true> with the tile queue) on each of the seven cases."""
    ref, _total, repeats = reference
    assert repeats[name][0] == 0 and not repeats[name][2]
    print("G = %d; %s" % (device, describe([name], device)))
    p, want = ref[name]
    assert_clean(run_one(srcnn, p, want), "case %s" % name)


@pytest.mark.gpu
def test_back_to_back_launches_reset_the_queue(srcnn, reference, device):
    """G+1, G/4+1, 3, 2G+1, 1 and G tiles queued on one stream with no host sync between them, then the same list once more:
    queue[0] / queue[1] reset themselves under a gridDim.x that changes from launch to launch."""
    ref, _total, _repeats = reference
    print("G = %d; %s" % (device, describe(B2B, device)))
    st = srcnn.Stream()
    try:
        rounds = run_back_to_back(srcnn, [ref[n][0] for n in B2B], [ref[n][1] for n in B2B], st)
    finally:
        st.destroy()
    for k, results in enumerate(rounds):
        for name, res in zip(B2B, results):
            assert_clean(res, "pass %d, case %s" % (k, name))


_CHILD = """
import sys
sys.path.insert(0, %(root)r)
sys.path.insert(0, %(tests)r)
import test_gpu_conv12_tile_loop as T
T.child_main(sys.argv[1])
"""


def child_main(spec_json):
    """A fresh process under the switches of spec["env"]: proves from debug_settings() that it runs what it names, regenerates the
    inputs, memory-maps the parent's oracle planes and prints one JSON line of counts."""
    import libsrcnn_amd as S
    spec = json.loads(spec_json)
    S.init(0)
    for kv in spec["expect"]:
        assert (kv + " ") in S.debug_settings(), (kv, S.debug_settings())
    G = device_G(S)
    assert G == spec["G"], (G, spec["G"])
    planes = {n: case_plane(n, G) for n in set(spec["cases"]) | set(spec["b2b"])}
    wants = {n: np.load(os.path.join(spec["dir"], n + ".npy"), mmap_mode="r") for n in planes}
    out = {"G": G, "cases": {n: run_one(S, planes[n], wants[n]) for n in spec["cases"]}}
    if spec["b2b"]:
        st = S.Stream()
        out["b2b"] = run_back_to_back(S, [planes[n] for n in spec["b2b"]], [wants[n] for n in spec["b2b"]], st, times=1)[0]
        st.destroy()
    print("RESULT " + json.dumps(out))


@pytest.fixture(scope="module")
def oracle_files(reference, tmp_path_factory):
    """save(name) -> the directory that holds <name>.npy, the case's oracle planes; each is written once for all children."""
    ref, _total, _repeats = reference
    d = str(tmp_path_factory.mktemp("conv12_tile_loop"))
    done = set()

    def save(name):
        if name not in done:
            np.save(os.path.join(d, name + ".npy"), ref[name][1])
            done.add(name)
        return d
    return save


def run_child(env, cases, b2b, G, oracle_files):
    for n in set(cases) | set(b2b):
        d = oracle_files(n)
    spec = {"dir": d, "cases": cases, "b2b": b2b, "G": G, "expect": ["%s=%s" % kv for kv in env.items()]}
    code = _CHILD % {"root": ROOT, "tests": os.path.join(ROOT, "tests")}
    r = subprocess.run([sys.executable, "-c", code, json.dumps(spec)], env=dict(os.environ, **env), capture_output=True, text=True, timeout=300)
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")]
    assert r.returncode == 0 and line, r.stdout + r.stderr
    return json.loads(line[-1][len("RESULT "):])


SWITCHES = [
    {"SRCNN_CONV12_QUEUE": "0"},                                 # the static-stride walk
    {"SRCNN_CONV12_DMA": "0"},                                   # load -> wait -> ds_write staging between two barriers
    {"SRCNN_CONV12_TIERS": "0"},                                 # the M_DEAD-only instance
    {"SRCNN_CONV12_PRUNE": "0"},                                 # the full body only
    {"SRCNN_CONV12_DMA": "0", "SRCNN_CONV12_QUEUE": "0"},
]


@pytest.mark.gpu
@pytest.mark.parametrize("env", SWITCHES, ids=lambda e: "+".join("%s=%s" % kv for kv in e.items()))
def test_other_instances_loop(reference, device, oracle_files, env):
    """Cases A, D and H in each other instance of the kernel, each in a fresh process (the switches are read at load); the
    SRCNN_CONV12_QUEUE=0 child also runs the back-to-back list."""
    b2b = B2B if env == {"SRCNN_CONV12_QUEUE": "0"} else []
    print("G = %d; %s" % (device, describe(SWITCH_CASES, device)))
    out = run_child(env, SWITCH_CASES, b2b, device, oracle_files)
    assert out["G"] == device
    for name in SWITCH_CASES:
        assert_clean(out["cases"][name], "%s, case %s" % (env, name))
    for name, res in zip(b2b, out.get("b2b", [])):
        assert_clean(res, "%s, back to back, case %s" % (env, name))
    assert len(out.get("b2b", [])) == len(b2b)


@pytest.mark.gpu
def test_without_spread(reference, device, oracle_files):
    """SRCNN_CONV12_SPREAD=0: G-1 tiles on G-1 workgroups, one whole tile each and no loop (case B), and the whole -> quarter
    switch of case D, which the switch does not touch."""
    print("G = %d; %s" % (device, describe(SPREAD0_CASES, device, spread=False)))
    out = run_child({"SRCNN_CONV12_SPREAD": "0"}, SPREAD0_CASES, [], device, oracle_files)
    for name in SPREAD0_CASES:
        assert_clean(out["cases"][name], "SRCNN_CONV12_SPREAD=0, case %s" % name)


# ---- through the whole path: a band launch, and the relaxed instance -----------------------------------------------------------
def conv12_tiles(dw, dh, r0, r1):
    """Tiles of the layer-1+2 launch behind output rows [r0, r1) of a dw x dh result: layer 3 needs the activations of 2 more
    rows on each interior side (y_path_halo of srcnn_y_path_geom.hpp)."""
    ca, cb = max(r0 - 2, 0), min(dh, r1 + 2)
    return -(-dw // TILE_W) * -(-(cb - ca) // TILE_H)


def frame_for(n, seed, rows_short=6):
    """An input plane whose 2x output has n layer-1+2 tiles: tiles_x columns with a ragged last one, the last tile row short."""
    tx = tiles_x_for(n)
    dw, dh = TILE_W * (tx - 1) + 38, TILE_H * (n // tx) - rows_short
    assert dw % 2 == 0 and dh % 2 == 0 and conv12_tiles(dw, dh, 0, dh) == n
    return content(dh // 2, dw // 2, seed)


@pytest.mark.gpu
def test_band_launch_loops(srcnn, oracle_lib, device):
    """One band of a frame whose layer-1+2 launch has G+1 tiles: out_row0, y_row_base and y_rows are all nonzero, so request()'s
    double clamp (to the image, then to the rows the band holds) and the stores' row offset run inside the loop.  The band starts
    at a row that is no multiple of 16, and the frame is about one tile row taller on each side."""
    n = device + 1
    tx = tiles_x_for(n)
    dw = TILE_W * (tx - 1) + 38
    row0 = TILE_H + 5
    rows = TILE_H * (n // tx) - 4 - 5                    # + 2 rows of halo on each side: n / tx tile rows, the last 5 rows short
    dh = row0 + rows + TILE_H + 2
    dh += dh % 2
    assert row0 % TILE_H != 0 and conv12_tiles(dw, dh, row0, row0 + rows) == n
    cls = deal(n, device, True)
    assert cls == (device, device, device + 4), cls
    print("G = %d; band rows [%d, %d) of %d x %d: (ntiles, grid, full, nitems) = %s" % (device, row0, row0 + rows, dw, dh, (n,) + cls))
    y = content(dh // 2, dw // 2, SEED + 401)
    want = oracle_lib.y_path(y)[row0:row0 + rows]
    assert not np.isnan(want).any()
    check(srcnn.y_upscale2x_band(y, row0, rows), want, "band of %d tiles" % n)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["D", "H"])
def test_relaxed_instance_loops(srcnn, oracle_lib, device, name):
    """SRCNN_MODE_FAST runs the relaxed instance <3, true, false> of the kernel.  Its bound (TOL_FAST of test_gpu_parity.py, applied
    as test_fast_modes_within_documented_bound applies it) is stated for the path's output, so the frame goes through the whole
    path, which has no poisoning hook: it is compared with the oracle under the bound AND, bit for bit, with the same frame
    assembled from bands of fewer than G/4 tiles each -- banding is documented bit-identical, and such bands never loop.  A
    dropped or misplaced tile misses either by orders of magnitude."""
    from test_gpu_parity import TOL_FAST
    S = srcnn
    n = CASES[name][0](device)
    cls = deal(n, device, True)
    assert cls == CASES[name][1](device, n), cls
    y = frame_for(n, SEED + 501 + ord(name))
    dh, dw = 2 * y.shape[0], 2 * y.shape[1]
    band = TILE_H * ((device // 4 - 1) // tiles_x_for(n)) - 4
    assert band >= TILE_H
    cuts = list(range(0, dh, band))
    for a in cuts:
        t = conv12_tiles(dw, dh, a, min(dh, a + band))
        assert t < device // 4 and deal(t, device, True) == (4 * t, 0, 4 * t), (a, t)      # one quarter item per workgroup
    print("G = %d; %d x %d: (ntiles, grid, full, nitems) = %s; %d bands of %d rows" % (device, dw, dh, (n,) + cls, len(cuts), band))
    want = oracle_lib.y_path(y)
    prev = S.set_mode(S.MODE_FAST)
    try:
        got = S.y_upscale2x(y)
        banded = np.concatenate([S.y_upscale2x_band(y, a, min(band, dh - a)) for a in cuts])
    finally:
        S.set_mode(prev)
    err = float(np.max(np.abs(got.astype(np.float64) - want)))
    print("SRCNN_MODE_FAST max|dY| = %.3g (bound %.1g)" % (err, TOL_FAST))
    assert err <= TOL_FAST, (name, err)
    assert err > 0.0                                    # the relaxed instance really ran
    check(got, banded, "SRCNN_MODE_FAST, case %s: whole frame against its bands" % name)
