#!/usr/bin/env python3
"""bench.py -- SRCNN Y-channel 2x throughput on MI355X (the metric BASELINE.json names).

    python bench.py [--gpus N] [--steps K] [--warmup W] [--frames F] [--full] [--dump-outputs DIR]
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 \
           --master-port P bench.py --gpus N --steps K --warmup W

A plain run sets up, warms up, times the K steps and prints the line: `value`, `ms_per_step`, the roofline of the
dominant kernel (from HIP events recorded inside the timed steps) and the HBM traffic of the committed profile.
Everything that takes runs of its own -- the CPU baseline, the other generator, the non-parity tiers, the PCIe-inclusive
stream, ProcessSRCNN wall times, BASELINE configs #2-#4, the event-timed and clock-probed steps, and at N > 1 the RCCL
probe -- runs only with --full.  --dump-outputs DIR writes a fixed sample of what the last timed step computed
(dump_outputs); the inputs are counter-based, so the same arguments give the same inputs in every run.

Workload ("step"): one pass of the hot path -- 2x Mitchell upscale + conv 9x9x1->64 + conv 1x1x64->32 +
conv 5x5x32->1, strict (bit-exact) mode -- over a batch of F synthetic 3840x2160 planar-float32 Y frames
per GPU, producing F 7680x4320 frames.  Inputs and outputs are resident in HBM for the whole timed
region.  Frames are independent, so ranks share nothing on the data path: each rank owns its own frames
(weak scaling); torch.distributed (gloo) is used only for the barriers and the max-over-ranks of the time.

One JSON line on rank 0.  `value` = output megapixels of ALL ranks / max-over-ranks wall time.
`roofline` is for the dominant kernel (layers 1+2, k_conv12_mfma): its average launch duration is measured
live inside the timed region with HIP events recorded on the launch stream by the library
(srcnn_profile_*), and priced with the algorithmic FLOPs per launch.
With --full: `cpu_baseline` = the reference's own OpenMP path (oracle/_ref, compiled from the reference sources) or the
C restatement (oracle/) timed on this host's cores, SURVEY.md 8(d) protocol: threads = min(physical cores, 64)
pinned with OMP_PROC_BIND=close OMP_PLACES=cores, best of 3, config #1 (ProcessSRCNN on the butterfly image) and
config #2 (one 1080p Y frame).  At N=1 the line also carries the rest of SURVEY 8(d): the PCIe-inclusive rate
(`pcie_inclusive`), the wall time of ProcessSRCNN itself -- the one number the reference's own harness prints
(src/test.cpp:653-672) -- for 1080p and 4K RGB (`process_srcnn_ms`), both synthetic generators (`generators`),
and the non-parity tiers with their measured error.
"""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

IN_W, IN_H = 3840, 2160                   # "4K" input frame; output 7680x4320
MAC_L12 = 64 * 81 + 32 * 64               # 7232 MAC per output pixel in the dominant kernel
MAC_ALL = MAC_L12 + 32 * 25               # 8032
PEAK_F32_TFLOPS = 157.3                   # MI355X_MICROARCH.md: FP32 matrix == FP32 vector peak
PEAK_HBM_GBS = 8000.0
METRIC = "megapixels/sec SRCNN Y-channel (2x upscale)"


def physical_cores():
    """Distinct (package, core) pairs of this host; falls back to the logical count."""
    try:
        seen, phys, core = set(), None, None
        for line in open("/proc/cpuinfo"):
            if line.startswith("physical id"):
                phys = line.split(":")[1].strip()
            elif line.startswith("core id"):
                core = line.split(":")[1].strip()
            elif not line.strip():
                if phys is not None and core is not None:
                    seen.add((phys, core))
                phys = core = None
        if seen:
            return len(seen)
    except OSError:
        pass
    return os.cpu_count() or 1


_CPU_CHILD = r"""
import json, os, sys, time
import numpy as np
sys.path.insert(0, sys.argv[1])
import oracle
from libsrcnn_amd import synth
budget, outdir = float(sys.argv[2]), sys.argv[3]
eng, kind = (oracle.Reference(), "reference") if oracle.have_reference() else (oracle.Oracle(), "port")
res = {"kind": kind}
t_all = time.perf_counter()
# config #1: ProcessSRCNN on the butterfly image (256x256x3 -> 512x512x3), best of 3
g = np.load(os.path.join(sys.argv[1], "tests", "golden", "butterfly.npz"))
ts = []
for _ in range(3):
    t0 = time.perf_counter(); rgb, conv = eng.process(g["rgb_in"], 2.0); ts.append(time.perf_counter() - t0)
res["config1_butterfly_processsrcnn_s"] = ts
res["config1_ok"] = bool(np.array_equal(rgb, g["rgb_out"]) and np.array_equal(conv, g["conv_y"]))
# config #2: one 1920x1080 Y frame -> 3840x2160 (falls back to a quarter frame if one run would blow the budget)
y = synth.plane(270, 480, synth.SEED0, "smooth")
t0 = time.perf_counter(); eng.y_path(y); probe = time.perf_counter() - t0
h, w = (1080, 1920) if probe * 16 * 3 <= budget else (540, 960)
y = synth.plane(h, w, synth.SEED0, "smooth")
ts = []
for _ in range(3):
    t0 = time.perf_counter(); out = eng.y_path(y); ts.append(time.perf_counter() - t0)
    if time.perf_counter() - t_all > budget:
        break
np.save(os.path.join(outdir, "cpu_out.npy"), out)
res.update({"config2_shape": [h, w], "config2_y_path_s": ts})
print(json.dumps(res))
"""


def cpu_baseline(S, budget_s=30.0):
    """The CPU-baseline leg (the only place bench.py touches oracle/): the reference CPU path in a child process
    whose OpenMP runtime is pinned as SURVEY 8(d) asks, then, on that same frame, the GPU output is compared with
    the CPU reference's (the "max |dY| vs CPU ref" half of the metric).  Returns (cpu_baseline object, max_abs_dY)."""
    from libsrcnn_amd import synth
    cores = physical_cores()
    threads = min(cores, 64)          # layer 1 has 64 parallel iterations, layer 2 has 32 (src/libsrcnn.cpp:791,817)
    env = dict(os.environ, OMP_NUM_THREADS=str(threads), OMP_PROC_BIND="close", OMP_PLACES="cores")
    with tempfile.TemporaryDirectory() as td:
        r = subprocess.run([sys.executable, "-c", _CPU_CHILD, ROOT, str(budget_s), td], env=env, capture_output=True,
                           text=True, timeout=budget_s * 4 + 60)
        if r.returncode != 0:
            raise RuntimeError("cpu baseline child failed: " + r.stderr[-400:])
        res = json.loads(r.stdout.strip().splitlines()[-1])
        ref_out = np.load(os.path.join(td, "cpu_out.npy"))
    h, w = res["config2_shape"]
    best2 = min(res["config2_y_path_s"])
    best1 = min(res["config1_butterfly_processsrcnn_s"])
    y = synth.plane(h, w, synth.SEED0, "smooth")
    gpu_out = S.y_upscale2x(y)
    max_abs = float(np.max(np.abs(gpu_out.astype(np.float64) - ref_out.astype(np.float64))))
    obj = {"value": round(4 * h * w / 1e6 / best2, 4), "unit": "MPix/s", "cores": threads, "kind": res["kind"],
           "sample": "config #2: one synthetic %dx%d -> %dx%d Y frame, best of %d runs %.2f s; OMP_NUM_THREADS=%d = "
                     "min(physical cores %d, 64), OMP_PROC_BIND=close OMP_PLACES=cores (layer 1 has 64 parallel "
                     "iterations, layer 2 has 32: src/libsrcnn.cpp:791,817); GPU output of the same frame compared "
                     "element-wise" % (w, h, 2 * w, 2 * h, len(res["config2_y_path_s"]), best2, threads, cores),
           "physical_cores": cores, "logical_cpus": os.cpu_count(),
           "config2_runs_s": [round(t, 3) for t in res["config2_y_path_s"]],
           "config1_butterfly_processsrcnn_ms": round(best1 * 1e3, 1),
           "config1_runs_ms": [round(t * 1e3, 1) for t in res["config1_butterfly_processsrcnn_s"]],
           "config1_matches_reference_pngs": res["config1_ok"]}
    return obj, max_abs


def synth_rgb(h, w, seed):
    from libsrcnn_amd import synth
    base = synth.plane(h, w, seed, "smooth")
    rng = np.random.default_rng(seed & 0xFFFF)
    img = np.empty((h, w, 3), np.uint8)
    for k in range(3):
        img[..., k] = np.clip(base * (0.6 + 0.2 * k) + rng.integers(0, 24, base.shape), 0, 255).astype(np.uint8)
    return img


def process_srcnn_wall(S):
    """Wall time of ProcessSRCNN(rgb, x2) -- host u8 in, new[]-allocated host u8 out, as a libsrcnn user calls it
    (and as the reference's harness times it, src/test.cpp:653-672).  Best of 5 after one warm-up."""
    import ctypes as C
    L = S.lib()
    S.ConfigureFilterSRCNN(S.SRCNNF_Bicubic, False)
    fn = getattr(L, S.CXX_SYMBOLS[1])
    out = {}
    for name, (h, w) in (("1920x1080_rgb", (1080, 1920)), ("3840x2160_rgb", (2160, 3840))):
        img = synth_rgb(h, w, 0x5C0DE000 + h)
        ts, cs = [], []
        for it in range(6):
            o, osz = C.c_void_p(), C.c_uint(0)
            c0 = time.process_time()
            t0 = time.perf_counter()
            rc = fn(img.ctypes.data, w, h, 3, 2.0, C.byref(o), C.byref(osz), None, None)
            dt = time.perf_counter() - t0
            dc = time.process_time() - c0
            assert rc == 0 and osz.value == 4 * h * w * 3, (rc, osz.value)
            L.srcnn_delete_array(o)
            if it:
                ts.append(dt)
                cs.append(dc)
        out[name] = {"best_ms": round(min(ts) * 1e3, 2), "median_ms": round(sorted(ts)[len(ts) // 2] * 1e3, 2),
                     "MPix/s": round(4 * h * w / 1e6 / min(ts), 1),
                     "host_cpu_ms_per_call": round(sorted(cs)[len(cs) // 2] * 1e3, 2)}
        ph = (C.c_double * 8)()
        mhz_in_call = None
        if h >= 2160:
            # one more call with the in-kernel clock probe on (include/srcnn_amd_debug.h): the shader clock every layer-1+2 launch of
            # the call ran at -- the same kernels run at ~2.35 GHz in the resident loop (`resident_layer12_mhz` below)
            S.clock_probe(True)
            o, osz = C.c_void_p(), C.c_uint(0)
            rc = fn(img.ctypes.data, w, h, 3, 2.0, C.byref(o), C.byref(osz), None, None)
            recs = S.clock_read(0)
            S.clock_probe(False)
            L.srcnn_delete_array(o)
            if rc == 0 and recs:
                mhz_in_call = [round(float(m)) for m, _us in recs]
        if L.srcnn_debug_process_phases(ph, 8) >= 6 and h >= 2160:
            # where the LAST call's time went (include/srcnn_amd_debug.h): milliseconds since the call's work began
            out[name]["phases_ms_last_call"] = {
                "call_ms": round(ts[-1] * 1e3, 2), "setup_done": round(ph[0], 2), "first_band_queued": round(ph[1], 2),
                "last_kernels_done": round(ph[2], 2), "last_band_landed": round(ph[3], 2), "fanned_out": round(ph[4], 2),
                "bands": int(ph[5]),
                "layer12_shader_mhz_per_band": mhz_in_call,
                "note": "device busy from first_band_queued to last_kernels_done; before it: lane lease, tables, the first band's "
                        "stage-in (memcpy into page-locked staging + H2D); after it: the last band's D2H and its copy into the "
                        "caller's fresh new[] block"}
    # The same image through the C ABI's srcnn_process_u8 into a caller-owned, REUSED result buffer: what a caller that
    # upscales a sequence should use -- no fresh 100 MB of pages per call (tools/concurrent_probe.py has the multi-caller runs).
    h, w = 2160, 3840
    img = synth_rgb(h, w, 0x5C0DE100)
    res = np.empty((2 * h, 2 * w, 3), np.uint8)
    ts = []
    for it in range(9):
        t0 = time.perf_counter()
        rc = L.srcnn_process_u8(img.ctypes.data, w, h, 3, 2.0, 2, res.ctypes.data, None)
        dt = time.perf_counter() - t0
        assert rc == 0, rc
        if it:
            ts.append(dt)
    out["3840x2160_rgb_reused_result_buffer"] = {
        "best_ms": round(min(ts) * 1e3, 2), "median_ms": round(sorted(ts)[len(ts) // 2] * 1e3, 2),
        "MPix/s": round(4 * h * w / 1e6 / min(ts), 1),
        "note": "srcnn_process_u8: host u8 RGB in -> caller-owned, reused host u8 RGB out, calls back to back"}
    # Round 4: a SEQUENCE of images the way a caller that owns its buffers should run it -- page-locked source and result
    # (srcnn_host_alloc_pinned: no staging memcpy, no fan-out) and two asynchronous jobs in flight whose kernels are chained
    # on the device (srcnn_process_u8_begin / _wait): milliseconds per image over 16 images.
    pin_img = S.PinnedArray(img.shape)
    pin_img.array[...] = img
    pins = [S.PinnedArray(res.shape), S.PinnedArray(res.shape)]
    try:
        ts = []
        for it in range(7):
            t0 = time.perf_counter()
            rc = L.srcnn_process_u8(pin_img.array.ctypes.data, w, h, 3, 2.0, 2, pins[0].array.ctypes.data, None)
            dt = time.perf_counter() - t0
            assert rc == 0, rc
            if it:
                ts.append(dt)
        out["3840x2160_rgb_page_locked_buffers"] = {
            "best_ms": round(min(ts) * 1e3, 2), "median_ms": round(sorted(ts)[len(ts) // 2] * 1e3, 2),
            "MPix/s": round(4 * h * w / 1e6 / min(ts), 1),
            "note": "srcnn_process_u8, source and result allocated with srcnn_host_alloc_pinned, blocking calls back to back"}
        same = bool(np.array_equal(pins[0].array, res))
        def sequence(n_img):
            jobs = []
            t0 = time.perf_counter()
            for i in range(n_img):
                j = C.c_void_p()
                rc = L.srcnn_process_u8_begin(pin_img.array.ctypes.data, w, h, 3, 2.0, 2, pins[i & 1].array.ctypes.data, None, C.byref(j))
                assert rc == 0, rc
                jobs.append(j)
                if len(jobs) == 2:
                    assert L.srcnn_process_u8_wait(jobs.pop(0)) == 0
            while jobs:
                assert L.srcnn_process_u8_wait(jobs.pop(0)) == 0
            return (time.perf_counter() - t0) / n_img
        # Round 5: the figure used to be ONE cold sequence of 16 images, and it came out 10.2 or 12.4 ms depending on the box:
        # the second job in flight needs a second lane (streams, scratch, staging), which the blocking calls before it never
        # created -- tens of milliseconds of one-off allocation inside a 160 ms measurement.  Now: the first sequence is
        # reported as what it is (cold), then three more; the figure is their best, the spread is in the line.
        n_img = 16
        cold = sequence(n_img)
        warm = [sequence(n_img) for _ in range(3)]
        per = min(warm)
        out["3840x2160_rgb_async_sequence"] = {
            "ms_per_image": round(per * 1e3, 2), "MPix/s": round(4 * h * w / 1e6 / per, 1), "images": n_img,
            "sequences_ms_per_image": [round(t * 1e3, 2) for t in warm], "first_cold_sequence_ms_per_image": round(cold * 1e3, 2),
            "results_equal_blocking_call": bool(same and np.array_equal(pins[1].array, res) and np.array_equal(pins[0].array, res)),
            "note": "srcnn_process_u8_begin/_wait, two jobs in flight, kernels chained on the device, page-locked buffers; best of "
                    "three 16-image sequences after one cold sequence (which creates the second lane: streams, scratch, staging)"}
    finally:
        pin_img.free()
        for p in pins:
            p.free()
    out["note"] = "host u8 RGB in -> host u8 RGB out through the drop-in symbol; includes H2D, colour split, chroma " \
                  "resample, Y path, merge, D2H and the new[] of the result"
    return out


def pcie_inclusive(S, frames=16):
    """Stream of host-resident (page-locked) 4K Y frames: H2D + path + D2H per frame, two slots; with the per-slot hipGraph
    replay BASELINE config #5 names, and with plain launches (same kernels, same overlap)."""
    w, h, F = IN_W, IN_H, frames

    def variant(use_graph):
        step, free = host_stream_setup(S, frames, use_graph)
        step()                                                   # warm-up (+ capture)
        step()
        ts, cs = [], []
        for _ in range(3):
            c0 = time.process_time()
            t0 = time.perf_counter()
            step()
            ts.append(time.perf_counter() - t0)
            cs.append(time.process_time() - c0)
        free()
        return {"MPix/s": round(F * 4 * w * h / 1e6 / min(ts), 1), "wall_s_per_frame": round(min(ts) / F, 6),
                "host_cpu_s_per_frame": round(min(cs) / F, 6)}
    eager, graph = variant(0), variant(2)
    auto = variant(1)
    g, p, fell = S.stream_mode()
    auto["last_call_frames_replayed_from_graph"], auto["last_call_frames_launched_plainly"], auto["fell_back_to_plain_launches"] = g, p, bool(fell) or p == F
    return {"value": graph["MPix/s"], "unit": "MPix/s", "frames": F, "best_of": 3,
            "use_graph_auto": auto,
            "bytes_per_output_px": {"h2d": 1.0, "d2h": 4.0},
            "host_cpu_s_per_frame": graph["host_cpu_s_per_frame"], "wall_s_per_frame": graph["wall_s_per_frame"],
            "plain_launches": eager,
            "note": "planar f32 Y frames in page-locked host memory, H2D + path + D2H overlapped over two slots "
                    "(srcnn_y_upscale2x_f32_stream); `value` = with one hipGraph per slot as BASELINE config #5 asks (use_graph = 2: "
                    "replay insisted on), `plain_launches` = the same stream without graphs (use_graph = 0), `use_graph_auto` = use_graph "
                    "= 1: replay kept only while its host CPU cost stays below SRCNN_GRAPH_MAX_CPU_PCT of a frame, otherwise plain "
                    "launches.  host_cpu_s_per_frame = process CPU time (all "
                    "threads) per frame: the library's threads sleep or poll; with graph replay a thread of the ROCm "
                    "runtime stays busy from launch to completion (tools/runtime_thread_probe.py).  Never the headline value"}


_CONFIG2_CHILD = r"""
import json, sys, time
t_start = time.perf_counter()
sys.path.insert(0, sys.argv[1])
import numpy as np
import libsrcnn_amd as S
from libsrcnn_amd import synth
t0 = time.perf_counter(); S.init(0); init_ms = (time.perf_counter() - t0) * 1e3
L = S.lib()
w, h = 1920, 1080
y = synth.plane(h, w, synth.SEED0, "smooth")
# (a) what a caller with host memory sees: pageable float32 in -> pageable float32 out, blocking
t0 = time.perf_counter(); out = S.y_upscale2x(y); cold_host = (time.perf_counter() - t0) * 1e3
warm_host = []
for _ in range(15):
    t0 = time.perf_counter(); out = S.y_upscale2x(y); warm_host.append((time.perf_counter() - t0) * 1e3)
# (b) resident: device pointer in -> device pointer out, call + device sync
d_in = S.DeviceBuffer.from_numpy(y); d_out = S.DeviceBuffer(4 * w * h * 4)
S.sync()
warm_dev = []
for _ in range(30):
    t0 = time.perf_counter(); S.check(L.srcnn_y_upscale2x_f32_dev(d_in.ptr, w, h, d_out.ptr, None)); S.sync()
    warm_dev.append((time.perf_counter() - t0) * 1e3)
warm_host.sort(); warm_dev.sort()
print(json.dumps({"init_ms": init_ms, "cold_first_call_host_ms": cold_host, "warm_host_median_ms": warm_host[len(warm_host) // 2],
                  "warm_host_min_ms": warm_host[0], "warm_resident_median_ms": warm_dev[len(warm_dev) // 2],
                  "warm_resident_min_ms": warm_dev[0], "process_start_to_first_result_ms": None}))
"""


def baseline_configs(S):
    """BASELINE.json configs #2, #3 and #4 on this one GPU, each with the reference's own yardstick -- the wall time of the
    call (src/test.cpp:653-672) -- outside the contract's timed region.
    #2 runs in a fresh child process, so that `cold_first_call` really is the first call of a process (context, streams,
    scratch, the resample table); #3 and #4 run here.  #4 goes through the RCCL entry point at world 1."""
    import ctypes as C
    from libsrcnn_amd import synth, multigpu
    L = S.lib()
    out = {}
    r = subprocess.run([sys.executable, "-c", _CONFIG2_CHILD, ROOT], capture_output=True, text=True, timeout=300)
    if r.returncode == 0:
        c2 = json.loads(r.stdout.strip().splitlines()[-1])
        n = 4 * 1920 * 1080 / 1e6
        out["2_single_1080p_frame"] = {
            "shape": "1920x1080 -> 3840x2160 Y, strict",
            "cold_first_call_ms": round(c2["cold_first_call_host_ms"], 2),
            "device_init_ms": round(c2["init_ms"], 1),
            "warm_median_ms": round(c2["warm_host_median_ms"], 3), "warm_min_ms": round(c2["warm_host_min_ms"], 3),
            "warm_resident_median_ms": round(c2["warm_resident_median_ms"], 3),
            "warm_resident_min_ms": round(c2["warm_resident_min_ms"], 3),
            "MPix/s_warm_resident": round(n / (c2["warm_resident_median_ms"] * 1e-3), 1),
            "note": "fresh process; cold_first_call / warm_median: srcnn_y_upscale2x_f32 on pageable host float32 in and out "
                    "(H2D + path + D2H, blocking; the first call also page-locks the 2 x 16 MB bounce slots pageable memory travels "
                    "through and allocates the device scratch); warm_resident: device pointers, call + device sync; device_init = "
                    "srcnn_init (its first touch of the device loads the code object: 50-250 ms by box)"}
    else:
        out["2_single_1080p_frame"] = {"error": r.stderr[-300:]}
    # #3: batch of 64 resident 1080p frames, one call per step
    w, h, F = 1920, 1080, 64
    d_in = S.DeviceBuffer(F * w * h * 4)
    d_out = S.DeviceBuffer(F * 4 * w * h * 4)
    two = synth.frames(2, h, w, 0, "smooth")
    for f in range(F):
        d_in.upload(two[f & 1], offset=f * w * h * 4)

    def step3():
        S.check(L.srcnn_y_upscale2x_f32_batch_dev(d_in.ptr, w, h, F, d_out.ptr, None))
    step3(); S.sync()
    ts = []
    for _ in range(3):
        t0 = time.perf_counter(); step3(); S.sync(); ts.append(time.perf_counter() - t0)
    out["3_batch_64x1080p"] = {"shape": "64 x (1920x1080 -> 3840x2160) resident, one call", "ms_per_batch": round(min(ts) * 1e3, 2),
                               "MPix/s": round(F * 4 * w * h / 1e6 / min(ts), 1), "best_of": 3}
    del d_in, d_out
    # #4: one 7680x4320 frame -> 15360x8640 through the multi-GPU entry point (RCCL communicator of ONE rank here: the band
    # plan, the piece loop and the comm stream run; ncclSend/ncclRecv have no peer to talk to)
    try:
        w, h = 7680, 4320
        d_in = S.DeviceBuffer.from_numpy(synth.plane(h, w, synth.SEED0, "smooth"))
        multigpu.init_comm_from_torch_dist(None, 0, 1)
        tiled = multigpu.TiledFrameGPU(w, h, 0, 1, nsub=4)

        def step4():
            tiled.step(d_in)
            S.check(L.srcnn_comm_wait(None))
            S.sync()
        step4()
        ts = []
        for _ in range(3):
            t0 = time.perf_counter(); step4(); ts.append(time.perf_counter() - t0)
        out["4_tiled_8k_frame_world1"] = {"shape": "7680x4320 -> 15360x8640 via srcnn_comm_tiled_y_upscale2x_f32_dev, world 1, 4 pieces",
                                          "ms_per_frame": round(min(ts) * 1e3, 2), "MPix/s": round(4 * w * h / 1e6 / min(ts), 1),
                                          "best_of": 3}
        del tiled, d_in
        L.srcnn_comm_destroy()
    except Exception as e:                                        # noqa: BLE001
        out["4_tiled_8k_frame_world1"] = {"error": repr(e)}
    return out


def roofline_all(stage_ms, n_out, in_px):
    """Every kernel of the strict path against ITS OWN bound: achieved, the peak or floor it is held to,
    and the fraction.  stage_ms = device time per 4K -> 8K frame (all of its launches: a frame is one band under the default scratch cap, more under a lower one) from the HIP
    events of the timed region."""
    CLK = 2.4e9
    SIMDS = 256 * 4
    rows = []
    if stage_ms.get("conv12"):
        ms = stage_ms["conv12"]
        tf = 2.0 * MAC_L12 * n_out / (ms * 1e-3) / 1e12
        # strict tap-step floor measured by tools/ubench/occupancy_tapstep.hip: 70 cycles per 1024 MAC and SIMD
        floor_ms = (MAC_L12 * n_out / 1024.0) * 70.0 / SIMDS / CLK * 1e3
        rows.append({"kernel": "k_conv12_mfma", "bound": "mfma", "achieved": round(tf, 2), "peak": PEAK_F32_TFLOPS, "unit": "TFLOP/s",
                     "frac": round(tf / PEAK_F32_TFLOPS, 4), "ms_per_frame": round(ms, 4),
                     "own_floor": {"what": "no-FMA ceiling (product and sum rounded separately): 0.5 of peak; measured floor of the "
                                           "MFMA-product + VALU-sum step: 70 cycles per 1024 MAC per SIMD at 2.4 GHz "
                                           "(profiles/r06_occupancy_tapstep.txt)",
                                   "frac_of_no_fma_ceiling": round(tf / (PEAK_F32_TFLOPS / 2), 4),
                                   "floor_ms": round(floor_ms, 3), "frac_of_floor": round(floor_ms / ms, 4)}})
    if stage_ms.get("conv3"):
        ms = stage_ms["conv3"]
        tf = 2.0 * 800 * n_out / (ms * 1e-3) / 1e12
        # per wave (64 lanes x 4 pixels) and channel: 50 v_pk_mul_f32 + 104 v_cvt_f64_f32 + 100 v_add_f64 = 254 instructions at the
        # 4.14 cycles per instruction of the same mix in a register-only stream (profiles/r03_valu_rates.txt, "conv3 pair")
        floor_ms = (n_out / 256.0) * 32 * 254 * 4.14 / SIMDS / CLK * 1e3
        rows.append({"kernel": "k_conv3", "bound": "valu", "achieved": round(tf, 2), "peak": PEAK_F32_TFLOPS, "unit": "TFLOP/s",
                     "frac": round(tf / PEAK_F32_TFLOPS, 4), "ms_per_frame": round(ms, 4),
                     "own_floor": {"what": "fp64-rate VALU issue: per MAC one half v_pk_mul_f32, one v_cvt_f64_f32 and one v_add_f64 "
                                           "(the reference rounds the product to fp32, then sums in fp64); 254 instructions per wave "
                                           "and channel at the mix's measured 4.14 cycles each (profiles/r03_valu_rates.txt), 2.4 GHz",
                                   "floor_ms": round(floor_ms, 3), "frac_of_floor": round(floor_ms / ms, 4)}})
    if stage_ms.get("resample"):
        ms = stage_ms["resample"]
        nbytes = 4.0 * in_px + 4.0 * n_out
        gbs = nbytes / (ms * 1e-3) / 1e9
        rows.append({"kernel": "k_rs2d_dma", "bound": "hbm", "achieved": round(gbs, 1), "peak": PEAK_HBM_GBS, "unit": "GB/s",
                     "frac": round(gbs / PEAK_HBM_GBS, 4), "ms_per_frame": round(ms, 4),
                     "own_floor": {"what": "algorithmic bytes: fp32 source plane in + fp32 2x plane out", "bytes_per_launch": nbytes,
                                   "floor_ms": round(nbytes / (PEAK_HBM_GBS * 1e9) * 1e3, 4),
                                   "frac_of_floor": round(nbytes / (PEAK_HBM_GBS * 1e9) * 1e3 / ms, 4)}})
    return rows


_RESULT_FD = None


def claim_stdout():
    """The contract is ONE line on stdout.  Libraries print there too (gloo's "[Gloo] Rank 0 is connected to ..." under
    torch.distributed.run, RCCL/ROCm notices): from here on fd 1 of this rank IS stderr, and only emit() writes to the
    real stdout."""
    global _RESULT_FD
    if _RESULT_FD is None:
        sys.stdout.flush()
        _RESULT_FD = os.dup(1)
        os.dup2(2, 1)


def emit(line):
    data = (line + "\n").encode()
    fd = _RESULT_FD if _RESULT_FD is not None else 1
    sys.stdout.flush()
    while data:
        data = data[os.write(fd, data):]


def _free_port():
    import socket
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def launch_ranks(n, argv):
    """`python bench.py --gpus N` without a launcher: start N rank processes ourselves.

    The parent NEVER touches the GPU (it does not even load libsrcnn_amd.so): every rank is a fresh child created
    with subprocess -- no exec from a process that has initialised HIP -- with the RANK / LOCAL_RANK / WORLD_SIZE /
    MASTER_* environment torch.distributed.run would have given it.  Rank 0's stdout carries the single JSON line,
    which the parent relays; the other ranks' stdout goes to stderr.  Exit code = first failing rank's, and a
    failed rank takes the others down (by PID) instead of leaving them blocked in a barrier."""
    port = int(os.environ.get("MASTER_PORT", "0")) or _free_port()
    procs = []
    for r in range(n):
        env = dict(os.environ, RANK=str(r), LOCAL_RANK=str(r), WORLD_SIZE=str(n), LOCAL_WORLD_SIZE=str(n),
                   MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), HSA_ENABLE_IPC_MODE_LEGACY=os.environ.get("HSA_ENABLE_IPC_MODE_LEGACY", "0"))
        procs.append(subprocess.Popen([sys.executable, os.path.abspath(__file__)] + list(argv), env=env,
                                      stdout=subprocess.PIPE if r == 0 else sys.stderr, text=(r == 0) or None))
    rc = 0
    out0 = ""
    try:
        pending = set(range(n))
        import threading
        box = {}
        t0 = threading.Thread(target=lambda: box.setdefault("out", procs[0].stdout.read()), daemon=True)
        t0.start()
        while pending:
            for r in sorted(pending):
                code = procs[r].poll()
                if code is None:
                    continue
                pending.discard(r)
                if code != 0 and rc == 0:
                    rc = code
                    print("bench.py: rank %d exited with %d; stopping the other ranks" % (r, code), file=sys.stderr)
                    for o in pending:
                        procs[o].terminate()
            time.sleep(0.05)
        t0.join(timeout=10)
        out0 = box.get("out", "") or ""
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
    lines = [ln for ln in out0.splitlines() if ln.startswith("{")]
    for ln in out0.splitlines():
        if not ln.startswith("{"):
            print(ln, file=sys.stderr)
    if lines:
        print(lines[-1], flush=True)
    elif rc == 0:
        rc = 3
        print("bench.py: rank 0 printed no result line", file=sys.stderr)
    return rc


def rendezvous(args):
    """RANK / LOCAL_RANK / WORLD_SIZE from the environment (torch.distributed.run or launch_ranks) and, for N > 1, a
    gloo process group: CPU-side only (barriers, max of a scalar, the RCCL id).  The data path of the headline
    workload has no collective, and each process drives its GPU through libsrcnn_amd.so's own HIP runtime."""
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if world != args.gpus:
        args.gpus = world
    dist = None
    if world > 1:
        import torch.distributed as dist
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        dist.init_process_group("gloo", rank=rank, world_size=world)
    return rank, local_rank, world, dist


def reduce_max(dist, x):
    if dist is None:
        return x
    import torch
    t = torch.tensor([x], dtype=torch.float64)
    dist.all_reduce(t, op=dist.ReduceOp.MAX)
    return float(t[0])


def gather_per_rank(dist, world, x):
    """Every rank's own figure, in rank order (so a straggler shows): a list on every rank."""
    if dist is None or world == 1:
        return [round(float(x), 4)]
    box = [None] * world
    dist.all_gather_object(box, round(float(x), 4))
    return box


def reduce_min(dist, x):
    return -reduce_max(dist, -x)


_RCCL_WEDGED = False       # a probe thread is stuck inside RCCL: leave with os._exit once the line is out (see leave())


def leave():
    """Normal return, unless a helper thread is wedged inside RCCL: then interpreter shutdown (atexit handlers, library
    destructors) could wait for it for ever, so the process ends here, after flushing what it printed."""
    if _RCCL_WEDGED:
        sys.stdout.flush()
        sys.stderr.flush()
        os._exit(0)


def rccl_probe(S, dist, rank, world, ndev, timeout_s=120.0):
    """Outside the timed region: create the RCCL communicator inside libsrcnn_amd.so across all ranks and run ONE
    srcnn_comm_barrier, so the line can say how many ranks RCCL actually connected (`rccl_ranks`).  The id travels
    over gloo in the main thread; init + barrier run in a helper thread with a deadline so that a wedged fabric
    costs the line its `rccl_ranks`, never the measurement (the headline data path has no collective).
    Returns (nranks or None, note or None)."""
    import ctypes as C
    import threading
    L = S.lib()
    timeout_s = float(os.environ.get("SRCNN_BENCH_RCCL_TIMEOUT", timeout_s))
    if world > ndev and not os.environ.get("SRCNN_BENCH_FORCE_RCCL_PROBE"):
        return None, "%d ranks alias %d device(s): RCCL refuses two ranks on one device, so no communicator was made" % (world, ndev)
    ident = (C.c_ubyte * 128)()
    ok = 1.0
    if rank == 0:
        ok = 1.0 if L.srcnn_comm_unique_id(ident) == 0 else 0.0
    if dist is not None:
        box = [bytes(ident) if ok else None]
        dist.broadcast_object_list(box, src=0)
        if box[0] is None:
            return None, "srcnn_comm_unique_id failed on rank 0"
        ident = (C.c_ubyte * 128).from_buffer_copy(box[0])
    elif not ok:
        return None, "srcnn_comm_unique_id failed: " + L.srcnn_last_error().decode()
    res = {}

    def work():
        try:
            if os.environ.get("SRCNN_BENCH_FAKE_RCCL_HANG"):        # test hook: a fabric that never answers
                time.sleep(1e6)
            S.check(L.srcnn_comm_init(ident, rank, world))
            S.check(L.srcnn_comm_barrier(None))
            r, n = C.c_int(-1), C.c_int(-1)
            S.check(L.srcnn_comm_rank(C.byref(r), C.byref(n)))
            res["n"] = n.value
        except Exception as e:                                   # noqa: BLE001
            res["err"] = repr(e)
    th = threading.Thread(target=work, daemon=True)
    th.start()
    th.join(timeout_s)
    mine = float(res.get("n", 0))
    agreed = reduce_min(dist, mine)                              # every rank must have seen the same communicator
    if th.is_alive():
        global _RCCL_WEDGED
        _RCCL_WEDGED = True
        return None, "RCCL init/barrier did not finish within %.0f s on rank %d" % (timeout_s, rank)
    if agreed != world:
        return None, res.get("err", "RCCL connected %d of %d ranks" % (int(agreed), world))
    return int(agreed), None


def host_stream_setup(S, frames, use_graph=1):
    """Page-locked 4K frames for the PCIe-inclusive stream (BASELINE config #5): returns (step, free)."""
    import ctypes as C
    from libsrcnn_amd import synth
    L = S.lib()
    w, h, F = IN_W, IN_H, frames
    pin_in = L.srcnn_host_alloc_pinned(F * w * h * 4)
    pin_out = L.srcnn_host_alloc_pinned(F * 4 * w * h * 4)
    if not pin_in or not pin_out:
        raise RuntimeError("pinned allocation failed: " + L.srcnn_last_error().decode())
    fr = np.ctypeslib.as_array(C.cast(pin_in, C.POINTER(C.c_float)), (F, h, w))
    two = synth.frames(2, h, w, 0, "smooth")
    for f in range(F):
        fr[f] = two[f & 1]

    def step():
        S.check(L.srcnn_y_upscale2x_f32_stream(pin_in, w, h, F, pin_out, use_graph))

    def free():
        L.srcnn_host_free_pinned(pin_in); L.srcnn_host_free_pinned(pin_out)
    return step, free


def side_workload(args):
    """The other BASELINE.json configurations.  Same timing protocol (barrier + device sync on both sides of the timed
    steps, max over ranks, whole-job aggregate); reported with the same keys but they are NOT the headline line the
    driver records (that is --workload frames)."""
    rank, local_rank, world, dist = rendezvous(args)
    if args.dry_run:
        return dry_run_line(args, rank, world, dist)
    import libsrcnn_amd as S
    from libsrcnn_amd import synth, multigpu
    ndev = max(1, S.device_count())
    S.init(local_rank % ndev)
    L = S.lib()
    extra = {}

    def barrier():
        if dist is not None:
            dist.barrier()

    verify = None
    cleanup = None
    cpu0 = None
    if args.workload == "tiled8k":
        import hashlib
        stand_in = os.environ.get("SRCNN_RCCL_LIB")
        if stand_in:
            # a rehearsal, not a measurement of xGMI: the ranks alias one device and move their bands through the test-suite's
            # RCCL stand-in (tests/rccl_double) -- what it shows is that the N > 1 choreography runs and assembles the right frame
            extra["rccl_library"] = stand_in
            extra["ranks_alias_devices"] = world > ndev
        if world > ndev and not stand_in:
            # the band gather is a real RCCL exchange, and RCCL refuses two ranks on one device
            if rank == 0:
                print("bench.py: --workload tiled8k needs one GPU per rank (%d ranks, %d device(s) visible)" % (world, ndev), file=sys.stderr)
            barrier()
            if dist is not None:
                dist.destroy_process_group()
            sys.exit(4)
        w, h = args.tiled_size
        y = synth.plane(h, w, synth.SEED0, "smooth")          # every rank can generate the frame (counter-based)
        d_in = S.DeviceBuffer.from_numpy(y)
        multigpu.init_comm_from_torch_dist(dist, rank, world)
        tiled = multigpu.TiledFrameGPU(w, h, rank, world, nsub=args.sub_bands)
        extra["rccl_ranks"] = world
        extra["sub_bands"] = tiled.nsub

        def step():
            tiled.step(d_in)

        def verify():
            """Once per run: the gathered frame on the root must be the whole-frame result, bit for bit."""
            if rank != 0:
                return None
            got = hashlib.sha256(tiled.result().tobytes()).hexdigest()
            d_ref = S.DeviceBuffer(4 * w * h * 4)
            S.check(L.srcnn_y_upscale2x_f32_dev(d_in.ptr, w, h, d_ref.ptr, None))
            S.sync()
            want = hashlib.sha256(d_ref.to_numpy(np.float32, (2 * h, 2 * w)).tobytes()).hexdigest()
            assert got == want, "gathered frame differs from the whole-frame result"
            return {"gathered_sha256": got, "equals_whole_frame_call": True}
        mpix_step = 4 * w * h / 1e6
        label = "one %dx%d Y frame -> %dx%d, %d output bands (each in %d sub-bands, gather of sub-band k overlapped with " \
                "the kernels of k+1) + RCCL gatherv to rank 0" % (w, h, 2 * w, 2 * h, world, tiled.nsub)
    elif args.workload == "host-stream":
        F = max(args.frames, 16)          # one call = one stream of F frames; the first H2D and the last D2H of a call are exposed
        step, cleanup = host_stream_setup(S, F, 0 if args.plain_launches else 2)
        mpix_step = world * F * 4 * IN_W * IN_H / 1e6
        label = "stream of %d host-resident (page-locked) 3840x2160 Y frames per rank per step: H2D + path + D2H over two " \
                "slots, %s (BASELINE config #5 shape), frames sharded %d-way" % (
                    F, "plain launches" if args.plain_launches else "one hipGraph per slot", world)
        extra["bytes_per_output_px_over_pcie"] = {"h2d": 1.0, "d2h": 4.0}
    elif args.workload == "frames-graph":
        import ctypes as C
        w, h, F = IN_W, IN_H, args.frames
        d_in = S.DeviceBuffer(F * w * h * 4)
        d_out = S.DeviceBuffer(F * 4 * w * h * 4)
        for f in range(F):
            d_in.upload(synth.plane(h, w, synth.SEED0 + rank * F + f, "smooth"), offset=f * w * h * 4)
        st = S.Stream()
        gh = C.c_void_p()
        S.check(L.srcnn_batch_graph_create(d_in.ptr, w, h, F, d_out.ptr, st.handle, C.byref(gh)))

        def step():
            S.check(L.srcnn_batch_graph_launch(gh))
        mpix_step = world * F * 4 * w * h / 1e6
        label = "%d resident 3840x2160 frames per rank per step, replayed from one captured hipGraph" % F
    else:
        w, h, F = 1920, 1080, 64
        d_in = S.DeviceBuffer(F * w * h * 4)
        d_out = S.DeviceBuffer(F * 4 * w * h * 4)
        for f in range(F):
            d_in.upload(synth.plane(h, w, synth.SEED0 + rank * F + f, "smooth"), offset=f * w * h * 4)

        def step():
            S.check(L.srcnn_y_upscale2x_f32_batch_dev(d_in.ptr, w, h, F, d_out.ptr, None))
        mpix_step = world * F * 4 * w * h / 1e6
        label = "batch of 64 resident 1920x1080 frames per rank per step"

    comm_made = args.workload == "tiled8k"

    def drain():
        # the tiled frame queues RCCL work: wait for it with the library's bounded wait (a missing peer or a mismatched gather
        # table ends in SRCNN_E_COMM after SRCNN_COMM_TIMEOUT_MS instead of hanging the job)
        if args.workload == "tiled8k":
            S.check(L.srcnn_comm_wait(None))
        S.sync()

    for _ in range(args.warmup):
        step()
    drain(); barrier()
    cpu0 = time.process_time()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        step()
    drain()
    t_own = time.perf_counter()
    barrier()
    ms = (time.perf_counter() - t0) * 1e3 / args.steps
    cpu_s = (time.process_time() - cpu0) / args.steps
    ms = reduce_max(dist, ms)
    cpu_s = reduce_max(dist, cpu_s)
    extra["per_rank_ms_per_step"] = gather_per_rank(dist, world, (t_own - t0) * 1e3 / args.steps)
    if verify is not None:
        extra["verify"] = verify()
    if args.workload != "tiled8k" and world > 1:      # after the measurement, like the headline workload
        extra["rccl_ranks"], note = rccl_probe(S, dist, rank, world, ndev)
        comm_made = extra["rccl_ranks"] is not None
        if note:
            extra["rccl_note"] = note
    if rank == 0:
        emit(json.dumps({"metric": METRIC + (" incl. PCIe" if args.workload == "host-stream" else ""),
                          "value": round(mpix_step / (ms * 1e-3), 2),
                          "unit": "MPix/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
                          "ms_per_step": round(ms, 4), "higher_is_better": True,
                          "scaling": "strong" if args.workload == "tiled8k" else "weak", "vs_baseline": None, "dtype": "f32",
                          "data": "synthetic", "config": {"workload": label, "mode": "strict"},
                          "host_cpu_s_per_step_max_rank": round(cpu_s, 5), **extra}))
    barrier()
    if cleanup is not None:
        cleanup()
    if comm_made:                          # never after a probe that timed out: its helper thread may still sit inside RCCL
        L.srcnn_comm_destroy()
    if dist is not None:
        dist.destroy_process_group()
    leave()


def dry_run_line(args, rank, world, dist):
    """--dry-run: the launcher / rendezvous / aggregation plumbing with NO device and no library load (CPU test of
    `bench.py --gpus N`).  `value` is null: nothing was measured."""
    import socket
    seen = [None] * world
    if dist is not None:
        dist.all_gather_object(seen, (rank, os.getpid()))
        dist.barrier()
    else:
        seen = [(rank, os.getpid())]
    t = reduce_max(dist, float(rank + 1))
    if rank == 0:
        emit(json.dumps({"metric": METRIC, "value": None, "unit": "MPix/s", "n_gpus": world, "steps": args.steps,
                          "warmup": args.warmup, "dry_run": True, "ranks_seen": [r for r, _ in seen],
                          "distinct_pids": len({p for _, p in seen}), "max_over_ranks_check": t,
                          "parent_pid": os.getppid(), "host": socket.gethostname(),
                          "config": {"workload": args.workload}}))
    if dist is not None:
        dist.barrier()
        dist.destroy_process_group()
    return 0


def traffic_record():
    """HBM bytes per launch of the dominant kernel from the committed PMC profile (rocprofv3 --pmc cannot run inside
    this process), with where it came from.  The profile records a sha256 over everything that decides the kernel's traffic
    (its text, its tile / LDS constants, the LDS-DMA primitive, its launchers: build.kernel_source_sha); if that differs in
    this tree, the figure is withheld (null) and the reason is given instead of a stale number.  Third value: the whole
    strict path's traffic per frame (all three kernels, same passes) against the algorithmic 5 B/px, or None -- each kernel's
    figure is held to its own fingerprint."""
    from libsrcnn_amd import build as _b
    now = _b.kernel_source_sha("k_conv12_mfma")
    for name in ("r06_pmc_conv12.json", "r05_pmc_conv12.json", "r04_pmc_conv12.json", "r03_pmc_conv12.json", "r02_pmc_conv12.json", "pmc_conv12.json"):
        path = os.path.join(ROOT, "profiles", name)
        if os.path.exists(path):
            try:
                rec = json.load(open(path))
            except Exception:
                continue
            src = "profiles/%s (%s)" % (name, rec.get("measured_at", "round 1, commit e142cbb"))
            then = rec.get("kernel_source_sha256")
            if then is None:
                return None, src + " -- WITHHELD: that profile does not say which kernel text it measured", None
            if then != now:
                return None, src + " -- WITHHELD: k_conv12_mfma (text, tile constants, staging primitive or launch geometry) has changed since (re-run tools/collect_profiles.sh)", None
            whole = None
            wp, parts = rec.get("whole_path"), rec.get("path", {})
            if wp and parts and all(v.get("kernel_source_sha256") == _b.kernel_source_sha(k) for k, v in parts.items()):
                whole = {"hbm_bytes_per_frame": wp["hbm_bytes_per_frame"], "algorithmic_bytes_per_frame": wp["algorithmic_bytes_per_frame"],
                         "ratio": round(wp["ratio"], 2),
                         "per_kernel_GB": {k: round((v["fetch_bytes"] + v["write_bytes"]) / 1e9, 3) for k, v in parts.items()},
                         "from": src}
            return rec.get("hbm_bytes_per_launch"), src, whole
    return None, None, None


DUMP_SEED = 0x5C0DE0D5          # fixed: the same positions in every run and every build
DUMP_MAX_FRAMES = 8
DUMP_SAMPLES = 1 << 20           # positions drawn per frame (duplicates dropped)
DUMP_EDGE = 16                   # border rows / columns kept whole: the guard-band logic lives there


def dump_outputs(outdir, d_out, frames, n_out):
    """--dump-outputs: what the last timed step left in the caller's output buffer (frames x 4320 x 7680 float32, rank 0's),
    reduced to at most DUMP_MAX_FRAMES x 5.5 MB so that two builds can be compared output for output:
      out_sample.npy    (nf, k)            float32  values at k fixed positions per frame (sorted flat indices into one
                                                    4320 x 7680 frame, drawn from DUMP_SEED; the same positions in every frame)
      out_edge_rows.npy (nf, 2*E, 7680)    float32  the first and the last E rows of each frame
      out_edge_cols.npy (nf, 4320, 2*E)    float32  the first and the last E columns of each frame
    nf = all frames up to DUMP_MAX_FRAMES, beyond that a seeded choice of DUMP_MAX_FRAMES of them (sorted)."""
    ow, oh, e = 2 * IN_W, 2 * IN_H, DUMP_EDGE
    rng = np.random.default_rng(DUMP_SEED)
    pick = np.arange(frames) if frames <= DUMP_MAX_FRAMES else np.sort(rng.choice(frames, DUMP_MAX_FRAMES, replace=False))
    pos = np.unique(rng.integers(0, n_out, DUMP_SAMPLES))
    sample = np.empty((len(pick), len(pos)), np.float32)
    rows = np.empty((len(pick), 2 * e, ow), np.float32)
    cols = np.empty((len(pick), oh, 2 * e), np.float32)
    for i, f in enumerate(pick):
        frame = d_out.to_numpy(np.float32, (oh, ow), offset=int(f) * n_out * 4)
        sample[i] = frame.reshape(-1)[pos]
        rows[i] = np.concatenate([frame[:e], frame[-e:]])
        cols[i] = np.concatenate([frame[:, :e], frame[:, -e:]], axis=1)
    os.makedirs(outdir, exist_ok=True)
    for name, a in (("out_sample", sample), ("out_edge_rows", rows), ("out_edge_cols", cols)):
        np.save(os.path.join(outdir, name + ".npy"), a)
    print("bench.py: wrote frames %s of the last timed step (%d sampled positions + %d-px borders each) to %s" %
          ([int(f) for f in pick], len(pos), e, outdir), file=sys.stderr)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--frames", type=int, default=4, help="4K frames per GPU per step")
    ap.add_argument("--full", action="store_true",
                    help="after the headline, also run everything else the line can carry: at N=1 the event-timed and clock-probed "
                         "steps, the other generator, the non-parity tiers, the PCIe-inclusive stream, ProcessSRCNN wall times, "
                         "BASELINE configs #2-#4 and the CPU baseline; at N>1 the RCCL connectivity probe.  Off by default: a plain "
                         "run sets up, warms up, times the steps and prints the line")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write what the last timed step computed (rank 0's output frames: a fixed sample, "
                         "see dump_outputs) to DIR/<name>.npy as float32")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="with --full: skip the CPU baseline")
    ap.add_argument("--no-extras", action="store_true", help="with --full: skip the PCIe / ProcessSRCNN / tier legs")
    ap.add_argument("--tier", default="strict", choices=["strict", "fast", "fast_f16"],
                    help="numerics tier of the timed loop.  strict (default) is the only parity mode and the only "
                         "headline; the others exist so that profiles of the non-parity kernels can be collected")
    ap.add_argument("--tiled-size", type=lambda s: tuple(int(v) for v in s.split("x")), default=(7680, 4320),
                    help="input WxH of the tiled8k workload (default 7680x4320 -> 15360x8640)")
    ap.add_argument("--workload", default="frames", choices=["frames", "frames-graph", "tiled8k", "host-stream", "batch1080p"],
                    help="frames (default, the headline metric): resident 4K frames sharded across ranks; "
                         "tiled8k: ONE 7680x4320 frame -> 15360x8640, output bands across ranks + RCCL gather (verified "
                         "against the whole-frame call once per run); "
                         "host-stream: PCIe-inclusive stream of 4K frames from host memory (hipGraph per slot); "
                         "batch1080p: 64 resident 1920x1080 frames per step; "
                         "frames-graph: the headline workload replayed from one captured hipGraph per step")
    ap.add_argument("--sub-bands", type=int, default=4, help="tiled8k: sub-bands per rank (gather of k overlaps compute of k+1)")
    ap.add_argument("--plain-launches", action="store_true", help="host-stream: no hipGraph replay (same kernels, same overlap)")
    ap.add_argument("--dry-run", action="store_true", help="launcher/rendezvous plumbing only: no device, value = null")
    args = ap.parse_args()
    if args.dump_outputs is not None and (args.workload != "frames" or args.dry_run):
        ap.error("--dump-outputs writes the headline workload's outputs: it needs --workload frames and no --dry-run")
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        # started without a launcher: become the launcher.  Nothing in this process has touched (or will touch) the GPU.
        sys.exit(launch_ranks(args.gpus, sys.argv[1:]))
    claim_stdout()
    if os.environ.get("SRCNN_BENCH_FAIL_RANK") == os.environ.get("RANK", "0") and args.dry_run:
        sys.exit(7)                        # test hook (tests/test_bench_launcher.py): a rank that dies before the rendezvous
    if args.workload != "frames":
        return side_workload(args)

    rank, local_rank, world, dist = rendezvous(args)
    if args.dry_run:
        return dry_run_line(args, rank, world, dist)

    def barrier():
        if dist is not None:
            dist.barrier()

    import libsrcnn_amd as S
    from libsrcnn_amd import synth
    ndev = max(1, S.device_count())
    S.init(local_rank % ndev)          # identity on a real N-GPU node; lets a 1-GPU box exercise the N>1 plumbing
    tier_mode = {"strict": S.MODE_STRICT, "fast": S.MODE_FAST, "fast_f16": S.MODE_FAST_F16}[args.tier]
    S.set_mode(tier_mode)
    L = S.lib()

    F = args.frames
    n_in, n_out = IN_W * IN_H, 4 * IN_W * IN_H
    d_in = S.DeviceBuffer(F * n_in * 4)
    d_out = S.DeviceBuffer(F * n_out * 4)

    def load(kind):   # rank r owns frames r*F .. r*F+F-1 of the synthetic stream, seed = 0x5C0DE000 + frame index
        for f in range(F):
            d_in.upload(synth.plane(IN_H, IN_W, synth.SEED0 + rank * F + f, kind), offset=f * n_in * 4)
    load("smooth")

    def step():
        S.check(L.srcnn_y_upscale2x_f32_batch_dev(d_in.ptr, IN_W, IN_H, F, d_out.ptr, None))

    def timed(k):
        S.sync()
        t0 = time.perf_counter()
        for _ in range(k):
            step()
        S.sync()
        return (time.perf_counter() - t0) / k

    for _ in range(args.warmup):
        step()
    S.sync()

    S.profile_reset()
    S.profile_enable(True)
    barrier()
    S.sync()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        step()
    S.sync()
    t_own = time.perf_counter()          # this rank's own finish, before the barrier: reported per rank, never the headline
    barrier()
    t1 = time.perf_counter()
    S.profile_enable(False)
    prof = S.profile_read()

    ms_per_step = reduce_max(dist, (t1 - t0) * 1e3 / args.steps)
    per_rank_ms = gather_per_rank(dist, world, (t_own - t0) * 1e3 / args.steps)

    # before anything else runs on d_out: the --full legs below overwrite it (other generator, other tiers)
    if args.dump_outputs is not None and rank == 0:
        dump_outputs(args.dump_outputs, d_out, F, n_out)

    # N > 1 (--full): prove, outside the timed region, that RCCL connects all N ranks (one communicator + one barrier); the
    # headline data path itself has no collective.  AFTER the measurement: a fabric that wedges half-way can leave
    # RCCL kernels spinning on the device, and those must not sit beside the timed steps.
    rccl_ranks, rccl_note = (None, None)
    if world > 1 and args.full:
        rccl_ranks, rccl_note = rccl_probe(S, dist, rank, world, ndev)

    if rank == 0:
        mpix_step = world * F * n_out / 1e6
        value = mpix_step / (ms_per_step * 1e-3)
        c12_ms, c12_n = prof["conv12"]
        avg12 = c12_ms / max(c12_n, 1)
        frames_timed = F * args.steps                            # frames this rank pushed through the timed region
        # One launch of the layer kernels = one BAND of a frame: a 7680x4320 frame holds 4.25 GB of layer-2 planes and the default
        # scratch cap (SRCNN_MAX_WORKSPACE_MB = 4608) holds them, a lower cap makes it several bands.  Algorithmic work per launch = the
        # frame's, divided by the launches per frame (recomputed halo rows are not algorithmic work).
        launches_per_frame = max(1.0, c12_n / max(frames_timed, 1))
        px_per_launch = n_out / launches_per_frame
        flops12 = 2.0 * MAC_L12 * px_per_launch                 # algorithmic FLOPs of one conv12 launch
        achieved = flops12 / (avg12 * 1e-3) / 1e12 if avg12 > 0 else 0.0
        traffic, traffic_from, whole_traffic = traffic_record()
        stage = {k: round(v[0] / max(frames_timed, 1), 4) for k, v in prof.items()}          # per FRAME (all its launches)
        alg_bytes12 = (4 + 128) * px_per_launch                 # layer-1+2 kernel: fp32 Y in, 32 fp32 planes out
        out = {
            "metric": METRIC,
            "value": round(value, 2), "unit": "MPix/s",
            "n_gpus": world, "steps": args.steps, "warmup": args.warmup, "ms_per_step": round(ms_per_step, 4),
            "per_rank_ms_per_step": per_rank_ms,
            "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
            "dtype": "f32", "data": "synthetic",
            "config": {"workload": "stream of synthetic 3840x2160 Y frames -> 7680x4320 (2x), %d frames/GPU/step, frames "
                                   "sharded across ranks, %s mode, generator 'smooth'" %
                                   (F, "strict (bit-exact)" if args.tier == "strict" else "NON-PARITY " + args.tier),
                       "frames_per_gpu_per_step": F, "in": [IN_W, IN_H], "out": [2 * IN_W, 2 * IN_H], "mode": args.tier,
                       "parallelism": "frames sharded %d-way, no data-path collective" % world},
            "roofline": {"kernel": "k_conv12_mfma (conv 9x9x1->64 + ReLU + conv 1x1x64->32 + ReLU)",
                         "bound": "mfma",
                         "bound_detail": "fp32 issue: per tap-step a wave pays 64 cycles of v_mfma_f32_32x32x1_2b_f32 (the rounded "
                                         "products) plus ~80 of v_pk_add_f32 (the rounded sums) and the two do not overlap on gfx950 "
                                         "(profiles/r01_mfma_coissue.txt): the binding resource is the SIMD's serialised MFMA + VALU issue, "
                                         "not the matrix pipe alone",
                         "achieved": round(achieved, 3), "peak": PEAK_F32_TFLOPS, "unit": "TFLOP/s",
                         "frac": round(achieved / PEAK_F32_TFLOPS, 4), "traffic": traffic, "traffic_from": traffic_from,
                         "frac_of_no_fma_ceiling": round(achieved / (PEAK_F32_TFLOPS / 2), 4),
                         "avg_launch_ms": round(avg12, 4), "launches": int(c12_n),
                         "launches_per_frame": round(launches_per_frame, 3), "output_px_per_launch": px_per_launch,
                         "flops_per_launch": flops12,
                         "note": "strict mode rounds product and sum separately (no FMA): ceiling is 0.5 of this peak",
                         "hbm": {"algorithmic_bytes_per_launch": alg_bytes12,
                                 "achieved_GBps": round(alg_bytes12 / (avg12 * 1e-3) / 1e9, 1) if avg12 > 0 else 0.0,
                                 "peak_GBps": PEAK_HBM_GBS,
                                 "frac": round(alg_bytes12 / (avg12 * 1e-3) / 1e9 / PEAK_HBM_GBS, 4) if avg12 > 0 else 0.0}},
            "roofline_all": roofline_all(stage, n_out, n_in),
            "stage_avg_ms_per_frame": stage,
            "whole_path": {"tflops": round(2.0 * MAC_ALL * mpix_step * 1e6 / (ms_per_step * 1e-3) / 1e12, 3),
                           "hbm_algorithmic_GBps": round(5 * mpix_step * 1e6 / (ms_per_step * 1e-3) / 1e9, 2),
                           # all kernels of the strict path, PMC FETCH+WRITE per 4K -> 8K frame vs the algorithmic 5 B/px: the 32 layer-2
                           # planes go through HBM once between the two layer kernels (neither is bandwidth-bound: DESIGN 4.5)
                           "hbm_traffic": whole_traffic},
            "max_abs_dY_vs_cpu_ref": None,
            "device": S.device_name(),
        }
        if world > 1:
            out["rccl_ranks"] = rccl_ranks
            out["devices_visible"] = ndev
            if not args.full:
                rccl_note = "RCCL connectivity is probed with --full"
            if rccl_note:
                out["rccl_note"] = rccl_note
        if args.tier != "strict":
            out["metric"] = METRIC + " [NON-PARITY tier %s]" % args.tier
            out["roofline"]["kernel"] = {"fast": "k_conv12_mfma<fast> (fp32 MFMA FMA chains)", "fast_f16": "k_fused_f16 (all three layers, split-fp16 MFMA)"}[args.tier]
            out["roofline"]["note"] = "non-parity tier: priced with the same algorithmic FLOPs of layers 1+2 (+3 for the fused kernel: see whole_path)"
        if world == 1 and args.full and not args.no_extras and args.tier == "strict":
            # SURVEY 8d also asks for the median of >= 10 device-timed steps: 10 more steps, each bracketed by HIP events on
            # the launch stream (outside the contract's timed region, which may not contain extra synchronisation)
            evs = [S.Event() for _ in range(11)]
            evs[0].record()
            for i in range(10):
                step()
                evs[i + 1].record()
            S.sync()
            per = sorted(evs[i].elapsed_ms(evs[i + 1]) for i in range(10))
            out["device_ms_per_step"] = {"median": round((per[4] + per[5]) / 2, 4), "min": round(per[0], 4), "max": round(per[-1], 4),
                                         "MPix/s_at_median": round(mpix_step / ((per[4] + per[5]) / 2 * 1e-3), 1), "steps": 10}
            # the shader clock the layer-1+2 launches of this loop run at (in-kernel probe, 3 more steps): what the drop-in call's
            # per-band clocks (process_srcnn_ms.*.phases_ms_last_call.layer12_shader_mhz_per_band) are to be held against
            S.clock_probe(True)
            for _ in range(3):
                step()
            S.sync()
            recs = S.clock_read(0)
            S.clock_probe(False)
            if recs:
                ms_ = sorted(float(m) for m, _us in recs)
                out["resident_layer12_mhz"] = {"median": round(ms_[len(ms_) // 2]), "min": round(ms_[0]), "max": round(ms_[-1]), "launches": len(ms_)}
            # both generators: the headline above is `smooth`; `noise` is the worst case for rounding
            gens = {"smooth": round(value, 1)}
            load("noise")
            step(); S.sync()
            gens["noise"] = round(F * n_out / 1e6 / timed(3), 1)
            load("smooth")
            out["generators"] = {"MPix/s": gens, "note": "same workload, 3 steps, frames from the other generator"}
            # non-parity tiers, same frames: throughput AND measured error against the strict result of frame 0
            # (strict == reference bit for bit, so this IS max|dY| vs the reference on a full 4K->8K frame)
            step(); S.sync()
            strict0 = d_out.to_numpy(np.float32, (2 * IN_H, 2 * IN_W))
            tiers = {}
            for mode, name in ((S.MODE_FAST, "fast_fp32_fma"), (S.MODE_FAST_F16, "fast_split_fp16_mfma")):
                S.set_mode(mode)
                step(); S.sync()
                dt = timed(3)
                got = d_out.to_numpy(np.float32, (2 * IN_H, 2 * IN_W))
                tiers[name] = {"MPix/s": round(F * n_out / 1e6 / dt, 1),
                               "max_abs_dY_vs_reference": float(np.max(np.abs(got.astype(np.float64) - strict0)))}
            S.set_mode(S.MODE_STRICT)
            out["non_parity_tiers"] = tiers
            del strict0
            try:
                out["pcie_inclusive"] = pcie_inclusive(S)
                out["process_srcnn_ms"] = process_srcnn_wall(S)
            except Exception as e:                                # noqa: BLE001
                out["extras_error"] = repr(e)
            try:
                out["configs"] = baseline_configs(S)
            except Exception as e:                                # noqa: BLE001
                out["configs"] = {"error": repr(e)}
        if world == 1 and args.full and not args.no_cpu_baseline and args.tier == "strict":
            try:
                out["cpu_baseline"], out["max_abs_dY_vs_cpu_ref"] = cpu_baseline(S)
            except Exception as e:                                # noqa: BLE001
                out["cpu_baseline"] = {"value": None, "unit": "MPix/s", "cores": physical_cores(), "kind": "port",
                                       "sample": "failed: %s" % e}
        emit(json.dumps(out))

    barrier()
    if world > 1 and rccl_ranks is not None:
        L.srcnn_comm_destroy()
    if dist is not None:
        dist.destroy_process_group()
    leave()


if __name__ == "__main__":
    main()
