"""CPU: the build's staleness check is content-based, bench.py never quotes an HBM-traffic counter that was measured
on a different text of the dominant kernel, and its --dump-outputs sample is fixed and bounded."""
import json
import os
import shutil
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def test_stale_is_content_based(tmp_path, monkeypatch):
    from libsrcnn_amd import build as b
    assert os.path.exists(b.LIB) and os.path.exists(b.STAMP), "run __graft_entry__.build() first"
    assert not b.stale()
    # newer file times alone do not make the build stale ...
    os.utime(os.path.join(b.CSRC, "srcnn_capi.cpp"))
    assert not b.stale()
    # ... a different content does, even if the .so is newer than every source (the case of a prebuilt .so shipped with
    # sources that changed under it)
    stamp = open(b.STAMP).read()
    try:
        open(b.STAMP, "w").write("0" * 64 + "\n")
        os.utime(b.LIB)
        assert b.stale()
    finally:
        open(b.STAMP, "w").write(stamp)
    assert not b.stale()


def test_digest_covers_every_source_and_header():
    from libsrcnn_amd import build as b
    have = {os.path.basename(d) for d in b.DEPS}
    for f in os.listdir(b.CSRC):
        if f.endswith((".hip", ".cpp", ".h", ".hpp", ".inc")):
            assert f in have, "%s is compiled or included but not part of the staleness digest" % f
    assert set(b.SOURCES) <= have


def test_traffic_is_withheld_for_a_different_kernel_text(tmp_path, monkeypatch):
    import bench
    from libsrcnn_amd import build as b
    prof = tmp_path / "profiles"
    prof.mkdir()
    monkeypatch.setattr(bench, "ROOT", str(tmp_path))
    rec = {"hbm_bytes_per_launch": 123.0, "measured_at": "test", "kernel_source_sha256": b.kernel_source_sha("k_conv12_mfma")}
    (prof / "r03_pmc_conv12.json").write_text(json.dumps(rec))
    val, src, _whole = bench.traffic_record()
    assert val == 123.0 and "r03_pmc_conv12.json" in src
    rec["kernel_source_sha256"] = "f" * 64
    (prof / "r03_pmc_conv12.json").write_text(json.dumps(rec))
    val, src, _whole = bench.traffic_record()
    assert val is None and "WITHHELD" in src
    del rec["kernel_source_sha256"]
    (prof / "r03_pmc_conv12.json").write_text(json.dumps(rec))
    val, src, _whole = bench.traffic_record()
    assert val is None and "WITHHELD" in src


def test_kernel_source_sha_sees_the_kernel():
    from libsrcnn_amd import build as b
    a = b.kernel_source_sha("k_conv12_mfma")
    assert a and len(a) == 64
    assert b.kernel_source_sha("k_conv3") not in (None, a)
    assert b.kernel_source_sha("k_does_not_exist") is None


class _HostFrames:
    """Stands in for the bench's device output buffer: to_numpy() of frames held in host memory."""
    def __init__(self, frames):
        self.data = frames

    def to_numpy(self, dtype, shape, offset=0):
        flat = self.data.reshape(-1)
        n = int(np.prod(shape))
        assert offset % 4 == 0 and offset // 4 + n <= flat.size
        return flat[offset // 4: offset // 4 + n].astype(dtype).reshape(shape)


def _frames(n):
    import bench
    oh, ow = 2 * bench.IN_H, 2 * bench.IN_W
    base = np.arange(oh * ow, dtype=np.float32).reshape(oh, ow)
    return np.stack([base + 1e6 * f for f in range(n)])


@pytest.mark.parametrize("frames", [1, 4, 11])
def test_dump_outputs_is_a_fixed_sample_of_every_frame_within_64mb(tmp_path, frames):
    """--dump-outputs: the same positions in every run, values that are the frames' own, the borders whole, float32 only,
    at most 64 MB in all."""
    import bench
    out = _frames(frames)
    n_out = 4 * bench.IN_W * bench.IN_H
    bench.dump_outputs(str(tmp_path / "a"), _HostFrames(out), frames, n_out)
    bench.dump_outputs(str(tmp_path / "b"), _HostFrames(out), frames, n_out)
    names = sorted(os.listdir(tmp_path / "a"))
    assert names == ["out_edge_cols.npy", "out_edge_rows.npy", "out_sample.npy"]
    total = 0
    for name in names:
        a, b = np.load(tmp_path / "a" / name), np.load(tmp_path / "b" / name)
        assert a.dtype == np.float32 and np.array_equal(a, b), name
        total += os.path.getsize(tmp_path / "a" / name)
    assert total <= 64 << 20
    sample, rows, cols = (np.load(tmp_path / "a" / n) for n in ("out_sample.npy", "out_edge_rows.npy", "out_edge_cols.npy"))
    nf = min(frames, bench.DUMP_MAX_FRAMES)
    assert sample.shape[0] == rows.shape[0] == cols.shape[0] == nf
    assert sample.shape[1] > bench.DUMP_SAMPLES // 2
    e = bench.DUMP_EDGE
    picked = np.round(rows[:, 0, 0] / 1e6).astype(int)             # frame f holds index + 1e6 * f
    assert len(set(picked)) == nf and all(0 <= f < frames for f in picked)
    for i, f in enumerate(picked):
        assert np.array_equal(rows[i], np.concatenate([out[f, :e], out[f, -e:]]))
        assert np.array_equal(cols[i], np.concatenate([out[f, :, :e], out[f, :, -e:]], axis=1))
        pos = (sample[i] - np.float32(1e6 * f)).astype(np.int64)
        assert np.array_equal(out[f].reshape(-1)[pos], sample[i])


def test_dump_outputs_is_refused_where_there_is_no_headline_output():
    import subprocess
    for extra in (["--dry-run"], ["--workload", "tiled8k"]):
        r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--dump-outputs", "x"] + extra,
                           capture_output=True, text=True, timeout=120)
        assert r.returncode == 2 and "--dump-outputs" in r.stderr, r.stderr
