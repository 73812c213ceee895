"""bench.py's two run shapes on the CPU (--dry-run-emu: the kernels' host emulation, the same plumbing as on the GPU).

A plain run prints the headline line only; --full adds the roofline, the compress leg and the CPU baseline.
--dump-outputs writes what the last timed step returned, the same bytes from run to run."""
import glob
import json
import os
import subprocess
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def bench(*extra):
    cmd = [sys.executable, "bench.py", "--dry-run-emu", "--unique-kib", "256", "--steps", "2", "--warmup", "1", *extra]
    r = subprocess.run(cmd, cwd=REPO, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1
    return json.loads(lines[0])


def test_plain_run_is_the_headline_and_dumps_the_last_step(tmp_path):
    a, b = tmp_path / "a", tmp_path / "b"
    res = bench("--dump-outputs", str(a))
    for key in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert key in res, key
    assert res["steps"] == 2 and res["warmup"] == 1 and res["ms_per_step"] > 0
    assert res["config"]["verified"] is True
    for key in ("roofline", "extras", "cpu_baseline", "notes", "summary"):
        assert key not in res, key
    bench("--dump-outputs", str(b))
    names = sorted(os.path.basename(p) for p in glob.glob(str(a / "*.npy")))
    assert names == ["actual_sizes.npy", "actual_sizes_chunks.npy", "decompressed_sample.npy",
                     "decompressed_sample_chunks.npy", "decompressed_sample_sizes.npy", "statuses.npy"]
    total = 0
    for name in names:
        x, y = np.load(a / name), np.load(b / name)
        assert x.dtype in (np.float32, np.float64) and np.array_equal(x, y), name
        total += x.nbytes
    assert total <= 64 << 20
    # what the caller got: every chunk of the batch decoded to the generator's bytes, full size, status 0
    sys.path.insert(0, REPO)
    from nvcomp_amd import datasets

    data = datasets.silesia_style(256 << 10, 0)
    chunks = np.load(a / "decompressed_sample_chunks.npy").astype(np.int64)
    assert chunks.tolist() == [0, 1, 2, 3]
    assert np.array_equal(np.load(a / "decompressed_sample.npy"), data.astype(np.float32))
    assert np.load(a / "actual_sizes.npy").tolist() == [65536.0] * 4
    assert np.load(a / "statuses.npy").tolist() == [0.0] * 4


def test_full_run_keeps_the_rest():
    res = bench("--full", "--algo", "snappy")
    assert res["roofline"]["bound"] == "hbm" and "gpu_compress_ratio" in res["extras"]
    assert res["cpu_baseline"]["value"] > 0 and "summary" in res
