"""GPU: a plain `bench.py` run (no --full) times exactly --steps steps and prints the headline line only; --dump-outputs writes
what the last timed step computed, and the decompressed half of it is the benchmark's input again."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from helpers import bench19

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu


def test_plain_run_with_dumped_outputs(tmp_path):
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    out = tmp_path / "out"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1", "--chunks", "4", "--chunk-mib", "8",
                        "--dump-outputs", str(out)], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    d = json.loads(lines[0])
    assert d["steps"] == 3 and d["warmup"] == 1 and d["ms_per_step"] > 0 and d["value"] > 0 and d["higher_is_better"] is True
    assert d["unit"] == "GB/s" and d["dtype"] == "u8" and d["metric"].startswith("compress+decompress GB/s")
    assert "roofline" not in d and "cpu_baseline" not in d and "legs" not in d          # --full material
    files = {f[:-4]: np.load(out / f) for f in os.listdir(out)}
    assert set(files) == {"cbytes", "compressed_head", "compressed_sample", "compressed_sums", "decompressed_sample", "decompressed_sums"}
    assert all(a.dtype in (np.float32, np.float64) for a in files.values()) and sum(a.nbytes for a in files.values()) <= 64_000_000
    n = 8 << 20
    data = bench19(n).astype(np.int64)
    want = [int(data.sum()), int((data * (np.arange(n) % 65521 + 1)).sum()) % (1 << 52)]
    assert files["decompressed_sums"].shape == (4, 2) and (files["decompressed_sums"] == want).all()
    cb = files["cbytes"]
    assert cb.shape == (4,) and (cb > 16).all() and abs(n * 4 / cb.sum() - d["ratio"]) < 1e-3 * d["ratio"]
    # the blosc header of every chunk: its nbytes and cbytes fields (bytes 4-7 and 12-15, little endian) as the call reported them
    head = files["compressed_head"]
    le = lambda row, k: sum(int(row[k + i]) << (8 * i) for i in range(4))
    assert all(le(head[i], 4) == n and le(head[i], 12) == cb[i] for i in range(4))
