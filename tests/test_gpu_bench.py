"""bench.py's plain run on the GPU: one line with the headline fields and none of what `--full` measures, and `--dump-outputs` writes the
records of the last timed step - equal to the CPU oracle's for the same seeded list."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import oracle_lib as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import synth  # noqa: E402

pytestmark = pytest.mark.gpu


def test_plain_bench_line_and_dumped_outputs_equal_the_oracle(tmp_path):
    n = 200_000
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--per-gpu", str(n), "--steps", "3", "--warmup", "1",
                        "--dump-outputs", str(tmp_path)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-1000:], r.stderr[-4000:])
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    j = json.loads(lines[0])
    assert j["steps"] == 3 and j["warmup"] == 1 and j["unit"] == "haystacks/s" and j["higher_is_better"] is True and j["dtype"] == "u8"
    assert j["ms_per_step"] > 0 and abs(j["value"] - n / (j["ms_per_step"] * 1e-3)) <= 1e-6 * j["value"]
    assert not {"roofline", "stages", "e2e", "e2e_cold", "check", "configs", "cpu_baseline", "two_queries_in_flight", "sharded"} & set(j), sorted(j)

    count = np.load(tmp_path / "match_count.npy")
    index, score, exact = (np.load(tmp_path / f"match_{k}.npy") for k in ("index", "score", "exact"))
    assert count.dtype == np.float64 and index.dtype == np.float64 and score.dtype == np.float32 and exact.dtype == np.float32
    assert int(count[0]) == len(index) == len(score) == len(exact) == j["config"]["matches_per_shard"] > 0
    rows = synth.make_rows(b"deadbe", n, 32, seed=12345, device="cuda")  # bench.py's list: the same generator, seed and device
    data = np.concatenate([rows.reshape(-1).cpu().numpy(), np.zeros(64, np.uint8)])
    want = O.Matcher("deadbe", lanes=(64, 64, 32), max_typos=0, sort="IndexAsc").match_packed(data, np.arange(1, n + 1, dtype=np.uint64) * np.uint64(32))
    assert index.tolist() == want["index"].astype(np.float64).tolist()
    assert score.tolist() == want["score"].astype(np.float32).tolist() and exact.tolist() == want["exact"].astype(np.float32).tolist()
