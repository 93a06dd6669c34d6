"""Every Python entry point of the repository byte-compiles, and bench.py's command line parses: a syntax slip in a script that only runs on
the GPU box (bench.py, tools/) must fail HERE, in the CPU suite, not at the end of a round."""
import glob
import os
import py_compile
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_every_script_byte_compiles(tmp_path):
    files = [os.path.join(ROOT, "bench.py"), os.path.join(ROOT, "__graft_entry__.py")]
    for pat in ("tools/*.py", "frizbee_amd/*.py", "oracle/*.py", "tests/*.py"):
        files += sorted(glob.glob(os.path.join(ROOT, pat)))
    assert len(files) > 20
    for f in files:
        py_compile.compile(f, cfile=str(tmp_path / (os.path.basename(f) + "c")), doraise=True)


def test_bench_command_line_parses():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--help"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-800:]
    for flag in ("--gpus", "--steps", "--warmup", "--full", "--dump-outputs"):
        assert flag in r.stdout


def test_bench_dump_outputs_samples_a_long_list(tmp_path):
    sys.path.insert(0, ROOT)
    import bench
    import frizbee_amd as F

    n = bench.DUMP_MAX_RECORDS + 12_345
    rec = np.zeros(n, F.MATCH_DTYPE)
    rec["index"] = np.arange(n, dtype=np.uint32) * 3 + 16_777_217  # beyond float32's exact integers
    rec["score"] = np.arange(n) % 700
    rec["exact"] = np.arange(n) % 2
    for d in (tmp_path / "a", tmp_path / "b"):
        bench.dump_outputs(str(d), rec)
    arrays = {f: np.load(tmp_path / "a" / f) for f in sorted(os.listdir(tmp_path / "a"))}
    assert sorted(arrays) == ["match_count.npy", "match_exact.npy", "match_index.npy", "match_score.npy"]
    assert arrays["match_count.npy"].tolist() == [n] and sum(a.nbytes for a in arrays.values()) <= 64 << 20
    idx = arrays["match_index.npy"]
    assert idx.dtype == np.float64 and len(idx) == bench.DUMP_MAX_RECORDS and (np.diff(idx) > 0).all()
    pos = ((idx - 16_777_217) / 3).astype(np.int64)  # the sampled positions: every field taken from the same records
    assert (idx == rec["index"][pos]).all() and (arrays["match_score.npy"] == rec["score"][pos]).all() and (arrays["match_exact.npy"] == rec["exact"][pos]).all()
    for f, a in arrays.items():  # a fixed sample: the same files every time
        assert a.dtype in (np.float32, np.float64) and np.array_equal(a, np.load(tmp_path / "b" / f)), f
