"""The RCCL forms refuse a matcher with a facet sink attached (fzb_match_list_parallel_rccl, fzb_multi_match_list_parallel_rccl): the refusal
is a rank-local failure inside the collective, reached here with a world of one rank in a child process - a Matcher, a MultiMatcher and a
Matcher with an empty needle each get FZB_ERR_INVALID naming set_facets(NULL), and each succeeds after set_facets(None)."""
import os
import subprocess
import sys

import pytest

from test_gpu_scope import PATHS

pytestmark = pytest.mark.gpu


def test_rccl_refuses_a_matcher_with_a_sink_with_one_rank():
    code = r'''
import sys
sys.path[:0] = [%(root)r, %(tests)r, %(tools)r]
import numpy as np
import frizbee_amd as F, synth
from frizbee_amd.distributed import RcclShardComm
data, ends = synth.ragged_corpus(b"deadbeef", 3000, 4, 96, seed=3)
cp = F.Corpus(packed=(data, ends))
comm = RcclShardComm(rank=0, world=1)
sink = F.Facets(cp)
ms = [F.Matcher("deadbeef", F.Config(pf_lanes=64)), F.MultiMatcher(F.parse_query("dead be !x"), F.Config(pf_lanes=64)), F.Matcher("", F.Config(pf_lanes=64))]
for m in ms:
    m.set_facets(sink)
    try:
        comm.match_list_parallel(m, cp, 3)
        raise SystemExit("a matcher with a sink was accepted")
    except F.FrizbeeError as e:
        assert e.code == 1 and "set_facets(NULL)" in str(e) and "rccl" in str(e), str(e)
for m in ms:
    m.set_facets(None)
    want = m.match_list(cp); want["index"] += 3
    assert comm.match_list_parallel(m, cp, 3).tolist() == want.tolist()
assert len(ms[0].match_list(cp)) > 10
comm.close()
print("FACETS-RCCL-OK")
''' % PATHS
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    env.pop("FZB_RCCL_LIB", None)
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0 and "FACETS-RCCL-OK" in r.stdout, (r.stdout[-2000:], r.stderr[-4000:])
