"""The multi-device forms of the multi-pattern matcher: `match_list_parallel(threads)`, fzb_multi_match_list_parallel_sharded (the whole
AND / NOT composition per shard, gathered and ordered once on the root) and fzb_multi_match_list_parallel_rccl (one rank per shard; here
the ranks are threads over the RCCL test double, and one rank over the real library).  Every result must be unsharded `match_list`'s and
the oracle's (reference property: tests/api_properties.rs:402-414)."""
import os
import subprocess
import sys

import numpy as np
import pytest

import frizbee_amd as F
import oracle_lib as O
from test_gpu_sharded import _fake_rccl

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import synth  # noqa: E402

pytestmark = pytest.mark.gpu
SORTS = ("ScoreThenIndexAsc", "ScoreThenIndexDesc", "IndexAsc", "IndexDesc")
QUERIES = ("dead be !x", "^dead 'ea f$", "!x", "")
PATHS = dict(root=ROOT, tests=os.path.join(ROOT, "tests"), tools=os.path.join(ROOT, "tools"))


@pytest.fixture(scope="module")
def ragged():
    data, ends = synth.ragged_corpus(b"deadbeef", 50_000, 4, 120, seed=21)
    return data, ends, np.concatenate([data, np.zeros(64, np.uint8)])


def test_match_list_parallel_threads_equals_match_list(ragged):
    data, ends, _ = ragged
    cp = F.Corpus(packed=(data, ends))
    for q in QUERIES:
        m = F.MultiMatcher(F.parse_query(q), F.Config(pf_lanes=64))
        want = m.match_list(cp)
        for t in (1, 8):
            assert m.match_list_parallel(cp, t).tolist() == want.tolist(), (q, t)
        with pytest.raises(F.PanicError, match="threads must be positive"):
            m.match_list_parallel(cp, 0)


@pytest.mark.parametrize("by_bytes", [False, True])
def test_sharded_equals_match_list_and_the_oracle(ragged, by_bytes):
    data, ends, odata = ragged
    cp = F.Corpus(packed=(data, ends))
    sharded = {ns: F.ShardedCorpus(packed=(data, ends), ndev=ns, by_bytes=by_bytes, oversubscribe=True) for ns in (1, 2, 3, 8)}
    for q in QUERIES:
        for sort in SORTS:
            cfg = F.Config(pf_lanes=64, sort=F.SortStrategy[sort])
            m = F.MultiMatcher(F.parse_query(q), cfg)
            want = O.MultiMatcher(O.parse_query(q), sort=sort).match_packed(odata, ends)
            assert m.match_list(cp).tolist() == want.tolist(), (q, sort)
            for ns, sc in sharded.items():
                got = m.match_list_parallel_sharded(sc)
                assert got.tolist() == want.tolist(), (q, sort, ns, by_bytes, len(got), len(want))
            if q:
                assert "shard 7 on device" in m.shard_report(), m.shard_report()


def test_set_patterns_reaches_the_per_shard_clones(ragged):
    data, ends, odata = ragged
    sc = F.ShardedCorpus(packed=(data, ends), ndev=3, oversubscribe=True)
    m = F.MultiMatcher(F.parse_query("dead be !x"), F.Config(pf_lanes=64))
    first = m.match_list_parallel_sharded(sc)
    assert first.tolist() == O.MultiMatcher(O.parse_query("dead be !x")).match_packed(odata, ends).tolist()
    for q, sort in (("ef !d", "ScoreThenIndexAsc"), ("'bee", "IndexDesc"), ("dead", "ScoreThenIndexDesc"), ("", "IndexDesc"), ("a !b !c", "IndexAsc")):
        m.set_patterns(F.parse_query(q))
        m.set_config(F.Config(pf_lanes=64, sort=F.SortStrategy[sort]))
        got = m.match_list_parallel_sharded(sc)
        assert got.tolist() == O.MultiMatcher(O.parse_query(q), sort=sort).match_packed(odata, ends).tolist(), (q, sort)


_RCCL_CODE = r'''
import sys, threading, time
sys.path[:0] = [%(root)r, %(tests)r, %(tools)r]
import numpy as np
import frizbee_amd as F, oracle_lib as O, synth
from frizbee_amd.distributed import RcclShardComm, shard_ranges_by_bytes
WORLD = int(sys.argv[1])
data, ends = synth.ragged_corpus(b"deadbeef", 40_000, 4, 120, seed=8)
odata = np.concatenate([data, np.zeros(64, np.uint8)])
ranges = shard_ranges_by_bytes(ends, WORLD)
def shard(lo, hi):
    b0 = int(ends[lo - 1]) if lo else 0
    b1 = int(ends[hi - 1]) if hi else 0
    return F.Corpus(packed=(data[b0:b1].copy(), (ends[lo:hi] - np.uint64(b0)).astype(np.uint64)))
shards = [shard(lo, hi) for lo, hi in ranges]
def run_world(query, sort, all_ranks, offsets):
    res, errs = [None] * WORLD, [None] * WORLD
    uid = RcclShardComm.unique_id()
    def rank_main(r):
        try:
            comm = RcclShardComm(rank=r, world=WORLD, unique_id=uid)
            m = F.MultiMatcher(F.parse_query(query), F.Config(pf_lanes=64, sort=F.SortStrategy[sort]))
            try:
                for rep in range(2):  # the second query reuses the communicator's buffers
                    res[r] = comm.match_list_parallel(m, shards[r], offsets[r], all_ranks=all_ranks)
            finally:
                comm.close()
        except F.FrizbeeError as e:
            errs[r] = (e.code, str(e))
    ts = [threading.Thread(target=rank_main, args=(r,)) for r in range(WORLD)]
    [t.start() for t in ts]; [t.join() for t in ts]
    return res, errs
for query in ("dead be !x", "^dead 'ea f$", "!x", ""):
    for sort in ("ScoreThenIndexAsc", "IndexDesc"):
        want = O.MultiMatcher(O.parse_query(query), sort=sort).match_packed(odata, ends)
        for all_ranks in (False, True):
            res, errs = run_world(query, sort, all_ranks, [lo for lo, _ in ranges])
            assert not any(errs), errs
            for r in range(WORLD):
                if r == 0 or all_ranks:
                    assert res[r].tolist() == want.tolist(), (query, sort, all_ranks, r, len(res[r]), len(want))
                else:
                    assert len(res[r]) == 0
# only the LAST rank's index offset trips the u32 guard: every rank fails with that rank's error, none is left waiting in the exchange
offsets = [lo for lo, _ in ranges]
offsets[-1] = 0xFFFFFFFF - 5
t0 = time.time()
res, errs = run_world("dead be !x", "ScoreThenIndexAsc", True, offsets)
took = time.time() - t0
assert all(e is not None and e[0] == 2 for e in errs), errs
assert all(("rank %%d" %% (WORLD - 1)) in e[1] for e in errs), errs
assert took < 20, took  # (the double gives up on a missing counterpart after 30 s)
print("MULTI-RCCL-OK", WORLD)
'''


@pytest.mark.parametrize("world", [2, 3, 8])
def test_rccl_exchange_over_thread_ranks(world):
    r = subprocess.run([sys.executable, "-c", _RCCL_CODE % PATHS, str(world)], capture_output=True, text=True, timeout=600, env=dict(os.environ, FZB_RCCL_LIB=_fake_rccl()))
    assert r.returncode == 0 and "MULTI-RCCL-OK" in r.stdout, (r.stdout[-2000:], r.stderr[-4000:])


def test_rccl_exchange_with_the_real_library_and_one_rank():
    code = r'''
import sys
sys.path[:0] = [%(root)r, %(tests)r, %(tools)r]
import numpy as np
import frizbee_amd as F, synth
from frizbee_amd.distributed import RcclShardComm
data, ends = synth.ragged_corpus(b"deadbeef", 60_000, 4, 120, seed=4)
cp = F.Corpus(packed=(data, ends))
comm = RcclShardComm(rank=0, world=1)
for q in ("dead be !x", "!x", ""):
    for sort in ("ScoreThenIndexDesc", "IndexAsc"):
        m = F.MultiMatcher(F.parse_query(q), F.Config(pf_lanes=64, sort=F.SortStrategy[sort]))
        want = m.match_list(cp); want["index"] += 3
        for all_ranks in (False, True):
            got = comm.match_list_parallel(m, cp, 3, all_ranks=all_ranks)
            assert got.tolist() == want.tolist(), (q, sort, all_ranks, len(got), len(want))
comm.close()
print("MULTI-RCCL-REAL-OK")
''' % PATHS
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    env.pop("FZB_RCCL_LIB", None)
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0 and "MULTI-RCCL-REAL-OK" in r.stdout, (r.stdout[-2000:], r.stderr[-4000:])
