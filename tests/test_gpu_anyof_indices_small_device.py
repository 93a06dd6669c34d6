"""Small-device parity of the grouped top + matched-positions query: the library told to behave as on a device of 1, 2 and 5 compute units
(FZB_DEBUG_CUS), each in a fresh child process, over 20 000 haystacks - `fuzzy0` as a base group and as a later group behind a fuzzy base.
Results equal the model of tests/anyof_indices_model.py; the proof that the grid-stride loops of the four new kernels took more than one trip
is from the grids the library recorded for that very call: work units / (recorded grid x the 256 a workgroup takes per trip) >= 2 at one
compute unit."""
import json
import os
import subprocess
import sys

import pytest

import anyof_indices_model as MI
from test_gpu_anyof import alternatives, make_list, positions

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N = 20000
LIMIT = 4000
CUS = (1, 2, 5)
QUERIES = ("base", "later")

CHILD = r'''
import json, sys
sys.path.insert(0, %(root)r)
sys.path.insert(0, %(tests)r)
import frizbee_amd as F
from test_gpu_anyof import alternatives, make_list, positions, matcher
hs = make_list("ragged", %(n)d)
cp = F.Corpus(hs)
out = {}
for name in %(queries)r:
    pats, groups = positions(alternatives("fuzzy0", "ragged"), "ragged")[name]
    res = {}
    for sort in ("ScoreThenIndexAsc", "IndexDesc"):
        fm = matcher(pats, groups, sort=sort)
        F.launch_grids()
        recs, found = fm.match_list_top_indices_groups(cp, %(limit)d)
        grids = F.launch_grids()
        res[sort] = dict(recs=[[r.index, r.score, int(r.exact), list(r.indices)] for r in recs], found=found, grids={k: list(v) for k, v in grids.items()})
    out[name] = res
print("GUNION-CHILD " + json.dumps(out))
'''


@pytest.mark.parametrize("cus", CUS)
def test_a_base_group_and_a_later_group_with_positions_on_a_small_device(cus):
    hs = make_list("ragged", N)
    code = CHILD % dict(root=ROOT, tests=os.path.join(ROOT, "tests"), n=N, queries=QUERIES, limit=LIMIT)
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300, env=dict(os.environ, FZB_DEBUG_CUS=str(cus)))
    assert r.returncode == 0 and "GUNION-CHILD " in r.stdout, (r.stdout[-2000:], r.stderr[-4000:])
    got = json.loads(r.stdout[r.stdout.index("GUNION-CHILD ") + 13:].splitlines()[0])
    alts = alternatives("fuzzy0", "ragged")
    for name in QUERIES:
        pats, groups = positions(alts, "ragged")[name]
        sources = sum(1 for p in pats if not p["negated"])
        for sort in ("ScoreThenIndexAsc", "IndexDesc"):
            want, found = MI.match_list_top_indices(pats, groups, hs, LIMIT, sort=sort)
            assert found > LIMIT and len(want) == LIMIT  # the head is full: every kernel walks LIMIT records
            res = got[name][sort]
            assert res["found"] == found and res["recs"] == [[i, s, int(e), ix] for i, s, e, ix in want], (cus, name, sort)
            grids = res["grids"]
            assert {k: v[2] for k, v in grids.items() if k.startswith("k_gunion")} == {"k_gunion_slots": 1, "k_gunion_clear": 1, "k_gunion_where": 1, "k_gunion_merge": 1}, grids
            assert "k_multi_union" not in grids
            # threads of work per kernel: a head record; a 16-byte word of the alternatives' maps; a (source, row) pair; a head record
            work = {"k_gunion_slots": LIMIT, "k_gunion_clear": len(alts) * LIMIT / 4, "k_gunion_where": sources * LIMIT, "k_gunion_merge": LIMIT}
            for kernel, threads in work.items():
                q = threads / 256 / grids[kernel][1]
                print("coverage", cus, name, kernel, grids[kernel], round(threads / 256, 1), round(q, 2))
                if cus == 1:
                    assert q >= 2, (name, kernel, q, grids[kernel], threads)
