"""Small-device parity of any-of groups: the library told to behave as on a device of 1, 2 and 5 compute units (FZB_DEBUG_CUS), each in a
fresh child process, over 20 000 haystacks - a base group and a later group behind a fuzzy base.  Records equal the model of
tests/anyof_model.py; the proof that the grid-stride loops of the new kernels took more than one trip is from the grids the library recorded
for that very call: work units / (recorded grid x what one workgroup takes per trip) >= 2 at one compute unit."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import anyof_model as M
from test_gpu_anyof import alternatives, make_list, positions

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N = 20000
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
        recs = fm.match_list(cp)
        grids = F.launch_grids()
        top, found = fm.match_list_top(cp, 100)
        res[sort] = dict(recs=[[int(r["index"]), int(r["score"]), int(r["exact"])] for r in recs], top=[[int(r["index"]), int(r["score"]), int(r["exact"])] for r in top], found=found,
                         grids={k: list(v) for k, v in grids.items()})
    out[name] = res
print("ANYOF-CHILD " + json.dumps(out))
'''


def triples(recs):
    return [[int(r["index"]), int(r["score"]), int(r["exact"])] for r in recs]


@pytest.mark.parametrize("cus", CUS)
def test_a_base_group_and_a_later_group_on_a_small_device(cus):
    hs = make_list("ragged", N)
    code = CHILD % dict(root=ROOT, tests=os.path.join(ROOT, "tests"), n=N, queries=QUERIES)
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300, env=dict(os.environ, FZB_DEBUG_CUS=str(cus)))
    assert r.returncode == 0 and "ANYOF-CHILD " in r.stdout, (r.stdout[-2000:], r.stderr[-4000:])
    got = json.loads(r.stdout[r.stdout.index("ANYOF-CHILD ") + 12:].splitlines()[0])
    alts = alternatives("fuzzy0", "ragged")
    fewest = min(len(M.pattern_hits(p, hs, {})) for p in alts)
    for name in QUERIES:
        pats, groups = positions(alts, "ragged")[name]
        # the positions of the group: the haystacks of the range, or the candidates the base pattern left
        slots = N if name == "base" else len(M.pattern_hits(pats[0], hs, {}))
        hits = fewest if name == "base" else min(len(set(M.pattern_hits(p, hs, {})) & set(M.pattern_hits(pats[0], hs, {}))) for p in alts)
        for sort in ("ScoreThenIndexAsc", "IndexDesc"):
            want = M.match_list(pats, groups, hs, sort=sort)
            assert 4096 < len(want) < N
            res = got[name][sort]
            assert res["recs"] == triples(want), (cus, name, sort)
            assert res["found"] == len(want) and res["top"] == triples(want[:100]), (cus, name, sort)
            grids = res["grids"]
            assert {k: v[2] for k, v in grids.items() if k.startswith("k_anyof")} == {"k_anyof_clear": 1, "k_anyof_accumulate": 3, "k_anyof_flag": 1, "k_anyof_compact": 1}, grids
            work = {"k_anyof_clear": slots / 4 / 256, "k_anyof_accumulate": hits / 256, "k_anyof_flag": slots / 1024, "k_anyof_compact": slots / 1024}
            for kernel, units in work.items():
                q = units / grids[kernel][1]
                print("coverage", cus, name, kernel, grids[kernel], round(units, 1), round(q, 2))
                if cus == 1:
                    assert q >= 2, (name, kernel, q, grids[kernel], units)
