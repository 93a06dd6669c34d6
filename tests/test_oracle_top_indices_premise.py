"""The premise the fused top + matched-positions query (fzb_match_list_top_indices) rests on, held to the oracle on the CPU: the fast
scorers behind `match_list` and the traced scorer behind `match_list_indices` give the same (index, score, exact), in the same order - the
accept decision is the same code in the reference (src/matcher/algo.rs:78-103 against :196-227) - so every record of a top-`limit` head
yields exactly one traced record at its place.  (On the device the pack kernel checks it again for every query.)"""
import os
import sys

import numpy as np
import pytest

import oracle_lib as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import synth  # noqa: E402

SORTS = ("ScoreThenIndexAsc", "ScoreThenIndexDesc", "IndexAsc", "IndexDesc")
QUERIES = [("deadbeef", dict(max_typos=0)), ("dead", dict(max_typos=0)), ("deadbeef", dict(max_typos=1)), ("db", dict(max_typos=None)),
           ("deadbeefdeadbeefdead", dict(max_typos=2)), ("dead", dict(matching="Substring")), ("de", dict(matching="Prefix"))]


def unpack(data, ends):
    raw = data.tobytes()
    out, start = [], 0
    for e in ends.tolist():
        out.append(raw[start:e])
        start = e
    return out


def same_records(needle, kw, data, ends, hs, sort):
    om = O.Matcher(needle, sort=sort, **kw)
    fast = om.match_packed(np.concatenate([data, np.zeros(64, np.uint8)]), ends)
    traced = om.match_list_indices_ordered(hs)
    assert [(int(r["index"]), int(r["score"]), bool(r["exact"])) for r in fast] == [t[:3] for t in traced], (needle, kw, sort)
    return len(traced)


@pytest.mark.parametrize("seed", [0, 1])
def test_fast_and_traced_scorers_agree_on_the_ragged_corpus(seed):
    data, ends = synth.ragged_corpus(b"deadbeef", 30_000, 4, 96, seed=seed)
    hs = unpack(data, ends)
    for needle, kw in QUERIES:
        for sort in SORTS:
            n = same_records(needle, kw, data, ends, hs, sort)
            if needle != "deadbeefdeadbeefdead":  # (matches nothing in this corpus: empty against empty)
                assert n > (100 if "matching" in kw else 1000), (needle, kw, n)


def test_fast_and_traced_scorers_agree_on_utf8():
    data, ends = synth.utf8_corpus(5_000, 32)
    hs = unpack(data, ends)
    for sort in SORTS:
        assert same_records("إنما", {}, data, ends, hs, sort) > 10
