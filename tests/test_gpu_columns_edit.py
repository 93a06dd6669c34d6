"""A corpus that carries BOTH per-haystack columns - the score bias and the tags - through the editing family (fzb_corpus_reserve /
_append / _truncate / _remove / _replace).  The two follow one set of helpers, so this is where one column's array, scratch or landing
place could end up in the other's.  A Python list of (haystack, bias, tag) is the model; after every step both device arrays equal the
model's exactly, and at the end a biased, scoped top-50 query equals the ORACLE's over the model's visible haystacks with the bias added
and every index mapped back."""
import os
import sys

import numpy as np
import pytest

import frizbee_amd as F
from test_gpu_scope import mapped, visible
from test_gpu_score_bias import biased
from test_gpu_topk import assert_top, single

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import synth  # noqa: E402

pytestmark = pytest.mark.gpu
REQUIRE, EXCLUDE = 1, 4


def make_model(n, seed=0):
    data, ends = synth.ragged_corpus(b"deadbeef", n, 4, 96, seed=seed, full=0.2, partial=0.3)
    raw, out, start = data.tobytes(), [], 0
    rng = np.random.default_rng(seed)
    bias = rng.integers(-300, 301, n)
    tags = rng.choice([0, 1, 3, 5, 0x8001, 0xFFFB], n)
    for e, b, t in zip(ends.tolist(), bias.tolist(), tags.tolist()):
        out.append((raw[start:e], int(b), int(t)))
        start = e
    return out


def upload(model):
    cp = F.Corpus([h for h, _, _ in model])
    cp.set_bias(np.array([b for _, b, _ in model], np.int16))
    cp.set_tags(np.array([t for _, _, t in model], np.uint16))
    cp.set_scope(REQUIRE, EXCLUDE)
    return cp


def appended(batch):
    return [(h, 0, 0) for h, _, _ in batch]


def check(cp, model, ctx, has_bias=True):
    assert len(cp) == len(model), ctx
    for name, col, dtype in (("bias", 1, np.int16), ("tags", 2, np.uint16)):
        got = cp.debug_read(name)
        want = np.array([p[col] for p in model], dtype) if has_bias or name == "tags" else np.zeros(0, dtype)
        assert np.array_equal(got, want), (ctx, name, np.flatnonzero(got != want)[:8].tolist() if len(got) == len(want) else (len(got), len(want)))
    info = cp.scope_info()
    assert (info["active"], info["require"], info["exclude"]) == (1, REQUIRE, EXCLUDE), ctx


_PAIR = []


def query(cp, model, ctx):
    """a biased, scoped top-50 query against the oracle: over the visible haystacks, the bias added, every index mapped back"""
    if not _PAIR:
        _PAIR.append((single("dead", sort="ScoreThenIndexAsc")[0], single("dead", sort="IndexAsc")[1]))
    fm, om = _PAIR[0]
    vis = visible([t for _, _, t in model], REQUIRE, EXCLUDE)
    asc = mapped(om.match_list([h for (h, _, _), v in zip(model, vis) if v]), vis)
    assert len(asc) > 50, ctx
    assert_top(fm.match_list_top(cp, 50), biased(asc, [b for _, b, _ in model], "ScoreThenIndexAsc"), 50, ctx)


def drop(model, idx):
    gone = set(int(i) for i in idx)
    return [p for k, p in enumerate(model) if k not in gone]


def test_the_editing_family_keeps_both_columns_in_step():
    model = make_model(1100, seed=11)  # one full tile and a partial one
    cp = upload(model)
    check(cp, model, "start")
    rng = np.random.default_rng(11)
    # append beyond the room: both arrays regrow, device to device, and the new haystacks start at zero in both
    cp.append([h for h, _, _ in make_model(700, seed=12)])
    model += appended(make_model(700, seed=12))
    assert cp.bias_info()["capacity"] >= len(model) and cp.scope_info()["capacity"] >= len(model)
    check(cp, model, "append")
    # both updates on appended haystacks in one go: they share the landing place of the pairs
    a, b = len(model) - 1, len(model) - 2
    cp.update_bias([a, b], [77, -9])
    cp.update_tags([b, a - 5], [1, 5])
    model[a] = (model[a][0], 77, model[a][2])
    model[b] = (model[b][0], -9, 1)
    model[a - 5] = (model[a - 5][0], model[a - 5][1], 5)
    check(cp, model, "updates of appended haystacks")
    # truncate clears the cut entries of both: an append behind it starts at zero
    model = model[: len(model) - 300]
    cp.truncate(len(model))
    check(cp, model, "truncate")
    cp.append([h for h, _, _ in make_model(150, seed=13)])
    model += appended(make_model(150, seed=13))
    check(cp, model, "append after truncate")
    # remove: one haystack (not tile-aligned, mid-word) - both scratches are counted, 2 bytes per suffix haystack each
    suffix = len(model) - 37
    cp.remove([37])
    model = drop(model, [37])
    check(cp, model, "remove one")
    assert cp.edit_info()["temp_bytes"] >= 4 * suffix
    idx = rng.choice(len(model), len(model) // 3, replace=True)
    cp.remove(idx)
    model = drop(model, idx)
    check(cp, model, "remove a random third")
    # a remove that fails validation leaves both arrays as they were
    with pytest.raises(F.FrizbeeError):
        cp.remove([0, len(model)])
    check(cp, model, "after a refused remove")
    # replace: the index map is the identity for both arrays
    idx = [len(model) - 1, 5, len(model) // 2]
    new = [b"src/dead/renamed_to_something_much_longer_than_it_was_before/file.cc", b"", b"dead"]
    cp.replace(idx, new)
    for i, h in zip(idx, new):
        model[i] = (h, model[i][1], model[i][2])
    check(cp, model, "replace")
    query(cp, model, "replace")
    # a cleared bias is no longer carried: the removal compacts the tags alone, and the bias array stays all zero with its room
    capacity = cp.bias_info()["capacity"]
    cp.set_bias(None)
    model = [(h, 0, t) for h, _, t in model]
    cp.remove([37, 500])
    model = drop(model, [37, 500])
    info = cp.bias_info()
    assert info["has_bias"] == 0 and info["capacity"] == capacity
    check(cp, model, "remove after clear_bias", has_bias=False)
    k = len(model) // 2
    cp.update_bias([k], [7])
    model[k] = (model[k][0], 7, model[k][2])
    check(cp, model, "update_bias after clear_bias: zero except at k")
    query(cp, model, "end")


def test_reserve_then_appends_and_updates_within_the_room_allocate_nothing():
    model = make_model(1100, seed=5)
    cp = upload(model)
    cp.reserve(len(model) + 2500, sum(len(h) + 15 for h, _, _ in model) + 2500 * 112)
    bias_info, scope_info = cp.bias_info(), cp.scope_info()
    assert bias_info["capacity"] >= len(model) + 2500 and scope_info["capacity"] >= len(model) + 2500
    fm = single("dead", sort="ScoreThenIndexAsc")[0]
    fm.reserve(cp)
    fm.match_list_top(cp, 50)
    batches = [make_model(1100, seed=300 + k) for k in range(2)]
    before = F.device_allocs()
    for batch in batches:
        cp.append([h for h, _, _ in batch])
        model += appended(batch)
        at = [len(model) - 1, len(model) - 600, 3]
        cp.update_bias(at, [5, -5, 300])
        cp.update_tags(at, [1, 3, 5])
        for i, b, t in zip(at, [5, -5, 300], [1, 3, 5]):
            model[i] = (model[i][0], b, t)
        fm.match_list_top(cp, 50)
        assert F.device_allocs() == before, "an append within the reserved room, an update behind it or the query allocated device memory"
    assert cp.bias_info() == bias_info and cp.scope_info() == scope_info
    check(cp, model, "appends within the room")
    query(cp, model, "appends within the room")
