"""The per-haystack tags stay in step with a corpus that grows and is edited (fzb_corpus_reserve / _append / _truncate / _remove /
_remove_device / _replace).  A Python list of (haystack, tag) pairs is the model; after every step the device's tags array equals the
model's (zeros for appended items, compaction on remove, identity on replace), and a scoped query equals the ORACLE's over the model's
visible haystacks with every index mapped back."""
import os
import sys

import numpy as np
import pytest

import frizbee_amd as F
from test_gpu_topk import assert_top, single

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import synth  # noqa: E402

pytestmark = pytest.mark.gpu
REQUIRE, EXCLUDE = 1, 4


def make_model(n, seed=0):
    data, ends = synth.ragged_corpus(b"deadbeef", n, 4, 96, seed=seed, full=0.2, partial=0.3)
    raw, out, start = data.tobytes(), [], 0
    tags = np.random.default_rng(seed).choice([0, 1, 3, 5, 0x8001, 0xFFFB], n)
    for e, t in zip(ends.tolist(), tags.tolist()):
        out.append((raw[start:e], int(t)))
        start = e
    return out


def upload(model):
    cp = F.Corpus([h for h, _ in model])
    cp.set_tags(np.array([t for _, t in model], np.uint16))
    cp.set_scope(REQUIRE, EXCLUDE)
    return cp


_PAIR = []


def pair():
    """(HIP matcher, oracle matcher), made once"""
    if not _PAIR:
        _PAIR.append(single("dead", sort="ScoreThenIndexAsc"))
    return _PAIR[0]


def check(cp, model, ctx):
    fm, om = pair()
    assert len(cp) == len(model), ctx
    got = cp.debug_read("tags")
    tags = np.array([t for _, t in model], np.uint16)
    assert np.array_equal(got, tags), (ctx, np.flatnonzero(got != tags)[:8].tolist() if len(got) == len(tags) else (len(got), len(tags)))
    info = cp.scope_info()
    assert (info["active"], info["require"], info["exclude"]) == (1, REQUIRE, EXCLUDE), ctx
    vis = ((tags & REQUIRE) == REQUIRE) & ((tags & EXCLUDE) == 0)
    sub = [h for (h, _), v in zip(model, vis) if v]
    want = om.match_list(sub) if sub else np.zeros(0, F.MATCH_DTYPE)
    want["index"] = np.flatnonzero(vis).astype(np.uint32)[want["index"]]
    assert fm.match_list(cp).tolist() == want.tolist(), ctx
    assert_top(fm.match_list_top(cp, 50), want, 50, ctx)


def drop(model, idx):
    gone = set(int(i) for i in idx)
    return [p for k, p in enumerate(model) if k not in gone]


@pytest.mark.parametrize("n", (1025, 3000))
def test_the_editing_family_keeps_the_tags_in_step(n):
    import torch

    model = make_model(n, seed=n)
    cp = upload(model)
    check(cp, model, "start")
    rng = np.random.default_rng(n)
    # append: the new haystacks start with tag 0 (beyond the room: the array moves device to device)
    batch = make_model(700, seed=n + 1)
    cp.append([h for h, _ in batch])
    model += [(h, 0) for h, _ in batch]
    assert cp.scope_info()["capacity"] >= len(model)
    check(cp, model, "append")
    cp.update_tags([len(model) - 1, len(model) - 2], [1, 5])
    model[-1], model[-2] = (model[-1][0], 1), (model[-2][0], 5)
    check(cp, model, "update of appended haystacks")
    # truncate clears the cut entries: an append behind it starts at 0
    keep = len(model) - 300
    cp.truncate(keep)
    model = model[:keep]
    check(cp, model, "truncate")
    batch = make_model(150, seed=n + 2)
    cp.append([h for h, _ in batch])
    model += [(h, 0) for h, _ in batch]
    check(cp, model, "append after truncate")
    # remove: one haystack (not tile-aligned, mid-word), then a random third in any order with repeats
    cp.remove([37])
    model = drop(model, [37])
    check(cp, model, "remove one")
    assert cp.edit_info()["temp_bytes"] >= 2 * (len(model) + 1 - 37)  # the tags' scratch is counted: 2 bytes per suffix haystack
    idx = rng.choice(len(model), len(model) // 3, replace=True)
    cp.remove(idx)
    model = drop(model, idx)
    check(cp, model, "remove a random third")
    # a remove that fails validation leaves the tags and the scope as they were
    with pytest.raises(F.FrizbeeError):
        cp.remove([0, len(model)])
    check(cp, model, "after a refused remove")
    # remove_device: "drop everything that matches this query" - the records of an UNSCOPED IndexAsc query are the index list (stride 8)
    fd = F.Matcher("beef", F.Config(sort=F.SortStrategy.IndexAsc, pf_lanes=64, sw_lanes=64))
    out = torch.zeros(len(model) * 8, dtype=torch.uint8, device="cuda")
    cnt = torch.zeros(2, dtype=torch.int32, device="cuda")
    cp.set_scope(0, 0)
    fd.match_list_device(cp, out.data_ptr(), len(model), cnt.data_ptr())
    torch.cuda.synchronize()
    cp.set_scope(REQUIRE, EXCLUDE)
    hit = out.cpu().numpy()[: int(cnt[0]) * 8].view(F.MATCH_DTYPE)["index"]
    assert 10 < len(hit) < len(model)
    cp.remove_device(out.data_ptr(), 8, cnt.data_ptr(), len(model))
    model = drop(model, hit)
    check(cp, model, "remove_device")
    # replace: the index is the identity, a renamed path keeps its tag
    idx = [len(model) - 1, 5, len(model) // 2]
    new = [b"src/dead/renamed_to_something_much_longer_than_it_was_before/file.cc", b"", b"dead"]
    cp.replace(idx, new)
    for i, h in zip(idx, new):
        model[i] = (h, model[i][1])
    check(cp, model, "replace")


def test_remove_a_whole_tile_and_over_many_tiles():
    model = make_model(12_000, seed=77)
    cp = upload(model)
    rng = np.random.default_rng(77)
    idx = 777 + np.flatnonzero(rng.random(12_000 - 777) < 0.35)
    idx = np.concatenate([[777], idx, np.arange(5 * 1024 + 777, 6 * 1024 + 777)])  # with one source tile removed whole
    cp.remove(rng.permutation(idx))
    model = drop(model, idx)
    check(cp, model, "twelve tiles")
    cp.remove(np.arange(len(model)))
    check(cp, [], "all")
    fresh = make_model(100, seed=78)
    cp.append([h for h, _ in fresh])
    check(cp, [(h, 0) for h, _ in fresh], "append after removing all: the freed tail was zero")


def test_reserve_then_appends_within_the_room_allocate_nothing():
    model = make_model(2000, seed=5)
    cp = upload(model)
    cp.reserve(len(model) + 2500, sum(len(h) + 15 for h, _ in model) + 2500 * 112)
    info = cp.scope_info()
    assert info["capacity"] >= len(model) + 2500
    check(cp, model, "reserve")
    fm = pair()[0]
    fm.reserve(cp)
    fm.match_list(cp)
    fm.match_list_top(cp, 50)
    batches = [make_model(1100, seed=300 + k) for k in range(2)]
    before = F.device_allocs()
    for batch in batches:
        cp.append([h for h, _ in batch])
        model += [(h, 0) for h, _ in batch]
        cp.update_tags([len(model) - 1], [1])
        model[-1] = (model[-1][0], 1)
        fm.match_list_top(cp, 50)
    assert F.device_allocs() == before, "an append within the reserved room, or the scoped query behind it, allocated device memory"
    assert cp.scope_info() == info
    check(cp, model, "appends within the room")
