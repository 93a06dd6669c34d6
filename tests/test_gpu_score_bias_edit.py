"""The per-haystack score bias stays in step with a corpus that grows and is edited (fzb_corpus_reserve / _append / _truncate / _remove /
_remove_device / _replace).  A Python list of (haystack, bias) pairs is the model; after every step the device's bias array equals the
model's, and a ScoreThenIndexAsc top-50 query equals that of a fresh Corpus of the model's haystacks with the model's biases set."""
import os
import sys

import numpy as np
import pytest

import frizbee_amd as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import synth  # noqa: E402

pytestmark = pytest.mark.gpu
SIZES = (1023, 1024, 1025, 3000)


def make_model(n, seed=0):
    data, ends = synth.ragged_corpus(b"deadbeef", n, 4, 96, seed=seed, full=0.2, partial=0.3)
    raw, out, start = data.tobytes(), [], 0
    bias = np.random.default_rng(seed).choice([0, 300, -32768, -4, 9, 31], n)
    for e, b in zip(ends.tolist(), bias.tolist()):
        out.append((raw[start:e], int(b)))
        start = e
    return out


def upload(model):
    cp = F.Corpus([h for h, _ in model])
    cp.set_bias(np.array([b for _, b in model], np.int16))
    return cp


def check(cp, model, fm, ctx):
    assert len(cp) == len(model), ctx
    got = cp.debug_read("bias")
    want = np.array([b for _, b in model], np.int16)
    assert np.array_equal(got, want), (ctx, np.flatnonzero(got != want)[:8].tolist() if len(got) == len(want) else (len(got), len(want)))
    recs, found = fm.match_list_top(cp, 50)
    if model:
        wrecs, wfound = fm.match_list_top(upload(model), 50)
        assert found == wfound and recs.tolist() == wrecs.tolist(), ctx
    else:
        assert found == 0 and len(recs) == 0


def matcher():
    return F.Matcher("dead", F.Config(sort=F.SortStrategy.ScoreThenIndexAsc, pf_lanes=64, sw_lanes=64))


def drop(model, idx):
    gone = set(int(i) for i in idx)
    return [p for k, p in enumerate(model) if k not in gone]


@pytest.mark.parametrize("n", SIZES)
def test_remove_keeps_the_bias_in_step(n):
    model = make_model(n, seed=n)
    cp, fm = upload(model), matcher()
    check(cp, model, fm, "start")
    rng = np.random.default_rng(n)
    # one haystack (not tile-aligned, mid-word)
    one = [min(n - 1, 37)]
    cp.remove(one)
    model = drop(model, one)
    check(cp, model, fm, "one haystack")
    assert cp.edit_info()["temp_bytes"] >= 2 * (len(model) + 1 - 37)  # the bias' scratch is counted: 2 bytes per suffix haystack
    # a random third, any order, with repeats
    idx = rng.choice(len(model), len(model) // 3, replace=True)
    cp.remove(idx)
    model = drop(model, idx)
    check(cp, model, fm, "a random third")
    # a failing remove (an index out of range) leaves the bias unchanged
    with pytest.raises(F.FrizbeeError):
        cp.remove([0, len(model)])
    check(cp, model, fm, "after a refused remove")
    # everything from a non-tile-aligned i0 on
    i0 = min(len(model) - 1, 333)
    cp.remove(np.arange(i0, len(model)))
    model = model[:i0]
    check(cp, model, fm, "everything from i0 on")
    cp.remove(np.arange(len(model)))
    model = []
    check(cp, model, fm, "all")
    # the freed tail is zero: appended haystacks start unbiased
    fresh = make_model(100, seed=n + 1)
    cp.append([h for h, _ in fresh])
    model = [(h, 0) for h, _ in fresh]
    check(cp, model, fm, "append after removing all")


def test_remove_a_whole_tile_and_through_remove_device():
    import torch

    model = make_model(3000, seed=9)
    cp, fm = upload(model), matcher()
    tile = np.arange(1024, 2048)
    cp.remove(tile)
    model = drop(model, tile)
    check(cp, model, fm, "a whole tile")
    # "drop everything that matches this query": the records of an IndexAsc query stay in HBM and are the index list (stride 8)
    fd = F.Matcher("beef", F.Config(sort=F.SortStrategy.IndexAsc, pf_lanes=64, sw_lanes=64))
    out = torch.zeros(len(model) * 8, dtype=torch.uint8, device="cuda")
    cnt = torch.zeros(2, dtype=torch.int32, device="cuda")
    fd.match_list_device(cp, out.data_ptr(), len(model), cnt.data_ptr())
    torch.cuda.synchronize()
    hit = out.cpu().numpy()[: int(cnt[0]) * 8].view(F.MATCH_DTYPE)["index"]
    assert 10 < len(hit) < len(model)
    cp.remove_device(out.data_ptr(), 8, cnt.data_ptr(), len(model))
    model = drop(model, hit)
    check(cp, model, fm, "remove_device")


def test_remove_over_many_tiles():
    """twelve source tiles from a non-tile-aligned, mid-word first index: every workgroup of k_col_compact lands at its scanned base"""
    model = make_model(12_000, seed=77)
    cp, fm = upload(model), matcher()
    rng = np.random.default_rng(77)
    idx = 777 + np.flatnonzero(rng.random(12_000 - 777) < 0.35)
    idx = np.concatenate([[777], idx, np.arange(5 * 1024 + 777, 6 * 1024 + 777)])  # with one source tile removed whole
    cp.remove(rng.permutation(idx))
    model = drop(model, idx)
    check(cp, model, fm, "twelve tiles")


@pytest.mark.parametrize("n", SIZES)
def test_replace_truncate_append_reserve(n):
    model = make_model(n, seed=100 + n)
    cp, fm = upload(model), matcher()
    # replace: the index is the identity, a renamed path keeps its bias
    idx = [n - 1, 5, n // 2]
    new = [b"src/dead/renamed_to_something_much_longer_than_it_was_before/file.cc", b"", b"dead"]
    cp.replace(idx, new)
    for i, h in zip(idx, new):
        model[i] = (h, model[i][1])
    check(cp, model, fm, "replace")
    # truncate clears the cut entries: an append behind it starts at 0
    keep = n - n // 4
    cp.truncate(keep)
    model = model[:keep]
    check(cp, model, fm, "truncate")
    batch = make_model(n // 4 + 7, seed=200 + n)
    cp.append([h for h, _ in batch])
    model += [(h, 0) for h, _ in batch]
    check(cp, model, fm, "append after truncate")
    # reserve, then appends within the room: the bias array grows with the reservation and not again
    cp.reserve(len(model) + 2500, sum(len(h) + 15 for h, _ in model) + 2500 * 112)
    info = cp.bias_info()
    assert info["capacity"] >= len(model) + 2500
    check(cp, model, fm, "reserve")
    for k in range(2):
        batch = make_model(1100, seed=300 + n + k)
        cp.append([h for h, _ in batch])
        model += [(h, 0) for h, _ in batch]
        assert cp.bias_info() == info, "the bias array was reallocated by an append within the reserved room"
        check(cp, model, fm, f"append {k} within the room")
    # without a reservation the array regrows with the items, device to device
    batch = make_model(700, seed=400 + n)
    cp.append([h for h, _ in batch])
    model += [(h, 0) for h, _ in batch]
    assert cp.bias_info()["capacity"] >= len(model)
    check(cp, model, fm, "append beyond the room")
    cp.update_bias([len(model) - 1], [77])
    model[-1] = (model[-1][0], 77)
    check(cp, model, fm, "update of an appended haystack")
