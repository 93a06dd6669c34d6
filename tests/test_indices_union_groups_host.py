"""The union step of the grouped top + matched-positions query on the CPU: frizbee_amd/csrc/indices_union_groups.h - what k_gunion_where and
k_gunion_merge call - compiled for the host (tests/gunion_host_lib.py) and held to a numpy model.  Per head record and term the model picks
the carrier: among the term's sources that are present, the largest key score << 1 | exact, the first on a tie.  Expected record: the
saturating u16 sum and the OR of the exact flags over the carriers, the head's index - its complement when a term has no present source.
Expected positions: np.unique(concat of the carriers' lists)[::-1], cut at `cap`."""
import os

import numpy as np
import pytest

import gunion_host_lib as G

pytestmark = pytest.mark.skipif(not G.available(), reason="g++ not installed")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def make_source(rng, head, present, stride, term, grouped, universe, scores, order="shuffled"):
    """one source: the traced records of the head records it is present at - in any order for an alternative, at row k for a plain pattern -
    with strictly descending position lists; npos may exceed the stride.  -> (source tuple, {k: (score, exact, list)})"""
    n = len(head)
    ks = np.flatnonzero(present)
    if grouped and order == "shuffled":
        ks = rng.permutation(ks)
    rows = max(n, 1)
    recs = np.zeros(rows, G.REC)
    recs["index"] = 0x00DEAD00  # (rows beyond the count must never be used)
    pos = np.full((rows, stride), 0xDEAD, np.uint32)
    npos = np.zeros(rows, np.uint32)
    per_k = {}
    for j, k in enumerate(ks.tolist()):
        ln = int(rng.integers(0, stride + 1)) if rng.random() < 0.7 else stride
        ln = min(ln, len(universe))
        vals = np.sort(rng.choice(universe, ln, replace=False))[::-1]
        s, e = int(rng.choice(scores)), int(rng.integers(0, 2))
        recs[j] = (head["index"][k], s, e, 0)
        pos[j, :ln] = vals
        npos[j] = ln + (int(rng.integers(0, 3)) if ln == stride else 0)
        per_k[k] = (s, e, vals.tolist())
    return (recs, len(ks), npos, pos.reshape(-1), stride, term, grouped), per_k


def model(head, sizes, per_src):
    """-> per head record: (index, score, exact, descending union, [carrier per term or None])"""
    out = []
    for k in range(len(head)):
        p, total, exact, lists, carriers, missing = 0, 0, 0, [], [], False
        for size in sizes:
            best, best_key = None, -1
            for q in range(p, p + size):
                if k in per_src[q]:
                    s, e, _ = per_src[q][k]
                    if (s << 1 | e) > best_key:
                        best, best_key = q, s << 1 | e
            carriers.append(best)
            if best is None:
                missing = True
            else:
                s, e, vals = per_src[best][k]
                total, exact = min(0xFFFF, total + s), exact | e
                lists.append(vals)
            p += size
        union = np.unique(np.array(sum(lists, []), np.int64))[::-1].tolist()
        index = int(head["index"][k])
        out.append(((~index) & 0xFFFFFFFF if missing else index, total, exact, union, carriers))
    return out


def run_case(rng, sizes, n, present_p=0.6, scores=(10, 10, 11, 300), overlap="interleaved", strides=None, every_term_present=True, cap=None):
    P = sum(sizes)
    n_hay = 10 * n + 5
    head = np.zeros(n, G.REC)
    head["index"] = rng.permutation(n_hay)[:n]
    strides = [int(x) for x in rng.integers(1, 9, P)] if strides is None else strides
    sources, per_src, p = [], [], 0
    for t, size in enumerate(sizes):
        grouped = size > 1
        masks = rng.random((size, n)) < present_p if grouped else np.ones((1, n), bool)
        if grouped and every_term_present:
            for k in np.flatnonzero(~masks.any(0)).tolist():
                masks[int(rng.integers(0, size)), k] = True
        for a in range(size):
            if overlap == "same":
                universe = np.arange(100, 100 + max(strides) + 1)
            elif overlap == "disjoint":
                universe = np.arange(1000 * p, 1000 * p + 2 * strides[p] + 1)
            else:
                universe = np.arange(0, 2 * sum(strides) + 2)
            src, per_k = make_source(rng, head, masks[a], strides[p], 7 + 3 * t, grouped, universe, scores)
            sources.append(src)
            per_src.append(per_k)
            p += 1
    maps = G.where_maps(sources, head, n_hay)
    for q, m in enumerate(maps):  # the maps say where every present record sits, and 0 elsewhere
        if m is not None:
            assert sorted(int(x) - 1 for x in m if x) == list(range(sources[q][1]))
            assert all(int(sources[q][0]["index"][int(m[k]) - 1]) == int(head["index"][k]) for k in per_src[q])
            assert all((m[k] != 0) == (k in per_src[q]) for k in range(n))
    U, p = 0, 0
    for size in sizes:
        U += max(strides[p:p + size])
        p += size
    cap_u = U if cap is None else cap
    comb, count, npos_u, pos_u, carrier_of = G.union(sources, maps, head, U=cap_u)
    assert count == n
    want = model(head, sizes, per_src)
    for k in range(n):
        index, score, exact, union, carriers = want[k]
        assert (int(comb["index"][k]), int(comb["score"][k]), int(comb["exact"][k] != 0)) == (index, score, exact), (sizes, k)
        assert len(union) <= U
        union = union[:cap_u]
        assert npos_u[k] == len(union) and pos_u[k, : len(union)].tolist() == union, (sizes, k, npos_u[k], union)
        assert (pos_u[k, len(union):] == 0xFFFFFFFF).all()  # nothing is written behind the union
        p = 0
        for size, c in zip(sizes, carriers):
            assert int(carrier_of[k, p]) == (p + size if c is None else c), (sizes, k, p)
            p += size
    return sources, maps, head, comb, want


def term_sizes(rng, P):
    sizes, left = [], P
    while left:
        s = int(rng.integers(1, min(8, left) + 1))
        sizes.append(s)
        left -= s
    return sizes


@pytest.mark.parametrize("P", range(1, 13))
@pytest.mark.parametrize("overlap", ["same", "disjoint", "interleaved"])
def test_record_carrier_and_merge_match_numpy(P, overlap):
    """1 to 12 sources - both sides of IUNION_BY_VALUE -, terms of 1 to 8 alternatives, random presence; scores drawn from (10, 10, 11, 300) with
    random flags give ties on the key and ties on the score with differing flags; the overlaps give shared positions between terms"""
    assert G.lib().gh_by_value() == 8 and G.lib().gh_absent() == 0xFFFFFFFF
    rng = np.random.default_rng(100 * P + len(overlap))
    for _ in range(6):
        run_case(rng, term_sizes(rng, P), int(rng.integers(1, 40)), overlap=overlap)
    run_case(rng, [min(P, 8)] + [1] * (P - min(P, 8)), 23, overlap=overlap)


def test_ties_on_the_key_go_to_the_first_and_ties_on_the_score_to_the_exact_one():
    head = np.zeros(3, G.REC)
    head["index"] = [5, 2, 9]

    def src(rows, term, grouped=True):
        recs = np.zeros(3, G.REC)
        pos = np.zeros((3, 2), np.uint32)
        for j, (h, s, e, vals) in enumerate(rows):
            recs[j] = (h, s, e, 0)
            pos[j, : len(vals)] = vals
        return (recs, len(rows), np.array([len(r[3]) for r in rows] + [0] * (3 - len(rows)), np.uint32), pos.reshape(-1), 2, term, grouped)

    a = src([(5, 40, 0, [9, 8]), (2, 40, 0, [7, 6]), (9, 40, 1, [5, 4])], 0)
    b = src([(9, 41, 0, [31, 30]), (2, 40, 1, [21, 20]), (5, 40, 0, [11, 10])], 0)  # (in another order than the head)
    for order, names in (([a, b], "ab"), ([b, a], "ba")):
        maps = G.where_maps(order, head, 16)
        comb, count, npos_u, pos_u, carrier_of = G.union(order, maps, head, U=2)
        first = {"a": [9, 8], "b": [11, 10]}[names[0]]
        assert pos_u[0].tolist() == first and carrier_of[0, 0] == 0  # equal keys: the first in query order
        assert pos_u[1].tolist() == [21, 20] and comb["exact"][1] == 1 and comb["score"][1] == 40  # equal scores: the exact one, wherever it stands
        assert pos_u[2].tolist() == [31, 30] and comb["exact"][2] == 0 and comb["score"][2] == 41  # a larger score wins whatever the flags
        assert comb["index"].tolist() == [5, 2, 9] and count == 3


def test_a_cap_smaller_than_the_lists_together_and_npos_beyond_the_stride():
    rng = np.random.default_rng(3)
    for cap in (0, 1, 3):
        run_case(rng, [3, 1, 2], 19, overlap="disjoint", strides=[4, 4, 4, 5, 3, 3], cap=cap)
    run_case(rng, [2, 2], 9, present_p=1.0, overlap="disjoint", strides=[200, 1, 1, 200])
    run_case(rng, [8], 30, overlap="same", strides=[1] * 8)


def test_scores_saturate():
    rng = np.random.default_rng(4)
    sources, maps, head, comb, want = run_case(rng, [2, 1, 3], 40, scores=(100, 20000, 30000, 65535), present_p=0.4)  # (three terms: 300 .. 3 x 65535)
    assert (comb["score"] == 65535).any() and (comb["score"] < 65535).any()


def test_a_group_with_no_present_alternative_gives_what_the_pack_check_rejects():
    rng = np.random.default_rng(5)
    sources, maps, head, comb, want = run_case(rng, [1, 3, 2], 60, present_p=0.3, every_term_present=False)
    missing = [k for k in range(60) if any(c is None for c in want[k][4])]
    assert missing and len(missing) < 60
    head = head.copy()
    head["score"], head["exact"] = comb["score"], comb["exact"]
    assert G.check(head, 60, comb, 60) == G.BAD_RECORD
    for k in missing:
        assert int(comb["index"][k]) == (~int(head["index"][k])) & 0xFFFFFFFF
    keep = [k for k in range(60) if k not in missing]
    assert G.check(head[keep], len(keep), comb[keep], len(keep)) == 0


def test_disagreement_on_index_sum_and_count():
    rng = np.random.default_rng(7)
    sizes = [1, 2]
    sources, maps, head, comb, want = run_case(rng, sizes, 12, present_p=1.0)
    head = head.copy()
    head["score"], head["exact"] = comb["score"], comb["exact"]
    assert G.check(head, 12, comb, 12) == 0
    U = sources[0][4] + max(sources[1][4], sources[2][4])
    # a carrier's record carries another index than the head's
    bad = [(s[0].copy(),) + s[1:] for s in sources]
    bad[0][0]["index"][5] ^= 1
    c2, count, _, _, _ = G.union(bad, maps, head, U=U)
    assert count == 12 and G.check(head, 12, c2, count) == G.BAD_RECORD and np.delete(c2["index"], 5).tolist() == np.delete(head["index"], 5).tolist()
    # the carriers' sum differs from the head's record
    h2 = head.copy()
    h2["score"][3] += 1
    assert G.check(h2, 12, comb, 12) == G.BAD_RECORD
    # a plain pattern with another count, an alternative with more than the head has; an alternative with fewer is what groups are about
    for q, other, bad_count in ((0, 11, True), (0, 13, True), (1, 13, True), (2, 20, True), (1, 11, False), (2, 0, False)):
        srcs = [s[:1] + ((other if p == q else s[1]),) + s[2:] for p, s in enumerate(sources)]
        c2, count, _, _, _ = G.union(srcs, maps, head, U=U)
        assert count == (other if bad_count else 12), (q, other, count)
        assert (G.check(head, 12, c2, count) & G.BAD_COUNT != 0) == bad_count


def test_no_source_and_a_head_longer_than_its_room():
    head = np.zeros(5, G.REC)
    head["index"] = [9, 3, 7, 1, 0]
    comb, count, npos_u, pos_u, _ = G.union([], [], head, U=0)
    assert count == 5 and comb["index"].tolist() == [9, 3, 7, 1, 0] and not comb["score"].any() and not comb["exact"].any() and not npos_u.any()
    rng = np.random.default_rng(8)
    sources, maps, head, comb, want = run_case(rng, [2, 1], 20)
    U = max(sources[0][4], sources[1][4]) + sources[2][4]
    c2, count, npos_u, pos_u, _ = G.union(sources, maps, head, head_count=20, max_records=7, U=U)
    assert len(c2) == 7 and c2.tolist() == comb[:7].tolist() and count == 20


def test_the_header_is_hip_free_and_a_build_dependency():
    csrc = os.path.join(ROOT, "frizbee_amd", "csrc")
    src = open(os.path.join(csrc, "indices_union_groups.h")).read()
    for word in ("#include <hip", "hipStream_t", "__global__", "__shared__", "threadIdx", "atomic"):
        assert word not in src, word
    for name in ("gunion_row(", "gunion_carrier(", "gunion_record(", "gunion_count(", "gunion_merge(", "iunion_add_score(", "anyof_pack(", "struct GUnionSrc", "const uint32_t* where", "uint32_t term"):
        assert name in src, name
    assert " indices_union_groups.h " in open(os.path.join(csrc, "Makefile")).read()
    kern = open(os.path.join(csrc, "kernels_indices.hip")).read()
    for name in ("k_gunion_slots", "k_gunion_clear", "k_gunion_where", "k_gunion_merge", "gunion_carriers(", "gunion_merge(", "gunion_count("):
        assert name in kern, name
    assert "hipLaunchKernelGGL" not in kern and "<<<" not in kern  # every launch through FZB_LAUNCH
    assert "#include <hip" not in open(os.path.join(ROOT, "tests", "kernel_host", "gunion_host.cpp")).read()
