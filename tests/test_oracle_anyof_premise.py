"""The premise of the any-of tests, held to the oracle on the CPU: the test model of tests/anyof_model.py - every pattern matched on its own
over the full list, unioned per group under the max rule, composed in numpy - IS `Matcher::from_patterns` where every group has one
alternative, and a group's result does not depend on the order of its alternatives.  So what the GPU tests hold the device to differs from
the reference's composition by the union rule alone."""
import itertools

import numpy as np

import anyof_model as M
import oracle_lib as O
import ref_generators as R

SORTS = ("ScoreThenIndexAsc", "ScoreThenIndexDesc", "IndexAsc", "IndexDesc")


def full(p):
    return O.P(p["needle"], negated=p["negated"], matching=p.get("matching"))


def test_groups_of_one_are_the_reference_composition():
    said = 0
    for k, (patterns, haystacks, cfg) in enumerate(R.multi_cases(150, 5)):
        pats = [full(p) for p in patterns]
        sort = SORTS[k % 4]
        want = O.MultiMatcher(pats, lanes=M.LANES, sort=sort, **cfg).match_list(haystacks)
        for group_of in (None, list(range(len(pats))), [7 * i + 3 for i in range(len(pats))]):
            got = M.match_list(pats, group_of, haystacks, sort=sort, **cfg)
            assert got.tolist() == want.tolist(), (patterns, haystacks, cfg, sort, group_of)
        said += len(want) > 0
    assert said > 20, said


def test_a_group_does_not_depend_on_the_order_of_its_alternatives():
    rng = np.random.default_rng(3)
    words = ["dead", "beef", "cafe", "dea", "de", "ad", "fe", "a"]
    hs = ["".join(rng.choice(["dead", "beef", "cafe", "x", "_", "De", "AD", "f"], int(rng.integers(1, 6)))) for _ in range(300)] + words
    tie = [12, 6, 5, 1, 36, 4, 4, 8, 4]  # "dea" under this scoring ties "dead" on the haystack "dead", without the exact flag
    alts = [O.P("dead"), O.P("dea", scoring=tie), O.P("beef", max_typos=1), O.P("fe", matching="Suffix"), O.P("cafe", matching="Substring")]
    first = None
    for perm in itertools.permutations(range(len(alts))):
        got = M.compose([O.P("a")] + [alts[i] for i in perm], [0] + [1] * len(alts), hs).tolist()
        first = first or got
        assert got == first, perm
    assert 0 < len(first) < len(hs)
    # the tie at the maximum takes the exact flag of the alternative that has it, in either order
    for pair in ([alts[0], alts[1]], [alts[1], alts[0]]):
        r = M.compose(pair, [0, 0], ["dead", "dea"])
        assert r.tolist() == [(0, 84, 1, 0), (1, 92, 1, 0)], r


def test_the_model_composes_groups_like_patterns():
    """by hand: `a | b` then `c`, then not `d` - union, intersection with summed scores, removal"""
    hs = ["a", "b", "ab", "ac", "bc", "abc", "abcd", "c", ""]
    pats = [O.P("a"), O.P("b"), O.P("c"), O.P("d", negated=True, matching="Substring")]
    got = M.compose(pats, [0, 0, 1, 2], hs)
    assert got["index"].tolist() == [3, 4, 5]
    one = {i: M.pattern_hits(p, hs, {}) for i, p in enumerate(pats)}
    for r in got:
        i = int(r["index"])
        best = max(one[k][i][0] for k in (0, 1) if i in one[k])
        assert int(r["score"]) == best + one[2][i][0]
