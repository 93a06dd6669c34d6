"""The premise of the grouped matched-positions tests, held to the oracle on the CPU: the model of tests/anyof_indices_model.py - the head of
tests/anyof_model.py, every pattern's positions from the oracle on its own over the full list, the carrier rule and the descending unique
union in Python - IS `Matcher::match_list_indices` over `from_patterns` (match_one_indices_multi, src/matcher/multi.rs:56-82), truncated,
where every group has one alternative.  So what the GPU tests hold the device to differs from the reference by the carrier rule alone."""
import anyof_indices_model as MI
import anyof_model as M
import oracle_lib as O
import ref_generators as R

SORTS = ("ScoreThenIndexAsc", "ScoreThenIndexDesc", "IndexAsc", "IndexDesc")


def full(p):
    return O.P(p["needle"], negated=p["negated"], matching=p.get("matching"))


def test_groups_of_one_are_match_list_indices_truncated():
    said = shared = 0
    for k, (patterns, haystacks, cfg) in enumerate(R.multi_cases(150, 5)):
        pats = [full(p) for p in patterns]
        sort = SORTS[k % 4]
        want = O.MultiMatcher(pats, lanes=M.LANES, sort=sort, **cfg).match_list_indices_ordered(haystacks)
        for limit in (1, 3, len(haystacks)):
            for group_of in (None, [7 * i + 3 for i in range(len(pats))]):
                got, found = MI.match_list_top_indices(pats, group_of, haystacks, limit, sort=sort, **cfg)
                assert found == len(want) and got == [(i, s, e, list(ix)) for i, s, e, ix in want[:limit]], (patterns, haystacks, cfg, sort, limit)
        said += sum(1 for w in want if len(w[3]) > 0)
    assert said > 20, said
    # patterns that share matched bytes: the union drops the repeats, as the reference does
    hs = ["deadbeef", "beefdead", "xdxe"]
    pats = [O.P("dead"), O.P("de"), O.P("e")]
    want = O.MultiMatcher(pats, lanes=M.LANES, sort="IndexAsc").match_list_indices_ordered(hs)
    got, found = MI.match_list_top_indices(pats, None, hs, 3, sort="IndexAsc")
    assert found == len(want) == 2 and got == [(i, s, e, list(ix)) for i, s, e, ix in want]
    for i, s, e, ix in want:
        shared += sum(len(MI.pattern_indices(p, hs, {})[i][2]) for p in pats) > len(ix)
    assert shared == 2


def test_the_carrier_rule_by_hand():
    """`ab | b` on "ab": the longer alternative scores more and carries; on "b" only the second matches; equal keys go to the first"""
    hs = ["ab", "b", "xb"]
    pats = [O.P("ab"), O.P("b")]
    got, found = MI.match_list_top_indices(pats, [0, 0], hs, 3, sort="IndexAsc")
    assert found == 3 and [(g[0], g[3]) for g in got] == [(0, [1, 0]), (1, [0]), (2, [1])]
    assert MI.carrier(pats, 0, hs, {}) == 0 and MI.carrier(pats, 1, hs, {}) == 1
    twice = [O.P("b"), O.P("b")]
    assert MI.carrier(twice, 1, hs, {}) == 0
    assert MI.stride(pats, [0, 0]) == 2 and MI.stride(pats, None) == 3 and MI.stride(pats + [O.P("xyz", negated=True)], [0, 0, 1]) == 2
