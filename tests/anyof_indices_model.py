"""The test model of matched positions for a matcher with any-of groups, built from the oracle alone.  The head is tests/anyof_model.py's
`match_list(...)[:limit]`.  Per pattern the positions come from `oracle_lib.MultiMatcher([pattern]).match_list_indices(haystacks)` over the
FULL list.  The rule is stated once, here:
  * the CARRIER of a group on a haystack is, among the alternatives that match it, the one with the largest key `score << 1 | exact`, the
    first in query order on equal keys;
  * the positions of a record are the strictly descending union without repeats of the positions of every plain non-negated pattern and of
    each group's carrier only.
tests/test_oracle_anyof_indices_premise.py holds the model to `oracle_lib.MultiMatcher.match_list_indices_ordered` where every group has one
alternative."""
import anyof_model as M
import oracle_lib as O

_IDX = {}


def pattern_indices(p, haystacks, cfg):
    """{index: (score, exact, [positions, descending])} of ONE pattern over the full list, its negation ignored (kept per list object)"""
    key = (id(haystacks), len(haystacks), repr(sorted(dict(p, negated=False).items(), key=str)), repr(sorted(cfg.items())))
    if key not in _IDX:
        om = O.MultiMatcher([dict(p, negated=False)], lanes=M.LANES, **dict(cfg, sort="IndexAsc"))
        recs, idx = om.match_list_indices(haystacks)
        _IDX[key] = (haystacks, {int(r["index"]): (int(r["score"]), int(r["exact"]), [int(x) for x in ix]) for r, ix in zip(recs, idx)})
    return _IDX[key][1]


def carrier(alts, i, haystacks, cfg):
    """the position in `alts` of the alternative that carries haystack i, or None when none matches it"""
    best, best_key = None, -1
    for a, p in enumerate(alts):
        hit = pattern_indices(p, haystacks, cfg).get(i)
        if hit is not None and (hit[0] << 1 | hit[1]) > best_key:
            best, best_key = a, hit[0] << 1 | hit[1]
    return best


def positions_of(patterns, group_of, haystacks, i, **cfg):
    """the positions of haystack i, which the composition accepts"""
    cfg.pop("sort", None)
    seen = set()
    for t in M.terms_of(patterns, group_of):
        if len(t) == 1 and t[0]["negated"]:
            continue
        c = carrier(t, i, haystacks, cfg)
        assert c is not None, ("the composition accepted a haystack a term does not match", i)
        seen.update(pattern_indices(t[c], haystacks, cfg)[i][2])
    return sorted(seen, reverse=True)


def with_positions(recs, patterns, group_of, haystacks, **cfg):
    """head records (MATCH_DTYPE, any order, scores possibly biased) -> [(index, score, exact, positions)]"""
    return [(int(r["index"]), int(r["score"]), bool(r["exact"]), positions_of(patterns, group_of, haystacks, int(r["index"]), **cfg)) for r in recs]


def match_list_top_indices(patterns, group_of, haystacks, limit, sort="ScoreThenIndexAsc", **cfg):
    """-> ([(index, score, exact, positions)], found)"""
    full = M.match_list(patterns, group_of, haystacks, sort=sort, **cfg)
    return with_positions(full[:limit], patterns, group_of, haystacks, **cfg), len(full)


def stride(patterns, group_of):
    """U_g: the needle bytes (at least 1) of the plain non-negated patterns + per group the largest among its alternatives"""
    total = 0
    for t in M.terms_of(patterns, group_of):
        if not (len(t) == 1 and t[0]["negated"]):
            total += max(max(1, len(p["needle"].encode() if isinstance(p["needle"], str) else p["needle"])) for p in t)
    return total
