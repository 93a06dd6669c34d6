"""The test model of any-of groups (`a | b`), built from the oracle alone.  The reference has no such operator, so the model states the
rule once, in numpy: every alternative is matched by the oracle over the FULL list on its own, a group's hits are the union by index with
score = the maximum of the matching alternatives' scores and exact = the OR of the exact flags of the alternatives that reach that maximum,
and the terms are then composed as `match_list_multi_into` composes patterns (src/matcher/multi.rs:84-152): every non-negated term must hit,
scores add with saturation at 65535, exact flags OR, a negated term that hits removes the haystack.  tests/test_oracle_anyof_premise.py
holds the model to `oracle_lib.MultiMatcher` where every group has one alternative."""
import numpy as np

import oracle_lib as O

LANES = (64, 64, 32)


def terms_of(patterns, group_of):
    """[(pattern, ...), ...]: the patterns of every term, in order; group_of None = every pattern its own term; empty needles dropped"""
    ids = list(range(len(patterns))) if group_of is None else list(group_of)
    terms, last = [], object()
    for p, g in zip(patterns, ids):
        if not p["needle"]:
            continue
        if g == last:
            terms[-1].append(p)
        else:
            terms.append([p])
        last = g
    return terms


_HITS = {}


def pattern_hits(p, haystacks, cfg):
    """{index: (score, exact)} of ONE pattern over the full list, its negation ignored (kept per list object: the lists are never changed)"""
    key = (id(haystacks), len(haystacks), repr(sorted(dict(p, negated=False).items(), key=str)), repr(sorted(cfg.items())))
    if key not in _HITS:
        _HITS[key] = (haystacks, _pattern_hits(p, haystacks, cfg))  # (the list is held, so its id stays its own)
    return _HITS[key][1]


def _pattern_hits(p, haystacks, cfg):
    om = O.MultiMatcher([dict(p, negated=False)], lanes=LANES, **dict(cfg, sort="IndexAsc"))
    return {int(r["index"]): (int(r["score"]), int(r["exact"])) for r in om.match_list(haystacks)}


def group_hits(alts, haystacks, cfg):
    """the union of the alternatives' hits: max score, exact from the max-scorers only"""
    out = {}
    for p in alts:
        for i, (s, e) in pattern_hits(p, haystacks, cfg).items():
            if i not in out or s > out[i][0]:
                out[i] = (s, e)
            elif s == out[i][0]:
                out[i] = (s, out[i][1] | e)
    return out


def compose(patterns, group_of, haystacks, **cfg):
    """the composed records in INDEX order (MATCH_DTYPE); cfg: make_config's keywords without `sort`"""
    cfg.pop("sort", None)
    alive = {i: (0, 0) for i in range(len(haystacks))}
    for t in terms_of(patterns, group_of):
        negated = len(t) == 1 and t[0]["negated"]
        hits = group_hits(t, haystacks, cfg)
        if negated:
            alive = {i: v for i, v in alive.items() if i not in hits}
        else:
            alive = {i: (min(0xFFFF, v[0] + hits[i][0]), v[1] | hits[i][1]) for i, v in alive.items() if i in hits}
    out = np.zeros(len(alive), O.MATCH_DTYPE)
    for k, i in enumerate(sorted(alive)):
        out[k] = (i, alive[i][0], alive[i][1], 0)
    return out


def ordered(recs, sort, by_score=True):
    """`Matcher::match_list`'s ordering step (src/matcher/mod.rs:212-222): reverse for the *Desc strategies, then the stable sort by descending
    score for the Score* ones (by_score False: a matcher with no compiled pattern is never sorted)"""
    r = recs[::-1] if sort in ("IndexDesc", "ScoreThenIndexDesc") else recs
    if by_score and sort in ("ScoreThenIndexAsc", "ScoreThenIndexDesc"):
        r = r[np.argsort(-r["score"].astype(np.int64), kind="stable")]
    return r.copy()


def match_list(patterns, group_of, haystacks, sort="ScoreThenIndexAsc", **cfg):
    return ordered(compose(patterns, group_of, haystacks, **cfg), sort, by_score=bool(terms_of(patterns, group_of)))
