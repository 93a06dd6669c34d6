"""The premise `frizbee_amd.NarrowingQuery` rests on, held to the oracle on the CPU.  For the compiled patterns P of the previous query and Q
of the new one, the rule "len(Q) >= len(P), every Q[i] refines P[i], Q != P" - a pattern refines when it is unchanged (negated or not) or is
a non-negated fuzzy 0-typo atom extended by a suffix - implies that `O.MultiMatcher(Q)`'s match set is a subset of `O.MultiMatcher(P)`'s: an
extended atom accepts less (tests/test_oracle_narrowing_premise.py), a further non-negated pattern intersects, a further negated one
subtracts, an unchanged negated one removes the same haystacks.  The class the rule refuses - a negated atom that changes - is shown NOT
to be monotone by a step the generators find, and the predicate is shown to refuse it and every other class outside the rule.  Host only:
the predicate is evaluated before anything is launched."""
import json
import os

import numpy as np
import pytest

import frizbee_amd as F
import oracle_lib as O
from ref_generators import api_cases
from test_gpu_parity import LANES, _expand
from test_oracle_narrowing_premise import CASINGS, ascii_needles

G = os.path.join(os.path.dirname(__file__), "golden")
MT = json.load(open(os.path.join(G, "matcher.json")))
KINDS = ("extended", "appended", "appended_negated", "unchanged_negated")


def match_set(pats, hs, lanes, casing):
    opats = [O.P(p.needle, negated=p.negated) for p in pats]
    return set(O.MultiMatcher(opats, lanes=lanes, max_typos=0, casing=casing, sort="IndexAsc").match_list(hs)["index"].tolist())


def host_query(config, max_fraction=1.0):
    """a NarrowingQuery without a device: only what the predicate reads"""
    nq = F.NarrowingQuery.__new__(F.NarrowingQuery)
    nq.config, nq.max_fraction, nq.within, nq._paths, nq._cur, nq._prev = config, max_fraction, None, {}, None, None

    class Gen:
        generation_now = 0

        def generation(self):
            return self.generation_now

        def __len__(self):
            return 10

    nq.corpus = Gen()
    return nq


def pairs_of(rng, atoms):
    """(kind, P, Q) for every kind the rule admits, from three atoms of at least two letters"""
    a, b, c = atoms
    k = int(rng.integers(1, len(a)))
    pat = F.Pattern
    yield "extended", [pat(a[:k])], [pat(a)]
    yield "appended", [pat(a[:k])], [pat(a[:k]), pat(b)]
    yield "appended_negated", [pat(a)], [pat(a), pat(c, negated=True)]
    yield "unchanged_negated", [pat(a[:k]), pat(c, negated=True)], [pat(a), pat(c, negated=True), pat(b[:1])]
    yield "unchanged_negated", [pat(c, negated=True), pat(a[:k])], [pat(c, negated=True), pat(a), pat(b, negated=True)]


def lists_of(pf):
    for _, hs, _ in api_cases(60, seed=300 + pf):
        if hs:
            yield hs
    for case in MT["cases"]:
        hs = _expand(case["haystacks"])
        if hs:
            yield hs


@pytest.mark.parametrize("pf", sorted(LANES))
@pytest.mark.parametrize("casing", CASINGS)
def test_the_rule_only_shrinks_the_match_set(pf, casing):
    rng = np.random.default_rng(17 * pf)
    nq = host_query(F.Config(pf_lanes=pf, sw_lanes=0, casing=F.CaseMatching[casing]))
    said = {k: 0 for k in KINDS}
    for hs in lists_of(pf):
        for _ in range(2):
            atoms = [s for s in ascii_needles(rng, hs, 6) if len(s) >= 2][:3]
            if len(atoms) < 3:
                continue
            for kind, P, Q in pairs_of(rng, atoms):
                cp, cq = nq.compile(P), nq.compile(Q)
                assert F.NarrowingQuery.rule(cp, cq), (kind, P, Q)  # generated to satisfy the rule
                before, after = match_set(P, hs, LANES[pf], casing), match_set(Q, hs, LANES[pf], casing)
                assert after <= before, (kind, P, Q, LANES[pf], casing, [hs[i] for i in sorted(after - before)[:3]])
                said[kind] += bool(before)
    assert sum(said.values()) >= 100 and all(v >= 10 for v in said.values()), said  # (P matched something, Q != P: the property had something to say)


def growing_step():
    """a list and a step `!x` -> `!xy` whose match set GROWS, searched in the generators"""
    for _, hs, _ in api_cases(60, seed=364):
        letters = sorted({c for h in hs for c in h if c.isascii() and c.isalnum()})
        for x in letters[:6]:
            for y in letters[:6]:
                P, Q = [F.Pattern(x, negated=True)], [F.Pattern(x + y, negated=True)]
                before, after = match_set(P, hs, LANES[64], "Smart"), match_set(Q, hs, LANES[64], "Smart")
                if after - before:
                    return hs, P, Q, before, after
    return None


def test_the_refused_class_is_not_monotone_and_the_predicate_refuses_it():
    found = growing_step()
    assert found is not None, "no growing negated step in the generators"
    hs, P, Q, before, after = found
    assert not after <= before
    cfg = F.Config(pf_lanes=64, sw_lanes=0)
    nq = host_query(cfg)
    rule = lambda p, q, c=None: F.NarrowingQuery.rule(nq.compile(p, c), nq.compile(q, c))  # noqa: E731
    pat = F.Pattern
    assert rule(P, Q) is False                                                                   # the step the oracle shows to grow
    assert rule([pat("dead"), pat("be")], [pat("deadb"), pat("be"), pat("x", negated=True)]) is True   # (the control: inside the rule)
    assert rule([pat("dead"), pat("t", negated=True)], [pat("deadb"), pat("t", negated=True)]) is True  # (an unchanged negated atom)
    assert rule([pat("dead")], [pat("dea")]) is False                                            # a shortened atom
    assert rule([pat("dead"), pat("be")], [pat("dead")]) is False                                # a removed atom
    assert rule([pat("dead"), pat("be")], [pat("be"), pat("dead")]) is False                     # (the same atoms in another order)
    assert rule([pat("dead"), pat("t", negated=True)], [pat("dead"), pat("te", negated=True)]) is False   # a changed negated atom
    assert rule([pat("dead"), pat("te", negated=True)], [pat("dead"), pat("t", negated=True)]) is False
    assert rule([pat("dead"), pat("t", negated=True)], [pat("deadb"), pat("t")]) is False         # (a negation taken away)
    assert rule([pat("dead")], [pat("dead")]) is False                                           # nothing changed
    assert rule([pat("dead"), pat("")], [pat("dead")]) is False                                  # (an empty needle is dropped first: nothing changed)
    assert rule([pat("dead", max_typos=1)], [pat("deadb", max_typos=1)]) is False                # a typo budget, per pattern ...
    typos = F.Config(pf_lanes=64, sw_lanes=0, max_typos=1)
    assert rule([pat("dead")], [pat("deadb")], typos) is False                                   # ... and inherited
    assert rule([pat("dead", max_typos=0)], [pat("deadb", max_typos=0)], typos) is True          # (the RESOLVED budget decides)
    for m in (F.Matching.Prefix, F.Matching.Suffix, F.Matching.Substring, F.Matching.Exact):
        assert rule([pat("foo", matching=m)], [pat("foob", matching=m)]) is False                # a literal-mode atom
    assert [p.matching for p in F.parse_query("^foo")] == [F.Matching.Prefix]
    assert rule(F.parse_query("^foo"), F.parse_query("^foob")) is False
    assert rule([pat("dead")], [pat("deadb", casing=F.CaseMatching.Respect)]) is False           # another field of the pattern
    smart = F.Config(pf_lanes=64, sw_lanes=0, unicode=F.UnicodeMatching.Smart)
    assert rule([pat("k")], [pat("ké")], smart) is False                                         # a changed unicode path
    old, new = nq.compile([pat("dead")])[0], nq.compile([pat("deadb")])[0]
    assert F.NarrowingQuery.refines(old, new) is True
    assert F.NarrowingQuery.refines(old, (new[0], new[1], (new[2][0], new[2][1], new[2][2] // 2))) is False   # a changed lane pair
    # the state around the patterns: a previous query that the rule admits, then a changed config / generation / `within`
    P2, Q2 = nq.compile([pat("dead")]), nq.compile([pat("deadb")])
    nq._cur, nq._prev = 0, (P2, F.Config(pf_lanes=64, sw_lanes=0, sort=F.SortStrategy.IndexAsc), 0, None)
    assert nq._may_narrow(Q2) is False                                                           # a changed config
    nq._prev = (P2, F.Config(pf_lanes=64, sw_lanes=0), 0, None)
    nq.corpus.generation_now = 1
    assert nq._may_narrow(Q2) is False                                                           # a changed generation
    nq.corpus.generation_now = 0
    nq._prev = (P2, F.Config(pf_lanes=64, sw_lanes=0), 0, (1234, 0))
    assert nq._may_narrow(Q2) is False                                                           # a changed `within`
    nq._prev = (nq.compile([pat("dead"), pat("t", negated=True)]), F.Config(pf_lanes=64, sw_lanes=0), 0, None)
    assert nq._may_narrow(nq.compile([pat("dead"), pat("te", negated=True)])) is False            # the refused class through the same door
    nq._cur = None
    assert nq._may_narrow(Q2) is False                                                           # no previous capture
