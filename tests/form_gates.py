"""TEST INFRASTRUCTURE: the host's form gates, transcribed.  The library picks each scorer's arithmetic form and the ordering's pass count from
bounds it computes out of the scoring and the needle's rows (frizbee_amd/csrc/host.hip: set_scorer_forms, build_long_needle, fzb_order_flags).
This file restates those bounds in plain Python - the reference's Scoring::max_per_char_bonus / max_one_time_bonus / guard_against_score_overflow
(src/lib.rs:480-537), the score ceiling the gates stand on and the gate expressions - and generates GATE SCORINGS: scorings whose gate expression is exactly T - 1 (the last value
inside the gate) and exactly T (the first outside).  Nothing here imports the library: a test that asks the library which form ran compares it with
what this file says.

A scoring is the list [match_score, mismatch_penalty, gap_open_penalty, gap_extend_penalty, prefix_bonus, capitalization_bonus,
matching_case_bonus, exact_match_bonus, delimiter_bonus] (the order of fzb_scoring and of the oracle)."""

DEFAULT = [12, 6, 5, 1, 12, 4, 4, 8, 4]
MATCH, MISMATCH, GAP_OPEN, GAP_EXTEND, PREFIX, CAPITALIZATION, MATCHING_CASE, EXACT, DELIMITER = range(9)
U16 = 0xFFFF
F16_INF = 0x7C00  # the first pattern that is no finite binary16: v_pk_maximum3_f16 is an integer maximum only below it


def sadd16(a, b):
    return min(a + b, U16)


def ssub16(a, b):
    return max(a - b, 0)


def _amortized(sc):
    bonus = max(sc[DELIMITER], sc[CAPITALIZATION])
    return bonus, max((bonus + 1) // 2, ssub16(bonus, sc[GAP_OPEN]))


def max_per_char_bonus(sc):
    _, amortized = _amortized(sc)
    return sadd16(amortized, sc[MATCHING_CASE])


def max_one_time_bonus(sc):
    bonus, amortized = _amortized(sc)
    return bonus - amortized


def max_matrix_score(sc, rows):
    return (sc[MATCH] + max_per_char_bonus(sc)) * rows + max_one_time_bonus(sc) + sc[PREFIX]


def score_ceiling(sc, rows):
    """what a matrix cell can really reach: match + the larger per-letter bonus + the case bonus per row, the prefix bonus once.  The gates stood on
    max_matrix_score (the reference's guard, which amortises the per-letter bonus) until tests/test_form_gates_host.py found needles that beat it:
    THE_REFERENCE_BOUND_IS_BEATEN below."""
    return (sc[MATCH] + max(sc[DELIMITER], sc[CAPITALIZATION]) + sc[MATCHING_CASE]) * rows + sc[PREFIX]


# (scoring, needle == haystack, the oracle's score): delimiter, lowercase behind it, capital behind the lowercase - two rows of every three earn
# the per-letter bonus with no gap, where the reference's guard allows for one of two.  Default scoring: 132 > M + exact = 130.
THE_REFERENCE_BOUND_IS_BEATEN = (DEFAULT, b"/aA/aA", 132)


def overflow_guard_ok(sc, rows):
    """Scoring::guard_against_score_overflow with the fuzzy matcher's amortised bonuses: True where the reference accepts needle and scoring"""
    max_per_char = sadd16(sc[MATCH], max_per_char_bonus(sc))
    if max_per_char == 0:
        return True
    headroom = ssub16(ssub16(ssub16(ssub16(U16, sc[PREFIX]), sc[EXACT]), sc[MISMATCH]), max_one_time_bonus(sc))
    return rows <= headroom // max_per_char and 32 * sc[GAP_EXTEND] + sc[GAP_OPEN] <= U16


# ---- the six gates: (lanes of gap_extend in the bound, threshold T); a gate's bound clause holds <=> expression < T ---------------------------
GATES = ("cf", "cfm", "cfm_long", "bias", "cfu", "one_pass")
THRESHOLD = {"cf": F16_INF, "cfm": F16_INF, "cfm_long": F16_INF, "bias": U16 + 1, "cfu": U16 + 1, "one_pass": 256}
LONG_LDS_ROWS = 1024  # the long-needle four-lane scorer stages at most this many rows


def gap_lanes(gate, rows):
    return {"cf": 130, "cfm": 200, "cfm_long": 137 + rows, "bias": 130, "cfu": 130}[gate]


def expression(gate, sc, rows):
    """the left side of the gate's bound as host.hip writes it"""
    if gate == "one_pass":
        return score_ceiling(sc, rows) + sc[EXACT]
    return score_ceiling(sc, rows) + sc[MISMATCH] + gap_lanes(gate, rows) * sc[GAP_EXTEND] + 64


def gap_clause(sc):
    return 2 * sc[GAP_EXTEND] <= sc[MISMATCH]


def cf_ok(sc, rows, pad_ok=True):
    return pad_ok and gap_clause(sc) and expression("cf", sc, rows) < F16_INF


def cfm_ok(sc, rows):
    return gap_clause(sc) and expression("cfm", sc, rows) < F16_INF


def cfm_long_ok(sc, rows):
    return rows <= LONG_LDS_ROWS and gap_clause(sc) and expression("cfm_long", sc, rows) < F16_INF


def bias_ok(sc, rows):
    return expression("bias", sc, rows) <= U16


def cfu_ok(sc, rows):
    return bias_ok(sc, rows) and gap_clause(sc)


def one_pass(sc, rows, sum_scores=False, literal_mode=False, bias_hi=0):
    return not sum_scores and not literal_mode and expression("one_pass", sc, rows) + bias_hi < 256


def gate(name, sc, rows, pad_ok=True):
    return {"cf": lambda: cf_ok(sc, rows, pad_ok), "cfm": lambda: cfm_ok(sc, rows), "cfm_long": lambda: cfm_long_ok(sc, rows), "bias": lambda: bias_ok(sc, rows),
            "cfu": lambda: cfu_ok(sc, rows), "one_pass": lambda: one_pass(sc, rows)}[name]()


def forms(sc, rows, pad_ok=True):
    """every gate of a short needle (rows <= 63) or a long one, by name"""
    names = ("cfm_long", "bias", "one_pass") if rows > 63 else ("cf", "cfm", "bias", "cfu", "one_pass")
    return {n: gate(n, sc, rows, pad_ok) for n in names}


# ---- gate scorings ----------------------------------------------------------------------------------------------------------------------------
FAMILIES = ("score", "gap")


def _with_prefix(base, gate_name, rows, target):
    """`base` with the prefix bonus - which enters score_ceiling one for one - set so that the gate's expression is `target`"""
    sc = list(base)
    sc[PREFIX] = 0
    sc[PREFIX] = target - expression(gate_name, sc, rows)
    assert 0 <= sc[PREFIX] <= U16 and expression(gate_name, sc, rows) == target, (gate_name, rows, target, sc)
    return sc


def _score_base(gate_name, rows, T):
    """SCORE-DOMINATED: one point of gap_extend (cf, cfm: so that the 70 lanes between their bounds keep the other gate on one side), the needle's
    rows worth nearly all of T.  gap_open = gap_extend = 1, so a haystack with every needle letter capitalised behind a delimiter earns
    match + bonus + case per row less one point per gap: a cell within `rows` points of the ceiling exists.
    The `bias` gate takes 2 * gap_extend > mismatch_penalty here, which keeps cfu_ok (and every 0x7C00 gate) false on both sides."""
    if gate_name == "one_pass":
        # no delimiter / capitalisation bonus: ceiling + exact = rows * (match + case) + prefix + exact, and a haystack equal to the needle scores exactly that
        case = 4
        match = (T - 1 - 8 - 12) // rows - case
        return [match, 6, 5, 1, 0, 0, case, 8, 0]
    gex, mismatch = (2, 3) if gate_name == "bias" else (1, 6)
    bonus, case = 30, 20
    fixed = mismatch + gap_lanes(gate_name, rows) * gex + 64
    match = (T - 1 - fixed - 12) // rows - bonus - case
    return [match, mismatch, gex, gex, 0, bonus, case, 8, bonus]


def _gap_base(gate_name, rows, T):
    """GAP-DOMINATED: the default scores and bonuses, gap_extend as large as the bound allows with mismatch_penalty = 2 * gap_extend (the clause's
    edge) and gap_open = gap_extend + 4 (the default's surcharge): the lane bias, not the score, carries the operand."""
    assert gate_name != "one_pass"
    sc = list(DEFAULT)
    sc[PREFIX] = 0
    fixed = score_ceiling(sc, rows) + 64
    gex = (T - 1 - fixed - DEFAULT[PREFIX]) // (gap_lanes(gate_name, rows) + 2)
    gex = min(gex, (U16 - 4) // 33)  # the reference's own guard: 32 * gap_extend + gap_open <= 65535
    sc[GAP_EXTEND], sc[MISMATCH], sc[GAP_OPEN] = gex, 2 * gex, gex + 4
    return sc


def gate_scorings(gate_name, rows, family):
    """(scoring with the gate's expression == T - 1, scoring with it == T): equal but for one point of prefix bonus"""
    T = THRESHOLD[gate_name]
    base = (_score_base if family == "score" else _gap_base)(gate_name, rows, T)
    inside, outside = _with_prefix(base, gate_name, rows, T - 1), _with_prefix(base, gate_name, rows, T)
    assert outside[PREFIX] == inside[PREFIX] + 1 and inside[:PREFIX] + inside[PREFIX + 1:] == outside[:PREFIX] + outside[PREFIX + 1:]
    for sc in (inside, outside):
        assert overflow_guard_ok(sc, rows), (gate_name, rows, family, sc)
    assert gate(gate_name, inside, rows) and not gate(gate_name, outside, rows), (gate_name, rows, family, inside, outside)
    # every OTHER gate sits on the same side at T - 1 and at T, except cfu_ok, which is bias_ok and the gap clause: it follows a `bias` scoring
    # whose clause holds, and a `cfu` scoring is such a one
    a, b = forms(inside, rows), forms(outside, rows)
    moved = {n for n in a if a[n] != b[n]}
    assert moved <= ({gate_name} | ({"bias", "cfu"} if gate_name in ("bias", "cfu") else set())), (gate_name, rows, family, moved)
    return inside, outside


def clause_scorings(gate_name, rows):
    """the 2 * gap_extend <= mismatch_penalty clause of cf / cfm / cfm_long / cfu at its edge: (2 * gex == mismatch, 2 * gex == mismatch + 1), the
    gate's bound far inside (default scores, gap_extend 3)"""
    inside = list(DEFAULT)
    inside[GAP_EXTEND], inside[MISMATCH] = 3, 6
    outside = list(inside)
    outside[MISMATCH] = 5
    assert gate(gate_name, inside, rows) and not gate(gate_name, outside, rows)
    assert overflow_guard_ok(inside, rows) and overflow_guard_ok(outside, rows)
    return inside, outside


def bound_scoring(rows, bound):
    """score_ceiling + exact_match_bonus == bound exactly, with no delimiter / capitalisation bonus: a haystack equal to the needle (lowercase letters) scores
    exactly `bound`, so the ordering gate's bound is one that lists realise"""
    base = _score_base("one_pass", rows, 256)
    sc = _with_prefix(base, "one_pass", rows, bound)
    assert overflow_guard_ok(sc, rows)
    return sc


def dense_bonus_case(gate_name):
    """named case (cf, cfm): 63 rows of "/aA" under a per-letter bonus of 300 that a gap costs in full.  The reference's guard amortises that bonus to
    150 a row, the needle earns 200.  -> (needle, the last scoring inside the gate while it stood on max_matrix_score - p_max3_s was given operands
    up to 0x8766 there -, the last scoring inside the gate as it stands on score_ceiling)"""
    rows, needle = 63, b"/aA" * 21
    before = {"cf": [328, 6, 300, 1, 19, 300, 20, 8, 300], "cfm": [327, 6, 300, 1, 12, 300, 20, 8, 300]}[gate_name]
    assert max_matrix_score(before, rows) + before[MISMATCH] + gap_lanes(gate_name, rows) * before[GAP_EXTEND] + 64 == F16_INF - 1
    assert gap_clause(before) and not gate(gate_name, before, rows) and overflow_guard_ok(before, rows)
    base = list(before)
    base[MATCH] = 0
    base[MATCH] = (F16_INF - 1 - expression(gate_name, base, rows)) // rows
    now = _with_prefix(base, gate_name, rows, F16_INF - 1)
    assert gate(gate_name, now, rows) and overflow_guard_ok(now, rows)
    return needle, before, now
