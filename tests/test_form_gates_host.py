"""The premise behind each form gate, searched on the CPU.  The host picks dp_cf.h / dp_cfm.h / dp_quad.h (whose three-way maximum is
v_pk_maximum3_f16 on integer patterns: exact only below 0x7C00) from a bound of its own: the largest biased operand is at most
C + mismatch + k * gap_extend + 64 with C the score ceiling (rows * (match + per-letter bonus + case) + prefix) and k = 130 (cf_ok), 200 (cfm_ok) or 137 + rows (the long needle's cfm_ok).  Here the scorings that sit
exactly ON each bound (tests/form_gates.py: expression == T - 1, both families) run through the host-compiled device arithmetic
(tests/kernel_host) on inputs that push the operands up (tests/form_gate_lists.py), with dp_body.h's precondition meter recording what
p_max3_s was given.  Asserted: the score is the oracle's, no operand reached 0x7C00, and one more point of prefix bonus (T) closes the gate.
Printed, not asserted: the largest operand per gate and 0x7C00 minus it - the gate's measured slack ("Form gates").

The biased forms behind bias_ok (the template flag of dp_single_chunk / dp_multi_chunk) get the same treatment with the meter's p_add wrap
count: at expression == 0xFFFF no 16-bit lane may wrap.

Second premise, from the oracle alone: fzb_order_flags trusts that no score exceeds C + exact_match_bonus.  (Both premises failed with the
reference's amortised bound M in C's place: the named cases at the end.)"""
import ctypes as C
import random
import zlib

import pytest

import form_gate_lists as L
import form_gates as G
import kernel_host_lib as K
import oracle_lib as O

pytestmark = pytest.mark.skipif(not K.available(), reason="ROCm clang++ not installed")


def _fits(n, sc):
    return bool(O.lib().fzo_score_fits_in_u8(n, (C.c_uint16 * 9)(*sc)))


def _inputs(rng, needle, widths, lanes, randoms):
    """(window, whether the four-lane harness takes it too): four host threads in lockstep cost milliseconds per window, so they take the built
    windows with the delimiter fill - at 1024 bytes the first two - and the thread-per-window forms take everything"""
    for w in widths:
        if w < len(needle):  # (a window shorter than the needle: what a typo budget admits) its head, its tail and the search
            for h in [needle[:w], needle[-w:]] + L.random_windows(rng, needle, w, randoms):
                yield h, False
            continue
        for fill in (b"_", b"a"):
            for i, h in enumerate(L.adversarial(needle, w, lanes, fill)):
                yield h, fill == b"_" and (w < 1024 or i < 2)
        for h in L.random_windows(rng, needle, w, randoms):
            yield h, False


def _needles(rng, rows):
    """the capital needle (every letter earns the case bonus; behind a delimiter or a lowercase letter the per-letter bonus too), the needle that
    beat the reference's amortised bound (delimiter, lowercase, capital: two rows of three earn the bonus with no gap) and a seeded random one"""
    return [L.capital_needle(rows), (b"/aA" * rows)[:rows], L.random_needle(rng, rows)]


class Slack:
    """largest p_max3_s operand per gate over the module's runs"""
    seen = {}

    @classmethod
    def note(cls, gate, family, rows, swl, sc):
        hi, bad, _ = K.meter_read()
        key = (gate, family)
        if hi > cls.seen.get(key, (-1,))[0]:
            cls.seen[key] = (hi, rows, swl, sc)
        return hi, bad


def _run_forms(gate, needle, hay, sc, swl, u8, quad=True):
    """{form name: score} of every host-compiled form the gate selects that takes this window"""
    cs = any(65 <= c <= 90 for c in needle)  # smart case
    m, n, nw = len(hay), len(needle), swl // 2
    got = {}
    if gate == "cf":  # dp_cf.h, one chunk: the narrowest class of computed lanes that holds the window and the full chunk; the short kernel's table form
        for real in sorted({r for r in (nw // 4, nw // 2, 3 * nw // 4, nw) if m <= 2 * r}):
            got["dp_cf real=%d" % real] = K.dp_single(needle, hay, sc, cs, True, swl, 3, real)
        if m <= swl // 2:
            got["dp_cf tab"] = K.dp_single(needle, hay, sc, cs, True, swl, 4, 0)
    elif gate == "cfm":  # dp_cfm.h chunk by chunk (slab and LDS pitch, the last chunk's padding in closed form) and dp_quad.h in its three layouts
        if m > swl:
            for form in (6, 7, 8, 16, 17, 18):
                got["dp_cfm form=%d" % form] = K.dp_multi(needle, hay, sc, cs, True, swl, form, u8)
        for form in (0, 1, 2) if quad else ():
            if form == 2 and n < 2:  # (one row: the host threads have no exchange between a park and its read)
                continue
            got["dp_quad form=%d" % form] = K.dp_quad(needle, hay, sc, cs, True, swl, form, u8, False)
    else:  # cfm_long: the long needle's rows through dp_cfm.h and dp_quad.h (NeedleLongRows)
        got["dp_cfm long"] = K.dp_multi_long(needle, hay, sc, cs, True, swl, 6, u8)
        for form in (0, 1, 2) if quad else ():
            got["dp_quad long form=%d" % form] = K.dp_quad(needle, hay, sc, cs, True, swl, form, u8, True)
    return cs, got


def _widths(gate, swl, rows):
    """the windows of a gate's forms; `rows` itself among them: the haystack that equals the needle"""
    if gate == "cf":
        return sorted({1, 2, swl // 4, swl // 4 + 1, swl // 2, swl // 2 + 1, 3 * swl // 4, swl - 1, swl} | ({rows} if rows <= swl else set()))
    if gate == "cfm":
        return sorted({1, rows, swl // 2, swl} | set(L.windows_of(swl)))
    return sorted({rows, 256, 257, 1024} | set(L.windows_of(swl)[:6]))


CASES = [(g, fam, rows, swl) for g, rws in (("cf", (1, 2, 13, 63)), ("cfm", (1, 2, 13, 63)), ("cfm_long", (65, 130))) for fam in G.FAMILIES for rows in rws for swl in (64, 32)]


@pytest.mark.parametrize("gate,family,rows,swl", CASES, ids=["%s-%s-%d-%d" % c for c in CASES])
def test_no_operand_reaches_0x7c00_on_the_gates_last_scoring(gate, family, rows, swl):
    inside, outside = G.gate_scorings(gate, rows, family)
    assert G.expression(gate, inside, rows) == G.THRESHOLD[gate] - 1 and G.gate(gate, inside, rows)
    assert G.expression(gate, outside, rows) == G.THRESHOLD[gate] and not G.gate(gate, outside, rows)  # at T the gate is closed
    rng = random.Random(zlib.crc32(repr((gate, family, rows, swl)).encode()))
    u8 = _fits(rows, inside)
    randoms = 2 if gate != "cf" else 12
    K.meter_reset()
    checked = 0
    for needle in _needles(rng, rows):
        assert L.oracle_accepts(needle, inside) and L.oracle_accepts(needle, outside)
        for hay, quad in _inputs(rng, needle, _widths(gate, swl, rows), swl, randoms):
            cs, got = _run_forms(gate, needle, hay, inside, swl, u8, quad)
            want = O.sw_score(needle, hay, scoring=inside, case_sensitive=cs, include_prefix=True, lanes=swl, is_u8=u8)
            for form, score in got.items():
                assert score == want, (gate, family, rows, swl, inside, needle, hay, form, score, want)
            checked += len(got)
    hi, bad = Slack.note(gate, family, rows, swl, inside)
    print("form gate %-8s %-5s rows %3d lanes %2d: scoring %s, %d runs, largest p_max3_s operand 0x%04X, slack 0x7C00 - it = %d" % (gate, family, rows, swl, inside, checked, hi, 0x7C00 - hi))
    assert checked >= 50
    assert bad == 0, (gate, family, rows, swl, inside, "p_max3_s was given an operand >= 0x7C00", hex(hi), bad)


def test_the_measured_slack_of_each_gate():
    """the table DESIGN.md quotes (run after the cases above; asserts nothing about the values)"""
    for (gate, family), (hi, rows, swl, sc) in sorted(Slack.seen.items()):
        print("slack %-8s %-5s: largest operand 0x%04X = %5d (rows %d, lanes %d, scoring %s), 0x7C00 - it = %d" % (gate, family, hi, hi, rows, swl, sc, 0x7C00 - hi))


# (cfu_ok is a short needle's gate; its scorings are bias_ok's with the gap clause true: the same first forms run under both)
BIAS_CASES = [(g, fam, rows, swl) for g, rws in (("bias", (1, 13, 63, 65, 130)), ("cfu", (1, 13, 63))) for fam in G.FAMILIES for rows in rws for swl in (64, 32)]


@pytest.mark.parametrize("gate,family,rows,swl", BIAS_CASES, ids=["%s-%s-%d-%d" % c for c in BIAS_CASES])
def test_no_16_bit_lane_wraps_in_the_biased_gap_scan_on_bias_oks_last_scoring(gate, family, rows, swl):
    """dp_body.h's first forms with BIAS = true (what bias_ok selects in k2b_dp, k2d_dp_multi and k2d_dp_long): expression == 0xFFFF"""
    inside, outside = G.gate_scorings(gate, rows, family)
    assert G.bias_ok(inside, rows) and not G.bias_ok(outside, rows)
    rng = random.Random(zlib.crc32(repr((gate, family, rows, swl)).encode()))
    u8 = _fits(rows, inside)
    K.meter_reset()
    checked = 0
    widths = sorted({1, swl // 2, swl, 256, 257} | set(L.windows_of(swl)))
    for needle in _needles(rng, rows)[:2]:
        assert L.oracle_accepts(needle, inside)
        cs = any(65 <= c <= 90 for c in needle)
        for hay, _ in _inputs(rng, needle, widths, swl, 2):
            want = O.sw_score(needle, hay, scoring=inside, case_sensitive=cs, include_prefix=True, lanes=swl, is_u8=u8)
            if rows > 63:
                got = K.dp_multi_long(needle, hay, inside, cs, True, swl, 5, u8)
            elif len(hay) <= swl:
                got = K.dp_single(needle, hay, inside, cs, True, swl, 0, 0)
            else:
                got = K.dp_multi(needle, hay, inside, cs, True, swl, 5, u8)
            assert got == want, (gate, family, rows, swl, inside, needle, hay, got, want)
            checked += 1
    _, _, wraps = K.meter_read()
    print("form gate %-4s %-5s rows %3d lanes %2d: scoring %s, %d runs, p_add lane wraps %d" % (gate, family, rows, swl, inside, checked, wraps))
    assert checked > 50
    assert wraps == 0, (gate, family, rows, swl, inside, wraps)


BOUND_ROWS = (1, 6, 12)


def test_no_oracle_score_exceeds_the_bound_one_pass_trusts():
    """score_ceiling + exact_match_bonus against a seeded search, rows 1..13: the default scoring and the scorings whose bound is exactly 255 / 256.
    The same search beat the bound one_pass stood on before (the reference's max_matrix_score + exact_match_bonus): the first column of the table."""
    print()
    beaten = 0
    for rows in range(1, 14):
        scorings = [("default", G.DEFAULT)] + ([("bound 255", G.bound_scoring(rows, 255)), ("bound 256", G.bound_scoring(rows, 256))] if rows in BOUND_ROWS else [])
        for name, sc in scorings:
            bound, ref_bound = G.expression("one_pass", sc, rows), G.max_matrix_score(sc, rows) + sc[G.EXACT]
            best, needle, hay = L.best_score_search(sc, rows)
            print("rows %2d %-9s %s: best oracle score %3d (needle %r in %r), reference's M + exact = %3d, ceiling + exact = %3d" % (rows, name, sc, best, needle, hay, ref_bound, bound))
            assert 0 <= best <= bound, (rows, name, sc, best, bound, needle, hay)
            beaten += best > ref_bound
            if name != "default":  # these scorings are built so that a list REALISES the bound (tests/test_gpu_form_gates.py stands on it)
                assert best == bound, (rows, name, sc, best, bound)
    assert beaten > 0  # (what moved the gates off max_matrix_score)
    assert G.expression("one_pass", G.DEFAULT, 11) == 240 and G.expression("one_pass", G.DEFAULT, 12) == 260
    assert G.one_pass(G.DEFAULT, 11) and not G.one_pass(G.DEFAULT, 12)


def test_the_needle_that_beat_the_references_bound():
    """named case: "/aA/aA" under the default scoring scores 132 where the reference's guard allows for M + exact = 130 - the input that showed
    fzb_order_flags (and every 0x7C00 gate) a bound that was none"""
    sc, needle, score = G.THE_REFERENCE_BOUND_IS_BEATEN
    recs = O.Matcher(needle, scoring=sc).match_list([needle])
    assert recs["score"].tolist() == [score] and recs["exact"].tolist() == [1]
    assert G.max_matrix_score(sc, len(needle)) + sc[G.EXACT] == 130 < score <= G.expression("one_pass", sc, len(needle))


@pytest.mark.parametrize("gate", ("cf", "cfm"))
def test_the_dense_bonus_needle_inside_the_gates_as_they_stand_now(gate):
    """named case: 63 rows of "/aA" under a per-letter bonus of 300 that a gap costs in full.  The reference's guard amortises that bonus to 150 a
    row, the needle earns 200: with the gates on max_matrix_score the scoring BEFORE sat inside cf_ok / cfm_ok and p_max3_s was given operands up to
    0x8720.  On score_ceiling that scoring is outside, and the scoring that is now the gate's last keeps every operand below 0x7C00."""
    needle, before, now = G.dense_bonus_case(gate)
    assert L.oracle_accepts(needle, now) and L.oracle_accepts(needle, before)
    for sc, violations in ((before, True), (now, False)):
        K.meter_reset()
        for swl in (64, 32):
            for hay in (needle, b"x" * (swl + 7) + needle, needle + b"x" * (3 * swl - 62)):
                if gate == "cf" and len(hay) > swl:
                    continue
                cs, got = _run_forms(gate, needle, hay, sc, swl, False)
                want = O.sw_score(needle, hay, scoring=sc, case_sensitive=cs, include_prefix=True, lanes=swl, is_u8=False)
                assert got and all(v == want for v in got.values()), (gate, sc, hay, got, want)  # (the host's plain maximum is right either way)
        hi, bad, _ = K.meter_read()
        print("dense-bonus needle, %s, scoring %s: largest p_max3_s operand 0x%04X, calls with an operand >= 0x7C00: %d" % (gate, sc, hi, bad))
        assert (bad > 0) == violations, (gate, sc, hex(hi), bad)
