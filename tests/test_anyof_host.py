"""frizbee_amd/csrc/anyof.h on the host (tests/kernel_host/anyof_host.cpp): the key pack, the max-combine, the unpack and the saturating
join against a numpy model written here, the combine's independence of the alternatives' order, and a whole group - clear, accumulate per
alternative, flag, compact - over slot arrays around the wave, the tile and two tiles, in its three forms (later group, base group over a
range, base group over a candidate set) and with grids of several sizes, against the union computed in numpy."""
import itertools
import subprocess

import numpy as np
import pytest

import anyof_host_lib as A

pytestmark = pytest.mark.skipif(not A.available(), reason="ROCm clang++ not installed")
REC = np.dtype([("index", "<u4"), ("score", "<u2"), ("exact", "u1"), ("_pad", "u1")])
SIZES = (1, 63, 64, 65, 1023, 1024, 1025, 2049)


def u32(a):
    return np.ascontiguousarray(a, dtype=np.uint32)


def pack(score, exact):
    score, exact, out = u32(score), u32(exact), np.zeros(len(score), np.uint32)  # (named: alive across the call)
    A.lib().aoh_pack(score.ctypes.data, exact.ctypes.data, len(score), out.ctypes.data)
    return out


def unpack(key):
    hit, score, exact = (np.zeros(len(key), np.uint32) for _ in range(3))
    key = u32(key)
    A.lib().aoh_unpack(key.ctypes.data, len(key), hit.ctypes.data, score.ctypes.data, exact.ctypes.data)
    return hit, score, exact


def combine(a, b):
    a, b, out = u32(a), u32(b), np.zeros(len(a), np.uint32)
    A.lib().aoh_combine(a.ctypes.data, b.ctypes.data, len(a), out.ctypes.data)
    return out


def model_union(scores, exacts, hit):
    """[alt][item] -> (any hit, max score of the hitting alternatives, OR of the exact flags of those that reach it)"""
    s = np.where(hit, scores, -1).astype(np.int64)
    best = s.max(axis=0)
    exact = (hit & (s == best) & (exacts != 0)).any(axis=0)
    return hit.any(axis=0), np.where(best < 0, 0, best), exact


def test_pack_unpack_and_the_zero_key():
    rng = np.random.default_rng(1)
    score = np.concatenate([rng.integers(0, 65536, 5000), [0, 0, 65535, 65535]])
    exact = np.concatenate([rng.integers(0, 2, 5000), [0, 1, 0, 1]])
    key = pack(score, exact)
    assert (key == (0x80000000 | (score.astype(np.uint32) << 1) | exact.astype(np.uint32))).all()
    hit, s, e = unpack(key)
    assert hit.all() and (s == score).all() and (e == exact).all()
    assert (key != 0).all()  # a hit of score 0 without the exact flag is still a hit
    hit, s, e = unpack(np.zeros(3, np.uint32))
    assert not hit.any() and not s.any() and not e.any()  # key 0 = no alternative hit
    assert A.lib().aoh_alts_max() == 8


def test_combine_is_the_rule_and_does_not_depend_on_the_order():
    rng = np.random.default_rng(2)
    n = 4000
    for k in range(2, 9):
        scores = rng.integers(0, 40, (k, n))  # few values: ties at the maximum are common
        scores[:, : n // 8] = rng.integers(0, 65536, (k, n // 8))
        exacts = rng.integers(0, 2, (k, n))
        hit = rng.random((k, n)) < 0.5
        keys = [np.where(hit[a], pack(scores[a], exacts[a]), 0).astype(np.uint32) for a in range(k)]
        any_hit, best, exact = model_union(scores, exacts, hit)
        assert ((hit.sum(axis=0) > 1) & exact & ~np.where(hit, exacts, 1).all(axis=0)).any()  # exact taken from a max-scorer while another alternative has none
        perms = list(itertools.permutations(range(k))) if k <= 4 else [rng.permutation(k).tolist() for _ in range(30)]
        for perm in perms:
            acc = np.zeros(n, np.uint32)
            for a in perm:
                acc = combine(acc, keys[a])
            h, s, e = unpack(acc)
            assert (h.astype(bool) == any_hit).all() and (s == best)[any_hit].all() and (e.astype(bool) == exact)[any_hit].all(), (k, perm)
    # associativity on raw keys
    a, b, c = (pack(rng.integers(0, 8, 3000), rng.integers(0, 2, 3000)) for _ in range(3))
    assert (combine(combine(a, b), c) == combine(a, combine(b, c))).all() and (combine(a, b) == combine(b, a)).all()


def test_the_join_saturates_at_65535_and_ors_the_flags():
    rng = np.random.default_rng(3)
    cs = np.concatenate([rng.integers(0, 65536, 4000), [65535, 0, 65535, 32768, 32767]])
    gs = np.concatenate([rng.integers(0, 65536, 4000), [65535, 0, 0, 32768, 32768]])
    ce, ge = rng.integers(0, 2, len(cs)), rng.integers(0, 2, len(cs))
    score, exact = np.zeros(len(cs), np.uint32), np.zeros(len(cs), np.uint32)
    cs32, ce32, key = u32(cs), u32(ce), pack(gs, ge)
    A.lib().aoh_join(cs32.ctypes.data, ce32.ctypes.data, key.ctypes.data, len(cs), score.ctypes.data, exact.ctypes.data)
    assert (score == np.minimum(cs + gs, 65535)).all() and (exact == (ce | ge)).all()
    assert (score == 65535).sum() > 1000 and (score < 65535).sum() > 1000


def test_find():
    rng = np.random.default_rng(4)
    for n in (0, 1, 2, 63, 1025):
        lst = np.sort(rng.choice(5 * n + 5, n, replace=False)).astype(np.uint32)
        vals = np.arange(5 * n + 7, dtype=np.uint32)
        out = np.zeros(len(vals), np.uint32)
        A.lib().aoh_find(lst.ctypes.data, n, vals.ctypes.data, len(vals), out.ctypes.data)
        where = {int(v): i for i, v in enumerate(lst)}
        assert out.tolist() == [where.get(int(v), n) for v in vals]


@pytest.mark.parametrize("form", ("later", "range", "set"))
@pytest.mark.parametrize("n", SIZES)
def test_a_whole_group_against_the_union_in_numpy(n, form):
    rng = np.random.default_rng(n * 3 + len(form))
    offset = 0 if form == "later" else 1000
    items = np.sort(rng.choice(4 * n + 3, n, replace=False)).astype(np.uint32)
    cand = np.zeros(n, REC)
    cand["index"] = np.sort(rng.choice(6 * n + 3, n, replace=False))
    cand["score"] = rng.integers(0, 65536, n)
    cand["score"][: n // 3] = rng.integers(60000, 65536, n // 3)  # joins that saturate
    cand["exact"] = rng.integers(0, 2, n)
    index_of = cand["index"] if form == "later" else offset + (items if form == "set" else np.arange(n))
    for k, density, grid in ((2, 0.5, 1), (8, 0.2, 2), (3, 0.0, 5), (4, 1.0, 3), (8, 0.03, 70)):
        hit = rng.random((k, n)) < density
        scores, exacts = rng.integers(0, 30 if k % 2 == 0 else 65536, (k, n)), rng.integers(0, 2, (k, n))
        chunks, n_hits = [], []
        for a in range(k):
            at = rng.permutation(np.flatnonzero(hit[a]))  # any order: the fold does not rely on it
            h = np.zeros(len(at), REC)
            h["index"], h["score"], h["exact"] = index_of[at], scores[a][at], exacts[a][at]
            chunks.append(h)
            n_hits.append(len(at))
        hits = np.ascontiguousarray(np.concatenate(chunks)) if chunks else np.zeros(0, REC)
        out = np.full(n + 1, 0xAB, np.uint8).repeat(8).view(REC).copy()
        counts = u32(n_hits)
        got = A.lib().aoh_group(hits.ctypes.data if len(hits) else None, counts.ctypes.data, k, n, offset, items.ctypes.data if form == "set" else None,
                                cand.ctypes.data if form == "later" else None, grid, out.ctypes.data)
        any_hit, best, exact = model_union(scores, exacts, hit)
        want = np.zeros(int(any_hit.sum()), REC)
        want["index"] = index_of[any_hit]
        if form == "later":
            want["score"] = np.minimum(cand["score"][any_hit].astype(np.int64) + best[any_hit], 65535)
            want["exact"] = cand["exact"][any_hit] | exact[any_hit]
        else:
            want["score"], want["exact"] = best[any_hit], exact[any_hit]
        assert got == len(want), (n, form, k, grid, got, len(want))
        assert out[:got].tolist() == want.tolist(), (n, form, k, grid)
        assert (out[got:].view(np.uint8) == 0xAB).all()  # nothing beyond the kept records
        assert (np.diff(out[:got]["index"].astype(np.int64)) > 0).all()  # index-ascending


def test_the_group_as_a_stand_alone_program_under_address_and_ub_sanitizers():
    """the same source with its own main, built with -fsanitize=address,undefined and run as a process of its own"""
    r = subprocess.run([A.build_sanitized()], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    assert r.stdout.strip().endswith("anyof_host ok") and "runtime error" not in r.stderr, (r.stdout[-500:], r.stderr[-2000:])
