"""frizbee_amd/csrc/facets.h on the host (tests/kernel_host/facets_host.cpp): the record form's and the column form's walk - the per-record
rule and the accumulation the kernels share - against the counts by their definition in numpy (tests/facets_model.py), over record counts
around the wave and tile edges, tags over all 16 bits, non-zero `first` and `index_offset`, haystacks beyond the tag column, and a grid of
scopes; and the same source as a stand-alone program under the sanitizers."""
import subprocess

import numpy as np
import pytest

import facets_host_lib as H
from facets_model import WORDS, facet_words

pytestmark = pytest.mark.skipif(not H.available(), reason="ROCm clang++ not installed")

COUNTS = (0, 1, 63, 64, 65, 1023, 1024, 1025, 21 * 1024 + 37)
SCOPES = [(0, 0), (1, 0), (0, 1), (2, 1), (1, 2), (3, 0), (0, 3), (0x8000, 0), (0, 0x8000), (0x8000, 1), (3, 3), (0xFFFF, 0), (0, 0xFFFF)]


def draw_tags(rng, n):
    """16-bit tags: bit 15 forced on a quarter, all ones on an eighth, zero on some"""
    t = rng.integers(0, 65536, n).astype(np.uint32)
    t[rng.random(n) < 0.25] |= 0x8000
    t[rng.random(n) < 0.125] = 0xFFFF
    t[rng.random(n) < 0.05] = 0
    return t.astype(np.uint16)


def records(rng, n, span, index_offset):
    at = np.sort(rng.choice(span, n, replace=False)) if n else np.zeros(0, np.int64)
    recs = np.zeros((n, 2), np.uint32)
    recs[:, 0] = ((at + index_offset) & 0xFFFFFFFF).astype(np.uint32)
    recs[:, 1] = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
    return recs, at


def tags_of(tags, haystacks):
    """the column's invariant: a haystack at or beyond its entries has tag 0"""
    h = np.asarray(haystacks, np.int64)
    out = np.zeros(len(h), np.uint16)
    inside = h < len(tags)
    out[inside] = tags[h[inside]]
    return out


def run_records(recs, tags, first, index_offset, require, exclude):
    out = np.full(WORDS + 4, 0xABABABAB, np.uint32)
    words = np.ascontiguousarray(recs, np.uint32)
    H.lib().fh_records(words.ctypes.data if len(recs) else None, len(recs), tags.ctypes.data if tags is not None else None, 0 if tags is None else len(tags), first, index_offset,
                       require, exclude, out.ctypes.data)
    assert (out[WORDS:] == 0xABABABAB).all()
    return out[:WORDS]


def run_column(items, n, tags, first, require, exclude):
    out = np.full(WORDS + 4, 0xABABABAB, np.uint32)
    it = None if items is None else np.ascontiguousarray(items, np.uint32)
    H.lib().fh_column(None if it is None or not len(it) else it.ctypes.data, n, tags.ctypes.data if tags is not None else None, 0 if tags is None else len(tags), first, require, exclude,
                      out.ctypes.data)
    assert (out[WORDS:] == 0xABABABAB).all()
    return out[:WORDS]


def test_layout():
    assert H.lib().fh_words() == WORDS == 34


@pytest.mark.parametrize("n", COUNTS)
def test_record_form_against_numpy(n):
    rng = np.random.default_rng(700 + n)
    for first, index_offset, beyond in ((0, 0, 0), (37, 7, 0), (1500, 4_000_000_000, 0), (37, 9, 11)):
        span = n + n // 3 + 5
        n_tags = first + span - beyond  # beyond: the last haystacks lie at and behind the column's end
        tags = draw_tags(rng, n_tags)
        recs, at = records(rng, n, span, index_offset)
        a_tags = tags_of(tags, first + at)
        if beyond and n:
            recs[-1, 0] = (index_offset + span - 1) & 0xFFFFFFFF  # one record on the last haystack: beyond n_tags, tag 0
            a_tags = tags_of(tags, np.concatenate([first + at[:-1], [first + span - 1]]))
        for require, exclude in SCOPES:
            got = run_records(recs, tags, first, index_offset, require, exclude)
            assert got.tolist() == facet_words(a_tags, require, exclude).tolist(), (n, first, index_offset, require, exclude)
        assert run_records(recs, None, first, index_offset, 0, 0).tolist() == facet_words(np.zeros(n, np.uint16)).tolist()  # a corpus without tags


@pytest.mark.parametrize("n", COUNTS)
def test_column_form_against_numpy(n):
    rng = np.random.default_rng(900 + n)
    for first in (0, 37):
        span = n + n // 2 + 3
        tags = draw_tags(rng, first + span - 2)  # the last two haystacks have no entry: tag 0
        items = np.sort(rng.choice(span, n, replace=False)).astype(np.uint32) if n else np.zeros(0, np.uint32)
        for require, exclude in SCOPES:
            assert run_column(None, n, tags, first, require, exclude).tolist() == facet_words(tags_of(tags, first + np.arange(n)), require, exclude).tolist()
            assert run_column(items, n, tags, first, require, exclude).tolist() == facet_words(tags_of(tags, first + items.astype(np.int64)), require, exclude).tolist()
        assert run_column(items, n, None, first, 0, 0).tolist() == facet_words(np.zeros(n, np.uint16)).tolist()


def test_sums_hold_together():
    """visible <= matched, a row's entry never exceeds its total, and the (0, 0) scope makes both rows equal"""
    rng = np.random.default_rng(5)
    n = 5000
    tags = draw_tags(rng, n)
    recs, at = records(rng, n, n, 0)
    w = run_records(recs, tags, 0, 0, 0, 0)
    assert w[0] == w[1] == n and w[2:18].tolist() == w[18:34].tolist()
    w = run_records(recs, tags, 0, 0, 2, 1)
    assert w[1] < w[0] and (w[18:34] <= w[2:18]).all() and w[18 + 1] == w[1] and w[18 + 0] == 0  # every visible record has bit 1 and lacks bit 0


def test_the_walk_as_a_stand_alone_program_under_address_and_ub_sanitizers():
    """the same source with its own main, built with -fsanitize=address,undefined and run as a process of its own"""
    r = subprocess.run([H.build_sanitized()], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    assert r.stdout.strip().endswith(" 0 mismatches") and "runtime error" not in r.stderr, (r.stdout[-500:], r.stderr[-2000:])
