"""The placement arithmetic of the sectioned top-`limit` with matched positions (frizbee_amd/csrc/sections.h: sections_slab_kept,
sections_head_base, sections_head_dest), compiled for the host and walked the way k_sec_items walks it: the S * limit slab slots of the
sectioned stage go to ONE dense head, head s behind the records of the heads in front of it.  Held against a numpy concatenation for every
S = 0..8 and limit in {0, 1, 2, 255, 256, 257, 1024}, the kept counts drawn from {0, 1, limit - 1, limit}, all-empty and all-full included;
the same source runs as a stand-alone program under AddressSanitizer + UBSan."""
import subprocess

import numpy as np
import pytest

import sections_items_host_lib as H

pytestmark = pytest.mark.skipif(not H.available(), reason="ROCm's clang++ is not installed")
LIMITS = (0, 1, 2, 255, 256, 257, 1024)
GUARD = 0xABABABAB


def walk(slabs, counts, S, limit, cap):
    head = np.full((cap + 2, 2), GUARD, np.uint32)
    items = np.full(cap + 2, GUARD, np.uint32)
    dev_counts = np.full(2 * S + 6, GUARD, np.uint32)
    words = np.zeros(3, np.uint32)
    dropped = H.lib().sih_items(slabs.ctypes.data, counts.ctypes.data, S, limit, cap, head.ctypes.data, items.ctypes.data, dev_counts.ctypes.data, words.ctypes.data)
    return head, items, dev_counts, words, dropped


def model(slabs, kept, S, limit):
    """the heads concatenated in section order"""
    parts = [slabs[s * limit:s * limit + kept[s]] for s in range(S)]
    return np.concatenate(parts) if parts else np.zeros((0, 2), np.uint32)


def draws(rng, S, limit):
    choice = [0, 1, max(limit - 1, 0), limit]
    yield [0] * S
    yield [limit] * S
    for _ in range(6):
        yield [min(int(rng.choice(choice)), limit) for _ in range(S)]


@pytest.mark.parametrize("limit", LIMITS)
def test_the_dense_head_is_the_concatenation_of_the_slabs_heads(limit):
    rng = np.random.default_rng(limit + 7)
    for S in range(0, 9):
        for kept in draws(rng, S, limit):
            slabs = rng.integers(0, 2**32, (S * limit + 1, 2), dtype=np.uint64).astype(np.uint32)
            counts = np.zeros(2 * S + 1, np.uint32)
            counts[0:2 * S:2] = kept
            counts[1:2 * S:2] = rng.integers(0, 2**32, S, dtype=np.uint64)
            want = model(slabs, kept, S, limit)
            cap = S * limit
            head, items, dev_counts, words, dropped = walk(slabs, counts, S, limit, cap)
            n = len(want)
            assert dropped == 0 and words.tolist() == [n, n, n], (S, limit, kept)
            assert np.array_equal(head[:n], want) and np.array_equal(items[:n], want[:, 0]), (S, limit, kept)
            assert (head[n:] == GUARD).all() and (items[n:] == GUARD).all(), "nothing behind the dense head is written"
            assert dev_counts[:2 * S].tolist() == counts[:2 * S].tolist()
            assert dev_counts[2 * S:].tolist() == [GUARD, GUARD, 0, 0, GUARD, GUARD], "[2S], [2S + 1] are the pack's, [2S + 2], [2S + 3] are cleared"
            # an exactly sized head: cap = the records in all
            head, items, _, words, dropped = walk(slabs, counts, S, limit, n)
            assert dropped == 0 and np.array_equal(head[:n], want) and (head[n:] == GUARD).all() and (items[n:] == GUARD).all()


def test_a_count_beyond_the_slab_is_clamped_and_a_short_head_drops_instead_of_writing():
    rng = np.random.default_rng(3)
    S, limit = 5, 9
    slabs = rng.integers(0, 2**32, (S * limit, 2), dtype=np.uint64).astype(np.uint32)
    counts = np.zeros(2 * S, np.uint32)
    counts[0::2] = [9, 100, 0, 4000000000, 3]
    want = model(slabs, [9, 9, 0, 9, 3], S, limit)
    head, items, dev_counts, words, dropped = walk(slabs, counts, S, limit, S * limit)
    assert dropped == 0 and words[0] == 30 and np.array_equal(head[:30], want) and dev_counts[0:2 * S:2].tolist() == [9, 9, 0, 9, 3]
    head, items, _, words, dropped = walk(slabs, counts, S, limit, 20)
    assert dropped == 10 and words.tolist() == [20, 20, 20] and np.array_equal(head[:20], want[:20]) and (head[20:] == GUARD).all() and (items[20:] == GUARD).all()


def test_the_kernel_calls_the_functions_this_walk_calls():
    src = open(H.SRC).read()
    for name in ("sections_head_base(", "sections_head_dest(", "sections_slab_kept("):
        assert name in src, name
    kern = open(H.CSRC + "/kernels_sections.hip").read()
    body = kern[kern.index("__global__ __launch_bounds__(256) void k_sec_items("):kern.index("void fzb_launch_sections_items(")]
    for name in ("sections_head_base(", "sections_head_dest(", "sections_slab_kept(", "gridDim.x * 256u"):  # the kernel calls what this file walks, grid-stride
        assert name in body, name
    assert "atomic" not in body  # no workgroup waits for another one, nothing is ordered by an atomic
    assert H.lib().sih_no_slot() == 0xFFFFFFFF


def test_the_walk_as_a_stand_alone_program_under_address_and_ub_sanitizers():
    """the same source with its own main, built with -fsanitize=address,undefined and run as a process of its own"""
    r = subprocess.run([H.build_sanitized()], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    assert r.stdout.strip().endswith(" 0 mismatches") and "runtime error" not in r.stderr, (r.stdout[-500:], r.stderr[-2000:])
