"""Edge cases of the boundary on the GPU: 64-bit end offsets, NUL bytes in haystacks and needles, a result buffer smaller
than the match list, one-item lists, every (fuzzy) kernel family on a device-built padded-16 corpus."""
import os
import sys

import numpy as np
import pytest
import torch

import frizbee_amd as F
import oracle_lib as O

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import synth  # noqa: E402

pytestmark = pytest.mark.gpu


def padded16(haystacks, dev, u64):
    """Build the device layout by hand: every haystack on a 16-byte boundary, exclusive ends, >= 96 zero bytes of tail."""
    ends, pos, chunks = [], 0, []
    for h in haystacks:
        pad = (-pos) % 16
        chunks.append(b"\0" * pad + h)
        pos += pad + len(h)
        ends.append(pos)
    blob = b"".join(chunks) + b"\0" * ((-pos) % 16 + 96)
    data = torch.frombuffer(bytearray(blob), dtype=torch.uint8).to(dev)
    e = torch.tensor(ends, dtype=torch.int64 if u64 else torch.int32, device=dev) if ends else torch.zeros(1, dtype=torch.int64 if u64 else torch.int32, device=dev)
    return F.Corpus.from_device(data.data_ptr(), e.data_ptr(), len(haystacks), data.numel(), ends_are_u64=u64, keep=(data, e))


@pytest.mark.parametrize("u64", [False, True])
def test_device_layout_with_32_and_64_bit_ends(u64):
    rng = np.random.default_rng(5)
    alpha = b"abcdeDEF_-/ 01\0"
    hs = [bytes(alpha[int(x)] for x in rng.integers(0, len(alpha), int(rng.choice([0, 1, 5, 16, 31, 32, 33, 64, 65, 100, 200, 1100])))) for _ in range(3000)]
    cp = padded16(hs, torch.device("cuda", 0), u64)
    for needle, cfg in (("deadbe", dict(max_typos=0)), ("dea", dict(max_typos=1)), ("ab_c", dict(max_typos=None)), ("a\0b", dict(max_typos=0)), ("é", dict(max_typos=0, unicode="Always"))):
        for matching in ("Fuzzy", "Substring"):
            want = O.Matcher(needle, matching=matching, **cfg).match_list(hs)
            fc = F.Config(max_typos=cfg["max_typos"], unicode=F.UnicodeMatching[cfg.get("unicode", "Smart")], matching=F.Matching[matching], pf_lanes=64)
            got = F.Matcher(needle, fc).match_list(cp)
            assert got.tolist() == want.tolist(), (needle, cfg, matching, u64)


def test_result_buffer_smaller_than_the_match_list_is_clamped_not_overrun():
    rows, ends = synth.fixed_corpus(b"deadbe", 200_000, 32)
    cp = F.Corpus(packed=(rows.numpy().reshape(-1), ends))
    m = F.Matcher("deadbe", F.Config(sort=F.SortStrategy.IndexAsc, pf_lanes=64, sw_lanes=64))
    whole = m.match_list(cp)
    cap = len(whole) // 3
    dev = torch.device("cuda", 0)
    out = torch.full(((cap + 64) * 8,), 0xAB, dtype=torch.uint8, device=dev)
    cnt = torch.zeros(4, dtype=torch.int32, device=dev)
    m.match_list_device(cp, out.data_ptr(), cap, cnt.data_ptr())
    torch.cuda.synchronize()
    assert int(cnt[0].item()) == cap
    host = out.cpu().numpy()
    assert host[: cap * 8].view(F.MATCH_DTYPE).tolist() == whole[:cap].tolist()  # index order: the first `cap` matches
    assert (host[cap * 8 :] == 0xAB).all()  # nothing written past the capacity


def test_tiny_lists():
    for hs in ([], [""], ["deadbe"], ["x"], ["", "deadbe", ""]):
        for typos in (0, 1, None):
            want = O.Matcher("deadbe", max_typos=typos).match_list(hs)
            got = F.Matcher("deadbe", F.Config(max_typos=typos, pf_lanes=64)).match_list(hs)
            assert got.tolist() == want.tolist(), (hs, typos)
        assert F.MultiMatcher(F.parse_query("dead !x"), F.Config(pf_lanes=64)).match_list(hs).tolist() == O.MultiMatcher(O.parse_query("dead !x")).match_list(hs).tolist()


def test_set_pattern_and_set_config_requery_a_resident_corpus():
    # Matcher::set_pattern / set_config (src/matcher/mod.rs:143-176): typing "deadbeef" one key at a time against one resident list
    rows, ends = synth.fixed_corpus(b"deadbeef", 200_000, 32)
    data = rows.numpy().reshape(-1)
    cp = F.Corpus(packed=(data, ends))
    odata = np.concatenate([data, np.zeros(64, np.uint8)])
    m = F.Matcher("d", F.Config(pf_lanes=64))
    for needle in ("d", "de", "dea", "dead", "deadb", "deadbe", "deadbee", "deadbeef", "Dead", "é", ""):
        m.set_pattern(needle)
        assert m.match_list(cp).tolist() == O.Matcher(needle).match_packed(odata, ends).tolist(), needle
    m.set_pattern("deadbe")
    for cfg, ocfg in ((F.Config(max_typos=2, pf_lanes=64), dict(max_typos=2)), (F.Config(max_typos=None, sort=F.SortStrategy.IndexDesc, pf_lanes=64), dict(max_typos=None, sort="IndexDesc")),
                      (F.Config(matching=F.Matching.Substring, pf_lanes=64), dict(matching="Substring")), (F.Config(pf_lanes=16), dict())):
        m.set_config(cfg)
        lanes = (16, 16, 8) if cfg.pf_lanes == 16 else (64, 64, 32)
        assert m.match_list(cp).tolist() == O.Matcher("deadbe", lanes=lanes, **ocfg).match_packed(odata, ends).tolist(), ocfg
    with pytest.raises(F.PanicError):
        m.set_pattern("a" * 3640)  # refused (the reference's overflow guard, src/lib.rs:506-527): the matcher keeps working as it was
    assert m.match_list(cp).tolist() == O.Matcher("deadbe", lanes=(16, 16, 8)).match_packed(odata, ends).tolist()


def test_every_synchronous_entry_point_interleaved_across_needle_changes():
    """match_list, match_list_top, match_list_indices and match_list_top_indices take turns on ONE matcher and one resident corpus while
    set_pattern / set_config walk it through every kind of needle (short, beyond 64 bytes, beyond 128, typos, unicode, empty, literal, the
    first again): what has to survive a needle change is the union of what the four keep on the device - workspace, staging, trace and top
    buffers, pinned count words and their guesses, the long needle's arrays.  Every result equals a freshly created matcher's; the
    oracle's records at the short, the 130-byte and the unicode step."""
    data, ends = synth.paths_corpus(b"linux", 2000, seed=21)
    starts = np.concatenate([[0], ends[:-1]]).astype(np.int64)
    hs = [data[int(a):int(b)].tobytes() for a, b in zip(starts, ends.astype(np.int64))]
    long_path = b"out/Release/gen/chrome/browser/resources/settings/privacy_page/security_keys_subpage/security_keys_bio_enroll_dialog.html.rollup.js.map"
    n70, n130 = long_path[:70], long_path[-130:]  # beyond the 64 bytes of the by-value needle, and beyond 128
    hs += [b"//" + n70 + b"~", b"a/" + n130 + b"/z", b"x/" * 520 + b"linux_" + n70, "éa_ü/linux".encode(), "zz/éXaü.txt".encode(), "日本語/é/a/ü".encode()]
    assert max(len(h) for h in hs) > 1024
    cp = F.Corpus(hs)
    base = dict(max_typos=0, pf_lanes=64)
    walk = (("linux", base, True), (n70, base, False), (n130, base, True), ("linx", dict(base, max_typos=1), False), ("éaü", dict(base, max_typos=1), True), ("", dict(base, max_typos=1), False),
            ("lin", dict(base, matching=F.Matching.Substring), False), ("linux", base, False))

    def four(mt):
        top, found = mt.match_list_top(cp, 5)
        topi, foundi = mt.match_list_top_indices(cp, 5)
        return mt.match_list(cp).tolist(), (top.tolist(), found), mt.match_list_indices(cp), (topi, foundi)

    m = F.Matcher(walk[0][0], F.Config(**base))
    cur = base
    for step, (needle, cfg, with_oracle) in enumerate(walk):
        if cfg != cur:
            m.set_config(F.Config(**cfg))
            cur = cfg
        m.set_pattern(needle)
        got, want = four(m), four(F.Matcher(needle, F.Config(**cfg)))
        for name, g, w in zip(("match_list", "match_list_top", "match_list_indices", "match_list_top_indices"), got, want):
            assert g == w, (step, needle, name)
        assert got[1][1] == len(got[0]) == got[3][1] and got[1][0] == got[0][:5], (step, needle)
        if with_oracle:
            rec = O.Matcher(needle, lanes=(64, 64, 32), max_typos=cfg["max_typos"]).match_list(hs)
            assert got[0] == rec.tolist() and len(rec) > 0, (step, needle)


def test_corpus_beyond_4_gib_uses_64_bit_offsets():
    # 41 M haystacks of 112 bytes = 4.59 GB: end offsets and byte addresses no longer fit 32 bits.  Built on the device
    # (padded-16 layout = back-to-back rows since 112 % 16 == 0); checked against the oracle on three windows of the list,
    # one of them entirely above the 4 GiB line, through sub-range calls and through the whole-list call.
    dev = torch.device("cuda", 0)
    n, L = 41_000_000, 112
    needle = b"deadbeef"
    g = torch.Generator(device=dev)
    g.manual_seed(7)
    flat = torch.empty(n * L + 256, dtype=torch.uint8, device=dev)
    alpha = torch.tensor(list(b"abcdefghijklmnopqrstuvwxyz_-/0123456789"), dtype=torch.uint8, device=dev)
    step = 1_000_000
    for lo in range(0, n, step):
        hi = min(lo + step, n)
        idx = torch.randint(0, len(alpha), ((hi - lo) * L,), generator=g, device=dev)
        flat[lo * L : hi * L] = alpha[idx]
    flat[n * L :] = 0
    ends = torch.arange(1, n + 1, dtype=torch.int64, device=dev) * L
    assert int(ends[-1].item()) > (1 << 32)
    cp = F.Corpus.from_device(flat.data_ptr(), ends.data_ptr(), n, flat.numel(), ends_are_u64=True, keep=(flat, ends))
    m = F.Matcher(needle.decode(), F.Config(max_typos=1, sort=F.SortStrategy.IndexAsc, pf_lanes=64, sw_lanes=64))
    om = O.Matcher(needle.decode(), max_typos=1, sort="IndexAsc")
    whole = m.match_list(cp)
    assert len(whole) > 1000
    for first in (0, 38_347_000, n - 200_000):  # 38_347_922 * 112 = 2^32: the second window straddles the line
        cnt = 200_000
        host = flat[first * L : (first + cnt) * L].cpu().numpy()
        want = om.match_packed(np.concatenate([host, np.zeros(64, np.uint8)]), np.arange(1, cnt + 1, dtype=np.uint64) * np.uint64(L))
        got = m.match_list_into(cp, first=first, count=cnt, index_offset=0)
        assert got.tolist() == want.tolist(), first
        sl = whole[(whole["index"] >= first) & (whole["index"] < first + cnt)].copy()
        sl["index"] -= first
        assert sl.tolist() == want.tolist(), first


@pytest.mark.gpu
def test_reserve_then_requery_does_not_change_results():
    """fzb_matcher_reserve sizes the workspace, scorer scratch, staging and sort buffers for a corpus; queries after it (and after
    set_pattern, which keeps them) give what a fresh matcher gives."""
    import random
    rng = random.Random(8)
    hs = ["".join(rng.choice("abcdeDEAB_-/ 01") for _ in range(rng.randint(0, 90))) for _ in range(5000)] + ["dead_beef" * 20, "deadbe"]
    corpus = F.Corpus(hs)
    m = F.Matcher("deadbe", F.Config(max_typos=1, pf_lanes=64, sw_lanes=64))
    m.reserve(corpus)
    for needle in ("deadbe", "abc", "dead_beefdead", "e"):
        m.set_pattern(needle)
        got = m.match_list(corpus)
        want = F.Matcher(needle, F.Config(max_typos=1, pf_lanes=64, sw_lanes=64)).match_list(corpus)
        assert got.tolist() == want.tolist(), needle


@pytest.mark.parametrize("pf", [64, 32, 16])
@pytest.mark.parametrize("typos", [0, 1, None])
def test_every_window_width_around_the_class_boundaries(pf, typos):
    """Classified scoring (k2w_classify + k2b_dp_class) and the short scorer: windows of EVERY width from 1 byte to well past a chunk, so
    that each class boundary (1/2, 3/4, 1 chunk, multi-chunk) is crossed at the three lane widths; the needle's bytes sit at both ends of
    the window and the filler holds partial matches.  A list with long haystacks (classes) and a short-only list (k2b_dp_short)."""
    import random
    rng = random.Random(1000 * pf + (typos or 7))
    lanes = {64: (64, 64, 32), 32: (32, 32, 16), 16: (16, 16, 8)}[pf]
    needle = "ab_c"
    hs = []
    for width in range(1, 150):
        for rep in range(3):
            inner = "".join(rng.choice("xyab_cAB ") for _ in range(max(0, width - 2)))
            core = ("a" + inner + "c")[:width] if width >= 2 else "a"
            lead = "".join(rng.choice("xyz") for _ in range(rng.choice([0, 0, 1, 5])))
            tail = "".join(rng.choice("xyz") for _ in range(rng.choice([0, 0, 3])))
            hs.append(lead + core + tail)
    rng.shuffle(hs)
    for sub in (hs, [h for h in hs if len(h) <= lanes[1] // 2]):
        want = O.Matcher(needle, lanes=lanes, max_typos=typos, sort="IndexAsc").match_list(sub)
        got = F.Matcher(needle, F.Config(max_typos=typos, sort=F.SortStrategy.IndexAsc, pf_lanes=pf)).match_list(sub)
        assert got.tolist() == want.tolist(), (pf, typos, len(sub))
        assert len(want) >= len(sub) // 8 or sub is not hs  # (the short-only list may hold few matches)


@pytest.mark.parametrize("length", [32, 20, 16, 7])
def test_uniform_length_corpus_needs_no_end_offsets(length):
    """A list whose haystacks all have the same length is detected by fzb_corpus_upload (or declared for borrowed memory): the hot kernels
    then compute start(i) = i * roundup16(len) instead of reading the end offsets.  Same records as the oracle, and as the same list made
    non-uniform by one extra haystack."""
    import random
    rng = random.Random(length)
    hs = ["".join(rng.choice("deadbeDEAB_x01") for _ in range(length)) for _ in range(4000)]
    for needle, kw in (("deadbe", dict(max_typos=0)), ("deadbe", dict(max_typos=2)), ("dea", dict(max_typos=None)), ("éa", dict(max_typos=0))):
        want = O.Matcher(needle, lanes=(64, 64, 32), sort="IndexAsc", **kw).match_list(hs)
        cfg = F.Config(sort=F.SortStrategy.IndexAsc, pf_lanes=64, sw_lanes=64, **kw)
        got_u = F.Matcher(needle, cfg).match_list(F.Corpus(hs))                 # uniform: detected at upload
        got_n = F.Matcher(needle, cfg).match_list(F.Corpus(hs + ["x" * (length + 3)]))  # not uniform
        assert got_u.tolist() == want.tolist(), (needle, kw, length)
        assert got_n[got_n["index"] < len(hs)].tolist() == want.tolist(), (needle, kw, length)
    # borrowed device memory with the promise
    cp = padded16([h.encode() for h in hs], torch.device("cuda", 0), False)
    F._check(F.lib().fzb_corpus_set_uniform_len(cp.h, length))
    want = O.Matcher("deadbe", lanes=(64, 64, 32), sort="IndexAsc", max_typos=1).match_list(hs)
    assert F.Matcher("deadbe", F.Config(sort=F.SortStrategy.IndexAsc, pf_lanes=64, sw_lanes=64, max_typos=1)).match_list(cp).tolist() == want.tolist()


@pytest.mark.parametrize("u64", [False, True])
def test_wrong_promises_about_borrowed_memory_are_refused(u64):
    """fzb_corpus_set_uniform_len / fzb_corpus_set_max_len on borrowed device memory select kernels that compute spans instead of reading
    the end offsets: a wrong promise would silently mis-span every haystack, so one device pass over the offsets checks it when it is made
    (round 4 verdict, weak item 8).  FZB_VERIFY_PROMISES=0 restores the unchecked behaviour."""
    import os
    dev = torch.device("cuda", 0)
    hs = [b"deadbeef_0123456"] * 3000 + [b"deadbeef_0123456xy"] + [b"deadbeef_0123456"] * 500  # one haystack of 18 bytes among 16-byte ones
    cp = padded16(hs, dev, u64)
    assert F.lib().fzb_corpus_set_uniform_len(cp.h, 16) == 1
    assert "first at index 3000" in F.lib().fzb_last_error().decode(), F.lib().fzb_last_error()
    assert F.lib().fzb_corpus_set_max_len(cp.h, 17) == 1 and "index 3000" in F.lib().fzb_last_error().decode()
    assert F.lib().fzb_corpus_set_max_len(cp.h, 18) == 0  # a true bound
    want = O.Matcher("deadbe", lanes=(64, 64, 32)).match_list([h.decode() for h in hs])
    assert F.Matcher("deadbe", F.Config(pf_lanes=64, sw_lanes=64)).match_list(cp).tolist() == want.tolist()
    ok = padded16([b"deadbeef_0123456"] * 1000, dev, u64)
    assert F.lib().fzb_corpus_set_uniform_len(ok.h, 16) == 0  # a true promise
    assert F.lib().fzb_corpus_set_uniform_len(ok.h, 0) == 0 and F.lib().fzb_corpus_set_uniform_len(ok.h, 15) == 1
    # decreasing offsets are a violation whatever is promised
    data = torch.zeros(4096, dtype=torch.uint8, device=dev)
    e = torch.tensor([16, 32, 20, 64], dtype=torch.int64 if u64 else torch.int32, device=dev)
    bad = F.Corpus.from_device(data.data_ptr(), e.data_ptr(), 4, data.numel(), ends_are_u64=u64, keep=(data, e))
    assert F.lib().fzb_corpus_set_max_len(bad.h, 64) == 1 and "index 2" in F.lib().fzb_last_error().decode()
    os.environ["FZB_VERIFY_PROMISES"] = "0"
    F.lib().fzb_debug_reload_knobs()
    try:
        assert F.lib().fzb_corpus_set_max_len(bad.h, 64) == 0  # unchecked, as before
    finally:
        os.environ.pop("FZB_VERIFY_PROMISES", None)
        F.lib().fzb_debug_reload_knobs()


@pytest.mark.parametrize("pf", [64, 16])
def test_window_kernel_mask_buffer_overflow_and_long_walks(pf):
    """The lane-exact window kernel's PRE form lays a quarter tile's (haystack, chunk) occurrence masks out in 40 KB of LDS; haystacks whose
    pairs do not fit compute their masks on demand inside the walk.  Long haystacks (600..1000 bytes = 10..16 chunks of 64, 38..63 of 16) with
    a 7-row and a 2-scalar needle make most of every part overflow; short ones in between keep the laid-out path busy in the same workgroup.
    ASCII and unicode, 1 / 2 / 3 typos, against the oracle."""
    rng = np.random.default_rng(900 + pf)
    alpha = b"deadbfxyz_-/ 01DEAB"
    hs = []
    for i in range(5000):
        L = int(rng.integers(600, 1001)) if i % 3 else int(rng.integers(0, 90))
        body = bytearray(alpha[int(x)] for x in rng.integers(0, len(alpha), L))
        if rng.random() < 0.5 and L >= 7:
            for q, ch in zip(sorted(rng.choice(L, size=7, replace=False).tolist()), b"deadbef"):
                body[q] = ch
        hs.append(bytes(body))
    cp = F.Corpus(hs)
    lanes = {64: (64, 64, 32), 16: (16, 16, 8)}[pf]
    for needle, typos in (("deadbef", 1), ("deadbef", 2), ("deadbef", 3), ("da", 1)):
        want = O.Matcher(needle, lanes=lanes, max_typos=typos).match_list(hs)
        got = F.Matcher(needle, F.Config(max_typos=typos, pf_lanes=pf)).match_list(cp)
        assert got.tolist() == want.tolist() and len(want) > 100, (needle, typos, pf, len(got), len(want))
    uni = ["".join("éaxüñ_ "[int(x)] for x in rng.integers(0, 7, int(rng.integers(300, 700)) if i % 2 else int(rng.integers(0, 40)))) for i in range(3000)]
    for needle, typos in (("éa", 1), ("éañ", 2)):
        want = O.Matcher(needle, lanes=lanes, max_typos=typos).match_list(uni)
        got = F.Matcher(needle, F.Config(max_typos=typos, pf_lanes=pf)).match_list(uni)
        assert got.tolist() == want.tolist() and len(want) > 100, (needle, typos, pf)


@pytest.mark.gpu
@pytest.mark.parametrize("needle,cfg", [("deadbe", dict()), ("deadbe", dict(max_typos=1)), ("éa", dict(max_typos=None)), ("éa", dict())])
def test_a_workspace_sized_by_a_small_range_is_not_reused_for_a_range_within_4096_of_its_capacity(needle, cfg):
    """The queue of windows wider than a chunk is anchored at `count + 4096` entries (the back: windows beyond 1024 bytes and the unicode
    scorer's handed-on stragglers).  A workspace allocated for 1000 items holds 1000 + 125 + 4096 = 5221 entries: a later range of 5000 items
    on the same matcher must grow it, not write its back entries at index 9095 of a 5221-entry array (the round-5 advisor's finding)."""
    import random
    rng = random.Random(11)
    alpha = "deabé_-/ xyzDEA"
    def hay(L):
        s = [rng.choice(alpha) for _ in range(L)]
        for q, c in zip(sorted(rng.sample(range(L), len(needle))), needle):
            s[q] = c
        return "".join(s)
    hs = [hay(rng.randint(8, 60)) for _ in range(5000)]
    for k in rng.sample(range(1000, 5000), 40):
        hs[k] = hay(rng.choice([1100, 1500, 300, 700]))  # windows beyond 1024 bytes (greedy: the queue's back) and beyond four chunks (handed on)
    cp = F.Corpus(hs)
    m = F.Matcher(needle, F.Config(pf_lanes=64, sw_lanes=64, max_typos=cfg.get("max_typos", 0)))
    om = O.Matcher(needle, lanes=(64, 64, 32), **cfg)
    head = O.Matcher(needle, lanes=(64, 64, 32), sort="IndexAsc", **cfg).match_list(hs[:1000])  # (index order = what match_list_into returns)
    assert m.match_list_into(cp, first=0, count=1000).tolist() == head.tolist()
    got = m.match_list(cp)   # 5000 items on the workspace the first call allocated for 1000
    assert got.tolist() == om.match_list(hs).tolist()
    fresh = F.Matcher(needle, F.Config(pf_lanes=64, sw_lanes=64, max_typos=cfg.get("max_typos", 0))).match_list(cp)
    assert got.tolist() == fresh.tolist()


@pytest.mark.gpu
def test_a_looser_bound_beside_a_uniform_length_is_accepted_and_a_tighter_one_refused():
    dev = torch.device("cuda", 0)
    n = 5000
    rows = synth.make_rows(b"deadbe", n, 32, seed=3, device=dev)
    flat = torch.zeros(n * 32 + 256, dtype=torch.uint8, device=dev)
    flat[: n * 32].view(n, 32).copy_(rows)
    ends = (torch.arange(1, n + 1, dtype=torch.int64, device=dev) * 32).to(torch.int32)
    cp = F.Corpus.from_device(flat.data_ptr(), ends.data_ptr(), n, flat.numel(), keep=(flat, ends), max_len=64, uniform_len=32)  # 64 >= 32: implied, ignored
    host = np.concatenate([flat[: n * 32].cpu().numpy(), np.zeros(64, np.uint8)])
    want = O.Matcher("deadbe").match_packed(host, np.arange(1, n + 1, dtype=np.uint64) * np.uint64(32))
    assert F.Matcher("deadbe", F.Config(pf_lanes=64)).match_list(cp).tolist() == want.tolist()
    with pytest.raises(F.FrizbeeError) as e:
        F.Corpus.from_device(flat.data_ptr(), ends.data_ptr(), n, flat.numel(), keep=(flat, ends), max_len=16, uniform_len=32)
    assert "not an upper bound" in str(e.value)
