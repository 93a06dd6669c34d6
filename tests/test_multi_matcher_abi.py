"""CPU-side checks of the multi-pattern matcher's lifecycle entry points (fzb_multi_matcher_set_patterns / _set_config / _reserve / _clone,
the parallel forms, the shard report, fzb_debug_device_allocs): argument checks, the reference's panic text for `threads == 0`, and that
the Rust binding declares every fzb_multi_* symbol of the header with the same number of parameters.  Nothing here touches a device."""
import ctypes as C
import os
import re

import pytest

import frizbee_amd as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["fzb_multi_matcher_set_patterns", "fzb_multi_matcher_set_config", "fzb_multi_matcher_reserve", "fzb_multi_matcher_clone", "fzb_multi_match_list_parallel",
       "fzb_multi_match_list_parallel_sharded", "fzb_multi_match_list_parallel_rccl", "fzb_multi_matcher_shard_report", "fzb_debug_device_allocs"]


def _last_error():
    return F.lib().fzb_last_error().decode()


def test_new_entry_points_reject_null_arguments():
    l = F.lib()
    cfg = F._c_config(F.Config())
    dummy = C.c_void_p(C.addressof(cfg))  # a non-null handle that no check below may dereference
    out, n = C.c_void_p(), C.c_size_t()
    calls = [
        lambda: l.fzb_multi_matcher_set_patterns(None, None, 0),
        lambda: l.fzb_multi_matcher_set_patterns(dummy, None, 2),
        lambda: l.fzb_multi_matcher_set_config(None, C.byref(cfg)),
        lambda: l.fzb_multi_matcher_set_config(dummy, None),
        lambda: l.fzb_multi_matcher_reserve(None, dummy),
        lambda: l.fzb_multi_matcher_reserve(dummy, None),
        lambda: l.fzb_multi_matcher_clone(None, C.byref(out)),
        lambda: l.fzb_multi_matcher_clone(dummy, None),
        lambda: l.fzb_multi_match_list_parallel(None, dummy, 1, C.byref(out), C.byref(n)),
        lambda: l.fzb_multi_match_list_parallel(dummy, None, 1, C.byref(out), C.byref(n)),
        lambda: l.fzb_multi_match_list_parallel_sharded(None, dummy, C.byref(out), C.byref(n)),
        lambda: l.fzb_multi_match_list_parallel_sharded(dummy, None, C.byref(out), C.byref(n)),
        lambda: l.fzb_multi_match_list_parallel_sharded(dummy, dummy, None, C.byref(n)),
        lambda: l.fzb_multi_match_list_parallel_rccl(None, dummy, 0, dummy, 0, C.byref(out), C.byref(n)),
        lambda: l.fzb_multi_match_list_parallel_rccl(dummy, None, 0, dummy, 0, C.byref(out), C.byref(n)),
        lambda: l.fzb_multi_match_list_parallel_rccl(dummy, dummy, 0, None, 0, C.byref(out), C.byref(n)),
        lambda: l.fzb_multi_match_list_parallel_rccl(dummy, dummy, 0, dummy, 0, None, C.byref(n)),
        lambda: l.fzb_debug_device_allocs(None),
    ]
    for i, call in enumerate(calls):
        assert call() == 1, (i, _last_error())  # FZB_ERR_INVALID
        assert "null" in _last_error(), (i, _last_error())
    assert l.fzb_multi_matcher_shard_report(None) == b""


def test_set_patterns_rejects_a_null_needle_and_keeps_the_matcher():
    m = F.MultiMatcher([F.Pattern("dead"), F.Pattern("x", negated=True)])
    arr = (F._CPattern * 1)()
    arr[0].needle_utf8, arr[0].needle_len, arr[0].casing, arr[0].unicode, arr[0].matching = None, 3, -1, -1, -1
    assert F.lib().fzb_multi_matcher_set_patterns(m.h, arr, 1) == 1 and "null" in _last_error()
    assert len(m) == 2
    arr2 = (F._CPattern * 2)()  # as many patterns as the matcher holds, the same lengths: checked before any comparison
    for i, k in enumerate((4, 1)):
        arr2[i].needle_utf8, arr2[i].needle_len, arr2[i].casing, arr2[i].unicode, arr2[i].matching = None, k, -1, -1, -1
    assert F.lib().fzb_multi_matcher_set_patterns(m.h, arr2, 2) == 1 and "null" in _last_error()
    assert len(m) == 2


def test_host_side_lifecycle_without_a_device():
    """set_patterns / set_config / clone only build host-side tables: the compiled-pattern count follows the reference's compile step
    (empty needles dropped, src/matcher/mod.rs:193-195), and an invalid needle leaves the matcher as it was."""
    m = F.MultiMatcher(F.parse_query("src linux !test"), F.Config(pf_lanes=64))
    assert len(m) == 3
    m.set_patterns(F.parse_query("src"))
    assert len(m) == 1
    m.set_patterns([F.Pattern(""), F.Pattern("a"), F.Pattern("b", negated=True), F.Pattern("")])
    assert len(m) == 2
    m.set_patterns([])
    assert len(m) == 0
    m.set_patterns(F.parse_query("a b c d"))
    assert len(m) == 4
    with pytest.raises(F.FrizbeeError, match="UTF-8"):
        m.set_patterns([F.Pattern("ok"), F.Pattern(b"\xff\xfe")])
    assert len(m) == 4 and [p.needle for p in m.patterns] == ["a", "b", "c", "d"]
    m.set_config(F.Config(pf_lanes=64, sort=F.SortStrategy.IndexDesc))
    assert m.config.sort == F.SortStrategy.IndexDesc and len(m) == 4
    c = m.clone()
    c.set_patterns(F.parse_query("x"))
    assert len(c) == 1 and len(m) == 4
    before = F.device_allocs()
    m.set_patterns(F.parse_query("a b c d"))  # identical patterns: nothing to do
    assert F.device_allocs() == before


def test_parallel_with_zero_threads_is_the_reference_panic():
    m = F.MultiMatcher(F.parse_query("dead !x"))
    cfg = F._c_config(F.Config())
    dummy = C.c_void_p(C.addressof(cfg))  # the thread count is checked before the corpus is read
    out, n = C.c_void_p(), C.c_size_t()
    assert F.lib().fzb_multi_match_list_parallel(m.h, dummy, 0, C.byref(out), C.byref(n)) == 2  # FZB_ERR_PANIC
    assert _last_error() == "threads must be positive"


def _c_params(decl):
    inner = decl[decl.index("(") + 1: decl.rindex(")")].strip()
    return 0 if inner in ("", "void") else inner.count(",") + 1


def test_rust_binding_declares_every_multi_symbol_with_its_arity():
    hdr = open(os.path.join(ROOT, "include", "frizbee_hip.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    c_decls = {m.group(1): _c_params(m.group(0)) for m in re.finditer(r"\b(fzb_multi_[a-z0-9_]+|fzb_debug_device_allocs)\s*\([^;{]*\)\s*;", hdr)}
    assert set(NEW) <= set(c_decls) | {"fzb_debug_device_allocs"}, sorted(c_decls)
    rs = open(os.path.join(ROOT, "rust", "src", "hip.rs")).read()
    block = rs[rs.index('extern "C" {'):]
    block = block[: block.index("\n}\n")]
    rust = {}
    for m in re.finditer(r"fn\s+(fzb_[a-z0-9_]+)\s*\(([^)]*)\)", block):
        args = m.group(2).strip().rstrip(",")
        rust[m.group(1)] = 0 if not args else args.count(",") + 1
    for name, arity in c_decls.items():
        if not name.startswith("fzb_multi_"):
            continue
        assert name in rust, f"{name} is declared in the header but not bound in rust/src/hip.rs"
        assert rust[name] == arity, (name, arity, rust[name])
