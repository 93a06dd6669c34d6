"""frizbee_amd - MI355X (gfx950) backend for saghen/frizbee's batched fuzzy-scoring path.

A thin ctypes mirror of the reference's public surface for this path (`Matcher::new`, `match_list`,
`match_list_parallel`, `Config`, `Scoring`, `Match`, `radix_sort_matches`; reference src/lib.rs:110-138,
src/matcher/mod.rs:86-222, src/matcher/parallel.rs:18-89) over the C ABI in include/frizbee_hip.h.
All scoring runs in hand-written HIP kernels (frizbee_amd/csrc); there is no CPU fallback: importing
works anywhere, but every scoring call raises unless libfrizbee_hip.so is built and a GPU is present.
"""
import ctypes as C
import weakref
import enum
import os
from copy import deepcopy
from dataclasses import dataclass, field, replace

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB_PATH = os.environ.get("FRIZBEE_HIP_LIB", os.path.join(_HERE, "libfrizbee_hip.so"))

MATCH_DTYPE = np.dtype([("index", "<u4"), ("score", "<u2"), ("exact", "u1"), ("_pad", "u1")])
MATCH_INDICES_DTYPE = np.dtype([("index", "<u4"), ("score", "<u2"), ("exact", "u1"), ("_pad", "u1"), ("positions_begin", "<u4"), ("positions_len", "<u4")])


class FrizbeeError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(msg)
        self.code = code


class PanicError(FrizbeeError):
    """The reference would `panic!` here; the message is the reference's panic text."""


class CaseMatching(enum.IntEnum):  # src/lib.rs:357-368
    Ignore = 0
    Smart = 1
    Respect = 2


class UnicodeMatching(enum.IntEnum):  # src/lib.rs:379-392
    Ignore = 0
    Smart = 1
    Always = 2


class SortStrategy(enum.IntEnum):  # src/lib.rs:311-326
    ScoreThenIndexAsc = 0
    ScoreThenIndexDesc = 1
    IndexAsc = 2
    IndexDesc = 3


class Matching(enum.IntEnum):  # src/lib.rs:414-427
    Fuzzy = 0
    Exact = 1
    Prefix = 2
    Suffix = 3
    Substring = 4


@dataclass
class Scoring:  # src/lib.rs:439-478, defaults src/const.rs:1-10
    match_score: int = 12
    mismatch_penalty: int = 6
    gap_open_penalty: int = 5
    gap_extend_penalty: int = 1
    prefix_bonus: int = 12
    capitalization_bonus: int = 4
    matching_case_bonus: int = 4
    exact_match_bonus: int = 8
    delimiter_bonus: int = 4

    def as_list(self):
        return [self.match_score, self.mismatch_penalty, self.gap_open_penalty, self.gap_extend_penalty, self.prefix_bonus,
                self.capitalization_bonus, self.matching_case_bonus, self.exact_match_bonus, self.delimiter_bonus]


@dataclass
class Config:  # src/lib.rs:236-271
    max_typos: "int | None" = 0
    casing: CaseMatching = CaseMatching.Smart
    unicode: UnicodeMatching = UnicodeMatching.Smart
    sort: SortStrategy = SortStrategy.ScoreThenIndexAsc
    scoring: Scoring = field(default_factory=Scoring)
    # which reference CPU backend to be bit-exact against; (0, 0) = what frizbee would pick on this host
    pf_lanes: int = 0
    sw_lanes: int = 0
    matching: Matching = Matching.Fuzzy


class _CScoring(C.Structure):
    _fields_ = [(n, C.c_uint16) for n in ("match_score", "mismatch_penalty", "gap_open_penalty", "gap_extend_penalty", "prefix_bonus",
                                          "capitalization_bonus", "matching_case_bonus", "exact_match_bonus", "delimiter_bonus")]


class _CConfig(C.Structure):
    _fields_ = [("max_typos", C.c_int32), ("casing", C.c_int32), ("unicode", C.c_int32), ("sort", C.c_int32), ("scoring", _CScoring),
                ("pf_lanes", C.c_uint16), ("sw_lanes", C.c_uint16), ("matching", C.c_int32)]


class _CPattern(C.Structure):
    _fields_ = [("needle_utf8", C.c_void_p), ("needle_len", C.c_size_t), ("negated", C.c_int32), ("has_max_typos", C.c_int32), ("max_typos", C.c_int32),
                ("casing", C.c_int32), ("unicode", C.c_int32), ("has_scoring", C.c_int32), ("scoring", _CScoring), ("matching", C.c_int32)]


_lib = None

SYMBOLS = [
    "fzb_last_error", "fzb_config_default", "fzb_matcher_create", "fzb_matcher_clone", "fzb_matcher_free", "fzb_matcher_info", "fzb_matcher_set_pattern", "fzb_matcher_set_config",
    "fzb_corpus_upload", "fzb_corpus_from_device", "fzb_corpus_set_max_len", "fzb_corpus_set_uniform_len", "fzb_corpus_free", "fzb_corpus_len", "fzb_match_list", "fzb_match_list_into",
    "fzb_match_list_device", "fzb_match_list_sorted_device", "fzb_match_list_parallel", "fzb_matches_free", "fzb_radix_sort_matches", "fzb_k_merge_matches",
    "fzb_matcher_reserve", "fzb_debug_unicode_dfa_accepts", "fzb_set_profiling", "fzb_last_timings", "fzb_last_stage_timings", "fzb_last_counters",
    "fzb_multi_matcher_create", "fzb_multi_matcher_free", "fzb_multi_matcher_len", "fzb_multi_match_list", "fzb_multi_match_list_device",
    "fzb_parse_query", "fzb_patterns_free", "fzb_match_list_indices", "fzb_match_indices_free", "fzb_multi_match_list_indices",
    "fzb_match_list_indices_into", "fzb_multi_match_list_into", "fzb_multi_match_list_indices_into",
    "fzb_device_count", "fzb_shard_ranges", "fzb_corpus_upload_sharded", "fzb_sharded_corpus_free", "fzb_sharded_corpus_len", "fzb_sharded_corpus_shards",
    "fzb_sharded_corpus_shard", "fzb_match_list_parallel_sharded", "fzb_debug_lcs_dfa_accepts", "fzb_debug_cdfa_state", "fzb_debug_kmp_dfa_accepts",
    "fzb_merge_shard_runs", "fzb_corpus_build_view", "fzb_debug_reload_knobs", "fzb_matcher_shard_report",
    "fzb_rccl_unique_id", "fzb_shard_comm_create", "fzb_shard_comm_free", "fzb_shard_comm_rank", "fzb_shard_comm_world", "fzb_match_list_parallel_rccl",
    "fzb_shard_comm_last_exchange",
    "fzb_multi_matcher_set_patterns", "fzb_multi_matcher_set_config", "fzb_multi_matcher_reserve", "fzb_multi_matcher_clone", "fzb_multi_match_list_parallel",
    "fzb_multi_match_list_parallel_sharded", "fzb_multi_match_list_parallel_rccl", "fzb_multi_matcher_shard_report", "fzb_debug_device_allocs",
    "fzb_match_list_top", "fzb_match_list_top_device", "fzb_multi_match_list_top", "fzb_match_list_top_sharded", "fzb_multi_match_list_top_sharded",
    "fzb_corpus_reserve", "fzb_corpus_append", "fzb_corpus_truncate", "fzb_corpus_info", "fzb_debug_corpus_read",
    "fzb_corpus_remove", "fzb_corpus_remove_device", "fzb_corpus_replace", "fzb_corpus_edit_info",
    "fzb_match_list_top_indices", "fzb_match_list_top_indices_device", "fzb_matcher_reserve_top_indices", "fzb_multi_match_list_top_indices",
    "fzb_multi_match_list_top_indices_device", "fzb_multi_match_list_top_indices_fused", "fzb_multi_matcher_reserve_top_indices",
    "fzb_corpus_signature_info", "fzb_debug_needle_signature", "fzb_debug_signature_threshold", "fzb_debug_set_filter_grid",
    "fzb_corpus_set_bias", "fzb_corpus_update_bias", "fzb_corpus_clear_bias", "fzb_corpus_bias_info",
    "fzb_corpus_set_tags", "fzb_corpus_update_tags", "fzb_corpus_clear_tags", "fzb_corpus_set_scope", "fzb_corpus_scope_info",
    "fzb_corpus_generation", "fzb_subset_create", "fzb_subset_free", "fzb_subset_set_indices", "fzb_subset_from_scope", "fzb_subset_info", "fzb_subset_read",
    "fzb_match_list_subset", "fzb_match_list_top_subset", "fzb_match_list_top_subset_device", "fzb_match_list_top_indices_subset",
    "fzb_multi_match_list_subset", "fzb_multi_match_list_top_subset", "fzb_multi_match_list_top_subset_device", "fzb_multi_match_list_top_indices_subset",
    "fzb_debug_set_items_dfa_min", "fzb_debug_set_fused_capture", "fzb_debug_launch_grids", "fzb_corpus_signature_planes_info", "fzb_corpus_signature_repeat_planes_info",
    "fzb_prompt_list_device", "fzb_prompt_top_device",
    "fzb_facets_create", "fzb_facets_free", "fzb_facets_read", "fzb_facets_device", "fzb_matcher_set_facets", "fzb_multi_matcher_set_facets",
    "fzb_match_list_top_sections", "fzb_match_list_top_sections_device", "fzb_multi_match_list_top_sections", "fzb_multi_match_list_top_sections_device",
    "fzb_match_list_top_sections_indices", "fzb_match_list_top_sections_indices_device", "fzb_multi_match_list_top_sections_indices",
    "fzb_multi_match_list_top_sections_indices_device",
    "fzb_multi_matcher_create_groups", "fzb_multi_matcher_set_pattern_groups", "fzb_parse_query_groups", "fzb_query_groups_free",
    "fzb_multi_match_list_top_indices_groups", "fzb_multi_match_list_top_indices_groups_device", "fzb_multi_matcher_groups_positions_stride",
    "fzb_multi_matcher_reserve_top_indices_groups",
]


def lib():
    """Loads libfrizbee_hip.so (raises if it has not been built: there is no fallback path)."""
    global _lib
    if _lib is None:
        if not os.path.exists(_LIB_PATH):
            raise FrizbeeError(4, f"{_LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` (make -C frizbee_amd/csrc)")
        l = C.CDLL(_LIB_PATH)
        l.fzb_last_error.restype = C.c_char_p
        l.fzb_config_default.argtypes = [C.POINTER(_CConfig)]
        l.fzb_matcher_create.argtypes = [C.POINTER(_CConfig), C.c_char_p, C.c_size_t, C.POINTER(C.c_void_p)]
        l.fzb_matcher_clone.argtypes = [C.c_void_p, C.POINTER(C.c_void_p)]
        l.fzb_matcher_free.argtypes = [C.c_void_p]
        l.fzb_matcher_set_pattern.argtypes = [C.c_void_p, C.c_char_p, C.c_size_t]
        l.fzb_matcher_set_config.argtypes = [C.c_void_p, C.POINTER(_CConfig)]
        l.fzb_matcher_info.argtypes = [C.c_void_p, C.POINTER(C.c_int32)]
        l.fzb_corpus_upload.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(C.c_void_p)]
        l.fzb_corpus_from_device.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_size_t, C.c_uint64, C.POINTER(C.c_void_p)]
        l.fzb_corpus_set_max_len.argtypes = [C.c_void_p, C.c_uint32]
        l.fzb_corpus_set_uniform_len.argtypes = [C.c_void_p, C.c_uint32]
        l.fzb_corpus_free.argtypes = [C.c_void_p]
        l.fzb_corpus_len.argtypes = [C.c_void_p]
        l.fzb_corpus_len.restype = C.c_size_t
        l.fzb_match_list.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_size_t)]
        l.fzb_match_list_into.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_size_t, C.c_uint32, C.POINTER(C.c_void_p), C.POINTER(C.c_size_t)]
        l.fzb_match_list_device.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_size_t, C.c_uint32, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]
        l.fzb_match_list_sorted_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]
        l.fzb_match_list_parallel.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(C.c_void_p), C.POINTER(C.c_size_t)]
        l.fzb_matches_free.argtypes = [C.c_void_p]
        l.fzb_radix_sort_matches.argtypes = [C.c_void_p, C.c_size_t]
        l.fzb_k_merge_matches.argtypes = [C.c_int32, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]
        l.fzb_matcher_reserve.argtypes = [C.c_void_p, C.c_void_p]
        l.fzb_debug_unicode_dfa_accepts.argtypes = [C.c_void_p, C.c_char_p, C.c_size_t]
        l.fzb_set_profiling.argtypes = [C.c_void_p, C.c_int]
        l.fzb_last_timings.argtypes = [C.c_void_p, C.POINTER(C.c_float)]
        l.fzb_last_stage_timings.argtypes = [C.c_void_p, C.POINTER(C.c_float)]
        l.fzb_last_counters.argtypes = [C.c_void_p, C.POINTER(C.c_uint32)]
        l.fzb_multi_matcher_create.argtypes = [C.POINTER(_CConfig), C.POINTER(_CPattern), C.c_size_t, C.POINTER(C.c_void_p)]
        l.fzb_multi_matcher_free.argtypes = [C.c_void_p]
        l.fzb_parse_query.argtypes = [C.c_char_p, C.c_size_t, C.POINTER(C.POINTER(_CPattern)), C.POINTER(C.c_size_t)]
        l.fzb_patterns_free.argtypes = [C.POINTER(_CPattern), C.c_size_t]
        l.fzb_multi_matcher_len.argtypes = [C.c_void_p]
        l.fzb_multi_matcher_len.restype = C.c_size_t
        l.fzb_multi_match_list.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_size_t)]
        l.fzb_multi_match_list_device.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_size_t, C.c_uint32, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]
        l.fzb_match_list_indices.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(C.c_void_p), C.POINTER(C.c_size_t), C.POINTER(C.c_void_p)]
        l.fzb_match_indices_free.argtypes = [C.c_void_p, C.c_void_p]
        l.fzb_multi_match_list_indices.argtypes = l.fzb_match_list_indices.argtypes
        l.fzb_match_list_indices_into.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_uint32, C.POINTER(C.c_void_p), C.POINTER(C.c_size_t), C.POINTER(C.c_void_p)]
        l.fzb_multi_match_list_indices_into.argtypes = l.fzb_match_list_indices_into.argtypes
        l.fzb_multi_match_list_into.argtypes = l.fzb_match_list_into.argtypes
        l.fzb_device_count.argtypes = [C.POINTER(C.c_int)]
        l.fzb_shard_ranges.argtypes = [C.c_void_p, C.c_size_t, C.c_int, C.c_int, C.c_void_p]
        l.fzb_corpus_upload_sharded.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_int, C.POINTER(C.c_void_p)]
        l.fzb_sharded_corpus_free.argtypes = [C.c_void_p]
        l.fzb_sharded_corpus_len.argtypes = [C.c_void_p]
        l.fzb_sharded_corpus_len.restype = C.c_size_t
        l.fzb_sharded_corpus_shards.argtypes = [C.c_void_p]
        l.fzb_sharded_corpus_shard.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(C.c_int)]
        l.fzb_match_list_parallel_sharded.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_size_t)]
        l.fzb_matcher_shard_report.argtypes = [C.c_void_p]
        l.fzb_matcher_shard_report.restype = C.c_char_p
        l.fzb_merge_shard_runs.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_size_t)]
        l.fzb_corpus_build_view.argtypes = [C.c_void_p, C.POINTER(C.c_int)]
        l.fzb_rccl_unique_id.argtypes = [C.c_void_p]
        l.fzb_shard_comm_create.argtypes = [C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_void_p)]
        l.fzb_shard_comm_free.argtypes = [C.c_void_p]
        l.fzb_shard_comm_rank.argtypes = [C.c_void_p]
        l.fzb_shard_comm_world.argtypes = [C.c_void_p]
        l.fzb_match_list_parallel_rccl.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_int, C.POINTER(C.c_void_p), C.POINTER(C.c_size_t)]
        l.fzb_shard_comm_last_exchange.argtypes = [C.c_void_p, C.POINTER(C.c_uint64)]
        l.fzb_debug_lcs_dfa_accepts.argtypes = [C.c_void_p, C.c_char_p, C.c_size_t, C.POINTER(C.c_int32)]
        l.fzb_debug_cdfa_state.argtypes = [C.c_void_p, C.c_char_p, C.c_size_t, C.POINTER(C.c_int32)]
        l.fzb_debug_kmp_dfa_accepts.argtypes = [C.c_void_p, C.c_char_p, C.c_size_t, C.c_size_t]
        l.fzb_multi_matcher_set_patterns.argtypes = [C.c_void_p, C.POINTER(_CPattern), C.c_size_t]
        l.fzb_multi_matcher_set_config.argtypes = [C.c_void_p, C.POINTER(_CConfig)]
        l.fzb_multi_matcher_reserve.argtypes = [C.c_void_p, C.c_void_p]
        l.fzb_multi_matcher_clone.argtypes = [C.c_void_p, C.POINTER(C.c_void_p)]
        l.fzb_multi_matcher_create_groups.argtypes = [C.POINTER(_CConfig), C.POINTER(_CPattern), C.c_size_t, C.POINTER(C.c_uint32), C.POINTER(C.c_void_p)]
        l.fzb_multi_matcher_set_pattern_groups.argtypes = [C.c_void_p, C.POINTER(_CPattern), C.c_size_t, C.POINTER(C.c_uint32)]
        l.fzb_parse_query_groups.argtypes = [C.c_char_p, C.c_size_t, C.POINTER(C.POINTER(_CPattern)), C.POINTER(C.POINTER(C.c_uint32)), C.POINTER(C.c_size_t)]
        l.fzb_query_groups_free.argtypes = [C.POINTER(_CPattern), C.POINTER(C.c_uint32), C.c_size_t]
        l.fzb_query_groups_free.restype = None
        l.fzb_multi_match_list_parallel.argtypes = l.fzb_match_list_parallel.argtypes
        l.fzb_multi_match_list_parallel_sharded.argtypes = l.fzb_match_list_parallel_sharded.argtypes
        l.fzb_multi_match_list_parallel_rccl.argtypes = l.fzb_match_list_parallel_rccl.argtypes
        l.fzb_multi_matcher_shard_report.argtypes = [C.c_void_p]
        l.fzb_multi_matcher_shard_report.restype = C.c_char_p
        l.fzb_debug_device_allocs.argtypes = [C.POINTER(C.c_uint64)]
        l.fzb_match_list_top.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(C.c_void_p), C.POINTER(C.c_size_t), C.POINTER(C.c_uint64)]
        l.fzb_match_list_top_device.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]
        l.fzb_multi_match_list_top.argtypes = l.fzb_match_list_top.argtypes
        l.fzb_match_list_top_sharded.argtypes = l.fzb_match_list_top.argtypes
        l.fzb_multi_match_list_top_sharded.argtypes = l.fzb_match_list_top.argtypes
        l.fzb_corpus_reserve.argtypes = [C.c_void_p, C.c_size_t, C.c_uint64]
        l.fzb_corpus_append.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t]
        l.fzb_corpus_truncate.argtypes = [C.c_void_p, C.c_size_t]
        l.fzb_corpus_info.argtypes = [C.c_void_p, C.POINTER(C.c_uint64)]
        l.fzb_debug_corpus_read.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t)]
        l.fzb_corpus_remove.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t]
        l.fzb_corpus_remove_device.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t]
        l.fzb_corpus_replace.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]
        l.fzb_corpus_edit_info.argtypes = [C.c_void_p, C.POINTER(C.c_uint64)]
        l.fzb_match_list_top_indices.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(C.c_void_p), C.POINTER(C.c_size_t), C.POINTER(C.c_void_p), C.POINTER(C.c_uint64)]
        l.fzb_match_list_top_indices_device.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]
        l.fzb_matcher_reserve_top_indices.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_size_t]
        l.fzb_multi_match_list_top_indices.argtypes = l.fzb_match_list_top_indices.argtypes
        l.fzb_multi_match_list_top_indices_fused.argtypes = l.fzb_match_list_top_indices.argtypes
        l.fzb_multi_match_list_top_indices_device.argtypes = l.fzb_match_list_top_indices_device.argtypes
        l.fzb_multi_matcher_reserve_top_indices.argtypes = l.fzb_matcher_reserve_top_indices.argtypes
        l.fzb_corpus_signature_info.argtypes = [C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_uint64)]
        l.fzb_corpus_signature_planes_info.argtypes = l.fzb_corpus_signature_info.argtypes
        l.fzb_corpus_signature_repeat_planes_info.argtypes = l.fzb_corpus_signature_info.argtypes
        l.fzb_debug_needle_signature.argtypes = [C.c_void_p, C.POINTER(C.c_uint32), C.POINTER(C.c_int)]
        l.fzb_debug_signature_threshold.argtypes = []
        l.fzb_debug_signature_threshold.restype = C.c_uint32
        l.fzb_debug_set_filter_grid.argtypes = [C.c_int]
        l.fzb_debug_set_filter_grid.restype = None
        l.fzb_corpus_set_bias.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t]
        l.fzb_corpus_update_bias.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t]
        l.fzb_corpus_clear_bias.argtypes = [C.c_void_p]
        l.fzb_corpus_bias_info.argtypes = [C.c_void_p, C.POINTER(C.c_uint64)]
        l.fzb_corpus_set_tags.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t]
        l.fzb_corpus_update_tags.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t]
        l.fzb_corpus_clear_tags.argtypes = [C.c_void_p]
        l.fzb_corpus_set_scope.argtypes = [C.c_void_p, C.c_uint16, C.c_uint16]
        l.fzb_corpus_scope_info.argtypes = [C.c_void_p, C.POINTER(C.c_uint64)]
        l.fzb_debug_set_items_dfa_min.argtypes = [C.c_uint32]
        l.fzb_debug_set_items_dfa_min.restype = None
        l.fzb_debug_set_fused_capture.argtypes = [C.c_int]
        l.fzb_debug_set_fused_capture.restype = None
        l.fzb_debug_launch_grids.argtypes = [C.c_char_p, C.c_size_t, C.POINTER(C.c_size_t), C.c_int]
        l.fzb_corpus_generation.argtypes = [C.c_void_p, C.POINTER(C.c_uint64)]
        l.fzb_subset_create.argtypes = [C.c_void_p, C.POINTER(C.c_void_p)]
        l.fzb_subset_free.argtypes = [C.c_void_p]
        l.fzb_subset_free.restype = None
        l.fzb_subset_set_indices.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t]
        l.fzb_subset_from_scope.argtypes = [C.c_void_p, C.c_void_p, C.c_uint16, C.c_uint16]
        l.fzb_subset_info.argtypes = [C.c_void_p, C.POINTER(C.c_uint64)]
        l.fzb_subset_read.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t)]
        l.fzb_match_list_subset.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_size_t)]
        l.fzb_match_list_top_subset.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(C.c_void_p), C.POINTER(C.c_size_t), C.POINTER(C.c_uint64)]
        l.fzb_match_list_top_subset_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]
        l.fzb_multi_match_list_subset.argtypes = l.fzb_match_list_subset.argtypes
        l.fzb_multi_match_list_top_subset.argtypes = l.fzb_match_list_top_subset.argtypes
        l.fzb_multi_match_list_top_subset_device.argtypes = l.fzb_match_list_top_subset_device.argtypes
        l.fzb_prompt_list_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_size_t, C.c_uint32, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]
        l.fzb_prompt_top_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]
        l.fzb_match_list_top_indices_subset.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(C.c_void_p), C.POINTER(C.c_size_t), C.POINTER(C.c_void_p),
                                                        C.POINTER(C.c_uint64)]
        l.fzb_multi_match_list_top_indices_subset.argtypes = l.fzb_match_list_top_indices_subset.argtypes
        l.fzb_multi_match_list_top_indices_groups.argtypes = l.fzb_match_list_top_indices_subset.argtypes
        l.fzb_multi_match_list_top_indices_groups_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p,
                                                                     C.c_void_p]
        l.fzb_multi_matcher_groups_positions_stride.argtypes = [C.c_void_p, C.POINTER(C.c_size_t)]
        l.fzb_multi_matcher_reserve_top_indices_groups.argtypes = l.fzb_matcher_reserve_top_indices.argtypes
        l.fzb_facets_create.argtypes = [C.c_void_p, C.POINTER(C.c_void_p)]
        l.fzb_facets_free.argtypes = [C.c_void_p]
        l.fzb_facets_free.restype = None
        l.fzb_facets_read.argtypes = [C.c_void_p, C.POINTER(C.c_uint32)]
        l.fzb_facets_device.argtypes = [C.c_void_p]
        l.fzb_facets_device.restype = C.c_void_p
        l.fzb_matcher_set_facets.argtypes = [C.c_void_p, C.c_void_p]
        l.fzb_multi_matcher_set_facets.argtypes = [C.c_void_p, C.c_void_p]
        l.fzb_match_list_top_sections.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_size_t, C.c_void_p, C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_size_t),
                                                  C.POINTER(C.c_uint64)]
        l.fzb_match_list_top_sections_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]
        l.fzb_multi_match_list_top_sections.argtypes = l.fzb_match_list_top_sections.argtypes
        l.fzb_multi_match_list_top_sections_device.argtypes = l.fzb_match_list_top_sections_device.argtypes
        l.fzb_match_list_top_sections_indices.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_size_t, C.c_void_p, C.c_void_p, C.POINTER(C.c_void_p),
                                                          C.POINTER(C.c_size_t), C.POINTER(C.c_void_p), C.POINTER(C.c_uint64)]
        l.fzb_match_list_top_sections_indices_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t,
                                                                 C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]
        l.fzb_multi_match_list_top_sections_indices.argtypes = l.fzb_match_list_top_sections_indices.argtypes
        l.fzb_multi_match_list_top_sections_indices_device.argtypes = l.fzb_match_list_top_sections_indices_device.argtypes
        _lib = l
    return _lib


def _check(rc):
    if rc:
        msg = lib().fzb_last_error().decode("utf-8", "replace")
        raise (PanicError if rc == 2 else FrizbeeError)(rc, msg)


def _b(s):
    return s if isinstance(s, (bytes, bytearray)) else s.encode("utf-8")


def pack(haystacks):
    """list[str|bytes] -> (uint8 array of the concatenated bytes, uint64 exclusive end offsets) - the upload format."""
    bs = [_b(h) for h in haystacks]
    ends = np.cumsum(np.fromiter((len(b) for b in bs), dtype=np.uint64, count=len(bs)), dtype=np.uint64) if bs else np.zeros(0, np.uint64)
    data = np.frombuffer(b"".join(bs) + b"\0", dtype=np.uint8).copy()
    return data, ends


def _top(fn, handle, target, limit, copy):
    """A top-`limit` entry point of the C ABI -> (records, found)."""
    out, n, found = C.c_void_p(), C.c_size_t(), C.c_uint64()
    _check(fn(handle, target, limit, C.byref(out), C.byref(n), C.byref(found)))
    return _take(out, n, copy), found.value


SECTIONS_MAX, SECTION_LIMIT_MAX = 8, 1024  # include/frizbee_hip.h FZB_SECTIONS_MAX, FZB_SECTION_LIMIT_MAX


def _section_array(sections):
    """a sequence of (require, exclude) pairs -> the C ABI's fzb_section array (uint16 pairs)"""
    arr = np.zeros((len(sections), 2), np.uint16)
    for s, (require, exclude) in enumerate(sections):
        if not (0 <= int(require) <= 0xFFFF and 0 <= int(exclude) <= 0xFFFF):
            raise ValueError("a section is a pair of 16-bit masks (require, exclude): %r" % ((require, exclude),))
        arr[s] = (int(require), int(exclude))
    return arr


def _top_sections(fn, handle, corpus, sections, limit, subset, capture):
    """the host form of a sectioned top-`limit` call -> [(records, found)] in section order; one block comes back and is split here"""
    arr = _section_array(sections)
    S = len(arr)
    out, lens, found = C.c_void_p(), (C.c_size_t * max(S, 1))(), (C.c_uint64 * max(S, 1))()
    _check(fn(handle, corpus.h, arr.ctypes.data if S else None, S, limit, _h(subset), _h(capture), C.byref(out), lens, found))
    total = sum(lens[s] for s in range(S))
    block = np.zeros(total, MATCH_DTYPE)
    if out.value:
        if total:
            C.memmove(block.ctypes.data, out, total * 8)
        lib().fzb_matches_free(out)
    heads, at = [], 0
    for s in range(S):
        heads.append((block[at:at + lens[s]].copy(), int(found[s])))
        at += lens[s]
    return heads


def _top_sections_device(fn, handle, corpus, sections, limit, dev_out_ptr, capacity, dev_counts_ptr, stream, subset, capture):
    arr = _section_array(sections)
    _check(fn(handle, corpus.h, arr.ctypes.data if len(arr) else None, len(arr), limit, _h(subset), _h(capture), dev_out_ptr, capacity, dev_counts_ptr, stream))


def _top_sections_indices(fn, handle, corpus, sections, limit, subset, capture):
    """the host form of a sectioned top-`limit` call with matched positions -> [(list[MatchIndices], found)] in section order; one block of
    records and one dense position array come back and are split here"""
    arr = _section_array(sections)
    S = len(arr)
    out, pos, lens, found = C.c_void_p(), C.c_void_p(), (C.c_size_t * max(S, 1))(), (C.c_uint64 * max(S, 1))()
    _check(fn(handle, corpus.h, arr.ctypes.data if S else None, S, limit, _h(subset), _h(capture), C.byref(out), lens, C.byref(pos), found))
    block = _take_indices(out, C.c_size_t(sum(lens[s] for s in range(S))), pos) if out.value else []
    heads, at = [], 0
    for s in range(S):
        heads.append((block[at:at + lens[s]], int(found[s])))
        at += lens[s]
    return heads


def _top_sections_indices_device(fn, handle, corpus, sections, limit, dev_out_ptr, capacity, dev_positions_ptr, positions_capacity, dev_counts_ptr, stream, subset, capture):
    arr = _section_array(sections)
    _check(fn(handle, corpus.h, arr.ctypes.data if len(arr) else None, len(arr), limit, _h(subset), _h(capture), dev_out_ptr, capacity, dev_positions_ptr, positions_capacity,
              dev_counts_ptr, stream))


def _take(out, n, copy=True):
    """Result list of the C ABI -> numpy.  copy=False wraps the library's (pinned, pooled) buffer without copying and
    returns it to the pool when the array is garbage collected."""
    if copy or not n.value:
        arr = np.zeros(n.value, MATCH_DTYPE)
        if n.value:
            C.memmove(arr.ctypes.data, out, n.value * 8)
        lib().fzb_matches_free(out)
        return arr
    base = np.ctypeslib.as_array(C.cast(out, C.POINTER(C.c_uint8)), shape=(n.value * 8,))
    weakref.finalize(base, lib().fzb_matches_free, C.c_void_p(out.value))
    return base.view(MATCH_DTYPE)


class Corpus:
    """A haystack list packed and resident in HBM (what `match_list(&haystacks)` borrows, uploaded once)."""

    def __init__(self, haystacks=None, *, packed=None):
        data, ends = packed if packed is not None else pack(haystacks)
        data = np.ascontiguousarray(data, dtype=np.uint8)
        ends = np.ascontiguousarray(ends, dtype=np.uint64)
        self.h = C.c_void_p()
        self._keep = None
        _check(lib().fzb_corpus_upload(data.ctypes.data, ends.ctypes.data if len(ends) else None, len(ends), C.byref(self.h)))

    @classmethod
    def from_device(cls, dev_bytes_ptr, dev_ends_ptr, n, total_bytes, ends_are_u64=False, keep=None, max_len=0, uniform_len=0):
        """Borrow device memory already in the padded-16 layout (see include/frizbee_hip.h).  max_len: optional upper bound
        on the haystack length (0 = unknown).  uniform_len: optional promise that EVERY haystack has exactly this many bytes
        (the hot kernels then do not read the end offsets; Corpus(...) / fzb_corpus_upload detect it themselves)."""
        self = cls.__new__(cls)
        self.h = C.c_void_p()
        self._keep = keep
        _check(lib().fzb_corpus_from_device(dev_bytes_ptr, dev_ends_ptr, int(ends_are_u64), n, total_bytes, C.byref(self.h)))
        # (both promises are verified on the device against the end offsets when they are made; the uniform length first: it implies its bound)
        if uniform_len:
            _check(lib().fzb_corpus_set_uniform_len(self.h, uniform_len))
        if max_len:  # (beside a uniform length a looser bound is accepted and ignored, a tighter one refused)
            _check(lib().fzb_corpus_set_max_len(self.h, max_len))
        return self

    def build_view(self):
        """fzb_corpus_build_view: the streaming filter's interleaved view for a borrowed ragged corpus (an uploaded one has it already).
        Returns True when the corpus has a view afterwards."""
        built = C.c_int()
        _check(lib().fzb_corpus_build_view(self.h, C.byref(built)))
        return bool(built.value)

    def append(self, haystacks=None, *, packed=None):
        """fzb_corpus_append: the batch becomes haystacks len(self) .. of the resident list; only the batch crosses the link.  `packed` =
        pack() of the batch alone.  For a corpus made by Corpus(...) - `Corpus([])` followed by appends is how a picker starts."""
        data, ends = packed if packed is not None else pack(haystacks)
        data = np.ascontiguousarray(data, dtype=np.uint8)
        ends = np.ascontiguousarray(ends, dtype=np.uint64)
        _check(lib().fzb_corpus_append(self.h, data.ctypes.data, ends.ctypes.data if len(ends) else None, len(ends)))

    def reserve(self, items, nbytes):
        """fzb_corpus_reserve: room for `items` haystacks and `nbytes` padded bytes (<= raw bytes + 15 per haystack), so that appends
        within it - and, after Matcher.reserve, the queries between them - allocate no device memory."""
        _check(lib().fzb_corpus_reserve(self.h, items, nbytes))

    def truncate(self, n):
        """fzb_corpus_truncate: keep the first n haystacks (capacity is kept)."""
        _check(lib().fzb_corpus_truncate(self.h, n))

    def remove(self, indices):
        """fzb_corpus_remove: drops the haystacks named by `indices` (any order, repeats allowed); the others keep their order and are
        renumbered, as a list comprehension over the kept ones would.  Only the indices cross the link."""
        ix = np.ascontiguousarray(indices, dtype=np.uint32)
        _check(lib().fzb_corpus_remove(self.h, ix.ctypes.data if len(ix) else None, len(ix)))

    def remove_device(self, ptr, stride, count_ptr, max_count):
        """fzb_corpus_remove_device: the index list lies in HBM - entry k is the uint32 at byte k * stride of `ptr`, min(*count_ptr,
        max_count) entries.  stride 8 reads the records Matcher.match_list_device wrote over the whole corpus: drop everything that matches."""
        _check(lib().fzb_corpus_remove_device(self.h, ptr, stride, count_ptr, max_count))

    def replace(self, indices, haystacks=None, *, packed=None):
        """fzb_corpus_replace: batch item k becomes the content of haystack indices[k] (unique indices, any order).  `packed` = pack() of
        the batch alone."""
        ix = np.ascontiguousarray(indices, dtype=np.uint32)
        data, ends = packed if packed is not None else pack(haystacks)
        data = np.ascontiguousarray(data, dtype=np.uint8)
        ends = np.ascontiguousarray(ends, dtype=np.uint64)
        if len(ix) != len(ends):
            raise FrizbeeError(1, f"Corpus.replace: {len(ix)} indices for {len(ends)} haystacks")
        _check(lib().fzb_corpus_replace(self.h, ix.ctypes.data if len(ix) else None, len(ix), data.ctypes.data, ends.ctypes.data if len(ends) else None))

    EDIT_INFO_FIELDS = ("first", "bytes_written", "view_tiles", "temp_bytes")

    def edit_info(self):
        """fzb_corpus_edit_info as a dict (EDIT_INFO_FIELDS): the last remove / replace that changed the corpus."""
        out = (C.c_uint64 * 4)()
        _check(lib().fzb_corpus_edit_info(self.h, out))
        return dict(zip(self.EDIT_INFO_FIELDS, (int(v) for v in out)))

    INFO_FIELDS = ("items", "item_capacity", "bytes", "byte_capacity", "max_len", "uniform_len", "has_view", "view_nv", "outliers", "ends_u64", "regrows",
                   "h2d_bytes")
    DEBUG_ARRAYS = {"bytes": (0, np.uint8), "ends": (1, None), "vbytes": (2, np.uint8), "vgofs": (3, np.uint32), "vgnv": (4, np.uint8), "vlen": (5, np.uint16),
                    "vperm": (6, np.uint16), "vlong": (7, np.uint32), "sig": (8, np.uint32), "bias": (9, np.int16), "tags": (10, np.uint16),
                    "sig_planes": (11, np.uint64), "sig_planes2": (12, np.uint64)}

    def set_bias(self, values):
        """fzb_corpus_set_bias: one int16 per haystack (len(values) == len(self)), added to every record's score on the device before
        anything selects or orders - reported score = clamp(score + bias[index], 0, 65535).  `None` = fzb_corpus_clear_bias: the corpus
        answers as before any bias.  The bias belongs to the list: it survives set_pattern and follows append / truncate / remove / replace."""
        if values is None:
            _check(lib().fzb_corpus_clear_bias(self.h))
            return
        v = np.asarray(values)
        if v.size and (v.min() < -32768 or v.max() > 32767):
            raise FrizbeeError(1, "Corpus.set_bias: a bias is a signed 16-bit value")
        v = np.ascontiguousarray(v, dtype=np.int16)
        _check(lib().fzb_corpus_set_bias(self.h, v.ctypes.data if len(v) else None, len(v)))

    def _update_column(self, fn, who, indices, v):
        """the sparse update of either column: `v` = the values, already in the column's dtype"""
        ix = np.ascontiguousarray(indices, dtype=np.uint32)
        if len(ix) != len(v):
            raise FrizbeeError(1, f"{who}: {len(ix)} indices for {len(v)} values")
        _check(fn(self.h, ix.ctypes.data if len(ix) else None, v.ctypes.data if len(v) else None, len(ix)))

    def update_bias(self, indices, values):
        """fzb_corpus_update_bias: bias[indices[k]] = values[k] (unique indices in range; what a picker does when a file is opened).  A
        corpus without a bias gets an all-zero one first."""
        v = np.asarray(values)
        if v.size and (v.min() < -32768 or v.max() > 32767):
            raise FrizbeeError(1, "Corpus.update_bias: a bias is a signed 16-bit value")
        self._update_column(lib().fzb_corpus_update_bias, "Corpus.update_bias", indices, np.ascontiguousarray(v, dtype=np.int16))

    BIAS_INFO_FIELDS = ("has_bias", "capacity", "bias_hi", "device_bytes")

    def bias_info(self):
        """fzb_corpus_bias_info as a dict (BIAS_INFO_FIELDS)."""
        out = (C.c_uint64 * 4)()
        _check(lib().fzb_corpus_bias_info(self.h, out))
        return dict(zip(self.BIAS_INFO_FIELDS, (int(x) for x in out)))

    @staticmethod
    def _tags16(values, who):
        v = np.asarray(values)
        if v.size and (v.dtype.kind not in "iub" or v.min() < 0 or v.max() > 65535):
            raise FrizbeeError(1, f"{who}: tags are 16 caller-defined bits (0 .. 65535)")
        return np.ascontiguousarray(v, dtype=np.uint16)

    def set_tags(self, values):
        """fzb_corpus_set_tags: one uint16 of caller-defined bits per haystack (len(values) == len(self)).  Together with `set_scope` they
        decide which haystacks a query sees.  The tags belong to the list: they survive set_pattern and follow append (new haystacks: tag
        0) / truncate / remove / replace."""
        v = self._tags16(values, "Corpus.set_tags")
        _check(lib().fzb_corpus_set_tags(self.h, v.ctypes.data if len(v) else None, len(v)))

    def update_tags(self, indices, values):
        """fzb_corpus_update_tags: tags[indices[k]] = values[k] (unique indices in range).  A corpus without tags gets an all-zero array first."""
        ix = np.asarray(indices)
        if ix.size and (ix.min() < 0 or ix.max() > 0xFFFFFFFF):
            raise FrizbeeError(1, "Corpus.update_tags: an index is an unsigned 32-bit value")
        self._update_column(lib().fzb_corpus_update_tags, "Corpus.update_tags", ix, self._tags16(values, "Corpus.update_tags"))

    def clear_tags(self):
        """fzb_corpus_clear_tags: every tag 0 and the scope (0, 0) - the corpus answers as before any tags."""
        _check(lib().fzb_corpus_clear_tags(self.h))

    def set_scope(self, require=0, exclude=0):
        """fzb_corpus_set_scope: haystack i is visible iff (tags[i] & require) == require and (tags[i] & exclude) == 0; a query returns what
        it returns over the visible haystacks alone, every index that of the full list.  Host only - two words, no device work: the
        "toggle ignored files" keystroke.  (0, 0) is no scope."""
        for name, v in (("require", require), ("exclude", exclude)):
            if not 0 <= int(v) <= 65535:
                raise FrizbeeError(1, f"Corpus.set_scope: {name} is a 16-bit mask (0 .. 65535)")
        _check(lib().fzb_corpus_set_scope(self.h, int(require), int(exclude)))

    SCOPE_INFO_FIELDS = ("active", "capacity", "scope", "device_bytes")

    def scope_info(self):
        """fzb_corpus_scope_info as a dict (SCOPE_INFO_FIELDS), with `require` and `exclude` taken apart from the packed `scope` word."""
        out = (C.c_uint64 * 4)()
        _check(lib().fzb_corpus_scope_info(self.h, out))
        d = dict(zip(self.SCOPE_INFO_FIELDS, (int(x) for x in out)))
        d["require"], d["exclude"] = d["scope"] & 0xFFFF, d["scope"] >> 16
        return d

    def signature_info(self):
        """fzb_corpus_signature_info: (built, bytes) - whether the corpus has letter signatures and their size in device memory."""
        built, nbytes = C.c_int(), C.c_uint64()
        _check(lib().fzb_corpus_signature_info(self.h, C.byref(built), C.byref(nbytes)))
        return bool(built.value), int(nbytes.value)

    def signature_planes_info(self):
        """fzb_corpus_signature_planes_info: (built, bytes) - whether the corpus has the signatures' bit-planes and their size in device memory."""
        built, nbytes = C.c_int(), C.c_uint64()
        _check(lib().fzb_corpus_signature_planes_info(self.h, C.byref(built), C.byref(nbytes)))
        return bool(built.value), int(nbytes.value)

    def signature_repeat_planes_info(self):
        """fzb_corpus_signature_repeat_planes_info: (built, bytes) - whether the corpus has the repeat planes and their size in device memory."""
        built, nbytes = C.c_int(), C.c_uint64()
        _check(lib().fzb_corpus_signature_repeat_planes_info(self.h, C.byref(built), C.byref(nbytes)))
        return bool(built.value), int(nbytes.value)

    def info(self):
        """fzb_corpus_info as a dict (INFO_FIELDS)."""
        out = (C.c_uint64 * 12)()
        _check(lib().fzb_corpus_info(self.h, out))
        return dict(zip(self.INFO_FIELDS, (int(v) for v in out)))

    def debug_read(self, what):
        """Test hook (fzb_debug_corpus_read): one of the corpus' device arrays (DEBUG_ARRAYS) as a numpy array."""
        code, dtype = self.DEBUG_ARRAYS[what]
        if dtype is None:
            dtype = np.uint64 if self.info()["ends_u64"] else np.uint32
        n = C.c_size_t()
        rc = lib().fzb_debug_corpus_read(self.h, code, None, 0, C.byref(n))
        if rc != 5:  # (FZB_ERR_CAPACITY carries the size)
            _check(rc)
        buf = np.zeros(n.value, np.uint8)
        if n.value:
            _check(lib().fzb_debug_corpus_read(self.h, code, buf.ctypes.data, buf.nbytes, C.byref(n)))
        return buf.view(dtype)

    def generation(self):
        """the list's generation: bumped by every append / truncate / remove / replace that changed it (what a `Subset` is checked against)"""
        out = C.c_uint64()
        _check(lib().fzb_corpus_generation(self.h, C.byref(out)))
        return out.value

    def __len__(self):
        return lib().fzb_corpus_len(self.h)

    def __del__(self):
        try:
            if getattr(self, "h", None):
                lib().fzb_corpus_free(self.h)
                self.h = None
        except Exception:
            pass


SHARD_BY_COUNT, SHARD_BY_BYTES, SHARD_OVERSUBSCRIBE = 0, 1, 2  # include/frizbee_hip.h FZB_SHARD_*


class Subset:
    """A candidate set of one resident `Corpus`: strictly ascending haystack indices in HBM (fzb_subset).  The input (`subset=`) or the
    captured match set (`capture=`) of `Matcher.match_list` / `match_list_top` / `match_list_top_device` / `match_list_top_indices`: a query
    over a subset returns what it returns over an upload of those haystacks alone, every index mapped back to the full list's.  The
    reference has no counterpart: its caller builds a new Vec of the survivors."""

    def __init__(self, corpus):
        self.corpus = corpus  # (keeps the corpus alive: the handle points at it)
        self.h = C.c_void_p()
        _check(lib().fzb_subset_create(corpus.h, C.byref(self.h)))

    def set_indices(self, indices):
        """the subset becomes `indices` (strictly ascending, each below len(corpus)); one host-to-device copy"""
        a = np.asarray(indices)
        if a.size and (a.dtype.kind not in "iu" or int(a.min()) < 0 or int(a.max()) > 0xFFFFFFFF):
            raise ValueError("Subset.set_indices: the indices must be integers that fit uint32")
        a = np.ascontiguousarray(a, dtype=np.uint32)
        _check(lib().fzb_subset_set_indices(self.h, a.ctypes.data if len(a) else None, len(a)))

    def from_scope(self, require=0, exclude=0):
        """the subset becomes the haystacks visible under (require, exclude) over the corpus' tags, computed on the device"""
        _check(lib().fzb_subset_from_scope(self.h, self.corpus.h, require, exclude))

    def info(self):
        out = (C.c_uint64 * 4)()
        _check(lib().fzb_subset_info(self.h, out))
        return dict(known=int(out[0]), count=int(out[1]), capacity=int(out[2]), generation=int(out[3]))

    def read(self):
        """the indices as a uint32 array (a synchronous copy)"""
        out = np.zeros(max(len(self), 1), np.uint32)
        n = C.c_size_t()
        _check(lib().fzb_subset_read(self.h, out.ctypes.data, len(out), C.byref(n)))
        return out[: n.value].copy()

    def __len__(self):
        return self.info()["count"]  # (synchronises when the last capture left the count on the device only)

    def __del__(self):
        try:
            if getattr(self, "h", None) is not None and self.h:
                lib().fzb_subset_free(self.h)
                self.h = None
        except Exception:
            pass


def _h(subset):
    return None if subset is None else subset.h


FACET_WORDS, FACET_BITS = 34, 16  # include/frizbee_hip.h FZB_FACET_WORDS; facets.h


class Facets:
    """A facet sink of one resident `Corpus` (fzb_facets): the per-tag match counts of a query, counted on the device.  Attach it with
    `Matcher.set_facets` / `MultiMatcher.set_facets`; every query that honours it then fills it, and `read()` returns, for the match set A
    of the last such query (what `capture=` would hold: before scope, bias, `limit` and ordering): `matched` = |A|, `visible` = the members
    of A the corpus' scope shows (the call's `found`), `all_by_bit[b]` = the members of A whose tag has bit b (hidden ones included: a chip
    for an excluded bit shows what it hides), `visible_by_bit[b]` = the same over the visible members.  The reference has no counterpart:
    its caller counts over the Vec `match_list` returned."""

    def __init__(self, corpus):
        self.corpus = corpus  # (keeps the corpus alive: the handle points at it)
        self.h = C.c_void_p()
        _check(lib().fzb_facets_create(corpus.h, C.byref(self.h)))

    def read_words(self):
        """the block as FACET_WORDS uint32 (after a `_device` form: waits for that form's stream)"""
        out = (C.c_uint32 * FACET_WORDS)()
        _check(lib().fzb_facets_read(self.h, out))
        return np.frombuffer(out, dtype=np.uint32).copy()

    def read(self):
        w = self.read_words()
        return dict(matched=int(w[0]), visible=int(w[1]), all_by_bit=w[2:2 + FACET_BITS].copy(), visible_by_bit=w[2 + FACET_BITS:2 + 2 * FACET_BITS].copy())

    def device_ptr(self):
        """the block's address in HBM, for stream-ordered consumers"""
        return lib().fzb_facets_device(self.h)

    def __del__(self):
        try:
            if getattr(self, "h", None) is not None and self.h:
                lib().fzb_facets_free(self.h)
                self.h = None
        except Exception:
            pass


def device_count():
    n = C.c_int()
    _check(lib().fzb_device_count(C.byref(n)))
    return n.value


def shard_ranges(ends, nshards, by_bytes=False):
    """fzb_shard_ranges: the contiguous index ranges [(lo, hi)] the sharded upload cuts a list into (host arithmetic, no device)."""
    ends = np.ascontiguousarray(ends, dtype=np.uint64)
    out = np.zeros(nshards + 1, np.uint64)
    _check(lib().fzb_shard_ranges(ends.ctypes.data if len(ends) else None, len(ends), nshards, int(by_bytes), out.ctypes.data))
    return [(int(out[g]), int(out[g + 1])) for g in range(nshards)]


class ShardedCorpus:
    """A haystack list cut into contiguous shards, shard g resident on device g (fzb_corpus_upload_sharded): the multi-device form of
    `match_list_parallel`'s chunks (src/matcher/parallel.rs:55-63).  Everything below it is the C ABI - no torch, no process group."""

    def __init__(self, haystacks=None, ndev=1, *, packed=None, by_bytes=False, oversubscribe=False):
        data, ends = packed if packed is not None else pack(haystacks)
        data = np.ascontiguousarray(data, dtype=np.uint8)
        ends = np.ascontiguousarray(ends, dtype=np.uint64)
        self.h = C.c_void_p()
        flags = (SHARD_BY_BYTES if by_bytes else 0) | (SHARD_OVERSUBSCRIBE if oversubscribe else 0)
        _check(lib().fzb_corpus_upload_sharded(data.ctypes.data, ends.ctypes.data if len(ends) else None, len(ends), ndev, flags, C.byref(self.h)))

    def __len__(self):
        return lib().fzb_sharded_corpus_len(self.h)

    def shards(self):
        """[(lo, hi, device)] per shard"""
        out = []
        for g in range(lib().fzb_sharded_corpus_shards(self.h)):
            lo, hi, dev = C.c_uint64(), C.c_uint64(), C.c_int()
            _check(lib().fzb_sharded_corpus_shard(self.h, g, C.byref(lo), C.byref(hi), C.byref(dev)))
            out.append((lo.value, hi.value, dev.value))
        return out

    def __del__(self):
        try:
            if getattr(self, "h", None):
                lib().fzb_sharded_corpus_free(self.h)
                self.h = None
        except Exception:
            pass


def _c_config(config):
    c = _CConfig()
    c.max_typos = -1 if config.max_typos is None else int(config.max_typos)
    c.casing, c.unicode, c.sort = int(config.casing), int(config.unicode), int(config.sort)
    for name, v in zip([f[0] for f in _CScoring._fields_], config.scoring.as_list()):
        setattr(c.scoring, name, v)
    c.pf_lanes, c.sw_lanes = config.pf_lanes, config.sw_lanes
    c.matching = int(config.matching)
    return c


@dataclass
class Pattern:
    """Reference `Pattern` + `PatternConfig` (src/pattern.rs:9-18, 230-262), fuzzy matching only.  `None` fields inherit the
    matcher's config; max_typos=k is `Some(k)` (there is no way to ask for unlimited typos per pattern, as in the reference)."""
    needle: "str | bytes"
    negated: bool = False
    max_typos: "int | None" = None
    casing: "CaseMatching | None" = None
    unicode: "UnicodeMatching | None" = None
    scoring: "Scoring | None" = None
    matching: "Matching | None" = None


def launch_grids(clear=True):
    """fzb_debug_launch_grids: {kernel: (min_grid, max_grid, launches)} of the launches recorded since the record was last cleared (test hook:
    nothing is recorded unless FZB_DEBUG_CUS is set)"""
    n = C.c_size_t()
    _check(lib().fzb_debug_launch_grids(None, 0, C.byref(n), 0))
    buf = C.create_string_buffer(n.value + 1)
    _check(lib().fzb_debug_launch_grids(buf, n.value + 1, C.byref(n), 1 if clear else 0))
    return {f[0]: (int(f[1]), int(f[2]), int(f[3])) for f in (line.split() for line in buf.value.decode().splitlines())}


def device_allocs():
    """fzb_debug_device_allocs: device allocations the library has made in this process so far (test hook)"""
    n = C.c_uint64()
    _check(lib().fzb_debug_device_allocs(C.byref(n)))
    return n.value


def _c_patterns(pats):
    """list[Pattern] -> (the C array, the needle bytes it points into - keep them alive for the call)"""
    arr = (_CPattern * max(len(pats), 1))()
    keep = []
    for i, p in enumerate(pats):
        n = _b(p.needle)
        keep.append(n)
        arr[i].needle_utf8, arr[i].needle_len, arr[i].negated = C.cast(C.c_char_p(n), C.c_void_p), len(n), int(p.negated)
        arr[i].has_max_typos, arr[i].max_typos = int(p.max_typos is not None), int(p.max_typos or 0)
        arr[i].casing = -1 if p.casing is None else int(p.casing)
        arr[i].unicode = -1 if p.unicode is None else int(p.unicode)
        arr[i].has_scoring = int(p.scoring is not None)
        arr[i].matching = -1 if p.matching is None else int(p.matching)
        for name, v in zip([f[0] for f in _CScoring._fields_], (p.scoring or Scoring()).as_list()):
            setattr(arr[i].scoring, name, v)
    return arr, keep


def parse_query(query):
    """`Pattern::parse_query` (src/pattern.rs:186-222) -> list[Pattern]"""
    q = _b(query)
    arr, n = C.POINTER(_CPattern)(), C.c_size_t()
    _check(lib().fzb_parse_query(q, len(q), C.byref(arr), C.byref(n)))
    out = [Pattern(C.string_at(arr[i].needle_utf8, arr[i].needle_len).decode("utf-8"), negated=bool(arr[i].negated),
                   matching=None if arr[i].matching < 0 else Matching(arr[i].matching)) for i in range(n.value)]
    lib().fzb_patterns_free(arr, n.value)
    return out


def parse_query_groups(query):
    """`parse_query` with the any-of operator -> (list[Pattern], group_of): an atom that is exactly `|` joins the atoms around it into one
    group (`^src rs$ | py$ | go$ !test`); group_of[i] is the term id of pattern i, equal ids = the alternatives of one group.  Pass both to
    `MultiMatcher(patterns, config, groups=group_of)`."""
    q = _b(query)
    arr, ids, n = C.POINTER(_CPattern)(), C.POINTER(C.c_uint32)(), C.c_size_t()
    _check(lib().fzb_parse_query_groups(q, len(q), C.byref(arr), C.byref(ids), C.byref(n)))
    out = [Pattern(C.string_at(arr[i].needle_utf8, arr[i].needle_len).decode("utf-8"), negated=bool(arr[i].negated),
                   matching=None if arr[i].matching < 0 else Matching(arr[i].matching)) for i in range(n.value)]
    group_of = [int(ids[i]) for i in range(n.value)]
    lib().fzb_query_groups_free(arr, ids, n.value)
    return out, group_of


def _c_groups(groups, n):
    """group_of (one term id per pattern) -> the C array, or None for no grouping"""
    if groups is None:
        return None
    groups = [int(g) for g in groups]
    if len(groups) != n:
        raise ValueError("groups: one term id per pattern (%d ids for %d patterns)" % (len(groups), n))
    return (C.c_uint32 * max(n, 1))(*groups)


class _IterApi:
    """The per-item side of the reference's interface (`match_iter`, `match_one`, `match_iter_indices`, `match_one_indices`,
    src/matcher/mod.rs:277-371), served by ONE batched device pass in list order - there is no per-item CPU path."""

    def match_iter(self, haystacks):
        """`Matcher::match_iter` (src/matcher/mod.rs:290-301): the matches in haystack order, whatever `config.sort` says"""
        return iter(self.match_list_into(haystacks))

    def match_one(self, haystack, index=0):
        """`Matcher::match_one(haystack, index)` (src/matcher/mod.rs:341-349) -> one record of MATCH_DTYPE or None"""
        r = self.match_list_into([haystack], index_offset=index)
        return r[0] if len(r) else None

    def match_iter_indices(self, haystacks):
        """`Matcher::match_iter_indices` (src/matcher/mod.rs:321-334)"""
        return iter(self._indices_into(haystacks, 0))

    def match_one_indices(self, haystack, index=0):
        """`Matcher::match_one_indices` (src/matcher/mod.rs:357-371)"""
        r = self._indices_into([haystack], index)
        return r[0] if r else None


def fuzzy_match(haystacks, needle, config=None):
    """`iter::FuzzyMatchExt::fuzzy_match` (src/matcher/iter.rs:35-78) = `Matcher::new(needle, config).match_iter(haystacks)`"""
    return Matcher(needle, config).match_iter(haystacks)


def fuzzy_match_indices(haystacks, needle, config=None):
    """`iter::FuzzyMatchExt::fuzzy_match_indices` (src/matcher/iter.rs:80-126)"""
    return Matcher(needle, config).match_iter_indices(haystacks)


class MultiMatcher(_IterApi):
    """`Matcher::from_patterns(&patterns, &config)` (src/matcher/mod.rs:95-111; composition src/matcher/multi.rs:84-152)."""

    def __init__(self, patterns, config=None, groups=None):
        """groups: one term id per pattern (`parse_query_groups`' second result) - patterns with equal, adjacent ids are the alternatives of
        one any-of group (matches when any of them does, scores their maximum); None: every pattern is a term of its own"""
        self.config = config or Config()
        pats = [p if isinstance(p, Pattern) else Pattern(p) for p in patterns]
        arr, self._keep = _c_patterns(pats)
        c = _c_config(self.config)
        self.h = C.c_void_p()
        if groups is None:
            _check(lib().fzb_multi_matcher_create(C.byref(c), arr, len(pats), C.byref(self.h)))
        else:
            _check(lib().fzb_multi_matcher_create_groups(C.byref(c), arr, len(pats), _c_groups(groups, len(pats)), C.byref(self.h)))
        self.patterns = pats  # `Matcher::patterns` / `Matcher::config` (src/matcher/mod.rs:144-150) are these two attributes
        self.groups = None if groups is None else [int(g) for g in groups]

    def __len__(self):
        return lib().fzb_multi_matcher_len(self.h)

    def set_patterns(self, patterns, groups=None):
        """`Matcher::set_patterns` (src/matcher/mod.rs:170-176): skipped when the patterns are the same; otherwise the sub-matchers are
        rebuilt in place and their device buffers kept (a re-query per keystroke allocates nothing once `reserve` sized them).  `patterns`:
        a list of `Pattern` / needles, or a query string, which is parsed with `parse_query` (`Matcher::from_query`'s syntax).
        groups: as the constructor's; None makes every pattern a single term again."""
        if isinstance(patterns, (str, bytes)):
            patterns = parse_query(patterns)
        pats = [p if isinstance(p, Pattern) else Pattern(p) for p in patterns]
        arr, keep = _c_patterns(pats)
        if groups is None:
            _check(lib().fzb_multi_matcher_set_patterns(self.h, arr, len(pats)))
        else:
            _check(lib().fzb_multi_matcher_set_pattern_groups(self.h, arr, len(pats), _c_groups(groups, len(pats))))
        self.patterns, self._keep = pats, keep
        self.groups = None if groups is None else [int(g) for g in groups]

    def set_config(self, config):
        """`Matcher::set_config` (src/matcher/mod.rs:154-162); a change of `sort` alone rebuilds no sub-matcher"""
        c = _c_config(config)
        _check(lib().fzb_multi_matcher_set_config(self.h, C.byref(c)))
        self.config = config

    def set_facets(self, facets):
        """Attach a `Facets` sink (None: detach): the counts are those of the COMPOSITION's match set.  It stays attached across
        `set_patterns` / `set_config`; entry points that cannot fill it refuse the matcher until it is detached."""
        _check(lib().fzb_multi_matcher_set_facets(self.h, None if facets is None else facets.h))
        self.facets = facets  # (keeps the sink alive while the matcher points at it)

    def reserve(self, corpus):
        """Allocate every device buffer queries over `corpus` can need now: the composition, ordering and staging, and every sub-matcher
        slot for any needle of up to 64 bytes in any matching form (later keystrokes that do not add a pattern allocate nothing)."""
        _check(lib().fzb_multi_matcher_reserve(self.h, corpus.h))

    def clone(self):
        """`impl Clone for Matcher` (src/matcher/parallel.rs:46): an independent matcher with its own device buffers"""
        out = MultiMatcher.__new__(MultiMatcher)
        out.h = C.c_void_p()
        _check(lib().fzb_multi_matcher_clone(self.h, C.byref(out.h)))
        out.config, out.patterns, out._keep = self.config, list(self.patterns), list(self._keep)
        out.groups = None if getattr(self, "groups", None) is None else list(self.groups)
        return out

    def match_list_parallel(self, haystacks, threads):
        """`Matcher::match_list_parallel` (src/matcher/parallel.rs:18-89); identical result for every thread count."""
        cp = haystacks if isinstance(haystacks, Corpus) else Corpus(haystacks)
        out, n = C.c_void_p(), C.c_size_t()
        _check(lib().fzb_multi_match_list_parallel(self.h, cp.h, threads, C.byref(out), C.byref(n)))
        return _take(out, n)

    def match_list_parallel_sharded(self, sharded, copy=True):
        """`match_list_parallel` with one DEVICE per worker: the whole composition per shard on its device, the runs gathered and ordered
        once on the root.  Equals `match_list` on the unsharded list."""
        out, n = C.c_void_p(), C.c_size_t()
        _check(lib().fzb_multi_match_list_parallel_sharded(self.h, sharded.h, C.byref(out), C.byref(n)))
        return _take(out, n, copy)

    def shard_report(self):
        """How the runs of the last `match_list_parallel_sharded` reached the root (see `Matcher.shard_report`)."""
        return lib().fzb_multi_matcher_shard_report(self.h).decode()

    def match_list(self, haystacks, copy=True, *, subset=None, capture=None):
        """subset / capture (`Subset`s of the corpus, here and in the top-`limit` forms): the composition runs over `subset` only, and
        `capture` receives the indices of every haystack the COMPOSITION accepted - every non-negated pattern hit, no negated one did -
        before bias, scope, `limit` and ordering (see `Matcher.match_list`)."""
        cp = haystacks if isinstance(haystacks, Corpus) else Corpus(haystacks)
        out, n = C.c_void_p(), C.c_size_t()
        if subset is None and capture is None:
            _check(lib().fzb_multi_match_list(self.h, cp.h, C.byref(out), C.byref(n)))
        else:
            _check(lib().fzb_multi_match_list_subset(self.h, cp.h, _h(subset), _h(capture), C.byref(out), C.byref(n)))
        return _take(out, n, copy)

    def match_list_top(self, haystacks, limit, copy=True, *, subset=None, capture=None):
        """(`match_list(haystacks)[:limit]`, len(`match_list(haystacks)`)), selected and ordered on the device (see `Matcher.match_list_top`)."""
        cp = haystacks if isinstance(haystacks, Corpus) else Corpus(haystacks)
        if subset is None and capture is None:
            return _top(lib().fzb_multi_match_list_top, self.h, cp.h, limit, copy)
        out, n, found = C.c_void_p(), C.c_size_t(), C.c_uint64()
        _check(lib().fzb_multi_match_list_top_subset(self.h, cp.h, _h(subset), _h(capture), limit, C.byref(out), C.byref(n), C.byref(found)))
        return _take(out, n, copy), found.value

    def match_list_top_device(self, corpus, limit, dev_out_ptr, capacity, dev_count_ptr, stream=0, *, subset=None, capture=None):
        """`match_list_top` with the result left in HBM: `capacity` >= min(limit, len(corpus)) records at `dev_out_ptr`, two count words
        (records written, matches found) at `dev_count_ptr`; asynchronous on `stream`.  A matcher without a compiled pattern is refused."""
        _check(lib().fzb_multi_match_list_top_subset_device(self.h, corpus.h, _h(subset), _h(capture), limit, dev_out_ptr, capacity, dev_count_ptr, stream))

    def match_list_top_sections(self, corpus, sections, limit, *, subset=None, capture=None):
        """`Matcher.match_list_top_sections` behind the composition: [(records, found)] per (require, exclude) section, one device call."""
        return _top_sections(lib().fzb_multi_match_list_top_sections, self.h, corpus, sections, limit, subset, capture)

    def match_list_top_sections_device(self, corpus, sections, limit, dev_out_ptr, capacity, dev_counts_ptr, stream=0, *, subset=None, capture=None):
        """`Matcher.match_list_top_sections_device` behind the composition."""
        _top_sections_device(lib().fzb_multi_match_list_top_sections_device, self.h, corpus, sections, limit, dev_out_ptr, capacity, dev_counts_ptr, stream, subset, capture)

    def match_list_top_sharded(self, sharded, limit, copy=True):
        """`match_list_top` over a `ShardedCorpus`: every shard selects its own head, only those records reach the root."""
        return _top(lib().fzb_multi_match_list_top_sharded, self.h, sharded.h, limit, copy)

    def match_list_top_sections_indices(self, corpus, sections, limit, *, subset=None, capture=None):
        """`Matcher.match_list_top_sections_indices` behind the composition: every record's positions are the de-duplicated union over the
        non-negated patterns, as `match_list_indices` reports them."""
        return _top_sections_indices(lib().fzb_multi_match_list_top_sections_indices, self.h, corpus, sections, limit, subset, capture)

    def match_list_top_sections_indices_device(self, corpus, sections, limit, dev_out_ptr, capacity, dev_positions_ptr, positions_capacity, dev_counts_ptr, stream=0, *, subset=None,
                                               capture=None):
        """`Matcher.match_list_top_sections_indices_device` behind the composition; the positions' stride is the non-negated patterns' bytes, summed."""
        _top_sections_indices_device(lib().fzb_multi_match_list_top_sections_indices_device, self.h, corpus, sections, limit, dev_out_ptr, capacity, dev_positions_ptr,
                                     positions_capacity, dev_counts_ptr, stream, subset, capture)

    def match_list_top_indices(self, haystacks, limit, *, subset=None, capture=None):
        """(`match_list_indices(haystacks)[:limit]` with `index` = the corpus index, len of the full list) for the compiled patterns, in one
        fused device call with one host wait: the multi top stage, one traced pass per non-negated pattern over the head, the union of their
        positions and the pack, all on the device (see `Matcher.match_list_top_indices`)."""
        cp = haystacks if isinstance(haystacks, Corpus) else Corpus(haystacks)
        if subset is None and capture is None:
            return _top_indices(lib().fzb_multi_match_list_top_indices_fused, self.h, cp, limit)
        out, n, pos, found = C.c_void_p(), C.c_size_t(), C.c_void_p(), C.c_uint64()
        _check(lib().fzb_multi_match_list_top_indices_subset(self.h, cp.h, _h(subset), _h(capture), limit, C.byref(out), C.byref(n), C.byref(pos), C.byref(found)))
        return _take_indices(out, n, pos), found.value

    def match_list_top_indices_device(self, corpus, limit, dev_out_ptr, capacity, dev_positions_ptr, positions_capacity, dev_count_ptr, stream=0):
        """`match_list_top_indices` with the result left in HBM, asynchronous on `stream` (see `Matcher.match_list_top_indices_device`):
        `positions_capacity` >= min(limit, len(corpus)) x U uint32, U = the needle bytes of the non-negated patterns together.  A matcher
        without a compiled pattern is refused."""
        _check(lib().fzb_multi_match_list_top_indices_device(self.h, corpus.h, limit, dev_out_ptr, capacity, dev_positions_ptr, positions_capacity, dev_count_ptr, stream))

    def reserve_top_indices(self, corpus, limit, max_needle_bytes):
        """After `reserve(corpus)`: no `match_list_top_indices` call with this `limit` or a smaller one allocates device memory, also after
        `set_patterns` / `set_config` that add no pattern slot and keep every needle within `max_needle_bytes` bytes."""
        _check(lib().fzb_multi_matcher_reserve_top_indices(self.h, corpus.h, limit, max_needle_bytes))

    def match_list_top_indices_groups(self, corpus, limit, *, subset=None, capture=None):
        """`match_list_top_indices` for a matcher that may have any-of groups -> (list[MatchIndices], found), one fused device call with one
        host wait.  The records are `match_list_top`'s; a record's positions are the descending union without repeats of the positions of
        every plain non-negated pattern and of each group's CARRIER only: among the alternatives that match the haystack, the one with the
        largest key `score << 1 | exact`, on equal keys the first in query order.  A matcher without a group takes the ungrouped path
        (`match_list_top_indices`'s launches, allocations and bytes)."""
        cp = corpus if isinstance(corpus, Corpus) else Corpus(corpus)
        out, n, pos, found = C.c_void_p(), C.c_size_t(), C.c_void_p(), C.c_uint64()
        _check(lib().fzb_multi_match_list_top_indices_groups(self.h, cp.h, _h(subset), _h(capture), limit, C.byref(out), C.byref(n), C.byref(pos), C.byref(found)))
        return _take_indices(out, n, pos), found.value

    def match_list_top_indices_groups_device(self, corpus, limit, dev_out_ptr, capacity, dev_positions_ptr, positions_capacity, dev_count_ptr, stream=0, *, subset=None, capture=None):
        """`match_list_top_indices_groups` with the result left in HBM, asynchronous on `stream`: `match_list_top_indices_device`'s
        buffers and four count words, `positions_capacity` >= min(limit, len(corpus)) x `groups_positions_stride()` uint32."""
        _check(lib().fzb_multi_match_list_top_indices_groups_device(self.h, corpus.h, _h(subset), _h(capture), limit, dev_out_ptr, capacity, dev_positions_ptr, positions_capacity,
                                                                    dev_count_ptr, stream))

    def groups_positions_stride(self):
        """U_g: the needle bytes of the plain non-negated patterns + per group the largest needle bytes among its alternatives (without a
        group: the U of `match_list_top_indices_device`)."""
        out = C.c_size_t()
        _check(lib().fzb_multi_matcher_groups_positions_stride(self.h, C.byref(out)))
        return out.value

    def reserve_top_indices_groups(self, corpus, limit, max_needle_bytes):
        """`reserve_top_indices`, and what the grouped forms own on top: after `reserve(corpus)` and this, no `match_list_top_indices_groups`
        call with this `limit` or a smaller one allocates device memory, also after `set_patterns` to another grouping of the same slots."""
        _check(lib().fzb_multi_matcher_reserve_top_indices_groups(self.h, corpus.h, limit, max_needle_bytes))

    def match_list_indices(self, haystacks, selection=None):
        """`Matcher::match_list_indices` over the compiled patterns (`match_one_indices_multi`, src/matcher/multi.rs:56-82); see
        `Matcher.match_list_indices` for `selection`."""
        cp = haystacks if isinstance(haystacks, Corpus) else Corpus(haystacks)
        return _match_list_indices(lib().fzb_multi_match_list_indices, self.h, cp, selection)

    def _indices_into(self, haystacks, index_offset):
        cp = haystacks if isinstance(haystacks, Corpus) else Corpus(haystacks)
        return _match_list_indices(lib().fzb_multi_match_list_indices_into, self.h, cp, None, index_offset)

    def match_list_into(self, haystacks, first=0, count=None, index_offset=0):
        """`Matcher::match_list_into` over the compiled patterns (src/matcher/mod.rs:373-392): unsorted, input order"""
        cp = haystacks if isinstance(haystacks, Corpus) else Corpus(haystacks)
        count = len(cp) - first if count is None else count
        out, n = C.c_void_p(), C.c_size_t()
        _check(lib().fzb_multi_match_list_into(self.h, cp.h, first, count, index_offset, C.byref(out), C.byref(n)))
        return _take(out, n)

    def match_list_device(self, corpus, dev_out_ptr, capacity, dev_count_ptr, stream=0, first=0, count=None, index_offset=0):
        count = len(corpus) - first if count is None else count
        _check(lib().fzb_multi_match_list_device(self.h, corpus.h, first, count, index_offset, dev_out_ptr, capacity, dev_count_ptr, stream))

    def __del__(self):
        try:
            if getattr(self, "h", None):
                lib().fzb_multi_matcher_free(self.h)
                self.h = None
        except Exception:
            pass


def _match_list_indices(fn, handle, cp, selection, index_offset=None):
    sel = None if selection is None else np.ascontiguousarray(selection, dtype=np.uint32)
    if sel is not None and len(sel) == 0:
        return []
    out, n, pos = C.c_void_p(), C.c_size_t(), C.c_void_p()
    args = (handle, cp.h, sel.ctypes.data if sel is not None else None, 0 if sel is None else len(sel)) + (() if index_offset is None else (index_offset,))
    _check(fn(*args, C.byref(out), C.byref(n), C.byref(pos)))
    return _take_indices(out, n, pos)


def _top_indices(fn, handle, cp, limit):
    """A top-`limit` matched-positions entry point of the C ABI -> (list[MatchIndices], found)."""
    out, n, pos, found = C.c_void_p(), C.c_size_t(), C.c_void_p(), C.c_uint64()
    _check(fn(handle, cp.h, limit, C.byref(out), C.byref(n), C.byref(pos), C.byref(found)))
    return _take_indices(out, n, pos), found.value


def _take_indices(out, n, pos):
    """Records + flat positions of a *_indices result -> list[MatchIndices]; releases the library's arrays."""
    try:
        recs = np.ctypeslib.as_array(C.cast(out, C.POINTER(C.c_uint8)), shape=(max(n.value, 1) * 16,))[: n.value * 16].view(MATCH_INDICES_DTYPE).copy()
        total = int((recs["positions_begin"].astype(np.int64) + recs["positions_len"]).max()) if len(recs) else 0
        flat = np.ctypeslib.as_array(C.cast(pos, C.POINTER(C.c_uint32)), shape=(max(total, 1),)).copy()
    finally:
        lib().fzb_match_indices_free(out, pos)
    return [MatchIndices(int(r["index"]), int(r["score"]), bool(r["exact"]), flat[int(r["positions_begin"]) : int(r["positions_begin"]) + int(r["positions_len"])].tolist())
            for r in recs]


class MatchIndices:
    """`frizbee::MatchIndices` (src/lib.rs:189-199)"""

    __slots__ = ("index", "score", "exact", "indices")

    def __init__(self, index, score, exact, indices):
        self.index, self.score, self.exact, self.indices = index, score, exact, indices

    def __eq__(self, o):
        if not isinstance(o, MatchIndices):
            return NotImplemented
        return (self.index, self.score, self.exact, self.indices) == (o.index, o.score, o.exact, o.indices)

    def __repr__(self):
        return f"MatchIndices(index={self.index}, score={self.score}, exact={self.exact}, indices={self.indices})"


class Matcher(_IterApi):
    """`frizbee::Matcher` for one (non-negated, fuzzy) pattern: `Matcher::new(needle, &config)` (src/matcher/mod.rs:90-92)."""

    def __init__(self, needle, config=None):
        self.config = config or Config()
        c = _c_config(self.config)
        n = _b(needle)
        self.needle = n
        self.h = C.c_void_p()
        _check(lib().fzb_matcher_create(C.byref(c), n, len(n), C.byref(self.h)))

    def set_pattern(self, needle):
        """`Matcher::set_pattern` (src/matcher/mod.rs:154-165): same matcher, new needle; the device workspace is kept."""
        n = _b(needle)
        _check(lib().fzb_matcher_set_pattern(self.h, n, len(n)))
        self.needle = n

    def set_config(self, config):
        """`Matcher::set_config` (src/matcher/mod.rs:143-152)"""
        c = _c_config(config)
        _check(lib().fzb_matcher_set_config(self.h, C.byref(c)))
        self.config = config

    def info(self):
        out = (C.c_int32 * 6)()
        _check(lib().fzb_matcher_info(self.h, out))
        return dict(pf_lanes=out[0], sw_lanes=out[1], use_u8=bool(out[2]), case_sensitive=bool(out[3]), unicode=bool(out[4]), rows=out[5])

    def _corpus(self, haystacks):
        return haystacks if isinstance(haystacks, Corpus) else Corpus(haystacks)

    def match_list(self, haystacks, copy=True, *, subset=None, capture=None):
        """`Matcher::match_list` (src/matcher/mod.rs:212-222). `haystacks` is a list of str/bytes or a resident `Corpus`.
        subset / capture (`Subset`s of that corpus, here and in the top-`limit` forms): the query runs over `subset` only, and `capture`
        receives the indices of every haystack the matcher accepted - before bias, scope, `limit` and ordering."""
        cp = self._corpus(haystacks)
        out, n = C.c_void_p(), C.c_size_t()
        if subset is None and capture is None:
            _check(lib().fzb_match_list(self.h, cp.h, C.byref(out), C.byref(n)))
        else:
            _check(lib().fzb_match_list_subset(self.h, cp.h, _h(subset), _h(capture), C.byref(out), C.byref(n)))
        return _take(out, n, copy)

    def match_list_top(self, haystacks, limit, copy=True, *, subset=None, capture=None):
        """(`match_list(haystacks)[:limit]`, len(`match_list(haystacks)`)): the threshold score, the records of the head (ties at the cut
        as the stable sort breaks them) and their order are found on the device; only `limit` records are copied.  The reference has no
        such call - its caller truncates the Vec `match_list` returns (src/matcher/mod.rs:212-222)."""
        if subset is None and capture is None:
            return _top(lib().fzb_match_list_top, self.h, self._corpus(haystacks).h, limit, copy)
        out, n, found = C.c_void_p(), C.c_size_t(), C.c_uint64()
        _check(lib().fzb_match_list_top_subset(self.h, self._corpus(haystacks).h, _h(subset), _h(capture), limit, C.byref(out), C.byref(n), C.byref(found)))
        return _take(out, n, copy), found.value

    def match_list_top_device(self, corpus, limit, dev_out_ptr, capacity, dev_count_ptr, stream=0, *, subset=None, capture=None):
        """`match_list_top` with the result left in HBM: `capacity` >= min(limit, len(corpus)) records at `dev_out_ptr`, two count words
        (records written, matches found) at `dev_count_ptr`; asynchronous on `stream`."""
        if subset is None and capture is None:
            _check(lib().fzb_match_list_top_device(self.h, corpus.h, limit, dev_out_ptr, capacity, dev_count_ptr, stream))
        else:
            _check(lib().fzb_match_list_top_subset_device(self.h, corpus.h, _h(subset), _h(capture), limit, dev_out_ptr, capacity, dev_count_ptr, stream))

    def prompt_list_device(self, corpus, dev_out_ptr, capacity, dev_count_ptr, stream=0, *, subset=None, first=0, count=None, index_offset=0):
        """The empty prompt's index-ordered list left in HBM - `match_list_device` for a matcher whose needle is empty (the `_device` forms
        refuse one): the haystacks of the range, or of `subset`, visible under the corpus' scope, score = the clamped bias (0 without one).
        At most `capacity` records at `dev_out_ptr`, two count words (records written, found) at `dev_count_ptr`; asynchronous on `stream`."""
        count = len(corpus) - first if count is None else count
        _check(lib().fzb_prompt_list_device(self.h, corpus.h, _h(subset), first, count, index_offset, dev_out_ptr, capacity, dev_count_ptr, stream))

    def prompt_top_device(self, corpus, limit, dev_out_ptr, capacity, dev_count_ptr, stream=0, *, subset=None):
        """The empty prompt's ordered head left in HBM - `match_list_top_device` for a matcher whose needle is empty: `capacity` >=
        min(limit, len(corpus)) records at `dev_out_ptr`, two count words (records written, found) at `dev_count_ptr`; asynchronous on
        `stream`."""
        _check(lib().fzb_prompt_top_device(self.h, corpus.h, _h(subset), limit, dev_out_ptr, capacity, dev_count_ptr, stream))

    def match_list_top_sections(self, corpus, sections, limit, *, subset=None, capture=None):
        """A picker's sections in one device call: `sections` is a sequence of (require, exclude) pairs over the corpus' 16 tag bits (the
        scope's predicate; at most SECTIONS_MAX = 8, `limit` <= SECTION_LIMIT_MAX = 1024).  Returns [(records, found)] in section order:
        element s is what `match_list_top(corpus, limit)` returns over a corpus whose scope is the corpus' own scope AND section s -
        from ONE pass of the filter and the scorers and one host wait.  Sections may overlap, repeat or be empty; (0, 0) is everything.
        The reference has no such call: its caller splits the Vec `match_list` returned."""
        return _top_sections(lib().fzb_match_list_top_sections, self.h, corpus, sections, limit, subset, capture)

    def match_list_top_sections_device(self, corpus, sections, limit, dev_out_ptr, capacity, dev_counts_ptr, stream=0, *, subset=None, capture=None):
        """`match_list_top_sections` with the result left in HBM: `capacity` >= len(sections) * limit records at `dev_out_ptr`, section s's
        head at record s * limit; 2 * len(sections) count words at `dev_counts_ptr` ([2s] = records of head s, [2s + 1] = matches in
        section s); asynchronous on `stream`.  What lies behind a head inside its slab is unspecified."""
        _top_sections_device(lib().fzb_match_list_top_sections_device, self.h, corpus, sections, limit, dev_out_ptr, capacity, dev_counts_ptr, stream, subset, capture)

    def match_list_top_sharded(self, sharded, limit, copy=True):
        """`match_list_top` over a `ShardedCorpus`: every shard selects its own head, only those records reach the root."""
        return _top(lib().fzb_match_list_top_sharded, self.h, sharded.h, limit, copy)

    def match_list_top_sections_indices(self, corpus, sections, limit, *, subset=None, capture=None):
        """`match_list_top_sections` with the matched byte positions of every head's records: [(list[MatchIndices], found)] in section
        order.  Element s is what `match_list_top_indices(corpus, limit)` returns over a corpus whose scope is the corpus' own scope AND
        section s - from ONE pass of the filter and the scorers, one traced pass over the heads and one host wait.  A haystack that sits
        in several sections appears in each head with its positions.  An empty needle returns the prompt's records with no positions."""
        return _top_sections_indices(lib().fzb_match_list_top_sections_indices, self.h, corpus, sections, limit, subset, capture)

    def match_list_top_sections_indices_device(self, corpus, sections, limit, dev_out_ptr, capacity, dev_positions_ptr, positions_capacity, dev_counts_ptr, stream=0, *, subset=None,
                                               capture=None):
        """`match_list_top_sections_indices` with the result left in HBM, asynchronous on `stream`: the heads DENSELY concatenated in section
        order at `dev_out_ptr` (`capacity` >= len(sections) * min(limit, len(corpus)) records of MATCH_INDICES_DTYPE), their dense positions
        at `dev_positions_ptr` (`positions_capacity` >= that many records * len(needle) uint32), and 2 S + 4 count words at `dev_counts_ptr`,
        S = len(sections): [2s] = records of head s, [2s + 1] = matches in section s, [2S] = records in all, [2S + 2] = positions written,
        [2S + 3] = 0 (non-zero: the traced pass disagreed with the stage).  Not for an empty needle."""
        _top_sections_indices_device(lib().fzb_match_list_top_sections_indices_device, self.h, corpus, sections, limit, dev_out_ptr, capacity, dev_positions_ptr, positions_capacity,
                                     dev_counts_ptr, stream, subset, capture)

    def match_list_top_indices(self, haystacks, limit, *, subset=None, capture=None):
        """(the first min(limit, found) entries of `Matcher::match_list_indices` over the whole list, found): what a picker shows after a
        keystroke.  `index` is the corpus index, `indices` the matched byte positions in reverse order.  The reference's caller truncates
        the Vec (src/matcher/mod.rs:234-275); here the top stage, a traced pass over its head and the packing of the positions are ONE
        device call with one host wait."""
        if subset is None and capture is None:
            return _top_indices(lib().fzb_match_list_top_indices, self.h, self._corpus(haystacks), limit)
        out, n, pos, found = C.c_void_p(), C.c_size_t(), C.c_void_p(), C.c_uint64()
        _check(lib().fzb_match_list_top_indices_subset(self.h, self._corpus(haystacks).h, _h(subset), _h(capture), limit, C.byref(out), C.byref(n), C.byref(pos), C.byref(found)))
        return _take_indices(out, n, pos), found.value

    def match_list_top_indices_device(self, corpus, limit, dev_out_ptr, capacity, dev_positions_ptr, positions_capacity, dev_count_ptr, stream=0):
        """`match_list_top_indices` with the result left in HBM, asynchronous on `stream`: `capacity` >= min(limit, len(corpus)) records of
        MATCH_INDICES_DTYPE at `dev_out_ptr`, `positions_capacity` >= min(limit, len(corpus)) * len(needle) uint32 at `dev_positions_ptr`
        (dense: `positions_begin` / `positions_len` index it), four count words at `dev_count_ptr`: records written, matches found,
        positions written, 0 (non-zero: the traced pass disagreed with the top stage)."""
        _check(lib().fzb_match_list_top_indices_device(self.h, corpus.h, limit, dev_out_ptr, capacity, dev_positions_ptr, positions_capacity, dev_count_ptr, stream))

    def reserve_top_indices(self, corpus, limit, max_needle_bytes):
        """After `reserve(corpus)`: no `match_list_top_indices` call with this `limit` or a smaller one, on a needle of up to
        `max_needle_bytes` bytes, allocates device memory - also across `set_pattern` / `set_config`."""
        _check(lib().fzb_matcher_reserve_top_indices(self.h, corpus.h, limit, max_needle_bytes))

    def match_list_parallel(self, haystacks, threads):
        """`Matcher::match_list_parallel` (src/matcher/parallel.rs:18-89); identical result for every thread count."""
        cp = self._corpus(haystacks)
        out, n = C.c_void_p(), C.c_size_t()
        _check(lib().fzb_match_list_parallel(self.h, cp.h, threads, C.byref(out), C.byref(n)))
        return _take(out, n)

    def match_list_parallel_sharded(self, sharded, copy=True):
        """`Matcher::match_list_parallel` with one DEVICE per worker (fzb_match_list_parallel_sharded): per-shard pipeline, the runs
        gathered device to device on the root and ordered there once (src/matcher/parallel.rs:66-87's result).  Equals `match_list`
        on the unsharded list."""
        out, n = C.c_void_p(), C.c_size_t()
        _check(lib().fzb_match_list_parallel_sharded(self.h, sharded.h, C.byref(out), C.byref(n)))
        return _take(out, n, copy)

    def shard_report(self):
        """How the runs of the last `match_list_parallel_sharded` reached the root (fzb_matcher_shard_report): gather form and, per shard,
        same device / peer access enabled / peer access refused (the runtime then stages the copy through host memory)."""
        return lib().fzb_matcher_shard_report(self.h).decode()

    @staticmethod
    def merge_args(run_ptrs, count_ptrs, run_caps):
        """Marshal the arguments of `merge_shard_runs` once (callers that merge the same buffers every step)."""
        n = len(run_ptrs)
        return ((C.c_void_p * max(n, 1))(*[int(p) for p in run_ptrs]), (C.c_void_p * max(n, 1))(*[int(p) for p in count_ptrs]),
                (C.c_size_t * max(n, 1))(*[int(c) for c in run_caps]), n)

    def merge_shard_runs(self, runs, cnts, caps, n=None, stream=0, copy=True):
        """fzb_merge_shard_runs: index-ordered per-shard runs resident on the current device (ascending shard order; each count pointer
        = the (records written, matches found) pair fzb_match_list_device wrote, in device memory) -> `match_list`'s ordered result on the
        host.  Concatenation + reverse / stable radix sort on the device.  Arguments: lists of addresses, or `merge_args(...)` unpacked."""
        if n is None:
            runs, cnts, caps, n = self.merge_args(runs, cnts, caps)
        out, ln = C.c_void_p(), C.c_size_t()
        _check(lib().fzb_merge_shard_runs(self.h, runs, cnts, caps, n, stream, C.byref(out), C.byref(ln)))
        return _take(out, ln, copy)

    def match_list_indices(self, haystacks, selection=None):
        """`Matcher::match_list_indices` (src/matcher/mod.rs:234-275): list of `MatchIndices` (src/lib.rs:189-199), the matched byte
        positions in reverse order.  `selection` (corpus indices) plays the role of the haystack list - typically the top of a
        `match_list` result over a resident `Corpus`; `index` then numbers the selection."""
        return _match_list_indices(lib().fzb_match_list_indices, self.h, self._corpus(haystacks), selection)

    def _indices_into(self, haystacks, index_offset):
        return _match_list_indices(lib().fzb_match_list_indices_into, self.h, self._corpus(haystacks), None, index_offset)

    def match_list_into(self, haystacks, first=0, count=None, index_offset=0):
        """`Specialized::match_list(haystacks, haystack_index_offset, &mut matches)` (src/matcher/algo.rs:78-103): unsorted, input order."""
        cp = self._corpus(haystacks)
        count = len(cp) - first if count is None else count
        out, n = C.c_void_p(), C.c_size_t()
        _check(lib().fzb_match_list_into(self.h, cp.h, first, count, index_offset, C.byref(out), C.byref(n)))
        return _take(out, n)

    def match_list_device(self, corpus, dev_out_ptr, capacity, dev_count_ptr, stream=0, first=0, count=None, index_offset=0):
        """Device-resident form: records + count stay in HBM, asynchronous on `stream` (a hipStream_t handle)."""
        count = len(corpus) - first if count is None else count
        _check(lib().fzb_match_list_device(self.h, corpus.h, first, count, index_offset, dev_out_ptr, capacity, dev_count_ptr, stream))

    def match_list_sorted_device(self, corpus, dev_out_ptr, capacity, dev_count_ptr, stream=0):
        """`match_list` with the result left in HBM, already in `config.sort` order (device-side reverse + radix sort)."""
        _check(lib().fzb_match_list_sorted_device(self.h, corpus.h, dev_out_ptr, capacity, dev_count_ptr, stream))

    def set_facets(self, facets):
        """Attach a `Facets` sink (None: detach).  It stays attached across `set_pattern` / `set_config`; entry points that cannot fill it
        refuse the matcher until it is detached."""
        _check(lib().fzb_matcher_set_facets(self.h, None if facets is None else facets.h))
        self.facets = facets  # (keeps the sink alive while the matcher points at it)

    def reserve(self, corpus):
        """Allocate every device buffer queries over `corpus` can need now, so that no later query (also after set_pattern) allocates."""
        _check(lib().fzb_matcher_reserve(self.h, corpus.h))

    def set_profiling(self, on=True):
        _check(lib().fzb_set_profiling(self.h, int(on)))

    def last_timings_ms(self):
        out = (C.c_float * 4)()
        _check(lib().fzb_last_timings(self.h, out))
        return dict(filter=out[0], total=out[1], calls=int(out[2]))

    def last_stage_timings_ms(self):
        """HIP-event averages of the profiled calls, by stage (filter kernel / compaction + lane-exact prefilter / scorers / whole pipeline)"""
        out = (C.c_float * 6)()
        _check(lib().fzb_last_stage_timings(self.h, out))
        return dict(filter=out[0], compaction_and_window=out[1], scorers=out[2], total=out[3], calls=int(out[4]))

    def last_counters(self):
        out = (C.c_uint32 * 4)()
        _check(lib().fzb_last_counters(self.h, out))
        return dict(filter_survivors=out[0], kept_by_exact_prefilter=out[1], generic_scored=out[2], multi_chunk_scored=out[3])

    def __del__(self):
        try:
            if getattr(self, "h", None):
                lib().fzb_matcher_free(self.h)
                self.h = None
        except Exception:
            pass


def _needle_extends(matching, max_typos, prev_needle, needle, prev_path, path):
    """The narrowing premise for ONE non-negated needle (tests/test_oracle_narrowing_premise.py): fuzzy matching, max_typos == 0, `needle` is
    `prev_needle` plus a non-empty suffix, and both report the same (unicode, pf_lanes, sw_lanes).  `NarrowingMatcher` asks it for its one
    needle, `NarrowingQuery` for every pattern that changed."""
    if matching != Matching.Fuzzy or max_typos != 0:
        return False
    if not prev_needle or len(needle) <= len(prev_needle) or not needle.startswith(prev_needle):
        return False
    return path == prev_path


class NarrowingMatcher:
    """The keystroke loop as a picker writes it: a `Matcher` over one resident `Corpus` and two `Subset`s that alternate.  Every query
    captures its match set; the next query runs over that capture instead of the whole list when ALL of these hold: fuzzy matching,
    max_typos == 0, the new needle is the previous one plus a non-empty suffix, `Matcher.info()` reports the same unicode path and lane
    pair for both needles, the corpus generation is unchanged, the captured count is known, and it is at most max_fraction x len(corpus).
    (The same unicode path: a non-ASCII suffix moves the matcher to the unicode kernels, whose case folding accepts haystacks the ASCII
    automaton of the shorter needle rejected - the subset relation is not given.  Smart case going from insensitive to sensitive only
    rejects more and needs no condition.  tests/test_oracle_narrowing_premise.py holds the premise against the oracle.)
    max_fraction: None = DEFAULT_MAX_FRACTION = 0.8 x the largest candidate fraction at which tools/bench_subset.py measured the narrowed
    call not slower than the whole-list call.  On its two (dense, synthetic) lists that was none - 5.5 to 17 % of the list as candidates,
    of which 78 - 90 % match again: narrowed + 10 to + 19 us (profiles/subset.txt) - so the default is 0.0: never narrow.  A caller whose
    lists thin out faster passes its own."""

    DEFAULT_MAX_FRACTION = 0.0

    def __init__(self, corpus, config=None, max_fraction=None):
        self.corpus = corpus
        self.config = config or Config()
        self.max_fraction = self.DEFAULT_MAX_FRACTION if max_fraction is None else float(max_fraction)
        self.matcher = Matcher("", self.config)
        self.subsets = [Subset(corpus), Subset(corpus)]
        self._cur = None         # index of the subset that holds the previous query's capture
        self._prev = None        # (needle bytes, (unicode, pf_lanes, sw_lanes), corpus generation) of that query
        self.last_narrowed = False

    def set_facets(self, facets):
        """pass a `Facets` sink of the corpus on to the matcher (None: detach): every query fills it - over the previous capture when it
        narrowed, whose members are the only haystacks that can still match"""
        self.matcher.set_facets(facets)

    def _may_narrow(self, needle, path):
        if self._cur is None or self._prev is None:
            return False
        prev_needle, prev_path, prev_gen = self._prev
        cfg = self.config
        if not _needle_extends(cfg.matching, cfg.max_typos, prev_needle, needle, prev_path, path):
            return False
        if self.corpus.generation() != prev_gen:
            return False
        cap = self.subsets[self._cur]
        out = (C.c_uint64 * 4)()
        _check(lib().fzb_subset_info(cap.h, out))
        return self.max_fraction > 0 and bool(out[0]) and out[1] <= self.max_fraction * len(self.corpus)

    def query(self, needle, limit, indices=False):
        """what `Matcher.match_list_top` (indices=False) / `match_list_top_indices` (True) return for `needle`; `last_narrowed` tells
        whether the previous capture was the input"""
        n = _b(needle)
        self.matcher.set_pattern(n)
        i = self.matcher.info()
        path = (i["unicode"], i["pf_lanes"], i["sw_lanes"])
        narrow = self._may_narrow(n, path)
        src = self.subsets[self._cur] if narrow else None
        dst_i = 1 - self._cur if self._cur is not None else 0
        dst = self.subsets[dst_i]
        self._cur = self._prev = None  # (an error below leaves no capture to narrow from)
        fn = self.matcher.match_list_top_indices if indices else self.matcher.match_list_top
        res = fn(self.corpus, limit, subset=src, capture=dst)
        self._cur, self._prev, self.last_narrowed = dst_i, (bytes(n), path, self.corpus.generation()), narrow
        return res


class NarrowingQuery:
    """`NarrowingMatcher` for query syntax: a `MultiMatcher` over one resident `Corpus`, `parse_query` per keystroke, two `Subset`s that
    alternate.  Every query captures the COMPOSITION's match set; the next one runs over that capture when the rule below holds, else over
    `within` (a `Subset`, e.g. the workspace folder; None: the whole list) - a restricted picker never falls back to the full corpus.
    The rule.  P = the compiled patterns of the previous query, Q = those of the new one (empty needles dropped, as the library's compile
    does).  The capture may be the input iff len(Q) >= len(P), Q[i] refines P[i] for every i < len(P), Q != P, the config, the corpus
    generation and `within` (identity and generation) are unchanged, and the capture's count is known and at most max_fraction x len(corpus).
    Q[i] refines P[i] when (a) the two are equal field for field, negated or not - an unchanged negated pattern removes the same haystacks -
    or (b) both are non-negated, equal in every field but the needle, and the needles satisfy `NarrowingMatcher`'s condition under the
    pattern's resolved config (fuzzy, resolved max_typos == 0, the new needle = the old one + a non-empty suffix, the same unicode path and
    lane pair).  The patterns Q[len(P):] are free: a further non-negated pattern intersects, a further negated one subtracts.
    A negated pattern that changes in any way does NOT refine: `!t` -> `!te` removes fewer haystacks, the match set grows
    (tests/test_oracle_query_narrowing_premise.py finds such a step with the oracle).  The extension of a literal-mode atom (`^foo` ->
    `^foob`) is monotone too but is left out on purpose: nobody has held it to the oracle yet.
    max_fraction: None = DEFAULT_MAX_FRACTION, under `NarrowingMatcher`'s policy: 0.8 x the largest candidate fraction at which
    tools/bench_multi_subset.py measured the narrowed call not slower than the un-narrowed one.  Measured (profiles/multi_subset.txt, host
    time per keystroke): on the paths-shaped 1.4 M list every narrowed step at 6.1 % of the list and below won 86 - 93 us of ~ 417, and lost
    14 - 39 us at 45 - 90 %; on the 10 M x 32 B list the step at 4.99 % won 6 us of 453 and the steps at 5.6 - 17 % lost 6 - 22 us.  The
    largest fraction with no loss at or below it on either list is 0.0499, so the default is 0.8 x that.  (A composition pays for every
    pattern over the whole list when it does not narrow, which is why this default is not `NarrowingMatcher`'s 0.0.)  A caller who refills
    `within` in place at the same corpus generation calls `reset()`."""

    DEFAULT_MAX_FRACTION = 0.039

    def __init__(self, corpus, config=None, max_fraction=None, within=None, facets=None):
        self.corpus = corpus
        self.config = config or Config()
        self.max_fraction = self.DEFAULT_MAX_FRACTION if max_fraction is None else float(max_fraction)
        self.within = within
        self.matcher = MultiMatcher([], self.config)
        if facets is not None:  # a `Facets` sink of the corpus: every query fills it with the composition's counts
            self.matcher.set_facets(facets)
        self.subsets = [Subset(corpus), Subset(corpus)]
        self._cur = None    # index of the subset that holds the previous query's capture
        self._prev = None   # (compiled patterns, config, corpus generation, within key) of that query
        self._paths = {}
        self.last_narrowed = False

    def set_facets(self, facets):
        """pass a `Facets` sink of the corpus on to the matcher (None: detach), as `facets=` does at construction"""
        self.matcher.set_facets(facets)

    def reset(self):
        """forget the previous capture: the next query runs over `within` / the whole list"""
        self._cur = self._prev = None

    @staticmethod
    def _resolved(p, cfg):
        """the config a pattern's sub-matcher gets (src/pattern.rs:230-262: `None` fields inherit the matcher's)"""
        return Config(max_typos=cfg.max_typos if p.max_typos is None else p.max_typos, casing=cfg.casing if p.casing is None else p.casing,
                      unicode=cfg.unicode if p.unicode is None else p.unicode, sort=SortStrategy.IndexAsc, scoring=p.scoring or cfg.scoring,
                      pf_lanes=cfg.pf_lanes, sw_lanes=cfg.sw_lanes, matching=cfg.matching if p.matching is None else p.matching)

    def compile(self, patterns, cfg=None):
        """list[Pattern] -> [(Pattern with a bytes needle, resolved Config, (unicode, pf_lanes, sw_lanes))], empty needles dropped; host work"""
        cfg = cfg or self.config
        out = []
        for p in patterns:
            p = p if isinstance(p, Pattern) else Pattern(p)
            n = _b(p.needle)
            if not n:
                continue
            p = replace(p, needle=bytes(n))
            r = self._resolved(p, cfg)
            key = (p.needle, r.max_typos, int(r.casing), int(r.unicode), r.pf_lanes, r.sw_lanes, int(r.matching))
            if key not in self._paths:
                i = Matcher(p.needle, r).info()
                self._paths[key] = (i["unicode"], i["pf_lanes"], i["sw_lanes"])
            out.append((p, r, self._paths[key]))
        return out

    @staticmethod
    def refines(old, new):
        """Q[i] refines P[i] (entries of `compile`)"""
        (po, ro, patho), (pn, rn, pathn) = old, new
        if po == pn and patho == pathn:
            return True
        if po.negated or pn.negated or replace(po, needle=pn.needle) != pn:
            return False
        return _needle_extends(rn.matching, rn.max_typos, po.needle, pn.needle, patho, pathn)

    @classmethod
    def rule(cls, P, Q):
        """the pattern part of the rule over two `compile`d lists"""
        if len(Q) < len(P) or not all(cls.refines(o, n) for o, n in zip(P, Q)):
            return False
        return [e[0] for e in Q] != [e[0] for e in P]

    def _within_key(self):
        w = self.within
        return None if w is None else (id(w), w.info()["generation"])

    def _may_narrow(self, Q):
        if self._cur is None or self._prev is None:
            return False
        P, prev_cfg, prev_gen, prev_within = self._prev
        if prev_cfg != self.config or not self.rule(P, Q):
            return False
        if self.corpus.generation() != prev_gen or self._within_key() != prev_within:
            return False
        cap = self.subsets[self._cur]
        out = (C.c_uint64 * 4)()
        _check(lib().fzb_subset_info(cap.h, out))
        return self.max_fraction > 0 and bool(out[0]) and out[1] <= self.max_fraction * len(self.corpus)

    def set_config(self, config):
        self.matcher.set_config(config)
        self.config = config

    def query(self, text, limit, indices=False):
        """what `MultiMatcher.match_list_top` (indices=False) / `match_list_top_indices` (True) return for the query string `text` (or a list
        of `Pattern`s) over `within`; `last_narrowed` tells whether the previous capture was the input"""
        pats = parse_query(text) if isinstance(text, (str, bytes)) else list(text)
        Q = self.compile(pats)
        narrow = self._may_narrow(Q)
        src = self.subsets[self._cur] if narrow else self.within
        dst_i = 1 - self._cur if self._cur is not None else 0
        dst = self.subsets[dst_i]
        self._cur = self._prev = None  # (an error below leaves no capture to narrow from)
        self.matcher.set_patterns(pats)
        fn = self.matcher.match_list_top_indices if indices else self.matcher.match_list_top
        res = fn(self.corpus, limit, subset=src, capture=dst)
        self._cur, self._prev, self.last_narrowed = dst_i, (Q, deepcopy(self.config), self.corpus.generation(), self._within_key()), narrow
        return res


def radix_sort_matches(matches):
    """`radix_sort_matches(&mut [Match])` (src/sort.rs:6-40): stable, descending score. Returns a sorted copy."""
    a = np.ascontiguousarray(matches.copy())
    lib().fzb_radix_sort_matches(a.ctypes.data, len(a))
    return a


def k_merge_matches(sort, runs):
    """`k_merge_matches_by_*` (src/k_merge.rs:56-132): merge per-shard runs, each already ordered per `sort`."""
    lens = np.array([len(r) for r in runs], dtype=np.uint64)
    cat = np.ascontiguousarray(np.concatenate(runs)) if runs else np.zeros(0, MATCH_DTYPE)
    out = np.zeros(len(cat), MATCH_DTYPE)
    _check(lib().fzb_k_merge_matches(int(sort), cat.ctypes.data, lens.ctypes.data, len(runs), out.ctypes.data))
    return out
