"""The empty prompt's device forms (fzb_prompt_list_device / fzb_prompt_top_device) and its producer, without a GPU: the two calls are
declared, listed and mirrored, bad arguments and a matcher with a needle are refused before anything touches a device, the header says what
now happens to an empty needle, the producer's header is a HIP-free build dependency and its kernels are part of the library."""
import ctypes as C
import os
import re

import frizbee_amd as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FZB_ERR_INVALID = 1
NEW = ("fzb_prompt_list_device", "fzb_prompt_top_device")


def read(*parts):
    return open(os.path.join(ROOT, *parts)).read()


def flat(text):
    return " ".join(text.replace("*", " ").split())


def test_symbols_are_declared_listed_and_mirrored():
    header = flat(read("include", "frizbee_hip.h"))
    assert ("int fzb_prompt_list_device(fzb_matcher m, const fzb_corpus c, const fzb_subset in, size_t first, size_t count, uint32_t index_offset, fzb_match dev_out, "
            "size_t capacity, uint32_t dev_count, void stream);") in header
    assert ("int fzb_prompt_top_device(fzb_matcher m, const fzb_corpus c, const fzb_subset in, size_t limit, fzb_match dev_out, size_t capacity, uint32_t dev_count, "
            "void stream);") in header
    # beside the _device forms they complete: behind the subset queries, ahead of the multi-pattern family
    raw = read("include", "frizbee_hip.h")
    assert raw.index("int fzb_match_list_top_indices_subset(") < raw.index("int fzb_prompt_list_device(") < raw.index("int fzb_prompt_top_device(") < raw.index("typedef struct fzb_pattern")
    for name in NEW:
        assert name in F.SYMBOLS
        assert getattr(F.lib(), name).argtypes is not None
    assert len(F.lib().fzb_prompt_list_device.argtypes) == 10 and len(F.lib().fzb_prompt_top_device.argtypes) == 8
    assert callable(F.Matcher.prompt_list_device) and callable(F.Matcher.prompt_top_device)
    hpp, rust = read("include", "frizbee_hip.hpp"), read("rust", "src", "hip.rs")
    for name in NEW:
        assert name + "(" in hpp and "fn " + name + "(" in rust
    assert "void prompt_list_device(" in hpp and "void prompt_top_device(" in hpp
    assert "pub unsafe fn prompt_list_device(" in rust and "pub unsafe fn prompt_top_device(" in rust


def test_bad_arguments_and_a_needle_are_refused_before_any_device_is_touched():
    l = F.lib()
    null, fake = C.c_void_p(None), C.c_void_p(64)  # fake: never dereferenced - the argument checks come first
    for call in (lambda m, c, out, cap, cnt: l.fzb_prompt_list_device(m, c, None, 0, 0, 0, out, cap, cnt, None),
                 lambda m, c, out, cap, cnt: l.fzb_prompt_top_device(m, c, None, 5, out, cap, cnt, None)):
        assert call(null, fake, fake, 8, fake) == FZB_ERR_INVALID
        assert call(fake, null, fake, 8, fake) == FZB_ERR_INVALID
        assert call(fake, fake, fake, 8, null) == FZB_ERR_INVALID
        assert call(fake, fake, null, 8, fake) == FZB_ERR_INVALID
        assert b"null" in l.fzb_last_error()
        m = F.Matcher("abc", F.Config(pf_lanes=64))  # compiled on the host: no device yet
        assert call(m.h, fake, fake, 8, fake) == FZB_ERR_INVALID  # the corpus is not looked at before the needle is
        msg = l.fzb_last_error()
        assert b"needle" in msg and b"not empty" in msg, msg


def test_the_header_says_what_happens_to_an_empty_needle():
    header = read("include", "frizbee_hip.h")
    bias = flat(header[header.index("A PER-HAYSTACK SCORE BIAS"):header.index("int fzb_corpus_set_bias(")])
    assert "AN EMPTY NEEDLE / NO PATTERN over a biased corpus" in bias and "The _device forms keep refusing an empty needle" in bias
    assert "runs on the device" in bias and "no column crosses the link" in bias and "fzb_prompt_top_device" in bias
    assert "one copy of the bias and the host's stable sort" not in bias
    scope = flat(header[header.index("PER-HAYSTACK TAGS AND A VISIBILITY SCOPE"):header.index("int fzb_corpus_set_tags(")])
    assert "one copy of the tags" not in scope and "flag pass over the tags" in scope and "fzb_prompt_list_device" in scope
    subset = flat(header[header.index("CANDIDATE SETS"):header.index("int fzb_match_list_top_indices_subset(")])
    assert "An EMPTY NEEDLE" in subset and "the set never crosses the link" in subset and "fzb_prompt_top_device takes a subset" in subset
    own = flat(header[header.index("THE EMPTY PROMPT on the device"):header.index("int fzb_prompt_top_device(")])
    for phrase in ("m must have an empty needle", "`in` may be NULL", "first == 0", "stale or foreign", "nothing synchronises", "zeroes the pair", "FZB_ERR_CAPACITY, nothing launched",
                   "every index, score 0", "clamp(bias[i], 0, 65535)", "only over a biased corpus", "dev_count[1] = found"):
        assert phrase.lower() in own.lower(), phrase
    design = read("DESIGN.md")
    assert "The empty prompt" in design and "k_prompt_records" in design and "k_prompt_compact" in design
    assert "k_prompt_records" in read("README.md") or "fzb_prompt_top_device" in read("README.md")
    assert "fzb_prompt_top_device" in read("INTEGRATION.md")
    assert "empty_prompt.txt" in read("profiles", "README.md")


def test_the_producer_is_part_of_the_build_and_its_rule_is_hip_free():
    mk = read("frizbee_amd", "csrc", "Makefile")
    assert "kernels_prompt.o" in mk and "prompt_records.h" in mk
    rule = read("frizbee_amd", "csrc", "prompt_records.h")
    assert "FZB_PROMPT_FN" in rule and "hipStream_t" not in rule and "#include <hip" not in rule
    assert '#include "scope.h"' in rule and '#include "score_bias.h"' in rule and "scope_visible(" in rule and "sbias_clamp_add(" in rule
    kernels = read("frizbee_amd", "csrc", "kernels_prompt.hip")
    assert '#include "prompt_records.h"' in kernels
    for k in ("k_prompt_records", "k_prompt_flag", "k_prompt_compact"):
        assert re.search(r"FZB_LAUNCH\(%s, " % k, kernels), k
    assert "tc_flag_pass(" in kernels and "tc_compact_items(" in kernels and "asm" not in kernels and "__shared__" not in kernels
    host = read("frizbee_amd", "csrc", "host.hip")
    assert "fzb_launch_prompt_records(" in host and "fzb_launch_prompt_compact(" in host
    assert "sbias_one_pass(0, fzb_corpus_bias_hi(c))" in host  # the prompt has no matrix score: one_pass from bias_hi alone


def test_the_library_exports_the_two_calls():
    for name in NEW:
        assert getattr(F.lib(), name) is not None
