"""The "behave as on a device of n compute units" switch (FZB_DEBUG_CUS, knobs.h) and the record of the grids launched under it
(fzb_debug_launch_grids), without a GPU: the switch and the hook are declared and documented, the device's compute-unit count is read in
ONE function, every launch of the library goes through the recording macro, no launch of host_upload.hip takes a grid capped by a bare
literal, and the override is off by default."""
import ctypes as C
import os
import re

import frizbee_amd as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "frizbee_amd", "csrc")
FZB_ERR_INVALID, FZB_ERR_CAPACITY = 1, 3

# launches of host_upload.hip whose grid is NOT a per-CU cap: the grid is the structure of the pass, not a number of resident workgroups
STRUCTURAL = {
    "k_up_tiles": "one workgroup per 1024-haystack tile: it writes that tile's sum and figures",
    "k_up_build": "one workgroup per tile: it places the tile at the offset the scan gave it",
    "k_up_view_sort": "one workgroup per tile of the view: the tile's sort lives in its LDS",
    "k_up_view_fill": "one workgroup per tile of the view: it fills the blocks k_up_view_sort laid out",
    "k_up_scan": "a single workgroup: a running carry over chunks of 1024 tiles",
    "k_up_vlong_prune": "a single workgroup: an in-place compaction with a running carry",
    "k_col_compact": "one workgroup per source tile of the edit pass: the tile's prefix comes from the pass' counts",
    "k_ed_tiles": "one workgroup per source tile of the edit pass",
    "k_ed_scan": "a single workgroup: a running carry over chunks of 1024 tiles",
    "k_ed_gather": "one workgroup per source tile of the chunk: it gathers into the slot the scan gave the tile",
}


def read(*parts):
    return open(os.path.join(ROOT, *parts)).read()


def sources():
    return {f: read("frizbee_amd", "csrc", f) for f in sorted(os.listdir(CSRC)) if f.endswith((".hip", ".h", ".inc"))}


def test_the_switch_and_the_hook_are_declared_listed_and_documented():
    knobs = read("frizbee_amd", "csrc", "knobs.h")
    assert re.search(r"int debug_cus = 0;\s*// FZB_DEBUG_CUS=n", knobs)
    assert "int fzb_effective_cus(int* out);" in knobs and "#define FZB_LAUNCH(" in knobs
    host = read("frizbee_amd", "csrc", "host.hip")
    assert 'num("FZB_DEBUG_CUS", 0)' in host  # parsed with the other switches, so fzb_debug_reload_knobs() re-reads it
    header = " ".join(read("include", "frizbee_hip.h").split())
    assert "int fzb_debug_launch_grids(char* out, size_t cap, size_t* out_len, int clear);" in header
    assert "FZB_DEBUG_CUS" in header and "name min_grid max_grid launches" in header
    assert "fzb_debug_launch_grids" in F.SYMBOLS and F.lib().fzb_debug_launch_grids.argtypes is not None
    assert "void fzb_debug_set_filter_grid(int grid);" in header  # the older, narrower hook stays
    assert callable(F.launch_grids)
    design, readme = read("DESIGN.md"), read("README.md")
    for text in (design, readme):
        assert "FZB_DEBUG_CUS" in text and "fzb_debug_launch_grids" in text
    assert "Small-device parity" in design and "families not reached" in design.lower()


def test_the_compute_unit_count_is_read_in_one_function():
    hits = {f: s.count("multiProcessorCount") for f, s in sources().items() if "multiProcessorCount" in s}
    assert list(hits) == ["host.hip"], hits
    host = read("frizbee_amd", "csrc", "host.hip")
    begin = host.index("int fzb_effective_cus(int* out) {")
    body = host[begin:host.index("\n}\n", begin)]
    assert body.count("multiProcessorCount") == hits["host.hip"] >= 1
    assert "fzb_knobs().debug_cus" in body
    assert "return (int)e;" in body  # a device that cannot be asked is an error, not a guess
    # the two places that used to ask the device, and still report its error
    assert "HIPCHK((hipError_t)fzb_effective_cus(&cus));" in host and "HIPCHK((hipError_t)fzb_effective_cus(&mm->num_cus));" in host


def test_every_launch_goes_through_the_recording_macro():
    for f, s in sources().items():
        if f == "knobs.h":
            assert s.count("hipLaunchKernelGGL(") == 1  # the macro's own
            continue
        assert "hipLaunchKernelGGL" not in s and "<<<" not in s, f
    knobs = read("frizbee_amd", "csrc", "knobs.h")
    macro = knobs[knobs.index("#define FZB_LAUNCH("):]
    assert "if (g_fzb_record_grids) fzb_record_grid(#kernel, fzb_grid_.x);" in macro  # one predictable branch when the switch is unset
    host = read("frizbee_amd", "csrc", "host.hip")
    assert "g_fzb_record_grids = knobs_storage().debug_cus > 0;" in host  # recorded while the override is set, and only then


def test_no_host_call_hands_a_launcher_a_bare_literal_as_its_grid():
    """the launchers take their grid right before the stream: a number there is a grid that does not follow the compute-unit count"""
    for f in ("host.hip", "host_shard.hip", "host_rccl.hip", "host_upload.hip"):
        src = read("frizbee_amd", "csrc", f)
        bad = re.findall(r"fzb_launch_[a-z_0-9]+\([^;]*, \d+u?, (?:nullptr|st|stream|\(hipStream_t\)stream|[a-z]+\.st|[a-z>-]*aux_stream)\)", src)
        assert not bad, (f, bad)
    host = read("frizbee_amd", "csrc", "host.hip")
    assert host.count("count_dev, (int)fzb_grid_cap(~0ull, 2), nullptr);") == 2  # fzb_subset_from_scope and the capture of a whole list


def launches(src):
    """(kernel name, grid expression) of every FZB_LAUNCH in a source text"""
    out = []
    for m in re.finditer(r"FZB_LAUNCH\(\(?([A-Za-z_0-9]+)(?:<[^>]*>)?\)?,\s*dim3\(", src):
        depth, k = 1, m.end()
        while depth:
            depth += {"(": 1, ")": -1}.get(src[k], 0)
            k += 1
        out.append((m.group(1), src[m.end():k - 1]))
    return out


def test_no_upload_launch_takes_a_grid_capped_by_a_bare_literal():
    src = read("frizbee_amd", "csrc", "host_upload.hip")
    found = launches(src)
    assert len(found) == src.count("FZB_LAUNCH(") >= 20
    capped, structural = set(), set()
    for kernel, grid in found:
        if kernel in STRUCTURAL:
            assert re.fullmatch(r"1|\(unsigned\)\(?(up_tiles\(n\)|tiles_r|tiles|te - ta)\)?", grid), (kernel, grid)
            structural.add(kernel)
            continue
        assert re.fullmatch(r"[a-z_]*grid", grid), (kernel, grid)  # a named grid ...
        defs = re.findall(r"const unsigned %s = ([^;]*);" % grid, src)
        assert defs, (kernel, grid)
        for d in defs:                                            # ... that is a per-CU cap
            assert re.fullmatch(r"fzb_grid_cap\(.*, \d+\)", d), (kernel, grid, d)
        capped.add(kernel)
    assert structural == set(STRUCTURAL), sorted(set(STRUCTURAL) - structural)
    assert capped == {"k_up_measure", "k_sig_build", "k_col_scatter", "k_ed_mark", "k_ed_place"}, sorted(capped)
    # the caps are today's constants on 256 compute units
    caps = sorted(int(k) * 256 for k in re.findall(r"fzb_grid_cap\([^;]*, (\d+)\);", src))
    assert caps == [1024, 2048, 2048, 4096, 8192], caps
    assert not re.search(r"grid = [^;]*std::min<u64>\([^;]*, \d+\)", src)


def test_the_override_is_off_by_default_and_the_record_is_empty_without_it():
    assert "FZB_DEBUG_CUS" not in os.environ
    l = F.lib()
    n = C.c_size_t(99)
    assert l.fzb_debug_launch_grids(None, 0, C.byref(n), 0) == 0 and n.value == 0
    buf = C.create_string_buffer(4)
    assert l.fzb_debug_launch_grids(buf, 4, C.byref(n), 1) == 0 and buf.value == b"" and n.value == 0
    assert F.launch_grids() == {}
    assert l.fzb_debug_launch_grids(buf, 4, None, 0) == FZB_ERR_INVALID
    assert l.fzb_debug_launch_grids(None, 4, C.byref(n), 0) == FZB_ERR_INVALID
    assert b"null" in l.fzb_last_error()
    try:  # set and re-read: still nothing to record without a launch, and unset again it is off
        os.environ["FZB_DEBUG_CUS"] = "2"
        l.fzb_debug_reload_knobs()
        assert F.launch_grids() == {}
    finally:
        os.environ.pop("FZB_DEBUG_CUS", None)
        l.fzb_debug_reload_knobs()
    assert F.launch_grids() == {}
