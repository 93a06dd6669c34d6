"""The multi-pattern matcher through the C++ host side (tests/cpp/test_facade_multi.cpp): from_query -> set_patterns -> the sharded
match_list_parallel equals match_list and does not throw."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "tests", "cpp", "test_facade_multi")


def build():
    src = EXE + ".cpp"
    hdrs = [os.path.join(ROOT, "include", h) for h in ("frizbee_hip.hpp", "frizbee_hip.h")]
    lib = os.path.join(ROOT, "frizbee_amd", "libfrizbee_hip.so")
    if not os.path.exists(EXE) or any(os.path.getmtime(f) > os.path.getmtime(EXE) for f in [src, lib] + hdrs):
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"), src, "-o", EXE, "-L", os.path.join(ROOT, "frizbee_amd"),
                               "-lfrizbee_hip", "-Wl,-rpath," + os.path.join(ROOT, "frizbee_amd")])
    return EXE


@pytest.mark.gpu
def test_multi_pattern_requery_and_sharded_parallel_through_the_cpp_facade():
    r = subprocess.run([build()], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "test_facade_multi: ok" in r.stdout, r.stdout + r.stderr
