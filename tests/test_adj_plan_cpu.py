"""The plan of the adjacency stage's boundary k-mer set (superplus_amd/csrc/dfk_adj_plan.h) is host arithmetic over counts
and the arena's free list: it runs here, on a CPU."""
import os
import subprocess

import pytest


@pytest.mark.parametrize("flags", [["-O1"], ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]], ids=["plain", "sanitized"])
def test_cpp_adj_plan(tmp_path, flags):
    """tests/cpp/test_adj_plan.cc: the set's slot count over 10^4 seeded random cases (never more than the block it names,
    never load > 0.6, never more than the power of two it had before, 0 exactly when no block reaches load 0.6), the
    estimate of the run's keys and the load test on hand-made part tables, one step of the default benchmark replayed in
    arenas of 180 and 186.4 GB up to the start of the last count (where the plan must give a set), and the slot walk for slot
    counts that are no power of two.  A stand-alone program, also under the sanitizers."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / "test_adj_plan")
    subprocess.check_call(["g++", *flags, "-std=c++17", "-Wall", "-o", exe, os.path.join(root, "tests", "cpp", "test_adj_plan.cc")])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "FAILED" not in out.stdout and out.stdout.count(": ok") == 5, out.stdout + out.stderr
