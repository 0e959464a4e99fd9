"""superplus_amd/csrc/dfk_soffsets.h -- the C++ restatement of Stackster's stack offsets, the device version's order of work and the layout
of a.stack.offsets -- against tests/soffsets_oracle.py: tests/cpp/test_soffsets.cc (its own main) built plain and under
-fsanitize=address,undefined and run directly, on the seeded cases recorded in tests/cpp/soffsets_cases.txt and on the six fixtures the
walks tests use, written out in the same form (the largest, graph_pathy2_k48, in the plain build).  It checks the literal transcription
(both stacks as grids, a std::set, ReverseSort and the filter loop), that the device-order form (masks, prefix sums, the maximum per
offset and kept( best, score ), batches of 1, 37 and everything, ranges) gives the same bytes, and the shared pieces (acceptable, minp
over masked windows, kept) against the loops as written.  CPU only."""
import os
import subprocess

import pytest

from tests import scons_cases, scons_oracle, soffsets_cases, soffsets_oracle
from tests.test_scons_cpu import fixture_case

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUILDS = {"plain": ["-O1"], "sanitized": ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]}
N_RECORDED = len(soffsets_cases.seeded())
FIXTURES = (("graph_pathy_k48", 48, "pathy"), ("graph_k40_nobc", 40, "reads"), ("graph_frag_k48", 48, "frag"), ("graph_k48", 48, "reads"), ("graph_special_k48", 48, "special"))
LARGEST = ("graph_pathy2_k48", 48, "pathy2")


def test_recorded_cases_are_what_the_oracle_says_now():
    """tests/cpp/soffsets_cases.txt is soffsets_cases.text(): regenerate it (python -m tests.soffsets_cases) when an oracle or the generator
    changes"""
    assert open(soffsets_cases.FILE).read() == soffsets_cases.text()
    assert N_RECORDED == 3 and os.path.getsize(soffsets_cases.FILE) < 400000


def fixture_text(golden_dir, case, K, which):
    return (scons_cases.case_text(case, fixture_case(golden_dir, case, K, which), scons_oracle.fixture_scons(golden_dir, case, K, which)) +
            soffsets_cases.result_text(soffsets_oracle.fixture_soffsets(golden_dir, case, K, which)))


@pytest.fixture(scope="module")
def more_cases(golden_dir, tmp_path_factory):
    """five fixtures in the form of soffsets_cases.txt; the largest fixture in a file of its own"""
    out = []
    for case, K, which in FIXTURES: out += fixture_text(golden_dir, case, K, which)
    d = tmp_path_factory.mktemp("soffsets")
    (d / "more_cases.txt").write_text("\n".join(out) + "\n")
    (d / "largest.txt").write_text("\n".join(fixture_text(golden_dir, *LARGEST)) + "\n")
    return str(d / "more_cases.txt"), str(d / "largest.txt")


@pytest.mark.parametrize("build", list(BUILDS))
def test_cpp_restatement_agrees_with_the_oracle(tmp_path, more_cases, build):
    exe = os.path.join(tmp_path, "test_soffsets")
    subprocess.check_call(["g++", *BUILDS[build], "-std=c++17", "-Wall", "-I", os.path.join(ROOT, "superplus_amd", "csrc"), "-o", exe,
                           os.path.join(ROOT, "tests", "cpp", "test_soffsets.cc")])
    runs = [(soffsets_cases.FILE, N_RECORDED), (more_cases[0], len(FIXTURES))]
    if build == "plain": runs.append((more_cases[1], 1))                        # (graph_pathy2_k48: long under the sanitizers)
    for cases, n in runs:
        out = subprocess.run([exe, cases], capture_output=True, text=True, timeout=1800)
        assert out.returncode == 0, out.stdout + out.stderr
        assert f"{n} recorded cases agree" in out.stdout
