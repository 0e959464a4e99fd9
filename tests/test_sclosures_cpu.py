"""superplus_amd/csrc/dfk_sclosures.h -- the C++ restatement of Stackster's closures, the device version's order of work and the layout of
a.stack.closures -- against tests/sclosures_oracle.py: tests/cpp/test_sclosures.cc (its own main) built plain and under
-fsanitize=address,undefined and run directly, on the seeded cases recorded in tests/cpp/sclosures_cases.txt and on the six fixtures the
walks tests use, written out in the same form (the largest, graph_pathy2_k48, in the plain build).  It checks the literal transcription
(both stacks as grids, Trim, Merge and Consensus1 as written), that the device-order form (the closable pairs alone, batches of 1, 37 and
everything, three row caps, the rows a tile skips, the flags counted) gives the same bytes, and merged_cols() / column_of_side() against
the literal Trim + Merge for every allowed offset of several width pairs.  Nothing is loaded into python under a sanitizer.  CPU only."""
import os
import subprocess

import pytest

from tests import sclosures_cases, sclosures_oracle, scons_oracle, soffsets_oracle
from tests.test_scons_cpu import fixture_case

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUILDS = {"plain": ["-O1"], "sanitized": ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]}
N_RECORDED = len(sclosures_cases.seeded())
FIXTURES = (("graph_pathy_k48", 48, "pathy"), ("graph_k40_nobc", 40, "reads"), ("graph_frag_k48", 48, "frag"), ("graph_k48", 48, "reads"), ("graph_special_k48", 48, "special"))
LARGEST = ("graph_pathy2_k48", 48, "pathy2")


def test_recorded_cases_are_what_the_oracle_says_now():
    """tests/cpp/sclosures_cases.txt is sclosures_cases.text(): regenerate it (python -m tests.sclosures_cases) when an oracle or the
    generator changes"""
    assert open(sclosures_cases.FILE).read() == sclosures_cases.text()
    assert N_RECORDED == 4 and os.path.getsize(sclosures_cases.FILE) < 400000


def fixture_text(golden_dir, case, K, which):
    c = dict(fixture_case(golden_dir, case, K, which), so_per=soffsets_oracle.fixture_soffsets(golden_dir, case, K, which)["per"], K=K)
    return sclosures_cases.case_text(case, c, scons_oracle.fixture_scons(golden_dir, case, K, which), sclosures_oracle.fixture_sclosures(golden_dir, case, K, which))


@pytest.fixture(scope="module")
def more_cases(golden_dir, tmp_path_factory):
    """five fixtures in the form of sclosures_cases.txt; the largest fixture in a file of its own"""
    out = []
    for case, K, which in FIXTURES: out += fixture_text(golden_dir, case, K, which)
    d = tmp_path_factory.mktemp("sclosures")
    (d / "more_cases.txt").write_text("\n".join(out) + "\n")
    (d / "largest.txt").write_text("\n".join(fixture_text(golden_dir, *LARGEST)) + "\n")
    return str(d / "more_cases.txt"), str(d / "largest.txt")


@pytest.mark.parametrize("build", list(BUILDS))
def test_cpp_restatement_agrees_with_the_oracle(tmp_path, more_cases, build):
    exe = os.path.join(tmp_path, "test_sclosures")
    subprocess.check_call(["g++", *BUILDS[build], "-std=c++17", "-Wall", "-I", os.path.join(ROOT, "superplus_amd", "csrc"), "-o", exe,
                           os.path.join(ROOT, "tests", "cpp", "test_sclosures.cc")])
    runs = [(sclosures_cases.FILE, N_RECORDED), (more_cases[0], len(FIXTURES))]
    if build == "plain": runs.append((more_cases[1], 1))                        # (graph_pathy2_k48: long under the sanitizers)
    for cases, n in runs:
        out = subprocess.run([exe, cases], capture_output=True, text=True, timeout=1800)
        assert out.returncode == 0, out.stdout + out.stderr
        assert f"{n} recorded cases agree" in out.stdout
