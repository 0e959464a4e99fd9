"""superplus_amd/csrc/dfk_scons.h -- the C++ restatement of Stackster's stack consensus, the device version's order of work and the layout
of a.stack.cons -- against tests/scons_oracle.py: tests/cpp/test_scons.cc (its own main) built plain and under
-fsanitize=address,undefined and run directly, on the seeded cases recorded in tests/cpp/scons_cases.txt and on the six fixtures the walks
tests use, their walks written out in the same form (the largest, graph_pathy2_k48, in the plain build).  It checks the literal
transcription (both stacks materialised), that the device-order form (live rows, batches, ranges, a lane a column, the flat pass, the
conflicts) gives the same bytes, and the shared pieces (the rounding against std::round, top_two against a sort).  CPU only."""
import os
import subprocess

import pytest

from tests import scons_cases, scons_oracle, walks_oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUILDS = {"plain": ["-O1"], "sanitized": ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]}
N_RECORDED = len(scons_cases.seeded())
FIXTURES = (("graph_pathy_k48", 48, "pathy"), ("graph_k40_nobc", 40, "reads"), ("graph_frag_k48", 48, "frag"), ("graph_k48", 48, "reads"), ("graph_special_k48", 48, "special"))
LARGEST = ("graph_pathy2_k48", 48, "pathy2")


def test_recorded_cases_are_what_the_oracle_says_now():
    """tests/cpp/scons_cases.txt is scons_cases.text(): regenerate it (python -m tests.scons_cases) when the oracle or the generator changes"""
    assert open(scons_cases.FILE).read() == scons_cases.text()
    assert N_RECORDED == 3 and os.path.getsize(scons_cases.FILE) < 200000


def fixture_case(golden_dir, case, K, which):
    """a fixture's walks and reads in the form of a seeded case"""
    i = walks_oracle.fixture_inputs(golden_dir, case, K, which)
    rs = i["rs"]
    return dict(recs=walks_oracle.fixture_walks(golden_dir, case, K, which)["recs"], reads=[i["read_bases"](id) for id in range(int(rs["n_reads"]))], pq=rs["pq_bytes"], pq_off=rs["pq_off"], K=K)


def fixture_text(golden_dir, case, K, which):
    return scons_cases.case_text(case, fixture_case(golden_dir, case, K, which), scons_oracle.fixture_scons(golden_dir, case, K, which))


@pytest.fixture(scope="module")
def more_cases(golden_dir, tmp_path_factory):
    """five fixtures in the form of scons_cases.txt; the largest fixture in a file of its own"""
    out = []
    for case, K, which in FIXTURES: out += fixture_text(golden_dir, case, K, which)
    d = tmp_path_factory.mktemp("scons")
    (d / "more_cases.txt").write_text("\n".join(out) + "\n")
    (d / "largest.txt").write_text("\n".join(fixture_text(golden_dir, *LARGEST)) + "\n")
    return str(d / "more_cases.txt"), str(d / "largest.txt")


@pytest.mark.parametrize("build", list(BUILDS))
def test_cpp_restatement_agrees_with_the_oracle(tmp_path, more_cases, build):
    exe = os.path.join(tmp_path, "test_scons")
    subprocess.check_call(["g++", *BUILDS[build], "-std=c++17", "-Wall", "-I", os.path.join(ROOT, "superplus_amd", "csrc"), "-o", exe,
                           os.path.join(ROOT, "tests", "cpp", "test_scons.cc")])
    runs = [(scons_cases.FILE, N_RECORDED), (more_cases[0], len(FIXTURES))]
    if build == "plain": runs.append((more_cases[1], 1))                        # (graph_pathy2_k48: long under the sanitizers)
    for cases, n in runs:
        out = subprocess.run([exe, cases], capture_output=True, text=True, timeout=900)
        assert out.returncode == 0, out.stdout + out.stderr
        assert f"{n} recorded cases agree" in out.stdout
