"""superplus_amd/csrc/dfk_hops.h -- the C++ restatement of FindEdgePairs that the kernel k_hops_edges and the host's exact route
both run -- against tests/hops_oracle.py: tests/cpp/test_hops.cc (its own main) built plain and under
-fsanitize=address,undefined, run on its cases worked out by hand, on the six seeded graphs recorded in tests/cpp/hops_cases.txt and
on two fixtures written out in the same form.  CPU only."""
import os
import subprocess

import pytest

from tests import hops_cases
from tests.test_hops_oracle import fixture_inputs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUILDS = {"plain": ["-O1"], "sanitized": ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]}


def test_recorded_cases_are_what_the_oracle_says_now():
    """tests/cpp/hops_cases.txt is hops_cases.text(): regenerate it (python -m tests.hops_cases) when the oracle or the generator changes"""
    assert open(hops_cases.FILE).read() == hops_cases.text()
    lines = open(hops_cases.FILE).read().split("\n")
    assert sum(l.startswith("graph ") for l in lines) == 6 and len(lines) < 4000      # six seeded graphs, each written once
    idx = [k for k, l in enumerate(lines) if l.startswith("variant ")]
    assert len(idx) == 24 and {lines[k].split()[1] for k in idx} == {"0", "1"}       # 24 recorded cases: ONE_GOOD both ways, the capacities
    # the cases are not empty: pairs of every method, searches that overflow some capacities and not others
    n_of = lambda k, j: int(lines[k + 1 + j].split()[0])
    assert all(sum(n_of(k, j) for k in idx) > 0 for j in range(4))
    host = [int(lines[k + 5].split()[6]) for k in idx]
    assert any(h == 0 for h in host) and any(h > 0 for h in host)


@pytest.fixture(scope="module")
def fixture_cases(golden_dir, tmp_path_factory):
    """pathy2 (a 7-round search, 160 double crossings, 62 pairs of method 2) and frag in the form of hops_cases.txt: default capacities,
    one slot (every searched edge overflows), and a middle value at which some do"""
    out = []
    for case, which, caps in (("graph_pathy2_k48", "pathy2", [(96, 24), (1, 24), (19, 24)]), ("graph_frag_k48", "frag", [(96, 24), (6, 3)])):
        i = fixture_inputs(golden_dir, case, 48, which)
        c = dict(i, n_vertices=int(max(i["to_left"].max(), i["to_right"].max())) + 1)
        out += hops_cases.case_text(case, c, 48, caps)
    path = tmp_path_factory.mktemp("hops") / "fixture_cases.txt"
    path.write_text("\n".join(out) + "\n")
    return str(path)


@pytest.mark.parametrize("build", list(BUILDS))
def test_cpp_restatement_agrees_with_the_oracle(tmp_path, fixture_cases, build):
    exe = os.path.join(tmp_path, "test_hops")
    subprocess.check_call(["g++", *BUILDS[build], "-std=c++17", "-Wall", "-I", os.path.join(ROOT, "superplus_amd", "csrc"), "-o", exe,
                           os.path.join(ROOT, "tests", "cpp", "test_hops.cc")])
    for cases, n in ((hops_cases.FILE, 24), (fixture_cases, 10)):
        out = subprocess.run([exe, cases], capture_output=True, text=True, timeout=600)
        assert out.returncode == 0, out.stdout + out.stderr
        assert f"the hand cases and {n} recorded cases agree" in out.stdout
