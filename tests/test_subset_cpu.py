"""superplus_amd/csrc/dfk_subset.h -- the C++ restatement of the subset of interest, the plan of its device version and the layouts of the
four files a.sub.* -- against tests/subset_oracle.py: tests/cpp/test_subset.cc (its own main) built plain and under
-fsanitize=address,undefined, run on the graph worked out by hand, on the seeded cases recorded in tests/cpp/subset_cases.txt and on two
fixtures written out in the same form.  CPU only."""
import os
import subprocess

import pytest

from tests import subset_cases
from tests.test_hops_oracle import fixture_hops, fixture_inputs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUILDS = {"plain": ["-O1"], "sanitized": ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]}
N_RECORDED = sum(1 for _, _, rec in subset_cases.seeded() if rec)


def test_recorded_cases_are_what_the_oracle_says_now():
    """tests/cpp/subset_cases.txt is subset_cases.text(): regenerate it (python -m tests.subset_cases) when the oracle or the generator changes"""
    assert open(subset_cases.FILE).read() == subset_cases.text()
    assert N_RECORDED == 8 and os.path.getsize(subset_cases.FILE) < 20000


@pytest.fixture(scope="module")
def fixture_cases(golden_dir, tmp_path_factory):
    """frag and graph_k40_nobc (the fixture whose reads cross an edge of interest twice) in the form of subset_cases.txt"""
    out = []
    for case, K, which in (("graph_frag_k48", 48, "frag"), ("graph_k40_nobc", 40, "reads")):
        i = fixture_inputs(golden_dir, case, K, which)
        out += subset_cases.case_text(case, dict(inv=[int(x) for x in i["inv"]], paths=i["paths"], pairs=fixture_hops(golden_dir, case, K, which)["pairs"]))
    path = tmp_path_factory.mktemp("subset") / "fixture_cases.txt"
    path.write_text("\n".join(out) + "\n")
    return str(path)


@pytest.mark.parametrize("build", list(BUILDS))
def test_cpp_restatement_agrees_with_the_oracle(tmp_path, fixture_cases, build):
    exe = os.path.join(tmp_path, "test_subset")
    subprocess.check_call(["g++", *BUILDS[build], "-std=c++17", "-Wall", "-I", os.path.join(ROOT, "superplus_amd", "csrc"), "-o", exe,
                           os.path.join(ROOT, "tests", "cpp", "test_subset.cc")])
    for cases, n in ((subset_cases.FILE, N_RECORDED), (fixture_cases, 2)):
        out = subprocess.run([exe, cases], capture_output=True, text=True, timeout=300)
        assert out.returncode == 0, out.stdout + out.stderr
        assert f"the hand case and {n} recorded cases agree" in out.stdout
