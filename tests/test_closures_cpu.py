"""superplus_amd/csrc/dfk_closures.h -- the C++ restatement of CloseGap2's closures (Merge and Consensus1 with qualities on the two stacks
of a pair), the plan of its device version and the layout of a.close.closures -- against tests/closures_oracle.py:
tests/cpp/test_closures.cc (its own main) built plain and under -fsanitize=address,undefined and run directly, on the seeded cases
recorded in tests/cpp/closures_cases.txt, on the larger seeded cases and on graph_pathy2_k48 and graph_frag_k48 written out in the same
form.  It checks the literal transcription (both stacks materialised, merged by resize / shift / append), and that the device-order form
gives the same bytes under closures_per_batch 1, 37 and 2^30 and under small ranges.  CPU only."""
import os
import subprocess

import pytest

from tests import closer_oracle, closures_cases, closures_oracle, partners_oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUILDS = {"plain": ["-O1"], "sanitized": ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]}
N_RECORDED = sum(1 for _, _, rec in closures_cases.seeded() if rec)
N_LARGER = sum(1 for _, _, rec in closures_cases.seeded() if not rec)


def test_recorded_cases_are_what_the_oracle_says_now():
    """tests/cpp/closures_cases.txt is closures_cases.text(): regenerate it (python -m tests.closures_cases) when the oracle or the generator
    changes"""
    assert open(closures_cases.FILE).read() == closures_cases.text()
    assert N_RECORDED == 5 and N_LARGER == 2 and os.path.getsize(closures_cases.FILE) < 100000


@pytest.fixture(scope="module")
def more_cases(golden_dir, tmp_path_factory):
    """the larger seeded cases, and pathy2 and frag in the form of closures_cases.txt"""
    out = closures_cases.text(recorded=False).splitlines()
    for case, K, which in (("graph_pathy2_k48", 48, "pathy2"), ("graph_frag_k48", 48, "frag")):
        i = partners_oracle.fixture_inputs(golden_dir, case, K, which)
        p = partners_oracle.fixture_partners(golden_dir, case, K, which)
        r = closures_oracle.fixture_closures(golden_dir, case, K, which)
        rs = i["rs"]
        n = int(rs["n_reads"])
        c = dict(inv=i["inv"], kmers=closer_oracle.fixture_inputs(golden_dir, case, K, which)["kmers"], ce=i["ce"], locs=i["locs_per"], parts=p["elements"], pairs=i["pairs"],
                 reads=[i["read_bases"](id) for id in range(n)], pq=rs["pq_bytes"], pq_off=rs["pq_off"], offsets=r["offsets_per"])
        out += closures_cases.case_text(case, c, r, K)
    path = tmp_path_factory.mktemp("closures") / "more_cases.txt"
    path.write_text("\n".join(out) + "\n")
    return str(path)


@pytest.mark.parametrize("build", list(BUILDS))
def test_cpp_restatement_agrees_with_the_oracle(tmp_path, more_cases, build):
    exe = os.path.join(tmp_path, "test_closures")
    subprocess.check_call(["g++", *BUILDS[build], "-std=c++17", "-Wall", "-I", os.path.join(ROOT, "superplus_amd", "csrc"), "-o", exe,
                           os.path.join(ROOT, "tests", "cpp", "test_closures.cc")])
    for cases, n in ((closures_cases.FILE, N_RECORDED), (more_cases, N_LARGER + 2)):
        out = subprocess.run([exe, cases], capture_output=True, text=True, timeout=900)
        assert out.returncode == 0, out.stdout + out.stderr
        assert f"{n} recorded cases agree" in out.stdout
