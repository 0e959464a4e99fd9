"""superplus_amd/csrc/dfk_walks.h -- the C++ restatement of Stackster's stack walks, the device version's order of work and the layout of
a.stack.walks -- against tests/walks_oracle.py: tests/cpp/test_walks.cc (its own main) built plain, under -fsanitize=address,undefined,
and with the hash cut to 8 bits, and run directly, on the seeded cases recorded in tests/cpp/walks_cases.txt, on the larger seeded case
and on the six fixtures that have pairs written out in the same form (the largest, graph_pathy2_k48, in the plain build).  It checks the literal transcription (the sorted
triple table materialised), and that the device-order form (hash search with verification, live list, batches, ranges, host route) gives
the same bytes.  CPU only."""
import os
import subprocess

import pytest

from tests import walks_cases, walks_oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUILDS = {"plain": ["-O1"], "sanitized": ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"], "hash8": ["-O1", "-DDFK_WALK_HASH_BITS=8"]}
N_RECORDED = sum(1 for _, _, rec in walks_cases.seeded() if rec)
N_LARGER = sum(1 for _, _, rec in walks_cases.seeded() if not rec)
FIXTURES = (("graph_pathy_k48", 48, "pathy"), ("graph_k40_nobc", 40, "reads"), ("graph_frag_k48", 48, "frag"), ("graph_k48", 48, "reads"), ("graph_special_k48", 48, "special"))
LARGEST = ("graph_pathy2_k48", 48, "pathy2")


def test_recorded_cases_are_what_the_oracle_says_now():
    """tests/cpp/walks_cases.txt is walks_cases.text(): regenerate it (python -m tests.walks_cases) when the oracle or the generator changes"""
    assert open(walks_cases.FILE).read() == walks_cases.text()
    assert N_RECORDED == 5 and N_LARGER == 1 and os.path.getsize(walks_cases.FILE) < 200000


def fixture_text(golden_dir, case, K, which):
    i = walks_oracle.fixture_inputs(golden_dir, case, K, which)
    rs = i["rs"]
    c = dict(inv=i["inv"], kmers=[len(b) - K + 1 for b in i["edge_bases"]], K=K, edge_bases=i["edge_bases"], ce=i["ce"], reads_per=i["reads_per"], pairs=i["pairs"],
             reads=[i["read_bases"](id) for id in range(int(rs["n_reads"]))], pq=rs["pq_bytes"], pq_off=rs["pq_off"])
    return walks_cases.case_text(case, c, walks_oracle.fixture_walks(golden_dir, case, K, which))


@pytest.fixture(scope="module")
def more_cases(golden_dir, tmp_path_factory):
    """the larger seeded case and five fixtures in the form of walks_cases.txt; the largest fixture in a file of its own"""
    out = walks_cases.text(recorded=False).splitlines()
    for case, K, which in FIXTURES: out += fixture_text(golden_dir, case, K, which)
    d = tmp_path_factory.mktemp("walks")
    (d / "more_cases.txt").write_text("\n".join(out) + "\n")
    (d / "largest.txt").write_text("\n".join(fixture_text(golden_dir, *LARGEST)) + "\n")
    return str(d / "more_cases.txt"), str(d / "largest.txt")


@pytest.mark.parametrize("build", list(BUILDS))
def test_cpp_restatement_agrees_with_the_oracle(tmp_path, more_cases, build):
    exe = os.path.join(tmp_path, "test_walks")
    subprocess.check_call(["g++", *BUILDS[build], "-std=c++17", "-Wall", "-I", os.path.join(ROOT, "superplus_amd", "csrc"), "-o", exe,
                           os.path.join(ROOT, "tests", "cpp", "test_walks.cc")])
    runs = [(walks_cases.FILE, N_RECORDED), (more_cases[0], N_LARGER + len(FIXTURES))]
    if build == "plain": runs.append((more_cases[1], 1))                        # (graph_pathy2_k48: minutes under the sanitizers)
    for cases, n in runs:
        out = subprocess.run([exe, cases], capture_output=True, text=True, timeout=900)
        assert out.returncode == 0, out.stdout + out.stderr
        assert f"{n} recorded cases agree" in out.stdout
