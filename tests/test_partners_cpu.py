"""superplus_amd/csrc/dfk_partners.h -- the C++ restatement of CloseGap2's search for unplaced partners, the plan of its device version and
the layout of a.close.partners -- against tests/partners_oracle.py: tests/cpp/test_partners.cc (its own main) built plain and under
-fsanitize=address,undefined and run directly, on the seeded cases recorded in tests/cpp/partners_cases.txt, on the larger seeded cases
and on graph_pathy2_k48 and graph_frag_k48 written out in the same form.  It checks the literal transcription, and that the device
version's order of work gives the same records under query batches of 1, 37 and 2^30 and under small ranges.  CPU only."""
import os
import subprocess

import pytest

from tests import partners_cases, partners_oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUILDS = {"plain": ["-O1"], "sanitized": ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]}
N_RECORDED = sum(1 for _, _, rec in partners_cases.seeded() if rec)
N_LARGER = sum(1 for _, _, rec in partners_cases.seeded() if not rec)


def test_recorded_cases_are_what_the_oracle_says_now():
    """tests/cpp/partners_cases.txt is partners_cases.text(): regenerate it (python -m tests.partners_cases) when the oracle or the generator changes"""
    assert open(partners_cases.FILE).read() == partners_cases.text()
    assert N_RECORDED == 5 and N_LARGER == 2 and os.path.getsize(partners_cases.FILE) < 100000


def test_seeded_cases_hold_what_the_fixtures_lack():
    got = {name: partners_cases.oracle(name, c) for name, c, _ in partners_cases.seeded()}
    p = got["planted"]
    # what the module's text says of the planted reads, element by element (es = {B, A}: 0, 1; {C, A}: 2, 3; {D, C}: 4, 5; {S, S}: 8, 9; {A, A}: 10, 11)
    assert p["elements"][0] == [(1, 27, True), (7, 67, True), (9, -33, True), (13, 37, True), (15, 7, True)]      # r3 dropped, r5 too short, r11 skipped
    assert p["elements"][1] == [(19, 7, True)] and p["elements"][3] == [(23, 2, True), (25, 5, True), (27, 0, True)]
    assert p["elements"][2] == p["elements"][4] == p["elements"][5] == p["elements"][10] == p["elements"][11] == []
    assert p["elements"][8] == p["elements"][9] == [(1, 20, True)]
    assert p["elements"][12:14] == p["elements"][0:2] and p["elements"][14:16] == [p["elements"][1], p["elements"][0]]     # a pair twice, and reversed
    for name in ("planted", "random", "planted-more", "many-queries", "large-bod"):
        assert got[name]["kept"] > 0 and got[name]["multi"] > 0 and got[name]["any_hit"] == got[name]["kept"] + got[name]["multi"], name
    for name in ("planted", "random", "planted-more"):
        assert any(pos < 0 for _, pos, _ in got[name]["records"]), name
    assert got["no-pairs"]["file"] == b"DFKCPRT1" + bytes(16) and got["no-reads"]["queries"] == 0 and got["no-reads"]["entries"] > 0
    assert got["many-queries"]["queries"] > 2 * 2048 and got["large-bod"]["largest_bod"] > 2 * 2048


@pytest.fixture(scope="module")
def more_cases(golden_dir, tmp_path_factory):
    """the larger seeded cases, and pathy2 and frag in the form of partners_cases.txt"""
    out = partners_cases.text(recorded=False).splitlines()
    for case, K, which in (("graph_pathy2_k48", 48, "pathy2"), ("graph_frag_k48", 48, "frag")):
        i = partners_oracle.fixture_inputs(golden_dir, case, K, which)
        c = dict(inv=i["inv"], edges=i["edge_bases"], ce=i["ce"], locs=i["locs_per"], anchors=i["anchors_per"], pairs=i["pairs"],
                 reads=[i["read_bases"](id) for id in range(i["rs"]["n_reads"])])
        out += partners_cases.case_text(case, c, partners_oracle.fixture_partners(golden_dir, case, K, which))
    path = tmp_path_factory.mktemp("partners") / "more_cases.txt"
    path.write_text("\n".join(out) + "\n")
    return str(path)


@pytest.mark.parametrize("build", list(BUILDS))
def test_cpp_restatement_agrees_with_the_oracle(tmp_path, more_cases, build):
    exe = os.path.join(tmp_path, "test_partners")
    subprocess.check_call(["g++", *BUILDS[build], "-std=c++17", "-Wall", "-I", os.path.join(ROOT, "superplus_amd", "csrc"), "-o", exe,
                           os.path.join(ROOT, "tests", "cpp", "test_partners.cc")])
    for cases, n in ((partners_cases.FILE, N_RECORDED), (more_cases, N_LARGER + 2)):
        out = subprocess.run([exe, cases], capture_output=True, text=True, timeout=600)
        assert out.returncode == 0, out.stdout + out.stderr
        assert f"{n} recorded cases agree" in out.stdout
