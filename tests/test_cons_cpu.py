"""superplus_amd/csrc/dfk_cons.h -- the C++ restatement of CloseGap2's read stacks and their column consensus, the plan of its device
version and the layout of a.close.cons -- against tests/cons_oracle.py: tests/cpp/test_cons.cc (its own main) built plain and under
-fsanitize=address,undefined and run directly, on the seeded cases recorded in tests/cpp/cons_cases.txt, on the larger seeded cases and
on graph_pathy2_k48 and graph_frag_k48 written out in the same form.  It checks the literal transcription (the stack materialised), and
that the windowed device-order form gives the same bytes under stacks_per_batch 1, 37 and 2^30 and under small ranges.  CPU only."""
import os
import subprocess

import numpy as np
import pytest

from tests import closer_oracle, cons_cases, cons_oracle, partners_oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUILDS = {"plain": ["-O1"], "sanitized": ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]}
N_RECORDED = sum(1 for _, _, rec in cons_cases.seeded() if rec)
N_LARGER = sum(1 for _, _, rec in cons_cases.seeded() if not rec)


def test_recorded_cases_are_what_the_oracle_says_now():
    """tests/cpp/cons_cases.txt is cons_cases.text(): regenerate it (python -m tests.cons_cases) when the oracle or the generator changes"""
    assert open(cons_cases.FILE).read() == cons_cases.text()
    assert N_RECORDED == 4 and N_LARGER == 2 and os.path.getsize(cons_cases.FILE) < 100000


def tenths_answer(sums_in_order):
    """what exact arithmetic in tenths would decide: [(base, q)] in row order -> base"""
    t = [0, 0, 0, 0]
    for b, q in sums_in_order: t[b] += 1 if q == 0 else 2 if q <= 2 else 10 * q
    return t.index(max(t))


def test_seeded_cases_hold_what_the_fixtures_lack():
    cases = {name: c for name, c, _ in cons_cases.seeded()}
    got = {name: cons_cases.oracle(name, c) for name, c in cases.items()}
    c, p = cases["planted"], got["planted"]
    st, edge = p["stacks"], c["edge"]
    # ROUND (stack 0): the two double-rounding columns.  Column 0: doubles against tenths; column 1: the order of the additions
    s = st[0]
    assert not s["reversed"] and s["M"] == 2 and list(s["bases"]) == [1, 1]
    assert (s["sums"][0][0], s["sums"][1][0]) == (20.2, 20.200000000000003) and tenths_answer([(0, 2), (0, 10), (0, 10), (1, 20), (1, 0), (1, 0)]) == 0
    assert (s["sums"][0][1], s["sums"][1][1]) == (47.3, 47.300000000000004) and sum(sorted([.2, 37., 10., .1])) == 47.3 and .2 + 37. + 10. + .1 == 47.300000000000004
    assert s["added"] == 14 and s["rows"] == s["rows_kept"] == 8                  # the cells at Q128 and Q130 are undefined
    assert list(st[17]["bases"]) == [2, 2] and st[17]["reversed"]                 # the same rows reversed: the complement here (no tie, no empty column)
    # TIE (stacks 8, 9): both reversed; a tie and two empty columns that do not fall as the complement of the unreversed answer would
    assert st[8]["reversed"] and st[9]["reversed"] and list(st[8]["bases"]) == list(st[9]["bases"])
    rows = c["locs"][c["ce"].index(edge["TIE"])]
    plain = cons_oracle.one_stack(rows, c["kmers"][edge["TIE"]] + cons_cases.K - 1, False, lambda id: c["reads"][id], lambda id: c["quals"][id])
    flipped = [3 - int(b) for b in plain["bases"][::-1]]
    assert plain["tied"] >= 1 and plain["empty"] == 2 and list(plain["bases"][:5]) == [0, 1, 0, 0, 0]
    differ = [i for i in range(8) if flipped[i] != int(st[8]["bases"][i])]
    assert differ == [3, 4, 5, 7] and [int(st[8]["bases"][i]) for i in differ] == [0, 0, 1, 0]      # the two empty columns give base 0, not 3; the ties the first of the complemented bases
    # M400, M401: M exactly 400 (no trim; the row wholly at negative columns and the one running off column 0 stay) and 401 (one column goes)
    assert (st[2]["rows"], st[2]["rows_kept"], st[2]["M"], st[2]["cols"], st[2]["trimmed"], st[2]["live"]) == (3, 3, 400, 400, False, 2)
    assert (st[4]["rows"], st[4]["rows_kept"], st[4]["M"], st[4]["cols"], st[4]["trimmed"]) == (6, 5, 401, 400, True)       # the read of 1 base at column 0 is erased
    r_edge = c["locs"][c["ce"].index(edge["M401"])][1][0]
    assert [r[0] for r in c["locs"][c["ce"].index(edge["M401"])]].count(r_edge) == 2 and r_edge in [r[0] for r in c["parts"][5]]   # one read in two rows, and as a partner row
    assert {127, 128, 190} <= set(int(x) for x in c["quals"][r_edge]) and max(len(r) for r in c["reads"]) == 401 and min(len(r) for r in c["reads"]) == 1
    with pytest.raises(Exception):
        from superplus_amd import feudal
        assert feudal.pq_decode(feudal.pq_encode([63, 255])) == [63, 255]        # 255 beside 63 is a range of 192: more than seven bits
    ne = c["kmers"][edge["M400"]] + cons_cases.K - 1
    back = c["locs"][c["ce"].index(edge["M400"])][2]
    assert not back[2] and ne - back[1] - (len(c["reads"][back[0]]) - 1) - 1 < 0   # a non-forward row with ne - pos - j - 1 < 0 for its last j
    # LONG: rows wholly in front of the window, erased; stacks without rows; the self-inverse edge; a pair twice and reversed
    assert (st[6]["M"], st[6]["cols"], st[6]["rows"], st[6]["rows_kept"], st[6]["live"]) == (1047, 400, 8, 5, 5)
    assert (st[1]["rows"], st[1]["M"], st[1]["cols"], st[1]["reversed"]) == (0, 0, 0, True)
    assert st[10]["reversed"] and st[11]["reversed"] and list(st[10]["bases"]) == list(st[11]["bases"]) and c["inv"][edge["S"]] == edge["S"]
    assert p["dims"][12:14] == p["dims"][14:16] == p["dims"][16:18][::-1] and c["pairs"][6] == c["pairs"][7] and c["pairs"][8] == (c["inv"][c["pairs"][6][1]], c["inv"][c["pairs"][6][0]])
    assert st[13]["rows"] == 4 and st[13]["partner_rows"] == 1                   # a partner row behind the locs rows
    # reads at odd byte offsets, the last read ending where the buffer ends
    a = cons_cases.arrays(c)
    assert any(int(o) % 2 for o in a["read_off"]) and int(a["read_off"][-1]) == len(a["read_packed"]) and int(a["pq_off"][-1]) == len(a["pq"])
    for name in ("random", "random-long", "many-rows", "many-stacks"):
        g = got[name]
        assert g["trimmed"] > 0 and g["tied"] > 0 and g["empty"] > 0 and g["lost_rows"] > 0 and g["live"] < g["rows"] and 0 < g["reversed"] < g["n_stacks"], name
    assert got["no-pairs"]["file"] == b"DFKCCON1" + bytes(16) and got["no-pairs"]["n_stacks"] == 0
    assert max(s["rows"] for s in got["many-rows"]["stacks"]) > 2 * 2048 and got["many-stacks"]["n_stacks"] > 2 * 2048


@pytest.fixture(scope="module")
def more_cases(golden_dir, tmp_path_factory):
    """the larger seeded cases, and pathy2 and frag in the form of cons_cases.txt"""
    out = cons_cases.text(recorded=False).splitlines()
    for case, K, which in (("graph_pathy2_k48", 48, "pathy2"), ("graph_frag_k48", 48, "frag")):
        i = partners_oracle.fixture_inputs(golden_dir, case, K, which)
        p = partners_oracle.fixture_partners(golden_dir, case, K, which)
        rs = i["rs"]
        n = int(rs["n_reads"])
        c = dict(inv=i["inv"], kmers=closer_oracle.fixture_inputs(golden_dir, case, K, which)["kmers"], ce=i["ce"], locs=i["locs_per"], parts=p["elements"], pairs=i["pairs"],
                 reads=[i["read_bases"](id) for id in range(n)], pq=rs["pq_bytes"], pq_off=rs["pq_off"])
        out += cons_cases.case_text(case, c, cons_oracle.fixture_cons(golden_dir, case, K, which), K)
    path = tmp_path_factory.mktemp("cons") / "more_cases.txt"
    path.write_text("\n".join(out) + "\n")
    return str(path)


@pytest.mark.parametrize("build", list(BUILDS))
def test_cpp_restatement_agrees_with_the_oracle(tmp_path, more_cases, build):
    exe = os.path.join(tmp_path, "test_cons")
    subprocess.check_call(["g++", *BUILDS[build], "-std=c++17", "-Wall", "-I", os.path.join(ROOT, "superplus_amd", "csrc"), "-o", exe,
                           os.path.join(ROOT, "tests", "cpp", "test_cons.cc")])
    for cases, n in ((cons_cases.FILE, N_RECORDED), (more_cases, N_LARGER + 2)):
        out = subprocess.run([exe, cases], capture_output=True, text=True, timeout=900)
        assert out.returncode == 0, out.stdout + out.stderr
        assert f"{n} recorded cases agree" in out.stdout
