"""tests/closures_oracle.py -- CloseGap2's closures restated in plain Python -- on the four fixtures that have pairs: the table the two
restatements (this one and superplus_amd/csrc/dfk_closures.h, held to each other by tests/test_closures_cpu.py) must reproduce, the
file's layout, and what each seeded case fires.  CPU only."""
import struct

import numpy as np
import pytest

from tests import closures_cases, closures_oracle, cons_cases, cons_oracle
from tests.test_offsets_oracle import TABLE as OFFSETS_TABLE

# fixture: closures (= pairs1 + 2 pairs2 of tests/test_offsets_oracle.py's table), columns, cells added, live rows walked, columns nothing
# was added to, closures shorter than K -- recorded from the oracle
ROWS = {"graph_frag_k48": (351, 109859, 1653365, 18056, 55, 0), "graph_pathy2_k48": (38, 10865, 279218, 2623, 0, 0), "graph_pathy_k48": (2, 1282, 46586, 458, 0, 0),
        "graph_k40_nobc": (1, 400, 9224, 106, 0, 0)}
TABLE = [(case, K, which, ROWS[case]) for case, K, which, _ in OFFSETS_TABLE]


@pytest.mark.parametrize("case,K,which,row", TABLE, ids=[t[0] for t in TABLE])
def test_the_table_on_the_fixtures(golden_dir, case, K, which, row):
    r = closures_oracle.fixture_closures(golden_dir, case, K, which)
    off = next(t[3] for t in OFFSETS_TABLE if t[0] == case)
    assert row[0] == off[7] + 2 * off[8]                                           # pairs1 + 2 pairs2
    assert (r["closures"], r["columns"], r["added"], r["live"], r["empty"], r["short"]) == row
    assert r["rowless"] == 0 and r["over"] == off[9] and r["closable"] == off[7] + off[8] and r["pairs"] == off[0]
    # one offset a pair and nothing else: the seeded cases carry the rest
    assert all(len(cl) <= 1 for cl in r["per"]) and [len(cl) for cl in r["per"]] == [1 if len(o) == 1 else 0 for o in r["offsets_per"]]
    n, npairs = r["closures"], r["pairs"]
    for (pi, off_, cols, rows), a, b in zip(r["records"], r["starts"], r["starts"][1:]):
        assert b - a == cols <= 800 and rows > 0 and r["pair_first"][pi + 1] - r["pair_first"][pi] == 1 and r["offsets_per"][pi] == [off_]
    assert set(int(x) for x in r["bases"]) <= {0, 1, 2, 3}
    # the file: magic, n, n_pairs, pair table, starts, records, bases, padding
    f = r["file"]
    nb = r["columns"]
    assert f[:8] == b"DFKCCLS1" and struct.unpack_from("<QQ", f, 8) == (n, npairs)
    assert len(f) == 24 + 8 * (npairs + 1) + 8 * (n + 1) + 16 * n + (nb + 7) // 8 * 8
    assert list(np.frombuffer(f, "<u8", npairs + 1, 24)) == r["pair_first"] and list(np.frombuffer(f, "<u8", n + 1, 24 + 8 * (npairs + 1))) == r["starts"]
    at = 24 + 8 * (npairs + 1) + 8 * (n + 1)
    assert struct.unpack_from("<IiII", f, at) == r["records"][0] and struct.unpack_from("<IiII", f, at + 16 * (n - 1)) == r["records"][-1]
    assert f[at + 16 * n: at + 16 * n + nb] == bytes(r["bases"]) and not any(f[at + 16 * n + nb:])


def test_seeded_cases_fire_what_the_fixtures_lack():
    cases = {name: c for name, c, _ in closures_cases.seeded()}
    got = {name: closures_cases.oracle(name, c) for name, c in cases.items()}
    c, p = cases["planted"], got["planted"]
    per = p["per"]
    quals_of, bases_of = (lambda id: c["quals"][id]), (lambda id: c["reads"][id])
    cons = cons_oracle.run(c["inv"], c["kmers"], cons_cases.K, c["ce"], c["locs"], c["parts"], c["pairs"], bases_of, quals_of)
    con = lambda q: [int(b) for b in cons["bases"][cons["starts"][q]:cons["starts"][q + 1]]]
    assert [len(x) for x in per] == [1, 1, 2, 1, 1, 1, 1, 1, 1, 0, 0, 1, 1, 1, 1] and p["over"] == 1 and p["closable"] == 13 and p["closures"] == 14
    # pair 0: the sums cross the stack boundary, and adding per-stack sums would give the other base
    x = per[0][0]
    assert x["cols"] == 1 and x["sums"][0][:2] == [20.200000000000003, 20.2] and list(x["bases"]) == [0]
    s0, s1 = 20.0, 0.2                                                             # stack 0 alone: base 0, base 1
    t0, t1 = 0.1 + 0.1, 10.0 + 10.0                                                # stack 1 alone
    assert (s0 + t0, s1 + t1) == (20.2, 20.2) and sorted([(s0 + t0, 0), (s1 + t1, 1)], reverse=True)[0][1] == 1
    # pair 1: a tie goes to the higher base where con of the same stack chose the lower; columns nothing was added to give 3, con gives 0
    x = per[1][0]
    assert list(x["bases"]) == [2, 3, 3, 1, 3] and con(2) == [0, 0, 0, 1, 3] and x["sums"][0] == [10.0, 0.0, 10.0, 0.0] and x["empty"] == 2 and x["rows"] == 3
    # offsets negative, zero and positive; the widths; abutting stacks; one inside the other; cols1 != cols2; two offsets in order
    assert [(r[1], r[2]) for r in p["records"]] == [(0, 1), (0, 5), (0, 256), (1, 257), (256, 512), (-256, 512), (200, 513), (10, 400), (-50, 400), (392, 792), (3, 13), (0, 0), (100, 500), (-20, 400)]
    dims = cons["dims"]
    assert [dims[2 * pi][3] for pi in (2, 5, 7, 8)] == [256, 400, 256, 400] and [dims[2 * pi + 1][3] for pi in (2, 5, 7, 8)] == [256, 313, 400, 400]
    assert dims[2 * 8][2] > 400 and dims[2 * 8 + 1][2] > 400                       # both trimmed
    assert max(0, 400 - (10 + 313)) == 77 and max(0, -50 + 400 - 256) == 94        # right_ext2 of pair 6, right_ext1 of pair 7
    assert all(f == (cl["cols"], cl["cols"]) for cls in per for cl in cls for f in [cl["forms"]])
    assert per[2][0]["offset"] == 0 and per[2][1]["offset"] == 1 and p["pair_first"][2:5] == [2, 4, 5] and c["pairs"][2] == c["pairs"][3] == c["pairs"][4]
    # abutting: every column is covered by one stack alone, and the closure is still no splice of the two con (ties and empty columns fall otherwise)
    x = per[3][0]
    differ = [(int(a), b) for a, b in zip(x["bases"][:256], con(6)) if a != b]
    assert x["cols"] == 512 and differ and all(a > b for a, b in differ) and (3, 0) in differ      # (a tie, or nothing added: the higher base here, the lower there)
    # T1's row that is defined only in front of the window is live, walked and erased; the partner row behind T1's rows is there
    assert (dims[10][0], dims[10][1]) == (5, 3) and per[5][0]["rows"] == 3 + 2 and per[6][0]["rows"] == 2 + 2
    # side 0 reversed; the self-inverse edge
    assert c["pairs"][11] == (c["edge"]["S"], c["edge"]["S"]) and cons["stacks"][22]["reversed"] and cons["stacks"][23]["reversed"]
    # a side without rows, both sides: the rowless rule
    assert (per[12][0]["cols"], per[12][0]["rows"]) == (0, 0) and (per[13][0]["cols"], per[13][0]["rows"]) == (500, 0) and set(per[13][0]["bases"]) == {3} and p["rowless"] == 2
    assert per[13][0]["empty"] == 500 and per[14][0]["rows"] == 3 and p["short"] == 4
    b = [int(v) for v in per[14][0]["bases"]]
    assert b[:20] == [3] * 20 and b[20:25] == [2, 3, 3, 1, 3] and b[25:] == [3] * 375
    # the qualities; one read in rows of both stacks
    qs = set(int(q) for qq in c["quals"] for q in qq)
    assert {0, 1, 2, 127, 128, 190} <= qs
    rows_of = lambda n: {r[0] for r in c["locs"][c["ce"].index(c["edge"][n])]}
    assert rows_of("W256") & rows_of("V256")
    # the other cases
    for name in ("random", "random-long"):
        g = got[name]
        assert g["closures"] > g["closable"] > 0 and g["over"] > 0 and g["empty"] > 0 and any(r[1] < 0 for r in g["records"]) and any(r[1] > 0 for r in g["records"]), name
    assert got["no-pairs"]["file"] == b"DFKCCLS1" + bytes(32) and got["no-pairs"]["pairs"] == 0
    n = got["none-closable"]
    assert n["pairs"] == 13 and n["closable"] == 0 and n["closures"] == 0 and n["over"] > 0 and n["file"] == b"DFKCCLS1" + struct.pack("<QQ", 0, 13) + bytes(8 * 14 + 8)
    assert max(len(per_) for per_ in cases["many-rows"]["locs"]) == 5000 and got["many-rows"]["closures"] == 5
    assert got["many-closures"]["closures"] >= 4200 > 2 * 2048 and got["many-closures"]["rowless"] > 0
