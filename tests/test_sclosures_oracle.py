"""tests/sclosures_oracle.py -- Stackster's closures restated in Python -- pinned: its table on the six fixtures the walks tests use
(computed once a session from tests/walks_oracle.py's walks and tests/soffsets_oracle.py's offsets; the figures below were recorded when
the two restatements first agreed on every fixture) and what each seeded plant of tests/sclosures_cases.py fires.  On every fixture
kept = closable = offsets (tests/test_soffsets_oracle.py), so each closable pair has one closure; two and three closures a pair, dropped
records, the edge trims with erased rows and the rowless rule are the seeded cases' ground.  CPU only."""
import struct

import numpy as np
import pytest

from tests import sclosures_cases, sclosures_oracle
from tests.sclosures_cases import COLS_AT
from tests.test_soffsets_oracle import TABLE as SOFFSETS_TABLE

# case: (closures, columns, rows over all closures, cells added, live rows walked, rows erased by the two trims, empty columns, closures
# shorter than K, digest)
TABLE = {
    ('graph_frag_k48', 48, 'frag'): (306, 89768, 14717, 1323668, 14756, 39, 0, 0, 'db760d526d184b8d061e4a4875c5bd00'),
    ('graph_pathy_k48', 48, 'pathy'): (1, 628, 245, 26253, 245, 0, 0, 0, '8c8b10137289fc44eae482f50b537704'),
    ('graph_k48', 48, 'reads'): (0, 0, 0, 0, 0, 0, 0, 0, '00000000000000000000000000000000'),
    ('graph_k40_nobc', 40, 'reads'): (0, 0, 0, 0, 0, 0, 0, 0, '00000000000000000000000000000000'),
    ('graph_special_k48', 48, 'special'): (6, 276, 638, 22924, 887, 249, 0, 6, '8d6e16a9d3523f81360beb9605f927bc'),
    ('graph_pathy2_k48', 48, 'pathy2'): (35, 8338, 2667, 268923, 2814, 147, 0, 1, 'f7927148c10ad0f802447f29f0becc40'),
}


@pytest.mark.parametrize("fixture", list(TABLE), ids=[f[0] for f in TABLE])
def test_table_on_the_fixtures(golden_dir, fixture):
    r = sclosures_oracle.fixture_sclosures(golden_dir, *fixture)
    so = SOFFSETS_TABLE[fixture]
    got = (r["closures"], r["columns"], sum(x[3] for x in r["records"]), r["added"], r["live"], r["erased"], r["empty"], r["short"], "%016x%016x" % r["digest"])
    assert got == TABLE[fixture]
    assert r["closures"] == r["closable"] == so[9] == so[8] and r["pairs"] == so[0] and r["yields"] == so[1] and r["none"] == so[0] - so[9] and r["over"] == 0 and r["rowless"] == 0
    n, npairs, nb = r["closures"], r["pairs"], r["columns"]
    for (pi, off, cols, rows), a, b in zip(r["records"], r["starts"], r["starts"][1:]):
        assert 8 <= b - a == cols <= 792 and rows > 0 and r["pair_first"][pi + 1] - r["pair_first"][pi] == 1
    assert set(int(x) for x in r["bases"]) <= {0, 1, 2, 3}
    # the file: magic, n, n_pairs, pair table, starts, records, bases, padding
    f = r["file"]
    assert f[:8] == b"DFKSCLS1" and struct.unpack_from("<QQ", f, 8) == (n, npairs)
    assert len(f) == 24 + 8 * (npairs + 1) + 8 * (n + 1) + 16 * n + (nb + 7) // 8 * 8
    assert list(np.frombuffer(f, "<u8", npairs + 1, 24)) == r["pair_first"] and list(np.frombuffer(f, "<u8", n + 1, 24 + 8 * (npairs + 1))) == r["starts"]
    at = 24 + 8 * (npairs + 1) + 8 * (n + 1)
    if n: assert struct.unpack_from("<IiII", f, at) == r["records"][0] and struct.unpack_from("<IiII", f, at + 16 * (n - 1)) == r["records"][-1]
    assert f[at + 16 * n: at + 16 * n + nb] == bytes(r["bases"]) and not any(f[at + 16 * n + nb:])


@pytest.fixture(scope="module")
def planted():
    name, c = sclosures_cases.seeded()[0]
    assert name == "planted"
    return c, sclosures_cases.oracle(name, c)


def pair(planted, name):
    """-> (the pair's closures as ( offset, cols, rows ), its closures, its two consensus elements)"""
    c, (sc, r) = planted
    pi = c["names"][name]
    return [(x["offset"], x["cols"], x["rows"]) for x in r["per"][pi]], r["per"][pi], sc["elements"][2 * pi:2 * pi + 2]


def test_which_pairs_get_closures(planted):
    c, (sc, r) = planted
    assert [c["names"][n] for n in ("NONE0", "NONE2")] == [0, r["pairs"] - 1] and 0 < c["names"]["NONE1"] < r["pairs"] - 1 and r["yields"] == r["pairs"] - 3
    for n in ("NONE0", "NONE1", "NONE2", "FOUR", "NOKEPT"): assert pair(planted, n)[0] == [], n
    assert [x[0] for x in pair(planted, "TWO")[0]] == [0, 12] and [x[0] for x in pair(planted, "THREE")[0]] == [-5, 3, 20]
    assert [x[0] for x in pair(planted, "DROPMID")[0]] == [0, 15]                # the dropped record between them is not merged
    assert (r["over"], r["none"], r["closable"], r["closures"]) == (1, 4, r["yields"] - 2, r["closable"] + 1 + 2 + 1 + 1)
    pf = r["pair_first"]
    assert [pf[i + 1] - pf[i] for i in range(r["pairs"])] == [len(cl) for cl in r["per"]] and [x[0] for x in r["records"]] == sorted(x[0] for x in r["records"])


def test_offsets_of_either_sign_and_the_edge_trims(planted):
    for n, (off, n1, n2) in dict(POS=(20, 60, 70), ZERO=(0, 50, 60), NEG=(-30, 40, 70)).items():
        cl, per, el = pair(planted, n)
        assert [e["cols"] for e in el] == [n1, n2] and n1 != n2 and [(x[0], x[1]) for x in cl] == [(off, off + n2)] and cl[0][2] == el[0]["rows_kept"] + el[1]["rows_kept"], n
    # a row wholly beyond the edge is erased, one that reaches 5 columns into the window stays
    for n in ("RTRIM", "LTRIM"):
        cl, per, el = pair(planted, n)
        assert cl == [(10 if n == "RTRIM" else -40, 60, 4)] and el[0]["rows_kept"] + el[1]["rows_kept"] == 5, n
    # ... and one whose only cells inside the window are undefined
    for n in ("QEDGE0", "QEDGE1"):
        cl, per, el = pair(planted, n)
        assert cl == [(10 if n == "QEDGE0" else -40, 60, 3)] and el[0]["rows_kept"] + el[1]["rows_kept"] == 4, n
    cl, per, el = pair(planted, "ROWLESS")
    assert cl == [(-42, 8, 0)] and list(per[0]["bases"]) == [3] * 8 and per[0]["empty"] == 8 and [e["cols"] for e in el] == [110, 50]
    c, (sc, r) = planted
    assert r["rowless"] == 1 and r["erased"] == 1 + 1 + 1 + 1 + 2


def test_the_order_of_the_sums_ties_and_the_lowered_qualities(planted):
    c, (sc, r) = planted
    sums = sclosures_oracle.run(c["recs"], lambda id: c["reads"][id], lambda id: c["quals"][id], c["K"],
                                [p if i == c["names"]["COLS"] else [] for i, p in enumerate(c["so_per"])], keep_sums=True)["per"][c["names"]["COLS"]][0]["sums"]
    cl, per, el = pair(planted, "COLS")
    b = per[0]["bases"]
    assert sums[COLS_AT["ORDER"]][:2] == [20.200000000000003, 20.2] and 20.0 + (0.1 + 0.1) == 0.2 + (10.0 + 10.0) and b[COLS_AT["ORDER"]] == 0      # per-stack sums would tie and base 1 would win
    assert sums[COLS_AT["TIE"]] == [30.0, 30.0, 6.0, 0.4] and b[COLS_AT["TIE"]] == 1
    assert sums[COLS_AT["Q12"]][:2] == [0.2 + 0.1, 0.2 + 0.1] and b[COLS_AT["Q12"]] == 1
    assert sums[COLS_AT["Q00"]] == [0.2, 0.2, 0.1, 0.2] and b[COLS_AT["Q00"]] == 3
    lo, hi = COLS_AT["GAP"]
    assert list(b[lo:hi]) == [3] * (hi - lo) and per[0]["empty"] == hi - lo and all(max(s) == 0.0 for s in sums[lo:hi]) and cl == [(0, 48, 12)]
    # the run of 20 is lowered to 5 and loses its column to the Q30 row; the run of 19 keeps its 40
    assert pair(planted, "HOMO20")[1][0]["bases"][15] == 1 and pair(planted, "HOMO19")[1][0]["bases"][15] == 0
    assert pair(planted, "HOMO20")[1][0]["bases"][12] == 0


def test_widths_rows_and_reads_that_stand_twice(planted):
    c, (sc, r) = planted
    assert pair(planted, "C8")[0] == [(0, 8, 2)] and [e["cols"] for e in pair(planted, "C8")[2]] == [8, 8]
    assert pair(planted, "C256")[0][0][:2] == (56, 256) and pair(planted, "C257")[0][0][:2] == (57, 257) and [e["cols"] for e in pair(planted, "C257")[2]] == [199, 200]
    assert pair(planted, "C792")[0][0][:2] == (392, 792) and [e["cols"] for e in pair(planted, "C792")[2]] == [400, 400]
    cl, per, el = pair(planted, "W460")
    assert cl[0][:2] == (240, 640) and [e["M"] for e in el] == [460, 460] and any(l[1] < 60 for l in c["recs"][2 * c["names"]["W460"]]["locs"])
    t = c["recs"][2 * c["names"]["TWICE"]]["locs"]
    assert t[0][0] == t[1][0] and t[0][2] != t[1][2] and pair(planted, "TWICE")[0] == [(12, 82, 3)]
    b0, b1 = (c["recs"][2 * c["names"]["BOTH"] + s]["locs"] for s in (0, 1))
    assert b0[0][0] == b1[0][0] and [x[:2] for x in pair(planted, "BOTH")[0]] == [(-9, 75), (30, 114)]
    assert pair(planted, "ROWS600")[0] == [(10, 72, 1200)]
    cl, per, el = pair(planted, "SKIPALL")
    assert cl == [(200, 600, 9)] and el[1]["cols"] == 400 and per[0]["empty"] == 200 and list(per[0]["bases"][400:]) == [3] * 200      # stack 1's rows end at merged column 300
    assert r["short"] == 3                                                       # C8, NEG (40) and ROWLESS


def test_the_other_seeded_cases():
    seeded = dict(sclosures_cases.seeded())
    c = seeded["soffsets-planted"]
    sc, r = sclosures_cases.oracle("soffsets-planted", c)
    n = lambda name: [x["offset"] for x in r["per"][c["names"][name]]]
    assert n("EDGE") == [0, 80] and n("KEPT3") == [0, 30, 60] and n("KEPT4") == [] and n("NEGATIVE") == [-30] and r["over"] == 1 and r["rowless"] == 0
    sc, r = sclosures_cases.oracle("random", seeded["random"])
    assert r["closures"] == 7 and r["erased"] > 0 and any(x[1] < 0 for x in r["records"]) and any(x[1] > 0 for x in r["records"])
    sc, r = sclosures_cases.oracle("no-pairs", seeded["no-pairs"])
    assert r["pairs"] == 0 and r["file"] == b"DFKSCLS1" + bytes(16) + bytes(8) + bytes(8) and r["pair_first"] == [0] and r["starts"] == [0]
