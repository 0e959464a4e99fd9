"""tests/scons_oracle.py -- Stackster's stack consensus restated in Python -- pinned: its table on the six fixtures the walks tests use
(computed once a session from tests/walks_oracle.py's walks; the figures below were recorded when the two restatements first agreed on
every fixture) and what each seeded plant of tests/scons_cases.py fires.  CPU only."""
import pytest

from tests import scons_cases, scons_oracle
from tests.scons_oracle import c_round

# case: (pairs, yields, rows, rows_kept, trimmed, columns, cells, capped, recount, flat, allowed, disallowed, digest)
TABLE = {
    ("graph_frag_k48", 48, "frag"): (937, 930, 34427, 34419, 23, 315676, 3137644, 265431, 916, 0, 86091, 229585, "9ef08394f9e447f031aada3f8df5232a"),
    ("graph_pathy_k48", 48, "pathy"): (63, 63, 10419, 10208, 43, 36701, 1091278, 34348, 94, 0, 3921, 32780, "180cc4f369aa052fd25941551ae98d96"),
    ("graph_k48", 48, "reads"): (48, 48, 1984, 1752, 14, 17274, 158708, 8582, 0, 92, 14540, 2734, "15a19c794447aebaeb2bfcdb003d2d62"),
    ("graph_k40_nobc", 40, "reads"): (138, 136, 4567, 3592, 35, 43550, 319296, 16838, 0, 156, 38488, 5062, "17f1968b1a1ecbae3ed2ababba598e2b"),
    ("graph_special_k48", 48, "special"): (6, 6, 887, 887, 0, 2164, 79448, 1958, 130, 0, 357, 1807, "bddbf3cd8294c8685fb5bfd6fb3e4d7e"),
    ("graph_pathy2_k48", 48, "pathy2"): (725, 721, 90562, 86611, 505, 433428, 9286544, 382202, 1971, 0, 83315, 350113, "00a0a04624bde58be4d8c752d3e1ea3a"),
}
KEYS = ("pairs", "yields", "rows", "rows_kept", "trimmed", "columns", "cells", "capped", "recount", "flat", "allowed", "disallowed")


@pytest.mark.parametrize("fixture", list(TABLE), ids=[f[0] for f in TABLE])
def test_table_on_the_fixtures(golden_dir, fixture):
    r = scons_oracle.fixture_scons(golden_dir, *fixture)
    assert tuple(r[k] for k in KEYS) + ("%016x%016x" % r["digest"],) == TABLE[fixture]
    assert r["stacks"] == 2 * r["yields"] and len(r["elements"]) == 2 * r["pairs"] and r["allowed"] + r["disallowed"] == sum(len(t) for t in r["counts"])
    assert len(r["file"]) == (16 + 8 * (2 * r["pairs"] + 1) + 8 * (r["pairs"] + 1) + 32 * r["pairs"] + 2 * r["columns"] + 2 * (r["allowed"] + r["disallowed"]) + 7) // 8 * 8
    for e in r["elements"]:
        assert e["cols"] == min(e["M"], 400) and len(e["con"]) == len(e["conq"]) == e["cols"] and e["rows_kept"] <= e["rows"]
        assert all(0 <= q <= 100 for q in e["conq"]) and all(0 <= b <= 3 for b in e["con"])


def test_the_rounding_is_c_round():
    assert [c_round(x) for x in (0.49999999999999994, 0.5, 1.5, 2.5, 99.5, 100.5, 9.499999999999998, 99.4, 0.0)] == [0, 1, 2, 3, 100, 101, 9, 99, 0]
    assert round(0.5) == 0 and round(2.5) == 2                                  # Python's own rounds half to even: not used


@pytest.fixture(scope="module")
def planted():
    name, c = scons_cases.seeded()[0]
    assert name == "planted"
    return c, scons_cases.oracle(name, c)


def side(planted, name, s=0):
    c, r = planted
    return r["elements"][2 * c["names"][name] + s]


def test_widths_trim_and_rows(planted):
    for M in (48, 255, 256, 257, 400):
        e = side(planted, "M%d" % M)
        assert (e["M"], e["cols"], e["rows_kept"]) == (M, M, e["rows"]) and set(e["conq"]) == {100}
    e = side(planted, "M401")
    assert (e["M"], e["cols"]) == (401, 400) and e["rows_kept"] == e["rows"]
    e = side(planted, "M460")
    assert (e["M"], e["cols"], e["rows"] - e["rows_kept"]) == (460, 400, 2)      # the rows that end at column 60 are erased; the one that ends at 61 stays
    c, r = planted
    locs = c["recs"][2 * c["names"]["NEG"]]["locs"]
    assert locs[0][1] == -7 and side(planted, "NEG")["M"] == 103 and side(planted, "NEG")["conq"][0] == 70 and side(planted, "NEG")["conq"][95] == 30
    locs = c["recs"][2 * c["names"]["TWICE"]]["locs"]
    assert locs[0][0] == locs[1][0] and locs[0][2] != locs[1][2] and side(planted, "TWICE")["rows"] == 2
    for n in (1, 255, 256, 257, 600):
        e = side(planted, "LIVE%d" % n)
        assert e["rows"] == e["rows_kept"] == n and e["cols"] == 70 + min(2, n - 1)


def test_the_chosen_columns(planted):
    """what the sums say, worked out here with Python floats: the order of the adds, the rounding at and just below a half, the cap, the
    recount's two thresholds, the second base among equals, qualities that leave a cell undefined"""
    assert 20 + .1 + .1 > .2 + 10 + 10 and 20 + .1 + .1 != 20.2
    assert 10 - (.2 + .2 + .1) == 9.5 and (10 + .1 + .2) - (.2 + .2 + .2 + .2) == 9.499999999999998
    assert c_round(100 - (.2 + .2 + .2)) == 99 and 100 - (.2 + .2 + .1) == 99.5
    want = dict(ORDER=(0, 0), HALF=(0, 10), BELOW=(0, 9), D994=(0, 99), D995=(0, 100), D100=(0, 100), D300=(0, 100), V100=(0, 100), V1001=(0, 0), ONE30=(0, 77), TWO30=(0, 0), Q29=(0, 10), Q30=(0, 0),
                TIE=(0, 16), Q128=(0, 1))
    for s, name in ((0, "COLS"), (1, "COLS1")):
        e = side(planted, name, s)
        assert {k: (e["con"][col], e["conq"][col]) for k, col in scons_cases.COLS_AT.items()} == want, name
        others = [q for col, q in enumerate(e["conq"]) if col not in scons_cases.COLS_AT.values()]
        assert set(others) == {100}
    assert side(planted, "COLS1", 0)["M"] == 460                                 # beside a trimmed side 0


def test_coverage_and_flat_runs(planted):
    e = side(planted, "GAP5")
    assert e["con"][50:55] == [3] * 5 and e["conq"][50:55] == [0] * 5 and e["conq"][49] == 40 and e["conq"][55] == 40
    e = side(planted, "GAP10")
    assert e["con"][50:60] == [3] * 10 and e["conq"][50:60] == [0] * 10 and e["conq"][49] == 40
    assert set(side(planted, "RUN9")["conq"]) == {100}
    for name, at in (("RUN10", 30), ("RUN255", 251), ("RUNEND", 90)):
        e = side(planted, name)
        assert [i for i, q in enumerate(e["conq"]) if q == 0] == list(range(at, at + 10)) and e["con"][at:at + 10] == [0] * 10
    assert side(planted, "RUNEND")["cols"] == 100


def test_conflicts_and_pairs_that_do_not_yield(planted):
    c, r = planted
    for name, off in (("CONF+", 30), ("CONF-", -30), ("CONF0-", 0)):
        for k in (9, 10):
            t = r["counts"][c["names"]["%s%d" % (name, k)]]
            assert len(t) == 200 and t[off + 100] == k and t[0] == 0             # index offset + n2; offset = -n2: no overlap
            assert (t[off + 100] < scons_oracle.CONFLICTS) == (k == 9)
    for name in ("SIDE1NONE", "STATUS1", "STATUS2"):
        pi = c["names"][name]
        assert r["counts"][pi] == [] and r["elements"][2 * pi] == r["elements"][2 * pi + 1] == dict(rows=0, rows_kept=0, M=0, cols=0, con=[], conq=[])
    assert c["recs"][2 * c["names"]["SIDE1NONE"]]["placed"] == 1                # side 0 placed a read: it enters no stack
    assert r["yields"] == r["pairs"] - 3 and r["recount"] == 6 and r["trimmed"] == 3


def test_the_other_seeded_cases():
    for name, c in scons_cases.seeded()[1:]:
        r = scons_cases.oracle(name, c)
        if name == "no-pairs": assert r["pairs"] == 0 and len(r["file"]) == 32 and r["file"][:8] == b"DFKSCON1"
        else: assert r["yields"] == r["pairs"] - 1 and r["trimmed"] and r["flat"] and r["recount"] and r["disallowed"]
