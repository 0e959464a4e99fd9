"""tests/soffsets_oracle.py -- Stackster's stack offsets restated in Python -- pinned: its table on the six fixtures the walks tests use
(computed once a session from tests/walks_oracle.py's walks and tests/scons_oracle.py's consensus; the figures below were recorded when
the two restatements first agreed on every fixture) and what each seeded plant of tests/soffsets_cases.py fires.  graph_k48 and
graph_k40_nobc have candidates but not one result (no row reaches 20 bits against the other stack's consensus): that ground is the
seeded cases'; no fixture has a pair with two kept offsets or a dropped one either (EDGE, KEPT3, KEPT4).  CPU only."""
import pytest

from tests import offsets_oracle, soffsets_cases, soffsets_oracle
from tests.soffsets_oracle import DROPPED, KEPT

# case: (pairs, yields, rows, hits, seen, disallowed-skipped, results, offsets, kept, closable, look-ups, digest)
TABLE = {
    ('graph_frag_k48', 48, 'frag'): (937, 930, 34419, 419787, 8347, 7095, 7067, 306, 306, 306, 12891039, '05c5626588e6117ccf0d766c328faf62'),
    ('graph_pathy_k48', 48, 'pathy'): (63, 63, 10208, 9883, 108, 3433, 92, 1, 1, 1, 261224, '43ca3d92307794f32f2987a02d00c0cf'),
    ('graph_k48', 48, 'reads'): (48, 48, 1752, 253, 95, 134, 0, 0, 0, 0, 91676, '1e3361f0f82265d1595a9fbfc62bc3f8'),
    ('graph_k40_nobc', 40, 'reads'): (138, 136, 3592, 247, 144, 93, 0, 0, 0, 0, 246699, '31e6fe6a3912a85140da099975c82766'),
    ('graph_special_k48', 48, 'special'): (6, 6, 887, 18198, 590, 0, 518, 6, 6, 6, 157626, 'f9b7d957b9bef32a152c76f63a60b37f'),
    ('graph_pathy2_k48', 48, 'pathy2'): (725, 721, 86611, 192051, 2750, 39424, 2060, 35, 35, 35, 8400126, 'c033f5e2c8423d31bcf51c052205e6d0'),
}
KEYS = ("pairs", "yields", "rows", "hits", "seen", "disallowed", "results", "offsets", "kept", "closable", "lookups")


@pytest.mark.parametrize("fixture", list(TABLE), ids=[f[0] for f in TABLE])
def test_table_on_the_fixtures(golden_dir, fixture):
    r = soffsets_oracle.fixture_soffsets(golden_dir, *fixture)
    assert tuple(r[k] for k in KEYS) + ("%016x%016x" % r["digest"],) == TABLE[fixture]
    assert len(r["file"]) == 16 + 8 * (r["pairs"] + 1) + 16 * r["pairs"] + 24 * r["offsets"] and r["file"][:8] == b"DFKSOFF1"
    assert r["kept"] + r["dropped"] == r["offsets"] and r["results"] <= r["seen"] <= r["hits"] and r["pairs_0"] + r["pairs_1"] + r["pairs_2"] + r["pairs_3"] + r["pairs_more"] == r["pairs"]
    for w, recs in zip(r["words"], r["per"]):
        assert w[1] == sum(x[1] for x in recs) and w[2] == sum(x[3] == KEPT for x in recs) and w[3] == int(1 <= w[2] <= 3) and [x[0] for x in recs] == sorted({x[0] for x in recs})
        assert all(x[2] >= 20.0 for x in recs) and (not recs or max(x[2] for x in recs) - min(x[2] for x in recs if x[3] == KEPT) <= 20.0)


def bits(n, k=0):
    return -offsets_oracle.table()[n, k] * 10.0 / 6.0


def test_the_table_and_the_bits():
    T = offsets_oracle.table()
    assert T[20, 20] == 0.0 and T[400, 400] == 0.0 and T[19].max() == T[19].min() == 0.0
    assert 20.06 < bits(20) < 20.08 and bits(20, 1) < 20.0 and bits(19) == 0.0 and abs(bits(60) - bits(40) - 20.069) < .001 and abs(bits(60) - bits(41) - 19.066) < .001


def test_acceptable_8mers():
    acc = lambda x: bool(soffsets_oracle.acceptable_kmers(x, 8))
    assert acc([0, 1, 2, 0, 1, 2, 0, 1]) and not acc([0, 0, 0, 0, 1, 2, 3, 1]) and not acc([1, 2, 3, 1, 0, 0, 0, 0]) and not acc([0, 1, 0, 1, 0, 1, 0, 1]) and acc([0, 0, 0, 1, 2, 2, 2, 3])
    assert soffsets_oracle.acceptable_kmers([0, 1, 2, 0, 1, 2, 0, 1, 2], 9) == {(0, 1, 2, 0, 1, 2, 0, 1): [0], (1, 2, 0, 1, 2, 0, 1, 2): [1]} and not soffsets_oracle.acceptable_kmers([0, 1, 2, 3, 0, 1, 2], 7)


@pytest.fixture(scope="module")
def planted():
    name, c = soffsets_cases.seeded()[0]
    assert name == "planted"
    return c, soffsets_cases.oracle(name, c)


def pair(planted, name):
    """-> (the pair's words, its records, its counters, its two consensus elements)"""
    c, (sc, r) = planted
    pi = c["names"][name]
    return r["words"][pi], r["per"][pi], r["per_counts"][pi], sc["elements"][2 * pi:2 * pi + 2]


def test_pairs_that_do_not_yield_and_acceptable_8mers(planted):
    c, (sc, r) = planted
    assert [c["names"][n] for n in ("NONE0", "NONE2")] == [0, r["pairs"] - 1] and 0 < c["names"]["NONE1"] < r["pairs"] - 1 and r["yields"] == r["pairs"] - 3
    for n in ("NONE0", "NONE1", "NONE2"):
        w, recs, k, el = pair(planted, n)
        assert w == (0, 0, 0, 0) and recs == [] and not any(k.values())
    w, recs, k, el = pair(planted, "ACC3")
    assert [e["cols"] for e in el] == [8, 8] and (k["rows"], k["kmers"], k["acceptable"], k["hits"], k["seen"]) == (2, 2, 2, 2, 2) and w == (2, 0, 0, 0)      # offset 0 from s = 0 and from s = 1; 8 columns: no window
    for n in ("FLAT1", "FLAT2", "TWO"):
        w, recs, k, el = pair(planted, n)
        assert (k["kmers"], k["acceptable"], k["hits"], k["seen"]) == (2, 0, 0, 0), n


def test_undefined_cells_and_row_ends(planted):
    w, recs, k, el = pair(planted, "UNDEF")
    assert k["kmers"] == (53 - 8 - 8) + 23 + 53 and k["rows"] == 3 and w[0] == 3 and [x[0] for x in recs] == [0]
    w, recs, k, el = pair(planted, "Q128MID")
    assert recs == [(10, 2, bits(40), KEPT)]                                     # the cell is compared and lies inside the window of all 40
    w, recs, k, el = pair(planted, "Q128END")
    assert recs == [(10, 2, bits(39), KEPT)] and el[1]["cols"] == 40             # the undefined cell is no window's end: 39 at most
    w, recs, k, el = pair(planted, "ALLMIS")
    assert recs == [(0, 2, bits(30), KEPT)] and k["lookups"] > 2 * sum(31 - n + 1 for n in range(20, 31))      # windows inside the 30 mismatching columns were looked up (T[n][n] = 0.0) and changed nothing


def test_offsets_of_either_sign_and_who_proposes_them(planted):
    w, recs, k, el = pair(planted, "ZERO")
    assert recs == [(0, 2, bits(60), KEPT)] and w == (2, 2, 1, 1) and k["hits"] >= 2 * 50 and k["seen"] == 2      # many 8-mers, one ( r, offset ) a side; both sides: two results
    assert pair(planted, "NEGATIVE")[1] == [(-30, 2, bits(40), KEPT)]
    w, recs, k, el = pair(planted, "ONLY1")
    assert recs == [(20, 1, bits(40), KEPT)] and w == (1, 1, 1, 1) and k["rows"] == 4       # stack 0's consensus follows the two rows that agree: only its third row, against stack 1's consensus, finds it
    assert pair(planted, "W27")[1] == [(20, 2, bits(27), KEPT)] and pair(planted, "W27")[3][1]["cols"] == 27
    for n, off in (("W400", 100), ("TRIM0", 240), ("TRIM1", 100)):
        w, recs, k, el = pair(planted, n)
        assert [(x[0], x[2], x[3]) for x in recs] == [(off, bits(100), KEPT)] and w[3] == 1, n
    assert [e["cols"] for e in pair(planted, "W400")[3]] == [400, 400] and pair(planted, "TRIM0")[3][0]["M"] == 460 and pair(planted, "TRIM1")[3][1]["M"] == 460
    c, (sc, r) = planted
    assert any(l[1] < 60 for l in c["recs"][2 * c["names"]["TRIM0"]]["locs"])    # rows that start in front of the window


def test_conflicts_windows_and_the_filter(planted):
    c, (sc, r) = planted
    w, recs, k, el = pair(planted, "CONF9")
    assert sc["counts"][c["names"]["CONF9"]][30 + 100] == 9 and [(x[0], x[1]) for x in recs] == [(30, 6)] and k["disallowed"] == 0
    w, recs, k, el = pair(planted, "CONF10")
    assert sc["counts"][c["names"]["CONF10"]][30 + 100] == 10 and recs == [] and w[0] == 0 and k["disallowed"] == k["hits"] > 0
    assert pair(planted, "PERF19")[0] == (2, 0, 0, 0) and pair(planted, "PERF20X")[0] == (2, 0, 0, 0)
    assert pair(planted, "PERF20")[1] == [(40, 2, bits(20), KEPT)] and pair(planted, "PERF20")[0] == (2, 2, 1, 1)
    w, recs, k, el = pair(planted, "EDGE")
    assert [(x[0], x[2], x[3]) for x in recs] == [(0, bits(60), KEPT), (40, bits(40), DROPPED), (80, bits(41), KEPT)] and w[2:] == (2, 1)
    assert bits(60) - bits(40) > 20.0 >= bits(60) - bits(41)
    w, recs, k, el = pair(planted, "KEPT3")
    assert [x[0] for x in recs] == [0, 30, 60] and w[2:] == (3, 1)
    w, recs, k, el = pair(planted, "KEPT4")
    assert [x[0] for x in recs] == [0, 30, 60, 90] and w[2:] == (4, 0)            # four offsets: not closable
    w, recs, k, el = pair(planted, "ROWS600")
    assert k["rows"] == 601 and [(x[0], x[1] >= 200) for x in recs] == [(8, True), (9, True), (10, True)] and w[0] >= 600
    assert (r["pairs_2"], r["pairs_3"], r["pairs_more"], r["dropped"]) == (1, 2, 1, 1)


def test_the_other_seeded_cases():
    for name, c in soffsets_cases.seeded()[1:]:
        sc, r = soffsets_cases.oracle(name, c)
        if name == "no-pairs": assert r["pairs"] == 0 and r["file"] == b"DFKSOFF1" + bytes(16) and r["starts"] == [0]
        else: assert r["yields"] == r["pairs"] - 1 and r["results"] and r["disallowed"] and r["seen"] > r["results"] and any(x[0] < 0 for x in r["records"]) and any(x[0] > 0 for x in r["records"])
