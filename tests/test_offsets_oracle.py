"""tests/offsets_oracle.py -- GetOffsets1 restated in plain Python -- on the four fixtures that have pairs: the table the two restatements
(this one and superplus_amd/csrc/dfk_offsets.h, held to each other by tests/test_offsets_cpu.py) must reproduce, the file's layout, the
value of the table of log binomial sums against exact fractions, the loops as written against the gathered form, and what each seeded
case fires.  CPU only."""
import math
import struct
from fractions import Fraction

import numpy as np
import pytest

from tests import offsets_cases, offsets_oracle

# fixture, K, reads: pairs, candidates, passed, invalidated, deleted as small, survivors, pairs with 0 / 1 / 2 / more survivors, look-ups
TABLE = [("graph_frag_k48", 48, "frag", (937, 764, 351, 0, 0, 351, 586, 351, 0, 0, 1399355)), ("graph_pathy2_k48", 48, "pathy2", (725, 1026, 38, 0, 0, 38, 687, 38, 0, 0, 5231979)),
         ("graph_pathy_k48", 48, "pathy", (63, 49, 2, 0, 0, 2, 61, 2, 0, 0, 224823)), ("graph_k40_nobc", 40, "reads", (138, 193, 1, 0, 0, 1, 137, 1, 0, 0, 1044376))]
# the largest relative error of the long-double sums against the exact BinomialSum( n, k, 3/4 ), measured over 20 <= n <= 400, k < n: at
# ( 393, 189 ), about 30 units of 2^-64.  The test allows twice that: a sanity bound on the value (a host may order its long double
# operations differently); the pin is the bit-equality of the two tables (tests/test_offsets_cpu.py)
MEASURED_REL_ERROR = 1.6354812281859572e-18


@pytest.mark.parametrize("case,K,which,row", TABLE, ids=[t[0] for t in TABLE])
def test_the_table_on_the_fixtures(golden_dir, case, K, which, row):
    r = offsets_oracle.fixture_offsets(golden_dir, case, K, which)
    assert (r["pairs"], r["candidates"], r["passed"], r["invalidated"], r["deleted_small"], r["survivors"], r["pairs0"], r["pairs1"], r["pairs2"], r["pairs_more"], r["lookups"]) == row
    assert r["closable"] == r["pairs1"] + r["pairs2"] and max(len(s) for s in r["seqs"]) <= offsets_oracle.MAX_N
    # the fixtures never fire invalidation or big near small and never leave more than one survivor: the seeded cases carry those
    n, nr = r["pairs"], r["passed"]
    for p, (g, w, a, b) in enumerate(zip(r["per"], r["words"], r["starts"], r["starts"][1:])):
        assert w == (g["candidates"], len(g["records"]), len(g["survivors"])) and b - a == w[1] and w[2] <= w[1] <= w[0]
        assert [x[0] for x in g["records"]] == sorted(x[0] for x in g["records"]) and all(x[4] >= 25.0 and x[2] == x[0] + len(r["seqs"][2 * p + 1]) for x in g["records"])
    # the file: magic, n, starts, words, records
    f = r["file"]
    assert f[:8] == b"DFKCOFF1" and struct.unpack_from("<Q", f, 8)[0] == n and len(f) == 16 + 8 * (n + 1) + 16 * n + 32 * nr
    assert list(np.frombuffer(f, "<u8", n + 1, 16)) == r["starts"] and struct.unpack_from("<IIII", f, 16 + 8 * (n + 1)) == r["words"][0] + (0,)
    at = 16 + 8 * (n + 1) + 16 * n
    assert struct.unpack_from("<iiiidII", f, at) == r["records"][0] + (0,) and struct.unpack_from("<iiiidII", f, at + 32 * (nr - 1)) == r["records"][-1] + (0,)


def test_the_table_of_log_binomial_sums():
    assert np.finfo(np.longdouble).nmant == 63
    T = offsets_oracle.table()
    assert T.shape == (401, 401) and not T[:20].any() and not np.triu(T, 0)[20:].any()              # the cells k >= n are never written: 0.0, T[n][n] among them
    assert (T <= 0).all() and (T[20:, :10] < 0).all()                                               # (a sum rounds to 1.0 where k nears a large n: log10 gives 0.0 there too)
    assert T[20, 0] == math.log10(0.25 ** 20) and T[400, 0] == math.log10(0.25 ** 400)
    assert abs(T[25, 0] * -10 / 6 - 25 * math.log10(4) * 10 / 6) < 1e-12                            # a perfect overlap of n bases: 1.00343 n bits
    worst = Fraction(0)
    for n in range(20, 401):
        sums = offsets_oracle.binomial_sums(n)
        acc, choose, den = 0, 1, 4 ** n
        for k in range(n):
            acc += choose * 3 ** k
            choose = choose * (n - k) // (k + 1)
            exact = Fraction(acc, den)
            worst = max(worst, abs(Fraction(*sums[k].as_integer_ratio()) - exact) / exact)
    print("largest relative error of the long-double sums: %.6g (measured %.6g)" % (float(worst), MEASURED_REL_ERROR))
    assert float(worst) <= 2 * MEASURED_REL_ERROR


def test_the_loops_as_written_give_what_the_gathered_form_gives():
    T = offsets_oracle.table()
    seeded = {name: seqs for name, seqs, _ in offsets_cases.seeded()}
    for name in ("thresholds", "bad-window", "all-mismatches", "big-near-small-30", "degenerate"):
        seqs = seeded[name]
        for p in range(len(seqs) // 2):
            a, b = offsets_oracle.get_offsets1(seqs[2 * p], seqs[2 * p + 1], T), offsets_oracle.get_offsets1(seqs[2 * p], seqs[2 * p + 1], T, loops=True)
            assert a == b and all(struct.pack("<d", x[4]) == struct.pack("<d", y[4]) for x, y in zip(a["records"], b["records"])), (name, p)


def test_seeded_cases_fire_what_the_fixtures_lack():
    got = {name: offsets_cases.oracle(name, seqs) for name, seqs, _ in offsets_cases.seeded()}
    seqs = {name: s for name, s, _ in offsets_cases.seeded()}
    assert max(len(s) for ss in seqs.values() for s in ss) == 400
    # the thresholds: 24 bases fail (24.08 bits), 25 pass (25.09); the only survivor is the true offset
    t = got["thresholds"]
    assert [[(r[0], r[1]) for r in g["records"]] for g in t["per"]] == [[], [], [], [(100, 25)], [(100, 39)], [(100, 40)]]
    assert [round(g["records"][0][4], 2) for g in t["per"][3:]] == [25.09, 39.13, 40.14]
    # the near-repeat: three offsets pass and offset 0 invalidates +-150
    assert [(r[0], r[5]) for r in got["near-repeat"]["records"]] == [(-150, 1), (0, 0), (150, 1)]
    # the tandem repeat: 49 candidates, 45 pass, none is removed (a perfect slope is 1.003 < 2): more than two survivors
    assert (got["tandem"]["candidates"], got["tandem"]["passed"], got["tandem"]["survivors"], got["tandem"]["pairs_more"]) == (49, 45, 45, 1)
    # big near small: 39 bases are not saved, 40 are
    b = {L: got[f"big-near-small-{L}"] for L in offsets_cases.STRETCHES}
    assert [(b[L]["passed"], b[L]["deleted_small"], b[L]["survivors"], b[L]["invalidated"]) for L in offsets_cases.STRETCHES] == [(5, 4, 1, 0), (11, 10, 1, 0), (19, 14, 5, 0), (25, 14, 11, 0)]
    assert [(r[0], round(r[4], 2)) for r in b[44]["records"] if r[5] == 0] == [(-4, 40.14), (-2, 42.14), (0, 246.67), (2, 42.14), (4, 40.14)]
    assert max(r[4] for r in b[44]["records"] if r[5] == 2) < 40.0
    # a bad window cuts the n loops short; a window of nothing but mismatches reads T[n][n]
    s1, s2 = seqs["bad-window"]
    se, bw = offsets_oracle.windows(s1, s2, 0, 300, 300)
    assert any(bw) and got["bad-window"]["lookups"] < sum(300 - s - 19 for s in range(281)) and got["bad-window"]["survivors"] == 1
    s1, s2 = seqs["all-mismatches"]
    se, bw = offsets_oracle.windows(s1, s2, 0, 120, 120)
    assert se[70] - se[50] == 20 and not any(bw[:11]) and got["all-mismatches"]["survivors"] == 1          # start 50, n 20: k == n, and no break before n = 50
    # the homopolymer: 31 pass and 30 are invalidated
    assert (got["homopolymer"]["passed"], got["homopolymer"]["invalidated"], got["homopolymer"]["survivors"]) == (31, 30, 1)
    # the degenerate shapes
    d = got["degenerate"]
    assert [w[0] for w in d["words"][:5]] == [0, 0, 0, 0, 0]                                          # lengths 0 and 7: no 8-mer
    assert d["words"][5] == (1, 0, 0)                                                                 # two identical 8-mers: a candidate with overlap 8 that fails
    assert [(r[0], r[1], r[3]) for r in d["per"][6]["records"]] == [(0, 400, 0)]                      # identical 400-mers
    assert [g["survivors"] for g in d["per"][7:11]] == [[60], [-60], [50], [-50]]                     # positive, negative, n1 != n2
    assert d["per"][11]["survivors"] == [-100] and d["per"][11]["records"][0][1] == 30 and d["per"][12]["survivors"] == [] and d["per"][12]["candidates"] >= 1
    assert d["per"][13]["survivors"] == [-100, 0] and d["pairs2"] == 1
    assert got["no-pairs"]["file"] == b"DFKCOFF1" + bytes(16)
    assert got["many"]["pairs"] == 4200 > 2 * 2048 and got["many"]["passed"] > 0 and got["many"]["pairs0"] > 0
    assert [w[1] >= 45 for w in got["busy"]["words"]] == [False, True, False, False] and got["busy"]["invalidated"] > 0
    assert got["random"]["deleted_small"] > 0 and got["random"]["pairs0"] > 0
