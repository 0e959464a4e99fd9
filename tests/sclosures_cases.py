"""Seeded inputs of Stackster's closures (tests/sclosures_oracle.py): reads, qualities and the walks' tables chosen directly, as
tests/soffsets_cases.py does (its Case is built on by import), with the dims tests/scons_oracle.py makes of them and the offsets GIVEN
BY HAND as a.stack.offsets records -- so a plant need not reach 20 bits -- for tests/cpp/test_sclosures.cc (recorded in
tests/cpp/sclosures_cases.txt: the C++ restatement of superplus_amd/csrc/dfk_sclosures.h against the Python one) and for
tests/test_gpu_sclosures.py (dfk_sclosures_build_arrays).  `python -m tests.sclosures_cases` rewrites the recorded file.

A PLANT is a pair given as the two stacks AS THEY STAND AFTER Reverse (soffsets_cases.Case.plant) and its records ( offset, state ).
`planted` holds, by plant name (`names`: the pair's index); tests/test_sclosures_oracle.py asserts what each is there for:
   NONE0 NONE1 NONE2   pairs that do not yield: the first, one in the middle, the last.
   POS ZERO NEG   offset +20, 0, -30 with n1 != n2 and no edge trim of the other stack; NEG trims stack 1 on the left.
   RTRIM LTRIM   n1 > offset + n2: stack 0 is trimmed on the right, a row lying wholly beyond is erased and one that reaches 5 columns in
             stays; the same on the left for stack 1 at a negative offset.
   QEDGE0 QEDGE1   a row whose only cells inside the window have quality 128, 190, 128: erased although its span meets the window
             (stack 0's right edge, stack 1's left edge).
   TWO THREE FOUR NOKEPT DROPMID   2 and 3 kept offsets (2 and 3 closures, ascending); 4: none; one dropped record alone: none; a dropped
             record between two kept ones: two closures.
   COLS      stack 0 two rows, stack 1 four, 40 and 48 columns at offset 0; the chosen columns (`COLS_AT`): ORDER (A: 20 from stack 0 then
             0.1, 0.1 from stack 1 = 20.200000000000003; C: 0.2 then 10, 10 = 20.2: A wins, per-stack sums would tie and C would win),
             TIE (A 30 from stack 0 against C 30 from stack 1, G 6, T 0.4: the higher of the two), Q12 (A Q1 + Q0 against C Q2 + Q0:
             0.30000000000000004 each, C), Q00 (A Q0 + Q0, C Q2, T Q0 + Q0: 0.2 each, T), GAP (columns nothing covers: base 3).
   HOMO20 HOMO19   a read with a homopolymer of 20 / 19 at stored quality 40 against a row of quality 30 on another base: lowered to 5
             the run loses the column, with 19 it is not lowered and wins.
   C8 C256 C257 C792 W460   merged widths 8 (two stacks of 8, one row each), 256 and 257 (the tile edge), 792 (two stacks of 400 at
             offset 392: four tiles, the last with 24 columns); both stacks 460 wide before their Trim, rows that start in front of the
             window.
   TWICE BOTH   a read in two rows of one stack, once with each flag; a read in both stacks.
   ROWS600   600 rows a stack (more than one staging chunk).
   SKIPALL   stack 1 is 400 wide and its rows stand in its output columns [0, 100) alone: in the tile of merged columns [512, 600)
             every row of stack 1 misses the tile.
   ROWLESS   offset -42 between a stack 0 whose one row stands at [50, 110) and a stack 1 whose one row stands at output columns [0, 30)
             of 50: the window is the 8 merged columns [0, 8), both rows lie outside it and are erased.  It can be planted without any
             quality of 128: the edge trims alone erase the rows.  Expected: 8 columns of base 3, rows 0, rowless 1.
The second case is soffsets_cases' own `planted` set with the offsets its oracle finds (EDGE: two closures, KEPT3: three, KEPT4: none),
the third its random case with offsets drawn by hand from the allowed range, the fourth has no pairs at all.
Qualities: feudal.pq_encode holds a block's least quality in six bits: 128 and 190 stand in a block with a 63."""
import os

import numpy as np

from tests import scons_cases, scons_oracle, sclosures_oracle, soffsets_cases
from tests.soffsets_oracle import DROPPED, KEPT
from tests.walks_cases import genome, rc

FILE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "cpp", "sclosures_cases.txt")
K = scons_cases.K
COLS_AT = dict(ORDER=5, TIE=9, Q12=13, Q00=17, GAP=(24, 29))


class Case(soffsets_cases.Case):
    def __init__(self, seed):
        super().__init__(seed)
        self.so_per = []

    def pair(self, name, locs0, locs1=None, status=(0, 0), offs=()):
        super().pair(name, locs0, locs1, status)
        self.so_per.append([(int(o), 1, 20.0 + i, int(st)) for i, (o, st) in enumerate(offs)])

    def plant(self, name, rows0, rows1, offs):
        self.pair(name, self.side0(rows0), self.side1(rows1), offs=offs)

    def done(self):
        return dict(super().done(), so_per=self.so_per)


def cols_rows(c):
    """COLS: the two stacks as rows ( bases, qualities, column, flag )"""
    g = genome(c.rng, 48)
    A, C_ = 0, 1
    g[[COLS_AT[k] for k in ("ORDER", "TIE", "Q12", "Q00")]] = 2
    B0 = np.tile(g[:40], (2, 1)); Q0 = np.full((2, 40), 40, np.uint8)
    B1 = np.tile(g, (4, 1)); Q1 = np.full((4, 48), 40, np.uint8)
    spec0 = dict(ORDER=[(A, 20), (C_, 1)], TIE=[(A, 30), (2, 3)], Q12=[(A, 1), (A, 0)], Q00=[(A, 0), (A, 0)])
    spec1 = dict(ORDER=[(A, 0), (A, 0), (C_, 10), (C_, 10)], TIE=[(C_, 30), (2, 3), (3, 2), (3, 2)], Q12=[(C_, 2), (C_, 0), (2, 0), (3, 0)], Q00=[(C_, 2), (2, 0), (3, 0), (3, 0)])
    for name in spec0:
        col = COLS_AT[name]
        for r, (b, q) in enumerate(spec0[name]): B0[r, col] = b; Q0[r, col] = q
        for r, (b, q) in enumerate(spec1[name]): B1[r, col] = b; Q1[r, col] = q
    lo, hi = COLS_AT["GAP"]
    rows0 = [(B0[r, :lo], Q0[r, :lo], 0, True) for r in range(2)] + [(B0[r, hi:], Q0[r, hi:], hi, r == 0) for r in range(2)]
    rows1 = [(B1[r, :lo], Q1[r, :lo], 0, r % 2 == 0) for r in range(4)] + [(B1[r, hi:], Q1[r, hi:], hi, True) for r in range(4)]
    return rows0, rows1


def homo(c, n):
    """a run of n A's in a read of 60 at Q40 on stack 0; on stack 1 the same columns with a C in the middle of the run at Q30"""
    g = genome(c.rng, 60)
    g[10:10 + n] = 0; g[9] = 1; g[10 + n] = 2
    h = g.copy(); h[15] = 1
    q = np.full(60, 30, np.uint8)
    return [(g, 40, 0, True)], [(h, q, 0, True)]


def planted():
    c = Case(31)
    rng = c.rng
    one = lambda seq, a=0, q=40: [(seq, q, a, True)]
    c.pair("NONE0", c.filler(), [])
    g = genome(rng, 100)
    c.plant("POS", c.tiles(g[:60], length=40, step=20), c.tiles(g[20:90], length=40, step=15), [(20, KEPT)])
    c.plant("ZERO", one(g[:50]), c.tiles(g[:60], length=40, step=20), [(0, KEPT)])
    c.plant("NEG", one(g[30:70]), c.tiles(g[:70], length=40, step=15), [(-30, KEPT)])
    g = genome(rng, 100)
    c.plant("RTRIM", c.tiles(g, length=60, step=40) + [(g[70:100], 40, 70, True), (g[55:95], 40, 55, False)], one(g[10:60]), [(10, KEPT)])
    c.plant("LTRIM", one(g[40:100]), c.tiles(g, length=60, step=40) + [(g[0:25], 40, 0, True), (g[5:45], 40, 5, False)], [(-40, KEPT)])
    edge = np.array([128, 190, 128, 63] + [40] * 36, np.uint8)
    c.plant("QEDGE0", c.tiles(g, length=60, step=40) + [(g[57:97], edge, 57, True)], one(g[10:60]), [(10, KEPT)])
    c.pair("NONE1", [], [], status=(0, 1))
    c.plant("QEDGE1", one(g[40:100]), c.tiles(g, length=60, step=40) + [(g[3:43], edge[::-1], 3, True)], [(-40, KEPT)])
    g = genome(rng, 120)
    two = lambda: (c.tiles(g[:80], length=50, step=30), c.tiles(g[10:70], length=50, step=10))
    c.plant("TWO", *two(), [(0, KEPT), (12, KEPT)])
    c.plant("THREE", *two(), [(-5, KEPT), (3, KEPT), (20, KEPT)])
    c.plant("FOUR", *two(), [(-5, KEPT), (3, KEPT), (20, KEPT), (21, KEPT)])
    c.plant("NOKEPT", *two(), [(5, DROPPED)])
    c.plant("DROPMID", *two(), [(0, KEPT), (7, DROPPED), (15, KEPT)])
    c.plant("COLS", *cols_rows(c), [(0, KEPT)])
    c.plant("HOMO20", *homo(c, 20), [(0, KEPT)])
    c.plant("HOMO19", *homo(c, 19), [(0, KEPT)])
    g = genome(rng, 8)
    c.plant("C8", one(g), one(g, q=30), [(0, KEPT)])
    g = genome(rng, 800)
    c.plant("C256", c.tiles(g[:200]), c.tiles(g[56:256]), [(56, KEPT)])
    c.plant("C257", c.tiles(g[:199]), c.tiles(g[57:257]), [(57, KEPT)])
    c.plant("C792", c.tiles(g[:400]), c.tiles(g[392:792]), [(392, KEPT)])
    g = genome(rng, 800)
    c.plant("W460", c.tiles(g[:460]), c.tiles(g[300:760]), [(240, KEPT)])        # the windows show g[60:460] and g[300:700]
    tw = c.row(genome(rng, 90), rng.choice(np.array([0, 2, 10, 37, 41], np.uint8), size=90), 0)
    c.pair("TWICE", [tw, (tw[0], 5, False)], c.side1(one(genome(rng, 70))), offs=[(12, KEPT)])
    both = c.row(genome(rng, 80), 37, 0)
    c.pair("BOTH", [both, c.row(genome(rng, 50), 20, 10)], [(both[0], 4, True), c.row(genome(rng, 84), 30, 0)], offs=[(-9, KEPT), (30, KEPT)])
    g = genome(rng, 80)
    i0, i1 = c.read(g[:60], 40), c.read(rc(g[10:70]), 37)
    c.pair("ROWS600", [(i0, i % 4, i % 5 != 0) for i in range(600)], [(i1, i % 3, True) for i in range(600)], offs=[(10, KEPT)])
    g = genome(rng, 600)
    c.pair("SKIPALL", c.side0(c.tiles(g[:400])), [c.row(rc(g[200:300]), 40, 300), c.row(rc(g[210:290]), 30, 310, fw=False)], offs=[(200, KEPT)])
    g, h = genome(rng, 60), genome(rng, 30)
    c.pair("ROWLESS", [c.row(g, 40, 50)], [c.row(rc(h), 40, 20)], offs=[(-42, KEPT)])
    c.pair("NONE2", c.filler(), [])
    return c.done()


def from_soffsets(name):
    """a case of soffsets_cases with the records its oracle finds"""
    c = dict(soffsets_cases.seeded())[name]
    return dict(c, so_per=[list(p) for p in soffsets_cases.oracle(name, c)[1]["per"]])


def random_offsets(seed=11):
    """soffsets_cases' random case with one to four records a yielding pair, drawn from the allowed range, some of them dropped"""
    name = "random"
    c = dict(soffsets_cases.seeded())[name]
    sc = soffsets_cases.oracle(name, c)[0]
    rng = np.random.RandomState(seed)
    per = []
    for pi in range(len(c["recs"]) // 2):
        n1, n2 = sc["elements"][2 * pi]["cols"], sc["elements"][2 * pi + 1]["cols"]
        if not scons_oracle.yields(c["recs"][2 * pi], c["recs"][2 * pi + 1]) or n1 < 8 or n2 < 8:
            per.append([])
            continue
        offs = sorted(set(int(x) for x in rng.randint(-(n2 - 8), n1 - 8 + 1, size=1 + pi % 4)))
        per.append([(o, 1, 25.0, DROPPED if (pi + i) % 5 == 4 else KEPT) for i, o in enumerate(offs)])
    return dict(c, so_per=per)


def no_pairs():
    return dict(soffsets_cases.no_pairs(), so_per=[])


_made = {}


def seeded():
    """[(name, case)]"""
    if not _made:
        _made["planted"] = planted(); _made["soffsets-planted"] = from_soffsets("planted"); _made["random"] = random_offsets(); _made["no-pairs"] = no_pairs()
    return list(_made.items())


_oracle = {}


def oracle(name, c):
    """-> (scons_oracle.run's result, sclosures_oracle.run's)"""
    if name not in _oracle:
        sc = scons_oracle.run(c["recs"], lambda id: c["reads"][id], lambda id: c["quals"][id])
        _oracle[name] = (sc, sclosures_oracle.run(c["recs"], lambda id: c["reads"][id], lambda id: c["quals"][id], c["K"], c["so_per"]))
    return _oracle[name]


def words_of(so_per):
    kept = [sum(r[3] == KEPT for r in p) for p in so_per]
    return [(len(p), sum(r[1] for r in p), k, int(1 <= k <= 3)) for p, k in zip(so_per, kept)]


def arrays(name, c):
    """the case as dfk_sclosures_build_arrays takes it"""
    from superplus_amd.dfk import SOFFSETS_RECORD
    a = scons_cases.arrays(c)
    sc = oracle(name, c)[0]
    recs = [r for p in c["so_per"] for r in p]
    so = np.zeros(len(recs), SOFFSETS_RECORD)
    for i, (o, n, b, st) in enumerate(recs): so[i] = (o, n, b, st, 0)
    a.update(dims=np.asarray([w for e in sc["elements"] for w in scons_oracle.dim_words(e)], np.uint32).reshape(-1, 4),
             so_starts=np.concatenate([[0], np.cumsum([len(p) for p in c["so_per"]])]).astype(np.uint64), so_words=np.asarray(words_of(c["so_per"]), np.uint32).reshape(-1, 4), so_records=so)
    return a


def result_text(c, r):
    """the offsets and what the oracle says, as tests/cpp/test_sclosures.cc reads them"""
    row = lambda v: " ".join(str(int(x)) for x in v) or "-"
    return [row([x for w in words_of(c["so_per"]) for x in w]), " ".join("%d %d %s %d" % (o, n, np.float64(b).tobytes().hex(), st) for p in c["so_per"] for o, n, b, st in p) or "-",
            row([x for rec in r["records"] for x in rec]), "".join(str(int(b)) for b in r["bases"]) or "-", row([r[k] for k in sclosures_oracle.COUNTS])]


def case_text(name, c, sc, r):
    """a case and what the oracles say of it: scons_cases' lines with K behind the header, the records a pair, result_text's"""
    t = scons_cases.case_text(name, c, sc)
    return [t[0] + " %d" % c["K"]] + t[1:] + [" ".join(str(len(p)) for p in c["so_per"]) or "-"] + result_text(c, r)


def text():
    out = []
    for name, c in seeded(): out += case_text(name, c, *oracle(name, c))
    return "\n".join(out) + "\n"


if __name__ == "__main__":
    open(FILE, "w").write(text())
