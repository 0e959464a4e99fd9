"""Seeded inputs of Stackster's stack offsets (tests/soffsets_oracle.py): reads, qualities and the walks' tables chosen directly, as
tests/scons_cases.py does, with the stack consensus tests/scons_oracle.py makes of them -- for tests/cpp/test_soffsets.cc (recorded in
tests/cpp/soffsets_cases.txt: the C++ restatement of superplus_amd/csrc/dfk_soffsets.h against the Python one) and for
tests/test_gpu_soffsets.py (dfk_soffsets_build_arrays).  `python -m tests.soffsets_cases` rewrites the recorded file.

A PLANT is a pair given as the two stacks AS THEY STAND AFTER Reverse: rows ( bases, qualities, column, flag ); side 1's reads are
stored so that the stage's orientation and Reverse show those bases there.  Stack 0's column i shows genome position i + A0, stack 1's
column i genome position i + A1: the true offset is A1 - A0.  A perfect overlap of n columns has n log10( 4 ) 10 / 6 = 1.00343 n bits.
`planted` holds, by plant name (`names`: the pair's index); tests/test_soffsets_oracle.py asserts what each is there for:
   NONE0 NONE1 NONE2   pairs that do not yield: the first, one in the middle, the last.
   ACC3 FLAT1 FLAT2 TWO   both stacks 8 columns wide, one 8-mer: exactly 3 distinct bases (acceptable: seen from both s, offset 0 twice);
             the first half flat only, the second half flat only, two distinct bases (each rejected: nothing seen).
   UNDEF     a row with quality 128 at column 30 and 190 at column 45 (8-mers over them are not defined) and a row of 30 columns in a
             stack of 60 (the 8-mers that hang over its end are not defined): 37 + 23 row 8-mers from stack 1, 53 from stack 0.
   ZERO NEGATIVE   offsets 0 and -30 (every other plant's is positive); ZERO: the same ( r, offset ) proposed by 53 8-mers, seen once.
   ONLY1     stack 0's consensus is outvoted away from the one row that matches stack 1: the offset is proposed from s = 1 alone.
   CONF9 CONF10   two stacks of 100 columns with conq 100 that agree at offset 30 but for 9 / 10 columns: allowed / every hit skipped.
   PERF19 PERF20 PERF20X   a row overlap of 19 (no window: 0 bits), of 20 (20.07 bits: a result from either s), of 20 with a mismatch
             (17.1 bits: none).
   ALLMIS    a row whose last 30 columns all differ from the consensus: the windows inside them read T[n][n] = 0.0.  (A window's end
             cells are defined, so they lie in the row's span and every cell between them holds a base: a ' ' cell is never inside
             a window, only in the prefix sums around it.)
   Q128MID Q128END   quality 128 in the middle of a row of 40 (the whole 40 is a window: 40.14 bits from s = 0) and at its last column
             (the longest window is 39).
   W27 W400 TRIM0 TRIM1   n1 != n2 everywhere; a stack of 27 columns; two of 400; stack 0 / stack 1 460 wide before Trim, rows that
             start at negative columns of the window.
   EDGE      row overlaps of 60, 40 and 41 at offsets 0, 40, 80: best 60.21; 40.14 is 20.07 below (dropped), 41.14 is 19.07 below (kept).
   KEPT3 KEPT4   three / four offsets with 50 columns each: closable / not.
   ROWS600   a stack of 600 rows (ACC3 has stacks of 1).
Qualities: feudal.pq_encode holds a block's least quality in six bits: 128 stands beside a 41 and 190 beside a 63 that their block can hold them with."""
import os

import numpy as np

from tests import scons_cases, scons_oracle, soffsets_oracle
from tests.walks_cases import genome, rc

FILE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "cpp", "soffsets_cases.txt")
K = scons_cases.K


class Case(scons_cases.Case):
    def side0(self, rows):
        return [self.row(b, q, a, fw) for b, q, a, fw in rows]

    def side1(self, rows):
        """rows in the columns Reverse leaves them in; the stack is as wide as they reach"""
        cols = max(a + len(b) for b, q, a, fw in rows)
        assert min(a for b, q, a, fw in rows) == 0                                # M is then `cols`
        return [self.row(rc(b), q if np.isscalar(q) else np.asarray(q, np.uint8)[::-1], cols - a - len(b), fw) for b, q, a, fw in rows]

    def tiles(self, seq, step=50, length=100):
        """( bases, 40, column, flag ) rows that show `seq` from column 0 to its end"""
        rows, a = [], 0
        while True:
            b = min(len(seq), a + length)
            rows.append((seq[a:b], 40, a, len(rows) % 3 != 1))
            if b == len(seq): return rows
            a += step

    def plant(self, name, rows0, rows1):
        self.pair(name, self.side0(rows0), self.side1(rows1))


def planted():
    c = Case(23)
    rng = c.rng
    one = lambda seq, a=0: [(seq, 40, a, True)]
    c.pair("NONE0", c.filler(), [])
    for name, x in (("ACC3", [0, 1, 2, 0, 1, 2, 0, 1]), ("FLAT1", [0, 0, 0, 0, 1, 2, 3, 1]), ("FLAT2", [1, 2, 3, 1, 0, 0, 0, 0]), ("TWO", [0, 1, 0, 1, 0, 1, 0, 1])):
        c.plant(name, one(np.asarray(x, np.uint8)), one(np.asarray(x, np.uint8)))
    g = genome(rng, 60)
    q = np.full(60, 40, np.uint8); q[30] = 128; q[31] = 41; q[45] = 190; q[46] = 63
    c.plant("UNDEF", one(g), [(g, q, 0, True), (g[:30], 40, 0, True)])
    g = genome(rng, 60)
    c.plant("ZERO", one(g), one(g))
    g = genome(rng, 100)
    c.plant("NEGATIVE", one(g[30:90]), one(g[0:70]))
    g, h = genome(rng, 60), genome(rng, 60)
    c.plant("ONLY1", [(h, 40, 0, True), (h, 40, 0, False), (g, 40, 0, True)], one(g[20:60]))
    c.pair("NONE1", [], [], status=(0, 1))
    for k in (9, 10):
        gc = genome(rng, 130)
        t1, t2 = gc[:100].copy(), gc[30:130].copy()
        for x in range(k): t1[33 + 5 * x] = (t1[33 + 5 * x] + 1) % 4
        c.plant("CONF%d" % k, [(t1, 40, 0, True)] * 3, [(t2, 40, 0, True)] * 3)
    g = genome(rng, 60)
    c.plant("PERF19", one(g), one(g[41:60]))
    g = genome(rng, 60)
    c.plant("PERF20", one(g), one(g[40:60]))
    g = genome(rng, 60)
    x = g[40:60].copy(); x[10] = (x[10] + 1) % 4
    c.plant("PERF20X", one(g), one(x))
    g = genome(rng, 60)
    x = g.copy(); x[30:] = (x[30:] + 1) % 4
    c.plant("ALLMIS", one(g), one(x))
    g = genome(rng, 60)
    q = np.full(40, 40, np.uint8); q[20] = 128; q[21] = 41
    c.plant("Q128MID", one(g), [(g[10:50], q, 0, True)])
    g = genome(rng, 60)
    q = np.full(40, 40, np.uint8); q[38] = 41; q[39] = 128
    c.plant("Q128END", one(g), [(g[10:50], q, 0, True)])
    g = genome(rng, 60)
    c.plant("W27", one(g), one(g[20:47]))
    g = genome(rng, 500)
    c.plant("W400", c.tiles(g[:400]), c.tiles(g[100:500]))
    g = genome(rng, 460)
    c.plant("TRIM0", c.tiles(g), c.tiles(g[300:420]))                          # the window shows g[60:460]: offset 240
    g = genome(rng, 560)
    c.plant("TRIM1", c.tiles(g[:200]), c.tiles(g[100:560]))                    # the window shows g[100:500]: offset 100
    g = genome(rng, 250)
    for at, cyc in ((60, (0, 1, 2)), (100, (1, 2, 0)), (150, (2, 0, 1)), (190, (0, 2, 1))):      # no base 3 beside the overlaps: an uncovered column of stack 1 (base 3) extends none
        g[at:at + 10] = [cyc[i % 3] for i in range(10)]
    c.plant("EDGE", c.tiles(g), [(g[0:60], 40, 0, True), (g[110:150], 40, 70, True), (g[200:241], 40, 120, True)])
    for n in (3, 4):
        g = genome(rng, 320)
        c.plant("KEPT%d" % n, c.tiles(g), [(g[90 * i:90 * i + 50], 40, 60 * i, True) for i in range(n)])
    g = genome(rng, 80)
    id = c.read(rc(g[10:70]), 40)                                              # one read in 600 rows: columns 0, 1, 2 after Reverse
    c.pair("ROWS600", c.side0(one(g)), [(id, i % 3, True) for i in range(600)])
    c.pair("NONE2", c.filler(), [])
    return c.done()


def random_case(seed, n_pairs=6):
    c = Case(seed)
    rng = c.rng
    quals = np.array([0, 1, 2, 10, 20, 30, 37, 41, 60], np.uint8)
    for p in range(n_pairs):
        G = genome(rng, 1200)
        if rng.rand() < .5: G[140:140 + int(rng.choice([9, 10, 25]))] = rng.randint(4)
        sides = []
        for s in range(2):
            width, at = int(rng.choice([60, 150, 300, 420])), int(rng.randint(0, 200))
            rows = []
            for i in range(int(rng.randint(1, 25))):
                n = int(rng.choice([48, 60, 100, 151]))
                n = min(n, width)
                a = 0 if i == 0 else int(rng.randint(0, width - n + 1))
                b = G[at + a:at + a + n].copy()
                for x in np.nonzero(rng.rand(n) < .03)[0]: b[x] = rng.randint(4)
                rows.append((b, rng.choice(quals, size=n), a, bool(rng.randint(2))))
            sides.append(rows)
        if p == 3: c.pair("R%d" % p, c.side0(sides[0]), [])
        else: c.plant("R%d" % p, sides[0], sides[1])
    return c.done()


def no_pairs():
    c = Case(41)
    c.read(genome(c.rng, 80), 30)
    return c.done()


_made = {}


def seeded():
    """[(name, case)]"""
    if not _made:
        _made["planted"] = planted(); _made["random"] = random_case(5); _made["no-pairs"] = no_pairs()
    return list(_made.items())


_oracle = {}


def oracle(name, c):
    """-> (scons_oracle.run's result, soffsets_oracle.run's)"""
    if name not in _oracle:
        sc = scons_oracle.run(c["recs"], lambda id: c["reads"][id], lambda id: c["quals"][id])
        _oracle[name] = (sc, soffsets_oracle.run(c["recs"], lambda id: c["reads"][id], lambda id: c["quals"][id], sc))
    return _oracle[name]


def cons_arrays(sc):
    """a stack consensus as dfk_scons_fetch gives it"""
    el = sc["elements"]
    return dict(cons_starts=np.concatenate([[0], np.cumsum([e["cols"] for e in el])]).astype(np.uint64), dims=np.asarray([w for e in el for w in scons_oracle.dim_words(e)], np.uint32).reshape(-1, 4),
                con=np.asarray([b for e in el for b in e["con"]], np.uint8), conq=np.asarray([q for e in el for q in e["conq"]], np.uint8),
                conflict_first=np.concatenate([[0], np.cumsum([len(t) for t in sc["counts"]])]).astype(np.uint64), counts=np.asarray([x for t in sc["counts"] for x in t], np.uint16))


def arrays(name, c):
    """the case as dfk_soffsets_build_arrays takes it"""
    a = scons_cases.arrays(c)
    a.update(cons_arrays(oracle(name, c)[0]))
    return a


def result_text(r):
    """what the oracle says, as tests/cpp/test_soffsets.cc reads it: the words, the records (best_bits as its 8 bytes), the counters"""
    row = lambda v: " ".join(str(int(x)) for x in v) or "-"
    return [row([x for w in r["words"] for x in w]), " ".join("%d %d %s %d" % (o, n, np.float64(b).tobytes().hex(), st) for o, n, b, st in r["records"]) or "-",
            row([r[k] for k in soffsets_oracle.COUNTS])]


def text():
    out = []
    for name, c in seeded():
        sc, so = oracle(name, c)
        out += scons_cases.case_text(name, c, sc) + result_text(so)
    return "\n".join(out) + "\n"


if __name__ == "__main__":
    open(FILE, "w").write(text())
