"""Seeded inputs of Stackster's stack consensus (tests/scons_oracle.py): reads, qualities and the walks' tables -- per pair and side the
placed records ( id, start, fw ), M and trim -- chosen directly, for tests/cpp/test_scons.cc (recorded in tests/cpp/scons_cases.txt: the
C++ restatement of superplus_amd/csrc/dfk_scons.h against the Python one) and for tests/test_gpu_scons.py (dfk_scons_build_arrays).
`python -m tests.scons_cases` rewrites the recorded file.

The stage takes the walks as dfk_walks_fetch gives them, so a case writes them itself: a PLANT is a stack given as rows ( oriented
bases, oriented qualities, start, flag ); the read is stored so that the stage's orientation ( reverse-complemented iff the flag is
false ) shows those bases.  A plant stands on side 0 beside a FILLER stack on side 1 unless it says otherwise.  `planted` holds, by
plant name (`names`: the pair's index):
   M48 M255 M256 M257 M400 M401 M460   a stack so wide, three rows deep: 256 is the tile's edge, 400 / 401 the trim's; M460 also holds a
             row that ends exactly at M - 400 (erased by Trim) and one that reaches one column into the window (kept).
   NEG       a row with start -7.           TWICE   one read in two rows, once with each flag.
   LIVE1 LIVE255 LIVE256 LIVE257 LIVE600   so many rows over one span, qualities 0, 1, 2, 40 and 3 in turn: the staging chunk of 256.
   COLS      eight rows over 80 columns, a chosen column each (`COLS_AT`): ORDER (20, Q0, Q0 on one base against Q1, 10, 10 on another),
             HALF (a difference of 9.5), BELOW (9.499999999999998), D994 D995 D100 D300 (99.4, 99.5, 100, 299.8), V100 (val(1) exactly
             100 with two rows of Q50), V1001 (100.1: recount), ONE30 (val(1) 103, one row of Q >= 30), TWO30 (113, two rows), Q29 Q30 (four
             rows of 29 / 30 on the second base), TIE (second and third base both 120: id(1) is the higher, with one row >= 30; the
             lower has two), Q128 (a quality of 128 and one of 190: undefined cells).
   COLS1     the same stack on side 1 (reversed), beside M460's on side 0.
   GAP5 GAP10   two reads that leave 5 / 10 columns uncovered: base 3, conq 0; ten of them are a flat run.
   RUN9 RUN10 RUN255 RUNEND   a run of 9 / 10 equal bases in the consensus, a run of 10 over columns 251-260, one that ends at the last
             column.
   CONF+9 CONF+10 CONF-9 CONF-10 CONF0-9 CONF0-10   two stacks of 100 columns with conq 100 throughout that agree at offset +30 / -30 / 0
             but for 9 / 10 columns.
   SIDE1NONE  side 1 placed nobody; STATUS1: side 0 placed nobody, side 1 not walked; STATUS2: side 0's edge was short.
Qualities: feudal.pq_encode holds a block's least quality in six bits: a run of one quality above 63 does not fit; the cases keep such
values single."""
import os

import numpy as np

from tests import scons_oracle, walks_oracle
from tests.partners_cases import pack
from tests.walks_cases import genome, pq_of, rc

FILE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "cpp", "scons_cases.txt")
K = 48
COLS_AT = dict(ORDER=5, HALF=9, BELOW=13, D994=17, D995=21, D100=25, D300=29, V100=33, V1001=37, ONE30=41, TWO30=45, Q29=49, Q30=53, TIE=57, Q128=70)


class Case:
    def __init__(self, seed):
        self.rng = np.random.RandomState(seed)
        self.reads, self.quals, self.recs, self.names = [], [], [], {}

    def read(self, bases, q):
        bases = np.asarray(bases, np.uint8)
        self.reads.append(bases); self.quals.append(np.full(len(bases), q, np.uint8) if np.isscalar(q) else np.asarray(q, np.uint8))
        assert len(self.reads[-1]) == len(self.quals[-1])
        return len(self.reads) - 1

    def row(self, bases, q, start, fw=True):
        """a row showing `bases` / `q` at `start` -> ( id, start, fw )"""
        q = np.full(len(bases), q, np.uint8) if np.isscalar(q) else np.asarray(q, np.uint8)
        return (self.read(bases, q) if fw else self.read(rc(bases), q[::-1]), int(start), bool(fw))

    def rec(self, locs, status=walks_oracle.WALKED):
        M = max([0] + [s + len(self.reads[id]) for id, s, fw in locs])
        return dict(status=status, entries=len(locs) + 1, placed=len(locs), dup_steps=0, nE=100, nEE=0, M=M, trim=max(0, M - 400), locs=list(locs), EE=[])

    def pair(self, name, locs0, locs1=None, status=(0, 0)):
        if locs1 is None: locs1 = self.filler()
        self.names[name] = len(self.recs) // 2
        self.recs += [self.rec(locs0, status[0]), self.rec(locs1, status[1])]

    def filler(self):
        g = genome(self.rng, 60)
        return [self.row(g, 40, 0)]

    def tiled(self, seq, depth=3, q=40, step=50, length=100):
        """rows that show `seq` from column 0 to its end, `depth` deep"""
        rows = []
        for d in range(depth):
            a = 0
            while True:
                b = min(len(seq), a + length)
                rows.append(self.row(seq[a:b], q, a, fw=(len(rows) % 3 != 1)))
                if b == len(seq): break
                a += step
        return rows

    def done(self):
        return dict(recs=self.recs, reads=self.reads, quals=self.quals, names=self.names, K=K)


def cols_stack(c, side):
    """COLS: eight rows at start 0 over 80 columns; the rows agree on a genome at Q40 but in the chosen columns"""
    g = genome(c.rng, 80)
    B = np.tile(g, (8, 1)); Q = np.full((8, 80), 40, np.uint8)
    A, C_, G, T = 0, 1, 2, 3
    spec = dict(ORDER=[(A, 20), (A, 0), (A, 0), (C_, 1), (C_, 10), (C_, 10)], HALF=[(A, 5), (A, 5), (C_, 1), (C_, 1), (C_, 0)], BELOW=[(A, 10), (A, 0), (A, 1), (C_, 1), (C_, 1), (C_, 1), (C_, 1)],
                D994=[(A, 50), (A, 50), (C_, 1), (C_, 1), (C_, 1)], D995=[(A, 50), (A, 50), (C_, 1), (C_, 1), (C_, 0)], D100=[(A, 40), (A, 30), (A, 20), (A, 10), (A, 5), (C_, 5)],
                D300=[(A, 60), (A, 60), (A, 60), (A, 60), (A, 60), (C_, 0)], V100=[(A, 60), (A, 60), (A, 60), (A, 60), (C_, 50), (C_, 50)], V1001=[(A, 60), (A, 60), (A, 60), (C_, 50), (C_, 50), (C_, 0)],
                ONE30=[(A, 60), (A, 60), (A, 60), (C_, 63), (C_, 20), (C_, 20)], TWO30=[(A, 60), (A, 60), (A, 60), (C_, 63), (C_, 30), (C_, 20)], Q29=[(A, 63), (A, 63), (C_, 29), (C_, 29), (C_, 29), (C_, 29)],
                Q30=[(A, 63), (A, 63), (C_, 30), (C_, 30), (C_, 30), (C_, 30)], TIE=[(A, 63), (A, 63), (A, 10), (C_, 60), (C_, 60), (G, 63), (G, 29), (G, 28)],
                Q128=[(A, 10), (A, 128), (C_, 190), (C_, 5), (C_, 4)])
    for name, col in COLS_AT.items():
        cells = spec[name] + [(T, 0)] * (8 - len(spec[name]))
        for r, (b, q) in enumerate(cells): B[r, col] = b; Q[r, col] = q
    Q[1, 71] = 41; Q[2, 71] = 63                                               # (128 and 190 each beside a value their block can hold them with)
    if side == 1: B, Q = (3 - B)[:, ::-1], Q[:, ::-1]                         # the stack shows the reverse complement: Reverse turns it back
    return [c.row(B[r], Q[r], 0, fw=(r % 2 == 0)) for r in range(8)]


def planted():
    c = Case(17)
    rng = c.rng
    for M in (48, 255, 256, 257, 400, 401):
        c.pair("M%d" % M, c.tiled(genome(rng, M)))
    g = genome(rng, 460)
    m460 = lambda: c.tiled(g) + [c.row(g[:60], 41, 0), c.row(g[:61], 42, 0), c.row(g[10:60], 43, 10, fw=False)]
    c.pair("M460", m460())
    g2 = genome(rng, 120)
    c.pair("NEG", [c.row(g2[:100], 40, -7), c.row(g2[7:110], 30, 0)])
    tw = c.row(genome(rng, 90), rng.choice(np.array([0, 2, 10, 37, 41], np.uint8), size=90), 0)
    c.pair("TWICE", [tw, (tw[0], 5, False)])
    for n in (1, 255, 256, 257, 600):
        gl = genome(rng, 70)
        alt = gl.copy(); alt[20:50] = (alt[20:50] + 1) % 4
        kinds = [c.row(gl, q, 0) for q in (0, 1, 2, 40, 3)] + [c.row(alt, 2, 0)]
        c.pair("LIVE%d" % n, [(kinds[i % 6][0], i % 3, True) for i in range(n)])
    c.pair("COLS", cols_stack(c, 0))
    c.pair("COLS1", m460(), cols_stack(c, 1))
    for gap in (5, 10):
        gg = genome(rng, 120)
        c.pair("GAP%d" % gap, [c.row(gg[:50], 40, 0), c.row(gg[50 + gap:], 40, 50 + gap)])
    def with_run(n, at, total):
        s = genome(rng, total)
        s[at:at + n] = 0
        if at: s[at - 1] = 1
        if at + n < total: s[at + n] = 2
        return s
    c.pair("RUN9", c.tiled(with_run(9, 30, 100)))
    c.pair("RUN10", c.tiled(with_run(10, 30, 100)))
    c.pair("RUN255", c.tiled(with_run(10, 251, 300)))
    c.pair("RUNEND", c.tiled(with_run(10, 90, 100)))
    for name, shift in (("CONF+", 30), ("CONF-", -30), ("CONF0-", 0)):
        for k in (9, 10):
            gc = genome(rng, 130)
            t1, t2 = (gc[:100].copy(), gc[shift:shift + 100].copy()) if shift >= 0 else (gc[-shift:-shift + 100].copy(), gc[:100].copy())
            # con1[i1] against con2[i1 - offset]: at offset = shift the two agree; k columns of the overlap are changed
            lo = max(0, shift)
            for x in range(k): t1[lo + 3 + 5 * x] = (t1[lo + 3 + 5 * x] + 1) % 4
            c.pair("%s%d" % (name, k), c.tiled(t1, length=100), c.tiled(rc(t2), length=100))
    c.pair("SIDE1NONE", c.filler(), [])
    c.pair("STATUS1", [], [], status=(0, 1))
    c.pair("STATUS2", [], [], status=(2, 1))
    return c.done()


def random_case(seed, n_pairs=6):
    c = Case(seed)
    rng = c.rng
    for p in range(n_pairs):
        sides = []
        for s in range(2):
            g = genome(rng, int(rng.choice([60, 300, 420, 520])))
            if rng.rand() < .5: g[40:40 + int(rng.choice([9, 10, 25]))] = rng.randint(4)
            rows = []
            for _ in range(int(rng.randint(1, 40))):
                a = int(rng.randint(0, max(1, len(g) - 48))); n = int(rng.choice([48, 60, 100, 151]))
                b = g[a:a + n].copy()
                for x in np.nonzero(rng.rand(len(b)) < .03)[0]: b[x] = rng.randint(4)
                rows.append(c.row(b, rng.choice(np.array([0, 1, 2, 10, 20, 30, 37, 41, 60], np.uint8), size=len(b)), a - int(rng.randint(0, 3)) * (a == 0), fw=bool(rng.randint(2))))
            sides.append(rows)
        c.pair("R%d" % p, sides[0], sides[1] if p != 3 else [])
    return c.done()


def no_pairs():
    c = Case(41)
    c.read(genome(c.rng, 80), 30)
    return c.done()


_made = {}


def seeded():
    """[(name, case)]"""
    if not _made:
        _made["planted"] = planted(); _made["random"] = random_case(3); _made["no-pairs"] = no_pairs()
    return list(_made.items())


_oracle = {}


def oracle(name, c):
    if name not in _oracle: _oracle[name] = scons_oracle.run(c["recs"], lambda id: c["reads"][id], lambda id: c["quals"][id])
    return _oracle[name]


def arrays(c):
    """the case as dfk_scons_build_arrays takes it"""
    from superplus_amd.dfk import WALKS_PLACED
    rp, ro, rl = pack(c["reads"])
    pq, pq_off = (np.asarray(c["pq"], np.uint8), np.asarray(c["pq_off"], np.uint64)) if "pq" in c else pq_of(c["quals"])      # (a fixture's own streams)
    recs = c["recs"]
    placed = np.zeros(sum(r["placed"] for r in recs), WALKS_PLACED)
    for i, (id, start, fw) in enumerate(l for r in recs for l in r["locs"]): placed[i] = (id, start, int(fw))
    return dict(starts=np.concatenate([[0], np.cumsum([r["placed"] for r in recs])]).astype(np.uint64), records=np.asarray([walks_oracle.record_words(r) for r in recs], np.uint32).reshape(-1, 8),
                placed=placed, read_packed=rp, read_off=ro, read_len=rl, pq=pq, pq_off=pq_off)


def case_text(name, c, r):
    """a case and what the oracle says of it, as tests/cpp/test_scons.cc reads it"""
    a = arrays(c)
    row = lambda v: " ".join(str(int(x)) for x in v) or "-"
    hexrow = lambda b: bytes(b).hex() or "-"
    digits = lambda v: "".join(str(int(x)) for x in v) or "-"
    el = r["elements"]
    return ["case %s %d %d" % (name, len(c["reads"]), len(c["recs"]) // 2), row(a["starts"]), row(a["records"].reshape(-1)), row([v for rec in c["recs"] for l in rec["locs"] for v in l]),
            row(a["read_len"]), hexrow(a["read_packed"]), row(a["pq_off"]), hexrow(a["pq"]),
            row([w for e in el for w in scons_oracle.dim_words(e)]), digits([b for e in el for b in e["con"]]), row([q for e in el for q in e["conq"]]), row([x for t in r["counts"] for x in t]),
            "%d %d %d %d %d %d" % (r["cells"], r["capped"], r["recount"], r["flat"], r["allowed"], r["disallowed"])]


def text():
    out = []
    for name, c in seeded(): out += case_text(name, c, oracle(name, c))
    return "\n".join(out) + "\n"


if __name__ == "__main__":
    open(FILE, "w").write(text())
