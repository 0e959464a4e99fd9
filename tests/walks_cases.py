"""Seeded inputs of Stackster's stack walks (tests/walks_oracle.py): small graphs with chosen closer edges, edge bases, read sets, pairs,
reads and qualities, for tests/cpp/test_walks.cc (recorded in tests/cpp/walks_cases.txt: the C++ restatement of
superplus_amd/csrc/dfk_walks.h against the Python one) and for tests/test_gpu_walks.py (dfk_walks_build_arrays).
`python -m tests.walks_cases` rewrites the recorded file.

The stage takes the read sets as dfk_closer_fetch gives them, so a case chooses them directly.  A case is built from PLANTS: a plant has
a genome of its own, an edge A cut from it (with its involution), reads cut from the genome and stored forward (set entry (id, True) of
A) or reverse-complemented ((id, False)), and by default the pair (A, inv[F]) with F an edge of another genome that only one far read
lies on: side 0 walks A, side 1 walks F and places that read.  `planted` (K = 48) holds, by plant name:
   EXACT48   an edge of exactly 48 bases under reads that run 150 bases on: the walk runs well past the edge's end.
   INSIDE    an edge of 200 bases, reads over its first 90 only: the walk stops inside the edge.
   NOBODY0   no read holds the first 48-mer: side 0 places nobody, side 1 is not walked.
   NOBODY1   pair (A, inv[G]) with G an edge no read lies on: side 1 is walked and places nobody.
   TANDEM    U + 6 x a 12-base unit + V: the long reads placed at the first step carry the walk through the repeat, every step inside
             it is a duplicate step (a read holds the 48-mer two or three times); read R, which starts inside the repeat, is placed only
             by the first 48-mer that leaves it: a later step.
   TANDEM0   the edge inside the repeat: the first step is a duplicate, nobody is ever placed.
   STARTS    reads that begin 7 bases before the edge (start -7), with it (0) and 30 bases in (placed at a later step: start 30).
   LEN48     a read of exactly 48 bases (placed, never live) and reads of 47 and 10 bases (no 48-mer: never placed) beside a carrier.
   BOTH      one read in the set with both flags.
   TH59 TH60 one read of 49 bases over the edge's first 48, quality 59 / 60 at the 49th: stop / append.
   TWICE TWICE1   two reads that differ at the 49th base with qualities 40 and 80 / 79: 80 >= 2 x 40 appends, 79 does not.
   THREE     three reads, three bases at the 49th: 63 + 37 (two reads of one base), 30, 20: appended.
   ZERO      a column of quality 0: the walk ends there.
   LOW19 LOW20    a homopolymer of 19 / 20 bases behind the edge under three reads of quality 63: the walk crosses it / ends where it begins.
   LOWENDS   reads with runs of 20 at either end and one that is a single run; qualities 0, 1, 4, 5, 6 in the runs; 127, 128, 190 elsewhere.
   M401      reads of 250 bases tiled over 460 bases of genome: M > 400, trim > 0.
   SELF      the self-inverse edge S (a palindrome) as e1.
   SAME      pair (A, inv[A]): es = { A, A }, every read in the set with both flags.
   LIVE1 LIVE64 LIVE65 LIVE300   so many copies of one read: the live list of 1, 64, 65, 300 entries.
   the pair of STARTS is listed twice; EMPTY is a pair of two edges without reads.
Qualities: feudal.pq_encode holds a block's least quality in six bits: a run of one quality above 63 does not fit; the cases keep such
values single."""
import os

import numpy as np

from superplus_amd import feudal
from tests import walks_oracle
from tests.closer_oracle import closer_edges, read_words
from tests.partners_cases import pack

FILE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "cpp", "walks_cases.txt")
K = 48


def rc(b):
    return (3 - np.asarray(b, np.uint8))[::-1].copy()


def genome(rng, n):
    """random bases without a run of 4 (so that no lowering and no tandem happens by accident)"""
    g = rng.randint(0, 4, size=n).astype(np.uint8)
    for i in range(3, n):
        if g[i] == g[i - 1] == g[i - 2] == g[i - 3]: g[i] = (g[i] + 1 + rng.randint(3)) % 4
    return g


class Case:
    def __init__(self, seed, K_=K):
        self.rng = np.random.RandomState(seed)
        self.K = K_
        self.edges, self.reads, self.quals, self.sets, self.pairs, self.name = [], [], [], {}, [], {}

    def edge(self, bases, name=None):
        """-> its id; its involution is id + 1"""
        e = len(self.edges)
        self.edges += [np.asarray(bases, np.uint8), rc(bases)]
        self.sets[e] = []; self.sets[e + 1] = []
        if name: self.name[name] = e
        return e

    def palindrome(self, half, name=None):
        e = len(self.edges)
        self.edges.append(np.concatenate([half, rc(half)]).astype(np.uint8))
        self.sets[e] = []
        if name: self.name[name] = e
        return e

    def read(self, bases, q=63):
        """a read and its mate of 7 bases -> the read's id"""
        bases = np.asarray(bases, np.uint8)
        self.reads.append(bases); self.quals.append(np.full(len(bases), q, np.uint8) if np.isscalar(q) else np.asarray(q, np.uint8))
        self.reads.append(genome(self.rng, 7)); self.quals.append(np.full(7, 20, np.uint8))
        assert len(self.reads[-2]) == len(self.quals[-2])
        return len(self.reads) - 2

    def lay(self, e, bases, q=63, stored_fw=True):
        """a read lying along O(e): stored as it lies, or reverse-complemented with the flag false"""
        if stored_fw: id = self.read(bases, q)
        else: id = self.read(rc(bases), q if np.isscalar(q) else np.asarray(q)[::-1])
        self.sets[e].append((id, stored_fw))
        return id

    def done(self):
        E = len(self.edges)
        inv = list(range(E))
        for e in range(E):
            if np.array_equal(rc(self.edges[e]), self.edges[e]): inv[e] = e
            elif e + 1 < E and np.array_equal(rc(self.edges[e]), self.edges[e + 1]): inv[e] = e + 1; inv[e + 1] = e
        ce = closer_edges(self.pairs, inv)
        kmers = [len(b) - self.K + 1 for b in self.edges]
        assert min(kmers + [1]) >= 1
        return dict(inv=inv, kmers=kmers, K=self.K, edge_bases=self.edges, ce=ce, reads_per=[sorted(set(self.sets[e])) for e in ce], pairs=self.pairs, reads=self.reads, quals=self.quals,
                    name=self.name)


def planted():
    c = Case(11)
    rng = c.rng
    gF = genome(rng, 200)
    F = c.edge(gF[:100], "F")
    c.lay(F, gF[:120])
    G = c.edge(genome(rng, 90), "G")
    EMPTY = c.edge(genome(rng, 70), "EMPTY")

    def plant(name, edge_len, glen=400, other=None):
        g = genome(rng, glen)
        e = c.edge(g[:edge_len], name)
        c.pairs.append((e, c_inv(F if other is None else other)))
        return g, e
    c_inv = lambda e: e + 1                                                    # (of an edge made by edge(): its neighbour)
    g, e = plant("EXACT48", 48)
    for a in (0, 20, 60, 100): c.lay(e, g[a:a + 150], stored_fw=a != 20)
    g, e = plant("INSIDE", 200)
    for a in (0, 5, 10): c.lay(e, g[a:a + 80])
    g, e = plant("NOBODY0", 100)
    c.lay(e, genome(rng, 150))
    g, e = plant("NOBODY1", 100, other=G)
    for a in (0, 3): c.lay(e, g[a:a + 150])
    # TANDEM
    unit = genome(rng, 12)
    U, V = genome(rng, 80), genome(rng, 120)
    g = np.concatenate([U, np.tile(unit, 6), V])
    e = c.edge(g[:60], "TANDEM"); c.pairs.append((e, c_inv(F)))
    for a in (0, 4, 9): c.lay(e, g[a:a + 250])
    c.name["TANDEM_R"] = c.lay(e, g[80 + 5:80 + 72 + 70])
    e = c.edge(g[80:80 + 60], "TANDEM0"); c.pairs.append((e, c_inv(F)))
    for a in (80, 83): c.lay(e, g[a:a + 150])
    g, e = plant("STARTS", 120)
    gpre = np.concatenate([genome(rng, 7), g])
    c.lay(e, gpre[:150]); c.lay(e, g[:150]); c.lay(e, g[:140], stored_fw=False); c.lay(e, g[30:200])
    c.pairs.append(c.pairs[-1])                                                # the pair listed twice
    g, e = plant("LEN48", 100)
    for a in (0, 2, 6): c.lay(e, g[a:a + 150])
    c.name["LEN48_R"] = c.lay(e, g[20:68]); c.lay(e, g[20:67]); c.lay(e, g[5:15])
    g, e = plant("BOTH", 100)
    for a in (0, 2, 6): c.lay(e, g[a:a + 150])
    c.sets[e].append((c.sets[e][0][0], False))
    tail = lambda x: [30] * 44 + [31, 30, 31, 30, x]                            # (a value above 63 inside a mixed block)
    for name, q49 in (("TH59", 59), ("TH60", 60)):
        g, e = plant(name, 60)
        c.lay(e, g[:49], tail(q49))
    for name, q in (("TWICE", 80), ("TWICE1", 79)):
        g, e = plant(name, 60)
        other = np.concatenate([g[:48], [(g[48] + 1) % 4]])
        c.lay(e, g[:49], tail(q)); c.lay(e, other, tail(40))
    g, e = plant("THREE", 60)
    alt = lambda d: np.concatenate([g[:48], [(g[48] + d) % 4]])
    c.lay(e, g[:49], [30] * 48 + [63]); c.lay(e, g[:49], [30] * 48 + [37]); c.lay(e, alt(1), 30); c.lay(e, alt(2), 20)
    g, e = plant("ZERO", 100)
    for a in (0, 1): c.lay(e, g[a:a + 120], [63] * (70 - a) + [0] + [63] * (49 + a))
    for name, run in (("LOW19", 19), ("LOW20", 20)):
        g = genome(rng, 300)
        g[70:70 + run] = 0; g[69] = 1; g[70 + run] = 2
        e = c.edge(g[:60], name); c.pairs.append((e, c_inv(F)))
        for a in (0, 3, 8): c.lay(e, g[a:a + 200])
    g = genome(rng, 300)
    g[:20] = 3; g[20] = 0; g[130:150] = 1; g[129] = 2
    e = c.edge(g[:100], "LOWENDS"); c.pairs.append((e, c_inv(F)))
    q = np.full(150, 63, np.uint8); q[:5] = [0, 1, 4, 5, 6]; q[60] = 127; q[62] = 128; q[64] = 190; q[145:150] = [6, 5, 4, 1, 0]
    c.lay(e, g[:150], q); c.lay(e, g[:150], 40); c.lay(e, g[:150], q, stored_fw=False)
    c.lay(e, np.full(60, 2, np.uint8), 41)                                     # a single run
    g, e = plant("M401", 300, glen=600)
    for a in range(0, 211, 35): c.lay(e, g[a:a + 250])
    half = genome(rng, 40)
    S = c.palindrome(half, "SELF")
    gs = np.concatenate([half, rc(half), genome(rng, 100)])
    for a in (0, 2): c.lay(S, gs[a:a + 150])
    c.pairs.append((S, c_inv(F)))
    g = genome(rng, 300)
    e = c.edge(g[:80], "SAME"); c.pairs.append((e, e + 1))
    for a in (0, 4, 7): c.lay(e, g[a:a + 150])
    for n in (1, 64, 65, 300):
        g, e = plant("LIVE%d" % n, 60)
        for _ in range(n): c.lay(e, g[:120], 63 if n == 1 else 2 if n == 300 else 3)
    c.pairs.append((EMPTY, c_inv(G)))
    return c.done()


def random_case(seed, n_genomes=6, K_=K):
    """genomes with planted homopolymers and tandem repeats, edges cut from them, reads at random places on either strand, random sets"""
    c = Case(seed, K_)
    rng = c.rng
    edges = []
    for gi in range(n_genomes):
        g = genome(rng, 500)
        if gi % 2: g[150:150 + int(rng.choice([19, 20, 25]))] = rng.randint(4)
        if gi % 3 == 0: g[250:250 + 60] = np.tile(genome(rng, 10), 6)
        a = int(rng.randint(0, 40))
        e = c.edge(g[a:a + int(rng.choice([K_ + 0, K_ + 1, 100, 180]))])
        edges += [e, e + 1]
        for _ in range(int(rng.randint(0, 60))):
            s = max(0, a + int(rng.randint(-30, 30 if rng.rand() < .5 else 200))); n = int(rng.choice([30, 47, 48, 49, 100, 151, 151]))
            q = rng.choice(np.array([0, 2, 10, 20, 30, 37, 41], np.uint8), size=n)
            id = c.lay(e, g[s:s + n], q, stored_fw=bool(rng.randint(2)))
            if rng.rand() < 0.2: c.sets[e + 1].append((id, bool(rng.randint(2))))
    for _ in range(10): c.pairs.append((int(rng.choice(edges)), int(rng.choice(edges))))
    c.pairs += [c.pairs[0], (c.pairs[1][1] ^ 1, c.pairs[1][0] ^ 1)]
    return c.done()


def k40_short():
    """K = 40: an edge of 47 bases (8 k-mers) as es[0] of one pair and as es[1] of another; both sides of a third pair are fine"""
    c = Case(31, 40)
    g, h = genome(c.rng, 300), genome(c.rng, 300)
    short = c.edge(g[:47], "SHORT"); fine = c.edge(h[:90], "FINE")
    for a in (0, 2): c.lay(short, g[a:a + 150]); c.lay(fine, h[a:a + 150])
    c.pairs += [(short, fine ^ 1), (fine, short ^ 1), (fine, fine ^ 1)]
    return c.done()


def no_pairs():
    c = Case(41)
    e = c.edge(genome(c.rng, 80)); c.lay(e, genome(c.rng, 100))
    return c.done()


def tiny(n_pairs=1500):
    """3 000 walks of tiny sets: the batch boundaries"""
    c = Case(51)
    g = genome(c.rng, 260)
    es = []
    for i in range(12):
        e = c.edge(g[i * 7:i * 7 + 60 + i]); es.append(e)
        for a in range(i % 3): c.lay(e, g[i * 7 + a:i * 7 + a + 60 + 10 * a])
    for i in range(n_pairs): c.pairs.append((es[i % 12], es[(i * 5 + 1) % 12] ^ 1))
    return c.done()


_made = {}


def seeded():
    """[(name, case, recorded)]"""
    if not _made:
        _made["planted"] = (planted(), True); _made["random"] = (random_case(2), True); _made["random-k60"] = (random_case(7, 4, 60), True)
        _made["k40-short"] = (k40_short(), True); _made["no-pairs"] = (no_pairs(), True); _made["tiny-3000"] = (tiny(), False)
    return [(name, c, rec) for name, (c, rec) in _made.items()]


_oracle = {}


def oracle(name, c):
    if name not in _oracle:
        _oracle[name] = walks_oracle.run(c["inv"], c["edge_bases"], c["ce"], c["reads_per"], c["pairs"], lambda id: c["reads"][id], lambda id: c["quals"][id])
    return _oracle[name]


def pq_of(quals):
    """-> (PQVec bytes, offsets [n + 1]); every stream decodes to what went in"""
    out, off = [], [0]
    for q in quals:
        b = feudal.pq_encode(q)
        assert feudal.pq_decode(b) == [int(x) for x in q]
        out.append(np.frombuffer(b, np.uint8)); off.append(off[-1] + len(b))
    return (np.concatenate(out) if out else np.zeros(0, np.uint8)), np.asarray(off, np.uint64)


def arrays(c):
    """the case as dfk_walks_build_arrays takes it"""
    rp, ro, rl = pack(c["reads"])
    ep, eo, el = pack(c["edge_bases"])
    pq, pq_off = (np.asarray(c["pq"], np.uint8), np.asarray(c["pq_off"], np.uint64)) if "pq" in c else pq_of(c["quals"])      # (a fixture's own streams)
    starts = lambda per: np.concatenate([[0], np.cumsum([len(x) for x in per])]).astype(np.uint64)
    return dict(inv=np.asarray(c["inv"], np.int32), kmers=np.asarray(c["kmers"], np.int32), edge_packed=ep, edge_off=eo, ce=np.asarray(c["ce"], np.uint64), read_first=starts(c["reads_per"]),
                reads=read_words([r for per in c["reads_per"] for r in per]), pairs=np.asarray(c["pairs"], np.int32).reshape(-1, 2), read_packed=rp, read_off=ro, read_len=rl, pq=pq, pq_off=pq_off)


def case_text(name, c, r):
    """a case and what the oracle says of it, as tests/cpp/test_walks.cc reads it"""
    a = arrays(c)
    row = lambda v: " ".join(str(int(x)) for x in v)
    hexrow = lambda b: bytes(b).hex() or "-"
    return ["case %s %d %d %d %d %d" % (name, len(c["inv"]), len(c["reads"]), len(c["pairs"]), len(c["ce"]), c["K"]), row(c["inv"]), row(c["kmers"]), hexrow(a["edge_packed"]), row(c["ce"]),
            row(a["read_first"]), row(a["reads"]), row([e for p in c["pairs"] for e in p]), row(a["read_len"]), hexrow(a["read_packed"]), row(a["pq_off"]), hexrow(a["pq"]),
            row([w for x in r["recs"] for w in walks_oracle.record_words(x)]), row([v for x in r["recs"] for l in x["locs"] for v in l]),
            "".join(str(int(b)) for x in r["recs"] for b in x["EE"]) or "-", "%d %d %d %d" % (r["walks"], r["steps"], r["live_sum"], r["live_max"])]


def text(recorded=True):
    out = []
    for name, c, rec in seeded():
        if rec == recorded: out += case_text(name, c, oracle(name, c))
    return "\n".join(out) + "\n"


if __name__ == "__main__":
    open(FILE, "w").write(text())
