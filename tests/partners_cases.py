"""Seeded inputs of the search for unplaced partners (tests/partners_oracle.py): small graphs with chosen edge bases, closer tables, pairs
and reads, for tests/cpp/test_partners.cc (recorded in tests/cpp/partners_cases.txt: the C++ restatement of
superplus_amd/csrc/dfk_partners.h against the Python one) and for tests/test_gpu_partners.py (dfk_partners_build_arrays).
`python -m tests.partners_cases` rewrites the recorded file.

The stage takes locs and anchors as dfk_closer_fetch gives them, so a case chooses them directly: per closer edge a forward part
(ascending ids with repeats), a backward part, and anchors (g, add, count) ascending by (g, add).  What a case holds, each at the
smallest size that can still go wrong (`planted`, the first edges and reads of the case; the rest is random):
   edges   0: 31 bases (no entry)   1: 32 (one entry)   2: 33   3: 40 x A (nine entries of key 0)   4: 32 x T (key all ones)
           5: 150 random bases      6: bases 10 .. 70 of edge 5   7: 100 random bases with its bases 0 .. 32 again at 50
           8: 4 bases, 9: 20 bases (K = 4 graphs have such edges)
   anchors of closer edge A = 10: (5, 7, 5) and (6, 17, 6) -- the 32-mers of edge 6 are edge 5's ten further on, and 17 = 7 + 10: one value
           of closer edge B = 11: (7, -3, 5): a 32-mer twice, at -3 and 47;  of closer edge C = 12: (3, 0, 5), (4, 2, 9), (0, 1, 5), (1, 5, 5), (2, 0, 7),
           (8, 0, 5), (9, 0, 5);  closer edge D = 13 has no anchors;  closer edge S (the last, self-inverse) has (5, 0, 5)
   pairs   (B, inv[A]) (C, inv[A]) (D, inv[C]) (A, inv[B]) (S, S) (A, inv[A]) and again (B, inv[A]), and its reverse (A, inv[B]) ... so that
           es = {B, A}, {C, A}, {D, C}, {A, B}, {S, S}, {A, A}
   reads   mates of the forward reads of B, searched against bod(A):
             r1  = edge 5 [20:84]: 33 positions, all say 7 + 20 -- and through edge 6 the same: kept at 27
             r3  = edge 5 [0:40] then edge 5 [100:140]: two runs that disagree (7 and 7 + 100 - 40): dropped
             r5  = 31 bases of edge 5: no position          r7 = edge 5 [60:92]: one position, 67, only edge 5 has it (6 ends at 70)
             r9  = 40 random bases then edge 5 [0:33]: 7 - 40 = -33, negative, twice
             r11 is in the forward part of A too: skipped     r13 is in A's backward part only: searched
             r15 = edge 5 [0:140] : 109 positions, a lane takes two
           mates of the forward reads of A, against bod(B): r17 = edge 7 [0:32]: -3 and 47: dropped; r19 = edge 7 [10:50]: kept at 7
           mates of the forward reads of C ... against bod(A); of A against bod(C): r21 = 36 x A: key 0 at nine places: dropped;
             r23 = 32 x T: kept at 2; r25 = edge 1: kept at 5; r27 = edge 2: two positions, 0 and 0: kept
   r0, r2, ... carry the forward records.  A read id with both flags: r0 on B."""
import os

import numpy as np

from tests import partners_oracle
from tests.closer_oracle import closer_edges

FILE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "cpp", "partners_cases.txt")
K = 48

# name, seed, E (random edges beyond the planted), N, pairs, planted, recorded
SPECS = [("planted", 1, 8, 64, 0, True, True), ("random", 2, 20, 120, 12, False, True), ("planted-more", 3, 16, 200, 10, True, True),
         ("no-pairs", 4, 10, 40, 0, False, True), ("no-reads", 5, 10, 0, 6, False, True),
         ("many-queries", 6, 12, 12000, 6, False, False),             # more queries than two tiles of device_scan (2 x 2048)
         ("large-bod", 7, 6, 400, 4, False, False)]                   # a bod of more entries than two tiles of the sort (2 x 2048)


def rand_bases(rng, n):
    return rng.randint(0, 4, size=n).astype(np.uint8)


def make(seed, E_more, N, n_pairs, planted, large=False):
    rng = np.random.RandomState(seed)
    edges = []
    if planted:
        e5 = rand_bases(rng, 150)
        e7 = rand_bases(rng, 100); e7[50:82] = e7[0:32]
        edges = [rand_bases(rng, 31), rand_bases(rng, 32), rand_bases(rng, 33), np.zeros(40, np.uint8), np.full(32, 3, np.uint8), e5, e5[10:70].copy(), e7,
                 rand_bases(rng, 4), rand_bases(rng, 20)]
        edges += [rand_bases(rng, 60) for _ in range(4)]           # A B C D = 10 .. 13
    n0 = len(edges)
    if (n0 + E_more) % 2 == 0: E_more += 1                           # the non-self-inverse edges pair up
    for _ in range(E_more):
        edges.append(rand_bases(rng, int(rng.choice([3000, 5000] if large else [20, 32, 33, 48, 90, 200, 64]))))
    E = len(edges)
    inv = [e ^ 1 for e in range(E - 1)] + [E - 1]                    # the last edge is its own involution
    S = E - 1
    pairs = []
    if planted:
        A, B, C, D = 10, 11, 12, 13
        pairs = [(B, inv[A]), (C, inv[A]), (D, inv[C]), (A, inv[B]), (S, S), (A, inv[A]), (B, inv[A]), (A, inv[B])]
    lo = n0
    pairs += [(int(rng.randint(lo, E)), int(rng.randint(lo, E))) for _ in range(n_pairs)]
    if n_pairs >= 2: pairs += [pairs[-1], (inv[pairs[-2][1]], inv[pairs[-2][0]])]        # a pair twice, one reversed
    ce = closer_edges(pairs, inv)
    rank = {e: k for k, e in enumerate(ce)}
    reads = [rand_bases(rng, int(rng.choice([0, 30, 31, 32, 33, 50, 100, 151]))) for _ in range(N)]
    locs = [[] for _ in ce]      # forward ids, then backward
    fwd, bwd, anchors = [[] for _ in ce], [[] for _ in ce], [[] for _ in ce]
    long_edges = [g for g in range(E) if len(edges[g]) >= 32]
    first_free = 28 if planted else 0
    for k, e in enumerate(ce):
        if planted and e in (10, 11, 12, 13, S): continue
        if N > first_free and rng.rand() < 0.85:
            n_f = int(rng.randint(1, max(2, min(N - first_free, N // max(1, len(ce)) * 2 + 2))))
            fwd[k] = sorted(int(x) for x in rng.randint(first_free, N, size=n_f))
        if N > first_free and rng.rand() < 0.7: bwd[k] = sorted(int(x) for x in rng.randint(first_free, N, size=int(rng.randint(1, 6))))
        if rng.rand() < 0.85:
            a = {(int(rng.choice(long_edges if rng.rand() < 0.9 else list(range(E)))), int(rng.randint(-40, 300))) for _ in range(int(rng.randint(1, 4)))}
            anchors[k] = [(g, add, int(rng.randint(5, 12))) for g, add in sorted(a)]
    if planted:
        assert N >= 28
        e5, e7 = edges[5], edges[7]
        anchors[rank[10]] = [(5, 7, 5), (6, 17, 6)]
        anchors[rank[11]] = [(7, -3, 5)]
        anchors[rank[12]] = sorted([(3, 0, 5), (4, 2, 9), (0, 1, 5), (1, 5, 5), (2, 0, 7), (8, 0, 5), (9, 0, 5)])
        anchors[rank[S]] = [(5, 0, 5)]
        fwd[rank[11]] = [0, 0, 2, 4, 6, 8, 10, 12, 14]; bwd[rank[11]] = [0, 30]
        fwd[rank[10]] = [11, 16, 18, 20, 22, 24, 26]; bwd[rank[10]] = [13]
        fwd[rank[12]] = [20, 22]; bwd[rank[12]] = []
        fwd[rank[13]] = []; bwd[rank[13]] = [1]
        fwd[rank[S]] = [0, 2]; bwd[rank[S]] = [0, 2]
        reads[1] = e5[20:84].copy()
        reads[3] = np.concatenate([e5[0:40], e5[100:140]])
        reads[5] = e5[0:31].copy(); reads[7] = e5[60:92].copy()
        reads[9] = np.concatenate([rand_bases(rng, 40), e5[0:33]])
        reads[11] = e5[0:50].copy(); reads[13] = e5[30:80].copy(); reads[15] = e5[0:140].copy()
        reads[17] = e7[0:32].copy(); reads[19] = e7[10:50].copy()
        reads[21] = np.zeros(36, np.uint8); reads[23] = np.full(32, 3, np.uint8); reads[25] = edges[1].copy(); reads[27] = edges[2].copy()
    # mates that will be found, missed or found twice: for a few forward reads of every side, a piece (or two) of an anchor of the other side
    for e1, e2 in pairs:
        ks = [rank[e1], rank[inv[e2]]]
        for ei in (0, 1):
            k, ko = ks[ei], ks[1 - ei]
            usable = [(g, add) for g, add, _ in anchors[ko] if len(edges[g]) >= 40]
            for id1 in fwd[k]:
                id2 = id1 ^ 1
                if id2 < first_free or not usable or rng.rand() < 0.5: continue
                g, _ = usable[int(rng.randint(len(usable)))]
                n = len(edges[g])
                a = int(rng.randint(0, n - 36)); b = int(rng.randint(a + 33, min(n, a + 120) + 1))
                piece = edges[g][a:b]
                if rng.rand() < 0.25 and n >= 80: piece = np.concatenate([piece, edges[g][0:34]])           # a second run that disagrees
                reads[id2] = np.concatenate([rand_bases(rng, int(rng.randint(0, 20))), piece])
            for id1 in fwd[k][:2]:                                                                        # a mate already placed on the other side; one placed backward only
                if id1 >= first_free and (id1 ^ 1) >= first_free and not (planted and ce[ko] in (10, 11, 12, 13, S)):
                    (fwd if rng.rand() < 0.5 else bwd)[ko].append(id1 ^ 1)
    for k in range(len(ce)):
        fwd[k].sort(); bwd[k].sort()
        locs[k] = [(id, int(rng.randint(-100, 400)), True) for id in fwd[k]] + [(id, int(rng.randint(-100, 400)), False) for id in bwd[k]]
    return dict(inv=inv, edges=edges, ce=ce, locs=locs, anchors=anchors, pairs=pairs, reads=reads, planted=planted)


def seeded():
    """[(name, case, recorded)]"""
    return [(name, make(seed, E, N, np_, planted, name == "large-bod"), rec) for name, seed, E, N, np_, planted, rec in SPECS]


_oracle = {}


def oracle(name, c):
    if name not in _oracle: _oracle[name] = partners_oracle.run(c["inv"], c["edges"], c["ce"], c["locs"], c["anchors"], c["pairs"], lambda id: c["reads"][id])
    return _oracle[name]


def pack(seqs):
    """base code arrays -> (packed bytes dense, byte offsets [n + 1], lengths): 2 bits a base, LSB first, a sequence a whole number of bytes"""
    out, off, lens = [], [0], []
    for s in seqs:
        s = np.asarray(s, np.uint8)
        pad = np.concatenate([s, np.zeros((-len(s)) % 4, np.uint8)]).reshape(-1, 4)
        b = (pad[:, 0] | (pad[:, 1] << 2) | (pad[:, 2] << 4) | (pad[:, 3] << 6)).astype(np.uint8)
        out.append(b); off.append(off[-1] + len(b)); lens.append(len(s))
    return (np.concatenate(out) if out else np.zeros(0, np.uint8)), np.asarray(off, np.uint64), np.asarray(lens, np.uint32)


def arrays(c):
    """the case as dfk_partners_build_arrays takes it"""
    ep, eo, el = pack(c["edges"])
    rp, ro, rl = pack(c["reads"])
    starts = lambda per: np.concatenate([[0], np.cumsum([len(x) for x in per])]).astype(np.uint64)
    from tests.closer_oracle import anchor_words, loc_words
    return dict(inv=np.asarray(c["inv"], np.int32), edge_packed=ep, edge_off=eo, edge_len=el, ce=np.asarray(c["ce"], np.uint64), loc_first=starts(c["locs"]),
                locs=loc_words([l for per in c["locs"] for l in per]), anchor_first=starts(c["anchors"]),
                anchors=anchor_words([a for per in c["anchors"] for a in per]).astype(np.int32), pairs=np.asarray(c["pairs"], np.int32).reshape(-1, 2),
                read_packed=rp, read_off=ro, read_len=rl)


def case_text(name, c, r=None):
    """a case and what the oracle says of it, as tests/cpp/test_partners.cc reads it"""
    if r is None: r = oracle(name, c)
    a = arrays(c)
    row = lambda v: " ".join(str(int(x)) for x in v)
    hexrow = lambda b: bytes(b).hex() or "-"
    return ["case %s %d %d %d %d" % (name, len(c["inv"]), len(c["reads"]), len(c["pairs"]), len(c["ce"])), row(c["inv"]), row(a["edge_len"]), hexrow(a["edge_packed"]),
            row(c["ce"]), row(a["loc_first"]), row([x for per in c["locs"] for l in per for x in l]), row(a["anchor_first"]), row([x for per in c["anchors"] for t in per for x in t]),
            row([e for p in c["pairs"] for e in p]), row(a["read_len"]), hexrow(a["read_packed"]), row(r["starts"]), row([x for rec in r["records"] for x in rec[:2]]),
            "%d %d %d %d %d %d %d" % (r["queries"], r["positions"], r["entries"], r["any_hit"], r["kept"], r["multi"], r["searched"])]


def text(recorded=True):
    out = []
    for name, c, rec in seeded():
        if rec == recorded: out += case_text(name, c)
    return "\n".join(out) + "\n"


if __name__ == "__main__":
    open(FILE, "w").write(text())
