"""Ten seeded small graphs with paired reads on them, and the text file tests/cpp/hops_cases.txt in which tests/hops_oracle.py's
answers for them (44 recorded cases: each graph with ONE_GOOD off and on, under one to three capacities) are recorded for tests/cpp/test_hops.cc (superplus_amd/csrc/dfk_hops.h, the C++ restatement of FindEdgePairs).
tests/test_gpu_hops_seeded.py hands the same graphs to the GPU.

    python -m tests.hops_cases            rewrites tests/cpp/hops_cases.txt

Two families.  The six of SPECS are dense and random, and not assemblies of anything: vertices come in reverse-complement pairs
(v, v ^ 1), an edge u -> v has the involuted edge (v ^ 1) -> (u ^ 1), now and then an edge u -> u ^ 1 is its own involution; edge
lengths are drawn from the thresholds' neighbourhoods (1, 39/40, 99/100, 120/121 k-mers).  A pair of reads is two pieces of one
walk, the second read on the other strand, so that mates land where the rule looks for them.  They are cyclic, so hardly an edge
passes the sink test and they give next to no pair: what they give is large sets.  The four of CHAIN_SPECS (further down) are chains
with gaps between them, which is what the rule was written for, with the motifs that put each threshold to work."""
import os

import numpy as np

from tests import hops_oracle

FILE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "cpp", "hops_cases.txt")
EXT_SLOTS, CAN = 32, 128                 # dfk_hops.h caps_of(): what does not follow DFK_HOPS_MAX_SEQS / DFK_HOPS_MAX_LEN

# (seed, edge pairs, vertex pairs, read pairs, K, capacities to run with: (max_seqs, max_len))
SPECS = [(1, 6, 4, 60, 24, [(96, 24), (1, 24)]), (2, 10, 5, 150, 24, [(96, 24), (6, 24), (96, 3)]), (3, 16, 9, 300, 30, [(96, 24), (8, 4)]),
         (4, 24, 10, 500, 24, [(96, 24), (12, 24)]), (5, 5, 2, 200, 10, [(96, 24), (20, 6)]), (6, 30, 20, 400, 48, [(96, 24)])]


def make(seed, edge_pairs, vertex_pairs, read_pairs, K):
    rng = np.random.default_rng(seed)
    lens = [1, 5, 20, 39, 40, 41, 60, 99, 100, 101, 120, 121, 150]
    to_left, to_right, inv, kmers = [], [], [], []
    for _ in range(edge_pairs):
        u, v = int(rng.integers(0, 2 * vertex_pairs)), int(rng.integers(0, 2 * vertex_pairs))
        k = int(rng.choice(lens))
        e = len(kmers)
        if rng.random() < 0.1:
            to_left.append(u); to_right.append(u ^ 1); inv.append(e); kmers.append(k)
        else:
            to_left += [u, v ^ 1]; to_right += [v, u ^ 1]; inv += [e + 1, e]; kmers += [k, k]
    E = len(kmers)
    frm = {}
    for e in range(E):
        frm.setdefault(to_left[e], []).append(e)
    paths = []
    for _ in range(read_pairs):
        w = [int(rng.integers(0, E))]
        while len(w) < 9 and rng.random() < 0.75 and frm.get(to_right[w[-1]]):
            nxt = frm[to_right[w[-1]]]
            w.append(int(nxt[int(rng.integers(0, len(nxt)))]))
        a = int(rng.integers(0, len(w) + 1)); b = int(rng.integers(0, len(w) + 1))
        r1 = w[:a] if rng.random() < 0.9 else []
        r2 = [inv[f] for f in reversed(w[b:])] if rng.random() < 0.85 else []
        pair = [r1, r2] if rng.random() < 0.5 else [r2, r1]
        paths += pair
    N = len(paths)
    bc = np.repeat(rng.integers(0, 6, N // 2), 2).astype(np.int64)          # both reads of a pair carry one barcode; 0 = none
    bad = (rng.random(N // 2) < 0.15).astype(np.uint8)
    return dict(K=K, kmers=kmers, inv=inv, to_left=to_left, to_right=to_right, paths=paths, bc=bc, bad=bad, n_vertices=2 * vertex_pairs)


# ---- the second family: gapped chains
# Linear chains of 1 to 6 edges through fresh vertices (every edge with its involution), short tips hung on them, read pairs cut from
# walks over the chains of a scaffold in order, so that mates land across the gaps: chain ends are sinks and chain starts are sources,
# which is where methods 1 and 2 look, and a chain's last edges cannot be extended, which is where method 3 looks.  On top of that each
# graph gets the motifs below: a few edges and reads of their own, each built so that ONE length or mark decides a pair.  What a motif
# plants is recorded beside the graph (`knobs`: what to move and where to; `marks`: edges a test looks up), and tests/test_hops_cpu.py
# asserts that moving it changes the union.  K is one of the library's (40, 48, 60), so the GPU runs these graphs as recorded.
# (name, seed, chains, read pairs, K, dense, capacities)
CHAIN_SPECS = [("chains1", 11, 8, 150, 40, False, [(96, 24), (3, 24), (96, 3)]), ("chains2", 12, 12, 200, 48, False, [(96, 24), (4, 24)]),
               ("chains3", 13, 16, 250, 60, False, [(96, 24), (1, 24)]), ("dense1", 14, 4, 40, 40, True, [(96, 24), (80, 24), (96, 3)])]
SHORT = 20                               # an edge no method-3 search starts from (< K + 1) and no `can` holds (< 40)


class _Builder:
    def __init__(self, K):
        self.K = K
        self.kmers, self.inv, self.to_left, self.to_right = [], [], [], []
        self.nv = 0
        self.paths, self.bc, self.sums = [], [], []
        self.knobs, self.marks = {}, {}

    def vertex(self):
        self.nv += 2
        return self.nv - 2

    def edge(self, u, v, k):
        e = len(self.kmers)
        if v == u ^ 1:                                                       # its own involution
            self.to_left.append(u); self.to_right.append(v); self.inv.append(e); self.kmers.append(k)
        else:
            self.to_left += [u, v ^ 1]; self.to_right += [v, u ^ 1]; self.inv += [e + 1, e]; self.kmers += [k, k]
        return e

    def chain(self, lens, start=None):
        v = self.vertex() if start is None else start
        out = []
        for k in lens:
            w = self.vertex(); out.append(self.edge(v, w, k)); v = w
        return out

    def tip_in(self, v, k):
        return self.edge(self.vertex(), v, k)

    def tip_out(self, v, k):
        return self.edge(v, self.vertex(), k)

    def pair(self, a, b, bc, sums=(0, 0), swap=False):
        """a pair of reads: a as it is, b (a walk on a's strand, further on) as its mate sees it; returns the pair's number"""
        r = [list(a), [self.inv[f] for f in reversed(b)]]
        s = list(sums)
        if swap: r.reverse(); s.reverse()
        self.paths += r; self.bc += [bc, bc]; self.sums += s
        return len(self.paths) // 2 - 1

    def blocked(self, k):
        """an edge of k k-mers that fails the source test (a tip of 130 k-mers enters its start) and whose involution fails the sink test"""
        s = self.vertex()
        self.tip_in(s, 130)
        return self.tip_out(s, k)

    def knob_kmers(self, name, e, there):
        self.knobs[name] = ("kmers", sorted({e, self.inv[e]}), there)

    def case(self):
        sums = np.asarray(self.sums, np.uint16)
        bad = ((sums[0::2] > 150) | (sums[1::2] > 150)).astype(np.uint8)
        return dict(K=self.K, kmers=self.kmers, inv=self.inv, to_left=self.to_left, to_right=self.to_right, paths=self.paths,
                    bc=np.asarray(self.bc, np.int64), bad=bad, sums=sums, n_vertices=self.nv, knobs=self.knobs, marks=self.marks)


def _motifs(b):
    K = b.K
    # the sink / source test at 120 | 121: a short edge a with one tip behind it, its reads' mates on a short far edge.  At 120
    # method 1 gives (a, far) and (inv far, inv a); at 121 a fails the sink test and inv a the source test, through that clause alone
    for k in (120, 121):
        a = b.chain([SHORT])[0]
        t = b.tip_out(b.to_right[a], k)
        far = b.chain([SHORT])[0]
        b.pair([a], [far], 1); b.pair([a], [far], 2, swap=True)
        b.knob_kmers(f"sink{k}", t, 241 - k)
        b.marks[f"sink{k}"] = (a, far)
    # method 2's landing at 100 | 99: a passes the sink test, its one supported e2 fails the source test
    for k in (100, 99):
        a = b.chain([SHORT])[0]
        far = b.blocked(k)
        b.pair([a], [far], 1); b.pair([a], [far], 3)
        b.knob_kmers(f"landing{k}", far, 199 - k)
        b.marks[f"landing{k}"] = (a, far)
    # MIN_RIGHT at 40 | 39, as it decides a member of `can` (methods 1 and 2 are kept off the pair: g fails the source test)
    for k in (40, 39):
        e = b.chain([K + 5])[0]
        g = b.blocked(k)
        b.pair([e], [g], 2); b.pair([e], [g], 4)
        b.knob_kmers(f"can{k}", g, 79 - k)
        b.marks[f"can{k}"] = (e, g)
    # ... and as it decides a member of too_easy: f lies directly behind e in the reads whose mates show f under two ids.  At 40 f
    # is in can and in too_easy; with the reads cut back to [e] it is in can alone and (e, f) appears.  At 39 it is in neither.
    # (e has 125 k-mers, so f fails the source test and method 1 leaves the pair alone.)
    for k in (40, 39):
        e, f = b.chain([125, k])
        p = [b.pair([e, f], [f], 1), b.pair([e, f], [f], 5)]
        b.knobs[f"easy{k}"] = ("paths", [2 * q for q in p], [e])
        b.marks[f"easy{k}"] = (e, f)
    # GOOD_EXT at 100 | 99: 60 + 40 k-mers behind e extend it; 60 + 39 do not, and (e, g) appears
    for k in (40, 39):
        e, f1, f2 = b.chain([K + 5, 60, k])
        h, g = b.chain([SHORT, 50])
        b.pair([e, f1, f2], [h, g], 1); b.pair([e, f1, f2], [h, g], 2, swap=True)
        b.knob_kmers(f"ext{60 + k}", f2, 79 - k)
        b.marks[f"ext{60 + k}"] = (e, g)
    # MIN_CAND: an edge of K k-mers is skipped, one of K + 1 searched, reads of two barcodes on both
    for k in (K, K + 1):
        e = b.chain([k])[0]
        g = b.blocked(50)
        b.pair([e], [g], 3); b.pair([e], [g], 5)
        b.knob_kmers(f"cand{k - K}", e, 2 * K + 1 - k)
        b.marks[f"cand{k - K}"] = (e, g)
    # MarkBads' sums at 150 | 151 on a pair that decides a candidate: two pairs show g to e, one of them carries the sum
    for v in (150, 151):
        e = b.chain([K + 5])[0]
        g = b.blocked(50)
        q = b.pair([e], [g], 1, sums=(v, 0)); b.pair([e], [g], 2)
        b.knobs[f"sum{v}"] = ("sums", [2 * q], 301 - v)
        b.marks[f"sum{v}"] = (e, g)
    # mate sets: (a, far) seen once; many times under one id; under exactly two ids of which one is the id all unbarcoded reads share
    a, far = b.chain([SHORT])[0], b.chain([SHORT])[0]
    b.pair([a], [far], 4)
    b.marks["once"] = (a, far)
    a, far = b.chain([SHORT])[0], b.chain([SHORT])[0]
    for _ in range(6): b.pair([a], [far], 3)
    b.marks["many"] = (a, far)
    a, far = b.chain([SHORT])[0], b.chain([SHORT])[0]
    b.pair([a], [far], 0); b.pair([a], [far], 4, swap=True)
    b.marks["shared0"] = (a, far)
    # a self-inverse edge long enough to be searched, with reads on it
    u = b.vertex()
    s = b.edge(u, u ^ 1, K + 10)
    a = b.tip_in(u, SHORT)
    g = b.chain([50])[0]
    b.pair([a, s], [g], 1); b.pair([s], [g], 2); b.pair([s], [], 3)
    b.marks["selfinv"] = (s, g)
    # a read that crosses an edge twice: a loop of 100 k-mers
    a = b.chain([SHORT])[0]
    v = b.to_right[a]
    l = b.edge(v, v, 100)
    c = b.tip_out(v, SHORT)
    b.pair([a, l, l, c], [], 1); b.pair([l], [], 2)
    b.marks["twice"] = (l, c)
    # a search of two rounds: [E0, E1] + [E1, E2] + [E2, E3], 40 k-mers an edge behind E0
    E = b.chain([K + 5, 40, 40, 40, 40])
    b.pair(E[0:2], E[1:3], 1); b.pair(E[0:2], E[2:4], 2)
    b.marks["rounds"] = (E[0], E[3])


def _dense(b):
    K = b.K
    # X of 1 + 12 * 13 / 2 = 79 sequences (fits the default capacities: the dedup loop strides past lane 63) and of 1 + 14 * 15 / 2 =
    # 106 (does not: the host's route at the defaults): reads on a hub edge whose mates lie on every sub-walk of a chain
    for m, name in ((12, "x79"), (14, "x106")):
        e = b.chain([K + 5])[0]
        G = b.chain([1 if i % 2 else 45 for i in range(m)])
        n = 0
        for i in range(m):
            for j in range(i + 1, m + 1):
                b.pair([e], G[i:j], 1 + n % 5, swap=n % 3 == 0); n += 1
        b.marks[name] = (e, G[0])
    # a combined-index list of 260 entries: 130 pairs whose reads lie on an edge and on its involution
    e = b.chain([K + 5])[0]
    for n in range(130): b.pair([e], [e], n % 6, sums=(0, 151 if n % 7 == 0 else 150))
    b.marks["list260"] = (e, b.inv[e])
    # 32 extensions at once: every walk down a ladder of five bubbles behind e (100 k-mers an edge: extended before any round)
    e = b.chain([K + 5])[0]
    v = b.to_right[e]
    rungs = []
    for _ in range(5):
        w = b.vertex()
        rungs.append((b.edge(v, w, 100), b.edge(v, w, 100))); v = w
    for n in range(32): b.pair([e] + [rungs[i][(n >> i) & 1] for i in range(5)], [], 1 + n % 4)
    b.marks["exts32"] = (e, rungs[0][0])
    # an extension of 49 edges (exts hold 48 at the defaults): 49 edges of one k-mer behind e, laid on one another by three mates'
    # windows; the 50th has 45 k-mers and two ids, so the pair (e, the 50th) comes from the host's route alone
    C = b.chain([K + 5] + [1] * 49 + [45])
    e, C = C[0], C[1:]
    b.pair([e] + C[:23], C[12:36], 1); b.pair([e], C[24:48], 2); b.pair([e], C[36:50], 3); b.pair([e], C[40:50], 4)
    b.marks["ext49"] = (e, C[49])


def make_chains(seed, n_chains, read_pairs, K, dense=False):
    rng = np.random.default_rng(seed)
    lens = [1, 5, 20, 39, 40, 41, 60, 99, 100, 101, 120, 121, 150]
    b = _Builder(K)
    chains = [b.chain([int(rng.choice(lens)) for _ in range(int(rng.integers(1, 7)))]) for _ in range(n_chains)]
    for ch in chains:                                                        # short tips on inner vertices
        for e in ch[:-1]:
            if rng.random() < 0.25:
                (b.tip_out if rng.random() < 0.5 else b.tip_in)(b.to_right[e], int(rng.choice(lens)))
    scaffolds, i = [], 0
    while i < n_chains:                                                      # two to four chains in a row, gaps between them
        n = int(rng.integers(2, 5)); scaffolds.append(chains[i:i + n]); i += n
    for _ in range(read_pairs):
        sc = scaffolds[int(rng.integers(0, len(scaffolds)))]
        flat = [(e, c) for c, ch in enumerate(sc) for e in ch]
        piece = lambda at, n: [e for e, c in flat[at:at + n] if c == flat[at][1]]       # a read does not cross a gap
        at = int(rng.integers(0, len(flat)))
        a = piece(at, int(rng.integers(1, 5))) if rng.random() < 0.9 else []
        at2 = min(len(flat) - 1, at + int(rng.integers(0, 5)))
        m = piece(at2, int(rng.integers(1, 5))) if rng.random() < 0.9 else []
        bad = rng.random() < 0.15
        sums = (int(rng.choice([151, 65535])), int(rng.choice([0, 150, 151, 65535]))) if bad else (int(rng.choice([0, 150])), int(rng.choice([0, 150])))
        b.pair(a, m, int(rng.integers(0, 6)), sums=sums if rng.random() < 0.5 else sums[::-1], swap=rng.random() < 0.5)
    _motifs(b)
    if dense: _dense(b)
    on = {g for p in b.paths for g in p}
    for e in range(len(b.kmers)):                                            # no edge without a read: a lone read, one barcode, decides nothing
        if e <= b.inv[e] and e not in on and b.inv[e] not in on: b.pair([e], [], 1)
    return b.case()


def moved(c, knob):
    """the graph with one knob moved to the other side of its threshold: (case, sums) -- the oracle's `bad` recomputed from the sums"""
    kind, where, there = knob
    d = dict(c)
    if kind == "kmers":
        d["kmers"] = list(c["kmers"])
        for e in where: d["kmers"][e] = there
    elif kind == "paths":
        d["paths"] = list(c["paths"])
        for i in where: d["paths"][i] = list(there)
    else:
        d["sums"] = c["sums"].copy()
        for i in where: d["sums"][i] = there
        d["bad"] = ((d["sums"][0::2] > 150) | (d["sums"][1::2] > 150)).astype(np.uint8)
    return d


def run(c, one_good=False, K=None):
    return hops_oracle.run(c["paths"], c["kmers"], c["inv"], c["to_left"], c["to_right"], c["bc"], c["bad"], K or c["K"], bool(one_good))


_seeded = {}


def seeded():
    """every seeded graph, old and new: [(name, case, K, capacities)], made once and handed out unchanged.  An old graph has no
    `sums`: its marks are all there is"""
    if not _seeded:
        for seed, ep, vp, rp, K, caps in SPECS:
            _seeded[f"seed{seed}"] = (make(seed, ep, vp, rp, K), K, caps)
        for name, seed, nc, rp, K, dense, caps in CHAIN_SPECS:
            _seeded[name] = (make_chains(seed, nc, rp, K, dense), K, caps)
    return [(name, c, K, caps) for name, (c, K, caps) in _seeded.items()]


def overflowing(r, max_seqs, max_len):
    """the searched edges that do not fit capacities (max_seqs, max_len) -- from the oracle's own sizes of their sets -- with the capacities
    each outgrows (dfk_hops.h OVER_*: the device names the first it meets, this names all)"""
    ext_len = max(32, 2 * max(1, max_len))
    out = {}
    for e, (nx, lx, most, le) in r["x_sizes"].items():
        why = [w for w, over in (("X_SLOTS", nx > max(1, max_seqs) - 1), ("X_LEN", lx > max(1, max_len)), ("EXT_SLOTS", most > EXT_SLOTS - 1), ("EXT_LEN", le > ext_len)) if over]
        if why: out[e] = why
    return out


def overflows(r, max_seqs, max_len):
    """how many searched edges do not fit capacities (max_seqs, max_len) -- from the oracle's own sizes of their sets"""
    return len(overflowing(r, max_seqs, max_len))


def case_text(name, c, K, caps, one_goods=(0, 1)):
    """the lines of one graph: its inputs once (c = dict(kmers, inv, to_left, to_right, paths, bc, bad, n_vertices)), then per
    variant (ONE_GOOD, capacities) a `variant` line and what the oracle expects of it"""
    ints = lambda v: " ".join(str(int(x)) for x in v)
    flat = lambda p: ints([len(p)] + [x for ab in p for x in ab])
    out = [f"graph {name} {K}", f"{len(c['kmers'])} {c['n_vertices']} {len(c['paths'])}"]
    for k in ("kmers", "inv", "to_left", "to_right", "bc", "bad"):
        out.append(ints(c[k]))
    for p in c["paths"]:
        out.append(ints([len(p)] + list(p)))
    for one_good in one_goods:
        r = hops_oracle.run(c["paths"], c["kmers"], c["inv"], c["to_left"], c["to_right"], c["bc"], c["bad"], K, bool(one_good))
        for max_seqs, max_len in caps:
            out.append(f"variant {one_good} {max_seqs} {max_len}")
            for k in ("m1", "m2", "m3", "pairs"):
                out.append(flat(r[k]))
            out.append(ints([r["searched"], r["extended"], r["most_rounds"], r["largest_x"], r["largest_exts"], r["longest"], overflows(r, max_seqs, max_len)]))
            out.append("%d %d" % r["digest"])
    return out


def text():
    out = []
    for name, c, K, caps in seeded():
        out += case_text(name, c, K, caps)
    return "\n".join(out) + "\n"


if __name__ == "__main__":
    open(FILE, "w").write(text())
    print(FILE, os.path.getsize(FILE), "bytes")
