"""tests/patch_cases.py -- TEST INFRASTRUCTURE: hand-made graphs at K = 48 with closures for the patched graph (tests/patch_oracle.py,
superplus_amd/csrc/dfk_patch.h), and tests/cpp/patch_cases.txt recorded from them (python -m tests.patch_cases).

A case's graph is the unipath graph of a few contigs (their K-mers with the contexts the contigs show, through oracle/graph_oracle.py), so it
holds together as the reference's does.  The plants, by case (tests/test_patch_oracle.py asserts what each fires):
  plain      two contigs, no closures: hb3 is the graph, every path one id, every left3 0
  join       a closure from a sink's end through 22 novel bases to a source's start: three things become one edge, the second old edge gets
             left3 > 0; 75 closure positions: three batches of 37
  interior   one closure leaves c1's interior and re-enters c2's, another leaves c2's interior further on: c1 splits in two, c2 in three --
             and so do their inverses
  onlyold    a closure lying wholly on c1: nothing new, no bit added
  bit        c2 repeats 47 bases of c1's interior; a closure of K + 1 bases shows c1's K-mer beside c2's: nothing new, two bits added, both
             edges split
  lengths    novel closures of K - 1, K and K + 1 bases: nothing, a one-K-mer edge with an empty context, a two-K-mer edge
  reversed   join's closure given reverse-complemented: join's graph
  selfrc     a closure equal to its own reverse complement: its middle K-mer is a novel palindrome, a one-K-mer edge
  twice      join's closure twice and a closure sharing 30 of its novel K-mers, then leaving
  cycle      a closure from a contig's end to its own start: a branch-free cycle through the cycle kernels, the old edge's path [c, c]
  selfinv    a contig through a palindromic K-mer: a self-inverse old edge; a closure leaves the contig before it
  cross      three contigs through one (K-1)-mer: a vertex with 2 x 2 crossings, one of which no contig shows
  random     graph_oracle on seeded reads from superplus_amd/synth.py, with closures between real edge ends and pure noise
The refusals (inv no involution, an end out of range, an edge shorter than K, an edge whose inverse is not its reverse complement, vertex ends that disagree, a K-mer on two canonical edges) are
made from `plain` by refusals()."""
import os

import numpy as np

from oracle import graph_oracle as go
from tests import patch_oracle as po

K = 48
FILE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "cpp", "patch_cases.txt")


def rnd(seed, n):
    return bytes(np.random.default_rng(seed).integers(0, 4, n, dtype=np.uint8))


def graph_of(contigs, K=K):
    d = {}
    for c in contigs:
        po.kmerize(c, K, d); po.kmerize(go.rc_seq(c), K, d)
    return graph_of_solid(po.solid_of(d, K), K)


def graph_of_solid(solid, K):
    edges, _ = go.build_edges(solid, K)
    h = go.build_hbv(edges, K)
    L, R = h.to_left_right()
    return dict(K=K, edges=list(h.edges), inv=h.involution(), to_left=L, to_right=R, n_vertices=len(h.frm))


def hand_made():
    c1, c2, c3, c4 = rnd(1, 200), rnd(2, 170), rnd(3, 150), rnd(4, 150)
    nov = rnd(9, 60)
    join = c1[-50:] + nov[:22] + c2[:50]
    x = rnd(12, 40)
    pal = rnd(13, 24); pal = pal + go.rc_seq(pal)
    other = lambda b: bytes([(b + 1) & 3])                                  # (the repeat's neighbours differ from c1's: the K-mers beside it are c2's own)
    c2b = rnd(5, 59) + other(c1[100]) + c1[101:148] + other(c1[148]) + rnd(6, 59)
    m = rnd(20, 47)
    out = [
        ("plain", [c1, c2], []),
        ("join", [c1, c2], [join]),
        ("interior", [c1, c2], [c1[50:110] + nov[:20] + c2[40:100], c2[60:130] + nov[30:52]]),
        ("onlyold", [c1, c2], [c1[20:120]]),
        ("bit", [c1, c2b], [c1[100:148] + c2b[107:108]]),
        ("lengths", [c1], [rnd(30, K - 1), rnd(31, K), rnd(32, K + 1)]),
        ("reversed", [c1, c2], [go.rc_seq(join)]),
        ("selfrc", [c1], [x + go.rc_seq(x)]),
        ("twice", [c1, c2], [join, join, c1[-50:] + nov[:22] + c2[:8] + rnd(33, 30)]),
        ("cycle", [c4], [c4[-60:] + nov[:10] + c4[:60]]),
        ("selfinv", [rnd(14, 60) + pal + rnd(15, 60), c3], [c3[-50:] + nov[:5] + (rnd(14, 60) + pal)[:70]]),
        ("cross", [rnd(21, 80) + m + rnd(22, 80), rnd(23, 80) + m + rnd(24, 80), (rnd(21, 80) + m)[-48:] + rnd(24, 80)[:40]], []),
    ]
    return [(name, graph_of(contigs), closures) for name, contigs, closures in out]


def random_case(oracle):
    from superplus_amd import synth
    genome = synth.make_genome(2500, 71, repeat_frac=0.05)
    rs = synth.make_reads(genome, 260, 72).numpy()
    ref = oracle.run(rs["packed"], rs["base_off"], rs["read_len"], rs["pq_bytes"], rs["pq_off"], rs["bc"], K=K)
    g = graph_of_solid(ref["solid"], K)
    rng = np.random.default_rng(73)
    E = len(g["edges"])
    to, frm = po.adjacency(g)
    sinks = [e for e in range(E) if not frm[g["to_right"][e]]] or list(range(E))
    sources = [e for e in range(E) if not to[g["to_left"][e]]] or list(range(E))
    closures = []
    for i in range(6):
        a, b = g["edges"][sinks[int(rng.integers(len(sinks)))]], g["edges"][sources[int(rng.integers(len(sources)))]]
        closures.append(bytes(a[-int(rng.integers(48, 70)):]) + rnd(80 + i, int(rng.integers(0, 12))) + bytes(b[:int(rng.integers(48, 70))]))
    closures += [rnd(90, 70), rnd(91, 20), closures[0]]
    e = g["edges"][int(rng.integers(E))]
    closures.append(bytes(e[:min(len(e), 90)]))
    return ("random", g, closures)


def all_cases(oracle=None):
    if oracle is None:
        from oracle import pyoracle as oracle
    return hand_made() + [random_case(oracle)]


def refusals():
    """(name, graph) that dfk_patch_build_arrays and check_graph refuse; the last holds together but has a K-mer on two canonical edges"""
    g = hand_made()[0][1]
    def change(**kw): return dict(g, **{k: f(list(g[k])) for k, f in kw.items()})
    def setat(i, v): return lambda a: a[:i] + [v] + a[i + 1:]
    two = graph_of([rnd(1, 200), rnd(2, 170)])
    # a third contig repeated as edges of its own: its K-mers lie on c1's edge too
    n, nv = len(two["edges"]), two["n_vertices"]
    piece = bytes(two["edges"][0][10:80])
    dup = dict(two, edges=two["edges"] + [piece, go.rc_seq(piece)], inv=two["inv"] + [n + 1, n], to_left=two["to_left"] + [nv, nv + 2], to_right=two["to_right"] + [nv + 1, nv + 3],
               n_vertices=nv + 4)
    return [("inv", change(inv=setat(0, 0) if g["inv"][0] != 0 else setat(0, 1))), ("end", change(to_right=setat(1, g["n_vertices"]))),
            ("short", change(edges=setat(0, g["edges"][0][:K - 1]))), ("notrc", change(edges=setat(0, g["edges"][0][:100] + bytes([g["edges"][0][100] ^ 1]) + g["edges"][0][101:]))), ("vertex", change(to_left=setat(0, g["to_left"][1]))), ("twice", dup)]


# ----------------------------------------------------------------------------------------------- the recorded form
def digits(s):
    return "".join(map(str, s)) or "-"


def ints(v):
    return " ".join(str(int(x)) for x in v) or "-"


def portable(r):
    """the oracle's result with hb3's ids as 2 * (place in HBVFromEdges' order) + rc: what dfk_patch.h's literal form names them"""
    h, edges = r["hbv"], r["edges3"]
    order = sorted(range(len(edges)), key=lambda i: (-len(edges[i]), edges[i]))
    place = {i: p for p, i in enumerate(order)}
    name = {}
    for i in range(len(edges)):
        name[h.fwd[i]] = 2 * place[i]
        if h.rev[i] != h.fwd[i]:
            name[h.rev[i]] = 2 * place[i] + 1
    return [edges[i] for i in order], [[name[x] for x in p] for p in r["to3"]]


COUNTERS = ("crossings", "short", "positions", "found", "new", "new_unique", "bits_added", "kmers3", "single3")


def case_text(name, g, closures, r):
    edges3, to3 = portable(r)
    first = np.concatenate([[0], np.cumsum([len(p) for p in to3])])
    return ["case " + name, ints([g["K"], g["n_vertices"], len(g["edges"]), len(closures), len(edges3)]), ints(g["inv"]), ints(g["to_left"]), ints(g["to_right"])] + \
           [digits(s) for s in g["edges"]] + [digits(s) for s in closures] + [digits(s) for s in edges3] + \
           [ints(first), ints([x for p in to3 for x in p]), ints(r["left3"]), ints([r["counters"][k] for k in COUNTERS])]


def text(oracle=None):
    out = []
    for name, g, closures in all_cases(oracle):
        out += case_text(name, g, closures, po.run(g, closures))
    for name, g in refusals():
        out += ["refuse " + name, ints([g["K"], g["n_vertices"], len(g["edges"])]), ints(g["inv"]), ints(g["to_left"]), ints(g["to_right"])] + [digits(s) for s in g["edges"]]
    return "\n".join(out) + "\n"


if __name__ == "__main__":
    open(FILE, "w").write(text())
