"""Six seeded small graphs with paired reads on them, and the text file tests/cpp/hops_cases.txt in which tests/hops_oracle.py's
answers for them (24 recorded cases: each graph with ONE_GOOD off and on, under one to three capacities) are recorded for tests/cpp/test_hops.cc (superplus_amd/csrc/dfk_hops.h, the C++ restatement of FindEdgePairs).

    python -m tests.hops_cases            rewrites tests/cpp/hops_cases.txt

The graphs are not assemblies of anything: vertices come in reverse-complement pairs (v, v ^ 1), an edge u -> v has the
involuted edge (v ^ 1) -> (u ^ 1), now and then an edge u -> u ^ 1 is its own involution; edge lengths are drawn from the
thresholds' neighbourhoods (1, 39/40, 99/100, 120/121 k-mers).  A pair of reads is two pieces of one walk, the second read
on the other strand, so that mates land where the rule looks for them."""
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


def overflows(r, max_seqs, max_len):
    """how many searched edges do not fit capacities (max_seqs, max_len) -- from the oracle's own sizes of their sets"""
    ext_len = max(32, 2 * max(1, max_len))
    return sum(1 for nx, lx, most, le in r["x_sizes"].values() if nx > max(1, max_seqs) - 1 or lx > max(1, max_len) or most > EXT_SLOTS - 1 or le > ext_len)


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
    for seed, ep, vp, rp, K, caps in SPECS:
        out += case_text(f"seed{seed}", make(seed, ep, vp, rp, K), K, caps)
    return "\n".join(out) + "\n"


if __name__ == "__main__":
    open(FILE, "w").write(text())
    print(FILE, os.path.getsize(FILE), "bytes")
