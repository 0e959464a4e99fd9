"""Seeded inputs of the subset of interest (tests/subset_oracle.py): small graphs with chosen pairs and paths, for
tests/cpp/test_subset.cc (recorded in tests/cpp/subset_cases.txt, the C++ restatement of superplus_amd/csrc/dfk_subset.h against the numpy
one) and for tests/test_gpu_subset.py (dfk_subset_build_arrays).  `python -m tests.subset_cases` rewrites the recorded file.

A case: E edges of which the last n_self are their own involution (the others pair up, e ^ 1), N reads with random paths of 0 to 4
edges, and in front of them -- where there are 16 reads and both a marked and an unmarked edge -- sixteen planted reads that hold every
branch of the rule whatever the seed gave:
   pair 0  [m, u] | [u]        taken through its even read only         pair 4  [u, u] | [u]     placed, no mark: not taken
   pair 1  [u] | [u, m]        ... through its odd read only            pair 5  [m, s, m] | [m]  both hit; m crossed twice
   pair 2  [] | [m]            an unplaced read whose mate hits         pair 6  [s, s, s] | [u]  s crossed three times
   pair 3  [] | []             two unplaced mates: not taken            pair 7  [u] | []         not taken
(m: the first marked edge that is not its own involution, s: a marked self-inverse edge, or m where there is none, u: the first
unmarked edge)."""
import os

import numpy as np

from tests import subset_oracle

FILE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "cpp", "subset_cases.txt")

# name, seed, E, n_self, N, pairs ("some", "none", "all", "twice"), recorded for the C++ test
SPECS = [("selfinv", 1, 14, 2, 64, "some", True), ("plain", 2, 8, 0, 40, "some", True), ("dense", 3, 64, 4, 400, "some", True),
         ("no-pairs", 4, 20, 0, 48, "none", True), ("every-edge", 5, 12, 2, 48, "all", True), ("twice-and-reversed", 6, 32, 2, 96, "twice", True),
         ("no-reads", 7, 16, 0, 0, "some", True), ("one-pair-of-reads", 8, 10, 0, 2, "some", True),
         ("three-scan-tiles", 9, 48, 2, 4500, "some", False)]


def make(seed, E, n_self, N, kind):
    rng = np.random.RandomState(seed)
    assert (E - n_self) % 2 == 0 and N % 2 == 0
    inv = [e ^ 1 for e in range(E - n_self)] + list(range(E - n_self, E))
    if kind == "none": pairs = []
    elif kind == "all": pairs = [(e, E - 1 - e) for e in range(E)]
    else:
        pairs = [(int(rng.randint(E)), int(rng.randint(E))) for _ in range(max(1, E // 10))]
        if n_self: pairs.append((E - 1, int(rng.randint(E - n_self))))      # a self-inverse edge named in a pair
        if kind == "twice": pairs += [pairs[0], (pairs[0][1], pairs[0][0])]
    m = subset_oracle.mark_edges(pairs, inv)
    paths = []
    for _ in range(N):
        n = 0 if rng.rand() < 0.2 else int(rng.randint(1, 5))
        paths.append([int(x) for x in rng.randint(E, size=n)])
    marked = [e for e in range(E - n_self) if m[e]]
    unmarked = [e for e in range(E) if not m[e]]
    planted = N >= 16 and bool(marked) and bool(unmarked)
    if planted:
        a, u = marked[0], unmarked[0]
        s = next((e for e in range(E - n_self, E) if m[e]), a)
        paths[:16] = [[a, u], [u], [u], [u, a], [], [a], [], [], [u, u], [u], [a, s, a], [a], [s, s, s], [u], [u], []]
    return dict(inv=inv, paths=paths, pairs=pairs, planted=planted, n_self=n_self)


def seeded():
    """[(name, case, recorded)]"""
    return [(name, make(seed, E, n_self, N, kind), rec) for name, seed, E, n_self, N, kind, rec in SPECS]


def case_text(name, c):
    r = subset_oracle.run(c["paths"], c["inv"], c["pairs"])
    first = np.concatenate([[0], np.cumsum([len(p) for p in c["paths"]])]).astype(np.int64)
    row = lambda v: " ".join(str(int(x)) for x in v)
    return ["case %s %d %d %d" % (name, len(c["inv"]), len(c["paths"]), len(c["pairs"])), row(c["inv"]), row(first), row([e for p in c["paths"] for e in p]),
            row([e for p in c["pairs"] for e in p]), "%d %s" % (len(r["eoi"]), row(r["eoi"])), "%d %s" % (len(r["ids"]), row(r["ids"])),
            "%d %d %d %d" % (r["path_entries"], r["index_entries"], r["one_read_only"], r["unplaced"]), row(r["index_first"])]


def text():
    out = []
    for name, c, rec in seeded():
        if rec: out += case_text(name, c)
    return "\n".join(out) + "\n"


if __name__ == "__main__":
    open(FILE, "w").write(text())
