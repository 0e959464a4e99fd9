"""Seeded inputs of the closers' read sets (tests/closer_oracle.py): small graphs with chosen pairs, paths, offsets and duplicate marks,
for tests/cpp/test_closer.cc (recorded in tests/cpp/closer_cases.txt: the C++ restatement of superplus_amd/csrc/dfk_closer.h against the
Python one) and for tests/test_gpu_closer.py (dfk_closer_build_arrays).  `python -m tests.closer_cases` rewrites the recorded file.

A case: E edges of which the last n_self are their own involution (the others pair up, e ^ 1), k-mer counts equal on an edge and its
involution, N reads with random paths of 0 to 4 edges drawn from edges 14 and up and random offsets, random duplicate marks.  A
`planted` case (E >= 24, n_self = 2, N >= 64, K = 48) has edges 0 .. 13 to itself and these pairs and reads, S = E - 1 the last
self-inverse edge:
   pairs (0, 3) (S, 5) (1, 7) (10, 11), then (0, 3) again and (3, 0)
       closer edges 0 and 2 = inv[3]; S and 4; 1 and 6 (so 0 and inv[0] = 1 both are); 10 twice (nobody crosses 10 or 11); 3 and 1
   r0  = [0, 8, 0]  crosses edge 0 twice: 4 records in locs(0)               r1 = []
   r2  = [S, S, S]  crosses S three times: 9 records a pass, S its own involution: 18 in locs(S)
   r4  = [2, 2, 12], r6 = r8 = r10 = [2, 12]    prec of edge 2 holds (12, kmers[2]) 2 + 3 = 5 times: an anchor through r4's double
                                                listing alone (it would be 4)
   r12 = r14 = r16 = r18 = [2, 13]              (13, kmers[2]) 4 times: no anchor
   kmers[6] = 700: kmers + K - 1 - pos1 = 747 - offset
   r20 = [6] at offset -53: 800, its mate r21 = [] is let in       r22 = [6] at offset -54: 801, r23 = [] is not
   r24 = [6], pair 12 marked a duplicate: in locs(6), not in reads(6), and r25 = [] is not let in
   r26 = [0] and r27 = [0], both at offset 0: r27 is in reads(0) as (27, true) from the list and as (27, false) as r26's mate
(the odd reads not named are unplaced; pairs 0 .. 13 but pair 12 are unmarked)."""
import os

import numpy as np

from tests import closer_oracle

FILE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "cpp", "closer_cases.txt")
K = 48

# name, seed, E, n_self, N, pairs ("planted", "some", "none", "all"), recorded for the C++ test
SPECS = [("planted", 1, 26, 2, 96, "planted", True), ("planted-more", 2, 40, 2, 300, "planted", True), ("plain", 3, 28, 0, 80, "some", True),
         ("every-edge", 4, 20, 2, 60, "all", True), ("no-pairs", 5, 24, 0, 48, "none", True), ("no-reads", 6, 24, 2, 0, "some", True),
         ("one-pair-of-reads", 7, 20, 0, 2, "some", True),
         ("over-256", 8, 20, 2, 1200, "all", False),              # an edge with more than 256 records
         ("over-1024", 9, 18, 0, 5000, "all", False)]            # ... with more than 1024; more reads than two tiles of device_scan, more records in a range than two of the sort


def make(seed, E, n_self, N, kind):
    rng = np.random.RandomState(seed)
    assert (E - n_self) % 2 == 0 and N % 2 == 0
    inv = [e ^ 1 for e in range(E - n_self)] + list(range(E - n_self, E))
    kmers = [0] * E
    for e in range(E):
        if inv[e] >= e: kmers[e] = kmers[inv[e]] = int(rng.randint(1, 400))
    planted = kind == "planted"
    lo = 14 if planted else 0
    if kind == "none": pairs = []
    elif kind == "all": pairs = [(e, int(rng.randint(E))) for e in range(E)]
    else: pairs = [(int(rng.randint(lo, E)), int(rng.randint(lo, E))) for _ in range(max(1, E // 6))]
    paths, offsets = [], []
    for _ in range(N):
        n = 0 if rng.rand() < 0.2 else int(rng.randint(1, 5))
        paths.append([int(x) for x in rng.randint(lo, E, size=n)])
        offsets.append(int(rng.randint(-150, 300)) if n else 0)
    dup = [bool(rng.rand() < 0.1) for _ in range(N // 2)]
    if planted:
        assert E >= 24 and n_self == 2 and N >= 64
        S = E - 1
        kmers[6] = kmers[7] = 700
        pairs = [(0, 3), (S, 5), (1, 7), (10, 11)] + pairs + [(0, 3), (3, 0)]
        plant = {0: [0, 8, 0], 2: [S, S, S], 4: [2, 2, 12], 6: [2, 12], 8: [2, 12], 10: [2, 12], 12: [2, 13], 14: [2, 13], 16: [2, 13], 18: [2, 13],
                 20: [6], 22: [6], 24: [6], 26: [0], 27: [0]}
        for i in range(28):
            paths[i] = list(plant.get(i, []))
            offsets[i] = 0
        offsets[20], offsets[22] = -53, -54
        for i in range(14): dup[i] = i == 12
    return dict(inv=inv, kmers=kmers, paths=paths, offsets=offsets, pairs=pairs, dup=dup, K=K, planted=planted)


def seeded():
    """[(name, case, recorded)]"""
    return [(name, make(seed, E, n_self, N, kind), rec) for name, seed, E, n_self, N, kind, rec in SPECS]


def oracle(c, index=None):
    return closer_oracle.run(c["paths"], c["offsets"], c["kmers"], c["inv"], c["pairs"], c["dup"], c["K"], index)


def case_text(name, c, r=None):
    """a case and what the oracle says of it, as tests/cpp/test_closer.cc reads it"""
    if r is None: r = oracle(c)
    first = np.concatenate([[0], np.cumsum([len(p) for p in c["paths"]])]).astype(np.int64)
    row = lambda v: " ".join(str(int(x)) for x in v)
    return ["case %s %d %d %d %d" % (name, len(c["inv"]), len(c["paths"]), len(c["pairs"]), c["K"]), row(c["inv"]), row(c["kmers"]), row(first),
            row([e for p in c["paths"] for e in p]), row(c["offsets"]), row([e for p in c["pairs"] for e in p]), row(c["dup"]),
            row(r["ce"]), row(r["loc_first"]), row(r["anchor_first"]), row(r["read_first"]),
            row([x for l in r["locs"] for x in l]), row([x for a in r["anchors"] for x in a]), row(closer_oracle.read_words(r["reads"])),
            "%d %d %d %d" % (r["prec"], r["mates_in"], r["mates_out"], r["dup_skipped"])]


def text(recorded=True):
    out = []
    for name, c, rec in seeded():
        if rec == recorded: out += case_text(name, c)
    return "\n".join(out) + "\n"


if __name__ == "__main__":
    open(FILE, "w").write(text())
