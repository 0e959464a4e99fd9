"""Seeded inputs of the closures (tests/closures_oracle.py): tests/cons_cases.py's kind of case -- a small graph with chosen closer
tables, partner records, pairs, reads and qualities -- and per pair a chosen list of offsets, for tests/cpp/test_closures.cc (recorded in
tests/cpp/closures_cases.txt: the C++ restatement of superplus_amd/csrc/dfk_closures.h against the Python one) and for
tests/test_gpu_closures.py (dfk_closures_build_arrays).  `python -m tests.closures_cases` rewrites the recorded file.

`planted` holds what the fixtures lack (they have one offset a pair and nothing else).  K = 48; edges 2 x and 2 x + 1 are each other's
involution, the last edge its own.  Pair (A, inv[B]) has es = {A, B}: side 0 is stack A as built, side 1 stack B REVERSED, so a
forward row of B with base b at its stack's last column shows 3 - b at output column 0.  Every row is forward; W<n> is a stack made
n columns wide by a read ending at column n.  The pairs, in order, with their offsets:
   0  (X0, X1) [0]         the cross-boundary column: stack 0 gives base 0 Q20 and base 1 Q2, stack 1 base 0 Q0, Q0 and base 1 Q10, Q10:
                           in row order 20.200000000000003 against 20.2 -- base 0; per-stack sums added tie at 20.2 and give base 1.
   1  (TIE, F) [0]         stack 1 has no rows: column 0 ties base 0 with 2 at Q10 -- 2, where con1 of a.close.cons holds 0; columns 1
                           and 2 hold nothing -- 3, where con1 holds 0.
   2  (W256, V256) [0, 1]  two offsets, two closures in order: 256 and 257 columns.
   3  (W256, V256) [256]   the same pair again; abutting, off == cols1: 512 columns.
   4  (W256, V256) [-256]  abutting, off == -cols2: 512 columns.
   5  (T1, V313) [200]     513 columns; T1 is 450 wide and trimmed to 400.
   6  (T1, V313) [10]      stack 1 wholly inside stack 0: right_ext2 = 77.
   7  (W256, T2) [-50]     stack 0 wholly inside stack 1 (T2 trimmed to 400): left_ext1 = 50, right_ext1 = 94; cols1 != cols2.
   8  (T1, T2) [392]       both stacks trimmed: 792 columns.
   9  (W256, V256) [0, 1, 2]   three offsets: none.
  10  (W256, V256) []      no offset: none.
  11  (S, S) [3]           the self-inverse edge: e1 == inv[e2], side 0 reversed too, both sides the same rows.
  12  (F, F2) [0]          two stacks without rows, 0 columns wide: a closure of no bases, rowless.
  13  (U1, U2) [100]       two stacks trimmed to 400 whose only row is a read without bases: both erased; 500 columns of base 3, rowless.
  14  (TIE, U1) [-20]      one side erased by Trim: its columns alone give 3.
T1 also holds a row that is defined (Q63, Q64) in front of the window and undefined (Q128, Q190) inside it: live, walked, and erased.
The read R stands in rows of W256 and of V256; the reads hold the qualities 0, 1, 2, 127, 128 and 190 (255 does not fit a PQVec block
beside 63: tests/cons_cases.py)."""
import os

import numpy as np

from tests import closures_oracle, cons_cases, cons_oracle
from tests.closer_oracle import closer_edges
from tests.cons_cases import K, rand_bases, rand_quals

FILE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "cpp", "closures_cases.txt")

PLANTED_OFFSETS = [[0], [0], [0, 1], [256], [-256], [200], [10], [-50], [392], [0, 1, 2], [], [3], [0], [100], [-20]]


def planted():
    rng = np.random.RandomState(21)
    names = ["X0", "X1", "TIE", "F", "F2", "W256", "V256", "T1", "T2", "V313", "U1", "U2"]
    edge = {n: 2 * i for i, n in enumerate(names)}
    E = 2 * len(names) + 1
    S = E - 1
    edge["S"] = S
    inv = [e ^ 1 for e in range(E - 1)] + [S]
    kmers = [10] * E
    reads, quals = [], []

    def read(b, q):
        reads.append(np.asarray(b, np.uint8)); quals.append(np.asarray(q, np.uint8))
        reads.append(rand_bases(rng, 5)); quals.append(rand_quals(rng, 5))            # its mate
        return len(reads) - 2

    locs = {n: [] for n in names + ["S"]}
    locs["X0"] = [(read([0], [20]), 0, True), (read([1], [2]), 0, True)]
    locs["X1"] = [(read([3], [0]), 0, True), (read([3], [0]), 0, True), (read([2], [10]), 0, True), (read([2], [10]), 0, True)]
    locs["TIE"] = [(read([0], [10]), 0, True), (read([2], [10]), 0, True), (read([1, 3], [37, 1]), 3, True)]
    R = read(rand_bases(rng, 100), rand_quals(rng, 100))
    locs["W256"] = [(read(rand_bases(rng, 80), rand_quals(rng, 80)), 0, True), (R, 156, True), (read(rand_bases(rng, 60), rand_quals(rng, 60)), 120, True)]
    locs["V256"] = [(R, 20, True), (read(rand_bases(rng, 151), rand_quals(rng, 151)), 105, True), (read(rand_bases(rng, 30), rand_quals(rng, 30)), -10, True)]
    gone = np.asarray([63, 64] * 25 + [128, 190] * 5, np.uint8)                      # defined in front of the window, undefined inside it: live, and erased
    locs["T1"] = [(read(rand_bases(rng, 120), rand_quals(rng, 120)), 330, True), (read(rand_bases(rng, 151), rand_quals(rng, 151)), 100, True), (read(rand_bases(rng, 40), rand_quals(rng, 40)), 0, True),
                  (read(rand_bases(rng, 60), gone), 0, True)]
    locs["T2"] = [(read(rand_bases(rng, 151), rand_quals(rng, 151)), 270, True), (read(rand_bases(rng, 151), rand_quals(rng, 151)), 200, True), (read(rand_bases(rng, 90), rand_quals(rng, 90)), 10, True)]
    locs["V313"] = [(read(rand_bases(rng, 151), rand_quals(rng, 151)), 162, True), (read(rand_bases(rng, 151), rand_quals(rng, 151)), 3, True)]
    locs["S"] = [(read(rand_bases(rng, 8), [0, 1, 2, 127, 0, 1, 2, 127]), 2, True), (read(rand_bases(rng, 8), [63, 128, 190, 63, 128, 190, 63, 63]), 0, True)]
    locs["U1"] = [(read([], []), 500, True)]                                          # a read without bases: it gives M its position and the stack no cell
    locs["U2"] = [(read([], []), 430, True)]
    e = lambda a, b: (edge[a], inv[edge[b]])
    pairs = [e("X0", "X1"), e("TIE", "F"), e("W256", "V256"), e("W256", "V256"), e("W256", "V256"), e("T1", "V313"), e("T1", "V313"), e("W256", "T2"), e("T1", "T2"),
             e("W256", "V256"), e("W256", "V256"), (S, S), e("F", "F2"), e("U1", "U2"), e("TIE", "U1")]
    ce = closer_edges(pairs, inv)
    per = [next((locs[n] for n in locs if edge[n] == x), []) for x in ce]
    parts = [[] for _ in range(2 * len(pairs))]
    parts[2 * 5 + 1] = [(R, 250, True)]                                               # pushed by side 1 of pair 5 onto locs[0]: a partner row of stack T1
    return dict(inv=inv, kmers=kmers, ce=ce, locs=per, parts=parts, pairs=pairs, reads=reads, quals=quals, edge=edge, offsets=[list(o) for o in PLANTED_OFFSETS])


def with_offsets(c, seed, counts, always=False):
    """a tests/cons_cases.py case and, per pair, offsets drawn inside [-cols2, cols1]"""
    rng = np.random.RandomState(seed)
    r = cons_oracle.run(c["inv"], c["kmers"], K, c["ce"], c["locs"], c["parts"], c["pairs"], lambda id: c["reads"][id], lambda id: c["quals"][id])
    offs = []
    for pi in range(len(c["pairs"])):
        cols1, cols2 = r["dims"][2 * pi][3], r["dims"][2 * pi + 1][3]
        n = int(rng.choice(counts))
        offs.append(sorted(int(rng.randint(-cols2, cols1 + 1)) for _ in range(n)) if not always else [0] * n)
    return dict(c, offsets=offs)


# name, recorded
SPECS = [("planted", True), ("random", True), ("random-long", True), ("no-pairs", True), ("none-closable", True), ("many-rows", False), ("many-closures", False)]
_made = {}


def seeded():
    """[(name, case, recorded)]"""
    if not _made:
        base = {n: c for n, c, _ in cons_cases.seeded()}
        _made["planted"] = planted()
        _made["random"] = with_offsets(base["random"], 31, [0, 1, 1, 1, 2, 2, 3])
        _made["random-long"] = with_offsets(base["random-long"], 32, [1, 1, 2, 2, 4])
        _made["no-pairs"] = with_offsets(base["no-pairs"], 33, [1])
        _made["none-closable"] = with_offsets(base["random"], 34, [0, 3, 5])
        _made["many-rows"] = with_offsets(base["many-rows"], 35, [1], always=True)            # a stack of 5 000 rows, its pair closable
        _made["many-closures"] = with_offsets(base["many-stacks"], 36, [2], always=True)      # 2 x 2 103 closures: more than two tiles of device_scan
    return [(name, _made[name], rec) for name, rec in SPECS]


_oracle = {}


def oracle(name, c):
    if name not in _oracle:
        _oracle[name] = closures_oracle.run(c["inv"], c["kmers"], K, c["ce"], c["locs"], c["parts"], c["pairs"], c["offsets"], lambda id: c["reads"][id], lambda id: c["quals"][id],
                                            keep_sums=name == "planted")
    return _oracle[name]


def arrays(c):
    """the case as dfk_closures_build_arrays takes it: (cons_cases.arrays' dict, off_first, offsets)"""
    return (cons_cases.arrays(c),) + closures_oracle.off_arrays(c["offsets"])


def case_text(name, c, r, K_=K):
    """a case and what the oracle says of it, as tests/cpp/test_closures.cc reads it: tests/cons_cases.py's thirteen lines of input, the
    offsets, the result"""
    row = lambda v: " ".join(str(int(x)) for x in v)
    none = dict(starts=[], dims=[], bases=[], rows=0, live=0, rows_kept=0, trimmed=0, reversed=0, columns=0, added=0)
    first, offs = closures_oracle.off_arrays(c["offsets"])
    return cons_cases.case_text(name, c, none, K_)[:13] + [
        row(first), row(offs), row(r["pair_first"]), row(r["starts"]), row([x for rec in r["records"] for x in rec]), "".join(str(int(b)) for b in r["bases"]) or "-",
        "%d %d %d %d %d %d %d %d" % (r["closable"], r["over"], r["columns"], r["added"], r["live"], r["empty"], r["short"], r["rowless"])]


def text(recorded=True):
    out = []
    for name, c, rec in seeded():
        if rec == recorded: out += case_text(name, c, oracle(name, c))
    return "\n".join(out) + "\n"


if __name__ == "__main__":
    open(FILE, "w").write(text())
