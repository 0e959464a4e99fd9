"""Seeded inputs for GetOffsets1 (tests/offsets_oracle.py, superplus_amd/csrc/dfk_offsets.h, the kernels): pairs of consensus sequences
of at most 400 bases that fire what the four fixtures never do -- the thresholds of the bits test, invalidation, big near small, bad
windows, a window of nothing but mismatches, pairs with many surviving offsets -- and the degenerate shapes.  seeded() gives
[(name, [con1, con2, con1, con2, ...], recorded)]; the recorded ones stand in tests/cpp/offsets_cases.txt with what the oracle says of
them (python -m tests.offsets_cases writes it), the others are written out by tests/test_offsets_cpu.py when it runs."""
import os
import struct

import numpy as np

from tests import offsets_oracle

FILE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "cpp", "offsets_cases.txt")
THRESHOLDS = (19, 20, 24, 25, 39, 40)
STRETCHES = (30, 36, 44, 50)


def rnd(rng, n):
    return [int(b) for b in rng.randint(0, 4, n)]


def substituted(rng, seq, places):
    out = list(seq)
    for p in places: out[p] = (out[p] + int(rng.randint(1, 4))) % 4
    return out


def thresholds(rng):
    """a true overlap of exactly n bases behind and in front of 100 unrelated ones: offset 100"""
    seqs = []
    for n in THRESHOLDS:
        a = rnd(rng, n)
        seqs += [rnd(rng, 100) + a, a + rnd(rng, 100)]
    return seqs


def near_repeat(rng):
    r1 = rnd(rng, 150)
    s = r1 + substituted(rng, r1, (31, 77, 120))
    return [s, list(s)]


def tandem(rng):
    s = rnd(rng, 12) * 25
    return [s, list(s)]


def big_near_small(rng, L):
    """left(126) (AC)^(L/2) right(126); con2 the same with a substitution every 18 bases counted outward from both bases adjacent to the
    stretch: no agreeing run of offset 0 outside the stretch is longer than 17, so none validates a position there"""
    left, right = rnd(rng, 125) + [int(rng.randint(2, 4))], [int(rng.randint(2, 4))] + rnd(rng, 125)
    con1 = left + [0, 1] * (L // 2) + right
    con2 = list(con1)
    for p in list(range(125, -1, -18)) + list(range(126 + L, len(con1), 18)):
        con2[p] = 5 - con2[p] if con2[p] >= 2 else con2[p] + 2                     # (never to A or C beside the stretch)
    return [con1, con2]


def bad_window(rng):
    s = rnd(rng, 300)
    return [s, substituted(rng, s, sorted(rng.choice(np.arange(120, 160), 25, replace=False)))]


def all_mismatches(rng):
    a, b, x = rnd(rng, 50), rnd(rng, 50), rnd(rng, 20)
    return [a + x + b, a + substituted(rng, x, range(20)) + b]


def homopolymer(rng):
    r, s = rnd(rng, 100), rnd(rng, 100)
    r[-1], s[0] = 1, 2
    con = r + [0] * 40 + s
    return [con, list(con)]


def degenerate(rng):
    a, r8, r400 = rnd(rng, 50), rnd(rng, 8), rnd(rng, 400)
    x, y = rnd(rng, 60) + a, a + rnd(rng, 60)
    r200 = rnd(rng, 200)
    e = rnd(rng, 30)
    return [[], [], [], rnd(rng, 30), rnd(rng, 30), [],
            rnd(rng, 7), rnd(rng, 7), r8[:7], r8[:7],
            r8, list(r8),                                  # two identical 8-mers: a candidate with overlap 8 that fails
            r400, list(r400),                              # identical 400-mers
            x, y, y, x,                                    # a positive offset and its mirror, a negative one
            r200, r200[50:120], r200[50:120], r200,        # n1 != n2: one within the other, at +50 and at -50
            e + rnd(rng, 100), rnd(rng, 100) + e,          # the overlap is one end of each only: offset -100, 30 bases
            rnd(rng, 100) + e[:9], e[:9] + rnd(rng, 100),  # ... and nine bases: a candidate that fails
            a + e, a + e + rnd(rng, 20) + a + e]           # two true offsets, 0 and -100: two survivors


def many(rng):
    """4 200 pairs of short sequences: more than two tiles of the device's scan; a third overlap truly, by 20 to 35 bases"""
    seqs = []
    for p in range(4200):
        if p % 3 == 0:
            a = rnd(rng, int(rng.randint(20, 36)))
            seqs += [rnd(rng, int(rng.randint(0, 12))) + a, a + rnd(rng, int(rng.randint(0, 12)))]
        else:
            seqs += [rnd(rng, int(rng.randint(0, 40))), rnd(rng, int(rng.randint(0, 40)))]
    return seqs


def busy(rng):
    """one pair with dozens of passing offsets between pairs with none"""
    return [rnd(rng, 50), rnd(rng, 50)] + tandem(rng) + [rnd(rng, 50), rnd(rng, 50), [], rnd(rng, 20)]


def random_pairs(rng):
    """related sequences of every length up to 400 with substitutions, low-complexity stretches and shifts"""
    seqs = []
    for _ in range(60):
        base = rnd(rng, int(rng.randint(30, 401)))
        if rng.rand() < 0.5:
            at, unit = int(rng.randint(0, len(base) - 20)), rnd(rng, int(rng.randint(1, 5)))
            n = int(rng.randint(10, 60))
            base[at:at + n] = (unit * n)[:n]
            base = base[:400]
        other = substituted(rng, base, [p for p in range(len(base)) if rng.rand() < rng.choice([0.0, 0.02, 0.1, 0.4])])
        cut = int(rng.randint(0, len(base) // 2))
        seqs += ([base[cut:], other[:len(other) - cut // 2]] if rng.rand() < 0.5 else [base[:len(base) - cut], other[cut // 3:]])
    return seqs


SPECS = (("thresholds", 11, thresholds, True), ("near-repeat", 12, near_repeat, True), ("tandem", 13, tandem, False),
         *((f"big-near-small-{L}", 20 + L, (lambda L: lambda rng: big_near_small(rng, L))(L), L in (30, 44)) for L in STRETCHES),
         ("bad-window", 14, bad_window, True), ("all-mismatches", 15, all_mismatches, True), ("homopolymer", 16, homopolymer, False),
         ("degenerate", 17, degenerate, True), ("no-pairs", 18, lambda rng: [], True), ("many", 19, many, False), ("busy", 9, busy, False),
         ("random", 10, random_pairs, False))

_made = {}
_oracle = {}


def seeded():
    if not _made:
        for name, seed, make, rec in SPECS: _made[name] = (make(np.random.RandomState(seed)), rec)
    return [(name, seqs, rec) for name, (seqs, rec) in _made.items()]


def oracle(name, seqs):
    if name not in _oracle: _oracle[name] = offsets_oracle.run(seqs)
    return _oracle[name]


def case_text(name, seqs, r):
    """a case and what the oracle says of it, as tests/cpp/test_offsets.cc reads it: the doubles as their 8 bytes in hex"""
    out = ["case %s %d %d" % (name, len(seqs) // 2, len(r["records"]))]
    out += ["".join(str(int(b)) for b in s) or "-" for s in seqs]
    out += ["%d %d %d %d" % (*w, g["lookups"]) for w, g in zip(r["words"], r["per"])]
    out += ["%d %d %d %d %s %d" % (o, ov, fl, mm, struct.pack("<d", bits).hex(), st) for o, ov, fl, mm, bits, st in r["records"]]
    return out


def text(recorded=True):
    out = []
    for name, seqs, rec in seeded():
        if rec == recorded: out += case_text(name, seqs, oracle(name, seqs))
    return "\n".join(out) + "\n"


if __name__ == "__main__":
    open(FILE, "w").write(text())
