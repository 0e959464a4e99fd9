"""tests/translate_cases.py -- TEST INFRASTRUCTURE: hand-made and seeded tables (to3, left3, hb3's K-mer counts) with read paths for the
translation onto the patched graph (tests/translate_oracle.py, superplus_amd/csrc/dfk_translate.h), and tests/cpp/translate_cases.txt
recorded from them (python -m tests.translate_cases).  K = 48: Bases = Kmers + 47.

hb3's edges, by id: A = 0 (20 K-mers, 67 bases), B = 1 (30, 77), C = 2 (5, 52), D = 3 (5, 52), E = 4 (7, 54), F = 5 (9, 56), S = 6 and
S2 = 7 (one K-mer, 48 bases), R = 8 (10, 57: the circle), 9 .. 48 forty edges of 3 K-mers (50 bases).  The plants, by case (fires() asserts
FROM THE ORACLE'S RESULT what each is there for):
  empty_before  paths empty before, with offsets 0, 5, -3: left alone
  no_to3        to3[path[0]] empty: cleared, the OLD offset (7, -4, 0) kept -- a cleared path whose old offset is nonzero and negative
  negative      start < 0 with left3 = 0 and with left3 = 3: the first hb3 edge takes it, the new offset negative
  bases_kmers   start at Kmers - 1, Kmers, Bases - 1 and Bases of the first hb3 edge, with left3 = 0 and left3 = 4: the first three stay on
                it (the test is against Bases), the fourth goes on with start - KMERS
  walks         walks ending on the 2nd of 2, the 2nd and 3rd of 3, the 2nd, 3rd and 40th of 40 ids
  circle        a circle's [R, R] with left3 = 5: on the first R, on the second, and off its end (path [c] and path [c, c]: OverlapAppend
                of [R, R] to [R, R] adds nothing)
  one_kmer      one-K-mer hb3 edges inside a walk: passed over, and landed on
  ranoff_neg    left3 = 200, offset -5: cleared by running off, the offset -5 kept
  overlaps      starts beyond to3[path[0]] (the host route) with OverlapAppend overlaps of 0, 1, a whole list (off the end, and with a third
                edge behind it) and the repeated motif A B C D C D + C D C D E F (overlap 4, not 2)
  break         a later edge with an empty to3 stops the appending: the same start lands with [a, b] and runs off with [a, z, b]
  random        700 reads over random tables: every kind, several batches
  pather        600 reads whose to3[e0] spells an old edge of kmers(e0) K-mers from left3[e0] and whose offset is below kmers(e0), as the pather
                makes them: no read leaves to3[e0]"""
import os

import numpy as np

from tests import translate_oracle as to

K = 48
FILE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "cpp", "translate_cases.txt")
A, B, C, D, E, F, S, S2, R = range(9)
KMERS3 = [20, 30, 5, 5, 7, 9, 1, 1, 10] + [3] * 40
FORTY = list(range(9, 49))


def case(to3, left3, paths, kmers3=KMERS3):
    return dict(K=K, to3=[list(x) for x in to3], left3=list(left3), kmers3=list(kmers3), paths=[(int(o), [int(e) for e in p]) for o, p in paths])


def hand_made():
    c = {}
    c["empty_before"] = case([[A]], [0], [(0, []), (5, []), (-3, [])])
    c["no_to3"] = case([[A], []], [0, 9], [(7, [1]), (-4, [1, 0]), (0, [1]), (3, [0])])
    c["negative"] = case([[A], [B]], [0, 3], [(-5, [0]), (-10, [1]), (-3, [1])])
    c["bases_kmers"] = case([[A, B], [A, B]], [0, 4], [(s - l, [e]) for e, l in ((0, 0), (1, 4)) for s in (19, 20, 66, 67)])
    c["walks"] = case([[A, B], [A, B, C], [FORTY[0]] + FORTY[1:]], [0, 0, 0],
                      [(67, [0]), (67, [1]), (100, [1]), (50, [2]), (53, [2]), (50 + 3 * 38, [2])])
    c["circle"] = case([[R, R]], [5], [(10, [0]), (55, [0]), (70, [0]), (55, [0, 0]), (70, [0, 0])])
    c["one_kmer"] = case([[A, S, S2, B]], [0], [(70, [0]), (68, [0]), (67, [0])])
    c["ranoff_neg"] = case([[A]], [200], [(-5, [0])])
    c["overlaps"] = case([[A], [B], [A, B], [B, C], [C], [A, B, C, D, C, D], [C, D, C, D, E, F]], [0] * 7,
                         [(70, [0, 1]), (100, [2, 3]), (100, [2, 2]), (100, [2, 2, 4]), (120, [5, 6]), (130, [5, 6]), (400, [5, 6])])
    c["break"] = case([[A], [B], []], [0, 0, 0], [(70, [0, 1]), (70, [0, 2, 1])])
    return c


def random_case(seed=11, n=700):
    g = np.random.default_rng(seed)
    E, E3 = 23, 17
    kmers3 = [int(x) for x in g.integers(1, 60, E3)]
    to3 = [[int(x) for x in g.integers(0, E3, int(g.integers(0, 5)))] for _ in range(E)]
    left3 = [int(x) for x in g.integers(0, 30, E)]
    paths = [(int(g.integers(-50, 200)), [int(x) for x in g.integers(0, E, int(g.integers(0, 5)))]) for _ in range(n)]
    return case(to3, left3, paths, kmers3)


def pather_case(seed=12, n=600):
    """(case, the old edges' K-mer counts)"""
    g = np.random.default_rng(seed)
    E, E3 = 19, 31
    kmers3 = [int(x) for x in g.integers(1, 40, E3)]
    to3, left3, kmers = [], [], []
    for _ in range(E):
        ids = [int(x) for x in g.integers(0, E3, int(g.integers(1, 6)))]
        l = int(g.integers(0, kmers3[ids[0]]))
        # the old edge begins on the first id at left3 and ends somewhere on the last: its K-mers
        total = sum(kmers3[i] for i in ids)
        lo = total - kmers3[ids[-1]] + 1 if len(ids) > 1 else l + 1
        to3.append(ids); left3.append(l); kmers.append(int(g.integers(max(lo, l + 1), total + 1)) - l)
    paths = []
    for _ in range(n):
        p = [int(x) for x in g.integers(0, E, int(g.integers(0, 4)))]
        paths.append((int(g.integers(-60, kmers[p[0]])) if p else 0, p))
    return case(to3, left3, paths, kmers3), kmers


def all_cases():
    c = hand_made()
    c["random"] = random_case()
    c["pather"] = pather_case()[0]
    return c


def run(c):
    return to.run(c["paths"], c["to3"], c["left3"], c["kmers3"], c["K"])


def fires(name, c, r):
    """what the case is there for, asserted from the oracle's result `r`"""
    kinds, new, old, n = r["kinds"], r["paths"], c["paths"], r["counters"]
    if name == "empty_before":
        assert set(kinds) == {"empty_before"} and new == old and [o for o, _ in old] == [0, 5, -3]
    elif name == "no_to3":
        assert kinds == ["cleared_empty"] * 3 + ["step2"] and new[:3] == [(7, []), (-4, []), (0, [])] and n["cleared_empty"] == 3
    elif name == "negative":
        assert kinds == ["step2"] * 3 and new == [(-5, [A]), (-7, [B]), (0, [B])] and c["left3"] == [0, 3]
    elif name == "bases_kmers":
        assert kinds == ["step2", "step2", "step2", "walk"] * 2
        assert new == [(19, [A]), (20, [A]), (66, [A]), (47, [B])] * 2 and not any(r["left"])            # Kmers(A) = 20, Bases(A) = 67: 67 - 20 = 47
        assert [o for o, _ in old[4:]] == [15, 16, 62, 63]
    elif name == "walks":
        assert kinds == ["walk"] * 6 and not any(r["left"])
        assert [e for _, e in new] == [[B], [B], [C], [FORTY[1]], [FORTY[2]], [FORTY[39]]] and len(c["to3"][2]) == 40
    elif name == "circle":
        assert kinds == ["step2", "walk", "cleared_ranoff", "walk", "cleared_ranoff"] and new == [(15, [R]), (50, [R]), (70, []), (50, [R]), (70, [])]
        assert r["overlaps"][3] == [0, 2] and r["left"] == [False, False, True, False, True]
    elif name == "one_kmer":
        assert kinds == ["walk"] * 3 and new == [(48, [B]), (47, [S2]), (47, [S])]
    elif name == "ranoff_neg":
        assert kinds == ["cleared_ranoff"] and new == [(-5, [])] and r["left"] == [True]
    elif name == "overlaps":
        assert [o for o in r["overlaps"]] == [[0, 0], [0, 1], [0, 2], [0, 2, 0], [0, 4], [0, 4], [0, 4]]
        assert kinds == ["walk", "walk", "cleared_ranoff", "walk", "walk", "walk", "cleared_ranoff"] and all(r["left"])
        assert new == [(50, [B]), (50, [C]), (100, []), (50, [C]), (50, [E]), (53, [F]), (400, [])]
    elif name == "break":
        assert kinds == ["walk", "cleared_ranoff"] and new == [(50, [B]), (70, [])] and r["overlaps"] == [[0, 0], [0]]
    elif name == "random":
        assert all(n[k] >= 10 for k in ("step2", "walk", "cleared_empty", "cleared_ranoff", "host")) and n["reads"] - n["placed_before"] >= 10 and n["reads"] == 700
        assert n["walk"] > sum(1 for k, l in zip(kinds, r["left"]) if k == "walk" and l) >= 10             # walks the device decides, and walks the host does
    elif name == "pather":
        assert n["host"] == 0 and n["cleared_ranoff"] == 0 and n["cleared_empty"] == 0 and n["walk"] >= 10 and n["step2"] >= 100 and n["reads"] == 600
    else:
        raise AssertionError(name)
    assert n["invalid"] == 0


def text():
    """tests/cpp/translate_cases.txt: per case the tables, then a line a read: the path | the oracle's outcome, kind, whether the walk left to3[e0]"""
    out = []
    for name, c in all_cases().items():
        r = run(c)
        first = np.concatenate([[0], np.cumsum([len(x) for x in c["to3"]])])
        row = lambda tag, v: out.append(" ".join([tag] + [str(int(x)) for x in v]))
        out.append(f"case {name} {c['K']} {len(c['left3'])} {len(c['kmers3'])} {len(c['paths'])}")
        row("F", first); row("T", [x for l in c["to3"] for x in l]); row("L", c["left3"]); row("M", c["kmers3"])
        for (o, p), (no, ne), k, l in zip(c["paths"], r["paths"], r["kinds"], r["left"]):
            row("R", [o, len(p), *p, no, ne[0] if ne else -1, to.KINDS.index(k), int(l)])
        out.append(f"digest {r['digest'][0]} {r['digest'][1]}")
    return "\n".join(out) + "\n"


# ---- wave and workgroup edges: n reads over two old edges, `placed(i)` and `flagged(i)` saying what read i is to be
def pattern_case(n, placed, flagged=lambda i: False):
    """old edge 0 -> [A]: placed by the first edge; old edge 1 -> nothing: cleared; a flagged read is (90, [2, 3]) with to3[2] = [A] and
    to3[3] = [B]: start 90 runs off [A] on the device, and the host, with [A, B], places it on B at 70"""
    paths = [((90, [2, 3]) if flagged(i) else (i % 19 - 3, [0]) if placed(i) else (i % 7 - 2, [1])) for i in range(n)]
    return case([[A], [], [A], [B]], [0, 0, 0, 0], paths)


if __name__ == "__main__":
    open(FILE, "w").write(text())
    print(FILE, os.path.getsize(FILE), "bytes")
