"""tests/hops_oracle.py (FindEdgePairs, 10X/Closomatic.cc:17-358, restated) on a graph worked out by hand and on the fixtures whose
paths and graphs the reference's classes wrote.  CPU only."""
import os

import numpy as np
import pytest

from tests import bads_oracle, hops_oracle
from tests.test_bads_oracle import TABLE as BADS_TABLE, fixture_expected
from tests.test_paths_oracle import decode_paths, load_reads

# fixture, K, reads from, graph edges, reads, (method 1, 2, 3, union), the same with ONE_GOOD, edges reaching the search, extended,
# most rounds, largest X, largest exts, longest member of an X, longest sequence the search built
TABLE = [("graph_pathy2_k48", 48, "pathy2", 3184, 23400, (69, 62, 667, 725), (257, 0, 667, 767), 938, 497, 7, 60, 8, 15, 17),
         ("graph_frag_k48", 48, "frag", 1816, 6000, (322, 39, 680, 937), (594, 0, 680, 1077), 378, 79, 3, 18, 5, 4, 6),
         ("graph_pathy_k48", 48, "pathy", 392, 3600, (0, 4, 63, 63), (8, 0, 63, 65), 116, 97, 4, 71, 10, 12, 12),
         ("graph_k48", 48, "reads", 262, 1800, (48, 0, 48, 48), (48, 0, 48, 48), 88, 0, 2, 38, 3, 3, 3),
         ("graph_k40_nobc", 40, "reads", 146, 1800, (109, 2, 133, 138), (136, 0, 133, 138), 62, 5, 0, 39, 4, 3, 3),
         ("graph_k60_nobc", 60, "reads", 312, 1800, (2, 0, 2, 2), (2, 0, 2, 2), 62, 0, 0, 10, 1, 2, 1)]
# the zoo (tests/zoo_synth.py) in rows of its own: reads that go round a short cycle name one edge dozens of times, so the members of
# an X are longer and the searches wider than the device's default LDS capacities hold (tests/test_gpu_hops.py asserts of every row
# of TABLE that they do); tests/test_gpu_zoo.py runs these and says how many edges the host must decide
ZOO_TABLE = [("graph_zoo_k40", 40, "zoo", 1346, 20624, (0, 0, 344, 344), (1, 0, 344, 345), 466, 396, 3, 38, 55, 37, 39),
             ("graph_zoo_k48", 48, "zoo", 1334, 20624, (0, 0, 465, 465), (2, 0, 465, 467), 354, 258, 2, 28, 54, 30, 59),
             ("graph_zoo_k60", 60, "zoo", 1054, 20624, (0, 0, 349, 349), (0, 0, 349, 349), 382, 287, 2, 25, 33, 22, 43)]
SPECIAL = ("graph_special_k48", 48, "special")
HOT = ("graph_hot_k48_minfreq2", 48, "hot")               # gives no pairs: the empty case

_cache = {}


def seeded_bc(n):
    """the barcodes the tests give the `special` fixture (its own put every read under one): 1 + pair % 7"""
    return (1 + (np.arange(n) // 2) % 7).astype(np.int32)


def fixture_inputs(golden_dir, case, K, which):
    """dict(paths, kmers, inv, to_left, to_right, bc, bad) of a fixture: the files the reference's classes wrote, MarkBads' marks from
    tests/bads_oracle.py; computed once per session and handed out unchanged"""
    key = ("in", case)
    if key not in _cache:
        if case in {r[0] for r in BADS_TABLE}:
            paths, _, _, _, sums = fixture_expected(golden_dir, case, K, which)
        else:                                                    # (special, hot: no row in the table of tests/test_bads_oracle.py)
            from oracle import paths_oracle
            reads, quals = paths_oracle.unpack_reads(load_reads(golden_dir, which))
            paths = decode_paths(open(os.path.join(golden_dir, case, "a.paths"), "rb").read())
            sums = bads_oracle.bad_sums(paths, reads, quals, bads_oracle.fixture_edges(golden_dir, case), K)
        bc = seeded_bc(len(paths)) if case == SPECIAL[0] else np.asarray(load_reads(golden_dir, which)["bc"], np.int32)
        kmers, inv, to_left, to_right = hops_oracle.fixture_graph(golden_dir, case, K)
        _cache[key] = dict(paths=[p for _, p in paths], kmers=kmers, inv=inv, to_left=to_left, to_right=to_right, bc=bc, bad=bads_oracle.bad_marks(sums))
    return _cache[key]


def fixture_hops(golden_dir, case, K, which, one_good=False):
    """hops_oracle.run on a fixture; computed once per session and handed out unchanged"""
    key = (case, bool(one_good))
    if key not in _cache:
        i = fixture_inputs(golden_dir, case, K, which)
        _cache[key] = hops_oracle.run(i["paths"], i["kmers"], i["inv"], i["to_left"], i["to_right"], i["bc"], i["bad"], K, one_good)
    return _cache[key]


# ---- a graph worked out by hand
# K = 4, so MIN_CAND = 5.  Fourteen edges, each with its involution (e ^ 1); vertices are named by what they join.
#
#        e0 (50)       e2 (60)                    a chain a -> b -> c that ends in c            inv: e1 (b' -> a'), e3 (c' -> b')
#    a --------> b --------> c
#       e12 (130)      e4 (110)                   q -> s -> t: the one edge that enters s is 130 k-mers long, and no read lies on it
#    q --------> s --------> t                                                                  inv: e13 (s' -> q'), e5 (t' -> s')
#        e6 (45)       e8 (121)                   a chain u -> v -> x that ends in x, its last edge 121 k-mers long
#    u --------> v --------> x                                                                  inv: e7 (v' -> u'), e9 (x' -> v')
#        e10 (200)                                an island y -> z                              inv: e11 (z' -> y')
#    y --------> z
HAND = dict(
    K=4,
    kmers=[50, 50, 60, 60, 110, 110, 45, 45, 121, 121, 200, 200, 130, 130],
    inv=[1, 0, 3, 2, 5, 4, 7, 6, 9, 8, 11, 10, 13, 12],
    #        e0 e1 e2 e3 e4 e5 e6 e7 e8 e9 e10 e11 e12 e13  vertices: a0 b1 c2 | c'3 b'4 a'5 | s6 t7 | t'8 s'9 | u10 v11 x12 | x'13 v'14 u'15 | y16 z17 | z'18 y'19 | q20 q'21
    to_left=[0, 4, 1, 3, 6, 8, 10, 14, 11, 13, 16, 18, 20, 9],
    to_right=[1, 5, 2, 4, 7, 9, 11, 15, 12, 14, 17, 19, 6, 21],
    # pairs:   0: (r0, r1)   1: (r2, r3)   2: (r4, r5)   3: (r6, r7)   4: (r8, r9)   5: (r10, r11)   6: (r12, r13)   7: (r14, r15)
    paths=[[0, 2], [5],      # r0 on e0 e2, its mate on inv[e4]
           [0], [5],         # r2 on e0, its mate on inv[e4]
           [2], [],          # r4 on e2, mate unplaced
           [0, 2], [],       # r6 on e0 e2, mate unplaced
           [6], [11],        # r8 on e6, its mate on inv[e10]
           [6, 8], [11],     # r10 on e6 e8, its mate on inv[e10]
           [10, 10], [7],    # r12 crosses e10 twice (a loop is not in the graph: the rule does not ask), its mate on inv[e6]
           [10], [9, 7]],    # r14 on e10, its mate on inv[e8] inv[e6]
    bc=[1, 1, 2, 2, 3, 3, 0, 0, 4, 4, 0, 0, 5, 5, 6, 6],
    bad=[0, 0, 0, 0, 0, 0, 0, 0])
# Sink test: e0 passes (after it only e2, which ends in c: nothing leaves c, one edge enters it, 60 <= 120).  e6 FAILS, and only
#   through the k-mers clause: after it only e8, which ends in x (nothing leaves, one enters), but kmers(e8) = 121 > 120.
#   e2, e4, e8, e10 and every involuted edge but e3, e9 (after e3 comes e1: a' has nothing behind it: passes; e9 -> e7: passes)
#   have nothing after them or pass likewise (e5 does not: e13 behind it is 130 k-mers long; it has nothing supported anyway); what
#   matters is which of them have mates to show.
# Mate sets (e2 = inv[last edge of the mate's path], id = barcode, 0 = the one id all unbarcoded reads share):
#   e0: r0 -> (e4, 1), r2 -> (e4, 2), r6 -> mate unplaced          e4 supported
#   e2: r0 -> (e4, 1), r4, r6 unplaced mates                       nothing supported
#   e5: r1 -> mate r0 ends on e2: (inv[e2] = e3, 1), r3 -> mate r2 ends on e0: (e1, 2)            nothing supported
#   e6: r8 -> (e10, 4), r10 -> (e10, 0)                            e10 supported by exactly two ids, one of them the shared one
#   e11: r9 -> (inv[e6] = e7, 4), r11 -> mate r10 ends on e8: (e9, 0)                             nothing supported
#   e10: r12 (listed once though it crosses twice) -> (inv[e7] = e6, 5), r14 -> mate ends on e7: (e6, 6)      e6 supported
#   e7: r13 -> mate r12 ends on e10: (e11, 5), r15 -> (e11, 6)     e11 supported
#   e9: r15 -> (e11, 6)                                            nothing supported
# Method 1: (e0, e4) is NOT emitted: e0 passes the sink test, but e4 fails the source test -- e12 enters s, nothing enters q and one
#           edge leaves it, but kmers(e12) = 130 > 120.  (Without e12 and e13 nothing enters s and method 1 takes (e0, e4): see the test.)
#           (e10, e6): nothing follows e10; e6: nothing enters u.
#           (e7, e11): nothing follows e7 (u' is an end); e11: nothing enters z'.
#           e6 is not an e1: it fails the sink test, so (e6, e10) is NOT emitted although e10 is supported.
# Method 2: e0 passes the sink test and method 1 gave it nothing: (e0, e4), as kmers(e4) = 110 >= 100 and ToRight(e0) = b != s.  Every
#           other e1 that passes and has a supported e2 was served by method 1.
# Method 3 (every edge has kmers >= 5; e12 and e13 carry no read and do not reach the search):
#   e0: reads on e0: r0, r2, r6 (ids 1, 2, 0); none on e1.  X = {[e0, e2], [e0], [e4]}.  exts = {[e0, e2] (60 behind e0), [e0] (0)}.
#       Round 1: [e0] + [e0, e2] at l = 0 -> [e0, e2]; from [e0, e2] nothing (e2 is nowhere followed).  exts = {[e0, e2]}: one round,
#       then nothing: not extended.  too_easy = {e2}; can = {(e4, 1), (e4, 2)}: (e0, e4).
#   e2: reads r0, r4, r6; X = {[e2], [e4]}: not extended; can = {(e4, 1)}: nothing.
#   e3 (reads on inv = e2: r0 at j = 1 -> [e3, e1]; r4 -> [e3]; r6 -> [e3, e1]): [e3, e1] has 50 behind e3; one round; not extended;
#       can = {(e1, 1), (e1, 0)}: (e3, e1).  e1 (reads on e0): X = {[e1]}; can holds only e1 itself, excluded: nothing.
#   e4 (reads on e5: r1, r3): X = {[e4]}: nothing to see.   e5 (r1, r3 on it): X = {[e5], [e3, e1], [e1]}; can = {(e3, 1), (e1, 1), (e1, 2)}: (e5, e1).
#   e6: reads r8, r10 (ids 4, 0).  X = {[e6], [e6, e8], [e10]}.  [e6, e8] has 121 >= 100 behind e6: EXTENDED at once, no round.
#   e8: r10 on it (id 0), r15 on inv[e8] = e9 (id 6): X = {[e8], [e10]}: not extended; can = {(e10, 0)}: one id: nothing.
#   e9: r15 on it, r10 on e8: X = {[e9, e7], [e11]}: 45 behind e9: not extended; too_easy = {e7}; can = {(e11, 6), (e7, 0)}: nothing.
#   e7 (r13, r15 on it; reads on inv = e6: r8, r10): X = {[e7] (r13, r8), [e7, ...]: r15 = [e9, e7] holds e7 at j = 1 -> suffix [e7];
#       mates: r12 -> inv-reversed [e11, e11]; r14 -> [e11]; from e6's reads: r10 = [e6, e8] holds e6 at j = 0 -> [e7]}.
#       X = {[e7], [e11, e11], [e11]}; exts = {[e7]}; nothing follows e7 in X: not extended, no round.
#       too_easy = {}; can: r13 (5) -> e11; r15 (6) -> e11; r8, r10 give only e7 itself: {(e11, 5), (e11, 6)}: (e7, e11).
#   e10 (r12, r14 on it; reads on e11: r9, r11): X = {[e10, e10], [e10] (r12 at j = 1, r14), [e6] (r13 reversed), [e6, e8] (r15),
#       [e10] again from r9 and r11}.  exts = {[e10, e10] (200 behind): EXTENDED.
#   e11 (r9, r11 on it; on e10: r12, r14): X = {[e11], [e7] (r8 reversed), [e9, e7] (r10 reversed), [e11] (r14), [e11, e11] and [e11]
#       (r12 at j = 1 and j = 0)}; exts = {[e11], [e11, e11] (200 behind)}: EXTENDED.
HAND_M1 = [(7, 11), (10, 6)]
HAND_M2 = [(0, 4)]
HAND_M3 = [(0, 4), (3, 1), (5, 1), (7, 11)]


def run_hand(**change):
    h = dict(HAND); h.update(change)
    return hops_oracle.run(h["paths"], h["kmers"], h["inv"], h["to_left"], h["to_right"], h["bc"], h["bad"], h["K"], h.get("one_good", False))


def test_rule_on_a_graph_worked_out_by_hand():
    r = run_hand()
    assert r["m1"] == HAND_M1 and r["m2"] == HAND_M2 and r["m3"] == HAND_M3
    assert r["pairs"] == sorted(set(HAND_M1) | set(HAND_M2) | set(HAND_M3))
    # e6 fails the sink test through the k-mers clause alone: with 120 k-mers on e8 it passes and (e6, e10) -- supported by exactly
    # two ids, one of them the id all unbarcoded reads share -- appears; and [e6, e8] still extends e6 (120 >= 100)
    km = list(HAND["kmers"]); km[8] = km[9] = 120
    assert set(run_hand(kmers=km)["m1"]) - set(HAND_M1) == {(6, 10)}
    # ... and with the unbarcoded r10 given r8's barcode, e10 has one id only
    bc = list(HAND["bc"]); bc[10] = bc[11] = 4
    assert (6, 10) not in run_hand(kmers=km, bc=bc)["pairs"]
    # a read that crosses e twice: r12 = [e10, e10] gives X two members, and counts once among the ids of e10
    assert r["x_sizes"][10][0] == 4                              # {[e10, e10], [e10], [e6] (the mate r13 = [e7]), [e6, e8] (the mate r15 = [e9, e7])}
    assert r["searched"] == 12 and r["extended"] == 3            # every edge has two ids on it and its involution; e6, e10, e11 are extended
    # method 2 lives on e4's failed source test, which fails through the k-mers clause of e12 alone: with 120 k-mers on e12, or without
    # e12 and e13, method 1 takes (e0, e4) and method 2 is left with nothing
    km12 = list(HAND["kmers"]); km12[12] = km12[13] = 120
    plain = {k: HAND[k][:12] for k in ("kmers", "inv", "to_left", "to_right")}
    for r2 in (run_hand(kmers=km12), run_hand(**plain)):
        assert r2["m1"] == [(0, 4)] + HAND_M1 and r2["m2"] == [] and r2["m3"] == HAND_M3
    assert run_hand(one_good=True)["m1"] == [(0, 4)] + HAND_M1   # ONE_GOOD: method 1 does not ask, method 2 is left with nothing
    assert run_hand(one_good=True)["m2"] == []
    # a candidate that exists only through a bad pair: pair 1 (r2, r3) bad -> (e4, 2) leaves e0's can, (e1, 2) leaves e5's
    bad = list(HAND["bad"]); bad[1] = 1
    r3 = run_hand(bad=bad)
    assert r3["m1"] == HAND_M1 and r3["m3"] == [(3, 1), (7, 11)]
    # a candidate removed by too_easy: a read r16 = [e0, e2] whose mate r17 lies on inv[e2] = e3 ... reversed and involuted that is
    # [e2]: can of e0 gains (e2, 7) and, from a second such pair, (e2, 8): two ids -- but e2 is directly behind e0 in the reads
    paths = HAND["paths"] + [[0, 2], [3], [0, 2], [3]]
    r4 = run_hand(paths=paths, bc=HAND["bc"] + [7, 7, 8, 8], bad=HAND["bad"] + [0, 0])
    assert (0, 2) not in r4["m3"] and (0, 4) in r4["m3"]
    # ... while e5, whose reads' mates r0 = [e0, e2] show it (e3, 1) only once, still has nothing for e3
    assert [p for p in r4["m3"] if p[0] == 5] == [(5, 1)]


# ---- a second graph worked out by hand, for the search (tests/cpp/test_hops.cc runs the same three on dfk_hops.h)
# K = 4.  A chain E0 .. E4 of forward edges e0, e2, e4, e6, e8 (E_i joins vertex i to i + 1; its involution is the odd neighbour, on a
# chain of its own, 10 - i -> 11 - i); kmers(E0) = 10, the others 40, so 100 k-mers behind E0 take three edges.  Two pairs, barcodes 1
# and 2, both with their first read on [E0, E1]; the mates decide what else X of E0 holds (a mate's path joins X reversed and involuted):
#   two rounds: mates [e5, e3] and [e7, e5]: X = {[E0, E1], [E1, E2], [E2, E3]}.  exts = {[E0, E1]} (40).  Round 1: [E1, E2] holds E1 at
#       l = 0: [E0, E1, E2] (80).  Round 2: [E2, E3] at l = 0: [E0, E1, E2, E3] (120): extended.
#   a mismatch before l: the first mate is [e5, e3, e9]: X = {[E0, E1], [E4, E1, E2], [E2, E3]}.  y = [E4, E1, E2] holds E1 at l = 1, but
#       laid on x = [E0, E1] its E4 (m = 0 < l) falls on E0: not laid on.  exts2 is empty at once: not extended, no round.
#       too_easy = {E1}; can = {(E4, 1), (E1, 1), (E2, 1), (E2, 2), (E3, 2)}: E2 has two ids and is not too easy: (E0, E2) = (e0, e4).
#   ... and with E0 in E4's place (mate [e5, e3, e1]) y = [E0, E1, E2] is in exts from the start (80); one round adds [E2, E3]: extended.
SEARCH = dict(K=4, kmers=[10, 10, 40, 40, 40, 40, 40, 40, 40, 40], inv=[1, 0, 3, 2, 5, 4, 7, 6, 9, 8],
              to_left=[0, 10, 1, 9, 2, 8, 3, 7, 4, 6], to_right=[1, 11, 2, 10, 3, 9, 4, 8, 5, 7], bc=[1, 1, 2, 2], bad=[0, 0])


@pytest.mark.parametrize("mate, X, extended, rounds, from_e0", [
    ([5, 3], [(0, 2), (2, 4), (4, 6)], True, 2, []),
    ([5, 3, 9], [(0, 2), (4, 6), (8, 2, 4)], False, 0, [(0, 4)]),
    ([5, 3, 1], [(0, 2), (0, 2, 4), (4, 6)], True, 1, [])], ids=["two-rounds", "mismatch-before-l", "agrees-before-l"])
def test_searches_of_a_graph_worked_out_by_hand(mate, X, extended, rounds, from_e0):
    g = SEARCH
    paths = [[0, 2], mate, [0, 2], [7, 5]]
    idx = hops_oracle.paths_index(paths, len(g["kmers"]))
    assert hops_oracle.build_x(0, idx, paths, g["inv"]) == X
    assert hops_oracle.search(0, X, g["kmers"])[:2] == (extended, rounds)
    r = hops_oracle.run(paths, g["kmers"], g["inv"], g["to_left"], g["to_right"], g["bc"], g["bad"], g["K"])
    assert [p for p in r["m3"] if p[0] == 0] == from_e0 and 0 in r["x_sizes"] and r["most_rounds"] >= rounds


def test_search_rounds_and_an_overlap_mismatch_before_l():
    """the search alone, on sets X written down: two rounds to reach 100 k-mers; a candidate whose overlap disagrees at a position
    before l is not laid on"""
    kmers = [10, 40, 40, 40, 40, 40, 40]
    # [e0, e1] -> + [e1, e2] -> + [e2, e3]: 40, 80, 120 k-mers behind e0: extended after two rounds
    X = sorted({(0, 1), (1, 2), (2, 3)})
    assert hops_oracle.search(0, X, kmers)[:2] == (True, 2)
    # y = [e4, e1, e2] holds e1 at l = 1, but its e4 in front of it would lie on x's e0: mismatch at m = 0 < l: [e0, e1] dies
    X = sorted({(0, 1), (4, 1, 2), (2, 3)})
    assert hops_oracle.search(0, X, kmers)[:2] == (False, 0)
    # ... and with e0 in that place it is laid on
    X = sorted({(0, 1), (0, 1, 2), (2, 3)})
    assert hops_oracle.search(0, X, kmers)[:2] == (True, 1)      # [e0, e1, e2] is a member already (80), + [e2, e3] -> 120


@pytest.mark.parametrize("row", TABLE + ZOO_TABLE, ids=[r[0] for r in TABLE + ZOO_TABLE])
def test_restatement_gives_the_counts_of_the_fixtures(golden_dir, row):
    case, K, which, E, N, plain, one_good, searched, extended, rounds, largest_x, largest_exts, longest, longest_ext = row
    i = fixture_inputs(golden_dir, case, K, which)
    assert (len(i["kmers"]), len(i["paths"])) == (E, N)
    for og, want in ((False, plain), (True, one_good)):
        r = fixture_hops(golden_dir, case, K, which, og)
        assert (len(r["m1"]), len(r["m2"]), len(r["m3"]), len(r["pairs"])) == want
        assert (r["searched"], r["extended"], r["most_rounds"], r["largest_x"], r["largest_exts"], r["longest"], r["longest_ext"]) == \
               (searched, extended, rounds, largest_x, largest_exts, longest, longest_ext)
        assert r["pairs"] == sorted(set(r["pairs"])) and set(r["pairs"]) == set(r["m1"]) | set(r["m2"]) | set(r["m3"])


def test_marks_double_crossings_and_unbarcoded_reads_are_in_play_on_pathy2(golden_dir):
    case, K, which = TABLE[0][:3]
    i = fixture_inputs(golden_dir, case, K, which)
    r = fixture_hops(golden_dir, case, K, which)
    blind = hops_oracle.run(i["paths"], i["kmers"], i["inv"], i["to_left"], i["to_right"], i["bc"], np.zeros_like(i["bad"]), K)
    assert len(set(blind["pairs"]) ^ set(r["pairs"])) == 179 and blind["m1"] == r["m1"] and blind["m2"] == r["m2"]   # the marks: method 3 alone
    assert sum(1 for p in i["paths"] if len(set(p)) < len(p)) == 160 and int((i["bc"] == 0).sum()) == 2340


def test_self_inverse_edge_of_the_special_fixture(golden_dir):
    case, K, which = SPECIAL
    i = fixture_inputs(golden_dir, case, K, which)
    selfinv = [e for e in range(len(i["inv"])) if i["inv"][e] == e]
    assert selfinv == [4] and sum(1 for p in i["paths"] if 4 in p) == 22
    own = np.asarray(load_reads(golden_dir, which)["bc"])
    assert len(set(own.tolist())) == 1                           # the fixture's own barcodes: one for all, so no edge has two ids on it
    assert hops_oracle.run(i["paths"], i["kmers"], i["inv"], i["to_left"], i["to_right"], own, i["bad"], K)["pairs"] == []
    r = fixture_hops(golden_dir, case, K, which)
    # with the seeded barcodes the rule has something to say; the self-inverse edge itself is one k-mer long and starts no search,
    # but its reads are listed under it both ways (as reads on e and as reads on inv[e]) and it is an e1 of methods 1 and 2
    assert (len(r["m1"]), len(r["m2"]), len(r["m3"]), len(r["pairs"])) == (2, 0, 6, 6) and i["kmers"][4] == 1 and 4 not in r["x_sizes"]


def test_hot_fixture_is_the_empty_case(golden_dir):
    r = fixture_hops(golden_dir, *HOT)
    assert r["pairs"] == [] and r["file"] == b"BINWRITE" + bytes(8) and r["digest"] == (0, 0)


def test_file_bytes_and_digest():
    pairs = [(0, 4), (3, 1), (7, 11)]
    f = hops_oracle.hops_file(pairs)
    assert f == b"BINWRITE" + (3).to_bytes(8, "little") + b"".join(int(x).to_bytes(4, "little", signed=True) for p in pairs for x in p)
    assert hops_oracle.hops_file([]) == b"BINWRITE" + bytes(8) and len(hops_oracle.hops_file([])) == 16
    a, b, whole = hops_oracle.hops_digest(pairs[:1]), hops_oracle.hops_digest(pairs[1:]), hops_oracle.hops_digest(pairs)
    assert ((a[0] + b[0]) & (2**64 - 1), a[1] ^ b[1]) == whole                   # disjoint sets: sums add, xors xor
    assert hops_oracle.hops_digest(pairs[::-1]) == whole and hops_oracle.hops_digest([(4, 0)]) != hops_oracle.hops_digest([(0, 4)])
    assert hops_oracle.hops_digest([]) == (0, 0)
