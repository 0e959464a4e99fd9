"""tests/subset_oracle.py (the subset of interest, 10X/runstages/RunStages.cc:208-254, restated) on a graph worked out by hand and on the
fixtures whose paths and graphs the reference's classes wrote.  CPU only."""
import os
import struct

import numpy as np
import pytest

from tests import subset_cases, subset_oracle
from tests.test_hops_oracle import HOT, SPECIAL, TABLE as HOPS_TABLE

# fixture, E, N, pairs (tests/hops_oracle.py, ONE_GOOD off), eoi, ids, path entries of the subset, of all reads, index entries, pairs taken
# through one read only, unplaced reads in the subset
TABLE = [("graph_pathy2_k48", 3184, 23400, 725, 804, 19094, 28889, 30995, 17318, 4097, 1580),
         ("graph_frag_k48", 1816, 6000, 937, 1028, 5878, 9315, 9418, 7640, 599, 314),
         ("graph_pathy_k48", 392, 3600, 63, 90, 3308, 5708, 6146, 2953, 720, 170),
         ("graph_k48", 262, 1800, 48, 42, 1142, 917, 1224, 721, 421, 234),
         ("graph_k40_nobc", 146, 1800, 138, 54, 1660, 1417, 1449, 1298, 369, 283),
         ("graph_k60_nobc", 312, 1800, 2, 4, 64, 47, 774, 35, 29, 18),
         ("graph_special_k48", 19, 700, 6, 14, 356, 522, 902, 454, 1, 0),
         ("graph_hot_k48_minfreq2", 56, 1500, 0, 0, 0, 0, 192, 0, 0, 0)]
FIXTURES = {h[0]: tuple(h[:3]) for h in list(HOPS_TABLE) + [SPECIAL, HOT]}      # case -> (case, K, reads from)

# ---- a graph worked out by hand
# Fourteen edges: e0 .. e11 in involution pairs (e ^ 1), e12 and e13 each its own involution.  Two edge pairs: (e0, e4) and (e12, e6).
#   in_pairs: e0, e4 and their involutions e1, e5; e12 (its own involution) and e6 with e7.        eoi = [0, 1, 4, 5, 6, 7, 12]
# Eight pairs of reads:
#   pair 0  r0 = [e0, e2]      hits (e0)     r1 = [e9]            does not      taken through its even read only
#   pair 1  r2 = [e8]          does not      r3 = [e3, e5]        hits (e5)     taken through its odd read only
#   pair 2  r4 = []            unplaced      r5 = [e4]            hits          taken: the unplaced r4 is in the subset
#   pair 3  r6 = []                          r7 = []                            two unplaced mates: not taken
#   pair 4  r8 = [e2, e8]      does not      r9 = [e10]           does not      placed, not taken
#   pair 5  r10 = [e6, e12, e6] hits         r11 = [e7]           hits          taken through both; r10 crosses e6 twice
#   pair 6  r12 = [e12, e12, e12] hits       r13 = [e13]          does not      taken; r12 crosses e12 three times (e13 is not marked)
#   pair 7  r14 = [e10, e11]   does not      r15 = [e3]           does not      not taken
#   read_ids = [0, 1, 2, 3, 4, 5, 10, 11, 12, 13]; four pairs through one read only (0, 1, 2, 6); one unplaced read (r4)
#   path entries of the subset: 2 + 1 + 1 + 2 + 0 + 1 + 3 + 1 + 3 + 1 = 15 of 21
#   index subset: e0: [0]; e1: []; e4: [5]; e5: [3]; e6: [10, 10]; e7: [11]; e12: [10, 12, 12, 12]: ten entries
HAND = dict(inv=[1, 0, 3, 2, 5, 4, 7, 6, 9, 8, 11, 10, 12, 13], pairs=[(0, 4), (12, 6)],
            paths=[[0, 2], [9], [8], [3, 5], [], [4], [], [], [2, 8], [10], [6, 12, 6], [7], [12, 12, 12], [13], [10, 11], [3]])
HAND_EOI = [0, 1, 4, 5, 6, 7, 12]
HAND_IDS = [0, 1, 2, 3, 4, 5, 10, 11, 12, 13]
HAND_LISTS = [[0], [], [5], [3], [10, 10], [11], [10, 12, 12, 12]]


def test_rule_on_a_graph_worked_out_by_hand():
    r = subset_oracle.run(HAND["paths"], HAND["inv"], HAND["pairs"])
    assert r["eoi"] == HAND_EOI and r["ids"] == HAND_IDS
    assert (r["path_entries"], r["all_entries"], r["index_entries"], r["one_read_only"], r["unplaced"], r["twice"]) == (15, 21, 10, 4, 1, 2)
    f = r["files"]
    assert f["a.sub.ids"] == b"BINWRITE" + struct.pack("<Q", 10) + np.asarray(HAND_IDS, "<u8").tobytes()
    assert f["a.sub.eoi"] == b"BINWRITE" + struct.pack("<Q", 7) + np.asarray(HAND_EOI, "<u8").tobytes()
    head, elems = subset_oracle.feudal_elements(f["a.sub.paths"])
    assert head == struct.pack("<IBBBBQQ", 10, 1, 0, 24, 4, 24 + 8 * 10 + 4 * 15, 24 + 8 * 10 + 4 * 15 + 8 * 11)
    assert elems == [struct.pack("<iI", 0, 0) + np.asarray(HAND["paths"][i], "<i4").tobytes() for i in HAND_IDS]
    head, elems = subset_oracle.feudal_elements(f["a.sub.paths.inv"])
    assert head == struct.pack("<IBBBBQQ", 7, 1, 0, 16, 8, 24 + 8 * 10, 24 + 8 * 10 + 8 * 8)
    assert elems == [np.asarray(l, "<u8").tobytes() for l in HAND_LISTS]
    assert r["index_first"] == [0, 1, 1, 2, 3, 5, 6, 10]
    # the pair given again, reversed, or named through its involution marks the same edges
    for pairs in ([(0, 4), (12, 6), (0, 4)], [(4, 0), (6, 12)], [(1, 5), (12, 7)]):
        assert subset_oracle.run(HAND["paths"], HAND["inv"], pairs)["files"] == f
    # no pairs: four valid files with n = 0
    e = subset_oracle.run(HAND["paths"], HAND["inv"], [])["files"]
    assert e["a.sub.ids"] == e["a.sub.eoi"] == b"BINWRITE" + bytes(8)
    assert e["a.sub.paths"] == struct.pack("<IBBBBQQQ", 0, 1, 0, 24, 4, 24, 32, 24) and e["a.sub.paths.inv"] == struct.pack("<IBBBBQQQ", 0, 1, 0, 16, 8, 24, 32, 24)


def test_slices_are_the_source_files_bytes_and_every_id_gives_the_source_back(golden_dir):
    for case, name in (("graph_frag_k48", "a.paths"), ("graph_frag_k48", "a.paths.inv")):
        b = open(os.path.join(golden_dir, case, name), "rb").read()
        n = int.from_bytes(b[:4], "little")
        assert subset_oracle.slice_feudal(b, range(n)) == b
        head, elems = subset_oracle.feudal_elements(b)
        assert subset_oracle.feudal_elements(subset_oracle.slice_feudal(b, [3, 5, n - 1]))[1] == [elems[3], elems[5], elems[n - 1]]


@pytest.mark.parametrize("row", TABLE, ids=[r[0] for r in TABLE])
def test_restatement_gives_the_counts_of_the_fixtures(golden_dir, row):
    case, E, N, n_pairs, n_eoi, n_ids, sub_entries, all_entries, index_entries, one, unplaced = row
    r = subset_oracle.fixture_subset(golden_dir, *FIXTURES[case])
    assert (len(r["pairs"]), len(r["eoi"]), len(r["ids"])) == (n_pairs, n_eoi, n_ids)
    assert (r["path_entries"], r["all_entries"], r["index_entries"], r["one_read_only"], r["unplaced"]) == (sub_entries, all_entries, index_entries, one, unplaced)
    assert int.from_bytes(open(os.path.join(golden_dir, case, "a.paths"), "rb").read()[:4], "little") == N
    assert r["reference_index"] == (case in ("graph_frag_k48", "graph_pathy2_k48"))
    # no fixture has a self-inverse edge of interest; only graph_k40_nobc has reads (4) that cross an edge of interest twice
    from tests.test_hops_oracle import fixture_inputs
    inv = fixture_inputs(golden_dir, *FIXTURES[case])["inv"]
    assert len(inv) == E and not [e for e in r["eoi"] if inv[e] == e]
    assert r["twice"] == (4 if case == "graph_k40_nobc" else 0)


def test_seeded_cases_supply_what_the_fixtures_lack():
    got = {name: (c, subset_oracle.run(c["paths"], c["inv"], c["pairs"])) for name, c, _ in subset_cases.seeded()}
    assert any(any(c["inv"][e] == e for e in r["eoi"]) for c, r in got.values())                 # a self-inverse edge of interest
    for name, (c, r) in got.items():
        if not c["planted"]: continue
        m = subset_oracle.mark_edges(c["pairs"], c["inv"])
        assert all(i in r["ids"] for i in (0, 1, 2, 3, 4, 5, 10, 11, 12, 13)) and not any(i in r["ids"] for i in (6, 7, 8, 9, 14, 15)), name
        assert max(c["paths"][10].count(e) for e in c["paths"][10] if m[e]) >= 2 and c["paths"][12].count(c["paths"][12][0]) == 3 and m[c["paths"][12][0]], name
        lists = subset_oracle.feudal_elements(r["files"]["a.sub.paths.inv"])[1]
        k = r["eoi"].index(c["paths"][12][0])
        assert list(np.frombuffer(lists[k], "<u8")).count(12) == 3, name                        # listed as often as it is crossed
    assert sum(1 for c, _ in got.values() if c["planted"]) >= 4
    assert got["no-pairs"][1]["ids"] == [] and got["no-pairs"][1]["eoi"] == []
    assert got["every-edge"][1]["eoi"] == list(range(12)) and len(got["no-reads"][1]["eoi"]) > 0 and got["no-reads"][1]["ids"] == []
    c = got["twice-and-reversed"][0]
    assert c["pairs"][-2] == c["pairs"][0] and c["pairs"][-1] == c["pairs"][0][::-1]
    assert len(got["three-scan-tiles"][0]["paths"]) > 2 * 256 * 8                                # device_scan's tile: SCAN_THREADS x SCAN_ITEMS (dfk_kernels.h)


def test_digest_is_positional():
    a, b = subset_oracle.seq_digest([2, 3, 10, 11], 0x7777), subset_oracle.seq_digest([2, 3], 0x7777)
    c = subset_oracle.seq_digest([10, 11], 0x7777 + 2)
    assert ((b[0] + c[0]) & (2**64 - 1), b[1] ^ c[1]) == a and subset_oracle.seq_digest([], 1) == (0, 0)
    assert subset_oracle.seq_digest([3, 2, 10, 11], 0x7777) != a
