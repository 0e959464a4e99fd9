"""tests/closer_oracle.py (the closers' front end, 10X/Closomatic.cc:503-552 and 10X/Stackster.cc:289-324, restated per edge) on a graph
worked out by hand, on the fixtures whose paths, index, marks and graphs the reference's classes wrote, and on the seeded cases that
supply what the fixtures lack.  CPU only."""
import struct

import numpy as np
import pytest

from tests import closer_cases, closer_oracle
from tests.test_hops_oracle import HOT, SPECIAL, TABLE as HOPS_TABLE

# fixture, closer edges, locs, prec tuples, anchors, groups of exactly 4, of exactly 5, set entries, list entries skipped as duplicates,
# mates within MAX_DIST, of which unplaced, longest element of locs, mates kept out by MAX_DIST, (read, closer edge) crossings of 2 or more
TABLE = [("graph_pathy2_k48", 553, 27285, 8529, 731, 108, 83, 41002, 17, 13927, 1432, 133, 0, 0),
         ("graph_frag_k48", 734, 12160, 4575, 451, 129, 92, 16395, 1421, 5666, 330, 49, 0, 0),
         ("graph_pathy_k48", 59, 4347, 1704, 136, 7, 16, 6519, 4, 2199, 149, 157, 0, 0),
         ("graph_k48", 29, 1152, 4, 0, 0, 0, 1732, 0, 593, 189, 117, 0, 0),
         ("graph_k40_nobc", 43, 2386, 59, 6, 0, 1, 3499, 0, 1173, 248, 166, 35, 8),
         ("graph_k60_nobc", 2, 35, 0, 0, 0, 0, 52, 0, 17, 8, 23, 0, 0),
         ("graph_special_k48", 8, 558, 80, 4, 0, 0, 548, 14, 267, 0, 104, 0, 0),
         ("graph_hot_k48_minfreq2", 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0)]
FIXTURES = {h[0]: tuple(h[:3]) for h in list(HOPS_TABLE) + [SPECIAL, HOT]}      # case -> (case, K, reads from)

# ---- a graph worked out by hand.  K = 4.
# Six edges: e0/e1 and e2/e3 are involution pairs, e4 and e5 each its own involution.  kmers = 10, 10, 20, 20, 7, 3.
# Pairs (e0, e3) and (e4, e1): closer edges {e0, inv[e3] = e2} and {e4, inv[e1] = e0}: ce = [0, 2, 4].
#   r0 = [e0, e2] at 5    r1 = []             r2 = [e3, e1] at 2    r3 = [e0] at -3
#   r4 = [e4, e0, e4] at 1    r5 = [e5] at 0  r6 = [e2] at 0        r7 = [e2] at 0, and the pair (r6, r7) is marked a duplicate
# index: e0: [0, 3, 4]   e1: [2]   e2: [0, 6, 7]   e3: [2]   e4: [4, 4]   e5: [5]
# e0  pass 1 (f = e0): r0, j = 0: prec (e2, 10), pos 5;  r3: pos -3;  r4, j = 1: prec (e4, 10), pos 1 - 7 = -6
#     pass 2 (f = e1): r2, j = 1: prec (inv[e3] = e2, 10), pos 2 - 20 = -18
#     reads: (0, T) (3, T) (4, T) from list(e0), (2, F) from list(e1), the mates (1, F) (2, F) (5, F)
# e2  pass 1 (f = e2): r0, j = 1: no edge behind it, pos 5 - 10 = -5;  r6, r7 at 0 (locs has no duplicate filter)
#     pass 2 (f = e3): r2, j = 0: no edge in front, pos 2
#     reads: (0, T), r6 and r7 skipped, (2, F), the mate (1, F)
# e4  its own involution: f = e4 in both passes, and r4 is listed twice and gives both its occurrences each time
#     pass 1: j = 0: prec (e0, 7) (e4, 17), pos 1;  j = 2: pos 1 - 7 - 10 = -16;  and again
#     pass 2: j = 0: pos 1;  j = 2: prec (inv[e0] = e1, 7) (inv[e4] = e4, 17), pos -16;  and again
#     prec: (e4, 17) four times -- one short of an anchor
#     reads: (4, T) and (4, F), the mate (5, F) four times over
HAND = dict(K=4, inv=[1, 0, 3, 2, 4, 5], kmers=[10, 10, 20, 20, 7, 3], pairs=[(0, 3), (4, 1)], dup=[0, 0, 0, 1],
            paths=[[0, 2], [], [3, 1], [0], [4, 0, 4], [5], [2], [2]], offsets=[5, 0, 2, -3, 1, 0, 0, 0])
T, F = True, False
HAND_LOCS = [[(0, 5, T), (3, -3, T), (4, -6, T), (2, -18, F)],
             [(0, -5, T), (6, 0, T), (7, 0, T), (2, 2, F)],
             [(4, 1, T), (4, -16, T), (4, 1, T), (4, -16, T), (4, 1, F), (4, -16, F), (4, 1, F), (4, -16, F)]]
HAND_READS = [[(0, T), (1, F), (2, F), (3, T), (4, T), (5, F)], [(0, T), (1, F), (2, F)], [(4, F), (4, T), (5, F)]]


def run_hand(**change):
    h = dict(HAND); h.update(change)
    return closer_oracle.run(h["paths"], h["offsets"], h["kmers"], h["inv"], h["pairs"], h["dup"], h["K"])


def test_rule_on_a_graph_worked_out_by_hand():
    r = run_hand()
    assert r["ce"] == [0, 2, 4]
    assert [p["locs"] for p in r["per"]] == HAND_LOCS and [p["reads"] for p in r["per"]] == HAND_READS
    assert sorted(r["per"][0]["prec"]) == [(2, 10), (2, 10), (4, 10)] and r["per"][1]["prec"] == []
    assert sorted(r["per"][2]["prec"]) == [(0, 7)] * 2 + [(1, 7)] * 2 + [(4, 17)] * 4
    assert r["anchors"] == [] and r["runs_of_4"] == 1
    assert (len(r["locs"]), r["prec"], len(r["reads"]), r["dup_skipped"], r["mates_in"], r["mates_out"], r["mates_unplaced"], r["longest"]) == (16, 11, 12, 2, 8, 0, 2, 8)
    # a fifth (e4, 17): r5 = [e4, e0, e4] too -- its own double listing gives four more -- makes the anchor
    more = run_hand(paths=HAND["paths"][:5] + [[4, 0, 4]] + HAND["paths"][6:], offsets=[5, 0, 2, -3, 1, 1, 0, 0])
    assert more["per"][2]["anchors"] == [(4, 17, 8)] and more["anchor_first"] == [0, 0, 0, 1]
    # the files
    f = r["files"]
    assert f["a.close.edges"] == b"BINWRITE" + struct.pack("<Q", 3) + np.asarray([0, 2, 4], "<u8").tobytes()
    want = b"DFKCLOC1" + struct.pack("<Q4Q", 3, 0, 4, 8, 16) + b"".join(struct.pack("<qiI", id, pos, fw) for l in HAND_LOCS for id, pos, fw in l)
    assert f["a.close.locs"] == want
    assert f["a.close.anchors"] == b"DFKCANC1" + struct.pack("<Q4Q", 3, 0, 0, 0, 0)
    assert more["files"]["a.close.anchors"] == b"DFKCANC1" + struct.pack("<Q4Q", 3, 0, 0, 0, 1) + struct.pack("<iii", 4, 17, 8)
    assert f["a.close.reads"] == b"DFKCRDS1" + struct.pack("<Q4Q", 3, 0, 6, 9, 12) + b"".join(struct.pack("<Q", id << 1 | fw) for l in HAND_READS for id, fw in l)
    # a pair given again or reversed adds its own closer edges and leaves the others' elements alone
    again = run_hand(pairs=HAND["pairs"] + [(0, 3)])
    assert again["files"] == f
    rev = run_hand(pairs=HAND["pairs"] + [(3, 0)])                    # (e3, e0): closer edges e3 and inv[e0] = e1
    assert rev["ce"] == [0, 1, 2, 3, 4] and [rev["per"][k]["locs"] for k in (0, 2, 4)] == HAND_LOCS
    # no pairs: four valid files with n = 0
    e = run_hand(pairs=[])["files"]
    assert e["a.close.edges"] == b"BINWRITE" + bytes(8) and [e[n] for n in closer_oracle.FILES[1:]] == [m + bytes(16) for m in (b"DFKCLOC1", b"DFKCANC1", b"DFKCRDS1")]


def pairs_compose(i, r):
    """the per-pair idsfw of the text's two spasses = the composition of the per-edge sets"""
    index = i.get("index") or closer_oracle.make_index(i["paths"], len(i["inv"]))
    rank = {e: k for k, e in enumerate(r["ce"])}
    for e1, e2 in sorted(set(i["pairs"])):
        lit = closer_oracle.pair_idsfw(e1, e2, i["paths"], i["offsets"], index, i["kmers"], i["inv"], i["dup"], i["K"])
        assert lit == closer_oracle.compose(r["per"][rank[e1]]["reads"], r["per"][rank[i["inv"][e2]]]["reads"]), (e1, e2)
    return len(set(i["pairs"]))


def test_a_pair_takes_the_composition_of_two_edges_sets(golden_dir):
    assert pairs_compose(HAND, run_hand()) == 2
    for name, c, _ in closer_cases.seeded():
        if len(c["paths"]) <= 300: pairs_compose(c, closer_cases.oracle(c))
    case = FIXTURES["graph_frag_k48"]
    assert pairs_compose(closer_oracle.fixture_inputs(golden_dir, *case), closer_oracle.fixture_closer(golden_dir, *case)) == 937


@pytest.mark.parametrize("row", TABLE, ids=[r[0] for r in TABLE])
def test_restatement_gives_the_counts_of_the_fixtures(golden_dir, row):
    case, n_ce, n_locs, prec, n_anchors, of_4, of_5, n_reads, dup_skipped, mates_in, unplaced, longest, mates_out, twice = row
    r = closer_oracle.fixture_closer(golden_dir, *FIXTURES[case])
    i = closer_oracle.fixture_inputs(golden_dir, *FIXTURES[case])
    assert (len(r["ce"]), len(r["locs"]), r["prec"], len(r["anchors"]), r["runs_of_4"], r["runs_of_5"], len(r["reads"])) == (n_ce, n_locs, prec, n_anchors, of_4, of_5, n_reads)
    assert (r["dup_skipped"], r["mates_in"], r["mates_unplaced"], r["longest"], r["mates_out"]) == (dup_skipped, mates_in, unplaced, longest, mates_out)
    assert i["reference_index"] == i["reference_dup"] == (case in ("graph_frag_k48", "graph_pathy2_k48"))
    # no fixture has a self-inverse closer edge; only graph_k40_nobc has reads that cross a closer edge (or its involution) twice
    assert not [e for e in r["ce"] if i["inv"][e] == e]
    crossings = sum(1 for e in r["ce"] for f in {e, i["inv"][e]} for id in set(i["index"][f]) if i["paths"][id].count(f) > 1)
    assert crossings == twice
    assert r["loc_first"][-1] == n_locs and r["anchor_first"][-1] == n_anchors and r["read_first"][-1] == n_reads and len(r["loc_first"]) == n_ce + 1


def test_seeded_cases_supply_what_the_fixtures_lack():
    got = {name: (c, closer_cases.oracle(c)) for name, c, _ in closer_cases.seeded()}
    n_planted = 0
    for name, (c, r) in got.items():
        if not c["planted"]: continue
        n_planted += 1
        S, inv, km = len(c["inv"]) - 1, c["inv"], c["kmers"]
        per = dict(zip(r["ce"], r["per"]))
        assert inv[S] == S and S in per                                                             # a self-inverse closer edge
        assert [l for l in per[0]["locs"] if l[0] == 0] == [(0, 0, T), (0, -km[0] - km[8], T)] * 2, name          # a double crossing: 4 records
        assert len([l for l in per[S]["locs"] if l[0] == 2]) == 18 and [l[2] for l in per[S]["locs"] if l[0] == 2] == [T] * 9 + [F] * 9      # a triple one: 9 a pass
        assert (12, km[2], 5) in per[2]["anchors"] and sorted(per[2]["prec"]).count((13, km[2])) == 4 and not [a for a in per[2]["anchors"] if a[0] == 13]
        assert sum(1 for i in (4, 6, 8, 10) for e in c["paths"][i] if e == 2) == 5 and len({4, 6, 8, 10}) == 4       # ... four reads: the fifth is r4's second listing
        assert km[6] + c["K"] - 1 - c["offsets"][20] == 800 and km[6] + c["K"] - 1 - c["offsets"][22] == 801
        assert (21, F) in per[6]["reads"] and (23, F) not in per[6]["reads"] and (20, T) in per[6]["reads"] and (22, T) in per[6]["reads"]
        assert c["dup"][12] and (24, 0, T) in per[6]["locs"] and not [x for x in per[6]["reads"] if x[0] in (24, 25)]  # a duplicate pair: in locs, not in reads, no mate
        assert (27, T) in per[0]["reads"] and (27, F) in per[0]["reads"]                           # an id with both flags
        assert 0 in per and 1 in per and inv[0] == 1                                               # e and inv[e] both closer edges
        assert 10 in per and per[10]["locs"] == [] and per[10]["reads"] == [] and per[10]["anchors"] == []           # a closer edge nobody crosses
        assert c["pairs"][-2] == c["pairs"][0] and c["pairs"][-1] == c["pairs"][0][::-1]           # a pair given twice and reversed
        assert r["mates_out"] >= 1
    assert n_planted == 2
    assert got["no-pairs"][1]["ce"] == [] and got["no-pairs"][1]["locs"] == []
    assert len(got["no-reads"][1]["ce"]) > 0 and got["no-reads"][1]["locs"] == [] and got["no-reads"][1]["reads"] == []
    assert 256 < got["over-256"][1]["longest"] <= 1024 < got["over-1024"][1]["longest"]
    # device_scan's tile is SCAN_THREADS x SCAN_ITEMS = 256 x 8 (dfk_kernels.h), the sort's RS_TILE = 64 x RS_ROUNDS = 2048 (dfk_paths_kernels.h)
    SCAN_TILE, RS_TILE = 256 * 8, 64 * 32
    c, r = got["over-1024"]
    assert len(c["paths"]) > 2 * SCAN_TILE and len(r["locs"]) > 2 * RS_TILE and r["prec"] > 2 * RS_TILE and len(r["reads"]) > 2 * RS_TILE
    assert any(len(a["anchors"]) for _, a in got.values())


def test_digest_is_positional_and_the_words_are_the_files_bytes():
    r = run_hand()
    lw = closer_oracle.loc_words(r["locs"])
    assert lw.astype("<u8").tobytes() == r["files"]["a.close.locs"][16 + 8 * 4:]
    a, b, c = closer_oracle.seq_digest(lw, 0xAAAA), closer_oracle.seq_digest(lw[:8], 0xAAAA), closer_oracle.seq_digest(lw[8:], 0xAAAA + 8)
    assert ((b[0] + c[0]) & (2**64 - 1), b[1] ^ c[1]) == a and closer_oracle.seq_digest([], 1) == (0, 0)
    assert closer_oracle.anchor_words([(4, -1, 8)]).tolist() == [4, 2**32 - 1, 8]
