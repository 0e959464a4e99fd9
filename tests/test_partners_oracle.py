"""tests/partners_oracle.py (CloseGap2's search for unplaced partners, 10X/Closomatic.cc:554-585, restated per pair) on a graph worked out
by hand and on the fixtures: the closer tables from tests/closer_oracle.py, the edges' bases from the reference-written a.fastb, the
fixtures' reads.  CPU only."""
import struct

import numpy as np
import pytest

from tests import partners_oracle
from tests.test_closer_oracle import FIXTURES

# fixture, pairs, queries, read positions, queries with any hit, kept, with several positions, largest bod (after UniqueSort), table entries
TABLE = [("graph_pathy2_k48", 725, 47552, 4235662, 274, 265, 9, 600, 63079),
         ("graph_frag_k48", 937, 11798, 814062, 2168, 2168, 0, 211, 30090),
         ("graph_pathy_k48", 63, 5259, 466977, 55, 45, 10, 496, 9945),
         ("graph_k40_nobc", 138, 11598, 606012, 7, 7, 0, 453, 894)]

# ---- a graph worked out by hand.
# Five edges: e0/e1 and e2/e3 are involution pairs, e4 is its own involution.  U is 40 bases with no 32-mer twice.
#   bases(e2) = U: nine 32-mers      bases(e4) = U[4:36]: one, e2's at l = 4      e0, e1, e3: 20 bases, none
# The pair (e0, e3): es = { e0, inv[e3] = e2 }, ce = [0, 2].
#   locs(e0) = (0, 5, T) (0, 9, T) (2, 1, T) (7, 0, F)      ids = [0, 2]: read 0 once, read 7 not at all
#   locs(e2) = (3, 4, T) (6, 2, T) (1, 7, F)                ids = [3, 6]
#   anchors(e0) = (e4, 100, 5)                  bod(e0) = ( U[4:36], 100 )
#   anchors(e2) = (e2, 10, 5) (e4, 14, 6)       bod(e2) = ( U[l:l+32], 10 + l ) for l = 0 .. 8, and ( U[4:36], 14 ) -- which it holds already
# ei = 0: the mates of 0 and 2 are 1 and 3.  3 is in ids(e2): skipped.  1 is on e2 backward only: searched.
#         r1 = "GG" + U[2:38], 38 bases, l = 0 .. 6: at l = 2 .. 6 it is U[l:l+32]: 10 + l - l = 10 five times (and 14 - 4 at l = 4): ( 1, 10 )
# ei = 1: the mates of 3 and 6 are 2 and 7.  2 is in ids(e0): skipped.  7 is on e0 backward only: searched against bod(e0).
#         r7 = U[4:36] twice over, 64 bases, l = 0 .. 32: hits at l = 0 and l = 32: 100 and 68 -- two values: dropped
#         with r7 = "T" + U[4:36] instead: l = 1: ( 7, 99 ), pushed onto locs[0]
U = "ACGTTGCAAGCTTCGGATCCATGGTACCGAGCTCGAATTC"
codes = lambda s: np.asarray(["ACGT".index(ch) for ch in s], np.uint8)
T, F = True, False
HAND = dict(inv=[1, 0, 3, 2, 4], edges=[codes("ACGT" * 5), codes("ACGT" * 5), codes(U), codes("TGCA" * 5), codes(U[4:36])], ce=[0, 2],
            locs=[[(0, 5, T), (0, 9, T), (2, 1, T), (7, 0, F)], [(3, 4, T), (6, 2, T), (1, 7, F)]], anchors=[[(4, 100, 5)], [(2, 10, 5), (4, 14, 6)]], pairs=[(0, 3)],
            reads=[codes("A" * 40), codes("GG" + U[2:38]), codes("C" * 40), codes(U), codes("A" * 31), codes(""), codes("G" * 50), codes(U[4:36] * 2)])


def run_hand(**change):
    h = dict(HAND); h.update(change)
    return partners_oracle.run(h["inv"], h["edges"], h["ce"], h["locs"], h["anchors"], h["pairs"], lambda id: h["reads"][id])


def test_rule_on_a_graph_worked_out_by_hand():
    assert len(U) == 40 and len(set(partners_oracle.kmers_of(codes(U)))) == 9
    r = run_hand()
    assert r["elements"] == [[(1, 10, T)], []] and r["starts"] == [0, 1, 1]
    assert (r["pairs"], r["queries"], r["positions"], r["any_hit"], r["kept"], r["multi"], r["entries"], r["largest_bod"]) == (1, 2, 7 + 33, 2, 1, 1, 1 + 9 + 1, 9)
    assert r["file"] == b"DFKCPRT1" + struct.pack("<Q3Q", 2, 0, 1, 1) + struct.pack("<qiI", 1, 10, 1)
    # one position instead of two: kept, onto locs[0]
    one = run_hand(reads=HAND["reads"][:7] + [codes("T" + U[4:36])])
    assert one["elements"] == [[(1, 10, T)], [(7, 99, T)]] and (one["kept"], one["multi"], one["positions"]) == (2, 0, 7 + 2)
    assert one["file"] == b"DFKCPRT1" + struct.pack("<Q3Q", 2, 0, 1, 2) + struct.pack("<qiI", 1, 10, 1) + struct.pack("<qiI", 7, 99, 1)
    # a record with fw false does not count, even when the same id has one with fw true: 1 forward on e2 -> the mate of 0 is skipped
    placed = run_hand(locs=[HAND["locs"][0], [(1, 0, T)] + HAND["locs"][1]])
    assert placed["elements"] == [[], []] and (placed["queries"], placed["multi"]) == (1, 1)       # (ids(e2) = [1, 3, 6]: the mate 0 is in ids(e0) too; 7 is still searched)
    # 31 bases: no position; a negative pos - l
    short = run_hand(reads=[HAND["reads"][0], codes(U[2:33])] + HAND["reads"][2:])
    assert short["elements"] == [[], []] and short["positions"] == 33
    neg = run_hand(reads=[HAND["reads"][0], codes("G" * 20 + U[0:32])] + HAND["reads"][2:])
    assert neg["elements"][0] == [(1, -10, T)]
    # the pair given again and reversed: (e2, e1) has es = { e2, inv[e1] = e0 }: the same two sides, the other way round
    both = run_hand(pairs=[(0, 3), (0, 3), (2, 1)])
    assert both["elements"] == [[(1, 10, T)], [], [(1, 10, T)], [], [], [(1, 10, T)]] and both["starts"] == [0, 1, 1, 2, 2, 2, 3] and both["queries"] == 6
    # no pairs: a valid file with n = 0
    assert run_hand(pairs=[])["file"] == b"DFKCPRT1" + bytes(16)
    # the digest is k_digest_seq's over the records' words
    assert r["digest"] == partners_oracle.seq_digest(np.asarray([1, 10 | 1 << 32], np.uint64), partners_oracle.SALT) and run_hand(pairs=[])["digest"] == (0, 0)


def test_32mers_as_numbers():
    a = partners_oracle.kmers_of(np.zeros(33, np.uint8))
    t = partners_oracle.kmers_of(np.full(32, 3, np.uint8))
    assert a == [0, 0] and t == [2**64 - 1] and partners_oracle.kmers_of(np.zeros(31, np.uint8)) == []
    c = codes(U)
    assert partners_oracle.kmers_of(c)[3] == sum(int(c[3 + j]) << (2 * j) for j in range(32))
    # unpack: the .fastb's packing, a sequence that starts at an odd byte
    assert list(partners_oracle.unpack(np.asarray([0xFF, 0x1B, 0x02], np.uint8), 1, 5)) == [3, 2, 1, 0, 2]


@pytest.mark.parametrize("row", TABLE, ids=[r[0] for r in TABLE])
def test_restatement_gives_the_counts_of_the_fixtures(golden_dir, row):
    case, pairs, queries, positions, any_hit, kept, multi, largest, entries = row
    r = partners_oracle.fixture_partners(golden_dir, *FIXTURES[case])
    assert (r["pairs"], r["queries"], r["positions"], r["any_hit"], r["kept"], r["multi"], r["largest_bod"], r["entries"]) == (pairs, queries, positions, any_hit, kept, multi, largest, entries)
    assert r["kept"] > 0 and len(r["records"]) == r["kept"] and r["starts"][-1] == r["kept"] and len(r["starts"]) == 2 * pairs + 1
    assert len(r["file"]) == 16 + 8 * (2 * pairs + 1) + 16 * kept and all(fw for _, _, fw in r["records"])
    i = partners_oracle.fixture_inputs(golden_dir, *FIXTURES[case])
    # every record is a read that is not forward on the edge it is pushed onto, and its mate is forward on the other
    rank = {e: k for k, e in enumerate(i["ce"])}
    for pi, (e1, e2) in enumerate(i["pairs"]):
        ks = [rank[e1], rank[i["inv"][e2]]]
        for ei in (0, 1):
            ids, other = partners_oracle.ids_of(i["locs_per"][ks[ei]]), partners_oracle.ids_of(i["locs_per"][ks[1 - ei]])
            for id2, _, _ in r["elements"][2 * pi + ei]: assert id2 ^ 1 in ids and id2 not in other


def test_fixtures_hold_kept_and_dropped_partners_and_reads_of_many_lengths(golden_dir):
    r = partners_oracle.fixture_partners(golden_dir, *FIXTURES["graph_pathy2_k48"])
    i = partners_oracle.fixture_inputs(golden_dir, *FIXTURES["graph_pathy2_k48"])
    lens = i["rs"]["read_len"]
    assert r["multi"] > 0 and (int(lens.min()), int(lens.max())) == (100, 151)
    short = partners_oracle.fixture_inputs(golden_dir, *FIXTURES["graph_k40_nobc"])["rs"]["read_len"]          # reads of fewer than 32 bases: graph_k40_nobc's
    assert int(short.min()) == 30 and int(short.max()) == 151
    assert len({int(lens[id]) for id, _, _ in r["records"]}) == 4 and min(pos for _, pos, _ in r["records"]) == -29        # reads of four lengths kept, one before the edge's start
