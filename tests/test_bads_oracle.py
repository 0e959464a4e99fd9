"""tests/bads_oracle.py (MarkBads, 10X/SecretOps.cc:71-109, restated) on a case worked out by hand and on the fixtures whose
paths and edges the reference's classes wrote.  CPU only."""
import os

import numpy as np
import pytest

from oracle import paths_oracle
from tests import bads_oracle
from tests.test_paths_oracle import decode_paths, load_reads

# fixture, K, reads from, reads, placed, sum > 0, marked pairs, largest sum, sum == 150, multi-edge paths, hang left, hang right
TABLE = [("graph_pathy2_k48", 48, "pathy2", 23400, 18556, 13768, 1309, None, 2, 8583, 1464, 3255),
         ("graph_pathy_k48", 48, "pathy", 3600, 3357, 2469, 2, None, 0, 1826, 193, 380),
         ("graph_frag_k48", 48, "frag", 6000, 5634, 1854, 0, 111, 0, 3231, 702, 1046),
         ("graph_k48", 48, "reads", 1800, 1215, 505, 6, 1437, 0, 8, 153, 334),
         ("graph_k40_nobc", 40, "reads", 1800, 1409, 693, 8, 1847, 0, 33, 88, 208),
         ("graph_k60_nobc", 60, "reads", 1800, 771, 271, 0, 120, 0, 3, 196, 348),
         # the zoo (tests/zoo_synth.py): a tenth of its reads carry one to three substitutions of quality 30 to 60
         ("graph_zoo_k40", 40, "zoo", 20624, 20461, 2129, 285, 3060, 80, 14504, 176, 2432),
         ("graph_zoo_k48", 48, "zoo", 20624, 20170, 1820, 234, 2820, 54, 13264, 154, 2260),
         ("graph_zoo_k60", 60, "zoo", 20624, 19566, 1196, 159, 1920, 25, 8021, 90, 1796)]

_cache = {}


def fixture_expected(golden_dir, case, K, which):
    """(paths, reads, quals, edges, sums) of a fixture; computed once per session and handed out unchanged"""
    if case not in _cache:
        reads, quals = paths_oracle.unpack_reads(load_reads(golden_dir, which))
        paths = decode_paths(open(os.path.join(golden_dir, case, "a.paths"), "rb").read())
        edges = bads_oracle.fixture_edges(golden_dir, case)
        sums = bads_oracle.bad_sums(paths, reads, quals, edges, K)
        sums.setflags(write=False)
        _cache[case] = (paths, reads, quals, edges, sums)
    return _cache[case]


def test_rule_on_a_case_worked_out_by_hand():
    K = 4                                               # neighbours share K-1 = 3 bases
    e0 = bytes([0, 1, 2, 3, 0, 1, 2, 3, 0, 1])          # ends 3,0,1
    e1 = bytes([3, 0, 1, 2, 2, 1, 0, 3])                # starts 3,0,1
    e2 = bytes([2, 3, 0, 1, 2, 3, 0, 1, 2, 3])          # the reverse complement of e0: the HBV edge a read on e0's other strand lies on
    assert e2 == bytes(3 - b for b in reversed(e0))
    edges = [e0, e1, e2]
    # Cat(e0, e1) = 0123012301 + 22103 (e1 from its base 3 on): fifteen bases
    m = [0, 1, 2, 3, 0, 1, 2, 3, 0, 1, 2, 2, 1, 0, 3]
    assert list(bads_oracle.cat([0, 1], edges, K)) == m
    cases = [
        # r0: offset -2, read bases 0 and 1 hang over the left end and are skipped whatever they are (qualities 40 do not count);
        #     base l lies on m[l-2]: 0,1,2,0,0,1 against m[0..5] = 0,1,2,3,0,1 -> one mismatch at l = 5, quality 25
        ((-2, [0, 1]), [3, 3, 0, 1, 2, 0, 0, 1], [40, 40, 10, 10, 10, 25, 10, 10], 25),
        # r1: offset 11, m ends at 15: only l = 0..3 count, against m[11..14] = 2,1,0,3; l = 1 differs (quality 30); the four
        #     bases beyond the right end carry quality 63 and are skipped
        ((11, [0, 1]), [2, 0, 0, 3, 1, 1, 1, 1], [5, 30, 5, 5, 63, 63, 63, 63], 30),
        # r2: on the reverse-complement edge at offset 1: m[1..6] = 3,0,1,2,3,0 against 3,0,2,2,3,1 -> l = 2 (7) and l = 5 (9)
        ((1, [2]), [3, 0, 2, 2, 3, 1], [1, 1, 7, 1, 1, 9], 16),
        # r3: on e1 = 3,0,1,2,2,1,0,3 at offset 0: 0,0,1,3,2,2,0,3 differs at l = 0, 3, 5 -> 50 + 50 + 50 = 150 exactly
        ((0, [1]), [0, 0, 1, 3, 2, 2, 0, 3], [50, 1, 1, 50, 1, 50, 1, 1], 150),
        # r4: the same read with one quality higher: 151
        ((0, [1]), [0, 0, 1, 3, 2, 2, 0, 3], [50, 1, 1, 50, 1, 51, 1, 1], 151),
        # r5: no path: nothing
        ((0, []), [0, 1, 2, 3, 0, 1], [60, 60, 60, 60, 60, 60], 0),
        # r6: across the junction, offset 6: m[6..13] = 2,3,0,1,2,2,1,0 against 2,3,0,1,2,0,1,0 -> l = 5 (m[11], on e1's share
        #     behind the K-1 shared bases; edges joined without their overlap would put a 0 there and count nothing), quality 12
        ((6, [0, 1]), [2, 3, 0, 1, 2, 0, 1, 0], [9, 9, 9, 9, 9, 12, 9, 9], 12),
        # r7: no path
        ((3, []), [1, 1, 1, 1], [30, 30, 30, 30], 0),
    ]
    paths = [c[0] for c in cases]
    reads = [bytes(c[1]) for c in cases]
    quals = [np.array(c[2], np.uint8) for c in cases]
    sums = bads_oracle.bad_sums(paths, reads, quals, edges, K)
    assert [int(s) for s in sums] == [c[3] for c in cases]
    # pairs (r0, r1) = (25, 30), (r2, r3) = (16, 150): 150 itself does not mark; (r4, r5) = (151, 0) does; (r6, r7) = (12, 0)
    assert list(bads_oracle.bad_marks(sums)) == [0, 0, 1, 0]
    assert bads_oracle.bad_file(sums) == b"BINWRITE" + (4).to_bytes(8, "little") + bytes([0, 0, 1, 0])
    assert list(bads_oracle.mismatch_positions(paths[2][1], paths[2][0], reads[2], edges, K)) == [2, 5]
    # a saturated sum is still above the threshold, and the digest is of the saturated value
    assert list(bads_oracle.bad_marks([70000, 0])) == [1] and bads_oracle.bad_digest([70000, 0]) == bads_oracle.bad_digest([65535, 0])
    # the digest of a run's ranks: sums add, xors xor
    a, b, whole = bads_oracle.bad_digest(sums[:4]), bads_oracle.bad_digest(sums[4:], first_read=4), bads_oracle.bad_digest(sums)
    assert ((a[0] + b[0]) & (2**64 - 1), a[1] ^ b[1]) == whole


@pytest.mark.parametrize("case,K,which,n,placed,nonzero,marked,largest,at150,multi,left,right", TABLE)
def test_restatement_gives_the_counts_of_the_fixtures(golden_dir, case, K, which, n, placed, nonzero, marked, largest, at150, multi, left, right):
    paths, reads, quals, edges, sums = fixture_expected(golden_dir, case, K, which)
    assert len(paths) == n and sum(1 for _, p in paths if p) == placed
    assert int((sums > 0).sum()) == nonzero
    assert int(bads_oracle.bad_marks(sums).sum()) == marked and len(bads_oracle.bad_marks(sums)) == n // 2
    if largest is not None:
        assert int(sums.max()) == largest
    assert int((sums == 150).sum()) == at150
    assert sum(1 for _, p in paths if len(p) > 1) == multi
    assert sum(1 for o, p in paths if p and o < 0) == left
    assert sum(1 for i, (o, p) in enumerate(paths) if p and o + len(reads[i]) > sum(len(edges[e]) - K + 1 for e in p) + K - 1) == right
    assert all(sums[i] == 0 for i, (_, p) in enumerate(paths) if not p)
