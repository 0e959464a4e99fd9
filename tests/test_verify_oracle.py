"""The CPU form of the path verifier (oracle/verify_oracle.py) on the files the reference's own classes wrote
(tests/golden/graph_*/): what the device verifier (dfk_paths_verify) treats as hard invariants must hold on them -- no path with
edges that do not meet, no offset behind the first edge, no placed read without a k-mer where its path says it is -- and the
numbers it finds are the ones tests/test_gpu_verify.py expects from the device for the same inputs.  Then the same verifier on
those sets damaged one way at a time (tests/verify_cases.py): each counter moves as the damage says it must, by the exact count
where the damage fixes one, and the numbers are the ones tests/test_gpu_verify_damaged.py expects from the device.  CPU only."""
import os

import pytest

from oracle import paths_oracle, verify_oracle
from tests import verify_cases
from tests.test_paths_oracle import CASES, decode_paths, load_reads

# [placed, broken, hits, consistent, no anchor, all consistent, dictionary bad, outside] per fixture, as computed from the
# reference-written files by oracle/verify_oracle.py (kept here so that a change of the verifier's definition shows)
EXPECT = {
    "graph_k48": [1215, 0, 35372, 35185, 0, 1211, 0, 4937],
    "graph_k40_nobc": [1409, 0, 51780, 51394, 0, 1402, 0, 3723],
    "graph_k60_nobc": [771, 0, 20003, 20003, 0, 771, 0, 3386],
    "graph_hot_k48_minfreq2": [92, 0, 1652, 1652, 0, 92, 0, 134],
    "graph_special_k48": [700, 0, 37036, 37036, 0, 700, 0, 64],
    "graph_pathy_k48": [3357, 0, 146851, 146029, 0, 3302, 0, 1947],
    "graph_frag_k48": [5634, 0, 232037, 223901, 0, 5277, 0, 15832],
    "graph_pathy2_k48": [18556, 0, 772254, 757058, 0, 17781, 0, 27569],
    "graph_zoo_k40": [20461, 0, 1159855, 1148731, 0, 20251, 0, 19516],
    "graph_zoo_k48": [20170, 0, 996227, 987599, 0, 19982, 0, 19339],
    "graph_zoo_k60": [19566, 0, 762432, 757410, 0, 19421, 0, 14263],
}

# (reads or paths damaged, the same eight counters) per (fixture, class of tests/verify_cases.py), as oracle/verify_oracle.py computes them
# from the damaged set (`python -m tests.verify_cases` prints this table): the reference for tests/test_gpu_verify_damaged.py too
DAMAGED = {
    ("graph_k48", "offset_plus_one"): (405, [1215, 2, 35279, 23536, 403, 806, 0, 5009]),
    ("graph_k48", "offset_at_n"): (304, [1215, 152, 26669, 26374, 151, 943, 0, 7960]),
    ("graph_k48", "offset_extremes"): (304, [1215, 101, 26394, 26230, 203, 1111, 0, 10276]),
    ("graph_k48", "edge_to_inv"): (4, [1215, 4, 35228, 35052, 0, 1208, 0, 4925]),
    ("graph_k48", "sibling"): (8, [1215, 0, 35189, 35085, 0, 1211, 0, 5120]),
    ("graph_k48", "id_out_of_range"): (243, [1215, 243, 28493, 28317, 0, 969, 0, 4083]),
    ("graph_k48", "id_behind_a_good_edge"): (8, [1215, 8, 34996, 34996, 0, 1207, 0, 4915]),
    ("graph_k48", "lengthened"): (61, [1215, 0, 35438, 35185, 0, 1209, 0, 4871]),
    ("graph_k48", "short_read"): (174, [1215, 0, 30295, 30131, 174, 1038, 0, 4243]),
    ("graph_k48", "other_reads"): (1800, [1215, 0, 20659, 0, 1215, 287, 0, 7154]),
    ("graph_k48", "unplaced"): (1215, [0, 0, 0, 0, 0, 0, 0, 0]),
    ("graph_k48", "no_reads"): (1800, [0, 0, 0, 0, 0, 0, 0, 0]),
    ("graph_k40_nobc", "offset_plus_one"): (470, [1409, 3, 51611, 34720, 467, 933, 0, 3661]),
    ("graph_k40_nobc", "offset_at_n"): (353, [1409, 177, 39374, 38829, 176, 1097, 0, 9461]),
    ("graph_k40_nobc", "offset_extremes"): (352, [1409, 117, 38785, 38580, 235, 1288, 0, 11876]),
    ("graph_k40_nobc", "edge_to_inv"): (17, [1409, 17, 50890, 50713, 0, 1388, 0, 3717]),
    ("graph_k40_nobc", "sibling"): (21, [1409, 0, 51355, 51131, 0, 1394, 0, 4148]),
    ("graph_k40_nobc", "id_out_of_range"): (282, [1409, 282, 41301, 40946, 0, 1121, 0, 3041]),
    ("graph_k40_nobc", "id_behind_a_good_edge"): (33, [1409, 33, 50111, 50106, 0, 1375, 0, 3702]),
    ("graph_k40_nobc", "lengthened"): (131, [1409, 0, 51880, 51399, 0, 1399, 0, 3623]),
    ("graph_k40_nobc", "short_read"): (202, [1409, 0, 44274, 43888, 202, 1200, 0, 3387]),
    ("graph_k40_nobc", "other_reads"): (1800, [1409, 0, 37746, 0, 1409, 161, 0, 6371]),
    ("graph_k40_nobc", "unplaced"): (1409, [0, 0, 0, 0, 0, 0, 0, 0]),
    ("graph_k40_nobc", "no_reads"): (1800, [0, 0, 0, 0, 0, 0, 0, 0]),
    ("graph_k60_nobc", "offset_plus_one"): (257, [771, 1, 19896, 13178, 256, 515, 0, 3492]),
    ("graph_k60_nobc", "offset_at_n"): (193, [771, 97, 14924, 14837, 96, 614, 0, 5598]),
    ("graph_k60_nobc", "offset_extremes"): (193, [771, 64, 15141, 15141, 129, 707, 0, 6473]),
    ("graph_k60_nobc", "id_out_of_range"): (155, [771, 155, 16084, 16084, 0, 616, 0, 2573]),
    ("graph_k60_nobc", "short_read"): (111, [771, 0, 17029, 17029, 111, 660, 0, 2652]),
    ("graph_k60_nobc", "other_reads"): (1800, [771, 0, 6044, 0, 771, 210, 0, 3888]),
    ("graph_k60_nobc", "unplaced"): (771, [0, 0, 0, 0, 0, 0, 0, 0]),
    ("graph_k60_nobc", "no_reads"): (1800, [0, 0, 0, 0, 0, 0, 0, 0]),
    ("graph_frag_k48", "offset_plus_one"): (1878, [5634, 24, 230967, 148707, 1854, 3514, 0, 16008]),
    ("graph_frag_k48", "offset_at_n"): (1409, [5634, 705, 191001, 168035, 691, 4032, 0, 26353]),
    ("graph_frag_k48", "offset_extremes"): (1409, [5634, 470, 173350, 167275, 939, 4900, 0, 54192]),
    ("graph_frag_k48", "edge_to_inv"): (1616, [5634, 1616, 160435, 155436, 0, 3793, 0, 13792]),
    ("graph_frag_k48", "sibling"): (2043, [5634, 0, 225159, 176047, 104, 3492, 0, 22710]),
    ("graph_frag_k48", "id_out_of_range"): (1127, [5634, 1127, 185892, 179363, 0, 4223, 0, 12672]),
    ("graph_frag_k48", "id_behind_a_good_edge"): (3231, [5634, 3231, 87182, 85927, 0, 2341, 0, 12147]),
    ("graph_frag_k48", "lengthened"): (1540, [5634, 0, 232966, 224410, 0, 5212, 0, 14903]),
    ("graph_frag_k48", "short_read"): (805, [5634, 0, 198953, 192134, 805, 4525, 0, 13378]),
    ("graph_frag_k48", "other_reads"): (6000, [5634, 0, 217199, 39, 5633, 151, 0, 23778]),
    ("graph_frag_k48", "unplaced"): (5634, [0, 0, 0, 0, 0, 0, 0, 0]),
    ("graph_frag_k48", "no_reads"): (6000, [0, 0, 0, 0, 0, 0, 0, 0]),
}


def fixture_counters(golden_dir, case, K, which):
    d = os.path.join(golden_dir, case)
    edges, left, right, _ = verify_oracle.load_graph_dir(d, K)
    paths = decode_paths(open(os.path.join(d, "a.paths"), "rb").read())
    reads, _ = paths_oracle.unpack_reads(load_reads(golden_dir, which))
    return verify_oracle.verify(edges, left, right, paths, reads, K)


@pytest.mark.parametrize("case,K,npz,which", CASES)
def test_reference_written_paths_satisfy_the_verifier(golden_dir, case, K, npz, which):
    c = fixture_counters(golden_dir, case, K, which)
    assert c == EXPECT[case]
    assert c[1] == 0 and c[4] == 0 and c[6] == 0          # the hard invariants
    assert c[3] >= 0.96 * c[2]                            # nearly every dictionary hit is where the path says


def test_verifier_sees_a_broken_path(golden_dir):
    """...and it is not blind: shift one read's offset, swap an edge for its neighbour, move a read to another's path."""
    case, K, _, which = CASES[0]
    d = os.path.join(golden_dir, case)
    edges, left, right, _ = verify_oracle.load_graph_dir(d, K)
    paths = decode_paths(open(os.path.join(d, "a.paths"), "rb").read())
    reads, _ = paths_oracle.unpack_reads(load_reads(golden_dir, which))
    placed = [i for i, (_, p) in enumerate(paths) if p]
    good = verify_oracle.verify(edges, left, right, paths, reads, K)
    i = placed[0]
    shifted = list(paths); shifted[i] = (paths[i][0] + 1, paths[i][1])
    c = verify_oracle.verify(edges, left, right, shifted, reads, K)
    assert c[3] < good[3] and c[4] == 1
    two = next(j for j in placed if len(paths[j][1]) >= 2)
    cut = list(paths); cut[two] = (paths[two][0], [paths[two][1][0], paths[two][1][0] ^ 1])
    c = verify_oracle.verify(edges, left, right, cut, reads, K)
    assert c[1] >= 1 or c[3] < good[3]


def test_digest_forms_distinguish_files(golden_dir):
    d = os.path.join(golden_dir, "graph_frag_k48")
    _, _, _, inv = verify_oracle.load_graph_dir(d, 48)
    paths = decode_paths(open(os.path.join(d, "a.paths"), "rb").read())
    f = lambda n: open(os.path.join(d, n), "rb").read()
    w = verify_oracle.expected_check_words(paths, f("a.paths.inv"), f("a.countsb"), f("a.dup"), inv)
    assert w["COUNTSB_SUM"] == 2 * w["INV_ENTRIES"] - w["SELF_INVERSE"] and w["INV_ENTRIES"] == w["N_PATH_EDGES"]
    assert 0 < w["DUP_MARKED"] <= w["N_PLACED"] // 2 + 1
    swapped = list(paths); swapped[0], swapped[1] = swapped[1], swapped[0]
    if swapped[0] != swapped[1]:
        assert verify_oracle.paths_digest(swapped) != (w["PATHS_SUM"], w["PATHS_XOR"])


def run_damaged(golden_dir, fixture, cls):
    f = verify_cases.load(golden_dir, fixture)
    name, paths, reads, n = verify_cases.damaged(golden_dir, fixture, cls)
    return f, paths, reads, n, verify_oracle.verify(f["edges"], f["to_left"], f["to_right"], paths, reads, f["K"])


@pytest.mark.parametrize("fixture,cls", verify_cases.CASES)
def test_verifier_counts_each_kind_of_damage(golden_dir, fixture, cls):
    """[placed, broken, hits, consistent, no anchor, all consistent, dictionary bad, outside] under one kind of damage: the recorded
    numbers, and what the damage itself implies about them (good = the undamaged fixture's)."""
    f, paths, reads, n, c = run_damaged(golden_dir, fixture, cls)
    good = EXPECT[fixture]
    assert (n, c) == DAMAGED[fixture, cls]
    assert n > 0 and c[6] == 0
    if cls not in ("unplaced", "no_reads"):
        assert c[0] == good[0]
    if cls == "offset_plus_one":
        assert c[3] < good[3] and c[4] > 0.9 * n and 0 < c[1] < 0.05 * n and c[1] + c[4] == n   # every shifted read: no k-mer where the path says, or behind its edge
    elif cls == "offset_at_n":
        assert c[1] == verify_cases.n_set_to_n(n) and n >= 2                # offset == n: broken, every one; offset == n - 1: none
    elif cls == "offset_extremes":
        assert c[1] == verify_cases.n_set_to_max(n) and c[4] == n - c[1] and c[7] > good[7] and n >= 3
    elif cls in ("edge_to_inv", "id_out_of_range", "id_behind_a_good_edge"):
        assert c[1] == n
    elif cls == "sibling":
        assert c[1] == 0 and c[3] < good[3]
    elif cls == "lengthened":
        assert c[1] == 0 and c[4] == 0 and c[7] < good[7] and c[2] > good[2] and c[3] >= good[3]
        if fixture == "graph_frag_k48":                                      # (the small graphs end after an edge or two)
            assert max(len(p) for _, p in paths) == 9 and max(len(p) for _, p in f["paths"]) == 4
    elif cls == "short_read":
        assert c[1] == 0 and c[4] == n
    elif cls == "other_reads":
        # a repeat can put a k-mer of another read where this read's path says: frag has 39 such hits in 217199, on one read
        assert c[1] == 0 and c[3] * 1000 < good[3] and c[4] >= c[0] - 1
        if fixture != "graph_frag_k48":
            assert c[3] == 0 and c[4] == c[0]
    else:
        assert c == [0] * 8
    undamaged = verify_oracle.paths_digest(f["paths"])
    if cls in verify_cases.CHANGE_NO_PATH:
        assert paths is f["paths"] and verify_oracle.paths_digest(paths) == undamaged
    else:
        assert verify_oracle.paths_digest(paths) != undamaged


def test_damage_classes_reach_what_they_are_for(golden_dir):
    """The fixtures supply every class: both kinds of id, at both ends; siblings; every cause of `broken` on its own."""
    f = verify_cases.load(golden_dir, "graph_frag_k48")
    E = len(f["edges"])
    assert sum(1 for _, p in f["paths"] if len(p) >= 2) == 3231
    _, paths, _, n = verify_cases.damaged(golden_dir, "graph_frag_k48", "sibling")
    assert n >= 20
    assert all(f["to_right"][a] == f["to_left"][b] for _, p in paths for a, b in zip(p, p[1:]))
    for fixture, _, _ in verify_cases.FIXTURES:
        g = verify_cases.load(golden_dir, fixture)
        _, paths, _, n = verify_cases.damaged(golden_dir, fixture, "id_out_of_range")
        bad = [(p.index(e), len(p), e) for (_, p) in paths for e in p if not 0 <= e < len(g["edges"])]
        assert len(bad) == n and {e for _, _, e in bad} == {len(g["edges"]), -1}
        assert any(at == 0 for at, _, _ in bad)
        if fixture == "graph_frag_k48":                                     # (elsewhere every 5th read misses the few longer paths:
            assert any(at > 0 for at, _, _ in bad)                          # id_behind_a_good_edge takes them all)
    _, paths, _, n = verify_cases.damaged(golden_dir, "graph_frag_k48", "id_behind_a_good_edge")
    assert n == 3231 and all(0 <= e < E for _, p in paths for e in p[:-1])
    _, paths, _, n = verify_cases.damaged(golden_dir, "graph_frag_k48", "edge_to_inv")
    assert all(0 <= e < E for _, p in paths for e in p)                     # (broken by the meet test alone)


def test_pack_reads_round_trips(golden_dir):
    f = verify_cases.load(golden_dir, "graph_k60_nobc")
    packed, base_off, read_len = verify_cases.pack_reads(f["reads"])
    back, _ = paths_oracle.unpack_reads(dict(packed=packed, base_off=base_off, read_len=read_len, pq_bytes=f["rs"]["pq_bytes"], pq_off=f["rs"]["pq_off"]))
    assert back == f["reads"]
    packed, base_off, read_len = verify_cases.pack_reads([bytes([1, 2, 3, 0, 3]), b"", bytes([2])])
    assert list(read_len) == [5, 0, 1] and list(base_off) == [0, 2, 2, 3] and list(packed) == [1 | 2 << 2 | 3 << 4, 3, 2]
