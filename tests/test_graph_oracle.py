"""The graph oracle (oracle/graph_oracle.py: unipath edges, canonical HBV, a.<K>/ files) against the fixtures the
reference's own classes produced (tests/golden/graph_*: oracle/_ref/refdrv graph = the real KmerDict and KMer walk the
edges, the real digraphE<basevector>, vecbvec and BinaryWriter write the files; oracle/ref_graph.cc).  CPU only."""
import os

import numpy as np
import pytest

from oracle import graph_oracle
from tests.test_oracle_golden import load_hot, load_inputs

FILES = ("a.k", "a.fastb", "a.hbv", "a.hbx", "a.kmers", "a.inv", "a.to_left", "a.to_right")
# (fixture dir, K, which expected dictionary)
CASES = [("graph_k48", 48, "expect_k48.npz"), ("graph_k40_nobc", 40, "expect_k40_nobc.npz"), ("graph_k60_nobc", 60, "expect_k60_nobc.npz"),
         ("graph_hot_k48_minfreq2", 48, "expect_hot_k48_minfreq2.npz"), ("graph_special_k48", 48, "expect_special_k48_nobc.npz")] + \
        [(f"graph_zoo_k{K}", K, f"expect_zoo_k{K}.npz") for K in (40, 48, 60)]


def expected_files(golden_dir, case):
    return {f: open(os.path.join(golden_dir, case, f), "rb").read() for f in FILES}


@pytest.mark.parametrize("case,K,npz", CASES)
def test_graph_oracle_matches_reference_files(golden_dir, case, K, npz):
    """From the reference's dictionary (post-recomputeAdjacencies entries) to every graph file, byte for byte."""
    solid = np.load(os.path.join(golden_dir, npz))["solid_post"]
    r = graph_oracle.run(solid, K)
    exp = expected_files(golden_dir, case)
    for f in FILES:
        assert r["files"][f] == exp[f], f"{case}/{f}"
    # every solid k-mer lies on exactly one canonical edge, at one offset
    assert len(r["place"]) == len(solid)
    assert sum(len(e) - K + 1 for e in r["edges"]) == len(solid)


def test_special_input_has_the_corner_cases(golden_dir):
    """The special fixture really contains a branch-free cycle, a palindromic one-k-mer edge and branch vertices."""
    solid = np.load(os.path.join(golden_dir, "expect_special_k48_nobc.npz"))["solid_post"]
    r = graph_oracle.run(solid, 48)
    h = r["hbv"]
    loops = [e for e, (a, b) in enumerate(zip(*h.to_left_right())) if a == b]
    assert any(len(h.edges[e]) == 400 + 47 for e in loops)                       # the 400-base circle: 400 k-mers, closed on itself
    assert any(len(s) == 48 and graph_oracle.rc_seq(s) == s for s in h.edges)    # the palindrome, an edge of its own
    assert max(len(v) for v in h.frm) >= 2                                       # a vertex with two outgoing edges
    inv = h.involution()
    assert all(inv[inv[e]] == e for e in range(len(inv)))


def test_oracle_chain_from_reads(oracle, golden_dir):
    """reads -> C oracle dictionary -> graph oracle reproduces the fixture too (the two restatements compose)."""
    rs = load_hot(golden_dir)
    r = oracle.run(rs["packed"], rs["base_off"], rs["read_len"], rs["pq_bytes"], rs["pq_off"], rs["bc"], K=48, min_freq=2)
    g = graph_oracle.run(r["solid"], 48)
    exp = expected_files(golden_dir, "graph_hot_k48_minfreq2")
    for f in FILES:
        assert g["files"][f] == exp[f], f
    rs = load_inputs(golden_dir)
    r = oracle.run(rs["packed"], rs["base_off"], rs["read_len"], rs["pq_bytes"], rs["pq_off"], None, K=60, min_freq=3, min_bc=0)
    g = graph_oracle.run(r["solid"], 60)
    exp = expected_files(golden_dir, "graph_k60_nobc")
    for f in FILES:
        assert g["files"][f] == exp[f], f


@pytest.mark.parametrize("K", [40, 48, 60])
def test_zoo_has_the_classes(golden_dir, K):
    """The zoo fixture (tests/zoo_synth.py through the reference's classes) really holds, at every K, the topology it was made for:
    this is what keeps it from silently losing a class when somebody regenerates it.  Everything is read from the reference's
    dictionary and files.  Two things cannot exist with K even and are asserted absent instead:
      * a cycle of EVEN length stored reversed: its edge starts with the cycle's smallest canonical k-mer m as m itself, its reverse
        complement with rc(last k-mer) >= canonical(last k-mer) > m, so the edge is smaller than its reverse complement and stays
        as walked (k_graph_walk_write's `rev = lt128(rc(last), first)` is false for every cycle);
      * a cycle of odd length whose middle base lies in the last k-mer and not in the first: L = n + K - 1 odd makes n even, then
        mid = (n + K - 2) / 2 >= n - 1 says n <= K, which is also what mid < K says (the kernel's `mid >= n - 1` arm is never
        reached for a cycle; n = K + 1 has even length).  The middle base of the cycles of n <= K lies in both."""
    from tests import zoo_synth
    from tests.test_bads_oracle import TABLE, fixture_expected
    case = f"graph_zoo_k{K}"
    g = graph_oracle.run(np.load(os.path.join(golden_dir, f"expect_zoo_k{K}.npz"))["solid_post"], K)
    c = zoo_synth.graph_classes(g, K)
    cyc = c["cycles"]
    assert any(n == 1 for n, _, _ in cyc)                                        # poly-A: a cycle of one k-mer
    assert {o for n, o, w in cyc if w is not None and n > 1} == {"fwd", "rev"}   # odd length: both stored orientations
    assert {o for n, o, w in cyc if w is None and n > 1} == {"fwd"}              # even length: as walked, always (see above)
    assert sum(1 for n, o, w in cyc if w is None and n > 1) >= 10
    # the middle base of an odd length: inside the first k-mer (and then the last), or reached by the pre-walk; each stored both ways
    assert {(o, w) for n, o, w in cyc if w is not None} == {("fwd", "firstlast"), ("rev", "firstlast"), ("fwd", "between"), ("rev", "between")}
    assert all((w == "firstlast") == (n <= K) for n, _, w in cyc if w is not None)
    assert {n for n, _, _ in cyc} >= set(zoo_synth.CIRCLES)                      # every circle is there as one edge
    assert {1, 2, 3, 4, zoo_synth.TANDEM_UNIT} <= set(c["loops"])                # loops on a vertex that other edges touch
    assert c["palindromes"] >= 2 and c["n_edges"] > 870
    assert {1, 2} <= c["ordinary"]                                               # walkers that meet at once; an odd length whose middle lies in the first k-mer
    paths, reads, quals, edges, sums = fixture_expected(golden_dir, case, K, "zoo")
    assert zoo_synth.most_repeats(paths) >= 10
    assert ((sums > 0) & (sums < 150)).any() and (sums == 150).any() and ((sums > 150) & (sums <= 200)).any()
    # the fixture is the committed generator's, and every error-free read of it is placed
    want, _, _, clean, _ = zoo_synth.zoo_members(zoo_synth.ZOO_SEED)
    assert [bytes(r) for r in reads] == [bytes(r) for r in want]
    assert all(p for (_, p), ok in zip(paths, clean) if ok)
