"""Degenerate topology on the GPU at K = 40, 48 and 60: the zoo of tests/zoo_synth.py -- branch-free circles from one k-mer to a
thousand (k_graph_cycles and the cycle arm of k_graph_walk_write: every way the stored orientation is found, both results), pure
tandem repeats, palindromic k-mers, loop edges on a branching vertex, reads that name one edge dozens of times -- from the count to
a.dup, byte for byte against (a) the files the reference's own classes wrote from it (tests/golden/graph_zoo_k*: what they hold is
asserted by tests/test_graph_oracle.py::test_zoo_has_the_classes) and (b) the Python oracles on other seeds and on a low-complexity
genome.  MarkBads' sums are compared by tests/test_gpu_bads.py and the verifier's counters and the digests, under three geometries,
by tests/test_gpu_verify.py: both take the zoo from their tables."""
import os
import subprocess

import numpy as np
import pytest

from tests import bads_oracle, hops_cases, zoo_synth
from tests.test_bads_oracle import fixture_expected
from tests.test_graph_oracle import FILES
from tests.test_gpu_paths import explain
from tests.test_hops_oracle import ZOO_TABLE, fixture_hops, fixture_inputs
from tests.test_paths_oracle import decode_paths, load_reads

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DF = os.path.join(ROOT, "superplus_amd", "DF")
ARRAYS = ("packed", "base_off", "read_len", "pq_bytes", "pq_off")
KS = (40, 48, 60)
TWELVE = FILES + ("a.paths", "a.paths.inv", "a.countsb", "a.dup")
# one part; several parts, tiny items, the reads kept; room for two parts a read (a read round a short cycle has dozens: its batch is
# done again with all of it) and no filter in front of the index, a.paths streamed; the paths index built forty entries at a time
# (one read stands dozens of times in one edge's list)
GEOMETRIES = {"default": dict(), "passes": dict(passes=3, inst_per_item=1500, keep_inputs=True), "slots": dict(slots=2), "ranges": dict(ranges="40")}


def rd(path):
    with open(path, "rb") as f:
        return f.read()


def all_files(d, rs, out, sink=False, kept=False):
    """graph_build -> graph_write -> paths_build -> paths_write -> paths_index_dups_write into `out`;
    -> (the twelve files, the stats of the graph and of the paths, paths() decoded, the pairs marked duplicate)"""
    os.makedirs(out, exist_ok=True)
    gst = d.graph_build()
    d.graph_write(out)
    if sink: d.paths_sink(os.path.join(out, "a.paths"))
    st = d.paths_build() if kept else d.paths_build(*(rs[k] for k in ARRAYS))
    d.paths_write(os.path.join(out, "a.paths"))
    off, first, edges = d.paths()
    decoded = [(int(o), [int(e) for e in edges[int(a):int(b)]]) for o, a, b in zip(off, first[:-1], first[1:])]
    marked = d.paths_index_dups_write(out, os.path.join(out, "a.dup"))
    return {f: rd(os.path.join(out, f)) for f in TWELVE}, gst, st, decoded, marked


# ---- 1. the fixture: every file the reference's classes wrote
@pytest.mark.parametrize("geometry", list(GEOMETRIES))
@pytest.mark.parametrize("K", KS)
def test_every_file_matches_the_reference_fixture(golden_dir, tmp_path, monkeypatch, K, geometry):
    from superplus_amd.dfk import Dfk
    rs = load_reads(golden_dir, "zoo")
    extra = dict(GEOMETRIES[geometry])
    sink = False
    if extra.pop("slots", None):
        monkeypatch.setenv("DFK_PATH_SLOTS", "2"); monkeypatch.setenv("DFK_NO_FILTER", "1"); sink = True
    if extra.get("ranges"): monkeypatch.setenv("DFK_PIDX_RANGE_PAIRS", extra.pop("ranges"))
    d = Dfk(K=K, min_bc=2, **extra)
    d.count(*(rs[k] for k in ARRAYS), rs["bc"])
    got, gst, st, decoded, marked = all_files(d, rs, os.path.join(tmp_path, "a"), sink=sink, kept=bool(extra.get("keep_inputs")))
    d.close()
    fix = os.path.join(golden_dir, f"graph_zoo_k{K}")
    exp = {f: rd(os.path.join(fix, f)) for f in TWELVE}
    for f in TWELVE:
        assert got[f] == exp[f], f"{f} K={K} {geometry}" + (": " + explain(got[f], exp[f]) if f == "a.paths" else "")
    want = decode_paths(exp["a.paths"])
    assert decoded == want
    assert gst["n_edges"] == int.from_bytes(exp["a.kmers"][8:16], "little")
    assert (st["n_reads"], st["n_placed"], st["n_path_edges"]) == (len(want), sum(1 for _, p in want if p), sum(len(p) for _, p in want))
    assert marked == int(np.frombuffer(exp["a.dup"], np.uint8, offset=16).sum())


# ---- 2. FindEdgePairs on the zoo (MarkBads' sums with it: the pairs ask for the marks)
@pytest.mark.parametrize("row", ZOO_TABLE, ids=[r[0] for r in ZOO_TABLE])
def test_hops_and_bads_match_the_oracles(golden_dir, tmp_path, monkeypatch, row):
    from tests.test_gpu_bads import saturated
    from tests.test_gpu_hops import built, check
    from superplus_amd.dfk import Dfk
    case, K, which = row[:3]
    want = fixture_hops(golden_dir, case, K, which)
    assert (len(want["m1"]), len(want["m2"]), len(want["m3"]), len(want["pairs"])) == row[5] and want["pairs"]
    _, _, _, _, sums = fixture_expected(golden_dir, case, K, which)
    rs = load_reads(golden_dir, which)
    monkeypatch.setenv("DFK_PATH_SLOTS", "2"); monkeypatch.setenv("DFK_NO_FILTER", "1")          # (batches done again: the sums of a batch too)
    d = Dfk(K=K, mark_bads=True, min_bc=2)
    d.count(*(rs[k] for k in ARRAYS), rs["bc"])
    d.graph_build()
    d.paths_build(*(rs[k] for k in ARRAYS))
    got_sums = d.bads_sums()
    assert np.array_equal(got_sums, saturated(sums))
    assert d.bads_write(None) == (int(bads_oracle.bad_marks(sums).sum()), bads_oracle.bad_digest(sums))
    got = built(d, fixture_inputs(golden_dir, case, K, which)["bc"], tmp_path)
    d.close()
    check(got, want, case)
    # a read round a short cycle makes the members of an X longer, and the searches wider, than the default capacities hold: those
    # edges are the host's, and the oracle's own sizes say how many they are (dfk_hops_build: 96 sequences of 24 edges)
    host = hops_cases.overflows(want, 96, 24)
    assert 0 < host < want["searched"] and got[2]["host_edges"] == host


# ---- 3. other seeds and a low-complexity genome against the oracle chain
_inputs, _expected = {}, {}
SEEDED = [("zoo", 7), ("zoo", 31), ("low-complexity", 71)]


def seeded_input(kind, seed):
    """the zoo of another seed (a short diploid stretch: no reference run needs its 870 edges), or 4000 pairs of a 12 kb genome with
    units of 1-6 bases planted over 15 % of it; made once and handed out unchanged"""
    if (kind, seed) not in _inputs:
        if kind == "zoo":
            rs = zoo_synth.read_set(*zoo_synth.make_zoo(seed, diploid=3000, diploid_pairs=1200))
        else:
            from superplus_amd import synth
            rs = synth.make_reads(synth.make_genome(12000, seed, low_complexity_frac=0.15), 4000, seed + 1).numpy()
        _inputs[(kind, seed)] = rs
    return _inputs[(kind, seed)]


@pytest.mark.parametrize("kind,seed", SEEDED, ids=[f"{k}-{s}" for k, s in SEEDED])
@pytest.mark.parametrize("K", KS)
def test_seeded_inputs_match_the_oracle_chain(oracle, tmp_path, K, kind, seed):
    """reads -> C oracle dictionary -> graph oracle -> paths oracle -> index and duplicates, against the product's files"""
    from oracle import graph_oracle, paths_oracle
    from superplus_amd.dfk import Dfk
    rs = seeded_input(kind, seed)
    ref = oracle.run(*(rs[k] for k in ARRAYS), rs["bc"], K=K)
    g = graph_oracle.run(ref["solid"], K)
    reads, quals = paths_oracle.unpack_reads(rs)
    r = paths_oracle.run(reads, quals, g, K)
    exp = {f: g["files"][f] for f in FILES}
    exp["a.paths"] = r["file"]
    exp.update(paths_oracle.paths_index(r["paths"], g["hbv"].involution()))
    exp["a.dup"] = paths_oracle.mark_dups(r["paths"], reads, quals)
    assert set(exp) == set(TWELVE)
    # the oracle's side holds what the input is here for: loop edges, and reads that name an edge again and again
    left, right = g["hbv"].to_left_right()
    c = zoo_synth.graph_classes(g, K)
    assert sum(1 for a, b in zip(left, right) if a == b) >= 2 and c["loops"] and (kind != "zoo" or len(c["cycles"]) >= 20)
    assert zoo_synth.most_repeats(r["paths"]) >= 10 and sum(1 for _, p in r["paths"] if len(p) and max(np.bincount(p)) > 1) >= 100
    d = Dfk(K=K, keep_inputs=True)
    d.count(*(rs[k] for k in ARRAYS), rs["bc"])
    got, gst, st, decoded, _ = all_files(d, rs, os.path.join(tmp_path, "a"), kept=True)
    # every k-mer carries its place on an edge: (edge id, offset) as KDef::set leaves them
    s = d.solid()
    d.close()
    for f in TWELVE:
        assert got[f] == exp[f], f"{f} K={K} {kind} {seed}" + (": " + explain(got[f], exp[f]) if f == "a.paths" else "")
    assert decoded == [(o, list(p)) for o, p in r["paths"]]
    assert (s["edge_id"] != 0xFFFFFFFF).all() and gst["n_canonical_edges"] == len(np.unique(s["edge_id"])) == len(g["edges"])
    per_edge = {}
    for km, e, cc in zip(graph_oracle._kmer_ints(s, K), s["edge_id"], s["count_ctx"]):
        per_edge.setdefault(int(e), []).append((int(cc) & 0xFFFFFF, g["place"][km]))
    for e, lst in per_edge.items():
        assert len({p[0] for _, p in lst}) == 1 and all(off == p[1] for off, p in lst), e     # the same grouping into edges, the same offsets


# ---- 4. DF on the fixture's reads
@pytest.mark.parametrize("mode", ["one", "loopback2"])
def test_df_writes_the_fixtures_files(tmp_path, golden_dir, mode):
    """`DF BADS=True HOPS=True` on one GPU, and `DF BADS=True` on two ranks over the loopback transport (FindEdgePairs runs on one GPU
    only): every a.* file under a.48 is the fixture's, or the oracle's where the reference's recipe writes none"""
    case, K, which = ZOO_TABLE[1][:3]
    assert K == 48
    _, _, _, _, sums = fixture_expected(golden_dir, case, K, which)
    known = {f: rd(os.path.join(golden_dir, case, f)) for f in TWELVE}
    known["a.bad"] = bads_oracle.bad_file(sums)
    env = dict(os.environ)
    if mode == "one":
        args = ["HOPS=True"]
        known["a.hops"] = fixture_hops(golden_dir, case, K, which, one_good=True)["file"]      # (ONE_GOOD is True unless said otherwise)
    else:
        args = ["NUM_GPUS=2"]; env["DF_TRANSPORT"] = "loopback"; env["DFK_A2A_PIECE_BYTES"] = "4096"
    r = subprocess.run([DF, f"ROOT={tmp_path}", f"LR={golden_dir}/{which}.fastb", "PIPELINE=cs", "ALIGN=False", "NUM_THREADS=8", "HBM_GB=8", "BADS=True", *args],
                       capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    w = f"{tmp_path}/GapToy/1/a.48"
    wrote = sorted(f for f in os.listdir(w) if f.startswith("a."))
    assert wrote == sorted(known), wrote
    for f in wrote:
        assert rd(f"{w}/{f}") == known[f], f
