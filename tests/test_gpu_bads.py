"""MarkBads on the GPU (DFK_F_MARK_BADS: dfk_paths_build gathers the per-read sums with k_bad_sums while a batch's reads,
qualities, edges and paths are on the device; dfk_bads_write folds them to a.bad) against tests/bads_oracle.py -- per read, so
that a single wrong position shows -- on the fixtures, on seeded sets with the threshold in play and reads longer than a PQVec
block, at the edges of the contract, and through `DF BADS=True` on one GPU and sharded."""
import os
import subprocess

import numpy as np
import pytest

from tests import bads_oracle, util
from tests.test_bads_oracle import TABLE, fixture_expected
from tests.test_gpu_paths import KW
from tests.test_paths_oracle import load_reads

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DF = os.path.join(ROOT, "superplus_amd", "DF")
ARRAYS = ("packed", "base_off", "read_len", "pq_bytes", "pq_off")

# the geometries of test_paths_file_matches_reference_fixture
GEOMETRIES = {"default": dict(), "passes": dict(passes=3, inst_per_item=1500, keep_inputs=True), "slots": dict(slots=2), "sink": dict(sink=True)}


def saturated(sums):
    return np.minimum(np.asarray(sums, np.int64), bads_oracle.SATURATED).astype(np.uint16)


def describe(got, want):
    bad = np.nonzero(got != want)[0]
    return f"{len(bad)} of {len(want)} reads differ, first {bad[:5].tolist()}: got {got[bad[:5]].tolist()} want {want[bad[:5]].tolist()}"


def run_bads(rs, K, tmp_path, bc=None, build="host", sink=False, **kw):
    """count -> graph_build -> paths_build with mark_bads=True -> (sums, bytes of a.bad, marked, digest)"""
    from superplus_amd.dfk import Dfk
    d = Dfk(K=K, mark_bads=True, **kw)
    d.count(*(rs[k] for k in ARRAYS), bc)
    d.graph_build()
    if sink: d.paths_sink(os.path.join(tmp_path, "a.paths"))
    if build == "kept": d.paths_build()
    elif build == "device":
        import torch
        dev = torch.device("cuda:0")
        t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a).view(dt) if dt is not None else np.ascontiguousarray(a)).to(dev)
        pad = torch.zeros(8, dtype=torch.uint8, device=dev)                  # (the streams are read as aligned words)
        d.paths_build_device(torch.cat([t(rs["packed"], None), pad]), t(rs["base_off"], np.int64), t(rs["read_len"].astype(np.uint32), np.int32),
                             torch.cat([t(rs["pq_bytes"], None), pad]), t(rs["pq_off"], np.int64))
    else: d.paths_build(*(rs[k] for k in ARRAYS))
    if sink: d.paths_write(os.path.join(tmp_path, "a.paths"))
    sums = d.bads_sums()
    out = os.path.join(tmp_path, "a.bad")
    marked, digest = d.bads_write(out)
    assert d.bads_write(None) == (marked, digest)                            # everything but the file
    d.close()
    return sums, open(out, "rb").read(), marked, digest


def check(got, expected_sums, what):
    sums, file, marked, digest = got
    want = saturated(expected_sums)
    assert (want > 0).any(), f"{what}: the expected side is empty"
    assert sums.dtype == np.uint16 and len(sums) == len(want) and np.array_equal(sums, want), f"{what}: " + describe(sums, want)
    assert file == bads_oracle.bad_file(expected_sums), what
    assert marked == int(bads_oracle.bad_marks(expected_sums).sum()), what
    assert digest == bads_oracle.bad_digest(expected_sums), what


# ---- 1. the fixtures: paths and edges written by the reference's classes
@pytest.mark.parametrize("case,K,which,geometry", [(r[0], r[1], r[2], g) for r in TABLE for g in (GEOMETRIES if r[2] in ("pathy2", "frag") else ["default"])])
def test_sums_and_file_match_the_restatement_on_the_fixtures(golden_dir, tmp_path, monkeypatch, case, K, which, geometry):
    row = next(r for r in TABLE if r[0] == case)
    _, _, _, _, exp = fixture_expected(golden_dir, case, K, which)
    rs = load_reads(golden_dir, which)
    kw = dict(KW[case]); nobc = kw.pop("nobc", False)
    extra = dict(GEOMETRIES[geometry]); sink = extra.pop("sink", False)
    if extra.pop("slots", None):                                             # room for two parts a read: batches done again with all of it
        monkeypatch.setenv("DFK_PATH_SLOTS", "2"); monkeypatch.setenv("DFK_NO_FILTER", "1"); sink = True
    got = run_bads(rs, K, tmp_path, bc=None if nobc else rs["bc"], build="kept" if extra.get("keep_inputs") else "host", sink=sink, **kw, **extra)
    check(got, exp, f"{case} {geometry}")
    assert got[2] == row[6]                                                  # the marked pairs of the table
    if sink:                                                                 # ... and the paths are still the fixture's
        assert open(os.path.join(tmp_path, "a.paths"), "rb").read() == open(os.path.join(golden_dir, case, "a.paths"), "rb").read()


# ---- shared seeded sets: built and pathed by the oracles once, handed out unchanged
_sets = {}


def rebuild(rs, reads, quals):
    """the ABI's arrays from lists of base codes and qualities, as test_paths_edge_cases rebuilds its own"""
    from superplus_amd import feudal
    packed = np.concatenate([feudal.pack_bases(np.frombuffer(r, np.uint8)[None, :])[0] for r in reads])
    read_len = np.array([len(r) for r in reads], np.uint32)
    base_off = np.concatenate([[0], np.cumsum((read_len.astype(np.uint64) + 3) // 4)]).astype(np.uint64)
    pqs = [np.frombuffer(feudal.pq_encode(np.asarray(q, np.uint8)), np.uint8) for q in quals]
    pq_bytes = np.concatenate(pqs); pq_off = np.concatenate([[0], np.cumsum([len(x) for x in pqs])]).astype(np.uint64)
    return dict(packed=packed, base_off=base_off, read_len=read_len, pq_bytes=pq_bytes, pq_off=pq_off, bc=rs["bc"], n_reads=len(reads))


def expected_of(oracle, rs, reads, quals, K=48):
    from oracle import graph_oracle, paths_oracle
    ref = oracle.run(*(rs[k] for k in ARRAYS), rs["bc"], K=K)
    g = graph_oracle.run(ref["solid"], K)
    paths = paths_oracle.run(reads, quals, g, K)["paths"]
    edges = [bytes(e) for e in g["hbv"].edges]
    sums = bads_oracle.bad_sums(paths, reads, quals, edges, K)
    sums.setflags(write=False)
    return dict(rs=rs, reads=reads, quals=quals, paths=paths, edges=edges, sums=sums)


def seeded_set(oracle):
    """util.make_set(511, 40000, 6000) with one to eight substitutions on every third read"""
    if "seeded" not in _sets:
        from oracle import paths_oracle
        rs = util.make_set(511, 40000, 6000)
        reads, quals = paths_oracle.unpack_reads(rs)
        rng = np.random.default_rng(511)
        reads = [bytearray(r) for r in reads]
        for i in range(0, len(reads), 3):
            k = int(rng.integers(1, 9))
            pos = rng.integers(0, len(reads[i]), k)
            for p, by in zip(pos, rng.integers(1, 4, k)):                    # (another base: + 1..3 mod 4)
                reads[i][p] = (reads[i][p] + int(by)) & 3
        reads = [bytes(r) for r in reads]
        _sets["seeded"] = expected_of(oracle, rebuild(rs, reads, quals), reads, quals)
    return _sets["seeded"]


def long_set(oracle):
    """util.make_long_set(521, 30000, 1500, err=0.02): 300 bases a read, mixed blocks, Q2 tails"""
    if "long" not in _sets:
        from oracle import paths_oracle
        rs = util.make_long_set(521, 30000, 1500, err=0.02)
        reads, quals = paths_oracle.unpack_reads(rs)
        _sets["long"] = expected_of(oracle, rs, reads, quals)
    return _sets["long"]


# ---- 2. a seeded set with the threshold in play
@pytest.mark.parametrize("build", ["host", "device"])
def test_seeded_set_with_sums_on_both_sides_of_the_threshold(oracle, tmp_path, build):
    s = seeded_set(oracle)
    exp = s["sums"]
    marks = bads_oracle.bad_marks(exp)
    assert 0 < marks.sum() < len(marks)
    assert (exp == 150).any()                                                # exactly at the threshold: not marked
    assert ((exp > 150) & (exp <= 200)).any() and ((exp >= 100) & (exp <= 150)).any()
    # (as the set was checked when the test was written)
    assert (sum(1 for _, p in s["paths"] if p), int(marks.sum()), int((exp == 150).sum()), int(((exp >= 101) & (exp <= 200)).sum())) == (9084, 169, 32, 467)
    check(run_bads(s["rs"], 48, tmp_path, bc=s["rs"]["bc"], build=build), exp, f"seeded set, {build} arrays")


# ---- 3. reads longer than one PQVec block (nQs is a byte): the walk over the block headers
def test_reads_longer_than_one_quality_block(oracle, tmp_path):
    s = long_set(oracle)
    exp = s["sums"]
    far = sum(1 for i, (off, p) in enumerate(s["paths"]) if (bads_oracle.mismatch_positions(p, off, s["reads"][i], s["edges"], 48) >= 255).any())
    assert far > 0                                                           # counted mismatches behind the first block
    assert (exp == 150).any() and 0 < bads_oracle.bad_marks(exp).sum() < len(exp) // 2
    assert (int(bads_oracle.bad_marks(exp).sum()), int((exp == 150).sum()), far) == (1284, 116, 1630)   # (as checked when the test was written)
    check(run_bads(s["rs"], 48, tmp_path, bc=s["rs"]["bc"]), exp, "long reads")


# ---- 4. the edges of the contract
def test_short_and_unplaceable_reads_odd_counts_and_a_second_build(oracle, tmp_path):
    from oracle import paths_oracle
    from superplus_amd.dfk import Dfk, DfkError
    rs0 = util.make_set(431, 40000, 3000)
    reads, quals = paths_oracle.unpack_reads(rs0)
    reads = [bytes(r) for r in reads]
    for i in range(0, len(reads), 97):                                       # shorter than K
        reads[i] = reads[i][:30]; quals[i] = quals[i][:30]
    rng = np.random.default_rng(9)
    for i in range(5, len(reads), 131):                                      # no solid k-mer
        reads[i] = rng.integers(0, 4, len(reads[i]), dtype=np.uint8).tobytes()
    rs = rebuild(rs0, reads, quals)
    e = expected_of(oracle, rs, reads, quals)
    exp = e["sums"]
    assert (exp > 0).any() and all(exp[i] == 0 for i in range(0, len(reads), 97)) and all(exp[i] == 0 for i in range(5, len(reads), 131))
    d = Dfk(K=48, mark_bads=True)
    d.count(*(rs[k] for k in ARRAYS), rs["bc"])
    with pytest.raises(DfkError, match="DFK_F_MARK_BADS"):
        d.bads_sums()                                                        # before a build
    d.graph_build()
    d.paths_build(*(rs[k] for k in ARRAYS))
    sums = d.bads_sums()
    assert np.array_equal(sums, saturated(exp)), describe(sums, saturated(exp))
    assert all(sums[i] == 0 for i in range(0, len(reads), 97)) and all(sums[i] == 0 for i in range(5, len(reads), 131))
    before = os.path.join(tmp_path, "before.bad"); after = os.path.join(tmp_path, "after.bad")
    m0, dg0 = d.bads_write(before)
    d.paths_index_dups_write(str(tmp_path), os.path.join(tmp_path, "a.dup"))  # gives the k-mer index back; the sums stay
    assert d.bads_write(after) == (m0, dg0)
    assert open(after, "rb").read() == open(before, "rb").read() == bads_oracle.bad_file(exp)
    # a second build (after dfk_graph_build) replaces the sums: the pairs in reverse order, then an odd number of reads
    d.graph_build()
    n = len(reads)
    order = np.arange(n).reshape(-1, 2)[::-1].reshape(-1)
    rs2 = rebuild(rs0, [reads[i] for i in order], [quals[i] for i in order])
    d.paths_build(*(rs2[k] for k in ARRAYS))
    sums2 = d.bads_sums()
    assert np.array_equal(sums2, saturated(exp)[order]) and not np.array_equal(sums2, sums)
    assert d.bads_write(None)[0] == m0
    d.graph_build()
    d.paths_build(rs["packed"][: int(rs["base_off"][-2])], rs["base_off"][:-1], rs["read_len"][:-1], rs["pq_bytes"][: int(rs["pq_off"][-2])], rs["pq_off"][:-1])
    assert np.array_equal(d.bads_sums(), saturated(exp)[:-1])                # an odd number of reads: the sums are fine ...
    with pytest.raises(DfkError):
        d.bads_write(os.path.join(tmp_path, "odd.bad"))                      # ... but MarkBads works on pairs
    d.close()


def test_without_the_flag_nothing_is_gathered_or_held(golden_dir, tmp_path):
    from superplus_amd.dfk import Dfk, DfkError
    rs = load_reads(golden_dir, "frag")
    held, files = {}, {}
    for name, kw in (("never", dict()), ("off", dict(mark_bads=False)), ("on", dict(mark_bads=True))):
        d = Dfk(K=48, **kw)
        d.count(*(rs[k] for k in ARRAYS), rs["bc"])
        d.graph_build()
        d.paths_build(*(rs[k] for k in ARRAYS))
        held[name] = d.stats()["hbm_held"]
        out = os.path.join(tmp_path, name + ".paths"); d.paths_write(out)
        files[name] = open(out, "rb").read()
        if name != "on":
            with pytest.raises(DfkError, match="DFK_F_MARK_BADS"):
                d.bads_sums()
            with pytest.raises(DfkError, match="DFK_F_MARK_BADS"):
                d.bads_write(os.path.join(tmp_path, "never.bad"))
            assert not os.path.exists(os.path.join(tmp_path, "never.bad"))
            assert d.stats()["us_bad_sums"] == 0
        else:
            assert (d.bads_sums() > 0).any()
        d.close()
    assert held["never"] == held["off"]
    # with the flag the context holds the sums -- two bytes a read, rounded up by the arena to at most a page -- and nothing else
    n = len(rs["read_len"])
    assert 2 * n <= held["on"] - held["off"] <= 2 * n + 4096
    assert files["never"] == files["off"] == files["on"] == open(os.path.join(golden_dir, "graph_frag_k48", "a.paths"), "rb").read()


# ---- 5. DF BADS=True
def bads_lines(out):
    return [l for l in out.splitlines() if l.startswith("DF_BADS ") or l.endswith("of pairs marked bad")]


@pytest.mark.parametrize("which,case", [("frag", "graph_frag_k48"), ("pathy2", "graph_pathy2_k48")])
@pytest.mark.parametrize("mode", ["one", "rccl1", "loopback2", "loopback4"])
def test_df_writes_a_bad_on_one_gpu_and_sharded(tmp_path, golden_dir, which, case, mode):
    _, _, _, _, exp = fixture_expected(golden_dir, case, 48, which)
    assert (exp > 0).any()
    env = dict(os.environ)
    args = []
    if mode == "rccl1":
        args, env["DF_FORCE_SHARDED"] = ["NUM_GPUS=1"], "1"
    elif mode != "one":
        args, env["DF_TRANSPORT"] = [f"NUM_GPUS={mode[-1]}"], "loopback"
        env["DFK_A2A_PIECE_BYTES"] = "4096"
    r = subprocess.run([DF, f"ROOT={tmp_path}", f"LR={golden_dir}/{which}.fastb", "PIPELINE=cs", "ALIGN=False", "NUM_THREADS=8", "HBM_GB=8", "BADS=True", *args],
                       capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    rd = lambda p: open(p, "rb").read()
    w = f"{tmp_path}/GapToy/1/a.48"
    assert rd(f"{w}/a.bad") == bads_oracle.bad_file(exp)
    for f in sorted(os.listdir(f"{golden_dir}/{case}")):                     # everything else DF writes there is still the fixture's
        if f.startswith("a."):
            assert rd(f"{w}/{f}") == rd(f"{golden_dir}/{case}/{f}"), f
    marks = bads_oracle.bad_marks(exp); dg = bads_oracle.bad_digest(exp)
    assert bads_lines(r.stdout) == ["%.3f%% of pairs marked bad" % (100.0 * marks.sum() / len(marks)),
                                    'DF_BADS {"a.bad": "%016x%016x", "bad_pairs": %d}' % (dg[0], dg[1], marks.sum())], bads_lines(r.stdout)
    assert len([l for l in r.stdout.splitlines() if l.startswith("DF_DIGESTS ")]) == 1


def test_df_without_bads_writes_and_prints_what_it_did(tmp_path, golden_dir):
    r = subprocess.run([DF, f"ROOT={tmp_path}", f"LR={golden_dir}/frag.fastb", "PIPELINE=cs", "ALIGN=False", "NUM_THREADS=8", "HBM_GB=8"],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    assert not os.path.exists(f"{tmp_path}/GapToy/1/a.48/a.bad") and os.path.exists(f"{tmp_path}/GapToy/1/a.48/a.dup")
    assert not bads_lines(r.stdout) and "DF_BADS" not in r.stdout and "marked bad" not in r.stdout
