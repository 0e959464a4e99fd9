"""The gap closers' read sets per edge on the GPU (dfk_closer_build / _write: the marks and ce, the weights per rank, then a range of ranks at a
time one sweep of the batches, the stable sorts and the compactions) against tests/closer_oracle.py: ce, the three tables, the four files
a.close.* byte for byte, the counters and the digests on every fixture; the same bytes under other batch geometries and ranges; seeded
arrays through dfk_closer_build_arrays; the edges of the contract; `DF HOPS=True CLOSER=True`.  Everything is exact.

The rule is pinned by the two restatements only (tests/closer_oracle.py, superplus_amd/csrc/dfk_closer.h); the paths the device works on
are those the existing tests pin on the reference-written a.paths, and the duplicate marks handed in are the reference-written a.dup's on
frag and pathy2."""
import os

import numpy as np
import pytest

from tests import closer_cases, closer_oracle
from tests.test_gpu_hops import ARRAYS, BOTH, FIXTURES, GEOMETRIES, pathed, run_df
from tests.test_gpu_paths import KW
from tests.test_hops_oracle import fixture_inputs as hops_inputs
from tests.test_paths_oracle import load_reads

pytestmark = pytest.mark.gpu

FILES = closer_oracle.FILES
COUNTERS = ("prec", "mates_in", "mates_out", "dup_skipped")


def files_in(d):
    return {f: open(os.path.join(d, f), "rb").read() for f in FILES}


def written(d, tmp_path, sub="out"):
    """dfk_closer_write into a directory of its own -> {name: bytes}, holding no more of the device than before"""
    out = os.path.join(tmp_path, sub)
    os.makedirs(out, exist_ok=True)
    held = d.stats()["hbm_held"]
    d.closer_write(out)
    assert d.stats()["hbm_held"] == held
    assert sorted(os.listdir(out)) == sorted(FILES)
    return files_in(out)


def check(st, got, files, want, what):
    assert [int(x) for x in got["ce"]] == want["ce"], what
    for key in ("loc_first", "anchor_first", "read_first"):
        assert [int(x) for x in got[key]] == want[key], f"{what}: {key}"
    assert np.array_equal(got["locs"].reshape(-1), closer_oracle.loc_words(want["locs"])), f"{what}: locs"
    assert np.array_equal(got["anchors"].reshape(-1).astype(np.uint32), closer_oracle.anchor_words(want["anchors"])), f"{what}: anchors"
    assert np.array_equal(got["reads"], closer_oracle.read_words(want["reads"])), f"{what}: reads"
    assert (st["edges"], st["locs"], st["anchors"], st["reads"]) == (len(want["ce"]), len(want["locs"]), len(want["anchors"]), len(want["reads"])), what
    assert tuple(st[k] for k in COUNTERS) == tuple(want[k] for k in COUNTERS), f"{what}: {[(k, st[k], want[k]) for k in COUNTERS]}"
    for f, k in zip(FILES, ("edges", "locs", "anchors", "reads")):
        assert (st[k + "_sum"], st[k + "_xor"]) == want["digests"][f], f"{what}: the digest of {f}"
    if files is not None:
        for f in FILES:
            assert files[f] == want["files"][f], f"{what}: {f} differs ({len(files[f])} bytes, {len(want['files'][f])} expected)"


def built(d, tmp_path, dup, pairs=None, sub="out"):
    held = d.stats()["hbm_held"]
    st = d.closer_build(dup, pairs)
    assert d.stats()["hbm_held"] == held
    got = d.closer_fetch()
    files = written(d, tmp_path, sub)
    assert d.closer_stats() == st
    return st, got, files


# ---- 1. every fixture
@pytest.mark.parametrize("case,K,which", FIXTURES, ids=[f[0] for f in FIXTURES])
def test_tables_files_and_counters_match_the_oracle_on_the_fixtures(golden_dir, tmp_path, case, K, which):
    from superplus_amd.dfk import Dfk
    want = closer_oracle.fixture_closer(golden_dir, case, K, which)
    i = closer_oracle.fixture_inputs(golden_dir, case, K, which)
    rs = load_reads(golden_dir, which)
    d = pathed(rs, case, K, tmp_path)
    d.hops_build(hops_inputs(golden_dir, case, K, which)["bc"])
    assert [tuple(int(x) for x in p) for p in d.hops_fetch()] == i["pairs"]
    got = built(d, tmp_path, i["dup"])
    d.close()
    check(*got, want, case)
    assert got[0]["ranges"] == (1 if want["ce"] else 0)
    if case == "graph_hot_k48_minfreq2":                                     # the empty case: four valid files with n = 0
        assert got[2]["a.close.edges"] == b"BINWRITE" + bytes(8) and [len(got[2][f]) for f in FILES[1:]] == [24, 24, 24]
    # the same pairs given explicitly, on a context without DFK_F_MARK_BADS
    ckw = dict(KW[case]); nobc = ckw.pop("nobc", False)
    d = Dfk(K=K, **ckw)
    d.count(*(rs[k] for k in ARRAYS), None if nobc else rs["bc"]); d.graph_build(); d.paths_build(*(rs[k] for k in ARRAYS))
    got2 = built(d, tmp_path, i["dup"], np.asarray(i["pairs"], np.int32).reshape(-1, 2), "explicit")
    d.close()
    check(*got2, want, case + " (pairs given)")
    assert got2[2] == got[2]


# ---- 2. the same bytes however the reads were batched and the ranks were split, before and after the index
VARIANTS = ["batch 1001", "batch 333"] + list(GEOMETRIES) + ["ranges", "after the index"]


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("case,K,which", BOTH, ids=[b[2] for b in BOTH])
def test_same_bytes_under_other_batches_and_ranges(golden_dir, tmp_path, monkeypatch, case, K, which, variant):
    want = closer_oracle.fixture_closer(golden_dir, case, K, which)
    dup = closer_oracle.fixture_inputs(golden_dir, case, K, which)["dup"]
    if variant.startswith("batch"): monkeypatch.setenv("DFK_PATH_BATCH_READS", variant.split()[1])      # odd: mates straddle batches
    if variant == "ranges": monkeypatch.setenv("DFK_PIDX_RANGE_PAIRS", "16000" if which == "pathy2" else "6000")
    d = pathed(load_reads(golden_dir, which), case, K, tmp_path, monkeypatch, variant if variant in GEOMETRIES else None)
    d.hops_build(hops_inputs(golden_dir, case, K, which)["bc"])
    got = built(d, tmp_path, dup, None, "first")
    check(*got, want, f"{case} {variant}")
    if variant == "ranges": assert got[0]["ranges"] >= 4
    else: assert got[0]["ranges"] == 1
    if variant == "after the index":
        d.paths_index_dups_write(str(tmp_path), os.path.join(tmp_path, "a.dup"))
        check(*built(d, tmp_path, dup, None, "second"), want, f"{case} built again after the index")
    d.close()


# ---- 3. seeded arrays
@pytest.fixture(scope="module")
def ctx():
    from superplus_amd.dfk import Dfk
    d = Dfk(K=closer_cases.K)
    yield d
    d.close()


def arrays(ctx, c, per=0, out=None, **change):
    a = dict(c); a.update(change)
    return ctx.closer_build_arrays(a["inv"], a["kmers"], a["paths"], a["offsets"], a["pairs"], a["dup"], per, out)


@pytest.mark.parametrize("name,c", [(n, c) for n, c, _ in closer_cases.seeded()], ids=[n for n, _, _ in closer_cases.seeded()])
def test_seeded_arrays_match_the_oracle(ctx, tmp_path, name, c):
    want = closer_cases.oracle(c)
    N = len(c["paths"])
    # reads_per_batch odd, so that mates straddle batches: 1, 7 and N on the small cases; on the large ones (a batch per read would be
    # thousands of uploads) 1499, device_scan's tile + 1 and N
    for per in (sorted({1, 7, N} - {0}) if N <= 400 else (1499, 2049, N)):
        out = os.path.join(tmp_path, f"per{per}")
        os.makedirs(out)
        held = ctx.stats()["hbm_held"]
        st = arrays(ctx, c, per, out)
        assert ctx.stats()["hbm_held"] == held
        check(st, ctx.closer_fetch(), files_in(out), want, f"{name} reads_per_batch={per}")
        assert sorted(os.listdir(out)) == sorted(FILES)
    # without a directory: the same result, no file; dfk_closer_write then writes the same four
    st = arrays(ctx, c)
    check(st, ctx.closer_fetch(), written(ctx, tmp_path, "later"), want, name)


def test_seeded_arrays_in_small_ranges(ctx, tmp_path, monkeypatch):
    name, c, _ = next(s for s in closer_cases.seeded() if s[0] == "over-256")
    want = closer_cases.oracle(c)
    monkeypatch.setenv("DFK_PIDX_RANGE_PAIRS", str((len(want["locs"]) + want["prec"] + len(want["reads"])) // 6))
    st = arrays(ctx, c, 7 * 31, str(tmp_path))
    check(st, ctx.closer_fetch(), files_in(tmp_path), want, name)
    assert st["ranges"] >= 4


def test_arrays_refusals(ctx, tmp_path):
    from superplus_amd.dfk import DfkError
    name, c, _ = closer_cases.seeded()[0]
    want = closer_cases.oracle(c)
    st = arrays(ctx, c)
    E = len(c["inv"])
    for change in (dict(pairs=[(0, E)]), dict(pairs=[(-1, 0)]), dict(pairs=c["pairs"] + [(E, 0)]),
                   dict(paths=c["paths"][:-1], offsets=c["offsets"][:-1]),                                  # an odd number of reads
                   dict(dup=None)):
        with pytest.raises(DfkError) as e:
            arrays(ctx, c, 0, str(tmp_path), **change)
        assert e.value.code == -1, change                                     # DFK_E_ARG
    assert not os.listdir(tmp_path)
    check(ctx.closer_stats(), ctx.closer_fetch(), None, want, "the earlier result")
    assert ctx.closer_stats() == st


# ---- 4. the contract
def test_state_rules_and_the_edges_of_the_contract(golden_dir, tmp_path):
    import ctypes as C
    from superplus_amd.dfk import Dfk, DfkError, lib
    case, K, which = BOTH[1]
    rs = load_reads(golden_dir, which)
    want = closer_oracle.fixture_closer(golden_dir, case, K, which)
    i = closer_oracle.fixture_inputs(golden_dir, case, K, which)
    pairs, dup = np.asarray(i["pairs"], np.int32).reshape(-1, 2), i["dup"]
    E = len(i["inv"])
    d = Dfk(K=K, mark_bads=True, **KW[case])
    d.count(*(rs[k] for k in ARRAYS), rs["bc"]); d.graph_build()
    for call in (lambda: d.closer_build(dup, pairs), lambda: d.closer_build(dup), lambda: d.closer_stats(), lambda: d.closer_fetch(), lambda: d.closer_write(str(tmp_path))):
        with pytest.raises(DfkError) as e:
            call()
        assert e.value.code == -6                                            # DFK_E_STATE: before dfk_paths_build
    d.paths_build(*(rs[k] for k in ARRAYS))
    with pytest.raises(DfkError, match="dfk_hops_build") as e:
        d.closer_build(dup)                                                  # no hops result to take the pairs from
    assert e.value.code == -6
    with pytest.raises(DfkError, match="dfk_closer_build") as e:
        d.closer_write(str(tmp_path))
    assert e.value.code == -6 and not os.listdir(tmp_path)
    first = built(d, tmp_path, dup, pairs)
    check(*first, want, "pairs given, no hops result")
    # refused: an edge id of E, one of -1, no duplicate marks: DFK_E_ARG, and the earlier result is still fetched whole
    for bad in (E, -1):
        p = pairs.copy(); p[len(p) // 2, 1] = bad
        with pytest.raises(DfkError) as e:
            d.closer_build(dup, p)
        assert e.value.code == -1
        check(d.closer_stats(), d.closer_fetch(), None, want, f"after a refused edge id {bad}")
    with pytest.raises(DfkError) as e:
        d.closer_build(None, pairs)
    assert e.value.code == -1
    check(d.closer_stats(), d.closer_fetch(), None, want, "after a refused call without marks")
    # a fetch buffer too small: the counts are still told
    n = [C.c_uint64() for _ in range(4)]
    small = np.zeros(max(1, len(want["locs"]) - 1) * 2, np.uint64)
    z = C.c_uint64(0)
    rc = lib().dfk_closer_fetch(d._ctx, None, z, C.byref(n[0]), None, small.ctypes.data_as(C.c_void_p), C.c_uint64(len(want["locs"]) - 1), C.byref(n[1]),
                                None, None, z, C.byref(n[2]), None, None, z, C.byref(n[3]))
    assert rc == -1 and [x.value for x in n] == [len(want["ce"]), len(want["locs"]), len(want["anchors"]), len(want["reads"])]
    # a directory that does not exist: an error, no partial files
    gone = os.path.join(tmp_path, "no", "such")
    with pytest.raises(DfkError) as e:
        d.closer_write(gone)
    assert e.value.code == -1 and not os.path.exists(os.path.join(tmp_path, "no"))
    # a directory in which one of the names cannot be made: the files opened before it are taken away again
    part = os.path.join(tmp_path, "part")
    os.makedirs(os.path.join(part, "a.close.anchors"))
    with pytest.raises(DfkError):
        d.closer_write(part)
    assert os.listdir(part) == ["a.close.anchors"]
    # from the context's own pairs, before and after the index, the duplicate marks and a.bad
    d.hops_build(hops_inputs(golden_dir, case, K, which)["bc"])
    check(*built(d, tmp_path, dup, None, "own"), want, "the context's own pairs")
    d.paths_index_dups_write(str(tmp_path), os.path.join(tmp_path, "a.dup"))
    d.bads_write(os.path.join(tmp_path, "a.bad"))
    assert np.array_equal(np.frombuffer(open(os.path.join(tmp_path, "a.dup"), "rb").read(), np.uint8, offset=16), dup)
    check(*built(d, tmp_path, dup, None, "after"), want, "after the index")
    # the graph built again: the paths and their sets are gone
    d.graph_build()
    with pytest.raises(DfkError) as e:
        d.closer_fetch()
    assert e.value.code == -6
    d.close()


# ---- 5. DF
def closer_lines(out):
    return [l for l in out.splitlines() if l.startswith("DF_CLOSER ")]


@pytest.mark.parametrize("case,K,which", BOTH, ids=[b[2] for b in BOTH])
def test_df_writes_the_closer_files(tmp_path, golden_dir, case, K, which):
    want = closer_oracle.fixture_closer(golden_dir, case, K, which)      # ONE_GOOD off, as the table was made
    r = run_df(tmp_path, golden_dir, which, "HOPS=True", "ONE_GOOD=False", "CLOSER=True")
    assert r.returncode == 0, r.stdout + r.stderr
    w = f"{tmp_path}/GapToy/1/a.48"
    for f in FILES:
        assert open(f"{w}/{f}", "rb").read() == want["files"][f], f
    for f in sorted(os.listdir(f"{golden_dir}/{case}")):                     # everything else DF writes there is still the fixture's
        if f.startswith("a."):
            assert open(f"{w}/{f}", "rb").read() == open(f"{golden_dir}/{case}/{f}", "rb").read(), f
    dg = want["digests"]
    assert closer_lines(r.stdout) == ['DF_CLOSER {"edges": %d, "locs": %d, "anchors": %d, "reads": %d, "ranges": 1, "a.close.edges": "%016x%016x", "a.close.locs": "%016x%016x", '
                                      '"a.close.anchors": "%016x%016x", "a.close.reads": "%016x%016x"}'
                                      % (len(want["ce"]), len(want["locs"]), len(want["anchors"]), len(want["reads"]), *dg["a.close.edges"], *dg["a.close.locs"],
                                         *dg["a.close.anchors"], *dg["a.close.reads"])], closer_lines(r.stdout)
    assert r.stdout.index("DF_HOPS ") < r.stdout.index("DF_CLOSER ") and not [f for f in os.listdir(w) if f.startswith("a.sub")]


def test_df_with_subset_and_closer_writes_both_in_order(tmp_path, golden_dir):
    r = run_df(tmp_path, golden_dir, "frag", "HOPS=True", "ONE_GOOD=False", "SUBSET=True", "CLOSER=True")
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.index("DF_HOPS ") < r.stdout.index("DF_SUBSET ") < r.stdout.index("DF_CLOSER ")
    w = f"{tmp_path}/GapToy/1/a.48"
    want = closer_oracle.fixture_closer(golden_dir, "graph_frag_k48", 48, "frag")
    assert all(open(f"{w}/{f}", "rb").read() == want["files"][f] for f in FILES) and len([f for f in os.listdir(w) if f.startswith("a.sub")]) == 4


def test_df_refuses_closer_without_hops(tmp_path, golden_dir):
    r = run_df(tmp_path, golden_dir, "frag", "CLOSER=True")
    assert r.returncode != 0 and "CLOSER=True needs HOPS=True" in r.stdout
    assert not os.path.exists(f"{tmp_path}/GapToy")
    r = run_df(tmp_path, golden_dir, "frag", "CLOSER=True", "HOPS=True", "PATHS=False")
    assert r.returncode != 0 and "CLOSER=True needs HOPS=True and PATHS=True" in r.stdout
    assert not os.path.exists(f"{tmp_path}/GapToy")


def test_df_refuses_closer_on_a_sharded_run(tmp_path, golden_dir):
    env = dict(os.environ)
    env["DF_FORCE_SHARDED"] = "1"
    r = run_df(tmp_path, golden_dir, "frag", "HOPS=True", "CLOSER=True", env=env)
    assert r.returncode != 0 and "runs on one GPU only" in r.stdout
    assert not os.path.exists(f"{tmp_path}/GapToy")


def test_df_without_the_switch_writes_and_prints_nothing_of_it(tmp_path, golden_dir):
    r = run_df(tmp_path, golden_dir, "frag", "HOPS=True", "SUBSET=True")
    assert r.returncode == 0, r.stdout + r.stderr
    w = f"{tmp_path}/GapToy/1/a.48"
    # the file list of a run without CLOSER: the fixture's files, a.hops and the four a.sub.*
    golden = {f for f in os.listdir(f"{golden_dir}/graph_frag_k48") if f.startswith("a.")}
    assert {f for f in os.listdir(w) if f.startswith("a.")} - golden <= {"a.hops", "a.sub.ids", "a.sub.eoi", "a.sub.paths", "a.sub.paths.inv", "a.bad"}
    assert not [f for f in os.listdir(w) if f.startswith("a.close")]
    assert not closer_lines(r.stdout) and "DF_CLOSER" not in r.stdout and "closer" not in r.stdout.lower()
