"""The patching stage's subset of interest on the GPU (dfk_subset_build / _write: the marks and eoi, the hit sweep folded per pair, the ids and
paths gather a batch at a time, the index subset a range of ranks at a time) against tests/subset_oracle.py: ids, eoi, the four files
a.sub.*, the counters and the digests on every fixture; the same bytes under other batch geometries and index ranges; seeded arrays through
dfk_subset_build_arrays; the edges of the contract; `DF HOPS=True SUBSET=True`.

On the fixtures the expected a.sub.paths is sliced from the reference-written a.paths, and on frag and pathy2 the expected a.sub.paths.inv
from the reference-written a.paths.inv; which ids and edges are taken is pinned by the restatements only (tests/subset_oracle.py)."""
import os
import subprocess

import numpy as np
import pytest

from tests import subset_cases, subset_oracle
from tests.test_gpu_hops import ARRAYS, BOTH, DF, FIXTURES, GEOMETRIES, pathed, run_df
from tests.test_gpu_paths import KW
from tests.test_hops_oracle import fixture_inputs
from tests.test_paths_oracle import load_reads

pytestmark = pytest.mark.gpu

FILES = subset_oracle.FILES


def files_in(d):
    return {f: open(os.path.join(d, f), "rb").read() for f in FILES}


def written(d, tmp_path, sub="out"):
    """dfk_subset_write into a directory of its own -> {name: bytes}, holding no more of the device than before"""
    out = os.path.join(tmp_path, sub)
    os.makedirs(out, exist_ok=True)
    held = d.stats()["hbm_held"]
    d.subset_write(out)
    assert d.stats()["hbm_held"] == held
    assert sorted(os.listdir(out)) == sorted(FILES)
    return files_in(out)


def check(st, ids, eoi, files, want, what):
    assert [int(x) for x in eoi] == want["eoi"], what
    missing, extra = sorted(set(want["ids"]) - set(int(x) for x in ids)), sorted(set(int(x) for x in ids) - set(want["ids"]))
    assert [int(x) for x in ids] == want["ids"], f"{what}: {len(missing)} ids missing (first {missing[:5]}), {len(extra)} too many (first {extra[:5]})"
    assert (st["eoi"], st["ids"], st["path_entries"], st["index_entries"], st["one_read_only"]) == \
           (len(want["eoi"]), len(want["ids"]), want["path_entries"], want["index_entries"], want["one_read_only"]), what
    assert (st["ids_sum"], st["ids_xor"]) == want["ids_digest"] and (st["eoi_sum"], st["eoi_xor"]) == want["eoi_digest"], what
    if files is not None:
        for f in FILES:
            assert files[f] == want["files"][f], f"{what}: {f} differs ({len(files[f])} bytes, {len(want['files'][f])} expected)"


def built(d, tmp_path, pairs=None, sub="out"):
    held = d.stats()["hbm_held"]
    st = d.subset_build(pairs)
    assert d.stats()["hbm_held"] == held
    ids, eoi = d.subset_fetch()
    files = written(d, tmp_path, sub)
    st2 = d.subset_stats()
    assert all(st2[k] == st[k] for k in st if not k.startswith("us") and k != "ranges")
    return st2, ids, eoi, files


# ---- 1. every fixture
@pytest.mark.parametrize("case,K,which", FIXTURES, ids=[f[0] for f in FIXTURES])
def test_ids_eoi_files_and_counters_match_the_oracle_on_the_fixtures(golden_dir, tmp_path, case, K, which):
    from superplus_amd.dfk import Dfk
    want = subset_oracle.fixture_subset(golden_dir, case, K, which)
    rs = load_reads(golden_dir, which)
    d = pathed(rs, case, K, tmp_path)
    d.hops_build(fixture_inputs(golden_dir, case, K, which)["bc"])
    assert [tuple(int(x) for x in p) for p in d.hops_fetch()] == want["pairs"]
    got = built(d, tmp_path)
    d.close()
    check(*got, want, case)
    if case == "graph_hot_k48_minfreq2":                                     # the empty case: four valid files with n = 0
        assert got[0]["ids"] == 0 and got[3]["a.sub.ids"] == b"BINWRITE" + bytes(8) and len(got[3]["a.sub.paths"]) == len(got[3]["a.sub.paths.inv"]) == 32
    # the same pairs given explicitly, on a context without DFK_F_MARK_BADS
    ckw = dict(KW[case]); nobc = ckw.pop("nobc", False)
    d = Dfk(K=K, **ckw)
    d.count(*(rs[k] for k in ARRAYS), None if nobc else rs["bc"]); d.graph_build(); d.paths_build(*(rs[k] for k in ARRAYS))
    got2 = built(d, tmp_path, np.asarray(want["pairs"], np.int32).reshape(-1, 2), "explicit")
    d.close()
    check(*got2, want, case + " (pairs given)")
    assert got2[3] == got[3]


# ---- 2. the same bytes however the reads were batched and the index subset was split, before and after the index
VARIANTS = ["batch 1001", "batch 333"] + list(GEOMETRIES) + ["ranges", "after the index"]


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("case,K,which", BOTH, ids=[b[2] for b in BOTH])
def test_same_bytes_under_other_batches_and_ranges(golden_dir, tmp_path, monkeypatch, case, K, which, variant):
    want = subset_oracle.fixture_subset(golden_dir, case, K, which)
    if variant.startswith("batch"): monkeypatch.setenv("DFK_PATH_BATCH_READS", variant.split()[1])      # odd: pairs straddle batches
    if variant == "ranges": monkeypatch.setenv("DFK_PIDX_RANGE_PAIRS", "4000" if which == "pathy2" else "1800")
    d = pathed(load_reads(golden_dir, which), case, K, tmp_path, monkeypatch, variant if variant in GEOMETRIES else None)
    d.hops_build(fixture_inputs(golden_dir, case, K, which)["bc"])
    got = built(d, tmp_path, None, "first")
    check(*got, want, f"{case} {variant}")
    if variant == "ranges": assert got[0]["ranges"] >= 4
    else: assert got[0]["ranges"] == 1
    if variant == "after the index":
        d.paths_index_dups_write(str(tmp_path), os.path.join(tmp_path, "a.dup"))
        check(*built(d, tmp_path, None, "second"), want, f"{case} built again after the index")
    d.close()


# ---- 3. seeded arrays
@pytest.fixture(scope="module")
def ctx():
    from superplus_amd.dfk import Dfk
    d = Dfk(K=48)
    yield d
    d.close()


@pytest.mark.parametrize("name,c", [(n, c) for n, c, _ in subset_cases.seeded()], ids=[n for n, _, _ in subset_cases.seeded()])
def test_seeded_arrays_match_the_oracle(ctx, tmp_path, name, c):
    want = subset_oracle.run(c["paths"], c["inv"], c["pairs"])
    N = len(c["paths"])
    # reads_per_batch 1, 7 and N; the case of 4500 reads (a batch per read would be 4500 uploads) takes 1499 -- odd, so pairs straddle
    # batches --, one scan tile and N
    for per in (sorted({1, 7, N} - {0}) if N <= 400 else (1499, 2048, N)):
        out = os.path.join(tmp_path, f"per{per}")
        os.makedirs(out)
        held = ctx.stats()["hbm_held"]
        st = ctx.subset_build_arrays(c["inv"], c["paths"], c["pairs"], per, out)
        assert ctx.stats()["hbm_held"] == held
        ids, eoi = ctx.subset_fetch()
        check(st, ids, eoi, files_in(out), want, f"{name} reads_per_batch={per}")
        assert sorted(os.listdir(out)) == sorted(FILES)
    # without a directory: the same result, no file; dfk_subset_write has nothing to write from
    from superplus_amd.dfk import DfkError
    st = ctx.subset_build_arrays(c["inv"], c["paths"], c["pairs"], 0, None)
    check(st, *ctx.subset_fetch(), None, want, name)
    with pytest.raises(DfkError) as e:
        ctx.subset_write(str(tmp_path))
    assert e.value.code == -6 and not any(f in os.listdir(tmp_path) for f in FILES)


def test_seeded_arrays_in_small_ranges(ctx, tmp_path, monkeypatch):
    name, c, _ = next(s for s in subset_cases.seeded() if s[0] == "dense")
    want = subset_oracle.run(c["paths"], c["inv"], c["pairs"])
    monkeypatch.setenv("DFK_PIDX_RANGE_PAIRS", str(max(1, want["index_entries"] // 6)))
    st = ctx.subset_build_arrays(c["inv"], c["paths"], c["pairs"], 7, str(tmp_path))
    check(st, *ctx.subset_fetch(), files_in(tmp_path), want, name)
    assert st["ranges"] >= 4


def test_arrays_refusals(ctx, tmp_path):
    from superplus_amd.dfk import DfkError
    name, c, _ = subset_cases.seeded()[0]
    want = subset_oracle.run(c["paths"], c["inv"], c["pairs"])
    st = ctx.subset_build_arrays(c["inv"], c["paths"], c["pairs"])
    E = len(c["inv"])
    for bad in ([(0, E)], [(-1, 0)], c["pairs"] + [(E, 0)]):
        with pytest.raises(DfkError) as e:
            ctx.subset_build_arrays(c["inv"], c["paths"], bad, 0, str(tmp_path))
        assert e.value.code == -1                                              # DFK_E_ARG
    with pytest.raises(DfkError) as e:
        ctx.subset_build_arrays(c["inv"], c["paths"][:-1], c["pairs"])       # an odd number of reads
    assert e.value.code == -1
    assert not os.listdir(tmp_path)
    check(ctx.subset_stats(), *ctx.subset_fetch(), None, want, "the earlier result")
    assert ctx.subset_stats() == st


# ---- 4. the contract
def test_state_rules_and_the_edges_of_the_contract(golden_dir, tmp_path):
    import ctypes as C
    from superplus_amd.dfk import Dfk, DfkError, lib
    case, K, which = BOTH[1]
    rs = load_reads(golden_dir, which)
    want = subset_oracle.fixture_subset(golden_dir, case, K, which)
    pairs = np.asarray(want["pairs"], np.int32).reshape(-1, 2)
    E = len(fixture_inputs(golden_dir, case, K, which)["inv"])
    d = Dfk(K=K, mark_bads=True, **KW[case])
    d.count(*(rs[k] for k in ARRAYS), rs["bc"]); d.graph_build()
    for call in (lambda: d.subset_build(pairs), lambda: d.subset_build(None), lambda: d.subset_stats(), lambda: d.subset_fetch(), lambda: d.subset_write(str(tmp_path))):
        with pytest.raises(DfkError) as e:
            call()
        assert e.value.code == -6                                            # DFK_E_STATE: before dfk_paths_build
    d.paths_build(*(rs[k] for k in ARRAYS))
    with pytest.raises(DfkError, match="dfk_hops_build") as e:
        d.subset_build(None)                                                 # no hops result to take the pairs from
    assert e.value.code == -6
    with pytest.raises(DfkError, match="dfk_subset_build") as e:
        d.subset_write(str(tmp_path))
    assert e.value.code == -6 and not os.listdir(tmp_path)
    first = built(d, tmp_path, pairs)
    check(*first, want, "pairs given, no hops result")
    # refused: an edge id of E, one of -1: DFK_E_ARG, and the earlier result is still fetched whole
    for bad in (E, -1):
        p = pairs.copy(); p[len(p) // 2, 1] = bad
        with pytest.raises(DfkError) as e:
            d.subset_build(p)
        assert e.value.code == -1
        ids, eoi = d.subset_fetch()
        check(d.subset_stats(), ids, eoi, None, want, f"after a refused edge id {bad}")
    # a fetch buffer too small
    n = C.c_uint64(); m = C.c_uint64()
    small = np.zeros(max(1, len(want["ids"]) - 1), np.uint64)
    rc = lib().dfk_subset_fetch(d._ctx, small.ctypes.data_as(C.c_void_p), C.c_uint64(len(want["ids"]) - 1), C.byref(n), None, C.c_uint64(0), C.byref(m))
    assert rc == -1 and (n.value, m.value) == (len(want["ids"]), len(want["eoi"]))
    rc = lib().dfk_subset_fetch(d._ctx, None, C.c_uint64(0), C.byref(n), small.ctypes.data_as(C.c_void_p), C.c_uint64(1), C.byref(m))
    assert rc == -1
    # a directory that does not exist: an error, no partial files
    gone = os.path.join(tmp_path, "no", "such")
    with pytest.raises(DfkError) as e:
        d.subset_write(gone)
    assert e.value.code == -1 and not os.path.exists(os.path.join(tmp_path, "no"))
    # a directory in which one of the names cannot be made: the files opened before it are taken away again
    part = os.path.join(tmp_path, "part")
    os.makedirs(os.path.join(part, "a.sub.paths"))
    with pytest.raises(DfkError):
        d.subset_write(part)
    assert os.listdir(part) == ["a.sub.paths"]
    # from the context's own pairs, before and after the index, the duplicate marks and a.bad
    d.hops_build(fixture_inputs(golden_dir, case, K, which)["bc"])
    check(*built(d, tmp_path, None, "own"), want, "the context's own pairs")
    d.paths_index_dups_write(str(tmp_path), os.path.join(tmp_path, "a.dup"))
    d.bads_write(os.path.join(tmp_path, "a.bad"))
    check(*built(d, tmp_path, None, "after"), want, "after the index")
    # the graph built again: the paths and their subset are gone
    d.graph_build()
    with pytest.raises(DfkError) as e:
        d.subset_fetch()
    assert e.value.code == -6
    d.close()


# ---- 5. DF
def subset_lines(out):
    return [l for l in out.splitlines() if l.startswith("DF_SUBSET ") or l.startswith("subset is size")]


@pytest.mark.parametrize("case,K,which", BOTH, ids=[b[2] for b in BOTH])
def test_df_writes_the_subset(tmp_path, golden_dir, case, K, which):
    want = subset_oracle.fixture_subset(golden_dir, case, K, which)      # ONE_GOOD off, as the table was made
    r = run_df(tmp_path, golden_dir, which, "HOPS=True", "ONE_GOOD=False", "SUBSET=True")
    assert r.returncode == 0, r.stdout + r.stderr
    w = f"{tmp_path}/GapToy/1/a.48"
    for f in FILES:
        assert open(f"{w}/{f}", "rb").read() == want["files"][f], f
    for f in sorted(os.listdir(f"{golden_dir}/{case}")):                     # everything else DF writes there is still the fixture's
        if f.startswith("a."):
            assert open(f"{w}/{f}", "rb").read() == open(f"{golden_dir}/{case}/{f}", "rb").read(), f
    assert subset_lines(r.stdout) == ["subset is size %d" % len(want["ids"]),
                                      'DF_SUBSET {"ids": %d, "eoi": %d, "path_entries": %d, "index_entries": %d, "ranges": 1, "a.sub.ids": "%016x%016x", "a.sub.eoi": "%016x%016x"}'
                                      % (len(want["ids"]), len(want["eoi"]), want["path_entries"], want["index_entries"], *want["ids_digest"], *want["eoi_digest"])], subset_lines(r.stdout)
    assert r.stdout.index("DF_HOPS ") < r.stdout.index("subset is size")


def test_df_refuses_subset_without_hops(tmp_path, golden_dir):
    r = run_df(tmp_path, golden_dir, "frag", "SUBSET=True")
    assert r.returncode != 0 and "SUBSET=True needs HOPS=True" in r.stdout
    assert not os.path.exists(f"{tmp_path}/GapToy")


@pytest.mark.parametrize("mode", ["loopback2", "forced", "gpus2"])
def test_df_refuses_subset_on_a_sharded_run(tmp_path, golden_dir, mode):
    env = dict(os.environ)
    args = ["HOPS=True", "SUBSET=True"]
    if mode == "loopback2": args.append("NUM_GPUS=2"); env["DF_TRANSPORT"] = "loopback"
    if mode == "forced": env["DF_FORCE_SHARDED"] = "1"
    if mode == "gpus2": args.append("NUM_GPUS=2")
    r = run_df(tmp_path, golden_dir, "frag", *args, env=env)
    assert r.returncode != 0 and "runs on one GPU only" in r.stdout
    assert not os.path.exists(f"{tmp_path}/GapToy")


def test_df_with_hops_alone_writes_no_subset(tmp_path, golden_dir):
    r = run_df(tmp_path, golden_dir, "frag", "HOPS=True")
    assert r.returncode == 0, r.stdout + r.stderr
    w = f"{tmp_path}/GapToy/1/a.48"
    assert os.path.exists(f"{w}/a.hops") and not [f for f in os.listdir(w) if f.startswith("a.sub")]
    assert not subset_lines(r.stdout) and "DF_SUBSET" not in r.stdout and "subset" not in r.stdout
