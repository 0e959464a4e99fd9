"""CloseGap2's search for unplaced partners on the GPU (dfk_partners_build / _write: the forward parts, the queries by flag, scan and emit,
the table of anchor 32-mers a range of ranks at a time, the search a wave a query, the compaction) against tests/partners_oracle.py:
records, starts, the file a.close.partners byte for byte, the counters and the digest on the fixtures after a real dfk_count ...
dfk_closer_build; seeded arrays through dfk_partners_build_arrays; the same bytes under small query batches and small ranges, before and
after the index; the edges of the contract; `DF HOPS=True CLOSER=True PARTNERS=True`.  Everything is exact.

The rule is pinned by the two restatements only (tests/partners_oracle.py, superplus_amd/csrc/dfk_partners.h); the closer tables the
device works on are those tests/test_gpu_closer.py holds to tests/closer_oracle.py."""
import os

import numpy as np
import pytest

from tests import partners_cases, partners_oracle
from tests.closer_oracle import loc_words
from tests.test_gpu_hops import ARRAYS, BOTH, pathed, run_df
from tests.test_hops_oracle import fixture_inputs as hops_inputs

pytestmark = pytest.mark.gpu

FILE = partners_oracle.FILE
COUNTERS = (("pairs", "pairs"), ("queries", "queries"), ("positions", "positions"), ("entries", "entries"), ("any_hit", "any_hit"), ("kept", "kept"), ("multi", "multi"), ("searched", "searched"))
# the fixtures of the issue's table: pairs, queries, read positions, any hit, kept, several positions
FIXTURES = [("graph_pathy2_k48", 48, "pathy2", (725, 47552, 4235662, 274, 265, 9)), ("graph_frag_k48", 48, "frag", (937, 11798, 814062, 2168, 2168, 0)),
            ("graph_pathy_k48", 48, "pathy", (63, 5259, 466977, 55, 45, 10)), ("graph_k40_nobc", 40, "reads", (138, 11598, 606012, 7, 7, 0))]


def written(d, tmp_path, sub="out"):
    """dfk_partners_write into a directory of its own -> the file's bytes, holding no more of the device than before"""
    out = os.path.join(tmp_path, sub)
    os.makedirs(out, exist_ok=True)
    held = d.stats()["hbm_held"]
    d.partners_write(out)
    assert d.stats()["hbm_held"] == held
    assert os.listdir(out) == [FILE]
    return open(os.path.join(out, FILE), "rb").read()


def check(st, got, file, want, what):
    assert [int(x) for x in got["starts"]] == want["starts"], f"{what}: starts"
    assert np.array_equal(got["recs"].reshape(-1), loc_words(want["records"])), f"{what}: records"
    assert tuple(st[k] for k, _ in COUNTERS) == tuple(want[k] for _, k in COUNTERS), f"{what}: {[(k, st[k], want[w]) for k, w in COUNTERS]}"
    assert (st["sum"], st["xor"]) == want["digest"], f"{what}: the digest"
    if file is not None: assert file == want["file"], f"{what}: {FILE} differs ({len(file)} bytes, {len(want['file'])} expected)"


def built(d, tmp_path, rs, pairs=None, sub="out", dense=False):
    held = d.stats()["hbm_held"]
    st = d.partners_build(rs["packed"], None if dense else rs["base_off"], rs["read_len"], pairs)
    assert d.stats()["hbm_held"] == held
    got = d.partners_fetch()
    file = written(d, tmp_path, sub)
    assert d.partners_stats() == st
    return st, got, file


def closed(golden_dir, tmp_path, case, K, which, monkeypatch=None):
    """count ... closer_build on a fixture -> (context, reads, the oracle's inputs)"""
    i = partners_oracle.fixture_inputs(golden_dir, case, K, which)
    d = pathed(i["rs"], case, K, tmp_path, monkeypatch)
    d.hops_build(hops_inputs(golden_dir, case, K, which)["bc"])
    d.closer_build(i["dup"])
    return d, i["rs"], i


# ---- 1. the fixtures
@pytest.mark.parametrize("case,K,which,row", FIXTURES, ids=[f[0] for f in FIXTURES])
def test_records_file_and_counters_match_the_oracle_on_the_fixtures(golden_dir, tmp_path, case, K, which, row):
    want = partners_oracle.fixture_partners(golden_dir, case, K, which)
    assert (want["pairs"], want["queries"], want["positions"], want["any_hit"], want["kept"], want["multi"]) == row and want["kept"] > 0
    d, rs, i = closed(golden_dir, tmp_path, case, K, which)
    got = built(d, tmp_path, rs)
    check(*got, want, case)
    assert got[0]["ranges"] == 1 and got[0]["batches"] == 1
    # the same pairs given explicitly; the reads dense (the fixtures' are: every read a whole number of bytes behind the one before)
    assert int(rs["base_off"][0]) == 0
    got2 = built(d, tmp_path, rs, np.asarray(i["pairs"], np.int32).reshape(-1, 2), "explicit", dense=True)
    d.close()
    check(*got2, want, case + " (pairs given, dense)")
    assert got2[2] == got[2]


# ---- 2. the same bytes under small ranges of the table and of the sides, and before and after the index
@pytest.mark.parametrize("variant", ["ranges", "after the index"])
@pytest.mark.parametrize("case,K,which", BOTH, ids=[b[2] for b in BOTH])
def test_same_bytes_under_small_ranges_and_after_the_index(golden_dir, tmp_path, monkeypatch, case, K, which, variant):
    want = partners_oracle.fixture_partners(golden_dir, case, K, which)
    d, rs, i = closed(golden_dir, tmp_path, case, K, which)
    if variant == "ranges":
        monkeypatch.setenv("DFK_PIDX_RANGE_PAIRS", str(want["entries"] // 6))
        got = built(d, tmp_path, rs, None, "ranges")
        check(*got, want, f"{case} {variant}")
        assert got[0]["ranges"] >= 4 and got[0]["batches"] >= got[0]["ranges"]
    else:
        first = built(d, tmp_path, rs, None, "first")
        check(*first, want, f"{case} before the index")
        d.paths_index_dups_write(str(tmp_path), os.path.join(tmp_path, "a.dup"))
        second = built(d, tmp_path, rs, None, "second")
        check(*second, want, f"{case} after the index")
        assert second[2] == first[2]
    d.close()


def test_a_fixture_through_the_arrays_in_small_batches(golden_dir, tmp_path):
    """frag's own closer tables as dfk_closer_fetch gives them, the edges' bases from the reference-written a.fastb, query batches of 997"""
    from superplus_amd import feudal
    case, K, which = BOTH[1]
    want = partners_oracle.fixture_partners(golden_dir, case, K, which)
    d, rs, i = closed(golden_dir, tmp_path, case, K, which)
    c = d.closer_fetch()
    ep, eo, el = feudal.read_fastb(os.path.join(golden_dir, case, "a.fastb"))
    a = dict(inv=np.asarray(i["inv"], np.int32), edge_packed=ep, edge_off=eo, edge_len=el, ce=c["ce"], loc_first=c["loc_first"], locs=c["locs"].reshape(-1),
             anchor_first=c["anchor_first"], anchors=c["anchors"].reshape(-1), pairs=np.asarray(i["pairs"], np.int32).reshape(-1, 2),
             read_packed=rs["packed"], read_off=rs["base_off"], read_len=rs["read_len"])
    held = d.stats()["hbm_held"]
    st = d.partners_build_arrays(a, 997, str(tmp_path))
    assert d.stats()["hbm_held"] == held
    check(st, d.partners_fetch(), open(os.path.join(tmp_path, FILE), "rb").read(), want, f"{case} through the arrays")
    assert st["batches"] == (want["searched"] + 996) // 997 > 1
    d.close()


# ---- 3. seeded arrays
@pytest.fixture(scope="module")
def ctx():
    from superplus_amd.dfk import Dfk
    d = Dfk(K=partners_cases.K)
    yield d
    d.close()


SEEDED = partners_cases.seeded()


@pytest.mark.parametrize("name,c", [(n, c) for n, c, _ in SEEDED], ids=[n for n, _, _ in SEEDED])
def test_seeded_arrays_match_the_oracle(ctx, tmp_path, name, c):
    want = partners_cases.oracle(name, c)
    a = partners_cases.arrays(c)
    nq = want["searched"]                                         # (queries against an edge without anchors never reach a batch)
    # query batches of 1, 37 and what fits on the small cases; a batch per query would be thousands of uploads on the large one
    for per in ((1, 37, 0) if nq <= 1000 else (2049, 0)):
        out = os.path.join(tmp_path, f"per{per}")
        os.makedirs(out)
        held = ctx.stats()["hbm_held"]
        st = ctx.partners_build_arrays(a, per, out)
        assert ctx.stats()["hbm_held"] == held
        check(st, ctx.partners_fetch(), open(os.path.join(out, FILE), "rb").read(), want, f"{name} queries_per_batch={per}")
        assert st["batches"] == ((nq + per - 1) // per if per else (1 if nq else 0)) and st["ranges"] == (1 if len(c["ce"]) else 0)
        assert os.listdir(out) == [FILE]
    # dense reads (the cases' are), no directory: the same result, no file; dfk_partners_write then writes the same
    st = ctx.partners_build_arrays(a, read_off=None)
    check(st, ctx.partners_fetch(), written(ctx, tmp_path, "later"), want, name + " dense")


@pytest.mark.parametrize("name", ["planted-more", "large-bod"])
def test_seeded_arrays_in_small_ranges(ctx, tmp_path, monkeypatch, name):
    c = next(c for n, c, _ in SEEDED if n == name)
    want = partners_cases.oracle(name, c)
    monkeypatch.setenv("DFK_PIDX_RANGE_PAIRS", str(max(1, want["entries"] // 5)))
    st = ctx.partners_build_arrays(partners_cases.arrays(c), 37, str(tmp_path))
    check(st, ctx.partners_fetch(), open(os.path.join(tmp_path, FILE), "rb").read(), want, name)
    assert st["ranges"] >= 3


def test_arrays_refusals(ctx, tmp_path):
    from superplus_amd.dfk import DfkError
    name, c, _ = SEEDED[0]
    want = partners_cases.oracle(name, c)
    a = partners_cases.arrays(c)
    st = ctx.partners_build_arrays(a)
    E = len(c["inv"])
    not_closer = next(e for e in range(E) if e not in c["ce"])
    fell = a["read_off"].copy(); fell[3] = fell[2] - 1
    short = a["read_off"].copy(); short[2:] -= 1                     # read 1 (64 bases) is left 15 bytes
    swapped = a["locs"].copy(); k = c["ce"].index(11); j = int(a["loc_first"][k]); swapped[2 * j], swapped[2 * j + 4] = swapped[2 * j + 4], swapped[2 * j]
    for code, change in ((-1, dict(pairs=np.asarray([(0, E)], np.int32))), (-1, dict(pairs=np.asarray([(-1, 0)], np.int32))),
                         (-1, dict(pairs=np.asarray([(not_closer, c["inv"][not_closer])], np.int32))),              # an edge of the graph that is no closer edge
                         (-1, dict(read_len=a["read_len"][:-1], read_off=a["read_off"][:-1])),                      # an odd number of reads
                         (-1, dict(locs=swapped)),                                                                 # the forward part not ascending
                         (-1, dict(inv=None)), (-1, dict(read_len=None)), (-1, dict(loc_first=None)),
                         (-5, dict(read_off=fell)), (-5, dict(read_off=short))):                                    # DFK_E_INPUT
        with pytest.raises(DfkError) as e:
            ctx.partners_build_arrays(a, 0, str(tmp_path), **change)
        assert e.value.code == code, (change.keys(), e.value)
    assert not os.listdir(tmp_path)
    check(ctx.partners_stats(), ctx.partners_fetch(), None, want, "the earlier result")
    assert ctx.partners_stats() == st


# ---- 4. the contract
def test_state_rules_and_the_edges_of_the_contract(golden_dir, tmp_path):
    import ctypes as C
    from superplus_amd.dfk import Dfk, DfkError, lib
    from tests.test_gpu_paths import KW
    case, K, which = BOTH[1]
    want = partners_oracle.fixture_partners(golden_dir, case, K, which)
    i = partners_oracle.fixture_inputs(golden_dir, case, K, which)
    rs, dup, pairs = i["rs"], i["dup"], np.asarray(i["pairs"], np.int32).reshape(-1, 2)
    reads = (rs["packed"], rs["base_off"], rs["read_len"])
    d = Dfk(K=K, mark_bads=True, **KW[case])
    d.count(*(rs[k] for k in ARRAYS), rs["bc"]); d.graph_build()
    for call in (lambda: d.partners_build(*reads, pairs), lambda: d.partners_stats(), lambda: d.partners_fetch(), lambda: d.partners_write(str(tmp_path))):
        with pytest.raises(DfkError) as e:
            call()
        assert e.value.code == -6                                            # DFK_E_STATE: before dfk_paths_build
    d.paths_build(*(rs[k] for k in ARRAYS))
    with pytest.raises(DfkError, match="dfk_closer_build") as e:
        d.partners_build(*reads, pairs)                                      # no closer sets
    assert e.value.code == -6
    d.closer_build(dup, pairs[:50])
    with pytest.raises(DfkError, match="not among the closer edges") as e:
        d.partners_build(*reads, pairs)                                      # closer sets made for other pairs
    assert e.value.code == -1
    with pytest.raises(DfkError, match="dfk_hops_build") as e:
        d.partners_build(*reads)                                             # no hops result to take the pairs from
    assert e.value.code == -6
    with pytest.raises(DfkError, match="dfk_partners_build") as e:
        d.partners_write(str(tmp_path))
    assert e.value.code == -6 and not os.listdir(tmp_path)
    d.closer_build(dup, pairs)
    first = built(d, tmp_path, rs, pairs)
    check(*first, want, "pairs given, no hops result")
    # refused, and the earlier result still served whole: reads that are not the paths', a null argument, an edge outside the graph, a table that falls
    E = len(i["inv"])
    bad_pairs = pairs.copy(); bad_pairs[3, 1] = E
    fell = rs["base_off"].copy(); fell[5] = fell[4] - 1
    for code, call in ((-1, lambda: d.partners_build(rs["packed"], rs["base_off"][:-2], rs["read_len"][:-2], pairs)), (-1, lambda: d.partners_build(None, rs["base_off"], rs["read_len"], pairs)),
                       (-1, lambda: d.partners_build(*reads, bad_pairs)), (-5, lambda: d.partners_build(rs["packed"], fell, rs["read_len"], pairs))):
        with pytest.raises(DfkError) as e:
            call()
        assert e.value.code == code
        check(d.partners_stats(), d.partners_fetch(), None, want, "after a refused call")
    assert d.partners_stats() == first[0]
    # a fetch buffer too small: the counts are still told
    ne, nr = C.c_uint64(), C.c_uint64()
    small = np.zeros(max(1, want["kept"] - 1) * 2, np.uint64)
    rc = lib().dfk_partners_fetch(d._ctx, None, C.byref(ne), small.ctypes.data_as(C.c_void_p), C.c_uint64(want["kept"] - 1), C.byref(nr))
    assert rc == -1 and (ne.value, nr.value) == (2 * len(pairs), want["kept"])
    # a directory that does not exist: an error, no file
    gone = os.path.join(tmp_path, "no", "such")
    with pytest.raises(DfkError) as e:
        d.partners_write(gone)
    assert e.value.code == -1 and not os.path.exists(os.path.join(tmp_path, "no"))
    # the graph built again: the paths and everything made from them are gone
    d.graph_build()
    with pytest.raises(DfkError) as e:
        d.partners_fetch()
    assert e.value.code == -6
    d.close()


# ---- 5. DF
def partners_lines(out):
    return [l for l in out.splitlines() if l.startswith("DF_PARTNERS ")]


@pytest.mark.parametrize("case,K,which", BOTH, ids=[b[2] for b in BOTH])
def test_df_writes_the_partners_file(tmp_path, golden_dir, case, K, which):
    want = partners_oracle.fixture_partners(golden_dir, case, K, which)      # ONE_GOOD off, as the table was made
    r = run_df(tmp_path, golden_dir, which, "HOPS=True", "ONE_GOOD=False", "CLOSER=True", "PARTNERS=True")
    assert r.returncode == 0, r.stdout + r.stderr
    w = f"{tmp_path}/GapToy/1/a.48"
    assert open(f"{w}/{FILE}", "rb").read() == want["file"]
    for f in sorted(os.listdir(f"{golden_dir}/{case}")):                     # everything else DF writes there is still the fixture's
        if f.startswith("a."):
            assert open(f"{w}/{f}", "rb").read() == open(f"{golden_dir}/{case}/{f}", "rb").read(), f
    assert partners_lines(r.stdout) == ['DF_PARTNERS {"pairs": %d, "queries": %d, "kept": %d, "dropped_multi": %d, "a.close.partners": "%016x%016x", "positions": %d, '
                                        '"entries": %d, "batches": 1, "ranges": 1}'
                                        % (want["pairs"], want["queries"], want["kept"], want["multi"], *want["digest"], want["positions"], want["entries"])], partners_lines(r.stdout)
    assert r.stdout.index("DF_CLOSER ") < r.stdout.index("DF_PARTNERS ")


def test_df_refuses_partners_without_closer_and_on_a_sharded_run(tmp_path, golden_dir):
    r = run_df(tmp_path, golden_dir, "frag", "HOPS=True", "PARTNERS=True")
    assert r.returncode != 0 and "PARTNERS=True needs CLOSER=True" in r.stdout
    assert not os.path.exists(f"{tmp_path}/GapToy")
    env = dict(os.environ)
    env["DF_FORCE_SHARDED"] = "1"
    r = run_df(tmp_path, golden_dir, "frag", "HOPS=True", "CLOSER=True", "PARTNERS=True", env=env)
    assert r.returncode != 0 and "runs on one GPU only" in r.stdout
    assert not os.path.exists(f"{tmp_path}/GapToy")


def test_df_without_the_switch_writes_and_prints_nothing_of_it(tmp_path, golden_dir):
    r = run_df(tmp_path, golden_dir, "frag", "HOPS=True", "CLOSER=True")
    assert r.returncode == 0, r.stdout + r.stderr
    w = f"{tmp_path}/GapToy/1/a.48"
    assert not os.path.exists(f"{w}/{FILE}") and sorted(f for f in os.listdir(w) if f.startswith("a.close")) == sorted(["a.close.edges", "a.close.locs", "a.close.anchors", "a.close.reads"])
    assert not partners_lines(r.stdout) and "DF_PARTNERS" not in r.stdout and "partners" not in r.stdout.lower()
