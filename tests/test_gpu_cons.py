"""CloseGap2's stack consensus on the GPU (dfk_cons_build / _write: dimensions a wave a stack, the live rows by flag, scan and emit, the
reads of a batch of stacks gathered once each and decoded, the consensus a workgroup a stack with a lane a column) against
tests/cons_oracle.py: starts, dims, bases, the file a.close.cons byte for byte, the counters and the digest on the fixtures after a real
dfk_count ... dfk_partners_build; the same bytes under small batches and small ranges, before and after the index; seeded arrays through
dfk_cons_build_arrays; the edges of the contract; `DF HOPS=True CLOSER=True PARTNERS=True CONS=True`.  Everything is exact.

The rule is pinned by the two restatements only (tests/cons_oracle.py, superplus_amd/csrc/dfk_cons.h); the closer tables and the partners
the device works on are those tests/test_gpu_closer.py and tests/test_gpu_partners.py hold to their oracles."""
import os

import numpy as np
import pytest

from tests import closer_oracle, cons_cases, cons_oracle, partners_oracle
from tests.test_gpu_hops import BOTH, pathed, run_df
from tests.test_hops_oracle import fixture_inputs as hops_inputs

pytestmark = pytest.mark.gpu

FILE = cons_oracle.FILE
COUNTERS = (("pairs", "pairs"), ("stacks", "n_stacks"), ("rows", "rows"), ("live", "live"), ("rows_kept", "rows_kept"), ("trimmed", "trimmed"), ("reversed", "reversed"),
            ("columns", "columns"), ("cells", "added"))
FIXTURES = [("graph_pathy2_k48", 48, "pathy2"), ("graph_frag_k48", 48, "frag"), ("graph_pathy_k48", 48, "pathy"), ("graph_k40_nobc", 40, "reads")]
READS = ("packed", "base_off", "read_len", "pq_bytes", "pq_off")


def written(d, tmp_path, sub="out"):
    """dfk_cons_write into a directory of its own -> the file's bytes, holding no more of the device than before"""
    out = os.path.join(tmp_path, sub)
    os.makedirs(out, exist_ok=True)
    held = d.stats()["hbm_held"]
    d.cons_write(out)
    assert d.stats()["hbm_held"] == held
    assert os.listdir(out) == [FILE]
    return open(os.path.join(out, FILE), "rb").read()


def check(st, got, file, want, what):
    assert [int(x) for x in got["starts"]] == want["starts"], f"{what}: starts"
    assert [tuple(int(x) for x in d) for d in got["dims"]] == want["dims"], f"{what}: dims"
    assert np.array_equal(got["bases"], want["bases"]), f"{what}: {int((got['bases'] != want['bases']).sum()) if len(got['bases']) == len(want['bases']) else 'all'} bases differ"
    assert tuple(st[k] for k, _ in COUNTERS) == tuple(want[k] for _, k in COUNTERS), f"{what}: {[(k, st[k], want[w]) for k, w in COUNTERS]}"
    assert (st["sum"], st["xor"]) == want["digest"], f"{what}: the digest"
    if file is not None: assert file == want["file"], f"{what}: {FILE} differs ({len(file)} bytes, {len(want['file'])} expected)"


def built(d, tmp_path, rs, pairs=None, sub="out", dense=False):
    held = d.stats()["hbm_held"]
    st = d.cons_build(rs["packed"], None if dense else rs["base_off"], rs["read_len"], rs["pq_bytes"], rs["pq_off"], pairs)
    assert d.stats()["hbm_held"] == held
    got = d.cons_fetch()
    file = written(d, tmp_path, sub)
    assert d.cons_stats() == st
    return st, got, file


def partnered(golden_dir, tmp_path, case, K, which):
    """count ... partners_build on a fixture -> (context, reads, the oracle's inputs)"""
    i = partners_oracle.fixture_inputs(golden_dir, case, K, which)
    rs = i["rs"]
    d = pathed(rs, case, K, tmp_path)
    d.hops_build(hops_inputs(golden_dir, case, K, which)["bc"])
    d.closer_build(i["dup"])
    d.partners_build(rs["packed"], rs["base_off"], rs["read_len"])
    return d, rs, i


def fixture_arrays(d, golden_dir, case, K, which, i):
    """the context's own closer tables and partners, as the arrays entry takes them"""
    c, p, rs = d.closer_fetch(), d.partners_fetch(), i["rs"]
    return dict(inv=np.asarray(i["inv"], np.int32), kmers=np.asarray(closer_oracle.fixture_inputs(golden_dir, case, K, which)["kmers"], np.int32), ce=c["ce"], loc_first=c["loc_first"],
                locs=c["locs"].reshape(-1), part_first=p["starts"], parts=p["recs"].reshape(-1), pairs=np.asarray(i["pairs"], np.int32).reshape(-1, 2),
                read_packed=rs["packed"], read_off=rs["base_off"], read_len=rs["read_len"], pq=rs["pq_bytes"], pq_off=rs["pq_off"])


# ---- 1. the fixtures
@pytest.mark.parametrize("case,K,which", FIXTURES, ids=[f[0] for f in FIXTURES])
def test_consensus_file_and_counters_match_the_oracle_on_the_fixtures(golden_dir, tmp_path, case, K, which):
    want = cons_oracle.fixture_cons(golden_dir, case, K, which)
    assert want["columns"] > 0
    d, rs, i = partnered(golden_dir, tmp_path, case, K, which)
    got = built(d, tmp_path, rs)
    check(*got, want, case)
    assert got[0]["ranges"] == 1 and got[0]["batches"] == 1 and 0 < got[0]["decoded"] <= len(set().union(*(s["ids"] for s in want["stacks"])))
    # the same pairs given explicitly; the reads dense (the fixtures' are: every read a whole number of bytes behind the one before)
    assert int(rs["base_off"][0]) == 0
    got2 = built(d, tmp_path, rs, np.asarray(i["pairs"], np.int32).reshape(-1, 2), "explicit", dense=True)
    d.close()
    check(*got2, want, case + " (pairs given, dense)")
    assert got2[2] == got[2]


# ---- 2. the same bytes under small batches, small ranges, and before and after the index
@pytest.mark.parametrize("variant", ["batches", "ranges", "after the index"])
@pytest.mark.parametrize("case,K,which", BOTH, ids=[b[2] for b in BOTH])
def test_same_bytes_under_small_batches_and_ranges_and_after_the_index(golden_dir, tmp_path, monkeypatch, case, K, which, variant):
    want = cons_oracle.fixture_cons(golden_dir, case, K, which)
    d, rs, i = partnered(golden_dir, tmp_path, case, K, which)
    if variant == "batches":
        a = fixture_arrays(d, golden_dir, case, K, which, i)
        for per in (37, 1):
            out = os.path.join(tmp_path, f"per{per}")
            os.makedirs(out)
            held = d.stats()["hbm_held"]
            st = d.cons_build_arrays(a, per, out)
            assert d.stats()["hbm_held"] == held
            check(st, d.cons_fetch(), open(os.path.join(out, FILE), "rb").read(), want, f"{case} stacks_per_batch={per}")
            assert st["batches"] == (want["n_stacks"] + per - 1) // per and st["ranges"] == 1
    elif variant == "ranges":
        monkeypatch.setenv("DFK_PIDX_RANGE_PAIRS", str(want["rows"] // 6))
        got = built(d, tmp_path, rs, None, "ranges")
        check(*got, want, f"{case} {variant}")
        assert got[0]["ranges"] >= 4 and got[0]["batches"] == got[0]["ranges"]
    else:
        first = built(d, tmp_path, rs, None, "first")
        check(*first, want, f"{case} before the index")
        d.paths_index_dups_write(str(tmp_path), os.path.join(tmp_path, "a.dup"))
        second = built(d, tmp_path, rs, None, "second")
        check(*second, want, f"{case} after the index")
        assert second[2] == first[2]
    d.close()


# ---- 3. seeded arrays
@pytest.fixture(scope="module")
def ctx():
    from superplus_amd.dfk import Dfk
    d = Dfk(K=cons_cases.K)
    yield d
    d.close()


SEEDED = cons_cases.seeded()


@pytest.mark.parametrize("name,c", [(n, c) for n, c, _ in SEEDED], ids=[n for n, _, _ in SEEDED])
def test_seeded_arrays_match_the_oracle(ctx, tmp_path, monkeypatch, name, c):
    want = cons_cases.oracle(name, c)
    a = cons_cases.arrays(c)
    ns = want["n_stacks"]
    # batches of 1, 37 and what fits on the small cases; a batch per stack would be thousands of uploads on the large one
    for per in ((1, 37, 0) if ns <= 1000 else (37, 0)):
        out = os.path.join(tmp_path, f"per{per}")
        os.makedirs(out)
        held = ctx.stats()["hbm_held"]
        st = ctx.cons_build_arrays(a, per, out)
        assert ctx.stats()["hbm_held"] == held
        check(st, ctx.cons_fetch(), open(os.path.join(out, FILE), "rb").read(), want, f"{name} stacks_per_batch={per}")
        assert st["batches"] == ((ns + per - 1) // per if per else (1 if ns else 0)) and st["ranges"] == (1 if ns else 0)
        assert os.listdir(out) == [FILE]
    # dense reads (the cases' are), no directory: the same result, no file; dfk_cons_write then writes the same
    st = ctx.cons_build_arrays(a, read_off=None)
    check(st, ctx.cons_fetch(), written(ctx, tmp_path, "later"), want, name + " dense")
    # small ranges of stacks
    if want["rows"] >= 12:
        monkeypatch.setenv("DFK_PIDX_RANGE_PAIRS", str(max(1, want["rows"] // 5)))
        st = ctx.cons_build_arrays(a, 37)
        check(st, ctx.cons_fetch(), None, want, name + " in small ranges")
        assert st["ranges"] >= 3


def test_arrays_refusals(ctx, tmp_path):
    from superplus_amd.dfk import DfkError
    name, c, _ = SEEDED[0]
    want = cons_cases.oracle(name, c)
    a = cons_cases.arrays(c)
    st = ctx.cons_build_arrays(a)
    E = len(c["inv"])
    not_closer = next(e for e in range(E) if e not in c["ce"])
    fell = a["read_off"].copy(); fell[3] = fell[2] - 1
    qfell = a["pq_off"].copy(); qfell[3] = qfell[2] - 1
    live_read = int(c["locs"][0][0][0])                                # the first row of the first closer edge (ROUND): live
    assert want["stacks"][0]["live"] == 8 and len(c["reads"][live_read]) == 2
    short = a["read_len"].copy(); short[live_read] += 1                 # its stream is now one value short
    for code, change in ((-1, dict(pairs=np.asarray([(0, E)], np.int32))), (-1, dict(pairs=np.asarray([(-1, 0)], np.int32))),
                         (-1, dict(pairs=np.asarray([(not_closer, c["inv"][not_closer])], np.int32), part_first=np.zeros(3, np.uint64))),      # an edge of the graph that is no closer edge
                         (-1, dict(inv=None)), (-1, dict(read_len=None)), (-1, dict(loc_first=None)), (-1, dict(pq=None)), (-1, dict(pq_off=None)), (-1, dict(part_first=None)),
                         (-5, dict(read_off=fell)), (-5, dict(pq_off=qfell)), (-5, dict(read_len=short))):                                     # DFK_E_INPUT
        with pytest.raises(DfkError) as e:
            ctx.cons_build_arrays(a, 0, str(tmp_path), **change)
        assert e.value.code == code, (change.keys(), e.value)
    assert not os.listdir(tmp_path)
    check(ctx.cons_stats(), ctx.cons_fetch(), None, want, "the earlier result")
    assert ctx.cons_stats() == st


# ---- 4. the contract
def test_state_rules_and_the_edges_of_the_contract(golden_dir, tmp_path):
    import ctypes as C
    from superplus_amd.dfk import Dfk, DfkError, lib
    from tests.test_gpu_hops import ARRAYS
    from tests.test_gpu_paths import KW
    case, K, which = BOTH[1]
    want = cons_oracle.fixture_cons(golden_dir, case, K, which)
    i = partners_oracle.fixture_inputs(golden_dir, case, K, which)
    rs, dup, pairs = i["rs"], i["dup"], np.asarray(i["pairs"], np.int32).reshape(-1, 2)
    reads = tuple(rs[k] for k in READS)
    d = Dfk(K=K, mark_bads=True, **KW[case])
    d.count(*(rs[k] for k in ARRAYS), rs["bc"]); d.graph_build()
    for call in (lambda: d.cons_build(*reads, pairs), lambda: d.cons_stats(), lambda: d.cons_fetch(), lambda: d.cons_write(str(tmp_path))):
        with pytest.raises(DfkError) as e:
            call()
        assert e.value.code == -6                                            # DFK_E_STATE: before dfk_paths_build
    d.paths_build(*(rs[k] for k in ARRAYS))
    with pytest.raises(DfkError, match="dfk_closer_build") as e:
        d.cons_build(*reads, pairs)                                          # no closer sets
    assert e.value.code == -6
    d.closer_build(dup, pairs)
    with pytest.raises(DfkError, match="dfk_partners_build") as e:
        d.cons_build(*reads, pairs)                                          # no partners
    assert e.value.code == -6
    d.partners_build(rs["packed"], rs["base_off"], rs["read_len"], pairs)
    with pytest.raises(DfkError, match="dfk_hops_build") as e:
        d.cons_build(*reads)                                                 # no hops result to take the pairs from
    assert e.value.code == -6
    with pytest.raises(DfkError, match="dfk_cons_build") as e:
        d.cons_write(str(tmp_path))
    assert e.value.code == -6 and not os.listdir(tmp_path)
    first = built(d, tmp_path, rs, pairs)
    check(*first, want, "pairs given, no hops result")
    # refused, and the earlier result still served whole: other pairs, reads that are not the paths', a null argument, a table that falls, a
    # PQVec stream one value short (of a read that stands in a stack's window)
    fell = rs["base_off"].copy(); fell[5] = fell[4] - 1
    qfell = rs["pq_off"].copy(); qfell[5] = qfell[4] - 1
    live_read = next(id for s in want["stacks"] if s["live"] == s["rows"] and s["rows"] for id in sorted(s["ids"]))
    longer = rs["read_len"].copy(); longer[live_read] += 1                  # one base more: its stream is now one value short
    packed1, off1 = rs["packed"], rs["base_off"]
    if rs["read_len"][live_read] % 4 == 0:                                  # (the base needs a byte of its own)
        packed1 = np.insert(rs["packed"], int(off1[live_read + 1]), 0); off1 = off1.copy(); off1[live_read + 1:] += 1
    for code, call in ((-1, lambda: d.cons_build(*reads, pairs[:50])), (-1, lambda: d.cons_build(*reads, pairs[::-1])),
                       (-1, lambda: d.cons_build(rs["packed"], rs["base_off"][:-2], rs["read_len"][:-2], rs["pq_bytes"], rs["pq_off"][:-2], pairs)),
                       (-1, lambda: d.cons_build(None, rs["base_off"], rs["read_len"], rs["pq_bytes"], rs["pq_off"], pairs)),
                       (-1, lambda: d.cons_build(rs["packed"], rs["base_off"], rs["read_len"], None, rs["pq_off"], pairs)),
                       (-5, lambda: d.cons_build(rs["packed"], fell, rs["read_len"], rs["pq_bytes"], rs["pq_off"], pairs)),
                       (-5, lambda: d.cons_build(rs["packed"], rs["base_off"], rs["read_len"], rs["pq_bytes"], qfell, pairs)),
                       (-5, lambda: d.cons_build(packed1, off1, longer, rs["pq_bytes"], rs["pq_off"], pairs))):
        held = d.stats()["hbm_held"]
        with pytest.raises(DfkError) as e:
            call()
        assert e.value.code == code, e.value
        assert d.stats()["hbm_held"] == held
        check(d.cons_stats(), d.cons_fetch(), None, want, "after a refused call")
    assert d.cons_stats() == first[0]
    # a fetch buffer too small: the counts are still told
    ne, nb = C.c_uint64(), C.c_uint64()
    small = np.zeros(want["columns"], np.uint8)
    rc = lib().dfk_cons_fetch(d._ctx, None, None, C.byref(ne), small.ctypes.data_as(C.c_void_p), C.c_uint64(want["columns"] - 1), C.byref(nb))
    assert rc == -1 and (ne.value, nb.value) == (2 * len(pairs), want["columns"])
    # a directory that does not exist: an error, no file
    gone = os.path.join(tmp_path, "no", "such")
    with pytest.raises(DfkError) as e:
        d.cons_write(gone)
    assert e.value.code == -1 and not os.path.exists(os.path.join(tmp_path, "no"))
    # the graph built again: the paths and everything made from them are gone
    d.graph_build()
    with pytest.raises(DfkError) as e:
        d.cons_fetch()
    assert e.value.code == -6
    d.close()


# ---- 5. DF
def cons_lines(out):
    return [l for l in out.splitlines() if l.startswith("DF_CONS ")]


def test_df_writes_the_consensus_file(tmp_path, golden_dir):
    case, K, which = BOTH[1]
    want = cons_oracle.fixture_cons(golden_dir, case, K, which)                # ONE_GOOD off, as the table was made
    r = run_df(tmp_path, golden_dir, which, "HOPS=True", "ONE_GOOD=False", "CLOSER=True", "PARTNERS=True", "CONS=True")
    assert r.returncode == 0, r.stdout + r.stderr
    w = f"{tmp_path}/GapToy/1/a.48"
    assert open(f"{w}/{FILE}", "rb").read() == want["file"]
    assert open(f"{w}/a.close.partners", "rb").read() == partners_oracle.fixture_partners(golden_dir, case, K, which)["file"]
    for f in sorted(os.listdir(f"{golden_dir}/{case}")):                       # everything else DF writes there is still the fixture's
        if f.startswith("a."):
            assert open(f"{w}/{f}", "rb").read() == open(f"{golden_dir}/{case}/{f}", "rb").read(), f
    assert cons_lines(r.stdout) == ['DF_CONS {"pairs": %d, "stacks": %d, "trimmed": %d, "rows_kept": %d, "columns": %d, "a.close.cons": "%016x%016x", "rows": %d, '
                                    '"live_rows": %d, "reversed": %d, "cells": %d, "batches": 1, "ranges": 1}'
                                    % (want["pairs"], want["n_stacks"], want["trimmed"], want["rows_kept"], want["columns"], *want["digest"], want["rows"], want["live"], want["reversed"],
                                       want["added"])], cons_lines(r.stdout)
    assert r.stdout.index("DF_PARTNERS ") < r.stdout.index("DF_CONS ")


def test_df_refuses_cons_without_partners_and_on_a_sharded_run(tmp_path, golden_dir):
    r = run_df(tmp_path, golden_dir, "frag", "HOPS=True", "CLOSER=True", "CONS=True")
    assert r.returncode != 0 and "CONS=True needs PARTNERS=True" in r.stdout
    assert not os.path.exists(f"{tmp_path}/GapToy")
    env = dict(os.environ)
    env["DF_FORCE_SHARDED"] = "1"
    r = run_df(tmp_path, golden_dir, "frag", "HOPS=True", "CLOSER=True", "PARTNERS=True", "CONS=True", env=env)
    assert r.returncode != 0 and "runs on one GPU only" in r.stdout
    assert not os.path.exists(f"{tmp_path}/GapToy")


def test_df_without_the_switch_writes_and_prints_what_it_did(tmp_path, golden_dir):
    """CONS=False against the argument absent: the same listing, the same a.close.* bytes, the same DF_ lines"""
    runs = []
    for sub, extra in (("absent", []), ("off", ["CONS=False"])):
        root = os.path.join(tmp_path, sub)
        os.makedirs(root)
        r = run_df(root, golden_dir, "frag", "HOPS=True", "CLOSER=True", "PARTNERS=True", *extra)
        assert r.returncode == 0, r.stdout + r.stderr
        w = f"{root}/GapToy/1/a.48"
        assert not os.path.exists(f"{w}/{FILE}") and "DF_CONS" not in r.stdout and "a.close.cons" not in r.stdout
        runs.append((sorted(os.listdir(w)), {f: open(f"{w}/{f}", "rb").read() for f in os.listdir(w) if f.startswith("a.close")},
                     [l.split(" ")[0] for l in r.stdout.splitlines() if l.startswith("DF_")],
                     [l for l in r.stdout.splitlines() if l.startswith(("DF_PARTNERS ", "DF_CLOSER ", "DF_HOPS ", "DF_DIGESTS "))]))
    assert runs[0] == runs[1] and "a.close.partners" in runs[0][0]
