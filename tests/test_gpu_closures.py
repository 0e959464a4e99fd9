"""CloseGap2's closures per pair on the GPU (dfk_closures_build / _build_arrays / _write: only the closable pairs' stacks touched, the
dimensions, live rows, gather and decode shared with the stack consensus, the merged consensus a workgroup a tile of a closure with a lane a
column over stack 0's live rows then stack 1's) against tests/closures_oracle.py: pair table, starts, records, bases, the file
a.close.closures byte for byte, the counters and the digest -- on every seeded case in batches of 1 and 37 closures and on the four
fixtures; the refusals; the chain dfk_count ... dfk_cons_build -> dfk_offsets_build -> dfk_closures_build; `DF ... OFFSETS=True
CLOSURES=True`.  Everything is exact.

The rule is pinned by the two restatements only (tests/closures_oracle.py, superplus_amd/csrc/dfk_closures.h)."""
import os

import numpy as np
import pytest

from tests import closures_cases, closures_oracle
from tests.test_closures_oracle import TABLE

pytestmark = pytest.mark.gpu

FILE = closures_oracle.FILE
COUNTERS = (("pairs", "pairs"), ("closable", "closable"), ("over", "over"), ("closures", "closures"), ("columns", "columns"), ("cells", "added"), ("live", "live"), ("empty", "empty"),
            ("short", "short"), ("rowless", "rowless"))


def check(st, got, file, want, what):
    assert [int(x) for x in got["pair_first"]] == want["pair_first"], f"{what}: the pair table"
    assert [int(x) for x in got["starts"]] == want["starts"], f"{what}: starts"
    assert [tuple(int(x) for x in r) for r in got["records"]] == want["records"], f"{what}: records"
    assert np.array_equal(got["bases"], want["bases"]), f"{what}: {int((got['bases'] != want['bases']).sum()) if len(got['bases']) == len(want['bases']) else 'all'} bases differ"
    assert tuple(st[k] for k, _ in COUNTERS) == tuple(want[k] for _, k in COUNTERS), f"{what}: {[(k, st[k], want[w]) for k, w in COUNTERS]}"
    assert (st["sum"], st["xor"]) == (want["digest"] if want["closures"] else (0, 0)), f"{what}: the digest"
    if file is not None: assert file == want["file"], f"{what}: {FILE} differs ({len(file)} bytes, {len(want['file'])} expected)"


def written(d, tmp_path, sub):
    out = os.path.join(tmp_path, sub)
    os.makedirs(out, exist_ok=True)
    held = d.stats()["hbm_held"]
    d.closures_write(out)
    assert d.stats()["hbm_held"] == held and os.listdir(out) == [FILE]
    return open(os.path.join(out, FILE), "rb").read()


def through_arrays(d, tmp_path, a, off_first, offsets, want, what, batches):
    n = want["closures"]
    for per in batches:
        out = os.path.join(tmp_path, f"per{per}")
        os.makedirs(out)
        held = d.stats()["hbm_held"]
        st = d.closures_build_arrays(a, off_first, offsets, per, out)
        assert d.stats()["hbm_held"] == held
        check(st, d.closures_fetch(), open(os.path.join(out, FILE), "rb").read(), want, f"{what} closures_per_batch={per}")
        assert st["batches"] == ((n + per - 1) // per if per else (1 if n else 0)) and st["ranges"] == (1 if n else 0) and os.listdir(out) == [FILE]
        assert d.closures_stats() == st


@pytest.fixture(scope="module")
def ctx():
    from superplus_amd.dfk import Dfk
    d = Dfk(K=closures_cases.K)
    yield d
    d.close()


SEEDED = closures_cases.seeded()


# ---- 1. the seeded cases
@pytest.mark.parametrize("name,c", [(n, c) for n, c, _ in SEEDED], ids=[n for n, _, _ in SEEDED])
def test_seeded_cases_match_the_oracle(ctx, tmp_path, monkeypatch, name, c):
    want = closures_cases.oracle(name, c)
    a, off_first, offsets = closures_cases.arrays(c)
    # batches of 1 and 37 closures
    through_arrays(ctx, tmp_path, a, off_first, offsets, want, name, (1, 37))
    # what fits, no directory, the reads dense (the cases' are): the same result, no file; dfk_closures_write then writes the same
    st = ctx.closures_build_arrays(a, off_first, offsets, read_off=None)
    check(st, ctx.closures_fetch(), written(ctx, tmp_path, "later"), want, name + " dense")
    assert st["batches"] == (1 if want["closures"] else 0)
    # small ranges of pairs
    if want["live"] >= 12 and want["closable"] >= 4:
        monkeypatch.setenv("DFK_PIDX_RANGE_PAIRS", str(max(7, want["live"] // 50)))
        st = ctx.closures_build_arrays(a, off_first, offsets, 37)
        check(st, ctx.closures_fetch(), None, want, name + " in small ranges")
        assert st["ranges"] >= 2 and st["batches"] >= st["ranges"]


# ---- 2. the fixtures: the closer tables and partners of the Python oracles, the offsets tests/offsets_oracle.py finds
@pytest.mark.parametrize("case,K,which,row", TABLE, ids=[t[0] for t in TABLE])
def test_fixtures_match_the_oracle(golden_dir, tmp_path, case, K, which, row):
    from superplus_amd.dfk import Dfk
    from tests import closer_oracle, cons_cases, partners_oracle
    want = closures_oracle.fixture_closures(golden_dir, case, K, which)
    assert want["closures"] == row[0] > 0 and want["rowless"] == 0
    i = partners_oracle.fixture_inputs(golden_dir, case, K, which)
    p = partners_oracle.fixture_partners(golden_dir, case, K, which)
    rs = i["rs"]
    c = dict(inv=i["inv"], kmers=closer_oracle.fixture_inputs(golden_dir, case, K, which)["kmers"], ce=i["ce"], locs=i["locs_per"], parts=p["elements"], pairs=i["pairs"],
             reads=[], pq=rs["pq_bytes"], pq_off=rs["pq_off"])
    a = cons_cases.arrays(c)
    a.update(read_packed=rs["packed"], read_off=rs["base_off"], read_len=rs["read_len"])
    d = Dfk(K=K)
    through_arrays(d, tmp_path, a, *closures_oracle.off_arrays(want["offsets_per"]), want, case, (37, 0))
    d.close()


# ---- 3. the refusals
def test_refusals_leave_the_earlier_result_served(tmp_path):
    import ctypes as C
    from superplus_amd.dfk import Dfk, DfkError, lib
    d = Dfk(K=closures_cases.K)
    none = np.zeros(1, np.uint8)
    for call in (lambda: d.closures_build(none, None, np.zeros(0, np.uint32), none, np.zeros(1, np.uint64)), lambda: d.closures_stats(), lambda: d.closures_fetch(),
                 lambda: d.closures_write(str(tmp_path))):
        with pytest.raises(DfkError) as e:
            call()
        assert e.value.code == -6                                                # DFK_E_STATE: no consensus, no closures
    name, c, _ = SEEDED[0]
    want = closures_cases.oracle(name, c)
    a, off_first, offsets = closures_cases.arrays(c)
    st = d.closures_build_arrays(a, off_first, offsets)
    check(st, d.closures_fetch(), None, want, name)
    fell = off_first.copy(); fell[3] = fell[4] + 1
    past, below = offsets.copy(), offsets.copy()
    past[3] = 257                                                                # pair 2's second offset: its stacks are 256 columns wide
    below[5] = -257                                                              # pair 4's
    assert (int(off_first[2]), int(off_first[4])) == (2, 5)
    for code, call in ((-1, lambda: d.closures_build_arrays(a, None, offsets)), (-1, lambda: d.closures_build_arrays(a, off_first, None)), (-1, lambda: d.closures_build_arrays(a, fell, offsets)),
                       (-1, lambda: d.closures_build_arrays(a, off_first, past)), (-1, lambda: d.closures_build_arrays(a, off_first, below)),
                       (-1, lambda: d.closures_build_arrays(a, off_first, offsets, 0, str(tmp_path), inv=None)), (-1, lambda: d.closures_build_arrays(a, off_first, offsets, 0, str(tmp_path), pq_off=None)),
                       (-6, lambda: d.closures_build(none, None, np.zeros(0, np.uint32), none, np.zeros(1, np.uint64)))):       # a consensus from arrays at most: no stacks in the context
        held = d.stats()["hbm_held"]
        with pytest.raises(DfkError) as e:
            call()
        assert e.value.code == code, e.value
        assert d.stats()["hbm_held"] == held
        check(d.closures_stats(), d.closures_fetch(), None, want, "after a refused call")
    assert d.closures_stats() == st and not os.listdir(tmp_path)
    # the ends of the range are taken: off == cols1 and off == -cols2 are cases of their own (pairs 3 and 4)
    # a fetch buffer too small: the counts are still told; NULL with cap 0 gives the counts alone
    npairs, nc, nb = C.c_uint64(), C.c_uint64(), C.c_uint64()
    small = np.zeros(want["columns"], np.uint8)
    rc = lib().dfk_closures_fetch(d._ctx, None, None, None, C.byref(npairs), C.byref(nc), small.ctypes.data_as(C.c_void_p), C.c_uint64(want["columns"] - 1), C.byref(nb))
    assert rc == -1 and (npairs.value, nc.value, nb.value) == (want["pairs"], want["closures"], want["columns"])
    assert lib().dfk_closures_fetch(d._ctx, None, None, None, C.byref(npairs), C.byref(nc), None, C.c_uint64(0), C.byref(nb)) == 0 and nb.value == want["columns"]
    # a directory that does not exist: an error, no file
    with pytest.raises(DfkError) as e:
        d.closures_write(os.path.join(tmp_path, "no", "such"))
    assert e.value.code == -1 and not os.path.exists(os.path.join(tmp_path, "no")) and not os.listdir(tmp_path)
    check(d.closures_stats(), d.closures_fetch(), None, want, "after all refusals")
    d.close()


# ---- 4. the chain, and its state rules
def test_chain_from_count_to_closures(golden_dir, tmp_path):
    from superplus_amd.dfk import DfkError
    from tests import offsets_oracle
    from tests.test_gpu_cons import fixture_arrays, partnered
    case, K, which, row = TABLE[2]                                               # graph_pathy_k48: 63 pairs, 2 closures
    want = closures_oracle.fixture_closures(golden_dir, case, K, which)
    d, rs, i = partnered(golden_dir, tmp_path, case, K, which)
    reads = (rs["packed"], rs["base_off"], rs["read_len"], rs["pq_bytes"], rs["pq_off"])

    def refused(match):
        held = d.stats()["hbm_held"]
        with pytest.raises(DfkError, match=match) as e:
            d.closures_build(*reads)
        assert e.value.code == -6 and d.stats()["hbm_held"] == held
    refused("no stack consensus")                                                # no consensus yet
    d.cons_build(*reads)
    refused("no offsets")                                                        # no offsets yet
    o = offsets_oracle.fixture_offsets(golden_dir, case, K, which)
    d.offsets_build_arrays(*offsets_oracle.starts_and_bases(o["seqs"]))
    refused("dfk_offsets_build_arrays")                                          # offsets from arrays
    d.offsets_build()
    held = d.stats()["hbm_held"]
    st = d.closures_build(*reads)
    assert d.stats()["hbm_held"] == held and st["batches"] == 1 and st["ranges"] == 1 and st["pairs"] == 63 and st["closures"] == 2
    check(st, d.closures_fetch(), written(d, tmp_path, "chain"), want, case + " through the chain")
    # a newer consensus makes the offsets older than it: refused, and the earlier closures are still served
    d.cons_build(*reads)
    refused("older stack consensus")
    check(d.closures_stats(), d.closures_fetch(), None, want, "after a refused call")
    # the read arguments are checked as dfk_cons_build checks them
    d.offsets_build()
    for code, args in ((-1, (None,) + reads[1:]), (-1, (rs["packed"], rs["base_off"][:-2], rs["read_len"][:-2], rs["pq_bytes"], rs["pq_off"][:-2]))):
        with pytest.raises(DfkError) as e:
            d.closures_build(*args)
        assert e.value.code == code
    # a consensus from arrays is the latest: the context holds no stacks for it
    d.cons_build_arrays(fixture_arrays(d, golden_dir, case, K, which, i))
    refused("dfk_cons_build_arrays")
    d.cons_build(*reads); d.offsets_build()
    st2 = d.closures_build(*reads)
    check(st2, d.closures_fetch(), written(d, tmp_path, "again"), want, case + " built again")
    d.close()


# ---- 5. DF
def lines(out, key):
    return [l for l in out.splitlines() if l.startswith(key + " ")]


def test_df_writes_the_closures_file_and_only_when_asked(tmp_path, golden_dir):
    from tests import offsets_oracle
    from tests.test_gpu_hops import run_df
    case, K, which, row = TABLE[0]                                               # graph_frag_k48
    want = closures_oracle.fixture_closures(golden_dir, case, K, which)          # ONE_GOOD off, as the table was made
    args = ("HOPS=True", "ONE_GOOD=False", "CLOSER=True", "PARTNERS=True", "CONS=True", "OFFSETS=True")
    on = os.path.join(tmp_path, "on"); off = os.path.join(tmp_path, "off"); refused = os.path.join(tmp_path, "refused")
    for p in (on, off, refused): os.makedirs(p)
    r = run_df(on, golden_dir, which, *args, "CLOSURES=True")
    assert r.returncode == 0, r.stdout + r.stderr
    w = f"{on}/GapToy/1/a.48"
    assert open(f"{w}/{FILE}", "rb").read() == want["file"]
    assert open(f"{w}/a.close.offsets", "rb").read() == offsets_oracle.fixture_offsets(golden_dir, case, K, which)["file"]
    assert lines(r.stdout, "DF_CLOSURES") == ['DF_CLOSURES {"pairs": %d, "closable": %d, "over": %d, "closures": %d, "columns": %d, "a.close.closures": "%016x%016x", "cells": %d, '
                                              '"live_rows": %d, "empty": %d, "short": %d, "rowless": 0, "batches": 1, "ranges": 1}'
                                              % (want["pairs"], want["closable"], want["over"], want["closures"], want["columns"], *want["digest"], want["added"], want["live"], want["empty"],
                                                 want["short"])], lines(r.stdout, "DF_CLOSURES")
    assert r.stdout.index("DF_OFFSETS ") < r.stdout.index("DF_CLOSURES ")
    # without the switch: no such file, no such line, every other a.close.* file and every DF_* line the same
    r2 = run_df(off, golden_dir, which, *args)
    assert r2.returncode == 0, r2.stdout + r2.stderr
    w2 = f"{off}/GapToy/1/a.48"
    assert not os.path.exists(f"{w2}/{FILE}") and "DF_CLOSURES" not in r2.stdout and FILE not in r2.stdout
    assert sorted(os.listdir(w2)) == sorted(f for f in os.listdir(w) if f != FILE)
    assert all(open(f"{w2}/{f}", "rb").read() == open(f"{w}/{f}", "rb").read() for f in os.listdir(w2) if f.startswith("a.close"))
    same = ("DF_OFFSETS ", "DF_CONS ", "DF_PARTNERS ", "DF_CLOSER ", "DF_HOPS ", "DF_DIGESTS ")
    assert [l for l in r2.stdout.splitlines() if l.startswith(same)] == [l for l in r.stdout.splitlines() if l.startswith(same)]
    assert [l.split(" ")[0] for l in r2.stdout.splitlines() if l.startswith("DF_")] == [l.split(" ")[0] for l in r.stdout.splitlines() if l.startswith("DF_") and not l.startswith("DF_CLOSURES ")]
    # CLOSURES without OFFSETS is refused at argument time, before anything is written
    r3 = run_df(refused, golden_dir, which, "HOPS=True", "CLOSER=True", "PARTNERS=True", "CONS=True", "CLOSURES=True")
    assert r3.returncode != 0 and "CLOSURES=True needs OFFSETS=True" in r3.stdout and not os.path.exists(f"{refused}/GapToy")
