"""Stackster's stack consensus per pair on the GPU (dfk_scons_build / _write: the live rows of a range of pairs from the walks' placed
records, the reads of a batch of stacks gathered once each, decoded and lowered, Consensus1 with qualities a workgroup a tile of 256
columns, the flat pass a lane a column, the conflicts a workgroup a pair) against tests/scons_oracle.py: the dims, con, conq, the
conflict counts, the file a.stack.cons byte for byte, the counters and the digest -- on every seeded case of tests/scons_cases.py in
batches of 1, 37 and what fits and in small ranges; on five fixtures after a real dfk_count ... dfk_closer_build, dfk_walks_build; each
refusal with the next good call behind it; `DF HOPS=True CLOSER=True WALKS=True SCONS=True`.  Everything is exact.

The rule is pinned by the two restatements only (tests/scons_oracle.py, superplus_amd/csrc/dfk_scons.h); the walks the device works on are
those tests/test_gpu_walks.py holds to its oracle.  graph_pathy2_k48 stays with the CPU tests."""
import os

import numpy as np
import pytest

from tests import closer_oracle, scons_cases, scons_oracle, walks_oracle
from tests.test_gpu_hops import pathed, run_df
from tests.test_hops_oracle import fixture_inputs as hops_inputs

pytestmark = pytest.mark.gpu

FILE = scons_oracle.FILE
COUNTERS = ("pairs", "yields", "stacks", "rows", "rows_kept", "trimmed", "columns", "cells", "capped", "recount", "flat", "allowed", "disallowed")
FIXTURES = [("graph_frag_k48", 48, "frag"), ("graph_pathy_k48", 48, "pathy"), ("graph_k48", 48, "reads"), ("graph_k40_nobc", 40, "reads"), ("graph_special_k48", 48, "special")]
READS = ("packed", "base_off", "read_len", "pq_bytes", "pq_off")
LIMIT = 300                                                                    # seconds a test may take


@pytest.fixture(autouse=True)
def time_limit():
    """every GPU step under a time limit of its own: faulthandler's watchdog is a thread of the C runtime, so it ends the process even
    while the test waits inside the library for a kernel that does not come back (a Python signal handler would not run there)"""
    import faulthandler
    faulthandler.dump_traceback_later(LIMIT, exit=True)
    yield
    faulthandler.cancel_dump_traceback_later()


def check(st, got, file, want, what):
    el = want["elements"]
    assert [tuple(int(x) for x in d) for d in got["dims"]] == [tuple(scons_oracle.dim_words(e)) for e in el], f"{what}: dims"
    assert [int(x) for x in got["starts"]] == [0] + list(np.cumsum([e["cols"] for e in el])), f"{what}: starts"
    assert [int(x) for x in got["conflict_first"]] == [0] + list(np.cumsum([len(t) for t in want["counts"]])), f"{what}: conflict starts"
    assert [int(b) for b in got["con"]] == [b for e in el for b in e["con"]], f"{what}: con"
    assert [int(q) for q in got["conq"]] == [q for e in el for q in e["conq"]], f"{what}: conq"
    assert [int(x) for x in got["counts"]] == [x for t in want["counts"] for x in t], f"{what}: conflict counts"
    assert tuple(st[k] for k in COUNTERS) == tuple(want[k] for k in COUNTERS), f"{what}: {[(k, st[k], want[k]) for k in COUNTERS]}"
    assert (st["sum"], st["xor"]) == want["digest"], f"{what}: the digest"
    if file is not None: assert file == want["file"], f"{what}: {FILE} differs ({len(file)} bytes, {len(want['file'])} expected)"


def written(d, tmp_path, sub="out"):
    out = os.path.join(tmp_path, sub)
    os.makedirs(out, exist_ok=True)
    held = d.stats()["hbm_held"]
    d.scons_write(out)
    assert d.stats()["hbm_held"] == held and os.listdir(out) == [FILE]
    return open(os.path.join(out, FILE), "rb").read()


# ---- 1. the seeded cases
@pytest.fixture(scope="module")
def ctx():
    from superplus_amd.dfk import Dfk
    d = Dfk(K=scons_cases.K)
    yield d
    d.close()


SEEDED = scons_cases.seeded()


@pytest.mark.parametrize("name,c", SEEDED, ids=[n for n, _ in SEEDED])
def test_seeded_arrays_match_the_oracle(ctx, tmp_path, monkeypatch, name, c):
    d = ctx
    want = scons_cases.oracle(name, c)
    a = scons_cases.arrays(c)
    npairs = want["pairs"]
    for per in (1, 37, 0):
        out = os.path.join(tmp_path, f"per{per}")
        os.makedirs(out)
        held = d.stats()["hbm_held"]
        st = d.scons_build_arrays(a, per, out)
        assert d.stats()["hbm_held"] == held
        check(st, d.scons_fetch(), open(os.path.join(out, FILE), "rb").read(), want, f"{name} stacks_per_batch={per}")
        assert st["batches"] == ((2 * npairs + per - 1) // per if per else (1 if npairs else 0)) and st["ranges"] == (1 if npairs else 0)
        assert os.listdir(out) == [FILE]
    # dense reads (the cases' are), no directory: the same result, no file; dfk_scons_write then writes the same
    st = d.scons_build_arrays(a, read_off=None)
    check(st, d.scons_fetch(), written(d, tmp_path, "later"), want, name + " dense")
    if npairs < 3: return
    # small ranges of pairs
    monkeypatch.setenv("DFK_PIDX_RANGE_PAIRS", str(max(1, want["rows"] // 5)))
    st = d.scons_build_arrays(a, 37)
    check(st, d.scons_fetch(), None, want, name + " in small ranges")
    assert st["ranges"] >= 3
    monkeypatch.setenv("DFK_PIDX_RANGE_PAIRS", "1")                             # a range a yielding pair
    st = d.scons_build_arrays(a)
    check(st, d.scons_fetch(), None, want, name + " a pair a range")
    assert want["yields"] <= st["ranges"] <= npairs


def test_arrays_refusals(ctx, tmp_path):
    from superplus_amd.dfk import DfkError
    d = ctx
    name, c = SEEDED[0]
    want = scons_cases.oracle(name, c)
    a = scons_cases.arrays(c)
    st = d.scons_build_arrays(a)
    fell = a["read_off"].copy(); fell[3] = fell[2] - 1
    qfell = a["pq_off"].copy(); qfell[3] = qfell[2] - 1
    sfell = a["starts"].copy(); sfell[1] = sfell[2] + 1
    shifted = a["starts"].copy(); shifted[1] -= 1                                # walk 0 one record short of its `placed`, walk 1 one over
    wide = a["records"].copy(); wide[0, 6] += 1                                  # M is not what the records reach
    far = a["placed"].copy(); far["id"][0] = len(a["read_len"])
    neg = a["placed"].copy(); neg["id"][0] = -1
    away = a["placed"].copy(); away["start"][0] = 1 << 30
    row0 = int(a["placed"]["id"][0])
    short = a["read_len"].copy(); short[row0] += 1                               # its stream is now one value short
    packed1, off1 = a["read_packed"], a["read_off"]
    if a["read_len"][row0] % 4 == 0:                                            # (the base needs a byte of its own)
        packed1 = np.insert(packed1, int(off1[row0 + 1]), 0); off1 = off1.copy(); off1[row0 + 1:] += 1
    wide_short = a["records"].copy(); wide_short[0, 6] += 1                      # (M follows the longer read, so that the stream is what refuses)
    for code, change in ((-1, dict(starts=None)), (-1, dict(records=None)), (-1, dict(placed=None)), (-1, dict(read_len=None)), (-1, dict(pq=None)), (-1, dict(pq_off=None)), (-1, dict(read_packed=None)),
                         (-1, dict(starts=sfell)), (-1, dict(starts=shifted)), (-1, dict(records=wide)), (-1, dict(placed=far)), (-1, dict(placed=neg)), (-1, dict(placed=away)),
                         (-5, dict(read_off=fell)), (-5, dict(pq_off=qfell)), (-5, dict(read_len=short, read_packed=packed1, read_off=off1, records=wide_short))):      # DFK_E_INPUT
        held = d.stats()["hbm_held"]
        with pytest.raises(DfkError) as e:
            d.scons_build_arrays(a, 0, str(tmp_path), **change)
            print("not refused:", list(change))
        assert e.value.code == code, (change.keys(), e.value)
        assert d.stats()["hbm_held"] == held and not os.listdir(tmp_path)
        check(d.scons_stats(), d.scons_fetch(), None, want, "the earlier result")       # ... is still served
    # the next good call after them
    st2 = d.scons_build_arrays(a, 37)
    check(st2, d.scons_fetch(), None, want, "after the refusals")
    same = lambda x: {k: v for k, v in x.items() if not k.startswith("us") and k not in ("batches", "decoded")}       # (a read is decoded once a batch)
    assert same(st) == same(st2)


# ---- 2. the fixtures, through the chain dfk_count ... dfk_closer_build -> dfk_walks_build -> dfk_scons_build
@pytest.mark.parametrize("case,K,which", FIXTURES, ids=[f[0] for f in FIXTURES])
def test_scons_file_and_counters_match_the_oracle_on_the_fixtures(golden_dir, tmp_path, case, K, which):
    from superplus_amd.dfk import DfkError
    want = scons_oracle.fixture_scons(golden_dir, case, K, which)
    assert want["yields"] > 0
    i = walks_oracle.fixture_inputs(golden_dir, case, K, which)
    rs = i["rs"]
    reads = tuple(rs[k] for k in READS)
    d = pathed(rs, case, K, tmp_path)
    d.hops_build(hops_inputs(golden_dir, case, K, which)["bc"])
    d.closer_build(closer_oracle.fixture_inputs(golden_dir, case, K, which)["dup"])
    with pytest.raises(DfkError, match="dfk_walks_build") as e:
        d.scons_build(*reads)
    assert e.value.code == -6                                                    # DFK_E_STATE: no walks yet
    d.walks_build(None, *reads)
    held = d.stats()["hbm_held"]
    st = d.scons_build(*reads)
    assert d.stats()["hbm_held"] == held
    check(st, d.scons_fetch(), written(d, tmp_path), want, case)
    assert st["ranges"] == 1 and st["batches"] == 1
    if case == "graph_pathy_k48":
        # the reads dense; other reads than the walks were made from are refused, the result stays
        st2 = d.scons_build(rs["packed"], None, rs["read_len"], rs["pq_bytes"], rs["pq_off"])
        check(st2, d.scons_fetch(), written(d, tmp_path, "dense"), want, case + " (dense)")
        with pytest.raises(DfkError) as e:
            d.scons_build(rs["packed"], rs["base_off"][:-2], rs["read_len"][:-2], rs["pq_bytes"], rs["pq_off"][:-2])
        assert e.value.code == -1
        check(d.scons_stats(), d.scons_fetch(), None, want, "after a refused call")
    d.close()


# ---- 3. DF
def test_df_writes_the_scons_file(tmp_path, golden_dir):
    case, K, which = FIXTURES[0]
    want = scons_oracle.fixture_scons(golden_dir, case, K, which)              # ONE_GOOD off, as the table was made
    r = run_df(tmp_path, golden_dir, which, "HOPS=True", "ONE_GOOD=False", "CLOSER=True", "WALKS=True", "SCONS=True")
    assert r.returncode == 0, r.stdout + r.stderr
    w = f"{tmp_path}/GapToy/1/a.48"
    assert open(f"{w}/{FILE}", "rb").read() == want["file"]
    assert open(f"{w}/{walks_oracle.FILE}", "rb").read() == walks_oracle.fixture_walks(golden_dir, case, K, which)["file"]
    for f in sorted(os.listdir(f"{golden_dir}/{case}")):                       # everything else DF writes there is still the fixture's
        if f.startswith("a."):
            assert open(f"{w}/{f}", "rb").read() == open(f"{golden_dir}/{case}/{f}", "rb").read(), f
    lines = [l for l in r.stdout.splitlines() if l.startswith("DF_SCONS ")]
    assert lines == ['DF_SCONS {"pairs": %d, "yields": %d, "stacks": %d, "rows": %d, "rows_kept": %d, "trimmed": %d, "columns": %d, "a.stack.cons": "%016x%016x", "cells": %d, "capped": %d, '
                     '"recount": %d, "flat": %d, "allowed": %d, "disallowed": %d, "batches": 1, "ranges": 1}'
                     % (want["pairs"], want["yields"], want["stacks"], want["rows"], want["rows_kept"], want["trimmed"], want["columns"], *want["digest"], want["cells"], want["capped"],
                        want["recount"], want["flat"], want["allowed"], want["disallowed"])], lines
    assert r.stdout.index("DF_WALKS ") < r.stdout.index("DF_SCONS ")


def test_df_refuses_scons_without_the_walks_and_on_a_sharded_run(tmp_path, golden_dir):
    r = run_df(tmp_path, golden_dir, "frag", "HOPS=True", "CLOSER=True", "SCONS=True")
    assert r.returncode != 0 and "SCONS=True needs WALKS=True" in r.stdout
    assert not os.path.exists(f"{tmp_path}/GapToy")
    env = dict(os.environ)
    env["DF_FORCE_SHARDED"] = "1"
    r = run_df(tmp_path, golden_dir, "frag", "HOPS=True", "CLOSER=True", "WALKS=True", "SCONS=True", env=env)
    assert r.returncode != 0 and "runs on one GPU only" in r.stdout
    assert not os.path.exists(f"{tmp_path}/GapToy")


def test_df_without_the_switch_writes_and_prints_what_it_did(tmp_path, golden_dir):
    """SCONS=False against the argument absent: the same listing, the same a.close.* and a.stack.* bytes, the same DF_ lines"""
    runs = []
    for sub, extra in (("absent", []), ("off", ["SCONS=False"])):
        root = os.path.join(tmp_path, sub)
        os.makedirs(root)
        r = run_df(root, golden_dir, "frag", "HOPS=True", "CLOSER=True", "WALKS=True", *extra)
        assert r.returncode == 0, r.stdout + r.stderr
        w = f"{root}/GapToy/1/a.48"
        assert not os.path.exists(f"{w}/{FILE}") and "DF_SCONS" not in r.stdout and "a.stack.cons" not in r.stdout
        runs.append((sorted(os.listdir(w)), {f: open(f"{w}/{f}", "rb").read() for f in os.listdir(w) if f.startswith(("a.close", "a.stack"))},
                     [l.split(" ")[0] for l in r.stdout.splitlines() if l.startswith("DF_")],
                     [l for l in r.stdout.splitlines() if l.startswith(("DF_CLOSER ", "DF_HOPS ", "DF_DIGESTS "))]))
    assert runs[0] == runs[1] and "a.stack.walks" in runs[0][0]
