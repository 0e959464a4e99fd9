"""Stackster's closures per pair on the GPU (dfk_sclosures_build / _write: the closable pairs' stacks alone, the reads of a batch of
closures gathered once each, decoded and lowered, the merged consensus a workgroup a tile of 256 merged columns with the rows a tile
misses skipped, the flags counted per closure and side) against tests/sclosures_oracle.py: pair_first, the starts, the records, the
bases, the file a.stack.closures byte for byte, the counters and the digest -- on every seeded case of tests/sclosures_cases.py with
closures_per_batch 1, 37 and 0, dense reads, small ranges and a pair a range; each refusal with the earlier result still served and the
next good call behind it; on five fixtures after a real dfk_count ... dfk_walks_build, dfk_scons_build, dfk_soffsets_build; `DF ...
SOFFSETS=True SCLOSURES=True`; the combined list a.closures.fastb of both closers.  Everything is exact.

The rule is pinned by the two restatements only (tests/sclosures_oracle.py, superplus_amd/csrc/dfk_sclosures.h); the walks, the stack
consensus and the offsets the device works on are those tests/test_gpu_walks.py, tests/test_gpu_scons.py and tests/test_gpu_soffsets.py
hold to their oracles.  graph_pathy2_k48 stays with the CPU tests."""
import os

import numpy as np
import pytest

from tests import closer_oracle, sclosures_cases, sclosures_oracle, soffsets_oracle, walks_oracle
from tests.test_gpu_hops import pathed, run_df
from tests.test_hops_oracle import fixture_inputs as hops_inputs

pytestmark = pytest.mark.gpu

FILE = sclosures_oracle.FILE
COUNTERS = ("pairs", "yields", "closable", "none", "over", "closures", "columns", "cells", "live", "erased", "empty", "short", "rowless")
WANT = ("pairs", "yields", "closable", "none", "over", "closures", "columns", "added", "live", "erased", "empty", "short", "rowless")
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
    assert [int(x) for x in got["pair_first"]] == want["pair_first"], f"{what}: pair_first"
    assert [int(x) for x in got["starts"]] == want["starts"], f"{what}: starts"
    assert [tuple(int(x) for x in r) for r in got["records"]] == want["records"], f"{what}: the records"
    assert got["bases"].tobytes() == bytes(want["bases"]), f"{what}: the bases"
    assert tuple(st[k] for k in COUNTERS) == tuple(want[k] for k in WANT), f"{what}: {[(k, st[k], want[w]) for k, w in zip(COUNTERS, WANT) if st[k] != want[w]]}"
    assert (st["sum"], st["xor"]) == want["digest"], f"{what}: the digest"
    assert st["skipped"] <= st["visits"] and st["live"] <= st["visits"] <= 4 * st["live"], f"{what}: the tile visits"
    if file is not None: assert file == want["file"], f"{what}: {FILE} differs ({len(file)} bytes, {len(want['file'])} expected)"


def written(d, tmp_path, sub="out"):
    out = os.path.join(tmp_path, sub)
    os.makedirs(out, exist_ok=True)
    held = d.stats()["hbm_held"]
    d.sclosures_write(out)
    assert d.stats()["hbm_held"] == held and os.listdir(out) == [FILE]
    return open(os.path.join(out, FILE), "rb").read()


# ---- 1. the seeded cases
@pytest.fixture(scope="module")
def ctx():
    from superplus_amd.dfk import Dfk
    d = Dfk(K=sclosures_cases.K)
    yield d
    d.close()


SEEDED = sclosures_cases.seeded()


@pytest.mark.parametrize("name,c", SEEDED, ids=[n for n, _ in SEEDED])
def test_seeded_arrays_match_the_oracle(ctx, tmp_path, monkeypatch, name, c):
    d = ctx
    want = sclosures_cases.oracle(name, c)[1]
    a = sclosures_cases.arrays(name, c)
    n = want["closures"]
    batches = {}
    for per in (1, 37, 0):
        out = os.path.join(tmp_path, f"per{per}")
        os.makedirs(out)
        held = d.stats()["hbm_held"]
        st = d.sclosures_build_arrays(a, per, out)
        assert d.stats()["hbm_held"] == held
        check(st, d.sclosures_fetch(), open(os.path.join(out, FILE), "rb").read(), want, f"{name} closures_per_batch={per}")
        assert st["ranges"] == (1 if n else 0) and os.listdir(out) == [FILE]
        batches[per] = st["batches"]
    assert batches[0] == (1 if n else 0) and batches[1] == n and batches[37] == (n + 36) // 37      # (two closures of one pair in two batches: the pair's reads go up twice)
    if name == "planted":
        assert 0 < st["skipped"] < st["visits"] and st["rowless"] == 1          # SKIPALL, C792 and W460: rows that miss a tile
    # dense reads (the cases' are), no directory: the same result, no file; dfk_sclosures_write then writes the same
    st = d.sclosures_build_arrays(a, read_off=None)
    check(st, d.sclosures_fetch(), written(d, tmp_path, "later"), want, name + " dense")
    if want["closable"] < 3: return
    # small ranges of closable pairs
    rows = [c["recs"][2 * pi]["placed"] + c["recs"][2 * pi + 1]["placed"] for pi, cl in enumerate(want["per"]) if cl]      # a range holds whole closable pairs, by their rows
    monkeypatch.setenv("DFK_PIDX_RANGE_PAIRS", str(max(1, sum(rows) // 5)))
    st = d.sclosures_build_arrays(a, 37)
    check(st, d.sclosures_fetch(), None, want, name + " in small ranges")
    assert 2 <= st["ranges"] <= want["closable"]                                # (one pair may hold most of the rows: ROWS600)
    monkeypatch.setenv("DFK_PIDX_RANGE_PAIRS", "1")                             # a range a closable pair
    st = d.sclosures_build_arrays(a)
    check(st, d.sclosures_fetch(), None, want, name + " a pair a range")
    assert st["ranges"] == want["closable"] == st["batches"]


def test_arrays_refusals(ctx, tmp_path):
    from superplus_amd.dfk import DfkError
    d = ctx
    name, c = SEEDED[0]
    want = sclosures_cases.oracle(name, c)[1]
    a = sclosures_cases.arrays(name, c)
    st = d.sclosures_build_arrays(a)
    names = c["names"]
    at = lambda n: int(a["so_starts"][names[n]])                                 # a plant's first record
    n1, n2 = (int(a["dims"][2 * names["POS"] + s, 3]) for s in (0, 1))
    sfell = a["starts"].copy(); sfell[1] = sfell[2] + 1
    ofell = a["so_starts"].copy(); ofell[names["TWO"] + 1] = ofell[names["TWO"]] - 1
    from1 = a["so_starts"].copy(); from1[0] = 1
    state2 = a["so_records"].copy(); state2["state"][at("POS")] = 2
    unsorted_ = a["so_records"].copy(); unsorted_["offset"][at("TWO") + 1] = unsorted_["offset"][at("TWO")]
    above = a["so_records"].copy(); above["offset"][at("POS")] = n1 - 7
    below = a["so_records"].copy(); below["offset"][at("POS")] = -(n2 - 7)
    extra = a["so_starts"].copy(); extra[names["NONE1"] + 1:] += 1               # a record for a pair that does not yield
    more = np.insert(a["so_records"], at("NONE1"), a["so_records"][0])
    kept1 = a["so_words"].copy(); kept1[names["TWO"], 2] = 1
    closable0 = a["so_words"].copy(); closable0[names["POS"], 3] = 0
    closable1 = a["so_words"].copy(); closable1[names["FOUR"], 3] = 1
    dims1 = a["dims"].copy(); dims1[2 * names["POS"], 3] += 1                    # dims that do not say what the walks do
    kept0 = a["dims"].copy(); kept0[2 * names["POS"], 1] -= 1
    wideM = a["records"].copy(); wideM[2 * names["POS"], 6] += 1                 # M is not what the records reach
    far = a["placed"].copy(); far["id"][0] = len(a["read_len"])
    qfell = a["pq_off"].copy(); qfell[3] = qfell[2] - 1
    for code, change in ((-1, dict(starts=None)), (-1, dict(records=None)), (-1, dict(placed=None)), (-1, dict(read_len=None)), (-1, dict(pq=None)), (-1, dict(dims=None)), (-1, dict(so_starts=None)),
                         (-1, dict(so_words=None)), (-1, dict(so_records=None)),
                         (-1, dict(starts=sfell)), (-1, dict(so_starts=ofell)), (-1, dict(so_starts=from1)), (-1, dict(so_records=state2)), (-1, dict(so_records=unsorted_)), (-1, dict(so_records=above)),
                         (-1, dict(so_records=below)), (-1, dict(so_starts=extra, so_records=more)), (-1, dict(so_words=kept1)), (-1, dict(so_words=closable0)), (-1, dict(so_words=closable1)),
                         (-1, dict(dims=dims1)), (-1, dict(dims=kept0)), (-1, dict(records=wideM)), (-1, dict(placed=far)),
                         (-5, dict(pq_off=qfell))):                                                     # DFK_E_INPUT
        held = d.stats()["hbm_held"]
        with pytest.raises(DfkError) as e:
            d.sclosures_build_arrays(a, 0, str(tmp_path), **change)
            print("not refused:", list(change))
        assert e.value.code == code, (change.keys(), e.value)
        assert d.stats()["hbm_held"] == held and not os.listdir(tmp_path)
        check(d.sclosures_stats(), d.sclosures_fetch(), None, want, "the earlier result")      # ... is still served
    # the ends of the allowed range are taken
    ends = a["so_records"].copy(); ends["offset"][at("POS")] = n1 - 8
    assert d.sclosures_build_arrays(a, so_records=ends)["closures"] == want["closures"]
    ends["offset"][at("POS")] = -(n2 - 8)
    assert d.sclosures_build_arrays(a, so_records=ends)["closures"] == want["closures"]
    # the next good call after them
    st2 = d.sclosures_build_arrays(a, 37)
    check(st2, d.sclosures_fetch(), None, want, "after the refusals")
    same = lambda x: {k: v for k, v in x.items() if not k.startswith("us") and k not in ("batches", "decoded")}       # (a read is decoded once a batch)
    assert same(st) == same(st2)


# ---- 2. the fixtures, through the chain dfk_count ... dfk_walks_build -> dfk_scons_build -> dfk_soffsets_build -> dfk_sclosures_build
@pytest.mark.parametrize("case,K,which", FIXTURES, ids=[f[0] for f in FIXTURES])
def test_sclosures_file_and_counters_match_the_oracle_on_the_fixtures(golden_dir, tmp_path, case, K, which):
    from superplus_amd.dfk import DfkError
    want = sclosures_oracle.fixture_sclosures(golden_dir, case, K, which)
    i = walks_oracle.fixture_inputs(golden_dir, case, K, which)
    rs = i["rs"]
    reads = tuple(rs[k] for k in READS)
    d = pathed(rs, case, K, tmp_path)
    d.hops_build(hops_inputs(golden_dir, case, K, which)["bc"])
    d.closer_build(closer_oracle.fixture_inputs(golden_dir, case, K, which)["dup"])
    d.walks_build(None, *reads)
    d.scons_build(*reads)

    def refused(match):
        held = d.stats()["hbm_held"]
        with pytest.raises(DfkError, match=match) as e:
            d.sclosures_build(*reads)
        assert e.value.code == -6 and d.stats()["hbm_held"] == held             # DFK_E_STATE
    refused("dfk_soffsets_build")                                                # no offsets yet
    d.soffsets_build(*reads)
    held = d.stats()["hbm_held"]
    st = d.sclosures_build(*reads)
    assert d.stats()["hbm_held"] == held
    check(st, d.sclosures_fetch(), written(d, tmp_path), want, case)
    assert st["ranges"] == st["batches"] == (1 if want["closures"] else 0)
    if case == "graph_pathy_k48":
        # the reads dense; other reads than the walks were made from are refused, the result stays
        st2 = d.sclosures_build(rs["packed"], None, rs["read_len"], rs["pq_bytes"], rs["pq_off"])
        check(st2, d.sclosures_fetch(), written(d, tmp_path, "dense"), want, case + " (dense)")
        with pytest.raises(DfkError) as e:
            d.sclosures_build(rs["packed"], rs["base_off"][:-2], rs["read_len"][:-2], rs["pq_bytes"], rs["pq_off"][:-2])
        assert e.value.code == -1
        check(d.sclosures_stats(), d.sclosures_fetch(), None, want, "after a refused call")
        # new walks and their consensus: the offsets are those of other walks
        d.walks_build(None, *reads)
        refused("other walks")
        d.scons_build(*reads)
        refused("of other walks")
        check(d.sclosures_stats(), d.sclosures_fetch(), None, want, "after a call refused for its state")
        d.soffsets_build(*reads)
        # a consensus made from arrays is the latest: the offsets are not its own
        from tests.test_scons_cpu import fixture_case
        from tests import scons_cases
        d.scons_build_arrays(scons_cases.arrays(fixture_case(golden_dir, case, K, which)))
        refused("dfk_scons_build_arrays")
        d.scons_build(*reads); d.soffsets_build(*reads)
        check(d.sclosures_build(*reads), d.sclosures_fetch(), None, want, case + " (again)")
    d.close()


# ---- 3. DF
DF_ARGS = ("HOPS=True", "ONE_GOOD=False", "CLOSER=True", "WALKS=True", "SCONS=True", "SOFFSETS=True")


def test_df_writes_the_sclosures_file(tmp_path, golden_dir):
    case, K, which = FIXTURES[0]
    want = sclosures_oracle.fixture_sclosures(golden_dir, case, K, which)      # ONE_GOOD off, as the table was made
    r = run_df(tmp_path, golden_dir, which, *DF_ARGS, "SCLOSURES=True")
    assert r.returncode == 0, r.stdout + r.stderr
    w = f"{tmp_path}/GapToy/1/a.48"
    assert open(f"{w}/{FILE}", "rb").read() == want["file"]
    assert open(f"{w}/{soffsets_oracle.FILE}", "rb").read() == soffsets_oracle.fixture_soffsets(golden_dir, case, K, which)["file"]
    for f in sorted(os.listdir(f"{golden_dir}/{case}")):                       # everything else DF writes there is still the fixture's
        if f.startswith("a."):
            assert open(f"{w}/{f}", "rb").read() == open(f"{golden_dir}/{case}/{f}", "rb").read(), f
    lines = [l for l in r.stdout.splitlines() if l.startswith("DF_SCLOSURES ")]
    assert lines == ['DF_SCLOSURES {"pairs": %d, "yields": %d, "closable": %d, "none": %d, "over": %d, "closures": %d, "columns": %d, "a.stack.closures": "%016x%016x", "cells": %d, "live_rows": %d, '
                     '"erased": %d, "empty": %d, "short": %d, "rowless": %d, "batches": 1, "ranges": 1}'
                     % (*(want[k] for k in WANT[:7]), *want["digest"], *(want[k] for k in WANT[7:]))], lines
    assert r.stdout.index("DF_SOFFSETS ") < r.stdout.index("DF_SCLOSURES ") and "a.closures.fastb" not in os.listdir(w) and "found " not in r.stdout


def test_df_refuses_sclosures_without_the_stack_offsets(tmp_path, golden_dir):
    r = run_df(tmp_path, golden_dir, "frag", "HOPS=True", "CLOSER=True", "WALKS=True", "SCONS=True", "SCLOSURES=True")
    assert r.returncode != 0 and "SCLOSURES=True needs SOFFSETS=True" in r.stdout
    assert not os.path.exists(f"{tmp_path}/GapToy")


def test_df_without_the_switch_writes_and_prints_what_it_did(tmp_path, golden_dir):
    """SCLOSURES=False against the argument absent: the same listing, the same a.close.* and a.stack.* bytes, the same DF_ lines"""
    runs = []
    for sub, extra in (("absent", []), ("off", ["SCLOSURES=False"])):
        root = os.path.join(tmp_path, sub)
        os.makedirs(root)
        r = run_df(root, golden_dir, "frag", "HOPS=True", "CLOSER=True", "WALKS=True", "SCONS=True", "SOFFSETS=True", *extra)
        assert r.returncode == 0, r.stdout + r.stderr
        w = f"{root}/GapToy/1/a.48"
        assert not os.path.exists(f"{w}/{FILE}") and "DF_SCLOSURES" not in r.stdout and "a.stack.closures" not in r.stdout and "found " not in r.stdout
        runs.append((sorted(os.listdir(w)), {f: open(f"{w}/{f}", "rb").read() for f in os.listdir(w) if f.startswith(("a.close", "a.stack"))},
                     [l.split(" ")[0] for l in r.stdout.splitlines() if l.startswith("DF_")],
                     [l for l in r.stdout.splitlines() if l.startswith(("DF_CLOSER ", "DF_HOPS ", "DF_DIGESTS ", "DF_SOFFSETS "))]))
    assert runs[0] == runs[1] and "a.stack.offsets" in runs[0][0]


# ---- 4. the combined list of both closers (RunStages.cc:290-325)
def interleaved(golden_dir, case, K, which):
    """per pair Stackster's closures, then CloseGap2's, the pairs in order -> [base arrays]"""
    from tests import closures_oracle
    s = sclosures_oracle.fixture_sclosures(golden_dir, case, K, which)
    g = closures_oracle.fixture_closures(golden_dir, case, K, which)
    assert len(s["per"]) == len(g["per"])
    out = []
    for a, b in zip(s["per"], g["per"]): out += [x["bases"] for x in a] + [x["bases"] for x in b]
    return out, s["closures"], g["closures"]


def fastb_sequences(path):
    from superplus_amd import feudal
    packed, off, rl = feudal.read_fastb(path)
    out = []
    for i, n in enumerate(rl):
        b = packed[int(off[i]):int(off[i + 1])]
        out.append(((b[np.arange(int(n)) >> 2] >> (2 * (np.arange(int(n)) & 3))) & 3).astype(np.uint8))
    return out


def same_sequences(got, want):
    return len(got) == len(want) and all(np.array_equal(a, b) for a, b in zip(got, want))


def test_the_combined_list_of_both_closers(golden_dir, tmp_path):
    from superplus_amd.dfk import ALLCLOSURES_FILE, DfkError
    from tests.test_gpu_cons import partnered
    case, K, which = FIXTURES[0]
    want, n_s, n_g = interleaved(golden_dir, case, K, which)
    assert n_s == 306 and n_g == 351
    d, rs, i = partnered(golden_dir, tmp_path, case, K, which)
    reads = tuple(rs[k] for k in READS)
    out = os.path.join(tmp_path, "all")
    os.makedirs(out)

    def refused(match):
        with pytest.raises(DfkError, match=match) as e:
            d.allclosures_write(out)
        assert e.value.code == -6 and not os.listdir(out)
    refused("dfk_sclosures_build")                                               # neither built
    d.cons_build(*reads); d.offsets_build(); d.closures_build(*reads)
    refused("dfk_sclosures_build")                                               # only the first closer's
    d.walks_build(None, *reads); d.scons_build(*reads); d.soffsets_build(*reads); d.sclosures_build(*reads)
    held = d.stats()["hbm_held"]
    got = d.allclosures_write(out)
    assert d.stats()["hbm_held"] == held and os.listdir(out) == [ALLCLOSURES_FILE]
    assert got == dict(closures=n_s + n_g, bases=sum(len(x) for x in want), stackster=n_s, closegap2=n_g)
    assert same_sequences(fastb_sequences(os.path.join(out, ALLCLOSURES_FILE)), want)
    d.close()
    # only Stackster's: the first closer's closures are missing
    d2 = pathed(rs, case, K, os.path.join(tmp_path, "second"))
    d2.hops_build(hops_inputs(golden_dir, case, K, which)["bc"])
    d2.closer_build(closer_oracle.fixture_inputs(golden_dir, case, K, which)["dup"])
    d2.walks_build(None, *reads); d2.scons_build(*reads); d2.soffsets_build(*reads); d2.sclosures_build(*reads)
    with pytest.raises(DfkError, match="dfk_closures_build") as e:
        d2.allclosures_write(out)
    assert e.value.code == -6
    d2.close()


def test_df_writes_the_combined_list(tmp_path, golden_dir):
    case, K, which = FIXTURES[0]
    want, n_s, n_g = interleaved(golden_dir, case, K, which)
    r = run_df(tmp_path, golden_dir, which, *DF_ARGS, "PARTNERS=True", "CONS=True", "OFFSETS=True", "CLOSURES=True", "SCLOSURES=True")
    assert r.returncode == 0, r.stdout + r.stderr
    w = f"{tmp_path}/GapToy/1/a.48"
    assert same_sequences(fastb_sequences(f"{w}/a.closures.fastb"), want)
    assert [l for l in r.stdout.splitlines() if l.startswith("found ")] == ["found %d closures" % (n_s + n_g)]
    assert open(f"{w}/{FILE}", "rb").read() == sclosures_oracle.fixture_sclosures(golden_dir, case, K, which)["file"]
