"""Stackster's stack offsets per pair on the GPU (dfk_soffsets_build / _write: the live rows of a range of pairs from the walks' placed
records, the reads of a batch of pairs gathered once each, decoded and lowered, the search a workgroup a pair and a wave a row, the
records scanned and emitted) against tests/soffsets_oracle.py: the starts, the per-pair words, the records with best_bits as its raw 8
bytes, the states, the file a.stack.offsets byte for byte, the counters and the digest -- on every seeded case of
tests/soffsets_cases.py with rows_per_batch 1, 37 and 0 and in small ranges; on five fixtures after a real dfk_count ...
dfk_walks_build, dfk_scons_build; each refusal with the next good call behind it; `DF HOPS=True CLOSER=True WALKS=True SCONS=True
SOFFSETS=True`.  Everything is exact.

The rule is pinned by the two restatements only (tests/soffsets_oracle.py, superplus_amd/csrc/dfk_soffsets.h); the walks and the stack
consensus the device works on are those tests/test_gpu_walks.py and tests/test_gpu_scons.py hold to their oracles.  graph_pathy2_k48
stays with the CPU tests."""
import os

import numpy as np
import pytest

from tests import closer_oracle, scons_oracle, soffsets_cases, soffsets_oracle, walks_oracle
from tests.test_gpu_hops import pathed, run_df
from tests.test_hops_oracle import fixture_inputs as hops_inputs

pytestmark = pytest.mark.gpu

FILE = soffsets_oracle.FILE
COUNTERS = ("pairs", "yields", "rows", "kmers", "acceptable", "hits", "seen", "disallowed", "lookups", "results", "offsets", "kept", "dropped", "pairs_0", "pairs_1", "pairs_2", "pairs_3", "pairs_more", "closable")
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
    assert [int(x) for x in got["starts"]] == want["starts"], f"{what}: starts"
    assert [tuple(int(x) for x in w) for w in got["words"]] == want["words"], f"{what}: the per-pair words"
    assert got["records"].tobytes() == soffsets_oracle.record_bytes(want["records"]), f"{what}: the records ({len(got['records'])}, {len(want['records'])} expected)"
    assert tuple(st[k] for k in COUNTERS) == tuple(want[k] for k in COUNTERS), f"{what}: {[(k, st[k], want[k]) for k in COUNTERS if st[k] != want[k]]}"
    assert (st["sum"], st["xor"]) == want["digest"], f"{what}: the digest"
    if file is not None: assert file == want["file"], f"{what}: {FILE} differs ({len(file)} bytes, {len(want['file'])} expected)"


def written(d, tmp_path, sub="out"):
    out = os.path.join(tmp_path, sub)
    os.makedirs(out, exist_ok=True)
    held = d.stats()["hbm_held"]
    d.soffsets_write(out)
    assert d.stats()["hbm_held"] == held and os.listdir(out) == [FILE]
    return open(os.path.join(out, FILE), "rb").read()


# ---- 1. the seeded cases
@pytest.fixture(scope="module")
def ctx():
    from superplus_amd.dfk import Dfk
    d = Dfk(K=soffsets_cases.K)
    yield d
    d.close()


SEEDED = soffsets_cases.seeded()


@pytest.mark.parametrize("name,c", SEEDED, ids=[n for n, _ in SEEDED])
def test_seeded_arrays_match_the_oracle(ctx, tmp_path, monkeypatch, name, c):
    d = ctx
    want = soffsets_cases.oracle(name, c)[1]
    a = soffsets_cases.arrays(name, c)
    npairs = want["pairs"]
    batches = {}
    for per in (1, 37, 0):
        out = os.path.join(tmp_path, f"per{per}")
        os.makedirs(out)
        held = d.stats()["hbm_held"]
        st = d.soffsets_build_arrays(a, per, out)
        assert d.stats()["hbm_held"] == held
        check(st, d.soffsets_fetch(), open(os.path.join(out, FILE), "rb").read(), want, f"{name} rows_per_batch={per}")
        assert st["ranges"] == (1 if npairs else 0) and os.listdir(out) == [FILE]
        batches[per] = st["batches"]
    assert batches[0] == (1 if npairs else 0) and batches[1] >= batches[37] >= batches[0] and want["yields"] <= batches[1] <= npairs
    if name == "planted": assert batches[37] > 1                                # (ROWS600 alone is a batch of 601 rows: a pair is never split)
    # dense reads (the cases' are), no directory: the same result, no file; dfk_soffsets_write then writes the same
    st = d.soffsets_build_arrays(a, read_off=None)
    check(st, d.soffsets_fetch(), written(d, tmp_path, "later"), want, name + " dense")
    if npairs < 3: return
    # small ranges of pairs
    monkeypatch.setenv("DFK_PIDX_RANGE_PAIRS", str(max(1, want["rows"] // 5)))
    st = d.soffsets_build_arrays(a, 37)
    check(st, d.soffsets_fetch(), None, want, name + " in small ranges")
    assert st["ranges"] >= 3
    monkeypatch.setenv("DFK_PIDX_RANGE_PAIRS", "1")                             # a range a yielding pair
    st = d.soffsets_build_arrays(a)
    check(st, d.soffsets_fetch(), None, want, name + " a pair a range")
    assert want["yields"] <= st["ranges"] <= npairs


def test_arrays_refusals(ctx, tmp_path):
    from superplus_amd.dfk import DfkError
    d = ctx
    name, c = SEEDED[0]
    want = soffsets_cases.oracle(name, c)[1]
    a = soffsets_cases.arrays(name, c)
    st = d.soffsets_build_arrays(a)
    y = 2 * c["names"]["ZERO"]                                                   # a yielding pair's first element, columns and counts in front of it
    sfell = a["starts"].copy(); sfell[1] = sfell[2] + 1
    from1 = a["cons_starts"].copy(); from1[0] = 1
    cfell = a["cons_starts"].copy(); cfell[y + 1] = cfell[y] - 1
    kfell = a["conflict_first"].copy(); kfell[y // 2 + 1] = kfell[y // 2] - 1
    base4 = a["con"].copy(); base4[int(a["cons_starts"][y])] = 4
    i400 = 2 * c["names"]["W400"]                                                # an element 401 wide: its neighbour gives a column
    wide = a["cons_starts"].copy(); wide[i400 + 1] += 1
    wide_dims = a["dims"].copy(); wide_dims[i400, 3] += 1; wide_dims[i400 + 1, 3] -= 1
    dims1 = a["dims"].copy(); dims1[y, 3] += 1                                   # dims that do not say what the starts do
    short = a["conflict_first"].copy(); short[y // 2 + 1:] -= 1                  # a counts table one short of n1 + n2
    extra = a["conflict_first"].copy(); extra[c["names"]["NONE1"] + 1:] += 1     # ... and one for a pair that does not yield
    more = np.concatenate([a["counts"], np.zeros(1, np.uint16)])
    wideM = a["records"].copy(); wideM[y, 6] += 1                                # M is not what the records reach
    far = a["placed"].copy(); far["id"][0] = len(a["read_len"])
    qfell = a["pq_off"].copy(); qfell[3] = qfell[2] - 1
    for code, change in ((-1, dict(starts=None)), (-1, dict(records=None)), (-1, dict(placed=None)), (-1, dict(read_len=None)), (-1, dict(pq=None)), (-1, dict(cons_starts=None)), (-1, dict(dims=None)),
                         (-1, dict(con=None)), (-1, dict(conq=None)), (-1, dict(conflict_first=None)), (-1, dict(counts=None)),
                         (-1, dict(starts=sfell)), (-1, dict(cons_starts=from1)), (-1, dict(cons_starts=cfell)), (-1, dict(conflict_first=kfell)), (-1, dict(con=base4)), (-1, dict(cons_starts=wide, dims=wide_dims)),
                         (-1, dict(dims=dims1)), (-1, dict(conflict_first=short)), (-1, dict(conflict_first=extra, counts=more)), (-1, dict(records=wideM)), (-1, dict(placed=far)),
                         (-5, dict(pq_off=qfell))):                                                     # DFK_E_INPUT
        held = d.stats()["hbm_held"]
        with pytest.raises(DfkError) as e:
            d.soffsets_build_arrays(a, 0, str(tmp_path), **change)
            print("not refused:", list(change))
        assert e.value.code == code, (change.keys(), e.value)
        assert d.stats()["hbm_held"] == held and not os.listdir(tmp_path)
        check(d.soffsets_stats(), d.soffsets_fetch(), None, want, "the earlier result")       # ... is still served
    # the next good call after them
    st2 = d.soffsets_build_arrays(a, 37)
    check(st2, d.soffsets_fetch(), None, want, "after the refusals")
    same = lambda x: {k: v for k, v in x.items() if not k.startswith("us") and k not in ("batches", "decoded")}       # (a read is decoded once a batch)
    assert same(st) == same(st2)


# ---- 2. the fixtures, through the chain dfk_count ... dfk_walks_build -> dfk_scons_build -> dfk_soffsets_build
@pytest.mark.parametrize("case,K,which", FIXTURES, ids=[f[0] for f in FIXTURES])
def test_soffsets_file_and_counters_match_the_oracle_on_the_fixtures(golden_dir, tmp_path, case, K, which):
    from superplus_amd.dfk import DfkError
    want = soffsets_oracle.fixture_soffsets(golden_dir, case, K, which)
    assert want["yields"] > 0 and want["seen"] > 0
    i = walks_oracle.fixture_inputs(golden_dir, case, K, which)
    rs = i["rs"]
    reads = tuple(rs[k] for k in READS)
    d = pathed(rs, case, K, tmp_path)
    d.hops_build(hops_inputs(golden_dir, case, K, which)["bc"])
    d.closer_build(closer_oracle.fixture_inputs(golden_dir, case, K, which)["dup"])
    with pytest.raises(DfkError, match="dfk_walks_build") as e:
        d.soffsets_build(*reads)
    assert e.value.code == -6                                                    # DFK_E_STATE: no walks yet
    d.walks_build(None, *reads)
    with pytest.raises(DfkError, match="dfk_scons_build") as e:
        d.soffsets_build(*reads)
    assert e.value.code == -6                                                    # DFK_E_STATE: no stack consensus yet
    d.scons_build(*reads)
    held = d.stats()["hbm_held"]
    st = d.soffsets_build(*reads)
    assert d.stats()["hbm_held"] == held
    check(st, d.soffsets_fetch(), written(d, tmp_path), want, case)
    assert st["ranges"] == 1 and st["batches"] == 1
    if case == "graph_pathy_k48":
        # the reads dense; other reads than the walks were made from are refused, the result stays
        st2 = d.soffsets_build(rs["packed"], None, rs["read_len"], rs["pq_bytes"], rs["pq_off"])
        check(st2, d.soffsets_fetch(), written(d, tmp_path, "dense"), want, case + " (dense)")
        with pytest.raises(DfkError) as e:
            d.soffsets_build(rs["packed"], rs["base_off"][:-2], rs["read_len"][:-2], rs["pq_bytes"], rs["pq_off"][:-2])
        assert e.value.code == -1
        check(d.soffsets_stats(), d.soffsets_fetch(), None, want, "after a refused call")
        # new walks: the consensus is no longer theirs; a consensus from arrays is nobody's
        d.walks_build(None, *reads)
        with pytest.raises(DfkError, match="other walks") as e:
            d.soffsets_build(*reads)
        assert e.value.code == -6
        check(d.soffsets_stats(), d.soffsets_fetch(), None, want, "after a call refused for its state")
        d.scons_build(*reads)
        check(d.soffsets_build(*reads), d.soffsets_fetch(), None, want, case + " (again)")
    d.close()


# ---- 3. DF
def test_df_writes_the_soffsets_file(tmp_path, golden_dir):
    case, K, which = FIXTURES[0]
    want = soffsets_oracle.fixture_soffsets(golden_dir, case, K, which)        # ONE_GOOD off, as the table was made
    r = run_df(tmp_path, golden_dir, which, "HOPS=True", "ONE_GOOD=False", "CLOSER=True", "WALKS=True", "SCONS=True", "SOFFSETS=True")
    assert r.returncode == 0, r.stdout + r.stderr
    w = f"{tmp_path}/GapToy/1/a.48"
    assert open(f"{w}/{FILE}", "rb").read() == want["file"]
    assert open(f"{w}/{scons_oracle.FILE}", "rb").read() == scons_oracle.fixture_scons(golden_dir, case, K, which)["file"]
    for f in sorted(os.listdir(f"{golden_dir}/{case}")):                       # everything else DF writes there is still the fixture's
        if f.startswith("a."):
            assert open(f"{w}/{f}", "rb").read() == open(f"{golden_dir}/{case}/{f}", "rb").read(), f
    lines = [l for l in r.stdout.splitlines() if l.startswith("DF_SOFFSETS ")]
    assert lines == ['DF_SOFFSETS {"pairs": %d, "yields": %d, "rows": %d, "kmers": %d, "acceptable": %d, "hits": %d, "seen": %d, "disallowed": %d, "lookups": %d, "results": %d, "offsets": %d, "kept": %d, '
                     '"dropped": %d, "pairs_0": %d, "pairs_1": %d, "pairs_2": %d, "pairs_3": %d, "pairs_more": %d, "closable": %d, "a.stack.offsets": "%016x%016x", "batches": 1, "ranges": 1}'
                     % (*(want[k] for k in COUNTERS), *want["digest"])], lines
    assert r.stdout.index("DF_SCONS ") < r.stdout.index("DF_SOFFSETS ")


def test_df_refuses_soffsets_without_the_stack_consensus(tmp_path, golden_dir):
    r = run_df(tmp_path, golden_dir, "frag", "HOPS=True", "CLOSER=True", "WALKS=True", "SOFFSETS=True")
    assert r.returncode != 0 and "SOFFSETS=True needs SCONS=True" in r.stdout
    assert not os.path.exists(f"{tmp_path}/GapToy")


def test_df_without_the_switch_writes_and_prints_what_it_did(tmp_path, golden_dir):
    """SOFFSETS=False against the argument absent: the same listing, the same a.close.* and a.stack.* bytes, the same DF_ lines"""
    runs = []
    for sub, extra in (("absent", []), ("off", ["SOFFSETS=False"])):
        root = os.path.join(tmp_path, sub)
        os.makedirs(root)
        r = run_df(root, golden_dir, "frag", "HOPS=True", "CLOSER=True", "WALKS=True", "SCONS=True", *extra)
        assert r.returncode == 0, r.stdout + r.stderr
        w = f"{root}/GapToy/1/a.48"
        assert not os.path.exists(f"{w}/{FILE}") and "DF_SOFFSETS" not in r.stdout and "a.stack.offsets" not in r.stdout
        runs.append((sorted(os.listdir(w)), {f: open(f"{w}/{f}", "rb").read() for f in os.listdir(w) if f.startswith(("a.close", "a.stack"))},
                     [l.split(" ")[0] for l in r.stdout.splitlines() if l.startswith("DF_")],
                     [l for l in r.stdout.splitlines() if l.startswith(("DF_CLOSER ", "DF_HOPS ", "DF_DIGESTS "))]))
    assert runs[0] == runs[1] and "a.stack.cons" in runs[0][0]
