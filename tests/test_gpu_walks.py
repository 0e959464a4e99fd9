"""Stackster's two stack walks per pair on the GPU (dfk_walks_build / _write: the reads of a batch of pairs gathered once each, decoded and
lowered, per side the 48-mers hashed and sorted by (pair, hash), a wave a walk with verification of every hit and the live list in LDS)
against tests/walks_oracle.py: the records, the placed tables, the EE bases, the file a.stack.walks byte for byte, the counters and the
digest -- on every seeded case of tests/walks_cases.py in batches of 1, 37 and what fits, in small ranges, with the live list forced
small (the host route) and the hash cut to 8 bits (collisions at nearly every look-up); on five fixtures after a real dfk_count ...
dfk_closer_build; each refusal with the next good call behind it; `DF HOPS=True CLOSER=True WALKS=True`.  Everything is exact.

The rule is pinned by the two restatements only (tests/walks_oracle.py, superplus_amd/csrc/dfk_walks.h); the closer sets the device works
on are those tests/test_gpu_closer.py holds to its oracle.  graph_pathy2_k48 stays with the CPU tests."""
import os

import numpy as np
import pytest

from tests import closer_oracle, walks_cases, walks_oracle
from tests.test_gpu_hops import pathed, run_df
from tests.test_hops_oracle import fixture_inputs as hops_inputs

pytestmark = pytest.mark.gpu

FILE = walks_oracle.FILE
COUNTERS = ("pairs", "walks", "entries", "placed", "dup_steps", "steps", "past_edge", "side0_empty", "side1_empty", "short", "trimmed", "yields", "live_sum", "live_max", "longest")
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
    recs = want["recs"]
    assert [tuple(int(x) for x in r) for r in got["records"]] == [tuple(walks_oracle.record_words(r)) for r in recs], f"{what}: records"
    assert [int(x) for x in got["starts"]] == [0] + list(np.cumsum([r["placed"] for r in recs])), f"{what}: starts"
    assert [int(x) for x in got["ee_starts"]] == [0] + list(np.cumsum([r["nEE"] for r in recs])), f"{what}: ee_starts"
    assert [(int(p["id"]), int(p["start"]), bool(p["fw"])) for p in got["placed"]] == [l for r in recs for l in r["locs"]], f"{what}: placed records"
    assert [int(b) for b in got["bases"]] == [b for r in recs for b in r["EE"]], f"{what}: EE bases"
    assert st["ee"] == want["sum_ee"] and tuple(st[k] for k in COUNTERS) == tuple(want[k] for k in COUNTERS), f"{what}: {[(k, st[k], want[k]) for k in COUNTERS]}"
    assert (st["sum"], st["xor"]) == want["digest"], f"{what}: the digest"
    if file is not None: assert file == want["file"], f"{what}: {FILE} differs ({len(file)} bytes, {len(want['file'])} expected)"


def written(d, tmp_path, sub="out"):
    out = os.path.join(tmp_path, sub)
    os.makedirs(out, exist_ok=True)
    held = d.stats()["hbm_held"]
    d.walks_write(out)
    assert d.stats()["hbm_held"] == held and os.listdir(out) == [FILE]
    return open(os.path.join(out, FILE), "rb").read()


# ---- 1. the seeded cases
@pytest.fixture(scope="module")
def ctx():
    from superplus_amd.dfk import Dfk
    made = {}

    def of(K):
        if K not in made: made[K] = Dfk(K=K)
        return made[K]
    yield of
    for d in made.values(): d.close()


SEEDED = walks_cases.seeded()


@pytest.mark.parametrize("name,c", [(n, c) for n, c, _ in SEEDED], ids=[n for n, _, _ in SEEDED])
def test_seeded_arrays_match_the_oracle(ctx, tmp_path, monkeypatch, name, c):
    d = ctx(c["K"])
    want = walks_cases.oracle(name, c)
    a = walks_cases.arrays(c)
    npairs = want["pairs"]
    # batches of one pair, of 19 and what fits (tiny-3000: 1 500 batches of a pair each, the batch boundaries)
    for per in (1, 37, 0):
        out = os.path.join(tmp_path, f"per{per}")
        os.makedirs(out)
        held = d.stats()["hbm_held"]
        st = d.walks_build_arrays(a, per, out)
        assert d.stats()["hbm_held"] == held
        check(st, d.walks_fetch(), open(os.path.join(out, FILE), "rb").read(), want, f"{name} walks_per_batch={per}")
        pb = (per + 1) // 2
        assert st["batches"] == ((npairs + pb - 1) // pb if per else (1 if npairs else 0)) and st["ranges"] == (1 if npairs else 0)
        assert st["host_route"] == 0 and st["collisions"] == 0 and os.listdir(out) == [FILE]
    # dense reads (the cases' are), no directory: the same result, no file; dfk_walks_write then writes the same
    st = d.walks_build_arrays(a, read_off=None)
    check(st, d.walks_fetch(), written(d, tmp_path, "later"), want, name + " dense")
    if npairs < 3: return
    # small ranges of pairs
    monkeypatch.setenv("DFK_PIDX_RANGE_PAIRS", str(max(1, want["entries"] // 5)))
    st = d.walks_build_arrays(a, 37)
    check(st, d.walks_fetch(), None, want, name + " in small ranges")
    assert st["ranges"] >= 3
    monkeypatch.delenv("DFK_PIDX_RANGE_PAIRS")
    # the live list forced small: the walks that outgrow it take the host route, the bytes are the same
    monkeypatch.setenv("DFK_WALK_MAX_LIVE", "2")
    st = d.walks_build_arrays(a)
    check(st, d.walks_fetch(), None, want, name + " with a live list of 2")
    assert (st["host_route"] > 0) == (want["live_max"] > 2)
    if name == "planted": assert st["host_route"] >= 8
    monkeypatch.delenv("DFK_WALK_MAX_LIVE")
    # the hash cut to 8 bits: collisions, which verification turns away
    monkeypatch.setenv("DFK_WALK_HASH_BITS", "8")
    st = d.walks_build_arrays(a)
    check(st, d.walks_fetch(), None, want, name + " with an 8-bit hash")
    assert st["collisions"] > 0 or want["steps"] < 100


def test_arrays_refusals(ctx, tmp_path):
    from superplus_amd.dfk import DfkError
    d = ctx(walks_cases.K)
    name, c, _ = SEEDED[0]
    want = walks_cases.oracle(name, c)
    a = walks_cases.arrays(c)
    st = d.walks_build_arrays(a)
    E = len(c["inv"])
    not_closer = next(e for e in range(E) if e not in c["ce"])
    fell = a["read_off"].copy(); fell[3] = fell[2] - 1
    qfell = a["pq_off"].copy(); qfell[3] = qfell[2] - 1
    efell = a["edge_off"].copy(); efell[1] = efell[0]
    placed_read = want["recs"][0]["locs"][0][0]
    short = a["read_len"].copy(); short[placed_read] += 1              # its stream is now one value short
    packed1, off1 = a["read_packed"], a["read_off"]
    if a["read_len"][placed_read] % 4 == 0:                             # (the base needs a byte of its own)
        packed1 = np.insert(packed1, int(off1[placed_read + 1]), 0); off1 = off1.copy(); off1[placed_read + 1:] += 1
    k2 = next(k for k in range(len(c["ce"])) if a["read_first"][k + 1] - a["read_first"][k] >= 2)
    j = int(a["read_first"][k2])
    unsorted = a["reads"].copy(); unsorted[[j, j + 1]] = unsorted[[j + 1, j]]
    for code, change in ((-1, dict(pairs=np.asarray([(0, E)], np.int32))), (-1, dict(pairs=np.asarray([(-1, 0)], np.int32))),
                         (-1, dict(pairs=np.asarray([(not_closer, c["inv"][not_closer])], np.int32))),            # an edge of the graph that is no closer edge
                         (-1, dict(inv=None)), (-1, dict(read_len=None)), (-1, dict(read_first=None)), (-1, dict(pq=None)), (-1, dict(pq_off=None)), (-1, dict(edge_off=None)), (-1, dict(reads=None)),
                         (-1, dict(edge_off=efell)), (-1, dict(reads=unsorted)),
                         (-5, dict(read_off=fell)), (-5, dict(pq_off=qfell)), (-5, dict(read_len=short, read_packed=packed1, read_off=off1))):      # DFK_E_INPUT
        held = d.stats()["hbm_held"]
        with pytest.raises(DfkError) as e:
            d.walks_build_arrays(a, 0, str(tmp_path), **change)
        assert e.value.code == code, (change.keys(), e.value)
        assert d.stats()["hbm_held"] == held and not os.listdir(tmp_path)
        check(d.walks_stats(), d.walks_fetch(), None, want, "the earlier result")       # ... is still served
    # the next good call after them
    st2 = d.walks_build_arrays(a, 37)
    check(st2, d.walks_fetch(), None, want, "after the refusals")
    same = lambda x: {k: v for k, v in x.items() if not k.startswith("us") and k not in ("batches", "decoded")}       # (a read is decoded once a batch)
    assert same(st) == same(st2)


def test_a_set_of_two_to_the_23_entries_is_refused(ctx):
    """the reference's int sums could overflow there; the refusal comes before anything is composed or sent"""
    from superplus_amd.dfk import DfkError
    d = ctx(48)
    n = 1 << 22                                                                # reads(0) holds (id, False) of every read, reads(1) too: negated they are (id, True): 2^23 distinct entries
    a = dict(inv=np.asarray([1, 0], np.int32), kmers=np.asarray([13, 13], np.int32), edge_packed=np.zeros(30, np.uint8), edge_off=np.asarray([0, 15, 30], np.uint64),
             ce=np.asarray([0, 1], np.uint64), read_first=np.asarray([0, n, 2 * n], np.uint64), reads=np.concatenate([2 * np.arange(n, dtype=np.uint64)] * 2),
             pairs=np.asarray([(0, 0)], np.int32), read_packed=np.zeros(1, np.uint8), read_off=np.zeros(n + 1, np.uint64), read_len=np.zeros(n, np.uint32), pq=np.zeros(1, np.uint8),
             pq_off=np.zeros(n + 1, np.uint64))
    held = d.stats()["hbm_held"]
    with pytest.raises(DfkError, match="2\\^23") as e:
        d.walks_build_arrays(a)
    assert e.value.code == -1 and d.stats()["hbm_held"] == held


# ---- 2. the fixtures, through the chain dfk_count ... dfk_closer_build -> dfk_walks_build
@pytest.mark.parametrize("case,K,which", FIXTURES, ids=[f[0] for f in FIXTURES])
def test_walks_file_and_counters_match_the_oracle_on_the_fixtures(golden_dir, tmp_path, case, K, which):
    from superplus_amd.dfk import DfkError
    want = walks_oracle.fixture_walks(golden_dir, case, K, which)
    assert want["placed"] > 0
    i = walks_oracle.fixture_inputs(golden_dir, case, K, which)
    rs = i["rs"]
    reads = tuple(rs[k] for k in READS)
    d = pathed(rs, case, K, tmp_path)
    with pytest.raises(DfkError, match="dfk_closer_build") as e:
        d.walks_build(None, *reads)
    assert e.value.code == -6
    d.hops_build(hops_inputs(golden_dir, case, K, which)["bc"])
    d.closer_build(closer_oracle.fixture_inputs(golden_dir, case, K, which)["dup"])
    held = d.stats()["hbm_held"]
    st = d.walks_build(None, *reads)
    assert d.stats()["hbm_held"] == held
    check(st, d.walks_fetch(), written(d, tmp_path), want, case)
    assert st["ranges"] == 1 and st["batches"] == 1 and st["host_route"] == 0 and st["collisions"] == 0
    if case == "graph_pathy_k48":
        # the pairs given explicitly and the reads dense; other pairs than the closer sets were made for are refused, the result stays
        pairs = np.asarray(i["pairs"], np.int32).reshape(-1, 2)
        st2 = d.walks_build(pairs, rs["packed"], None, rs["read_len"], rs["pq_bytes"], rs["pq_off"])
        check(st2, d.walks_fetch(), written(d, tmp_path, "explicit"), want, case + " (pairs given, dense)")
        other = next(e for e in range(len(i["inv"])) if e not in i["ce"])
        with pytest.raises(DfkError) as e:
            d.walks_build(np.asarray([(other, pairs[0][1])], np.int32), *reads)
        assert e.value.code == -1
        with pytest.raises(DfkError) as e:
            d.walks_build(pairs, rs["packed"], rs["base_off"][:-2], rs["read_len"][:-2], rs["pq_bytes"], rs["pq_off"][:-2])
        assert e.value.code == -1
        check(d.walks_stats(), d.walks_fetch(), None, want, "after refused calls")
    d.close()


# ---- 3. DF
def test_df_writes_the_walks_file(tmp_path, golden_dir):
    case, K, which = FIXTURES[0]
    want = walks_oracle.fixture_walks(golden_dir, case, K, which)              # ONE_GOOD off, as the table was made
    r = run_df(tmp_path, golden_dir, which, "HOPS=True", "ONE_GOOD=False", "CLOSER=True", "WALKS=True")
    assert r.returncode == 0, r.stdout + r.stderr
    w = f"{tmp_path}/GapToy/1/a.48"
    assert open(f"{w}/{FILE}", "rb").read() == want["file"]
    for f in sorted(os.listdir(f"{golden_dir}/{case}")):                       # everything else DF writes there is still the fixture's
        if f.startswith("a."):
            assert open(f"{w}/{f}", "rb").read() == open(f"{golden_dir}/{case}/{f}", "rb").read(), f
    lines = [l for l in r.stdout.splitlines() if l.startswith("DF_WALKS ")]
    assert lines == ['DF_WALKS {"pairs": %d, "walks": %d, "entries": %d, "placed": %d, "bases": %d, "longest": %d, "a.stack.walks": "%016x%016x", "steps": %d, "dup_steps": %d, '
                     '"past_edge": %d, "side0_empty": %d, "side1_empty": %d, "short": %d, "trimmed": %d, "yields": %d, "live_max": %d, "host_route": 0, "batches": 1, "ranges": 1}'
                     % (want["pairs"], want["walks"], want["entries"], want["placed"], want["sum_ee"], want["longest"], *want["digest"], want["steps"], want["dup_steps"], want["past_edge"],
                        want["side0_empty"], want["side1_empty"], want["short"], want["trimmed"], want["yields"], want["live_max"])], lines
    assert r.stdout.index("DF_CLOSER ") < r.stdout.index("DF_WALKS ")


def test_df_refuses_walks_without_the_closer_and_on_a_sharded_run(tmp_path, golden_dir):
    r = run_df(tmp_path, golden_dir, "frag", "HOPS=True", "WALKS=True")
    assert r.returncode != 0 and "WALKS=True needs CLOSER=True" in r.stdout
    assert not os.path.exists(f"{tmp_path}/GapToy")
    env = dict(os.environ)
    env["DF_FORCE_SHARDED"] = "1"
    r = run_df(tmp_path, golden_dir, "frag", "HOPS=True", "CLOSER=True", "WALKS=True", env=env)
    assert r.returncode != 0 and "runs on one GPU only" in r.stdout
    assert not os.path.exists(f"{tmp_path}/GapToy")


def test_df_without_the_switch_writes_and_prints_what_it_did(tmp_path, golden_dir):
    """WALKS=False against the argument absent: the same listing, the same a.close.* bytes, the same DF_ lines"""
    runs = []
    for sub, extra in (("absent", []), ("off", ["WALKS=False"])):
        root = os.path.join(tmp_path, sub)
        os.makedirs(root)
        r = run_df(root, golden_dir, "frag", "HOPS=True", "CLOSER=True", *extra)
        assert r.returncode == 0, r.stdout + r.stderr
        w = f"{root}/GapToy/1/a.48"
        assert not os.path.exists(f"{w}/{FILE}") and "DF_WALKS" not in r.stdout and "a.stack.walks" not in r.stdout
        runs.append((sorted(os.listdir(w)), {f: open(f"{w}/{f}", "rb").read() for f in os.listdir(w) if f.startswith("a.close")},
                     [l.split(" ")[0] for l in r.stdout.splitlines() if l.startswith("DF_")],
                     [l for l in r.stdout.splitlines() if l.startswith(("DF_CLOSER ", "DF_HOPS ", "DF_DIGESTS "))]))
    assert runs[0] == runs[1] and "a.close.reads" in runs[0][0]
