"""The patched graph on the GPU (dfk_patch_build / _build_arrays / _fetch / _write: the dictionary of allx written from the old edges, the
closures' K-mers looked up in batches, the graph kernels over the two parts, the old edges' paths read off the entries) against
tests/patch_oracle.py: the nine files a.patch.* byte for byte, to3_first, to3, left3, the counters and the digest -- on every case of
tests/patch_cases.py with kmers_per_batch 1, 37 and 0; the no-closure case on two fixtures' own files (K = 40 and 48) against the files the
reference wrote; each refusal with the earlier result still served and the next good call behind it; the chain after a real dfk_count ...
dfk_sclosures_build on two fixtures, with dfk_paths_build afterwards giving the paths it gave before; `DF ... CLOSURES=True SCLOSURES=True
PATCH=True` on frag with its 657 closures against the oracle's files, its refusals, and DF without the switch.  Everything is exact.
Whatever the device returned or wrote is also held to tests/patch_seeded.py's check_invariants, which asks no oracle: every old edge read
back off hb3 along to3 from left3, and hb3 holding together."""
import os

import numpy as np
import pytest

from oracle import graph_oracle as go
from tests import patch_cases, patch_oracle as po, patch_seeded

pytestmark = pytest.mark.gpu

COUNTERS = ("edges", "canonical", "vertices", "crossings", "closures", "short", "positions", "found", "new", "new_unique", "bits_added", "kmers3", "canonical3", "vertices3", "edges3", "single3",
            "path1", "path2", "path3", "to3", "left3")
LIMIT = 300                                                                    # seconds a test may take


@pytest.fixture(autouse=True)
def time_limit():
    """every GPU step under a time limit of its own: faulthandler's watchdog is a thread of the C runtime, so it ends the process even
    while the test waits inside the library for a kernel that does not come back (a Python signal handler would not run there)"""
    import faulthandler
    faulthandler.dump_traceback_later(LIMIT, exit=True)
    yield
    faulthandler.cancel_dump_traceback_later()


def arrays(g, closures):
    packed = [go._pack(bytes(s)) for s in g["edges"]]
    off = np.concatenate([[0], np.cumsum([len(p) for p in packed])])[:-1].astype(np.uint64) if packed else np.zeros(0, np.uint64)
    starts = np.concatenate([[0], np.cumsum([len(c) for c in closures])]).astype(np.uint64)
    return (np.asarray(g["inv"], np.int32), np.asarray(g["to_left"], np.int32), np.asarray(g["to_right"], np.int32), g["n_vertices"], np.frombuffer(b"".join(packed), np.uint8), off,
            np.asarray([len(s) for s in g["edges"]], np.uint32), starts, np.frombuffer(b"".join(bytes(c) for c in closures), np.uint8))


def written_edges(directory):
    """hb3's edges by id as a.patch.fastb in `directory` holds them"""
    from superplus_amd import feudal
    packed, off, ln = feudal.read_fastb(os.path.join(directory, "a.patch.fastb"))
    return po.unpack(packed.tobytes(), np.asarray(off, np.int64) - int(off[0]), ln) if len(ln) else []


def check(d, st, want, tmp_path, sub, what, g, closures):
    """the device's result against the oracle's `want`, then by itself against the old graph `g` and the closures"""
    got = d.patch_fetch()
    first = np.concatenate([[0], np.cumsum([len(p) for p in want["to3"]])])
    assert [int(x) for x in got["to3_first"]] == [int(x) for x in first], f"{what}: to3_first"
    assert [int(x) for x in got["to3"]] == [x for p in want["to3"] for x in p], f"{what}: to3"
    assert [int(x) for x in got["left3"]] == want["left3"], f"{what}: left3"
    for k, w in (("kmers", "kmers3"), ("inv", "inv3"), ("to_left", "to_left3"), ("to_right", "to_right3")):
        assert [int(x) for x in got[k]] == [int(x) for x in want[w]], f"{what}: hb3's {k}"
    assert tuple(st[k] for k in COUNTERS) == tuple(want["counters"][k] for k in COUNTERS), f"{what}: {[(k, st[k], want['counters'][k]) for k in COUNTERS if st[k] != want['counters'][k]]}"
    assert (st["sum"], st["xor"]) == want["digest"], f"{what}: the digest"
    out = os.path.join(tmp_path, sub)
    os.makedirs(out, exist_ok=True)
    held = d.stats()["hbm_held"]
    d.patch_write(out)
    assert d.stats()["hbm_held"] == held and sorted(os.listdir(out)) == sorted(want["files"])
    for f in want["files"]:
        assert open(os.path.join(out, f), "rb").read() == want["files"][f], f"{what}: {f}"
    first = [int(x) for x in got["to3_first"]]
    patch_seeded.check_invariants(g, closures, written_edges(out), got["inv"], got["to_left"], got["to_right"], [[int(x) for x in got["to3"][a:b]] for a, b in zip(first, first[1:])],
                                  got["left3"], got["kmers"], what)


# ---- 1. the hand-made and seeded cases
@pytest.fixture(scope="module")
def ctx():
    from superplus_amd.dfk import Dfk
    d = Dfk(K=patch_cases.K)
    yield d
    d.close()


@pytest.fixture(scope="module")
def cases(oracle):
    return {name: (g, cl, po.run(g, cl)) for name, g, cl in patch_cases.all_cases(oracle)}


NAMES = ("plain", "join", "interior", "onlyold", "bit", "lengths", "reversed", "selfrc", "twice", "cycle", "selfinv", "cross", "random")


@pytest.mark.parametrize("name", NAMES)
def test_arrays_match_the_oracle(ctx, cases, tmp_path, name):
    d = ctx
    g, closures, want = cases[name]
    n = want["counters"]["positions"]
    for per in (1, 37, 0):
        held = d.stats()["hbm_held"]
        st = d.patch_build_arrays(*arrays(g, closures), per)
        assert d.stats()["hbm_held"] == held
        check(d, st, want, tmp_path, f"per{per}", f"{name} kmers_per_batch={per}", g, closures)
        assert st["batches"] == ((n + per - 1) // per if per else (1 if n else 0))
    assert st["cycle_kmers"] == (160 if name == "cycle" else 0)
    if name == "join": assert st["batches"] == 1 and n == 75                    # (37: three batches, asserted above)


def test_all_cases_are_run(cases):
    assert sorted(cases) == sorted(NAMES)


# ---- 2. no closures: the fixture's own files come back
@pytest.mark.parametrize("case,K", [("graph_special_k48", 48), ("graph_k40_nobc", 40), ("graph_k60_nobc", 60), ("graph_zoo_k40", 40), ("graph_zoo_k48", 48), ("graph_zoo_k60", 60)])
def test_without_closures_the_fixture_comes_back(golden_dir, tmp_path, case, K):
    from superplus_amd.dfk import Dfk
    g = po.fixture_graph(golden_dir, case, K)
    d = Dfk(K=K)
    st = d.patch_build_arrays(*arrays(g, []))
    d.patch_write(tmp_path)
    for f in po.FILES:
        assert open(os.path.join(tmp_path, "a.patch." + f[2:]), "rb").read() == open(os.path.join(golden_dir, case, f), "rb").read(), f
    got = d.patch_fetch()
    E = len(g["edges"])
    assert [int(x) for x in got["to3"]] == list(range(E)) and not got["left3"].any() and [int(x) for x in got["to3_first"]] == list(range(E + 1))
    assert (st["edges3"], st["vertices3"], st["new_unique"], st["bits_added"], st["path1"], st["batches"]) == (E, g["n_vertices"], 0, 0, E, 0)
    d.close()


# ---- 3. the refusals
def test_refusals(ctx, cases, tmp_path):
    from superplus_amd.dfk import Dfk, DfkError
    fresh = Dfk(K=patch_cases.K)
    for call in (fresh.patch_stats, fresh.patch_fetch, lambda: fresh.patch_write(tmp_path), fresh.patch_build):     # nothing built; no graph
        with pytest.raises(DfkError) as e:
            call()
        assert e.value.code == -6                                              # DFK_E_STATE
    fresh.close()
    d = ctx
    g, closures, want = cases["interior"]
    st = d.patch_build_arrays(*arrays(g, closures))
    refused = patch_cases.refusals()
    assert [n for n, _ in refused] == ["inv", "end", "short", "notrc", "vertex", "twice"]
    for name, bad in refused:
        held = d.stats()["hbm_held"]
        with pytest.raises(DfkError) as e:
            d.patch_build_arrays(*arrays(bad, closures))
        assert e.value.code == -1 and d.stats()["hbm_held"] == held, name      # DFK_E_ARG
        check(d, d.patch_stats(), want, tmp_path, "after_" + name, "after the refusal " + name, g, closures)
    a = list(arrays(g, closures))
    fell = a[7].copy(); fell[1] = fell[2] + 1
    late = a[7].copy(); late[0] = 1
    four = a[8].copy(); four[3] = 4
    for what, bad_args in (("the starts fall", (*a[:7], fell, a[8])), ("the starts do not begin at 0", (*a[:7], late, a[8])), ("a closure base above 3", (*a[:8], four))):
        held = d.stats()["hbm_held"]
        with pytest.raises(DfkError) as e:
            d.patch_build_arrays(*bad_args)
        assert e.value.code == -1 and d.stats()["hbm_held"] == held, what
        check(d, d.patch_stats(), want, tmp_path, "after_closures", "after the refusal: " + what, g, closures)
    with pytest.raises(DfkError) as e:                                          # a context without a graph of its own has nothing to patch
        d.patch_build()
    assert e.value.code == -6
    g2, cl2, want2 = cases["join"]
    check(d, d.patch_build_arrays(*arrays(g2, cl2), 37), want2, tmp_path, "next", "the next good call", g2, cl2)


# ---- 4. the chain after a real count
@pytest.mark.parametrize("case,K,which", [("graph_special_k48", 48, "special"), ("graph_pathy_k48", 48, "pathy")], ids=["graph_special_k48", "graph_pathy_k48"])
def test_chain_on_the_fixtures(golden_dir, tmp_path, case, K, which):
    from superplus_amd.dfk import DfkError
    from tests.test_gpu_cons import partnered
    from tests.test_gpu_hops import ARRAYS
    from tests.test_gpu_sclosures import READS, interleaved
    closures = [bytes(np.asarray(c, np.uint8)) for c in interleaved(golden_dir, case, K, which)[0]]
    g = po.fixture_graph(golden_dir, case, K)
    want = po.run(g, closures)
    d, rs, i = partnered(golden_dir, tmp_path, case, K, which)
    reads = tuple(rs[k] for k in READS)
    before = d.paths()
    with pytest.raises(DfkError) as e:
        d.patch_build()
    assert e.value.code == -6                                                  # no closures yet
    d.cons_build(*reads); d.offsets_build(); d.closures_build(*reads)
    with pytest.raises(DfkError, match="dfk_sclosures_build") as e:
        d.patch_build()
    assert e.value.code == -6                                                  # only the first closer's
    d.walks_build(None, *reads); d.scons_build(*reads); d.soffsets_build(*reads); d.sclosures_build(*reads)
    held = d.stats()["hbm_held"]
    st = d.patch_build()
    assert d.stats()["hbm_held"] == held and st["closures"] == len(closures)
    check(d, st, want, tmp_path, "chain", case, g, closures)
    check(d, d.patch_build(37), want, tmp_path, "chain37", case + " kmers_per_batch=37", g, closures)
    # the context's own graph and pathing state are untouched: pathing the reads again gives what it gave
    d.paths_build(*(rs[k] for k in ARRAYS))
    after = d.paths()
    assert all(np.array_equal(a, b) for a, b in zip(before, after))
    d.close()


# ---- 5. DF
def df_args():
    from tests.test_gpu_sclosures import DF_ARGS
    return (*DF_ARGS, "PARTNERS=True", "CONS=True", "OFFSETS=True", "CLOSURES=True", "SCLOSURES=True")


def test_df_writes_the_patched_graph(tmp_path, golden_dir):
    from superplus_amd.dfk import PATCH_FILES
    from tests.test_gpu_hops import run_df
    from tests.test_gpu_sclosures import FIXTURES, interleaved
    case, K, which = FIXTURES[0]
    seqs, n_s, n_g = interleaved(golden_dir, case, K, which)
    assert n_s + n_g == 657
    g, closures = po.fixture_graph(golden_dir, case, K), [bytes(np.asarray(c, np.uint8)) for c in seqs]
    want = po.run(g, closures)
    r = run_df(tmp_path, golden_dir, which, *df_args(), "PATCH=True")
    assert r.returncode == 0, r.stdout + r.stderr
    w = f"{tmp_path}/GapToy/1/a.48"
    assert sorted(want["files"]) == sorted(PATCH_FILES)
    for f in PATCH_FILES:
        assert open(f"{w}/{f}", "rb").read() == want["files"][f], f
    for f in sorted(os.listdir(f"{golden_dir}/{case}")):                       # everything else DF writes there is still the fixture's
        if f.startswith("a."):
            assert open(f"{w}/{f}", "rb").read() == open(f"{golden_dir}/{case}/{f}", "rb").read(), f
    c = want["counters"]
    lines = [l for l in r.stdout.splitlines() if l.startswith("DF_PATCH ")]
    assert lines == ['DF_PATCH {"edges": %d, "closures": %d, "positions": %d, "found": %d, "new": %d, "new_unique": %d, "bits_added": %d, "kmers3": %d, "canonical3": %d, "vertices3": %d, '
                     '"edges3": %d, "to3": %d, "left3": %d, "a.patch.to3": "%016x%016x", "batches": 1}'
                     % (*(c[k] for k in ("edges", "closures", "positions", "found", "new", "new_unique", "bits_added", "kmers3", "canonical3", "vertices3", "edges3", "to3", "left3")), *want["digest"])], lines
    assert r.stdout.index("found 657 closures") < r.stdout.index("DF_PATCH ")
    # what DF wrote, by itself: the tables read back from its files
    from tests.hops_oracle import read_ints
    f = open(f"{w}/a.patch.to3", "rb").read()
    E, n = (int(x) for x in np.frombuffer(f, "<u8", 2, 8))
    first = [int(x) for x in np.frombuffer(f, "<u8", E + 1, 24)]
    to3, left3 = np.frombuffer(f, "<i4", n, 24 + 8 * (E + 1)), np.frombuffer(f, "<i4", E, 24 + 8 * (E + 1) + 4 * n)
    assert f[:8] == po.MAGIC and E == len(g["edges"]) and len(f) == 24 + 8 * (E + 1) + 4 * n + 4 * E
    patch_seeded.check_invariants(g, closures, written_edges(w), read_ints(f"{w}/a.patch.inv"), read_ints(f"{w}/a.patch.to_left"), read_ints(f"{w}/a.patch.to_right"),
                                  [[int(x) for x in to3[a:b]] for a, b in zip(first, first[1:])], left3, read_ints(f"{w}/a.patch.kmers"), "DF on frag")


def test_df_refuses_patch_without_both_closers_or_sharded(tmp_path, golden_dir):
    from tests.test_gpu_hops import run_df
    r = run_df(tmp_path, golden_dir, "frag", *[a for a in df_args() if a != "CLOSURES=True"], "PATCH=True")
    assert r.returncode != 0 and "PATCH=True needs CLOSURES=True and SCLOSURES=True" in r.stdout
    r = run_df(tmp_path, golden_dir, "frag", *df_args(), "PATCH=True", "NUM_GPUS=2")      # (the chain PATCH needs begins with HOPS=True, which says it)
    assert r.returncode != 0 and "runs on one GPU only" in r.stdout
    assert not os.path.exists(f"{tmp_path}/GapToy")


def test_df_without_the_switch_writes_and_prints_what_it_did(tmp_path, golden_dir):
    """PATCH=False against the argument absent: the same listing, the same bytes, the same DF_ lines -- and no a.patch.* file"""
    from tests.test_gpu_hops import run_df
    runs = []
    for sub, extra in (("absent", []), ("off", ["PATCH=False"])):
        root = os.path.join(tmp_path, sub)
        os.makedirs(root)
        r = run_df(root, golden_dir, "frag", *df_args(), *extra)
        assert r.returncode == 0, r.stdout + r.stderr
        w = f"{root}/GapToy/1/a.48"
        assert "DF_PATCH" not in r.stdout and not [f for f in os.listdir(w) if f.startswith("a.patch")]
        runs.append((sorted(os.listdir(w)), {f: open(f"{w}/{f}", "rb").read() for f in os.listdir(w) if f.startswith(("a.close", "a.stack", "a.closures"))},
                     [l.split(" ")[0] for l in r.stdout.splitlines() if l.startswith("DF_")], [l for l in r.stdout.splitlines() if l.startswith(("DF_CLOSURES ", "DF_SCLOSURES ", "found "))]))
    assert runs[0] == runs[1] and "a.closures.fastb" in runs[0][0]
