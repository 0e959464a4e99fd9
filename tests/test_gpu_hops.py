"""FindEdgePairs on the GPU (dfk_hops_build: the combined index, methods 1 and 2 through a table keyed by (e1, e2), method 3 a wave per
edge with its sets in LDS, the host's exact route for the edges that do not fit) against tests/hops_oracle.py: the pairs, the file
a.hops, the per-method counters and the digest on every fixture; the same bytes under other batch geometries, index ranges and LDS
capacities; ONE_GOOD; the edges of the contract; `DF HOPS=True`."""
import os
import subprocess

import numpy as np
import pytest

from tests import hops_cases, hops_oracle
from tests.test_gpu_paths import KW
from tests.test_hops_oracle import HOT, SPECIAL, TABLE, fixture_hops, fixture_inputs
from tests.test_paths_oracle import load_reads

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DF = os.path.join(ROOT, "superplus_amd", "DF")
ARRAYS = ("packed", "base_off", "read_len", "pq_bytes", "pq_off")
# the geometries of test_gpu_bads.py
GEOMETRIES = {"passes": dict(passes=3, inst_per_item=1500, keep_inputs=True), "slots": dict(slots=2), "sink": dict(sink=True)}
FIXTURES = [r[:3] for r in TABLE] + [SPECIAL, HOT]
BOTH = [("graph_pathy2_k48", 48, "pathy2"), ("graph_frag_k48", 48, "frag")]


def pathed(rs, case, K, tmp_path, monkeypatch=None, geometry=None, **kw):
    """count -> graph_build -> paths_build with mark_bads=True; the context"""
    from superplus_amd.dfk import Dfk
    ckw = dict(KW[case]); nobc = ckw.pop("nobc", False)
    extra = dict(GEOMETRIES[geometry]) if geometry else {}
    sink = extra.pop("sink", False)
    if extra.pop("slots", None):
        monkeypatch.setenv("DFK_PATH_SLOTS", "2"); monkeypatch.setenv("DFK_NO_FILTER", "1"); sink = True
    d = Dfk(K=K, mark_bads=True, **ckw, **extra, **kw)
    d.count(*(rs[k] for k in ARRAYS), None if nobc else rs["bc"])
    d.graph_build()
    if sink: d.paths_sink(os.path.join(tmp_path, "a.paths"))
    if extra.get("keep_inputs"): d.paths_build()
    else: d.paths_build(*(rs[k] for k in ARRAYS))
    if sink: d.paths_write(os.path.join(tmp_path, "a.paths"))
    return d


def built(d, bc, tmp_path, one_good=False):
    """hops_build -> (pairs as a list of tuples, bytes of a.hops, stats, digest)"""
    st = d.hops_build(bc, one_good)
    pairs = d.hops_fetch()
    out = os.path.join(tmp_path, "a.hops")
    n, digest = d.hops_write(out)
    assert d.hops_write(None) == (n, digest) and n == len(pairs) == st["pairs"]
    return [tuple(int(x) for x in p) for p in pairs], open(out, "rb").read(), st, digest


def check(got, want, what):
    pairs, file, st, digest = got
    missing, extra = sorted(set(want["pairs"]) - set(pairs)), sorted(set(pairs) - set(want["pairs"]))
    assert pairs == want["pairs"], f"{what}: {len(missing)} pairs missing (first {missing[:5]}), {len(extra)} too many (first {extra[:5]})"
    assert file == want["file"] and digest == want["digest"], what
    assert (st["m1"], st["m2"], st["m3"]) == (len(want["m1"]), len(want["m2"]), len(want["m3"])), what
    assert (st["searched"], st["extended"], st["most_rounds"], st["largest_x"]) == (want["searched"], want["extended"], want["most_rounds"], want["largest_x"]), what


# ---- 1. every fixture
@pytest.mark.parametrize("case,K,which", FIXTURES, ids=[f[0] for f in FIXTURES])
def test_pairs_file_counters_and_digest_match_the_oracle_on_the_fixtures(golden_dir, tmp_path, case, K, which):
    want = fixture_hops(golden_dir, case, K, which)
    row = next((r for r in TABLE if r[0] == case), None)
    if row:                                                                  # the expected side is what the table says, method by method
        assert (len(want["m1"]), len(want["m2"]), len(want["m3"]), len(want["pairs"])) == row[5]
    if case == SPECIAL[0]: assert want["pairs"]
    if case == HOT[0]: assert not want["pairs"]
    d = pathed(load_reads(golden_dir, which), case, K, tmp_path)
    got = built(d, fixture_inputs(golden_dir, case, K, which)["bc"], tmp_path)
    d.close()
    check(got, want, case)
    assert got[2]["host_edges"] == 0                                         # the default capacities hold every fixture


# ---- 2. the same bytes however the reads were batched, the index was split, and wherever an edge was decided
VARIANTS = [("geometry", g) for g in GEOMETRIES] + [("ranges", None), ("all on the host", None), ("some on the host", None)]


@pytest.mark.parametrize("variant,arg", VARIANTS, ids=[v[1] or v[0] for v in VARIANTS])
@pytest.mark.parametrize("case,K,which", BOTH, ids=[b[2] for b in BOTH])
def test_same_bytes_under_other_batches_ranges_and_capacities(golden_dir, tmp_path, monkeypatch, case, K, which, variant, arg):
    want = fixture_hops(golden_dir, case, K, which)
    assert want["m1"] and want["m2"] and want["m3"]
    if variant == "ranges": monkeypatch.setenv("DFK_PIDX_RANGE_PAIRS", "12000" if which == "pathy2" else "4000")
    if variant == "all on the host": monkeypatch.setenv("DFK_HOPS_MAX_SEQS", "1")
    if variant == "some on the host": monkeypatch.setenv("DFK_HOPS_MAX_SEQS", "19" if which == "pathy2" else "8")
    d = pathed(load_reads(golden_dir, which), case, K, tmp_path, monkeypatch, arg if variant == "geometry" else None)
    got = built(d, fixture_inputs(golden_dir, case, K, which)["bc"], tmp_path)
    d.close()
    check(got, want, f"{case} {variant} {arg}")
    st = got[2]
    if variant == "ranges": assert st["ranges"] >= 4
    if variant == "all on the host": assert st["host_edges"] == want["searched"] > 0
    if variant == "some on the host":
        # the oracle's own sizes of the edges' sets say which do not fit: some but not all
        expect = hops_cases.overflows(want, 19 if which == "pathy2" else 8, 24)
        assert 0 < expect < want["searched"] and st["host_edges"] == expect
    if variant not in ("all on the host", "some on the host"): assert st["host_edges"] == 0


# ---- 3. ONE_GOOD
@pytest.mark.parametrize("case,K,which", BOTH, ids=[b[2] for b in BOTH])
def test_one_good(golden_dir, tmp_path, case, K, which):
    want = fixture_hops(golden_dir, case, K, which, one_good=True)
    plain = fixture_hops(golden_dir, case, K, which)
    assert len(want["m1"]) > len(plain["m1"]) and want["m2"] == [] and want["pairs"] != plain["pairs"]
    d = pathed(load_reads(golden_dir, which), case, K, tmp_path)
    check(built(d, fixture_inputs(golden_dir, case, K, which)["bc"], tmp_path, one_good=True), want, f"{case} ONE_GOOD")
    check(built(d, fixture_inputs(golden_dir, case, K, which)["bc"], tmp_path), plain, f"{case} built again without")
    d.close()


# ---- 4. the contract
def test_state_rules_and_the_edges_of_the_contract(golden_dir, tmp_path):
    from superplus_amd import feudal
    from superplus_amd.dfk import Dfk, DfkError
    case, K, which = BOTH[1]
    rs = load_reads(golden_dir, which)
    bc = fixture_inputs(golden_dir, case, K, which)["bc"]
    want = fixture_hops(golden_dir, case, K, which)
    never = os.path.join(tmp_path, "never.hops")
    # without the flag: DFK_E_STATE, the message names the flag, no file
    d = Dfk(K=K, **KW[case])
    d.count(*(rs[k] for k in ARRAYS), rs["bc"]); d.graph_build(); d.paths_build(*(rs[k] for k in ARRAYS))
    for call in (lambda: d.hops_build(bc), lambda: d.hops_stats(), lambda: d.hops_fetch(), lambda: d.hops_write(never)):
        with pytest.raises(DfkError, match="DFK_F_MARK_BADS") as e:
            call()
        assert e.value.code == -6                                            # DFK_E_STATE
    assert not os.path.exists(never)
    d.close()
    # with it: before the paths, and before a build of the pairs
    d = Dfk(K=K, mark_bads=True, **KW[case])
    d.count(*(rs[k] for k in ARRAYS), rs["bc"]); d.graph_build()
    with pytest.raises(DfkError, match="dfk_paths_build") as e:
        d.hops_build(bc)
    assert e.value.code == -6
    d.paths_build(*(rs[k] for k in ARRAYS))
    with pytest.raises(DfkError, match="dfk_hops_build"):
        d.hops_write(never)
    assert not os.path.exists(never)
    with pytest.raises(DfkError):
        d.hops_build(np.full(len(bc), -1, np.int32))                         # barcodes are not negative
    # before and after the index and the duplicate marks; nothing held afterwards
    held = d.stats()["hbm_held"]
    first = built(d, bc, tmp_path)
    check(first, want, "before the index")
    assert d.stats()["hbm_held"] == held
    d.paths_index_dups_write(str(tmp_path), os.path.join(tmp_path, "a.dup"))
    d.bads_write(os.path.join(tmp_path, "a.bad"))
    held = d.stats()["hbm_held"]
    check(built(d, bc, tmp_path), want, "after the index")
    assert d.stats()["hbm_held"] == held
    # the barcode index instead of the expanded vector
    bci = feudal.read_bci(os.path.join(golden_dir, which + ".bci"))
    assert np.array_equal(feudal.bci_to_bc(bci, len(bc)), bc)
    st = d.hops_build_bci(bci)
    assert d.hops_write(None) == (len(want["pairs"]), want["digest"]) and st["m3"] == len(want["m3"])
    # no barcodes at all: every read under the one shared id: nothing has two: an empty file of 16 bytes
    st = d.hops_build(np.zeros(len(bc), np.int32))
    out = os.path.join(tmp_path, "empty.hops")
    assert d.hops_write(out)[0] == 0 and st["pairs"] == 0 and open(out, "rb").read() == b"BINWRITE" + bytes(8) and len(d.hops_fetch()) == 0
    d.close()


def test_second_build_on_the_pairs_in_reverse_order(golden_dir, tmp_path):
    """the same reads with the pairs in reverse order: the same graph, every read id changed: the pairs of the permuted set"""
    from tests.test_gpu_bads import rebuild
    from oracle import paths_oracle
    case, K, which = BOTH[1]
    rs = load_reads(golden_dir, which)
    i = fixture_inputs(golden_dir, case, K, which)
    n = len(i["bc"])
    order = np.arange(n).reshape(-1, 2)[::-1].reshape(-1)
    want = hops_oracle.run([i["paths"][k] for k in order], i["kmers"], i["inv"], i["to_left"], i["to_right"], i["bc"][order], i["bad"][::-1], K)
    assert want["pairs"]
    d = pathed(rs, case, K, tmp_path)
    check(built(d, i["bc"], tmp_path), fixture_hops(golden_dir, case, K, which), "first build")
    reads, quals = paths_oracle.unpack_reads(rs)
    rs2 = rebuild(rs, [bytes(reads[k]) for k in order], [quals[k] for k in order])
    d.graph_build()
    with pytest.raises(Exception, match="dfk_paths_build"):
        d.hops_fetch()                                                       # the graph was built again: the paths and their pairs are gone
    d.paths_build(*(rs2[k] for k in ARRAYS))
    check(built(d, i["bc"][order], tmp_path), want, "the pairs in reverse order")
    d.close()


# ---- 5. DF HOPS=True
def hops_lines(out):
    return [l for l in out.splitlines() if l.startswith("DF_HOPS ") or l.startswith("pairs.size( )")]


def run_df(tmp_path, golden_dir, which, *args, env=None):
    return subprocess.run([DF, f"ROOT={tmp_path}", f"LR={golden_dir}/{which}.fastb", "PIPELINE=cs", "ALIGN=False", "NUM_THREADS=8", "HBM_GB=8", *args],
                          capture_output=True, text=True, env=env, timeout=600)


@pytest.mark.parametrize("one_good", [True, False], ids=["default", "ONE_GOOD=False"])
@pytest.mark.parametrize("case,K,which", BOTH, ids=[b[2] for b in BOTH])
def test_df_writes_a_hops(tmp_path, golden_dir, case, K, which, one_good):
    want = fixture_hops(golden_dir, case, K, which, one_good=one_good)      # ONE_GOOD is True unless said otherwise, as in the reference
    assert want["m1"] and want["m3"]
    r = run_df(tmp_path, golden_dir, which, "HOPS=True", *([] if one_good else ["ONE_GOOD=False"]))
    assert r.returncode == 0, r.stdout + r.stderr
    rd = lambda p: open(p, "rb").read()
    w = f"{tmp_path}/GapToy/1/a.48"
    assert rd(f"{w}/a.hops") == want["file"]
    for f in sorted(os.listdir(f"{golden_dir}/{case}")):                     # everything else DF writes there is still the fixture's
        if f.startswith("a."):
            assert rd(f"{w}/{f}") == rd(f"{golden_dir}/{case}/{f}"), f
    assert not os.path.exists(f"{w}/a.bad") and "DF_BADS" not in r.stdout    # HOPS gathers MarkBads' sums; a.bad itself is BADS=True's
    assert hops_lines(r.stdout) == ["pairs.size( ) = %d" % len(want["pairs"]),
                                    'DF_HOPS {"a.hops": "%016x%016x", "pairs": %d, "m1": %d, "m2": %d, "m3": %d, "host_edges": 0}'
                                    % (want["digest"][0], want["digest"][1], len(want["pairs"]), len(want["m1"]), len(want["m2"]), len(want["m3"]))], hops_lines(r.stdout)
    assert r.stdout.index("DF_DIGESTS ") < r.stdout.index("DF_HOPS ")


def test_df_with_bads_and_hops_writes_a_bad_first(tmp_path, golden_dir):
    from tests import bads_oracle
    from tests.test_bads_oracle import fixture_expected
    case, K, which = BOTH[1]
    r = run_df(tmp_path, golden_dir, which, "HOPS=True", "BADS=True")
    assert r.returncode == 0, r.stdout + r.stderr
    w = f"{tmp_path}/GapToy/1/a.48"
    assert open(f"{w}/a.bad", "rb").read() == bads_oracle.bad_file(fixture_expected(golden_dir, case, K, which)[4])
    assert open(f"{w}/a.hops", "rb").read() == fixture_hops(golden_dir, case, K, which, one_good=True)["file"]
    assert r.stdout.index("DF_BADS ") < r.stdout.index("DF_HOPS ")


# ---- 6. refused where the paths are spread over ranks
@pytest.mark.parametrize("mode", ["loopback2", "forced", "gpus2"])
def test_df_refuses_hops_on_a_sharded_run(tmp_path, golden_dir, mode):
    env = dict(os.environ)
    args = ["HOPS=True"]
    if mode == "loopback2": args.append("NUM_GPUS=2"); env["DF_TRANSPORT"] = "loopback"
    if mode == "forced": env["DF_FORCE_SHARDED"] = "1"
    if mode == "gpus2": args.append("NUM_GPUS=2")
    r = run_df(tmp_path, golden_dir, "frag", *args, env=env)
    assert r.returncode != 0
    lines = [l for l in r.stdout.splitlines() if l.strip() and l != "Giving up." and not l.startswith("DF_MAIN_EPOCH ")]     # (DF's first line, always)
    assert len(lines) == 1 and lines[0].startswith("HOPS=True runs on one GPU only"), r.stdout
    assert not os.path.exists(f"{tmp_path}/GapToy")                          # no a.48/, nothing at all


# ---- 7. without HOPS: what DF did
def test_df_without_hops_writes_and_prints_what_it_did(tmp_path, golden_dir):
    r = run_df(tmp_path, golden_dir, "frag")
    assert r.returncode == 0, r.stdout + r.stderr
    w = f"{tmp_path}/GapToy/1/a.48"
    assert not os.path.exists(f"{w}/a.hops") and not os.path.exists(f"{w}/a.bad") and os.path.exists(f"{w}/a.dup")
    assert not hops_lines(r.stdout) and "DF_HOPS" not in r.stdout and "edge pairs" not in r.stdout and "pairs.size" not in r.stdout
    for f in sorted(os.listdir(f"{golden_dir}/graph_frag_k48")):
        if f.startswith("a."):
            assert open(f"{w}/{f}", "rb").read() == open(f"{golden_dir}/graph_frag_k48/{f}", "rb").read(), f
