"""The read paths moved onto the patched graph on the GPU (dfk_translate_build / _build_arrays / _fetch / _write / _drop: k_tp_decide a lane a
read, the host route for flagged reads, the scan over the units' word counts, k_tp_emit) against tests/translate_oracle.py: the fetched
paths, a.patch.paths byte for byte, every counter and the digest -- on every case of tests/translate_cases.py with reads_per_batch 0, 1, 37
and 257; read counts at the wave and workgroup edges with placed / cleared / flagged patterns; with no closures on fixtures' own graphs against
the reference-written a.paths cut to first edges; the chain after a real dfk_count ... dfk_patch_build on two fixtures, where the bases under
every translated read are also compared with the bases under it before, asking no oracle; every refusal with the earlier result still served;
`DF ... PATCH=True TRANSLATE=True` on frag, its refusal without PATCH=True, and DF without the switch.  Everything is exact."""
import ctypes as C
import os

import numpy as np
import pytest

from tests import translate_cases as tc, translate_oracle as to

pytestmark = pytest.mark.gpu

COUNTERS = ("reads", "placed_before", "step2", "walk", "cleared_empty", "cleared_ranoff", "host", "invalid", "edge_changed", "offset_changed", "placed", "var_bytes")
LIMIT = 300                                                                    # seconds a test may take


@pytest.fixture(autouse=True)
def time_limit():
    """every GPU step under a time limit of its own: faulthandler's watchdog is a thread of the C runtime, so it ends the process even
    while the test waits inside the library for a kernel that does not come back (a Python signal handler would not run there)"""
    import faulthandler
    faulthandler.dump_traceback_later(LIMIT, exit=True)
    yield
    faulthandler.cancel_dump_traceback_later()


def tables(c):
    first = np.concatenate([[0], np.cumsum([len(x) for x in c["to3"]])]).astype(np.uint64)
    return first, np.asarray([x for l in c["to3"] for x in l], np.int32), np.asarray(c["left3"], np.int32), np.asarray(c["kmers3"], np.int32)


def as_list(fetched):
    off, first, edges = fetched
    return [(int(o), [int(x) for x in edges[int(a):int(b)]]) for o, a, b in zip(off, first, first[1:])]


def check(d, st, want, tmp_path, sub, what, batches=None):
    assert as_list(d.translate_fetch()) == want["paths"], f"{what}: the paths"
    c = want["counters"]
    assert tuple(st[k] for k in COUNTERS) == tuple(c[k] for k in COUNTERS), f"{what}: {[(k, st[k], c[k]) for k in COUNTERS if st[k] != c[k]]}"
    assert (st["sum"], st["xor"]) == want["digest"], f"{what}: the digest"
    if batches is not None: assert st["batches"] == batches, f"{what}: {st['batches']} batches"
    out = os.path.join(tmp_path, sub)
    os.makedirs(out, exist_ok=True)
    held = d.stats()["hbm_held"]
    d.translate_write(out)
    assert d.stats()["hbm_held"] == held and os.listdir(out) == ["a.patch.paths"]
    assert open(os.path.join(out, "a.patch.paths"), "rb").read() == want["file"], f"{what}: a.patch.paths"


@pytest.fixture(scope="module")
def ctx():
    from superplus_amd.dfk import Dfk
    d = Dfk(K=tc.K)
    yield d
    d.close()


@pytest.fixture(scope="module")
def cases():
    out = {}
    for name, c in tc.all_cases().items():
        r = tc.run(c)
        tc.fires(name, c, r)                                                   # before any device is asked
        out[name] = (c, r)
    return out


NAMES = ("empty_before", "no_to3", "negative", "bases_kmers", "walks", "circle", "one_kmer", "ranoff_neg", "overlaps", "break", "random", "pather")


# ---- 1. the hand-made and seeded cases
@pytest.mark.parametrize("name", NAMES)
def test_arrays_match_the_oracle(ctx, cases, tmp_path, name):
    d = ctx
    c, want = cases[name]
    n = len(c["paths"])
    d.translate_drop()
    empty = d.stats()["hbm_held"]
    for per in (0, 1, 37, 257):
        st = d.translate_build_arrays(*tables(c), c["paths"], per)
        check(d, st, want, tmp_path, f"per{per}", f"{name} reads_per_batch={per}", (n + per - 1) // per if per else 1)
        assert d.stats()["hbm_held"] > empty                                   # the result is on the device ...
    d.translate_drop()
    assert d.stats()["hbm_held"] == empty                                      # ... and gone with _drop: every scratch block went back before
    d.translate_drop()                                                         # (nothing to drop: nothing happens)
    if name == "pather": assert st["host"] == 0


def test_all_cases_are_run(cases):
    assert sorted(cases) == sorted(NAMES)


def test_the_file_is_written_by_the_arrays_call_when_asked(ctx, cases, tmp_path):
    c, want = cases["random"]
    ctx.translate_build_arrays(*tables(c), c["paths"], 100, tmp_path)
    assert open(os.path.join(tmp_path, "a.patch.paths"), "rb").read() == want["file"]


# ---- 2. wave and workgroup edges
def patterns(n):
    """(what, placed(i), flagged(i)): all placed, all cleared, alternating, a lone placed read on lane 0 and lane 63, on the first and last slot
    of a workgroup's unit; flagged reads in lane 0 alone, lane 63 alone, a whole wave, none"""
    never = lambda i: False
    last_unit = (n - 1) // 256 * 256
    yield "all placed", (lambda i: True), never
    yield "all cleared", never, never
    yield "alternating", (lambda i: i % 2 == 0), never
    yield "alternating the other way", (lambda i: i % 2 == 1), never
    for what, at in (("lane 0", 0), ("lane 63", 63), ("lane 0 of the last wave", (n - 1) // 64 * 64), ("the last read", n - 1), ("the first slot of the last unit", last_unit), ("the last slot of the first unit", 255)):
        if at < n:
            yield "a lone placed read on " + what, (lambda i, at=at: i == at), never
            yield "a lone cleared read on " + what, (lambda i, at=at: i != at), never
            yield "a lone flagged read on " + what + " among placed", (lambda i: True), (lambda i, at=at: i == at)
            yield "a lone flagged read on " + what + " among cleared", never, (lambda i, at=at: i == at)
    yield "the first wave flagged", (lambda i: i % 3 == 0), (lambda i: i < 64)
    yield "the last wave flagged", (lambda i: i % 3 == 0), (lambda i: i >= (n - 1) // 64 * 64)
    yield "all flagged", never, (lambda i: True)


@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257, 1025])
def test_wave_and_workgroup_edges(ctx, tmp_path, n):
    d = ctx
    for what, placed, flagged in patterns(n):
        c = tc.pattern_case(n, placed, flagged)
        want = tc.run(c)
        k = want["counters"]
        assert k["host"] == sum(1 for i in range(n) if flagged(i)) == k["walk"] and k["step2"] == sum(1 for i in range(n) if placed(i) and not flagged(i)) and k["cleared_ranoff"] == 0, what
        for per in (0, 100):                                                   # (100: the scan's carries across waves, units and batches)
            st = d.translate_build_arrays(*tables(c), c["paths"], per)
            check(d, st, want, tmp_path, "edges", f"{n} reads, {what}, reads_per_batch={per}", (n + per - 1) // per if per else 1)


# ---- 3. no closures: the reference's a.paths cut to first edges
@pytest.mark.parametrize("case,K", [("graph_special_k48", 48), ("graph_k40_nobc", 40), ("graph_k60_nobc", 60), ("graph_zoo_k48", 48)])
def test_without_closures_the_paths_are_cut_to_their_first_edge(golden_dir, tmp_path, case, K):
    from superplus_amd.dfk import Dfk
    from tests import patch_oracle as po
    from tests.test_gpu_patch import arrays
    from tests.test_paths_oracle import decode_paths
    g = po.fixture_graph(golden_dir, case, K)
    paths = decode_paths(open(os.path.join(golden_dir, case, "a.paths"), "rb").read())
    d = Dfk(K=K)
    d.patch_build_arrays(*arrays(g, []))
    t = d.patch_fetch()
    E = len(g["edges"])
    assert [int(x) for x in t["to3"]] == list(range(E)) and not t["left3"].any()
    st = d.translate_build_arrays(t["to3_first"], t["to3"], t["left3"], t["kmers"], paths, 4099)
    cut = [(o, p[:1]) for o, p in paths]
    assert as_list(d.translate_fetch()) == cut
    d.translate_write(tmp_path)
    assert open(os.path.join(tmp_path, "a.patch.paths"), "rb").read() == to.paths_file(cut)
    placed = sum(1 for _, p in paths if p)
    assert (st["step2"], st["walk"], st["host"], st["cleared_empty"], st["cleared_ranoff"], st["offset_changed"], st["edge_changed"], st["invalid"]) == (placed, 0, 0, 0, 0, 0, 0, 0) and placed
    assert (st["sum"], st["xor"]) == to.paths_digest(cut) and st["batches"] == (len(paths) + 4098) // 4099
    d.close()


# ---- 4. the refusals
def test_refusals(ctx, cases, tmp_path):
    from superplus_amd import dfk
    from superplus_amd.dfk import Dfk, DfkError
    fresh = Dfk(K=tc.K)
    for call in (fresh.translate_stats, fresh.translate_fetch, lambda: fresh.translate_write(tmp_path), fresh.translate_build):     # nothing built; no paths
        with pytest.raises(DfkError) as e:
            call()
        assert e.value.code == -6                                              # DFK_E_STATE
    fresh.translate_drop()
    fresh.close()
    d = ctx
    c, want = cases["overlaps"]
    first, to3, left3, kmers3 = tables(c)
    st = d.translate_build_arrays(first, to3, left3, kmers3, c["paths"])
    check(d, st, want, tmp_path, "good", "the good call")
    late, fell = first.copy(), first.copy()
    late[0] = 1; fell[1] = fell[2] + 1
    id3, neg3, k0, l30 = to3.copy(), to3.copy(), kmers3.copy(), left3.copy()
    id3[3] = len(kmers3); neg3[0] = -1; k0[2] = 0; l30[1] = 1 << 30
    P = c["paths"]
    bad_paths = {"an old edge past the graph": P[:2] + [(0, [len(left3)])], "a negative old edge": [(0, [-1])] + P[:2], "an offset of 2^30": P[:1] + [(1 << 30, [0])],
                 "an offset of -2^30": P[:1] + [(-(1 << 30), [0])]}
    bad = [("to3_first does not start at 0", (late, to3, left3, kmers3, P)), ("to3_first falls", (fell, to3, left3, kmers3, P)), ("a to3 id past hb3", (first, id3, left3, kmers3, P)),
           ("a negative to3 id", (first, neg3, left3, kmers3, P)), ("kmers3 below 1", (first, to3, left3, k0, P)), ("left3 of 2^30", (first, to3, l30, kmers3, P))]
    bad += [(w, (first, to3, left3, kmers3, p)) for w, p in bad_paths.items()]
    off, pf, ed = np.zeros(3, np.int32), np.array([0, 1, 3, 2], np.uint64), np.zeros(4, np.int32)
    bad += [("the paths' starts fall", (first, to3, left3, kmers3, (off, pf, ed))), ("the paths do not start at 0", (first, to3, left3, kmers3, (off, np.array([1, 1, 2, 3], np.uint64), ed)))]
    for what, args in bad:
        held = d.stats()["hbm_held"]
        with pytest.raises(DfkError) as e:
            d.translate_build_arrays(*args)
        assert e.value.code == -1 and d.stats()["hbm_held"] == held, what      # DFK_E_ARG
        check(d, d.translate_stats(), want, tmp_path, "after", "after the refusal: " + what)
    # null arguments, 2^31 reads and a batch of 2^32 bytes, through the library itself: what is named is refused before anything is read
    p = dfk._p
    offs = np.zeros(2, np.int32); pfirst = np.array([0, 1], np.uint64); edges = np.zeros(2, np.int32); huge = np.array([0, 1 << 30], np.uint64)
    good = [d._ctx, C.c_uint64(len(left3)), p(first), p(to3), p(left3), C.c_uint64(len(kmers3)), p(kmers3), C.c_uint64(1), p(pfirst), p(edges), p(offs), C.c_uint64(0), None]
    assert dfk.lib().dfk_translate_build_arrays(*good) == 0
    st1 = d.translate_stats()
    assert st1["reads"] == 1
    for what, at, value in (("null to3_first", 2, None), ("null to3", 3, None), ("null left3", 4, None), ("null kmers3", 6, None), ("null first", 8, None), ("null edges", 9, None),
                            ("null offsets", 10, None), ("2^31 reads", 7, C.c_uint64(1 << 31)), ("a batch of 2^32 bytes", 8, p(huge))):
        a = list(good); a[at] = value
        held = d.stats()["hbm_held"]
        assert dfk.lib().dfk_translate_build_arrays(*a) == -1 and d.stats()["hbm_held"] == held, what
        assert d.translate_stats() == st1, what
    assert dfk.lib().dfk_translate_build_arrays(None, *good[1:]) == -1
    c2, want2 = cases["random"]
    check(d, d.translate_build_arrays(*tables(c2), c2["paths"], 37), want2, tmp_path, "next", "the next good call")


# ---- 5. the chain after a real count
def check_bases(K, old_edges, new_edges, before, after, to3_first, to3, left3, what):
    """no oracle: under every translated read with old offset >= 0 the hb3 edge shows from the new offset what the old first edge showed from
    the old offset, over min(K, what either edge has left); a negative offset moves by left3[e0] onto to3[e0][0]"""
    n_pos = n_neg = 0
    for i, ((o, p), (no, ne)) in enumerate(zip(before, after)):
        if not p:
            assert (no, ne) == (o, []), f"{what}: read {i} had no path"
            continue
        if not ne: continue
        a, b = old_edges[p[0]], new_edges[ne[0]]
        if o >= 0:
            n = min(K, len(a) - o, len(b) - no)
            assert no >= 0 and n > 0 and bytes(a[o:o + n]) == bytes(b[no:no + n]), f"{what}: read {i}: {n} bases at {o} of edge {p[0]} are not those at {no} of hb3's {ne[0]}"
            n_pos += 1
        else:
            assert no == o + int(left3[p[0]]) and ne[0] == int(to3[int(to3_first[p[0]])]), f"{what}: read {i} with offset {o}"
            n_neg += 1
    return n_pos, n_neg


@pytest.mark.parametrize("case,K,which", [("graph_special_k48", 48, "special"), ("graph_pathy_k48", 48, "pathy")], ids=["graph_special_k48", "graph_pathy_k48"])
def test_chain_on_the_fixtures(golden_dir, tmp_path, case, K, which):
    from superplus_amd.dfk import DfkError
    from tests import patch_oracle as po
    from tests.test_gpu_cons import partnered
    from tests.test_gpu_patch import arrays, written_edges
    from tests.test_gpu_sclosures import READS
    g = po.fixture_graph(golden_dir, case, K)
    d, rs, i = partnered(golden_dir, tmp_path, case, K, which)
    reads = tuple(rs[k] for k in READS)
    before = d.paths()
    with pytest.raises(DfkError, match="dfk_patch_build") as e:
        d.translate_build()
    assert e.value.code == -6                                                  # paths, but no patched graph
    d.patch_build_arrays(*arrays(g, []))
    with pytest.raises(DfkError, match="dfk_patch_build_arrays") as e:
        d.translate_build()
    assert e.value.code == -6                                                  # a patched graph, but not this context's
    d.cons_build(*reads); d.offsets_build(); d.closures_build(*reads)
    d.walks_build(None, *reads); d.scons_build(*reads); d.soffsets_build(*reads); d.sclosures_build(*reads)
    assert d.patch_build()["closures"] > 0
    held = d.stats()["hbm_held"]
    st = d.translate_build()
    with_result = d.stats()["hbm_held"]
    t = d.patch_fetch()
    first = [int(x) for x in t["to3_first"]]
    old = as_list(before)
    want = to.run(old, [[int(x) for x in t["to3"][a:b]] for a, b in zip(first, first[1:])], [int(x) for x in t["left3"]], [int(x) for x in t["kmers"]], K)
    check(d, st, want, tmp_path, "chain", case)
    assert st["host"] == 0 and st["invalid"] == 0 and st["cleared_ranoff"] == 0 and st["cleared_empty"] == 0 and st["placed"] == st["placed_before"] > 0
    assert all(np.array_equal(a, b) for a, b in zip(before, d.paths()))          # the context's own paths are as they were
    d.patch_write(tmp_path)
    n_pos, n_neg = check_bases(K, g["edges"], written_edges(tmp_path), old, as_list(d.translate_fetch()), t["to3_first"], t["to3"], t["left3"], case)
    assert n_pos > 0 and n_pos + n_neg == st["placed"]
    again = d.translate_build()                                                # again: the earlier result's blocks go back
    assert d.stats()["hbm_held"] == with_result and (again["sum"], again["xor"]) == (st["sum"], st["xor"])
    d.translate_drop()
    assert d.stats()["hbm_held"] == held < with_result
    d.close()


# ---- 6. DF
def df_args():
    from tests.test_gpu_patch import df_args as patch_args
    return (*patch_args(), "PATCH=True")


def test_df_writes_the_translated_paths(tmp_path, golden_dir):
    from tests import patch_oracle as po
    from tests.hops_oracle import read_ints
    from tests.test_gpu_hops import run_df
    from tests.test_gpu_sclosures import FIXTURES, interleaved
    from tests.test_paths_oracle import decode_paths
    case, K, which = FIXTURES[0]
    seqs, n_s, n_g = interleaved(golden_dir, case, K, which)
    assert n_s + n_g == 657
    r = run_df(tmp_path, golden_dir, which, *df_args(), "TRANSLATE=True")
    assert r.returncode == 0, r.stdout + r.stderr
    w = f"{tmp_path}/GapToy/1/a.48"
    assert open(f"{w}/a.paths", "rb").read() == open(f"{golden_dir}/{case}/a.paths", "rb").read()
    # the oracle on the fixture's paths and the tables DF wrote (which tests/test_gpu_patch.py holds to the patch's oracle)
    f = open(f"{w}/a.patch.to3", "rb").read()
    E, n = (int(x) for x in np.frombuffer(f, "<u8", 2, 8))
    first = [int(x) for x in np.frombuffer(f, "<u8", E + 1, 24)]
    to3, left3 = np.frombuffer(f, "<i4", n, 24 + 8 * (E + 1)), np.frombuffer(f, "<i4", E, 24 + 8 * (E + 1) + 4 * n)
    paths = decode_paths(open(f"{golden_dir}/{case}/a.paths", "rb").read())
    want = to.run(paths, [[int(x) for x in to3[a:b]] for a, b in zip(first, first[1:])], [int(x) for x in left3], [int(x) for x in read_ints(f"{w}/a.patch.kmers")], K)
    assert open(f"{w}/a.patch.paths", "rb").read() == want["file"]
    c = want["counters"]
    lines = [l for l in r.stdout.splitlines() if l.startswith("DF_TRANSLATE ")]
    import re
    head = ('DF_TRANSLATE {"reads": %d, "placed_before": %d, "step2": %d, "walk": %d, "cleared_empty": %d, "cleared_ranoff": %d, "host": %d, "invalid": %d, "edge_changed": %d, '
            '"offset_changed": %d, "placed": %d, "a.patch.paths": "%016x%016x", "batches": '
            % (*(c[k] for k in ("reads", "placed_before", "step2", "walk", "cleared_empty", "cleared_ranoff", "host", "invalid", "edge_changed", "offset_changed", "placed")), *want["digest"]))
    assert len(lines) == 1 and lines[0].startswith(head) and re.fullmatch(r"[1-9][0-9]*\}", lines[0][len(head):]), lines    # (the batches are the pathing's)
    assert c["host"] == 0 and c["invalid"] == 0 and r.stdout.index("DF_PATCH ") < r.stdout.index("DF_TRANSLATE ")
    g = po.fixture_graph(golden_dir, case, K)
    from tests.test_gpu_patch import written_edges
    n_pos, n_neg = check_bases(K, g["edges"], written_edges(w), paths, want["paths"], first, to3, left3, "DF on frag")
    assert n_pos + n_neg == c["placed"]


def test_df_refuses_translate_without_patch(tmp_path, golden_dir):
    from tests.test_gpu_hops import run_df
    r = run_df(tmp_path, golden_dir, "frag", *[a for a in df_args() if a != "PATCH=True"], "TRANSLATE=True")
    assert r.returncode != 0 and "TRANSLATE=True needs PATCH=True" in r.stdout
    assert not os.path.exists(f"{tmp_path}/GapToy")


def test_df_without_the_switch_writes_and_prints_what_it_did(tmp_path, golden_dir):
    """TRANSLATE=False against the argument absent: the same listing, the same bytes, the same DF_ lines -- and no a.patch.paths"""
    from tests.test_gpu_hops import run_df
    runs = []
    for sub, extra in (("absent", []), ("off", ["TRANSLATE=False"])):
        root = os.path.join(tmp_path, sub)
        os.makedirs(root)
        r = run_df(root, golden_dir, "frag", *df_args(), *extra)
        assert r.returncode == 0, r.stdout + r.stderr
        w = f"{root}/GapToy/1/a.48"
        assert "DF_TRANSLATE" not in r.stdout and not os.path.exists(f"{w}/a.patch.paths")
        runs.append((sorted(os.listdir(w)), {f: open(f"{w}/{f}", "rb").read() for f in os.listdir(w) if f.startswith(("a.patch", "a.closures", "a.paths"))},
                     [l.split(" ")[0] for l in r.stdout.splitlines() if l.startswith("DF_")], [l for l in r.stdout.splitlines() if l.startswith(("DF_PATCH ", "DF_SCLOSURES ", "found "))]))
    assert runs[0] == runs[1] and "a.patch.to3" in runs[0][0]
