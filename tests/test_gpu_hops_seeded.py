"""FindEdgePairs on the GPU on the seeded graphs of tests/hops_cases.py (the six dense random ones, the gapped chains, the dense graph of
the sizes), handed to the stage as arrays (dfk_hops_build_arrays: the batches laid out as the pather leaves them, then the very
hops_build() that dfk_hops_build and `DF HOPS=True` run) against tests/hops_oracle.py on the same arrays: the pairs, the bytes of a.hops,
the digest, the counts per method and the search's counters, as tests/test_gpu_hops.py checks them on the fixtures -- at the defaults, with
ONE_GOOD, under other capacities, ranges, batches and result buffers, with MarkBads' sums at the threshold, with the pairs in reverse
order; and the `frag` fixture through the same entry.

The library works at K = 40, 48 or 60 (the context's K is the stage's): the gapped chains are made for those, the six dense graphs
(recorded for the host at K = 10 to 48) run here at K = 40 where theirs is another, the oracle with them."""
import os

import numpy as np
import pytest

from tests import hops_cases, hops_oracle
from tests.test_gpu_hops import check
from tests.test_hops_oracle import fixture_hops, fixture_inputs

pytestmark = pytest.mark.gpu

GRAPHS = [(name, c, K if K in (40, 48, 60) else 40) for name, c, K, _ in hops_cases.seeded()]
NEW = {s[0] for s in hops_cases.CHAIN_SPECS}
_want = {}


def sums_of(c):
    """MarkBads' per-read sums: the gapped chains carry theirs (0, 150, 151, 65535); a dense graph's marks written as 0 / 151 on the first read"""
    if "sums" in c: return c["sums"]
    s = np.zeros(len(c["paths"]), np.uint16)
    s[0::2] = 151 * np.asarray(c["bad"], np.uint16)
    return s


def want(name, c, K, one_good=False):
    """the oracle on a seeded graph at the K the GPU runs it with; computed once and handed out unchanged"""
    key = (name, K, bool(one_good))
    if key not in _want:
        _want[key] = hops_cases.run(c, one_good, K)
    return _want[key]


@pytest.fixture(scope="module")
def ctx():
    """a context per K, with DFK_F_MARK_BADS, without a count, a graph or paths of its own"""
    from superplus_amd.dfk import Dfk
    made = {}

    def get(K):
        if K not in made: made[K] = Dfk(K=K, mark_bads=True)
        return made[K]
    yield get
    for d in made.values(): d.close()


def built(d, c, tmp_path, sums=None, one_good=False, reads_per_batch=0):
    """dfk_hops_build_arrays -> (pairs as a list of tuples, bytes of a.hops, stats, digest), holding no more of the device than before"""
    held = d.stats()["hbm_held"]
    st = d.hops_build_arrays(c["kmers"], c["inv"], c["to_left"], c["to_right"], c["n_vertices"], c["paths"], c["bc"], sums_of(c) if sums is None else sums,
                             one_good, reads_per_batch)
    assert d.stats()["hbm_held"] == held
    pairs = d.hops_fetch()
    out = os.path.join(tmp_path, "a.hops")
    n, digest = d.hops_write(out)
    assert d.hops_write(None) == (n, digest) and n == len(pairs) == st["pairs"] and st == d.hops_stats()
    return [tuple(int(x) for x in p) for p in pairs], open(out, "rb").read(), st, digest


def list_lengths(c):
    """entries per list of the combined index: an edge's crossings and its involution's"""
    n = [0] * len(c["kmers"])
    for p in c["paths"]:
        for g in p: n[g] += 1; n[c["inv"][g]] += 1
    return n


def ranges_of(n, cap):
    """a range of the combined index: the longest run of edges whose lists together hold at most `cap` entries, one edge at the least"""
    k, e0 = 0, 0
    while e0 < len(n):
        e1, tot = e0 + 1, n[e0]
        while e1 < len(n) and tot + n[e1] <= cap: tot += n[e1]; e1 += 1
        k += 1; e0 = e1
    return k


def device_results(r, max_seqs=96, max_len=24):
    """results the kernels emit (a pair once per method that finds it); the edges decided on the host add theirs there"""
    over = hops_cases.overflowing(r, max_seqs, max_len)
    return len(r["m1"]) + len(r["m2"]) + sum(1 for e, _ in r["m3"] if e not in over)


# ---- 1. the defaults, and ONE_GOOD
@pytest.mark.parametrize("one_good", [False, True], ids=["defaults", "ONE_GOOD"])
def test_seeded_graphs_match_the_oracle(ctx, tmp_path, one_good):
    some_on_the_host = []
    for name, c, K in GRAPHS:
        r = want(name, c, K, one_good)
        got = built(ctx(K), c, tmp_path, one_good=one_good)
        check(got, r, f"{name} K={K}")
        expect = hops_cases.overflows(r, 96, 24)
        assert got[2]["host_edges"] == expect and got[2]["ranges"] == 1, name
        if expect: some_on_the_host.append(name)
        if name in NEW and one_good: assert set(r["m1"]) > set(want(name, c, K)["m1"]) and not r["m2"]
    assert "dense1" in some_on_the_host                                     # X of 106, 32 exts, an extension of 49 edges


# ---- 2. capacities
@pytest.mark.parametrize("variant", ["one slot", "middle", "max_len 3"])
def test_seeded_graphs_under_other_capacities(ctx, tmp_path, monkeypatch, variant):
    n_middle = 0
    for name, c, K in GRAPHS:
        r = want(name, c, K)
        if variant == "one slot":
            seqs, length = 1, 24
        elif variant == "max_len 3":
            seqs, length = 96, 3
        else:
            # from the oracle's own sizes of the edges' sets: the capacity that sends nearest to half of the searched edges to the host
            sizes = sorted({nx for nx, _, _, _ in r["x_sizes"].values()})
            seqs = min(sizes, key=lambda m: abs(2 * hops_cases.overflows(r, m, 24) - r["searched"]))
            length = 24
        monkeypatch.setenv("DFK_HOPS_MAX_SEQS", str(seqs)); monkeypatch.setenv("DFK_HOPS_MAX_LEN", str(length))
        got = built(ctx(K), c, tmp_path)
        check(got, r, f"{name} {variant} ({seqs} x {length})")
        expect = hops_cases.overflows(r, seqs, length)
        assert got[2]["host_edges"] == expect, name
        if variant == "one slot": assert expect == r["searched"] > 0
        if variant == "middle" and 0 < expect < r["searched"]: n_middle += 1
        if variant == "max_len 3" and name in NEW: assert "X_LEN" in {w for v in hops_cases.overflowing(r, 96, 3).values() for w in v}
    if variant == "middle": assert n_middle == len(GRAPHS)                  # some on the host and not all, on every graph


# ---- 3. ranges of the combined index
@pytest.mark.parametrize("variant", ["every edge", "middle"])
def test_seeded_graphs_under_other_ranges(ctx, tmp_path, monkeypatch, variant):
    for name, c, K in GRAPHS:
        n = list_lengths(c)
        cap = 1 if variant == "every edge" else max(2, sum(n) // 5)
        monkeypatch.setenv("DFK_PIDX_RANGE_PAIRS", str(cap))
        got = built(ctx(K), c, tmp_path)
        check(got, want(name, c, K), f"{name} ranges of {cap}")
        assert got[2]["ranges"] == ranges_of(n, cap) and got[2]["host_edges"] == hops_cases.overflows(want(name, c, K), 96, 24), name
        if variant == "every edge": assert got[2]["ranges"] == len(n) and min(n) > 0      # (every seeded edge has a read on it or on its involution)
        if variant == "middle": assert 4 <= got[2]["ranges"] < len(n)


# ---- 4. batches
@pytest.mark.parametrize("per", [0, 7, 2], ids=["one batch", "batches of 7", "batches of 2"])
def test_seeded_graphs_under_other_batches(ctx, tmp_path, per):
    ends, begins = 0, 0
    for name, c, K in GRAPHS:
        if per == 7:
            # mates fall in different batches (reads 6 and 7, 20 and 21, ...); a batch ends with an unplaced read, another begins with one
            assert len(c["paths"]) > 14
            ends += sum(1 for i in range(6, len(c["paths"]), 7) if not c["paths"][i])
            begins += sum(1 for i in range(7, len(c["paths"]), 7) if not c["paths"][i])
        check(built(ctx(K), c, tmp_path, reads_per_batch=per), want(name, c, K), f"{name} batches of {per}")
    if per == 7: assert ends and begins


# ---- 5. the result buffer: a first attempt that is too small is done again with the counted size
@pytest.mark.parametrize("variant", ["one", "one short", "exact"])
def test_seeded_graphs_with_a_small_result_buffer(ctx, tmp_path, monkeypatch, variant):
    second = 0
    for name, c, K in GRAPHS:
        r = want(name, c, K)
        n = device_results(r)                                               # one range: what its kernels emit
        cap = 1 if variant == "one" else n if variant == "exact" else n - 1
        if cap < 1: continue                                                 # (a dense graph without pairs: nothing to be short of)
        second += n > cap
        monkeypatch.setenv("DFK_HOPS_OUT_CAP", str(cap))
        got = built(ctx(K), c, tmp_path)
        check(got, r, f"{name} room for {cap} of {n} results")
        assert got[2]["ranges"] == 1 and got[2]["host_edges"] == hops_cases.overflows(r, 96, 24), name
        if name in NEW: assert n > 1
    assert second == (0 if variant == "exact" else len([1 for name, c, K in GRAPHS if device_results(want(name, c, K)) > 1]))


# ---- 6. MarkBads' sums at the threshold
def test_seeded_graphs_with_sums_at_the_threshold(ctx, tmp_path):
    for name, c, K in GRAPHS:
        if name in NEW:
            # the chains' own sums are 0, 150, 151 and 65535 (section 1 ran them); here the two that decide a candidate change sides
            assert sorted(set(c["sums"].tolist())) == [0, 150, 151, 65535]
            base = set(want(name, c, K)["pairs"])
            for knob, at, pair in (("sum150", 150, False), ("sum151", 151, True)):
                kind, reads, there = c["knobs"][knob]
                assert kind == "sums" and [int(c["sums"][i]) for i in reads] == [at] and (c["marks"][knob] in base) != pair
                d = hops_cases.moved(c, c["knobs"][knob])
                r = hops_cases.run(d, K=K)
                assert (c["marks"][knob] in r["pairs"]) == pair
                check(built(ctx(K), d, tmp_path), r, f"{name} {knob} moved to {there}")
        else:
            # a dense graph's marks as sums on either read or both: 0 and 150 where it is not bad, 151 and 65535 where it is
            rng = np.random.default_rng(len(c["paths"]))
            bad = np.repeat(np.asarray(c["bad"], bool), 2)
            s = np.where(bad, rng.choice([0, 150, 151, 65535], len(bad)), rng.choice([0, 150], len(bad))).astype(np.uint16)
            first = bad[0::2] & (s[0::2] <= 150) & (s[1::2] <= 150)
            s[0::2][first] = 151
            assert np.array_equal((s[0::2] > 150) | (s[1::2] > 150), np.asarray(c["bad"], bool))
            check(built(ctx(K), c, tmp_path, sums=s), want(name, c, K), f"{name} sums")


# ---- 7. the order of the lists: nothing depends on what the atomics gave
def test_seeded_graphs_with_the_pairs_in_reverse_order(ctx, tmp_path):
    for name, c, K in GRAPHS:
        order = np.arange(len(c["paths"])).reshape(-1, 2)[::-1].reshape(-1)
        d = dict(c, paths=[c["paths"][k] for k in order], bc=np.asarray(c["bc"])[order], bad=np.asarray(c["bad"])[::-1], sums=sums_of(c)[order])
        r = hops_cases.run(d, K=K)
        assert r["pairs"] == want(name, c, K)["pairs"]                      # (edges are what the pairs name: the same set)
        check(built(ctx(K), d, tmp_path), r, f"{name} reversed")
        check(built(ctx(K), d, tmp_path, reads_per_batch=5), r, f"{name} reversed, batches of 5")


# ---- 8. a fixture through the array entry gives the fixture's a.hops
def test_frag_fixture_through_the_array_entry(ctx, golden_dir, tmp_path):
    case, K, which = "graph_frag_k48", 48, "frag"
    i = fixture_inputs(golden_dir, case, K, which)
    c = dict(i, n_vertices=int(max(i["to_left"].max(), i["to_right"].max())) + 1)
    for one_good in (False, True):
        r = fixture_hops(golden_dir, case, K, which, one_good)
        assert r["m1"] and r["m3"]
        got = built(ctx(K), c, tmp_path, one_good=one_good, reads_per_batch=1000)
        check(got, r, f"{case} ONE_GOOD={one_good}")
        assert got[2]["host_edges"] == 0


# ---- 9. the contract
def test_array_entry_refuses_what_dfk_hops_build_refuses(ctx, tmp_path):
    from superplus_amd.dfk import Dfk, DfkError
    name, c, K = next(g for g in GRAPHS if g[0] == "chains1")
    d = ctx(K)
    first = built(d, c, tmp_path)
    check(first, want(name, c, K), name)

    def refused(code, match, **change):
        with pytest.raises(DfkError, match=match) as e:
            built(d, dict(c, **change), tmp_path, sums=sums_of(dict(c, **change)))
        assert e.value.code == code
    bc = np.asarray(c["bc"]).copy(); bc[5] = -1
    refused(-1, "barcode", bc=bc)
    refused(-1, "pairs", paths=c["paths"][:-1], bc=c["bc"][:-1], sums=c["sums"][:-1])
    inv = list(c["inv"]); inv[0] = 3
    refused(-1, "involution", inv=inv)
    inv = list(c["inv"]); inv[0] = len(inv)
    refused(-1, "involution", inv=inv)
    for e in (len(c["kmers"]), -1):
        paths = list(c["paths"]); paths[3] = [e]
        refused(-1, "a path holds edge", paths=paths)
    tl = list(c["to_left"]); tl[2] = c["n_vertices"]
    refused(-1, "vertex out of range", to_left=tl)
    # a refused call changes nothing: the earlier result is still served, and the next build is whole
    assert [tuple(int(x) for x in p) for p in d.hops_fetch()] == first[0]
    check(built(d, c, tmp_path), want(name, c, K), f"{name} again")
    # without the flag: DFK_E_STATE, and the message names the flag
    plain = Dfk(K=K)
    with pytest.raises(DfkError, match="DFK_F_MARK_BADS") as e:
        plain.hops_build_arrays(c["kmers"], c["inv"], c["to_left"], c["to_right"], c["n_vertices"], c["paths"], c["bc"], c["sums"])
    assert e.value.code == -6
    plain.close()
    # no reads at all, no edges at all: an empty file
    empty = dict(c, paths=[], bc=np.zeros(0, np.int32), sums=np.zeros(0, np.uint16))
    assert built(d, empty, tmp_path)[1] == b"BINWRITE" + bytes(8)
