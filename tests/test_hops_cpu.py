"""superplus_amd/csrc/dfk_hops.h -- the C++ restatement of FindEdgePairs that the kernel k_hops_edges and the host's exact route
both run -- against tests/hops_oracle.py: tests/cpp/test_hops.cc (its own main) built plain and under
-fsanitize=address,undefined, run on its cases worked out by hand, on the ten seeded graphs recorded in tests/cpp/hops_cases.txt and
on two fixtures written out in the same form; and what the seeded graphs of tests/hops_cases.py must hold for those runs (and the GPU's,
tests/test_gpu_hops_seeded.py) to mean something.  CPU only."""
import os
import subprocess

import pytest

from tests import hops_cases, hops_oracle
from tests.test_hops_oracle import fixture_inputs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUILDS = {"plain": ["-O1"], "sanitized": ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]}
N_RECORDED = 2 * sum(len(caps) for _, _, _, caps in hops_cases.seeded())             # 24 of the six dense graphs, 20 of the gapped chains
NEW = [g for g in hops_cases.seeded() if g[0] in {s[0] for s in hops_cases.CHAIN_SPECS}]
_runs = {}


def ran(name, c, knob=None, **kw):
    """hops_oracle.run on a seeded graph, or on it with one knob moved; computed once"""
    key = (name, knob, tuple(sorted(kw.items())))
    if key not in _runs:
        _runs[key] = hops_cases.run(hops_cases.moved(c, c["knobs"][knob]) if knob else c, **kw)
    return _runs[key]


def test_recorded_cases_are_what_the_oracle_says_now():
    """tests/cpp/hops_cases.txt is hops_cases.text(): regenerate it (python -m tests.hops_cases) when the oracle or the generator changes"""
    assert open(hops_cases.FILE).read() == hops_cases.text()
    lines = open(hops_cases.FILE).read().split("\n")
    assert sum(l.startswith("graph ") for l in lines) == 10 and len(lines) < 6800     # ten seeded graphs, each written once
    idx = [k for k, l in enumerate(lines) if l.startswith("variant ")]
    assert len(idx) == N_RECORDED and {lines[k].split()[1] for k in idx} == {"0", "1"}    # the recorded cases: ONE_GOOD both ways, the capacities
    # the cases are not empty: with ONE_GOOD off every method has pairs; searches that overflow some capacities and not others
    n_of = lambda k, j: int(lines[k + 1 + j].split()[0])
    off = [k for k in idx if lines[k].split()[1] == "0"]
    assert all(sum(n_of(k, j) for k in off) > 0 for j in range(4))
    host = [int(lines[k + 5].split()[6]) for k in idx]
    assert any(h == 0 for h in host) and any(h > 0 for h in host)


@pytest.fixture(scope="module")
def fixture_cases(golden_dir, tmp_path_factory):
    """pathy2 (a 7-round search, 160 double crossings, 62 pairs of method 2) and frag in the form of hops_cases.txt: default capacities,
    one slot (every searched edge overflows), and a middle value at which some do"""
    out = []
    for case, which, caps in (("graph_pathy2_k48", "pathy2", [(96, 24), (1, 24), (19, 24)]), ("graph_frag_k48", "frag", [(96, 24), (6, 3)])):
        i = fixture_inputs(golden_dir, case, 48, which)
        c = dict(i, n_vertices=int(max(i["to_left"].max(), i["to_right"].max())) + 1)
        out += hops_cases.case_text(case, c, 48, caps)
    path = tmp_path_factory.mktemp("hops") / "fixture_cases.txt"
    path.write_text("\n".join(out) + "\n")
    return str(path)


@pytest.mark.parametrize("build", list(BUILDS))
def test_cpp_restatement_agrees_with_the_oracle(tmp_path, fixture_cases, build):
    exe = os.path.join(tmp_path, "test_hops")
    subprocess.check_call(["g++", *BUILDS[build], "-std=c++17", "-Wall", "-I", os.path.join(ROOT, "superplus_amd", "csrc"), "-o", exe,
                           os.path.join(ROOT, "tests", "cpp", "test_hops.cc")])
    for cases, n in ((hops_cases.FILE, N_RECORDED), (fixture_cases, 10)):
        out = subprocess.run([exe, cases], capture_output=True, text=True, timeout=600)
        assert out.returncode == 0, out.stdout + out.stderr
        assert f"the hand cases and {n} recorded cases agree" in out.stdout


# ---- what the gapped chains must hold (ONE_GOOD off throughout)
def test_gapped_chains_have_pairs_of_every_method():
    assert len(NEW) == 4 and N_RECORDED == 44
    for name, c, K, _ in NEW:
        assert K in (40, 48, 60) and len(c["kmers"]) <= 340 and len(c["paths"]) <= 1200, name
        r = ran(name, c)
        assert r["m1"] and r["m3"], name
    assert sum(1 for name, c, _, _ in NEW if ran(name, c)["m2"]) >= 2


@pytest.mark.parametrize("name,c,K", [g[:3] for g in NEW], ids=[g[0] for g in NEW])
def test_gapped_chains_thresholds_are_decisive(name, c, K):
    """every planted length or sum decides a pair: the union changes when it moves to the other side, and in the direction the rule says"""
    r = ran(name, c)
    here = set(r["pairs"])
    there = lambda knob: set(ran(name, c, knob)["pairs"])
    frm, to = hops_oracle.adjacency(c["to_left"], c["to_right"])
    inv, km = c["inv"], c["kmers"]
    # the sink test (and, seen from the far side, the source test) at 120 | 121
    a, far = c["marks"]["sink121"]
    d = hops_cases.moved(c, c["knobs"]["sink121"])
    assert not hops_oracle.sink_ok(a, km, c["to_right"], frm, to) and hops_oracle.sink_ok(a, d["kmers"], c["to_right"], frm, to)
    assert not hops_oracle.source_ok(inv[a], km, c["to_left"], frm, to) and hops_oracle.source_ok(inv[a], d["kmers"], c["to_left"], frm, to)
    assert there("sink121") - here == {(a, far), (inv[far], inv[a])} and not here - there("sink121")
    a, far = c["marks"]["sink120"]
    assert hops_oracle.sink_ok(a, km, c["to_right"], frm, to) and {(a, far), (inv[far], inv[a])} <= set(r["m1"])
    assert here - there("sink120") == {(a, far), (inv[far], inv[a])} and not there("sink120") - here
    # method 2's landing at 100 | 99
    a, far = c["marks"]["landing100"]
    assert km[far] == 100 and (a, far) in r["m2"] and (a, far) not in r["m1"] and here - there("landing100") == {(a, far)}
    a, far = c["marks"]["landing99"]
    assert km[far] == 99 and (a, far) not in here and there("landing99") - here == {(a, far)}
    # MIN_RIGHT at 40 | 39: a member of can ...
    e, g = c["marks"]["can40"]
    assert km[g] == 40 and (e, g) in r["m3"] and here - there("can40") == {(e, g)}
    e, g = c["marks"]["can39"]
    assert km[g] == 39 and there("can39") - here == {(e, g)}
    # ... and of too_easy: f is 40 k-mers long, two ids show it to e, and it is not emitted because it lies directly behind e in those
    # reads: cut them back to [e] and it is.  At 39 it is no member of either set.  (The one predicate gates both sets, so a
    # too_easy member's own length cannot change the union: what decides is the can side, above.)
    e, f = c["marks"]["easy40"]
    assert km[f] == 40 and (e, f) not in here and there("easy40") - here == {(e, f)}
    e, f = c["marks"]["easy39"]
    assert km[f] == 39 and (e, f) not in here and (e, f) not in there("easy39")
    # GOOD_EXT at 100 | 99
    e, g = c["marks"]["ext100"]
    assert (e, g) not in here and (e, g) in there("ext100")
    e, g = c["marks"]["ext99"]
    assert (e, g) in r["m3"] and (e, g) not in there("ext99")
    # MIN_CAND: K k-mers skipped, K + 1 searched, two barcodes on both
    idx = hops_oracle.paths_index(c["paths"], len(km))
    e, g = c["marks"]["cand0"]
    assert km[e] == K and len({c["bc"][i] for i in idx[e]}) == 2 and e not in r["x_sizes"] and there("cand0") - here == {(e, g)}
    e, g = c["marks"]["cand1"]
    assert km[e] == K + 1 and len({c["bc"][i] for i in idx[e]}) == 2 and e in r["x_sizes"] and here - there("cand1") == {(e, g)}
    # MarkBads' sums at 150 | 151 on a pair that decides a candidate
    e, g = c["marks"]["sum150"]
    assert (e, g) in r["m3"] and (e, g) not in there("sum150")
    e, g = c["marks"]["sum151"]
    assert (e, g) not in here and (e, g) in there("sum151")
    assert sorted(set(c["sums"].tolist())) == [0, 150, 151, 65535]
    # the marks matter
    assert set(hops_cases.run(dict(c, bad=c["bad"] * 0))["pairs"]) != here


@pytest.mark.parametrize("name,c,K", [g[:3] for g in NEW], ids=[g[0] for g in NEW])
def test_gapped_chains_mate_sets_and_shapes(name, c, K):
    r = ran(name, c)
    N, inv, km = len(c["paths"]), c["inv"], c["kmers"]
    idx = hops_oracle.paths_index(c["paths"], len(km))
    bid = [N + int(x) for x in c["bc"]]
    frm, to = hops_oracle.adjacency(c["to_left"], c["to_right"])
    ids_of = lambda e1, e2: sorted(b - N for f, b in hops_oracle.mate_set(e1, idx, c["paths"], inv, bid) if f == e2)
    seen = lambda e1, e2: sum(1 for i in idx[e1] if c["paths"][i ^ 1] and inv[c["paths"][i ^ 1][-1]] == e2)
    a, far = c["marks"]["once"]
    assert seen(a, far) == 1 and len(ids_of(a, far)) == 1 and (a, far) not in r["pairs"]
    a, far = c["marks"]["many"]
    assert seen(a, far) == 6 and len(ids_of(a, far)) == 1 and (a, far) not in r["pairs"]
    a, far = c["marks"]["shared0"]
    assert ids_of(a, far) == [0, 4] and (a, far) in r["m1"]
    # method 1 refuses a supported (e1, e2) because e2 fails the source test: what ONE_GOOD adds
    refused = [(e1, e2) for e1 in range(len(km)) if hops_oracle.sink_ok(e1, km, c["to_right"], frm, to)
               for e2 in hops_oracle.supported(hops_oracle.mate_set(e1, idx, c["paths"], inv, bid)) if not hops_oracle.source_ok(e2, km, c["to_left"], frm, to)]
    assert refused and set(ran(name, c, one_good=True)["m1"]) - set(r["m1"]) == set(refused)
    # a self-inverse edge that is searched, with reads on it; a read that crosses an edge twice; a search of two rounds
    s, _ = c["marks"]["selfinv"]
    assert inv[s] == s and km[s] >= K + 1 and s in r["x_sizes"] and len(idx[s]) >= 3
    l, _ = c["marks"]["twice"]
    assert any(p.count(l) == 2 for p in c["paths"]) and l in r["x_sizes"]
    e0, _ = c["marks"]["rounds"]
    assert r["most_rounds"] >= 2 and hops_oracle.search(e0, hops_oracle.build_x(e0, idx, c["paths"], inv), km)[:2] == (True, 2)


def test_seeded_graphs_reach_the_sizes_where_the_kernels_change_path():
    """over all seeded graphs: lists longer than a wave and than a block, an X that strides past lane 63 and fits, one that does not,
    and every capacity of dfk_hops.h that these sizes can outgrow (OVER_CAN and OVER_EASY need 129 distinct edges of 40 k-mers on one
    edge's mates: not within these sizes)"""
    longest_list, fits, reasons, reasons3 = 0, [], set(), set()
    for name, c, K, _ in hops_cases.seeded():
        n = [0] * len(c["kmers"])
        for p in c["paths"]:
            for g in p: n[g] += 1; n[c["inv"][g]] += 1
        longest_list = max(longest_list, max(n))
        r = ran(name, c) if "knobs" in c else hops_cases.run(c)
        over = hops_cases.overflowing(r, 96, 24)
        fits += [nx for e, (nx, _, _, _) in r["x_sizes"].items() if e not in over]
        reasons |= {w for v in over.values() for w in v}
        reasons3 |= {w for v in hops_cases.overflowing(r, 96, 3).values() for w in v}
        if name == "dense1":
            assert sorted(n, reverse=True)[:2] == [260, 260] and sum(1 for x in n if 64 < x <= 256) >= 2
            assert {e: w for e, w in over.items()} == {c["marks"]["x106"][0]: ["X_SLOTS"], c["marks"]["exts32"][0]: ["EXT_SLOTS"], c["marks"]["ext49"][0]: ["EXT_LEN"]}
            assert r["x_sizes"][c["marks"]["x79"][0]][0] == 79 and r["x_sizes"][c["marks"]["x106"][0]][0] == 106
            assert all(any(p[0] == e for p in r["m3"]) for e in (c["marks"]["x79"][0], c["marks"]["x106"][0], c["marks"]["ext49"][0]))     # their verdicts show
    assert longest_list > 256 and any(65 <= nx <= 95 for nx in fits)
    assert reasons == {"X_SLOTS", "EXT_SLOTS", "EXT_LEN"} and "X_LEN" in reasons3
