"""tests/patch_oracle.py held to the reference's own files and to what the plants of tests/patch_cases.py must fire.  CPU only.

With no closures the patched graph must BE the graph: BuildAll's edges and crossings, kmerized without counts and without
recomputeAdjacencies, give on every fixture the eight files the reference wrote (palindromes, cycle and hairpins of graph_special_k48
included), every old edge's path is its own id and every left3 is 0 -- the contexts the count leaves after its adjacency clean-up say
exactly what the crossings say."""
import os

import pytest

from tests import patch_cases, patch_oracle as po
from tests.test_sclosures_cpu import FIXTURES, LARGEST


@pytest.mark.parametrize("case,K,which", FIXTURES + (LARGEST,), ids=[f[0] for f in FIXTURES + (LARGEST,)])
def test_without_closures_the_patched_graph_is_the_graph(golden_dir, case, K, which):
    g = po.fixture_graph(golden_dir, case, K)
    r = po.run(g, [])
    for f in po.FILES:
        assert r["files"]["a.patch." + f[2:]] == open(os.path.join(golden_dir, case, f), "rb").read(), f
    E = len(g["edges"])
    assert r["to3"] == [[e] for e in range(E)] and r["left3"] == [0] * E
    c = r["counters"]
    assert (c["edges3"], c["vertices3"], c["new_unique"], c["bits_added"], c["to3"], c["left3"]) == (E, g["n_vertices"], 0, 0, E, 0)


@pytest.fixture(scope="module")
def runs(oracle):
    return {name: (g, cl, po.run(g, cl)) for name, g, cl in patch_cases.all_cases(oracle)}


def lens(r):
    return [len(p) for p in r["to3"]]


def test_every_plant_fires(runs):
    K = patch_cases.K
    g, _, r = runs["plain"]
    assert r["to3"] == [[e] for e in range(4)] and r["left3"] == [0] * 4 and r["hbv"].edges == g["edges"]
    g, _, r = runs["join"]                                                   # three things become one edge; 75 positions = three batches of 37
    c = r["counters"]
    assert c["canonical3"] == 1 and c["edges3"] == 2 and c["positions"] == 75 and c["new_unique"] == 69 and c["bits_added"] == 2
    assert sorted(r["left3"]) == [0, 0, 192, 222] and lens(r) == [1] * 4
    assert runs["reversed"][2]["files"] == r["files"] and runs["reversed"][2]["to3"] == r["to3"]
    g, _, r = runs["interior"]
    assert sorted(lens(r)) == [2, 2, 3, 3] and all(lens(r)[e] == lens(r)[g["inv"][e]] for e in range(4)) and r["left3"] == [0] * 4
    inv3 = r["inv3"]
    for e in range(4):                                                       # the path of inv[e] is e's reversed through hb3's involution
        assert r["to3"][g["inv"][e]] == [inv3[x] for x in reversed(r["to3"][e])]
    c = runs["onlyold"][2]["counters"]
    assert c["new"] == 0 and c["bits_added"] == 0 and c["found"] == c["positions"] == 53 and runs["onlyold"][2]["files"] == runs["plain"][2]["files"]
    c = runs["bit"][2]["counters"]
    assert (c["positions"], c["found"], c["new"], c["bits_added"]) == (2, 2, 0, 2) and lens(runs["bit"][2]) == [2] * 4
    c = runs["lengths"][2]["counters"]
    assert (c["short"], c["positions"], c["new_unique"], c["single3"], c["canonical3"]) == (1, 3, 3, 1, 3)
    assert sorted(len(s) for s in runs["lengths"][2]["edges3"]) == [K, K + 1, 200]
    _, cl, r = runs["selfrc"]
    assert cl[0] == po.go.rc_seq(cl[0]) and r["counters"]["new"] == 33 and r["counters"]["new_unique"] == 17 and r["counters"]["single3"] == 1
    assert any(len(s) == K and s == po.go.rc_seq(s) for s in r["edges3"])     # the novel palindrome, an edge of its own
    c = runs["twice"][2]["counters"]
    assert c["new"] == 198 and c["new_unique"] == 99
    g, _, r = runs["cycle"]
    assert r["counters"]["canonical3"] == 1 and r["to3"] == [[0, 0], [1, 1]] and r["left3"] == [60, 157] and r["kmers3"] == [160, 160]
    assert r["to_left3"] == r["to_right3"]                                    # a cycle: the edge comes back to its vertex
    g, _, r = runs["selfinv"]
    assert sum(1 for e in range(len(g["edges"])) if g["inv"][e] == e) == 1 and r["counters"]["single3"] == 1 and r["counters"]["crossings"] == 4
    g, _, r = runs["cross"]
    to, frm = po.adjacency(g)
    assert any(len(to[v]) == 2 and len(frm[v]) == 2 for v in range(g["n_vertices"])) and r["counters"]["crossings"] == 8
    assert r["hbv"].edges == g["edges"] and lens(r) == [1] * 8
    g, cl, r = runs["random"]
    c = r["counters"]
    assert c["closures"] == 10 and c["short"] == 1 and c["new_unique"] == 334 and c["bits_added"] == 11 and c["canonical3"] == 10 and c["left3"] == 9


def test_to3_file_and_digest(runs):
    import struct
    _, _, r = runs["interior"]
    f = r["files"]["a.patch.to3"]
    n = sum(lens(r))
    assert f[:8] == b"DFKPTO31" and struct.unpack_from("<QQ", f, 8) == (4, n) and len(f) == 24 + 8 * 5 + 4 * n + 4 * 4
    assert r["digest"] != runs["plain"][2]["digest"] and r["digest"] == po.to3_digest(r["to3"], r["left3"])


# fixture: closures (per pair Stackster's, then CloseGap2's: the oracles' of tests/sclosures_oracle.py and tests/closures_oracle.py), novel K-mers, context bits added,
# hb3's canonical edges / vertices / edges, to3 entries, nonzero left3
TABLE = {
    "graph_special_k48": (12, 95, 2, 14, 30, 27, 23, 0),
    "graph_k40_nobc": (1, 68, 6, 72, 270, 144, 148, 5),
    "graph_k48": (0, 0, 0, 131, 514, 262, 262, 0),
    "graph_pathy_k48": (3, 83, 6, 205, 332, 410, 404, 0),
    "graph_frag_k48": (657, 2171, 339, 931, 1736, 1862, 2000, 245),
    "graph_pathy2_k48": (73, 317, 48, 1620, 3304, 3240, 3232, 24),
}


def fixture_closures(golden_dir, case, K, which):
    """the combined list (RunStages.cc:290-325) as the two closers' oracles give it"""
    import numpy as np
    from tests import closures_oracle, sclosures_oracle
    s, g = sclosures_oracle.fixture_sclosures(golden_dir, case, K, which), closures_oracle.fixture_closures(golden_dir, case, K, which)
    out = []
    for a, b in zip(s["per"], g["per"]):
        out += [bytes(np.asarray(x["bases"], np.uint8)) for x in a] + [bytes(np.asarray(x["bases"], np.uint8)) for x in b]
    return out


@pytest.mark.parametrize("case,K,which", FIXTURES + (LARGEST,), ids=[f[0] for f in FIXTURES + (LARGEST,)])
def test_fixture_table(golden_dir, case, K, which):
    g = po.fixture_graph(golden_dir, case, K)
    r = po.run(g, fixture_closures(golden_dir, case, K, which))
    c = r["counters"]
    assert (c["closures"], c["new_unique"], c["bits_added"], c["canonical3"], c["vertices3"], c["edges3"], c["to3"], c["left3"]) == TABLE[case]
    inv3 = r["inv3"]
    for e in range(len(g["edges"])):                                          # the inv route holds on real closures too
        assert r["to3"][g["inv"][e]] == [inv3[x] for x in reversed(r["to3"][e])]
