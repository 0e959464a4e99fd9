"""tests/translate_oracle.py pinned: every case of tests/translate_cases.py fires what it is there for, by the oracle's own result; the
writer and the digest against the project's other restatement of a.paths; and a fact that needs no device -- with NO closures, to3[e] = [e]
and left3 = 0 (the patched graph is the graph), so on every graph fixture that holds a reference-written a.paths the translation is that
file with every non-empty path cut to its first edge and every offset unchanged: the pather's offset < kmers(e0) < Bases(e0) lets the
first edge take every read.  CPU only."""
import os

import numpy as np
import pytest

from tests import translate_cases as tc, translate_oracle as to
from tests.hops_oracle import fixture_graph
from tests.test_paths_oracle import decode_paths

FIXTURES = [("graph_frag_k48", 48), ("graph_hot_k48_minfreq2", 48), ("graph_k40_nobc", 40), ("graph_k48", 48), ("graph_k60_nobc", 60), ("graph_pathy2_k48", 48), ("graph_pathy_k48", 48),
            ("graph_special_k48", 48), ("graph_zoo_k40", 40), ("graph_zoo_k48", 48), ("graph_zoo_k60", 60)]
NAMES = ("empty_before", "no_to3", "negative", "bases_kmers", "walks", "circle", "one_kmer", "ranoff_neg", "overlaps", "break", "random", "pather")


def test_every_fixture_with_paths_is_listed(golden_dir):
    assert sorted(c for c, _ in FIXTURES) == sorted(d for d in os.listdir(golden_dir) if os.path.exists(os.path.join(golden_dir, d, "a.paths")))


def test_all_cases_are_there():
    assert tuple(tc.all_cases()) == NAMES


@pytest.mark.parametrize("name", NAMES)
def test_case_fires_what_it_is_there_for(name):
    c = tc.all_cases()[name]
    r = tc.run(c)
    tc.fires(name, c, r)
    n = r["counters"]
    assert n["placed"] == n["step2"] + n["walk"] and n["placed_before"] == n["placed"] + n["cleared_empty"] + n["cleared_ranoff"]
    assert n["var_bytes"] == 8 * n["reads"] + 4 * n["placed"] == len(r["file"]) - 24 - 8 * (n["reads"] + 1)
    assert all(len(e) <= 1 for _, e in r["paths"])                             # "this truncates to length 1"


def test_overlap_append_by_its_loop():
    for v1, v2, want, best in (([], [1, 2], [1, 2], 0), ([1, 2], [3], [1, 2, 3], 0), ([1, 2], [2, 3], [1, 2, 3], 1), ([1, 2], [1, 2], [1, 2], 2),
                               ([1, 2, 3, 4, 3, 4], [3, 4, 3, 4, 5, 6], [1, 2, 3, 4, 3, 4, 5, 6], 4), ([7, 7], [7, 7, 7], [7, 7, 7], 2), ([1], [], [1], 0)):
        p = list(v1)
        assert to.overlap_append(p, v2) == best and p == want


def test_writer_and_digest_agree_with_the_paths_restatement():
    """the file against oracle/paths_oracle.py's writer, and back through the reader the paths tests use; the digest against the numpy form
    tests/verify_oracle.py checks dfk_paths_digest with"""
    from oracle import paths_oracle, verify_oracle
    paths = tc.run(tc.random_case())["paths"] + [(0, []), (-7, [3, 4, 5])]
    f = to.paths_file(paths)
    assert f == paths_oracle.paths_file(paths) and decode_paths(f) == paths
    assert tuple(int(x) for x in verify_oracle.paths_digest(paths)) == to.paths_digest(paths)


@pytest.mark.parametrize("case,K", FIXTURES)
def test_without_closures_the_paths_are_cut_to_their_first_edge(golden_dir, case, K):
    kmers = [int(x) for x in fixture_graph(golden_dir, case, K)[0]]
    paths = decode_paths(open(os.path.join(golden_dir, case, "a.paths"), "rb").read())
    E = len(kmers)
    assert all(o < kmers[p[0]] for o, p in paths if p)                          # what makes the first edge take every read
    r = to.run(paths, [[e] for e in range(E)], [0] * E, kmers, K)
    assert r["paths"] == [(o, p[:1]) for o, p in paths]
    n = r["counters"]
    assert (n["step2"], n["walk"], n["host"], n["cleared_empty"], n["cleared_ranoff"], n["offset_changed"], n["edge_changed"], n["invalid"]) == (n["placed_before"], 0, 0, 0, 0, 0, 0, 0)
    assert r["file"] == to.paths_file([(o, p[:1]) for o, p in paths]) and n["placed_before"] > 0
