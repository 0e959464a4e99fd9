"""The patched graph on the GPU (dfk_patch_build_arrays) at K = 40, 48 and 60 on the seeded cases of tests/patch_seeded.py: the zoo
(circles of many lengths, tandem and reverse-complement symmetric circles, a loop on a branching vertex, one-K-mer old edges, ~30 closures
of every kind) with kmers_per_batch 0, 37, 257 and 1; the aligned cases, whose heads lie on lanes 0 and 63 and on the first and last slot
of a block of 256 and whose closure positions fill whole waves with novel K-mers, with one in lane 0 or lane 63 alone, or with none; and
closures made of two fixtures' own edges.  Each run is held to tests/patch_oracle.py as tests/test_gpu_patch.py's check() does (the nine
files, the arrays, the counters, the digest, no device memory kept) and, in there, to check_invariants on what the device itself returned
and wrote.  Everything is exact."""
import faulthandler

import numpy as np
import pytest

from tests import patch_oracle as po, patch_seeded as ps
from tests.test_gpu_patch import LIMIT, arrays, check

pytestmark = pytest.mark.gpu

_want = {}


@pytest.fixture(autouse=True)
def time_limit():
    """as tests/test_gpu_patch.py: the C runtime's watchdog ends the process even inside a kernel that does not come back"""
    faulthandler.dump_traceback_later(LIMIT, exit=True)
    yield
    faulthandler.cancel_dump_traceback_later()


def case(kind, K, which):
    """(graph, closures, the oracle's result): made once and handed out unchanged"""
    if (kind, K, which) not in _want:
        g, cl = ps.seeded_case(K, which) if kind == "zoo" else ps.aligned_case(K, which)
        _want[kind, K, which] = (g, cl, po.run(g, cl))
    return _want[kind, K, which]


@pytest.fixture(scope="module")
def ctx():
    """a context per K"""
    from superplus_amd.dfk import Dfk
    made = {}

    def get(K):
        if K not in made: made[K] = Dfk(K=K)
        return made[K]
    yield get
    for d in made.values(): d.close()


def run(d, g, closures, want, tmp_path, what, batches):
    n = want["counters"]["positions"]
    for per in batches:
        held = d.stats()["hbm_held"]
        st = d.patch_build_arrays(*arrays(g, closures), per)
        assert d.stats()["hbm_held"] == held
        check(d, st, want, tmp_path, f"per{per}", f"{what} kmers_per_batch={per}", g, closures)
        assert st["batches"] == ((n + per - 1) // per if per else (1 if n else 0))
    return st


@pytest.mark.parametrize("seed", ps.SEEDS)
@pytest.mark.parametrize("K", ps.KS)
def test_zoo_matches_the_oracle(ctx, tmp_path, K, seed):
    g, closures, want = case("zoo", K, seed)
    st = run(ctx(K), g, closures, want, tmp_path, f"zoo K={K} seed={seed}", (0, 37, 257) + ((1,) if seed == ps.SEEDS[0] else ()))
    assert st["cycle_kmers"] > 0 and st["short"] >= 3 and st["bits_added"] > 0          # (the plants: tests/test_patch_seeded_cpu.py)


@pytest.mark.parametrize("variant", ps.VARIANTS)
@pytest.mark.parametrize("K", ps.KS)
def test_aligned_heads_and_waves(ctx, tmp_path, K, variant):
    g, closures, want = case("aligned", K, variant)
    what = f"aligned K={K} {variant}"
    ps.assert_coverage(g, closures, want, variant, what)                                # the case reaches what it is for, or the test says what it misses
    st = run(ctx(K), g, closures, want, tmp_path, what, (0, 37, 257))
    # the device's own heads are where the case put them
    got = ctx(K).patch_fetch()
    first = [int(x) for x in got["to3_first"]]
    mine = dict(to3=[[int(x) for x in got["to3"][a:b]] for a, b in zip(first, first[1:])], left3=[int(x) for x in got["left3"]], kmers3=[int(x) for x in got["kmers"]])
    assert set(ps.AFTER) | set(ps.BEFORE) <= set(ps.head_slots(g, mine)[0]), what
    assert st["positions"] % 256 == ps.VARIANTS.index(variant)


@pytest.mark.parametrize("fixture,K", [("graph_k40_nobc", 40), ("graph_k60_nobc", 60), ("graph_zoo_k48", 48)])
def test_closures_of_a_fixtures_own_edges(ctx, golden_dir, tmp_path, fixture, K):
    """146 and 312 edges of real reads' graphs, and one zoo fixture (1334 edges, some 38 000 slots: 150 blocks of 256; the oracle takes 1.5 s on it;
    the zoo at K = 60 takes 2.3 s and is left to the no-closure test)"""
    g = po.fixture_graph(golden_dir, fixture, K)
    closures = ps.closures_for(g, np.random.default_rng([K, 7004]), 2)
    want = po.run(g, closures)
    assert want["counters"]["new_unique"] > 0 and want["counters"]["bits_added"] > 0 and want["counters"]["path2"] + want["counters"]["path3"] > 0
    run(ctx(K), g, closures, want, tmp_path, fixture, (0, 37))
