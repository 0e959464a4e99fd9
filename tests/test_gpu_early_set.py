"""The adjacency clean-up's set of boundary k-mers is allocated when the last pass's count is about to start, cut to the
largest free block, and filled from the finished parts' lists on the second stream while that count runs; the stage then
adds the last part and looks up, or discards the set and builds one as before (dfk.hip: plan_early_set, launch_early_set,
stage_adjacency; dfk_adj_plan.h).  Every way through must give the oracle's dictionary before and after the clean-up and
what the DFK_NO_EARLY_SET=1 run of the same input under the same settings gives (solid set, spectrum, digests, adj_probes,
n_passes), and dfk_adj_outcome must name the way taken -- so that a silent fallback cannot pass.

adj_probes counts the context bits k_count could not settle inside an item's table, and the items follow the budget and
DFK_NO_OVERLAP; a run is therefore compared with the DFK_NO_EARLY_SET=1 run at the same budget and switches.

Budgets are derived from the runs' own hbm_bytes_peak: the smallest budget at which the DFK_NO_EARLY_SET=1 run still
completes is found by confining the run to its peak and halving the bracket that leaves (_tight_budget)."""
import numpy as np
import pytest

from tests import util

pytestmark = pytest.mark.gpu

E_NOMEM = -4
OFF = {"DFK_NO_EARLY_SET": "1"}
_CACHE = {}


def _input(golden_dir, which):
    if ("in", which) not in _CACHE:
        if which == "hot":
            from tests.test_oracle_golden import load_hot
            _CACHE["in", which] = (load_hot(golden_dir), 2)
        else:
            _CACHE["in", which] = (util.make_set(91, 60000, 6000), 3)
    return _CACHE["in", which]


def _ref(oracle, golden_dir, which, K):
    """The oracle's result, computed once per input and K and left unchanged."""
    if ("ref", which, K) not in _CACHE:
        rs, min_freq = _input(golden_dir, which)
        _CACHE["ref", which, K] = oracle.run(rs["packed"], rs["base_off"], rs["read_len"], rs["pq_bytes"], rs["pq_off"], rs["bc"], K=K, min_freq=min_freq)
    return _CACHE["ref", which, K]


def _run(monkeypatch, oracle, golden_dir, which, K, passes, env=None, budget=0, light=False):
    """One count under `env`.  light: only the statistics, or None if the budget was too small (DFK_E_NOMEM); otherwise
    parity with the oracle is checked and everything the runs are compared by comes back."""
    from superplus_amd.dfk import Dfk, DfkError
    rs, min_freq = _input(golden_dir, which)
    with monkeypatch.context() as mp:
        for k in ("DFK_NO_EARLY_SET", "DFK_EARLY_SET_SCALE", "DFK_NO_OVERLAP"):
            mp.delenv(k, raising=False)
        for k, v in (env or {}).items():
            mp.setenv(k, v)
        d = Dfk(K=K, keep_pre_adjacency=True, min_freq=min_freq, passes=passes, hbm_budget_bytes=budget)
        try:
            try:
                d.count(rs["packed"], rs["base_off"], rs["read_len"], rs["pq_bytes"], rs["pq_off"], rs["bc"])
            except DfkError as e:
                if light and e.code == E_NOMEM:
                    return None
                raise
            st = d.stats()
            outcome, slots = d.adj_outcome()
            if light:
                return dict(st=st, outcome=outcome, slots=slots)
            util.check_parity(_ref(oracle, golden_dir, which, K), d)
            return dict(st=st, outcome=outcome, slots=slots, solid=d.solid(), spectrum=d.spectrum(), digest=d.digest(),
                        digest_pre=d.digest(pre_adjacency=True))
        finally:
            d.close()


def _same(a, b, what):
    util.assert_same_solid(a["solid"], b["solid"], what)
    assert np.array_equal(a["spectrum"], b["spectrum"]), what
    assert a["digest"] == b["digest"] and a["digest_pre"] == b["digest_pre"], what
    for k in ("adj_probes", "n_passes", "n_solid"):
        assert a["st"][k] == b["st"][k], (what, k, a["st"][k], b["st"][k])


def _tight_budget(monkeypatch, oracle, golden_dir, which, K, passes, eps):
    """The smallest budget, to within eps, at which the DFK_NO_EARLY_SET=1 run completes -- plus eps, so that the counts
    that vary from run to run (a KB of peak) cannot make it fail.  From the run's own peak at the default budget: a run
    confined to its peak either fits (its scratch follows the free room) or leaves a bracket to halve."""
    def peak_at(budget):
        r = _run(monkeypatch, oracle, golden_dir, which, K, passes, env=OFF, budget=budget, light=True)
        return None if r is None else r["st"]["hbm_bytes_peak"]
    hi, lo = peak_at(0), 0
    assert peak_at(hi) is not None, "the run does not fit the peak it had at the default budget"
    for _ in range(8):
        p = peak_at(hi)
        if p >= hi:
            break
        if peak_at(p) is None:
            lo = p
            break
        hi = p
    while hi - lo > eps:
        mid = (lo + hi) // 2
        if peak_at(mid) is None:
            lo = mid
        else:
            hi = mid
    return hi + eps


@pytest.mark.parametrize("passes", [1, 2, 5])
@pytest.mark.parametrize("K", [40, 48])
@pytest.mark.parametrize("which", ["hot", "synthetic"])
def test_early_set_gives_what_the_late_set_gives(oracle, golden_dir, monkeypatch, which, K, passes):
    """Default budget: parity with the oracle (pre- and post-adjacency views), everything equal to the DFK_NO_EARLY_SET=1 run.
    On the synthetic set the early set must have been used with 2 and 5 passes, with look-ups made; one pass has no last
    count with finished parts: not applicable."""
    early = _run(monkeypatch, oracle, golden_dir, which, K, passes)
    late = _run(monkeypatch, oracle, golden_dir, which, K, passes, env=OFF)
    _same(early, late, f"{which} K={K} passes={passes}")
    assert early["st"]["n_passes"] == passes
    if passes == 1:
        assert early["outcome"] == "not applicable" and late["outcome"] == "not applicable"
    elif which == "synthetic":
        assert early["outcome"] == "used", early["outcome"]
        assert early["st"]["adj_probes"] > 0 and early["slots"] > 0
        assert late["outcome"] == "switched off", late["outcome"]
    else:
        assert early["outcome"] in ("used", "not applicable") and late["outcome"] in ("switched off", "not applicable")


@pytest.mark.parametrize("passes", [2, 5])
@pytest.mark.parametrize("K", [40, 48])
def test_guess_too_low_is_discarded(oracle, golden_dir, monkeypatch, K, passes):
    """DFK_EARLY_SET_SCALE=0.01: a set for a hundredth of the keys; the final count fails the load test, the set is
    discarded and built again after the count."""
    low = _run(monkeypatch, oracle, golden_dir, "synthetic", K, passes, env={"DFK_EARLY_SET_SCALE": "0.01"})
    late = _run(monkeypatch, oracle, golden_dir, "synthetic", K, passes, env=OFF)
    assert low["outcome"] == "discarded: guess too low", low["outcome"]
    assert low["st"]["adj_probes"] > 0
    _same(low, late, f"K={K} passes={passes} scale 0.01")


@pytest.mark.parametrize("passes", [2, 5])
@pytest.mark.parametrize("K", [40, 48])
def test_one_stream_is_not_applicable(oracle, golden_dir, monkeypatch, K, passes):
    """DFK_NO_OVERLAP=1: no second stream to fill the set on."""
    one = _run(monkeypatch, oracle, golden_dir, "synthetic", K, passes, env={"DFK_NO_OVERLAP": "1"})
    late = _run(monkeypatch, oracle, golden_dir, "synthetic", K, passes, env={"DFK_NO_OVERLAP": "1", **OFF})
    assert one["outcome"] == "not applicable" and late["outcome"] == "not applicable"
    _same(one, late, f"K={K} passes={passes} one stream")


@pytest.mark.parametrize("passes", [2, 5])
@pytest.mark.parametrize("K", [40, 48])
def test_no_block_at_a_tight_budget(oracle, golden_dir, monkeypatch, K, passes):
    """The smallest budget the run completes in (from its own peak, to within a quarter of the set it used at the default
    budget): what is free when the last count starts is what that pass still has to allocate, which the set leaves
    alone -- no block holds it.  The run completes, with parity, and the set is built after the count.  (The run's peak at
    the default budget is not such a budget: there the scan's scratch, which follows the free room, sets the peak -- 319.8 MB
    at K=48 with two passes against 306.8 MB in the tight budget of 307.6 MB -- and 12 MB are free at the last count.)"""
    used = _run(monkeypatch, oracle, golden_dir, "synthetic", K, passes, light=True)
    assert used["outcome"] == "used" and used["slots"] >= 1024
    budget = _tight_budget(monkeypatch, oracle, golden_dir, "synthetic", K, passes, eps=used["slots"] * 16 // 4)
    tight = _run(monkeypatch, oracle, golden_dir, "synthetic", K, passes, budget=budget)
    late = _run(monkeypatch, oracle, golden_dir, "synthetic", K, passes, env=OFF, budget=budget)
    print(f"K={K} passes={passes}: default peak {used['st']['hbm_bytes_peak']}, tight budget {budget}, peak there {tight['st']['hbm_bytes_peak']}, "
          f"outcome {tight['outcome']}, slots {tight['slots']} (default budget: {used['slots']})")
    assert tight["outcome"] == "no block", tight["outcome"]
    assert tight["slots"] > 0 and tight["st"]["adj_probes"] > 0
    _same(tight, late, f"K={K} passes={passes} budget {budget}")


@pytest.mark.parametrize("K", [40, 48])
def test_hot_fixture_at_a_tight_budget(oracle, golden_dir, monkeypatch, K):
    """The hot fixture (a bucket that takes the fallback's allocations) with two passes, in a budget just above its peak
    without the set: the run completes with parity, never an error, and the early set either found no block or was
    dropped for an allocation.  (With two passes the fixture's hot bucket, 39961 instances, lies in the FIRST range and is
    counted in sub-passes at this budget; the last pass's fallback has nothing to allocate, and what is free when it
    starts -- a few KB above what it still needs -- is less than the set leaves alone for the pass: "no block" on the
    MI355X, K=40 and 48.)"""
    used = _run(monkeypatch, oracle, golden_dir, "hot", K, 2, light=True)
    budget = _tight_budget(monkeypatch, oracle, golden_dir, "hot", K, 2, eps=max(used["slots"], 1024) * 16 // 4)
    tight = _run(monkeypatch, oracle, golden_dir, "hot", K, 2, budget=budget)
    late = _run(monkeypatch, oracle, golden_dir, "hot", K, 2, env=OFF, budget=budget)
    print(f"K={K}: default peak {used['st']['hbm_bytes_peak']}, tight budget {budget}, peak there {tight['st']['hbm_bytes_peak']}, outcome {tight['outcome']}")
    assert tight["outcome"] in ("no block", "dropped for an allocation"), tight["outcome"]
    _same(tight, late, f"hot K={K} budget {budget}")
