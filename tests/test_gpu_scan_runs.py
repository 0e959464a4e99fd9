"""The runs the counting scan cuts: a run ends where the bucket of the k-mers' minimizer changes or at NK_MAX k-mers, and
whatever the scan's position loop is made of, the records, instances and items of a step are those of that rule.  Each case
runs at K = 40, 48 and 60 with the run keys forced on (DFK_SCAN_KEY_PIECE) and forced off (DFK_SCAN_NO_KEYS) and checks
  - the dictionary against the CPU oracle (util.run_both / check_parity), and
  - n_records, n_inst and n_items against tests/golden/scan_runs_expected.json, recorded from the build before the scan's
    position loop was shortened (`python -m tests.test_gpu_scan_runs record` writes the file from whatever library is loaded;
    recording also checks n_records against the restatement of the rule in numpy below).
The cases: few buckets (16-64, so that successive minimizers share a bucket often), poly-A and dinucleotide repeats between
random flanks (nk reaches NK_MAX), 300-base reads with more than ten runs and reads with more than ten minimizer changes
but at most ten runs, lengths around the blocks of W m-mer positions with the last read ending on the last byte of a
packed buffer that is no multiple of four bytes, and the owner interleave of two ranks."""
import functools
import json
import os

import numpy as np
import pytest

from tests import util

pytestmark = pytest.mark.gpu

M = 16
MMER_SALT = 0x2C6B39D1
Q = 35
KS = (40, 48, 60)
EXPECTED = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "scan_runs_expected.json")
KEY_MODES = {"keys": {"DFK_SCAN_KEY_PIECE": "512"}, "no keys": {"DFK_SCAN_NO_KEYS": "1"}}


# ---- the rule, in numpy
def _mix32(x):
    x = x ^ (x >> np.uint64(15))
    x = (x * np.uint64(0x2C1B3C6D)) & np.uint64(0xFFFFFFFF)
    return x ^ (x >> np.uint64(12))


def _minimizers(codes, K):
    """The minimum canonical m-mer hash of every k-mer of a read (empty below K + 1 bases: such a read emits nothing)."""
    L = len(codes)
    if L < K + 1:
        return np.zeros(0, np.uint64)
    c = codes.astype(np.uint64)
    n_m = L - M + 1
    f = np.zeros(n_m, np.uint64); rc = np.zeros(n_m, np.uint64)
    for j in range(M):
        f |= c[j:j + n_m] << np.uint64(2 * (M - 1 - j))
        rc |= (np.uint64(3) - c[j:j + n_m]) << np.uint64(2 * j)
    h = _mix32(np.minimum(f, rc) ^ np.uint64(MMER_SALT))
    return np.lib.stride_tricks.sliding_window_view(h, K - M + 1).min(axis=1)


def _runs(mins, K, log2_nb):
    """-> (runs, changes of minimizer hash, longest run) of one read at 2^log2_nb buckets (one rank: no interleave)."""
    if len(mins) == 0:
        return 0, 0, 0
    b = ((mins * np.uint64(0x9E3779B1)) & np.uint64(0xFFFFFFFF)) >> np.uint64(32 - log2_nb)
    nk_max = 95 - K
    cuts = np.flatnonzero(b[1:] != b[:-1]) + 1
    seg = np.diff(np.concatenate([[0], cuts, [len(b)]]))          # stretches of one bucket, each cut every nk_max k-mers
    return int(((seg + nk_max - 1) // nk_max).sum()), int((mins[1:] != mins[:-1]).sum()), int(min(seg.max(), nk_max))


def _log2_nb(n_inst):
    v, l = n_inst // 850 + 1, 0
    while (1 << l) < v:
        l += 1
    return min(max(l, 4), 28)


def _n_inst(reads, K):
    return sum(len(r) - K + 1 for r in reads if len(r) >= K + 1)


# ---- read sets
def _pack(reads):
    """Reads (arrays of base codes) packed back to back, constant Q35 (nothing is trimmed), a barcode per pair."""
    from superplus_amd import feudal
    n = len(reads)
    lens = np.array([len(r) for r in reads], np.uint32)
    base_off = np.concatenate([[0], np.cumsum((lens.astype(np.uint64) + 3) // 4)]).astype(np.uint64)
    packed = np.concatenate([feudal.pack_bases(r[None, :]).reshape(-1) for r in reads])
    assert len(packed) == int(base_off[-1])
    blocks = {}
    pqs = [blocks.setdefault(len(r), np.frombuffer(feudal.pq_encode(np.full(len(r), Q, np.uint8)), np.uint8)) for r in reads]
    pq_off = np.concatenate([[0], np.cumsum([len(x) for x in pqs])]).astype(np.uint64)
    bc = (1 + np.arange(n) // 2 % 9).astype(np.int32)
    return dict(packed=packed, base_off=base_off, read_len=lens, pq_bytes=np.concatenate(pqs), pq_off=pq_off, bc=bc, n_reads=n)


def _drawer(rng, genome, err=0.005):
    def draw(L):
        a = int(rng.integers(0, len(genome) - L))
        r = genome[a:a + L].copy()
        if rng.random() < 0.5:
            r = (3 - r[::-1]).astype(np.uint8)
        hit = rng.random(L) < err
        r[hit] = (r[hit] + rng.integers(1, 4, int(hit.sum()))) & 3
        return r
    return draw


def _few_buckets(K):
    """2000 short reads over a 3 kb genome: 16-64 buckets, so that a change of minimizer often stays in its bucket."""
    rng = np.random.default_rng(100 + K)
    draw = _drawer(rng, rng.integers(0, 4, 3000, dtype=np.uint8))
    reads = [draw(int(L)) for L in rng.integers(K + 1, K + 26, 2000)]
    assert 4 <= _log2_nb(_n_inst(reads, K)) <= 6
    return reads


def _repeats(K):
    """Poly-A and dinucleotide repeats of 60-200 bases between random flanks of 0-80: nk reaches NK_MAX inside the repeat,
    and a run that begins in a flank crosses NK_MAX inside it."""
    rng = np.random.default_rng(200 + K)
    units = [[0], [3], [0, 3], [0, 1], [1, 2], [2, 0]]
    reads = []
    for i in range(1500):
        u = units[i % len(units)]
        rep = np.resize(np.array(u, np.uint8), int(rng.integers(60, 201)))
        fl = [rng.integers(0, 4, int(rng.integers(0, 81)), dtype=np.uint8) for _ in range(2)]
        reads.append(np.concatenate([fl[0], rep, fl[1]]))
    return reads


def _long(K):
    """The 300-base pairs of util.make_long_set (more than ten runs at every K) as plain reads."""
    rs = util.make_long_set(300 + K, 40_000, 600)
    L = int(rs["read_len"][0])
    nb = (L + 3) // 4
    by = rs["packed"].reshape(-1, nb)
    codes = np.stack([(by >> s) & 3 for s in (0, 2, 4, 6)], axis=2).reshape(len(by), -1)[:, :L].astype(np.uint8)
    return list(codes)


def _many_changes(K):
    """48 reads (12 at K = 60), so few k-mers that the set gets 16 buckets, each with more than ten changes of minimizer and at most ten
    runs by the bucket rule: ten slots of runs are enough for them, and they are no overflow reads.  (A minimizer lasts
    (W + 1) / 2 k-mers on average: the reads are long enough for eleven.)"""
    rng = np.random.default_rng(400 + K)
    draw = _drawer(rng, rng.integers(0, 4, 20_000, dtype=np.uint8), err=0.0)
    # (at K = 60 a bucket's stretch is also cut at NK_MAX = 35 k-mers, and three reads in a thousand qualify: twelve of them)
    L = K - 1 + (11 if K < 60 else 9) * (K - M + 2) // 2
    reads = []
    while len(reads) < (48 if K < 60 else 12):
        r = draw(L)
        runs, changes, _ = _runs(_minimizers(r, K), K, 4)
        if changes > 10 and runs <= 10:
            reads.append(r)
    assert _log2_nb(_n_inst(reads, K)) == 4
    return reads


def _lengths(K):
    """n_mmers = W-1, W, W+1, 2W-1, 2W, 2W+1, 3W (lengths K-1, K, K+1, ...: the first two emit nothing) at every byte phase
    of a word, among reads of 100-300 bases; the last read ends on the last byte of packed, which is no multiple of 4."""
    rng = np.random.default_rng(500 + K)
    draw = _drawer(rng, rng.integers(0, 4, 40_000, dtype=np.uint8))
    W = K - M + 1
    special = sorted({n + M - 1 for n in (W - 1, W, W + 1, 2 * W - 1, 2 * W, 2 * W + 1, 3 * W)} | {K, K + 1})
    reads, byte_at = [], 0
    for rep in range(6):
        for L in special:
            for phase in range(4):
                pad = draw(int(rng.integers(100, 301)))
                while (byte_at + (len(pad) + 3) // 4) % 4 != phase:
                    pad = np.concatenate([pad, draw(4)])
                for r in (pad, draw(L)):
                    reads.append(r); byte_at += (len(r) + 3) // 4
    while len(reads) < 1999:
        r = draw(int(rng.integers(100, 301)))
        reads.append(r); byte_at += (len(r) + 3) // 4
    last = draw(3 * W + M - 1)
    while (byte_at + (len(last) + 3) // 4) % 4 != 1:
        last = np.concatenate([last, draw(4)])
    reads.append(last)
    return reads


CASES = {"few buckets": _few_buckets, "repeats": _repeats, "long": _long, "many changes": _many_changes, "lengths": _lengths}


@functools.lru_cache(maxsize=None)
def _case(name, K):
    reads = CASES[name](K)
    return _pack(reads), reads


@functools.lru_cache(maxsize=None)
def _expected():
    with open(EXPECTED) as f:
        return json.load(f)


def _count(oracle, rs, K, env):
    mp = pytest.MonkeyPatch()
    try:
        for k, v in env.items():
            mp.setenv(k, v)
        ref, d = util.run_both(oracle, rs, K=K, min_freq=2)
        st = util.check_parity(ref, d)
        d.close()
    finally:
        mp.undo()
    return {k: int(st[k]) for k in ("n_records", "n_inst", "n_items", "n_buckets")}


def _replica_rank(rs, K, world=2):
    """Rank 0 of `world` against replicas of itself: the scan by class, buckets laid out owner-major."""
    import torch
    from superplus_amd.dist import DistDfk, ReplicaComm
    dev = torch.device("cuda", 0)
    t = lambda x, dt: torch.from_numpy(np.ascontiguousarray(x).astype(dt)).to(dev)
    d = DistDfk(K=K, device=0, comm=ReplicaComm(world))
    d.count_device(t(rs["packed"], np.uint8), t(rs["base_off"], np.int64), t(rs["read_len"], np.int32), t(rs["pq_bytes"], np.uint8),
                   t(rs["pq_off"], np.int64), t(rs["bc"], np.int32), read_id0=0)
    st = d.stats()
    out = {k: int(st[k]) for k in ("n_records", "n_inst", "n_items", "n_distinct")}
    out["digest"] = [int(x) for x in d.digest()]
    d.close()
    return out


@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("name", list(CASES))
def test_runs_match_oracle_and_recorded_counts(oracle, name, K):
    rs, reads = _case(name, K)
    if name == "lengths":
        assert len(rs["packed"]) % 4 == 1 and int(rs["base_off"][-1]) == len(rs["packed"])
    exp = _expected()[f"{name}/K{K}"]
    for mode, env in KEY_MODES.items():
        got = _count(oracle, rs, K, env)
        print(f"{name} K={K} {mode}: {got}")
        for k in ("n_records", "n_inst", "n_items"):
            assert got[k] == exp[k], (name, K, mode, k, got[k], exp[k])


@pytest.mark.parametrize("K", KS)
def test_two_ranks_owner_interleave(oracle, K):
    """The buckets of a sharded scan are laid out owner-major (bucket_of with log2_world = 1): two ranks in one process
    against the oracle, and rank 0 of two against replicas of itself (ReplicaComm) against the recorded counts."""
    import torch
    from superplus_amd.dist import DistDfk, run_inprocess
    from tests.test_gpu_shard import _shards
    rs, _ = _case("few buckets", K)
    ref = oracle.run(rs["packed"], rs["base_off"], rs["read_len"], rs["pq_bytes"], rs["pq_off"], rs["bc"], K=K)
    ranks = [DistDfk(K=K, device=0) for _ in range(2)]
    n_global = run_inprocess(ranks, _shards(rs, 2, torch.device("cuda", 0)))
    assert n_global == ref["n_inst"]
    allk = np.concatenate([d.solid() for d in ranks])
    util.assert_same_solid(allk[np.lexsort((allk["w1"], allk["w0"]))], ref["solid"], f"two ranks, K={K}")
    for d in ranks:
        d.close()
    got = _replica_rank(rs, K)
    print(f"replica rank K={K}: {got}")
    assert got == _expected()[f"replica/K{K}"]


def _record():
    """Writes the expected counts from the library that is loaded; every count must be the same with and without keys, and
    n_records that of the rule restated above."""
    from oracle import pyoracle
    pyoracle.lib()
    out = {}
    for name in CASES:
        for K in KS:
            rs, reads = _case(name, K)
            got = [_count(pyoracle, rs, K, env) for env in KEY_MODES.values()]
            assert got[0] == got[1], (name, K, got)
            lb = _log2_nb(got[0]["n_inst"])
            assert got[0]["n_buckets"] == 1 << lb
            per = [_runs(_minimizers(r, K), K, lb) for r in reads]
            assert got[0]["n_records"] == sum(p[0] for p in per), (name, K)
            assert got[0]["n_inst"] == _n_inst(reads, K)
            if name == "few buckets":
                assert sum(p[1] + 1 for p in per if p[0]) > got[0]["n_records"], "minimizers that share a bucket"
            if name == "repeats":
                assert sum(1 for p in per if p[2] == 95 - K) > 500, "runs of NK_MAX k-mers"
            if name == "long":
                assert sum(1 for p in per if p[0] > 10) > 100, "reads with more than ten runs"
            if name == "many changes":
                assert all(p[1] > 10 and p[0] <= 10 for p in per)
            out[f"{name}/K{K}"] = {k: got[0][k] for k in ("n_records", "n_inst", "n_items")}
            print(name, K, out[f"{name}/K{K}"], flush=True)
    for K in KS:
        out[f"replica/K{K}"] = _replica_rank(_case("few buckets", K)[0], K)
        print("replica", K, out[f"replica/K{K}"], flush=True)
    dst = os.environ.get("SCAN_RUNS_EXPECTED_OUT", EXPECTED)
    with open(dst, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    import sys
    if sys.argv[1:] == ["record"]:
        _record()
