"""The counting scan reads each read's bases a block of W positions at a time (the words of the next block loaded while
this one computes) and closes runs with two LDS stores, building the summaries after the read.  These reads hit its edges:
every byte phase of a word at the start, lengths around K and around the block boundaries, long reads, reads with 10, 11
and 12 runs (a summary holds ten), and a last read that ends in the last byte of the packed bases -- at K=40, 48 and 60,
in one launch, in pieces of 64 reads and under the upload of the bases.  Parity with the oracle, and the record count
against a restatement of the scan's runs in numpy."""
import numpy as np
import pytest

from tests import util

pytestmark = pytest.mark.gpu

M = 16
MMER_SALT = 0x2C6B39D1
Q = 35


def _mix32(x):
    x = x ^ (x >> np.uint64(15))
    x = (x * np.uint64(0x2C1B3C6D)) & np.uint64(0xFFFFFFFF)
    return x ^ (x >> np.uint64(12))


def _runs(codes, K, log2_nb):
    """Runs (records) of one read as the scan makes them: a run ends where the bucket of the k-mer's minimizer changes or
    it reaches NK_MAX k-mers.  Buckets are compared before the owner permutation (one rank: none)."""
    L = len(codes)
    if L < K + 1:
        return 0
    c = codes.astype(np.uint64)
    n_m = L - M + 1
    f = np.zeros(n_m, np.uint64); rc = np.zeros(n_m, np.uint64)
    for j in range(M):
        f |= c[j:j + n_m] << np.uint64(2 * (M - 1 - j))
        rc |= (np.uint64(3) - c[j:j + n_m]) << np.uint64(2 * j)
    h = _mix32(np.minimum(f, rc) ^ np.uint64(MMER_SALT))
    W = K - M + 1
    mins = np.lib.stride_tricks.sliding_window_view(h, W).min(axis=1)
    b = ((mins * np.uint64(0x9E3779B1)) & np.uint64(0xFFFFFFFF)) >> np.uint64(32 - log2_nb)
    nk_max = 95 - K
    runs, nk = 0, 0
    for s in range(len(b)):
        if s == 0 or b[s] != b[s - 1] or nk == nk_max:
            runs += 1; nk = 0
        nk += 1
    return runs


def _log2_nb(n_inst):
    v, l = n_inst // 850 + 1, 0
    while (1 << l) < v:
        l += 1
    return min(max(l, 4), 28)


def _read_set(K, seed=11):
    """Reads of the lengths and byte phases above, drawn from a 40 kb random genome (0.5 % substitutions, both strands),
    packed back to back with no padding after the last one."""
    from superplus_amd import feudal
    rng = np.random.default_rng(seed + K)
    genome = rng.integers(0, 4, 40_000, dtype=np.uint8)
    W = K - M + 1

    def draw(L):
        a = int(rng.integers(0, len(genome) - L))
        r = genome[a:a + L].copy()
        if rng.random() < 0.5:
            r = (3 - r[::-1]).astype(np.uint8)
        hit = rng.random(L) < 0.005
        r[hit] = (r[hit] + rng.integers(1, 4, int(hit.sum()))) & 3
        return r

    special = [K, K + 1, K + 2, 255, 256, 1000, 1203]
    for n in range(1, 5):
        special += [W * n - 1, W * n, W * n + 1, M - 1 + W * n - 1, M - 1 + W * n, M - 1 + W * n + 1]
    special = sorted(set(L for L in special if L >= K))
    bulk = [draw(int(L)) for L in rng.integers(100, 301, 2400)]
    reads = []
    byte_at = 0

    def put(r):
        nonlocal byte_at
        reads.append(r); byte_at += (len(r) + 3) // 4

    bi = iter(bulk)
    for L in special:
        for phase in range(4):                                   # a read of length L starting at every byte of a word
            pad = next(bi)
            while (byte_at + (len(pad) + 3) // 4) % 4 != phase:
                pad = np.concatenate([pad, draw(4)])             # one byte more
            put(pad); put(draw(L))
    for r in bi:
        put(r)
    # long reads with exactly 10, 11 and 12 runs at the bucket count the whole set gets
    n_long = 18
    n_inst = sum(max(0, len(r) - K + 1) for r in reads if len(r) >= K + 1) + n_long * (310 - K + 1) + 1000
    lb = _log2_nb(n_inst)
    many = {10: [], 11: [], 12: []}
    while sum(len(v) for v in many.values()) < n_long:
        r = draw(int(rng.integers(200, 420)))
        nr = _runs(r, K, lb)
        if nr in many and len(many[nr]) < n_long // 3:
            many[nr].append(r)
    for v in many.values():
        for r in v:
            put(r)
    put(draw(1000 + 4 * int(rng.integers(0, 4)) + 2))            # the last read ends mid-byte in the last byte of packed
    assert _log2_nb(sum(max(0, len(r) - K + 1) for r in reads if len(r) >= K + 1)) == lb
    n = len(reads)
    lens = np.array([len(r) for r in reads], np.uint32)
    nbytes = (lens.astype(np.uint64) + 3) // 4
    base_off = np.concatenate([[0], np.cumsum(nbytes)]).astype(np.uint64)
    packed = np.concatenate([feudal.pack_bases(r[None, :]).reshape(-1) for r in reads])
    assert len(packed) == int(base_off[-1])
    pqs = [np.frombuffer(feudal.pq_encode(np.full(len(r), Q, np.uint8)), np.uint8) for r in reads]
    pq_off = np.concatenate([[0], np.cumsum([len(x) for x in pqs])]).astype(np.uint64)
    bc = (1 + np.arange(n) // 2 % 9).astype(np.int32)
    rs = dict(packed=packed, base_off=base_off, read_len=lens, pq_bytes=np.concatenate(pqs), pq_off=pq_off, bc=bc, n_reads=n)
    return rs, reads


_MODES = {"one launch": {}, "pieces of 64": {"DFK_SCAN_KEY_PIECE": "64"},
          "under the upload": {"DFK_SCAN_UNDER_UPLOAD_MIN": "0", "DFK_UPLOAD_SEGMENT": "4096"}}


@pytest.mark.parametrize("K", [40, 48, 60])
def test_scan_edges_match_oracle(oracle, monkeypatch, K):
    rs, reads = _read_set(K)
    stats = {}
    for mode, env in _MODES.items():
        with monkeypatch.context() as mp:
            for k, v in env.items():
                mp.setenv(k, v)
            ref, d = util.run_both(oracle, rs, K=K, min_freq=2)
            st = util.check_parity(ref, d)
            good = d.good_lens()
            d.close()
        assert np.array_equal(good, rs["read_len"]), f"{mode}: constant Q{Q} trims nothing"
        stats[mode] = st
    st = stats["one launch"]
    log2_nb = _log2_nb(st["n_inst"])
    assert st["n_buckets"] == 1 << log2_nb
    per_read = [_runs(r, K, log2_nb) for r in reads]
    assert {10, 11, 12} <= set(per_read) and sum(1 for x in per_read if x > 10) >= 12, "reads around a summary's ten runs"
    assert st["n_records"] == sum(per_read)
    for mode, s in stats.items():
        for k in ("n_records", "n_inst", "n_passes"):
            assert s[k] == st[k], (mode, k, s[k], st[k])
