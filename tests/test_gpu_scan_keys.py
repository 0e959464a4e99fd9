"""The counting scan's run keys: per-bucket totals built from keys counted in LDS (k_keys_*), a piece of reads at a time,
must give the dictionary the oracle gives -- over one piece or many, under the upload of the bases or after it, and with
one bucket holding far more records than a class slice has room for (those keys are counted by the global atomic)."""
import os

import numpy as np
import pytest

from tests import util

pytestmark = pytest.mark.gpu


def _hot_case(golden_dir, K):
    from superplus_amd.dfk import Dfk
    from tests.test_oracle_golden import load_hot
    rs = load_hot(golden_dir)
    d = Dfk(K=K, min_freq=2, keep_pre_adjacency=True)
    d.count(rs["packed"], rs["base_off"], rs["read_len"], rs["pq_bytes"], rs["pq_off"], rs["bc"])
    out = dict(good=d.good_lens(), solid=d.solid(), spectrum=d.spectrum(), digest=d.digest(), st=d.stats())
    d.close()
    return out


@pytest.mark.parametrize("K", [40, 48, 60])
@pytest.mark.parametrize("under_upload", [False, True])
def test_hot_fixture_counted_in_many_pieces(golden_dir, monkeypatch, K, under_upload):
    """The hot-minimizer fixture at K=40/48/60: counted in pieces of 64 reads, the same result as in one piece (and, at K=48,
    as the reference's classes: tests/golden/expect_hot_k48_minfreq2.npz)."""
    if under_upload:
        monkeypatch.setenv("DFK_SCAN_UNDER_UPLOAD_MIN", "0")
        monkeypatch.setenv("DFK_UPLOAD_SEGMENT", "4096")
    whole = _hot_case(golden_dir, K)
    monkeypatch.setenv("DFK_SCAN_KEY_PIECE", "64")
    pieces = _hot_case(golden_dir, K)
    assert np.array_equal(pieces["good"], whole["good"])
    util.assert_same_solid(pieces["solid"], whole["solid"], f"K={K} pieces")
    assert np.array_equal(pieces["spectrum"], whole["spectrum"])
    assert pieces["digest"] == whole["digest"]
    for k in ("n_records", "n_inst", "n_passes"):
        assert pieces["st"][k] == whole["st"][k], k
    if K == 48:
        exp = np.load(os.path.join(golden_dir, "expect_hot_k48_minfreq2.npz"))
        util.assert_same_solid(pieces["solid"], exp["solid_post"], "hot: Dict view")
        assert np.array_equal(pieces["spectrum"], exp["spectrum"])


@pytest.mark.parametrize("piece", [None, "1000"])
def test_one_bucket_beyond_its_class_slice(oracle, monkeypatch, piece):
    """200 k poly-A reads: 200 k records of one fine bucket (> 2^16), far more than its class slice holds; the keys that do
    not fit are counted by the global atomic.  Parity with the oracle, in one piece and in pieces of 1000 reads."""
    if piece:
        monkeypatch.setenv("DFK_SCAN_KEY_PIECE", piece)
    n = 200_000
    rng = np.random.default_rng(23)
    extra = rng.integers(0, 4, (3000, 100), dtype=np.uint8)
    extra[1000:2000] = extra[:1000]; extra[2000:] = extra[:1000]
    from superplus_amd import feudal
    packed = np.concatenate([np.zeros(25 * n, np.uint8), feudal.pack_bases(extra).reshape(-1)])
    N = n + len(extra)
    blk = np.array([100, (35 << 3) & 0xFF, 35 >> 5, 0], np.uint8)
    rs = dict(packed=packed, base_off=(np.arange(N + 1, dtype=np.uint64) * 25), read_len=np.full(N, 100, np.uint32),
              pq_bytes=np.tile(blk, N), pq_off=(np.arange(N + 1, dtype=np.uint64) * 4),
              bc=(1 + np.arange(N) % 7).astype(np.int32), n_reads=N)
    ref, d = util.run_both(oracle, rs, K=48)
    st = util.check_parity(ref, d)
    assert st["n_records"] > (1 << 16)
