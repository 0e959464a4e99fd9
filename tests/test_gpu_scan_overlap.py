"""The counting scan counts each piece's run keys on the second stream, under the scan of the next piece: two key slices
that the pieces take in turn, the per-bucket add of k_keys_count an atomic because the next scan's direct atomics land on
the same table.  Many pieces (both slices reused several times) must give what one piece gives and what the oracle gives
-- from host arrays under the upload of the bases, from host arrays after it, and from device-resident inputs; a bucket
whose keys overflow its class slice in every piece (those keys take the direct atomic, beside the count of the piece
before) must come out whole; and DFK_NO_OVERLAP=1 (one stream, one slice) must give the same digest."""
import numpy as np
import pytest

from tests import util

pytestmark = pytest.mark.gpu

PIECES = 10          # at least 8: each of the two slices is reused four times or more


def _run(rs, K, device_inputs=False, **kw):
    """One count of `rs`; what it computed, and the open Dfk (the caller closes it)."""
    from superplus_amd.dfk import Dfk
    d = Dfk(K=K, keep_pre_adjacency=True, **kw)
    if device_inputs:
        import torch
        dev = torch.device("cuda", 0)
        t = [torch.from_numpy(np.ascontiguousarray(rs[k]).view(v)).to(dev)
             for k, v in (("packed", np.uint8), ("base_off", np.int64), ("read_len", np.int32), ("pq_bytes", np.uint8),
                          ("pq_off", np.int64), ("bc", np.int32))]
        d.count_device(*t)
        torch.cuda.synchronize()
    else:
        d.count(rs["packed"], rs["base_off"], rs["read_len"], rs["pq_bytes"], rs["pq_off"], rs["bc"])
    out = dict(good=d.good_lens(), solid=d.solid(), spectrum=d.spectrum(), digest=d.digest(), st=d.stats())
    return out, d


def _same(a, b, what, keys=("n_records", "n_inst", "n_passes")):
    assert np.array_equal(a["good"], b["good"]), what
    util.assert_same_solid(a["solid"], b["solid"], what)
    assert np.array_equal(a["spectrum"], b["spectrum"]), what
    assert a["digest"] == b["digest"], what
    for k in keys:
        assert a["st"][k] == b["st"][k], (what, k, a["st"][k], b["st"][k])


def _sets(golden_dir):
    from tests.test_oracle_golden import load_hot
    return {"hot": (load_hot(golden_dir), 2), "synthetic": (util.make_set(91, 60000, 6000), 3)}


_WAYS = {"under the upload": dict(env={"DFK_SCAN_UNDER_UPLOAD_MIN": "0", "DFK_UPLOAD_SEGMENT": "8192"}, device_inputs=False),
         "host arrays": dict(env={}, device_inputs=False),
         "device inputs": dict(env={}, device_inputs=True)}


@pytest.mark.parametrize("K", [40, 48])
@pytest.mark.parametrize("which", ["hot", "synthetic"])
def test_many_pieces_on_two_slices(oracle, golden_dir, monkeypatch, K, which):
    """(a) At least PIECES pieces, from host arrays under the upload, from host arrays and from device-resident inputs: the
    one-piece run's result, and the oracle's."""
    rs, min_freq = _sets(golden_dir)[which]
    n = len(rs["read_len"])
    ref = oracle.run(rs["packed"], rs["base_off"], rs["read_len"], rs["pq_bytes"], rs["pq_off"], rs["bc"], K=K, min_freq=min_freq)
    whole, d = _run(rs, K, min_freq=min_freq)
    util.check_parity(ref, d)
    d.close()
    for way, how in _WAYS.items():
        with monkeypatch.context() as mp:
            for k, v in how["env"].items():
                mp.setenv(k, v)
            mp.setenv("DFK_SCAN_KEY_PIECE", str(max(1, n // PIECES)))
            got, d = _run(rs, K, device_inputs=how["device_inputs"], min_freq=min_freq)
            util.check_parity(ref, d)
            d.close()
        _same(got, whole, f"{which} K={K} {way}")


@pytest.mark.parametrize("K", [40, 48])
def test_halving_tail_of_the_last_range(oracle, monkeypatch, K):
    """(a') The pieces of the range that ends the reads halve down to DFK_SCAN_KEY_TAIL: pieces of at most 4096 reads with a
    tail of 256, so the last range ends in pieces of 2048, 1024, 512 and 256 reads -- from device inputs, from host arrays,
    and under the upload, where only the final range has the tail.  Each way gives the one-piece run's result and the
    oracle's; so does DFK_SCAN_KEY_TAIL=0 (equal pieces)."""
    rs, min_freq = util.make_set(91, 60000, 6000), 3
    ref = oracle.run(rs["packed"], rs["base_off"], rs["read_len"], rs["pq_bytes"], rs["pq_off"], rs["bc"], K=K, min_freq=min_freq)
    whole, d = _run(rs, K, min_freq=min_freq)
    util.check_parity(ref, d)
    d.close()
    for tail in ("256", "0"):
        for way, how in _WAYS.items():
            with monkeypatch.context() as mp:
                for k, v in how["env"].items():
                    mp.setenv(k, v)
                mp.setenv("DFK_SCAN_KEY_PIECE", "4096")
                mp.setenv("DFK_SCAN_KEY_TAIL", tail)
                got, d = _run(rs, K, device_inputs=how["device_inputs"], min_freq=min_freq)
                util.check_parity(ref, d)
                d.close()
            _same(got, whole, f"synthetic K={K} tail {tail} {way}")


def _poly_a_set(n_poly, seed=23):
    """The reads of test_one_bucket_beyond_its_class_slice: n_poly poly-A reads (two runs each, all of one fine bucket), then
    3000 random reads of which each occurs three times."""
    from superplus_amd import feudal
    rng = np.random.default_rng(seed)
    extra = rng.integers(0, 4, (3000, 100), dtype=np.uint8)
    extra[1000:2000] = extra[:1000]; extra[2000:] = extra[:1000]
    packed = np.concatenate([np.zeros(25 * n_poly, np.uint8), feudal.pack_bases(extra).reshape(-1)])
    N = n_poly + len(extra)
    blk = np.array([100, (35 << 3) & 0xFF, 35 >> 5, 0], np.uint8)
    return dict(packed=packed, base_off=(np.arange(N + 1, dtype=np.uint64) * 25), read_len=np.full(N, 100, np.uint32),
                pq_bytes=np.tile(blk, N), pq_off=(np.arange(N + 1, dtype=np.uint64) * 4),
                bc=(1 + np.arange(N) % 7).astype(np.int32), n_reads=N)


@pytest.mark.parametrize("K", [40, 48])
def test_direct_atomics_beside_the_count_of_the_piece_before(oracle, monkeypatch, K):
    """(b) 12 000 poly-A reads in pieces of 1000: a class slice holds 1024 keys or a few more (its floor), every poly-A piece
    makes 2000 keys of one bucket, so in every piece about half of them take the scan's direct atomic on that bucket -- while
    k_keys_count adds the piece before's half to it.  Parity with the oracle, and the one-piece run's totals."""
    rs = _poly_a_set(12_000)
    ref = oracle.run(rs["packed"], rs["base_off"], rs["read_len"], rs["pq_bytes"], rs["pq_off"], rs["bc"], K=K)
    whole, d = _run(rs, K)
    util.check_parity(ref, d)
    d.close()
    assert whole["st"]["n_records"] >= 2 * 12_000
    monkeypatch.setenv("DFK_SCAN_KEY_PIECE", "1000")
    for rep in range(3):
        got, d = _run(rs, K, device_inputs=bool(rep & 1))
        util.check_parity(ref, d)
        d.close()
        _same(got, whole, f"poly-A K={K} run {rep}")


@pytest.mark.parametrize("K", [40, 48])
def test_no_overlap_gives_the_same_digest(golden_dir, monkeypatch, K):
    """(c) The inputs of (a) and (b) in many pieces, with the second stream and with DFK_NO_OVERLAP=1."""
    sets = {k: v for k, v in _sets(golden_dir).items()}
    sets["poly-A"] = (_poly_a_set(12_000), 3)
    for which, (rs, min_freq) in sets.items():
        piece = "1000" if which == "poly-A" else str(max(1, len(rs["read_len"]) // PIECES))
        monkeypatch.setenv("DFK_SCAN_KEY_PIECE", piece)
        monkeypatch.delenv("DFK_NO_OVERLAP", raising=False)
        two, d = _run(rs, K, min_freq=min_freq)
        d.close()
        monkeypatch.setenv("DFK_NO_OVERLAP", "1")
        one, d = _run(rs, K, min_freq=min_freq)
        d.close()
        _same(one, two, f"{which} K={K} DFK_NO_OVERLAP", keys=("n_records", "n_inst"))   # (the switch also serialises the passes)
