"""The device's path verifier (k_path_verify, csrc/dfk_check_kernels.h) shown to COUNT: on paths and reads damaged one way at a time
(tests/verify_cases.py) its eight counters are the ones oracle/verify_oracle.py computes from the same damaged set -- recorded in
tests/test_verify_oracle.py's DAMAGED, which the CPU suite holds to the oracle -- and the paths digest is the one those paths give.

The damaged paths reach the kernel through dfk_paths_verify_arrays (the context's graph, k-mer index and tables; the paths given),
under reads_per_batch 0, 1, 7 and 1000; damaged READS also through dfk_paths_verify and dfk_paths_verify_device on the context's own
paths, and on a context pathed in batches of 333 reads (r0 > 0).  Then the refusals of the three entries.  Every counter but dict_bad
is asserted at a non-zero value here; `broken` for each of its causes: an id out of range first in a path (id_out_of_range), behind
a good edge (id_behind_a_good_edge), edges that do not meet (edge_to_inv), an offset behind the first edge (offset_at_n)."""
import ctypes as C

import numpy as np
import pytest

from oracle import verify_oracle
from tests import verify_cases
from tests.test_gpu_paths import KW
from tests.test_verify_oracle import DAMAGED, EXPECT

pytestmark = pytest.mark.gpu

PER = (0, 1, 7, 1000)
NAMES = [f for f, _, _ in verify_cases.FIXTURES]
ARRAYS = ("packed", "base_off", "read_len")


def build_context(f, fixture):
    from superplus_amd.dfk import Dfk
    rs = f["rs"]
    kw = dict(KW[fixture]); nobc = kw.pop("nobc", False)
    d = Dfk(K=f["K"], **kw)
    d.count(rs["packed"], rs["base_off"], rs["read_len"], rs["pq_bytes"], rs["pq_off"], None if nobc else rs["bc"])
    d.graph_build()
    d.paths_build(rs["packed"], rs["base_off"], rs["read_len"], rs["pq_bytes"], rs["pq_off"])
    return d


@pytest.fixture(scope="module")
def context(golden_dir):
    """context(fixture) -> (the fixture as verify_cases loads it, a context that counted, built and pathed it): one at a time, kept
    while the tests ask for the same fixture (they are ordered by fixture)"""
    held = {}

    def get(fixture):
        f = verify_cases.load(golden_dir, fixture)
        if fixture not in held:
            for d in held.values(): d.close()
            held.clear()
            held[fixture] = build_context(f, fixture)
        return f, held[fixture]
    yield get
    for d in held.values(): d.close()


def counters(v):
    from superplus_amd.dfk import VERIFY
    return [v[k] for k in VERIFY]


def arrays_of(f, reads):
    """the reads as the library takes them: the fixture's own arrays when they are the fixture's reads"""
    return tuple(f["rs"][k] for k in ARRAYS) if reads is f["reads"] else verify_cases.pack_reads(reads)


def only_unplaced(paths, per):
    return sum(1 for r0 in range(0, len(paths), per) if all(not p for _, p in paths[r0:r0 + per]))


@pytest.mark.parametrize("fixture", NAMES)
def test_undamaged_paths_through_all_three_entries(context, fixture):
    """dfk_paths_verify still gives EXPECT; dfk_paths_verify_arrays on the context's own paths gives the same counters and the
    context's own digest, however they are cut; dfk_paths_verify_device gives what the host entry gives."""
    import torch
    f, d = context(fixture)
    rs = f["rs"]
    assert counters(d.paths_verify(*(rs[k] for k in ARRAYS))) == EXPECT[fixture]
    ck = d.paths_digest()
    assert (ck["PATHS_SUM"], ck["PATHS_XOR"]) == verify_oracle.paths_digest(f["paths"])
    own = d.paths()
    assert len(own[0]) == len(f["paths"]) and [int(x) for x in own[2]] == [e for _, p in f["paths"] for e in p]
    held = d.stats()["hbm_held"]
    for per in PER:
        for given in (own, f["paths"]):
            v, dg = d.paths_verify_arrays(*(rs[k] for k in ARRAYS), given, per)
            assert counters(v) == EXPECT[fixture], per
            assert dg == (ck["PATHS_SUM"], ck["PATHS_XOR"]), per
        assert d.stats()["hbm_held"] == held
    # what the batches are: pairs straddle batches of 7 (odd), a batch of one read is often an unplaced read alone, and on the two
    # fixtures that have seven unplaced reads in a row at a multiple of 7 a batch of 7 holds no path either
    N = len(f["paths"])
    assert N % 2 == 0 and N > 1000 and only_unplaced(f["paths"], 1) >= 300
    assert only_unplaced(f["paths"], 7) >= {"graph_k48": 1, "graph_k60_nobc": 10}.get(fixture, 0)
    dev = [torch.from_numpy(np.array(rs["packed"], np.uint8)).cuda(), torch.from_numpy(np.array(rs["base_off"], np.uint64).view(np.int64)).cuda(),
           torch.from_numpy(np.array(rs["read_len"], np.uint32).view(np.int32)).cuda()]
    assert counters(d.paths_verify_device(*dev)) == EXPECT[fixture]
    # the context's own paths and results are as they were
    assert d.paths_digest() == ck and counters(d.paths_verify(*(rs[k] for k in ARRAYS))) == EXPECT[fixture]


@pytest.mark.parametrize("fixture,cls", verify_cases.CASES)
def test_device_counts_what_the_oracle_counts(context, golden_dir, fixture, cls):
    f, d = context(fixture)
    name, paths, reads, n = verify_cases.damaged(golden_dir, fixture, cls)
    n_want, want = DAMAGED[fixture, cls]
    assert n == n_want
    want_dg = verify_oracle.paths_digest(paths)
    arrays = arrays_of(f, reads)
    if cls == "unplaced":
        assert only_unplaced(paths, 7) == (len(paths) + 6) // 7
    held = d.stats()["hbm_held"]
    for per in PER:
        v, dg = d.paths_verify_arrays(*arrays, paths, per)
        print(fixture, name, "reads_per_batch", per, counters(v), "want", want)
        assert counters(v) == want, (name, per)
        assert dg == want_dg, (name, per)
    assert d.stats()["hbm_held"] == held
    # the context's own paths are untouched by all that
    ck = d.paths_digest()
    assert (ck["PATHS_SUM"], ck["PATHS_XOR"]) == verify_oracle.paths_digest(f["paths"])


@pytest.mark.parametrize("fixture", NAMES)
def test_damaged_reads_through_the_entries_the_pipeline_uses(context, golden_dir, fixture):
    """No array entry involved: dfk_paths_verify and dfk_paths_verify_device on the context's own paths, given other reads."""
    import torch
    f, d = context(fixture)
    for cls in ("other_reads", "short_read"):
        _, paths, reads, _ = verify_cases.damaged(golden_dir, fixture, cls)
        assert paths is f["paths"]
        packed, base_off, read_len = verify_cases.pack_reads(reads)
        assert counters(d.paths_verify(packed, base_off, read_len)) == DAMAGED[fixture, cls][1], cls
        dev = [torch.from_numpy(packed).cuda(), torch.from_numpy(base_off.view(np.int64)).cuda(), torch.from_numpy(read_len.view(np.int32)).cuda()]
        assert counters(d.paths_verify_device(*dev)) == DAMAGED[fixture, cls][1], cls
    assert counters(d.paths_verify(*(f["rs"][k] for k in ARRAYS))) == EXPECT[fixture]


@pytest.mark.parametrize("fixture", ["graph_k48", "graph_frag_k48"])
def test_paths_built_in_batches_of_333(golden_dir, monkeypatch, fixture):
    """r0 > 0 in the context's OWN batches (every other small test paths its reads in one): the reads are indexed with r0 + i."""
    f = verify_cases.load(golden_dir, fixture)
    monkeypatch.setenv("DFK_PATH_BATCH_READS", "333")
    d = build_context(f, fixture)
    try:
        assert counters(d.paths_verify(*(f["rs"][k] for k in ARRAYS))) == EXPECT[fixture]
        ck = d.paths_digest()
        assert (ck["PATHS_SUM"], ck["PATHS_XOR"]) == verify_oracle.paths_digest(f["paths"])
        for cls in ("other_reads", "short_read"):
            _, _, reads, _ = verify_cases.damaged(golden_dir, fixture, cls)
            assert counters(d.paths_verify(*verify_cases.pack_reads(reads))) == DAMAGED[fixture, cls][1], cls
    finally:
        d.close()


def test_a_hand_made_set_of_any_size(context, golden_dir):
    """n_reads is free: five reads of the fixture (an odd number), then one, against the oracle on just those"""
    f, d = context("graph_k48")
    placed = [i for i, (_, p) in enumerate(f["paths"]) if p]
    pick = placed[:3] + [next(i for i, (_, p) in enumerate(f["paths"]) if not p)] + placed[-1:]
    paths, reads = [f["paths"][i] for i in pick], [f["reads"][i] for i in pick]
    paths[1] = (paths[1][0], [len(f["edges"])]); reads[2] = reads[2][:f["K"] - 1]
    for n in (5, 1):
        want = verify_oracle.verify(f["edges"], f["to_left"], f["to_right"], paths[:n], reads[:n], f["K"])
        assert want[0] == min(n, 4) and (n == 1 or (want[1] == 1 and want[4] == 1))
        for per in (0, 1, 2):
            v, dg = d.paths_verify_arrays(*verify_cases.pack_reads(reads[:n]), paths[:n], per)
            assert counters(v) == want and dg == verify_oracle.paths_digest(paths[:n])


def raw_arrays(d, packed, base_off, read_len, n, offsets, first, edges, per, out=True):
    """dfk_paths_verify_arrays as C sees it (None = NULL; n as claimed) -> (return code, message, out)"""
    from superplus_amd.dfk import lib, _p
    res = (C.c_uint64 * 10)(*([7] * 10))
    rc = lib().dfk_paths_verify_arrays(d._ctx, _p(packed), _p(base_off), _p(read_len), C.c_uint64(n), _p(offsets), _p(first), _p(edges),
                                       C.c_uint64(per), res if out else None)
    return rc, lib().dfk_last_error().decode(), list(res)


def test_refusals_and_the_call_after_them(golden_dir):
    """(a context of its own: it ends with the k-mer index given back)"""
    fixture = "graph_k48"
    f = verify_cases.load(golden_dir, fixture)
    d = build_context(f, fixture)
    try:
        refusals(f, d, fixture)
    finally:
        d.close()


def refusals(f, d, fixture):
    import torch
    from superplus_amd.dfk import Dfk, DfkError
    rs = f["rs"]
    packed, base_off, read_len = (np.array(rs[k], t) for k, t in zip(ARRAYS, (np.uint8, np.uint64, np.uint32)))
    N = len(read_len)
    offsets, first, edges = (np.ascontiguousarray(a) for a in d.paths())
    held = d.stats()["hbm_held"]
    ck = d.paths_digest()

    def still_right():
        v, dg = d.paths_verify_arrays(packed, base_off, read_len, (offsets, first, edges), 7)
        assert counters(v) == EXPECT[fixture] and dg == (ck["PATHS_SUM"], ck["PATHS_XOR"])
        assert counters(d.paths_verify(packed, base_off, read_len)) == EXPECT[fixture]
        assert d.stats()["hbm_held"] == held and d.paths_digest() == ck

    def refused(code, word, *a, **k):
        rc, msg, out = raw_arrays(d, *a, **k)
        assert rc == code and word in msg, (rc, msg)
        assert out == [7] * 10                                                  # nothing written
        still_right()

    good = (packed, base_off, read_len, N, offsets, first, edges, 0)
    rc, _, out = raw_arrays(d, *good)
    assert rc == 0 and out[:8] == EXPECT[fixture]
    # null arguments
    for at in (0, 1, 2, 4, 5, 6):
        a = list(good); a[at] = None
        refused(-1, "null argument", *a)
    refused(-1, "null argument", *good, out=False)
    # first: not starting at 0, falling
    bad = first.copy(); bad[0] = 1
    refused(-1, "do not start at 0", packed, base_off, read_len, N, offsets, bad, edges, 0)
    i = int(np.flatnonzero(np.diff(first.astype(np.int64)) > 0)[3])             # the fourth placed read: first[i] >= 3
    bad = first.copy(); bad[i + 1] = first[i] - 1
    refused(-1, "fall at read", packed, base_off, read_len, N, offsets, bad, edges, 7)
    # sizes: 2^31 reads (claimed: refused before an array is read); 2^31 path edges; a batch of 2^32 bytes (one read of 2^30 edges:
    # 8 + 4 * 2^30 bytes) -- each refused from `first` alone, before `edges` is looked at
    refused(-1, "2^31 - 1 at most", packed, base_off, read_len, 1 << 31, offsets, first, edges, 0)
    one = (packed, base_off[:2].copy(), read_len[:1].copy(), 1, offsets[:1].copy())
    refused(-1, "2^31 - 1 at most", *one, np.array([0, 1 << 31], np.uint64), edges, 0)
    refused(-1, "32 bits", *one, np.array([0, 1 << 30], np.uint64), edges, 0)
    refused(-1, "32 bits", packed, base_off[:3].copy(), read_len[:2].copy(), 2, offsets[:2].copy(), np.array([0, 5, (1 << 30) + 5], np.uint64), edges, 1)
    # the reads' tables (k_check_tables): not monotone; the last read left too few bytes -- from all three entries
    nm = base_off.copy(); nm[7] = nm[9]
    short = base_off.copy(); short[-1] -= 9
    for bad in (nm, short):
        refused(-5, "offset table", packed, bad, read_len, N, offsets, first, edges, 7)
        with pytest.raises(DfkError) as e:
            d.paths_verify(packed, bad, read_len)
        assert e.value.code == -5
        dev = [torch.from_numpy(packed).cuda(), torch.from_numpy(bad.view(np.int64)).cuda(), torch.from_numpy(read_len.view(np.int32)).cuda()]
        with pytest.raises(DfkError) as e:
            d.paths_verify_device(*dev)
        assert e.value.code == -5
        still_right()
    # a read count other than the pathed one: the two entries that verify the context's own paths refuse it, the array entry is free
    with pytest.raises(DfkError) as e:
        d.paths_verify(packed, base_off[:N - 1], read_len[:N - 2])
    assert e.value.code == -1 and "pathed" in str(e.value)
    dev = [torch.from_numpy(packed).cuda(), torch.from_numpy(base_off[:N - 1].view(np.int64).copy()).cuda(), torch.from_numpy(read_len[:N - 2].view(np.int32).copy()).cuda()]
    with pytest.raises(DfkError) as e:
        d.paths_verify_device(*dev)
    assert e.value.code == -1 and "pathed" in str(e.value)
    still_right()
    # a context that has no paths
    bare = Dfk(K=48)
    rc, msg, _ = raw_arrays(bare, *good)
    assert rc == -6 and "no paths" in msg
    bare.close()
    # after the index was given back: all three entries, and the message says why
    d.paths_index_write(None)
    dev = [torch.from_numpy(packed).cuda(), torch.from_numpy(base_off.view(np.int64)).cuda(), torch.from_numpy(read_len.view(np.int32)).cuda()]
    for call in (lambda: d.paths_verify(packed, base_off, read_len), lambda: d.paths_verify_device(*dev),
                 lambda: d.paths_verify_arrays(packed, base_off, read_len, (offsets, first, edges))):
        with pytest.raises(DfkError) as e:
            call()
        assert e.value.code == -6 and "index was given back" in str(e.value)
    assert d.stats()["hbm_held"] <= held
    w = d.paths_digest()
    assert (w["PATHS_SUM"], w["PATHS_XOR"]) == (ck["PATHS_SUM"], ck["PATHS_XOR"])
