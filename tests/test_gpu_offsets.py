"""GetOffsets1 per pair on the GPU (dfk_offsets_build / _build_arrays / _write: the candidates a workgroup a pair by an LDS bitmap, flag,
scan and emit, the bits test a workgroup a candidate, the compaction of those that pass, the tail on the host) against
tests/offsets_oracle.py: starts, per-pair words, records with `bits` as its raw 8 bytes, states, the file a.close.offsets byte for byte,
the counters and the digest -- on every seeded case and on the four fixtures' consensus as tests/cons_oracle.py gives it, in batches of
1 and 37 pairs; the refusals; the chain dfk_count ... dfk_cons_build -> dfk_offsets_build; `DF ... CONS=True OFFSETS=True`.  Everything
is exact.

The rule is pinned by the two restatements only (tests/offsets_oracle.py, superplus_amd/csrc/dfk_offsets.h)."""
import os

import numpy as np
import pytest

from tests import offsets_cases, offsets_oracle
from tests.test_offsets_oracle import TABLE

pytestmark = pytest.mark.gpu

FILE = offsets_oracle.FILE
COUNTERS = (("pairs", "pairs"), ("candidates", "candidates"), ("passed", "passed"), ("invalidated", "invalidated"), ("deleted_small", "deleted_small"), ("survivors", "survivors"),
            ("pairs_0", "pairs0"), ("pairs_1", "pairs1"), ("pairs_2", "pairs2"), ("pairs_more", "pairs_more"), ("closable", "closable"), ("lookups", "lookups"))


def records_bytes(records):
    import struct
    return b"".join(struct.pack("<iiiidII", *r, 0) for r in records)


def check(st, got, file, want, what):
    assert [int(x) for x in got["starts"]] == want["starts"], f"{what}: starts"
    assert [tuple(int(x) for x in w) for w in got["words"]] == [w + (0,) for w in want["words"]], f"{what}: the per-pair words"
    assert [int(x) for x in got["records"]["offset"]] == [r[0] for r in want["records"]], f"{what}: the offsets that passed"
    assert [int(x) for x in got["records"]["state"]] == [r[5] for r in want["records"]], f"{what}: states"
    assert got["records"].tobytes() == records_bytes(want["records"]), f"{what}: the records (bits as its 8 bytes)"
    assert tuple(st[k] for k, _ in COUNTERS) == tuple(want[k] for _, k in COUNTERS), f"{what}: {[(k, st[k], want[w]) for k, w in COUNTERS]}"
    assert (st["sum"], st["xor"]) == want["digest"], f"{what}: the digest"
    if file is not None: assert file == want["file"], f"{what}: {FILE} differs ({len(file)} bytes, {len(want['file'])} expected)"


def written(d, tmp_path, sub):
    out = os.path.join(tmp_path, sub)
    os.makedirs(out, exist_ok=True)
    held = d.stats()["hbm_held"]
    d.offsets_write(out)
    assert d.stats()["hbm_held"] == held and os.listdir(out) == [FILE]
    return open(os.path.join(out, FILE), "rb").read()


def through_arrays(d, tmp_path, seqs, want, what, batches):
    starts, bases = offsets_oracle.starts_and_bases(seqs)
    n = want["pairs"]
    for per in batches:
        out = os.path.join(tmp_path, f"per{per}")
        os.makedirs(out)
        held = d.stats()["hbm_held"]
        st = d.offsets_build_arrays(starts, bases, per, out)
        assert d.stats()["hbm_held"] == held
        check(st, d.offsets_fetch(), open(os.path.join(out, FILE), "rb").read(), want, f"{what} pairs_per_batch={per}")
        assert st["batches"] == ((n + per - 1) // per if per else (1 if n else 0)) and os.listdir(out) == [FILE]
        assert d.offsets_stats() == st
    # no directory: the same result, no file; dfk_offsets_write then writes the same
    st = d.offsets_build_arrays(starts, bases)
    check(st, d.offsets_fetch(), written(d, tmp_path, "later"), want, what + " no directory")


@pytest.fixture(scope="module")
def ctx():
    from superplus_amd.dfk import Dfk
    d = Dfk(K=48)
    yield d
    d.close()


SEEDED = offsets_cases.seeded()


# ---- 1. the seeded cases
@pytest.mark.parametrize("name,seqs", [(n, s) for n, s, _ in SEEDED], ids=[n for n, _, _ in SEEDED])
def test_seeded_cases_match_the_oracle(ctx, tmp_path, name, seqs):
    through_arrays(ctx, tmp_path, seqs, offsets_cases.oracle(name, seqs), name, (1, 37))


# ---- 2. the fixtures' consensus, from the Python cons oracle
@pytest.mark.parametrize("case,K,which,row", TABLE, ids=[t[0] for t in TABLE])
def test_fixtures_consensus_matches_the_oracle(ctx, golden_dir, tmp_path, case, K, which, row):
    want = offsets_oracle.fixture_offsets(golden_dir, case, K, which)
    assert want["passed"] > 0
    through_arrays(ctx, tmp_path, want["seqs"], want, case, (1, 37))


# ---- 3. the refusals
def test_refusals_leave_the_earlier_result_served(tmp_path):
    import ctypes as C
    from superplus_amd.dfk import OFFSETS_RECORD, Dfk, DfkError, lib
    d = Dfk(K=48)
    for call in (lambda: d.offsets_build(), lambda: d.offsets_stats(), lambda: d.offsets_fetch(), lambda: d.offsets_write(str(tmp_path))):
        with pytest.raises(DfkError) as e:
            call()
        assert e.value.code == -6                                                # DFK_E_STATE: no consensus, no offsets
    name, seqs, _ = next(s for s in SEEDED if s[0] == "near-repeat")
    want = offsets_cases.oracle(name, seqs)
    starts, bases = offsets_oracle.starts_and_bases(seqs)
    st = d.offsets_build_arrays(starts, bases)
    check(st, d.offsets_fetch(), None, want, name)
    fell = starts.copy(); fell[1] = fell[2] + 1
    from1 = starts.copy(); from1[0] = 1
    high = bases.copy(); high[17] = 4
    long_starts = np.asarray([0, 401, 500], np.uint64)
    for code, call in ((-1, lambda: d.offsets_build_arrays(None, bases)), (-1, lambda: d.offsets_build_arrays(starts, None)), (-1, lambda: d.offsets_build_arrays(fell, bases)),
                       (-1, lambda: d.offsets_build_arrays(from1, bases)), (-1, lambda: d.offsets_build_arrays(starts, high)),
                       (-1, lambda: d.offsets_build_arrays(long_starts, np.zeros(500, np.uint8))), (-6, lambda: d.offsets_build())):
        held = d.stats()["hbm_held"]
        with pytest.raises(DfkError) as e:
            call()
        assert e.value.code == code, e.value
        assert d.stats()["hbm_held"] == held
        check(d.offsets_stats(), d.offsets_fetch(), None, want, "after a refused call")
    assert d.offsets_stats() == st
    # an element of exactly 400 bases is taken
    d.offsets_build_arrays(np.asarray([0, 400, 800], np.uint64), np.zeros(800, np.uint8))
    assert d.offsets_stats()["candidates"] == 785 and d.offsets_stats()["pairs"] == 1
    st = d.offsets_build_arrays(starts, bases)
    # a fetch buffer too small: the counts are still told; NULL with cap 0 gives the counts alone
    npairs, nr = C.c_uint64(), C.c_uint64()
    small = np.zeros(3, OFFSETS_RECORD)
    rc = lib().dfk_offsets_fetch(d._ctx, None, None, C.byref(npairs), small.ctypes.data_as(C.c_void_p), C.c_uint64(2), C.byref(nr))
    assert rc == -1 and (npairs.value, nr.value) == (1, 3)
    assert lib().dfk_offsets_fetch(d._ctx, None, None, C.byref(npairs), None, C.c_uint64(0), C.byref(nr)) == 0 and nr.value == 3
    # a directory that does not exist: an error, no file
    with pytest.raises(DfkError) as e:
        d.offsets_write(os.path.join(tmp_path, "no", "such"))
    assert e.value.code == -1 and not os.path.exists(os.path.join(tmp_path, "no")) and not os.listdir(tmp_path)
    d.close()


# ---- 4. the chain
def test_chain_from_count_to_offsets(golden_dir, tmp_path):
    from tests.test_gpu_cons import partnered
    case, K, which, _ = TABLE[2]                                                 # graph_pathy_k48: 63 pairs
    want = offsets_oracle.fixture_offsets(golden_dir, case, K, which)
    d, rs, i = partnered(golden_dir, tmp_path, case, K, which)
    from superplus_amd.dfk import DfkError
    with pytest.raises(DfkError) as e:
        d.offsets_build()                                                        # no consensus yet
    assert e.value.code == -6
    d.cons_build(rs["packed"], rs["base_off"], rs["read_len"], rs["pq_bytes"], rs["pq_off"])
    held = d.stats()["hbm_held"]
    st = d.offsets_build()
    assert d.stats()["hbm_held"] == held and st["batches"] == 1 and st["pairs"] == 63
    check(st, d.offsets_fetch(), written(d, tmp_path, "chain"), want, case + " through the chain")
    d.close()


# ---- 5. DF
def offsets_lines(out):
    return [l for l in out.splitlines() if l.startswith("DF_OFFSETS ")]


def test_df_writes_the_offsets_file_and_only_when_asked(tmp_path, golden_dir):
    from tests import cons_oracle
    from tests.test_gpu_hops import run_df
    case, K, which, _ = TABLE[0]                                                 # graph_frag_k48
    want = offsets_oracle.fixture_offsets(golden_dir, case, K, which)            # ONE_GOOD off, as the table was made
    args = ("HOPS=True", "ONE_GOOD=False", "CLOSER=True", "PARTNERS=True", "CONS=True")
    on = os.path.join(tmp_path, "on"); off = os.path.join(tmp_path, "off"); refused = os.path.join(tmp_path, "refused")
    for p in (on, off, refused): os.makedirs(p)
    r = run_df(on, golden_dir, which, *args, "OFFSETS=True")
    assert r.returncode == 0, r.stdout + r.stderr
    w = f"{on}/GapToy/1/a.48"
    assert open(f"{w}/{FILE}", "rb").read() == want["file"]
    assert open(f"{w}/a.close.cons", "rb").read() == cons_oracle.fixture_cons(golden_dir, case, K, which)["file"]
    assert offsets_lines(r.stdout) == ['DF_OFFSETS {"pairs": %d, "candidates": %d, "passed": %d, "invalidated": %d, "deleted_small": %d, "survivors": %d, "a.close.offsets": "%016x%016x", '
                                       '"pairs_0": %d, "pairs_1": %d, "pairs_2": %d, "pairs_more": %d, "closable": %d, "lookups": %d, "batches": 1}'
                                       % (want["pairs"], want["candidates"], want["passed"], want["invalidated"], want["deleted_small"], want["survivors"], *want["digest"], want["pairs0"],
                                          want["pairs1"], want["pairs2"], want["pairs_more"], want["closable"], want["lookups"])], offsets_lines(r.stdout)
    assert r.stdout.index("DF_CONS ") < r.stdout.index("DF_OFFSETS ")
    # without the switch: no such file, no such line, everything else the same
    r2 = run_df(off, golden_dir, which, *args)
    assert r2.returncode == 0, r2.stdout + r2.stderr
    w2 = f"{off}/GapToy/1/a.48"
    assert not os.path.exists(f"{w2}/{FILE}") and "DF_OFFSETS" not in r2.stdout and FILE not in r2.stdout
    assert sorted(os.listdir(w2)) == sorted(f for f in os.listdir(w) if f != FILE)
    assert all(open(f"{w2}/{f}", "rb").read() == open(f"{w}/{f}", "rb").read() for f in os.listdir(w2) if f.startswith("a.close"))
    assert [l for l in r2.stdout.splitlines() if l.startswith(("DF_CONS ", "DF_PARTNERS ", "DF_DIGESTS "))] == [l for l in r.stdout.splitlines() if l.startswith(("DF_CONS ", "DF_PARTNERS ", "DF_DIGESTS "))]
    # OFFSETS without CONS is refused at argument time
    r3 = run_df(refused, golden_dir, which, "HOPS=True", "CLOSER=True", "PARTNERS=True", "OFFSETS=True")
    assert r3.returncode != 0 and "OFFSETS=True needs CONS=True" in r3.stdout and not os.path.exists(f"{refused}/GapToy")
