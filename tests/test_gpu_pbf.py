"""SURVEY 8(f)-3 on the GPU: ParseBarcodedFastqs with the pair order, the 2-bit packing and the PQVec encoder on the device
(dfk_pbf_run, the program's default path) -- byte for byte against the fixture the reference's own binary wrote
(tests/golden/pbf/), against what that binary wrote from the same seeded inputs (tests/golden/pbf_ref.json), and against
the program's HOST=True path on seeded inputs: ragged lengths, duplicates (ties in the per-barcode order), reads with N,
READS_PER_BC, bucket counts from 1 to 256, and a set larger than MAX_MEM_GB done in groups of buckets.  And on the edge
profiles of tests/fastq_synth.py::make_fastq_edges: reads above 256 bases (the encoder's plan in HBM scratch and the second
length byte of the pair order), the longest read at exactly 256, and the encoder in many batches (DFK_PBF_BATCH_READS)."""
import gzip
import os
import subprocess

import pytest

from tests.fastq_synth import case_name, cut_fastq, edge_case_name, make_fastq
from tests.test_parse_barcoded_fastqs import EDGE_CASES, EDGE_IDS, OURS, edge_run, run, same_as_reference, same_files  # noqa: F401 (edge_run: a fixture)

pytestmark = pytest.mark.gpu


def test_device_path_matches_the_reference_fixture(tmp_path, golden_dir):
    g = os.path.join(golden_dir, "pbf")
    r = run(OURS, g + "/r_1.fq.gz", g + "/r_2.fq.gz", f"{tmp_path}/o/reads", "NUM_BUCKETS=4", "NUM_THREADS=3", device=True)
    assert r.returncode == 0, r.stderr
    assert "device: pair order" in r.stderr
    same_files(f"{tmp_path}/o/reads", g + "/reads")


@pytest.mark.parametrize("pairs,seed,n_bc,ragged,extra", [
    (2000, 11, 40, True, ("NUM_BUCKETS=5",)), (1500, 12, 300, False, ()), (800, 13, 3, True, ("NUM_BUCKETS=256",)),
    (1200, 14, 25, True, ("NUM_BUCKETS=2",)), (1500, 15, 30, False, ("NUM_BUCKETS=7", "READS_PER_BC=90")), (900, 16, 12, True, ("NUM_BUCKETS=1",))])
def test_device_path_matches_host_path_and_reference_binary(tmp_path, pairs, seed, n_bc, ragged, extra):
    fq1, fq2 = f"{tmp_path}/a_1.fq.gz", f"{tmp_path}/a_2.fq.gz"
    make_fastq(fq1, fq2, pairs, seed, n_bc=n_bc, ragged=ragged)
    d = run(OURS, fq1, fq2, f"{tmp_path}/dev/reads", "NUM_THREADS=4", *extra, device=True)
    assert d.returncode == 0, d.stderr
    h = run(OURS, fq1, fq2, f"{tmp_path}/host/reads", "NUM_THREADS=4", *extra)
    assert h.returncode == 0, h.stderr
    same_files(f"{tmp_path}/dev/reads", f"{tmp_path}/host/reads")
    if "NUM_BUCKETS=1" not in extra:                                          # (the reference aborts on one bucket)
        same_as_reference(f"{tmp_path}/dev/reads", fq1, fq2, case_name(pairs, seed, n_bc, ragged, extra))


def test_two_hundred_thousand_pairs_and_groups_of_buckets(tmp_path):
    """A seeded 200 k-pair set (ragged lengths, 3000 barcodes): the device path whole, the device path with a MAX_MEM_GB that
    forces several groups of buckets (each group a dfk_pbf_run of its own), and the host path -- three identical file sets."""
    fq1, fq2 = f"{tmp_path}/a_1.fq.gz", f"{tmp_path}/a_2.fq.gz"
    make_fastq(fq1, fq2, 200_000, 77, n_bc=3000, ragged=True)
    whole = run(OURS, fq1, fq2, f"{tmp_path}/whole/reads", "NUM_THREADS=8", "NUM_BUCKETS=16", device=True)
    assert whole.returncode == 0 and "more passes" not in whole.stderr, whole.stderr
    grouped = run(OURS, fq1, fq2, f"{tmp_path}/groups/reads", "NUM_THREADS=8", "NUM_BUCKETS=16", "MAX_MEM_GB=0.04", device=True)
    assert grouped.returncode == 0, grouped.stderr
    assert int(grouped.stderr.split("allowed: ")[1].split()[0]) >= 3, grouped.stderr
    host = run(OURS, fq1, fq2, f"{tmp_path}/host/reads", "NUM_THREADS=8", "NUM_BUCKETS=16")
    assert host.returncode == 0, host.stderr
    same_files(f"{tmp_path}/whole/reads", f"{tmp_path}/host/reads")
    same_files(f"{tmp_path}/groups/reads", f"{tmp_path}/host/reads")


def test_device_path_refuses_what_the_reference_refuses(tmp_path):
    """A quality above 63 (PQVecEncoder: "Your input reads are funny", feudal/PQVec.cc:30-35) and a character that is no base."""
    def write(p, recs):
        with gzip.open(p, "wt") as f:
            for name, s, q in recs: f.write(f"@{name}\n{s}\n+\n{q}\n")
    ok = [("r0#1_2_3/1", "ACGTACGTAC", "IIIIIIIIII"), ("r1#1_2_3/1", "ACGTTCGTAC", "IIIIIIIIII")]
    write(f"{tmp_path}/a_2.fq.gz", [(n.replace("/1", "/2"), s, q) for n, s, q in ok])
    write(f"{tmp_path}/q_1.fq.gz", [ok[0], ("r1#1_2_3/1", "ACGTTCGTAC", "IIII" + chr(33 + 64) + "IIIII")])
    r = run(OURS, f"{tmp_path}/q_1.fq.gz", f"{tmp_path}/a_2.fq.gz", f"{tmp_path}/o1/reads", device=True)
    assert r.returncode != 0 and "funny" in r.stderr and not os.path.exists(f"{tmp_path}/o1/reads.fastb")
    write(f"{tmp_path}/b_1.fq.gz", [ok[0], ("r1#1_2_3/1", "ACGTXCGTAC", "IIIIIIIIII")])
    r = run(OURS, f"{tmp_path}/b_1.fq.gz", f"{tmp_path}/a_2.fq.gz", f"{tmp_path}/o2/reads", device=True)
    assert r.returncode != 0 and "unexpected base" in r.stderr and not os.path.exists(f"{tmp_path}/o2/reads.fastb")


def run_traced(fq1, fq2, head, *extra, batch_reads=None):
    """The device path under DFK_TRACE=1 -> (the finished run, its "pbf: encoder batch" lines: one per batch of the encoder)."""
    env = dict(os.environ, DFK_TRACE="1")
    env.pop("DFK_PBF_BATCH_READS", None)
    if batch_reads: env["DFK_PBF_BATCH_READS"] = str(batch_reads)
    r = subprocess.run([OURS, "FASTQS={" + fq1 + "," + fq2 + "}", "OUT_HEAD=" + head, "NUM_THREADS=4", *extra], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    return r, [l for l in r.stderr.splitlines() if "pbf: encoder batch of" in l]


@pytest.mark.parametrize("case", EDGE_CASES, ids=EDGE_IDS)
def test_edges_device_path_matches_host_path_and_reference_binary(tmp_path, edge_run, case):
    """Unbatched, one group: one plan launch -- k_pbf_pq_plan where a read is above 256 bases, k_pbf_pq_plan_lds with the
    longest read at exactly 256."""
    fq1, fq2, host, pairs, _ = edge_run(case)
    longest = max(len(s) for p in pairs for s in p[1:3])
    assert longest == 256 if case[0] == "lds_edge" else longest > 256
    _, batches = run_traced(fq1, fq2, f"{tmp_path}/dev/reads", *case[2])
    assert len(batches) == 1 and batches[0].endswith("plan in LDS" if case[0] == "lds_edge" else "plan in HBM"), batches
    same_files(f"{tmp_path}/dev/reads", host)
    same_as_reference(f"{tmp_path}/dev/reads", fq1, fq2, edge_case_name(*case))


@pytest.mark.parametrize("batch_reads", [7, 64, 65])
@pytest.mark.parametrize("case", EDGE_CASES[:2], ids=EDGE_IDS[:2])
def test_edges_encoder_in_batches(tmp_path, edge_run, case, batch_reads):
    """DFK_PBF_BATCH_READS: batches that end inside a pair (7, 65) and on a wave of the LDS plan (64), the last one short."""
    fq1, fq2, host, pairs, _ = edge_run(case)
    _, batches = run_traced(fq1, fq2, f"{tmp_path}/dev/reads", *case[2], batch_reads=batch_reads)
    assert len(batches) == -(-2 * len(pairs) // batch_reads) > 1, batches
    same_files(f"{tmp_path}/dev/reads", host)
    same_as_reference(f"{tmp_path}/dev/reads", fq1, fq2, edge_case_name(*case))


@pytest.mark.parametrize("case", EDGE_CASES[:3], ids=EDGE_IDS[:3])
def test_edges_one_read_a_batch(tmp_path, edge_run, case):
    """The first 100 pairs, DFK_PBF_BATCH_READS=1: every read a batch of its own (one live lane in a wave of the LDS plan)."""
    fq1, fq2 = f"{tmp_path}/c_1.fq.gz", f"{tmp_path}/c_2.fq.gz"
    cut_fastq(*edge_run(case)[:2], fq1, fq2, 100)
    h = run(OURS, fq1, fq2, f"{tmp_path}/host/reads", "NUM_THREADS=4", *case[2])
    assert h.returncode == 0, h.stderr
    _, batches = run_traced(fq1, fq2, f"{tmp_path}/dev/reads", *case[2], batch_reads=1)
    assert len(batches) == 200, len(batches)
    same_files(f"{tmp_path}/dev/reads", f"{tmp_path}/host/reads")


def test_edges_groups_of_buckets_take_both_plan_kernels(tmp_path, edge_run):
    """`long` under a MAX_MEM_GB that holds a part of it: the unbarcoded pairs (256 bases at most) are a group planned in LDS,
    the buckets (reads up to 1000) groups planned in HBM scratch -- the same three files."""
    case = EDGE_CASES[1]
    fq1, fq2, host, _, _ = edge_run(case)
    r, batches = run_traced(fq1, fq2, f"{tmp_path}/dev/reads", *case[2], f"MAX_MEM_GB={0.9 / 1024}")
    assert int(r.stderr.split("allowed: ")[1].split()[0]) >= 3, r.stderr
    assert {b.rsplit(" ", 1)[1] for b in batches} == {"LDS", "HBM"}, batches
    same_files(f"{tmp_path}/dev/reads", host)
    same_as_reference(f"{tmp_path}/dev/reads", fq1, fq2, edge_case_name(*case))
