"""ParseBarcodedFastqs: stLFR fastq.gz pairs -> barcode-sorted .fastb/.qualp/.bci, byte for byte against
the reference's own binary -- oracle/_ref/ParseBarcodedFastqs, built from 10X/ParseBarcodedFastqs.cc where it lies
(flags only): against the fixture it wrote (tests/golden/pbf/) and, on seeded inputs, against the SHA-256 of the files it
wrote from them (tests/golden/pbf_ref.json; both made by tests/golden/make_golden.py).
These run the program's HOST=True path (its own host code for the pair order, the packing and the PQVec encoder), on the
CPU; the default path -- the same three steps on the MI355X (dfk_pbf_run) -- is compared with both in tests/test_gpu_pbf.py."""
import hashlib
import json
import os
import subprocess

import numpy as np
import pytest

from superplus_amd import feudal
from tests.fastq_synth import case_name, edge_case_name, fastq_digest, make_fastq, make_fastq_edges, read_fastq_pairs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OURS = os.path.join(ROOT, "superplus_amd", "ParseBarcodedFastqs")
REF_WRITTEN = os.path.join(ROOT, "tests", "golden", "pbf_ref.json")


def run(binary, fq1, fq2, head, *extra, device=False):
    host = ["HOST=True"] if binary == OURS and not device else []
    return subprocess.run([binary, "FASTQS={" + fq1 + "," + fq2 + "}", "OUT_HEAD=" + head, *extra, *host], capture_output=True, text=True, timeout=600)


def same_files(a, b):
    for ext in ("fastb", "qualp", "bci"):
        assert open(f"{a}.{ext}", "rb").read() == open(f"{b}.{ext}", "rb").read(), ext


def same_as_reference(head, fq1, fq2, key):
    """head.{fastb,qualp,bci} against what the reference's binary wrote from the same input with the same arguments
    (single-threaded): the SHA-256 of each file in tests/golden/pbf_ref.json."""
    exp = json.load(open(REF_WRITTEN))[key]
    assert fastq_digest(fq1, fq2) == exp["input"], "make_fastq no longer makes the input the reference's files were written from"
    for ext in ("fastb", "qualp", "bci"):
        assert hashlib.sha256(open(f"{head}.{ext}", "rb").read()).hexdigest() == exp[ext], ext


def test_fixture_written_by_the_reference_binary(tmp_path, golden_dir):
    g = os.path.join(golden_dir, "pbf")
    r = run(OURS, g + "/r_1.fq.gz", g + "/r_2.fq.gz", f"{tmp_path}/o/reads", "NUM_BUCKETS=4", "NUM_THREADS=3")
    assert r.returncode == 0, r.stderr
    same_files(f"{tmp_path}/o/reads", g + "/reads")
    # and what it wrote is a valid DF input: pairs, barcode 0 first, index ascending and complete
    _, _, rlen = feudal.read_fastb(f"{tmp_path}/o/reads.fastb")
    bci = feudal.read_bci(f"{tmp_path}/o/reads.bci")
    assert bci[0] == 0 and bci[-1] == len(rlen) == 600 and np.all(np.diff(bci) >= 0) and np.all(bci % 2 == 0)


@pytest.mark.parametrize("pairs,seed,n_bc,ragged,extra", [
    (2000, 11, 40, True, ("NUM_BUCKETS=5",)), (1500, 12, 300, False, ()), (800, 13, 3, True, ("NUM_BUCKETS=256",)),
    (1200, 14, 25, True, ("NUM_BUCKETS=2",)), (1500, 15, 30, False, ("NUM_BUCKETS=7", "READS_PER_BC=90"))])
def test_against_the_reference_binary(tmp_path, pairs, seed, n_bc, ragged, extra):
    fq1, fq2 = f"{tmp_path}/a_1.fq.gz", f"{tmp_path}/a_2.fq.gz"
    make_fastq(fq1, fq2, pairs, seed, n_bc=n_bc, ragged=ragged)
    o = run(OURS, fq1, fq2, f"{tmp_path}/ours/reads", "NUM_THREADS=4", *extra)
    assert o.returncode == 0, o.stderr
    same_as_reference(f"{tmp_path}/ours/reads", fq1, fq2, case_name(pairs, seed, n_bc, ragged, extra))


def test_one_bucket_works(tmp_path):
    """NUM_BUCKETS=1 makes the reference abort (its bucket loop never closes the only bucket: vec::back() on an empty
    vec, 10X/ParseBarcodedFastqs.cc:331-335); here it is simply one bucket: all barcodes ascending."""
    fq1, fq2 = f"{tmp_path}/a_1.fq.gz", f"{tmp_path}/a_2.fq.gz"
    make_fastq(fq1, fq2, 300, 31, n_bc=9)
    assert run(OURS, fq1, fq2, f"{tmp_path}/o/reads", "NUM_BUCKETS=1").returncode == 0
    bci = feudal.read_bci(f"{tmp_path}/o/reads.bci")
    assert bci[-1] == 600 and len(bci) >= 3


def test_refuses_what_the_reference_refuses(tmp_path):
    fq1, fq2 = f"{tmp_path}/a_1.fq.gz", f"{tmp_path}/a_2.fq.gz"
    make_fastq(fq1, fq2, 50, 3)
    make_fastq(f"{tmp_path}/b_1.fq.gz", f"{tmp_path}/b_2.fq.gz", 40, 4)
    assert run(OURS, fq1, f"{tmp_path}/b_2.fq.gz", f"{tmp_path}/o/reads").returncode != 0       # files that are not a pair
    open(f"{tmp_path}/plain.fq", "w").write("@r#0_0_0/1\nACGT\n+\nIIII\n")
    r = run(OURS, f"{tmp_path}/plain.fq", fq2, f"{tmp_path}/o/reads")
    assert r.returncode != 0 and "gz format" in r.stderr
    assert run(OURS, fq1, fq2, f"{tmp_path}/o/").returncode != 0                                  # OUT_HEAD ending in '/'


def test_output_feeds_the_df_front_end(tmp_path):
    """runall.sh:125-127: ParseBarcodedFastqs then DF, the ingest half (no GPU needed for EXIT_LOAD)."""
    fq1, fq2 = f"{tmp_path}/a_1.fq.gz", f"{tmp_path}/a_2.fq.gz"
    make_fastq(fq1, fq2, 700, 21, n_bc=30)
    assert run(OURS, fq1, fq2, f"{tmp_path}/tmp/reads", "NUM_BUCKETS=6").returncode == 0
    df = subprocess.run([os.path.join(ROOT, "superplus_amd", "DF"), f"ROOT={tmp_path}/tmp", f"LR={tmp_path}/tmp/reads.fastb", "PIPELINE=cs",
                         "ALIGN=False", "NUM_THREADS=4", "MAX_MEM_GB=640", "EXIT_LOAD=True"], capture_output=True, text=True)
    assert df.returncode == 0, df.stdout + df.stderr
    same_files(f"{tmp_path}/tmp/GapToy/1/data/frag_reads_orig", f"{tmp_path}/tmp/reads")


@pytest.mark.parametrize("mem_mb,extra", [(1.3, ("NUM_BUCKETS=8",)), (0.7, ("NUM_BUCKETS=16",)), (1.0, ("NUM_BUCKETS=9", "READS_PER_BC=400")),
                                          (0.3, ("NUM_BUCKETS=64",))])            # (the last: the unbarcoded pairs alone take several pieces)
def test_a_set_larger_than_max_mem_gb_is_done_in_groups_of_buckets(tmp_path, mem_mb, extra):
    """The reads do not fit MAX_MEM_GB: the first pass keeps barcodes and lengths, the inputs are read again once per group of
    consecutive buckets that fits (the unbarcoded pairs, which keep the file's order, in as many pieces as it takes) -- and the
    three files come out as when everything is held at once (and as the reference's binary writes them)."""
    fq1, fq2 = f"{tmp_path}/a_1.fq.gz", f"{tmp_path}/a_2.fq.gz"
    make_fastq(fq1, fq2, 3000, 41, n_bc=40, ragged=True)
    whole = run(OURS, fq1, fq2, f"{tmp_path}/whole/reads", "NUM_THREADS=3", *extra)
    assert whole.returncode == 0 and "more passes" not in whole.stderr, whole.stderr
    o = run(OURS, fq1, fq2, f"{tmp_path}/groups/reads", "NUM_THREADS=3", f"MAX_MEM_GB={mem_mb / 1024}", *extra)
    assert o.returncode == 0, o.stderr
    n_passes = int(o.stderr.split("allowed: ")[1].split()[0])
    assert n_passes >= 3, o.stderr
    same_files(f"{tmp_path}/groups/reads", f"{tmp_path}/whole/reads")
    same_as_reference(f"{tmp_path}/groups/reads", fq1, fq2, case_name(3000, 41, 40, True, extra))


def test_refuses_an_input_that_does_not_fit_max_mem_gb(tmp_path):
    """A SINGLE bucket whose reads do not fit MAX_MEM_GB ends the run with a message saying so (and no half-written files),
    not with the OOM killer."""
    from tests.fastq_synth import make_fastq
    make_fastq(f"{tmp_path}/a_1.fq.gz", f"{tmp_path}/a_2.fq.gz", 3000, 5, n_bc=6)
    r = subprocess.run([OURS, "FASTQS={" + f"{tmp_path}/a_1.fq.gz,{tmp_path}/a_2.fq.gz" + "}", f"OUT_HEAD={tmp_path}/o", "NUM_BUCKETS=2", "MAX_MEM_GB=0.0005", "HOST=True"],
                       capture_output=True, text=True)
    assert r.returncode != 0 and "MAX_MEM_GB" in r.stderr and not os.path.exists(f"{tmp_path}/o.fastb")


def test_without_a_device_the_default_path_fails_loudly(tmp_path):
    """The product path is the device's: where there is no GPU the program says so and writes nothing (HOST=True is explicit)."""
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    fq1, fq2 = f"{tmp_path}/a_1.fq.gz", f"{tmp_path}/a_2.fq.gz"
    make_fastq(fq1, fq2, 50, 3)
    r = run(OURS, fq1, fq2, f"{tmp_path}/o/reads", device=True)
    assert r.returncode != 0 and "HOST=True" in r.stderr and not os.path.exists(f"{tmp_path}/o/reads.fastb")


# ---- the edges make_fastq never reaches (tests/fastq_synth.py::make_fastq_edges): reads up to 1000 bases, reads of 1 to 5,
#      pairs that only a length orders, every PQVec width, Q0 and Q63, blocks cut at 255 values.  (profile, seed, arguments),
#      as in tests/golden/make_golden.py::PBF_EDGE_CASES
EDGE_CASES = [("lds_edge", 61, ("NUM_BUCKETS=3",)), ("long", 62, ("NUM_BUCKETS=3",)), ("long_one_file", 63, ("NUM_BUCKETS=3",)),
              ("long", 62, ("NUM_BUCKETS=3", "READS_PER_BC=170"))]
EDGE_IDS = ["-".join((p, str(s)) + e[1:]) for p, s, e in EDGE_CASES]


def decode_output(head):
    """head.{fastb,qualp,bci} -> one list per entry of the barcode index (the first: the unbarcoded pairs) of
    (read 1, read 2, qualities 1, qualities 2) in the files' order, reads as text over ACGT."""
    packed, off, rlen = feudal.read_fastb(head + ".fastb")
    pq, pq_off = feudal.read_qualp(head + ".qualp")
    bci = feudal.read_bci(head + ".bci")
    assert len(pq_off) == len(off) and bci[0] == 0 and bci[-1] == len(rlen) and np.all(bci % 2 == 0) and np.all(np.diff(bci) >= 0)
    reads, quals, blocks = [], [], []
    for k in range(len(rlen)):
        assert int(off[k + 1] - off[k]) == (int(rlen[k]) + 3) // 4
        codes = (packed[int(off[k]):int(off[k + 1])][:, None] >> np.array([0, 2, 4, 6])) & 3
        reads.append("".join("ACGT"[c] for c in codes.reshape(-1)[:int(rlen[k])]))
        assert not np.any(codes.reshape(-1)[int(rlen[k]):]), "bits behind the last base"
        b = feudal.pq_blocks(pq[int(pq_off[k]):int(pq_off[k + 1])])
        blocks += b
        quals.append([v for x in b for v in x[3]])
    groups = [[(reads[k], reads[k + 1], quals[k], quals[k + 1]) for k in range(int(bci[g]), int(bci[g + 1]), 2)] for g in range(len(bci) - 1)]
    return groups, blocks


def only_a_length_orders(x, y):
    """One of the two sequences is the other plus a tail of A."""
    s, l = sorted((x, y), key=len)
    return len(s) < len(l) and l.startswith(s) and set(l[len(s):]) == {"A"}


@pytest.fixture(scope="module")
def edge_run(tmp_path_factory):
    """case -> (fq1, fq2, head of the HOST=True run's files, the input's pairs, the output decoded): made once per case."""
    done = {}

    def get(case):
        if case not in done:
            profile, seed, extra = case
            d = tmp_path_factory.mktemp("edges")
            fq1, fq2 = f"{d}/a_1.fq.gz", f"{d}/a_2.fq.gz"
            make_fastq_edges(fq1, fq2, seed, profile)
            o = run(OURS, fq1, fq2, f"{d}/host/reads", "NUM_THREADS=4", *extra)
            assert o.returncode == 0, o.stderr
            done[case] = (fq1, fq2, f"{d}/host/reads", read_fastq_pairs(fq1, fq2), decode_output(f"{d}/host/reads"))
        return done[case]
    return get


@pytest.mark.parametrize("case", EDGE_CASES, ids=EDGE_IDS)
def test_edges_against_the_reference_binary(edge_run, case):
    fq1, fq2, head, _, _ = edge_run(case)
    same_as_reference(head, fq1, fq2, edge_case_name(*case))


@pytest.mark.parametrize("case", EDGE_CASES, ids=EDGE_IDS)
def test_edges_output_holds_the_input_in_order(edge_run, case):
    """Without the digests: the three files read back hold the input's pairs -- every barcode's (READS_PER_BC: those it keeps)
    as one entry of the index, bases with N as A, qualities as they were; the unbarcoded pairs in file order, inside a barcode
    the pairs descending by (read 1, read 2) under plain lexicographic comparison, equal pairs in file order."""
    _, _, _, pairs, (groups, _) = edge_run(case)
    per_bc = {}
    for bc, s1, s2, q1, q2 in pairs:
        assert max(len(s1), len(s2)) <= 1000 and max(q1 + q2) <= 63 and min(len(s1), len(s2)) >= 1
        per_bc.setdefault(bc, []).append((s1.replace("N", "A"), s2.replace("N", "A"), q1, q2))
    limit = max([int(e.split("=")[1]) for e in case[2] if e.startswith("READS_PER_BC=")], default=0)
    kept = {bc: v for bc, v in per_bc.items() if bc == 0 or not limit or 2 * len(v) < limit}
    assert not limit or 1 < len(kept) < len(per_bc), "READS_PER_BC must drop some barcodes and keep some"
    assert 7 <= len(per_bc) <= 13 and 0.05 < len(per_bc[0]) / len(pairs) < 0.2 and 200 <= len(pairs) <= 1500
    assert groups[0] == kept[0]
    assert sorted(sorted(g) for g in groups[1:]) == sorted(sorted(v) for bc, v in kept.items() if bc != 0)
    for g in groups[1:]:
        assert all((a[0], a[1]) >= (b[0], b[1]) for a, b in zip(g, g[1:])), "a barcode's pairs do not descend"
        v = next(v for bc, v in kept.items() if bc != 0 and sorted(v) == sorted(g))
        assert g == sorted(v, key=lambda p: (p[0], p[1]), reverse=True), "equal pairs left the file's order"      # (a stable sort)


@pytest.mark.parametrize("case", EDGE_CASES, ids=EDGE_IDS)
def test_edges_hold_what_they_are_for(edge_run, case):
    """Conditions on the generator, counted in the input and in the decoded output: neighbours that only a length orders (in the
    long profiles also by the second length byte alone), the lengths at the LDS kernel's limit, every PQVec width, a full block,
    minq at both ends."""
    _, _, _, pairs, (groups, blocks) = edge_run(case)
    long_profile = case[0] != "lds_edge"
    by_length, by_second_byte = 0, 0
    for g in groups[1:]:
        for a, b in zip(g, g[1:]):
            x, y = (a[0], b[0]) if a[0] != b[0] else (a[1], b[1])
            if only_a_length_orders(x, y):
                by_length += 1
                by_second_byte += (len(x) - len(y)) % 256 == 0
    assert by_length >= 20, by_length
    assert not long_profile or by_second_byte >= 5, by_second_byte
    out_lengths = {len(s) for g in groups for p in g for s in p[:2]}
    assert [max(len(p[f]) for p in pairs) for f in (1, 2)] == {"lds_edge": [256, 256], "long": [1000, 1000], "long_one_file": [151, 1000]}[case[0]]
    assert {1, 2, 3, 255, 256} <= out_lengths
    assert not long_profile or {257, 1000} <= out_lengths
    assert {b[1] for b in blocks} == set(range(7)), "PQVec widths"
    assert max(b[0] for b in blocks) == 255
    assert {0, 63} <= {b[2] for b in blocks}, "minq"
