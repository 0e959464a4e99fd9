"""tools/offsets_cost.py [--pairs N] [--genome-mb G] [--reps R] [--dir D] -- what GetOffsets1 per pair (dfk_offsets_build, dfk_offsets_write) costs.

One seeded set, generated on the device (the sets of tools/partners_cost.py); a context with DFK_F_MARK_BADS counts it, builds the graph,
paths the reads, marks the duplicates, builds the edge pairs, the closers' read sets, the partners and the stack consensus, then finds the
offsets and writes a.close.offsets into D (default /dev/shm) R times.  Prints one JSON line: of every repetition the counters (pairs,
candidates, passed, survivors, look-ups), the wall time of the build and of the write, and the split dfk_offsets_stats gives: HIP events
around the candidate kernels with their scan (us_candidates), the bits kernel (us_bits) and the scan and compaction of those that passed
(us_compact); wall time of the tail on the host (us_tail) and of the uploads and copies back (us_copy).  For scale the same pairs through
the literal form of csrc/dfk_offsets.h on one host thread (superplus_amd/test_offsets --literal), and the wall time of dfk_cons_build in
the same run; the device bytes held before and after (the same)."""
import argparse
import json
import os
import shutil
import subprocess
import sys
import tempfile
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from superplus_amd import synth  # noqa: E402
from superplus_amd.dfk import Dfk, LIB_PATH, OFFSETS_FILE  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--pairs", type=int, default=4_000_000)
ap.add_argument("--genome-mb", type=float, default=20.0)
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--dir", default="/dev/shm")
a = ap.parse_args()

dev = torch.device("cuda:0")
genome = synth.make_genome(int(a.genome_mb * 1e6), 20250, device=dev)
rs = synth.make_reads(genome, a.pairs, 20267)
del genome
torch.cuda.synchronize(); torch.cuda.empty_cache()
bc = rs.bc.cpu().numpy()
h_packed, h_off, h_len = rs.packed.cpu().numpy(), rs.base_off.cpu().numpy().astype(np.uint64), rs.read_len.cpu().numpy().astype(np.uint32)
h_pq, h_qoff = rs.pq_bytes.cpu().numpy(), rs.pq_off.cpu().numpy().astype(np.uint64)

d = Dfk(K=48, device=0, mark_bads=True)
d.count_device(rs.packed, rs.base_off, rs.read_len, rs.pq_bytes, rs.pq_off, rs.bc)
g = d.graph_build()
st = d.paths_build_device(rs.packed, rs.base_off, rs.read_len, rs.pq_bytes, rs.pq_off)
work = tempfile.mkdtemp(prefix="offsets_cost_", dir=a.dir)
try:
    d.dups_write(os.path.join(work, "a.dup"))
    dup = np.frombuffer(open(os.path.join(work, "a.dup"), "rb").read(), np.uint8, offset=16).copy()
    os.remove(os.path.join(work, "a.dup"))
    h = d.hops_build(bc)
    d.closer_build(dup)
    d.partners_build(h_packed, h_off, h_len)
    t = time.perf_counter()
    cs = d.cons_build(h_packed, h_off, h_len, h_pq, h_qoff)
    us_cons = int(1e6 * (time.perf_counter() - t))
    out = dict(lib=LIB_PATH, pairs=a.pairs, genome_mb=a.genome_mb, edges=g["n_edges"], reads=st["n_reads"], hops=h["pairs"], columns=cs["columns"], us_cons_build=us_cons,
               hbm_held_before=d.stats()["hbm_held"], runs=[])
    for _ in range(a.reps):
        t = time.perf_counter()
        s = d.offsets_build()
        wall_build = int(1e6 * (time.perf_counter() - t))
        t = time.perf_counter()
        d.offsets_write(work)
        wall_write = int(1e6 * (time.perf_counter() - t))
        out["runs"].append(dict(s, wall_build_us=wall_build, wall_write_us=wall_write, file_bytes=os.path.getsize(os.path.join(work, OFFSETS_FILE))))
    out["hbm_held_after"] = d.stats()["hbm_held"]
    # for scale: the literal form on one host thread
    c = d.cons_fetch()
    seqs = os.path.join(work, "seqs.bin")
    with open(seqs, "wb") as f:
        f.write(np.uint64(len(c["starts"]) // 2).tobytes()); f.write(np.ascontiguousarray(c["starts"], "<u8").tobytes()); f.write(np.ascontiguousarray(c["bases"], np.uint8).tobytes())
    exe = os.path.join(os.path.dirname(LIB_PATH), "test_offsets")
    out["host_literal"] = json.loads(subprocess.run([exe, "--literal", seqs], capture_output=True, text=True, check=True).stdout)
finally:
    shutil.rmtree(work, ignore_errors=True)
d.close()
print("OFFSETS_COST " + json.dumps(out))
