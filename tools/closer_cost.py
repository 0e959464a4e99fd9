"""tools/closer_cost.py [--pairs N] [--genome-mb G] [--reps R] [--dir D] -- what the closers' read sets per edge (dfk_closer_build, dfk_closer_write) cost.

One seeded set, generated on the device (the sets of tools/hops_cost.py); a context with DFK_F_MARK_BADS counts it, builds the graph, paths
the reads, marks the duplicates (a.dup into D, read back), builds the edge pairs and the subset of interest, then builds the closers' sets
and writes their four files into D (default /dev/shm) R times.  Prints one JSON line: of every repetition the wall time of the build and
of the write, the per-phase split from HIP events (marks and ranks, the weights per rank, the ranges' sweeps, their sorts and compactions
with the copies to the host), and the bytes each phase must read and write, from the counters:
  weights   reads the batches once (4 bytes a read of elem_off, 8 of headers, 4 an edge) and half a byte a read of duplicate marks
  sweeps    reads the batches twice a range (count, emit) and writes 24 bytes a read of counts and places, 16 bytes a locs record, 12 a prec
            tuple, 8 a raw set entry
  sorts     8 bytes in and out a pass an element sorted (locs 1 sort, prec 3, set entries 2), the gathers, and the records out: 16 / 12 / 8
with the achieved bytes per second of the weights and of the sweeps.  Beside them the same run's us_paths and the wall times of
dfk_hops_build and dfk_subset_build, for scale; the device bytes held before and after (the same)."""
import argparse
import json
import os
import shutil
import sys
import tempfile
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from superplus_amd import synth  # noqa: E402
from superplus_amd.dfk import Dfk, LIB_PATH  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--pairs", type=int, default=4_000_000)
ap.add_argument("--genome-mb", type=float, default=20.0)
ap.add_argument("--reps", type=int, default=2)
ap.add_argument("--dir", default="/dev/shm")
a = ap.parse_args()

dev = torch.device("cuda:0")
genome = synth.make_genome(int(a.genome_mb * 1e6), 20250, device=dev)
rs = synth.make_reads(genome, a.pairs, 20267)
del genome
torch.cuda.synchronize(); torch.cuda.empty_cache()
bc = rs.bc.cpu().numpy()

d = Dfk(K=48, device=0, mark_bads=True)
d.count_device(rs.packed, rs.base_off, rs.read_len, rs.pq_bytes, rs.pq_off, rs.bc)
g = d.graph_build()
st = d.paths_build_device(rs.packed, rs.base_off, rs.read_len, rs.pq_bytes, rs.pq_off)
work = tempfile.mkdtemp(prefix="closer_cost_", dir=a.dir)
try:
    n_dup = d.dups_write(os.path.join(work, "a.dup"))
    dup = np.frombuffer(open(os.path.join(work, "a.dup"), "rb").read(), np.uint8, offset=16).copy()
    os.remove(os.path.join(work, "a.dup"))
    t = time.perf_counter()
    h = d.hops_build(bc)
    us_hops = int(1e6 * (time.perf_counter() - t))
    t = time.perf_counter()
    sub = d.subset_build(None)
    us_subset = int(1e6 * (time.perf_counter() - t))
    n, e = st["n_reads"], st["n_path_edges"]
    batch_bytes = 12 * n + 4 * e                                             # elem_off, two header words, the edges
    out = dict(lib=LIB_PATH, pairs=a.pairs, genome_mb=a.genome_mb, edges=g["n_edges"], reads=n, placed=st["n_placed"], path_edges=e, hops=h["pairs"], dup_pairs=n_dup,
               us_paths=d.stats()["us_paths"], us_hops_build=us_hops, us_subset_build=us_subset, subset_ids=sub["ids"], hbm_held_before=d.stats()["hbm_held"], runs=[])
    for _ in range(a.reps):
        t = time.perf_counter()
        s = d.closer_build(dup)
        wall_build = int(1e6 * (time.perf_counter() - t))
        t = time.perf_counter()
        d.closer_write(work)
        wall_write = int(1e6 * (time.perf_counter() - t))
        raw_entries = s["locs"] + s["mates_in"] - s["dup_skipped"]          # an upper bound of the raw set entries: a list entry each record at most, the mates let in
        weigh_bytes = batch_bytes + n // 2
        sweep_bytes = s["ranges"] * (2 * batch_bytes + n + 24 * n) + 16 * s["locs"] + 12 * s["prec"] + 8 * raw_entries
        sort_bytes = 16 * (s["locs"] + 3 * s["prec"] + 2 * raw_entries) + 16 * s["locs"] + 12 * s["anchors"] + 8 * s["reads"]
        r = dict(s, wall_build_us=wall_build, wall_write_us=wall_write, weigh_bytes=weigh_bytes, sweep_bytes=sweep_bytes, sort_bytes_at_least=sort_bytes,
                 files_bytes={f: os.path.getsize(os.path.join(work, f)) for f in sorted(os.listdir(work))},
                 weigh_GBps=round(weigh_bytes / max(1, s["us_weigh"]) / 1e3, 1), sweep_GBps=round(sweep_bytes / max(1, s["us_sweep"]) / 1e3, 1))
        out["runs"].append(r)
finally:
    shutil.rmtree(work, ignore_errors=True)
out["hbm_held_after"] = d.stats()["hbm_held"]
d.close()
print("CLOSER_COST " + json.dumps(out))
