"""tools/subset_cost.py [--pairs N] [--genome-mb G] [--reps R] [--dir D] -- what the subset of interest (dfk_subset_build, dfk_subset_write) costs.

One seeded set, generated on the device (the sets of tools/hops_cost.py); a context with DFK_F_MARK_BADS counts it, builds the graph, paths
the reads, builds the edge pairs, then builds the subset and writes its four files into D (default /dev/shm) R times.  Prints one JSON
line: of every repetition the wall time of the build and of the write, the per-phase split from HIP events (marks + sweep, the ids and
paths gather, the index subset), and the bytes each phase reads and writes, from the counters:
  marks + sweep   reads the batches once (4 bytes a read of elem_off, 8 of headers, 4 an edge) and writes a byte a read
  gather          reads 4 bytes a read of offsets (sizes), 4 + the taken elements (copy); writes 16 bytes a taken read (id, offset) and the elements
  index subset    reads the batches twice a range (count, list); sorts 8 bytes an entry a pass; writes 8 bytes an entry
with the achieved bytes per second of the sweep and of the gather.  Beside them the same run's us_paths, the wall time of the paths
index without files and of dfk_hops_build, for scale; the device bytes held before and after (the same); the subset's share of the reads."""
import argparse
import json
import os
import shutil
import sys
import tempfile
import time

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
t = time.perf_counter()
h = d.hops_build(bc)
us_hops = int(1e6 * (time.perf_counter() - t))
n, e = st["n_reads"], st["n_path_edges"]
batch_bytes = 12 * n + 4 * e                                             # elem_off, two header words, the edges
out = dict(lib=LIB_PATH, pairs=a.pairs, genome_mb=a.genome_mb, edges=g["n_edges"], reads=n, placed=st["n_placed"], path_edges=e, hops=h["pairs"],
           us_paths=d.stats()["us_paths"], us_hops_build=us_hops, hbm_held_before=d.stats()["hbm_held"], runs=[])
work = tempfile.mkdtemp(prefix="subset_cost_", dir=a.dir)
try:
    for _ in range(a.reps):
        t = time.perf_counter()
        b = d.subset_build(None)
        wall_build = int(1e6 * (time.perf_counter() - t))
        t = time.perf_counter()
        d.subset_write(work)
        wall_write = int(1e6 * (time.perf_counter() - t))
        s = d.subset_stats()
        taken_bytes = 8 * s["ids"] + 4 * s["path_entries"]
        sweep_bytes = batch_bytes + n                                    # the batches once; a byte a read of hits
        gather_bytes = (4 * n + 8 * s["ids"]) + (8 * n + taken_bytes + 16 * s["ids"] + taken_bytes)      # the build's sizes and ids; the write's sizes, copy in and out
        r = dict(s, wall_build_us=wall_build, wall_write_us=wall_write, us_gather_write=s["us_gather"] - b["us_gather"], us_index_write=s["us_index"] - b["us_index"],
                 sweep_bytes=sweep_bytes, gather_bytes=gather_bytes, index_bytes_written=8 * s["index_entries"],
                 files_bytes={f: os.path.getsize(os.path.join(work, f)) for f in sorted(os.listdir(work))},
                 sweep_GBps=round(sweep_bytes / max(1, s["us_sweep"]) / 1e3, 1), gather_GBps=round(gather_bytes / max(1, s["us_gather"]) / 1e3, 1),
                 share_of_reads=round(s["ids"] / max(1, n), 4))
        out["runs"].append(r)
finally:
    shutil.rmtree(work, ignore_errors=True)
out["hbm_held_after"] = d.stats()["hbm_held"]
t = time.perf_counter()
d.paths_index_write(None)
out["us_paths_index"] = int(1e6 * (time.perf_counter() - t))
d.close()
print("SUBSET_COST " + json.dumps(out))
