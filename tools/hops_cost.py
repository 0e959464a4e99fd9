"""tools/hops_cost.py [--pairs N] [--genome-mb G] [--reps R] [--one-good] -- what FindEdgePairs (dfk_hops_build) costs.

One seeded set, generated on the device; a context with DFK_F_MARK_BADS counts it, builds the graph, paths the reads and
builds the edge pairs R times.  Prints one JSON line: of every repetition the call's wall time and the per-kernel split from
HIP events (the combined index, the kernels of methods 1 and 2, the kernel of method 3), the edges decided on the host and that
route's wall time; beside them the same run's us_paths (dfk_stats' reserved[3]) and the wall time of the paths index
(dfk_paths_index_write without files), for scale; and the device bytes held before and after the builds (the same).
DFK_HOPS_MAX_SEQS / DFK_HOPS_MAX_LEN in the environment move edges between the device and the host route."""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from superplus_amd import synth  # noqa: E402
from superplus_amd.dfk import Dfk, LIB_PATH  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--pairs", type=int, default=4_000_000)
ap.add_argument("--genome-mb", type=float, default=20.0)
ap.add_argument("--reps", type=int, default=2)
ap.add_argument("--one-good", action="store_true")
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
out = dict(lib=LIB_PATH, pairs=a.pairs, genome_mb=a.genome_mb, one_good=a.one_good, edges=g["n_edges"], placed=st["n_placed"], path_edges=st["n_path_edges"],
           us_paths=d.stats()["us_paths"], hbm_held_before=d.stats()["hbm_held"], builds=[])
for _ in range(a.reps):
    t = time.perf_counter()
    h = d.hops_build(bc, a.one_good)
    h["wall_us"] = int(1e6 * (time.perf_counter() - t))
    out["builds"].append(h)
out["hbm_held_after"] = d.stats()["hbm_held"]
out["digest"] = "%016x%016x" % d.hops_write(None)[1]
t = time.perf_counter()
d.paths_index_write(None)
out["us_paths_index"] = int(1e6 * (time.perf_counter() - t))
d.close()
print("HOPS_COST " + json.dumps(out))
