"""tools/partners_cost.py [--pairs N] [--genome-mb G] [--reps R] [--dir D] -- what CloseGap2's search for unplaced partners (dfk_partners_build, dfk_partners_write) costs.

One seeded set, generated on the device (the sets of tools/hops_cost.py); a context with DFK_F_MARK_BADS counts it, builds the graph, paths
the reads, marks the duplicates (a.dup into D, read back), builds the edge pairs and the closers' read sets, then searches for the partners
-- the reads handed over again as host arrays -- and writes a.close.partners into D (default /dev/shm) R times.  Prints one JSON line: of
every repetition the wall time of the build and of the write, the per-phase split (HIP events: the queries with the uploads of the closer's
tables, the table, the search; wall time: the gather of the reads' bases on the host and the copies), and the bytes each phase must move, from
the counters:
  queries   uploads 16 bytes a locs record; reads 16 a forward record of a side and a binary search of the other side's; writes 16 bytes an
            item of flags and places and 8 a query
  table     writes 16 bytes an entry, sorts them in two or three passes of 8 bytes in and out an element and pass of 8 bits, writes 12 a sorted entry
  search    reads the bytes of the searched reads nine a position, and log2(slice) + 1 keys of 8 bytes a position
  copies    the bases of the searched reads (a quarter byte a base) and 16 bytes a query up, 8 bytes a kept record down
Beside them the same run's us_paths and the wall time of dfk_closer_build, for scale; the device bytes held before and after (the same)."""
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
h_packed, h_off, h_len = rs.packed.cpu().numpy(), rs.base_off.cpu().numpy().astype(np.uint64), rs.read_len.cpu().numpy().astype(np.uint32)

d = Dfk(K=48, device=0, mark_bads=True)
d.count_device(rs.packed, rs.base_off, rs.read_len, rs.pq_bytes, rs.pq_off, rs.bc)
g = d.graph_build()
st = d.paths_build_device(rs.packed, rs.base_off, rs.read_len, rs.pq_bytes, rs.pq_off)
work = tempfile.mkdtemp(prefix="partners_cost_", dir=a.dir)
try:
    n_dup = d.dups_write(os.path.join(work, "a.dup"))
    dup = np.frombuffer(open(os.path.join(work, "a.dup"), "rb").read(), np.uint8, offset=16).copy()
    os.remove(os.path.join(work, "a.dup"))
    h = d.hops_build(bc)
    t = time.perf_counter()
    cl = d.closer_build(dup)
    us_closer = int(1e6 * (time.perf_counter() - t))
    out = dict(lib=LIB_PATH, pairs=a.pairs, genome_mb=a.genome_mb, edges=g["n_edges"], reads=st["n_reads"], hops=h["pairs"], closer_edges=cl["edges"], locs=cl["locs"],
               anchors=cl["anchors"], us_paths=d.stats()["us_paths"], us_closer_build=us_closer, hbm_held_before=d.stats()["hbm_held"], runs=[])
    for _ in range(a.reps):
        t = time.perf_counter()
        s = d.partners_build(h_packed, h_off, h_len)
        wall_build = int(1e6 * (time.perf_counter() - t))
        t = time.perf_counter()
        d.partners_write(work)
        wall_write = int(1e6 * (time.perf_counter() - t))
        mean_len = float(h_len.mean()) if len(h_len) else 0.0
        slice_keys = int(np.ceil(np.log2(max(2, s["entries"] / max(1, cl["edges"]))))) + 1
        r = dict(s, wall_build_us=wall_build, wall_write_us=wall_write,
                 query_bytes_at_least=16 * cl["locs"] + 8 * s["queries"], table_bytes_at_least=(16 + 2 * 4 * 16 + 12) * s["entries"],
                 search_bytes_at_least=s["positions"] * s["searched"] // max(1, s["queries"]) * (9 + 8 * slice_keys),
                 copy_bytes=int(s["searched"] * (mean_len / 4 + 16)) + 8 * s["kept"], file_bytes=os.path.getsize(os.path.join(work, "a.close.partners")))
        out["runs"].append(r)
finally:
    shutil.rmtree(work, ignore_errors=True)
out["hbm_held_after"] = d.stats()["hbm_held"]
d.close()
print("PARTNERS_COST " + json.dumps(out))
