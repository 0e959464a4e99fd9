"""tools/closures_cost.py [--pairs N] [--genome-mb G] [--reps R] [--dir D] -- what CloseGap2's closures per pair (dfk_closures_build, dfk_closures_write) cost.

One seeded set, generated on the device (the sets of tools/partners_cost.py and tools/cons_cost.py); a context with DFK_F_MARK_BADS counts
it, builds the graph, paths the reads, marks the duplicates, builds the edge pairs, the closers' read sets, the partners, the stack consensus
and the offsets, then builds the closures -- the reads and their qualities handed over again as host arrays -- and writes a.close.closures
into D (default /dev/shm) R times.  Prints one JSON line: of every repetition the counters (pairs, closable pairs, closures, columns, cells
added, live rows walked, empty columns), the wall time of the build and of the write, and the split dfk_closures_stats gives: HIP events
around the uploads of the tables and lengths with the dimensions and live rows of the closable pairs' stacks (us_dims), the decode
(us_decode) and the merged consensus (us_cons); wall time of the gather of the reads on the host and the copies either way (us_copy).
Beside them, of the same run, the wall times of dfk_cons_build and dfk_offsets_build with their own splits, for scale; the device bytes held
before and after (the same)."""
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
from superplus_amd.dfk import Dfk, LIB_PATH, CLOSURES_FILE  # noqa: E402

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
work = tempfile.mkdtemp(prefix="closures_cost_", dir=a.dir)
try:
    d.dups_write(os.path.join(work, "a.dup"))
    dup = np.frombuffer(open(os.path.join(work, "a.dup"), "rb").read(), np.uint8, offset=16).copy()
    os.remove(os.path.join(work, "a.dup"))
    h = d.hops_build(bc)
    d.closer_build(dup)
    d.partners_build(h_packed, h_off, h_len)
    t = time.perf_counter()
    cs = d.cons_build(h_packed, h_off, h_len, h_pq, h_qoff)
    wall_cons = int(1e6 * (time.perf_counter() - t))
    t = time.perf_counter()
    os_ = d.offsets_build()
    wall_offsets = int(1e6 * (time.perf_counter() - t))
    keep = lambda s, keys: {k: s[k] for k in keys}
    out = dict(lib=LIB_PATH, pairs=a.pairs, genome_mb=a.genome_mb, edges=g["n_edges"], reads=st["n_reads"], hops=h["pairs"],
               cons_build=dict(keep(cs, ("stacks", "rows", "live", "columns", "cells", "decoded", "us", "us_dims", "us_copy", "us_decode", "us_cons")), wall_us=wall_cons),
               offsets_build=dict(keep(os_, ("survivors", "closable", "pairs_more", "us", "us_candidates", "us_bits", "us_tail", "us_copy")), wall_us=wall_offsets),
               hbm_held_before=d.stats()["hbm_held"], runs=[])
    for _ in range(a.reps):
        t = time.perf_counter()
        s = d.closures_build(h_packed, h_off, h_len, h_pq, h_qoff)
        wall_build = int(1e6 * (time.perf_counter() - t))
        t = time.perf_counter()
        d.closures_write(work)
        wall_write = int(1e6 * (time.perf_counter() - t))
        out["runs"].append(dict(s, wall_build_us=wall_build, wall_write_us=wall_write, file_bytes=os.path.getsize(os.path.join(work, CLOSURES_FILE))))
finally:
    shutil.rmtree(work, ignore_errors=True)
out["hbm_held_after"] = d.stats()["hbm_held"]
d.close()
print("CLOSURES_COST " + json.dumps(out))
