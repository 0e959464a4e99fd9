"""tools/sclosures_cost.py [--pairs N] [--genome-mb G] [--reps R] [--dir D] -- what Stackster's closures (dfk_sclosures_build, dfk_sclosures_write) cost.

One seeded set, generated on the device (the set of tools/walks_cost.py); a context with DFK_F_MARK_BADS counts it, builds the graph, paths
the reads, marks the duplicates (a.dup into D, read back), builds the edge pairs, the closers' read sets, the two stack walks of every pair,
the stack consensus of every yielding pair and the stack offsets, then builds the closures -- the reads and their qualities handed over
again as host arrays -- and writes a.stack.closures into D (default /dev/shm) R times.  Prints one JSON line: the wall time of walks_build,
scons_build and soffsets_build of the same run, and of every repetition the wall time of the build and of the write and the split
dfk_sclosures_stats gives -- us_copy: wall time of the live rows and the gather of the batches' distinct reads on the host, their upload and
the copies back; us_decode: HIP events around k_cn_decode and k_wk_lower; us_cons: HIP events around k_scl_closures; us_rows: around
k_scl_rows and its counts' way back -- with every counter, the ( row, tile ) visits the consensus kernel skipped against those it made, and
the device bytes held before and after (the same)."""
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
from superplus_amd.dfk import Dfk, LIB_PATH, SCLOSURES_FILE  # noqa: E402

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
h_pq, h_qoff = rs.pq_bytes.cpu().numpy(), rs.pq_off.cpu().numpy().astype(np.uint64)
reads = (h_packed, h_off, h_len, h_pq, h_qoff)

d = Dfk(K=48, device=0, mark_bads=True)
d.count_device(rs.packed, rs.base_off, rs.read_len, rs.pq_bytes, rs.pq_off, rs.bc)
g = d.graph_build()
st = d.paths_build_device(rs.packed, rs.base_off, rs.read_len, rs.pq_bytes, rs.pq_off)
work = tempfile.mkdtemp(prefix="sclosures_cost_", dir=a.dir)
try:
    d.dups_write(os.path.join(work, "a.dup"))
    dup = np.frombuffer(open(os.path.join(work, "a.dup"), "rb").read(), np.uint8, offset=16).copy()
    os.remove(os.path.join(work, "a.dup"))
    h = d.hops_build(bc)
    cl = d.closer_build(dup)
    us = {}
    for name, call in (("walks", lambda: d.walks_build(None, *reads)), ("scons", lambda: d.scons_build(*reads)), ("soffsets", lambda: d.soffsets_build(*reads))):
        t = time.perf_counter()
        us[name] = call()
        us["us_%s_build" % name] = int(1e6 * (time.perf_counter() - t))
    out = dict(lib=os.path.relpath(LIB_PATH, os.path.dirname(os.path.dirname(os.path.abspath(__file__)))), pairs=a.pairs, genome_mb=a.genome_mb, edges=g["n_edges"], reads=st["n_reads"], hops=h["pairs"],
               closer_edges=cl["edges"], walks=us["walks"]["walks"], placed=us["walks"]["placed"], yields=us["walks"]["yields"], rows_kept=us["scons"]["rows_kept"], kept_offsets=us["soffsets"]["kept"],
               us_walks_build=us["us_walks_build"], us_scons_build=us["us_scons_build"], us_soffsets_build=us["us_soffsets_build"], hbm_held_before=d.stats()["hbm_held"], runs=[])
    for _ in range(a.reps):
        t = time.perf_counter()
        s = d.sclosures_build(*reads)
        wall_build = int(1e6 * (time.perf_counter() - t))
        t = time.perf_counter()
        d.sclosures_write(work)
        wall_write = int(1e6 * (time.perf_counter() - t))
        out["runs"].append(dict(s, wall_build_us=wall_build, wall_write_us=wall_write, file_bytes=os.path.getsize(os.path.join(work, SCLOSURES_FILE)),
                                skipped_share=float("%.4g" % (s["skipped"] / max(1, s["visits"])))))
    out["hbm_held_after"] = d.stats()["hbm_held"]
finally:
    shutil.rmtree(work, ignore_errors=True)
d.close()
print("SCLOSURES_COST " + json.dumps(out))
