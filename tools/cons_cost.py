"""tools/cons_cost.py [--pairs N] [--genome-mb G] [--reps R] [--dir D] -- what CloseGap2's stack consensus (dfk_cons_build, dfk_cons_write) costs.

One seeded set, generated on the device (the sets of tools/partners_cost.py); a context with DFK_F_MARK_BADS counts it, builds the graph,
paths the reads, marks the duplicates (a.dup into D, read back), builds the edge pairs, the closers' read sets and the partners, then builds
the stack consensus -- the reads and their qualities handed over again as host arrays -- and writes a.close.cons into D (default /dev/shm) R
times.  Prints one JSON line: of every repetition the wall time of the build and of the write, the per-phase split (HIP events: the uploads
of the tables and lengths with the dimensions and live rows, the decode, the consensus; wall time: the gather of the reads on the host and
the copies), and the bytes each phase must move, from the counters:
  dims      uploads 16 bytes a locs record and a partner record and 4 a read (the lengths); reads a record and a length a row, twice (M, then
            the flag); writes 16 bytes a row of flags and places and 12 a live row
  copies    per read decoded its packed bases (a quarter byte a base), its PQVec bytes and 24 bytes of starts up, 4 bytes a live row up, a byte
            a column and 12 a stack down
  decode    reads the PQVec bytes, writes a byte a base
  consensus reads 24 bytes of header a live row and two bytes a cell added; writes a byte a column
Beside them the same run's us_paths and the wall times of dfk_closer_build and dfk_partners_build, for scale; the device bytes held before
and after (the same)."""
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
h_pq, h_qoff = rs.pq_bytes.cpu().numpy(), rs.pq_off.cpu().numpy().astype(np.uint64)

d = Dfk(K=48, device=0, mark_bads=True)
d.count_device(rs.packed, rs.base_off, rs.read_len, rs.pq_bytes, rs.pq_off, rs.bc)
g = d.graph_build()
st = d.paths_build_device(rs.packed, rs.base_off, rs.read_len, rs.pq_bytes, rs.pq_off)
work = tempfile.mkdtemp(prefix="cons_cost_", dir=a.dir)
try:
    n_dup = d.dups_write(os.path.join(work, "a.dup"))
    dup = np.frombuffer(open(os.path.join(work, "a.dup"), "rb").read(), np.uint8, offset=16).copy()
    os.remove(os.path.join(work, "a.dup"))
    h = d.hops_build(bc)
    t = time.perf_counter()
    cl = d.closer_build(dup)
    us_closer = int(1e6 * (time.perf_counter() - t))
    t = time.perf_counter()
    pt = d.partners_build(h_packed, h_off, h_len)
    us_partners = int(1e6 * (time.perf_counter() - t))
    out = dict(lib=LIB_PATH, pairs=a.pairs, genome_mb=a.genome_mb, edges=g["n_edges"], reads=st["n_reads"], hops=h["pairs"], closer_edges=cl["edges"], locs=cl["locs"],
               partners=pt["kept"], us_paths=d.stats()["us_paths"], us_closer_build=us_closer, us_partners_build=us_partners, hbm_held_before=d.stats()["hbm_held"], runs=[])
    mean_len = float(h_len.mean()) if len(h_len) else 0.0
    mean_pq = float(h_qoff[-1]) / max(1, len(h_len))
    for _ in range(a.reps):
        t = time.perf_counter()
        s = d.cons_build(h_packed, h_off, h_len, h_pq, h_qoff)
        wall_build = int(1e6 * (time.perf_counter() - t))
        t = time.perf_counter()
        d.cons_write(work)
        wall_write = int(1e6 * (time.perf_counter() - t))
        r = dict(s, wall_build_us=wall_build, wall_write_us=wall_write,
                 dims_bytes_at_least=16 * (cl["locs"] + pt["kept"]) + 4 * st["n_reads"] + (2 * 20 + 16) * s["rows"] + 12 * s["live"],
                 copy_bytes=int(s["decoded"] * (mean_len / 4 + mean_pq + 24)) + 4 * s["live"] + s["columns"] + 12 * s["stacks"],
                 decode_bytes=int(s["decoded"] * (mean_pq + mean_len)), consensus_bytes_at_least=24 * s["live"] + 2 * s["cells"] + s["columns"],
                 file_bytes=os.path.getsize(os.path.join(work, "a.close.cons")))
        out["runs"].append(r)
finally:
    shutil.rmtree(work, ignore_errors=True)
out["hbm_held_after"] = d.stats()["hbm_held"]
d.close()
print("CONS_COST " + json.dumps(out))
