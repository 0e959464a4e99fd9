"""tools/bads_cost.py [--pairs N] [--genome-mb G] [--reps R] [--off-only] -- what gathering MarkBads' sums costs the pathing.

One seeded set, generated on the device; in one process a context without DFK_F_MARK_BADS and one with it each count the
set, build the graph and path the reads R times.  Prints one JSON line: dfk_stats' us_paths (reserved[3]: the whole build
on the device, from HIP events) of every repetition for both contexts, and k_bad_sums' share of it (reserved[7]: HIP events
around the kernel alone).  --off-only leaves the second context out: with DFK_LIB pointing at a library built from the
parent commit this gives the parent's figure on the same set and machine (run it three times for the run-to-run spread).
Under `rocprofv3 --kernel-trace --stats -- python tools/bads_cost.py ...` the kernel's own line is in the statistics."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from superplus_amd import synth  # noqa: E402
from superplus_amd.dfk import Dfk, LIB_PATH  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--pairs", type=int, default=3_000_000)
ap.add_argument("--genome-mb", type=float, default=20.0)
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--off-only", action="store_true")
a = ap.parse_args()

dev = torch.device("cuda:0")
genome = synth.make_genome(int(a.genome_mb * 1e6), 20250, device=dev)
rs = synth.make_reads(genome, a.pairs, 20267)
del genome
torch.cuda.synchronize(); torch.cuda.empty_cache()

out = dict(lib=LIB_PATH, pairs=a.pairs, genome_mb=a.genome_mb)
for name, flag in (("off", False),) + ((() if a.off_only else (("on", True),))):
    d = Dfk(K=48, device=0, mark_bads=flag)
    d.count_device(rs.packed, rs.base_off, rs.read_len, rs.pq_bytes, rs.pq_off, rs.bc)
    d.graph_build()
    us, us_bads = [], []
    for _ in range(a.reps):
        st = d.paths_build_device(rs.packed, rs.base_off, rs.read_len, rs.pq_bytes, rs.pq_off)
        s = d.stats()
        us.append(s["us_paths"]); us_bads.append(s["us_bad_sums"])
    out[name] = dict(us_paths=us, us_bad_sums=us_bads, placed=st["n_placed"], hbm_held=d.stats()["hbm_held"])
    if flag:
        marked, digest = d.bads_write(None)
        out[name]["bad_pairs"] = marked
    d.close()
if "on" in out:
    off, on = min(out["off"]["us_paths"]), min(out["on"]["us_paths"])
    out["added_us"] = on - off
    out["added_share"] = round((on - off) / off, 4)
    out["kernel_share_of_on"] = round(min(out["on"]["us_bad_sums"]) / on, 4)
print("BADS_COST " + json.dumps(out))
