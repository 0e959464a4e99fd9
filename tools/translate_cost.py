"""tools/translate_cost.py [--pairs N] [--genome-mb G] [--reps R] [--dir D] -- what moving the read paths onto the patched graph
(dfk_translate_build, dfk_translate_write) costs.

One seeded set, generated on the device (the set of tools/patch_cost.py); a context with DFK_F_MARK_BADS counts it, builds the graph, paths
the reads (timed: dfk_paths_build of the same run, the figure to hold the translation beside), marks the duplicates, builds the edge pairs,
the closers' read sets, both closers' chains and the patched graph, then translates the paths R times and writes a.patch.paths into D
(default /dev/shm).  Prints one JSON line TRANSLATE_COST: of every repetition the wall time of the build and of the write and the split
dfk_translate_stats gives -- us_decide: HIP events around k_tp_decide and its flagged count's way back, all batches; us_host: wall time of the
host route; us_scan: events around the scans and their totals' way back; us_emit: events around k_tp_emit; us_copy: wall time of the tables
checked and sent, the scratch, the counters' way back -- with every counter, the bytes each kernel reads and writes by its arguments (decide:
a read's 4-byte element offset, its offset word and first edge id, 8 bytes of record out; emit: the record in, the element and its 4-byte
offset out; the gathers into the tables are not counted) and the rate that gives, and the device bytes held before the first build, with a
result, and after dfk_translate_drop.  Beside it dfk_translate.h's literal() on one host thread over the same reads and tables
(tests/cpp/test_translate.cc --time, g++ -O2), whose digest must be the device's."""
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
from superplus_amd.dfk import Dfk, LIB_PATH, TRANSLATE_FILE  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--pairs", type=int, default=4_000_000)
ap.add_argument("--genome-mb", type=float, default=30.0)
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
reads = (h_packed, h_off, h_len, h_pq, h_qoff)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def literal_run(d, work):
    """dfk_translate.h's literal() on one host thread over the context's paths and the patch's tables"""
    off, first, edges = d.paths()
    t = d.patch_fetch()
    path = os.path.join(work, "translate_time.bin")
    with open(path, "wb") as f:
        np.asarray([48, len(t["left3"]), len(t["to3"]), len(t["kmers"]), len(off), len(edges)], "<u8").tofile(f)
        for x, ty in ((t["to3_first"], "<u8"), (t["to3"], "<i4"), (t["left3"], "<i4"), (t["kmers"], "<i4"), (off, "<i4"), (first, "<u8"), (edges, "<i4")):
            np.ascontiguousarray(x, ty).tofile(f)
    bin_dir = tempfile.mkdtemp(prefix="translate_cost_bin_")                    # (not under D: /dev/shm may not run programs)
    try:
        exe = os.path.join(bin_dir, "test_translate")
        subprocess.run(["g++", "-O2", "-std=c++17", "-I", os.path.join(ROOT, "superplus_amd", "csrc"), "-o", exe, os.path.join(ROOT, "tests", "cpp", "test_translate.cc")], check=True, capture_output=True)
        r = subprocess.run([exe, "--time", path], capture_output=True, text=True, timeout=900)
    finally:
        shutil.rmtree(bin_dir, ignore_errors=True)
        os.remove(path)
    lit = [json.loads(l.split(" ", 1)[1]) for l in r.stdout.splitlines() if l.startswith("LITERAL ")]
    return lit[0] if lit else r.stdout[-300:] + r.stderr[-300:]


d = Dfk(K=48, device=0, mark_bads=True)
d.count_device(rs.packed, rs.base_off, rs.read_len, rs.pq_bytes, rs.pq_off, rs.bc)
g = d.graph_build()
t = time.perf_counter()
st = d.paths_build_device(rs.packed, rs.base_off, rs.read_len, rs.pq_bytes, rs.pq_off)
us_paths_build = int(1e6 * (time.perf_counter() - t))
work = tempfile.mkdtemp(prefix="translate_cost_", dir=a.dir)
try:
    d.dups_write(os.path.join(work, "a.dup"))
    dup = np.frombuffer(open(os.path.join(work, "a.dup"), "rb").read(), np.uint8, offset=16).copy()
    os.remove(os.path.join(work, "a.dup"))
    d.hops_build(bc)
    d.closer_build(dup)
    d.partners_build(h_packed, h_off, h_len); d.cons_build(*reads); d.offsets_build(); d.closures_build(*reads)
    d.walks_build(None, *reads); d.scons_build(*reads); d.soffsets_build(*reads); d.sclosures_build(*reads)
    p = d.patch_build()
    held0 = d.stats()["hbm_held"]
    out = dict(lib=os.path.relpath(LIB_PATH, ROOT), pairs=a.pairs, genome_mb=a.genome_mb, edges=g["n_edges"], reads=st["n_reads"], path_edges=st["n_path_edges"],
               us_paths_build=us_paths_build, us_paths_stat=d.stats()["us_paths"], edges3=p["edges3"], to3=p["to3"], left3=p["left3"], hbm_held_before=held0, runs=[])
    for _ in range(a.reps):
        t = time.perf_counter()
        s = d.translate_build()
        wall_build = int(1e6 * (time.perf_counter() - t))
        t = time.perf_counter()
        d.translate_write(work)
        wall_write = int(1e6 * (time.perf_counter() - t))
        n = s["reads"]
        decide_bytes, emit_bytes = n * (4 + 8 + 8), n * (8 + 4) + s["var_bytes"]
        out["runs"].append(dict(s, wall_build_us=wall_build, wall_write_us=wall_write, file_bytes=os.path.getsize(os.path.join(work, TRANSLATE_FILE)), decide_bytes=decide_bytes,
                                emit_bytes=emit_bytes, decide_gb_s=round(decide_bytes / max(1, s["us_decide"]) / 1e3, 1), emit_gb_s=round(emit_bytes / max(1, s["us_emit"]) / 1e3, 1)))
    out["hbm_held_with_result"] = d.stats()["hbm_held"]
    out["literal"] = literal_run(d, work)
    d.translate_drop()
    out["hbm_held_after_drop"] = d.stats()["hbm_held"]
    print("TRANSLATE_COST " + json.dumps(out), flush=True)
finally:
    shutil.rmtree(work, ignore_errors=True)
d.close()
