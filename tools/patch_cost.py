"""tools/patch_cost.py [--pairs N] [--genome-mb G] [--reps R] [--dir D] -- what the patched graph (dfk_patch_build, dfk_patch_write) costs.

One seeded set, generated on the device (the set of tools/sclosures_cost.py); a context with DFK_F_MARK_BADS counts it, builds the graph
(timed: dfk_graph_build of the same run, the figure to hold the patch beside), paths the reads, marks the duplicates, builds the edge
pairs, the closers' read sets and both closers' chains up to their closures, then builds the patched graph R times and writes a.patch.*
into D (default /dev/shm).  Prints one JSON line PATCH_COST (and PATCH_COST_SAMPLE, below): the wall time of graph_build, and of every repetition the wall time of the build and of
the write and the split dfk_patch_stats gives -- us_entries: HIP events around k_patch_entries; us_index: around the fill, k_graph_index and
k_patch_check over the old edges' K-mers; us_closures: around k_patch_closure_kmers and its counters' way back, all batches; us_sort: wall time
of the novel K-mers' sort and merge on the host; us_graph: events around the graph kernels over the two parts (their own index included);
us_number: wall time of build_hbv; us_paths: events around k_patch_heads, device_scan and k_patch_emit; us_copy: wall time of the tables unpacked and
checked, packing the edges and the closures, the uploads, the copies back and the paths' layout on the host -- with every counter and the device bytes held before
and after (the same).  Beside it the header's literal form (dfk_patch.h's literal(): BuildAll, kmerize into a std::map, BigKEdgeBuilder
as written, the Pather loop) on one host thread: on a SAMPLE, because a std::map of every K-mer of the whole set needs tens of gigabytes --
the first edges of the graph with their inverses up to --literal-bases bases and the first --literal-closures closures, a graph that holds
together by itself; tests/cpp/test_patch.cc is compiled with g++ -O2 and run on it (its "time" block), and dfk_patch_build_arrays of a
second context is timed on the same sample."""
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
from superplus_amd import feudal, synth  # noqa: E402
from superplus_amd.dfk import Dfk, LIB_PATH, PATCH_FILES  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--pairs", type=int, default=4_000_000)
ap.add_argument("--genome-mb", type=float, default=30.0)
ap.add_argument("--reps", type=int, default=2)
ap.add_argument("--dir", default="/dev/shm")
ap.add_argument("--literal-bases", type=int, default=2_000_000)
ap.add_argument("--literal-closures", type=int, default=300)
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


def ints(path):
    b = open(path, "rb").read()
    return np.frombuffer(b, "<i4", int.from_bytes(b[8:16], "little"), 16)


def unpacked(packed, off, ln, i):
    b = packed[int(off[i]):int(off[i]) + (int(ln[i]) + 3) // 4]
    return ((b[:, None] >> np.array([0, 2, 4, 6], np.uint8)) & 3).reshape(-1)[:int(ln[i])].astype(np.uint8)


def sample_run(d, work):
    """the literal form on one host thread and the device on the same sample of the graph and the closures"""
    d.graph_write(work); d.allclosures_write(work)
    packed, off, ln = feudal.read_fastb(os.path.join(work, "a.fastb"))
    off = np.asarray(off, np.int64) - int(off[0])
    inv, to_left, to_right = (ints(os.path.join(work, "a." + f)) for f in ("inv", "to_left", "to_right"))
    take, bases = [], 0
    for e in range(len(inv)):
        if inv[e] < e: continue
        take += [e] if inv[e] == e else [e, int(inv[e])]
        bases += int(ln[e]) * (1 if inv[e] == e else 2)
        if bases >= a.literal_bases: break
    new = {e: i for i, e in enumerate(take)}
    vs = {}
    for e in take:
        vs.setdefault(int(to_left[e]), len(vs)); vs.setdefault(int(to_right[e]), len(vs))
    edges = [unpacked(packed, off, ln, e) for e in take]
    cp, coff, cln = feudal.read_fastb(os.path.join(work, "a.closures.fastb"))
    coff = np.asarray(coff, np.int64) - int(coff[0])
    closures = [unpacked(cp, coff, cln, i) for i in range(min(len(cln), a.literal_closures))]
    s_inv = np.asarray([new[int(inv[e])] for e in take], np.int32)
    s_left = np.asarray([vs[int(to_left[e])] for e in take], np.int32); s_right = np.asarray([vs[int(to_right[e])] for e in take], np.int32)
    digits = lambda x: "".join(map(str, x.tolist())) or "-"
    row = lambda v: " ".join(str(int(x)) for x in v) or "-"
    path = os.path.join(work, "sample.txt")
    with open(path, "w") as f:
        f.write("\n".join(["time sample", row([48, len(vs), len(take), len(closures)]), row(s_inv), row(s_left), row(s_right)] + [digits(x) for x in edges] + [digits(x) for x in closures]) + "\n")
    bin_dir = tempfile.mkdtemp(prefix="patch_cost_bin_")                        # (not under D: /dev/shm may not run programs)
    try:
        exe = os.path.join(bin_dir, "test_patch")
        subprocess.run(["g++", "-O2", "-std=c++17", "-I", os.path.join(ROOT, "superplus_amd", "csrc"), "-o", exe, os.path.join(ROOT, "tests", "cpp", "test_patch.cc")], check=True, capture_output=True)
        r = subprocess.run([exe, path], capture_output=True, text=True, timeout=900)
    finally:
        shutil.rmtree(bin_dir, ignore_errors=True)
    lit = [json.loads(l.split(" ", 2)[2]) for l in r.stdout.splitlines() if l.startswith("LITERAL ")]
    def pack(x):
        y = np.concatenate([x, np.zeros((-len(x)) % 4, np.uint8)]).reshape(-1, 4)
        return (y[:, 0] | (y[:, 1] << 2) | (y[:, 2] << 4) | (y[:, 3] << 6)).astype(np.uint8)
    packs = [pack(x) for x in edges]
    eoff = np.concatenate([[0], np.cumsum([len(x) for x in packs])])[:-1].astype(np.uint64)
    starts = np.concatenate([[0], np.cumsum([len(x) for x in closures])]).astype(np.uint64)
    d2 = Dfk(K=48, device=0)
    runs = []
    for _ in range(2):
        t = time.perf_counter()
        s2 = d2.patch_build_arrays(s_inv, s_left, s_right, len(vs), np.concatenate(packs), eoff, np.asarray([len(x) for x in edges], np.uint32), starts,
                                   np.concatenate(closures) if closures else np.zeros(0, np.uint8))
        runs.append(dict(s2, wall_build_us=int(1e6 * (time.perf_counter() - t))))
    d2.close()
    return dict(edges=len(take), bases=bases, closures=len(closures), literal=lit[0] if lit else r.stdout[-300:] + r.stderr[-300:], device=runs)


d = Dfk(K=48, device=0, mark_bads=True)
cst = d.count_device(rs.packed, rs.base_off, rs.read_len, rs.pq_bytes, rs.pq_off, rs.bc)
t = time.perf_counter()
g = d.graph_build()
us_graph_build = int(1e6 * (time.perf_counter() - t))
st = d.paths_build_device(rs.packed, rs.base_off, rs.read_len, rs.pq_bytes, rs.pq_off)
work = tempfile.mkdtemp(prefix="patch_cost_", dir=a.dir)
try:
    d.dups_write(os.path.join(work, "a.dup"))
    dup = np.frombuffer(open(os.path.join(work, "a.dup"), "rb").read(), np.uint8, offset=16).copy()
    os.remove(os.path.join(work, "a.dup"))
    h = d.hops_build(bc)
    cl = d.closer_build(dup)
    t = time.perf_counter()
    d.partners_build(h_packed, h_off, h_len); d.cons_build(*reads); d.offsets_build(); c1 = d.closures_build(*reads)
    us_first = int(1e6 * (time.perf_counter() - t))
    t = time.perf_counter()
    d.walks_build(None, *reads); d.scons_build(*reads); d.soffsets_build(*reads); c2 = d.sclosures_build(*reads)
    us_second = int(1e6 * (time.perf_counter() - t))
    out = dict(lib=os.path.relpath(LIB_PATH, os.path.dirname(os.path.dirname(os.path.abspath(__file__)))), pairs=a.pairs, genome_mb=a.genome_mb, solid=d.solid_count(), edges=g["n_edges"],
               reads=st["n_reads"], hops=h["pairs"], closegap2_closures=c1["closures"], stackster_closures=c2["closures"], us_graph_build=us_graph_build,
               us_closegap2_chain=us_first, us_stackster_chain=us_second, hbm_held_before=d.stats()["hbm_held"], runs=[])
    for _ in range(a.reps):
        t = time.perf_counter()
        s = d.patch_build()
        wall_build = int(1e6 * (time.perf_counter() - t))
        t = time.perf_counter()
        d.patch_write(work)
        wall_write = int(1e6 * (time.perf_counter() - t))
        out["runs"].append(dict(s, wall_build_us=wall_build, wall_write_us=wall_write, file_bytes=sum(os.path.getsize(os.path.join(work, f)) for f in PATCH_FILES)))
    out["hbm_held_after"] = d.stats()["hbm_held"]
    print("PATCH_COST " + json.dumps(out), flush=True)
    print("PATCH_COST_SAMPLE " + json.dumps(sample_run(d, work)), flush=True)
finally:
    shutil.rmtree(work, ignore_errors=True)
d.close()
