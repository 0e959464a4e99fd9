"""tools/walks_cost.py [--pairs N] [--genome-mb G] [--reps R] [--sample S] [--dir D] -- what Stackster's stack walks (dfk_walks_build, dfk_walks_write) cost.

One seeded set, generated on the device (the sets of tools/cons_cost.py); a context with DFK_F_MARK_BADS counts it, builds the graph, paths
the reads, marks the duplicates (a.dup into D, read back), builds the edge pairs and the closers' read sets, then walks both stacks of every
pair -- the reads and their qualities handed over again as host arrays -- and writes a.stack.walks into D (default /dev/shm) R times.  Prints
one JSON line: of every repetition the wall time of the build and of the write and the split dfk_walks_stats gives -- us_copy: wall time of
the gather of the batches' distinct reads on the host and their upload; us_decode: HIP events around k_cn_decode and k_wk_lower; us_sort:
HIP events around k_wk_kmers, the radix sorts and k_wk_sorted of both sides; us_walk: HIP events around k_wk_walk, k_wk_collect and the
copies back -- with the walks, steps, live entries a step (live_sum / steps), the longest live list and the walks done on the host.

For scale the first S pairs (default 200) once more, as a set of their own with its reads renumbered: through dfk_walks_build_arrays (the
walk kernel's time on them) and through the literal form of csrc/dfk_walks.h on one host thread (superplus_amd/test_walks --literal), the
same pairs.  The device bytes held before and after (the same)."""
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
from superplus_amd.dfk import Dfk, LIB_PATH, WALKS_FILE  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--pairs", type=int, default=4_000_000)
ap.add_argument("--genome-mb", type=float, default=20.0)
ap.add_argument("--reps", type=int, default=2)
ap.add_argument("--sample", type=int, default=200)      # 0: the whole set alone
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
work = tempfile.mkdtemp(prefix="walks_cost_", dir=a.dir)
try:
    d.dups_write(os.path.join(work, "a.dup"))
    dup = np.frombuffer(open(os.path.join(work, "a.dup"), "rb").read(), np.uint8, offset=16).copy()
    os.remove(os.path.join(work, "a.dup"))
    h = d.hops_build(bc)
    t = time.perf_counter()
    cl = d.closer_build(dup)
    us_closer = int(1e6 * (time.perf_counter() - t))
    out = dict(lib=os.path.relpath(LIB_PATH, os.path.dirname(os.path.dirname(os.path.abspath(__file__)))), pairs=a.pairs, genome_mb=a.genome_mb, edges=g["n_edges"], reads=st["n_reads"], hops=h["pairs"], closer_edges=cl["edges"], set_entries=cl["reads"],
               us_paths=d.stats()["us_paths"], us_closer_build=us_closer, hbm_held_before=d.stats()["hbm_held"], runs=[])
    for _ in range(a.reps):
        t = time.perf_counter()
        s = d.walks_build(None, h_packed, h_off, h_len, h_pq, h_qoff)
        wall_build = int(1e6 * (time.perf_counter() - t))
        t = time.perf_counter()
        d.walks_write(work)
        wall_write = int(1e6 * (time.perf_counter() - t))
        out["runs"].append(dict(s, wall_build_us=wall_build, wall_write_us=wall_write, live_per_step=round(s["live_sum"] / max(1, s["steps"]), 2),
                                file_bytes=os.path.getsize(os.path.join(work, WALKS_FILE))))
    out["hbm_held_after"] = d.stats()["hbm_held"]
    # ---- for scale: the first S pairs as a set of their own, on the device and through the literal form on one host thread
    pairs = d.hops_fetch()[: a.sample]
    if len(pairs):
        c = d.closer_fetch()
        gdir = os.path.join(work, "graph"); os.makedirs(gdir)
        d.graph_write(gdir)
        e_packed, e_off, e_len = feudal.read_fastb(os.path.join(gdir, "a.fastb"))
        inv = np.frombuffer(open(os.path.join(gdir, "a.inv"), "rb").read(), "<i4", offset=16)
        rank = {int(e): k for k, e in enumerate(c["ce"])}
        need = sorted({int(p[0]) for p in pairs} | {int(inv[p[1]]) for p in pairs})
        idx = {e: j for j, e in enumerate(need)}
        code = lambda e: ((e_packed[int(e_off[e]): int(e_off[e]) + (int(e_len[e]) + 3) // 4][:, None] >> np.array([0, 2, 4, 6], np.uint8)) & 3).reshape(-1)[: int(e_len[e])].astype(np.uint8)
        edge_bases = []
        for e in need: edge_bases += [code(e), (3 - code(e))[::-1].copy()]
        sets = [c["reads"][int(c["read_first"][rank[e]]): int(c["read_first"][rank[e] + 1])] for e in need]
        ids = np.unique(np.concatenate([x >> np.uint64(1) for x in sets] + [np.zeros(0, np.uint64)]))
        ids = np.unique(np.concatenate([ids, ids ^ np.uint64(1)]))                       # (an even count: a read and its mate)
        renum = lambda x: (np.searchsorted(ids, x >> np.uint64(1)).astype(np.uint64) << np.uint64(1)) | (x & np.uint64(1))
        reads_per = [[(int(w) >> 1, bool(int(w) & 1)) for w in renum(x)] for x in sets]
        per = []
        for j in range(len(need)): per += [reads_per[j], []]
        rbases = [((h_packed[int(h_off[i]): int(h_off[i]) + (int(h_len[i]) + 3) // 4][:, None] >> np.array([0, 2, 4, 6], np.uint8)) & 3).reshape(-1)[: int(h_len[i])].astype(np.uint8) for i in ids]
        pq = np.concatenate([h_pq[int(h_qoff[i]): int(h_qoff[i + 1])] for i in ids] + [np.zeros(0, np.uint8)])
        pq_off = np.concatenate([[0], np.cumsum([int(h_qoff[i + 1]) - int(h_qoff[i]) for i in ids])]).astype(np.uint64)
        case = dict(inv=[e ^ 1 for e in range(2 * len(need))], kmers=[len(b) - 47 for b in edge_bases], K=48, edge_bases=edge_bases, ce=list(range(0, 2 * len(need), 2)),
                    reads_per=per[0::2], pairs=[(2 * idx[int(p[0])], 2 * idx[int(inv[p[1]])] + 1) for p in pairs], reads=rbases, pq=pq, pq_off=pq_off)
        from tests import walks_cases  # noqa: E402
        arr = walks_cases.arrays(case)
        t = time.perf_counter()
        ss = d.walks_build_arrays(arr)
        sample = dict(ss, wall_build_us=int(1e6 * (time.perf_counter() - t)), reads=len(ids))
        empty = dict(recs=[], walks=0, steps=0, live_sum=0, live_max=0)
        text = os.path.join(work, "sample.txt")
        open(text, "w").write("\n".join(walks_cases.case_text("sample", case, empty)) + "\n")
        exe = os.path.join(os.path.dirname(LIB_PATH), "test_walks")
        sample["host_literal"] = json.loads(subprocess.run([exe, "--literal", text], capture_output=True, text=True, check=True).stdout)
        out["sample"] = sample
finally:
    shutil.rmtree(work, ignore_errors=True)
d.close()
print("WALKS_COST " + json.dumps(out))
