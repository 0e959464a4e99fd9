"""tests/patch_oracle.py -- TEST INFRASTRUCTURE: plain-Python restatement of the statements of the reference's patching stage that put
the closures into the assembly (10X/runstages/RunStages.cc:330-360), for small cases.

What it restates (reference paths relative to lib/assembly/src):
  paths/long/large/GapToyTools4.cc:132-159   BuildAll: every edge, a (K+1)-mer per vertex crossing, then (RunStages.cc:342) the closures
  kmers/BigKPather.cc:40-55,97-106           BigKMerizer::kmerize: canonical K-mer -> OR of the contexts its occurrences show
  kmers/BigKPather.cc:112-307                BigKEdgeBuilder + buildHBVFromEdges: through oracle/graph_oracle.py's build_edges / build_hbv
  kmers/BigKPather.cc:310-353                Pather, for the old edges only (RunStages.cc:355-358): to3 and left3
and the writer of a.patch.to3 with its digest (superplus_amd/csrc/dfk_patch.h states the layout).

A graph here is a dict: K, edges (bytes of base codes 0-3 per edge), inv, to_left, to_right, n_vertices."""
import os
import struct

import numpy as np

from oracle import graph_oracle as go
from tests.subset_oracle import seq_digest

MAGIC = b"DFKPTO31"
SALT = 0x9A7C
FILES = ("a.k", "a.hbv", "a.hbx", "a.to_left", "a.to_right", "a.inv", "a.fastb", "a.kmers")


# ----------------------------------------------------------------------------------------------- BuildAll
def adjacency(g):
    """To(v) and From(v) as digraphE keeps them: by neighbouring vertex, equal neighbours by edge number"""
    to = [[] for _ in range(g["n_vertices"])]; frm = [[] for _ in range(g["n_vertices"])]
    for e in range(len(g["edges"])):
        frm[g["to_left"][e]].append((g["to_right"][e], e)); to[g["to_right"][e]].append((g["to_left"][e], e))
    return [[e for _, e in sorted(r)] for r in to], [[e for _, e in sorted(r)] for r in frm]


def build_all(g, closures):
    K = g["K"]
    allx = [bytes(s) for s in g["edges"]]                                   # :142-143
    to, frm = adjacency(g)
    for v in range(g["n_vertices"]):                                         # :150-159
        for e1 in to[v]:
            for e2 in frm[v]:
                x1, x2 = g["edges"][e1], g["edges"][e2]
                if not len(x1) or not len(x2):
                    continue
                allx.append(bytes(x1[len(x1) - K:]) + bytes(x2[K - 1:K]))
    n_cross = len(allx) - len(g["edges"])
    return allx + [bytes(c) for c in closures], n_cross                      # RunStages.cc:342


# ----------------------------------------------------------------------------------------------- kmerize
def kmer_int(s):
    x = 0
    for b in s:
        x = (x << 2) | b
    return x


def rolled(bv, K):
    """the K-mers of bv and their reverse complements as integers, each from the one before (BigKMer::successor)"""
    mask = (1 << (2 * K)) - 1
    k = kmer_int(bv[:K]); r = go._rc(k, K)
    yield k, r
    for b in bv[K:]:
        k = ((k << 2) | b) & mask; r = (r >> 2) | ((3 - b) << (2 * K - 2))
        yield k, r


def kmerize(bv, K, d):
    """BigKMerizer::kmerize + add + canonicalAdd: d[canonical K-mer] |= context (rc'd with the K-mer when it isRev())"""
    n = len(bv)
    if n < K:
        return
    for p, (k, r) in enumerate(rolled(bv, K)):
        ctx = 0
        if n > K:
            if p > 0:
                ctx |= 16 << bv[p - 1]                                       # predecessor bits: high nibble
            if p < n - K:
                ctx |= 1 << bv[p + K]                                        # successor bits: low nibble
        if r < k:                                                            # isRev(): stored as its reverse complement
            k, ctx = r, go._CTX_RC[ctx]
        d[k] = d.get(k, 0) | ctx


def solid_of(d, K):
    """the dict as graph_oracle's structured entries (w0, w1 left-aligned, context in count_ctx bits 24-31)"""
    a = np.zeros(len(d), dtype=[("w0", "<u8"), ("w1", "<u8"), ("count_ctx", "<u4")])
    for i, k in enumerate(sorted(d)):
        x = k << (128 - 2 * K)
        a[i] = (x >> 64, x & ((1 << 64) - 1), d[k] << 24)
    return a


# ----------------------------------------------------------------------------------------------- Pather
def pather(read, K, place, edges, fwd, rev):
    """Pather::operator() -> (ids, firstSkip)"""
    if len(read) < K:
        return [], 0

    def lookup(pos):
        # Pather::lookup, :356-363.  updateDict (:86-94) has left in the entry of a canonical K-mer where it lies on its edge, and mRC where
        # the edge shows its reverse complement; a read K-mer that isRev() gets pEnt->rc() (BigKMer.h:89-91), which turns both round.  So:
        # -> (edge, offset counted in the read's direction, isRC = the read runs against the edge as stored)
        w = bytes(read[pos:pos + K])
        k = kmer_int(w)
        e, off = place[min(k, go._rc(k, K))]
        if edges[e][off:off + K] == w:
            return e, off, False
        return e, len(edges[e]) - off - K, True

    e, off, rc = lookup(0)
    first_skip = off
    ids = [rev[e] if rc else fwd[e]]
    read_left = len(read); edge_left = len(edges[e]) - off
    while read_left > edge_left:
        read_left = read_left - edge_left + K - 1
        e, off, rc = lookup(len(read) - read_left)
        assert off == 0                                                      # ForceAssertEq, :341
        ids.append(rev[e] if rc else fwd[e])
        edge_left = len(edges[e])
    return ids, first_skip


# ----------------------------------------------------------------------------------------------- a.patch.to3
def to3_file(to3, left3):
    first = np.concatenate([[0], np.cumsum([len(p) for p in to3])]).astype("<u8")
    flat = np.asarray([i for p in to3 for i in p], "<i4")
    return MAGIC + struct.pack("<QQ", len(to3), len(flat)) + first.tobytes() + flat.tobytes() + np.asarray(left3, "<i4").tobytes()


def to3_digest(to3, left3):
    first = np.concatenate([[0], np.cumsum([len(p) for p in to3])]).astype(np.uint64)
    flat = np.asarray([i for p in to3 for i in p], np.uint64)
    return seq_digest(np.concatenate([first, flat, np.asarray(left3, np.uint64)]), SALT)


# ----------------------------------------------------------------------------------------------- the stage
def run(g, closures):
    K = g["K"]
    E = len(g["edges"])
    allx, n_cross = build_all(g, closures)
    base = {}
    for s in allx[:E + n_cross]:
        kmerize(s, K, base)
    d = dict(base)
    n_pos = n_found = 0
    for s in allx[E + n_cross:]:
        kmerize(s, K, d)
        if len(s) >= K:
            for k, r in rolled(s, K):
                n_pos += 1; n_found += min(k, r) in base
    bits_added = sum(bin(d[k] & ~base[k]).count("1") for k in base)
    edges, place = go.build_edges(solid_of(d, K), K)
    h = go.build_hbv(edges, K)
    files, E3 = go.graph_files(h)
    to3, left3 = [], []
    for e in range(E):
        ids, skip = pather(allx[e], K, place, edges, h.fwd, h.rev)
        to3.append(ids); left3.append(skip)
    out = {"a.patch." + f[2:]: files[f] for f in FILES}
    out["a.patch.to3"] = to3_file(to3, left3)
    L3, R3 = h.to_left_right()
    lens = [len(p) for p in to3]
    return dict(files=out, to3=to3, left3=left3, hbv=h, edges3=edges, inv3=h.involution(), to_left3=L3, to_right3=R3, kmers3=[len(s) - K + 1 for s in h.edges],
                digest=to3_digest(to3, left3),
                counters=dict(edges=E, canonical=sum(1 for e in range(E) if e <= g["inv"][e]), vertices=g["n_vertices"], crossings=n_cross, closures=len(closures),
                              short=sum(1 for c in closures if len(c) < K), positions=n_pos, found=n_found, new=n_pos - n_found, new_unique=len(d) - len(base),
                              bits_added=bits_added, kmers3=len(d), canonical3=len(edges), vertices3=len(h.frm), edges3=E3,
                              single3=sum(1 for s in edges if len(s) == K), path1=lens.count(1), path2=lens.count(2), path3=sum(1 for n in lens if n >= 3),
                              to3=sum(lens), left3=sum(1 for x in left3 if x)))


# ----------------------------------------------------------------------------------------------- fixtures
def unpack(packed, off, ln):
    out = []
    for i in range(len(ln)):
        b = np.frombuffer(packed, np.uint8, (int(ln[i]) + 3) // 4, int(off[i]))
        out.append(bytes(((b[:, None] >> np.array([0, 2, 4, 6], np.uint8)) & 3).reshape(-1)[:int(ln[i])].astype(np.uint8)))
    return out


def fixture_graph(golden_dir, case, K):
    from superplus_amd import feudal
    from tests.hops_oracle import read_ints
    d = os.path.join(golden_dir, case)
    packed, off, ln = feudal.read_fastb(os.path.join(d, "a.fastb"))
    to_left = read_ints(os.path.join(d, "a.to_left")); to_right = read_ints(os.path.join(d, "a.to_right"))
    nv = int(max(list(to_left) + list(to_right) + [-1])) + 1
    return dict(K=K, edges=unpack(packed.tobytes(), np.asarray(off, np.int64) - int(off[0]), ln), inv=[int(x) for x in read_ints(os.path.join(d, "a.inv"))],
                to_left=[int(x) for x in to_left], to_right=[int(x) for x in to_right], n_vertices=nv)
