"""FindEdgePairs (10X/Closomatic.cc:17-358, called from StagePatch, 10X/runstages/RunStages.cc:204-205; DF writes its
result as a.<K>/a.hops, 10X/DF.cc:603) restated in plain Python.

A COMPONENT-LEVEL PIN, like tests/bads_oracle.py: 10X/Closomatic.cc includes paths/HyperBasevector.h, which the recipe under
oracle/ cannot compile, so no file here was written by the reference's own function.  What this module restates is the rule;
what it works on -- a.paths, a.inv, a.to_left, a.to_right, a.fastb of tests/golden/graph_* -- was written by the reference's
classes.  superplus_amd/csrc/dfk_hops.h restates the same text a second time, in C++, independently of this module.

Names: N reads, the mate of id is id ^ 1, kmers(e) = hb.Kmers(e) = length - K + 1, bid[id] = N + bc[id] (:33-47 with the
data-set table of an LR= run, 10X/DfTools.cc:124-141: both branches give N + bc[id], all unbarcoded reads share N).

  method 1 (:54-120)   e1 passes the sink test (:63-74); e2 = inv[last edge of the mate's path] over the reads on e1, e2 != e1,
                       seen with >= 2 distinct bid; ONE_GOOD or e2 passes the source test (:101-111)
  method 2 (:126-179)  an e1 that passes the sink test and got nothing from method 1; e2 as above with kmers(e2) >= 100 and
                       ToRight(e1) != ToLeft(e2)
  method 3 (:191-341)  every e with kmers(e) >= K + 1 and >= 2 distinct bid among the reads on e and on inv[e]: the set X of
                       edge sequences seen to the right of e, the search for an extension of >= 100 k-mers built from
                       overlapping members of X; where there is none, every f with kmers(f) >= 40 seen with >= 2 distinct bid
                       among the not-bad reads' mates (can) and not directly behind e in a not-bad read's own path (too_easy)
  pairs = the sorted set union (:345)."""
import struct

import numpy as np

MAX_DIST_TO_END = 120      # :51
MIN_LANDING = 100          # :52
GOOD_EXT = 100             # :199
MIN_RIGHT = 40             # :200


def paths_index(paths, n_edges):
    """per edge the ascending ids of the reads whose path holds it (a.paths.inv; a read that crosses an edge twice is listed
    once -- the rule works on sets throughout, so a second listing would change nothing)"""
    idx = [[] for _ in range(n_edges)]
    for i, p in enumerate(paths):
        for e in sorted(set(p)):
            idx[e].append(i)
    return idx


def adjacency(to_left, to_right):
    """From(v) / To(v) as lists of edges"""
    nv = (max(max(to_left), max(to_right)) + 1) if len(to_left) else 0
    frm = [[] for _ in range(nv)]; to = [[] for _ in range(nv)]
    for e in range(len(to_left)):
        frm[to_left[e]].append(e); to[to_right[e]].append(e)
    return frm, to


def sink_ok(e1, kmers, to_right, frm, to):
    for e in frm[to_right[e1]]:                                  # :63-74
        w = to_right[e]
        if len(frm[w]) > 0 or len(to[w]) > 1 or kmers[e] > MAX_DIST_TO_END:
            return False
    return True


def source_ok(e2, kmers, to_left, frm, to):
    for e in to[to_left[e2]]:                                    # :101-111
        w = to_left[e]
        if len(to[w]) > 0 or len(frm[w]) > 1 or kmers[e] > MAX_DIST_TO_END:
            return False
    return True


def mate_set(e1, idx, paths, inv, bid):
    s = set()                                                    # :77-91
    for id1 in idx[e1]:
        p2 = paths[id1 ^ 1]
        if p2:
            e2 = inv[p2[-1]]
            if e2 != e1:
                s.add((e2, bid[id1]))
    return s


def supported(pairs):
    """the first members seen with at least two distinct second members, ascending"""
    n = {}
    for f, _ in pairs:
        n[f] = n.get(f, 0) + 1
    return sorted(f for f, c in n.items() if c >= 2)


def build_x(e, idx, paths, inv):
    re = inv[e]
    X = set()                                                    # :217-246
    for id1 in idx[e]:
        p1 = paths[id1]
        for j in range(len(p1)):
            if p1[j] == e:
                X.add(tuple(p1[j:]))
        p2 = paths[id1 ^ 1]
        if p2:
            X.add(tuple(inv[f] for f in reversed(p2)))
    for id_ in idx[re]:
        p = paths[id_]
        for j in range(len(p)):
            if p[j] == re:
                X.add(tuple(inv[p[l]] for l in range(j, -1, -1)))
    return sorted(X)


def search(e, X, kmers):
    """:256-292 -> (extended, rounds, largest |exts|, longest sequence); a round = one replacement of exts by exts2"""
    exts = [x for x in X if x[0] == e]
    rounds, most, longest = 0, len(exts), max([len(x) for x in exts], default=0)
    while True:
        for x in exts:
            if sum(kmers[f] for f in x[1:]) >= GOOD_EXT:
                return True, rounds, most, longest
        exts2 = set()
        for x in exts:
            f = x[-1]
            for y in X:
                for l in range(len(y) - 1):
                    if y[l] != f:
                        continue
                    mismatch = False
                    for m in range(len(y)):
                        n = m + len(x) - 1 - l
                        if n < 0 or n >= len(x):
                            continue
                        if x[n] != y[m]:
                            mismatch = True
                            break
                    if not mismatch:
                        exts2.add(x + y[l + 1:])
        if not exts2:
            return False, rounds, most, longest
        exts = sorted(exts2)
        rounds += 1
        most = max(most, len(exts)); longest = max(longest, max(len(x) for x in exts))


def rights(e, idx, paths, inv, kmers, bid, bad):
    re = inv[e]
    too_easy, can = set(), set()                                 # :297-338
    ok = lambda f: kmers[f] >= MIN_RIGHT and f != e and f != re
    for id1 in idx[e]:
        if bad[id1 // 2]:
            continue
        p1 = paths[id1]
        for j in range(len(p1)):
            if p1[j] == e:
                too_easy.update(f for f in p1[j + 1:] if ok(f))
        for f in (inv[g] for g in paths[id1 ^ 1]):
            if ok(f):
                can.add((f, bid[id1]))
    for id_ in idx[re]:
        if bad[id_ // 2]:
            continue
        p = paths[id_]
        for j in range(len(p)):
            if p[j] == re:
                for l in range(j + 1):
                    f = inv[p[l]]
                    if ok(f):
                        can.add((f, bid[id_]))
    return [f for f in supported(can) if f not in too_easy]


def hops_file(pairs):
    """bytes of a.hops: a vec<pair<int,int>> as BinaryWriter writes it (feudal/BinaryStream.h:447-462)"""
    a = np.asarray(pairs, "<i4").reshape(-1, 2)
    return b"BINWRITE" + struct.pack("<Q", len(a)) + a.tobytes()


def _mix(x):
    x = x ^ (x >> np.uint64(30)); x = x * np.uint64(0xBF58476D1CE4E5B9)
    x = x ^ (x >> np.uint64(27)); x = x * np.uint64(0x94D049BB133111EB)
    return x ^ (x >> np.uint64(31))


def hops_digest(pairs):
    """(sum, xor) over the pairs of h(first << 32 | second): order-independent, so the digests of disjoint sets add / xor"""
    a = np.asarray(pairs, np.int64).reshape(-1, 2)
    v = (a[:, 0].astype(np.uint64) << np.uint64(32)) | (a[:, 1].astype(np.uint64) & np.uint64(0xFFFFFFFF))
    with np.errstate(over="ignore"):
        h = _mix(v + np.uint64(0x9E3779B97F4A7C15))
        x = _mix(h + np.uint64(0xD1B54A32D192ED03))
        return int(h.sum(dtype=np.uint64)), (int(np.bitwise_xor.reduce(x)) if len(x) else 0)


def run(paths, kmers, inv, to_left, to_right, bc, bad, K, one_good=False):
    """paths [[edge ids]] per read, kmers / inv / to_left / to_right per edge, bc per read, bad per pair ->
    dict(m1, m2, m3, pairs, file, digest, and the counters of the search)"""
    paths = [list(p) for p in paths]
    kmers = [int(x) for x in kmers]; inv = [int(x) for x in inv]
    to_left = [int(x) for x in to_left]; to_right = [int(x) for x in to_right]
    N, E = len(paths), len(kmers)
    bid = [N + int(b) for b in bc]
    idx = paths_index(paths, E)
    frm, to = adjacency(to_left, to_right)
    m1, m2, m3 = [], [], []
    for e1 in range(E):
        if not sink_ok(e1, kmers, to_right, frm, to):
            continue
        sup = supported(mate_set(e1, idx, paths, inv, bid))
        got = [(e1, e2) for e2 in sup if one_good or source_ok(e2, kmers, to_left, frm, to)]
        m1 += got
        if not got:                                              # :128-130, 138: seen[e1]
            m2 += [(e1, e2) for e2 in sup if kmers[e2] >= MIN_LANDING and to_right[e1] != to_left[e2]]
    # searched: edges that reached the search; longest: the longest member of any X; longest_ext: the longest sequence the search built;
    # x_sizes[e] = (|X|, longest member of X, largest |exts|, longest extension): what decides whether the device can hold the edge
    c = dict(searched=0, extended=0, most_rounds=0, largest_x=0, largest_exts=0, longest=0, longest_ext=0, x_sizes={})
    for e in range(E):
        if kmers[e] < K + 1:                                     # :198, :204
            continue
        if len({bid[i] for i in idx[e]} | {bid[i] for i in idx[inv[e]]}) < 2:
            continue
        X = build_x(e, idx, paths, inv)
        ext, rounds, most, longest = search(e, X, kmers)
        c["searched"] += 1; c["extended"] += int(ext)
        c["most_rounds"] = max(c["most_rounds"], rounds); c["largest_x"] = max(c["largest_x"], len(X))
        lx = max(len(x) for x in X)
        c["largest_exts"] = max(c["largest_exts"], most); c["longest"] = max(c["longest"], lx); c["longest_ext"] = max(c["longest_ext"], longest)
        c["x_sizes"][e] = (len(X), lx, most, longest)
        if not ext:
            m3 += [(e, f) for f in rights(e, idx, paths, inv, kmers, bid, bad)]
    pairs = sorted(set(m1) | set(m2) | set(m3))
    return dict(m1=m1, m2=m2, m3=m3, pairs=pairs, file=hops_file(pairs), digest=hops_digest(pairs), **c)


def read_ints(path):
    """a vec<int> as BinaryWriter wrote it"""
    b = open(path, "rb").read()
    assert b[:8] == b"BINWRITE"
    return np.frombuffer(b, "<i4", int.from_bytes(b[8:16], "little"), 16)


def fixture_graph(golden_dir, case, K):
    """(kmers, inv, to_left, to_right) of tests/golden/<case>"""
    import os
    from superplus_amd import feudal
    d = os.path.join(golden_dir, case)
    _, _, ln = feudal.read_fastb(os.path.join(d, "a.fastb"))
    return (np.asarray(ln, np.int64) - K + 1, read_ints(os.path.join(d, "a.inv")), read_ints(os.path.join(d, "a.to_left")),
            read_ints(os.path.join(d, "a.to_right")))
