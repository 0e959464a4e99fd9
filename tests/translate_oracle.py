"""TranslatePaths and the Validate behind it, the end of StagePatch (10X/runstages/RunStages.cc:364-371), restated in plain Python from the
reference's text (paths/long/large/GapToyTools4.cc:163-196; OverlapAppend, Vec.h:593-606; ReadPath's clear() / resize(), paths/long/ReadPath.h:
24-88; ValidateReadPath, paths/long/ReadPathTools.cc:35-105), with the writer of a.patch.paths and its content digest.  Python lists for p,
OverlapAppend by its loop.  It shares nothing with superplus_amd/csrc/dfk_translate.h: what the library computes is held to this.

A path is (offset, [edges]); to3 a list of lists of hb3 edge ids, one per old edge; left3 a list; kmers3 hb3's edges' K-mer counts."""
import struct

M64 = (1 << 64) - 1
KINDS = ("empty_before", "cleared_empty", "step2", "walk", "cleared_ranoff")


def overlap_append(v1, v2):
    """Vec.h:593-606: the longest suffix of v1 that is a prefix of v2 is not appended again; -> that overlap"""
    best = 0
    for overl in range(min(len(v1), len(v2)), 0, -1):
        if v1[len(v1) - overl:] == v2[:overl]:
            best = overl
            break
    v1.extend(v2[best:])
    return best


def translate_one(path, to3, left3, kmers3, K):
    """-> ((offset, [edges]), kind, whether the walk left to3[path[0]], the overlaps OverlapAppend found)"""
    offset, edges = path
    if not edges:                                             # :168
        return (offset, []), "empty_before", False, []
    e0 = edges[0]
    start = offset + left3[e0]                                # :169
    if not to3[e0]:                                           # :171-173: clear() keeps the offset
        return (offset, []), "cleared_empty", False, []
    bases = lambda e: kmers3[e] + K - 1
    if start < bases(to3[e0][0]):                             # :175-179
        return (start, [to3[e0][0]]), "step2", False, []
    p, overlaps = [], []
    for e in edges:                                           # :182-184
        if not to3[e]:
            break
        overlaps.append(overlap_append(p, to3[e]))
    trim = 0
    while start >= bases(p[trim]):                            # :186-189
        start -= kmers3[p[trim]]
        trim += 1
        if trim == len(p):
            break
    left = trim >= len(to3[e0])                               # p begins with to3[e0]: the walk went past its end
    if trim == len(p):                                        # :191-193
        return (offset, []), "cleared_ranoff", left, overlaps
    return (start, [p[trim]]), "walk", left, overlaps         # :194-196


def validate_refuses(path, n_edges3):
    """ValidateReadPath with read_length = 0 on a path: only `edge_id >= edge_count` can fire (the offset tests cannot, one edge has no
    next edge to connect to)"""
    return any(e >= n_edges3 for e in path[1])


def paths_file(paths):
    """the feudal file ReadPathVec::WriteAll writes (feudal/FeudalFileWriter.cc:26-121): a 24-byte control block (n, flags 1, sizeofFixed 0,
    sizeofX 24, sizeofA 4, where the offsets start, where the file ends), per read {i32 offset, u32 lastSkip = 0, i32 edges...}, n + 1
    absolute u64 offsets"""
    var, offs = bytearray(), []
    for off, edges in paths:
        offs.append(24 + len(var))
        var += struct.pack("<iI", off, 0) + b"".join(struct.pack("<i", e) for e in edges)
    offs.append(24 + len(var))
    n = len(paths)
    var_tab = 24 + len(var)
    return struct.pack("<IBBBBQQ", n, 1, 0, 24, 4, var_tab, var_tab + 8 * (n + 1)) + bytes(var) + struct.pack("<%dQ" % (n + 1), *offs)


def _mix(x):
    x &= M64
    x ^= x >> 30; x = x * 0xBF58476D1CE4E5B9 & M64
    x ^= x >> 27; x = x * 0x94D049BB133111EB & M64
    return x ^ (x >> 31)


def paths_digest(paths):
    """(sum, xor) over reads r of h(r, offset, lastSkip, edges...), as DFK_CK_PATHS_SUM / _XOR are formed (include/dfk.h)"""
    s = x = 0
    for r, (off, edges) in enumerate(paths):
        h = _mix(r + 0x9E3779B97F4A7C15)
        for w in (off & 0xFFFFFFFF, 0, *(e & 0xFFFFFFFF for e in edges)):
            h = _mix(h ^ w)
        s = (s + h) & M64
        x ^= _mix(h + 0xD1B54A32D192ED03)
    return s, x


def run(paths, to3, left3, kmers3, K):
    """-> dict(paths, kinds, left, overlaps, file, digest, counters)"""
    out = [translate_one(p, to3, left3, kmers3, K) for p in paths]
    new = [o[0] for o in out]
    kinds = [o[1] for o in out]
    n = lambda k: sum(1 for x in kinds if x == k)
    c = dict(reads=len(paths), placed_before=sum(1 for _, e in paths if e), step2=n("step2"), walk=n("walk"), cleared_empty=n("cleared_empty"), cleared_ranoff=n("cleared_ranoff"),
             host=sum(1 for o in out if o[2]), invalid=sum(1 for p in new if validate_refuses(p, len(kmers3))),
             edge_changed=sum(1 for a, b in zip(paths, new) if a[1] and b[1] != a[1][:1]), offset_changed=sum(1 for a, b in zip(paths, new) if a[0] != b[0]),
             placed=sum(1 for _, e in new if e), var_bytes=sum(8 + 4 * len(e) for _, e in new))
    return dict(paths=new, kinds=kinds, left=[o[2] for o in out], overlaps=[o[3] for o in out], file=paths_file(new), digest=paths_digest(new), counters=c)
