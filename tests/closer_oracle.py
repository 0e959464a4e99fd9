"""The front end the two gap closers share -- CloseGap2 (10X/Closomatic.cc:503-552) and Stackster (10X/Stackster.cc:289-324) -- restated
in plain Python per closer edge, and the four files a.close.edges / a.close.locs / a.close.anchors / a.close.reads of dfk_closer_write.

What is pinned on what: no reference-written form of these sets exists (neither closer compiles here), so the rule is pinned by two
restatements written independently from the reference's text -- this module and superplus_amd/csrc/dfk_closer.h.  The INPUTS are the
reference's own where the fixtures hold them: a.paths (every fixture), a.paths.inv and a.dup (graph_frag_k48, graph_pathy2_k48), the
graph files; elsewhere the index and the marks come from oracle/paths_oracle.py, which tests/test_paths_oracle.py pins on
reference-written bytes.

The text, with `index[f]` for paths_index[f] (read ids ascending, a read listed once per occurrence of f on its path):

  closer edges   CloseGap2 works on es = { e1, inv[e2] } (Closomatic.cc:504), Stackster on e = ( spass == 1 ? e1 : inv[e2] )
                 (Stackster.cc:296): everything below depends on that one edge e.  ce = sorted set of them over the pairs.
  locs           Closomatic.cc:511-535.  for pass in 1, 2: f = e if pass == 1 else inv[e]; for id in index[f]; for j in range(n):
                 if p[j] == f: pos = offset - sum(kmers[p[l]] for l < j); locs.push( id, pos, pass == 1 ).
  prec           :519-530, inside the same `if`.  pass 1: add = 0; for l in j+1 .. n-1: add += kmers[p[l-1]]; push( p[l], add ).
                 pass 2: add = 0; for l in j-1 .. 0: add += kmers[p[l+1]]; push( inv[p[l]], add ).
  anchors        :536-552.  Sort(prec); every maximal run of equal pairs with j - i >= MIN_EDGE_COUNT (5) is kept: (g, add, j - i).
  reads          Stackster.cc:295-324 for spass == 1 (e = e1), ALT False.  :298-309: for pass in 1, 2, f as above, for id in index[f]:
                 skip if dup[id/2]; push( id, spass == 1 ^ pass == 2 ) = (id, pass == 1).  :310-322: for id1 in index[e]: skip if
                 dup[id1/2]; id2 = the mate; for j with p1[j] == e: pos1 as pos above; skip if kmers[e] + K - 1 - pos1 > MAX_DIST (800);
                 push( id2, spass == 2 ) = (id2, False).  :324 UniqueSort.
  a pair         spass == 2 runs the same loops on e = inv[e2] and pushes the negated flags: (id, pass == 2) and (id2, True).  So the
                 pair's idsfw is reads(e1) | {(id, not fw) for (id, fw) in reads(inv[e2])}; pair_idsfw() below runs both spasses as
                 the text has them, and the tests compare."""
import os
import struct

import numpy as np

MIN_EDGE_COUNT, MAX_DIST = 5, 800
SALT_EDGES, SALT_LOCS, SALT_ANCHORS, SALT_READS = 0x9999, 0xAAAA, 0xBBBB, 0xCCCC
FILES = ("a.close.edges", "a.close.locs", "a.close.anchors", "a.close.reads")
MAGIC = {"a.close.locs": b"DFKCLOC1", "a.close.anchors": b"DFKCANC1", "a.close.reads": b"DFKCRDS1"}


def i32(x):
    """the reference computes pos and add in an int"""
    return (int(x) + 2**31) % 2**32 - 2**31


def make_index(paths, n_edges):
    """paths_index as writePathsIndex leaves it: (edge, read) pairs sorted, a read that crosses an edge twice listed twice"""
    index = [[] for _ in range(n_edges)]
    for i, p in enumerate(paths):
        for e in p: index[e].append(i)
    return index


def index_from_file(b):
    """a.paths.inv (feudal VecULongVec) -> [[read ids]] per edge"""
    n = int.from_bytes(b[:4], "little")
    var_tab = int.from_bytes(b[8:16], "little")
    offs = np.frombuffer(b, "<u8", n + 1, var_tab)
    return [[int(x) for x in np.frombuffer(b, "<u8", (int(offs[i + 1]) - int(offs[i])) // 8, int(offs[i]))] for i in range(n)]


def closer_edges(pairs, inv):
    return sorted({int(a) for a, _ in pairs} | {int(inv[b]) for _, b in pairs})


def edge_sets(e, paths, offsets, index, kmers, inv, dup, K):
    """-> dict(locs [(id, pos, fw)], prec [(g, add)] unsorted, anchors [(g, add, count)], reads [(id, fw)] sorted distinct, counters)"""
    locs, prec = [], []
    for ps in (1, 2):
        f = e if ps == 1 else inv[e]
        for id in index[f]:
            p = paths[id]
            n = len(p)
            for j in range(n):
                if p[j] == f:
                    add = 0
                    if ps == 1:
                        for l in range(j + 1, n):
                            add += kmers[p[l - 1]]
                            prec.append((p[l], i32(add)))
                    else:
                        for l in range(j - 1, -1, -1):
                            add += kmers[p[l + 1]]
                            prec.append((inv[p[l]], i32(add)))
                    pos = offsets[id]
                    for l in range(j): pos -= kmers[p[l]]
                    locs.append((id, i32(pos), ps == 1))
    sp = sorted(prec)
    anchors, sizes, i = [], [], 0
    while i < len(sp):
        j = i + 1
        while j < len(sp) and sp[j] == sp[i]: j += 1
        sizes.append(j - i)
        if j - i >= MIN_EDGE_COUNT: anchors.append((sp[i][0], sp[i][1], j - i))
        i = j
    idsfw, dup_skipped, mates_in, mates_out, unplaced = [], 0, 0, 0, 0
    for ps in (1, 2):
        f = e if ps == 1 else inv[e]
        for id in index[f]:
            if dup[id // 2]:
                dup_skipped += 1
                continue
            idsfw.append((id, (1 == 1) ^ (ps == 2)))
    for id1 in index[e]:
        if dup[id1 // 2]: continue
        id2 = id1 + 1 if id1 % 2 == 0 else id1 - 1
        p1 = paths[id1]
        for j in range(len(p1)):
            if p1[j] == e:
                pos1 = offsets[id1]
                for l in range(j): pos1 -= kmers[p1[l]]
                if kmers[e] + K - 1 - i32(pos1) > MAX_DIST:
                    mates_out += 1
                    continue
                mates_in += 1
                unplaced += not paths[id2]
                idsfw.append((id2, False))
    return dict(locs=locs, prec=prec, anchors=anchors, reads=sorted(set(idsfw)), dup_skipped=dup_skipped, mates_in=mates_in, mates_out=mates_out,
                mates_unplaced=unplaced, run_sizes=sizes)


def pair_idsfw(e1, e2, paths, offsets, index, kmers, inv, dup, K):
    """Stackster.cc:295-324 for a pair, both spasses, as the text has them"""
    idsfw = []
    for spass in (1, 2):
        e = e1 if spass == 1 else inv[e2]
        for ps in (1, 2):
            f = e if ps == 1 else inv[e]
            for id in index[f]:
                if dup[id // 2]: continue
                idsfw.append((id, (spass == 1) ^ (ps == 2)))
        for id1 in index[e]:
            if dup[id1 // 2]: continue
            id2 = id1 + 1 if id1 % 2 == 0 else id1 - 1
            p1 = paths[id1]
            for j in range(len(p1)):
                if p1[j] == e:
                    pos1 = offsets[id1]
                    for l in range(j): pos1 -= kmers[p1[l]]
                    if kmers[e] + K - 1 - i32(pos1) > MAX_DIST: continue
                    idsfw.append((id2, spass == 2))
    return sorted(set(idsfw))


def compose(reads_e1, reads_inv_e2):
    return sorted(set(reads_e1) | {(id, not fw) for id, fw in reads_inv_e2})


# ---- the files
def edges_file(ce):
    return b"BINWRITE" + struct.pack("<Q", len(ce)) + np.asarray(ce, "<u8").tobytes()


def table_file(magic, starts, records):
    """magic | u64 n | n + 1 u64 starts | records"""
    return magic + struct.pack("<Q", len(starts) - 1) + np.asarray(starts, "<u8").tobytes() + records


def loc_words(locs):
    """a locs record {i64 id, i32 pos, u32 fw} as two little-endian 64-bit words"""
    w = np.zeros(2 * len(locs), np.uint64)
    for i, (id, pos, fw) in enumerate(locs):
        w[2 * i] = id
        w[2 * i + 1] = (pos % 2**32) | (int(bool(fw)) << 32)
    return w


def anchor_words(anchors):
    return np.asarray([x % 2**32 for a in anchors for x in a], np.uint32)


def read_words(reads):
    return np.asarray([(id << 1) | int(bool(fw)) for id, fw in reads], np.uint64)


def _mix(x):
    x = x ^ (x >> np.uint64(30)); x = x * np.uint64(0xBF58476D1CE4E5B9)
    x = x ^ (x >> np.uint64(27)); x = x * np.uint64(0x94D049BB133111EB)
    return x ^ (x >> np.uint64(31))


def seq_digest(values, salt):
    """k_digest_seq: (sum, xor) over positions i of h = mix(mix(i + salt) ^ v[i])"""
    v = np.asarray(values).astype(np.uint64)
    with np.errstate(over="ignore"):
        h = _mix(_mix(np.arange(len(v), dtype=np.uint64) + np.uint64(salt)) ^ v)
        x = _mix(h + np.uint64(0xD1B54A32D192ED03))
        return int(h.sum(dtype=np.uint64)), (int(np.bitwise_xor.reduce(x)) if len(x) else 0)


def run(paths, offsets, kmers, inv, pairs, dup, K, index=None):
    """paths [[edge ids]] and offsets per read, kmers and inv per edge, pairs [(e1, e2)], dup per PAIR of reads; index: paths_index as
    lists (None: made from the paths) -> dict(ce, per-edge results, the tables, files {name: bytes}, the counters, the digests)"""
    paths = [[int(e) for e in p] for p in paths]
    offsets = [int(x) for x in offsets]
    kmers = [int(x) for x in kmers]
    inv = [int(x) for x in inv]
    dup = [bool(x) for x in dup]
    assert len(paths) % 2 == 0 and len(dup) == len(paths) // 2 and len(offsets) == len(paths)
    if index is None: index = make_index(paths, len(inv))
    ce = closer_edges(pairs, inv)
    per = [edge_sets(e, paths, offsets, index, kmers, inv, dup, K) for e in ce]
    locs = [x for r in per for x in r["locs"]]
    anchors = [x for r in per for x in r["anchors"]]
    reads = [x for r in per for x in r["reads"]]
    starts = lambda key: [0] + [int(x) for x in np.cumsum([len(r[key]) for r in per])]
    lw, aw, rw = loc_words(locs), anchor_words(anchors), read_words(reads)
    files = {"a.close.edges": edges_file(ce),
             "a.close.locs": table_file(MAGIC["a.close.locs"], starts("locs"), lw.astype("<u8").tobytes()),
             "a.close.anchors": table_file(MAGIC["a.close.anchors"], starts("anchors"), aw.astype("<u4").tobytes()),
             "a.close.reads": table_file(MAGIC["a.close.reads"], starts("reads"), rw.astype("<u8").tobytes())}
    sizes = [s for r in per for s in r["run_sizes"]]
    total = lambda key: sum(r[key] for r in per)
    return dict(ce=ce, per=per, locs=locs, anchors=anchors, reads=reads, loc_first=starts("locs"), anchor_first=starts("anchors"), read_first=starts("reads"),
                files=files, prec=sum(len(r["prec"]) for r in per), dup_skipped=total("dup_skipped"), mates_in=total("mates_in"), mates_out=total("mates_out"),
                mates_unplaced=total("mates_unplaced"), runs_of_4=sizes.count(4), runs_of_5=sizes.count(5),
                longest=max([len(r["locs"]) for r in per] + [0]),
                digests={"a.close.edges": seq_digest(ce, SALT_EDGES), "a.close.locs": seq_digest(lw, SALT_LOCS),
                         "a.close.anchors": seq_digest(aw, SALT_ANCHORS), "a.close.reads": seq_digest(rw, SALT_READS)})


_cache = {}


def fixture_inputs(golden_dir, case, K, which):
    """what run() takes, of a fixture: a.paths as the reference wrote it; the index and the marks reference-written where the fixture
    holds them (graph_frag_k48, graph_pathy2_k48), else from oracle/paths_oracle.py; the pairs from tests/hops_oracle.py (ONE_GOOD off)"""
    key = ("in", case)
    if key not in _cache:
        from oracle import paths_oracle
        from tests.test_hops_oracle import fixture_hops, fixture_inputs as hops_inputs
        from tests.test_paths_oracle import decode_paths, load_reads
        i = hops_inputs(golden_dir, case, K, which)
        at = lambda f: os.path.join(golden_dir, case, f)
        with_off = decode_paths(open(at("a.paths"), "rb").read())
        inv = [int(x) for x in i["inv"]]
        if os.path.exists(at("a.paths.inv")): index = index_from_file(open(at("a.paths.inv"), "rb").read())
        else: index = index_from_file(paths_oracle.paths_index(with_off, inv)["a.paths.inv"])
        if os.path.exists(at("a.dup")): dup_file = open(at("a.dup"), "rb").read()
        else:
            reads, quals = paths_oracle.unpack_reads(load_reads(golden_dir, which))
            dup_file = paths_oracle.mark_dups(with_off, reads, quals)
        dup = np.frombuffer(dup_file, np.uint8, offset=16).copy()
        _cache[key] = dict(paths=[[int(e) for e in p] for _, p in with_off], offsets=[int(o) for o, _ in with_off], kmers=[int(x) for x in i["kmers"]], inv=inv,
                           pairs=[(int(a), int(b)) for a, b in fixture_hops(golden_dir, case, K, which)["pairs"]], dup=dup, K=K, index=index,
                           reference_index=os.path.exists(at("a.paths.inv")), reference_dup=os.path.exists(at("a.dup")))
    return _cache[key]


def fixture_closer(golden_dir, case, K, which):
    """run() on a fixture; computed once per session and handed out unchanged"""
    if case not in _cache:
        i = fixture_inputs(golden_dir, case, K, which)
        _cache[case] = run(i["paths"], i["offsets"], i["kmers"], i["inv"], i["pairs"], i["dup"], K, i["index"])
    return _cache[case]
