"""CloseGap2's search for unplaced partners (10X/Closomatic.cc:554-585) restated in plain Python per pair, the file a.close.partners of
dfk_partners_write and its digest.

What is pinned on what: no reference-written form of this result exists (Closomatic.cc does not compile here), so the rule is pinned by
two restatements written independently from the reference's text -- this module and superplus_amd/csrc/dfk_partners.h.  The INPUTS are
tests/closer_oracle.py's per-edge results (locs and anchors, themselves made from reference-written paths, index and marks where the
fixtures hold them), the edges' bases from the fixture's reference-written a.fastb, and the reads of the fixture.

The text, for a pair (e1, e2), es = [e1, inv[e2]], L = 32:

  bod[ei]   :546-551.  for every anchor (g, add, count) of es[ei]: E = hb.O(g); for l in 0 .. len(E) - L: push( E[l:l+L], add + l ), the
            sum an int.  :561 UniqueSort( bod[ei] ).
  ids[ei]   :556-561.  the ids of the records of locs[ei] with fw true, UniqueSort.
  search    :562-585.  for ei in 0, 1: for id1 in ids[ei]: id2 = id1 + 1 if id1 even else id1 - 1; skip if BinMember( ids[1-ei], id2 );
            b = bases[id2]; finds = []; for l in 0 .. len(b) - L: x = b[l:l+L]; low = LowerBound1( bod[1-ei], x ); high = UpperBound1(
            bod[1-ei], x ); for m in low .. high - 1: finds.push( bod[1-ei][m].second - l ).  UniqueSort( finds ); if finds.solo( ):
            locs[1-ei].push( id2, finds[0], True ).
            ids[] were made before the loop: what ei = 0 pushes is not seen by ei = 1.

A 32-mer is kept as one number, base j of it at bits 2j: kmer<32> compares all 32 bases (kmers/KmerRecord.h:719-757) and only equality
decides a result, so any one-to-one key does."""
import bisect
import os
import struct

import numpy as np

from tests import closer_oracle
from tests.closer_oracle import i32, loc_words, seq_digest

L = 32
SALT = 0xDDDD
FILE = "a.close.partners"
MAGIC = b"DFKCPRT1"


def kmers_of(codes):
    """the 32-mers of a sequence of base codes, one number each: [] for fewer than 32 bases"""
    out, x = [], 0
    for i, b in enumerate(codes):
        x = (x >> 2) | (int(b) << 62)
        if i >= L - 1: out.append(x)
    return out


def bod_of(anchors, edge_bases):
    """:546-551 and :561 -> (sorted distinct [(32-mer, pos)], entries before UniqueSort)"""
    bod = []
    for g, add, _ in anchors:
        for l, x in enumerate(kmers_of(edge_bases[g])):
            bod.append((x, i32(add + l)))
    return sorted(set(bod)), len(bod)


def ids_of(locs):
    return sorted({id for id, _, fw in locs if fw})


def search(ids, ids_other, bod_other, read_bases):
    """:563-585 for one ei -> (the records pushed onto locs[1 - ei], counters; searched: the queries against a bod that is not empty)"""
    keys = [x for x, _ in bod_other]
    out, queries, positions, any_hit, multi = [], 0, 0, 0, 0
    for id1 in ids:
        id2 = id1 + 1 if id1 % 2 == 0 else id1 - 1
        if bisect.bisect_left(ids_other, id2) < len(ids_other) and ids_other[bisect.bisect_left(ids_other, id2)] == id2: continue     # BinMember
        queries += 1
        finds = []
        for l, x in enumerate(kmers_of(read_bases(id2))):
            positions += 1
            low, high = bisect.bisect_left(keys, x), bisect.bisect_right(keys, x)
            for m in range(low, high): finds.append(i32(bod_other[m][1] - l))
        finds = sorted(set(finds))
        if finds: any_hit += 1
        if len(finds) == 1: out.append((id2, finds[0], True))
        elif finds: multi += 1
    return out, dict(queries=queries, positions=positions, any_hit=any_hit, multi=multi, searched=queries if bod_other else 0)


def partners_file(starts, records):
    return closer_oracle.table_file(MAGIC, starts, loc_words(records).astype("<u8").tobytes())


def run(inv, edge_bases, ce, locs_per, anchors_per, pairs, read_bases):
    """inv per edge; edge_bases[g] the base codes of hb.O(g); ce ascending, locs_per / anchors_per the records per rank of ce; pairs
    [(e1, e2)]; read_bases(id) the base codes of read id -> dict(elements, starts, records, file, counters, digest)"""
    rank = {int(e): k for k, e in enumerate(ce)}
    bods, ids, memo = {}, {}, {}
    entries = 0
    for k in range(len(ce)):
        bods[k], n = bod_of(anchors_per[k], edge_bases)
        entries += n
        ids[k] = ids_of(locs_per[k])
    elements, tot = [], dict(queries=0, positions=0, any_hit=0, multi=0, searched=0)
    for e1, e2 in pairs:
        ks = [rank[int(e1)], rank[int(inv[e2])]]
        for ei in (0, 1):
            key = (ks[ei], ks[1 - ei])                    # the result depends on ( es[ei], es[1 - ei] ) alone
            if key not in memo: memo[key] = search(ids[ks[ei]], ids[ks[1 - ei]], bods[ks[1 - ei]], read_bases)
            recs, c = memo[key]
            elements.append(recs)
            for name in tot: tot[name] += c[name]
    records = [r for el in elements for r in el]
    starts = [0] + [int(x) for x in np.cumsum([len(el) for el in elements])]
    return dict(elements=elements, starts=starts, records=records, file=partners_file(starts, records), pairs=len(pairs), queries=tot["queries"],
                positions=tot["positions"], searched=tot["searched"], any_hit=tot["any_hit"], kept=len(records), multi=tot["multi"], entries=entries,
                largest_bod=max([len(b) for b in bods.values()] + [0]), digest=seq_digest(loc_words(records), SALT))


# ---- the fixtures
def unpack(packed, off, n):
    """n base codes of a 2-bit LSB-first stream starting at byte `off`"""
    b = np.asarray(packed[off:off + (n + 3) // 4], np.uint8)
    return ((b[:, None] >> np.array([0, 2, 4, 6], np.uint8)) & 3).reshape(-1)[:n]


def fastb_codes(path):
    from superplus_amd import feudal
    packed, off, lens = feudal.read_fastb(path)
    return [unpack(packed, int(off[i]), int(lens[i])) for i in range(len(lens))]


_cache = {}


def fixture_inputs(golden_dir, case, K, which):
    """what run() takes, of a fixture: closer_oracle's per-edge results, the bases of a.fastb, the fixture's reads"""
    if ("in", case) not in _cache:
        from tests.test_paths_oracle import load_reads
        c = closer_oracle.fixture_closer(golden_dir, case, K, which)
        i = closer_oracle.fixture_inputs(golden_dir, case, K, which)
        rs = load_reads(golden_dir, which)
        edge_bases = fastb_codes(os.path.join(golden_dir, case, "a.fastb"))
        assert len(edge_bases) == len(i["inv"]) and all(len(edge_bases[e]) == i["kmers"][e] + K - 1 for e in range(len(edge_bases)))
        read_bases = lambda id: unpack(rs["packed"], int(rs["base_off"][id]), int(rs["read_len"][id]))
        _cache[("in", case)] = dict(inv=i["inv"], edge_bases=edge_bases, ce=c["ce"], locs_per=[r["locs"] for r in c["per"]], anchors_per=[r["anchors"] for r in c["per"]],
                                    pairs=i["pairs"], read_bases=read_bases, rs=rs, dup=i["dup"])
    return _cache[("in", case)]


def fixture_partners(golden_dir, case, K, which):
    """run() on a fixture; computed once per session and handed out unchanged"""
    if case not in _cache:
        i = fixture_inputs(golden_dir, case, K, which)
        _cache[case] = run(i["inv"], i["edge_bases"], i["ce"], i["locs_per"], i["anchors_per"], i["pairs"], i["read_bases"])
    return _cache[case]
