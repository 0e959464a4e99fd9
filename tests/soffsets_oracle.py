"""Stackster's stack offsets per pair (10X/Stackster.cc:461-645: the acceptable 8-mers of one stack's consensus, the rows of the other
stack searched for them, the bits of a ( row, offset ), the filter over the results) restated in plain Python per pair, the file
a.stack.offsets of dfk_soffsets_write and its digest.

What is pinned on what: no reference-written form of this result exists (Stackster.cc does not compile here), so the rule is pinned by
two restatements written independently from the reference's text -- this module and superplus_amd/csrc/dfk_soffsets.h.  The INPUTS are
the walks of tests/walks_oracle.py, the reads with their PQVec qualities, and con and the conflict counts of tests/scons_oracle.py.

The text, for a pair that reaches :461 (both sides placed an entry), ALT = False, EXP = False:

  the stacks  as tests/scons_oracle.build_stack leaves them after Trim and Reverse: grids with ' ' (here -1) and quality -1 where no read
            stands; a quality of 128 or more is negative in its char: Def( r, c ) is Qual >= 0, and the base of such a cell is the read's.
  :499-517  for s in 0, 1: s1 = stacks[s], s2 = stacks[1 - s], con1 = the consensus of side s.  bbs: every j in [0, s1.Cols( ) - 8] whose
            8-mer bb has bb[m] != bb[m - 1] for some m in 1..3, bb[4 + m] != bb[4 + m - 1] for some m in 1..3, and at least 3 bases present.
  :521-565  for r in rows of s2, l in [0, s2.Cols( ) - 8] with all 8 cells Def, every entry of bbs equal to the row's 8-mer: offset = j - l
            if s == 0 else l - j; continue if ( r, offset ) in sees; continue if the offset has 10 conflicting columns or more (the table
            of scons_oracle at index offset + n2: what the lazily filled allowed / disallowed vectors hold); sees.insert.
  :571-598  offx = offset if s == 0 else -offset; pos1 = max( offx, 0 ); pos2 = max( -offx, 0 ); overlap = IntervalOverlap( 0, s1.Cols( ),
            offx, offx + s2.Cols( ) ); err_sum[v] = err_sum[v - 1] + ( con1[pos1 + v - 1] != s2.Base( r, pos2 + v - 1 ) ); minp = 0; for
            start in [0, overlap), n in [20, overlap - start]: unless Def of both end cells, continue; minp = Min( minp, gBS[n][k] ).
            bits = -minp * 10.0 / 6.0; if bits < 20.0 continue; results.push( bits, offset ).
  :634-645  ReverseSort( results ); offsets: results[0]'s, then every offset not yet a Member with results[0].first - score <= 20.0;
            Sort( offsets ).  :715: closures are made iff offsets.isize( ) <= 3 (and there is one).

gBS is tests/offsets_oracle.table(): PrecomputedBinomialSums<1000>( 20, 0.75 ) built in long double, gBS[n][n] = 0.0.  The window loop is
the text's with the n loop of a start done at once by numpy over the ends that are Def (min over the same values; Min has no order)."""
import struct

import numpy as np

from tests import offsets_oracle, scons_oracle
from tests.closer_oracle import seq_digest

MM = 8
WID = 20
MIN_BITS = 20.0
MAX_DIFF = 20.0
MAX_OFFSETS = 3
CONFLICTS = 10
SALT = 0x50FF
FILE = "a.stack.offsets"
MAGIC = b"DFKSOFF1"
KEPT, DROPPED = 0, 1
COUNTS = ("rows", "kmers", "acceptable", "hits", "seen", "disallowed", "lookups", "results")


def acceptable_kmers(con1, cols):
    """:499-517 -> {8-mer: [j...]}"""
    bbs = {}
    for j in range(0, cols - MM + 1):
        bb = tuple(int(x) for x in con1[j:j + MM])
        if not any(bb[m] != bb[m - 1] for m in range(1, MM // 2)): continue
        if not any(bb[MM // 2 + m] != bb[MM // 2 + m - 1] for m in range(1, MM // 2)): continue
        if len(set(bb)) < 3: continue
        bbs.setdefault(bb, []).append(j)
    return bbs


def bits_of(con1, row_b, row_def, cols1, cols2, offx, T, n):
    pos1, pos2 = max(offx, 0), max(-offx, 0)
    overlap = max(0, min(cols1, offx + cols2) - max(0, offx))
    err = np.concatenate([[0], np.cumsum(con1[pos1:pos1 + overlap] != row_b[pos2:pos2 + overlap])]).astype(np.int64)
    d = row_def[pos2:pos2 + overlap]
    ends = np.nonzero(d)[0]
    minp = 0.0
    for start in range(overlap):
        if not d[start]: continue
        e = ends[ends >= start + WID - 1]               # start + n - 1 for n in [WID, overlap - start] with Def
        if not len(e): continue
        v = T[e - start + 1, err[e + 1] - err[start]]
        n["lookups"] += len(e)
        minp = min(minp, float(v.min()))
    return -minp * 10.0 / 6.0


def one_pair(stacks, cons, counts, T, n):
    """stacks: two of scons_oracle.build_stack; cons: con of both sides; counts: the pair's conflict table -> (seen, records)"""
    n2 = stacks[1]["cols"]
    results = []
    seen = 0
    for s in range(2):
        s1, s2 = stacks[s], stacks[1 - s]
        con1 = np.asarray(cons[s], np.int64)
        sees = set()
        bbs = acceptable_kmers(con1, s1["cols"])
        n["acceptable"] += sum(len(v) for v in bbs.values())
        B, Q = s2["bases"], s2["quals"]
        for r in range(B.shape[0]):
            n["rows"] += 1
            row_def = Q[r] >= 0
            for l in range(0, s2["cols"] - MM + 1):
                if not row_def[l:l + MM].all(): continue
                n["kmers"] += 1
                for j in bbs.get(tuple(int(x) for x in B[r, l:l + MM]), ()):
                    n["hits"] += 1
                    offset = j - l if s == 0 else l - j
                    if (r, offset) in sees: continue
                    if counts[offset + n2] >= CONFLICTS:
                        n["disallowed"] += 1
                        continue
                    sees.add((r, offset))
                    seen += 1
                    bits = bits_of(con1, B[r], row_def, s1["cols"], s2["cols"], offset if s == 0 else -offset, T, n)
                    if bits < MIN_BITS: continue
                    results.append((bits, offset))
    n["seen"] += seen; n["results"] += len(results)
    results = sorted(results, reverse=True)
    offsets = []
    for score, offset in results:
        if not offsets: offsets.append(offset)
        elif offset in offsets: continue
        elif results[0][0] - score <= MAX_DIFF: offsets.append(offset)
    offsets.sort()
    records = []
    for o in sorted({o for _, o in results}):
        mine = [b for b, x in results if x == o]
        records.append((o, len(mine), max(mine), KEPT if o in offsets else DROPPED))
    return seen, records


def run(recs, bases_of, quals_of, scons):
    """recs: walks_oracle's records, two a pair; scons: scons_oracle.run's result for them -> dict(words, records and counters per pair, starts, file,
    digest, the counters)"""
    T = offsets_oracle.table()
    memo = {}

    def b_of(id):
        if id not in memo: memo[id] = bases_of(id)
        return memo[id]
    n = dict.fromkeys(COUNTS, 0)
    words, per, per_counts = [], [], []
    yielding = 0
    for pi in range(len(recs) // 2):
        a, b = recs[2 * pi], recs[2 * pi + 1]
        if not scons_oracle.yields(a, b):
            words.append((0, 0, 0, 0)); per.append([]); per_counts.append(dict.fromkeys(COUNTS, 0))
            continue
        yielding += 1
        stacks = [scons_oracle.build_stack(r["locs"], spass, b_of, quals_of) for spass, r in ((1, a), (2, b))]
        el = scons["elements"][2 * pi:2 * pi + 2]
        assert [st["cols"] for st in stacks] == [e["cols"] for e in el]
        mine = dict.fromkeys(COUNTS, 0)
        seen, records = one_pair(stacks, [el[0]["con"], el[1]["con"]], scons["counts"][pi], T, mine)
        per_counts.append(mine)
        for k in COUNTS: n[k] += mine[k]
        kept = sum(r[3] == KEPT for r in records)
        words.append((seen, sum(r[1] for r in records), kept, int(1 <= kept <= MAX_OFFSETS)))
        per.append(records)
    records = [r for p in per for r in p]
    starts = [0] + [int(x) for x in np.cumsum([len(p) for p in per])]
    ks = [w[2] for w in words]
    return dict(words=words, per=per, per_counts=per_counts, records=records, starts=starts, file=soffsets_file(starts, words, records), digest=digest_of(words, records), pairs=len(words), yields=yielding,
                offsets=len(records), kept=sum(r[3] == KEPT for r in records), dropped=sum(r[3] == DROPPED for r in records), pairs_0=sum(k == 0 for k in ks), pairs_1=sum(k == 1 for k in ks),
                pairs_2=sum(k == 2 for k in ks), pairs_3=sum(k == 3 for k in ks), pairs_more=sum(k > 3 for k in ks), closable=sum(w[3] for w in words), **n)


def record_bytes(records):
    return b"".join(struct.pack("<iIdII", r[0], r[1], r[2], r[3], 0) for r in records)


def soffsets_file(starts, words, records):
    return MAGIC + struct.pack("<Q", len(starts) - 1) + np.asarray(starts, "<u8").tobytes() + b"".join(struct.pack("<IIII", *w) for w in words) + record_bytes(records)


def digest_of(words, records):
    w = np.frombuffer(b"".join(struct.pack("<IIII", *x) for x in words), "<u4")
    r = np.frombuffer(record_bytes(records), "<u4")
    return seq_digest(np.concatenate([w.astype(np.uint64), r.astype(np.uint64)]), SALT)


# ---- the fixtures
_cache = {}


def fixture_soffsets(golden_dir, case, K, which):
    """run() on a fixture's walks and stack consensus; computed once per session and handed out unchanged"""
    if case not in _cache:
        from tests import walks_oracle
        i = walks_oracle.fixture_inputs(golden_dir, case, K, which)
        w = walks_oracle.fixture_walks(golden_dir, case, K, which)
        _cache[case] = run(w["recs"], i["read_bases"], i["quals_of"], scons_oracle.fixture_scons(golden_dir, case, K, which))
    return _cache[case]
