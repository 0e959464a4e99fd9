"""CloseGap2's closures per pair (10X/Closomatic.cc:651-660; paths/long/ReadStack.cc:355-398 Merge, :406-427 Consensus1 with
qualities, :26-45 BaseMetrics) restated in plain Python, the file a.close.closures of dfk_closures_write and its digest.

What is pinned on what: no reference-written form of this result exists (neither ReadStack.cc nor Closomatic.cc compiles here), so the
rule is pinned by two restatements written independently from the reference's text -- this module and
superplus_amd/csrc/dfk_closures.h.  The INPUTS are tests/cons_oracle.py's (the two stacks of a pair materialised as grids by its
stack_of / trim / reverse, exactly as it materialises them) and, per pair, the offsets GetOffsets1 returned (tests/offsets_oracle.py's
survivors).

The text, for pair pi with offsets o:

  :651      if ( o.size( ) <= 2 ) for ( j = 0; j < o.size( ); j++ ): with more than two offsets, or none, nothing is pushed.
  :653-654  readstack s( stacks[0] ); s.Merge( stacks[1], o[j] );
  Merge     rows1, rows2, cols1, cols2; left_ext1 = Max( 0, -offset ), right_ext1 = Max( 0, offset + cols2 - cols1 ).  Every row i of s:
            if left_ext1 > 0: resize to left_ext1 + cols1, shift right by left_ext1 from the back, fill the front with ' ' / -1; then
            resize by right_ext1 more, filled with ' ' / -1.  The rows of the other stack are appended.  left_ext2 = Max( 0, offset ),
            right_ext2 = Max( 0, cols1 - ( offset + cols2 ) ): the same for the appended rows.  cols_ = bases_[0].size( ).
  :657      s.Consensus1( f, fragq ): per column i, BaseMetrics<double> mx (four (0.0, id) pairs); for the rows j in order:
            q = Qual(j,i); if q <= 2: q = Min( q, 0.2 ); if q == 0: q = 0.1; if Qual(j,i) >= 0: mx.val( Base(j,i) ) += q.  Then
            mx.reverseSort( ) -- std::sort with std::greater< pair<double,int> > -- and con[i] = mx.id(0): the greatest (sum, id).
            conq and the max_qcomp block go nowhere (:660 pushes f alone).
  :660      closures.push_back(f).

The one undefined place: rows1 + rows2 == 0 makes bases_[0] a read of an empty vector.  Decided (dfk_closures.h): the closure has
C = max(cols1, offset + cols2) - min(0, offset) columns of base 3, and `rowless` counts it.

A Python float is the reference's double, and a column's sum is added to one cell at a time in row order."""
import struct

import numpy as np

from tests import closer_oracle, cons_oracle, partners_oracle
from tests.closer_oracle import seq_digest

SALT = 0xF1F1
FILE = "a.close.closures"
MAGIC = b"DFKCCLS1"
UNDEF = cons_oracle.UNDEF
MAX_WIDTH = cons_oracle.MAX_WIDTH


def stack_grids(rows, ne, reversed_, bases_of, quals_of):
    """stacks[ei] as :639 stores it: tests/cons_oracle.py's grid after Trim and Reverse -> (B, Q as lists of rows, cols, live rows)"""
    B, Q, M = cons_oracle.stack_of(rows, ne, bases_of, quals_of)
    w0 = M - MAX_WIDTH if M > MAX_WIDTH else 0
    live = 0
    for id, pos, fw in rows:
        n = len(bases_of(id))
        live += n > 0 and (pos + n if fw else ne - pos) > w0
    if M > MAX_WIDTH: B, Q = cons_oracle.trim(B, Q, w0, M)
    if reversed_: B, Q = cons_oracle.reverse(B, Q)
    return [[int(x) for x in r] for r in B], [[int(x) for x in r] for r in Q], int(B.shape[1]), int(live)


def merge(B1, Q1, cols1, B2, Q2, cols2, offset):
    """readstack::Merge, by its resize / shift / append -> (bases_, quals_, the two forms of the width)"""
    bases_, quals_ = [list(r) for r in B1], [list(r) for r in Q1]                 # readstack s( stacks[0] )
    rows1, rows2 = len(B1), len(B2)
    left_ext1 = max(0, -offset)
    right_ext1 = max(0, offset + cols2 - cols1)
    for i in range(rows1):
        if left_ext1 > 0:
            bases_[i] += [None] * left_ext1; quals_[i] += [None] * left_ext1       # resize( left_ext1 + cols1 )
            for j in range(left_ext1 + cols1 - 1, left_ext1 - 1, -1):
                bases_[i][j] = bases_[i][j - left_ext1]; quals_[i][j] = quals_[i][j - left_ext1]
            for j in range(left_ext1):
                bases_[i][j] = UNDEF; quals_[i][j] = -1
        bases_[i] += [UNDEF] * right_ext1; quals_[i] += [-1] * right_ext1
    bases_ += [list(r) for r in B2]; quals_ += [list(r) for r in Q2]
    left_ext2 = max(0, offset)
    right_ext2 = max(0, cols1 - (offset + cols2))
    for i in range(rows2):
        ip = rows1 + i
        if left_ext2 > 0:
            bases_[ip] += [None] * left_ext2; quals_[ip] += [None] * left_ext2
            for j in range(left_ext2 + cols2 - 1, left_ext2 - 1, -1):
                bases_[ip][j] = bases_[ip][j - left_ext2]; quals_[ip][j] = quals_[ip][j - left_ext2]
            for j in range(left_ext2):
                bases_[ip][j] = UNDEF; quals_[ip][j] = -1
        bases_[ip] += [UNDEF] * right_ext2; quals_[ip] += [-1] * right_ext2
    return bases_, quals_, (left_ext1 + cols1 + right_ext1, left_ext2 + cols2 + right_ext2)


def consensus1(bases_, quals_, cols):
    """readstack::Consensus1( con, conq ), con alone -> (bases, defined cells added, columns nothing was added to, the sums)"""
    sums = [[0.0, 0.0, 0.0, 0.0] for _ in range(cols)]
    added = 0
    for brow, qrow in zip(bases_, quals_):                                        # (row after row: every column's additions in row order)
        assert len(brow) == len(qrow) == cols
        for i, qual in enumerate(qrow):
            if qual < 0: continue
            q = float(qual)
            if q <= 2: q = min(q, 0.2)
            if q == 0: q = 0.1
            sums[i][brow[i]] += q
            added += 1
    con = [sorted(((s[b], b) for b in range(4)), reverse=True)[0][1] for s in sums]     # mx.reverseSort( ); mx.id(0)
    return con, added, sum(1 for s in sums if max(s) == 0.0), sums


def closures_of_pair(st0, st1, offsets):
    """:651-660 for one pair -> [dict(offset, cols, rows, bases, added, empty, forms, sums)]"""
    out = []
    if not 1 <= len(offsets) <= 2: return out
    (B1, Q1, cols1, _), (B2, Q2, cols2, _) = st0, st1
    for off in offsets:
        assert -cols2 <= off <= cols1, (off, cols1, cols2)
        bases_, quals_, forms = merge(B1, Q1, cols1, B2, Q2, cols2, off)
        C = max(cols1, off + cols2) - min(0, off)
        assert forms == (C, C)
        if bases_:
            cols = len(bases_[0])                                                 # cols_ = bases_[0].size( )
            assert cols == C
            con, added, empty, sums = consensus1(bases_, quals_, cols)
        else:
            con, added, empty, sums = [3] * C, 0, C, [[0.0] * 4 for _ in range(C)]      # the rowless rule
        out.append(dict(offset=int(off), cols=C, rows=len(bases_), bases=np.asarray(con, np.uint8), added=added, empty=empty, forms=forms, sums=sums))
    return out


def closures_file(pair_first, starts, recs, bases):
    b = np.asarray(bases, np.uint8).tobytes()
    return (MAGIC + struct.pack("<QQ", len(recs), len(pair_first) - 1) + np.asarray(pair_first, "<u8").tobytes() + np.asarray(starts, "<u8").tobytes()
            + b"".join(struct.pack("<IiII", *r) for r in recs) + b + bytes((-len(b)) % 8))


def digest_of(recs, bases):
    w = np.frombuffer(b"".join(struct.pack("<IiII", *r) for r in recs), "<u4")
    return seq_digest(np.concatenate([w.astype(np.uint64), np.asarray(bases, np.uint64)]), SALT)


def run(inv, kmers, K, ce, locs_per, partner_elements, pairs, offsets_per, bases_of, quals_of, keep_sums=False):
    """cons_oracle.run's inputs and offsets_per[pi] = the offsets of pair pi -> dict(per, pair_first, starts, records, bases, file,
    digest, the counters)"""
    rank = {int(e): k for k, e in enumerate(ce)}
    per, live = [], 0
    for pi, (e1, e2) in enumerate(pairs):
        offs = [int(o) for o in offsets_per[pi]]
        if not 1 <= len(offs) <= 2:
            per.append([])
            continue
        es = [int(e1), int(inv[e2])]
        st = []
        for ei in (0, 1):
            e = es[ei]
            rows = list(locs_per[rank[e]]) + list(partner_elements[2 * pi + (1 - ei)])
            st.append(stack_grids(rows, kmers[e] + K - 1, e == int(inv[e2]), bases_of, quals_of))
        cl = closures_of_pair(st[0], st[1], offs)
        live += len(cl) * (st[0][3] + st[1][3])
        if not keep_sums:
            for c in cl: del c["sums"]
        per.append(cl)
    flat = [(pi, c) for pi, cl in enumerate(per) for c in cl]
    recs = [(pi, c["offset"], c["cols"], c["rows"]) for pi, c in flat]
    pair_first = [0] + [int(x) for x in np.cumsum([len(cl) for cl in per])]
    starts = [0] + [int(x) for x in np.cumsum([c["cols"] for _, c in flat])]
    bases = np.concatenate([c["bases"] for _, c in flat] + [np.zeros(0, np.uint8)])
    n_off = [len(o) for o in offsets_per]
    return dict(per=per, pair_first=pair_first, starts=starts, records=recs, bases=bases, file=closures_file(pair_first, starts, recs, bases), digest=digest_of(recs, bases),
                pairs=len(pairs), closable=sum(1 <= n <= 2 for n in n_off), over=sum(n > 2 for n in n_off), closures=len(recs), columns=int(starts[-1]),
                added=sum(c["added"] for _, c in flat), live=live, empty=sum(c["empty"] for _, c in flat), short=sum(c["cols"] < K for _, c in flat),
                rowless=sum(c["rows"] == 0 for _, c in flat))


def off_arrays(offsets_per):
    """the offsets as dfk_closures_build_arrays takes them"""
    first = np.zeros(len(offsets_per) + 1, np.uint64)
    first[1:] = np.cumsum([len(o) for o in offsets_per], dtype=np.uint64)
    return first, np.asarray([int(x) for o in offsets_per for x in o], np.int32)


# ---- the fixtures
_cache = {}


def fixture_closures(golden_dir, case, K, which):
    """run() on a fixture with the offsets tests/offsets_oracle.py finds; computed once per session and handed out unchanged"""
    if case not in _cache:
        from tests import offsets_oracle
        i = partners_oracle.fixture_inputs(golden_dir, case, K, which)
        p = partners_oracle.fixture_partners(golden_dir, case, K, which)
        kmers = closer_oracle.fixture_inputs(golden_dir, case, K, which)["kmers"]
        offsets_per = [g["survivors"] for g in offsets_oracle.fixture_offsets(golden_dir, case, K, which)["per"]]
        memo = {}

        def bases_of(id):
            if id not in memo: memo[id] = i["read_bases"](id)
            return memo[id]
        _cache[case] = dict(run(i["inv"], kmers, K, i["ce"], i["locs_per"], p["elements"], i["pairs"], offsets_per, bases_of, cons_oracle.fixture_quals(i["rs"])), offsets_per=offsets_per)
    return _cache[case]
