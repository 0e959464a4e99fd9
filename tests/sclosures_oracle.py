"""Stackster's closures per pair (10X/Stackster.cc:712-757; paths/long/ReadStack.cc:714-725 Trim, :355-398 Merge, :406-427 Consensus1
with qualities, :26-45 BaseMetrics) restated in plain Python, the file a.stack.closures of dfk_sclosures_write and its digest.

What is pinned on what: no reference-written form of this result exists (Stackster.cc does not compile here), so the rule is pinned by
two restatements written independently from the reference's text -- this module and superplus_amd/csrc/dfk_sclosures.h.  The INPUTS
are the two stacks of a pair as tests/scons_oracle.build_stack leaves them after Trim and Reverse (grids with ' ' = -1 and quality -1
where no read stands; a quality of 128 or more is negative in its char) and, per pair, the records of tests/soffsets_oracle.py.

The text, for a pair that reaches :712 with `offsets` = its kept offsets, ascending (:644):

  :714-716  MAX_OFFSETS = 3; if ( offsets.isize( ) <= MAX_OFFSETS ) for ( j = 0; j < offsets.isize( ); j++ ): with more than three,
            or none, nothing is pushed.
  :717-728  readstack s1( stacks[0] ), s2( stacks[1] ); o = offset; right_ext = s1.Cols( ) - offset - s2.Cols( ); if right_ext > 0:
            s1.Trim( 0, s1.Cols( ) - right_ext ); left_ext = -offset; if left_ext > 0: s2.Trim( left_ext, s2.Cols( ) ) and o = 0.
  Trim      to_remove[i] = True unless some Def( i, j ) for j in [start, stop); every row becomes its [start, stop) part; cols_ = stop -
            start; Erase( to_remove ).
  :732-733  readstack s( s1 ); s.Merge( s2, o ): ReadStack.cc:355-398 by its resize / shift / append (tests/closures_oracle.merge).
  :753      s.Consensus1( f, fragq ): per column four ( 0.0, id ); for the rows in order q = Qual; if q <= 2: q = Min( q, 0.2 ); if q == 0:
            q = 0.1; if Qual >= 0: mx.val( Base ) += q.  reverseSort: con = id(0), the greatest ( sum, id ).  fragq goes nowhere.
  :757      closures.push_back( f ).

The one undefined place: no row left in either stack makes cols_ = bases_[0].size( ) a read of an empty vector.  Decided
(dfk_sclosures.h): the closure has C = offset + n2 columns of base 3, and `rowless` counts it.

A Python float is the reference's double, and a column's sum is added to one cell at a time in row order."""
import struct

import numpy as np

from tests import closures_oracle, scons_oracle, soffsets_oracle
from tests.closer_oracle import seq_digest

SALT = 0x5C15
FILE = "a.stack.closures"
MAGIC = b"DFKSCLS1"
MAX_OFFSETS = 3
MAX_WIDTH = scons_oracle.MAX_WIDTH
UNDEF = closures_oracle.UNDEF
COUNTS = ("pairs", "yields", "closable", "none", "over", "closures", "columns", "added", "live", "erased", "empty", "short", "rowless")


def grids(st):
    """scons_oracle.build_stack's grids as lists of rows with closures_oracle's ' ' -> (bases_, quals_, cols)"""
    B = [[UNDEF if int(b) == scons_oracle.BLANK else int(b) for b in r] for r in st["bases"]]
    Q = [[int(q) for q in r] for r in st["quals"]]
    return B, Q, int(st["cols"])


def trim(bases_, quals_, start, stop):
    """readstack::Trim( start, stop ) -> (bases_, quals_, cols_)"""
    rows = len(bases_)
    to_remove = [True] * rows
    for i in range(rows):
        for j in range(start, stop):
            if quals_[i][j] >= 0:
                to_remove[i] = False
                break
        bases_[i] = bases_[i][start:stop]
        quals_[i] = quals_[i][start:stop]
    return [r for i, r in enumerate(bases_) if not to_remove[i]], [r for i, r in enumerate(quals_) if not to_remove[i]], stop - start


def closures_of_pair(st0, st1, offsets):
    """:714-757 for one pair; st0, st1: grids() of its stacks -> [dict(offset, cols, rows, bases, added, empty, sums)]"""
    out = []
    if not len(offsets) <= MAX_OFFSETS: return out
    for offset in offsets:
        B1, Q1, cols1 = [list(r) for r in st0[0]], [list(r) for r in st0[1]], st0[2]      # readstack s1( stacks[0] ), s2( stacks[1] )
        B2, Q2, cols2 = [list(r) for r in st1[0]], [list(r) for r in st1[1]], st1[2]
        C = offset + cols2
        o = offset
        right_ext = cols1 - offset - cols2
        if right_ext > 0: B1, Q1, cols1 = trim(B1, Q1, 0, cols1 - right_ext)
        left_ext = -offset
        if left_ext > 0:
            B2, Q2, cols2 = trim(B2, Q2, left_ext, cols2)
            o = 0
        bases_, quals_, forms = closures_oracle.merge(B1, Q1, cols1, B2, Q2, cols2, o)
        assert forms == (C, C), (forms, C)
        if bases_:
            cols = len(bases_[0])                                                 # cols_ = bases_[0].size( )
            assert cols == C
            con, added, empty, sums = closures_oracle.consensus1(bases_, quals_, cols)
        else:
            con, added, empty, sums = [3] * C, 0, C, [[0.0] * 4 for _ in range(C)]      # the rowless rule
        out.append(dict(offset=int(offset), cols=C, rows=len(bases_), bases=np.asarray(con, np.uint8), added=added, empty=empty, sums=sums))
    return out


def live_rows(locs, M, len_of):
    w0 = M - MAX_WIDTH if M > MAX_WIDTH else 0
    return sum(1 for id, pos, fw in locs if len_of(id) > 0 and pos + len_of(id) > w0)


def closures_file(pair_first, starts, recs, bases):
    b = np.asarray(bases, np.uint8).tobytes()
    return (MAGIC + struct.pack("<QQ", len(recs), len(pair_first) - 1) + np.asarray(pair_first, "<u8").tobytes() + np.asarray(starts, "<u8").tobytes()
            + b"".join(struct.pack("<IiII", *r) for r in recs) + b + bytes((-len(b)) % 8))


def digest_of(recs, bases):
    w = np.frombuffer(b"".join(struct.pack("<IiII", *r) for r in recs), "<u4")
    return seq_digest(np.concatenate([w.astype(np.uint64), np.asarray(bases, np.uint64)]), SALT)


def run(recs, bases_of, quals_of, K, records_per, keep_sums=False):
    """recs: walks_oracle's records, two a pair; records_per[pi]: soffsets_oracle's records of the pair ( offset, results, best_bits,
    state ) -> dict(per, pair_first, starts, records, bases, file, digest, the counters)"""
    memo = {}

    def b_of(id):
        if id not in memo: memo[id] = bases_of(id)
        return memo[id]
    per = []
    n = dict(yields=0, closable=0, none=0, over=0, live=0, erased=0)
    for pi in range(len(recs) // 2):
        a, b = recs[2 * pi], recs[2 * pi + 1]
        y = scons_oracle.yields(a, b)
        n["yields"] += y
        offsets = [int(r[0]) for r in records_per[pi] if r[3] == soffsets_oracle.KEPT]
        assert offsets == sorted(offsets) and (y or not records_per[pi])
        n["none"] += not offsets; n["over"] += len(offsets) > MAX_OFFSETS
        if not 1 <= len(offsets) <= MAX_OFFSETS:
            per.append([])
            continue
        n["closable"] += 1
        stacks = [scons_oracle.build_stack(r["locs"], spass, b_of, quals_of) for spass, r in ((1, a), (2, b))]
        cl = closures_of_pair(grids(stacks[0]), grids(stacks[1]), offsets)
        live = sum(live_rows(r["locs"], st["M"], lambda id: len(b_of(id))) for r, st in zip((a, b), stacks))
        n["live"] += len(cl) * live
        n["erased"] += sum(stacks[0]["rows_kept"] + stacks[1]["rows_kept"] - c["rows"] for c in cl)
        if not keep_sums:
            for c in cl: del c["sums"]
        per.append(cl)
    flat = [(pi, c) for pi, cl in enumerate(per) for c in cl]
    records = [(pi, c["offset"], c["cols"], c["rows"]) for pi, c in flat]
    pair_first = [0] + [int(x) for x in np.cumsum([len(cl) for cl in per])]
    starts = [0] + [int(x) for x in np.cumsum([c["cols"] for _, c in flat])]
    bases = np.concatenate([c["bases"] for _, c in flat] + [np.zeros(0, np.uint8)])
    return dict(per=per, pair_first=pair_first, starts=starts, records=records, bases=bases, file=closures_file(pair_first, starts, records, bases), digest=digest_of(records, bases),
                pairs=len(recs) // 2, closures=len(records), columns=int(starts[-1]), added=sum(c["added"] for _, c in flat), empty=sum(c["empty"] for _, c in flat),
                short=sum(c["cols"] < K for _, c in flat), rowless=sum(c["rows"] == 0 for _, c in flat), **n)


def sequences(r):
    """the closures as base arrays, per pair"""
    return [[c["bases"] for c in cl] for cl in r["per"]]


# ---- the fixtures
_cache = {}


def fixture_sclosures(golden_dir, case, K, which):
    """run() on a fixture's walks with the offsets tests/soffsets_oracle.py finds; computed once per session and handed out unchanged"""
    if case not in _cache:
        from tests import walks_oracle
        i = walks_oracle.fixture_inputs(golden_dir, case, K, which)
        w = walks_oracle.fixture_walks(golden_dir, case, K, which)
        so = soffsets_oracle.fixture_soffsets(golden_dir, case, K, which)
        _cache[case] = run(w["recs"], i["read_bases"], i["quals_of"], K, so["per"])
    return _cache[case]
