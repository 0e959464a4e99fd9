"""Stackster's stack consensus per pair (10X/Stackster.cc:396-489: the two stacks, Trim, Reverse, Consensus1( con, conq, QUALCAP ), the
MIN_FLAT zeroing; :546-563: the conflicting columns of an offset) restated in plain Python per pair, the file a.stack.cons of
dfk_scons_write and its digest.

What is pinned on what: no reference-written form of this result exists (Stackster.cc does not compile here), so the rule is pinned by
two restatements written independently from the reference's text -- this module and superplus_amd/csrc/dfk_scons.h.  The INPUTS are the
walks of tests/walks_oracle.py (per pair and side the locs of :403, M, trim), the reads and their PQVec qualities.

The text, for a pair, ALT = False, EXP = False:

  which     :404-408.  locs empty on a side: Stackster returns.  Only a pair with status 0 and placed > 0 on both sides reaches :461;
            every other pair has two elements of 0 rows, 0 columns and no conflict entries.
  the stack :409-431.  M = Max over locs of pos + len.  stack.Initialize( rows, M ): every cell ' ' / -1.  Row i: b, q = basesy / qualsy of
            the entry -- the read lowered (:348-360) as stored, then reverse-complemented iff the loc's flag is false (:425 SetRc2( i,
            !fw ); walks_oracle.one_pair) -- base b[j], qual q[j] at p = pos + j where 0 <= p < M.  The quality lands in a char: 128 and
            more are negative there, and Def( i, p ) is Qual >= 0.
  Trim      :435-440, ReadStack.cc:714-725.  M > 400: the columns [M - 400, M) kept; the rows with no Def cell among them erased.
  Reverse   :446 spass 2 only; ReadStack.cc:346-353: bases_[i] reversed, every base that is not ' ' replaced by 3 - base, quals_[i] reversed.
  Consensus1  ReadStack.cc:406-427 with qualcap 100.  Per column mx = four ( 0.0, id ); for the rows in order: q = Qual; if q <= 2: q =
            Min( q, 0.2 ); if q == 0: q = 0.1; if Qual >= 0: mx.val( Base ) += q.  reverseSort: descending ( value, id ).  con = id(0);
            conq = Min( 100, int( round( val(0) - val(1) ) ) ); if val(1) > 100: badcount = rows with Qual >= 30 and Base == id(1); two or
            more: conq = 0.
  MIN_FLAT  :473-489 on each side's con: for i: j = the end of the run of con[i]; if j - i >= 10: conq[i:j] = 0; i = j.
  conflicts :546-563.  n1, n2 = the columns of the stacks.  For an offset: the i1 in [0, n1) with i2 = i1 - offset in [0, n2), conq1x[i1]
            == 100, conq2x[i2] == 100 and con1x[i1] != con2x[i2].  The reference asks for the offsets in [-n2, n1) that an 8-mer proposes
            and keeps the answer per offset; the table holds every offset, at index offset + n2.  Fewer than 10: allowed.

The sums are Python floats added a cell at a time in row order; the sort is sorted(..., reverse=True) on ( sum, id ); the rounding is C's
round (half away from zero) through decimal's ROUND_HALF_UP on the exact value, not Python's round()."""
import struct
from decimal import ROUND_HALF_UP, Decimal

import numpy as np

from tests import walks_oracle
from tests.closer_oracle import seq_digest

QUALCAP = 100
MAX_QCOMP = 100
MIN_FLAT = 10
CONFLICTS = 10
MAX_WIDTH = 400
SALT = 0x5C05
FILE = "a.stack.cons"
MAGIC = b"DFKSCON1"
BLANK = -1                                          # ' '


def c_round(x):
    """C's round( double ) -> int"""
    return int(Decimal(x).quantize(Decimal(1), rounding=ROUND_HALF_UP))


def as_char(q):
    return int(q) - 256 if int(q) >= 128 else int(q)


def yields(a, b):
    return a["status"] == walks_oracle.WALKED and b["status"] == walks_oracle.WALKED and a["placed"] > 0 and b["placed"] > 0


def build_stack(locs, spass, bases_of, quals_of):
    """:409-446 -> dict(bases, quals: the grids as they stand after Trim and Reverse, rows, rows_kept, M, cols)"""
    rows = []
    for id, pos, fw in locs:
        b = np.asarray(bases_of(id), np.int64)
        q = walks_oracle.lower(b, quals_of(id))
        if not fw: b, q = walks_oracle.revcomp(b, q)
        rows.append((int(pos), b, q))
    M = 0
    for pos, b, q in rows: M = max(M, pos + len(b))
    bases = np.full((len(rows), M), BLANK, np.int64)
    quals = np.full((len(rows), M), -1, np.int64)
    for i, (pos, b, q) in enumerate(rows):
        for j in range(len(b)):
            p = pos + j
            if 0 <= p < M:
                bases[i, p] = b[j]; quals[i, p] = as_char(q[j])
    n_rows, cols = len(rows), M
    if cols > MAX_WIDTH:
        start, stop = cols - MAX_WIDTH, cols
        keep = [i for i in range(len(rows)) if (quals[i, start:stop] >= 0).any()]
        bases, quals = bases[keep, start:stop], quals[keep, start:stop]
        cols = stop - start
    if spass == 2:
        bases = bases[:, ::-1].copy(); quals = quals[:, ::-1].copy()
        bases[bases != BLANK] = 3 - bases[bases != BLANK]
    return dict(bases=bases, quals=quals, rows=n_rows, rows_kept=bases.shape[0], M=M, cols=cols)


def consensus1(st, qualcap=QUALCAP):
    """ReadStack.cc:406-427 -> con, conq, (cells, capped, recount)"""
    bases, quals = st["bases"], st["quals"]
    sums = [[0.0, 0.0, 0.0, 0.0] for _ in range(st["cols"])]
    cells = 0
    for j in range(bases.shape[0]):                # the rows in order; within a row every column has a sum of its own
        for i in np.nonzero(quals[j] >= 0)[0]:
            q = float(quals[j, i])
            if q <= 2: q = min(q, 0.2)
            if q == 0: q = 0.1
            sums[i][int(bases[j, i])] += q
            cells += 1
    con, conq = [], []
    capped = recount = 0
    for i in range(st["cols"]):
        mx = sorted(((sums[i][b], b) for b in range(4)), reverse=True)
        con.append(mx[0][1])
        r = c_round(mx[0][0] - mx[1][0])
        capped += r >= qualcap
        cq = min(qualcap, r)
        if mx[1][0] > MAX_QCOMP:
            badcount = int(((quals[:, i] >= 30) & (bases[:, i] == mx[1][1])).sum())
            if badcount >= 2:
                cq = 0; recount += 1
        conq.append(cq)
    return con, conq, (cells, capped, recount)


def min_flat(con, conq):
    """:473-489 -> the columns zeroed"""
    n = 0
    i = 0
    while i < len(con):
        j = i + 1
        while j < len(con):
            if con[j] != con[i]: break
            j += 1
        if j - i >= MIN_FLAT:
            for k in range(i, j): conq[k] = 0
            n += j - i
        i = j
    return n


def conflicts(con1x, conq1x, con2x, conq2x, offset):
    n = 0
    for i1 in range(len(con1x)):
        i2 = i1 - offset
        if i2 < 0 or i2 >= len(con2x): continue
        if conq1x[i1] == QUALCAP and conq2x[i2] == QUALCAP and con1x[i1] != con2x[i2]: n += 1
    return n


def conflict_table(con1x, conq1x, con2x, conq2x):
    """conflicts() for every offset in [-n2, n1), by numpy (the same count)"""
    c1, q1, c2, q2 = (np.asarray(x, np.int64) for x in (con1x, conq1x, con2x, conq2x))
    n1, n2 = len(c1), len(c2)
    out = []
    for offset in range(-n2, n1):
        lo, hi = max(0, offset), min(n1, offset + n2)
        a, b = slice(lo, hi), slice(lo - offset, hi - offset)
        out.append(int(((q1[a] == QUALCAP) & (q2[b] == QUALCAP) & (c1[a] != c2[b])).sum()))
    return out


def run(recs, bases_of, quals_of):
    """recs: walks_oracle's records, two a pair -> dict(elements: two a pair, counts per pair, file, digest, the counters)"""
    memo = {}

    def b_of(id):
        if id not in memo: memo[id] = bases_of(id)
        return memo[id]
    el, per_pair = [], []
    tot = dict(cells=0, capped=0, recount=0, flat=0, allowed=0, disallowed=0, trimmed=0, yields=0)
    for pi in range(len(recs) // 2):
        a, b = recs[2 * pi], recs[2 * pi + 1]
        if not yields(a, b):
            el += [dict(rows=0, rows_kept=0, M=0, cols=0, con=[], conq=[])] * 2
            per_pair.append([])
            continue
        tot["yields"] += 1
        sides = []
        for spass, r in ((1, a), (2, b)):
            st = build_stack(r["locs"], spass, b_of, quals_of)
            assert st["M"] == r["M"] and (st["M"] - st["cols"]) == r["trim"]
            con, conq, (cells, capped, recount) = consensus1(st)
            tot["cells"] += cells; tot["capped"] += capped; tot["recount"] += recount; tot["trimmed"] += st["M"] > MAX_WIDTH
            tot["flat"] += min_flat(con, conq)
            sides.append(dict(rows=st["rows"], rows_kept=st["rows_kept"], M=st["M"], cols=st["cols"], con=con, conq=conq))
        el += sides
        t = conflict_table(sides[0]["con"], sides[0]["conq"], sides[1]["con"], sides[1]["conq"])
        n1, n2 = sides[0]["cols"], sides[1]["cols"]
        for offset in (-n2, -1, 0, n1 - 1):         # the numpy count is the text's count
            assert t[offset + n2] == conflicts(sides[0]["con"], sides[0]["conq"], sides[1]["con"], sides[1]["conq"], offset)
        tot["allowed"] += sum(1 for x in t if x < CONFLICTS); tot["disallowed"] += sum(1 for x in t if x >= CONFLICTS)
        per_pair.append(t)
    return dict(elements=el, counts=per_pair, file=scons_file(el, per_pair), digest=digest_of(el, per_pair), pairs=len(recs) // 2, stacks=2 * tot["yields"],
                rows=sum(e["rows"] for e in el), rows_kept=sum(e["rows_kept"] for e in el), columns=sum(e["cols"] for e in el), **tot)


def dim_words(e):
    return [e["rows"], e["rows_kept"], e["M"] % 2**32, e["cols"]]


def scons_file(el, per_pair):
    n = len(el)
    starts = np.concatenate([[0], np.cumsum([e["cols"] for e in el])]).astype("<u8")
    cfirst = np.concatenate([[0], np.cumsum([len(t) for t in per_pair])]).astype("<u8")
    body = (np.asarray([c for e in el for c in e["con"]], np.uint8).tobytes() + np.asarray([c for e in el for c in e["conq"]], np.uint8).tobytes() +
            np.asarray([x for t in per_pair for x in t], "<u2").tobytes())
    return MAGIC + struct.pack("<Q", n) + starts.tobytes() + cfirst.tobytes() + np.asarray([w for e in el for w in dim_words(e)], "<u4").tobytes() + body + bytes((-len(body)) % 8)


def digest_of(el, per_pair):
    words = [np.asarray([w for e in el for w in dim_words(e)], np.uint64), np.asarray([c for e in el for c in e["con"]], np.uint64),
             np.asarray([c for e in el for c in e["conq"]], np.uint64), np.asarray([x for t in per_pair for x in t], np.uint64)]
    return seq_digest(np.concatenate(words), SALT)


# ---- the fixtures
_cache = {}


def fixture_scons(golden_dir, case, K, which):
    """run() on a fixture's walks; computed once per session and handed out unchanged"""
    if case not in _cache:
        i = walks_oracle.fixture_inputs(golden_dir, case, K, which)
        w = walks_oracle.fixture_walks(golden_dir, case, K, which)
        _cache[case] = run(w["recs"], i["read_bases"], i["quals_of"])
    return _cache[case]
