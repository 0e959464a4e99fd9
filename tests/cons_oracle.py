"""CloseGap2's read stacks and their column consensus (10X/Closomatic.cc:587-640, paths/long/ReadStack.cc:346-353, 400-404, 714-725,
1841-1861) restated in plain Python per pair and side, the file a.close.cons of dfk_cons_write and its digest.

What is pinned on what: no reference-written form of this result exists (neither ReadStack.cc nor Closomatic.cc compiles here), so the
rule is pinned by two restatements written independently from the reference's text -- this module and superplus_amd/csrc/dfk_cons.h.
The INPUTS are tests/partners_oracle.py's inputs and results (locs per closer edge, the records each side's loop pushed), the reads and
their PQVec qualities as the fixtures hold them (decoded by oracle.pyoracle.pq_decode), kmers per edge.

The text, for pair pi = (e1, e2), es = [e1, inv[e2]], side ei, e = es[ei], ne = hb.Bases(e) = kmers[e] + K - 1, max_width = 400
(10X/DF.cc:590):

  rows      :599-612.  locs[ei]: the closer's locs(e), then what the loop for 1 - ei of :562-585 pushed onto locs[ei].
  M         :598-604.  M = 0; a forward row: M = Max( M, pos + len(id) ); any other: M = Max( M, ne - pos ).
  the stack :605.  readstack( rows, M ): every base ' ', every quality -1 (ReadStack.h:56-63: undefined).
  cells     :606-629.  forward: for j: p = pos + j; if p >= 0: base(i, p) = b[j], qual(i, p) = q[j].  other: for j: p = pos + j; if
            ne - p - 1 >= 0: base(i, ne - p - 1) = 3 - b[j], qual(i, ne - p - 1) = q[j].  q = quals[id].unpack: the whole read.  The
            quality is stored in a char (ReadStack.h:29,120): 128 and more become negative, and Def( ) is qual >= 0 (ReadStack.h:103).
  Trim      :633-634, ReadStack.cc:714-725.  only if Cols( ) > 400: start = Cols( ) - 400, stop = Cols( ); a row with no Def cell in
            [start, stop) is erased, the others keep their order; the columns [start, stop) are kept.
  Reverse   :638, ReadStack.cc:346-353.  if e == inv[e2]: every row reversed; every base that is not ' ' becomes 3 - base; the
            qualities reversed.
  consensus ReadStack.cc:1219-1223 (GetOffsets1 takes Consensus1 of both stacks), :400-404, :1841-1861.  per column: sum[4] doubles from
            0; for the rows in order: q = qual; q < 0: skip; val = .1 for 0, .2 for 1 and 2, q otherwise; sum[base] += val; the result
            std::max_element( sum, sum + 4 ) - sum: the FIRST maximum, base 0 where nothing was added.

A Python float is the reference's double, and the rows are added one at a time in their order: numpy adds a whole row's cells to the
column sums at once, each column's additions still one after the other in row order."""
import os
import struct

import numpy as np

from tests import closer_oracle, partners_oracle
from tests.closer_oracle import seq_digest

MAX_WIDTH = 400
SALT = 0xEEEE
FILE = "a.close.cons"
MAGIC = b"DFKCCON1"
UNDEF = 32                                        # ' '


def as_char(q):
    """a quality as the stack's char holds it"""
    q = np.asarray(q, np.int64)
    return np.where(q >= 128, q - 256, q).astype(np.int64)


def stack_of(rows, ne, bases_of, quals_of):
    """:598-629 -> (base grid, quality grid, M): rows x M, ' ' and -1 where nothing was set"""
    M = 0
    for id, pos, fw in rows:
        M = max(M, pos + len(bases_of(id))) if fw else max(M, ne - pos)
    B = np.full((len(rows), M), UNDEF, np.int64)
    Q = np.full((len(rows), M), -1, np.int64)
    for i, (id, pos, fw) in enumerate(rows):
        b, q = np.asarray(bases_of(id), np.int64), as_char(quals_of(id))
        assert len(b) == len(q)
        p = pos + np.arange(len(b), dtype=np.int64)              # (all j at once: no two j share a column)
        if fw:
            ok = p >= 0
            B[i, p[ok]] = b[ok]; Q[i, p[ok]] = q[ok]
        else:
            ok = ne - p - 1 >= 0
            B[i, (ne - p - 1)[ok]] = 3 - b[ok]; Q[i, (ne - p - 1)[ok]] = q[ok]
    return B, Q, M


def trim(B, Q, start, stop):
    """ReadStack.cc:714-725"""
    keep = [i for i in range(B.shape[0]) if (Q[i, start:stop] >= 0).any()]
    return B[keep, start:stop], Q[keep, start:stop]


def reverse(B, Q):
    """ReadStack.cc:346-353"""
    B = B[:, ::-1].copy()
    B[B != UNDEF] = 3 - B[B != UNDEF]
    return B, Q[:, ::-1].copy()


def consensus(B, Q):
    """ReadStack.cc:400-404, 1841-1861 -> (one base a column, defined cells added)"""
    cols = B.shape[1]
    sums = np.zeros((4, cols), np.float64)
    at = np.arange(cols)
    added = 0
    for i in range(B.shape[0]):
        d = Q[i] >= 0
        if not d.any(): continue
        q = Q[i, d]
        val = np.where(q == 0, .1, np.where(q <= 2, .2, q.astype(np.float64)))
        sums[B[i, d], at[d]] += val               # (a row has one cell a column: no place is added to twice here)
        added += int(d.sum())
    return np.argmax(sums, axis=0).astype(np.uint8), added, sums       # argmax: the first maximum


def one_stack(rows, ne, reversed_, bases_of, quals_of):
    """one pair and side -> dict(rows, rows_kept, M, cols, bases, ...)"""
    B, Q, M = stack_of(rows, ne, bases_of, quals_of)
    n_rows = len(rows)
    trimmed = M > MAX_WIDTH
    w0 = M - MAX_WIDTH if trimmed else 0
    # (the rows whose span meets the kept columns: what the device walks)
    live = 0
    for id, pos, fw in rows:
        n = len(bases_of(id))
        hi = pos + n if fw else ne - pos
        live += n > 0 and hi > w0
    if trimmed: B, Q = trim(B, Q, w0, M)
    if reversed_: B, Q = reverse(B, Q)
    con, added, sums = consensus(B, Q)
    top = np.sort(sums, axis=0)
    return dict(rows=n_rows, rows_kept=B.shape[0], M=M, cols=B.shape[1], bases=con, trimmed=trimmed, added=added, live=live,
                tied=int(((top[3] == top[2]) & (top[3] > 0)).sum()), empty=int((top[3] == 0).sum()), sums=sums)


def cons_file(starts, dims, bases):
    b = np.asarray(bases, np.uint8).tobytes()
    return (MAGIC + struct.pack("<Q", len(starts) - 1) + np.asarray(starts, "<u8").tobytes() + b"".join(struct.pack("<IIiI", *d) for d in dims)
            + b + bytes((-len(b)) % 8))


def dims_words(dims):
    return np.asarray([x % 2**32 for d in dims for x in d], np.uint32)


def digest_of(dims, bases):
    return seq_digest(np.concatenate([dims_words(dims).astype(np.uint64), np.asarray(bases, np.uint64)]), SALT)


def run(inv, kmers, K, ce, locs_per, partner_elements, pairs, bases_of, quals_of, keep_sums=False):
    """inv and kmers per edge; ce ascending, locs_per the records per rank; partner_elements[2 pi + ei] what the loop for ei of pair
    pi pushed onto locs[1 - ei]; pairs [(e1, e2)] -> dict(stacks, starts, dims, bases, file, counters, digest)"""
    rank = {int(e): k for k, e in enumerate(ce)}
    stacks = []
    for pi, (e1, e2) in enumerate(pairs):
        es = [int(e1), int(inv[e2])]
        for ei in (0, 1):
            e = es[ei]
            rows = list(locs_per[rank[e]]) + list(partner_elements[2 * pi + (1 - ei)])
            s = one_stack(rows, kmers[e] + K - 1, e == int(inv[e2]), bases_of, quals_of)
            s["reversed"] = e == int(inv[e2])
            s["partner_rows"] = len(partner_elements[2 * pi + (1 - ei)])
            s["ids"] = {id for id, pos, fw in rows}
            if not keep_sums: del s["sums"]
            stacks.append(s)
    dims = [(s["rows"], s["rows_kept"], s["M"], s["cols"]) for s in stacks]
    starts = [0] + [int(x) for x in np.cumsum([s["cols"] for s in stacks])]
    bases = np.concatenate([s["bases"] for s in stacks] + [np.zeros(0, np.uint8)])
    total = lambda k: sum(int(s[k]) for s in stacks)
    return dict(stacks=stacks, starts=starts, dims=dims, bases=bases, file=cons_file(starts, dims, bases), digest=digest_of(dims, bases),
                pairs=len(pairs), n_stacks=len(stacks), rows=total("rows"), live=total("live"), rows_kept=total("rows_kept"), trimmed=total("trimmed"),
                reversed=total("reversed"), columns=total("cols"), added=total("added"), partner_rows=total("partner_rows"),
                side0_reversed=sum(int(s["reversed"]) for s in stacks[0::2]), tied=total("tied"), empty=total("empty"),
                lost_rows=sum(1 for s in stacks if s["rows_kept"] < s["rows"]))


# ---- the fixtures
_cache = {}


def fixture_quals(rs):
    from oracle import pyoracle
    memo = {}

    def quals_of(id):
        if id not in memo: memo[id] = pyoracle.pq_decode(rs["pq_bytes"][int(rs["pq_off"][id]):int(rs["pq_off"][id + 1])])
        return memo[id]
    return quals_of


def fixture_cons(golden_dir, case, K, which):
    """run() on a fixture; computed once per session and handed out unchanged"""
    if case not in _cache:
        i = partners_oracle.fixture_inputs(golden_dir, case, K, which)
        p = partners_oracle.fixture_partners(golden_dir, case, K, which)
        kmers = closer_oracle.fixture_inputs(golden_dir, case, K, which)["kmers"]
        memo = {}

        def bases_of(id):
            if id not in memo: memo[id] = i["read_bases"](id)
            return memo[id]
        _cache[case] = run(i["inv"], kmers, K, i["ce"], i["locs_per"], p["elements"], i["pairs"], bases_of, fixture_quals(i["rs"]))
    return _cache[case]
