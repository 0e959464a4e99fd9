"""Stackster's two stack walks per pair (10X/Stackster.cc:207-262 StackWalk, :326-414 the loading, lowering, orientation and the locs of
each side) restated in plain Python per pair, the file a.stack.walks of dfk_walks_write and its digest.

What is pinned on what: no reference-written form of this result exists (Stackster.cc does not compile here), so the rule is pinned by
two restatements written independently from the reference's text -- this module and superplus_amd/csrc/dfk_walks.h.  The INPUTS are
tests/closer_oracle.py's read sets per closer edge, the edges' bases from the fixture's reference-written a.fastb, the reads and their
PQVec qualities as the fixtures hold them.

The text, for a pair (e1, e2), ALT = False, idsfw2 empty:

  the set   :295-324.  idsfw: closer_oracle.compose(reads(e1), reads(inv[e2])): sorted distinct (id, fw); a read may stand twice.
  loading   :329-344.  entry i: bases[id], quals[id].unpack: the whole read, a byte a quality, unsigned.
  lowering  :348-360.  for j: k = the end of the run of b[j] from j; if k - j >= 20: q[l] = Min(q[l], 5) for l in [j, k); j = k.
  sides     :368-371: an entry with fw false is reverse-complemented, its qualities reversed.  :375-386: spass 1 walks edges[0] = O(e1)
            over these; spass 2 reverse-complements every entry once more and walks edges[1] = O(e2) reverse-complemented = O(inv[e2]).
  the walk  :207-262, K = 48.  kmers_plus: (48-mer, entry, pos) of every forward 48-mer of every entry, sorted (MakeKmerLookup0).
            EE = E[0:48].  Forever: x = the last 48 bases of EE; [low, high) its lower and upper bound; duplicate if two neighbours there
            share the entry; if not duplicate: every entry there not yet placed is placed, start = |EE| - 48 - pos.  qsum[4] ints from 0:
            for every placed entry: pos = |EE| - start; if pos >= len: skip; qsum[b[pos]] += q[pos].  ReverseSortSync; return if
            qsum[0] < 60 or double(qsum[0]) < 2.0 * double(qsum[1]); else EE.push_back(ids[0]).
  locs      :398-408.  for the placed entries in order: (ids[i], start[i], idsfw[i].second ^ spass == 2); none: Stackster returns --
            after side 0, side 1 is never walked.
  M, trim   :409-414, :436-438.  M = 0; M = Max(M, pos + len); trim = M - 400 where M > 400.

An edge of fewer than 48 bases (K < 48 only) cannot start a walk (EE.SetToSubOf(E, 0, 48) is undefined there): the side is not walked
and marked SHORT.  Status: 0 walked, 1 not walked because side 0 placed nobody (or was short), 2 short edge."""
import struct

import numpy as np

from tests import closer_oracle
from tests.closer_oracle import seq_digest

KW = 48
MIN_WIN = 60
HSTAR = 5
HRUN = 20
MAX_WIDTH = 400
SALT = 0xABAB
FILE = "a.stack.walks"
MAGIC = b"DFKSWLK1"
WALKED, NOT_WALKED, SHORT = 0, 1, 2
_W16 = (np.uint64(4) ** np.arange(15, -1, -1, dtype=np.uint64))
_W32 = (np.uint64(4) ** np.arange(31, -1, -1, dtype=np.uint64))


def lower(b, q):
    """:348-360 -> the lowered qualities (a copy)"""
    q = [int(x) for x in q]
    j = 0
    while j < len(q):
        k = j + 1
        while k < len(q):
            if b[k] != b[j]: break
            k += 1
        if k - j >= HRUN:
            for l in range(j, k): q[l] = min(q[l], HSTAR)
        j = k
    return np.asarray(q, np.int64)


def revcomp(b, q):
    return (3 - np.asarray(b, np.int64))[::-1].copy(), np.asarray(q, np.int64)[::-1].copy()


def lookup_table(bases):
    """MakeKmerLookup0 -> (hi, lo, entry, pos) sorted by (48-mer, entry, pos); the 48-mer as two integers, its first 16 bases and its last 32"""
    hi, lo, ent, pos = [], [], [], []
    for i, b in enumerate(bases):
        if len(b) < KW: continue
        w = np.lib.stride_tricks.sliding_window_view(np.asarray(b, np.uint64), KW)
        hi.append(w[:, :16] @ _W16); lo.append(w[:, 16:] @ _W32)
        ent.append(np.full(len(w), i, np.int64)); pos.append(np.arange(len(w), dtype=np.int64))
    if not hi: return (np.zeros(0, np.uint64),) * 2 + (np.zeros(0, np.int64),) * 2
    hi, lo, ent, pos = (np.concatenate(x) for x in (hi, lo, ent, pos))
    o = np.lexsort((pos, ent, lo, hi))
    return hi[o], lo[o], ent[o], pos[o]


def bounds(table, x):
    """LowerBound1, UpperBound1 of the 48-mer x (a list of 48 codes)"""
    hi, lo = table[0], table[1]
    xh = np.uint64(sum(int(c) << (2 * (15 - j)) for j, c in enumerate(x[:16])))
    xl = np.uint64(sum(int(c) << (2 * (31 - j)) for j, c in enumerate(x[16:])))
    a, b = int(np.searchsorted(hi, xh, "left")), int(np.searchsorted(hi, xh, "right"))
    return a + int(np.searchsorted(lo[a:b], xl, "left")), a + int(np.searchsorted(lo[a:b], xl, "right"))


def stack_walk(E, bases, quals):
    """:207-262 -> dict(placed, start, EE, dup_steps, steps, sums: the four sums of the last step)"""
    n = len(bases)
    placed, start = [False] * n, [-1] * n
    placed_ids = []                                # (the placed entries, so that the sums need not pass over the others: their order does not matter to integer sums)
    table = lookup_table(bases)
    EE = [int(c) for c in E[:KW]]
    dup_steps = steps = 0
    live_sum = live_max = 0
    while True:
        steps += 1
        low, high = bounds(table, EE[len(EE) - KW:])
        duplicate = False
        for i in range(low + 1, high):
            if table[2][i] == table[2][i - 1]:
                duplicate = True
                break
        if not duplicate:
            for i in range(low, high):
                id = int(table[2][i])
                if placed[id]: continue
                placed[id] = True
                placed_ids.append(id)
                start[id] = len(EE) - KW - int(table[3][i])
        else: dup_steps += 1
        qsum = [0, 0, 0, 0]
        live = 0
        for id in placed_ids:
            pos = len(EE) - start[id]
            if pos >= len(bases[id]): continue
            qsum[int(bases[id][pos])] += int(quals[id][pos])
            live += 1
        live_sum += live; live_max = max(live_max, live)
        order = sorted(range(4), key=lambda b: -qsum[b])
        if qsum[order[0]] < MIN_WIN or float(qsum[order[0]]) < 2.0 * float(qsum[order[1]]):
            return dict(placed=placed, start=start, EE=EE, dup_steps=dup_steps, steps=steps, sums=qsum, live_sum=live_sum, live_max=live_max)
        assert qsum[order[0]] > qsum[order[1]]                                     # a base is appended only when the maximum is unique
        EE.append(order[0])


def ee_bound(lens):
    """no walk over entries of these lengths gives an EE longer than this (dfk_walks.h proves it)"""
    return KW + sum(max(0, int(l) - KW) for l in lens)


def one_pair(idsfw, E0, E1, bases_of, quals_of):
    """a pair -> its two records: dict(status, entries, placed, dup_steps, nE, nEE, M, trim, locs, EE, ...)"""
    basesx = [np.asarray(bases_of(id), np.int64) for id, fw in idsfw]
    qualsy = [lower(b, quals_of(id)) for b, (id, fw) in zip(basesx, idsfw)]
    basesy = list(basesx)
    for i, (id, fw) in enumerate(idsfw):
        if not fw: basesy[i], qualsy[i] = revcomp(basesy[i], qualsy[i])
    out = []
    for spass in (1, 2):
        E = E0 if spass == 1 else E1
        rec = dict(status=WALKED, entries=len(idsfw), placed=0, dup_steps=0, nE=len(E), nEE=0, M=0, trim=0, locs=[], EE=[], steps=0, live_sum=0, live_max=0, sums=None)
        out.append(rec)
        if spass == 2:
            for i in range(len(basesy)): basesy[i], qualsy[i] = revcomp(basesy[i], qualsy[i])
        if len(E) < KW:
            rec["status"] = SHORT
        else:
            w = stack_walk(E, basesy, qualsy)
            assert len(w["EE"]) <= ee_bound([len(b) for b in basesy])
            rec.update(nEE=len(w["EE"]), EE=w["EE"], dup_steps=w["dup_steps"], steps=w["steps"], sums=w["sums"], live_sum=w["live_sum"], live_max=w["live_max"])
            M = 0
            for i, (id, fw) in enumerate(idsfw):
                if not w["placed"][i]: continue
                rec["locs"].append((int(id), w["start"][i], bool(fw) ^ (spass == 2)))
                M = max(M, w["start"][i] + len(basesy[i]))
            rec.update(placed=len(rec["locs"]), M=M, trim=max(0, M - MAX_WIDTH))
        if not rec["locs"]:
            if spass == 1: out.append(dict(rec, status=NOT_WALKED, placed=0, dup_steps=0, nE=len(E1), nEE=0, M=0, trim=0, locs=[], EE=[], steps=0, live_sum=0, live_max=0, sums=None))
            break
    return out


def record_words(r):
    return [r["status"], r["entries"], r["placed"], r["dup_steps"], r["nE"] % 2**32, r["nEE"], r["M"] % 2**32, r["trim"] % 2**32]


def pack2(codes):
    c = np.concatenate([np.asarray(codes, np.uint8), np.zeros((-len(codes)) % 4, np.uint8)]).reshape(-1, 4)
    return (c[:, 0] | (c[:, 1] << 2) | (c[:, 2] << 4) | (c[:, 3] << 6)).astype(np.uint8)


def walks_file(recs):
    n = len(recs)
    starts = np.concatenate([[0], np.cumsum([r["placed"] for r in recs])]).astype("<u8")
    ee = np.concatenate([[0], np.cumsum([r["nEE"] for r in recs])]).astype("<u8")
    locs = closer_oracle.loc_words([l for r in recs for l in r["locs"]]).astype("<u8").tobytes()
    b = pack2([c for r in recs for c in r["EE"]]).tobytes()
    return (MAGIC + struct.pack("<Q", n) + starts.tobytes() + ee.tobytes() + np.asarray([w for r in recs for w in record_words(r)], "<u4").tobytes() + locs + b + bytes((-len(b)) % 8))


def digest_of(recs):
    words = [np.asarray([w for r in recs for w in record_words(r)], np.uint64), closer_oracle.loc_words([l for r in recs for l in r["locs"]]),
             np.asarray([c for r in recs for c in r["EE"]], np.uint64)]
    return seq_digest(np.concatenate(words), SALT)


def run(inv, edge_bases, ce, reads_per, pairs, bases_of, quals_of):
    """inv per edge; edge_bases[e] the codes of O(e); ce ascending, reads_per the (id, fw) per rank; pairs [(e1, e2)] ->
    dict(recs: two a pair, file, digest, the counters)"""
    rank = {int(e): k for k, e in enumerate(ce)}
    recs = []
    for e1, e2 in pairs:
        es = [int(e1), int(inv[e2])]
        idsfw = closer_oracle.compose(reads_per[rank[es[0]]], reads_per[rank[es[1]]])
        recs += one_pair(idsfw, edge_bases[es[0]], edge_bases[es[1]], bases_of, quals_of)
    walked = [r for r in recs if r["status"] == WALKED]
    total = lambda k, rs=recs: sum(int(r[k]) for r in rs)
    return dict(recs=recs, file=walks_file(recs), digest=digest_of(recs), pairs=len(pairs), walks=len(walked), entries=total("entries", walked), placed=total("placed"),
                sum_ee=total("nEE"), longest=max([r["nEE"] for r in recs] + [0]), dup_steps=total("dup_steps"), steps=total("steps"),
                past_edge=sum(1 for r in walked if r["nEE"] > r["nE"]), side0_empty=sum(1 for r in recs[0::2] if r["placed"] == 0),
                side1_empty=sum(1 for r in recs[1::2] if r["status"] == WALKED and r["placed"] == 0), short=sum(1 for r in recs if r["status"] == SHORT),
                trimmed=sum(1 for r in recs if r["trim"] > 0), live_sum=total("live_sum"), live_max=max([r["live_max"] for r in recs] + [0]),
                yields=sum(1 for a, b in zip(recs[0::2], recs[1::2]) if a["placed"] and b["placed"]))


# ---- the fixtures
_cache = {}


def fixture_inputs(golden_dir, case, K, which):
    from tests import cons_oracle, partners_oracle
    if ("in", case) not in _cache:
        i = partners_oracle.fixture_inputs(golden_dir, case, K, which)
        c = closer_oracle.fixture_closer(golden_dir, case, K, which)
        _cache[("in", case)] = dict(inv=i["inv"], edge_bases=i["edge_bases"], ce=c["ce"], reads_per=[r["reads"] for r in c["per"]], pairs=i["pairs"], rs=i["rs"],
                                    read_bases=i["read_bases"], quals_of=cons_oracle.fixture_quals(i["rs"]))
    return _cache[("in", case)]


def fixture_walks(golden_dir, case, K, which):
    """run() on a fixture; computed once per session and handed out unchanged"""
    if case not in _cache:
        i = fixture_inputs(golden_dir, case, K, which)
        memo = {}

        def bases_of(id):
            if id not in memo: memo[id] = i["read_bases"](id)
            return memo[id]
        _cache[case] = run(i["inv"], i["edge_bases"], i["ce"], i["reads_per"], i["pairs"], bases_of, i["quals_of"])
    return _cache[case]
