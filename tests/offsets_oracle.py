"""GetOffsets1 (paths/long/ReadStack.cc:1192-1512), the next statement of CloseGap2 (10X/Closomatic.cc:648), restated in plain Python on
the two consensus sequences of a pair, the file a.close.offsets of dfk_offsets_write and its digest.

What is pinned on what: no reference-written form of this result exists (ReadStack.cc does not compile here), so the rule is pinned by
two restatements written independently from the reference's text -- this module and superplus_amd/csrc/dfk_offsets.h.  The INPUTS are
the consensus bases per pair and side (tests/cons_oracle.py on the fixtures, tests/offsets_cases.py's seeded sequences).

The text, for con1, con2 (values 0..3, at most 400 long each; the early return for 1000 and more, :1229, cannot be reached):

  table       :48-62, :1214, random/Bernoulli.cc:40-50.  gBS[n][k] = log10( BinomialSum( n, k, 0.75 ) ) for 20 <= n, 0 <= k < n; the sum
              in LONG DOUBLE: sum += choose * product; choose *= double(n - i); choose /= double(i + 1); product *= p / (1.0 - p), from
              product = pow( 1.0 - p, double(n) ); the return converts to double.  gBS[n][n] is never written: the object is static, so 0.
  candidates  :1233-1254.  the 8-mers of both, sorted; within a run of equal 8-mers every ( l1 on con1, l2 on con2 ) gives
              o = third(l1) - third(l2); UniqueSort.
  oom         :1258-1269.  per o: overlap and mismatch over p1 with 0 <= p1 - o < |con2|.
  bits        :1275-1332.  pos1, pos2; sum_errors; bad_window (errs over a window of wx = 40, set at Max( 0, m - wx ) when errs >= 20);
              for start, for n from w = 20: bad if n - wx >= 0 and bad_window[ start + n - wx ]; k; break if bad; minp = Min( minp,
              gBS[n][k] ).  bitsj = -minp * 10.0 / 6.0; kept if bitsj >= 25.0 with fraglen = offset + |con2|.
  invalidates :1422-1485.  val1, val2 per offset from the agreeing runs less flank = 10 at each end (the inner loop advances the outer
              loop's p1); invalidates[j][i]; the two-step deletion; EraseIf.
  big / small :1489-1502.  to_delete2, the test of to_delete2[i1] inside the inner loop; EraseIf.

Every vector is materialised as the loops stand.  One thing is not a Python loop: the `n` loop of a `start` takes its gBS values with one
numpy gather and one minimum (Min is exact and order-free); bits_loops() below is the same statement with the loop and the break as
written, and tests/test_offsets_oracle.py holds the two to each other."""
import math
import struct

import numpy as np

from tests.closer_oracle import seq_digest

FILE = "a.close.offsets"
MAGIC = b"DFKCOFF1"
SALT = 0xF0F0
MAX_N = 400
SURVIVES, INVALIDATED, SMALL = 0, 1, 2

_table = None


def binomial_sums(n, p=0.75):
    """BinomialSum( n, k, p ) for k = 0..n-1 as long doubles: the loop of Bernoulli.cc:44-50 run once, its sum read after every pass
    (the calls for k and k + 1 do the same operations up to pass k)"""
    assert np.finfo(np.longdouble).nmant == 63
    L = np.longdouble
    sum_, choose, product = L(0), L(1.0), L(math.pow(1.0 - p, float(n)))
    ratio = L(p / (1.0 - p))
    out = []
    for i in range(n):
        sum_ = sum_ + choose * product
        out.append(sum_)
        choose = choose * L(float(n - i))
        choose = choose / L(float(i + 1))
        product = product * ratio
    return out


def table():
    """gBS as a (401, 401) float64 array: rows 20..400, cells k < n; everything else 0 (static storage)"""
    global _table
    if _table is None:
        T = np.zeros((MAX_N + 1, MAX_N + 1), np.float64)
        for n in range(20, MAX_N + 1):
            for k, s in enumerate(binomial_sums(n)):
                T[n, k] = math.log10(float(s))
        T.setflags(write=False)
        _table = T
    return _table


def candidates(con1, con2):
    """:1233-1254"""
    K = 8
    kmers_plus = []
    for idx, con in enumerate((con1, con2)):
        for j in range(len(con) - K + 1):
            kmers_plus.append((tuple(int(b) for b in con[j:j + K]), idx, j))
    kmers_plus.sort()
    doffsets = []
    i = 0
    while i < len(kmers_plus):
        j = i + 1
        while j < len(kmers_plus) and kmers_plus[j][0] == kmers_plus[i][0]: j += 1
        for l1 in range(i, j):
            if kmers_plus[l1][1] != 0: continue
            for l2 in range(i, j):
                if kmers_plus[l2][1] != 1: continue
                doffsets.append(kmers_plus[l1][2] - kmers_plus[l2][2])
        i = j
    return sorted(set(doffsets))


def windows(con1, con2, offset, overlap, size):
    """:1279-1304 -> (sum_errors, bad_window), bad_window of `size` entries"""
    wx, max_ewx = 40, 20
    pos1 = 0 if offset < 0 else offset
    pos2 = -offset if offset < 0 else 0
    sum_errors = [0] * (overlap + 1)
    for i in range(1, overlap + 1):
        sum_errors[i] = sum_errors[i - 1] + (1 if con1[pos1 + i - 1] != con2[pos2 + i - 1] else 0)
    errs = 0
    bad_window = [False] * size
    for m in range(0, overlap - wx + 1):
        if con1[pos1 + m] != con2[pos2 + m]: errs += 1
        if m >= wx and con1[pos1 + m - wx] != con2[pos2 + m - wx]: errs -= 1
        if errs >= max_ewx: bad_window[max(0, m - wx)] = True
    return sum_errors, bad_window


def bits_loops(sum_errors, bad_window, overlap, T):
    """:1306-1327 with the loops and the break as written -> (bits, look-ups)"""
    w, wx = 20, 40
    minp = 0.
    lookups = 0
    for start in range(overlap):
        bad = False                                   # (:1310's loop never runs: w - wx < 0)
        for n in range(w, overlap - start + 1):
            if n - wx >= 0 and bad_window[start + n - wx]: bad = True
            k = sum_errors[start + n] - sum_errors[start]
            if bad: break
            g = float(T[n, k])
            minp = g if g < minp else minp
            lookups += 1
    return -minp * 10.0 / 6.0, lookups


def bits_of(sum_errors, bad_window, overlap, T):
    """the same, the `n` loop of a `start` one gather and one minimum"""
    w, wx = 20, 40
    S = np.asarray(sum_errors, np.int64)
    bw = np.asarray(bad_window, bool)
    minp = 0.
    lookups = 0
    for start in range(overlap):
        last = overlap - start
        if last >= wx:
            hit = np.flatnonzero(bw[start:start + last - wx + 1])       # bad_window[ start + n - wx ] for n = wx .. last
            if len(hit): last = wx + int(hit[0]) - 1                     # the break at the first
        if last < w: continue
        ns = np.arange(w, last + 1)
        g = float(T[ns, S[start + ns] - S[start]].min())
        minp = g if g < minp else minp
        lookups += len(ns)
    return -minp * 10.0 / 6.0, lookups


def tail(con1, con2, offsets):
    """:1422-1502 on the offsets that passed the bits test, [(offset, bits)] -> a state per offset"""
    n1, n2 = len(con1), len(con2)
    N = len(offsets)
    flank = 10
    val1 = [[False] * n1 for _ in range(N)]
    val2 = [[False] * n2 for _ in range(N)]
    for i in range(N):
        o = offsets[i][0]
        p1 = 0
        while p1 < n1:
            p2 = p1 - o
            if p2 < 0 or p2 >= n2 or con1[p1] != con2[p2]:
                p1 += 1
                continue
            low1 = p1
            while p1 < n1:
                p2 = p1 - o
                if p2 >= n2: break
                if con1[p1] != con2[p2]: break
                p1 += 1
            high1 = p1
            for q1 in range(low1 + flank, high1 - flank):
                val1[i][q1] = True
                val2[i][q1 - o] = True
            p1 += 1
    invalidates = [[False] * N for _ in range(N)]
    for i in range(N):
        o = offsets[i][0]
        for p1 in range(n1):
            p2 = p1 - o
            if p2 < 0 or p2 >= n2: continue
            if con1[p1] == con2[p2]: continue
            for j in range(N):
                if val1[j][p1] and val2[j][p2]: invalidates[j][i] = True
    to_delete = [False] * N
    for i in range(N):
        good = True
        for j in range(N):
            if invalidates[j][i]: good = False
        if not good: continue
        for j in range(N):
            if invalidates[i][j]: to_delete[j] = True
    state = [INVALIDATED if to_delete[i] else SURVIVES for i in range(N)]
    left = [i for i in range(N) if not to_delete[i]]
    min_bits_save, min_slope, min_add = 40.0, 2.0, 10.0
    to_delete2 = [False] * len(left)
    for i1 in range(len(left)):
        for i2 in range(len(left)):
            if to_delete2[i1]: continue
            if offsets[left[i2]][1] >= min_bits_save: continue
            delta_bits = offsets[left[i1]][1] - offsets[left[i2]][1]
            if delta_bits < min_add: continue
            if delta_bits / abs(offsets[left[i1]][0] - offsets[left[i2]][0]) < min_slope: continue
            to_delete2[i2] = True
    for x, i in enumerate(left):
        if to_delete2[x]: state[i] = SMALL
    return state


def get_offsets1(con1, con2, T=None, loops=False):
    """-> dict(candidates, records [(offset, overlap, fraglen, mismatch, bits, state)] for the offsets that passed the bits test,
    survivors [offset], lookups, tnn: windows read at gBS[n][n])"""
    T = table() if T is None else T
    con1, con2 = [int(b) for b in con1], [int(b) for b in con2]
    assert max(len(con1), len(con2), 0) <= MAX_N
    doffsets = candidates(con1, con2)
    oom = []
    max_overlap_seen = 0
    for o in doffsets:
        overlap = mismatch = 0
        for p1 in range(len(con1)):
            p2 = p1 - o
            if p2 < 0 or p2 >= len(con2): continue
            overlap += 1
            if con1[p1] != con2[p2]: mismatch += 1
        max_overlap_seen = max(max_overlap_seen, overlap)
        oom.append((o, overlap, mismatch))
    offsets = []
    lookups = 0
    for offset, overlap, mismatch in oom:
        assert overlap > 0
        sum_errors, bad_window = windows(con1, con2, offset, overlap, max_overlap_seen)
        bitsj, n = (bits_loops if loops else bits_of)(sum_errors, bad_window, overlap, T)
        lookups += n
        if bitsj >= 25.0: offsets.append((offset, overlap, offset + len(con2), mismatch, bitsj))
    state = tail(con1, con2, [(r[0], r[4]) for r in offsets])
    records = [r + (s,) for r, s in zip(offsets, state)]
    return dict(candidates=len(doffsets), records=records, survivors=[r[0] for r in records if r[5] == SURVIVES], lookups=lookups)


def offsets_file(starts, words, records):
    return (MAGIC + struct.pack("<Q", len(starts) - 1) + np.asarray(starts, "<u8").tobytes() + b"".join(struct.pack("<IIII", *w, 0) for w in words)
            + b"".join(struct.pack("<iiiidII", *r, 0) for r in records))


def digest_of(words, records):
    w = np.frombuffer(b"".join(struct.pack("<IIII", *x, 0) for x in words), "<u4")
    r = np.frombuffer(b"".join(struct.pack("<iiiidII", *x, 0) for x in records), "<u4")
    return seq_digest(np.concatenate([w.astype(np.uint64), r.astype(np.uint64)]), SALT)


def run(seqs):
    """seqs: [con1 of pair 0, con2 of pair 0, con1 of pair 1, ...] -> dict(per, starts, words, records, file, digest, the counters)"""
    assert len(seqs) % 2 == 0
    T = table()
    per = [get_offsets1(seqs[2 * p], seqs[2 * p + 1], T) for p in range(len(seqs) // 2)]
    words = [(g["candidates"], len(g["records"]), len(g["survivors"])) for g in per]
    records = [r for g in per for r in g["records"]]
    starts = [0] + [int(x) for x in np.cumsum([w[1] for w in words])]
    ns = [w[2] for w in words]
    return dict(per=per, starts=starts, words=words, records=records, file=offsets_file(starts, words, records), digest=digest_of(words, records),
                pairs=len(per), candidates=sum(w[0] for w in words), passed=len(records), invalidated=sum(r[5] == INVALIDATED for r in records),
                deleted_small=sum(r[5] == SMALL for r in records), survivors=sum(ns), pairs0=sum(n == 0 for n in ns), pairs1=sum(n == 1 for n in ns),
                pairs2=sum(n == 2 for n in ns), pairs_more=sum(n > 2 for n in ns), closable=sum(n in (1, 2) for n in ns), lookups=sum(g["lookups"] for g in per))


def starts_and_bases(seqs):
    """the arrays dfk_offsets_build_arrays takes"""
    starts = np.zeros(len(seqs) + 1, np.uint64)
    starts[1:] = np.cumsum([len(s) for s in seqs], dtype=np.uint64)
    return starts, np.concatenate([np.asarray(s, np.uint8) for s in seqs] + [np.zeros(0, np.uint8)])


# ---- the fixtures
_cache = {}


def fixture_offsets(golden_dir, case, K, which):
    """run() on a fixture's consensus as tests/cons_oracle.py gives it; computed once per session and handed out unchanged"""
    if case not in _cache:
        from tests import cons_oracle
        c = cons_oracle.fixture_cons(golden_dir, case, K, which)
        seqs = [c["bases"][c["starts"][q]:c["starts"][q + 1]] for q in range(c["n_stacks"])]
        _cache[case] = dict(run(seqs), seqs=seqs)
    return _cache[case]
