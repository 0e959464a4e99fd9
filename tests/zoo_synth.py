"""A seeded "zoo" of degenerate graph topology for the graph, path and mark tests: branch-free circles of many lengths (pure tandem
repeats among them), reverse-complement-symmetric repeats, homopolymers and microsatellites between random flanks, tandem repeats
whose unit is longer than K, and a diploid stretch read by pairs with PCR duplicates.  One read set serves K = 40, 48 and 60: every
member is covered by 100-base reads from both strands, three copies or more, from two barcodes or more (MIN_FREQ = 3, min_bc = 2).
tests/golden/make_golden.py writes make_zoo(ZOO_SEED) through the reference's classes (tests/golden/zoo.*, graph_zoo_k*/); the GPU
tests run other seeds against the Python oracles.  Harness only.

Members the reference refuses ("not a graph input"): none -- the reference's edge builder, HBV builder, pather, writePathsIndex
and MarkDups took every member below at all three K.
"""
import numpy as np

ZOO_SEED = 2024
READ = 100
# isolated circles: every length of the list once; the reads wrap around
CIRCLES = (1, 2, 3, 5, 6, 7, 11, 37) + tuple(K + d for K in (40, 48, 60) for d in (-1, 0, 1, 2, 3)) + (97, 128, 129, 401, 1000)
# the small ones are pure tandem repeats: primitive units, none a rotation of its own reverse complement (a random unit may be)
UNITS = {1: "A", 2: "AC", 3: "AAC", 5: "AACCG", 6: "AACCGT", 7: "AACGTGC", 11: "AACAGATCCGT"}
# ... and these are: their k-mers are palindromes or pair up with another rotation, differently at each K
SYMMETRIC = ("AT", "ACGT", "AACGTT")
# (unit, bases) between random flanks: loop edges on a branching vertex; no unit is a rotation of a circle's or of its complement
STRETCHES = (("C", 70), ("C", 180), ("AG", 65), ("AG", 151), ("ACT", 90), ("AAG", 92), ("AAGC", 199), ("ACATG", 74), ("AGGTCT", 197))
# a unit of 70 bases, longer than K, four times and a part of a fifth: the loop closes on ONE vertex where the stretch has K-1 bases
# more than whole units, so there is one such repeat for each K (at the other two K its cycle is cut into two edges)
TANDEM_UNIT = 70
TANDEMS = tuple(4 * TANDEM_UNIT + K - 1 for K in (40, 48, 60))
QUALS = (30, 35, 37, 40, 50, 60)                            # one a read; three substitutions reach 150 and pass it


def codes(s):
    return np.array(["ACGT".index(c) for c in s], np.uint8)


def rc(a):
    return (3 - a[::-1]).astype(np.uint8)


def _rotations(u):
    return {bytes(np.roll(u, -i)) for i in range(len(u))}


def check_units():
    """the explicit units are primitive, not reverse-complement symmetric, and no two members share a repeat"""
    seen = set()
    for s in list(UNITS.values()) + list(dict(STRETCHES)):
        u = codes(s)
        assert len(_rotations(u)) == len(u), f"{s} is not primitive"
        assert bytes(rc(u)) not in _rotations(u), f"{s} is a rotation of its reverse complement"
        assert not (_rotations(u) | _rotations(rc(u))) & seen, f"{s} is another member's repeat"
        seen |= _rotations(u) | _rotations(rc(u))
    for s in SYMMETRIC:
        assert bytes(rc(codes(s))) in _rotations(codes(s))


def _tile(seq, step, copies):
    """100-base reads around the circle seq every `step` bases, `copies` of each, strands alternating"""
    n = len(seq)
    seq = np.tile(seq, (max(n, 2 * step) + READ) // n + 2)
    out = []
    for pos in range(0, max(n, 2 * step), step):
        for c in range(copies):
            r = seq[pos:pos + READ].copy()
            out.append(rc(r) if (pos // step + c) % 2 else r)
    return out


def _between_flanks(rng, stretch, period):
    """the stretch and 300 random bases, closed to a circle (no ends, where the coverage would thin out); the random bases next to
    the stretch do not continue its period"""
    f = rng.integers(0, 4, 300, dtype=np.uint8)
    if f[0] == stretch[len(stretch) - period]: f[0] = (f[0] + 1) & 3
    if f[-1] == stretch[period - 1]: f[-1] = (f[-1] + 1) & 3
    return np.concatenate([stretch, f])


def zoo_members(seed, diploid=20000, diploid_pairs=8000, copies=3):
    """-> (reads, quals, bci, clean, member): base codes and qualities a read, the barcode index (pairs sorted by barcode), whether
    a read is error-free, and the name of the member it was read from"""
    check_units()
    rng = np.random.default_rng(seed)
    pairs = []                                               # (r1, r2, member, barcode)
    n_bc = 24

    def add(name, reads):
        if len(reads) % 2: reads.append(reads[0].copy())
        for i in range(0, len(reads), 2):
            pairs.append((reads[i], reads[i + 1], name, 1 + len(pairs) % n_bc))   # neighbours -- the copies of a read -- differ in barcode

    for n in CIRCLES:
        unit = codes(UNITS[n]) if n in UNITS else rng.integers(0, 4, n, dtype=np.uint8)
        add(f"circle{n}", _tile(unit, 7, copies))
    for s in SYMMETRIC:
        add(f"symmetric{len(s)}", _tile(codes(s), 7, copies))
    for u, bases in STRETCHES:
        stretch = np.tile(codes(u), bases // len(u) + 1)[:bases]
        add(f"stretch{u}{bases}", _tile(_between_flanks(rng, stretch, len(u)), 5, copies))
    for bases in TANDEMS:
        unit = rng.integers(0, 4, TANDEM_UNIT, dtype=np.uint8)
        add(f"tandem{bases}", _tile(_between_flanks(rng, np.tile(unit, 5)[:bases], TANDEM_UNIT), 5, copies))
    # the diploid stretch: make_frag's, closed to a circle and without its low-quality errors (the substitutions below are the zoo's)
    a = rng.integers(0, 4, diploid, dtype=np.uint8)
    b = a.copy()
    pos = 200
    while pos < diploid - 200:
        b[pos] = (b[pos] + rng.integers(1, 4)) & 3
        pos += int(rng.choice([30, 50, 70, 90, 140]))
    first = len(pairs)
    for p in range(diploid_pairs):
        if p > 10 and rng.random() < 0.10:                   # a PCR duplicate of an earlier pair
            r1, r2 = (x.copy() for x in pairs[first + int(rng.integers(0, p))][:2])
        else:
            ins = int(rng.integers(250, 400)); start = int(rng.integers(0, diploid)); h = (a, b)[int(rng.integers(0, 2))]
            h = np.concatenate([h[start:], h[:start]])       # (the circle cut open at the pair's start)
            r1 = h[:READ].copy(); r2 = rc(h[ins - READ:ins])
            if rng.random() < 0.5: r1, r2 = r2, r1
        pairs.append((r1, r2, "diploid", 0 if rng.random() < 0.1 else int(rng.integers(1, n_bc + 1))))
    order = sorted(range(len(pairs)), key=lambda i: pairs[i][3])             # (stable: the barcode index wants the pairs sorted)
    reads, quals, clean, member = [], [], [], []
    for i in order:
        r1, r2, name, _ = pairs[i]
        for r in (r1, r2):
            ok = rng.random() >= 0.10
            if not ok:                                       # one to three substitutions of high quality, drawn for this copy alone
                k = int(rng.integers(1, 4))
                at = rng.choice(READ, k, replace=False)
                r[at] = (r[at] + rng.integers(1, 4, k)) & 3
            reads.append(r); quals.append(np.full(READ, QUALS[int(rng.integers(0, len(QUALS)))], np.uint8))
            clean.append(ok); member.append(name)
    counts = np.bincount([pairs[i][3] for i in order], minlength=n_bc + 1)
    bci = np.concatenate([[0], np.cumsum(counts * 2)]).astype(np.int64)
    return reads, quals, bci, np.array(clean), member


def make_zoo(seed, **kw):
    """-> (reads, quals, bci) like the makers of tests/golden/make_golden.py"""
    return zoo_members(seed, **kw)[:3]


def read_set(reads, quals, bci):
    """the arrays the ABI takes (feudal.pq_encode writes the qualities: a valid encoding, not necessarily the reference's bytes)"""
    from superplus_amd import feudal
    n = len(reads)
    read_len = np.array([len(r) for r in reads], np.uint32)
    packed = np.concatenate([feudal.pack_bases(r[None, :])[0] for r in reads])
    base_off = np.concatenate([[0], np.cumsum((read_len.astype(np.uint64) + 3) // 4)]).astype(np.uint64)
    pqs = [np.frombuffer(feudal.pq_encode(q), np.uint8) for q in quals]
    pq_off = np.concatenate([[0], np.cumsum([len(x) for x in pqs])]).astype(np.uint64)
    return dict(packed=packed, base_off=base_off, read_len=read_len, pq_bytes=np.concatenate(pqs), pq_off=pq_off,
                bc=feudal.bci_to_bc(bci, n), n_reads=n)


def graph_classes(g, K):
    """What a graph (oracle.graph_oracle.run's result, or any object with .edges / .hbv) holds of the zoo's classes:
    cycles: (k-mers, stored orientation, where the middle base of an odd length lies) per branch-free cycle edge (canonical edges:
            a circle gives one, its mirror image is the HBV's business); the orientation is that of the stored edge against the walk
            from the cycle's smallest canonical k-mer in that k-mer's canonical orientation
    loops:  k-mers of every HBV edge that starts and ends on one vertex which other edges touch too
    palindromes: one-k-mer edges equal to their reverse complement
    ordinary: the k-mers of the HBV edges that are neither (the set of them)"""
    h = g["hbv"]
    left, right = h.to_left_right()
    rcs = lambda s: bytes(3 - b for b in reversed(s))
    cycles, loops = [], []
    for c, s in enumerate(g["edges"]):
        e = h.fwd[c]
        if left[e] != right[e] or len(h.frm[left[e]]) != 1 or len(h.to[left[e]]) != 1: continue
        n, L = len(s) - K + 1, len(s)
        best = min(range(n), key=lambda i: min(s[i:i + K], rcs(s[i:i + K])))
        as_walked = s[best:best + K] <= rcs(s[best:best + K])
        assert best == (0 if as_walked else n - 1) or n == 1
        mid = L // 2
        where = None if L % 2 == 0 else ("first" if mid < K else "") + ("last" if mid >= n - 1 else "") or "between"
        cycles.append((n, "fwd" if as_walked else "rev", where))
    for e in range(len(h.edges)):
        v = left[e]
        if v == right[e] and (len(h.frm[v]) > 1 or len(h.to[v]) > 1): loops.append(len(h.edges[e]) - K + 1)
    pal = sum(1 for s in h.edges if len(s) == K and rcs(s) == s)
    ordinary = {len(s) - K + 1 for e, s in enumerate(h.edges) if left[e] != right[e] and not (len(s) == K and rcs(s) == s)}
    return dict(cycles=cycles, loops=sorted(loops), palindromes=pal, ordinary=ordinary, n_edges=len(h.edges))


def most_repeats(paths):
    """the largest number of times one read's path names one edge"""
    return max((max(np.bincount(p)) for _, p in paths if len(p)), default=0)
