"""tests/patch_seeded.py -- TEST INFRASTRUCTURE for the patched graph (tests/patch_oracle.py, superplus_amd/csrc/dfk_patch.h): seeded graphs
with closures at every K, closures placed so that heads and novel K-mers fall on the lanes and blocks where the kernels' ranking can go
wrong, and the properties a consumer of hb3 / to3 / left3 relies on, stated without the oracle.  CPU-only code.

  small_zoo(K, seed)        contigs for patch_cases.graph_of: circles of many lengths (a circle is a contig followed by its own first K - 1
                            bases: the old graph shows it as an edge from a vertex to itself, BuildAll's crossing closes it, and hb3 starts the
                            cycle at its smallest canonical K-mer, not where the old edge starts), pure tandem circles, reverse-complement
                            symmetric circles (palindromic K-mers: self-inverse one-K-mer edges), a loop on a branching vertex, a tandem
                            repeat with a unit longer than K, a palindrome, a 2 x 2 vertex, plain contigs down to one K-mer
  closures_for(g, rng, n)   closures made of the graph's own edges: joins, interior jumps (given forwards, reverse-complemented and twice),
                            windows on old edges, noise around K bases, novel palindromes, walks across a vertex, an edge's end back to its
                            own start or to its inverse, SNP bubbles, tandem closures; empty ones first, last and two side by side
  aligned_case(K, variant)  one long contig and three short ones; closures of K + 1 bases put heads at chosen slots, novel and old closures
                            are laid out so that whole waves of closure positions are all novel, novel in lane 0 or lane 63 alone, or not
                            at all; `coverage()` says what the case reaches and tests assert it
  head_slots, fresh_flags   where the heads and the novel K-mers are, from a result and from the sequences
  check_invariants(...)     an old edge can be read back off hb3 along to3 from left3, and hb3 holds together"""
import numpy as np

from oracle import graph_oracle as go
from tests import patch_cases, patch_oracle as po

KS = (40, 48, 60)
SEEDS = (1, 2)
VARIANTS = ("A", "B")
TANDEM_UNITS = ("AACCG", "AACGTGC")
SYMMETRIC = ("AT", "ACGT")


def codes(s):
    return bytes("ACGT".index(c) for c in s)


def circle(unit, K):
    """the circle of `unit` cut open: the unit, then its own first K - 1 bases (around the circle again where it is shorter)"""
    n = len(unit)
    return (unit * ((n + K - 1) // n + 1))[:n + K - 1]


def small_zoo(K, seed):
    rng = np.random.default_rng([seed, K, 7001])
    rnd = lambda n: bytes(rng.integers(0, 4, int(n), dtype=np.uint8))
    out = [circle(rnd(n), K) for n in (K - 1, K, K + 1, 97, 249)]
    out += [circle(codes(u), K) for u in TANDEM_UNITS + SYMMETRIC]
    stretch = (codes("AAG") * 31)[:92]                                        # between random bases that do not continue its period
    f = bytearray(rnd(300))
    if f[0] == stretch[92 - 3]: f[0] = (f[0] + 1) & 3
    if f[-1] == stretch[2]: f[-1] = (f[-1] + 1) & 3
    out.append(circle(stretch + bytes(f), K))
    out.append(rnd(80) + (rnd(70) * 5)[:4 * 70 + K - 1] + rnd(80))
    p = rnd(K // 2)
    out.append(rnd(60) + p + go.rc_seq(p) + rnd(60))
    m = rnd(K - 1)
    out += [rnd(80) + m + rnd(80), rnd(80) + m + rnd(80)]
    out += [rnd(n) for n in (K, K + 1, 150, 333, 700)]
    return out


# ----------------------------------------------------------------------------------------------- closures
def closures_for(g, rng, n_each=2):
    K, edges = g["K"], g["edges"]
    E = len(edges)
    _, frm = po.adjacency(g)
    noise = lambda n: bytes(rng.integers(0, 4, int(n), dtype=np.uint8))
    r = lambda lo, hi: int(rng.integers(lo, hi + 1))                         # both ends included

    def pick(min_len=0, ok=lambda e: True):
        c = [e for e in range(E) if len(edges[e]) >= min_len and ok(e)] or [e for e in range(E) if ok(e)] or list(range(E))
        return c[r(0, len(c) - 1)]

    def tail(e): return edges[e][-min(len(edges[e]), K + r(0, 22)):]
    def head(e): return edges[e][:K + r(0, 22)]

    def window(e, n):
        s = edges[e]
        n = min(n, len(s))
        a = r(0, len(s) - n)
        return s[a:a + n]

    def interior(e):
        s = edges[e]
        if len(s) < K + 2: return s
        n = r(K, min(len(s) - 2, K + 30))
        a = r(1, len(s) - n - 1)
        return s[a:a + n]

    out = []
    for _ in range(n_each):
        out.append(tail(pick()) + noise(r(0, 29)) + head(pick()))
        jump = interior(pick(K + 2)) + noise(r(0, 29)) + interior(pick(K + 2))
        out += [jump, go.rc_seq(jump), jump]
        out.append(window(pick(K + 20), r(K, K + 60)))
        out += [noise(r(0, K - 1)), noise(K), noise(K + 1)]
        x = noise(r(K // 2 + 1, K))
        out.append(x + go.rc_seq(x))
        e = pick(ok=lambda e: len(frm[g["to_right"][e]]) > 0)
        nxt = frm[g["to_right"][e]]
        if nxt:
            f = edges[nxt[r(0, len(nxt) - 1)]]
            out.append(tail(e) + f[K - 1:K - 1 + r(1, 30)])
        else:
            out.append(tail(e))
        e = pick(K + 2)
        out.append(tail(e) + noise(r(0, 29)) + head(e))
        t = tail(pick())
        out.append(t + noise(r(0, 29)) + go.rc_seq(t))
        w = bytearray(window(pick(2 * K + 20), r(K + 1, 2 * K + 20)))
        w[len(w) // 2] = (w[len(w) // 2] + r(1, 3)) & 3
        out.append(bytes(w))
        unit = noise(r(1, 11))
        out.append((unit * (2 * K))[:r(K + 1, K + 39)])
    mid = len(out) // 2
    return [b""] + out[:mid] + [b"", b""] + out[mid:] + [b""]


# ----------------------------------------------------------------------------------------------- the plan, heads, novel K-mers
def plan(g):
    """the canonical old edges in id order and first[c] = the K-mers before them (dfk_patch.h's plan_of)"""
    canon = [e for e in range(len(g["edges"])) if e <= g["inv"][e]]
    first = [0]
    for e in canon:
        first.append(first[-1] + len(g["edges"][e]) - g["K"] + 1)
    return canon, first


def head_slots(g, result):
    """{canonical old edge: the slots at which its walk starts a new hb3 edge}, read off to3 / left3 / kmers3"""
    canon, first = plan(g)
    out = {}
    for c, e in enumerate(canon):
        ids = result["to3"][e]
        pos, heads = 0, []
        for j, x in enumerate(ids):
            heads.append(first[c] + pos)
            pos += result["kmers3"][x] - (result["left3"][e] if j == 0 else 0)
        assert heads and heads[-1] < first[c + 1] <= first[c] + pos, f"old edge {e}: its path does not cover it"
        out[e] = heads
    return out


def old_keys(g):
    d = {}
    for e in range(len(g["edges"])):
        po.kmerize(g["edges"][e], g["K"], d)
    return d


def fresh_flags(g, closures):
    """per closure K-mer position, in the order the device numbers them: its canonical K-mer is on no old edge"""
    K = g["K"]
    old = old_keys(g)
    return [min(k, r) not in old for s in closures if len(s) >= K for k, r in po.rolled(s, K)]


# ----------------------------------------------------------------------------------------------- closures at chosen lanes and blocks
LONG = 1024                                                                   # K-mers of the long contig: four blocks of 256 slots
# heads wanted on the long contig: (slot, which kind of closure makes it)
AFTER = (63, 256, 512, 767)                                                   # L[p:p + K] + b with p = slot - 1: a second successor before the slot
BEFORE = (64, 255, 511, 768, 1023)                                            # b + L[p:p + K] with p = slot: a second predecessor at the slot


def aligned_case(K, variant):
    """-> (graph, closures).  The long contig's canonical edge is the first (HBVFromEdges numbers by length): slots 0 .. 1023; the three
    short ones bring the base K-mers to a multiple of 256 (variant A) or one more (B).  Closure positions: 128 novel; one novel, 63 old;
    63 old, one novel; 64 old; two a head closure (one old, one novel); then old ones up to a multiple of 256 (A) or one more (B)."""
    assert variant in VARIANTS
    rng = np.random.default_rng([K, 7002, VARIANTS.index(variant)])
    rnd = lambda n: bytes(rng.integers(0, 4, int(n), dtype=np.uint8))
    extra = 0 if variant == "A" else 1
    shorts = (100, 90, 66 + extra)
    g = patch_cases.graph_of([rnd(LONG + K - 1)] + [rnd(n + K - 1) for n in shorts], K)
    canon, first = plan(g)
    assert first[1] == LONG and first[-1] == LONG + 256 + extra
    L = g["edges"][canon[0]]
    other = lambda b: bytes([(b + 1 + int(rng.integers(0, 3))) & 3])
    S = g["edges"][canon[1]]                                                  # 100 K-mers: windows that lie wholly on an old edge
    closures = [rnd(128 + K - 1), rnd(K), S[:K + 62], S[20:20 + K + 62], rnd(K), S[10:10 + K + 63]]
    for slot in AFTER:
        p = slot - 1
        closures.append(L[p:p + K] + other(L[p + K]))
    for slot in BEFORE:
        closures.append(other(L[slot - 1]) + L[slot:slot + K])
    n_pos = sum(len(c) - K + 1 for c in closures)
    pad = (extra - n_pos) % 256
    while pad:
        n = min(pad, 100)
        closures.append(S[:K + n - 1]); pad -= n
    return g, closures


def coverage(g, closures, result):
    """what an aligned case reaches, from the oracle's side: {condition: holds}"""
    canon, first = plan(g)
    heads = head_slots(g, result)
    slots = sorted(s for h in heads.values() for s in h)
    fresh = fresh_flags(g, closures)
    runs = [fresh[i:i + 64] for i in range(0, len(fresh) - 63, 64)]
    return {
        "a head in lane 0": any(s % 64 == 0 for s in slots),
        "a head in lane 63": any(s % 64 == 63 for s in slots),
        "a head on a block's first slot, not slot 0": any(s > 0 and s % 256 == 0 for s in slots),
        "a head on a block's last slot": any(s % 256 == 255 for s in slots),
        "an old edge with heads in three blocks": any(len({s // 256 for s in h}) >= 3 for h in heads.values()),
        "a canonical edge starting on a block's first slot": any(f > 0 and f % 256 == 0 for f in first[:-1]),
        "a canonical edge ending on a block's last slot": any(f % 256 == 0 for f in first[1:]),
        "a wave of novel positions": any(all(r) for r in runs),
        "a wave novel in lane 0 alone": any(r[0] and not any(r[1:]) for r in runs),
        "a wave novel in lane 63 alone": any(r[63] and not any(r[:63]) for r in runs),
        "a wave without a novel position": any(not any(r) for r in runs),
        "n_base mod 256": first[-1] % 256,
        "n_pos mod 256": len(fresh) % 256,
    }


def assert_coverage(g, closures, result, variant, what):
    want = 0 if variant == "A" else 1
    for k, v in coverage(g, closures, result).items():
        assert v == (want if k.endswith("mod 256") else True), f"{what}: {k}: {v}"


# ----------------------------------------------------------------------------------------------- what a consumer relies on
def check_invariants(g, closures, edges3, inv3, to_left3, to_right3, to3, left3, kmers3=None, what=""):
    """edges3: hb3's edges by id (bytes of base codes); to3: a list of ids per old edge.  No oracle: the sequences alone."""
    K, edges = g["K"], g["edges"]
    E, E3 = len(edges), len(edges3)
    edges3 = [bytes(s) for s in edges3]
    assert len(inv3) == len(to_left3) == len(to_right3) == E3 and len(to3) == len(left3) == E, f"{what}: table sizes"
    # 1. spelling, 2. tightness
    for e in range(E):
        ids = [int(x) for x in to3[e]]
        assert ids, f"{what}: old edge {e} has an empty path"
        assert all(0 <= x < E3 for x in ids), f"{what}: old edge {e} names an edge hb3 does not have"
        spelled = edges3[ids[0]]
        for x in ids[1:]:
            assert spelled[-(K - 1):] == edges3[x][:K - 1], f"{what}: old edge {e}: hb3 edge {x} does not overlap the one before it in K - 1 bases"
            spelled += edges3[x][K - 1:]
        left = int(left3[e])
        assert 0 <= left <= len(edges3[ids[0]]) - K, f"{what}: old edge {e}: left3 {left} skips the whole first edge of its path"
        assert spelled[left:left + len(edges[e])] == bytes(edges[e]), f"{what}: old edge {e} is not what its path spells from left3"
        right = len(spelled) - left - len(edges[e])
        assert 0 <= right <= len(edges3[ids[-1]]) - K, f"{what}: old edge {e}: the last edge of its path is not used"
    # 3. the K-mer set
    want = old_keys(g)
    for c in closures:
        po.kmerize(bytes(c), K, want)
    got = {}
    for s in edges3:
        po.kmerize(s, K, got)
    assert set(got) == set(want), f"{what}: hb3 holds {len(set(got) - set(want))} K-mers nobody gave it and lacks {len(set(want) - set(got))}"
    assert all(len(s) >= K for s in edges3), f"{what}: an hb3 edge shorter than K"
    if kmers3 is not None:
        assert [int(x) for x in kmers3] == [len(s) - K + 1 for s in edges3], f"{what}: kmers3"
    assert sum(len(edges3[i]) - K + 1 for i in range(E3) if i <= inv3[i]) == len(want), f"{what}: a K-mer lies on two canonical hb3 edges"
    # 4. inv3
    twin = {}
    for i in range(E3):
        j = int(inv3[i])
        assert 0 <= j < E3 and int(inv3[j]) == i, f"{what}: inv3 is no involution at {i}"
        assert edges3[j] == go.rc_seq(edges3[i]), f"{what}: hb3 edge inv3[{i}] is not its reverse complement"
        for v, w in ((int(to_right3[i]), int(to_left3[j])), (int(to_left3[i]), int(to_right3[j]))):
            assert twin.setdefault(v, w) == w and twin.setdefault(w, v) == v, f"{what}: the ends of hb3 edge {i} and its inverse do not pair up"
    # 5. vertex ends
    ends = {}
    for i in range(E3):
        for v, k in ((int(to_left3[i]), edges3[i][:K - 1]), (int(to_right3[i]), edges3[i][-(K - 1):])):
            assert ends.setdefault(v, k) == k, f"{what}: hb3 edge {i} disagrees with vertex {v}'s K - 1 bases"
    assert len(set(ends.values())) == len(ends), f"{what}: two hb3 vertices with the same K - 1 bases"
    # 6. the inverse route
    for e in range(E):
        assert [int(x) for x in to3[g["inv"][e]]] == [int(inv3[x]) for x in reversed(to3[e])], f"{what}: the path of inv[{e}] is not {e}'s reversed through inv3"


def invariants_of_result(g, closures, r, what=""):
    """check_invariants on a result of patch_oracle.run"""
    check_invariants(g, closures, r["hbv"].edges, r["inv3"], r["to_left3"], r["to_right3"], r["to3"], r["left3"], r["kmers3"], what)


def seeded_case(K, seed):
    g = patch_cases.graph_of(small_zoo(K, seed), K)
    return g, closures_for(g, np.random.default_rng([seed, K, 7003]), 2)
