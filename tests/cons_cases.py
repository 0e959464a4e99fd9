"""Seeded inputs of the stack consensus (tests/cons_oracle.py): small graphs with chosen closer tables, partner records, pairs, reads
and qualities, for tests/cpp/test_cons.cc (recorded in tests/cpp/cons_cases.txt: the C++ restatement of superplus_amd/csrc/dfk_cons.h
against the Python one) and for tests/test_gpu_cons.py (dfk_cons_build_arrays).  `python -m tests.cons_cases` rewrites the recorded
file.

The stage takes locs as dfk_closer_fetch gives them and the partners as dfk_partners_fetch gives them, so a case chooses both directly.
`planted` holds what the fixtures lack, each on a closer edge of its own (K = 48, so an edge of k k-mers has ne = k + 47 bases; edges
2 x and 2 x + 1 are each other's involution, the last edge its own); pair x is (E_x, inv[F]) with F an edge without rows, so that side 0
is stack E_x unreversed and side 1 the empty stack F reversed, unless said otherwise:
   ROUND   eight forward rows of two bases at pos 0.  Column 0: base 0 with Q2, Q10, Q10 then base 1 with Q20, Q0, Q0 (rows 6, 7: Q128 and
           Q130, undefined): 20.2 against 20.200000000000003 -- base 1, where exact tenths tie and give base 0.  Column 1: base 1 with
           Q2, Q37, Q10, Q0 then base 0 with Q0, Q2, Q10, Q37: 47.300000000000004 against 47.3 -- base 1, where sums in another order tie.
   TIE     pair (TIE, inv[TIE]): es = {TIE, TIE}, both sides reversed.  Two forward rows at pos 0: bases 0 1 2 and 3 1 0 at Q10, a third
           row at pos 5: column 0 ties 0 with 3, columns 3 and 4 are empty: reversed they give base 0, not the complement's 3.
   M400    a forward row of 100 bases at pos 300 (M = 400: no trim) beside a forward row wholly at negative columns (pos -200, 100 bases:
           not live, yet kept) and a non-forward row at pos ne - 3 whose bases run off column 0.
   M401    the read of 401 bases forward at pos 0 (M = 401: one column trimmed) over a row of 1 base at pos 0 (outside the window: erased),
           a row of 100 bases at pos 0 whose qualities are 127 where the window begins and 128 from there on, the same read again at pos 250
           (two rows, one read), and that read once more as a partner row.
   LONG    ne = 1047: non-forward rows at pos 0 .. (M = 1047), forward rows far in front of the window (erased).
   S       the self-inverse edge, pair (S, S): both sides the same edge, both reversed.
   (ROUND, inv[M400])   a pair of two stacks with rows; given twice, and once more as (M400, inv[ROUND]): the pair reversed.
Qualities: feudal.pq_encode holds a block's least quality in six bits and its range in seven: 127 and 128 fit, 255 does not -- the
largest a valid stream can hold beside a quality of 63 is 190, and that is what the cases use."""
import os

import numpy as np

from superplus_amd import feudal
from tests import cons_oracle
from tests.closer_oracle import closer_edges, loc_words
from tests.partners_cases import pack

FILE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "cpp", "cons_cases.txt")
K = 48

# name, seed, edges, reads, pairs, planted, recorded
SPECS = [("planted", 1, 0, 0, 0, True, True), ("random", 2, 14, 60, 10, False, True), ("random-long", 3, 10, 40, 8, False, True), ("no-pairs", 4, 6, 10, 0, False, True),
         ("many-rows", 5, 4, 300, 2, False, False),               # a stack of more rows than two tiles of device_scan (2 x 2048)
         ("many-stacks", 6, 12, 80, 2100, False, False)]          # more stacks than two tiles


def rand_bases(rng, n):
    return rng.randint(0, 4, size=n).astype(np.uint8)


def rand_quals(rng, n):
    return rng.choice(np.array([0, 1, 2, 10, 10, 20, 37, 37, 41], np.uint8), size=n)


def planted():
    rng = np.random.RandomState(11)
    names = ["ROUND", "TIE", "M400", "M401", "LONG", "F"]
    edge = {n: 2 * i for i, n in enumerate(names)}
    E = 2 * len(names) + 1
    S = E - 1
    inv = [e ^ 1 for e in range(E - 1)] + [S]
    kmers = [10] * E
    kmers[edge["LONG"]] = 1000; kmers[edge["M400"]] = 200; kmers[edge["M401"]] = 300
    ne = lambda n: kmers[edge[n]] + K - 1
    reads, quals = [], []

    def read(b, q):
        reads.append(np.asarray(b, np.uint8)); quals.append(np.asarray(q, np.uint8))
        reads.append(rand_bases(rng, 7)); quals.append(rand_quals(rng, 7))        # its mate
        return len(reads) - 2
    locs = {n: [] for n in names + ["S"]}
    # ROUND
    col0 = [(0, 2), (0, 10), (0, 10), (1, 20), (1, 0), (1, 0), (2, 128), (3, 130)]
    col1 = [(1, 2), (1, 37), (1, 10), (1, 0), (0, 0), (0, 2), (0, 10), (0, 37)]
    for (b0, q0), (b1, q1) in zip(col0, col1): locs["ROUND"].append((read([b0, b1], [q0, q1]), 0, True))
    # TIE
    locs["TIE"] = [(read([0, 1, 2], [10] * 3), 0, True), (read([3, 1, 0], [10] * 3), 0, True), (read([2, 2, 1], [37, 2, 1]), 5, True)]
    # M400
    r100 = read(rand_bases(rng, 100), rand_quals(rng, 100))
    locs["M400"] = [(r100, 300, True), (read(rand_bases(rng, 100), rand_quals(rng, 100)), -200, True), (read(rand_bases(rng, 10), rand_quals(rng, 10)), ne("M400") - 3, False)]
    # M401
    r401 = read(rand_bases(rng, 401), rand_quals(rng, 401))
    q = np.full(100, 63, np.uint8); q[1] = 127; q[2:] = np.where(np.arange(98) % 2 == 0, 128, 190); q[50] = 63
    r_edge = read(rand_bases(rng, 100), q)
    r1 = read([2], [30])
    locs["M401"] = [(r1, 0, True), (r_edge, 0, True), (r401, 0, True), (r_edge, 250, True)]
    # LONG
    locs["LONG"] = [(read(rand_bases(rng, 151), rand_quals(rng, 151)), 10 * i, True) for i in range(3)] + \
                   [(read(rand_bases(rng, 120), rand_quals(rng, 120)), 7 * i, False) for i in range(4)] + [(r100, 40, False)]
    locs["S"] = [(read(rand_bases(rng, 60), rand_quals(rng, 60)), -5, True), (read(rand_bases(rng, 60), rand_quals(rng, 60)), 3, False)]
    F = edge["F"]
    pairs = [(edge[n], inv[F]) for n in ("ROUND", "M400", "M401", "LONG")] + [(edge["TIE"], inv[edge["TIE"]]), (S, S)]
    pairs += [(edge["ROUND"], inv[edge["M400"]])] * 2 + [(edge["M400"], inv[edge["ROUND"]])]
    edge["S"] = S
    ce = closer_edges(pairs, inv)
    per = [next((locs[n] for n in locs if edge[n] == e), []) for e in ce]
    for rows in per: rows.sort(key=lambda r: (not r[2],))               # (the forward records first, as the closer gives them; the order inside kept)
    parts = [[] for _ in range(2 * len(pairs))]
    parts[2 * 2 + 1] = [(r_edge, 280, True), (r100 + 1, 394, True)]     # pushed by side 1 of pair 2 onto locs[0]: stack M401
    parts[2 * 6 + 0] = parts[2 * 7 + 0] = parts[2 * 8 + 1] = [(r1, 1, True)]      # pushed by ROUND's side of pairs 6, 7 and 8 onto the other's locs: stack M400
    return dict(inv=inv, kmers=kmers, ce=ce, locs=per, parts=parts, pairs=pairs, reads=reads, quals=quals, edge=edge)


def make(seed, E, N, n_pairs, name):
    rng = np.random.RandomState(seed)
    if E % 2 == 0: E += 1
    inv = [e ^ 1 for e in range(E - 1)] + [E - 1]
    long_ = name in ("random-long", "many-rows")
    kmers = [int(rng.choice([1, 5, 60, 200, 353, 354, 700] if not long_ else [353, 354, 900, 2500])) for _ in range(E)]
    lens = [0, 1, 30, 100, 151, 250] if name != "many-rows" else [1, 30, 40]
    reads = [rand_bases(rng, int(rng.choice(lens))) for _ in range(N)]
    quals = [rand_quals(rng, len(r)) for r in reads]
    pairs = [(int(rng.randint(E)), int(rng.randint(E))) for _ in range(n_pairs)]
    if 2 <= n_pairs < 100: pairs += [pairs[-1], (inv[pairs[-2][1]], inv[pairs[-2][0]]), (pairs[0][0], inv[pairs[0][0]])]
    ce = closer_edges(pairs, inv)
    per = []
    for k, e in enumerate(ce):
        ne = kmers[e] + K - 1
        n_rows = 5000 if name == "many-rows" and k == 0 else int(rng.randint(0, 4 if name == "many-stacks" else 14)) if N else 0
        fw = sorted(int(x) for x in rng.randint(0, max(1, N), size=n_rows // 2 + n_rows % 2))
        bw = sorted(int(x) for x in rng.randint(0, max(1, N), size=n_rows // 2))
        # positions: mostly near the end of the edge, where the window lies; some far from it, some off either end
        near = lambda: int(ne - rng.randint(0, 420)) if rng.rand() < 0.7 else int(rng.randint(-260, ne + 60))
        per.append([(id, near(), True) for id in fw] + [(id, int(rng.randint(-60, 420)) if rng.rand() < 0.7 else int(rng.randint(-60, ne + 60)), False) for id in bw])
    parts = [[(int(rng.randint(N)), int(rng.randint(-100, 700)), True) for _ in range(int(rng.choice([0, 0, 1, 2])))] if N else [] for _ in range(2 * len(pairs))]
    return dict(inv=inv, kmers=kmers, ce=ce, locs=per, parts=parts, pairs=pairs, reads=reads, quals=quals)


_made = {}


def seeded():
    """[(name, case, recorded)]"""
    if not _made:
        for name, seed, E, N, np_, is_planted, rec in SPECS: _made[name] = (planted() if is_planted else make(seed, E, N, np_, name), rec)
    return [(name, c, rec) for name, (c, rec) in _made.items()]


_oracle = {}


def oracle(name, c):
    if name not in _oracle:
        _oracle[name] = cons_oracle.run(c["inv"], c["kmers"], K, c["ce"], c["locs"], c["parts"], c["pairs"], lambda id: c["reads"][id], lambda id: c["quals"][id], keep_sums=True)
    return _oracle[name]


def pq_of(quals):
    """-> (PQVec bytes, offsets [n + 1]); every stream decodes to what went in"""
    out, off = [], [0]
    for q in quals:
        b = feudal.pq_encode(q)
        assert feudal.pq_decode(b) == [int(x) for x in q]
        out.append(np.frombuffer(b, np.uint8)); off.append(off[-1] + len(b))
    return (np.concatenate(out) if out else np.zeros(0, np.uint8)), np.asarray(off, np.uint64)


def arrays(c):
    """the case as dfk_cons_build_arrays takes it"""
    rp, ro, rl = pack(c["reads"])
    pq, pq_off = (np.asarray(c["pq"], np.uint8), np.asarray(c["pq_off"], np.uint64)) if "pq" in c else pq_of(c["quals"])      # (a fixture's own streams)
    starts = lambda per: np.concatenate([[0], np.cumsum([len(x) for x in per])]).astype(np.uint64)
    return dict(inv=np.asarray(c["inv"], np.int32), kmers=np.asarray(c["kmers"], np.int32), ce=np.asarray(c["ce"], np.uint64), loc_first=starts(c["locs"]),
                locs=loc_words([l for per in c["locs"] for l in per]), part_first=starts(c["parts"]), parts=loc_words([l for per in c["parts"] for l in per]),
                pairs=np.asarray(c["pairs"], np.int32).reshape(-1, 2), read_packed=rp, read_off=ro, read_len=rl, pq=pq, pq_off=pq_off)


def case_text(name, c, r, K_=K):
    """a case and what the oracle says of it, as tests/cpp/test_cons.cc reads it"""
    a = arrays(c)
    row = lambda v: " ".join(str(int(x)) for x in v)
    hexrow = lambda b: bytes(b).hex() or "-"
    return ["case %s %d %d %d %d %d" % (name, len(c["inv"]), len(c["reads"]), len(c["pairs"]), len(c["ce"]), K_), row(c["inv"]), row(c["kmers"]), row(c["ce"]), row(a["loc_first"]),
            row([int(x) for per in c["locs"] for l in per for x in l]), row(a["part_first"]), row([int(x) for per in c["parts"] for l in per for x in l]),
            row([e for p in c["pairs"] for e in p]), row(a["read_len"]), hexrow(a["read_packed"]), row(a["pq_off"]), hexrow(a["pq"]),
            row(r["starts"]), row([x for d in r["dims"] for x in d]), "".join(str(int(b)) for b in r["bases"]) or "-",
            "%d %d %d %d %d %d %d" % (r["rows"], r["live"], r["rows_kept"], r["trimmed"], r["reversed"], r["columns"], r["added"])]


def text(recorded=True):
    out = []
    for name, c, rec in seeded():
        if rec == recorded: out += case_text(name, c, oracle(name, c))
    return "\n".join(out) + "\n"


if __name__ == "__main__":
    open(FILE, "w").write(text())
