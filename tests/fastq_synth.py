"""Seeded synthetic stLFR fastq.gz pairs for the ParseBarcodedFastqs tests (names "@id#b1_b2_b3/1<TAB>...", barcode
0_0_0 = unbarcoded; split_barcode_PEXXX_42_unsort_reads.pl's format).  Harness only."""
import gzip
import hashlib

import numpy as np


def case_name(n_pairs, seed, n_bc, ragged, extra):
    """The key of make_fastq(n_pairs, seed, n_bc, ragged) run with the arguments `extra` in tests/golden/pbf_ref.json."""
    return f"p{n_pairs}_s{seed}_bc{n_bc}" + ("_ragged" if ragged else "") + "".join("_" + e for e in extra)


def fastq_digest(path1, path2):
    """SHA-256 of the two files' text (not of the .gz bytes: gzip stamps the time)."""
    h = hashlib.sha256()
    for p in (path1, path2):
        with gzip.open(p, "rb") as f:
            h.update(f.read())
    return h.hexdigest()


def edge_case_name(profile, seed, extra):
    """The key of make_fastq_edges(profile, seed) run with the arguments `extra` in tests/golden/pbf_ref.json."""
    return f"edges_{profile}_s{seed}" + "".join("_" + e for e in extra)


def cut_fastq(src1, src2, dst1, dst2, n_pairs):
    """The first n_pairs records of a pair of fastq.gz files."""
    for src, dst in ((src1, dst1), (src2, dst2)):
        with gzip.open(src, "rt") as f, gzip.open(dst, "wt") as g:
            for _ in range(4 * n_pairs):
                g.write(f.readline())


def read_fastq_pairs(path1, path2):
    """-> [(barcode, read 1, read 2, qualities 1, qualities 2)] in file order: barcode as the program numbers it
    (b1 * 1537^2 + b2 * 1537 + b3), reads as text, qualities as lists of integers."""
    out = []
    with gzip.open(path1, "rt") as f1, gzip.open(path2, "rt") as f2:
        while True:
            name = f1.readline()
            if not name:
                break
            s1 = f1.readline().rstrip("\n"); f1.readline(); q1 = f1.readline().rstrip("\n")
            f2.readline(); s2 = f2.readline().rstrip("\n"); f2.readline(); q2 = f2.readline().rstrip("\n")
            b = [int(x) for x in name.split("#")[1].split("/")[0].split("_")]
            out.append((b[0] * 1537 * 1537 + b[1] * 1537 + b[2], s1, s2, [ord(c) - 33 for c in q1], [ord(c) - 33 for c in q2]))
    return out


_SHORT = (1, 2, 3, 4, 5, 49, 100, 254, 255, 256)
_LONG = _SHORT + (257, 300, 511, 512, 513, 1000)
# profile -> the lengths of the random reads and of the base read of a family, per file
EDGE_PROFILES = {
    "lds_edge": {"lengths": (_SHORT, _SHORT), "base": ((1, 2, 3, 5, 49, 100, 250, 251),) * 2},
    "long": {"lengths": (_LONG, _LONG), "base": ((1, 3, 49, 100, 251, 255, 256, 488),) * 2},
    "long_one_file": {"lengths": ((1, 2, 3, 4, 5, 49, 100, 151), _LONG), "base": ((1, 2, 3, 5, 49, 100, 145, 146), (1, 3, 49, 100, 251, 255, 256, 488))},
}
_TWO_LEVEL_STEPS = (1, 2, 3, 4, 5, 8, 9, 16, 17, 32, 33, 63)


def _edge_quals(rng, n):
    """One of six patterns of n qualities in 0..63 (see make_fastq_edges)."""
    kind = int(rng.integers(0, 6))
    if kind == 0:
        return rng.integers(0, 64, n)
    if kind == 1:
        return np.full(n, int(rng.choice([0, 63, int(rng.integers(0, 64))])))
    if kind == 2:
        r = int(rng.choice(_TWO_LEVEL_STEPS)); a = int(rng.integers(0, 64 - r))
        q = a + r * rng.integers(0, 2, n)
        q[0] = a
        q[-1] = a + r                                                     # (a read of one value keeps a + r)
        return q
    if kind == 3:
        return (np.arange(n) + int(rng.integers(0, 64))) % 64
    if kind == 4:
        q = np.full(n, int(rng.integers(0, 64)))
        for j in rng.integers(0, n, 1 + n // 80):
            q[j] = int(rng.integers(0, 64))
        return q
    q = np.empty(n, dtype=np.int64)
    i = 0
    v = int(rng.integers(0, 64))
    while i < n:
        run = int(rng.choice([255, 256, 510]))
        q[i:i + run] = v
        i += run
        v = (v + int(rng.integers(1, 64))) % 64
    return q


def make_fastq_edges(path1, path2, seed, profile):
    """The inputs make_fastq never makes (same names; 8 barcodes, a tenth of the pairs unbarcoded; a few hundred pairs):
      lengths     1 to 5, 49, 100, 254 to 256 in `lds_edge` (the longest read is exactly 256); up to 1000 in both files in
                  `long`; file 1 at most 151 and file 2 up to 1000 in `long_one_file`.  In `long` the unbarcoded pairs hold reads
                  of at most 256 only: done in groups of buckets (MAX_MEM_GB) they are a group whose qualities are planned in LDS.
      families    in one barcode, for read 1 with read 2 held equal and the other way round: a read X, X cut short, X + A..A
                  and X + N..N (1 to 5), X + A..A + C, copies -- and in the long profiles, where the file allows 1000 bases,
                  X + 256 A and X + 512 N -- dealt to random places of the file.  Only the lengths order such pairs.
      qualities   per read one of: uniform in 0..63; constant (0 and 63 among them); two levels a and a + r; a ramp 0..63
                  repeated; a constant with single spikes; constant runs of 255, 256 and 510 values.
    No line is longer than 1000 characters and no read is empty."""
    P = EDGE_PROFILES[profile]
    rng = np.random.default_rng(seed)
    n_bc = 8
    long_profile = profile != "lds_edge"
    bases = lambda n: "".join("ACGT"[x] for x in rng.integers(0, 4, n))
    recs = []                                                                 # (barcode number k, 0 = unbarcoded; read 1; read 2)
    for _ in range(360 if long_profile else 420):
        k = 0 if rng.random() < 0.1 else int(rng.choice(np.arange(1, n_bc + 1), p=np.array([3, 1, 4, 1, 5, 2, 2, 2]) / 20))
        s = []
        for f in (0, 1):
            choice = [l for l in P["lengths"][f] if l <= 256] if profile == "long" and k == 0 else P["lengths"][f]
            x = bases(int(rng.choice(choice)))
            if rng.random() < 0.1:
                j = int(rng.integers(0, len(x))); x = x[:j] + "N" + x[j + 1:]
            s.append(x)
        recs.append((k, s[0], s[1]))
    for f in (0, 1):
        top = max(P["lengths"][f])
        for lx in P["base"][f]:
            k = int(rng.integers(1, n_bc + 1))
            X = bases(lx)
            other = bases(int(rng.choice([l for l in P["lengths"][1 - f] if l >= 3])))
            js = sorted(int(j) for j in rng.choice(np.arange(1, 6), 3, replace=False))
            members = [X] * int(rng.integers(2, 4))
            if lx >= 2:
                members.append(X[:int(rng.integers(1, lx))])
            for j in js:
                members += [X + "A" * j, X + "N" * j]
            members.append(X + "A" * js[1] + "C")
            if lx + 256 <= top:
                members.append(X + "A" * 256)
            if lx + 512 <= top:
                members.append(X + "N" * 512)
            for m in members:
                recs.insert(int(rng.integers(0, len(recs) + 1)), (k, m, other) if f == 0 else (k, other, m))
    with gzip.open(path1, "wt") as f1, gzip.open(path2, "wt") as f2:
        for i, (k, s1, s2) in enumerate(recs):
            b = (k % 7 + 1, (k * 13) % 1500 + 1, (k * 101) % 1536 + 1) if k else (0, 0, 0)
            for f, mate, s in ((f1, 1, s1), (f2, 2, s2)):
                q = _edge_quals(rng, len(s))
                f.write(f"@r{i}#{b[0]}_{b[1]}_{b[2]}/{mate}\t{i}\t1\n{s}\n+\n{''.join(chr(33 + int(x)) for x in q)}\n")


def make_fastq(path1, path2, n_pairs, seed, n_bc=40, L=100, ragged=False):
    rng = np.random.default_rng(seed)
    G = rng.integers(0, 4, 5000)
    prev = None
    with gzip.open(path1, "wt") as f1, gzip.open(path2, "wt") as f2:
        for i in range(n_pairs):
            if rng.random() < 0.12:
                b = (0, 0, 0)
            else:
                k = int(rng.integers(1, n_bc + 1)); b = (k % 7 + 1, (k * 13) % 1500 + 1, (k * 101) % 1536 + 1)
            cur = {}
            for f, mate in ((f1, 1), (f2, 2)):
                l = int(rng.choice([L, L, L, 75, 151, 49])) if ragged else L
                pos = int(rng.integers(0, len(G) - l))
                s = "".join("ACGT"[x] for x in G[pos:pos + l])
                if rng.random() < 0.1:
                    j = int(rng.integers(0, l)); s = s[:j] + "N" + s[j + 1:]
                if rng.random() < 0.3 and prev is not None:
                    s = prev[mate]                                        # duplicates: ties in the per-barcode sort
                q = rng.choice([37, 37, 37, 30, 25, 12, 2], len(s))
                if rng.random() < 0.3:
                    q[:] = 35
                if rng.random() < 0.3:
                    q[-int(rng.integers(1, 20)):] = 2
                f.write(f"@r{i}#{b[0]}_{b[1]}_{b[2]}/{mate}\t{i}\t1\n{s}\n+\n{''.join(chr(33 + int(x)) for x in q)}\n")
                cur[mate] = s
            prev = cur
