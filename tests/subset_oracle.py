"""The patching stage's subset of interest (StagePatch, 10X/runstages/RunStages.cc:208-254) restated in numpy, and the four files
a.sub.ids / a.sub.eoi / a.sub.paths / a.sub.paths.inv of dfk_subset_write.

What is pinned on what: the CHOICE of ids and edges is a restatement of the rule (this module; superplus_amd/csrc/dfk_subset.h restates it
a second time, independently).  The two feudal subsets are not restated: they are made by SLICING an a.paths and an a.paths.inv --
element bytes by the files' own offset tables, control block copied -- so where the fixture holds the reference-written file (a.paths:
every fixture; a.paths.inv: graph_frag_k48, graph_pathy2_k48) the expected bytes are the reference's own.  For the other fixtures'
index and for seeded inputs the source files come from oracle/paths_oracle.py (paths_file, paths_index), which
tests/test_paths_oracle.py pins on reference-written bytes.

  in_pairs (:213-219)  x in {first, second, inv[first], inv[second]} over the pairs
  eoi (:222-226)       the marked edges, ascending; a vec<size_type>, size_type = size_t (system/Types.h:126): 8 bytes in the file
  read_ids (:228-241)  both reads of every pair of which either read's path holds a marked edge, ascending
  subsets (:253-254)   SubsetMasterVec::build (feudal/SubsetMasterVec.h:29-38): push_back( src.at( id ) ) over the sorted ids"""
import os
import struct

import numpy as np

SALT_IDS, SALT_EOI = 0x7777, 0x8888
FILES = ("a.sub.ids", "a.sub.eoi", "a.sub.paths", "a.sub.paths.inv")


def mark_edges(pairs, inv):
    m = np.zeros(len(inv), bool)
    for a, b in pairs:
        m[a] = m[b] = m[inv[a]] = m[inv[b]] = True
    return m


def bin_file(values):
    """BinaryWriter::writeFile of a vec<uint64_t> (feudal/BinaryStream.h:447-462)"""
    a = np.asarray(values, "<u8")
    return b"BINWRITE" + struct.pack("<Q", len(a)) + a.tobytes()


def feudal_elements(b):
    """a feudal file with no fixed data -> (control block, [element bytes])"""
    n = int.from_bytes(b[:4], "little")
    var_tab = int.from_bytes(b[8:16], "little")
    offs = np.frombuffer(b, "<u8", n + 1, var_tab)
    return b[:24], [b[int(offs[i]):int(offs[i + 1])] for i in range(n)]


def slice_feudal(b, ids):
    """the file SubsetMasterVec( source, ids ) would write: the source's control block with n = len(ids), element k = the bytes of
    element ids[k], absolute offsets"""
    head, elems = feudal_elements(b)
    var = b"".join(elems[int(i)] for i in ids)
    offs = np.concatenate([[0], np.cumsum([len(elems[int(i)]) for i in ids])]).astype(np.uint64) + np.uint64(24)
    var_tab = 24 + len(var)
    return struct.pack("<I", len(ids)) + head[4:8] + struct.pack("<QQ", var_tab, var_tab + 8 * (len(ids) + 1)) + var + offs.astype("<u8").tobytes()


def _mix(x):
    x = x ^ (x >> np.uint64(30)); x = x * np.uint64(0xBF58476D1CE4E5B9)
    x = x ^ (x >> np.uint64(27)); x = x * np.uint64(0x94D049BB133111EB)
    return x ^ (x >> np.uint64(31))


def seq_digest(values, salt):
    """k_digest_seq: (sum, xor) over positions i of h = mix(mix(i + salt) ^ v[i])"""
    v = np.asarray(values, np.uint64)
    with np.errstate(over="ignore"):
        h = _mix(_mix(np.arange(len(v), dtype=np.uint64) + np.uint64(salt)) ^ v)
        x = _mix(h + np.uint64(0xD1B54A32D192ED03))
        return int(h.sum(dtype=np.uint64)), (int(np.bitwise_xor.reduce(x)) if len(x) else 0)


def run(paths, inv, pairs, paths_bytes=None, index_bytes=None):
    """paths [[edge ids]] per read, inv per edge, pairs [(e1, e2)]; paths_bytes / index_bytes: the a.paths and a.paths.inv to slice
    (None: made by oracle/paths_oracle.py, every offset 0) -> dict(eoi, ids, files {name: bytes}, the counters, the digests)"""
    from oracle import paths_oracle
    paths = [list(p) for p in paths]
    inv = [int(x) for x in inv]
    N = len(paths)
    assert N % 2 == 0
    m = mark_edges(pairs, inv)
    eoi = [e for e in range(len(inv)) if m[e]]
    hit = [any(m[e] for e in p) for p in paths]
    ids, one = [], 0
    for i in range(N // 2):
        if hit[2 * i] or hit[2 * i + 1]:
            ids += [2 * i, 2 * i + 1]
            one += hit[2 * i] != hit[2 * i + 1]
    with_off = [(0, p) for p in paths]
    if paths_bytes is None: paths_bytes = paths_oracle.paths_file(with_off)
    if index_bytes is None: index_bytes = paths_oracle.paths_index(with_off, inv)["a.paths.inv"]
    files = {"a.sub.ids": bin_file(ids), "a.sub.eoi": bin_file(eoi), "a.sub.paths": slice_feudal(paths_bytes, ids), "a.sub.paths.inv": slice_feudal(index_bytes, eoi)}
    lists = feudal_elements(files["a.sub.paths.inv"])[1]
    return dict(eoi=eoi, ids=ids, files=files, path_entries=sum(len(paths[i]) for i in ids), all_entries=sum(len(p) for p in paths),
                index_entries=sum(len(l) // 8 for l in lists), index_first=[0] + [int(x) for x in np.cumsum([len(l) // 8 for l in lists])],
                one_read_only=int(one), unplaced=sum(1 for i in ids if not paths[i]),
                twice=sum(1 for i in ids if any(paths[i].count(e) > 1 for e in set(paths[i]) if m[e])),
                ids_digest=seq_digest(ids, SALT_IDS), eoi_digest=seq_digest(eoi, SALT_EOI))


_cache = {}


def fixture_subset(golden_dir, case, K, which):
    """run() on a fixture with tests/hops_oracle.py's pairs (ONE_GOOD off), slicing the fixture's own files; computed once per session and
    handed out unchanged"""
    if case not in _cache:
        from tests.test_hops_oracle import fixture_hops, fixture_inputs
        i = fixture_inputs(golden_dir, case, K, which)
        rd = lambda f: open(os.path.join(golden_dir, case, f), "rb").read() if os.path.exists(os.path.join(golden_dir, case, f)) else None
        pb = rd("a.paths")
        index = rd("a.paths.inv")
        if index is None:                                        # (no reference-written index in this fixture: the pinned restatement's)
            from oracle import paths_oracle
            from tests.test_paths_oracle import decode_paths
            index = paths_oracle.paths_index(decode_paths(pb), [int(x) for x in i["inv"]])["a.paths.inv"]
        r = run(i["paths"], i["inv"], fixture_hops(golden_dir, case, K, which)["pairs"], pb, index)
        r["pairs"] = fixture_hops(golden_dir, case, K, which)["pairs"]
        r["reference_index"] = rd("a.paths.inv") is not None
        _cache[case] = r
    return _cache[case]
