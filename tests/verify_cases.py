"""tests/verify_cases.py -- TEST INFRASTRUCTURE: damaged paths and reads for the path verifier, in one place.

The reference-written fixtures hold correct paths only, so on them the verifier's hard counters (broken, no_anchor) are 0 whether
or not the verifier can count at all.  Every function here takes a fixture's (paths, reads, edges, to_left, to_right, inv, K) --
verify_oracle.load_graph_dir, decode_paths, paths_oracle.unpack_reads -- and returns (name, paths', reads', n_damaged): the same
set with ONE kind of damage, chosen so that what the verifier must answer follows from the damage alone (the last column of the
table in DESIGN.md section 15).  Pure Python, deterministic, no randomness: tests/test_verify_oracle.py pins the CPU verifier
(oracle/verify_oracle.py) on them, tests/test_gpu_verify_damaged.py the device's (k_path_verify) against it.

A path is (offset, [edge ids]); a read is its base codes as bytes.  Nothing is changed in place."""
import numpy as np

INT32_MIN, INT32_MAX = -(1 << 31), (1 << 31) - 1

# (directory under tests/golden, K, the read set's name for tests.test_paths_oracle.load_reads)
FIXTURES = [("graph_k48", 48, "reads"), ("graph_k40_nobc", 40, "reads"), ("graph_k60_nobc", 60, "reads"), ("graph_frag_k48", 48, "frag")]
# graph_k60_nobc has 3 paths of two edges: the classes that need a second edge prove nothing there
MULTI_EDGE_FIXTURES = ("graph_k48", "graph_k40_nobc", "graph_frag_k48")


def _placed(paths):
    return [i for i, (_, p) in enumerate(paths) if p]


def _nk(edges, K):
    return [len(s) - K + 1 for s in edges]


def offset_plus_one(paths, reads, edges, to_left, to_right, inv, K):
    """every 3rd placed read's offset + 1: its k-mers are no longer where the path says (a few reach the edge's end: broken)"""
    out, hit = list(paths), _placed(paths)[::3]
    for i in hit:
        out[i] = (paths[i][0] + 1, paths[i][1])
    return "offset+1", out, reads, len(hit)


def offset_at_n(paths, reads, edges, to_left, to_right, inv, K):
    """every 4th placed read's offset set to the k-mer count n of its first edge (even ones of those: behind the edge, broken) or
    to n - 1 (odd ones: the last place on it, not broken): the boundary of `offset >= n`"""
    nk, out, hit = _nk(edges, K), list(paths), _placed(paths)[::4]
    for k, i in enumerate(hit):
        out[i] = (nk[paths[i][1][0]] - (k & 1), paths[i][1])
    return "offset at n", out, reads, len(hit)


def n_set_to_n(n_damaged):
    """of offset_at_n's damaged reads, those whose offset is n itself"""
    return (n_damaged + 1) // 2


def offset_extremes(paths, reads, edges, to_left, to_right, inv, K):
    """every 4th placed read's offset in turn INT32_MIN, INT32_MAX, -(its read's length): the middle one lies behind any edge
    (broken); the other two put every k-mer in front of the path (outside, so no anchor) -- unless offset + position wraps"""
    out, hit = list(paths), _placed(paths)[1::4]
    for k, i in enumerate(hit):
        out[i] = ((INT32_MIN, INT32_MAX, -len(reads[i]))[k % 3], paths[i][1])
    return "offset extremes", out, reads, len(hit)


def n_set_to_max(n_damaged):
    """of offset_extremes' damaged reads, those set to INT32_MAX"""
    return (n_damaged + 1) // 3


def edge_to_inv(paths, reads, edges, to_left, to_right, inv, K):
    """the second edge of every other multi-edge path replaced by its involution, where that does not leave the vertex the first
    edge enters (it never does but on a hairpin): two consecutive edges that do not meet"""
    out, hit = list(paths), []
    multi = [i for i in _placed(paths) if len(paths[i][1]) >= 2 and to_right[paths[i][1][0]] != to_left[inv[paths[i][1][1]]]]
    for i in multi[::2]:
        p = list(paths[i][1]); p[1] = inv[p[1]]
        out[i] = (paths[i][0], p); hit.append(i)
    return "edge -> inv", out, reads, len(hit)


def sibling(paths, reads, edges, to_left, to_right, inv, K):
    """the last edge of a multi-edge path replaced by another edge that leaves the same vertex, where there is one: the edges still
    meet (the test reads vertices, not ids), the read's k-mers on that edge are no longer where the path says"""
    leaving = {}
    for e, v in enumerate(to_left):
        leaving.setdefault(v, []).append(e)
    out, n = list(paths), 0
    for i in _placed(paths):
        p = paths[i][1]
        if len(p) < 2:
            continue
        others = [g for g in leaving[to_left[p[-1]]] if g != p[-1]]
        if others:
            out[i] = (paths[i][0], p[:-1] + [others[0]]); n += 1
    return "sibling", out, reads, n


def id_out_of_range(paths, reads, edges, to_left, to_right, inv, K):
    """every 5th placed read gets an edge id outside the graph -- E and -1 alternately -- first or last in its path, alternately
    by pairs: caught at the edge itself (j == 0) or as the successor of a good edge (j + 1)"""
    E, out, hit = len(edges), list(paths), _placed(paths)[::5]
    for k, i in enumerate(hit):
        p = list(paths[i][1]); p[0 if (k >> 1) & 1 == 0 else -1] = E if k & 1 == 0 else -1
        out[i] = (paths[i][0], p)
    return "id out of range", out, reads, len(hit)


def id_behind_a_good_edge(paths, reads, edges, to_left, to_right, inv, K):
    """EVERY multi-edge path's last edge gets an id outside the graph (E and -1 alternately): its first edges are good, so this is
    caught where the verifier looks at the successor (j + 1) and nowhere else"""
    E, out, n = len(edges), list(paths), 0
    for i in _placed(paths):
        if len(paths[i][1]) >= 2:
            out[i] = (paths[i][0], paths[i][1][:-1] + [E if n & 1 == 0 else -1]); n += 1
    return "id at j+1", out, reads, n


def lengthened(paths, reads, edges, to_left, to_right, inv, K):
    """single-edge paths extended along the graph by up to 8 successors that DO meet (the lowest-numbered edge leaving the vertex
    reached): nothing is broken, the path is longer than any fixture's (4 edges), what lay behind its end is now on it"""
    leaving = {}
    for e, v in enumerate(to_left):
        leaving.setdefault(v, []).append(e)
    out, n = list(paths), 0
    for i in _placed(paths):
        p = list(paths[i][1])
        if len(p) != 1:
            continue
        while len(p) < 9 and leaving.get(to_right[p[-1]]):
            p.append(leaving[to_right[p[-1]]][0])
        if len(p) > 1:
            out[i] = (paths[i][0], p); n += 1
    return "lengthened", out, reads, n


def short_read(paths, reads, edges, to_left, to_right, inv, K):
    """every 7th placed read cut to K - 1 bases, its path kept: a placed read without one k-mer"""
    out, hit = list(reads), _placed(paths)[::7]
    for i in hit:
        out[i] = reads[i][:K - 1]
    return "short read", paths, out, len(hit)


def other_reads(paths, reads, edges, to_left, to_right, inv, K):
    """the paths against other reads: read i is the MATE of the read one pair on (rotated by a pair, mates swapped)"""
    n = len(reads)
    return "other reads", paths, [reads[((i ^ 1) + 2) % n] for i in range(n)], n


def unplaced(paths, reads, edges, to_left, to_right, inv, K):
    """every path emptied"""
    return "unplaced", [(0, [])] * len(paths), reads, len(_placed(paths))


def no_reads(paths, reads, edges, to_left, to_right, inv, K):
    """n_reads == 0"""
    return "no reads", [], [], len(paths)


CLASSES = {f.__name__: f for f in (offset_plus_one, offset_at_n, offset_extremes, edge_to_inv, sibling, id_out_of_range, id_behind_a_good_edge,
                                   lengthened, short_read, other_reads, unplaced, no_reads)}
NEED_SECOND_EDGE = ("edge_to_inv", "sibling", "id_behind_a_good_edge", "lengthened")
CHANGE_NO_PATH = ("short_read", "other_reads")
CASES = [(fx, cl) for fx, _, _ in FIXTURES for cl in CLASSES if fx in MULTI_EDGE_FIXTURES or cl not in NEED_SECOND_EDGE]

_loaded = {}


def load(golden_dir, fixture):
    """-> dict(K, paths, reads, edges, to_left, to_right, inv, rs): the fixture as the classes take it, rs the read set as the
    library takes it.  Loaded once; nobody changes it."""
    import os
    from oracle import paths_oracle, verify_oracle
    from tests.test_paths_oracle import decode_paths, load_reads
    if fixture not in _loaded:
        K, which = next((k, w) for f, k, w in FIXTURES if f == fixture)
        d = os.path.join(golden_dir, fixture)
        edges, left, right, inv = verify_oracle.load_graph_dir(d, K)
        rs = load_reads(golden_dir, which)
        _loaded[fixture] = dict(K=K, paths=decode_paths(open(os.path.join(d, "a.paths"), "rb").read()), reads=paths_oracle.unpack_reads(rs)[0],
                                edges=edges, to_left=left, to_right=right, inv=inv, rs=rs)
    return _loaded[fixture]


def damaged(golden_dir, fixture, cls):
    """-> (name, paths', reads', n_damaged) of one class on one fixture"""
    f = load(golden_dir, fixture)
    return CLASSES[cls](f["paths"], f["reads"], f["edges"], f["to_left"], f["to_right"], f["inv"], f["K"])


def pack_reads(reads):
    """base codes as bytes -> (packed u8, base_off u64[n + 1], read_len u32[n]) as the library takes reads: four bases a byte, the
    first in the low bits, every read on a byte of its own"""
    lens = np.array([len(r) for r in reads], np.uint32)
    sizes = (lens.astype(np.uint64) + np.uint64(3)) // np.uint64(4)
    base_off = np.zeros(len(reads) + 1, np.uint64)
    base_off[1:] = np.cumsum(sizes, dtype=np.uint64)
    packed = np.zeros(int(base_off[-1]), np.uint8)
    for r, at in zip(reads, base_off[:-1]):
        c = np.zeros((len(r) + 3) // 4 * 4, np.uint8); c[:len(r)] = np.frombuffer(r, np.uint8)
        c = c.reshape(-1, 4)
        packed[int(at):int(at) + len(c)] = c[:, 0] | (c[:, 1] << 2) | (c[:, 2] << 4) | (c[:, 3] << 6)
    return packed, base_off, lens


if __name__ == "__main__":                                   # python -m tests.verify_cases: the table of tests/test_verify_oracle.py
    import os
    from oracle import verify_oracle
    g = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
    for fx, cl in CASES:
        f = load(g, fx)
        name, p, r, n = damaged(g, fx, cl)
        print(f'    ("{fx}", "{cl}"): ({n}, {verify_oracle.verify(f["edges"], f["to_left"], f["to_right"], p, r, f["K"])}),')
