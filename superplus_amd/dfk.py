"""ctypes binding of libdfk.so (include/dfk.h) -- the host-side mirror used by tests, bench.py
and the multi-GPU driver.  The library is HIP-only: if it cannot be loaded, or no gfx950
device is usable, everything here raises; there is no CPU fallback.

Reference interface mirrored: createDict(work_dir, reads, quals, minQual, minFreq,
ignBcBelow, mem_frac, minBC, bcp) -- lib/assembly/src/paths/long/BuildReadQGraph48.cc:211-215.
"""
import ctypes as C
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("DFK_LIB") or os.path.join(_HERE, "libdfk.so")      # DFK_LIB: a developer's timing variant (tools/)
ABI_VERSION = 3
F_KEEP_PRE_ADJ = 1
F_KEEP_INPUTS = 2
F_MARK_BADS = 4

ENTRY_DTYPE = np.dtype([("w0", "<u8"), ("w1", "<u8"), ("edge_id", "<u4"), ("count_ctx", "<u4"),
                        ("bc", "<i4"), ("pad", "<u4")])

EXPORTS = [
    "dfk_create", "dfk_destroy", "dfk_last_error", "dfk_abi_version", "dfk_count", "dfk_count_bci", "dfk_count_device",
    "dfk_hint_file_range", "dfk_qual_hist", "dfk_paths_sink", "dfk_good_lens", "dfk_spectrum", "dfk_spectrum_json", "dfk_solid_count", "dfk_solid_fetch", "dfk_solid_fetch_unsorted", "dfk_solid_digest",
    "dfk_write_kvec", "dfk_write_kvec_part", "dfk_get_stats", "dfk_adj_outcome", "dfk_shard_begin", "dfk_shard_begin_host", "dfk_shard_plan", "dfk_shard_partition", "dfk_shard_partition_begin", "dfk_shard_partition_end", "dfk_shard_recv_buffer", "dfk_shard_count", "dfk_shard_adj_queries",
    "dfk_shard_adj_answer", "dfk_shard_adj_apply", "dfk_graph_build", "dfk_graph_stats", "dfk_graph_write",
    "dfk_shard_dict_share", "dfk_shard_dict_adopt", "dfk_shard_dict_whole",
    "dfk_paths_build", "dfk_paths_build_device", "dfk_paths_stats", "dfk_paths_write", "dfk_paths_fetch", "dfk_paths_index_write", "dfk_dups_write", "dfk_paths_index_dups_write",
    "dfk_paths_digest", "dfk_paths_verify", "dfk_paths_verify_device", "dfk_paths_verify_arrays", "dfk_pbf_run", "dfk_pbf_result", "dfk_pbf_free",
    "dfk_paths_var_bytes", "dfk_paths_write_part", "dfk_shard_pidx_pairs", "dfk_shard_pidx_write", "dfk_shard_dup_keys", "dfk_shard_dup_answer", "dfk_shard_dup_write",
    "dfk_bads_sums", "dfk_bads_write", "dfk_bads_write_part",
    "dfk_hops_build", "dfk_hops_build_bci", "dfk_hops_build_arrays", "dfk_hops_stats", "dfk_hops_fetch", "dfk_hops_write",
    "dfk_subset_build", "dfk_subset_build_arrays", "dfk_subset_stats", "dfk_subset_fetch", "dfk_subset_write",
    "dfk_closer_build", "dfk_closer_build_arrays", "dfk_closer_stats", "dfk_closer_fetch", "dfk_closer_write",
    "dfk_partners_build", "dfk_partners_build_arrays", "dfk_partners_stats", "dfk_partners_fetch", "dfk_partners_write",
    "dfk_cons_build", "dfk_cons_build_arrays", "dfk_cons_stats", "dfk_cons_fetch", "dfk_cons_write",
    "dfk_offsets_build", "dfk_offsets_build_arrays", "dfk_offsets_stats", "dfk_offsets_fetch", "dfk_offsets_write",
    "dfk_closures_build", "dfk_closures_build_arrays", "dfk_closures_stats", "dfk_closures_fetch", "dfk_closures_write",
    "dfk_walks_build", "dfk_walks_build_arrays", "dfk_walks_stats", "dfk_walks_fetch", "dfk_walks_write",
    "dfk_scons_build", "dfk_scons_build_arrays", "dfk_scons_stats", "dfk_scons_fetch", "dfk_scons_write",
    "dfk_soffsets_build", "dfk_soffsets_build_arrays", "dfk_soffsets_stats", "dfk_soffsets_fetch", "dfk_soffsets_write",
    "dfk_sclosures_build", "dfk_sclosures_build_arrays", "dfk_sclosures_stats", "dfk_sclosures_fetch", "dfk_sclosures_write", "dfk_allclosures_write",
    "dfk_patch_build", "dfk_patch_build_arrays", "dfk_patch_stats", "dfk_patch_fetch", "dfk_patch_write",
    "dfk_translate_build", "dfk_translate_build_arrays", "dfk_translate_stats", "dfk_translate_fetch", "dfk_translate_write", "dfk_translate_drop",
]

# dfk_paths_digest's words (include/dfk.h, DFK_CK_*) and dfk_paths_verify's counters
CHECK_WORDS = 20
CK = ["PATHS_SUM", "PATHS_XOR", "N_READS", "N_PLACED", "N_PATH_EDGES", "INV_SUM", "INV_XOR", "INV_STARTS", "INV_ENTRIES",
      "COUNTSB_DIGEST", "COUNTSB_SUM", "SELF_INVERSE", "DUP_DIGEST", "DUP_MARKED", "EDGE_KMERS", "N_SOLID", "INV_VIOLATIONS",
      "N_EDGES", "VALID"]
# dfk_hops_stats' words (include/dfk.h, DFK_HOPS_*)
HOPS_WORDS = 16
HOPS = ["m1", "m2", "m3", "pairs", "searched", "extended", "host_edges", "most_rounds", "us", "us_index", "us_m12", "us_m3", "us_host", "largest_x", "ranges"]
# dfk_subset_stats' words (include/dfk.h, DFK_SUBSET_*)
SUBSET_WORDS = 16
SUBSET = ["eoi", "ids", "path_entries", "index_entries", "ranges", "one_read_only", "us", "us_sweep", "us_gather", "us_index",
          "ids_sum", "ids_xor", "eoi_sum", "eoi_xor"]
SUBSET_FILES = ("a.sub.ids", "a.sub.eoi", "a.sub.paths", "a.sub.paths.inv")
# dfk_closer_stats' words (include/dfk.h, DFK_CLOSER_*)
CLOSER_WORDS = 24
CLOSER = ["edges", "locs", "anchors", "reads", "prec", "mates_in", "mates_out", "dup_skipped", "ranges", "us", "us_mark", "us_weigh", "us_sweep", "us_sort",
          "edges_sum", "edges_xor", "locs_sum", "locs_xor", "anchors_sum", "anchors_xor", "reads_sum", "reads_xor"]
CLOSER_FILES = ("a.close.edges", "a.close.locs", "a.close.anchors", "a.close.reads")
# dfk_partners_stats' words (include/dfk.h, DFK_PARTNERS_*)
PARTNERS_WORDS = 20
PARTNERS = ["pairs", "queries", "positions", "entries", "any_hit", "kept", "multi", "batches", "ranges", "us", "us_table", "us_queries", "us_search", "us_copy", "sum", "xor", "searched"]
PARTNERS_FILE = "a.close.partners"
# dfk_cons_stats' words (include/dfk.h, DFK_CONS_*)
CONS_WORDS = 24
CONS = ["pairs", "stacks", "rows", "live", "rows_kept", "trimmed", "reversed", "columns", "cells", "decoded", "batches", "ranges", "us", "us_dims", "us_copy", "us_decode", "us_cons",
        "sum", "xor"]
CONS_FILE = "a.close.cons"
# dfk_offsets_stats' words (include/dfk.h, DFK_OFFSETS_*)
OFFSETS_WORDS = 24
OFFSETS = ["pairs", "candidates", "passed", "invalidated", "deleted_small", "survivors", "pairs_0", "pairs_1", "pairs_2", "pairs_more", "closable", "lookups", "batches",
           "us", "us_candidates", "us_bits", "us_compact", "us_tail", "us_copy", "sum", "xor"]
OFFSETS_FILE = "a.close.offsets"
OFFSETS_RECORD = np.dtype([("offset", "<i4"), ("overlap", "<i4"), ("fraglen", "<i4"), ("mismatch", "<i4"), ("bits", "<f8"), ("state", "<u4"), ("zero", "<u4")])
# dfk_closures_stats' words (include/dfk.h, DFK_CLOSURES_*)
CLOSURES_WORDS = 24
CLOSURES = ["pairs", "closable", "over", "closures", "columns", "cells", "live", "empty", "short", "rowless", "batches", "ranges", "us", "us_dims", "us_copy", "us_decode", "us_cons",
            "sum", "xor"]
CLOSURES_FILE = "a.close.closures"
# dfk_walks_stats' words (include/dfk.h, DFK_WALKS_*)
WALKS_WORDS = 32
WALKS = ["pairs", "walks", "entries", "placed", "ee", "longest", "dup_steps", "steps", "past_edge", "side0_empty", "side1_empty", "short", "trimmed", "yields", "live_sum", "live_max",
         "host_route", "verified", "collisions", "kmers", "decoded", "batches", "ranges", "us", "us_copy", "us_decode", "us_sort", "us_walk", "sum", "xor"]
WALKS_FILE = "a.stack.walks"
WALKS_PLACED = np.dtype([("id", "<i8"), ("start", "<i4"), ("fw", "<u4")])
# dfk_scons_stats' words (include/dfk.h, DFK_SCONS_*)
SCONS_WORDS = 32
SCONS = ["pairs", "yields", "stacks", "rows", "rows_kept", "trimmed", "columns", "cells", "capped", "recount", "flat", "allowed", "disallowed", "live", "decoded", "batches", "ranges",
         "us", "us_copy", "us_decode", "us_cons", "us_flat", "us_conflicts", "sum", "xor"]
SCONS_FILE = "a.stack.cons"
# dfk_soffsets_stats' words (include/dfk.h, DFK_SOFFSETS_*)
SOFFSETS_WORDS = 32
SOFFSETS = ["pairs", "yields", "rows", "kmers", "acceptable", "hits", "seen", "disallowed", "lookups", "results", "offsets", "kept", "dropped", "pairs_0", "pairs_1", "pairs_2", "pairs_3",
            "pairs_more", "closable", "live", "decoded", "batches", "ranges", "us", "us_copy", "us_decode", "us_search", "us_emit", "sum", "xor"]
SOFFSETS_FILE = "a.stack.offsets"
SOFFSETS_RECORD = np.dtype([("offset", "<i4"), ("results", "<u4"), ("best_bits", "<f8"), ("state", "<u4"), ("zero", "<u4")])
# dfk_sclosures_stats' words (include/dfk.h, DFK_SCLOSURES_*)
SCLOSURES_WORDS = 32
SCLOSURES = ["pairs", "yields", "closable", "none", "over", "closures", "columns", "cells", "live", "erased", "empty", "short", "rowless", "decoded", "batches", "ranges", "visits", "skipped",
             "us", "us_copy", "us_decode", "us_cons", "us_rows", "sum", "xor"]
SCLOSURES_FILE = "a.stack.closures"
ALLCLOSURES_FILE = "a.closures.fastb"
# dfk_patch_stats' words (include/dfk.h, DFK_PATCH_*)
PATCH_WORDS = 40
PATCH = ["edges", "canonical", "vertices", "crossings", "closures", "short", "positions", "found", "new", "new_unique", "bits_added", "kmers3", "canonical3", "vertices3", "edges3", "single3",
         "cycle_kmers", "path1", "path2", "path3", "to3", "left3", "batches", "us", "us_entries", "us_index", "us_closures", "us_sort", "us_graph", "us_number", "us_paths", "us_copy", "sum", "xor"]
PATCH_FILES = ("a.patch.k", "a.patch.hbv", "a.patch.hbx", "a.patch.to_left", "a.patch.to_right", "a.patch.inv", "a.patch.fastb", "a.patch.kmers", "a.patch.to3")
# dfk_translate_stats' words (include/dfk.h, DFK_TRANSLATE_*)
TRANSLATE_WORDS = 32
TRANSLATE = ["reads", "placed_before", "step2", "walk", "cleared_empty", "cleared_ranoff", "host", "invalid", "edge_changed", "offset_changed", "batches", "placed", "var_bytes",
             "us", "us_decide", "us_host", "us_scan", "us_emit", "us_copy", "sum", "xor"]
TRANSLATE_FILE = "a.patch.paths"
# dfk_adj_outcome's codes (include/dfk.h, DFK_ADJ_*)
ADJ_OUTCOMES = ["not applicable", "used", "discarded: guess too low", "discarded: list problem", "no block", "dropped for an allocation",
                "switched off"]
VERIFY = ["placed", "broken", "hits", "consistent", "no_anchor", "all_consistent", "dict_bad", "outside"]


class DfkError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"dfk error {code}: {msg}")
        self.code = code


class Config(C.Structure):
    _fields_ = [("abi_version", C.c_uint32), ("K", C.c_uint32), ("min_qual", C.c_uint32), ("min_freq", C.c_uint32),
                ("min_bc", C.c_uint32), ("device", C.c_int32), ("ign_bc_below", C.c_int64),
                ("hbm_budget_bytes", C.c_uint64), ("minimizer_len", C.c_uint32), ("flags", C.c_uint32),
                ("inst_per_item", C.c_uint64), ("reserved", C.c_uint64 * 4)]


class Stats(C.Structure):
    _fields_ = [("n_reads", C.c_uint64), ("n_inst", C.c_uint64), ("n_records", C.c_uint64), ("n_buckets", C.c_uint64),
                ("n_items", C.c_uint64), ("n_overflow_items", C.c_uint64), ("n_distinct", C.c_uint64),
                ("n_solid", C.c_uint64), ("adj_probes", C.c_uint64),
                ("ms_upload", C.c_float), ("ms_trim", C.c_float), ("ms_part_count", C.c_float),
                ("ms_part_scatter", C.c_float), ("ms_count", C.c_float), ("ms_fallback", C.c_float),
                ("ms_adjacency", C.c_float), ("ms_total", C.c_float),
                ("hbm_bytes_peak", C.c_uint64), ("reserved", C.c_uint64 * 8)]

    def asdict(self):
        d = {k: getattr(self, k) for k, _ in self._fields_ if k != "reserved"}
        d["n_passes"] = int(self.reserved[0])
        d["us_graph_device"], d["us_graph_host"], d["us_paths"] = int(self.reserved[1]), int(self.reserved[2]), int(self.reserved[3])
        d["gate_timeouts"] = int(self.reserved[4])
        d["hbm_held"] = int(self.reserved[5])
        d["n_scan_launches"] = int(self.reserved[6])
        d["us_bad_sums"] = int(self.reserved[7])
        return d


_lib = None


def build():
    """Compile libdfk.so for gfx950 (hipcc cross-compiles without a GPU)."""
    subprocess.check_call(["make", "-s", "-C", os.path.join(_HERE, "csrc")])


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise DfkError(-2, f"{LIB_PATH} is missing: run `make -C superplus_amd/csrc` (hipcc, gfx950). "
                               "There is no CPU fallback.")
        L = C.CDLL(LIB_PATH)
        L.dfk_last_error.restype = C.c_char_p
        _lib = L
    return _lib


def _check(rc):
    if rc != 0:
        raise DfkError(rc, lib().dfk_last_error().decode())


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


class Dfk:
    """One context on one GPU.  count(...) takes numpy host arrays; count_device(...) takes
    torch tensors already on this context's device."""

    def __init__(self, K=48, min_qual=7, min_freq=3, min_bc=2, ign_bc_below=0, device=0, hbm_budget_bytes=0,
                 minimizer_len=0, keep_pre_adjacency=False, inst_per_item=0, passes=0, keep_inputs=False, mark_bads=False):
        cfg = Config(abi_version=ABI_VERSION, K=K, min_qual=min_qual, min_freq=min_freq, min_bc=min_bc, device=device,
                     ign_bc_below=ign_bc_below, hbm_budget_bytes=hbm_budget_bytes, minimizer_len=minimizer_len,
                     flags=(F_KEEP_PRE_ADJ if keep_pre_adjacency else 0) | (F_KEEP_INPUTS if keep_inputs else 0) | (F_MARK_BADS if mark_bads else 0),
                     inst_per_item=inst_per_item)
        cfg.reserved[0] = passes          # forced number of bucket-range passes; 0 = sized from the free HBM
        self._ctx = C.c_void_p()
        _check(lib().dfk_create(C.byref(cfg), C.byref(self._ctx)))
        self.K = K

    def close(self):
        if self._ctx:
            lib().dfk_destroy(self._ctx)
            self._ctx = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def count(self, packed, base_off, read_len, pq_bytes, pq_off, bc):
        packed = np.ascontiguousarray(packed, np.uint8); base_off = None if base_off is None else np.ascontiguousarray(base_off, np.uint64)
        read_len = np.ascontiguousarray(read_len, np.uint32); pq_bytes = np.ascontiguousarray(pq_bytes, np.uint8)
        pq_off = np.ascontiguousarray(pq_off, np.uint64)
        bc = None if bc is None else np.ascontiguousarray(bc, np.int32)
        _check(lib().dfk_count(self._ctx, _p(packed), _p(base_off), _p(read_len), _p(pq_bytes), _p(pq_off), _p(bc),
                               C.c_uint64(len(read_len))))

    def count_bci(self, packed, base_off, read_len, pq_bytes, pq_off, bci):
        """dfk_count_bci: the barcode index (as read from .bci) instead of the expanded vector; base_off None = dense bases."""
        packed = np.ascontiguousarray(packed, np.uint8); read_len = np.ascontiguousarray(read_len, np.uint32)
        base_off = None if base_off is None else np.ascontiguousarray(base_off, np.uint64)
        pq_bytes = np.ascontiguousarray(pq_bytes, np.uint8); pq_off = np.ascontiguousarray(pq_off, np.uint64)
        bci = np.ascontiguousarray(bci, np.int64)
        _check(lib().dfk_count_bci(self._ctx, _p(packed), _p(base_off), _p(read_len), _p(pq_bytes), _p(pq_off), _p(bci),
                                   C.c_uint64(len(bci)), C.c_uint64(len(read_len))))

    def count_device(self, packed, base_off, read_len, pq_bytes, pq_off, bc):
        """torch tensors on the GPU: packed u8, base_off i64[n+1], read_len i32[n], pq_bytes u8,
        pq_off i64[n+1], bc i32[n] or None."""
        def dp(t):
            return C.c_void_p(0 if t is None else t.data_ptr())
        for t in (packed, base_off, read_len, pq_bytes, pq_off):
            assert t.is_cuda and t.is_contiguous()
        _check(lib().dfk_count_device(self._ctx, dp(packed), C.c_uint64(packed.numel()), dp(base_off), dp(read_len),
                                      dp(pq_bytes), C.c_uint64(pq_bytes.numel()), dp(pq_off), dp(bc),
                                      C.c_uint64(read_len.numel())))

    def hint_file_range(self, array, fd, file_off=0):
        """dfk_hint_file_range: `array` (a numpy array over a mapped file, e.g. np.memmap) is a mapping of a file.  fd >= 0: its
        bytes are those of descriptor `fd` from `file_off` on, and the host-buffer calls read the file (the mapping may go away
        while they run); fd = -1: they read the memory and drop the pages they have read from the page table.  None forgets."""
        if array is None:
            _check(lib().dfk_hint_file_range(self._ctx, None, C.c_uint64(0), C.c_int(-1), C.c_uint64(0)))
        else:
            _check(lib().dfk_hint_file_range(self._ctx, C.c_void_p(array.ctypes.data), C.c_uint64(array.nbytes), C.c_int(fd), C.c_uint64(file_off)))

    def qual_hist(self, max_len):
        """dfk_qual_hist: int64 [2][max_len][256] from the kept reads."""
        out = np.zeros((2, max_len, 256), np.int64)
        _check(lib().dfk_qual_hist(self._ctx, C.c_uint32(max_len), _p(out)))
        return out

    def good_lens(self):
        n = self.stats()["n_reads"]
        out = np.zeros(n, np.uint32)
        _check(lib().dfk_good_lens(self._ctx, _p(out), C.c_uint64(n)))
        return out

    def spectrum(self):
        h = C.POINTER(C.c_int64)(); n = C.c_uint64()
        _check(lib().dfk_spectrum(self._ctx, C.byref(h), C.byref(n)))
        return np.ctypeslib.as_array(h, shape=(n.value,)).copy() if n.value else np.zeros(0, np.int64)

    def spectrum_json(self):
        need = C.c_uint64()
        _check(lib().dfk_spectrum_json(self._ctx, None, C.c_uint64(0), C.byref(need)))
        buf = C.create_string_buffer(need.value + 1)
        _check(lib().dfk_spectrum_json(self._ctx, buf, C.c_uint64(need.value + 1), C.byref(need)))
        return buf.raw[: need.value].decode()

    def solid_count(self):
        n = C.c_uint64()
        _check(lib().dfk_solid_count(self._ctx, C.byref(n)))
        return n.value

    def solid(self, pre_adjacency=False):
        n = self.solid_count()
        out = np.zeros(n, dtype=ENTRY_DTYPE)
        _check(lib().dfk_solid_fetch(self._ctx, _p(out), C.c_uint64(n), C.c_int(1 if pre_adjacency else 0)))
        return out

    def solid_unsorted(self, pre_adjacency=False):
        n = self.solid_count()
        out = np.zeros(n, dtype=ENTRY_DTYPE)
        _check(lib().dfk_solid_fetch_unsorted(self._ctx, _p(out), C.c_uint64(n), C.c_int(1 if pre_adjacency else 0)))
        return out

    def digest(self, pre_adjacency=False):
        """(sum, xor) digest of the dictionary entries, order-independent (dfk_solid_digest)."""
        out = (C.c_uint64 * 2)()
        _check(lib().dfk_solid_digest(self._ctx, C.c_int(1 if pre_adjacency else 0), out))
        return int(out[0]), int(out[1])

    def write_kvec(self, path, pre_adjacency=False, in_order=False):
        """kmers.kvec image; device order unless in_order (ascending k-mers, sorted on the host)."""
        _check(lib().dfk_write_kvec(self._ctx, path.encode(), C.c_int((1 if pre_adjacency else 0) | (2 if in_order else 0))))

    def graph_build(self):
        """Unipath edges (device) + canonical HyperBasevector (host) of the last count's dictionary."""
        _check(lib().dfk_graph_build(self._ctx))
        a, b, c = C.c_uint64(), C.c_uint64(), C.c_uint64()
        _check(lib().dfk_graph_stats(self._ctx, C.byref(a), C.byref(b), C.byref(c)))
        return dict(n_canonical_edges=a.value, n_vertices=b.value, n_edges=c.value)

    def graph_write(self, directory):
        """a.k, a.hbv, a.hbx, a.to_left, a.to_right, a.inv, a.fastb, a.kmers into `directory` (which must exist)."""
        _check(lib().dfk_graph_write(self._ctx, directory.encode()))

    def paths_build(self, packed=None, base_off=None, read_len=None, pq_bytes=None, pq_off=None):
        """Path every read onto the graph (dfk_graph_build first).  numpy host arrays as for count(); none at all = the reads
        the last count() uploaded and kept (keep_inputs=True)."""
        if packed is None:
            _check(lib().dfk_paths_build(self._ctx, None, None, None, None, None, C.c_uint64(0)))
        else:
            packed = np.ascontiguousarray(packed, np.uint8); base_off = np.ascontiguousarray(base_off, np.uint64)
            read_len = np.ascontiguousarray(read_len, np.uint32); pq_bytes = np.ascontiguousarray(pq_bytes, np.uint8)
            pq_off = np.ascontiguousarray(pq_off, np.uint64)
            _check(lib().dfk_paths_build(self._ctx, _p(packed), _p(base_off), _p(read_len), _p(pq_bytes), _p(pq_off), C.c_uint64(len(read_len))))
        return self.paths_stats()

    def paths_build_device(self, packed, base_off, read_len, pq_bytes, pq_off):
        """torch tensors on the GPU, as for count_device()."""
        def dp(t):
            return C.c_void_p(t.data_ptr())
        _check(lib().dfk_paths_build_device(self._ctx, dp(packed), C.c_uint64(packed.numel()), dp(base_off), dp(read_len),
                                            dp(pq_bytes), C.c_uint64(pq_bytes.numel()), dp(pq_off), C.c_uint64(read_len.numel())))
        return self.paths_stats()

    def paths_stats(self):
        a, b, c = C.c_uint64(), C.c_uint64(), C.c_uint64()
        _check(lib().dfk_paths_stats(self._ctx, C.byref(a), C.byref(b), C.byref(c)))
        return dict(n_reads=a.value, n_placed=b.value, n_path_edges=c.value)

    def paths_sink(self, path):
        """dfk_paths_sink: the next paths_build streams a.paths' variable data into `path`; paths_write(path) completes it."""
        _check(lib().dfk_paths_sink(self._ctx, None if path is None else path.encode()))

    def paths_write(self, path):
        """a.paths (feudal file of ReadPath) as WriteAssemblyFiles writes it."""
        _check(lib().dfk_paths_write(self._ctx, path.encode()))

    def paths_index_write(self, directory):
        """a.paths.inv and a.countsb (writePathsIndex) into `directory`; None = everything but the files (paths_digest)."""
        _check(lib().dfk_paths_index_write(self._ctx, None if directory is None else directory.encode()))

    def dups_write(self, path):
        """a.dup (MarkDups); returns the number of pairs marked.  None = no file."""
        n = C.c_uint64()
        _check(lib().dfk_dups_write(self._ctx, None if path is None else path.encode(), C.byref(n)))
        return n.value

    def paths_index_dups_write(self, directory, path):
        """dfk_paths_index_dups_write: both steps, a.paths.inv's lists written under the duplicate marking; returns the pairs marked."""
        n = C.c_uint64()
        _check(lib().dfk_paths_index_dups_write(self._ctx, None if directory is None else directory.encode(), None if path is None else path.encode(), C.byref(n)))
        return n.value

    def bads_sums(self):
        """dfk_bads_sums: MarkBads' per-read sums, u16[n_reads] (mark_bads=True; saturated at 65535, 0 = unplaced or no mismatch)."""
        a = C.c_uint64()
        n = a.value if lib().dfk_paths_stats(self._ctx, C.byref(a), None, None) == 0 else 0      # (no paths: dfk_bads_sums says what is missing)
        out = np.zeros(n, np.uint16)
        _check(lib().dfk_bads_sums(self._ctx, _p(out), C.c_uint64(n)))
        return out

    def bads_write(self, path):
        """a.bad (MarkBads); returns (pairs marked, (sum, xor) digest of the per-read sums).  None = no file."""
        n = C.c_uint64(); dg = (C.c_uint64 * 2)()
        _check(lib().dfk_bads_write(self._ctx, None if path is None else path.encode(), C.byref(n), dg))
        return n.value, (int(dg[0]), int(dg[1]))

    def hops_build(self, bc, one_good=False):
        """dfk_hops_build: FindEdgePairs from the paths, MarkBads' sums (mark_bads=True) and one barcode per read; returns hops_stats()."""
        bc = np.ascontiguousarray(bc, np.int32)
        _check(lib().dfk_hops_build(self._ctx, _p(bc), C.c_int(1 if one_good else 0)))
        return self.hops_stats()

    def hops_build_bci(self, bci, one_good=False):
        """dfk_hops_build_bci: the same from the barcode index (as read from .bci)."""
        bci = np.ascontiguousarray(bci, np.int64)
        _check(lib().dfk_hops_build_bci(self._ctx, _p(bci), C.c_uint64(len(bci)), C.c_int(1 if one_good else 0)))
        return self.hops_stats()

    def hops_build_arrays(self, kmers, inv, to_left, to_right, n_vertices, paths, bc, sums, one_good=False, reads_per_batch=0):
        """dfk_hops_build_arrays: the same stage on a graph and paths given as arrays (paths: a list of edge lists, one per read; sums:
        MarkBads' per-read sums, u16); reads_per_batch 0 = one batch.  Returns hops_stats()."""
        kmers, inv, to_left, to_right, bc = (np.ascontiguousarray(a, np.int32) for a in (kmers, inv, to_left, to_right, bc))
        sums = np.ascontiguousarray(sums, np.uint16)
        first = np.zeros(len(paths) + 1, np.uint64)
        first[1:] = np.cumsum([len(p) for p in paths], dtype=np.uint64)
        edges = np.ascontiguousarray([e for p in paths for e in p] or [0], np.int32)
        assert len(inv) == len(to_left) == len(to_right) == len(kmers) and len(bc) == len(sums) == len(paths)
        _check(lib().dfk_hops_build_arrays(self._ctx, C.c_uint64(len(kmers)), C.c_uint64(n_vertices), _p(kmers), _p(inv), _p(to_left), _p(to_right),
                                           C.c_uint64(len(paths)), _p(first), _p(edges), _p(bc), _p(sums), C.c_int(1 if one_good else 0),
                                           C.c_uint64(reads_per_batch)))
        return self.hops_stats()

    def hops_stats(self):
        """dfk_hops_stats: {counter: value} -- pairs per method and in all, edges searched / extended / decided on the host, times."""
        out = (C.c_uint64 * HOPS_WORDS)()
        _check(lib().dfk_hops_stats(self._ctx, out))
        return {k: int(out[i]) for i, k in enumerate(HOPS)}

    def hops_fetch(self):
        """dfk_hops_fetch: the sorted pairs, int32[n, 2]."""
        n = C.c_uint64()
        _check(lib().dfk_hops_fetch(self._ctx, None, C.c_uint64(0), C.byref(n)))
        out = np.zeros((n.value, 2), np.int32)
        _check(lib().dfk_hops_fetch(self._ctx, _p(out), C.c_uint64(n.value), C.byref(n)))
        return out

    def hops_write(self, path):
        """a.hops (FindEdgePairs); returns (pairs, (sum, xor) digest of the pairs).  None = no file."""
        n = C.c_uint64(); dg = (C.c_uint64 * 2)()
        _check(lib().dfk_hops_write(self._ctx, None if path is None else path.encode(), C.byref(n), dg))
        return n.value, (int(dg[0]), int(dg[1]))

    def subset_build(self, pairs=None):
        """dfk_subset_build: the subset of interest from the edge pairs (None = the context's own hops result; else int32[n, 2]);
        returns subset_stats()."""
        if pairs is None:
            _check(lib().dfk_subset_build(self._ctx, None, C.c_uint64(0)))
        else:
            pairs = np.ascontiguousarray(pairs, np.int32).reshape(-1, 2)
            room = pairs if len(pairs) else np.zeros((1, 2), np.int32)      # (an empty list is still a list: NULL would mean the hops result)
            _check(lib().dfk_subset_build(self._ctx, _p(room), C.c_uint64(len(pairs))))
        return self.subset_stats()

    def subset_build_arrays(self, inv, paths, pairs, reads_per_batch=0, directory=None):
        """dfk_subset_build_arrays: the same stage on arrays (paths: a list of edge lists, one per read; pairs: [(e1, e2)]); with a
        directory the four files a.sub.* are written there.  Returns subset_stats()."""
        inv = np.ascontiguousarray(inv, np.int32)
        first = np.zeros(len(paths) + 1, np.uint64)
        first[1:] = np.cumsum([len(p) for p in paths], dtype=np.uint64)
        edges = np.ascontiguousarray([e for p in paths for e in p] or [0], np.int32)
        pr = np.ascontiguousarray(list(pairs) or [(0, 0)], np.int32).reshape(-1, 2)
        _check(lib().dfk_subset_build_arrays(self._ctx, C.c_uint64(len(inv)), _p(inv), C.c_uint64(len(paths)), _p(first), _p(edges), _p(pr),
                                             C.c_uint64(len(pairs)), C.c_uint64(reads_per_batch), None if directory is None else str(directory).encode()))
        return self.subset_stats()

    def subset_stats(self):
        """dfk_subset_stats: {counter: value} -- eoi, ids, path and index entries, ranges, pairs taken through one read only, times, digests."""
        out = (C.c_uint64 * SUBSET_WORDS)()
        _check(lib().dfk_subset_stats(self._ctx, out))
        return {k: int(out[i]) for i, k in enumerate(SUBSET)}

    def subset_fetch(self):
        """dfk_subset_fetch: (read_ids, eoi), ascending uint64."""
        ni, ne = C.c_uint64(), C.c_uint64()
        _check(lib().dfk_subset_fetch(self._ctx, None, C.c_uint64(0), C.byref(ni), None, C.c_uint64(0), C.byref(ne)))
        ids, eoi = np.zeros(ni.value, np.uint64), np.zeros(ne.value, np.uint64)
        _check(lib().dfk_subset_fetch(self._ctx, _p(ids), C.c_uint64(ni.value), C.byref(ni), _p(eoi), C.c_uint64(ne.value), C.byref(ne)))
        return ids, eoi

    def subset_write(self, directory):
        """dfk_subset_write: a.sub.ids, a.sub.eoi, a.sub.paths, a.sub.paths.inv into `directory` (which must exist)."""
        _check(lib().dfk_subset_write(self._ctx, None if directory is None else str(directory).encode()))

    def closer_build(self, dup, pairs=None):
        """dfk_closer_build: the closers' read sets per closer edge.  dup: a byte per PAIR of reads (a.dup's payload); pairs None = the
        context's own hops result, else int32[n, 2].  Returns closer_stats()."""
        dup = None if dup is None else np.ascontiguousarray(dup, np.uint8)
        room_d = dup if dup is None or len(dup) else np.zeros(1, np.uint8)
        if pairs is None:
            _check(lib().dfk_closer_build(self._ctx, None, C.c_uint64(0), _p(room_d)))
        else:
            pairs = np.ascontiguousarray(pairs, np.int32).reshape(-1, 2)
            room = pairs if len(pairs) else np.zeros((1, 2), np.int32)      # (an empty list is still a list: NULL would mean the hops result)
            _check(lib().dfk_closer_build(self._ctx, _p(room), C.c_uint64(len(pairs)), _p(room_d)))
        return self.closer_stats()

    def closer_build_arrays(self, inv, kmers, paths, offsets, pairs, dup, reads_per_batch=0, directory=None):
        """dfk_closer_build_arrays: the same stage on arrays (paths: a list of edge lists, one per read, offsets their offset words;
        pairs: [(e1, e2)]; dup a byte per pair of reads; K is the context's); with a directory the four files a.close.* are written
        there.  Returns closer_stats()."""
        inv, kmers = np.ascontiguousarray(inv, np.int32), np.ascontiguousarray(kmers, np.int32)
        first = np.zeros(len(paths) + 1, np.uint64)
        first[1:] = np.cumsum([len(p) for p in paths], dtype=np.uint64)
        edges = np.ascontiguousarray([e for p in paths for e in p] or [0], np.int32)
        off = np.ascontiguousarray(list(offsets) or [0], np.int32)
        pr = np.ascontiguousarray(list(pairs) or [(0, 0)], np.int32).reshape(-1, 2)
        dp = None if dup is None else np.ascontiguousarray(list(dup) or [0], np.uint8)
        assert len(inv) == len(kmers) and len(offsets) == len(paths)
        _check(lib().dfk_closer_build_arrays(self._ctx, C.c_uint64(len(inv)), _p(inv), _p(kmers), C.c_uint64(len(paths)), _p(first), _p(edges), _p(off), _p(pr),
                                             C.c_uint64(len(pairs)), _p(dp), C.c_uint64(reads_per_batch), None if directory is None else str(directory).encode()))
        return self.closer_stats()

    def closer_stats(self):
        """dfk_closer_stats: {counter: value} -- closer edges, records, anchors, set entries, prec tuples, mates let in and kept out, list
        entries skipped as duplicates, ranges, times, digests."""
        out = (C.c_uint64 * CLOSER_WORDS)()
        _check(lib().dfk_closer_stats(self._ctx, out))
        return {k: int(out[i]) for i, k in enumerate(CLOSER)}

    def closer_fetch(self):
        """dfk_closer_fetch: dict(ce uint64[n], loc_first / anchor_first / read_first uint64[n + 1], locs uint64[m, 2] (id, pos | fw << 32),
        anchors int32[a, 3] (g, add, count), reads uint64[r] (id << 1 | fw))."""
        ne, nl, na, nr = C.c_uint64(), C.c_uint64(), C.c_uint64(), C.c_uint64()
        z = C.c_uint64(0)
        _check(lib().dfk_closer_fetch(self._ctx, None, z, C.byref(ne), None, None, z, C.byref(nl), None, None, z, C.byref(na), None, None, z, C.byref(nr)))
        ce, locs, anchors, reads = np.zeros(ne.value, np.uint64), np.zeros((nl.value, 2), np.uint64), np.zeros((na.value, 3), np.int32), np.zeros(nr.value, np.uint64)
        lf, af, rf = (np.zeros(ne.value + 1, np.uint64) for _ in range(3))
        _check(lib().dfk_closer_fetch(self._ctx, _p(ce), C.c_uint64(ne.value), C.byref(ne), _p(lf), _p(locs), C.c_uint64(nl.value), C.byref(nl),
                                      _p(af), _p(anchors), C.c_uint64(na.value), C.byref(na), _p(rf), _p(reads), C.c_uint64(nr.value), C.byref(nr)))
        return dict(ce=ce, loc_first=lf, locs=locs, anchor_first=af, anchors=anchors, read_first=rf, reads=reads)

    def closer_write(self, directory):
        """dfk_closer_write: a.close.edges, a.close.locs, a.close.anchors, a.close.reads into `directory` (which must exist)."""
        _check(lib().dfk_closer_write(self._ctx, None if directory is None else str(directory).encode()))

    def partners_build(self, packed, base_off, read_len, pairs=None):
        """dfk_partners_build: CloseGap2's unplaced partners per pair and side, after closer_build for the same pairs.  The reads as
        paths_verify takes them (base_off None = dense); pairs None = the context's own hops result.  Returns partners_stats()."""
        packed = None if packed is None else np.ascontiguousarray(packed, np.uint8)
        base_off = None if base_off is None else np.ascontiguousarray(base_off, np.uint64)
        read_len = None if read_len is None else np.ascontiguousarray(read_len, np.uint32)
        n = 0 if read_len is None else len(read_len)
        if pairs is None:
            _check(lib().dfk_partners_build(self._ctx, None, C.c_uint64(0), _p(packed), _p(base_off), _p(read_len), C.c_uint64(n)))
        else:
            pairs = np.ascontiguousarray(pairs, np.int32).reshape(-1, 2)
            room = pairs if len(pairs) else np.zeros((1, 2), np.int32)      # (an empty list is still a list: NULL would mean the hops result)
            _check(lib().dfk_partners_build(self._ctx, _p(room), C.c_uint64(len(pairs)), _p(packed), _p(base_off), _p(read_len), C.c_uint64(n)))
        return self.partners_stats()

    def partners_build_arrays(self, a, queries_per_batch=0, directory=None, **change):
        """dfk_partners_build_arrays: the same stage on arrays.  a: dict(inv int32[E], edge_packed uint8[], edge_off uint64[E + 1],
        edge_len uint32[E], ce uint64[n], loc_first uint64[n + 1], locs uint64[2 m], anchor_first uint64[n + 1], anchors int32[3 a],
        pairs int32[p, 2], read_packed uint8[], read_off uint64[N + 1] or None (dense), read_len uint32[N]); with a directory
        a.close.partners is written there.  Returns partners_stats()."""
        a = dict(a); a.update(change)
        kinds = dict(inv=np.int32, edge_packed=np.uint8, edge_off=np.uint64, edge_len=np.uint32, ce=np.uint64, loc_first=np.uint64, locs=np.uint64,
                     anchor_first=np.uint64, anchors=np.int32, pairs=np.int32, read_packed=np.uint8, read_off=np.uint64, read_len=np.uint32)
        n = {k: (0 if a[k] is None else len(a[k])) for k in kinds}
        # (an empty array still has an address: NULL is for what is left out on purpose)
        v = {k: None if a[k] is None else np.ascontiguousarray(a[k] if len(a[k]) else np.zeros(1, t), t) for k, t in kinds.items()}
        _check(lib().dfk_partners_build_arrays(self._ctx, C.c_uint64(n["inv"]), _p(v["inv"]), _p(v["edge_packed"]), _p(v["edge_off"]), _p(v["edge_len"]), C.c_uint64(n["ce"]),
                                               _p(v["ce"]), _p(v["loc_first"]), _p(v["locs"]), _p(v["anchor_first"]), _p(v["anchors"]), _p(v["pairs"]), C.c_uint64(n["pairs"]),
                                               _p(v["read_packed"]), _p(v["read_off"]), _p(v["read_len"]), C.c_uint64(n["read_len"]), C.c_uint64(queries_per_batch),
                                               None if directory is None else str(directory).encode()))
        return self.partners_stats()

    def partners_stats(self):
        """dfk_partners_stats: {counter: value} -- pairs, queries, read positions, table entries, queries with a hit, kept, dropped,
        batches, ranges, times, digest."""
        out = (C.c_uint64 * PARTNERS_WORDS)()
        _check(lib().dfk_partners_stats(self._ctx, out))
        return {k: int(out[i]) for i, k in enumerate(PARTNERS)}

    def partners_fetch(self):
        """dfk_partners_fetch: dict(starts uint64[2 p + 1], recs uint64[m, 2] (id, pos | 1 << 32))."""
        ne, nr = C.c_uint64(), C.c_uint64()
        _check(lib().dfk_partners_fetch(self._ctx, None, C.byref(ne), None, C.c_uint64(0), C.byref(nr)))
        starts, recs = np.zeros(ne.value + 1, np.uint64), np.zeros((nr.value, 2), np.uint64)
        _check(lib().dfk_partners_fetch(self._ctx, _p(starts), C.byref(ne), _p(recs), C.c_uint64(nr.value), C.byref(nr)))
        return dict(starts=starts, recs=recs)

    def partners_write(self, directory):
        """dfk_partners_write: a.close.partners into `directory` (which must exist)."""
        _check(lib().dfk_partners_write(self._ctx, None if directory is None else str(directory).encode()))

    def cons_build(self, packed, base_off, read_len, pq_bytes, pq_off, pairs=None):
        """dfk_cons_build: CloseGap2's stack consensus per pair and side, after closer_build and partners_build for the same pairs.  The
        reads and their PQVec qualities as paths_build takes them (base_off None = dense); pairs None = the context's own hops result.
        Returns cons_stats()."""
        packed = None if packed is None else np.ascontiguousarray(packed, np.uint8)
        base_off = None if base_off is None else np.ascontiguousarray(base_off, np.uint64)
        read_len = None if read_len is None else np.ascontiguousarray(read_len, np.uint32)
        pq_bytes = None if pq_bytes is None else np.ascontiguousarray(pq_bytes, np.uint8)
        pq_off = None if pq_off is None else np.ascontiguousarray(pq_off, np.uint64)
        n = 0 if read_len is None else len(read_len)
        if pairs is None:
            _check(lib().dfk_cons_build(self._ctx, None, C.c_uint64(0), _p(packed), _p(base_off), _p(read_len), _p(pq_bytes), _p(pq_off), C.c_uint64(n)))
        else:
            pairs = np.ascontiguousarray(pairs, np.int32).reshape(-1, 2)
            room = pairs if len(pairs) else np.zeros((1, 2), np.int32)      # (an empty list is still a list: NULL would mean the hops result)
            _check(lib().dfk_cons_build(self._ctx, _p(room), C.c_uint64(len(pairs)), _p(packed), _p(base_off), _p(read_len), _p(pq_bytes), _p(pq_off), C.c_uint64(n)))
        return self.cons_stats()

    def cons_build_arrays(self, a, stacks_per_batch=0, directory=None, **change):
        """dfk_cons_build_arrays: the same stage on arrays.  a: dict(inv int32[E], kmers int32[E], ce uint64[n], loc_first uint64[n + 1],
        locs uint64[2 m], part_first uint64[2 p + 1], parts uint64[2 r], pairs int32[p, 2], read_packed uint8[], read_off uint64[N + 1] or
        None (dense), read_len uint32[N], pq uint8[], pq_off uint64[N + 1]); with a directory a.close.cons is written there.  Returns
        cons_stats()."""
        a = dict(a); a.update(change)
        kinds = dict(inv=np.int32, kmers=np.int32, ce=np.uint64, loc_first=np.uint64, locs=np.uint64, part_first=np.uint64, parts=np.uint64, pairs=np.int32,
                     read_packed=np.uint8, read_off=np.uint64, read_len=np.uint32, pq=np.uint8, pq_off=np.uint64)
        n = {k: (0 if a[k] is None else len(a[k])) for k in kinds}
        # (an empty array still has an address: NULL is for what is left out on purpose)
        v = {k: None if a[k] is None else np.ascontiguousarray(a[k] if len(a[k]) else np.zeros(1, t), t) for k, t in kinds.items()}
        _check(lib().dfk_cons_build_arrays(self._ctx, C.c_uint64(n["inv"]), _p(v["inv"]), _p(v["kmers"]), C.c_uint64(n["ce"]), _p(v["ce"]), _p(v["loc_first"]), _p(v["locs"]),
                                           _p(v["part_first"]), _p(v["parts"]), _p(v["pairs"]), C.c_uint64(n["pairs"]), _p(v["read_packed"]), _p(v["read_off"]), _p(v["read_len"]),
                                           _p(v["pq"]), _p(v["pq_off"]), C.c_uint64(n["read_len"]), C.c_uint64(stacks_per_batch), None if directory is None else str(directory).encode()))
        return self.cons_stats()

    def cons_stats(self):
        """dfk_cons_stats: {counter: value} -- pairs, stacks, rows, live rows, rows kept, stacks trimmed and reversed, columns, cells added,
        reads decoded, batches, ranges, times, digest."""
        out = (C.c_uint64 * CONS_WORDS)()
        _check(lib().dfk_cons_stats(self._ctx, out))
        return {k: int(out[i]) for i, k in enumerate(CONS)}

    def cons_fetch(self):
        """dfk_cons_fetch: dict(starts uint64[2 p + 1], dims int64[2 p, 4] (rows, rows_kept, M, cols), bases uint8[columns])."""
        ne, nb = C.c_uint64(), C.c_uint64()
        _check(lib().dfk_cons_fetch(self._ctx, None, None, C.byref(ne), None, C.c_uint64(0), C.byref(nb)))
        starts, dims, bases = np.zeros(ne.value + 1, np.uint64), np.zeros((max(1, ne.value), 4), np.uint32), np.zeros(max(1, nb.value), np.uint8)
        _check(lib().dfk_cons_fetch(self._ctx, _p(starts), _p(dims), C.byref(ne), _p(bases), C.c_uint64(nb.value), C.byref(nb)))
        dims = dims[: ne.value].astype(np.int64)
        dims[:, 2] = dims[:, 2].astype(np.uint32).view(np.int32) if len(dims) else dims[:, 2]
        return dict(starts=starts, dims=dims, bases=bases[: nb.value])

    def cons_write(self, directory):
        """dfk_cons_write: a.close.cons into `directory` (which must exist)."""
        _check(lib().dfk_cons_write(self._ctx, None if directory is None else str(directory).encode()))

    def offsets_build(self):
        """dfk_offsets_build: GetOffsets1 per pair on the context's latest cons_build* result.  Returns offsets_stats()."""
        _check(lib().dfk_offsets_build(self._ctx))
        return self.offsets_stats()

    def offsets_build_arrays(self, starts, bases, pairs_per_batch=0, directory=None):
        """dfk_offsets_build_arrays: the same stage on arrays: starts uint64[2 p + 1], bases uint8[] (a byte a base, element 2 pi + ei the
        consensus of side ei of pair pi); with a directory a.close.offsets is written there.  Returns offsets_stats()."""
        n = 0 if starts is None else (len(starts) - 1) // 2
        starts = None if starts is None else np.ascontiguousarray(starts, np.uint64)
        # (an empty array still has an address: NULL is for what is left out on purpose)
        bases = None if bases is None else np.ascontiguousarray(bases if len(bases) else np.zeros(1, np.uint8), np.uint8)
        _check(lib().dfk_offsets_build_arrays(self._ctx, C.c_uint64(n), _p(starts), _p(bases), C.c_uint64(pairs_per_batch), None if directory is None else str(directory).encode()))
        return self.offsets_stats()

    def offsets_stats(self):
        """dfk_offsets_stats: {counter: value} -- pairs, candidates, passed, invalidated, deleted as small, survivors, pairs with 0 / 1 / 2 /
        more survivors, closable pairs, look-ups, batches, times, digest."""
        out = (C.c_uint64 * OFFSETS_WORDS)()
        _check(lib().dfk_offsets_stats(self._ctx, out))
        return {k: int(out[i]) for i, k in enumerate(OFFSETS)}

    def offsets_fetch(self):
        """dfk_offsets_fetch: dict(starts uint64[p + 1] in records, words uint32[p, 4] (candidates, passed, survivors, 0), records
        OFFSETS_RECORD[passed])."""
        npairs, nr = C.c_uint64(), C.c_uint64()
        _check(lib().dfk_offsets_fetch(self._ctx, None, None, C.byref(npairs), None, C.c_uint64(0), C.byref(nr)))
        starts, words, recs = np.zeros(npairs.value + 1, np.uint64), np.zeros((max(1, npairs.value), 4), np.uint32), np.zeros(max(1, nr.value), OFFSETS_RECORD)
        _check(lib().dfk_offsets_fetch(self._ctx, _p(starts), _p(words), C.byref(npairs), _p(recs), C.c_uint64(nr.value), C.byref(nr)))
        return dict(starts=starts, words=words[: npairs.value], records=recs[: nr.value])

    def offsets_write(self, directory):
        """dfk_offsets_write: a.close.offsets into `directory` (which must exist)."""
        _check(lib().dfk_offsets_write(self._ctx, None if directory is None else str(directory).encode()))

    def closures_build(self, packed, base_off, read_len, pq_bytes, pq_off):
        """dfk_closures_build: CloseGap2's closures per pair, after cons_build and the offsets_build made from that consensus.  The reads
        are the pathed ones, as cons_build takes them.  Returns closures_stats()."""
        n = 0 if read_len is None else len(read_len)
        packed, read_len, pq_bytes = (None if x is None else np.ascontiguousarray(x, t) for x, t in ((packed, np.uint8), (read_len, np.uint32), (pq_bytes, np.uint8)))
        base_off, pq_off = (None if x is None else np.ascontiguousarray(x, np.uint64) for x in (base_off, pq_off))
        _check(lib().dfk_closures_build(self._ctx, _p(packed), _p(base_off), _p(read_len), _p(pq_bytes), _p(pq_off), C.c_uint64(n)))
        return self.closures_stats()

    def closures_build_arrays(self, a, off_first, offsets, closures_per_batch=0, directory=None, **change):
        """dfk_closures_build_arrays: the same stage on arrays.  a: what cons_build_arrays takes; off_first uint64[p + 1] and offsets int32[]
        the offsets of every pair (a pair with none or more than two gets no closure); with a directory a.close.closures is written there.
        Returns closures_stats()."""
        a = dict(a); a.update(change)
        kinds = dict(inv=np.int32, kmers=np.int32, ce=np.uint64, loc_first=np.uint64, locs=np.uint64, part_first=np.uint64, parts=np.uint64, pairs=np.int32,
                     read_packed=np.uint8, read_off=np.uint64, read_len=np.uint32, pq=np.uint8, pq_off=np.uint64)
        n = {k: (0 if a[k] is None else len(a[k])) for k in kinds}
        # (an empty array still has an address: NULL is for what is left out on purpose)
        v = {k: None if a[k] is None else np.ascontiguousarray(a[k] if len(a[k]) else np.zeros(1, t), t) for k, t in kinds.items()}
        off_first = None if off_first is None else np.ascontiguousarray(off_first, np.uint64)
        offsets = None if offsets is None else np.ascontiguousarray(offsets if len(offsets) else np.zeros(1, np.int32), np.int32)
        _check(lib().dfk_closures_build_arrays(self._ctx, C.c_uint64(n["inv"]), _p(v["inv"]), _p(v["kmers"]), C.c_uint64(n["ce"]), _p(v["ce"]), _p(v["loc_first"]), _p(v["locs"]),
                                               _p(v["part_first"]), _p(v["parts"]), _p(v["pairs"]), C.c_uint64(n["pairs"]), _p(v["read_packed"]), _p(v["read_off"]), _p(v["read_len"]),
                                               _p(v["pq"]), _p(v["pq_off"]), C.c_uint64(n["read_len"]), _p(off_first), _p(offsets), C.c_uint64(closures_per_batch),
                                               None if directory is None else str(directory).encode()))
        return self.closures_stats()

    def closures_stats(self):
        """dfk_closures_stats: {counter: value} -- pairs, closable pairs, pairs left out for more than two offsets, closures, columns, cells
        added, live rows walked, empty columns, closures shorter than K, rowless closures, batches, ranges, times, digest."""
        out = (C.c_uint64 * CLOSURES_WORDS)()
        _check(lib().dfk_closures_stats(self._ctx, out))
        return {k: int(out[i]) for i, k in enumerate(CLOSURES)}

    def closures_fetch(self):
        """dfk_closures_fetch: dict(pair_first uint64[p + 1], starts uint64[n + 1], records int64[n, 4] (pair, offset, cols, rows), bases
        uint8[columns])."""
        npairs, nc, nb = C.c_uint64(), C.c_uint64(), C.c_uint64()
        _check(lib().dfk_closures_fetch(self._ctx, None, None, None, C.byref(npairs), C.byref(nc), None, C.c_uint64(0), C.byref(nb)))
        pair_first, starts = np.zeros(npairs.value + 1, np.uint64), np.zeros(nc.value + 1, np.uint64)
        recs, bases = np.zeros((max(1, nc.value), 4), np.uint32), np.zeros(max(1, nb.value), np.uint8)
        _check(lib().dfk_closures_fetch(self._ctx, _p(pair_first), _p(starts), _p(recs), C.byref(npairs), C.byref(nc), _p(bases), C.c_uint64(nb.value), C.byref(nb)))
        recs = recs[: nc.value].astype(np.int64)
        recs[:, 1] = recs[:, 1].astype(np.uint32).view(np.int32) if len(recs) else recs[:, 1]
        return dict(pair_first=pair_first, starts=starts, records=recs, bases=bases[: nb.value])

    def closures_write(self, directory):
        """dfk_closures_write: a.close.closures into `directory` (which must exist)."""
        _check(lib().dfk_closures_write(self._ctx, None if directory is None else str(directory).encode()))

    def walks_build(self, pairs, packed, base_off, read_len, pq_bytes, pq_off):
        """dfk_walks_build: Stackster's two stack walks per pair, after closer_build.  pairs int32[p, 2] or None (the hops_build pairs); the
        reads are the pathed ones with their PQVec qualities, as cons_build takes them.  Returns walks_stats()."""
        n = 0 if read_len is None else len(read_len)
        pairs = None if pairs is None else np.ascontiguousarray(np.asarray(pairs, np.int32).reshape(-1, 2))
        packed, read_len, pq_bytes = (None if x is None else np.ascontiguousarray(x, t) for x, t in ((packed, np.uint8), (read_len, np.uint32), (pq_bytes, np.uint8)))
        base_off, pq_off = (None if x is None else np.ascontiguousarray(x, np.uint64) for x in (base_off, pq_off))
        _check(lib().dfk_walks_build(self._ctx, _p(pairs), C.c_uint64(0 if pairs is None else len(pairs)), _p(packed), _p(base_off), _p(read_len), _p(pq_bytes), _p(pq_off), C.c_uint64(n)))
        return self.walks_stats()

    def walks_build_arrays(self, a, walks_per_batch=0, directory=None, **change):
        """dfk_walks_build_arrays: the same stage on arrays.  a: dict(inv, kmers int32[E], edge_packed uint8[], edge_off uint64[E + 1], ce
        uint64[], read_first uint64[n_ce + 1], reads uint64[] (id << 1 | fw), pairs int32[p, 2], read_packed, read_off, read_len, pq,
        pq_off); a key in `change` replaces one (None: a NULL pointer).  With a directory a.stack.walks is written there.  Returns
        walks_stats()."""
        a = dict(a); a.update(change)
        kinds = dict(inv=np.int32, kmers=np.int32, edge_packed=np.uint8, edge_off=np.uint64, ce=np.uint64, read_first=np.uint64, reads=np.uint64, pairs=np.int32,
                     read_packed=np.uint8, read_off=np.uint64, read_len=np.uint32, pq=np.uint8, pq_off=np.uint64)
        n = {k: (0 if a[k] is None else len(a[k])) for k in kinds}
        # (an empty array still has an address: NULL is for what is left out on purpose)
        v = {k: None if a[k] is None else np.ascontiguousarray(a[k] if len(a[k]) else np.zeros(1, t), t) for k, t in kinds.items()}
        _check(lib().dfk_walks_build_arrays(self._ctx, C.c_uint64(n["inv"]), _p(v["inv"]), _p(v["kmers"]), _p(v["edge_packed"]), _p(v["edge_off"]), C.c_uint64(n["ce"]), _p(v["ce"]),
                                            _p(v["read_first"]), _p(v["reads"]), _p(v["pairs"]), C.c_uint64(n["pairs"]), _p(v["read_packed"]), _p(v["read_off"]), _p(v["read_len"]),
                                            _p(v["pq"]), _p(v["pq_off"]), C.c_uint64(n["read_len"]), C.c_uint64(walks_per_batch), None if directory is None else str(directory).encode()))
        return self.walks_stats()

    def walks_stats(self):
        """dfk_walks_stats: {counter: value} -- pairs, walks, entries, placed, bases walked, the longest walk, duplicate steps, steps, walks past
        their edge, empty sides, short edges, trimmed sides, live entries, walks done on the host, table hits, batches, ranges, times, digest."""
        out = (C.c_uint64 * WALKS_WORDS)()
        _check(lib().dfk_walks_stats(self._ctx, out))
        return {k: int(out[i]) for i, k in enumerate(WALKS)}

    def walks_fetch(self):
        """dfk_walks_fetch: dict(starts uint64[n + 1], ee_starts uint64[n + 1], records uint32[n, 8] (status, entries, placed, dup_steps, nE,
        nEE, M, trim), placed WALKS_PLACED[], bases uint8[])."""
        n, nl, nb = C.c_uint64(), C.c_uint64(), C.c_uint64()
        _check(lib().dfk_walks_fetch(self._ctx, None, None, None, C.byref(n), None, C.c_uint64(0), C.byref(nl), None, C.c_uint64(0), C.byref(nb)))
        starts, ee_starts = np.zeros(n.value + 1, np.uint64), np.zeros(n.value + 1, np.uint64)
        recs, placed, bases = np.zeros((max(1, n.value), 8), np.uint32), np.zeros(max(1, nl.value), WALKS_PLACED), np.zeros(max(1, nb.value), np.uint8)
        _check(lib().dfk_walks_fetch(self._ctx, _p(starts), _p(ee_starts), _p(recs), C.byref(n), _p(placed), C.c_uint64(nl.value), C.byref(nl), _p(bases), C.c_uint64(nb.value), C.byref(nb)))
        return dict(starts=starts, ee_starts=ee_starts, records=recs[: n.value], placed=placed[: nl.value], bases=bases[: nb.value])

    def walks_write(self, directory):
        """dfk_walks_write: a.stack.walks into `directory` (which must exist)."""
        _check(lib().dfk_walks_write(self._ctx, None if directory is None else str(directory).encode()))

    def scons_build(self, packed, base_off, read_len, pq_bytes, pq_off):
        """dfk_scons_build: Stackster's stack consensus per pair, after walks_build; the reads are the ones the walks were made from with
        their PQVec qualities.  Returns scons_stats()."""
        n = 0 if read_len is None else len(read_len)
        packed, read_len, pq_bytes = (None if x is None else np.ascontiguousarray(x, t) for x, t in ((packed, np.uint8), (read_len, np.uint32), (pq_bytes, np.uint8)))
        base_off, pq_off = (None if x is None else np.ascontiguousarray(x, np.uint64) for x in (base_off, pq_off))
        _check(lib().dfk_scons_build(self._ctx, _p(packed), _p(base_off), _p(read_len), _p(pq_bytes), _p(pq_off), C.c_uint64(n)))
        return self.scons_stats()

    def scons_build_arrays(self, a, stacks_per_batch=0, directory=None, **change):
        """dfk_scons_build_arrays: the same stage on arrays.  a: dict(starts uint64[2 p + 1], records uint32[2 p, 8], placed WALKS_PLACED[]
        (walks_fetch's forms), read_packed, read_off, read_len, pq, pq_off); a key in `change` replaces one (None: a NULL pointer).  With
        a directory a.stack.cons is written there.  Returns scons_stats()."""
        a = dict(a); a.update(change)
        kinds = dict(starts=np.uint64, records=np.uint32, placed=WALKS_PLACED, read_packed=np.uint8, read_off=np.uint64, read_len=np.uint32, pq=np.uint8, pq_off=np.uint64)
        n = {k: (0 if a[k] is None else len(a[k])) for k in kinds}
        # (an empty array still has an address: NULL is for what is left out on purpose)
        v = {k: None if a[k] is None else np.ascontiguousarray(a[k] if len(a[k]) else np.zeros(1, t), t) for k, t in kinds.items()}
        _check(lib().dfk_scons_build_arrays(self._ctx, _p(v["starts"]), _p(v["records"]), _p(v["placed"]), C.c_uint64((n["starts"] - 1) // 2 if n["starts"] else n["records"] // 2), _p(v["read_packed"]), _p(v["read_off"]), _p(v["read_len"]),
                                            _p(v["pq"]), _p(v["pq_off"]), C.c_uint64(n["read_len"]), C.c_uint64(stacks_per_batch), None if directory is None else str(directory).encode()))
        return self.scons_stats()

    def scons_stats(self):
        """dfk_scons_stats: {counter: value} -- pairs, yielding pairs, stacks, rows, rows kept, trimmed stacks, columns, cells, columns capped,
        recounted and flat, offsets allowed and disallowed, live rows, decoded reads, batches, ranges, times, digest."""
        out = (C.c_uint64 * SCONS_WORDS)()
        _check(lib().dfk_scons_stats(self._ctx, out))
        return {k: int(out[i]) for i, k in enumerate(SCONS)}

    def scons_fetch(self):
        """dfk_scons_fetch: dict(starts uint64[n + 1], conflict_first uint64[n / 2 + 1], dims uint32[n, 4] (rows, rows_kept, M, cols), con
        uint8[], conq uint8[], counts uint16[])."""
        n, nc, nk = C.c_uint64(), C.c_uint64(), C.c_uint64()
        _check(lib().dfk_scons_fetch(self._ctx, None, None, None, C.byref(n), None, None, C.c_uint64(0), C.byref(nc), None, C.c_uint64(0), C.byref(nk)))
        starts, cfirst = np.zeros(n.value + 1, np.uint64), np.zeros(n.value // 2 + 1, np.uint64)
        dims, con, conq, counts = np.zeros((max(1, n.value), 4), np.uint32), np.zeros(max(1, nc.value), np.uint8), np.zeros(max(1, nc.value), np.uint8), np.zeros(max(1, nk.value), np.uint16)
        _check(lib().dfk_scons_fetch(self._ctx, _p(starts), _p(cfirst), _p(dims), C.byref(n), _p(con), _p(conq), C.c_uint64(nc.value), C.byref(nc), _p(counts), C.c_uint64(nk.value), C.byref(nk)))
        return dict(starts=starts, conflict_first=cfirst, dims=dims[: n.value], con=con[: nc.value], conq=conq[: nc.value], counts=counts[: nk.value])

    def scons_write(self, directory):
        """dfk_scons_write: a.stack.cons into `directory` (which must exist)."""
        _check(lib().dfk_scons_write(self._ctx, None if directory is None else str(directory).encode()))

    def soffsets_build(self, packed, base_off, read_len, pq_bytes, pq_off):
        """dfk_soffsets_build: Stackster's stack offsets per pair, after walks_build and scons_build; the reads are the ones they were
        made from with their PQVec qualities.  Returns soffsets_stats()."""
        n = 0 if read_len is None else len(read_len)
        packed, read_len, pq_bytes = (None if x is None else np.ascontiguousarray(x, t) for x, t in ((packed, np.uint8), (read_len, np.uint32), (pq_bytes, np.uint8)))
        base_off, pq_off = (None if x is None else np.ascontiguousarray(x, np.uint64) for x in (base_off, pq_off))
        _check(lib().dfk_soffsets_build(self._ctx, _p(packed), _p(base_off), _p(read_len), _p(pq_bytes), _p(pq_off), C.c_uint64(n)))
        return self.soffsets_stats()

    def soffsets_build_arrays(self, a, rows_per_batch=0, directory=None, **change):
        """dfk_soffsets_build_arrays: the same stage on arrays.  a: scons_build_arrays' dict and, in scons_fetch's forms, cons_starts
        uint64[2 p + 1], dims uint32[2 p, 4], con uint8[], conq uint8[], conflict_first uint64[p + 1], counts uint16[]; a key in `change`
        replaces one (None: a NULL pointer).  With a directory a.stack.offsets is written there.  Returns soffsets_stats()."""
        a = dict(a); a.update(change)
        kinds = dict(starts=np.uint64, records=np.uint32, placed=WALKS_PLACED, read_packed=np.uint8, read_off=np.uint64, read_len=np.uint32, pq=np.uint8, pq_off=np.uint64,
                     cons_starts=np.uint64, dims=np.uint32, con=np.uint8, conq=np.uint8, conflict_first=np.uint64, counts=np.uint16)
        n = {k: (0 if a[k] is None else len(a[k])) for k in kinds}
        # (an empty array still has an address: NULL is for what is left out on purpose)
        v = {k: None if a[k] is None else np.ascontiguousarray(a[k] if len(a[k]) else np.zeros(1, t), t) for k, t in kinds.items()}
        _check(lib().dfk_soffsets_build_arrays(self._ctx, _p(v["starts"]), _p(v["records"]), _p(v["placed"]), C.c_uint64((n["starts"] - 1) // 2 if n["starts"] else n["records"] // 2), _p(v["read_packed"]), _p(v["read_off"]),
                                               _p(v["read_len"]), _p(v["pq"]), _p(v["pq_off"]), C.c_uint64(n["read_len"]), _p(v["cons_starts"]), _p(v["dims"]), _p(v["con"]), _p(v["conq"]), _p(v["conflict_first"]),
                                               _p(v["counts"]), C.c_uint64(rows_per_batch), None if directory is None else str(directory).encode()))
        return self.soffsets_stats()

    def soffsets_stats(self):
        """dfk_soffsets_stats: {counter: value} -- pairs, yielding pairs, rows searched, row 8-mers defined, acceptable con 8-mers, hits,
        candidates seen, hits skipped as disallowed, look-ups, results, distinct offsets, kept, dropped, pairs by kept offsets, closable pairs,
        live rows, decoded reads, batches, ranges, times, digest."""
        out = (C.c_uint64 * SOFFSETS_WORDS)()
        _check(lib().dfk_soffsets_stats(self._ctx, out))
        return {k: int(out[i]) for i, k in enumerate(SOFFSETS)}

    def soffsets_fetch(self):
        """dfk_soffsets_fetch: dict(starts uint64[n + 1], words uint32[n, 4] (seen, results, kept, closable), records SOFFSETS_RECORD[])."""
        n, nr = C.c_uint64(), C.c_uint64()
        _check(lib().dfk_soffsets_fetch(self._ctx, None, None, C.byref(n), None, C.c_uint64(0), C.byref(nr)))
        starts, words, recs = np.zeros(n.value + 1, np.uint64), np.zeros((max(1, n.value), 4), np.uint32), np.zeros(max(1, nr.value), SOFFSETS_RECORD)
        _check(lib().dfk_soffsets_fetch(self._ctx, _p(starts), _p(words), C.byref(n), _p(recs), C.c_uint64(nr.value), C.byref(nr)))
        return dict(starts=starts, words=words[: n.value], records=recs[: nr.value])

    def soffsets_write(self, directory):
        """dfk_soffsets_write: a.stack.offsets into `directory` (which must exist)."""
        _check(lib().dfk_soffsets_write(self._ctx, None if directory is None else str(directory).encode()))

    def sclosures_build(self, packed, base_off, read_len, pq_bytes, pq_off):
        """dfk_sclosures_build: Stackster's closures per pair, after walks_build, scons_build and soffsets_build; the reads are the ones
        they were made from with their PQVec qualities.  Returns sclosures_stats()."""
        n = 0 if read_len is None else len(read_len)
        packed, read_len, pq_bytes = (None if x is None else np.ascontiguousarray(x, t) for x, t in ((packed, np.uint8), (read_len, np.uint32), (pq_bytes, np.uint8)))
        base_off, pq_off = (None if x is None else np.ascontiguousarray(x, np.uint64) for x in (base_off, pq_off))
        _check(lib().dfk_sclosures_build(self._ctx, _p(packed), _p(base_off), _p(read_len), _p(pq_bytes), _p(pq_off), C.c_uint64(n)))
        return self.sclosures_stats()

    def sclosures_build_arrays(self, a, closures_per_batch=0, directory=None, **change):
        """dfk_sclosures_build_arrays: the same stage on arrays.  a: scons_build_arrays' dict and dims uint32[2 p, 4] (scons_fetch's form),
        so_starts uint64[p + 1], so_words uint32[p, 4], so_records SOFFSETS_RECORD[] (soffsets_fetch's forms); a key in `change` replaces
        one (None: a NULL pointer).  With a directory a.stack.closures is written there.  Returns sclosures_stats()."""
        a = dict(a); a.update(change)
        kinds = dict(starts=np.uint64, records=np.uint32, placed=WALKS_PLACED, read_packed=np.uint8, read_off=np.uint64, read_len=np.uint32, pq=np.uint8, pq_off=np.uint64,
                     dims=np.uint32, so_starts=np.uint64, so_words=np.uint32, so_records=SOFFSETS_RECORD)
        n = {k: (0 if a[k] is None else len(a[k])) for k in kinds}
        # (an empty array still has an address: NULL is for what is left out on purpose)
        v = {k: None if a[k] is None else np.ascontiguousarray(a[k] if len(a[k]) else np.zeros(1, t), t) for k, t in kinds.items()}
        _check(lib().dfk_sclosures_build_arrays(self._ctx, _p(v["starts"]), _p(v["records"]), _p(v["placed"]), C.c_uint64((n["starts"] - 1) // 2 if n["starts"] else n["records"] // 2), _p(v["read_packed"]), _p(v["read_off"]),
                                                _p(v["read_len"]), _p(v["pq"]), _p(v["pq_off"]), C.c_uint64(n["read_len"]), _p(v["dims"]), _p(v["so_starts"]), _p(v["so_words"]), _p(v["so_records"]),
                                                C.c_uint64(closures_per_batch), None if directory is None else str(directory).encode()))
        return self.sclosures_stats()

    def sclosures_stats(self):
        """dfk_sclosures_stats: {counter: value} -- pairs, yielding pairs, closable pairs, pairs with no kept offset and with more than
        three, closures, columns, cells added, live rows walked, rows erased by the edge trims, empty columns, closures shorter than K,
        rowless closures, decoded reads, batches, ranges, tile visits and those skipped, times, digest."""
        out = (C.c_uint64 * SCLOSURES_WORDS)()
        _check(lib().dfk_sclosures_stats(self._ctx, out))
        return {k: int(out[i]) for i, k in enumerate(SCLOSURES)}

    def sclosures_fetch(self):
        """dfk_sclosures_fetch: dict(pair_first uint64[p + 1], starts uint64[n + 1], records int64[n, 4] (pair, offset, cols, rows), bases
        uint8[columns])."""
        npairs, nc, nb = C.c_uint64(), C.c_uint64(), C.c_uint64()
        _check(lib().dfk_sclosures_fetch(self._ctx, None, None, None, C.byref(npairs), C.byref(nc), None, C.c_uint64(0), C.byref(nb)))
        pair_first, starts = np.zeros(npairs.value + 1, np.uint64), np.zeros(nc.value + 1, np.uint64)
        recs, bases = np.zeros((max(1, nc.value), 4), np.uint32), np.zeros(max(1, nb.value), np.uint8)
        _check(lib().dfk_sclosures_fetch(self._ctx, _p(pair_first), _p(starts), _p(recs), C.byref(npairs), C.byref(nc), _p(bases), C.c_uint64(nb.value), C.byref(nb)))
        recs = recs[: nc.value].astype(np.int64)
        recs[:, 1] = recs[:, 1].astype(np.uint32).view(np.int32) if len(recs) else recs[:, 1]
        return dict(pair_first=pair_first, starts=starts, records=recs, bases=bases[: nb.value])

    def sclosures_write(self, directory):
        """dfk_sclosures_write: a.stack.closures into `directory` (which must exist)."""
        _check(lib().dfk_sclosures_write(self._ctx, None if directory is None else str(directory).encode()))

    def allclosures_write(self, directory):
        """dfk_allclosures_write: a.closures.fastb into `directory` -- per pair Stackster's closures, then CloseGap2's, after closures_build
        and sclosures_build over the same pairs.  Returns dict(closures, bases, stackster, closegap2)."""
        out = (C.c_uint64 * 4)()
        _check(lib().dfk_allclosures_write(self._ctx, None if directory is None else str(directory).encode(), out))
        return dict(closures=int(out[0]), bases=int(out[1]), stackster=int(out[2]), closegap2=int(out[3]))

    def patch_build(self, kmers_per_batch=0):
        """dfk_patch_build: the patched graph hb3 and the old edges' paths to3 / left3 from the context's graph and both closers' closures,
        after closures_build and sclosures_build over the same pairs.  Returns patch_stats()."""
        _check(lib().dfk_patch_build(self._ctx, C.c_uint64(kmers_per_batch)))
        return self.patch_stats()

    def patch_build_arrays(self, inv, to_left, to_right, n_vertices, packed, edge_off, edge_len, closure_starts, closure_bases, kmers_per_batch=0):
        """dfk_patch_build_arrays: the same stage on arrays.  The graph: inv, to_left, to_right int32[n_edges], its edges' bases packed four to
        the byte, edge e at byte edge_off[e] with edge_len[e] bases; the closures: starts uint64[n + 1] into closure_bases uint8[] (0-3).
        Returns patch_stats()."""
        room = lambda a, t: np.ascontiguousarray(a if len(a) else np.zeros(1, t), t)     # (an empty array still has an address)
        n = len(inv)
        inv, to_left, to_right = room(inv, np.int32), room(to_left, np.int32), room(to_right, np.int32)
        packed, edge_off, edge_len = room(packed, np.uint8), room(edge_off, np.uint64), room(edge_len, np.uint32)
        closure_starts = np.ascontiguousarray(closure_starts, np.uint64); closure_bases = room(closure_bases, np.uint8)
        _check(lib().dfk_patch_build_arrays(self._ctx, C.c_uint64(n), C.c_uint64(n_vertices), _p(inv), _p(to_left), _p(to_right), _p(packed), _p(edge_off), _p(edge_len),
                                            C.c_uint64(len(closure_starts) - 1), _p(closure_starts), _p(closure_bases), C.c_uint64(kmers_per_batch)))
        return self.patch_stats()

    def patch_stats(self):
        """dfk_patch_stats: {counter: value} -- the old graph, the closures and their K-mers (found, new, new after de-duplication, context
        bits added), hb3, the old edges' paths by length, to3 entries, nonzero left3, batches, times, digest."""
        out = (C.c_uint64 * PATCH_WORDS)()
        _check(lib().dfk_patch_stats(self._ctx, out))
        return {k: int(out[i]) for i, k in enumerate(PATCH)}

    def patch_fetch(self):
        """dfk_patch_fetch: dict(to3_first uint64[E + 1], to3 int32[], left3 int32[E], kmers, inv, to_left, to_right int32[E3] of hb3)."""
        ne, nt, n3 = C.c_uint64(), C.c_uint64(), C.c_uint64()
        _check(lib().dfk_patch_fetch(self._ctx, C.byref(ne), C.byref(nt), C.byref(n3), None, None, None, None, None, None, None))
        first = np.zeros(ne.value + 1, np.uint64)
        to3, left3 = np.zeros(max(1, nt.value), np.int32), np.zeros(max(1, ne.value), np.int32)
        g = [np.zeros(max(1, n3.value), np.int32) for _ in range(4)]
        _check(lib().dfk_patch_fetch(self._ctx, None, None, None, _p(first), _p(to3), _p(left3), _p(g[0]), _p(g[1]), _p(g[2]), _p(g[3])))
        return dict(to3_first=first, to3=to3[: nt.value], left3=left3[: ne.value], kmers=g[0][: n3.value], inv=g[1][: n3.value], to_left=g[2][: n3.value], to_right=g[3][: n3.value])

    def patch_write(self, directory):
        """dfk_patch_write: a.patch.{k,hbv,hbx,to_left,to_right,inv,fastb,kmers} and a.patch.to3 into `directory` (which must exist)."""
        _check(lib().dfk_patch_write(self._ctx, None if directory is None else str(directory).encode()))

    def translate_build(self):
        """dfk_translate_build: the context's paths moved onto the patched graph dfk_patch_build left (TranslatePaths), as a second list of
        batches on the device; the context's own paths stay.  Returns translate_stats()."""
        _check(lib().dfk_translate_build(self._ctx))
        return self.translate_stats()

    def translate_build_arrays(self, to3_first, to3, left3, kmers3, paths, reads_per_batch=0, directory=None):
        """dfk_translate_build_arrays: the same on arrays.  to3_first uint64[n_edges + 1], to3 int32[], left3 int32[n_edges], kmers3
        int32[n_edges3]; paths as [(offset, [edges])...] or the tuple paths() returns, cut into batches of reads_per_batch (0 = one);
        directory: where a.patch.paths is written too, or None.  Returns translate_stats()."""
        room = lambda a, t: np.ascontiguousarray(a if len(a) else np.zeros(1, t), t)     # (an empty array still has an address)
        if isinstance(paths, tuple):
            offsets, first, edges = paths
        else:
            offsets = np.array([o for o, _ in paths], np.int64)
            first = np.zeros(len(paths) + 1, np.uint64)
            first[1:] = np.cumsum([len(p) for _, p in paths], dtype=np.uint64)
            edges = np.array([e for _, p in paths for e in p], np.int64)
        n, n_edges, n_edges3 = len(offsets), len(left3), len(kmers3)
        to3_first = np.ascontiguousarray(to3_first, np.uint64); first = np.ascontiguousarray(first, np.uint64)
        assert len(to3_first) == n_edges + 1 and len(first) == n + 1
        to3, left3, kmers3, offsets, edges = room(to3, np.int32), room(left3, np.int32), room(kmers3, np.int32), room(offsets, np.int32), room(edges, np.int32)
        _check(lib().dfk_translate_build_arrays(self._ctx, C.c_uint64(n_edges), _p(to3_first), _p(to3), _p(left3), C.c_uint64(n_edges3), _p(kmers3), C.c_uint64(n), _p(first), _p(edges),
                                                _p(offsets), C.c_uint64(reads_per_batch), None if directory is None else str(directory).encode()))
        return self.translate_stats()

    def translate_stats(self):
        """dfk_translate_stats: {counter: value} -- reads, placed before, taken by the first hb3 edge / by the walk, cleared for an empty to3 /
        by running off, decided on the host, ids Validate would refuse, edges / offsets changed, batches, placed now, bytes, times, digest."""
        out = (C.c_uint64 * TRANSLATE_WORDS)()
        _check(lib().dfk_translate_stats(self._ctx, out))
        return {k: int(out[i]) for i, k in enumerate(TRANSLATE)}

    def translate_fetch(self):
        """dfk_translate_fetch -> (offsets i32[n], first_edge u64[n+1], edges i32[...]), as paths()"""
        st = self.translate_stats()
        off = np.zeros(max(1, st["reads"]), np.int32); first = np.zeros(st["reads"] + 1, np.uint64)
        edges = np.zeros(max(1, st["placed"]), np.int32)
        _check(lib().dfk_translate_fetch(self._ctx, _p(off), _p(first), _p(edges), C.c_uint64(len(edges))))
        return off[: st["reads"]], first, edges[: st["placed"]]

    def translate_write(self, directory):
        """dfk_translate_write: a.patch.paths into `directory` (which must exist)."""
        _check(lib().dfk_translate_write(self._ctx, None if directory is None else str(directory).encode()))

    def translate_drop(self):
        """dfk_translate_drop: the translated paths' device blocks go back to the arena."""
        _check(lib().dfk_translate_drop(self._ctx))

    def paths_digest(self):
        """dfk_paths_digest: {name: word} -- content digests of a.paths / a.paths.inv / a.countsb / a.dup and the graph's identities."""
        out = (C.c_uint64 * CHECK_WORDS)()
        _check(lib().dfk_paths_digest(self._ctx, out))
        return {k: int(out[i]) for i, k in enumerate(CK)}

    def paths_verify(self, packed, base_off, read_len):
        """dfk_paths_verify on numpy host arrays (the reads that were pathed): {counter: value}."""
        packed = np.ascontiguousarray(packed, np.uint8); base_off = np.ascontiguousarray(base_off, np.uint64)
        read_len = np.ascontiguousarray(read_len, np.uint32)
        out = (C.c_uint64 * 8)()
        _check(lib().dfk_paths_verify(self._ctx, _p(packed), _p(base_off), _p(read_len), C.c_uint64(len(read_len)), out))
        return {k: int(out[i]) for i, k in enumerate(VERIFY)}

    def paths_verify_device(self, packed, base_off, read_len):
        out = (C.c_uint64 * 8)()
        _check(lib().dfk_paths_verify_device(self._ctx, C.c_void_p(packed.data_ptr()), C.c_uint64(packed.numel()), C.c_void_p(base_off.data_ptr()),
                                             C.c_void_p(read_len.data_ptr()), C.c_uint64(read_len.numel()), out))
        return {k: int(out[i]) for i, k in enumerate(VERIFY)}

    def paths_verify_arrays(self, packed, base_off, read_len, paths, reads_per_batch=0):
        """dfk_paths_verify_arrays: the verifier over paths given as [(offset, [edges])...], one per read (or as the tuple paths()
        returns), cut into batches of reads_per_batch (0 = one).  -> ({counter: value}, (PATHS_SUM, PATHS_XOR) of those paths).
        Offsets and edge ids are taken modulo 2^32, as the file's words hold them."""
        packed = np.ascontiguousarray(packed, np.uint8); base_off = np.ascontiguousarray(base_off, np.uint64)
        read_len = np.ascontiguousarray(read_len, np.uint32)
        if isinstance(paths, tuple):
            offsets, first, edges = paths
        else:
            offsets = np.array([o for o, _ in paths], np.int64).astype(np.uint32).view(np.int32)
            first = np.zeros(len(paths) + 1, np.uint64)
            first[1:] = np.cumsum([len(p) for _, p in paths], dtype=np.uint64)
            edges = np.array([e for _, p in paths for e in p], np.int64).astype(np.uint32).view(np.int32)
        offsets = np.ascontiguousarray(offsets, np.int32); first = np.ascontiguousarray(first, np.uint64)
        edges = np.ascontiguousarray(edges if len(edges) else [0], np.int32)
        assert len(offsets) == len(read_len) == len(first) - 1
        room = lambda a: a if len(a) else np.zeros(1, a.dtype)               # (no reads: still arrays, not NULL)
        out = (C.c_uint64 * 10)()
        _check(lib().dfk_paths_verify_arrays(self._ctx, _p(room(packed)), _p(base_off if len(read_len) else np.zeros(1, np.uint64)), _p(room(read_len)),
                                             C.c_uint64(len(read_len)), _p(room(offsets)), _p(first), _p(edges), C.c_uint64(reads_per_batch), out))
        return {k: int(out[i]) for i, k in enumerate(VERIFY)}, (int(out[8]), int(out[9]))

    def paths(self):
        """-> (offsets i32[n], first_edge u64[n+1], edges i32[...])"""
        st = self.paths_stats()
        off = np.zeros(st["n_reads"], np.int32); first = np.zeros(st["n_reads"] + 1, np.uint64)
        edges = np.zeros(max(1, st["n_path_edges"]), np.int32)
        _check(lib().dfk_paths_fetch(self._ctx, _p(off), _p(first), _p(edges), C.c_uint64(len(edges))))
        return off, first, edges[: st["n_path_edges"]]

    def stats(self):
        s = Stats()
        _check(lib().dfk_get_stats(self._ctx, C.byref(s)))
        return s.asdict()

    def adj_outcome(self):
        """dfk_adj_outcome: (what became of the boundary k-mer set started under the last pass's count -- one of
        ADJ_OUTCOMES -- , slots of the set the adjacency clean-up used)."""
        code, slots = C.c_uint32(), C.c_uint64()
        _check(lib().dfk_adj_outcome(self._ctx, C.byref(code), C.byref(slots)))
        return ADJ_OUTCOMES[code.value], int(slots.value)


def _mix(x):
    x = x ^ (x >> np.uint64(30)); x = x * np.uint64(0xBF58476D1CE4E5B9)
    x = x ^ (x >> np.uint64(27)); x = x * np.uint64(0x94D049BB133111EB)
    return x ^ (x >> np.uint64(31))


def digest_of(entries):
    """numpy form of k_digest (dfk_solid_digest) over 32-byte dictionary entries: (sum, xor).  What a CPU-side answer
    is turned into to be compared with a dictionary that stays on the device."""
    w = np.ascontiguousarray(entries).view(np.uint64).reshape(-1, 4)
    with np.errstate(over="ignore"):
        h = _mix(w[:, 0] ^ _mix(w[:, 1] ^ _mix(w[:, 2] ^ _mix(w[:, 3] + np.uint64(0x9E3779B97F4A7C15)))))
        x = _mix(h + np.uint64(0xD1B54A32D192ED03))
        return int(h.sum(dtype=np.uint64)), int(np.bitwise_xor.reduce(x)) if len(x) else 0
