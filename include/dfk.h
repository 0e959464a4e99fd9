/* include/dfk.h -- C ABI of libdfk.so: the MI355X-native replacement for the k-mer counting
 * hot path that SuperPlus runs as the vendored Supernova `DF` binary.
 *
 * The reference has no plugin/FFI seam for this path; the seam it does have is one
 * file-static C++ call (all reference paths relative to lib/assembly/src):
 *
 *   Dict* createDict(String const& work_dir, vecbvec const& reads,
 *                    ObjectManager<VecPQVec>& quals, unsigned minQual, unsigned minFreq,
 *                    int64_t ignBcBelow, float mem_frac, unsigned minBC,
 *                    vec<int32_t> const* bcp)          paths/long/BuildReadQGraph48.cc:211-215
 *   called from buildReadQGraph48()                    paths/long/BuildReadQGraph48.cc:1626
 *   called from StageBuildGraph()                      10X/runstages/RunStages.cc:389
 *
 * Each entry point below names the part of that call it replaces.  Plain pointers and
 * sizes only; no exceptions cross the boundary; every function returns 0 on success or a
 * negative DFK_E_* code, with a message available from dfk_last_error().  One context per
 * GPU; calls on one context must be serialised by the caller (createDict is likewise
 * called once, from the main thread: MapReduceEngine.h:423-427).
 *
 * There is NO CPU fallback: if no gfx950 device is usable, dfk_create() fails.
 */
#ifndef DFK_H
#define DFK_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define DFK_ABI_VERSION 3
#define DFK_MAX_MIN_BC 8u

enum {
    DFK_OK            = 0,
    DFK_E_ARG         = -1,   /* bad argument / unsupported configuration */
    DFK_E_NODEVICE    = -2,   /* no usable HIP device (the product has no CPU path) */
    DFK_E_HIP         = -3,   /* a HIP runtime call failed */
    DFK_E_NOMEM       = -4,   /* does not fit the HBM budget */
    DFK_E_INPUT       = -5,   /* malformed input (e.g. PQVec length != read length) */
    DFK_E_STATE       = -6,   /* call out of order (e.g. fetch before count) */
    DFK_E_NOGOOD      = -7    /* "almost no good bases": createDict's Scram(1), BuildReadQGraph48.cc:227-230 */
};

/* Mirrors createDict's scalar arguments.  K: the reference instantiates 40, 48 and 60
 * (BuildReadQGraph{40,48,60}.cc); DF's CLI only reaches 48 (RunStages.cc:388). */
typedef struct dfk_config {
    uint32_t abi_version;       /* DFK_ABI_VERSION */
    uint32_t K;                 /* 40, 48 or 60 */
    uint32_t min_qual;          /* MIN_QUAL, default 7   (10X/DF.cc:129-132) */
    uint32_t min_freq;          /* MIN_FREQ, default 3 */
    uint32_t min_bc;            /* MIN_BC,   default 2; 0..DFK_MAX_MIN_BC (a table slot remembers MIN_BC-1 distinct barcodes) */
    int32_t  device;            /* HIP device ordinal */
    int64_t  ign_bc_below;      /* createDict ignBcBelow (= bc_start, DF.cc:344-349) */
    uint64_t hbm_budget_bytes;  /* 0 = 90 % of free HBM (mem_frac analogue, GRAPHMEM=0.9); larger requests are clamped to that */
    uint32_t minimizer_len;     /* 0 = default; 8..16 */
    uint32_t flags;             /* DFK_F_* */
    uint64_t inst_per_item;     /* 0 = default; k-mer instances packed into one LDS table pass */
    uint64_t reserved[4];       /* [0] = forced number of bucket-range passes, 0 = sized from the free HBM */
} dfk_config;

#define DFK_F_KEEP_PRE_ADJ   1u   /* also keep contexts before recomputeAdjacencies (kmers.kvec view) */
#define DFK_F_KEEP_INPUTS    2u   /* dfk_count keeps its device copies of the reads (for dfk_paths_build) until the next count */
#define DFK_F_MARK_BADS 4u        /* dfk_paths_build* also gathers MarkBads' per-read sums (dfk_bads_*); set at dfk_create */

/* 32-byte image of KmerDictEntry<K> (kmers/ReadPather.h:105-146,169-195):
 * w0 = bases 0..31 MSB-first, w1 = remaining bases left-aligned (kmers/KMer.h:154-160),
 * edge_id = 0xFFFFFFFF (null), count in bits 0-23 and KMerContext byte in bits 24-31 of
 * count_ctx, tempBC = -1, pad = 0. */
typedef struct dfk_entry32 {
    uint64_t w0, w1;
    uint32_t edge_id;
    uint32_t count_ctx;
    int32_t  bc;
    uint32_t pad;
} dfk_entry32;

typedef struct dfk_stats {
    uint64_t n_reads;
    uint64_t n_inst;            /* k-mer instances Kmerizer::map would emit (the metric's unit) */
    uint64_t n_records;         /* super-k-mer records written by the partition kernel */
    uint64_t n_buckets;         /* fine minimizer buckets */
    uint64_t n_items;           /* LDS table passes */
    uint64_t n_overflow_items;  /* items that had to be split or re-run in the HBM table */
    uint64_t n_distinct;        /* distinct canonical k-mers seen */
    uint64_t n_solid;
    uint64_t adj_probes;        /* neighbour look-ups issued by the adjacency kernel */
    /* GPU time of each stage of the last dfk_count*, milliseconds, from HIP events on the
     * context's stream */
    float ms_upload, ms_trim, ms_part_count, ms_part_scatter, ms_count, ms_fallback, ms_adjacency, ms_total;
    uint64_t hbm_bytes_peak;    /* peak device bytes held by the context */
    uint64_t reserved[8];       /* [0] = passes used, [1..3] = microseconds (graph device, graph host, pathing), [4] = gate timeouts, [5] = device bytes held now, [6] = launches of the counting scan, [7] = microseconds of the pathing spent in k_bad_sums (DFK_F_MARK_BADS) */
} dfk_stats;

typedef struct dfk_ctx dfk_ctx;

/* Construct / destroy.  Replaces nothing in the reference (its state lives on createDict's stack). */
int         dfk_create(const dfk_config* cfg, dfk_ctx** out);
void        dfk_destroy(dfk_ctx* ctx);
const char* dfk_last_error(void);
int         dfk_abi_version(void);

/* The quality histogram of DF's side file frag_reads_orig.qhist (10X/DF.cc:50-68, DfTools.cc:172-238) from the reads
 * dfk_count kept on the device (DFK_F_KEEP_INPUTS): hist[parity][pos][q], parity = read index & 1, pos < max_len, q < 256 --
 * 2 * max_len * 256 counts.  Positions from max_len on are left out. */
int dfk_qual_hist(dfk_ctx* ctx, uint32_t max_len, int64_t* hist);

/* A hint for the host-buffer calls (dfk_count, dfk_shard_begin_host, dfk_paths_build): the host range
 * [base, base + bytes) is a shared, read-only mapping of a file.  Unmapping a 90-GB input every page of which was touched
 * is three seconds of page-table work for one thread -- at exit, if not before; with the hint it is not left to one thread:
 *   fd >= 0  the mapping shows the file from `file_off` on, and the library READS THE FILE (pread) for every byte of an
 *            input array inside the range instead of the memory: pages nobody else touched are never mapped, and the caller
 *            may unmap the range while the call runs (the descriptor must stay open).  A failing read is DFK_E_INPUT,
 *            never a quiet fall back to the memory.  (Measured: 15 GB/s whatever the number of lanes.)
 *   fd = -1  the library reads the memory and DROPS what it has read from the caller's page table (MADV_DONTNEED: the file
 *            keeps the pages; a later access faults them in again) -- each transfer lane its own chunks -- and marks the
 *            mapping MADV_SEQUENTIAL, without which every page that leaves a page table is marked accessed under one lock
 *            (a freshly written tmpfs file: 25 against 130 GB/s for its first reading).  The mapping must stay until the
 *            call returns.  (Measured: 40-50 GB/s.)
 * base = NULL forgets all hints; at most 8 are kept; dfk_destroy forgets them.  Replaces nothing in the reference (LoadData
 * reads its files through read(2) into vectors, feudal/FeudalFileReader.cc). */
int dfk_hint_file_range(dfk_ctx* ctx, const void* base, uint64_t bytes, int fd, uint64_t file_off);

/* createDict(...) on host buffers laid out exactly as the .fastb/.qualp var data and DF's
 * expanded barcode vector (DF.cc:447-452):
 *   packed_bases + base_off[n+1]  BaseVec bytes, 2-bit LSB-first (feudal/FieldVec.h:766-770)
 *   read_len[n]                   bases per read
 *   pq_bytes + pq_off[n+1]        PQVec block streams (feudal/PQVec.cc:87-127)
 *   bc[n] or NULL                 per-read barcode id; NULL = no barcode test at all
 *                                 (the K=40/60 variants, BuildReadQGraph60.cc:103-151)
 * Runs: quality-tail trim (:218-225), canonical k-mer extraction with contexts (:148-165),
 * counting and the MIN_FREQ/MIN_BC solid filter (:167-174), the spectrum (:192-209) and
 * recomputeAdjacencies (ReadPather.h:329-364, gated by minFreq > 1 as at :313). */
/* Input contract (both calls): the offset tables are checked on the device before anything is read through them
 * (monotone, last offset <= the array size, base_off[r+1]-base_off[r] >= ceil(read_len[r]/4)) and a violation is
 * DFK_E_INPUT.  packed_bases need not start at the first read (a mapped .fastb file with its absolute offset table
 * is a valid input).  Device arrays: packed_bases 4-byte aligned and readable up to 3 bytes past packed_bytes (the
 * 2-bit stream is read as aligned 32-bit words); the offset tables 8-byte aligned.
 * From host buffers the qualities and tables are uploaded first and the bases last, in pieces (from 1 GB of bases on): the
 * trim runs beside the first piece and the counting scan follows the pieces, so that upload and count overlap by what the
 * two take (0.4 s at configs[1]); the result does not depend on it (dfk_stats.reserved[6]: launches of the scan). */
int dfk_count(dfk_ctx* ctx,
              const uint8_t* packed_bases, const uint64_t* base_off, const uint32_t* read_len,
              const uint8_t* pq_bytes, const uint64_t* pq_off, const int32_t* bc,
              uint64_t n_reads);
/* What need not cross PCIe (DF, 10X/DF.cc:300-452, holds both in this form when it reaches createDict):
 *   base_off == NULL (either call)  the bases are DENSE: read r starts where read r-1 ended, ceil(read_len/4) bytes each, read 0
 *                                   at packed_bases -- what BaseVec's feudal writer produces (feudal/FeudalFileWriter.cc:100-121).
 *                                   The offset table is derived on the device from read_len (8 bytes a read not uploaded).
 *   dfk_count_bci                   takes the barcode INDEX of head.bci / frag_reads_orig.bci (n_bci entries, ascending, bci[0] = 0:
 *                                   reads [bci[b], bci[b+1]) carry barcode b) in place of the vector DF expands it to at
 *                                   10X/DF.cc:447-452; the expansion runs on the device (4 bytes a read not uploaded, and not
 *                                   written by the host first).  Reads beyond bci[n_bci-1] are unbarcoded (0). */
int dfk_count_bci(dfk_ctx* ctx,
              const uint8_t* packed_bases, const uint64_t* base_off, const uint32_t* read_len,
              const uint8_t* pq_bytes, const uint64_t* pq_off, const int64_t* bci, uint64_t n_bci,
              uint64_t n_reads);

/* Same call with every array already resident in this context's device memory (bench.py's
 * timed region; multi-GPU shards).  packed_bytes / pq_nbytes are the allocation sizes. */
int dfk_count_device(dfk_ctx* ctx,
              const void* d_packed_bases, uint64_t packed_bytes, const void* d_base_off,
              const void* d_read_len, const void* d_pq_bytes, uint64_t pq_nbytes,
              const void* d_pq_off, const void* d_bc, uint64_t n_reads);

/* goodLens (BuildReadQGraph48.cc:218-225) of the last count, for parity tests. */
int dfk_good_lens(dfk_ctx* ctx, uint32_t* out, uint64_t cap);

/* WriteKmerSpectrum's vector (BuildReadQGraph48.cc:192-209): hist[c] = #solid k-mers with
 * count c, c in [0,max]; *nbins = max+1 (0 when there is no solid k-mer).  The pointer
 * stays valid until the next dfk_count* or dfk_destroy. */
int dfk_spectrum(dfk_ctx* ctx, const int64_t** hist, uint64_t* nbins);
/* Exact text of stats/histogram_kmer_count.json (10X/MakeHist.cc:67-92).  Returns bytes
 * needed (excl. NUL) through *need; writes at most cap bytes. */
int dfk_spectrum_json(dfk_ctx* ctx, char* out, uint64_t cap, uint64_t* need);

/* The Dict's content: number of solid k-mers, then the entries sorted ascending by
 * (w0,w1) with contexts AFTER recomputeAdjacencies.  pre_adjacency != 0 returns the
 * kmers.kvec view (contexts before; needs DFK_F_KEEP_PRE_ADJ). */
int dfk_solid_count(dfk_ctx* ctx, uint64_t* n);
int dfk_solid_fetch(dfk_ctx* ctx, dfk_entry32* out, uint64_t cap, int pre_adjacency);
/* The same entries in the order the device holds them (one copy per pass, no sort): what a caller that
 * inserts them into its own dictionary needs -- the reference's kmers.kvec is in thread-arrival order too. */
int dfk_solid_fetch_unsorted(dfk_ctx* ctx, dfk_entry32* out, uint64_t cap, int pre_adjacency);

/* Order-independent digest of the same entries, computed on the device: digest[0] = sum over entries of h(entry)
 * mod 2^64, digest[1] = xor of h'(entry), h = a 64-bit mix of the entry's 32 bytes (k_digest in dfk_kernels.h;
 * tests/util.py has the numpy form).  Replaces nothing in the reference: it is how two dictionaries of billions
 * of entries are compared without fetching them (pass geometries, single GPU against sharded: digests of the
 * ranks' disjoint shares add / xor). */
int dfk_solid_digest(dfk_ctx* ctx, int pre_adjacency, uint64_t* digest /* [2] */);

/* kmers.kvec image ("BINWRITE" | u64 n | n x 32-B entries; BuildReadQGraph48.cc:287-288,
 * feudal/BinaryStream.h:33-46) written straight to a file, streamed from the device in the order the
 * device holds the entries -- the reference's own file is in thread-arrival order (ReadPather.h:406-418)
 * and its reader inserts the entries into a hash set (BuildReadQGraph48.cc:294-301), so no order is
 * promised by either side.  flags: DFK_KVEC_PRE_ADJ = contexts before recomputeAdjacencies (needs
 * DFK_F_KEEP_PRE_ADJ); DFK_KVEC_SORTED = ascending (w0,w1), sorted on the host (parity tests: needs two
 * host copies of the dictionary). */
#define DFK_KVEC_PRE_ADJ 1
#define DFK_KVEC_SORTED  2
int dfk_write_kvec(dfk_ctx* ctx, const char* path, int flags);
/* The same file written by several ranks (multi-GPU runs: solid sets are disjoint): every rank writes its share at
 * entry first_entry of a file of total_entries entries (the caller derives first_entry from the ranks' solid counts);
 * the rank with first_entry == 0 writes the header.  Device order only. */
int dfk_write_kvec_part(dfk_ctx* ctx, const char* path, int flags, uint64_t first_entry, uint64_t total_entries);

int dfk_get_stats(dfk_ctx* ctx, dfk_stats* out);

/* The adjacency clean-up's set of boundary k-mers is allocated when the last pass's count is about to start, cut to
 * the largest free block, and filled from the finished parts while that count runs.  What became of that set in the
 * last run, and the slots of the set the clean-up used (0: it built none). */
#define DFK_ADJ_NOT_APPLICABLE    0u   /* one pass, one stream (DFK_NO_OVERLAP), min_freq 1, a sharded run, or no finished part had a list */
#define DFK_ADJ_USED              1u
#define DFK_ADJ_DISCARDED_LOW     2u   /* the guess of the run's keys was too low: the set would be loaded past 0.6; rebuilt after the count */
#define DFK_ADJ_DISCARDED_LIST    3u   /* a boundary list overflowed or the lists' totals disagree; rebuilt after the count */
#define DFK_ADJ_NO_BLOCK          4u   /* no free block held a set at load <= 0.6 at that moment; built after the count */
#define DFK_ADJ_DROPPED_FOR_ALLOC 5u   /* the last pass needed the room; built after the count */
#define DFK_ADJ_SWITCHED_OFF      6u   /* DFK_NO_EARLY_SET=1 */
int dfk_adj_outcome(dfk_ctx* ctx, uint32_t* outcome, uint64_t* slots);

/* ---- the graph of the solid k-mers (single-GPU counts) ----
 * dfk_graph_build replaces, on the dictionary of the last dfk_count*:
 *   buildEdges         (paths/long/BuildReadQGraph48.cc:505-530, EdgeBuilder :320-503): the unipath edges, each once
 *                      in canonical form -- on the device; as in the reference every dictionary entry then carries
 *                      (edge id, offset on the edge) in place of (null, count) (KDef::set, kmers/ReadPather.h:122-127),
 *                      so dfk_solid_fetch afterwards returns offsets where it returned counts;
 *   buildHBVFromEdges  (paths/long/HBVFromEdges.cc:244-296): vertices = the (K-1)-mers at the edge ends, edges numbered
 *                      in the reference's canonical traversal order, both orientations of every edge -- on the host
 *                      (the numbering IS a sequential traversal).
 * dfk_graph_write writes what WriteAssemblyFiles (10X/WriteFiles.cc:69-101) writes of a.<K>/ for the graph itself:
 * a.k, a.hbv (K | digraphE<basevector>), a.hbx (HyperBasevectorX), a.to_left, a.to_right, a.inv
 * (HyperBasevector::Involution), a.fastb (the edges), a.kmers -- byte for byte; the paths files need the read pather
 * (SURVEY 8(f)-2).  dfk_stats.reserved[1] / [2]: microseconds spent on the edges (device) / the numbering (host). */
int dfk_graph_build(dfk_ctx* ctx);
int dfk_graph_stats(dfk_ctx* ctx, uint64_t* n_canonical_edges, uint64_t* n_vertices, uint64_t* n_edges);
int dfk_graph_write(dfk_ctx* ctx, const char* dir);

/* a.paths written WHILE the reads are being pathed: the next dfk_paths_build creates `path` and a thread of the library's
 * takes every finished batch's variable data to its place in the file; dfk_paths_write(ctx, path) -- the same path -- then
 * waits for that thread and adds what only the whole build knows (control block, offset table).  One file on a tmpfs takes
 * what one writer gives (9 GB/s): this starts the 37 GB of configs[1] two seconds earlier.  path = NULL: back to
 * dfk_paths_write writing everything.  A build that fails removes the file.  (ReadPathVec::WriteAll, 10X/WriteFiles.cc:78-82,
 * writes after pathReads has returned.) */
/* A file that exists at `path` is not truncated when the build starts (dfk_paths_write sets its size): a caller that has made it
 * about as large as a.paths will be (fallocate of 20-odd bytes a read, while the GPU counts) saves the writer the allocation
 * of every page under the file's lock.  The same holds for dir/a.paths.inv of dfk_paths_index_write. */
int dfk_paths_sink(dfk_ctx* ctx, const char* path);

/* ---- read pathing ("correction by pathing") on the graph dfk_graph_build left in the context ----
 * dfk_paths_build replaces pathReads (paths/long/BuildReadQGraph48.cc:1420-1442) as buildReadQGraph48 calls it
 * (:1664-1665, with useNewAligner = True from StageBuildGraph, 10X/runstages/RunStages.cc:389-390): every read --
 * whole, not quality-trimmed -- is looked up k-mer by k-mer in the dictionary and followed along the unipath edges
 * (Pather::path, :685-733), the parts are edited by the rules of HBVPather::algorithmTwo (:1212-1317) and the path is
 * extended left and right over read ends that hang beyond it by the quality-weighted scores of ExtendReadPath
 * (paths/long/ExtendReadPath.cc).  One ReadPath per read: an offset on its first edge and HBV edge ids.
 *   dfk_paths_build         reads in host memory, laid out as for dfk_count (uploaded, pathed, freed); all five arrays
 *                           NULL = the reads the last dfk_count uploaded and kept (DFK_F_KEEP_INPUTS)
 *   dfk_paths_build_device  the same arrays already resident on the context's device
 *   dfk_paths_write         a.<K>/a.paths as WriteAssemblyFiles writes it (10X/WriteFiles.cc:78-82: ReadPathVec::WriteAll, a feudal
 *                           file of {i32 offset, u32 lastSkip = 0, i32 edges...}, paths/long/ReadPath.h:56-63) -- byte for byte
 *   dfk_paths_fetch         offsets[n], first_edge[n+1] (read r's edges are edges[first_edge[r] .. first_edge[r+1])), edges
 * Needs dfk_graph_build on the same count.  dfk_stats.reserved[3]: microseconds spent pathing.
 * dfk_graph_write and dfk_paths_write only READ the context (host tables, finished device buffers) and allocate nothing on the
 * device: each may run on a thread of its own beside the NEXT call in the chain -- dfk_graph_write beside dfk_paths_build,
 * dfk_paths_write beside dfk_paths_index_write / dfk_dups_write -- which is how DF hides the files under the device work.
 * Every other call on a context is serialised by the caller. */
int dfk_paths_build(dfk_ctx* ctx, const uint8_t* packed_bases, const uint64_t* base_off, const uint32_t* read_len,
              const uint8_t* pq_bytes, const uint64_t* pq_off, uint64_t n_reads);
int dfk_paths_build_device(dfk_ctx* ctx, const void* d_packed_bases, uint64_t packed_bytes, const void* d_base_off,
              const void* d_read_len, const void* d_pq_bytes, uint64_t pq_nbytes, const void* d_pq_off, uint64_t n_reads);
int dfk_paths_stats(dfk_ctx* ctx, uint64_t* n_reads, uint64_t* n_placed, uint64_t* n_path_edges);
int dfk_paths_write(dfk_ctx* ctx, const char* path);
int dfk_paths_fetch(dfk_ctx* ctx, int32_t* offsets, uint64_t* first_edge, int32_t* edges, uint64_t edges_cap);

/* ---- the two steps DF takes right after StageBuildGraph (10X/DF.cc:550,560), on the paths dfk_paths_build made ----
 * dfk_paths_index_write  writePathsIndex (10X/PathsIndex.cc:23-146): dir/a.paths.inv -- per HBV edge the reads whose path holds
 *                        it, ascending (a stable radix sort of the (edge, read) pairs on the device; a feudal file of unsigned
 *                        long lists) -- and dir/a.countsb (reads per edge, an edge and its involution summed).  Defined for any
 *                        graph; the reference itself overruns below ~870 edges (caveat 1).
 * dfk_dups_write         MarkDups (10X/SecretOps.cc:410-566): a.dup, one byte per PAIR -- reads with the same first edge, offset
 *                        and first five bases of their mate are duplicates; the one whose pair has the highest quality sum (the
 *                        lowest read id among equals) stays.  Grouped in a hash table on the device instead of sorted. */
/* The index is built one range of edges at a time when the room is short or the paths hold 2^31 entries or more (the
 * reference's 30 chunk files, PathsIndex.cc:32-99, are the same idea): no limit on the number of path entries.  Limits, refused
 * loudly (DFK_E_ARG) rather than wrapped: fewer than 2^32 reads on any ONE edge, fewer than 2^29 HBV edges and offsets within
 * +-2^24 (the duplicate key).  dir / path NULL: everything but the files (dfk_paths_digest). */
int dfk_paths_index_write(dfk_ctx* ctx, const char* dir);
int dfk_dups_write(dfk_ctx* ctx, const char* path, uint64_t* n_marked_pairs);
/* Both steps, as DF takes them one after the other (10X/DF.cc:550,560): the same files, with the lists of a.paths.inv leaving
 * the device and entering the file while the duplicates are marked (when the index is built in one range; otherwise exactly the
 * two calls above). */
int dfk_paths_index_dups_write(dfk_ctx* ctx, const char* dir, const char* dup_path, uint64_t* n_marked_pairs);

/* ---- the first step of the reference's patching stage: MarkBads (10X/SecretOps.cc:71-109, called by StagePatch,
 * 10X/runstages/RunStages.cc:196-200; written as a.<K>/a.bad, 10X/DF.cc:604) ----
 * Every placed read is laid over the concatenation of its path's edges (hb.Cat: K-1 bases shared between neighbours) at its
 * offset; the qualities of the whole read's bases that disagree with the graph, where the two overlap, are added up, and a
 * PAIR is bad when the sum of either of its reads is strictly greater than 150.  The reference reopens .qualp from disk for
 * this; here the sums are gathered by dfk_paths_build* while a batch's reads, qualities, edges and finished paths are on the
 * device together (k_bad_sums, csrc/dfk_paths_kernels.h) -- on a context created with DFK_F_MARK_BADS; without the flag the
 * build launches and allocates nothing for it and the three calls return DFK_E_STATE.
 *   dfk_bads_sums        the per-read sums (saturated at 65535, 0 for a read without a path), for tests
 *   dfk_bads_write       folds the sums to a byte per pair on the device, writes a.bad ("BINWRITE" | u64 pairs | the bytes) and
 *                        returns the number marked; path NULL = everything but the file; digest (or NULL) = sum and xor over the
 *                        reads of h(whole-set read id, sum), so that two runs are compared without fetching: the shares of a
 *                        sharded run's ranks add / xor.  An odd number of reads is DFK_E_ARG, as for dfk_dups_write.
 *   dfk_bads_write_part  a rank's bytes at pair first_pair of a file of total_pairs (the rank with first_pair == 0 writes the
 *                        header), like dfk_shard_dup_write
 * Valid from dfk_paths_build until the paths are dropped (the next build or graph), before or after dfk_paths_index_write /
 * dfk_dups_write: they need neither the reads nor the k-mer index. */
int dfk_bads_sums(dfk_ctx* ctx, uint16_t* out, uint64_t cap);
int dfk_bads_write(dfk_ctx* ctx, const char* path, uint64_t* n_marked_pairs, uint64_t* digest /* [2] or NULL */);
int dfk_bads_write_part(dfk_ctx* ctx, const char* path, uint64_t first_pair, uint64_t total_pairs, uint64_t* n_marked, uint64_t* digest /* [2] or NULL */);

/* ---- the second step of the patching stage: FindEdgePairs (10X/Closomatic.cc:17-358, called by StagePatch,
 * 10X/runstages/RunStages.cc:204-205; written as a.<K>/a.hops, 10X/DF.cc:603) ----
 * Chooses the pairs of graph edges (e1, e2) the gap closer will try to join, by three methods (stated in csrc/dfk_hops.h):
 * an e1 near a sink whose reads' mates end on one e2 under two barcodes (methods 1 and 2), and an edge that the reads on it
 * and on its involution cannot extend by 100 k-mers, with the edges its not-bad reads' mates see under two barcodes (method 3).
 * It reads what dfk_paths_build* left on the device -- the paths, the graph's tables, MarkBads' sums -- and one barcode id per
 * read (bid = N + bc[id]: only equality matters, so bc itself, or the .bci index as dfk_count_bci reads it).  The reference walks
 * a.paths.inv from disk three times with all paths in host memory.
 *   dfk_hops_build      builds the pairs: a combined index of the reads on an edge and on its involution, a range of edges at a
 *                       time (the ranges of the paths index); methods 1 and 2 through an open-address table; method 3 a wave per
 *                       edge with its sets in LDS.  An edge whose sets outgrow the capacities (DFK_HOPS_MAX_SEQS sequences of
 *                       DFK_HOPS_MAX_LEN edges, read from the environment) is never truncated: the host decides it exactly and
 *                       the call counts it.  one_good: the reference's ONE_GOOD (method 1 without the source test).  Holds no
 *                       device memory when it returns; the sorted pairs stay in host memory.  Negative barcodes and an odd
 *                       number of reads are DFK_E_ARG.
 *   dfk_hops_build_bci  the same from the barcode index
 *   dfk_hops_build_arrays  the same stage on a graph and paths given as host arrays, for tests that choose their graph: per edge
 *                       kmers / inv / to_left / to_right (an edge and its involution of one length), the paths as a CSR
 *                       (first[n_reads + 1], edges), one barcode and one MarkBads sum (bad: > 150 on either read of a pair) per read,
 *                       reads_per_batch reads to a batch of paths (0 = one batch).  It lays the paths out as dfk_paths_build does
 *                       and runs what dfk_hops_build runs, with the context's K; needs no count, graph or paths on the context
 *                       and leaves those it has alone.  inv that is no involution, an edge or vertex out of range: DFK_E_ARG.
 *                       Its result is what dfk_hops_stats / _fetch / _write serve until the next dfk_hops_build*.
 *   dfk_hops_stats      out[DFK_HOPS_WORDS]: the counters below
 *   dfk_hops_fetch      the pairs, two int32 each, sorted; pairs NULL and cap 0 = the count alone
 *   dfk_hops_write      a.hops ("BINWRITE" | u64 n | n x (i32, i32)); path NULL = everything but the file; digest (or NULL) = sum
 *                       and xor over the pairs of a 64-bit mix of (first << 32 | second)
 * Valid from dfk_paths_build* on a context created with DFK_F_MARK_BADS until the paths are dropped, before or after
 * dfk_paths_index_write / dfk_dups_write / dfk_bads_write; otherwise DFK_E_STATE.  Not for the ranks of a sharded run: method 3
 * needs the paths of every read on an edge and on its involution in one place. */
#define DFK_HOPS_WORDS 16
#define DFK_HOPS_M1 0            /* pairs of method 1, 2, 3 (each a set) ... */
#define DFK_HOPS_M2 1
#define DFK_HOPS_M3 2
#define DFK_HOPS_PAIRS 3         /* ... and of their union: what a.hops holds */
#define DFK_HOPS_SEARCHED 4      /* edges that reached method 3's search */
#define DFK_HOPS_EXTENDED 5      /* ... of which extended */
#define DFK_HOPS_HOST_EDGES 6    /* ... of which decided on the host (their sets did not fit) */
#define DFK_HOPS_MOST_ROUNDS 7
#define DFK_HOPS_US 8            /* microseconds: the call, */
#define DFK_HOPS_US_INDEX 9      /* the combined index's kernels, */
#define DFK_HOPS_US_M12 10       /* the kernels of methods 1 and 2, */
#define DFK_HOPS_US_M3 11        /* the kernel of method 3, */
#define DFK_HOPS_US_HOST 12      /* the host's exact route (wall) */
#define DFK_HOPS_LARGEST_X 13
#define DFK_HOPS_RANGES 14
int dfk_hops_build(dfk_ctx* ctx, const int32_t* bc /* [n_reads], host */, int one_good);
int dfk_hops_build_bci(dfk_ctx* ctx, const int64_t* bci, uint64_t n_bci, int one_good);
int dfk_hops_build_arrays(dfk_ctx* ctx, uint64_t n_edges, uint64_t n_vertices, const int32_t* kmers, const int32_t* inv, const int32_t* to_left, const int32_t* to_right,
                          uint64_t n_reads, const uint64_t* first /* [n_reads + 1] */, const int32_t* edges, const int32_t* bc, const uint16_t* sums, int one_good,
                          uint64_t reads_per_batch);
int dfk_hops_stats(dfk_ctx* ctx, uint64_t* out /* [DFK_HOPS_WORDS] */);
int dfk_hops_fetch(dfk_ctx* ctx, int32_t* pairs /* 2 per pair */, uint64_t cap, uint64_t* n_pairs);
int dfk_hops_write(dfk_ctx* ctx, const char* path /* NULL = all but the file */, uint64_t* n_pairs, uint64_t* digest /* [2] or NULL */);

/* ---- the third step of the patching stage: the subset of interest (StagePatch, 10X/runstages/RunStages.cc:208-254) ----
 * From the edge pairs: in_pairs[x] for x in {first, second, inv[first], inv[second]} (:213-219); eoi, the marked edges ascending
 * (:222-226); read_ids, both reads of every pair of which either read's path holds a marked edge, ascending (:228-241); and the two
 * subsets the reference then loads from disk element by element: the ReadPaths of read_ids and the ULongVecs of eoi (:253-254).
 * The rule, the plan and the files' layouts are stated in csrc/dfk_subset.h.  The qualities subset (:252) is not made: the ids file
 * is what the reference's own SubsetMasterVec<PQVec>( qualp, read_ids ) needs.
 *   dfk_subset_build    pairs NULL: the context's own dfk_hops_build* result (DFK_E_STATE without one).  Otherwise n_pairs x (i32, i32),
 *                       e.g. read back from an a.hops; needs dfk_paths_build only, not DFK_F_MARK_BADS.  Marks, eoi, the sweep over
 *                       the paths, the ids' number and digest, the entries per edge of interest.  Holds no device memory when it
 *                       returns; eoi, the marks, a bit per pair and the lists' starts stay in host memory.
 *   dfk_subset_build_arrays  the same stage on host arrays, for tests that choose graph, paths and pairs (dfk_hops_build_arrays'
 *                       layout of first / edges).  The arrays do not outlive the call: with dir the four files are written there
 *                       (NULL = none).  Its result is what dfk_subset_stats / _fetch serve until the next dfk_subset_build*;
 *                       dfk_subset_write after it is DFK_E_STATE.  Leaves the context's count, graph and paths alone.
 *   dfk_subset_stats    out[DFK_SUBSET_WORDS]: the counters below
 *   dfk_subset_fetch    read_ids and eoi, ascending u64; a NULL buffer with cap 0 = that count alone; a buffer too small: DFK_E_ARG
 *   dfk_subset_write    into dir (which must exist), all four or none:
 *                         a.sub.ids, a.sub.eoi   "BINWRITE" | u64 n | n x u64 (vec<uint64_t> read_ids; vec<size_type> eoi, size_type =
 *                                                size_t, system/Types.h:126)
 *                         a.sub.paths            feudal ReadPathVec, a.paths' control block, n = ids: element k = the bytes of element
 *                                                read_ids[k] of a.paths; absolute offsets
 *                         a.sub.paths.inv        feudal VecULongVec, a.paths.inv's control block, n = eoi: element k = the bytes of
 *                                                element eoi[k] of a.paths.inv
 *                       streamed a batch of paths and a range of eoi ranks at a time (DFK_PIDX_RANGE_PAIRS forces small ranges):
 *                       neither subset is ever whole on the device.
 * Valid from dfk_paths_build until the paths are dropped, before or after dfk_paths_index_write / dfk_dups_write / dfk_bads_write;
 * otherwise DFK_E_STATE.  A refused call changes nothing and an earlier result is still served: an edge id outside [0, E), an odd
 * number of reads, a paths subset of 2^32 elements or more (a feudal file counts in 32 bits), one edge with 2^32 entries or more
 * are DFK_E_ARG.  Not for the ranks of a sharded run. */
#define DFK_SUBSET_WORDS 16
#define DFK_SUBSET_N_EOI 0
#define DFK_SUBSET_N_IDS 1
#define DFK_SUBSET_PATH_ENTRIES 2    /* path entries of the reads in the subset */
#define DFK_SUBSET_INDEX_ENTRIES 3   /* entries of the index subset */
#define DFK_SUBSET_RANGES 4          /* ranges of eoi ranks the index subset is (the build: would be) written in */
#define DFK_SUBSET_ONE_READ_ONLY 5   /* pairs taken through one read only */
#define DFK_SUBSET_US 6              /* microseconds: the build call, */
#define DFK_SUBSET_US_SWEEP 7        /* its marks, ranks and sweep, */
#define DFK_SUBSET_US_GATHER 8       /* the ids and paths gather: the build's scans and ids, and the last write's copies, */
#define DFK_SUBSET_US_INDEX 9        /* the index subset: the build's counts, and the last write's listing and sorting */
#define DFK_SUBSET_IDS_SUM 10        /* sum and xor over positions i of read_ids of h(i, id) (k_digest_seq, salt 0x7777), */
#define DFK_SUBSET_IDS_XOR 11
#define DFK_SUBSET_EOI_SUM 12        /* ... and of eoi (salt 0x8888) */
#define DFK_SUBSET_EOI_XOR 13
int dfk_subset_build(dfk_ctx* ctx, const int32_t* pairs /* 2 per pair, or NULL */, uint64_t n_pairs);
int dfk_subset_build_arrays(dfk_ctx* ctx, uint64_t n_edges, const int32_t* inv, uint64_t n_reads, const uint64_t* first /* [n_reads + 1] */, const int32_t* edges,
                            const int32_t* pairs, uint64_t n_pairs, uint64_t reads_per_batch, const char* dir /* NULL = no files */);
int dfk_subset_stats(dfk_ctx* ctx, uint64_t* out /* [DFK_SUBSET_WORDS] */);
int dfk_subset_fetch(dfk_ctx* ctx, uint64_t* ids, uint64_t ids_cap, uint64_t* n_ids, uint64_t* eoi, uint64_t eoi_cap, uint64_t* n_eoi);
int dfk_subset_write(dfk_ctx* ctx, const char* dir);

/* ---- the fourth step of the patching stage: the gap closers' read sets per edge (CloseGap2, 10X/Closomatic.cc:503-552; Stackster,
 * 10X/Stackster.cc:289-324) ----
 * For every pair StagePatch calls both closers (RunStages.cc:276-309), and both begin by walking paths_index[f], f in {e, inv[e]},
 * for e = e1 and e = inv[e2], fetching every listed read's path and working out where it lies against the edge.  That front end is
 * all they take from paths and paths_index; it depends on e alone, so it is built once per CLOSER EDGE -- ce = the ascending
 * distinct {first, inv[second]} over the pairs -- and not per pair:
 *   locs(e)     CloseGap2's locs[ei] in the reference's order: (id, pos, fw), pos = offset - k-mers of the edges before the occurrence
 *   anchors(e)  the distinct (g, add) of its prec with MIN_EDGE_COUNT = 5 occurrences or more, with their counts, ascending
 *   reads(e)    Stackster's idsfw for spass 1 (ALT = False): sorted distinct id << 1 | fw, duplicates (dup[id / 2]) left out, mates
 *               within MAX_DIST = 800 let in.  A pair takes reads(e1) U {(id, !fw) : (id, fw) in reads(inv[e2])}.
 * The rule, the plan and the files' layouts are stated in csrc/dfk_closer.h.  Nothing that needs bases or qualities is made.
 *   dfk_closer_build    pairs NULL: the context's own dfk_hops_build* result (DFK_E_STATE without one).  Otherwise n_pairs x (i32, i32).
 *                       dup: n_reads / 2 host bytes, a.dup's payload, required.  The result stays in host memory with the paths.
 *   dfk_closer_build_arrays  the same stage on host arrays, for tests that choose graph, paths, offsets, pairs and marks; K is the
 *                       context's.  reads_per_batch 0 = one batch.  With dir the four files are written there.  Its result is what
 *                       dfk_closer_stats / _fetch / _write serve until the next dfk_closer_build*.
 *   dfk_closer_stats    out[DFK_CLOSER_WORDS]: the counters below
 *   dfk_closer_fetch    ce, and each table's starts ([n_edges + 1] words, or NULL) and records (locs: 2 u64 a record, {id, pos | fw << 32};
 *                       anchors: 3 i32; reads: u64).  A NULL buffer with cap 0 = that count alone; a buffer too small: DFK_E_ARG
 *   dfk_closer_write    into dir (which must exist), all four or none.  Little-endian, no byte undefined:
 *                         a.close.edges    "BINWRITE" | u64 n | n x u64
 *                         the tables       magic[8] | u64 n | (n + 1) x u64 starts | the records; element k belongs to ce[k]
 *                         a.close.locs     "DFKCLOC1", 16-byte records {i64 id, i32 pos, u32 fw}
 *                         a.close.anchors  "DFKCANC1", 12-byte records {i32 g, i32 add, i32 count}
 *                         a.close.reads    "DFKCRDS1",  8-byte records id << 1 | fw
 * Built a range of ce ranks at a time (DFK_PIDX_RANGE_PAIRS forces small ranges): neither table is ever whole on the device.
 * Valid from dfk_paths_build until the paths are dropped, before or after dfk_paths_index_write / dfk_dups_write / dfk_bads_write;
 * otherwise DFK_E_STATE.  A refused call changes nothing and an earlier result is still served: an edge id outside [0, E), an odd
 * number of reads, a read id of 2^31 or more, one edge with 2^32 records or more, dup NULL are DFK_E_ARG.  Not for the ranks of a
 * sharded run. */
#define DFK_CLOSER_WORDS 24
#define DFK_CLOSER_N_EDGES 0         /* closer edges */
#define DFK_CLOSER_N_LOCS 1          /* locs records */
#define DFK_CLOSER_N_ANCHORS 2
#define DFK_CLOSER_N_READS 3         /* set entries */
#define DFK_CLOSER_PREC 4            /* prec tuples seen */
#define DFK_CLOSER_MATES_IN 5        /* mates let in (Stackster.cc:322, before UniqueSort) */
#define DFK_CLOSER_MATES_OUT 6       /* ... and kept out by MAX_DIST (:321) */
#define DFK_CLOSER_DUP_SKIPPED 7     /* list entries skipped as duplicates (:302) */
#define DFK_CLOSER_RANGES 8          /* ranges of ce ranks the tables were built in */
#define DFK_CLOSER_US 9              /* microseconds: the build call, */
#define DFK_CLOSER_US_MARK 10        /* its marks and ranks, */
#define DFK_CLOSER_US_WEIGH 11       /* the weights per rank, */
#define DFK_CLOSER_US_SWEEP 12       /* the ranges' sweeps (counts, scans, records), */
#define DFK_CLOSER_US_SORT 13        /* their sorts, compactions and copies to the host */
#define DFK_CLOSER_EDGES_SUM 14      /* sum and xor over positions i of h(i, word) (k_digest_seq): ce as u64 (salt 0x9999), */
#define DFK_CLOSER_EDGES_XOR 15
#define DFK_CLOSER_LOCS_SUM 16       /* the locs records as u64 words, two a record (salt 0xAAAA), */
#define DFK_CLOSER_LOCS_XOR 17
#define DFK_CLOSER_ANCHORS_SUM 18    /* the anchors records as u32 words, three a record (salt 0xBBBB), */
#define DFK_CLOSER_ANCHORS_XOR 19
#define DFK_CLOSER_READS_SUM 20      /* the reads records as u64 (salt 0xCCCC) */
#define DFK_CLOSER_READS_XOR 21
int dfk_closer_build(dfk_ctx* ctx, const int32_t* pairs /* 2 per pair, or NULL */, uint64_t n_pairs, const uint8_t* dup /* [n_reads / 2] */);
int dfk_closer_build_arrays(dfk_ctx* ctx, uint64_t n_edges, const int32_t* inv, const int32_t* kmers, uint64_t n_reads, const uint64_t* first /* [n_reads + 1] */,
                            const int32_t* edges, const int32_t* offsets /* [n_reads] */, const int32_t* pairs, uint64_t n_pairs, const uint8_t* dup /* [n_reads / 2] */,
                            uint64_t reads_per_batch, const char* dir /* NULL = no files */);
int dfk_closer_stats(dfk_ctx* ctx, uint64_t* out /* [DFK_CLOSER_WORDS] */);
int dfk_closer_fetch(dfk_ctx* ctx, uint64_t* edges, uint64_t edges_cap, uint64_t* n_edges, uint64_t* loc_first, uint64_t* locs, uint64_t locs_cap, uint64_t* n_locs,
                     uint64_t* anchor_first, int32_t* anchors, uint64_t anchors_cap, uint64_t* n_anchors, uint64_t* read_first, uint64_t* reads, uint64_t reads_cap, uint64_t* n_reads);
int dfk_closer_write(dfk_ctx* ctx, const char* dir);

/* ---- the fifth step of the patching stage: CloseGap2's search for unplaced partners (10X/Closomatic.cc:554-585) ----
 * For every pair (e1, e2), es = {e1, inv[e2]}, and each side ei: the forward reads on e = es[ei] whose mate is not forward on
 * e' = es[1 - ei]; every 32-mer of the mate's bases (the whole read, as the .fastb has it) looked up among the 32-mers of the
 * anchors of e' (bod); the mate kept, at pos - l, where all hits agree on one position.  Element 2 * pi + ei is what the loop for
 * ei of pair pi pushes onto locs[1 - ei], in push order.  The rule, the packing of a 32-mer, the plan and the file's layout are
 * stated in csrc/dfk_partners.h.  No qualities are read and no stack is built.
 *   dfk_partners_build  needs the context's dfk_closer_build result, made for the same pairs: DFK_E_STATE without one, DFK_E_ARG for a
 *                       pair whose closer edges are not in ce.  pairs NULL: the context's own dfk_hops_build* result.  The reads as
 *                       dfk_paths_verify takes them, on the host (the kept reads have gone back to the arena by then); base_off NULL:
 *                       dense.  Only the bases of the reads that are searched cross to the device, a batch of queries at a time.
 *                       n_reads that is not the paths' n_reads, a null argument: DFK_E_ARG; an offset table that is not monotone or
 *                       leaves a read fewer bytes than its bases need: DFK_E_INPUT.
 *   dfk_partners_build_arrays  the same stage on host arrays, for tests that choose everything: inv; the edges' bases (packed,
 *                       edge_off[n_edges + 1] in bytes, edge_len in bases); ce, loc_first, locs, anchor_first, anchors in
 *                       dfk_closer_fetch's forms (in every rank the forward records first, ascending by id: DFK_E_ARG otherwise);
 *                       pairs; reads; queries_per_batch (0 = what fits).  With dir the file is written there.  Its result is what
 *                       dfk_partners_stats / _fetch / _write serve until the next dfk_partners_build*.
 *   dfk_partners_stats  out[DFK_PARTNERS_WORDS]: the counters below
 *   dfk_partners_fetch  starts ([n_elements + 1] words, or NULL; n_elements = 2 * n_pairs) and records (2 u64 a record,
 *                       {id, pos | 1 << 32}).  A NULL buffer with cap 0 = the counts alone; a buffer too small: DFK_E_ARG
 *   dfk_partners_write  into dir (which must exist), whole or not at all.  Little-endian, no byte undefined:
 *                         a.close.partners  "DFKCPRT1" | u64 n = 2 * n_pairs | (n + 1) x u64 starts | 16-byte records
 *                                           {i64 id, i32 pos, u32 fw = 1} -- the locs record
 * The table of anchor 32-mers is built a range of ce ranks at a time (DFK_PIDX_RANGE_PAIRS forces small ranges, of the table and
 * of the sides the queries are found in).  Every device block comes from the arena and is back when build returns.  Valid from
 * dfk_closer_build until the paths are dropped, before or after dfk_paths_index_write; a later dfk_closer_build does not change a
 * result already made.  A refused call changes nothing and an earlier result is still served.  Not for the ranks of a sharded run. */
#define DFK_PARTNERS_WORDS 20
#define DFK_PARTNERS_PAIRS 0         /* pairs */
#define DFK_PARTNERS_QUERIES 1       /* mates searched (:566 passed) */
#define DFK_PARTNERS_POSITIONS 2     /* read positions looked at (:574) */
#define DFK_PARTNERS_ENTRIES 3       /* table entries: one per anchor and position of its edge, before UniqueSort, each closer edge once */
#define DFK_PARTNERS_ANY_HIT 4       /* queries with any hit, */
#define DFK_PARTNERS_KEPT 5          /* with one position (kept: the records), */
#define DFK_PARTNERS_MULTI 6         /* with several (dropped) */
#define DFK_PARTNERS_BATCHES 7       /* batches of queries */
#define DFK_PARTNERS_RANGES 8        /* ranges of ce ranks the table was built in */
#define DFK_PARTNERS_US 9            /* microseconds: the build call, */
#define DFK_PARTNERS_US_TABLE 10     /* the table (entries, sorts), */
#define DFK_PARTNERS_US_QUERIES 11   /* the queries (uploads of the closer's tables, forward parts, flags, scans), */
#define DFK_PARTNERS_US_SEARCH 12    /* the search and the compaction, */
#define DFK_PARTNERS_US_COPY 13      /* the gather of the reads' bases on the host and the copies either way */
#define DFK_PARTNERS_SUM 14          /* sum and xor over positions i of h(i, word) (k_digest_seq): the records as u64 words, two a record (salt 0xDDDD) */
#define DFK_PARTNERS_XOR 15
#define DFK_PARTNERS_SEARCHED 16     /* queries against an edge that has anchors: those whose reads' bases cross to the device */
int dfk_partners_build(dfk_ctx* ctx, const int32_t* pairs /* 2 per pair, or NULL */, uint64_t n_pairs, const uint8_t* packed_bases, const uint64_t* base_off /* or NULL: dense */,
                       const uint32_t* read_len, uint64_t n_reads);
int dfk_partners_build_arrays(dfk_ctx* ctx, uint64_t n_edges, const int32_t* inv, const uint8_t* edge_packed, const uint64_t* edge_off /* [n_edges + 1] */, const uint32_t* edge_len,
                              uint64_t n_ce, const uint64_t* ce, const uint64_t* loc_first, const uint64_t* locs, const uint64_t* anchor_first, const int32_t* anchors,
                              const int32_t* pairs, uint64_t n_pairs, const uint8_t* packed_bases, const uint64_t* base_off /* or NULL: dense */, const uint32_t* read_len, uint64_t n_reads,
                              uint64_t queries_per_batch, const char* dir /* NULL = no file */);
int dfk_partners_stats(dfk_ctx* ctx, uint64_t* out /* [DFK_PARTNERS_WORDS] */);
int dfk_partners_fetch(dfk_ctx* ctx, uint64_t* starts, uint64_t* n_elements, uint64_t* recs, uint64_t recs_cap, uint64_t* n_recs);
int dfk_partners_write(dfk_ctx* ctx, const char* dir);

/* ---- the sixth step of the patching stage: CloseGap2's read stacks and their column consensus (10X/Closomatic.cc:587-640) ----
 * For every pair (e1, e2), es = {e1, inv[e2]}, and each side ei: the readstack of locs(e) and the partners pushed onto it, M columns
 * wide, trimmed to its last 400 columns where it is wider, reversed where e == inv[e2] (ReadStack.cc:714-725, 346-353), and the
 * column consensus GetOffsets1 takes of it first (ReadStack.cc:1219-1223, 400-404, 1841-1861): per column the rows in row order, a
 * defined cell adding 0.1 for Q0, 0.2 for Q1 and Q2 and q otherwise to its base's double, the first maximum.  NO STACK IS STORED:
 * what is kept per pair and side is the consensus (at most 400 bases) and the stack's dimensions.  Element 2 * pi + ei is stacks[ei]
 * of pair pi.  The rule, the cell, the plan and the file's layout are stated in csrc/dfk_cons.h.
 *   dfk_cons_build      needs the context's dfk_closer_build AND dfk_partners_build results, made for the same pairs: DFK_E_STATE
 *                       without either; DFK_E_ARG for pairs that are not those the partners were made for.  pairs NULL: the
 *                       context's own dfk_hops_build* result.  The reads with their PQVec qualities as dfk_paths_build takes them, on
 *                       the host; base_off NULL: dense.  Only the reads that rows inside a stack's window name cross to the device,
 *                       each once per batch of stacks, and are decoded there.  n_reads that is not the paths' n_reads, a null
 *                       argument: DFK_E_ARG; an offset table (bases or qualities) that is not monotone or leaves a read fewer bytes
 *                       than its bases need, a PQVec stream that does not hold exactly read_len values: DFK_E_INPUT.
 *   dfk_cons_build_arrays  the same stage on host arrays, for tests that choose everything: inv and kmers per edge (K is the
 *                       context's); ce, loc_first, locs in dfk_closer_fetch's forms; the partners' starts ([2 * n_pairs + 1]) and
 *                       records in dfk_partners_fetch's forms; pairs; reads and qualities; stacks_per_batch (0 = what fits).  With
 *                       dir the file is written there.  Its result is what dfk_cons_stats / _fetch / _write serve until the next
 *                       dfk_cons_build*.
 *   dfk_cons_stats      out[DFK_CONS_WORDS]: the counters below
 *   dfk_cons_fetch      starts ([n_elements + 1] words, or NULL; n_elements = 2 * n_pairs), dims (4 u32 an element: rows,
 *                       rows_kept, M, cols; or NULL) and the bases, a byte each.  A NULL buffer with cap 0 = the counts alone; a
 *                       buffer too small: DFK_E_ARG
 *   dfk_cons_write      into dir (which must exist), whole or not at all.  Little-endian, no byte undefined:
 *                         a.close.cons  "DFKCCON1" | u64 n = 2 * n_pairs | (n + 1) x u64 starts, in bases | n x 16-byte dims
 *                                       {u32 rows, u32 rows_kept, i32 M, u32 cols} | the bases, a byte each (0..3) | zero bytes to
 *                                       a multiple of 8.  starts[k + 1] - starts[k] == cols[k]
 * Dimensions and live rows are found a range of stacks at a time (DFK_PIDX_RANGE_PAIRS forces small ranges, in rows).  Every device
 * block comes from the arena and is back when build returns.  The result stays in host memory with the paths until the next build or
 * until the paths are dropped.  A refused call changes nothing and an earlier result is still served.  Not for the ranks of a
 * sharded run. */
#define DFK_CONS_WORDS 24
#define DFK_CONS_PAIRS 0             /* pairs */
#define DFK_CONS_STACKS 1            /* stacks: two a pair */
#define DFK_CONS_ROWS 2              /* rows of all stacks (:599), */
#define DFK_CONS_LIVE 3              /* those whose span meets their stack's kept columns: the rows the device walks, */
#define DFK_CONS_ROWS_KEPT 4         /* the rows the stacks have after Trim */
#define DFK_CONS_TRIMMED 5           /* stacks wider than 400 columns */
#define DFK_CONS_REVERSED 6          /* stacks reversed (e == inv[e2]) */
#define DFK_CONS_COLUMNS 7           /* columns of all stacks after Trim: the bases of the result */
#define DFK_CONS_CELLS 8             /* defined cells added to a column's sums */
#define DFK_CONS_DECODED 9           /* reads sent up and decoded, summed over the batches */
#define DFK_CONS_BATCHES 10          /* batches of stacks */
#define DFK_CONS_RANGES 11           /* ranges of stacks the dimensions and live rows were found in */
#define DFK_CONS_US 12               /* microseconds: the build call, */
#define DFK_CONS_US_DIMS 13          /* the uploads of the tables and lengths, dimensions and live rows, */
#define DFK_CONS_US_COPY 14          /* the gather of the reads on the host and the copies either way, */
#define DFK_CONS_US_DECODE 15        /* the decode, */
#define DFK_CONS_US_CONS 16          /* the consensus */
#define DFK_CONS_SUM 17              /* sum and xor over positions i of h(i, value) (k_digest_seq, salt 0xEEEE): the dims as u32 words, then the bases one value each */
#define DFK_CONS_XOR 18
int dfk_cons_build(dfk_ctx* ctx, const int32_t* pairs /* 2 per pair, or NULL */, uint64_t n_pairs, const uint8_t* packed_bases, const uint64_t* base_off /* or NULL: dense */,
                   const uint32_t* read_len, const uint8_t* pq, const uint64_t* pq_off, uint64_t n_reads);
int dfk_cons_build_arrays(dfk_ctx* ctx, uint64_t n_edges, const int32_t* inv, const int32_t* kmers, uint64_t n_ce, const uint64_t* ce, const uint64_t* loc_first, const uint64_t* locs,
                          const uint64_t* part_first /* [2 * n_pairs + 1] */, const uint64_t* parts, const int32_t* pairs, uint64_t n_pairs,
                          const uint8_t* packed_bases, const uint64_t* base_off /* or NULL: dense */, const uint32_t* read_len, const uint8_t* pq, const uint64_t* pq_off, uint64_t n_reads,
                          uint64_t stacks_per_batch, const char* dir /* NULL = no file */);
int dfk_cons_stats(dfk_ctx* ctx, uint64_t* out /* [DFK_CONS_WORDS] */);
int dfk_cons_fetch(dfk_ctx* ctx, uint64_t* starts, uint32_t* dims, uint64_t* n_elements, uint8_t* bases, uint64_t bases_cap, uint64_t* n_bases);
int dfk_cons_write(dfk_ctx* ctx, const char* dir);

/* ---- the seventh step of the patching stage: CloseGap2's stack offsets per pair (GetOffsets1, paths/long/ReadStack.cc:1192-1512) ----
 * The statement behind the stacks' consensus (10X/Closomatic.cc:648): the offsets at which a pair's two consensus sequences overlap
 * convincingly -- the candidates from shared 8-mers, the bits test against a table of log binomial sums, invalidation, big near small.
 * A pair gets a closure only with one or two surviving offsets (:651).  The result is a function of the two consensus sequences
 * alone.  The rule, the table, the plan and the file's layout are stated in csrc/dfk_offsets.h.
 *   dfk_offsets_build   works from the context's latest dfk_cons_build* result: DFK_E_STATE without one.
 *   dfk_offsets_build_arrays  the same stage on host arrays, for tests that choose everything: element 2 * pi + ei is con(ei + 1) of
 *                       pair pi, bases[starts[q] .. starts[q + 1]), a byte a base.  DFK_E_ARG for a null argument, starts that do not
 *                       begin at 0 or fall, a base above 3, an element longer than 400.  pairs_per_batch 0 = what fits; with a dir
 *                       the file is written there.
 *   A refused call changes nothing: dfk_offsets_stats / _fetch / _write serve the latest result of either build until the next one.
 *   dfk_offsets_stats   out[DFK_OFFSETS_WORDS]: the counters below
 *   dfk_offsets_fetch   starts ([n_pairs + 1] words, in records, or NULL), words (4 u32 a pair: candidates, passed, survivors, 0, or
 *                       NULL), the 32-byte records; NULL with cap 0 gives the counts alone; a buffer too small DFK_E_ARG, the counts
 *                       still told.
 *   dfk_offsets_write   into dir (which must exist), whole or not at all.  Little-endian, no byte undefined:
 *                         a.close.offsets  "DFKCOFF1" | u64 n_pairs | (n_pairs + 1) x u64 starts, in records | n_pairs x 16-byte
 *                                       { u32 candidates, u32 passed, u32 survivors, u32 0 } | 32-byte records { i32 offset,
 *                                       i32 overlap, i32 fraglen, i32 mismatch, f64 bits, u32 state, u32 0 }: one per offset that
 *                                       passed the bits test, ascending; state 0 surviving, 1 removed by invalidation, 2 removed as
 *                                       small near big. */
#define DFK_OFFSETS_WORDS 24
#define DFK_OFFSETS_PAIRS 0          /* pairs */
#define DFK_OFFSETS_CANDIDATES 1     /* candidate offsets (:1254), */
#define DFK_OFFSETS_PASSED 2         /* those with bits >= 25.0 (:1328): the records, */
#define DFK_OFFSETS_INVALIDATED 3    /* of them removed by another offset's validated positions (:1485), */
#define DFK_OFFSETS_DELETED_SMALL 4  /* removed as small near big (:1502), */
#define DFK_OFFSETS_SURVIVORS 5      /* returned */
#define DFK_OFFSETS_PAIRS_0 6        /* pairs with no surviving offset, */
#define DFK_OFFSETS_PAIRS_1 7        /* one, */
#define DFK_OFFSETS_PAIRS_2 8        /* two, */
#define DFK_OFFSETS_PAIRS_MORE 9     /* more */
#define DFK_OFFSETS_CLOSABLE 10      /* pairs with one or two (Closomatic.cc:651) */
#define DFK_OFFSETS_LOOKUPS 11       /* table cells read by the bits test (:1324) */
#define DFK_OFFSETS_BATCHES 12       /* batches of pairs */
#define DFK_OFFSETS_US 13            /* microseconds: the build call, */
#define DFK_OFFSETS_US_CANDIDATES 14 /* the candidate kernels with their scan, */
#define DFK_OFFSETS_US_BITS 15       /* the bits kernel, */
#define DFK_OFFSETS_US_COMPACT 16    /* the scan and compaction of those that passed, */
#define DFK_OFFSETS_US_TAIL 17       /* invalidation and big near small on the host, */
#define DFK_OFFSETS_US_COPY 18       /* the uploads and the copies back */
#define DFK_OFFSETS_SUM 19           /* sum and xor over positions i of h(i, value) (k_digest_seq, salt 0xF0F0): the per-pair words, then the records as u32 words */
#define DFK_OFFSETS_XOR 20
int dfk_offsets_build(dfk_ctx* ctx);
int dfk_offsets_build_arrays(dfk_ctx* ctx, uint64_t n_pairs, const uint64_t* starts /* [2 * n_pairs + 1] */, const uint8_t* bases, uint64_t pairs_per_batch /* 0 = what fits */,
                             const char* dir /* NULL = no file */);
int dfk_offsets_stats(dfk_ctx* ctx, uint64_t* out /* [DFK_OFFSETS_WORDS] */);
int dfk_offsets_fetch(dfk_ctx* ctx, uint64_t* starts, uint32_t* words, uint64_t* n_pairs, void* records, uint64_t records_cap, uint64_t* n_records);
int dfk_offsets_write(dfk_ctx* ctx, const char* dir);

/* ---- the eighth step of the patching stage: CloseGap2's closures per pair (10X/Closomatic.cc:651-660) ----
 * The function's last statements, and the only thing it returns: for a pair with one or two surviving offsets the two stacks merged at
 * each offset (ReadStack.cc:355-398) and Consensus1 with qualities of the merged stack (:406-427): the base of the greatest (sum, id)
 * pair, so ties go to the HIGHEST base and a column nothing was added to gives base 3.  The sums run over stack 0's rows, then stack
 * 1's, one IEEE double after the other.  No stack is stored.  Where both stacks have no rows (the reference reads an empty vector) the
 * closure is C columns of base 3 and DFK_CLOSURES_ROWLESS counts it.  The rule, the plan and the file's layout: csrc/dfk_closures.h.
 *   dfk_closures_build  works from the context's dfk_cons_build result (with the closer sets and partners it was made from still in
 *                       place) and the dfk_offsets_build result made FROM THAT consensus: DFK_E_STATE without either, when the latest
 *                       consensus or the offsets came from a *_build_arrays call, or when the offsets were made from an older
 *                       consensus.  The read arguments are checked as dfk_cons_build checks them.
 *   dfk_closures_build_arrays  the same stage on host arrays: dfk_cons_build_arrays' arguments, then off_first [n_pairs + 1] and the
 *                       int32 offsets of every pair (the rule :651 is applied to the list given), closures_per_batch 0 = what fits;
 *                       with a dir the file is written there.  DFK_E_ARG for an offset outside [-cols2, cols1] of its pair (so a
 *                       merged stack is never wider than 800 columns; abutting stacks are allowed), starts that fall, null arguments.
 *   A refused call changes nothing: dfk_closures_stats / _fetch / _write serve the latest result of either build until the next one.
 *   dfk_closures_stats  out[DFK_CLOSURES_WORDS]: the counters below
 *   dfk_closures_fetch  pair_first ([n_pairs + 1] words: the first closure of each pair, or NULL), starts ([n_closures + 1] words, in
 *                       bases, or NULL), records (4 u32 a closure: pair, offset as i32, cols, rows, or NULL), the bases a byte each;
 *                       NULL with cap 0 gives the counts alone; a buffer too small DFK_E_ARG, the counts still told.
 *   dfk_closures_write  into dir (which must exist), whole or not at all.  Little-endian, no byte undefined:
 *                         a.close.closures  "DFKCCLS1" | u64 n closures | u64 n_pairs | (n_pairs + 1) x u64 first closure of each pair |
 *                                       (n + 1) x u64 starts, in bases | n x 16-byte { u32 pair, i32 offset, u32 cols, u32 rows }, rows
 *                                       = rows_kept of both stacks | the bases, a byte each (0..3) | zero bytes to a multiple of 8. */
#define DFK_CLOSURES_WORDS 24
#define DFK_CLOSURES_PAIRS 0         /* pairs */
#define DFK_CLOSURES_CLOSABLE 1      /* pairs with one or two offsets (:651): the only ones whose stacks are touched, */
#define DFK_CLOSURES_OVER 2          /* pairs left out for more than two offsets */
#define DFK_CLOSURES_CLOSURES 3      /* closures: one per offset of a closable pair */
#define DFK_CLOSURES_COLUMNS 4       /* columns of all merged stacks: the bases of the result */
#define DFK_CLOSURES_CELLS 5         /* defined cells added to a column's sums */
#define DFK_CLOSURES_LIVE 6          /* live rows walked, summed over the closures */
#define DFK_CLOSURES_EMPTY 7         /* columns nothing was added to (base 3) */
#define DFK_CLOSURES_SHORT 8         /* closures shorter than K (MapClosures drops them later; here they are only counted) */
#define DFK_CLOSURES_ROWLESS 9       /* closures of two stacks without rows */
#define DFK_CLOSURES_BATCHES 10      /* batches of closures */
#define DFK_CLOSURES_RANGES 11       /* ranges of pairs the dimensions and live rows were found in */
#define DFK_CLOSURES_US 12           /* microseconds: the build call, */
#define DFK_CLOSURES_US_DIMS 13      /* the uploads of the tables and lengths, dimensions and live rows, */
#define DFK_CLOSURES_US_COPY 14      /* the gather of the reads on the host and the copies either way, */
#define DFK_CLOSURES_US_DECODE 15    /* the decode, */
#define DFK_CLOSURES_US_CONS 16      /* the merged consensus */
#define DFK_CLOSURES_SUM 17          /* sum and xor over positions i of h(i, value) (k_digest_seq, salt 0xF1F1): the records as u32 words, then the bases one value each */
#define DFK_CLOSURES_XOR 18
int dfk_closures_build(dfk_ctx* ctx, const uint8_t* packed_bases, const uint64_t* base_off /* or NULL: dense */, const uint32_t* read_len, const uint8_t* pq, const uint64_t* pq_off,
                       uint64_t n_reads);
int dfk_closures_build_arrays(dfk_ctx* ctx, uint64_t n_edges, const int32_t* inv, const int32_t* kmers, uint64_t n_ce, const uint64_t* ce, const uint64_t* loc_first, const uint64_t* locs,
                              const uint64_t* part_first, const uint64_t* parts, const int32_t* pairs, uint64_t n_pairs, const uint8_t* packed_bases, const uint64_t* base_off,
                              const uint32_t* read_len, const uint8_t* pq, const uint64_t* pq_off, uint64_t n_reads, const uint64_t* off_first /* [n_pairs + 1] */, const int32_t* offsets,
                              uint64_t closures_per_batch /* 0 = what fits */, const char* dir /* NULL = no file */);
int dfk_closures_stats(dfk_ctx* ctx, uint64_t* out /* [DFK_CLOSURES_WORDS] */);
int dfk_closures_fetch(dfk_ctx* ctx, uint64_t* pair_first, uint64_t* starts, uint32_t* records, uint64_t* n_pairs, uint64_t* n_closures, uint8_t* bases, uint64_t bases_cap, uint64_t* n_bases);
int dfk_closures_write(dfk_ctx* ctx, const char* dir);

/* ---- the second closer's walks: Stackster's two stack walks per pair (10X/Stackster.cc:207-262 StackWalk, :326-414) ----
 * Stackster loads the reads of a pair's set (a.close.reads of es = { e1, inv[e2] } composed), lowers their qualities in homopolymers of 20
 * bases or more, orients them, and for side 0 then side 1 extends the edge's first 48-mer base by base through the set's reads
 * (k = 48 whatever the graph's K): a read is placed by the first step whose 48-mer it holds once, at start = |EE| - 48 - pos; a base is
 * appended while the largest quality sum under it is >= 60 and >= twice the second.  Kept per pair and side: |E|, |EE|, the bases of
 * EE, the steps that met a duplicate, M = max( start + len ), trim = max( 0, M - 400 ), and per placed entry ( id, start, fw ^ side ):
 * the locs the stacks are built from.  No stack is stored.  Side 1 is not walked where side 0 placed nobody (Stackster returns); an
 * edge of fewer than 48 bases (K < 48 only) is not walked.  The rule, the plan and the file's layout: csrc/dfk_walks.h.
 *   dfk_walks_build   works from the context's dfk_closer_build result and the graph's edges; pairs NULL: the dfk_hops_build pairs.  The
 *                     read arguments are the pathed reads with their PQVec qualities, checked as dfk_cons_build checks them.
 *   dfk_walks_build_arrays  the same stage on host arrays: inv and kmers per edge, the bases of EVERY edge 2-bit packed with their byte
 *                     offsets [n_edges + 1] (a.fastb's data), ce ascending, read_first [n_ce + 1] and the sets as dfk_closer_fetch gives
 *                     them ( id << 1 | fw, ascending and distinct per rank ), the pairs, the reads; walks_per_batch 0 = what fits (a batch
 *                     holds whole pairs: ( w + 1 ) / 2 of them); with a dir the file is written there.
 *   DFK_E_ARG for a pair's edge outside the graph or not among ce, tables that fall, null arguments, and for a set of 2^23 entries or
 *   more (the reference's int sums could overflow there); DFK_E_INPUT for a PQVec stream that does not hold its read's length.  A
 *   refused call changes nothing: dfk_walks_stats / _fetch / _write serve the latest result of either build, hbm_held is as before.
 *   A walk whose live list (placed entries that still cover the current column) outgrows DFK_WALK_MAX_LIVE (1024) is done exactly on
 *   the host and counted (DFK_WALKS_HOST_ROUTE); the environment's DFK_WALK_MAX_LIVE (smaller) and DFK_WALK_HASH_BITS (fewer than 64)
 *   are for tests: they force that route, and collisions of the table's hash, which cost time and never change a byte.
 *   dfk_walks_stats   out[DFK_WALKS_WORDS]: the counters below
 *   dfk_walks_fetch   starts and ee_starts ([n_walks + 1] words each, or NULL), records (8 u32 a walk, or NULL), the placed records (16
 *                     bytes each) and the EE bases a byte each; NULL with cap 0 gives the counts alone; a buffer too small DFK_E_ARG.
 *   dfk_walks_write   into dir (which must exist), whole or not at all.  Little-endian, no byte undefined:
 *                       a.stack.walks  "DFKSWLK1" | u64 n = 2 * n_pairs | (n + 1) x u64 first placed record of each walk | (n + 1) x u64
 *                                     first base of each EE | n x 32-byte { u32 status (0 walked, 1 not walked: side 0 placed nobody, 2 the
 *                                     edge is shorter than 48), u32 entries, u32 placed, u32 dup_steps, i32 nE, u32 nEE, i32 M, i32 trim } |
 *                                     the placed records { i64 id, i32 start, u32 fw } | the EE bases four a byte, the first in the low
 *                                     bits | zero bytes to a multiple of 8.  Element 2 pi + s is side s of pair pi. */
#define DFK_WALKS_WORDS 32
#define DFK_WALKS_PAIRS 0            /* pairs */
#define DFK_WALKS_WALKS 1            /* sides walked */
#define DFK_WALKS_ENTRIES 2          /* set entries of the walked sides */
#define DFK_WALKS_PLACED 3           /* entries placed: the placed records */
#define DFK_WALKS_EE 4               /* bases of all EE */
#define DFK_WALKS_LONGEST 5          /* the longest EE */
#define DFK_WALKS_DUP_STEPS 6        /* steps that placed nobody because an entry held the 48-mer twice */
#define DFK_WALKS_STEPS 7            /* steps */
#define DFK_WALKS_PAST_EDGE 8        /* walks whose EE is longer than their edge */
#define DFK_WALKS_SIDE0_EMPTY 9      /* pairs whose side 0 placed nobody (side 1 not walked) */
#define DFK_WALKS_SIDE1_EMPTY 10     /* pairs whose side 1 was walked and placed nobody */
#define DFK_WALKS_SHORT 11           /* sides not walked for an edge shorter than 48 bases */
#define DFK_WALKS_TRIMMED 12         /* sides with M > 400 */
#define DFK_WALKS_YIELDS 13          /* pairs with entries placed on both sides */
#define DFK_WALKS_LIVE_SUM 14        /* live entries summed over the steps */
#define DFK_WALKS_LIVE_MAX 15        /* the longest live list */
#define DFK_WALKS_HOST_ROUTE 16      /* walks done on the host: their live list outgrew its room */
#define DFK_WALKS_VERIFIED 17        /* table hits whose 48 bases matched, */
#define DFK_WALKS_COLLISIONS 18      /* and hits of the hash alone (device walks) */
#define DFK_WALKS_KMERS 19           /* 48-mers sorted, both sides */
#define DFK_WALKS_DECODED 20         /* reads gathered, decoded and lowered, a read once a batch */
#define DFK_WALKS_BATCHES 21         /* batches of pairs */
#define DFK_WALKS_RANGES 22          /* ranges of pairs */
#define DFK_WALKS_US 23              /* microseconds: the build call, */
#define DFK_WALKS_US_COPY 24         /* the gather of the reads on the host and their copies, */
#define DFK_WALKS_US_DECODE 25       /* decode and lowering, */
#define DFK_WALKS_US_SORT 26         /* the tables: 48-mers, hashes, sorts, */
#define DFK_WALKS_US_WALK 27         /* the walk kernel with its copies back */
#define DFK_WALKS_SUM 28             /* sum and xor over positions i of h(i, value) (k_digest_seq, salt 0xABAB): the records as u32 words, the placed records as u64 words, the EE bases */
#define DFK_WALKS_XOR 29
int dfk_walks_build(dfk_ctx* ctx, const int32_t* pairs /* or NULL */, uint64_t n_pairs, const uint8_t* packed_bases, const uint64_t* base_off /* or NULL: dense */, const uint32_t* read_len,
                    const uint8_t* pq, const uint64_t* pq_off, uint64_t n_reads);
int dfk_walks_build_arrays(dfk_ctx* ctx, uint64_t n_edges, const int32_t* inv, const int32_t* kmers, const uint8_t* edge_packed, const uint64_t* edge_off /* [n_edges + 1], bytes */, uint64_t n_ce,
                           const uint64_t* ce, const uint64_t* read_first /* [n_ce + 1] */, const uint64_t* reads, const int32_t* pairs, uint64_t n_pairs, const uint8_t* packed_bases,
                           const uint64_t* base_off, const uint32_t* read_len, const uint8_t* pq, const uint64_t* pq_off, uint64_t n_reads, uint64_t walks_per_batch /* 0 = what fits */,
                           const char* dir /* NULL = no file */);
int dfk_walks_stats(dfk_ctx* ctx, uint64_t* out /* [DFK_WALKS_WORDS] */);
int dfk_walks_fetch(dfk_ctx* ctx, uint64_t* starts, uint64_t* ee_starts, uint32_t* records, uint64_t* n_walks, void* placed, uint64_t placed_cap, uint64_t* n_placed, uint8_t* bases, uint64_t bases_cap,
                    uint64_t* n_bases);
int dfk_walks_write(dfk_ctx* ctx, const char* dir);

/* ---- the second closer's stack consensus: Stackster's two stacks per pair, their Consensus1 with QUALCAP, the MIN_FLAT zeroing and the
 * conflicting columns per offset (10X/Stackster.cc:396-489, :546-563; ReadStack.cc's Trim, Reverse, Consensus1 with qualities) ----
 * For a pair where both walks placed an entry (a.stack.walks: status 0 and placed > 0 on both sides) Stackster builds a stack a side from
 * the placed entries -- row i the read oriented and lowered as the walk saw it, at offset start -- trims it to its last 400 columns,
 * reverses side 1, and takes Consensus1( con, conq, 100 ) of each: per column four double sums added in row order (0.1 for Q0, 0.2 for
 * Q1 and Q2, q otherwise), con the base of the greatest ( sum, id ) pair (base 3 where nothing covers), conq = min( 100, int( round(
 * val(0) - val(1) ) ) ), zeroed where val(1) > 100 and two rows or more of quality >= 30 show the second base.  conq is then zeroed
 * over every run of 10 equal bases or more of con.  An offset in [-n2, n1) between the two is allowed while fewer than 10 columns have
 * conq 100 on both sides and different bases; the count is kept for every offset.  No stack is stored.  Every other pair has two
 * elements of 0 rows and 0 columns and no conflict entries.  The rule, the plan and the file's layout: csrc/dfk_scons.h.
 *   dfk_scons_build   works from the context's latest dfk_walks_build* result; the read arguments are the reads the walks were made
 *                     from with their PQVec qualities, checked as dfk_cons_build checks them.  DFK_E_STATE without a walks result.
 *   dfk_scons_build_arrays  the same stage on host arrays: the walks in dfk_walks_fetch's forms -- starts [2 * n_pairs + 1], records (8
 *                     u32 a walk), the placed records (16 bytes each) -- and the reads; stacks_per_batch 0 = what fits; with a dir
 *                     the file is written there.
 *   DFK_E_ARG for null arguments, starts that fall or disagree with a record's placed, a placed record that names no read or lies
 *   2^30 columns away, an M that is not the maximum of start + len over a yielding side's records; DFK_E_INPUT for offset tables of
 *   the reads that fall and for a PQVec stream that does not hold its read's length.  A refused call changes nothing: dfk_scons_stats /
 *   _fetch / _write serve the latest result of either build, hbm_held is as before.
 *   dfk_scons_stats   out[DFK_SCONS_WORDS]: the counters below
 *   dfk_scons_fetch   starts ([n_elements + 1] words, or NULL), conflict_first ([n_elements / 2 + 1] words, or NULL), dims (4 u32 an
 *                     element, or NULL), con and conq (a byte a column each; both or neither), the conflict counts (u16 each); NULL
 *                     with cap 0 gives the counts alone; a buffer too small DFK_E_ARG.
 *   dfk_scons_write   into dir (which must exist), whole or not at all.  Little-endian, no byte undefined:
 *                       a.stack.cons  "DFKSCON1" | u64 n = 2 * n_pairs | (n + 1) x u64 starts, in columns | (n_pairs + 1) x u64 first
 *                                     conflict entry of each pair | n x 16-byte { u32 rows, u32 rows_kept, i32 M, u32 cols } | con, a
 *                                     byte a base | conq, a byte each, after the flat pass | the conflict counts, u16 each: n1 + n2 a
 *                                     yielding pair, the offset's at index offset + n2 | zero bytes to a multiple of 8.  Element
 *                                     2 pi + s is side s of pair pi. */
#define DFK_SCONS_WORDS 32
#define DFK_SCONS_PAIRS 0            /* pairs */
#define DFK_SCONS_YIELDS 1           /* pairs with entries placed on both sides: the only ones with stacks */
#define DFK_SCONS_STACKS 2           /* their stacks */
#define DFK_SCONS_ROWS 3             /* rows: the placed records of those stacks */
#define DFK_SCONS_ROWS_KEPT 4        /* rows after Trim */
#define DFK_SCONS_TRIMMED 5          /* stacks with M > 400 */
#define DFK_SCONS_COLUMNS 6          /* columns of all stacks */
#define DFK_SCONS_CELLS 7            /* defined cells added to a sum */
#define DFK_SCONS_CAPPED 8           /* columns whose int( round( val(0) - val(1) ) ) was 100 or more */
#define DFK_SCONS_RECOUNT 9          /* columns the recount zeroed: val(1) > 100, two rows of quality >= 30 on id(1) */
#define DFK_SCONS_FLAT 10            /* columns in runs of 10 equal bases or more: zeroed as flat */
#define DFK_SCONS_ALLOWED 11         /* offsets with fewer than 10 conflicting columns, */
#define DFK_SCONS_DISALLOWED 12      /* and the others */
#define DFK_SCONS_LIVE 13            /* rows whose span meets their stack's window */
#define DFK_SCONS_DECODED 14         /* reads gathered, decoded and lowered, a read once a batch */
#define DFK_SCONS_BATCHES 15         /* batches of stacks */
#define DFK_SCONS_RANGES 16          /* ranges of pairs */
#define DFK_SCONS_US 17              /* microseconds: the build call, */
#define DFK_SCONS_US_COPY 18         /* the live rows and the gather on the host and the copies, */
#define DFK_SCONS_US_DECODE 19       /* decode and lowering, */
#define DFK_SCONS_US_CONS 20         /* the consensus kernel, */
#define DFK_SCONS_US_FLAT 21         /* the flat pass, */
#define DFK_SCONS_US_CONFLICTS 22    /* the conflicts */
#define DFK_SCONS_SUM 23             /* sum and xor over positions i of h(i, value) (k_digest_seq, salt 0x5C05): the dims as u32 words, con, conq, the conflict counts */
#define DFK_SCONS_XOR 24
int dfk_scons_build(dfk_ctx* ctx, const uint8_t* packed_bases, const uint64_t* base_off /* or NULL: dense */, const uint32_t* read_len, const uint8_t* pq, const uint64_t* pq_off, uint64_t n_reads);
int dfk_scons_build_arrays(dfk_ctx* ctx, const uint64_t* starts /* [2 * n_pairs + 1] */, const uint32_t* records /* 8 a walk */, const void* placed, uint64_t n_pairs, const uint8_t* packed_bases,
                           const uint64_t* base_off, const uint32_t* read_len, const uint8_t* pq, const uint64_t* pq_off, uint64_t n_reads, uint64_t stacks_per_batch /* 0 = what fits */,
                           const char* dir /* NULL = no file */);
int dfk_scons_stats(dfk_ctx* ctx, uint64_t* out /* [DFK_SCONS_WORDS] */);
int dfk_scons_fetch(dfk_ctx* ctx, uint64_t* starts, uint64_t* conflict_first, uint32_t* dims, uint64_t* n_elements, uint8_t* con, uint8_t* conq, uint64_t cols_cap, uint64_t* n_cols, uint16_t* counts,
                    uint64_t counts_cap, uint64_t* n_counts);
int dfk_scons_write(dfk_ctx* ctx, const char* dir);

/* ---- Stackster's stack offsets per pair: the rows of one stack searched for the acceptable 8-mers of the other stack's consensus, the
 * bits of every ( row, offset ), the offsets within 20 bits of the best (10X/Stackster.cc:461-645) ----
 * For s in 0, 1 an 8-mer of side s's con is acceptable when neither half is flat and it holds three different bases; every row of the
 * other stack whose 8 cells at l are all defined (lowered quality below 128) and equal an acceptable 8-mer at j proposes offset = ( s
 * == 0 ? j - l : l - j ).  A ( row, offset ) counts once a side, and only where a.stack.cons' conflict count of the offset is below 10.
 * Its bits: over the overlap of con and the stack at that offset the windows of 20 columns or more whose two end cells the row defines,
 * minp = Min T[n][mismatches] over the table of log binomial sums (dfk_offsets'), bits = -minp * 10.0 / 6.0; a result with 20 bits or
 * more.  Per distinct offset the greatest bits; an offset is kept within 20.0 of the pair's best; a pair is closable with 1 to 3 kept
 * offsets.  Every pair that does not yield has no record.  The rule, the plan and the file's layout: csrc/dfk_soffsets.h.
 *   dfk_soffsets_build   works from the context's latest dfk_walks_build* AND dfk_scons_build results; the read arguments are the reads
 *                     they were made from.  DFK_E_STATE without both, or when the consensus was not made by dfk_scons_build from
 *                     these walks.
 *   dfk_soffsets_build_arrays  the same stage on host arrays and without a graph: the walks in dfk_walks_fetch's forms, the reads, the
 *                     stack consensus in dfk_scons_fetch's forms -- cons_starts [2 * n_pairs + 1], dims (4 u32 an element), con,
 *                     conq, conflict_first [n_pairs + 1], counts --; rows_per_batch 0 = what fits, else whole pairs while their live
 *                     rows stay at it (one pair at least); with a dir the file is written there.
 *   DFK_E_ARG for what dfk_scons_build_arrays refuses and for consensus starts that do not begin at 0 or fall, a base above 3, an
 *   element wider than 400 or not as wide as its dims and its walk's M say, a counts table that is not n1 + n2 long for a yielding
 *   pair (0 for another).  A refused call changes nothing: dfk_soffsets_stats / _fetch / _write serve the latest result of either
 *   build, hbm_held is as before.
 *   dfk_soffsets_stats   out[DFK_SOFFSETS_WORDS]: the counters below
 *   dfk_soffsets_fetch   starts ([n_pairs + 1] words, or NULL), words (4 u32 a pair, or NULL), the records (24 bytes each); NULL with
 *                     cap 0 gives the counts alone; a buffer too small DFK_E_ARG.
 *   dfk_soffsets_write   into dir (which must exist), whole or not at all.  Little-endian, no byte undefined:
 *                       a.stack.offsets  "DFKSOFF1" | u64 n_pairs | (n_pairs + 1) x u64 starts, in records | n_pairs x 16-byte { u32
 *                                     seen, u32 results, u32 kept, u32 closable } | 24-byte records { i32 offset, u32 results, f64
 *                                     best_bits, u32 state, u32 0 }, one per distinct offset with a result, ascending; state 0 kept, 1
 *                                     dropped. */
#define DFK_SOFFSETS_WORDS 32
#define DFK_SOFFSETS_PAIRS 0         /* pairs */
#define DFK_SOFFSETS_YIELDS 1        /* pairs with entries placed on both sides: the only ones searched */
#define DFK_SOFFSETS_ROWS 2          /* rows searched: the rows their stacks kept */
#define DFK_SOFFSETS_KMERS 3         /* row 8-mers with all 8 cells defined */
#define DFK_SOFFSETS_ACCEPTABLE 4    /* acceptable 8-mers of con, both sides */
#define DFK_SOFFSETS_HITS 5          /* ( row 8-mer, acceptable con 8-mer ) that are equal */
#define DFK_SOFFSETS_SEEN 6          /* candidates ( s, row, offset ) seen */
#define DFK_SOFFSETS_DISALLOWED 7    /* hits skipped because their offset has 10 conflicting columns or more */
#define DFK_SOFFSETS_LOOKUPS 8       /* look-ups in the table of log binomial sums */
#define DFK_SOFFSETS_RESULTS 9       /* candidates with 20 bits or more */
#define DFK_SOFFSETS_OFFSETS 10      /* distinct offsets with a result: the records */
#define DFK_SOFFSETS_KEPT 11         /* of them kept, */
#define DFK_SOFFSETS_DROPPED 12      /* and dropped as more than 20 bits below the pair's best */
#define DFK_SOFFSETS_PAIRS_0 13      /* pairs with no kept offset, */
#define DFK_SOFFSETS_PAIRS_1 14      /* one, */
#define DFK_SOFFSETS_PAIRS_2 15      /* two, */
#define DFK_SOFFSETS_PAIRS_3 16      /* three, */
#define DFK_SOFFSETS_PAIRS_MORE 17   /* more */
#define DFK_SOFFSETS_CLOSABLE 18     /* pairs with one to three kept offsets */
#define DFK_SOFFSETS_LIVE 19         /* rows whose span meets their stack's window */
#define DFK_SOFFSETS_DECODED 20      /* reads gathered, decoded and lowered, a read once a batch */
#define DFK_SOFFSETS_BATCHES 21      /* batches of pairs */
#define DFK_SOFFSETS_RANGES 22       /* ranges of pairs */
#define DFK_SOFFSETS_US 23           /* microseconds: the build call, */
#define DFK_SOFFSETS_US_COPY 24      /* the live rows and the gather on the host and the copies, */
#define DFK_SOFFSETS_US_DECODE 25    /* decode and lowering, */
#define DFK_SOFFSETS_US_SEARCH 26    /* the search kernel, */
#define DFK_SOFFSETS_US_EMIT 27      /* the scan and the emit */
#define DFK_SOFFSETS_SUM 28          /* sum and xor over positions i of h(i, value) (k_digest_seq, salt 0x50FF): the per-pair words, then the records as u32 words */
#define DFK_SOFFSETS_XOR 29
int dfk_soffsets_build(dfk_ctx* ctx, const uint8_t* packed_bases, const uint64_t* base_off /* or NULL: dense */, const uint32_t* read_len, const uint8_t* pq, const uint64_t* pq_off, uint64_t n_reads);
int dfk_soffsets_build_arrays(dfk_ctx* ctx, const uint64_t* starts /* [2 * n_pairs + 1] */, const uint32_t* records /* 8 a walk */, const void* placed, uint64_t n_pairs, const uint8_t* packed_bases,
                              const uint64_t* base_off, const uint32_t* read_len, const uint8_t* pq, const uint64_t* pq_off, uint64_t n_reads, const uint64_t* cons_starts /* [2 * n_pairs + 1] */,
                              const uint32_t* dims /* 4 an element */, const uint8_t* con, const uint8_t* conq, const uint64_t* conflict_first /* [n_pairs + 1] */, const uint16_t* counts,
                              uint64_t rows_per_batch /* 0 = what fits */, const char* dir /* NULL = no file */);
int dfk_soffsets_stats(dfk_ctx* ctx, uint64_t* out /* [DFK_SOFFSETS_WORDS] */);
int dfk_soffsets_fetch(dfk_ctx* ctx, uint64_t* starts, uint32_t* words, uint64_t* n_pairs, void* records, uint64_t records_cap, uint64_t* n_records);
int dfk_soffsets_write(dfk_ctx* ctx, const char* dir);

/* ---- Stackster's closures per pair: the two stacks trimmed to the edges, merged at each kept offset, Consensus1 of the merged stack
 * (10X/Stackster.cc:712-757; ReadStack.cc's Trim, Merge and Consensus1 with qualities) ----
 * A pair with one to three kept offsets (the state-0 records of a.stack.offsets) gets one closure per kept offset, ascending; every
 * other pair none.  At an offset stack 0 is cut to the columns [0, offset + n2) where it is wider, stack 1 to [-offset, n2) where the
 * offset is negative; rows without a defined cell in the kept columns go.  The merged stack is C = offset + n2 columns wide; per column
 * four doubles take the defined cells of stack 0's rows, then stack 1's, in row order (0.1 for Q0, 0.2 for Q1 and Q2, q otherwise, on
 * the lowered quality); the base of the greatest ( sum, id ) wins, ties to the highest base, a column nothing was added to gives base 3.
 * Where no row is left at all the closure is C columns of base 3 (rowless; no offset a.stack.offsets holds leads there).  The rule,
 * the plan and the file's layout: csrc/dfk_sclosures.h.
 *   dfk_sclosures_build  works from the context's latest dfk_walks_build*, dfk_scons_build AND dfk_soffsets_build results; the read
 *                     arguments are the reads they were made from.  DFK_E_STATE without any of them, or when the consensus was not
 *                     made by dfk_scons_build from these walks or the offsets not by dfk_soffsets_build from this consensus.
 *   dfk_sclosures_build_arrays  the same stage on host arrays and without a graph: the walks in dfk_walks_fetch's forms, the reads, dims
 *                     in dfk_scons_fetch's form (4 u32 an element), the offsets in dfk_soffsets_fetch's forms -- so_starts [n_pairs +
 *                     1], so_words (4 u32 a pair), so_records (24 bytes each) --; closures_per_batch 0 = what fits; with a dir the file
 *                     is written there.
 *   DFK_E_ARG for what dfk_scons_build_arrays refuses and for dims that do not say what the walks do, offsets' starts that do not begin
 *   at 0 or fall, a state other than 0 or 1, offsets of a pair that do not ascend, a kept offset outside [-(n2 - 8), n1 - 8], records
 *   for a pair that does not yield, words whose kept / closable do not say what the records do.  A refused call changes nothing:
 *   dfk_sclosures_stats / _fetch / _write serve the latest result of either build, hbm_held is as before.
 *   dfk_sclosures_stats  out[DFK_SCLOSURES_WORDS]: the counters below
 *   dfk_sclosures_fetch  pair_first ([n_pairs + 1] words, or NULL), starts ([n_closures + 1] words, or NULL), records (4 u32 a closure,
 *                     or NULL), the bases a byte each; NULL with cap 0 gives the counts alone; a buffer too small DFK_E_ARG.
 *   dfk_sclosures_write  into dir (which must exist), whole or not at all.  Little-endian, no byte undefined; a.close.closures' layout:
 *                       a.stack.closures  "DFKSCLS1" | u64 n closures | u64 n_pairs | (n_pairs + 1) x u64 first closure of each pair |
 *                                     (n + 1) x u64 starts, in bases | n x 16-byte { u32 pair, i32 offset, u32 cols, u32 rows } | the
 *                                     bases, a byte each (0..3) | zero bytes to a multiple of 8.
 *   dfk_allclosures_write  the product of the reference's pair traversal (RunStages.cc:290-325): per pair Stackster's closures, then
 *                     CloseGap2's, the pairs in order, as dir/a.closures.fastb (a feudal .fastb).  Host only.  DFK_E_STATE unless the
 *                     context holds a dfk_closures_build and a dfk_sclosures_build result over the same pairs.  out (or NULL):
 *                     { closures, bases, from Stackster, from CloseGap2 }. */
#define DFK_SCLOSURES_WORDS 32
#define DFK_SCLOSURES_PAIRS 0        /* pairs */
#define DFK_SCLOSURES_YIELDS 1       /* pairs with entries placed on both sides */
#define DFK_SCLOSURES_CLOSABLE 2     /* pairs with one to three kept offsets: the only ones whose stacks are touched */
#define DFK_SCLOSURES_NONE 3         /* pairs with no kept offset */
#define DFK_SCLOSURES_OVER 4         /* pairs with more than three */
#define DFK_SCLOSURES_CLOSURES 5     /* closures */
#define DFK_SCLOSURES_COLUMNS 6      /* their columns: the bases */
#define DFK_SCLOSURES_CELLS 7        /* defined cells added to a column's sums */
#define DFK_SCLOSURES_LIVE 8         /* live rows walked: per closure those of its pair's two stacks */
#define DFK_SCLOSURES_ERASED 9       /* rows the two edge trims erased, over all closures */
#define DFK_SCLOSURES_EMPTY 10       /* columns nothing was added to */
#define DFK_SCLOSURES_SHORT 11       /* closures shorter than K */
#define DFK_SCLOSURES_ROWLESS 12     /* closures whose merged stack has no row */
#define DFK_SCLOSURES_DECODED 13     /* reads gathered, decoded and lowered, a read once a batch */
#define DFK_SCLOSURES_BATCHES 14     /* batches of closures */
#define DFK_SCLOSURES_RANGES 15      /* ranges of closable pairs */
#define DFK_SCLOSURES_VISITS 16      /* ( live row, tile of 256 merged columns ) visits */
#define DFK_SCLOSURES_SKIPPED 17     /* of them skipped by the whole workgroup: the row's span misses the tile */
#define DFK_SCLOSURES_US 18          /* microseconds: the build call, */
#define DFK_SCLOSURES_US_COPY 19     /* the live rows and the gather on the host and the copies, */
#define DFK_SCLOSURES_US_DECODE 20   /* decode and lowering, */
#define DFK_SCLOSURES_US_CONS 21     /* the consensus kernel, */
#define DFK_SCLOSURES_US_ROWS 22     /* the row counts */
#define DFK_SCLOSURES_SUM 23         /* sum and xor over positions i of h(i, value) (k_digest_seq, salt 0x5C15): the records as u32 words, then the bases */
#define DFK_SCLOSURES_XOR 24
int dfk_sclosures_build(dfk_ctx* ctx, const uint8_t* packed_bases, const uint64_t* base_off /* or NULL: dense */, const uint32_t* read_len, const uint8_t* pq, const uint64_t* pq_off, uint64_t n_reads);
int dfk_sclosures_build_arrays(dfk_ctx* ctx, const uint64_t* starts /* [2 * n_pairs + 1] */, const uint32_t* records /* 8 a walk */, const void* placed, uint64_t n_pairs, const uint8_t* packed_bases,
                               const uint64_t* base_off, const uint32_t* read_len, const uint8_t* pq, const uint64_t* pq_off, uint64_t n_reads, const uint32_t* dims /* 4 an element */,
                               const uint64_t* so_starts /* [n_pairs + 1] */, const uint32_t* so_words /* 4 a pair */, const void* so_records, uint64_t closures_per_batch /* 0 = what fits */,
                               const char* dir /* NULL = no file */);
int dfk_sclosures_stats(dfk_ctx* ctx, uint64_t* out /* [DFK_SCLOSURES_WORDS] */);
int dfk_sclosures_fetch(dfk_ctx* ctx, uint64_t* pair_first, uint64_t* starts, uint32_t* records, uint64_t* n_pairs, uint64_t* n_closures, uint8_t* bases, uint64_t bases_cap, uint64_t* n_bases);
int dfk_sclosures_write(dfk_ctx* ctx, const char* dir);
int dfk_allclosures_write(dfk_ctx* ctx, const char* dir, uint64_t* out /* [4] or NULL */);

/* ---- the patched graph: the closures go into the assembly (10X/runstages/RunStages.cc:330-360) ----
 * Replaces BuildAll (paths/long/large/GapToyTools4.cc:132-159), buildBigKHBVFromReads( K, allx, 4, &hb3, &allx_paths )
 * (kmers/BigKPather.cc:450-535) and the lines that keep the old edges' paths as to3 / left3 (RunStages.cc:355-358): what TranslatePaths
 * will move the read paths onto the new graph with.  The rule, the shared pieces, the order of work and a.patch.to3's layout:
 * csrc/dfk_patch.h.
 *   dfk_patch_build   works from the context's graph and the closures of BOTH closers: DFK_E_STATE unless the context holds a built
 *                     graph, a dfk_closures_build and a dfk_sclosures_build result made for the same pairs (dfk_allclosures_write's
 *                     test); the closures are taken in the combined list's order.  kmers_per_batch: closure K-mer positions looked up
 *                     at a time, 0 = what fits.
 *   dfk_patch_build_arrays  the same stage on host arrays and without a graph in the context (its K is the context's): the graph as
 *                     inv, to_left, to_right [n_edges], its edges' bases packed as a .fastb packs them, edge e at byte edge_off[e] with
 *                     edge_len[e] bases; the closures as starts [n_closures + 1] into closure_bases (a base a byte, 0-3).  A table that
 *                     does not hold together is DFK_E_ARG: inv no involution or inv[e] not e's reverse complement, an end that is no
 *                     vertex, an edge shorter than K, edges at a vertex that do not share its K-1 bases, a K-mer on two canonical edges; closure starts
 *                     that do not begin at 0 or fall, a closure base above 3.
 *   After any refusal the earlier result is still served.  Every device block comes from the arena and is back on return (hbm_held is
 *   as before); the context's graph, index, filter and pathing state are not touched.
 *   dfk_patch_stats   out[DFK_PATCH_WORDS]: the counters below
 *   dfk_patch_fetch   the sizes (any may be NULL), to3_first ([n_edges + 1]), to3 ([n_to3]), left3 ([n_edges]) and hb3's kmers, inv,
 *                     to_left, to_right ([n_edges3] each); an array that is NULL is left out
 *   dfk_patch_write   into dir (which must exist): hb3's eight graph files as a.patch.{k,hbv,hbx,to_left,to_right,inv,fastb,kmers}, by
 *                     the code that writes a.*, and a.patch.to3 ("DFKPTO31", csrc/dfk_patch.h) */
#define DFK_PATCH_WORDS 40
#define DFK_PATCH_EDGES 0           /* old edges, */
#define DFK_PATCH_CANONICAL 1       /* of them e <= inv[e], */
#define DFK_PATCH_VERTICES 2        /* vertices, */
#define DFK_PATCH_CROSSINGS 3       /* vertex crossings: the (K+1)-mers BuildAll adds */
#define DFK_PATCH_CLOSURES 4        /* closures, */
#define DFK_PATCH_SHORT 5           /* of them shorter than K, */
#define DFK_PATCH_POSITIONS 6       /* their K-mer positions */
#define DFK_PATCH_FOUND 7           /* closure K-mers found on the old edges, */
#define DFK_PATCH_NEW 8             /* not found, */
#define DFK_PATCH_NEW_UNIQUE 9      /* and those after de-duplication: the dictionary's second part */
#define DFK_PATCH_BITS_ADDED 10     /* context bits the closures added to old entries */
#define DFK_PATCH_KMERS3 11         /* hb3: K-mers, */
#define DFK_PATCH_CANONICAL3 12     /* canonical edges, */
#define DFK_PATCH_VERTICES3 13      /* vertices, */
#define DFK_PATCH_EDGES3 14         /* edges, */
#define DFK_PATCH_SINGLE3 15        /* canonical edges of one K-mer, */
#define DFK_PATCH_CYCLE_KMERS 16    /* K-mers on branch-free cycles */
#define DFK_PATCH_PATH1 17          /* old edges whose path has 1, */
#define DFK_PATCH_PATH2 18          /* 2, */
#define DFK_PATCH_PATH3 19          /* 3 or more ids */
#define DFK_PATCH_TO3 20            /* to3 entries */
#define DFK_PATCH_LEFT3 21          /* old edges with left3 != 0 */
#define DFK_PATCH_BATCHES 22        /* batches of closure K-mer positions */
#define DFK_PATCH_US 23             /* microseconds: the build call from its first statement, */
#define DFK_PATCH_US_ENTRIES 24     /* the entries kernel, */
#define DFK_PATCH_US_INDEX 25       /* the index over them and the check, */
#define DFK_PATCH_US_CLOSURES 26    /* the closure K-mers, */
#define DFK_PATCH_US_SORT 27        /* the novel K-mers sorted and merged (host), */
#define DFK_PATCH_US_GRAPH 28       /* the graph kernels, */
#define DFK_PATCH_US_NUMBER 29      /* build_hbv (host), */
#define DFK_PATCH_US_PATHS 30       /* heads, scan and emit, */
#define DFK_PATCH_US_COPY 31        /* the tables unpacked and checked, packing, copies and the paths' layout on the host */
#define DFK_PATCH_SUM 32            /* sum and xor over positions i of h(i, value) (k_digest_seq's h, salt 0x9A7C): to3_first, then to3, then left3 */
#define DFK_PATCH_XOR 33
int dfk_patch_build(dfk_ctx* ctx, uint64_t kmers_per_batch);
int dfk_patch_build_arrays(dfk_ctx* ctx, uint64_t n_edges, uint64_t n_vertices, const int32_t* inv, const int32_t* to_left, const int32_t* to_right, const uint8_t* packed_bases,
                           const uint64_t* edge_off, const uint32_t* edge_len, uint64_t n_closures, const uint64_t* closure_starts, const uint8_t* closure_bases, uint64_t kmers_per_batch);
int dfk_patch_stats(dfk_ctx* ctx, uint64_t* out /* [DFK_PATCH_WORDS] */);
int dfk_patch_fetch(dfk_ctx* ctx, uint64_t* n_edges, uint64_t* n_to3, uint64_t* n_edges3, uint64_t* to3_first, int32_t* to3, int32_t* left3, int32_t* kmers3, int32_t* inv3, int32_t* to_left3,
                    int32_t* to_right3);
int dfk_patch_write(dfk_ctx* ctx, const char* dir);

/* ---- the end of the patching stage: the read paths moved onto the patched graph (TranslatePaths, paths/long/large/GapToyTools4.cc:163-196,
 * and the Validate behind it; 10X/runstages/RunStages.cc:364-371) ----
 * Every placed read becomes a path of ONE hb3 edge with a new offset, or loses its path (and keeps its old offset).  The rule, the
 * bound that lets the device decide every path the pather can make, the plan and the layout: csrc/dfk_translate.h.  The result is a
 * second list of path batches in the arena, batch for batch beside the context's paths, which stay as they are; it is released by
 * dfk_translate_drop, by the next dfk_translate_build*, and with the paths.  A refused call changes nothing and the earlier result is
 * still served.  Not for the ranks of a sharded run.
 *   dfk_translate_build         DFK_E_STATE unless the context holds built paths and a dfk_patch_build result (one made by
 *                               dfk_patch_build_arrays does not count: its graph need not be the paths')
 *   dfk_translate_build_arrays  the same on host arrays and with nothing on the context but its K: to3_first ([n_edges + 1], from 0, not
 *                               falling; a list may be empty), to3 (ids in [0, n_edges3)), left3 ([n_edges]), kmers3 ([n_edges3], >= 1);
 *                               the paths as dfk_hops_build_arrays takes them (first [n_reads + 1], edges, ids in [0, n_edges)) with
 *                               offsets ([n_reads]), cut into batches of reads_per_batch (0 = one).  dir: NULL, or where a.patch.paths is
 *                               written too.  DFK_E_ARG for a null argument, a table that breaks the above, |offset| or |left3| of 2^30 or
 *                               more, n_reads >= 2^31 and a batch of 2^32 bytes.
 *   dfk_translate_stats         out[DFK_TRANSLATE_WORDS]: the counters below
 *   dfk_translate_fetch         offsets[n_reads], first_edge[n_reads + 1], edges (edges_cap >= DFK_TRANSLATE_PLACED), as dfk_paths_fetch
 *   dfk_translate_write         dir/a.patch.paths: the feudal ReadPathVec that ReadPathVec::WriteAll would write of `paths` on return from
 *                               StagePatch, by the code that writes a.paths
 *   dfk_translate_drop          the result's blocks go back to the arena (no result: nothing happens) */
#define DFK_TRANSLATE_WORDS 32
#define DFK_TRANSLATE_READS 0           /* reads, */
#define DFK_TRANSLATE_PLACED_BEFORE 1   /* of them with a path before */
#define DFK_TRANSLATE_STEP2 2           /* taken by the first hb3 edge of to3[path[0]] (start < its Bases), */
#define DFK_TRANSLATE_WALK 3            /* by the walk over the ids, */
#define DFK_TRANSLATE_CLEARED_EMPTY 4   /* cleared: to3[path[0]] is empty, */
#define DFK_TRANSLATE_CLEARED_RANOFF 5  /* cleared: the walk ran off the end of p */
#define DFK_TRANSLATE_HOST 6            /* decided on the host: the walk ran off to3[path[0]] (0 on a context's own paths) */
#define DFK_TRANSLATE_INVALID 7         /* edge ids Validate would refuse (must be 0) */
#define DFK_TRANSLATE_EDGE_CHANGED 8    /* reads placed before whose edge is no longer path[0] (a cleared read's is not), */
#define DFK_TRANSLATE_OFFSET_CHANGED 9  /* whose offset changed */
#define DFK_TRANSLATE_BATCHES 10        /* batches */
#define DFK_TRANSLATE_PLACED 11         /* reads with a path now = the edges of the result */
#define DFK_TRANSLATE_VAR_BYTES 12      /* bytes of the result's variable data */
#define DFK_TRANSLATE_US 13             /* microseconds: the build call from its first statement, */
#define DFK_TRANSLATE_US_DECIDE 14      /* k_tp_decide, */
#define DFK_TRANSLATE_US_HOST 15        /* the host route (copies, the literal rule, k_tp_override), */
#define DFK_TRANSLATE_US_SCAN 16        /* the scans, */
#define DFK_TRANSLATE_US_EMIT 17        /* k_tp_emit, */
#define DFK_TRANSLATE_US_COPY 18        /* tables checked and sent, scratch, counters back */
#define DFK_TRANSLATE_SUM 19            /* the content digest as DFK_CK_PATHS_SUM/XOR form it: over reads r of h(r, offset, lastSkip, edge) */
#define DFK_TRANSLATE_XOR 20
int dfk_translate_build(dfk_ctx* ctx);
int dfk_translate_build_arrays(dfk_ctx* ctx, uint64_t n_edges, const uint64_t* to3_first, const int32_t* to3, const int32_t* left3, uint64_t n_edges3, const int32_t* kmers3,
                               uint64_t n_reads, const uint64_t* first /* [n_reads + 1] */, const int32_t* edges, const int32_t* offsets, uint64_t reads_per_batch, const char* dir);
int dfk_translate_stats(dfk_ctx* ctx, uint64_t* out /* [DFK_TRANSLATE_WORDS] */);
int dfk_translate_fetch(dfk_ctx* ctx, int32_t* offsets, uint64_t* first_edge, int32_t* edges, uint64_t edges_cap);
int dfk_translate_write(dfk_ctx* ctx, const char* dir);
int dfk_translate_drop(dfk_ctx* ctx);

/* ---- rows f-1 / f-2 / f-4 checked where no oracle runs (tests/test_gpu_fullsize_graph.py; DF prints the digests) ----
 * Replaces nothing in the reference (its nearest thing is hbv.CheckSum() / Validate(hbv, paths), 10X/DF.cc:597-598).
 * dfk_paths_digest  fills out[DFK_CHECK_WORDS] with digests that depend on the CONTENT of a.paths, a.paths.inv, a.countsb and
 *                   a.dup only -- not on the batches the reads were pathed in, the passes the dictionary was counted in or the
 *                   entry numbering the k-mer index holds -- and with the graph's identities:
 *   DFK_CK_PATHS_SUM/XOR    over reads r of h(r, offset, lastSkip, edge ids...), the element as a.paths holds it (after dfk_paths_build)
 *   DFK_CK_N_READS / N_PLACED / N_PATH_EDGES
 *   DFK_CK_INV_SUM/XOR      over positions i of a.paths.inv's data of h(i, read id); DFK_CK_INV_STARTS over edges e of h(e, first
 *                           position of e's list); DFK_CK_INV_ENTRIES = the lists' total length     (after dfk_paths_index_write)
 *   DFK_CK_COUNTSB_DIGEST   over edges of h(e, a.countsb[e]); DFK_CK_COUNTSB_SUM their plain sum; DFK_CK_SELF_INVERSE = entries on
 *                           edges that are their own involution: COUNTSB_SUM = 2 * INV_ENTRIES - SELF_INVERSE
 *   DFK_CK_DUP_DIGEST       over pairs p of h(p, a.dup[p]); DFK_CK_DUP_MARKED the number marked               (after dfk_dups_write)
 *   DFK_CK_EDGE_KMERS       sum of the canonical edges' k-mers (= DFK_CK_N_SOLID: every solid k-mer lies on exactly one edge);
 *   DFK_CK_INV_VIOLATIONS   HBV edges e with inv(inv(e)) != e or inv(e) out of range; DFK_CK_N_EDGES
 *   DFK_CK_VALID            DFK_CK_HAS_* bits: which of the three groups are filled
 *   dfk_paths_index_write(ctx, NULL) / dfk_dups_write(ctx, NULL, &n) do everything but write the files.
 * dfk_paths_verify  a second look at every placed read by a kernel that shares no code with the pather (k_path_verify,
 *                   csrc/dfk_check_kernels.h): out[8] = reads placed; paths with an edge id out of range, two consecutive edges
 *                   that do not meet at a vertex (pathPartsToReadPath cuts there, BuildReadQGraph48.cc:1365-1402) or an offset
 *                   behind the first edge; k-mers of placed reads found in the dictionary at a position the path covers; those
 *                   whose (edge, position) is what the path implies there; placed reads with NO such k-mer (the seed a path was
 *                   built from always is one); placed reads all of whose hits agree; dictionary entries whose edge bases are not
 *                   the k-mer; hits at positions outside the path.  [1], [4], [6] must be 0.  Before dfk_paths_index_write /
 *                   dfk_dups_write (they give the k-mer index back).  The reads are those given to dfk_paths_build*. */
#define DFK_CHECK_WORDS 20
enum { DFK_CK_PATHS_SUM = 0, DFK_CK_PATHS_XOR = 1, DFK_CK_N_READS = 2, DFK_CK_N_PLACED = 3, DFK_CK_N_PATH_EDGES = 4,
       DFK_CK_INV_SUM = 5, DFK_CK_INV_XOR = 6, DFK_CK_INV_STARTS = 7, DFK_CK_INV_ENTRIES = 8,
       DFK_CK_COUNTSB_DIGEST = 9, DFK_CK_COUNTSB_SUM = 10, DFK_CK_SELF_INVERSE = 11,
       DFK_CK_DUP_DIGEST = 12, DFK_CK_DUP_MARKED = 13,
       DFK_CK_EDGE_KMERS = 14, DFK_CK_N_SOLID = 15, DFK_CK_INV_VIOLATIONS = 16, DFK_CK_N_EDGES = 17, DFK_CK_VALID = 18 };
#define DFK_CK_HAS_PATHS 1u
#define DFK_CK_HAS_INDEX 2u
#define DFK_CK_HAS_DUPS  4u
int dfk_paths_digest(dfk_ctx* ctx, uint64_t* out /* [DFK_CHECK_WORDS] */);
int dfk_paths_verify(dfk_ctx* ctx, const uint8_t* packed_bases, const uint64_t* base_off, const uint32_t* read_len, uint64_t n_reads,
              uint64_t* out /* [8] */);
int dfk_paths_verify_device(dfk_ctx* ctx, const void* d_packed_bases, uint64_t packed_bytes, const void* d_base_off, const void* d_read_len,
              uint64_t n_reads, uint64_t* out /* [8] */);
/* dfk_paths_verify_arrays  the verifier on paths given as host arrays, for tests that choose (and damage) their paths: the same
 *                   kernel on the context's graph, k-mer index and tables, over `n_reads` reads of any number and their paths --
 *                   offsets[i], and first[i] .. first[i + 1] of `edges` -- laid out as the pather leaves its batches and cut into
 *                   batches of reads_per_batch (0 = one batch).  out[0..7] the eight counters, out[8..9] DFK_CK_PATHS_SUM / _XOR of
 *                   the paths given.  Needs what dfk_paths_verify needs; leaves the context's paths, marks and results alone and
 *                   holds no more of the device afterwards.  Refused before anything is launched (DFK_E_ARG): a null argument,
 *                   first[0] != 0, a falling first, n_reads or first[n_reads] >= 2^31, a batch of 2^32 bytes or more (8 a read, 4
 *                   an edge); DFK_E_INPUT: the reads' offset table, as dfk_paths_verify.  Edge ids and offsets of ANY value are
 *                   let through: they are what the kernel is there to count. */
int dfk_paths_verify_arrays(dfk_ctx* ctx, const uint8_t* packed_bases, const uint64_t* base_off, const uint32_t* read_len, uint64_t n_reads,
              const int32_t* offsets /* [n_reads] */, const uint64_t* first /* [n_reads + 1] */, const int32_t* edges,
              uint64_t reads_per_batch, uint64_t* out /* [10] */);

/* ---- the data-parallel half of ParseBarcodedFastqs (10X/ParseBarcodedFastqs.cc:306-539) ----
 * The host inflates the two .gz files, cuts them into lines and decides where every barcode stands in the output (the buckets
 * are the iteration order of a std::unordered_set, :311-336: a container's business).  For one group of pairs it holds, the
 * device then does the rest:
 *   the order of the pairs   by the place of their barcode, inside a barcode DEScending by (read 1, read 2) as base sequences,
 *                            equal pairs in file order (the list insertion of :434-449) -- a stable radix sort on the sequences
 *   bases -> 2-bit codes     N -> A (:407-412), LSB-first as BaseVec stores them (feudal/FieldVec.h:766-770)
 *   qualities -> PQVec       PQVecEncoder::init/encode (feudal/PQVec.cc:18-127), the block choice AND its cut-back rule
 * dfk_pbf_run takes the reads as the fastq has them (ASCII) and returns the group's share of OUT_HEAD.fastb / .qualp ready to be
 * appended: the pairs' order, the reads' lengths, both files' variable data with their offsets.  Errors as the reference's:
 * DFK_E_INPUT for a quality above 63 ("Your input reads are funny", PQVec.cc:30-35) or a character that is no base.
 * Any context will do (K plays no part); its HBM budget bounds the group. */
#define DFK_PBF_DROP 0xFFFFFFFFu
typedef struct dfk_pbf_input {
    const uint8_t*  seq[2];      /* file 1 / file 2: the held reads' base characters, one read behind the other */
    const uint8_t*  qual[2];     /* their quality characters (phred + 33), same layout */
    const uint64_t* off[2];      /* [m + 1]: where read i starts in seq / qual */
    const uint32_t* rank;        /* [m]: the place of pair i's barcode in the output; 0 = unbarcoded (file order kept);
                                    DFK_PBF_DROP = the pair is left out (READS_PER_BC, :328) */
    uint64_t m;                  /* pairs held */
} dfk_pbf_input;
typedef struct dfk_pbf_output {
    uint64_t n_pairs;            /* pairs written: 2 * n_pairs reads, read 2k = read 1 of pair order[k], 2k+1 its mate */
    const uint32_t* order;       /* [n_pairs] */
    const uint32_t* read_len;    /* [2 n_pairs]: the .fastb fixed data */
    const uint8_t*  fastb_var;  const uint64_t* fastb_off;   /* [2 n_pairs + 1], relative to fastb_var */
    const uint8_t*  qualp_var;  const uint64_t* qualp_off;
    float ms_sort, ms_encode, ms_total;   /* device time: the order; packing + PQVec; the whole call with its transfers */
} dfk_pbf_output;
typedef struct dfk_pbf dfk_pbf;
int  dfk_pbf_run(dfk_ctx* ctx, const dfk_pbf_input* in, dfk_pbf** out);
int  dfk_pbf_result(const dfk_pbf* r, dfk_pbf_output* o);      /* pointers stay valid until dfk_pbf_free */
void dfk_pbf_free(dfk_pbf* r);

/* ---- multi-GPU pieces (one process per GPU; the caller owns the RCCL exchange) ----
 * The reference's only exchange is MapReduceEngine's thread all-to-all ("swizzle",
 * MapReduceEngine.h:345-388): every key goes to the thread that owns hash % T.  Here every
 * k-mer goes to the rank that owns its minimizer bucket (owner = bucket & (world-1); world is
 * a power of two), travelling inside 32-byte super-k-mer records:
 *
 *   dfk_shard_begin       trim this rank's reads; returns its k-mer instance count
 *   <caller: all-reduce the instance counts so that every rank derives the same bucket count>
 *   dfk_shard_plan        passes (equal bucket ranges) this rank needs to fit its HBM (caller takes the max over ranks)
 *   for pass in 0 .. 2^log2_passes - 1:
 *     dfk_shard_partition   kmerize the pass's minimizer buckets into records grouped by destination rank
 *     <caller: all-to-all of send_counts; dfk_shard_recv_buffer; all-to-all of the record bytes, over RCCL/xGMI>
 *     dfk_shard_count       regroup the received records by fine bucket and count them; after the
 *                           last pass this rank holds the solid k-mers it owns, pre-adjacency
 *   dfk_shard_adj_queries neighbour keys of the local solid k-mers, grouped by owner rank
 *   <caller: all-to-all of the 16-byte keys>
 *   dfk_shard_adj_answer  presence of each received key in the local solid set
 *   <caller: all-to-all of the answer bytes back>
 *   dfk_shard_adj_apply   clear the context bits whose neighbour is not solid anywhere
 *
 * Afterwards dfk_solid_count/fetch, dfk_spectrum, dfk_good_lens return this rank's share
 * (solid sets are disjoint; spectra add).  superplus_amd/dist.py drives these with
 * torch.distributed; INTEGRATION.md shows the plain RCCL calls. */
int dfk_shard_begin(dfk_ctx* ctx,
              const void* d_packed_bases, uint64_t packed_bytes, const void* d_base_off,
              const void* d_read_len, const void* d_pq_bytes, uint64_t pq_nbytes,
              const void* d_pq_off, const void* d_bc, uint64_t n_reads,
              int64_t global_read_offset /* index of this shard's first read (ign_bc_below is global) */,
              uint64_t* n_inst_local);
/* The same from host memory, for a host that maps the read files (DF NUM_GPUS=N): the tables are this rank's SLICE of
 * the whole set's tables -- base_off / pq_off keep the whole set's offsets and packed_bases / pq_bytes are the whole
 * set's arrays -- and only the bytes of this rank's reads are uploaded.  The device copies live until the next run. */
int dfk_shard_begin_host(dfk_ctx* ctx,
              const uint8_t* packed_bases, const uint64_t* base_off /* n+1 */, const uint32_t* read_len,
              const uint8_t* pq_bytes, const uint64_t* pq_off /* n+1 */, const int32_t* bc, uint64_t n_reads,
              int64_t global_read_offset, uint64_t* n_inst_local);
int dfk_shard_plan(dfk_ctx* ctx, uint32_t world, uint64_t n_inst_global, uint32_t* log2_passes);
int dfk_shard_partition(dfk_ctx* ctx, uint32_t world, uint64_t n_inst_global, uint32_t log2_passes, uint32_t pass,
              const void** d_records, uint64_t* send_counts /* [world], in 32-byte records */);
/* The same in two steps, for a driver that hides the partition of pass p+2 under the count of pass p (while the
 * records of pass p+1 travel): _begin returns the send buffer and the send counts at once -- the counts are known from
 * the counting scan -- and starts the kernels now (defer = 0) or, on the library's second stream, right behind the
 * k_count of the dfk_shard_count call that follows (defer = 1); _end waits for them and checks that every slice
 * received what the scan counted.  The buffer may be sent only after _end.  One partition at a time; the send buffers
 * of two consecutive passes are alive together, the one of pass p is given back when pass p is counted or pass p+2
 * begun.  dfk_shard_partition = _begin(defer = 0) + _end. */
int dfk_shard_partition_begin(dfk_ctx* ctx, uint32_t world, uint64_t n_inst_global, uint32_t log2_passes, uint32_t pass, int defer,
              const void** d_records, uint64_t* send_counts /* [world], in 32-byte records */);
int dfk_shard_partition_end(dfk_ctx* ctx, uint32_t pass);
/* Room for the records this rank is about to receive, from the library's own HBM budget (so that the
 * send, receive and regroup buffers of a pass are all planned in one place); dfk_shard_count frees it.
 * Optional: dfk_shard_count accepts any device pointer. */
int dfk_shard_recv_buffer(dfk_ctx* ctx, uint64_t n_records, void** d_buf);
int dfk_shard_count(dfk_ctx* ctx, const void* d_records, uint64_t n_records, uint32_t pass);
int dfk_shard_adj_queries(dfk_ctx* ctx, const void** d_keys,
              uint64_t* send_counts /* [world], in 16-byte keys */);
int dfk_shard_adj_answer(dfk_ctx* ctx, const void* d_keys, uint64_t n_keys, void* d_present /* u8[n_keys] */);
int dfk_shard_adj_apply(dfk_ctx* ctx, const void* d_present, uint64_t n_keys);
/* The whole dictionary on ONE rank, for what the reference does with it after createDict whatever its thread count
 * (buildEdges, buildHBVFromEdges, pathReads: BuildReadQGraph48.cc:1636,1664): every other rank sends the entries
 * dfk_shard_dict_share names (32 bytes each, contexts final) to the gathering rank, which receives them into the room
 * dfk_shard_dict_adopt returns (it first gives back what the run's exchange still held: this rank's staged reads, the
 * send / receive buffers) and then declares the dictionary whole: from dfk_shard_dict_whole on the context answers as
 * after a single-GPU count (dfk_solid_count, dfk_write_kvec, dfk_graph_build, dfk_paths_build); the spectrum stays this
 * rank's share. */
int dfk_shard_dict_share(dfk_ctx* ctx, const void** d_entries, uint64_t* n_entries);
int dfk_shard_dict_adopt(dfk_ctx* ctx, uint64_t n_entries, void** d_room);
int dfk_shard_dict_whole(dfk_ctx* ctx);

/* ---- rows f-2 / f-4 of a multi-GPU run: every rank holds the whole dictionary (dfk_shard_dict_adopt on every rank) and has built
 * the same graph; the reads stay sharded by pair range as for the count.  The reference's pathReads is a parallelFor over the reads
 * (paths/long/BuildReadQGraph48.cc:1420-1442), writePathsIndex a sort of (edge, read) pairs (10X/PathsIndex.cc:23-146), MarkDups a
 * group-by (10X/SecretOps.cc:410-566); the caller owns the exchanges (csrc/df_shard.h):
 *   dfk_paths_build(ctx, NULL...)   paths the pair range dfk_shard_begin_host staged (kept under DFK_F_KEEP_INPUTS)
 *   dfk_paths_var_bytes             this rank's share of a.paths' variable data  <caller: all-gather>
 *   dfk_paths_write_part            its elements and offset-table entries at their place in the file (rank of read 0: the control block)
 *   dfk_shard_pidx_pairs            its (edge << 32 | whole-set read id) pairs sorted by edge; send_counts[r] = pairs on the edges
 *                                   rank r owns (edges [r n / world, (r+1) n / world)); counts_host[n_edges] = its reads per edge
 *   <caller: all-to-all of the 8-byte pairs; sum of counts_host over the ranks>
 *   dfk_shard_pidx_write            merges what arrived (stable by edge: sources hold ascending read ranges) and writes this rank's
 *                                   range of a.paths.inv; rank 0 also a.countsb
 *   dfk_shard_dup_keys              {key, score} of every placed read grouped by owner rank = hash(key) % world (16 bytes each)
 *   <caller: all-to-all>            dfk_shard_dup_answer: a byte per received item (1 = not its group's best)  <caller: back>
 *   dfk_shard_dup_write             marks this rank's pairs and writes their bytes of a.dup (rank of pair 0: the header)
 * dfk_paths_digest then returns THIS rank's share of the digests: sums add and xors xor over the ranks. */
int dfk_paths_var_bytes(dfk_ctx* ctx, uint64_t* bytes);
int dfk_paths_write_part(dfk_ctx* ctx, const char* path, uint64_t first_read, uint64_t total_reads, uint64_t var_before, uint64_t var_total);
int dfk_shard_pidx_pairs(dfk_ctx* ctx, uint32_t world, const void** d_pairs, uint64_t* send_counts /* [world] */, uint64_t* counts_host /* [n_edges] */);
int dfk_shard_pidx_write(dfk_ctx* ctx, uint32_t world, uint32_t rank, const void* d_pairs_in, uint64_t n_in, const uint64_t* counts_global /* [n_edges] */, const char* dir);
int dfk_shard_dup_keys(dfk_ctx* ctx, uint32_t world, const void** d_items, uint64_t* send_counts /* [world], 16-byte items */);
int dfk_shard_dup_answer(dfk_ctx* ctx, const void* d_items_in, uint64_t n_in, void* d_answers /* u8[n_in] */);
int dfk_shard_dup_write(dfk_ctx* ctx, const void* d_answers_back, uint64_t n, const char* path, uint64_t first_pair, uint64_t total_pairs, uint64_t* n_marked);

#ifdef __cplusplus
}
#endif
#endif
