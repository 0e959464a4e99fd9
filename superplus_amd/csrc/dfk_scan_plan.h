// superplus_amd/csrc/dfk_scan_plan.h -- the plan of the counting scan: every host decision between the launches of
// scan_begin, scan_keys_piece, scan_range and run_under_upload (dfk.hip).  Host-only: plain functions over read counts,
// byte counts and a handful of constants, so they run on a CPU (tests/cpp/test_scan_plan.cc).  What is decided here:
//   1. whether the scan builds run keys at all and their classes and sub-slices (plan_scan); the room of a class slice, the
//      sizes of the four scratch buffers and how many reads a piece takes (size_scan_keys);
//   2. the pieces of a range of reads, halving towards the end of the reads (scan_piece_sizes);
//   3. which key slice a piece fills and what it waits for (scan_piece_step);
//   4. the grid and the LDS of a scan launch (scan_grid, scan_lds); the overflow list's room; the number of fine buckets;
//   5. under the upload of the bases: the upload's pieces, the offset samples, the reads a piece completes.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <vector>
#include "dfk_fallback.h"   // ceil_log2

namespace dfk {

// ---- what the host and the kernels share
constexpr int PART_THREADS = 128;
constexpr int PART_RING = 2;          // words of its read a lane of the general counting scan (k_partition) keeps staged in LDS
// Per-read run summary written by the counting scan (16 bytes): bits 0-3 = number of runs (super-k-mers) or
// SUMMARY_OVERFLOW, then from bit 8 twelve bits per run: nk (6) | offset of its minimizer from the run's
// first k-mer (6, < W).  The scatter passes rebuild each run's bucket from the 2M bits at that offset
// instead of scanning the read again.
constexpr int SUMMARY_RUNS = 10;
// Sharded runs do not need per-bucket counts on the sending side (the owner regroups what it receives), only
// how many records go to each owner in each pass: bucket space of an owner cut into PART_CLASSES equal
// classes; a pass is a whole number of classes.
constexpr uint32_t PART_CLASSES = 64;

// the run keys of a scan launch (k_scan_count<K, M, true>; dfk_kernels.h "run keys")
struct ScanKeys {
    uint32_t* keys;                   // [n_cls][cap] keys of each class
    unsigned long long* fill;         // [n_cls] keys reserved in each class slice (may pass cap: the rest were counted directly)
    uint64_t cap;                     // room of a class slice
    uint32_t ib;                      // bits of a bucket within its class: log2_nb - min(6, log2_nb)
};
constexpr int SCAN_STAGE = 1536;      // keys a scan block stages (5 B each): with the scan's own 7.5 KB, under 16 KB -- ten blocks a CU at K=40
constexpr uint32_t KEY_SUB_BITS = 14; // buckets of a sub-slice: 2^14 u64 counters = 128 KB of LDS
// LDS of the scan: its runs (bucket and summary field of each), then the class counts or (KEYS) the staging
constexpr size_t SCAN_RUN_LDS = (sizeof(uint32_t) + sizeof(uint16_t)) * SUMMARY_RUNS * PART_THREADS;
constexpr size_t SCAN_STAGE_LDS = (sizeof(uint32_t) + 1) * SCAN_STAGE + (sizeof(unsigned long long) + sizeof(uint32_t)) * PART_CLASSES + sizeof(uint32_t);
static_assert(SCAN_RUN_LDS + SCAN_STAGE_LDS <= 16384, "ten scan blocks a CU (160 KB of LDS)");

// ---- constants of the plan
constexpr uint64_t SCAN_TAIL_READS = 32ull << 20;   // the last piece of a keyed scan whose keys are counted under the next scan
constexpr uint64_t KEY_SCRATCH_MAX = 16ull << 30;   // most the keys' copies may take
constexpr uint32_t SCAN_BLOCKS_PER_CU = 128;        // of a grid-stride scan (12 blocks per CU: 57 ms per 225 M reads, 128: 47 ms)

// DFK_SCAN_KEY_PIECE, DFK_SCAN_KEY_TAIL, DFK_NO_OVERLAP, DFK_SCAN_NO_KEYS: read once per scan (tests switch them within one
// process); DFK_SCAN_BLOCKS (blocks per CU of a scan's grid, 0 = unset): once per process.  scan_switches (dfk.hip) reads the five.
struct ScanSwitches {
    bool key_piece_set = false; uint64_t key_piece = 0;   // set: the scan is keyed whatever its reads, in pieces of at most this
    uint64_t key_tail = SCAN_TAIL_READS;                  // 0: equal pieces
    uint32_t scan_blocks = 0;
    bool no_overlap = false;
    bool no_keys = false;                                 // DFK_SCAN_NO_KEYS: the scan keeps its atomics whatever its reads (tests: the unkeyed kernel at every K)
};

struct ScanInputs {
    int K; uint32_t W, log2_nb, log2_world;
    uint64_t n_reads, packed_bytes;
    bool by_class;                    // sharded: counts per owner and class, no per-bucket counters
    bool register_scan;               // k_scan_count applies (it takes ranges of reads); otherwise the general k_partition
    bool second_stream;
    ScanSwitches sw;
};

// The run keys (k_scan_count<K, 16, true>): class slices, their partition into sub-slices, and per sub-slice
// totals | offsets | cursors -- all scratch, counted a piece of at most piece_reads reads at a time.
// With a second stream the keys of piece i are counted under the scan of piece i + 1: `keys` and `fill` are n_slices = 2
// slices that the pieces take in turn.
struct ScanPlan {
    ScanSwitches sw;
    uint32_t W = 0; uint64_t nb = 0, n_bins = 0, ovf_cap = 0; bool by_class = false, register_scan = false;
    bool keyed = false; uint32_t n_cls = 0, ib = 0, sb = 0, n_sub = 0, n_slices = 1;
    double keys_per_read = 0.0;       // room a read's keys are given
    uint64_t n_reads = 0, cap = 0, piece_reads = 0, tail_reads = 0;
    uint64_t keys_bytes = 0, keys2_bytes = 0, fill_bytes = 0, sub_bytes = 0;
    uint64_t n_subs() const { return (uint64_t)n_cls * n_sub; }
};

// reads whose runs do not fit a summary are listed by the scan itself (two in 10^5 at 2x100 bp); if the list
// outgrows the room set aside for it the summaries are searched instead
inline uint64_t ovf_cap(uint64_t n_reads) { return n_reads / 16 + 1024; }

// ---- 1. the plan
// What does not depend on the arena: the tables' sizes, whether the scan is keyed, the keys' classes and sub-slices.
inline ScanPlan plan_scan(const ScanInputs& in)
{
    ScanPlan p;
    p.sw = in.sw; p.W = in.W; p.n_reads = in.n_reads; p.by_class = in.by_class; p.register_scan = in.register_scan;
    p.nb = 1ull << in.log2_nb;
    p.n_bins = 2ull * (PART_CLASSES << in.log2_world);
    p.ovf_cap = ovf_cap(in.n_reads);
    // keys a read makes: its first run and about two per W + 1 k-mers (random minimizers).  The keys pay where that is
    // four or more (at 2 x 100 bp: K=40, 5.7 runs a read, the scan 505 -> 409 ms; K=48, 4.1, 368 -> 333); at K=60 (2.8)
    // the counting kernels cost more than the atomics they replace (284 -> 313 ms), and the scan keeps its atomics
    const double runs = in.n_reads ? 1.0 + 2.0 * std::max(0.0, 4.0 * (double)in.packed_bytes / (double)in.n_reads - in.K + 1) / (in.W + 1) : 0.0;
    p.keyed = !in.by_class && in.register_scan && in.n_reads && (runs >= 3.5 || in.sw.key_piece_set) && !in.sw.no_keys;
    if (!p.keyed) return p;
    const uint32_t cb = std::min<uint32_t>(6, in.log2_nb);
    p.ib = in.log2_nb - cb; p.n_cls = 1u << cb;
    p.sb = std::min(KEY_SUB_BITS, p.ib); p.n_sub = 1u << (p.ib - p.sb);
    // a quarter to spare for reads longer than the mean and classes fuller than the mean (what still does not fit is
    // counted by the global atomic)
    p.keys_per_read = 1.25 * runs;
    p.n_slices = in.second_stream && !in.sw.no_overlap ? 2 : 1;
    // the last piece's keys have no scan to be counted under: the pieces halve towards the end of the reads, down to
    // tail_reads (profiles/r07_scan_overlap.txt: flat from 0 to 64 M reads; every extra piece is a k_keys_count launch)
    p.tail_reads = in.sw.key_tail;
    return p;
}

// The room of a keyed scan, once its tables are allocated: largest_allocatable is the arena's at that moment.
inline void size_scan_keys(ScanPlan& p, uint64_t largest_allocatable)
{
    const double per_read = p.keys_per_read;
    // the keys' copies (a piece's slices, or two pieces' when they are counted under the next scan; their partition); at
    // most a third of what the arena can still give, and never more than KEY_SCRATCH_MAX, so that the pass plan after
    // the scan finds the arena as it was
    const uint32_t copies = p.n_slices + 1;
    const uint64_t want = 4ull * copies * (uint64_t)(per_read * (double)p.n_reads) + 4ull * copies * p.n_cls;
    const uint64_t room = std::min<uint64_t>(std::min(want, KEY_SCRATCH_MAX), largest_allocatable / 3);
    p.cap = std::max<uint64_t>(1024, room / (4 * copies) / p.n_cls) & ~3ull;   // (16-byte loads of the slices)
    p.piece_reads = std::max<uint64_t>(PART_THREADS, (uint64_t)((double)(p.cap * p.n_cls) / per_read));
    if (p.sw.key_piece_set) p.piece_reads = std::max<uint64_t>(1, std::min<uint64_t>(p.piece_reads, p.sw.key_piece));
    p.keys_bytes = p.n_slices * p.cap * p.n_cls * 4;
    p.keys2_bytes = p.cap * p.n_cls * 4;
    p.fill_bytes = p.n_slices * p.n_cls * 8;
    p.sub_bytes = (3 * p.n_subs() + 1) * 8;
}

// ---- 2. the pieces of a range of n reads
// Of piece_reads, and -- where the range ends the reads and the keys are counted under the next scan -- halving over the
// last ones down to tail_reads, so that little is left to count when the last scan ends (a piece's counting takes
// under half its scan's time).
inline std::vector<uint64_t> scan_piece_sizes(const ScanPlan& p, uint64_t n, bool last)
{
    std::vector<uint64_t> tail;
    uint64_t t_sum = 0;
    if (last && p.n_slices > 1 && p.tail_reads)
        for (uint64_t t = p.tail_reads; t < p.piece_reads && t_sum + t < n; t *= 2) { tail.push_back(t); t_sum += t; }
    std::vector<uint64_t> v;
    const uint64_t body = n - t_sum, nb = (body + p.piece_reads - 1) / p.piece_reads;
    for (uint64_t i = 0, at = 0; i < nb; ++i) { const uint64_t e = body * (i + 1) / nb; v.push_back(e - at); at = e; }
    v.insert(v.end(), tail.rbegin(), tail.rend());
    return v;
}

// ---- 3. piece i of a job (counted across its ranges)
// Two slices: piece i's scan fills slice i % 2 once the partition that read the slice last (piece i - 2's) is done; its
// subcount | offsets | partition write keys2 and the sub-slice tables, which the count of piece i - 1 reads: they wait for it.
struct PieceStep { uint32_t slice; bool wait_slice_reader, wait_prev_count; };

inline PieceStep scan_piece_step(const ScanPlan& p, uint64_t i)
{
    const bool two = p.n_slices > 1;
    return PieceStep{two ? (uint32_t)(i & 1) : 0u, two && i >= 2, two && i >= 1};
}

// ---- 4. launches
// Blocks of a scan over n reads on `cus` CUs: a block per PART_THREADS reads; the keyed scan and the scan by class are
// grid-stride (the class counts and the staged keys are flushed once per block) at SCAN_BLOCKS_PER_CU, the others only
// under DFK_SCAN_BLOCKS.
inline unsigned scan_grid(const ScanPlan& p, uint64_t n, unsigned cus)
{
    const uint64_t blocks = (n + PART_THREADS - 1) / PART_THREADS;
    const uint64_t per_cu = p.sw.scan_blocks ? p.sw.scan_blocks : p.keyed || p.by_class ? SCAN_BLOCKS_PER_CU : 0;
    return (unsigned)(per_cu ? std::min<uint64_t>(blocks, per_cu * cus) : blocks);
}

// LDS bytes of a block of the scan the plan selects: keyed, register or general
inline size_t scan_lds(const ScanPlan& p)
{
    if (p.keyed) return SCAN_RUN_LDS + SCAN_STAGE_LDS;
    const size_t window = (sizeof(uint32_t) + 1) * p.W * PART_THREADS + sizeof(uint32_t) * PART_RING * PART_THREADS;
    return (p.register_scan ? SCAN_RUN_LDS : window) + (p.by_class ? p.n_bins * 4 : 0);
}

// Fine buckets of ~430-850 instances (the count is a power of two); an item packs several of them up to its
// instance budget.  Measured on configs[1] at K = 40/48/60: 2^27 buckets beat 2^28 (the scan's atomics run on a
// 1 GB counter table instead of 2 GB: -7..-23 ms) and 2^26 (items overflow their tables: +190 ms).
// (When sharded, the record header keeps 24 bits of the bucket id inside the pass for the receiver's
// regroup: dfk_shard_plan asks for enough passes that a pass has <= 2^24 buckets per owner.)
inline uint32_t pick_log2_nb(uint64_t n_inst, uint32_t log2_world, uint64_t inst_per_bucket)
{
    uint32_t l = ceil_log2(n_inst / inst_per_bucket + 1);
    l = std::max<uint32_t>(l, 4 + log2_world);
    return std::min<uint32_t>(l, 28);
}

// ---- 5. the scan under the upload of the bases (run_under_upload)
// bytes of a piece of the upload; seg_switch: DFK_UPLOAD_SEGMENT, 0 = unset (tests: small pieces)
inline uint64_t upload_segment_bytes(uint64_t packed_bytes, uint64_t seg_switch)
{
    return seg_switch ? std::max<uint64_t>(64, seg_switch & ~63ull) : std::max<uint64_t>(256ull << 20, ((packed_bytes / 12) + (64ull << 20)) & ~((64ull << 20) - 1));
}

// where the reads end, coarsely: entry min(i * stride, n) of the offset table for i < n_samp, read back once
struct OffsetSampling { uint64_t stride, n_samp; };
inline OffsetSampling offset_sampling(uint64_t n_reads)
{
    const uint64_t stride = std::max<uint64_t>(1, (n_reads + 32767) / 32768);
    return OffsetSampling{stride, n_reads / stride + 2};
}

// reads whose bases end at or before `bytes` (a multiple of the stride, or all)
inline uint64_t reads_within(const std::vector<uint64_t>& samp, uint64_t stride, uint64_t n, uint64_t bytes)
{
    const uint64_t i = (uint64_t)(std::upper_bound(samp.begin(), samp.end(), bytes) - samp.begin());   // samp[i-1] <= bytes < samp[i]
    return i ? std::min<uint64_t>((i - 1) * stride, n) : 0;
}

} // namespace dfk
