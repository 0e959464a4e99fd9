// tests/cpp/test_scan_plan.cc -- the counting scan's plan (superplus_amd/csrc/dfk_scan_plan.h) on a CPU: tables of what the
// scan's host code computed for fixed inputs before the plan moved into the header (scan_plan_expected.h), the
// properties every plan must have over seeded random cases, and the per-piece step replayed against a model of the two
// key slices.  One "name: ok" line per case, exit status 1 if any failed.
//   g++ -O1 -std=c++17 -Wall -o test_scan_plan tests/cpp/test_scan_plan.cc && ./test_scan_plan
#include "../../superplus_amd/csrc/dfk_scan_plan.h"
#include "scan_plan_expected.h"
#include <bitset>
#include <cstdio>
#include <functional>
#include <random>

using namespace dfk;

static int g_bad = 0;
#define CHECK(x) do { if (!(x)) { if (++g_bad <= 5) printf("  line %d: %s\n", __LINE__, #x); } } while (0)
static int done(const char* name) { printf("%s: %s\n", name, g_bad ? "FAILED" : "ok"); const int b = g_bad; g_bad = 0; return b != 0; }
template <class T, size_t N> constexpr size_t len(const T (&)[N]) { return N; }

static uint64_t fnv(const std::vector<uint64_t>& v) { uint64_t h = 1469598103934665603ull; for (uint64_t x : v) { h ^= x; h *= 1099511628211ull; } return h; }

// the plan of a row of X_PLAN (its first 14 columns), as scan_begin makes it
static ScanPlan plan_of(const uint64_t* r)
{
    ScanSwitches sw;
    sw.key_piece_set = r[9] != 0; sw.key_piece = r[10];
    if (r[11]) sw.key_tail = r[12];
    sw.no_overlap = r[13] != 0;
    const int K = (int)r[0];
    ScanPlan p = plan_scan(ScanInputs{K, (uint32_t)K - 16 + 1, (uint32_t)r[1], (uint32_t)r[2], r[3], r[4], r[5] != 0, r[6] != 0, r[7] != 0, sw});
    if (p.keyed) size_scan_keys(p, r[8]);
    return p;
}

// ------------------------------------------------------------------ tables
static int test_plan_table()
{
    const size_t n_rows = len(X_PLAN) / X_PLAN_COLS;
    CHECK(len(X_PLAN) % X_PLAN_COLS == 0 && n_rows > 300);
    bool floor_cap = false, floor_piece = false, seen_keyed[2] = {false, false}, sub_lt = false, sub_gt = false, cls_lt = false;
    for (size_t i = 0; i < n_rows; ++i) {
        const uint64_t* r = X_PLAN + i * X_PLAN_COLS;
        const uint64_t* w = r + 14;
        const ScanPlan p = plan_of(r);
        CHECK(p.keyed == (w[0] != 0) && p.n_cls == w[1] && p.ib == w[2] && p.sb == w[3] && p.n_sub == w[4] && p.n_slices == w[5]);
        CHECK(p.cap == w[6] && p.piece_reads == w[7] && p.tail_reads == w[8]);
        CHECK(p.keys_bytes == w[9] && p.keys2_bytes == w[10] && p.fill_bytes == w[11] && p.sub_bytes == w[12]);
        CHECK(p.ovf_cap == w[13] && ovf_cap(r[3]) == w[13] && p.n_bins == w[14] && p.W == w[15] && p.nb == 1ull << r[1]);
        seen_keyed[p.keyed] = true;
        if (p.keyed) {
            floor_cap |= p.cap == 1024; floor_piece |= p.piece_reads == (uint64_t)PART_THREADS && !p.sw.key_piece_set;
            sub_lt |= p.ib < KEY_SUB_BITS; sub_gt |= p.ib > KEY_SUB_BITS; cls_lt |= p.n_cls < 64;
        }
    }
    CHECK(floor_cap && floor_piece && seen_keyed[0] && seen_keyed[1] && sub_lt && sub_gt && cls_lt);   // the table reaches what it is there for
    // row 0, the default benchmark: nine pieces -- five equal ones, then 256 M, 128 M, 64 M and 32 M reads, as the
    // timeline of profiles/r07_scan_overlap.txt shows them (five scans of ~30 ms, then 30.9, 17.2, 8.9 and 4.5 ms)
    const ScanPlan p = plan_of(X_PLAN);
    CHECK(X_PLAN[0] == 48 && X_PLAN[1] == 27 && X_PLAN[3] == 1800000000ull && X_PLAN[4] == 45000000000ull);
    CHECK(p.keyed && p.n_slices == 2 && p.n_cls == 64 && p.n_sub == 128 && p.keys_bytes + p.keys2_bytes <= KEY_SCRATCH_MAX);
    const std::vector<uint64_t> v = scan_piece_sizes(p, 1800000000ull, true);
    const std::vector<uint64_t> want = {259336704ull, 259336704ull, 259336704ull, 259336704ull, 259336704ull, 256ull << 20, 128ull << 20, 64ull << 20, 32ull << 20};
    CHECK(v == want);
    return done("the key plan against the recorded table (K = 40, 48, 60; both sides of every threshold; the default benchmark's nine pieces)");
}

static int test_piece_table()
{
    const size_t n_rows = len(X_PLAN) / X_PLAN_COLS;
    size_t at = 0, n_lists = 0, n_tails = 0;
    for (size_t i = 0; i < n_rows; ++i) {
        const ScanPlan p = plan_of(X_PLAN + i * X_PLAN_COLS);
        if (!p.keyed) continue;
        for (int k = 0; k < 6; ++k) {
            if (at + 4 > len(X_PIECES)) { CHECK(!"X_PIECES ends early"); return done("piece sizes against the recorded table"); }
            const uint64_t n = X_PIECES[at], last = X_PIECES[at + 1], count = X_PIECES[at + 2], hash = X_PIECES[at + 3];
            at += 4;
            const std::vector<uint64_t> v = scan_piece_sizes(p, n, last != 0);
            CHECK(v.size() == count && fnv(v) == hash);
            if (count <= 12) { for (size_t j = 0; j < count && j < v.size(); ++j) CHECK(at + j < len(X_PIECES) && v[j] == X_PIECES[at + j]); at += count; }
            ++n_lists; n_tails += v.size() >= 2 && v.back() == p.tail_reads && v[v.size() - 2] == 2 * p.tail_reads;
        }
    }
    CHECK(at == len(X_PIECES) && n_lists > 1000 && n_tails > 50);
    return done("piece sizes against the recorded table");
}

static int test_launch_tables()
{
    CHECK(len(X_GRID) % 6 == 0 && len(X_LDS) % 6 == 0);
    for (size_t i = 0; i + 5 < len(X_GRID); i += 6) {
        const uint64_t* r = X_GRID + i;
        ScanPlan p; p.keyed = r[0] == 0; p.register_scan = r[0] <= 1; p.by_class = r[1] != 0; p.sw.scan_blocks = (uint32_t)r[3];
        CHECK(scan_grid(p, r[2], (unsigned)r[4]) == r[5]);
    }
    for (size_t i = 0; i + 5 < len(X_LDS); i += 6) {
        const uint64_t* r = X_LDS + i;
        const int K = (int)r[0];
        ScanInputs in{K, (uint32_t)K - 16 + 1, 27, (uint32_t)r[1], 1000, 25000, r[2] != 0, true, true, ScanSwitches()};
        ScanPlan p = plan_scan(in);
        if (!r[2]) { ScanPlan k = p; k.keyed = true; CHECK(scan_lds(k) == r[3]); }
        p.keyed = false;
        CHECK(scan_lds(p) == r[4]);
        p.register_scan = false;
        CHECK(scan_lds(p) == r[5]);
    }
    CHECK(SCAN_RUN_LDS + SCAN_STAGE_LDS == X_LDS[3]);
    return done("scan grids (the three rules, DFK_SCAN_BLOCKS set and unset) and LDS bytes against the recorded tables");
}

static int test_small_tables()
{
    for (size_t i = 0; i + 3 < len(X_LOG2NB); i += 4) CHECK(pick_log2_nb(X_LOG2NB[i], (uint32_t)X_LOG2NB[i + 1], X_LOG2NB[i + 2]) == X_LOG2NB[i + 3]);
    for (size_t i = 0; i + 2 < len(X_SEGMENT); i += 3) CHECK(upload_segment_bytes(X_SEGMENT[i], X_SEGMENT[i + 1]) == X_SEGMENT[i + 2]);
    for (size_t i = 0; i + 2 < len(X_SAMPLING); i += 3) { const OffsetSampling s = offset_sampling(X_SAMPLING[i]); CHECK(s.stride == X_SAMPLING[i + 1] && s.n_samp == X_SAMPLING[i + 2]); }
    return done("pick_log2_nb, upload segments and offset sampling against the recorded tables");
}

// an offset table of n reads and its samples as k_sample_u64 takes them: entry min(i * stride, n)
static std::vector<uint64_t> samples_of(const std::vector<uint64_t>& off, uint64_t n, const OffsetSampling& s)
{
    std::vector<uint64_t> samp(s.n_samp);
    for (uint64_t i = 0; i < s.n_samp; ++i) samp[i] = off[std::min(i * s.stride, n)];
    return samp;
}

static int test_within_table()
{
    uint64_t n_now = ~0ull; std::vector<uint64_t> off, samp; OffsetSampling s{};
    for (size_t i = 0; i + 2 < len(X_WITHIN); i += 3) {
        const uint64_t n = X_WITHIN[i];
        if (n != n_now) {
            off.assign(n + 1, 0);
            for (uint64_t k = 0; k < n; ++k) off[k + 1] = off[k] + (k % 7 == 6 ? 13 : 25);
            s = offset_sampling(n); samp = samples_of(off, n, s); n_now = n;
        }
        CHECK(reads_within(samp, s.stride, n, X_WITHIN[i + 1]) == X_WITHIN[i + 2]);
    }
    return done("reads_within against the recorded table");
}

// ------------------------------------------------------------------ properties
static uint64_t log_uniform(std::mt19937_64& rng, uint64_t hi) { const uint64_t v = rng() >> (rng() % 64); return hi == ~0ull ? v : v % (hi + 1); }

static int test_plan_properties(std::mt19937_64& rng)
{
    int n_keyed = 0, n_tail = 0;
    for (int it = 0; it < 10000; ++it) {
        const int Ks[3] = {40, 48, 60}, K = Ks[rng() % 3];
        const uint32_t lb = 4 + (uint32_t)(rng() % 25), lw = (uint32_t)(rng() % std::min<uint32_t>(4, lb - 3));
        const uint64_t n_reads = 1 + log_uniform(rng, 1800000000ull - 1);
        const double L = (it % 9 == 0) ? 500.0 + (double)(rng() % 20000) : 30.0 + (double)(rng() % 300);
        const uint64_t room = (it % 11 == 0) ? rng() % 100000 : log_uniform(rng, 150000000000ull);
        ScanSwitches sw;
        if (rng() % 3 == 0) { sw.key_piece_set = true; sw.key_piece = (rng() % 4 == 0) ? rng() % 3 : log_uniform(rng, 1ull << 36); }
        if (rng() % 2 == 0) sw.key_tail = (rng() % 4 == 0) ? 0 : log_uniform(rng, 1ull << 20);   // (unset: 32 M reads, beyond most of these ranges)
        sw.no_overlap = rng() % 4 == 0;
        const bool two_streams = rng() % 4 != 0;
        ScanPlan p = plan_scan(ScanInputs{K, (uint32_t)K - 15, lb, lw, n_reads, (uint64_t)((double)n_reads * L / 4.0), rng() % 8 == 0, rng() % 8 != 0, two_streams, sw});
        CHECK(p.nb == 1ull << lb && p.n_bins == 2ull * (PART_CLASSES << lw) && p.ovf_cap == ovf_cap(n_reads) && p.ovf_cap > n_reads / 16);
        if (!p.keyed) { CHECK(p.n_slices == 1 && p.cap == 0); continue; }
        ++n_keyed;
        size_scan_keys(p, room);
        CHECK(!p.by_class && p.register_scan);
        CHECK(p.n_slices == (two_streams && !sw.no_overlap ? 2u : 1u));
        CHECK(((uint64_t)p.n_cls << p.ib) == (1ull << lb) && ((uint64_t)p.n_sub << p.sb) == (1ull << p.ib));      // classes x buckets of a class, sub-slices x buckets of a sub-slice
        CHECK(p.n_cls <= 64 && p.sb <= KEY_SUB_BITS && (p.n_sub == 1 || p.sb == KEY_SUB_BITS));
        CHECK(p.cap % 4 == 0 && p.cap >= 1024);
        const uint64_t copies = p.n_slices + 1;
        CHECK(p.keys_bytes == p.n_slices * p.cap * p.n_cls * 4 && p.keys2_bytes == p.cap * p.n_cls * 4);
        CHECK(p.fill_bytes == p.n_slices * p.n_cls * 8 && p.sub_bytes == (3 * p.n_subs() + 1) * 8);
        // n_slices + 1 copies of the keys fit the room given (a third of the arena's block, KEY_SCRATCH_MAX), the floor apart
        CHECK(p.cap == 1024 || (p.keys_bytes + p.keys2_bytes <= room / 3 && p.keys_bytes + p.keys2_bytes <= KEY_SCRATCH_MAX));
        CHECK(p.keys_bytes + p.keys2_bytes == copies * p.cap * p.n_cls * 4);
        CHECK(p.piece_reads >= 1 && (sw.key_piece_set || p.piece_reads >= (uint64_t)PART_THREADS));
        if (sw.key_piece_set) CHECK(p.piece_reads <= std::max<uint64_t>(1, sw.key_piece));
        CHECK(p.tail_reads == sw.key_tail);
        // ---- the pieces of a range
        const uint64_t n = 1 + rng() % std::min<uint64_t>(n_reads, 300 * p.piece_reads);
        const bool last = rng() % 2;
        const std::vector<uint64_t> v = scan_piece_sizes(p, n, last);
        uint64_t sum = 0;
        for (uint64_t m : v) { sum += m; CHECK(m >= 1 && m <= p.piece_reads); }
        CHECK(sum == n);
        // the tail: tail_reads, doubling backwards while a piece stays below piece_reads and a read is left for the body
        size_t m_tail = 0;
        if (last && p.n_slices > 1 && p.tail_reads)
            for (uint64_t t = p.tail_reads, s = 0; t < p.piece_reads && s + t < n; s += t, t *= 2) ++m_tail;
        CHECK(v.size() > m_tail);
        if (v.size() <= m_tail) continue;
        for (size_t j = 0; j < m_tail; ++j) CHECK(v[v.size() - 1 - j] == p.tail_reads << j);              // strictly halving, ends at tail_reads
        n_tail += m_tail > 0;
        // the body: equal pieces (they differ by a read at most), as few as piece_reads allows
        const size_t n_body = v.size() - m_tail;
        uint64_t lo = ~0ull, hi = 0, body = 0;
        for (size_t j = 0; j < n_body; ++j) { lo = std::min(lo, v[j]); hi = std::max(hi, v[j]); body += v[j]; }
        CHECK(hi - lo <= 1 && n_body == (body + p.piece_reads - 1) / p.piece_reads);
        if (!(last && p.n_slices > 1)) CHECK(m_tail == 0);                                                 // no tail but on the range that ends the reads, with two slices
    }
    CHECK(n_keyed > 3000 && n_tail > 300);                                                                 // (the cases reach both)
    return done("plans: geometry, room, scratch sizes; pieces sum to the range, within piece_reads, the tail halves down to tail_reads (10^4 cases)");
}

static int test_within_properties(std::mt19937_64& rng)
{
    int reached = 0;
    for (int it = 0; it < 10000; ++it) {
        const uint64_t n = (it % 50 == 0) ? 32768 + rng() % 70000 : 1 + rng() % 3000;
        std::vector<uint64_t> off(n + 1, 0);
        const uint64_t mean = 1 + rng() % 60;
        for (uint64_t k = 0; k < n; ++k) off[k + 1] = off[k] + ((rng() % 5 == 0) ? 0 : rng() % (2 * mean));   // (reads without bases among them)
        const OffsetSampling s = offset_sampling(n);
        CHECK(s.stride >= 1 && (s.n_samp - 1) * s.stride >= n && s.n_samp <= 32768 + 2);                     // the samples reach the last read; a bounded read-back
        const std::vector<uint64_t> samp = samples_of(off, n, s);
        uint64_t before = 0, sent = 0;
        const uint64_t seg = upload_segment_bytes(off[n], 1 + rng() % (off[n] / 4 + 64));
        CHECK(seg >= 64 && seg % 64 == 0);
        for (int step = 0; step < 40; ++step) {
            if (step % 3 != 2) sent = std::min(off[n] + 1, sent + seg);
            const uint64_t bytes = step % 3 == 2 ? rng() % (off[n] + 2) : sent;                               // the upload's pieces, and anywhere
            const uint64_t r = reads_within(samp, s.stride, n, bytes);
            CHECK(r <= n && (r == n || r % s.stride == 0));
            CHECK(off[r] <= bytes);                                                                           // no read passed whose bases end beyond `bytes`
            if (bytes < off[n]) CHECK(r < n); else ++reached;                                                 // all reads only once all bases are there
            if (step % 3 != 2) { CHECK(r >= before); before = r; }                                            // monotone
            const uint64_t r2 = reads_within(samp, s.stride, n, bytes + 1 + rng() % 100);
            CHECK(r2 >= r);
        }
    }
    CHECK(reached > 1000);
    return done("reads_within: monotone, never beyond the bytes sent, all reads only when every base has arrived (10^4 cases)");
}

// ------------------------------------------------------------------ the per-piece step
// scan_range | scan_keys_piece | scan_keys_count | scan_end (dfk.hip) as a sequence of operations on two streams, with the
// events they record and wait for; `step` decides what scan_piece_step decides there.  An operation's predecessors are
// what its stream had seen when it was issued: the stream's own earlier operations and those behind every event waited for.
struct Replay {
    using Set = std::bitset<256>;
    enum Kind { SCAN, PART, COUNT };
    struct Op { Kind kind; uint64_t piece; uint32_t slice; Set before; };
    std::vector<Op> ops;
    Set seen[2];                                                        // by stream: 0 = the main stream, 1 = the second
    Set ev_scan, ev_count, ev_part[2];
    uint64_t n_pieces = 0; bool count_due = false;
    std::vector<int> counted;
    uint32_t n_slices;
    std::function<PieceStep(uint64_t)> step;

    void issue(int stream, Kind k, uint64_t piece, uint32_t slice) { ops.push_back(Op{k, piece, slice, seen[stream]}); seen[stream].set(ops.size() - 1); }
    void keys_count()
    {
        if (n_slices > 1) seen[0] |= ev_part[step(n_pieces - 1).slice];
        issue(0, COUNT, n_pieces - 1, 0);
        if (n_pieces - 1 < counted.size()) ++counted[n_pieces - 1];
        if (n_slices > 1) ev_count = seen[0];
        count_due = false;
    }
    void piece()
    {
        const bool two = n_slices > 1;
        const PieceStep st = step(n_pieces);
        const int ks = two ? 1 : 0;
        if (st.wait_slice_reader) seen[0] |= ev_part[st.slice];
        issue(0, SCAN, n_pieces, st.slice);
        if (two) {
            ev_scan = seen[0];
            if (count_due) keys_count();
            seen[ks] |= ev_scan;
            if (st.wait_prev_count) seen[ks] |= ev_count;
        }
        issue(ks, PART, n_pieces, st.slice);
        if (two) ev_part[st.slice] = seen[ks];
        ++n_pieces; count_due = true;
        if (!two) keys_count();
    }
    void range(uint64_t pieces, bool last) { for (uint64_t i = 0; i < pieces; ++i) piece(); if (last && count_due) keys_count(); }
    void end() { if (count_due) keys_count(); }

    // violations of: no slice rewritten before the partition that read it is done; no partition (it writes keys2 and the
    // sub-slice tables) before its own scan, nor before the count that read them; no count before its partition
    int violations() const
    {
        int bad = 0;
        for (size_t a = 0; a < ops.size(); ++a)
            for (size_t b = 0; b < ops.size(); ++b) {
                const Op &x = ops[a], &y = ops[b];
                bool must = false;                                      // must y be done before x starts?
                if (x.kind == SCAN && y.kind == PART) must = y.piece < x.piece && y.slice == x.slice;
                if (x.kind == PART && y.kind == SCAN) must = y.piece == x.piece;
                if (x.kind == PART && y.kind == COUNT) must = y.piece < x.piece;
                if (x.kind == COUNT && y.kind == PART) must = y.piece == x.piece;
                if (x.kind == COUNT && y.kind == COUNT) must = y.piece < x.piece;   // (both add into the bucket table from keys2: in order)
                if (must && !x.before.test(b)) ++bad;
            }
        return bad;
    }
};

static int test_piece_steps()
{
    const std::vector<std::vector<uint64_t>> splits = {{20}, {1, 1, 1, 17}, {3, 1, 5, 2, 9}, {7, 13}, {19, 1}};
    for (uint32_t n_slices : {1u, 2u})
        for (const auto& ranges : splits)
            for (int drained_by_end : {0, 1}) {
                ScanPlan p; p.keyed = true; p.n_slices = n_slices;
                Replay r; r.n_slices = n_slices; r.counted.assign(20, 0);
                r.step = [&](uint64_t i) { return scan_piece_step(p, i); };
                for (size_t k = 0; k < ranges.size(); ++k) r.range(ranges[k], k + 1 == ranges.size() && !drained_by_end);
                r.end();
                CHECK(r.n_pieces == 20 && !r.count_due && r.violations() == 0);
                for (int c : r.counted) CHECK(c == 1);                  // every piece's count exactly once, the drain included
                size_t n_scan = 0, n_part = 0, n_count = 0;
                for (const Replay::Op& o : r.ops) { n_scan += o.kind == Replay::SCAN; n_part += o.kind == Replay::PART; n_count += o.kind == Replay::COUNT; }
                CHECK(n_scan == 20 && n_part == 20 && n_count == 20);
                for (const Replay::Op& o : r.ops) CHECK(o.slice == (n_slices > 1 ? o.piece & 1 : 0) || o.kind == Replay::COUNT);
                // with two slices a piece's partition and count do not hold up the next scan: it needs neither
                if (n_slices > 1)
                    for (size_t a = 0; a < r.ops.size(); ++a)
                        if (r.ops[a].kind == Replay::SCAN && r.ops[a].piece >= 1)
                            for (size_t b = 0; b < r.ops.size(); ++b)
                                if (r.ops[b].kind != Replay::SCAN && r.ops[b].piece + 1 == r.ops[a].piece) CHECK(!r.ops[a].before.test(b));
            }
    // the model sees what it is there to see: a step that does not wait for the previous count, or that fills one slice
    // every time, is caught.  (Not so one that only skips the wait for the slice's last reader: the main stream has
    // waited for that partition already, on behalf of its count, which is queued behind the scan in between.)
    for (int which : {0, 1}) {
        ScanPlan p; p.keyed = true; p.n_slices = 2;
        Replay r; r.n_slices = 2; r.counted.assign(20, 0);
        r.step = [&](uint64_t i) { PieceStep s = scan_piece_step(p, i); if (which) s.wait_prev_count = false; else { s.slice = 0; s.wait_slice_reader = false; } return s; };
        r.range(20, true);
        CHECK(r.violations() > 0);
    }
    return done("the per-piece step: 20 pieces over two slices, keys2 and the sub-slice tables; every count once, the drain included");
}

int main()
{
    std::mt19937_64 rng(20261);
    int bad = 0;
    bad += test_plan_table();
    bad += test_piece_table();
    bad += test_launch_tables();
    bad += test_small_tables();
    bad += test_within_table();
    bad += test_plan_properties(rng);
    bad += test_within_properties(rng);
    bad += test_piece_steps();
    return bad ? 1 : 0;
}
