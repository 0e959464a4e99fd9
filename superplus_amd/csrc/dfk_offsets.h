// superplus_amd/csrc/dfk_offsets.h -- GetOffsets1 (paths/long/ReadStack.cc:1192-1512), the statement of CloseGap2 behind the stacks'
// consensus (10X/Closomatic.cc:648): per pair the offsets at which the two consensus sequences overlap convincingly.  The rule over
// plain arrays, the table of log binomial sums, the pieces host and kernels share stated once, the tail (invalidation, big near small)
// as one function, the form the device runs and its plan, the layout of a.close.offsets.
//
// No HIP call and no device pointer is dereferenced here by the host, so tests/cpp/test_offsets.cc compiles this header with a plain
// host compiler (and once more under -fsanitize=address,undefined) and checks it against cases recorded from tests/offsets_oracle.py.
// It is the SECOND restatement of the rule -- written from the reference's text, not from the Python.
//
// GetOffsets1 takes Consensus1( ) of both stacks (:1219-1223) and after that reads con1 and con2 only (stack1.Cols( ) at :1430 is
// con1.size( )): the result is a function of the two byte strings a.close.cons holds for a pair.  They are at most max_width = 400
// long (10X/DF.cc:590), so the early return at 1000 (:1229) cannot be reached; a longer element is refused.
//
// The rule (con1, con2 with values 0..3, lengths n1, n2 <= 400):
//   table (:48-62, :1214, random/Bernoulli.cc:40-50)   T[n][k] = log10( (double) S ) for 20 <= n <= 400, 0 <= k < n; S the LONG DOUBLE
//                       sum of Bernoulli.cc:44-50 as written: sum += choose * product; choose *= double(n - i); choose /= double(i + 1);
//                       product *= p / (1.0 - p) (exactly 3), from product = pow( 0.25, n ) (exactly 2^-2n).  T[n][n] = 0.0: the object
//                       is static and that cell is never written; it IS read, by a window of nothing but mismatches.  Built on the
//                       host only (LDBL_MANT_DIG == 64), outside device compilation; the device gathers doubles and computes no log.
//   candidates (:1233-1254)   every o = j1 - j2 with con1[j1, j1 + 8) == con2[j2, j2 + 8): unique, ascending.  A sequence shorter than
//                       8 gives none.
//   overlap, mismatch (:1258-1269)   per candidate over p1 with 0 <= p1 - o < n2.  max_overlap_seen only sizes the scratch vectors.
//   bits (:1275-1332)   pos1 = max( o, 0 ), pos2 = max( -o, 0 ); sum_errors the prefix sums of the mismatches along the overlap.  With
//                       wx = 40, max_ewx = 20, w = 20: errs at m is the mismatch count of overlap positions [max(0, m - 39), m];
//                       bad_window[max(0, m - 40)] is set when that is >= 20, for m <= overlap - 40.  The loop at :1310 never runs
//                       (w - wx < 0).  A start's n runs from 20 to overlap - start and stops before the first n >= 40 with
//                       bad_window[start + n - 40].  minp starts at 0. and takes Min( minp, T[n][k] ), k = sum_errors[start + n] -
//                       sum_errors[start].  bits = -minp * 10.0 / 6.0; the offset is kept when bits >= 25.0, fraglen = o + n2.
//   invalidation (:1422-1485)   per kept offset val1 / val2: the agreeing runs less flank = 10 positions at each end (the inner loop
//                       advances the outer loop's p1).  invalidates[j][i] when a mismatch ( p1, p2 ) of offset i has val1[j][p1] and
//                       val2[j][p2].  An offset that nothing invalidates deletes those it invalidates (two steps: first the matrix).
//   big near small (:1489-1502)   min_bits_save = 40.0, min_add = 10.0, min_slope = 2.0, over what is left, i1 outside, i2 inside,
//                       to_delete2[i1] tested inside the inner loop; the division is by Abs of an int.
//   result              the surviving offsets in order.
//   Min is b < a ? b : a: exact, and the same in any order.  A perfect overlap of n bases has bits = n log10(4) 10 / 6 = 1.00343 n.
//
// Stated ONCE for host and kernels: pack8 (an 8-mer in 16 bits), cand_bit (the bitmap place of o), overlap_of / pos1_of / pos2_of,
// mismatch_at (the mismatch bit at an overlap position), window_is_bad and bad_index (bad_window from prefix sums), last_n (where a
// start's n loop ends given the first bad index at or behind it), min_of and bits_of.
//
// The form the device runs (dfk_offsets_kernels.h, dfk_offsets.inc; offsets_plan() below is its order of work on the host):
//   batches    `pairs_per_batch` pairs at a time, or as many as fit the room.
//   candidates a workgroup a pair: both sequences' 8-mers packed into LDS as u16, a lane a con1 position running over con2's, bit
//              o + n2 - 1 of an LDS bitmap of 800 bits set by an LDS bit-or: the only atomic, and order-free.  Counts per pair, an
//              exclusive scan, the candidates emitted ascending at the scanned places.
//   bits       a workgroup a candidate: the mismatch bits of the overlap as 64-bit ballots in LDS, the prefix sums from popcounts,
//              bad_window, its ballots; a lane takes a start and the start mirrored from the far end, finds the first bad index at or
//              behind it and gathers T[n][k] over its n; the minimum over lanes by shuffles and LDS.  ( o, overlap, mismatch, bits,
//              look-ups ) per candidate; those with bits >= 25.0 compacted by scan, the order kept.
//   tail       on the host through tail() below, over the offsets that passed: a handful a pair on real data.
//
// The file (dfk_offsets_write).  Numbers are little-endian, no byte undefined.
//   a.close.offsets   "DFKCOFF1" | u64 n_pairs | (n_pairs + 1) x u64 starts, in records | n_pairs x 16-byte { u32 candidates, u32 passed,
//                  u32 survivors, u32 0 } | 32-byte records { i32 offset, i32 overlap, i32 fraglen, i32 mismatch, f64 bits, u32 state,
//                  u32 0 }: one per offset that passed the bits test, ascending; state 0 surviving, 1 removed by invalidation, 2
//                  removed as small near big.  The survivors of a pair are its state-0 records in order.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define DFK_OF_HD __host__ __device__ inline
#else
#define DFK_OF_HD inline
#endif

namespace dfk_offsets {

constexpr int MAX_N = 400;                         // 10X/DF.cc:590: no consensus is longer
constexpr int T_DIM = MAX_N + 1;                   // T is T_DIM x T_DIM doubles, row n, cell k
constexpr int MIN_STRETCH = 8, W = 20, WX = 40, MAX_EWX = 20;        // :1205-1210
constexpr double MIN_BITS = 25.0, MIN_BITS_SAVE = 40.0, MIN_SLOPE = 2.0, MIN_ADD = 10.0;
constexpr int FLANK = 10;                          // :1434
constexpr uint32_t BITMAP_WORDS = 25;              // 800 bits: o + n2 - 1 lies in [0, n1 + n2 - 2]
constexpr uint32_t GROUP = 256;
constexpr uint64_t SALT = 0xF0F0ull;               // k_digest_seq's, over the per-pair words, then the records as u32 words
constexpr uint32_t SURVIVES = 0, INVALIDATED = 1, SMALL = 2;

// the 8-mer at s[0, 8) in 16 bits
DFK_OF_HD uint16_t pack8(const uint8_t* s)
{
    uint32_t x = 0;
    for (int i = 0; i < MIN_STRETCH; ++i) x |= (uint32_t)(s[i] & 3u) << (2 * i);
    return (uint16_t)x;
}
DFK_OF_HD uint32_t cand_bit(int j1, int j2, int n2) { return (uint32_t)(j1 - j2 + n2 - 1); }
DFK_OF_HD int cand_offset(uint32_t bit, int n2) { return (int)bit - (n2 - 1); }
DFK_OF_HD int pos1_of(int o) { return o < 0 ? 0 : o; }                                              // :1279
DFK_OF_HD int pos2_of(int o) { return o < 0 ? -o : 0; }                                             // :1280
DFK_OF_HD int overlap_of(int o, int n1, int n2)                                                    // :1263-1266, counted
{
    const int a = n1 - pos1_of(o), b = n2 - pos2_of(o);
    return a < b ? a : b;
}
DFK_OF_HD bool mismatch_at(const uint8_t* con1, const uint8_t* con2, int pos1, int pos2, int i) { return con1[pos1 + i] != con2[pos2 + i]; }
// bad_window from the prefix sums S (S[i] = mismatches in front of overlap position i): what :1299-1304 leaves for m
template <class Sums> DFK_OF_HD bool window_is_bad(const Sums& S, int m) { return (int)S[m + 1] - (int)S[m >= WX ? m - WX + 1 : 0] >= MAX_EWX; }
DFK_OF_HD int bad_index(int m) { return m > WX ? m - WX : 0; }
// where a start's n loop ends: overlap - start, or in front of the first n >= 40 with bad_window[start + n - 40]; next_bad the first
// bad index >= start, or -1
DFK_OF_HD int last_n(int start, int overlap, int next_bad) { return next_bad < 0 ? overlap - start : next_bad - start + WX - 1; }
DFK_OF_HD double min_of(double a, double b) { return b < a ? b : a; }                                // Min( a, b )
DFK_OF_HD double bits_of(double minp) { return -minp * 10.0 / 6.0; }                                // :1327

struct Rec { int32_t offset, overlap, fraglen, mismatch; double bits; uint32_t state, zero; };
struct PairWords { uint32_t candidates, passed, survivors, zero; };

} // namespace dfk_offsets

// ---------------------------------------------------------------------------------------------------------------- host only
#include <float.h>
#include <math.h>
#include <stdlib.h>
#include <algorithm>
#include <tuple>
#include <vector>

namespace dfk_offsets {

static_assert(sizeof(Rec) == 32 && sizeof(PairWords) == 16, "a.close.offsets records");

// ---- the table: PrecomputedBinomialSums<1000>( 20, 0.75 ), its rows up to 400 (ReadStack.cc:48-62).  The device pass of a HIP
// compilation reads this header too, with a long double of 53 bits: it gets no table code at all.
#if defined(__HIP_DEVICE_COMPILE__)
inline double binomial_sum(int, int, double) { return 0.; }
inline const std::vector<double>& table() { static const std::vector<double> none; return none; }
#else
static_assert(LDBL_MANT_DIG == 64, "BinomialSum adds in the x87 extended format");
inline double binomial_sum(int n, int k, double p)                                                  // Bernoulli.cc:40-50
{
    long double sum = 0, choose = 1.0, product = pow(1.0 - p, double(n));
    for (int i = 0; i <= k; i++) {
        sum += choose * product;
        choose *= double(n - i);
        choose /= double(i + 1);
        product *= p / (1.0 - p);
    }
    return sum;
}
// the same sums, the loop run once a row: the call for k does the passes 0..k of the call for k + 1
inline std::vector<double> make_table()
{
    std::vector<double> T((size_t)T_DIM * T_DIM, 0.0);
    const double p = 0.75;
    for (int n = W; n <= MAX_N; ++n) {
        long double sum = 0, choose = 1.0, product = pow(1.0 - p, double(n));
        for (int k = 0; k != n; ++k) {
            sum += choose * product;
            choose *= double(n - k);
            choose /= double(k + 1);
            product *= p / (1.0 - p);
            T[(size_t)n * T_DIM + k] = log10((double)sum);
        }
    }
    return T;
}
inline const std::vector<double>& table() { static const std::vector<double> T = make_table(); return T; }
#endif

struct PairResult {
    uint32_t candidates = 0;
    uint64_t lookups = 0;
    std::vector<Rec> recs;                          // the offsets that passed the bits test, ascending, with their states
};

// ---- the tail (:1422-1502) over the offsets that passed, as written: sets offsets[i].state
inline void tail_literal(const uint8_t* con1, int n1, const uint8_t* con2, int n2, Rec* offsets, int N)
{
    std::vector<std::vector<char>> val1(N), val2(N);                                                // :1422
    for (int i = 0; i < N; i++) {
        val1[i].assign(n1, 0); val2[i].assign(n2, 0);                                               // :1430-1431
        const int o = offsets[i].offset;
        for (int p1 = 0; p1 < n1; p1++) {                                                           // :1435
            int p2 = p1 - o;
            if (p2 < 0 || p2 >= n2) continue;
            if (con1[p1] != con2[p2]) continue;
            const int low1 = p1;
            for (; p1 < n1; p1++) {                                                                 // :1440
                p2 = p1 - o;
                if (p2 >= n2) break;
                if (con1[p1] != con2[p2]) break;
            }
            const int high1 = p1;
            for (int q1 = low1 + FLANK; q1 < high1 - FLANK; q1++) { const int q2 = q1 - o; val1[i][q1] = val2[i][q2] = 1; }   // :1450-1452
        }
    }
    std::vector<std::vector<char>> invalidates(N, std::vector<char>(N, 0));                         // :1453
    for (int i = 0; i < N; i++) {
        const int o = offsets[i].offset;
        for (int p1 = 0; p1 < n1; p1++) {
            const int p2 = p1 - o;
            if (p2 < 0 || p2 >= n2) continue;
            if (con1[p1] == con2[p2]) continue;
            for (int j = 0; j < N; j++) if (val1[j][p1] && val2[j][p2]) invalidates[j][i] = 1;      // :1466-1476
        }
    }
    std::vector<char> to_delete(N, 0);                                                              // :1477
    for (int i = 0; i < N; i++) {
        bool good = true;
        for (int j = 0; j < N; j++) if (invalidates[j][i]) good = false;
        if (!good) continue;
        for (int j = 0; j < N; j++) if (invalidates[i][j]) to_delete[j] = 1;
    }
    std::vector<int> left;                                                                          // EraseIf
    for (int i = 0; i < N; i++) { offsets[i].state = to_delete[i] ? INVALIDATED : SURVIVES; if (!to_delete[i]) left.push_back(i); }
    const int L = (int)left.size();
    std::vector<char> to_delete2(L, 0);                                                             // :1491
    for (int i1 = 0; i1 < L; i1++)
        for (int i2 = 0; i2 < L; i2++) {
            if (to_delete2[i1]) continue;
            if (offsets[left[i2]].bits >= MIN_BITS_SAVE) continue;
            const double delta_bits = offsets[left[i1]].bits - offsets[left[i2]].bits;
            if (delta_bits < MIN_ADD) continue;
            if (delta_bits / abs(offsets[left[i1]].offset - offsets[left[i2]].offset) < MIN_SLOPE) continue;
            to_delete2[i2] = 1;
        }
    for (int x = 0; x < L; x++) if (to_delete2[x]) offsets[left[x]].state = SMALL;
}
// ... and as the stage runs it.  None or one: nothing is removed -- an offset never invalidates itself (val1[i] holds agreeing positions
// of offset i only, and invalidates[ ][i] is looked up at its mismatches), and :1497 skips i1 == i2 (delta_bits 0 < min_add).  Most
// pairs end here, without the vectors.
inline void tail(const uint8_t* con1, int n1, const uint8_t* con2, int n2, Rec* offsets, int N)
{
    if (N <= 1) { if (N == 1) offsets[0].state = SURVIVES; return; }
    tail_literal(con1, n1, con2, n2, offsets, N);
}

// ---- the literal transcription for one pair: :1233-1332 with every vector as it stands, then the tail
inline PairResult offsets_literal(const uint8_t* con1, int n1, const uint8_t* con2, int n2, const double* T)
{
    PairResult R;
    std::vector<std::tuple<uint32_t, int, int>> kmers_plus;                                         // :1236-1237: < kmer, index, offset >, sorted
    for (int idx = 0; idx < 2; idx++) {
        const uint8_t* con = idx ? con2 : con1;
        const int n = idx ? n2 : n1;
        for (int j = 0; j + MIN_STRETCH <= n; j++) kmers_plus.emplace_back(pack8(con + j), idx, j);
    }
    std::sort(kmers_plus.begin(), kmers_plus.end());
    std::vector<int> doffsets;
    const int nk = (int)kmers_plus.size();
    for (int i = 0; i < nk; i++) {                                                                  // :1239
        int j;
        for (j = i + 1; j < nk; j++) if (std::get<0>(kmers_plus[j]) != std::get<0>(kmers_plus[i])) break;
        for (int l1 = i; l1 < j; l1++) {
            if (std::get<1>(kmers_plus[l1]) != 0) continue;
            for (int l2 = i; l2 < j; l2++) {
                if (std::get<1>(kmers_plus[l2]) != 1) continue;
                doffsets.push_back(std::get<2>(kmers_plus[l1]) - std::get<2>(kmers_plus[l2]));
            }
        }
        i = j - 1;
    }
    std::sort(doffsets.begin(), doffsets.end());                                                    // UniqueSort
    doffsets.erase(std::unique(doffsets.begin(), doffsets.end()), doffsets.end());
    R.candidates = (uint32_t)doffsets.size();
    std::vector<std::tuple<int, int, int>> oom;                                                     // :1258
    size_t max_overlap_seen = 0;
    for (size_t oi = 0; oi < doffsets.size(); oi++) {
        const int o = doffsets[oi];
        int overlap = 0, mismatch = 0;
        for (int p1 = 0; p1 < n1; p1++) {
            const int p2 = p1 - o;
            if (p2 < 0 || p2 >= n2) continue;
            overlap++;
            if (con1[p1] != con2[p2]) mismatch++;
        }
        max_overlap_seen = std::max(max_overlap_seen, (size_t)overlap);
        oom.emplace_back(o, overlap, mismatch);
    }
    std::vector<char> bad_window(max_overlap_seen);                                                 // :1272
    std::vector<int> sum_errors(max_overlap_seen + 1);                                              // :1273
    for (size_t j = 0; j < oom.size(); j++) {
        const int offset = std::get<0>(oom[j]), overlap = std::get<1>(oom[j]), mismatch = std::get<2>(oom[j]);
        const int pos1 = offset < 0 ? 0 : offset, pos2 = offset < 0 ? -offset : 0;
        sum_errors[0] = 0;
        for (int i = 1; i <= overlap; ++i) sum_errors[i] = sum_errors[i - 1] + ((con1[pos1 + i - 1] != con2[pos2 + i - 1]) ? 1 : 0);
        int errs = 0;
        for (size_t i = 0; i < max_overlap_seen; ++i) bad_window[i] = 0;
        for (int m = 0; m <= overlap - WX; m++) {                                                   // :1299
            if (con1[pos1 + m] != con2[pos2 + m]) errs++;
            if (m >= WX && con1[pos1 + m - WX] != con2[pos2 + m - WX]) errs--;
            if (errs >= MAX_EWX) bad_window[std::max(0, m - WX)] = 1;
        }
        double minp = 0.;                                                                           // :1306
        for (int start = 0; start < overlap; start++) {
            bool bad = false;
            for (int m = 0; !bad && m < W - WX; m++) if (bad_window[start + m]) bad = true;         // (never runs)
            for (int n = W; n <= overlap - start; n++) {                                            // :1315
                if (n - WX >= 0 && bad_window[start + n - WX]) bad = true;
                const int k = sum_errors[start + n] - sum_errors[start];
                if (bad) break;
                minp = min_of(minp, T[(size_t)n * T_DIM + k]);
                ++R.lookups;
            }
        }
        const double bitsj = -minp * 10.0 / 6.0;
        if (bitsj >= MIN_BITS) R.recs.push_back(Rec{offset, overlap, offset + n2, mismatch, bitsj, 0, 0});
    }
    tail_literal(con1, n1, con2, n2, R.recs.data(), (int)R.recs.size());
    return R;
}

// ---- the plan: pairs per batch.  A pair costs its bases, its bitmap and count, and for every candidate it may have (n1 + n2 - 1 at
// most, seldom more than a few dozen) the candidate's pair and offset, its record, its flag and place, and the compacted record.
constexpr uint64_t BYTES_PER_PAIR = 2 * (uint64_t)MAX_N + 4 * BITMAP_WORDS + 32;
constexpr uint64_t BYTES_PER_CANDIDATE = 8 + 32 + 16 + 32;
constexpr uint64_t MAX_BATCH = 1ull << 20;
inline uint64_t pairs_per_batch(uint64_t free_now, uint64_t forced)
{
    if (forced) return forced;
    return std::max<uint64_t>(1, std::min<uint64_t>(MAX_BATCH, free_now / 2 / (BYTES_PER_PAIR + 64 * BYTES_PER_CANDIDATE)));
}
inline unsigned group_grid(uint64_t n, unsigned cus) { return (unsigned)std::max<uint64_t>(1, std::min<uint64_t>(n, 64ull * cus)); }

// starts [2 n_pairs + 1] and bases as the stage takes them: 0 fine; 1 not monotone or not from 0; 2 an element longer than 400; 3 a base above 3
inline int check_input(uint64_t n_pairs, const uint64_t* starts, const uint8_t* bases)
{
    if (starts[0] != 0) return 1;
    for (uint64_t q = 0; q < 2 * n_pairs; ++q) {
        if (starts[q + 1] < starts[q]) return 1;
        if (starts[q + 1] - starts[q] > (uint64_t)MAX_N) return 2;
    }
    for (uint64_t i = 0; i < starts[2 * n_pairs]; ++i) if (bases[i] > 3) return 3;
    return 0;
}

struct HostResult {
    std::vector<uint64_t> starts;                   // [n_pairs + 1], in records
    std::vector<PairWords> words;
    std::vector<Rec> recs;
    uint64_t candidates = 0, lookups = 0, batches = 0;
};

// The device version's order of work on the host, for the CPU test: candidates by bitmap, bad_window from prefix sums, a start's last
// n from the first bad index at or behind it, the lanes' minima folded pairwise, the tail per pair.  per_batch 0 = all in one.
inline void offsets_plan(uint64_t n_pairs, const uint64_t* starts, const uint8_t* bases, uint64_t per_batch, const double* T, HostResult* R)
{
    R->starts.assign(1, 0);
    for (uint64_t p0 = 0; p0 < n_pairs;) {
        const uint64_t p1 = per_batch ? std::min(n_pairs, p0 + std::min<uint64_t>(per_batch, n_pairs)) : n_pairs, nb = p1 - p0;
        ++R->batches;
        // candidates (a workgroup a pair): the bitmaps and the counts; the scan; the emit
        std::vector<uint32_t> bitmap(nb * BITMAP_WORDS, 0);
        std::vector<uint64_t> count(nb + 1, 0), place(nb + 1, 0);
        for (uint64_t b = 0; b < nb; ++b) {
            const uint64_t q = 2 * (p0 + b);
            const uint8_t* con1 = bases + starts[q]; const uint8_t* con2 = bases + starts[q + 1];
            const int n1 = (int)(starts[q + 1] - starts[q]), n2 = (int)(starts[q + 2] - starts[q + 1]);
            std::vector<uint16_t> km1(std::max(0, n1 - MIN_STRETCH + 1)), km2(std::max(0, n2 - MIN_STRETCH + 1));
            for (size_t j = 0; j < km1.size(); ++j) km1[j] = pack8(con1 + j);
            for (size_t j = 0; j < km2.size(); ++j) km2[j] = pack8(con2 + j);
            for (size_t j1 = 0; j1 < km1.size(); ++j1)
                for (size_t j2 = 0; j2 < km2.size(); ++j2)
                    if (km1[j1] == km2[j2]) { const uint32_t bit = cand_bit((int)j1, (int)j2, n2); bitmap[b * BITMAP_WORDS + (bit >> 5)] |= 1u << (bit & 31u); }
            for (uint32_t w = 0; w < BITMAP_WORDS; ++w) count[b] += (uint64_t)__builtin_popcount(bitmap[b * BITMAP_WORDS + w]);
        }
        for (uint64_t b = 0; b < nb; ++b) place[b + 1] = place[b] + count[b];
        const uint64_t C = place[nb];
        std::vector<uint32_t> c_pair(C); std::vector<int32_t> c_off(C);
        for (uint64_t b = 0; b < nb; ++b) {
            const int n2 = (int)(starts[2 * (p0 + b) + 2] - starts[2 * (p0 + b) + 1]);
            uint64_t at = place[b];
            for (uint32_t bit = 0; bit < 32 * BITMAP_WORDS; ++bit)
                if (bitmap[b * BITMAP_WORDS + (bit >> 5)] >> (bit & 31u) & 1u) { c_pair[at] = (uint32_t)b; c_off[at] = cand_offset(bit, n2); ++at; }
        }
        R->candidates += C;
        // bits (a workgroup a candidate), the flags, the scan, the compaction
        std::vector<Rec> recs(C);
        std::vector<uint64_t> flag(C + 1, 0), fplace(C + 1, 0);
        for (uint64_t ci = 0; ci < C; ++ci) {
            const uint64_t q = 2 * (p0 + c_pair[ci]);
            const uint8_t* con1 = bases + starts[q]; const uint8_t* con2 = bases + starts[q + 1];
            const int n1 = (int)(starts[q + 1] - starts[q]), n2 = (int)(starts[q + 2] - starts[q + 1]);
            const int o = c_off[ci], pos1 = pos1_of(o), pos2 = pos2_of(o), overlap = overlap_of(o, n1, n2);
            std::vector<uint16_t> S(overlap + 1, 0);
            for (int i = 0; i < overlap; ++i) S[i + 1] = (uint16_t)(S[i] + (mismatch_at(con1, con2, pos1, pos2, i) ? 1 : 0));
            std::vector<char> bad(overlap + 1, 0);
            for (int m = 0; m <= overlap - WX; ++m) if (window_is_bad(S, m)) bad[bad_index(m)] = 1;
            std::vector<int> next_bad(overlap + 1, -1);
            for (int i = overlap - 1; i >= 0; --i) next_bad[i] = bad[i] ? i : next_bad[i + 1];
            std::vector<double> lane(GROUP, 0.);                                                     // a lane a start and its mirror
            uint64_t looked = 0;
            for (int start = 0; start < overlap; ++start) {
                const uint32_t l = (uint32_t)start < GROUP ? (uint32_t)start : 2 * GROUP - 1 - (uint32_t)start;
                const int last = last_n(start, overlap, next_bad[start]);
                for (int n = W; n <= last; ++n) { lane[l] = min_of(lane[l], T[(size_t)n * T_DIM + (S[start + n] - S[start])]); ++looked; }
            }
            for (uint32_t d = GROUP / 2; d >= 1; d >>= 1) for (uint32_t l = 0; l < d; ++l) lane[l] = min_of(lane[l], lane[l + d]);
            recs[ci] = Rec{o, overlap, o + n2, (int32_t)S[overlap], bits_of(lane[0]), 0, 0};
            R->lookups += looked;
            flag[ci] = recs[ci].bits >= MIN_BITS ? 1u : 0u;
        }
        for (uint64_t ci = 0; ci < C; ++ci) fplace[ci + 1] = fplace[ci] + flag[ci];
        std::vector<Rec> passed(fplace[C]); std::vector<uint32_t> passed_pair(fplace[C]);
        for (uint64_t ci = 0; ci < C; ++ci) if (flag[ci]) { passed[fplace[ci]] = recs[ci]; passed_pair[fplace[ci]] = c_pair[ci]; }
        // the tail (the host), a pair at a time
        uint64_t at = 0;
        for (uint64_t b = 0; b < nb; ++b) {
            const uint64_t q = 2 * (p0 + b), first = at;
            while (at < passed.size() && passed_pair[at] == b) ++at;
            tail(bases + starts[q], (int)(starts[q + 1] - starts[q]), bases + starts[q + 1], (int)(starts[q + 2] - starts[q + 1]), passed.data() + first, (int)(at - first));
            uint32_t alive = 0;
            for (uint64_t i = first; i < at; ++i) alive += passed[i].state == SURVIVES;
            R->words.push_back(PairWords{(uint32_t)count[b], (uint32_t)(at - first), alive, 0});
            R->recs.insert(R->recs.end(), passed.begin() + first, passed.begin() + at);
            R->starts.push_back(R->recs.size());
        }
        p0 = p1;
    }
}

// ---- the file's fixed parts
constexpr const char* MAGIC = "DFKCOFF1";
inline uint64_t words_at(uint64_t n) { return 16 + 8 * (n + 1); }
inline uint64_t recs_at(uint64_t n) { return words_at(n) + 16 * n; }
inline uint64_t file_size(uint64_t n, uint64_t n_recs) { return recs_at(n) + 32 * n_recs; }

} // namespace dfk_offsets
