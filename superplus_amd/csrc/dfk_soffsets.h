// superplus_amd/csrc/dfk_soffsets.h -- Stackster's stack offsets per pair (10X/Stackster.cc:461-645: the 8-mers of one stack's consensus
// that are acceptable :499-517, the rows of the other stack searched for them :521-565, the bits of a ( row, offset ) :571-598, the
// filter over the results :631-645; paths/long/ReadStack.h:103 Def, ReadStack.cc:64-69 and :346-353 the ' ' cell, :48-62 the table).
// The rule over plain arrays, the pieces host and kernels share stated once, the form the device runs and its plan, the layout of
// a.stack.offsets.
//
// No HIP call and no device pointer is dereferenced here by the host, so tests/cpp/test_soffsets.cc compiles this header with a plain
// host compiler (and once more under -fsanitize=address,undefined) and checks it against cases recorded from tests/soffsets_oracle.py.
// It is the SECOND restatement of the rule -- written from the reference's text, not from the Python.
//
// The input of a pair: its two stacks after Trim and Reverse exactly as dfk_scons.h defines them (the cell, the row orientation and
// the live-row rule are that header's and dfk_walks.h's: cell_index, stack_column, row_rc, span_meets, oriented_base, oriented_qual),
// and con, conq and the conflict count of every offset as a.stack.cons holds them.  Only a pair that yields has anything.
//
// The rule (ALT = False, EXP = False, idsfw2 empty).  A cell is DEFINED iff its lowered quality is below 128.  A cell outside its row's
// span has base ' ', which differs from every base of con; a cell inside the span with quality 128 or more has its real base
// (complemented on side 1) and is undefined.  For s in 0, 1 with s1 = stacks[s], s2 = stacks[1 - s], con1 = con of side s:
//   acceptable (:499-517)   position j in [0, s1.Cols( ) - 8] iff bases j..j+3 are not all equal, bases j+4..j+7 are not all equal and
//                       at least 3 distinct bases stand in the 8.
//   candidates (:521-565)   every row r of s2, every l in [0, s2.Cols( ) - 8] whose 8 cells are all defined, every acceptable j with
//                       the same 8-mer: offset = ( s == 0 ? j - l : l - j ) -- always stack 1 against stack 0.  Skipped if ( r, offset )
//                       was seen for this s; skipped if the conflict count at index offset + n2 is 10 or more (the lazily filled
//                       allowed / disallowed of :548-563 is a.stack.cons' table); otherwise seen.
//   bits (:571-598)     offx = ( s == 0 ? offset : -offset ), pos1 = max( offx, 0 ), pos2 = max( -offx, 0 ), overlap = IntervalOverlap(
//                       0, s1.Cols( ), offx, offx + s2.Cols( ) ); err_sum the prefix sums of con1[pos1 + v] != s2.Base( r, pos2 + v ).
//                       minp = 0.; every start in [0, overlap) and n in [20, overlap - start] whose END CELLS s2( r, pos2 + start ) and
//                       s2( r, pos2 + start + n - 1 ) are both defined: minp = Min( minp, T[n][k] ), k the mismatches of the window.
//                       bits = -minp * 10.0 / 6.0, a result iff bits >= 20.0.  T is dfk_offsets::table( ): the same class and the
//                       same BinomialSum, n <= 400; T[n][n] = 0.0 is read by a window of nothing but mismatches.
//   filter (:631-645)   results ( bits, offset ) sorted descending; offsets takes results[0]'s, then every offset not yet taken whose
//                       first occurrence has results[0].first - score <= 20.0.  offsets sorted ascending.  Closable: 1 <= |offsets| <= 3
//                       (:715).
//   EQUIVALENT, and what the device computes: per distinct offset the MAXIMUM of bits, best = the maximum over the pair; an offset is
//   kept iff best - max_bits( offset ) <= 20.0.  The first occurrence of an offset in the descending order carries its greatest
//   score; results[0] passes with difference 0; the test is a function of the score alone.  tests/cpp/test_soffsets.cc holds it to
//   the literal sort-and-scan form.
//   Exact: the table is built once on the host in long double; after it integer counts, Min / Max of doubles (order-free, no NaN), one
//   negate, one multiply, one divide, one subtract, comparisons.  bits >= 20 > 0, and non-negative doubles order like their bit
//   patterns: the maximum is taken on u64.  No logarithm on the device, no fast-math flag.
//
// The form the device runs (dfk_soffsets_kernels.h, dfk_soffsets.inc; soffsets_plan() below is its order of work on the host):
//   ranges     whole pairs, as dfk_scons.h's.
//   batches    whole pairs of the range: as many as keep their live rows at rows_per_batch, or as fit the room; never less than one
//              pair, never a part of one.  The reads their live rows name gathered once each, decoded, lowered (as dfk_scons.inc).
//   search     a workgroup a pair: both con, their acceptable 8-mers (u16, NO_KMER where unacceptable), the allowed bits of the 800
//              conflict counts and a table of 800 ( u64 max bits, u32 results ) in LDS.  A WAVE a live row of either stack: the row's
//              cells (base or BLANK, the defined bits as ballots) into LDS once; a lane an l running over the con 8-mers, the
//              ( r, offset ) deduplicated by an LDS bit-or into the wave's bitmap of 800 bits; then, the cells still in LDS, the
//              wave takes the set bits one after the other: mismatch and defined ballots of the overlap, prefix sums by popcount,
//              a lane a defined start running over the defined ends alone, Min by __shfl_xor; a result goes into the pair's table by
//              an LDS u64 max and u32 add (order-free).  No candidate is stored, so no batch can overflow with them.
//   records    the same workgroup: best by a tree, the table compacted ascending by a scan over the workgroup into the pair's slot
//              (the slots lie at the conflict entries' places: a pair cannot have more records); the per-pair words and counts.
//   emit       counts scanned (device_scan), the records copied to their scanned places.
//
// The file (dfk_soffsets_write).  Numbers are little-endian, no byte undefined.
//   a.stack.offsets   "DFKSOFF1" | u64 n_pairs | (n_pairs + 1) x u64 starts, in records | n_pairs x 16-byte { u32 seen, u32 results,
//                  u32 kept, u32 closable } | 24-byte records { i32 offset, u32 results, f64 best_bits, u32 state, u32 0 }: one per distinct
//                  offset with a result, ascending; state 0 kept, 1 dropped.  (A multiple of 8 as it stands.)
#pragma once
#include <stdint.h>
#include "dfk_scons.h"
#include "dfk_offsets.h"

namespace dfk_soffsets {

constexpr int MM = 8;                              // :464
constexpr int WID = 20;                            // :573
constexpr double MIN_BITS = 20.0, MAX_DIFF = 20.0; // :597, :635
constexpr uint32_t MAX_OFFSETS = 3;                // :714
constexpr int64_t MAX_WIDTH = dfk_scons::MAX_WIDTH;
constexpr uint32_t N_IDX = 2 * (uint32_t)MAX_WIDTH; // offset + n2 lies in [0, n1 + n2)
constexpr uint32_t BITMAP_WORDS = N_IDX / 32;      // 25
constexpr uint32_t MASK_WORDS = 8;                 // 400 columns in 7 words of 64, and one of zeros behind them
constexpr uint8_t BLANK = 4;                       // ' ': no base
constexpr uint8_t DEF_BIT = 8;
constexpr uint16_t NO_KMER = 0;                    // AAAAAAAA is flat: never acceptable
constexpr uint32_t GROUP = 256, WAVES = 4;
constexpr uint32_t KEPT = 0, DROPPED = 1;
constexpr uint64_t SALT = 0x50FFull;               // k_digest_seq's: the per-pair words, then the records as u32 words

// ACCEPTABLE (:503-515): the 8-mer packed as dfk_offsets::pack8 does, base m in bits 2m, 2m + 1
DFK_CN_HD bool acceptable(uint32_t km)
{
    const uint32_t lo = km & 0xFFu, hi = (km >> 8) & 0xFFu;
    if (lo == (lo & 3u) * 0x55u) return false;                                                      // bases 0..3 all equal
    if (hi == (hi & 3u) * 0x55u) return false;                                                      // bases 4..7 all equal
    uint32_t present = 0;
    for (int m = 0; m < MM; ++m) present |= 1u << ((km >> (2 * m)) & 3u);
    return ((present & 1u) + ((present >> 1) & 1u) + ((present >> 2) & 1u) + ((present >> 3) & 1u)) >= 3u;
}
// the 8 bits of a mask of MASK_WORDS words from bit l on (l + 8 <= 64 * (MASK_WORDS - 1) + 8)
DFK_CN_HD uint32_t bits8(const unsigned long long* m, int l)
{
    const int w = l >> 6, s = l & 63;
    unsigned long long x = m[w] >> s;
    if (s > 56) x |= m[w + 1] << (64 - s);
    return (uint32_t)(x & 0xFFull);
}
DFK_CN_HD bool bit_at(const unsigned long long* m, int i) { return (m[i >> 6] >> (i & 63)) & 1ull; }
// THE ROW 8-MER at l: true iff its 8 cells are all defined; cells: a base or BLANK a column
DFK_CN_HD bool row_kmer(const uint8_t* cells, const unsigned long long* defined, int l, uint16_t* km)
{
    if (bits8(defined, l) != 0xFFu) return false;
    *km = dfk_offsets::pack8(cells + l);
    return true;
}
// the con 8-mer at j, or NO_KMER
DFK_CN_HD uint16_t con_kmer(const uint8_t* con, int cols, int j)
{
    if (j + MM > cols) return NO_KMER;
    const uint16_t km = dfk_offsets::pack8(con + j);
    return acceptable(km) ? km : NO_KMER;
}
DFK_CN_HD int offset_of(int s, int j, int l) { return s == 0 ? j - l : l - j; }                      // :543
DFK_CN_HD int offx_of(int s, int offset) { return s == 0 ? offset : -offset; }                      // :576
DFK_CN_HD int pos1_of(int offx) { return offx >= 0 ? offx : 0; }
DFK_CN_HD int pos2_of(int offx) { return offx <= 0 ? -offx : 0; }
DFK_CN_HD int overlap_of(int offx, int cols1, int cols2)                                            // IntervalOverlap( 0, cols1, offx, offx + cols2 )
{
    const int lo = offx > 0 ? offx : 0, hi = cols1 < offx + cols2 ? cols1 : offx + cols2;
    return hi > lo ? hi - lo : 0;
}
DFK_CN_HD bool mismatch(uint8_t con_base, uint8_t cell_base) { return con_base != cell_base; }      // BLANK differs from every base
// THE CELL of a row in stack column sc (before Trim and Reverse): base | DEF_BIT, or BLANK
DFK_CN_HD uint8_t cell_of(int32_t start, uint32_t len, bool rc, bool reversed, int64_t sc, const uint8_t* packed, const uint8_t* quals)
{
    const int64_t j = dfk_scons::cell_index(start, len, sc);
    if (j < 0) return BLANK;
    const uint8_t q = dfk_walks::oriented_qual(quals, len, rc, (uint32_t)j);
    const uint32_t b = dfk_walks::oriented_base(packed, len, rc, (uint32_t)j);
    return (uint8_t)((reversed ? 3u - b : b) | (dfk_cons::cell_defined(q) ? DEF_BIT : 0u));
}
// MINP of one start over the row's windows (:589-595): S[i] the mismatches in front of overlap position i, `defined` the defined bits
// of the overlap's positions (zero from `overlap` on).  Only defined ends are visited; *looked counts the look-ups.
template <class Sums> DFK_CN_HD double minp_of_start(const Sums& S, const unsigned long long* defined, int overlap, int start, const double* T, double minp, uint32_t* looked)
{
    if (!bit_at(defined, start)) return minp;
    const int first = start + WID - 1, s0 = (int)S[start];
    for (int w = first >> 6; 64 * w < overlap; ++w) {
        unsigned long long x = defined[w];
        if (w == (first >> 6)) x &= ~0ull << (first & 63);
        while (x) {
            const int e = 64 * w + __builtin_ctzll(x);
            x &= x - 1;
            const int n = e - start + 1;
            minp = dfk_offsets::min_of(minp, T[n * dfk_offsets::T_DIM + ((int)S[e + 1] - s0)]);
            ++*looked;
        }
    }
    return minp;
}
DFK_CN_HD double bits_of(double minp) { return dfk_offsets::bits_of(minp); }                        // :596
DFK_CN_HD bool passes(double bits) { return bits >= MIN_BITS; }                                     // :598
DFK_CN_HD bool kept(double best, double score) { return best - score <= MAX_DIFF; }                 // :642
DFK_CN_HD bool closable(uint32_t n_kept) { return n_kept >= 1 && n_kept <= MAX_OFFSETS; }           // :715

struct Rec { int32_t offset; uint32_t results; double best_bits; uint32_t state, zero; };
struct PairWords { uint32_t seen, results, kept, closable; };
// what a pair's search counts
enum Count : uint32_t { C_KMERS = 0, C_ACCEPTABLE, C_HITS, C_SEEN, C_DISALLOWED, C_LOOKUPS, C_RESULTS, N_COUNTS };

} // namespace dfk_soffsets

// ---------------------------------------------------------------------------------------------------------------- host only
#include <set>
#include <string.h>

namespace dfk_soffsets {

static_assert(sizeof(Rec) == 24 && sizeof(PairWords) == 16, "a.stack.offsets records");

// the walks and the reads (dfk_scons.h's Input) and the stack consensus made from them, in dfk_scons_fetch's forms
struct Input {
    dfk_scons::Input W;
    const uint64_t* cons_starts /* [2 * n_pairs + 1] */; const dfk_scons::Dim* dims; const uint8_t* con; const uint8_t* conq; const uint64_t* cfirst /* [n_pairs + 1] */; const uint16_t* counts;
};
struct HostResult {
    std::vector<uint64_t> starts;                  // [n_pairs + 1], in records
    std::vector<PairWords> words;
    std::vector<Rec> recs;
    uint64_t yielding = 0, rows = 0, n[N_COUNTS] = {}, batches = 0, ranges = 0;
};

// what the consensus tables must hold: 0 fine; -5 the starts fall or do not begin at 0; -6 an element wider than 400 or not as wide as
// its dims say; -7 a base above 3; -8 the counts of a pair are not n1 + n2 (yielding) or 0 (not)
inline int check_cons(const Input& I)
{
    const uint64_t np = I.W.n_pairs;
    if (I.cons_starts[0] != 0 || I.cfirst[0] != 0) return -5;
    for (uint64_t q = 0; q < 2 * np; ++q) {
        if (I.cons_starts[q + 1] < I.cons_starts[q]) return -5;
        const uint64_t w = I.cons_starts[q + 1] - I.cons_starts[q];
        if (w > (uint64_t)MAX_WIDTH || w != I.dims[q].cols) return -6;
    }
    for (uint64_t i = 0; i < I.cons_starts[2 * np]; ++i) if (I.con[i] > 3) return -7;
    for (uint64_t pi = 0; pi < np; ++pi) {
        if (I.cfirst[pi + 1] < I.cfirst[pi]) return -5;
        const uint64_t want = dfk_scons::yields(I.W.recs, pi) ? I.cons_starts[2 * pi + 2] - I.cons_starts[2 * pi] : 0;
        if (I.cfirst[pi + 1] - I.cfirst[pi] != want) return -8;
        if (dfk_scons::yields(I.W.recs, pi))
            for (uint64_t q = 2 * pi; q < 2 * pi + 2; ++q) {
                const int64_t M = I.W.recs[q].M;
                if ((int64_t)I.dims[q].cols != M - dfk_scons::window_start(M)) return -6;
            }
    }
    return 0;
}

inline void finish_pair(HostResult* R, uint32_t seen, const std::vector<Rec>& recs)
{
    PairWords w{seen, 0, 0, 0};
    for (const Rec& r : recs) { w.results += r.results; w.kept += r.state == KEPT; }
    w.closable = closable(w.kept) ? 1u : 0u;
    R->words.push_back(w);
    R->recs.insert(R->recs.end(), recs.begin(), recs.end());
    R->starts.push_back(R->recs.size());
}

// ---- the literal transcription for one pair: :490-645 as written over the two grids (dfk_scons::stack_grids), a std::set for sees, a
// vector of results, ReverseSort and the filter loop
inline void pair_literal(const dfk_cons::Grids* stacks, const uint8_t* con1x, const uint8_t* con2x, const uint16_t* counts, const double* gBS, HostResult* R)
{
    const int n2 = stacks[1].cols;
    std::vector<std::pair<double, int>> results;                                                    // :490
    uint32_t n_seen = 0;
    for (int s = 0; s < 2; s++) {
        const dfk_cons::Grids &s1 = stacks[s], &s2 = stacks[1 - s];
        const uint8_t* con1 = s == 0 ? con1x : con2x;
        std::set<std::pair<int, int>> sees;
        std::vector<std::pair<std::vector<uint8_t>, int>> bbs;                                      // :499
        for (int j = 0; j <= s1.cols - MM; j++) {
            std::vector<uint8_t> bb(con1 + j, con1 + j + MM);
            bool diff = false;
            for (int m = 1; m < MM / 2; m++) if (bb[m] != bb[m - 1]) diff = true;
            if (!diff) continue;
            diff = false;
            for (int m = 1; m < MM / 2; m++) if (bb[MM / 2 + m] != bb[MM / 2 + m - 1]) diff = true;
            if (!diff) continue;
            bool present[4] = {false, false, false, false};
            for (int m = 0; m < MM; m++) present[bb[m]] = true;
            if (present[0] + present[1] + present[2] + present[3] < 3) continue;
            bbs.emplace_back(bb, j);
        }
        std::sort(bbs.begin(), bbs.end());
        R->n[C_ACCEPTABLE] += bbs.size();
        for (int r = 0; r < s2.rows; r++) {                                                         // :521
            ++R->rows;
            for (int l = 0; l <= s2.cols - MM; l++) {
                bool defined = true;
                for (int m = 0; m < MM; m++) if (!(s2.quals_[r][l + m] >= 0)) { defined = false; break; }
                if (!defined) continue;
                ++R->n[C_KMERS];
                std::vector<uint8_t> bb2(MM);
                for (int m = 0; m < MM; m++) bb2[m] = (uint8_t)s2.bases_[r][l + m];
                for (size_t v = 0; v < bbs.size(); v++) {                                           // (LowerBound1 .. UpperBound1: the entries equal to bb2)
                    if (bbs[v].first != bb2) continue;
                    ++R->n[C_HITS];
                    const int j = bbs[v].second;
                    const int offset = s == 0 ? j - l : l - j;
                    if (sees.count(std::make_pair(r, offset))) continue;
                    if (counts[offset + n2] >= dfk_scons::CONFLICTS) { ++R->n[C_DISALLOWED]; continue; }   // :548-563
                    sees.insert(std::make_pair(r, offset));
                    ++n_seen;
                    const int offx = s == 0 ? offset : -offset;                                     // :576
                    const int pos1 = offx >= 0 ? offx : 0, pos2 = offx <= 0 ? -offx : 0;
                    const int overlap = std::max(0, std::min(s1.cols, offx + s2.cols) - std::max(0, offx));
                    double minp = 0;
                    std::vector<int> err_sum(overlap + 1, 0);
                    for (int x = 1; x <= overlap; x++) {
                        err_sum[x] = err_sum[x - 1];
                        if ((int)con1[pos1 + x - 1] != (int)s2.bases_[r][pos2 + x - 1]) err_sum[x]++;
                    }
                    for (int start = 0; start < overlap; start++)
                        for (int n = WID; n <= overlap - start; n++) {
                            if (!(s2.quals_[r][pos2 + start] >= 0) || !(s2.quals_[r][pos2 + start + n - 1] >= 0)) continue;
                            const int k = err_sum[start + n] - err_sum[start];
                            minp = std::min(minp, gBS[n * dfk_offsets::T_DIM + k]);
                            ++R->n[C_LOOKUPS];
                        }
                    const double bits = -minp * 10.0 / 6.0;
                    if (bits < MIN_BITS) continue;
                    results.emplace_back(bits, offset);                                             // :602
                }
            }
        }
    }
    R->n[C_SEEN] += n_seen; R->n[C_RESULTS] += results.size();
    std::sort(results.begin(), results.end(), std::greater<std::pair<double, int>>());              // :634 ReverseSort
    std::vector<int> offsets;
    for (size_t i = 0; i < results.size(); i++) {                                                   // :637
        const double score = results[i].first;
        const int offset = results[i].second;
        if (offsets.empty()) offsets.push_back(offset);
        else if (std::find(offsets.begin(), offsets.end(), offset) != offsets.end()) continue;
        else if (results[0].first - score <= MAX_DIFF) offsets.push_back(offset);
    }
    std::sort(offsets.begin(), offsets.end());
    // the records: a distinct offset with a result each, ascending; its results, its greatest score, kept or dropped
    std::vector<int> all;
    for (const auto& x : results) all.push_back(x.second);
    std::sort(all.begin(), all.end()); all.erase(std::unique(all.begin(), all.end()), all.end());
    std::vector<Rec> recs;
    for (int o : all) {
        Rec rec{o, 0, 0., std::find(offsets.begin(), offsets.end(), o) != offsets.end() ? KEPT : DROPPED, 0};
        for (const auto& x : results) if (x.second == o) { ++rec.results; rec.best_bits = std::max(rec.best_bits, x.first); }
        recs.push_back(rec);
    }
    finish_pair(R, n_seen, recs);
}

// -1..-4: dfk_scons.h's; -5..-8: check_cons'
inline int soffsets_literal(const Input& I, HostResult* R)
{
    if (int rc = dfk_scons::check_walks(I.W)) return rc;
    if (int rc = check_cons(I)) return rc;
    const double* T = dfk_offsets::table().data();
    R->starts.assign(1, 0);
    for (uint64_t pi = 0; pi < I.W.n_pairs; ++pi) {
        if (!dfk_scons::yields(I.W.recs, pi)) { finish_pair(R, 0, {}); continue; }
        ++R->yielding;
        dfk_cons::Grids G[2];
        dfk_scons::HostResult unused;
        for (uint32_t s = 0; s < 2; ++s) { dfk_scons::Dim d{}; if (int rc = dfk_scons::stack_grids(I.W, 2 * pi + s, s, &d, &G[s], &unused)) return rc; }
        pair_literal(G, I.con + I.cons_starts[2 * pi], I.con + I.cons_starts[2 * pi + 1], I.counts + I.cfirst[pi], T, R);
    }
    return 0;
}

// ---- the plan
// A batch of PAIRS [b0, b1) of a range: live_first[p] the live rows in front of pair p, cost_first[p] the bytes.  rows_per_batch 0 = what
// fits `room`.  Never less than one pair.
inline uint64_t next_batch(const uint64_t* live_first, const uint64_t* cost_first, uint64_t n, uint64_t b0, uint64_t room, uint64_t rows_per_batch)
{
    uint64_t b1 = b0 + 1;
    if (rows_per_batch) while (b1 < n && live_first[b1 + 1] - live_first[b0] <= rows_per_batch) ++b1;
    else while (b1 < n && cost_first[b1 + 1] - cost_first[b0] <= room) ++b1;
    return b1;
}
// what a pair costs a batch beside its stacks' rows (dfk_cons.h's live_row_cost): its slot of records, its words and counts
inline uint64_t pair_cost(uint64_t n_idx) { return 2 * dfk_cons::BYTES_PER_STACK + sizeof(Rec) * n_idx + sizeof(PairWords) + 8 * (N_COUNTS + 2); }

// one row of s2 against con1, as a wave runs it: the cells and the defined bits, the bitmap, the set bits in turn.  table: the pair's
// N_IDX ( max bits as u64, results )
inline void row_search(int s, const uint8_t* cells /* [cols2] */, const unsigned long long* defined, int cols2, const uint8_t* con1, const uint16_t* km1, int cols1, int n2,
                       const uint32_t* allowed, const double* T, uint64_t* tmax, uint32_t* tcnt, uint64_t* n)
{
    uint32_t bitmap[BITMAP_WORDS] = {};
    for (int l = 0; l + MM <= cols2; ++l) {
        uint16_t km;
        if (!row_kmer(cells, defined, l, &km)) continue;
        ++n[C_KMERS];
        if (!acceptable(km)) continue;
        for (int j = 0; j + MM <= cols1; ++j) {
            if (km1[j] != km) continue;
            ++n[C_HITS];
            const uint32_t idx = (uint32_t)(offset_of(s, j, l) + n2);
            if (allowed[idx >> 5] >> (idx & 31u) & 1u) bitmap[idx >> 5] |= 1u << (idx & 31u); else ++n[C_DISALLOWED];
        }
    }
    for (uint32_t idx = 0; idx < N_IDX; ++idx) {
        if (!(bitmap[idx >> 5] >> (idx & 31u) & 1u)) continue;
        ++n[C_SEEN];
        const int offx = offx_of(s, (int)idx - n2), pos1 = pos1_of(offx), pos2 = pos2_of(offx), overlap = overlap_of(offx, cols1, cols2);
        unsigned long long mis[MASK_WORDS] = {}, def[MASK_WORDS] = {};
        for (int v = 0; v < overlap; ++v) {
            if (mismatch(con1[pos1 + v], cells[pos2 + v])) mis[v >> 6] |= 1ull << (v & 63);
            if (bit_at(defined, pos2 + v)) def[v >> 6] |= 1ull << (v & 63);
        }
        std::vector<uint16_t> S(overlap + 1, 0);
        for (int v = 0; v < overlap; ++v) S[v + 1] = (uint16_t)(S[v] + (bit_at(mis, v) ? 1 : 0));
        double lane[64];
        for (double& x : lane) x = 0.;
        uint32_t looked = 0;
        for (int start = 0; start < overlap; ++start) lane[start & 63] = minp_of_start(S, def, overlap, start, T, lane[start & 63], &looked);
        for (int d = 32; d >= 1; d >>= 1) for (int l = 0; l < 64; ++l) lane[l] = dfk_offsets::min_of(lane[l], lane[l ^ d]);
        n[C_LOOKUPS] += looked;
        const double bits = bits_of(lane[0]);
        if (!passes(bits)) continue;
        ++n[C_RESULTS];
        uint64_t u; memcpy(&u, &bits, 8);
        tmax[idx] = std::max(tmax[idx], u); ++tcnt[idx];
    }
}

// The device version's order of work on the host, for the CPU test.  rows_per_batch 0 = what fits `room`; returns as soffsets_literal
inline int soffsets_plan(const Input& I, uint64_t rows_per_batch, uint64_t room, uint64_t rows_cap, HostResult* R)
{
    if (int rc = dfk_scons::check_walks(I.W)) return rc;
    if (int rc = check_cons(I)) return rc;
    const dfk_scons::Input& W = I.W;
    const double* T = dfk_offsets::table().data();
    const uint64_t np_all = W.n_pairs;
    std::vector<uint64_t> prows(np_all, 0);
    for (uint64_t pi = 0; pi < np_all; ++pi) if (dfk_scons::yields(W.recs, pi)) { prows[pi] = W.starts[2 * pi + 2] - W.starts[2 * pi]; ++R->yielding; R->rows += I.dims[2 * pi].rows_kept + I.dims[2 * pi + 1].rows_kept; }
    const std::vector<uint64_t> pfirst = dfk::prefix_sums(prows.data(), np_all);
    R->starts.assign(1, 0);
    for (uint64_t p0 = 0; p0 < np_all;) {
        const uint64_t p1 = dfk::pidx_next_range(pfirst.data(), np_all, p0, rows_cap).e1, np = p1 - p0;
        ++R->ranges;
        // the live rows of the range's stacks (host), what a pair costs
        std::vector<uint64_t> lfirst(2 * np + 1, 0), plive(np + 1, 0), pcost(np + 1, 0);
        std::vector<uint32_t> l_id, l_len; std::vector<int32_t> l_start; std::vector<uint8_t> l_rc;
        for (uint64_t s = 0; s < 2 * np; ++s) {
            const uint64_t q = 2 * p0 + s;
            if (dfk_scons::yields(W.recs, q / 2)) {
                const int64_t w0 = dfk_scons::window_start(W.recs[q].M);
                for (uint64_t j = W.starts[q]; j < W.starts[q + 1]; ++j) {
                    const dfk_walks::Loc& L = W.locs[j];
                    if (!dfk_scons::span_meets(L.start, W.read_len[L.id], w0)) continue;
                    l_id.push_back((uint32_t)L.id); l_start.push_back(L.start); l_len.push_back(W.read_len[L.id]); l_rc.push_back(dfk_scons::row_rc(L.fw != 0));
                }
            }
            lfirst[s + 1] = l_id.size();
        }
        for (uint64_t p = 0; p < np; ++p) {
            plive[p + 1] = lfirst[2 * p + 2];
            uint64_t cost = pair_cost(I.cfirst[p0 + p + 1] - I.cfirst[p0 + p]);
            for (uint64_t l = lfirst[2 * p]; l < lfirst[2 * p + 2]; ++l) cost += dfk_cons::live_row_cost(l_len[l]);
            pcost[p + 1] = pcost[p] + cost;
        }
        for (uint64_t b0 = 0; b0 < np;) {
            const uint64_t b1 = next_batch(plive.data(), pcost.data(), np, b0, room, rows_per_batch);
            ++R->batches;
            // the reads of the batch, each once, ascending; the gather; the decode and the lowering
            std::vector<uint32_t> ids(l_id.begin() + lfirst[2 * b0], l_id.begin() + lfirst[2 * b1]);
            std::sort(ids.begin(), ids.end()); ids.erase(std::unique(ids.begin(), ids.end()), ids.end());
            std::vector<uint64_t> b_at(ids.size() + 1, 0), q_at(ids.size() + 1, 0);
            for (size_t i = 0; i < ids.size(); ++i) { const uint32_t len = W.read_len[ids[i]]; b_at[i + 1] = b_at[i] + (len + 3) / 4; q_at[i + 1] = q_at[i] + len; }
            std::vector<uint8_t> bases(b_at.back()), quals(q_at.back());
            for (size_t i = 0; i < ids.size(); ++i) {
                std::copy(W.read_packed + W.read_off[ids[i]], W.read_packed + W.read_off[ids[i]] + (b_at[i + 1] - b_at[i]), bases.begin() + b_at[i]);
                if (!dfk_cons::decode_quals(W.pq, W.pq_off[ids[i]], W.pq_off[ids[i] + 1], quals.data() + q_at[i], W.read_len[ids[i]])) return -3;
                dfk_walks::lower_read(bases.data() + b_at[i], W.read_len[ids[i]], quals.data() + q_at[i]);
            }
            // a workgroup a pair
            for (uint64_t p = b0; p < b1; ++p) {
                const uint64_t pi = p0 + p;
                if (!dfk_scons::yields(W.recs, pi)) { finish_pair(R, 0, {}); continue; }
                const uint8_t* con[2] = {I.con + I.cons_starts[2 * pi], I.con + I.cons_starts[2 * pi + 1]};
                const int cols[2] = {(int)I.dims[2 * pi].cols, (int)I.dims[2 * pi + 1].cols}, n2 = cols[1];
                std::vector<uint16_t> km[2];
                for (int s = 0; s < 2; ++s) { km[s].assign((size_t)MAX_WIDTH, NO_KMER); for (int j = 0; j < cols[s]; ++j) { km[s][j] = con_kmer(con[s], cols[s], j); R->n[C_ACCEPTABLE] += km[s][j] != NO_KMER; } }
                uint32_t allowed[BITMAP_WORDS] = {};
                for (int idx = 0; idx < cols[0] + cols[1]; ++idx) if (I.counts[I.cfirst[pi] + idx] < dfk_scons::CONFLICTS) allowed[idx >> 5] |= 1u << (idx & 31);
                std::vector<uint64_t> tmax(N_IDX, 0); std::vector<uint32_t> tcnt(N_IDX, 0);
                const uint64_t seen0 = R->n[C_SEEN];
                for (int t2 = 0; t2 < 2; ++t2) {                                                  // the rows of stack t2 are searched with s = 1 - t2
                    const int s = 1 - t2;
                    const int64_t M = W.recs[2 * pi + t2].M, w0 = dfk_scons::window_start(M);
                    for (uint64_t l = lfirst[2 * p + t2]; l < lfirst[2 * p + t2 + 1]; ++l) {
                        const uint64_t slot = dfk_cons::slot_of(ids.data(), ids.size(), l_id[l]);
                        std::vector<uint8_t> cells((size_t)MAX_WIDTH + MM, BLANK);
                        unsigned long long def[MASK_WORDS] = {};
                        for (int c = 0; c < cols[t2]; ++c) {
                            const uint8_t v = cell_of(l_start[l], l_len[l], l_rc[l] != 0, t2 == 1, dfk_scons::stack_column(w0, cols[t2], t2 == 1, c), bases.data() + b_at[slot], quals.data() + q_at[slot]);
                            cells[c] = v & 7u;
                            if (v & DEF_BIT) def[c >> 6] |= 1ull << (c & 63);
                        }
                        row_search(s, cells.data(), def, cols[t2], con[s], km[s].data(), cols[s], n2, allowed, T, tmax.data(), tcnt.data(), R->n);
                    }
                }
                // the records: best, the kept flags, the table compacted ascending
                uint64_t best = 0;
                for (uint32_t idx = 0; idx < N_IDX; ++idx) if (tcnt[idx]) best = std::max(best, tmax[idx]);
                double bestd; memcpy(&bestd, &best, 8);
                std::vector<Rec> recs;
                for (uint32_t idx = 0; idx < N_IDX; ++idx) {
                    if (!tcnt[idx]) continue;
                    double score; memcpy(&score, &tmax[idx], 8);
                    recs.push_back(Rec{(int32_t)idx - n2, tcnt[idx], score, kept(bestd, score) ? KEPT : DROPPED, 0});
                }
                finish_pair(R, (uint32_t)(R->n[C_SEEN] - seen0), recs);
            }
            b0 = b1;
        }
        p0 = p1;
    }
    return 0;
}

// ---- the file's fixed parts
constexpr const char* MAGIC = "DFKSOFF1";
inline uint64_t words_at(uint64_t n) { return 16 + 8 * (n + 1); }
inline uint64_t recs_at(uint64_t n) { return words_at(n) + 16 * n; }
inline uint64_t file_size(uint64_t n, uint64_t n_recs) { return recs_at(n) + sizeof(Rec) * n_recs; }

} // namespace dfk_soffsets
