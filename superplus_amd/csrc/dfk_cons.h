// superplus_amd/csrc/dfk_cons.h -- CloseGap2's read stacks and their column consensus (10X/Closomatic.cc:587-640; paths/long/
// ReadStack.cc:346-353 Reverse, :400-404 Consensus1, :714-725 Trim, :1841-1861 ColumnConsensus1, taken first by GetOffsets1 at
// :1219-1223): per pair and side the consensus sequence of the stack and the stack's dimensions.  No stack is stored: the rule over
// plain arrays, the cell a row puts in a column stated once, the windowed form the device runs and its plan, the layout of
// a.close.cons.
//
// No HIP call and no device pointer is dereferenced here by the host, so tests/cpp/test_cons.cc compiles this header with a plain
// host compiler (and once more under -fsanitize=address,undefined) and checks it against cases recorded from tests/cons_oracle.py.
// It is the SECOND restatement of the rule -- written from the reference's text, not from the Python.
//
// The rule (max_width = 400, 10X/DF.cc:590; a pair pi = (e1, e2), es = { e1, inv[e2] } (:504), e = es[ei], ne = hb.Bases(e) =
// kmers[e] + K - 1):
//   rows (:599-612)     locs[ei]: locs(e) in the closer's order (dfk_closer.h), behind them the records the loop for 1 - ei of
//                       :562-585 pushed onto locs[ei]: element 2 pi + (1 - ei) of a.close.partners, in push order.  A read id may
//                       stand in several rows.
//   M (:598-604)        from 0, the maximum of pos + len(id) over the forward rows and of ne - pos over the others.
//   cells (:606-629)    a forward row puts base j at column pos + j where that is >= 0; any other row 3 - base j at column
//                       ne - pos - j - 1 where that is >= 0.  The quality stored is q[j] of the whole PQVec-decoded read, in a char
//                       (ReadStack.h:29,120); a cell is DEFINED iff that char is >= 0 (ReadStack.h:103): a quality of 128 or more
//                       leaves the cell undefined.
//   Trim (:633-634, ReadStack.cc:714-725)   only when M > 400: the columns [M - 400, M) are kept, the rows without a defined cell
//                       among them erased, the order of the others kept.  Without a trim no row is erased, however empty.
//   Reverse (:638, ReadStack.cc:346-353)    when e == inv[e2] (side 1 always; side 0 too when e1 == inv[e2]): the columns reversed,
//                       the bases that were set complemented.
//   consensus (ReadStack.cc:400-404, 1841-1861)   per column four double sums from 0; the rows IN ROW ORDER; a defined cell adds
//                       0.1 for Q0, 0.2 for Q1 and Q2, q otherwise to its base's sum; the result the FIRST maximum
//                       (std::max_element), base 0 where nothing was added.  It runs on the stack as it stands after Reverse: ties
//                       and empty columns do not fall as the complement of the unreversed answer would.
//   The sums are IEEE doubles added one row after the other: 0.2 + 10 + 10 and 20 + 0.1 + 0.1 differ in the last place, and so do
//   0.2 + 37 + 10 + 0.1 and the same four sorted.  No integer tenths, no tree over the rows, no reassociation, no contraction.
//   The result of a pair and a side depends on ( e, es[1 - ei], reversed ) alone.
//
// The cell, stated ONCE (cell_index, cell_base; host and kernels): column sc of the stack as built (before Trim and Reverse) holds,
// of a forward row, base j = sc - pos; of any other, 3 - base j with j = ne - pos - 1 - sc; if 0 <= j < len.  sc >= 0 always.  The
// kept columns are [w0, M), w0 = M - 400 when M > 400, else 0; cols = M - w0; output column c is stack column w0 + c, or, reversed,
// w0 + cols - 1 - c with the base complemented once more.  A row erased by Trim has no defined cell among the kept columns and adds
// nothing: the consensus is over ALL rows in order; rows_kept counts those with a defined cell there (all rows without a trim).
//
// The form the device runs (dfk_cons_kernels.h, dfk_cons.inc; cons_plan() below is its order of work on the host):
//   stacks     element q = 2 pi + ei; its rank k(q) of e in ce; its rows: locs(k(q)), then element q ^ 1 of the partners.
//   dimensions a RANGE of stacks at a time (as many as keep their rows at the cap; DFK_PIDX_RANGE_PAIRS forces small ranges): M
//              per stack, a maximum over its rows that needs the reads' lengths only; the window follows.
//   live rows  an ITEM is a row of a stack of the range.  It is LIVE when its span -- [pos, pos + len) forward, [ne - pos - len,
//              ne - pos) otherwise -- meets the window and len > 0.  Flag, scan, emit: ( id, pos, fw, len ) at the scanned places,
//              the order kept.  On a long edge most of locs(e) lies far from the window and is never touched again.
//   batches    as many stacks of the range as fit the room (or stacks_per_batch).  The reads the live rows of the batch name,
//              each ONCE, ascending: their packed bases and PQVec bytes gathered on the host and sent up; a thread a read decodes
//              one quality byte a base; a stream that does not hold exactly len values refuses the call.
//   consensus  a workgroup a stack, a lane a column (two where cols > 256): the live rows walked once in order, their headers
//              staged through LDS; a lane whose column the row covers loads the 2-bit base and the quality byte and adds a double.
//              The first maximum is written at the scanned place.  No atomics take part in the result.
//
// The file (dfk_cons_write).  Numbers are little-endian, no byte undefined.
//   a.close.cons   "DFKCCON1" | u64 n = 2 * n_pairs | (n + 1) x u64 starts, in bases | n x 16-byte dims { u32 rows, u32 rows_kept,
//                  i32 M, u32 cols } | the bases, a byte each (0..3) | zero bytes to a multiple of 8.  Element 2 pi + ei is
//                  stacks[ei] of pair pi; starts[k + 1] - starts[k] == cols[k].
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define DFK_CN_HD __host__ __device__ inline
#else
#define DFK_CN_HD inline
#endif

namespace dfk_cons {

constexpr int64_t MAX_WIDTH = 400;                 // 10X/DF.cc:590
constexpr uint64_t SALT = 0xEEEEull;               // k_digest_seq's, over the dims as u32 words, then the bases one value each
constexpr uint32_t GROUP = 256;                    // lanes of a workgroup: a stack's columns in ceil(400 / 256) = 2 rounds

// a row as the tables hold it: two words, ( id, pos | fw << 32 ) -- the locs record and the partners' record alike
DFK_CN_HD uint64_t rec_id(const uint64_t* recs, uint64_t i) { return recs[2 * i]; }
DFK_CN_HD int32_t rec_pos(const uint64_t* recs, uint64_t i) { return (int32_t)(uint32_t)recs[2 * i + 1]; }
DFK_CN_HD bool rec_fw(const uint64_t* recs, uint64_t i) { return ((recs[2 * i + 1] >> 32) & 1u) != 0; }
// the column behind a row's last cell: what it gives M (:603-604), and where its span ends
DFK_CN_HD int64_t row_end(bool fw, int32_t pos, uint32_t len, int32_t ne) { return fw ? (int64_t)pos + (int64_t)len : (int64_t)ne - (int64_t)pos; }
DFK_CN_HD int64_t window_start(int64_t M) { return M > MAX_WIDTH ? M - MAX_WIDTH : 0; }            // :633-634
DFK_CN_HD bool row_live(bool fw, int32_t pos, uint32_t len, int32_t ne, int64_t w0) { return len != 0 && row_end(fw, pos, len, ne) > w0; }
// the stack column of output column c
DFK_CN_HD int64_t stack_column(int64_t w0, int64_t cols, bool reversed, int64_t c) { return reversed ? w0 + cols - 1 - c : w0 + c; }
// THE CELL: the base index j of the row's read that column sc of the stack holds, or -1
DFK_CN_HD int64_t cell_index(bool fw, int32_t pos, uint32_t len, int32_t ne, int64_t sc)
{
    const int64_t j = fw ? sc - (int64_t)pos : (int64_t)ne - (int64_t)pos - 1 - sc;               // :617 p = pos + j; :627 ne - p - 1
    return j >= 0 && j < (int64_t)len ? j : -1;
}
// ... and the base the consensus sees there: complemented by a row that is not forward (:627), and once more by Reverse
DFK_CN_HD uint32_t cell_base(uint32_t b, bool fw, bool reversed) { return fw != reversed ? b : 3u - b; }
DFK_CN_HD bool cell_defined(uint8_t q) { return q < 128u; }                                         // the char is >= 0
DFK_CN_HD uint32_t base_at(const uint8_t* packed, uint64_t j) { return (packed[j >> 2] >> (2 * (j & 3))) & 3u; }
// ColumnConsensus1's switch (:1854-1858) and its sum: one IEEE add, nothing else
DFK_CN_HD double quality_value(uint8_t q) { return q == 0 ? .1 : q <= 2 ? .2 : (double)q; }
DFK_CN_HD void add_cell(double* sum, uint32_t base, uint8_t q)
{
    const double val = quality_value(q);
    switch (base) {
        case 0: sum[0] += val; break;
        case 1: sum[1] += val; break;
        case 2: sum[2] += val; break;
        default: sum[3] += val; break;
    }
}
DFK_CN_HD uint32_t first_max(const double* sum)                                                     // std::max_element: the first
{
    uint32_t best = 0;
    for (uint32_t b = 1; b < 4; ++b) if (sum[best] < sum[b]) best = b;
    return best;
}
// one row's cell in output column c added to the column's sums; true if the cell is defined
DFK_CN_HD bool add_row(double* sum, bool fw, int32_t pos, uint32_t len, int32_t ne, bool reversed, int64_t sc, const uint8_t* bases, const uint8_t* quals)
{
    const int64_t j = cell_index(fw, pos, len, ne, sc);
    if (j < 0) return false;
    const uint8_t q = quals[j];
    if (!cell_defined(q)) return false;
    add_cell(sum, cell_base(base_at(bases, (uint64_t)j), fw, reversed), q);
    return true;
}
// the last i in [0, n) with first[i] <= x, first ascending with first[0] <= x
DFK_CN_HD uint64_t owner_of(const uint64_t* first, uint64_t n, uint64_t x)
{
    uint64_t lo = 0, hi = n;
    while (hi - lo > 1) { const uint64_t mid = lo + (hi - lo) / 2; if (first[mid] <= x) lo = mid; else hi = mid; }
    return lo;
}
// where an ascending list of distinct ids holds id (the caller knows it is there)
DFK_CN_HD uint64_t slot_of(const uint32_t* ids, uint64_t n, uint32_t id)
{
    uint64_t lo = 0, hi = n;
    while (lo < hi) { const uint64_t mid = lo + (hi - lo) / 2; if (ids[mid] < id) lo = mid + 1; else hi = mid; }
    return lo;
}

} // namespace dfk_cons

// ---------------------------------------------------------------------------------------------------------------- host only
#include <algorithm>
#include <vector>
#include "dfk_paths_plan.h"   // pidx_next_range, prefix_sums

namespace dfk_cons {

struct Dim { uint32_t rows, rows_kept; int32_t M; uint32_t cols; };
static_assert(sizeof(Dim) == 16, "a.close.cons dims");

// everything as plain arrays: the graph, the closer's locs in dfk_closer_fetch's forms, the partners in dfk_partners_fetch's, the reads
struct Input {
    uint64_t n_edges; const int32_t* inv; const int32_t* kmers; uint32_t K;
    uint64_t n_ce; const uint64_t* ce; const uint64_t* loc_first; const uint64_t* locs /* two words a record */;
    const uint64_t* part_first /* [2 * n_pairs + 1] */; const uint64_t* parts /* two words a record */;
    uint64_t n_reads; const uint8_t* read_packed; const uint64_t* read_off /* [N + 1], bytes */; const uint32_t* read_len;
    const uint8_t* pq; const uint64_t* pq_off /* [N + 1] */;
};

struct HostResult {
    std::vector<uint64_t> starts;                  // [2 * n_pairs + 1]
    std::vector<Dim> dims;
    std::vector<uint8_t> bases;
    uint64_t rows = 0, live = 0, rows_kept = 0, trimmed = 0, reversed = 0, columns = 0, added = 0, decoded = 0, batches = 0, ranges = 0;
};

// PQVecEncoder::decode (feudal/PQVec.cc:129-188) of one read on the host; false if the stream does not hold exactly n values
inline bool decode_quals(const uint8_t* pq, uint64_t p, uint64_t end, uint8_t* out, uint32_t n)
{
    uint32_t idx = 0;
    while (p < end) {
        const uint32_t nQs = pq[p];
        if (!nQs) break;
        if (p + 3 > end) return false;
        const uint32_t hdr = pq[p + 1] | ((uint32_t)pq[p + 2] << 8), nBits = hdr & 7u, minQ = (hdr >> 3) & 63u;
        const uint64_t blk = ((uint64_t)nQs * nBits + 24) >> 3;
        if (p + blk > end || idx + nQs > n) return false;
        uint64_t bit = 8 * (p + 1) + 9;
        for (uint32_t i = 0; i < nQs; ++i) {
            uint32_t v = 0;
            for (uint32_t k = 0; k < nBits; ++k, ++bit) v |= ((uint32_t)(pq[bit >> 3] >> (bit & 7)) & 1u) << k;
            out[idx++] = (uint8_t)(minQ + v);
        }
        p += blk;
    }
    return idx == n;
}

inline uint64_t rank_in(const uint64_t* ce, uint64_t n_ce, uint64_t e)
{
    const uint64_t k = (uint64_t)(std::lower_bound(ce, ce + n_ce, e) - ce);
    return k < n_ce && ce[k] == e ? k : n_ce;
}
// per stack q = 2 pi + ei: the rank of es[ei] and whether Reverse applies (:638).  -1: a pair names an edge outside [0, E); -2: a
// closer edge of a pair is not in ce
inline int stacks_of(const Input& I, const int32_t* pairs, uint64_t n_pairs, std::vector<uint32_t>* side_rank, std::vector<uint8_t>* reversed)
{
    side_rank->assign(2 * n_pairs, 0); reversed->assign(2 * n_pairs, 0);
    for (uint64_t i = 0; i < 2 * n_pairs; ++i) if (pairs[i] < 0 || (uint64_t)pairs[i] >= I.n_edges) return -1;
    for (uint64_t pi = 0; pi < n_pairs; ++pi) {
        const uint64_t es[2] = {(uint64_t)pairs[2 * pi], (uint64_t)I.inv[pairs[2 * pi + 1]]};    // :504
        for (int ei = 0; ei < 2; ++ei) {
            const uint64_t k = rank_in(I.ce, I.n_ce, es[ei]);
            if (k == I.n_ce) return -2;
            (*side_rank)[2 * pi + ei] = (uint32_t)k;
            (*reversed)[2 * pi + ei] = es[ei] == (uint64_t)I.inv[pairs[2 * pi + 1]];              // :638
        }
    }
    return 0;
}
inline int32_t bases_of_edge(const Input& I, uint64_t e) { return (int32_t)((int64_t)I.kmers[e] + (int64_t)I.K - 1); }   // hb.Bases(e)

// ---- the literal transcription for one pair and side: Closomatic.cc:589-640 and the readstack's members as they stand, the stack
// materialised.  -3: a read's PQVec stream does not hold len values
struct Triple { int64_t id; int pos; bool fw; };
// the stack as it stands after Trim and Reverse (:598-638): what Consensus1 below and Merge (dfk_closures.h) take
struct Grids { std::vector<std::vector<int8_t>> bases_, quals_; int rows = 0, cols = 0; };
inline int stack_grids(const Input& I, int32_t e2, uint64_t e, const std::vector<Triple>& locs, Dim* dim, Grids* G, HostResult* counters)
{
    const int ne = bases_of_edge(I, e);                                                          // :592
    auto len_of = [&](int64_t id) { return (int)I.read_len[id]; };
    auto base_of = [&](int64_t id, int j) { return (int)base_at(I.read_packed + I.read_off[id], (uint64_t)j); };
    int M = 0;                                                                                   // :598
    for (size_t i = 0; i < locs.size(); i++) {                                                   // :599
        if (locs[i].fw) M = std::max(M, locs[i].pos + len_of(locs[i].id));                       // :603
        else M = std::max(M, ne - locs[i].pos);                                                  // :604
    }
    int rows = (int)locs.size(), cols = M;
    std::vector<std::vector<int8_t>> bases_(rows, std::vector<int8_t>(M, ' ')), quals_(rows, std::vector<int8_t>(M, -1));    // :605
    for (size_t i = 0; i < locs.size(); i++) {                                                   // :606
        const int64_t id = locs[i].id;
        std::vector<uint8_t> q((size_t)len_of(id) + 1);                                          // :608-609
        if (!decode_quals(I.pq, I.pq_off[id], I.pq_off[id + 1], q.data(), (uint32_t)len_of(id))) return -3;
        const int pos = locs[i].pos;
        if (locs[i].fw) {                                                                        // :614
            for (int j = 0; j < len_of(id); j++) {
                const int p = pos + j;
                if (p >= 0) { bases_[i][p] = (int8_t)base_of(id, j); quals_[i][p] = (int8_t)q[j]; }      // :618-620
            }
        } else {
            for (int j = 0; j < len_of(id); j++) {
                const int p = pos + j;
                if (ne - p - 1 >= 0) { bases_[i][ne - p - 1] = (int8_t)(3 - base_of(id, j)); quals_[i][ne - p - 1] = (int8_t)q[j]; }   // :626-629
            }
        }
    }
    dim->rows = (uint32_t)rows; dim->M = M;
    if (cols > (int)MAX_WIDTH) {                                                                 // :633-634; ReadStack.cc:714-725
        const int start = cols - (int)MAX_WIDTH, stop = cols;
        std::vector<std::vector<int8_t>> b2, q2;
        for (int i = 0; i < rows; i++) {
            bool to_remove = true;
            for (int j = start; j < stop; j++) if (quals_[i][j] >= 0) { to_remove = false; break; }
            if (to_remove) continue;
            b2.emplace_back(bases_[i].begin() + start, bases_[i].begin() + stop); q2.emplace_back(quals_[i].begin() + start, quals_[i].begin() + stop);
        }
        bases_.swap(b2); quals_.swap(q2);
        cols = stop - start; rows = (int)bases_.size();
        ++counters->trimmed;
    }
    if (e == (uint64_t)I.inv[e2]) {                                                              // :638; ReadStack.cc:346-353
        for (int i = 0; i < rows; i++) {
            std::reverse(bases_[i].begin(), bases_[i].end());
            for (int j = 0; j < cols; j++) if (bases_[i][j] != ' ') bases_[i][j] = (int8_t)(3 - bases_[i][j]);
            std::reverse(quals_[i].begin(), quals_[i].end());
        }
        ++counters->reversed;
    }
    dim->rows_kept = (uint32_t)rows; dim->cols = (uint32_t)cols;
    G->bases_.swap(bases_); G->quals_.swap(quals_); G->rows = rows; G->cols = cols;
    return 0;
}
inline int stack_literal(const Input& I, int32_t e2, uint64_t e, const std::vector<Triple>& locs, Dim* dim, std::vector<uint8_t>* con, HostResult* counters)
{
    Grids G;
    if (int rc = stack_grids(I, e2, e, locs, dim, &G, counters)) return rc;
    const std::vector<std::vector<int8_t>>& bases_ = G.bases_; const std::vector<std::vector<int8_t>>& quals_ = G.quals_;
    const int rows = G.rows, cols = G.cols;
    con->assign((size_t)cols, 0);
    for (int c = 0; c < cols; c++) {                                                             // ReadStack.cc:400-404
        double sum[4]{0., 0., 0., 0.};                                                           // :1846
        for (int i = 0; i < rows; i++) {                                                         // :1849
            const int q = quals_[i][c];
            if (q < 0) continue;
            double val;
            switch (q) { case 0: val = .1; break; case 1: val = .2; break; case 2: val = .2; break; default: val = q; break; }
            sum[(int)bases_[i][c]] += val;
            ++counters->added;
        }
        (*con)[c] = (uint8_t)(std::max_element(sum, sum + 4) - sum);                             // :1861
    }
    return 0;
}

// -1, -2: stacks_of's; -3: a PQVec stream of the wrong length
inline int cons_literal(const Input& I, const int32_t* pairs, uint64_t n_pairs, HostResult* R)
{
    std::vector<uint32_t> side_rank; std::vector<uint8_t> reversed;
    if (int rc = stacks_of(I, pairs, n_pairs, &side_rank, &reversed)) return rc;
    R->starts.assign(1, 0);
    for (uint64_t pi = 0; pi < n_pairs; ++pi) {
        const uint64_t es[2] = {(uint64_t)pairs[2 * pi], (uint64_t)I.inv[pairs[2 * pi + 1]]};
        for (int ei = 0; ei < 2; ++ei) {
            std::vector<Triple> locs;                                                            // locs[ei] as :585 leaves it
            const uint64_t k = side_rank[2 * pi + ei], po = 2 * pi + (1 - ei);
            for (uint64_t j = I.loc_first[k]; j < I.loc_first[k + 1]; ++j) locs.push_back(Triple{(int64_t)rec_id(I.locs, j), rec_pos(I.locs, j), rec_fw(I.locs, j)});
            for (uint64_t j = I.part_first[po]; j < I.part_first[po + 1]; ++j) locs.push_back(Triple{(int64_t)rec_id(I.parts, j), rec_pos(I.parts, j), rec_fw(I.parts, j)});
            Dim d{}; std::vector<uint8_t> con;
            if (int rc = stack_literal(I, pairs[2 * pi + 1], es[ei], locs, &d, &con, R)) return rc;
            R->dims.push_back(d); R->bases.insert(R->bases.end(), con.begin(), con.end()); R->starts.push_back(R->bases.size());
            R->rows += d.rows; R->rows_kept += d.rows_kept; R->columns += d.cols;
        }
    }
    return 0;
}

// ---- the plan
// Dimensions and live rows are found a range of STACKS at a time: as many stacks as keep their rows at the cap.  A row costs its
// flag and its place (two u64) and, where it is live, its header (id, pos, fw and len: 12 bytes) and the slot of its read.
constexpr uint64_t BYTES_PER_ROW = 32;
inline uint64_t row_cap(uint64_t free_now, uint64_t forced) { return forced ? forced : std::max<uint64_t>(1ull << 18, free_now / 2 / BYTES_PER_ROW); }
inline dfk::PidxRange next_range(const uint64_t* first, uint64_t n, uint64_t q0, uint64_t cap) { return dfk::pidx_next_range(first, n, q0, cap); }
// A batch of stacks: a stack costs its fixed words (64 bytes), its columns, and for every live row the row's slot and -- counted per
// row though a read crosses once -- the read's packed bases, PQVec bytes (at most 3 + len + 1 a block of 255) and quality bytes.
// cost_first: the prefix sums.  A batch holds `forced` stacks, or with forced == 0 as many as keep the cost at `room`, one at least.
constexpr uint64_t BYTES_PER_STACK = 64 + (uint64_t)MAX_WIDTH;
inline uint64_t live_row_cost(uint32_t len) { return 48 + (len + 3) / 4 + 2 * (uint64_t)len + 4 * ((uint64_t)len / 255 + 1); }
inline uint64_t batch_room(uint64_t free_now) { return std::max<uint64_t>(1ull << 20, free_now / 2); }
inline uint64_t next_batch(const uint64_t* cost_first, uint64_t n, uint64_t b0, uint64_t room, uint64_t forced)
{
    if (forced) return std::min(n, b0 + forced);
    uint64_t b1 = b0 + 1;
    while (b1 < n && cost_first[b1 + 1] - cost_first[b0] <= room) ++b1;
    return b1;
}
inline unsigned cons_grid(uint64_t n_stacks, unsigned cus) { return (unsigned)std::max<uint64_t>(1, std::min<uint64_t>(n_stacks, 32ull * cus)); }   // a workgroup a stack

// a stack's row r: from locs(k), or behind them from the partners' element
struct RowView { const uint64_t* recs; uint64_t at; };
inline RowView row_of(const Input& I, uint64_t k, uint64_t po, uint64_t r)
{
    const uint64_t nl = I.loc_first[k + 1] - I.loc_first[k];
    return r < nl ? RowView{I.locs, I.loc_first[k] + r} : RowView{I.parts, I.part_first[po] + (r - nl)};
}

// The device version's order of work on the host, for the CPU test.  stacks_per_batch 0 = what fits `room`; -3: a PQVec stream of
// the wrong length
inline int cons_plan(const Input& I, const int32_t* pairs, uint64_t n_pairs, uint64_t stacks_per_batch, uint64_t room, uint64_t rows_cap, HostResult* R)
{
    std::vector<uint32_t> side_rank; std::vector<uint8_t> reversed;
    if (int rc = stacks_of(I, pairs, n_pairs, &side_rank, &reversed)) return rc;
    const uint64_t n_stacks = 2 * n_pairs;
    std::vector<uint64_t> n_rows(n_stacks);
    for (uint64_t q = 0; q < n_stacks; ++q) n_rows[q] = (I.loc_first[side_rank[q] + 1] - I.loc_first[side_rank[q]]) + (I.part_first[(q ^ 1) + 1] - I.part_first[q ^ 1]);
    const std::vector<uint64_t> rfirst = dfk::prefix_sums(n_rows.data(), n_stacks);
    R->dims.assign(n_stacks, Dim{}); R->starts.assign(n_stacks + 1, 0);
    std::vector<std::vector<uint8_t>> con(n_stacks);
    for (uint64_t q0 = 0; q0 < n_stacks;) {
        const uint64_t q1 = next_range(rfirst.data(), n_stacks, q0, rows_cap).e1, ns = q1 - q0, n_items = rfirst[q1] - rfirst[q0];
        ++R->ranges;
        // dimensions (a wave a stack)
        std::vector<int64_t> M(ns, 0), w0(ns);
        std::vector<int32_t> ne(ns);
        for (uint64_t s = 0; s < ns; ++s) {
            const uint64_t q = q0 + s, k = side_rank[q];
            ne[s] = bases_of_edge(I, I.ce[k]);
            for (uint64_t r = 0; r < n_rows[q]; ++r) {
                const RowView v = row_of(I, k, q ^ 1, r);
                M[s] = std::max(M[s], row_end(rec_fw(v.recs, v.at), rec_pos(v.recs, v.at), I.read_len[rec_id(v.recs, v.at)], ne[s]));
            }
            w0[s] = window_start(M[s]);
        }
        // live rows (a thread an item): flag, scan, emit
        std::vector<uint64_t> rel(ns + 1), flag(n_items + 1, 0), place(n_items + 1, 0);
        for (uint64_t s = 0; s <= ns; ++s) rel[s] = rfirst[q0 + s] - rfirst[q0];
        auto item = [&](uint64_t i, uint64_t* s) { *s = owner_of(rel.data(), ns, i); return row_of(I, side_rank[q0 + *s], (q0 + *s) ^ 1, i - rel[*s]); };
        for (uint64_t i = 0; i < n_items; ++i) {
            uint64_t s; const RowView v = item(i, &s);
            flag[i] = row_live(rec_fw(v.recs, v.at), rec_pos(v.recs, v.at), I.read_len[rec_id(v.recs, v.at)], ne[s], w0[s]) ? 1u : 0u;
        }
        for (uint64_t i = 0; i < n_items; ++i) place[i + 1] = place[i] + flag[i];
        const uint64_t n_live = place[n_items];
        std::vector<uint32_t> l_id(n_live), l_len(n_live); std::vector<int32_t> l_pos(n_live); std::vector<uint8_t> l_fw(n_live);
        for (uint64_t i = 0; i < n_items; ++i) {
            if (!flag[i]) continue;
            uint64_t s; const RowView v = item(i, &s);
            l_id[place[i]] = (uint32_t)rec_id(v.recs, v.at); l_pos[place[i]] = rec_pos(v.recs, v.at); l_fw[place[i]] = rec_fw(v.recs, v.at); l_len[place[i]] = I.read_len[rec_id(v.recs, v.at)];
        }
        std::vector<uint64_t> lfirst(ns + 1);
        for (uint64_t s = 0; s <= ns; ++s) lfirst[s] = place[rel[s]];
        R->live += n_live;
        // batches of stacks
        std::vector<uint64_t> cost(ns);
        for (uint64_t s = 0; s < ns; ++s) { cost[s] = BYTES_PER_STACK; for (uint64_t l = lfirst[s]; l < lfirst[s + 1]; ++l) cost[s] += live_row_cost(l_len[l]); }
        const std::vector<uint64_t> cfirst = dfk::prefix_sums(cost.data(), ns);
        for (uint64_t b0 = 0; b0 < ns;) {
            const uint64_t b1 = next_batch(cfirst.data(), ns, b0, room, stacks_per_batch);
            ++R->batches;
            // the reads of the batch, each once, ascending; the gather; the decode (a thread a read)
            std::vector<uint32_t> ids(l_id.begin() + lfirst[b0], l_id.begin() + lfirst[b1]);
            std::sort(ids.begin(), ids.end()); ids.erase(std::unique(ids.begin(), ids.end()), ids.end());
            std::vector<uint64_t> b_at(ids.size() + 1, 0), q_at(ids.size() + 1, 0), p_at(ids.size() + 1, 0);
            for (size_t i = 0; i < ids.size(); ++i) {
                const uint32_t len = I.read_len[ids[i]];
                b_at[i + 1] = b_at[i] + (len + 3) / 4; q_at[i + 1] = q_at[i] + len; p_at[i + 1] = p_at[i] + (I.pq_off[ids[i] + 1] - I.pq_off[ids[i]]);
            }
            std::vector<uint8_t> bases(b_at.back()), pq(p_at.back()), quals(q_at.back());        // (capacity == size: a read past the end is the sanitizer's to see)
            for (size_t i = 0; i < ids.size(); ++i) {
                std::copy(I.read_packed + I.read_off[ids[i]], I.read_packed + I.read_off[ids[i]] + (b_at[i + 1] - b_at[i]), bases.begin() + b_at[i]);
                std::copy(I.pq + I.pq_off[ids[i]], I.pq + I.pq_off[ids[i] + 1], pq.begin() + p_at[i]);
            }
            for (size_t i = 0; i < ids.size(); ++i)
                if (!decode_quals(pq.data(), p_at[i], p_at[i + 1], quals.data() + q_at[i], I.read_len[ids[i]])) return -3;
            R->decoded += ids.size();
            // the consensus (a workgroup a stack, a lane a column, the live rows in order)
            for (uint64_t s = b0; s < b1; ++s) {
                const uint64_t q = q0 + s;
                const int64_t cols = M[s] - w0[s];
                const bool trimmed = M[s] > MAX_WIDTH, rev = reversed[q] != 0;
                std::vector<uint8_t> defined(lfirst[s + 1] - lfirst[s], 0);
                con[q].assign((size_t)cols, 0);
                for (int64_t c = 0; c < cols; ++c) {
                    const int64_t sc = stack_column(w0[s], cols, rev, c);
                    double sum[4] = {0., 0., 0., 0.};
                    for (uint64_t l = lfirst[s]; l < lfirst[s + 1]; ++l) {
                        const uint64_t slot = slot_of(ids.data(), ids.size(), l_id[l]);
                        if (add_row(sum, l_fw[l] != 0, l_pos[l], l_len[l], ne[s], rev, sc, bases.data() + b_at[slot], quals.data() + q_at[slot])) { defined[l - lfirst[s]] = 1; ++R->added; }
                    }
                    con[q][(size_t)c] = (uint8_t)first_max(sum);
                }
                uint64_t kept = 0;
                for (uint8_t d : defined) kept += d;
                R->dims[q] = Dim{(uint32_t)n_rows[q], (uint32_t)(trimmed ? kept : n_rows[q]), (int32_t)M[s], (uint32_t)cols};
                R->trimmed += trimmed; R->reversed += rev;
            }
            b0 = b1;
        }
        q0 = q1;
    }
    for (uint64_t q = 0; q < n_stacks; ++q) {
        R->bases.insert(R->bases.end(), con[q].begin(), con[q].end()); R->starts[q + 1] = R->bases.size();
        R->rows += R->dims[q].rows; R->rows_kept += R->dims[q].rows_kept; R->columns += R->dims[q].cols;
    }
    return 0;
}

// ---- the file's fixed parts
constexpr const char* MAGIC = "DFKCCON1";
inline uint64_t dims_at(uint64_t n) { return 16 + 8 * (n + 1); }
inline uint64_t bases_at(uint64_t n) { return dims_at(n) + 16 * n; }
inline uint64_t padded(uint64_t n_bases) { return (n_bases + 7) & ~7ull; }
inline uint64_t file_size(uint64_t n, uint64_t n_bases) { return bases_at(n) + padded(n_bases); }

} // namespace dfk_cons
