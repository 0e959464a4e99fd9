// superplus_amd/csrc/dfk_closures.h -- CloseGap2's closures per pair (10X/Closomatic.cc:651-660; paths/long/ReadStack.cc:355-398
// Merge, :406-427 Consensus1 with qualities, :26-45 BaseMetrics): for a pair with one or two surviving offsets the two stacks merged
// at each offset and the consensus of the merged stack -- the basevector CloseGap2 pushes onto `closures`, the only thing it returns.
// No stack is stored: the rule over plain arrays, the merged width, the two column maps and the (sum, id) maximum stated once, the
// form the device runs and its plan, the layout of a.close.closures.
//
// No HIP call and no device pointer is dereferenced here by the host, so tests/cpp/test_closures.cc compiles this header with a plain
// host compiler (and once more under -fsanitize=address,undefined) and checks it against cases recorded from
// tests/closures_oracle.py.  It is the SECOND restatement of the rule -- written from the reference's text, not from the Python.
//
// The rule (pair pi; o = the offsets GetOffsets1 returned for it: the state-0 records of a.close.offsets, in record order):
//   which pairs (:651)    o.size() == 0 or o.size() > 2: no closure.  Otherwise one closure per offset, in that order; the closures of
//                         all pairs follow in pair order (CloseGap2's share of `closures`, RunStages.cc:290-324).
//   Merge (ReadStack.cc:355-398)   stacks[0] (a copy, :653) and stacks[1] as they stand after Trim and Reverse -- dfk_cons.h's cols1,
//                         cols2, w0, reversed.  left_ext1 = Max(0, -off), right_ext1 = Max(0, off + cols2 - cols1): every row of
//                         stack 0 is shifted right by left_ext1 and filled with ' ' / -1 to left_ext1 + cols1 + right_ext1.  The rows
//                         of stack 1 are appended; left_ext2 = Max(0, off), right_ext2 = Max(0, cols1 - (off + cols2)): each is
//                         shifted by left_ext2 and filled to left_ext2 + cols2 + right_ext2.  cols_ = bases_[0].size() (:398).
//                         Both forms are C = max(cols1, off + cols2) - min(0, off) (merged_cols; both_forms says so and the test
//                         checks it), so it does not matter whose row bases_[0] is.  Merged column c holds stack 0's output column
//                         c - max(0, -off) and stack 1's output column c - max(0, off) where those fall inside their stacks
//                         (column_of_side).  Rows: stack 0's in their order, then stack 1's in theirs; Reverse reorders no rows.
//                         A row erased by Trim has no defined cell in the window: as in dfk_cons.h the walk is over all live rows.
//   Consensus1 (:406-427)  per merged column four doubles from 0 (BaseMetrics), the rows in the order above; a cell with Qual >= 0
//                         adds 0.1 for Q0, 0.2 for Q1 and Q2, q otherwise (:415-418: dfk_cons::quality_value; the same char rule: a
//                         quality of 128 or more is undefined).  Then mx.reverseSort() -- std::sort with std::greater<std::pair<
//                         double, int>> (:41) -- and con = mx.id(0): the base of the GREATEST (sum, id) pair.  Ties go to the highest
//                         base id and a column nothing was added to gives base 3 (last_max) -- the opposite of ColumnConsensus1's
//                         first maximum that a.close.cons holds, so a closure is not a splice of con1 and con2.  conq and the
//                         max_qcomp block are thrown away by the caller (:656-660) and are not built.
//   The sums cross the stack boundary: a column's sum is ((stack 0's rows ...) + stack 1's first row) + ..., IEEE doubles added one
//   row after the other.  20 from stack 0 then 0.1, 0.1 from stack 1 is 20.200000000000003; 0.2 then 10, 10 is 20.2: base 0 wins,
//   where per-stack sums added would tie (20.2 and 20.2) and base 1 would win.  No per-stack sums, no tree, no reassociation.
//   The one undefined place: both stacks without rows -- the reference reads bases_[0] of an empty vector (:398).  Decided here: the
//   closure has C columns of base 3 (what the walk over no rows gives), and `rowless` counts such closures.
//
// The form the device runs (dfk_closures_kernels.h, dfk_closures.inc; closures_plan() below is its order of work on the host):
//   closable   the pairs with one or two offsets, in pair order; ONLY their stacks are touched: two a closable pair, the partners'
//              records of those pairs alone.  Ranges, dimensions, live rows, the gather of a batch's distinct reads and the decode are
//              dfk_cons.inc's own steps (cn_*), shared with cons_build; a range holds whole pairs.
//   batches    as many closures of the range as fit the room (or closures_per_batch); the reads the live rows of their pairs' stacks
//              name, each once.  Two closures of one pair may fall into two batches: the pair's reads then go up twice.
//   consensus  a workgroup a TILE of 256 merged columns of a closure (4 tiles a closure: 800 columns at most), a lane a column: the
//              live rows of stack 0, then those of stack 1, walked once in order, their headers staged through LDS 256 at a time; a
//              lane whose column the row covers adds one double.  last_max is written at the closure's place.  No atomics.
//   rows       a record's rows = rows_kept of both stacks: all rows without a trim, else the live rows that had a defined cell in
//              some merged column (every kept column of a stack is some merged column): a flag a live row, every writer writes 1.
//
// The file (dfk_closures_write).  Numbers are little-endian, no byte undefined.
//   a.close.closures   "DFKCCLS1" | u64 n closures | u64 n_pairs | (n_pairs + 1) x u64 first closure of each pair | (n + 1) x u64
//                      starts, in bases | n x 16-byte { u32 pair, i32 offset, u32 cols, u32 rows } | the bases, a byte each (0..3) |
//                      zero bytes to a multiple of 8.
#pragma once
#include <stdint.h>
#include "dfk_cons.h"

namespace dfk_closures {

constexpr uint64_t SALT = 0xF1F1ull;               // k_digest_seq's, over the records as u32 words, then the bases one value each
constexpr uint32_t GROUP = dfk_cons::GROUP;        // lanes of a workgroup: a tile of merged columns
constexpr int64_t MAX_COLS = 2 * dfk_cons::MAX_WIDTH;                         // abutting stacks of 400 columns each
constexpr uint32_t TILES = (uint32_t)((MAX_COLS + GROUP - 1) / GROUP);        // 4

// Merge's width: left_ext1 + cols1 + right_ext1 == left_ext2 + cols2 + right_ext2 == this, for off in [-cols2, cols1]
DFK_CN_HD int64_t merged_cols(int64_t cols1, int64_t cols2, int64_t off)
{
    const int64_t hi = cols1 > off + cols2 ? cols1 : off + cols2, lo = off < 0 ? off : 0;
    return hi - lo;
}
DFK_CN_HD bool offset_ok(int64_t cols1, int64_t cols2, int64_t off) { return off >= -cols2 && off <= cols1; }
// the output column of stack `side` that merged column c holds, or -1
DFK_CN_HD int64_t column_of_side(int side, int64_t cols, int64_t off, int64_t c)
{
    const int64_t left_ext = side == 0 ? (off < 0 ? -off : 0) : (off > 0 ? off : 0);                 // :357, :373
    const int64_t x = c - left_ext;
    return x >= 0 && x < cols ? x : -1;
}
// mx.reverseSort(); mx.id(0): the base of the greatest (sum, id) pair
DFK_CN_HD uint32_t last_max(const double* sum)
{
    uint32_t best = 0;
    for (uint32_t b = 1; b < 4; ++b) if (!(sum[b] < sum[best])) best = b;
    return best;
}

} // namespace dfk_closures

// ---------------------------------------------------------------------------------------------------------------- host only
#include <functional>
#include <utility>

namespace dfk_closures {

struct Rec { uint32_t pair; int32_t offset; uint32_t cols, rows; };
static_assert(sizeof(Rec) == 16, "a.close.closures records");

struct HostResult {
    std::vector<uint64_t> pair_first;              // [n_pairs + 1]
    std::vector<uint64_t> starts;                  // [n + 1]
    std::vector<Rec> recs;
    std::vector<uint8_t> bases;
    uint64_t closable = 0, over = 0, columns = 0, added = 0, live = 0, empty = 0, shorter = 0, rowless = 0, batches = 0, ranges = 0;
};

// the two forms of Merge's width, as it computes them (:357-358, :373-374)
inline void both_forms(int cols1, int cols2, int offset, int* form1, int* form2)
{
    const int left_ext1 = std::max(0, -offset), right_ext1 = std::max(0, offset + cols2 - cols1);
    const int left_ext2 = std::max(0, offset), right_ext2 = std::max(0, cols1 - (offset + cols2));
    *form1 = left_ext1 + cols1 + right_ext1; *form2 = left_ext2 + cols2 + right_ext2;
}

// readstack::Merge as written, on the grids (only what Consensus1 reads: bases_, quals_, cols_)
inline void merge_literal(dfk_cons::Grids* t, const dfk_cons::Grids& s, const int offset)
{
    std::vector<std::vector<int8_t>>& bases_ = t->bases_; std::vector<std::vector<int8_t>>& quals_ = t->quals_;
    int rows1 = t->rows, rows2 = s.rows, cols1 = t->cols, cols2 = s.cols;                         // :356
    int left_ext1 = std::max(0, -offset);
    int right_ext1 = std::max(0, offset + cols2 - cols1);
    for (int i = 0; i < rows1; i++) {
        if (left_ext1 > 0) {
            bases_[i].resize(left_ext1 + cols1);
            quals_[i].resize(left_ext1 + cols1);
            for (int j = left_ext1 + cols1 - 1; j >= left_ext1; j--) { bases_[i][j] = bases_[i][j - left_ext1]; quals_[i][j] = quals_[i][j - left_ext1]; }
            for (int j = 0; j < left_ext1; j++) { bases_[i][j] = ' '; quals_[i][j] = -1; }
        }
        bases_[i].resize(bases_[i].size() + right_ext1, ' ');
        quals_[i].resize(quals_[i].size() + right_ext1, -1);
    }
    bases_.insert(bases_.end(), s.bases_.begin(), s.bases_.end());                                // :371-372
    quals_.insert(quals_.end(), s.quals_.begin(), s.quals_.end());
    int left_ext2 = std::max(0, offset);
    int right_ext2 = std::max(0, cols1 - (offset + cols2));
    for (int i = 0; i < rows2; i++) {
        int ip = rows1 + i;
        if (left_ext2 > 0) {
            bases_[ip].resize(left_ext2 + cols2);
            quals_[ip].resize(left_ext2 + cols2);
            for (int j = left_ext2 + cols2 - 1; j >= left_ext2; j--) { bases_[ip][j] = bases_[ip][j - left_ext2]; quals_[ip][j] = quals_[ip][j - left_ext2]; }
            for (int j = 0; j < left_ext2; j++) { bases_[ip][j] = ' '; quals_[ip][j] = -1; }
        }
        bases_[ip].resize(bases_[ip].size() + right_ext2, ' ');
        quals_[ip].resize(quals_[ip].size() + right_ext2, -1);
    }
    t->rows = rows1 + rows2;
    t->cols = t->rows ? (int)bases_[0].size() : (int)merged_cols(cols1, cols2, offset);            // :398; without rows: the rule above
}

// readstack::Consensus1( con, conq ) as written, con alone (:406-420)
inline void consensus1_literal(const dfk_cons::Grids& s, std::vector<uint8_t>* con, HostResult* counters)
{
    con->assign((size_t)s.cols, 0);
    for (int i = 0; i < s.cols; i++) {
        std::pair<double, int> mVals[4];                                                           // BaseMetrics<double> mx
        for (int idx = 0; idx < 4; ++idx) { mVals[idx].first = 0.; mVals[idx].second = idx; }
        bool any = false;
        for (int j = 0; j < s.rows; j++) {
            double q = s.quals_[j][i];
            if (q <= 2) q = std::min(q, 0.2);
            if (q == 0) q = 0.1;
            if (s.quals_[j][i] >= 0) { mVals[(int)s.bases_[j][i]].first += q; ++counters->added; any = true; }
        }
        std::sort(mVals, mVals + 4, std::greater<std::pair<double, int>>());                       // mx.reverseSort()
        (*con)[i] = (uint8_t)mVals[0].second;
        counters->empty += !any;
    }
}

// the rows of stack ei of pair pi, as :585 leaves them
inline std::vector<dfk_cons::Triple> rows_of(const dfk_cons::Input& I, uint64_t k, uint64_t po)
{
    using namespace dfk_cons;
    std::vector<Triple> locs;
    for (uint64_t j = I.loc_first[k]; j < I.loc_first[k + 1]; ++j) locs.push_back(Triple{(int64_t)rec_id(I.locs, j), rec_pos(I.locs, j), rec_fw(I.locs, j)});
    for (uint64_t j = I.part_first[po]; j < I.part_first[po + 1]; ++j) locs.push_back(Triple{(int64_t)rec_id(I.parts, j), rec_pos(I.parts, j), rec_fw(I.parts, j)});
    return locs;
}

inline void push_closure(HostResult* R, uint64_t pi, int32_t off, uint32_t rows, const std::vector<uint8_t>& con, uint32_t K)
{
    R->recs.push_back(Rec{(uint32_t)pi, off, (uint32_t)con.size(), rows});
    R->bases.insert(R->bases.end(), con.begin(), con.end()); R->starts.push_back(R->bases.size());
    R->columns += con.size(); R->shorter += con.size() < K; R->rowless += rows == 0;
}

// -1, -2: stacks_of's; -3: a PQVec stream of the wrong length; -4: an offset outside [-cols2, cols1] of its pair, or off_first falls.
// The literal form: both stacks of a closable pair materialised, Merge and Consensus1 as written.
inline int closures_literal(const dfk_cons::Input& I, const int32_t* pairs, uint64_t n_pairs, const uint64_t* off_first, const int32_t* offsets, HostResult* R)
{
    using namespace dfk_cons;
    std::vector<uint32_t> side_rank; std::vector<uint8_t> reversed;
    if (int rc = stacks_of(I, pairs, n_pairs, &side_rank, &reversed)) return rc;
    for (uint64_t pi = 0; pi < n_pairs; ++pi) if (off_first[pi + 1] < off_first[pi]) return -4;
    R->pair_first.assign(1, 0); R->starts.assign(1, 0);
    for (uint64_t pi = 0; pi < n_pairs; ++pi) {
        const uint64_t no = off_first[pi + 1] - off_first[pi];
        R->over += no > 2;
        if (no >= 1 && no <= 2) {                                                                  // :651 (with none the loop runs no time)
            ++R->closable;
            const uint64_t es[2] = {(uint64_t)pairs[2 * pi], (uint64_t)I.inv[pairs[2 * pi + 1]]};
            Grids stacks[2]; Dim d[2];
            dfk_cons::HostResult unused;
            for (int ei = 0; ei < 2; ++ei)
                if (int rc = stack_grids(I, pairs[2 * pi + 1], es[ei], rows_of(I, side_rank[2 * pi + ei], 2 * pi + (1 - ei)), &d[ei], &stacks[ei], &unused)) return rc;
            for (uint64_t j = 0; j < no; ++j) {                                                    // :652
                const int32_t off = offsets[off_first[pi] + j];
                if (!offset_ok(stacks[0].cols, stacks[1].cols, off)) return -4;
                Grids s(stacks[0]);                                                                // :653
                merge_literal(&s, stacks[1], off);                                                 // :654
                std::vector<uint8_t> f;
                if (s.rows) consensus1_literal(s, &f, R);                                          // :657
                else { f.assign((size_t)s.cols, 3); R->empty += (uint64_t)s.cols; }                // the rowless rule
                push_closure(R, pi, off, (uint32_t)s.rows, f, I.K);                                // :660
            }
        }
        R->pair_first.push_back(R->recs.size());
    }
    return 0;
}

// ---- the plan
// A batch of closures: a closure costs its fixed words and its columns, and its pair's two stacks what dfk_cons.h says a stack costs
// (counted per closure though two closures of a pair share them).
constexpr uint64_t BYTES_PER_CLOSURE = 64 + (uint64_t)MAX_COLS;
inline unsigned closures_grid(uint64_t n_closures, unsigned cus) { return (unsigned)std::max<uint64_t>(1, std::min<uint64_t>(n_closures * TILES, 32ull * cus)); }   // a workgroup a tile

// the closable pairs and their closures: cp[i] the pair, cl_first[i] its first closure in `cl_off`
struct Closable { std::vector<uint64_t> cp, cl_first; std::vector<int32_t> cl_off; uint64_t over = 0; };
inline Closable closable_of(uint64_t n_pairs, const uint64_t* off_first, const int32_t* offsets)
{
    Closable C;
    C.cl_first.push_back(0);
    for (uint64_t pi = 0; pi < n_pairs; ++pi) {
        const uint64_t no = off_first[pi + 1] - off_first[pi];
        C.over += no > 2;
        if (no < 1 || no > 2) continue;
        C.cp.push_back(pi);
        for (uint64_t j = 0; j < no; ++j) C.cl_off.push_back(offsets[off_first[pi] + j]);
        C.cl_first.push_back(C.cl_off.size());
    }
    return C;
}

// The device version's order of work on the host, for the CPU test.  closures_per_batch 0 = what fits `room`
inline int closures_plan(const dfk_cons::Input& I, const int32_t* pairs, uint64_t n_pairs, const uint64_t* off_first, const int32_t* offsets, uint64_t closures_per_batch, uint64_t room,
                         uint64_t rows_cap, HostResult* R)
{
    using namespace dfk_cons;
    std::vector<uint32_t> side_rank; std::vector<uint8_t> reversed;
    if (int rc = stacks_of(I, pairs, n_pairs, &side_rank, &reversed)) return rc;
    for (uint64_t pi = 0; pi < n_pairs; ++pi) if (off_first[pi + 1] < off_first[pi]) return -4;
    const Closable C = closable_of(n_pairs, off_first, offsets);
    const uint64_t n_cp = C.cp.size(), n_stacks = 2 * n_cp, n = C.cl_off.size();
    R->closable = n_cp; R->over = C.over;
    // the stacks of the closable pairs alone: stack 2 i + ei is side ei of pair cp[i]
    auto q_of = [&](uint64_t s) { return 2 * C.cp[s / 2] + (s & 1); };
    std::vector<uint64_t> n_rows(n_stacks), prows(n_cp);
    for (uint64_t s = 0; s < n_stacks; ++s) { const uint64_t q = q_of(s); n_rows[s] = (I.loc_first[side_rank[q] + 1] - I.loc_first[side_rank[q]]) + (I.part_first[(q ^ 1) + 1] - I.part_first[q ^ 1]); }
    for (uint64_t i = 0; i < n_cp; ++i) prows[i] = n_rows[2 * i] + n_rows[2 * i + 1];
    const std::vector<uint64_t> rfirst = dfk::prefix_sums(n_rows.data(), n_stacks), pfirst = dfk::prefix_sums(prows.data(), n_cp);
    std::vector<std::vector<uint8_t>> con(n);
    std::vector<uint32_t> rows_of_closure(n, 0);
    for (uint64_t p0 = 0; p0 < n_cp;) {
        const uint64_t p1 = next_range(pfirst.data(), n_cp, p0, rows_cap).e1, q0 = 2 * p0, ns = 2 * (p1 - p0), n_items = rfirst[2 * p1] - rfirst[q0];
        ++R->ranges;
        // dimensions and live rows: dfk_cons.h's, on the stacks of the range
        std::vector<int64_t> M(ns, 0), w0(ns);
        std::vector<int32_t> ne(ns);
        auto row = [&](uint64_t s, uint64_t r) { const uint64_t q = q_of(q0 + s); return row_of(I, side_rank[q], q ^ 1, r); };
        for (uint64_t s = 0; s < ns; ++s) {
            ne[s] = bases_of_edge(I, I.ce[side_rank[q_of(q0 + s)]]);
            for (uint64_t r = 0; r < n_rows[q0 + s]; ++r) { const RowView v = row(s, r); M[s] = std::max(M[s], row_end(rec_fw(v.recs, v.at), rec_pos(v.recs, v.at), I.read_len[rec_id(v.recs, v.at)], ne[s])); }
            w0[s] = window_start(M[s]);
        }
        std::vector<uint64_t> lfirst(ns + 1, 0);
        std::vector<uint32_t> l_id, l_len; std::vector<int32_t> l_pos; std::vector<uint8_t> l_fw;
        for (uint64_t s = 0; s < ns; ++s) {
            for (uint64_t r = 0; r < n_rows[q0 + s]; ++r) {
                const RowView v = row(s, r);
                const uint32_t id = (uint32_t)rec_id(v.recs, v.at);
                if (!row_live(rec_fw(v.recs, v.at), rec_pos(v.recs, v.at), I.read_len[id], ne[s], w0[s])) continue;
                l_id.push_back(id); l_pos.push_back(rec_pos(v.recs, v.at)); l_fw.push_back(rec_fw(v.recs, v.at)); l_len.push_back(I.read_len[id]);
            }
            lfirst[s + 1] = l_id.size();
        }
        (void)n_items;
        std::vector<uint8_t> defined(l_id.size(), 0);
        // the closures of the range, their offsets checked against the dimensions, their cost
        const uint64_t k0 = C.cl_first[p0], k1 = C.cl_first[p1];
        std::vector<uint64_t> pair_of(k1 - k0), cost(k1 - k0);
        for (uint64_t i = p0; i < p1; ++i)
            for (uint64_t k = C.cl_first[i]; k < C.cl_first[i + 1]; ++k) {
                const uint64_t s0 = 2 * (i - p0);
                if (!offset_ok(M[s0] - w0[s0], M[s0 + 1] - w0[s0 + 1], C.cl_off[k])) return -4;
                pair_of[k - k0] = i - p0;
                cost[k - k0] = BYTES_PER_CLOSURE + 2 * BYTES_PER_STACK;
                for (uint64_t l = lfirst[s0]; l < lfirst[s0 + 2]; ++l) cost[k - k0] += live_row_cost(l_len[l]);
            }
        const std::vector<uint64_t> cfirst = dfk::prefix_sums(cost.data(), k1 - k0);
        for (uint64_t b0 = 0; b0 < k1 - k0;) {
            const uint64_t b1 = next_batch(cfirst.data(), k1 - k0, b0, room, closures_per_batch);
            ++R->batches;
            // the reads of the batch's pairs, each once, ascending; the gather; the decode
            const uint64_t sa = 2 * pair_of[b0], sb = 2 * pair_of[b1 - 1] + 2;
            std::vector<uint32_t> ids(l_id.begin() + lfirst[sa], l_id.begin() + lfirst[sb]);
            std::sort(ids.begin(), ids.end()); ids.erase(std::unique(ids.begin(), ids.end()), ids.end());
            std::vector<uint64_t> b_at(ids.size() + 1, 0), q_at(ids.size() + 1, 0);
            for (size_t i = 0; i < ids.size(); ++i) { const uint32_t len = I.read_len[ids[i]]; b_at[i + 1] = b_at[i] + (len + 3) / 4; q_at[i + 1] = q_at[i] + len; }
            std::vector<uint8_t> bases(b_at.back()), quals(q_at.back());
            for (size_t i = 0; i < ids.size(); ++i) {
                std::copy(I.read_packed + I.read_off[ids[i]], I.read_packed + I.read_off[ids[i]] + (b_at[i + 1] - b_at[i]), bases.begin() + b_at[i]);
                if (!decode_quals(I.pq, I.pq_off[ids[i]], I.pq_off[ids[i] + 1], quals.data() + q_at[i], I.read_len[ids[i]])) return -3;
            }
            // the consensus: a lane a merged column, stack 0's live rows then stack 1's
            for (uint64_t k = b0; k < b1; ++k) {
                const uint64_t s0 = 2 * pair_of[k];
                const int64_t off = C.cl_off[k0 + k], cols[2] = {M[s0] - w0[s0], M[s0 + 1] - w0[s0 + 1]}, Cm = merged_cols(cols[0], cols[1], off);
                con[k0 + k].assign((size_t)Cm, 0);
                R->live += lfirst[s0 + 2] - lfirst[s0];
                for (int64_t c = 0; c < Cm; ++c) {
                    double sum[4] = {0., 0., 0., 0.};
                    bool any = false;
                    for (int side = 0; side < 2; ++side) {
                        const uint64_t s = s0 + side;
                        const int64_t x = column_of_side(side, cols[side], off, c);
                        if (x < 0) continue;
                        const bool rev = reversed[q_of(q0 + s)] != 0;
                        const int64_t sc = stack_column(w0[s], cols[side], rev, x);
                        for (uint64_t l = lfirst[s]; l < lfirst[s + 1]; ++l) {
                            const uint64_t slot = slot_of(ids.data(), ids.size(), l_id[l]);
                            if (add_row(sum, l_fw[l] != 0, l_pos[l], l_len[l], ne[s], rev, sc, bases.data() + b_at[slot], quals.data() + q_at[slot])) { defined[l] = 1; ++R->added; any = true; }
                        }
                    }
                    con[k0 + k][(size_t)c] = (uint8_t)last_max(sum);
                    R->empty += !any;
                }
            }
            b0 = b1;
        }
        // rows_kept of the range's stacks, and with them the closures' rows
        for (uint64_t i = p0; i < p1; ++i) {
            uint32_t rows = 0;
            for (uint64_t s = 2 * (i - p0); s < 2 * (i - p0) + 2; ++s) {
                uint64_t kept = 0;
                for (uint64_t l = lfirst[s]; l < lfirst[s + 1]; ++l) kept += defined[l];
                rows += (uint32_t)(M[s] > MAX_WIDTH ? kept : n_rows[q0 + s]);
            }
            for (uint64_t k = C.cl_first[i]; k < C.cl_first[i + 1]; ++k) rows_of_closure[k] = rows;
        }
        p0 = p1;
    }
    R->pair_first.assign(n_pairs + 1, 0); R->starts.assign(1, 0);
    for (uint64_t i = 0; i < n_cp; ++i) {
        for (uint64_t k = C.cl_first[i]; k < C.cl_first[i + 1]; ++k) push_closure(R, C.cp[i], C.cl_off[k], rows_of_closure[k], con[k], I.K);
        R->pair_first[C.cp[i] + 1] = C.cl_first[i + 1] - C.cl_first[i];
    }
    for (uint64_t pi = 0; pi < n_pairs; ++pi) R->pair_first[pi + 1] += R->pair_first[pi];
    return 0;
}

// ---- the file's fixed parts
constexpr const char* MAGIC = "DFKCCLS1";
inline uint64_t pair_first_at() { return 24; }
inline uint64_t starts_at(uint64_t n_pairs) { return 24 + 8 * (n_pairs + 1); }
inline uint64_t recs_at(uint64_t n, uint64_t n_pairs) { return starts_at(n_pairs) + 8 * (n + 1); }
inline uint64_t bases_at(uint64_t n, uint64_t n_pairs) { return recs_at(n, n_pairs) + 16 * n; }
inline uint64_t file_size(uint64_t n, uint64_t n_pairs, uint64_t n_bases) { return bases_at(n, n_pairs) + dfk_cons::padded(n_bases); }

} // namespace dfk_closures
