// superplus_amd/csrc/dfk_sclosures.h -- Stackster's closures per pair (10X/Stackster.cc:712-757; paths/long/ReadStack.cc:714-725 Trim,
// :355-398 Merge, :406-427 Consensus1 with qualities, :26-45 BaseMetrics): for a pair with one to three kept offsets the two stacks
// trimmed to the edges, merged at each offset and the consensus of the merged stack -- the basevector Stackster pushes onto `closures`,
// the only thing it returns.  No stack is stored: the rule over plain arrays, the merged width, the two column maps and the tile's span
// stated once, the form the device runs and its plan, the layout of a.stack.closures.
//
// No HIP call and no device pointer is dereferenced here by the host, so tests/cpp/test_sclosures.cc compiles this header with a plain
// host compiler (and once more under -fsanitize=address,undefined) and checks it against cases recorded from
// tests/sclosures_oracle.py.  It is the SECOND restatement of the rule -- written from the reference's text, not from the Python.
//
// The rule (pair pi, ALT = False, EXP = False, idsfw2 empty; stacks[0], stacks[1]: the two stacks as dfk_scons.h defines them after Trim to
// 400 and Reverse -- rows the placed entries in entry order, lowered and oriented, a cell defined iff its lowered quality is below 128;
// n1, n2 their columns; offsets: the state-0 records of the pair in a.stack.offsets, ascending as Sort( offsets ) of :644 left them):
//   which pairs (:715)   offsets.isize( ) <= MAX_OFFSETS = 3: a pair with 1 to 3 kept offsets gets one closure per kept offset, in that
//                        order; with none the loop runs no time, with more than 3 nothing is merged.  A pair that does not yield never
//                        reaches :461 and has no offsets.  A record of state 1 (dropped at :642) is not in `offsets`.  The closures of
//                        all pairs follow in pair order (Stackster's share of `closures`, RunStages.cc:290-324).
//   the edges (:722-728) on copies s1( stacks[0] ), s2( stacks[1] ): o = offset; right_ext = s1.Cols( ) - offset - s2.Cols( ), from the
//                        untrimmed widths; if right_ext > 0: s1.Trim( 0, s1.Cols( ) - right_ext ), i.e. to the columns [0, offset + n2).
//                        left_ext = -offset; if left_ext > 0: s2.Trim( left_ext, s2.Cols( ) ) and o = 0.
//   Trim (ReadStack.cc:714-725)  to_remove[i] = no Def( i, j ) for j in [start, stop); every row cut to [start, stop); cols_ = stop - start;
//                        Erase( to_remove ): the rows without a defined cell in the kept columns go, the order of the others stays.
//   Merge (:732-733)     readstack s( s1 ); s.Merge( s2, o ) -- ReadStack.cc:355-398, dfk_closures.h's merge_literal.  Written out for
//                        both signs: offset >= 0: s1 is min( n1, offset + n2 ) wide, s2 is n2 wide and shifted by offset: the width is
//                        offset + n2.  offset < 0: s1 is min( n1, offset + n2 ) wide, s2 is n2 + offset wide and not shifted: offset + n2
//                        again.  So the merged width is always C = offset + n2 (merged_cols); merged column c holds stack 0's output
//                        column c where c < n1 and stack 1's output column c - offset where 0 <= c - offset (column_of_side;
//                        tests/cpp/test_sclosures.cc holds both to the literal Trim and Merge for every allowed offset).  A kept offset
//                        is j - l with an 8-mer at j of one stack's consensus and at l of a row of the other, both inside their stacks:
//                        offset lies in [-(n2 - 8), n1 - 8] (offset_ok), 8 <= C <= 792, and the stacks share 8 columns at least.
//   Consensus1 (:753)    default qualcap; per merged column four doubles from 0 (BaseMetrics); the surviving rows of stack 0 in their
//                        order, then those of stack 1; a cell with Qual >= 0 adds 0.1 for Q0, 0.2 for Q1 and Q2, q otherwise (:415-418:
//                        dfk_cons::quality_value) on the LOWERED quality.  mx.reverseSort( ) and con = mx.id(0): the base of the greatest
//                        ( sum, id ) pair (dfk_closures::last_max): ties go to the highest base, a column nothing was added to gives
//                        base 3.  fragq (conq) is thrown away (:757 pushes f alone) and is not built.
//   The sums cross the stack boundary in row order: 20 from stack 0 then 0.1, 0.1 from stack 1 is 20.200000000000003; 0.2 then 10, 10 is
//   20.2: base 0 wins where per-stack sums added would tie and base 1 would win.  No per-stack sums, no tree, no reassociation, no FMA.
//   An erased row has no defined cell in the window, so it adds nothing: the walk may run over all live rows.
//   rows                 a closure's rows = the rows the merged stack has: per stack, where its edge trim applies (right_ext > 0 for
//                        stack 0, left_ext > 0 for stack 1) the rows with a defined cell in the merged window, else all the rows the
//                        stack kept after its own Trim to 400.  A live row whose span meets the window only in cells of quality 128 or
//                        more is erased.
//   The one undefined place: every row of both stacks erased -- the reference reads bases_[0] of an empty vector (ReadStack.cc:398).
//   Decided here as dfk_closures.h decided: the closure has C columns of base 3 (what the walk over no rows gives), and `rowless`
//   counts such closures.  It cannot happen for an offset a.stack.offsets really holds: an offset was proposed by a row r of one stack
//   whose 8 cells at l are all defined and equal the 8-mer at j of the other stack's consensus (Stackster.cc:521-543).  With s = 0 the
//   row stands in stack 1, offset = j - l, and its cells show in the merged columns [j, j + 8): j >= 0 >= offset keeps them at or behind
//   stack 1's left edge -offset, and j + 8 = offset + l + 8 <= offset + n2 = C.  With s = 1 the row stands in stack 0, offset = l - j,
//   its cells are the merged columns [l, l + 8) and l + 8 = offset + j + 8 <= offset + n2 = C: inside [0, C), which stack 0's trim keeps.
//   Either way the row survives its stack's trim, so the merged stack has a row.  Only hand-given offsets (dfk_sclosures_build_arrays)
//   reach the rowless rule.
//
// The form the device runs (dfk_sclosures_kernels.h, dfk_sclosures.inc; sclosures_plan() below is its order of work on the host):
//   closable   the pairs with one to three kept offsets, in pair order; ONLY their stacks are touched.  Ranges hold whole closable pairs,
//              as many as keep the rows of their stacks at the cap (dfk_scons.h's row_cap); the live rows of a stack are dfk_scons.h's.
//   batches    as many closures of the range as fit the room (or closures_per_batch); the reads the live rows of their pairs' stacks
//              name gathered once each, decoded and lowered.  Two closures of one pair may fall into two batches.
//   consensus  a workgroup a TILE of 256 merged columns of a closure (4 tiles: 792 columns at most), a lane a column: the live rows of
//              stack 0, then those of stack 1, walked once in order, their headers staged through LDS 256 at a time; a lane whose
//              column the row covers adds one double.  A row whose span misses the stack columns the tile shows (tile_span, row_meets)
//              is skipped by the whole workgroup: it would add nothing.  last_max is written at the closure's place.  No atomics.
//   rows       a flag per ( closure, live row of its pair ): 1 where the row had a defined cell in some merged column (every writer
//              writes 1); a second kernel counts the flags per closure and side.  Where neither the edge trim nor the Trim to 400
//              applies to a stack every row it has stays.
//
// The file (dfk_sclosures_write).  Numbers are little-endian, no byte undefined.  a.close.closures' layout under another magic:
//   a.stack.closures   "DFKSCLS1" | u64 n closures | u64 n_pairs | (n_pairs + 1) x u64 first closure of each pair | (n + 1) x u64
//                      starts, in bases | n x 16-byte { u32 pair, i32 offset, u32 cols, u32 rows } | the bases, a byte each (0..3) |
//                      zero bytes to a multiple of 8.
#pragma once
#include <stdint.h>
#include "dfk_scons.h"
#include "dfk_soffsets.h"

namespace dfk_sclosures {

constexpr uint64_t SALT = 0x5C15ull;               // k_digest_seq's, over the records as u32 words, then the bases one value each
constexpr uint32_t GROUP = 256;                    // lanes of a workgroup: a tile of merged columns
constexpr int64_t MAX_WIDTH = dfk_scons::MAX_WIDTH;
constexpr int64_t MM = dfk_soffsets::MM;           // the 8-mer both stacks share at a kept offset
constexpr int64_t MAX_COLS = 2 * MAX_WIDTH - MM;   // 792: two stacks of 400 at offset 392
constexpr uint32_t TILES = (uint32_t)((MAX_COLS + GROUP - 1) / GROUP);        // 4
constexpr uint32_t MAX_OFFSETS = dfk_soffsets::MAX_OFFSETS;                   // :714

DFK_CN_HD bool offset_ok(int64_t n1, int64_t n2, int64_t off) { return off >= -(n2 - MM) && off <= n1 - MM; }
// the merged width, whatever the sign of the offset and whichever trims apply
DFK_CN_HD int64_t merged_cols(int64_t n2, int64_t off) { return off + n2; }
// does the edge trim of :722-728 apply to the stack?  (right_ext from the untrimmed widths)
DFK_CN_HD bool edge_trimmed(int side, int64_t n1, int64_t n2, int64_t off) { return side == 0 ? n1 - off - n2 > 0 : -off > 0; }
// the output column (after Trim to 400 and Reverse, before the edge trim) of stack `side` that merged column c in [0, C) holds, or -1
DFK_CN_HD int64_t column_of_side(int side, int64_t n1, int64_t n2, int64_t off, int64_t c)
{
    if (side == 0) return c < n1 ? c : -1;
    const int64_t x = c - off;
    return x >= 0 && x < n2 ? x : -1;
}
// the stack columns [*lo, *hi] (before Trim and Reverse: where a row's start counts) that the merged columns [c0, c1) show of a side;
// false: they show none of it.  c1 <= C.
DFK_CN_HD bool tile_span(int side, int64_t n1, int64_t n2, int64_t off, int64_t w0, bool reversed, int64_t c0, int64_t c1, int64_t* lo, int64_t* hi)
{
    const int64_t cols = side == 0 ? n1 : n2;
    int64_t x0 = side == 0 ? c0 : c0 - off, x1 = side == 0 ? c1 : c1 - off;                          // output columns [x0, x1)
    if (x0 < 0) x0 = 0;
    if (x1 > cols) x1 = cols;
    if (x1 <= x0) return false;
    const int64_t a = dfk_scons::stack_column(w0, cols, reversed, x0), b = dfk_scons::stack_column(w0, cols, reversed, x1 - 1);
    *lo = a < b ? a : b; *hi = a < b ? b : a;
    return true;
}
// does the row's span [start, start + len) meet the stack columns [lo, hi]?  A row that does not adds nothing to the tile.
DFK_CN_HD bool row_meets(int32_t start, uint32_t len, int64_t lo, int64_t hi) { return (int64_t)start <= hi && (int64_t)start + (int64_t)len > lo; }
// one row's cell in a column added to the column's sums; true if the cell is defined.  packed and quals: the read as stored, quals lowered
DFK_CN_HD bool add_row(double* sum, int32_t start, uint32_t len, bool rc, bool reversed, int64_t sc, const uint8_t* packed, const uint8_t* quals)
{
    const int64_t j = dfk_scons::cell_index(start, len, sc);
    if (j < 0) return false;
    const uint8_t q = dfk_walks::oriented_qual(quals, len, rc, (uint32_t)j);
    if (!dfk_cons::cell_defined(q)) return false;
    const uint32_t b = dfk_walks::oriented_base(packed, len, rc, (uint32_t)j);
    dfk_cons::add_cell(sum, reversed ? 3u - b : b, q);
    return true;
}

} // namespace dfk_sclosures

// ---------------------------------------------------------------------------------------------------------------- host only
namespace dfk_sclosures {

typedef dfk_closures::Rec Rec;                     // { u32 pair, i32 offset, u32 cols, u32 rows }

// everything as plain arrays: the walks in dfk_walks_fetch's forms and the reads, dims in dfk_scons_fetch's form, the offsets in
// dfk_soffsets_fetch's forms
struct Input {
    dfk_scons::Input W;
    const dfk_scons::Dim* dims /* [2 * n_pairs] */;
    const uint64_t* so_starts /* [n_pairs + 1] */; const dfk_soffsets::PairWords* words /* [n_pairs] */; const dfk_soffsets::Rec* recs;
};

struct HostResult {
    std::vector<uint64_t> pair_first;              // [n_pairs + 1]
    std::vector<uint64_t> starts;                  // [n + 1]
    std::vector<Rec> recs;
    std::vector<uint8_t> bases;
    uint64_t yields = 0, closable = 0, none = 0, over = 0, columns = 0, added = 0, live = 0, erased = 0, empty = 0, shorter = 0, rowless = 0, decoded = 0, batches = 0, ranges = 0,
             visits = 0, skipped = 0;
};

// what the tables must hold beside dfk_scons.h's check_walks.  0 fine; -5 the dims of a yielding pair do not say what its walks do (rows,
// cols, rows_kept above rows or below them without a Trim); -6 the offsets' starts do not begin at 0 or fall; -7 a state other than 0 or
// 1; -8 the offsets of a pair do not ascend; -9 a kept offset outside [-(n2 - 8), n1 - 8]; -10 records for a pair that does not yield;
// -11 words whose kept / closable do not say what the records do.  *where: the pair.  yields( pi ), M_of( q ), placed_of( q ): the walks'.
template <class Y, class MF, class PF>
inline int check_tables(uint64_t n_pairs, Y yields, MF M_of, PF placed_of, const dfk_scons::Dim* dims, const uint64_t* so_starts, const dfk_soffsets::PairWords* words, const dfk_soffsets::Rec* recs, uint64_t* where)
{
    uint64_t none = 0;
    if (!where) where = &none;
    *where = 0;
    if (so_starts[0] != 0) return -6;
    for (uint64_t pi = 0; pi < n_pairs; ++pi) if (so_starts[pi + 1] < so_starts[pi]) { *where = pi; return -6; }
    for (uint64_t pi = 0; pi < n_pairs; ++pi) {
        *where = pi;
        const bool y = yields(pi);
        if (y)
            for (uint64_t q = 2 * pi; q < 2 * pi + 2; ++q) {
                const int64_t M = M_of(q);
                if ((int64_t)dims[q].cols != M - dfk_scons::window_start(M) || dims[q].M != (int32_t)M || dims[q].rows != placed_of(q) || dims[q].rows_kept > dims[q].rows || (M <= MAX_WIDTH && dims[q].rows_kept != dims[q].rows)) return -5;
            }
        if (!y && so_starts[pi + 1] != so_starts[pi]) return -10;
        uint32_t kept = 0;
        for (uint64_t j = so_starts[pi]; j < so_starts[pi + 1]; ++j) {
            if (recs[j].state != dfk_soffsets::KEPT && recs[j].state != dfk_soffsets::DROPPED) return -7;
            if (j > so_starts[pi] && recs[j].offset <= recs[j - 1].offset) return -8;
            if (recs[j].state == dfk_soffsets::KEPT) {
                ++kept;
                if (!offset_ok(dims[2 * pi].cols, dims[2 * pi + 1].cols, recs[j].offset)) return -9;
            }
        }
        if (words[pi].kept != kept || words[pi].closable != (dfk_soffsets::closable(kept) ? 1u : 0u)) return -11;
    }
    return 0;
}
inline int check_tables(const Input& I, uint64_t* where = nullptr)
{
    return check_tables(I.W.n_pairs, [&](uint64_t pi) { return dfk_scons::yields(I.W.recs, pi); }, [&](uint64_t q) { return (int64_t)I.W.recs[q].M; },
                        [&](uint64_t q) { return I.W.recs[q].placed; }, I.dims, I.so_starts, I.words, I.recs, where);
}

// the closable pairs and their closures: cp[i] the pair, cl_first[i] its first closure in `cl_off`; none, over: pairs with no kept offset
// and with more than three
struct Closable { std::vector<uint64_t> cp, cl_first; std::vector<int32_t> cl_off; uint64_t none = 0, over = 0; };
inline Closable closable_of(uint64_t n_pairs, const uint64_t* so_starts, const dfk_soffsets::Rec* recs)
{
    Closable C;
    C.cl_first.push_back(0);
    for (uint64_t pi = 0; pi < n_pairs; ++pi) {
        uint32_t kept = 0;
        for (uint64_t j = so_starts[pi]; j < so_starts[pi + 1]; ++j) kept += recs[j].state == dfk_soffsets::KEPT;
        C.none += kept == 0; C.over += kept > MAX_OFFSETS;
        if (!dfk_soffsets::closable(kept)) continue;                                                // :715
        C.cp.push_back(pi);
        for (uint64_t j = so_starts[pi]; j < so_starts[pi + 1]; ++j) if (recs[j].state == dfk_soffsets::KEPT) C.cl_off.push_back(recs[j].offset);
        C.cl_first.push_back(C.cl_off.size());
    }
    return C;
}

// readstack::Trim( start, stop ) as written (ReadStack.cc:714-725), on the grids
inline void trim_literal(dfk_cons::Grids* g, const int start, const int stop)
{
    std::vector<bool> to_remove((size_t)g->rows, true);
    for (int i = 0; i < g->rows; i++) {
        for (int j = start; j < stop; j++) {
            if (g->quals_[i][j] >= 0) {                                                             // Def(i,j)
                to_remove[i] = false;
                break;
            }
        }
        g->bases_[i] = std::vector<int8_t>(g->bases_[i].begin() + start, g->bases_[i].begin() + stop);   // SetToSubOf( bases_[i], start, stop - start )
        g->quals_[i] = std::vector<int8_t>(g->quals_[i].begin() + start, g->quals_[i].begin() + stop);
    }
    g->cols = stop - start;
    std::vector<std::vector<int8_t>> b2, q2;                                                        // Erase( to_remove )
    for (int i = 0; i < g->rows; i++) if (!to_remove[i]) { b2.push_back(g->bases_[i]); q2.push_back(g->quals_[i]); }
    g->bases_.swap(b2); g->quals_.swap(q2);
    g->rows = (int)g->bases_.size();
}

// :717-733 for one offset: the copies, the two trims, the merge -> the merged stack
inline dfk_cons::Grids merged_literal(const dfk_cons::Grids* stacks, const int offset)
{
    dfk_cons::Grids s1(stacks[0]), s2(stacks[1]);                                                   // :717
    int o = offset;                                                                                 // :722
    int right_ext = s1.cols - offset - s2.cols;
    if (right_ext > 0) trim_literal(&s1, 0, s1.cols - right_ext);
    int left_ext = -offset;
    if (left_ext > 0) {
        trim_literal(&s2, left_ext, s2.cols);
        o = 0;
    }
    dfk_cons::Grids s(s1);                                                                          // :732
    dfk_closures::merge_literal(&s, s2, o);                                                         // :733 (without rows its width is merged_cols: the rule above)
    return s;
}

inline void push_closure(HostResult* R, uint64_t pi, int32_t off, uint32_t rows, const std::vector<uint8_t>& con, uint32_t K)
{
    R->recs.push_back(Rec{(uint32_t)pi, off, (uint32_t)con.size(), rows});
    R->bases.insert(R->bases.end(), con.begin(), con.end()); R->starts.push_back(R->bases.size());
    R->columns += con.size(); R->shorter += con.size() < K; R->rowless += rows == 0;
}

// -1, -2, -4: dfk_scons.h's check_walks; -3: a PQVec stream of the wrong length; -5 ... -11: check_tables'.
// The literal form: both stacks of a closable pair materialised, Trim, Merge and Consensus1 as written.
inline int sclosures_literal(const Input& I, uint32_t K, HostResult* R)
{
    if (int rc = dfk_scons::check_walks(I.W)) return rc;
    if (int rc = check_tables(I)) return rc;
    R->pair_first.assign(1, 0); R->starts.assign(1, 0);
    for (uint64_t pi = 0; pi < I.W.n_pairs; ++pi) {
        R->yields += dfk_scons::yields(I.W.recs, pi);
        std::vector<int> offsets;                                                                   // :636-644: what the filter kept, sorted
        for (uint64_t j = I.so_starts[pi]; j < I.so_starts[pi + 1]; ++j) if (I.recs[j].state == dfk_soffsets::KEPT) offsets.push_back(I.recs[j].offset);
        R->none += offsets.empty(); R->over += offsets.size() > MAX_OFFSETS;
        if (!offsets.empty() && offsets.size() <= MAX_OFFSETS) {                                    // :715 (with none the loop runs no time)
            ++R->closable;
            dfk_cons::Grids stacks[2]; dfk_scons::Dim d[2];
            dfk_scons::HostResult unused;
            uint64_t live = 0;
            for (uint32_t s = 0; s < 2; ++s) {
                if (int rc = dfk_scons::stack_grids(I.W, 2 * pi + s, s, &d[s], &stacks[s], &unused)) return rc;
                for (uint64_t j = I.W.starts[2 * pi + s]; j < I.W.starts[2 * pi + s + 1]; ++j) live += dfk_scons::span_meets(I.W.locs[j].start, I.W.read_len[I.W.locs[j].id], dfk_scons::window_start(d[s].M));
            }
            for (size_t j = 0; j < offsets.size(); j++) {                                           // :716
                const dfk_cons::Grids s = merged_literal(stacks, offsets[j]);
                std::vector<uint8_t> f;
                dfk_closures::HostResult cnt;
                if (s.rows) dfk_closures::consensus1_literal(s, &f, &cnt);                          // :753
                else { f.assign((size_t)s.cols, 3); cnt.empty = (uint64_t)s.cols; }                 // the rowless rule
                R->added += cnt.added; R->empty += cnt.empty; R->live += live; R->erased += (uint64_t)(stacks[0].rows + stacks[1].rows - s.rows);
                push_closure(R, pi, offsets[j], (uint32_t)s.rows, f, K);                            // :757
            }
        }
        R->pair_first.push_back(R->recs.size());
    }
    return 0;
}

// ---- the plan
// A batch of closures: a closure costs its fixed words and its columns, a flag a live row of its pair, and its pair's two stacks what
// dfk_cons.h says a stack costs (counted per closure though the closures of a pair share them).
constexpr uint64_t BYTES_PER_CLOSURE = 96 + (uint64_t)MAX_COLS;
inline unsigned closures_grid(uint64_t n_closures, unsigned cus) { return (unsigned)std::max<uint64_t>(1, std::min<uint64_t>(n_closures * TILES, 32ull * cus)); }   // a workgroup a tile
inline unsigned rows_grid(uint64_t n_closures, unsigned cus) { return (unsigned)std::max<uint64_t>(1, std::min<uint64_t>(n_closures, 32ull * cus)); }             // a workgroup a closure

// The device version's order of work on the host, for the CPU test.  closures_per_batch 0 = what fits `room`; returns as sclosures_literal
inline int sclosures_plan(const Input& I, uint32_t K, uint64_t closures_per_batch, uint64_t room, uint64_t rows_cap, HostResult* R)
{
    using dfk_scons::window_start;
    if (int rc = dfk_scons::check_walks(I.W)) return rc;
    if (int rc = check_tables(I)) return rc;
    const uint64_t n_pairs = I.W.n_pairs;
    for (uint64_t pi = 0; pi < n_pairs; ++pi) R->yields += dfk_scons::yields(I.W.recs, pi);
    const Closable C = closable_of(n_pairs, I.so_starts, I.recs);
    const uint64_t n_cp = C.cp.size(), n = C.cl_off.size();
    R->closable = n_cp; R->none = C.none; R->over = C.over;
    auto q_of = [&](uint64_t s) { return 2 * C.cp[s / 2] + (s & 1); };                              // stack 2 i + side is side `side` of pair cp[i]
    std::vector<uint64_t> prows(n_cp);
    for (uint64_t i = 0; i < n_cp; ++i) prows[i] = I.W.starts[2 * C.cp[i] + 2] - I.W.starts[2 * C.cp[i]];
    const std::vector<uint64_t> pfirst = dfk::prefix_sums(prows.data(), n_cp);
    std::vector<std::vector<uint8_t>> con(n);
    std::vector<uint32_t> rows_of_closure(n, 0);
    for (uint64_t p0 = 0; p0 < n_cp;) {
        const uint64_t p1 = dfk::pidx_next_range(pfirst.data(), n_cp, p0, rows_cap).e1, ns = 2 * (p1 - p0);
        ++R->ranges;
        // the stacks of the range: M, the window, the live rows (host)
        std::vector<int64_t> M(ns, 0), w0(ns, 0);
        std::vector<uint64_t> n_rows(ns, 0), lfirst(ns + 1, 0);
        std::vector<uint32_t> l_id, l_len; std::vector<int32_t> l_start; std::vector<uint8_t> l_rc;
        for (uint64_t s = 0; s < ns; ++s) {
            const uint64_t q = q_of(2 * p0 + s);
            M[s] = I.W.recs[q].M; w0[s] = window_start(M[s]); n_rows[s] = I.W.starts[q + 1] - I.W.starts[q];
            for (uint64_t j = I.W.starts[q]; j < I.W.starts[q + 1]; ++j) {
                const dfk_walks::Loc& L = I.W.locs[j];
                if (!dfk_scons::span_meets(L.start, I.W.read_len[L.id], w0[s])) continue;
                l_id.push_back((uint32_t)L.id); l_start.push_back(L.start); l_len.push_back(I.W.read_len[L.id]); l_rc.push_back(dfk_scons::row_rc(L.fw != 0));
            }
            lfirst[s + 1] = l_id.size();
        }
        // the closures of the range and what each costs a batch
        const uint64_t k0 = C.cl_first[p0], nk = C.cl_first[p1] - k0;
        std::vector<uint64_t> pair_of(nk), cost(nk);
        for (uint64_t i = p0; i < p1; ++i)
            for (uint64_t k = C.cl_first[i]; k < C.cl_first[i + 1]; ++k) {
                const uint64_t s0 = 2 * (i - p0);
                pair_of[k - k0] = i - p0;
                cost[k - k0] = BYTES_PER_CLOSURE + 2 * dfk_cons::BYTES_PER_STACK + 4 * (lfirst[s0 + 2] - lfirst[s0]);
                for (uint64_t l = lfirst[s0]; l < lfirst[s0 + 2]; ++l) cost[k - k0] += dfk_cons::live_row_cost(l_len[l]);
            }
        const std::vector<uint64_t> cfirst = dfk::prefix_sums(cost.data(), nk);
        for (uint64_t b0 = 0; b0 < nk;) {
            const uint64_t b1 = dfk_cons::next_batch(cfirst.data(), nk, b0, room, closures_per_batch);
            ++R->batches;
            // the reads of the batch's pairs, each once, ascending; the gather; the decode and the lowering
            const uint64_t sa = 2 * pair_of[b0], sb = 2 * pair_of[b1 - 1] + 2;
            std::vector<uint32_t> ids(l_id.begin() + lfirst[sa], l_id.begin() + lfirst[sb]);
            std::sort(ids.begin(), ids.end()); ids.erase(std::unique(ids.begin(), ids.end()), ids.end());
            std::vector<uint64_t> b_at(ids.size() + 1, 0), q_at(ids.size() + 1, 0);
            for (size_t i = 0; i < ids.size(); ++i) { const uint32_t len = I.W.read_len[ids[i]]; b_at[i + 1] = b_at[i] + (len + 3) / 4; q_at[i + 1] = q_at[i] + len; }
            std::vector<uint8_t> bases(b_at.back()), quals(q_at.back());                            // (capacity == size: a read past the end is the sanitizer's to see)
            for (size_t i = 0; i < ids.size(); ++i) {
                std::copy(I.W.read_packed + I.W.read_off[ids[i]], I.W.read_packed + I.W.read_off[ids[i]] + (b_at[i + 1] - b_at[i]), bases.begin() + b_at[i]);
                if (!dfk_cons::decode_quals(I.W.pq, I.W.pq_off[ids[i]], I.W.pq_off[ids[i] + 1], quals.data() + q_at[i], I.W.read_len[ids[i]])) return -3;
                dfk_walks::lower_read(bases.data() + b_at[i], I.W.read_len[ids[i]], quals.data() + q_at[i]);
            }
            R->decoded += ids.size();
            // the consensus: a workgroup a tile, a lane a merged column; stack 0's live rows, then stack 1's
            for (uint64_t k = b0; k < b1; ++k) {
                const uint64_t s0 = 2 * pair_of[k];
                const int64_t off = C.cl_off[k0 + k], n1 = M[s0] - w0[s0], n2 = M[s0 + 1] - w0[s0 + 1], Cm = merged_cols(n2, off);
                con[k0 + k].assign((size_t)Cm, 0);
                std::vector<uint8_t> flag(lfirst[s0 + 2] - lfirst[s0], 0);
                R->live += flag.size();
                for (uint32_t tile = 0; tile < TILES && (int64_t)tile * GROUP < Cm; ++tile) {
                    const int64_t c0 = (int64_t)tile * GROUP, c1 = std::min<int64_t>(Cm, c0 + GROUP);
                    double sum[GROUP][4] = {};
                    bool any[GROUP] = {};
                    for (int side = 0; side < 2; ++side) {
                        const uint64_t s = s0 + side;
                        const bool rev = side == 1;
                        const int64_t cols = side ? n2 : n1;
                        int64_t lo = 0, hi = 0;
                        R->visits += lfirst[s + 1] - lfirst[s];
                        if (!tile_span(side, n1, n2, off, w0[s], rev, c0, c1, &lo, &hi)) { R->skipped += lfirst[s + 1] - lfirst[s]; continue; }
                        for (uint64_t l = lfirst[s]; l < lfirst[s + 1]; ++l) {
                            if (!row_meets(l_start[l], l_len[l], lo, hi)) { ++R->skipped; continue; }
                            const uint64_t slot = dfk_cons::slot_of(ids.data(), ids.size(), l_id[l]);
                            for (int64_t c = c0; c < c1; ++c) {
                                const int64_t x = column_of_side(side, n1, n2, off, c);
                                if (x < 0) continue;
                                if (add_row(sum[c - c0], l_start[l], l_len[l], l_rc[l] != 0, rev, dfk_scons::stack_column(w0[s], cols, rev, x), bases.data() + b_at[slot], quals.data() + q_at[slot])) {
                                    flag[l - lfirst[s0]] = 1; ++R->added; any[c - c0] = true;
                                }
                            }
                        }
                    }
                    for (int64_t c = c0; c < c1; ++c) { con[k0 + k][(size_t)c] = (uint8_t)dfk_closures::last_max(sum[c - c0]); R->empty += !any[c - c0]; }
                }
                // the rows: the flags counted per side
                uint32_t rows = 0;
                for (int side = 0; side < 2; ++side) {
                    const uint64_t s = s0 + side;
                    uint64_t kept = 0;
                    for (uint64_t l = lfirst[s]; l < lfirst[s + 1]; ++l) kept += flag[l - lfirst[s0]];
                    const bool cut = edge_trimmed(side, n1, n2, off);
                    const uint64_t had = I.dims[q_of(2 * p0 + s)].rows_kept;                       // (with a Trim to 400 only the cells can say how many rows it kept)
                    if (kept > had || (!cut && M[s] > MAX_WIDTH && kept != had)) return -5;
                    rows += (uint32_t)(cut || M[s] > MAX_WIDTH ? kept : n_rows[s]);
                }
                rows_of_closure[k0 + k] = rows;
                R->erased += (uint64_t)I.dims[q_of(2 * p0 + s0)].rows_kept + I.dims[q_of(2 * p0 + s0 + 1)].rows_kept - rows;
            }
            b0 = b1;
        }
        p0 = p1;
    }
    R->pair_first.assign(n_pairs + 1, 0); R->starts.assign(1, 0);
    for (uint64_t i = 0; i < n_cp; ++i) {
        for (uint64_t k = C.cl_first[i]; k < C.cl_first[i + 1]; ++k) push_closure(R, C.cp[i], C.cl_off[k], rows_of_closure[k], con[k], K);
        R->pair_first[C.cp[i] + 1] = C.cl_first[i + 1] - C.cl_first[i];
    }
    for (uint64_t pi = 0; pi < n_pairs; ++pi) R->pair_first[pi + 1] += R->pair_first[pi];
    return 0;
}

// ---- the file's fixed parts: a.close.closures' (dfk_closures.h) under this magic
constexpr const char* MAGIC = "DFKSCLS1";
using dfk_closures::pair_first_at;
using dfk_closures::starts_at;
using dfk_closures::recs_at;
using dfk_closures::bases_at;
using dfk_closures::file_size;

} // namespace dfk_sclosures
