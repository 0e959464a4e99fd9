// superplus_amd/csrc/dfk_scons.h -- Stackster's stack consensus per pair (10X/Stackster.cc:396-489 the two stacks, their Trim and Reverse,
// Consensus1( con, conq, QUALCAP ) of each and the MIN_FLAT zeroing of conq; :546-563 the conflicting columns of an offset; paths/long/
// ReadStack.cc:346-353 Reverse, :406-427 Consensus1 with qualities, :714-725 Trim, :26-45 BaseMetrics).  No stack is stored: the rule
// over plain arrays, the pieces host and kernels share stated once, the form the device runs and its plan, the layout of a.stack.cons.
//
// No HIP call and no device pointer is dereferenced here by the host, so tests/cpp/test_scons.cc compiles this header with a plain
// host compiler (and once more under -fsanitize=address,undefined) and checks it against cases recorded from tests/scons_oracle.py.
// It is the SECOND restatement of the rule -- written from the reference's text, not from the Python.
//
// The rule (a pair pi, ALT = False, EXP = False; the input is a.stack.walks: per pair and side the placed entries with the locs of :403,
// M and trim -- dfk_walks.h):
//   which pairs (:404-408)   only a pair where both sides placed an entry (status 0 and placed > 0 on both: what DFK_WALKS_YIELDS counts).
//                        Every other pair makes Stackster return before any consensus: its two elements have 0 rows, 0 columns, M 0
//                        and no conflict entries.
//   the stack (:398-431) rows: the placed entries of the side in entry order.  Row i has offset = start, len, and the read oriented and
//                        lowered as the walk saw it (dfk_walks::lower_read on the read as stored, then oriented_base / oriented_qual
//                        with rc = !fw of the loc: the loc's flag is fw ^ ( side == 1 ) and entry_rc is fw == ( side == 1 ), so
//                        both sides give rc = !loc.fw -- :425 SetRc2( i, !fw )).  Cell ( i, start + j ) is set for 0 <= start + j < M;
//                        start may be negative.  A read may stand twice, once with each flag: two rows.  The quality goes into a
//                        char (ReadStack.h:29): a lowered quality of 128 or more leaves the cell UNDEFINED (Def is Qual >= 0).
//   Trim (:435-440, ReadStack.cc:714-725)   only when M > 400: the columns [M - 400, M) are kept, the rows without a defined cell
//                        there erased, the order of the others kept.  Every cell inside a row's span is defined unless its quality is
//                        128 or more, so where no such quality stands rows_kept == the rows whose span [start, start + len) meets
//                        the window (span_meets; tests/cpp/test_scons.cc checks it on such cases).  The device counts the defined
//                        cells' rows themselves, so the rule holds with such qualities too.
//   Reverse (:446, ReadStack.cc:346-353)    side 1 only: the columns reversed, the bases that were set complemented; no row reordered.
//   Consensus1, qualcap = 100 (ReadStack.cc:406-427)   per column four doubles from 0 (BaseMetrics); the kept rows IN ROW ORDER, one IEEE
//                        add a defined cell: 0.1 for Q0, 0.2 for Q1 and Q2, q otherwise (dfk_cons::quality_value).  No per-tile sums, no
//                        tree, no reassociation, no FMA.  mx.reverseSort() is std::sort with std::greater< pair< double, int > >:
//                        con = id(0), the base of the greatest ( sum, id ) pair (dfk_closures::last_max; ties to the highest base, a
//                        column nothing covers gives base 3); val(1), id(1) belong to the second greatest pair (among equal sums the
//                        higher id).  conq = Min( 100, int( round( val(0) - val(1) ) ) ), round half away from zero.  If val(1) > 100:
//                        the kept rows with Qual >= 30 (the char: 30..127) that show base id(1) in the column are counted; two or more
//                        set conq = 0.
//   MIN_FLAT (:473-489)  on each side's final con (side 1: the reversed one): every maximal run of 10 or more equal bases gets conq = 0;
//                        runs of base 3 over uncovered columns count too.
//   conflicts (:546-563) n1, n2 the columns of the two stacks; for offset in [-n2, n1): the i1 with 0 <= i1 - offset < n2, conq1x[i1] ==
//                        100, conq2x[i1 - offset] == 100 and con1x[i1] != con2x[i1 - offset].  The reference evaluates it lazily for the
//                        offsets some 8-mer proposes and remembers the answer in allowed / disallowed; it is a function of the offset
//                        alone, so the whole table says the same.  The count is kept; below 10 the offset is allowed.
//   20 then 0.1, 0.1 is 20.200000000000003 and 0.2 then 10, 10 is 20.2 (dfk_closures.h): the order of the rows decides a column.
//
// The form the device runs (dfk_scons_kernels.h, dfk_scons.inc; scons_plan() below is its order of work on the host):
//   ranges     whole pairs, as many as keep the rows of their stacks at the cap (DFK_PIDX_RANGE_PAIRS forces small ranges).  Stack
//              2 p + s of the range is side s of its pair p; a pair that does not yield has two stacks of no rows and no columns.  The
//              LIVE rows of a stack -- len > 0 and start + len > w0, w0 = the window's start -- are found on the host from the placed
//              records and the reads' lengths: the walk already left every other entry out, so nearly every row is live.
//   batches    as many stacks of the range as fit the room (or stacks_per_batch); the reads their live rows name gathered once each
//              (dfk_cons.inc's cn_batch_reads), decoded (k_cn_decode) and lowered (k_wk_lower).
//   consensus  a workgroup a TILE of 256 columns of a stack (2 tiles a stack), a lane a column: the live rows walked once in order,
//              their headers staged through LDS 256 at a time; a lane carries four doubles and four counts of cells with Qual >= 30, a
//              base each, so the recount needs no second pass.  con and the unflattened conq are written at the stack's place.
//   flat       a lane a column of the range: the run through its column measured at most 9 columns each way (flat_at), across tiles.
//   conflicts  a workgroup a pair, both con and conq in LDS, a lane an offset index (conflicts_at).
//
// The file (dfk_scons_write).  Numbers are little-endian, no byte undefined.
//   a.stack.cons   "DFKSCON1" | u64 n = 2 * n_pairs | (n + 1) x u64 starts, in columns | (n_pairs + 1) x u64 first conflict entry of each
//                  pair | n x 16-byte dims { u32 rows, u32 rows_kept, i32 M, u32 cols } | con, a byte a base | conq, a byte each, after
//                  the flat pass | the conflict counts, u16 each: n1 + n2 a yielding pair, offset at index offset + n2 | zero bytes to a
//                  multiple of 8.  Element 2 pi + s is side s of pair pi.
#pragma once
#include <stdint.h>
#include <math.h>
#include "dfk_walks.h"
#include "dfk_cons.h"
#include "dfk_closures.h"

namespace dfk_scons {

constexpr int32_t QUALCAP = 100;                   // Stackster.cc:468
constexpr double MAX_QCOMP = 100.0;                // ReadStack.cc:422
constexpr uint8_t BAD_QUAL = 30;                   // ReadStack.cc:426
constexpr uint32_t BAD_COUNT = 2;                  // ReadStack.cc:427
constexpr int64_t MIN_FLAT = 10;                   // Stackster.cc:473
constexpr uint32_t CONFLICTS = 10;                 // Stackster.cc:558
constexpr int64_t MAX_WIDTH = dfk_walks::MAX_WIDTH;
constexpr uint32_t GROUP = 256;                    // lanes of a workgroup: a tile of columns
constexpr uint32_t TILES = (uint32_t)((MAX_WIDTH + GROUP - 1) / GROUP);       // 2
constexpr uint64_t SALT = 0x5C05ull;               // k_digest_seq's: the dims as u32 words, con, conq, the conflict counts, a value each

DFK_CN_HD int64_t window_start(int64_t M) { return M > MAX_WIDTH ? M - MAX_WIDTH : 0; }            // :436-440: trim
DFK_CN_HD bool row_rc(bool loc_fw) { return !loc_fw; }                                               // :425
DFK_CN_HD bool span_meets(int32_t start, uint32_t len, int64_t w0) { return len != 0 && (int64_t)start + (int64_t)len > w0; }
// the stack column (before Trim and Reverse) of output column c: Reverse applies to side 1
DFK_CN_HD int64_t stack_column(int64_t w0, int64_t cols, bool reversed, int64_t c) { return reversed ? w0 + cols - 1 - c : w0 + c; }
// THE CELL: the index j into the row's ORIENTED read that stack column sc holds, or -1 (:427-431; sc >= 0 and sc < M by construction)
DFK_CN_HD int64_t cell_index(int32_t start, uint32_t len, int64_t sc)
{
    const int64_t j = sc - (int64_t)start;
    return j >= 0 && j < (int64_t)len ? j : -1;
}
DFK_CN_HD void add4(uint32_t* cnt, uint32_t base, uint32_t v)
{
    switch (base) {
        case 0: cnt[0] += v; break;
        case 1: cnt[1] += v; break;
        case 2: cnt[2] += v; break;
        default: cnt[3] += v; break;
    }
}
// one row's cell in a column added to the column's sums and, with Qual >= 30 (as a char: below 128 too), to its base's count; true if
// the cell is defined.  packed and quals are the read as stored, quals lowered.
DFK_CN_HD bool add_row(double* sum, uint32_t* bad, int32_t start, uint32_t len, bool rc, bool reversed, int64_t sc, const uint8_t* packed, const uint8_t* quals)
{
    const int64_t j = cell_index(start, len, sc);
    if (j < 0) return false;
    const uint8_t q = dfk_walks::oriented_qual(quals, len, rc, (uint32_t)j);
    if (!dfk_cons::cell_defined(q)) return false;
    const uint32_t b = dfk_walks::oriented_base(packed, len, rc, (uint32_t)j), base = reversed ? 3u - b : b;
    dfk_cons::add_cell(sum, base, q);
    add4(bad, base, q >= BAD_QUAL ? 1u : 0u);
    return true;
}
// THE ROUNDING: C's round, half away from zero.  x - trunc(x) is exact in a double, so the comparison with 0.5 is; floor(x + 0.5) is not
// round: 0.49999999999999994 + 0.5 is 1.
DFK_CN_HD double round_half_away(double x)
{
    const double t = ::trunc(x), f = ::fabs(x - t);
    return f >= 0.5 ? t + (x < 0 ? -1.0 : 1.0) : t;
}
// mx.reverseSort(): id(0), val(0) of the greatest ( sum, id ) pair, id(1), val(1) of the second greatest
struct TopTwo { uint32_t id0, id1; double val0, val1; };
DFK_CN_HD TopTwo top_two(const double* sum)
{
    const double s0 = sum[0], s1 = sum[1], s2 = sum[2], s3 = sum[3];
    TopTwo t{0, 4, s0, 0.};
    if (!(s1 < t.val0)) { t.id0 = 1; t.val0 = s1; }
    if (!(s2 < t.val0)) { t.id0 = 2; t.val0 = s2; }
    if (!(s3 < t.val0)) { t.id0 = 3; t.val0 = s3; }
    if (t.id0 != 0) { t.id1 = 0; t.val1 = s0; }
    if (t.id0 != 1 && (t.id1 == 4 || !(s1 < t.val1))) { t.id1 = 1; t.val1 = s1; }
    if (t.id0 != 2 && (t.id1 == 4 || !(s2 < t.val1))) { t.id1 = 2; t.val1 = s2; }
    if (t.id0 != 3 && (t.id1 == 4 || !(s3 < t.val1))) { t.id1 = 3; t.val1 = s3; }
    return t;
}
DFK_CN_HD uint32_t pick4(const uint32_t* v, uint32_t i) { return i == 0 ? v[0] : i == 1 ? v[1] : i == 2 ? v[2] : v[3]; }
// THE CAP and the recount: conq of a column before the flat pass.  capped: int( round( . ) ) was 100 or more; recount: val(1) > 100 and
// two rows or more of Qual >= 30 on id(1)
struct Conq { uint8_t conq; bool capped, recount; };
DFK_CN_HD Conq conq_of(const TopTwo& t, const uint32_t* bad)
{
    const double r = round_half_away(t.val0 - t.val1);                                              // ReadStack.cc:421; >= 0
    Conq c{(uint8_t)(r >= (double)QUALCAP ? QUALCAP : (int32_t)r), r >= (double)QUALCAP, false};
    if (t.val1 > MAX_QCOMP && pick4(bad, t.id1) >= BAD_COUNT) { c.conq = 0; c.recount = true; }     // :423-427
    return c;
}
// THE FLAT TEST: does column c of con[0, cols) lie in a run of MIN_FLAT equal bases or more?  At most 9 columns each way are looked at.
DFK_CN_HD bool flat_at(const uint8_t* con, int64_t cols, int64_t c)
{
    const uint8_t b = con[c];
    int64_t run = 1;
    for (int64_t j = c - 1; j >= 0 && run < MIN_FLAT && con[j] == b; --j) ++run;
    for (int64_t j = c + 1; j < cols && run < MIN_FLAT && con[j] == b; ++j) ++run;
    return run >= MIN_FLAT;
}
// THE CONFLICT TEST (:554-556) and the count of an offset (:550-557)
DFK_CN_HD bool conflict(uint8_t c1, uint8_t q1, uint8_t c2, uint8_t q2) { return q1 == QUALCAP && q2 == QUALCAP && c1 != c2; }
DFK_CN_HD uint32_t conflicts_at(const uint8_t* con1, const uint8_t* q1, int64_t n1, const uint8_t* con2, const uint8_t* q2, int64_t n2, int64_t offset)
{
    const int64_t lo = offset > 0 ? offset : 0, hi = n1 < offset + n2 ? n1 : offset + n2;          // 0 <= i1 < n1 and 0 <= i1 - offset < n2
    uint32_t n = 0;
    for (int64_t i1 = lo; i1 < hi; ++i1) n += conflict(con1[i1], q1[i1], con2[i1 - offset], q2[i1 - offset]) ? 1u : 0u;
    return n;
}

} // namespace dfk_scons

// ---------------------------------------------------------------------------------------------------------------- host only
#include <cmath>
#include <functional>
#include <utility>

namespace dfk_scons {

typedef dfk_cons::Dim Dim;                         // { u32 rows, u32 rows_kept, i32 M, u32 cols }

// everything as plain arrays: the walks in dfk_walks_fetch's forms, the reads
struct Input {
    uint64_t n_pairs; const uint64_t* starts /* [2 * n_pairs + 1] */; const dfk_walks::Rec* recs; const dfk_walks::Loc* locs;
    uint64_t n_reads; const uint8_t* read_packed; const uint64_t* read_off /* [N + 1], bytes */; const uint32_t* read_len;
    const uint8_t* pq; const uint64_t* pq_off /* [N + 1] */;
};

struct HostResult {
    std::vector<uint64_t> starts;                  // [2 * n_pairs + 1], in columns
    std::vector<uint64_t> cfirst;                  // [n_pairs + 1], in conflict entries
    std::vector<Dim> dims;
    std::vector<uint8_t> con, conq;
    std::vector<uint16_t> counts;
    uint64_t yielding = 0, rows = 0, rows_kept = 0, trimmed = 0, cells = 0, capped = 0, recount = 0, flat = 0, allowed = 0, disallowed = 0, decoded = 0, batches = 0, ranges = 0;
};

inline bool yields(const dfk_walks::Rec* recs, uint64_t pi)
{
    return recs[2 * pi].status == dfk_walks::WALKED && recs[2 * pi + 1].status == dfk_walks::WALKED && recs[2 * pi].placed > 0 && recs[2 * pi + 1].placed > 0;
}
// what the tables must hold for the stage to read them.  -1: the starts fall, do not begin at 0 or disagree with `placed`; -2: a placed
// record names a read outside [0, N) or lies 2^30 away; -4: M of a yielding side is not the maximum of start + len over its rows
inline int check_walks(const Input& I)
{
    if (I.starts[0] != 0) return -1;
    for (uint64_t q = 0; q < 2 * I.n_pairs; ++q) if (I.starts[q + 1] < I.starts[q] || I.starts[q + 1] - I.starts[q] != I.recs[q].placed) return -1;
    for (uint64_t j = 0; j < I.starts[2 * I.n_pairs]; ++j)
        if (I.locs[j].id < 0 || (uint64_t)I.locs[j].id >= I.n_reads || I.locs[j].start <= -(1 << 30) || I.locs[j].start >= (1 << 30) || I.locs[j].fw > 1) return -2;
    for (uint64_t pi = 0; pi < I.n_pairs; ++pi) {
        if (!yields(I.recs, pi)) continue;
        for (uint64_t q = 2 * pi; q < 2 * pi + 2; ++q) {
            int64_t M = 0;
            for (uint64_t j = I.starts[q]; j < I.starts[q + 1]; ++j) M = std::max<int64_t>(M, (int64_t)I.locs[j].start + (int64_t)I.read_len[I.locs[j].id]);
            if (M != I.recs[q].M || M >= (1ll << 31)) return -4;
        }
    }
    return 0;
}

// ---- the literal transcription for one side: Stackster.cc:409-440 and the readstack's members as they stand, the stack materialised.
// -3: a read's PQVec stream does not hold len values
inline int stack_grids(const Input& I, uint64_t q, uint32_t side, Dim* dim, dfk_cons::Grids* G, HostResult* counters)
{
    const uint64_t l0 = I.starts[q], n = I.starts[q + 1] - l0;
    std::vector<dfk_walks::basevector> by(n); std::vector<dfk_walks::qualvector> qy(n);
    for (uint64_t i = 0; i < n; i++) {                                                           // basesy[ src[i] ], qualsy[ src[i] ]: loaded, lowered, oriented (:329-380)
        const dfk_walks::Loc& L = I.locs[l0 + i];
        const uint32_t len = I.read_len[L.id];
        const uint8_t* pk = I.read_packed + I.read_off[L.id];
        std::vector<uint8_t> qq((size_t)len + 1);
        if (!dfk_cons::decode_quals(I.pq, I.pq_off[L.id], I.pq_off[L.id + 1], qq.data(), len)) return -3;
        dfk_walks::lower_read(pk, len, qq.data());
        const bool rc = !L.fw;                                                                   // :425 SetRc2( i, !fw ): the entry was reverse-complemented
        by[i].resize(len); qy[i].resize(len);
        for (uint32_t j = 0; j < len; j++) { by[i][j] = (uint8_t)dfk_walks::oriented_base(pk, len, rc, j); qy[i][j] = dfk_walks::oriented_qual(qq.data(), len, rc, j); }
    }
    int M = 0;                                                                                   // :409
    for (uint64_t i = 0; i < n; i++) M = std::max(M, I.locs[l0 + i].start + (int)by[i].size());  // :414
    int rows = (int)n, cols = M;
    std::vector<std::vector<int8_t>> bases_(rows, std::vector<int8_t>(M, ' ')), quals_(rows, std::vector<int8_t>(M, -1));    // :416
    for (uint64_t i = 0; i < n; i++) {                                                           // :417
        const int pos = I.locs[l0 + i].start;
        for (int j = 0; j < (int)by[i].size(); j++) {
            const int p = pos + j;
            if (p >= 0 && p < cols) { bases_[i][p] = (int8_t)by[i][j]; quals_[i][p] = (int8_t)qy[i][j]; }   // :429-431
        }
    }
    dim->rows = (uint32_t)rows; dim->M = M;
    if (cols > (int)MAX_WIDTH) {                                                                 // :437-440; ReadStack.cc:714-725
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
    if (side == 1) {                                                                             // :446; ReadStack.cc:346-353
        for (int i = 0; i < rows; i++) {
            std::reverse(bases_[i].begin(), bases_[i].end());
            for (int j = 0; j < cols; j++) if (bases_[i][j] != ' ') bases_[i][j] = (int8_t)(3 - bases_[i][j]);
            std::reverse(quals_[i].begin(), quals_[i].end());
        }
    }
    dim->rows_kept = (uint32_t)rows; dim->cols = (uint32_t)cols;
    G->bases_.swap(bases_); G->quals_.swap(quals_); G->rows = rows; G->cols = cols;
    return 0;
}
// readstack::Consensus1( con, conq, qualcap ) as written (ReadStack.cc:406-427)
inline void consensus1_literal(const dfk_cons::Grids& s, const int qualcap, std::vector<uint8_t>* con, std::vector<uint8_t>* conq, HostResult* counters)
{
    con->assign((size_t)s.cols, 0); conq->assign((size_t)s.cols, 0);
    for (int i = 0; i < s.cols; i++) {
        std::pair<double, int> mVals[4];                                                          // BaseMetrics<double> mx
        for (int idx = 0; idx < 4; ++idx) { mVals[idx].first = 0.; mVals[idx].second = idx; }
        for (int j = 0; j < s.rows; j++) {
            double q = s.quals_[j][i];
            if (q <= 2) q = std::min(q, 0.2);
            if (q == 0) q = 0.1;
            if (s.quals_[j][i] >= 0) { mVals[(int)s.bases_[j][i]].first += q; ++counters->cells; }
        }
        std::sort(mVals, mVals + 4, std::greater<std::pair<double, int>>());                      // mx.reverseSort()
        (*con)[i] = (uint8_t)mVals[0].second;
        const int r = int(std::round(mVals[0].first - mVals[1].first));
        (*conq)[i] = (uint8_t)std::min(qualcap, r);                                               // :421
        counters->capped += r >= qualcap;
        const int max_qcomp = 100;
        if (mVals[1].first > max_qcomp) {
            int badcount = 0;
            for (int j = 0; j < s.rows; j++) if (s.quals_[j][i] >= 30 && s.bases_[j][i] == mVals[1].second) badcount++;
            if (badcount >= 2) { (*conq)[i] = 0; ++counters->recount; }
        }
    }
}
// :473-489, on one side
inline void min_flat_literal(const std::vector<uint8_t>& con1x, std::vector<uint8_t>* conq1x, HostResult* counters)
{
    const int MIN_FLAT_ = 10;
    for (int i = 0; i < (int)con1x.size(); i++) {
        int j;
        for (j = i + 1; j < (int)con1x.size(); j++) if (con1x[j] != con1x[i]) break;
        if (j - i >= MIN_FLAT_) { for (int k = i; k < j; k++) (*conq1x)[k] = 0; counters->flat += (uint64_t)(j - i); }
        i = j - 1;
    }
}
// :550-557 for one offset
inline int conflicts_literal(const std::vector<uint8_t>& con1x, const std::vector<uint8_t>& conq1x, const std::vector<uint8_t>& con2x, const std::vector<uint8_t>& conq2x, int offset)
{
    int conflicts = 0;
    for (int i1 = 0; i1 < (int)con1x.size(); i1++) {
        int i2 = i1 - offset;
        if (i2 < 0 || i2 >= (int)con2x.size()) continue;
        if (conq1x[i1] == QUALCAP && conq2x[i2] == QUALCAP && con1x[i1] != con2x[i2]) conflicts++;
    }
    return conflicts;
}
inline void push_side(HostResult* R, const Dim& d, const std::vector<uint8_t>& con, const std::vector<uint8_t>& conq)
{
    R->dims.push_back(d); R->con.insert(R->con.end(), con.begin(), con.end()); R->conq.insert(R->conq.end(), conq.begin(), conq.end());
    R->starts.push_back(R->con.size()); R->rows += d.rows; R->rows_kept += d.rows_kept;
}

// -1, -2, -4: check_walks'; -3: a PQVec stream of the wrong length
inline int scons_literal(const Input& I, HostResult* R)
{
    if (int rc = check_walks(I)) return rc;
    R->starts.assign(1, 0); R->cfirst.assign(1, 0);
    for (uint64_t pi = 0; pi < I.n_pairs; ++pi) {
        if (yields(I.recs, pi)) {
            ++R->yielding;
            std::vector<uint8_t> conx[2], conqx[2];
            for (uint32_t s = 0; s < 2; ++s) {
                Dim d{}; dfk_cons::Grids G;
                if (int rc = stack_grids(I, 2 * pi + s, s, &d, &G, R)) return rc;
                consensus1_literal(G, QUALCAP, &conx[s], &conqx[s], R);                          // :471-472
                min_flat_literal(conx[s], &conqx[s], R);
                push_side(R, d, conx[s], conqx[s]);
            }
            const int n1 = (int)conx[0].size(), n2 = (int)conx[1].size();                        // :466
            for (int offset = -n2; offset < n1; ++offset) {
                const int conflicts = conflicts_literal(conx[0], conqx[0], conx[1], conqx[1], offset);
                R->counts.push_back((uint16_t)conflicts);                                        // at index offset + n2
                if (conflicts < (int)CONFLICTS) ++R->allowed; else ++R->disallowed;              // :559-562
            }
        } else for (int s = 0; s < 2; ++s) push_side(R, Dim{0, 0, 0, 0}, {}, {});
        R->cfirst.push_back(R->counts.size());
    }
    return 0;
}

// ---- the plan
// A range of PAIRS: as many as keep the rows of their stacks at the cap; a row costs its header on the host and the device (24 bytes).
constexpr uint64_t BYTES_PER_ROW = 24;
inline uint64_t row_cap(uint64_t free_now, uint64_t forced) { return forced ? forced : std::max<uint64_t>(1ull << 18, free_now / 2 / BYTES_PER_ROW); }
// A batch of stacks of the range: dfk_cons.h's cost of a stack and of a live row, and its next_batch.
inline unsigned cons_grid(uint64_t n_stacks, unsigned cus) { return (unsigned)std::max<uint64_t>(1, std::min<uint64_t>(n_stacks * TILES, 32ull * cus)); }   // a workgroup a tile
inline unsigned pair_grid(uint64_t n_pairs, unsigned cus) { return (unsigned)std::max<uint64_t>(1, std::min<uint64_t>(n_pairs, 32ull * cus)); }            // a workgroup a pair

// The device version's order of work on the host, for the CPU test.  stacks_per_batch 0 = what fits `room`; returns as scons_literal
inline int scons_plan(const Input& I, uint64_t stacks_per_batch, uint64_t room, uint64_t rows_cap, HostResult* R)
{
    if (int rc = check_walks(I)) return rc;
    const uint64_t np_all = I.n_pairs;
    std::vector<uint64_t> prows(np_all, 0);
    for (uint64_t pi = 0; pi < np_all; ++pi) if (yields(I.recs, pi)) { prows[pi] = I.starts[2 * pi + 2] - I.starts[2 * pi]; ++R->yielding; }
    const std::vector<uint64_t> pfirst = dfk::prefix_sums(prows.data(), np_all);
    R->starts.assign(1, 0); R->cfirst.assign(1, 0);
    for (uint64_t p0 = 0; p0 < np_all;) {
        const uint64_t p1 = dfk::pidx_next_range(pfirst.data(), np_all, p0, rows_cap).e1, ns = 2 * (p1 - p0);
        ++R->ranges;
        // the stacks of the range: M, the window, the live rows (host)
        std::vector<int64_t> M(ns, 0), w0(ns, 0);
        std::vector<uint64_t> n_rows(ns, 0), lfirst(ns + 1, 0), ofirst(ns + 1, 0), cost(ns, 0);
        std::vector<uint32_t> l_id, l_len; std::vector<int32_t> l_start; std::vector<uint8_t> l_rc;
        for (uint64_t s = 0; s < ns; ++s) {
            const uint64_t q = 2 * p0 + s;
            if (yields(I.recs, q / 2)) {
                M[s] = I.recs[q].M; w0[s] = window_start(M[s]); n_rows[s] = I.starts[q + 1] - I.starts[q];
                for (uint64_t j = I.starts[q]; j < I.starts[q + 1]; ++j) {
                    const dfk_walks::Loc& L = I.locs[j];
                    if (!span_meets(L.start, I.read_len[L.id], w0[s])) continue;
                    l_id.push_back((uint32_t)L.id); l_start.push_back(L.start); l_len.push_back(I.read_len[L.id]); l_rc.push_back(row_rc(L.fw != 0));
                }
            }
            lfirst[s + 1] = l_id.size(); ofirst[s + 1] = ofirst[s] + (uint64_t)(M[s] - w0[s]);
            cost[s] = dfk_cons::BYTES_PER_STACK;
            for (uint64_t l = lfirst[s]; l < lfirst[s + 1]; ++l) cost[s] += dfk_cons::live_row_cost(l_len[l]);
        }
        std::vector<uint8_t> con(ofirst[ns]), conq(ofirst[ns]), defined(l_id.size(), 0);
        const std::vector<uint64_t> cfirst = dfk::prefix_sums(cost.data(), ns);
        for (uint64_t b0 = 0; b0 < ns;) {
            const uint64_t b1 = dfk_cons::next_batch(cfirst.data(), ns, b0, room, stacks_per_batch);
            ++R->batches;
            // the reads of the batch, each once, ascending; the gather; the decode and the lowering (a thread a read)
            std::vector<uint32_t> ids(l_id.begin() + lfirst[b0], l_id.begin() + lfirst[b1]);
            std::sort(ids.begin(), ids.end()); ids.erase(std::unique(ids.begin(), ids.end()), ids.end());
            std::vector<uint64_t> b_at(ids.size() + 1, 0), q_at(ids.size() + 1, 0);
            for (size_t i = 0; i < ids.size(); ++i) { const uint32_t len = I.read_len[ids[i]]; b_at[i + 1] = b_at[i] + (len + 3) / 4; q_at[i + 1] = q_at[i] + len; }
            std::vector<uint8_t> bases(b_at.back()), quals(q_at.back());                          // (capacity == size: a read past the end is the sanitizer's to see)
            for (size_t i = 0; i < ids.size(); ++i) {
                std::copy(I.read_packed + I.read_off[ids[i]], I.read_packed + I.read_off[ids[i]] + (b_at[i + 1] - b_at[i]), bases.begin() + b_at[i]);
                if (!dfk_cons::decode_quals(I.pq, I.pq_off[ids[i]], I.pq_off[ids[i] + 1], quals.data() + q_at[i], I.read_len[ids[i]])) return -3;
                dfk_walks::lower_read(bases.data() + b_at[i], I.read_len[ids[i]], quals.data() + q_at[i]);
            }
            R->decoded += ids.size();
            // the consensus: a lane a column, the live rows in order
            for (uint64_t s = b0; s < b1; ++s) {
                const int64_t cols = M[s] - w0[s];
                const bool rev = (s & 1) != 0;
                for (int64_t c = 0; c < cols; ++c) {
                    const int64_t sc = stack_column(w0[s], cols, rev, c);
                    double sum[4] = {0., 0., 0., 0.};
                    uint32_t bad[4] = {0, 0, 0, 0};
                    for (uint64_t l = lfirst[s]; l < lfirst[s + 1]; ++l) {
                        const uint64_t slot = dfk_cons::slot_of(ids.data(), ids.size(), l_id[l]);
                        if (add_row(sum, bad, l_start[l], l_len[l], l_rc[l] != 0, rev, sc, bases.data() + b_at[slot], quals.data() + q_at[slot])) { defined[l] = 1; ++R->cells; }
                    }
                    const TopTwo t = top_two(sum);
                    const Conq k = conq_of(t, bad);
                    con[ofirst[s] + (uint64_t)c] = (uint8_t)t.id0; conq[ofirst[s] + (uint64_t)c] = k.conq;
                    R->capped += k.capped; R->recount += k.recount;
                }
            }
            b0 = b1;
        }
        // the flat pass: a lane a column of the range (in place: a lane reads con and writes its own conq)
        for (uint64_t s = 0; s < ns; ++s)
            for (int64_t c = 0; c < (int64_t)(ofirst[s + 1] - ofirst[s]); ++c)
                if (flat_at(con.data() + ofirst[s], (int64_t)(ofirst[s + 1] - ofirst[s]), c)) { conq[ofirst[s] + (uint64_t)c] = 0; ++R->flat; }
        // the conflicts: a workgroup a pair, a lane an offset index
        for (uint64_t p = 0; p < p1 - p0; ++p) {
            const int64_t n1 = (int64_t)(ofirst[2 * p + 1] - ofirst[2 * p]), n2 = (int64_t)(ofirst[2 * p + 2] - ofirst[2 * p + 1]);
            if (yields(I.recs, p0 + p))
                for (int64_t k = 0; k < n1 + n2; ++k) {
                    const uint32_t n = conflicts_at(con.data() + ofirst[2 * p], conq.data() + ofirst[2 * p], n1, con.data() + ofirst[2 * p + 1], conq.data() + ofirst[2 * p + 1], n2, k - n2);
                    R->counts.push_back((uint16_t)n);
                    if (n < CONFLICTS) ++R->allowed; else ++R->disallowed;
                }
            R->cfirst.push_back(R->counts.size());
        }
        for (uint64_t s = 0; s < ns; ++s) {
            uint64_t kept = 0;
            for (uint64_t l = lfirst[s]; l < lfirst[s + 1]; ++l) kept += defined[l];
            const Dim d{(uint32_t)n_rows[s], (uint32_t)(M[s] > MAX_WIDTH ? kept : n_rows[s]), (int32_t)M[s], (uint32_t)(M[s] - w0[s])};
            R->dims.push_back(d); R->rows += d.rows; R->rows_kept += d.rows_kept; R->trimmed += M[s] > MAX_WIDTH;
            R->starts.push_back(R->starts.back() + d.cols);
        }
        R->con.insert(R->con.end(), con.begin(), con.end()); R->conq.insert(R->conq.end(), conq.begin(), conq.end());
        p0 = p1;
    }
    return 0;
}

// ---- the file's fixed parts
constexpr const char* MAGIC = "DFKSCON1";
inline uint64_t cfirst_at(uint64_t n) { return 16 + 8 * (n + 1); }
inline uint64_t dims_at(uint64_t n) { return cfirst_at(n) + 8 * (n / 2 + 1); }
inline uint64_t con_at(uint64_t n) { return dims_at(n) + 16 * n; }
inline uint64_t conq_at(uint64_t n, uint64_t n_cols) { return con_at(n) + n_cols; }
inline uint64_t counts_at(uint64_t n, uint64_t n_cols) { return conq_at(n, n_cols) + n_cols; }
inline uint64_t file_size(uint64_t n, uint64_t n_cols, uint64_t n_counts) { return (counts_at(n, n_cols) + 2 * n_counts + 7) & ~7ull; }

} // namespace dfk_scons
