// superplus_amd/csrc/dfk_walks.h -- Stackster's two stack walks per pair (10X/Stackster.cc:207-262 StackWalk; :326-414 loading, lowering,
// orientation, the locs, M and trim of each side): which entries of the pair's read set enter each stack and where, and the walked
// sequence EE.  No stack is stored.  The rule over plain arrays, the pieces host and kernels share stated once, the form the device
// runs and its plan, the layout of a.stack.walks.
//
// No HIP call and no device pointer is dereferenced here by the host, so tests/cpp/test_walks.cc compiles this header with a plain
// host compiler (and once more under -fsanitize=address,undefined) and checks it against cases recorded from tests/walks_oracle.py.
// It is the SECOND restatement of the rule -- written from the reference's text, not from the Python.
//
// The rule (a pair pi = (e1, e2), es = { e1, inv[e2] }, ALT = False, idsfw2 empty, k = 48 whatever the graph's K):
//   the set (:295-324)   idsfw = dfk_closer.h's pair_composed(reads(es[0]), reads(es[1])): sorted distinct ( id << 1 | fw ).  A read may
//                        stand twice, once with each flag: two ENTRIES.
//   lowering (:348-360)  on the read as stored: every maximal run of one base of length >= 20 gets q = min(q, 5); q the PQVec-decoded
//                        bytes (unsigned char).
//   sides (:368-391)     side s walks E = O(es[s]) (:386 reverse-complements edges[1] = O(e2)).  Entry ( id, fw ) is reverse-complemented,
//                        its qualities reversed, iff fw == ( s == 1 ): as stored on side 0 when fw (:369-371), the other way round on
//                        side 1 (:378-380).
//   StackWalk (:207-262) EE = E[0:48].  Each step: x = the last 48 bases of EE; [low, high) its range in the sorted table of
//                        ( 48-mer, entry, pos ) over all forward 48-mers of the oriented entries (MakeKmerLookup0); if two neighbours in
//                        the range share the entry the step places nobody (:238-242); else every entry there not yet placed is placed
//                        with start = |EE| - 48 - pos (may be negative).  qsum[b], ints from 0: over placed entries with p = |EE| - start
//                        < len (p >= 48 always) the quality at p under the base at p.  The walk ends if the largest sum is < 60 or
//                        double(largest) < 2.0 * double(second); else the base of the largest is appended.
//   locs (:398-408)      per placed entry in entry order ( id, start, fw ^ ( s == 1 ) ); none: Stackster returns -- after side 0, side 1 is
//                        not walked.  M = max over placed of start + len from 0 (:409-414); trim = max(0, M - 400) (:436-438).
//   An edge of fewer than 48 bases (K < 48 only; the reference's SetToSubOf is undefined there) is not walked: status SHORT, and a side 1
//   behind a side 0 that placed nobody or was short has status NOT_WALKED.
//
// What does not depend on order, and what needs no tie rule (tests/cpp/test_walks.cc checks each):
//   - placement: an entry is placed by the first step whose 48-mer it holds (once, that step), with a start that depends on that step and
//     its own pos alone; the sums are integers: neither depends on the order of the entries.  The sums cannot wrap: a set of 2^23
//     entries or more is refused, and 2^23 x 255 < 2^31.
//   - a base is appended only when top >= 60 and top >= 2 x second, so top > second: the maximum is unique.
//   - :261's double comparison is the integer one: both sums are ints below 2^31, exact in a double, and so is twice one (decide()).
//
// THE BOUND on |EE| (ee_bound): |EE| <= 48 + the sum over entries with len >= 48 of (len - 48).  Proof: let R = max(48, max over placed
// entries of start + len).  A base is appended at |EE| = L only if some placed entry has L - start < len, so L < R: |EE| <= R always.  An
// entry is placed at some |EE| = L <= R with start = L - 48 - pos <= L - 48, which raises R to at most max(R, L - 48 + len) <= R + (len -
// 48).  Every entry is placed at most once and R starts at 48.  The device's output is sized by it and its step loop counted by it: a
// walk is never cut silently.
//
// The form the device runs (dfk_walks_kernels.h, dfk_walks.inc; walks_plan() below is its order of work on the host):
//   ranges     whole pairs, as many as keep their set entries at the cap (DFK_PIDX_RANGE_PAIRS forces small ranges): the sets of a range
//              are composed on the host from the closer's per-edge sets (a merge of two sorted lists).
//   batches    whole pairs of the range, as many as fit the room (or walks_per_batch walks, rounded up to whole pairs: side 1 needs side 0's
//              outcome).  The distinct reads of the batch are gathered and decoded ONCE (dfk_cons.inc's gather and decode) and lowered
//              once per read: lowering does not depend on orientation (lower_read).
//   the table  per side: every forward 48-mer of every oriented entry gives ( pair, 64-bit hash of the 48-mer ) -> ( entry, pos ); one
//              device-wide STABLE sort by ( pair, hash ) (the closer's radix sort on a permutation: hash low word, high word, pair).  The
//              48-mers are generated in ( pair, entry, pos ) order, so within one hash value of one pair they stay in ( entry, pos ) order.
//   the walk   a wave a walk.  The 96-bit key of the last 48 bases stays in registers and is rolled by a base (Key96, roll()).  A step
//              finds the lower bound of hash(key) in the pair's segment, and every lane takes one hit: it VERIFIES all 48 bases against
//              the oriented read (key_at), so a collision costs time, never correctness.  A verified hit whose entry has another verified
//              hit makes the step a duplicate: the lane looks back while the entry stays the same (the order above).  Otherwise the
//              verified hits place their entries.  A placed entry that still covers the current column joins the LIVE list in LDS; the
//              sums run over that list a lane an entry, four integer sums reduced across the wave; an entry retires when the walk passes
//              its end.  A walk whose live list would outgrow DFK_WALK_MAX_LIVE (1024: 16 KiB of LDS a wave; the fixtures' largest list
//              is 47) stops and is done exactly by stack_walk() below on the host; the stats count it.
//
// The file (dfk_walks_write).  Numbers are little-endian, no byte undefined.
//   a.stack.walks  "DFKSWLK1" | u64 n = 2 * n_pairs | (n + 1) x u64 first placed record of each walk | (n + 1) x u64 first base of each EE |
//                  n x 32-byte records { u32 status, u32 entries, u32 placed, u32 dup_steps, i32 nE, u32 nEE, i32 M, i32 trim } | the
//                  placed records, 16 bytes { i64 id, i32 start, u32 fw } (dfk_closer::Loc) | the EE bases of all walks end to end, four
//                  a byte, the first in the low bits | zero bytes to a multiple of 8.  Element 2 pi + s is side s of pair pi.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define DFK_WK_HD __host__ __device__ inline
#else
#define DFK_WK_HD inline
#endif

#ifndef DFK_WALK_MAX_LIVE
#define DFK_WALK_MAX_LIVE 1024
#endif
#ifndef DFK_WALK_HASH_BITS
#define DFK_WALK_HASH_BITS 64        // the host test builds with 8 too: nearly every look-up then meets collisions, and verification decides
#endif

namespace dfk_walks {

constexpr uint32_t KW = 48;                        // Stackster.cc:212
constexpr int32_t MIN_WIN = 60;                    // :213
constexpr uint8_t HSTAR = 5;                       // :348
constexpr uint32_t HRUN = 20;                      // :357
constexpr int64_t MAX_WIDTH = 400;                 // :436
constexpr uint64_t MAX_ENTRIES = 1ull << 23;       // a set of so many entries is refused: 2^23 x 255 could pass an int
constexpr uint32_t MAX_LIVE = DFK_WALK_MAX_LIVE;
constexpr uint64_t SALT = 0xABABull;               // k_digest_seq's: the records as u32 words, the placed records as u64 words, the EE bases
enum Status : uint32_t { WALKED = 0, NOT_WALKED = 1, SHORT = 2 };

DFK_WK_HD uint32_t base_at(const uint8_t* packed, uint64_t j) { return (packed[j >> 2] >> (2 * (j & 3))) & 3u; }
// THE ORIENTATION of an entry on a side (:369-371, :378-380)
DFK_WK_HD bool entry_rc(bool fw, uint32_t side) { return fw == (side == 1); }
DFK_WK_HD uint32_t oriented_base(const uint8_t* packed, uint32_t len, bool rc, uint32_t j) { return rc ? 3u - base_at(packed, len - 1 - j) : base_at(packed, j); }
DFK_WK_HD uint8_t oriented_qual(const uint8_t* q, uint32_t len, bool rc, uint32_t j) { return rc ? q[len - 1 - j] : q[j]; }
DFK_WK_HD bool loc_fw(bool fw, uint32_t side) { return fw != (side == 1); }                       // :403

// THE LOWERING of one read, in place (:350-360)
DFK_WK_HD void lower_read(const uint8_t* packed, uint32_t len, uint8_t* q)
{
    for (uint32_t j = 0; j < len;) {
        uint32_t k = j + 1;
        const uint32_t b = base_at(packed, j);
        while (k < len && base_at(packed, k) == b) ++k;
        if (k - j >= HRUN) for (uint32_t l = j; l < k; ++l) if (q[l] > HSTAR) q[l] = HSTAR;
        j = k;
    }
}

// THE KEY: 48 bases in 96 bits, the newest in the lowest two; rolled by a base
struct Key96 { uint64_t lo; uint32_t hi; };
DFK_WK_HD Key96 roll(Key96 k, uint32_t b) { return Key96{(k.lo << 2) | b, (k.hi << 2) | (uint32_t)(k.lo >> 62)}; }
DFK_WK_HD bool same_key(Key96 a, Key96 b) { return a.lo == b.lo && a.hi == b.hi; }
DFK_WK_HD Key96 key_at(const uint8_t* packed, uint32_t len, bool rc, uint32_t pos)                 // pos + 48 <= len
{
    Key96 k{0, 0};
    for (uint32_t j = 0; j < KW; ++j) k = roll(k, oriented_base(packed, len, rc, pos + j));
    return k;
}
DFK_WK_HD Key96 key_of_edge(const uint8_t* packed) { return key_at(packed, KW, false, 0); }
DFK_WK_HD uint64_t mix64(uint64_t x)
{
    x ^= x >> 30; x *= 0xBF58476D1CE4E5B9ull; x ^= x >> 27; x *= 0x94D049BB133111EBull;
    return x ^ (x >> 31);
}
DFK_WK_HD uint64_t hash_mask(uint32_t bits) { return bits >= 64 ? ~0ull : (1ull << bits) - 1; }
// (the mask: all ones, but for the tests that want collisions; the library takes its bits from DFK_WALK_HASH_BITS in the environment)
DFK_WK_HD uint64_t hash_of(Key96 k, uint64_t mask = hash_mask(DFK_WALK_HASH_BITS)) { return mix64(k.lo ^ mix64((uint64_t)k.hi + 0x9E3779B97F4A7C15ull)) & mask; }

// THE DECISION of a step from its four sums (:259-262): true and the base to append, or false: the walk ends
DFK_WK_HD bool decide(const int32_t* sum, uint32_t* base)
{
    uint32_t top = 0;
    for (uint32_t b = 1; b < 4; ++b) if (sum[b] > sum[top]) top = b;
    int32_t second = -1;
    for (uint32_t b = 0; b < 4; ++b) if (b != top && sum[b] > second) second = sum[b];
    if (sum[top] < MIN_WIN) return false;
    if ((int64_t)sum[top] < 2 * (int64_t)second) return false;                                    // == double(top) < 2.0 * double(second)
    *base = top;
    return true;
}
DFK_WK_HD int32_t trim_of(int32_t M) { return M > MAX_WIDTH ? (int32_t)(M - MAX_WIDTH) : 0; }
DFK_WK_HD uint64_t kmers_of_len(uint32_t len) { return len >= KW ? (uint64_t)len - KW + 1 : 0; }
DFK_WK_HD uint64_t reach_of_len(uint32_t len) { return len >= KW ? (uint64_t)len - KW : 0; }       // what an entry adds to the bound
// the last i in [0, n) with first[i] <= x, first ascending with first[0] <= x
DFK_WK_HD uint64_t owner_of(const uint64_t* first, uint64_t n, uint64_t x)
{
    uint64_t lo = 0, hi = n;
    while (hi - lo > 1) { const uint64_t mid = lo + (hi - lo) / 2; if (first[mid] <= x) lo = mid; else hi = mid; }
    return lo;
}
DFK_WK_HD uint64_t lower_bound64(const uint64_t* a, uint64_t lo, uint64_t hi, uint64_t x)
{
    while (lo < hi) { const uint64_t mid = lo + (hi - lo) / 2; if (a[mid] < x) lo = mid + 1; else hi = mid; }
    return lo;
}

} // namespace dfk_walks

// ---------------------------------------------------------------------------------------------------------------- host only
#include <algorithm>
#include <array>
#include <tuple>
#include <vector>
#include "dfk_cons.h"         // decode_quals, slot_of
#include "dfk_paths_plan.h"   // pidx_next_range, prefix_sums

namespace dfk_walks {

struct Rec { uint32_t status, entries, placed, dup_steps; int32_t nE; uint32_t nEE; int32_t M, trim; };
struct Loc { int64_t id; int32_t start; uint32_t fw; };
static_assert(sizeof(Rec) == 32 && sizeof(Loc) == 16, "a.stack.walks records");

// everything as plain arrays: the graph, the closer edges with their bases ( O(ce[k]), 2-bit packed, at edge_at[k] ) and read sets in
// dfk_closer_fetch's form, the reads
struct Input {
    uint64_t n_edges; const int32_t* inv;
    uint64_t n_ce; const uint64_t* ce; const uint8_t* edge_store; const uint64_t* edge_at; const int32_t* edge_len;
    const uint64_t* read_first; const uint64_t* reads /* id << 1 | fw */;
    uint64_t n_reads; const uint8_t* read_packed; const uint64_t* read_off /* [N + 1], bytes */; const uint32_t* read_len;
    const uint8_t* pq; const uint64_t* pq_off /* [N + 1] */;
};

struct HostResult {
    std::vector<Rec> recs;                         // [2 * n_pairs]
    std::vector<uint64_t> starts, ee_starts;       // [2 * n_pairs + 1]
    std::vector<Loc> locs;
    std::vector<uint8_t> ee;                       // a byte a base
    uint64_t walks = 0, steps = 0, live_sum = 0, live_max = 0, host_route = 0, verified = 0, collisions = 0, decoded = 0, batches = 0, ranges = 0;
};

inline uint64_t rank_in(const uint64_t* ce, uint64_t n_ce, uint64_t e)
{
    const uint64_t k = (uint64_t)(std::lower_bound(ce, ce + n_ce, e) - ce);
    return k < n_ce && ce[k] == e ? k : n_ce;
}
// the ranks of es[0] and es[1] per pair.  -1: a pair names an edge outside [0, E); -2: a closer edge of a pair is not in ce
inline int sides_of(const Input& I, const int32_t* pairs, uint64_t n_pairs, std::vector<uint32_t>* side_rank)
{
    side_rank->assign(2 * n_pairs, 0);
    for (uint64_t i = 0; i < 2 * n_pairs; ++i) if (pairs[i] < 0 || (uint64_t)pairs[i] >= I.n_edges) return -1;
    for (uint64_t pi = 0; pi < n_pairs; ++pi) {
        const uint64_t es[2] = {(uint64_t)pairs[2 * pi], (uint64_t)I.inv[pairs[2 * pi + 1]]};
        for (int s = 0; s < 2; ++s) {
            const uint64_t k = rank_in(I.ce, I.n_ce, es[s]);
            if (k == I.n_ce) return -2;
            (*side_rank)[2 * pi + s] = (uint32_t)k;
        }
    }
    return 0;
}
// idsfw of a pair from the per-edge sets (dfk_closer.h, "a pair"): a merge of two ascending lists, the second with its flags negated
// (negating the lowest bit of ascending distinct words keeps them ascending but for neighbours id << 1, id << 1 | 1: sorted again)
inline void compose(const Input& I, uint64_t k0, uint64_t k1, std::vector<uint64_t>* out)
{
    out->assign(I.reads + I.read_first[k0], I.reads + I.read_first[k0 + 1]);
    for (uint64_t j = I.read_first[k1]; j < I.read_first[k1 + 1]; ++j) out->push_back(I.reads[j] ^ 1);
    std::sort(out->begin(), out->end());
    out->erase(std::unique(out->begin(), out->end()), out->end());
}
inline uint64_t ee_bound(const uint32_t* lens, uint64_t n)
{
    uint64_t b = KW;
    for (uint64_t i = 0; i < n; ++i) b += reach_of_len(lens[i]);
    return b;
}

// ---- the literal transcription
typedef std::vector<uint8_t> basevector;           // a byte a base
typedef std::vector<uint8_t> qualvector;
struct Walk { std::vector<uint8_t> placed; std::vector<int> start; basevector EE; uint32_t dup_steps = 0; uint64_t steps = 0, live_sum = 0, live_max = 0; int32_t last_sums[4] = {0, 0, 0, 0}; };

// StackWalk (:207-262) as it stands: the table materialised and sorted, lower and upper bound, the loop with its return
inline void stack_walk(const basevector& E, const std::vector<basevector>& bases, const std::vector<qualvector>& quals, Walk* W)
{
    const int K = 48;                                                                            // :212
    const int n = (int)bases.size();                                                             // :218
    W->placed.assign(n, 0); W->start.assign(n, -1);                                              // :219-220
    typedef std::tuple<std::array<uint8_t, 48>, int, int> triple;
    std::vector<triple> kmers_plus;                                                              // :221-222 MakeKmerLookup0
    for (int i = 0; i < n; i++)
        for (int p = 0; p + K <= (int)bases[i].size(); p++) {
            std::array<uint8_t, 48> x;
            std::copy(bases[i].begin() + p, bases[i].begin() + p + K, x.begin());
            kmers_plus.emplace_back(x, i, p);
        }
    std::sort(kmers_plus.begin(), kmers_plus.end());
    basevector& EE = W->EE;
    EE.assign(E.begin(), E.begin() + K);                                                         // :223
    while (1) {                                                                                  // :227
        ++W->steps;
        std::array<uint8_t, 48> x;                                                               // :231-232
        std::copy(EE.end() - K, EE.end(), x.begin());
        const int low = (int)(std::lower_bound(kmers_plus.begin(), kmers_plus.end(), x, [](const triple& t, const std::array<uint8_t, 48>& v) { return std::get<0>(t) < v; }) - kmers_plus.begin());   // :236
        const int high = (int)(std::upper_bound(kmers_plus.begin(), kmers_plus.end(), x, [](const std::array<uint8_t, 48>& v, const triple& t) { return v < std::get<0>(t); }) - kmers_plus.begin());  // :237
        bool duplicate = false;                                                                  // :238
        for (int i = low + 1; i < high; i++) if (std::get<1>(kmers_plus[i]) == std::get<1>(kmers_plus[i - 1])) { duplicate = true; break; }    // :239-242
        if (!duplicate) {                                                                        // :243
            for (int i = low; i < high; i++) {
                const int id = std::get<1>(kmers_plus[i]);
                if (W->placed[id]) continue;                                                     // :246
                const int pos = std::get<2>(kmers_plus[i]);
                W->placed[id] = 1;
                W->start[id] = (int)EE.size() - K - pos;                                         // :249
            }
        } else ++W->dup_steps;
        int qsum[4] = {0, 0, 0, 0}, ids[4] = {0, 1, 2, 3};                                       // :253
        uint64_t live = 0;
        for (int id = 0; id < n; id++) {                                                         // :254
            if (!W->placed[id]) continue;
            const int pos = (int)EE.size() - W->start[id];
            if (pos >= (int)bases[id].size()) continue;                                          // :257
            qsum[bases[id][pos]] += quals[id][pos];                                              // :258
            ++live;
        }
        W->live_sum += live; W->live_max = std::max(W->live_max, live);
        for (int b = 0; b < 4; b++) W->last_sums[b] = qsum[b];
        std::stable_sort(ids, ids + 4, [&](int a, int b) { return qsum[a] > qsum[b]; });         // :259 ReverseSortSync
        const int q0 = qsum[ids[0]], q1 = qsum[ids[1]];
        if (q0 < 60) return;                                                                     // :260
        if (double(q0) < 2.0 * double(q1)) return;                                               // :261
        EE.push_back((uint8_t)ids[0]);                                                           // :262
    }
}

// the reads of one pair loaded, unpacked, lowered and oriented for side 0 (:329-371).  -3: a PQVec stream of the wrong length
inline int load_pair(const Input& I, const std::vector<uint64_t>& idsfw, std::vector<basevector>* basesy, std::vector<qualvector>* qualsy)
{
    basesy->assign(idsfw.size(), basevector()); qualsy->assign(idsfw.size(), qualvector());
    for (size_t i = 0; i < idsfw.size(); i++) {
        const uint64_t id = idsfw[i] >> 1;
        const uint32_t len = I.read_len[id];
        basevector& b = (*basesy)[i]; qualvector& q = (*qualsy)[i];
        b.resize(len); q.resize(len);
        for (uint32_t j = 0; j < len; j++) b[j] = (uint8_t)base_at(I.read_packed + I.read_off[id], j);
        std::vector<uint8_t> qq((size_t)len + 1);
        if (!dfk_cons::decode_quals(I.pq, I.pq_off[id], I.pq_off[id + 1], qq.data(), len)) return -3;
        std::copy(qq.begin(), qq.begin() + len, q.begin());
        for (int j = 0; j < (int)q.size(); j++) {                                                // :353-360
            int k;
            for (k = j + 1; k < (int)q.size(); k++) if (b[k] != b[j]) break;
            if (k - j >= 20) for (int l = j; l < k; l++) q[l] = (uint8_t)std::min((int)q[l], 5);
            j = k - 1;
        }
        if (!(idsfw[i] & 1)) {                                                                   // :369-371
            std::reverse(b.begin(), b.end()); for (auto& x : b) x = (uint8_t)(3 - x);
            std::reverse(q.begin(), q.end());
        }
    }
    return 0;
}
inline basevector edge_bases(const Input& I, uint64_t k)
{
    basevector E((size_t)I.edge_len[k]);
    for (size_t j = 0; j < E.size(); j++) E[j] = (uint8_t)base_at(I.edge_store + I.edge_at[k], j);
    return E;
}
// one side after its walk: the locs, M, trim (:398-414, :436-438)
inline void finish_side(const std::vector<uint64_t>& idsfw, const uint32_t* lens, uint32_t side, const uint8_t* placed, const int32_t* start, Rec* r, std::vector<Loc>* locs)
{
    int M = 0;
    uint32_t n = 0;
    for (size_t i = 0; i < idsfw.size(); i++) {
        if (!placed[i]) continue;
        locs->push_back(Loc{(int64_t)(idsfw[i] >> 1), start[i], loc_fw((idsfw[i] & 1) != 0, side) ? 1u : 0u});
        M = std::max(M, start[i] + (int)lens[i]);
        ++n;
    }
    r->placed = n; r->M = M; r->trim = trim_of(M);
}
inline void append_walk(HostResult* R, const Rec& r, const std::vector<Loc>& locs, const uint8_t* ee)
{
    R->recs.push_back(r);
    R->locs.insert(R->locs.end(), locs.begin(), locs.end());
    R->ee.insert(R->ee.end(), ee, ee + r.nEE);
    R->starts.push_back(R->locs.size()); R->ee_starts.push_back(R->ee.size());
    if (r.status == WALKED) ++R->walks;
}

// -1, -2: sides_of's; -3: a PQVec stream of the wrong length; -4: a set of 2^23 entries or more
inline int walks_literal(const Input& I, const int32_t* pairs, uint64_t n_pairs, HostResult* R)
{
    std::vector<uint32_t> side_rank;
    if (int rc = sides_of(I, pairs, n_pairs, &side_rank)) return rc;
    R->starts.assign(1, 0); R->ee_starts.assign(1, 0);
    for (uint64_t pi = 0; pi < n_pairs; ++pi) {
        std::vector<uint64_t> idsfw;
        compose(I, side_rank[2 * pi], side_rank[2 * pi + 1], &idsfw);
        if (idsfw.size() >= MAX_ENTRIES) return -4;
        std::vector<basevector> basesy; std::vector<qualvector> qualsy;
        if (int rc = load_pair(I, idsfw, &basesy, &qualsy)) return rc;
        std::vector<uint32_t> lens(idsfw.size());
        for (size_t i = 0; i < idsfw.size(); i++) lens[i] = (uint32_t)basesy[i].size();
        bool go = true;
        for (uint32_t s = 0; s < 2; ++s) {
            const uint64_t k = side_rank[2 * pi + s];
            Rec r{go ? (uint32_t)WALKED : (uint32_t)NOT_WALKED, (uint32_t)idsfw.size(), 0, 0, I.edge_len[k], 0, 0, 0};
            std::vector<Loc> locs;
            Walk W;
            if (go && s == 1)                                                                    // :378-380
                for (size_t i = 0; i < basesy.size(); i++) { std::reverse(basesy[i].begin(), basesy[i].end()); for (auto& x : basesy[i]) x = (uint8_t)(3 - x); std::reverse(qualsy[i].begin(), qualsy[i].end()); }
            if (go && r.nE < (int32_t)KW) r.status = SHORT;
            else if (go) {
                stack_walk(edge_bases(I, k), basesy, qualsy, &W);                                // :391
                r.nEE = (uint32_t)W.EE.size(); r.dup_steps = W.dup_steps;
                finish_side(idsfw, lens.data(), s, W.placed.data(), W.start.data(), &r, &locs);
                R->steps += W.steps; R->live_sum += W.live_sum; R->live_max = std::max(R->live_max, W.live_max);
            }
            append_walk(R, r, locs, W.EE.data());
            if (!r.placed) go = false;                                                           // :404-408
        }
    }
    return 0;
}

// ---- the plan
// A range of PAIRS: as many as keep the entries of their sets (counted before duplicates between the two edges' sets are removed) at
// the cap; an entry costs its word on the host and, in a batch, what entry_cost says.
inline uint64_t entry_cap(uint64_t free_now, uint64_t forced) { return forced ? forced : std::max<uint64_t>(1ull << 18, free_now / 2 / 64); }
inline dfk::PidxRange next_range(const uint64_t* first, uint64_t n, uint64_t p0, uint64_t cap) { return dfk::pidx_next_range(first, n, p0, cap); }
// A batch of pairs.  An entry costs its slot, flags and both sides' placed / start (32 bytes), the read's packed bases, PQVec bytes and
// quality bytes (counted per entry though a read crosses once), its 48-mers in the table of one side (the two key words, pair, entry
// and position before the sort, two keys and two places in it, the sorted hash and value behind it: 52 bytes) and its share of EE's room.
constexpr uint64_t BYTES_PER_PAIR = 256 + 2 * KW;
inline uint64_t entry_cost(uint32_t len) { return 32 + (len + 3) / 4 + 2 * (uint64_t)len + 4 * ((uint64_t)len / 255 + 1) + 52 * kmers_of_len(len) + 2 * reach_of_len(len); }
inline uint64_t batch_room(uint64_t free_now) { return std::min<uint64_t>(std::max<uint64_t>(1ull << 20, free_now / 2), (1ull << 32) - 1); }     // (32-bit places in the sort, 32-bit offsets in LDS)
inline uint64_t pairs_per_batch(uint64_t walks_per_batch) { return (walks_per_batch + 1) / 2; }
inline uint64_t next_batch(const uint64_t* cost_first, uint64_t n, uint64_t b0, uint64_t room, uint64_t forced_pairs)
{
    if (forced_pairs) return std::min(n, b0 + forced_pairs);
    uint64_t b1 = b0 + 1;
    while (b1 < n && cost_first[b1 + 1] - cost_first[b0] <= room) ++b1;
    return b1;
}
inline unsigned walk_grid(uint64_t n_pairs, unsigned cus) { return (unsigned)std::max<uint64_t>(1, std::min<uint64_t>(n_pairs, 64ull * cus)); }     // a wave a walk

// ---- the device's walk on the host: the sorted ( hash ) -> ( entry, pos ) segment, verification, the live list.  Returns false where the
// live list outgrows max_live (the caller takes the host route), and never writes past `bound` bases.
struct Entry { const uint8_t* packed; const uint8_t* quals /* lowered */; uint32_t len; bool rc; };
struct TableView { const uint64_t* hash; const uint64_t* val /* entry << 32 | pos */; uint64_t n; };
inline bool walk_device_order(const uint8_t* edge_packed, const Entry* ent, uint64_t n_ent, const TableView& T, uint32_t max_live, uint64_t bound,
                              uint8_t* placed, int32_t* start, uint8_t* EE, Rec* r, HostResult* counters)
{
    for (uint64_t i = 0; i < n_ent; ++i) { placed[i] = 0; start[i] = -1; }
    Key96 key = key_of_edge(edge_packed);
    for (uint32_t j = 0; j < KW; ++j) EE[j] = (uint8_t)base_at(edge_packed, j);
    uint64_t L = KW;
    std::vector<uint32_t> live;                    // the entries of the live list
    r->dup_steps = 0;
    for (uint64_t step = 0; step + KW <= bound; ++step) {                                        // counted: at most bound - 48 + 1 steps
        ++counters->steps;
        const uint64_t h = hash_of(key);
        const uint64_t lo = lower_bound64(T.hash, 0, T.n, h);
        auto verified = [&](uint64_t i) { const Entry& e = ent[T.val[i] >> 32]; return same_key(key_at(e.packed, e.len, e.rc, (uint32_t)T.val[i]), key); };
        bool dup = false;
        for (uint64_t i = lo; i < T.n && T.hash[i] == h; ++i) {
            if (!verified(i)) { ++counters->collisions; continue; }
            ++counters->verified;
            for (uint64_t j = i; j-- > lo && (T.val[j] >> 32) == (T.val[i] >> 32);) if (verified(j)) dup = true;
        }
        if (dup) ++r->dup_steps;
        else for (uint64_t i = lo; i < T.n && T.hash[i] == h; ++i) {
            if (!verified(i)) continue;
            const uint32_t e = (uint32_t)(T.val[i] >> 32), pos = (uint32_t)T.val[i];
            if (placed[e]) continue;
            placed[e] = 1; start[e] = (int32_t)((int64_t)L - KW - pos);
            if ((uint64_t)KW + pos < ent[e].len) { if (live.size() == max_live) return false; live.push_back(e); }
        }
        int32_t sum[4] = {0, 0, 0, 0};
        size_t w = 0;
        counters->live_sum += live.size(); counters->live_max = std::max<uint64_t>(counters->live_max, live.size());
        for (size_t i = 0; i < live.size(); ++i) {
            const Entry& e = ent[live[i]];
            const uint32_t p = (uint32_t)((int64_t)L - start[live[i]]);
            sum[oriented_base(e.packed, e.len, e.rc, p)] += oriented_qual(e.quals, e.len, e.rc, p);
            if (p + 1 < e.len) live[w++] = live[i];                                              // it retires when the walk passes its end
        }
        live.resize(w);
        uint32_t b;
        if (!decide(sum, &b)) break;
        if (L >= bound) return false;                                                            // (the bound says this cannot happen)
        EE[L++] = (uint8_t)b;
        key = roll(key, b);
    }
    r->nEE = (uint32_t)L;
    return true;
}

// The device version's order of work on the host, for the CPU test.  walks_per_batch 0 = what fits `room`; returns as walks_literal
inline int walks_plan(const Input& I, const int32_t* pairs, uint64_t n_pairs, uint64_t walks_per_batch, uint64_t room, uint64_t entries_cap, uint32_t max_live, HostResult* R)
{
    std::vector<uint32_t> side_rank;
    if (int rc = sides_of(I, pairs, n_pairs, &side_rank)) return rc;
    std::vector<uint64_t> n_ent(n_pairs);
    for (uint64_t pi = 0; pi < n_pairs; ++pi)
        n_ent[pi] = (I.read_first[side_rank[2 * pi] + 1] - I.read_first[side_rank[2 * pi]]) + (I.read_first[side_rank[2 * pi + 1] + 1] - I.read_first[side_rank[2 * pi + 1]]);
    const std::vector<uint64_t> efirst = dfk::prefix_sums(n_ent.data(), n_pairs);
    R->starts.assign(1, 0); R->ee_starts.assign(1, 0);
    for (uint64_t p0 = 0; p0 < n_pairs;) {
        const uint64_t p1 = next_range(efirst.data(), n_pairs, p0, entries_cap).e1, np = p1 - p0;
        ++R->ranges;
        std::vector<std::vector<uint64_t>> sets(np);
        std::vector<uint64_t> cost(np);
        for (uint64_t p = 0; p < np; ++p) {
            compose(I, side_rank[2 * (p0 + p)], side_rank[2 * (p0 + p) + 1], &sets[p]);
            if (sets[p].size() >= MAX_ENTRIES) return -4;
            cost[p] = BYTES_PER_PAIR;
            for (uint64_t w : sets[p]) cost[p] += entry_cost(I.read_len[w >> 1]);
        }
        const std::vector<uint64_t> cfirst = dfk::prefix_sums(cost.data(), np);
        for (uint64_t b0 = 0; b0 < np;) {
            const uint64_t b1 = next_batch(cfirst.data(), np, b0, room, pairs_per_batch(walks_per_batch)), nb = b1 - b0;
            ++R->batches;
            // the reads of the batch, each once, ascending; the gather; the decode and the lowering (a thread a read)
            std::vector<uint32_t> ids;
            for (uint64_t p = b0; p < b1; ++p) for (uint64_t w : sets[p]) ids.push_back((uint32_t)(w >> 1));
            std::sort(ids.begin(), ids.end()); ids.erase(std::unique(ids.begin(), ids.end()), ids.end());
            std::vector<uint64_t> b_at(ids.size() + 1, 0), q_at(ids.size() + 1, 0);
            for (size_t i = 0; i < ids.size(); ++i) { const uint32_t len = I.read_len[ids[i]]; b_at[i + 1] = b_at[i] + (len + 3) / 4; q_at[i + 1] = q_at[i] + len; }
            std::vector<uint8_t> bases(b_at.back()), quals(q_at.back());                          // (capacity == size: a read past the end is the sanitizer's to see)
            for (size_t i = 0; i < ids.size(); ++i) {
                std::copy(I.read_packed + I.read_off[ids[i]], I.read_packed + I.read_off[ids[i]] + (b_at[i + 1] - b_at[i]), bases.begin() + b_at[i]);
                if (!dfk_cons::decode_quals(I.pq, I.pq_off[ids[i]], I.pq_off[ids[i] + 1], quals.data() + q_at[i], I.read_len[ids[i]])) return -3;
                lower_read(bases.data() + b_at[i], I.read_len[ids[i]], quals.data() + q_at[i]);
            }
            R->decoded += ids.size();
            // the entries of the batch's pairs
            std::vector<uint64_t> ent_first(nb + 1, 0);
            for (uint64_t p = 0; p < nb; ++p) ent_first[p + 1] = ent_first[p] + sets[b0 + p].size();
            const uint64_t ne = ent_first[nb];
            std::vector<Entry> ent(ne);
            std::vector<uint32_t> lens(ne);
            std::vector<uint64_t> kfirst(ne + 1, 0), bound(nb);
            for (uint64_t p = 0; p < nb; ++p) for (size_t i = 0; i < sets[b0 + p].size(); ++i) {
                const uint64_t w = sets[b0 + p][i], slot = dfk_cons::slot_of(ids.data(), ids.size(), (uint32_t)(w >> 1)), at = ent_first[p] + i;
                lens[at] = I.read_len[w >> 1];
                ent[at] = Entry{bases.data() + b_at[slot], quals.data() + q_at[slot], lens[at], false};
                kfirst[at + 1] = kfirst[at] + kmers_of_len(lens[at]);
            }
            for (uint64_t p = 0; p < nb; ++p) bound[p] = ee_bound(lens.data() + ent_first[p], ent_first[p + 1] - ent_first[p]);
            std::vector<Rec> recs(2 * nb);
            std::vector<std::vector<Loc>> locs(2 * nb);
            std::vector<std::vector<uint8_t>> ees(2 * nb);
            std::vector<uint8_t> go(nb, 1);
            for (uint32_t s = 0; s < 2; ++s) {
                // the table of the side: ( pair, hash ) -> ( entry, pos ), a stable sort
                for (uint64_t p = 0; p < nb; ++p) for (uint64_t at = ent_first[p]; at < ent_first[p + 1]; ++at) ent[at].rc = entry_rc((sets[b0 + p][at - ent_first[p]] & 1) != 0, s);
                struct Item { uint64_t pair, hash, val; };
                std::vector<Item> items(kfirst[ne]);
                for (uint64_t p = 0; p < nb; ++p) for (uint64_t at = ent_first[p]; at < ent_first[p + 1]; ++at) for (uint64_t i = kfirst[at]; i < kfirst[at + 1]; ++i)
                    items[i] = Item{p, hash_of(key_at(ent[at].packed, ent[at].len, ent[at].rc, (uint32_t)(i - kfirst[at]))), (at - ent_first[p]) << 32 | (i - kfirst[at])};
                std::stable_sort(items.begin(), items.end(), [](const Item& a, const Item& b) { return a.pair != b.pair ? a.pair < b.pair : a.hash < b.hash; });
                std::vector<uint64_t> hash(items.size() + 1, 0), val(items.size() + 1, 0);
                for (size_t i = 0; i < items.size(); ++i) { hash[i] = items[i].hash; val[i] = items[i].val; }
                // the walks (a wave a walk)
                for (uint64_t p = 0; p < nb; ++p) {
                    const uint64_t pi = p0 + b0 + p, k = side_rank[2 * pi + s], e0 = ent_first[p], n = ent_first[p + 1] - e0;
                    Rec& r = recs[2 * p + s];
                    r = Rec{go[p] ? (uint32_t)WALKED : (uint32_t)NOT_WALKED, (uint32_t)n, 0, 0, I.edge_len[k], 0, 0, 0};
                    if (go[p] && r.nE < (int32_t)KW) r.status = SHORT;
                    else if (go[p]) {
                        std::vector<uint8_t> placed(n + 1), EE(bound[p]);
                        std::vector<int32_t> start(n + 1);
                        const TableView T{hash.data() + kfirst[e0], val.data() + kfirst[e0], kfirst[e0 + n] - kfirst[e0]};
                        if (!walk_device_order(I.edge_store + I.edge_at[k], ent.data() + e0, n, T, max_live, bound[p], placed.data(), start.data(), EE.data(), &r, R)) {
                            // the host route: the literal form on this walk alone
                            ++R->host_route;
                            std::vector<basevector> by(n); std::vector<qualvector> qy(n);
                            for (uint64_t i = 0; i < n; ++i) {
                                const Entry& e = ent[e0 + i];
                                by[i].resize(e.len); qy[i].resize(e.len);
                                for (uint32_t j = 0; j < e.len; ++j) { by[i][j] = (uint8_t)oriented_base(e.packed, e.len, e.rc, j); qy[i][j] = oriented_qual(e.quals, e.len, e.rc, j); }
                            }
                            Walk W;
                            stack_walk(edge_bases(I, k), by, qy, &W);
                            r.nEE = (uint32_t)W.EE.size(); r.dup_steps = W.dup_steps;
                            EE = W.EE; placed = W.placed; start.assign(W.start.begin(), W.start.end());
                        }
                        finish_side(sets[b0 + p], lens.data() + e0, s, placed.data(), start.data(), &r, &locs[2 * p + s]);
                        ees[2 * p + s].assign(EE.begin(), EE.begin() + r.nEE);
                    }
                    if (!r.placed) go[p] = 0;
                }
            }
            for (uint64_t q = 0; q < 2 * nb; ++q) append_walk(R, recs[q], locs[q], ees[q].data());
            b0 = b1;
        }
        p0 = p1;
    }
    return 0;
}

// ---- the file's fixed parts
constexpr const char* MAGIC = "DFKSWLK1";
inline uint64_t ee_starts_at(uint64_t n) { return 16 + 8 * (n + 1); }
inline uint64_t recs_at(uint64_t n) { return ee_starts_at(n) + 8 * (n + 1); }
inline uint64_t locs_at(uint64_t n) { return recs_at(n) + 32 * n; }
inline uint64_t bases_at(uint64_t n, uint64_t n_locs) { return locs_at(n) + 16 * n_locs; }
inline uint64_t packed_bytes(uint64_t n_bases) { return ((n_bases + 3) / 4 + 7) & ~7ull; }
inline uint64_t file_size(uint64_t n, uint64_t n_locs, uint64_t n_bases) { return bases_at(n, n_locs) + packed_bytes(n_bases); }
inline std::vector<uint8_t> pack_ee(const std::vector<uint8_t>& ee)
{
    std::vector<uint8_t> out(packed_bytes(ee.size()), 0);
    for (size_t i = 0; i < ee.size(); ++i) out[i >> 2] |= (uint8_t)(ee[i] << (2 * (i & 3)));
    return out;
}

} // namespace dfk_walks
