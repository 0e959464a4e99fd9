// superplus_amd/csrc/dfk_partners_kernels.h -- CloseGap2's search for unplaced partners (dfk_partners.h) on the device (gfx950,
// wave64): the forward parts of the ranks, the queries of a range of sides (flag, scan, emit), the table of a range of ranks
// (entries, stable radix sorts of a permutation, the sorted keys and positions), the search of a batch of queries a wave a query,
// the compaction of the kept.  No LDS tables, no MFMA: 2-bit windows and binary searches, bound by the latency of dependent loads.
//
// The cut (dfk_partners::cut32), the searches and the folds are the header's own functions, which the CPU test runs too.  A cut
// loads bytes l >> 2 .. (l + 31) >> 2 of its sequence one by one -- a read or an edge may start at any byte and the last of a
// buffer ends with the allocation, so no wider load is safe without slack -- and every caller holds l + 32 <= the bases.
//
// Nothing that reaches a file depends on the order in which atomics arrive: every place in an output comes from an exclusive scan
// or a stable sort; the two atomics add integers (queries with a hit, queries with several positions).
#pragma once
#include "dfk_closer_kernels.h"   // k_cl_iota, k_cl_gather
#include "dfk_partners.h"

namespace dfk {

// ---- the forward part of every rank: its leading records with fw true
__global__ void __launch_bounds__(256)
k_pt_forward(const uint64_t* __restrict__ loc_first, const uint64_t* __restrict__ locs, uint64_t n_ce, uint64_t* __restrict__ fw_n)
{
    for (uint64_t k = (uint64_t)blockIdx.x * 256 + threadIdx.x; k < n_ce; k += (uint64_t)gridDim.x * 256)
        fw_n[k] = dfk_partners::forward_count(locs, loc_first[k], loc_first[k + 1]);
}

// ---- the queries of the sides [q0, q0 + n_sides): an item is a forward record of a side's rank
struct PtSides {
    const uint32_t* side_rank;        // [all sides]
    const uint64_t* item_first;       // [n_sides + 1], of this range
    const uint64_t* loc_first; const uint64_t* locs; const uint64_t* fw_n;
    uint64_t q0, n_sides, n_items;
};
// the record of item i, its side, and whether it is a query: the head of a run of equal ids whose mate is not forward on the other rank
__device__ __forceinline__ bool pt_item(const PtSides& S, uint64_t i, uint64_t* q, uint64_t* id1)
{
    const uint64_t s = dfk_partners::owner_of(S.item_first, S.n_sides, i);
    *q = S.q0 + s;
    const uint64_t k = S.side_rank[*q], ko = S.side_rank[*q ^ 1], lo = S.loc_first[k], r = lo + (i - S.item_first[s]);
    *id1 = dfk_partners::loc_id(S.locs, r);
    if (r != lo && dfk_partners::loc_id(S.locs, r - 1) == *id1) return false;
    return !dfk_partners::has_id(S.locs, S.loc_first[ko], S.loc_first[ko] + S.fw_n[ko], *id1 ^ 1);
}
__global__ void __launch_bounds__(256)
k_pt_flag(PtSides S, uint64_t* __restrict__ flags /* [n_items + 1], 0 behind the last */)
{
    for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i <= S.n_items; i += (uint64_t)gridDim.x * 256) {
        uint64_t q, id1;
        flags[i] = i < S.n_items && pt_item(S, i, &q, &id1) ? 1u : 0u;
    }
}
__global__ void __launch_bounds__(256)
k_pt_emit(PtSides S, const uint64_t* __restrict__ flags, const uint64_t* __restrict__ place /* exclusive scan of flags */, uint32_t* __restrict__ q_side, uint32_t* __restrict__ q_id)
{
    for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < S.n_items; i += (uint64_t)gridDim.x * 256) {
        if (!flags[i]) continue;
        uint64_t q, id1;
        (void)pt_item(S, i, &q, &id1);
        q_side[place[i]] = (uint32_t)q; q_id[place[i]] = (uint32_t)(id1 ^ 1);
    }
}

// ---- the table of a range of ranks: entry i belongs to the anchor a with ent_first[a] <= i < ent_first[a + 1], l = i - ent_first[a]
struct PtAnchors {
    const uint64_t* ent_first;        // [n_anchors + 1], of this range
    const uint64_t* edge_at;          // [n_anchors] where the anchor's edge starts in the store, bytes
    const int32_t* add; const uint32_t* rank;      // [n_anchors] add; the rank of e' relative to the range
    uint64_t n_anchors, n_entries;
};
__global__ void __launch_bounds__(256)
k_pt_entries(PtAnchors A, const uint8_t* __restrict__ store, uint32_t* __restrict__ key_lo, uint32_t* __restrict__ key_hi, uint32_t* __restrict__ rank, int32_t* __restrict__ pos)
{
    for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < A.n_entries; i += (uint64_t)gridDim.x * 256) {
        const uint64_t a = dfk_partners::owner_of(A.ent_first, A.n_anchors, i);
        const uint32_t l = (uint32_t)(i - A.ent_first[a]);
        const uint64_t x = dfk_partners::cut32(store + A.edge_at[a], l);       // (l + 32 <= the edge's bases: ent_first counts positions())
        key_lo[i] = (uint32_t)x; key_hi[i] = (uint32_t)(x >> 32); rank[i] = A.rank[a]; pos[i] = dfk_partners::entry_pos(A.add[a], l);
    }
}
// the sorted table: the keys whole and the positions, by the permutation the sorts carried (one word behind the last, never read as a hit)
__global__ void __launch_bounds__(256)
k_pt_sorted(const uint32_t* __restrict__ perm, const uint32_t* __restrict__ key_lo, const uint32_t* __restrict__ key_hi, const int32_t* __restrict__ pos, uint64_t n,
            uint64_t* __restrict__ keys, int32_t* __restrict__ spos)
{
    for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (uint64_t)gridDim.x * 256) {
        const uint32_t p = perm[i];
        keys[i] = (uint64_t)key_lo[p] | ((uint64_t)key_hi[p] << 32); spos[i] = pos[p];
    }
}

// ---- the search: a wave a query.  Query w of the batch: the read's bytes at bases + q_off[w], q_len[w] bases, against the slice
// of rank side_rank[q_side[w] ^ 1] -- [t_first[k - k0], t_first[k - k0 + 1]) of the sorted table.
struct PtBatch {
    const uint8_t* bases; const uint64_t* q_off; const uint32_t* q_len; const uint32_t* q_side; uint64_t n;
    const uint32_t* side_rank; uint32_t k0, k1;
    const uint64_t* t_first; const uint64_t* keys; const int32_t* pos;
};
__global__ void __launch_bounds__(256)
k_pt_search(PtBatch B, uint32_t* __restrict__ status, int32_t* __restrict__ found, uint64_t* __restrict__ kept /* [n + 1], 0 behind the last */, unsigned long long* __restrict__ ctr /* any hit, several */)
{
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t waves = (uint64_t)gridDim.x * 4;
    for (uint64_t w = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6); w <= B.n; w += waves) {
        if (w == B.n) { if (lane == 0) kept[w] = 0; continue; }
        const uint32_t ko = B.side_rank[B.q_side[w] ^ 1u];
        dfk_partners::Fold f{0, 0, 0u};
        if (ko >= B.k0 && ko < B.k1)
            f = dfk_partners::search_lane(B.bases + B.q_off[w], B.q_len[w], lane, B.keys, B.pos, B.t_first[ko - B.k0], B.t_first[ko - B.k0 + 1]);
        for (int d = 32; d >= 1; d >>= 1) {                                  // the wave's fold: every lane ends with all 64
            dfk_partners::Fold o;
            o.lo = __shfl_xor(f.lo, d, 64); o.hi = __shfl_xor(f.hi, d, 64); o.hit = __shfl_xor(f.hit, d, 64);
            f = dfk_partners::fold_join(f, o);
        }
        if (lane == 0) {
            const uint32_t st = dfk_partners::status_of(f);
            status[w] = st; found[w] = f.lo; kept[w] = st == dfk_partners::Q_KEPT ? 1u : 0u;
            if (st != dfk_partners::Q_NONE) atomicAdd(&ctr[0], 1ull);
            if (st == dfk_partners::Q_MULTI) atomicAdd(&ctr[1], 1ull);
        }
    }
}
// the kept queries of a batch in query order: ( query of the batch, pos )
__global__ void __launch_bounds__(256)
k_pt_compact(const uint64_t* __restrict__ kept, const uint64_t* __restrict__ place /* exclusive scan of kept */, const int32_t* __restrict__ found, uint64_t n, uint32_t* __restrict__ out /* [2 * kept] */)
{
    for (uint64_t w = (uint64_t)blockIdx.x * 256 + threadIdx.x; w < n; w += (uint64_t)gridDim.x * 256) {
        if (!kept[w]) continue;
        out[2 * place[w]] = (uint32_t)w; out[2 * place[w] + 1] = (uint32_t)found[w];
    }
}

} // namespace dfk
