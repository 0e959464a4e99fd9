// superplus_amd/csrc/dfk_walks_kernels.h -- Stackster's stack walks (dfk_walks.h) on the device (gfx950, wave64): the lowering of a
// batch's reads (a thread a read), the 48-mers of a side's oriented entries with their hashes (a thread a 48-mer), the sorted table
// written out by the permutation the radix sorts carried, the walk (a WAVE a walk: one workgroup of 64 lanes), the walked sequences
// brought together.  No MFMA, no floating point: byte loads, integer sums.
//
// The orientation, the lowering, the key and its roll, the hash and the step's decision are the header's own functions, which the CPU
// test runs too.  A base is loaded as the byte that holds it and a quality as its byte: a read may start at any byte and the last of
// a buffer ends with the allocation.
//
// k_wk_walk keeps its walk's state in registers and LDS: the rolling 96-bit key, |EE|, the live list (start, len | rc << 31, where the
// read's bases and qualities begin: 16 bytes an entry, DFK_WALK_MAX_LIVE entries).  Nothing in the step loop is an atomic; the loop is
// counted by the header's bound; the workgroup is one wave, so its barriers are the wave's own.  Every index into the table stays
// inside the walk's segment [t0, t1), every entry inside [e0, e0 + n), every write to EE below the walk's bound.
#pragma once
#include "dfk_cons_kernels.h"
#include "dfk_walks.h"

namespace dfk {

// the batch: pairs [0, n_pairs), their entries, the reads' slots
struct WkBatch {
    uint64_t n_pairs, n_ent;
    const uint64_t* ent_first;         // [n_pairs + 1]
    const uint32_t* ent_slot;          // [n_ent] the read's slot in the batch | fw << 31
    const uint64_t* kfirst;            // [n_ent + 1] the first 48-mer of every entry: the same on both sides
    const uint64_t* b_at; const uint64_t* q_at;      // [slots + 1] where a slot's bases and qualities start; q_at[s + 1] - q_at[s] is the read's length
    const uint8_t* bases; const uint8_t* quals;      // quals: decoded and lowered
};
struct WkEntry { const uint8_t* packed; const uint8_t* quals; uint32_t len; bool rc; uint32_t b_off, q_off; };
__device__ __forceinline__ WkEntry wk_entry(const WkBatch& B, uint64_t at, uint32_t side)
{
    const uint32_t w = B.ent_slot[at], slot = w & 0x7FFFFFFFu;
    const uint64_t b = B.b_at[slot], q = B.q_at[slot];
    return WkEntry{B.bases + b, B.quals + q, (uint32_t)(B.q_at[slot + 1] - q), dfk_walks::entry_rc((w >> 31) != 0, side), (uint32_t)b, (uint32_t)q};
}

// ---- the lowering: a thread a read of the batch, in place, once whatever the sides
__global__ void __launch_bounds__(256)
k_wk_lower(const uint8_t* __restrict__ bases, const uint64_t* __restrict__ b_at, const uint64_t* __restrict__ q_at, uint64_t n, uint8_t* __restrict__ quals)
{
    for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (uint64_t)gridDim.x * 256)
        dfk_walks::lower_read(bases + b_at[i], (uint32_t)(q_at[i + 1] - q_at[i]), quals + q_at[i]);
}

// ---- the 48-mers of a side: item i is 48-mer i - kfirst[at] of entry `at`
__global__ void __launch_bounds__(256)
k_wk_kmers(WkBatch B, uint32_t side, uint64_t mask, uint64_t n_items, uint32_t* __restrict__ key_lo, uint32_t* __restrict__ key_hi, uint32_t* __restrict__ pair, uint32_t* __restrict__ ent, uint32_t* __restrict__ pos)
{
    for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < n_items; i += (uint64_t)gridDim.x * 256) {
        const uint64_t at = dfk_walks::owner_of(B.kfirst, B.n_ent, i), p = dfk_walks::owner_of(B.ent_first, B.n_pairs, at);
        const WkEntry e = wk_entry(B, at, side);
        const uint32_t l = (uint32_t)(i - B.kfirst[at]);                       // (l + 48 <= len: kfirst counts kmers_of_len())
        const uint64_t h = dfk_walks::hash_of(dfk_walks::key_at(e.packed, e.len, e.rc, l), mask);
        key_lo[i] = (uint32_t)h; key_hi[i] = (uint32_t)(h >> 32); pair[i] = (uint32_t)p; ent[i] = (uint32_t)(at - B.ent_first[p]); pos[i] = l;
    }
}
// the sorted table: the hashes whole and ( entry << 32 | pos ), by the permutation the sorts carried
__global__ void __launch_bounds__(256)
k_wk_sorted(const uint32_t* __restrict__ perm, const uint32_t* __restrict__ key_lo, const uint32_t* __restrict__ key_hi, const uint32_t* __restrict__ ent, const uint32_t* __restrict__ pos, uint64_t n,
            uint64_t* __restrict__ hash, uint64_t* __restrict__ val)
{
    for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (uint64_t)gridDim.x * 256) {
        const uint32_t j = perm[i];
        hash[i] = (uint64_t)key_lo[j] | ((uint64_t)key_hi[j] << 32); val[i] = ((uint64_t)ent[j] << 32) | pos[j];
    }
}

// ---- the walk
struct WkOut { uint32_t state /* 0 done, 1 the live list outgrew its room, 2 the bound was met (never) */, nEE, dup_steps, placed; int32_t M; uint32_t live_max; uint64_t steps, live_sum, verified, collisions; };
static_assert(sizeof(WkOut) == 56, "a walk's words");
struct WkWalks {
    uint32_t side, max_live; uint64_t mask;
    const uint8_t* go;                 // [n_pairs] walk this pair's side
    const uint8_t* edges; const uint64_t* edge_at;   // [n_pairs] where O(es[side]) starts (48 bases at least where go)
    const uint64_t* hash; const uint64_t* val;       // the sorted table of this side
    const uint64_t* ee_first;          // [n_pairs + 1] the walk's room in `ee`: its bound
};
__device__ __forceinline__ int32_t wk_wave_sum(int32_t v) { for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d, 64); return v; }

__global__ void __launch_bounds__(64)
k_wk_walk(WkBatch B, WkWalks W, uint8_t* __restrict__ placed /* [n_ent] */, int32_t* __restrict__ start /* [n_ent] */, uint8_t* __restrict__ ee, WkOut* __restrict__ out /* [n_pairs] */)
{
    using namespace dfk_walks;
    __shared__ int32_t l_start[MAX_LIVE];
    __shared__ uint32_t l_len[MAX_LIVE], l_b[MAX_LIVE], l_q[MAX_LIVE];
    const uint32_t lane = threadIdx.x;
    const uint64_t below = lane ? (~0ull >> (64 - lane)) : 0ull;               // the lanes before this one
    for (uint64_t p = blockIdx.x; p < B.n_pairs; p += gridDim.x) {
        if (!W.go[p]) continue;
        const uint64_t e0 = B.ent_first[p], n = B.ent_first[p + 1] - e0, t0 = B.kfirst[e0], t1 = B.kfirst[e0 + n];
        const uint64_t bound = W.ee_first[p + 1] - W.ee_first[p];
        uint8_t* EE = ee + W.ee_first[p];
        const uint8_t* edge = W.edges + W.edge_at[p];
        for (uint64_t i = lane; i < n; i += 64) { placed[e0 + i] = 0; start[e0 + i] = -1; }
        if (lane < KW) EE[lane] = (uint8_t)base_at(edge, lane);                // (bound >= 48)
        Key96 key = key_of_edge(edge);
        uint64_t L = KW, steps = 0, live_sum = 0, verified = 0, collisions = 0;
        uint32_t n_live = 0, dup_steps = 0, state = 0, live_max = 0;
        __syncthreads();                                                       // placed and start are cleared before any lane places
        for (uint64_t step = 0; step + KW <= bound; ++step) {                   // counted: at most bound - 48 + 1 steps
            ++steps;
            const uint64_t h = hash_of(key, W.mask);
            const uint64_t lo = lower_bound64(W.hash, t0, t1, h);
            // the hits, a lane a hit: verified against the read; a duplicate where an entry has two verified hits
            bool dup = false, ver0 = false, one_chunk = false;                   // ver0: this lane's hit of the first chunk is verified; one_chunk: the run ends in it
            for (uint64_t c0 = lo; c0 < t1; c0 += 64) {
                const uint64_t i = c0 + lane;
                const bool hit = i < t1 && W.hash[i] == h;
                bool ver = false, mine = false;
                if (hit) {
                    const uint64_t v = W.val[i];
                    const WkEntry e = wk_entry(B, e0 + (v >> 32), W.side);
                    ver = same_key(key_at(e.packed, e.len, e.rc, (uint32_t)v), key);
                    if (ver) for (uint64_t j = i; j-- > lo && (W.val[j] >> 32) == (v >> 32);)
                        if (same_key(key_at(e.packed, e.len, e.rc, (uint32_t)W.val[j]), key)) { mine = true; break; }
                }
                const uint64_t hits = __ballot(hit);
                verified += __popcll(__ballot(ver)); collisions += __popcll(hits) - __popcll(__ballot(ver));
                if (__ballot(mine)) dup = true;
                if (c0 == lo) { ver0 = ver; one_chunk = hits != ~0ull; }
                if (hits != ~0ull) break;                                      // the run of this hash ends in this chunk
            }
            if (dup) ++dup_steps;
            else for (uint64_t c0 = lo; c0 < t1 && !state; c0 += 64) {
                const uint64_t i = c0 + lane;
                const bool hit = i < t1 && W.hash[i] == h;
                bool join = false;
                int32_t st = 0; uint32_t lr = 0, bo = 0, qo = 0;
                if (hit) {
                    const uint64_t v = W.val[i];
                    const uint32_t pos = (uint32_t)v;
                    const WkEntry e = wk_entry(B, e0 + (v >> 32), W.side);
                    const bool ver = one_chunk ? ver0 : same_key(key_at(e.packed, e.len, e.rc, pos), key);      // (the usual case: what the pass above found)
                    if (ver && !placed[e0 + (v >> 32)]) {       // (an entry has one verified hit here: no two lanes place it)
                        st = (int32_t)((int64_t)L - KW - pos);
                        placed[e0 + (v >> 32)] = 1; start[e0 + (v >> 32)] = st;
                        join = (uint64_t)KW + pos < e.len;                     // it covers the current column
                        lr = e.len | (e.rc ? 0x80000000u : 0u); bo = e.b_off; qo = e.q_off;
                    }
                }
                const uint64_t joins = __ballot(join);
                const uint32_t nj = (uint32_t)__popcll(joins);
                if (n_live + nj > W.max_live) { state = 1; break; }            // (uniform: the host takes this walk)
                if (join) { const uint32_t at = n_live + (uint32_t)__popcll(joins & below); l_start[at] = st; l_len[at] = lr; l_b[at] = bo; l_q[at] = qo; }
                n_live += nj;
                if (__ballot(hit) != ~0ull) break;
            }
            if (state) break;
            __syncthreads();                                                   // the list as the placing lanes left it
            // the sums over the live list, a lane an entry; an entry retires when the walk passes its end
            live_sum += n_live; live_max = n_live > live_max ? n_live : live_max;
            int32_t s0 = 0, s1 = 0, s2 = 0, s3 = 0;
            uint32_t w = 0;
            for (uint32_t c0 = 0; c0 < n_live; c0 += 64) {
                const uint32_t i = c0 + lane;
                const bool act = i < n_live;
                bool keep = false;
                int32_t st = 0; uint32_t lr = 0, bo = 0, qo = 0;
                if (act) {
                    st = l_start[i]; lr = l_len[i]; bo = l_b[i]; qo = l_q[i];
                    const uint32_t len = lr & 0x7FFFFFFFu, pcol = (uint32_t)((int64_t)L - st);       // 48 <= pcol < len
                    const bool rc = (lr >> 31) != 0;
                    const uint32_t b = oriented_base(B.bases + bo, len, rc, pcol);
                    const int32_t q = oriented_qual(B.quals + qo, len, rc, pcol);
                    s0 += b == 0 ? q : 0; s1 += b == 1 ? q : 0; s2 += b == 2 ? q : 0; s3 += b == 3 ? q : 0;
                    keep = pcol + 1 < len;
                }
                __syncthreads();                                               // every lane holds its entry before any is overwritten
                const uint64_t keeps = __ballot(keep);
                if (keep) { const uint32_t at = w + (uint32_t)__popcll(keeps & below); l_start[at] = st; l_len[at] = lr; l_b[at] = bo; l_q[at] = qo; }      // at <= i
                w += (uint32_t)__popcll(keeps);
                __syncthreads();
            }
            n_live = w;
            const int32_t sum[4] = {wk_wave_sum(s0), wk_wave_sum(s1), wk_wave_sum(s2), wk_wave_sum(s3)};
            uint32_t b;
            if (!decide(sum, &b)) break;
            if (L >= bound) { state = 2; break; }                              // (the bound says this cannot happen)
            if (lane == 0) EE[L] = (uint8_t)b;
            ++L;
            key = roll(key, b);
        }
        __syncthreads();
        // placed, M (:409-414)
        int32_t M = 0, cnt = 0;
        for (uint64_t i = lane; i < n; i += 64)
            if (placed[e0 + i]) { const int32_t end = start[e0 + i] + (int32_t)wk_entry(B, e0 + i, W.side).len; M = end > M ? end : M; ++cnt; }
        for (int d = 32; d >= 1; d >>= 1) { const int32_t o = __shfl_xor(M, d, 64); M = o > M ? o : M; }
        cnt = wk_wave_sum(cnt);
        if (lane == 0) out[p] = WkOut{state, (uint32_t)L, dup_steps, (uint32_t)cnt, M, live_max, steps, live_sum, verified, collisions};
        __syncthreads();
    }
}

// ---- the walked sequences brought together: base i of the batch's output is base i - out_first[w] of walk w
__global__ void __launch_bounds__(256)
k_wk_collect(const uint8_t* __restrict__ ee, const uint64_t* __restrict__ ee_first, const uint64_t* __restrict__ out_first /* [n_pairs + 1] */, uint64_t n_pairs, uint64_t n_out, uint8_t* __restrict__ out)
{
    for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < n_out; i += (uint64_t)gridDim.x * 256) {
        const uint64_t w = dfk_walks::owner_of(out_first, n_pairs, i);
        out[i] = ee[ee_first[w] + (i - out_first[w])];
    }
}

} // namespace dfk
