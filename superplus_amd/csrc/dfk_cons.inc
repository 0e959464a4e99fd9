// superplus_amd/csrc/dfk_cons.inc -- CloseGap2's stack consensus per pair and side (10X/Closomatic.cc:587-640, ReadStack.cc's
// Trim, Reverse, Consensus1) and the file a.close.cons, included by dfk.hip.
//
// The rule, the cell, the plan and the file's layout: dfk_cons.h.  The kernels: dfk_cons_kernels.h.  Here: cons_build() -- a range
// of stacks at a time the dimensions and the live rows, under it the batches of stacks: the reads the batch's live rows name, each
// once, gathered on the host (packed bases and PQVec bytes) and sent up, decoded, the consensus a workgroup a stack, the bases and
// the two counts a stack coming back -- and cons_write().  Everything on the device comes from the arena and goes back before build
// returns.  The reads' lengths go up whole (four bytes a read): the dimensions need the length of every row's read.  The steps up
// to the decode are functions of their own (cn_sides, cn_tables_up, cn_range_live, cn_batch_reads): closures_build
// (dfk_closures.inc) walks the same stacks and calls them too.
#include "dfk_cons_kernels.h"

namespace {

struct ConsResult {
    std::vector<uint64_t> starts;                 // [2 * n_pairs + 1], in bases
    std::vector<dfk_cons::Dim> dims;              // [2 * n_pairs]
    std::vector<uint8_t> bases;                   // padded with zero bytes to a multiple of 8
    uint64_t n_bases = 0;
    uint64_t stats[DFK_CONS_WORDS] = {};
    uint64_t serial = 0;                          // which build made it: dfk_offsets_build notes it, dfk_closures_build asks for the same
    std::vector<int32_t> pairs;                   // dfk_cons_build: the pairs it was made for
};
uint64_t cons_next_serial() { static std::atomic<uint64_t> n{0}; return ++n; }
void cons_result_free(ConsResult* r) { delete r; }

struct ConsSource {
    uint64_t n_edges; const int32_t* inv;
    uint64_t n_ce; const uint64_t* ce; const int32_t* rank_ne /* [n_ce] hb.Bases of the closer edges */; const uint64_t* loc_first; const uint64_t* locs;
    uint64_t n_parts /* elements: 2 * the pairs they were made for */; const uint64_t* part_first; const uint64_t* parts;
    const PartnerReads* reads; const uint8_t* pq; const uint64_t* pq_off;
};
uint64_t cons_pq_at(const uint64_t* pq_off, uint64_t r) { uint64_t x; memcpy(&x, (const char*)pq_off + 8 * r, 8); return x; }     // (the table may sit at any address)

// ---- the steps cons_build and closures_build (dfk_closures.inc) share: the sides of the pairs, the tables on the device, the
// dimensions and live rows of a range of stacks, the reads of a batch of stacks gathered and decoded
struct CnSides { std::vector<uint32_t> rank; std::vector<int32_t> ne; std::vector<uint8_t> rev; std::vector<uint64_t> n_rows, rfirst; };
struct CnTimes { float ms_dims = 0, ms_decode = 0; double s_copy = 0; };
struct CnTables { DevBuf loc_first, locs, part_first, parts, side_rank, side_ne, side_rev, len, bad; };
struct CnRange {
    uint64_t q0 = 0, ns = 0, n_items = 0, got = 0;
    DevBuf rel, M, flags, place, lfirst, l_id, l_pos, l_len;
    std::vector<long long> h_M;                   // [ns]
    std::vector<uint64_t> h_lfirst, cost;         // [ns + 1] into the range's live rows; [ns] what a stack costs a batch
    std::vector<uint32_t> h_id, h_len;            // the live rows' reads and lengths (| fw << 31)
};
struct CnReads { uint64_t live0 = 0, nl = 0, n_ids = 0; DevBuf bases, pq, quals, bat, qat, pat, slot; };

int cn_up(dfk_ctx* c, DevBuf& d, const void* h, uint64_t bytes, const char* what)
{
    if (int r = c->alloc(d, std::max<uint64_t>(8, bytes), what, Place::Low)) return r;
    return bytes ? upload(c, d.p, h, bytes) : 0;
}

// per stack q = 2 pi + ei: the rank of es[ei], hb.Bases of it, whether Reverse applies (:638), its rows; what the tables name checked
int cn_sides(const ConsSource& S, const int32_t* pairs, uint64_t n_pairs, CnSides* X)
{
    using namespace dfk_cons;
    const uint64_t N = S.reads->n, n_ce = S.n_ce, n_stacks = 2 * n_pairs, n_locs = S.loc_first[n_ce], n_parts = S.part_first[S.n_parts];
    if (S.n_parts != n_stacks) return fail(DFK_E_ARG, "cons: %llu pairs given, the partners were made for %llu", (unsigned long long)n_pairs, (unsigned long long)(S.n_parts / 2));
    if (N > (1ull << 31) || n_pairs >= (1ull << 30)) return fail(DFK_E_ARG, "%llu reads, %llu pairs: a row keeps its read in 32 bits", (unsigned long long)N, (unsigned long long)n_pairs);
    for (uint64_t i = 0; i < 2 * n_pairs; ++i)
        if (pairs[i] < 0 || (uint64_t)pairs[i] >= S.n_edges) return fail(DFK_E_ARG, "pair %llu names edge %d: the graph has %llu", (unsigned long long)(i / 2), pairs[i], (unsigned long long)S.n_edges);
    X->rank.assign(std::max<uint64_t>(1, n_stacks), 0); X->ne.assign(std::max<uint64_t>(1, n_stacks), 0); X->rev.assign(std::max<uint64_t>(1, n_stacks), 0);
    for (uint64_t pi = 0; pi < n_pairs; ++pi) {
        const uint64_t es[2] = {(uint64_t)pairs[2 * pi], (uint64_t)S.inv[pairs[2 * pi + 1]]};
        for (int ei = 0; ei < 2; ++ei) {
            const uint64_t k = rank_in(S.ce, n_ce, es[ei]);
            if (k == n_ce) return fail(DFK_E_ARG, "pair %llu: edge %llu is not among the closer edges: the closer sets were built for other pairs", (unsigned long long)pi, (unsigned long long)es[ei]);
            X->rank[2 * pi + ei] = (uint32_t)k; X->ne[2 * pi + ei] = S.rank_ne[k]; X->rev[2 * pi + ei] = es[ei] == es[1];       // :638: e == inv[e2]
        }
    }
    for (uint64_t j = 0; j < n_parts; ++j) if (S.parts[2 * j] >= N) return fail(DFK_E_ARG, "a partner record names read %llu of %llu", (unsigned long long)S.parts[2 * j], (unsigned long long)N);
    if (n_locs + n_parts && !N) return fail(DFK_E_ARG, "rows, and no reads");
    X->n_rows.assign(n_stacks, 0);
    for (uint64_t q = 0; q < n_stacks; ++q) X->n_rows[q] = (S.loc_first[X->rank[q] + 1] - S.loc_first[X->rank[q]]) + (S.part_first[(q ^ 1) + 1] - S.part_first[q ^ 1]);
    X->rfirst = prefix_sums(X->n_rows.data(), n_stacks);
    return 0;
}

// the tables, the sides and the reads' lengths sent up; the count of streams that did not decode zeroed
int cn_tables_up(dfk_ctx* c, const ConsSource& S, const CnSides& X, uint64_t n_stacks, CnTables* T)
{
    int rc;
    const uint64_t N = S.reads->n, n_ce = S.n_ce, n_locs = S.loc_first[n_ce], n_parts = S.part_first[S.n_parts];
    if ((rc = cn_up(c, T->loc_first, S.loc_first, (n_ce + 1) * 8, "locs starts")) || (rc = cn_up(c, T->locs, S.locs, n_locs * 16, "locs records")) ||
        (rc = cn_up(c, T->part_first, S.part_first, (n_stacks + 1) * 8, "partners starts")) || (rc = cn_up(c, T->parts, S.parts, n_parts * 16, "partners records")) ||
        (rc = cn_up(c, T->side_rank, X.rank.data(), n_stacks * 4, "ranks of the stacks")) || (rc = cn_up(c, T->side_ne, X.ne.data(), n_stacks * 4, "bases of the stacks' edges")) ||
        (rc = cn_up(c, T->side_rev, X.rev.data(), n_stacks, "stacks reversed")) || (rc = c->alloc(T->len, std::max<uint64_t>(8, N * 4), "read lengths", Place::Low)) ||
        (rc = c->alloc(T->bad, 8, "streams that did not decode", Place::Low))) return rc;
    {   // the lengths: through host_read, a piece at a time (they may lie in a hinted file range)
        std::vector<uint32_t> piece(std::min<uint64_t>(std::max<uint64_t>(1, N), 1ull << 22));
        for (uint64_t r0 = 0; r0 < N; r0 += piece.size()) {
            const uint64_t n = std::min<uint64_t>(piece.size(), N - r0);
            if ((rc = host_read(c, piece.data(), S.reads->len + r0, n * 4)) || (rc = upload(c, (char*)T->len.p + 4 * r0, piece.data(), n * 4))) return rc;
        }
    }
    HIP_TRY(hipMemsetAsync(T->bad.p, 0, 8, c->stream));
    return 0;
}

// the stacks [q0, q1) with their n_items rows: the dimensions (a wave a stack), the live rows by flag, scan and emit; M, the live
// rows' starts, reads and lengths back, checked; what every stack costs a batch
int cn_range_live(dfk_ctx* c, const ConsSource& S, const CnSides& X, const CnTables& T, uint64_t q0, uint64_t q1, uint64_t n_items, CnRange* G)
{
    using namespace dfk_cons;
    int rc;
    const unsigned cus = (unsigned)c->prop.multiProcessorCount;
    const uint64_t N = S.reads->n, ns = q1 - q0;
    G->q0 = q0; G->ns = ns; G->n_items = n_items;
    std::vector<uint64_t> rel(ns + 1);
    for (uint64_t s = 0; s <= ns; ++s) rel[s] = X.rfirst[q0 + s] - X.rfirst[q0];
    if ((rc = cn_up(c, G->rel, rel.data(), (ns + 1) * 8, "rows per stack")) || (rc = c->alloc(G->M, ns * 8, "stack widths", Place::Low)) || (rc = c->alloc(G->flags, (n_items + 1) * 8, "live flags", Place::Low)) ||
        (rc = c->alloc(G->place, (n_items + 1) * 8, "live places", Place::Low)) || (rc = c->alloc(G->lfirst, (ns + 1) * 8, "live rows per stack", Place::Low))) return rc;
    const CnStacks P{(const uint32_t*)T.side_rank.p, (const int32_t*)T.side_ne.p, (const uint64_t*)G->rel.p, (const uint64_t*)T.loc_first.p, (const uint64_t*)T.locs.p,
                     (const uint64_t*)T.part_first.p, (const uint64_t*)T.parts.p, (const uint32_t*)T.len.p, q0, ns, n_items};
    hipLaunchKernelGGL(k_cn_dims, dim3((unsigned)std::min<uint64_t>((ns + 3) / 4, 16ull * cus)), dim3(256), 0, c->stream, P, (long long*)G->M.p);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(k_cn_flag, dim3(grid_256(n_items + 1, cus)), dim3(256), 0, c->stream, P, (const long long*)G->M.p, (uint64_t*)G->flags.p);
    HIP_TRY(hipGetLastError());
    if ((rc = device_scan(c, (const uint64_t*)G->flags.p, (uint64_t*)G->place.p, n_items + 1))) return rc;
    hipLaunchKernelGGL(k_cn_live_first, dim3(grid_256(ns + 1, cus)), dim3(256), 0, c->stream, (const uint64_t*)G->rel.p, (const uint64_t*)G->place.p, ns, (uint64_t*)G->lfirst.p);
    HIP_TRY(hipGetLastError());
    G->h_M.assign(ns, 0); G->h_lfirst.assign(ns + 1, 0);
    HIP_TRY(hipMemcpyAsync(G->h_M.data(), G->M.p, ns * 8, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipMemcpyAsync(G->h_lfirst.data(), G->lfirst.p, (ns + 1) * 8, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    const std::vector<uint64_t>& lfirst = G->h_lfirst;
    const uint64_t got = G->got = lfirst[ns];
    if (got > n_items || lfirst[0] != 0) return fail(DFK_E_HIP, "cons: %llu live rows among %llu", (unsigned long long)got, (unsigned long long)n_items);
    G->h_id.assign(got, 0); G->h_len.assign(got, 0);
    if (got) {
        if ((rc = c->alloc(G->l_id, got * 4, "live rows' reads", Place::Low)) || (rc = c->alloc(G->l_pos, got * 4, "live rows' positions", Place::Low)) || (rc = c->alloc(G->l_len, got * 4, "live rows' lengths", Place::Low))) return rc;
        hipLaunchKernelGGL(k_cn_emit, dim3(grid_256(n_items, cus)), dim3(256), 0, c->stream, P, (const long long*)G->M.p, (const uint64_t*)G->flags.p, (const uint64_t*)G->place.p, (uint32_t*)G->l_id.p, (int32_t*)G->l_pos.p, (uint32_t*)G->l_len.p);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(G->h_id.data(), G->l_id.p, got * 4, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipMemcpyAsync(G->h_len.data(), G->l_len.p, got * 4, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
    }
    G->cost.assign(ns, 0);
    for (uint64_t s = 0; s < ns; ++s) {
        const long long M = G->h_M[s];
        if (M < 0 || M > 0x7FFFFFFFll || lfirst[s + 1] < lfirst[s] || lfirst[s + 1] - lfirst[s] > X.n_rows[q0 + s]) return fail(DFK_E_HIP, "cons: stack %llu is %lld columns wide with %llu live rows of %llu", (unsigned long long)(q0 + s), M, (unsigned long long)(lfirst[s + 1] - lfirst[s]), (unsigned long long)X.n_rows[q0 + s]);
        G->cost[s] = BYTES_PER_STACK;
        for (uint64_t l = lfirst[s]; l < lfirst[s + 1]; ++l) {
            if (G->h_id[l] >= N) return fail(DFK_E_HIP, "cons: a live row names read %u", G->h_id[l]);
            G->cost[s] += live_row_cost(G->h_len[l] & 0x7FFFFFFFu);
        }
    }
    return 0;
}

// the reads the live rows of the range's stacks [s0, s1) name, each once, ascending: gathered on the host through host_read, sent up
// with their starts and every live row's slot, decoded (a thread a read); a stream that does not hold len values refuses the call
int cn_batch_reads(dfk_ctx* c, const ConsSource& S, const CnTables& T, const CnRange& G, uint64_t s0, uint64_t s1, Timer& tm, CnTimes* times, CnReads* B)
{
    using namespace dfk_cons;
    int rc;
    const unsigned cus = (unsigned)c->prop.multiProcessorCount;
    const double t_g = wall_now();
    const uint64_t live0 = B->live0 = G.h_lfirst[s0], nl = B->nl = G.h_lfirst[s1] - live0;
    std::vector<uint32_t> ids(G.h_id.begin() + live0, G.h_id.begin() + live0 + nl);
    std::sort(ids.begin(), ids.end()); ids.erase(std::unique(ids.begin(), ids.end()), ids.end());
    const uint64_t n_ids = B->n_ids = ids.size();
    std::vector<uint64_t> b_at(n_ids + 1, 0), q_at(n_ids + 1, 0), p_at(n_ids + 1, 0), p_src(n_ids);
    for (uint64_t i = 0; i < n_ids; ++i) {
        uint32_t len; uint64_t pe[2];
        if ((rc = host_read(c, &len, S.reads->len + ids[i], 4)) || (rc = host_read(c, pe, (const char*)S.pq_off + 8 * (uint64_t)ids[i], 16))) return rc;
        if (pe[1] < pe[0]) return fail(DFK_E_INPUT, "cons: the qualities' offset table falls at read %u", ids[i]);
        b_at[i + 1] = b_at[i] + ((uint64_t)len + 3) / 4; q_at[i + 1] = q_at[i] + len; p_at[i + 1] = p_at[i] + (pe[1] - pe[0]); p_src[i] = pe[0];
    }
    std::vector<uint8_t> bases(b_at[n_ids]), pq(p_at[n_ids]);
    for (uint64_t i = 0; i < n_ids; ++i) {
        if (const uint64_t n = b_at[i + 1] - b_at[i]) if ((rc = host_read(c, bases.data() + b_at[i], S.reads->packed + S.reads->at(ids[i]), n))) return rc;
        if (const uint64_t n = p_at[i + 1] - p_at[i]) if ((rc = host_read(c, pq.data() + p_at[i], S.pq + p_src[i], n))) return rc;
    }
    std::vector<uint32_t> slot(nl);
    for (uint64_t l = 0; l < nl; ++l) slot[l] = (uint32_t)slot_of(ids.data(), n_ids, G.h_id[live0 + l]);
    if ((rc = cn_up(c, B->bases, bases.data(), bases.size(), "stack reads' bases")) || (rc = cn_up(c, B->pq, pq.data(), pq.size(), "stack reads' PQVec bytes")) || (rc = cn_up(c, B->bat, b_at.data(), (n_ids + 1) * 8, "stack reads' starts")) ||
        (rc = cn_up(c, B->qat, q_at.data(), (n_ids + 1) * 8, "stack reads' quality starts")) || (rc = cn_up(c, B->pat, p_at.data(), (n_ids + 1) * 8, "stack reads' PQVec starts")) || (rc = cn_up(c, B->slot, slot.data(), nl * 4, "live rows' reads in the batch")) ||
        (rc = c->alloc(B->quals, std::max<uint64_t>(8, q_at[n_ids]), "stack reads' qualities", Place::Low))) return rc;
    times->s_copy += wall_now() - t_g;
    tm.start();
    if (n_ids) {
        hipLaunchKernelGGL(k_cn_decode, dim3(grid_256(n_ids, cus)), dim3(256), 0, c->stream, (const uint8_t*)B->pq.p, (const uint64_t*)B->pat.p, (const uint64_t*)B->qat.p, n_ids, (uint8_t*)B->quals.p, (unsigned long long*)T.bad.p);
        HIP_TRY(hipGetLastError());
    }
    uint64_t n_bad = 0;
    HIP_TRY(hipMemcpyAsync(&n_bad, T.bad.p, 8, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    times->ms_decode += tm.stop();
    if (n_bad) return fail(DFK_E_INPUT, "cons: %llu PQVec stream(s) do not hold exactly as many qualities as their reads have bases", (unsigned long long)n_bad);
    return 0;
}

int cons_build(dfk_ctx* c, const ConsSource& S, const int32_t* pairs, uint64_t n_pairs, uint64_t stacks_per_batch, ConsResult* R)
{
    using namespace dfk_cons;
    const uint64_t n_stacks = 2 * n_pairs;
    CnSides X;
    if (int rc = cn_sides(S, pairs, n_pairs, &X)) return rc;
    const std::vector<uint64_t>& n_rows = X.n_rows; const std::vector<uint64_t>& rfirst = X.rfirst;
    const unsigned cus = (unsigned)c->prop.multiProcessorCount;
    const double t_in = wall_now();
    const uint64_t mark = c->alloc_seq;
    CnTimes times;
    float ms_cons = 0;
    uint64_t n_batches = 0, n_ranges = 0, n_live = 0, n_decoded = 0, n_cells = 0, h_dg[8] = {};
    R->dims.assign(n_stacks, Dim{}); R->starts.assign(n_stacks + 1, 0);
    std::vector<long long> M_all(n_stacks, 0);
    std::vector<uint32_t> kept_all(n_stacks, 0);
    std::vector<std::vector<uint8_t>> parts_out;                                // the bases a batch at a time, in stack order
    auto body = [&]() -> int {
        int rc;
        Timer tm(c->stream);
        CnTables T;
        tm.start();
        if ((rc = cn_tables_up(c, S, X, n_stacks, &T))) return rc;
        times.ms_dims += tm.stop();
        const uint64_t forced = path_switches().pidx_range_pairs;
        for (uint64_t q0 = 0; q0 < n_stacks;) {
            const PidxRange range = next_range(rfirst.data(), n_stacks, q0, row_cap(c->largest_allocatable(), forced));
            const uint64_t q1 = range.e1, ns = q1 - q0, n_items = range.n;
            if (!range.ok) return fail(DFK_E_ARG, "stack %llu alone has %llu rows: a range keeps 32-bit places", (unsigned long long)q0, (unsigned long long)n_items);
            ++n_ranges;
            const uint64_t rmark = c->alloc_seq;
            // ---- dimensions and live rows
            tm.start();
            CnRange G;
            if ((rc = cn_range_live(c, S, X, T, q0, q1, n_items, &G))) return rc;
            times.ms_dims += tm.stop();
            const std::vector<uint64_t>& lfirst = G.h_lfirst;
            std::copy(G.h_M.begin(), G.h_M.end(), M_all.begin() + q0);
            n_live += G.got;
            std::vector<uint64_t> ofirst(ns + 1, 0);
            for (uint64_t s = 0; s < ns; ++s) ofirst[s + 1] = ofirst[s] + (uint64_t)(G.h_M[s] - window_start(G.h_M[s]));
            const std::vector<uint64_t> cfirst = prefix_sums(G.cost.data(), ns);
            DevBuf d_ofirst;
            if ((rc = cn_up(c, d_ofirst, ofirst.data(), (ns + 1) * 8, "columns per stack"))) return rc;
            // ---- the batches of stacks
            for (uint64_t b0 = 0; b0 < ns;) {
                const uint64_t b1 = next_batch(cfirst.data(), ns, b0, batch_room(c->largest_allocatable()), stacks_per_batch), nb = b1 - b0;
                ++n_batches;
                const uint64_t bmark = c->alloc_seq;
                // the reads of the batch, each once, ascending; the gather; the decode
                CnReads B;
                if ((rc = cn_batch_reads(c, S, T, G, b0, b1, tm, &times, &B))) return rc;
                n_decoded += B.n_ids;
                const uint64_t n_out = ofirst[b1] - ofirst[b0];
                DevBuf d_out, d_kept, d_cells;
                if ((rc = c->alloc(d_out, std::max<uint64_t>(8, n_out), "consensus bases", Place::Low)) || (rc = c->alloc(d_kept, nb * 4, "rows kept", Place::Low)) || (rc = c->alloc(d_cells, nb * 8, "cells added", Place::Low))) return rc;
                tm.start();
                const CnBatch Bk{b0, nb, q0, (const long long*)G.M.p, (const int32_t*)T.side_ne.p, (const uint8_t*)T.side_rev.p, (const uint64_t*)G.lfirst.p, (const int32_t*)G.l_pos.p, (const uint32_t*)G.l_len.p,
                                 (const uint32_t*)B.slot.p, B.live0, (const uint64_t*)B.bat.p, (const uint64_t*)B.qat.p, (const uint8_t*)B.bases.p, (const uint8_t*)B.quals.p, (const uint64_t*)d_ofirst.p};
                hipLaunchKernelGGL(k_cn_consensus, dim3(cons_grid(nb, cus)), dim3(GROUP), 0, c->stream, Bk, (uint8_t*)d_out.p, (uint32_t*)d_kept.p, (unsigned long long*)d_cells.p);
                HIP_TRY(hipGetLastError());
                HIP_TRY(hipStreamSynchronize(c->stream));
                ms_cons += tm.stop();
                const double t_d = wall_now();
                parts_out.emplace_back(n_out);
                std::vector<uint64_t> h_cells(nb);
                if (n_out) HIP_TRY(hipMemcpyAsync(parts_out.back().data(), d_out.p, n_out, hipMemcpyDeviceToHost, c->stream));
                HIP_TRY(hipMemcpyAsync(kept_all.data() + q0 + b0, d_kept.p, nb * 4, hipMemcpyDeviceToHost, c->stream));
                HIP_TRY(hipMemcpyAsync(h_cells.data(), d_cells.p, nb * 8, hipMemcpyDeviceToHost, c->stream));
                HIP_TRY(hipStreamSynchronize(c->stream));
                for (uint64_t s = b0; s < b1; ++s) {
                    if (kept_all[q0 + s] > lfirst[s + 1] - lfirst[s]) return fail(DFK_E_HIP, "cons: stack %llu keeps %u of %llu live rows", (unsigned long long)(q0 + s), kept_all[q0 + s], (unsigned long long)(lfirst[s + 1] - lfirst[s]));
                    n_cells += h_cells[s - b0];
                }
                times.s_copy += wall_now() - t_d;
                c->release_since(bmark);
                b0 = b1;
            }
            c->release_since(rmark);
            q0 = q1;
        }
        // ---- the result in stack order, the digest
        uint64_t total = 0;
        for (const auto& p : parts_out) total += p.size();
        R->n_bases = total;
        R->bases.assign(padded(total), 0);
        uint64_t at = 0;
        for (const auto& p : parts_out) { if (!p.empty()) memcpy(R->bases.data() + at, p.data(), p.size()); at += p.size(); }
        for (uint64_t q = 0; q < n_stacks; ++q) {
            const long long M = M_all[q];
            const uint32_t cols = (uint32_t)(M - window_start(M));
            R->dims[q] = Dim{(uint32_t)n_rows[q], M > MAX_WIDTH ? kept_all[q] : (uint32_t)n_rows[q], (int32_t)M, cols};
            R->starts[q + 1] = R->starts[q] + cols;
        }
        if (R->starts[n_stacks] != total) return fail(DFK_E_HIP, "cons: %llu bases came back for %llu columns", (unsigned long long)total, (unsigned long long)R->starts[n_stacks]);
        for (uint64_t i = 0; i < total; ++i) if (R->bases[i] > 3) return fail(DFK_E_HIP, "cons: base %u at %llu", R->bases[i], (unsigned long long)i);
        if (n_stacks) {
            DevBuf d_dims, d_b, dg;
            if ((rc = cn_up(c, d_dims, R->dims.data(), n_stacks * 16, "a.close.cons dims")) || (rc = cn_up(c, d_b, R->bases.data(), total, "a.close.cons bases")) || (rc = c->alloc(dg, 32, "cons digest", Place::Low))) return rc;
            HIP_TRY(hipMemsetAsync(dg.p, 0, 32, c->stream));
            hipLaunchKernelGGL(HIP_KERNEL_NAME(k_digest_seq<uint32_t>), dim3(grid_256(4 * n_stacks, cus)), dim3(256), 0, c->stream, (const uint32_t*)d_dims.p, (uint64_t)(4 * n_stacks), SALT, (unsigned long long*)dg.p);
            if (total) hipLaunchKernelGGL(HIP_KERNEL_NAME(k_digest_seq<uint8_t>), dim3(grid_256(total, cus)), dim3(256), 0, c->stream, (const uint8_t*)d_b.p, total, SALT + 4 * n_stacks, (unsigned long long*)dg.p);
            HIP_TRY(hipGetLastError());
            HIP_TRY(hipMemcpyAsync(h_dg, dg.p, 32, hipMemcpyDeviceToHost, c->stream));
        }
        HIP_TRY(hipStreamSynchronize(c->stream));
        return 0;
    };
    int rc;
    try { rc = body(); } catch (const std::runtime_error& e) { rc = fail(DFK_E_HIP, "%s", e.what()); }
    (void)hipStreamSynchronize(c->stream);
    c->release_since(mark);
    if (rc) return rc;
    const float ms_dims = times.ms_dims, ms_decode = times.ms_decode;
    const double s_copy = times.s_copy;
    R->serial = cons_next_serial();
    uint64_t* s = R->stats;
    s[DFK_CONS_PAIRS] = n_pairs; s[DFK_CONS_STACKS] = n_stacks; s[DFK_CONS_ROWS] = rfirst[n_stacks]; s[DFK_CONS_LIVE] = n_live; s[DFK_CONS_COLUMNS] = R->n_bases; s[DFK_CONS_CELLS] = n_cells;
    s[DFK_CONS_DECODED] = n_decoded; s[DFK_CONS_BATCHES] = n_batches; s[DFK_CONS_RANGES] = n_ranges;
    for (uint64_t q = 0; q < n_stacks; ++q) { s[DFK_CONS_ROWS_KEPT] += R->dims[q].rows_kept; s[DFK_CONS_TRIMMED] += R->dims[q].M > MAX_WIDTH; s[DFK_CONS_REVERSED] += X.rev[q]; }
    s[DFK_CONS_US] = (uint64_t)(1e6 * (wall_now() - t_in)); s[DFK_CONS_US_DIMS] = (uint64_t)(1000.0f * ms_dims); s[DFK_CONS_US_COPY] = (uint64_t)(1e6 * s_copy);
    s[DFK_CONS_US_DECODE] = (uint64_t)(1000.0f * ms_decode); s[DFK_CONS_US_CONS] = (uint64_t)(1000.0f * ms_cons); s[DFK_CONS_SUM] = h_dg[0]; s[DFK_CONS_XOR] = h_dg[1];
    TRACE("cons: %llu pairs, %llu rows (%llu live, %llu kept), %llu stacks trimmed, %llu columns, %llu cells, %llu reads decoded in %llu range(s), %llu batch(es); dims and live rows %.1f ms, decode %.1f ms, consensus %.1f ms, gather and copies %.1f ms",
          (unsigned long long)n_pairs, (unsigned long long)rfirst[n_stacks], (unsigned long long)n_live, (unsigned long long)s[DFK_CONS_ROWS_KEPT], (unsigned long long)s[DFK_CONS_TRIMMED], (unsigned long long)R->n_bases,
          (unsigned long long)n_cells, (unsigned long long)n_decoded, (unsigned long long)n_ranges, (unsigned long long)n_batches, ms_dims, ms_decode, ms_cons, 1e3 * s_copy);
    return 0;
}

// the file into `dir`: whole, or not at all
int cons_write(const ConsResult* R, const std::string& dir)
{
    using namespace dfk_cons;
    const std::string path = dir + "/a.close.cons";
    const uint64_t n = R->starts.size() - 1;
    const int fd = open(path.c_str(), O_WRONLY | O_CREAT | O_TRUNC, 0666);
    if (fd < 0) return fail(DFK_E_ARG, "cannot open %s", path.c_str());
    const dfk_closer::BinHead h = dfk_closer::head_of(MAGIC, n);
    bool bad = pwrite_all(fd, &h, 16, 0) != 0 || pwrite_all(fd, R->starts.data(), 8 * (n + 1), 16) != 0;
    if (!bad && n) bad = pwrite_all(fd, R->dims.data(), 16 * n, dims_at(n)) != 0;
    if (!bad && !R->bases.empty()) bad = pwrite_all(fd, R->bases.data(), R->bases.size(), bases_at(n)) != 0;
    if (close(fd) != 0) bad = true;
    if (bad) { (void)unlink(path.c_str()); return fail(DFK_E_ARG, "short write to %s", path.c_str()); }
    return 0;
}

void cons_drop_arrays(dfk_ctx* c)
{
    HostGraph* G = graph_of(c);
    if (G->cons_arrays) { cons_result_free(G->cons_arrays); G->cons_arrays = nullptr; }
}

// the latest build's result: dfk_cons_build_arrays keeps its own beside the graph until the next build of either kind
int cons_result_of(dfk_ctx* c, ConsResult** out)
{
    if (!c) return fail(DFK_E_ARG, "null context");
    if (c->graph_state && graph_of(c)->cons_arrays) { *out = graph_of(c)->cons_arrays; return 0; }
    PathState* P = built_paths(c);
    if (!P) return fail(DFK_E_STATE, "no stack consensus: call dfk_paths_build, dfk_closer_build, dfk_partners_build and dfk_cons_build");
    if (!P->cons) return fail(DFK_E_STATE, "no stack consensus: call dfk_cons_build");
    *out = P->cons;
    return 0;
}

// the qualities' offset table of the kind the stage refuses: not monotone
int cons_pq_check(const uint64_t* pq_off, uint64_t n)
{
    uint64_t prev = n ? cons_pq_at(pq_off, 0) : 0;
    for (uint64_t r = 0; r < n; ++r) {
        const uint64_t next = cons_pq_at(pq_off, r + 1);
        if (next < prev) return fail(DFK_E_INPUT, "cons: the qualities' offset table is not monotone at read %llu", (unsigned long long)r);
        prev = next;
    }
    return 0;
}

// what dfk_cons_build and dfk_closures_build (dfk_closures.inc) take from the context: the closers' locs and the partners as they
// stand, the graph's involution and edge lengths, the reads as given, checked here
struct ConsContext { std::vector<int32_t> inv, rank_ne; PartnerReads reads; ConsSource S; };
int cons_context(dfk_ctx* c, PathState* P, const uint8_t* packed, const uint64_t* base_off, const uint32_t* read_len, const uint8_t* pq, const uint64_t* pq_off, uint64_t n_reads, ConsContext* X)
{
    if (n_reads != P->n_reads) return fail(DFK_E_ARG, "cons: %llu reads given, %llu pathed", (unsigned long long)n_reads, (unsigned long long)P->n_reads);
    if (n_reads && (!packed || !read_len || !pq)) return fail(DFK_E_ARG, "null argument");
    if (!pq_off) return fail(DFK_E_ARG, "null argument");
    X->reads = PartnerReads{packed, base_off, read_len, n_reads, {}};
    if (int rc = partner_reads_check(X->reads)) return rc;
    if (int rc = cons_pq_check(pq_off, n_reads)) return rc;
    if (!base_off) X->reads.index_dense();
    HIP_TRY(hipSetDevice(c->device));
    const HostGraph* G = graph_of(c);
    const CloserResult* C = P->closer;
    const PartnersResult* Q = P->partners;
    X->inv = involution_of(G);
    X->rank_ne.assign(std::max<uint64_t>(1, C->ce.size()), 0);
    for (uint64_t k = 0; k < C->ce.size(); ++k) {
        if (C->ce[k] >= G->he.size()) return fail(DFK_E_STATE, "the closer sets name edge %llu: the graph has %llu", (unsigned long long)C->ce[k], (unsigned long long)G->he.size());
        X->rank_ne[k] = (int32_t)(G->ce[G->he[C->ce[k]].ce].n + G->K - 1);
    }
    X->S = ConsSource{X->inv.size(), X->inv.data(), C->ce.size(), C->ce.data(), X->rank_ne.data(), C->loc_first.data(), C->locs.data(), Q->starts.size() - 1, Q->starts.data(), Q->recs.data(), &X->reads, pq, pq_off};
    return 0;
}

// dfk_cons_build_arrays' and dfk_closures_build_arrays' arguments checked for the forms dfk_closer_fetch and dfk_partners_fetch give
int cons_arrays_source(dfk_ctx* c, uint64_t n_edges, const int32_t* inv, const int32_t* kmers, uint64_t n_ce, const uint64_t* ce, const uint64_t* loc_first, const uint64_t* locs,
                       const uint64_t* part_first, const uint64_t* parts, const int32_t* pairs, uint64_t n_pairs, const uint8_t* packed, const uint64_t* base_off, const uint32_t* read_len,
                       const uint8_t* pq, const uint64_t* pq_off, uint64_t n_reads, ConsContext* X)
{
    if (!c) return fail(DFK_E_ARG, "null context");
    const uint64_t E = n_edges, N = n_reads;
    if ((E && (!inv || !kmers)) || !loc_first || !part_first || !pq_off || (n_ce && !ce) || (n_pairs && !pairs) || (N && (!packed || !read_len || !pq))) return fail(DFK_E_ARG, "null argument");
    if (N >= (1ull << 31) || E >= (1ull << 31)) return fail(DFK_E_ARG, "%llu reads, %llu edges: 2^31 - 1 of each at most", (unsigned long long)N, (unsigned long long)E);
    for (uint64_t e = 0; e < E; ++e) {
        if (inv[e] < 0 || (uint64_t)inv[e] >= E || inv[inv[e]] != (int32_t)e) return fail(DFK_E_ARG, "inv is not an involution at edge %llu", (unsigned long long)e);
        if (kmers[e] < 1 || kmers[e] > (1 << 30)) return fail(DFK_E_ARG, "edge %llu has %d k-mers", (unsigned long long)e, kmers[e]);
    }
    if (loc_first[0] != 0 || part_first[0] != 0) return fail(DFK_E_ARG, "the tables do not start at 0");
    for (uint64_t k = 0; k < n_ce; ++k) {
        if (ce[k] >= E || (k && ce[k] <= ce[k - 1])) return fail(DFK_E_ARG, "the closer edges are not ascending edges of the graph at rank %llu", (unsigned long long)k);
        if (loc_first[k + 1] < loc_first[k]) return fail(DFK_E_ARG, "the locs' starts fall at rank %llu", (unsigned long long)k);
    }
    for (uint64_t q = 0; q < 2 * n_pairs; ++q) if (part_first[q + 1] < part_first[q]) return fail(DFK_E_ARG, "the partners' starts fall at element %llu", (unsigned long long)q);
    if ((loc_first[n_ce] && !locs) || (part_first[2 * n_pairs] && !parts)) return fail(DFK_E_ARG, "null argument");
    const int64_t far = 1ll << 30;
    for (uint64_t j = 0; j < loc_first[n_ce]; ++j) {
        if (locs[2 * j] >= N) return fail(DFK_E_ARG, "a locs record names read %llu of %llu", (unsigned long long)locs[2 * j], (unsigned long long)N);
        if (dfk_cons::rec_pos(locs, j) <= -far || dfk_cons::rec_pos(locs, j) >= far) return fail(DFK_E_ARG, "a locs record lies at %d", dfk_cons::rec_pos(locs, j));
    }
    for (uint64_t j = 0; j < part_first[2 * n_pairs]; ++j)
        if (dfk_cons::rec_pos(parts, j) <= -far || dfk_cons::rec_pos(parts, j) >= far) return fail(DFK_E_ARG, "a partner record lies at %d", dfk_cons::rec_pos(parts, j));
    X->reads = PartnerReads{packed, base_off, read_len, N, {}};
    if (int rc = partner_reads_check(X->reads)) return rc;
    if (int rc = cons_pq_check(pq_off, N)) return rc;
    if (!base_off) X->reads.index_dense();
    HIP_TRY(hipSetDevice(c->device));
    X->rank_ne.assign(std::max<uint64_t>(1, n_ce), 0);
    for (uint64_t k = 0; k < n_ce; ++k) X->rank_ne[k] = (int32_t)(kmers[ce[k]] + (int32_t)c->cfg.K - 1);
    X->S = ConsSource{E, inv, n_ce, ce, X->rank_ne.data(), loc_first, locs, 2 * n_pairs, part_first, parts, &X->reads, pq, pq_off};
    return 0;
}

} // namespace

extern "C" {

int dfk_cons_build(dfk_ctx* c, const int32_t* pairs, uint64_t n_pairs, const uint8_t* packed, const uint64_t* base_off, const uint32_t* read_len, const uint8_t* pq, const uint64_t* pq_off, uint64_t n_reads)
{
    return guarded([&]() -> int {
    if (!c) return fail(DFK_E_ARG, "null context");
    PathState* P = built_paths(c);
    if (!P) return fail(DFK_E_STATE, "no paths: call dfk_paths_build");
    if (!P->closer) return fail(DFK_E_STATE, "no closer sets: call dfk_closer_build for these pairs first");
    if (!P->partners) return fail(DFK_E_STATE, "no partners: call dfk_partners_build for these pairs first");
    if (!pairs) {
        if (n_pairs) return fail(DFK_E_ARG, "null argument");
        if (!P->hops_valid) return fail(DFK_E_STATE, "no edge pairs: call dfk_hops_build, or pass the pairs");
        pairs = P->hops.data(); n_pairs = P->hops.size() / 2;
    }
    const PartnersResult* Q = P->partners;
    if (Q->pairs.size() != 2 * n_pairs || (n_pairs && memcmp(Q->pairs.data(), pairs, 8 * n_pairs) != 0)) return fail(DFK_E_ARG, "cons: these are not the pairs the partners were made for");
    ConsContext X;
    if (int rc = cons_context(c, P, packed, base_off, read_len, pq, pq_off, n_reads, &X)) return rc;
    std::unique_ptr<ConsResult> R(new ConsResult);
    if (int rc = cons_build(c, X.S, pairs, n_pairs, 0, R.get())) return rc;        // (refused: the earlier result is still served)
    R->pairs.assign(pairs, pairs + 2 * n_pairs);
    cons_drop_arrays(c);
    if (P->cons) cons_result_free(P->cons);
    P->cons = R.release(); P->cons_free = cons_result_free;
    return 0;
    });
}

// The stage on host arrays: everything it reads is given, and checked here for the forms dfk_closer_fetch and dfk_partners_fetch give.
int dfk_cons_build_arrays(dfk_ctx* c, uint64_t n_edges, const int32_t* inv, const int32_t* kmers, uint64_t n_ce, const uint64_t* ce, const uint64_t* loc_first, const uint64_t* locs,
                          const uint64_t* part_first, const uint64_t* parts, const int32_t* pairs, uint64_t n_pairs, const uint8_t* packed, const uint64_t* base_off, const uint32_t* read_len,
                          const uint8_t* pq, const uint64_t* pq_off, uint64_t n_reads, uint64_t stacks_per_batch, const char* dir)
{
    return guarded([&]() -> int {
    ConsContext X;
    if (int rc = cons_arrays_source(c, n_edges, inv, kmers, n_ce, ce, loc_first, locs, part_first, parts, pairs, n_pairs, packed, base_off, read_len, pq, pq_off, n_reads, &X)) return rc;
    std::unique_ptr<ConsResult> R(new ConsResult);
    if (int rc = cons_build(c, X.S, pairs, n_pairs, stacks_per_batch, R.get())) return rc;
    if (dir) if (int rc = cons_write(R.get(), dir)) return rc;
    cons_drop_arrays(c);
    graph_of(c)->cons_arrays = R.release(); graph_of(c)->cons_free = cons_result_free;
    return 0;
    });
}
int dfk_cons_stats(dfk_ctx* c, uint64_t* out)
{
    return guarded([&]() -> int {
    ConsResult* R = nullptr;
    if (int rc = cons_result_of(c, &R)) return rc;
    if (!out) return fail(DFK_E_ARG, "null argument");
    for (int i = 0; i < DFK_CONS_WORDS; ++i) out[i] = R->stats[i];
    return 0;
    });
}

int dfk_cons_fetch(dfk_ctx* c, uint64_t* starts, uint32_t* dims, uint64_t* n_elements, uint8_t* bases, uint64_t bases_cap, uint64_t* n_bases)
{
    return guarded([&]() -> int {
    ConsResult* R = nullptr;
    if (int rc = cons_result_of(c, &R)) return rc;
    const uint64_t n = R->starts.size() - 1, nb = R->n_bases;
    if (n_elements) *n_elements = n;
    if (n_bases) *n_bases = nb;
    if ((bases || bases_cap) && bases_cap < nb) return fail(DFK_E_ARG, "buffer too small: %llu < %llu consensus bases", (unsigned long long)bases_cap, (unsigned long long)nb);
    if (bases_cap && nb && !bases) return fail(DFK_E_ARG, "null argument");
    if (bases && nb) memcpy(bases, R->bases.data(), nb);
    if (starts) memcpy(starts, R->starts.data(), 8 * (n + 1));                 // the starts: room for n_elements + 1 words
    if (dims && n) memcpy(dims, R->dims.data(), 16 * n);                       // the dims: room for 4 * n_elements words
    return 0;
    });
}

int dfk_cons_write(dfk_ctx* c, const char* dir)
{
    return guarded([&]() -> int {
    ConsResult* R = nullptr;
    if (int rc = cons_result_of(c, &R)) return rc;
    if (!dir) return fail(DFK_E_ARG, "null directory");
    return cons_write(R, dir);
    });
}

} // extern "C"
