// superplus_amd/csrc/dfk_closures.inc -- CloseGap2's closures per pair (10X/Closomatic.cc:651-660; ReadStack.cc's Merge and
// Consensus1 with qualities) and the file a.close.closures, included by dfk.hip.
//
// The rule, the shared pieces, the plan and the file's layout: dfk_closures.h.  The kernel: dfk_closures_kernels.h.  Here:
// closures_build() -- the closable pairs picked out and their stacks alone made a source of their own; then dfk_cons.inc's own steps
// (cn_sides, cn_tables_up, cn_range_live, cn_batch_reads): a range of whole pairs at a time the dimensions and the live rows, under it
// the batches of closures: the reads the live rows of their pairs' stacks name gathered once each and decoded, the merged consensus a
// workgroup a tile of a closure, the bases and the counts coming back -- and closures_write().  Everything on the device comes from
// the arena and goes back before build returns.
#include "dfk_closures_kernels.h"

namespace {

struct ClosuresResult {
    std::vector<uint64_t> pair_first;             // [n_pairs + 1], in closures
    std::vector<uint64_t> starts;                 // [n + 1], in bases
    std::vector<dfk_closures::Rec> recs;          // [n]
    std::vector<uint8_t> bases;                   // padded with zero bytes to a multiple of 8
    uint64_t n_bases = 0;
    uint64_t stats[DFK_CLOSURES_WORDS] = {};
    std::vector<int32_t> pairs;                   // dfk_closures_build: the pairs it was made for (dfk_allclosures_write asks)
};
void closures_result_free(ClosuresResult* r) { delete r; }

int closures_build(dfk_ctx* c, const ConsSource& S0, const int32_t* pairs, uint64_t n_pairs, const uint64_t* off_first, const int32_t* offsets, uint64_t per_batch, ClosuresResult* R)
{
    using namespace dfk_cons;
    using dfk_closures::TILES;
    if (S0.n_parts != 2 * n_pairs) return fail(DFK_E_ARG, "closures: %llu pairs given, the partners were made for %llu", (unsigned long long)n_pairs, (unsigned long long)(S0.n_parts / 2));
    if (n_pairs >= (1ull << 30)) return fail(DFK_E_ARG, "%llu pairs: a closure keeps its pair in 32 bits", (unsigned long long)n_pairs);
    if (off_first[0] != 0) return fail(DFK_E_ARG, "the offsets' starts do not begin at 0");
    for (uint64_t pi = 0; pi < n_pairs; ++pi) if (off_first[pi + 1] < off_first[pi]) return fail(DFK_E_ARG, "the offsets' starts fall at pair %llu", (unsigned long long)pi);
    for (uint64_t i = 0; i < 2 * n_pairs; ++i)
        if (pairs[i] < 0 || (uint64_t)pairs[i] >= S0.n_edges) return fail(DFK_E_ARG, "pair %llu names edge %d: the graph has %llu", (unsigned long long)(i / 2), pairs[i], (unsigned long long)S0.n_edges);
    // ---- the closable pairs (:651), their stacks alone: two a pair, the partners' elements of those pairs
    const dfk_closures::Closable C = dfk_closures::closable_of(n_pairs, off_first, offsets);
    const uint64_t n_cp = C.cp.size(), n_stacks = 2 * n_cp, n = C.cl_off.size();
    std::vector<int32_t> cpairs(std::max<uint64_t>(1, 2 * n_cp));
    std::vector<uint64_t> part_first(n_stacks + 1, 0), parts(2, 0);
    for (uint64_t i = 0; i < n_cp; ++i) {
        cpairs[2 * i] = pairs[2 * C.cp[i]]; cpairs[2 * i + 1] = pairs[2 * C.cp[i] + 1];
        for (int ei = 0; ei < 2; ++ei) {
            const uint64_t q = 2 * C.cp[i] + ei, a = S0.part_first[q], b = S0.part_first[q + 1];
            if (b > a) parts.insert(parts.end() - 2, S0.parts + 2 * a, S0.parts + 2 * b);             // (two spare words stay behind: never an empty table)
            part_first[2 * i + ei + 1] = part_first[2 * i + ei] + (b - a);
        }
    }
    ConsSource S = S0;
    S.n_parts = n_stacks; S.part_first = part_first.data(); S.parts = parts.data();
    CnSides X;
    if (int rc = cn_sides(S, cpairs.data(), n_cp, &X)) return rc;
    std::vector<uint64_t> pfirst(n_cp + 1);                                                // rows before closable pair i
    for (uint64_t i = 0; i <= n_cp; ++i) pfirst[i] = X.rfirst[2 * i];
    const unsigned cus = (unsigned)c->prop.multiProcessorCount;
    const double t_in = wall_now();
    const uint64_t mark = c->alloc_seq;
    CnTimes times;
    float ms_cons = 0;
    uint64_t n_batches = 0, n_ranges = 0, n_walked = 0, n_cells = 0, n_empty = 0, h_dg[8] = {};
    std::vector<std::vector<uint8_t>> parts_out;                                           // the bases a batch at a time, in closure order
    std::vector<uint32_t> cl_cols(n, 0), cl_rows(n, 0);
    auto body = [&]() -> int {
        int rc;
        Timer tm(c->stream);
        CnTables T;
        tm.start();
        if (n_cp) if ((rc = cn_tables_up(c, S, X, n_stacks, &T))) return rc;
        times.ms_dims += tm.stop();
        const uint64_t forced = path_switches().pidx_range_pairs;
        for (uint64_t p0 = 0; p0 < n_cp;) {
            const PidxRange range = next_range(pfirst.data(), n_cp, p0, row_cap(c->largest_allocatable(), forced));
            const uint64_t p1 = range.e1, q0 = 2 * p0, ns = 2 * (p1 - p0), n_items = range.n;
            if (!range.ok) return fail(DFK_E_ARG, "pair %llu alone has %llu rows: a range keeps 32-bit places", (unsigned long long)C.cp[p0], (unsigned long long)n_items);
            ++n_ranges;
            const uint64_t rmark = c->alloc_seq;
            // ---- dimensions and live rows of the range's stacks
            tm.start();
            CnRange G;
            if ((rc = cn_range_live(c, S, X, T, q0, q0 + ns, n_items, &G))) return rc;
            DevBuf d_def;
            if ((rc = c->alloc(d_def, std::max<uint64_t>(8, G.got * 4), "live rows with a defined cell", Place::Low))) return rc;
            HIP_TRY(hipMemsetAsync(d_def.p, 0, std::max<uint64_t>(8, G.got * 4), c->stream));
            times.ms_dims += tm.stop();
            const std::vector<uint64_t>& lfirst = G.h_lfirst;
            auto cols_of = [&](uint64_t s) { return (int64_t)(G.h_M[s] - window_start(G.h_M[s])); };
            // ---- the closures of the range: their offsets against the dimensions, their widths, what they cost a batch
            const uint64_t k0 = C.cl_first[p0], nk = C.cl_first[p1] - k0;
            std::vector<uint32_t> pair_of(nk);
            std::vector<uint64_t> cost(nk);
            for (uint64_t i = p0; i < p1; ++i)
                for (uint64_t k = C.cl_first[i]; k < C.cl_first[i + 1]; ++k) {
                    const uint64_t s0 = 2 * (i - p0);
                    const int64_t cols1 = cols_of(s0), cols2 = cols_of(s0 + 1), off = C.cl_off[k];
                    if (!dfk_closures::offset_ok(cols1, cols2, off))
                        return fail(DFK_E_ARG, "closures: pair %llu has the offset %lld: outside [%lld, %lld], its stacks are %lld and %lld columns wide", (unsigned long long)C.cp[i], (long long)off, (long long)-cols2, (long long)cols1, (long long)cols1, (long long)cols2);
                    pair_of[k - k0] = (uint32_t)(i - p0);
                    cl_cols[k] = (uint32_t)dfk_closures::merged_cols(cols1, cols2, off);
                    cost[k - k0] = dfk_closures::BYTES_PER_CLOSURE + G.cost[s0] + G.cost[s0 + 1];
                    n_walked += lfirst[s0 + 2] - lfirst[s0];
                }
            const std::vector<uint64_t> cfirst = prefix_sums(cost.data(), nk);
            // ---- the batches of closures
            for (uint64_t b0 = 0; b0 < nk;) {
                const uint64_t b1 = next_batch(cfirst.data(), nk, b0, batch_room(c->largest_allocatable()), per_batch), nb = b1 - b0;
                ++n_batches;
                const uint64_t bmark = c->alloc_seq;
                // the reads of the batch's pairs' stacks, each once, ascending; the gather; the decode
                const uint64_t sa = 2 * (uint64_t)pair_of[b0], sb = 2 * (uint64_t)pair_of[b1 - 1] + 2;
                CnReads B;
                if ((rc = cn_batch_reads(c, S, T, G, sa, sb, tm, &times, &B))) return rc;
                const double t_u = wall_now();
                std::vector<uint64_t> ofirst(nb + 1, 0);
                for (uint64_t k = 0; k < nb; ++k) ofirst[k + 1] = ofirst[k] + cl_cols[k0 + b0 + k];
                const uint64_t n_out = ofirst[nb];
                DevBuf d_pair, d_off, d_ofirst, d_out, d_cells, d_empty;
                if ((rc = cn_up(c, d_pair, pair_of.data() + b0, nb * 4, "closures' pairs")) || (rc = cn_up(c, d_off, C.cl_off.data() + k0 + b0, nb * 4, "closures' offsets")) ||
                    (rc = cn_up(c, d_ofirst, ofirst.data(), (nb + 1) * 8, "columns per closure")) || (rc = c->alloc(d_out, std::max<uint64_t>(8, n_out), "closure bases", Place::Low)) ||
                    (rc = c->alloc(d_cells, nb * TILES * 8, "cells added", Place::Low)) || (rc = c->alloc(d_empty, nb * TILES * 4, "columns nothing was added to", Place::Low))) return rc;
                times.s_copy += wall_now() - t_u;
                tm.start();
                const CsBatch Bk{nb, (const uint32_t*)d_pair.p, (const int32_t*)d_off.p, (const uint64_t*)d_ofirst.p, q0, (const long long*)G.M.p, (const int32_t*)T.side_ne.p, (const uint8_t*)T.side_rev.p,
                                 (const uint64_t*)G.lfirst.p, (const int32_t*)G.l_pos.p, (const uint32_t*)G.l_len.p, (const uint32_t*)B.slot.p, B.live0, (const uint64_t*)B.bat.p, (const uint64_t*)B.qat.p,
                                 (const uint8_t*)B.bases.p, (const uint8_t*)B.quals.p};
                hipLaunchKernelGGL(k_cs_closures, dim3(dfk_closures::closures_grid(nb, cus)), dim3(dfk_closures::GROUP), 0, c->stream, Bk, (uint8_t*)d_out.p, (uint32_t*)d_def.p, (unsigned long long*)d_cells.p, (uint32_t*)d_empty.p);
                HIP_TRY(hipGetLastError());
                HIP_TRY(hipStreamSynchronize(c->stream));
                ms_cons += tm.stop();
                const double t_d = wall_now();
                parts_out.emplace_back(n_out);
                std::vector<uint64_t> h_cells(nb * TILES);
                std::vector<uint32_t> h_empty(nb * TILES);
                if (n_out) HIP_TRY(hipMemcpyAsync(parts_out.back().data(), d_out.p, n_out, hipMemcpyDeviceToHost, c->stream));
                HIP_TRY(hipMemcpyAsync(h_cells.data(), d_cells.p, nb * TILES * 8, hipMemcpyDeviceToHost, c->stream));
                HIP_TRY(hipMemcpyAsync(h_empty.data(), d_empty.p, nb * TILES * 4, hipMemcpyDeviceToHost, c->stream));
                HIP_TRY(hipStreamSynchronize(c->stream));
                for (uint64_t i = 0; i < nb * TILES; ++i) { n_cells += h_cells[i]; n_empty += h_empty[i]; }
                times.s_copy += wall_now() - t_d;
                c->release_since(bmark);
                b0 = b1;
            }
            // ---- rows_kept of the range's stacks: all rows without a trim, else the live rows that had a defined cell
            std::vector<uint32_t> h_def(G.got);
            if (G.got) HIP_TRY(hipMemcpyAsync(h_def.data(), d_def.p, G.got * 4, hipMemcpyDeviceToHost, c->stream));
            HIP_TRY(hipStreamSynchronize(c->stream));
            for (uint64_t i = p0; i < p1; ++i) {
                uint64_t rows = 0;
                for (uint64_t s = 2 * (i - p0); s < 2 * (i - p0) + 2; ++s) {
                    uint64_t kept = 0;
                    for (uint64_t l = lfirst[s]; l < lfirst[s + 1]; ++l) { if (h_def[l] > 1) return fail(DFK_E_HIP, "closures: flag %u at live row %llu", h_def[l], (unsigned long long)l); kept += h_def[l]; }
                    rows += G.h_M[s] > MAX_WIDTH ? kept : X.n_rows[q0 + s];
                }
                for (uint64_t k = C.cl_first[i]; k < C.cl_first[i + 1]; ++k) cl_rows[k] = (uint32_t)rows;
            }
            c->release_since(rmark);
            p0 = p1;
        }
        // ---- the result in closure order, the digest
        uint64_t total = 0;
        for (const auto& p : parts_out) total += p.size();
        R->n_bases = total;
        R->bases.assign(padded(total), 0);
        uint64_t at = 0;
        for (const auto& p : parts_out) { if (!p.empty()) memcpy(R->bases.data() + at, p.data(), p.size()); at += p.size(); }
        R->pair_first.assign(n_pairs + 1, 0); R->starts.assign(n + 1, 0); R->recs.assign(n, dfk_closures::Rec{});
        for (uint64_t i = 0; i < n_cp; ++i) {
            R->pair_first[C.cp[i] + 1] = C.cl_first[i + 1] - C.cl_first[i];
            for (uint64_t k = C.cl_first[i]; k < C.cl_first[i + 1]; ++k) { R->recs[k] = dfk_closures::Rec{(uint32_t)C.cp[i], C.cl_off[k], cl_cols[k], cl_rows[k]}; R->starts[k + 1] = R->starts[k] + cl_cols[k]; }
        }
        for (uint64_t pi = 0; pi < n_pairs; ++pi) R->pair_first[pi + 1] += R->pair_first[pi];
        if (R->starts[n] != total) return fail(DFK_E_HIP, "closures: %llu bases came back for %llu columns", (unsigned long long)total, (unsigned long long)R->starts[n]);
        for (uint64_t i = 0; i < total; ++i) if (R->bases[i] > 3) return fail(DFK_E_HIP, "closures: base %u at %llu", R->bases[i], (unsigned long long)i);
        if (n) {
            DevBuf d_r, d_b, dg;
            if ((rc = cn_up(c, d_r, R->recs.data(), n * 16, "a.close.closures records")) || (rc = cn_up(c, d_b, R->bases.data(), total, "a.close.closures bases")) || (rc = c->alloc(dg, 32, "closures digest", Place::Low))) return rc;
            HIP_TRY(hipMemsetAsync(dg.p, 0, 32, c->stream));
            hipLaunchKernelGGL(HIP_KERNEL_NAME(k_digest_seq<uint32_t>), dim3(grid_256(4 * n, cus)), dim3(256), 0, c->stream, (const uint32_t*)d_r.p, (uint64_t)(4 * n), dfk_closures::SALT, (unsigned long long*)dg.p);
            if (total) hipLaunchKernelGGL(HIP_KERNEL_NAME(k_digest_seq<uint8_t>), dim3(grid_256(total, cus)), dim3(256), 0, c->stream, (const uint8_t*)d_b.p, total, dfk_closures::SALT + 4 * n, (unsigned long long*)dg.p);
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
    uint64_t* s = R->stats;
    s[DFK_CLOSURES_PAIRS] = n_pairs; s[DFK_CLOSURES_CLOSABLE] = n_cp; s[DFK_CLOSURES_OVER] = C.over; s[DFK_CLOSURES_CLOSURES] = n; s[DFK_CLOSURES_COLUMNS] = R->n_bases; s[DFK_CLOSURES_CELLS] = n_cells;
    s[DFK_CLOSURES_LIVE] = n_walked; s[DFK_CLOSURES_EMPTY] = n_empty; s[DFK_CLOSURES_BATCHES] = n_batches; s[DFK_CLOSURES_RANGES] = n_ranges;
    for (const dfk_closures::Rec& r : R->recs) { s[DFK_CLOSURES_SHORT] += r.cols < (uint32_t)c->cfg.K; s[DFK_CLOSURES_ROWLESS] += r.rows == 0; }
    s[DFK_CLOSURES_US] = (uint64_t)(1e6 * (wall_now() - t_in)); s[DFK_CLOSURES_US_DIMS] = (uint64_t)(1000.0f * times.ms_dims); s[DFK_CLOSURES_US_COPY] = (uint64_t)(1e6 * times.s_copy);
    s[DFK_CLOSURES_US_DECODE] = (uint64_t)(1000.0f * times.ms_decode); s[DFK_CLOSURES_US_CONS] = (uint64_t)(1000.0f * ms_cons); s[DFK_CLOSURES_SUM] = h_dg[0]; s[DFK_CLOSURES_XOR] = h_dg[1];
    TRACE("closures: %llu pairs, %llu closable, %llu closures, %llu columns (%llu empty), %llu cells, %llu live rows walked in %llu range(s), %llu batch(es); dims and live rows %.1f ms, decode %.1f ms, consensus %.1f ms, gather and copies %.1f ms",
          (unsigned long long)n_pairs, (unsigned long long)n_cp, (unsigned long long)n, (unsigned long long)R->n_bases, (unsigned long long)n_empty, (unsigned long long)n_cells, (unsigned long long)n_walked,
          (unsigned long long)n_ranges, (unsigned long long)n_batches, times.ms_dims, times.ms_decode, ms_cons, 1e3 * times.s_copy);
    return 0;
}

// the file into `dir`: whole, or not at all
int closures_write(const ClosuresResult* R, const std::string& dir)
{
    using namespace dfk_closures;
    const std::string path = dir + "/a.close.closures";
    const uint64_t n = R->recs.size(), np = R->pair_first.size() - 1;
    const int fd = open(path.c_str(), O_WRONLY | O_CREAT | O_TRUNC, 0666);
    if (fd < 0) return fail(DFK_E_ARG, "cannot open %s", path.c_str());
    const dfk_closer::BinHead h = dfk_closer::head_of(MAGIC, n);
    bool bad = pwrite_all(fd, &h, 16, 0) != 0 || pwrite_all(fd, &np, 8, 16) != 0 || pwrite_all(fd, R->pair_first.data(), 8 * (np + 1), pair_first_at()) != 0 ||
               pwrite_all(fd, R->starts.data(), 8 * (n + 1), starts_at(np)) != 0;
    if (!bad && n) bad = pwrite_all(fd, R->recs.data(), 16 * n, recs_at(n, np)) != 0;
    if (!bad && !R->bases.empty()) bad = pwrite_all(fd, R->bases.data(), R->bases.size(), bases_at(n, np)) != 0;
    if (close(fd) != 0) bad = true;
    if (bad) { (void)unlink(path.c_str()); return fail(DFK_E_ARG, "short write to %s", path.c_str()); }
    return 0;
}

// the latest dfk_closures_build*'s result: one a context, kept beside the graph
int closures_result_of(dfk_ctx* c, ClosuresResult** out)
{
    if (!c) return fail(DFK_E_ARG, "null context");
    if (!c->graph_state || !graph_of(c)->closures) return fail(DFK_E_STATE, "no closures: call dfk_closures_build or dfk_closures_build_arrays");
    *out = graph_of(c)->closures;
    return 0;
}
void closures_keep(dfk_ctx* c, ClosuresResult* R)
{
    HostGraph* G = graph_of(c);
    if (G->closures) closures_result_free(G->closures);
    G->closures = R; G->closures_free = closures_result_free;
}

} // namespace

extern "C" {

int dfk_closures_build(dfk_ctx* c, const uint8_t* packed, const uint64_t* base_off, const uint32_t* read_len, const uint8_t* pq, const uint64_t* pq_off, uint64_t n_reads)
{
    return guarded([&]() -> int {
    ConsResult* K = nullptr;
    if (int rc = cons_result_of(c, &K)) return rc;                                          // DFK_E_STATE without a consensus
    PathState* P = built_paths(c);
    if (!P || K != P->cons) return fail(DFK_E_STATE, "the latest stack consensus came from dfk_cons_build_arrays: the context holds no stacks for it; call dfk_closures_build_arrays");
    OffsetsResult* O = nullptr;
    if (int rc = offsets_result_of(c, &O)) return rc;                                       // DFK_E_STATE without offsets
    if (!O->cons_serial) return fail(DFK_E_STATE, "the offsets came from dfk_offsets_build_arrays: call dfk_offsets_build after dfk_cons_build");
    if (O->cons_serial != K->serial) return fail(DFK_E_STATE, "the offsets were made from an older stack consensus: call dfk_offsets_build again");
    if (!P->closer || !P->partners) return fail(DFK_E_STATE, "the closer sets or the partners the stack consensus was made from are gone: build them and the consensus again");
    const uint64_t n_pairs = K->pairs.size() / 2;
    if (P->partners->pairs != K->pairs || O->starts.size() != n_pairs + 1) return fail(DFK_E_STATE, "the partners or the offsets are not those of the stack consensus' pairs: build the chain again");
    std::vector<uint64_t> off_first(n_pairs + 1, 0);
    std::vector<int32_t> offsets(1, 0);
    for (uint64_t pi = 0; pi < n_pairs; ++pi) {                                             // what GetOffsets1 returned: the state-0 records, in record order
        for (uint64_t j = O->starts[pi]; j < O->starts[pi + 1]; ++j) if (O->recs[j].state == dfk_offsets::SURVIVES) offsets.insert(offsets.end() - 1, O->recs[j].offset);
        off_first[pi + 1] = offsets.size() - 1;
    }
    ConsContext X;
    if (int rc = cons_context(c, P, packed, base_off, read_len, pq, pq_off, n_reads, &X)) return rc;
    const int32_t none[2] = {0, 0};
    std::unique_ptr<ClosuresResult> R(new ClosuresResult);
    if (int rc = closures_build(c, X.S, n_pairs ? K->pairs.data() : none, n_pairs, off_first.data(), offsets.data(), 0, R.get())) return rc;     // (refused: the earlier result is still served)
    R->pairs = K->pairs;
    closures_keep(c, R.release());
    return 0;
    });
}

// The stage on host arrays: dfk_cons_build_arrays' arguments, checked as it checks them, and the offsets of every pair.
int dfk_closures_build_arrays(dfk_ctx* c, uint64_t n_edges, const int32_t* inv, const int32_t* kmers, uint64_t n_ce, const uint64_t* ce, const uint64_t* loc_first, const uint64_t* locs,
                              const uint64_t* part_first, const uint64_t* parts, const int32_t* pairs, uint64_t n_pairs, const uint8_t* packed, const uint64_t* base_off, const uint32_t* read_len,
                              const uint8_t* pq, const uint64_t* pq_off, uint64_t n_reads, const uint64_t* off_first, const int32_t* offsets, uint64_t closures_per_batch, const char* dir)
{
    return guarded([&]() -> int {
    ConsContext X;
    if (int rc = cons_arrays_source(c, n_edges, inv, kmers, n_ce, ce, loc_first, locs, part_first, parts, pairs, n_pairs, packed, base_off, read_len, pq, pq_off, n_reads, &X)) return rc;
    if (!off_first) return fail(DFK_E_ARG, "null argument");
    for (uint64_t pi = 0; pi < n_pairs; ++pi) if (off_first[pi + 1] < off_first[pi]) return fail(DFK_E_ARG, "the offsets' starts fall at pair %llu", (unsigned long long)pi);
    if (off_first[n_pairs] > off_first[0] && !offsets) return fail(DFK_E_ARG, "null argument");
    const int32_t none[2] = {0, 0};
    std::unique_ptr<ClosuresResult> R(new ClosuresResult);
    if (int rc = closures_build(c, X.S, n_pairs ? pairs : none, n_pairs, off_first, offsets ? offsets : none, closures_per_batch, R.get())) return rc;
    if (dir) if (int rc = closures_write(R.get(), dir)) return rc;
    closures_keep(c, R.release());
    return 0;
    });
}

int dfk_closures_stats(dfk_ctx* c, uint64_t* out)
{
    return guarded([&]() -> int {
    ClosuresResult* R = nullptr;
    if (int rc = closures_result_of(c, &R)) return rc;
    if (!out) return fail(DFK_E_ARG, "null argument");
    for (int i = 0; i < DFK_CLOSURES_WORDS; ++i) out[i] = R->stats[i];
    return 0;
    });
}

int dfk_closures_fetch(dfk_ctx* c, uint64_t* pair_first, uint64_t* starts, uint32_t* records, uint64_t* n_pairs, uint64_t* n_closures, uint8_t* bases, uint64_t bases_cap, uint64_t* n_bases)
{
    return guarded([&]() -> int {
    ClosuresResult* R = nullptr;
    if (int rc = closures_result_of(c, &R)) return rc;
    const uint64_t np = R->pair_first.size() - 1, n = R->recs.size(), nb = R->n_bases;
    if (n_pairs) *n_pairs = np;
    if (n_closures) *n_closures = n;
    if (n_bases) *n_bases = nb;
    if ((bases || bases_cap) && bases_cap < nb) return fail(DFK_E_ARG, "buffer too small: %llu < %llu closure bases", (unsigned long long)bases_cap, (unsigned long long)nb);
    if (bases_cap && nb && !bases) return fail(DFK_E_ARG, "null argument");
    if (bases && nb) memcpy(bases, R->bases.data(), nb);
    if (pair_first) memcpy(pair_first, R->pair_first.data(), 8 * (np + 1));      // room for n_pairs + 1 words
    if (starts) memcpy(starts, R->starts.data(), 8 * (n + 1));                   // room for n_closures + 1 words
    if (records && n) memcpy(records, R->recs.data(), 16 * n);                   // room for 4 * n_closures u32
    return 0;
    });
}

int dfk_closures_write(dfk_ctx* c, const char* dir)
{
    return guarded([&]() -> int {
    ClosuresResult* R = nullptr;
    if (int rc = closures_result_of(c, &R)) return rc;
    if (!dir) return fail(DFK_E_ARG, "null directory");
    return closures_write(R, dir);
    });
}

} // extern "C"
