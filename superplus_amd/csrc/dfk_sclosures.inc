// superplus_amd/csrc/dfk_sclosures.inc -- Stackster's closures per pair (10X/Stackster.cc:712-757; ReadStack.cc's Trim, Merge and
// Consensus1 with qualities), the file a.stack.closures and the combined list a.closures.fastb (RunStages.cc:290-325), included by
// dfk.hip.
//
// The rule, the shared pieces, the plan and the file's layout: dfk_sclosures.h.  The kernels: dfk_sclosures_kernels.h.  Here:
// sclosures_build() -- the tables checked (dfk_scons.inc's checks of the walks, dfk_sclosures.h's check_tables of the dims and the
// offsets), the closable pairs picked out; a range of whole closable pairs at a time the live rows from the walks' placed records
// (host, dfk_scons.h's rule), under it the batches of closures: the reads the live rows of their pairs' stacks name gathered once each,
// decoded and lowered (dfk_cons.inc's cn_batch_reads, k_wk_lower), the merged consensus a workgroup a tile of a closure, the flags
// counted per closure and side, the bases and the counts coming back -- sclosures_write() and allclosures_write().  Everything on the
// device comes from the arena and goes back before build returns.
#include "dfk_sclosures_kernels.h"
#include "feudal_io.h"

namespace {

struct SclosuresResult {
    std::vector<uint64_t> pair_first;             // [n_pairs + 1], in closures
    std::vector<uint64_t> starts;                 // [n + 1], in bases
    std::vector<dfk_sclosures::Rec> recs;         // [n]
    std::vector<uint8_t> bases;                   // padded with zero bytes to a multiple of 8
    uint64_t n_bases = 0;
    uint64_t stats[DFK_SCLOSURES_WORDS] = {};
    std::vector<int32_t> pairs;                   // dfk_sclosures_build: the pairs the walks were made for (dfk_allclosures_write asks)
    bool from_chain = false;                      // made by dfk_sclosures_build
};
void sclosures_result_free(SclosuresResult* r) { delete r; }

struct SclosuresSource {
    SconsSource W;                                // the walks and the reads
    const dfk_scons::Dim* dims; const uint64_t* so_starts; const dfk_soffsets::PairWords* words; const dfk_soffsets::Rec* recs;
};

int sclosures_build(dfk_ctx* c, const SclosuresSource& X, uint64_t per_batch, SclosuresResult* R)
{
    using namespace dfk_sclosures;
    const SconsSource& S = X.W;
    const uint64_t N = S.rd->n, n_pairs = S.n_pairs, n_all = 2 * n_pairs;
    if (N > (1ull << 31) || n_pairs >= (1ull << 30)) return fail(DFK_E_ARG, "%llu reads, %llu pairs: a row keeps its read in 31 bits", (unsigned long long)N, (unsigned long long)n_pairs);
    // ---- the walks' tables, checked as dfk_scons.inc checks them
    if (S.starts[0] != 0) return fail(DFK_E_ARG, "sclosures: the walks' starts do not begin at 0");
    for (uint64_t q = 0; q < n_all; ++q)
        if (S.starts[q + 1] < S.starts[q] || S.starts[q + 1] - S.starts[q] != S.recs[q].placed) return fail(DFK_E_ARG, "sclosures: the walks' starts fall or leave walk %llu other than its %u placed records", (unsigned long long)q, S.recs[q].placed);
    const uint64_t n_locs = S.starts[n_all];
    std::vector<uint32_t> loc_len(n_locs + 1, 0);
    for (uint64_t j = 0; j < n_locs; ++j) {
        const dfk_walks::Loc& L = S.locs[j];
        if (L.id < 0 || (uint64_t)L.id >= N) return fail(DFK_E_ARG, "a placed record names read %lld of %llu", (long long)L.id, (unsigned long long)N);
        if (L.start <= -(1 << 30) || L.start >= (1 << 30) || L.fw > 1) return fail(DFK_E_ARG, "a placed record lies at %d with the flag %u", L.start, L.fw);
        if (int rc = host_read(c, &loc_len[j], S.rd->len + L.id, 4)) return rc;
    }
    uint64_t n_yield = 0;
    for (uint64_t pi = 0; pi < n_pairs; ++pi) {
        if (!dfk_scons::yields(S.recs, pi)) continue;
        ++n_yield;
        for (uint64_t q = 2 * pi; q < 2 * pi + 2; ++q) {
            int64_t M = 0;
            for (uint64_t j = S.starts[q]; j < S.starts[q + 1]; ++j) M = std::max<int64_t>(M, (int64_t)S.locs[j].start + (int64_t)loc_len[j]);
            if (M != S.recs[q].M || M >= (1ll << 31)) return fail(DFK_E_ARG, "sclosures: walk %llu says M = %d, its placed records reach %lld", (unsigned long long)q, S.recs[q].M, (long long)M);
        }
    }
    // ---- the dims and the offsets (dfk_sclosures.h's check_tables)
    {
        uint64_t where = 0;
        const int bad = check_tables(n_pairs, [&](uint64_t pi) { return dfk_scons::yields(S.recs, pi); }, [&](uint64_t q) { return (int64_t)S.recs[q].M; }, [&](uint64_t q) { return S.recs[q].placed; },
                                     X.dims, X.so_starts, X.words, X.recs, &where);
        static const char* const why[] = {"the dims do not say what the walks do", "the offsets' starts do not begin at 0 or fall", "a record's state is neither 0 nor 1", "the offsets do not ascend",
                                          "a kept offset lies outside [-(n2 - 8), n1 - 8]", "a pair that does not yield has records", "the words' kept / closable do not say what the records do"};
        if (bad) return fail(DFK_E_ARG, "sclosures: pair %llu: %s", (unsigned long long)where, why[-bad - 5]);
    }
    // ---- the closable pairs (:715), their stacks alone: stack 2 i + side is side `side` of pair cp[i]
    const Closable C = closable_of(n_pairs, X.so_starts, X.recs);
    const uint64_t n_cp = C.cp.size(), n = C.cl_off.size();
    auto q_of = [&](uint64_t s) { return 2 * C.cp[s / 2] + (s & 1); };
    std::vector<uint64_t> prows(n_cp);
    for (uint64_t i = 0; i < n_cp; ++i) prows[i] = S.starts[2 * C.cp[i] + 2] - S.starts[2 * C.cp[i]];
    const std::vector<uint64_t> pfirst = prefix_sums(prows.data(), n_cp);
    const unsigned cus = (unsigned)c->prop.multiProcessorCount;
    const double t_in = wall_now();
    const uint64_t mark = c->alloc_seq;
    CnTimes times;
    float ms_lower = 0, ms_cons = 0, ms_rows = 0;
    uint64_t n_batches = 0, n_ranges = 0, n_decoded = 0, n_walked = 0, n_cells = 0, n_empty = 0, n_visits = 0, n_skipped = 0, n_erased = 0, h_dg[8] = {};
    std::vector<std::vector<uint8_t>> parts_out;                                           // the bases a batch at a time, in closure order
    std::vector<uint32_t> cl_cols(n, 0), cl_rows(n, 0);
    auto body = [&]() -> int {
        int rc;
        Timer tm(c->stream);
        CnTables T;                                                            // (of the consensus' tables only the count of streams that did not decode)
        if ((rc = c->alloc(T.bad, 8, "streams that did not decode", Place::Low))) return rc;
        HIP_TRY(hipMemsetAsync(T.bad.p, 0, 8, c->stream));
        const ConsSource CS{0, nullptr, 0, nullptr, nullptr, nullptr, nullptr, 0, nullptr, nullptr, S.rd, S.pq, S.pq_off};
        const uint64_t forced = path_switches().pidx_range_pairs;
        for (uint64_t p0 = 0; p0 < n_cp;) {
            const PidxRange range = pidx_next_range(pfirst.data(), n_cp, p0, dfk_scons::row_cap(c->largest_allocatable(), forced));
            const uint64_t p1 = range.e1, ns = 2 * (p1 - p0);
            if (!range.ok) return fail(DFK_E_ARG, "pair %llu alone has %llu rows: a range keeps 32-bit places", (unsigned long long)C.cp[p0], (unsigned long long)range.n);
            ++n_ranges;
            const uint64_t rmark = c->alloc_seq;
            // ---- the stacks of the range: the window, the live rows, what each costs a batch (host)
            const double t_h = wall_now();
            std::vector<int32_t> M(ns, 0);
            std::vector<uint64_t> n_rows(ns, 0), scost(ns, 0);
            CnRange G;
            G.h_lfirst.assign(ns + 1, 0);
            std::vector<int32_t> l_start; std::vector<uint32_t> l_len;
            for (uint64_t s = 0; s < ns; ++s) {
                const uint64_t q = q_of(2 * p0 + s);
                M[s] = S.recs[q].M; n_rows[s] = S.starts[q + 1] - S.starts[q];
                const int64_t w0 = dfk_scons::window_start(M[s]);
                scost[s] = dfk_cons::BYTES_PER_STACK;
                for (uint64_t j = S.starts[q]; j < S.starts[q + 1]; ++j) {
                    if (!dfk_scons::span_meets(S.locs[j].start, loc_len[j], w0)) continue;
                    G.h_id.push_back((uint32_t)S.locs[j].id); l_start.push_back(S.locs[j].start); l_len.push_back(loc_len[j] | (dfk_scons::row_rc(S.locs[j].fw != 0) ? 0x80000000u : 0u));
                    scost[s] += dfk_cons::live_row_cost(loc_len[j]) + 4;
                }
                G.h_lfirst[s + 1] = G.h_id.size();
            }
            const std::vector<uint64_t>& lfirst = G.h_lfirst;
            const uint64_t got = G.h_id.size();
            auto cols_of = [&](uint64_t s) { return (int64_t)M[s] - dfk_scons::window_start(M[s]); };
            // ---- the closures of the range: their widths, what they cost a batch
            const uint64_t k0 = C.cl_first[p0], nk = C.cl_first[p1] - k0;
            std::vector<uint32_t> pair_of(nk);
            std::vector<uint64_t> cost(nk);
            for (uint64_t i = p0; i < p1; ++i)
                for (uint64_t k = C.cl_first[i]; k < C.cl_first[i + 1]; ++k) {
                    const uint64_t s0 = 2 * (i - p0);
                    const int64_t cols = merged_cols(cols_of(s0 + 1), C.cl_off[k]);
                    if (cols < MM || cols > MAX_COLS) return fail(DFK_E_HIP, "sclosures: a closure of %lld columns", (long long)cols);      // (check_tables refused what leads here)
                    pair_of[k - k0] = (uint32_t)(i - p0);
                    cl_cols[k] = (uint32_t)cols;
                    cost[k - k0] = BYTES_PER_CLOSURE + scost[s0] + scost[s0 + 1];
                    n_walked += lfirst[s0 + 2] - lfirst[s0];
                }
            const std::vector<uint64_t> cfirst = prefix_sums(cost.data(), nk);
            DevBuf d_M, d_lfirst, d_lstart, d_llen;
            if ((rc = cn_up(c, d_M, M.data(), ns * 4, "stack widths")) || (rc = cn_up(c, d_lfirst, lfirst.data(), (ns + 1) * 8, "live rows per stack")) ||
                (rc = cn_up(c, d_lstart, l_start.data(), got * 4, "live rows' starts")) || (rc = cn_up(c, d_llen, l_len.data(), got * 4, "live rows' lengths"))) return rc;
            times.s_copy += wall_now() - t_h;
            // ---- the batches of closures
            for (uint64_t b0 = 0; b0 < nk;) {
                const uint64_t b1 = dfk_cons::next_batch(cfirst.data(), nk, b0, dfk_cons::batch_room(c->largest_allocatable()), per_batch), nb = b1 - b0;
                ++n_batches;
                const uint64_t bmark = c->alloc_seq;
                // the reads of the batch's pairs' stacks, each once, ascending; the gather; the decode; the lowering
                const uint64_t sa = 2 * (uint64_t)pair_of[b0], sb = 2 * (uint64_t)pair_of[b1 - 1] + 2;
                CnReads B;
                if ((rc = cn_batch_reads(c, CS, T, G, sa, sb, tm, &times, &B))) return rc;
                n_decoded += B.n_ids;
                tm.start();
                if (B.n_ids) {
                    hipLaunchKernelGGL(k_wk_lower, dim3(grid_256(B.n_ids, cus)), dim3(256), 0, c->stream, (const uint8_t*)B.bases.p, (const uint64_t*)B.bat.p, (const uint64_t*)B.qat.p, B.n_ids, (uint8_t*)B.quals.p);
                    HIP_TRY(hipGetLastError());
                }
                HIP_TRY(hipStreamSynchronize(c->stream));
                ms_lower += tm.stop();
                const double t_u = wall_now();
                std::vector<uint64_t> ofirst(nb + 1, 0), ffirst(nb + 1, 0);
                for (uint64_t k = 0; k < nb; ++k) {
                    const uint64_t s0 = 2 * (uint64_t)pair_of[b0 + k];
                    ofirst[k + 1] = ofirst[k] + cl_cols[k0 + b0 + k]; ffirst[k + 1] = ffirst[k] + (lfirst[s0 + 2] - lfirst[s0]);
                }
                const uint64_t n_out = ofirst[nb], n_flags = ffirst[nb];
                DevBuf d_pair, d_off, d_ofirst, d_ffirst, d_out, d_flags, d_cnt, d_rows;
                if ((rc = cn_up(c, d_pair, pair_of.data() + b0, nb * 4, "closures' pairs")) || (rc = cn_up(c, d_off, C.cl_off.data() + k0 + b0, nb * 4, "closures' offsets")) ||
                    (rc = cn_up(c, d_ofirst, ofirst.data(), (nb + 1) * 8, "columns per closure")) || (rc = cn_up(c, d_ffirst, ffirst.data(), (nb + 1) * 8, "flags per closure")) ||
                    (rc = c->alloc(d_out, std::max<uint64_t>(8, n_out), "closure bases", Place::Low)) || (rc = c->alloc(d_flags, std::max<uint64_t>(8, n_flags * 4), "live rows with a defined cell, a closure", Place::Low)) ||
                    (rc = c->alloc(d_cnt, nb * TILES * SCL_COUNTS * 8, "cells, empty columns, visits and skips", Place::Low)) || (rc = c->alloc(d_rows, nb * 2 * 4, "rows per closure and side", Place::Low))) return rc;
                HIP_TRY(hipMemsetAsync(d_flags.p, 0, std::max<uint64_t>(8, n_flags * 4), c->stream));
                times.s_copy += wall_now() - t_u;
                tm.start();
                const SclBatch Bk{nb, (const uint32_t*)d_pair.p, (const int32_t*)d_off.p, (const uint64_t*)d_ofirst.p, (const uint64_t*)d_ffirst.p, (const int32_t*)d_M.p, (const uint64_t*)d_lfirst.p, (const int32_t*)d_lstart.p,
                                  (const uint32_t*)d_llen.p, (const uint32_t*)B.slot.p, B.live0, (const uint64_t*)B.bat.p, (const uint64_t*)B.qat.p, (const uint8_t*)B.bases.p, (const uint8_t*)B.quals.p};
                hipLaunchKernelGGL(k_scl_closures, dim3(closures_grid(nb, cus)), dim3(GROUP), 0, c->stream, Bk, (uint8_t*)d_out.p, (uint32_t*)d_flags.p, (unsigned long long*)d_cnt.p);
                HIP_TRY(hipGetLastError());
                HIP_TRY(hipStreamSynchronize(c->stream));
                ms_cons += tm.stop();
                tm.start();
                hipLaunchKernelGGL(k_scl_rows, dim3(rows_grid(nb, cus)), dim3(256), 0, c->stream, nb, (const uint32_t*)d_pair.p, (const uint64_t*)d_ffirst.p, (const uint64_t*)d_lfirst.p, (const uint32_t*)d_flags.p, (uint32_t*)d_rows.p);
                HIP_TRY(hipGetLastError());
                std::vector<uint32_t> h_rows(2 * nb);
                HIP_TRY(hipMemcpyAsync(h_rows.data(), d_rows.p, nb * 2 * 4, hipMemcpyDeviceToHost, c->stream));
                HIP_TRY(hipStreamSynchronize(c->stream));
                ms_rows += tm.stop();
                const double t_d = wall_now();
                parts_out.emplace_back(n_out);
                std::vector<uint64_t> h_cnt(nb * TILES * SCL_COUNTS);
                if (n_out) HIP_TRY(hipMemcpyAsync(parts_out.back().data(), d_out.p, n_out, hipMemcpyDeviceToHost, c->stream));
                HIP_TRY(hipMemcpyAsync(h_cnt.data(), d_cnt.p, h_cnt.size() * 8, hipMemcpyDeviceToHost, c->stream));
                HIP_TRY(hipStreamSynchronize(c->stream));
                for (uint64_t i = 0; i < nb * TILES; ++i) { n_cells += h_cnt[SCL_COUNTS * i]; n_empty += h_cnt[SCL_COUNTS * i + 1]; n_visits += h_cnt[SCL_COUNTS * i + 2]; n_skipped += h_cnt[SCL_COUNTS * i + 3]; }
                times.s_copy += wall_now() - t_d;
                // the rows of the batch's closures: where a trim applies the rows with a defined cell in the window, else all the stack has
                for (uint64_t k = 0; k < nb; ++k) {
                    const uint64_t s0 = 2 * (uint64_t)pair_of[b0 + k];
                    const int64_t n1 = cols_of(s0), n2 = cols_of(s0 + 1), off = C.cl_off[k0 + b0 + k];
                    uint64_t rows = 0;
                    for (int side = 0; side < 2; ++side) {
                        const uint64_t s = s0 + side, kept = h_rows[2 * k + side], had = X.dims[q_of(2 * p0 + s)].rows_kept;
                        const bool cut = edge_trimmed(side, n1, n2, off);
                        if (kept > lfirst[s + 1] - lfirst[s]) return fail(DFK_E_HIP, "sclosures: %llu flags for %llu live rows", (unsigned long long)kept, (unsigned long long)(lfirst[s + 1] - lfirst[s]));
                        if (kept > had || (!cut && M[s] > MAX_WIDTH && kept != had))                 // (with a Trim to 400 only the cells can say how many rows it kept)
                            return fail(DFK_E_ARG, "sclosures: element %llu says it kept %llu rows, %llu have a defined cell in its window", (unsigned long long)q_of(2 * p0 + s), (unsigned long long)had, (unsigned long long)kept);
                        const uint64_t r = cut || M[s] > MAX_WIDTH ? kept : n_rows[s];
                        rows += r; n_erased += had - r;
                    }
                    cl_rows[k0 + b0 + k] = (uint32_t)rows;
                }
                c->release_since(bmark);
                b0 = b1;
            }
            c->release_since(rmark);
            p0 = p1;
        }
        // ---- the result in closure order, the digest
        uint64_t total = 0;
        for (const auto& p : parts_out) total += p.size();
        R->n_bases = total;
        R->bases.assign(dfk_cons::padded(total), 0);
        uint64_t at = 0;
        for (const auto& p : parts_out) { if (!p.empty()) memcpy(R->bases.data() + at, p.data(), p.size()); at += p.size(); }
        R->pair_first.assign(n_pairs + 1, 0); R->starts.assign(n + 1, 0); R->recs.assign(n, Rec{});
        for (uint64_t i = 0; i < n_cp; ++i) {
            R->pair_first[C.cp[i] + 1] = C.cl_first[i + 1] - C.cl_first[i];
            for (uint64_t k = C.cl_first[i]; k < C.cl_first[i + 1]; ++k) { R->recs[k] = Rec{(uint32_t)C.cp[i], C.cl_off[k], cl_cols[k], cl_rows[k]}; R->starts[k + 1] = R->starts[k] + cl_cols[k]; }
        }
        for (uint64_t pi = 0; pi < n_pairs; ++pi) R->pair_first[pi + 1] += R->pair_first[pi];
        if (R->starts[n] != total) return fail(DFK_E_HIP, "sclosures: %llu bases came back for %llu columns", (unsigned long long)total, (unsigned long long)R->starts[n]);
        for (uint64_t i = 0; i < total; ++i) if (R->bases[i] > 3) return fail(DFK_E_HIP, "sclosures: base %u at %llu", R->bases[i], (unsigned long long)i);
        if (n) {
            DevBuf d_r, d_b, dg;
            if ((rc = cn_up(c, d_r, R->recs.data(), n * 16, "a.stack.closures records")) || (rc = cn_up(c, d_b, R->bases.data(), total, "a.stack.closures bases")) || (rc = c->alloc(dg, 32, "sclosures digest", Place::Low))) return rc;
            HIP_TRY(hipMemsetAsync(dg.p, 0, 32, c->stream));
            hipLaunchKernelGGL(HIP_KERNEL_NAME(k_digest_seq<uint32_t>), dim3(grid_256(4 * n, cus)), dim3(256), 0, c->stream, (const uint32_t*)d_r.p, (uint64_t)(4 * n), SALT, (unsigned long long*)dg.p);
            if (total) hipLaunchKernelGGL(HIP_KERNEL_NAME(k_digest_seq<uint8_t>), dim3(grid_256(total, cus)), dim3(256), 0, c->stream, (const uint8_t*)d_b.p, total, SALT + 4 * n, (unsigned long long*)dg.p);
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
    s[DFK_SCLOSURES_PAIRS] = n_pairs; s[DFK_SCLOSURES_YIELDS] = n_yield; s[DFK_SCLOSURES_CLOSABLE] = n_cp; s[DFK_SCLOSURES_NONE] = C.none; s[DFK_SCLOSURES_OVER] = C.over; s[DFK_SCLOSURES_CLOSURES] = n;
    s[DFK_SCLOSURES_COLUMNS] = R->n_bases; s[DFK_SCLOSURES_CELLS] = n_cells; s[DFK_SCLOSURES_LIVE] = n_walked; s[DFK_SCLOSURES_ERASED] = n_erased; s[DFK_SCLOSURES_EMPTY] = n_empty;
    for (const Rec& r : R->recs) { s[DFK_SCLOSURES_SHORT] += r.cols < (uint32_t)c->cfg.K; s[DFK_SCLOSURES_ROWLESS] += r.rows == 0; }
    s[DFK_SCLOSURES_DECODED] = n_decoded; s[DFK_SCLOSURES_BATCHES] = n_batches; s[DFK_SCLOSURES_RANGES] = n_ranges; s[DFK_SCLOSURES_VISITS] = n_visits; s[DFK_SCLOSURES_SKIPPED] = n_skipped;
    s[DFK_SCLOSURES_US] = (uint64_t)(1e6 * (wall_now() - t_in)); s[DFK_SCLOSURES_US_COPY] = (uint64_t)(1e6 * times.s_copy); s[DFK_SCLOSURES_US_DECODE] = (uint64_t)(1000.0f * (times.ms_decode + ms_lower));
    s[DFK_SCLOSURES_US_CONS] = (uint64_t)(1000.0f * ms_cons); s[DFK_SCLOSURES_US_ROWS] = (uint64_t)(1000.0f * ms_rows); s[DFK_SCLOSURES_SUM] = h_dg[0]; s[DFK_SCLOSURES_XOR] = h_dg[1];
    TRACE("sclosures: %llu pairs, %llu closable, %llu closures, %llu columns (%llu empty), %llu cells, %llu live rows walked, %llu of %llu tile visits skipped, %llu rows erased, %llu reads decoded in %llu range(s), %llu batch(es); gather and copies %.1f ms, decode and lowering %.1f ms, consensus %.1f ms, rows %.1f ms",
          (unsigned long long)n_pairs, (unsigned long long)n_cp, (unsigned long long)n, (unsigned long long)R->n_bases, (unsigned long long)n_empty, (unsigned long long)n_cells, (unsigned long long)n_walked,
          (unsigned long long)n_skipped, (unsigned long long)n_visits, (unsigned long long)n_erased, (unsigned long long)n_decoded, (unsigned long long)n_ranges, (unsigned long long)n_batches, 1e3 * times.s_copy,
          times.ms_decode + ms_lower, ms_cons, ms_rows);
    return 0;
}

// the file into `dir`: whole, or not at all
int sclosures_write(const SclosuresResult* R, const std::string& dir)
{
    using namespace dfk_sclosures;
    const std::string path = dir + "/a.stack.closures";
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

// the latest dfk_sclosures_build*'s result: one a context, kept beside the graph
int sclosures_result_of(dfk_ctx* c, SclosuresResult** out)
{
    if (!c) return fail(DFK_E_ARG, "null context");
    if (!c->graph_state || !graph_of(c)->sclosures) return fail(DFK_E_STATE, "no stack closures: call dfk_sclosures_build or dfk_sclosures_build_arrays");
    *out = graph_of(c)->sclosures;
    return 0;
}
void sclosures_keep(dfk_ctx* c, SclosuresResult* R)
{
    HostGraph* G = graph_of(c);
    if (G->sclosures) sclosures_result_free(G->sclosures);
    G->sclosures = R; G->sclosures_free = sclosures_result_free;
}

// RunStages.cc:290-325: per pair Stackster's closures (:299-302), then CloseGap2's (:305-309), the pairs in order -- the thousand
// batches are consecutive ranges of pairs appended in order (:323-324), so their concatenation is exactly that.  a.closures.fastb
int allclosures_write(const SclosuresResult* A, const ClosuresResult* B, const std::string& dir, uint64_t* out)
{
    const uint64_t np = A->pair_first.size() - 1;
    std::vector<uint8_t> packed;
    std::vector<uint64_t> off(1, 0);
    std::vector<uint32_t> len;
    auto push = [&](const uint8_t* b, uint64_t n) {
        const uint64_t at = packed.size();
        packed.resize(at + (n + 3) / 4, 0);
        for (uint64_t j = 0; j < n; ++j) packed[at + (j >> 2)] |= (uint8_t)((b[j] & 3u) << (2 * (j & 3)));
        off.push_back(packed.size()); len.push_back((uint32_t)n);
    };
    uint64_t n_bases = 0;
    for (uint64_t pi = 0; pi < np; ++pi) {
        for (uint64_t k = A->pair_first[pi]; k < A->pair_first[pi + 1]; ++k) { push(A->bases.data() + A->starts[k], A->starts[k + 1] - A->starts[k]); n_bases += A->starts[k + 1] - A->starts[k]; }
        for (uint64_t k = B->pair_first[pi]; k < B->pair_first[pi + 1]; ++k) { push(B->bases.data() + B->starts[k], B->starts[k + 1] - B->starts[k]); n_bases += B->starts[k + 1] - B->starts[k]; }
    }
    if (len.size() >= (1ull << 32)) return fail(DFK_E_ARG, "%llu closures: a feudal file counts its elements in 32 bits", (unsigned long long)len.size());
    const std::string path = dir + "/a.closures.fastb";
    try { feudal::write_fastb(path, packed.data(), off, len); }
    catch (const std::runtime_error& e) { (void)unlink(path.c_str()); return fail(DFK_E_ARG, "%s", e.what()); }
    if (out) { out[0] = len.size(); out[1] = n_bases; out[2] = A->recs.size(); out[3] = B->recs.size(); }
    return 0;
}

} // namespace

extern "C" {

int dfk_sclosures_build(dfk_ctx* c, const uint8_t* packed, const uint64_t* base_off, const uint32_t* read_len, const uint8_t* pq, const uint64_t* pq_off, uint64_t n_reads)
{
    return guarded([&]() -> int {
    WalksResult* W = nullptr;
    SconsResult* K = nullptr;
    SoffsetsResult* O = nullptr;
    if (int rc = walks_result_of(c, &W)) return rc;                                         // DFK_E_STATE without walks,
    if (int rc = scons_result_of(c, &K)) return rc;                                         // without their stack consensus,
    if (int rc = soffsets_result_of(c, &O)) return rc;                                      // without its offsets,
    if (!K->walks_serial) return fail(DFK_E_STATE, "the stack consensus came from dfk_scons_build_arrays: call dfk_scons_build after dfk_walks_build");
    if (K->walks_serial != W->serial) return fail(DFK_E_STATE, "the stack consensus was made from other walks: call dfk_scons_build and dfk_soffsets_build again");
    if (!O->scons_serial) return fail(DFK_E_STATE, "the stack offsets came from dfk_soffsets_build_arrays: call dfk_soffsets_build after dfk_scons_build");
    if (O->scons_serial != K->serial) return fail(DFK_E_STATE, "the stack offsets were made from another stack consensus, of other walks: call dfk_soffsets_build again");      // and with results not made from each other
    if (n_reads != W->n_reads) return fail(DFK_E_ARG, "sclosures: %llu reads given, the walks were made from %llu", (unsigned long long)n_reads, (unsigned long long)W->n_reads);
    const uint64_t n_pairs = W->recs.size() / 2;
    if (K->dims.size() != W->recs.size() || O->words.size() != n_pairs || O->starts.size() != n_pairs + 1) return fail(DFK_E_STATE, "the stack consensus or the stack offsets are not those of the walks' %llu pairs", (unsigned long long)n_pairs);
    PartnerReads reads;
    if (int rc = walks_reads(packed, base_off, read_len, pq, pq_off, n_reads, &reads)) return rc;
    HIP_TRY(hipSetDevice(c->device));
    const dfk_walks::Rec no_rec{}; const dfk_walks::Loc no_loc{}; const dfk_scons::Dim no_dim{}; const dfk_soffsets::PairWords no_words{}; const dfk_soffsets::Rec no_so{};
    const SclosuresSource X{SconsSource{n_pairs, W->starts.data(), W->recs.empty() ? &no_rec : W->recs.data(), W->locs.empty() ? &no_loc : W->locs.data(), &reads, pq, pq_off},
                            K->dims.empty() ? &no_dim : K->dims.data(), O->starts.data(), O->words.empty() ? &no_words : O->words.data(), O->recs.empty() ? &no_so : O->recs.data()};
    std::unique_ptr<SclosuresResult> R(new SclosuresResult);
    if (int rc = sclosures_build(c, X, 0, R.get())) return rc;                              // (refused: the earlier result is still served)
    R->pairs = W->pairs; R->from_chain = true;
    sclosures_keep(c, R.release());
    return 0;
    });
}

// The stage on host arrays: the walks in dfk_walks_fetch's forms, the reads, dims in dfk_scons_fetch's form, the offsets in
// dfk_soffsets_fetch's forms, checked here.
int dfk_sclosures_build_arrays(dfk_ctx* c, const uint64_t* starts, const uint32_t* records, const void* placed, uint64_t n_pairs, const uint8_t* packed, const uint64_t* base_off, const uint32_t* read_len,
                               const uint8_t* pq, const uint64_t* pq_off, uint64_t n_reads, const uint32_t* dims, const uint64_t* so_starts, const uint32_t* so_words, const void* so_records,
                               uint64_t closures_per_batch, const char* dir)
{
    return guarded([&]() -> int {
    if (!c) return fail(DFK_E_ARG, "null context");
    if (!starts || !so_starts || (n_pairs && (!records || !dims || !so_words))) return fail(DFK_E_ARG, "null argument");
    if (n_reads >= (1ull << 31) || n_pairs >= (1ull << 30)) return fail(DFK_E_ARG, "%llu reads, %llu pairs: 2^31 - 1 reads and 2^30 - 1 pairs at most", (unsigned long long)n_reads, (unsigned long long)n_pairs);
    if (starts[0] != 0 || so_starts[0] != 0) return fail(DFK_E_ARG, "the tables do not start at 0");
    for (uint64_t q = 0; q < 2 * n_pairs; ++q) if (starts[q + 1] < starts[q]) return fail(DFK_E_ARG, "the walks' starts fall at walk %llu", (unsigned long long)q);
    for (uint64_t p = 0; p < n_pairs; ++p) if (so_starts[p + 1] < so_starts[p]) return fail(DFK_E_ARG, "the offsets' starts fall at pair %llu", (unsigned long long)p);
    if ((starts[2 * n_pairs] && !placed) || (so_starts[n_pairs] && !so_records)) return fail(DFK_E_ARG, "null argument");
    PartnerReads reads;
    if (int rc = walks_reads(packed, base_off, read_len, pq, pq_off, n_reads, &reads)) return rc;
    HIP_TRY(hipSetDevice(c->device));
    const dfk_walks::Rec no_rec{}; const dfk_walks::Loc no_loc{}; const dfk_scons::Dim no_dim{}; const dfk_soffsets::PairWords no_words{}; const dfk_soffsets::Rec no_so{};
    const SclosuresSource X{SconsSource{n_pairs, starts, n_pairs ? (const dfk_walks::Rec*)records : &no_rec, placed ? (const dfk_walks::Loc*)placed : &no_loc, &reads, pq, pq_off},
                            n_pairs ? (const dfk_scons::Dim*)dims : &no_dim, so_starts, n_pairs ? (const dfk_soffsets::PairWords*)so_words : &no_words, so_records ? (const dfk_soffsets::Rec*)so_records : &no_so};
    std::unique_ptr<SclosuresResult> R(new SclosuresResult);
    if (int rc = sclosures_build(c, X, closures_per_batch, R.get())) return rc;
    if (dir) if (int rc = sclosures_write(R.get(), dir)) return rc;
    sclosures_keep(c, R.release());
    return 0;
    });
}

int dfk_sclosures_stats(dfk_ctx* c, uint64_t* out)
{
    return guarded([&]() -> int {
    SclosuresResult* R = nullptr;
    if (int rc = sclosures_result_of(c, &R)) return rc;
    if (!out) return fail(DFK_E_ARG, "null argument");
    for (int i = 0; i < DFK_SCLOSURES_WORDS; ++i) out[i] = R->stats[i];
    return 0;
    });
}

int dfk_sclosures_fetch(dfk_ctx* c, uint64_t* pair_first, uint64_t* starts, uint32_t* records, uint64_t* n_pairs, uint64_t* n_closures, uint8_t* bases, uint64_t bases_cap, uint64_t* n_bases)
{
    return guarded([&]() -> int {
    SclosuresResult* R = nullptr;
    if (int rc = sclosures_result_of(c, &R)) return rc;
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

int dfk_sclosures_write(dfk_ctx* c, const char* dir)
{
    return guarded([&]() -> int {
    SclosuresResult* R = nullptr;
    if (int rc = sclosures_result_of(c, &R)) return rc;
    if (!dir) return fail(DFK_E_ARG, "null directory");
    return sclosures_write(R, dir);
    });
}

int dfk_allclosures_write(dfk_ctx* c, const char* dir, uint64_t* out)
{
    return guarded([&]() -> int {
    if (!c) return fail(DFK_E_ARG, "null context");
    if (!c->graph_state || !graph_of(c)->sclosures || !graph_of(c)->sclosures->from_chain) return fail(DFK_E_STATE, "no stack closures of this context's walks: call dfk_sclosures_build");
    if (!graph_of(c)->closures) return fail(DFK_E_STATE, "no closures of the first closer: call dfk_closures_build");
    const SclosuresResult* A = graph_of(c)->sclosures;
    const ClosuresResult* B = graph_of(c)->closures;
    if (B->pairs.empty() && B->pair_first.size() > 1) return fail(DFK_E_STATE, "the first closer's closures came from dfk_closures_build_arrays: call dfk_closures_build");
    if (A->pairs != B->pairs || A->pair_first.size() != B->pair_first.size()) return fail(DFK_E_STATE, "the two closers' closures were not made for the same pairs: build both chains for one set of pairs");
    if (!dir) return fail(DFK_E_ARG, "null directory");
    return allclosures_write(A, B, dir, out);
    });
}

} // extern "C"
