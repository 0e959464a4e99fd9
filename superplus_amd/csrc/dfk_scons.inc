// superplus_amd/csrc/dfk_scons.inc -- Stackster's stack consensus per pair (10X/Stackster.cc:396-489, :546-563; ReadStack.cc's Trim,
// Reverse and Consensus1 with qualities) and the file a.stack.cons, included by dfk.hip.
//
// The rule, the shared pieces, the plan and the file's layout: dfk_scons.h.  The kernels: dfk_scons_kernels.h.  Here: scons_build() -- a
// range of whole pairs at a time the stacks' windows and live rows from the walks' placed records (host), under it the batches of
// stacks: the reads their live rows name gathered once each, decoded and lowered (dfk_cons.inc's cn_batch_reads, k_wk_lower), the
// consensus a workgroup a tile of a stack; then the flat pass and the conflicts over the range, everything coming back once a range --
// and scons_write().  Everything on the device comes from the arena and goes back before build returns.
#include "dfk_scons_kernels.h"

namespace {

struct SconsResult {
    std::vector<uint64_t> starts;                 // [2 * n_pairs + 1], in columns
    std::vector<uint64_t> cfirst;                 // [n_pairs + 1], in conflict entries
    std::vector<dfk_scons::Dim> dims;             // [2 * n_pairs]
    std::vector<uint8_t> con, conq;
    std::vector<uint16_t> counts;
    uint64_t stats[DFK_SCONS_WORDS] = {};
    uint64_t walks_serial = 0;                    // dfk_scons_build: the walks it was made from (0: from arrays); dfk_soffsets_build asks
    uint64_t serial = 0;                          // dfk_scons_build: which build made it; dfk_soffsets_build notes it, dfk_sclosures_build asks for the same
};
void scons_result_free(SconsResult* r) { delete r; }

struct SconsSource {
    uint64_t n_pairs; const uint64_t* starts; const dfk_walks::Rec* recs; const dfk_walks::Loc* locs;
    const PartnerReads* rd; const uint8_t* pq; const uint64_t* pq_off;
};

int scons_build(dfk_ctx* c, const SconsSource& S, uint64_t stacks_per_batch, SconsResult* R)
{
    using namespace dfk_scons;
    const uint64_t N = S.rd->n, n_pairs = S.n_pairs, n_stacks = 2 * n_pairs;
    if (N > (1ull << 31) || n_pairs >= (1ull << 30)) return fail(DFK_E_ARG, "%llu reads, %llu pairs: a row keeps its read in 31 bits", (unsigned long long)N, (unsigned long long)n_pairs);
    // ---- the walks' tables, checked (dfk_scons.h's check_walks, the lengths through host_read)
    if (S.starts[0] != 0) return fail(DFK_E_ARG, "scons: the walks' starts do not begin at 0");
    for (uint64_t q = 0; q < n_stacks; ++q)
        if (S.starts[q + 1] < S.starts[q] || S.starts[q + 1] - S.starts[q] != S.recs[q].placed) return fail(DFK_E_ARG, "scons: the walks' starts fall or leave walk %llu other than its %u placed records", (unsigned long long)q, S.recs[q].placed);
    const uint64_t n_locs = S.starts[n_stacks];
    std::vector<uint32_t> loc_len(n_locs + 1, 0);
    for (uint64_t j = 0; j < n_locs; ++j) {
        const dfk_walks::Loc& L = S.locs[j];
        if (L.id < 0 || (uint64_t)L.id >= N) return fail(DFK_E_ARG, "a placed record names read %lld of %llu", (long long)L.id, (unsigned long long)N);
        if (L.start <= -(1 << 30) || L.start >= (1 << 30) || L.fw > 1) return fail(DFK_E_ARG, "a placed record lies at %d with the flag %u", L.start, L.fw);
        if (int rc = host_read(c, &loc_len[j], S.rd->len + L.id, 4)) return rc;
    }
    std::vector<uint64_t> prows(n_pairs, 0);
    uint64_t n_yield = 0;
    for (uint64_t pi = 0; pi < n_pairs; ++pi) {
        if (!yields(S.recs, pi)) continue;
        ++n_yield;
        prows[pi] = S.starts[2 * pi + 2] - S.starts[2 * pi];
        for (uint64_t q = 2 * pi; q < 2 * pi + 2; ++q) {
            int64_t M = 0;
            for (uint64_t j = S.starts[q]; j < S.starts[q + 1]; ++j) M = std::max<int64_t>(M, (int64_t)S.locs[j].start + (int64_t)loc_len[j]);
            if (M != S.recs[q].M || M >= (1ll << 31)) return fail(DFK_E_ARG, "scons: walk %llu says M = %d, its placed records reach %lld", (unsigned long long)q, S.recs[q].M, (long long)M);
        }
    }
    const std::vector<uint64_t> pfirst = prefix_sums(prows.data(), n_pairs);
    const unsigned cus = (unsigned)c->prop.multiProcessorCount;
    const double t_in = wall_now();
    const uint64_t mark = c->alloc_seq;
    CnTimes times;
    float ms_lower = 0, ms_cons = 0, ms_flat = 0, ms_conf = 0;
    uint64_t n_batches = 0, n_ranges = 0, n_decoded = 0, n_cells = 0, n_capped = 0, n_recount = 0, n_flat = 0, n_allowed = 0, n_disallowed = 0, n_live = 0, h_dg[8] = {};
    R->starts.assign(1, 0); R->cfirst.assign(1, 0); R->dims.clear(); R->con.clear(); R->conq.clear(); R->counts.clear();
    auto body = [&]() -> int {
        int rc;
        Timer tm(c->stream);
        CnTables T;                                                            // (of the consensus' tables only the count of streams that did not decode)
        if ((rc = c->alloc(T.bad, 8, "streams that did not decode", Place::Low))) return rc;
        HIP_TRY(hipMemsetAsync(T.bad.p, 0, 8, c->stream));
        const ConsSource CS{0, nullptr, 0, nullptr, nullptr, nullptr, nullptr, 0, nullptr, nullptr, S.rd, S.pq, S.pq_off};
        const uint64_t forced = path_switches().pidx_range_pairs;
        for (uint64_t p0 = 0; p0 < n_pairs;) {
            const PidxRange range = pidx_next_range(pfirst.data(), n_pairs, p0, row_cap(c->largest_allocatable(), forced));
            const uint64_t p1 = range.e1, np = p1 - p0, ns = 2 * np;
            if (!range.ok) return fail(DFK_E_ARG, "pair %llu alone has %llu rows: a range keeps 32-bit places", (unsigned long long)p0, (unsigned long long)range.n);
            ++n_ranges;
            const uint64_t rmark = c->alloc_seq;
            // ---- the stacks of the range: the window, the live rows, the columns, the conflict entries, what each costs a batch (host)
            const double t_h = wall_now();
            std::vector<int32_t> M(ns, 0);
            std::vector<uint64_t> n_rows(ns, 0), ofirst(ns + 1, 0), cost(ns, 0), cnt_first(np + 1, 0);
            CnRange G;
            G.h_lfirst.assign(ns + 1, 0);
            std::vector<int32_t> l_start; std::vector<uint32_t> l_len;
            for (uint64_t s = 0; s < ns; ++s) {
                const uint64_t q = 2 * p0 + s;
                if (yields(S.recs, q / 2)) {
                    M[s] = S.recs[q].M; n_rows[s] = S.starts[q + 1] - S.starts[q];
                    const int64_t w0 = window_start(M[s]);
                    for (uint64_t j = S.starts[q]; j < S.starts[q + 1]; ++j) {
                        if (!span_meets(S.locs[j].start, loc_len[j], w0)) continue;
                        G.h_id.push_back((uint32_t)S.locs[j].id); l_start.push_back(S.locs[j].start); l_len.push_back(loc_len[j] | (row_rc(S.locs[j].fw != 0) ? 0x80000000u : 0u));
                    }
                }
                G.h_lfirst[s + 1] = G.h_id.size(); ofirst[s + 1] = ofirst[s] + (uint64_t)(M[s] - window_start(M[s]));
                cost[s] = dfk_cons::BYTES_PER_STACK;
                for (uint64_t l = G.h_lfirst[s]; l < G.h_lfirst[s + 1]; ++l) cost[s] += dfk_cons::live_row_cost(l_len[l] & 0x7FFFFFFFu);
            }
            for (uint64_t p = 0; p < np; ++p) cnt_first[p + 1] = cnt_first[p] + (yields(S.recs, p0 + p) ? ofirst[2 * p + 2] - ofirst[2 * p] : 0);
            const uint64_t got = G.h_id.size(), n_cols = ofirst[ns], n_cnt = cnt_first[np];
            n_live += got;
            const std::vector<uint64_t> cfirst = prefix_sums(cost.data(), ns);
            DevBuf d_M, d_ofirst, d_lfirst, d_lstart, d_llen, d_def, d_con, d_conq, d_cntfirst, d_counts, d_flat;
            const unsigned flat_grid = std::max(1u, grid_256(n_cols, cus));
            if ((rc = cn_up(c, d_M, M.data(), ns * 4, "stack widths")) || (rc = cn_up(c, d_ofirst, ofirst.data(), (ns + 1) * 8, "columns per stack")) ||
                (rc = cn_up(c, d_lfirst, G.h_lfirst.data(), (ns + 1) * 8, "live rows per stack")) || (rc = cn_up(c, d_lstart, l_start.data(), got * 4, "live rows' starts")) ||
                (rc = cn_up(c, d_llen, l_len.data(), got * 4, "live rows' lengths")) || (rc = c->alloc(d_def, std::max<uint64_t>(8, got * 4), "live rows with a defined cell", Place::Low)) ||
                (rc = c->alloc(d_con, std::max<uint64_t>(8, n_cols), "consensus bases", Place::Low)) || (rc = c->alloc(d_conq, std::max<uint64_t>(8, n_cols), "consensus qualities", Place::Low)) ||
                (rc = cn_up(c, d_cntfirst, cnt_first.data(), (np + 1) * 8, "conflict entries per pair")) || (rc = c->alloc(d_counts, std::max<uint64_t>(8, n_cnt * 2), "conflict counts", Place::Low)) ||
                (rc = c->alloc(d_flat, flat_grid * 8ull, "flat columns", Place::Low))) return rc;
            HIP_TRY(hipMemsetAsync(d_def.p, 0, std::max<uint64_t>(8, got * 4), c->stream));
            times.s_copy += wall_now() - t_h;
            // ---- the batches of stacks
            for (uint64_t b0 = 0; b0 < ns;) {
                const uint64_t b1 = dfk_cons::next_batch(cfirst.data(), ns, b0, dfk_cons::batch_room(c->largest_allocatable()), stacks_per_batch), nb = b1 - b0;
                ++n_batches;
                const uint64_t bmark = c->alloc_seq;
                // the reads of the batch, each once, ascending; the gather; the decode; the lowering
                CnReads B;
                if ((rc = cn_batch_reads(c, CS, T, G, b0, b1, tm, &times, &B))) return rc;
                n_decoded += B.n_ids;
                tm.start();
                if (B.n_ids) {
                    hipLaunchKernelGGL(k_wk_lower, dim3(grid_256(B.n_ids, cus)), dim3(256), 0, c->stream, (const uint8_t*)B.bases.p, (const uint64_t*)B.bat.p, (const uint64_t*)B.qat.p, B.n_ids, (uint8_t*)B.quals.p);
                    HIP_TRY(hipGetLastError());
                }
                DevBuf d_cnt;
                if ((rc = c->alloc(d_cnt, nb * TILES * SC_COUNTS * 8, "cells, capped and recounted columns", Place::Low))) return rc;
                HIP_TRY(hipStreamSynchronize(c->stream));
                ms_lower += tm.stop();
                tm.start();
                const ScBatch Bk{b0, nb, (const int32_t*)d_M.p, (const uint64_t*)d_ofirst.p, (const uint64_t*)d_lfirst.p, (const int32_t*)d_lstart.p, (const uint32_t*)d_llen.p, (const uint32_t*)B.slot.p, B.live0,
                                 (const uint64_t*)B.bat.p, (const uint64_t*)B.qat.p, (const uint8_t*)B.bases.p, (const uint8_t*)B.quals.p};
                hipLaunchKernelGGL(k_sc_consensus, dim3(cons_grid(nb, cus)), dim3(GROUP), 0, c->stream, Bk, (uint8_t*)d_con.p, (uint8_t*)d_conq.p, (uint32_t*)d_def.p, (unsigned long long*)d_cnt.p);
                HIP_TRY(hipGetLastError());
                std::vector<uint64_t> h_cnt(nb * TILES * SC_COUNTS);
                HIP_TRY(hipMemcpyAsync(h_cnt.data(), d_cnt.p, h_cnt.size() * 8, hipMemcpyDeviceToHost, c->stream));
                HIP_TRY(hipStreamSynchronize(c->stream));
                ms_cons += tm.stop();
                for (uint64_t i = 0; i < nb * TILES; ++i) { n_cells += h_cnt[SC_COUNTS * i]; n_capped += h_cnt[SC_COUNTS * i + 1]; n_recount += h_cnt[SC_COUNTS * i + 2]; }
                c->release_since(bmark);
                b0 = b1;
            }
            // ---- the flat pass over the range's columns, then the conflicts of its pairs
            std::vector<uint8_t> h_con(n_cols + 1), h_conq(n_cols + 1);
            std::vector<uint16_t> h_counts(n_cnt + 1);
            std::vector<uint32_t> h_def(got + 1);
            std::vector<uint64_t> h_flat(flat_grid, 0);
            if (n_cols) {
                tm.start();
                hipLaunchKernelGGL(k_sc_flat, dim3(flat_grid), dim3(256), 0, c->stream, (const uint8_t*)d_con.p, (const uint64_t*)d_ofirst.p, ns, n_cols, (uint8_t*)d_conq.p, (unsigned long long*)d_flat.p);
                HIP_TRY(hipGetLastError());
                HIP_TRY(hipMemcpyAsync(h_flat.data(), d_flat.p, flat_grid * 8ull, hipMemcpyDeviceToHost, c->stream));
                HIP_TRY(hipStreamSynchronize(c->stream));
                ms_flat += tm.stop();
                for (uint64_t x : h_flat) n_flat += x;
            }
            if (n_cnt) {
                for (uint64_t s = 0; s < ns; ++s) if (ofirst[s + 1] - ofirst[s] > (uint64_t)MAX_WIDTH) return fail(DFK_E_HIP, "scons: a stack of %llu columns", (unsigned long long)(ofirst[s + 1] - ofirst[s]));
                tm.start();
                hipLaunchKernelGGL(k_sc_conflicts, dim3(pair_grid(np, cus)), dim3(256), 0, c->stream, (const uint8_t*)d_con.p, (const uint8_t*)d_conq.p, (const uint64_t*)d_ofirst.p, (const uint64_t*)d_cntfirst.p, np, (uint16_t*)d_counts.p);
                HIP_TRY(hipGetLastError());
                HIP_TRY(hipStreamSynchronize(c->stream));
                ms_conf += tm.stop();
            }
            const double t_d = wall_now();
            if (n_cols) { HIP_TRY(hipMemcpyAsync(h_con.data(), d_con.p, n_cols, hipMemcpyDeviceToHost, c->stream)); HIP_TRY(hipMemcpyAsync(h_conq.data(), d_conq.p, n_cols, hipMemcpyDeviceToHost, c->stream)); }
            if (n_cnt) HIP_TRY(hipMemcpyAsync(h_counts.data(), d_counts.p, n_cnt * 2, hipMemcpyDeviceToHost, c->stream));
            if (got) HIP_TRY(hipMemcpyAsync(h_def.data(), d_def.p, got * 4, hipMemcpyDeviceToHost, c->stream));
            HIP_TRY(hipStreamSynchronize(c->stream));
            times.s_copy += wall_now() - t_d;
            // ---- the range's share of the result, checked
            for (uint64_t i = 0; i < n_cols; ++i) if (h_con[i] > 3 || h_conq[i] > QUALCAP) return fail(DFK_E_HIP, "scons: base %u with quality %u at column %llu of the range", h_con[i], h_conq[i], (unsigned long long)i);
            for (uint64_t i = 0; i < n_cnt; ++i) {
                if (h_counts[i] > MAX_WIDTH) return fail(DFK_E_HIP, "scons: %u conflicts at an offset", h_counts[i]);
                if (h_counts[i] < CONFLICTS) ++n_allowed; else ++n_disallowed;
            }
            for (uint64_t s = 0; s < ns; ++s) {
                uint64_t kept = 0;
                for (uint64_t l = G.h_lfirst[s]; l < G.h_lfirst[s + 1]; ++l) { if (h_def[l] > 1) return fail(DFK_E_HIP, "scons: flag %u at live row %llu", h_def[l], (unsigned long long)l); kept += h_def[l]; }
                R->dims.push_back(Dim{(uint32_t)n_rows[s], (uint32_t)(M[s] > MAX_WIDTH ? kept : n_rows[s]), M[s], (uint32_t)(ofirst[s + 1] - ofirst[s])});
                R->starts.push_back(R->starts.back() + (ofirst[s + 1] - ofirst[s]));
            }
            for (uint64_t p = 0; p < np; ++p) R->cfirst.push_back(R->cfirst.back() + (cnt_first[p + 1] - cnt_first[p]));
            R->con.insert(R->con.end(), h_con.begin(), h_con.begin() + n_cols); R->conq.insert(R->conq.end(), h_conq.begin(), h_conq.begin() + n_cols);
            R->counts.insert(R->counts.end(), h_counts.begin(), h_counts.begin() + n_cnt);
            c->release_since(rmark);
            p0 = p1;
        }
        // ---- the digest: the dims, con, conq, the counts
        const uint64_t total = R->con.size(), n_cnt = R->counts.size();
        if (n_stacks) {
            DevBuf d_dims, d_a, d_b, d_c, dg;
            if ((rc = cn_up(c, d_dims, R->dims.data(), n_stacks * 16, "a.stack.cons dims")) || (rc = cn_up(c, d_a, R->con.data(), total, "a.stack.cons bases")) || (rc = cn_up(c, d_b, R->conq.data(), total, "a.stack.cons qualities")) ||
                (rc = cn_up(c, d_c, R->counts.data(), n_cnt * 2, "a.stack.cons conflict counts")) || (rc = c->alloc(dg, 32, "scons digest", Place::Low))) return rc;
            HIP_TRY(hipMemsetAsync(dg.p, 0, 32, c->stream));
            hipLaunchKernelGGL(HIP_KERNEL_NAME(k_digest_seq<uint32_t>), dim3(grid_256(4 * n_stacks, cus)), dim3(256), 0, c->stream, (const uint32_t*)d_dims.p, (uint64_t)(4 * n_stacks), SALT, (unsigned long long*)dg.p);
            if (total) {
                hipLaunchKernelGGL(HIP_KERNEL_NAME(k_digest_seq<uint8_t>), dim3(grid_256(total, cus)), dim3(256), 0, c->stream, (const uint8_t*)d_a.p, total, SALT + 4 * n_stacks, (unsigned long long*)dg.p);
                hipLaunchKernelGGL(HIP_KERNEL_NAME(k_digest_seq<uint8_t>), dim3(grid_256(total, cus)), dim3(256), 0, c->stream, (const uint8_t*)d_b.p, total, SALT + 4 * n_stacks + total, (unsigned long long*)dg.p);
            }
            if (n_cnt) hipLaunchKernelGGL(HIP_KERNEL_NAME(k_digest_seq<uint16_t>), dim3(grid_256(n_cnt, cus)), dim3(256), 0, c->stream, (const uint16_t*)d_c.p, n_cnt, SALT + 4 * n_stacks + 2 * total, (unsigned long long*)dg.p);
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
    if (R->dims.size() != n_stacks || R->cfirst.size() != n_pairs + 1) return fail(DFK_E_HIP, "scons: %llu elements for %llu stacks", (unsigned long long)R->dims.size(), (unsigned long long)n_stacks);
    uint64_t* s = R->stats;
    s[DFK_SCONS_PAIRS] = n_pairs; s[DFK_SCONS_YIELDS] = n_yield; s[DFK_SCONS_STACKS] = 2 * n_yield; s[DFK_SCONS_LIVE] = n_live; s[DFK_SCONS_COLUMNS] = R->con.size(); s[DFK_SCONS_CELLS] = n_cells;
    s[DFK_SCONS_CAPPED] = n_capped; s[DFK_SCONS_RECOUNT] = n_recount; s[DFK_SCONS_FLAT] = n_flat; s[DFK_SCONS_ALLOWED] = n_allowed; s[DFK_SCONS_DISALLOWED] = n_disallowed;
    s[DFK_SCONS_DECODED] = n_decoded; s[DFK_SCONS_BATCHES] = n_batches; s[DFK_SCONS_RANGES] = n_ranges;
    for (const Dim& d : R->dims) { s[DFK_SCONS_ROWS] += d.rows; s[DFK_SCONS_ROWS_KEPT] += d.rows_kept; s[DFK_SCONS_TRIMMED] += d.M > MAX_WIDTH; }
    s[DFK_SCONS_US] = (uint64_t)(1e6 * (wall_now() - t_in)); s[DFK_SCONS_US_COPY] = (uint64_t)(1e6 * times.s_copy); s[DFK_SCONS_US_DECODE] = (uint64_t)(1000.0f * (times.ms_decode + ms_lower));
    s[DFK_SCONS_US_CONS] = (uint64_t)(1000.0f * ms_cons); s[DFK_SCONS_US_FLAT] = (uint64_t)(1000.0f * ms_flat); s[DFK_SCONS_US_CONFLICTS] = (uint64_t)(1000.0f * ms_conf);
    s[DFK_SCONS_SUM] = h_dg[0]; s[DFK_SCONS_XOR] = h_dg[1];
    TRACE("scons: %llu pairs, %llu yielding, %llu rows (%llu live, %llu kept), %llu stacks trimmed, %llu columns (%llu capped, %llu recounted, %llu flat), %llu cells, %llu offsets allowed of %llu, %llu reads decoded in %llu range(s), %llu batch(es); gather and copies %.1f ms, decode and lowering %.1f ms, consensus %.1f ms, flat %.1f ms, conflicts %.1f ms",
          (unsigned long long)n_pairs, (unsigned long long)n_yield, (unsigned long long)s[DFK_SCONS_ROWS], (unsigned long long)n_live, (unsigned long long)s[DFK_SCONS_ROWS_KEPT], (unsigned long long)s[DFK_SCONS_TRIMMED],
          (unsigned long long)R->con.size(), (unsigned long long)n_capped, (unsigned long long)n_recount, (unsigned long long)n_flat, (unsigned long long)n_cells, (unsigned long long)n_allowed, (unsigned long long)(n_allowed + n_disallowed),
          (unsigned long long)n_decoded, (unsigned long long)n_ranges, (unsigned long long)n_batches, 1e3 * times.s_copy, times.ms_decode + ms_lower, ms_cons, ms_flat, ms_conf);
    return 0;
}

// the file into `dir`: whole, or not at all
int scons_write(const SconsResult* R, const std::string& dir)
{
    using namespace dfk_scons;
    const std::string path = dir + "/a.stack.cons";
    const uint64_t n = R->dims.size(), nc = R->con.size(), nk = R->counts.size();
    std::vector<uint8_t> tail(file_size(n, nc, nk) - con_at(n), 0);                         // con, conq, the counts, the zero bytes
    if (nc) { memcpy(tail.data(), R->con.data(), nc); memcpy(tail.data() + nc, R->conq.data(), nc); }
    if (nk) memcpy(tail.data() + 2 * nc, R->counts.data(), 2 * nk);
    const int fd = open(path.c_str(), O_WRONLY | O_CREAT | O_TRUNC, 0666);
    if (fd < 0) return fail(DFK_E_ARG, "cannot open %s", path.c_str());
    const dfk_closer::BinHead h = dfk_closer::head_of(MAGIC, n);
    bool bad = pwrite_all(fd, &h, 16, 0) != 0 || pwrite_all(fd, R->starts.data(), 8 * (n + 1), 16) != 0 || pwrite_all(fd, R->cfirst.data(), 8 * (n / 2 + 1), cfirst_at(n)) != 0;
    if (!bad && n) bad = pwrite_all(fd, R->dims.data(), 16 * n, dims_at(n)) != 0;
    if (!bad && !tail.empty()) bad = pwrite_all(fd, tail.data(), tail.size(), con_at(n)) != 0;
    if (close(fd) != 0) bad = true;
    if (bad) { (void)unlink(path.c_str()); return fail(DFK_E_ARG, "short write to %s", path.c_str()); }
    return 0;
}

// the latest dfk_scons_build*'s result: one a context, kept beside the graph
int scons_result_of(dfk_ctx* c, SconsResult** out)
{
    if (!c) return fail(DFK_E_ARG, "null context");
    if (!c->graph_state || !graph_of(c)->scons) return fail(DFK_E_STATE, "no stack consensus of the walks: call dfk_scons_build or dfk_scons_build_arrays");
    *out = graph_of(c)->scons;
    return 0;
}
void scons_keep(dfk_ctx* c, SconsResult* R)
{
    HostGraph* G = graph_of(c);
    if (G->scons) scons_result_free(G->scons);
    G->scons = R; G->scons_free = scons_result_free;
}

} // namespace

extern "C" {

int dfk_scons_build(dfk_ctx* c, const uint8_t* packed, const uint64_t* base_off, const uint32_t* read_len, const uint8_t* pq, const uint64_t* pq_off, uint64_t n_reads)
{
    return guarded([&]() -> int {
    WalksResult* W = nullptr;
    if (int rc = walks_result_of(c, &W)) return rc;                                         // DFK_E_STATE without walks
    if (n_reads != W->n_reads) return fail(DFK_E_ARG, "scons: %llu reads given, the walks were made from %llu", (unsigned long long)n_reads, (unsigned long long)W->n_reads);
    PartnerReads reads;
    if (int rc = walks_reads(packed, base_off, read_len, pq, pq_off, n_reads, &reads)) return rc;
    HIP_TRY(hipSetDevice(c->device));
    const dfk_walks::Rec no_rec{}; const dfk_walks::Loc no_loc{};
    const SconsSource S{W->recs.size() / 2, W->starts.data(), W->recs.empty() ? &no_rec : W->recs.data(), W->locs.empty() ? &no_loc : W->locs.data(), &reads, pq, pq_off};
    std::unique_ptr<SconsResult> R(new SconsResult);
    if (int rc = scons_build(c, S, 0, R.get())) return rc;                                  // (refused: the earlier result is still served)
    R->walks_serial = W->serial; R->serial = cons_next_serial();
    scons_keep(c, R.release());
    return 0;
    });
}

// The stage on host arrays: the walks in dfk_walks_fetch's forms and the reads, checked here.
int dfk_scons_build_arrays(dfk_ctx* c, const uint64_t* starts, const uint32_t* records, const void* placed, uint64_t n_pairs, const uint8_t* packed, const uint64_t* base_off, const uint32_t* read_len,
                           const uint8_t* pq, const uint64_t* pq_off, uint64_t n_reads, uint64_t stacks_per_batch, const char* dir)
{
    return guarded([&]() -> int {
    if (!c) return fail(DFK_E_ARG, "null context");
    if (!starts || (n_pairs && !records)) return fail(DFK_E_ARG, "null argument");
    if (n_reads >= (1ull << 31) || n_pairs >= (1ull << 30)) return fail(DFK_E_ARG, "%llu reads, %llu pairs: 2^31 - 1 reads and 2^30 - 1 pairs at most", (unsigned long long)n_reads, (unsigned long long)n_pairs);
    if (starts[0] != 0) return fail(DFK_E_ARG, "the tables do not start at 0");
    for (uint64_t q = 0; q < 2 * n_pairs; ++q) if (starts[q + 1] < starts[q]) return fail(DFK_E_ARG, "the walks' starts fall at walk %llu", (unsigned long long)q);
    if (starts[2 * n_pairs] && !placed) return fail(DFK_E_ARG, "null argument");
    PartnerReads reads;
    if (int rc = walks_reads(packed, base_off, read_len, pq, pq_off, n_reads, &reads)) return rc;
    HIP_TRY(hipSetDevice(c->device));
    const dfk_walks::Rec no_rec{}; const dfk_walks::Loc no_loc{};
    const SconsSource S{n_pairs, starts, n_pairs ? (const dfk_walks::Rec*)records : &no_rec, placed ? (const dfk_walks::Loc*)placed : &no_loc, &reads, pq, pq_off};
    std::unique_ptr<SconsResult> R(new SconsResult);
    if (int rc = scons_build(c, S, stacks_per_batch, R.get())) return rc;
    if (dir) if (int rc = scons_write(R.get(), dir)) return rc;
    scons_keep(c, R.release());
    return 0;
    });
}

int dfk_scons_stats(dfk_ctx* c, uint64_t* out)
{
    return guarded([&]() -> int {
    SconsResult* R = nullptr;
    if (int rc = scons_result_of(c, &R)) return rc;
    if (!out) return fail(DFK_E_ARG, "null argument");
    for (int i = 0; i < DFK_SCONS_WORDS; ++i) out[i] = R->stats[i];
    return 0;
    });
}

int dfk_scons_fetch(dfk_ctx* c, uint64_t* starts, uint64_t* conflict_first, uint32_t* dims, uint64_t* n_elements, uint8_t* con, uint8_t* conq, uint64_t cols_cap, uint64_t* n_cols, uint16_t* counts, uint64_t counts_cap,
                    uint64_t* n_counts)
{
    return guarded([&]() -> int {
    SconsResult* R = nullptr;
    if (int rc = scons_result_of(c, &R)) return rc;
    const uint64_t n = R->dims.size(), nc = R->con.size(), nk = R->counts.size();
    if (n_elements) *n_elements = n;
    if (n_cols) *n_cols = nc;
    if (n_counts) *n_counts = nk;
    if ((con || conq || cols_cap) && cols_cap < nc) return fail(DFK_E_ARG, "buffer too small: %llu < %llu consensus columns", (unsigned long long)cols_cap, (unsigned long long)nc);
    if ((counts || counts_cap) && counts_cap < nk) return fail(DFK_E_ARG, "buffer too small: %llu < %llu conflict counts", (unsigned long long)counts_cap, (unsigned long long)nk);
    if ((cols_cap && nc && (!con || !conq)) || (counts_cap && nk && !counts)) return fail(DFK_E_ARG, "null argument");
    if (con && nc) { memcpy(con, R->con.data(), nc); memcpy(conq, R->conq.data(), nc); }
    if (counts && nk) memcpy(counts, R->counts.data(), 2 * nk);
    if (starts) memcpy(starts, R->starts.data(), 8 * (n + 1));                  // room for n_elements + 1 words
    if (conflict_first) memcpy(conflict_first, R->cfirst.data(), 8 * (n / 2 + 1));     // room for n_elements / 2 + 1 words
    if (dims && n) memcpy(dims, R->dims.data(), 16 * n);                        // room for 4 * n_elements words
    return 0;
    });
}

int dfk_scons_write(dfk_ctx* c, const char* dir)
{
    return guarded([&]() -> int {
    SconsResult* R = nullptr;
    if (int rc = scons_result_of(c, &R)) return rc;
    if (!dir) return fail(DFK_E_ARG, "null directory");
    return scons_write(R, dir);
    });
}

} // extern "C"
