// superplus_amd/csrc/dfk_soffsets.inc -- Stackster's stack offsets per pair (10X/Stackster.cc:461-645) and the file a.stack.offsets,
// included by dfk.hip.
//
// The rule, the shared pieces, the plan and the file's layout: dfk_soffsets.h.  The kernels: dfk_soffsets_kernels.h.  Here:
// soffsets_build() -- the table of log binomial sums sent up once a call (dfk_offsets::table()), a range of whole pairs at a time the
// live rows from the walks' placed records (host, dfk_scons.h's rule) and the range's con and conflict counts up, under it the batches
// of whole pairs: the reads their live rows name gathered once each, decoded and lowered (dfk_cons.inc's cn_batch_reads, k_wk_lower),
// the search a workgroup a pair, the records' counts scanned, the records emitted and brought back -- and soffsets_write().
// Everything on the device comes from the arena and goes back before build returns.
#include "dfk_soffsets_kernels.h"

namespace {

struct SoffsetsResult {
    std::vector<uint64_t> starts;                 // [n_pairs + 1], in records
    std::vector<dfk_soffsets::PairWords> words;   // [n_pairs]
    std::vector<dfk_soffsets::Rec> recs;
    uint64_t stats[DFK_SOFFSETS_WORDS] = {};
    uint64_t scons_serial = 0;                    // dfk_soffsets_build: the stack consensus it was made from (0: from arrays); dfk_sclosures_build asks
};
void soffsets_result_free(SoffsetsResult* r) { delete r; }

struct SoffsetsSource {
    SconsSource W;                                // the walks and the reads
    const uint64_t* cons_starts; const dfk_scons::Dim* dims; const uint8_t* con; const uint8_t* conq; const uint64_t* cfirst; const uint16_t* counts;
};

int soffsets_build(dfk_ctx* c, const SoffsetsSource& X, uint64_t rows_per_batch, SoffsetsResult* R)
{
    using namespace dfk_soffsets;
    const SconsSource& S = X.W;
    const uint64_t N = S.rd->n, n_pairs = S.n_pairs, n_stacks = 2 * n_pairs;
    if (N > (1ull << 31) || n_pairs >= (1ull << 30)) return fail(DFK_E_ARG, "%llu reads, %llu pairs: a row keeps its read in 31 bits", (unsigned long long)N, (unsigned long long)n_pairs);
    // ---- the walks' tables, checked as dfk_scons.inc checks them
    if (S.starts[0] != 0) return fail(DFK_E_ARG, "soffsets: the walks' starts do not begin at 0");
    for (uint64_t q = 0; q < n_stacks; ++q)
        if (S.starts[q + 1] < S.starts[q] || S.starts[q + 1] - S.starts[q] != S.recs[q].placed) return fail(DFK_E_ARG, "soffsets: the walks' starts fall or leave walk %llu other than its %u placed records", (unsigned long long)q, S.recs[q].placed);
    const uint64_t n_locs = S.starts[n_stacks];
    std::vector<uint32_t> loc_len(n_locs + 1, 0);
    for (uint64_t j = 0; j < n_locs; ++j) {
        const dfk_walks::Loc& L = S.locs[j];
        if (L.id < 0 || (uint64_t)L.id >= N) return fail(DFK_E_ARG, "a placed record names read %lld of %llu", (long long)L.id, (unsigned long long)N);
        if (L.start <= -(1 << 30) || L.start >= (1 << 30) || L.fw > 1) return fail(DFK_E_ARG, "a placed record lies at %d with the flag %u", L.start, L.fw);
        if (int rc = host_read(c, &loc_len[j], S.rd->len + L.id, 4)) return rc;
    }
    // ---- the consensus' tables, checked (dfk_soffsets.h's check_cons)
    if (X.cons_starts[0] != 0 || X.cfirst[0] != 0) return fail(DFK_E_ARG, "soffsets: the consensus' starts do not begin at 0");
    for (uint64_t q = 0; q < n_stacks; ++q) {
        if (X.cons_starts[q + 1] < X.cons_starts[q]) return fail(DFK_E_ARG, "soffsets: the consensus' starts fall at element %llu", (unsigned long long)q);
        const uint64_t w = X.cons_starts[q + 1] - X.cons_starts[q];
        if (w > (uint64_t)MAX_WIDTH || w != X.dims[q].cols) return fail(DFK_E_ARG, "soffsets: element %llu is %llu columns wide, its dims say %u: %lld at most", (unsigned long long)q, (unsigned long long)w, X.dims[q].cols, (long long)MAX_WIDTH);
    }
    for (uint64_t i = 0; i < X.cons_starts[n_stacks]; ++i) if (X.con[i] > 3) return fail(DFK_E_ARG, "soffsets: base %u at column %llu of the consensus", X.con[i], (unsigned long long)i);
    std::vector<uint64_t> prows(n_pairs, 0);
    uint64_t n_yield = 0, n_rows = 0;
    for (uint64_t pi = 0; pi < n_pairs; ++pi) {
        const bool y = dfk_scons::yields(S.recs, pi);
        if (X.cfirst[pi + 1] < X.cfirst[pi] || X.cfirst[pi + 1] - X.cfirst[pi] != (y ? X.cons_starts[2 * pi + 2] - X.cons_starts[2 * pi] : 0))
            return fail(DFK_E_ARG, "soffsets: pair %llu has %lld conflict counts, not the %llu of its offsets", (unsigned long long)pi, (long long)(X.cfirst[pi + 1] - X.cfirst[pi]),
                        (unsigned long long)(y ? X.cons_starts[2 * pi + 2] - X.cons_starts[2 * pi] : 0));
        if (!y) continue;
        ++n_yield;
        prows[pi] = S.starts[2 * pi + 2] - S.starts[2 * pi];
        for (uint64_t q = 2 * pi; q < 2 * pi + 2; ++q) {
            int64_t M = 0;
            for (uint64_t j = S.starts[q]; j < S.starts[q + 1]; ++j) M = std::max<int64_t>(M, (int64_t)S.locs[j].start + (int64_t)loc_len[j]);
            if (M != S.recs[q].M || M >= (1ll << 31)) return fail(DFK_E_ARG, "soffsets: walk %llu says M = %d, its placed records reach %lld", (unsigned long long)q, S.recs[q].M, (long long)M);
            if ((int64_t)X.dims[q].cols != M - dfk_scons::window_start(M)) return fail(DFK_E_ARG, "soffsets: element %llu has %u columns, its walk's M = %lld gives %lld", (unsigned long long)q, X.dims[q].cols, (long long)M, (long long)(M - dfk_scons::window_start(M)));
            n_rows += X.dims[q].rows_kept;
        }
    }
    const std::vector<uint64_t> pfirst = prefix_sums(prows.data(), n_pairs);
    const unsigned cus = (unsigned)c->prop.multiProcessorCount;
    const double t_in = wall_now();
    const uint64_t mark = c->alloc_seq;
    CnTimes times;
    float ms_lower = 0, ms_search = 0, ms_emit = 0;
    uint64_t n_batches = 0, n_ranges = 0, n_decoded = 0, n_live = 0, n_cnt[N_COUNTS] = {}, h_dg[8] = {};
    R->starts.assign(1, 0); R->words.clear(); R->recs.clear();
    auto body = [&]() -> int {
        int rc;
        Timer tm(c->stream);
        CnTables T;                                                            // (of the consensus' tables only the count of streams that did not decode)
        if ((rc = c->alloc(T.bad, 8, "streams that did not decode", Place::Low))) return rc;
        HIP_TRY(hipMemsetAsync(T.bad.p, 0, 8, c->stream));
        DevBuf d_T;
        const std::vector<double>& table = dfk_offsets::table();
        if (n_yield) if ((rc = cn_up(c, d_T, table.data(), table.size() * 8, "log binomial sums"))) return rc;
        const ConsSource CS{0, nullptr, 0, nullptr, nullptr, nullptr, nullptr, 0, nullptr, nullptr, S.rd, S.pq, S.pq_off};
        const uint64_t forced = path_switches().pidx_range_pairs;
        for (uint64_t p0 = 0; p0 < n_pairs;) {
            const PidxRange range = pidx_next_range(pfirst.data(), n_pairs, p0, dfk_scons::row_cap(c->largest_allocatable(), forced));
            const uint64_t p1 = range.e1, np = p1 - p0, ns = 2 * np;
            if (!range.ok) return fail(DFK_E_ARG, "pair %llu alone has %llu rows: a range keeps 32-bit places", (unsigned long long)p0, (unsigned long long)range.n);
            ++n_ranges;
            const uint64_t rmark = c->alloc_seq;
            // ---- the stacks of the range: the live rows, the columns, the conflict entries, what each pair costs a batch (host)
            const double t_h = wall_now();
            std::vector<int32_t> M(ns, 0);
            std::vector<uint64_t> col_first(ns + 1, 0), cnt_first(np + 1, 0), plive(np + 1, 0), pcost(np + 1, 0);
            CnRange G;
            G.h_lfirst.assign(ns + 1, 0);
            std::vector<int32_t> l_start; std::vector<uint32_t> l_len;
            for (uint64_t s = 0; s < ns; ++s) {
                const uint64_t q = 2 * p0 + s;
                if (dfk_scons::yields(S.recs, q / 2)) {
                    M[s] = S.recs[q].M;
                    const int64_t w0 = dfk_scons::window_start(M[s]);
                    for (uint64_t j = S.starts[q]; j < S.starts[q + 1]; ++j) {
                        if (!dfk_scons::span_meets(S.locs[j].start, loc_len[j], w0)) continue;
                        G.h_id.push_back((uint32_t)S.locs[j].id); l_start.push_back(S.locs[j].start); l_len.push_back(loc_len[j] | (dfk_scons::row_rc(S.locs[j].fw != 0) ? 0x80000000u : 0u));
                    }
                }
                G.h_lfirst[s + 1] = G.h_id.size();
                col_first[s + 1] = X.cons_starts[q + 1] - X.cons_starts[2 * p0];
            }
            for (uint64_t p = 0; p < np; ++p) {
                cnt_first[p + 1] = X.cfirst[p0 + p + 1] - X.cfirst[p0];
                plive[p + 1] = G.h_lfirst[2 * p + 2];
                uint64_t cost = pair_cost(cnt_first[p + 1] - cnt_first[p]);
                for (uint64_t l = G.h_lfirst[2 * p]; l < G.h_lfirst[2 * p + 2]; ++l) cost += dfk_cons::live_row_cost(l_len[l] & 0x7FFFFFFFu);
                pcost[p + 1] = pcost[p] + cost;
            }
            const uint64_t got = G.h_id.size(), n_cols = col_first[ns], n_cnt_range = cnt_first[np];
            n_live += got;
            DevBuf d_M, d_colfirst, d_con, d_cntfirst, d_counts, d_lfirst, d_lstart, d_llen;
            if ((rc = cn_up(c, d_M, M.data(), ns * 4, "stack widths")) || (rc = cn_up(c, d_colfirst, col_first.data(), (ns + 1) * 8, "columns per stack")) ||
                (rc = cn_up(c, d_con, X.con + X.cons_starts[2 * p0], n_cols, "consensus bases")) || (rc = cn_up(c, d_cntfirst, cnt_first.data(), (np + 1) * 8, "conflict entries per pair")) ||
                (rc = cn_up(c, d_counts, X.counts + X.cfirst[p0], n_cnt_range * 2, "conflict counts")) || (rc = cn_up(c, d_lfirst, G.h_lfirst.data(), (ns + 1) * 8, "live rows per stack")) ||
                (rc = cn_up(c, d_lstart, l_start.data(), got * 4, "live rows' starts")) || (rc = cn_up(c, d_llen, l_len.data(), got * 4, "live rows' lengths"))) return rc;
            times.s_copy += wall_now() - t_h;
            // ---- the batches of whole pairs
            for (uint64_t b0 = 0; b0 < np;) {
                const uint64_t b1 = next_batch(plive.data(), pcost.data(), np, b0, dfk_cons::batch_room(c->largest_allocatable()), rows_per_batch), nb = b1 - b0;
                ++n_batches;
                const uint64_t bmark = c->alloc_seq;
                const uint64_t n_slots = cnt_first[b1] - cnt_first[b0];
                std::vector<PairWords> h_words(nb);
                std::vector<uint64_t> h_nrec(nb + 1, 0), h_cnt(nb * N_COUNTS, 0);
                std::vector<Rec> h_recs;
                if (n_slots) {                                               // (no entry: no pair of the batch yields)
                    // the reads of the batch, each once, ascending; the gather; the decode; the lowering
                    CnReads B;
                    if ((rc = cn_batch_reads(c, CS, T, G, 2 * b0, 2 * b1, tm, &times, &B))) return rc;
                    n_decoded += B.n_ids;
                    tm.start();
                    if (B.n_ids) {
                        hipLaunchKernelGGL(k_wk_lower, dim3(grid_256(B.n_ids, cus)), dim3(256), 0, c->stream, (const uint8_t*)B.bases.p, (const uint64_t*)B.bat.p, (const uint64_t*)B.qat.p, B.n_ids, (uint8_t*)B.quals.p);
                        HIP_TRY(hipGetLastError());
                    }
                    DevBuf d_slots, d_nrec, d_place, d_words, d_cnt, d_recs;
                    if ((rc = c->alloc(d_slots, n_slots * sizeof(Rec), "records per pair", Place::Low)) || (rc = c->alloc(d_nrec, (nb + 1) * 8, "records a pair", Place::Low)) ||
                        (rc = c->alloc(d_place, (nb + 1) * 8, "record places", Place::Low)) || (rc = c->alloc(d_words, nb * sizeof(PairWords), "per-pair words", Place::Low)) ||
                        (rc = c->alloc(d_cnt, nb * N_COUNTS * 8, "search counts", Place::Low))) return rc;
                    HIP_TRY(hipStreamSynchronize(c->stream));
                    ms_lower += tm.stop();
                    tm.start();
                    const SoBatch Bk{b0, nb, (const int32_t*)d_M.p, (const uint64_t*)d_colfirst.p, (const uint8_t*)d_con.p, (const uint64_t*)d_cntfirst.p, (const uint16_t*)d_counts.p, (const uint64_t*)d_lfirst.p,
                                     (const int32_t*)d_lstart.p, (const uint32_t*)d_llen.p, (const uint32_t*)B.slot.p, B.live0, (const uint64_t*)B.bat.p, (const uint64_t*)B.qat.p, (const uint8_t*)B.bases.p,
                                     (const uint8_t*)B.quals.p, (const double*)d_T.p};
                    hipLaunchKernelGGL(k_so_search, dim3(dfk_scons::pair_grid(nb + 1, cus)), dim3(GROUP), 0, c->stream, Bk, (Rec*)d_slots.p, (uint64_t*)d_nrec.p, (PairWords*)d_words.p, (unsigned long long*)d_cnt.p);
                    HIP_TRY(hipGetLastError());
                    HIP_TRY(hipStreamSynchronize(c->stream));
                    ms_search += tm.stop();
                    tm.start();
                    if ((rc = device_scan(c, (const uint64_t*)d_nrec.p, (uint64_t*)d_place.p, nb + 1))) return rc;
                    uint64_t n_out = 0;
                    HIP_TRY(hipMemcpyAsync(&n_out, (const uint64_t*)d_place.p + nb, 8, hipMemcpyDeviceToHost, c->stream));
                    HIP_TRY(hipStreamSynchronize(c->stream));
                    if (n_out > n_slots) return fail(DFK_E_HIP, "soffsets: %llu records for %llu offsets", (unsigned long long)n_out, (unsigned long long)n_slots);
                    h_recs.resize(n_out);
                    if (n_out) {
                        if ((rc = c->alloc(d_recs, n_out * sizeof(Rec), "records", Place::Low))) return rc;
                        hipLaunchKernelGGL(k_so_emit, dim3(grid_256(n_slots, cus)), dim3(256), 0, c->stream, Bk, (const Rec*)d_slots.p, (const uint64_t*)d_nrec.p, (const uint64_t*)d_place.p, (Rec*)d_recs.p);
                        HIP_TRY(hipGetLastError());
                        HIP_TRY(hipMemcpyAsync(h_recs.data(), d_recs.p, n_out * sizeof(Rec), hipMemcpyDeviceToHost, c->stream));
                    }
                    HIP_TRY(hipMemcpyAsync(h_nrec.data(), d_nrec.p, (nb + 1) * 8, hipMemcpyDeviceToHost, c->stream));
                    HIP_TRY(hipMemcpyAsync(h_words.data(), d_words.p, nb * sizeof(PairWords), hipMemcpyDeviceToHost, c->stream));
                    HIP_TRY(hipMemcpyAsync(h_cnt.data(), d_cnt.p, nb * N_COUNTS * 8, hipMemcpyDeviceToHost, c->stream));
                    HIP_TRY(hipStreamSynchronize(c->stream));
                    ms_emit += tm.stop();
                } else for (PairWords& w : h_words) w = PairWords{0, 0, 0, 0};
                // ---- the batch's share of the result, checked
                uint64_t at = 0;
                for (uint64_t p = 0; p < nb; ++p) {
                    const uint64_t slots = cnt_first[b0 + p + 1] - cnt_first[b0 + p];
                    if (h_nrec[p] > slots || at + h_nrec[p] > h_recs.size()) return fail(DFK_E_HIP, "soffsets: pair %llu has %llu records of %llu offsets", (unsigned long long)(p0 + b0 + p), (unsigned long long)h_nrec[p], (unsigned long long)slots);
                    const int n2 = (int)(col_first[2 * (b0 + p) + 2] - col_first[2 * (b0 + p) + 1]);
                    uint32_t n_kept = 0, n_res = 0;
                    for (uint64_t i = at; i < at + h_nrec[p]; ++i) {
                        const Rec& r = h_recs[i];
                        if (r.state > DROPPED || r.zero || !r.results || !(r.best_bits >= MIN_BITS) || r.offset + n2 < 0 || (uint64_t)(r.offset + n2) >= slots || (i > at && r.offset <= h_recs[i - 1].offset))
                            return fail(DFK_E_HIP, "soffsets: record %llu of pair %llu: offset %d, %u results, state %u", (unsigned long long)(i - at), (unsigned long long)(p0 + b0 + p), r.offset, r.results, r.state);
                        n_kept += r.state == KEPT; n_res += r.results;
                    }
                    const PairWords& w = h_words[p];
                    if (w.kept != n_kept || w.results != n_res || w.closable != (closable(n_kept) ? 1u : 0u) || w.results > w.seen) return fail(DFK_E_HIP, "soffsets: the words of pair %llu do not say what its records do", (unsigned long long)(p0 + b0 + p));
                    at += h_nrec[p];
                    R->words.push_back(w);
                    R->starts.push_back(R->recs.size() + at);
                    for (uint32_t k = 0; k < N_COUNTS; ++k) n_cnt[k] += h_cnt[p * N_COUNTS + k];
                }
                if (at != h_recs.size()) return fail(DFK_E_HIP, "soffsets: %llu records emitted, %llu counted", (unsigned long long)h_recs.size(), (unsigned long long)at);
                R->recs.insert(R->recs.end(), h_recs.begin(), h_recs.end());
                c->release_since(bmark);
                b0 = b1;
            }
            c->release_since(rmark);
            p0 = p1;
        }
        // ---- the digest: the per-pair words, then the records as u32 words
        if (n_pairs) {
            DevBuf d_w, d_r, dg;
            const uint64_t nw = 4 * n_pairs, nr = 6 * (uint64_t)R->recs.size();
            if ((rc = cn_up(c, d_w, R->words.data(), nw * 4, "a.stack.offsets words")) || (rc = cn_up(c, d_r, R->recs.data(), nr * 4, "a.stack.offsets records")) || (rc = c->alloc(dg, 32, "soffsets digest", Place::Low))) return rc;
            HIP_TRY(hipMemsetAsync(dg.p, 0, 32, c->stream));
            hipLaunchKernelGGL(HIP_KERNEL_NAME(k_digest_seq<uint32_t>), dim3(grid_256(nw, cus)), dim3(256), 0, c->stream, (const uint32_t*)d_w.p, nw, SALT, (unsigned long long*)dg.p);
            if (nr) hipLaunchKernelGGL(HIP_KERNEL_NAME(k_digest_seq<uint32_t>), dim3(grid_256(nr, cus)), dim3(256), 0, c->stream, (const uint32_t*)d_r.p, nr, SALT + nw, (unsigned long long*)dg.p);
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
    if (R->words.size() != n_pairs || R->starts.size() != n_pairs + 1) return fail(DFK_E_HIP, "soffsets: %llu elements for %llu pairs", (unsigned long long)R->words.size(), (unsigned long long)n_pairs);
    uint64_t* s = R->stats;
    s[DFK_SOFFSETS_PAIRS] = n_pairs; s[DFK_SOFFSETS_YIELDS] = n_yield; s[DFK_SOFFSETS_ROWS] = n_rows; s[DFK_SOFFSETS_KMERS] = n_cnt[C_KMERS]; s[DFK_SOFFSETS_ACCEPTABLE] = n_cnt[C_ACCEPTABLE];
    s[DFK_SOFFSETS_HITS] = n_cnt[C_HITS]; s[DFK_SOFFSETS_SEEN] = n_cnt[C_SEEN]; s[DFK_SOFFSETS_DISALLOWED] = n_cnt[C_DISALLOWED]; s[DFK_SOFFSETS_LOOKUPS] = n_cnt[C_LOOKUPS]; s[DFK_SOFFSETS_RESULTS] = n_cnt[C_RESULTS];
    s[DFK_SOFFSETS_OFFSETS] = R->recs.size();
    for (const Rec& r : R->recs) { s[DFK_SOFFSETS_KEPT] += r.state == KEPT; s[DFK_SOFFSETS_DROPPED] += r.state == DROPPED; }
    for (const PairWords& w : R->words) {
        s[w.kept == 0 ? DFK_SOFFSETS_PAIRS_0 : w.kept == 1 ? DFK_SOFFSETS_PAIRS_1 : w.kept == 2 ? DFK_SOFFSETS_PAIRS_2 : w.kept == 3 ? DFK_SOFFSETS_PAIRS_3 : DFK_SOFFSETS_PAIRS_MORE] += 1;
        s[DFK_SOFFSETS_CLOSABLE] += w.closable;
    }
    s[DFK_SOFFSETS_LIVE] = n_live; s[DFK_SOFFSETS_DECODED] = n_decoded; s[DFK_SOFFSETS_BATCHES] = n_batches; s[DFK_SOFFSETS_RANGES] = n_ranges;
    s[DFK_SOFFSETS_US] = (uint64_t)(1e6 * (wall_now() - t_in)); s[DFK_SOFFSETS_US_COPY] = (uint64_t)(1e6 * times.s_copy); s[DFK_SOFFSETS_US_DECODE] = (uint64_t)(1000.0f * (times.ms_decode + ms_lower));
    s[DFK_SOFFSETS_US_SEARCH] = (uint64_t)(1000.0f * ms_search); s[DFK_SOFFSETS_US_EMIT] = (uint64_t)(1000.0f * ms_emit);
    s[DFK_SOFFSETS_SUM] = h_dg[0]; s[DFK_SOFFSETS_XOR] = h_dg[1];
    TRACE("soffsets: %llu pairs, %llu yielding, %llu rows (%llu live), %llu row 8-mers, %llu hits, %llu candidates, %llu results, %llu offsets (%llu kept), %llu closable, %llu look-ups, %llu reads decoded in %llu range(s), %llu batch(es); gather and copies %.1f ms, decode and lowering %.1f ms, search %.1f ms, scan and emit %.1f ms",
          (unsigned long long)n_pairs, (unsigned long long)n_yield, (unsigned long long)n_rows, (unsigned long long)n_live, (unsigned long long)n_cnt[C_KMERS], (unsigned long long)n_cnt[C_HITS], (unsigned long long)n_cnt[C_SEEN],
          (unsigned long long)n_cnt[C_RESULTS], (unsigned long long)R->recs.size(), (unsigned long long)s[DFK_SOFFSETS_KEPT], (unsigned long long)s[DFK_SOFFSETS_CLOSABLE], (unsigned long long)n_cnt[C_LOOKUPS],
          (unsigned long long)n_decoded, (unsigned long long)n_ranges, (unsigned long long)n_batches, 1e3 * times.s_copy, times.ms_decode + ms_lower, ms_search, ms_emit);
    return 0;
}

// the file into `dir`: whole, or not at all
int soffsets_write(const SoffsetsResult* R, const std::string& dir)
{
    using namespace dfk_soffsets;
    const std::string path = dir + "/a.stack.offsets";
    const uint64_t n = R->starts.size() - 1;
    const int fd = open(path.c_str(), O_WRONLY | O_CREAT | O_TRUNC, 0666);
    if (fd < 0) return fail(DFK_E_ARG, "cannot open %s", path.c_str());
    const dfk_closer::BinHead h = dfk_closer::head_of(MAGIC, n);
    bool bad = pwrite_all(fd, &h, 16, 0) != 0 || pwrite_all(fd, R->starts.data(), 8 * (n + 1), 16) != 0;
    if (!bad && n) bad = pwrite_all(fd, R->words.data(), 16 * n, words_at(n)) != 0;
    if (!bad && !R->recs.empty()) bad = pwrite_all(fd, R->recs.data(), sizeof(Rec) * R->recs.size(), recs_at(n)) != 0;
    if (close(fd) != 0) bad = true;
    if (bad) { (void)unlink(path.c_str()); return fail(DFK_E_ARG, "short write to %s", path.c_str()); }
    return 0;
}

// the latest dfk_soffsets_build*'s result: one a context, kept beside the graph
int soffsets_result_of(dfk_ctx* c, SoffsetsResult** out)
{
    if (!c) return fail(DFK_E_ARG, "null context");
    if (!c->graph_state || !graph_of(c)->soffsets) return fail(DFK_E_STATE, "no stack offsets: call dfk_soffsets_build or dfk_soffsets_build_arrays");
    *out = graph_of(c)->soffsets;
    return 0;
}
void soffsets_keep(dfk_ctx* c, SoffsetsResult* R)
{
    HostGraph* G = graph_of(c);
    if (G->soffsets) soffsets_result_free(G->soffsets);
    G->soffsets = R; G->soffsets_free = soffsets_result_free;
}

} // namespace

extern "C" {

int dfk_soffsets_build(dfk_ctx* c, const uint8_t* packed, const uint64_t* base_off, const uint32_t* read_len, const uint8_t* pq, const uint64_t* pq_off, uint64_t n_reads)
{
    return guarded([&]() -> int {
    WalksResult* W = nullptr;
    SconsResult* K = nullptr;
    if (int rc = walks_result_of(c, &W)) return rc;                                         // DFK_E_STATE without walks,
    if (int rc = scons_result_of(c, &K)) return rc;                                         // without their stack consensus,
    if (!K->walks_serial) return fail(DFK_E_STATE, "the stack consensus came from dfk_scons_build_arrays: call dfk_scons_build after dfk_walks_build");
    if (K->walks_serial != W->serial) return fail(DFK_E_STATE, "the stack consensus was made from other walks: call dfk_scons_build again");      // and with one of other walks
    if (n_reads != W->n_reads) return fail(DFK_E_ARG, "soffsets: %llu reads given, the walks were made from %llu", (unsigned long long)n_reads, (unsigned long long)W->n_reads);
    PartnerReads reads;
    if (int rc = walks_reads(packed, base_off, read_len, pq, pq_off, n_reads, &reads)) return rc;
    HIP_TRY(hipSetDevice(c->device));
    const dfk_walks::Rec no_rec{}; const dfk_walks::Loc no_loc{}; const dfk_scons::Dim no_dim{}; const uint8_t none = 0; const uint16_t no_count = 0;
    const SoffsetsSource X{SconsSource{W->recs.size() / 2, W->starts.data(), W->recs.empty() ? &no_rec : W->recs.data(), W->locs.empty() ? &no_loc : W->locs.data(), &reads, pq, pq_off},
                           K->starts.data(), K->dims.empty() ? &no_dim : K->dims.data(), K->con.empty() ? &none : K->con.data(), K->conq.empty() ? &none : K->conq.data(), K->cfirst.data(),
                           K->counts.empty() ? &no_count : K->counts.data()};
    if (K->dims.size() != W->recs.size()) return fail(DFK_E_STATE, "the stack consensus holds %llu elements, the walks %llu", (unsigned long long)K->dims.size(), (unsigned long long)W->recs.size());
    std::unique_ptr<SoffsetsResult> R(new SoffsetsResult);
    if (int rc = soffsets_build(c, X, 0, R.get())) return rc;                               // (refused: the earlier result is still served)
    R->scons_serial = K->serial;
    soffsets_keep(c, R.release());
    return 0;
    });
}

// The stage on host arrays: the walks in dfk_walks_fetch's forms, the reads, the consensus in dfk_scons_fetch's forms, checked here.
int dfk_soffsets_build_arrays(dfk_ctx* c, const uint64_t* starts, const uint32_t* records, const void* placed, uint64_t n_pairs, const uint8_t* packed, const uint64_t* base_off, const uint32_t* read_len,
                              const uint8_t* pq, const uint64_t* pq_off, uint64_t n_reads, const uint64_t* cons_starts, const uint32_t* dims, const uint8_t* con, const uint8_t* conq, const uint64_t* conflict_first,
                              const uint16_t* counts, uint64_t rows_per_batch, const char* dir)
{
    return guarded([&]() -> int {
    if (!c) return fail(DFK_E_ARG, "null context");
    if (!starts || !cons_starts || !conflict_first || (n_pairs && (!records || !dims))) return fail(DFK_E_ARG, "null argument");
    if (n_reads >= (1ull << 31) || n_pairs >= (1ull << 30)) return fail(DFK_E_ARG, "%llu reads, %llu pairs: 2^31 - 1 reads and 2^30 - 1 pairs at most", (unsigned long long)n_reads, (unsigned long long)n_pairs);
    if (starts[0] != 0 || cons_starts[0] != 0 || conflict_first[0] != 0) return fail(DFK_E_ARG, "the tables do not start at 0");
    for (uint64_t q = 0; q < 2 * n_pairs; ++q) if (starts[q + 1] < starts[q] || cons_starts[q + 1] < cons_starts[q]) return fail(DFK_E_ARG, "the starts fall at element %llu", (unsigned long long)q);
    for (uint64_t p = 0; p < n_pairs; ++p) if (conflict_first[p + 1] < conflict_first[p]) return fail(DFK_E_ARG, "the conflict entries' starts fall at pair %llu", (unsigned long long)p);
    if ((starts[2 * n_pairs] && !placed) || (cons_starts[2 * n_pairs] && (!con || !conq)) || (conflict_first[n_pairs] && !counts)) return fail(DFK_E_ARG, "null argument");
    PartnerReads reads;
    if (int rc = walks_reads(packed, base_off, read_len, pq, pq_off, n_reads, &reads)) return rc;
    HIP_TRY(hipSetDevice(c->device));
    const dfk_walks::Rec no_rec{}; const dfk_walks::Loc no_loc{}; const dfk_scons::Dim no_dim{}; const uint8_t none = 0; const uint16_t no_count = 0;
    const SoffsetsSource X{SconsSource{n_pairs, starts, n_pairs ? (const dfk_walks::Rec*)records : &no_rec, placed ? (const dfk_walks::Loc*)placed : &no_loc, &reads, pq, pq_off},
                           cons_starts, n_pairs ? (const dfk_scons::Dim*)dims : &no_dim, con ? con : &none, conq ? conq : &none, conflict_first, counts ? counts : &no_count};
    std::unique_ptr<SoffsetsResult> R(new SoffsetsResult);
    if (int rc = soffsets_build(c, X, rows_per_batch, R.get())) return rc;
    if (dir) if (int rc = soffsets_write(R.get(), dir)) return rc;
    soffsets_keep(c, R.release());
    return 0;
    });
}

int dfk_soffsets_stats(dfk_ctx* c, uint64_t* out)
{
    return guarded([&]() -> int {
    SoffsetsResult* R = nullptr;
    if (int rc = soffsets_result_of(c, &R)) return rc;
    if (!out) return fail(DFK_E_ARG, "null argument");
    for (int i = 0; i < DFK_SOFFSETS_WORDS; ++i) out[i] = R->stats[i];
    return 0;
    });
}

int dfk_soffsets_fetch(dfk_ctx* c, uint64_t* starts, uint32_t* words, uint64_t* n_pairs, void* records, uint64_t records_cap, uint64_t* n_records)
{
    return guarded([&]() -> int {
    SoffsetsResult* R = nullptr;
    if (int rc = soffsets_result_of(c, &R)) return rc;
    const uint64_t n = R->starts.size() - 1, nr = R->recs.size();
    if (n_pairs) *n_pairs = n;
    if (n_records) *n_records = nr;
    if ((records || records_cap) && records_cap < nr) return fail(DFK_E_ARG, "buffer too small: %llu < %llu records", (unsigned long long)records_cap, (unsigned long long)nr);
    if (records_cap && nr && !records) return fail(DFK_E_ARG, "null argument");
    if (records && nr) memcpy(records, R->recs.data(), sizeof(dfk_soffsets::Rec) * nr);
    if (starts) memcpy(starts, R->starts.data(), 8 * (n + 1));                   // the starts: room for n_pairs + 1 words
    if (words && n) memcpy(words, R->words.data(), 16 * n);                      // the words: room for 4 * n_pairs u32
    return 0;
    });
}

int dfk_soffsets_write(dfk_ctx* c, const char* dir)
{
    return guarded([&]() -> int {
    SoffsetsResult* R = nullptr;
    if (int rc = soffsets_result_of(c, &R)) return rc;
    if (!dir) return fail(DFK_E_ARG, "null directory");
    return soffsets_write(R, dir);
    });
}

} // extern "C"
