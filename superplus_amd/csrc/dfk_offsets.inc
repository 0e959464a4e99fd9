// superplus_amd/csrc/dfk_offsets.inc -- GetOffsets1 per pair (paths/long/ReadStack.cc:1192-1512, called at 10X/Closomatic.cc:648) and
// the file a.close.offsets, included by dfk.hip.
//
// The rule, the table, the shared pieces, the tail, the plan and the file's layout: dfk_offsets.h.  The kernels: dfk_offsets_kernels.h.
// Here: offsets_build() -- the table sent up once a call, then a batch of pairs at a time the sequences up, the candidates (bitmaps,
// counts, scan, emit), the bits test (a workgroup a candidate), the compaction of those that passed, their records back, the tail on
// the host a pair at a time -- and offsets_write().  Everything on the device comes from the arena and goes back before build returns.
#include "dfk_offsets_kernels.h"

namespace {

struct OffsetsResult {
    std::vector<uint64_t> starts;                 // [n_pairs + 1], in records
    std::vector<dfk_offsets::PairWords> words;    // [n_pairs]
    std::vector<dfk_offsets::Rec> recs;
    uint64_t stats[DFK_OFFSETS_WORDS] = {};
    uint64_t cons_serial = 0;                     // dfk_offsets_build: the consensus it was made from (0: from arrays); dfk_closures_build asks
};
void offsets_result_free(OffsetsResult* r) { delete r; }

int offsets_build(dfk_ctx* c, uint64_t n_pairs, const uint64_t* starts, const uint8_t* bases, uint64_t per_batch, OffsetsResult* R)
{
    using namespace dfk_offsets;
    if (n_pairs >= (1ull << 31)) return fail(DFK_E_ARG, "%llu pairs: a candidate keeps its pair in 32 bits", (unsigned long long)n_pairs);
    const unsigned cus = (unsigned)c->prop.multiProcessorCount;
    const double t_in = wall_now();
    const uint64_t mark = c->alloc_seq;
    float ms_cand = 0, ms_bits = 0, ms_compact = 0;
    double s_tail = 0, s_copy = 0;
    uint64_t n_batches = 0, n_cand = 0, n_lookups = 0, h_dg[4] = {};
    R->starts.assign(1, 0); R->words.clear(); R->recs.clear();
    auto body = [&]() -> int {
        int rc;
        Timer tm(c->stream);
        auto up = [&](DevBuf& d, const void* h, uint64_t bytes, const char* what) -> int {
            if (int r = c->alloc(d, std::max<uint64_t>(8, bytes), what, Place::Low)) return r;
            return bytes ? upload(c, d.p, h, bytes) : 0;
        };
        DevBuf d_T;
        const std::vector<double>& T = table();
        if (n_pairs) if ((rc = up(d_T, T.data(), T.size() * 8, "log binomial sums"))) return rc;
        for (uint64_t p0 = 0; p0 < n_pairs;) {
            const uint64_t nb = std::min(n_pairs - p0, pairs_per_batch(c->largest_allocatable(), per_batch)), p1 = p0 + nb;
            ++n_batches;
            const uint64_t bmark = c->alloc_seq;
            const uint64_t b_first = starts[2 * p0], n_bases = starts[2 * p1] - b_first;
            // ---- candidates
            double t0 = wall_now();
            DevBuf d_first, d_bases, d_bitmaps, d_counts, d_place, d_cpair, d_coff;
            if ((rc = up(d_first, starts + 2 * p0, (2 * nb + 1) * 8, "consensus starts")) || (rc = up(d_bases, bases + b_first, n_bases, "consensus bases")) ||
                (rc = c->alloc(d_bitmaps, nb * BITMAP_WORDS * 4, "offset bitmaps", Place::Low)) || (rc = c->alloc(d_counts, (nb + 1) * 8, "candidates per pair", Place::Low)) ||
                (rc = c->alloc(d_place, (nb + 1) * 8, "candidate places", Place::Low))) return rc;
            s_copy += wall_now() - t0;
            const OfBatch B{(const uint64_t*)d_first.p, (const uint8_t*)d_bases.p, nb};
            tm.start();
            hipLaunchKernelGGL(k_of_candidates, dim3(group_grid(nb + 1, cus)), dim3(GROUP), 0, c->stream, B, (uint32_t*)d_bitmaps.p, (uint64_t*)d_counts.p);
            HIP_TRY(hipGetLastError());
            if ((rc = device_scan(c, (const uint64_t*)d_counts.p, (uint64_t*)d_place.p, nb + 1))) return rc;
            std::vector<uint64_t> h_counts(nb + 1);
            uint64_t C = 0;
            HIP_TRY(hipMemcpyAsync(&C, (const uint64_t*)d_place.p + nb, 8, hipMemcpyDeviceToHost, c->stream));
            HIP_TRY(hipMemcpyAsync(h_counts.data(), d_counts.p, (nb + 1) * 8, hipMemcpyDeviceToHost, c->stream));
            HIP_TRY(hipStreamSynchronize(c->stream));
            if (C > nb * (2ull * MAX_N)) return fail(DFK_E_HIP, "offsets: %llu candidates for %llu pairs", (unsigned long long)C, (unsigned long long)nb);
            if (C) {
                if ((rc = c->alloc(d_cpair, C * 4, "candidates' pairs", Place::Low)) || (rc = c->alloc(d_coff, C * 4, "candidates' offsets", Place::Low))) return rc;
                hipLaunchKernelGGL(k_of_emit, dim3(grid_256(nb, cus)), dim3(256), 0, c->stream, B, (const uint32_t*)d_bitmaps.p, (const uint64_t*)d_place.p, (uint32_t*)d_cpair.p, (int32_t*)d_coff.p);
                HIP_TRY(hipGetLastError());
            }
            ms_cand += tm.stop();
            n_cand += C;
            // ---- the bits test, the compaction
            std::vector<Rec> recs;
            std::vector<uint32_t> rec_pair;
            if (C) {
                DevBuf d_cand, d_flags, d_fplace, d_recs, d_rpair;
                if ((rc = c->alloc(d_cand, C * sizeof(OfCand), "candidates' bits", Place::Low)) || (rc = c->alloc(d_flags, (C + 1) * 8, "passed flags", Place::Low)) ||
                    (rc = c->alloc(d_fplace, (C + 1) * 8, "passed places", Place::Low))) return rc;
                tm.start();
                hipLaunchKernelGGL(k_of_bits, dim3(group_grid(C + 1, cus)), dim3(GROUP), 0, c->stream, B, (const uint32_t*)d_cpair.p, (const int32_t*)d_coff.p, C, (const double*)d_T.p, (OfCand*)d_cand.p,
                                   (uint64_t*)d_flags.p);
                HIP_TRY(hipGetLastError());
                HIP_TRY(hipStreamSynchronize(c->stream));
                ms_bits += tm.stop();
                tm.start();
                if ((rc = device_scan(c, (const uint64_t*)d_flags.p, (uint64_t*)d_fplace.p, C + 1))) return rc;
                uint64_t n_pass = 0;
                HIP_TRY(hipMemcpyAsync(&n_pass, (const uint64_t*)d_fplace.p + C, 8, hipMemcpyDeviceToHost, c->stream));
                HIP_TRY(hipStreamSynchronize(c->stream));
                if (n_pass > C) return fail(DFK_E_HIP, "offsets: %llu of %llu candidates passed", (unsigned long long)n_pass, (unsigned long long)C);
                if (n_pass) {
                    if ((rc = c->alloc(d_recs, n_pass * sizeof(Rec), "passed records", Place::Low)) || (rc = c->alloc(d_rpair, n_pass * 4, "passed records' pairs", Place::Low))) return rc;
                    hipLaunchKernelGGL(k_of_compact, dim3(grid_256(C, cus)), dim3(256), 0, c->stream, B, (const OfCand*)d_cand.p, (const uint32_t*)d_cpair.p, (const uint64_t*)d_flags.p, (const uint64_t*)d_fplace.p, C,
                                       (Rec*)d_recs.p, (uint32_t*)d_rpair.p);
                    HIP_TRY(hipGetLastError());
                }
                HIP_TRY(hipStreamSynchronize(c->stream));
                ms_compact += tm.stop();
                t0 = wall_now();
                std::vector<OfCand> h_cand(C);
                recs.resize(n_pass); rec_pair.resize(n_pass);
                HIP_TRY(hipMemcpyAsync(h_cand.data(), d_cand.p, C * sizeof(OfCand), hipMemcpyDeviceToHost, c->stream));
                if (n_pass) {
                    HIP_TRY(hipMemcpyAsync(recs.data(), d_recs.p, n_pass * sizeof(Rec), hipMemcpyDeviceToHost, c->stream));
                    HIP_TRY(hipMemcpyAsync(rec_pair.data(), d_rpair.p, n_pass * 4, hipMemcpyDeviceToHost, c->stream));
                }
                HIP_TRY(hipStreamSynchronize(c->stream));
                for (const OfCand& x : h_cand) n_lookups += x.lookups;
                s_copy += wall_now() - t0;
            }
            // ---- the tail, a pair at a time (the host)
            t0 = wall_now();
            uint64_t at = 0;
            for (uint64_t b = 0; b < nb; ++b) {
                const uint64_t q = 2 * (p0 + b), first = at;
                while (at < recs.size() && rec_pair[at] == b) ++at;
                if (at - first > h_counts[b]) return fail(DFK_E_HIP, "offsets: pair %llu has %llu records of %llu candidates", (unsigned long long)(p0 + b), (unsigned long long)(at - first), (unsigned long long)h_counts[b]);
                tail(bases + starts[q], (int)(starts[q + 1] - starts[q]), bases + starts[q + 1], (int)(starts[q + 2] - starts[q + 1]), recs.data() + first, (int)(at - first));
                uint32_t alive = 0;
                for (uint64_t i = first; i < at; ++i) alive += recs[i].state == SURVIVES;
                R->words.push_back(PairWords{(uint32_t)h_counts[b], (uint32_t)(at - first), alive, 0});
                R->starts.push_back(R->recs.size() + (at - first));
                R->recs.insert(R->recs.end(), recs.begin() + first, recs.begin() + at);
            }
            if (at != recs.size()) return fail(DFK_E_HIP, "offsets: the passed records are not in the order of their pairs");
            s_tail += wall_now() - t0;
            c->release_since(bmark);
            p0 = p1;
        }
        // ---- the digest: the per-pair words, then the records as u32 words
        if (n_pairs) {
            DevBuf d_w, d_r, dg;
            const uint64_t nw = 4 * n_pairs, nr = 8 * (uint64_t)R->recs.size();
            if ((rc = up(d_w, R->words.data(), nw * 4, "a.close.offsets words")) || (rc = up(d_r, R->recs.data(), nr * 4, "a.close.offsets records")) || (rc = c->alloc(dg, 32, "offsets digest", Place::Low))) return rc;
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
    uint64_t* s = R->stats;
    s[DFK_OFFSETS_PAIRS] = n_pairs; s[DFK_OFFSETS_CANDIDATES] = n_cand; s[DFK_OFFSETS_PASSED] = R->recs.size(); s[DFK_OFFSETS_LOOKUPS] = n_lookups; s[DFK_OFFSETS_BATCHES] = n_batches;
    for (const Rec& r : R->recs) { s[DFK_OFFSETS_INVALIDATED] += r.state == INVALIDATED; s[DFK_OFFSETS_DELETED_SMALL] += r.state == SMALL; s[DFK_OFFSETS_SURVIVORS] += r.state == SURVIVES; }
    for (const PairWords& w : R->words) {
        s[w.survivors == 0 ? DFK_OFFSETS_PAIRS_0 : w.survivors == 1 ? DFK_OFFSETS_PAIRS_1 : w.survivors == 2 ? DFK_OFFSETS_PAIRS_2 : DFK_OFFSETS_PAIRS_MORE] += 1;
        s[DFK_OFFSETS_CLOSABLE] += w.survivors == 1 || w.survivors == 2;                  // :651: a closure is tried with at most two offsets
    }
    s[DFK_OFFSETS_US] = (uint64_t)(1e6 * (wall_now() - t_in)); s[DFK_OFFSETS_US_CANDIDATES] = (uint64_t)(1000.0f * ms_cand); s[DFK_OFFSETS_US_BITS] = (uint64_t)(1000.0f * ms_bits);
    s[DFK_OFFSETS_US_COMPACT] = (uint64_t)(1000.0f * ms_compact); s[DFK_OFFSETS_US_TAIL] = (uint64_t)(1e6 * s_tail); s[DFK_OFFSETS_US_COPY] = (uint64_t)(1e6 * s_copy);
    s[DFK_OFFSETS_SUM] = h_dg[0]; s[DFK_OFFSETS_XOR] = h_dg[1];
    TRACE("offsets: %llu pairs, %llu candidates, %llu passed, %llu survive, %llu look-ups in %llu batch(es); candidates %.1f ms, bits %.1f ms, compaction %.1f ms, tail %.1f ms, copies %.1f ms",
          (unsigned long long)n_pairs, (unsigned long long)n_cand, (unsigned long long)R->recs.size(), (unsigned long long)s[DFK_OFFSETS_SURVIVORS], (unsigned long long)n_lookups, (unsigned long long)n_batches,
          ms_cand, ms_bits, ms_compact, 1e3 * s_tail, 1e3 * s_copy);
    return 0;
}

// the file into `dir`: whole, or not at all
int offsets_write(const OffsetsResult* R, const std::string& dir)
{
    using namespace dfk_offsets;
    const std::string path = dir + "/a.close.offsets";
    const uint64_t n = R->starts.size() - 1;
    const int fd = open(path.c_str(), O_WRONLY | O_CREAT | O_TRUNC, 0666);
    if (fd < 0) return fail(DFK_E_ARG, "cannot open %s", path.c_str());
    const dfk_closer::BinHead h = dfk_closer::head_of(MAGIC, n);
    bool bad = pwrite_all(fd, &h, 16, 0) != 0 || pwrite_all(fd, R->starts.data(), 8 * (n + 1), 16) != 0;
    if (!bad && n) bad = pwrite_all(fd, R->words.data(), 16 * n, words_at(n)) != 0;
    if (!bad && !R->recs.empty()) bad = pwrite_all(fd, R->recs.data(), 32 * R->recs.size(), recs_at(n)) != 0;
    if (close(fd) != 0) bad = true;
    if (bad) { (void)unlink(path.c_str()); return fail(DFK_E_ARG, "short write to %s", path.c_str()); }
    return 0;
}

// the latest dfk_offsets_build*'s result: one a context, kept beside the graph
int offsets_result_of(dfk_ctx* c, OffsetsResult** out)
{
    if (!c) return fail(DFK_E_ARG, "null context");
    if (!c->graph_state || !graph_of(c)->offsets) return fail(DFK_E_STATE, "no offsets: call dfk_offsets_build or dfk_offsets_build_arrays");
    *out = graph_of(c)->offsets;
    return 0;
}
void offsets_keep(dfk_ctx* c, OffsetsResult* R)
{
    HostGraph* G = graph_of(c);
    if (G->offsets) offsets_result_free(G->offsets);
    G->offsets = R; G->offsets_free = offsets_result_free;
}

} // namespace

extern "C" {

int dfk_offsets_build(dfk_ctx* c)
{
    return guarded([&]() -> int {
    ConsResult* C = nullptr;
    if (int rc = cons_result_of(c, &C)) return rc;                                       // DFK_E_STATE without a dfk_cons_build* result
    const uint64_t n = C->starts.size() - 1;
    if (n % 2) return fail(DFK_E_STATE, "the stack consensus holds %llu elements: not two a pair", (unsigned long long)n);
    if (int bad = dfk_offsets::check_input(n / 2, C->starts.data(), C->bases.data())) return fail(DFK_E_STATE, "the stack consensus is not what dfk_cons_build makes (%d)", bad);
    HIP_TRY(hipSetDevice(c->device));
    std::unique_ptr<OffsetsResult> R(new OffsetsResult);
    if (int rc = offsets_build(c, n / 2, C->starts.data(), C->bases.data(), 0, R.get())) return rc;     // (refused: the earlier result is still served)
    R->cons_serial = C->serial;
    offsets_keep(c, R.release());
    return 0;
    });
}

int dfk_offsets_build_arrays(dfk_ctx* c, uint64_t n_pairs, const uint64_t* starts, const uint8_t* bases, uint64_t pairs_per_batch, const char* dir)
{
    return guarded([&]() -> int {
    if (!c) return fail(DFK_E_ARG, "null context");
    if (!starts) return fail(DFK_E_ARG, "null argument");
    if (n_pairs >= (1ull << 31)) return fail(DFK_E_ARG, "%llu pairs: 2^31 - 1 at most", (unsigned long long)n_pairs);
    if (starts[0] != 0) return fail(DFK_E_ARG, "the starts do not begin at 0");
    for (uint64_t q = 0; q < 2 * n_pairs; ++q) {
        if (starts[q + 1] < starts[q]) return fail(DFK_E_ARG, "the starts fall at element %llu", (unsigned long long)q);
        if (starts[q + 1] - starts[q] > (uint64_t)dfk_offsets::MAX_N) return fail(DFK_E_ARG, "element %llu is %llu bases long: a consensus has %d at most", (unsigned long long)q, (unsigned long long)(starts[q + 1] - starts[q]), dfk_offsets::MAX_N);
    }
    if (starts[2 * n_pairs] && !bases) return fail(DFK_E_ARG, "null argument");
    for (uint64_t i = 0; i < starts[2 * n_pairs]; ++i) if (bases[i] > 3) return fail(DFK_E_ARG, "base %u at %llu", bases[i], (unsigned long long)i);
    HIP_TRY(hipSetDevice(c->device));
    const uint8_t none = 0;
    std::unique_ptr<OffsetsResult> R(new OffsetsResult);
    if (int rc = offsets_build(c, n_pairs, starts, bases ? bases : &none, pairs_per_batch, R.get())) return rc;
    if (dir) if (int rc = offsets_write(R.get(), dir)) return rc;
    offsets_keep(c, R.release());
    return 0;
    });
}

int dfk_offsets_stats(dfk_ctx* c, uint64_t* out)
{
    return guarded([&]() -> int {
    OffsetsResult* R = nullptr;
    if (int rc = offsets_result_of(c, &R)) return rc;
    if (!out) return fail(DFK_E_ARG, "null argument");
    for (int i = 0; i < DFK_OFFSETS_WORDS; ++i) out[i] = R->stats[i];
    return 0;
    });
}

int dfk_offsets_fetch(dfk_ctx* c, uint64_t* starts, uint32_t* words, uint64_t* n_pairs, void* records, uint64_t records_cap, uint64_t* n_records)
{
    return guarded([&]() -> int {
    OffsetsResult* R = nullptr;
    if (int rc = offsets_result_of(c, &R)) return rc;
    const uint64_t n = R->starts.size() - 1, nr = R->recs.size();
    if (n_pairs) *n_pairs = n;
    if (n_records) *n_records = nr;
    if ((records || records_cap) && records_cap < nr) return fail(DFK_E_ARG, "buffer too small: %llu < %llu records", (unsigned long long)records_cap, (unsigned long long)nr);
    if (records_cap && nr && !records) return fail(DFK_E_ARG, "null argument");
    if (records && nr) memcpy(records, R->recs.data(), 32 * nr);
    if (starts) memcpy(starts, R->starts.data(), 8 * (n + 1));                   // the starts: room for n_pairs + 1 words
    if (words && n) memcpy(words, R->words.data(), 16 * n);                      // the words: room for 4 * n_pairs u32
    return 0;
    });
}

int dfk_offsets_write(dfk_ctx* c, const char* dir)
{
    return guarded([&]() -> int {
    OffsetsResult* R = nullptr;
    if (int rc = offsets_result_of(c, &R)) return rc;
    if (!dir) return fail(DFK_E_ARG, "null directory");
    return offsets_write(R, dir);
    });
}

} // extern "C"
