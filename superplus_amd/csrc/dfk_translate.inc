// superplus_amd/csrc/dfk_translate.inc -- the read paths moved onto the patched graph (TranslatePaths and Validate, the end of StagePatch,
// 10X/runstages/RunStages.cc:364-371), included by dfk.hip.
//
// The rule, the shared pieces, the bound and the plan: dfk_translate.h.  The kernels: dfk_translate_kernels.h.  Here: translate_run() --
// the tables sent once, then per batch of paths decide, the host route for flagged reads (the batch's words come back whole, as
// dfk_paths_fetch reads them: only hand-made paths get here), the scan over the units' word counts, the result batch allocated to the
// scan's total, emit.  The scratch is that of the largest batch, from the arena and back before the call returns; the result's blocks stay
// in the arena until translate_free.  The context's paths, marks, index and every earlier result are only read.
#include "dfk_translate_kernels.h"

namespace {

struct TranslateResult {
    std::vector<PathBatch> batches;
    uint64_t n_reads = 0, n_placed = 0, var_total = 0;
    uint64_t stats[DFK_TRANSLATE_WORDS] = {};
};
void translate_free(dfk_ctx* c, TranslateResult* R)
{
    if (c) for (PathBatch& b : R->batches) { c->release(b.var); c->release(b.elem_off); }
    delete R;
}

// t_in: when the extern "C" call began
int translate_run(dfk_ctx* c, const std::vector<PathBatch>& src, uint64_t n_reads, const dfk_translate::Tables& T, const double t_in, TranslateResult* R)
{
    using namespace dfk_translate;
    const std::string why = check_tables(T);
    if (!why.empty()) return fail(DFK_E_ARG, "translate: %s", why.c_str());
    if (T.n_edges() >= (1ull << 31) || T.kmers3.size() >= (1ull << 31)) return fail(DFK_E_ARG, "translate: %llu old edges, %llu of hb3: 2^31 - 1 at most", (unsigned long long)T.n_edges(), (unsigned long long)T.kmers3.size());
    const unsigned cus = (unsigned)c->prop.multiProcessorCount;
    const uint64_t mark = c->alloc_seq;
    uint64_t max_n = 0;
    for (const PathBatch& b : src) max_n = std::max(max_n, b.n);
    const Plan plan = plan_of(max_n);
    const unsigned max_grid = std::max(1u, grid_256(max_n, cus));
    float ms_decide = 0, ms_scan = 0, ms_emit = 0;
    double s_host = 0, s_copy = 0;
    uint64_t n_host = 0, host_walk = 0, host_ranoff = 0, host_edge_ch = 0, host_off_ch = 0;
    std::vector<uint64_t> slots((size_t)max_grid * TP_SLOTS, 0);
    auto body = [&]() -> int {
        int rc;
        Timer tm(c->stream);
        double t0 = wall_now();
        DevBuf d_first, d_to3, d_left, d_kmers, d_rec, d_words, d_at, d_flag, d_ctr, d_slots;
        if ((rc = cn_up(c, d_first, T.to3_first.data(), T.to3_first.size() * 8, "to3_first")) || (rc = cn_up(c, d_to3, T.to3.data(), T.to3.size() * 4, "to3")) ||
            (rc = cn_up(c, d_left, T.left3.data(), T.left3.size() * 4, "left3")) || (rc = cn_up(c, d_kmers, T.kmers3.data(), T.kmers3.size() * 4, "K-mers of hb3's edges")) ||
            (rc = c->alloc(d_rec, std::max<uint64_t>(8, max_n * 8), "translated records", Place::Low)) || (rc = c->alloc(d_words, plan.scan_words * 8, "words per unit", Place::Low)) ||
            (rc = c->alloc(d_at, plan.scan_words * 8, "words before a unit", Place::Low)) || (rc = c->alloc(d_flag, std::max<uint64_t>(4, max_n * 4), "flagged reads", Place::Low)) ||
            (rc = c->alloc(d_ctr, 64, "translate counters", Place::Low)) || (rc = c->alloc(d_slots, slots.size() * 8, "translate counters per workgroup", Place::Low))) return rc;
        HIP_TRY(hipMemsetAsync(d_slots.p, 0, slots.size() * 8, c->stream));
        s_copy += wall_now() - t0;
        const TpTables tt{(const uint64_t*)d_first.p, (const int32_t*)d_to3.p, (const int32_t*)d_left.p, (const int32_t*)d_kmers.p, (uint32_t)T.n_edges(), (uint32_t)T.kmers3.size(), T.K};
        uint64_t file_at = 24;
        for (const PathBatch& b : src) {
            PathBatch B; B.r0 = b.r0; B.n = b.n; B.file_base = file_at;
            const Plan bp = plan_of(b.n);
            const unsigned grid = std::max(1u, grid_256(b.n, cus));
            uint64_t total_words = 0;
            if (b.n) {
                // ---- decide
                tm.start();
                HIP_TRY(hipMemsetAsync(d_ctr.p, 0, 8, c->stream));
                hipLaunchKernelGGL(k_tp_decide, dim3(grid), dim3(256), 0, c->stream, (const uint32_t*)b.var.p, (const uint32_t*)b.elem_off.p, b.n, b.var_bytes, tt, (int2*)d_rec.p,
                                   (uint64_t*)d_words.p, (uint32_t*)d_flag.p, (unsigned int*)d_ctr.p, (unsigned long long*)d_slots.p);
                HIP_TRY(hipGetLastError());
                uint32_t n_flag = 0;
                HIP_TRY(hipMemcpyAsync(&n_flag, d_ctr.p, 4, hipMemcpyDeviceToHost, c->stream));
                HIP_TRY(hipStreamSynchronize(c->stream));
                ms_decide += tm.stop();
                if (n_flag > b.n) return fail(DFK_E_HIP, "translate: %u reads flagged in a batch of %llu", n_flag, (unsigned long long)b.n);
                // ---- the host route: literal() on the flagged reads' whole paths
                if (n_flag) {
                    t0 = wall_now();
                    std::vector<uint32_t> ids(n_flag), var(b.var_bytes / 4), eo(b.n);
                    HIP_TRY(hipMemcpy(ids.data(), d_flag.p, (uint64_t)n_flag * 4, hipMemcpyDeviceToHost));
                    HIP_TRY(hipMemcpy(var.data(), b.var.p, b.var_bytes, hipMemcpyDeviceToHost));
                    HIP_TRY(hipMemcpy(eo.data(), b.elem_off.p, b.n * 4, hipMemcpyDeviceToHost));
                    std::sort(ids.begin(), ids.end());
                    std::vector<int4> fixes(n_flag);
                    std::vector<uint2> gains;
                    Path p;
                    for (uint32_t k = 0; k < n_flag; ++k) {
                        const uint64_t i = ids[k];
                        if (i >= b.n || (k && ids[k - 1] == ids[k])) return fail(DFK_E_HIP, "translate: the list of flagged reads names read %llu of %llu, or one twice", (unsigned long long)i, (unsigned long long)b.n);
                        const uint64_t w0 = eo[i] / 4, w1 = i + 1 < b.n ? eo[i + 1] / 4 : b.var_bytes / 4;
                        p.offset = (int32_t)var[w0];
                        p.edges.assign((const int32_t*)var.data() + w0 + 2, (const int32_t*)var.data() + w1);
                        const std::string bad = check_path(T, p);
                        if (!bad.empty()) return fail(DFK_E_ARG, "translate: %s", bad.c_str());
                        Kind kind;
                        const Outcome o = literal(T, p, &kind);
                        fixes[k] = make_int4((int)i, o.offset, o.edge, 0);
                        host_walk += kind == WALK; host_ranoff += kind == CLEARED_RANOFF;
                        host_edge_ch += o.edge != p.edges[0]; host_off_ch += o.offset != p.offset;
                        if (o.edge >= 0) {
                            const uint32_t u = (uint32_t)unit_of(i);
                            if (!gains.empty() && gains.back().x == u) ++gains.back().y; else gains.push_back(make_uint2(u, 1u));
                        }
                    }
                    n_host += n_flag;
                    DevBuf d_fix, d_gain;
                    if ((rc = cn_up(c, d_fix, fixes.data(), fixes.size() * sizeof(int4), "records settled on the host")) ||
                        (rc = cn_up(c, d_gain, gains.data(), gains.size() * sizeof(uint2), "their units' words"))) return rc;
                    hipLaunchKernelGGL(k_tp_override, dim3((n_flag + 255) / 256), dim3(256), 0, c->stream, (const int4*)d_fix.p, n_flag, (const uint2*)d_gain.p, (uint32_t)gains.size(),
                                       (int2*)d_rec.p, (uint64_t*)d_words.p);
                    HIP_TRY(hipGetLastError());
                    HIP_TRY(hipStreamSynchronize(c->stream));
                    c->release(d_gain); c->release(d_fix);
                    s_host += wall_now() - t0;
                }
                // ---- layout
                tm.start();
                if ((rc = device_scan(c, (const uint64_t*)d_words.p, (uint64_t*)d_at.p, bp.scan_words))) return rc;
                HIP_TRY(hipMemcpyAsync(&total_words, (const uint64_t*)d_at.p + bp.n_units, 8, hipMemcpyDeviceToHost, c->stream));
                HIP_TRY(hipStreamSynchronize(c->stream));
                ms_scan += tm.stop();
                if (total_words < 2 * b.n || total_words > 3 * b.n) return fail(DFK_E_HIP, "translate: %llu words for a batch of %llu reads", (unsigned long long)total_words, (unsigned long long)b.n);
            }
            B.var_bytes = total_words * 4;
            if (B.var_bytes >= (1ull << 32)) return fail(DFK_E_ARG, "translate: a batch of %llu reads holds %llu bytes of paths: its offsets keep 32 bits", (unsigned long long)B.n, (unsigned long long)B.var_bytes);
            if ((rc = c->alloc(B.var, std::max<uint64_t>(4, B.var_bytes), "a.patch.paths data")) || (rc = c->alloc(B.elem_off, std::max<uint64_t>(4, b.n * 4), "a.patch.paths offsets"))) return rc;
            R->batches.push_back(B);
            if (b.n) {
                tm.start();
                hipLaunchKernelGGL(k_tp_emit, dim3(grid), dim3(256), 0, c->stream, (const int2*)d_rec.p, b.n, b.r0, (const uint64_t*)d_at.p, (int64_t)T.kmers3.size(), (uint32_t*)B.var.p,
                                   (uint32_t*)B.elem_off.p, (unsigned long long*)d_slots.p);
                HIP_TRY(hipGetLastError());
                ms_emit += tm.stop();
            }
            file_at += B.var_bytes;
            R->var_total += B.var_bytes;
        }
        t0 = wall_now();
        HIP_TRY(hipMemcpyAsync(slots.data(), d_slots.p, slots.size() * 8, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
        c->release(d_slots); c->release(d_ctr); c->release(d_flag); c->release(d_at); c->release(d_words); c->release(d_rec);
        c->release(d_kmers); c->release(d_left); c->release(d_to3); c->release(d_first);
        s_copy += wall_now() - t0;
        return 0;
    };
    int rc;
    try { rc = body(); } catch (const std::runtime_error& e) { rc = fail(DFK_E_HIP, "%s", e.what()); }
    (void)hipStreamSynchronize(c->stream);
    if (rc) { c->release_since(mark); R->batches.clear(); return rc; }       // (the scratch and the batches made so far)
    auto give_back = [&]() { for (PathBatch& b : R->batches) { c->release(b.var); c->release(b.elem_off); } R->batches.clear(); };
    uint64_t k[TP_SLOTS] = {};
    for (unsigned g = 0; g < max_grid; ++g)
        for (int j = 0; j < TP_SLOTS; ++j) { if (j == TP_XOR) k[j] ^= slots[(size_t)g * TP_SLOTS + j]; else k[j] += slots[(size_t)g * TP_SLOTS + j]; }
    if (k[TP_BAD]) { give_back(); return fail(DFK_E_ARG, "translate: %llu paths begin with an edge the graph does not have", (unsigned long long)k[TP_BAD]); }
    if (k[TP_FLAGGED] != n_host) { give_back(); return fail(DFK_E_HIP, "translate: %llu reads flagged, %llu settled", (unsigned long long)k[TP_FLAGGED], (unsigned long long)n_host); }
    R->n_reads = n_reads;
    R->n_placed = k[TP_STEP2] + k[TP_WALK] + host_walk;
    uint64_t* s = R->stats;
    s[DFK_TRANSLATE_READS] = n_reads; s[DFK_TRANSLATE_PLACED_BEFORE] = k[TP_PLACED_BEFORE]; s[DFK_TRANSLATE_STEP2] = k[TP_STEP2]; s[DFK_TRANSLATE_WALK] = k[TP_WALK] + host_walk;
    s[DFK_TRANSLATE_CLEARED_EMPTY] = k[TP_CLEARED_EMPTY]; s[DFK_TRANSLATE_CLEARED_RANOFF] = host_ranoff; s[DFK_TRANSLATE_HOST] = n_host; s[DFK_TRANSLATE_INVALID] = k[TP_INVALID];
    s[DFK_TRANSLATE_EDGE_CHANGED] = k[TP_EDGE_CHANGED] + host_edge_ch; s[DFK_TRANSLATE_OFFSET_CHANGED] = k[TP_OFFSET_CHANGED] + host_off_ch; s[DFK_TRANSLATE_BATCHES] = src.size();
    s[DFK_TRANSLATE_PLACED] = R->n_placed; s[DFK_TRANSLATE_VAR_BYTES] = R->var_total;
    s[DFK_TRANSLATE_US] = (uint64_t)(1e6 * (wall_now() - t_in)); s[DFK_TRANSLATE_US_DECIDE] = (uint64_t)(1000.0f * ms_decide); s[DFK_TRANSLATE_US_HOST] = (uint64_t)(1e6 * s_host);
    s[DFK_TRANSLATE_US_SCAN] = (uint64_t)(1000.0f * ms_scan); s[DFK_TRANSLATE_US_EMIT] = (uint64_t)(1000.0f * ms_emit); s[DFK_TRANSLATE_US_COPY] = (uint64_t)(1e6 * s_copy);
    s[DFK_TRANSLATE_SUM] = k[TP_SUM]; s[DFK_TRANSLATE_XOR] = k[TP_XOR];
    if (R->var_total != 8 * n_reads + 4 * R->n_placed) { give_back(); return fail(DFK_E_HIP, "translate: %llu bytes laid out for %llu reads, %llu of them placed", (unsigned long long)R->var_total, (unsigned long long)n_reads, (unsigned long long)R->n_placed); }
    TRACE("translate: %llu reads in %zu batch(es), %llu placed before: %llu by the first edge, %llu by the walk, %llu cleared (no to3), %llu ran off, %llu on the host; decide %.1f ms, host %.1f ms, scan %.1f ms, emit %.1f ms",
          (unsigned long long)n_reads, src.size(), (unsigned long long)k[TP_PLACED_BEFORE], (unsigned long long)k[TP_STEP2], (unsigned long long)s[DFK_TRANSLATE_WALK], (unsigned long long)k[TP_CLEARED_EMPTY],
          (unsigned long long)host_ranoff, (unsigned long long)n_host, ms_decide, 1e3 * s_host, ms_scan, ms_emit);
    return 0;
}

int translate_result_of(dfk_ctx* c, TranslateResult** out)
{
    if (!c) return fail(DFK_E_ARG, "null context");
    if (!c->graph_state || !graph_of(c)->paths || !graph_of(c)->paths->translate) return fail(DFK_E_STATE, "no translated paths: call dfk_translate_build or dfk_translate_build_arrays");
    *out = graph_of(c)->paths->translate;
    return 0;
}
void translate_keep(dfk_ctx* c, TranslateResult* R)
{
    PathState* P = path_state_of(c, graph_of(c));
    if (P->translate) translate_free(c, P->translate);
    P->translate = R; P->translate_free = translate_free;
}

} // namespace

extern "C" {

int dfk_translate_build(dfk_ctx* c)
{
    return guarded([&]() -> int {
    const double t_in = wall_now();
    if (!c) return fail(DFK_E_ARG, "null context");
    PathState* P = built_paths(c);
    if (!P) return fail(DFK_E_STATE, "no paths: call dfk_paths_build");
    if (P->shard) return fail(DFK_E_STATE, "the paths are a rank's share of a sharded run: the patching stage runs on one GPU");
    const HostGraph* G = graph_of(c);
    const PatchResult* X = G->patch;
    if (!X) return fail(DFK_E_STATE, "no patched graph: call dfk_patch_build");
    if (!X->from_chain) return fail(DFK_E_STATE, "the patched graph came from dfk_patch_build_arrays: call dfk_patch_build");
    if (X->left3.size() != G->he.size()) return fail(DFK_E_STATE, "the patched graph was made from %zu edges, the graph has %zu: call dfk_patch_build", X->left3.size(), G->he.size());
    dfk_translate::Tables T;
    T.K = (int32_t)G->K; T.to3_first = X->to3_first; T.to3 = X->to3; T.left3 = X->left3;
    T.kmers3.resize(X->hb3.he.size());
    for (size_t e = 0; e < T.kmers3.size(); ++e) T.kmers3[e] = (int32_t)X->hb3.ce[X->hb3.he[e].ce].n;
    HIP_TRY(hipSetDevice(c->device));
    std::unique_ptr<TranslateResult> R(new TranslateResult);
    if (int rc = translate_run(c, P->batches, P->n_reads, T, t_in, R.get())) return rc;          // (refused: the earlier result is still served)
    translate_keep(c, R.release());
    return 0;
    });
}

int dfk_translate_build_arrays(dfk_ctx* c, uint64_t n_edges, const uint64_t* to3_first, const int32_t* to3, const int32_t* left3, uint64_t n_edges3, const int32_t* kmers3,
                               uint64_t n_reads, const uint64_t* first, const int32_t* edges, const int32_t* offsets, uint64_t reads_per_batch, const char* dir)
{
    return guarded([&]() -> int {
    const double t_in = wall_now();
    if (!c) return fail(DFK_E_ARG, "null context");
    const uint64_t E = n_edges, N = n_reads;
    if (!to3_first || !first || (E && !left3) || (n_edges3 && !kmers3) || (N && !offsets)) return fail(DFK_E_ARG, "null argument");
    if (N >= (1ull << 31) || E >= (1ull << 31) || n_edges3 >= (1ull << 31)) return fail(DFK_E_ARG, "%llu reads, %llu edges, %llu of hb3: 2^31 - 1 of each at most", (unsigned long long)N, (unsigned long long)E, (unsigned long long)n_edges3);
    if (to3_first[0] != 0) return fail(DFK_E_ARG, "translate: to3_first does not start at 0");
    for (uint64_t e = 0; e < E; ++e) if (to3_first[e + 1] < to3_first[e]) return fail(DFK_E_ARG, "translate: to3_first falls at edge %llu", (unsigned long long)e);
    if (to3_first[E] && !to3) return fail(DFK_E_ARG, "null argument");
    if (first[0] != 0) return fail(DFK_E_ARG, "the paths do not start at 0");
    for (uint64_t i = 0; i < N; ++i) {
        if (first[i + 1] < first[i]) return fail(DFK_E_ARG, "the paths' starts fall at read %llu", (unsigned long long)i);
        if (offsets[i] <= -dfk_translate::LIMIT || offsets[i] >= dfk_translate::LIMIT) return fail(DFK_E_ARG, "read %llu has offset %d: below 2^30 in size", (unsigned long long)i, offsets[i]);
    }
    if (first[N] && !edges) return fail(DFK_E_ARG, "null argument");
    const uint64_t per = reads_per_batch ? reads_per_batch : std::max<uint64_t>(1, N);
    for (uint64_t r0 = 0; r0 < N; r0 += per) {                                                  // (before any edge is read: `first` alone says how many there are)
        const uint64_t n = std::min(per, N - r0), bytes = 8 * n + 4 * (first[r0 + n] - first[r0]);
        if (bytes >= (1ull << 32)) return fail(DFK_E_ARG, "a batch of %llu reads holds %llu bytes of paths: its offsets keep 32 bits", (unsigned long long)n, (unsigned long long)bytes);
    }
    for (uint64_t k = 0; k < first[N]; ++k) if (edges[k] < 0 || (uint64_t)edges[k] >= E) return fail(DFK_E_ARG, "a path holds edge %d: the graph has %llu", edges[k], (unsigned long long)E);
    dfk_translate::Tables T;
    T.K = (int32_t)c->cfg.K;
    T.to3_first.assign(to3_first, to3_first + E + 1); T.to3.assign(to3, to3 + to3_first[E]); T.left3.assign(left3, left3 + E); T.kmers3.assign(kmers3, kmers3 + n_edges3);
    HIP_TRY(hipSetDevice(c->device));
    std::unique_ptr<TranslateResult> R(new TranslateResult);
    std::vector<PathBatch> batches;
    const uint64_t mark = c->alloc_seq;
    auto body = [&]() -> int {
        int rc;
        std::vector<uint32_t> var, off;
        for (uint64_t r0 = 0; r0 < N; r0 += per) {
            PathBatch B; B.r0 = r0; B.n = std::min(per, N - r0); B.file_base = 24 + 8 * r0 + 4 * first[r0];
            layout_batch(first, edges, offsets, r0, B.n, var, off);
            B.var_bytes = var.size() * 4;
            if ((rc = upload_vec(c, B.var, var, "a.paths data")) || (rc = upload_vec(c, B.elem_off, off, "a.paths offsets"))) return rc;
            batches.push_back(B);
        }
        return 0;
    };
    int rc;
    try { rc = body(); } catch (const std::runtime_error& e) { rc = fail(DFK_E_HIP, "%s", e.what()); }
    if (!rc) rc = translate_run(c, batches, N, T, t_in, R.get());
    (void)hipStreamSynchronize(c->stream);
    if (rc) { c->release_since(mark); return rc; }
    for (PathBatch& b : batches) { c->release(b.var); c->release(b.elem_off); }                  // the given paths; the result's blocks stay
    translate_keep(c, R.release());
    return dir ? dfk_translate_write(c, dir) : 0;
    });
}

int dfk_translate_stats(dfk_ctx* c, uint64_t* out)
{
    return guarded([&]() -> int {
    TranslateResult* R = nullptr;
    if (int rc = translate_result_of(c, &R)) return rc;
    if (!out) return fail(DFK_E_ARG, "null argument");
    for (int i = 0; i < DFK_TRANSLATE_WORDS; ++i) out[i] = R->stats[i];
    return 0;
    });
}

int dfk_translate_fetch(dfk_ctx* c, int32_t* offsets, uint64_t* first_edge, int32_t* edges, uint64_t edges_cap)
{
    return guarded([&]() -> int {
    TranslateResult* R = nullptr;
    if (int rc = translate_result_of(c, &R)) return rc;
    if ((!offsets && R->n_reads) || !first_edge || (!edges && R->n_placed)) return fail(DFK_E_ARG, "null argument");
    if (edges_cap < R->n_placed) return fail(DFK_E_ARG, "buffer too small: %llu < %llu path edges", (unsigned long long)edges_cap, (unsigned long long)R->n_placed);
    HIP_TRY(hipSetDevice(c->device));
    uint64_t at = 0;
    std::vector<uint32_t> var, eo;
    for (const PathBatch& b : R->batches) {
        var.resize(b.var_bytes / 4); eo.resize(b.n);
        if (b.var_bytes) HIP_TRY(hipMemcpy(var.data(), b.var.p, b.var_bytes, hipMemcpyDeviceToHost));
        if (b.n) HIP_TRY(hipMemcpy(eo.data(), b.elem_off.p, b.n * 4, hipMemcpyDeviceToHost));
        for (uint64_t i = 0; i < b.n; ++i) {
            const uint64_t w0 = eo[i] / 4, w1 = i + 1 < b.n ? eo[i + 1] / 4 : b.var_bytes / 4;
            if (w1 < w0 + 2 || w1 > var.size() || at + (w1 - w0 - 2) > R->n_placed) return fail(DFK_E_HIP, "translate: read %llu's element is not where the scan put it", (unsigned long long)(b.r0 + i));
            offsets[b.r0 + i] = (int32_t)var[w0];
            first_edge[b.r0 + i] = at;
            for (uint64_t w = w0 + 2; w < w1; ++w) edges[at++] = (int32_t)var[w];
        }
    }
    first_edge[R->n_reads] = at;
    return 0;
    });
}

int dfk_translate_write(dfk_ctx* c, const char* dir)
{
    return guarded([&]() -> int {
    TranslateResult* R = nullptr;
    if (int rc = translate_result_of(c, &R)) return rc;
    if (!dir) return fail(DFK_E_ARG, "null directory");
    HIP_TRY(hipSetDevice(c->device));
    const std::string path = std::string(dir) + "/a.patch.paths";
    const FeudalLayout lay = feudal_layout(R->n_reads, 24, 4, R->var_total);
    const int fd = open(path.c_str(), O_WRONLY | O_CREAT | O_TRUNC, 0666);
    if (fd < 0) return fail(DFK_E_ARG, "cannot open %s", path.c_str());
    return path_batches_to_file(c, fd, path.c_str(), lay, R->n_reads, R->batches, false);
    });
}

int dfk_translate_drop(dfk_ctx* c)
{
    return guarded([&]() -> int {
    if (!c) return fail(DFK_E_ARG, "null context");
    if (!c->graph_state || !graph_of(c)->paths || !graph_of(c)->paths->translate) return 0;
    PathState* P = graph_of(c)->paths;
    translate_free(c, P->translate);
    P->translate = nullptr;
    return 0;
    });
}

} // extern "C"
