// superplus_amd/csrc/dfk_hops.inc -- FindEdgePairs (10X/Closomatic.cc:17-358, the second call of StagePatch,
// 10X/runstages/RunStages.cc:204-205) and the file a.hops (10X/DF.cc:603), included by dfk.hip.
//
// The rule: dfk_hops.h.  The kernels: dfk_hops_kernels.h.  Here: the combined index a range of edges at a time (the ranges
// of the paths index: DFK_PIDX_RANGE_PAIRS forces small ones), the three methods per range, the host's exact route for the
// edges whose sets outgrew the LDS capacities (DFK_HOPS_MAX_SEQS / DFK_HOPS_MAX_LEN), the sorted union.  Everything on the
// device comes from the arena and goes back before the call returns; the result stays in host memory with the paths' state.
#include "dfk_hops_kernels.h"

namespace {

// the paths with MarkBads' sums beside them (the `bad` argument of FindEdgePairs), or an error
int hops_of(dfk_ctx* c, PathState** out)
{
    if (!c) return fail(DFK_E_ARG, "null context");
    if (!(c->cfg.flags & DFK_F_MARK_BADS)) return fail(DFK_E_STATE, "no edge pairs: the context was created without DFK_F_MARK_BADS (FindEdgePairs takes MarkBads' marks)");
    PathState* P = built_paths(c);
    if (!P || !P->bad_sums.p) return fail(DFK_E_STATE, "no edge pairs: call dfk_paths_build (on a context created with DFK_F_MARK_BADS)");
    *out = P;
    return 0;
}

void hops_drop_arrays(dfk_ctx* c)
{
    HostGraph* G = graph_of(c);
    if (G->hops_arrays) { path_state_free(G->hops_arrays); G->hops_arrays = nullptr; }
}

// the latest build's result: dfk_hops_build_arrays keeps its own beside the graph until the next build of either kind
int hops_result_of(dfk_ctx* c, PathState** out)
{
    if (c && (c->cfg.flags & DFK_F_MARK_BADS) && c->graph_state && graph_of(c)->hops_arrays) { *out = graph_of(c)->hops_arrays; return 0; }
    if (int rc = hops_of(c, out)) return rc;
    if (!(*out)->hops_valid) return fail(DFK_E_STATE, "no edge pairs: call dfk_hops_build");
    return 0;
}

// The exact route's paths: those of the reads on an edge's list and of their mates, gathered on the device (their lengths,
// then their edges behind one another) and brought over in two copies an edge, whatever the length of the list.
struct HopsFetched {
    std::vector<uint32_t> ids;                                            // ascending
    std::vector<uint64_t> off;                                            // [ids.size() + 1]
    std::vector<int32_t> edges;
    int len(uint32_t id, const int32_t** p) const
    {
        const size_t i = (size_t)(std::lower_bound(ids.begin(), ids.end(), id) - ids.begin());
        *p = edges.data() + off[i];
        return (int)(off[i + 1] - off[i]);
    }
};

int hops_fetch_paths(dfk_ctx* c, const HopsPaths& paths, const std::vector<uint32_t>& list, HopsFetched* F)
{
    F->ids.clear();
    for (uint32_t v : list) { F->ids.push_back(v >> 1); F->ids.push_back((v >> 1) ^ 1u); }
    std::sort(F->ids.begin(), F->ids.end());
    F->ids.erase(std::unique(F->ids.begin(), F->ids.end()), F->ids.end());
    const uint64_t n = F->ids.size();
    F->off.assign(n + 1, 0); F->edges.assign(1, 0);
    if (!n) return 0;
    const uint64_t mark = c->alloc_seq;
    DevBuf d_ids, d_lens, d_off, d_out;
    int rc;
    if ((rc = upload_vec(c, d_ids, F->ids, "reads of an edge for the host")) || (rc = c->alloc(d_lens, n * 4, "their path lengths", Place::Low))) return rc;
    const unsigned grid = (unsigned)std::min<uint64_t>((n + 255) / 256, 1024);
    hipLaunchKernelGGL(k_hops_path_lens, dim3(grid), dim3(256), 0, c->stream, (const uint32_t*)d_ids.p, n, paths, (uint32_t*)d_lens.p);
    HIP_TRY(hipGetLastError());
    std::vector<uint32_t> lens(n);
    HIP_TRY(hipMemcpyAsync(lens.data(), d_lens.p, n * 4, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    for (uint64_t i = 0; i < n; ++i) F->off[i + 1] = F->off[i] + lens[i];
    const uint64_t total = F->off[n];
    F->edges.assign(total + 1, 0);
    if (total) {
        if ((rc = upload_vec(c, d_off, F->off, "their places")) || (rc = c->alloc(d_out, total * 4, "their paths", Place::Low))) return rc;
        hipLaunchKernelGGL(k_hops_path_copy, dim3(grid), dim3(256), 0, c->stream, (const uint32_t*)d_ids.p, n, paths, (const uint64_t*)d_off.p, (int32_t*)d_out.p);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(F->edges.data(), d_out.p, total * 4, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
    }
    c->release_since(mark);
    return 0;
}

// bc: host [n_reads] (or null with d_bc_given: already on the device, expanded from a barcode index)
int hops_build(dfk_ctx* c, HostGraph* G, PathState* P, const int32_t* bc, const int64_t* bci, uint64_t n_bci, int one_good)
{
    const uint64_t N = P->n_reads, n_he = G->he.size();
    if (N % 2) return fail(DFK_E_ARG, "%llu reads: FindEdgePairs works on pairs", (unsigned long long)N);
    if (N >= (1ull << 31)) return fail(DFK_E_ARG, "%llu reads: the combined index keeps a read's number in 31 bits", (unsigned long long)N);
    if (n_he >= (1ull << 31)) return fail(DFK_E_ARG, "%llu edges", (unsigned long long)n_he);
    if (bci && (n_bci < 2 || bci[0] != 0 || (uint64_t)bci[n_bci - 1] != N)) return fail(DFK_E_ARG, "the barcode index does not describe %llu reads", (unsigned long long)N);
    if (bc) for (uint64_t i = 0; i < N; ++i) if (bc[i] < 0) return fail(DFK_E_ARG, "read %llu has barcode %d: barcodes are not negative", (unsigned long long)i, bc[i]);
    P->hops_valid = false; P->hops.clear();
    for (uint64_t& w : P->hops_stats) w = 0;
    const int K = (int)c->cfg.K;
    int max_seqs = 96, max_len = 24;                                      // what the largest fixture asks for (71 sequences of 15 edges) and a third more
    if (const char* e = getenv("DFK_HOPS_MAX_SEQS")) max_seqs = std::max(1, atoi(e));
    if (const char* e = getenv("DFK_HOPS_MAX_LEN")) max_len = std::max(1, atoi(e));
    const dfk_hops::Caps cp = dfk_hops::caps_of(max_seqs, max_len);
    if (cp.words() * 4 > 64 * 1024) return fail(DFK_E_ARG, "DFK_HOPS_MAX_SEQS=%d x DFK_HOPS_MAX_LEN=%d asks for %llu bytes of LDS a wave: 65536 at most", max_seqs, max_len, (unsigned long long)(cp.words() * 4));
    int rc = paths_tables(c, G, P); if (rc) return rc;
    const unsigned cus = (unsigned)c->prop.multiProcessorCount;
    const double t_in = wall_now();
    const uint64_t mark = c->alloc_seq;
    std::vector<std::pair<int32_t, int32_t>> by_method[3];
    uint64_t searched = 0, extended = 0, host_edges = 0, most_rounds = 0, largest_x = 0, n_ranges = 0;
    float ms_index = 0, ms_mates = 0, ms_edges = 0; double s_host = 0;
    // the graph's per-edge tables on both sides
    std::vector<int32_t> kmers(n_he), inv(n_he), hl(n_he), hr(n_he);
    for (size_t e = 0; e < n_he; ++e) {
        kmers[e] = (int32_t)G->ce[G->he[e].ce].n; inv[e] = G->he[e].rc ? G->fwd[G->he[e].ce] : G->rev[G->he[e].ce];
        hl[e] = G->he[e].v; hr[e] = G->he[e].w;
    }
    const dfk_hops::Graph hg{kmers.data(), inv.data(), hl.data(), hr.data(), G->from_start.data(), G->from_v.data(), G->from_e.data(),
                             G->to_start.data(), G->to_v.data(), G->to_e.data()};
    std::vector<int32_t> h_bc; std::vector<uint16_t> h_sums;              // fetched when the exact route first needs them
    auto body = [&]() -> int {
        if (!n_he || !N) return 0;
        Timer tm(c->stream);
        DevBuf d_kmers, d_inv, d_bc, d_bci, d_batches, flags, seen, c64, first, ctr;
        if ((rc = upload_vec(c, d_kmers, kmers, "edge k-mers")) || (rc = upload_vec(c, d_inv, inv, "involution"))) return rc;
        if ((rc = c->alloc(d_bc, N * 4, "barcode ids", Place::Low))) return rc;
        if (bci) {
            if ((rc = c->alloc(d_bci, n_bci * 8, "barcode index", Place::Low))) return rc;
            HIP_TRY(hipMemcpyAsync(d_bci.p, bci, n_bci * 8, hipMemcpyHostToDevice, c->stream));
            hipLaunchKernelGGL(k_expand_bci, dim3((unsigned)std::min<uint64_t>((N + 255) / 256, 32ull * cus)), dim3(256), 0, c->stream, (const int64_t*)d_bci.p, n_bci, N, (int32_t*)d_bc.p);
            HIP_TRY(hipGetLastError());
            HIP_TRY(hipStreamSynchronize(c->stream));
            c->release(d_bci);
        } else {
            HIP_TRY(hipMemcpyAsync(d_bc.p, bc, N * 4, hipMemcpyHostToDevice, c->stream));
            HIP_TRY(hipStreamSynchronize(c->stream));
        }
        std::vector<HopsBatch> hb;
        for (const PathBatch& b : P->batches) hb.push_back(HopsBatch{(const uint32_t*)b.var.p, (const uint32_t*)b.elem_off.p, b.r0, b.n, b.var_bytes});
        if ((rc = upload_vec(c, d_batches, hb, "path batches"))) return rc;
        const HopsPaths paths{(const HopsBatch*)d_batches.p, (uint32_t)hb.size()};
        const HopsBad bad{(const uint16_t*)P->bad_sums.p};
        const dfk_hops::Graph dg{(const int32_t*)d_kmers.p, (const int32_t*)d_inv.p, (const int32_t*)P->he_left.p, (const int32_t*)P->he_right.p,
                                 (const uint32_t*)P->from_start.p, (const int32_t*)P->from_vtx.p, (const int32_t*)P->from_edge.p,
                                 (const uint32_t*)P->to_start.p, (const int32_t*)P->to_vtx.p, (const int32_t*)P->to_edge.p};
        // ---- the combined index's counts and list starts; the two tests per edge
        tm.start();
        if ((rc = c->alloc(flags, n_he, "sink / source flags", Place::Low)) || (rc = c->alloc(seen, n_he, "edges method 1 served", Place::Low)) ||
            (rc = c->alloc(c64, (n_he + 1) * 8, "reads per edge and involution", Place::Low)) ||
            (rc = c->alloc(first, (n_he + 1) * 8, "list starts", Place::Low)) || (rc = c->alloc(ctr, 8 * HC_N, "hops counters", Place::Low))) return rc;
        HIP_TRY(hipMemsetAsync(seen.p, 0, n_he, c->stream));
        HIP_TRY(hipMemsetAsync(c64.p, 0, (n_he + 1) * 8, c->stream));
        const unsigned egrid = (unsigned)std::min<uint64_t>((n_he + 255) / 256, 32ull * cus);
        for (const PathBatch& b : P->batches)
            hipLaunchKernelGGL(k_hops_count, dim3((unsigned)std::min<uint64_t>((b.n + 255) / 256, 32ull * cus)), dim3(256), 0, c->stream, (const uint32_t*)b.var.p,
                               (const uint32_t*)b.elem_off.p, b.n, b.var_bytes, (const int32_t*)d_inv.p, (unsigned long long*)c64.p);
        hipLaunchKernelGGL(k_hops_flags, dim3(egrid), dim3(256), 0, c->stream, dg, n_he, (uint8_t*)flags.p);
        HIP_TRY(hipGetLastError());
        rc = device_scan(c, (const uint64_t*)c64.p, (uint64_t*)first.p, n_he + 1); if (rc) return rc;
        std::vector<uint64_t> h_first(n_he + 1);
        HIP_TRY(hipMemcpyAsync(h_first.data(), first.p, (n_he + 1) * 8, hipMemcpyDeviceToHost, c->stream));
        ms_index += tm.stop();
        if (h_first[n_he] != 2 * P->n_edges) return fail(DFK_E_HIP, "edge pairs: the combined index counts %llu entries, the paths hold %llu", (unsigned long long)h_first[n_he], (unsigned long long)P->n_edges);
        c->release(c64);
        // ---- a range of edges at a time: 4 bytes an entry for the lists, 26 for the table at load <= 0.5, 24 for two results
        uint64_t cap = std::min<uint64_t>((1ull << 31) - 1, std::max<uint64_t>(1ull << 20, c->largest_allocatable() / 2 / 64));
        if (const char* e = getenv("DFK_PIDX_RANGE_PAIRS")) cap = std::max<uint64_t>(1, (uint64_t)atoll(e));
        for (uint64_t e0 = 0; e0 < n_he;) {
            uint64_t e1 = e0 + 1;
            while (e1 < n_he && h_first[e1 + 1] - h_first[e0] <= cap) ++e1;
            const uint64_t n_r = h_first[e1] - h_first[e0], ne = e1 - e0;
            if (n_r >= (1ull << 32)) return fail(DFK_E_ARG, "edge %llu alone is on %llu reads: a list of the combined index is placed with 32-bit cursors", (unsigned long long)e0, (unsigned long long)n_r);
            ++n_ranges;
            if (n_r) {
                const uint64_t rmark = c->alloc_seq;
                DevBuf vals, cursor, tk, tb, tmk, host_list, out;
                const uint64_t slots = 1ull << std::max<uint32_t>(10, ceil_log2(2 * n_r));
                if ((rc = c->alloc(vals, n_r * 4, "combined index lists", Place::Low)) || (rc = c->alloc(cursor, ne * 4, "list cursors", Place::Low)) ||
                    (rc = c->alloc(tk, slots * 8, "edge pair keys", Place::Low)) || (rc = c->alloc(tb, slots * 4, "edge pair ids", Place::Low)) ||
                    (rc = c->alloc(tmk, slots, "edge pair marks", Place::Low)) || (rc = c->alloc(host_list, ne * 4, "edges for the host", Place::Low))) return rc;
                tm.start();
                HIP_TRY(hipMemsetAsync(cursor.p, 0, ne * 4, c->stream));
                for (const PathBatch& b : P->batches)
                    hipLaunchKernelGGL(k_hops_scatter, dim3((unsigned)std::min<uint64_t>((b.n + 255) / 256, 32ull * cus)), dim3(256), 0, c->stream, (const uint32_t*)b.var.p,
                                       (const uint32_t*)b.elem_off.p, b.n, b.r0, b.var_bytes, (const int32_t*)d_inv.p, (uint32_t)e0, (uint32_t)e1, (const uint64_t*)first.p,
                                       (uint32_t*)cursor.p, (uint32_t*)vals.p);
                HIP_TRY(hipGetLastError());
                ms_index += tm.stop();
                // methods 1 and 2: the gather once, the verdicts below (idempotent: a larger result buffer repeats only them)
                tm.start();
                hipLaunchKernelGGL(k_fill_u64, dim3(4096), dim3(256), 0, c->stream, (uint64_t*)tk.p, slots, ~0ull);
                HIP_TRY(hipMemsetAsync(tb.p, 0xFF, slots * 4, c->stream));
                HIP_TRY(hipMemsetAsync(tmk.p, 0, slots, c->stream));
                const unsigned wgrid = (unsigned)std::min<uint64_t>(ne, 64ull * cus);
                hipLaunchKernelGGL(k_hops_mates, dim3(wgrid), dim3(64), 0, c->stream, (uint32_t)e0, (uint32_t)e1, (const uint64_t*)first.p, (const uint32_t*)vals.p,
                                   (const uint8_t*)flags.p, (const int32_t*)d_inv.p, paths, (const int32_t*)d_bc.p, (unsigned long long*)tk.p, (uint32_t*)tb.p, (uint8_t*)tmk.p, slots - 1);
                HIP_TRY(hipGetLastError());
                ms_mates += tm.stop();
                uint64_t out_cap = std::max<uint64_t>(4096, n_r / 4);
                if (const char* e = getenv("DFK_HOPS_OUT_CAP")) out_cap = std::max<uint64_t>(1, (uint64_t)atoll(e));    // (tests: the second attempt)
                uint64_t h_ctr[HC_N] = {};
                for (int attempt = 0;; ++attempt) {
                    if ((rc = c->alloc(out, out_cap * 12, "edge pairs found", Place::Low))) return rc;
                    HIP_TRY(hipMemsetAsync(ctr.p, 0, 8 * HC_N, c->stream));
                    const unsigned sgrid = (unsigned)std::min<uint64_t>((slots + 255) / 256, 32ull * cus);
                    tm.start();
                    hipLaunchKernelGGL(k_hops_m1, dim3(sgrid), dim3(256), 0, c->stream, (const unsigned long long*)tk.p, (const uint8_t*)tmk.p, slots, (const uint8_t*)flags.p, one_good,
                                       (uint8_t*)seen.p, HopsOut{(int32_t*)out.p, out_cap, (unsigned long long*)ctr.p, 1});
                    hipLaunchKernelGGL(k_hops_m2, dim3(sgrid), dim3(256), 0, c->stream, (const unsigned long long*)tk.p, (const uint8_t*)tmk.p, slots, (const uint8_t*)seen.p, dg,
                                       HopsOut{(int32_t*)out.p, out_cap, (unsigned long long*)ctr.p, 2});
                    HIP_TRY(hipGetLastError());
                    ms_mates += tm.stop();
                    tm.start();
                    hipLaunchKernelGGL(k_hops_edges, dim3(wgrid), dim3(64), (size_t)cp.words() * 4, c->stream, (uint32_t)e0, (uint32_t)e1, (const uint64_t*)first.p, (const uint32_t*)vals.p,
                                       dg, K, paths, (const int32_t*)d_bc.p, bad, cp, HopsOut{(int32_t*)out.p, out_cap, (unsigned long long*)ctr.p, 3}, (uint32_t*)host_list.p,
                                       (unsigned long long*)ctr.p);
                    HIP_TRY(hipGetLastError());
                    ms_edges += tm.stop();
                    HIP_TRY(hipMemcpy(h_ctr, ctr.p, 8 * HC_N, hipMemcpyDeviceToHost));
                    if (h_ctr[HC_INTERNAL]) return fail(DFK_E_HIP, "edge pairs: a search went past %d rounds", dfk_hops::MAX_ROUNDS);
                    if (h_ctr[HC_OUT] <= out_cap) break;
                    if (attempt) return fail(DFK_E_HIP, "edge pairs: %llu results where %llu were counted", (unsigned long long)h_ctr[HC_OUT], (unsigned long long)out_cap);
                    c->release(out); out_cap = h_ctr[HC_OUT];                // (counted in full: the second attempt fits)
                }
                std::vector<int32_t> h_out(3 * h_ctr[HC_OUT]);
                if (!h_out.empty()) HIP_TRY(hipMemcpy(h_out.data(), out.p, h_out.size() * 4, hipMemcpyDeviceToHost));
                for (size_t i = 0; i + 2 < h_out.size(); i += 3) {
                    if (h_out[i + 2] < 1 || h_out[i + 2] > 3) return fail(DFK_E_HIP, "edge pairs: a result without a method");
                    by_method[h_out[i + 2] - 1].emplace_back(h_out[i], h_out[i + 1]);
                }
                searched += h_ctr[HC_SEARCHED]; extended += h_ctr[HC_EXTENDED];
                most_rounds = std::max(most_rounds, h_ctr[HC_ROUNDS]); largest_x = std::max(largest_x, h_ctr[HC_LARGEST_X]);
                // ---- the exact route: the edges whose sets did not fit, decided from their lists and the paths fetched for them
                if (h_ctr[HC_HOST]) {
                    const double t_h = wall_now();
                    if (h_ctr[HC_HOST] > ne) return fail(DFK_E_HIP, "edge pairs: more edges for the host than the range has");
                    std::vector<uint32_t> todo(h_ctr[HC_HOST]);
                    HIP_TRY(hipMemcpy(todo.data(), host_list.p, todo.size() * 4, hipMemcpyDeviceToHost));
                    std::sort(todo.begin(), todo.end());
                    if (h_bc.empty()) { h_bc.resize(N); HIP_TRY(hipMemcpy(h_bc.data(), d_bc.p, N * 4, hipMemcpyDeviceToHost)); }
                    if (h_sums.empty()) { h_sums.resize(N); HIP_TRY(hipMemcpy(h_sums.data(), P->bad_sums.p, N * 2, hipMemcpyDeviceToHost)); }
                    const HopsBad hbad{h_sums.data()};
                    HopsFetched got;
                    for (uint32_t e : todo) {
                        std::vector<uint32_t> list(h_first[e + 1] - h_first[e]);
                        if (!list.empty()) HIP_TRY(hipMemcpy(list.data(), (const uint32_t*)vals.p + (h_first[e] - h_first[e0]), list.size() * 4, hipMemcpyDeviceToHost));
                        if ((rc = hops_fetch_paths(c, paths, list, &got))) return rc;
                        dfk_hops::EdgeStat st;
                        const int r = dfk_hops::edge_pairs_exact(hg, K, (int32_t)e, list.data(), list.size(), got, h_bc.data(), hbad, &by_method[2], &st);
                        if (r < 0) return fail(DFK_E_HIP, "edge pairs: the exact route gave up on edge %u (its sets need more than %llu MiB on the host)", e, (unsigned long long)(dfk_hops::EXACT_MAX_WORDS >> 18));
                        if (r == dfk_hops::HOPS_SKIP) return fail(DFK_E_HIP, "edge pairs: edge %u reached the search on the device and not on the host", e);
                        ++searched; extended += r == dfk_hops::HOPS_EXTENDED;
                        most_rounds = std::max<uint64_t>(most_rounds, (uint64_t)st.rounds); largest_x = std::max<uint64_t>(largest_x, (uint64_t)st.n_x);
                    }
                    host_edges += todo.size();
                    s_host += wall_now() - t_h;
                }
                c->release_since(rmark);
            }
            e0 = e1;
        }
        return 0;
    };
    try { rc = body(); } catch (const std::runtime_error& e) { rc = fail(DFK_E_HIP, "%s", e.what()); }
    (void)hipStreamSynchronize(c->stream);
    c->release_since(mark);
    if (rc) return rc;
    std::vector<std::pair<int32_t, int32_t>> all;
    for (auto& m : by_method) all.insert(all.end(), m.begin(), m.end());
    std::sort(all.begin(), all.end());
    all.erase(std::unique(all.begin(), all.end()), all.end());             // :345 UniqueSort(pairs)
    P->hops.reserve(2 * all.size());
    for (const auto& p : all) { P->hops.push_back(p.first); P->hops.push_back(p.second); }
    uint64_t* s = P->hops_stats;
    s[DFK_HOPS_M1] = by_method[0].size(); s[DFK_HOPS_M2] = by_method[1].size(); s[DFK_HOPS_M3] = by_method[2].size(); s[DFK_HOPS_PAIRS] = all.size();
    s[DFK_HOPS_SEARCHED] = searched; s[DFK_HOPS_EXTENDED] = extended; s[DFK_HOPS_HOST_EDGES] = host_edges; s[DFK_HOPS_MOST_ROUNDS] = most_rounds;
    s[DFK_HOPS_US] = (uint64_t)(1e6 * (wall_now() - t_in)); s[DFK_HOPS_US_INDEX] = (uint64_t)(1000.0f * ms_index); s[DFK_HOPS_US_M12] = (uint64_t)(1000.0f * ms_mates);
    s[DFK_HOPS_US_M3] = (uint64_t)(1000.0f * ms_edges); s[DFK_HOPS_US_HOST] = (uint64_t)(1e6 * s_host); s[DFK_HOPS_LARGEST_X] = largest_x; s[DFK_HOPS_RANGES] = n_ranges;
    P->hops_valid = true;
    TRACE("edge pairs: %zu + %zu + %zu -> %zu pairs; %llu edges searched, %llu extended, %llu on the host; %llu range(s); index %.1f ms, methods 1/2 %.1f ms, method 3 %.1f ms, host %.3f s",
          by_method[0].size(), by_method[1].size(), by_method[2].size(), all.size(), (unsigned long long)searched, (unsigned long long)extended, (unsigned long long)host_edges,
          (unsigned long long)n_ranges, ms_index, ms_mates, ms_edges, s_host);
    return 0;
}

} // namespace

extern "C" {

int dfk_hops_build(dfk_ctx* c, const int32_t* bc, int one_good)
{
    return guarded([&]() -> int {
    PathState* P = nullptr;
    if (int rc = hops_of(c, &P)) return rc;
    if (!bc && P->n_reads) return fail(DFK_E_ARG, "null barcode vector");
    HIP_TRY(hipSetDevice(c->device));
    hops_drop_arrays(c);
    return hops_build(c, graph_of(c), P, bc, nullptr, 0, one_good);
    });
}

int dfk_hops_build_bci(dfk_ctx* c, const int64_t* bci, uint64_t n_bci, int one_good)
{
    return guarded([&]() -> int {
    PathState* P = nullptr;
    if (int rc = hops_of(c, &P)) return rc;
    if (!bci) return fail(DFK_E_ARG, "null barcode index");
    HIP_TRY(hipSetDevice(c->device));
    hops_drop_arrays(c);
    return hops_build(c, graph_of(c), P, nullptr, bci, n_bci, one_good);
    });
}

// The stage on a graph and paths given as host arrays: a HostGraph and a PathState made for the call (the batches laid out as
// k_path_emit leaves them: two header words, offset and lastSkip, before a read's edges, elem_off in bytes; an unplaced read is its
// two zero words alone), then hops_build() as dfk_hops_build calls it.
int dfk_hops_build_arrays(dfk_ctx* c, uint64_t n_edges, uint64_t n_vertices, const int32_t* kmers, const int32_t* inv, const int32_t* to_left, const int32_t* to_right,
                          uint64_t n_reads, const uint64_t* first, const int32_t* edges, const int32_t* bc, const uint16_t* sums, int one_good, uint64_t reads_per_batch)
{
    return guarded([&]() -> int {
    if (!c) return fail(DFK_E_ARG, "null context");
    if (!(c->cfg.flags & DFK_F_MARK_BADS)) return fail(DFK_E_STATE, "no edge pairs: the context was created without DFK_F_MARK_BADS (FindEdgePairs takes MarkBads' marks)");
    const uint64_t E = n_edges, N = n_reads;
    if ((E && (!kmers || !inv || !to_left || !to_right)) || !first || (N && (!bc || !sums))) return fail(DFK_E_ARG, "null argument");
    if (N % 2) return fail(DFK_E_ARG, "%llu reads: FindEdgePairs works on pairs", (unsigned long long)N);
    if (N >= (1ull << 31) || E >= (1ull << 31) || n_vertices >= (1ull << 31)) return fail(DFK_E_ARG, "%llu reads, %llu edges, %llu vertices: 2^31 - 1 of each at most", (unsigned long long)N, (unsigned long long)E, (unsigned long long)n_vertices);
    for (uint64_t e = 0; e < E; ++e) {
        if (inv[e] < 0 || (uint64_t)inv[e] >= E || inv[inv[e]] != (int32_t)e) return fail(DFK_E_ARG, "inv is not an involution at edge %llu", (unsigned long long)e);
        if (kmers[e] < 1 || kmers[inv[e]] != kmers[e]) return fail(DFK_E_ARG, "edge %llu has %d k-mers, its involution %d", (unsigned long long)e, kmers[e], kmers[inv[e]]);
        if (to_left[e] < 0 || (uint64_t)to_left[e] >= n_vertices || to_right[e] < 0 || (uint64_t)to_right[e] >= n_vertices) return fail(DFK_E_ARG, "edge %llu joins a vertex out of range", (unsigned long long)e);
    }
    if (first[0] != 0) return fail(DFK_E_ARG, "the paths do not start at 0");
    for (uint64_t i = 0; i < N; ++i) {
        if (first[i + 1] < first[i]) return fail(DFK_E_ARG, "the paths' starts fall at read %llu", (unsigned long long)i);
        if (bc[i] < 0) return fail(DFK_E_ARG, "read %llu has barcode %d: barcodes are not negative", (unsigned long long)i, bc[i]);
    }
    if (first[N] && !edges) return fail(DFK_E_ARG, "null argument");
    for (uint64_t k = 0; k < first[N]; ++k) if (edges[k] < 0 || (uint64_t)edges[k] >= E) return fail(DFK_E_ARG, "a path holds edge %d: the graph has %llu", edges[k], (unsigned long long)E);
    HIP_TRY(hipSetDevice(c->device));
    hops_drop_arrays(c);
    // the graph: a canonical edge per edge and its involution, the smaller number its forward orientation
    HostGraph G;
    G.K = c->cfg.K; G.n_vertices = n_vertices; G.he.resize(E);
    for (uint64_t e = 0; e < E; ++e) {
        if ((uint64_t)inv[e] < e) continue;
        const uint32_t ce = (uint32_t)G.ce.size();
        G.ce.push_back(GraphEdge{(uint32_t)kmers[e], 0}); G.fwd.push_back((int32_t)e); G.rev.push_back(inv[e]);
        G.he[e] = HostGraph::HEdge{ce, 0, to_left[e], to_right[e]};
        if ((uint64_t)inv[e] != e) G.he[inv[e]] = HostGraph::HEdge{ce, 1, to_left[inv[e]], to_right[inv[e]]};
    }
    graph_rows(G);
    G.built = true;
    // the paths
    PathState* P = new PathState;
    P->c = c;
    struct Holder { dfk_ctx* c; PathState* P; ~Holder() { if (P) path_state_free(P); } } holder{c, P};
    const uint64_t mark = c->alloc_seq;
    const uint64_t per = reads_per_batch ? reads_per_batch : std::max<uint64_t>(1, N);
    auto body = [&]() -> int {
        int rc;
        for (uint64_t r0 = 0; r0 < N; r0 += per) {
            PathBatch B; B.r0 = r0; B.n = std::min(per, N - r0); B.file_base = 24 + 8 * r0 + 4 * first[r0];
            std::vector<uint32_t> var, off;
            layout_batch(first, edges, nullptr, r0, B.n, var, off);
            B.var_bytes = var.size() * 4;
            if (B.var_bytes >= (1ull << 32)) return fail(DFK_E_ARG, "a batch of %llu reads holds %llu bytes of paths: its offsets keep 32 bits", (unsigned long long)B.n, (unsigned long long)B.var_bytes);
            if ((rc = upload_vec(c, B.var, var, "a.paths data")) || (rc = upload_vec(c, B.elem_off, off, "a.paths offsets"))) return rc;
            P->batches.push_back(B);
        }
        if ((rc = c->alloc(P->bad_sums, std::max<uint64_t>(1, N) * 2, "bad-base sums"))) return rc;
        if (N) HIP_TRY(hipMemcpy(P->bad_sums.p, sums, N * 2, hipMemcpyHostToDevice));
        P->n_reads = N; P->n_edges = first[N]; P->built = true;
        for (uint64_t i = 0; i < N; ++i) P->n_placed += first[i + 1] > first[i];
        return hops_build(c, &G, P, bc, nullptr, 0, one_good);
    };
    int rc;
    try { rc = body(); } catch (const std::runtime_error& e) { rc = fail(DFK_E_HIP, "%s", e.what()); }
    (void)hipStreamSynchronize(c->stream);
    c->release_since(mark);                                                  // the batches, the sums, the graph's tables
    P->batches.clear(); P->built = false; P->tables = false;
    P->bad_sums = P->xlat = P->he_ce = P->he_left = P->he_right = P->from_start = P->from_vtx = P->from_edge = P->to_start = P->to_vtx = P->to_edge = DevBuf{};
    if (rc) return rc;
    holder.P = nullptr;
    graph_of(c)->hops_arrays = P;                                            // hops, hops_stats and hops_valid are what is left in it
    graph_of(c)->paths_free = path_state_free;
    return 0;
    });
}

int dfk_hops_stats(dfk_ctx* c, uint64_t* out)
{
    return guarded([&]() -> int {
    PathState* P = nullptr;
    if (int rc = hops_result_of(c, &P)) return rc;
    if (!out) return fail(DFK_E_ARG, "null argument");
    for (int i = 0; i < DFK_HOPS_WORDS; ++i) out[i] = P->hops_stats[i];
    return 0;
    });
}

int dfk_hops_fetch(dfk_ctx* c, int32_t* pairs, uint64_t cap, uint64_t* n_pairs)
{
    return guarded([&]() -> int {
    PathState* P = nullptr;
    if (int rc = hops_result_of(c, &P)) return rc;
    const uint64_t n = P->hops.size() / 2;
    if (n_pairs) *n_pairs = n;
    if (!pairs && !cap) return 0;                                          // (asked for the count alone)
    if (cap < n) return fail(DFK_E_ARG, "buffer too small: %llu < %llu pairs", (unsigned long long)cap, (unsigned long long)n);
    if (n && !pairs) return fail(DFK_E_ARG, "null argument");
    if (n) memcpy(pairs, P->hops.data(), n * 8);
    return 0;
    });
}

int dfk_hops_write(dfk_ctx* c, const char* path, uint64_t* n_pairs, uint64_t* digest)
{
    return guarded([&]() -> int {
    PathState* P = nullptr;
    if (int rc = hops_result_of(c, &P)) return rc;
    const uint64_t n = P->hops.size() / 2;
    if (path) {
        // BinaryWriter::writeFile of vec<pair<int,int>> (feudal/BinaryStream.h:447-462): "BINWRITE", the count, the pairs
        try { OutFile f(path); f.raw("BINWRITE", 8); f.pod<uint64_t>(n); f.raw(P->hops.data(), 8 * n); f.close(); }
        catch (const std::runtime_error& e) { return fail(DFK_E_ARG, "%s", e.what()); }
    }
    if (n_pairs) *n_pairs = n;
    if (digest) {
        std::vector<std::pair<int32_t, int32_t>> v(n);
        for (uint64_t i = 0; i < n; ++i) v[i] = {P->hops[2 * i], P->hops[2 * i + 1]};
        dfk_hops::pairs_digest(v, digest);
    }
    return 0;
    });
}

} // extern "C"
