// superplus_amd/csrc/dfk_patch.inc -- the patched graph from edges and closures (10X/runstages/RunStages.cc:330-360): the dictionary of
// allx, its unipath graph hb3, and the old edges' paths to3 / left3, included by dfk.hip.
//
// The rule, the shared pieces, the order of work and a.patch.to3's layout: dfk_patch.h.  The kernels: dfk_patch_kernels.h.  Here:
// patch_build() -- the tables checked (dfk_patch.h's check_graph), the base entries written, indexed and checked, the closures' K-mers
// in batches, the novel ones sorted and merged on the host, the graph kernels over the two parts (graph_edges_typed, dfk_graph.inc) into
// a HostGraph of this stage's own, build_hbv, heads / scan / emit, the paths of the inverse edges on the host.  Everything on the device
// comes from the arena and goes back before build returns; the context's own graph, index, filter and pathing state are not touched.
#include "dfk_patch_kernels.h"

namespace {

struct PatchResult {
    HostGraph hb3;
    std::vector<uint64_t> to3_first;              // [n_edges + 1]
    std::vector<int32_t> to3, left3;
    uint64_t stats[DFK_PATCH_WORDS] = {};
    bool from_chain = false;                      // made by dfk_patch_build: from the context's graph and its two closers' closures,
    std::vector<int32_t> pairs;                   // which were made for these pairs
};
void patch_result_free(PatchResult* r) { delete r; }

// 2-bit stream of sequences, a sequence anywhere; eight zero words behind it (patch_load)
struct PatchStream {
    std::vector<uint32_t> words; std::vector<uint64_t> at; uint64_t n = 0;
    void push(const dfk_patch::Seq& s)
    {
        at.push_back(n);
        words.resize((n + s.size() + 15) / 16 + 8, 0);
        for (size_t i = 0; i < s.size(); ++i, ++n) words[n >> 4] |= (uint32_t)(s[i] & 3u) << (2 * (n & 15));
    }
    void close() { words.resize((n + 15) / 16 + 8, 0); if (at.empty()) at.push_back(0); }
};

template <int K>
int patch_build_typed(dfk_ctx* c, const dfk_patch::Graph& G, const std::vector<dfk_patch::Seq>& closures, uint64_t per_batch, const double t_in, PatchResult* R)
{
    using namespace dfk_patch;
    const size_t E = G.edges.size();
    const Plan P = plan_of(G);
    const uint32_t nc = (uint32_t)P.canon.size();
    const uint64_t n_base = P.first[nc];
    uint64_t n_pos = 0, n_short = 0, crossings = 0;
    std::vector<uint64_t> cfirst(1, 0);
    for (const Seq& s : closures) { n_short += s.size() < (size_t)K; n_pos += s.size() >= (size_t)K ? s.size() - K + 1 : 0; cfirst.push_back(n_pos); }
    { std::vector<uint32_t> nt(G.n_vertices, 0), nf(G.n_vertices, 0);
      for (size_t e = 0; e < E; ++e) { ++nf[G.to_left[e]]; ++nt[G.to_right[e]]; }
      for (uint32_t v = 0; v < G.n_vertices; ++v) crossings += (uint64_t)nt[v] * nf[v]; }
    if (n_base + n_pos >= 0xFFFFFFFFull || closures.size() >= 0xFFFFFFFFull) return fail(DFK_E_ARG, "patch: %llu K-mers on the edges and %llu in the closures: the edge builder indexes K-mers with 32 bits", (unsigned long long)n_base, (unsigned long long)n_pos);
    const unsigned cus = (unsigned)c->prop.multiProcessorCount;
    const uint64_t mark = c->alloc_seq;
    HostGraph& H = R->hb3;
    H.K = K;
    float ms_entries = 0, ms_index = 0, ms_closures = 0, ms_graph = 0, ms_paths = 0;
    double s_sort = 0, s_number = 0, s_copy = wall_now() - t_in;                 // (what the call did before this: the tables unpacked to a byte a base and checked)
    uint64_t n_found = 0, n_bits = 0, n_batches = 0, n_cycle = 0;
    std::vector<dfk_entry32> fresh;
    std::vector<uint64_t> ids_first(nc + 1, 0);
    std::vector<int32_t> ids, left(nc, 0), left_inv(nc, 0);
    auto body = [&]() -> int {
        int rc;
        Timer tm(c->stream);
        // ---- the old edges' bases, the slot table, the crossings' bits: up
        double t0 = wall_now();
        PatchStream es;
        for (uint32_t e : P.canon) es.push(G.edges[e]);
        es.close();
        const std::vector<uint32_t> ends(P.ends.begin(), P.ends.end());
        DevBuf d_words, d_ebase, d_first, d_ends, d_ent, d_rev;
        if ((rc = cn_up(c, d_words, es.words.data(), es.words.size() * 4, "old edges' bases")) || (rc = cn_up(c, d_ebase, es.at.data(), es.at.size() * 8, "old edges' starts")) ||
            (rc = cn_up(c, d_first, P.first.data(), P.first.size() * 8, "slots per old edge")) || (rc = cn_up(c, d_ends, ends.data(), ends.size() * 4, "crossings per old edge")) ||
            (rc = c->alloc(d_ent, std::max<uint64_t>(32, n_base * 32), "dictionary of the old edges", Place::Low)) || (rc = c->alloc(d_rev, (n_base + 63) / 64 * 8 + 8, "orientation of the old edges' K-mers", Place::Low))) return rc;
        s_copy += wall_now() - t0;
        tm.start();
        if (n_base) {
            hipLaunchKernelGGL(HIP_KERNEL_NAME(k_patch_entries<K>), dim3(grid_256(n_base, cus)), dim3(256), 0, c->stream, (const uint32_t*)d_words.p, (const uint64_t*)d_ebase.p, (const uint64_t*)d_first.p,
                               (const uint32_t*)d_ends.p, nc, n_base, (uint4*)d_ent.p, (unsigned long long*)d_rev.p);
            HIP_TRY(hipGetLastError());
        }
        HIP_TRY(hipStreamSynchronize(c->stream));
        ms_entries = tm.stop();
        // ---- the index over them; every entry finds itself, or a K-mer lies on two canonical edges
        PartTable pt{};
        pt.n_parts = n_base ? 1 : 0; pt.start[0] = 0; pt.ptr[0] = (uint4*)d_ent.p; pt.start[pt.n_parts] = n_base;
        const uint64_t slots = std::max<uint64_t>(1024, (2 * n_base + 2 + 1) & ~1ull);
        DevBuf d_index, d_ctr;
        if ((rc = c->alloc(d_index, slots * 4, "K-mer index of the old edges")) || (rc = c->alloc(d_ctr, 64, "patch counters", Place::Low))) return rc;
        tm.start();
        HIP_TRY(hipMemsetAsync(d_ctr.p, 0, 64, c->stream));
        hipLaunchKernelGGL(k_fill_u64, dim3(4096), dim3(256), 0, c->stream, (uint64_t*)d_index.p, slots / 2, ~0ull);
        if (n_base) {
            hipLaunchKernelGGL(HIP_KERNEL_NAME(k_graph_index<K>), dim3(grid_256(n_base, cus)), dim3(256), 0, c->stream, pt, n_base, (uint32_t*)d_index.p, slots);
            hipLaunchKernelGGL(HIP_KERNEL_NAME(k_patch_check<K>), dim3(grid_256(n_base, cus)), dim3(256), 0, c->stream, pt, n_base, (const uint32_t*)d_index.p, slots, (unsigned int*)((uint64_t*)d_ctr.p + 7));
        }
        HIP_TRY(hipGetLastError());
        uint64_t h[8] = {};
        HIP_TRY(hipMemcpyAsync(h, d_ctr.p, 64, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
        ms_index = tm.stop();
        if (h[7]) return fail(DFK_E_ARG, "patch: a K-mer lies on two canonical edges (or twice on one): this is no unipath graph");
        // ---- the closures' K-mers, a batch of positions at a time
        if (n_pos) {
            t0 = wall_now();
            PatchStream cs;
            for (const Seq& s : closures) cs.push(s);
            cs.close();
            DevBuf d_cw, d_cat, d_cfirst, d_list;
            if ((rc = cn_up(c, d_cw, cs.words.data(), cs.words.size() * 4, "closures' bases")) || (rc = cn_up(c, d_cat, cs.at.data(), cs.at.size() * 8, "closures' starts")) ||
                (rc = cn_up(c, d_cfirst, cfirst.data(), cfirst.size() * 8, "positions per closure"))) return rc;
            // 0 = what fits: half of what is free NOW, with the old edges' dictionary and its index resident, at 32 bytes a position.  The batches bound the
            // device list only: the novel K-mers of all batches gather in `fresh` on the host, 32 bytes each, at most one a closure K-mer position.
            const uint64_t room = std::max<uint64_t>(1, c->largest_allocatable() / 64);
            const uint64_t per = std::min(n_pos, per_batch ? per_batch : room);
            if ((rc = c->alloc(d_list, per * 32, "closure K-mers that are not on the old edges", Place::Low))) return rc;
            s_copy += wall_now() - t0;
            for (uint64_t q0 = 0; q0 < n_pos; q0 += per) {
                const uint64_t q1 = std::min(n_pos, q0 + per);
                ++n_batches;
                tm.start();
                HIP_TRY(hipMemsetAsync(d_ctr.p, 0, 8, c->stream));            // word [0] alone: the batch's appended K-mers; [1] found and [2] bits added run on over the batches
                hipLaunchKernelGGL(HIP_KERNEL_NAME(k_patch_closure_kmers<K>), dim3(grid_256(q1 - q0, cus)), dim3(256), 0, c->stream, pt, (const uint32_t*)d_index.p, slots, (const uint32_t*)d_cw.p,
                                   (const uint64_t*)d_cat.p, (const uint64_t*)d_cfirst.p, (uint32_t)closures.size(), q0, q1, (uint4*)d_list.p, (unsigned long long*)d_ctr.p);
                HIP_TRY(hipGetLastError());
                HIP_TRY(hipMemcpyAsync(h, d_ctr.p, 24, hipMemcpyDeviceToHost, c->stream));
                HIP_TRY(hipStreamSynchronize(c->stream));
                ms_closures += tm.stop();
                if (h[0] > q1 - q0) return fail(DFK_E_HIP, "patch: %llu K-mers appended for %llu positions", (unsigned long long)h[0], (unsigned long long)(q1 - q0));
                t0 = wall_now();
                const size_t was = fresh.size();
                fresh.resize(was + h[0]);
                if (h[0]) HIP_TRY(hipMemcpy(fresh.data() + was, d_list.p, h[0] * 32, hipMemcpyDeviceToHost));
                s_copy += wall_now() - t0;
            }
            n_found = h[1]; n_bits = h[2];
            c->release(d_list); c->release(d_cfirst); c->release(d_cat); c->release(d_cw);
        }
        c->release(d_index);
        // ---- the novel K-mers: by key, equal keys' contexts OR-ed (a few million at most: the host; a device sort would need the list whole)
        t0 = wall_now();
        std::sort(fresh.begin(), fresh.end(), [](const dfk_entry32& a, const dfk_entry32& b) { return a.w0 != b.w0 ? a.w0 < b.w0 : a.w1 < b.w1; });
        size_t n2 = 0;
        for (size_t i = 0; i < fresh.size(); ++i) {
            if (n2 && fresh[n2 - 1].w0 == fresh[i].w0 && fresh[n2 - 1].w1 == fresh[i].w1) fresh[n2 - 1].count_ctx |= fresh[i].count_ctx;
            else fresh[n2++] = fresh[i];
        }
        fresh.resize(n2);
        s_sort = wall_now() - t0;
        DevBuf d_part2;
        if (n2) {
            t0 = wall_now();
            if ((rc = c->alloc(d_part2, n2 * 32, "dictionary of the closures' own K-mers", Place::Low))) return rc;
            if ((rc = upload(c, d_part2.p, fresh.data(), n2 * 32))) return rc;
            s_copy += wall_now() - t0;
        }
        // ---- hb3: the graph kernels over the two parts, the numbering on the host
        const uint64_t n = n_base + n2;
        pt.n_parts = 0;
        if (n_base) { pt.start[pt.n_parts] = 0; pt.ptr[pt.n_parts++] = (uint4*)d_ent.p; }
        if (n2) { pt.start[pt.n_parts] = n_base; pt.ptr[pt.n_parts++] = (uint4*)d_part2.p; }
        pt.start[pt.n_parts] = n;
        if (n) { if ((rc = graph_edges_typed<K>(c, pt, n, &H, &ms_graph))) return rc; }
        t0 = wall_now();
        build_hbv(H);
        s_number = wall_now() - t0;
        c->release(H.d_index); H.d_index = DevBuf{};
        // ---- the old edges' paths off the entries
        if (n_base) {
            std::vector<EdgeRec> hrec(H.ce.size());
            HIP_TRY(hipMemcpy(hrec.data(), H.d_recs.p, hrec.size() * sizeof(EdgeRec), hipMemcpyDeviceToHost));
            for (const EdgeRec& r : hrec) if (r.flags & ER_CYCLE) n_cycle += r.n;
            const uint64_t n_blocks = (n_base + 255) / 256;
            DevBuf d_heads, d_cnt, d_blk, d_fwd, d_rv, d_ids, d_idsf, d_left, d_linv;
            t0 = wall_now();
            if ((rc = c->alloc(d_heads, (n_base + 63) / 64 * 8 + 8, "heads", Place::Low)) || (rc = c->alloc(d_cnt, (n_blocks + 1) * 8, "heads per block", Place::Low)) ||
                (rc = c->alloc(d_blk, (n_blocks + 1) * 8, "ids before a block", Place::Low)) || (rc = cn_up(c, d_fwd, H.fwd.data(), H.fwd.size() * 4, "fwdXlat")) ||
                (rc = cn_up(c, d_rv, H.rev.data(), H.rev.size() * 4, "revXlat")) || (rc = c->alloc(d_idsf, (uint64_t)nc * 8 + 8, "ids before an old edge", Place::Low)) ||
                (rc = c->alloc(d_left, (uint64_t)nc * 4 + 8, "left3 of the canonical edges", Place::Low)) || (rc = c->alloc(d_linv, (uint64_t)nc * 4 + 8, "left3 of their inverses", Place::Low))) return rc;
            s_copy += wall_now() - t0;
            tm.start();
            HIP_TRY(hipMemsetAsync((uint64_t*)d_cnt.p + n_blocks, 0, 8, c->stream));
            hipLaunchKernelGGL(HIP_KERNEL_NAME(k_patch_heads<K>), dim3((unsigned)n_blocks), dim3(256), 0, c->stream, pt, n_base, (const uint64_t*)d_first.p, nc, (const unsigned long long*)d_rev.p,
                               (const EdgeRec*)H.d_recs.p, (const uint8_t*)H.d_store.p, (unsigned long long*)d_heads.p, (unsigned long long*)d_cnt.p);
            if ((rc = device_scan(c, (const uint64_t*)d_cnt.p, (uint64_t*)d_blk.p, n_blocks + 1))) return rc;          // (exclusive: word n_blocks is the total)
            HIP_TRY(hipGetLastError());
            uint64_t n_ids = 0;
            HIP_TRY(hipMemcpyAsync(&n_ids, (const uint64_t*)d_blk.p + n_blocks, 8, hipMemcpyDeviceToHost, c->stream));
            HIP_TRY(hipStreamSynchronize(c->stream));
            if (n_ids < nc || n_ids > n_base) return fail(DFK_E_HIP, "patch: %llu heads on %u old edges of %llu K-mers", (unsigned long long)n_ids, nc, (unsigned long long)n_base);
            if ((rc = c->alloc(d_ids, n_ids * 4 + 8, "ids of the canonical edges' paths", Place::Low))) return rc;
            hipLaunchKernelGGL(HIP_KERNEL_NAME(k_patch_emit<K>), dim3((unsigned)n_blocks), dim3(256), 0, c->stream, pt, n_base, (const uint64_t*)d_first.p, nc, (const unsigned long long*)d_rev.p,
                               (const EdgeRec*)H.d_recs.p, (const uint8_t*)H.d_store.p, (const unsigned long long*)d_heads.p, (const unsigned long long*)d_blk.p, (const int32_t*)d_fwd.p,
                               (const int32_t*)d_rv.p, (int32_t*)d_ids.p, (unsigned long long*)d_idsf.p, (int32_t*)d_left.p, (int32_t*)d_linv.p);
            HIP_TRY(hipGetLastError());
            HIP_TRY(hipStreamSynchronize(c->stream));
            ms_paths = tm.stop();
            t0 = wall_now();
            ids.resize(n_ids);
            HIP_TRY(hipMemcpy(ids.data(), d_ids.p, n_ids * 4, hipMemcpyDeviceToHost));
            HIP_TRY(hipMemcpy(ids_first.data(), d_idsf.p, (uint64_t)nc * 8, hipMemcpyDeviceToHost));
            HIP_TRY(hipMemcpy(left.data(), d_left.p, (uint64_t)nc * 4, hipMemcpyDeviceToHost));
            HIP_TRY(hipMemcpy(left_inv.data(), d_linv.p, (uint64_t)nc * 4, hipMemcpyDeviceToHost));
            ids_first[nc] = n_ids;
            s_copy += wall_now() - t0;
        }
        return 0;
    };
    int rc;
    try { rc = body(); } catch (const std::runtime_error& e) { rc = fail(DFK_E_HIP, "%s", e.what()); }
    (void)hipStreamSynchronize(c->stream);
    c->release_since(mark);
    H.d_index = H.d_recs = H.d_store = DevBuf{};
    if (rc) return rc;
    // ---- to3 / left3 for every old edge: a canonical edge's ids as the device left them, its inverse's reversed through hb3's involution
    const double t1 = wall_now();
    const size_t E3 = H.he.size();
    std::vector<int32_t> inv3(E3);
    for (size_t e = 0; e < E3; ++e) inv3[e] = H.he[e].rc ? H.fwd[H.he[e].ce] : H.rev[H.he[e].ce];
    std::vector<uint32_t> place(E, 0);
    for (uint32_t i = 0; i < nc; ++i) { place[P.canon[i]] = i; place[G.inv[P.canon[i]]] = i; }
    R->to3_first.assign(E + 1, 0); R->left3.assign(E, 0);
    for (size_t e = 0; e < E; ++e) {
        const uint32_t i = place[e];
        if (ids_first[i + 1] <= ids_first[i] || ids_first[i + 1] > ids.size()) return fail(DFK_E_HIP, "patch: the ids of old edge %zu are not where the scan put them", e);
        R->to3_first[e + 1] = R->to3_first[e] + (ids_first[i + 1] - ids_first[i]);
    }
    R->to3.resize(R->to3_first[E]);
    uint64_t path_n[3] = {}, n_left = 0;
    for (size_t e = 0; e < E; ++e) {
        const uint32_t i = place[e];
        const uint64_t n_ids = ids_first[i + 1] - ids_first[i];
        int32_t* out = R->to3.data() + R->to3_first[e];
        const int32_t* mine = ids.data() + ids_first[i];
        for (uint64_t j = 0; j < n_ids; ++j) if (mine[j] < 0 || (size_t)mine[j] >= E3) return fail(DFK_E_HIP, "patch: old edge %zu goes over hb3's edge %d of %zu", e, mine[j], E3);
        if ((size_t)P.canon[i] == e) std::copy(mine, mine + n_ids, out);
        else inv_route(mine, n_ids, [&](int32_t id) { return inv3[id]; }, out);                 // (dfk_patch.h: reversed, through hb3's involution)
        R->left3[e] = (size_t)P.canon[i] == e ? left[i] : left_inv[i];
        ++path_n[std::min<uint64_t>(n_ids, 3) - 1]; n_left += R->left3[e] != 0;
    }
    uint64_t sum = 0, xr = 0;
    digest(R->to3_first, R->to3, R->left3, &sum, &xr);
    s_copy += wall_now() - t1;
    uint64_t* s = R->stats;
    s[DFK_PATCH_EDGES] = E; s[DFK_PATCH_CANONICAL] = nc; s[DFK_PATCH_VERTICES] = G.n_vertices; s[DFK_PATCH_CROSSINGS] = crossings; s[DFK_PATCH_CLOSURES] = closures.size(); s[DFK_PATCH_SHORT] = n_short;
    s[DFK_PATCH_POSITIONS] = n_pos; s[DFK_PATCH_FOUND] = n_found; s[DFK_PATCH_NEW] = n_pos - n_found; s[DFK_PATCH_NEW_UNIQUE] = fresh.size(); s[DFK_PATCH_BITS_ADDED] = n_bits;
    s[DFK_PATCH_KMERS3] = n_base + fresh.size(); s[DFK_PATCH_CANONICAL3] = H.ce.size(); s[DFK_PATCH_VERTICES3] = H.n_vertices; s[DFK_PATCH_EDGES3] = E3;
    for (const GraphEdge& g : H.ce) s[DFK_PATCH_SINGLE3] += g.n == 1;
    s[DFK_PATCH_CYCLE_KMERS] = n_cycle; s[DFK_PATCH_PATH1] = path_n[0]; s[DFK_PATCH_PATH2] = path_n[1]; s[DFK_PATCH_PATH3] = path_n[2]; s[DFK_PATCH_TO3] = R->to3.size(); s[DFK_PATCH_LEFT3] = n_left;
    s[DFK_PATCH_BATCHES] = n_batches; s[DFK_PATCH_US] = (uint64_t)(1e6 * (wall_now() - t_in)); s[DFK_PATCH_US_ENTRIES] = (uint64_t)(1000.0f * ms_entries); s[DFK_PATCH_US_INDEX] = (uint64_t)(1000.0f * ms_index);
    s[DFK_PATCH_US_CLOSURES] = (uint64_t)(1000.0f * ms_closures); s[DFK_PATCH_US_SORT] = (uint64_t)(1e6 * s_sort); s[DFK_PATCH_US_GRAPH] = (uint64_t)(1000.0f * ms_graph);
    s[DFK_PATCH_US_NUMBER] = (uint64_t)(1e6 * s_number); s[DFK_PATCH_US_PATHS] = (uint64_t)(1000.0f * ms_paths); s[DFK_PATCH_US_COPY] = (uint64_t)(1e6 * s_copy); s[DFK_PATCH_SUM] = sum; s[DFK_PATCH_XOR] = xr;
    TRACE("patch: %zu old edges (%u canonical, %llu K-mers), %zu closures with %llu K-mers: %llu found, %llu new (%zu distinct), %llu bits added; hb3: %zu canonical edges, %llu vertices, %zu edges; %zu ids, %llu batch(es); "
          "entries %.1f ms, index %.1f ms, closures %.1f ms, sort %.1f ms, graph %.1f ms, numbering %.1f ms, paths %.1f ms, copies %.1f ms",
          E, nc, (unsigned long long)n_base, closures.size(), (unsigned long long)n_pos, (unsigned long long)n_found, (unsigned long long)(n_pos - n_found), fresh.size(), (unsigned long long)n_bits, H.ce.size(),
          (unsigned long long)H.n_vertices, E3, R->to3.size(), (unsigned long long)n_batches, ms_entries, ms_index, ms_closures, 1e3 * s_sort, ms_graph, 1e3 * s_number, ms_paths, 1e3 * s_copy);
    return 0;
}

// t_in: when the extern "C" call began (DFK_PATCH_US is the whole call's, the unpacking of its tables included)
int patch_build(dfk_ctx* c, const dfk_patch::Graph& G, const std::vector<dfk_patch::Seq>& closures, uint64_t per_batch, const double t_in, PatchResult* R)
{
    const std::string why = dfk_patch::check_graph(G);
    if (!why.empty()) return fail(DFK_E_ARG, "patch: %s", why.c_str());
    for (const dfk_patch::Seq& s : closures) for (uint8_t b : s) if (b > 3) return fail(DFK_E_ARG, "patch: a closure has a base above 3");
    HIP_TRY(hipSetDevice(c->device));
    switch (G.K) {
    case 40: return patch_build_typed<40>(c, G, closures, per_batch, t_in, R);
    case 48: return patch_build_typed<48>(c, G, closures, per_batch, t_in, R);
    case 60: return patch_build_typed<60>(c, G, closures, per_batch, t_in, R);
    }
    return fail(DFK_E_ARG, "patch: K = %u (40, 48 or 60)", G.K);
}

int patch_write(const PatchResult* R, const std::string& dir)
{
    try { write_graph_files(R->hb3, dir, "a.patch."); }
    catch (const std::runtime_error& e) { return fail(DFK_E_ARG, "%s", e.what()); }
    const std::string path = dir + "/a.patch.to3";
    const std::vector<uint8_t> f = dfk_patch::to3_file(R->to3_first, R->to3, R->left3);
    const int fd = open(path.c_str(), O_WRONLY | O_CREAT | O_TRUNC, 0666);
    if (fd < 0) return fail(DFK_E_ARG, "cannot open %s", path.c_str());
    bool bad = pwrite_all(fd, f.data(), f.size(), 0) != 0;
    if (close(fd) != 0) bad = true;
    if (bad) { (void)unlink(path.c_str()); return fail(DFK_E_ARG, "short write to %s", path.c_str()); }
    return 0;
}

int patch_result_of(dfk_ctx* c, PatchResult** out)
{
    if (!c) return fail(DFK_E_ARG, "null context");
    if (!c->graph_state || !graph_of(c)->patch) return fail(DFK_E_STATE, "no patched graph: call dfk_patch_build or dfk_patch_build_arrays");
    *out = graph_of(c)->patch;
    return 0;
}
void patch_keep(dfk_ctx* c, PatchResult* R)
{
    HostGraph* G = graph_of(c);
    if (G->patch) patch_result_free(G->patch);
    G->patch = R; G->patch_free = patch_result_free;
}

} // namespace

extern "C" {

int dfk_patch_build(dfk_ctx* c, uint64_t kmers_per_batch)
{
    return guarded([&]() -> int {
    const double t_in = wall_now();
    if (!c) return fail(DFK_E_ARG, "null context");
    if (!c->graph_state || !graph_of(c)->built) return fail(DFK_E_STATE, "no graph: call dfk_graph_build");
    const HostGraph* G = graph_of(c);
    // (dfk_allclosures_write's test: both closers' closures, made by the chain for the same pairs)
    if (!G->sclosures || !G->sclosures->from_chain) return fail(DFK_E_STATE, "no stack closures of this context's walks: call dfk_sclosures_build");
    if (!G->closures) return fail(DFK_E_STATE, "no closures of the first closer: call dfk_closures_build");
    const SclosuresResult* A = G->sclosures;
    const ClosuresResult* B = G->closures;
    if (B->pairs.empty() && B->pair_first.size() > 1) return fail(DFK_E_STATE, "the first closer's closures came from dfk_closures_build_arrays: call dfk_closures_build");
    if (A->pairs != B->pairs || A->pair_first.size() != B->pair_first.size()) return fail(DFK_E_STATE, "the two closers' closures were not made for the same pairs: build both chains for one set of pairs");
    dfk_patch::Graph X;
    X.K = G->K; X.n_vertices = (uint32_t)G->n_vertices;
    const size_t E = G->he.size();
    X.edges.resize(E); X.inv.resize(E); X.to_left.resize(E); X.to_right.resize(E);
    for (size_t e = 0; e < E; ++e) {
        const HostGraph::HEdge& h = G->he[e];
        const SeqView v{G->bases.data() + G->ce[h.ce].byte_off, G->ce[h.ce].n + G->K - 1, h.rc != 0};
        X.edges[e].resize(v.L);
        for (uint32_t i = 0; i < v.L; ++i) X.edges[e][i] = (uint8_t)v[i];
        X.inv[e] = h.rc ? G->fwd[h.ce] : G->rev[h.ce]; X.to_left[e] = h.v; X.to_right[e] = h.w;
    }
    std::vector<dfk_patch::Seq> closures;                                                   // the combined list's order (allclosures_write)
    for (uint64_t pi = 0; pi + 1 < A->pair_first.size(); ++pi) {
        for (uint64_t k = A->pair_first[pi]; k < A->pair_first[pi + 1]; ++k) closures.emplace_back(A->bases.begin() + A->starts[k], A->bases.begin() + A->starts[k + 1]);
        for (uint64_t k = B->pair_first[pi]; k < B->pair_first[pi + 1]; ++k) closures.emplace_back(B->bases.begin() + B->starts[k], B->bases.begin() + B->starts[k + 1]);
    }
    std::unique_ptr<PatchResult> R(new PatchResult);
    if (int rc = patch_build(c, X, closures, kmers_per_batch, t_in, R.get())) return rc;          // (refused: the earlier result is still served)
    R->from_chain = true; R->pairs = A->pairs;
    patch_keep(c, R.release());
    return 0;
    });
}

int dfk_patch_build_arrays(dfk_ctx* c, uint64_t n_edges, uint64_t n_vertices, const int32_t* inv, const int32_t* to_left, const int32_t* to_right, const uint8_t* packed, const uint64_t* edge_off,
                           const uint32_t* edge_len, uint64_t n_closures, const uint64_t* closure_starts, const uint8_t* closure_bases, uint64_t kmers_per_batch)
{
    return guarded([&]() -> int {
    const double t_in = wall_now();
    if (!c) return fail(DFK_E_ARG, "null context");
    if ((n_edges && (!inv || !to_left || !to_right || !packed || !edge_off || !edge_len)) || !closure_starts) return fail(DFK_E_ARG, "null argument");
    if (n_edges >= (1ull << 31) || n_vertices >= (1ull << 31) || n_closures >= (1ull << 31)) return fail(DFK_E_ARG, "patch: %llu edges, %llu vertices, %llu closures: 2^31 - 1 at most", (unsigned long long)n_edges, (unsigned long long)n_vertices, (unsigned long long)n_closures);
    if (closure_starts[0] != 0) return fail(DFK_E_ARG, "patch: the closures' starts do not begin at 0");
    for (uint64_t i = 0; i < n_closures; ++i) if (closure_starts[i + 1] < closure_starts[i]) return fail(DFK_E_ARG, "patch: the closures' starts fall at closure %llu", (unsigned long long)i);
    if (closure_starts[n_closures] && !closure_bases) return fail(DFK_E_ARG, "null argument");
    dfk_patch::Graph X;
    X.K = (uint32_t)c->cfg.K; X.n_vertices = (uint32_t)n_vertices;
    X.inv.assign(inv, inv + n_edges); X.to_left.assign(to_left, to_left + n_edges); X.to_right.assign(to_right, to_right + n_edges);
    X.edges.resize(n_edges);
    for (uint64_t e = 0; e < n_edges; ++e) {
        X.edges[e].resize(edge_len[e]);
        const uint8_t* p = packed + edge_off[e];
        for (uint32_t i = 0; i < edge_len[e]; ++i) X.edges[e][i] = (uint8_t)base_at(p, i);
    }
    std::vector<dfk_patch::Seq> closures(n_closures);
    for (uint64_t i = 0; i < n_closures; ++i) closures[i].assign(closure_bases + closure_starts[i], closure_bases + closure_starts[i + 1]);
    std::unique_ptr<PatchResult> R(new PatchResult);
    if (int rc = patch_build(c, X, closures, kmers_per_batch, t_in, R.get())) return rc;
    (void)graph_of(c);
    patch_keep(c, R.release());
    return 0;
    });
}

int dfk_patch_stats(dfk_ctx* c, uint64_t* out)
{
    return guarded([&]() -> int {
    PatchResult* R = nullptr;
    if (int rc = patch_result_of(c, &R)) return rc;
    if (!out) return fail(DFK_E_ARG, "null argument");
    for (int i = 0; i < DFK_PATCH_WORDS; ++i) out[i] = R->stats[i];
    return 0;
    });
}

int dfk_patch_fetch(dfk_ctx* c, uint64_t* n_edges, uint64_t* n_to3, uint64_t* n_edges3, uint64_t* to3_first, int32_t* to3, int32_t* left3, int32_t* kmers3, int32_t* inv3, int32_t* to_left3, int32_t* to_right3)
{
    return guarded([&]() -> int {
    PatchResult* R = nullptr;
    if (int rc = patch_result_of(c, &R)) return rc;
    const HostGraph& H = R->hb3;
    const size_t E = R->left3.size(), E3 = H.he.size();
    if (n_edges) *n_edges = E;
    if (n_to3) *n_to3 = R->to3.size();
    if (n_edges3) *n_edges3 = E3;
    if (to3_first) memcpy(to3_first, R->to3_first.data(), 8 * (E + 1));                      // room for n_edges + 1 words
    if (to3 && !R->to3.empty()) memcpy(to3, R->to3.data(), 4 * R->to3.size());
    if (left3 && E) memcpy(left3, R->left3.data(), 4 * E);
    for (size_t e = 0; e < E3; ++e) {                                                       // room for n_edges3 words each
        if (kmers3) kmers3[e] = (int32_t)H.ce[H.he[e].ce].n;
        if (inv3) inv3[e] = H.he[e].rc ? H.fwd[H.he[e].ce] : H.rev[H.he[e].ce];
        if (to_left3) to_left3[e] = H.he[e].v;
        if (to_right3) to_right3[e] = H.he[e].w;
    }
    return 0;
    });
}

int dfk_patch_write(dfk_ctx* c, const char* dir)
{
    return guarded([&]() -> int {
    PatchResult* R = nullptr;
    if (int rc = patch_result_of(c, &R)) return rc;
    if (!dir) return fail(DFK_E_ARG, "null directory");
    return patch_write(R, dir);
    });
}

} // extern "C"
