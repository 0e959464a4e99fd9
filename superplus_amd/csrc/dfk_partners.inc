// superplus_amd/csrc/dfk_partners.inc -- CloseGap2's search for unplaced partners (10X/Closomatic.cc:554-585) and the file
// a.close.partners, included by dfk.hip.
//
// The rule, the plan and the file's layout: dfk_partners.h.  The kernels: dfk_partners_kernels.h.  Here: partners_build() -- the
// forward parts, the queries a range of sides at a time, then a range of ranks at a time the table and under it the batches of
// the queries whose other edge lies in the range, the bases of each batch's reads gathered on the host and sent up, the kept
// records coming back -- and partners_write().  Everything on the device comes from the arena and goes back before build returns.
//
// The edges' bases: the graph keeps the CANONICAL edges' bases on the device (HostGraph::d_store) only as long as the pather's
// look-up lives, and hb.O(g) of a reverse edge is not in it at all.  So the bases of the edges the anchors name are packed again
// from what the context holds on the host (packed_edge, as a.fastb is written) and uploaded: a few bytes per anchor edge.
#include "dfk_partners_kernels.h"

#include <unordered_map>

namespace {

struct PartnersResult {
    std::vector<uint64_t> starts;                 // [2 * n_pairs + 1]
    std::vector<uint64_t> recs;                   // two words a record: id, pos | 1 << 32
    std::vector<int32_t> pairs;                   // the pairs it was made for (dfk_cons_build takes no others)
    uint64_t stats[DFK_PARTNERS_WORDS] = {};
};
void partners_result_free(PartnersResult* r) { delete r; }

// the reads as the caller holds them; off == NULL: dense, found from block sums of the lengths
struct PartnerReads {
    const uint8_t* packed; const uint64_t* off; const uint32_t* len; uint64_t n;
    std::vector<uint64_t> block_at;               // dense: where read 1024 b starts
    static constexpr uint64_t BLOCK = 1024;
    void index_dense()
    {
        block_at.assign(n / BLOCK + 1, 0);
        uint64_t at = 0;
        for (uint64_t r = 0; r < n; ++r) { if (r % BLOCK == 0) block_at[r / BLOCK] = at; at += ((uint64_t)len[r] + 3) / 4; }
    }
    uint64_t at(uint64_t r) const
    {
        if (off) { uint64_t x; memcpy(&x, (const char*)off + 8 * r, 8); return x; }           // (the table may sit at any address)
        uint64_t x = block_at[r / BLOCK];
        for (uint64_t i = r / BLOCK * BLOCK; i < r; ++i) x += ((uint64_t)len[i] + 3) / 4;
        return x;
    }
};
// the offset table of the kind dfk_paths_verify refuses: not monotone, or a read given fewer bytes than its bases need
int partner_reads_check(const PartnerReads& R)
{
    if (!R.off) return 0;
    uint64_t prev = R.n ? R.at(0) : 0;
    for (uint64_t r = 0; r < R.n; ++r) {
        const uint64_t next = R.at(r + 1);
        if (next < prev || next - prev < ((uint64_t)R.len[r] + 3) / 4)
            return fail(DFK_E_INPUT, "partners: the reads' offset table is not monotone, or leaves a read fewer bytes than its bases need");
        prev = next;
    }
    return 0;
}

struct PartnersSource {
    uint64_t n_edges; const int32_t* inv;
    const uint8_t* store; uint64_t store_bytes;   // the packed bases of the anchors' edges
    const uint64_t* edge_at; const uint32_t* edge_len;   // per ANCHOR: where its edge starts in the store, its bases
    uint64_t n_ce; const uint64_t* ce; const uint64_t* loc_first; const uint64_t* locs; const uint64_t* anchor_first; const int32_t* anchors;
    const PartnerReads* reads;
};

int partners_build(dfk_ctx* c, const PartnersSource& S, const int32_t* pairs, uint64_t n_pairs, uint64_t queries_per_batch, PartnersResult* R)
{
    using namespace dfk_partners;
    const uint64_t N = S.reads->n, n_ce = S.n_ce, n_sides = 2 * n_pairs, n_locs = S.loc_first[n_ce], n_anchors = S.anchor_first[n_ce];
    if (N % 2) return fail(DFK_E_ARG, "%llu reads: the closers take a read's mate as id ^ 1", (unsigned long long)N);
    if (N > (1ull << 31) || n_pairs >= (1ull << 30)) return fail(DFK_E_ARG, "%llu reads, %llu pairs: a query keeps its read and its side in 32 bits each", (unsigned long long)N, (unsigned long long)n_pairs);
    for (uint64_t i = 0; i < 2 * n_pairs; ++i)
        if (pairs[i] < 0 || (uint64_t)pairs[i] >= S.n_edges) return fail(DFK_E_ARG, "pair %llu names edge %d: the graph has %llu", (unsigned long long)(i / 2), pairs[i], (unsigned long long)S.n_edges);
    std::vector<uint32_t> side_rank(std::max<uint64_t>(1, n_sides), 0);
    for (uint64_t pi = 0; pi < n_pairs; ++pi) {
        const uint64_t es[2] = {(uint64_t)pairs[2 * pi], (uint64_t)S.inv[pairs[2 * pi + 1]]};
        for (int ei = 0; ei < 2; ++ei) {
            const uint64_t k = rank_in(S.ce, n_ce, es[ei]);
            if (k == n_ce) return fail(DFK_E_ARG, "pair %llu: edge %llu is not among the closer edges: the closer sets were built for other pairs", (unsigned long long)pi, (unsigned long long)es[ei]);
            side_rank[2 * pi + ei] = (uint32_t)k;
        }
    }
    const unsigned cus = (unsigned)c->prop.multiProcessorCount;
    const double t_in = wall_now();
    const uint64_t mark = c->alloc_seq;
    float ms_table = 0, ms_queries = 0, ms_search = 0;
    double s_copy = 0;
    uint64_t n_batches = 0, n_ranges = 0, n_positions = 0, n_searched = 0, h_ctr[2] = {}, h_dg[4] = {};
    std::vector<uint32_t> q_side, q_id;                                        // the queries, in push order
    std::vector<uint8_t> q_kept; std::vector<int32_t> q_pos;
    std::vector<uint64_t> tfirst;
    auto body = [&]() -> int {
        int rc;
        Timer tm(c->stream);
        DevBuf d_loc_first, d_locs, d_side_rank, d_fw, d_store, ctr;
        auto up = [&](DevBuf& d, const void* h, uint64_t bytes, const char* what) -> int {
            if (int r = c->alloc(d, std::max<uint64_t>(8, bytes), what, Place::Low)) return r;
            return bytes ? upload(c, d.p, h, bytes) : 0;
        };
        // ---- the forward part of every rank
        tm.start();
        if ((rc = up(d_loc_first, S.loc_first, (n_ce + 1) * 8, "locs starts")) || (rc = up(d_locs, S.locs, n_locs * 16, "locs records")) ||
            (rc = up(d_side_rank, side_rank.data(), n_sides * 4, "ranks of the sides")) || (rc = up(d_store, S.store, S.store_bytes, "anchor edges' bases")) ||
            (rc = c->alloc(d_fw, std::max<uint64_t>(1, n_ce) * 8, "forward records per rank", Place::Low)) || (rc = c->alloc(ctr, 16, "partners counters", Place::Low))) return rc;
        HIP_TRY(hipMemsetAsync(ctr.p, 0, 16, c->stream));
        std::vector<uint64_t> fw_n(n_ce, 0);
        if (n_ce) {
            hipLaunchKernelGGL(k_pt_forward, dim3(grid_256(n_ce, cus)), dim3(256), 0, c->stream, (const uint64_t*)d_loc_first.p, (const uint64_t*)d_locs.p, n_ce, (uint64_t*)d_fw.p);
            HIP_TRY(hipGetLastError());
            HIP_TRY(hipMemcpyAsync(fw_n.data(), d_fw.p, n_ce * 8, hipMemcpyDeviceToHost, c->stream));
        }
        HIP_TRY(hipStreamSynchronize(c->stream));
        for (uint64_t k = 0; k < n_ce; ++k)
            if (fw_n[k] > S.loc_first[k + 1] - S.loc_first[k]) return fail(DFK_E_HIP, "partners: rank %llu has %llu forward records of %llu", (unsigned long long)k, (unsigned long long)fw_n[k], (unsigned long long)(S.loc_first[k + 1] - S.loc_first[k]));
        // ---- the queries, a range of sides at a time
        const uint64_t forced = path_switches().pidx_range_pairs;
        std::vector<uint64_t> side_items(n_sides);
        for (uint64_t q = 0; q < n_sides; ++q) side_items[q] = fw_n[side_rank[q]];
        const std::vector<uint64_t> ifirst = prefix_sums(side_items.data(), n_sides);
        for (uint64_t q0 = 0; q0 < n_sides;) {
            const PidxRange range = next_range(ifirst.data(), n_sides, q0, item_cap(c->largest_allocatable(), forced));
            const uint64_t q1 = range.e1, ns = q1 - q0, n_items = range.n;
            if (n_items) {
                const uint64_t rmark = c->alloc_seq;
                std::vector<uint64_t> rel(ns + 1);
                for (uint64_t s = 0; s <= ns; ++s) rel[s] = ifirst[q0 + s] - ifirst[q0];
                DevBuf d_rel, flags, place, d_qs, d_qi;
                if ((rc = up(d_rel, rel.data(), (ns + 1) * 8, "items per side")) || (rc = c->alloc(flags, (n_items + 1) * 8, "query flags", Place::Low)) ||
                    (rc = c->alloc(place, (n_items + 1) * 8, "query places", Place::Low))) return rc;
                const PtSides P{(const uint32_t*)d_side_rank.p, (const uint64_t*)d_rel.p, (const uint64_t*)d_loc_first.p, (const uint64_t*)d_locs.p, (const uint64_t*)d_fw.p, q0, ns, n_items};
                hipLaunchKernelGGL(k_pt_flag, dim3(grid_256(n_items + 1, cus)), dim3(256), 0, c->stream, P, (uint64_t*)flags.p);
                HIP_TRY(hipGetLastError());
                if ((rc = device_scan(c, (const uint64_t*)flags.p, (uint64_t*)place.p, n_items + 1))) return rc;
                uint64_t got = 0;
                HIP_TRY(hipMemcpyAsync(&got, (const uint64_t*)place.p + n_items, 8, hipMemcpyDeviceToHost, c->stream));
                HIP_TRY(hipStreamSynchronize(c->stream));
                if (got > n_items) return fail(DFK_E_HIP, "partners: %llu queries among %llu items", (unsigned long long)got, (unsigned long long)n_items);
                if (got) {
                    if ((rc = c->alloc(d_qs, got * 4, "query sides", Place::Low)) || (rc = c->alloc(d_qi, got * 4, "query reads", Place::Low))) return rc;
                    hipLaunchKernelGGL(k_pt_emit, dim3(grid_256(n_items, cus)), dim3(256), 0, c->stream, P, (const uint64_t*)flags.p, (const uint64_t*)place.p, (uint32_t*)d_qs.p, (uint32_t*)d_qi.p);
                    HIP_TRY(hipGetLastError());
                    const uint64_t at = q_side.size();
                    q_side.resize(at + got); q_id.resize(at + got);
                    HIP_TRY(hipMemcpyAsync(q_side.data() + at, d_qs.p, got * 4, hipMemcpyDeviceToHost, c->stream));
                    HIP_TRY(hipMemcpyAsync(q_id.data() + at, d_qi.p, got * 4, hipMemcpyDeviceToHost, c->stream));
                    HIP_TRY(hipStreamSynchronize(c->stream));
                }
                c->release_since(rmark);
            }
            q0 = q1;
        }
        ms_queries = tm.stop();
        const uint64_t n_q = q_side.size();
        for (uint64_t i = 0; i < n_q; ++i)
            if (q_side[i] >= n_sides || q_id[i] >= N) return fail(DFK_E_HIP, "partners: query %llu names side %u, read %u", (unsigned long long)i, q_side[i], q_id[i]);
        q_kept.assign(n_q, 0); q_pos.assign(n_q, 0);
        // ---- the table a range of ranks at a time; under each the batches of the queries whose other edge lies in it
        std::vector<uint64_t> ent_n(n_ce, 0), a_first(n_anchors + 1, 0);
        for (uint64_t k = 0; k < n_ce; ++k)
            for (uint64_t a = S.anchor_first[k]; a < S.anchor_first[k + 1]; ++a) { const uint64_t n = positions(S.edge_len[a]); ent_n[k] += n; a_first[a + 1] = a_first[a] + n; }
        tfirst = prefix_sums(ent_n.data(), n_ce);
        for (uint64_t k0 = 0; k0 < n_ce;) {
            const PidxRange range = next_range(tfirst.data(), n_ce, k0, range_cap(c->largest_allocatable(), forced));
            const uint64_t k1 = range.e1, nk = k1 - k0, n_t = range.n, a0 = S.anchor_first[k0], a1 = S.anchor_first[k1], n_a = a1 - a0;
            if (!range.ok) return fail(DFK_E_ARG, "edge %llu alone has %llu anchor 32-mers: a range of the table sorts 32-bit places", (unsigned long long)S.ce[k0], (unsigned long long)range.n);
            ++n_ranges;
            const uint64_t rmark = c->alloc_seq;
            tm.start();
            DevBuf keys, spos, d_tfirst;
            std::vector<uint64_t> trel(nk + 1);
            for (uint64_t k = 0; k <= nk; ++k) trel[k] = tfirst[k0 + k] - tfirst[k0];
            if ((rc = c->alloc(keys, (n_t + 1) * 8, "anchor 32-mers, sorted", Place::Low)) || (rc = c->alloc(spos, (n_t + 1) * 4, "their positions", Place::Low)) ||
                (rc = up(d_tfirst, trel.data(), (nk + 1) * 8, "table starts per rank"))) return rc;
            if (n_t) {
                const uint64_t smark = c->alloc_seq;
                std::vector<uint64_t> erel(n_a + 1), eat(n_a);
                std::vector<int32_t> add(n_a); std::vector<uint32_t> rk(n_a);
                for (uint64_t a = 0; a <= n_a; ++a) erel[a] = a_first[a0 + a] - a_first[a0];
                for (uint64_t k = k0; k < k1; ++k)
                    for (uint64_t a = S.anchor_first[k]; a < S.anchor_first[k + 1]; ++a) { eat[a - a0] = S.edge_at[a]; add[a - a0] = S.anchors[3 * a + 1]; rk[a - a0] = (uint32_t)(k - k0); }
                DevBuf d_erel, d_eat, d_add, d_rk, klo, khi, krank, kpos, k[2], v[2];
                auto u32s = [&](DevBuf& d, const char* what) { return c->alloc(d, n_t * 4, what, Place::Low); };
                if ((rc = up(d_erel, erel.data(), (n_a + 1) * 8, "entries per anchor")) || (rc = up(d_eat, eat.data(), n_a * 8, "anchor edges")) || (rc = up(d_add, add.data(), n_a * 4, "anchor distances")) ||
                    (rc = up(d_rk, rk.data(), n_a * 4, "anchor ranks")) || (rc = u32s(klo, "32-mers, low words")) || (rc = u32s(khi, "32-mers, high words")) || (rc = u32s(krank, "entry ranks")) ||
                    (rc = u32s(kpos, "entry positions")) || (rc = u32s(k[0], "sort keys")) || (rc = u32s(k[1], "sort keys")) || (rc = u32s(v[0], "sort places")) || (rc = u32s(v[1], "sort places"))) return rc;
                const PtAnchors A{(const uint64_t*)d_erel.p, (const uint64_t*)d_eat.p, (const int32_t*)d_add.p, (const uint32_t*)d_rk.p, n_a, n_t};
                const unsigned g = grid_256(n_t, cus);
                hipLaunchKernelGGL(k_pt_entries, dim3(g), dim3(256), 0, c->stream, A, (const uint8_t*)d_store.p, (uint32_t*)klo.p, (uint32_t*)khi.p, (uint32_t*)krank.p, (int32_t*)kpos.p);
                // sorted by (rank, 32-mer): the permutation by the key's low word, its high word, the rank -- least significant first, every sort stable
                int cur = 0;
                HIP_TRY(hipMemcpyAsync(k[0].p, klo.p, n_t * 4, hipMemcpyDeviceToDevice, c->stream));
                hipLaunchKernelGGL(k_cl_iota, dim3(g), dim3(256), 0, c->stream, (uint32_t*)v[0].p, n_t);
                HIP_TRY(hipGetLastError());
                if ((rc = radix_sort_pairs(c, k, v, n_t, 32, &cur))) return rc;
                hipLaunchKernelGGL(k_cl_gather, dim3(g), dim3(256), 0, c->stream, (const uint32_t*)khi.p, (const uint32_t*)v[cur].p, n_t, (uint32_t*)k[cur].p);
                HIP_TRY(hipGetLastError());
                if ((rc = radix_sort_pairs(c, k, v, n_t, 32, &cur))) return rc;
                if (nk > 1) {
                    hipLaunchKernelGGL(k_cl_gather, dim3(g), dim3(256), 0, c->stream, (const uint32_t*)krank.p, (const uint32_t*)v[cur].p, n_t, (uint32_t*)k[cur].p);
                    HIP_TRY(hipGetLastError());
                    if ((rc = radix_sort_pairs(c, k, v, n_t, bits_for(nk), &cur))) return rc;
                }
                hipLaunchKernelGGL(k_pt_sorted, dim3(g), dim3(256), 0, c->stream, (const uint32_t*)v[cur].p, (const uint32_t*)klo.p, (const uint32_t*)khi.p, (const int32_t*)kpos.p, n_t, (uint64_t*)keys.p, (int32_t*)spos.p);
                HIP_TRY(hipGetLastError());
                HIP_TRY(hipStreamSynchronize(c->stream));
                c->release_since(smark);
            }
            ms_table += tm.stop();
            // the queries of this range, in query order, and what each costs a batch
            std::vector<uint64_t> sel;
            for (uint64_t i = 0; i < n_q; ++i) {                                  // (a query against an empty slice finds nothing: it is counted and stays here)
                const uint64_t ko = side_rank[q_side[i] ^ 1u];
                if (ko < k0 || ko >= k1) continue;
                if (tfirst[ko + 1] == tfirst[ko]) n_positions += positions(S.reads->len[q_id[i]]); else sel.push_back(i);
            }
            n_searched += sel.size();
            std::vector<uint64_t> cost(sel.size());
            for (size_t i = 0; i < sel.size(); ++i) cost[i] = query_cost(S.reads->len[q_id[sel[i]]]);
            const std::vector<uint64_t> cfirst = prefix_sums(cost.data(), cost.size());
            for (uint64_t b0 = 0; b0 < sel.size();) {
                const uint64_t b1 = next_batch(cfirst.data(), sel.size(), b0, batch_room(c->largest_allocatable()), queries_per_batch), nb = b1 - b0;
                ++n_batches;
                const uint64_t bmark = c->alloc_seq;
                // the gather: the batch's reads one behind the other, the last ending where the block ends
                const double t_g = wall_now();
                std::vector<uint64_t> off(nb); std::vector<uint32_t> len(nb), side(nb);
                uint64_t bytes = 0;
                for (uint64_t i = 0; i < nb; ++i) { const uint32_t id2 = q_id[sel[b0 + i]]; off[i] = bytes; len[i] = S.reads->len[id2]; side[i] = q_side[sel[b0 + i]]; bytes += ((uint64_t)len[i] + 3) / 4; n_positions += positions(len[i]); }
                std::vector<uint8_t> bases(bytes);
                for (uint64_t i = 0; i < nb; ++i)
                    if (const uint64_t n = ((uint64_t)len[i] + 3) / 4) if ((rc = host_read(c, bases.data() + off[i], S.reads->packed + S.reads->at(q_id[sel[b0 + i]]), n))) return rc;
                DevBuf d_bases, d_off, d_len, d_side, status, found, kept, place, out;
                if ((rc = up(d_bases, bases.data(), bytes, "partner reads' bases")) || (rc = up(d_off, off.data(), nb * 8, "partner reads' starts")) || (rc = up(d_len, len.data(), nb * 4, "partner reads' lengths")) ||
                    (rc = up(d_side, side.data(), nb * 4, "query sides")) || (rc = c->alloc(status, nb * 4, "query status", Place::Low)) || (rc = c->alloc(found, nb * 4, "query positions", Place::Low)) ||
                    (rc = c->alloc(kept, (nb + 1) * 8, "queries kept", Place::Low)) || (rc = c->alloc(place, (nb + 1) * 8, "their places", Place::Low))) return rc;
                s_copy += wall_now() - t_g;
                tm.start();
                const PtBatch B{(const uint8_t*)d_bases.p, (const uint64_t*)d_off.p, (const uint32_t*)d_len.p, (const uint32_t*)d_side.p, nb, (const uint32_t*)d_side_rank.p, (uint32_t)k0, (uint32_t)k1,
                                (const uint64_t*)d_tfirst.p, (const uint64_t*)keys.p, (const int32_t*)spos.p};
                hipLaunchKernelGGL(k_pt_search, dim3((unsigned)std::min<uint64_t>((nb + 4) / 4, 16ull * cus)), dim3(256), 0, c->stream, B, (uint32_t*)status.p, (int32_t*)found.p, (uint64_t*)kept.p, (unsigned long long*)ctr.p);
                HIP_TRY(hipGetLastError());
                if ((rc = device_scan(c, (const uint64_t*)kept.p, (uint64_t*)place.p, nb + 1))) return rc;
                uint64_t n_kept = 0;
                HIP_TRY(hipMemcpyAsync(&n_kept, (const uint64_t*)place.p + nb, 8, hipMemcpyDeviceToHost, c->stream));
                HIP_TRY(hipStreamSynchronize(c->stream));
                if (n_kept > nb) return fail(DFK_E_HIP, "partners: %llu kept among %llu queries", (unsigned long long)n_kept, (unsigned long long)nb);
                std::vector<uint32_t> h_out(2 * n_kept);
                if (n_kept) {
                    if ((rc = c->alloc(out, n_kept * 8, "a.close.partners records", Place::Low))) return rc;
                    hipLaunchKernelGGL(k_pt_compact, dim3(grid_256(nb, cus)), dim3(256), 0, c->stream, (const uint64_t*)kept.p, (const uint64_t*)place.p, (const int32_t*)found.p, nb, (uint32_t*)out.p);
                    HIP_TRY(hipGetLastError());
                }
                ms_search += tm.stop();
                const double t_d = wall_now();
                if (n_kept) {
                    HIP_TRY(hipMemcpyAsync(h_out.data(), out.p, n_kept * 8, hipMemcpyDeviceToHost, c->stream));
                    HIP_TRY(hipStreamSynchronize(c->stream));
                }
                for (uint64_t i = 0; i < n_kept; ++i) {
                    if (h_out[2 * i] >= nb) return fail(DFK_E_HIP, "partners: a kept record names query %u of %llu", h_out[2 * i], (unsigned long long)nb);
                    q_kept[sel[b0 + h_out[2 * i]]] = 1; q_pos[sel[b0 + h_out[2 * i]]] = (int32_t)h_out[2 * i + 1];
                }
                s_copy += wall_now() - t_d;
                c->release_since(bmark);
                b0 = b1;
            }
            c->release_since(rmark);
            k0 = k1;
        }
        // ---- the records in query order, the starts per side, the digest
        R->starts.assign(n_sides + 1, 0); R->pairs.assign(pairs, pairs + 2 * n_pairs);
        for (uint64_t i = 0; i < n_q; ++i) {
            if (!q_kept[i]) continue;
            R->recs.push_back(q_id[i]); R->recs.push_back(dfk_closer::loc_word1(q_pos[i], true));
            ++R->starts[q_side[i] + 1];
        }
        for (uint64_t q = 0; q < n_sides; ++q) R->starts[q + 1] += R->starts[q];
        HIP_TRY(hipMemcpyAsync(h_ctr, ctr.p, 16, hipMemcpyDeviceToHost, c->stream));
        if (!R->recs.empty()) {
            DevBuf d_recs, dg;
            if ((rc = up(d_recs, R->recs.data(), R->recs.size() * 8, "a.close.partners records")) || (rc = c->alloc(dg, 32, "partners digest", Place::Low))) return rc;
            HIP_TRY(hipMemsetAsync(dg.p, 0, 32, c->stream));
            hipLaunchKernelGGL(HIP_KERNEL_NAME(k_digest_seq<uint64_t>), dim3(grid_256(R->recs.size(), cus)), dim3(256), 0, c->stream, (const uint64_t*)d_recs.p, (uint64_t)R->recs.size(), SALT, (unsigned long long*)dg.p);
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
    s[DFK_PARTNERS_PAIRS] = n_pairs; s[DFK_PARTNERS_QUERIES] = q_side.size(); s[DFK_PARTNERS_POSITIONS] = n_positions; s[DFK_PARTNERS_ENTRIES] = tfirst.empty() ? 0 : tfirst.back();
    s[DFK_PARTNERS_ANY_HIT] = h_ctr[0]; s[DFK_PARTNERS_KEPT] = R->recs.size() / 2; s[DFK_PARTNERS_MULTI] = h_ctr[1]; s[DFK_PARTNERS_BATCHES] = n_batches; s[DFK_PARTNERS_RANGES] = n_ranges;
    s[DFK_PARTNERS_US] = (uint64_t)(1e6 * (wall_now() - t_in)); s[DFK_PARTNERS_US_TABLE] = (uint64_t)(1000.0f * ms_table); s[DFK_PARTNERS_US_QUERIES] = (uint64_t)(1000.0f * ms_queries);
    s[DFK_PARTNERS_US_SEARCH] = (uint64_t)(1000.0f * ms_search); s[DFK_PARTNERS_US_COPY] = (uint64_t)(1e6 * s_copy);
    s[DFK_PARTNERS_SUM] = h_dg[0]; s[DFK_PARTNERS_XOR] = h_dg[1]; s[DFK_PARTNERS_SEARCHED] = n_searched;
    if (s[DFK_PARTNERS_ANY_HIT] != s[DFK_PARTNERS_KEPT] + s[DFK_PARTNERS_MULTI]) return fail(DFK_E_HIP, "partners: %llu queries with a hit, %llu kept and %llu dropped", (unsigned long long)h_ctr[0], (unsigned long long)s[DFK_PARTNERS_KEPT], (unsigned long long)h_ctr[1]);
    TRACE("partners: %llu pairs, %llu queries, %llu positions, %llu table entries in %llu range(s), %llu batch(es): %llu kept, %llu dropped; queries %.1f ms, table %.1f ms, search %.1f ms, copies %.1f ms",
          (unsigned long long)n_pairs, (unsigned long long)q_side.size(), (unsigned long long)n_positions, (unsigned long long)s[DFK_PARTNERS_ENTRIES], (unsigned long long)n_ranges, (unsigned long long)n_batches,
          (unsigned long long)s[DFK_PARTNERS_KEPT], (unsigned long long)h_ctr[1], ms_queries, ms_table, ms_search, 1e3 * s_copy);
    return 0;
}

// the file into `dir`: whole, or not at all
int partners_write(const PartnersResult* R, const std::string& dir)
{
    using namespace dfk_partners;
    const std::string path = dir + "/a.close.partners";
    const uint64_t n = R->starts.size() - 1;
    const int fd = open(path.c_str(), O_WRONLY | O_CREAT | O_TRUNC, 0666);
    if (fd < 0) return fail(DFK_E_ARG, "cannot open %s", path.c_str());
    const dfk_closer::BinHead h = dfk_closer::head_of(MAGIC, n);
    bool bad = pwrite_all(fd, &h, 16, 0) != 0 || pwrite_all(fd, R->starts.data(), 8 * (n + 1), 16) != 0;
    if (!bad && !R->recs.empty()) bad = pwrite_all(fd, R->recs.data(), 8 * (uint64_t)R->recs.size(), records_at(n)) != 0;
    if (close(fd) != 0) bad = true;
    if (bad) { (void)unlink(path.c_str()); return fail(DFK_E_ARG, "short write to %s", path.c_str()); }
    return 0;
}

void partners_drop_arrays(dfk_ctx* c)
{
    HostGraph* G = graph_of(c);
    if (G->partners_arrays) { partners_result_free(G->partners_arrays); G->partners_arrays = nullptr; }
}

// the latest build's result: dfk_partners_build_arrays keeps its own beside the graph until the next build of either kind
int partners_result_of(dfk_ctx* c, PartnersResult** out)
{
    if (!c) return fail(DFK_E_ARG, "null context");
    if (c->graph_state && graph_of(c)->partners_arrays) { *out = graph_of(c)->partners_arrays; return 0; }
    PathState* P = built_paths(c);
    if (!P) return fail(DFK_E_STATE, "no partners: call dfk_paths_build, dfk_closer_build and dfk_partners_build");
    if (!P->partners) return fail(DFK_E_STATE, "no partners: call dfk_partners_build");
    *out = P->partners;
    return 0;
}

} // namespace

extern "C" {

int dfk_partners_build(dfk_ctx* c, const int32_t* pairs, uint64_t n_pairs, const uint8_t* packed, const uint64_t* base_off, const uint32_t* read_len, uint64_t n_reads)
{
    return guarded([&]() -> int {
    if (!c) return fail(DFK_E_ARG, "null context");
    PathState* P = built_paths(c);
    if (!P) return fail(DFK_E_STATE, "no paths: call dfk_paths_build");
    if (!P->closer) return fail(DFK_E_STATE, "no closer sets: call dfk_closer_build for these pairs first");
    if (!pairs) {
        if (n_pairs) return fail(DFK_E_ARG, "null argument");
        if (!P->hops_valid) return fail(DFK_E_STATE, "no edge pairs: call dfk_hops_build, or pass the pairs");
        pairs = P->hops.data(); n_pairs = P->hops.size() / 2;
    }
    if (n_reads != P->n_reads) return fail(DFK_E_ARG, "partners: %llu reads given, %llu pathed", (unsigned long long)n_reads, (unsigned long long)P->n_reads);
    if (n_reads && (!packed || !read_len)) return fail(DFK_E_ARG, "null argument");
    PartnerReads reads{packed, base_off, read_len, n_reads, {}};
    if (int rc = partner_reads_check(reads)) return rc;
    if (!base_off) reads.index_dense();
    HIP_TRY(hipSetDevice(c->device));
    const HostGraph* G = graph_of(c);
    const CloserResult* C = P->closer;
    const std::vector<int32_t> inv = involution_of(G);
    // the bases of the edges the anchors name, each once, as a.fastb holds them
    const uint64_t n_anchors = C->anchors.size() / 3;
    std::vector<uint8_t> store, pk;
    std::vector<uint64_t> edge_at(std::max<uint64_t>(1, n_anchors)); std::vector<uint32_t> edge_len(std::max<uint64_t>(1, n_anchors));
    std::unordered_map<uint32_t, uint64_t> at_of;
    for (uint64_t a = 0; a < n_anchors; ++a) {
        const uint32_t g = C->anchors[3 * a];
        if (g >= G->he.size()) return fail(DFK_E_STATE, "the closer sets name edge %u: the graph has %llu", g, (unsigned long long)G->he.size());
        auto it = at_of.find(g);
        if (it == at_of.end()) { packed_edge(*G, G->he[g], &pk); it = at_of.emplace(g, (uint64_t)store.size()).first; store.insert(store.end(), pk.begin(), pk.end()); }
        edge_at[a] = it->second; edge_len[a] = G->ce[G->he[g].ce].n + G->K - 1;
    }
    const PartnersSource S{inv.size(), inv.data(), store.data(), store.size(), edge_at.data(), edge_len.data(), C->ce.size(), C->ce.data(), C->loc_first.data(), C->locs.data(),
                           C->anchor_first.data(), (const int32_t*)C->anchors.data(), &reads};
    std::unique_ptr<PartnersResult> R(new PartnersResult);
    if (int rc = partners_build(c, S, pairs, n_pairs, 0, R.get())) return rc;     // (refused: the earlier result is still served)
    partners_drop_arrays(c);
    if (P->partners) partners_result_free(P->partners);
    P->partners = R.release(); P->partners_free = partners_result_free;
    return 0;
    });
}

// The stage on host arrays: everything it reads is given, and checked here for the form dfk_closer_fetch gives -- ce ascending,
// the starts rising, in every rank the forward records first and ascending by id, every id a read, every anchor an edge.
int dfk_partners_build_arrays(dfk_ctx* c, uint64_t n_edges, const int32_t* inv, const uint8_t* edge_packed, const uint64_t* edge_off, const uint32_t* edge_len,
                              uint64_t n_ce, const uint64_t* ce, const uint64_t* loc_first, const uint64_t* locs, const uint64_t* anchor_first, const int32_t* anchors,
                              const int32_t* pairs, uint64_t n_pairs, const uint8_t* packed, const uint64_t* base_off, const uint32_t* read_len, uint64_t n_reads,
                              uint64_t queries_per_batch, const char* dir)
{
    return guarded([&]() -> int {
    if (!c) return fail(DFK_E_ARG, "null context");
    const uint64_t E = n_edges, N = n_reads;
    if ((E && (!inv || !edge_len)) || !edge_off || !loc_first || !anchor_first || (n_ce && !ce) || (n_pairs && !pairs) || (N && (!packed || !read_len))) return fail(DFK_E_ARG, "null argument");
    if (N >= (1ull << 31) || E >= (1ull << 31)) return fail(DFK_E_ARG, "%llu reads, %llu edges: 2^31 - 1 of each at most", (unsigned long long)N, (unsigned long long)E);
    for (uint64_t e = 0; e < E; ++e) {
        if (inv[e] < 0 || (uint64_t)inv[e] >= E || inv[inv[e]] != (int32_t)e) return fail(DFK_E_ARG, "inv is not an involution at edge %llu", (unsigned long long)e);
        if (edge_off[e + 1] < edge_off[e] || edge_off[e + 1] - edge_off[e] < ((uint64_t)edge_len[e] + 3) / 4) return fail(DFK_E_ARG, "edge %llu has fewer bytes than its bases need", (unsigned long long)e);
    }
    if (edge_off[E] && !edge_packed) return fail(DFK_E_ARG, "null argument");
    if (loc_first[0] != 0 || anchor_first[0] != 0) return fail(DFK_E_ARG, "the tables do not start at 0");
    for (uint64_t k = 0; k < n_ce; ++k) {
        if (ce[k] >= E || (k && ce[k] <= ce[k - 1])) return fail(DFK_E_ARG, "the closer edges are not ascending edges of the graph at rank %llu", (unsigned long long)k);
        if (loc_first[k + 1] < loc_first[k] || anchor_first[k + 1] < anchor_first[k]) return fail(DFK_E_ARG, "a table's starts fall at rank %llu", (unsigned long long)k);
    }
    if ((loc_first[n_ce] && !locs) || (anchor_first[n_ce] && !anchors)) return fail(DFK_E_ARG, "null argument");
    for (uint64_t k = 0; k < n_ce; ++k)
        for (uint64_t j = loc_first[k]; j < loc_first[k + 1]; ++j) {
            if (locs[2 * j] >= N) return fail(DFK_E_ARG, "a locs record names read %llu of %llu", (unsigned long long)locs[2 * j], (unsigned long long)N);
            if (j > loc_first[k] && dfk_partners::loc_fw(locs, j) && (!dfk_partners::loc_fw(locs, j - 1) || locs[2 * j] < locs[2 * (j - 1)]))
                return fail(DFK_E_ARG, "rank %llu: the forward records do not come first, ascending by id, as dfk_closer_fetch gives them", (unsigned long long)k);
        }
    const uint64_t n_anchors = anchor_first[n_ce];
    std::vector<uint64_t> edge_at(std::max<uint64_t>(1, n_anchors)); std::vector<uint32_t> a_len(std::max<uint64_t>(1, n_anchors));
    for (uint64_t a = 0; a < n_anchors; ++a) {
        if (anchors[3 * a] < 0 || (uint64_t)anchors[3 * a] >= E) return fail(DFK_E_ARG, "an anchor names edge %d: the graph has %llu", anchors[3 * a], (unsigned long long)E);
        edge_at[a] = edge_off[anchors[3 * a]]; a_len[a] = edge_len[anchors[3 * a]];
    }
    PartnerReads reads{packed, base_off, read_len, N, {}};
    if (int rc = partner_reads_check(reads)) return rc;
    if (!base_off) reads.index_dense();
    HIP_TRY(hipSetDevice(c->device));
    const PartnersSource S{E, inv, edge_packed, edge_off[E], edge_at.data(), a_len.data(), n_ce, ce, loc_first, locs, anchor_first, anchors, &reads};
    std::unique_ptr<PartnersResult> R(new PartnersResult);
    if (int rc = partners_build(c, S, pairs, n_pairs, queries_per_batch, R.get())) return rc;
    if (dir) if (int rc = partners_write(R.get(), dir)) return rc;
    partners_drop_arrays(c);
    graph_of(c)->partners_arrays = R.release(); graph_of(c)->partners_free = partners_result_free;
    return 0;
    });
}

int dfk_partners_stats(dfk_ctx* c, uint64_t* out)
{
    return guarded([&]() -> int {
    PartnersResult* R = nullptr;
    if (int rc = partners_result_of(c, &R)) return rc;
    if (!out) return fail(DFK_E_ARG, "null argument");
    for (int i = 0; i < DFK_PARTNERS_WORDS; ++i) out[i] = R->stats[i];
    return 0;
    });
}

int dfk_partners_fetch(dfk_ctx* c, uint64_t* starts, uint64_t* n_elements, uint64_t* recs, uint64_t recs_cap, uint64_t* n_recs)
{
    return guarded([&]() -> int {
    PartnersResult* R = nullptr;
    if (int rc = partners_result_of(c, &R)) return rc;
    const uint64_t n = R->starts.size() - 1, nr = R->recs.size() / 2;
    if (n_elements) *n_elements = n;
    if (n_recs) *n_recs = nr;
    if ((recs || recs_cap) && recs_cap < nr) return fail(DFK_E_ARG, "buffer too small: %llu < %llu partner records", (unsigned long long)recs_cap, (unsigned long long)nr);
    if (recs_cap && nr && !recs) return fail(DFK_E_ARG, "null argument");
    if (recs && nr) memcpy(recs, R->recs.data(), 16 * nr);
    if (starts) memcpy(starts, R->starts.data(), 8 * (n + 1));                 // the starts: room for n_elements + 1 words
    return 0;
    });
}

int dfk_partners_write(dfk_ctx* c, const char* dir)
{
    return guarded([&]() -> int {
    PartnersResult* R = nullptr;
    if (int rc = partners_result_of(c, &R)) return rc;
    if (!dir) return fail(DFK_E_ARG, "null directory");
    return partners_write(R, dir);
    });
}

} // extern "C"
