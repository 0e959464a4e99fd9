// superplus_amd/csrc/dfk_walks.inc -- Stackster's two stack walks per pair (10X/Stackster.cc:207-262, :326-414) and the file
// a.stack.walks, included by dfk.hip.
//
// The rule, the shared pieces, the plan and the file's layout: dfk_walks.h.  The kernels: dfk_walks_kernels.h.  Here: walks_build() -- a
// range of pairs at a time the sets composed on the host, under it the batches of pairs: the distinct reads of the batch gathered on the
// host and decoded on the device (dfk_cons.inc's cn_batch_reads), lowered once a read, then side 0 and side 1 in turn: the side's
// 48-mers hashed, sorted by ( pair, hash ) with the closer's radix sort on a permutation, the walks a wave each, the outcome back, the
// walks whose live list outgrew its room done by the header's literal form on the host, the walked sequences brought together -- and
// walks_write().  Everything on the device comes from the arena and goes back before build returns.
#include "dfk_walks_kernels.h"

namespace {

struct WalksResult {
    std::vector<uint64_t> starts, ee_starts;      // [2 * n_pairs + 1]
    std::vector<dfk_walks::Rec> recs;             // [2 * n_pairs]
    std::vector<dfk_walks::Loc> locs;
    std::vector<uint8_t> ee;                      // a byte a base
    uint64_t n_reads = 0;                         // the reads it was made from: dfk_scons_build asks for as many
    uint64_t stats[DFK_WALKS_WORDS] = {};
    uint64_t serial = 0;                          // which build made it: dfk_scons_build notes it, dfk_soffsets_build asks for the same
    std::vector<int32_t> pairs;                   // dfk_walks_build: the pairs it was made for (dfk_allclosures_write asks)
};
void walks_result_free(WalksResult* r) { delete r; }

struct WalksSource {
    uint64_t n_edges; const int32_t* inv;
    uint64_t n_ce; const uint64_t* ce; const uint8_t* edge_store; uint64_t edge_store_bytes; const uint64_t* edge_at; const int32_t* edge_len;   // per rank: O(ce[k])
    const uint64_t* read_first; const uint64_t* reads;
    const PartnerReads* rd; const uint8_t* pq; const uint64_t* pq_off;
};

struct WkSwitches { uint32_t max_live, hash_bits; };
WkSwitches walk_switches()                         // DFK_WALK_MAX_LIVE (at most the kernel's room), DFK_WALK_HASH_BITS: tests force the host route and collisions
{
    WkSwitches s{dfk_walks::MAX_LIVE, 64};
    if (const char* e = getenv("DFK_WALK_MAX_LIVE")) s.max_live = (uint32_t)std::min<long long>(dfk_walks::MAX_LIVE, std::max<long long>(1, atoll(e)));
    if (const char* e = getenv("DFK_WALK_HASH_BITS")) s.hash_bits = (uint32_t)std::min<long long>(64, std::max<long long>(1, atoll(e)));
    return s;
}

// one walk by the header's literal form on the host: the entries' reads fetched, decoded, lowered and oriented here
int walk_on_host(dfk_ctx* c, const WalksSource& S, const std::vector<uint64_t>& set, uint32_t side, uint64_t k, dfk_walks::Walk* W)
{
    using namespace dfk_walks;
    std::vector<basevector> by(set.size()); std::vector<qualvector> qy(set.size());
    for (size_t i = 0; i < set.size(); ++i) {
        const uint64_t id = set[i] >> 1;
        uint32_t len; uint64_t pe[2];
        int rc;
        if ((rc = host_read(c, &len, S.rd->len + id, 4)) || (rc = host_read(c, pe, (const char*)S.pq_off + 8 * id, 16))) return rc;
        std::vector<uint8_t> pk(((uint64_t)len + 3) / 4 + 1), pq(pe[1] - pe[0] + 1), q((uint64_t)len + 1);
        if (len && (rc = host_read(c, pk.data(), S.rd->packed + S.rd->at(id), ((uint64_t)len + 3) / 4))) return rc;
        if (pe[1] > pe[0] && (rc = host_read(c, pq.data(), S.pq + pe[0], pe[1] - pe[0]))) return rc;
        if (!dfk_cons::decode_quals(pq.data(), 0, pe[1] - pe[0], q.data(), len)) return fail(DFK_E_INPUT, "walks: a PQVec stream does not hold exactly as many qualities as its read has bases");
        lower_read(pk.data(), len, q.data());
        const bool rcf = entry_rc((set[i] & 1) != 0, side);
        by[i].resize(len); qy[i].resize(len);
        for (uint32_t j = 0; j < len; ++j) { by[i][j] = (uint8_t)oriented_base(pk.data(), len, rcf, j); qy[i][j] = oriented_qual(q.data(), len, rcf, j); }
    }
    basevector E((size_t)S.edge_len[k]);
    for (size_t j = 0; j < E.size(); ++j) E[j] = (uint8_t)base_at(S.edge_store + S.edge_at[k], j);
    stack_walk(E, by, qy, W);
    return 0;
}

int walks_build(dfk_ctx* c, const WalksSource& S, const int32_t* pairs, uint64_t n_pairs, uint64_t walks_per_batch, WalksResult* R)
{
    using namespace dfk_walks;
    const uint64_t N = S.rd->n, n_ce = S.n_ce, n_set = S.read_first[n_ce];
    if (N > (1ull << 31) || n_pairs >= (1ull << 30)) return fail(DFK_E_ARG, "%llu reads, %llu pairs: an entry keeps its read in 31 bits", (unsigned long long)N, (unsigned long long)n_pairs);
    for (uint64_t i = 0; i < 2 * n_pairs; ++i)
        if (pairs[i] < 0 || (uint64_t)pairs[i] >= S.n_edges) return fail(DFK_E_ARG, "pair %llu names edge %d: the graph has %llu", (unsigned long long)(i / 2), pairs[i], (unsigned long long)S.n_edges);
    std::vector<uint32_t> side_rank(std::max<uint64_t>(1, 2 * n_pairs), 0);
    std::vector<uint64_t> n_ent(n_pairs, 0);
    for (uint64_t pi = 0; pi < n_pairs; ++pi) {
        const uint64_t es[2] = {(uint64_t)pairs[2 * pi], (uint64_t)S.inv[pairs[2 * pi + 1]]};
        for (int s = 0; s < 2; ++s) {
            const uint64_t k = rank_in(S.ce, n_ce, es[s]);
            if (k == n_ce) return fail(DFK_E_ARG, "pair %llu: edge %llu is not among the closer edges: the closer sets were built for other pairs", (unsigned long long)pi, (unsigned long long)es[s]);
            side_rank[2 * pi + s] = (uint32_t)k;
            n_ent[pi] += S.read_first[k + 1] - S.read_first[k];
        }
        if (n_ent[pi] >= MAX_ENTRIES) {                                        // (rare: the set composed here too, since entries the two edges share count once)
            std::vector<uint64_t> set(S.reads + S.read_first[side_rank[2 * pi]], S.reads + S.read_first[side_rank[2 * pi] + 1]);
            for (uint64_t j = S.read_first[side_rank[2 * pi + 1]]; j < S.read_first[side_rank[2 * pi + 1] + 1]; ++j) set.push_back(S.reads[j] ^ 1);
            std::sort(set.begin(), set.end());
            const uint64_t n = (uint64_t)(std::unique(set.begin(), set.end()) - set.begin());
            if (n >= MAX_ENTRIES) return fail(DFK_E_ARG, "pair %llu: a set of %llu entries: the walk's integer sums are safe below 2^23", (unsigned long long)pi, (unsigned long long)n);
        }
    }
    for (uint64_t j = 0; j < n_set; ++j) if ((S.reads[j] >> 1) >= N) return fail(DFK_E_ARG, "a set entry names read %llu of %llu", (unsigned long long)(S.reads[j] >> 1), (unsigned long long)N);
    const std::vector<uint64_t> efirst = prefix_sums(n_ent.data(), n_pairs);
    const WkSwitches sw = walk_switches();
    const uint64_t mask = hash_mask(sw.hash_bits);
    const unsigned cus = (unsigned)c->prop.multiProcessorCount;
    const double t_in = wall_now();
    const uint64_t mark = c->alloc_seq;
    CnTimes times;
    float ms_lower = 0, ms_sort = 0, ms_walk = 0;
    uint64_t n_batches = 0, n_ranges = 0, n_decoded = 0, n_items_all = 0, n_host = 0, n_steps = 0, live_sum = 0, live_max = 0, n_verified = 0, n_collisions = 0, h_dg[8] = {};
    R->starts.assign(1, 0); R->ee_starts.assign(1, 0); R->n_reads = N; R->serial = cons_next_serial();
    auto len_of = [&](uint64_t id, uint32_t* len) { return host_read(c, len, S.rd->len + id, 4); };
    auto body = [&]() -> int {
        int rc;
        Timer tm(c->stream);
        DevBuf d_edges;
        CnTables T;                                                            // (of the consensus' tables only the count of streams that did not decode)
        if ((rc = cn_up(c, d_edges, S.edge_store, S.edge_store_bytes, "closer edges' bases")) || (rc = c->alloc(T.bad, 8, "streams that did not decode", Place::Low))) return rc;
        HIP_TRY(hipMemsetAsync(T.bad.p, 0, 8, c->stream));
        const ConsSource CS{S.n_edges, S.inv, 0, nullptr, nullptr, nullptr, nullptr, 0, nullptr, nullptr, S.rd, S.pq, S.pq_off};
        const uint64_t forced = path_switches().pidx_range_pairs;
        for (uint64_t p0 = 0; p0 < n_pairs;) {
            const PidxRange range = next_range(efirst.data(), n_pairs, p0, entry_cap(c->largest_allocatable(), forced));
            const uint64_t p1 = range.e1, np = p1 - p0;
            ++n_ranges;
            // ---- the sets of the range, composed; what each pair costs a batch
            std::vector<std::vector<uint64_t>> sets(np);
            std::vector<std::vector<uint32_t>> lens(np);
            std::vector<uint64_t> cost(np);
            for (uint64_t p = 0; p < np; ++p) {
                const uint64_t k0 = side_rank[2 * (p0 + p)], k1 = side_rank[2 * (p0 + p) + 1];
                sets[p].assign(S.reads + S.read_first[k0], S.reads + S.read_first[k0 + 1]);
                for (uint64_t j = S.read_first[k1]; j < S.read_first[k1 + 1]; ++j) sets[p].push_back(S.reads[j] ^ 1);
                std::sort(sets[p].begin(), sets[p].end());
                sets[p].erase(std::unique(sets[p].begin(), sets[p].end()), sets[p].end());
                lens[p].resize(sets[p].size());
                cost[p] = BYTES_PER_PAIR;
                uint64_t qbytes = 0;
                for (size_t i = 0; i < sets[p].size(); ++i) { if ((rc = len_of(sets[p][i] >> 1, &lens[p][i]))) return rc; cost[p] += entry_cost(lens[p][i]); qbytes += lens[p][i]; }
                if (qbytes >= (1ull << 31)) return fail(DFK_E_ARG, "pair %llu: its set holds %llu bases: a walk keeps 32-bit offsets", (unsigned long long)(p0 + p), (unsigned long long)qbytes);
            }
            const std::vector<uint64_t> cfirst = prefix_sums(cost.data(), np);
            for (uint64_t b0 = 0; b0 < np;) {
                const uint64_t b1 = next_batch(cfirst.data(), np, b0, batch_room(c->largest_allocatable()), pairs_per_batch(walks_per_batch)), nb = b1 - b0;
                ++n_batches;
                const uint64_t bmark = c->alloc_seq;
                // ---- the entries of the batch; the reads, each once: gathered, decoded, lowered
                std::vector<uint64_t> ent_first(nb + 1, 0);
                for (uint64_t p = 0; p < nb; ++p) ent_first[p + 1] = ent_first[p] + sets[b0 + p].size();
                const uint64_t ne = ent_first[nb];
                CnRange G;
                G.h_lfirst = {0, ne};
                G.h_id.resize(ne);
                std::vector<uint32_t> ent_len(ne);
                for (uint64_t p = 0; p < nb; ++p) for (size_t i = 0; i < sets[b0 + p].size(); ++i) { G.h_id[ent_first[p] + i] = (uint32_t)(sets[b0 + p][i] >> 1); ent_len[ent_first[p] + i] = lens[b0 + p][i]; }
                std::vector<uint32_t> ids(G.h_id);
                std::sort(ids.begin(), ids.end()); ids.erase(std::unique(ids.begin(), ids.end()), ids.end());
                {   // the walk keeps where a read's bases and qualities begin in 32 bits: batch_room() sees to that, a forced batch is checked here
                    uint64_t qbytes = 0;
                    for (uint32_t id : ids) { uint32_t len; if ((rc = len_of(id, &len))) return rc; qbytes += (uint64_t)len + 4; }
                    if (qbytes >= (1ull << 32)) return fail(DFK_E_ARG, "walks: a batch of %llu pairs holds %llu bases: 2^32 at most (fewer walks a batch)", (unsigned long long)nb, (unsigned long long)qbytes);
                }
                const double t_batch = wall_now();
                CnReads B;
                if ((rc = cn_batch_reads(c, CS, T, G, 0, 1, tm, &times, &B))) return rc;
                if (B.n_ids != ids.size()) return fail(DFK_E_HIP, "walks: %llu reads gathered for %llu", (unsigned long long)B.n_ids, (unsigned long long)ids.size());
                n_decoded += B.n_ids;
                tm.start();
                if (B.n_ids) {
                    hipLaunchKernelGGL(k_wk_lower, dim3(grid_256(B.n_ids, cus)), dim3(256), 0, c->stream, (const uint8_t*)B.bases.p, (const uint64_t*)B.bat.p, (const uint64_t*)B.qat.p, B.n_ids, (uint8_t*)B.quals.p);
                    HIP_TRY(hipGetLastError());
                }
                std::vector<uint32_t> ent_slot(ne);
                std::vector<uint64_t> kfirst(ne + 1, 0), ee_first(nb + 1, 0);
                for (uint64_t p = 0; p < nb; ++p) {
                    for (size_t i = 0; i < sets[b0 + p].size(); ++i) {
                        const uint64_t at = ent_first[p] + i;
                        ent_slot[at] = (uint32_t)dfk_cons::slot_of(ids.data(), ids.size(), G.h_id[at]) | ((sets[b0 + p][i] & 1) ? 0x80000000u : 0u);
                        kfirst[at + 1] = kfirst[at] + kmers_of_len(ent_len[at]);
                    }
                    ee_first[p + 1] = ee_first[p] + ee_bound(ent_len.data() + ent_first[p], ent_first[p + 1] - ent_first[p]);
                }
                const uint64_t n_items = kfirst[ne];
                if (n_items >= (1ull << 32)) return fail(DFK_E_ARG, "walks: a batch of %llu 48-mers: the sort keeps 32-bit places", (unsigned long long)n_items);
                DevBuf d_ent_first, d_ent_slot, d_kfirst, d_ee_first, d_go, d_edge_at, d_placed, d_start, d_ee, d_out, d_hash, d_val, d_ofirst, d_eeout;
                if ((rc = cn_up(c, d_ent_first, ent_first.data(), (nb + 1) * 8, "entries per pair")) || (rc = cn_up(c, d_ent_slot, ent_slot.data(), ne * 4, "entries' reads")) ||
                    (rc = cn_up(c, d_kfirst, kfirst.data(), (ne + 1) * 8, "48-mers per entry")) || (rc = cn_up(c, d_ee_first, ee_first.data(), (nb + 1) * 8, "walks' bounds")) ||
                    (rc = c->alloc(d_go, std::max<uint64_t>(8, nb), "walks to make", Place::Low)) || (rc = c->alloc(d_edge_at, nb * 8, "walks' edges", Place::Low)) ||
                    (rc = c->alloc(d_placed, std::max<uint64_t>(8, ne), "placed flags", Place::Low)) || (rc = c->alloc(d_start, std::max<uint64_t>(8, ne * 4), "starts", Place::Low)) ||
                    (rc = c->alloc(d_ee, std::max<uint64_t>(8, ee_first[nb]), "walked sequences", Place::Low)) || (rc = c->alloc(d_out, nb * sizeof(WkOut), "walks' outcomes", Place::Low)) ||
                    (rc = c->alloc(d_hash, (n_items + 1) * 8, "48-mer hashes, sorted", Place::Low)) || (rc = c->alloc(d_val, (n_items + 1) * 8, "their entries and positions", Place::Low)) ||
                    (rc = c->alloc(d_ofirst, (nb + 1) * 8, "walked sequences' places", Place::Low))) return rc;
                HIP_TRY(hipStreamSynchronize(c->stream));
                ms_lower += tm.stop();
                const WkBatch Bk{nb, ne, (const uint64_t*)d_ent_first.p, (const uint32_t*)d_ent_slot.p, (const uint64_t*)d_kfirst.p, (const uint64_t*)B.bat.p, (const uint64_t*)B.qat.p,
                                 (const uint8_t*)B.bases.p, (const uint8_t*)B.quals.p};
                std::vector<Rec> recs(2 * nb);
                std::vector<std::vector<Loc>> locs(2 * nb);
                std::vector<std::vector<uint8_t>> ees(2 * nb);
                std::vector<uint8_t> go(nb, 1);
                for (uint32_t side = 0; side < 2; ++side) {
                    std::vector<uint64_t> edge_at(nb);
                    std::vector<uint8_t> walk(nb, 0);
                    uint64_t n_go = 0;
                    for (uint64_t p = 0; p < nb; ++p) {
                        const uint64_t k = side_rank[2 * (p0 + b0 + p) + side];
                        edge_at[p] = S.edge_at[k];
                        recs[2 * p + side] = Rec{go[p] ? (uint32_t)WALKED : (uint32_t)NOT_WALKED, (uint32_t)(ent_first[p + 1] - ent_first[p]), 0, 0, S.edge_len[k], 0, 0, 0};
                        if (go[p] && S.edge_len[k] < (int32_t)KW) recs[2 * p + side].status = SHORT;
                        walk[p] = go[p] && recs[2 * p + side].status == WALKED;
                        n_go += walk[p];
                    }
                    std::vector<WkOut> outs(nb);
                    std::vector<uint8_t> h_placed(ne + 1, 0), h_ee;
                    std::vector<int32_t> h_start(ne + 1, -1);
                    std::vector<uint64_t> out_first(nb + 1, 0);
                    if (n_go) {
                        // ---- the table of the side: ( pair, hash ) -> ( entry, pos )
                        tm.start();
                        if (n_items) {
                            const uint64_t smark = c->alloc_seq;
                            DevBuf klo, khi, kpair, kent, kpos, k[2], v[2];
                            auto u32s = [&](DevBuf& d, const char* what) { return c->alloc(d, n_items * 4, what, Place::Low); };
                            if ((rc = u32s(klo, "hashes, low words")) || (rc = u32s(khi, "hashes, high words")) || (rc = u32s(kpair, "48-mers' pairs")) || (rc = u32s(kent, "48-mers' entries")) ||
                                (rc = u32s(kpos, "48-mers' positions")) || (rc = u32s(k[0], "sort keys")) || (rc = u32s(k[1], "sort keys")) || (rc = u32s(v[0], "sort places")) || (rc = u32s(v[1], "sort places"))) return rc;
                            const unsigned g = grid_256(n_items, cus);
                            hipLaunchKernelGGL(k_wk_kmers, dim3(g), dim3(256), 0, c->stream, Bk, side, mask, n_items, (uint32_t*)klo.p, (uint32_t*)khi.p, (uint32_t*)kpair.p, (uint32_t*)kent.p, (uint32_t*)kpos.p);
                            HIP_TRY(hipGetLastError());
                            // sorted by ( pair, hash ): the permutation by the hash's low word, its high word, the pair -- least significant first, every sort stable
                            int cur = 0;
                            HIP_TRY(hipMemcpyAsync(k[0].p, klo.p, n_items * 4, hipMemcpyDeviceToDevice, c->stream));
                            hipLaunchKernelGGL(k_cl_iota, dim3(g), dim3(256), 0, c->stream, (uint32_t*)v[0].p, n_items);
                            HIP_TRY(hipGetLastError());
                            if ((rc = radix_sort_pairs(c, k, v, n_items, std::min<uint32_t>(32, sw.hash_bits), &cur))) return rc;
                            if (sw.hash_bits > 32) {
                                hipLaunchKernelGGL(k_cl_gather, dim3(g), dim3(256), 0, c->stream, (const uint32_t*)khi.p, (const uint32_t*)v[cur].p, n_items, (uint32_t*)k[cur].p);
                                HIP_TRY(hipGetLastError());
                                if ((rc = radix_sort_pairs(c, k, v, n_items, sw.hash_bits - 32, &cur))) return rc;
                            }
                            if (nb > 1) {
                                hipLaunchKernelGGL(k_cl_gather, dim3(g), dim3(256), 0, c->stream, (const uint32_t*)kpair.p, (const uint32_t*)v[cur].p, n_items, (uint32_t*)k[cur].p);
                                HIP_TRY(hipGetLastError());
                                if ((rc = radix_sort_pairs(c, k, v, n_items, dfk_closer::bits_for(nb), &cur))) return rc;
                            }
                            hipLaunchKernelGGL(k_wk_sorted, dim3(g), dim3(256), 0, c->stream, (const uint32_t*)v[cur].p, (const uint32_t*)klo.p, (const uint32_t*)khi.p, (const uint32_t*)kent.p, (const uint32_t*)kpos.p, n_items,
                                               (uint64_t*)d_hash.p, (uint64_t*)d_val.p);
                            HIP_TRY(hipGetLastError());
                            HIP_TRY(hipStreamSynchronize(c->stream));
                            c->release_since(smark);
                            n_items_all += n_items;
                        }
                        ms_sort += tm.stop();
                        // ---- the walks, a wave each
                        tm.start();
                        if ((rc = upload(c, d_go.p, walk.data(), nb)) || (rc = upload(c, d_edge_at.p, edge_at.data(), nb * 8))) return rc;
                        const WkWalks Wk{side, sw.max_live, mask, (const uint8_t*)d_go.p, (const uint8_t*)d_edges.p, (const uint64_t*)d_edge_at.p, (const uint64_t*)d_hash.p, (const uint64_t*)d_val.p, (const uint64_t*)d_ee_first.p};
                        hipLaunchKernelGGL(k_wk_walk, dim3(walk_grid(nb, cus)), dim3(64), 0, c->stream, Bk, Wk, (uint8_t*)d_placed.p, (int32_t*)d_start.p, (uint8_t*)d_ee.p, (WkOut*)d_out.p);
                        HIP_TRY(hipGetLastError());
                        HIP_TRY(hipMemcpyAsync(outs.data(), d_out.p, nb * sizeof(WkOut), hipMemcpyDeviceToHost, c->stream));
                        if (ne) {
                            HIP_TRY(hipMemcpyAsync(h_placed.data(), d_placed.p, ne, hipMemcpyDeviceToHost, c->stream));
                            HIP_TRY(hipMemcpyAsync(h_start.data(), d_start.p, ne * 4, hipMemcpyDeviceToHost, c->stream));
                        }
                        HIP_TRY(hipStreamSynchronize(c->stream));
                        for (uint64_t p = 0; p < nb; ++p) {
                            const bool dev = walk[p] && outs[p].state == 0;
                            if (walk[p] && outs[p].state > 1) return fail(DFK_E_HIP, "walks: pair %llu side %u met its bound of %llu bases", (unsigned long long)(p0 + b0 + p), side, (unsigned long long)(ee_first[p + 1] - ee_first[p]));
                            if (dev && (outs[p].nEE < KW || outs[p].nEE > ee_first[p + 1] - ee_first[p] || outs[p].placed > ent_first[p + 1] - ent_first[p]))
                                return fail(DFK_E_HIP, "walks: pair %llu side %u walked %u bases and placed %u", (unsigned long long)(p0 + b0 + p), side, outs[p].nEE, outs[p].placed);
                            out_first[p + 1] = out_first[p] + (dev ? outs[p].nEE : 0);
                        }
                        h_ee.assign(out_first[nb] + 1, 0);
                        if (out_first[nb]) {
                            if ((rc = c->alloc(d_eeout, out_first[nb], "walked sequences, together", Place::Low)) || (rc = upload(c, d_ofirst.p, out_first.data(), (nb + 1) * 8))) return rc;
                            hipLaunchKernelGGL(k_wk_collect, dim3(grid_256(out_first[nb], cus)), dim3(256), 0, c->stream, (const uint8_t*)d_ee.p, (const uint64_t*)d_ee_first.p, (const uint64_t*)d_ofirst.p, nb, out_first[nb], (uint8_t*)d_eeout.p);
                            HIP_TRY(hipGetLastError());
                            HIP_TRY(hipMemcpyAsync(h_ee.data(), d_eeout.p, out_first[nb], hipMemcpyDeviceToHost, c->stream));
                            HIP_TRY(hipStreamSynchronize(c->stream));
                            c->release(d_eeout);
                        }
                        ms_walk += tm.stop();
                    }
                    // ---- the records of the side; the host route where the live list outgrew its room
                    for (uint64_t p = 0; p < nb; ++p) {
                        Rec& r = recs[2 * p + side];
                        if (walk[p]) {
                            const uint64_t e0 = ent_first[p];
                            if (outs[p].state == 1) {
                                ++n_host;
                                Walk W;
                                if ((rc = walk_on_host(c, S, sets[b0 + p], side, side_rank[2 * (p0 + b0 + p) + side], &W))) return rc;
                                r.nEE = (uint32_t)W.EE.size(); r.dup_steps = W.dup_steps;
                                std::vector<int32_t> st(W.start.begin(), W.start.end());
                                finish_side(sets[b0 + p], ent_len.data() + e0, side, W.placed.data(), st.data(), &r, &locs[2 * p + side]);
                                ees[2 * p + side] = W.EE;
                                n_steps += W.steps; live_sum += W.live_sum; live_max = std::max(live_max, W.live_max);
                            } else {
                                r.nEE = outs[p].nEE; r.dup_steps = outs[p].dup_steps;
                                finish_side(sets[b0 + p], ent_len.data() + e0, side, h_placed.data() + e0, h_start.data() + e0, &r, &locs[2 * p + side]);
                                if (r.placed != outs[p].placed || r.M != outs[p].M) return fail(DFK_E_HIP, "walks: pair %llu side %u: %u placed with M %d on the device, %u with %d here", (unsigned long long)(p0 + b0 + p), side, outs[p].placed, outs[p].M, r.placed, r.M);
                                ees[2 * p + side].assign(h_ee.begin() + out_first[p], h_ee.begin() + out_first[p + 1]);
                                for (uint8_t b : ees[2 * p + side]) if (b > 3) return fail(DFK_E_HIP, "walks: base %u in a walked sequence", b);
                                n_steps += outs[p].steps; live_sum += outs[p].live_sum; live_max = std::max<uint64_t>(live_max, outs[p].live_max);
                                n_verified += outs[p].verified; n_collisions += outs[p].collisions;
                            }
                        }
                        if (!r.placed) go[p] = 0;                              // :404-408
                    }
                }
                for (uint64_t q = 0; q < 2 * nb; ++q) {
                    R->recs.push_back(recs[q]);
                    R->locs.insert(R->locs.end(), locs[q].begin(), locs[q].end());
                    R->ee.insert(R->ee.end(), ees[q].begin(), ees[q].end());
                    R->starts.push_back(R->locs.size()); R->ee_starts.push_back(R->ee.size());
                }
                TRACE("walks: batch %llu: pairs [%llu, %llu) of %llu, %llu entries, %llu 48-mers a side, %.2f s; so far table %.1f ms, walks %.1f ms, %llu steps", (unsigned long long)n_batches,
                      (unsigned long long)(p0 + b0), (unsigned long long)(p0 + b1), (unsigned long long)n_pairs, (unsigned long long)ne, (unsigned long long)n_items, wall_now() - t_batch, ms_sort, ms_walk, (unsigned long long)n_steps);
                c->release_since(bmark);
                b0 = b1;
            }
            p0 = p1;
        }
        // ---- the digest
        const uint64_t n = 2 * n_pairs, nl = R->locs.size(), nbases = R->ee.size();
        if (n) {
            DevBuf d_r, d_l, d_b, dg;
            if ((rc = cn_up(c, d_r, R->recs.data(), n * 32, "a.stack.walks records")) || (rc = cn_up(c, d_l, R->locs.data(), nl * 16, "a.stack.walks placed records")) ||
                (rc = cn_up(c, d_b, R->ee.data(), nbases, "a.stack.walks bases")) || (rc = c->alloc(dg, 32, "walks digest", Place::Low))) return rc;
            HIP_TRY(hipMemsetAsync(dg.p, 0, 32, c->stream));
            hipLaunchKernelGGL(HIP_KERNEL_NAME(k_digest_seq<uint32_t>), dim3(grid_256(8 * n, cus)), dim3(256), 0, c->stream, (const uint32_t*)d_r.p, (uint64_t)(8 * n), SALT, (unsigned long long*)dg.p);
            if (nl) hipLaunchKernelGGL(HIP_KERNEL_NAME(k_digest_seq<uint64_t>), dim3(grid_256(2 * nl, cus)), dim3(256), 0, c->stream, (const uint64_t*)d_l.p, (uint64_t)(2 * nl), SALT + 8 * n, (unsigned long long*)dg.p);
            if (nbases) hipLaunchKernelGGL(HIP_KERNEL_NAME(k_digest_seq<uint8_t>), dim3(grid_256(nbases, cus)), dim3(256), 0, c->stream, (const uint8_t*)d_b.p, nbases, SALT + 8 * n + 2 * nl, (unsigned long long*)dg.p);
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
    s[DFK_WALKS_PAIRS] = n_pairs; s[DFK_WALKS_STEPS] = n_steps; s[DFK_WALKS_LIVE_SUM] = live_sum; s[DFK_WALKS_LIVE_MAX] = live_max; s[DFK_WALKS_HOST_ROUTE] = n_host;
    s[DFK_WALKS_VERIFIED] = n_verified; s[DFK_WALKS_COLLISIONS] = n_collisions; s[DFK_WALKS_KMERS] = n_items_all; s[DFK_WALKS_DECODED] = n_decoded; s[DFK_WALKS_BATCHES] = n_batches; s[DFK_WALKS_RANGES] = n_ranges;
    for (uint64_t q = 0; q < 2 * n_pairs; ++q) {
        const Rec& r = R->recs[q];
        if (r.status == WALKED) { ++s[DFK_WALKS_WALKS]; s[DFK_WALKS_ENTRIES] += r.entries; s[DFK_WALKS_PAST_EDGE] += (int64_t)r.nEE > r.nE; if (q % 2 && !r.placed) ++s[DFK_WALKS_SIDE1_EMPTY]; }
        if (q % 2 == 0 && !r.placed) ++s[DFK_WALKS_SIDE0_EMPTY];
        s[DFK_WALKS_PLACED] += r.placed; s[DFK_WALKS_EE] += r.nEE; s[DFK_WALKS_LONGEST] = std::max<uint64_t>(s[DFK_WALKS_LONGEST], r.nEE); s[DFK_WALKS_DUP_STEPS] += r.dup_steps;
        s[DFK_WALKS_SHORT] += r.status == SHORT; s[DFK_WALKS_TRIMMED] += r.trim > 0;
        if (q % 2 && r.placed && R->recs[q - 1].placed) ++s[DFK_WALKS_YIELDS];
    }
    s[DFK_WALKS_US] = (uint64_t)(1e6 * (wall_now() - t_in)); s[DFK_WALKS_US_COPY] = (uint64_t)(1e6 * times.s_copy); s[DFK_WALKS_US_DECODE] = (uint64_t)(1000.0f * (times.ms_decode + ms_lower));
    s[DFK_WALKS_US_SORT] = (uint64_t)(1000.0f * ms_sort); s[DFK_WALKS_US_WALK] = (uint64_t)(1000.0f * ms_walk); s[DFK_WALKS_SUM] = h_dg[0]; s[DFK_WALKS_XOR] = h_dg[1];
    TRACE("walks: %llu pairs, %llu walks, %llu placed of %llu entries, %llu bases walked in %llu steps (%llu duplicate), %llu on the host, %llu 48-mers, %llu reads decoded in %llu range(s), %llu batch(es); gather %.1f ms, decode and lowering %.1f ms, table %.1f ms, walks %.1f ms",
          (unsigned long long)n_pairs, (unsigned long long)s[DFK_WALKS_WALKS], (unsigned long long)s[DFK_WALKS_PLACED], (unsigned long long)s[DFK_WALKS_ENTRIES], (unsigned long long)s[DFK_WALKS_EE], (unsigned long long)n_steps,
          (unsigned long long)s[DFK_WALKS_DUP_STEPS], (unsigned long long)n_host, (unsigned long long)n_items_all, (unsigned long long)n_decoded, (unsigned long long)n_ranges, (unsigned long long)n_batches,
          1e3 * times.s_copy, times.ms_decode + ms_lower, ms_sort, ms_walk);
    return 0;
}

// the file into `dir`: whole, or not at all
int walks_write(const WalksResult* R, const std::string& dir)
{
    using namespace dfk_walks;
    const std::string path = dir + "/a.stack.walks";
    const uint64_t n = R->recs.size(), nl = R->locs.size();
    const std::vector<uint8_t> packed = pack_ee(R->ee);
    const int fd = open(path.c_str(), O_WRONLY | O_CREAT | O_TRUNC, 0666);
    if (fd < 0) return fail(DFK_E_ARG, "cannot open %s", path.c_str());
    const dfk_closer::BinHead h = dfk_closer::head_of(MAGIC, n);
    bool bad = pwrite_all(fd, &h, 16, 0) != 0 || pwrite_all(fd, R->starts.data(), 8 * (n + 1), 16) != 0 || pwrite_all(fd, R->ee_starts.data(), 8 * (n + 1), ee_starts_at(n)) != 0;
    if (!bad && n) bad = pwrite_all(fd, R->recs.data(), 32 * n, recs_at(n)) != 0;
    if (!bad && nl) bad = pwrite_all(fd, R->locs.data(), 16 * nl, locs_at(n)) != 0;
    if (!bad && !packed.empty()) bad = pwrite_all(fd, packed.data(), packed.size(), bases_at(n, nl)) != 0;
    if (close(fd) != 0) bad = true;
    if (bad) { (void)unlink(path.c_str()); return fail(DFK_E_ARG, "short write to %s", path.c_str()); }
    return 0;
}

// the latest dfk_walks_build*'s result: one a context, kept beside the graph
int walks_result_of(dfk_ctx* c, WalksResult** out)
{
    if (!c) return fail(DFK_E_ARG, "null context");
    if (!c->graph_state || !graph_of(c)->walks) return fail(DFK_E_STATE, "no stack walks: call dfk_walks_build or dfk_walks_build_arrays");
    *out = graph_of(c)->walks;
    return 0;
}
void walks_keep(dfk_ctx* c, WalksResult* R)
{
    HostGraph* G = graph_of(c);
    if (G->walks) walks_result_free(G->walks);
    G->walks = R; G->walks_free = walks_result_free;
}

int walks_reads(const uint8_t* packed, const uint64_t* base_off, const uint32_t* read_len, const uint8_t* pq, const uint64_t* pq_off, uint64_t n_reads, PartnerReads* reads)
{
    if (n_reads && (!packed || !read_len || !pq)) return fail(DFK_E_ARG, "null argument");
    if (!pq_off) return fail(DFK_E_ARG, "null argument");
    *reads = PartnerReads{packed, base_off, read_len, n_reads, {}};
    if (int rc = partner_reads_check(*reads)) return rc;
    if (int rc = cons_pq_check(pq_off, n_reads)) return rc;
    if (!base_off) reads->index_dense();
    return 0;
}

} // namespace

extern "C" {

int dfk_walks_build(dfk_ctx* c, const int32_t* pairs, uint64_t n_pairs, const uint8_t* packed, const uint64_t* base_off, const uint32_t* read_len, const uint8_t* pq, const uint64_t* pq_off, uint64_t n_reads)
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
    if (n_reads != P->n_reads) return fail(DFK_E_ARG, "walks: %llu reads given, %llu pathed", (unsigned long long)n_reads, (unsigned long long)P->n_reads);
    PartnerReads reads;
    if (int rc = walks_reads(packed, base_off, read_len, pq, pq_off, n_reads, &reads)) return rc;
    HIP_TRY(hipSetDevice(c->device));
    const HostGraph* G = graph_of(c);
    const CloserResult* C = P->closer;
    const std::vector<int32_t> inv = involution_of(G);
    // the bases of the closer edges, as a.fastb holds them (dfk_partners.inc: the graph keeps canonical edges only)
    const uint64_t n_ce = C->ce.size();
    std::vector<uint8_t> store, pk;
    std::vector<uint64_t> edge_at(std::max<uint64_t>(1, n_ce)); std::vector<int32_t> edge_len(std::max<uint64_t>(1, n_ce));
    for (uint64_t k = 0; k < n_ce; ++k) {
        if (C->ce[k] >= G->he.size()) return fail(DFK_E_STATE, "the closer sets name edge %llu: the graph has %llu", (unsigned long long)C->ce[k], (unsigned long long)G->he.size());
        packed_edge(*G, G->he[C->ce[k]], &pk);
        edge_at[k] = store.size(); edge_len[k] = (int32_t)(G->ce[G->he[C->ce[k]].ce].n + G->K - 1);
        store.insert(store.end(), pk.begin(), pk.end());
    }
    const int32_t none[2] = {0, 0};
    const WalksSource S{inv.size(), inv.data(), n_ce, C->ce.data(), store.data(), store.size(), edge_at.data(), edge_len.data(), C->read_first.data(), C->reads.data(), &reads, pq, pq_off};
    std::unique_ptr<WalksResult> R(new WalksResult);
    if (int rc = walks_build(c, S, n_pairs ? pairs : none, n_pairs, 0, R.get())) return rc;          // (refused: the earlier result is still served)
    R->pairs.assign(pairs, pairs + 2 * n_pairs);
    walks_keep(c, R.release());
    return 0;
    });
}

// The stage on host arrays: everything it reads is given, and checked here for the forms dfk_closer_fetch gives and a.fastb holds.
int dfk_walks_build_arrays(dfk_ctx* c, uint64_t n_edges, const int32_t* inv, const int32_t* kmers, const uint8_t* edge_packed, const uint64_t* edge_off, uint64_t n_ce, const uint64_t* ce,
                           const uint64_t* read_first, const uint64_t* reads, const int32_t* pairs, uint64_t n_pairs, const uint8_t* packed, const uint64_t* base_off, const uint32_t* read_len,
                           const uint8_t* pq, const uint64_t* pq_off, uint64_t n_reads, uint64_t walks_per_batch, const char* dir)
{
    return guarded([&]() -> int {
    if (!c) return fail(DFK_E_ARG, "null context");
    const uint64_t E = n_edges, N = n_reads;
    if ((E && (!inv || !kmers || !edge_packed)) || !edge_off || !read_first || (n_ce && !ce) || (n_pairs && !pairs)) return fail(DFK_E_ARG, "null argument");
    if (N >= (1ull << 31) || E >= (1ull << 31)) return fail(DFK_E_ARG, "%llu reads, %llu edges: 2^31 - 1 of each at most", (unsigned long long)N, (unsigned long long)E);
    const int64_t K = (int64_t)c->cfg.K;
    for (uint64_t e = 0; e < E; ++e) {
        if (inv[e] < 0 || (uint64_t)inv[e] >= E || inv[inv[e]] != (int32_t)e) return fail(DFK_E_ARG, "inv is not an involution at edge %llu", (unsigned long long)e);
        if (kmers[e] < 1 || kmers[e] > (1 << 30)) return fail(DFK_E_ARG, "edge %llu has %d k-mers", (unsigned long long)e, kmers[e]);
        if (edge_off[e + 1] < edge_off[e] || edge_off[e + 1] - edge_off[e] < ((uint64_t)(kmers[e] + K - 1) + 3) / 4) return fail(DFK_E_ARG, "the edges' offset table leaves edge %llu fewer bytes than its bases need", (unsigned long long)e);
    }
    if (read_first[0] != 0) return fail(DFK_E_ARG, "the tables do not start at 0");
    for (uint64_t k = 0; k < n_ce; ++k) {
        if (ce[k] >= E || (k && ce[k] <= ce[k - 1])) return fail(DFK_E_ARG, "the closer edges are not ascending edges of the graph at rank %llu", (unsigned long long)k);
        if (read_first[k + 1] < read_first[k]) return fail(DFK_E_ARG, "the sets' starts fall at rank %llu", (unsigned long long)k);
        for (uint64_t j = read_first[k]; reads && j + 1 < read_first[k + 1]; ++j) if (reads[j + 1] <= reads[j]) return fail(DFK_E_ARG, "the set of rank %llu is not ascending and distinct", (unsigned long long)k);
    }
    if (read_first[n_ce] && !reads) return fail(DFK_E_ARG, "null argument");
    PartnerReads rd;
    if (int rc = walks_reads(packed, base_off, read_len, pq, pq_off, N, &rd)) return rc;
    HIP_TRY(hipSetDevice(c->device));
    std::vector<uint64_t> edge_at(std::max<uint64_t>(1, n_ce)); std::vector<int32_t> edge_len(std::max<uint64_t>(1, n_ce));
    for (uint64_t k = 0; k < n_ce; ++k) { edge_at[k] = edge_off[ce[k]]; edge_len[k] = (int32_t)(kmers[ce[k]] + K - 1); }
    const int32_t none[2] = {0, 0};
    const uint64_t zero = 0;
    const WalksSource S{E, inv, n_ce, ce, edge_packed, E ? edge_off[E] : 0, edge_at.data(), edge_len.data(), read_first, reads ? reads : &zero, &rd, pq, pq_off};
    std::unique_ptr<WalksResult> R(new WalksResult);
    if (int rc = walks_build(c, S, n_pairs ? pairs : none, n_pairs, walks_per_batch, R.get())) return rc;
    if (dir) if (int rc = walks_write(R.get(), dir)) return rc;
    walks_keep(c, R.release());
    return 0;
    });
}

int dfk_walks_stats(dfk_ctx* c, uint64_t* out)
{
    return guarded([&]() -> int {
    WalksResult* R = nullptr;
    if (int rc = walks_result_of(c, &R)) return rc;
    if (!out) return fail(DFK_E_ARG, "null argument");
    for (int i = 0; i < DFK_WALKS_WORDS; ++i) out[i] = R->stats[i];
    return 0;
    });
}

int dfk_walks_fetch(dfk_ctx* c, uint64_t* starts, uint64_t* ee_starts, uint32_t* records, uint64_t* n_walks, void* placed, uint64_t placed_cap, uint64_t* n_placed, uint8_t* bases, uint64_t bases_cap, uint64_t* n_bases)
{
    return guarded([&]() -> int {
    WalksResult* R = nullptr;
    if (int rc = walks_result_of(c, &R)) return rc;
    const uint64_t n = R->recs.size(), nl = R->locs.size(), nb = R->ee.size();
    if (n_walks) *n_walks = n;
    if (n_placed) *n_placed = nl;
    if (n_bases) *n_bases = nb;
    if ((placed || placed_cap) && placed_cap < nl) return fail(DFK_E_ARG, "buffer too small: %llu < %llu placed records", (unsigned long long)placed_cap, (unsigned long long)nl);
    if ((bases || bases_cap) && bases_cap < nb) return fail(DFK_E_ARG, "buffer too small: %llu < %llu walked bases", (unsigned long long)bases_cap, (unsigned long long)nb);
    if ((placed_cap && nl && !placed) || (bases_cap && nb && !bases)) return fail(DFK_E_ARG, "null argument");
    if (placed && nl) memcpy(placed, R->locs.data(), 16 * nl);
    if (bases && nb) memcpy(bases, R->ee.data(), nb);
    if (starts) memcpy(starts, R->starts.data(), 8 * (n + 1));                   // room for n_walks + 1 words
    if (ee_starts) memcpy(ee_starts, R->ee_starts.data(), 8 * (n + 1));
    if (records && n) memcpy(records, R->recs.data(), 32 * n);                   // room for 8 * n_walks u32
    return 0;
    });
}

int dfk_walks_write(dfk_ctx* c, const char* dir)
{
    return guarded([&]() -> int {
    WalksResult* R = nullptr;
    if (int rc = walks_result_of(c, &R)) return rc;
    if (!dir) return fail(DFK_E_ARG, "null directory");
    return walks_write(R, dir);
    });
}

} // extern "C"
