// superplus_amd/csrc/dfk_closer.inc -- the closers' read sets per edge (CloseGap2, 10X/Closomatic.cc:503-552; Stackster,
// 10X/Stackster.cc:289-324) and the files a.close.edges, a.close.locs, a.close.anchors, a.close.reads, included by dfk.hip.
//
// The rule, the plan and the files' layouts: dfk_closer.h.  The kernels: dfk_closer_kernels.h.  Here: closer_build() -- the
// marks, ce, the weights per rank, then a range of ranks at a time one sweep of the batches, the sorts and the compactions, each
// range's records leaving for the host as they are made -- and closer_write(), which puts the host's copy into the four files.
// Everything on the device comes from the arena and goes back before either returns; neither table is ever whole on the device.
#include "dfk_closer_kernels.h"

namespace {

struct CloserResult {
    uint64_t n_edges = 0, n_reads = 0;
    std::vector<uint64_t> ce, loc_first, anchor_first, read_first;   // [n_ce], [n_ce + 1] x 3
    std::vector<uint64_t> locs;                                      // two words a record
    std::vector<uint32_t> anchors;                                   // three words a record
    std::vector<uint64_t> reads;
    uint64_t stats[DFK_CLOSER_WORDS] = {};
};
void closer_result_free(CloserResult* r) { delete r; }

struct CloserSource { const std::vector<PathBatch>* batches; uint64_t n_reads, n_edges; const int32_t* inv; const int32_t* kmers; int32_t K; };

int closer_build(dfk_ctx* c, const CloserSource& S, const int32_t* pairs, uint64_t n_pairs, const uint8_t* dup, CloserResult* R)
{
    using namespace dfk_closer;
    const uint64_t N = S.n_reads, E = S.n_edges;
    if (N % 2) return fail(DFK_E_ARG, "%llu reads: the closers take a read's mate as id ^ 1", (unsigned long long)N);
    if (N > (1ull << 31)) return fail(DFK_E_ARG, "%llu reads: a set entry keeps id << 1 | fw in 32 bits while it is sorted", (unsigned long long)N);
    if (E >= (1ull << 31)) return fail(DFK_E_ARG, "%llu edges", (unsigned long long)E);
    if ((n_pairs && !pairs) || !dup) return fail(DFK_E_ARG, "null argument");
    for (uint64_t i = 0; i < 2 * n_pairs; ++i)
        if (pairs[i] < 0 || (uint64_t)pairs[i] >= E) return fail(DFK_E_ARG, "pair %llu names edge %d: the graph has %llu", (unsigned long long)(i / 2), pairs[i], (unsigned long long)E);
    const unsigned cus = (unsigned)c->prop.multiProcessorCount;
    const double t_in = wall_now();
    const uint64_t mark = c->alloc_seq;
    R->n_edges = E; R->n_reads = N;
    float ms_mark = 0, ms_weigh = 0, ms_sweep = 0, ms_sort = 0;
    uint64_t h_ctr[4] = {}, h_dg[16] = {}, n_ce = 0, n_ranges = 0, n_prec = 0;
    auto body = [&]() -> int {
        int rc;
        Timer tm(c->stream);
        DevBuf d_pairs, d_inv, d_kmers, d_dup, d_marks, flags, rank, rank_of, d_ce, dg, ctr, d_w;
        // ---- marks, their ranks, ce
        tm.start();
        if ((rc = c->alloc(d_marks, std::max<uint64_t>(1, dfk_subset::mark_words(E)) * 4, "closer edges", Place::Low)) || (rc = c->alloc(rank_of, std::max<uint64_t>(1, E) * 4, "ranks of the closer edges", Place::Low)) ||
            (rc = c->alloc(dg, 128, "closer digests", Place::Low)) || (rc = c->alloc(ctr, 32, "closer counters", Place::Low)) ||
            (rc = c->alloc(d_inv, std::max<uint64_t>(1, E) * 4, "involution", Place::Low)) || (rc = c->alloc(d_kmers, std::max<uint64_t>(1, E) * 4, "edge k-mers", Place::Low)) ||
            (rc = c->alloc(d_dup, std::max<uint64_t>(1, N / 2), "duplicate marks", Place::Low)) ||
            (rc = c->alloc(flags, (E + 1) * 8, "edge flags", Place::Low)) || (rc = c->alloc(rank, (E + 1) * 8, "edge ranks", Place::Low))) return rc;
        HIP_TRY(hipMemsetAsync(d_marks.p, 0, std::max<uint64_t>(1, dfk_subset::mark_words(E)) * 4, c->stream));
        HIP_TRY(hipMemsetAsync(dg.p, 0, 128, c->stream));
        HIP_TRY(hipMemsetAsync(ctr.p, 0, 32, c->stream));
        if (E) {
            HIP_TRY(hipMemcpyAsync(d_inv.p, S.inv, E * 4, hipMemcpyHostToDevice, c->stream));
            HIP_TRY(hipMemcpyAsync(d_kmers.p, S.kmers, E * 4, hipMemcpyHostToDevice, c->stream));
        }
        if (N) HIP_TRY(hipMemcpyAsync(d_dup.p, dup, N / 2, hipMemcpyHostToDevice, c->stream));
        if (n_pairs) {
            if ((rc = c->alloc(d_pairs, n_pairs * 8, "edge pairs", Place::Low))) return rc;
            HIP_TRY(hipMemcpyAsync(d_pairs.p, pairs, n_pairs * 8, hipMemcpyHostToDevice, c->stream));
            hipLaunchKernelGGL(k_cl_mark, dim3(grid_256(n_pairs, cus)), dim3(256), 0, c->stream, (const int32_t*)d_pairs.p, n_pairs, (const int32_t*)d_inv.p, (uint32_t*)d_marks.p);
        }
        hipLaunchKernelGGL(k_sub_flags, dim3(grid_256(E + 1, cus)), dim3(256), 0, c->stream, (const uint32_t*)d_marks.p, E, (uint64_t*)flags.p);
        HIP_TRY(hipGetLastError());
        if ((rc = device_scan(c, (const uint64_t*)flags.p, (uint64_t*)rank.p, E + 1))) return rc;
        HIP_TRY(hipMemcpyAsync(&n_ce, (const uint64_t*)rank.p + E, 8, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
        if (n_ce > E || n_ce > 2 * n_pairs) return fail(DFK_E_HIP, "closer: %llu closer edges from %llu pairs among %llu edges", (unsigned long long)n_ce, (unsigned long long)n_pairs, (unsigned long long)E);
        if ((rc = c->alloc(d_ce, std::max<uint64_t>(1, n_ce) * 8, "closer edges, ascending", Place::Low))) return rc;
        if (E) hipLaunchKernelGGL(k_sub_eoi, dim3(grid_256(E, cus)), dim3(256), 0, c->stream, (const uint32_t*)d_marks.p, (const uint64_t*)rank.p, E, (uint64_t*)d_ce.p, (uint32_t*)rank_of.p);
        if (n_ce) hipLaunchKernelGGL(HIP_KERNEL_NAME(k_digest_seq<uint64_t>), dim3(grid_256(n_ce, cus)), dim3(256), 0, c->stream, (const uint64_t*)d_ce.p, n_ce, SALT_EDGES, (unsigned long long*)dg.p);
        HIP_TRY(hipGetLastError());
        R->ce.assign(n_ce, 0);
        if (n_ce) HIP_TRY(hipMemcpyAsync(R->ce.data(), d_ce.p, n_ce * 8, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
        c->release(flags); c->release(rank); c->release(d_ce);
        if (n_pairs) c->release(d_pairs);
        ms_mark = tm.stop();
        R->loc_first.assign(1, 0); R->anchor_first.assign(1, 0); R->read_first.assign(1, 0);
        if (!n_ce) return 0;
        const Tables T{(const uint32_t*)d_marks.p, (const uint32_t*)rank_of.p, (const int32_t*)d_inv.p, (const int32_t*)d_kmers.p};
        auto batch_of = [&](const PathBatch& b) { return ClBatch{(const uint32_t*)b.var.p, (const uint32_t*)b.elem_off.p, b.n, b.r0, b.var_bytes, (const uint8_t*)d_dup.p}; };
        // ---- the weights per rank: what each closer edge's sweep will emit
        tm.start();
        std::vector<uint64_t> w(3 * n_ce, 0);
        if ((rc = c->alloc(d_w, 3 * n_ce * 8, "weights per closer edge", Place::Low))) return rc;
        HIP_TRY(hipMemsetAsync(d_w.p, 0, 3 * n_ce * 8, c->stream));
        for (const PathBatch& b : *S.batches)
            if (b.n) hipLaunchKernelGGL(k_cl_weigh, dim3(grid_256(b.n, cus)), dim3(256), 0, c->stream, batch_of(b), T, (uint32_t)n_ce, S.K, (unsigned long long*)d_w.p, (unsigned long long*)ctr.p);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(w.data(), d_w.p, 3 * n_ce * 8, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipMemcpyAsync(h_ctr, ctr.p, 32, hipMemcpyDeviceToHost, c->stream));
        ms_weigh = tm.stop();
        c->release(d_w);
        std::vector<uint64_t> weight(n_ce), nl(n_ce), np(n_ce), ne(n_ce);
        for (uint64_t k = 0; k < n_ce; ++k) {
            nl[k] = w[3 * k]; np[k] = w[3 * k + 1]; ne[k] = w[3 * k + 2]; weight[k] = nl[k] + np[k] + ne[k]; n_prec += np[k];
            if (weight[k] >= (1ull << 32)) return fail(DFK_E_ARG, "edge %llu alone gives %llu records: a range of the closers' tables sorts 32-bit positions", (unsigned long long)R->ce[k], (unsigned long long)weight[k]);
        }
        const std::vector<uint64_t> wfirst = prefix_sums(weight.data(), n_ce), lfirst = prefix_sums(nl.data(), n_ce), pfirst = prefix_sums(np.data(), n_ce), efirst = prefix_sums(ne.data(), n_ce);
        R->loc_first = lfirst;
        R->locs.resize(2 * lfirst[n_ce]);
        // ---- a range of ranks at a time
        const uint64_t cap = range_cap(c->largest_allocatable(), path_switches().pidx_range_pairs);
        uint64_t anchors_done = 0, reads_done = 0;
        for (uint64_t k0 = 0; k0 < n_ce;) {
            const PidxRange range = next_range(wfirst.data(), n_ce, k0, cap);
            const uint64_t k1 = range.e1, nk = k1 - k0;
            if (!range.ok) return fail(DFK_E_ARG, "edge %llu alone gives %llu records: a range of the closers' tables sorts 32-bit positions", (unsigned long long)R->ce[k0], (unsigned long long)range.n);
            ++n_ranges;
            const uint64_t n_l = lfirst[k1] - lfirst[k0], n_p = pfirst[k1] - pfirst[k0], n_e = efirst[k1] - efirst[k0];
            std::vector<uint64_t> na(nk, 0), nr(nk, 0);
            if (n_l) {
                const uint64_t rmark = c->alloc_seq;
                DevBuf lk[2], lv[2], lid, lpos, pk, pg, pa, ek[2], ew[2], per_rank;
                auto u32s = [&](DevBuf& d, uint64_t n, const char* what) { return c->alloc(d, std::max<uint64_t>(1, n) * 4, what, Place::Low); };
                if ((rc = u32s(lk[0], n_l, "record keys")) || (rc = u32s(lv[0], n_l, "record places")) || (rc = u32s(lid, n_l, "record ids")) || (rc = u32s(lpos, n_l, "record positions")) ||
                    (rc = u32s(pk, n_p, "prec ranks")) || (rc = u32s(pg, n_p, "prec edges")) || (rc = u32s(pa, n_p, "prec distances")) ||
                    (rc = u32s(ek[0], n_e, "set ranks")) || (rc = u32s(ew[0], n_e, "set entries")) || (rc = c->alloc(per_rank, 2 * nk * 8, "anchors and set entries per rank", Place::Low))) return rc;
                HIP_TRY(hipMemsetAsync(per_rank.p, 0, 2 * nk * 8, c->stream));
                const ClStreams St{(uint32_t*)lk[0].p, (uint32_t*)lv[0].p, (uint32_t*)lid.p, (int32_t*)lpos.p, (uint32_t*)pk.p, (uint32_t*)pg.p, (uint32_t*)pa.p, (uint32_t*)ek[0].p, (uint32_t*)ew[0].p};
                // the sweep: every batch once, three scans a batch
                tm.start();
                uint64_t base_l = 0, base_p = 0, base_e = 0;
                for (const PathBatch& b : *S.batches) {
                    if (!b.n) continue;
                    DevBuf cnt[3], at[3];
                    for (int i = 0; i < 3; ++i) if ((rc = c->alloc(cnt[i], (b.n + 1) * 8, "records per read", Place::Low)) || (rc = c->alloc(at[i], (b.n + 1) * 8, "their places", Place::Low))) return rc;
                    hipLaunchKernelGGL(k_cl_count, dim3(grid_reads(b.n, cus)), dim3(256), 0, c->stream, batch_of(b), T, (uint32_t)k0, (uint32_t)k1, S.K, (uint64_t*)cnt[0].p, (uint64_t*)cnt[1].p, (uint64_t*)cnt[2].p);
                    HIP_TRY(hipGetLastError());
                    uint64_t got[3] = {};
                    for (int i = 0; i < 3; ++i) {
                        if ((rc = device_scan(c, (const uint64_t*)cnt[i].p, (uint64_t*)at[i].p, b.n + 1))) return rc;
                        HIP_TRY(hipMemcpyAsync(&got[i], (const uint64_t*)at[i].p + b.n, 8, hipMemcpyDeviceToHost, c->stream));
                    }
                    HIP_TRY(hipStreamSynchronize(c->stream));
                    if (base_l + got[0] > n_l || base_p + got[1] > n_p || base_e + got[2] > n_e)
                        return fail(DFK_E_HIP, "closer: more records listed for ranks [%llu, %llu) than the weights counted", (unsigned long long)k0, (unsigned long long)k1);
                    if (got[0]) hipLaunchKernelGGL(k_cl_emit, dim3(grid_256(b.n, cus)), dim3(256), 0, c->stream, batch_of(b), T, (uint32_t)k0, (uint32_t)k1, S.K, (const uint64_t*)at[0].p, (const uint64_t*)at[1].p,
                                                   (const uint64_t*)at[2].p, base_l, base_p, base_e, St);
                    HIP_TRY(hipGetLastError());
                    HIP_TRY(hipStreamSynchronize(c->stream));
                    for (int i = 2; i >= 0; --i) { c->release(at[i]); c->release(cnt[i]); }
                    base_l += got[0]; base_p += got[1]; base_e += got[2];
                }
                if (base_l != n_l || base_p != n_p || base_e != n_e)
                    return fail(DFK_E_HIP, "closer: %llu + %llu + %llu records listed for ranks [%llu, %llu), the weights counted %llu + %llu + %llu", (unsigned long long)base_l, (unsigned long long)base_p,
                                (unsigned long long)base_e, (unsigned long long)k0, (unsigned long long)k1, (unsigned long long)n_l, (unsigned long long)n_p, (unsigned long long)n_e);
                ms_sweep += tm.stop();
                tm.start();
                // locs: a stable sort by (rank, pass) of the records' places, then the records as the file holds them
                {
                    const uint64_t lmark = c->alloc_seq;
                    DevBuf out;
                    if ((rc = u32s(lk[1], n_l, "record keys")) || (rc = u32s(lv[1], n_l, "record places"))) return rc;
                    int cur = 0;
                    if ((rc = radix_sort_pairs(c, lk, lv, n_l, loc_key_bits(nk), &cur))) return rc;
                    if ((rc = c->alloc(out, n_l * 16, "a.close.locs records", Place::Low))) return rc;
                    hipLaunchKernelGGL(k_cl_loc_records, dim3(grid_256(n_l, cus)), dim3(256), 0, c->stream, (const uint32_t*)lk[cur].p, (const uint32_t*)lv[cur].p, (const uint32_t*)lid.p, (const int32_t*)lpos.p, n_l, (uint64_t*)out.p);
                    hipLaunchKernelGGL(HIP_KERNEL_NAME(k_digest_seq<uint64_t>), dim3(grid_256(2 * n_l, cus)), dim3(256), 0, c->stream, (const uint64_t*)out.p, 2 * n_l, SALT_LOCS + 2 * lfirst[k0], (unsigned long long*)dg.p + 4);
                    HIP_TRY(hipGetLastError());
                    HIP_TRY(hipMemcpyAsync(R->locs.data() + 2 * lfirst[k0], out.p, n_l * 16, hipMemcpyDeviceToHost, c->stream));
                    HIP_TRY(hipStreamSynchronize(c->stream));
                    c->release_since(lmark);
                }
                // anchors: prec sorted by (rank, g, add), least significant field first; the runs of 5 and more
                if (n_p) {
                    const uint64_t amark = c->alloc_seq;
                    DevBuf k[2], v[2], sk, sg, sa, fl, run, heads, keep, place, out;
                    for (int i = 0; i < 2; ++i) if ((rc = u32s(k[i], n_p, "prec keys")) || (rc = u32s(v[i], n_p, "prec places"))) return rc;
                    const unsigned g = grid_256(n_p, cus);
                    int cur = 0;
                    HIP_TRY(hipMemcpyAsync(k[0].p, pa.p, n_p * 4, hipMemcpyDeviceToDevice, c->stream));
                    hipLaunchKernelGGL(k_cl_iota, dim3(g), dim3(256), 0, c->stream, (uint32_t*)v[0].p, n_p);
                    HIP_TRY(hipGetLastError());
                    if ((rc = radix_sort_pairs(c, k, v, n_p, 32, &cur))) return rc;
                    hipLaunchKernelGGL(k_cl_gather, dim3(g), dim3(256), 0, c->stream, (const uint32_t*)pg.p, (const uint32_t*)v[cur].p, n_p, (uint32_t*)k[cur].p);
                    HIP_TRY(hipGetLastError());
                    if ((rc = radix_sort_pairs(c, k, v, n_p, bits_for(E), &cur))) return rc;
                    hipLaunchKernelGGL(k_cl_gather, dim3(g), dim3(256), 0, c->stream, (const uint32_t*)pk.p, (const uint32_t*)v[cur].p, n_p, (uint32_t*)k[cur].p);
                    HIP_TRY(hipGetLastError());
                    if ((rc = radix_sort_pairs(c, k, v, n_p, bits_for(nk), &cur))) return rc;
                    if ((rc = u32s(sk, n_p, "prec ranks, sorted")) || (rc = u32s(sg, n_p, "prec edges, sorted")) || (rc = u32s(sa, n_p, "prec distances, sorted")) ||
                        (rc = c->alloc(fl, (n_p + 1) * 8, "run heads", Place::Low)) || (rc = c->alloc(run, (n_p + 1) * 8, "run numbers", Place::Low))) return rc;
                    hipLaunchKernelGGL(k_cl_gather, dim3(g), dim3(256), 0, c->stream, (const uint32_t*)pk.p, (const uint32_t*)v[cur].p, n_p, (uint32_t*)sk.p);
                    hipLaunchKernelGGL(k_cl_gather, dim3(g), dim3(256), 0, c->stream, (const uint32_t*)pg.p, (const uint32_t*)v[cur].p, n_p, (uint32_t*)sg.p);
                    hipLaunchKernelGGL(k_cl_gather, dim3(g), dim3(256), 0, c->stream, (const uint32_t*)pa.p, (const uint32_t*)v[cur].p, n_p, (uint32_t*)sa.p);
                    hipLaunchKernelGGL(k_cl_heads, dim3(grid_256(n_p + 1, cus)), dim3(256), 0, c->stream, (const uint32_t*)sk.p, (const uint32_t*)sg.p, (const uint32_t*)sa.p, n_p, (uint64_t*)fl.p);
                    HIP_TRY(hipGetLastError());
                    if ((rc = device_scan(c, (const uint64_t*)fl.p, (uint64_t*)run.p, n_p + 1))) return rc;
                    uint64_t n_runs = 0, kept = 0;
                    HIP_TRY(hipMemcpyAsync(&n_runs, (const uint64_t*)run.p + n_p, 8, hipMemcpyDeviceToHost, c->stream));
                    HIP_TRY(hipStreamSynchronize(c->stream));
                    if (!n_runs || n_runs > n_p) return fail(DFK_E_HIP, "closer: %llu runs among %llu prec tuples", (unsigned long long)n_runs, (unsigned long long)n_p);
                    if ((rc = c->alloc(heads, (n_runs + 1) * 8, "run starts", Place::Low)) || (rc = c->alloc(keep, (n_runs + 1) * 8, "runs kept", Place::Low)) || (rc = c->alloc(place, (n_runs + 1) * 8, "their places", Place::Low))) return rc;
                    hipLaunchKernelGGL(k_cl_run_starts, dim3(grid_256(n_p + 1, cus)), dim3(256), 0, c->stream, (const uint64_t*)fl.p, (const uint64_t*)run.p, n_p, (uint64_t*)heads.p);
                    hipLaunchKernelGGL(k_cl_keep, dim3(grid_256(n_runs + 1, cus)), dim3(256), 0, c->stream, (const uint64_t*)heads.p, n_runs, (uint64_t*)keep.p);
                    HIP_TRY(hipGetLastError());
                    if ((rc = device_scan(c, (const uint64_t*)keep.p, (uint64_t*)place.p, n_runs + 1))) return rc;
                    HIP_TRY(hipMemcpyAsync(&kept, (const uint64_t*)place.p + n_runs, 8, hipMemcpyDeviceToHost, c->stream));
                    HIP_TRY(hipStreamSynchronize(c->stream));
                    if (kept > n_runs) return fail(DFK_E_HIP, "closer: %llu anchors among %llu runs", (unsigned long long)kept, (unsigned long long)n_runs);
                    if (kept) {
                        if ((rc = c->alloc(out, kept * 12, "a.close.anchors records", Place::Low))) return rc;
                        hipLaunchKernelGGL(k_cl_anchors, dim3(grid_256(n_runs, cus)), dim3(256), 0, c->stream, (const uint64_t*)heads.p, (const uint64_t*)keep.p, (const uint64_t*)place.p, n_runs,
                                           (const uint32_t*)sk.p, (const uint32_t*)sg.p, (const uint32_t*)sa.p, (uint32_t*)out.p, (unsigned long long*)per_rank.p);
                        hipLaunchKernelGGL(HIP_KERNEL_NAME(k_digest_seq<uint32_t>), dim3(grid_256(3 * kept, cus)), dim3(256), 0, c->stream, (const uint32_t*)out.p, 3 * kept, SALT_ANCHORS + 3 * anchors_done, (unsigned long long*)dg.p + 8);
                        HIP_TRY(hipGetLastError());
                        R->anchors.resize(3 * (anchors_done + kept));
                        HIP_TRY(hipMemcpyAsync(R->anchors.data() + 3 * anchors_done, out.p, kept * 12, hipMemcpyDeviceToHost, c->stream));
                        HIP_TRY(hipMemcpyAsync(na.data(), per_rank.p, nk * 8, hipMemcpyDeviceToHost, c->stream));
                        HIP_TRY(hipStreamSynchronize(c->stream));
                        anchors_done += kept;
                    }
                    c->release_since(amark);
                }
                // reads: sorted by (rank, id << 1 | fw), the distinct ones
                if (n_e) {
                    const uint64_t smark = c->alloc_seq;
                    DevBuf fl, place, out;
                    if ((rc = u32s(ek[1], n_e, "set ranks")) || (rc = u32s(ew[1], n_e, "set entries"))) return rc;
                    // (by the entry first, the rank its value; then by the rank, the entry its value)
                    DevBuf a[2] = {ew[0], ew[1]}, b[2] = {ek[0], ek[1]};
                    int cur = 0;
                    if ((rc = radix_sort_pairs(c, a, b, n_e, bits_for(2 * std::max<uint64_t>(1, N)), &cur))) return rc;
                    DevBuf b2[2] = {b[cur], b[cur ^ 1]}, a2[2] = {a[cur], a[cur ^ 1]};
                    cur = 0;
                    if ((rc = radix_sort_pairs(c, b2, a2, n_e, bits_for(nk), &cur))) return rc;
                    if ((rc = c->alloc(fl, (n_e + 1) * 8, "distinct entries", Place::Low)) || (rc = c->alloc(place, (n_e + 1) * 8, "their places", Place::Low))) return rc;
                    hipLaunchKernelGGL(k_cl_heads, dim3(grid_256(n_e + 1, cus)), dim3(256), 0, c->stream, (const uint32_t*)b2[cur].p, (const uint32_t*)a2[cur].p, (const uint32_t*)nullptr, n_e, (uint64_t*)fl.p);
                    HIP_TRY(hipGetLastError());
                    if ((rc = device_scan(c, (const uint64_t*)fl.p, (uint64_t*)place.p, n_e + 1))) return rc;
                    uint64_t kept = 0;
                    HIP_TRY(hipMemcpyAsync(&kept, (const uint64_t*)place.p + n_e, 8, hipMemcpyDeviceToHost, c->stream));
                    HIP_TRY(hipStreamSynchronize(c->stream));
                    if (!kept || kept > n_e) return fail(DFK_E_HIP, "closer: %llu distinct among %llu set entries", (unsigned long long)kept, (unsigned long long)n_e);
                    if ((rc = c->alloc(out, kept * 8, "a.close.reads records", Place::Low))) return rc;
                    hipLaunchKernelGGL(k_cl_reads_out, dim3(grid_256(n_e, cus)), dim3(256), 0, c->stream, (const uint64_t*)fl.p, (const uint64_t*)place.p, (const uint32_t*)b2[cur].p, (const uint32_t*)a2[cur].p, n_e,
                                       (uint64_t*)out.p, (unsigned long long*)per_rank.p + nk);
                    hipLaunchKernelGGL(HIP_KERNEL_NAME(k_digest_seq<uint64_t>), dim3(grid_256(kept, cus)), dim3(256), 0, c->stream, (const uint64_t*)out.p, kept, SALT_READS + reads_done, (unsigned long long*)dg.p + 12);
                    HIP_TRY(hipGetLastError());
                    R->reads.resize(reads_done + kept);
                    HIP_TRY(hipMemcpyAsync(R->reads.data() + reads_done, out.p, kept * 8, hipMemcpyDeviceToHost, c->stream));
                    HIP_TRY(hipMemcpyAsync(nr.data(), (const uint64_t*)per_rank.p + nk, nk * 8, hipMemcpyDeviceToHost, c->stream));
                    HIP_TRY(hipStreamSynchronize(c->stream));
                    reads_done += kept;
                    c->release_since(smark);
                }
                ms_sort += tm.stop();
                c->release_since(rmark);
            }
            for (uint64_t k = 0; k < nk; ++k) { R->anchor_first.push_back(R->anchor_first.back() + na[k]); R->read_first.push_back(R->read_first.back() + nr[k]); }
            k0 = k1;
        }
        if (R->anchor_first.back() != anchors_done || R->read_first.back() != reads_done) return fail(DFK_E_HIP, "closer: the per-rank counts do not add up to the records");
        HIP_TRY(hipMemcpyAsync(h_dg, dg.p, 128, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
        return 0;
    };
    int rc;
    try { rc = body(); } catch (const std::runtime_error& e) { rc = fail(DFK_E_HIP, "%s", e.what()); }
    (void)hipStreamSynchronize(c->stream);
    c->release_since(mark);
    if (rc) return rc;
    uint64_t* s = R->stats;
    s[DFK_CLOSER_N_EDGES] = n_ce; s[DFK_CLOSER_N_LOCS] = R->locs.size() / 2; s[DFK_CLOSER_N_ANCHORS] = R->anchors.size() / 3; s[DFK_CLOSER_N_READS] = R->reads.size();
    s[DFK_CLOSER_PREC] = n_prec; s[DFK_CLOSER_MATES_IN] = h_ctr[0]; s[DFK_CLOSER_MATES_OUT] = h_ctr[1]; s[DFK_CLOSER_DUP_SKIPPED] = h_ctr[2]; s[DFK_CLOSER_RANGES] = n_ranges;
    s[DFK_CLOSER_US] = (uint64_t)(1e6 * (wall_now() - t_in)); s[DFK_CLOSER_US_MARK] = (uint64_t)(1000.0f * ms_mark); s[DFK_CLOSER_US_WEIGH] = (uint64_t)(1000.0f * ms_weigh);
    s[DFK_CLOSER_US_SWEEP] = (uint64_t)(1000.0f * ms_sweep); s[DFK_CLOSER_US_SORT] = (uint64_t)(1000.0f * ms_sort);
    for (int i = 0; i < 4; ++i) { s[DFK_CLOSER_EDGES_SUM + 2 * i] = h_dg[4 * i]; s[DFK_CLOSER_EDGES_SUM + 2 * i + 1] = h_dg[4 * i + 1]; }
    TRACE("closer: %llu closer edges, %llu locs, %llu prec tuples, %llu anchors, %llu set entries in %llu range(s); marks %.1f ms, weights %.1f ms, sweeps %.1f ms, sorts %.1f ms",
          (unsigned long long)n_ce, (unsigned long long)s[DFK_CLOSER_N_LOCS], (unsigned long long)n_prec, (unsigned long long)s[DFK_CLOSER_N_ANCHORS], (unsigned long long)s[DFK_CLOSER_N_READS],
          (unsigned long long)n_ranges, ms_mark, ms_weigh, ms_sweep, ms_sort);
    return 0;
}

// the four files into `dir`: all of them, or none
int closer_write(const CloserResult* R, const std::string& dir)
{
    using namespace dfk_closer;
    const char* names[4] = {"a.close.edges", "a.close.locs", "a.close.anchors", "a.close.reads"};
    const char* magic[4] = {MAGIC_EDGES, MAGIC_LOCS, MAGIC_ANCHORS, MAGIC_READS};
    const uint64_t n = R->ce.size();
    const std::vector<uint64_t>* starts[4] = {nullptr, &R->loc_first, &R->anchor_first, &R->read_first};
    const void* rec[4] = {R->ce.data(), R->locs.data(), R->anchors.data(), R->reads.data()};
    const uint64_t rec_bytes[4] = {8 * n, 8 * (uint64_t)R->locs.size(), 4 * (uint64_t)R->anchors.size(), 8 * (uint64_t)R->reads.size()};
    std::string path[4]; int fd[4] = {-1, -1, -1, -1};
    int rc = 0;
    for (int i = 0; i < 4 && !rc; ++i) {
        path[i] = dir + "/" + names[i];
        fd[i] = open(path[i].c_str(), O_WRONLY | O_CREAT | O_TRUNC, 0666);
        if (fd[i] < 0) { rc = fail(DFK_E_ARG, "cannot open %s", path[i].c_str()); break; }
        const BinHead h = head_of(magic[i], n);
        uint64_t at = 16;
        bool bad = pwrite_all(fd[i], &h, 16, 0) != 0;
        if (!bad && starts[i]) { bad = pwrite_all(fd[i], starts[i]->data(), 8 * (n + 1), at) != 0; at += 8 * (n + 1); }
        if (!bad && rec_bytes[i]) bad = pwrite_all(fd[i], rec[i], rec_bytes[i], at) != 0;
        if (bad) rc = fail(DFK_E_ARG, "short write to %s", path[i].c_str());
    }
    const std::string first_err = rc ? g_err : std::string();
    for (int i = 0; i < 4; ++i)
        if (fd[i] >= 0 && close(fd[i]) != 0 && !rc) rc = fail(DFK_E_ARG, "short write to %s", path[i].c_str());
    if (rc) {
        for (int i = 0; i < 4; ++i) if (fd[i] >= 0) (void)unlink(path[i].c_str());
        return first_err.empty() ? rc : fail(rc, "%s", first_err.c_str());
    }
    return 0;
}

void closer_drop_arrays(dfk_ctx* c)
{
    HostGraph* G = graph_of(c);
    if (G->closer_arrays) { closer_result_free(G->closer_arrays); G->closer_arrays = nullptr; }
}

// the latest build's result: dfk_closer_build_arrays keeps its own beside the graph until the next build of either kind
int closer_result_of(dfk_ctx* c, CloserResult** out)
{
    if (!c) return fail(DFK_E_ARG, "null context");
    if (c->graph_state && graph_of(c)->closer_arrays) { *out = graph_of(c)->closer_arrays; return 0; }
    PathState* P = built_paths(c);
    if (!P) return fail(DFK_E_STATE, "no closer sets: call dfk_paths_build and dfk_closer_build");
    if (!P->closer) return fail(DFK_E_STATE, "no closer sets: call dfk_closer_build");
    *out = P->closer;
    return 0;
}

} // namespace

extern "C" {

int dfk_closer_build(dfk_ctx* c, const int32_t* pairs, uint64_t n_pairs, const uint8_t* dup)
{
    return guarded([&]() -> int {
    if (!c) return fail(DFK_E_ARG, "null context");
    PathState* P = built_paths(c);
    if (!P) return fail(DFK_E_STATE, "no paths: call dfk_paths_build");
    if (!pairs) {
        if (n_pairs) return fail(DFK_E_ARG, "null argument");
        if (!P->hops_valid) return fail(DFK_E_STATE, "no edge pairs: call dfk_hops_build, or pass the pairs");
        pairs = P->hops.data(); n_pairs = P->hops.size() / 2;
    }
    if (!dup) return fail(DFK_E_ARG, "null argument: the duplicate marks (a.dup, a byte a pair) are required");
    HIP_TRY(hipSetDevice(c->device));
    const HostGraph* G = graph_of(c);
    const std::vector<int32_t> inv = involution_of(G);
    std::vector<int32_t> kmers(inv.size());
    for (size_t e = 0; e < kmers.size(); ++e) kmers[e] = (int32_t)G->ce[G->he[e].ce].n;
    const CloserSource S{&P->batches, P->n_reads, inv.size(), inv.data(), kmers.data(), (int32_t)c->cfg.K};
    std::unique_ptr<CloserResult> R(new CloserResult);
    if (int rc = closer_build(c, S, pairs, n_pairs, dup, R.get())) return rc;  // (refused: the earlier result is still served)
    closer_drop_arrays(c);
    if (P->closer) closer_result_free(P->closer);
    P->closer = R.release(); P->closer_free = closer_result_free;
    return 0;
    });
}

// The stage on paths given as host arrays: the batches laid out as k_path_emit leaves them (dfk_subset_build_arrays does the
// same, here with the offset words), then closer_build() and -- with a directory -- closer_write().
int dfk_closer_build_arrays(dfk_ctx* c, uint64_t n_edges, const int32_t* inv, const int32_t* kmers, uint64_t n_reads, const uint64_t* first, const int32_t* edges,
                            const int32_t* offsets, const int32_t* pairs, uint64_t n_pairs, const uint8_t* dup, uint64_t reads_per_batch, const char* dir)
{
    return guarded([&]() -> int {
    if (!c) return fail(DFK_E_ARG, "null context");
    const uint64_t E = n_edges, N = n_reads;
    if ((E && (!inv || !kmers)) || !first || (n_pairs && !pairs) || !dup || (N && !offsets)) return fail(DFK_E_ARG, "null argument");
    if (N % 2) return fail(DFK_E_ARG, "%llu reads: the closers take a read's mate as id ^ 1", (unsigned long long)N);
    if (N >= (1ull << 31) || E >= (1ull << 31)) return fail(DFK_E_ARG, "%llu reads, %llu edges: 2^31 - 1 of each at most", (unsigned long long)N, (unsigned long long)E);
    for (uint64_t e = 0; e < E; ++e) {
        if (inv[e] < 0 || (uint64_t)inv[e] >= E || inv[inv[e]] != (int32_t)e) return fail(DFK_E_ARG, "inv is not an involution at edge %llu", (unsigned long long)e);
        if (kmers[e] < 1 || kmers[inv[e]] != kmers[e]) return fail(DFK_E_ARG, "edge %llu has %d k-mers, its involution %d", (unsigned long long)e, kmers[e], kmers[inv[e]]);
    }
    if (first[0] != 0) return fail(DFK_E_ARG, "the paths do not start at 0");
    for (uint64_t i = 0; i < N; ++i) if (first[i + 1] < first[i]) return fail(DFK_E_ARG, "the paths' starts fall at read %llu", (unsigned long long)i);
    if (first[N] && !edges) return fail(DFK_E_ARG, "null argument");
    for (uint64_t k = 0; k < first[N]; ++k) if (edges[k] < 0 || (uint64_t)edges[k] >= E) return fail(DFK_E_ARG, "a path holds edge %d: the graph has %llu", edges[k], (unsigned long long)E);
    HIP_TRY(hipSetDevice(c->device));
    std::vector<PathBatch> batches;
    const uint64_t mark = c->alloc_seq;
    const uint64_t per = reads_per_batch ? reads_per_batch : std::max<uint64_t>(1, N);
    std::unique_ptr<CloserResult> R(new CloserResult);
    auto body = [&]() -> int {
        int rc;
        for (uint64_t r0 = 0; r0 < N; r0 += per) {
            PathBatch B; B.r0 = r0; B.n = std::min(per, N - r0); B.file_base = 24 + 8 * r0 + 4 * first[r0];
            std::vector<uint32_t> var, off;
            layout_batch(first, edges, offsets, r0, B.n, var, off);
            B.var_bytes = var.size() * 4;
            if (B.var_bytes >= (1ull << 32)) return fail(DFK_E_ARG, "a batch of %llu reads holds %llu bytes of paths: its offsets keep 32 bits", (unsigned long long)B.n, (unsigned long long)B.var_bytes);
            if ((rc = upload_vec(c, B.var, var, "a.paths data")) || (rc = upload_vec(c, B.elem_off, off, "a.paths offsets"))) return rc;
            batches.push_back(B);
        }
        const CloserSource S{&batches, N, E, inv, kmers, (int32_t)c->cfg.K};
        if ((rc = closer_build(c, S, pairs, n_pairs, dup, R.get()))) return rc;
        return dir ? closer_write(R.get(), dir) : 0;
    };
    int rc;
    try { rc = body(); } catch (const std::runtime_error& e) { rc = fail(DFK_E_HIP, "%s", e.what()); }
    (void)hipStreamSynchronize(c->stream);
    c->release_since(mark);                                                  // the batches
    if (rc) return rc;
    closer_drop_arrays(c);
    graph_of(c)->closer_arrays = R.release(); graph_of(c)->closer_free = closer_result_free;
    return 0;
    });
}

int dfk_closer_stats(dfk_ctx* c, uint64_t* out)
{
    return guarded([&]() -> int {
    CloserResult* R = nullptr;
    if (int rc = closer_result_of(c, &R)) return rc;
    if (!out) return fail(DFK_E_ARG, "null argument");
    for (int i = 0; i < DFK_CLOSER_WORDS; ++i) out[i] = R->stats[i];
    return 0;
    });
}

int dfk_closer_fetch(dfk_ctx* c, uint64_t* edges, uint64_t edges_cap, uint64_t* n_edges, uint64_t* loc_first, uint64_t* locs, uint64_t locs_cap, uint64_t* n_locs,
                     uint64_t* anchor_first, int32_t* anchors, uint64_t anchors_cap, uint64_t* n_anchors, uint64_t* read_first, uint64_t* reads, uint64_t reads_cap, uint64_t* n_reads)
{
    return guarded([&]() -> int {
    CloserResult* R = nullptr;
    if (int rc = closer_result_of(c, &R)) return rc;
    const uint64_t ne = R->ce.size(), nl = R->locs.size() / 2, na = R->anchors.size() / 3, nr = R->reads.size();
    if (n_edges) *n_edges = ne;
    if (n_locs) *n_locs = nl;
    if (n_anchors) *n_anchors = na;
    if (n_reads) *n_reads = nr;
    if ((edges || edges_cap) && edges_cap < ne) return fail(DFK_E_ARG, "buffer too small: %llu < %llu closer edges", (unsigned long long)edges_cap, (unsigned long long)ne);
    if ((locs || locs_cap) && locs_cap < nl) return fail(DFK_E_ARG, "buffer too small: %llu < %llu locs records", (unsigned long long)locs_cap, (unsigned long long)nl);
    if ((anchors || anchors_cap) && anchors_cap < na) return fail(DFK_E_ARG, "buffer too small: %llu < %llu anchors", (unsigned long long)anchors_cap, (unsigned long long)na);
    if ((reads || reads_cap) && reads_cap < nr) return fail(DFK_E_ARG, "buffer too small: %llu < %llu set entries", (unsigned long long)reads_cap, (unsigned long long)nr);
    if ((edges_cap && ne && !edges) || (locs_cap && nl && !locs) || (anchors_cap && na && !anchors) || (reads_cap && nr && !reads)) return fail(DFK_E_ARG, "null argument");
    if (edges && ne) memcpy(edges, R->ce.data(), 8 * ne);
    if (locs && nl) memcpy(locs, R->locs.data(), 16 * nl);
    if (anchors && na) memcpy(anchors, R->anchors.data(), 12 * na);
    if (reads && nr) memcpy(reads, R->reads.data(), 8 * nr);
    if (loc_first) memcpy(loc_first, R->loc_first.data(), 8 * (ne + 1));                         // the starts: room for n_edges + 1 words each
    if (anchor_first) memcpy(anchor_first, R->anchor_first.data(), 8 * (ne + 1));
    if (read_first) memcpy(read_first, R->read_first.data(), 8 * (ne + 1));
    return 0;
    });
}

int dfk_closer_write(dfk_ctx* c, const char* dir)
{
    return guarded([&]() -> int {
    CloserResult* R = nullptr;
    if (int rc = closer_result_of(c, &R)) return rc;
    if (!dir) return fail(DFK_E_ARG, "null directory");
    return closer_write(R, dir);
    });
}

} // extern "C"
