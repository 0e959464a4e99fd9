// superplus_amd/csrc/dfk_pbf.inc -- SURVEY 8(f)-3 (included by dfk.hip): dfk_pbf_*, the device half of ParseBarcodedFastqs.
// Kernels and what each replaces: dfk_pbf_kernels.h.  Host side here: upload of a group's held reads, the stable LSD radix
// sort (k_rs_hist / k_rs_scatter of dfk_paths_kernels.h with digits read off the sequences), the two-phase PQVec encoder in
// batches that fit the arena, the results back in host memory.
#include "dfk_pbf_kernels.h"

struct dfk_pbf {
    std::vector<uint32_t> order, read_len;
    std::vector<uint8_t> fastb_var, qualp_var;
    std::vector<uint64_t> fastb_off, qualp_off;
    float ms_sort = 0, ms_encode = 0, ms_total = 0;
};

namespace {

int pbf_run(dfk_ctx* c, const dfk_pbf_input* in, dfk_pbf* R)
{
    const uint64_t m = in->m;
    if (m >= (1ull << 31)) return fail(DFK_E_ARG, "more than 2^31-1 pairs in one group");
    Timer t_all(c->stream); t_all.start();
    const uint64_t mark = c->alloc_seq;
    const unsigned cus = (unsigned)c->prop.multiProcessorCount;
    auto grid_for = [&](uint64_t n, unsigned per = 256) { return (unsigned)std::max<uint64_t>(1, std::min<uint64_t>((n + per - 1) / per, 32ull * cus)); };
    auto body = [&]() -> int {
        int rc = 0;
        uint64_t sb[2] = {0, 0};
        for (int f = 0; f < 2; ++f) if (m) { rc = host_read(c, &sb[f], (const char*)in->off[f] + 8 * m, 8); if (rc) return rc; }
        DevBuf d_seq[2], d_qual[2], d_off[2], d_rank, perm[2], digit[2], hist, place, ctr;
        for (int f = 0; f < 2; ++f) {
            if ((rc = c->alloc(d_seq[f], sb[f] + 8, "fastq bases")) || (rc = c->alloc(d_qual[f], sb[f] + 8, "fastq qualities")) || (rc = c->alloc(d_off[f], (m + 1) * 8, "fastq offsets"))) return rc;
            if ((rc = upload(c, d_seq[f].p, in->seq[f], sb[f])) || (rc = upload(c, d_qual[f].p, in->qual[f], sb[f])) || (rc = upload(c, d_off[f].p, in->off[f], (m + 1) * 8))) return rc;
        }
        if ((rc = c->alloc(d_rank, std::max<uint64_t>(1, m) * 4, "barcode places")) || (rc = upload(c, d_rank.p, in->rank, m * 4))) return rc;
        if ((rc = c->alloc(ctr, 64, "pbf counters"))) return rc;
        HIP_TRY(hipMemsetAsync(ctr.p, 0, 64, c->stream));
        unsigned int* bad = (unsigned int*)ctr.p;
        unsigned long long* d_n = (unsigned long long*)((char*)ctr.p + 8);
        unsigned long long* d_max = (unsigned long long*)((char*)ctr.p + 16);      // [2]
        const PbfFiles F{{(const uint8_t*)d_seq[0].p, (const uint8_t*)d_seq[1].p}, {(const uint8_t*)d_qual[0].p, (const uint8_t*)d_qual[1].p},
                         {(const uint64_t*)d_off[0].p, (const uint64_t*)d_off[1].p}};
        for (int i = 0; i < 2; ++i) if ((rc = c->alloc(perm[i], std::max<uint64_t>(1, m) * 4, "pair order")) || (rc = c->alloc(digit[i], std::max<uint64_t>(1, m) * 4, "sort digits"))) return rc;
        // ---- which pairs are written, in file order; the longest read of either file
        Timer t(c->stream); t.start();
        hipLaunchKernelGGL(k_pbf_keep, dim3(1), dim3(256), 0, c->stream, (const uint32_t*)d_rank.p, m, (uint32_t*)perm[0].p, d_n);
        for (int f = 0; f < 2; ++f) if (m) hipLaunchKernelGGL(k_pbf_max_len, dim3(grid_for(m)), dim3(256), 0, c->stream, F.off[f], m, d_max + f);
        HIP_TRY(hipGetLastError());
        uint64_t h[4] = {};
        HIP_TRY(hipMemcpyAsync(h, ctr.p, 32, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
        const uint64_t n = h[1];
        const uint32_t max_len[2] = {(uint32_t)h[2], (uint32_t)h[3]};
        if (h[2] > 65535 || h[3] > 65535) return fail(DFK_E_INPUT, "a read of %llu bases (65535 at most)", (unsigned long long)std::max(h[2], h[3]));
        // ---- the order: stable LSD radix sort, least significant digit first
        int cur = 0;
        if (n > 1) {
            const uint64_t n_tiles = (n + RS_TILE - 1) / RS_TILE;
            if ((rc = c->alloc(hist, 256 * n_tiles * 8, "sort counts")) || (rc = c->alloc(place, 256 * n_tiles * 8, "sort places"))) return rc;
            const unsigned sgrid = (unsigned)std::min<uint64_t>((n_tiles + RS_WAVES - 1) / RS_WAVES, 16ull * cus);
            auto pass = [&](int what, int file, uint32_t window) -> int {
                hipLaunchKernelGGL(k_pbf_digit, dim3(grid_for(n)), dim3(256), 0, c->stream, F, (const uint32_t*)d_rank.p, (const uint32_t*)perm[cur].p, n, what, file, window,
                                   (uint32_t*)digit[0].p, bad);
                hipLaunchKernelGGL(k_rs_hist, dim3(sgrid), dim3(64 * RS_WAVES), 0, c->stream, (const uint32_t*)digit[0].p, n, 0u, n_tiles, (uint64_t*)hist.p);
                HIP_TRY(hipGetLastError());
                int r = device_scan(c, (const uint64_t*)hist.p, (uint64_t*)place.p, 256 * n_tiles); if (r) return r;
                hipLaunchKernelGGL(k_rs_scatter, dim3(sgrid), dim3(64 * RS_WAVES), 0, c->stream, (const uint32_t*)digit[0].p, (const uint32_t*)perm[cur].p, n, 0u, n_tiles,
                                   (const uint64_t*)place.p, (uint32_t*)digit[1].p, (uint32_t*)perm[cur ^ 1].p);
                HIP_TRY(hipGetLastError());
                cur ^= 1;
                return 0;
            };
            uint32_t max_rank = 0;
            for (uint64_t i = 0; i < m; ++i) if (in->rank[i] != PBF_DROP) max_rank = std::max(max_rank, in->rank[i]);
            for (int f = 1; f >= 0; --f) {
                for (uint32_t b = 0; b < 2; ++b) if ((max_len[f] >> (8 * b)) || b == 0) { if ((rc = pass(1, f, b))) return rc; }
                for (uint32_t w = (max_len[f] + 3) / 4; w-- > 0;) if ((rc = pass(0, f, w))) return rc;
            }
            for (uint32_t b = 0; b < 4; ++b) if ((max_rank >> (8 * b)) || b == 0) { if ((rc = pass(2, 0, b))) return rc; }
        }
        R->ms_sort = t.stop();
        const uint64_t n_reads = 2 * n;
        const uint32_t* order = (const uint32_t*)perm[cur].p;
        // ---- lengths, 2-bit bases
        t.start();
        DevBuf d_len, fb_sz, fb_off, fb_var, pq_sz, pq_off, pq_var;
        if ((rc = c->alloc(d_len, std::max<uint64_t>(1, n_reads) * 4, "read lengths")) || (rc = c->alloc(fb_sz, (n_reads + 1) * 8, "fastb sizes")) || (rc = c->alloc(fb_off, (n_reads + 1) * 8, "fastb offsets")) ||
            (rc = c->alloc(pq_sz, (n_reads + 1) * 8, "qualp sizes")) || (rc = c->alloc(pq_off, (n_reads + 1) * 8, "qualp offsets"))) return rc;
        hipLaunchKernelGGL(k_pbf_sizes, dim3(grid_for(n_reads + 1)), dim3(256), 0, c->stream, F, order, n_reads, (uint32_t*)d_len.p, (uint64_t*)fb_sz.p);
        HIP_TRY(hipGetLastError());
        rc = device_scan(c, (const uint64_t*)fb_sz.p, (uint64_t*)fb_off.p, n_reads + 1); if (rc) return rc;
        uint64_t fb_bytes = 0;
        HIP_TRY(hipMemcpyAsync(&fb_bytes, (uint64_t*)fb_off.p + n_reads, 8, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
        if ((rc = c->alloc(fb_var, fb_bytes + 8, ".fastb data"))) return rc;
        if (n_reads) hipLaunchKernelGGL(k_pbf_pack, dim3(grid_for(n_reads)), dim3(256), 0, c->stream, F, order, n_reads, (const uint64_t*)fb_off.p, (uint8_t*)fb_var.p, bad);
        HIP_TRY(hipGetLastError());
        // ---- PQVec: plan (the encoder's dynamic programme, block lists in scratch: 8 bytes a base + 4 a read), sizes, then the bit
        //      streams.  The scratch is taken in pieces of at most a quarter of the free room (one allocation each) and stays until
        //      the streams are written: a group the host could hold is far below what the device holds.
        HIP_TRY(hipMemsetAsync((uint64_t*)pq_sz.p + n_reads, 0, 8, c->stream));
        struct Batch { uint64_t k0, nk; DevBuf scratch, soff, nblk; };
        std::vector<Batch> batches;
        const uint64_t per_read = 8ull * std::max(max_len[0], max_len[1]) + 4 + 32;
        const uint64_t room = std::max<uint64_t>(64ull << 20, c->largest_allocatable() / 4);
        uint64_t per_batch = std::max<uint64_t>(1, std::min<uint64_t>(n_reads, room / per_read));
        if (const char* e = getenv("DFK_PBF_BATCH_READS")) per_batch = std::min(per_batch, std::max<uint64_t>(1, (uint64_t)atoll(e)));      // (tests: more than one batch)
        const bool plan_in_lds = std::max(max_len[0], max_len[1]) <= PBF_LDS_LEN;
        for (uint64_t k0 = 0; k0 < n_reads; k0 += per_batch) {
            Batch B; B.k0 = k0; B.nk = std::min(per_batch, n_reads - k0);
            DevBuf ssz;
            if ((rc = c->alloc(ssz, (B.nk + 1) * 8, "scratch sizes", Place::Low)) || (rc = c->alloc(B.soff, (B.nk + 1) * 8, "scratch offsets", Place::Low)) || (rc = c->alloc(B.nblk, B.nk * 4, "block counts", Place::Low))) return rc;
            hipLaunchKernelGGL(k_pbf_scratch_sizes, dim3(grid_for(B.nk + 1)), dim3(256), 0, c->stream, F, order, B.k0, B.nk, (uint64_t*)ssz.p);
            HIP_TRY(hipGetLastError());
            rc = device_scan(c, (const uint64_t*)ssz.p, (uint64_t*)B.soff.p, B.nk + 1); if (rc) return rc;
            uint64_t words = 0;
            HIP_TRY(hipMemcpyAsync(&words, (uint64_t*)B.soff.p + B.nk, 8, hipMemcpyDeviceToHost, c->stream));
            HIP_TRY(hipStreamSynchronize(c->stream));
            c->release(ssz);
            if ((rc = c->alloc(B.scratch, std::max<uint64_t>(1, words) * 4, "encoder scratch", Place::Low))) return rc;
            TRACE("pbf: encoder batch of %llu reads from read %llu of %llu, %llu words of scratch, plan in %s", (unsigned long long)B.nk, (unsigned long long)B.k0,
                  (unsigned long long)n_reads, (unsigned long long)words, plan_in_lds ? "LDS" : "HBM");
            if (plan_in_lds)
                hipLaunchKernelGGL(k_pbf_pq_plan_lds, dim3((unsigned)std::max<uint64_t>(1, std::min<uint64_t>((B.nk + 63) / 64, 64ull * cus))), dim3(64), 0, c->stream, F, order, B.k0, B.nk,
                                   (const uint64_t*)B.soff.p, (uint32_t*)B.scratch.p, (uint32_t*)B.nblk.p, (uint64_t*)pq_sz.p + B.k0, bad);
            else
                hipLaunchKernelGGL(k_pbf_pq_plan, dim3(grid_for(B.nk, 128)), dim3(128), 0, c->stream, F, order, B.k0, B.nk, (const uint64_t*)B.soff.p, (uint32_t*)B.scratch.p,
                                   (uint32_t*)B.nblk.p, (uint64_t*)pq_sz.p + B.k0, bad);
            HIP_TRY(hipGetLastError());
            batches.push_back(B);
        }
        rc = device_scan(c, (const uint64_t*)pq_sz.p, (uint64_t*)pq_off.p, n_reads + 1); if (rc) return rc;
        uint64_t pq_bytes = 0;
        unsigned flags = 0;
        HIP_TRY(hipMemcpyAsync(&pq_bytes, (uint64_t*)pq_off.p + n_reads, 8, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipMemcpyAsync(&flags, bad, 4, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
        if (flags & 1u) return fail(DFK_E_INPUT, "unexpected base in a read (A, C, G, T, N in either case are what a fastq holds)");
        if (flags & 2u) return fail(DFK_E_INPUT, "Your input reads are funny.  I found a quality score above 63. The maximum value that I allow is 63.");
        if ((rc = c->alloc(pq_var, pq_bytes + 8, ".qualp data"))) return rc;
        for (const Batch& B : batches)
            hipLaunchKernelGGL(k_pbf_pq_emit, dim3(grid_for(B.nk, 128)), dim3(128), 0, c->stream, F, order, B.k0, B.nk, (const uint64_t*)B.soff.p, (const uint32_t*)B.scratch.p,
                               (const uint32_t*)B.nblk.p, (const uint64_t*)pq_off.p, (uint8_t*)pq_var.p);
        HIP_TRY(hipGetLastError());
        R->ms_encode = t.stop();
        // ---- results to the host
        R->order.resize(n); R->read_len.resize(n_reads); R->fastb_var.resize(fb_bytes); R->qualp_var.resize(pq_bytes);
        R->fastb_off.resize(n_reads + 1); R->qualp_off.resize(n_reads + 1);
        auto down = [&](void* dst, const void* src, uint64_t bytes) -> int { if (bytes) HIP_TRY(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, c->stream)); return 0; };
        if ((rc = down(R->order.data(), order, n * 4)) || (rc = down(R->read_len.data(), d_len.p, n_reads * 4)) || (rc = down(R->fastb_var.data(), fb_var.p, fb_bytes)) ||
            (rc = down(R->qualp_var.data(), pq_var.p, pq_bytes)) || (rc = down(R->fastb_off.data(), fb_off.p, (n_reads + 1) * 8)) || (rc = down(R->qualp_off.data(), pq_off.p, (n_reads + 1) * 8))) return rc;
        HIP_TRY(hipStreamSynchronize(c->stream));
        return 0;
    };
    int rc;
    try { rc = body(); } catch (const std::runtime_error& e) { rc = fail(DFK_E_HIP, "%s", e.what()); }
    (void)hipStreamSynchronize(c->stream);
    c->release_since(mark);
    R->ms_total = t_all.stop();
    return rc;
}

} // namespace

extern "C" {

int dfk_pbf_run(dfk_ctx* c, const dfk_pbf_input* in, dfk_pbf** out)
{
    return guarded([&]() -> int {
    if (!c || !in || !out) return fail(DFK_E_ARG, "null argument");
    *out = nullptr;
    if (in->m && (!in->seq[0] || !in->seq[1] || !in->qual[0] || !in->qual[1] || !in->off[0] || !in->off[1] || !in->rank)) return fail(DFK_E_ARG, "null input array");
    HIP_TRY(hipSetDevice(c->device));
    std::unique_ptr<dfk_pbf> R(new dfk_pbf);
    const int rc = pbf_run(c, in, R.get());
    if (rc) return rc;
    *out = R.release();
    return 0;
    });
}

int dfk_pbf_result(const dfk_pbf* r, dfk_pbf_output* o)
{
    if (!r || !o) return fail(DFK_E_ARG, "null argument");
    o->n_pairs = r->order.size();
    o->order = r->order.data(); o->read_len = r->read_len.data();
    o->fastb_var = r->fastb_var.data(); o->fastb_off = r->fastb_off.data();
    o->qualp_var = r->qualp_var.data(); o->qualp_off = r->qualp_off.data();
    o->ms_sort = r->ms_sort; o->ms_encode = r->ms_encode; o->ms_total = r->ms_total;
    return 0;
}

void dfk_pbf_free(dfk_pbf* r) { delete r; }

} // extern "C"
