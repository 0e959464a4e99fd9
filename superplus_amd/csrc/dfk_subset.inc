// superplus_amd/csrc/dfk_subset.inc -- the patching stage's subset of interest (StagePatch, 10X/runstages/RunStages.cc:208-254)
// and the files a.sub.ids, a.sub.eoi, a.sub.paths, a.sub.paths.inv, included by dfk.hip.
//
// The rule, the plan and the files' layouts: dfk_subset.h.  The kernels: dfk_subset_kernels.h.  Here: subset_build() -- the marks,
// eoi, the hit sweep and its fold per pair, the ids (for their count, their digest and the subset's size) and the entries per
// edge of interest -- and subset_write() -- the gather a batch at a time, the index subset a range of ranks at a time, both
// through write_pieces.  Everything on the device comes from the arena and goes back before either returns; between the calls
// the host keeps eoi, the marks, a bit per pair and where each edge's list starts.
#include "dfk_subset_kernels.h"

namespace {

struct SubsetResult {
    uint64_t n_edges = 0, n_reads = 0;
    std::vector<uint64_t> eoi;                        // ascending
    std::vector<uint32_t> marks;                      // in_pairs, a bit an edge
    std::vector<unsigned long long> pair_bits;        // a bit a pair: taken
    std::vector<uint64_t> index_first;                // [n_eoi + 1]: entries of the index subset before rank k
    uint64_t stats[DFK_SUBSET_WORDS] = {};
    uint64_t us_gather_build = 0, us_index_build = 0; // the build's share of DFK_SUBSET_US_GATHER / _US_INDEX (a write adds its own)
    bool from_arrays = false;                         // built by dfk_subset_build_arrays: what it was built from is gone
};
void subset_result_free(SubsetResult* r) { delete r; }

// what both steps read: the batches as the pather left them, the involution
struct SubsetSource { const std::vector<PathBatch>* batches; uint64_t n_reads, n_edges; const int32_t* inv; };

int pwrite_all(int fd, const void* p, uint64_t n, uint64_t off)
{
    for (uint64_t done = 0; done < n;) {
        const ssize_t w = pwrite(fd, (const char*)p + done, n - done, (off_t)(off + done));
        if (w <= 0) return -1;
        done += (uint64_t)w;
    }
    return 0;
}

int subset_build(dfk_ctx* c, const SubsetSource& S, const int32_t* pairs, uint64_t n_pairs, SubsetResult* R)
{
    using namespace dfk_subset;
    const uint64_t N = S.n_reads, E = S.n_edges, n_rp = N / 2;
    if (N % 2) return fail(DFK_E_ARG, "%llu reads: the subset of interest is taken pair by pair", (unsigned long long)N);
    if (N >= (1ull << 32)) return fail(DFK_E_ARG, "%llu reads: a feudal file counts its elements in 32 bits", (unsigned long long)N);
    if (E >= (1ull << 31)) return fail(DFK_E_ARG, "%llu edges", (unsigned long long)E);
    if (n_pairs && !pairs) return fail(DFK_E_ARG, "null argument");
    for (uint64_t i = 0; i < 2 * n_pairs; ++i)
        if (pairs[i] < 0 || (uint64_t)pairs[i] >= E) return fail(DFK_E_ARG, "pair %llu names edge %d: the graph has %llu", (unsigned long long)(i / 2), pairs[i], (unsigned long long)E);
    const unsigned cus = (unsigned)c->prop.multiProcessorCount;
    const double t_in = wall_now();
    const uint64_t mark = c->alloc_seq;
    R->n_edges = E; R->n_reads = N;
    float ms_sweep = 0, ms_gather = 0, ms_index = 0;
    uint64_t h_ctr[2] = {}, h_dg[8] = {}, n_eoi = 0, n_ids = 0, sub_bytes = 0;
    auto body = [&]() -> int {
        int rc;
        Timer tm(c->stream);
        DevBuf d_pairs, d_inv, d_marks, flags, rank, rank_of, d_eoi, dg, hit, bits, ctr;
        // ---- marks, their ranks, eoi
        tm.start();
        if ((rc = c->alloc(d_marks, std::max<uint64_t>(1, mark_words(E)) * 4, "edges in pairs", Place::Low)) || (rc = c->alloc(rank_of, std::max<uint64_t>(1, E) * 4, "ranks of the edges of interest", Place::Low)) ||
            (rc = c->alloc(dg, 64, "subset digests", Place::Low)) || (rc = c->alloc(flags, (E + 1) * 8, "edge flags", Place::Low)) || (rc = c->alloc(rank, (E + 1) * 8, "edge ranks", Place::Low))) return rc;
        HIP_TRY(hipMemsetAsync(d_marks.p, 0, std::max<uint64_t>(1, mark_words(E)) * 4, c->stream));
        HIP_TRY(hipMemsetAsync(dg.p, 0, 64, c->stream));
        if (n_pairs) {
            if ((rc = c->alloc(d_pairs, n_pairs * 8, "edge pairs", Place::Low)) || (rc = c->alloc(d_inv, E * 4, "involution", Place::Low))) return rc;
            HIP_TRY(hipMemcpyAsync(d_pairs.p, pairs, n_pairs * 8, hipMemcpyHostToDevice, c->stream));
            HIP_TRY(hipMemcpyAsync(d_inv.p, S.inv, E * 4, hipMemcpyHostToDevice, c->stream));
            hipLaunchKernelGGL(k_sub_mark, dim3(grid_256(2 * n_pairs, cus)), dim3(256), 0, c->stream, (const int32_t*)d_pairs.p, 2 * n_pairs, (const int32_t*)d_inv.p, (uint32_t*)d_marks.p);
        }
        hipLaunchKernelGGL(k_sub_flags, dim3(grid_256(E + 1, cus)), dim3(256), 0, c->stream, (const uint32_t*)d_marks.p, E, (uint64_t*)flags.p);
        HIP_TRY(hipGetLastError());
        if ((rc = device_scan(c, (const uint64_t*)flags.p, (uint64_t*)rank.p, E + 1))) return rc;
        HIP_TRY(hipMemcpyAsync(&n_eoi, (const uint64_t*)rank.p + E, 8, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
        if (n_eoi > E) return fail(DFK_E_HIP, "subset: %llu edges of interest among %llu edges", (unsigned long long)n_eoi, (unsigned long long)E);
        if ((rc = c->alloc(d_eoi, std::max<uint64_t>(1, n_eoi) * 8, "edges of interest", Place::Low))) return rc;
        if (E) hipLaunchKernelGGL(k_sub_eoi, dim3(grid_256(E, cus)), dim3(256), 0, c->stream, (const uint32_t*)d_marks.p, (const uint64_t*)rank.p, E, (uint64_t*)d_eoi.p, (uint32_t*)rank_of.p);
        if (n_eoi) hipLaunchKernelGGL(HIP_KERNEL_NAME(k_digest_seq<uint64_t>), dim3(grid_256(n_eoi, cus)), dim3(256), 0, c->stream, (const uint64_t*)d_eoi.p, n_eoi, SALT_EOI, (unsigned long long*)dg.p + 4);
        HIP_TRY(hipGetLastError());
        R->eoi.assign(n_eoi, 0); R->marks.assign(std::max<uint64_t>(1, mark_words(E)), 0u);
        if (n_eoi) HIP_TRY(hipMemcpyAsync(R->eoi.data(), d_eoi.p, n_eoi * 8, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipMemcpyAsync(R->marks.data(), d_marks.p, R->marks.size() * 4, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
        c->release(flags); c->release(rank); c->release(d_eoi);
        if (n_pairs) { c->release(d_pairs); c->release(d_inv); }
        // ---- the hit sweep, a batch at a time; the fold per pair after all of them
        if ((rc = c->alloc(hit, std::max<uint64_t>(1, N), "reads that hit", Place::Low)) || (rc = c->alloc(bits, std::max<uint64_t>(1, pair_words(n_rp)) * 8, "pairs taken", Place::Low)) ||
            (rc = c->alloc(ctr, 16, "subset counters", Place::Low))) return rc;
        HIP_TRY(hipMemsetAsync(hit.p, 0, std::max<uint64_t>(1, N), c->stream));
        HIP_TRY(hipMemsetAsync(bits.p, 0, std::max<uint64_t>(1, pair_words(n_rp)) * 8, c->stream));
        HIP_TRY(hipMemsetAsync(ctr.p, 0, 16, c->stream));
        for (const PathBatch& b : *S.batches)
            if (b.n) hipLaunchKernelGGL(k_sub_hit, dim3(grid_256(b.n, cus)), dim3(256), 0, c->stream, (const uint32_t*)b.var.p, (const uint32_t*)b.elem_off.p, b.n, b.r0, b.var_bytes,
                                        (const uint32_t*)d_marks.p, (uint8_t*)hit.p);
        if (n_rp) hipLaunchKernelGGL(k_sub_fold, dim3(grid_pairs(n_rp, cus)), dim3(256), 0, c->stream, (const uint8_t*)hit.p, n_rp, (unsigned long long*)bits.p, (unsigned long long*)ctr.p);
        HIP_TRY(hipGetLastError());
        R->pair_bits.assign(std::max<uint64_t>(1, pair_words(n_rp)), 0ull);
        HIP_TRY(hipMemcpyAsync(R->pair_bits.data(), bits.p, R->pair_bits.size() * 8, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipMemcpyAsync(h_ctr, ctr.p, 16, hipMemcpyDeviceToHost, c->stream));
        ms_sweep = tm.stop();
        c->release(hit);
        n_ids = 2 * h_ctr[0];
        if (n_ids > N) return fail(DFK_E_HIP, "subset: %llu ids of %llu reads", (unsigned long long)n_ids, (unsigned long long)N);
        if (n_ids >= (1ull << 32)) return fail(DFK_E_ARG, "the paths subset holds %llu elements: a feudal file counts its elements in 32 bits", (unsigned long long)n_ids);
        // ---- the ids, from the gather's scan: their number, their digest, the subset's bytes
        tm.start();
        uint64_t ids_done = 0;
        for (const PathBatch& b : *S.batches) {
            if (!b.n) continue;
            const GatherScratch gs = gather_scratch(b.n, 0, 0, false);
            DevBuf words, place, ids;
            if ((rc = c->alloc(words, gs.words, "gather sizes", Place::Low)) || (rc = c->alloc(place, gs.places, "gather places", Place::Low))) return rc;
            hipLaunchKernelGGL(k_sub_sizes, dim3(grid_reads(b.n, cus)), dim3(256), 0, c->stream, (const uint32_t*)b.elem_off.p, b.n, b.r0, b.var_bytes, (const unsigned long long*)bits.p, (uint64_t*)words.p);
            HIP_TRY(hipGetLastError());
            if ((rc = device_scan(c, (const uint64_t*)words.p, (uint64_t*)place.p, b.n + 1))) return rc;
            uint64_t total = 0;
            HIP_TRY(hipMemcpyAsync(&total, (const uint64_t*)place.p + b.n, 8, hipMemcpyDeviceToHost, c->stream));
            HIP_TRY(hipStreamSynchronize(c->stream));
            const uint64_t cnt = gather_rank(total);
            if (cnt > b.n || gather_byte(total) > b.var_bytes) return fail(DFK_E_HIP, "subset: a batch of %llu reads gives %llu", (unsigned long long)b.n, (unsigned long long)cnt);
            if (cnt) {
                if ((rc = c->alloc(ids, gather_scratch(b.n, cnt, 0, false).ids, "read ids", Place::Low))) return rc;
                hipLaunchKernelGGL(k_sub_gather, dim3(grid_256(b.n, cus)), dim3(256), 0, c->stream, (const uint32_t*)b.var.p, (const uint32_t*)b.elem_off.p, b.n, b.r0, b.var_bytes,
                                   (const unsigned long long*)bits.p, (const uint64_t*)place.p, 0ull, (uint64_t*)ids.p, (uint64_t*)nullptr, (uint32_t*)nullptr);
                hipLaunchKernelGGL(HIP_KERNEL_NAME(k_digest_seq<uint64_t>), dim3(grid_256(cnt, cus)), dim3(256), 0, c->stream, (const uint64_t*)ids.p, cnt, SALT_IDS + ids_done, (unsigned long long*)dg.p);
                HIP_TRY(hipGetLastError());
                HIP_TRY(hipStreamSynchronize(c->stream));
                c->release(ids);
            }
            c->release(words); c->release(place);
            ids_done += cnt; sub_bytes += gather_byte(total);
        }
        ms_gather = tm.stop();
        if (ids_done != n_ids) return fail(DFK_E_HIP, "subset: %llu ids gathered, %llu counted", (unsigned long long)ids_done, (unsigned long long)n_ids);
        // ---- entries per edge of interest: where each list of the index subset starts
        tm.start();
        std::vector<uint64_t> counts(n_eoi, 0);
        if (n_eoi) {
            DevBuf d_counts;
            if ((rc = c->alloc(d_counts, n_eoi * 8, "entries per edge of interest", Place::Low))) return rc;
            HIP_TRY(hipMemsetAsync(d_counts.p, 0, n_eoi * 8, c->stream));
            for (const PathBatch& b : *S.batches)
                if (b.n) hipLaunchKernelGGL(k_sub_rank_count, dim3(grid_256(b.n, cus)), dim3(256), 0, c->stream, (const uint32_t*)b.var.p, (const uint32_t*)b.elem_off.p, b.n, b.var_bytes,
                                            (const uint32_t*)d_marks.p, (const uint32_t*)rank_of.p, (unsigned long long*)d_counts.p);
            HIP_TRY(hipGetLastError());
            HIP_TRY(hipMemcpyAsync(counts.data(), d_counts.p, n_eoi * 8, hipMemcpyDeviceToHost, c->stream));
        }
        HIP_TRY(hipMemcpyAsync(h_dg, dg.p, 64, hipMemcpyDeviceToHost, c->stream));
        ms_index = tm.stop();
        for (uint64_t k = 0; k < n_eoi; ++k)
            if (counts[k] >= (1ull << 32)) return fail(DFK_E_ARG, "edge %llu alone is on %llu reads: a range of the index subset sorts 32-bit positions", (unsigned long long)R->eoi[k], (unsigned long long)counts[k]);
        R->index_first = prefix_sums(counts.data(), n_eoi);
        return 0;
    };
    int rc;
    try { rc = body(); } catch (const std::runtime_error& e) { rc = fail(DFK_E_HIP, "%s", e.what()); }
    (void)hipStreamSynchronize(c->stream);
    c->release_since(mark);
    if (rc) return rc;
    uint64_t* s = R->stats;
    s[DFK_SUBSET_N_EOI] = n_eoi; s[DFK_SUBSET_N_IDS] = n_ids; s[DFK_SUBSET_PATH_ENTRIES] = (sub_bytes - 8 * n_ids) / 4; s[DFK_SUBSET_INDEX_ENTRIES] = R->index_first[n_eoi];
    s[DFK_SUBSET_RANGES] = count_ranges(R->index_first.data(), n_eoi, range_cap(c->largest_allocatable(), path_switches().pidx_range_pairs));
    s[DFK_SUBSET_ONE_READ_ONLY] = h_ctr[1];
    R->us_gather_build = (uint64_t)(1000.0f * ms_gather); R->us_index_build = (uint64_t)(1000.0f * ms_index);
    s[DFK_SUBSET_US] = (uint64_t)(1e6 * (wall_now() - t_in)); s[DFK_SUBSET_US_SWEEP] = (uint64_t)(1000.0f * ms_sweep);
    s[DFK_SUBSET_US_GATHER] = R->us_gather_build; s[DFK_SUBSET_US_INDEX] = R->us_index_build;
    s[DFK_SUBSET_IDS_SUM] = h_dg[0]; s[DFK_SUBSET_IDS_XOR] = h_dg[1]; s[DFK_SUBSET_EOI_SUM] = h_dg[4]; s[DFK_SUBSET_EOI_XOR] = h_dg[5];
    TRACE("subset: %llu edges of interest, %llu ids (%llu pairs through one read only), %llu path entries, %llu index entries in %llu range(s); marks and sweep %.1f ms, ids %.1f ms, counts %.1f ms",
          (unsigned long long)n_eoi, (unsigned long long)n_ids, (unsigned long long)h_ctr[1], (unsigned long long)s[DFK_SUBSET_PATH_ENTRIES], (unsigned long long)s[DFK_SUBSET_INDEX_ENTRIES],
          (unsigned long long)s[DFK_SUBSET_RANGES], ms_sweep, ms_gather, ms_index);
    return 0;
}

// the four files into `dir`: all of them, or none
int subset_write(dfk_ctx* c, const SubsetSource& S, SubsetResult* R, const std::string& dir)
{
    using namespace dfk_subset;
    const uint64_t N = S.n_reads, E = S.n_edges, n_rp = N / 2;
    const uint64_t n_eoi = R->eoi.size(), n_ids = R->stats[DFK_SUBSET_N_IDS], path_entries = R->stats[DFK_SUBSET_PATH_ENTRIES], index_entries = R->index_first[n_eoi];
    if (R->n_reads != N || R->n_edges != E) return fail(DFK_E_STATE, "the subset was built from other paths: call dfk_subset_build");
    const unsigned cus = (unsigned)c->prop.multiProcessorCount;
    const char* names[4] = {"a.sub.ids", "a.sub.eoi", "a.sub.paths", "a.sub.paths.inv"};
    std::string path[4]; int fd[4] = {-1, -1, -1, -1};
    const uint64_t mark = c->alloc_seq;
    float ms_gather = 0, ms_index = 0; uint64_t n_ranges = 0;
    auto body = [&]() -> int {
        int rc;
        for (int i = 0; i < 4; ++i) {
            path[i] = dir + "/" + names[i];
            fd[i] = open(path[i].c_str(), O_WRONLY | O_CREAT | O_TRUNC, 0666);
            if (fd[i] < 0) return fail(DFK_E_ARG, "cannot open %s", path[i].c_str());
        }
        // ---- the fixed parts: headers, sizes, eoi, the index subset's offsets
        const BinHead hi = bin_head(n_ids), he = bin_head(n_eoi);
        const FeudalLayout lp = paths_layout(n_ids, path_entries), lx = index_layout(n_eoi, index_entries);
        std::vector<uint64_t> eo(n_eoi + 1);
        for (uint64_t k = 0; k <= n_eoi; ++k) eo[k] = 24 + index_elem_bytes(R->index_first[k]);
        const uint64_t last = lp.var_tab;                                       // the (n + 1)-th offset of a.sub.paths: the end of its data
        if (pwrite_all(fd[0], &hi, 16, 0) || ftruncate(fd[0], (off_t)ids_file_size(n_ids)) != 0) return fail(DFK_E_ARG, "short write to %s", path[0].c_str());
        if (pwrite_all(fd[1], &he, 16, 0) || pwrite_all(fd[1], R->eoi.data(), 8 * n_eoi, 16)) return fail(DFK_E_ARG, "short write to %s", path[1].c_str());
        if (pwrite_all(fd[2], &lp.head, 24, 0) || ftruncate(fd[2], (off_t)lp.file_size) != 0 || pwrite_all(fd[2], &last, 8, lp.var_tab + 8 * n_ids)) return fail(DFK_E_ARG, "short write to %s", path[2].c_str());
        if (pwrite_all(fd[3], &lx.head, 24, 0) || ftruncate(fd[3], (off_t)lx.file_size) != 0 || pwrite_all(fd[3], eo.data(), 8 * (n_eoi + 1), lx.var_tab)) return fail(DFK_E_ARG, "short write to %s", path[3].c_str());
        // ---- what the host kept, on the device again
        std::vector<uint32_t> h_rank(std::max<uint64_t>(1, E), 0u);
        for (uint64_t k = 0; k < n_eoi; ++k) h_rank[R->eoi[k]] = (uint32_t)k;
        DevBuf d_marks, rank_of, bits;
        if ((rc = upload_vec(c, d_marks, R->marks, "edges in pairs")) || (rc = upload_vec(c, rank_of, h_rank, "ranks of the edges of interest")) || (rc = upload_vec(c, bits, R->pair_bits, "pairs taken"))) return rc;
        Timer tm(c->stream);
        // ---- ids and paths, a batch at a time
        uint64_t ids_done = 0, bytes_done = 0;
        for (const PathBatch& b : *S.batches) {
            if (!b.n || !n_rp) continue;
            const uint64_t bmark = c->alloc_seq;
            DevBuf words, place, ids, offs, data;
            if ((rc = c->alloc(words, gather_scratch(b.n, 0, 0, true).words, "gather sizes", Place::Low)) || (rc = c->alloc(place, gather_scratch(b.n, 0, 0, true).places, "gather places", Place::Low))) return rc;
            tm.start();
            hipLaunchKernelGGL(k_sub_sizes, dim3(grid_reads(b.n, cus)), dim3(256), 0, c->stream, (const uint32_t*)b.elem_off.p, b.n, b.r0, b.var_bytes, (const unsigned long long*)bits.p, (uint64_t*)words.p);
            HIP_TRY(hipGetLastError());
            if ((rc = device_scan(c, (const uint64_t*)words.p, (uint64_t*)place.p, b.n + 1))) return rc;
            uint64_t total = 0;
            HIP_TRY(hipMemcpyAsync(&total, (const uint64_t*)place.p + b.n, 8, hipMemcpyDeviceToHost, c->stream));
            ms_gather += tm.stop();
            const uint64_t cnt = gather_rank(total), bytes = gather_byte(total);
            if (ids_done + cnt > n_ids || bytes_done + bytes > lp.var_tab - 24) return fail(DFK_E_HIP, "subset: the gather outgrows what the build counted");
            if (cnt) {
                const GatherScratch gs = gather_scratch(b.n, cnt, bytes, true);
                if ((rc = c->alloc(ids, gs.ids, "read ids", Place::Low)) || (rc = c->alloc(offs, gs.offsets, "element offsets", Place::Low)) || (rc = c->alloc(data, gs.data, "a.sub.paths data", Place::Low))) return rc;
                tm.start();
                hipLaunchKernelGGL(k_sub_gather, dim3(grid_256(b.n, cus)), dim3(256), 0, c->stream, (const uint32_t*)b.var.p, (const uint32_t*)b.elem_off.p, b.n, b.r0, b.var_bytes,
                                   (const unsigned long long*)bits.p, (const uint64_t*)place.p, 24 + bytes_done, (uint64_t*)ids.p, (uint64_t*)offs.p, (uint32_t*)data.p);
                HIP_TRY(hipGetLastError());
                ms_gather += tm.stop();
                std::vector<FilePiece> to_ids, to_paths;
                append_pieces(to_ids, (const char*)ids.p, 8 * cnt, 16 + 8 * ids_done, XFER_CHUNK);
                append_pieces(to_paths, (const char*)data.p, bytes, 24 + bytes_done, XFER_CHUNK);
                append_pieces(to_paths, (const char*)offs.p, 8 * cnt, lp.var_tab + 8 * ids_done, XFER_CHUNK);
                if (write_pieces(c, fd[0], to_ids)) return fail(DFK_E_ARG, "short write to %s", path[0].c_str());
                if (write_pieces(c, fd[2], to_paths)) return fail(DFK_E_ARG, "short write to %s", path[2].c_str());
            }
            c->release_since(bmark);
            ids_done += cnt; bytes_done += bytes;
        }
        if (ids_done != n_ids || bytes_done != lp.var_tab - 24) return fail(DFK_E_HIP, "subset: %llu ids and %llu bytes gathered, the build counted %llu and %llu", (unsigned long long)ids_done,
                                                                            (unsigned long long)bytes_done, (unsigned long long)n_ids, (unsigned long long)(lp.var_tab - 24));
        // ---- the index subset, a range of ranks at a time: 24 bytes per entry while a range is sorted and widened
        const uint64_t cap = range_cap(c->largest_allocatable(), path_switches().pidx_range_pairs);
        for (uint64_t k0 = 0; k0 < n_eoi;) {
            const PidxRange range = next_range(R->index_first.data(), n_eoi, k0, cap);
            const uint64_t k1 = range.e1, n_r = range.n;
            if (!range.ok) return fail(DFK_E_ARG, "edge %llu alone is on %llu reads: a range of the index subset sorts 32-bit positions", (unsigned long long)R->eoi[k0], (unsigned long long)n_r);
            ++n_ranges;
            if (n_r) {
                const uint64_t rmark = c->alloc_seq;
                DevBuf k[2], v[2], wide;
                for (int i = 0; i < 2; ++i) { if ((rc = c->alloc(k[i], n_r * 4, "index keys", Place::Low)) || (rc = c->alloc(v[i], n_r * 4, "index reads", Place::Low))) return rc; }
                tm.start();
                uint64_t pair_base = 0;
                for (const PathBatch& b : *S.batches) {
                    if (!b.n) continue;
                    const RangeScratch rs = range_scratch(b.n);
                    DevBuf n_in, at_of;
                    if ((rc = c->alloc(n_in, rs.counts, "entries in the range", Place::Low)) || (rc = c->alloc(at_of, rs.places, "their places", Place::Low))) return rc;
                    hipLaunchKernelGGL(k_sub_range_count, dim3(grid_reads(b.n, cus)), dim3(256), 0, c->stream, (const uint32_t*)b.var.p, (const uint32_t*)b.elem_off.p, b.n, b.var_bytes,
                                       (const uint32_t*)d_marks.p, (const uint32_t*)rank_of.p, (uint32_t)k0, (uint32_t)k1, (uint64_t*)n_in.p);
                    HIP_TRY(hipGetLastError());
                    if ((rc = device_scan(c, (const uint64_t*)n_in.p, (uint64_t*)at_of.p, b.n + 1))) return rc;
                    uint64_t got = 0;
                    HIP_TRY(hipMemcpyAsync(&got, (const uint64_t*)at_of.p + b.n, 8, hipMemcpyDeviceToHost, c->stream));
                    HIP_TRY(hipStreamSynchronize(c->stream));
                    if (pair_base + got > n_r) return fail(DFK_E_HIP, "subset: more entries listed for ranks [%llu, %llu) than the build counted", (unsigned long long)k0, (unsigned long long)k1);
                    hipLaunchKernelGGL(k_sub_range_pairs, dim3(grid_256(b.n, cus)), dim3(256), 0, c->stream, (const uint32_t*)b.var.p, (const uint32_t*)b.elem_off.p, b.n, b.r0, b.var_bytes,
                                       (const uint32_t*)d_marks.p, (const uint32_t*)rank_of.p, (uint32_t)k0, (uint32_t)k1, (const uint64_t*)at_of.p, pair_base, (uint32_t*)k[0].p, (uint32_t*)v[0].p);
                    HIP_TRY(hipGetLastError());
                    HIP_TRY(hipStreamSynchronize(c->stream));
                    c->release(n_in); c->release(at_of);
                    pair_base += got;
                }
                if (pair_base != n_r) return fail(DFK_E_HIP, "subset: %llu entries listed for ranks [%llu, %llu), the build counted %llu", (unsigned long long)pair_base, (unsigned long long)k0, (unsigned long long)k1, (unsigned long long)n_r);
                // stable sort by rank: the read ids stay ascending inside an edge, a read that crosses it twice stays twice
                int cur = 0;
                if ((rc = radix_sort_pairs(c, k, v, n_r, range_key_bits(k1 - k0), &cur))) return rc;
                c->release(k[0]); c->release(k[1]); c->release(v[cur ^ 1]);
                if ((rc = c->alloc(wide, n_r * 8, "a.sub.paths.inv data", Place::Low))) return rc;
                hipLaunchKernelGGL(k_widen_u32, dim3(grid_256(n_r, cus)), dim3(256), 0, c->stream, (const uint32_t*)v[cur].p, n_r, (uint64_t*)wide.p, 0ull);
                HIP_TRY(hipGetLastError());
                ms_index += tm.stop();
                std::vector<FilePiece> pieces;
                append_pieces(pieces, (const char*)wide.p, 8 * n_r, 24 + 8 * R->index_first[k0], XFER_CHUNK);
                if (write_pieces(c, fd[3], pieces)) return fail(DFK_E_ARG, "short write to %s", path[3].c_str());
                c->release_since(rmark);
            }
            k0 = k1;
        }
        return 0;
    };
    int rc;
    try { rc = body(); } catch (const std::runtime_error& e) { rc = fail(DFK_E_HIP, "%s", e.what()); }
    const std::string first_err = rc ? g_err : std::string();
    for (int i = 0; i < 4; ++i)
        if (fd[i] >= 0 && close(fd[i]) != 0 && !rc) rc = fail(DFK_E_ARG, "short write to %s", path[i].c_str());
    (void)hipStreamSynchronize(c->stream);
    c->release_since(mark);
    if (rc) {                                                              // all four, or none
        for (int i = 0; i < 4; ++i) if (fd[i] >= 0) (void)unlink(path[i].c_str());
        return first_err.empty() ? rc : fail(rc, "%s", first_err.c_str());
    }
    R->stats[DFK_SUBSET_RANGES] = n_ranges;
    R->stats[DFK_SUBSET_US_GATHER] = R->us_gather_build + (uint64_t)(1000.0f * ms_gather);
    R->stats[DFK_SUBSET_US_INDEX] = R->us_index_build + (uint64_t)(1000.0f * ms_index);
    TRACE("subset: a.sub.* written: %llu ids, %llu range(s); gather %.1f ms, index %.1f ms on the device", (unsigned long long)n_ids, (unsigned long long)n_ranges, ms_gather, ms_index);
    return 0;
}

void subset_drop_arrays(dfk_ctx* c)
{
    HostGraph* G = graph_of(c);
    if (G->subset_arrays) { subset_result_free(G->subset_arrays); G->subset_arrays = nullptr; }
}

// the latest build's result: dfk_subset_build_arrays keeps its own beside the graph until the next build of either kind
int subset_result_of(dfk_ctx* c, SubsetResult** out)
{
    if (!c) return fail(DFK_E_ARG, "null context");
    if (c->graph_state && graph_of(c)->subset_arrays) { *out = graph_of(c)->subset_arrays; return 0; }
    PathState* P = built_paths(c);
    if (!P) return fail(DFK_E_STATE, "no subset: call dfk_paths_build and dfk_subset_build");
    if (!P->sub) return fail(DFK_E_STATE, "no subset: call dfk_subset_build");
    *out = P->sub;
    return 0;
}

std::vector<int32_t> involution_of(const HostGraph* G)
{
    std::vector<int32_t> inv(G->he.size());
    for (size_t e = 0; e < inv.size(); ++e) inv[e] = G->he[e].rc ? G->fwd[G->he[e].ce] : G->rev[G->he[e].ce];
    return inv;
}

} // namespace

extern "C" {

int dfk_subset_build(dfk_ctx* c, const int32_t* pairs, uint64_t n_pairs)
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
    HIP_TRY(hipSetDevice(c->device));
    const HostGraph* G = graph_of(c);
    const std::vector<int32_t> inv = involution_of(G);
    const SubsetSource S{&P->batches, P->n_reads, inv.size(), inv.data()};
    std::unique_ptr<SubsetResult> R(new SubsetResult);
    if (int rc = subset_build(c, S, pairs, n_pairs, R.get())) return rc;       // (refused: the earlier result is still served)
    subset_drop_arrays(c);
    if (P->sub) subset_result_free(P->sub);
    P->sub = R.release(); P->sub_free = subset_result_free;
    return 0;
    });
}

// The stage on paths given as host arrays: the batches laid out as k_path_emit leaves them (dfk_hops_build_arrays does the same),
// then subset_build() and -- with a directory -- subset_write() as dfk_subset_build / dfk_subset_write call them.
int dfk_subset_build_arrays(dfk_ctx* c, uint64_t n_edges, const int32_t* inv, uint64_t n_reads, const uint64_t* first, const int32_t* edges,
                            const int32_t* pairs, uint64_t n_pairs, uint64_t reads_per_batch, const char* dir)
{
    return guarded([&]() -> int {
    if (!c) return fail(DFK_E_ARG, "null context");
    const uint64_t E = n_edges, N = n_reads;
    if ((E && !inv) || !first || (n_pairs && !pairs)) return fail(DFK_E_ARG, "null argument");
    if (N % 2) return fail(DFK_E_ARG, "%llu reads: the subset of interest is taken pair by pair", (unsigned long long)N);
    if (N >= (1ull << 31) || E >= (1ull << 31)) return fail(DFK_E_ARG, "%llu reads, %llu edges: 2^31 - 1 of each at most", (unsigned long long)N, (unsigned long long)E);
    for (uint64_t e = 0; e < E; ++e)
        if (inv[e] < 0 || (uint64_t)inv[e] >= E || inv[inv[e]] != (int32_t)e) return fail(DFK_E_ARG, "inv is not an involution at edge %llu", (unsigned long long)e);
    if (first[0] != 0) return fail(DFK_E_ARG, "the paths do not start at 0");
    for (uint64_t i = 0; i < N; ++i) if (first[i + 1] < first[i]) return fail(DFK_E_ARG, "the paths' starts fall at read %llu", (unsigned long long)i);
    if (first[N] && !edges) return fail(DFK_E_ARG, "null argument");
    for (uint64_t k = 0; k < first[N]; ++k) if (edges[k] < 0 || (uint64_t)edges[k] >= E) return fail(DFK_E_ARG, "a path holds edge %d: the graph has %llu", edges[k], (unsigned long long)E);
    HIP_TRY(hipSetDevice(c->device));
    std::vector<PathBatch> batches;
    const uint64_t mark = c->alloc_seq;
    const uint64_t per = reads_per_batch ? reads_per_batch : std::max<uint64_t>(1, N);
    std::unique_ptr<SubsetResult> R(new SubsetResult);
    auto body = [&]() -> int {
        int rc;
        for (uint64_t r0 = 0; r0 < N; r0 += per) {
            PathBatch B; B.r0 = r0; B.n = std::min(per, N - r0); B.file_base = 24 + 8 * r0 + 4 * first[r0];
            std::vector<uint32_t> var, off;
            layout_batch(first, edges, nullptr, r0, B.n, var, off);
            B.var_bytes = var.size() * 4;
            if (B.var_bytes >= (1ull << 32)) return fail(DFK_E_ARG, "a batch of %llu reads holds %llu bytes of paths: its offsets keep 32 bits", (unsigned long long)B.n, (unsigned long long)B.var_bytes);
            if ((rc = upload_vec(c, B.var, var, "a.paths data")) || (rc = upload_vec(c, B.elem_off, off, "a.paths offsets"))) return rc;
            batches.push_back(B);
        }
        const SubsetSource S{&batches, N, E, inv};
        if ((rc = subset_build(c, S, pairs, n_pairs, R.get()))) return rc;
        return dir ? subset_write(c, S, R.get(), dir) : 0;
    };
    int rc;
    try { rc = body(); } catch (const std::runtime_error& e) { rc = fail(DFK_E_HIP, "%s", e.what()); }
    (void)hipStreamSynchronize(c->stream);
    c->release_since(mark);                                                  // the batches
    if (rc) return rc;
    R->from_arrays = true;
    subset_drop_arrays(c);
    graph_of(c)->subset_arrays = R.release(); graph_of(c)->subset_free = subset_result_free;
    return 0;
    });
}

int dfk_subset_stats(dfk_ctx* c, uint64_t* out)
{
    return guarded([&]() -> int {
    SubsetResult* R = nullptr;
    if (int rc = subset_result_of(c, &R)) return rc;
    if (!out) return fail(DFK_E_ARG, "null argument");
    for (int i = 0; i < DFK_SUBSET_WORDS; ++i) out[i] = R->stats[i];
    return 0;
    });
}

int dfk_subset_fetch(dfk_ctx* c, uint64_t* ids, uint64_t ids_cap, uint64_t* n_ids, uint64_t* eoi, uint64_t eoi_cap, uint64_t* n_eoi)
{
    return guarded([&]() -> int {
    SubsetResult* R = nullptr;
    if (int rc = subset_result_of(c, &R)) return rc;
    const uint64_t ni = R->stats[DFK_SUBSET_N_IDS], ne = R->eoi.size();
    if (n_ids) *n_ids = ni;
    if (n_eoi) *n_eoi = ne;
    if ((ids || ids_cap) && ids_cap < ni) return fail(DFK_E_ARG, "buffer too small: %llu < %llu ids", (unsigned long long)ids_cap, (unsigned long long)ni);
    if ((eoi || eoi_cap) && eoi_cap < ne) return fail(DFK_E_ARG, "buffer too small: %llu < %llu edges of interest", (unsigned long long)eoi_cap, (unsigned long long)ne);
    if ((ids_cap && ni && !ids) || (eoi_cap && ne && !eoi)) return fail(DFK_E_ARG, "null argument");
    if (ids) {
        uint64_t at = 0;
        for (uint64_t p = 0; p < R->n_reads / 2; ++p) if (dfk_subset::pair_bit(R->pair_bits.data(), p)) { ids[at++] = 2 * p; ids[at++] = 2 * p + 1; }
    }
    if (eoi && ne) memcpy(eoi, R->eoi.data(), 8 * ne);
    return 0;
    });
}

int dfk_subset_write(dfk_ctx* c, const char* dir)
{
    return guarded([&]() -> int {
    SubsetResult* R = nullptr;
    if (int rc = subset_result_of(c, &R)) return rc;
    if (!dir) return fail(DFK_E_ARG, "null directory");
    if (R->from_arrays) return fail(DFK_E_STATE, "the subset was built from arrays that did not outlive dfk_subset_build_arrays: that call writes the files");
    PathState* P = built_paths(c);
    if (!P) return fail(DFK_E_STATE, "no paths: call dfk_paths_build");
    HIP_TRY(hipSetDevice(c->device));
    const std::vector<int32_t> inv = involution_of(graph_of(c));
    const SubsetSource S{&P->batches, P->n_reads, inv.size(), inv.data()};
    return subset_write(c, S, R, dir);
    });
}

} // extern "C"
