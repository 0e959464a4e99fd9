// superplus_amd/csrc/dfk_paths_shard.inc -- rows f-2 and f-4 of a multi-GPU run (included by dfk.hip behind dfk_paths.inc).
//
// The reference paths reads with parallelForBatch over the read ids (paths/long/BuildReadQGraph48.cc:1420-1442): the step shards
// by read.  writePathsIndex is a sort of (edge, read) pairs (10X/PathsIndex.cc:23-146) and MarkDups a group-by on (first edge,
// offset, mate head) (10X/SecretOps.cc:410-566): both shard by key.  So, after the dictionary has been gathered on EVERY rank
// (df_shard.h, shard_allgather_dict) and every rank has built the same graph:
//   dfk_paths_build(ctx, NULL...)      a rank paths ITS pair range (the reads dfk_shard_begin_host staged, kept under
//                                      DFK_F_KEEP_INPUTS), dfk_paths_write_part puts its elements at their place in a.paths
//   dfk_shard_pidx_pairs / _write      its (edge, global read id) pairs sorted by edge, the slice of every edge range to that
//                                      range's owner (one all-to-all of 8-byte pairs); the owner merges what arrives -- runs
//                                      sorted by edge with ascending reads, from ranks holding ascending read ranges: a stable
//                                      sort by edge again -- and writes its range of a.paths.inv; rank 0 writes a.countsb from the
//                                      counts summed over the ranks
//   dfk_shard_dup_keys / _answer / _write   {key, score} of every placed read to the rank owning hash(key) (one all-to-all of
//                                      16-byte items), which finds each key's best member and answers a byte per item; the
//                                      marks go back in query order and every rank writes its pairs' bytes of a.dup
// The caller (df_shard.h) owns the exchanges, as for the count.
namespace {

__global__ void __launch_bounds__(256)
k_pack_pairs(const uint32_t* __restrict__ keys, const uint32_t* __restrict__ vals, uint64_t n, uint64_t* __restrict__ out)
{
    for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (uint64_t)gridDim.x * 256) out[i] = ((uint64_t)keys[i] << 32) | vals[i];
}
__global__ void __launch_bounds__(256)
k_unpack_pairs(const uint64_t* __restrict__ in, uint64_t n, uint32_t e0, uint32_t e1, uint32_t* __restrict__ keys, uint32_t* __restrict__ vals, uint32_t* __restrict__ counts, unsigned int* __restrict__ bad)
{
    for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (uint64_t)gridDim.x * 256) {
        const uint32_t e = (uint32_t)(in[i] >> 32);
        if (e < e0 || e >= e1) { atomicOr(bad, 1u); keys[i] = 0; vals[i] = 0; continue; }
        keys[i] = e - e0; vals[i] = (uint32_t)in[i];
        atomicAdd(&counts[e - e0], 1u);
    }
}

struct DupItem { unsigned long long key, score; };
// pass 0: items per owner; pass 1: the items, grouped by owner (cursor[] starts at the groups' first places), and which local read each is
template <bool PLACE>
__global__ void __launch_bounds__(256)
k_dup_items(const uint32_t* __restrict__ var, const uint32_t* __restrict__ elem_off, uint64_t nb, uint64_t r0, uint64_t var_bytes, const uint32_t* __restrict__ digest,
            uint64_t id_bias, uint32_t world, unsigned long long* __restrict__ cursor /* [world] */, DupItem* __restrict__ items, uint32_t* __restrict__ src, unsigned int* __restrict__ bad)
{
    for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < nb; i += (uint64_t)gridDim.x * 256) {
        uint64_t score = 0;
        const uint64_t k = dup_key(var, elem_off, i, nb, r0, var_bytes, digest, &score, bad, id_bias);
        if (k == DUP_EMPTY) continue;
        const uint32_t owner = (uint32_t)(dup_hash(k) >> 40) % world;
        const unsigned long long at = atomicAdd(&cursor[owner], 1ull);
        if (PLACE) { items[at] = DupItem{(unsigned long long)k, (unsigned long long)score}; src[at] = (uint32_t)(r0 + i); }
    }
}
template <bool ANSWER>
__global__ void __launch_bounds__(256)
k_dup_table(const DupItem* __restrict__ items, uint64_t n, unsigned long long* __restrict__ tkey, unsigned long long* __restrict__ tbest, uint64_t mask,
            uint8_t* __restrict__ ans, unsigned int* __restrict__ bad)
{
    for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (uint64_t)gridDim.x * 256) {
        const DupItem it = items[i];
        uint64_t s = dup_hash(it.key) & mask;
        for (uint64_t guard = 0; guard <= mask; ++guard, s = (s + 1) & mask) {
            if (!ANSWER) {
                const unsigned long long old = atomicCAS(&tkey[s], DUP_EMPTY, it.key);
                if (old == DUP_EMPTY || old == it.key) { atomicMax(&tbest[s], it.score); break; }
            } else {
                const unsigned long long cur = tkey[s];
                if (cur == it.key) { ans[i] = tbest[s] != it.score ? 1 : 0; break; }
                if (cur == DUP_EMPTY) { atomicOr(bad, 2u); ans[i] = 0; break; }
            }
        }
    }
}
__global__ void __launch_bounds__(256)
k_dup_mark(const uint8_t* __restrict__ ans, const uint32_t* __restrict__ src, uint64_t n, uint8_t* __restrict__ dup)
{
    for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (uint64_t)gridDim.x * 256) if (ans[i]) dup[src[i] >> 1] = 1;
}

struct ShardPaths {                 // what the sharded steps keep between their calls (hangs off PathState)
    DevBuf pairs;                   // dfk_shard_pidx_pairs: u64 (edge << 32 | global read), sorted by edge
    DevBuf items, src; uint64_t n_items = 0;
};
ShardPaths* shard_paths_of(PathState* P) { if (!P->shard) { P->shard = new ShardPaths; P->shard_free = [](void* p) { delete (ShardPaths*)p; }; } return (ShardPaths*)P->shard; }

} // namespace

extern "C" {

int dfk_paths_var_bytes(dfk_ctx* c, uint64_t* bytes)
{
    PathState* P = built_paths(c);
    if (!P || !bytes) return fail(DFK_E_STATE, "no paths: call dfk_paths_build");
    *bytes = P->var_total;
    return 0;
}

int dfk_paths_write_part(dfk_ctx* c, const char* path, uint64_t first_read, uint64_t total_reads, uint64_t var_before, uint64_t var_total)
{
    return guarded([&]() -> int {
    PathState* P = built_paths(c);
    if (!P) return fail(DFK_E_STATE, "no paths: call dfk_paths_build");
    if (!path) return fail(DFK_E_ARG, "null path");
    if (P->sink) return fail(DFK_E_STATE, "the paths are being written whole (dfk_paths_sink)");
    const uint64_t n = P->n_reads;
    if (first_read + n > total_reads || var_before + P->var_total > var_total || total_reads >= (1ull << 32)) return fail(DFK_E_ARG, "this rank's paths do not fit the file described");
    HIP_TRY(hipSetDevice(c->device));
    const FeudalLayout lay = feudal_layout(total_reads, 24, 4, var_total);
    const uint64_t var_tab = lay.var_tab, file_size = lay.file_size;
    const int fd = open(path, O_WRONLY | O_CREAT, 0666);
    if (fd < 0) return fail(DFK_E_ARG, "cannot open %s", path);
    int rc = 0;
    if (first_read == 0 && pwrite(fd, &lay.head, 24, 0) != 24) rc = fail(DFK_E_ARG, "short write to %s", path);
    if (!rc && ftruncate(fd, (off_t)file_size) != 0) rc = fail(DFK_E_ARG, "cannot size %s", path);      // every rank: the same size
    if (!rc && first_read + n == total_reads && pwrite(fd, &var_tab, 8, (off_t)(var_tab + 8 * total_reads)) != 8) rc = fail(DFK_E_ARG, "short write to %s", path);
    if (!rc) {
        std::vector<FilePiece> pieces;
        for (const PathBatch& b : P->batches) {
            const uint64_t at = var_before + b.file_base;                        // (file_base counts from 24 within this rank's data)
            append_pieces(pieces, (const char*)b.var.p, b.var_bytes, at, XFER_CHUNK);
            append_wide_pieces(pieces, (const char*)b.elem_off.p, b.n * 4, var_tab + 8 * (first_read + b.r0), at, XFER_CHUNK);
        }
        rc = write_pieces(c, fd, pieces);
        if (rc) rc = fail(DFK_E_ARG, "short write to %s", path);
    }
    if (close(fd) != 0 && !rc) rc = fail(DFK_E_ARG, "short write to %s", path);
    return rc;
    });
}

int dfk_shard_pidx_pairs(dfk_ctx* c, uint32_t world, const void** d_pairs, uint64_t* send_counts, uint64_t* counts_host)
{
    return guarded([&]() -> int {
    PathState* P = built_paths(c);
    if (!P) return fail(DFK_E_STATE, "no paths: call dfk_paths_build");
    if (!d_pairs || !send_counts || !counts_host || !world) return fail(DFK_E_ARG, "null argument");
    HIP_TRY(hipSetDevice(c->device));
    HostGraph* G = graph_of(c);
    release_path_lookup(c, G);
    const uint64_t n_pairs = P->n_edges, n_he = G->he.size();
    if (!n_he) return fail(DFK_E_STATE, "the graph has no edges");
    if (n_pairs >= (1ull << 32)) return fail(DFK_E_ARG, "%llu path entries on this rank: the paths index sorts 32-bit positions", (unsigned long long)n_pairs);
    const unsigned cus = (unsigned)c->prop.multiProcessorCount;
    ShardPaths* S = shard_paths_of(P);
    c->release(S->pairs);
    DevBuf k[2], v[2], counts;
    int rc;
    const uint64_t np1 = std::max<uint64_t>(1, n_pairs);
    if ((rc = c->alloc(S->pairs, np1 * 8, "index pairs to send"))) return rc;
    const uint64_t mark = c->alloc_seq;
    auto body = [&]() -> int {
        for (int i = 0; i < 2; ++i) { if ((rc = c->alloc(k[i], np1 * 4, "index keys", Place::Low)) || (rc = c->alloc(v[i], np1 * 4, "index reads", Place::Low))) return rc; }
        if ((rc = c->alloc(counts, n_he * 4, "reads per edge", Place::Low))) return rc;
        HIP_TRY(hipMemsetAsync(counts.p, 0, n_he * 4, c->stream));
        uint64_t pair_base = 0;
        for (const PathBatch& b : P->batches) {
            hipLaunchKernelGGL(k_pidx_pairs, dim3(grid_256(b.n, cus)), dim3(256), 0, c->stream, (const uint32_t*)b.var.p,
                               (const uint32_t*)b.elem_off.p, b.n, b.r0 + (uint64_t)P->read_id0, b.var_bytes, pair_base, (uint32_t*)k[0].p, (uint32_t*)v[0].p, (uint32_t*)counts.p);
            pair_base += b.var_bytes / 4 - 2 * b.n;
        }
        HIP_TRY(hipGetLastError());
        if (pair_base != n_pairs) return fail(DFK_E_HIP, "paths index: %llu path entries listed, %llu counted", (unsigned long long)pair_base, (unsigned long long)n_pairs);
        int cur = 0;
        if ((rc = radix_sort_pairs(c, k, v, n_pairs, pidx_key_bits(n_he), &cur))) return rc;
        if (n_pairs) hipLaunchKernelGGL(k_pack_pairs, dim3(grid_256(n_pairs, cus)), dim3(256), 0, c->stream, (const uint32_t*)k[cur].p,
                                        (const uint32_t*)v[cur].p, n_pairs, (uint64_t*)S->pairs.p);
        HIP_TRY(hipGetLastError());
        std::vector<uint32_t> hc(n_he);
        HIP_TRY(hipMemcpyAsync(hc.data(), counts.p, n_he * 4, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
        for (uint64_t e = 0; e < n_he; ++e) counts_host[e] = hc[e];
        shard_send_counts(hc.data(), n_he, world, send_counts);
        return 0;
    };
    try { rc = body(); } catch (const std::runtime_error& e) { rc = fail(DFK_E_HIP, "%s", e.what()); }
    (void)hipStreamSynchronize(c->stream);
    c->release_since(mark);
    *d_pairs = S->pairs.p;
    return rc;
    });
}

int dfk_shard_pidx_write(dfk_ctx* c, uint32_t world, uint32_t rank, const void* d_pairs_in, uint64_t n_in, const uint64_t* counts_global, const char* dir)
{
    return guarded([&]() -> int {
    PathState* P = built_paths(c);
    if (!P) return fail(DFK_E_STATE, "no paths: call dfk_paths_build");
    if (!counts_global || !dir || rank >= world || (n_in && !d_pairs_in)) return fail(DFK_E_ARG, "bad argument");
    HIP_TRY(hipSetDevice(c->device));
    HostGraph* G = graph_of(c);
    const unsigned cus = (unsigned)c->prop.multiProcessorCount;
    const uint64_t n_he = G->he.size(), e0 = edge_range_start(n_he, world, rank), e1 = edge_range_start(n_he, world, rank + 1), ne = e1 - e0;
    ShardPaths* S = shard_paths_of(P);
    c->release(S->pairs);                                                  // (sent: the room goes to the merge)
    const std::vector<uint64_t> first = prefix_sums(counts_global, n_he);
    const uint64_t total = first[n_he];
    if (first[e1] - first[e0] != n_in) return fail(DFK_E_HIP, "paths index: rank %u received %llu entries for its edges, the counts say %llu", rank, (unsigned long long)n_in,
                                                   (unsigned long long)(first[e1] - first[e0]));
    if (n_in >= (1ull << 32)) return fail(DFK_E_ARG, "%llu path entries for one rank's edges: the paths index sorts 32-bit positions", (unsigned long long)n_in);
    const uint64_t mark = c->alloc_seq;
    auto body = [&]() -> int {
        int rc;
        DevBuf k[2], v[2], cnt, var, d_bad;
        const uint64_t np1 = std::max<uint64_t>(1, n_in);
        for (int i = 0; i < 2; ++i) { if ((rc = c->alloc(k[i], np1 * 4, "index keys", Place::Low)) || (rc = c->alloc(v[i], np1 * 4, "index reads", Place::Low))) return rc; }
        if ((rc = c->alloc(cnt, std::max<uint64_t>(1, ne) * 4, "reads per edge", Place::Low)) || (rc = c->alloc(d_bad, 16, "index check", Place::Low))) return rc;
        HIP_TRY(hipMemsetAsync(cnt.p, 0, std::max<uint64_t>(1, ne) * 4, c->stream));
        HIP_TRY(hipMemsetAsync(d_bad.p, 0, 16, c->stream));
        if (n_in) hipLaunchKernelGGL(k_unpack_pairs, dim3(grid_256(n_in, cus)), dim3(256), 0, c->stream, (const uint64_t*)d_pairs_in, n_in,
                                     (uint32_t)e0, (uint32_t)e1, (uint32_t*)k[0].p, (uint32_t*)v[0].p, (uint32_t*)cnt.p, (unsigned int*)d_bad.p);
        HIP_TRY(hipGetLastError());
        int cur = 0;
        if ((rc = radix_sort_pairs(c, k, v, n_in, pidx_key_bits(ne), &cur))) return rc;
        std::vector<uint32_t> hc(ne);
        unsigned bad = 0;
        if (ne) HIP_TRY(hipMemcpyAsync(hc.data(), cnt.p, ne * 4, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipMemcpyAsync(&bad, d_bad.p, 4, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
        if (bad) return fail(DFK_E_HIP, "paths index: a pair arrived at a rank that does not own its edge");
        for (uint64_t e = 0; e < ne; ++e) if (hc[e] != counts_global[e0 + e]) return fail(DFK_E_HIP, "paths index: edge %llu received %u reads, the counts say %llu", (unsigned long long)(e0 + e), hc[e], (unsigned long long)counts_global[e0 + e]);
        c->release(k[0]); c->release(k[1]); c->release(v[cur ^ 1]);
        if ((rc = c->alloc(var, np1 * 8, "a.paths.inv data", Place::Low))) return rc;
        if (n_in) hipLaunchKernelGGL(k_widen_u32, dim3(grid_256(n_in, cus)), dim3(256), 0, c->stream, (const uint32_t*)v[cur].p, n_in, (uint64_t*)var.p);
        HIP_TRY(hipGetLastError());
        {   // digests of this rank's share (dfk_paths_digest; the caller adds / xors the ranks' words): positions and edges are the whole file's
            DevBuf dg, d_first;
            if ((rc = c->alloc(dg, 128, "index digest", Place::Low)) || (rc = c->alloc(d_first, (ne + 1) * 8, "list starts", Place::Low))) return rc;
            HIP_TRY(hipMemsetAsync(dg.p, 0, 128, c->stream));
            const uint64_t n_first = shard_table_entries(ne, world, rank);   // (the last rank also holds the end of the last list)
            HIP_TRY(hipMemcpyAsync(d_first.p, first.data() + e0, n_first * 8, hipMemcpyHostToDevice, c->stream));
            unsigned long long* d = (unsigned long long*)dg.p;
            if (n_in) hipLaunchKernelGGL(HIP_KERNEL_NAME(k_digest_seq<uint32_t>), dim3(grid_256(n_in, cus)), dim3(256), 0, c->stream,
                                         (const uint32_t*)v[cur].p, n_in, 0x1111ull + first[e0], d);
            if (n_first) hipLaunchKernelGGL(HIP_KERNEL_NAME(k_digest_seq<uint64_t>), dim3(grid_256(n_first, cus)), dim3(256), 0, c->stream,
                                            (const uint64_t*)d_first.p, n_first, 0x2222ull + e0, d + 4);
            HIP_TRY(hipGetLastError());
            uint64_t h[16] = {};
            HIP_TRY(hipMemcpyAsync(h, dg.p, 128, hipMemcpyDeviceToHost, c->stream));
            HIP_TRY(hipStreamSynchronize(c->stream));
            P->ck[DFK_CK_INV_SUM] = h[0]; P->ck[DFK_CK_INV_XOR] = h[1]; P->ck[DFK_CK_INV_STARTS] = h[4]; P->ck[DFK_CK_INV_ENTRIES] = n_in;
            P->ck[DFK_CK_COUNTSB_DIGEST] = P->ck[DFK_CK_COUNTSB_SUM] = P->ck[DFK_CK_SELF_INVERSE] = 0;
            P->ck[DFK_CK_VALID] |= DFK_CK_HAS_INDEX;
        }
        // this rank's range of a.paths.inv: the lists of edges [e0, e1) and their entries of the offset table
        const std::string path = std::string(dir) + "/a.paths.inv";
        const FeudalLayout lay = feudal_layout(n_he, 16, 8, 8 * total);
        const int fd = open(path.c_str(), O_WRONLY | O_CREAT, 0666);
        if (fd < 0) return fail(DFK_E_ARG, "cannot open %s", path.c_str());
        int wrc = 0;
        if (rank == 0 && pwrite(fd, &lay.head, 24, 0) != 24) wrc = fail(DFK_E_ARG, "short write to %s", path.c_str());
        if (!wrc && ftruncate(fd, (off_t)lay.file_size) != 0) wrc = fail(DFK_E_ARG, "cannot size %s", path.c_str());
        if (!wrc) {
            const std::vector<uint64_t> eo = shard_table_slice(first, e0, e1);
            const uint64_t n_eo = shard_table_entries(ne, world, rank);
            if (n_eo && pwrite(fd, eo.data(), 8 * n_eo, (off_t)(lay.var_tab + 8 * e0)) != (ssize_t)(8 * n_eo)) wrc = fail(DFK_E_ARG, "short write to %s", path.c_str());
        }
        if (!wrc) {
            std::vector<FilePiece> pieces;
            append_pieces(pieces, (const char*)var.p, 8 * n_in, 24 + 8 * first[e0], XFER_CHUNK);
            wrc = write_pieces(c, fd, pieces);
            if (wrc) wrc = fail(DFK_E_ARG, "short write to %s", path.c_str());
        }
        if (close(fd) != 0 && !wrc) wrc = fail(DFK_E_ARG, "short write to %s", path.c_str());
        if (wrc) return wrc;
        if (rank == 0) {   // a.countsb: reads per edge, an edge and its involution summed (:124-135), from the counts of all ranks
            std::vector<int32_t> csb(n_he);
            uint64_t sum = 0, self = 0, dsum = 0;
            for (uint64_t e = 0; e < n_he; ++e) {
                const uint64_t o = G->he[e].rc ? (uint64_t)G->fwd[G->he[e].ce] : (uint64_t)G->rev[G->he[e].ce];
                const uint64_t v2 = counts_global[e] + (o != e ? counts_global[o] : 0);
                csb[e] = (int32_t)v2; sum += v2; if (o == e) self += counts_global[e];
                auto mix = [](uint64_t x) { x ^= x >> 30; x *= 0xBF58476D1CE4E5B9ull; x ^= x >> 27; x *= 0x94D049BB133111EBull; return x ^ (x >> 31); };
                dsum += mix(mix(e + 0x3333ull) ^ (uint64_t)(uint32_t)csb[e]);
            }
            P->ck[DFK_CK_COUNTSB_DIGEST] = dsum; P->ck[DFK_CK_COUNTSB_SUM] = sum; P->ck[DFK_CK_SELF_INVERSE] = self;
            try { OutFile f(std::string(dir) + "/a.countsb"); f.raw("BINWRITE", 8); f.pod<uint64_t>(1); f.vec_i32(csb); f.close(); }
            catch (const std::runtime_error& e) { return fail(DFK_E_ARG, "%s", e.what()); }
        }
        return 0;
    };
    int rc;
    try { rc = body(); } catch (const std::runtime_error& e) { rc = fail(DFK_E_HIP, "%s", e.what()); }
    (void)hipStreamSynchronize(c->stream);
    c->release_since(mark);
    return rc;
    });
}

int dfk_shard_dup_keys(dfk_ctx* c, uint32_t world, const void** d_items, uint64_t* send_counts)
{
    return guarded([&]() -> int {
    PathState* P = built_paths(c);
    if (!P) return fail(DFK_E_STATE, "no paths: call dfk_paths_build");
    if (!d_items || !send_counts || !world || world > 64) return fail(DFK_E_ARG, "bad argument");
    if (P->n_reads % 2) return fail(DFK_E_ARG, "%llu reads: MarkDups works on pairs", (unsigned long long)P->n_reads);
    HIP_TRY(hipSetDevice(c->device));
    release_path_lookup(c, graph_of(c));
    const unsigned cus = (unsigned)c->prop.multiProcessorCount;
    ShardPaths* S = shard_paths_of(P);
    c->release(S->items); c->release(S->src);
    DevBuf cur, d_bad;
    int rc;
    if ((rc = c->alloc(cur, 64 * 8, "dup cursors", Place::Low)) || (rc = c->alloc(d_bad, 16, "dup check", Place::Low))) return rc;
    HIP_TRY(hipMemsetAsync(cur.p, 0, 64 * 8, c->stream));
    HIP_TRY(hipMemsetAsync(d_bad.p, 0, 16, c->stream));
    auto sweep = [&](bool place) {
        for (const PathBatch& b : P->batches) {
            const unsigned grid = grid_256(b.n, cus);
            if (!place) hipLaunchKernelGGL(HIP_KERNEL_NAME(k_dup_items<false>), dim3(grid), dim3(256), 0, c->stream, (const uint32_t*)b.var.p, (const uint32_t*)b.elem_off.p, b.n, b.r0, b.var_bytes,
                                           (const uint32_t*)P->digest.p, (uint64_t)P->read_id0, world, (unsigned long long*)cur.p, (DupItem*)nullptr, (uint32_t*)nullptr, (unsigned int*)d_bad.p);
            else hipLaunchKernelGGL(HIP_KERNEL_NAME(k_dup_items<true>), dim3(grid), dim3(256), 0, c->stream, (const uint32_t*)b.var.p, (const uint32_t*)b.elem_off.p, b.n, b.r0, b.var_bytes,
                                    (const uint32_t*)P->digest.p, (uint64_t)P->read_id0, world, (unsigned long long*)cur.p, (DupItem*)S->items.p, (uint32_t*)S->src.p, (unsigned int*)d_bad.p);
        }
    };
    sweep(false);
    HIP_TRY(hipGetLastError());
    uint64_t hcnt[64] = {};
    HIP_TRY(hipMemcpyAsync(hcnt, cur.p, 64 * 8, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    uint64_t starts[64] = {}, total = 0;
    for (uint32_t r = 0; r < world; ++r) { send_counts[r] = hcnt[r]; starts[r] = total; total += hcnt[r]; }
    if ((rc = c->alloc(S->items, std::max<uint64_t>(1, total) * sizeof(DupItem), "duplicate keys to send")) || (rc = c->alloc(S->src, std::max<uint64_t>(1, total) * 4, "duplicate key sources"))) return rc;
    S->n_items = total;
    HIP_TRY(hipMemcpyAsync(cur.p, starts, 64 * 8, hipMemcpyHostToDevice, c->stream));
    sweep(true);
    HIP_TRY(hipGetLastError());
    unsigned bad = 0;
    HIP_TRY(hipMemcpyAsync(&bad, d_bad.p, 4, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    c->release(cur); c->release(d_bad);
    if (bad & 1u) return fail(DFK_E_ARG, "duplicate marking packs a read's first edge in 29 bits and its offset in 25: this graph does not fit");
    *d_items = S->items.p;
    return 0;
    });
}

int dfk_shard_dup_answer(dfk_ctx* c, const void* d_items_in, uint64_t n_in, void* d_ans)
{
    return guarded([&]() -> int {
    if (!c || (n_in && (!d_items_in || !d_ans))) return fail(DFK_E_ARG, "null argument");
    HIP_TRY(hipSetDevice(c->device));
    if (!n_in) return 0;
    const unsigned cus = (unsigned)c->prop.multiProcessorCount;
    const uint64_t slots = 1ull << std::max<uint32_t>(10, ceil_log2(2 * n_in + 1024));
    DevBuf tk, tb, d_bad;
    int rc;
    if ((rc = c->alloc(tk, slots * 8, "duplicate keys", Place::Low)) || (rc = c->alloc(tb, slots * 8, "duplicate winners", Place::Low)) || (rc = c->alloc(d_bad, 16, "dup check", Place::Low))) return rc;
    hipLaunchKernelGGL(k_fill_u64, dim3(4096), dim3(256), 0, c->stream, (uint64_t*)tk.p, slots, ~0ull);
    HIP_TRY(hipMemsetAsync(tb.p, 0, slots * 8, c->stream));
    HIP_TRY(hipMemsetAsync(d_bad.p, 0, 16, c->stream));
    const unsigned grid = grid_256(n_in, cus);
    hipLaunchKernelGGL(HIP_KERNEL_NAME(k_dup_table<false>), dim3(grid), dim3(256), 0, c->stream, (const DupItem*)d_items_in, n_in, (unsigned long long*)tk.p, (unsigned long long*)tb.p, slots - 1, (uint8_t*)d_ans, (unsigned int*)d_bad.p);
    hipLaunchKernelGGL(HIP_KERNEL_NAME(k_dup_table<true>), dim3(grid), dim3(256), 0, c->stream, (const DupItem*)d_items_in, n_in, (unsigned long long*)tk.p, (unsigned long long*)tb.p, slots - 1, (uint8_t*)d_ans, (unsigned int*)d_bad.p);
    HIP_TRY(hipGetLastError());
    unsigned bad = 0;
    HIP_TRY(hipMemcpyAsync(&bad, d_bad.p, 4, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    c->release(tk); c->release(tb); c->release(d_bad);
    if (bad) return fail(DFK_E_HIP, "duplicate marking: a key vanished between its two passes");
    return 0;
    });
}

int dfk_shard_dup_write(dfk_ctx* c, const void* d_ans_back, uint64_t n, const char* path, uint64_t first_pair, uint64_t total_pairs, uint64_t* n_marked)
{
    return guarded([&]() -> int {
    PathState* P = built_paths(c);
    if (!P) return fail(DFK_E_STATE, "no paths: call dfk_paths_build");
    ShardPaths* S = shard_paths_of(P);
    if (n != S->n_items || (n && !d_ans_back) || !path) return fail(DFK_E_ARG, "the answers are not those of dfk_shard_dup_keys' items");
    HIP_TRY(hipSetDevice(c->device));
    const uint64_t n_pairs = P->n_reads / 2;
    if (first_pair + n_pairs > total_pairs) return fail(DFK_E_ARG, "this rank's pairs do not fit the file described");
    const unsigned cus = (unsigned)c->prop.multiProcessorCount;
    DevBuf dup, dg;
    int rc;
    if ((rc = c->alloc(dup, std::max<uint64_t>(1, n_pairs), "duplicate marks", Place::Low)) || (rc = c->alloc(dg, 32, "dup digest", Place::Low))) return rc;
    HIP_TRY(hipMemsetAsync(dup.p, 0, std::max<uint64_t>(1, n_pairs), c->stream));
    HIP_TRY(hipMemsetAsync(dg.p, 0, 32, c->stream));
    if (n) hipLaunchKernelGGL(k_dup_mark, dim3(grid_256(n, cus)), dim3(256), 0, c->stream, (const uint8_t*)d_ans_back, (const uint32_t*)S->src.p, n, (uint8_t*)dup.p);
    if (n_pairs) hipLaunchKernelGGL(HIP_KERNEL_NAME(k_digest_seq<uint8_t>), dim3(grid_256(n_pairs, cus)), dim3(256), 0, c->stream,
                                    (const uint8_t*)dup.p, n_pairs, 0x4444ull + first_pair, (unsigned long long*)dg.p);
    HIP_TRY(hipGetLastError());
    std::vector<uint8_t> h(n_pairs);
    uint64_t hd[4] = {};
    if (n_pairs) HIP_TRY(hipMemcpyAsync(h.data(), dup.p, n_pairs, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipMemcpyAsync(hd, dg.p, 32, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    c->release(dup); c->release(dg); c->release(S->items); c->release(S->src); S->n_items = 0;
    // (k_digest_seq hashes every position, marked or not: the unmarked positions' share is the same in every run of this size)
    P->ck[DFK_CK_DUP_DIGEST] = hd[0]; P->ck[DFK_CK_DUP_MARKED] = hd[2]; P->ck[DFK_CK_VALID] |= DFK_CK_HAS_DUPS;
    if (n_marked) *n_marked = hd[2];
    const int fd = open(path, O_WRONLY | O_CREAT, 0666);
    if (fd < 0) return fail(DFK_E_ARG, "cannot open %s", path);
    if (first_pair == 0) { char head[16]; memcpy(head, "BINWRITE", 8); memcpy(head + 8, &total_pairs, 8); if (pwrite(fd, head, 16, 0) != 16) rc = fail(DFK_E_ARG, "short write to %s", path); }
    if (!rc && ftruncate(fd, (off_t)(16 + total_pairs)) != 0) rc = fail(DFK_E_ARG, "cannot size %s", path);
    if (!rc && n_pairs && pwrite(fd, h.data(), n_pairs, (off_t)(16 + first_pair)) != (ssize_t)n_pairs) rc = fail(DFK_E_ARG, "short write to %s", path);
    if (close(fd) != 0 && !rc) rc = fail(DFK_E_ARG, "short write to %s", path);
    return rc;
    });
}

int dfk_bads_write_part(dfk_ctx* c, const char* path, uint64_t first_pair, uint64_t total_pairs, uint64_t* n_marked, uint64_t* digest)
{
    return guarded([&]() -> int {
    PathState* P = nullptr;
    if (int rc = bads_of(c, &P)) return rc;
    HIP_TRY(hipSetDevice(c->device));
    return bads_write(c, P, path, true, first_pair, total_pairs, 2 * first_pair, n_marked, digest);
    });
}

} // extern "C"
