// superplus_amd/csrc/dfk_paths.inc -- SURVEY 8(f)-2 (included by dfk.hip): every read pathed onto the graph dfk_graph_build
// left in the context, and the a.paths file.
//
// Reference being replaced (lib/assembly/src):
//   pathReads            paths/long/BuildReadQGraph48.cc:1420-1442: batches of reads through HBVPather (algorithmTwo,
//                        :1212-1317; Pather::path :685-733; ExtendReadPath) into an IncrementalWriter<ReadPath>
//   ReadPathVec::WriteAll 10X/WriteFiles.cc:78-82 -> a.<K>/a.paths (feudal file of ReadPath, paths/long/ReadPath.h:56-63)
// Kernels: dfk_paths_kernels.h.  Host side here: the HyperBasevector's tables as flat device arrays, the batch loop (the
// scratch of a batch -- parts, path room, decoded qualities -- is sized by the reads' k-mer counts), the file.
#include "dfk_check_kernels.h"
#include "dfk_paths_plan.h"   // the host decisions of everything here and in dfk_paths_shard.inc: batches, file layouts, ranges, passes, grids

namespace {

struct PathBatch { uint64_t r0 = 0, n = 0, var_bytes = 0, file_base = 0; DevBuf var, elem_off; };

// dfk_paths_sink: the file a.paths being written while the reads are still being pathed.  A thread of its own takes the
// finished batches' variable data to their places in the file; dfk_paths_write on the same path joins it and adds the rest.
struct PathSink {
    std::string path; int fd = -1;
    std::thread th; std::mutex mu; std::condition_variable cv;
    std::vector<struct PathBatch> queue; bool closed = false;        // closed: no more batches will come
    int rc = 0; std::string err;
};
void sink_abort(struct PathState* P);

struct PathState {
    dfk_ctx* c = nullptr;
    std::string sink_path;                             // asked for by dfk_paths_sink, for the next build
    PathSink* sink = nullptr;                          // the one at work (or done, waiting for dfk_paths_write)
    ~PathState() { sink_abort(this); if (shard && shard_free) shard_free(shard); if (sub && sub_free) sub_free(sub); if (closer && closer_free) closer_free(closer); if (partners && partners_free) partners_free(partners); if (cons && cons_free) cons_free(cons); if (translate && translate_free) translate_free(nullptr, translate); }
    DevBuf xlat, he_ce, he_left, he_right, from_start, from_vtx, from_edge, to_start, to_vtx, to_edge;
    bool tables = false;
    std::vector<PathBatch> batches;
    uint64_t n_reads = 0, n_placed = 0, n_edges = 0, var_total = 0;
    DevBuf digest;                                    // u32[n_reads]: first five bases | quality sum << 10 (k_read_digest), for MarkDups
    DevBuf bad_sums;                                  // u16[n_reads]: MarkBads' per-read sums (k_bad_sums), under DFK_F_MARK_BADS only
    std::vector<int32_t> hops;                        // FindEdgePairs' sorted pairs, two words each (dfk_hops_build, dfk_hops.inc): host memory
    uint64_t hops_stats[DFK_HOPS_WORDS] = {}; bool hops_valid = false;
    struct SubsetResult* sub = nullptr;               // the subset of interest (dfk_subset_build, dfk_subset.inc): host memory
    void (*sub_free)(struct SubsetResult*) = nullptr;
    struct CloserResult* closer = nullptr;            // the closers' read sets per edge (dfk_closer_build, dfk_closer.inc): host memory
    void (*closer_free)(struct CloserResult*) = nullptr;
    struct PartnersResult* partners = nullptr;        // the closers' unplaced partners (dfk_partners_build, dfk_partners.inc): host memory
    void (*partners_free)(struct PartnersResult*) = nullptr;
    struct ConsResult* cons = nullptr;                // the stacks' consensus per pair and side (dfk_cons_build, dfk_cons.inc): host memory
    void (*cons_free)(struct ConsResult*) = nullptr;
    struct TranslateResult* translate = nullptr;      // the paths on the patched graph (dfk_translate_build*, dfk_translate.inc): a second list of batches in the arena
    void (*translate_free)(dfk_ctx*, struct TranslateResult*) = nullptr;   // (a null context: the blocks have gone with the arena)
    uint64_t ck[DFK_CHECK_WORDS] = {};                // dfk_paths_digest: what the steps so far have left (ck[DFK_CK_VALID]: which)
    int64_t read_id0 = 0;                             // a rank of a sharded run: the whole set's number of its first read (dfk_paths_shard.inc)
    void* shard = nullptr; void (*shard_free)(void*) = nullptr;
    bool built = false;
    float ms = 0;
};

void path_state_free(PathState* p) { delete p; }      // (its device blocks belong to the arena: released with the graph or the run)

void paths_drop_results(dfk_ctx* c, PathState* P)
{
    for (PathBatch& b : P->batches) { c->release(b.var); c->release(b.elem_off); }
    c->release(P->digest); c->release(P->bad_sums);
    P->batches.clear(); P->built = false; P->n_reads = P->n_placed = P->n_edges = P->var_total = 0;
    P->hops.clear(); P->hops_valid = false;
    if (P->sub && P->sub_free) P->sub_free(P->sub);
    P->sub = nullptr;
    if (P->closer && P->closer_free) P->closer_free(P->closer);
    P->closer = nullptr;
    if (P->partners && P->partners_free) P->partners_free(P->partners);
    P->partners = nullptr;
    if (P->cons && P->cons_free) P->cons_free(P->cons);
    P->cons = nullptr;
    if (P->translate && P->translate_free) P->translate_free(c, P->translate);
    P->translate = nullptr;
    for (uint64_t& w : P->ck) w = 0;
}

template <class T> int upload_vec(dfk_ctx* c, DevBuf& d, const std::vector<T>& v, const char* what)
{
    int rc = c->alloc(d, std::max<size_t>(1, v.size()) * sizeof(T), what); if (rc) return rc;
    if (!v.empty()) HIP_TRY(hipMemcpyAsync(d.p, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));          // (v may be a temporary of the caller)
    return 0;
}

// Reads [r0, r0 + n) of paths given as host arrays (first[i] .. first[i + 1] of `edges` are read i's), laid out as k_path_emit
// leaves a batch: the offset word (offsets null: 0), a zero lastSkip word, then the edges; elem_off in bytes; an unplaced read is its
// two words alone.  What the entries that take arrays upload (dfk_hops_build_arrays, dfk_subset_build_arrays, dfk_paths_verify_arrays).
inline void layout_batch(const uint64_t* first, const int32_t* edges, const int32_t* offsets, uint64_t r0, uint64_t n,
                         std::vector<uint32_t>& var, std::vector<uint32_t>& off)
{
    var.clear(); off.resize(n);
    for (uint64_t i = 0; i < n; ++i) {
        off[i] = (uint32_t)(var.size() * 4);
        var.push_back(offsets ? (uint32_t)offsets[r0 + i] : 0u); var.push_back(0u);
        for (uint64_t k = first[r0 + i]; k < first[r0 + i + 1]; ++k) var.push_back((uint32_t)edges[k]);
    }
}

// fwdEdgeXlat / revEdgeXlat, ToLeft / ToRight and digraphE's adjacency (in its own sorted order: the extension rules take
// the first of equally good edges) as flat arrays
int paths_tables(dfk_ctx* c, HostGraph* G, PathState* P)
{
    if (P->tables) return 0;
    const size_t nCE = G->ce.size(), E = G->he.size(), V = (size_t)G->n_vertices;
    std::vector<int2> xlat(nCE);
    for (size_t i = 0; i < nCE; ++i) xlat[i] = int2{G->fwd[i], G->rev[i]};
    std::vector<uint32_t> he_ce(E); std::vector<int32_t> hl(E), hr(E);
    for (size_t e = 0; e < E; ++e) { he_ce[e] = (G->he[e].ce << 1) | G->he[e].rc; hl[e] = G->he[e].v; hr[e] = G->he[e].w; }
    const std::vector<uint32_t>& fs = G->from_start; const std::vector<uint32_t>& ts = G->to_start;
    const std::vector<int32_t>& fv = G->from_v; const std::vector<int32_t>& fe = G->from_e; const std::vector<int32_t>& tv = G->to_v; const std::vector<int32_t>& te = G->to_e;
    (void)V;
    int rc;
    if ((rc = upload_vec(c, P->xlat, xlat, "edge translation")) || (rc = upload_vec(c, P->he_ce, he_ce, "graph edges")) ||
        (rc = upload_vec(c, P->he_left, hl, "to_left")) || (rc = upload_vec(c, P->he_right, hr, "to_right")) ||
        (rc = upload_vec(c, P->from_start, fs, "from index")) || (rc = upload_vec(c, P->from_vtx, fv, "from")) || (rc = upload_vec(c, P->from_edge, fe, "from edges")) ||
        (rc = upload_vec(c, P->to_start, ts, "to index")) || (rc = upload_vec(c, P->to_vtx, tv, "to")) || (rc = upload_vec(c, P->to_edge, te, "to edges")))
        return rc;
    P->tables = true;
    return 0;
}

PathState* path_state_of(dfk_ctx* c, HostGraph* G)
{
    if (!G->paths) { G->paths = new PathState; G->paths->c = c; G->paths_free = path_state_free; }
    return G->paths;
}

int sink_open(dfk_ctx* c, PathState* P);
void sink_push(PathState* P, const PathBatch& B);
void sink_close(PathState* P);

PartTable part_table_of(dfk_ctx* c)
{
    PartTable pt{};
    pt.n_parts = 0;
    uint64_t at = 0;
    for (const dfk_ctx::Part& p : c->parts) { if (!p.n) continue; pt.start[pt.n_parts] = at; pt.ptr[pt.n_parts] = (uint4*)p.buf.p; ++pt.n_parts; at += p.n; }
    pt.start[pt.n_parts] = at;
    return pt;
}
PathGraph path_graph_of(HostGraph* G, PathState* P)
{
    return PathGraph{(const EdgeRec*)G->d_recs.p, (const uint8_t*)G->d_store.p, (const int2*)P->xlat.p, (const uint32_t*)P->he_ce.p,
                     (const int32_t*)P->he_left.p, (const int32_t*)P->he_right.p, (const uint32_t*)P->from_start.p, (const int32_t*)P->from_vtx.p,
                     (const int32_t*)P->from_edge.p, (const uint32_t*)P->to_start.p, (const int32_t*)P->to_vtx.p, (const int32_t*)P->to_edge.p,
                     (uint32_t)G->ce.size(), (uint32_t)G->he.size(), (uint32_t)G->n_vertices, (uint64_t)(G->d_store.bytes / 4)};
}

// the switches of dfk_paths_plan.h, as the environment sets them now
PathSwitches path_switches()
{
    PathSwitches sw;
    if (const char* e = getenv("DFK_PATH_SLOTS")) sw.slots = (uint32_t)std::max(1, atoi(e));
    sw.no_filter = getenv("DFK_NO_FILTER") != nullptr;
    if (const char* e = getenv("DFK_PATH_BATCH_READS")) sw.batch_reads = std::max<uint64_t>(1, (uint64_t)atoll(e));
    if (const char* e = getenv("DFK_PIDX_RANGE_PAIRS")) sw.pidx_range_pairs = std::max<uint64_t>(1, (uint64_t)atoll(e));
    if (const char* e = getenv("DFK_DUP_PASSES")) sw.dup_passes = (uint32_t)std::min<long long>(1024, std::max<long long>(1, atoll(e)));
    return sw;
}

template <int K>
int paths_build_typed(dfk_ctx* c, HostGraph* G, PathState* P, const Inputs& in)
{
    const double t_in = wall_now();
    sink_abort(P);                                                             // (a file begun by an earlier build and never finished)
    int rc = paths_tables(c, G, P); if (rc) return rc;
    TRACE("paths: %.3f s in, the graph's tables are on the device", wall_now() - t_in);
    paths_drop_results(c, P);
    rc = sink_open(c, P); if (rc) return rc;
    struct SinkGuard { PathState* P; bool ok = false; ~SinkGuard() { if (ok) sink_close(P); else sink_abort(P); } } sink_guard{P};
    const PartTable pt = part_table_of(c);
    const PathGraph pg = path_graph_of(G, P);
    Timer t(c->stream);
    t.start();
    c->release(c->good_len); c->good_len = DevBuf{};                           // (the count's, 4 bytes a read: the paths need the room)
    DevBuf ctr; rc = c->alloc(ctr, 32, "path counters"); if (rc) return rc;
    HIP_TRY(hipMemsetAsync(ctr.p, 0, 32, c->stream));
    const unsigned cus = (unsigned)c->prop.multiProcessorCount;
    const uint64_t n = in.n_reads;
    // The reads need not be the ones dfk_count saw (whose tables k_trim checked): the offset tables are checked again before
    // anything is read through them, and the longest read bounds a batch -- k_path_slots keeps two running sums in one
    // 64-bit scan (slots low, quality bytes high), neither of which may pass 2^32.
    uint32_t max_len = 0;
    if (n) {
        const unsigned g = grid_256(n, cus);
        hipLaunchKernelGGL(k_check_tables, dim3(g), dim3(256), 0, c->stream, in.base_off, in.packed_bytes, in.read_len, in.pq_off, in.pq_bytes, n, (unsigned int*)ctr.p);
        hipLaunchKernelGGL(k_max_u32, dim3(g), dim3(256), 0, c->stream, in.read_len, n, (unsigned int*)ctr.p + 1);
        HIP_TRY(hipGetLastError());
        unsigned h[2] = {};
        HIP_TRY(hipMemcpyAsync(h, ctr.p, 8, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
        if (h[0]) return fail(DFK_E_INPUT, "paths: an offset table is not monotone, runs past its array, or leaves a read fewer bytes than its bases need");
        max_len = h[1];
        if (max_len > 65535u) return fail(DFK_E_ARG, "paths: a read of %u bases (at most 65535)", max_len);
        HIP_TRY(hipMemsetAsync(ctr.p, 0, 32, c->stream));
    }
    // what MarkDups (row f-4) will want of every read, while the reads are here
    rc = c->alloc(P->digest, std::max<uint64_t>(1, n) * 4, "read digests"); if (rc) return rc;
    if (n) {
        hipLaunchKernelGGL(k_read_digest, dim3(grid_256(n, cus)), dim3(256), 0, c->stream, in.packed, in.base_off, in.read_len,
                           in.pq, in.pq_off, in.pq_bytes, n, (uint32_t*)P->digest.p);
        HIP_TRY(hipGetLastError());
    }
    // what MarkBads (10X/SecretOps.cc:71-109) will want of every read: asked for at dfk_create, since the reads are gone afterwards
    const bool mark_bads = (c->cfg.flags & DFK_F_MARK_BADS) != 0;
    if (mark_bads) { rc = c->alloc(P->bad_sums, std::max<uint64_t>(1, n) * 2, "bad-base sums"); if (rc) return rc; }
    std::unique_ptr<Timer> bads_timer(mark_bads ? new Timer(c->stream) : nullptr);
    float bads_ms = 0;                                                         // k_bad_sums alone, over the batches (dfk_stats.reserved[7])
    TRACE("paths: %.3f s in, tables checked, digests launched", wall_now() - t_in);
    // the filter in front of the index (dfk_paths_kernels.h): two bytes per k-mer, if the device has them to spare
    DevBuf filter;
    KmerFilter kf{nullptr, 0};
    const PathSwitches sw = path_switches();
    {
        const uint64_t n_kmers = pt.start[pt.n_parts], free_now = c->largest_allocatable();
        const PathFilterPlan fp = plan_path_filter(n_kmers, n, free_now, G->d_filter.p ? G->filter_words : 0, sw.no_filter);
        if (fp.use == PathFilter::Reuse) {                                     // made under the graph's numbering (dfk_graph.inc)
            filter = G->d_filter; G->d_filter = DevBuf{}; G->filter_words = 0;
        } else if (fp.use == PathFilter::Build) {
            rc = c->alloc(filter, fp.words * 4, "k-mer filter"); if (rc) return rc;
            HIP_TRY(hipMemsetAsync(filter.p, 0, fp.words * 4, c->stream));
            hipLaunchKernelGGL(HIP_KERNEL_NAME(k_filter_build<K>), dim3(grid_256(n_kmers, cus)), dim3(256), 0, c->stream,
                               pt, n_kmers, (uint32_t*)filter.p, fp.words);
            HIP_TRY(hipGetLastError());
        } else TRACE("paths: no room for the k-mer filter (%.1f GB free)", free_now / 1e9);
        if (filter.p) kf = KmerFilter{(const uint32_t*)filter.p, fp.words};
    }
    // the batches: PathBatcher (dfk_paths_plan.h) says which reads, with how many slots, in what room and where in the file
    PathBatcher bp(n, path_batch_bound(max_len, (uint32_t)K), sw);
    uint64_t placed = 0, path_edges = 0;
    unsigned bad = 0;
    while (bp.more()) {
        bp.begin(c->largest_allocatable());
        const uint64_t r0 = bp.r0;
        DevBuf slots, slot_off;
        uint64_t total = 0, qtotal = 0;
        for (;;) {                                                              // shrink until the real scratch fits
            rc = c->alloc(slots, (bp.nb + 1) * 8, "path slots", Place::Low); if (rc) return rc;
            rc = c->alloc(slot_off, (bp.nb + 1) * 8, "path slot offsets", Place::Low); if (rc) return rc;
            hipLaunchKernelGGL(k_path_slots, dim3(grid_256(bp.nb, cus, 16)), dim3(256), 0, c->stream, in.read_len, r0, bp.nb, (uint32_t)K, bp.cap, (uint64_t*)slots.p);
            HIP_TRY(hipMemsetAsync((uint64_t*)slots.p + bp.nb, 0, 8, c->stream));
            rc = device_scan(c, (const uint64_t*)slots.p, (uint64_t*)slot_off.p, bp.nb + 1); if (rc) return rc;
            uint64_t both = 0;
            HIP_TRY(hipMemcpyAsync(&both, (uint64_t*)slot_off.p + bp.nb, 8, hipMemcpyDeviceToHost, c->stream));
            HIP_TRY(hipStreamSynchronize(c->stream));
            total = both & 0xFFFFFFFFull; qtotal = both >> 32;
            if (bp.fits(total, qtotal)) break;
            c->release(slots); c->release(slot_off);
        }
        c->release(slots);
        const uint64_t nb = bp.nb;
        const unsigned grid = grid_256(nb, cus, 16), pgrid = grid_256(nb, cus, 64);
        const PathScratch sz = bp.scratch(total, qtotal);
        static_assert(sizeof(PartD) == 16, "PathScratch counts 16 bytes a part");
        DevBuf parts, path, quals, o_off, o_len, o_first, sizes, size_off;
        PathBatch B; B.r0 = r0; B.n = nb; B.file_base = bp.file_base;
        if ((rc = c->alloc(parts, sz.parts, "path parts", Place::Low)) || (rc = c->alloc(path, sz.path, "path room", Place::Low)) ||
            (rc = c->alloc(quals, sz.quals, "decoded qualities", Place::Low)) ||
            (rc = c->alloc(o_off, sz.o_off, "path offsets", Place::Low)) || (rc = c->alloc(o_len, sz.o_len, "path lengths", Place::Low)) ||
            (rc = c->alloc(o_first, sz.o_first, "path starts", Place::Low)) ||
            (rc = c->alloc(sizes, sz.sizes, "element sizes", Place::Low)) || (rc = c->alloc(size_off, sz.size_off, "element offsets", Place::Low)))
            return rc;
        HIP_TRY(hipMemsetAsync(ctr.p, 0, 32, c->stream));                        // this batch's: reads placed, path edges, flags
        hipLaunchKernelGGL(HIP_KERNEL_NAME(k_path_reads<K>), dim3(pgrid), dim3(256), 0, c->stream, pt, (const uint32_t*)G->d_index.p, G->index_slots, kf, pg,
                           in.packed, in.packed_bytes, in.base_off, in.read_len, in.pq, in.pq_off, r0, nb, (const uint64_t*)slot_off.p,
                           (PartD*)parts.p, (int32_t*)path.p, (uint8_t*)quals.p, (int32_t*)o_off.p, (uint32_t*)o_len.p, (uint32_t*)o_first.p,
                           (unsigned long long*)ctr.p, (unsigned int*)((char*)ctr.p + 16));
        hipLaunchKernelGGL(k_path_sizes, dim3(grid), dim3(256), 0, c->stream, (const uint32_t*)o_len.p, nb, (uint64_t*)sizes.p);
        HIP_TRY(hipMemsetAsync((uint64_t*)sizes.p + nb, 0, 8, c->stream));
        HIP_TRY(hipGetLastError());
        rc = device_scan(c, (const uint64_t*)sizes.p, (uint64_t*)size_off.p, nb + 1); if (rc) return rc;
        uint64_t h[4] = {};
        HIP_TRY(hipMemcpyAsync(&B.var_bytes, (uint64_t*)size_off.p + nb, 8, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipMemcpyAsync(h, ctr.p, 32, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
        const bool again = ((unsigned)h[2] & 32u) != 0;                          // a read wants more slots than it was given
        if (!again) {
            bad |= (unsigned)h[2]; placed += h[0]; path_edges += h[1];
            if (B.var_bytes >= (1ull << 32)) return fail(DFK_E_ARG, "a batch of %llu reads holds %llu bytes of paths: its offsets keep 32 bits", (unsigned long long)nb, (unsigned long long)B.var_bytes);
            if ((rc = c->alloc(B.var, std::max<uint64_t>(4, B.var_bytes), "a.paths data")) || (rc = c->alloc(B.elem_off, nb * 4, "a.paths offsets"))) return rc;
            hipLaunchKernelGGL(k_path_emit, dim3(grid), dim3(256), 0, c->stream, (const uint64_t*)size_off.p, (const uint64_t*)slot_off.p, (const int32_t*)path.p,
                               (const int32_t*)o_off.p, (const uint32_t*)o_len.p, (const uint32_t*)o_first.p, nb, (uint32_t*)B.var.p, (uint32_t*)B.elem_off.p);
            unsigned bflag = 0;
            if (mark_bads) {                                                  // on the paths that stay: this attempt's, as k_path_emit left them
                bads_timer->start();
                hipLaunchKernelGGL(HIP_KERNEL_NAME(k_bad_sums<K>), dim3(pgrid), dim3(256), 0, c->stream, pg, in.packed, in.packed_bytes, in.base_off, in.read_len,
                                   in.pq, in.pq_off, (const uint32_t*)B.var.p, (const uint32_t*)B.elem_off.p, nb, r0, B.var_bytes,
                                   (uint16_t*)P->bad_sums.p, (unsigned int*)((char*)ctr.p + 24));
                bads_ms += bads_timer->stop();
                HIP_TRY(hipMemcpyAsync(&bflag, (char*)ctr.p + 24, 4, hipMemcpyDeviceToHost, c->stream));
            }
            HIP_TRY(hipGetLastError());
            HIP_TRY(hipStreamSynchronize(c->stream));
            bad |= bflag;
        }
        c->release(parts); c->release(path); c->release(quals); c->release(o_off); c->release(o_len); c->release(o_first);
        c->release(sizes); c->release(size_off); c->release(slot_off);
        if (!again) { P->batches.push_back(B); sink_push(P, B); }
        else TRACE("paths: a read of [%llu, %llu) wants more than %u slots: the batch again with all", (unsigned long long)r0, (unsigned long long)(r0 + nb), sw.slots);
        bp.end(again, B.var_bytes);
    }
    TRACE("paths: %.3f s in, the last batch is launched", wall_now() - t_in);
    c->release(ctr);
    if (filter.p) c->release(filter);
    P->ms = t.stop();
    TRACE("paths: %.3f s in, the device is done", wall_now() - t_in);
    if (bad & 4u) return fail(DFK_E_STATE, "paths: a dictionary entry without an edge (the graph does not belong to this dictionary)");
    if (bad & 8u) return fail(DFK_E_HIP, "paths: a path outgrew its read's k-mer count (bound of the scratch layout violated)");
    if (bad & 16u) return fail(DFK_E_INPUT, "paths: a read's PQVec does not hold one quality per base");
    P->n_reads = n; P->n_placed = placed; P->n_edges = path_edges; P->var_total = bp.file_base - 24; P->built = true;
    {   // dfk_paths_digest: the file's elements, whatever batches they were made in
        const unsigned dgrid = 32u * cus;                                       // (a slot pair per block, then the fold: see k_paths_digest)
        DevBuf dg; rc = c->alloc(dg, 32 + 16ull * dgrid, "paths digest", Place::Low); if (rc) return rc;
        HIP_TRY(hipMemsetAsync(dg.p, 0, 32 + 16ull * dgrid, c->stream));
        unsigned long long* slots = (unsigned long long*)dg.p + 4;
        for (const PathBatch& b : P->batches)
            hipLaunchKernelGGL(k_paths_digest, dim3(grid_256(b.n, cus)), dim3(256), 0, c->stream, (const uint32_t*)b.var.p,
                               (const uint32_t*)b.elem_off.p, b.n, b.r0 + (uint64_t)P->read_id0, b.var_bytes, slots);
        hipLaunchKernelGGL(k_paths_digest_fold, dim3(1), dim3(256), 0, c->stream, (const unsigned long long*)slots, dgrid, (unsigned long long*)dg.p);
        HIP_TRY(hipGetLastError());
        uint64_t h[2] = {};
        HIP_TRY(hipMemcpyAsync(h, dg.p, 16, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
        c->release(dg);
        P->ck[DFK_CK_PATHS_SUM] = h[0]; P->ck[DFK_CK_PATHS_XOR] = h[1];
        P->ck[DFK_CK_N_READS] = n; P->ck[DFK_CK_N_PLACED] = placed; P->ck[DFK_CK_N_PATH_EDGES] = path_edges;
        P->ck[DFK_CK_VALID] = DFK_CK_HAS_PATHS;
    }
    sink_guard.ok = true;
    c->st.reserved[3] = (uint64_t)(P->ms * 1000.0f);                           // microseconds spent pathing
    if (mark_bads) c->st.reserved[7] = (uint64_t)(bads_ms * 1000.0f);          // ... of which in k_bad_sums
    TRACE("paths: %llu reads, %llu placed, %llu path edges, %zu batches, %.1f ms", (unsigned long long)n, (unsigned long long)P->n_placed,
          (unsigned long long)P->n_edges, P->batches.size(), P->ms);
    return 0;
}

int paths_build_any(dfk_ctx* c, const Inputs& in)
{
    if (!c->have) return fail(DFK_E_STATE, "no completed count");
    if (!c->graph_state || !graph_of(c)->built) return fail(DFK_E_STATE, "no graph: call dfk_graph_build first");
    if (!graph_of(c)->d_index.p) return fail(DFK_E_STATE, "the graph's k-mer index was given back by dfk_paths_index_write / dfk_dups_write: call dfk_graph_build again");
    if (in.n_reads >= (1ull << 32)) return fail(DFK_E_ARG, "more than 2^32-1 reads (a feudal file counts its elements in 32 bits)");
    HostGraph* G = graph_of(c);
    PathState* P = path_state_of(c, G);
    const uint64_t mark = c->alloc_seq;
    const bool had_tables = P->tables;
    int rc;
    try {
        switch (c->cfg.K) {
        case 40: rc = paths_build_typed<40>(c, G, P, in); break;
        case 48: rc = paths_build_typed<48>(c, G, P, in); break;
        default: rc = paths_build_typed<60>(c, G, P, in); break;
        }
    } catch (const std::runtime_error& e) { rc = fail(DFK_E_HIP, "%s", e.what()); }
    if (rc) {
        (void)hipStreamSynchronize(c->stream);
        c->release_since(mark);
        P->batches.clear(); P->built = false; P->digest = P->bad_sums = DevBuf{};
        if (!had_tables) { P->tables = false; P->xlat = P->he_ce = P->he_left = P->he_right = P->from_start = P->from_vtx = P->from_edge = P->to_start = P->to_vtx = P->to_edge = DevBuf{}; }
    }
    return rc;
}

// A range of a file whose pages EXIST (fallocate, or written before), mapped: lanes that copy into it need no turn at the file
// -- pwrite()s to one inode take turns, at 6-10 GB/s on the GPU box's tmpfs whatever their number -- provided every piece is
// entered into the page table with one call first (MADV_POPULATE_WRITE, Linux 5.14): 26 GB/s from four lanes, 49 from eight,
// against 9 and 11 when each page faults for itself, and 4 on a file that was only ftruncate()d (tools/tmpfs_write.cc,
// profiles/r04_tmpfs_write.txt).
struct FileMap {
    char* p = nullptr; uint64_t lo = 0, hi = 0;                          // file bytes [lo, hi) at p (lo a multiple of the page size)
    bool map(int fd, uint64_t from, uint64_t to)
    {
        drop();
        lo = from & ~4095ull; hi = to;
        if (hi <= lo) { lo = hi = 0; return false; }
        void* q = mmap(nullptr, (size_t)(hi - lo), PROT_READ | PROT_WRITE, MAP_SHARED, fd, (off_t)lo);
        if (q == MAP_FAILED) { lo = hi = 0; return false; }
        p = (char*)q;
        return true;
    }
    char* at(uint64_t file_off, uint64_t bytes) const { return p && file_off >= lo && file_off + bytes <= hi ? p + (file_off - lo) : nullptr; }
    void drop() { if (p) (void)munmap(p, (size_t)(hi - lo)); p = nullptr; lo = hi = 0; }
    ~FileMap() { drop(); }
};

// device bytes -> a file, through the transfer lanes (FilePiece, dfk_paths_plan.h: where from, how many, where to, widened
// or not); one writer at a time.
int write_pieces(dfk_ctx* c, int fd, const std::vector<FilePiece>& pieces, const FileMap* fm = nullptr)
{
    struct Pending { uint64_t bytes = 0, file_off = 0, add = 0; bool widen = false, live = false; };
    std::vector<Pending> pend(2 * (size_t)xfer_threads());
    std::vector<std::vector<uint64_t>> wide(xfer_threads());
    std::mutex file_turn;
    auto flush = [&](XferLane& l, unsigned t, int k) -> int {
        Pending& p = pend[2 * t + k];
        if (!p.live) return 0;
        HIP_TRY(hipEventSynchronize(l.ev[k]));
        const char* data = (const char*)l.pin[k];
        uint64_t nbytes = p.bytes;
        if (char* dst = fm ? fm->at(p.file_off, p.widen ? 2 * p.bytes : p.bytes) : nullptr) {      // pages that exist, mapped: no turn to wait for
            const uint64_t out = p.widen ? 2 * p.bytes : p.bytes;
            const uintptr_t a = (uintptr_t)dst & ~(uintptr_t)4095, b = std::min<uintptr_t>(((uintptr_t)dst + out + 4095) & ~(uintptr_t)4095, (uintptr_t)fm->p + (((fm->hi - fm->lo) + 4095) & ~4095ull));
            (void)madvise((void*)a, b - a, 23 /* MADV_POPULATE_WRITE */);     // (an older kernel refuses: the copy then faults the pages in one by one)
            if (p.widen) {
                const uint32_t* v = (const uint32_t*)l.pin[k];
                for (uint64_t i = 0; i < p.bytes / 4; ++i) { const uint64_t x = (uint64_t)v[i] + p.add; memcpy(dst + 8 * i, &x, 8); }
            } else memcpy(dst, data, nbytes);
            p.live = false;
            return 0;
        }
        if (p.widen) {
            std::vector<uint64_t>& w = wide[t];
            const uint64_t n = p.bytes / 4;
            w.resize(n);
            const uint32_t* v = (const uint32_t*)l.pin[k];
            for (uint64_t i = 0; i < n; ++i) w[i] = (uint64_t)v[i] + p.add;
            data = (const char*)w.data(); nbytes = 8 * n;
        }
        {
            std::lock_guard<std::mutex> turn(file_turn);
            for (uint64_t done = 0; done < nbytes;) {
                const ssize_t wr = pwrite(fd, data + done, nbytes - done, (off_t)(p.file_off + done));
                if (wr <= 0) return fail(DFK_E_ARG, "short write");
                done += (uint64_t)wr;
            }
        }
        p.live = false;
        return 0;
    };
    return xfer_run(c, pieces.size(),
        [&](unsigned t, XferLane& l, uint64_t i) -> int {
            const int k = l.turn++ & 1;
            int r = flush(l, t, k); if (r) return r;
            const FilePiece& pc = pieces[i];
            HIP_TRY(hipMemcpyAsync(l.pin[k], pc.src, pc.bytes, hipMemcpyDeviceToHost, l.st));
            HIP_TRY(hipEventRecord(l.ev[k], l.st));
            pend[2 * t + k] = Pending{pc.bytes, pc.file_off, pc.add, pc.widen, true};
            return flush(l, t, k ^ 1);
        },
        [&](unsigned t, XferLane& l) -> int { int r = flush(l, t, 0); return r ? r : flush(l, t, 1); });
}

// A list of batches as a feudal file of ReadPath into the open `fd`, which is closed: the control block, the size, the last offset, then
// the batches' data as it is (`streamed`: it is in the file already) and their elements' absolute file offsets -- the 32-bit ones kept
// per read, widened in the transfer lanes.  Nothing is allocated on the device.  dfk_paths_write's a.paths and dfk_translate_write's
// a.patch.paths (dfk_translate.inc).
int path_batches_to_file(dfk_ctx* c, int fd, const char* path, const FeudalLayout& lay, uint64_t n, const std::vector<PathBatch>& batches, bool streamed)
{
    const uint64_t var_tab = lay.var_tab;
    int rc = pwrite(fd, &lay.head, 24, 0) == 24 ? 0 : fail(DFK_E_ARG, "short write to %s", path);
    if (!rc && ftruncate(fd, (off_t)lay.file_size) != 0) rc = fail(DFK_E_ARG, "cannot size %s", path);
    const uint64_t last = var_tab;                                            // the (n+1)-th offset: the end of the variable data
    if (!rc && pwrite(fd, &last, 8, (off_t)(var_tab + 8 * n)) != 8) rc = fail(DFK_E_ARG, "short write to %s", path);
    if (!rc) {
        std::vector<FilePiece> pieces;
        for (const PathBatch& b : batches) {
            if (!streamed) append_pieces(pieces, (const char*)b.var.p, b.var_bytes, b.file_base, XFER_CHUNK);
            append_wide_pieces(pieces, (const char*)b.elem_off.p, b.n * 4, var_tab + 8 * b.r0, b.file_base, XFER_CHUNK);
        }
        rc = write_pieces(c, fd, pieces);
        if (rc) rc = fail(DFK_E_ARG, "short write to %s", path);
    }
    if (close(fd) != 0 && !rc) rc = fail(DFK_E_ARG, "short write to %s", path);
    return rc;
}

// ---- dfk_paths_sink (see PathSink)
void sink_loop(dfk_ctx* c, PathSink* S)
{
    (void)hipSetDevice(c->device);
    for (;;) {
        std::vector<PathBatch> take;
        {
            std::unique_lock<std::mutex> lk(S->mu);
            S->cv.wait(lk, [&] { return !S->queue.empty() || S->closed; });
            if (S->queue.empty()) return;
            take.swap(S->queue);
        }
        if (S->rc) continue;                                                   // (a failed file: the rest is only taken off the queue)
        std::vector<FilePiece> pieces;
        for (const PathBatch& b : take) append_pieces(pieces, (const char*)b.var.p, b.var_bytes, b.file_base, XFER_CHUNK);
        if (write_pieces(c, S->fd, pieces)) { S->rc = DFK_E_ARG; S->err = std::string("short write to ") + S->path + " (" + dfk_last_error() + ")"; }
    }
}
int sink_open(dfk_ctx* c, PathState* P)
{
    if (P->sink_path.empty()) return 0;
    PathSink* S = new PathSink;
    S->path = P->sink_path;
    // A file that is there is NOT truncated (dfk_paths_write sets the size at the end): a caller that can guess how large a.paths
    // will be may have made its pages beforehand (fallocate, while the GPU counted), and a pwrite into pages that exist does not
    // allocate them under the file's lock -- at configs[1] what is left to write after the pathing takes 2.0-2.7 s instead of
    // 3.4-3.8 (DESIGN.md section 14).
    S->fd = open(S->path.c_str(), O_WRONLY | O_CREAT, 0666);
    if (S->fd < 0) { const std::string p = S->path; delete S; return fail(DFK_E_ARG, "cannot open %s", p.c_str()); }
    S->th = std::thread(sink_loop, c, S);
    P->sink = S;
    return 0;
}
void sink_push(PathState* P, const PathBatch& B)
{
    if (!P->sink) return;
    { std::lock_guard<std::mutex> lk(P->sink->mu); P->sink->queue.push_back(B); }
    P->sink->cv.notify_one();
}
void sink_close(PathState* P)
{
    if (!P->sink) return;
    { std::lock_guard<std::mutex> lk(P->sink->mu); P->sink->closed = true; }
    P->sink->cv.notify_one();
}
// the thread's work done (all of the variable data is in the file, or an error is): the descriptor goes to the caller
int sink_finish(PathState* P, int* fd)
{
    PathSink* S = P->sink;
    sink_close(P);
    if (S->th.joinable()) S->th.join();
    const int rc = S->rc; const std::string err = S->err;
    *fd = S->fd;
    P->sink = nullptr;
    delete S;
    if (rc) { close(*fd); *fd = -1; return fail(rc, "%s", err.c_str()); }
    return 0;
}
void sink_abort(PathState* P)
{
    if (!P->sink) return;
    int fd = -1;
    const std::string path = P->sink->path;
    (void)sink_finish(P, &fd);
    if (fd >= 0) close(fd);
    unlink(path.c_str());
}

// stable LSD radix sort of (key, value) pairs by the low `bits` bits of the key, eight bits a pass (k_rs_hist / k_rs_scatter):
// the sorted pairs end in k[*cur], v[*cur]
int radix_sort_pairs(dfk_ctx* c, DevBuf k[2], DevBuf v[2], uint64_t n, uint32_t bits, int* cur)
{
    if (!n) return 0;
    const unsigned cus = (unsigned)c->prop.multiProcessorCount;
    const uint64_t n_tiles = (n + RS_TILE - 1) / RS_TILE;
    DevBuf hist, place;
    int rc;
    if ((rc = c->alloc(hist, 256 * n_tiles * 8, "sort counts", Place::Low)) || (rc = c->alloc(place, 256 * n_tiles * 8, "sort places", Place::Low))) return rc;
    const unsigned sgrid = (unsigned)std::min<uint64_t>((n_tiles + RS_WAVES - 1) / RS_WAVES, 16ull * cus);
    for (uint32_t shift = 0; shift < bits; shift += 8) {
        hipLaunchKernelGGL(k_rs_hist, dim3(sgrid), dim3(64 * RS_WAVES), 0, c->stream, (const uint32_t*)k[*cur].p, n, shift, n_tiles, (uint64_t*)hist.p);
        HIP_TRY(hipGetLastError());
        rc = device_scan(c, (const uint64_t*)hist.p, (uint64_t*)place.p, 256 * n_tiles); if (rc) return rc;
        hipLaunchKernelGGL(k_rs_scatter, dim3(sgrid), dim3(64 * RS_WAVES), 0, c->stream, (const uint32_t*)k[*cur].p, (const uint32_t*)v[*cur].p, n, shift, n_tiles,
                           (const uint64_t*)place.p, (uint32_t*)k[*cur ^ 1].p, (uint32_t*)v[*cur ^ 1].p);
        HIP_TRY(hipGetLastError());
        *cur ^= 1;
    }
    HIP_TRY(hipStreamSynchronize(c->stream));
    c->release(hist); c->release(place);
    return 0;
}

// ---- row f-4
// writePathsIndex (10X/PathsIndex.cc:23-146): a.paths.inv + a.countsb
// (dir empty: everything but the files -- the tables are built and digested for dfk_paths_digest)
// The index is built one RANGE OF EDGES at a time: a range's (edge, read) pairs are listed in read order, sorted by edge and
// written as that part of the file.  One range when everything fits (the usual case: 1.76e9 entries at configs[1]); several when
// the room is short or the paths hold 2^31 entries or more (a real genome has two or three edges a read) -- the reference's own
// 30 chunk files (PathsIndex.cc:32-99) are the same idea for the same reason.  DFK_PIDX_RANGE_PAIRS forces small ranges (tests).
// dfk_paths_index_dups_write: the lists of a.paths.inv (14 GB at configs[1]) leave the device and enter the file in a thread
// of their own while the caller goes on to mark duplicates -- the thread allocates nothing (the arena belongs to the caller's
// thread), the block it reads was taken before the index's scratch and is given back by finish().
struct IndexTail {
    DevBuf var; int fd = -1; std::thread th; int rc = 0; std::string err;
    int finish(dfk_ctx* c)
    {
        if (th.joinable()) th.join();
        if (fd >= 0 && close(fd) != 0 && !rc) { rc = DFK_E_ARG; err = "short write to a.paths.inv"; }
        fd = -1;
        c->release(var);
        return rc ? fail(rc, "%s", err.c_str()) : 0;
    }
};

int paths_index_write(dfk_ctx* c, HostGraph* G, PathState* P, const std::string& dir, IndexTail* tail = nullptr)
{
    const uint64_t n_pairs = P->n_edges, n_he = G->he.size();
    if (!n_he) return fail(DFK_E_STATE, "the graph has no edges (the reference asserts the same, PathsIndex.cc:29)");
    const unsigned cus = (unsigned)c->prop.multiProcessorCount;
    const PathSwitches sw = path_switches();
    if (tail && (!pidx_tail_applies(!dir.empty(), n_pairs, c->largest_allocatable()) || c->alloc(tail->var, 8 * n_pairs, "a.paths.inv data", Place::Low))) tail = nullptr;
    const uint64_t mark = c->alloc_seq;
    int fd = -1;
    uint64_t had = 0;                                                    // bytes a.paths.inv had when it was opened (pages the caller made)
    auto body = [&]() -> int {
        DevBuf counts, first, c64, eo, csb, d_inv;
        int rc;
        // ---- reads per edge, where each edge's list starts, the counts with the involuted edge's added
        if ((rc = c->alloc(counts, n_he * 4, "reads per edge", Place::Low))) return rc;
        HIP_TRY(hipMemsetAsync(counts.p, 0, n_he * 4, c->stream));
        uint64_t listed = 0;
        for (const PathBatch& b : P->batches) {
            hipLaunchKernelGGL(k_pidx_count, dim3(grid_256(b.n, cus)), dim3(256), 0, c->stream, (const uint32_t*)b.var.p,
                               (const uint32_t*)b.elem_off.p, b.n, b.var_bytes, (uint32_t*)counts.p);
            listed += b.var_bytes / 4 - 2 * b.n;
        }
        HIP_TRY(hipGetLastError());
        if (listed != n_pairs) return fail(DFK_E_HIP, "paths index: %llu path entries listed, %llu counted", (unsigned long long)listed, (unsigned long long)n_pairs);
        std::vector<int32_t> inv(n_he);
        for (size_t e = 0; e < n_he; ++e) inv[e] = G->he[e].rc ? G->fwd[G->he[e].ce] : G->rev[G->he[e].ce];
        if ((rc = upload_vec(c, d_inv, inv, "involution")) || (rc = c->alloc(c64, (n_he + 1) * 8, "counts", Place::Low)) || (rc = c->alloc(first, (n_he + 1) * 8, "list starts", Place::Low)) ||
            (rc = c->alloc(eo, (n_he + 1) * 8, "list offsets", Place::Low)) || (rc = c->alloc(csb, n_he * 4, "countsb", Place::Low))) return rc;
        const unsigned egrid = grid_256(n_he + 1, cus);                      // (+ 1: these launches have always had (n + 256) / 256 blocks)
        HIP_TRY(hipMemsetAsync(c64.p, 0, (n_he + 1) * 8, c->stream));
        hipLaunchKernelGGL(k_widen_u32, dim3(egrid), dim3(256), 0, c->stream, (const uint32_t*)counts.p, n_he, (uint64_t*)c64.p);
        HIP_TRY(hipGetLastError());
        rc = device_scan(c, (const uint64_t*)c64.p, (uint64_t*)first.p, n_he + 1); if (rc) return rc;
        hipLaunchKernelGGL(k_pidx_tables, dim3(egrid), dim3(256), 0, c->stream, (const uint32_t*)counts.p, (const uint64_t*)first.p, (const int32_t*)d_inv.p, n_he,
                           (uint64_t*)eo.p, (int32_t*)csb.p);
        HIP_TRY(hipGetLastError());
        std::vector<uint64_t> h_first(n_he + 1);
        HIP_TRY(hipMemcpyAsync(h_first.data(), first.p, (n_he + 1) * 8, hipMemcpyDeviceToHost, c->stream));
        // dfk_paths_digest: where the lists start, the summed counts (the lists themselves range by range below)
        DevBuf dg; if ((rc = c->alloc(dg, 128, "index digest", Place::Low))) return rc;
        HIP_TRY(hipMemsetAsync(dg.p, 0, 128, c->stream));
        unsigned long long* d = (unsigned long long*)dg.p;
        hipLaunchKernelGGL(HIP_KERNEL_NAME(k_digest_seq<uint64_t>), dim3(egrid), dim3(256), 0, c->stream, (const uint64_t*)first.p, n_he + 1, 0x2222ull, d + 4);
        hipLaunchKernelGGL(HIP_KERNEL_NAME(k_digest_seq<uint32_t>), dim3(egrid), dim3(256), 0, c->stream, (const uint32_t*)csb.p, n_he, 0x3333ull, d + 8);
        hipLaunchKernelGGL(k_self_inverse_sum, dim3(egrid), dim3(256), 0, c->stream, (const uint32_t*)counts.p, (const int32_t*)d_inv.p, n_he, d + 12);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipStreamSynchronize(c->stream));
        if (h_first[n_he] != n_pairs) return fail(DFK_E_HIP, "paths index: the per-edge counts add up to %llu, the paths hold %llu entries", (unsigned long long)h_first[n_he], (unsigned long long)n_pairs);
        c->release(c64); c->release(first); c->release(d_inv);
        // ---- the files' fixed parts
        const FeudalLayout lay = feudal_layout(n_he, 16, 8, 8 * n_pairs);
        const std::string path = dir + "/a.paths.inv";
        if (!dir.empty()) {
            // a.paths.inv: feudal file of SerfVec<unsigned long> (IncrementalWriter<ULongVec>, :76): control block {n, 1, 0, 16, 8}, the
            // ids, n+1 absolute offsets
            // (not truncated either: pages made beforehand are used, the size is set here -- and when they were ALL there, the lists
            // go in through a mapping, every lane at once: FileMap)
            fd = open(path.c_str(), O_RDWR | O_CREAT, 0666);
            if (fd < 0) return fail(DFK_E_ARG, "cannot open %s", path.c_str());
            { struct stat sb; had = fstat(fd, &sb) == 0 ? (uint64_t)sb.st_size : 0; }
            if (!(pwrite(fd, &lay.head, 24, 0) == 24 && ftruncate(fd, (off_t)lay.file_size) == 0)) return fail(DFK_E_ARG, "short write to %s", path.c_str());
            std::vector<FilePiece> pieces;
            append_pieces(pieces, (const char*)eo.p, 8 * (n_he + 1), lay.var_tab, XFER_CHUNK);
            if (write_pieces(c, fd, pieces)) return fail(DFK_E_ARG, "short write to %s", path.c_str());
            // a.countsb: BinaryWriter::writeFile of vec<vec<int>> with one row (:64,131)
            std::vector<int32_t> hc(n_he);
            HIP_TRY(hipMemcpy(hc.data(), csb.p, n_he * 4, hipMemcpyDeviceToHost));
            try { OutFile f(dir + "/a.countsb"); f.raw("BINWRITE", 8); f.pod<uint64_t>(1); f.vec_i32(hc); f.close(); }
            catch (const std::runtime_error& e) { return fail(DFK_E_ARG, "%s", e.what()); }
        }
        c->release(eo); c->release(csb); c->release(counts);
        // ---- the lists, a range of edges at a time: 24 bytes per entry while a range is sorted and widened
        const uint64_t cap = pidx_range_cap(c->largest_allocatable(), sw.pidx_range_pairs);
        uint32_t n_ranges = 0;
        for (uint64_t e0 = 0; e0 < n_he;) {
            const PidxRange range = pidx_next_range(h_first.data(), n_he, e0, cap);
            const uint64_t e1 = range.e1, n_r = range.n;
            if (!range.ok) return fail(DFK_E_ARG, "edge %llu alone is on %llu reads: a range of the paths index sorts 32-bit positions", (unsigned long long)e0, (unsigned long long)n_r);
            ++n_ranges;
            if (n_r) {
                DevBuf k[2], v[2], var;
                for (int i = 0; i < 2; ++i) { if ((rc = c->alloc(k[i], n_r * 4, "index keys", Place::Low)) || (rc = c->alloc(v[i], n_r * 4, "index reads", Place::Low))) return rc; }
                const bool whole = e0 == 0 && e1 == n_he;
                if (tail && !whole) { c->release(tail->var); tail = nullptr; }      // (several ranges: each is written before the next is sorted)
                uint64_t pair_base = 0;
                for (const PathBatch& b : P->batches) {
                    const unsigned grid = grid_256(b.n + 1, cus);      // (+ 1: as egrid)
                    if (whole) {                                            // every entry of every read: its place follows from the elements' offsets
                        hipLaunchKernelGGL(k_pidx_range_pairs, dim3(grid), dim3(256), 0, c->stream, (const uint32_t*)b.var.p, (const uint32_t*)b.elem_off.p, b.n, b.r0, b.var_bytes, 0u, (uint32_t)n_he,
                                           (const uint64_t*)nullptr, pair_base, (uint32_t*)k[0].p, (uint32_t*)v[0].p);
                        pair_base += b.var_bytes / 4 - 2 * b.n;
                    } else {
                        DevBuf n_in, at_of;
                        if ((rc = c->alloc(n_in, (b.n + 1) * 8, "entries in the range", Place::Low)) || (rc = c->alloc(at_of, (b.n + 1) * 8, "their places", Place::Low))) return rc;
                        hipLaunchKernelGGL(k_pidx_range_count, dim3(grid), dim3(256), 0, c->stream, (const uint32_t*)b.var.p, (const uint32_t*)b.elem_off.p, b.n, b.var_bytes, (uint32_t)e0, (uint32_t)e1, (uint64_t*)n_in.p);
                        HIP_TRY(hipGetLastError());
                        rc = device_scan(c, (const uint64_t*)n_in.p, (uint64_t*)at_of.p, b.n + 1); if (rc) return rc;
                        uint64_t got = 0;
                        HIP_TRY(hipMemcpyAsync(&got, (const uint64_t*)at_of.p + b.n, 8, hipMemcpyDeviceToHost, c->stream));
                        hipLaunchKernelGGL(k_pidx_range_pairs, dim3(grid), dim3(256), 0, c->stream, (const uint32_t*)b.var.p, (const uint32_t*)b.elem_off.p, b.n, b.r0, b.var_bytes, (uint32_t)e0, (uint32_t)e1,
                                           (const uint64_t*)at_of.p, pair_base, (uint32_t*)k[0].p, (uint32_t*)v[0].p);
                        HIP_TRY(hipGetLastError());
                        HIP_TRY(hipStreamSynchronize(c->stream));
                        c->release(n_in); c->release(at_of);
                        pair_base += got;
                    }
                }
                HIP_TRY(hipGetLastError());
                if (pair_base != n_r) return fail(DFK_E_HIP, "paths index: %llu entries listed for edges [%llu, %llu), the counts say %llu", (unsigned long long)pair_base, (unsigned long long)e0, (unsigned long long)e1, (unsigned long long)n_r);
                // stable sort by edge: read ids stay ascending inside an edge (ParallelSort of (edge, read) pairs, :87)
                int cur = 0;
                if ((rc = radix_sort_pairs(c, k, v, n_r, pidx_key_bits(e1 - e0), &cur))) return rc;
                c->release(k[0]); c->release(k[1]); c->release(v[cur ^ 1]);
                hipLaunchKernelGGL(HIP_KERNEL_NAME(k_digest_seq<uint32_t>), dim3(grid_256(n_r, cus)), dim3(256), 0, c->stream,
                                   (const uint32_t*)v[cur].p, n_r, 0x1111ull + h_first[e0], d);
                HIP_TRY(hipGetLastError());
                if (!dir.empty()) {
                    if (!tail && (rc = c->alloc(var, n_r * 8, "a.paths.inv data", Place::Low))) return rc;
                    uint64_t* wide = (uint64_t*)(tail ? tail->var.p : var.p);
                    hipLaunchKernelGGL(k_widen_u32, dim3(grid_256(n_r, cus)), dim3(256), 0, c->stream, (const uint32_t*)v[cur].p, n_r, wide);
                    HIP_TRY(hipGetLastError());
                    HIP_TRY(hipStreamSynchronize(c->stream));
                    const PidxMap pm = pidx_map(had, lay.var_tab, h_first[e0], n_r);
                    const bool mapped = pm.mapped;          // the lists' pages exist: through a mapping
                    const uint64_t m_lo = pm.lo, m_hi = pm.hi;
                    std::vector<FilePiece> pieces;
                    append_pieces(pieces, (const char*)wide, 8 * n_r, m_lo, XFER_CHUNK);
                    if (tail) {
                        tail->fd = fd; fd = -1;
                        const int dev = c->device;
                        tail->th = std::thread([c, tail, dev, pieces, mapped, m_lo, m_hi] {
                            FileMap fm;
                            const double tw = wall_now();
                            if (mapped) (void)fm.map(tail->fd, m_lo, m_hi);
                            if (hipSetDevice(dev) != hipSuccess || write_pieces(c, tail->fd, pieces, fm.p ? &fm : nullptr)) { tail->rc = DFK_E_ARG; tail->err = "short write to a.paths.inv: " + g_err; }
                            const double tu = wall_now();
                            fm.drop();
                            TRACE("paths index: %.2f GB of lists written in %.3f s%s, %.3f s unmapping", 1e-9 * (double)(m_hi - m_lo), tu - tw, mapped ? " through a mapping" : "", wall_now() - tu);
                        });
                    } else {
                        const double tw = wall_now();
                        FileMap fm;
                        if (mapped) (void)fm.map(fd, m_lo, m_hi);
                        if (write_pieces(c, fd, pieces, fm.p ? &fm : nullptr)) return fail(DFK_E_ARG, "short write to %s", path.c_str());
                        fm.drop();
                        TRACE("paths index: %.2f GB of lists written in %.3f s%s", 8e-9 * (double)n_r, wall_now() - tw, mapped ? " through a mapping" : "");
                        c->release(var);
                    }
                }
                HIP_TRY(hipStreamSynchronize(c->stream));
                c->release(v[cur]);
            }
            e0 = e1;
        }
        TRACE("paths index: %llu entries over %llu edges in %u range(s)", (unsigned long long)n_pairs, (unsigned long long)n_he, n_ranges);
        uint64_t h[16] = {};
        HIP_TRY(hipMemcpyAsync(h, dg.p, 128, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
        P->ck[DFK_CK_INV_SUM] = h[0]; P->ck[DFK_CK_INV_XOR] = h[1]; P->ck[DFK_CK_INV_STARTS] = h[4];
        P->ck[DFK_CK_INV_ENTRIES] = n_pairs;
        P->ck[DFK_CK_COUNTSB_DIGEST] = h[8]; P->ck[DFK_CK_COUNTSB_SUM] = h[10]; P->ck[DFK_CK_SELF_INVERSE] = h[12];
        P->ck[DFK_CK_VALID] |= DFK_CK_HAS_INDEX;
        return 0;
    };
    int rc = body();
    if (fd >= 0 && close(fd) != 0 && !rc) rc = fail(DFK_E_ARG, "short write to %s/a.paths.inv", dir.c_str());
    (void)hipStreamSynchronize(c->stream);
    c->release_since(mark);                                              // everything here is scratch
    return rc;
}

// MarkDups (10X/SecretOps.cc:410-566): a.dup
int dups_write(dfk_ctx* c, PathState* P, const std::string& path, uint64_t* n_marked)
{
    const uint64_t n = P->n_reads, n_pairs = n / 2;
    const unsigned cus = (unsigned)c->prop.multiProcessorCount;
    const uint64_t mark = c->alloc_seq;
    uint64_t marked = 0;
    const double t_in = wall_now();
    auto body = [&]() -> int {
        DevBuf dup, tk, tb, d_bad;
        int rc;
        if ((rc = c->alloc(dup, std::max<uint64_t>(1, n_pairs), "duplicate marks", Place::Low)) || (rc = c->alloc(d_bad, 16, "dup check", Place::Low))) return rc;
        HIP_TRY(hipMemsetAsync(dup.p, 0, std::max<uint64_t>(1, n_pairs), c->stream));
        HIP_TRY(hipMemsetAsync(d_bad.p, 0, 16, c->stream));
        // as many passes as the free HBM asks for: a pass's table holds the keys dealt to it at load <= 0.5
        const DupPlan plan = plan_dups(P->n_placed, c->largest_allocatable(), path_switches().dup_passes);
        const uint32_t n_pass = plan.n_pass;
        const uint64_t slots = plan.slots;
        if ((rc = c->alloc(tk, slots * 8, "duplicate keys", Place::Low)) || (rc = c->alloc(tb, slots * 8, "duplicate winners", Place::Low))) return rc;
        for (uint32_t pass = 0; pass < n_pass; ++pass) {
            hipLaunchKernelGGL(k_fill_u64, dim3(4096), dim3(256), 0, c->stream, (uint64_t*)tk.p, slots, ~0ull);
            HIP_TRY(hipMemsetAsync(tb.p, 0, slots * 8, c->stream));
            for (int markp = 0; markp < 2; ++markp)
                for (const PathBatch& b : P->batches) {
                    const unsigned grid = grid_256(b.n, cus);
                    if (!markp) hipLaunchKernelGGL(HIP_KERNEL_NAME(k_dup_pass<false>), dim3(grid), dim3(256), 0, c->stream, (const uint32_t*)b.var.p, (const uint32_t*)b.elem_off.p, b.n, b.r0,
                                                   b.var_bytes, (const uint32_t*)P->digest.p, (unsigned long long*)tk.p, (unsigned long long*)tb.p, slots - 1, n_pass, pass,
                                                   (uint8_t*)dup.p, (unsigned int*)d_bad.p);
                    else hipLaunchKernelGGL(HIP_KERNEL_NAME(k_dup_pass<true>), dim3(grid), dim3(256), 0, c->stream, (const uint32_t*)b.var.p, (const uint32_t*)b.elem_off.p, b.n, b.r0,
                                            b.var_bytes, (const uint32_t*)P->digest.p, (unsigned long long*)tk.p, (unsigned long long*)tb.p, slots - 1, n_pass, pass,
                                            (uint8_t*)dup.p, (unsigned int*)d_bad.p);
                }
            HIP_TRY(hipGetLastError());
        }
        unsigned bad = 0;
        HIP_TRY(hipMemcpy(&bad, d_bad.p, 4, hipMemcpyDeviceToHost));
        TRACE("duplicates: %u pass(es) over a table of %.1f GB, %.3f s on the device", n_pass, 16e-9 * (double)slots, wall_now() - t_in);
        if (bad & 1u) return fail(DFK_E_ARG, "duplicate marking packs a read's first edge in 29 bits and its offset in 25: this graph does not fit");
        if (bad & 2u) return fail(DFK_E_HIP, "duplicate marking: a key vanished between its two passes");
        {   // dfk_paths_digest: which pairs are marked, and how many
            DevBuf dg; if ((rc = c->alloc(dg, 32, "dup digest", Place::Low))) return rc;
            HIP_TRY(hipMemsetAsync(dg.p, 0, 32, c->stream));
            if (n_pairs) hipLaunchKernelGGL(HIP_KERNEL_NAME(k_digest_seq<uint8_t>), dim3(grid_256(n_pairs, cus)), dim3(256), 0, c->stream,
                                            (const uint8_t*)dup.p, n_pairs, 0x4444ull, (unsigned long long*)dg.p);
            HIP_TRY(hipGetLastError());
            uint64_t h[4] = {};
            HIP_TRY(hipMemcpyAsync(h, dg.p, 32, hipMemcpyDeviceToHost, c->stream));
            HIP_TRY(hipStreamSynchronize(c->stream));
            P->ck[DFK_CK_DUP_DIGEST] = h[0]; P->ck[DFK_CK_DUP_MARKED] = h[2];
            P->ck[DFK_CK_VALID] |= DFK_CK_HAS_DUPS;
            marked = h[2];                                                     // (the marks are 0 or 1: their sum)
        }
        if (!path.empty()) {
            // BinaryWriter::writeFile of vec<Bool> (DF.cc:561): "BINWRITE", the count, a byte a pair -- from the device through the lanes
            const int fd = open(path.c_str(), O_WRONLY | O_CREAT | O_TRUNC, 0666);
            if (fd < 0) return fail(DFK_E_ARG, "cannot open %s", path.c_str());
            struct { char magic[8]; uint64_t n; } hd{{'B', 'I', 'N', 'W', 'R', 'I', 'T', 'E'}, n_pairs};
            rc = pwrite(fd, &hd, 16, 0) == 16 ? 0 : fail(DFK_E_ARG, "short write to %s", path.c_str());
            std::vector<FilePiece> pieces;
            append_pieces(pieces, (const char*)dup.p, n_pairs, 16, XFER_CHUNK);
            if (!rc && write_pieces(c, fd, pieces)) rc = fail(DFK_E_ARG, "short write to %s", path.c_str());
            if (close(fd) != 0 && !rc) rc = fail(DFK_E_ARG, "short write to %s", path.c_str());
            if (rc) return rc;
        }
        return 0;
    };
    int rc = body();
    (void)hipStreamSynchronize(c->stream);
    c->release_since(mark);
    if (rc) return rc;
    if (n_marked) *n_marked = marked;
    TRACE("duplicates: %.3f s in all", wall_now() - t_in);
    return 0;
}

// The steps after pathing work from the paths alone: the k-mer index (4 bytes per slot at load <= 0.5: 34 GB for a human
// dictionary) goes back to the arena before they start.  Pathing again needs dfk_graph_build again.
void release_path_lookup(dfk_ctx* c, HostGraph* G) { c->release(G->d_index); c->release(G->d_filter); G->d_index = G->d_filter = DevBuf{}; G->filter_words = 0; }

// dfk_paths_verify: k_path_verify over every batch of the paths the context holds, against the reads given
// (dfk_paths_verify_arrays: over the batches it laid out, and their digest as paths_build_typed takes the context's own)
template <int K>
int paths_verify_typed(dfk_ctx* c, HostGraph* G, PathState* P, const Inputs& in, const std::vector<PathBatch>& batches, uint64_t* out, uint64_t* digest)
{
    DevBuf ctr; int rc = c->alloc(ctr, 8 * PV_N + 8, "verify counters", Place::Low); if (rc) return rc;
    HIP_TRY(hipMemsetAsync(ctr.p, 0, 8 * PV_N + 8, c->stream));
    const unsigned cus = (unsigned)c->prop.multiProcessorCount;
    const unsigned g = grid_256(in.n_reads, cus);
    hipLaunchKernelGGL(k_check_tables, dim3(std::max(1u, g)), dim3(256), 0, c->stream, in.base_off, in.packed_bytes, in.read_len, (const uint64_t*)nullptr, 0ull, in.n_reads,
                       (unsigned int*)((char*)ctr.p + 8 * PV_N));
    const PartTable pt = part_table_of(c);
    const PathGraph pg = path_graph_of(G, P);
    unsigned bad = 0;
    HIP_TRY(hipMemcpyAsync(&bad, (char*)ctr.p + 8 * PV_N, 4, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    if (bad) { c->release(ctr); return fail(DFK_E_INPUT, "verify: the reads' offset table is not monotone, runs past its array, or leaves a read fewer bytes than its bases need"); }
    for (const PathBatch& b : batches)
        hipLaunchKernelGGL(HIP_KERNEL_NAME(k_path_verify<K>), dim3(grid_256(b.n, cus, 64)), dim3(256), 0, c->stream, pt,
                           (const uint32_t*)G->d_index.p, G->index_slots, pg, in.packed, in.base_off, in.read_len,
                           (const uint32_t*)b.var.p, (const uint32_t*)b.elem_off.p, b.n, b.r0, b.var_bytes, (unsigned long long*)ctr.p);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(out, ctr.p, 8 * PV_N, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    c->release(ctr);
    if (!digest) return 0;
    const unsigned dgrid = 32u * cus;                                           // (a slot pair per block, then the fold: see k_paths_digest)
    DevBuf dg; rc = c->alloc(dg, 32 + 16ull * dgrid, "paths digest", Place::Low); if (rc) return rc;
    HIP_TRY(hipMemsetAsync(dg.p, 0, 32 + 16ull * dgrid, c->stream));
    unsigned long long* slots = (unsigned long long*)dg.p + 4;
    for (const PathBatch& b : batches)
        hipLaunchKernelGGL(k_paths_digest, dim3(grid_256(b.n, cus)), dim3(256), 0, c->stream, (const uint32_t*)b.var.p,
                           (const uint32_t*)b.elem_off.p, b.n, b.r0, b.var_bytes, slots);
    hipLaunchKernelGGL(k_paths_digest_fold, dim3(1), dim3(256), 0, c->stream, (const unsigned long long*)slots, dgrid, (unsigned long long*)dg.p);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(digest, dg.p, 16, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    c->release(dg);
    return 0;
}

PathState* built_paths(dfk_ctx* c);
// what a verify needs of the context: paths built (for the graph's tables) and the k-mer index still held
int verify_state(dfk_ctx* c)
{
    if (!built_paths(c)) return fail(DFK_E_STATE, "no paths: call dfk_paths_build");
    if (!graph_of(c)->d_index.p) return fail(DFK_E_STATE, "the graph's k-mer index was given back by dfk_paths_index_write / dfk_dups_write: verify before them");
    return 0;
}
// given: the batches of dfk_paths_verify_arrays, of any number of reads (null: the context's own paths, of the reads pathed)
int paths_verify_any(dfk_ctx* c, const Inputs& in, uint64_t* out, const std::vector<PathBatch>* given = nullptr, uint64_t* digest = nullptr)
{
    if (int rc = verify_state(c)) return rc;
    PathState* P = built_paths(c);
    HostGraph* G = graph_of(c);
    if (!given && in.n_reads != P->n_reads) return fail(DFK_E_ARG, "verify: %llu reads given, %llu pathed", (unsigned long long)in.n_reads, (unsigned long long)P->n_reads);
    const std::vector<PathBatch>& batches = given ? *given : P->batches;
    try {
        switch (c->cfg.K) {
        case 40: return paths_verify_typed<40>(c, G, P, in, batches, out, digest);
        case 48: return paths_verify_typed<48>(c, G, P, in, batches, out, digest);
        default: return paths_verify_typed<60>(c, G, P, in, batches, out, digest);
        }
    } catch (const std::runtime_error& e) { return fail(DFK_E_HIP, "%s", e.what()); }
}

// a host caller's reads on the device (outside the arena, as dfk_paths_verify always took them) for one paths_verify_any
int verify_host_reads(dfk_ctx* c, const uint8_t* packed, const uint64_t* base_off, const uint32_t* read_len, uint64_t n_reads, uint64_t* out,
                      const std::vector<PathBatch>* given, uint64_t* digest)
{
    uint64_t pb = 0;
    if (n_reads) { const int r1 = host_read(c, &pb, (const char*)base_off + 8 * n_reads, 8); if (r1) return r1; }
    void* d[3] = {};
    int rc = 0;
    auto up = [&](void** dp, const void* h, size_t bytes) {
        if (rc) return;
        if (hipMalloc(dp, bytes + 64) != hipSuccess) { (void)hipGetLastError(); rc = fail(DFK_E_NOMEM, "no room on the device for %zu bytes of input", bytes); return; }
        rc = upload(c, *dp, h, bytes);
    };
    up(&d[0], packed, pb); up(&d[1], base_off, n_reads ? (n_reads + 1) * 8 : 0); up(&d[2], read_len, n_reads * 4);   // (no reads: the tables may be null)
    if (!rc) {
        Inputs in{(const uint8_t*)d[0], pb, (const uint64_t*)d[1], (const uint32_t*)d[2], nullptr, 0, nullptr, nullptr, n_reads};
        rc = paths_verify_any(c, in, out, given, digest);
    }
    for (void* p : d) (void)hipFree(p);
    return rc;
}

PathState* built_paths(dfk_ctx* c)
{
    if (!c || !c->graph_state) return nullptr;
    HostGraph* G = graph_of(c);
    return (G->paths && G->paths->built) ? G->paths : nullptr;
}

// MarkBads (10X/SecretOps.cc:71-109): the paths that carry the per-read sums k_bad_sums gathered during the build, or
// an error
int bads_of(dfk_ctx* c, PathState** out)
{
    if (!c) return fail(DFK_E_ARG, "null context");
    if (!(c->cfg.flags & DFK_F_MARK_BADS)) return fail(DFK_E_STATE, "no bad-base sums: the context was created without DFK_F_MARK_BADS");
    PathState* P = built_paths(c);
    if (!P || !P->bad_sums.p) return fail(DFK_E_STATE, "no bad-base sums: call dfk_paths_build (on a context created with DFK_F_MARK_BADS)");
    *out = P;
    return 0;
}

// a.bad (10X/DF.cc:604): the sums folded to a byte per pair, counted, digested and -- with a path -- written: whole
// (part = false: "BINWRITE", the count, the bytes) or as this rank's bytes at pair first_pair of a file of total_pairs
int bads_write(dfk_ctx* c, PathState* P, const char* path, bool part, uint64_t first_pair, uint64_t total_pairs, uint64_t first_read, uint64_t* n_marked, uint64_t* digest)
{
    const uint64_t n = P->n_reads, n_pairs = n / 2;
    if (n % 2) return fail(DFK_E_ARG, "%llu reads: MarkBads works on pairs", (unsigned long long)n);
    if (part && first_pair + n_pairs > total_pairs) return fail(DFK_E_ARG, "this rank's pairs do not fit the file described");
    const unsigned cus = (unsigned)c->prop.multiProcessorCount;
    const uint64_t mark = c->alloc_seq;
    uint64_t hd[8] = {};
    auto body = [&]() -> int {
        DevBuf marks, dg;
        int rc;
        if ((rc = c->alloc(marks, std::max<uint64_t>(1, n_pairs), "bad-pair marks", Place::Low)) || (rc = c->alloc(dg, 64, "bad digest", Place::Low))) return rc;
        HIP_TRY(hipMemsetAsync(dg.p, 0, 64, c->stream));
        if (n_pairs) {
            const unsigned grid = grid_256(n_pairs, cus);
            hipLaunchKernelGGL(k_bad_marks, dim3(grid), dim3(256), 0, c->stream, (const uint16_t*)P->bad_sums.p, n_pairs, (uint8_t*)marks.p);
            // over reads of h(whole-set read id, sum); the marks' plain sum is their number
            hipLaunchKernelGGL(HIP_KERNEL_NAME(k_digest_seq<uint16_t>), dim3(grid_256(n, cus)), dim3(256), 0, c->stream,
                               (const uint16_t*)P->bad_sums.p, n, 0x5555ull + first_read, (unsigned long long*)dg.p);
            hipLaunchKernelGGL(HIP_KERNEL_NAME(k_digest_seq<uint8_t>), dim3(grid), dim3(256), 0, c->stream, (const uint8_t*)marks.p, n_pairs, 0x6666ull + first_pair, (unsigned long long*)dg.p + 4);
            HIP_TRY(hipGetLastError());
        }
        HIP_TRY(hipMemcpyAsync(hd, dg.p, 64, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
        if (!path) return 0;
        const int fd = open(path, part ? O_WRONLY | O_CREAT : O_WRONLY | O_CREAT | O_TRUNC, 0666);
        if (fd < 0) return fail(DFK_E_ARG, "cannot open %s", path);
        const uint64_t in_file = part ? total_pairs : n_pairs;
        if (!part || first_pair == 0) {                                   // BinaryWriter::writeFile of vec<Bool>, as for a.dup
            struct { char magic[8]; uint64_t n; } h{{'B', 'I', 'N', 'W', 'R', 'I', 'T', 'E'}, in_file};
            if (pwrite(fd, &h, 16, 0) != 16) rc = fail(DFK_E_ARG, "short write to %s", path);
        }
        if (!rc && part && ftruncate(fd, (off_t)(16 + in_file)) != 0) rc = fail(DFK_E_ARG, "cannot size %s", path);      // every rank: the same size
        if (!rc) {
            std::vector<FilePiece> pieces;
            append_pieces(pieces, (const char*)marks.p, n_pairs, 16 + first_pair, XFER_CHUNK);
            if (write_pieces(c, fd, pieces)) rc = fail(DFK_E_ARG, "short write to %s", path);
        }
        if (close(fd) != 0 && !rc) rc = fail(DFK_E_ARG, "short write to %s", path);
        return rc;
    };
    int rc;
    try { rc = body(); } catch (const std::runtime_error& e) { rc = fail(DFK_E_HIP, "%s", e.what()); }
    (void)hipStreamSynchronize(c->stream);
    c->release_since(mark);
    if (rc) return rc;
    if (n_marked) *n_marked = hd[6];
    if (digest) { digest[0] = hd[0]; digest[1] = hd[1]; }
    return 0;
}

} // namespace

extern "C" {

int dfk_paths_build_device(dfk_ctx* c, const void* d_packed, uint64_t packed_bytes, const void* d_base_off, const void* d_read_len,
                           const void* d_pq, uint64_t pq_nbytes, const void* d_pq_off, uint64_t n_reads)
{
    return guarded([&]() -> int {
    if (!c) return fail(DFK_E_ARG, "null context");
    if (n_reads && (!d_packed || !d_base_off || !d_read_len || !d_pq || !d_pq_off)) return fail(DFK_E_ARG, "null input array");
    HIP_TRY(hipSetDevice(c->device));
    Inputs in{(const uint8_t*)d_packed, packed_bytes, (const uint64_t*)d_base_off, (const uint32_t*)d_read_len,
              (const uint8_t*)d_pq, pq_nbytes, (const uint64_t*)d_pq_off, nullptr, n_reads};
    return paths_build_any(c, in);
    });
}

int dfk_paths_build(dfk_ctx* c, const uint8_t* packed, const uint64_t* base_off, const uint32_t* read_len,
                    const uint8_t* pq, const uint64_t* pq_off, uint64_t n_reads)
{
    return guarded([&]() -> int {
    if (!c) return fail(DFK_E_ARG, "null context");
    HIP_TRY(hipSetDevice(c->device));
    if (!packed && !base_off && !read_len && !pq && !pq_off) {
        // the reads dfk_count uploaded and kept (DFK_F_KEEP_INPUTS) -- or, on a rank of a sharded run, the pair range
        // dfk_shard_begin_host staged (kept through dfk_shard_dict_adopt under the same flag): the rank paths ITS reads
        if (!c->kept[0] && c->sh_staged[0] && c->sh_staged_reads) {
            if (!c->graph_state || !graph_of(c)->built) return fail(DFK_E_STATE, "no graph: call dfk_graph_build first");
            path_state_of(c, graph_of(c))->read_id0 = c->sh_read_id0;
            Inputs in{(const uint8_t*)c->sh_staged[0] - c->sh_b0, c->sh_b1, (const uint64_t*)c->sh_staged[1], (const uint32_t*)c->sh_staged[2],
                      (const uint8_t*)c->sh_staged[3] - c->sh_q0, c->sh_q1, (const uint64_t*)c->sh_staged[4], nullptr, c->sh_staged_reads};
            const int rc = paths_build_any(c, in);
            if (!rc) { for (void*& p : c->sh_staged) if (p) { (void)hipFree(p); p = nullptr; } c->budget += c->budget_taken; c->budget_taken = 0; c->sh_staged_reads = 0; }
            return rc;
        }
        if (!c->kept[0]) return fail(DFK_E_STATE, "no kept inputs: count with DFK_F_KEEP_INPUTS, or pass the reads");
        if (c->graph_state) path_state_of(c, graph_of(c))->read_id0 = 0;
        Inputs in{(const uint8_t*)c->kept[0], c->kept_packed_bytes, (const uint64_t*)c->kept[1], (const uint32_t*)c->kept[2],
                  (const uint8_t*)c->kept[3], c->kept_pq_bytes, (const uint64_t*)c->kept[4], nullptr, c->kept_n_reads};
        const int rc = paths_build_any(c, in);
        if (!rc) c->adopt_kept();                                         // they were kept for this; their room goes to the arena
        return rc;
    }
    if (n_reads && (!packed || !base_off || !read_len || !pq || !pq_off)) return fail(DFK_E_ARG, "null input array");
    uint64_t pb = 0, qb = 0;
    if (n_reads) { int r1 = host_read(c, &pb, (const char*)base_off + 8 * n_reads, 8); if (!r1) r1 = host_read(c, &qb, (const char*)pq_off + 8 * n_reads, 8); if (r1) return r1; }
    void *d[5] = {};
    int rc = 0;
    auto up = [&](void** dp, const void* h, size_t bytes) {
        if (rc) return;
        if (hipMalloc(dp, bytes + 64) != hipSuccess) { (void)hipGetLastError(); rc = fail(DFK_E_NOMEM, "no room on the device for %zu bytes of input", bytes); return; }
        rc = upload(c, *dp, h, bytes);
    };
    up(&d[0], packed, pb); up(&d[1], base_off, (n_reads + 1) * 8); up(&d[2], read_len, n_reads * 4); up(&d[3], pq, qb); up(&d[4], pq_off, (n_reads + 1) * 8);
    if (!rc) {
        const uint64_t staged = pb + qb + (n_reads + 1) * 16 + n_reads * 4 + 5 * 64;
        const uint64_t saved = c->budget;
        c->budget = c->budget > staged ? c->budget - staged : 0;
        Inputs in{(const uint8_t*)d[0], pb, (const uint64_t*)d[1], (const uint32_t*)d[2], (const uint8_t*)d[3], qb, (const uint64_t*)d[4], nullptr, n_reads};
        rc = paths_build_any(c, in);
        c->budget = saved;
    }
    for (void* p : d) (void)hipFree(p);
    return rc;
    });
}

int dfk_paths_stats(dfk_ctx* c, uint64_t* n_reads, uint64_t* n_placed, uint64_t* n_path_edges)
{
    PathState* P = built_paths(c);
    if (!P) return fail(DFK_E_STATE, "no paths: call dfk_paths_build");
    if (n_reads) *n_reads = P->n_reads;
    if (n_placed) *n_placed = P->n_placed;
    if (n_path_edges) *n_path_edges = P->n_edges;
    return 0;
}

int dfk_paths_sink(dfk_ctx* c, const char* path)
{
    return guarded([&]() -> int {
    if (!c) return fail(DFK_E_ARG, "null context");
    if (!c->graph_state || !graph_of(c)->built) return fail(DFK_E_STATE, "no graph: call dfk_graph_build first");
    PathState* P = path_state_of(c, graph_of(c));
    P->sink_path = path ? path : "";
    return 0;
    });
}

int dfk_paths_write(dfk_ctx* c, const char* path)
{
    return guarded([&]() -> int {
    PathState* P = built_paths(c);
    if (!P) return fail(DFK_E_STATE, "no paths: call dfk_paths_build");
    if (!path) return fail(DFK_E_ARG, "null path");
    HIP_TRY(hipSetDevice(c->device));
    // feudal file (feudal/FeudalControlBlock.h:159-165, FeudalFileWriter.cc:26-121): control block | variable data |
    // n+1 absolute offsets | no fixed data (ReadPath keeps none outside the variable part)
    const uint64_t n = P->n_reads;
    const FeudalLayout lay = feudal_layout(n, 24, 4, P->var_total);
    // This call only reads the context (see dfk.h) and may run on a thread of its own beside the calls that follow it.
    // (with dfk_paths_sink on this path the variable data is in the file already, or on its way: wait for it, add the rest)
    const bool streamed = P->sink && P->sink->path == path;
    if (P->sink && !streamed) return fail(DFK_E_STATE, "the paths are being written to %s (dfk_paths_sink): write that file first", P->sink->path.c_str());
    int fd = -1, rc = 0;
    if (streamed) { rc = sink_finish(P, &fd); if (rc) return rc; }
    else fd = open(path, O_WRONLY | O_CREAT | O_TRUNC, 0666);
    if (fd < 0) return fail(DFK_E_ARG, "cannot open %s", path);
    return path_batches_to_file(c, fd, path, lay, n, P->batches, streamed);
    });
}

int dfk_qual_hist(dfk_ctx* c, uint32_t max_len, int64_t* hist)
{
    return guarded([&]() -> int {
    if (!c || !hist) return fail(DFK_E_ARG, "null argument");
    if (!c->kept[0]) return fail(DFK_E_STATE, "no reads on the device: dfk_count with DFK_F_KEEP_INPUTS keeps them");
    if (!max_len || max_len > 4095) return fail(DFK_E_ARG, "max_len %u: 1 .. 4095", max_len);
    HIP_TRY(hipSetDevice(c->device));
    const uint64_t n = c->kept_n_reads, nd = (uint64_t)2 * max_len * 256, nf = (uint64_t)2 * 256 * (max_len + 1);
    std::fill(hist, hist + nd, 0);
    if (!n) return 0;
    DevBuf tab;
    int rc = c->alloc(tab, nf * 8, "quality histogram", Place::Low); if (rc) return rc;
    HIP_TRY(hipMemsetAsync(tab.p, 0, nf * 8, c->stream));
    const unsigned cus = (unsigned)c->prop.multiProcessorCount;
    const size_t lds = (size_t)2 * QH_Q * (QH_POS + 1) * 4;
    HIP_TRY(hipFuncSetAttribute((const void*)k_qual_hist, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL(k_qual_hist, dim3((unsigned)std::min<uint64_t>((n + 1023) / 1024, cus)), dim3(1024), lds, c->stream,
                       (const uint8_t*)c->kept[3], (const uint64_t*)c->kept[4], n, max_len, (long long*)tab.p);
    HIP_TRY(hipGetLastError());
    std::vector<int64_t> diff(nf);
    HIP_TRY(hipMemcpyAsync(diff.data(), tab.p, nf * 8, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    c->release(tab);
    for (uint32_t par = 0; par < 2; ++par)
        for (uint32_t q = 0; q < 256; ++q) {
            const int64_t* row = &diff[((size_t)par * 256 + q) * (max_len + 1)];
            int64_t run = 0;
            for (uint32_t pos = 0; pos < max_len; ++pos) { run += row[pos]; hist[((size_t)par * max_len + pos) * 256 + q] += run; }
        }
    return 0;
    });
}

int dfk_paths_fetch(dfk_ctx* c, int32_t* offsets, uint64_t* first_edge, int32_t* edges, uint64_t edges_cap)
{
    return guarded([&]() -> int {
    PathState* P = built_paths(c);
    if (!P) return fail(DFK_E_STATE, "no paths: call dfk_paths_build");
    if (!offsets || !first_edge || (!edges && P->n_edges)) return fail(DFK_E_ARG, "null argument");
    if (edges_cap < P->n_edges) return fail(DFK_E_ARG, "buffer too small: %llu < %llu path edges", (unsigned long long)edges_cap, (unsigned long long)P->n_edges);
    HIP_TRY(hipSetDevice(c->device));
    uint64_t at = 0;
    std::vector<uint32_t> var, eo;
    for (const PathBatch& b : P->batches) {
        var.resize(b.var_bytes / 4); eo.resize(b.n);
        if (b.var_bytes) HIP_TRY(hipMemcpy(var.data(), b.var.p, b.var_bytes, hipMemcpyDeviceToHost));
        HIP_TRY(hipMemcpy(eo.data(), b.elem_off.p, b.n * 4, hipMemcpyDeviceToHost));
        for (uint64_t i = 0; i < b.n; ++i) {
            const uint64_t w0 = eo[i] / 4, w1 = i + 1 < b.n ? eo[i + 1] / 4 : b.var_bytes / 4;
            offsets[b.r0 + i] = (int32_t)var[w0];
            first_edge[b.r0 + i] = at;
            for (uint64_t w = w0 + 2; w < w1; ++w) edges[at++] = (int32_t)var[w];
        }
    }
    first_edge[P->n_reads] = at;
    return 0;
    });
}

int dfk_paths_digest(dfk_ctx* c, uint64_t* out)
{
    return guarded([&]() -> int {
    PathState* P = built_paths(c);
    if (!P) return fail(DFK_E_STATE, "no paths: call dfk_paths_build");
    if (!out) return fail(DFK_E_ARG, "null argument");
    const HostGraph* G = graph_of(c);
    // row f-1's identities, from the host half of the graph: every solid k-mer on exactly one canonical edge, the
    // involution its own inverse and in range
    uint64_t kmers = 0, viol = 0;
    for (const GraphEdge& e : G->ce) kmers += e.n;
    const size_t E = G->he.size();
    auto inv_of = [&](size_t e) -> int64_t { return G->he[e].rc ? G->fwd[G->he[e].ce] : G->rev[G->he[e].ce]; };
    for (size_t e = 0; e < E; ++e) { const int64_t o = inv_of(e); if (o < 0 || (size_t)o >= E || (size_t)inv_of((size_t)o) != e) ++viol; }
    for (int i = 0; i < DFK_CHECK_WORDS; ++i) out[i] = P->ck[i];
    out[DFK_CK_EDGE_KMERS] = kmers; out[DFK_CK_N_SOLID] = c->n_solid; out[DFK_CK_INV_VIOLATIONS] = viol; out[DFK_CK_N_EDGES] = E;
    return 0;
    });
}

int dfk_paths_verify_device(dfk_ctx* c, const void* d_packed, uint64_t packed_bytes, const void* d_base_off, const void* d_read_len,
                            uint64_t n_reads, uint64_t* out)
{
    return guarded([&]() -> int {
    if (!c || !out) return fail(DFK_E_ARG, "null argument");
    if (n_reads && (!d_packed || !d_base_off || !d_read_len)) return fail(DFK_E_ARG, "null input array");
    HIP_TRY(hipSetDevice(c->device));
    Inputs in{(const uint8_t*)d_packed, packed_bytes, (const uint64_t*)d_base_off, (const uint32_t*)d_read_len, nullptr, 0, nullptr, nullptr, n_reads};
    return paths_verify_any(c, in, out);
    });
}

int dfk_paths_verify(dfk_ctx* c, const uint8_t* packed, const uint64_t* base_off, const uint32_t* read_len, uint64_t n_reads, uint64_t* out)
{
    return guarded([&]() -> int {
    if (!c || !out) return fail(DFK_E_ARG, "null argument");
    if (n_reads && (!packed || !base_off || !read_len)) return fail(DFK_E_ARG, "null input array");
    HIP_TRY(hipSetDevice(c->device));
    return verify_host_reads(c, packed, base_off, read_len, n_reads, out, nullptr, nullptr);
    });
}

// The verifier on paths given as host arrays: the batches laid out as k_path_emit leaves them (layout_batch), each with its r0,
// then k_path_verify on the context's graph, k-mer index and tables as dfk_paths_verify launches it, and the paths digest over
// the same batches.  Edge ids and offsets go to the device as they are: counting them is the kernel's work, and no host array is
// indexed by either.
int dfk_paths_verify_arrays(dfk_ctx* c, const uint8_t* packed, const uint64_t* base_off, const uint32_t* read_len, uint64_t n_reads,
                            const int32_t* offsets, const uint64_t* first, const int32_t* edges, uint64_t reads_per_batch, uint64_t* out)
{
    return guarded([&]() -> int {
    const uint64_t N = n_reads;
    if (!c || !out || !first || (N && (!packed || !base_off || !read_len || !offsets))) return fail(DFK_E_ARG, "null argument");
    if (int rc = verify_state(c)) return rc;
    if (N >= (1ull << 31)) return fail(DFK_E_ARG, "%llu reads: 2^31 - 1 at most", (unsigned long long)N);
    if (first[0] != 0) return fail(DFK_E_ARG, "the paths do not start at 0");
    for (uint64_t i = 0; i < N; ++i) if (first[i + 1] < first[i]) return fail(DFK_E_ARG, "the paths' starts fall at read %llu", (unsigned long long)i);
    if (first[N] >= (1ull << 31)) return fail(DFK_E_ARG, "%llu path edges: 2^31 - 1 at most", (unsigned long long)first[N]);
    if (first[N] && !edges) return fail(DFK_E_ARG, "null argument");
    const uint64_t per = reads_per_batch ? reads_per_batch : std::max<uint64_t>(1, N);
    for (uint64_t r0 = 0; r0 < N; r0 += per) {
        const uint64_t n = std::min(per, N - r0), bytes = 8 * n + 4 * (first[r0 + n] - first[r0]);
        if (bytes >= (1ull << 32)) return fail(DFK_E_ARG, "a batch of %llu reads holds %llu bytes of paths: its offsets keep 32 bits", (unsigned long long)n, (unsigned long long)bytes);
    }
    HIP_TRY(hipSetDevice(c->device));
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
        uint64_t res[PV_N + 2] = {};
        if ((rc = verify_host_reads(c, packed, base_off, read_len, N, res, &batches, res + PV_N))) return rc;
        for (int i = 0; i < PV_N + 2; ++i) out[i] = res[i];
        return 0;
    };
    int rc;
    try { rc = body(); } catch (const std::runtime_error& e) { rc = fail(DFK_E_HIP, "%s", e.what()); }
    (void)hipStreamSynchronize(c->stream);
    c->release_since(mark);                                                  // the batches
    return rc;
    });
}

int dfk_paths_index_write(dfk_ctx* c, const char* dir)
{
    return guarded([&]() -> int {
    PathState* P = built_paths(c);
    if (!P) return fail(DFK_E_STATE, "no paths: call dfk_paths_build");
    HIP_TRY(hipSetDevice(c->device));
    release_path_lookup(c, graph_of(c));
    try { return paths_index_write(c, graph_of(c), P, dir ? dir : ""); }
    catch (const std::runtime_error& e) { return fail(DFK_E_HIP, "%s", e.what()); }
    });
}

int dfk_paths_index_dups_write(dfk_ctx* c, const char* dir, const char* dup_path, uint64_t* n_marked_pairs)
{
    return guarded([&]() -> int {
    PathState* P = built_paths(c);
    if (!P) return fail(DFK_E_STATE, "no paths: call dfk_paths_build");
    if (P->n_reads % 2) return fail(DFK_E_ARG, "%llu reads: MarkDups works on pairs", (unsigned long long)P->n_reads);
    HIP_TRY(hipSetDevice(c->device));
    release_path_lookup(c, graph_of(c));
    IndexTail tail;
    int rc = 0;
    try {
        rc = paths_index_write(c, graph_of(c), P, dir ? dir : "", &tail);
        if (!rc) rc = dups_write(c, P, dup_path ? dup_path : "", n_marked_pairs);
    } catch (const std::runtime_error& e) { rc = fail(DFK_E_HIP, "%s", e.what()); }
    const std::string first = rc ? g_err : std::string();
    const int rc_tail = tail.finish(c);
    return rc ? fail(rc, "%s", first.c_str()) : rc_tail;
    });
}

int dfk_dups_write(dfk_ctx* c, const char* path, uint64_t* n_marked_pairs)
{
    return guarded([&]() -> int {
    PathState* P = built_paths(c);
    if (!P) return fail(DFK_E_STATE, "no paths: call dfk_paths_build");
    if (P->n_reads % 2) return fail(DFK_E_ARG, "%llu reads: MarkDups works on pairs", (unsigned long long)P->n_reads);
    HIP_TRY(hipSetDevice(c->device));
    release_path_lookup(c, graph_of(c));
    try { return dups_write(c, P, path ? path : "", n_marked_pairs); }
    catch (const std::runtime_error& e) { return fail(DFK_E_HIP, "%s", e.what()); }
    });
}

int dfk_bads_sums(dfk_ctx* c, uint16_t* out, uint64_t cap)
{
    return guarded([&]() -> int {
    PathState* P = nullptr;
    if (int rc = bads_of(c, &P)) return rc;
    if (!out && P->n_reads) return fail(DFK_E_ARG, "null argument");
    if (cap < P->n_reads) return fail(DFK_E_ARG, "buffer too small: %llu < %llu reads", (unsigned long long)cap, (unsigned long long)P->n_reads);
    HIP_TRY(hipSetDevice(c->device));
    if (P->n_reads) HIP_TRY(hipMemcpy(out, P->bad_sums.p, P->n_reads * 2, hipMemcpyDeviceToHost));
    return 0;
    });
}

int dfk_bads_write(dfk_ctx* c, const char* path, uint64_t* n_marked_pairs, uint64_t* digest)
{
    return guarded([&]() -> int {
    PathState* P = nullptr;
    if (int rc = bads_of(c, &P)) return rc;
    HIP_TRY(hipSetDevice(c->device));
    return bads_write(c, P, path, false, 0, P->n_reads / 2, (uint64_t)P->read_id0, n_marked_pairs, digest);
    });
}

} // extern "C"
