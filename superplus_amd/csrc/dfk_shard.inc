// superplus_amd/csrc/dfk_shard.inc -- multi-GPU entry points (included by dfk.hip).
// One process per GPU; the caller moves bytes between ranks (RCCL all-to-all over xGMI).
namespace {

// host wall time of one sharded entry point, booked on the context's statistics when it returns
struct CallClock {
    dfk_ctx* c; float* also; std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now();
    CallClock(dfk_ctx* ctx, float* stage) : c(ctx), also(stage) {}
    ~CallClock()
    {
        if (!c) return;
        (void)hipStreamSynchronize(c->stream);
        const float ms = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count();
        c->st.ms_total += ms;
        c->st.hbm_bytes_peak = c->peak;
        if (also) *also += ms;
    }
};

uint32_t log2_exact(uint32_t v) { uint32_t l = 0; while ((1u << l) < v) ++l; return l; }

// state kept between the passes of one sharded run
// a partition that has been prepared (buffers, expected fills) and is launched now or behind the next k_count
struct PendingPartition {
    bool active = false, launched = false, last = false;
    uint32_t pass = 0, world = 0;
    DevBuf d_slice, d_fill;
    std::vector<uint64_t> expect;
    std::function<int()> launch;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    ~PendingPartition() { if (e0) { (void)hipEventDestroy(e0); (void)hipEventDestroy(e1); } }
};
struct ShardState { BucketTable T; CountRun R; uint32_t log2_pass = 0; bool counted = false, run_open = false; PendingPartition pend; };
void shard_state_delete(void* p) { delete static_cast<ShardState*>(p); }
ShardState* shard_state(dfk_ctx* c)
{
    if (!c->shard_state) { c->shard_state = new ShardState; c->shard_state_free = shard_state_delete; }
    return static_cast<ShardState*>(c->shard_state);
}

Inputs shard_inputs(const dfk_ctx* c)
{
    return Inputs{(const uint8_t*)c->sh_in[0], c->sh_packed_bytes, (const uint64_t*)c->sh_in[1], (const uint32_t*)c->sh_in[2],
                  (const uint8_t*)c->sh_in[3], c->sh_pq_bytes, (const uint64_t*)c->sh_in[4], (const int32_t*)c->sh_in[5], c->sh_n_reads};
}

template <int K>
int shard_count_buckets(dfk_ctx* c, uint32_t world, uint64_t n_inst_global)
{
    ShardState* S = shard_state(c);
    if (S->counted) return 0;
    const uint32_t lw = log2_exact(world);
    S->T.log2_nb = pick_log2_nb(n_inst_global, lw);
    // the sending side keeps no per-bucket counters: the owner of a bucket regroups what it receives
    int rc = partition_count<K>(c, shard_inputs(c), c->sh_n_inst_local, lw, c->sh_read_id0, &S->T, true); if (rc) return rc;
    S->counted = true;
    c->shard_world = world; c->shard_log2_nb = S->T.log2_nb;
    return 0;
}

// passes this rank would like: a pass sends its records, receives about as many and regroups them
template <int K>
int shard_plan_typed(dfk_ctx* c, uint32_t world, uint64_t n_inst_global, uint32_t* log2_passes)
{
    int rc = shard_count_buckets<K>(c, world, n_inst_global); if (rc) return rc;
    const ShardState* S = shard_state(c);
    const uint64_t room = c->budget > c->held ? c->budget - c->held : 0;
    uint32_t l = 0;
    // around the regroup of pass p: received p, regrouped p, and -- the exchange of pass p+1 and the partition of pass
    // p+2 run under the count of p -- send p+1, received p+1 and send p+2
    // (with one or two passes there is no pass p+2: four buffers)
    while (l < 8 && (l < 2 ? 4.0 : 5.0) * (double)S->T.n_records * 32.0 / (double)(1u << l) > 0.45 * (double)room) ++l;
    // With peers, at least four passes even when one would fit: the all-to-all of a pass hides under the count of the
    // pass before, so one pass exposes all of it and four a quarter -- at eight ranks 28 GB in and out per rank, 60 ms at
    // the links' peak and nearer 100 in practice, against the 11 ms the three extra sweeps cost (rehearsal: 0.261 s
    // per rank with one pass, 0.272 s with four; the rehearsal moves no bytes).
    if (world > 1) l = std::max(l, 2u);
    if (c->cfg.reserved[0]) { l = 0; while ((1ull << l) < c->cfg.reserved[0]) ++l; }
    const uint32_t log2_sub = S->T.log2_nb - log2_exact(world);
    if (log2_sub > 24) l = std::max(l, log2_sub - 24);               // the record header carries 24 bits of the in-pass bucket id
    *log2_passes = std::min<uint32_t>(std::min<uint32_t>(l, 6), log2_sub > 4 ? log2_sub - 4 : 0);   // a pass is a whole number of the 64 classes
    return 0;
}

// Partition pass `pass`: room for its records, the fill each owner's slice must reach (known from the counting scan's
// class totals: the caller gets its send counts without waiting for a kernel), and the launch -- now, or (defer) behind
// the k_count of the dfk_shard_count call that follows, on the second stream: the sweep then runs beside that count
// as a single-GPU sweep does, and for the same reason not ahead of it (DESIGN.md section 9, the cliff).
template <int K>
int shard_partition_begin_typed(dfk_ctx* c, uint32_t world, uint64_t n_inst_global, uint32_t log2_passes, uint32_t pass, bool defer,
                                const void** d_records, uint64_t* send_counts)
{
    const uint32_t lw = log2_exact(world);
    int rc = shard_count_buckets<K>(c, world, n_inst_global); if (rc) return rc;
    ShardState* S = shard_state(c);
    if (S->pend.active) return fail(DFK_E_STATE, "dfk_shard_partition_begin: pass %u has not been ended", S->pend.pass);
    S->log2_pass = log2_passes;
    // every rank cuts its owners' bucket spaces into the same 2^log2_passes equal ranges (whole classes)
    const uint32_t log2_sub = S->T.log2_nb - lw;
    const uint32_t sub_n = (1u << log2_sub) >> log2_passes;
    const uint32_t n_cls = 1u << std::min<uint32_t>(6, log2_sub);
    if ((n_cls >> log2_passes) == 0) return fail(DFK_E_ARG, "2^%u passes over %u bucket classes", log2_passes, n_cls);
    const uint32_t cls_per_pass = n_cls >> log2_passes;
    std::vector<uint64_t> slice(world + 1, 0);
    for (uint32_t o = 0; o < world; ++o) {
        uint64_t n = 0;
        for (uint32_t k = 0; k < cls_per_pass; ++k) n += S->T.h_class[(uint64_t)o * PART_CLASSES + pass * cls_per_pass + k];
        send_counts[o] = n; slice[o + 1] = slice[o] + n;
    }
    const Inputs in = shard_inputs(c);
    const PartParams pp = part_params<K>(c, S->T.log2_nb, lw, c->sh_read_id0, pass * sub_n, sub_n);
    PendingPartition& Q = S->pend;
    DevBuf& rec = c->shard_send[pass & 1];                             // (its last occupant, pass - 2, has long arrived)
    c->release(rec); c->shard_send_pass[pass & 1] = ~0u;
    rc = c->alloc(rec, std::max<uint64_t>(1, slice[world]) * 32, "records to send"); if (rc) return rc;
    rc = c->alloc(Q.d_slice, (world + 1) * 8, "slice bases"); if (rc) { c->release(rec); return rc; }
    rc = c->alloc(Q.d_fill, world * 8, "slice fill"); if (rc) { c->release(rec); c->release(Q.d_slice); return rc; }
    c->shard_send_pass[pass & 1] = pass;
    Q.active = true; Q.launched = false; Q.pass = pass; Q.world = world; Q.last = pass + 1 == (1u << log2_passes);
    Q.expect.assign(send_counts, send_counts + world);
    if (!Q.e0) { HIP_TRY(hipEventCreate(&Q.e0)); HIP_TRY(hipEventCreate(&Q.e1)); }
    const uint64_t n_ovf = S->T.n_ovf, n_out = slice[world];
    const uint4* summ = (const uint4*)S->T.summ.p; const uint32_t* classes = (const uint32_t*)S->T.classes.p; const uint32_t* ovf = (const uint32_t*)S->T.ovf_list.p;
    uint4* out = (uint4*)rec.p; uint64_t* d_slice = (uint64_t*)Q.d_slice.p; unsigned long long* d_fill = (unsigned long long*)Q.d_fill.p;
    const uint32_t* good_len = (const uint32_t*)c->good_len.p; const int64_t ign = (int64_t)c->cfg.ign_bc_below;
    Q.launch = [=]() -> int {
        ShardState* S2 = shard_state(c);
        hipStream_t st = c->stream2;
        HIP_TRY(hipEventRecord(S2->pend.e0, st));
        HIP_TRY(hipMemcpyAsync(d_slice, slice.data(), (world + 1) * 8, hipMemcpyHostToDevice, st));   // (pageable: copied out before the call returns)
        HIP_TRY(hipMemsetAsync(d_fill, 0, world * 8, st));
        if (in.n_reads)
            hipLaunchKernelGGL(HIP_KERNEL_NAME(k_scatter_slices<K>), dim3((unsigned)((in.n_reads + 256ull * SLICE_READS - 1) / (256ull * SLICE_READS))),
                               dim3(256), 0, st, in.packed, in.packed_bytes, in.base_off, good_len, in.bc, ign, in.n_reads, pp, summ, classes,
                               (const uint64_t*)d_slice, d_fill, out);
        HIP_TRY(hipGetLastError());
        if (n_ovf) {                                                     // reads with more runs than a summary holds
            const size_t lds_b = sizeof(uint32_t) * pp.W * PART_THREADS + sizeof(uint32_t) * 2 * PART_QCAP * PART_THREADS;
            hipLaunchKernelGGL(HIP_KERNEL_NAME(k_partition<K, true>), dim3((unsigned)((n_ovf + PART_THREADS - 1) / PART_THREADS)),
                               dim3(PART_THREADS), lds_b, st, in.packed, in.packed_bytes, in.base_off, good_len, in.bc, ign, in.n_reads, pp,
                               (unsigned long long*)nullptr, (unsigned long long*)nullptr, d_fill, n_out, out, (uint4*)nullptr,
                               ovf, n_ovf, (const uint64_t*)d_slice, (uint32_t*)nullptr);
            HIP_TRY(hipGetLastError());
        }
        HIP_TRY(hipEventRecord(S2->pend.e1, st));
        S2->pend.launched = true;
        return 0;
    };
    if (defer) c->after_count_launch = [c]() -> int { ShardState* S2 = shard_state(c); return S2->pend.active && !S2->pend.launched ? S2->pend.launch() : 0; };
    else { rc = Q.launch(); if (rc) return rc; }
    *d_records = rec.p;
    return 0;
}

int shard_partition_end(dfk_ctx* c, uint32_t pass)
{
    ShardState* S = shard_state(c);
    PendingPartition& Q = S->pend;
    if (!Q.active || Q.pass != pass) return fail(DFK_E_STATE, "dfk_shard_partition_end: pass %u has not been begun", pass);
    c->after_count_launch = nullptr;
    int rc = 0;
    if (!Q.launched) rc = Q.launch();                                    // (the count in between launched nothing: no items)
    std::vector<uint64_t> fill(Q.world, 0);
    if (!rc && hipMemcpyAsync(fill.data(), Q.d_fill.p, Q.world * 8, hipMemcpyDeviceToHost, c->stream2) != hipSuccess) rc = fail(DFK_E_HIP, "reading the slice fills");
    if (!rc && hipStreamSynchronize(c->stream2) != hipSuccess) rc = fail(DFK_E_HIP, "the partition of pass %u failed: %s", pass, hipGetErrorString(hipGetLastError()));
    float ms = 0;
    if (!rc && hipEventElapsedTime(&ms, Q.e0, Q.e1) == hipSuccess) c->st.ms_part_scatter += ms;
    c->release(Q.d_slice); c->release(Q.d_fill);
    Q.active = false; Q.launch = nullptr;
    if (rc) return rc;
    for (uint32_t o = 0; o < Q.world; ++o)
        if (fill[o] != Q.expect[o])
            return fail(DFK_E_HIP, "pass %u: %llu records for rank %u, the counting scan saw %llu", pass, (unsigned long long)fill[o], o,
                        (unsigned long long)Q.expect[o]);
    if (Q.last) { c->release(S->T.summ); c->release(S->T.classes); c->release(S->T.ovf_list); c->release(S->T.class_hist); }   // last pass: no longer needed
    return 0;
}

template <int K>
int shard_count_typed(dfk_ctx* c, const void* d_records, uint64_t n_records, uint32_t pass)
{
    ShardState* S = shard_state(c);
    const uint32_t n_passes = 1u << S->log2_pass;
    c->want_blist = false;                                               // (the parts are merged; the neighbour queries have their own lists)
    // the send buffer is no longer needed once the caller has the received records
    // (unless the caller has already partitioned the next pass, whose exchange may be in flight under this count)
    if (c->shard_send_pass[pass & 1] == pass) { c->release(c->shard_send[pass & 1]); c->shard_send_pass[pass & 1] = ~0u; }
    const uint32_t lw = log2_exact(c->shard_world);
    const uint32_t l2_local = c->shard_log2_nb - lw - S->log2_pass;
    const uint64_t nb = 1ull << l2_local;
    // regroup by fine bucket -- two levels of counting sort with LDS counters (k_rg_*), no global atomics; booked
    // as partition time.
    Timer t_regroup(c->stream);
    t_regroup.start();
    if (l2_local > 24) return fail(DFK_E_ARG, "a pass of 2^%u buckets per rank: the record header keeps 24 bits", l2_local);
    DevBuf acc; int rc = c->alloc(acc, nb * 8, "regroup counters"); if (rc) return rc;
    Partition P;
    const uint64_t budget = item_budget<K>(c);
    DevBuf* mine = nullptr;                                              // the receive buffer, if it is the library's
    for (DevBuf& rb : c->shard_recv) if (rb.p && d_records == rb.p) mine = &rb;
    if (n_records == 0) {                                                // nothing received: empty tables, no kernel
        HIP_TRY(hipMemsetAsync(acc.p, 0, nb * 8, c->stream));
        rc = pass_tables(c, acc, l2_local, 1, 0, (uint32_t)nb, budget, &P); if (rc) return rc;
        c->release(acc);
        rc = c->alloc(P.records, 0, "regrouped records"); if (rc) return rc;
    } else {
        const uint32_t part_shift = l2_local > RG_LOG2_PARTS ? l2_local - RG_LOG2_PARTS : 0;
        const uint32_t n_parts = (uint32_t)(nb >> part_shift);
        const uint64_t chunk = std::max<uint64_t>(4096, (n_records + 2047) / 2048);
        const unsigned B = (unsigned)((n_records + chunk - 1) / chunk);
        const uint64_t n_h = (uint64_t)n_parts * B + 1;
        DevBuf h1, h1off, tmp;
        rc = c->alloc(h1, n_h * 8, "regroup block counts"); if (rc) return rc;
        rc = c->alloc(h1off, n_h * 8, "regroup block offsets"); if (rc) return rc;
        rc = c->alloc(tmp, n_records * 32, "records by partition"); if (rc) return rc;
        HIP_TRY(hipMemsetAsync((char*)h1.p + (n_h - 1) * 8, 0, 8, c->stream));
        hipLaunchKernelGGL(k_rg_hist, dim3(B), dim3(256), 0, c->stream, (const uint4*)d_records, n_records, chunk, (uint32_t)(nb - 1),
                           part_shift, n_parts, (uint64_t*)h1.p);
        HIP_TRY(hipGetLastError());
        rc = device_scan(c, (const uint64_t*)h1.p, (uint64_t*)h1off.p, n_h); if (rc) return rc;
        hipLaunchKernelGGL(k_rg_scatter, dim3(B), dim3(256), 0, c->stream, (const uint4*)d_records, n_records, chunk, (uint32_t)(nb - 1),
                           part_shift, n_parts, (const uint64_t*)h1off.p, (uint4*)tmp.p);
        HIP_TRY(hipGetLastError());
        // level 2 writes into the receive buffer when that is the library's own (it is no longer needed), else
        // into a third buffer
        if (mine) { P.records = *mine; *mine = DevBuf{}; }
        else { rc = c->alloc(P.records, n_records * 32, "regrouped records"); if (rc) return rc; }
        hipLaunchKernelGGL(k_rg_finish, dim3(std::min<unsigned>(n_parts, 4096)), dim3(256), 0, c->stream, (const uint4*)tmp.p, n_records,
                           (uint32_t)(nb - 1), part_shift, n_parts, B, (const uint64_t*)h1off.p, (unsigned long long*)acc.p, (uint4*)P.records.p);
        HIP_TRY(hipGetLastError());
        DevBuf keep = P.records;
        rc = pass_tables(c, acc, l2_local, 1, 0, (uint32_t)nb, budget, &P); if (rc) return rc;
        P.records = keep;
        HIP_TRY(hipStreamSynchronize(c->stream));
        c->release(acc); c->release(tmp); c->release(h1off); c->release(h1);
        if (P.n_records != n_records) return fail(DFK_E_HIP, "regroup lost records");
    }
    c->st.ms_part_scatter += t_regroup.stop();
    for (DevBuf& rb : c->shard_recv) if (rb.p && d_records == rb.p) c->release(rb);      // regrouped: the received copy can go
    if (pass == 0) c->st.n_records = 0;                                  // (the scan left the records this rank SENDS there)
    c->st.n_records += n_records; c->st.n_buckets = nb << S->log2_pass;
    if (!S->run_open) { c->seg_attempt = 0; c->distinct_per_inst = 0.0; rc = count_run_begin(c, &S->R); if (rc) return rc; S->run_open = true; }
    TRACE("pass %u: %llu records, %llu instances, %llu items", pass, (unsigned long long)P.n_records, (unsigned long long)P.n_inst,
          (unsigned long long)P.n_items);
    const dfk_stats before = c->st;
    for (;;) {
        // a pass whose solid k-mers outgrow the room reserved for them is undone and redone with twice the room
        rc = count_snapshot(c, &S->R, false); if (rc) return rc;
        rc = stage_count<K>(c, P, S->R, c->shard_use_bc);
        if (rc != E_SEGMENT_FULL || c->seg_attempt >= 6) break;
        ++c->seg_attempt;
        rc = count_snapshot(c, &S->R, true); if (rc) return rc;
        c->st.n_items = before.n_items; c->st.n_overflow_items = before.n_overflow_items;
    }
    c->seg_attempt = 0;
    if (rc == E_SEGMENT_FULL) rc = DFK_E_NOMEM;
    if (rc) return rc;
    release_pass(c, &P);
    if (pass + 1 < n_passes) return 0;
    // last pass: spectrum, one dense dictionary part, the set that answers the peers' neighbour queries
    rc = count_run_end(c, &S->R); if (rc) return rc;
    S->run_open = false;
    if (c->parts.size() > 1) {
        dfk_ctx::Part all; all.n = c->n_solid;
        rc = c->alloc(all.buf, all.n * 32, "merged solid k-mer entries"); if (rc) return rc;
        uint64_t at = 0;
        for (dfk_ctx::Part& pt : c->parts) {
            if (pt.n) HIP_TRY(hipMemcpyAsync((char*)all.buf.p + 32 * at, pt.buf.p, 32 * pt.n, hipMemcpyDeviceToDevice, c->stream));
            at += pt.n;
        }
        HIP_TRY(hipStreamSynchronize(c->stream));
        for (dfk_ctx::Part& pt : c->parts) c->release(pt.buf);
        c->parts.assign(1, all);
    }
    c->st.reserved[0] = n_passes;
    rc = make_pre_view(c); if (rc) return rc;
    rc = build_set(c); if (rc) return rc;
    HIP_TRY(hipStreamSynchronize(c->stream));
    c->have = true;
    return 0;
}

template <int K>
int shard_adj_queries_typed(dfk_ctx* c, const void** d_keys, uint64_t* send_counts)
{
    const uint32_t world = c->shard_world, lw = log2_exact(world);
    const uint32_t M = c->cfg.minimizer_len;
    PartParams pp{M, (uint32_t)K - M + 1, c->shard_log2_nb, lw, 0, 0, 0};
    for (uint32_t o = 0; o < world; ++o) send_counts[o] = 0;
    c->adj_n = 0; *d_keys = nullptr;
    if (c->cfg.min_freq <= 1 || c->n_solid == 0) return 0;             // BuildReadQGraph48.cc:313
    if (world > 256) return fail(DFK_E_ARG, "more than 256 ranks");
    DevBuf ctr, dbase, list, tkeys, owner;
    int rc = c->alloc(ctr, 8ull * (world + 1), "query counters"); if (rc) return rc;
    HIP_TRY(hipMemsetAsync(ctr.p, 0, 8ull * (world + 1), c->stream));
    unsigned long long* d_n = (unsigned long long*)ctr.p + world;
    const uint4* ents = (const uint4*)c->parts[0].buf.p;
    const unsigned grid = (unsigned)std::min<uint64_t>((c->n_solid + ADJ_ROUND - 1) / ADJ_ROUND, 8192);
    // 1. how many look-ups, then the list of them
    hipLaunchKernelGGL(k_adj_list, dim3(grid), dim3(256), 0, c->stream, ents, c->n_solid, d_n, (uint64_t*)nullptr);
    HIP_TRY(hipGetLastError());
    uint64_t n_items = 0;
    HIP_TRY(hipMemcpyAsync(&n_items, d_n, 8, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    c->adj_n = n_items;
    if (n_items) {
        rc = c->alloc(list, n_items * 8, "neighbour query list"); if (rc) return rc;
        rc = c->alloc(tkeys, n_items * 16, "neighbour query keys (ungrouped)"); if (rc) return rc;
        rc = c->alloc(owner, n_items, "neighbour query owners"); if (rc) return rc;
        HIP_TRY(hipMemsetAsync(d_n, 0, 8, c->stream));
        hipLaunchKernelGGL(k_adj_list, dim3(grid), dim3(256), 0, c->stream, ents, c->n_solid, d_n, (uint64_t*)list.p);
        HIP_TRY(hipGetLastError());
        // 2. canonical neighbour and its owner, densely
        const unsigned g2 = (unsigned)std::min<uint64_t>((n_items + 255) / 256, 8192);
        hipLaunchKernelGGL(HIP_KERNEL_NAME(k_adj_owner<K>), dim3(g2), dim3(256), 0, c->stream, ents, (const uint64_t*)list.p, n_items, pp,
                           (SetSlot*)tkeys.p, (uint8_t*)owner.p, (unsigned long long*)ctr.p);
        HIP_TRY(hipGetLastError());
    }
    std::vector<uint64_t> cnt(world), base(world + 1, 0);
    HIP_TRY(hipMemcpyAsync(cnt.data(), ctr.p, 8ull * world, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    for (uint32_t o = 0; o < world; ++o) { base[o + 1] = base[o] + cnt[o]; send_counts[o] = cnt[o]; }
    if (base[world] != n_items) return fail(DFK_E_HIP, "neighbour queries: %llu listed, %llu routed", (unsigned long long)n_items, (unsigned long long)base[world]);
    rc = c->alloc(c->adj_keys, std::max<uint64_t>(1, n_items) * 16, "neighbour query keys"); if (rc) return rc;
    rc = c->alloc(c->adj_src, std::max<uint64_t>(1, n_items) * 8, "neighbour query sources"); if (rc) return rc;
    if (n_items) {
        // 3. grouped by owner
        rc = c->alloc(dbase, 8ull * (world + 1), "query bases"); if (rc) return rc;
        HIP_TRY(hipMemcpyAsync(dbase.p, base.data(), 8ull * (world + 1), hipMemcpyHostToDevice, c->stream));
        HIP_TRY(hipMemsetAsync(ctr.p, 0, 8ull * world, c->stream));
        const unsigned g3 = (unsigned)std::min<uint64_t>((n_items + ADJ_ROUND - 1) / ADJ_ROUND, 8192);
        hipLaunchKernelGGL(k_adj_place, dim3(g3), dim3(256), 0, c->stream, (const uint64_t*)list.p, (const SetSlot*)tkeys.p,
                           (const uint8_t*)owner.p, n_items, world, (const uint64_t*)dbase.p, (unsigned long long*)ctr.p,
                           (SetSlot*)c->adj_keys.p, (uint64_t*)c->adj_src.p);
        HIP_TRY(hipGetLastError());
    }
    HIP_TRY(hipStreamSynchronize(c->stream));
    c->release(ctr); c->release(dbase); c->release(list); c->release(tkeys); c->release(owner);
    c->st.adj_probes = c->adj_n;
    *d_keys = c->adj_keys.p;
    return 0;
}

} // namespace

extern "C" {

int dfk_shard_begin(dfk_ctx* c, const void* d_packed, uint64_t packed_bytes, const void* d_base_off, const void* d_read_len,
                    const void* d_pq, uint64_t pq_nbytes, const void* d_pq_off, const void* d_bc, uint64_t n_reads,
                    int64_t global_read_offset, uint64_t* n_inst_local)
{
    return guarded([&]() -> int {
    if (!c || !n_inst_local) return fail(DFK_E_ARG, "null argument");
    if (n_reads && (!d_packed || !d_base_off || !d_read_len || !d_pq || !d_pq_off)) return fail(DFK_E_ARG, "null input array");
    HIP_TRY(hipSetDevice(c->device));
    CallClock clock(c, &c->st.ms_trim);
    c->release_all();
    c->st = dfk_stats{}; c->peak = 0;
    c->first_chunk_hint = 8 * (packed_bytes + pq_nbytes + 28 * n_reads) + (1ull << 30);
    Inputs in{(const uint8_t*)d_packed, packed_bytes, (const uint64_t*)d_base_off, (const uint32_t*)d_read_len,
              (const uint8_t*)d_pq, pq_nbytes, (const uint64_t*)d_pq_off, (const int32_t*)d_bc, n_reads};
    uint64_t n_inst = 0;
    int rc;
    switch (c->cfg.K) {
    case 40: rc = stage_trim<40>(c, in, &n_inst); break;
    case 48: rc = stage_trim<48>(c, in, &n_inst); break;
    default: rc = stage_trim<60>(c, in, &n_inst); break;
    }
    // a shard with no good bases is legal as long as some other shard has them: the caller decides
    if (rc == DFK_E_NOGOOD) { rc = 0; n_inst = 0; }
    if (rc) { c->release_all(); return rc; }
    c->sh_in[0] = d_packed; c->sh_in[1] = d_base_off; c->sh_in[2] = d_read_len; c->sh_in[3] = d_pq; c->sh_in[4] = d_pq_off; c->sh_in[5] = d_bc;
    c->sh_packed_bytes = packed_bytes; c->sh_pq_bytes = pq_nbytes; c->sh_n_reads = n_reads; c->sh_n_inst_local = n_inst;
    c->sh_read_id0 = global_read_offset; c->shard_use_bc = d_bc != nullptr; c->shard_open = true;
    c->n_reads = n_reads; c->st.n_reads = n_reads; c->st.n_inst = n_inst;
    *n_inst_local = n_inst;
    return 0;
    });
}

int dfk_shard_begin_host(dfk_ctx* c, const uint8_t* packed, const uint64_t* base_off, const uint32_t* read_len,
                         const uint8_t* pq, const uint64_t* pq_off, const int32_t* bc, uint64_t n_reads,
                         int64_t global_read_offset, uint64_t* n_inst_local)
{
    return guarded([&]() -> int {
    if (!c || !n_inst_local) return fail(DFK_E_ARG, "null argument");
    if (n_reads && (!packed || !base_off || !read_len || !pq || !pq_off)) return fail(DFK_E_ARG, "null input array");
    HIP_TRY(hipSetDevice(c->device));
    c->release_all();
    // The tables are this rank's slice of the whole set's tables and keep the whole set's offsets: only the bytes of
    // this rank's reads are uploaded, and the device pointers handed on are biased so that those offsets address them.
    int rd = 0;
    auto at = [&](const void* tab, uint64_t i) { uint64_t v = 0; if (!rd) rd = host_read(c, &v, (const char*)tab + 8 * i, 8); return v; };   // (tables may sit at any address, or in a hinted file)
    const uint64_t b0 = n_reads ? at(base_off, 0) & ~(uint64_t)3 : 0, b1 = n_reads ? at(base_off, n_reads) : 0;
    const uint64_t q0 = n_reads ? at(pq_off, 0) : 0, q1 = n_reads ? at(pq_off, n_reads) : 0;
    if (rd) return rd;
    if (b1 < b0 || q1 < q0) return fail(DFK_E_INPUT, "offset tables are not ascending");
    int rc = 0;
    Timer t(c->stream);
    t.start();
    auto up = [&](int slot, const void* h, uint64_t bytes) {
        if (rc) return;
        if (hipMalloc(&c->sh_staged[slot], bytes + 64) != hipSuccess) { (void)hipGetLastError(); rc = fail(DFK_E_NOMEM, "no room on the device for %llu bytes of input", (unsigned long long)bytes); return; }
        rc = upload(c, c->sh_staged[slot], h, bytes);
    };
    up(0, packed + b0, b1 - b0);
    up(1, base_off, (n_reads + 1) * 8);
    up(2, read_len, n_reads * 4);
    up(3, pq + q0, q1 - q0);
    up(4, pq_off, (n_reads + 1) * 8);
    if (bc) up(5, bc, n_reads * 4);
    const float ms_up = t.stop();
    if (rc) { for (void*& p : c->sh_staged) if (p) { (void)hipFree(p); p = nullptr; } return rc; }
    const uint64_t staged = (b1 - b0) + (q1 - q0) + (n_reads + 1) * 16 + n_reads * 8 + 6 * 64;
    void* keep[6]; memcpy(keep, c->sh_staged, sizeof keep); memset(c->sh_staged, 0, sizeof keep);   // (dfk_shard_begin starts with release_all)
    rc = dfk_shard_begin(c, (const char*)keep[0] - b0, b1, keep[1], keep[2], (const char*)keep[3] - q0, q1, keep[4], bc ? keep[5] : nullptr, n_reads,
                         global_read_offset, n_inst_local);
    memcpy(c->sh_staged, keep, sizeof keep);
    if (rc) { for (void*& p : c->sh_staged) if (p) { (void)hipFree(p); p = nullptr; } return rc; }
    c->sh_b0 = b0; c->sh_b1 = b1; c->sh_q0 = q0; c->sh_q1 = q1; c->sh_staged_reads = n_reads;
    // the staged inputs share the device with the arena for the whole run (given back by release_all)
    c->budget_taken = std::min(c->budget, staged);
    c->budget -= c->budget_taken;
    c->st.ms_upload = ms_up;
    return 0;
    });
}

int dfk_shard_plan(dfk_ctx* c, uint32_t world, uint64_t n_inst_global, uint32_t* log2_passes)
{
    return guarded([&]() -> int {
    if (!c || !log2_passes) return fail(DFK_E_ARG, "null argument");
    if (!c->shard_open) return fail(DFK_E_STATE, "dfk_shard_begin has not been called");
    if (world == 0 || (world & (world - 1)) || world > 64) return fail(DFK_E_ARG, "world must be a power of two <= 64");
    HIP_TRY(hipSetDevice(c->device));
    CallClock clock(c, nullptr);
    switch (c->cfg.K) {
    case 40: return shard_plan_typed<40>(c, world, n_inst_global, log2_passes);
    case 48: return shard_plan_typed<48>(c, world, n_inst_global, log2_passes);
    default: return shard_plan_typed<60>(c, world, n_inst_global, log2_passes);
    }
    });
}

int dfk_shard_partition_begin(dfk_ctx* c, uint32_t world, uint64_t n_inst_global, uint32_t log2_passes, uint32_t pass, int defer,
                              const void** d_records, uint64_t* send_counts)
{
    return guarded([&]() -> int {
    if (!c || !d_records || !send_counts) return fail(DFK_E_ARG, "null argument");
    if (!c->shard_open) return fail(DFK_E_STATE, "dfk_shard_begin has not been called");
    if (world == 0 || (world & (world - 1)) || world > 64) return fail(DFK_E_ARG, "world must be a power of two <= 64");
    if (log2_passes > 8 || pass >= (1u << log2_passes)) return fail(DFK_E_ARG, "pass %u of 2^%u", pass, log2_passes);
    HIP_TRY(hipSetDevice(c->device));
    CallClock clock(c, nullptr);
    switch (c->cfg.K) {
    case 40: return shard_partition_begin_typed<40>(c, world, n_inst_global, log2_passes, pass, defer != 0, d_records, send_counts);
    case 48: return shard_partition_begin_typed<48>(c, world, n_inst_global, log2_passes, pass, defer != 0, d_records, send_counts);
    default: return shard_partition_begin_typed<60>(c, world, n_inst_global, log2_passes, pass, defer != 0, d_records, send_counts);
    }
    });
}

int dfk_shard_partition_end(dfk_ctx* c, uint32_t pass)
{
    return guarded([&]() -> int {
    if (!c) return fail(DFK_E_ARG, "null context");
    if (!c->shard_open || !c->shard_state) return fail(DFK_E_STATE, "dfk_shard_partition_begin has not been called");
    HIP_TRY(hipSetDevice(c->device));
    CallClock clock(c, nullptr);
    return shard_partition_end(c, pass);
    });
}

int dfk_shard_partition(dfk_ctx* c, uint32_t world, uint64_t n_inst_global, uint32_t log2_passes, uint32_t pass,
                        const void** d_records, uint64_t* send_counts)
{
    const int rc = dfk_shard_partition_begin(c, world, n_inst_global, log2_passes, pass, 0, d_records, send_counts);
    return rc ? rc : dfk_shard_partition_end(c, pass);
}

int dfk_shard_recv_buffer(dfk_ctx* c, uint64_t n_records, void** d_buf)
{
    return guarded([&]() -> int {
    if (!c || !d_buf) return fail(DFK_E_ARG, "null argument");
    if (!c->shard_open) return fail(DFK_E_STATE, "dfk_shard_begin has not been called");
    HIP_TRY(hipSetDevice(c->device));
    CallClock clock(c, nullptr);
    DevBuf& rb = c->shard_recv[c->shard_recv_seq++ & 1];           // the other one may still be waiting to be counted
    c->release(rb);
    int rc = c->alloc(rb, std::max<uint64_t>(1, n_records) * 32, "received records"); if (rc) return rc;
    *d_buf = rb.p;
    return 0;
    });
}

int dfk_shard_count(dfk_ctx* c, const void* d_records, uint64_t n_records, uint32_t pass)
{
    return guarded([&]() -> int {
    if (!c) return fail(DFK_E_ARG, "null context");
    if (!c->shard_open || !c->shard_state) return fail(DFK_E_STATE, "dfk_shard_partition has not been called");
    if (n_records && !d_records) return fail(DFK_E_ARG, "null records");
    HIP_TRY(hipSetDevice(c->device));
    CallClock clock(c, nullptr);
    switch (c->cfg.K) {
    case 40: return shard_count_typed<40>(c, d_records, n_records, pass);
    case 48: return shard_count_typed<48>(c, d_records, n_records, pass);
    default: return shard_count_typed<60>(c, d_records, n_records, pass);
    }
    });
}

int dfk_shard_adj_queries(dfk_ctx* c, const void** d_keys, uint64_t* send_counts)
{
    return guarded([&]() -> int {
    if (!c || !d_keys || !send_counts) return fail(DFK_E_ARG, "null argument");
    if (!c->have) return fail(DFK_E_STATE, "dfk_shard_count has not completed");
    HIP_TRY(hipSetDevice(c->device));
    CallClock clock(c, &c->st.ms_adjacency);
    switch (c->cfg.K) {
    case 40: return shard_adj_queries_typed<40>(c, d_keys, send_counts);
    case 48: return shard_adj_queries_typed<48>(c, d_keys, send_counts);
    default: return shard_adj_queries_typed<60>(c, d_keys, send_counts);
    }
    });
}

int dfk_shard_adj_answer(dfk_ctx* c, const void* d_keys, uint64_t n_keys, void* d_present)
{
    return guarded([&]() -> int {
    if (!c) return fail(DFK_E_ARG, "null context");
    if (!c->have || !c->set.p) return fail(DFK_E_STATE, "dfk_shard_count has not completed");
    if (n_keys == 0) return 0;
    if (!d_keys || !d_present) return fail(DFK_E_ARG, "null argument");
    HIP_TRY(hipSetDevice(c->device));
    CallClock clock(c, &c->st.ms_adjacency);
    hipLaunchKernelGGL(k_adj_answer, dim3((unsigned)((n_keys + 255) / 256)), dim3(256), 0, c->stream, (const SetSlot*)d_keys, n_keys,
                       (const SetSlot*)c->set.p, c->set_slots, (uint8_t*)d_present);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(c->stream));
    return 0;
    });
}

int dfk_shard_adj_apply(dfk_ctx* c, const void* d_present, uint64_t n_keys)
{
    return guarded([&]() -> int {
    if (!c) return fail(DFK_E_ARG, "null context");
    if (!c->have) return fail(DFK_E_STATE, "dfk_shard_count has not completed");
    if (n_keys != c->adj_n) return fail(DFK_E_ARG, "expected %llu answers, got %llu", (unsigned long long)c->adj_n, (unsigned long long)n_keys);
    HIP_TRY(hipSetDevice(c->device));
    CallClock clock(c, &c->st.ms_adjacency);
    if (n_keys) {
        if (!d_present) return fail(DFK_E_ARG, "null answers");
        hipLaunchKernelGGL(k_adj_apply, dim3((unsigned)((n_keys + 255) / 256)), dim3(256), 0, c->stream, (uint4*)c->parts[0].buf.p,
                           (const uint64_t*)c->adj_src.p, (const uint8_t*)d_present, n_keys);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipStreamSynchronize(c->stream));
    }
    if (c->n_solid) {                                                  // the pad field carried the unresolved bits
        hipLaunchKernelGGL(k_clear_pad, dim3((unsigned)((c->n_solid + 255) / 256)), dim3(256), 0, c->stream, (uint4*)c->parts[0].buf.p, c->n_solid);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipStreamSynchronize(c->stream));
    }
    c->release(c->adj_keys); c->release(c->adj_src); c->release(c->set);
    c->sorted_ok = false;
    return 0;
    });
}

// ---- after a sharded run: the whole dictionary on one rank (the graph and the read paths are built from a whole
// dictionary: buildEdges / buildHBVFromEdges / pathReads run after createDict whatever the thread count,
// BuildReadQGraph48.cc:1636,1664)
int dfk_shard_dict_share(dfk_ctx* c, const void** d_entries, uint64_t* n_entries)
{
    if (!c || !d_entries || !n_entries) return fail(DFK_E_ARG, "null argument");
    if (!c->have) return fail(DFK_E_STATE, "no completed count");
    if (c->parts.size() > 1) return fail(DFK_E_STATE, "the dictionary is in %zu parts: a sharded run leaves one", c->parts.size());
    *d_entries = c->parts.empty() ? nullptr : c->parts[0].buf.p;
    *n_entries = c->parts.empty() ? 0 : c->parts[0].n;
    return 0;
}

int dfk_shard_dict_adopt(dfk_ctx* c, uint64_t n_entries, void** d_room)
{
    return guarded([&]() -> int {
    if (!c || !d_room) return fail(DFK_E_ARG, "null argument");
    if (!c->have) return fail(DFK_E_STATE, "no completed count");
    HIP_TRY(hipSetDevice(c->device));
    *d_room = nullptr;
    // what the exchange of the run still holds goes first: the staged reads of this rank, the shard tables
    if (c->shard_state) {
        ShardState* S = shard_state(c);
        for (DevBuf* d : {&S->T.acc, &S->T.summ, &S->T.classes, &S->T.ovf_list, &S->T.class_hist}) c->release(*d);
        c->shard_state_free(c->shard_state); c->shard_state = nullptr;
    }
    // (under DFK_F_KEEP_INPUTS the staged reads stay: the rank paths them once the graph is built, dfk_paths_build(ctx, NULL...))
    if (!(c->cfg.flags & DFK_F_KEEP_INPUTS)) {
        for (void*& p : c->sh_staged) if (p) { (void)hipFree(p); p = nullptr; }
        c->budget += c->budget_taken; c->budget_taken = 0; c->sh_staged_reads = 0;
    } else if (c->sh_staged[5]) { (void)hipFree(c->sh_staged[5]); c->sh_staged[5] = nullptr; }      // (the barcodes are createDict's alone)
    for (DevBuf* d : {&c->shard_send[0], &c->shard_send[1], &c->shard_recv[0], &c->shard_recv[1], &c->adj_keys, &c->adj_src, &c->set}) c->release(*d);
    if (!n_entries) return 0;
    dfk_ctx::Part pt; pt.n = n_entries;
    int rc = c->alloc(pt.buf, n_entries * 32, "solid k-mer entries of the other ranks"); if (rc) return rc;
    *d_room = pt.buf.p;
    c->parts.push_back(pt);
    return 0;
    });
}

int dfk_shard_dict_whole(dfk_ctx* c)
{
    return guarded([&]() -> int {
    if (!c) return fail(DFK_E_ARG, "null context");
    if (!c->have) return fail(DFK_E_STATE, "no completed count");
    uint64_t n = 0;
    for (const dfk_ctx::Part& pt : c->parts) n += pt.n;
    c->n_solid = n; c->st.n_solid = n;
    if (c->shard_state) { c->shard_state_free(c->shard_state); c->shard_state = nullptr; }
    c->shard_world = 1; c->shard_open = false;
    c->sorted_ok = c->sorted_pre_ok = false;
    for (dfk_ctx::Part& pt : c->parts) c->release(pt.pre);                 // (a pre-adjacency view of one share means nothing for the whole)
    return 0;
    });
}

} // extern "C"
