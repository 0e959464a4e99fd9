// superplus_amd/csrc/dfk_arena.h -- where libdfk.so's device memory goes: the arena every run allocates from and
// the planner that sizes a pass from what the arena has free.  Host-only: the arena hands out addresses and never
// dereferences one, so both run on a CPU against a backing store that only counts (tests/cpp/test_arena.cc).
#pragma once
#include <algorithm>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <string>
#include <vector>

namespace dfk {

struct DevBuf {
    void* p = nullptr; size_t bytes = 0;
    bool sub = false;            // carved from a pass block (Arena::PassBlock): given back with the block, not on its own
};

// Where a block goes.  The two kinds sit at opposite ends of a chunk so that they do not fragment each other.
enum class Place {
    High,                        // per-pass blocks and temporaries: the upper end of the highest free block that fits, or the current pass block
    Low,                         // long-lived (dictionary parts, goodLens, bucket counters, summaries): the lower end of the lowest, where the dictionary grows
};

// Device memory comes from a few large chunks that are kept for the life of the context and managed
// by first-fit free lists with coalescing.  hipMalloc/hipFree of multi-GB blocks cost milliseconds to
// seconds each (and hipFree synchronises the device); a 30x human run moves hundreds of GB per pass.
class Arena {
public:
    enum { E_BUDGET = 1, E_FRAGMENTED, E_BACKING };  // what alloc returns when it fails; the message is in `err`
    struct Free { uint64_t off, bytes; };
    // Everything one pass holds while it is in flight (bucket tables, records) comes out of ONE
    // arena block, so that two passes in flight plus the growing dictionary never interleave: the blocks of
    // successive passes do not grow, so each fits the hole left by the pass before the running one.
    struct PassBlock { DevBuf block; size_t used = 0; };
    struct Current {                                 // while it lives, Place::High allocations are bumped out of the block when they fit
        Arena& a;
        Current(Arena& ar, PassBlock& blk) : a(ar) { a.sub = &blk; }
        ~Current() { a.sub = nullptr; }
    };
    typedef void* (*GetFn)(uint64_t bytes, const char** why);   // a chunk of the backing store, or nullptr and the reason
    typedef void (*GiveFn)(void* p);

    uint64_t budget = 0, held = 0, peak = 0;
    uint64_t reserved = 0;                           // sum of chunk sizes
    uint64_t alloc_seq = 0;                          // the journal's clock: release_since(a value of it) undoes what came later
    uint64_t first_chunk_hint = 0;                   // set from the input size before a run: one big chunk, no growth
    bool trace = false;
    std::string err;

    Arena(GetFn get_, GiveFn give_) : get(get_), give(give_) {}

    int alloc(DevBuf& b, size_t bytes, const char* what, Place where = Place::High)
    {
        bytes = bytes ? (bytes + 255) & ~(size_t)255 : 256;
        if (sub && where == Place::High && sub->used + bytes <= sub->block.bytes) {
            b.p = (char*)sub->block.p + sub->used; b.bytes = bytes; b.sub = true;
            sub->used += bytes;
            return 0;
        }
        if (held + bytes > budget)
            return fail(E_BUDGET, "HBM budget exceeded allocating %zu bytes for %s (held %llu, budget %llu)",
                        bytes, what, (unsigned long long)held, (unsigned long long)budget);
        bool ok = false;
        for (Chunk& k : chunks) if (carve(k, bytes, b, where)) { ok = true; break; }
        if (!ok) {
            // grow: the first chunk is sized from the input (a run needs a few times its input), later ones
            // twice the request (later requests reuse the slack); never past the budget
            uint64_t want = std::max<uint64_t>(2 * (uint64_t)bytes, 64ull << 20);
            if (chunks.empty()) want = std::max<uint64_t>(want, std::min<uint64_t>(first_chunk_hint, budget));
            if (reserved + want > budget) { drop_empty_chunks(); want = std::min<uint64_t>(want, budget > reserved ? budget - reserved : 0); }
            want &= ~(uint64_t)0xFFF;                  // blocks carved from the top of a chunk must stay aligned
            if (want < bytes) {
                if (trace) {
                    for (const Chunk& k : chunks) trace_free(k.free_list);
                    for (const Owned& o : owned) if (o.bytes >= (1ull << 28)) fprintf(stderr, "[dfk]   held %.2f GB at %.2f GB (#%llu)\n", o.bytes / 1e9, ((char*)o.p - chunks[0].p) / 1e9, (unsigned long long)o.seq);
                }
                return fail(E_FRAGMENTED, "HBM budget exhausted by fragmentation allocating %zu bytes for %s", bytes, what);
            }
            const char* why = "";
            void* p = get(want, &why);
            if (!p && want > bytes) { want = bytes; p = get(want, &why); }
            if (!p) return fail(E_BACKING, "hipMalloc(%llu) for %s: %s", (unsigned long long)want, what, why);
            chunks.push_back(Chunk{(char*)p, want, {Free{0, want}}});
            reserved += want;
            say("new device chunk %p, %.2f GB (reserved %.2f of %.2f GB)", p, want / 1e9, (reserved) / 1e9, budget / 1e9);
            carve(chunks.back(), bytes, b, where);
        }
        held += bytes; peak = std::max(peak, held);
        owned.push_back(Owned{b.p, (uint64_t)bytes, ++alloc_seq});
        if (bytes >= (1ull << 30)) say("alloc %-28s %8.2f GB at %p (%s), held %.2f GB", what, bytes / 1e9, b.p, where == Place::Low ? "low" : "high", held / 1e9);
        return 0;
    }
    // the largest block alloc() could hand out now: a free block of a chunk, or a new chunk within the budget
    uint64_t largest_allocatable() const
    {
        uint64_t best = budget > reserved ? (budget - reserved) & ~(uint64_t)0xFFF : 0;
        for (const Chunk& k : chunks) for (const Free& f : k.free_list) best = std::max<uint64_t>(best, f.bytes);
        return std::min<uint64_t>(best, budget > held ? budget - held : 0);
    }
    // every block alloc() could carve from now: the chunks' free blocks and, within the budget, a new chunk (offsets are
    // within each block's own chunk; a new chunk's is 0)
    std::vector<Free> allocatable_blocks() const
    {
        std::vector<Free> all;
        for (const Chunk& k : chunks) all.insert(all.end(), k.free_list.begin(), k.free_list.end());
        const uint64_t grow = budget > reserved ? (budget - reserved) & ~(uint64_t)0xFFF : 0;
        if (grow) all.push_back(Free{0, grow});
        return all;
    }
    void release(DevBuf& b)
    {
        if (!b.p) return;
        if (b.sub) { b = DevBuf{}; return; }
        auto it = std::find_if(owned.begin(), owned.end(), [&](const Owned& o) { return o.p == b.p; });
        if (it != owned.end()) owned.erase(it);
        for (Chunk& k : chunks)
            if ((char*)b.p >= k.p && (char*)b.p < k.p + k.bytes) {
                std::vector<Free>& fl = k.free_list;
                const uint64_t off = (uint64_t)((char*)b.p - k.p);
                size_t i = 0;
                while (i < fl.size() && fl[i].off < off) ++i;
                fl.insert(fl.begin() + i, Free{off, b.bytes});
                if (i + 1 < fl.size() && fl[i].off + fl[i].bytes == fl[i + 1].off) { fl[i].bytes += fl[i + 1].bytes; fl.erase(fl.begin() + i + 1); }
                if (i > 0 && fl[i - 1].off + fl[i - 1].bytes == fl[i].off) { fl[i - 1].bytes += fl[i].bytes; fl.erase(fl.begin() + i); }
                break;
            }
        held -= b.bytes; b.p = nullptr; b.bytes = 0;
    }
    // keep only the first `keep` bytes of a block: a reservation made for an upper bound is cut to what was
    // needed; the tail goes back to the free room above it (long-lived blocks grow upwards)
    void shrink(DevBuf& b, size_t keep)
    {
        keep = keep ? (keep + 255) & ~(size_t)255 : 256;
        if (!b.p || keep >= b.bytes) return;
        auto it = std::find_if(owned.begin(), owned.end(), [&](const Owned& o) { return o.p == b.p; });
        DevBuf tail; tail.p = (char*)b.p + keep; tail.bytes = b.bytes - keep;
        b.bytes = keep;
        if (it != owned.end()) { it->bytes = keep; owned.push_back(Owned{tail.p, (uint64_t)tail.bytes, it->seq}); }
        else owned.push_back(Owned{tail.p, (uint64_t)tail.bytes, alloc_seq});
        release(tail);
    }
    // give back everything allocated after `mark` (= alloc_seq at some earlier moment) except the block of `keep`:
    // what an abandoned pass left behind.  The DevBufs that pointed at those blocks are dead; the caller resets them.
    void release_since(uint64_t mark, const DevBuf* keep = nullptr)
    {
        for (size_t i = owned.size(); i-- > 0;)
            if (owned[i].seq > mark && !(keep && owned[i].p == keep->p)) { DevBuf b; b.p = owned[i].p; b.bytes = owned[i].bytes; release(b); }
    }
    void drop_empty_chunks()
    {
        for (size_t i = 0; i < chunks.size();)
            if (chunks[i].free_list.size() == 1 && chunks[i].free_list[0].bytes == chunks[i].bytes) drop_chunk(i);
            else ++i;
    }
    void drop_pool() { while (!chunks.empty()) drop_chunk(chunks.size() - 1); }
    // memory the caller already holds becomes a chunk; it goes back to the backing store at the next reset()
    // (a run plans with ONE large chunk)
    void adopt(void* p, uint64_t bytes) { chunks.push_back(Chunk{(char*)p, bytes, {Free{0, bytes}}, true}); reserved += bytes; }
    // whatever is still allocated is forgotten: the arena is declared empty
    void reset()
    {
        owned.clear(); held = 0;
        for (size_t i = 0; i < chunks.size();) if (chunks[i].adopted) drop_chunk(i); else ++i;
        for (Chunk& k : chunks) k.free_list.assign(1, Free{0, k.bytes});
    }
    // the free blocks by rising offset, when the arena is one chunk (what a run plans with); nullptr otherwise
    const std::vector<Free>* free_blocks() const { return chunks.size() == 1 ? &chunks[0].free_list : nullptr; }
    uint64_t offset_of(const DevBuf& b) const          // of a block in its chunk
    {
        for (const Chunk& k : chunks) if ((char*)b.p >= k.p && (char*)b.p < k.p + k.bytes) return (uint64_t)((char*)b.p - k.p);
        return 0;
    }
    static void trace_free(const std::vector<Free>& fl) { for (const Free& f : fl) fprintf(stderr, "[dfk]   free %.2f GB at %.2f GB\n", f.bytes / 1e9, f.off / 1e9); }

private:
    friend struct ArenaTest;                         // tests/cpp/test_arena.cc checks the invariants on the lists themselves
    struct Chunk { char* p; uint64_t bytes; std::vector<Free> free_list; bool adopted = false; };     // free_list sorted by offset
    struct Owned { void* p; uint64_t bytes, seq; };
    GetFn get; GiveFn give;
    std::vector<Chunk> chunks;
    std::vector<Owned> owned;                        // live blocks, in allocation order
    PassBlock* sub = nullptr;                        // see Current

    bool carve(Chunk& k, size_t bytes, DevBuf& b, Place where)
    {
        if (where == Place::High) {
            for (size_t i = k.free_list.size(); i-- > 0;)
                if (k.free_list[i].bytes >= bytes) {
                    k.free_list[i].bytes -= bytes;
                    b.p = k.p + k.free_list[i].off + k.free_list[i].bytes; b.bytes = bytes;
                    if (!k.free_list[i].bytes) k.free_list.erase(k.free_list.begin() + i);
                    return true;
                }
            return false;
        }
        for (size_t i = 0; i < k.free_list.size(); ++i)
            if (k.free_list[i].bytes >= bytes) {
                b.p = k.p + k.free_list[i].off; b.bytes = bytes;
                k.free_list[i].off += bytes; k.free_list[i].bytes -= bytes;
                if (!k.free_list[i].bytes) k.free_list.erase(k.free_list.begin() + i);
                return true;
            }
        return false;
    }
    void drop_chunk(size_t i) { give(chunks[i].p); reserved -= chunks[i].bytes; chunks.erase(chunks.begin() + i); }
    int fail(int code, const char* fmt, ...)
    {
        char buf[512];
        va_list ap; va_start(ap, fmt); vsnprintf(buf, sizeof buf, fmt, ap); va_end(ap);
        err = buf;
        return code;
    }
    void say(const char* fmt, ...) const
    {
        if (!trace) return;
        fputs("[dfk] ", stderr);
        va_list ap; va_start(ap, fmt); vfprintf(stderr, fmt, ap); va_end(ap);
        fputc('\n', stderr); fflush(stderr);
    }
};

// ------------------------------------------------------------------ what a pass holds, and how many buckets fit
// The two sizes below are what is allocated.  The planner further down asks for a little more than either -- 81 B
// per bucket and 32.5 B per record against 1.01 x (80 and 32), 1.12 x the observed solid/instance ratio against
// 1.10 x, the constant ends (16 MB, 65536 entries, the workgroups' chunk ends) under `fixed` -- so that a planned
// range still fits when the hash has dealt it a little more than its share.  Its figures were tuned on the machine:
// whoever changes what a pass holds changes the size here and follows with the planner's figure.

// the block of a pass over n of sub_nb buckets: tables (80 B per bucket with their scratch) and records (an
// estimate: what does not fit the block falls back to the open arena)
inline uint64_t pass_block_bytes(uint32_t n, uint32_t sub_nb, uint64_t n_records)
{
    const double share = (double)n / sub_nb;
    return (uint64_t)(1.01 * (80.0 * n + 32.0 * share * (double)n_records)) + (16ull << 20);
}
// solid k-mers a pass of n_inst instances is expected to emit at most (entries of its part's reservation, before
// the chunk ends): every one has >= min_freq instances, and buckets are hash-distributed, so once a pass has been
// counted the solid/instance ratio holds to a fraction of a percent
inline uint64_t part_entries(uint64_t n_inst, uint32_t min_freq, uint64_t inst_seen, uint64_t solid_seen)
{
    const uint64_t cap = n_inst / std::max<uint32_t>(1, min_freq) + 1;
    if (inst_seen) return std::min<uint64_t>(cap, (uint64_t)(1.10 * (double)solid_seen / (double)inst_seen * (double)n_inst) + 65536);
    return std::min<uint64_t>(cap, n_inst / 10 + (1u << 20));       // first pass: a prior (30x data: n_inst/15, 58x: n_inst/28); too small -> redone
}

struct PlanInputs {
    double room;                          // budget - held
    uint32_t sub_nb, lo;                  // fine buckets of the set; first one not yet in a pass
    uint64_t n_inst, n_records;           // of the whole set
    uint64_t inst_seen, solid_seen;       // of the passes counted so far
    uint32_t min_freq; unsigned seg_attempt;
    double plan_derate;                   // share of the free HBM a pass is planned into
    bool overlap;                         // the next range is scattered while this one is counted
    double first_div, growth;             // DFK_PLAN_FIRST, DFK_PLAN_GROWTH
    bool trace;
};
struct RunningPass { uint64_t bytes_held; uint64_t n_inst; uint32_t n_buckets; uint64_t block_off; };

// How many buckets fit the arena's actual free blocks `fl` (one chunk).  A pass block goes to the highest free
// block that holds it -- now, beside the running pass.  The reservation for its part is made later, when the
// running pass's block is gone, and goes to the lowest free block (the dictionary grows upwards): it has to fit
// there, or it lands higher up and cuts the room of later blocks.  Largest n for which both hold, by bisection.
inline double fit_free_blocks(const std::vector<Arena::Free>* fl_, double per_block, double per_res, const RunningPass& run)
{
    if (!fl_ || fl_->empty()) return 1e300;
    const std::vector<Arena::Free>& fl = *fl_;
    auto feasible = [&](double n) {
        const uint64_t B = (uint64_t)(per_block * n / 0.98) + 1;
        size_t at = fl.size();
        for (size_t i = fl.size(); i-- > 0;) if (fl[i].bytes >= B) { at = i; break; }
        if (at == fl.size()) return false;
        // free list once the running block is gone and the new block is in place (at the upper end of fl[at])
        std::vector<Arena::Free> h(fl.begin(), fl.end());
        h[at].bytes -= B;
        h.push_back(Arena::Free{run.block_off, run.bytes_held});
        std::sort(h.begin(), h.end(), [](const Arena::Free& a, const Arena::Free& b) { return a.off < b.off; });
        uint64_t low_off = 0, low_bytes = 0; bool have = false;
        for (const Arena::Free& f : h) {                               // the lowest run of adjacent free blocks
            if (!f.bytes) continue;
            if (!have) { low_off = f.off; low_bytes = f.bytes; have = true; }
            else if (low_off + low_bytes == f.off) low_bytes += f.bytes;
            else break;
        }
        return per_res * n <= 0.98 * (double)low_bytes;
    };
    double lo = 0.0, hi = 0.0;
    for (const Arena::Free& f : fl) hi = std::max(hi, 0.98 * (double)f.bytes / per_block);
    if (feasible(hi)) return hi;
    for (int it = 0; it < 30; ++it) { const double mid = 0.5 * (lo + hi); if (feasible(mid)) lo = mid; else hi = mid; }
    return lo;
}

// How many fine buckets the next pass may take, from what is free now.  A pass holds its bucket tables, its
// records (32 B each) and its dense part of the dictionary (reserved when the pass is counted); the parts of
// earlier passes stay resident, so later passes are smaller.  Buckets are hash-distributed, so a range holds
// its share of the records and instances to within a fraction of a percent.
// `running` != null: the range is scattered while that pass is being counted, so (1) its tables and records
// must fit beside everything the running pass holds, and (2) its part must fit once the running pass has been
// released.
inline uint32_t plan_range(const PlanInputs& in, const std::vector<Arena::Free>* free_blocks, const RunningPass* running)
{
    const double room = in.room;
    const uint32_t sub_nb = in.sub_nb;
    const double inst_per = (double)in.n_inst / sub_nb, rec_per = (double)in.n_records / sub_nb;
    // solid k-mers per instance: observed on the passes done so far, else the prior part_entries starts from
    double ratio = in.inst_seen ? 1.12 * (double)in.solid_seen / (double)in.inst_seen : 1.0 / 10.0;
    ratio = std::min(ratio, 1.0 / std::max<uint32_t>(1, in.min_freq));
    const double per_in = 81.0 + 32.5 * rec_per;                                         // tables and records: the pass block
    const double per_seg = 0.0;                                                                       // (workgroups write straight into the part's reservation: nothing else per pass)
    const double per_out = 32.0 * ratio * inst_per * (double)(1u << in.seg_attempt);                  // the part's reservation
    const double fixed = 120e6;                                       // chunk ends left empty by the workgroups (67 MB), small tables
    const double left = (double)(sub_nb - in.lo);
    double fit;
    if (!running) {
        fit = room > fixed ? (room - fixed) / (per_in + per_out) : 0.0;
        // more than one pass to go: leave room for the records of the next one, which is scattered while this
        // one is counted (passes of equal or decreasing size also keep the arena from fragmenting: each new
        // range fits the hole left by the pass before the running one)
        if (in.plan_derate * fit < left && in.overlap) {
            fit = room > fixed ? (room - fixed) / (2.0 * per_in + per_seg + per_out) : 0.0;
            // the very first scatter has nothing to hide under: keep it short (its fixed cost, reading every
            // summary, is paid anyway; a tenth of the buckets -- a sixteenth while k_count ran at 75 G instances/s
            // and a range could grow by 1.3 from pass to pass -- measured: DFK_PLAN_FIRST / DFK_PLAN_GROWTH, tools/plan_sweep.sh)
            if (in.lo == 0) fit = std::min(fit, (double)sub_nb / in.first_div / in.plan_derate);
        }
    } else {
        const double now = room - fixed;                              // (the running pass's part is reserved already)
        const double later = room + (double)running->bytes_held - fixed;
        if (in.trace) {
            fprintf(stderr, "[dfk] plan: now %.1f%% later %.1f%% geometry %.1f%% balance %.1f%% (room %.1f GB, running block %.1f GB)\n",
                    100 * 0.9 * now / (per_in + per_seg) / sub_nb, 100 * later / (per_in + per_out) / sub_nb,
                    100 * fit_free_blocks(free_blocks, per_in + per_seg, per_out - per_seg, *running) / sub_nb,
                    100 * std::max(0.0, room + (double)running->bytes_held - fixed) / (2.0 * (per_in + per_seg) + (per_out - per_seg)) / sub_nb,
                    room / 1e9, running->bytes_held / 1e9);
            if (free_blocks) Arena::trace_free(*free_blocks);
            fflush(stderr);
        }
        // (a range that does not fit beside the running pass loses the overlap: plan it with more slack --
        // the free room is in several pieces by now)
        fit = std::max(0.0, std::min(0.9 * now / (per_in + per_seg), later / (per_in + per_out)));
        fit = std::min(fit, fit_free_blocks(free_blocks, per_in + per_seg, per_out - per_seg, *running) / in.plan_derate);
        // and leave the pass after this one (planned while this one is counted, the running one gone by then)
        // a block of the same size: greedy ranges alternate between huge and tiny
        fit = std::min(fit, std::max(0.0, room + (double)running->bytes_held - fixed) / (2.0 * (per_in + per_seg) + (per_out - per_seg)));
    }
    double n = in.plan_derate * fit;
    // the range is scattered while the running pass is counted: no larger than what that count hides (beside
    // k_count a sweep moves a range's records about 1.15 times as fast as k_count counts them -- 8.3 ms against 9.6 ms
    // per percent of the human-scale set's buckets -- after ~10 ms of reading masks; with 1.3, the value from when
    // k_count ran at 75 G instances/s, the first three counts each waited 13-18 ms for the records of the next)
    if (running && in.overlap) n = std::min(n, in.growth * (double)running->n_buckets);
    if (left <= 0.99 * fit && left < 1.06 * n) n = left;              // no sliver of a last pass if the rest (almost certainly) fits
    else if (left > n && left < 1.3 * n) n = 0.5 * left + 1.0;        // two even passes rather than a big one and a sliver (1.7 while the cliff of section 9 was unexplained: a big count beside a small sweep)
    n = std::min(n, left);
    if (n < 16.0) return running ? 0u : (uint32_t)std::min(16.0, left);
    return (uint32_t)n;
}

} // namespace dfk
