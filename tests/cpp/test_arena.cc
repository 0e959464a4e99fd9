// tests/cpp/test_arena.cc -- the device arena and the pass planner of superplus_amd/csrc/dfk_arena.h on a CPU.  The
// backing store hands out addresses from a counter and touches no memory, so a 180-GB arena costs nothing; one step
// of the default benchmark is replayed at full size.  One "name: ok" line per case, exit status 1 if any failed.
//   g++ -O1 -std=c++17 -Wall -o test_arena tests/cpp/test_arena.cc && ./test_arena
// With a file name as its argument the program also writes there every address, error and planned range it sees:
// two builds of the header behave alike exactly when they write the same file.
#include "../../superplus_amd/csrc/dfk_arena.h"
#include <random>

using namespace dfk;

// ------------------------------------------------------------------ the backing store
static uint64_t g_next = 1ull << 32;       // next address: 4096-aligned, a page of nothing between two chunks
static int g_refuse = 0;                   // requests still to be refused
static std::vector<uint64_t> g_got;        // sizes handed out, and addresses taken back
static std::vector<void*> g_given;
static void* fake_get(uint64_t bytes, const char** why)
{
    if (g_refuse > 0) { --g_refuse; *why = "out of memory"; return nullptr; }
    void* p = (void*)g_next;
    g_next += ((bytes + 4095) & ~4095ull) + 4096;
    g_got.push_back(bytes);
    return p;
}
static void fake_give(void* p) { g_given.push_back(p); }
static void fake_reset() { g_refuse = 0; g_got.clear(); g_given.clear(); }

static FILE* g_log = nullptr;
static void logv(const char* tag, uint64_t v) { if (g_log) fprintf(g_log, "%s %llu\n", tag, (unsigned long long)v); }

static int g_bad = 0;
#define CHECK(x) do { if (!(x)) { if (++g_bad <= 5) printf("  line %d: %s\n", __LINE__, #x); } } while (0)
static int done(const char* name) { printf("%s: %s\n", name, g_bad ? "FAILED" : "ok"); const int b = g_bad; g_bad = 0; return b != 0; }

namespace dfk {
struct ArenaTest {                         // the arena's own lists
    static size_t n_chunks(const Arena& a) { return a.chunks.size(); }
    static uint64_t chunk_bytes(const Arena& a, size_t k) { return a.chunks[k].bytes; }
    static char* chunk_base(const Arena& a, size_t k) { return a.chunks[k].p; }
    static const std::vector<Arena::Free>& free_of(const Arena& a, size_t k) { return a.chunks[k].free_list; }
    // free blocks sorted, disjoint, not touching; free and owned blocks tile every chunk; the totals agree
    static bool consistent(const Arena& a)
    {
        uint64_t held = 0, reserved = 0;
        for (const auto& o : a.owned) held += o.bytes;
        for (const auto& k : a.chunks) {
            reserved += k.bytes;
            std::vector<Arena::Free> all;
            for (size_t i = 0; i < k.free_list.size(); ++i) {
                const Arena::Free& f = k.free_list[i];
                if (!f.bytes || (i && k.free_list[i - 1].off + k.free_list[i - 1].bytes >= f.off)) return false;
                all.push_back(f);
            }
            for (const auto& o : a.owned) if ((char*)o.p >= k.p && (char*)o.p < k.p + k.bytes) all.push_back(Arena::Free{(uint64_t)((char*)o.p - k.p), o.bytes});
            std::sort(all.begin(), all.end(), [](const Arena::Free& x, const Arena::Free& y) { return x.off < y.off; });
            uint64_t at = 0;
            for (const Arena::Free& f : all) { if (f.off != at) return false; at += f.bytes; }
            if (at != k.bytes) return false;
        }
        return held == a.held && reserved == a.reserved && reserved <= a.budget && a.peak >= a.held;
    }
};
}
typedef ArenaTest AT;

static bool same(const std::vector<Arena::Free>& a, const std::vector<Arena::Free>& b)
{
    if (a.size() != b.size()) return false;
    for (size_t i = 0; i < a.size(); ++i) if (a[i].off != b[i].off || a[i].bytes != b[i].bytes) return false;
    return true;
}
static uint64_t off(const Arena& a, const DevBuf& b) { return a.offset_of(b); }

constexpr uint64_t MiB = 1ull << 20;

// one chunk of 64 MiB with three holes of 1, 3 and 2 MiB (by rising offset) between blocks that stay
struct Holes {
    Arena a{fake_get, fake_give};
    DevBuf fill[4], hole[3];
    Holes()
    {
        fake_reset();
        a.budget = 64 * MiB;
        const uint64_t hs[3] = {1 * MiB, 3 * MiB, 2 * MiB};
        for (int i = 0; i < 3; ++i) { a.alloc(fill[i], 4 * MiB, "fill", Place::Low); a.alloc(hole[i], hs[i], "hole", Place::Low); }
        a.alloc(fill[3], 64 * MiB - 18 * MiB, "fill", Place::Low);       // the rest of the chunk
        for (int i = 0; i < 3; ++i) a.release(hole[i]);
    }
};

static int test_placement()
{
    Holes h; Arena& a = h.a;
    CHECK(AT::n_chunks(a) == 1 && AT::chunk_bytes(a, 0) == 64 * MiB && AT::free_of(a, 0).size() == 3);
    DevBuf lo, hi, z, odd;
    CHECK(a.alloc(lo, 2 * MiB, "low", Place::Low) == 0 && off(a, lo) == 9 * MiB);              // the 1-MiB hole at 4 MiB does not fit: the lower end of the 3-MiB one
    CHECK(a.alloc(hi, 1 * MiB, "high", Place::High) == 0 && off(a, hi) == 17 * MiB);           // the upper end of the highest hole, [16, 18) MiB
    CHECK(a.alloc(z, 0, "nothing") == 0 && z.bytes == 256 && off(a, z) == 17 * MiB - 256);
    CHECK(a.alloc(odd, 257, "odd", Place::Low) == 0 && odd.bytes == 512 && off(a, odd) == 4 * MiB);
    CHECK(!lo.sub && !hi.sub && a.held == 58 * MiB + 3 * MiB + 768 && a.peak == 64 * MiB);
    CHECK(AT::consistent(a));
    return done("placement");
}

static int test_coalescing()
{
    const int order[6][3] = {{0, 1, 2}, {0, 2, 1}, {1, 0, 2}, {1, 2, 0}, {2, 0, 1}, {2, 1, 0}};
    for (const int* o : order) {
        fake_reset();
        Arena a(fake_get, fake_give); a.budget = 64 * MiB;
        DevBuf edge[2], b[3];
        a.alloc(edge[0], 1 * MiB, "edge", Place::Low);
        for (int i = 0; i < 3; ++i) a.alloc(b[i], (i + 1) * MiB, "neighbour", Place::Low);
        a.alloc(edge[1], 64 * MiB - 7 * MiB, "edge", Place::Low);
        CHECK(AT::free_of(a, 0).empty());
        for (int i = 0; i < 3; ++i) { a.release(b[o[i]]); CHECK(AT::consistent(a) && !b[o[i]].p); }
        CHECK(same(AT::free_of(a, 0), {{1 * MiB, 6 * MiB}}) && a.held == 58 * MiB);
    }
    return done("coalescing");
}

static int test_shrink()
{
    fake_reset();
    Arena a(fake_get, fake_give); a.budget = 64 * MiB;
    DevBuf base, part;
    a.alloc(base, 1 * MiB, "base", Place::Low);
    const uint64_t mark = a.alloc_seq;
    const std::vector<Arena::Free> at_mark = AT::free_of(a, 0);
    a.alloc(part, 8 * MiB, "part", Place::Low);
    a.shrink(part, 8 * MiB); a.shrink(part, 9 * MiB);                                         // at or above its size: nothing happens
    CHECK(part.bytes == 8 * MiB && a.held == 9 * MiB && same(AT::free_of(a, 0), {{9 * MiB, 55 * MiB}}));
    a.shrink(part, 3 * MiB - 100);                                                            // (rounded up to 256)
    CHECK(part.bytes == 3 * MiB && off(a, part) == 1 * MiB && a.held == 4 * MiB);
    CHECK(same(AT::free_of(a, 0), {{4 * MiB, 60 * MiB}}) && AT::consistent(a));                // the tail joined the room above it
    a.release_since(mark);                                                                    // the kept head goes too
    CHECK(a.held == 1 * MiB && same(AT::free_of(a, 0), at_mark) && AT::consistent(a));
    return done("shrink");
}

static int test_release_since()
{
    for (int with_keep = 0; with_keep < 2; ++with_keep) {
        Holes h; Arena& a = h.a;
        const uint64_t mark = a.alloc_seq, held = a.held;
        const std::vector<Arena::Free> at_mark = AT::free_of(a, 0);
        DevBuf b[5];
        a.alloc(b[0], MiB / 2, "a", Place::Low); a.alloc(b[1], MiB, "b", Place::High); a.alloc(b[2], 2 * MiB, "c", Place::Low);
        a.alloc(b[3], MiB / 4, "d", Place::High); a.alloc(b[4], 256, "e", Place::Low);
        a.release(b[0]);
        a.shrink(b[2], MiB);
        CHECK(AT::consistent(a));
        if (!with_keep) {
            a.release_since(mark);
            CHECK(same(AT::free_of(a, 0), at_mark) && a.held == held);
        } else {
            a.release_since(mark, &b[3]);
            a.release_since(mark, &b[3]);                                                     // (again: nothing left but the kept block)
            CHECK(a.held == held + MiB / 4 && !same(AT::free_of(a, 0), at_mark));
            a.release(b[3]);
            CHECK(same(AT::free_of(a, 0), at_mark) && a.held == held);
        }
        CHECK(AT::consistent(a));
    }
    return done("release_since");
}

static int test_pass_block()
{
    fake_reset();
    Arena a(fake_get, fake_give); a.budget = 64 * MiB;
    Arena::PassBlock blk;
    DevBuf t[3], low, big;
    CHECK(a.alloc(blk.block, 4 * MiB, "pass block") == 0 && off(a, blk.block) == 60 * MiB);
    const uint64_t seq = a.alloc_seq, held = a.held;
    {
        Arena::Current in_blk(a, blk);
        CHECK(a.alloc(t[0], 1 * MiB, "t0") == 0 && t[0].sub && t[0].p == blk.block.p);
        CHECK(a.alloc(t[1], 2 * MiB + 1, "t1") == 0 && t[1].sub && t[1].p == (char*)blk.block.p + 1 * MiB && t[1].bytes == 2 * MiB + 256);
        CHECK(a.alloc(low, 1 * MiB, "low", Place::Low) == 0 && !low.sub && off(a, low) == 0);  // never from the block
        CHECK(a.alloc(big, 1 * MiB, "does not fit") == 0 && !big.sub && off(a, big) == 59 * MiB);   // the open arena, journalled
        CHECK(a.alloc_seq == seq + 2 && a.held == held + 2 * MiB);
        CHECK(a.alloc(t[2], MiB / 2, "t2") == 0 && t[2].sub && blk.used == 3 * MiB + 256 + MiB / 2);   // what still fits is still bumped
        const std::vector<Arena::Free> before = AT::free_of(a, 0);
        a.release(t[0]);
        CHECK(!t[0].p && same(AT::free_of(a, 0), before) && a.held == held + 2 * MiB && blk.used == 3 * MiB + 256 + MiB / 2);
    }
    DevBuf after;
    CHECK(a.alloc(after, 256, "no block current") == 0 && !after.sub);
    a.release(after); a.release(big); a.release(low);
    a.release(blk.block);
    CHECK(a.held == 0 && same(AT::free_of(a, 0), {{0, 64 * MiB}}) && AT::consistent(a));
    return done("pass block");
}

static int test_budget_and_growth()
{
    fake_reset();
    {   // past the budget: an error, nothing changes
        Arena a(fake_get, fake_give); a.budget = 256 * MiB;
        DevBuf b, c;
        CHECK(a.alloc(b, 100 * MiB, "b") == 0);
        const uint64_t seq = a.alloc_seq;
        CHECK(a.alloc(c, 156 * MiB + 1, "c") == Arena::E_BUDGET && !c.p && a.held == 100 * MiB && a.alloc_seq == seq && a.reserved == 200 * MiB);
        CHECK(a.err.find("HBM budget exceeded allocating") == 0 && a.err.find("for c (held 104857600, budget 268435456)") != std::string::npos);
        CHECK(g_got.size() == 1 && AT::consistent(a));
    }
    {   // the first chunk: max(2 x request, 64 MiB, min(hint, budget)), cut to the budget and to 4 KiB; later ones twice the request
        const uint64_t hint[4] = {0, 0, 300 * MiB, 5000 * MiB}, req[4] = {1 * MiB, 40 * MiB, 40 * MiB, 40 * MiB};
        const uint64_t budget = 1000 * MiB + 4097, expect[4] = {64 * MiB, 80 * MiB, 300 * MiB, 1000 * MiB + 4096};
        for (int i = 0; i < 4; ++i) {
            fake_reset();
            Arena a(fake_get, fake_give); a.budget = budget; a.first_chunk_hint = hint[i];
            DevBuf b, c;
            CHECK(a.alloc(b, req[i], "first") == 0 && g_got.size() == 1 && g_got[0] == expect[i] && a.reserved == expect[i]);
            if (i == 2) {
                CHECK(a.alloc(c, 280 * MiB, "second") == 0 && g_got.size() == 2 && g_got[1] == 560 * MiB && AT::n_chunks(a) == 2);
                CHECK(a.largest_allocatable() == 280 * MiB);                                  // a free block; a new chunk could be 140 MiB + 4096
                a.release(c);
                CHECK(a.largest_allocatable() == 560 * MiB && AT::consistent(a));
            }
        }
    }
    {   // the backing refuses the larger size: the exact size is tried once
        fake_reset();
        Arena a(fake_get, fake_give); a.budget = 1000 * MiB;
        DevBuf b, c;
        g_refuse = 1;
        CHECK(a.alloc(b, 10 * MiB + 100, "b") == 0 && g_got.size() == 1 && g_got[0] == 10 * MiB + 256 && AT::free_of(a, 0).empty());
        g_refuse = 2;
        const uint64_t seq = a.alloc_seq;
        CHECK(a.alloc(c, 20 * MiB, "c") == Arena::E_BACKING && g_refuse == 0 && !c.p && a.alloc_seq == seq && a.held == 10 * MiB + 256 && AT::n_chunks(a) == 1);
        CHECK(a.err == "hipMalloc(20971520) for c: out of memory");
        CHECK(AT::consistent(a));
    }
    {   // empty chunks are dropped before the budget is declared exhausted; room in pieces that are each too small is fragmentation
        fake_reset();
        Arena a(fake_get, fake_give); a.budget = 256 * MiB;
        DevBuf b[4], c;
        for (int i = 0; i < 4; ++i) CHECK(a.alloc(b[i], 32 * MiB, "quarter") == 0);         // two chunks of 64 MiB
        CHECK(AT::n_chunks(a) == 2 && a.reserved == 128 * MiB);
        a.release(b[0]); a.release(b[1]);                                                     // the first chunk is empty
        void* first = AT::chunk_base(a, 0);
        CHECK(a.alloc(c, 100 * MiB, "c") == 0 && g_given.size() == 1 && g_given[0] == first && g_got.back() == 192 * MiB && a.reserved == 256 * MiB);
        a.release(c);
        a.release(b[2]);                                                                      // free: 32 MiB beside b[3], 192 MiB; held 32 MiB
        DevBuf d[2], e;
        CHECK(a.alloc(d[0], 64 * MiB, "d0", Place::Low) == 0 && a.alloc(d[1], 64 * MiB, "d1", Place::High) == 0);   // 192 MiB -> [64 held][64 free][64 held]
        const uint64_t seq = a.alloc_seq, held = a.held;
        CHECK(held == 160 * MiB && a.largest_allocatable() == 64 * MiB);
        CHECK(a.alloc(e, 80 * MiB, "e") == Arena::E_FRAGMENTED && !e.p && a.held == held && a.alloc_seq == seq && AT::n_chunks(a) == 2);
        CHECK(a.err == "HBM budget exhausted by fragmentation allocating 83886080 bytes for e");
        CHECK(AT::consistent(a));
        a.drop_pool();
        CHECK(AT::n_chunks(a) == 0 && a.reserved == 0 && g_given.size() == 3);
    }
    return done("budget and growth");
}

static int test_adopted()
{
    fake_reset();
    Arena a(fake_get, fake_give); a.budget = 1000 * MiB;
    DevBuf b, c, d;
    CHECK(a.alloc(b, 60 * MiB, "b", Place::Low) == 0 && a.reserved == 120 * MiB);
    const char* why;
    void* kept = fake_get(100 * MiB, &why);
    a.adopt(kept, 100 * MiB);
    CHECK(AT::n_chunks(a) == 2 && a.reserved == 220 * MiB && a.free_blocks() == nullptr && AT::consistent(a));
    CHECK(a.alloc(c, 90 * MiB, "c", Place::Low) == 0 && c.p == kept && g_got.size() == 2);     // served from the adopted chunk
    CHECK(a.alloc(d, 10 * MiB, "d") == 0 && AT::consistent(a));
    a.reset();                                                                                // as release_all: the adopted chunk leaves, the other is one free block
    CHECK(g_given.size() == 1 && g_given[0] == kept && AT::n_chunks(a) == 1 && a.reserved == 120 * MiB && a.held == 0);
    CHECK(a.free_blocks() && same(*a.free_blocks(), {{0, 120 * MiB}}) && AT::consistent(a));
    return done("adopted chunks");
}

// ------------------------------------------------------------------ 10^5 mixed operations
static int test_random()
{
    fake_reset();
    std::mt19937_64 rng(20240607);
    Arena a(fake_get, fake_give); a.budget = 384 * MiB; a.first_chunk_hint = 128 * MiB;
    struct Live { DevBuf b; uint64_t seq; };
    std::vector<Live> live;
    std::vector<uint64_t> marks;
    Arena::PassBlock blk; Arena::Current* cur = nullptr; std::vector<DevBuf> bumped;
    uint64_t n_err[4] = {0, 0, 0, 0}, n_sub = 0;
    auto pick = [&](uint64_t n) { return (size_t)(rng() % n); };
    for (int op = 0; op < 100000; ++op) {
        const unsigned what = (unsigned)(rng() % 100);
        if (what < 50 || live.empty()) {                                                      // allocate
            const unsigned r = (unsigned)(rng() % 16);
            const uint64_t bytes = r == 0 ? 0 : r < 10 ? rng() % (256 * 1024) : r < 15 ? rng() % (24 * MiB) : rng() % (160 * MiB);
            if (rng() % 3 == 0) g_refuse = 1 + (int)(rng() % 2);
            DevBuf b;
            const int rc = a.alloc(b, bytes, "block", rng() % 3 ? Place::High : Place::Low);
            g_refuse = 0;
            logv("alloc", (uint64_t)rc); logv("at", (uint64_t)b.p);
            ++n_err[rc];
            if (rc) { CHECK(!b.p && !a.err.empty()); if (g_log) fprintf(g_log, "%s\n", a.err.c_str()); }
            else if (b.sub) { bumped.push_back(b); ++n_sub; }
            else live.push_back(Live{b, a.alloc_seq});
        } else if (what < 68) {                                                               // release
            const size_t i = pick(live.size());
            a.release(live[i].b); live.erase(live.begin() + i);
        } else if (what < 78) {                                                               // shrink
            Live& l = live[pick(live.size())];
            a.shrink(l.b, rng() % (l.b.bytes + l.b.bytes / 4 + 1));
            logv("shrunk", l.b.bytes);
        } else if (what < 82) marks.push_back(a.alloc_seq);
        else if (what < 84 && !marks.empty()) {                                               // undo back to a mark, at times but for one block
            const uint64_t mark = marks[pick(marks.size())];
            const DevBuf* keep = rng() % 2 ? &live[pick(live.size())].b : nullptr;
            if (cur && blk.block.p != (keep ? keep->p : nullptr) && a.alloc_seq > mark) {      // (the block goes with the rest)
                bool gone = false;
                for (const Live& l : live) if (l.b.p == blk.block.p) gone = l.seq > mark;
                if (gone) { delete cur; cur = nullptr; bumped.clear(); blk = Arena::PassBlock{}; }
            }
            a.release_since(mark, keep);
            for (size_t i = live.size(); i-- > 0;) if (live[i].seq > mark && !(keep && live[i].b.p == keep->p)) live.erase(live.begin() + i);
            while (!marks.empty() && marks.back() > mark) marks.pop_back();
        } else if (what < 92) {                                                               // a pass block comes or goes
            if (!cur) {
                blk = Arena::PassBlock{};
                if (a.alloc(blk.block, 1 * MiB + rng() % (32 * MiB), "pass block") == 0) { live.push_back(Live{blk.block, a.alloc_seq}); cur = new Arena::Current(a, blk); }
                logv("block", (uint64_t)blk.block.p);
            } else {
                delete cur; cur = nullptr;
                for (DevBuf& b : bumped) a.release(b);                                        // (changes nothing)
                bumped.clear();
                for (size_t i = 0; i < live.size(); ++i) if (live[i].b.p == blk.block.p) { a.release(live[i].b); live.erase(live.begin() + i); break; }
            }
        } else if (what < 93) {                                                               // memory of the caller's joins
            const char* why; const uint64_t bytes = (64 + rng() % 64) * MiB;
            if (a.reserved + bytes <= a.budget) a.adopt(fake_get(bytes, &why), bytes);
        } else if (what < 94) a.drop_empty_chunks();
        else if (what == 99 && rng() % 8 == 0) {                                              // a new run
            delete cur; cur = nullptr; bumped.clear();
            a.reset(); live.clear(); marks.clear();
        }
        logv("held", a.held); logv("reserved", a.reserved); logv("largest", a.largest_allocatable());
        if (!AT::consistent(a)) { CHECK(!"consistent after every operation"); printf("  (operation %d)\n", op); break; }
        uint64_t sum = 0; for (const Live& l : live) sum += l.b.bytes;
        if (sum != a.held) { CHECK(!"held is what the live blocks hold"); printf("  (operation %d)\n", op); break; }
    }
    delete cur;
    printf("  %llu allocations, %llu of them bumped from a pass block; refused: %llu budget, %llu fragmentation, %llu backing\n", (unsigned long long)n_err[0],
           (unsigned long long)n_sub, (unsigned long long)n_err[1], (unsigned long long)n_err[2], (unsigned long long)n_err[3]);
    CHECK(n_err[0] > 20000 && n_err[Arena::E_BUDGET] > 10 && n_err[Arena::E_FRAGMENTED] > 10 && n_err[Arena::E_BACKING] > 10 && n_sub > 1000);   // every path was taken
    return done("10^5 mixed operations");
}

// ------------------------------------------------------------------ one step of the default benchmark
// DESIGN.md section 5 (configs[1]): N reads, I k-mer instances, R records, S solid k-mers; an arena of 180 GB.  The
// calls are the ones run_typed makes, in its order, without the small scratch buffers of the stages.
static int test_replay()
{
    const uint64_t N = 1800000000ull, I = 88200000000ull, R = 6900000000ull, S = 3100000000ull;
    // The parent of the commit that moved the arena into the header (4cc07e0) planned these ranges for this step: its
    // arena and planner, lifted out of dfk.hip as they stood, were driven by this file.
    static const uint32_t expect[] = {13421772, 14763949, 16240343, 17864377, 19281192, 16132624, 12862872, 11536319, 9183345, 2930935};
    fake_reset();
    Arena a(fake_get, fake_give); a.budget = 180000000000ull; a.first_chunk_hint = a.budget;
    uint32_t log2_nb = 0; while ((1ull << log2_nb) < I / 850 + 1) ++log2_nb;                   // pick_log2_nb
    const uint32_t sub_nb = 1u << log2_nb, min_freq = 3, grid = 512; const uint64_t out_chunk = 4096;
    CHECK(log2_nb == 27);
    int rc = 0;
    DevBuf good_len, acc, summ, classes, d_hist, d_g, d_snap;
    rc |= a.alloc(good_len, 4 * N, "goodLens", Place::Low);
    rc |= a.alloc(acc, 8ull * sub_nb, "bucket counters", Place::Low);
    rc |= a.alloc(summ, 16 * N, "run summaries", Place::Low);
    rc |= a.alloc(classes, 4 * N, "read bucket classes", Place::Low);
    rc |= a.alloc(d_hist, 8ull << 24, "spectrum bins", Place::Low);
    rc |= a.alloc(d_g, 256, "count globals", Place::Low);
    rc |= a.alloc(d_snap, (8ull << 24) + 256, "spectrum snapshot", Place::Low);
    CHECK(rc == 0 && AT::n_chunks(a) == 1);

    struct Job { Arena::PassBlock blk; uint32_t lo = 0, n = 0; bool valid = false; };
    uint64_t inst_seen = 0, solid_seen = 0;
    std::vector<uint32_t> ranges; std::vector<DevBuf> parts;
    size_t max_pieces = 0;
    auto pieces = [&] { if (!parts.empty()) max_pieces = std::max(max_pieces, a.free_blocks()->size()); };
    auto plan = [&](uint32_t lo, const RunningPass* running) {
        const PlanInputs in{(double)(a.budget - a.held), sub_nb, lo, I, R, inst_seen, solid_seen, min_freq, 0, 0.95, true, 10.0, 1.1, false};
        const uint32_t n = plan_range(in, a.free_blocks(), running);
        logv("range", n);
        return n;
    };
    auto start = [&](Job& j, uint32_t lo, uint32_t n) {                                      // the block, and what the scatter bumps out of it
        j = Job{}; j.lo = lo; j.n = n;
        rc |= a.alloc(j.blk.block, pass_block_bytes(n, sub_nb, R), "pass block");
        logv("at", off(a, j.blk.block)); pieces();
        Arena::Current in_blk(a, j.blk);
        DevBuf tables, records;
        rc |= a.alloc(tables, 80ull * n, "bucket tables");
        rc |= a.alloc(records, (uint64_t)((double)n / sub_nb * (double)R) * 32, "super-k-mer records");
        CHECK(!rc && tables.sub && records.sub);
        j.valid = !rc; ranges.push_back(n);
    };
    Job cur, nxt;
    start(cur, 0, plan(0, nullptr));
    while (cur.valid && ranges.size() < 1000) {
        const uint32_t n = cur.n, nlo = cur.lo + n;
        const double share = (double)n / sub_nb;
        const uint64_t p_inst = (uint64_t)(share * (double)I);
        DevBuf d_wg, part;
        {   // count_prepare: the part's reservation
            Arena::Current in_blk(a, cur.blk);
            uint64_t res = part_entries(p_inst, min_freq, inst_seen, solid_seen) + grid * out_chunk;
            const uint64_t room = a.budget - a.held;
            if (res * 32 > room) res = room / 32;
            rc |= a.alloc(d_wg, 24 * grid, "workgroup output state");
            rc |= a.alloc(part, res * 32, "solid k-mer entries", Place::Low);
            logv("at", off(a, part)); pieces();
        }
        nxt.valid = false;
        if (nlo < sub_nb) {
            const RunningPass rp{cur.blk.block.bytes, p_inst, n, off(a, cur.blk.block)};
            const uint32_t n2 = plan(nlo, &rp);
            if (n2) start(nxt, nlo, n2);
        }
        const uint64_t solid = (uint64_t)(share * (double)S);                                 // count_run: cut to size
        CHECK(solid * 32 <= part.bytes);
        a.shrink(part, solid * 32); pieces();
        parts.push_back(part);
        solid_seen += solid; inst_seen += p_inst;
        a.release(cur.blk.block); pieces();
        if (nxt.valid) { cur = nxt; nxt = Job{}; }
        else { cur = Job{}; if (nlo < sub_nb) start(cur, nlo, plan(nlo, nullptr)); }
        CHECK(!rc && AT::consistent(a));
        if (rc) { printf("  %s\n", a.err.c_str()); break; }
    }
    uint64_t covered = 0; for (uint32_t n : ranges) covered += n;
    CHECK(rc == 0 && covered == sub_nb && !cur.valid);                                        // every bucket once: the ranges are laid end to end
    CHECK(max_pieces <= 2);                                                                   // the free room stays in one or two pieces
    CHECK(AT::n_chunks(a) == 1 && g_got.size() == 1 && a.peak <= a.budget);
    const size_t n_expect = sizeof expect / sizeof expect[0];
    CHECK(ranges.size() == n_expect);
    for (size_t i = 0; i < ranges.size() && i < n_expect; ++i) CHECK(ranges[i] == expect[i]);
    printf("  replayed step: %zu ranges, peak %.1f GB, free room in at most %zu pieces after the first pass\n", ranges.size(), a.peak / 1e9, max_pieces);
    return done("replayed benchmark step");
}

int main(int argc, char** argv)
{
    if (argc > 1) g_log = fopen(argv[1], "w");
    int fails = 0;
    fails += test_placement();
    fails += test_coalescing();
    fails += test_shrink();
    fails += test_release_since();
    fails += test_pass_block();
    fails += test_budget_and_growth();
    fails += test_adopted();
    fails += test_random();
    fails += test_replay();
    if (g_log) fclose(g_log);
    return fails ? 1 : 0;
}
