// tests/cpp/test_adj_plan.cc -- the plan of the adjacency stage's boundary k-mer set (superplus_amd/csrc/dfk_adj_plan.h) on a
// CPU: the sizing function's properties over seeded random cases, the estimate and the load test on hand-made part
// tables, one step of the default benchmark replayed in the arena (the calls of tests/cpp/test_arena.cc's replay, plus the
// boundary lists behind the parts) up to the moment the last count starts, and the slot walk for slot counts that are
// no power of two.  One "name: ok" line per case, exit status 1 if any failed.
//   g++ -O1 -std=c++17 -Wall -o test_adj_plan tests/cpp/test_adj_plan.cc && ./test_adj_plan
#include "../../superplus_amd/csrc/dfk_adj_plan.h"
#include <cmath>
#include <random>

using namespace dfk;

static int g_bad = 0;
#define CHECK(x) do { if (!(x)) { if (++g_bad <= 5) printf("  line %d: %s\n", __LINE__, #x); } } while (0)
static int done(const char* name) { printf("%s: %s\n", name, g_bad ? "FAILED" : "ok"); const int b = g_bad; g_bad = 0; return b != 0; }

typedef unsigned __int128 u128;

// ------------------------------------------------------------------ the sizing function
static int test_sizing_random()
{
    std::mt19937_64 rng(20241019);
    uint64_t n_zero = 0, n_cut = 0, n_pow2 = 0, n_room = 0;
    for (int it = 0; it < 10000; ++it) {
        const uint64_t keys = (uint64_t)std::exp2((double)(rng() % 3400) / 100.0) - (rng() % 2);      // 0 .. 1.7e10, every magnitude
        std::vector<Arena::Free> blocks(rng() % 5);
        // block sizes around what the set needs, so that both answers and the cut come up
        const double need = (double)keys / 0.6 * 16.0 + 4096.0;
        for (Arena::Free& f : blocks) { f.off = rng() % (1ull << 40); f.bytes = (uint64_t)(need * std::exp2((double)(rng() % 600) / 100.0 - 3.0)) + rng() % 512; }
        const uint64_t room = rng() % 4 ? ~0ull >> 8 : (uint64_t)(need * std::exp2((double)(rng() % 400) / 100.0 - 2.0));
        size_t at = 99;
        const uint64_t slots = adj_set_slots(keys, blocks, room, &at);
        const uint64_t pow2 = adj_pow2_slots(keys);
        CHECK(pow2 >= 1024 && (pow2 & (pow2 - 1)) == 0 && pow2 >= 2 * keys + 2 && (pow2 == 1024 || pow2 / 2 < 2 * keys + 2));
        uint64_t largest = 0;
        for (const Arena::Free& f : blocks) largest = std::max(largest, f.bytes);
        // the most slots any block holds whole, the arena's rounding respected, within the room
        const uint64_t fit = (std::min(largest, room) / ADJ_ALIGN) * (ADJ_ALIGN / ADJ_SLOT_BYTES);
        const bool reaches = fit && (u128)keys * 5 <= (u128)fit * 3;                                   // load <= 0.6 in some block
        CHECK((slots == 0) == !reaches);
        if (!slots) { ++n_zero; continue; }
        CHECK(at < blocks.size() && blocks[at].bytes == largest);
        const uint64_t bytes = (slots * ADJ_SLOT_BYTES + ADJ_ALIGN - 1) & ~(ADJ_ALIGN - 1);            // what the arena will take for it
        CHECK(bytes <= blocks[at].bytes && bytes <= room);                                             // never more than the block it names
        CHECK((u128)keys * 5 <= (u128)slots * 3 && (double)keys / (double)slots <= 0.6 + 1e-12);       // never load > 0.6
        CHECK(slots <= pow2);                                                                          // never more than the power of two
        CHECK(slots == std::min(fit, pow2));                                                           // the largest that fits
        CHECK(slots >= adj_min_slots(keys) && adj_load_ok(keys, slots));
        if (slots == pow2) ++n_pow2; else { ++n_cut; CHECK(slots % (ADJ_ALIGN / ADJ_SLOT_BYTES) == 0); }
        if (room < largest) ++n_room;
    }
    printf("  %llu cases without a block, %llu at the power of two, %llu cut to a block (%llu of all bounded by the room)\n", (unsigned long long)n_zero,
           (unsigned long long)n_pow2, (unsigned long long)n_cut, (unsigned long long)n_room);
    CHECK(n_zero > 500 && n_pow2 > 500 && n_cut > 500 && n_room > 100);                               // every answer came up
    // edges: no blocks; a block one byte short of the least set; exactly the least set
    CHECK(adj_set_slots(1000, {}, ~0ull) == 0);
    const uint64_t least = ((adj_min_slots(6000000) + 15) / 16) * 16;
    CHECK(least == 10000000 && adj_set_slots(6000000, {{0, least * 16 - 1}}, ~0ull) == 0);
    CHECK(adj_set_slots(6000000, {{0, least * 16}}, ~0ull) == least);
    CHECK(adj_set_slots(6000000, {{0, 1ull << 40}}, ~0ull) == (1ull << 24));                          // plenty of room: the value before
    CHECK(adj_set_slots(6000000, {{0, 1ull << 40}}, least * 16) == least);                            // the budget's room binds
    CHECK(adj_set_slots(0, {{0, 1ull << 20}}, ~0ull) == 1024);
    return done("sizing over 10^4 random cases");
}

// ------------------------------------------------------------------ estimate and load test
static int test_estimate_and_load()
{
    auto near = [](uint64_t got, double exact) { return (double)got >= exact && (double)got <= exact + 2.0; };
    // three finished parts over 300 of 1000 buckets, one of them without boundary entries
    CHECK(near(adj_estimate_keys({100, 0, 50}, 1000, 300), 150.0 * 1000 / 300 * 1.05));
    CHECK(near(adj_estimate_keys({0, 0, 7}, 1u << 27, 1u << 20), 7.0 * 128 * 1.05));
    // only one finished part
    CHECK(near(adj_estimate_keys({80}, 64, 8), 80.0 * 8 * 1.05));
    CHECK(near(adj_estimate_keys({43000000}, 134217728, 13421772), 43e6 * (134217728.0 / 13421772.0) * 1.05));
    // nothing to go by: no parts, no entries, no buckets done
    CHECK(adj_estimate_keys({}, 1000, 300) == 0 && adj_estimate_keys({0, 0}, 1000, 300) == 0 && adj_estimate_keys({5}, 1000, 0) == 0);
    // the scale (a test's way to a guess that is too low)
    CHECK(near(adj_estimate_keys({100, 0, 50}, 1000, 300, 0.01), 1.5 * 1000 / 300 * 1.05));
    // all buckets but the last range done: the margin alone
    CHECK(near(adj_estimate_keys({1000000, 1000000}, 1000, 999), 2e6 * 1000 / 999 * 1.05));
    // the load test after the last pass: 0.6 is in, anything above is out
    CHECK(adj_load_ok(600, 1000) && !adj_load_ok(601, 1000) && adj_load_ok(0, 16) && !adj_load_ok(0, 0) && !adj_load_ok(1, 1) && adj_load_ok(3, 5));
    CHECK(adj_load_ok(1ull << 62, 1ull << 63) && !adj_load_ok(~0ull, ~0ull));                        // (no overflow)
    // a guess with the margin holds for a run whose last part is 1.4 times as rich as its share; one scaled to 1 % does not
    const uint64_t parts8 = 8 * 43000000ull, all = parts8 + (uint64_t)(1.4 * 43000000);
    const uint64_t slots = adj_set_slots(adj_estimate_keys(std::vector<uint64_t>(8, 43000000), 9000, 8000), {{0, 11ull << 30}}, ~0ull);
    CHECK(slots && adj_load_ok(all, slots));
    const uint64_t tiny = adj_set_slots(adj_estimate_keys(std::vector<uint64_t>(8, 43000000), 9000, 8000, 0.01), {{0, 11ull << 30}}, ~0ull);
    CHECK(tiny && !adj_load_ok(all, tiny));
    return done("estimate and load test");
}

// ------------------------------------------------------------------ one step of the default benchmark, to the last count
// The calls run_typed makes (tests/cpp/test_arena.cc, test_replay), with each part's boundary list behind its entries:
// 16 bytes of counters and 4 bytes per boundary entry, one entry in eight.
static void* fake_get(uint64_t, const char**) { static uint64_t next = 1ull << 32; void* p = (void*)next; next += 1ull << 40; return p; }
static void fake_give(void*) {}

static int test_replay(uint64_t budget, const char* name)
{
    const uint64_t N = 1800000000ull, I = 88200000000ull, R = 6900000000ull, S = 3100000000ull;
    Arena a(fake_get, fake_give); a.budget = budget; a.first_chunk_hint = a.budget;
    uint32_t log2_nb = 0; while ((1ull << log2_nb) < I / 850 + 1) ++log2_nb;
    const uint32_t sub_nb = 1u << log2_nb, min_freq = 3, grid = 512; const uint64_t out_chunk = 4096;
    int rc = 0;
    DevBuf good_len, acc, summ, classes, d_hist, d_g, d_snap;
    rc |= a.alloc(good_len, 4 * N, "goodLens", Place::Low);
    rc |= a.alloc(acc, 8ull * sub_nb, "bucket counters", Place::Low);
    rc |= a.alloc(summ, 16 * N, "run summaries", Place::Low);
    rc |= a.alloc(classes, 4 * N, "read bucket classes", Place::Low);
    rc |= a.alloc(d_hist, 8ull << 24, "spectrum bins", Place::Low);
    rc |= a.alloc(d_g, 256, "count globals", Place::Low);
    rc |= a.alloc(d_snap, (8ull << 24) + 256, "spectrum snapshot", Place::Low);
    CHECK(rc == 0);
    struct Job { Arena::PassBlock blk; uint32_t lo = 0, n = 0; bool valid = false; };
    uint64_t inst_seen = 0, solid_seen = 0;
    std::vector<uint64_t> n_blist; uint32_t n_ranges = 0;
    auto plan = [&](uint32_t lo, const RunningPass* running) {
        const PlanInputs in{(double)(a.budget - a.held), sub_nb, lo, I, R, inst_seen, solid_seen, min_freq, 0, 0.95, true, 10.0, 1.1, false};
        return plan_range(in, a.free_blocks(), running);
    };
    auto start = [&](Job& j, uint32_t lo, uint32_t n) {
        j = Job{}; j.lo = lo; j.n = n;
        rc |= a.alloc(j.blk.block, pass_block_bytes(n, sub_nb, R), "pass block");
        Arena::Current in_blk(a, j.blk);
        DevBuf tables, records;
        rc |= a.alloc(tables, 80ull * n, "bucket tables");
        rc |= a.alloc(records, (uint64_t)((double)n / sub_nb * (double)R) * 32, "super-k-mer records");
        j.valid = !rc; ++n_ranges;
    };
    uint64_t slots_at_last = 0; bool saw_last = false;
    Job cur, nxt;
    start(cur, 0, plan(0, nullptr));
    while (cur.valid && n_ranges < 1000) {
        const uint32_t n = cur.n, nlo = cur.lo + n;
        const double share = (double)n / sub_nb;
        const uint64_t p_inst = (uint64_t)(share * (double)I);
        DevBuf d_wg, part;
        {
            Arena::Current in_blk(a, cur.blk);
            uint64_t res = part_entries(p_inst, min_freq, inst_seen, solid_seen) + grid * out_chunk;
            const uint64_t room = a.budget - a.held;
            if (res * 32 > room) res = room / 32;
            rc |= a.alloc(d_wg, 24 * grid, "workgroup output state");
            rc |= a.alloc(part, res * 32, "solid k-mer entries", Place::Low);
        }
        nxt.valid = false;
        if (nlo < sub_nb) {
            const RunningPass rp{cur.blk.block.bytes, p_inst, n, a.offset_of(cur.blk.block)};
            const uint32_t n2 = plan(nlo, &rp);
            if (n2) start(nxt, nlo, n2);
        } else {
            // ---- the last count is about to start: the set's plan, from the parts that are finished
            saw_last = true;
            const uint64_t est = adj_estimate_keys(n_blist, sub_nb, cur.lo);
            const std::vector<Arena::Free> blocks = a.allocatable_blocks();
            size_t at = 0;
            const uint64_t slots = adj_set_slots(est, blocks, a.budget - a.held, &at);
            slots_at_last = slots;
            printf("  %s: %u ranges; at the last count %.2f GB held, free", name, n_ranges, a.held / 1e9);
            for (const Arena::Free& f : blocks) printf(" %.2f", f.bytes / 1e9);
            printf(" GB; estimate %llu keys, %llu slots (%.2f GB, load %.3f)\n", (unsigned long long)est, (unsigned long long)slots, slots * 16 / 1e9,
                   slots ? (double)est / (double)slots : 0.0);
            CHECK(est >= S / 8 && est <= (uint64_t)(1.06 * (double)(S / 8)) + 16);                    // the run's keys and the margin
            CHECK(slots != 0);                                                                       // it starts at the flagship size
            CHECK(blocks.size() <= 2);
            if (slots) {
                CHECK(slots * 16 <= blocks[at].bytes && adj_load_ok(S / 8, slots) && slots <= adj_pow2_slots(est));
                DevBuf set;
                CHECK(a.alloc(set, slots * 16, "boundary k-mer set") == 0 && set.bytes == slots * 16);  // the arena takes it, to the byte
                CHECK((a.allocatable_blocks().size() <= blocks.size()));                             // out of one block's end: no new piece
                a.release(set);
            }
        }
        const uint64_t solid = (uint64_t)(share * (double)S), nb = solid / 8;
        const uint64_t keep = solid * 32 + 16 + 4 * nb;
        CHECK(keep <= part.bytes);
        a.shrink(part, keep);
        n_blist.push_back(nb);
        solid_seen += solid; inst_seen += p_inst;
        a.release(cur.blk.block);
        if (nxt.valid) { cur = nxt; nxt = Job{}; }
        else { cur = Job{}; if (nlo < sub_nb) start(cur, nlo, plan(nlo, nullptr)); }
        CHECK(!rc);
        if (rc) { printf("  %s\n", a.err.c_str()); break; }
    }
    CHECK(saw_last && slots_at_last != 0 && n_ranges >= 2);
    return done(name);
}

// ------------------------------------------------------------------ the slot walk
// As the kernels do it: home = high 64 bits of hash x slots, then one slot on with wrap at `slots`.  From any home the
// walk visits every slot exactly once, and the homes of evenly spread hashes cover the slots evenly.
static int test_slot_walk()
{
    std::mt19937_64 rng(7);
    const uint64_t counts[] = {1, 2, 3, 7, 1000, 1008, 1040, 4099, 65521, 99991, (1u << 16) + 16, 1u << 12};
    for (uint64_t slots : counts) {
        for (int rep = 0; rep < 4; ++rep) {
            const uint64_t hash = rep == 0 ? 0 : rep == 1 ? ~0ull : rng();
            uint64_t s = adj_home(hash, slots);
            CHECK(s < slots);
            if (rep == 0) CHECK(s == 0);
            if (rep == 1) CHECK(s == slots - 1);
            std::vector<uint8_t> seen(slots, 0);
            uint64_t visited = 0;
            for (uint64_t step = 0; step < slots; ++step) { CHECK(s < slots); if (s >= slots) break; visited += !seen[s]; seen[s] = 1; s = adj_next(s, slots); }
            CHECK(visited == slots && s == adj_home(hash, slots));                                   // every slot once, and back at the start
        }
        // homes of hashes spread over the 64 bits: monotone in the hash, every slot the home of some hash
        std::vector<uint32_t> hits(slots, 0);
        const uint64_t n = 64 * slots;
        uint64_t last = 0;
        for (uint64_t i = 0; i < n; ++i) { const uint64_t h = (uint64_t)(((u128)i << 64) / n); const uint64_t s = adj_home(h, slots); CHECK(s >= last && s < slots); last = s; if (s < slots) ++hits[s]; }
        for (uint64_t s = 0; s < slots; ++s) CHECK(hits[s] >= 63 && hits[s] <= 65);
    }
    CHECK(adj_home(~0ull, 3ull << 40) == (3ull << 40) - 1 && adj_home(1ull << 63, 3ull << 40) == (3ull << 39));   // no overflow at sizes past 2^32
    return done("slot walk for slot counts that are no power of two");
}

int main()
{
    int fails = 0;
    fails += test_sizing_random();
    fails += test_estimate_and_load();
    fails += test_replay(180000000000ull, "replayed benchmark step at 180 GB");
    fails += test_replay(186400000000ull, "replayed benchmark step at 186.4 GB");
    fails += test_slot_walk();
    return fails ? 1 : 0;
}
