// tests/cpp/test_fallback.cc -- the hot-bucket fallback's decisions (superplus_amd/csrc/dfk_fallback.h) on a CPU: tables
// of what the count stage computed for fixed inputs before the decisions moved into the header (fallback_expected.h),
// and the properties every plan must have, over seeded random cases.  One "name: ok" line per case, exit status 1 if
// any failed.
//   g++ -O1 -std=c++17 -Wall -o test_fallback tests/cpp/test_fallback.cc && ./test_fallback
#include "../../superplus_amd/csrc/dfk_fallback.h"
#include "fallback_expected.h"
#include <cstdio>
#include <random>

using namespace dfk;

static int g_bad = 0;
#define CHECK(x) do { if (!(x)) { if (++g_bad <= 5) printf("  line %d: %s\n", __LINE__, #x); } } while (0)
static int done(const char* name) { printf("%s: %s\n", name, g_bad ? "FAILED" : "ok"); const int b = g_bad; g_bad = 0; return b != 0; }
template <class T, size_t N> constexpr size_t len(const T (&)[N]) { return N; }

static FallbackSwitches switches(int w) { FallbackSwitches s; s.split_from_log2 = X_SWITCH[w][0]; s.max_subpass_log2 = X_SWITCH[w][1]; return s; }
static std::vector<ItemRange> ranges_of(const uint32_t* v, size_t n) { std::vector<ItemRange> r; for (size_t i = 0; i + 1 < n; i += 2) r.push_back({v[i], v[i + 1]}); return r; }
static bool same(const std::vector<ItemRange>& a, const uint32_t* v, size_t n)
{
    if (2 * a.size() != n) return false;
    for (size_t i = 0; i < a.size(); ++i) if (a[i].b0 != v[2 * i] || a[i].b1 != v[2 * i + 1]) return false;
    return true;
}
static std::vector<ItemRange> buckets(size_t n, uint32_t first = 0) { std::vector<ItemRange> r; for (uint32_t i = 0; i < n; ++i) r.push_back({first + i, first + i + 1}); return r; }

// ------------------------------------------------------------------ tables
static int test_route_tables()
{
    const size_t n = len(X_INST);
    const std::vector<uint64_t> inst(X_INST, X_INST + n);
    const std::vector<ItemRange> singles = buckets(n);
    CHECK(len(X_ROUTE) == 4 * 3 * n && len(X_ROUTE_UNSPLIT) == 4 * 3 * n);
    CHECK(FallbackSwitches().split_from_log2 == X_SWITCH[0][0] && FallbackSwitches().max_subpass_log2 == X_SWITCH[0][1]);
    for (int s = 0; s < 4; ++s) {
        const double dpi = route_distinct_per_inst(X_SEEN[s]);
        CHECK(dpi == X_ROUTE_DPI[s]);
        CHECK(table_distinct_per_inst(X_SEEN[s]) == X_TABLE_DPI[s]);
        for (int w = 0; w < 3; ++w) {
            const FallbackSwitches sw = switches(w);
            const uint16_t* want = X_ROUTE + (s * 3 + w) * n;
            const uint16_t* unsplit = X_ROUTE_UNSPLIT + (s * 3 + w) * n;
            // the split first, the other two routes for what it leaves -- as count_run goes about it
            const SplitCandidates sp = split_candidates(inst, dpi, sw);
            std::vector<uint8_t> taken(n, 0);
            for (size_t i = 0; i < sp.at.size(); ++i) {
                CHECK(sp.at[i] < n && want[sp.at[i]] == 100 + sp.log2p[i]);
                CHECK(i == 0 || sp.at[i] > sp.at[i - 1]);
                taken[sp.at[i]] = 1;
            }
            const SubpassPlan pl = plan_subpasses(singles, inst, taken, dpi, X_LOG2S, sw);
            size_t at = 0, hu = 0;
            for (size_t i = 0; i < n; ++i) {
                if (taken[i]) continue;
                CHECK(want[i] == unsplit[i]);
                if (want[i] == 300) { CHECK(hu < pl.huge.size() && pl.huge[hu].b0 == i); ++hu; continue; }
                const uint32_t p = want[i] - 200u;
                CHECK(want[i] > 200 && want[i] < 300);
                for (uint32_t k = 0; k < (1u << p); ++k, ++at)
                    CHECK(at < pl.items.size() && pl.items[at].b0 == i && pl.items[at].b1 == i + 1 && pl.words[at] == ((p << 8) | k));
            }
            CHECK(at == pl.items.size() && at == pl.words.size() && hu == pl.huge.size());
            // and every bucket when no split finds room
            const SubpassPlan all = plan_subpasses(singles, inst, std::vector<uint8_t>(n, 0), dpi, X_LOG2S, sw);
            std::vector<uint32_t> code(n, 0);
            for (const ItemRange& r : all.huge) code[r.b0] = 300;
            for (size_t j = 0; j < all.items.size(); ++j) code[all.items[j].b0] = 200 + (all.words[j] >> 8);
            for (size_t i = 0; i < n; ++i) CHECK(unsplit[i] == code[i]);
        }
    }
    return done("routes of single buckets against the recorded tables");
}

static int test_plan_tables()
{
    const size_t n = len(X_PLAN_INST);
    const SubpassPlan pl = plan_subpasses(buckets(n, 10), std::vector<uint64_t>(X_PLAN_INST, X_PLAN_INST + n), std::vector<uint8_t>(n, 0),
                                          route_distinct_per_inst(1.0), X_LOG2S, FallbackSwitches());
    CHECK(pl.items.size() == len(X_PLAN_BUCKET) && pl.words.size() == len(X_PLAN_WORD) && pl.huge.size() == len(X_PLAN_HUGE));
    for (size_t i = 0; i < pl.items.size() && i < len(X_PLAN_BUCKET); ++i)
        CHECK(pl.items[i].b0 == X_PLAN_BUCKET[i] && pl.items[i].b1 == X_PLAN_BUCKET[i] + 1 && pl.words[i] == X_PLAN_WORD[i]);
    for (size_t i = 0; i < pl.huge.size() && i < len(X_PLAN_HUGE); ++i) CHECK(pl.huge[i].b0 == X_PLAN_HUGE[i]);

    SubpassPlan next; ItemRange bad{};
    next.huge = pl.huge;
    CHECK(refine_subpasses(ranges_of(X_AGAIN, len(X_AGAIN)), &next, &bad));
    CHECK(next.items.size() == len(X_REFINED_BUCKET) && next.words.size() == len(X_REFINED_WORD) && next.huge.size() == pl.huge.size());
    for (size_t i = 0; i < next.items.size() && i < len(X_REFINED_BUCKET); ++i)
        CHECK(next.items[i].b0 == X_REFINED_BUCKET[i] && next.items[i].b1 == X_REFINED_BUCKET[i] + 1 && next.words[i] == X_REFINED_WORD[i]);
    // no marker bit; all selector bits in use
    CHECK(!refine_subpasses({{5, (3u << 8) | 1}}, &next, &bad) && bad.b0 == 5 && bad.b1 == ((3u << 8) | 1));
    CHECK(!refine_subpasses({{4, 0x80000000u | (1u << 8)}, {6, 0x80000000u | (MAX_SELECTOR_BITS << 8) | 200}}, &next, &bad) && bad.b0 == 6);
    CHECK(refine_subpasses({{6, 0x80000000u | ((MAX_SELECTOR_BITS - 1) << 8) | 100}}, &next, &bad) && next.words.size() == 2);

    std::vector<ItemRange> singles;
    const std::vector<ItemRange> nx = halve_items(ranges_of(X_HALVE_IN, len(X_HALVE_IN)), &singles);
    CHECK(same(nx, X_HALVE_NEXT, len(X_HALVE_NEXT)) && same(singles, X_HALVE_SINGLES, len(X_HALVE_SINGLES)));

    for (size_t i = 0; i < len(X_CAN); ++i) CHECK(split_group_cap(X_CAN[i]) == X_CAP[i]);
    const std::vector<uint64_t> gi(X_GROUP_INST, X_GROUP_INST + len(X_GROUP_INST));
    std::vector<uint32_t> all_of(gi.size());
    for (uint32_t i = 0; i < all_of.size(); ++i) all_of[i] = i;
    size_t i0 = 0, g = 0;
    for (; g < len(X_GROUP_END); ++g) {
        const size_t i1 = split_group_end(gi, all_of, i0, X_CAP[4]);
        CHECK(i1 == X_GROUP_END[g]);
        if (i1 == i0) break;
        i0 = i1;
    }
    CHECK(g == len(X_GROUP_END) - 1);                       // the walk ended on the bucket that does not fit

    const std::vector<uint64_t> pre = chunk_prefixes(std::vector<uint64_t>(X_CHUNK_REC, X_CHUNK_REC + len(X_CHUNK_REC)));
    CHECK(pre.size() == len(X_CHUNK_PRE));
    for (size_t i = 0; i < pre.size() && i < len(X_CHUNK_PRE); ++i) CHECK(pre[i] == X_CHUNK_PRE[i]);
    return done("sub-pass words, refinement, halving, groups and chunk prefixes against the recorded tables");
}

static int test_table_sizes()
{
    const size_t n = len(X_BIG_INST);
    const std::vector<uint64_t> inst(X_BIG_INST, X_BIG_INST + n);
    const std::vector<ItemRange> b = buckets(n, 3);
    CHECK(len(X_BIG_LOG2S) == 2 * 4 * n && len(X_BIG_OFF) == 4 * 5 * n && len(X_BIG_WORDS) == 4 * 5);
    for (int rep = 0; rep < 2; ++rep)
        for (int s = 0; s < 4; ++s) {
            double per_inst = table_distinct_per_inst(X_SEEN[s]);
            if (rep) per_inst = table_retry_per_inst(per_inst);
            for (int cf = 0; cf < 5; ++cf) {
                const uint32_t sw = big_slot_words(X_BIG_CFG[cf][1], X_BIG_CFG[cf][2]);
                const BigTables t = size_big_tables(b, inst, per_inst, sw);
                CHECK(t.items.size() == n && t.slot_pre.size() == n + 1 && t.slot_pre[0] == 0);
                CHECK(t.certain == (X_BIG_CERTAIN[rep * 4 + s] != 0) && t.slot_pre[n] == X_BIG_SLOTS[rep * 4 + s]);
                if (!rep) CHECK(t.words == X_BIG_WORDS[s * 5 + cf]);
                for (size_t i = 0; i < n; ++i) {
                    CHECK(t.items[i].log2s == X_BIG_LOG2S[(rep * 4 + s) * n + i] && t.items[i].b0 == 3 + i && t.items[i].b1 == 4 + i && t.items[i].pad == 0);
                    if (!rep) CHECK(t.items[i].tab_off == X_BIG_OFF[(s * 5 + cf) * n + i]);
                    CHECK(t.slot_pre[i + 1] - t.slot_pre[i] == 1ull << t.items[i].log2s);
                }
            }
        }
    return done("HBM table sizes at K = 40, 48, 60 against the recorded tables");
}

static std::vector<WgOut> wg_of(const uint64_t* v, size_t n) { std::vector<WgOut> w; for (size_t i = 0; i + 1 < n; i += 2) w.push_back(WgOut{v[i], (unsigned)v[i + 1], 0}); return w; }
static bool same_moves(const std::vector<uint64_t>& a, const uint64_t* v, size_t n)   // (the recorded lists end with ~0)
{
    if (a.size() + 1 != n || v[n - 1] != ~0ull) return false;
    for (size_t i = 0; i < a.size(); ++i) if (a[i] != v[i]) return false;
    return true;
}
#define HOLE_CASE(NAME) do { \
        const HoleMoves m = plan_hole_moves(wg_of(X_HOLES_##NAME##_WG, len(X_HOLES_##NAME##_WG)), 8, X_HOLES_##NAME##_CLAIMED); \
        CHECK(m.n_lds == X_HOLES_##NAME##_NLDS && m.src.size() == m.dst.size()); \
        CHECK(same_moves(m.src, X_HOLES_##NAME##_SRC, len(X_HOLES_##NAME##_SRC)) && same_moves(m.dst, X_HOLES_##NAME##_DST, len(X_HOLES_##NAME##_DST))); \
    } while (0)
static int test_hole_tables()
{
    HOLE_CASE(NOHOLES); HOLE_CASE(UNTOUCHED); HOLE_CASE(ABOVE); HOLE_CASE(ONE); HOLE_CASE(MIXED);
    // sizes disagree: a part_cursor that lost a chunk leaves holes nothing can fill
    const HoleMoves m = plan_hole_moves({WgOut{0, 0, 0}, WgOut{8, 0, 0}}, 8, 8);
    CHECK(m.src.size() != m.dst.size());
    return done("hole moves against the recorded tables");
}

// ------------------------------------------------------------------ properties
static int test_halving_properties(std::mt19937_64& rng)
{
    for (int it = 0; it < 10000; ++it) {
        std::vector<ItemRange> cur, singles;
        uint64_t want = 0; uint32_t b = (uint32_t)(rng() % 1000), n_parents = 1 + (uint32_t)(rng() % 6);
        std::vector<uint8_t> seen;
        const uint32_t first = b;
        for (uint32_t i = 0; i < n_parents; ++i) {
            const uint32_t w = (it & 1) ? 1u + (uint32_t)(rng() % 40) : 1u << (rng() % 8);
            b += (uint32_t)(rng() % 3);
            cur.push_back({b, b + w}); want += w; b += w;
        }
        seen.assign(b - first, 0);
        int rounds = 0;
        while (!cur.empty() && rounds < 40) {
            uint64_t before = 0, after = 0;
            for (const ItemRange& r : cur) before += r.b1 - r.b0;
            const size_t s0 = singles.size();
            const std::vector<ItemRange> next = halve_items(cur, &singles);
            for (const ItemRange& r : next) { after += r.b1 - r.b0; CHECK(r.b1 > r.b0); }
            CHECK(after + (singles.size() - s0) == before);             // the children tile the parents
            // two children per parent that is wider than one bucket, adjoining, covering it
            size_t c = 0, s = s0;
            for (const ItemRange& r : cur) {
                if (r.b1 - r.b0 <= 1) { CHECK(s < singles.size() && singles[s].b0 == r.b0 && singles[s].b1 == r.b1); ++s; continue; }
                CHECK(c + 1 < next.size() && next[c].b0 == r.b0 && next[c].b1 == next[c + 1].b0 && next[c + 1].b1 == r.b1);
                c += 2;
            }
            CHECK(c == next.size() && s == singles.size());
            cur = next; ++rounds;
        }
        CHECK(cur.empty() && rounds <= 9);                              // widths up to 2^7 / 40: it ends
        CHECK(singles.size() == want);
        for (const ItemRange& r : singles) { CHECK(r.b1 == r.b0 + 1 && !seen[r.b0 - first]); seen[r.b0 - first] = 1; }
    }
    return done("halving: children tile the parents, singles are the width-1 ranges, it ends (10^4 cases)");
}

static uint64_t random_inst(std::mt19937_64& rng)
{
    const uint64_t around[] = {700, 1400, 1024, 2048, 1024ull << 8, (1ull << 22) * 700, 1ull << 32};
    switch (rng() % 3) {
    case 0: return 1 + rng() % 4000;
    case 1: return 1 + (rng() >> (20 + rng() % 43));
    default: { const uint64_t a = around[rng() % 7]; return a - 3 + rng() % 7; }
    }
}

static int test_route_properties(std::mt19937_64& rng)
{
    for (int it = 0; it < 10000; ++it) {
        const size_t n = 1 + rng() % 6;
        std::vector<uint64_t> inst(n);
        for (uint64_t& v : inst) v = random_inst(rng);
        const double seen = (it % 5 == 0) ? 0.0 : (double)(rng() % 1000 + 1) / 1000.0, dpi = route_distinct_per_inst(seen);
        FallbackSwitches sw; sw.split_from_log2 = (uint32_t)(rng() % 24); sw.max_subpass_log2 = (uint32_t)(rng() % (MAX_SELECTOR_BITS + 1));   // (the selector has no more bits)
        const uint32_t log2s = 10 + (uint32_t)(rng() % 3);
        const std::vector<ItemRange> singles = buckets(n, 50);
        const SplitCandidates sp = split_candidates(inst, dpi, sw);
        CHECK(sp.log2p.size() == sp.at.size());
        std::vector<uint8_t> taken(n, 0);
        std::vector<int> routes(n, 0);
        for (size_t i = 0; i < sp.at.size(); ++i) {
            CHECK(sp.at[i] < n && (i == 0 || sp.at[i] > sp.at[i - 1]) && sp.log2p[i] >= sw.split_from_log2 && sp.log2p[i] <= SPLIT_MAX_LOG2P && inst[sp.at[i]] < (1ull << 32));
            CHECK(distinct_guess(inst[sp.at[i]], dpi) <= SPLIT_SUB_DISTINCT << sp.log2p[i]);      // at most 700 distinct k-mers per sub-bucket, by the guess
            if (rng() % 4) { taken[sp.at[i]] = 1; ++routes[sp.at[i]]; }      // (some find no room)
        }
        const SubpassPlan pl = plan_subpasses(singles, inst, taken, dpi, log2s, sw);
        for (const ItemRange& r : pl.huge) ++routes[r.b0 - 50];
        std::vector<std::vector<uint8_t>> sel(n);
        std::vector<uint32_t> pp(n, ~0u);
        CHECK(pl.items.size() == pl.words.size());
        for (size_t i = 0; i < pl.items.size(); ++i) {
            const uint32_t b = pl.items[i].b0 - 50, p = pl.words[i] >> 8, k = pl.words[i] & 0xFFu;
            CHECK(b < n && pl.items[i].b1 == pl.items[i].b0 + 1 && p >= 1 && p <= MAX_SELECTOR_BITS && p <= sw.max_subpass_log2 && k < (1u << p));
            if (b >= n || p > 8) continue;
            if (pp[b] == ~0u) { pp[b] = p; sel[b].assign(1u << p, 0); ++routes[b]; }
            CHECK(pp[b] == p && k < sel[b].size() && !sel[b][k]);
            if (k < sel[b].size()) sel[b][k] = 1;
        }
        for (size_t b = 0; b < n; ++b) {
            CHECK(routes[b] == 1);                                            // exactly one route
            for (uint8_t s : sel[b]) CHECK(s);                                // selectors 0 .. 2^p - 1, once each
            if (pp[b] != ~0u) CHECK(inst[b] <= ((1ull << log2s) / 2) << MAX_SELECTOR_BITS);   // the refinement can end
        }
    }
    return done("routes: one per bucket, the sub-passes of a bucket enumerate its selectors once (10^4 cases)");
}

static int test_refinement_properties(std::mt19937_64& rng)
{
    for (int it = 0; it < 10000; ++it) {
        const uint32_t p = 1 + (uint32_t)(rng() % MAX_SELECTOR_BITS), k = (uint32_t)(rng() % (1u << std::min(p, 8u))), bucket = (uint32_t)rng() & 0x7FFFFFFFu;
        SubpassPlan next; ItemRange bad{};
        const bool ok = refine_subpasses({{bucket, 0x80000000u | (p << 8) | k}}, &next, &bad);
        if (p >= MAX_SELECTOR_BITS) { CHECK(!ok && bad.b0 == bucket); continue; }
        CHECK(ok && next.items.size() == 2 && next.words.size() == 2);
        if (!ok || next.words.size() != 2) continue;
        // a k-mer of selector value v (8 bits) belongs to the sub-pass (p, k) when its low p bits are k: the children's sets partition the parent's
        for (uint32_t v = 0; v < 256; ++v) {
            const bool in_parent = (v & ((1u << p) - 1)) == k;
            int in_children = 0;
            for (int c = 0; c < 2; ++c) {
                const uint32_t cp = next.words[c] >> 8, ck = next.words[c] & 0xFFu;
                CHECK(cp == p + 1 && next.items[c].b0 == bucket && next.items[c].b1 == bucket + 1);
                in_children += (v & ((1u << cp) - 1)) == ck;
            }
            CHECK(in_children == (in_parent ? 1 : 0));
        }
    }
    return done("refinement: two children that partition the parent's selectors, an error at the last selector bit (10^4 cases)");
}

static int test_group_properties(std::mt19937_64& rng)
{
    for (int it = 0; it < 10000; ++it) {
        const size_t n = 1 + rng() % 12;
        std::vector<uint64_t> inst(n);
        for (uint64_t& v : inst) v = 1 + rng() % 50000000;
        const uint64_t can = (it % 7 == 0) ? rng() % (600ull << 20) : (512ull << 20) + rng() % (8ull << 30), cap = split_group_cap(can);
        CHECK(cap * 34 <= (can > (512ull << 20) ? can - (512ull << 20) : 0));      // the records (32 B) and what goes with them fit the block
        std::vector<uint32_t> at;                                                  // the candidates: some of the buckets, in order
        for (uint32_t i = 0; i < n; ++i) if (rng() % 3) at.push_back(i);
        const size_t m = at.size();
        size_t i0 = 0;
        while (i0 < m) {
            const size_t i1 = split_group_end(inst, at, i0, cap);
            CHECK(i1 >= i0 && i1 <= m);
            uint64_t sum = 0;
            for (size_t i = i0; i < i1; ++i) sum += inst[at[i]];
            CHECK(sum <= cap);                                                     // within the cap
            CHECK(i1 == m || sum + inst[at[i1]] > cap);                            // and as many as it holds
            if (i1 == i0) { CHECK(inst[at[i0]] > cap); break; }                    // none fits: exactly when the first exceeds it
            CHECK(inst[at[i0]] <= cap);
            i0 = i1;                                                               // contiguous, in order
        }
    }
    return done("groups: contiguous, in order, each within the cap, 'none fits' when the first candidate exceeds it (10^4 cases)");
}

static int test_table_properties(std::mt19937_64& rng)
{
    for (int it = 0; it < 10000; ++it) {
        const size_t n = 1 + rng() % 8;
        std::vector<uint64_t> inst(n);
        for (uint64_t& v : inst) v = 1 + (rng() >> (24 + rng() % 39));
        double per_inst = table_distinct_per_inst((it % 5 == 0) ? 0.0 : (double)(rng() % 1000 + 1) / 1000.0);
        CHECK(per_inst >= 0.05 && per_inst <= 1.0);
        const uint32_t sw = big_slot_words(3 + (int)(rng() % 2), (int)(rng() % 8));
        CHECK(sw >= 7 && sw <= 14);
        int steps = 0;
        for (;; ++steps) {
            const BigTables t = size_big_tables(buckets(n), inst, per_inst, sw);
            uint64_t at = 0; bool certain = true;
            for (size_t i = 0; i < n; ++i) {
                const uint64_t guess = std::min<uint64_t>(inst[i], (uint64_t)((double)inst[i] * per_inst) + 256);
                CHECK(2 * guess <= 1ull << t.items[i].log2s && t.items[i].log2s >= BIG_MIN_LOG2S);   // load <= 0.5 at the guess
                CHECK(t.items[i].tab_off == at);                                                      // tables adjoin, none overlaps
                at += (uint64_t)sw << t.items[i].log2s;
                CHECK(t.slot_pre[i + 1] == t.slot_pre[i] + (1ull << t.items[i].log2s));
                certain = certain && guess == inst[i];
            }
            CHECK(t.words == at && t.certain == certain);
            if (per_inst >= 1.0) CHECK(t.certain);
            if (t.certain || steps > 8) break;
            const double next = table_retry_per_inst(per_inst);
            CHECK(next > per_inst);
            per_inst = next;
        }
        CHECK(steps <= 5);                                  // from 0.05: 0.1, 0.2, 0.4, 0.8, 1.0
    }
    return done("HBM tables: load <= 0.5 at the guess, no overlap, doubling reaches the certain bound (10^4 cases)");
}

static int test_hole_properties(std::mt19937_64& rng)
{
    for (int it = 0; it < 10000; ++it) {
        // a part as the persistent workgroups leave it: every chunk belongs to one workgroup, which filled all its chunks but
        // the last one to the end; entry values: 0 = hole, otherwise a serial number
        const uint64_t CH = 1 + rng() % 9;
        const size_t n_wg = (it % 10 == 0) ? 1 : 1 + rng() % 7, n_chunks = rng() % 20;
        const int kind = it % 4;                            // 1: no holes; 2: every workgroup without a chunk; 3: holes only at the top
        std::vector<WgOut> wg(n_wg, WgOut{~0ull, (unsigned)CH, 0});
        std::vector<uint64_t> part(n_chunks * CH, 0);
        uint64_t serial = 0, claimed = kind == 2 ? 0 : n_chunks * CH;
        if (kind != 2)
            for (size_t ch = 0; ch < n_chunks; ++ch) {
                WgOut& w = wg[kind == 3 ? std::min(ch, n_wg - 1) : rng() % n_wg];
                if (w.chunk != ~0ull) for (uint64_t i = w.used; i < CH; ++i) part[w.chunk + i] = ++serial;   // its earlier chunk was filled up before it took this one
                w.chunk = ch * CH;
                w.used = (unsigned)((kind == 1 || (kind == 3 && ch + 1 < n_chunks && ch + 1 < n_wg)) ? CH : rng() % (CH + 1));
                for (uint64_t i = 0; i < w.used; ++i) part[w.chunk + i] = ++serial;
            }
        else part.clear();
        const HoleMoves mv = plan_hole_moves(wg, CH, claimed);
        const std::vector<uint64_t>&src = mv.src, &dst = mv.dst;
        const uint64_t n_lds = mv.n_lds;
        CHECK(n_lds == serial);
        CHECK(src.size() == dst.size());
        if (kind == 1) CHECK(n_lds == claimed);
        if (kind != 0) CHECK(src.empty());
        for (size_t i = 0; i < src.size() && i < dst.size(); ++i) {
            CHECK(src[i] >= n_lds && src[i] < claimed && part[src[i]] != 0);      // nothing is moved from inside a hole
            CHECK(dst[i] < n_lds && part[dst[i]] == 0);                           // and only into one
            if (src[i] < part.size() && dst[i] < part.size()) { part[dst[i]] = part[src[i]]; part[src[i]] = 0; }
        }
        std::vector<uint8_t> got(serial + 1, 0);
        for (uint64_t i = 0; i < n_lds && i < part.size(); ++i) { CHECK(part[i] != 0 && !got[part[i]]); got[part[i]] = 1; }   // dense, each entry once
        for (uint64_t i = n_lds; i < part.size(); ++i) CHECK(part[i] == 0);
    }
    return done("hole moves: [0, n_lds) holds every entry once and no hole; nothing moves out of a hole (10^4 cases)");
}

int main()
{
    std::mt19937_64 rng(20260);
    int bad = 0;
    bad += test_route_tables();
    bad += test_plan_tables();
    bad += test_table_sizes();
    bad += test_hole_tables();
    bad += test_halving_properties(rng);
    bad += test_route_properties(rng);
    bad += test_refinement_properties(rng);
    bad += test_group_properties(rng);
    bad += test_table_properties(rng);
    bad += test_hole_properties(rng);
    return bad ? 1 : 0;
}
