// tests/cpp/test_walks.cc -- superplus_amd/csrc/dfk_walks.h on the host: the literal per-pair transcription (reads oriented, the sorted
// triple table materialised) against the cases recorded from tests/walks_oracle.py (tests/cpp/walks_cases.txt, and fixtures written out
// in the same form), the device version's order of work (walks_plan: ranges of pairs, batches, the reads of a batch each once, decoded
// and lowered once, the table sorted by (pair, hash), the search with verification, the live list) against the literal one under
// walks_per_batch 1, 37 and 0, several entry caps, a live list forced small (the host route) and -- built with -DDFK_WALK_HASH_BITS=8
// -- under hash collisions at nearly every look-up; the shared pieces; the bound on |EE| on random sets.  Its own main; built plain
// and under -fsanitize=address,undefined by tests/test_walks_cpu.py.
//   test_walks <cases file>
//   test_walks --literal <cases file>    the literal form alone on the file's inputs (what it records as expected is not read), timed on
//                                        this one thread: a JSON line a case (tools/walks_cost.py)
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <sstream>
#include <string>
#include "dfk_walks.h"

static int g_failed = 0;
#define CHECK(x) do { if (!(x)) { printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #x); ++g_failed; } } while (0)

struct Case {
    std::string name;
    uint32_t K = 0;
    std::vector<int32_t> inv, kmers, pairs, edge_len;
    std::vector<uint32_t> read_len;
    std::vector<uint8_t> edge_packed, read_packed, pq, ee;
    std::vector<uint64_t> edge_off, read_off, pq_off, ce, read_first, reads;
    std::vector<int64_t> recs, locs;
    uint64_t walks = 0, steps = 0, live_sum = 0, live_max = 0;
};

template <class T> static std::vector<T> row(const std::string& line)
{
    std::istringstream in(line);
    std::vector<T> v;
    long long x;
    while (in >> x) v.push_back((T)x);
    return v;
}
static std::vector<uint64_t> urow(const std::string& line)
{
    std::istringstream in(line);
    std::vector<uint64_t> v;
    unsigned long long x;
    while (in >> x) v.push_back(x);
    return v;
}
static std::vector<uint8_t> hexrow(const std::string& line)
{
    std::vector<uint8_t> v;
    if (line == "-") return v;
    auto nib = [](char c) { return (uint8_t)(c <= '9' ? c - '0' : c - 'a' + 10); };
    for (size_t i = 0; i + 1 < line.size(); i += 2) v.push_back((uint8_t)(nib(line[i]) << 4 | nib(line[i + 1])));
    return v;
}
template <class T> static std::vector<uint64_t> dense(const std::vector<T>& len)
{
    std::vector<uint64_t> off(len.size() + 1, 0);
    for (size_t i = 0; i < len.size(); ++i) off[i + 1] = off[i] + ((uint64_t)len[i] + 3) / 4;
    return off;
}

static bool same(const dfk_walks::HostResult& a, const dfk_walks::HostResult& b)
{
    if (a.starts != b.starts || a.ee_starts != b.ee_starts || a.ee != b.ee || a.recs.size() != b.recs.size() || a.locs.size() != b.locs.size()) return false;
    if (!a.recs.empty() && memcmp(a.recs.data(), b.recs.data(), a.recs.size() * sizeof(dfk_walks::Rec)) != 0) return false;
    if (!a.locs.empty() && memcmp(a.locs.data(), b.locs.data(), a.locs.size() * sizeof(dfk_walks::Loc)) != 0) return false;
    return a.walks == b.walks && a.steps == b.steps && a.live_sum == b.live_sum && a.live_max == b.live_max;
}

static void run_case(const Case& c)
{
    using namespace dfk_walks;
    std::vector<uint8_t> rp(c.read_packed), pq(c.pq), ep(c.edge_packed);       // (exactly sized copies: the last read ends at the allocation's end)
    rp.shrink_to_fit(); pq.shrink_to_fit(); ep.shrink_to_fit();
    auto room = [](auto v) { if (v.empty()) v.push_back(0); return v; };
    const std::vector<uint64_t> reads = room(c.reads), ce = room(c.ce);
    const std::vector<uint32_t> read_len = room(c.read_len);
    const std::vector<int32_t> pairs = room(c.pairs);
    std::vector<uint64_t> edge_at(ce.size(), 0); std::vector<int32_t> edge_len(ce.size(), 0);
    for (size_t k = 0; k < c.ce.size(); ++k) { edge_at[k] = c.edge_off[c.ce[k]]; edge_len[k] = c.edge_len[c.ce[k]]; }
    const Input I{c.inv.size(), c.inv.data(), c.ce.size(), ce.data(), ep.data(), edge_at.data(), edge_len.data(), c.read_first.data(), reads.data(),
                  c.read_len.size(), rp.data(), c.read_off.data(), read_len.data(), pq.data(), c.pq_off.data()};
    const uint64_t n_pairs = c.pairs.size() / 2;
    HostResult r;
    const int rc = walks_literal(I, pairs.data(), n_pairs, &r);
    CHECK(rc == 0);
    if (rc) return;
    // ---- the literal transcription against the Python restatement
    bool ok = 8 * r.recs.size() == c.recs.size() && 3 * r.locs.size() == c.locs.size() && r.ee == c.ee;
    for (size_t i = 0; ok && i < r.recs.size(); ++i) {
        const Rec& x = r.recs[i]; const int64_t* w = &c.recs[8 * i];
        ok = x.status == (uint32_t)w[0] && x.entries == (uint32_t)w[1] && x.placed == (uint32_t)w[2] && x.dup_steps == (uint32_t)w[3] && x.nE == (int32_t)(uint32_t)w[4] && x.nEE == (uint32_t)w[5] &&
             x.M == (int32_t)(uint32_t)w[6] && x.trim == (int32_t)(uint32_t)w[7];
    }
    for (size_t i = 0; ok && i < r.locs.size(); ++i) ok = r.locs[i].id == c.locs[3 * i] && r.locs[i].start == (int32_t)c.locs[3 * i + 1] && r.locs[i].fw == (uint32_t)c.locs[3 * i + 2];
    if (!ok) printf("case %s: records, placed records or EE differ from the recorded ones\n", c.name.c_str());
    CHECK(ok);
    CHECK(r.walks == c.walks && r.steps == c.steps && r.live_sum == c.live_sum && r.live_max == c.live_max);
    for (size_t i = 0; i < r.recs.size(); ++i) {
        const Rec& x = r.recs[i];
        CHECK(r.starts[i + 1] - r.starts[i] == x.placed && r.ee_starts[i + 1] - r.ee_starts[i] == x.nEE && x.trim == trim_of(x.M));
        CHECK(x.status == WALKED ? x.nEE >= KW && x.nE >= (int32_t)KW : x.nEE == 0 && x.placed == 0);
        if (i % 2 && r.recs[i - 1].placed == 0) CHECK(x.status == NOT_WALKED);
    }
    // ---- the device version's order of work gives the same, whatever the batches, the ranges and the room of the live list
    for (uint64_t per : {(uint64_t)1, (uint64_t)37, (uint64_t)0})
        for (uint64_t cap : {(uint64_t)1, (uint64_t)100, (uint64_t)1 << 30}) {
            if (per == 37 && cap == 1) continue;
            HostResult s;
            CHECK(walks_plan(I, pairs.data(), n_pairs, per, 1ull << 30, cap, MAX_LIVE, &s) == 0);
            CHECK(same(r, s));
            CHECK(s.host_route == 0);
            if (cap == (1ull << 30)) CHECK(s.ranges == (n_pairs ? 1u : 0u));
            if (per == 0 && cap == (1ull << 30)) CHECK(s.batches == s.ranges);
            if (per == 1) CHECK(s.batches == n_pairs);
            if (DFK_WALK_HASH_BITS < 64 && c.steps > 100) CHECK(s.collisions > 0);
            if (DFK_WALK_HASH_BITS >= 64) CHECK(s.collisions == 0);
        }
    {   // batches sized by a small room; a live list of 8: the host route, the same bytes
        HostResult s, t;
        CHECK(walks_plan(I, pairs.data(), n_pairs, 0, 30000, 1ull << 30, MAX_LIVE, &s) == 0 && same(r, s));
        CHECK(walks_plan(I, pairs.data(), n_pairs, 0, 1ull << 30, 1ull << 30, 8, &t) == 0);
        t.steps = r.steps; t.live_sum = r.live_sum; t.live_max = r.live_max;   // (a walk given up half way counted its steps twice)
        CHECK(same(r, t));
        CHECK((t.host_route > 0) == (c.live_max > 8));
    }
    CHECK(file_size(2 * n_pairs, r.locs.size(), r.ee.size()) == 16 + 16 * (2 * n_pairs + 1) + 64 * n_pairs + 16 * r.locs.size() + ((r.ee.size() + 3) / 4 + 7) / 8 * 8);
    // streams that do not hold len values (every one ends at once) refuse the call in both forms
    if (c.walks && r.recs[0].entries) {
        const std::vector<uint8_t> none(pq.size(), 0);
        Input J = I; J.pq = none.data();
        HostResult x, y;
        CHECK(walks_literal(J, pairs.data(), n_pairs, &x) == -3 && walks_plan(J, pairs.data(), n_pairs, 0, 1ull << 30, 1ull << 30, MAX_LIVE, &y) == -3);
    }
}

static uint32_t rnd(uint64_t* s) { *s = *s * 6364136223846793005ull + 1442695040888963407ull; return (uint32_t)(*s >> 33); }

static void pieces_and_the_bound()
{
    using namespace dfk_walks;
    // the orientation
    CHECK(!entry_rc(true, 0) && entry_rc(false, 0) && entry_rc(true, 1) && !entry_rc(false, 1));
    CHECK(loc_fw(true, 0) && !loc_fw(false, 0) && !loc_fw(true, 1) && loc_fw(false, 1));
    const uint8_t packed[] = {0xE4, 0x01};                                     // 0 1 2 3 1
    CHECK(oriented_base(packed, 5, false, 0) == 0 && oriented_base(packed, 5, false, 4) == 1 && oriented_base(packed, 5, true, 0) == 2 && oriented_base(packed, 5, true, 4) == 3);
    const uint8_t q5[] = {1, 2, 3, 4, 5};
    CHECK(oriented_qual(q5, 5, false, 1) == 2 && oriented_qual(q5, 5, true, 1) == 4);
    // the lowering: runs of 19 and 20, at either end, the whole read, qualities already below 5, the largest bytes
    auto lowered = [](const std::vector<uint8_t>& b, std::vector<uint8_t> q) {
        std::vector<uint8_t> p((b.size() + 3) / 4, 0);
        for (size_t i = 0; i < b.size(); ++i) p[i >> 2] |= (uint8_t)(b[i] << (2 * (i & 3)));
        lower_read(p.data(), (uint32_t)b.size(), q.data());
        return q;
    };
    std::vector<uint8_t> b(60, 1), q(60, 40);
    b[19] = 2;                                                                  // a run of 19, then one of 40
    std::vector<uint8_t> l = lowered(b, q);
    CHECK(l[0] == 40 && l[18] == 40 && l[19] == 40 && l[20] == 5 && l[59] == 5);
    b.assign(60, 3); b[20] = 0; b[39] = 0;                                      // 20 | 0 | 18 | 0 | 20
    q.assign(60, 255); q[0] = 0; q[1] = 4; q[2] = 5; q[3] = 6; q[30] = 128; q[59] = 127;
    l = lowered(b, q);
    CHECK(l[0] == 0 && l[1] == 4 && l[2] == 5 && l[3] == 5 && l[19] == 5 && l[20] == 255 && l[21] == 255 && l[30] == 128 && l[38] == 255 && l[39] == 255 && l[40] == 5 && l[59] == 5);
    b.assign(20, 2); q.assign(20, 41);
    l = lowered(b, q);
    CHECK(l[0] == 5 && l[19] == 5 && lowered(std::vector<uint8_t>(19, 2), std::vector<uint8_t>(19, 41))[0] == 41 && lowered({}, {}).empty());
    // the key: rolled, and taken from a read in either orientation
    uint64_t seed = 7;
    std::vector<uint8_t> g(120);
    for (auto& x : g) x = (uint8_t)(rnd(&seed) & 3);
    std::vector<uint8_t> gp(30, 0), rcp(30, 0);
    for (size_t i = 0; i < 120; ++i) { gp[i >> 2] |= (uint8_t)(g[i] << (2 * (i & 3))); rcp[i >> 2] |= (uint8_t)((3 - g[119 - i]) << (2 * (i & 3))); }
    Key96 k = key_at(gp.data(), 120, false, 0);
    CHECK(same_key(k, key_of_edge(gp.data())));
    for (uint32_t p = 1; p + KW <= 120; ++p) {
        k = roll(k, g[p + KW - 1]);
        CHECK(same_key(k, key_at(gp.data(), 120, false, p)) && same_key(k, key_at(rcp.data(), 120, true, p)));
        CHECK(hash_of(k) == hash_of(key_at(rcp.data(), 120, true, p)));
    }
    CHECK(!same_key(key_at(gp.data(), 120, false, 0), key_at(gp.data(), 120, false, 1)));
    CHECK((k.lo & 3) == g[119] && (k.hi >> 30) == g[72]);
    // the decision: the thresholds, and the double comparison of :261 is the integer one
    uint32_t base = 9;
    const int32_t s59[4] = {0, 59, 0, 0}, s60[4] = {0, 60, 0, 0}, tw[4] = {40, 0, 80, 0}, tw1[4] = {40, 0, 79, 0}, three[4] = {30, 100, 20, 0}, zero[4] = {0, 0, 0, 0}, tie[4] = {70, 70, 0, 0};
    CHECK(!decide(s59, &base) && decide(s60, &base) && base == 1 && decide(tw, &base) && base == 2 && !decide(tw1, &base) && decide(three, &base) && base == 1 && !decide(zero, &base) && !decide(tie, &base));
    for (int i = 0; i < 20000; ++i) {
        int32_t s[4];
        for (auto& x : s) x = (int32_t)(rnd(&seed) % (i % 2 ? 200u : 0x7FFFFFFFu));
        if (i % 5 == 0) s[1] = s[0] / 2;
        if (i % 7 == 0) s[2] = 2 * (s[3] / 4) + (i & 1);
        int32_t t[4] = {s[0], s[1], s[2], s[3]};
        std::sort(t, t + 4);
        const bool ref = !(t[3] < 60) && !(double(t[3]) < 2.0 * double(t[2]));
        uint32_t bb = 9;
        CHECK(decide(s, &bb) == ref);
        if (ref) CHECK(s[bb] == t[3] && t[3] > t[2]);                           // appended only where the maximum is unique
    }
    CHECK(trim_of(400) == 0 && trim_of(401) == 1 && trim_of(0) == 0 && kmers_of_len(47) == 0 && kmers_of_len(48) == 1 && reach_of_len(48) == 0 && reach_of_len(151) == 103);
    const uint64_t first[] = {0, 0, 3, 3, 7}, arr[] = {1, 3, 3, 9};
    CHECK(owner_of(first, 4, 0) == 1 && owner_of(first, 4, 6) == 3 && lower_bound64(arr, 0, 4, 3) == 1 && lower_bound64(arr, 0, 4, 4) == 3 && lower_bound64(arr, 0, 4, 10) == 4);
    // the plans and the file's fixed parts
    const uint64_t cost[] = {0, 100, 200, 300, 400};
    CHECK(next_batch(cost, 4, 0, 250, 0) == 2 && next_batch(cost, 4, 0, 50, 0) == 1 && next_batch(cost, 4, 1, 50, 2) == 3 && pairs_per_batch(1) == 1 && pairs_per_batch(37) == 19 && pairs_per_batch(0) == 0);
    CHECK(entry_cap(1ull << 40, 77) == 77 && entry_cap(0, 0) == (1ull << 18) && batch_room(0) == (1ull << 20) && batch_room(1ull << 40) == (1ull << 32) - 1 && walk_grid(0, 256) == 1 && walk_grid(1ull << 20, 256) == 16384);
    CHECK(entry_cost(151) >= 32 + 38 + 302 + 52 * 104 + 206 && strlen(MAGIC) == 8 && recs_at(0) == 32 && locs_at(2) == 16 + 48 + 64 && packed_bytes(0) == 0 && packed_bytes(1) == 8 && packed_bytes(33) == 16 && file_size(0, 0, 0) == 32);
    CHECK((pack_ee({0, 1, 2, 3, 1}) == std::vector<uint8_t>{0xE4, 0x01, 0, 0, 0, 0, 0, 0}));
    // THE BOUND on random sets: reads cut from one genome at random places and lengths, so that walks chain from read to read
    for (int round = 0; round < 30; ++round) {
        std::vector<uint8_t> G(400 + rnd(&seed) % 400);
        for (auto& x : G) x = (uint8_t)(rnd(&seed) & 3);
        const size_t n = 1 + rnd(&seed) % 40;
        std::vector<basevector> bases(n); std::vector<qualvector> quals(n);
        std::vector<uint32_t> lens(n);
        for (size_t i = 0; i < n; ++i) {
            const size_t len = 40 + rnd(&seed) % 160, at = rnd(&seed) % (round % 3 ? 60 : G.size() - len);
            bases[i].assign(G.begin() + at, G.begin() + at + len); quals[i].assign(len, (uint8_t)(30 + rnd(&seed) % 34)); lens[i] = (uint32_t)len;
        }
        Walk W;
        stack_walk(basevector(G.begin(), G.begin() + 48 + rnd(&seed) % 50), bases, quals, &W);
        CHECK(W.EE.size() <= ee_bound(lens.data(), n));
        int R = 48;
        for (size_t i = 0; i < n; ++i) if (W.placed[i]) R = std::max(R, W.start[i] + (int)lens[i]);
        CHECK((int)W.EE.size() <= R);
    }
    // the refusals
    const int32_t inv[] = {1, 0, 2};
    const uint64_t ce[] = {0, 2}, zeros[4] = {0, 0, 0, 0};
    const int32_t el[] = {60, 60};
    const uint32_t rl[] = {0};
    const uint8_t store[16] = {};
    const Input I{3, inv, 2, ce, store, zeros, el, zeros, zeros, 0, nullptr, zeros, rl, nullptr, zeros};
    HostResult r;
    const int32_t past[2] = {0, 3}, neg[2] = {-1, 0}, other[2] = {1, 2}, fine[2] = {0, 2};
    CHECK(walks_literal(I, past, 1, &r) == -1 && walks_literal(I, neg, 1, &r) == -1 && walks_literal(I, other, 1, &r) == -2);
    HostResult e;
    CHECK(walks_literal(I, fine, 1, &e) == 0 && e.recs.size() == 2 && e.recs[0].status == WALKED && e.recs[0].nEE == 48 && e.recs[0].placed == 0 && e.recs[1].status == NOT_WALKED && e.ee.size() == 48);
}

int main(int argc, char** argv)
{
    const bool literal = argc == 3 && std::string(argv[1]) == "--literal";
    if (argc != 2 && !literal) { printf("usage: test_walks [--literal] <cases file>\n"); return 2; }
    if (!literal) pieces_and_the_bound();
    std::ifstream in(argv[argc - 1]);
    if (!in) { printf("cannot read %s\n", argv[1]); return 2; }
    std::string line;
    int n_cases = 0;
    while (std::getline(in, line)) {
        if (line.rfind("case ", 0) != 0) { printf("unexpected line: %.60s\n", line.c_str()); return 2; }
        Case c;
        long long E = 0, N = 0, np = 0, nce = 0, K = 0;
        { std::istringstream h(line.substr(5)); h >> c.name >> E >> N >> np >> nce >> K; }
        c.K = (uint32_t)K;
        std::string l[15];
        for (auto& s : l) if (!std::getline(in, s)) { printf("case %s is cut short\n", c.name.c_str()); return 2; }
        c.inv = row<int32_t>(l[0]); c.kmers = row<int32_t>(l[1]); c.edge_packed = hexrow(l[2]); c.ce = urow(l[3]); c.read_first = urow(l[4]); c.reads = urow(l[5]);
        c.pairs = row<int32_t>(l[6]); c.read_len = row<uint32_t>(l[7]); c.read_packed = hexrow(l[8]); c.pq_off = urow(l[9]); c.pq = hexrow(l[10]); c.recs = row<int64_t>(l[11]); c.locs = row<int64_t>(l[12]);
        if (l[13] != "-") for (char ch : l[13]) c.ee.push_back((uint8_t)(ch - '0'));
        const std::vector<uint64_t> k = urow(l[14]);
        for (int32_t x : c.kmers) c.edge_len.push_back(x + (int32_t)K - 1);
        c.edge_off = dense(c.edge_len); c.read_off = dense(c.read_len);
        if (k.size() != 4 || c.inv.size() != (size_t)E || c.kmers.size() != (size_t)E || c.read_len.size() != (size_t)N || c.pairs.size() != 2 * (size_t)np || c.ce.size() != (size_t)nce ||
            c.read_first.size() != (size_t)nce + 1 || c.reads.size() != c.read_first.back() || c.read_packed.size() != c.read_off.back() || c.edge_packed.size() != c.edge_off.back() ||
            c.pq_off.size() != (size_t)N + 1 || c.pq.size() != c.pq_off.back() || (!literal && c.recs.size() != 16 * (size_t)np) || c.locs.size() % 3) {
            printf("case %s is malformed\n", c.name.c_str()); return 2;
        }
        c.walks = k[0]; c.steps = k[1]; c.live_sum = k[2]; c.live_max = k[3];
        if (literal) {
            using namespace dfk_walks;
            std::vector<uint64_t> edge_at(c.ce.size() + 1, 0); std::vector<int32_t> edge_len(c.ce.size() + 1, 0);
            for (size_t r = 0; r < c.ce.size(); ++r) { edge_at[r] = c.edge_off[c.ce[r]]; edge_len[r] = c.edge_len[c.ce[r]]; }
            const Input I{c.inv.size(), c.inv.data(), c.ce.size(), c.ce.data(), c.edge_packed.data(), edge_at.data(), edge_len.data(), c.read_first.data(), c.reads.data(),
                          c.read_len.size(), c.read_packed.data(), c.read_off.data(), c.read_len.data(), c.pq.data(), c.pq_off.data()};
            HostResult r;
            const auto t0 = std::chrono::steady_clock::now();
            const int rc = walks_literal(I, c.pairs.data(), c.pairs.size() / 2, &r);
            const double us = std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count();
            printf("{\"case\": \"%s\", \"rc\": %d, \"pairs\": %zu, \"walks\": %llu, \"steps\": %llu, \"placed\": %zu, \"bases\": %zu, \"us\": %.0f}\n", c.name.c_str(), rc, c.pairs.size() / 2,
                   (unsigned long long)r.walks, (unsigned long long)r.steps, r.locs.size(), r.ee.size(), us);
            ++n_cases;
            continue;
        }
        run_case(c);
        ++n_cases;
    }
    if (literal) return 0;
    if (g_failed) { printf("%d check(s) failed\n", g_failed); return 1; }
    printf("%d recorded cases agree\n", n_cases);
    return 0;
}
