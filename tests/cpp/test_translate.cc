// tests/cpp/test_translate.cc -- superplus_amd/csrc/dfk_translate.h on the host (tests/test_translate_cpu.py builds it plain and under
// -fsanitize=address,undefined; `make` builds ../test_translate):
//   1. literal() -- GapToyTools4.cc:163-196 as written -- and translate_one() -- the device's order of work, with literal() where it flags
//      -- against the cases tests/translate_cases.py recorded from tests/translate_oracle.py: outcome, kind, whether the host route is
//      taken, the content digest;
//   2. walk_first() plus the host route against literal() on random tables;
//   3. the bound: on random tables whose to3[e0] spells e0 from left3[e0] (check_invariants' condition) no offset below kmers(e0) is flagged,
//      and start < inside_bound() never runs off;
//   4. the refusals of check_tables() / check_path().
//   test_translate tests/cpp/translate_cases.txt
//   test_translate --time FILE    tools/translate_cost.py's timing of literal() on one thread: FILE holds little-endian u64 K, E, n_to3, E3, N,
//                                 n_path_edges, then to3_first u64[E + 1], to3 i32[], left3 i32[E], kmers3 i32[E3], offsets i32[N], first u64[N + 1], edges i32[]
#include "dfk_translate.h"

#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <random>
#include <sstream>

using namespace dfk_translate;

static int g_bad = 0;
#define CHECK(cond, ...) do { if (!(cond)) { ++g_bad; fprintf(stderr, "FAIL %s:%d: ", __FILE__, __LINE__); fprintf(stderr, __VA_ARGS__); fputc('\n', stderr); } } while (0)

static std::vector<long long> numbers(const std::string& line, const char* tag)
{
    std::istringstream in(line);
    std::string t; in >> t;
    if (t != tag) { fprintf(stderr, "expected a %s line, got: %s\n", tag, line.c_str()); exit(2); }
    std::vector<long long> v; long long x;
    while (in >> x) v.push_back(x);
    return v;
}

static int recorded(const char* file)
{
    std::ifstream in(file);
    if (!in) { fprintf(stderr, "cannot open %s\n", file); exit(2); }
    std::string line;
    int n_cases = 0;
    while (std::getline(in, line)) {
        std::istringstream head(line);
        std::string tag, name; long long K, E, E3, N;
        head >> tag >> name >> K >> E >> E3 >> N;
        if (tag != "case") { fprintf(stderr, "expected a case line, got: %s\n", line.c_str()); exit(2); }
        Tables T; T.K = (int32_t)K;
        std::getline(in, line); for (long long x : numbers(line, "F")) T.to3_first.push_back((uint64_t)x);
        std::getline(in, line); for (long long x : numbers(line, "T")) T.to3.push_back((int32_t)x);
        std::getline(in, line); for (long long x : numbers(line, "L")) T.left3.push_back((int32_t)x);
        std::getline(in, line); for (long long x : numbers(line, "M")) T.kmers3.push_back((int32_t)x);
        CHECK((long long)T.left3.size() == E && (long long)T.kmers3.size() == E3, "%s: table sizes", name.c_str());
        CHECK(check_tables(T).empty(), "%s: %s", name.c_str(), check_tables(T).c_str());
        uint64_t sum = 0, xr = 0;
        for (long long r = 0; r < N; ++r) {
            std::getline(in, line);
            const std::vector<long long> v = numbers(line, "R");
            Path p; p.offset = (int32_t)v[0];
            const size_t n = (size_t)v[1];
            for (size_t j = 0; j < n; ++j) p.edges.push_back((int32_t)v[2 + j]);
            const int32_t want_off = (int32_t)v[2 + n], want_edge = (int32_t)v[3 + n];
            const Kind want_kind = (Kind)v[4 + n];
            const bool want_host = v[5 + n] != 0;
            CHECK(check_path(T, p).empty(), "%s read %lld: %s", name.c_str(), r, check_path(T, p).c_str());
            Kind k1, k2; bool host = false;
            const Outcome a = literal(T, p, &k1), b = translate_one(T, p, &k2, &host);
            CHECK(a.offset == want_off && a.edge == want_edge && k1 == want_kind, "%s read %lld: literal() gives (%d, %d) kind %d, recorded (%d, %d) kind %d", name.c_str(), r, a.offset, a.edge, (int)k1,
                  want_off, want_edge, (int)want_kind);
            CHECK(b.offset == want_off && b.edge == want_edge && k2 == want_kind, "%s read %lld: translate_one() gives (%d, %d) kind %d, recorded (%d, %d) kind %d", name.c_str(), r, b.offset, b.edge,
                  (int)k2, want_off, want_edge, (int)want_kind);
            CHECK(host == want_host, "%s read %lld: host route %d, recorded %d", name.c_str(), r, (int)host, (int)want_host);
            CHECK(record_words(b.edge) == (b.edge < 0 ? 2u : 3u) && valid_id(b.edge, E3), "%s read %lld: words / valid", name.c_str(), r);
            const uint64_t h = read_digest((uint64_t)r, b.offset, b.edge);
            sum += h; xr ^= mix64(h + DIGEST_XOR);
        }
        std::getline(in, line);
        std::istringstream d(line);
        unsigned long long ws = 0, wx = 0;
        d >> tag >> ws >> wx;
        CHECK(tag == "digest" && ws == sum && wx == xr, "%s: digest %llu %llu, recorded %llu %llu", name.c_str(), (unsigned long long)sum, (unsigned long long)xr, ws, wx);
        ++n_cases;
    }
    return n_cases;
}

static Tables random_tables(std::mt19937_64& g, bool spelled, std::vector<int32_t>* kmers_old)
{
    auto below = [&](uint64_t n) { return (int64_t)(g() % n); };
    Tables T; T.K = 2 * (int32_t)(2 + below(30));
    const int E = 1 + (int)below(12), E3 = 1 + (int)below(12);
    for (int e = 0; e < E3; ++e) T.kmers3.push_back(1 + (int32_t)below(50));
    T.to3_first.push_back(0);
    for (int e = 0; e < E; ++e) {
        const int n = spelled ? 1 + (int)below(5) : (int)below(5);
        int64_t total = 0;
        for (int j = 0; j < n; ++j) { T.to3.push_back((int32_t)below(E3)); total += T.kmers3[T.to3.back()]; }
        T.to3_first.push_back(T.to3.size());
        if (spelled) {                                                  // e lies on its ids from left3 on: left3 + kmers(e) <= the ids' K-mers
            const int32_t l = (int32_t)below(T.kmers3[T.to3[T.to3_first[e]]]);
            T.left3.push_back(l);
            kmers_old->push_back(1 + (int32_t)below(total - l));
        } else T.left3.push_back((int32_t)below(40));
    }
    return T;
}

static void random_agreement()
{
    std::mt19937_64 g(20240607);
    uint64_t n_host = 0, n_dev = 0;
    for (int t = 0; t < 3000; ++t) {
        const Tables T = random_tables(g, false, nullptr);
        CHECK(check_tables(T).empty(), "random tables: %s", check_tables(T).c_str());
        for (int r = 0; r < 20; ++r) {
            Path p; p.offset = (int32_t)(g() % 400) - 60;
            const int n = (int)(g() % 5);
            for (int j = 0; j < n; ++j) p.edges.push_back((int32_t)(g() % T.n_edges()));
            Kind k1, k2; bool host = false;
            const Outcome a = literal(T, p, &k1), b = translate_one(T, p, &k2, &host);
            CHECK(a.offset == b.offset && a.edge == b.edge && k1 == k2, "random: literal (%d, %d) kind %d, shared pieces (%d, %d) kind %d", a.offset, a.edge, (int)k1, b.offset, b.edge, (int)k2);
            // a read the device decides needs nothing but the first edge: the rest of the path must not matter
            if (!host && n) { Path q = p; q.edges.resize(1); const Outcome c = literal(T, q); CHECK(c.offset == a.offset && c.edge == a.edge, "random: the answer depends on edges behind the first"); }
            (host ? n_host : n_dev) += 1;
        }
    }
    CHECK(n_host > 1000 && n_dev > 1000, "random: %llu on the host route, %llu not", (unsigned long long)n_host, (unsigned long long)n_dev);
}

static void bound()
{
    std::mt19937_64 g(777);
    uint64_t n_walk = 0;
    for (int t = 0; t < 3000; ++t) {
        std::vector<int32_t> kmers;
        const Tables T = random_tables(g, true, &kmers);
        for (uint64_t e = 0; e < T.n_edges(); ++e) {
            const int32_t* ids = T.to3.data() + T.to3_first[e];
            const uint64_t n = T.to3_first[e + 1] - T.to3_first[e];
            const int64_t S = inside_bound(ids, n, T.kmers3.data());
            CHECK(S >= (int64_t)T.left3[e] + kmers[e], "bound: the ids of edge %llu hold %lld K-mers, left3 + kmers = %d", (unsigned long long)e, (long long)S, T.left3[e] + kmers[e]);
            for (int32_t off = -5; off < kmers[e]; ++off) {                    // every offset the pather can give
                bool flagged = true; Kind k;
                const Outcome o = decide(T, off, true, (int32_t)e, &flagged, &k);
                CHECK(!flagged && o.edge >= 0, "bound: offset %d on an edge of %d K-mers is flagged", off, kmers[e]);
                n_walk += k == WALK;
            }
            for (int32_t start = (int32_t)S - 1; start >= 0 && start >= (int32_t)S - 3; --start)   // the bound itself, at its edge
                CHECK(walk_first(ids, n, T.kmers3.data(), T.K, start).edge >= 0, "bound: start %d < %lld runs off", start, (long long)S);
        }
    }
    CHECK(n_walk > 1000, "bound: only %llu walks", (unsigned long long)n_walk);
}

static int refusals()
{
    Tables T; T.K = 48; T.to3_first = {0, 1, 2}; T.to3 = {0, 1}; T.left3 = {0, 3}; T.kmers3 = {5, 6};
    CHECK(check_tables(T).empty(), "the good tables: %s", check_tables(T).c_str());
    int n = 0;
    auto refused = [&](const Tables& X, const char* what) { CHECK(!check_tables(X).empty(), "not refused: %s", what); ++n; };
    { Tables X = T; X.to3_first[0] = 1; refused(X, "to3_first not starting at 0"); }
    { Tables X = T; X.to3_first[1] = 3; refused(X, "to3_first falling"); }
    { Tables X = T; X.to3_first[2] = 1; refused(X, "to3_first not ending at the entries"); }
    { Tables X = T; X.to3[1] = 2; refused(X, "a to3 id past hb3"); }
    { Tables X = T; X.to3[0] = -1; refused(X, "a negative to3 id"); }
    { Tables X = T; X.kmers3[1] = 0; refused(X, "an hb3 edge of no K-mers"); }
    { Tables X = T; X.left3[0] = LIMIT; refused(X, "left3 of 2^30"); }
    { Tables X = T; X.to3_first.pop_back(); refused(X, "to3_first too short"); }
    Path p; p.offset = 0; p.edges = {1, 0};
    CHECK(check_path(T, p).empty(), "the good path");
    { Path q = p; q.offset = LIMIT; CHECK(!check_path(T, q).empty(), "not refused: an offset of 2^30"); ++n; }
    { Path q = p; q.offset = -LIMIT; CHECK(!check_path(T, q).empty(), "not refused: an offset of -2^30"); ++n; }
    { Path q = p; q.edges[1] = 2; CHECK(!check_path(T, q).empty(), "not refused: an edge past the graph"); ++n; }
    { Path q = p; q.edges[0] = -1; CHECK(!check_path(T, q).empty(), "not refused: a negative edge"); ++n; }
    // Validate's one test, signed as the reference has it
    CHECK(valid_id(0, 2) && valid_id(1, 2) && !valid_id(2, 2) && valid_id(-1, 2), "valid_id");
    CHECK(plan_of(0).n_units == 0 && plan_of(1).n_units == 1 && plan_of(256).n_units == 1 && plan_of(257).n_units == 2 && plan_of(257).scan_words == 3 && unit_of(255) == 0 && unit_of(256) == 1, "plan");
    return n;
}

static int timed(const char* file)
{
    FILE* f = fopen(file, "rb");
    if (!f) { fprintf(stderr, "cannot open %s\n", file); return 2; }
    uint64_t h[6];
    bool ok = fread(h, 8, 6, f) == 6;
    Tables T; T.K = (int32_t)h[0];
    T.to3_first.resize(h[1] + 1); T.to3.resize(h[2]); T.left3.resize(h[1]); T.kmers3.resize(h[3]);
    std::vector<int32_t> offsets(h[4]), edges(h[5]);
    std::vector<uint64_t> first(h[4] + 1);
    auto rd = [&](void* p, size_t size, size_t n) { if (n && fread(p, size, n, f) != n) ok = false; };
    rd(T.to3_first.data(), 8, T.to3_first.size()); rd(T.to3.data(), 4, T.to3.size()); rd(T.left3.data(), 4, T.left3.size()); rd(T.kmers3.data(), 4, T.kmers3.size());
    rd(offsets.data(), 4, offsets.size()); rd(first.data(), 8, first.size()); rd(edges.data(), 4, edges.size());
    fclose(f);
    if (!ok || !check_tables(T).empty()) { fprintf(stderr, "%s does not hold what --time reads: %s\n", file, check_tables(T).c_str()); return 2; }
    const auto t0 = std::chrono::steady_clock::now();
    uint64_t sum = 0, xr = 0, placed = 0;
    Path p;
    for (uint64_t r = 0; r < h[4]; ++r) {
        p.offset = offsets[r];
        p.edges.assign(edges.begin() + first[r], edges.begin() + first[r + 1]);
        const Outcome o = literal(T, p);
        const uint64_t d = read_digest(r, o.offset, o.edge);
        sum += d; xr ^= mix64(d + DIGEST_XOR); placed += o.edge >= 0;
    }
    const double us = std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count();
    printf("LITERAL {\"us\": %.0f, \"reads\": %llu, \"placed\": %llu, \"sum\": %llu, \"xor\": %llu}\n", us, (unsigned long long)h[4], (unsigned long long)placed, (unsigned long long)sum, (unsigned long long)xr);
    return 0;
}

int main(int argc, char** argv)
{
    if (argc == 3 && std::string(argv[1]) == "--time") return timed(argv[2]);
    if (argc != 2) { fprintf(stderr, "usage: %s translate_cases.txt\n", argv[0]); return 2; }
    const int n_cases = recorded(argv[1]);
    random_agreement();
    bound();
    const int n_refused = refusals();
    if (g_bad) { printf("%d checks failed\n", g_bad); return 1; }
    printf("%d recorded cases agree, %d refusals refused\n", n_cases, n_refused);
    return 0;
}
