// tests/cpp/test_offsets.cc -- superplus_amd/csrc/dfk_offsets.h against tests/offsets_oracle.py, CPU only, its own main.
//
//   test_offsets CASES [TABLE]
//   test_offsets --literal SEQS     (tools/offsets_cost.py, for scale: the literal form over u64 n_pairs | (2 n_pairs + 1) x u64 starts | the
//                                    bases, on this one thread; prints the counts and the microseconds)
//
// CASES: a file as tests/offsets_cases.py writes it (tests/cpp/offsets_cases.txt holds the recorded ones): per case the pairs'
// sequences, per pair "candidates passed survivors look-ups", per record "offset overlap fraglen mismatch bits-as-hex state".
// TABLE: 401 x 401 little-endian doubles, the Python's table; every cell must equal the header's bit for bit.
// Checked per case: the literal transcription gives the recorded words and records, the doubles as their 8 bytes; the device-order
// form (candidates by bitmap, bad_window from prefix sums, a start's last n, lanes folded pairwise) gives the same bytes in batches
// of 1, 37 and 2^30 pairs, with the same candidates and look-ups; check_input refuses what the stage refuses.
#include <stdio.h>
#include <string.h>
#include <chrono>
#include <fstream>
#include <iostream>
#include <sstream>
#include <string>
#include "dfk_offsets.h"

using namespace dfk_offsets;

static int failures = 0;
#define CHECK(cond, ...) do { if (!(cond)) { ++failures; printf("FAIL %s:%d: ", __FILE__, __LINE__); printf(__VA_ARGS__); printf("\n"); } } while (0)

static double from_hex(const std::string& h)
{
    uint8_t b[8];
    for (int i = 0; i < 8; ++i) b[i] = (uint8_t)std::stoul(h.substr(2 * i, 2), nullptr, 16);
    double d; memcpy(&d, b, 8); return d;
}
static bool same_rec(const Rec& a, const Rec& b) { return memcmp(&a, &b, sizeof(Rec)) == 0; }

int main(int argc, char** argv)
{
    if (argc < 2) { printf("usage: test_offsets CASES [TABLE] | --literal SEQS\n"); return 2; }
    const std::vector<double>& T = table();
    if (std::string(argv[1]) == "--literal") {
        if (argc < 3) return 2;
        std::ifstream f(argv[2], std::ios::binary);
        uint64_t n = 0;
        f.read((char*)&n, 8);
        std::vector<uint64_t> starts(2 * n + 1);
        f.read((char*)starts.data(), (std::streamsize)(8 * starts.size()));
        std::vector<uint8_t> bases(starts.back() + 1);
        f.read((char*)bases.data(), (std::streamsize)starts.back());
        if (!f || check_input(n, starts.data(), bases.data())) { printf("%s: not a sequence file\n", argv[2]); return 2; }
        const auto t0 = std::chrono::steady_clock::now();
        uint64_t cand = 0, passed = 0, alive = 0, looked = 0;
        for (uint64_t p = 0; p < n; ++p) {
            const PairResult R = offsets_literal(bases.data() + starts[2 * p], (int)(starts[2 * p + 1] - starts[2 * p]), bases.data() + starts[2 * p + 1], (int)(starts[2 * p + 2] - starts[2 * p + 1]), T.data());
            cand += R.candidates; passed += R.recs.size(); looked += R.lookups;
            for (const Rec& r : R.recs) alive += r.state == SURVIVES;
        }
        const double us = std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count();
        printf("{\"pairs\": %llu, \"candidates\": %llu, \"passed\": %llu, \"survivors\": %llu, \"lookups\": %llu, \"us\": %.0f}\n", (unsigned long long)n, (unsigned long long)cand,
               (unsigned long long)passed, (unsigned long long)alive, (unsigned long long)looked, us);
        return 0;
    }
    CHECK(T.size() == (size_t)T_DIM * T_DIM, "table size");
    // what the table is by itself: a spot value, the unwritten cells, the per-call form equal to the per-row form
    for (int n = W; n <= MAX_N; n += 19)
        for (int k = 0; k < n; k += 7) { const double v = log10(binomial_sum(n, k, 0.75)); CHECK(memcmp(&v, &T[(size_t)n * T_DIM + k], 8) == 0, "table[%d][%d]: the call and the row differ", n, k); }
    for (int n = 0; n <= MAX_N; ++n) CHECK(T[(size_t)n * T_DIM + n] == 0.0 && (n >= W || T[(size_t)n * T_DIM] == 0.0), "table[%d][%d] is written", n, n);
    CHECK(T[(size_t)20 * T_DIM] == log10(pow(0.25, 20.0)), "table[20][0]");
    if (argc > 2) {
        std::ifstream tf(argv[2], std::ios::binary);
        std::vector<double> P((size_t)T_DIM * T_DIM);
        tf.read((char*)P.data(), (std::streamsize)(P.size() * 8));
        CHECK((size_t)tf.gcount() == P.size() * 8, "%s: short", argv[2]);
        uint64_t differ = 0;
        for (size_t i = 0; i < P.size(); ++i) differ += memcmp(&P[i], &T[i], 8) != 0;
        CHECK(differ == 0, "%llu cells of the table differ from the Python's", (unsigned long long)differ);
        printf("table: %d x %d cells equal bit for bit\n", T_DIM, T_DIM);
    }
    std::ifstream in(argv[1]);
    if (!in) { printf("cannot open %s\n", argv[1]); return 2; }
    std::string line;
    int n_cases = 0;
    while (std::getline(in, line)) {
        if (line.empty()) continue;
        std::istringstream head(line);
        std::string word, name; uint64_t n_pairs = 0, n_recs = 0;
        head >> word >> name >> n_pairs >> n_recs;
        if (word != "case") { printf("bad line: %s\n", line.c_str()); return 2; }
        std::vector<uint64_t> starts(1, 0); std::vector<uint8_t> bases;
        for (uint64_t q = 0; q < 2 * n_pairs; ++q) {
            std::getline(in, line);
            if (line != "-") for (char ch : line) bases.push_back((uint8_t)(ch - '0'));
            starts.push_back(bases.size());
        }
        std::vector<PairWords> want_words(n_pairs); std::vector<uint64_t> want_lookups(n_pairs); std::vector<Rec> want(n_recs);
        for (uint64_t p = 0; p < n_pairs; ++p) { std::getline(in, line); std::istringstream s(line); s >> want_words[p].candidates >> want_words[p].passed >> want_words[p].survivors >> want_lookups[p]; want_words[p].zero = 0; }
        for (uint64_t r = 0; r < n_recs; ++r) {
            std::getline(in, line); std::istringstream s(line); std::string hex;
            memset(&want[r], 0, sizeof(Rec));
            s >> want[r].offset >> want[r].overlap >> want[r].fraglen >> want[r].mismatch >> hex >> want[r].state;
            want[r].bits = from_hex(hex);
        }
        bases.shrink_to_fit();                                                                       // (a read past the end is the sanitizer's to see)
        const uint8_t none = 0;
        const uint8_t* B = bases.empty() ? &none : bases.data();
        CHECK(check_input(n_pairs, starts.data(), B) == 0, "%s: check_input", name.c_str());
        // the literal form
        uint64_t at = 0, total_cand = 0, total_look = 0;
        std::vector<Rec> lit;
        for (uint64_t p = 0; p < n_pairs; ++p) {
            const PairResult R = offsets_literal(B + starts[2 * p], (int)(starts[2 * p + 1] - starts[2 * p]), B + starts[2 * p + 1], (int)(starts[2 * p + 2] - starts[2 * p + 1]), T.data());
            uint32_t alive = 0;
            for (const Rec& r : R.recs) alive += r.state == SURVIVES;
            CHECK(R.candidates == want_words[p].candidates && R.recs.size() == want_words[p].passed && alive == want_words[p].survivors && R.lookups == want_lookups[p],
                  "%s pair %llu: %u candidates, %zu passed, %u survive, %llu look-ups; the oracle %u, %u, %u, %llu", name.c_str(), (unsigned long long)p, R.candidates, R.recs.size(), alive,
                  (unsigned long long)R.lookups, want_words[p].candidates, want_words[p].passed, want_words[p].survivors, (unsigned long long)want_lookups[p]);
            for (size_t i = 0; i < R.recs.size() && at + i < n_recs; ++i)
                CHECK(same_rec(R.recs[i], want[at + i]), "%s pair %llu record %zu: offset %d bits %.17g state %u; the oracle offset %d bits %.17g state %u", name.c_str(), (unsigned long long)p, i,
                      R.recs[i].offset, R.recs[i].bits, R.recs[i].state, want[at + i].offset, want[at + i].bits, want[at + i].state);
            at += R.recs.size(); total_cand += R.candidates; total_look += R.lookups;
            lit.insert(lit.end(), R.recs.begin(), R.recs.end());
        }
        CHECK(at == n_recs, "%s: %llu records, the oracle %llu", name.c_str(), (unsigned long long)at, (unsigned long long)n_recs);
        // the device-order form
        for (uint64_t per : {(uint64_t)1, (uint64_t)37, (uint64_t)1 << 30}) {
            HostResult H;
            offsets_plan(n_pairs, starts.data(), B, per, T.data(), &H);
            bool same = H.words.size() == n_pairs && H.recs.size() == lit.size() && H.starts.size() == n_pairs + 1 && H.candidates == total_cand && H.lookups == total_look;
            for (uint64_t p = 0; same && p < n_pairs; ++p) same = memcmp(&H.words[p], &want_words[p], 16) == 0 && H.starts[p + 1] - H.starts[p] == want_words[p].passed;
            for (size_t i = 0; same && i < lit.size(); ++i) same = same_rec(H.recs[i], lit[i]);
            CHECK(same, "%s: the device-order form differs in batches of %llu", name.c_str(), (unsigned long long)per);
            CHECK(H.batches == (n_pairs + std::min<uint64_t>(per, std::max<uint64_t>(1, n_pairs)) - 1) / std::min<uint64_t>(per, std::max<uint64_t>(1, n_pairs)), "%s: %llu batches", name.c_str(), (unsigned long long)H.batches);
        }
        ++n_cases;
    }
    // what the stage refuses
    {
        const uint64_t fall[3] = {0, 5, 4}, from1[3] = {1, 2, 3}, longer[3] = {0, 401, 401}, fine[3] = {0, 400, 800};
        std::vector<uint8_t> b(800, 1);
        CHECK(check_input(1, fall, b.data()) == 1 && check_input(1, from1, b.data()) == 1 && check_input(1, longer, b.data()) == 2 && check_input(1, fine, b.data()) == 0, "check_input");
        b[799] = 4;
        CHECK(check_input(1, fine, b.data()) == 3, "check_input: a base above 3");
    }
    CHECK(pairs_per_batch(1ull << 40, 0) == MAX_BATCH && pairs_per_batch(0, 0) == 1 && pairs_per_batch(1ull << 40, 37) == 37, "pairs_per_batch");
    CHECK(file_size(0, 0) == 24 && file_size(2, 3) == 16 + 24 + 32 + 96, "file_size");
    if (failures) { printf("%d failure(s)\n", failures); return 1; }
    printf("%d recorded cases agree\n", n_cases);
    return 0;
}
