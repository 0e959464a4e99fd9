// tests/cpp/fallback_expected.h -- inputs of tests/cpp/test_fallback.cc and what the count stage's host code computed for
// them before its decisions moved into superplus_amd/csrc/dfk_fallback.h (recorded once from that code; numbers only).
#pragma once
#include <cstdint>

static const int X_LOG2S = 11;   // CountCfg<K>::LOG2S, the same at K = 40, 48 and 60
static const uint64_t X_INST[] = {
    1ull, 699ull, 700ull, 701ull, 1400ull, 1401ull, 1023ull, 1024ull, 1025ull, 2047ull, 2048ull, 2049ull,
    2800ull, 2801ull, 5000ull, 70000ull, 100000ull, 262143ull, 262144ull, 262145ull, 1048576ull, 100000000ull, 1468006400ull, 2936012099ull,
    2936012100ull, 2936012799ull, 2936012800ull, 2936012801ull, 4294967295ull, 4294967296ull, 4294967297ull, 5872025600ull, 5872025601ull, 1099511627776ull,
};
static const double X_SEEN[4] = {0.0, 0.02, 0.3, 1.0};                     // distinct_per_inst (0: first pass)
static const uint32_t X_SWITCH[3][2] = {{2, 8}, {20, 8}, {20, 0}};         // DFK_SPLIT_FROM_LOG2, DFK_MAX_SUBPASS_LOG2
static const double X_ROUTE_DPI[4] = {0.5, 0.040000000000000001, 0.59999999999999998, 1, };
static const double X_TABLE_DPI[4] = {1, 0.050000000000000003, 0.44999999999999996, 1, };
// the route of a single bucket, [seen][switch][inst]: kind * 100 + p; kind 1 = split into 2^p sub-buckets, 2 = 2^p sub-passes, 3 = HBM table
static const uint16_t X_ROUTE[] = {
    201, 201, 201, 201, 201, 201, 201, 201, 201, 201, 201, 201,
    102, 102, 102, 106, 107, 108, 108, 108, 110, 117, 121, 121,
    121, 121, 122, 122, 122, 300, 300, 300, 300, 300, 201, 201,
    201, 201, 201, 201, 201, 201, 201, 201, 201, 201, 201, 201,
    202, 206, 206, 207, 208, 300, 300, 300, 121, 121, 121, 121,
    122, 122, 122, 300, 300, 300, 300, 300, 300, 300, 300, 300,
    300, 300, 300, 300, 300, 300, 300, 300, 300, 300, 300, 300,
    300, 300, 300, 300, 300, 300, 121, 121, 121, 121, 122, 122,
    122, 300, 300, 300, 300, 300, 201, 201, 201, 201, 201, 201,
    201, 201, 201, 201, 201, 201, 201, 201, 201, 103, 103, 104,
    104, 104, 106, 113, 117, 118, 118, 118, 118, 118, 118, 300,
    300, 300, 300, 300, 201, 201, 201, 201, 201, 201, 201, 201,
    201, 201, 201, 201, 201, 201, 201, 202, 202, 204, 204, 300,
    300, 300, 300, 300, 300, 300, 300, 300, 300, 300, 300, 300,
    300, 300, 300, 300, 300, 300, 300, 300, 300, 300, 300, 300,
    300, 300, 300, 300, 300, 300, 300, 300, 300, 300, 300, 300,
    300, 300, 300, 300, 300, 300, 300, 300, 300, 300, 300, 300,
    201, 201, 201, 201, 201, 201, 201, 201, 201, 201, 201, 201,
    102, 102, 103, 106, 107, 108, 108, 108, 110, 117, 121, 122,
    122, 122, 122, 122, 122, 300, 300, 300, 300, 300, 201, 201,
    201, 201, 201, 201, 201, 201, 201, 201, 201, 201, 201, 201,
    202, 206, 206, 208, 208, 300, 300, 300, 121, 122, 122, 122,
    122, 122, 122, 300, 300, 300, 300, 300, 300, 300, 300, 300,
    300, 300, 300, 300, 300, 300, 300, 300, 300, 300, 300, 300,
    300, 300, 300, 300, 300, 300, 121, 122, 122, 122, 122, 122,
    122, 300, 300, 300, 300, 300, 201, 201, 201, 201, 102, 102,
    201, 201, 201, 102, 102, 102, 103, 103, 103, 107, 108, 109,
    109, 109, 111, 118, 122, 122, 122, 122, 300, 300, 300, 300,
    300, 300, 300, 300, 201, 201, 201, 201, 201, 201, 201, 201,
    201, 201, 202, 202, 202, 202, 203, 207, 207, 208, 300, 300,
    300, 300, 122, 122, 122, 122, 300, 300, 300, 300, 300, 300,
    300, 300, 300, 300, 300, 300, 300, 300, 300, 300, 300, 300,
    300, 300, 300, 300, 300, 300, 300, 300, 300, 300, 300, 300,
    122, 122, 122, 122, 300, 300, 300, 300, 300, 300, 300, 300,
};
// the same for a bucket that is not split (no room, or not a candidate)
static const uint16_t X_ROUTE_UNSPLIT[] = {
    201, 201, 201, 201, 201, 201, 201, 201, 201, 201, 201, 201,
    201, 201, 202, 206, 206, 207, 208, 300, 300, 300, 300, 300,
    300, 300, 300, 300, 300, 300, 300, 300, 300, 300, 201, 201,
    201, 201, 201, 201, 201, 201, 201, 201, 201, 201, 201, 201,
    202, 206, 206, 207, 208, 300, 300, 300, 300, 300, 300, 300,
    300, 300, 300, 300, 300, 300, 300, 300, 300, 300, 300, 300,
    300, 300, 300, 300, 300, 300, 300, 300, 300, 300, 300, 300,
    300, 300, 300, 300, 300, 300, 300, 300, 300, 300, 300, 300,
    300, 300, 300, 300, 300, 300, 201, 201, 201, 201, 201, 201,
    201, 201, 201, 201, 201, 201, 201, 201, 201, 202, 202, 204,
    204, 300, 300, 300, 300, 300, 300, 300, 300, 300, 300, 300,
    300, 300, 300, 300, 201, 201, 201, 201, 201, 201, 201, 201,
    201, 201, 201, 201, 201, 201, 201, 202, 202, 204, 204, 300,
    300, 300, 300, 300, 300, 300, 300, 300, 300, 300, 300, 300,
    300, 300, 300, 300, 300, 300, 300, 300, 300, 300, 300, 300,
    300, 300, 300, 300, 300, 300, 300, 300, 300, 300, 300, 300,
    300, 300, 300, 300, 300, 300, 300, 300, 300, 300, 300, 300,
    201, 201, 201, 201, 201, 201, 201, 201, 201, 201, 201, 201,
    201, 201, 202, 206, 206, 208, 208, 300, 300, 300, 300, 300,
    300, 300, 300, 300, 300, 300, 300, 300, 300, 300, 201, 201,
    201, 201, 201, 201, 201, 201, 201, 201, 201, 201, 201, 201,
    202, 206, 206, 208, 208, 300, 300, 300, 300, 300, 300, 300,
    300, 300, 300, 300, 300, 300, 300, 300, 300, 300, 300, 300,
    300, 300, 300, 300, 300, 300, 300, 300, 300, 300, 300, 300,
    300, 300, 300, 300, 300, 300, 300, 300, 300, 300, 300, 300,
    300, 300, 300, 300, 300, 300, 201, 201, 201, 201, 201, 201,
    201, 201, 201, 201, 202, 202, 202, 202, 203, 207, 207, 208,
    300, 300, 300, 300, 300, 300, 300, 300, 300, 300, 300, 300,
    300, 300, 300, 300, 201, 201, 201, 201, 201, 201, 201, 201,
    201, 201, 202, 202, 202, 202, 203, 207, 207, 208, 300, 300,
    300, 300, 300, 300, 300, 300, 300, 300, 300, 300, 300, 300,
    300, 300, 300, 300, 300, 300, 300, 300, 300, 300, 300, 300,
    300, 300, 300, 300, 300, 300, 300, 300, 300, 300, 300, 300,
    300, 300, 300, 300, 300, 300, 300, 300, 300, 300, 300, 300,
};
// one plan of sub-passes: buckets 10 + i of X_PLAN_INST[i] instances, seen = 1.0, default switches, none split
static const uint64_t X_PLAN_INST[] = {
    1ull, 1401ull, 3000ull, 5000ull, 262145ull, 1025ull,
};
static const uint32_t X_PLAN_BUCKET[] = {
    10u, 10u, 11u, 11u, 12u, 12u, 12u, 12u, 13u, 13u, 13u, 13u,
    13u, 13u, 13u, 13u, 15u, 15u,
};
static const uint32_t X_PLAN_WORD[] = {
    256u, 257u, 256u, 257u, 512u, 513u, 514u, 515u, 768u, 769u, 770u, 771u,
    772u, 773u, 774u, 775u, 256u, 257u,
};
static const uint32_t X_PLAN_HUGE[] = {
    14u,
};
// sub-passes that overflowed again {bucket, marker | word} and what replaces them
static const uint32_t X_AGAIN[] = {
    7u, 2147483904u, 7u, 2147483905u, 9u, 2147484421u, 11u, 2147485567u, 12u, 2147484163u,
};
static const uint32_t X_REFINED_BUCKET[] = {
    7u, 7u, 7u, 7u, 9u, 9u, 11u, 11u, 12u, 12u,
};
static const uint32_t X_REFINED_WORD[] = {
    512u, 514u, 513u, 515u, 1029u, 1037u, 2175u, 2303u, 771u, 775u,
};
// instances a group of split buckets may hold, by the arena's largest free block
static const uint64_t X_CAN[] = {
    0ull, 536870912ull, 536870913ull, 536870948ull, 1073741824ull, 30000000000ull, 180000000000ull,
};
static const uint64_t X_CAP[] = {
    0ull, 0ull, 0ull, 1ull, 15000804ull, 823234489ull, 5014410959ull,
};
// the groups of these candidates under X_CAP[4] (ends; the last one repeats its start: that bucket does not fit)
static const uint64_t X_GROUP_INST[] = {
    5000000ull, 5000000ull, 5000001ull, 1ull, 14999999ull, 15000001ull, 3ull, 15000000ull, 20000000ull, 4ull,
};
static const uint64_t X_GROUP_END[] = {
    4ull, 5ull, 7ull, 8ull, 8ull,
};
static const uint64_t X_BIG_INST[] = {
    1ull, 255ull, 256ull, 4031ull, 4032ull, 4033ull, 5000ull, 81000ull, 100000ull, 1048576ull, 100000000ull, 4294967295ull,
    4294967296ull,
};
// [seen] -> per_inst = X_TABLE_DPI[seen]: log2 of the slots of every table, whether all are certain; then the same after one doubling
static const uint32_t X_BIG_LOG2S[] = {
    13u, 13u, 13u, 13u, 13u, 13u, 14u, 18u, 18u, 22u, 28u, 34u,
    34u, 13u, 13u, 13u, 13u, 13u, 13u, 13u, 14u, 14u, 17u, 24u,
    29u, 29u, 13u, 13u, 13u, 13u, 13u, 13u, 13u, 17u, 17u, 20u,
    27u, 32u, 32u, 13u, 13u, 13u, 13u, 13u, 13u, 14u, 18u, 18u,
    22u, 28u, 34u, 34u, 13u, 13u, 13u, 13u, 13u, 13u, 14u, 18u,
    18u, 22u, 28u, 34u, 34u, 13u, 13u, 13u, 13u, 13u, 13u, 13u,
    15u, 15u, 18u, 25u, 30u, 30u, 13u, 13u, 13u, 13u, 13u, 13u,
    14u, 18u, 18u, 21u, 28u, 33u, 33u, 13u, 13u, 13u, 13u, 13u,
    13u, 14u, 18u, 18u, 22u, 28u, 34u, 34u,
};
static const uint8_t X_BIG_CERTAIN[] = {
    1, 0, 0, 1, 1, 0, 0, 1,
};
static const uint64_t X_BIG_SLOTS[] = {
    34632957952ull, 1090740224ull, 8725520384ull, 34632957952ull, 34632957952ull, 2181423104ull, 17450991616ull, 34632957952ull,
};
static const int X_BIG_CFG[5][3] = {{40, 3, 1}, {48, 3, 0}, {48, 3, 3}, {60, 4, 1}, {60, 4, 7}};   // K, KTraits<K>::KW, barcode words of a slot
// [seen][cfg][table]: the table's first word in the pool; [seen][cfg]: words of the pool
static const uint64_t X_BIG_OFF[] = {
    0ull, 57344ull, 114688ull, 172032ull, 229376ull, 286720ull, 344064ull, 458752ull, 2293760ull, 4128768ull, 33488896ull, 1912537088ull,
    122171621376ull, 0ull, 57344ull, 114688ull, 172032ull, 229376ull, 286720ull, 344064ull, 458752ull, 2293760ull, 4128768ull, 33488896ull,
    1912537088ull, 122171621376ull, 0ull, 73728ull, 147456ull, 221184ull, 294912ull, 368640ull, 442368ull, 589824ull, 2949120ull, 5308416ull,
    43057152ull, 2458976256ull, 157077798912ull, 0ull, 65536ull, 131072ull, 196608ull, 262144ull, 327680ull, 393216ull, 524288ull, 2621440ull,
    4718592ull, 38273024ull, 2185756672ull, 139624710144ull, 0ull, 114688ull, 229376ull, 344064ull, 458752ull, 573440ull, 688128ull, 917504ull,
    4587520ull, 8257536ull, 66977792ull, 3825074176ull, 244343242752ull, 0ull, 57344ull, 114688ull, 172032ull, 229376ull, 286720ull, 344064ull,
    401408ull, 516096ull, 630784ull, 1548288ull, 118988800ull, 3877085184ull, 0ull, 57344ull, 114688ull, 172032ull, 229376ull, 286720ull,
    344064ull, 401408ull, 516096ull, 630784ull, 1548288ull, 118988800ull, 3877085184ull, 0ull, 73728ull, 147456ull, 221184ull, 294912ull,
    368640ull, 442368ull, 516096ull, 663552ull, 811008ull, 1990656ull, 152985600ull, 4984823808ull, 0ull, 65536ull, 131072ull, 196608ull,
    262144ull, 327680ull, 393216ull, 458752ull, 589824ull, 720896ull, 1769472ull, 135987200ull, 4430954496ull, 0ull, 114688ull, 229376ull,
    344064ull, 458752ull, 573440ull, 688128ull, 802816ull, 1032192ull, 1261568ull, 3096576ull, 237977600ull, 7754170368ull, 0ull, 57344ull,
    114688ull, 172032ull, 229376ull, 286720ull, 344064ull, 401408ull, 1318912ull, 2236416ull, 9576448ull, 949100544ull, 31013871616ull, 0ull,
    57344ull, 114688ull, 172032ull, 229376ull, 286720ull, 344064ull, 401408ull, 1318912ull, 2236416ull, 9576448ull, 949100544ull, 31013871616ull,
    0ull, 73728ull, 147456ull, 221184ull, 294912ull, 368640ull, 442368ull, 516096ull, 1695744ull, 2875392ull, 12312576ull, 1220272128ull,
    39874977792ull, 0ull, 65536ull, 131072ull, 196608ull, 262144ull, 327680ull, 393216ull, 458752ull, 1507328ull, 2555904ull, 10944512ull,
    1084686336ull, 35444424704ull, 0ull, 114688ull, 229376ull, 344064ull, 458752ull, 573440ull, 688128ull, 802816ull, 2637824ull, 4472832ull,
    19152896ull, 1898201088ull, 62027743232ull, 0ull, 57344ull, 114688ull, 172032ull, 229376ull, 286720ull, 344064ull, 458752ull, 2293760ull,
    4128768ull, 33488896ull, 1912537088ull, 122171621376ull, 0ull, 57344ull, 114688ull, 172032ull, 229376ull, 286720ull, 344064ull, 458752ull,
    2293760ull, 4128768ull, 33488896ull, 1912537088ull, 122171621376ull, 0ull, 73728ull, 147456ull, 221184ull, 294912ull, 368640ull, 442368ull,
    589824ull, 2949120ull, 5308416ull, 43057152ull, 2458976256ull, 157077798912ull, 0ull, 65536ull, 131072ull, 196608ull, 262144ull, 327680ull,
    393216ull, 524288ull, 2621440ull, 4718592ull, 38273024ull, 2185756672ull, 139624710144ull, 0ull, 114688ull, 229376ull, 344064ull, 458752ull,
    573440ull, 688128ull, 917504ull, 4587520ull, 8257536ull, 66977792ull, 3825074176ull, 244343242752ull,
};
static const uint64_t X_BIG_WORDS[] = {
    242430705664ull, 242430705664ull, 311696621568ull, 277063663616ull, 484861411328ull, 7635181568ull, 7635181568ull, 9816662016ull, 8725921792ull, 15270363136ull, 61078642688ull, 61078642688ull,
    78529683456ull, 69804163072ull, 122157285376ull, 242430705664ull, 242430705664ull, 311696621568ull, 277063663616ull, 484861411328ull,
};
static const uint64_t X_CHUNK_REC[] = {
    0ull, 1ull, 31ull, 32ull, 33ull, 64ull, 1000ull, 4294967301ull,
};
static const uint64_t X_CHUNK_PRE[] = {
    0ull, 0ull, 1ull, 2ull, 3ull, 5ull, 7ull, 39ull, 134217768ull,
};
// hole compaction: parts of chunks of 8 entries; per case the WgOut {chunk, used} pairs, part_cursor, n_lds and the moves
static const uint64_t X_HOLES_NOHOLES_WG[] = {
    0ull, 8ull, 16ull, 8ull, 8ull, 8ull,
};
static const uint64_t X_HOLES_NOHOLES_CLAIMED = 24, X_HOLES_NOHOLES_NLDS = 24;
static const uint64_t X_HOLES_NOHOLES_SRC[] = {
    18446744073709551615ull,
};
static const uint64_t X_HOLES_NOHOLES_DST[] = {
    18446744073709551615ull,
};
static const uint64_t X_HOLES_UNTOUCHED_WG[] = {
    18446744073709551615ull, 8ull, 18446744073709551615ull, 8ull,
};
static const uint64_t X_HOLES_UNTOUCHED_CLAIMED = 0, X_HOLES_UNTOUCHED_NLDS = 0;
static const uint64_t X_HOLES_UNTOUCHED_SRC[] = {
    18446744073709551615ull,
};
static const uint64_t X_HOLES_UNTOUCHED_DST[] = {
    18446744073709551615ull,
};
static const uint64_t X_HOLES_ABOVE_WG[] = {
    0ull, 8ull, 8ull, 8ull, 16ull, 5ull,
};
static const uint64_t X_HOLES_ABOVE_CLAIMED = 24, X_HOLES_ABOVE_NLDS = 21;
static const uint64_t X_HOLES_ABOVE_SRC[] = {
    18446744073709551615ull,
};
static const uint64_t X_HOLES_ABOVE_DST[] = {
    18446744073709551615ull,
};
static const uint64_t X_HOLES_ONE_WG[] = {
    24ull, 3ull,
};
static const uint64_t X_HOLES_ONE_CLAIMED = 32, X_HOLES_ONE_NLDS = 27;
static const uint64_t X_HOLES_ONE_SRC[] = {
    18446744073709551615ull,
};
static const uint64_t X_HOLES_ONE_DST[] = {
    18446744073709551615ull,
};
static const uint64_t X_HOLES_MIXED_WG[] = {
    32ull, 2ull, 0ull, 3ull, 18446744073709551615ull, 8ull, 24ull, 8ull, 40ull, 7ull, 48ull, 0ull,
};
static const uint64_t X_HOLES_MIXED_CLAIMED = 56, X_HOLES_MIXED_NLDS = 36;
static const uint64_t X_HOLES_MIXED_SRC[] = {
    40ull, 41ull, 42ull, 43ull, 44ull, 45ull, 46ull, 18446744073709551615ull,
};
static const uint64_t X_HOLES_MIXED_DST[] = {
    3ull, 4ull, 5ull, 6ull, 7ull, 34ull, 35ull, 18446744073709551615ull,
};
// halving: overflowed items {b0, b1}, the items of the next launch, the single buckets
static const uint32_t X_HALVE_IN[] = {
    0u, 8u, 8u, 9u, 9u, 12u, 12u, 14u, 100u, 100u, 4000000000u, 4000000005u,
};
static const uint32_t X_HALVE_NEXT[] = {
    0u, 4u, 4u, 8u, 9u, 10u, 10u, 12u, 12u, 13u, 13u, 14u,
    4000000000u, 4000000002u, 4000000002u, 4000000005u,
};
static const uint32_t X_HALVE_SINGLES[] = {
    8u, 9u, 100u, 100u,
};
