// superplus_amd/csrc/dfk_adj_plan.h -- the plan of the adjacency stage's boundary k-mer set: how many keys the whole run
// will put into it, guessed from the parts that are finished, and how many slots it gets from what the arena has free.
// Host-only arithmetic over counts and the arena's free list, so it runs on a CPU (tests/cpp/test_adj_plan.cc).
//
// The set is an open-addressing table of 16-byte slots (SetSlot, dfk_kernels.h) that any slot count serves: a key's
// home is the high product of its hash and the slot count, a probe steps by one and wraps at the slot count.  So the set
// can be cut to the free block it has to live in -- which is what lets it be made while the last pass is still being
// counted, when most of the device is held -- as long as its load stays at or below ADJ_MAX_LOAD.
#pragma once
#include "dfk_arena.h"

namespace dfk {

constexpr uint64_t ADJ_SLOT_BYTES = 16;           // sizeof(SetSlot)
constexpr uint64_t ADJ_ALIGN = 256;               // the arena hands out multiples of this
constexpr uint64_t ADJ_LOAD_NUM = 3, ADJ_LOAD_DEN = 5;   // the highest load a set is used at: 0.6
constexpr double ADJ_MARGIN = 1.05;               // the guess of the run's keys is taken this much higher

// what became of the set started under the last pass's count (dfk_adj_outcome)
enum AdjOutcome : uint32_t {
    ADJ_NOT_APPLICABLE = 0,       // one pass, one stream, min_freq 1, a sharded run, or no finished part has a list
    ADJ_USED = 1,
    ADJ_DISCARDED_LOW = 2,        // the guess of the keys was too low: the final count would load the set past 0.6
    ADJ_DISCARDED_LIST = 3,       // a boundary list overflowed, or the lists' totals are not the run's
    ADJ_NO_BLOCK = 4,             // no free block holds a set at load <= 0.6
    ADJ_DROPPED_FOR_ALLOC = 5,    // the last pass needed the room
    ADJ_SWITCHED_OFF = 6,         // DFK_NO_EARLY_SET
};

// keys <= 0.6 * slots, in integers
inline bool adj_load_ok(uint64_t keys, uint64_t slots) { return slots && (unsigned __int128)keys * ADJ_LOAD_DEN <= (unsigned __int128)slots * ADJ_LOAD_NUM; }

// the fewest slots that hold `keys` at load <= 0.6
inline uint64_t adj_min_slots(uint64_t keys) { return (uint64_t)(((unsigned __int128)keys * ADJ_LOAD_DEN + ADJ_LOAD_NUM - 1) / ADJ_LOAD_NUM) + (keys ? 0 : 1); }

// the power of two the set was given before it could be cut to a block: at least 1024 slots, load <= 0.5
inline uint64_t adj_pow2_slots(uint64_t keys)
{
    uint32_t l = 10;
    while (l < 63 && (1ull << l) < 2 * keys + 2) ++l;
    return 1ull << l;
}

// The boundary keys of the whole run, from the lists of the parts that are finished: those parts cover `buckets_done` of
// the `sub_nb` fine buckets, buckets are hash-distributed, so the rest holds its share -- and a margin on top.
// `scale` is DFK_EARLY_SET_SCALE (tests force a guess that is too low with it).
inline uint64_t adj_estimate_keys(const std::vector<uint64_t>& n_blist, uint32_t sub_nb, uint32_t buckets_done, double scale = 1.0)
{
    uint64_t sum = 0;
    for (uint64_t n : n_blist) sum += n;
    if (!buckets_done || !sum) return 0;
    const double est = (double)sum * ((double)sub_nb / (double)buckets_done) * ADJ_MARGIN * scale;
    return est >= 1.8e19 ? ~0ull : (uint64_t)est + 1;
}

// Slots of a set for `keys` keys given the arena's free blocks and `room` (budget - held): the largest count that fits
// one block whole -- the arena rounds a request up to ADJ_ALIGN bytes, so the count is cut to a multiple of
// ADJ_ALIGN / ADJ_SLOT_BYTES -- and the room, no more than adj_pow2_slots(keys); 0 when that does not reach load <= 0.6.
// `*block` (if given) is the index of the block it fits, the largest one.
inline uint64_t adj_set_slots(uint64_t keys, const std::vector<Arena::Free>& blocks, uint64_t room, size_t* block = nullptr)
{
    size_t at = blocks.size(); uint64_t best = 0;
    for (size_t i = 0; i < blocks.size(); ++i) if (blocks[i].bytes > best) { best = blocks[i].bytes; at = i; }
    if (block) *block = at;
    const uint64_t bytes = std::min(best, room) & ~(ADJ_ALIGN - 1);
    const uint64_t slots = std::min(bytes / ADJ_SLOT_BYTES, adj_pow2_slots(keys));
    return adj_load_ok(keys, slots) ? slots : 0;
}

// a key's home slot and the probe step, as the kernels do them (set_home / set_next in dfk_kernels.h)
inline uint64_t adj_home(uint64_t hash, uint64_t slots) { return (uint64_t)(((unsigned __int128)hash * slots) >> 64); }
inline uint64_t adj_next(uint64_t s, uint64_t slots) { return s + 1 == slots ? 0 : s + 1; }

} // namespace dfk
