// Host planner of ivfadc_clone_subset (subset.hip.h holds the two kernels).  Plain C++ (no HIP types), so that the planner and the index
// arithmetic it shares with the kernels compile and run without a GPU (tests/c/subset_plan_check.cpp).
//
// A subset is chosen by a bitmap over STORED ids: id i is selected iff i < nbits and bit (i & 31) of word bits[i >> 5] is set.  The
// lists are cut into work items (list, chunk of SUBSET_CHUNK points); a count pass leaves one number per item, the functions below turn
// the numbers into per-list totals and per-item destinations, and a scatter pass writes every kept entry to
//     (item's base within its new list) + (kept entries before it in the item),
// which keeps the stored order (a stable compaction, deleteat! of utils.jl:98-99 without _shift_inverse_index!).
#pragma once

#include <cstddef>
#include <cstdint>
#include <vector>

#if defined(__HIPCC__)
#define SUBSET_HD __host__ __device__ __forceinline__
#else
#define SUBSET_HD inline
#endif

namespace subset {

// points per work item: one workgroup of four waves, each wave SUBSET_WAVE_POINTS consecutive points in rounds of 64
constexpr int SUBSET_CHUNK = 1024;
constexpr int SUBSET_WAVE_POINTS = SUBSET_CHUNK / 4;
constexpr int SUBSET_ROUNDS = SUBSET_WAVE_POINTS / 64;
static_assert(SUBSET_CHUNK % 256 == 0, "a wave's share is a whole number of 64-point rounds");

// the one definition of "selected" (count kernel, scatter kernel, CPU check)
SUBSET_HD bool subset_selected(const uint32_t *bits, uint64_t nbits, uint32_t id)
{
    return (uint64_t)id < nbits && ((bits[id >> 5] >> (id & 31u)) & 1u) != 0u;
}

// position within its list of the point that lane `lane` of wave `wave` reads in round `round` of chunk `chunk`
// (a position fits 32 bits; the sum is formed in 64 so that the lanes behind the end of a list of nearly 2^32 points do not wrap into it)
SUBSET_HD int64_t subset_point(uint32_t chunk, int wave, int round, int lane)
{
    return (int64_t)chunk * SUBSET_CHUNK + (wave * SUBSET_WAVE_POINTS + round * 64 + lane);
}

struct Item {
    uint32_t list, chunk;   // points [chunk * SUBSET_CHUNK, min(len, (chunk + 1) * SUBSET_CHUNK)) of list `list`
};

// every non-empty chunk of every list, lists ascending, chunks ascending within a list
inline std::vector<Item> make_items(const std::vector<int64_t> &len)
{
    std::vector<Item> items;
    for (size_t l = 0; l < len.size(); ++l)
        for (int64_t c = 0; c * SUBSET_CHUNK < len[l]; ++c) items.push_back(Item{(uint32_t)l, (uint32_t)c});
    return items;
}

// item counts -> kept points per list (kept, sized like the lists) and every item's exclusive base within its new list
inline void make_bases(const std::vector<Item> &items, const std::vector<uint32_t> &count, size_t nlists, std::vector<int64_t> &kept,
                       std::vector<uint32_t> &base)
{
    kept.assign(nlists, 0);
    base.assign(items.size(), 0);
    for (size_t i = 0; i < items.size(); ++i) {
        base[i] = (uint32_t)kept[items[i].list];
        kept[items[i].list] += count[i];
    }
}

}  // namespace subset
