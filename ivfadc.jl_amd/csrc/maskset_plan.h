// Layout and bit addressing of a mask set (ivfadc_maskset_create; maskset.hip.h holds the kernels).  Plain C++ (no HIP types), in the
// manner of subset_plan.h, so that the layout and the arithmetic the kernels share with it compile and run without a GPU
// (tests/c/maskset_plan_check.cpp).
//
// A mask set is nmasks bitmaps over STORED ids (the bit definition of ivfadc_clone_subset: subset::subset_selected), converted once into
// SLOT space: one bit per stored entry, in list order.  The row of list l holds 2 * ceil(len_l / 64) words -- whole 64-point wave rounds,
// so a wave writes and reads the bits of its 64 consecutive points as two whole words, with plain vector stores, no atomics, and no word
// shared between two lists.  word_off[l] is the exclusive prefix of the row lengths, W their total; mask r of list l starts at word
// r * W + word_off[l].  Position p of a list is bit (p & 31) of word p >> 5 of the row; the bits behind list_len are 0.
#pragma once

#include <cstddef>
#include <cstdint>
#include <vector>

#if defined(__HIPCC__)
#define MASKSET_HD __host__ __device__ __forceinline__
#else
#define MASKSET_HD inline
#endif

namespace maskset {

constexpr int ROUND = 64;             // points per wave round
constexpr int ROUND_WORDS = 2;        // ... and their words

// words of the row of a list of `len` points (64-bit: a list may hold nearly 2^32 points)
MASKSET_HD uint64_t row_words(uint64_t len) { return (uint64_t)ROUND_WORDS * ((len + (uint64_t)ROUND - 1) / (uint64_t)ROUND); }

// the one definition of "word and bit of position p" within a list's row (build kernel, scan kernel, generic path, CPU check)
MASKSET_HD uint64_t word_of(uint64_t p) { return p >> 5; }
MASKSET_HD uint32_t bit_of(uint64_t p) { return (uint32_t)(p & 31u); }
// first word of the round that holds position p (p a multiple of ROUND for a wave's first lane)
MASKSET_HD uint64_t round_word(uint64_t p) { return (p / (uint64_t)ROUND) * (uint64_t)ROUND_WORDS; }

// first word of mask r's row of the list whose row starts at word_off_l
MASKSET_HD uint64_t row_start(uint64_t W, uint64_t word_off_l, uint32_t r) { return (uint64_t)r * W + word_off_l; }

// position p of the list whose row is `row` is selected
MASKSET_HD bool slot_selected(const uint32_t *row, uint64_t p) { return ((row[word_of(p)] >> bit_of(p)) & 1u) != 0u; }

// the 64 bits of a round from its two words: lane i of the round is bit i
MASKSET_HD uint64_t round_bits(uint32_t lo, uint32_t hi) { return (uint64_t)lo | ((uint64_t)hi << 32); }

struct Layout {
    std::vector<uint64_t> word_off;   // [nlists + 1]: exclusive prefix of row_words; word_off[nlists] == W
    uint64_t W = 0;                   // words of one mask
};

inline Layout make_layout(const std::vector<int64_t> &len)
{
    Layout L;
    L.word_off.assign(len.size() + 1, 0);
    for (size_t l = 0; l < len.size(); ++l) L.word_off[l + 1] = L.word_off[l] + row_words((uint64_t)(len[l] > 0 ? len[l] : 0));
    L.W = L.word_off[len.size()];
    return L;
}

// mask_of_query as the device entry ingests it: into [-1, nmasks)
MASKSET_HD int32_t clamp_mask(int32_t v, int32_t nmasks) { return v < -1 ? -1 : (v >= nmasks ? nmasks - 1 : v); }

}  // namespace maskset
