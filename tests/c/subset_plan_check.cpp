// Stand-alone check of csrc/subset_plan.h (tests/test_subset_plan.py builds it with -fsanitize=address,undefined and runs it).
//
// The host planner (make_items, make_bases) and a plain-C++ restatement of the two kernels of csrc/subset.hip.h -- the same work items,
// the same subset_point / subset_selected, a wave's ballot and popcount spelled out lane by lane -- are run over the case table of
// tests/subset.py (its list lengths, its masks, both choices of nbits, every code stride in dwords) and compared with a brute-force
// filter.  Every destination is written through a bounds-checked index into buffers of exactly the planned size, so an index that
// leaves its list is reported here (and by the sanitizer) instead of on a device.  Exit status 0: everything agrees.
#include "../../ivfadc.jl_amd/csrc/subset_plan.h"

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <numeric>

using namespace subset;

namespace {

uint64_t g_rng = 0x9E3779B97F4A7C15ull;
uint32_t rnd()
{
    g_rng ^= g_rng << 13; g_rng ^= g_rng >> 7; g_rng ^= g_rng << 17;
    return (uint32_t)(g_rng >> 32);
}

struct Lists {
    std::vector<int64_t> len, pos;      // per list: length, offset of its first entry
    std::vector<uint32_t> ids, codes;   // ids[n], codes[n * nw]
    int nw;
};

Lists make_lists(int nw)
{
    const int64_t C = SUBSET_CHUNK;
    const int64_t one[12] = {0, 1, 63, 64, 65, 255, 256, 257, C - 1, C, C + 1, 2 * C + 1};
    Lists L;
    L.nw = nw;
    for (int i = 0; i < 12; ++i) L.len.push_back(one[i]);
    for (int i = 11; i >= 0; --i) L.len.push_back(one[i]);
    int64_t n = 0;
    for (int64_t v : L.len) { L.pos.push_back(n); n += v; }
    L.ids.resize((size_t)n);
    std::iota(L.ids.begin(), L.ids.end(), 0u);
    for (size_t i = L.ids.size(); i > 1; --i) std::swap(L.ids[i - 1], L.ids[rnd() % i]);
    L.codes.resize((size_t)n * nw);
    for (uint32_t &c : L.codes) c = rnd();
    return L;
}

// the masks of tests/subset.py, per list position -> a bitmap over ids
std::vector<uint32_t> make_bits(const Lists &L, int kind, uint64_t nbits_all)
{
    const int64_t C = SUBSET_CHUNK;
    std::vector<uint32_t> bits((size_t)((nbits_all + 31) / 32), 0u);
    for (size_t l = 0; l < L.len.size(); ++l)
        for (int64_t p = 0; p < L.len[l]; ++p) {
            bool on = false;
            switch (kind) {
            case 0: on = true; break;
            case 1: on = false; break;
            case 2: on = (p & 1) == 0; break;
            case 3: on = p == 0; break;
            case 4: on = p == L.len[l] - 1; break;
            case 5: on = p >= C - 50 && p < C + 50; break;
            case 6: on = (rnd() & 1) != 0; break;
            default: on = rnd() % 100 == 0; break;
            }
            const uint32_t id = L.ids[(size_t)(L.pos[l] + p)];
            if (on) bits[id >> 5] |= 1u << (id & 31);
        }
    return bits;
}

int fails = 0;
#define EXPECT(cond, ...)                                      \
    do {                                                       \
        if (!(cond)) {                                         \
            if (fails++ < 20) { fprintf(stderr, __VA_ARGS__); fputc('\n', stderr); } \
        }                                                      \
    } while (0)

// the keep bits of one wave's share of an item, as subset_wave_masks computes them
uint32_t wave_masks(const Lists &L, const Item it, int wv, const uint32_t *bits, uint64_t nbits, uint64_t (&mask)[SUBSET_ROUNDS])
{
    uint32_t total = 0;
    for (int r = 0; r < SUBSET_ROUNDS; ++r) {
        mask[r] = 0;
        for (int lane = 0; lane < 64; ++lane) {
            const int64_t p = subset_point(it.chunk, wv, r, lane);
            if (p < L.len[it.list] && subset_selected(bits, nbits, L.ids[(size_t)(L.pos[it.list] + p)])) mask[r] |= 1ull << lane;
        }
        total += (uint32_t)__builtin_popcountll(mask[r]);
    }
    return total;
}

void run_case(int nw, int kind, bool half)
{
    const Lists L = make_lists(nw);
    const uint64_t top = L.ids.empty() ? 0 : *std::max_element(L.ids.begin(), L.ids.end());
    const std::vector<uint32_t> bits = make_bits(L, kind, top + 1);
    const uint64_t nbits = half ? top / 2 : top + 1;      // the words behind nbits stay in the array: they must not be looked at

    // planner: items cover every point of every list once, in order
    const std::vector<Item> items = make_items(L.len);
    {
        size_t i = 0;
        for (size_t l = 0; l < L.len.size(); ++l)
            for (int64_t c = 0; c * SUBSET_CHUNK < L.len[l]; ++c, ++i)
                EXPECT(i < items.size() && items[i].list == l && items[i].chunk == (uint32_t)c, "item %zu is not (list %zu, chunk %lld)", i, l, (long long)c);
        EXPECT(i == items.size(), "%zu items, expected %zu", items.size(), i);
    }
    // count pass
    std::vector<uint32_t> count(items.size(), 0);
    for (size_t i = 0; i < items.size(); ++i)
        for (int wv = 0; wv < 4; ++wv) {
            uint64_t mask[SUBSET_ROUNDS];
            count[i] += wave_masks(L, items[i], wv, bits.data(), nbits, mask);
        }
    std::vector<int64_t> kept;
    std::vector<uint32_t> base;
    make_bases(items, count, L.len.size(), kept, base);

    // brute force
    std::vector<int64_t> exp_len(L.len.size(), 0);
    std::vector<uint32_t> exp_ids, exp_codes;
    for (size_t l = 0; l < L.len.size(); ++l)
        for (int64_t p = 0; p < L.len[l]; ++p) {
            const uint32_t id = L.ids[(size_t)(L.pos[l] + p)];
            if ((uint64_t)id < nbits && ((bits[id / 32] >> (id % 32)) & 1u)) {
                ++exp_len[l];
                exp_ids.push_back(id);
                for (int w = 0; w < nw; ++w) exp_codes.push_back(L.codes[(size_t)(L.pos[l] + p) * nw + w]);
            }
        }
    EXPECT(kept == exp_len, "kind %d nw %d half %d: per-list totals differ", kind, nw, (int)half);
    if (kept != exp_len) return;

    // scatter pass into buffers of exactly the planned size
    std::vector<int64_t> dpos(kept.size(), 0);
    int64_t n = 0;
    for (size_t l = 0; l < kept.size(); ++l) { dpos[l] = n; n += kept[l]; }
    const uint32_t POISON = 0xDEADBEEFu;
    std::vector<uint32_t> out_ids((size_t)n, POISON), out_codes((size_t)n * nw, POISON);
    std::vector<uint8_t> written((size_t)n, 0);
    for (size_t i = 0; i < items.size(); ++i) {
        const Item it = items[i];
        uint64_t mask[4][SUBSET_ROUNDS];
        uint32_t s_wave[4];
        for (int wv = 0; wv < 4; ++wv) s_wave[wv] = wave_masks(L, it, wv, bits.data(), nbits, mask[wv]);
        for (int wv = 0; wv < 4; ++wv) {
            uint32_t run = base[i];
            for (int v = 0; v < wv; ++v) run += s_wave[v];
            for (int r = 0; r < SUBSET_ROUNDS; ++r) {
                for (int lane = 0; lane < 64; ++lane)
                    if ((mask[wv][r] >> lane) & 1ull) {
                        const int64_t p = subset_point(it.chunk, wv, r, lane);
                        const uint32_t dst = run + (uint32_t)__builtin_popcountll(mask[wv][r] & ((1ull << lane) - 1ull));
                        EXPECT((int64_t)dst < kept[it.list], "destination %u outside list %u of %lld", dst, it.list, (long long)kept[it.list]);
                        if ((int64_t)dst >= kept[it.list]) continue;
                        const size_t o = (size_t)(dpos[it.list] + dst);
                        EXPECT(!written.at(o), "slot %zu written twice", o);
                        written.at(o) = 1;
                        out_ids.at(o) = L.ids[(size_t)(L.pos[it.list] + p)];
                        for (int w = 0; w < nw; ++w) out_codes.at(o * nw + w) = L.codes[(size_t)(L.pos[it.list] + p) * nw + w];
                    }
                run += (uint32_t)__builtin_popcountll(mask[wv][r]);
            }
        }
    }
    EXPECT(out_ids == exp_ids, "kind %d nw %d half %d: ids differ from the brute-force filter", kind, nw, (int)half);
    EXPECT(out_codes == exp_codes, "kind %d nw %d half %d: code rows differ from the brute-force filter", kind, nw, (int)half);
}

}  // namespace

int main()
{
    // the bit test at its edges: the last bit below nbits, the first at it, word boundaries
    {
        const uint32_t w[3] = {0x80000001u, 0x80000001u, 0xFFFFFFFFu};
        EXPECT(subset_selected(w, 64, 0) && subset_selected(w, 64, 31) && subset_selected(w, 64, 32) && subset_selected(w, 64, 63), "set bits");
        EXPECT(!subset_selected(w, 64, 1) && !subset_selected(w, 64, 30) && !subset_selected(w, 64, 33), "clear bits");
        EXPECT(!subset_selected(w, 64, 64) && !subset_selected(w, 63, 63) && subset_selected(w, 65, 64), "nbits is exclusive");
        EXPECT(!subset_selected(nullptr, 0, 0) && !subset_selected(nullptr, 0, 0xFFFFFFFFu), "nbits == 0 selects nothing and reads nothing");
    }
    // subset_point covers a chunk exactly once, in order of (wave, round, lane)
    {
        int64_t next = 3 * (int64_t)SUBSET_CHUNK;
        for (int wv = 0; wv < 4; ++wv)
            for (int r = 0; r < SUBSET_ROUNDS; ++r)
                for (int lane = 0; lane < 64; ++lane, ++next) EXPECT(subset_point(3, wv, r, lane) == next, "subset_point(3, %d, %d, %d)", wv, r, lane);
        EXPECT(next == 4 * (int64_t)SUBSET_CHUNK, "a chunk is four waves of SUBSET_ROUNDS rounds");
        EXPECT(subset_point(0xFFFFFFFFu / SUBSET_CHUNK, 3, SUBSET_ROUNDS - 1, 63) == (int64_t)(0xFFFFFFFFu / SUBSET_CHUNK) * SUBSET_CHUNK + SUBSET_CHUNK - 1,
               "positions near 2^32 do not wrap");
    }
    const int strides[] = {1, 2, 3, 4, 12};   // dwords per code row: cs = 4, 8, 12, 16, 48
    for (int nw : strides)
        for (int kind = 0; kind < 8; ++kind)
            for (int half = 0; half < 2; ++half) run_case(nw, kind, half != 0);
    if (fails) {
        fprintf(stderr, "subset_plan_check: %d failures\n", fails);
        return 1;
    }
    printf("subset_plan_check ok: SUBSET_CHUNK %d, %d cases\n", SUBSET_CHUNK, 5 * 8 * 2);
    return 0;
}
