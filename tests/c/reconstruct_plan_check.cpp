// Stand-alone check of csrc/reconstruct_plan.h and of the index arithmetic the kernels of csrc/reconstruct.hip.h build on it, on the CPU
// (tests/test_reconstruct_plan.py builds it with AddressSanitizer and UndefinedBehaviorSanitizer and runs it as a child process).
//
// sim_locate restates recon_locate_kernel lane by lane -- workgroups striding over the work items, four waves, four rounds, the bound at
// list_len, the LDS filter or the exact bitmap, the binary search, the maximum of hit_key -- over id arrays that carry STALE slots behind
// every list's end, and is compared with the rule itself (last list, first position, live entries only).  sim_decode restates
// recon_decode_kernel's gather per component.  Every array is a std::vector of exactly the size the runtime allocates, so an index the
// arithmetic gets wrong is an AddressSanitizer report.
#include "../../ivfadc.jl_amd/csrc/reconstruct_plan.h"

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <unordered_map>
#include <vector>

using namespace recon;

static const int64_t CASE_LENS[] = {0, 1, 63, 64, 65, 255, 256, 257, 3, 17, 40, 100, 71};
static const int64_t MORE_LENS[] = {1023, 1024, 1025, 0, 0, 2049, 5, 4097, 0};

#define CHECK(cond)                                                                      \
    do {                                                                                 \
        if (!(cond)) {                                                                   \
            std::fprintf(stderr, "%s:%d: check failed: %s\n", __FILE__, __LINE__, #cond); \
            std::exit(1);                                                                \
        }                                                                                \
    } while (0)

struct Lists {
    std::vector<int64_t> len, cap, pos;   // pos: first id slot of a list
    std::vector<uint32_t> ids;            // every slot, stale ones included
};

// ids: distinct live ids drawn from `pool`, a few of them repeated within and across lists; every slot behind a list's end holds an id
// that is ALSO wanted (a stale row), so a read at or behind list_len shows as a wrong answer
static Lists make_lists(const int64_t *lens, size_t n, std::mt19937 &rng, const std::vector<uint32_t> &pool, size_t &used, uint32_t stale_id)
{
    Lists L;
    int64_t p = 0;
    for (size_t l = 0; l < n; ++l) {
        L.len.push_back(lens[l]);
        L.cap.push_back(lens[l] + std::max<int64_t>(32, lens[l] / 8));
        L.pos.push_back(p);
        p += L.cap.back();
    }
    L.ids.assign((size_t)p, stale_id);
    for (size_t l = 0; l < n; ++l)
        for (int64_t i = 0; i < L.len[l]; ++i) L.ids[(size_t)(L.pos[l] + i)] = pool[used++ % pool.size()];
    // repeats: within the first list of 40 or more points, and from it into the last such list
    std::vector<size_t> big;
    for (size_t l = 0; l < n; ++l)
        if (L.len[l] >= 40) big.push_back(l);
    if (big.size() >= 2) {
        const size_t a = big.front(), c = big.back();
        L.ids[(size_t)L.pos[a] + 30] = L.ids[(size_t)L.pos[a] + 5];
        L.ids[(size_t)L.pos[c] + 9] = L.ids[(size_t)L.pos[a] + 7];
        L.ids[(size_t)L.pos[c] + 20] = L.ids[(size_t)L.pos[a] + 7];
    }
    (void)rng;
    return L;
}

// the rule itself: lists ascending (later lists overwrite), and within a list only the first position of an id stands
static std::vector<uint64_t> brute(const Lists &L, const std::vector<uint32_t> &want)
{
    std::unordered_map<uint32_t, uint64_t> where;
    for (size_t l = 0; l < L.len.size(); ++l) {
        std::unordered_map<uint32_t, uint64_t> first;
        for (int64_t p = 0; p < L.len[l]; ++p) first.emplace(L.ids[(size_t)(L.pos[l] + p)], hit_key((uint32_t)l, (uint32_t)p));
        for (const auto &kv : first) where[kv.first] = kv.second;
    }
    std::vector<uint64_t> best(want.size(), 0);
    for (size_t s = 0; s < want.size(); ++s) {
        const auto it = where.find(want[s]);
        if (it != where.end()) best[s] = it->second;
    }
    return best;
}

// recon_locate_kernel, lane by lane
static void sim_locate(const Lists &L, const std::vector<uint64_t> &chunk_off, const std::vector<uint32_t> &want, bool hash, uint32_t lo,
                       uint64_t nbits, bool from_want, const std::vector<uint32_t> &bitmap, uint32_t grid, std::vector<uint64_t> &best,
                       uint64_t &reads)
{
    const uint64_t nwant = want.size();
    if (!hash && from_want) span_of(want.data(), nwant, lo, nbits);
    const uint32_t nlists = (uint32_t)L.len.size();
    const uint64_t items = chunk_off[nlists];
    std::vector<uint32_t> filt(hash ? FILTER_WORDS : 1, 0u);
    for (uint32_t block = 0; block < grid; ++block) {
        if (hash) {
            std::fill(filt.begin(), filt.end(), 0u);
            for (int tid = 0; tid < 256; ++tid)
                for (uint64_t i = (uint64_t)tid; i < nwant; i += 256) {
                    const uint32_t h = filter_hash(want.at((size_t)i));
                    filt.at(filter_word(h)) |= 1u << filter_bit(h);
                }
        }
        for (uint64_t item = block; item < items; item += grid) {
            const uint32_t l = item_list(chunk_off.data(), nlists, item);
            CHECK(l < nlists && chunk_off[l] <= item && item < chunk_off[l + 1]);
            const uint32_t chunk = (uint32_t)(item - chunk_off[l]);
            const uint32_t len = (uint32_t)L.len[l];
            for (int tid = 0; tid < 256; ++tid) {
                const int lane = tid & 63, wv = tid >> 6;
                for (int r = 0; r < subset::SUBSET_ROUNDS; ++r) {
                    const int64_t p = subset::subset_point(chunk, wv, r, lane);
                    if (p >= (int64_t)len) continue;
                    const uint32_t id = L.ids.at((size_t)(L.pos[l] + p));
                    ++reads;
                    bool maybe;
                    if (hash) {
                        const uint32_t h = filter_hash(id);
                        maybe = ((filt.at(filter_word(h)) >> filter_bit(h)) & 1u) != 0u;
                    } else {
                        maybe = bitmap_covers(lo, nbits, id) && ((bitmap.at((size_t)bitmap_word(lo, id)) >> bitmap_bit(lo, id)) & 1u) != 0u;
                    }
                    if (!maybe) continue;
                    const int64_t slot = slot_of(want.data(), 0, nwant, id);
                    if (slot >= 0) best.at((size_t)slot) = std::max(best.at((size_t)slot), hit_key(l, (uint32_t)p));
                }
            }
        }
    }
}

// recon_chunk_prefix_kernel, thread by thread, against the host's make_chunk_off
static std::vector<uint64_t> sim_chunk_prefix(const std::vector<int64_t> &len)
{
    const uint32_t nlists = (uint32_t)len.size();
    std::vector<uint64_t> off((size_t)nlists + 1, ~0ull), part(256, 0);
    uint32_t covered = 0;
    for (uint32_t t = 0; t < 256; ++t) {
        const uint32_t b = prefix_begin(nlists, 256, t), e = prefix_begin(nlists, 256, t + 1);
        CHECK(b == covered && e >= b && e <= nlists);
        covered = e;
        for (uint32_t l = b; l < e; ++l) part[t] += list_chunks((uint64_t)len.at(l));
    }
    CHECK(covered == nlists);
    uint64_t run = 0;
    for (int i = 0; i < 256; ++i) {
        const uint64_t v = part[(size_t)i];
        part[(size_t)i] = run;
        run += v;
    }
    off.at(nlists) = run;
    for (uint32_t t = 0; t < 256; ++t) {
        uint64_t r = part[t];
        for (uint32_t l = prefix_begin(nlists, 256, t); l < prefix_begin(nlists, 256, t + 1); ++l) {
            off.at(l) = r;
            r += list_chunks((uint64_t)len.at(l));
        }
    }
    CHECK(off == make_chunk_off(len));
    return off;
}

static uint64_t g_runs = 0, g_points = 0, g_bitmap_runs = 0, g_hash_runs = 0, g_full_space_runs = 0;
static std::vector<uint32_t> g_bitmap;   // the words of the span the kernels work on, and one stale word behind them

// one locate as the runtime drives it: plan, bitmap fill or LDS filter, and the comparison with the rule
static void run_locate(const Lists &L, std::vector<uint32_t> want, bool dedup, bool span_known, int num_cu)
{
    std::sort(want.begin(), want.end());
    if (dedup) want.erase(std::unique(want.begin(), want.end()), want.end());
    const std::vector<uint64_t> chunk_off = sim_chunk_prefix(L.len);
    uint64_t stored = 0;
    for (int64_t v : L.len) stored += (uint64_t)v;
    const Plan pl = make_plan(want.size(), span_known, want.empty() ? 0u : want.front(), want.empty() ? 0u : want.back(), chunk_off.back(), stored,
                              num_cu);
    std::vector<uint64_t> best(std::max<size_t>(1, want.size()), 0);
    uint64_t reads = 0;
    if (pl.mode == MODE_BITMAP) {
        CHECK(pl.nbits <= ID_SPACE_BITS && pl.words == bitmap_words(pl.nbits) && pl.grid >= 1 && pl.grid <= pl.items);
        CHECK(pl.nbits <= BITMAP_MAX_BITS || want.size() > FILTER_MAX_WANTED);
        CHECK(pl.span_from_want == !span_known);
        CHECK(span_known ? (pl.lo == want.front() && pl.nbits == (uint64_t)want.back() - want.front() + 1) : (pl.lo == 0 && pl.nbits == ID_SPACE_BITS));
        // the span the kernels work on: the plan's, or (device entries) the one they read from the wanted ids, within the plan's buffer
        uint32_t lo = pl.lo;
        uint64_t nbits = pl.nbits;
        if (pl.span_from_want) span_of(want.data(), want.size(), lo, nbits);
        CHECK(lo == want.front() && nbits == (uint64_t)want.back() - want.front() + 1 && bitmap_words(nbits) <= pl.words);
        // the buffer holds stale bits from earlier calls outside this span; the zero kernel (or the memset) clears the span's words
        g_bitmap.assign((size_t)bitmap_words(nbits) + 1, 0xFFFFFFFFu);
        for (uint64_t i = 0; i < bitmap_words(nbits); ++i) g_bitmap.at((size_t)i) = 0u;
        for (uint32_t id : want) {
            CHECK(bitmap_covers(lo, nbits, id) && bitmap_word(lo, id) < bitmap_words(nbits));
            g_bitmap.at((size_t)bitmap_word(lo, id)) |= 1u << bitmap_bit(lo, id);
        }
        sim_locate(L, chunk_off, want, false, pl.lo, pl.nbits, pl.span_from_want, g_bitmap, pl.grid, best, reads);
        CHECK(reads == stored);
        ++g_bitmap_runs;
        if (pl.nbits == ID_SPACE_BITS) ++g_full_space_runs;
    } else if (pl.mode == MODE_HASH) {
        CHECK(want.size() <= FILTER_MAX_WANTED && pl.grid >= 1 && pl.grid <= pl.items);
        CHECK(!span_known || (uint64_t)want.back() - want.front() + 1 > BITMAP_MAX_BITS);
        sim_locate(L, chunk_off, want, true, 0, 0, false, std::vector<uint32_t>(), pl.grid, best, reads);
        CHECK(reads == stored);
        ++g_hash_runs;
    } else {
        CHECK(want.empty() || chunk_off.back() == 0);
    }
    CHECK(pl.id_bytes == stored * 4);
    const std::vector<uint64_t> expect = brute(L, want);
    // (a repeated wanted id: the FIRST slot that holds it is the one a request reads; what a later slot holds is never read)
    for (size_t s = 0; s < want.size(); ++s)
        if (s == 0 || want[s] != want[s - 1]) CHECK(best[s] == expect[s]);
    // request order: every wanted id, and ids that are not wanted, find their slot again
    for (size_t s = 0; s < want.size(); ++s) {
        const int64_t slot = slot_of(want.data(), 0, want.size(), want[s]);
        CHECK(slot >= 0 && want[(size_t)slot] == want[s] && (slot == 0 || want[(size_t)slot - 1] != want[s]));
        const uint64_t key = best[(size_t)slot];
        CHECK(key_found(key) == (key != 0));
        if (key) {
            const int32_t l = key_list(key);
            const int64_t p = key_pos(key);
            CHECK(l >= 0 && (size_t)l < L.len.size() && p >= 0 && p < L.len[(size_t)l] && L.ids[(size_t)(L.pos[(size_t)l] + p)] == want[s]);
        } else {
            CHECK(key_list(key) == -1 && key_pos(key) == -1);
        }
    }
    ++g_runs;
    g_points += reads;
}

// recon_decode_kernel's gather for one stored row
static uint64_t sim_decode(int d, int m, int ksub, bool u16, std::mt19937 &rng)
{
    const int dsub = d / m, cb = u16 ? 2 * m : m, cs = (cb + 3) & ~3;
    std::vector<float> codebooks((size_t)m * ksub * dsub);
    for (size_t i = 0; i < codebooks.size(); ++i) codebooks[i] = (float)i;
    std::vector<uint8_t> labels((size_t)m * ksub), inv((size_t)m * 256, 0), row((size_t)cs, 0xEE);
    std::vector<uint32_t> c((size_t)m);
    for (int ii = 0; ii < m; ++ii) {
        std::vector<int> perm(u16 ? ksub : 256);
        for (size_t i = 0; i < perm.size(); ++i) perm[i] = (int)i;
        std::shuffle(perm.begin(), perm.end(), rng);
        c[(size_t)ii] = (uint32_t)(rng() % (uint32_t)ksub);
        if (u16) {
            row.at((size_t)2 * ii) = (uint8_t)(c[(size_t)ii] & 0xFF);
            row.at((size_t)2 * ii + 1) = (uint8_t)(c[(size_t)ii] >> 8);
        } else {
            for (int k = 0; k < ksub; ++k) {
                labels[(size_t)ii * ksub + k] = (uint8_t)perm[(size_t)k];
                inv.at(label_slot((uint32_t)ii, (uint32_t)perm[(size_t)k])) = (uint8_t)k;
            }
            row.at((size_t)ii) = labels[(size_t)ii * ksub + c[(size_t)ii]];
        }
    }
    uint64_t n = 0;
    for (int t0 = 0; t0 < 256; ++t0)            // the lanes of the workgroup
        for (int t = t0; t < d; t += 256) {
            const uint32_t ii = decode_block((uint32_t)t, (uint32_t)dsub);
            CHECK(ii < (uint32_t)m);
            uint32_t cw;
            if (u16) cw = (uint32_t)row.at((size_t)2 * ii) | ((uint32_t)row.at((size_t)2 * ii + 1) << 8);
            else cw = inv.at(label_slot(ii, row.at(ii)));
            CHECK(cw == c[ii]);
            const uint64_t e = codeword_elem(ii, cw, (uint32_t)t, (uint32_t)dsub, (uint32_t)ksub);
            CHECK(codebooks.at((size_t)e) == (float)(((size_t)ii * ksub + cw) * dsub + ((size_t)t - (size_t)ii * dsub)));
            ++n;
        }
    CHECK(n == (uint64_t)d);
    return n;
}

int main()
{
    std::mt19937 rng(20240611u);
    // ---- the pool of ids: both halves of the unsigned range, its ends included
    std::vector<uint32_t> pool = {0xFFFFFFFFu, 0xFFFFFFFEu, 0x80000000u, 0x80000001u, 0x7FFFFFFFu, 0u};
    for (uint32_t i = 0; i < 20000; ++i) pool.push_back(i % 3 == 0 ? 0x80000002u + 7u * i : 1u + 5u * i);
    const uint32_t STALE = 0x12345677u;   // in no list's live part
    CHECK(std::find(pool.begin(), pool.end(), STALE) == pool.end());

    size_t used = 0;
    std::vector<Lists> all;
    all.push_back(make_lists(CASE_LENS, sizeof CASE_LENS / sizeof *CASE_LENS, rng, pool, used, STALE));
    all.push_back(make_lists(MORE_LENS, sizeof MORE_LENS / sizeof *MORE_LENS, rng, pool, used, STALE));
    const int64_t none[] = {0, 0, 0};
    all.push_back(make_lists(none, 3, rng, pool, used, STALE));

    // ---- wanted-set sizes: small ones, and both sides of the LDS filter's cap (behind it: the bitmap, over the whole id space if need be)
    const size_t sizes[] = {1, 2, 64, 65, 1000, FILTER_MAX_WANTED - 1, FILTER_MAX_WANTED, FILTER_MAX_WANTED + 1, 2 * FILTER_MAX_WANTED, 2 * FILTER_MAX_WANTED + 1};
    int lengths = 0;
    for (const Lists &L : all) {
        lengths += (int)L.len.size();
        for (size_t sz : sizes) {
            // stored ids, the stale id, absent ids; not sorted, with repeats
            std::vector<uint32_t> want;
            want.push_back(STALE);
            for (size_t i = 0; want.size() < sz; ++i) want.push_back(i % 4 == 3 ? 0x40000000u + (uint32_t)i : pool[(i * 7) % pool.size()]);
            want.resize(sz);
            const bool big = sz >= FILTER_MAX_WANTED - 1;
            run_locate(L, want, true, true, 256);    // host entry: unique, span known (the pool spans the whole range: hashed)
            run_locate(L, want, false, false, 256);  // device entry: repeats stay, span unknown
            if (!big) run_locate(L, want, true, true, 1);      // one compute unit: the grid strides
            // a narrow span: the exact bitmap
            std::vector<uint32_t> narrow;
            for (uint32_t id : want)
                if (id >= 1u && id < 1u + 5u * 20000u) narrow.push_back(id);
            narrow.push_back(1u + 5u * 3u);
            run_locate(L, narrow, true, true, 256);
            if (!big) run_locate(L, narrow, true, true, 1);
        }
        run_locate(L, std::vector<uint32_t>(), true, true, 256);   // nothing wanted
    }

    // ---- plan cases: the bitmap's boundary, SIFT1B-sized counts
    uint64_t plans = 0;
    {
        const uint64_t items = 1000000, stored = 1000000000ull;
        Plan p = make_plan(163840, true, 0u, (uint32_t)(BITMAP_MAX_BITS - 1), items, stored, 256);
        CHECK(p.mode == MODE_BITMAP && p.nbits == BITMAP_MAX_BITS && p.words == BITMAP_MAX_BITS / 32 && p.grid == 256 * GRID_WG_PER_CU_BITMAP);
        p = make_plan(163840, true, 0u, (uint32_t)BITMAP_MAX_BITS, items, stored, 256);
        CHECK(p.mode == MODE_BITMAP && p.nbits == BITMAP_MAX_BITS + 1 && p.id_bytes == 4000000000ull);   // beyond the LDS filter's cap
        p = make_plan(FILTER_MAX_WANTED, true, 0u, (uint32_t)BITMAP_MAX_BITS, items, stored, 256);
        CHECK(p.mode == MODE_HASH && p.grid == 256 * GRID_WG_PER_CU_HASH);
        p = make_plan(FILTER_MAX_WANTED + 1, true, 0u, (uint32_t)BITMAP_MAX_BITS, items, stored, 256);
        CHECK(p.mode == MODE_BITMAP);
        p = make_plan(163840, false, 0u, 0u, items, stored, 256);
        CHECK(p.mode == MODE_BITMAP && p.lo == 0 && p.nbits == ID_SPACE_BITS && p.words == ID_SPACE_BITS / 32);
        p = make_plan(FILTER_MAX_WANTED, false, 0u, 0u, items, stored, 256);
        CHECK(p.mode == MODE_HASH);
        p = make_plan(1, true, 0xFFFFFFFFu, 0xFFFFFFFFu, items, stored, 256);
        CHECK(p.mode == MODE_BITMAP && p.lo == 0xFFFFFFFFu && p.nbits == 1 && p.words == 1);
        p = make_plan(2, true, 0u, 0xFFFFFFFFu, items, stored, 256);
        CHECK(p.mode == MODE_HASH);
        p = make_plan(1024, true, 5u, 1000000004u, 3, 2500, 256);
        CHECK(p.mode == MODE_BITMAP && p.grid == 3);
        p = make_plan(0x7FFFFFFFull, false, 0u, 0u, items, stored, 256);
        CHECK(p.mode == MODE_BITMAP && p.nbits == ID_SPACE_BITS && bitmap_covers(p.lo, p.nbits, 0xFFFFFFFFu) &&
              bitmap_word(p.lo, 0xFFFFFFFFu) == p.words - 1 && bitmap_bit(p.lo, 0xFFFFFFFFu) == 31);
        plans += 10;
        // a billion points over 2^20 lists, one list of nearly 2^32 points among them
        std::vector<int64_t> len((size_t)1 << 20, 953);
        len[12345] = 0;
        len[777] = 0xFFFFFFFEll;
        const std::vector<uint64_t> off = sim_chunk_prefix(len);
        CHECK(off.back() == ((uint64_t)len.size() - 2) * 1 + list_chunks(0xFFFFFFFEull));
        for (uint64_t item = 0; item < off.back(); item += 9973) {
            const uint32_t l = item_list(off.data(), (uint32_t)len.size(), item);
            CHECK(off[l] <= item && item < off[l + 1] && len[l] > 0);
            const uint32_t chunk = (uint32_t)(item - off[l]);
            CHECK((int64_t)chunk * subset::SUBSET_CHUNK < len[l]);
            CHECK(subset::subset_point(chunk, 3, subset::SUBSET_ROUNDS - 1, 63) == (int64_t)chunk * subset::SUBSET_CHUNK + 1023);
            ++plans;
        }
        CHECK(item_list(off.data(), (uint32_t)len.size(), off.back() - 1) == (uint32_t)len.size() - 1);
        CHECK(item_list(off.data(), (uint32_t)len.size(), 0) == 0);
        // keys at the ends of their fields; the code row of the last point of a 12 GB code buffer
        CHECK(key_list(hit_key(0x7FFFFFFFu, 0xFFFFFFFEu)) == 0x7FFFFFFF && key_pos(hit_key(0x7FFFFFFFu, 0xFFFFFFFEu)) == 0xFFFFFFFEll);
        CHECK(hit_key(0, 0xFFFFFFFEu) != 0 && key_list(hit_key(0, 0)) == 0 && key_pos(hit_key(0, 0)) == 0);
        CHECK(hit_key(5, 0) > hit_key(4, 0) && hit_key(5, 0) > hit_key(5, 1) && hit_key(5, 0xFFFFFFFEu) > hit_key(4, 0));
        CHECK(code_row(12000000000ull, 0xFFFFFFFEull, 8) == 12000000000ull + 8ull * 0xFFFFFFFEull);
        plans += 6;
    }

    // ---- decode shapes: code strides 8 and 4, dsub no multiple of 4, d no multiple of 64, d beyond one workgroup's lanes, both widths
    const int shapes[][3] = {{24, 8, 256}, {24, 3, 256}, {50, 10, 256}, {24, 8, 200}, {128, 8, 256}, {960, 48, 256}, {130, 1, 7}, {7, 7, 1}};
    uint64_t decodes = 0;
    for (const auto &s : shapes) {
        sim_decode(s[0], s[1], s[2], false, rng);
        sim_decode(s[0], s[1], s[2] == 256 ? 300 : s[2], true, rng);
        decodes += 2;
    }
    sim_decode(24, 3, 65536, true, rng);
    ++decodes;

    CHECK(g_bitmap_runs > 20 && g_hash_runs > 20 && g_full_space_runs > 5);
    std::printf("reconstruct_plan_check ok: %llu simulated locates over %d lengths, %llu ids read, %llu plan cases, %llu decode shapes\n",
                (unsigned long long)g_runs, lengths, (unsigned long long)g_points, (unsigned long long)plans, (unsigned long long)decodes);
    return 0;
}
