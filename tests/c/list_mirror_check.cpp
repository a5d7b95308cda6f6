// Stand-alone check of csrc/list_mirror.h (tests/test_list_mirror.py builds it with -fsanitize=address,undefined and runs it directly).
//
// 1. The mirror against a naive model: ONE flat vector of (list, id, code row) in insertion order, which knows nothing of per-list vectors,
//    lengths or totals.  Seeded random chains of assign / append / erase / shift / layout drive both, for kc = 1, 2, 7 and cb = 1, 3, 8, 16
//    (16: 8 x uint16); after every step the gathered state (offsets, codes, ids), h_len, n, maxlen and ntotal are compared in full.  The
//    chains hold empty lists and the empty index, appends of 0 and 1 points, erases of nothing present, of everything and of unsorted
//    requests with duplicates, shifts that wrap uint32, and the two-step erase (after find_ids alone the mirror is byte-identical).
// 2. The in-place decision and the destination pairs of append against the model's own layout (prefix sums restated here), with an append
//    that exactly fills a list's capacity and one that overflows it by one; stage() against the same layout.
// 3. layout_from_caps and check_offsets at the 2^32 refusals, on lengths alone (nothing is allocated from them).
// 4. The label map: identity, permuted and sparse labels, ksub = 2 and 257, round trips, and one non-label code at the first, a middle and
//    the last position with a second offender behind it: the reported point / codebook / value are the first offender's.
#include "../../ivfadc.jl_amd/csrc/list_mirror.h"

#include <cstdio>
#include <cstdlib>
#include <random>

using namespace list_mirror;

static int g_fail = 0;
#define CHECK(c)                                                              \
    do {                                                                      \
        if (!(c)) {                                                           \
            fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #c); \
            if (++g_fail > 20) exit(1);                                       \
        }                                                                     \
    } while (0)

struct Row {
    int list;
    uint32_t id;
    std::vector<uint8_t> code;
};

struct Model {
    int kc, cb, cs;
    std::vector<Row> rows;                  // insertion order
    bool current = false;                   // a device layout stands and no edit has outgrown it
    std::vector<int64_t> cap, pos, codeoff;
    int64_t len(int l) const
    {
        int64_t c = 0;
        for (const Row &r : rows) c += r.list == l;
        return c;
    }
    void layout(const std::vector<int64_t> &caps)
    {
        cap = caps;
        pos.assign(kc, 0);
        codeoff.assign(kc, 0);
        int64_t p = 0, o = 0;
        for (int l = 0; l < kc; ++l) {
            pos[l] = p;
            codeoff[l] = o;
            p += cap[l];
            o += (cap[l] * cs + 255) / 256 * 256;
        }
        current = true;
    }
};

static long long g_steps = 0, g_appends = 0, g_inplace = 0, g_erases = 0, g_erased = 0, g_layouts = 0;

static void compare(const Model &m, const ListMirror &mir)
{
    ++g_steps;
    std::vector<int64_t> off(m.kc + 1, -1), woff(m.kc + 1, 0);
    std::vector<uint8_t> codes(m.rows.size() * m.cb + 1, 0xEE), wcodes;
    std::vector<uint32_t> ids(m.rows.size() + 1, 0xEEEEEEEEu), wids;
    mir.gather(off.data(), codes.data(), ids.data(), m.cb);
    int64_t maxlen = 0;
    for (int l = 0; l < m.kc; ++l) {
        for (const Row &r : m.rows)
            if (r.list == l) {
                wids.push_back(r.id);
                wcodes.insert(wcodes.end(), r.code.begin(), r.code.end());
            }
        woff[l + 1] = (int64_t)wids.size();
        CHECK(mir.h_len[l] == woff[l + 1] - woff[l]);
        CHECK((int64_t)mir.hl_ids[l].size() == mir.h_len[l] && (int64_t)mir.hl_codes[l].size() == mir.h_len[l] * m.cb);
        maxlen = std::max(maxlen, mir.h_len[l]);
    }
    CHECK(off == woff);
    codes.resize(wcodes.size());
    ids.resize(wids.size());
    CHECK(codes == wcodes && ids == wids);
    CHECK(mir.n == (int64_t)m.rows.size() && mir.ntotal() == mir.n && mir.maxlen == maxlen);
    mir.gather(nullptr, nullptr, nullptr, m.cb);   // every output is optional
}

static std::vector<uint8_t> random_codes(std::mt19937 &rng, size_t bytes)
{
    std::vector<uint8_t> c(bytes);
    for (uint8_t &b : c) b = (uint8_t)rng();
    return c;
}

// the device layout: d_cap as given, then the mirror's own arithmetic and stage() against the model's
static void do_layout(Model &m, const ListMirror &mir, DeviceLayout &lay, const std::vector<int64_t> &caps)
{
    ++g_layouts;
    lay.d_cap = caps;
    LayoutTotals tot;
    CHECK(!layout_from_caps(lay, mir.h_len, m.cs, tot));
    m.layout(caps);
    CHECK(lay.d_pos == m.pos && lay.d_codeoff == m.codeoff);
    int64_t slots = 0;
    for (int64_t c : caps) slots += c;
    CHECK(tot.id_slots == slots && tot.n == mir.n && tot.maxlen == mir.maxlen);
    CHECK(tot.code_bytes == (size_t)(m.codeoff[m.kc - 1] + (caps[m.kc - 1] * m.cs + 255) / 256 * 256) + CODE_SLACK);
    std::vector<uint8_t> codes, want;
    std::vector<uint32_t> ids, wids;
    mir.stage(lay, tot, m.cb, m.cs, codes, ids);
    want.assign(tot.code_bytes, 0);
    wids.assign((size_t)std::max<int64_t>(1, slots), 0);
    std::vector<int64_t> at(m.kc, 0);
    for (const Row &r : m.rows) {
        memcpy(want.data() + m.codeoff[r.list] + at[r.list] * m.cs, r.code.data(), (size_t)m.cb);
        wids[(size_t)(m.pos[r.list] + at[r.list]++)] = r.id;
    }
    CHECK(codes == want && ids == wids);
}

static void do_append(Model &m, ListMirror &mir, const DeviceLayout &lay, std::mt19937 &rng, const std::vector<int32_t> &lst, uint32_t &next_id)
{
    ++g_appends;
    const int64_t nnew = (int64_t)lst.size();
    const std::vector<uint8_t> cod = random_codes(rng, (size_t)nnew * m.cb);
    std::vector<uint32_t> ids((size_t)nnew);
    for (uint32_t &v : ids) v = (rng() % 4 == 0) ? (uint32_t)rng() : next_id++;
    // the model's decision and destinations, from its own layout
    bool want_inplace = m.current;
    std::vector<int64_t> at(m.kc), add(m.kc, 0), want_dst;
    for (int l = 0; l < m.kc; ++l) at[l] = m.len(l);
    for (int32_t l : lst) add[l]++;
    for (int l = 0; l < m.kc && m.current; ++l) want_inplace = want_inplace && at[l] + add[l] <= m.cap[l];
    for (int64_t i = 0; i < nnew; ++i) {
        const int l = lst[i];
        if (want_inplace) {
            want_dst.push_back(m.codeoff[l] + at[l] * m.cs);
            want_dst.push_back(m.pos[l] + at[l]);
            CHECK(at[l] < m.cap[l]);   // inside the list's capacity: what the device scatter relies on
        }
        ++at[l];
        m.rows.push_back(Row{l, ids[i], std::vector<uint8_t>(cod.begin() + i * m.cb, cod.begin() + (i + 1) * m.cb)});
    }
    std::vector<int64_t> dst(3, -7);
    const bool inplace = mir.append(nnew, lst.data(), cod.data(), ids.data(), m.cb, m.current ? &lay : nullptr, m.cs, dst);
    CHECK(inplace == want_inplace && dst == want_dst);
    g_inplace += inplace;
    m.current = inplace;   // (the runtime leaves the handle stale otherwise)
    compare(m, mir);
}

static void do_erase(Model &m, ListMirror &mir, const std::vector<uint32_t> &req)
{
    ++g_erases;
    const ListMirror before = mir;
    const std::vector<uint32_t> rem = mir.find_ids((int64_t)req.size(), req.data());
    CHECK(mir.h_len == before.h_len && mir.hl_codes == before.hl_codes && mir.hl_ids == before.hl_ids && mir.n == before.n &&
          mir.maxlen == before.maxlen);
    std::vector<uint32_t> gone;
    for (const Row &r : m.rows)
        if (std::find(req.begin(), req.end(), r.id) != req.end()) gone.push_back(r.id);
    std::sort(gone.begin(), gone.end());
    CHECK(rem == gone);
    if (rem.empty()) return compare(m, mir);   // the entry returns here: nothing may have changed
    g_erased += (long long)rem.size();
    std::vector<Row> kept;
    for (const Row &r : m.rows) {
        if (std::find(req.begin(), req.end(), r.id) != req.end()) continue;
        uint32_t below = 0;
        for (uint32_t g : gone) below += g < r.id;
        kept.push_back(Row{r.list, r.id - below, r.code});
    }
    m.rows.swap(kept);
    mir.erase_ids(rem, m.cb);
    compare(m, mir);
}

static void run_shape(int kc, int cb, uint32_t seed)
{
    std::mt19937 rng(seed);
    Model m{kc, cb, (cb + 3) / 4 * 4, {}, false, {}, {}, {}};
    ListMirror mir;
    DeviceLayout lay;
    mir.reset(kc);
    compare(m, mir);   // the empty index
    uint32_t next_id = 0;
    auto spare = [&] {
        std::vector<int64_t> caps(kc);
        for (int l = 0; l < kc; ++l) caps[l] = spare_cap(mir.h_len[l]);
        return caps;
    };
    do_layout(m, mir, lay, spare());   // (of the empty index: 32 slots a list)
    for (int round = 0; round < 6; ++round) {
        // assign: random lengths, list 0 or the last one empty in turn, everything empty once
        std::vector<int64_t> off(kc + 1, 0);
        for (int l = 0; l < kc; ++l) off[l + 1] = off[l] + ((round == 3 || l == (round % 2 ? 0 : kc - 1)) && kc > 1 ? 0 : (int64_t)(rng() % 40));
        if (round == 3) off.assign(kc + 1, 0);
        const int64_t n = off[kc];
        const std::vector<uint8_t> codes = random_codes(rng, (size_t)n * cb);
        std::vector<uint32_t> ids((size_t)n);
        for (uint32_t &v : ids) v = next_id++;
        CHECK(!ListMirror::check_offsets(kc, off.data(), n ? codes.data() : nullptr, n ? ids.data() : nullptr));
        mir.assign(off.data(), n ? codes.data() : nullptr, n ? ids.data() : nullptr, cb);
        m.rows.clear();
        m.current = false;
        for (int l = 0; l < kc; ++l)
            for (int64_t p = off[l]; p < off[l + 1]; ++p)
                m.rows.push_back(Row{l, ids[p], std::vector<uint8_t>(codes.begin() + p * cb, codes.begin() + (p + 1) * cb)});
        compare(m, mir);
        do_append(m, mir, lay, rng, {(int32_t)(rng() % kc)}, next_id);   // on a stale layout: never in place
        do_layout(m, mir, lay, spare());
        do_append(m, mir, lay, rng, {}, next_id);                        // 0 points
        do_append(m, mir, lay, rng, {(int32_t)(rng() % kc)}, next_id);   // 1 point
        // exactly fill list t's capacity, then overflow it by one
        const int t = (int)(rng() % kc);
        std::vector<int64_t> caps = spare();
        caps[t] = mir.h_len[t] + 3;
        do_layout(m, mir, lay, caps);
        do_append(m, mir, lay, rng, {t, t, t}, next_id);
        CHECK(m.current && mir.h_len[t] == caps[t]);
        do_append(m, mir, lay, rng, {t}, next_id);
        CHECK(!m.current);
        do_layout(m, mir, lay, spare());
        for (int step = 0; step < 30; ++step) {
            const unsigned op = rng() % 8;
            if (op < 3) {
                std::vector<int32_t> lst(rng() % 12);
                for (int32_t &l : lst) l = (int32_t)(rng() % kc);
                do_append(m, mir, lay, rng, lst, next_id);
            } else if (op < 5) {   // unsorted, duplicated, partly absent
                std::vector<uint32_t> req;
                for (unsigned i = 0, k = rng() % 6; i < k; ++i) {
                    req.push_back(m.rows.empty() || rng() % 3 == 0 ? (uint32_t)rng() : m.rows[rng() % m.rows.size()].id);
                    if (rng() % 2) req.push_back(req[rng() % req.size()]);
                }
                do_erase(m, mir, req);
            } else if (op == 5) {
                const uint32_t delta = rng() % 2 ? (uint32_t)rng() : (uint32_t)-(int32_t)(1 + rng() % 3);   // wraps uint32 either way
                for (Row &r : m.rows) r.id += delta;
                mir.shift_ids(delta);
                compare(m, mir);
            } else if (op == 6) {
                do_layout(m, mir, lay, spare());
            } else {
                do_erase(m, mir, {0xFFFFFFF0u, 0xFFFFFFF0u});   // (almost surely) nothing present
            }
        }
        // erase, then a shift that wraps: the largest id goes past 2^32
        if (!m.rows.empty()) do_erase(m, mir, {m.rows.front().id});
        uint32_t mx = 0, above = 0;
        for (const Row &r : m.rows) mx = std::max(mx, r.id);
        CHECK(mir.first_id_above(mx, above) == false && (m.rows.empty() || mx == 0 || (mir.first_id_above(mx - 1, above) && above == mx)));
        const uint32_t wrap = 0u - mx;   // mx -> 0
        for (Row &r : m.rows) r.id += wrap;
        mir.shift_ids(wrap);
        compare(m, mir);
        // everything
        std::vector<uint32_t> all;
        for (const Row &r : m.rows) all.push_back(r.id);
        std::shuffle(all.begin(), all.end(), rng);
        do_erase(m, mir, all);
        CHECK(mir.n == 0 && mir.maxlen == 0);
        do_erase(m, mir, {1u, 2u});   // of the empty index
    }
}

// ---- 3. the 2^32 refusals, on lengths alone ---------------------------------------------------------------------------------------------
static int check_limits()
{
    int cases = 0;
    const int64_t half = (int64_t)1 << 31;
    struct Case { std::vector<int64_t> cap, len; Error::Kind want; };
    const Case table[] = {
        {{half, half - 1}, {half, half - 1}, Error::None},          // 2^32 - 1 slots, 2^32 - 1 points
        {{half, half}, {half, half - 1}, Error::TooManySlots},      // 2^32 slots
        {{half, half}, {half, half}, Error::TooManyPoints},         // 2^32 points (named before the slots)
        {{ID_LIMIT}, {0}, Error::None},
        {{ID_LIMIT + 1}, {0}, Error::TooManySlots},
        {{0, 0, ID_LIMIT}, {0, 0, 0}, Error::None},
    };
    for (const Case &c : table) {
        DeviceLayout lay;
        lay.d_cap = c.cap;
        LayoutTotals tot;
        for (int cs : {4, 8, 16}) {
            CHECK(layout_from_caps(lay, c.len, cs, tot).kind == c.want);
            if (c.want == Error::None) CHECK(lay.d_pos.back() + c.cap.back() == tot.id_slots && tot.code_bytes >= (size_t)tot.id_slots * cs);
            ++cases;
        }
    }
    const uint8_t some_codes[1] = {0};
    const uint32_t some_ids[1] = {0};
    const int64_t ok[3] = {0, half, ID_LIMIT}, over[3] = {0, half, ID_LIMIT + 1}, back[3] = {0, 5, 4}, start[3] = {1, 2, 3}, none[3] = {0, 0, 0};
    CHECK(!ListMirror::check_offsets(2, ok, some_codes, some_ids));   // (pointers are not followed)
    CHECK(ListMirror::check_offsets(2, over, some_codes, some_ids).kind == Error::TooManyPoints);
    const Error eb = ListMirror::check_offsets(2, back, some_codes, some_ids);
    CHECK(eb.kind == Error::OffsetsOrder && eb.list == 1);
    CHECK(ListMirror::check_offsets(2, start, some_codes, some_ids).kind == Error::OffsetsStart);
    CHECK(ListMirror::check_offsets(2, ok, nullptr, some_ids).kind == Error::NullArrays && ListMirror::check_offsets(2, ok, some_codes, nullptr).kind == Error::NullArrays);
    CHECK(!ListMirror::check_offsets(2, none, nullptr, nullptr));
    CHECK(spare_cap(0) == 32 && spare_cap(255) == 287 && spare_cap(256) == 288 && spare_cap(264) == 297);
    return cases + 7;
}

// ---- 4. the label map -------------------------------------------------------------------------------------------------------------------
static long long g_offenders = 0;

static int check_labels()
{
    std::mt19937 rng(4242);
    int maps = 0;
    const int m = 3, n = 9;
    for (int ksub : {2, 257})
        for (int kind = 0; kind < 3; ++kind) {   // identity, permuted, sparse
            std::vector<uint16_t> lab((size_t)m * ksub);
            for (int i = 0; i < m; ++i) {
                std::vector<uint16_t> pool(kind == 2 ? 65536 : ksub);
                for (size_t v = 0; v < pool.size(); ++v) pool[v] = (uint16_t)v;
                if (kind) std::shuffle(pool.begin(), pool.end(), rng);
                if (kind == 1 && pool[0] == 0) std::swap(pool[0], pool[1]);
                std::copy(pool.begin(), pool.begin() + ksub, lab.begin() + (size_t)i * ksub);
            }
            LabelMap lm;
            CHECK(!lm.init16(lab.data(), m, ksub));
            CHECK(lm.identity == (kind == 0));
            ++maps;
            auto is_label = [&](int i, uint16_t v) { return std::find(lab.begin() + (size_t)i * ksub, lab.begin() + (size_t)(i + 1) * ksub, v) != lab.begin() + (size_t)(i + 1) * ksub; };
            std::vector<uint16_t> idx((size_t)n * m), codes((size_t)n * m);
            for (int e = 0; e < n * m; ++e) {
                idx[e] = (uint16_t)(rng() % ksub);
                codes[e] = lab[(size_t)(e % m) * ksub + idx[e]];
            }
            std::vector<uint8_t> out;
            CHECK(!lm.to_indices(n, codes.data(), out) && out.size() == idx.size() * 2 && memcmp(out.data(), idx.data(), out.size()) == 0);
            lm.to_labels(n, out.data());
            CHECK(memcmp(out.data(), codes.data(), out.size()) == 0);
            CHECK(!lm.to_indices(0, nullptr, out) && out.empty());
            uint16_t bad = 0;
            while (is_label(0, bad) || is_label(1, bad) || is_label(2, bad)) bad = (uint16_t)rng();
            for (int at : {0, n * m / 2, n * m - 1}) {
                std::vector<uint16_t> c2 = codes;
                c2[at] = bad;
                if (at + 1 < n * m) c2[n * m - 1] = bad;   // a later offender must not be the one reported
                const Error e = lm.to_indices(n, c2.data(), out);
                CHECK(e.kind == Error::NotALabel && e.point == at / m && e.codebook == at % m && e.value == (int)bad);
                ++g_offenders;
            }
            // a duplicate label in the last block
            lab[(size_t)(m - 1) * ksub + 1] = lab[(size_t)(m - 1) * ksub];
            const Error d = lm.init16(lab.data(), m, ksub);
            CHECK(d.kind == Error::DuplicateLabel && d.codebook == m - 1 && d.value == (int)lab[(size_t)(m - 1) * ksub]);
        }
    // 8-bit handles: label bytes are kept as they are and only validated
    for (int ksub : {2, 256}) {
        std::vector<uint8_t> lab((size_t)m * ksub);
        for (int i = 0; i < m; ++i)
            for (int c = 0; c < ksub; ++c) lab[(size_t)i * ksub + c] = (uint8_t)(ksub == 256 ? c : 5 + 100 * c + i);
        LabelMap lm;
        CHECK(!lm.init8(lab.data(), m, ksub) && lm.identity == (ksub == 256));
        ++maps;
        std::vector<uint8_t> codes((size_t)n * m);
        for (int e = 0; e < n * m; ++e) codes[e] = lab[(size_t)(e % m) * ksub + rng() % ksub];
        CHECK(!lm.check8(n, codes.data()) && !lm.check8(0, nullptr));
        if (ksub == 256) continue;   // every byte is a label
        for (int at : {0, n * m / 2, n * m - 1}) {
            std::vector<uint8_t> c2 = codes;
            c2[at] = 4;
            if (at + 1 < n * m) c2[n * m - 1] = 4;
            const Error e = lm.check8(n, c2.data());
            CHECK(e.kind == Error::NotALabel && e.point == at / m && e.codebook == at % m && e.value == 4);
            ++g_offenders;
        }
        lab[1] = lab[0];
        const Error d = lm.init8(lab.data(), m, ksub);
        CHECK(d.kind == Error::DuplicateLabel && d.codebook == 0 && d.value == (int)lab[0]);
    }
    return maps;
}

int main()
{
    int shapes = 0;
    for (int kc : {1, 2, 7})
        for (int cb : {1, 3, 8, 16}) {
            run_shape(kc, cb, 1000u + (uint32_t)(kc * 100 + cb));
            ++shapes;
        }
    const int limits = check_limits();
    const int maps = check_labels();
    if (g_fail) {
        fprintf(stderr, "list_mirror_check: %d checks failed\n", g_fail);
        return 1;
    }
    printf("list_mirror_check ok: %d shapes, %lld steps, %lld appends, %lld in place, %lld erases, %lld ids erased, %lld layouts, %d limit cases, %d label maps, %lld offenders\n",
           shapes, g_steps, g_appends, g_inplace, g_erases, g_erased, g_layouts, limits, maps, g_offenders);
    return 0;
}
