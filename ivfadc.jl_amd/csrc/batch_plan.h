// The schedule of the host-pointer searches (ivfadc_search, ivfadc_search_batches, ivfadc_mg_search); DESIGN.md 4.8 states the rules.
// Plain C++ (no HIP types, no handle), in the manner of search_call.h / range_plan.h: it compiles and runs without a GPU
// (tests/c/batch_plan_check.cpp).  The host runtime keeps the HIP calls: events, ingest_rows, search_dev.
#pragma once

#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <vector>

namespace batch_plan {

// The non-empty batches of a run, in order: batch i is rows [start[i], start[i] + cnt[i]) of the run's total rows.
struct Batches {
    std::vector<int64_t> start, cnt;
    int64_t total = 0;
    size_t size() const { return start.size(); }
};
// -1, or the first batch whose size is negative (out is then unspecified)
inline int non_empty_batches(const int64_t *batch_nq, int nbatches, Batches &out)
{
    out = Batches();
    out.start.reserve(nbatches > 0 ? (size_t)nbatches : 0);
    out.cnt.reserve(nbatches > 0 ? (size_t)nbatches : 0);
    for (int b = 0; b < nbatches; ++b) {
        if (batch_nq[b] < 0) return b;
        if (batch_nq[b] > 0) { out.start.push_back(out.total); out.cnt.push_back(batch_nq[b]); }
        out.total += batch_nq[b];
    }
    return -1;
}

// Upload groups: consecutive batches that travel as one ingest launch and one event.  stride = the lanes that search (1 or 2).  The first
// `stride` groups are single batches, the others hold `per`: a run never needs more than MAX_GROUPS events.
constexpr size_t MAX_GROUPS = 256;
struct Groups {
    std::vector<size_t> first;   // group g = batches [first[g], first[g + 1])
    std::vector<size_t> of;      // of[i]: the group of batch i
    size_t size() const { return first.empty() ? 0 : first.size() - 1; }
};
inline Groups upload_groups(size_t nbat, size_t stride)
{
    Groups gr;
    const size_t per = std::max<size_t>(stride, (nbat + 251) / 252);
    gr.first.reserve(std::min(nbat, MAX_GROUPS) + 1);
    for (size_t at = 0; at < nbat; at += (at < stride) ? 1 : per) gr.first.push_back(at);
    gr.first.push_back(nbat);
    gr.of.resize(nbat);
    for (size_t g = 0; g + 1 < gr.first.size(); ++g)
        for (size_t i = gr.first[g]; i < gr.first[g + 1]; ++i) gr.of[i] = g;
    return gr;
}

// What group g moves, in rows of row_bytes each: from its first batch's first row to its last batch's last (consecutive groups tile the run)
struct ByteRange { size_t off, bytes; };
inline ByteRange group_bytes(const Batches &bt, const Groups &gr, size_t g, size_t row_bytes)
{
    const size_t b1 = gr.first[g + 1] - 1, r0 = (size_t)bt.start[gr.first[g]], r1 = (size_t)bt.start[b1] + (size_t)bt.cnt[b1];
    return ByteRange{r0 * row_bytes, (r1 - r0) * row_bytes};
}

// The library's own numbering of the batches it hints to itself: never 0 (0 = undeclared), bit 63 set, counted on from the handle's base
inline uint64_t batch_token(uint64_t base, size_t i) { return (base + i + 1) | ((uint64_t)1 << 63); }

// Step i of a run of nbat batches on `stride` lanes
struct Step {
    size_t lane;            // 0: the handle itself; 1: its internal view
    uint64_t token;         // what the search declares for its own rows
    bool has_next;          // the last `stride` steps name no successor
    size_t next;            // the successor: the lane's next batch ...
    uint64_t next_token;    // ... under the token that step will declare
    size_t on_their_way;    // batches [0, on_their_way) are uploaded (or as many as there are) before the step is issued
};
inline Step step_of(size_t i, size_t nbat, size_t stride, uint64_t base)
{
    const bool has_next = i + stride < nbat;
    return Step{stride == 2 ? (i & 1) : 0, batch_token(base, i), has_next, i + stride, has_next ? batch_token(base, i + stride) : 0, i + 2 * stride + 1};
}

// Which ingest a lane still has to wait for.  The copy lane is in order, so the newest group a search needs covers the ones before it:
// groups [0, done[l]) are known complete to lane l, and a group seen fired marks every group before it.
struct IngestTracker {
    static constexpr size_t NOTHING = (size_t)-1;
    explicit IngestTracker(const Groups &groups) : gr(&groups), seen_(groups.size(), 0) {}
    // the group lane `lane` has to be sure of before it reads batch `batch` (clamped to the last one), or NOTHING; named to a lane once
    size_t needs(size_t lane, size_t batch)
    {
        const size_t g = gr->of[std::min(batch, gr->of.size() - 1)];
        if (done[lane] > g) return NOTHING;
        done[lane] = g + 1;
        return g;
    }
    void fired(size_t g) { std::fill(seen_.begin(), seen_.begin() + (ptrdiff_t)g + 1, (char)1); }
    bool seen(size_t g) const { return seen_[g] != 0; }

private:
    const Groups *gr;
    std::vector<char> seen_;
    size_t done[2] = {0, 0};
};

// The packed result block of `rows` queries, [ids rows*K | dists rows*K | counts rows], every element 32 bits wide: offsets and total in
// 32-bit words (the multi-device gather) or in bytes (the pinned block the kernels write)
struct ResultBlock {
    size_t ids, dists, counts, total;
    size_t ids_len() const { return dists - ids; }        // of ids, and of dists
    size_t counts_len() const { return total - counts; }
};
inline ResultBlock result_words(size_t rows, size_t K) { return ResultBlock{0, rows * K, 2 * rows * K, 2 * rows * K + rows}; }
inline ResultBlock result_bytes(size_t rows, size_t K) { return ResultBlock{0, 4 * rows * K, 8 * rows * K, 8 * rows * K + 4 * rows}; }

// device r's block of a batch of nq queries split over G devices: [mg_lo(r), mg_lo(r + 1)), contiguous, sizes differ by at most one
inline int64_t mg_lo(int64_t r, int64_t nq, int64_t G) { return r * (nq / G) + std::min<int64_t>(r, nq % G); }

}  // namespace batch_plan
