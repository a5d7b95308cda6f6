// The queries a function of the host runtime is working on, as ONE object carried from the C entries to the kernel launches.  Plain C++
// (no HIP types), in the manner of range_plan.h: the only pointer arithmetic on per-query rows -- slice() -- compiles and runs without a
// GPU (tests/c/search_call_check.cpp).  Every sub-batch, stage-A batch, sort group and grid-y block of a search is a slice of the call it
// came from: a row that is present advances by its own stride, a row that is absent (null) stays absent.
#pragma once

#include <cstddef>
#include <cstdint>

namespace ivf {

// An aggregate: a plain call is SearchCall{nq, d, K, w, q, ids, dists, counts}; the entries that have more rows fill them in.
struct SearchCall {
    int64_t nq = 0;                            // queries of this call (or slice)
    int d = 0, K = 0, w = 0;
    const float *q = nullptr;                  // [nq][d]
    uint32_t *ids = nullptr;                   // [nq][K]  (null: ivfadc_search_device_partial leaves keys instead)
    float *dists = nullptr;                    // [nq][K]
    int32_t *counts = nullptr;                 // [nq]
    const float *radii = nullptr;              // [nq]     range search only
    const int *pre_list = nullptr;             // [nq][w]  the caller's probes in visit order (ivfadc_search_preassigned) ...
    const float *pre_dc = nullptr;             // [nq][w]  ... and their coarse distances
    int32_t *out_list = nullptr;               // [nq][w]  coarse search only: where the probes go ...
    float *out_dc = nullptr;                   // [nq][w]  ... and their distances
    const uint32_t *mask_words = nullptr;      // [nmasks][W]  masked search only: the set's slot-space rows (constant over a call) ...
    const uint64_t *mask_word_off = nullptr;   // [kc + 1]
    uint64_t mask_W = 0;
    const int32_t *mask_of_query = nullptr;    // [nq]     ... and the mask number of every query, each in [-1, nmasks)
    bool whole_batch = true;                   // this IS the entry's call, not a part of it: hints and prefetched rows apply
    bool pre() const { return pre_list != nullptr; }
    bool masked() const { return mask_words != nullptr; }

    // queries b0 .. b0 + n - 1 of this call
    SearchCall slice(int64_t b0, int64_t n) const
    {
        SearchCall s = *this;
        const size_t o = (size_t)b0, sd = (size_t)d, sK = (size_t)K, sw = (size_t)w;
        if (q) s.q = q + o * sd;
        if (ids) s.ids = ids + o * sK;
        if (dists) s.dists = dists + o * sK;
        if (counts) s.counts = counts + o;
        if (radii) s.radii = radii + o;
        if (pre_list) s.pre_list = pre_list + o * sw;
        if (pre_dc) s.pre_dc = pre_dc + o * sw;
        if (out_list) s.out_list = out_list + o * sw;
        if (out_dc) s.out_dc = out_dc + o * sw;
        if (mask_of_query) s.mask_of_query = mask_of_query + o;
        s.nq = n;
        s.whole_batch = whole_batch && b0 == 0 && n == nq;
        return s;
    }
};

// The probe rows a coarse stage left for the queries of a batch (the handle's probe_list / probe_dc / probe_base): [queries][w] each.
struct ProbeRows {
    const int *list = nullptr;   // [queries][w] each
    const float *dc = nullptr;
    const uint32_t *base = nullptr;
    int w = 0;
    ProbeRows slice(int64_t g0) const   // the rows from query g0 of the batch on
    {
        const size_t o = (size_t)g0 * (size_t)w;
        return ProbeRows{list ? list + o : list, dc ? dc + o : dc, base ? base + o : base, w};
    }
};

}  // namespace ivf
