// The host side of the inverted lists (ivfadc_hip.hip's write path).  Plain C++ (no HIP types), in the manner of search_call.h /
// range_plan.h, so that every edit of the mirror compiles and runs without a GPU (tests/c/list_mirror_check.cpp).
//
// The mirror is the source of truth: one (codes, ids) pair per list, codes in MIRROR FORM -- cb bytes per point: m label bytes on an
// 8-bit handle, m little-endian uint16 codeword INDICES on a 16-bit one (LabelMap translates at the boundary).  The device copy is a
// layout of the same lists with spare capacity behind each (spare_cap, layout_from_caps, stage); the launches and copies that keep it
// current are the .hip file's.
//
// INVARIANT: h_len[l] == hl_ids[l].size() == hl_codes[l].size() / cb for every list that keeps data (synthetic lists and views keep
// lengths only), n == the sum of h_len, maxlen == its maximum.  Every edit below keeps it, and an edit that can fail (an allocation)
// fails before it has changed anything.
//
// Errors leave as a code and the facts a message needs; the caller words them.
#pragma once

#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <vector>

namespace list_mirror {

constexpr int64_t ID_LIMIT = (int64_t)0xFFFFFFFFll;   // ids are UInt32 positions
constexpr size_t CODE_SLACK = 64 << 10;                // readable bytes behind the last list's codes
constexpr size_t CODE_ALIGN = 256;                     // every list's code block starts on one

struct Error {
    enum Kind {
        None,
        OffsetsStart,    // offsets[0] != 0
        OffsetsOrder,    // list: the first l with offsets[l + 1] < offsets[l]
        TooManyPoints,   // more than ID_LIMIT points
        NullArrays,      // points, but no codes or no ids
        TooManySlots,    // more than ID_LIMIT id slots once every list has its capacity
        NotALabel,       // value: the code, point, codebook: the first offender in point-major order
        DuplicateLabel,  // value: the label, codebook
    } kind = None;
    int64_t list = 0, point = 0;
    int value = 0, codebook = 0;
    explicit operator bool() const { return kind != None; }
};

// ---- the label map: code labels <-> codeword indices ----------------------------------------------------------------------------------
struct LabelMap {
    int m = 0, ksub = 0;
    bool identity = false;             // label c of every block is c: nothing to translate
    std::vector<uint8_t> ok8;          // 8-bit handles: [m][256] validity of a label byte
    std::vector<uint16_t> lab16;       // 16-bit handles: [m][ksub] labels ...
    std::vector<uint32_t> sorted;      // ... and label << 16 | codeword index, ascending within each block

    Error init8(const uint8_t *labels, int m_, int ksub_)
    {
        m = m_; ksub = ksub_;
        ok8.assign((size_t)m * 256, 0);
        identity = true;
        for (int i = 0; i < m; ++i)
            for (int c = 0; c < ksub; ++c) {
                const uint8_t lab = labels[(size_t)i * ksub + c];
                if (ok8[(size_t)i * 256 + lab]) return Error{Error::DuplicateLabel, 0, 0, (int)lab, i};
                ok8[(size_t)i * 256 + lab] = 1;
                identity = identity && lab == c;
            }
        return Error{};
    }

    Error init16(const uint16_t *labels, int m_, int ksub_)
    {
        m = m_; ksub = ksub_;
        lab16.assign(labels, labels + (size_t)m * ksub);
        sorted.resize((size_t)m * ksub);
        identity = true;
        for (int i = 0; i < m; ++i) {
            uint32_t *b = sorted.data() + (size_t)i * ksub;
            for (int c = 0; c < ksub; ++c) {
                b[c] = ((uint32_t)labels[(size_t)i * ksub + c] << 16) | (uint32_t)c;
                identity = identity && labels[(size_t)i * ksub + c] == c;
            }
            std::sort(b, b + ksub);
            for (int c = 1; c < ksub; ++c)
                if ((b[c] >> 16) == (b[c - 1] >> 16)) return Error{Error::DuplicateLabel, 0, 0, (int)(b[c] >> 16), i};
        }
        return Error{};
    }

    // codeword index of label v in block i, -1: not a label of the block
    int32_t find16(int i, uint16_t v) const
    {
        if (identity) return v < ksub ? (int32_t)v : -1;
        const uint32_t *b = sorted.data() + (size_t)i * ksub, *e = b + ksub;
        const uint32_t *it = std::lower_bound(b, e, (uint32_t)v << 16);
        return (it != e && (*it >> 16) == v) ? (int32_t)(*it & 0xFFFFu) : -1;
    }

    // n x m label bytes: every one a label of its block (the mirror keeps them as they are)
    Error check8(int64_t n, const uint8_t *codes) const
    {
        if (ksub == 256) return Error{};   // every byte is a label
        for (int64_t p = 0; p < n; ++p)
            for (int i = 0; i < m; ++i)
                if (!ok8[(size_t)i * 256 + codes[(size_t)p * m + i]]) return Error{Error::NotALabel, 0, p, (int)codes[(size_t)p * m + i], i};
        return Error{};
    }

    // labels (n x m uint16) -> codeword indices in mirror form
    Error to_indices(int64_t n, const uint16_t *lab, std::vector<uint8_t> &out) const
    {
        out.resize((size_t)n * m * 2);
        for (int64_t p = 0; p < n; ++p)
            for (int i = 0; i < m; ++i) {
                const uint16_t v = lab[(size_t)p * m + i];
                const int32_t c = find16(i, v);
                if (c < 0) return Error{Error::NotALabel, 0, p, (int)v, i};
                const uint16_t c16 = (uint16_t)c;
                memcpy(out.data() + ((size_t)p * m + i) * 2, &c16, 2);
            }
        return Error{};
    }

    // codeword indices (mirror form, n x m uint16) -> labels, in place
    void to_labels(int64_t n, void *codes) const
    {
        if (identity) return;
        uint8_t *c = (uint8_t *)codes;
        for (size_t e = 0; e < (size_t)n * m; ++e) {
            uint16_t v;
            memcpy(&v, c + e * 2, 2);
            v = lab16[(e % (size_t)m) * ksub + v];
            memcpy(c + e * 2, &v, 2);
        }
    }
};

// ---- the device layout, as far as it is arithmetic ------------------------------------------------------------------------------------
// what upload_lists gives every list: room for push! to write in place for a while
inline int64_t spare_cap(int64_t len) { return len + std::max<int64_t>(32, len / 8); }

struct DeviceLayout {
    std::vector<int64_t> d_cap, d_pos, d_codeoff;   // per list: capacity in points, first id slot, first code byte
};

struct LayoutTotals {
    size_t code_bytes = 0;               // the code buffer, CODE_SLACK included
    int64_t id_slots = 0, n = 0, maxlen = 0;
};

// d_cap -> the offsets of every list in the id array and in the code buffer (cs: bytes of a point there), and the totals.  Arithmetic on
// lengths only: nothing here is sized by them.
inline Error layout_from_caps(DeviceLayout &lay, const std::vector<int64_t> &len, int cs, LayoutTotals &out)
{
    const size_t kc = lay.d_cap.size();
    lay.d_pos.assign(kc, 0);
    lay.d_codeoff.assign(kc, 0);
    size_t run = 0;
    int64_t pos = 0, maxlen = 0, n = 0;
    for (size_t l = 0; l < kc; ++l) {
        lay.d_pos[l] = pos;
        lay.d_codeoff[l] = (int64_t)run;
        pos += lay.d_cap[l];
        run += ((size_t)lay.d_cap[l] * (size_t)cs + CODE_ALIGN - 1) / CODE_ALIGN * CODE_ALIGN;
        maxlen = std::max(maxlen, len[l]);
        n += len[l];
    }
    if (n > ID_LIMIT) return Error{Error::TooManyPoints, 0, 0, 0, 0};
    if (pos > ID_LIMIT) return Error{Error::TooManySlots, 0, 0, 0, 0};
    out.code_bytes = run + CODE_SLACK;
    out.id_slots = pos;
    out.n = n;
    out.maxlen = maxlen;
    return Error{};
}

// ---- the mirror -----------------------------------------------------------------------------------------------------------------------
struct ListMirror {
    std::vector<int64_t> h_len;                  // [kc] points per list (kept for synthetic lists and views too)
    std::vector<std::vector<uint8_t>> hl_codes;  // [kc] len x cb bytes
    std::vector<std::vector<uint32_t>> hl_ids;   // [kc]
    int64_t n = 0, maxlen = 0;

    int64_t ntotal() const { return n; }

    void refresh_totals()
    {
        n = 0; maxlen = 0;
        for (int64_t v : h_len) { n += v; maxlen = std::max(maxlen, v); }
    }

    // kc empty lists
    void reset(int kc)
    {
        h_len.assign((size_t)kc, 0);
        hl_codes.assign((size_t)kc, {});
        hl_ids.assign((size_t)kc, {});
        n = maxlen = 0;
    }

    // what a view is given: lengths, no data
    void copy_lengths(const ListMirror &o) { h_len = o.h_len; n = o.n; maxlen = o.maxlen; }

    // lengths without data (device-synthesised lists)
    void assign_lengths(const int64_t *offsets)
    {
        for (size_t l = 0; l < h_len.size(); ++l) {
            h_len[l] = offsets[l + 1] - offsets[l];
            std::vector<uint8_t>().swap(hl_codes[l]);
            std::vector<uint32_t>().swap(hl_ids[l]);
        }
        refresh_totals();
    }

    static Error check_offsets(int kc, const int64_t *offsets, const void *codes, const uint32_t *ids)
    {
        if (offsets[0] != 0) return Error{Error::OffsetsStart, 0, 0, 0, 0};
        for (int l = 0; l < kc; ++l)
            if (offsets[l + 1] < offsets[l]) return Error{Error::OffsetsOrder, l, 0, 0, 0};
        if (offsets[kc] > ID_LIMIT) return Error{Error::TooManyPoints, 0, 0, 0, 0};
        if (offsets[kc] > 0 && (!codes || !ids)) return Error{Error::NullArrays, 0, 0, 0, 0};
        return Error{};
    }

    // mirror <- (offsets that passed check_offsets, codes in mirror form, ids)
    void assign(const int64_t *offsets, const uint8_t *codes, const uint32_t *ids, int cb)
    {
        for (size_t l = 0; l < h_len.size(); ++l) {
            const int64_t a = offsets[l], b = offsets[l + 1];
            h_len[l] = b - a;
            if (b > a) {
                hl_codes[l].assign(codes + (size_t)a * cb, codes + (size_t)b * cb);
                hl_ids[l].assign(ids + a, ids + b);
            } else {
                hl_codes[l].clear();
                hl_ids[l].clear();
            }
        }
        refresh_totals();
    }

    // the lists one behind the other; every output is optional, offsets has kc + 1 entries
    void gather(int64_t *offsets, uint8_t *codes, uint32_t *ids, int cb) const
    {
        int64_t run = 0;
        for (size_t l = 0; l < h_len.size(); ++l) {
            const int64_t len = h_len[l];
            if (offsets) offsets[l] = run;
            if (codes && len) memcpy(codes + (size_t)run * cb, hl_codes[l].data(), (size_t)len * cb);
            if (ids && len) memcpy(ids + run, hl_ids[l].data(), (size_t)len * 4);
            run += len;
        }
        if (offsets) offsets[h_len.size()] = run;
    }

    // push!: new points go to the END of their list, in call order (utils.jl:143-144).  lst / cod: the assignment and the codes (mirror
    // form) of the nnew points.  `lay`: the device layout when it is current (have_lists && !dirty), null when it is not.  True: every
    // target list has room, and dst holds the (code byte offset, id slot) pair of each new point for the in-place device update; false:
    // dst is empty and the next search lays the lists out again.  Everything that can fail -- one histogram, the reserves -- comes before
    // the first change.
    bool append(int64_t nnew, const int32_t *lst, const uint8_t *cod, const uint32_t *ids, int cb, const DeviceLayout *lay, int cs,
                std::vector<int64_t> &dst)
    {
        const size_t kc = h_len.size();
        std::vector<int64_t> add(kc, 0);
        for (int64_t i = 0; i < nnew; ++i) add[lst[i]]++;
        bool inplace = lay != nullptr;
        for (size_t l = 0; l < kc && inplace; ++l)
            if (h_len[l] + add[l] > lay->d_cap[l]) inplace = false;
        dst.clear();
        if (inplace) dst.resize((size_t)nnew * 2);
        for (size_t l = 0; l < kc; ++l)
            if (add[l]) {
                hl_codes[l].reserve(hl_codes[l].size() + (size_t)add[l] * cb);
                hl_ids[l].reserve(hl_ids[l].size() + (size_t)add[l]);
            }
        for (int64_t i = 0; i < nnew; ++i) {
            const int l = lst[i];
            if (inplace) {
                dst[2 * i] = lay->d_codeoff[l] + h_len[l] * cs;
                dst[2 * i + 1] = lay->d_pos[l] + h_len[l];
            }
            hl_codes[l].insert(hl_codes[l].end(), cod + (size_t)i * cb, cod + (size_t)(i + 1) * cb);
            hl_ids[l].push_back(ids[i]);
            h_len[l]++;
            maxlen = std::max(maxlen, h_len[l]);
        }
        n += nnew;
        return inplace;
    }

    // deleteat!, step 1: the stored ids among the nreq requested ones (any order, duplicates allowed), ascending, one per stored entry.
    // Changes nothing.
    std::vector<uint32_t> find_ids(int64_t nreq, const uint32_t *req) const
    {
        std::vector<uint32_t> want(req, req + nreq), rem;
        std::sort(want.begin(), want.end());
        want.erase(std::unique(want.begin(), want.end()), want.end());
        for (const std::vector<uint32_t> &lid : hl_ids)
            for (uint32_t v : lid)
                if (std::binary_search(want.begin(), want.end(), v)) rem.push_back(v);
        std::sort(rem.begin(), rem.end());
        return rem;
    }

    // step 2, with find_ids' result: drop those entries (stable), lower every surviving id by the number of removed ids below it
    // (_shift_inverse_index!, utils.jl:11-27), refresh the lengths, n and maxlen.  Allocates nothing.
    void erase_ids(const std::vector<uint32_t> &rem, int cb)
    {
        for (size_t l = 0; l < h_len.size(); ++l) {
            std::vector<uint32_t> &lid = hl_ids[l];
            std::vector<uint8_t> &lco = hl_codes[l];
            size_t wr = 0;
            for (size_t p = 0; p < lid.size(); ++p) {
                const size_t below = (size_t)(std::lower_bound(rem.begin(), rem.end(), lid[p]) - rem.begin());
                if (below < rem.size() && rem[below] == lid[p]) continue;
                if (wr != p) memmove(lco.data() + wr * cb, lco.data() + p * cb, (size_t)cb);
                lid[wr++] = lid[p] - (uint32_t)below;
            }
            lid.resize(wr);
            lco.resize(wr * cb);
            h_len[l] = (int64_t)wr;
        }
        refresh_totals();
    }

    // every id + delta, modulo 2^32
    void shift_ids(uint32_t delta)
    {
        for (std::vector<uint32_t> &lid : hl_ids)
            for (uint32_t &v : lid) v += delta;
    }

    // the first stored id above lim, in list order (false: there is none)
    bool first_id_above(uint32_t lim, uint32_t &out) const
    {
        for (const std::vector<uint32_t> &lid : hl_ids)
            for (uint32_t v : lid)
                if (v > lim) { out = v; return true; }
        return false;
    }

    // the buffers upload_lists copies to the device: codes at stride cs inside zeroed, aligned blocks; ids at their slots
    void stage(const DeviceLayout &lay, const LayoutTotals &tot, int cb, int cs, std::vector<uint8_t> &codes, std::vector<uint32_t> &ids) const
    {
        codes.assign(tot.code_bytes, 0);
        ids.assign((size_t)std::max<int64_t>(1, tot.id_slots), 0);
        for (size_t l = 0; l < h_len.size(); ++l) {
            const int64_t len = h_len[l];
            if (!len) continue;
            uint8_t *dst = codes.data() + lay.d_codeoff[l];
            const uint8_t *src = hl_codes[l].data();
            if (cs == cb) memcpy(dst, src, (size_t)len * cb);
            else
                for (int64_t p = 0; p < len; ++p) memcpy(dst + (size_t)p * cs, src + (size_t)p * cb, (size_t)cb);
            memcpy(ids.data() + lay.d_pos[l], hl_ids[l].data(), (size_t)len * 4);
        }
    }
};

}  // namespace list_mirror
