// wg8scan.hip.h -- list-major scan for long lists, EIGHT waves per workgroup on ONE table set (m = 8, ksub = 256, K <= 64; sub-spaces
// DS = 4, 8, 12 or 16 wide: d = 32, 64, 96 -- the Deep1B-style PQ8 shapes -- and 128, the SIFT1B shape), for NQ = 4 or 8 queries per
// code stream: wg8_scan_kernel<NQ> (DS = 16) and wg8_scan_kernel<NQ, DS> (DS = 4, 8, 12).  Included by kernels.hip.h, namespace ivf.
// 64 < K <= 128 runs the same body with a pool of TWO entries per lane (KP = 2: wg8_wide_scan_kernel<NQ, DS>, every DS; on request, table
// modes 8 / 9): the pool is the only thing in the kernel that is tied to 64 -- filter, bias test, rings and passes are per point, the
// cold-start bounds take the ceil(K / 8)-th and K-th of a step's 256 sums -- see THE WIDE POOL at w8_pool_offer.  KP = 1 is the code that
// every measurement below was taken with, unchanged behind `if constexpr`.
// m = 16 (d = 128 -- PQ16 -- and d = 64; K <= 64; on request, table modes 6 / 7) is wg8_m16_scan_kernel<NQ, DS>: the same design on a
// 256-byte row of 2 x 16 x 8 B or 16 x 16 B, 11-bit filter fields, one point per 16-byte request -- see THE M-GENERIC BODY and SIXTEEN
// SUB-QUANTIZERS below, and THE FILTER AT SIXTEEN TERMS at w8m_scan_items' quantisation.
// Only the residual fill and the table build know DS: the scan looks 8 code bytes per point up in a 64 KB integer table whatever the
// sub-spaces' width, so the scan loop, the pool, the passes and the hand-over are per NQ alone, and the LDS layout is the one of DS = 16
// (narrower sub-spaces leave residual rows unused).
//
// Reference: src/coarsequantizers.jl:40-45 (residuals), src/index.jl:232-236 (table build), :240-246 (scan), :247-254 (bounded top-K).
//
// What binds the four-wave kernel (scan_kernel<8, 16, 4, ..., STRIPE>) on this shape, by the counters: the LDS array is
// 81 % busy and two thirds of its cycles are bank-conflict replays -- the 32 lanes of a ds_read_b64 service group look the SAME
// sub-quantizer up at random codes, ~3 distinct rows per bank pair -- at 12 waves per CU (164 registers, 53 KB of LDS per workgroup).
// This kernel changes the three things that follow from that:
//
//   * CONFLICT-FREE GATHERS.  The 16-bit integer filter table (four queries per 8-byte entry, quantize as in quantize_tables_m8)
//     stands in FOUR copies; a code's row is exactly 256 bytes -- 4 copies x 8 sub-quantizers x 8 B = the 64 banks once -- and lane l
//     looks sub-quantizer (t + l) mod 8 up at slot t in copy (l / 8) mod 4: the 32 lanes of a service group read 32 different bank
//     pairs whatever their codes are.  Integer addition is associative, so the rotated order costs nothing, and because a row is
//     256 B the whole address (code << 8 | lane part) is ONE v_perm_b32 of the rotated code dword and a lane-constant dword.
//   * SIXTEEN WAVES PER CU.  512-thread workgroups, two per CU, at most 128 registers: one table build and one quantisation per
//     eight waves, four waves per SIMD to cover the LDS round trips.
//   * The f32 tables leave the LDS (64 KB of integer copies + 5 KB of state: two workgroups per CU).  The build writes them -- the
//     reference's sums, index.jl:232-236 order -- to a 32 KB block of device memory per workgroup (it stays in L2 / the memory-side
//     cache); what the filter lets through is parked and gets its reference-order sum from there, eight points per pass (lane ii of a
//     segment fetches sub-quantizer ii's entry, the running sum walks along the segment: drain as in drain_parked).  Only these sums
//     meet the selectors: ids and distances stay bit-identical to the oracle.
//   * A CROWD (a cold work item: no bound yet, every point a candidate) is not summed exactly point by point: the integer sums bound
//     the distances from ABOVE as well -- S < (dc + (Q + 8) / inv)(1 + 2^-16) -- so the K-th smallest integer sum of a step gives a
//     bound that K real points meet without one exact sum, and only what still passes under it is parked.
//
// Selection, bounds (workgroup-shared word in LDS, per-query word in HBM), partial results and the merge kernel behind it are those of
// scan_kernel; the work items are the same (list, group of <= NQ queries, chunk).
//
// EIGHT QUERIES PER CODE STREAM (NQ = 8).  The four-query form is bound by instruction issue (vector ALU 63 % + LDS
// instructions 18 % of the SIMD cycles, and the two add): a point costs 8 address perms + 8 gathers + 8 three-operand adds per FOUR
// queries.  With 16-byte table entries -- eight 16-bit fields -- the same perm and ONE ds_read_b128 serve EIGHT queries, 16 adds: 32
// instructions per point and eight queries instead of 48.  The table keeps its 64 KB: a code's row is 2 copies x 8 sub-quantizers x 16 B
// = 256 B, lane l reads sub-quantizer (t + l) mod 8 in copy (l / 16) mod 2 -- the four 16-lane service groups of a ds_read_b128 ({0-3,
// 12-15, 20-27}, {4-11, 16-19, 28-31}, and the same + 32: MI355X_MICROARCH.md) each see 16 different four-bank groups.  Work items are
// (list, group of <= 8 queries, chunk): half as many table builds, set-ups and hand-overs per probed list; the f32 tables in device
// memory are 64 KB per workgroup.  Everything else is the four-query form's, eight slots wide: the two differ in the half-step gather,
// the residual fill, the table build's trips and the quantised store, each behind `if constexpr (NQ == 8)`.  The plan takes this form
// where a list is probed by eight queries or more on average.
#pragma once

// W8_NW, W8_THREADS, W8_ES, W8_TAB_BYTES, the LDS layout W8Lds<NQ, KP, M> and w8_ds_ok are shared with the plan: scan_layouts.h, which
// kernels.hip.h includes in front of namespace ivf
template <int NQ, int M = 8> constexpr u32 W8_GTAB_FLOATS = (u32)M * 256u * (u32)NQ;   // f32 tables of a work item in device memory: [ii][label][NQ queries]
// the integer filter's cap per entry: M entries of at most W8_QCAP sum to less than 0x8000 (8 x 4095 = 32 760, 16 x 2047 = 32 752) -- see
// THE FILTER AT SIXTEEN TERMS below
template <int M> constexpr u32 W8_QCAP = M == 8 ? 4095u : 2047u;
static_assert(8u * W8_QCAP<8> <= 0x7FFFu && 16u * W8_QCAP<16> <= 0x7FFFu, "a point's integer sum stays below 0x8000");
static_assert(0x8000u + 16u * W8_QCAP<16> < 0x10000u && 0x8000u + 8u * W8_QCAP<8> < 0x10000u, "a biased field never carries into its neighbour");

// the residuals' floats per sub-quantizer: DS rows of NQ queries and ONE row of padding (why: at w8_ds_ok in scan_layouts.h)
template <int NQ, int DS> constexpr u32 W8_RES_STRIDE = (u32)((DS + 1) * NQ);

static __device__ __forceinline__ u32 w8_perm(u32 s0, u32 s1, u32 sel)
{
    u32 o;
    asm("v_perm_b32 %0, %1, %2, %3" : "=v"(o) : "v"(s0), "v"(s1), "s"(sel));
    return o;
}
// ... with the selector in a vector register (m = 16: the byte of the code dword a slot looks up depends on the lane)
static __device__ __forceinline__ u32 w8_permv(u32 s0, u32 s1, u32 sel)
{
    u32 o;
    asm("v_perm_b32 %0, %1, %2, %3" : "=v"(o) : "v"(s0), "v"(s1), "v"(sel));
    return o;
}

// the work item's per-slot constants stand in LDS at fixed addresses (the kernel owns the whole allocation: the dynamic segment starts
// at address 0); the rare paths read them there instead of holding two dozen scalars across the scan loop
template <class T> static __device__ __forceinline__ T w8_lds(u32 byte_addr) { return lds_load_abs<T>(byte_addr); }
// a pointer into the workgroup's dynamic LDS segment (for stores and atomics: an integer cast to a generic pointer is NOT an LDS address)
template <class T> static __device__ __forceinline__ T *w8_ptr(u32 byte_off)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char w8_smem[];
    return (T *)(w8_smem + byte_off);
}
template <int NQ> static __device__ __forceinline__ float w8_dc(int s) { return __uint_as_float(__builtin_amdgcn_readfirstlane(w8_lds<u32>(W8Lds<NQ>::QC + 4u * s))); }
template <int NQ> static __device__ __forceinline__ u32 w8_sbase(int s) { return __builtin_amdgcn_readfirstlane(w8_lds<u32>(W8Lds<NQ>::QC + 4u * NQ + 4u * s)); }
template <int NQ> static __device__ __forceinline__ float w8_inv(int s) { return __uint_as_float(__builtin_amdgcn_readfirstlane(w8_lds<u32>(W8Lds<NQ>::SMAX + 4u * NQ + 4u * s))); }
template <int NQ> static __device__ __forceinline__ u64 w8_sthr(int s) { return readfirstlane64(w8_lds<u64>(W8Lds<NQ>::STHR + 8u * s)); }

// The accumulator BIAS of the NQ queries under the bounds of the moment (two 16-bit fields per dword): field s of a point's accumulators
// starts at B_s = 0x7FFF - T_s (T_s = qf_targets' integer budget of query s; an unused slot gets 0x8000), so "field < 0x8000" <=>
// "sum_s <= T_s": the candidate test of a step is NQ ANDs and a compare, and the first add of a point absorbs the bias.  sum <= 32760,
// B <= 0x8000: fields never carry.  The bounds are the workgroup's (STHR in LDS: the pool's K-th key, the item's bound from outside, an
// integer-sum bound of a cold start -- whichever is smallest); a wave holds no bound of its own.
// Lane s (mod NQ) evaluates slot s -- qf_targets' arithmetic, operation for operation (its argument is what makes the filter exact) -- on the
// slot's constants in LDS: one round trip and a dozen vector instructions for the slots (evaluated slot by slot on uniform values it
// was eight dependent LDS round trips and ~200 instructions, paid at every refresh and after every pass: most of the candidate path).
template <int NQ> static __device__ __forceinline__ void w8_bias(int nvalid, u32 (&bias)[NQ / 2])
{
    const u32 sl = (u32)lane_id() & (u32)(NQ - 1);
    const u32 th = w8_lds<u32>(W8Lds<NQ>::STHR + 8u * sl + 4u);
    const float dc = w8_lds<float>(W8Lds<NQ>::QC + 4u * sl);
    const float inv = w8_lds<float>(W8Lds<NQ>::SMAX + 4u * NQ + 4u * sl);
    u32 T = 0x7FFFu;
    if (th < 0x7F800000u) {   // a finite bound
        const float thr = __uint_as_float(th);
        const float x = (thr * 1.0000038146972656f - dc) * inv * 1.0000038146972656f;   // (1 + 2^-18): as qf_targets
        T = x < 0.0f ? 0u : (x < 32000.0f ? (u32)x + 2u : 0x7FFFu);
    }
    const u32 B = (int)sl < nvalid ? 0x7FFFu - T : 0x8000u;
#pragma unroll
    for (int i = 0; i < NQ / 2; ++i)
        bias[i] = (u32)__builtin_amdgcn_readlane((int)B, 2 * i) | ((u32)__builtin_amdgcn_readlane((int)B, 2 * i + 1) << 16);
}
// the AND of a point's accumulator dwords: a field's top bit survives only if it is set for every query
static __device__ __forceinline__ u32 w8_and(const u32 (&q)[2]) { return q[0] & q[1]; }
static __device__ __forceinline__ u32 w8_and(const u32 (&q)[4]) { return (q[0] & q[1]) & (q[2] & q[3]); }
// ... of accumulators that were summed under the bias b and are to be tested under n
static __device__ __forceinline__ u32 w8_and_rebased(const u32 (&q)[2], const u32 (&b)[2], const u32 (&n)[2]) { return (q[0] - b[0] + n[0]) & (q[1] - b[1] + n[1]); }
static __device__ __forceinline__ u32 w8_and_rebased(const u32 (&q)[4], const u32 (&b)[4], const u32 (&n)[4])
{
    return ((q[0] - b[0] + n[0]) & (q[1] - b[1] + n[1])) & ((q[2] - b[2] + n[2]) & (q[3] - b[3] + n[3]));
}

// ---- the workgroup's selection: ONE pool of K keys per slot in LDS, shared by the eight waves ---------------------------------------------
// (index.jl:247-254: the bounded heap of a query.)  Eight per-wave selectors bound the union's K-th key only loosely -- a wave's own K-th
// key is the K-th of an eighth of the points, and max over the waves of their ceil(K / 8)-th keys sits near rank 3.6 K of what the workgroup
// has seen (the 2nd-order statistics' maximum) -- and every candidate the looser bound lets through costs an exact sum and a trip to L2:
// at w = 1, where every work item starts cold, the candidate path was a third of the kernel (knock-out build: 1.65 -> 1.09 ms).  The pool
// is the exact thing: its largest entry IS the K-th smallest key of everything the workgroup has offered.
//   pool[s][0 .. K): unordered, KEY_MAX = empty.  An offer x reads the K entries (one per lane), takes their maximum mx; x >= mx: K keys
//   below x exist, x is out.  Else lane 0 swaps x in for mx (compare-and-swap: another wave may have replaced that entry meanwhile -- an
//   entry only ever DECREASES, so a failed swap means progress elsewhere and the offer starts again; no ABA).  Dropping mx is safe: at the
//   moment of the swap the other K - 1 entries are at or below their snapshot values, all below mx, and so is x.  Keys are unique, so the
//   K smallest keys of all offers are never refused and never dropped: the pool ends as the exact top K in any interleaving (ids and
//   distances bit-identical to the oracle); the order is restored by one 64-lane sort when the work item is done.
//   The maximum of ANY snapshot -- K distinct keys that were offered -- is an upper bound of the K-th key: published with atomicMin.
// THE WIDE POOL (KP = 2, 64 < K <= 128; wg8_wide_scan_kernel).  A slot holds 128 entries, lane l owns entries l and l + 64 and a snapshot
// is two values per lane (v: entries 0 .. 63, vh: entries 64 .. 127; entries >= K read 0).  Nothing above counts lanes: an offer reads the K
// entries, mx is the wave's maximum of the per-lane maxima -- the value of ONE entry below K, keys being unique -- and the swap's target is the
// lowest index whose snapshot value is mx (a ballot on the low entries, then one on the high ones: empty entries are KEY_MAX, so the pool
// still fills from index 0, and an index is filled only by a wave whose snapshot showed every lower one filled -- the hand-over's prefix).
// Dropping mx is safe as before: the other K - 1 entries are at or below their snapshot values, all below mx.  TERMINATION of the offer loop:
// every trip either swaps a key in (the mask loses a bit) or fails, and a failed swap returns the value of the moment of the entry that was
// ADDRESSED, which is below its snapshot value mx (entries only decrease, and it is not mx); that value is patched into the half of the
// snapshot the index came from -- v for idx < 64, vh for idx >= 64, lane idx mod 64 -- so the sum of the snapshot strictly falls.  (A patch
// into the other half would leave the addressed entry's snapshot at mx: the same swap fails for ever.)
static __device__ __forceinline__ u32 w8_row_max_u32(u32 x)
{
    // running maximum along each row of 16 lanes (row_shr 1, 2, 4, 8: a lane without a source reads 0), rows' last lanes -> scalar unit
    x = max(x, (u32)__builtin_amdgcn_update_dpp(0, (int)x, 0x111, 0xf, 0xf, true));
    x = max(x, (u32)__builtin_amdgcn_update_dpp(0, (int)x, 0x112, 0xf, 0xf, true));
    x = max(x, (u32)__builtin_amdgcn_update_dpp(0, (int)x, 0x114, 0xf, 0xf, true));
    x = max(x, (u32)__builtin_amdgcn_update_dpp(0, (int)x, 0x118, 0xf, 0xf, true));
    const u32 a = __builtin_amdgcn_readlane(x, 15), b = __builtin_amdgcn_readlane(x, 31), c = __builtin_amdgcn_readlane(x, 47), d = __builtin_amdgcn_readlane(x, 63);
    const u32 ab = a > b ? a : b, cd = c > d ? c : d;
    return ab > cd ? ab : cd;
}
static __device__ __forceinline__ u64 w8_wave_max_u64(u64 v)
{
    const u32 hi = (u32)(v >> 32), lo = (u32)v;
    const u32 mh = w8_row_max_u32(hi);
    const u32 ml = w8_row_max_u32(hi == mh ? lo : 0u);
    return ((u64)mh << 32) | ml;
}
// the pool's entries of slot s, one per lane (lanes >= K: 0, below every key); KP = 2: entry lane + 64 half of the slot (half = 0, 1)
template <int NQ, int KP = 1> static __device__ __forceinline__ u64 w8_pool_read(int s, int K, int lane, int half = 0)
{
    if constexpr (KP == 1) {
        return lane < K ? w8_lds<u64>(W8Lds<NQ>::POOL + 512u * (u32)s + 8u * (u32)lane) : 0ull;
    } else {
        const int e = lane + 64 * half;
        return e < K ? w8_lds<u64>(W8Lds<NQ, 2>::POOL + 1024u * (u32)s + 8u * (u32)e) : 0ull;
    }
}
// Offers the keys of the lanes in `mask` (uniform, non-empty) to slot s, starting from the snapshot v the caller read a while ago.  A stale
// snapshot is as good as a fresh one for every decision above -- each of its values WAS that entry's, entries only decrease -- it merely
// fails a swap more often, and a failed swap returns the entry's value of the moment: the snapshot is patched and the offer goes on
// without another read.  An offer costs one LDS round trip per swap attempt (under the scan's gathers a round trip is several hundred
// cycles: the dependent trips, not the instructions, were the cost of a pass).  Returns the slot's new bound, KEY_MAX if nothing went in
// or the pool is not full.  (KP = 2: vh is the snapshot of entries 64 .. 127; KP = 1 has none.)
template <int NQ, int KP = 1> static __device__ __forceinline__ u64 w8_pool_offer(int s, u64 v, u64 key, u64 mask, int K, int lane, u64 vh = 0ull)
{
    bool any = false;
    if constexpr (KP == 2) {
        u64 *pool = w8_ptr<u64>(W8Lds<NQ, 2>::POOL + 1024u * (u32)s);
        u64 mx = w8_wave_max_u64(v > vh ? v : vh);
        for (;;) {   // uniform; terminates: see THE WIDE POOL above
            mask &= __builtin_amdgcn_ballot_w64(key < mx);
            if (mask == 0) break;
            const int src = __builtin_ctzll(mask);
            const u64 x = readlane64(key, src);
            // the lowest index whose snapshot is mx: low entries first (mx is one entry's value, so one of the two ballots is not empty;
            // an index is never formed from an empty one)
            const u64 blo = __builtin_amdgcn_ballot_w64(lane < K && v == mx), bhi = __builtin_amdgcn_ballot_w64(lane + 64 < K && vh == mx);
            if ((blo | bhi) == 0) break;
            const bool high = blo == 0;
            const int il = __builtin_ctzll(high ? bhi : blo);    // the owning lane; the entry is il + 64 high < K
            u64 old = 0;
            if (lane == 0) old = atomicCAS((unsigned long long *)&pool[il + (high ? 64 : 0)], (unsigned long long)mx, (unsigned long long)x);
            old = readfirstlane64(old);
            const u64 now = old == mx ? x : old;   // the addressed entry's value of the moment: x is in, or another wave's key sits there
            if (high) vh = lane == il ? now : vh;  // (uniform) the half that was addressed, and only that one
            else v = lane == il ? now : v;
            if (old == mx) {   // (uniform)
                any = true;
                mask &= mask - 1ull;
            }
            mx = w8_wave_max_u64(v > vh ? v : vh);
        }
        if (!any || mx == KEY_MAX) return KEY_MAX;
        if (lane == 0) atomicMin(w8_ptr<u64>(W8Lds<NQ>::STHR + 8u * (u32)s), mx);
        return mx;
    } else {
    u64 *pool = w8_ptr<u64>(W8Lds<NQ>::POOL + 512u * (u32)s);
    u64 mx = w8_wave_max_u64(v);
    for (;;) {   // uniform
        mask &= __builtin_amdgcn_ballot_w64(key < mx);   // (every lane's key against the bound of this moment: most offers of a crowd end here)
        if (mask == 0) break;
        const int src = __builtin_ctzll(mask);
        const u64 x = readlane64(key, src);
        const int idx = __builtin_ctzll(__builtin_amdgcn_ballot_w64(lane < K && v == mx));
        u64 old = 0;
        if (lane == 0) old = atomicCAS((unsigned long long *)&pool[idx], (unsigned long long)mx, (unsigned long long)x);
        old = readfirstlane64(old);
        if (old == mx) {   // (uniform) x is in
            v = lane == idx ? x : v;
            any = true;
            mask &= mask - 1ull;
        } else {
            v = lane == idx ? old : v;   // another wave's key sits there now
        }
        mx = w8_wave_max_u64(v);
    }
    if (!any || mx == KEY_MAX) return KEY_MAX;
    if (lane == 0) atomicMin(w8_ptr<u64>(W8Lds<NQ>::STHR + 8u * (u32)s), mx);
    return mx;
    }
}

// ---- reference-order sums of parked points, 8 per pass, entries from the work item's f32 tables in device memory -------------------
// (scope: the tables were written by this workgroup before a barrier; the loads go to L2 -- sc1 -- so that no line of an earlier work
// item's tables can be served from this CU's vector cache)
// queries 4 q4 .. 4 q4 + 3 of entry [ii][byte]
template <int NQ> static __device__ __forceinline__ v4f w8_gtab_load(__amdgpu_buffer_rsrc_t rs, u32 ii, u32 byte, int q4)
{
    const v4u v = __builtin_amdgcn_raw_buffer_load_b128(rs, (int)((((ii << 8) | byte) * (4u * NQ)) + 16u * (u32)q4), 0, 16);
    return (v4f){__uint_as_float(v.x), __uint_as_float(v.y), __uint_as_float(v.z), __uint_as_float(v.w)};
}

// A pass in flight: lane 8 e + ii holds the f32 entries (four queries per register set) of sub-quantizer ii at parked point e's code
// byte, and the point's position.  Requested when eight points are waiting (w8_pass_issue) and worked off at the top of the NEXT step,
// right behind the wait for that step's code bytes -- older than the gather -- so the trip to L2 costs the wave nothing (a pass worked off
// where it is requested waits for the code stream's request in flight AND its own: ~4 us per pass, measured).
template <int NQ> struct W8Pass {
    v4f ev[NQ / 4];
    u32 pos;
    bool ok;
};
// cache policy of the code stream's requests (aux of raw_buffer_load).  Measured with 2 (nt, "streaming": the lines are not kept in L2 ahead
// of the work items' f32 tables, which the passes gather from): 16 384 x w = 8 scan 6.15 -> 7.35 ms, 2048 x w = 8 1.15 -> 1.31 -- the four
// or five groups that stream the same list side by side live on each other's lines in L2 / the memory-side cache.  Default policy.
constexpr int W8_STREAM_AUX = 0;
constexpr int W8_TRIG = 8;        // parked points that trigger a pass (m = 8; a pass takes 64 / M points: w8_pp)
template <int M> constexpr int w8_pp = 64 / M;   // points per pass: a segment of M lanes per point
constexpr int W8_REFRESH = 8;     // steps between looks at the workgroup's shared bounds
constexpr int W8_PRIO_SCAN = 3;   // wave priority while the code stream is scanned, and after it
constexpr int W8_PRIO_REST = 0;
constexpr int W8_RING = 32;    // parked points per wave (a ring: entries head .. head + cnt - 1 mod 32)

template <int NQ> static __device__ __forceinline__ void w8_pass_issue(W8Pass<NQ> &ps, u32 cbuf_addr, int &head, int &cnt, __amdgpu_buffer_rsrc_t gt, int lane)
{
    const int seg = lane >> 3, ii = lane & 7;
    ps.ok = seg < cnt;
    const u32 ea = cbuf_addr + (u32)((head + (ps.ok ? seg : 0)) & (W8_RING - 1)) * (W8_ES * 4u);
    // (parked: the point's ROTATED code bytes -- out byte t = code byte (t + j) mod 8, j = the parking lane's rotation, kept in the position
    // word's top three bits: the scan loop holds no unrotated copy of a step's bytes)
    const u32 pj = w8_lds<u32>(ea + 8u);
    const u32 idx = ((u32)ii - (pj >> 29)) & 7u;
    const u32 dw = w8_lds<u32>(ea + 4u * (idx >> 2));
    ps.pos = pj & 0x1FFFFFFFu;
#pragma unroll
    for (int q4 = 0; q4 < NQ / 4; ++q4) ps.ev[q4] = w8_gtab_load<NQ>(gt, (u32)ii, (dw >> (8 * (idx & 3))) & 0xffu, q4);
    const int take = cnt < 8 ? cnt : 8;
    head = (head + take) & (W8_RING - 1);
    cnt -= take;
}

// ---- THE M-GENERIC BODY (w8m_*) ------------------------------------------------------------------------------------------------------
// w8m_pass_issue, w8m_pass_finish, w8m_scan_range and w8m_scan_items are the functions above with the number of sub-quantizers M as a
// template parameter, M = 8 behind `if constexpr`.  They are instantiated for M = 16 ONLY (wg8_m16_scan_kernel): the sixteen m = 8 kernels
// keep the functions above, untouched.  Instantiating THEM from the M-generic body was tried and changes their register allocation (the same
// instructions in the scan loop, some eighty more around it, other scalar registers spilled) although every M = 8 branch is the same text --
// and these are the kernels every measurement in DESIGN.md was taken with: they must disassemble to the same instructions, one for one.
// Folding the two bodies into one is a change of its own, to be made when it can be timed.
template <int NQ, int M = 8> static __device__ __forceinline__ void w8m_pass_issue(W8Pass<NQ> &ps, u32 cbuf_addr, int &head, int &cnt, __amdgpu_buffer_rsrc_t gt, int lane)
{
    if constexpr (M == 16) {
        // four points per pass, a row of sixteen lanes each.  Parked: the point's code DWORDS rotated (out dword k = code dword
        // (k + jd) mod 4, jd = the parking lane's j / 4 -- the bytes inside a dword stand where they stood, see w8_scan_range) and j in the
        // position word's top four bits
        // (the lane number passes through an opaque move: what is derived from it here -- segment, sub-quantizer, ring and table offsets --
        // is computed where it is used, a few instructions of a rare path, instead of living, spilled, across the scan loop)
        asm volatile("" : "+v"(lane));
        const int seg = lane >> 4, ii = lane & 15;
        ps.ok = seg < cnt;
        const u32 ea = cbuf_addr + (u32)((head + (ps.ok ? seg : 0)) & (W8_RING - 1)) * (5u * 4u);
        const u32 pj = w8_lds<u32>(ea + 16u);
        const u32 k = (((u32)ii >> 2) - (pj >> 30)) & 3u;
        const u32 dw = w8_lds<u32>(ea + 4u * k);
        ps.pos = pj & 0x0FFFFFFFu;
#pragma unroll
        for (int q4 = 0; q4 < NQ / 4; ++q4) ps.ev[q4] = w8_gtab_load<NQ>(gt, (u32)ii, (dw >> (8 * (ii & 3))) & 0xffu, q4);
        const int take = cnt < 4 ? cnt : 4;
        head = (head + take) & (W8_RING - 1);
        cnt -= take;
        return;
    }
    const int seg = lane >> 3, ii = lane & 7;
    ps.ok = seg < cnt;
    const u32 ea = cbuf_addr + (u32)((head + (ps.ok ? seg : 0)) & (W8_RING - 1)) * (W8_ES * 4u);
    // (parked: the point's ROTATED code bytes -- out byte t = code byte (t + j) mod 8, j = the parking lane's rotation, kept in the position
    // word's top three bits: the scan loop holds no unrotated copy of a step's bytes)
    const u32 pj = w8_lds<u32>(ea + 8u);
    const u32 idx = ((u32)ii - (pj >> 29)) & 7u;
    const u32 dw = w8_lds<u32>(ea + 4u * (idx >> 2));
    ps.pos = pj & 0x1FFFFFFFu;
#pragma unroll
    for (int q4 = 0; q4 < NQ / 4; ++q4) ps.ev[q4] = w8_gtab_load<NQ>(gt, (u32)ii, (dw >> (8 * (idx & 3))) & 0xffu, q4);
    const int take = cnt < 8 ? cnt : 8;
    head = (head + take) & (W8_RING - 1);
    cnt -= take;
}

// Works a pass off.  (Measured and dropped: everything the pass needs from LDS -- constants, bounds, a snapshot of every slot's pool, the
// bias arithmetic's operands -- requested in one go ahead of the running sums, the bias computed from registers: 16 384 x w = 8
// 5.87 -> 5.91 ms, w = 1 1.38 -> 1.44.  The pass does not wait for memory -- 260 of its 7 700 cycles, by cycle counters -- it is ~400 dependent
// instructions on a SIMD it shares with three scanning waves.)
template <int NQ, int KP = 1> static __device__ __forceinline__ void w8_pass_finish(const W8Pass<NQ> &ps, int nvalid, int K, int lane)
{
    const int ii = lane & 7;
    float ev[NQ];
#pragma unroll
    for (int s = 0; s < NQ; ++s) ev[s] = ps.ev[s >> 2][s & 3];
    float x[NQ];
#pragma unroll
    for (int s = 0; s < NQ; ++s) x[s] = w8_dc<NQ>(s) + ev[s];
#pragma unroll
    for (int i = 1; i < 8; ++i)
#pragma unroll
        for (int s = 0; s < NQ; ++s) {
            // lane l <- lane l-1 within a row of 16 (row_shr:1): what lane i reads at step i is lane i-1's value of step i-1, so the
            // segment's last lane ends with ((dc + t0) + t1) + ... + t7 (index.jl:242-246)
            const float up = __uint_as_float((u32)__builtin_amdgcn_update_dpp(0, (int)__float_as_uint(x[s]), 0x111, 0xf, 0xf, false));
            x[s] = up + ev[s];
        }
#pragma unroll
    for (int s = 0; s < NQ; ++s) {
        if (s >= nvalid) continue;   // uniform
        // (keys are unique: the exclusive test loses nothing -- a key that IS the bound sits in the pool already, or came from another list)
        const u64 key = make_key(x[s], w8_sbase<NQ>(s) + ps.pos);
        const u64 mask = __builtin_amdgcn_ballot_w64(ps.ok && ii == 7 && key < w8_sthr<NQ>(s));
        if constexpr (KP == 1) {
        if (mask != 0) w8_pool_offer<NQ>(s, w8_pool_read<NQ>(s, K, lane), key, mask, K, lane);   // uniform: most parked points pass for one query of the group
        } else {
            if (mask != 0) w8_pool_offer<NQ, 2>(s, w8_pool_read<NQ, 2>(s, K, lane, 0), key, mask, K, lane, w8_pool_read<NQ, 2>(s, K, lane, 1));
        }
    }
}

template <int NQ, int KP = 1, int M = 8> static __device__ __forceinline__ void w8m_pass_finish(const W8Pass<NQ> &ps, int nvalid, int K, int lane)
{
    const int ii = lane & (M - 1);
    float ev[NQ];
#pragma unroll
    for (int s = 0; s < NQ; ++s) ev[s] = ps.ev[s >> 2][s & 3];
    float x[NQ];
#pragma unroll
    for (int s = 0; s < NQ; ++s) x[s] = w8_dc<NQ>(s) + ev[s];
#pragma unroll
    for (int i = 1; i < M; ++i)
#pragma unroll
        for (int s = 0; s < NQ; ++s) {
            // lane l <- lane l-1 within a row of 16 (row_shr:1): what lane i reads at step i is lane i-1's value of step i-1, so the
            // segment's last lane ends with ((dc + t0) + t1) + ... + t7 (index.jl:242-246; m = 16: a segment is the row, ... + t15)
            const float up = __uint_as_float((u32)__builtin_amdgcn_update_dpp(0, (int)__float_as_uint(x[s]), 0x111, 0xf, 0xf, false));
            x[s] = up + ev[s];
        }
#pragma unroll
    for (int s = 0; s < NQ; ++s) {
        if (s >= nvalid) continue;   // uniform
        // (keys are unique: the exclusive test loses nothing -- a key that IS the bound sits in the pool already, or came from another list)
        const u64 key = make_key(x[s], w8_sbase<NQ>(s) + ps.pos);
        const u64 mask = __builtin_amdgcn_ballot_w64(ps.ok && ii == M - 1 && key < w8_sthr<NQ>(s));
        if constexpr (KP == 1) {
        if (mask != 0) w8_pool_offer<NQ>(s, w8_pool_read<NQ>(s, K, lane), key, mask, K, lane);   // uniform: most parked points pass for one query of the group
        } else {
            if (mask != 0) w8_pool_offer<NQ, 2>(s, w8_pool_read<NQ, 2>(s, K, lane, 0), key, mask, K, lane, w8_pool_read<NQ, 2>(s, K, lane, 1));
        }
    }
}

// ---- the scan of one work item by one wave -----------------------------------------------------------------------------------------------
// K-th smallest integer sum of slot S over the step's four points per lane (radix select, as w8_kth_sum)
static __device__ __attribute__((noinline)) u32 w8_kth_sum4(u32 v0, u32 v1, u32 v2, u32 v3, u32 validbits, int need)
{
    u32 prefix = 0;
#pragma unroll 1
    for (int bit = 14; bit >= 0; --bit) {   // uniform
        const u32 want = prefix >> bit;
        const int c0 = __popcll(__builtin_amdgcn_ballot_w64((validbits & 1u) && (v0 >> bit) == want)) +
                       __popcll(__builtin_amdgcn_ballot_w64((validbits & 2u) && (v1 >> bit) == want)) +
                       __popcll(__builtin_amdgcn_ballot_w64((validbits & 4u) && (v2 >> bit) == want)) +
                       __popcll(__builtin_amdgcn_ballot_w64((validbits & 8u) && (v3 >> bit) == want));
        if (c0 < need) {
            need -= c0;
            prefix |= 1u << bit;
        }
    }
    return prefix;
}

template <int NQ, int KP = 1>
static __device__ __forceinline__ void w8_scan_range(__amdgpu_buffer_rsrc_t codes, u32 p0, u32 p1, int nvalid, int K, int wv, int lane,
                                                     v4u ca, v4u cb, __amdgpu_buffer_rsrc_t gt)
{
    // A step of a wave is 256 points: four per lane in two 16-byte registers sets, ca (points pb + 2 lane, + 1) and cb (pb + 128 + 2 lane,
    // + 1), requested by the caller for the first step.  The code stream comes through a buffer resource over the list: the lane's offset
    // (16 lane) is a constant register, the step's offset a scalar -- a request is ONE instruction and no address arithmetic -- and each half
    // of the NEXT step is requested into its register set the moment this step's half has left it (rotated, four v_perm): two requests
    // of 1 KB per wave are in flight at any time, each with a whole step to arrive, and there is no second register set and no move.
    // (One request per wave -- 4 MB on the chip -- at the loaded latency of HBM is 2 TB/s: the conflict-free scan waited on every step.)
    using L = W8Lds<NQ, KP>;
    constexpr u32 STEP = 256;
    constexpr int NB = NQ / 2;          // accumulator dwords of a point: two 16-bit fields each
    constexpr u32 EB = 2u * NQ, CB = 16u * NQ;   // bytes of a table entry, of a copy's eight entries
    constexpr int CSH = NQ == 8 ? 4 : 3, CMASK = NQ == 8 ? 1 : 3;   // lane -> copy
    const u32 cbuf_addr = L::PARK + (u32)wv * (W8_RING * W8_ES * 4u);
    u32 bias[NB];
    w8_bias<NQ>(nvalid, bias);
    // lane constants: byte rotation of a point's code (out byte t = code byte (t + j) mod 8) and the low address byte of slot t:
    // copy * 8 EB | ((t + j) mod 8) * EB (four copies of 8-byte entries, two of 16-byte ones)
    const int j = lane & 7, cpy = (lane >> CSH) & CMASK;
    u32 rsel0 = 0, rsel1 = 0, ap0 = 0, ap1 = 0;
#pragma unroll
    for (int b = 0; b < 4; ++b) {
        rsel0 |= (u32)((b + j) & 7) << (8 * b);
        rsel1 |= (u32)((4 + b + j) & 7) << (8 * b);
        ap0 |= ((u32)((b + j) & 7) * EB + (u32)cpy * CB) << (8 * b);
        ap1 |= ((u32)((4 + b + j) & 7) * EB + (u32)cpy * CB) << (8 * b);
    }
    // address of slot t = perm{byte 0: lane part of slot t, byte 1: rotated code byte t, bytes 2, 3: zero}
    const u32 asel[4] = {0x0C0C0400u, 0x0C0C0501u, 0x0C0C0602u, 0x0C0C0703u};
    const int lane16 = lane * 16;
    int head = 0, ccnt = 0;
    u32 since = 0;
    bool pend = false;
    W8Pass<NQ> ps;
#pragma unroll
    for (int q4 = 0; q4 < NQ / 4; ++q4) ps.ev[q4] = (v4f){0.f, 0.f, 0.f, 0.f};
    ps.pos = 0;
    ps.ok = false;
    u32 rw[4][2];
    u64 fm[4];
    bool flush = false;
    // A COLD work item (a slot whose query has no bound yet: every point of the first step is a candidate) starts with one exchange between
    // the eight waves: each takes the ceil(K / 8)-th smallest integer sum of ITS first 256 points, T = the largest of the eight -- every
    // wave holds ceil(K / 8) points at or below T, the workgroup K -- and (T + 8) / inv + dc bounds K real distances from above (header):
    // the bound of the 16th-or-so best of 2048 points instead of each wave's own K-th of 256, five times fewer candidates in the steps
    // that follow, and not one exact sum spent on it.  Workgroup-uniform conditions only (the item's own constants in LDS, a range that
    // gives every wave a whole first step), so all eight waves reach the barrier.
    u32 coldmask = 0;
    if (p1 - p0 >= (u32)W8_NW * STEP) {
#pragma unroll
        for (int s = 0; s < NQ; ++s) {
            const float inv = w8_inv<NQ>(s);
            const u32 hh = __builtin_amdgcn_readfirstlane(w8_lds<u32>(L::HARD + 8u * s + 4u));
            if (s < nvalid && hh >= 0x7F800000u && inv > 0.0f && inv < 1.0e30f) coldmask |= 1u << s;
        }
    }
    bool first = true;
    const u32 ptail = p1 > 2u * W8_NW * STEP ? p1 - 2u * W8_NW * STEP : 0u;   // a wave's last two steps start at or behind this point
    for (u32 pb = p0 + wv * STEP;; pb += W8_NW * STEP) {
        bool overflow = false;
        if (pb >= p1) {   // uniform: past the end -- what is still parked gets its sums, then the wave leaves
            if (ccnt == 0 && !pend) break;
            flush = true;
#pragma unroll
            for (int r = 0; r < 4; ++r) fm[r] = 0;
        } else {
            if (__builtin_expect(pend, 0)) {   // uniform: the pass requested during the previous step
                pend = false;
                w8_pass_finish<NQ, KP>(ps, nvalid, K, lane);
                since = 0;
                w8_bias<NQ>(nvalid, bias);   // (the other waves' offers moved the bounds as well)
                if (ccnt >= W8_TRIG || (ccnt > 0 && pb >= ptail)) {   // the next ones are waiting already (or the range ends)
                    w8_pass_issue<NQ>(ps, cbuf_addr, head, ccnt, gt, lane);
                    pend = true;
                }
            } else if (__builtin_expect(ccnt > 0 && pb >= ptail, 0)) {
                // the wave's last two steps: what is parked does not wait for company -- its pass is under way while these steps are
                // scanned, and the end of the range finds an empty ring nine times in ten (a pass worked off THERE is a trip to L2 the
                // wave sits out, with the other seven waiting for it at the barrier behind: the wait was 8 % of the kernel)
                wave_sync();
                w8_pass_issue<NQ>(ps, cbuf_addr, head, ccnt, gt, lane);
                pend = true;
            } else if (++since >= (u32)W8_REFRESH) {
                // the workgroup's bounds move even when this wave has no candidates of its own
                since = 0;
                w8_bias<NQ>(nvalid, bias);
            }
            // the next step's offsets: past the end the wave's current halves are read once more (no branch around a request, no second
            // value for a register set to merge with; a half that starts beyond the list repeats the first one: never a byte beyond the
            // 127 points of slack the four-wave kernels read too)
            const u32 pn = pb + W8_NW * STEP;
            const u32 pa = pn < p1 ? pn : pb;
            const u32 pbb = pa + 128u < p1 ? pa + 128u : pa;
            u32 qa[4][NB];
            auto half = [&](auto hc, v4u &cx, u32 pnext) __attribute__((always_inline)) {
                constexpr int h = decltype(hc)::value;
                // the half's bytes leave its register set rotated (tied together so that no part of them can sink below the request that
                // follows), and the next step's half is requested INTO it
                rw[2 * h][0] = __builtin_amdgcn_perm(cx.y, cx.x, rsel0);
                rw[2 * h][1] = __builtin_amdgcn_perm(cx.y, cx.x, rsel1);
                rw[2 * h + 1][0] = __builtin_amdgcn_perm(cx.w, cx.z, rsel0);
                rw[2 * h + 1][1] = __builtin_amdgcn_perm(cx.w, cx.z, rsel1);
                asm volatile("" : "+v"(rw[2 * h][0]), "+v"(rw[2 * h][1]), "+v"(rw[2 * h + 1][0]), "+v"(rw[2 * h + 1][1]), "+v"(cx));
                cx = __builtin_amdgcn_raw_buffer_load_b128(codes, lane16, (int)(pnext * 8u), W8_STREAM_AUX);
                // the gathers and adds of the half's two points: each form's order is hand-made and measured
                if constexpr (NQ == 8) {
                    // eight gathers (32 registers) in flight: the first point's are issued before the first add; each of its entries, once
                    // summed, hands its registers to the same slot's gather of the second point (one fill and one drain per half)
                    v4u ev[8];
                    static_for<8>([&](auto tc) {
                        constexpr int t = decltype(tc)::value;
                        const u32 ea = w8_perm(rw[2 * h][t >> 2], t < 4 ? ap0 : ap1, asel[t & 3]);
                        ev[t] = lds_load_abs<v4u>(ea);
                    });
                    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                    for (int i = 0; i < 4; ++i) qa[2 * h][i] = bias[i];
                    static_for<8>([&](auto tc) {
                        constexpr int t = decltype(tc)::value;
                        qa[2 * h][0] += ev[t].x;
                        qa[2 * h][1] += ev[t].y;
                        qa[2 * h][2] += ev[t].z;
                        qa[2 * h][3] += ev[t].w;
                        const u32 ea = w8_perm(rw[2 * h + 1][t >> 2], t < 4 ? ap0 : ap1, asel[t & 3]);
                        ev[t] = lds_load_abs<v4u>(ea);
                        __builtin_amdgcn_sched_barrier(0);
                    });
#pragma unroll
                    for (int i = 0; i < 4; ++i) qa[2 * h + 1][i] = bias[i];
#pragma unroll
                    for (int t = 0; t < 8; ++t) {
                        qa[2 * h + 1][0] += ev[t].x;
                        qa[2 * h + 1][1] += ev[t].y;
                        qa[2 * h + 1][2] += ev[t].z;
                        qa[2 * h + 1][3] += ev[t].w;
                    }
                } else {
                    // all sixteen gathers of the half are issued before the first add (left alone the compiler waits after every second read)
                    v2u ev[2][8];
                    static_for<2>([&](auto rc) {
                        constexpr int r = decltype(rc)::value;
                        static_for<8>([&](auto tc) {
                            constexpr int t = decltype(tc)::value;
                            const u32 ea = w8_perm(rw[2 * h + r][t >> 2], t < 4 ? ap0 : ap1, asel[t & 3]);
                            ev[r][t] = lds_load_abs<v2u>(ea);
                        });
                    });
                    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                    for (int r = 0; r < 2; ++r) {
                        qa[2 * h + r][0] = bias[0];
                        qa[2 * h + r][1] = bias[1];
#pragma unroll
                        for (int t = 0; t < 8; ++t) {
                            qa[2 * h + r][0] += ev[r][t].x;
                            qa[2 * h + r][1] += ev[r][t].y;
                        }
                    }
                }
                __builtin_amdgcn_sched_barrier(0);
            };
            half(IntC<0>{}, ca, pa);
            half(IntC<1>{}, cb, pbb);
            // a field below 0x8000 <=> that query's integer sum is within its budget (w8_bias); one compare for the four points
            u32 x[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) x[r] = w8_and(qa[r]);
            u64 anym = __builtin_amdgcn_ballot_w64((((x[0] & x[1]) & (x[2] & x[3])) & 0x80008000u) != 0x80008000u);
            if (__builtin_expect(first && coldmask != 0u, 0)) {   // uniform over the WORKGROUP: see above
                const int r8 = (K + W8_NW - 1) / W8_NW;
                static_for<NQ>([&](auto sc) {
                    constexpr int s = decltype(sc)::value;
                    if ((coldmask >> s) & 1u) {   // uniform
                        // (the slot's bias is 0 while it has no bound: the fields are the sums)
                        u32 f[4];
#pragma unroll
                        for (int r = 0; r < 4; ++r) f[r] = (s & 1) ? (qa[r][s >> 1] >> 16) : (qa[r][s >> 1] & 0xffffu);
                        const u32 V = w8_kth_sum4(f[0], f[1], f[2], f[3], 0xFu, r8);
                        if (lane == 0) *w8_ptr<u32>(L::COLD + L::COLD_SLOT * s + 4u * (u32)wv) = V;
                    }
                });
                __syncthreads();
                static_for<NQ>([&](auto sc) {
                    constexpr int s = decltype(sc)::value;
                    if ((coldmask >> s) & 1u) {   // uniform
                        u32 T = 0;
#pragma unroll
                        for (int v = 0; v < W8_NW; ++v) {
                            const u32 o = __builtin_amdgcn_readfirstlane(w8_lds<u32>(L::COLD + L::COLD_SLOT * s + 4u * (u32)v));
                            T = o > T ? o : T;
                        }
                        const float ub = (w8_dc<NQ>(s) + (float)(T + 8u) * (1.00001f / w8_inv<NQ>(s))) * 1.00002f;
                        // (every wave arrives at the same bound; the wave's own atomic is ahead of its own reads of the word)
                        if (ub < 3.0e38f && lane == 0) atomicMin(w8_ptr<u64>(L::STHR + 8u * s), make_key(ub, 0xFFFFFFFFu));
                    }
                });
                // the step's fields were accumulated under the old bias: re-based on the new one, and the step is tested again
                u32 nb[NB];
                w8_bias<NQ>(nvalid, nb);
#pragma unroll
                for (int r = 0; r < 4; ++r) {
#pragma unroll
                    for (int i = 0; i < NB; ++i) qa[r][i] = qa[r][i] - bias[i] + nb[i];
                    x[r] = w8_and(qa[r]);
                }
#pragma unroll
                for (int i = 0; i < NB; ++i) bias[i] = nb[i];
                anym = __builtin_amdgcn_ballot_w64((((x[0] & x[1]) & (x[2] & x[3])) & 0x80008000u) != 0x80008000u);
            }
            first = false;
            if (__builtin_expect(anym != 0, 0)) {   // uniform; a step in ten once the bounds are tight
                // the lane's four candidate flags; a list's last step masks the points past its end (they carry whatever was loaded)
                bool c[4];
#pragma unroll
                for (int r = 0; r < 4; ++r) c[r] = (x[r] & 0x80008000u) != 0x80008000u;
                const u32 pt0 = pb + (u32)lane * 2u;
                if (pb + STEP > p1) {   // uniform
#pragma unroll
                    for (int r = 0; r < 4; ++r) c[r] = c[r] && pt0 + (u32)(r >> 1) * 128u + (u32)(r & 1) < p1;
                }
                u64 m[4];
                int n[4], ntot = 0;
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    m[r] = __builtin_amdgcn_ballot_w64(c[r]);
                    n[r] = __popcll(m[r]);
                    ntot += n[r];
                }
                // a crowd with no bound at all (a cold work item's first step): bounds from the integer sums first (header)
                if (ntot > 8 && (int)min(p1 - pb, STEP) >= K) {
                    bool moved = false;
                    u32 vb = 0;
#pragma unroll
                    for (int r = 0; r < 4; ++r) vb |= (pt0 + (u32)(r >> 1) * 128u + (u32)(r & 1) < p1) ? (1u << r) : 0u;
                    static_for<NQ>([&](auto sc) {
                        constexpr int s = decltype(sc)::value;
                        const float inv = w8_inv<NQ>(s);
                        // (a scale that is not a normal number -- all-zero or denormal tables -- keeps the plain path)
                        if (s < nvalid && (u32)(w8_sthr<NQ>(s) >> 32) >= 0x7F800000u && inv > 0.0f && inv < 1.0e30f) {   // uniform
                            // the sums themselves: field - bias (no borrow: every field started from its bias)
                            const u32 bs = (s & 1) ? (bias[s >> 1] >> 16) : (bias[s >> 1] & 0xffffu);
                            u32 f[4];
#pragma unroll
                            for (int r = 0; r < 4; ++r) f[r] = ((s & 1) ? (qa[r][s >> 1] >> 16) : (qa[r][s >> 1] & 0xffffu)) - bs;
                            const u32 U = w8_kth_sum4(f[0], f[1], f[2], f[3], vb, K);
                            const float ub = (w8_dc<NQ>(s) + (float)(U + 8u) * (1.00001f / inv)) * 1.00002f;
                            if (ub < 3.0e38f) {
                                if (lane == 0) atomicMin(w8_ptr<u64>(L::STHR + 8u * s), make_key(ub, 0xFFFFFFFFu));
                                moved = true;
                            }
                        }
                    });
                    if (moved) {
                        // the step's fields were accumulated under the old bias: re-based on the new one before they are tested again
                        u32 nb[NB];
                        w8_bias<NQ>(nvalid, nb);
                        ntot = 0;
#pragma unroll
                        for (int r = 0; r < 4; ++r) {
                            const u32 y = w8_and_rebased(qa[r], bias, nb);
                            c[r] = (y & 0x80008000u) != 0x80008000u && ((vb >> r) & 1u) != 0u;
                            m[r] = __builtin_amdgcn_ballot_w64(c[r]);
                            n[r] = __popcll(m[r]);
                            ntot += n[r];
                        }
#pragma unroll
                        for (int i = 0; i < NB; ++i) bias[i] = nb[i];
                    }
                }
                // park (rotated code bytes, position | rotation << 29: positions stay below 2^28, the code stream's byte offsets are 31-bit)
                if (__builtin_expect(ccnt + ntot <= W8_RING, 1)) {
                    int base = head + ccnt;
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        if (n[r] == 0) continue;   // uniform
                        const int rank = (int)__builtin_amdgcn_mbcnt_hi((u32)(m[r] >> 32), __builtin_amdgcn_mbcnt_lo((u32)m[r], 0u));
                        if (c[r]) {
                            u32 *ent = w8_ptr<u32>(cbuf_addr + (u32)((base + rank) & (W8_RING - 1)) * (W8_ES * 4u));
                            ent[0] = rw[r][0];
                            ent[1] = rw[r][1];
                            ent[2] = (pt0 + (u32)(r >> 1) * 128u + (u32)(r & 1)) | ((u32)j << 29);
                        }
                        base += n[r];
                    }
                    ccnt += ntot;
                    // a pass is requested when eight points wait and none is in flight; it is worked off at the top of the next step
                    if (!pend && (ccnt >= W8_TRIG || pb >= ptail)) {
                        wave_sync();
                        w8_pass_issue<NQ>(ps, cbuf_addr, head, ccnt, gt, lane);
                        pend = true;
                    }
                } else {
#pragma unroll
                    for (int r = 0; r < 4; ++r) fm[r] = m[r];
                    overflow = true;
                }
            }
        }
        // No room in the ring (a crowd the integer bound could not thin out), or the end of the range: ONE copy of the code that parks in
        // portions and works passes off here and now (the wave waits for each trip to L2; rare)
        if (__builtin_expect(overflow || flush, 0)) {
            const u32 pt0 = pb + (u32)lane * 2u;
            for (;;) {   // uniform
#pragma unroll 1
                for (int r = 0; r < 4; ++r) {
                    const u64 mm = r == 0 ? fm[0] : (r == 1 ? fm[1] : (r == 2 ? fm[2] : fm[3]));
                    if (mm == 0 || ccnt == W8_RING) continue;
                    const int room = W8_RING - ccnt;
                    const int rank = (int)__builtin_amdgcn_mbcnt_hi((u32)(mm >> 32), __builtin_amdgcn_mbcnt_lo((u32)mm, 0u));
                    const bool mine = ((mm >> lane) & 1ull) != 0 && rank < room;
                    if (mine) {
                        u32 *ent = w8_ptr<u32>(cbuf_addr + (u32)((head + ccnt + rank) & (W8_RING - 1)) * (W8_ES * 4u));
                        ent[0] = r == 0 ? rw[0][0] : (r == 1 ? rw[1][0] : (r == 2 ? rw[2][0] : rw[3][0]));
                        ent[1] = r == 0 ? rw[0][1] : (r == 1 ? rw[1][1] : (r == 2 ? rw[2][1] : rw[3][1]));
                        ent[2] = (pt0 + (u32)(r >> 1) * 128u + (u32)(r & 1)) | ((u32)j << 29);
                    }
                    const u64 took = __builtin_amdgcn_ballot_w64(mine);
                    ccnt += __popcll(took);
                    if (r == 0) fm[0] &= ~took; else if (r == 1) fm[1] &= ~took; else if (r == 2) fm[2] &= ~took; else fm[3] &= ~took;
                }
                const bool more = (fm[0] | fm[1] | fm[2] | fm[3]) != 0;
                if (pend) {
                    pend = false;
                    w8_pass_finish<NQ, KP>(ps, nvalid, K, lane);
                    w8_bias<NQ>(nvalid, bias);
                }
                if (ccnt > 0 && (more || flush || ccnt >= 8)) {
                    wave_sync();
                    w8_pass_issue<NQ>(ps, cbuf_addr, head, ccnt, gt, lane);
                    pend = true;
                    if (more || flush) continue;   // (uniform) worked off at once: room for what is left / nothing may stay behind
                }
                if (!more) break;
            }
            if (flush) break;
        }
    }
}

template <int NQ, int KP = 1, int M = 8>
static __device__ __forceinline__ void w8m_scan_range(__amdgpu_buffer_rsrc_t codes, u32 p0, u32 p1, int nvalid, int K, int wv, int lane,
                                                     v4u ca, v4u cb, v4u cc, v4u cd, __amdgpu_buffer_rsrc_t gt)
{
    // A step of a wave is 256 points: four per lane in two 16-byte registers sets, ca (points pb + 2 lane, + 1) and cb (pb + 128 + 2 lane,
    // + 1), requested by the caller for the first step.  The code stream comes through a buffer resource over the list: the lane's offset
    // (16 lane) is a constant register, the step's offset a scalar -- a request is ONE instruction and no address arithmetic -- and each half
    // of the NEXT step is requested into its register set the moment this step's half has left it (rotated, four v_perm): two requests
    // of 1 KB per wave are in flight at any time, each with a whole step to arrive, and there is no second register set and no move.
    // (One request per wave -- 4 MB on the chip -- at the loaded latency of HBM is 2 TB/s: the conflict-free scan waited on every step.)
    //
    // SIXTEEN SUB-QUANTIZERS (M = 16; wg8_m16_scan_kernel<NQ, DS>).  A point is 16 bytes: one 16-byte request is ONE point per lane, a
    // step keeps its 256 points -- four per lane in FOUR register sets (ca, cc, cb, cd: point pb + 64 r + lane, r = 0 .. 3), each requested in place as above:
    // four requests of 1 KB per wave in flight.  Registers a step holds: the four sets (16), their rotated copies rw (16: what parks), the
    // lane constants (4 address dwords, 4 selectors), the accumulators of the four points (2 NQ) and the gathers in flight (32: NQ = 4
    // all sixteen of a point, NQ = 8 eight at a time, as at m = 8) -- 24 more than the m = 8 forms hold.  The four-query form fits: 128
    // registers, no scratch access in the loop.  The EIGHT-query form with four points per lane did NOT: the compiler spilled inside the
    // loop (23 scratch accesses per step; four gathers in flight instead of eight changed nothing: the pressure was the step's state,
    // not the gathers).  It takes a 128-POINT STEP instead -- two points per lane in the sets ca and cc, two requests of 1 KB in flight
    // (NPT below) -- and its loop is free of scratch accesses too (tests/test_resources_wg8_m16.py).
    // A code's 256-byte row is 2 copies x 16 sub-quantizers x 8 B (NQ = 4) or 16 x 16 B (NQ = 8).  With j = lane mod 16 = 4 jd + jb, lane
    // l looks up, at slot t = 4 td + tb, sub-quantizer sigma(t) = 4 ((td + jd) mod 4) + ((tb + jb) mod 4), in copy (l / 16) mod 2
    // (NQ = 4): for a fixed slot sigma is one-to-one in j, so the 32 lanes of a ds_read_b64 service group read 16 sub-quantizers x 2
    // copies = 32 different bank pairs, and the 16-lane service groups of a ds_read_b128 -- {0-3, 12-15, 20-27}, {4-11, 16-19, 28-31},
    // + 32: sixteen different j each -- read sixteen different four-bank groups, whatever the codes are.  A byte rotation by j across 16
    // bytes would take a v_perm per output dword and a lane-dependent choice of its two source dwords; sigma needs only the DWORDS rotated by
    // jd (two rounds of four selects per point: by jd's low bit, then by its high bit) -- the byte inside the dword is picked by the
    // address perm itself, whose selector is a lane constant in a vector register: ONE v_perm_b32 per lookup, as at m = 8.
    using L = W8Lds<NQ, KP, M>;
    // NPT: the step's points per lane.  Four (a 256-point step) with four queries; TWO with eight -- a 128-point step in the sets ca and cc:
    // with four points the eight-query step holds 24 registers more than at m = 8 (two more sets, their rotated copies, 16-byte code
    // words) and the compiler spilled inside the loop, the fourth set right behind its request.  Everything below that speaks of the
    // step takes STEP = 64 NPT points: the cold-start exchange (every wave's ceil(K / 8)-th smallest sum of its first STEP points:
    // ceil(K / 8) <= 8 <= 128), the crowd bound (the K-th sum of a step: K <= 64 <= 128), the tail (a wave's last two steps), the caller's
    // first requests.  Points r >= NPT do not exist: their flags and masks are constants the compiler folds.
    constexpr int NPT = NQ == 8 ? 2 : 4;
    constexpr u32 STEP = 64u * NPT;
    static_assert(M == 16, "the M-generic body is instantiated for M = 16 only");
    static_assert((W8_NW + 64 - 1) / W8_NW <= (int)STEP && 64 <= (int)STEP, "the cold-start bounds take the ceil(K / 8)-th and the K-th of a step's sums, K <= 64");
    constexpr int NB = NQ / 2;          // accumulator dwords of a point: two 16-bit fields each
    constexpr u32 EB = 2u * NQ, CB = 2u * M * NQ;   // bytes of a table entry, of a copy's M entries
    constexpr int CSH = M == 16 ? 4 : (NQ == 8 ? 4 : 3), CMASK = M == 16 ? (NQ == 8 ? 0 : 1) : (NQ == 8 ? 1 : 3);   // lane -> copy
    static_assert((u32)(CMASK + 1) * CB == 256u, "a code's row is 256 bytes: the 64 banks once");
    constexpr u32 ES = L::ES;
    const u32 cbuf_addr = L::PARK + (u32)wv * (W8_RING * ES * 4u);
    u32 bias[NB];
    w8_bias<NQ>(nvalid, bias);
    // lane constants: byte rotation of a point's code (out byte t = code byte (t + j) mod 8) and the low address byte of slot t:
    // copy * 8 EB | ((t + j) mod 8) * EB (four copies of 8-byte entries, two of 16-byte ones)
    const int j = lane & (M - 1), cpy = (lane >> CSH) & CMASK;
    u32 rsel0 = 0, rsel1 = 0, ap0 = 0, ap1 = 0;
    // (m = 16: apv[td] byte tb = the low address byte of slot 4 td + tb, copy * CB | sigma * EB; aselv[tb] = the address perm's selector)
    u32 apv[4] = {0u, 0u, 0u, 0u}, aselv[4] = {0u, 0u, 0u, 0u};
    if constexpr (M == 16) {
        const int jd = j >> 2, jb = j & 3;
#pragma unroll
        for (int td = 0; td < 4; ++td)
#pragma unroll
            for (int tb = 0; tb < 4; ++tb)
                apv[td] |= ((u32)(4 * ((td + jd) & 3) + ((tb + jb) & 3)) * EB + (u32)cpy * CB) << (8 * tb);
#pragma unroll
        for (int tb = 0; tb < 4; ++tb) aselv[tb] = 0x0C0C0000u | ((4u + (u32)((tb + jb) & 3)) << 8) | (u32)tb;
    } else {
#pragma unroll
    for (int b = 0; b < 4; ++b) {
        rsel0 |= (u32)((b + j) & 7) << (8 * b);
        rsel1 |= (u32)((4 + b + j) & 7) << (8 * b);
        ap0 |= ((u32)((b + j) & 7) * EB + (u32)cpy * CB) << (8 * b);
        ap1 |= ((u32)((4 + b + j) & 7) * EB + (u32)cpy * CB) << (8 * b);
    }
    }
    const bool jlo = (j & 4) != 0, jhi = (j & 8) != 0;   // (m = 16) the dword rotation's two rounds
    // address of slot t = perm{byte 0: lane part of slot t, byte 1: rotated code byte t, bytes 2, 3: zero}
    const u32 asel[4] = {0x0C0C0400u, 0x0C0C0501u, 0x0C0C0602u, 0x0C0C0703u};
    const int lane16 = lane * 16;
    int head = 0, ccnt = 0;
    u32 since = 0;
    bool pend = false;
    W8Pass<NQ> ps;
#pragma unroll
    for (int q4 = 0; q4 < NQ / 4; ++q4) ps.ev[q4] = (v4f){0.f, 0.f, 0.f, 0.f};
    ps.pos = 0;
    ps.ok = false;
    u32 rw[4][M / 4] = {};
    u64 fm[4] = {0, 0, 0, 0};
    bool flush = false;
    // A COLD work item (a slot whose query has no bound yet: every point of the first step is a candidate) starts with one exchange between
    // the eight waves: each takes the ceil(K / 8)-th smallest integer sum of ITS first 256 points, T = the largest of the eight -- every
    // wave holds ceil(K / 8) points at or below T, the workgroup K -- and (T + 8) / inv + dc bounds K real distances from above (header):
    // the bound of the 16th-or-so best of 2048 points instead of each wave's own K-th of 256, five times fewer candidates in the steps
    // that follow, and not one exact sum spent on it.  Workgroup-uniform conditions only (the item's own constants in LDS, a range that
    // gives every wave a whole first step), so all eight waves reach the barrier.
    u32 coldmask = 0;
    if (p1 - p0 >= (u32)W8_NW * STEP) {
#pragma unroll
        for (int s = 0; s < NQ; ++s) {
            const float inv = w8_inv<NQ>(s);
            const u32 hh = __builtin_amdgcn_readfirstlane(w8_lds<u32>(L::HARD + 8u * s + 4u));
            if (s < nvalid && hh >= 0x7F800000u && inv > 0.0f && inv < 1.0e30f) coldmask |= 1u << s;
        }
    }
    // the list position of the lane's r-th point of the step that starts at pb
    auto pidx = [&](u32 pb, int r) __attribute__((always_inline)) -> u32 {
        if constexpr (M == 16) return pb + 64u * (u32)r + (u32)lane;
        else return pb + (u32)lane * 2u + (u32)(r >> 1) * 128u + (u32)(r & 1);
    };
    constexpr int PP = w8_pp<M>;      // points a pass takes, and the parked points that trigger one
    static_assert(w8_pp<8> == W8_TRIG, "m = 8: a pass takes the eight points that trigger it");
    constexpr u32 JSH = M == 16 ? 28u : 29u;   // the parking lane's j in the position word's top bits
    bool first = true;
    const u32 ptail = p1 > 2u * W8_NW * STEP ? p1 - 2u * W8_NW * STEP : 0u;   // a wave's last two steps start at or behind this point
    for (u32 pb = p0 + wv * STEP;; pb += W8_NW * STEP) {
        bool overflow = false;
        if (pb >= p1) {   // uniform: past the end -- what is still parked gets its sums, then the wave leaves
            if (ccnt == 0 && !pend) break;
            flush = true;
#pragma unroll
            for (int r = 0; r < 4; ++r) fm[r] = 0;
        } else {
            if (__builtin_expect(pend, 0)) {   // uniform: the pass requested during the previous step
                pend = false;
                w8m_pass_finish<NQ, KP, M>(ps, nvalid, K, lane);
                since = 0;
                w8_bias<NQ>(nvalid, bias);   // (the other waves' offers moved the bounds as well)
                if (ccnt >= PP || (ccnt > 0 && pb >= ptail)) {   // the next ones are waiting already (or the range ends)
                    w8m_pass_issue<NQ, M>(ps, cbuf_addr, head, ccnt, gt, lane);
                    pend = true;
                }
            } else if (__builtin_expect(ccnt > 0 && pb >= ptail, 0)) {
                // the wave's last two steps: what is parked does not wait for company -- its pass is under way while these steps are
                // scanned, and the end of the range finds an empty ring nine times in ten (a pass worked off THERE is a trip to L2 the
                // wave sits out, with the other seven waiting for it at the barrier behind: the wait was 8 % of the kernel)
                wave_sync();
                w8m_pass_issue<NQ, M>(ps, cbuf_addr, head, ccnt, gt, lane);
                pend = true;
            } else if (++since >= (u32)W8_REFRESH) {
                // the workgroup's bounds move even when this wave has no candidates of its own
                since = 0;
                w8_bias<NQ>(nvalid, bias);
            }
            // the next step's offsets: past the end the wave's current halves are read once more (no branch around a request, no second
            // value for a register set to merge with; a half that starts beyond the list repeats the first one: never a byte beyond the
            // 127 points of slack the four-wave kernels read too)
            const u32 pn = pb + W8_NW * STEP;
            const u32 pa = pn < p1 ? pn : pb;
            const u32 pbb = pa + 128u < p1 ? pa + 128u : pa;
            u32 qa[4][NB] = {};
            auto half = [&](auto hc, v4u &cx, u32 pnext) __attribute__((always_inline)) {
                constexpr int h = decltype(hc)::value;
                // the half's bytes leave its register set rotated (tied together so that no part of them can sink below the request that
                // follows), and the next step's half is requested INTO it
                rw[2 * h][0] = __builtin_amdgcn_perm(cx.y, cx.x, rsel0);
                rw[2 * h][1] = __builtin_amdgcn_perm(cx.y, cx.x, rsel1);
                rw[2 * h + 1][0] = __builtin_amdgcn_perm(cx.w, cx.z, rsel0);
                rw[2 * h + 1][1] = __builtin_amdgcn_perm(cx.w, cx.z, rsel1);
                asm volatile("" : "+v"(rw[2 * h][0]), "+v"(rw[2 * h][1]), "+v"(rw[2 * h + 1][0]), "+v"(rw[2 * h + 1][1]), "+v"(cx));
                cx = __builtin_amdgcn_raw_buffer_load_b128(codes, lane16, (int)(pnext * 8u), W8_STREAM_AUX);
                // the gathers and adds of the half's two points: each form's order is hand-made and measured
                if constexpr (NQ == 8) {
                    // eight gathers (32 registers) in flight: the first point's are issued before the first add; each of its entries, once
                    // summed, hands its registers to the same slot's gather of the second point (one fill and one drain per half)
                    v4u ev[8];
                    static_for<8>([&](auto tc) {
                        constexpr int t = decltype(tc)::value;
                        const u32 ea = w8_perm(rw[2 * h][t >> 2], t < 4 ? ap0 : ap1, asel[t & 3]);
                        ev[t] = lds_load_abs<v4u>(ea);
                    });
                    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                    for (int i = 0; i < 4; ++i) qa[2 * h][i] = bias[i];
                    static_for<8>([&](auto tc) {
                        constexpr int t = decltype(tc)::value;
                        qa[2 * h][0] += ev[t].x;
                        qa[2 * h][1] += ev[t].y;
                        qa[2 * h][2] += ev[t].z;
                        qa[2 * h][3] += ev[t].w;
                        const u32 ea = w8_perm(rw[2 * h + 1][t >> 2], t < 4 ? ap0 : ap1, asel[t & 3]);
                        ev[t] = lds_load_abs<v4u>(ea);
                        __builtin_amdgcn_sched_barrier(0);
                    });
#pragma unroll
                    for (int i = 0; i < 4; ++i) qa[2 * h + 1][i] = bias[i];
#pragma unroll
                    for (int t = 0; t < 8; ++t) {
                        qa[2 * h + 1][0] += ev[t].x;
                        qa[2 * h + 1][1] += ev[t].y;
                        qa[2 * h + 1][2] += ev[t].z;
                        qa[2 * h + 1][3] += ev[t].w;
                    }
                } else {
                    // all sixteen gathers of the half are issued before the first add (left alone the compiler waits after every second read)
                    v2u ev[2][8];
                    static_for<2>([&](auto rc) {
                        constexpr int r = decltype(rc)::value;
                        static_for<8>([&](auto tc) {
                            constexpr int t = decltype(tc)::value;
                            const u32 ea = w8_perm(rw[2 * h + r][t >> 2], t < 4 ? ap0 : ap1, asel[t & 3]);
                            ev[r][t] = lds_load_abs<v2u>(ea);
                        });
                    });
                    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                    for (int r = 0; r < 2; ++r) {
                        qa[2 * h + r][0] = bias[0];
                        qa[2 * h + r][1] = bias[1];
#pragma unroll
                        for (int t = 0; t < 8; ++t) {
                            qa[2 * h + r][0] += ev[r][t].x;
                            qa[2 * h + r][1] += ev[r][t].y;
                        }
                    }
                }
                __builtin_amdgcn_sched_barrier(0);
            };
            // (m = 16) a quarter of the step: ONE point per lane.  The set's dwords leave it rotated by jd, the next step's quarter is
            // requested into it, then the point's sixteen lookups
            auto quarter = [&](auto rc, v4u &cx, u32 pnext) __attribute__((always_inline)) {
                constexpr int r = decltype(rc)::value;
                {
                    const u32 d0 = jlo ? cx.y : cx.x, d1 = jlo ? cx.z : cx.y, d2 = jlo ? cx.w : cx.z, d3 = jlo ? cx.x : cx.w;
                    rw[r][0] = jhi ? d2 : d0;
                    rw[r][1] = jhi ? d3 : d1;
                    rw[r][2] = jhi ? d0 : d2;
                    rw[r][3] = jhi ? d1 : d3;
                }
                asm volatile("" : "+v"(rw[r][0]), "+v"(rw[r][1]), "+v"(rw[r][2]), "+v"(rw[r][3]), "+v"(cx));
                // (the lane's offset is formed here from the lane number, one shift per request: held in a register of its own across the
                // loop it was the one value the eight-query form still spilled)
                int lq = lane;
                asm volatile("" : "+v"(lq));
                cx = __builtin_amdgcn_raw_buffer_load_b128(codes, lq * 16, (int)(pnext * 16u), W8_STREAM_AUX);
                if constexpr (NQ == 8) {
                    // eight gathers (32 registers) in flight: slots 0 .. 7 are issued before the first add; each entry, once summed, hands its
                    // registers to the gather of slot t + 8 (one fill and one drain per point)
                    v4u ev[8];
                    static_for<8>([&](auto tc) {
                        constexpr int t = decltype(tc)::value;
                        ev[t] = lds_load_abs<v4u>(w8_permv(rw[r][t >> 2], apv[t >> 2], aselv[t & 3]));
                    });
                    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                    for (int i = 0; i < 4; ++i) qa[r][i] = bias[i];
                    static_for<8>([&](auto tc) {
                        constexpr int t = decltype(tc)::value;
                        qa[r][0] += ev[t].x;
                        qa[r][1] += ev[t].y;
                        qa[r][2] += ev[t].z;
                        qa[r][3] += ev[t].w;
                        ev[t] = lds_load_abs<v4u>(w8_permv(rw[r][2 + (t >> 2)], apv[2 + (t >> 2)], aselv[t & 3]));
                        __builtin_amdgcn_sched_barrier(0);
                    });
#pragma unroll
                    for (int t = 0; t < 8; ++t) {
                        qa[r][0] += ev[t].x;
                        qa[r][1] += ev[t].y;
                        qa[r][2] += ev[t].z;
                        qa[r][3] += ev[t].w;
                    }
                } else {
                    // all sixteen gathers of the point are issued before the first add
                    v2u ev[16];
                    static_for<16>([&](auto tc) {
                        constexpr int t = decltype(tc)::value;
                        ev[t] = lds_load_abs<v2u>(w8_permv(rw[r][t >> 2], apv[t >> 2], aselv[t & 3]));
                    });
                    __builtin_amdgcn_sched_barrier(0);
                    qa[r][0] = bias[0];
                    qa[r][1] = bias[1];
#pragma unroll
                    for (int t = 0; t < 16; ++t) {
                        qa[r][0] += ev[t].x;
                        qa[r][1] += ev[t].y;
                    }
                }
                __builtin_amdgcn_sched_barrier(0);
            };
            if constexpr (M == 16) {
                // (a quarter that starts beyond the list repeats the first one: never a byte beyond the 63 points -- 1 008 bytes -- of slack
                // behind a request that starts inside the list, less than the 127 x 8 bytes the m = 8 forms read)
                quarter(IntC<0>{}, ca, pa);
                quarter(IntC<1>{}, cc, pa + 64u < p1 ? pa + 64u : pa);
                if constexpr (NPT == 4) {
                    quarter(IntC<2>{}, cb, pbb);
                    quarter(IntC<3>{}, cd, pa + 192u < p1 ? pa + 192u : pa);
                }
            } else {
            half(IntC<0>{}, ca, pa);
            half(IntC<1>{}, cb, pbb);
            }
            // a field below 0x8000 <=> that query's integer sum is within its budget (w8_bias); one compare for the four points
            u32 x[4] = {0x80008000u, 0x80008000u, 0x80008000u, 0x80008000u};   // (a point that does not exist is no candidate)
#pragma unroll
            for (int r = 0; r < NPT; ++r) x[r] = w8_and(qa[r]);
            u64 anym = __builtin_amdgcn_ballot_w64((((x[0] & x[1]) & (x[2] & x[3])) & 0x80008000u) != 0x80008000u);
            if (__builtin_expect(first && coldmask != 0u, 0)) {   // uniform over the WORKGROUP: see above
                const int r8 = (K + W8_NW - 1) / W8_NW;
                static_for<NQ>([&](auto sc) {
                    constexpr int s = decltype(sc)::value;
                    if ((coldmask >> s) & 1u) {   // uniform
                        // (the slot's bias is 0 while it has no bound: the fields are the sums)
                        u32 f[4] = {0u, 0u, 0u, 0u};
#pragma unroll
                        for (int r = 0; r < NPT; ++r) f[r] = (s & 1) ? (qa[r][s >> 1] >> 16) : (qa[r][s >> 1] & 0xffffu);
                        const u32 V = w8_kth_sum4(f[0], f[1], f[2], f[3], (1u << NPT) - 1u, r8);
                        if (lane == 0) *w8_ptr<u32>(L::COLD + L::COLD_SLOT * s + 4u * (u32)wv) = V;
                    }
                });
                __syncthreads();
                static_for<NQ>([&](auto sc) {
                    constexpr int s = decltype(sc)::value;
                    if ((coldmask >> s) & 1u) {   // uniform
                        u32 T = 0;
#pragma unroll
                        for (int v = 0; v < W8_NW; ++v) {
                            const u32 o = __builtin_amdgcn_readfirstlane(w8_lds<u32>(L::COLD + L::COLD_SLOT * s + 4u * (u32)v));
                            T = o > T ? o : T;
                        }
                        const float ub = (w8_dc<NQ>(s) + (float)(T + (u32)M) * (1.00001f / w8_inv<NQ>(s))) * 1.00002f;
                        // (every wave arrives at the same bound; the wave's own atomic is ahead of its own reads of the word)
                        if (ub < 3.0e38f && lane == 0) atomicMin(w8_ptr<u64>(L::STHR + 8u * s), make_key(ub, 0xFFFFFFFFu));
                    }
                });
                // the step's fields were accumulated under the old bias: re-based on the new one, and the step is tested again
                u32 nb[NB];
                w8_bias<NQ>(nvalid, nb);
#pragma unroll
                for (int r = 0; r < NPT; ++r) {
#pragma unroll
                    for (int i = 0; i < NB; ++i) qa[r][i] = qa[r][i] - bias[i] + nb[i];
                    x[r] = w8_and(qa[r]);
                }
#pragma unroll
                for (int i = 0; i < NB; ++i) bias[i] = nb[i];
                anym = __builtin_amdgcn_ballot_w64((((x[0] & x[1]) & (x[2] & x[3])) & 0x80008000u) != 0x80008000u);
            }
            first = false;
            if (__builtin_expect(anym != 0, 0)) {   // uniform; a step in ten once the bounds are tight
                // the lane's four candidate flags; a list's last step masks the points past its end (they carry whatever was loaded)
                bool c[4] = {false, false, false, false};
#pragma unroll
                for (int r = 0; r < NPT; ++r) c[r] = (x[r] & 0x80008000u) != 0x80008000u;
                if (pb + STEP > p1) {   // uniform
#pragma unroll
                    for (int r = 0; r < NPT; ++r) c[r] = c[r] && pidx(pb, r) < p1;
                }
                u64 m[4] = {0, 0, 0, 0};
                int n[4] = {0, 0, 0, 0}, ntot = 0;
#pragma unroll
                for (int r = 0; r < NPT; ++r) {
                    m[r] = __builtin_amdgcn_ballot_w64(c[r]);
                    n[r] = __popcll(m[r]);
                    ntot += n[r];
                }
                // a crowd with no bound at all (a cold work item's first step): bounds from the integer sums first (header)
                if (ntot > 8 && (int)min(p1 - pb, STEP) >= K) {
                    bool moved = false;
                    u32 vb = 0;
#pragma unroll
                    for (int r = 0; r < NPT; ++r) vb |= (pidx(pb, r) < p1) ? (1u << r) : 0u;
                    static_for<NQ>([&](auto sc) {
                        constexpr int s = decltype(sc)::value;
                        const float inv = w8_inv<NQ>(s);
                        // (a scale that is not a normal number -- all-zero or denormal tables -- keeps the plain path)
                        if (s < nvalid && (u32)(w8_sthr<NQ>(s) >> 32) >= 0x7F800000u && inv > 0.0f && inv < 1.0e30f) {   // uniform
                            // the sums themselves: field - bias (no borrow: every field started from its bias)
                            const u32 bs = (s & 1) ? (bias[s >> 1] >> 16) : (bias[s >> 1] & 0xffffu);
                            u32 f[4] = {0u, 0u, 0u, 0u};
#pragma unroll
                            for (int r = 0; r < NPT; ++r) f[r] = ((s & 1) ? (qa[r][s >> 1] >> 16) : (qa[r][s >> 1] & 0xffffu)) - bs;
                            const u32 U = w8_kth_sum4(f[0], f[1], f[2], f[3], vb, K);
                            const float ub = (w8_dc<NQ>(s) + (float)(U + (u32)M) * (1.00001f / inv)) * 1.00002f;
                            if (ub < 3.0e38f) {
                                if (lane == 0) atomicMin(w8_ptr<u64>(L::STHR + 8u * s), make_key(ub, 0xFFFFFFFFu));
                                moved = true;
                            }
                        }
                    });
                    if (moved) {
                        // the step's fields were accumulated under the old bias: re-based on the new one before they are tested again
                        u32 nb[NB];
                        w8_bias<NQ>(nvalid, nb);
                        ntot = 0;
#pragma unroll
                        for (int r = 0; r < NPT; ++r) {
                            const u32 y = w8_and_rebased(qa[r], bias, nb);
                            c[r] = (y & 0x80008000u) != 0x80008000u && ((vb >> r) & 1u) != 0u;
                            m[r] = __builtin_amdgcn_ballot_w64(c[r]);
                            n[r] = __popcll(m[r]);
                            ntot += n[r];
                        }
#pragma unroll
                        for (int i = 0; i < NB; ++i) bias[i] = nb[i];
                    }
                }
                // park (rotated code bytes, position | rotation << 29: positions stay below 2^28, the code stream's byte offsets are 31-bit)
                if (__builtin_expect(ccnt + ntot <= W8_RING, 1)) {
                    int base = head + ccnt;
#pragma unroll
                    for (int r = 0; r < NPT; ++r) {
                        if (n[r] == 0) continue;   // uniform
                        const int rank = (int)__builtin_amdgcn_mbcnt_hi((u32)(m[r] >> 32), __builtin_amdgcn_mbcnt_lo((u32)m[r], 0u));
                        if (c[r]) {
                            u32 *ent = w8_ptr<u32>(cbuf_addr + (u32)((base + rank) & (W8_RING - 1)) * (ES * 4u));
#pragma unroll
                            for (int k = 0; k < M / 4; ++k) ent[k] = rw[r][k];
                            ent[M / 4] = pidx(pb, r) | ((u32)j << JSH);
                        }
                        base += n[r];
                    }
                    ccnt += ntot;
                    // a pass is requested when eight points wait and none is in flight; it is worked off at the top of the next step
                    if (!pend && (ccnt >= PP || pb >= ptail)) {
                        wave_sync();
                        w8m_pass_issue<NQ, M>(ps, cbuf_addr, head, ccnt, gt, lane);
                        pend = true;
                    }
                } else {
#pragma unroll
                    for (int r = 0; r < 4; ++r) fm[r] = m[r];
                    overflow = true;
                }
            }
        }
        // No room in the ring (a crowd the integer bound could not thin out), or the end of the range: ONE copy of the code that parks in
        // portions and works passes off here and now (the wave waits for each trip to L2; rare)
        if (__builtin_expect(overflow || flush, 0)) {
            for (;;) {   // uniform
#pragma unroll 1
                for (int r = 0; r < NPT; ++r) {
                    const u64 mm = r == 0 ? fm[0] : (r == 1 ? fm[1] : (r == 2 ? fm[2] : fm[3]));
                    if (mm == 0 || ccnt == W8_RING) continue;
                    const int room = W8_RING - ccnt;
                    const int rank = (int)__builtin_amdgcn_mbcnt_hi((u32)(mm >> 32), __builtin_amdgcn_mbcnt_lo((u32)mm, 0u));
                    const bool mine = ((mm >> lane) & 1ull) != 0 && rank < room;
                    if (mine) {
                        u32 *ent = w8_ptr<u32>(cbuf_addr + (u32)((head + ccnt + rank) & (W8_RING - 1)) * (ES * 4u));
#pragma unroll
                        for (int k = 0; k < M / 4; ++k) ent[k] = r == 0 ? rw[0][k] : (r == 1 ? rw[1][k] : (r == 2 ? rw[2][k] : rw[3][k]));
                        ent[M / 4] = pidx(pb, r) | ((u32)j << JSH);
                    }
                    const u64 took = __builtin_amdgcn_ballot_w64(mine);
                    ccnt += __popcll(took);
                    if (r == 0) fm[0] &= ~took; else if (r == 1) fm[1] &= ~took; else if (r == 2) fm[2] &= ~took; else fm[3] &= ~took;
                }
                const bool more = (fm[0] | fm[1] | fm[2] | fm[3]) != 0;
                if (pend) {
                    pend = false;
                    w8m_pass_finish<NQ, KP, M>(ps, nvalid, K, lane);
                    w8_bias<NQ>(nvalid, bias);
                }
                if (ccnt > 0 && (more || flush || ccnt >= PP)) {
                    wave_sync();
                    w8m_pass_issue<NQ, M>(ps, cbuf_addr, head, ccnt, gt, lane);
                    pend = true;
                    if (more || flush) continue;   // (uniform) worked off at once: room for what is left / nothing may stay behind
                }
                if (!more) break;
            }
            if (flush) break;
        }
    }
}

// ---- the kernel ---------------------------------------------------------------------------------------------------------------------
// item_list[i] = the list of work item i (bucket_scan_kernel writes it next to wi_off: one load instead of a 13-step binary search
// of dependent loads per work item)
// xq: nranges work-queue heads, 64 B apart, zero at launch.  Work items are ordered by list, so the four or five groups of one list are
// neighbours in the queue: the item range is cut into one contiguous part per XCD and a workgroup pulls from the part of the XCD it runs
// on (HW_REG_XCC_ID) -- the groups that stream the same list then run side by side under ONE L2 and the list crosses the fabric once.
// Placement is a matter of speed only: a workgroup whose part is exhausted moves on to the next one; every wave leaves when all are.
template <int NQ, int DS, int KP = 1>
static __device__ __forceinline__ void w8_scan_items(const ScanArgs &a, float *__restrict__ gtabs, const u32 *__restrict__ item_list,
                                                     u32 *__restrict__ xq, int nranges)
{
    using L = W8Lds<NQ, KP>;
    static_assert(w8_ds_ok(DS), "sub-spaces of 4, 8, 12 or 16 dimensions");
    static_assert(8u * W8_RES_STRIDE<NQ, DS> * 4u <= L::SMAX - L::RES, "the residuals fit the block sized for DS = 16");
    constexpr int D = 8 * DS;               // m = 8
    constexpr u32 RS = W8_RES_STRIDE<NQ, DS>;
    constexpr int G = DS / 4;               // 16-byte groups of a codeword
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const IndexView &ix = a.ix;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);     // (a scalar: branches on the wave's number and its position in the list are scalar branches)
    const int K = a.K;
    float *res = (float *)(smem + L::RES);
    u32 *smax = (u32 *)(smem + L::SMAX);
    float *sinv = (float *)(smem + L::SMAX) + NQ;
    float *sdc = (float *)(smem + L::QC);
    u32 *ssb = (u32 *)(smem + L::QC) + NQ;
    u32 *spi = (u32 *)(smem + L::QC) + 2 * NQ;
    u32 *sqi = (u32 *)(smem + L::QC) + 3 * NQ;
    u64 *shard = (u64 *)(smem + L::HARD);
    u64 *sthr = (u64 *)(smem + L::STHR);
    u32 *swi = (u32 *)(smem + L::SWI);
    const u32 total = a.wi_off[ix.kc];
    float *gt = gtabs + (size_t)blockIdx.x * W8_GTAB_FLOATS<NQ>;
    const __amdgpu_buffer_rsrc_t gtr = __builtin_amdgcn_make_buffer_rsrc((void *)gt, 0, (int)(W8_GTAB_FLOATS<NQ> * 4u), 0x00020000);

    u64 *pool = (u64 *)(smem + L::POOL);
    // (thread 0's: the part it pulls from, the parts found empty so far)
    int qcur = nranges > 1 ? (int)(__builtin_amdgcn_s_getreg(20 | (3 << 11)) & 7u) : 0, qtried = 0;
    // the item behind ticket k of the current part; a part that is exhausted hands over to the next one (a trip per part: the tail only)
    auto resolve = [&](u32 k) -> u32 {
        for (;;) {
            // (nranges is 8 or 1: no division -- this runs between two barriers of every work item)
            const u32 r0 = nranges == 1 ? 0u : (u32)(((u64)total * (u32)qcur) >> 3), r1 = nranges == 1 ? total : (u32)(((u64)total * (u32)(qcur + 1)) >> 3);
            if (k < r1 - r0) return r0 + k;
            qcur = qcur + 1 == nranges ? 0 : qcur + 1;
            if (++qtried >= nranges) return 0xFFFFFFFFu;
            k = atomicAdd(xq + qcur * 16, 1u);
        }
    };
    if (tid == 0) swi[0] = resolve(atomicAdd(xq + qcur * 16, 1u));
    __syncthreads();
    u32 wi = __builtin_amdgcn_readfirstlane(swi[0]);
    for (;;) {
        if (wi >= total) break;   // uniform: every wave of every workgroup reaches this
        // the NEXT work item's ticket is pulled now and looked at when this one is done: the atomic's trip is off the critical path
        u32 pulled = 0;
        if (tid == 0 && qtried < nranges) pulled = atomicAdd(xq + qcur * 16, 1u);
        do {   // (one trip: `break` = this work item is finished)
        const int l = __builtin_amdgcn_readfirstlane((int)item_list[wi]);
        const u32 cnt = __builtin_amdgcn_readfirstlane(a.list_cnt[l]);
        const u32 ng = (cnt + (u32)(NQ - 1)) / (u32)NQ;
        const u32 local = wi - __builtin_amdgcn_readfirstlane(a.wi_off[l]);
        const u32 chunk = local / ng, grp = local - chunk * ng;
        const u32 len = __builtin_amdgcn_readfirstlane(ix.list_len[l]);
        const u32 p0 = chunk * a.CH;
        if (p0 >= len) break;   // uniform
        const u32 p1 = min(len, p0 + a.CH);
        const int nvalid = min(NQ, (int)(cnt - grp * (u32)NQ));

        // the queries of the group: thread s < NQ fetches slot s (slots past nvalid repeat slot 0 and can never be candidates)
        if (tid < NQ) {
            const int ss = tid < nvalid ? tid : 0;
            const u32 pi = a.bucket_items[a.bucket_off[l] + grp * (u32)NQ + ss];
            const u32 qq = pi / (u32)a.w;
            spi[tid] = pi;
            sqi[tid] = qq;
            ssb[tid] = a.probe_base[pi];
            sdc[tid] = a.probe_dc[pi];
            const u64 t0 = __hip_atomic_load(&a.qthr[qq], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            shard[tid] = t0;
            sthr[tid] = t0;
            smax[tid] = 0u;
        }
        // (the pool's 64 NQ entries: the workgroup's last threads, which fetch no slot)
        if constexpr (KP == 1) {
        if (tid >= W8_THREADS - 64 * NQ && tid < W8_THREADS) pool[tid - (W8_THREADS - 64 * NQ)] = KEY_MAX;
        } else {
            // (the wide pool's 128 NQ entries: one or two per thread)
#pragma unroll
            for (int i = 0; i < 128 * NQ / W8_THREADS; ++i) pool[tid + i * W8_THREADS] = KEY_MAX;
        }
        __syncthreads();
        // exact pruning of whole work items, as in scan_kernel: no sum of this list lies below its coarse distance
        if (a.prune) {
            bool all = true;
#pragma unroll
            for (int s = 0; s < NQ; ++s)
                all = all && (s >= nvalid || __builtin_amdgcn_readfirstlane(__float_as_uint(sdc[s])) > (u32)(readfirstlane64(shard[s]) >> 32));
            if (all) {   // uniform
                if (tid < nvalid) {
                    const u32 pi = spi[tid];
                    a.part_cnt[(size_t)pi * a.maxch + chunk] = 0u;
                    atomicAdd(a.scanned_points + (size_t)(pi & 63u) * 8 + 1, (u64)(p1 - p0));
                }
                break;
            }
        }
        // (a chunk's byte offset pb * 8 stays below 2^31: lists of < 2^28 points)
        const uint8_t *cbase = ix.codes + (int64_t)readfirstlane64((u64)ix.list_codeoff[l]);

        // (1) residuals r_s = q_s - c (coarsequantizers.jl:40-45), D NQ elements -- NQ / 4 per thread at DS = 16, fewer or none below:
        // res[ii][t][s], DS + 1 rows of NQ per sub-quantizer (W8_RES_STRIDE)
        if constexpr (NQ == 8) {
            const u32 tb = (u32)tid & 511u;
#pragma unroll
            for (u32 e = tb; e < 8u * D; e += 512u) {
                const u32 i = e >> 3, s = e & 7u;
                res[(i / DS) * RS + (i % DS) * 8u + s] = a.queries[(size_t)sqi[s] * D + i] - ix.centroids[(size_t)l * D + i];
            }
        } else {
            // (element tb = 4 i + s stands 4 (i / DS) floats on: the padding rows of the sub-quantizers below its own)
            const int tb = tid & 511, i = tb >> 2, s = tb & 3;
            if (DS == 16 || tb < 4 * D) res[tb + (i / DS) * 4] = a.queries[(size_t)sqi[s] * D + i] - ix.centroids[(size_t)l * D + i];
        }
        // (the thread number passes through an opaque move inside the item loop: the lane-constant addresses it feeds -- codewords, table
        // rows, LDS slots -- would otherwise be hoisted to kernel entry and live, spilled, across the whole persistent loop)
        int tidb = tid & 511;
        asm volatile("" : "+v"(tidb));
        // A thread builds FOUR codewords' entries of ONE sub-quantizer: ii = lane mod 4 (+ 4 for odd waves), codewords cg, cg + 64, + 128,
        // + 192.  A residual row read from LDS serves the four codewords (16 reads of 16 B per thread; one codeword in each of four
        // sub-quantizers per thread was 64 -- on the LDS queue the other workgroup's gathers fill), the four lanes of a quad read four
        // different bank groups (the padding), and the quantised rows below leave conflict-free as they are: the 16 lanes of a store's
        // service group hold 4 sub-quantizers x 4 copies.
        const int ii = (tidb & 3) | (((tidb >> 6) & 1) << 2);
        const int cg = ((tidb >> 2) & 15) | ((tidb >> 7) << 4);
        const float4 *ct = (const float4 *)ix.codebooks_t;        // [ii][g][c][4], G = DS / 4 groups, ksub = 256
        // The four codewords come four dimensions at a time (g = 0 .. G - 1), two register sets that take turns inside a REAL loop of
        // G / 2 trips, two groups each: fully unrolled, the scheduler hoists every request of the build above the arithmetic -- 64 registers
        // of codewords next to 64 of residual rows -- and spills them as they arrive, a wait for memory each.  An odd count (DS = 4: one
        // group, DS = 12: three) leaves its last group behind the loop: it stands in cwa by then -- requested up front (G = 1) or by the
        // trip's second request (G = 3) -- and takes four rows of its own.  Dimensions ascend through trips and tail: the reference's order.
        float4 cwa[4], cwb[4];
        const u32 cofs = (u32)ii * (u32)(G * 256) + (u32)cg;
        auto ldcw = [&](float4 (&d)[4], int g) __attribute__((always_inline)) {
#pragma unroll
            for (int j = 0; j < 4; ++j) d[j] = ct[cofs + (u32)(g * 256 + 64 * j)];
        };
        ldcw(cwa, 0);       // on its way while the residuals settle
        __syncthreads();
        // (2) the f32 entries (index.jl:232-236: df = cb - r, sum += df * df for t ascending; no contraction; two queries per packed
        // instruction: the same IEEE operations element by element), to device memory by label; per-query maxima
        v4f ent[4][NQ / 4];      // [codeword][queries 4 qh .. 4 qh + 3]
        if constexpr (NQ == 8) {
            float mx[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
            const u32 roff = L::RES + (u32)ii * (RS * 4u);
            // four queries at a time (the four-query build on each half of the residual rows; the codewords are requested again)
            static_for<2>([&](auto qc) {
                constexpr int qh = decltype(qc)::value;
                if (qh == 1) ldcw(cwa, 0);
                v2f sum[4][2];
#pragma unroll
                for (int j = 0; j < 4; ++j) sum[j][0] = sum[j][1] = (v2f){0.0f, 0.0f};
                // (the rows of a trip -- eight dimensions -- are requested together at its top)
                v4f rv[8];
                auto grp = [&](const float4 (&cq)[4], int g2) __attribute__((always_inline)) {
#pragma unroll
                    for (int t = 0; t < 4; ++t) {
                        const v2f r01 = (v2f){rv[4 * g2 + t].x, rv[4 * g2 + t].y}, r23 = (v2f){rv[4 * g2 + t].z, rv[4 * g2 + t].w};
#pragma unroll
                        for (int j = 0; j < 4; ++j) {
                            const float cv = t == 0 ? cq[j].x : (t == 1 ? cq[j].y : (t == 2 ? cq[j].z : cq[j].w));
                            const v2f c2 = (v2f){cv, cv};
                            const v2f d0 = c2 - r01, d1 = c2 - r23;
                            sum[j][0] = sum[j][0] + d0 * d0;
                            sum[j][1] = sum[j][1] + d1 * d1;
                        }
                    }
                };
#pragma unroll 1
                for (int h = 0; h < G / 2; ++h) {
#pragma unroll
                    for (int t = 0; t < 8; ++t) rv[t] = w8_lds<v4f>(roff + (u32)(8 * h + t) * 32u + 16u * qh);
                    ldcw(cwb, 2 * h + 1);
                    grp(cwa, 0);
                    if constexpr (G > 2) ldcw(cwa, h == 0 ? 2 : G - 1);      // (the last trip of an even count repeats a request: no branch around one, no second value to merge)
                    grp(cwb, 1);
                }
                if constexpr (G & 1) {
#pragma unroll
                    for (int t = 0; t < 4; ++t) rv[t] = w8_lds<v4f>(roff + (u32)(4 * (G - 1) + t) * 32u + 16u * qh);
                    grp(cwa, 0);
                }
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    ent[j][qh] = (v4f){sum[j][0].x, sum[j][0].y, sum[j][1].x, sum[j][1].y};
                    const int c = cg + 64 * j;
                    const int label = ix.identity_labels ? c : (int)ix.labels[ii * 256 + c];
                    *(v4f *)(gt + ((size_t)(ii * 256 + label) << 3) + 4 * qh) = ent[j][qh];
                    mx[4 * qh + 0] = fmaxf(mx[4 * qh + 0], ent[j][qh].x);
                    mx[4 * qh + 1] = fmaxf(mx[4 * qh + 1], ent[j][qh].y);
                    mx[4 * qh + 2] = fmaxf(mx[4 * qh + 2], ent[j][qh].z);
                    mx[4 * qh + 3] = fmaxf(mx[4 * qh + 3], ent[j][qh].w);
                }
            });
            // (entries are >= +0: the bit pattern orders like the value; the wave's maximum on the DPP network and the scalar unit)
#pragma unroll
            for (int s = 0; s < 8; ++s) {
                const u32 wm = w8_row_max_u32(__float_as_uint(mx[s]));
                if (lane == 0) atomicMax(&smax[s], wm);
            }
        } else {
            v2f sum[4][2];
#pragma unroll
            for (int j = 0; j < 4; ++j) sum[j][0] = sum[j][1] = (v2f){0.0f, 0.0f};
            const u32 roff = L::RES + (u32)ii * (RS * 4u);
            // (the rows of a trip -- eight dimensions -- are requested together at its top: a request waits ~1 000 cycles in the LDS queue behind
            // the other workgroup's gathers, and the build pays that wait once per batch)
            v4f rv[8];
            auto grp = [&](const float4 (&cq)[4], int g2) __attribute__((always_inline)) {
#pragma unroll
                for (int t = 0; t < 4; ++t) {
                    const v2f r01 = (v2f){rv[4 * g2 + t].x, rv[4 * g2 + t].y}, r23 = (v2f){rv[4 * g2 + t].z, rv[4 * g2 + t].w};
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        const float cv = t == 0 ? cq[j].x : (t == 1 ? cq[j].y : (t == 2 ? cq[j].z : cq[j].w));
                        const v2f c2 = (v2f){cv, cv};
                        const v2f d0 = c2 - r01, d1 = c2 - r23;
                        sum[j][0] = sum[j][0] + d0 * d0;
                        sum[j][1] = sum[j][1] + d1 * d1;
                    }
                }
            };
#pragma unroll 1
            for (int h = 0; h < G / 2; ++h) {
#pragma unroll
                for (int t = 0; t < 8; ++t) rv[t] = w8_lds<v4f>(roff + (u32)(8 * h + t) * 16u);
                ldcw(cwb, 2 * h + 1);
                grp(cwa, 0);
                if constexpr (G > 2) ldcw(cwa, h == 0 ? 2 : G - 1);      // (the last trip of an even count repeats a request: no branch around one, no second value to merge)
                grp(cwb, 1);
            }
            if constexpr (G & 1) {
#pragma unroll
                for (int t = 0; t < 4; ++t) rv[t] = w8_lds<v4f>(roff + (u32)(4 * (G - 1) + t) * 16u);
                grp(cwa, 0);
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) ent[j][0] = (v4f){sum[j][0].x, sum[j][0].y, sum[j][1].x, sum[j][1].y};
            float mx[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int c = cg + 64 * j;
                const int label = ix.identity_labels ? c : (int)ix.labels[ii * 256 + c];
                *(v4f *)(gt + ((size_t)(ii * 256 + label) << 2)) = ent[j][0];
                mx[0] = fmaxf(mx[0], ent[j][0].x);
                mx[1] = fmaxf(mx[1], ent[j][0].y);
                mx[2] = fmaxf(mx[2], ent[j][0].z);
                mx[3] = fmaxf(mx[3], ent[j][0].w);
            }
            // (entries are >= +0: the bit pattern orders like the value.  The wave's maximum on the DPP network and the scalar unit: a shuffle
            // is a trip through the LDS queue -- ~1 000 cycles behind the other workgroup's gathers, six of them in a row per query)
#pragma unroll
            for (int s = 0; s < 4; ++s) {
                const u32 wm = w8_row_max_u32(__float_as_uint(mx[s]));
                if (lane == 0) atomicMax(&smax[s], wm);
            }
        }
        __syncthreads();
        // (3) quantise (quantize_tables_m8's rule: q = min(4095, floor(t * inv)), inv = 4095 / largest entry of the query) and write the
        // copies of sub-quantizer ii's entry (consecutive labels are 256 B apart: the same banks)
        {
            float inv[NQ];
#pragma unroll
            for (int s = 0; s < NQ; ++s) {
                const float mxs = __uint_as_float(smax[s]);
                inv[s] = mxs > 0.0f ? 4095.0f / mxs : 0.0f;
            }
            if (tid < NQ) sinv[tid] = inv[tid];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                float ev[NQ];
#pragma unroll
                for (int qh = 0; qh < NQ / 4; ++qh) {
                    ev[4 * qh + 0] = ent[j][qh].x;
                    ev[4 * qh + 1] = ent[j][qh].y;
                    ev[4 * qh + 2] = ent[j][qh].z;
                    ev[4 * qh + 3] = ent[j][qh].w;
                }
                u32 f[NQ];
#pragma unroll
                for (int s = 0; s < NQ; ++s) {
                    const u32 v = (u32)floorf(ev[s] * inv[s]);
                    f[s] = v < 4095u ? v : 4095u;
                }
                if constexpr (NQ == 8) {
                    // two copies, copy (cp + lane / 4) mod 2: the 8 lanes of a 16-byte store's service group write 8 different four-bank groups
                    const uint4 qv = make_uint4(f[0] | (f[1] << 16), f[2] | (f[3] << 16), f[4] | (f[5] << 16), f[6] | (f[7] << 16));
                    const int c = cg + 64 * j;
                    const int lb = ix.identity_labels ? c : (int)ix.labels[ii * 256 + c];
                    const u32 row = ((u32)lb << 8) | ((u32)ii << 4);
#pragma unroll
                    for (int cp = 0; cp < 2; ++cp) *(uint4 *)(smem + (row | ((u32)((cp + (lane >> 2)) & 1) << 7))) = qv;
                } else {
                    // four copies, copy (cp + lane / 4) mod 4: the 16 lanes of a store's service group write 16 different bank pairs
                    const uint2 qv = make_uint2(f[0] | (f[1] << 16), f[2] | (f[3] << 16));
                    const int c = cg + 64 * j;
                    const int lb = ix.identity_labels ? c : (int)ix.labels[ii * 256 + c];
                    const u32 row = ((u32)lb << 8) | ((u32)ii << 3);
#pragma unroll
                    for (int cp = 0; cp < 4; ++cp) *(uint2 *)(smem + (row | ((u32)((cp + (lane >> 2)) & 3) << 6))) = qv;
                }
            }
        }
        // the wave's first two steps of code bytes: requested here, behind the build (held across it they were spilled: a store that waits
        // for the load it saves)
        // (a list's last step reads up to 127 points past p1 -- other lists' bytes or the slack behind the last list, never used: as scan_kernel)
        const __amdgpu_buffer_rsrc_t codes = __builtin_amdgcn_make_buffer_rsrc((void *)cbase, 0, (int)0x7FFFFFF0, 0x00020000);
        v4u ca = (v4u){0u, 0u, 0u, 0u}, cb = ca;
        {
            const u32 pb0 = p0 + (u32)wv * 256u;
            if (pb0 < p1) {
                ca = __builtin_amdgcn_raw_buffer_load_b128(codes, lane * 16, (int)(pb0 * 8u), 0);
                cb = __builtin_amdgcn_raw_buffer_load_b128(codes, lane * 16, (int)((pb0 + 128u < p1 ? pb0 + 128u : pb0) * 8u), 0);
            }
        }
        __syncthreads();   // tables complete (LDS copies; the f32 stores have left for L2: the barrier's release covers them)

        __builtin_amdgcn_s_setprio(W8_PRIO_SCAN);
        w8_scan_range<NQ, KP>(codes, p0, p1, nvalid, K, wv, lane, ca, cb, gtr);
        __builtin_amdgcn_s_setprio(W8_PRIO_REST);

        // ---- every wave has offered what it had: wave s < nvalid hands slot s of the pool over as it is -- the entries fill from index 0
        // (an offer takes the first empty one), the merge kernel behind pushes them through a selector in any order
        __syncthreads();
        if constexpr (KP == 2) {
        // (the wide pool: both halves of slot s, entries 0 .. fc - 1 -- a prefix, as above -- in the pool's order)
        if (wv < nvalid) {
            const int s = wv;
            const u64 v = lane < K ? pool[128 * s + lane] : 0ull;
            const u64 vh = lane + 64 < K ? pool[128 * s + 64 + lane] : 0ull;
            const int fc = __popcll(__builtin_amdgcn_ballot_w64(lane < K && v != KEY_MAX)) + __popcll(__builtin_amdgcn_ballot_w64(lane + 64 < K && vh != KEY_MAX));
            const size_t slot = (size_t)spi[s] * a.maxch + chunk;
            if (lane < fc) a.part_keys[slot * K + lane] = v;
            if (lane + 64 < fc) a.part_keys[slot * K + 64 + lane] = vh;
            if (fc == K) {   // uniform
                const u64 kth = w8_wave_max_u64(v > vh ? v : vh);
                if (lane == 0) atomicMin(&a.qthr[sqi[s]], kth);
            }
            if (lane == 0) a.part_cnt[slot] = (u32)fc;
        }
        } else {
        if (wv < nvalid) {
            const int s = wv;
            const u64 v = lane < K ? pool[64 * s + lane] : 0ull;
            const int fc = __popcll(__builtin_amdgcn_ballot_w64(lane < K && v != KEY_MAX));
            const size_t slot = (size_t)spi[s] * a.maxch + chunk;
            if (lane < fc) a.part_keys[slot * K + lane] = v;
            if (fc == K) {   // uniform
                const u64 kth = w8_wave_max_u64(v);
                if (lane == 0) atomicMin(&a.qthr[sqi[s]], kth);
            }
            if (lane == 0) a.part_cnt[slot] = (u32)fc;
        }
        }
        } while (false);
        __syncthreads();            // every wave is done with this item's state in LDS
        if (tid == 0) swi[0] = qtried < nranges ? resolve(pulled) : 0xFFFFFFFFu;
        __syncthreads();
        wi = __builtin_amdgcn_readfirstlane(swi[0]);
    }
}

template <int NQ, int DS, int KP = 1, int M = 8>
static __device__ __forceinline__ void w8m_scan_items(const ScanArgs &a, float *__restrict__ gtabs, const u32 *__restrict__ item_list,
                                                     u32 *__restrict__ xq, int nranges)
{
    using L = W8Lds<NQ, KP, M>;
    static_assert(w8_ds_ok(DS), "sub-spaces of 4, 8, 12 or 16 dimensions");
    static_assert(M == 8 || (M == 16 && (DS == 4 || DS == 8)), "m = 16: d = 64 and d = 128");
    static_assert(M != 8 || 8u * W8_RES_STRIDE<NQ, DS> * 4u <= L::SMAX - L::RES, "the residuals fit the block sized for DS = 16");
    static_assert(M != 16 || 16u * W8_RES_STRIDE<NQ, DS> * 4u <= L::COLD - L::PARK, "m = 16: the residuals fit the rings' block (W8Lds::RESB)");
    static_assert((u32)M * 256u / 4u == (u32)(M / 8) * (u32)W8_THREADS, "the build: four codewords of one sub-quantizer per thread and trip");
    static_assert(NQ == 8 || 4 * (DS * M) <= W8_THREADS, "NQ = 4: the residual fill is one element per thread");
    constexpr int D = M * DS;
    constexpr u32 RS = W8_RES_STRIDE<NQ, DS>;
    constexpr int G = DS / 4;               // 16-byte groups of a codeword
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const IndexView &ix = a.ix;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);     // (a scalar: branches on the wave's number and its position in the list are scalar branches)
    const int K = a.K;
    float *res = (float *)(smem + L::RESB);
    u32 *smax = (u32 *)(smem + L::SMAX);
    float *sinv = (float *)(smem + L::SMAX) + NQ;
    float *sdc = (float *)(smem + L::QC);
    u32 *ssb = (u32 *)(smem + L::QC) + NQ;
    u32 *spi = (u32 *)(smem + L::QC) + 2 * NQ;
    u32 *sqi = (u32 *)(smem + L::QC) + 3 * NQ;
    u64 *shard = (u64 *)(smem + L::HARD);
    u64 *sthr = (u64 *)(smem + L::STHR);
    u32 *swi = (u32 *)(smem + L::SWI);
    const u32 total = a.wi_off[ix.kc];
    float *gt = gtabs + (size_t)blockIdx.x * W8_GTAB_FLOATS<NQ, M>;
    const __amdgpu_buffer_rsrc_t gtr = __builtin_amdgcn_make_buffer_rsrc((void *)gt, 0, (int)(W8_GTAB_FLOATS<NQ, M> * 4u), 0x00020000);

    u64 *pool = (u64 *)(smem + L::POOL);
    // (thread 0's: the part it pulls from, the parts found empty so far)
    int qcur = nranges > 1 ? (int)(__builtin_amdgcn_s_getreg(20 | (3 << 11)) & 7u) : 0, qtried = 0;
    // the item behind ticket k of the current part; a part that is exhausted hands over to the next one (a trip per part: the tail only)
    auto resolve = [&](u32 k) -> u32 {
        for (;;) {
            // (nranges is 8 or 1: no division -- this runs between two barriers of every work item)
            const u32 r0 = nranges == 1 ? 0u : (u32)(((u64)total * (u32)qcur) >> 3), r1 = nranges == 1 ? total : (u32)(((u64)total * (u32)(qcur + 1)) >> 3);
            if (k < r1 - r0) return r0 + k;
            qcur = qcur + 1 == nranges ? 0 : qcur + 1;
            if (++qtried >= nranges) return 0xFFFFFFFFu;
            k = atomicAdd(xq + qcur * 16, 1u);
        }
    };
    if (tid == 0) swi[0] = resolve(atomicAdd(xq + qcur * 16, 1u));
    __syncthreads();
    u32 wi = __builtin_amdgcn_readfirstlane(swi[0]);
    for (;;) {
        if (wi >= total) break;   // uniform: every wave of every workgroup reaches this
        // the NEXT work item's ticket is pulled now and looked at when this one is done: the atomic's trip is off the critical path
        u32 pulled = 0;
        if (tid == 0 && qtried < nranges) pulled = atomicAdd(xq + qcur * 16, 1u);
        do {   // (one trip: `break` = this work item is finished)
        const int l = __builtin_amdgcn_readfirstlane((int)item_list[wi]);
        const u32 cnt = __builtin_amdgcn_readfirstlane(a.list_cnt[l]);
        const u32 ng = (cnt + (u32)(NQ - 1)) / (u32)NQ;
        const u32 local = wi - __builtin_amdgcn_readfirstlane(a.wi_off[l]);
        const u32 chunk = local / ng, grp = local - chunk * ng;
        const u32 len = __builtin_amdgcn_readfirstlane(ix.list_len[l]);
        const u32 p0 = chunk * a.CH;
        if (p0 >= len) break;   // uniform
        const u32 p1 = min(len, p0 + a.CH);
        const int nvalid = min(NQ, (int)(cnt - grp * (u32)NQ));

        // the queries of the group: thread s < NQ fetches slot s (slots past nvalid repeat slot 0 and can never be candidates)
        if (tid < NQ) {
            const int ss = tid < nvalid ? tid : 0;
            const u32 pi = a.bucket_items[a.bucket_off[l] + grp * (u32)NQ + ss];
            const u32 qq = pi / (u32)a.w;
            spi[tid] = pi;
            sqi[tid] = qq;
            ssb[tid] = a.probe_base[pi];
            sdc[tid] = a.probe_dc[pi];
            const u64 t0 = __hip_atomic_load(&a.qthr[qq], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            shard[tid] = t0;
            sthr[tid] = t0;
            smax[tid] = 0u;
        }
        // (the pool's 64 NQ entries: the workgroup's last threads, which fetch no slot)
        if constexpr (KP == 1) {
        if (tid >= W8_THREADS - 64 * NQ && tid < W8_THREADS) pool[tid - (W8_THREADS - 64 * NQ)] = KEY_MAX;
        } else {
            // (the wide pool's 128 NQ entries: one or two per thread)
#pragma unroll
            for (int i = 0; i < 128 * NQ / W8_THREADS; ++i) pool[tid + i * W8_THREADS] = KEY_MAX;
        }
        __syncthreads();
        // exact pruning of whole work items, as in scan_kernel: no sum of this list lies below its coarse distance
        if (a.prune) {
            bool all = true;
#pragma unroll
            for (int s = 0; s < NQ; ++s)
                all = all && (s >= nvalid || __builtin_amdgcn_readfirstlane(__float_as_uint(sdc[s])) > (u32)(readfirstlane64(shard[s]) >> 32));
            if (all) {   // uniform
                if (tid < nvalid) {
                    const u32 pi = spi[tid];
                    a.part_cnt[(size_t)pi * a.maxch + chunk] = 0u;
                    atomicAdd(a.scanned_points + (size_t)(pi & 63u) * 8 + 1, (u64)(p1 - p0));
                }
                break;
            }
        }
        // (a chunk's byte offset pb * 8 stays below 2^31: lists of < 2^28 points; m = 16: pb * 16, lists of < 2^27 points)
        const uint8_t *cbase = ix.codes + (int64_t)readfirstlane64((u64)ix.list_codeoff[l]);

        // (1) residuals r_s = q_s - c (coarsequantizers.jl:40-45), D NQ elements -- NQ / 4 per thread at DS = 16, fewer or none below:
        // res[ii][t][s], DS + 1 rows of NQ per sub-quantizer (W8_RES_STRIDE)
        if constexpr (NQ == 8) {
            const u32 tb = (u32)tid & 511u;
#pragma unroll
            for (u32 e = tb; e < 8u * D; e += 512u) {
                const u32 i = e >> 3, s = e & 7u;
                res[(i / DS) * RS + (i % DS) * 8u + s] = a.queries[(size_t)sqi[s] * D + i] - ix.centroids[(size_t)l * D + i];
            }
        } else {
            // (element tb = 4 i + s stands 4 (i / DS) floats on: the padding rows of the sub-quantizers below its own)
            const int tb = tid & 511, i = tb >> 2, s = tb & 3;
            if (DS == 16 || tb < 4 * D) res[tb + (i / DS) * 4] = a.queries[(size_t)sqi[s] * D + i] - ix.centroids[(size_t)l * D + i];
        }
        // (the thread number passes through an opaque move inside the item loop: the lane-constant addresses it feeds -- codewords, table
        // rows, LDS slots -- would otherwise be hoisted to kernel entry and live, spilled, across the whole persistent loop)
        int tidb = tid & 511;
        asm volatile("" : "+v"(tidb));
        // A thread builds FOUR codewords' entries of ONE sub-quantizer: ii = lane mod 4 (+ 4 for odd waves), codewords cg, cg + 64, + 128,
        // + 192.  A residual row read from LDS serves the four codewords (16 reads of 16 B per thread; one codeword in each of four
        // sub-quantizers per thread was 64 -- on the LDS queue the other workgroup's gathers fill), the four lanes of a quad read four
        // different bank groups (the padding), and the quantised rows below leave conflict-free as they are: the 16 lanes of a store's
        // service group hold 4 sub-quantizers x 4 copies.
        // (m = 16: two trips of the build, sub-quantizers ii and ii + 8; the entries go to device memory by label trip by trip and are
        // quantised from there, step (3))
        int ii = (tidb & 3) | (((tidb >> 6) & 1) << 2);
        const int cg = ((tidb >> 2) & 15) | ((tidb >> 7) << 4);
        const float4 *ct = (const float4 *)ix.codebooks_t;        // [ii][g][c][4], G = DS / 4 groups, ksub = 256
        // The four codewords come four dimensions at a time (g = 0 .. G - 1), two register sets that take turns inside a REAL loop of
        // G / 2 trips, two groups each: fully unrolled, the scheduler hoists every request of the build above the arithmetic -- 64 registers
        // of codewords next to 64 of residual rows -- and spills them as they arrive, a wait for memory each.  An odd count (DS = 4: one
        // group, DS = 12: three) leaves its last group behind the loop: it stands in cwa by then -- requested up front (G = 1) or by the
        // trip's second request (G = 3) -- and takes four rows of its own.  Dimensions ascend through trips and tail: the reference's order.
        float4 cwa[4], cwb[4];
        u32 cofs = (u32)ii * (u32)(G * 256) + (u32)cg;
        auto ldcw = [&](float4 (&d)[4], int g) __attribute__((always_inline)) {
#pragma unroll
            for (int j = 0; j < 4; ++j) d[j] = ct[cofs + (u32)(g * 256 + 64 * j)];
        };
        ldcw(cwa, 0);       // on its way while the residuals settle
        __syncthreads();
        // (2) the f32 entries (index.jl:232-236: df = cb - r, sum += df * df for t ascending; no contraction; two queries per packed
        // instruction: the same IEEE operations element by element), to device memory by label; per-query maxima
        v4f ent[4][NQ / 4];      // [codeword][queries 4 qh .. 4 qh + 3]
#pragma unroll 1
        for (int tr = 0; tr < M / 8; ++tr) {
        if (M == 16 && tr > 0) {
            ii += 8;
            cofs += 8u * (u32)(G * 256);
            ldcw(cwa, 0);
        }
        if constexpr (NQ == 8) {
            float mx[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
            const u32 roff = L::RESB + (u32)ii * (RS * 4u);
            // four queries at a time (the four-query build on each half of the residual rows; the codewords are requested again)
            static_for<2>([&](auto qc) {
                constexpr int qh = decltype(qc)::value;
                if (qh == 1) ldcw(cwa, 0);
                v2f sum[4][2];
#pragma unroll
                for (int j = 0; j < 4; ++j) sum[j][0] = sum[j][1] = (v2f){0.0f, 0.0f};
                // (the rows of a trip -- eight dimensions -- are requested together at its top)
                v4f rv[8];
                auto grp = [&](const float4 (&cq)[4], int g2) __attribute__((always_inline)) {
#pragma unroll
                    for (int t = 0; t < 4; ++t) {
                        const v2f r01 = (v2f){rv[4 * g2 + t].x, rv[4 * g2 + t].y}, r23 = (v2f){rv[4 * g2 + t].z, rv[4 * g2 + t].w};
#pragma unroll
                        for (int j = 0; j < 4; ++j) {
                            const float cv = t == 0 ? cq[j].x : (t == 1 ? cq[j].y : (t == 2 ? cq[j].z : cq[j].w));
                            const v2f c2 = (v2f){cv, cv};
                            const v2f d0 = c2 - r01, d1 = c2 - r23;
                            sum[j][0] = sum[j][0] + d0 * d0;
                            sum[j][1] = sum[j][1] + d1 * d1;
                        }
                    }
                };
#pragma unroll 1
                for (int h = 0; h < G / 2; ++h) {
#pragma unroll
                    for (int t = 0; t < 8; ++t) rv[t] = w8_lds<v4f>(roff + (u32)(8 * h + t) * 32u + 16u * qh);
                    ldcw(cwb, 2 * h + 1);
                    grp(cwa, 0);
                    if constexpr (G > 2) ldcw(cwa, h == 0 ? 2 : G - 1);      // (the last trip of an even count repeats a request: no branch around one, no second value to merge)
                    grp(cwb, 1);
                }
                if constexpr (G & 1) {
#pragma unroll
                    for (int t = 0; t < 4; ++t) rv[t] = w8_lds<v4f>(roff + (u32)(4 * (G - 1) + t) * 32u + 16u * qh);
                    grp(cwa, 0);
                }
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    ent[j][qh] = (v4f){sum[j][0].x, sum[j][0].y, sum[j][1].x, sum[j][1].y};
                    const int c = cg + 64 * j;
                    const int label = ix.identity_labels ? c : (int)ix.labels[ii * 256 + c];
                    *(v4f *)(gt + ((size_t)(ii * 256 + label) << 3) + 4 * qh) = ent[j][qh];
                    mx[4 * qh + 0] = fmaxf(mx[4 * qh + 0], ent[j][qh].x);
                    mx[4 * qh + 1] = fmaxf(mx[4 * qh + 1], ent[j][qh].y);
                    mx[4 * qh + 2] = fmaxf(mx[4 * qh + 2], ent[j][qh].z);
                    mx[4 * qh + 3] = fmaxf(mx[4 * qh + 3], ent[j][qh].w);
                }
            });
            // (entries are >= +0: the bit pattern orders like the value; the wave's maximum on the DPP network and the scalar unit)
#pragma unroll
            for (int s = 0; s < 8; ++s) {
                const u32 wm = w8_row_max_u32(__float_as_uint(mx[s]));
                if (lane == 0) atomicMax(&smax[s], wm);
            }
        } else {
            v2f sum[4][2];
#pragma unroll
            for (int j = 0; j < 4; ++j) sum[j][0] = sum[j][1] = (v2f){0.0f, 0.0f};
            const u32 roff = L::RESB + (u32)ii * (RS * 4u);
            // (the rows of a trip -- eight dimensions -- are requested together at its top: a request waits ~1 000 cycles in the LDS queue behind
            // the other workgroup's gathers, and the build pays that wait once per batch)
            v4f rv[8];
            auto grp = [&](const float4 (&cq)[4], int g2) __attribute__((always_inline)) {
#pragma unroll
                for (int t = 0; t < 4; ++t) {
                    const v2f r01 = (v2f){rv[4 * g2 + t].x, rv[4 * g2 + t].y}, r23 = (v2f){rv[4 * g2 + t].z, rv[4 * g2 + t].w};
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        const float cv = t == 0 ? cq[j].x : (t == 1 ? cq[j].y : (t == 2 ? cq[j].z : cq[j].w));
                        const v2f c2 = (v2f){cv, cv};
                        const v2f d0 = c2 - r01, d1 = c2 - r23;
                        sum[j][0] = sum[j][0] + d0 * d0;
                        sum[j][1] = sum[j][1] + d1 * d1;
                    }
                }
            };
#pragma unroll 1
            for (int h = 0; h < G / 2; ++h) {
#pragma unroll
                for (int t = 0; t < 8; ++t) rv[t] = w8_lds<v4f>(roff + (u32)(8 * h + t) * 16u);
                ldcw(cwb, 2 * h + 1);
                grp(cwa, 0);
                if constexpr (G > 2) ldcw(cwa, h == 0 ? 2 : G - 1);      // (the last trip of an even count repeats a request: no branch around one, no second value to merge)
                grp(cwb, 1);
            }
            if constexpr (G & 1) {
#pragma unroll
                for (int t = 0; t < 4; ++t) rv[t] = w8_lds<v4f>(roff + (u32)(4 * (G - 1) + t) * 16u);
                grp(cwa, 0);
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) ent[j][0] = (v4f){sum[j][0].x, sum[j][0].y, sum[j][1].x, sum[j][1].y};
            float mx[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int c = cg + 64 * j;
                const int label = ix.identity_labels ? c : (int)ix.labels[ii * 256 + c];
                *(v4f *)(gt + ((size_t)(ii * 256 + label) << 2)) = ent[j][0];
                mx[0] = fmaxf(mx[0], ent[j][0].x);
                mx[1] = fmaxf(mx[1], ent[j][0].y);
                mx[2] = fmaxf(mx[2], ent[j][0].z);
                mx[3] = fmaxf(mx[3], ent[j][0].w);
            }
            // (entries are >= +0: the bit pattern orders like the value.  The wave's maximum on the DPP network and the scalar unit: a shuffle
            // is a trip through the LDS queue -- ~1 000 cycles behind the other workgroup's gathers, six of them in a row per query)
#pragma unroll
            for (int s = 0; s < 4; ++s) {
                const u32 wm = w8_row_max_u32(__float_as_uint(mx[s]));
                if (lane == 0) atomicMax(&smax[s], wm);
            }
        }
        }
        __syncthreads();
        // (3) quantise (quantize_tables_m8's rule: q = min(4095, floor(t * inv)), inv = 4095 / largest entry of the query) and write the
        // copies of sub-quantizer ii's entry (consecutive labels are 256 B apart: the same banks)
        {
            float inv[NQ];
#pragma unroll
            for (int s = 0; s < NQ; ++s) {
                const float mxs = __uint_as_float(smax[s]);
                inv[s] = mxs > 0.0f ? (float)W8_QCAP<M> / mxs : 0.0f;
            }
            if (tid < NQ) sinv[tid] = inv[tid];
            if constexpr (M == 16) {
                // THE FILTER AT SIXTEEN TERMS.  q = min(2047, floor(t * inv)), inv = 2047 / largest entry: 16 x 2047 = 32 752 <= 0x7FFF, and
                // 0x8000 + 32 752 < 2^16 -- a biased field (w8_bias: B <= 0x8000) never carries.  w8_bias is used AS IT IS, and its constants
                // hold at sixteen terms for this reason: with S the reference's float sum (dc, then sixteen entries, all >= +0, so
                // S >= (dc + sum t)(1 - u)^16, u = 2^-24), S <= thr implies sum t <= thr (1 + 17 u) - dc, and
                //   sum q <= sum fl(t inv) <= inv (1 + u)(thr (1 + 17 u) - dc).
                // w8_bias computes x = ((thr (1 + 2^-18) - dc) inv)(1 + 2^-18) in floats.  fl(thr (1 + 64 u)) >= thr (1 + 62 u): 45 u thr above
                // what the argument needs, which covers the subtraction's rounding (<= 1 u of a result <= thr (1 + 64 u)); the second
                // factor's 64 u covers the (1 + u) above and the three roundings behind the subtraction.  So sum q <= floor(x): the `+ 2` is
                // margin here as at eight terms (where the same argument needs 1 + 9 u).  x >= 32 000 saturates to "every point passes"
                // (32 752 <= 0x7FFF); x < 0 means thr (1 + 62 u) < dc: no candidate exists; a scale of 0, inf or NaN (all-zero or denormal
                // tables) makes x 0, +-inf or NaN: every point passes, or thr < dc.  The cold-start bounds read S < (dc + (Q + 16) / inv)
                // (1 + 19 u) -- t inv (1 - u) < q + 1 per term, sixteen roundings of S -- against the (1 + 168 u)(1 + 335 u) of the code.
                // tests/test_wg8_m16_filter.py restates all of this in numpy and shows that the cap 4095 of m = 8 overflows at sixteen terms.
                // The entries come back from device memory (written by
                // this workgroup in front of the barrier above, read from L2 as the passes read them), by LABEL: thread -> sub-quantizer
                // tid mod 16, labels tid / 16 + 32 k, four at a time.  The 16 lanes of a row write the 16 sub-quantizers of one label -- NQ = 8:
                // 16 x 16 B, the 64 banks once; NQ = 4: 16 x 8 B, and the next row the other copy (copy (cp + lane / 16) mod 2): the 32 lanes
                // of a store's service group write 32 different bank pairs.
                const u32 i3 = (u32)tidb & 15u, l0 = (u32)tidb >> 4;
#pragma unroll 1
                for (u32 k = 0; k < 8u; k += 4u) {
                    v4f e[4][NQ / 4];
#pragma unroll
                    for (int jj = 0; jj < 4; ++jj)
#pragma unroll
                        for (int q4 = 0; q4 < NQ / 4; ++q4) e[jj][q4] = w8_gtab_load<NQ>(gtr, i3, l0 + 32u * (k + (u32)jj), q4);
#pragma unroll
                    for (int jj = 0; jj < 4; ++jj) {
                        const u32 lb = l0 + 32u * (k + (u32)jj);
                        u32 f[NQ];
#pragma unroll
                        for (int s = 0; s < NQ; ++s) {
                            const u32 v = (u32)floorf(e[jj][s >> 2][s & 3] * inv[s]);
                            f[s] = v < W8_QCAP<16> ? v : W8_QCAP<16>;
                        }
                        if constexpr (NQ == 8) {
                            *(uint4 *)(smem + ((lb << 8) | (i3 << 4))) = make_uint4(f[0] | (f[1] << 16), f[2] | (f[3] << 16), f[4] | (f[5] << 16), f[6] | (f[7] << 16));
                        } else {
                            const uint2 qv = make_uint2(f[0] | (f[1] << 16), f[2] | (f[3] << 16));
#pragma unroll
                            for (int cp = 0; cp < 2; ++cp) *(uint2 *)(smem + ((lb << 8) | (i3 << 3) | ((u32)((cp + (lane >> 4)) & 1) << 7))) = qv;
                        }
                    }
                }
            } else {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                float ev[NQ];
#pragma unroll
                for (int qh = 0; qh < NQ / 4; ++qh) {
                    ev[4 * qh + 0] = ent[j][qh].x;
                    ev[4 * qh + 1] = ent[j][qh].y;
                    ev[4 * qh + 2] = ent[j][qh].z;
                    ev[4 * qh + 3] = ent[j][qh].w;
                }
                u32 f[NQ];
#pragma unroll
                for (int s = 0; s < NQ; ++s) {
                    const u32 v = (u32)floorf(ev[s] * inv[s]);
                    f[s] = v < 4095u ? v : 4095u;
                }
                if constexpr (NQ == 8) {
                    // two copies, copy (cp + lane / 4) mod 2: the 8 lanes of a 16-byte store's service group write 8 different four-bank groups
                    const uint4 qv = make_uint4(f[0] | (f[1] << 16), f[2] | (f[3] << 16), f[4] | (f[5] << 16), f[6] | (f[7] << 16));
                    const int c = cg + 64 * j;
                    const int lb = ix.identity_labels ? c : (int)ix.labels[ii * 256 + c];
                    const u32 row = ((u32)lb << 8) | ((u32)ii << 4);
#pragma unroll
                    for (int cp = 0; cp < 2; ++cp) *(uint4 *)(smem + (row | ((u32)((cp + (lane >> 2)) & 1) << 7))) = qv;
                } else {
                    // four copies, copy (cp + lane / 4) mod 4: the 16 lanes of a store's service group write 16 different bank pairs
                    const uint2 qv = make_uint2(f[0] | (f[1] << 16), f[2] | (f[3] << 16));
                    const int c = cg + 64 * j;
                    const int lb = ix.identity_labels ? c : (int)ix.labels[ii * 256 + c];
                    const u32 row = ((u32)lb << 8) | ((u32)ii << 3);
#pragma unroll
                    for (int cp = 0; cp < 4; ++cp) *(uint2 *)(smem + (row | ((u32)((cp + (lane >> 2)) & 3) << 6))) = qv;
                }
            }
            }
        }
        // the wave's first two steps of code bytes: requested here, behind the build (held across it they were spilled: a store that waits
        // for the load it saves)
        // (a list's last step reads up to 127 points past p1 -- other lists' bytes or the slack behind the last list, never used: as scan_kernel)
        const __amdgpu_buffer_rsrc_t codes = __builtin_amdgcn_make_buffer_rsrc((void *)cbase, 0, (int)0x7FFFFFF0, 0x00020000);
        // (m = 16: four sets -- ca, cc, cb, cd hold the step's quarters 0, 1, 2, 3; m = 8 leaves cc and cd alone)
        v4u ca = (v4u){0u, 0u, 0u, 0u}, cb = ca, cc = ca, cd = ca;
        {
            // (m = 16 with eight queries: a step is 128 points, the sets ca and cc -- w8m_scan_range, NPT)
            const u32 pb0 = p0 + (u32)wv * (M == 16 && NQ == 8 ? 128u : 256u);
            if (pb0 < p1) {
                if constexpr (M == 16 && NQ == 8) {
                    ca = __builtin_amdgcn_raw_buffer_load_b128(codes, lane * 16, (int)(pb0 * 16u), 0);
                    cc = __builtin_amdgcn_raw_buffer_load_b128(codes, lane * 16, (int)((pb0 + 64u < p1 ? pb0 + 64u : pb0) * 16u), 0);
                } else if constexpr (M == 16) {
                    ca = __builtin_amdgcn_raw_buffer_load_b128(codes, lane * 16, (int)(pb0 * 16u), 0);
                    cc = __builtin_amdgcn_raw_buffer_load_b128(codes, lane * 16, (int)((pb0 + 64u < p1 ? pb0 + 64u : pb0) * 16u), 0);
                    cb = __builtin_amdgcn_raw_buffer_load_b128(codes, lane * 16, (int)((pb0 + 128u < p1 ? pb0 + 128u : pb0) * 16u), 0);
                    cd = __builtin_amdgcn_raw_buffer_load_b128(codes, lane * 16, (int)((pb0 + 192u < p1 ? pb0 + 192u : pb0) * 16u), 0);
                } else {
                ca = __builtin_amdgcn_raw_buffer_load_b128(codes, lane * 16, (int)(pb0 * 8u), 0);
                cb = __builtin_amdgcn_raw_buffer_load_b128(codes, lane * 16, (int)((pb0 + 128u < p1 ? pb0 + 128u : pb0) * 8u), 0);
                }
            }
        }
        __syncthreads();   // tables complete (LDS copies; the f32 stores have left for L2: the barrier's release covers them)

        __builtin_amdgcn_s_setprio(W8_PRIO_SCAN);
        w8m_scan_range<NQ, KP, M>(codes, p0, p1, nvalid, K, wv, lane, ca, cb, cc, cd, gtr);
        __builtin_amdgcn_s_setprio(W8_PRIO_REST);

        // ---- every wave has offered what it had: wave s < nvalid hands slot s of the pool over as it is -- the entries fill from index 0
        // (an offer takes the first empty one), the merge kernel behind pushes them through a selector in any order
        __syncthreads();
        if constexpr (KP == 2) {
        // (the wide pool: both halves of slot s, entries 0 .. fc - 1 -- a prefix, as above -- in the pool's order)
        if (wv < nvalid) {
            const int s = wv;
            const u64 v = lane < K ? pool[128 * s + lane] : 0ull;
            const u64 vh = lane + 64 < K ? pool[128 * s + 64 + lane] : 0ull;
            const int fc = __popcll(__builtin_amdgcn_ballot_w64(lane < K && v != KEY_MAX)) + __popcll(__builtin_amdgcn_ballot_w64(lane + 64 < K && vh != KEY_MAX));
            const size_t slot = (size_t)spi[s] * a.maxch + chunk;
            if (lane < fc) a.part_keys[slot * K + lane] = v;
            if (lane + 64 < fc) a.part_keys[slot * K + 64 + lane] = vh;
            if (fc == K) {   // uniform
                const u64 kth = w8_wave_max_u64(v > vh ? v : vh);
                if (lane == 0) atomicMin(&a.qthr[sqi[s]], kth);
            }
            if (lane == 0) a.part_cnt[slot] = (u32)fc;
        }
        } else {
        if (wv < nvalid) {
            const int s = wv;
            const u64 v = lane < K ? pool[64 * s + lane] : 0ull;
            const int fc = __popcll(__builtin_amdgcn_ballot_w64(lane < K && v != KEY_MAX));
            const size_t slot = (size_t)spi[s] * a.maxch + chunk;
            if (lane < fc) a.part_keys[slot * K + lane] = v;
            if (fc == K) {   // uniform
                const u64 kth = w8_wave_max_u64(v);
                if (lane == 0) atomicMin(&a.qthr[sqi[s]], kth);
            }
            if (lane == 0) a.part_cnt[slot] = (u32)fc;
        }
        }
        } while (false);
        __syncthreads();            // every wave is done with this item's state in LDS
        if (tid == 0) swi[0] = qtried < nranges ? resolve(pulled) : 0xFFFFFFFFu;
        __syncthreads();
        wi = __builtin_amdgcn_readfirstlane(swi[0]);
    }
}

// The entry points.  wg8_scan_kernel<NQ> is the kernel of DS = 16 (d = 128) under the name it has always had -- what the profiles, the
// counters' kernel filters and the register-budget test look for; wg8_scan_kernel<NQ, DS> are the narrower sub-spaces.
template <int NQ>
__global__ __launch_bounds__(W8_THREADS, W8_NW / 2) void wg8_scan_kernel(const ScanArgs a, float *__restrict__ gtabs, const u32 *__restrict__ item_list,
                                                                 u32 *__restrict__ xq, int nranges)
{
    w8_scan_items<NQ, 16>(a, gtabs, item_list, xq, nranges);
}
template <int NQ, int DS>
__global__ __launch_bounds__(W8_THREADS, W8_NW / 2) void wg8_scan_kernel(const ScanArgs a, float *__restrict__ gtabs, const u32 *__restrict__ item_list,
                                                                 u32 *__restrict__ xq, int nranges)
{
    static_assert(DS != 16, "DS = 16 is wg8_scan_kernel<NQ>");
    w8_scan_items<NQ, DS>(a, gtabs, item_list, xq, nranges);
}
// The wide pool (KP = 2: 64 < K <= 128), every width under one name -- one that does not contain the narrow kernels': what looks those up
// by name finds what it always found.
template <int NQ, int DS>
__global__ __launch_bounds__(W8_THREADS, W8_NW / 2) void wg8_wide_scan_kernel(const ScanArgs a, float *__restrict__ gtabs, const u32 *__restrict__ item_list,
                                                                      u32 *__restrict__ xq, int nranges)
{
    w8_scan_items<NQ, DS, 2>(a, gtabs, item_list, xq, nranges);
}
// Sixteen sub-quantizers (M = 16: d = 16 DS, DS = 8 -- PQ16 at d = 128 -- and 4; K <= 64; on request, table modes 6 / 7), again under a
// name of its own.
template <int NQ, int DS>
__global__ __launch_bounds__(W8_THREADS, W8_NW / 2) void wg8_m16_scan_kernel(const ScanArgs a, float *__restrict__ gtabs, const u32 *__restrict__ item_list,
                                                                     u32 *__restrict__ xq, int nranges)
{
    w8m_scan_items<NQ, DS, 1, 16>(a, gtabs, item_list, xq, nranges);
}
