// ivfadc_hip.hip -- host runtime behind the C ABI of include/ivfadc_hip.h.
//
// Replaces, for the knn_search hot path, the Julia functions
//   knn_search            /root/reference/src/index.jl:204-273
//   coarse_search & co.   /root/reference/src/coarsequantizers.jl:33-48
//   _encode_point/_push!  /root/reference/src/utils.jl:127-161
// There is no CPU fallback: without a HIP device every compute entry point fails.
#include "../../include/ivfadc_hip.h"
#include "kernels.hip.h"
#include "train.hip.h"
#include "generic.hip.h"
#include "u16scan.hip.h"
#include "twolevel.hip.h"
#include "subset.hip.h"
#include "maskset.hip.h"
#include "range.hip.h"
#include "reconstruct.hip.h"
#include "score.hip.h"
#include "pack_operands.h"
#include "plan.h"   // the search planner (pure; on scan_layouts.h, which the kernel headers above share)
#include "search_call.h"   // the batch a function works on, and the one function that slices it (pure)
#include "batch_plan.h"    // the schedule of the host-pointer searches: batches, upload groups, tokens, result blocks, device split (pure)
#include "list_mirror.h"   // the host mirror of the lists, its edits, the label map and the device layout's arithmetic (pure)

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <mutex>
#include <new>
#include <stdexcept>
#include <string>
#include <thread>
#include <vector>

#include <dlfcn.h>
#include <execinfo.h>
#include <fcntl.h>
#include <signal.h>
#include <sys/stat.h>
#include <unistd.h>
#include <rccl/rccl.h>   // types and prototypes only: the library is bound with dlopen (see rccl_api)

#include <rocprim/device/device_segmented_radix_sort.hpp>   // generic path only (after <cstring>: its headers use memset)
#include <rocprim/device/device_radix_sort.hpp>             // ivfadc_locate_device: the wanted ids, sorted on the device

// Diagnostic (off unless IVFADC_ABORT_TRACE=<file> is set when the library is loaded; tests/conftest.py sets it): a process that dies in
// abort() -- the HIP runtime after a queue error, glibc after a heap check, an escaped exception -- under a test runner that captures fd 2
// leaves nothing behind but the signal.  The handler appends the native backtrace of the aborting thread to the file, restores the default
// action and returns into the abort.  Async-signal-safe calls only (open / write / backtrace_symbols_fd).
namespace {
char g_abort_trace_path[512];
struct sigaction g_abort_prev;   // whoever handled SIGABRT before (Python's faulthandler under pytest): called afterwards
void abort_trace_handler(int sig)
{
    const int fd = open(g_abort_trace_path, O_WRONLY | O_CREAT | O_APPEND, 0644);
    if (fd >= 0) {
        static const char head[] = "---- SIGABRT: native backtrace of the aborting thread (libivfadc_hip abort trace) ----\n";
        (void)!write(fd, head, sizeof head - 1);
        void *frames[64];
        const int n = backtrace(frames, 64);
        backtrace_symbols_fd(frames, n, fd);
        close(fd);
    }
    sigaction(sig, &g_abort_prev, nullptr);
    if (g_abort_prev.sa_handler != SIG_DFL && g_abort_prev.sa_handler != SIG_IGN && !(g_abort_prev.sa_flags & SA_SIGINFO))
        g_abort_prev.sa_handler(sig);
}
struct AbortTraceInit {
    AbortTraceInit()
    {
        const char *p = getenv("IVFADC_ABORT_TRACE");
        if (!p || !*p || strlen(p) >= sizeof g_abort_trace_path) return;
        strcpy(g_abort_trace_path, p);
        void *warm[4];
        (void)backtrace(warm, 4);   // loads libgcc's unwinder now, not inside the handler
        struct sigaction sa;
        memset(&sa, 0, sizeof sa);
        sa.sa_handler = abort_trace_handler;
        sigaction(SIGABRT, &sa, &g_abort_prev);
    }
} g_abort_trace_init;
}   // namespace

using namespace ivf;

static thread_local std::string g_err;

static int fail(int code, const char *fmt, ...)
{
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    g_err = buf;
    return code;
}

#define HIP_TRY(expr)                                                                              \
    do {                                                                                           \
        hipError_t e_ = (expr);                                                                    \
        if (e_ != hipSuccess)                                                                      \
            return fail(IVFADC_ERR_HIP, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), __FILE__, __LINE__); \
    } while (0)

// No C++ exception crosses the C ABI: every extern "C" entry point is a function-try-block ending in IVF_CATCH
// (std::vector growth on hostile sizes, std::bad_alloc, ...).
static int on_exception() noexcept
{
    try { throw; }
    catch (const std::bad_alloc &) { return fail(IVFADC_ERR_INVALID, "out of host memory"); }
    catch (const std::exception &e) { return fail(IVFADC_ERR_INVALID, "C++ exception: %s", e.what()); }
    catch (...) { return fail(IVFADC_ERR_INVALID, "unknown C++ exception"); }
}
#define IVF_CATCH catch (...) { return on_exception(); }

#define TRY(expr)                  \
    do {                           \
        int rc_ = (expr);          \
        if (rc_ != IVFADC_OK) return rc_; \
    } while (0)

namespace {

struct DevBuf {
    void *p = nullptr;
    size_t bytes = 0;
    bool owned = true;   // false: an alias of another handle's buffer (ivfadc_clone_view) -- never freed, never grown
    int ensure(size_t need)
    {
        if (need <= bytes) return IVFADC_OK;
        if (!owned) return fail(IVFADC_ERR_STATE, "a view cannot grow a buffer of the index it was taken from");
        if (p) { (void)hipFree(p); p = nullptr; bytes = 0; }
        size_t want = need + need / 4;
        hipError_t e = hipMalloc(&p, want);
        if (e != hipSuccess) {
            e = hipMalloc(&p, need);
            want = need;
        }
        if (e != hipSuccess) { p = nullptr; return fail(IVFADC_ERR_HIP, "hipMalloc(%zu) failed: %s", need, hipGetErrorString(e)); }
        bytes = want;
        return IVFADC_OK;
    }
    // exactly `need` bytes, for a buffer that is written once and never grows (a subset view's lists); the buffer must be empty
    int alloc_exact(size_t need)
    {
        const hipError_t e = hipMalloc(&p, need);
        if (e != hipSuccess) { p = nullptr; return fail(IVFADC_ERR_HIP, "hipMalloc(%zu) failed: %s", need, hipGetErrorString(e)); }
        bytes = need;
        return IVFADC_OK;
    }
    void release()
    {
        if (p && owned) (void)hipFree(p);
        p = nullptr;
        bytes = 0;
        owned = true;
    }
    void alias() { owned = false; }
    template <class T> T *as() const { return (T *)p; }
};

// Page-locked host ranges the library knows to be readable and writable by kernels at their host address: what ivfadc_host_alloc
// handed out and what the caller pinned with ivfadc_host_register.  A host-pointer search whose arrays lie inside one skips the
// staging copy for that array (queries are ingested from it directly, results are written into it by the final kernel).
struct HostRange { uintptr_t lo, hi; bool owned; };
std::mutex g_host_mu;
std::vector<HostRange> g_host_ranges;

bool host_known(const void *p, size_t bytes)
{
    if (!p) return false;
    const uintptr_t a = (uintptr_t)p, b = a + bytes;
    std::lock_guard<std::mutex> lk(g_host_mu);
    for (const HostRange &r : g_host_ranges)
        if (a >= r.lo && b <= r.hi) return true;
    return false;
}

struct PinnedBuf {
    void *p = nullptr;
    size_t bytes = 0;
    int ensure(size_t need)
    {
        if (need <= bytes) return IVFADC_OK;
        if (p) { (void)hipHostFree(p); p = nullptr; bytes = 0; }
        const size_t want = need + need / 4;
        hipError_t e = hipHostMalloc(&p, want, hipHostMallocPortable | hipHostMallocMapped);
        if (e != hipSuccess) { p = nullptr; return fail(IVFADC_ERR_HIP, "hipHostMalloc(%zu) failed: %s", want, hipGetErrorString(e)); }
        bytes = want;
        return IVFADC_OK;
    }
    void release()
    {
        if (p) (void)hipHostFree(p);
        p = nullptr;
        bytes = 0;
    }
};

// ---- host <-> device copies of PAGEABLE memory go through the library's own page-locked bounce buffers ---------------------------------
// hipMemcpy{,Async} stages pageable copies of up to 1 MB itself; beyond that the runtime page-locks the CALLER's pages, lets the copy
// engine read or write them in place ("HSA Copy Using Pinned resource", rocblit.cpp; tools/pin_probe.py), and keeps the locked mapping in
// a cache keyed by address.  The callers here are short-lived std::vectors and numpy arrays on the malloc heap: freed, trimmed, handed out
// again at the same address -- and one run in four of the `-m gpu` suite died with "Memory access fault by GPU ... on address <a heap
// page>", the host inside ivfadc_set_lists uploading a 1-2 MB staging vector (round 5; found with the abort trace below and
// pytest --capture=sys).  So nothing pageable larger than BOUNCE_DIRECT_MAX is handed to the runtime: it is copied in 4 MB pieces through
// two page-locked buffers of the library's own (one process-wide pair, a mutex around a copy; the memcpy of piece i + 1 overlaps the
// transfer of piece i).  Both calls return when the data has arrived (they synchronise `s`).
constexpr size_t BOUNCE_DIRECT_MAX = (size_t)256 << 10;
constexpr size_t BOUNCE_PIECE = (size_t)4 << 20;
struct Bounce {
    std::mutex mu;
    void *buf[2] = {nullptr, nullptr};
    int ensure()
    {
        for (int i = 0; i < 2; ++i)
            if (!buf[i]) {
                hipError_t e = hipHostMalloc(&buf[i], BOUNCE_PIECE, hipHostMallocPortable | hipHostMallocMapped);
                if (e != hipSuccess) { buf[i] = nullptr; return fail(IVFADC_ERR_HIP, "hipHostMalloc(bounce buffer) failed: %s", hipGetErrorString(e)); }
            }
        return IVFADC_OK;
    }
};
Bounce g_bounce;

int h2d_copy(void *dst, const void *src, size_t bytes, hipStream_t s)
{
    if (bytes == 0) return IVFADC_OK;
    if (bytes <= BOUNCE_DIRECT_MAX) {
        HIP_TRY(hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, s));
        HIP_TRY(hipStreamSynchronize(s));
        return IVFADC_OK;
    }
    std::lock_guard<std::mutex> lk(g_bounce.mu);
    TRY(g_bounce.ensure());
    int i = 0;
    for (size_t off = 0; off < bytes; off += BOUNCE_PIECE, i ^= 1) {
        const size_t n = std::min(BOUNCE_PIECE, bytes - off);
        memcpy(g_bounce.buf[i], (const char *)src + off, n);                 // (buf[i]'s previous transfer was waited for below)
        if (off) HIP_TRY(hipStreamSynchronize(s));                           // the transfer out of the OTHER buffer: it overlapped this memcpy
        HIP_TRY(hipMemcpyAsync((char *)dst + off, g_bounce.buf[i], n, hipMemcpyHostToDevice, s));
    }
    HIP_TRY(hipStreamSynchronize(s));
    return IVFADC_OK;
}

int d2h_copy(void *dst, const void *src, size_t bytes, hipStream_t s)
{
    if (bytes == 0) return IVFADC_OK;
    if (bytes <= BOUNCE_DIRECT_MAX) {
        HIP_TRY(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
        return IVFADC_OK;
    }
    std::lock_guard<std::mutex> lk(g_bounce.mu);
    TRY(g_bounce.ensure());
    int i = 0;
    size_t prev_off = 0, prev_n = 0;
    for (size_t off = 0; off < bytes; off += BOUNCE_PIECE, i ^= 1) {
        const size_t n = std::min(BOUNCE_PIECE, bytes - off);
        HIP_TRY(hipMemcpyAsync(g_bounce.buf[i], (const char *)src + off, n, hipMemcpyDeviceToHost, s));
        if (prev_n) memcpy((char *)dst + prev_off, g_bounce.buf[i ^ 1], prev_n);   // the previous piece (waited for at the end of its turn)
        HIP_TRY(hipStreamSynchronize(s));
        prev_off = off;
        prev_n = n;
    }
    if (prev_n) memcpy((char *)dst + prev_off, g_bounce.buf[i ^ 1], prev_n);
    return IVFADC_OK;
}

}  // namespace

// ---- environment -------------------------------------------------------------------------------------------------------------------
// The library reads EIGHT environment variables (include/ivfadc_hip.h lists them), with getenv where they are used: switches a deployment
// may need without a rebuild -- validation (exact kernels only), safety valves (no zero-copy host access, no stream probing, one batch in
// flight), the abort trace.

// ---- thread safety ------------------------------------------------------------------------------------------------------------------
// Every entry point locks its handle (a recursive mutex: entry points call each other), so calls on ONE handle from several threads
// are serialised; calls on DIFFERENT handles -- an index and its views, or unrelated indexes -- run concurrently, which is what
// ivfadc_clone_view is for.  What ties handles together is guarded by one process-wide mutex, g_topo_mu: the list of an index's views,
// a view's link to its index, the generation numbers.  Lock order: handle (index) -> g_topo_mu -> handle (view); a view's own calls
// take g_topo_mu only hand-over-hand in front of their own mutex (HandleLock) and NEVER behind it (check_view_current reads the link and
// the generation under the view's own mutex: their writers hold it), a mutator holds g_topo_mu and every view's mutex for
// as long as it edits the lists (MutationScope): no view search starts, or is still being enqueued, while the lists change, and the
// first one afterwards sees the new generation and refuses.
static std::recursive_mutex g_topo_mu;
static uint64_t next_handle_serial()
{
    static std::atomic<uint64_t> g_serial{0};
    return g_serial.fetch_add(1, std::memory_order_relaxed) + 1;
}

// an int that may be read without the handle's lock (make_plan's hint)
struct RelaxedInt {
    std::atomic<int> v{0};
    int load() const { return v.load(std::memory_order_relaxed); }
    void store(int x) { v.store(x, std::memory_order_relaxed); }
    void fetch_add(int x) { v.fetch_add(x, std::memory_order_relaxed); }
    int fetch_add_get(int x) { return v.fetch_add(x, std::memory_order_relaxed); }
};

// ---- the handle, in ownership groups -----------------------------------------------------------------------------------------------
// ivfadc_index is composed of the plain structs below ("The handle is its ownership groups").  A group that holds DevBufs
// names them ONCE, in its each_buf, next to their declarations: ivfadc_destroy releases every group through it, clone_view aliases the
// shared groups through it.  A new buffer is declared in its group and listed in that group's each_buf -- nowhere else.

// shape and device: copied to a view
struct Dims {
    int device = 0;
    int d = 0, kc = 0, m = 0, ksub = 0, dsub = 0, cs = 0;
    int num_cu = 256;
    // U = UInt16 (ivfadc_create_u16, u16scan.hip.h): the host mirror and the device hold CODEWORD INDICES (little-endian uint16, cb = 2m
    // bytes per point); labels are translated at the boundary (set / get lists, encode, save / load), so a table needs m x ksub slots
    bool u16 = false;
    int cb = 0;                        // code bytes per point of the host mirror: m (UInt8) or 2m (UInt16)
};

// the quantizers and every operand derived from them: written by ivfadc_create (the two-level grouping: by the index's first search of
// a large quantizer), immutable afterwards; a view aliases the buffers and copies the rest
struct Quantizers {
    DevBuf centroids, codebooks, codebooks_t, codebooks_p, labels, cnorm;
    DevBuf label_inv;            // 8-bit handles: label byte -> codeword index, [m][256] (pack::label_inverse; recon_decode_kernel)
    // lower-bound tables on the matrix cores (lbscan.hip.h): bf16 split of the codebook, ||codeword||^2 and the f32 codewords, all in
    // label order, and max ||codeword|| per sub-quantizer; present for the shapes lb_shape() names
    DevBuf lb_split, lb_n2, lb_lab, lb_maxn;
    DevBuf lb_f16, lb_isc;       // round 5: f16 codewords x 2^e_ii and 2^-e_ii for the one-product build (lb_build_tables_f16)
    // narrow-field list-major scan (nfscan.hip.h; m = 8, dsub = 16, ksub = 256): ||codeword||^2 by codeword index, f32 codewords by label
    DevBuf nf_n2, nf_lab;
    DevBuf cent_t;               // small-batch path (smallq.hip.h): centroids regrouped [d / 4][kc][4]
    DevBuf cent_hi, cent_lo;     // bf16 split operands of coarse_bf16_kernel ([rows][dp], dp = d rounded up to 32)
    DevBuf cent_f16;             // round 5: the one-product f16 form of the same filter: scaled f16 centroids
    float f16_scale = 0.f;       // power of two: 2^11 <= scale * max|centroid component| <= 2^12 (0: the form is not available)
    int dp32 = 0;
    float cmaxn = 0.f;            // >= max ||centroid||, for the MFMA filter's error bound
    // certified two-level coarse search (twolevel.hip.h): group centres [G][d], slot ranges, radii, grouped centroids, slot -> cluster id
    DevBuf tl_centres, tl_off, tl_rad, tl_cent, tl_slot;
    int tl_G = 0;
    bool tl_tried = false, tl_use = false;
    float tl_eps = 0.f, tl_probe_fraction = -1.f;
    list_mirror::LabelMap labmap;      // code labels <-> codeword indices, on the host (the entries validate and convert through it)
    // the residual quantizer's rotation as loaded from an index file (nrows x nrows, column by column as persistency.jl:62-64 writes it);
    // empty = identity (:pq).  knn_search never reads it (index.jl:204-258): a rotated (:opq) index is SEARCHED as it is; quantize_data --
    // push! / encode -- would need it (third-party arithmetic, unverifiable here), so those entries refuse on such a handle.
    std::vector<float> rot;
    template <class F> void each_buf(F f)
    {
        for (DevBuf *b : {&centroids, &codebooks, &codebooks_t, &codebooks_p, &labels, &cnorm, &label_inv, &lb_split, &lb_n2, &lb_lab, &lb_maxn, &lb_f16, &lb_isc,
                          &nf_n2, &nf_lab, &cent_t, &cent_hi, &cent_lo, &cent_f16, &tl_centres, &tl_off, &tl_rad, &tl_cent, &tl_slot})
            f(*b);
    }
};

// the inverted lists as the device holds them: a view aliases the buffers and copies the layout; a subset view (ivfadc_clone_subset) OWNS
// compacted ones of its own, and the scalars here are then the subset's.  (DeviceLayout: d_cap, d_pos, d_codeoff)
struct Lists : list_mirror::DeviceLayout {
    bool have_lists = false;
    bool synthetic = false;
    bool dirty = false;           // host mirror changed, device copy stale (StaleGuard)
    DevBuf list_pos, list_len, list_codeoff, codes, ids;
    template <class F> void each_buf(F f)
    {
        for (DevBuf *b : {&list_pos, &list_len, &list_codeoff, &codes, &ids}) f(*b);
    }
};

// (the host mirror, list_mirror::ListMirror: one (codes, ids) pair per list -- the source of truth; the device copy gives every list spare
// capacity so push! writes in place (re-layout only when a list overflows).  Its data stays with the index: a view is given the lengths.)

// every field a setter or an environment switch writes and the planners read: a view starts from its index's, and the second lane of
// ivfadc_search_batches is given the index's before every use (copy_search_config)
struct SearchConfig {
    bool lb_use_f16 = true;      // ivfadc_set_table_mode(h, 3): the three-product bf16 split instead (A/B)
    bool allow_nf = true;
    int wg8_mode = 0;            // ivfadc_set_tuning(h, 4, chunk) keeps the plan's choice; wg8_mode: 0 = where it pays, 1 = wherever it exists, -1 = never
    int u16_tables = 0;          // ivfadc_set_u16_tables: 0 per-pass ADC tables; 1 table-free (u16_direct_*_scan_kernel); 2 table-free where the rule of make_plan_u16 expects it to win
    bool u16_wide = false;       // table mode 10: a 16-bit handle runs 64 < K on the scan kernel's LDS-selector form (u16_wide_scan_kernel) where its LDS need fits
    bool wg8_wide = false;       // table modes 8 / 9: 64 < K <= 128 runs the kernel's wide-pool form (wg8_wide_scan_kernel) wherever wg8_mode takes the kernel
    // list-partitioned multi-GPU mode (ivfadc_set_list_partition): this handle scans the probed lists l with l % part_n == part_i only and
    // leaves partial top-K keys
    int part_n = 1, part_i = 0;
    bool allow_sq = true, sq_inside = false;
    bool allow_lb = true;
    bool force_lb = false;       // ivfadc_set_table_mode(h, 2): the matrix-core rounds wherever they are instantiated, not only where they pay
    bool allow_f16 = true;
    bool allow_bf16 = true;
    bool allow_prune = true;     // query-major scan: skip probes whose coarse distance exceeds the K-th best key (exact)
    bool allow_listed = true;    // listed mode: per-tile records instead of the score matrix (run_coarse)
    bool allow_filt = true;      // striped tables + rotated-order filter sums in the list-major kernels (ivfadc_set_table_mode)
    int tl_mode = 0;             // two-level coarse search: 0 = automatic (built on the first search of a large quantizer, used if a self-probe says the bounds cut), 1 = on, -1 = off
    bool allow_mfma = true;
    int mfma_min_kc = 2048;
    size_t ws_budget = (size_t)8 << 30;
    int force_qg = 0, force_chunk = 0;
};

// what one lane's searches write and read between their launches: a view starts with an empty one of its own
struct Workspace {
    DevBuf tmin, tlist;
    // eight-wave list-major scan (wg8scan.hip.h; m = 8, dsub = 4 / 8 / 12 / 16, ksub = 256, K <= 64, with the wide pool K <= 128; m = 16, dsub = 4 / 8, K <= 64): the work items'
    // f32 tables, 32 or 64 KB per workgroup
    DevBuf wg8_tabs, wg8_items;  // (wg8_items: work item -> list, written by bucket_scan_kernel)
    // list-partitioned mode: partial_keys: where the running call wants the partial top-K keys (null: ids as usual); the batch whose
    // probe arrays stand
    uint64_t *partial_keys = nullptr;
    int64_t partial_nq = -1;
    int partial_w = 0, partial_K = 0;
    DevBuf sq_keys, sq_cnt, sq_arrive;   // small-batch path (smallq.hip.h): partial results, arrival counters
    DevBuf q_hi, q_lo;           // the batch's bf16 split queries (coarse_bf16_kernel)
    DevBuf q_f16, q_flags;       // the batch's scaled f16 queries, per-query overflow flags
    bool last_coarse_f16 = false, last_coarse_bf16 = false, last_listed = false;   // what the last coarse launch ran (run_coarse)
    DevBuf tl_gdist;
    bool dev_entry = false;   // the running search came in through a device-pointer entry AND another lane of this replica searched since this
                              // handle's previous search (the caller drives several lanes side by side: see make_plan)
    DevBuf gen_a, gen_b, gen_tmp, gen_off, gen_tot;   // generic path: key buffers (sort in/out), rocPRIM scratch, offsets
    DevBuf rng_cnt, rng_off, rng_tot, rng_radii, rng_lims;   // range search (range.hip.h): item counts, their scan, per-query totals, the host entry's radii, a group's lims
    int tlist_ldq = 0;
    int tmin_tiles = 0, tmin_tile_w = 0;   // set by run_coarse when the last coarse launch wrote tile minima
    DevBuf app_stage;
    // ivfadc_set_next_queries: the hinted batch (good for one search), and the batch whose exact coarse rows stand in cdist2 -- written
    // by the tiles that rode behind the previous search's scan launch
    // A batch is named by (pointer, count, token): the token is the caller's generation number of the buffer's CONTENTS, so rows computed
    // from a buffer that has been refilled since can never be taken for the new contents.  pf_*: what the last search's riders wrote;
    // avail_*: what the running search may pick up (set at the top of search_dev, on every path, from pf_* -- rows serve the very next
    // search or none); cur_token: the token the caller declared for the next search's queries (ivfadc_set_query_token; 0 = undeclared)
    const float *hint_q = nullptr, *pf_q = nullptr, *avail_q = nullptr;
    int64_t hint_nq = 0, pf_nq = 0, avail_nq = 0;
    uint64_t hint_token = 0, pf_token = 0, cur_token = 0, own_token = 0;   // own_token: numbering of ivfadc_search_batches
    hipEvent_t hint_ev = nullptr;   // ivfadc_search_batches: the hinted rows are on the device once this event has fired (null: they are)
    DevBuf cdist2;
    DevBuf pre_list, pre_dc;   // ivfadc_search_preassigned (host pointers): the caller's probes on the device
    DevBuf mask_q;             // ivfadc_search_masked: the batch's mask numbers on the device, every value in [-1, nmasks)
    // ivfadc_locate / ivfadc_reconstruct (reconstruct.hip.h): sorted wanted ids, one key per wanted slot, the exact bitmap, the lists' chunk
    // prefix, rocPRIM scratch, and the host entries' staging of requests and results
    DevBuf rc_want, rc_best, rc_bitmap, rc_chunk, rc_tmp, rc_req, rc_list, rc_pos, rc_found, rc_vec;
    DevBuf sc_q, sc_ids, sc_cnt, sc_dist, sc_found;   // ivfadc_score_ids (host pointers): the caller's queries, ids and counts on the device, the results
    DevBuf q_stage, cdist, probe_list, probe_dc, probe_base, list_cnt, bucket_off, wi_off, cursor, bucket_items, misc,
        qthr, part_keys, part_cnt, out_ids, out_dists, out_counts, assign, enc_codes, pts_stage, dbg;
    PinnedBuf pin_in, pin_out;   // host staging of ivfadc_search: pageable user buffers <-> pinned (the kernels read / write it in place)
    bool hc_out_direct = false;   // the running host-pointer call: results go straight into the caller's arrays
    size_t qthr_armed = 0;       // entries of qthr known to hold KEY_MAX
    bool list_cnt_armed = false;
    template <class F> void each_buf(F f)
    {
        for (DevBuf *b : {&tmin, &tlist, &wg8_tabs, &wg8_items, &sq_keys, &sq_cnt, &sq_arrive, &q_hi, &q_lo, &q_f16, &q_flags, &tl_gdist, &gen_a, &gen_b,
                          &gen_tmp, &gen_off, &gen_tot, &rng_cnt, &rng_off, &rng_tot, &rng_radii, &rng_lims, &app_stage, &cdist2, &pre_list, &pre_dc, &mask_q, &rc_want, &rc_best, &rc_bitmap, &rc_chunk, &rc_tmp, &rc_req, &rc_list, &rc_pos, &rc_found, &rc_vec, &sc_q, &sc_ids, &sc_cnt, &sc_dist, &sc_found, &q_stage, &cdist, &probe_list, &probe_dc, &probe_base,
                          &list_cnt, &bucket_off, &wi_off, &cursor, &bucket_items, &misc, &qthr, &part_keys, &part_cnt, &out_ids, &out_dists,
                          &out_counts, &assign, &enc_codes, &pts_stage, &dbg})
            f(*b);
    }
};

// what belongs to this handle alone -- its lock and stream, statistics, feedback, the batches pipeline, the communicator, its place
// among the views: never copied, a view starts with the defaults written here (clone_view hands it prune_est and fn_cfg)
struct HandleState {
    std::recursive_mutex mu;
    hipStream_t stream = nullptr;
    bool own_stream = true;
    // one-process-per-GPU result merge inside the library (ivfadc_comm_*): this rank's communicator, a side stream for the
    // collectives and one completion event per result slot
    void *comm = nullptr;
    int comm_ranks = 0, comm_rank = 0;
    hipStream_t comm_stream = nullptr;
    hipEvent_t comm_ready = nullptr;
    static constexpr int COMM_SLOTS = 8;
    hipEvent_t comm_done[COMM_SLOTS] = {};
    bool comm_busy[COMM_SLOTS] = {};
    int64_t comm_collectives = 0;
    // collectives complete in issue order on the side stream: seq numbers them, comm_slot_seq[s] = the last one that read slot s, and a
    // search stream (this handle's, or a view's: its own copy of comm_waited) has waited for every collective up to comm_waited
    int64_t comm_seq = 0, comm_slot_seq[COMM_SLOTS] = {}, comm_waited = 0;
    // feedback for make_plan's probes-per-round choice: how much of what the query-major scans probed was pruned (see fb_poll / fb_snapshot)
    PinnedBuf fb_pin;          // 4 KB: a snapshot of the sharded counters
    hipEvent_t fb_ev = nullptr;
    bool fb_pending = false;
    int fb_countdown = 0;
    int64_t fb_sp = 0, fb_pp = 0;   // counters at the last snapshot that was read
    float prune_est = -1.0f;        // smoothed pruned fraction of the probed points (< 0: not known yet)
    RelaxedInt lane_ticket;   // root index only: one ticket per device-entry search on the index or any of its views
    int my_ticket = -1;       // this handle's last ticket
    RelaxedInt n_views;   // live views of this index (a hint for make_plan: several batches are in flight on this replica)
    int64_t inplace_appends = 0;
    hipStream_t copy_stream = nullptr;               // ivfadc_search_batches: query ingest ahead of the searches
    hipStream_t copy_probed_a = nullptr, copy_probed_b = nullptr;   // ... probed to run beside these two (ensure_overlap)
    std::vector<hipEvent_t> ingest_ev;               // ... one event per upload group
    ivfadc_host_stats hstats{};
    // cumulative counters of internal views that no longer exist (a stale second lane of ivfadc_search_batches)
    int64_t carry_queries = 0, carry_scanned = 0, carry_pruned = 0, carry_surv = 0, carry_fallbacks = 0, carry_launches = 0;

    // profiling
    bool profiling = false;
    int profiling_level = 0;
    struct EvPair { hipEvent_t a, b; int kind; };
    std::vector<EvPair> pending;
    std::vector<EvPair> free_ev;
    ivfadc_stats stats{};
    int64_t scanned_base = 0, fallback_base = 0, pruned_base = 0, surv_base = 0, visited_base = 0;
    struct FnCfg { const void *fn; size_t lds; int occ; };
    std::vector<FnCfg> fn_cfg;

    // Read-only views (ivfadc_clone_view): a second handle on the SAME device arrays of quantizers and lists, with a stream and a
    // workspace of its own, so that two batches can be in flight on one replica (a SIFT1M-shape launch is 1024 workgroups that all start
    // together: its ramp and its tail leave the chip half empty, and a second stream fills them).  A view holds no host mirror and cannot
    // change anything; any change to the index it was taken from (generation) makes it refuse to search.
    ivfadc_index *view_of = nullptr;
    bool is_view = false, orphan = false;
    bool is_subset = false;   // a view with lists of its own (ivfadc_clone_subset): a mask set of the index does not describe them
    // what a mask set remembers of the index it was made from (ivfadc_maskset_create): a process-wide serial number, not the pointer --
    // a new index may be allocated at a freed one's address
    uint64_t serial = next_handle_serial();
    uint64_t generation = 0, view_gen = 0;
    std::vector<ivfadc_index *> views;
    ivfadc_index *pipe_view = nullptr;            // ivfadc_search_batches' second lane (created on first use)
    hipEvent_t pipe_ev_in = nullptr;
};

struct ivfadc_index : Dims, Quantizers, Lists, SearchConfig, Workspace, HandleState {
    list_mirror::ListMirror mirror;   // lengths of every handle; codes and ids of an index (never of a view)
    // every DevBuf of the handle, each group once
    template <class F> void each_buf(F f)
    {
        Quantizers::each_buf(f);
        Lists::each_buf(f);
        Workspace::each_buf(f);
    }
};

// A mask set (ivfadc_maskset_create; maskset_plan.h, maskset.hip.h): nmasks slot-space bitmaps of the lists of ONE index as they stood at
// ONE generation.  Immutable once made: any number of handles and threads search with it at once, nothing here is written again.
struct ivfadc_maskset {
    int device = 0;
    DevBuf words;       // [nmasks][W] u32
    DevBuf word_off;    // [kc + 1] u64
    int nmasks = 0, kc = 0;
    uint64_t W = 0;
    uint64_t index_serial = 0, generation = 0;   // the index it was made from (HandleState::serial) and that index's generation then
};

// The result of a range search (ivfadc_range_search; range.hip.h): CSR rows in device memory the RESULT owns -- allocated for it alone, in no
// ownership group of the handle -- complete when the search returns.  It holds no pointer to the handle: it outlives later searches, the
// handle's mutators and the handle itself, and goes only by ivfadc_range_result_destroy.
struct ivfadc_range_result {
    int device = 0;
    int64_t nq = 0, total = 0;
    std::vector<int64_t> lims;     // [nq + 1], the host's copy
    int64_t *d_lims = nullptr;     // [nq + 1]
    uint32_t *d_ids = nullptr;     // [max(total, 1)]
    float *d_dists = nullptr;      // [max(total, 1)]
    ~ivfadc_range_result()
    {
        if (!d_lims && !d_ids && !d_dists) return;
        int prev = -1;   // the calling thread's current device is the caller's: left as it was
        if (hipGetDevice(&prev) != hipSuccess) prev = -1;
        if (hipSetDevice(device) != hipSuccess) return;
        if (d_lims) (void)hipFree(d_lims);
        if (d_ids) (void)hipFree(d_ids);
        if (d_dists) (void)hipFree(d_dists);
        if (prev >= 0 && prev != device) (void)hipSetDevice(prev);
    }
};

// the lock of an entry point on handle h (null: nothing to lock).  A view takes the topology mutex first and lets it go once its own
// mutex is held: a mutator of its index, which holds the topology mutex while it waits for the views, is never waited for in a cycle.
struct HandleLock {
    ivfadc_index *h;
    explicit HandleLock(ivfadc_index *x) : h(x)
    {
        if (!h) return;
        if (h->is_view) {
            std::lock_guard<std::recursive_mutex> topo(g_topo_mu);
            h->mu.lock();
        } else {
            h->mu.lock();
        }
    }
    ~HandleLock() { if (h) h->mu.unlock(); }
    HandleLock(const HandleLock &) = delete;
    HandleLock &operator=(const HandleLock &) = delete;
};

namespace {

// Low-latency wait for short batches: hipStreamSynchronize can take a sleep/interrupt path that adds a few
// hundred microseconds; poll for up to ~2 ms first.
int wait_stream(ivfadc_index *h)
{
    for (int i = 0; i < 200000; ++i) {
        const hipError_t e = hipStreamQuery(h->stream);
        if (e == hipSuccess) return IVFADC_OK;
        if (e != hipErrorNotReady) return fail(IVFADC_ERR_HIP, "hipStreamQuery failed: %s", hipGetErrorString(e));
        if (i > 20000) break;
    }
    HIP_TRY(hipStreamSynchronize(h->stream));
    return IVFADC_OK;
}

int set_device(ivfadc_index *h)
{
    HIP_TRY(hipSetDevice(h->device));
    return IVFADC_OK;
}

// b <- bytes of host memory, grown to fit (synchronous: h2d_copy)
int upload(ivfadc_index *h, DevBuf &b, const void *src, size_t bytes)
{
    TRY(b.ensure(bytes));
    return h2d_copy(b.p, src, bytes, h->stream);
}
template <class T> int upload(ivfadc_index *h, DevBuf &b, const std::vector<T> &v) { return upload(h, b, v.data(), v.size() * sizeof(T)); }

// ---- events ------------------------------------------------------------------------------
int ev_begin(ivfadc_index *h, int kind, ivfadc_index::EvPair &ep)
{
    if (!h->free_ev.empty()) {
        ep = h->free_ev.back();
        h->free_ev.pop_back();
    } else {
        HIP_TRY(hipEventCreate(&ep.a));
        HIP_TRY(hipEventCreate(&ep.b));
    }
    ep.kind = kind;
    HIP_TRY(hipEventRecord(ep.a, h->stream));
    return IVFADC_OK;
}

int ev_end(ivfadc_index *h, ivfadc_index::EvPair &ep)
{
    HIP_TRY(hipEventRecord(ep.b, h->stream));
    h->pending.push_back(ep);
    return IVFADC_OK;
}

int ev_fold(ivfadc_index *h)
{
    if (h->pending.empty()) return IVFADC_OK;
    HIP_TRY(hipStreamSynchronize(h->stream));
    for (auto &ep : h->pending) {
        float ms = 0.f;
        HIP_TRY(hipEventElapsedTime(&ms, ep.a, ep.b));
        if (ep.kind == 0) { h->stats.scan_ms += ms; h->stats.scan_launches++; }
        else if (ep.kind == 2) { h->stats.lb_build_ms += ms; h->stats.lb_build_launches++; }
        else h->stats.coarse_ms += ms;
        h->free_ev.push_back(ep);
    }
    h->pending.clear();
    return IVFADC_OK;
}

// ---- device layout of the lists --------------------------------------------------------------
using list_mirror::CODE_SLACK;

int code_stride(int m) { return (int)align_up((size_t)m, 4); }   // every kernel variant reads this stride

// a list_mirror::Error in the entries' words.  wide: the codes are UInt16; prefix: the loader's "<path>: "
int mirror_fail(const list_mirror::Error &e, bool wide, const char *prefix = "")
{
    typedef list_mirror::Error E;
    switch (e.kind) {
    case E::None: return IVFADC_OK;
    case E::OffsetsStart: return fail(IVFADC_ERR_INVALID, "offsets[0] must be 0");
    case E::OffsetsOrder: return fail(IVFADC_ERR_INVALID, "offsets must be non-decreasing (list %d)", (int)e.list);
    case E::TooManyPoints: return fail(IVFADC_ERR_ASSERT, "index capacity of UInt32 ids exceeded");
    case E::NullArrays: return fail(IVFADC_ERR_INVALID, "null codes/ids");
    case E::TooManySlots: return fail(IVFADC_ERR_INVALID, "id array with spare capacity exceeds 2^32 slots");
    case E::NotALabel:
        return fail(IVFADC_ERR_INVALID, "%scode %s%d of point %lld is not a label of codebook %d", prefix, wide ? "" : "byte ", e.value,
                    (long long)e.point, e.codebook);
    case E::DuplicateLabel: return fail(IVFADC_ERR_INVALID, "%sduplicate label %d in codebook %d", prefix, e.value, e.codebook);
    }
    return fail(IVFADC_ERR_INVALID, "list mirror error %d", (int)e.kind);
}

// h->d_cap -> offsets of every list in the id array and in the code buffer, and the handle's n and maxlen (list_mirror.h)
int layout_from_caps(ivfadc_index *h, list_mirror::LayoutTotals &tot)
{
    TRY(mirror_fail(list_mirror::layout_from_caps(*h, h->mirror.h_len, h->cs, tot), h->u16));
    h->mirror.maxlen = tot.maxlen;
    h->mirror.n = tot.n;
    return IVFADC_OK;
}

int upload_list_tables(ivfadc_index *h)
{
    const int kc = h->kc;
    std::vector<uint32_t> len32((size_t)kc);
    for (int l = 0; l < kc; ++l) len32[l] = (uint32_t)h->mirror.h_len[l];
    TRY(h->list_pos.ensure((size_t)kc * 8));
    TRY(h->list_len.ensure((size_t)kc * 4));
    TRY(h->list_codeoff.ensure((size_t)kc * 8));
    TRY(h2d_copy(h->list_pos.p, h->d_pos.data(), (size_t)kc * 8, h->stream));       // (synchronous: h2d_copy)
    TRY(h2d_copy(h->list_len.p, len32.data(), (size_t)kc * 4, h->stream));
    TRY(h2d_copy(h->list_codeoff.p, h->d_codeoff.data(), (size_t)kc * 8, h->stream));
    return IVFADC_OK;
}

// The device copy of the lists is stale until proven current.  Whoever is about to change the mirror, or the device copy itself, makes
// one of these FIRST: the handle is marked stale there and then, and current() declares the copy current again only once the device
// update has been queued and, where its staging is stack-owned, synchronised.  So a failure half-way (allocation, copy, launch) leaves
// a handle whose next search lays the lists out again from the mirror, never one that searches stale lists; and a mutator that found
// the copy already stale (!in_place()) edits the mirror only.
struct StaleGuard {
    ivfadc_index *h;
    const bool was_dirty;
    explicit StaleGuard(ivfadc_index *x) : h(x), was_dirty(x->dirty) { h->dirty = true; }
    bool in_place() const { return h->have_lists && !was_dirty; }   // the device copy was current: the edit can be repeated on it
    void current() { h->dirty = false; }
};

// full re-layout: host mirror -> device, every list gets spare capacity behind it
int upload_lists(ivfadc_index *h)
{
    StaleGuard stale(h);
    h->d_cap.resize((size_t)h->kc);
    for (int l = 0; l < h->kc; ++l) h->d_cap[l] = list_mirror::spare_cap(h->mirror.h_len[l]);
    list_mirror::LayoutTotals tot;
    TRY(layout_from_caps(h, tot));
    std::vector<uint8_t> stage;
    std::vector<uint32_t> idstage;
    h->mirror.stage(*h, tot, h->cb, h->cs, stage, idstage);
    TRY(h->codes.ensure(stage.size()));
    TRY(h->ids.ensure(idstage.size() * 4));
    TRY(h2d_copy(h->codes.p, stage.data(), stage.size(), h->stream));
    TRY(h2d_copy(h->ids.p, idstage.data(), idstage.size() * 4, h->stream));
    TRY(upload_list_tables(h));
    h->have_lists = true;
    h->synthetic = false;
    stale.current();
    return IVFADC_OK;
}

// ---- scan kernel dispatch ----------------------------------------------------------------------
typedef void (*scan_fn_t)(const ScanArgs);
typedef void (*qscan_fn_t)(const QScanArgs);

// Specialised (m, dsub) pairs; every other shape runs the fully generic <0, 0> kernels.
template <int M, int DS, bool SMALL> scan_fn_t scan_fn_qg(int qg, bool stripe)
{
    if constexpr ((M == 8 || M == 16) && DS > 0) {
        if (stripe && qg == 4) return scan_kernel<M, DS, 4, SMALL, true>;
    }
    switch (qg) {
    case 1: return scan_kernel<M, DS, 1, SMALL>;
    case 2: return scan_kernel<M, DS, 2, SMALL>;
    default: return scan_kernel<M, DS, 4, SMALL>;
    }
}

template <int M, int DS, bool SMALL> qscan_fn_t qscan_fn_pg(int pg)
{
    switch (pg) {
    case 1: return qscan_kernel<M, DS, 1, SMALL>;
    case 2: return qscan_kernel<M, DS, 2, SMALL>;
    default: return qscan_kernel<M, DS, 4, SMALL>;
    }
}

#define IVF_SHAPES(X) X(8, 16) X(16, 6) X(16, 8) X(48, 16)

// (the shapes the matrix-core lower-bound rounds -- qscan_kernel<..., LB = true> -- are instantiated for: lb_shape, scan_layouts.h)
template <int M, int DS> qscan_fn_t pick_qscan_lb_pg(int pg)
{
    switch (pg) {
    case 1: return qscan_kernel<M, DS, 1, true, true>;
    case 2: return qscan_kernel<M, DS, 2, true, true>;
    case 3: return qscan_kernel<M, DS, 3, true, true>;
    default: return qscan_kernel<M, DS, 4, true, true>;
    }
}

qscan_fn_t pick_qscan_lb(int m, int dsub, int pg)
{
    if (m == 48 && dsub == 16) return pick_qscan_lb_pg<48, 16>(pg);
    if (m == 16 && dsub == 6) return pick_qscan_lb_pg<16, 6>(pg);
    return nullptr;
}

// the plan's LDS figure of these kernels (lb_lds_bytes, scan_layouts.h) is the kernel's own layout: LbCfg<M, DS, PG>::END, and behind it
// the tail qscan_body carves (FwTail), whose size does not depend on where it stands
template <int M, int DS, int PG> constexpr size_t lb_kernel_lds = LbCfg<M, DS, PG>::END + fw_tail(0, PG).end;
#define X(M_, D_, P_) static_assert(lb_lds_bytes(M_, D_, P_) == lb_kernel_lds<M_, D_, P_>, "the planned LDS bytes of qscan_kernel<M, DS, PG, true, true> are its carve");
IVF_LB_SHAPES(X)
#undef X

template <bool SMALL> scan_fn_t pick_scan_s(int m, int dsub, int qg, bool stripe)
{
#define X(M_, D_) if (m == M_ && dsub == D_) return scan_fn_qg<M_, D_, SMALL>(qg, stripe);
    IVF_SHAPES(X)
#undef X
    return scan_fn_qg<0, 0, SMALL>(qg, false);
}

template <bool SMALL> qscan_fn_t pick_qscan_s(int m, int dsub, int pg)
{
#define X(M_, D_) if (m == M_ && dsub == D_) return qscan_fn_pg<M_, D_, SMALL>(pg);
    IVF_SHAPES(X)
#undef X
    return qscan_fn_pg<0, 0, SMALL>(pg);
}

scan_fn_t pick_scan(int m, int dsub, int qg, bool small, bool stripe)
{
    return small ? pick_scan_s<true>(m, dsub, qg, stripe) : pick_scan_s<false>(m, dsub, qg, stripe);
}

qscan_fn_t pick_qscan(int m, int dsub, int pg, bool small)
{
    return small ? pick_qscan_s<true>(m, dsub, pg) : pick_qscan_s<false>(m, dsub, pg);
}

// query-major scan with the next batch's coarse tiles behind it (qscan_coarse_kernel): the register-selector kernels of the shapes below
typedef void (*qscan_coarse_fn_t)(const QScanArgs, const CoarseNext);
qscan_coarse_fn_t pick_qscan_coarse(int m, int dsub, int pg)
{
    if (pg != 1 && pg != 2) return nullptr;
    if (m == 8 && dsub == 16) return pg == 1 ? qscan_coarse_kernel<8, 16, 1> : qscan_coarse_kernel<8, 16, 2>;
    if (m == 16 && dsub == 8) return pg == 1 ? qscan_coarse_kernel<16, 8, 1> : qscan_coarse_kernel<16, 8, 2>;
    if (m == 16 && dsub == 6) return pg == 1 ? qscan_coarse_kernel<16, 6, 1> : qscan_coarse_kernel<16, 6, 2>;
    if (m == 48 && dsub == 16) return nullptr;   // three workgroups per CU at 168 registers: not worth a second instantiation
    return pg == 1 ? qscan_coarse_kernel<0, 0, 1> : qscan_coarse_kernel<0, 0, 2>;
}

typedef void (*sq_fn_t)(const SqArgs);
sq_fn_t pick_sq(int m, int dsub)
{
#define X(M_, D_) if (m == M_ && dsub == D_) return sq_kernel<M_, D_>;
    IVF_SHAPES(X)
#undef X
    return sq_kernel<0, 0>;
}

// (filt_shape, nf_shape, w8_dsub, w8_m16_dsub -- the shapes the striped, the narrow-field and the eight-wave kernels are instantiated
// for -- and the LDS figures of all of them: scan_layouts.h)
typedef void (*nf_fn_t)(const ScanArgs, const NfView);
typedef void (*u16_fn_t)(const ScanArgs, int);
typedef void (*wg8_fn_t)(const ScanArgs, float *, const u32 *, u32 *, int);
wg8_fn_t pick_wg8(bool q8, int m, int dsub)
{
    if (m == 16) {
#define X(D_) if (dsub == D_) return q8 ? wg8_m16_scan_kernel<8, D_> : wg8_m16_scan_kernel<4, D_>;
        X(4) X(8)
#undef X
        return nullptr;
    }
    if (m != 8) return nullptr;
    if (dsub == 16) return q8 ? wg8_scan_kernel<8> : wg8_scan_kernel<4>;
#define X(D_) if (dsub == D_) return q8 ? wg8_scan_kernel<8, D_> : wg8_scan_kernel<4, D_>;
    X(4) X(8) X(12)
#undef X
    return nullptr;
}
// the wide-pool form (two pool entries per lane: 64 < K <= W8_WIDE_MAX_K; table modes 8 / 9)
wg8_fn_t pick_wg8_wide(bool q8, int dsub)
{
#define X(D_) if (dsub == D_) return q8 ? wg8_wide_scan_kernel<8, D_> : wg8_wide_scan_kernel<4, D_>;
    X(4) X(8) X(12) X(16)
#undef X
    return nullptr;
}
// misc device block: [0, 4096) 64 scanned-point counters at a 64-B stride; [4096] work-queue head; [4096 + 64] coarse fallbacks;
// [4096 + 256, + 512) the eight per-XCD queue heads of the narrow-field kernel, 64 B apart
constexpr size_t MISC_BYTES = 4096 + 256 + 512 + 4096;
constexpr size_t MISC_SINK = 4096 + 256 + 512;   // 64 counter lines nobody reads: where a coarse search alone (ivfadc_coarse_search) sends the B_alg counts of its top-w kernel
// the eight queue heads of the narrow-field and the eight-wave kernel, zeroed in front of the launch that pulls from them
int clear_xcd_heads(ivfadc_index *h, u32 *&xq)
{
    xq = (u32 *)((char *)h->misc.p + 4096 + 256);
    HIP_TRY(hipMemsetAsync(xq, 0, 512, h->stream));
    return IVFADC_OK;
}

// ---- the plan of a search: plan.h decides (a pure function of PlanFacts), this file reads the handle and picks the kernel -------------
// Feedback for the probes-per-round choice of plan_query_major (PG1_MIN_PRUNED in plan.h says why): every few searches a 4 KB snapshot
// of the scan kernels' probed / pruned counters follows the scan on the stream into pinned memory, and a later search that finds it
// arrived (hipEventQuery: no wait, ever) folds the pruned fraction into h->prune_est.
int fb_poll(ivfadc_index *h)
{
    if (!h->fb_pending) return IVFADC_OK;
    const hipError_t q = hipEventQuery(h->fb_ev);
    if (q == hipErrorNotReady) return IVFADC_OK;
    if (q != hipSuccess) return fail(IVFADC_ERR_HIP, "hipEventQuery failed: %s", hipGetErrorString(q));
    h->fb_pending = false;
    const int64_t *sh = (const int64_t *)h->fb_pin.p;
    int64_t sp = 0, pp = 0;
    for (int i = 0; i < 64; ++i) { sp += sh[i * 8]; pp += sh[i * 8 + 1]; }
    const int64_t dsp = sp - h->fb_sp, dpp = pp - h->fb_pp;
    h->fb_sp = sp;
    h->fb_pp = pp;
    if (dsp > 0 && dpp >= 0 && dpp <= dsp) {
        const float f = (float)((double)dpp / (double)dsp);
        h->prune_est = h->prune_est < 0.0f ? f : 0.5f * h->prune_est + 0.5f * f;
    }
    return IVFADC_OK;
}
int fb_snapshot(ivfadc_index *h)   // behind a query-major scan launch, on its stream
{
    if (h->fb_pending || !h->misc.p) return IVFADC_OK;
    if (--h->fb_countdown > 0) return IVFADC_OK;
    h->fb_countdown = 8;
    TRY(h->fb_pin.ensure(4096));
    if (!h->fb_ev) HIP_TRY(hipEventCreateWithFlags(&h->fb_ev, hipEventDisableTiming));
    HIP_TRY(hipMemcpyAsync(h->fb_pin.p, h->misc.p, 4096, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipEventRecord(h->fb_ev, h->stream));
    h->fb_pending = true;
    return IVFADC_OK;
}

// the ONE place that reads the handle for planning
PlanFacts plan_facts(const ivfadc_index *h)
{
    PlanFacts f;
    f.d = h->d; f.kc = h->kc; f.m = h->m; f.dsub = h->dsub; f.ksub = h->ksub;
    f.n = h->mirror.n; f.maxlen = h->mirror.maxlen;
    f.num_cu = h->num_cu;
    f.u16 = h->u16;
    f.allow_filt = h->allow_filt; f.allow_lb = h->allow_lb; f.force_lb = h->force_lb; f.allow_nf = h->allow_nf;
    f.allow_prune = h->allow_prune; f.allow_mfma = h->allow_mfma; f.mfma_min_kc = h->mfma_min_kc;
    f.wg8_mode = h->wg8_mode; f.wg8_wide = h->wg8_wide; f.u16_tables = h->u16_tables; f.part_n = h->part_n;
    f.force_qg = h->force_qg; f.force_chunk = h->force_chunk; f.ws_budget = h->ws_budget;
    f.tl_use = h->tl_use; f.tl_G = h->tl_G;
    f.prune_est = h->prune_est;
    f.have_lb_operands = h->lb_split.p != nullptr;
    f.have_nf_operands = h->nf_n2.p != nullptr;
    f.lanes_active = h->dev_entry && (h->is_view || h->n_views.load() > 0);
    return f;
}

// masked_scan_kernel (maskset.hip.h): any m, dsub, ksub <= 256; groups of 1 / 2 / 4, register / LDS selectors
masked_fn_t pick_masked(int qg, bool small)
{
    if (small) return qg == 4 ? masked_scan_kernel<4, true> : (qg == 2 ? masked_scan_kernel<2, true> : masked_scan_kernel<1, true>);
    return qg == 4 ? masked_scan_kernel<4, false> : (qg == 2 ? masked_scan_kernel<2, false> : masked_scan_kernel<1, false>);
}

// the kernel of a planned form (Plan::fn)
int plan_kernel(Plan &pl, int m, int dsub)
{
    switch (pl.form) {
    case ScanForm::QueryMajor: pl.fn = (const void *)pick_qscan(m, dsub, pl.qg, pl.small_k); break;
    case ScanForm::QueryMajorLb: pl.fn = (const void *)pick_qscan_lb(m, dsub, pl.qg); break;
    case ScanForm::FourWave: pl.fn = (const void *)pick_scan(m, dsub, pl.qg, pl.small_k, pl.stripe); break;
    case ScanForm::NarrowField: pl.fn = (const void *)(nf_fn_t)nf_scan_kernel<4>; break;   // four points per lane and step (measured: two 9.2 ms, eight 8.1 ms -- and 74 spilled registers -- against 7.76 ms)
    case ScanForm::EightWave:
        pl.fn = (const void *)(pl.wide ? (m == 8 ? pick_wg8_wide(pl.q8, dsub) : nullptr) : pick_wg8(pl.q8, m, dsub));
        if (!pl.fn) return fail(IVFADC_ERR_STATE, "eight-wave scan planned for m = %d, dsub = %d, which has no instantiation", m, dsub);
        break;
    case ScanForm::U16: pl.fn = (const void *)(u16_fn_t)u16_scan_kernel; break;
    case ScanForm::U16Wide: pl.fn = (const void *)(u16_fn_t)u16_wide_scan_kernel; break;
    case ScanForm::U16Direct: pl.fn = (const void *)(u16_fn_t)u16_direct_scan_kernel; break;
    case ScanForm::U16DirectWide: pl.fn = (const void *)(u16_fn_t)u16_direct_wide_scan_kernel; break;
    case ScanForm::Masked: pl.fn = (const void *)pick_masked(pl.qg, pl.small_k); break;
    }
    return IVFADC_OK;
}

int ensure_common_ws(ivfadc_index *h)
{
    const int kc = h->kc;
    TRY(h->list_cnt.ensure((size_t)kc * 4));
    TRY(h->bucket_off.ensure((size_t)(kc + 1) * 4));
    TRY(h->wi_off.ensure((size_t)(kc + 1) * 4));
    TRY(h->cursor.ensure((size_t)kc * 4));
    TRY(h->misc.ensure(MISC_BYTES));
    if (!h->list_cnt_armed) {
        HIP_TRY(hipMemsetAsync(h->list_cnt.p, 0, (size_t)kc * 4, h->stream));
        HIP_TRY(hipMemsetAsync(h->misc.p, 0, MISC_BYTES, h->stream));
        h->list_cnt_armed = true;
    }
    return IVFADC_OK;
}

// The exact VALU distances of nb queries to n centres (the centroids, or the two-level search's group centres), out[nb][n].  Small
// batches: narrower query tiles multiply the workgroup count until every SIMD has its four waves.  sgpr: small problems (every
// workgroup resident at once) may take the centre-per-lane kernel, queries in SGPRs -- no LDS traffic to speak of, the wave's
// instruction stream is the VALU minimum (SIFT1M-shape, 1024 queries: 14.9 -> see DESIGN 4.1)
void launch_coarse_exact(ivfadc_index *h, const float *d_q, int64_t nb, const float *centres, int n, float *out, bool sgpr)
{
    const int64_t wg64 = (int64_t)((n + CO_T - 1) / CO_T) * ((nb + 63) / 64);
    const int tq = wg64 >= 4 * (int64_t)h->num_cu ? 64 : (2 * wg64 >= 4 * (int64_t)h->num_cu ? 32 : 16);
    const dim3 grid((n + CO_T - 1) / CO_T, (unsigned)((nb + tq - 1) / tq));
    if (sgpr && (h->d & 7) == 0 && (nb + 15) / 16 <= 65535 && tq < 64)
        hipLaunchKernelGGL(coarse_sgpr_kernel<4>, dim3((n + 63) / 64, (unsigned)((nb + 15) / 16)), dim3(256), 0, h->stream, d_q, centres, out,
                           (int)nb, n, h->d);
    else
        hipLaunchKernelGGL((tq == 16 ? coarse_dist_kernel<16> : tq == 32 ? coarse_dist_kernel<32> : coarse_dist_kernel<64>), grid, dim3(256), 0,
                           h->stream, d_q, centres, out, (int)nb, n, h->d, h->d);
}

// want_tmin: also write the per-tile minimum scores (stand-alone top-w with one wave per query reads them)
// want_listed: the only reader is the stand-alone top-w with one wave per query (select_listed): when the split-bf16 kernel
// runs, it writes the four smallest keys of every (query, 64-centroid tile) and NO score matrix (Deep1B shape: 0.16 GB
// instead of 2.7 GB per batch); otherwise ignored
int run_coarse(ivfadc_index *h, const float *d_q, int64_t nb, bool mfma, bool want_tmin = false, bool want_listed = false, int w = 0)
{
    h->tmin_tiles = 0;
    h->last_listed = false;
    const bool big128 = (int64_t)((h->kc + 127) / 128) * ((nb + 127) / 128) >= 2 * (int64_t)h->num_cu;
    // (records pay when the bound -- the w-th smallest of the tile minima -- cuts most tiles: at least 4 w tiles of 64 centroids;
    // with fewer, every tile qualifies and select_listed would fall back to the exact recompute for every query)
    const bool listed = mfma && want_tmin && want_listed && h->allow_listed && big128 && h->allow_bf16 && (h->kc + 63) / 64 >= 4 * std::max(1, w);
    if (!listed) TRY(h->cdist.ensure((size_t)nb * h->kc * 4));
    ivfadc_index::EvPair ep;
    if (h->profiling) TRY(ev_begin(h, 1, ep));
    if (mfma) {
        // scores ||c||^2 - 2 q.c (coarse_mfma_kernel); 64-wide tiles when 128-wide ones would leave CUs idle
        const int64_t wg128 = (int64_t)((h->kc + 127) / 128) * ((nb + 127) / 128);
        const bool big = wg128 >= 2 * (int64_t)h->num_cu;
        const int tb = big ? 128 : 64, tile_w = tb / 2;
        const int ntiles = (h->kc + tile_w - 1) / tile_w;
        float *tmin = nullptr;
        if (want_tmin) {
            TRY(h->tmin.ensure((size_t)nb * ntiles * 4));
            tmin = h->tmin.as<float>();
            h->tmin_tiles = ntiles;
            h->tmin_tile_w = tile_w;
        }
        dim3 grid((h->kc + tb - 1) / tb, (unsigned)((nb + tb - 1) / tb));
        // small problems (every workgroup resident at once): 64-deep chunks, so a workgroup's chain is 2-3 trips to memory
        const bool deep = !big && (int64_t)grid.x * grid.y <= 4 * (int64_t)h->num_cu && h->d >= 64;
        // (small problems stay on the f32 kernels: at kc = 1024 x 1024 queries a 64 x 64-tile bf16 variant plus the split pass took 13.9 us
        // against 15.3 us for the exact VALU kernel -- launch-bound either way -- and the refine costs the scan prologue 4 us)
        h->last_coarse_bf16 = big && h->allow_bf16;
        h->last_coarse_f16 = h->last_coarse_bf16 && h->allow_f16 && h->f16_scale > 0.f && h->cent_f16.p != nullptr;
        uint4 *tl = nullptr;
        if (listed) {   // (implies the f16 or the split-bf16 kernel below)
            TRY(h->tlist.ensure((size_t)ntiles * nb * 16));
            tl = h->tlist.as<uint4>();
            h->last_listed = true;
            h->tlist_ldq = (int)nb;
        }
        if (h->last_coarse_f16) {
            // one f16 product per score (kernels.hip.h, "round 5"): scaled f16 queries + overflow flags, then the same tile kernel
            const int dp = h->dp32;
            TRY(h->q_f16.ensure((size_t)nb * dp * 2));
            TRY(h->q_flags.ensure((size_t)nb * 4));
            HIP_TRY(hipMemsetAsync(h->q_flags.p, 0, (size_t)nb * 4, h->stream));
            hipLaunchKernelGGL(split_f16_kernel, dim3((unsigned)std::min<int64_t>(4096, (nb * dp + 255) / 256)), dim3(256), 0, h->stream, d_q,
                               (int64_t)nb, h->d, dp, h->f16_scale, h->q_f16.as<unsigned short>(), h->q_flags.as<u32>());
            HIP_TRY(hipGetLastError());
            const float neg2 = -2.0f / (h->f16_scale * h->f16_scale);
            hipLaunchKernelGGL((coarse_bf16_kernel<128, true>), grid, dim3(256), 0, h->stream, h->q_f16.as<unsigned short>(),
                               (const unsigned short *)nullptr, h->cent_f16.as<unsigned short>(), (const unsigned short *)nullptr,
                               h->cnorm.as<float>(), listed ? (float *)nullptr : h->cdist.as<float>(), (int)nb, h->kc, dp, tmin, ntiles, tl,
                               (int)nb, neg2);
        } else if (h->last_coarse_bf16) {
            // split-bf16 filter: 3 bf16 MFMAs per product instead of one f32 MFMA at a sixteenth of the rate
            const int dp = h->dp32;
            TRY(h->q_hi.ensure((size_t)nb * dp * 2));
            TRY(h->q_lo.ensure((size_t)nb * dp * 2));
            hipLaunchKernelGGL(split_bf16_kernel, dim3((unsigned)std::min<int64_t>(4096, (nb * dp + 255) / 256)), dim3(256), 0, h->stream, d_q,
                               (int64_t)nb, h->d, dp, h->q_hi.as<unsigned short>(), h->q_lo.as<unsigned short>());
            HIP_TRY(hipGetLastError());
            hipLaunchKernelGGL(coarse_bf16_kernel<128>, grid, dim3(256), 0, h->stream, h->q_hi.as<unsigned short>(),
                               h->q_lo.as<unsigned short>(), h->cent_hi.as<unsigned short>(), h->cent_lo.as<unsigned short>(),
                               h->cnorm.as<float>(), listed ? (float *)nullptr : h->cdist.as<float>(), (int)nb, h->kc, dp, tmin, ntiles, tl,
                               (int)nb, -2.0f);
        } else if (big)
            hipLaunchKernelGGL((coarse_mfma_kernel<128, 16>), grid, dim3(256), 0, h->stream, d_q, h->centroids.as<float>(),
                               h->cnorm.as<float>(), h->cdist.as<float>(), (int)nb, h->kc, h->d, tmin, ntiles);
        else if (deep)
            hipLaunchKernelGGL((coarse_mfma_kernel<64, 64>), grid, dim3(256), 0, h->stream, d_q, h->centroids.as<float>(),
                               h->cnorm.as<float>(), h->cdist.as<float>(), (int)nb, h->kc, h->d, tmin, ntiles);
        else
            hipLaunchKernelGGL((coarse_mfma_kernel<64, 16>), grid, dim3(256), 0, h->stream, d_q, h->centroids.as<float>(),
                               h->cnorm.as<float>(), h->cdist.as<float>(), (int)nb, h->kc, h->d, tmin, ntiles);
    } else
        launch_coarse_exact(h, d_q, nb, h->centroids.as<float>(), h->kc, h->cdist.as<float>(), true);
    HIP_TRY(hipGetLastError());
    if (h->profiling) TRY(ev_end(h, ep));
    return IVFADC_OK;
}

RefineArgs refine_args(const ivfadc_index *h, const float *d_q)
{
    RefineArgs r;
    r.queries = d_q;
    r.centroids = h->centroids.as<float>();
    r.d = h->d;
    r.kc = h->kc;
    r.cmaxn = h->cmaxn;
    const float u = 5.9604645e-8f;   // 2^-24
    // score error / (||c|| + ||q||)^2.  f32 MFMA: rounded norms + the fma chain on q.c (refine_probes).  Split bf16: the
    // representation x = hi + lo + O(2^-18 |x|) costs (2 * 2^-18 + 2^-18 (dropped lo.lo)) |q||c| <= 0.76 * 2^-18 (||c|| + ||q||)^2
    // on q.c, doubled in the score: 1.51 * 2^-18 = 96.6 u; the f32 accumulation of 3 d products (+ padding) another
    // 0.51 (3 d + 40) u; norms and final roundings (d + 8) u as before.
    // One f16 product (kernels.hip.h, "round 5"): x^ = fl16(s x) / s, |x^ - x| <= 2^-11 |x| + 2^-25 / s, so q^ . c^ misses q . c by at most
    // (2^-10 + 2^-22) |q||c| <= 0.25 (2^-10 + 2^-22)(||c|| + ||q||)^2, doubled in the score: 8192 (1 + 2^-12) u; the subnormal term stays
    // below 2^-36 sqrt(d) of the same square (2 u with room to spare); f32 accumulation of d products and the norms as before.
    r.eps_coef = h->last_coarse_f16 ? 2.0f * (8194.0f + 2.0f + 0.51f * (float)(h->d + 40) + (float)(h->d + 8)) * u
               : h->last_coarse_bf16 ? 2.0f * (97.0f + 0.51f * (float)(3 * h->d + 40) + (float)(h->d + 8)) * u
                                     : 2.0f * (float)(h->d + 3) * u;
    r.qflags = h->last_coarse_f16 ? h->q_flags.as<u32>() : (const u32 *)nullptr;
    // listed mode: a key carries the score with its low 6 bits replaced (< 64 ulp = 2^-17 |score|, |score| <= (||c|| + ||q||)^2)
    if (h->last_listed) r.eps_coef += 128.0f * u;
    r.tlist = h->last_listed ? h->tlist.as<uint4>() : (const uint4 *)nullptr;
    r.ldq = h->tlist_ldq;
    r.gam = 4.0f * (float)(h->d + 2) * u;
    r.fallbacks = (u64 *)((char *)h->misc.p + 4096 + 64);
    r.tmin = h->tmin_tiles > 0 ? h->tmin.as<float>() : (const float *)nullptr;
    r.ntiles = h->tmin_tiles;
    r.tile_w = h->tmin_tile_w;
    return r;
}

IndexView index_view(const ivfadc_index *h)
{
    IndexView ix;
    ix.centroids = h->centroids.as<float>();
    ix.codebooks = h->codebooks.as<float>();
    ix.codebooks_t = h->codebooks_t.as<float>();
    ix.codebooks_p = h->codebooks_p.as<float>();
    ix.labels = h->labels.as<uint8_t>();
    ix.codes = h->codes.as<uint8_t>();
    ix.list_pos = h->list_pos.as<int64_t>();
    ix.list_len = h->list_len.as<u32>();
    ix.list_codeoff = h->list_codeoff.as<int64_t>();
    ix.ids = h->synthetic ? (const u32 *)nullptr : h->ids.as<u32>();
    ix.d = h->d; ix.kc = h->kc; ix.m = h->m; ix.ksub = h->ksub; ix.dsub = h->dsub; ix.cs = h->cs;
    ix.identity_labels = h->labmap.identity ? 1 : 0;
    return ix;
}

// hipFuncAttributeMaxDynamicSharedMemorySize is a property of (function, device), not of a handle: one process-wide table
// per device records the largest size ever requested for a function and only ever RAISES the attribute, so two live
// handles that share a kernel instantiation with different LDS sizes (another K, another m through the <0, 0> kernels)
// cannot leave each other with an attribute below their launch size.  Occupancy is cached per (function, size).
struct FnAttr { int device; const void *fn; size_t max_lds; bool checked; };
std::mutex g_fn_mu;
std::vector<FnAttr> g_fn_attr;

int fn_raise_lds(int device, const void *fn, size_t lds, bool need_no_static)
{
    std::lock_guard<std::mutex> lk(g_fn_mu);
    FnAttr *e = nullptr;
    for (auto &c : g_fn_attr)
        if (c.device == device && c.fn == fn) e = &c;
    if (!e) {
        g_fn_attr.push_back({device, fn, 0, false});
        e = &g_fn_attr.back();
    }
    if (need_no_static && !e->checked) {
        // the scan kernels address their tables by absolute LDS offsets (lds_load_abs): the dynamic segment must start at 0
        hipFuncAttributes fa;
        HIP_TRY(hipFuncGetAttributes(&fa, fn));
        if (fa.sharedSizeBytes != 0) return fail(IVFADC_ERR_STATE, "scan kernel carries %zu B of static LDS", (size_t)fa.sharedSizeBytes);
        e->checked = true;
    }
    if (lds > e->max_lds) {
        HIP_TRY(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        e->max_lds = lds;
    }
    return IVFADC_OK;
}

int fn_occupancy(ivfadc_index *h, const void *fn, size_t lds, int &occ, bool abs_lds = true, int threads = 256)
{
    TRY(fn_raise_lds(h->device, fn, lds, abs_lds));
    occ = 0;
    for (auto &c : h->fn_cfg)
        if (c.fn == fn && c.lds == lds) occ = c.occ;
    if (occ == 0) {
        HIP_TRY(hipOccupancyMaxActiveBlocksPerMultiprocessor(&occ, fn, threads, lds));
        occ = std::max(1, std::min(occ, 8));
        h->fn_cfg.push_back({fn, lds, occ});
    }
    return IVFADC_OK;
}

// coarse stage by the certified two-level search: distances to the G group centres (the exact tile kernel), then one wave per query
int run_twolevel(ivfadc_index *h, const float *d_q, int64_t nb, int w, int *d_probe_list, float *d_probe_dc, u32 *d_probe_base, u32 *d_list_cnt,
                 u64 *d_scanned)
{
    const int G = h->tl_G;
    TRY(h->tl_gdist.ensure((size_t)nb * G * 4));
    ivfadc_index::EvPair ep;
    if (h->profiling) TRY(ev_begin(h, 1, ep));
    launch_coarse_exact(h, d_q, nb, h->tl_centres.as<float>(), G, h->tl_gdist.as<float>(), false);
    HIP_TRY(hipGetLastError());
    TwoLevelView tv;
    tv.gdist = h->tl_gdist.as<float>();
    tv.g_off = h->tl_off.as<u32>();
    tv.g_rad = h->tl_rad.as<float>();
    tv.cent_g = h->tl_cent.as<float>();
    tv.slot_id = h->tl_slot.as<u32>();
    tv.G = G;
    tv.d = h->d;
    tv.eps = h->tl_eps;
    const size_t lds = (size_t)4 * h->d * 4 + 4 * 64 * 8;
    if (lds > (size_t)(48 << 10)) TRY(fn_raise_lds(h->device, (const void *)twolevel_topw_kernel, lds, false));
    hipLaunchKernelGGL(twolevel_topw_kernel, dim3((unsigned)((nb + 3) / 4)), dim3(256), lds, h->stream, d_q, tv, (int)nb, w, h->list_len.as<u32>(),
                       d_probe_list, d_probe_dc, d_probe_base, d_list_cnt, d_scanned, h->part_n, h->part_i);
    HIP_TRY(hipGetLastError());
    if (h->profiling) TRY(ev_end(h, ep));
    return IVFADC_OK;
}

// The stand-alone top-w selection over the n coarse rows in h->cdist (or the records run_coarse left instead): lists, distances and
// visit-order bases of the w probes per query.  mfma: the rows are matrix-core scores (implies w <= 48: register selectors);
// wpq4: a workgroup per query instead of a wave; lc: the probe histogram, where a grouped list-major scan follows
int launch_topw(ivfadc_index *h, const float *d_q, int64_t n, int w, int capw, bool mfma, bool wpq4, int *out_list, float *out_dc, u32 *out_base,
                u32 *lc, u64 *counters, int part_n, int part_i)
{
    const size_t lds = (size_t)4 * capw * 8;
    void (*fn)(const float *, int, int, int, int, const u32 *, int *, float *, u32 *, u32 *, u64 *, const RefineArgs, int, int);
    if (mfma)
        fn = wpq4 ? topw_select_kernel<true, 4, true> : topw_select_kernel<true, 1, true>;
    else if (w <= 64)
        fn = wpq4 ? topw_select_kernel<true, 4, false> : topw_select_kernel<true, 1, false>;
    else
        fn = wpq4 ? topw_select_kernel<false, 4, false> : topw_select_kernel<false, 1, false>;
    const unsigned grid = wpq4 ? (unsigned)n : (unsigned)((n + 3) / 4);
    if (lds > (size_t)(32 << 10)) { int occ_unused = 0; TRY(fn_occupancy(h, (const void *)fn, lds, occ_unused, false)); }
    hipLaunchKernelGGL(fn, dim3(grid), dim3(256), lds, h->stream, h->cdist.as<float>(), (int)n, h->kc, w, capw, h->list_len.as<u32>(), out_list,
                       out_dc, out_base, lc, counters, refine_args(h, d_q), part_n, part_i);
    HIP_TRY(hipGetLastError());
    return IVFADC_OK;
}

LbView lb_view(const ivfadc_index *h)
{
    LbView v;
    v.cb_split = h->lb_split.as<uint4>();
    v.cb_n2 = h->lb_n2.as<float>();
    v.cb_lab = h->lb_lab.as<float>();
    v.cb_maxn = h->lb_maxn.as<float>();
    v.cb_f16 = (h->lb_use_f16 && h->lb_f16.p) ? h->lb_f16.as<uint4>() : (const uint4 *)nullptr;
    v.cb_isc = h->lb_isc.as<float>();
    v.mu = v.cb_f16 ? 1.48e-3f : 9.2e-5f;
    return v;
}

// The probes of a sub-batch into probe_list / probe_dc / probe_base: the caller's (pre_list: index.jl:220-257 given the output of any
// coarse_search -- the coarse stage and the top-w selection are one ingest launch), the two-level search's, or the coarse rows -- computed
// here, or standing already (written by the previous search's launch behind a hint: ivfadc_set_next_queries) -- and, unless the scan
// fuses it, the stand-alone top-w.  lc: the probe histogram (grouped list-major only)
int probe_stage(ivfadc_index *h, const Plan &pl, const SearchCall &c, u32 *lc)
{
    const bool pre = c.pre();
    const int64_t nb = c.nq; const float *d_q = c.q; const int w = c.w;
    u64 *d_scanned = h->misc.as<u64>();          // 64 sharded counters
    // one wave per query leaves the chip empty on small batches: the stand-alone top-w uses a workgroup per query there
    const bool wpq4 = !pl.lanes && nb * 1 < (int64_t)8 * h->num_cu * 4 && h->kc >= 512 && !(pl.form == ScanForm::QueryMajorLb && !pl.fuse_topw);
    // (a masked search takes no prefetched rows: its sub-batches never counted as the whole batch)
    const bool have_rows = c.whole_batch && !pre && !c.masked() && !pl.coarse_mfma && !pl.twolevel && h->avail_q == d_q && h->avail_nq == nb && h->cdist2.p != nullptr;
    h->avail_q = nullptr;
    if (pre || pl.twolevel || have_rows) {
        h->tmin_tiles = 0;
        h->last_listed = false;
    }
    if (pre) {
        hipLaunchKernelGGL(probe_ingest_kernel, dim3((unsigned)((nb + 3) / 4)), dim3(256), 0, h->stream, c.pre_list, c.pre_dc, (int)nb, h->kc, w,
                           h->list_len.as<u32>(), h->probe_list.as<int>(), h->probe_dc.as<float>(), h->probe_base.as<u32>(), lc, (u32 *)nullptr,
                           d_scanned);
        HIP_TRY(hipGetLastError());
    } else if (pl.twolevel) {
        TRY(run_twolevel(h, d_q, nb, w, h->probe_list.as<int>(), h->probe_dc.as<float>(), h->probe_base.as<u32>(), lc, d_scanned));
    } else if (have_rows) {
        std::swap(h->cdist, h->cdist2);
    } else {
        TRY(run_coarse(h, d_q, nb, pl.coarse_mfma, pl.coarse_mfma && (pl.fuse_topw ? h->m > 16 : !wpq4),   // who reads them
                       !pl.fuse_topw && !wpq4, w));
    }
    if (!pl.fuse_topw && !pl.twolevel && !pre)
        TRY(launch_topw(h, d_q, nb, w, pl.capw, pl.coarse_mfma, wpq4, h->probe_list.as<int>(), h->probe_dc.as<float>(), h->probe_base.as<u32>(), lc,
                        d_scanned, h->part_n, h->part_i));
    h->stats.last_rider = 0;
    h->stats.coarse_prefetched = have_rows ? 1 : 0;
    h->stats.last_twolevel = pl.twolevel ? 1 : 0;
    h->stats.coarse_mfma = pl.coarse_mfma ? 1 : 0;
    h->stats.coarse_f16 = (pl.coarse_mfma && h->last_coarse_f16 && !have_rows) ? 1 : 0;
    h->stats.coarse_listed = h->last_listed ? 1 : 0;
    return IVFADC_OK;
}

// query-major scan: a workgroup per query
int scan_query_major(ivfadc_index *h, const Plan &pl, const SearchCall &c)
{
    const int kc = h->kc, K = c.K, w = c.w;
    const int64_t nb = c.nq; const float *d_q = c.q; const bool pre = c.pre();
    const bool lb = pl.form == ScanForm::QueryMajorLb;
    QScanArgs a;
    a.ix = index_view(h);
    a.queries = d_q;
    a.nq = (int)nb; a.w = w; a.K = K; a.cap = pl.cap;
    a.probe_list = h->probe_list.as<int>(); a.probe_dc = h->probe_dc.as<float>(); a.probe_base = h->probe_base.as<u32>();
    a.out_ids = c.ids; a.out_dists = c.dists; a.out_counts = c.counts;
    a.cdist = pl.fuse_topw ? h->cdist.as<float>() : (const float *)nullptr;
    a.scanned_points = h->misc.as<u64>();
    a.approx = pl.coarse_mfma ? 1 : 0;
    a.rf = refine_args(h, d_q);
    a.prune = h->allow_prune ? (pre ? 2 : 1) : 0;   // 2: ranks in the caller's order -- a list above the bound is skipped, the query goes on
    a.lb = lb_view(h);
    int occ = 0;
    TRY(fn_occupancy(h, pl.fn, pl.lds, occ));
    ivfadc_index::EvPair ep;
    // riders: the hinted batch will take the exact small-problem coarse kernel whatever its K and w (no matrix-core filter at this kc)
    const bool ride = c.whole_batch && !pre && !h->tl_use && h->hint_q != nullptr && h->hint_nq > 0 && !lb && pl.small_k && (h->d & 7) == 0 &&
                      (!h->allow_mfma || kc < h->mfma_min_kc) && (h->hint_nq + 4 * RIDER_QW - 1) / (4 * RIDER_QW) <= 65535 &&
                      (size_t)h->hint_nq * kc * 4 <= h->ws_budget / 4;
    // a hinted next batch (ivfadc_set_next_queries): its exact coarse tiles ride behind this batch's scan in the same grid
    qscan_coarse_fn_t fk = ride ? pick_qscan_coarse(h->m, h->dsub, pl.qg) : nullptr;
    if (fk) {
        TRY(h->cdist2.ensure((size_t)h->hint_nq * kc * 4));
        CoarseNext cn;
        cn.queries = h->hint_q; cn.out = h->cdist2.as<float>(); cn.nq = (int)h->hint_nq; cn.ncx = (kc + 63) / 64;
        const size_t lds = std::max<size_t>(pl.lds, (size_t)64 * 132 * 4);
        TRY(fn_raise_lds(h->device, (const void *)fk, lds, true));
        const unsigned grid = (unsigned)(nb + (int64_t)cn.ncx * ((h->hint_nq + 4 * RIDER_QW - 1) / (4 * RIDER_QW)));
        if (h->hint_ev) {   // the hinted rows' ingest (ivfadc_search_batches): in front of the one launch that reads them
            HIP_TRY(hipStreamWaitEvent(h->stream, h->hint_ev, 0));
            h->hint_ev = nullptr;
        }
        if (h->profiling) TRY(ev_begin(h, 0, ep));
        hipLaunchKernelGGL(fk, dim3(grid), dim3(256), lds, h->stream, a, cn);
        HIP_TRY(hipGetLastError());
        if (h->profiling) TRY(ev_end(h, ep));
        h->pf_q = h->hint_q;
        h->pf_nq = h->hint_nq;
        h->pf_token = h->hint_token;
        h->stats.last_rider = 1;
    } else {
        if (h->profiling) TRY(ev_begin(h, 0, ep));
        hipLaunchKernelGGL((qscan_fn_t)pl.fn, dim3((unsigned)nb), dim3(pl.threads), pl.lds, h->stream, a);
        HIP_TRY(hipGetLastError());
        if (h->profiling) TRY(ev_end(h, ep));
    }
    h->stats.last_scan_grid = (int)nb;
    if (!lb) TRY(fb_snapshot(h));
    if (h->profiling_level >= 2 && lb && !pl.fuse_topw && pl.qg == 4) {
        // the table build alone, over the probes this batch used (measurement only)
        void (*bk)(const IndexView, const LbView, const float *, const int *, int, u32 *) =
            (h->m == 48) ? lb_build_only_kernel<48, 16, 4> : lb_build_only_kernel<16, 6, 4>;
        TRY(fn_raise_lds(h->device, (const void *)bk, pl.lds, false));
        TRY(h->dbg.ensure((size_t)nb * 4));
        ivfadc_index::EvPair eb;
        TRY(ev_begin(h, 2, eb));
        hipLaunchKernelGGL(bk, dim3((unsigned)nb), dim3(256), pl.lds, h->stream, a.ix, a.lb, d_q, h->probe_list.as<int>(), w,
                           h->dbg.as<u32>());
        HIP_TRY(hipGetLastError());
        TRY(ev_end(h, eb));
    }
    return IVFADC_OK;
}

// One list-major scan launch, whichever the kernel: a persistent grid of as many workgroups as fit the chip, at most one per work item
// (upper), between the profiling events of the scan; fn is pl.fn under its own type, extra what it takes behind the ScanArgs
template <class... P, class... X>
int launch_list_scan(ivfadc_index *h, const Plan &pl, size_t upper, void (*fn)(const ScanArgs, P...), const ScanArgs &a, X... extra)
{
    int occ = 0;
    TRY(fn_occupancy(h, pl.fn, pl.lds, occ, true, pl.threads));   // (occupancy is clamped to 8 workgroups per CU)
    const unsigned grid = (unsigned)std::max<size_t>(1, std::min<size_t>(upper, (size_t)h->num_cu * occ));
    ivfadc_index::EvPair ep;
    if (h->profiling) TRY(ev_begin(h, 0, ep));
    hipLaunchKernelGGL(fn, dim3(grid), dim3(pl.threads), pl.lds, h->stream, a, extra...);
    HIP_TRY(hipGetLastError());
    if (h->profiling) TRY(ev_end(h, ep));
    h->stats.last_scan_grid = (int)grid;
    return IVFADC_OK;
}

// list-major scan: work items from the probe histogram (direct: one per (query, probe, chunk), nothing to group), the form's kernel,
// and the merge of the partial results
int scan_list_major(ivfadc_index *h, const Plan &pl, const SearchCall &c, bool direct)
{
    const int kc = h->kc, K = c.K, w = c.w;
    const int64_t nb = c.nq;
    const size_t np = (size_t)nb * w;
    const bool w8 = pl.form == ScanForm::EightWave;
    u32 *d_qhead = (u32 *)((char *)h->misc.p + 4096);
    TRY(h->bucket_items.ensure(np * 4));
    TRY(h->part_keys.ensure(np * pl.maxch * K * 8));
    TRY(h->part_cnt.ensure(np * pl.maxch * 4));
    {
        const size_t before = h->qthr.bytes;
        TRY(h->qthr.ensure((size_t)nb * 8));
        if (h->qthr.bytes != before) h->qthr_armed = 0;
        if (h->qthr_armed < (size_t)nb) {
            const size_t cnt = h->qthr.bytes / 8;
            hipLaunchKernelGGL(fill_u64_kernel, dim3(256), dim3(256), 0, h->stream, h->qthr.as<u64>(), cnt, (u64)KEY_MAX);
            HIP_TRY(hipGetLastError());
            h->qthr_armed = cnt;
        }
    }
    if (!direct) {
        u32 *item_list = nullptr;
        if (w8) {
            TRY(h->wg8_items.ensure(np * (size_t)pl.maxch * 4));
            item_list = h->wg8_items.as<u32>();
        }
        hipLaunchKernelGGL(bucket_scan_kernel, dim3(1), dim3(1024), 0, h->stream, h->list_cnt.as<u32>(), h->list_len.as<u32>(),
                           kc, pl.qg, pl.CH, h->bucket_off.as<u32>(), h->wi_off.as<u32>(), h->cursor.as<u32>(), d_qhead, item_list);
        HIP_TRY(hipGetLastError());
        hipLaunchKernelGGL(bucket_scatter_kernel, dim3((unsigned)((np + 255) / 256)), dim3(256), 0, h->stream,
                           h->probe_list.as<int>(), (int)np, h->bucket_off.as<u32>(), h->cursor.as<u32>(), h->bucket_items.as<u32>(),
                           h->part_n, h->part_i);
        HIP_TRY(hipGetLastError());
    }

    ScanArgs a;
    a.ix = index_view(h);
    a.queries = c.q;
    a.w = w; a.K = K; a.cap = pl.cap;
    a.probe_dc = h->probe_dc.as<float>(); a.probe_base = h->probe_base.as<u32>(); a.list_cnt = h->list_cnt.as<u32>();
    a.bucket_off = h->bucket_off.as<u32>(); a.wi_off = h->wi_off.as<u32>(); a.bucket_items = h->bucket_items.as<u32>();
    a.queue_head = d_qhead;
    a.qthr = h->qthr.as<u64>();
    a.part_keys = h->part_keys.as<u64>(); a.part_cnt = h->part_cnt.as<u32>(); a.maxch = pl.maxch; a.CH = pl.CH;
    a.probe_list = h->probe_list.as<int>();
    a.direct_items = direct ? (u32)(np * (size_t)pl.maxch) : 0u;
    a.prune = h->allow_prune ? 1 : 0;
    a.scanned_points = h->misc.as<u64>();

    const size_t upper = np * (size_t)pl.maxch;
    if (w8) {
        u32 *xq = nullptr;
        TRY(clear_xcd_heads(h, xq));
        // (the larger form of the handle's m: eight queries)
        TRY(h->wg8_tabs.ensure((size_t)h->num_cu * 8 * (h->m == 16 ? W8_GTAB_FLOATS<8, 16> : W8_GTAB_FLOATS<8>) * 4));
        TRY(launch_list_scan(h, pl, upper, (wg8_fn_t)pl.fn, a, h->wg8_tabs.as<float>(), h->wg8_items.as<u32>(), xq, 8));
    } else if (pl.form == ScanForm::NarrowField) {
        NfView nv;
        nv.n2 = h->nf_n2.as<float>();
        nv.cb_lab = h->nf_lab.as<float>();
        nv.maxn2 = h->nf_n2.as<float>() + (size_t)h->m * 256;
        nv.nranges = 8;
        TRY(clear_xcd_heads(h, nv.xq));
        TRY(launch_list_scan(h, pl, upper, (nf_fn_t)pl.fn, a, nv));
    } else if (pl.form == ScanForm::FourWave) {
        TRY(launch_list_scan(h, pl, upper, (scan_fn_t)pl.fn, a));
    } else if (pl.form == ScanForm::Masked) {
        if (!c.masked()) return fail(IVFADC_ERR_STATE, "masked scan planned without a mask set");
        TRY(launch_list_scan(h, pl, upper, (masked_fn_t)pl.fn, a, mask_view(c)));
    } else {
        TRY(launch_list_scan(h, pl, upper, (u16_fn_t)pl.fn, a, pl.qg));
    }

    const size_t mlds = pl.small_k ? 0 : (size_t)4 * pl.cap * 8;
    auto mk = pl.small_k ? merge_kernel<true> : merge_kernel<false>;
    if (mlds > (size_t)(32 << 10)) { int occ_unused = 0; TRY(fn_occupancy(h, (const void *)mk, mlds, occ_unused, false)); }
    hipLaunchKernelGGL(mk, dim3((unsigned)((nb + 3) / 4)), dim3(256), mlds, h->stream, (int)nb, w, K, pl.cap, pl.maxch, pl.CH, kc,
                       h->probe_list.as<int>(), h->probe_base.as<u32>(), h->list_pos.as<int64_t>(), h->list_len.as<u32>(),
                       h->synthetic ? (const u32 *)nullptr : h->ids.as<u32>(), h->part_keys.as<u64>(), h->part_cnt.as<u32>(), c.ids, c.dists,
                       c.counts, h->qthr.as<u64>(), h->list_cnt.as<u32>(), d_qhead, h->part_n, h->part_i, (u64 *)h->partial_keys);
    HIP_TRY(hipGetLastError());
    return IVFADC_OK;
}

// c: one sub-batch of the plan (c.whole_batch: the call's whole batch, to which hints and prefetched rows apply)
int search_subbatch(ivfadc_index *h, const Plan &pl, const SearchCall &c)
{
    const bool qm = pl.query_major();
    const int64_t nb = c.nq;
    const size_t np = (size_t)nb * c.w;
    TRY(ensure_common_ws(h));
    TRY(h->probe_list.ensure(np * 4));
    TRY(h->probe_dc.ensure(np * 4));
    TRY(h->probe_base.ensure(np * 4));
    // list-major with one query per code stream: every (query, probe) pair is a work item of its own, nothing to group
    // by list -- no probe histogram, no bucket kernels
    const bool direct = !qm && pl.qg == 1 && np * (size_t)pl.maxch < ((size_t)1 << 31) && h->part_n <= 1;
    TRY(probe_stage(h, pl, c, (qm || direct) ? (u32 *)nullptr : h->list_cnt.as<u32>()));
    // what the plan runs (last_lb: of the latest query-major scan; last_striped, last_nf: of the latest list-major one)
    h->stats.last_qg = qm ? 0 : pl.qg;
    h->stats.last_chunk = (int)pl.CH;
    h->stats.last_scan_lds = (int)pl.lds;
    if (qm) {
        h->stats.last_lb = pl.form == ScanForm::QueryMajorLb ? 1 : 0;
        TRY(scan_query_major(h, pl, c));
    } else {
        h->stats.last_striped = pl.striped();
        h->stats.last_nf = pl.form == ScanForm::NarrowField ? 1 : 0;
        TRY(scan_list_major(h, pl, c, direct));
    }
    h->stats.queries += nb;
    if (h->profiling && h->pending.size() > 2048) TRY(ev_fold(h));
    return IVFADC_OK;
}

// mutators: not on a view; every other holder of the device arrays learns that they changed
int check_mutable(ivfadc_index *h, const char *what)
{
    if (h->is_view) return fail(IVFADC_ERR_STATE, "%s: this handle is a read-only view (ivfadc_clone_view / ivfadc_clone_subset)", what);
    return IVFADC_OK;
}

// A mutator's critical section.  begin() is called once the arguments have been validated and the call is known to change something (a
// failing or no-op call leaves the views, and the internal second lane of ivfadc_search_batches, valid): from there until the scope ends
// the topology mutex and every view's mutex are held -- no view call is running or can start -- the views' streams have drained, and
// the generation has moved on, so the first view search afterwards refuses.
struct MutationScope {
    ivfadc_index *h = nullptr;
    std::vector<ivfadc_index *> held;
    bool topo = false;
    int begin(ivfadc_index *x, const char *what)
    {
        TRY(check_mutable(x, what));
        if (h) return IVFADC_OK;   // (once per call)
        h = x;
        g_topo_mu.lock();
        topo = true;
        for (ivfadc_index *v : h->views) { v->mu.lock(); held.push_back(v); }
        h->generation++;
        // searches still in flight on views read the arrays that are about to change: they finish first
        if (!h->views.empty()) TRY(set_device(h));
        for (ivfadc_index *v : h->views)
            if (v->stream) HIP_TRY(hipStreamSynchronize(v->stream));
        return IVFADC_OK;
    }
    ~MutationScope()
    {
        for (ivfadc_index *v : held) v->mu.unlock();
        if (topo) g_topo_mu.unlock();
    }
};

// Called with the view's own mutex held (every entry point's HandleLock), and with that alone: whoever changes what is read here -- a
// mutator bumping the generation (MutationScope), the index's destructor cutting the link -- holds this view's mutex while doing so, so
// the topology mutex is NOT taken (taking it here, behind the view's own mutex, would invert the order a mutator takes the two in).
int check_view_current(ivfadc_index *h)
{
    if (!h->is_view) return IVFADC_OK;
    if (h->orphan || !h->view_of) return fail(IVFADC_ERR_STATE, "the index this view was taken from has been destroyed");
    if (h->view_of->generation != h->view_gen) return fail(IVFADC_ERR_STATE, "the index has changed since this view was taken: take a new one");
    return IVFADC_OK;
}

int check_search_args(ivfadc_index *h, int64_t nq, int K, int &w)
{
    if (!h) return fail(IVFADC_ERR_INVALID, "null handle");
    TRY(check_view_current(h));
    if (K < 1) return fail(IVFADC_ERR_ASSERT, "Number of neighbors must be k >= 1");
    if (w < 1) return fail(IVFADC_ERR_ASSERT, "Number of clusters to search in must be w >= 1");
    if (nq < 0) return fail(IVFADC_ERR_INVALID, "nq < 0");
    if (!h->have_lists && !h->dirty) return fail(IVFADC_ERR_STATE, "no inverted lists set");
    w = std::min(w, h->kc);
    if ((int64_t)nq * K > ((int64_t)1 << 40)) return fail(IVFADC_ERR_INVALID, "nq x K = %lld result slots", (long long)nq * K);
    return IVFADC_OK;
}

// ---- generic path (generic.hip.h): dump every key, sort, take the first K ------------------------------------
int gen_sort(ivfadc_index *h, const u64 *in, u64 *out, int64_t total, int segments, const u32 *d_off)
{
    if (total == 0) return IVFADC_OK;
    size_t tmp = 0;
    HIP_TRY(rocprim::segmented_radix_sort_keys(nullptr, tmp, in, out, (unsigned)total, (unsigned)segments, d_off, d_off + 1, 0, 64,
                                               h->stream));
    TRY(h->gen_tmp.ensure(std::max<size_t>(tmp, 16)));
    HIP_TRY(rocprim::segmented_radix_sort_keys(h->gen_tmp.p, tmp, in, out, (unsigned)total, (unsigned)segments, d_off, d_off + 1, 0, 64,
                                               h->stream));
    return IVFADC_OK;
}

// stage A of the generic path: coarse distances (exact VALU kernel), rows -> keys -> sorted rows -> the w probes of na queries
// (na x kc < 2^31 keys; h->gen_tot holds na words)
int gen_stage_a(ivfadc_index *h, const float *qa, int64_t na, int w, int *d_pl, float *d_pd, u32 *d_pb, u64 *d_scanned)
{
    const int kc = h->kc;
    TRY(run_coarse(h, qa, na, false));
    const int64_t rk = na * kc;
    TRY(h->gen_a.ensure((size_t)rk * 8));
    TRY(h->gen_b.ensure((size_t)rk * 8));
    hipLaunchKernelGGL(gen_row_keys_kernel, dim3((unsigned)std::min<int64_t>(8192, (rk + 255) / 256)), dim3(256), 0, h->stream,
                       h->cdist.as<float>(), rk, kc, h->gen_a.as<u64>());
    HIP_TRY(hipGetLastError());
    std::vector<u32> off((size_t)na + 1);
    for (int64_t q = 0; q <= na; ++q) off[q] = (u32)(q * kc);
    TRY(h->gen_off.ensure(((size_t)na + 1) * 4));
    TRY(h2d_copy(h->gen_off.p, off.data(), ((size_t)na + 1) * 4, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));   // `off` goes away
    TRY(gen_sort(h, h->gen_a.as<u64>(), h->gen_b.as<u64>(), rk, (int)na, h->gen_off.as<u32>()));
    hipLaunchKernelGGL(gen_probes_kernel, dim3((unsigned)na), dim3(256), 0, h->stream, h->gen_b.as<u64>(), kc, w, h->list_len.as<u32>(),
                       d_pl, d_pd, d_pb, h->gen_tot.as<u32>(), d_scanned);
    HIP_TRY(hipGetLastError());
    return IVFADC_OK;
}

// The queries of a batch in groups the segmented sort can take (range_plan::next_group; tot: keys per query).  For every group: its 32-bit
// offset row in gen_off, gen_a / gen_b sized for its keys (at least one key's worth), body(g0, ng, keys), and a synchronisation, since
// all three are reused by the next group.  skip_empty: a group without keys is passed over (range search; the generic path still emits
// its zero counts).  A batch holds at most range_plan::MAX_GRID_Y queries (the generic path's nba clamp, the range plan's nb): within
// that bound next_group's grid-y term never cuts a group that the key budget would not (tests/c/search_call_check.cpp).
template <class Body>
int for_sort_groups(ivfadc_index *h, const std::vector<uint64_t> &tot, int64_t cap_keys, bool skip_empty, const char *verb, const char *noun, Body body)
{
    const int64_t n = (int64_t)tot.size();
    if (n > range_plan::MAX_GRID_Y) return fail(IVFADC_ERR_STATE, "a sort batch of %lld queries (at most %lld)", (long long)n, (long long)range_plan::MAX_GRID_Y);
    std::vector<u32> off;
    for (int64_t g0 = 0; g0 < n;) {
        uint64_t keys = 0;
        const int64_t g1 = range_plan::next_group(tot, g0, cap_keys, &keys);
        if (g1 == g0)
            return fail(IVFADC_ERR_INVALID, "a single query %s %llu %s: too many for one sort", verb, (unsigned long long)tot[(size_t)g0], noun);
        const int64_t ng = g1 - g0;
        if (keys > 0 || !skip_empty) {
            off.resize((size_t)ng + 1);
            off[0] = 0;
            for (int64_t q = 0; q < ng; ++q) off[(size_t)q + 1] = off[(size_t)q] + (u32)tot[(size_t)(g0 + q)];
            TRY(h->gen_a.ensure((size_t)std::max<uint64_t>(1, keys) * 8));
            TRY(h->gen_b.ensure((size_t)std::max<uint64_t>(1, keys) * 8));
            TRY(h->gen_off.ensure(((size_t)ng + 1) * 4));
            TRY(h2d_copy(h->gen_off.p, off.data(), ((size_t)ng + 1) * 4, h->stream));
            TRY(body(g0, ng, (int64_t)keys));
            HIP_TRY(hipStreamSynchronize(h->stream));   // `off` and the key buffers are reused by the next group
        }
        g0 = g1;
    }
    return IVFADC_OK;
}

// the probe rows the coarse stage of the current batch left in the handle
ProbeRows probe_rows(ivfadc_index *h, int w) { return ProbeRows{h->probe_list.as<int>(), h->probe_dc.as<float>(), h->probe_base.as<u32>(), w}; }

// c.pre_list: the caller's probes (ivfadc_search_preassigned), stage A is their ingest.  A masked search: rejected points leave all-ones
// keys, which sort last and are counted out.
int search_generic(ivfadc_index *h, const SearchCall &c)
{
    const int kc = h->kc, K = c.K, w = c.w;
    const int64_t nq = c.nq;
    const size_t lds = (align_up((size_t)h->d, 4) + (h->u16 ? (size_t)GEN16_TILE : (size_t)h->m * 256)) * 4;
    if (lds > LDS_MAX) return fail(IVFADC_ERR_INVALID, "m=%d needs %zu B of LDS in the generic path (> %zu)", h->m, lds, LDS_MAX);
    void (*dump)(const IndexView, const float *, int, const int *, const float *, const u32 *, const u32 *, u64 *, const MaskView) =
        h->u16 ? gen_dump_u16_kernel : gen_dump_kernel;
    TRY(fn_raise_lds(h->device, (const void *)dump, lds, false));
    TRY(ensure_common_ws(h));
    u64 *d_scanned = h->misc.as<u64>();
    const IndexView ix = index_view(h);
    const u32 *idp = h->synthetic ? (const u32 *)nullptr : h->ids.as<u32>();
    // stage A batches: the kc-key rows of a batch are sorted in one call (< 2^32 keys, inside the workspace budget)
    const int64_t per_q = (int64_t)kc * (4 + 16) + (int64_t)w * 12 + 64;
    int64_t nba = std::max<int64_t>(1, (int64_t)(h->ws_budget / (size_t)per_q));
    nba = std::min<int64_t>(std::min<int64_t>(nba, nq), std::min<int64_t>(65535, ((int64_t)1 << 31) / std::max(1, kc)));
    // stage B groups: as many queries as fit the key budget (two key buffers + sort scratch), at least one
    const int64_t cap_keys = range_plan::sort_cap_keys(h->ws_budget);
    std::vector<u32> tot32;
    std::vector<uint64_t> tot;   // (the same, as next_group takes them)
    for (int64_t a0 = 0; a0 < nq; a0 += nba) {
        const SearchCall ca = c.slice(a0, std::min(nba, nq - a0));
        const int64_t na = ca.nq;
        const size_t np = (size_t)na * w;
        TRY(h->probe_list.ensure(np * 4));
        TRY(h->probe_dc.ensure(np * 4));
        TRY(h->probe_base.ensure(np * 4));
        TRY(h->gen_tot.ensure((size_t)na * 4));
        if (ca.pre()) {
            hipLaunchKernelGGL(probe_ingest_kernel, dim3((unsigned)((na + 3) / 4)), dim3(256), 0, h->stream, ca.pre_list, ca.pre_dc, (int)na, kc, w,
                               h->list_len.as<u32>(), h->probe_list.as<int>(), h->probe_dc.as<float>(), h->probe_base.as<u32>(), (u32 *)nullptr,
                               h->gen_tot.as<u32>(), d_scanned);
            HIP_TRY(hipGetLastError());
        } else {
            TRY(gen_stage_a(h, ca.q, na, w, h->probe_list.as<int>(), h->probe_dc.as<float>(), h->probe_base.as<u32>(), d_scanned));
        }
        tot32.resize((size_t)na);
        TRY(d2h_copy(tot32.data(), h->gen_tot.p, (size_t)na * 4, h->stream));
        HIP_TRY(hipStreamSynchronize(h->stream));
        tot.assign(tot32.begin(), tot32.end());
        TRY(for_sort_groups(h, tot, cap_keys, false, "probes", "points", [&](int64_t g0, int64_t ng, int64_t keys) -> int {
            const SearchCall cg = ca.slice(g0, ng);
            const ProbeRows pg = probe_rows(h, w).slice(g0);
            for (int64_t y0 = 0; y0 < ng; y0 += 32768) {   // grid.y limit
                const SearchCall cy = cg.slice(y0, std::min<int64_t>(32768, ng - y0));
                const ProbeRows py = pg.slice(y0);
                hipLaunchKernelGGL(dump, dim3((unsigned)w, (unsigned)cy.nq), dim3(256), lds, h->stream, ix, cy.q, w, py.list, py.dc, py.base,
                                   h->gen_off.as<u32>() + y0, h->gen_a.as<u64>(), mask_view(cy));
                HIP_TRY(hipGetLastError());
            }
            TRY(gen_sort(h, h->gen_a.as<u64>(), h->gen_b.as<u64>(), keys, (int)ng, h->gen_off.as<u32>()));
            hipLaunchKernelGGL(gen_emit_kernel, dim3((unsigned)ng), dim3(256), 0, h->stream, h->gen_b.as<u64>(), h->gen_off.as<u32>(),
                               h->gen_tot.as<u32>() + g0, w, K, pg.list, pg.base, h->list_pos.as<int64_t>(), idp, cg.ids, cg.dists, cg.counts);
            HIP_TRY(hipGetLastError());
            return IVFADC_OK;
        }));
        h->stats.queries += na;
    }
    h->stats.last_qg = -2;
    h->stats.coarse_mfma = 0;
    return IVFADC_OK;
}

// The latency path (smallq.hip.h): a handful of queries in ONE launch, (query, probe, chunk)-parallel with a last-arriver merge
// (two launches when the coarse quantizer is too large to be searched by every workgroup for itself).
// Largest coarse quantizer the small-batch launch searches inside itself.  Measured (SIFT1M shape, one query, w = 8): 32.9 us with the
// search inside -- a lane walking its own centroid rows touches 64 cache lines per load instruction -- against 24.8 us with the exact
// coarse kernel one launch earlier: the default is the separate kernel; ivfadc_set_coarse_mode(h, 5) takes the single-launch form.
int sq_inside_kc(const ivfadc_index *h)
{
    return (h->sq_inside && h->cent_t.p) ? SQ_COARSE_INSIDE : 0;
}

bool sq_eligible(const ivfadc_index *h, int64_t nq, int K, int w)
{
    static const bool off = getenv("IVFADC_NO_SMALLQ") != nullptr;
    if (off || !h->allow_sq || h->force_qg != 0 || h->u16) return false;
    if (K > 64 || w > 64 || nq > 64 || nq * w > 512) return false;
    if ((h->d & 3) != 0) return false;
    const size_t lds = sq_lds_bytes(h->m, h->d, h->kc <= sq_inside_kc(h) ? h->kc : 0);
    return lds <= LDS_MAX;
}

int search_small(ivfadc_index *h, const SearchCall &c)
{
    const int64_t nq = c.nq; const float *d_q = c.q; const int K = c.K, w = c.w;
    TRY(ensure_common_ws(h));
    const bool inside = h->kc <= sq_inside_kc(h);
    if (!inside) {
        if (h->cent_t.p && nq <= 65535) {
            // exact distances, a lane per (centroid, query): half the time of the tiled kernel for a handful of queries (smallq.hip.h)
            TRY(h->cdist.ensure((size_t)nq * h->kc * 4));
            ivfadc_index::EvPair ec;
            if (h->profiling) TRY(ev_begin(h, 1, ec));
            void (*ck)(const float4 *, const float *, float *, int, int, int) =
                h->d == 128 ? coarse_lane_kernel<32> : (h->d == 96 ? coarse_lane_kernel<24> : (h->d == 64 ? coarse_lane_kernel<16> : coarse_lane_kernel<0>));
            hipLaunchKernelGGL(ck, dim3((unsigned)((h->kc + 255) / 256), (unsigned)nq), dim3(256), 0, h->stream,
                               h->cent_t.as<float4>(), d_q, h->cdist.as<float>(), (int)nq, h->kc, h->d);
            HIP_TRY(hipGetLastError());
            if (h->profiling) TRY(ev_end(h, ec));
        } else {
            TRY(run_coarse(h, d_q, nq, false));   // exact distances (the 3-op VALU kernel): nothing to refine
        }
    }
    // chunks: about two workgroups per CU in all, a chunk no shorter than 4096 points
    const int64_t items = nq * w;
    int nch = (int)std::max<int64_t>(1, std::min<int64_t>((h->mirror.maxlen + 4095) / 4096, (2 * (int64_t)h->num_cu) / std::max<int64_t>(1, items)));
    uint32_t CH = (uint32_t)align_up((size_t)std::max<int64_t>(1, (h->mirror.maxlen + nch - 1) / nch), 1024);
    nch = (int)std::max<int64_t>(1, (h->mirror.maxlen + CH - 1) / CH);
    const size_t slots = (size_t)items * nch;
    TRY(h->sq_keys.ensure(slots * K * 8));
    TRY(h->sq_cnt.ensure(slots * 4));
    if (!h->sq_arrive.p) {
        TRY(h->sq_arrive.ensure(64 * 4));
        HIP_TRY(hipMemsetAsync(h->sq_arrive.p, 0, h->sq_arrive.bytes, h->stream));
    }
    SqArgs a;
    a.ix = index_view(h);
    a.queries = d_q;
    a.nq = (int)nq; a.w = w; a.K = K; a.nch = nch; a.CH = CH;
    a.cdist = inside ? (const float *)nullptr : h->cdist.as<float>();
    a.centroids_t = h->cent_t.as<float>();
    a.part_keys = h->sq_keys.as<u64>();
    a.part_cnt = h->sq_cnt.as<u32>();
    a.arrive = h->sq_arrive.as<u32>();
    a.out_ids = c.ids; a.out_dists = c.dists; a.out_counts = c.counts;
    a.scanned_points = h->misc.as<u64>();
    const size_t lds = sq_lds_bytes(h->m, h->d, inside ? h->kc : 0);
    sq_fn_t fn = pick_sq(h->m, h->dsub);
    int occ = 0;
    TRY(fn_occupancy(h, (const void *)fn, lds, occ));
    ivfadc_index::EvPair ep;
    if (h->profiling) TRY(ev_begin(h, 0, ep));
    hipLaunchKernelGGL(fn, dim3((unsigned)slots), dim3(256), lds, h->stream, a);
    HIP_TRY(hipGetLastError());
    if (h->profiling) TRY(ev_end(h, ep));
    h->stats.queries += nq;
    h->stats.last_qg = -3;
    h->stats.coarse_mfma = 0;
    h->stats.coarse_listed = 0;
    h->stats.last_lb = 0;
    h->stats.last_chunk = (int)CH;
    h->stats.last_scan_grid = (int)slots;
    h->stats.last_scan_lds = (int)lds;
    return IVFADC_OK;
}

// clears the hint of ivfadc_set_next_queries when a search ends, however it ends (a hint is good for ONE search)
struct HintScope {
    ivfadc_index *h;
    ~HintScope()
    {
        // (a wait that no rider launch consumed still belongs in the stream: the NEXT search on this lane reads those rows as its own)
        if (h->hint_ev && h->stream) (void)hipStreamWaitEvent(h->stream, h->hint_ev, 0);
        h->hint_ev = nullptr;
        h->hint_q = nullptr; h->hint_nq = 0; h->hint_token = 0; h->avail_q = nullptr; h->avail_nq = 0;
    }
};

// ---- certified two-level coarse search: grouping of the centroids (twolevel.hip.h) ---------------------------------------------------
int twolevel_group(ivfadc_index *h, int G, std::vector<int> &assign);   // (with the trainer, below: k-means of the centroids into h->tl_centres)

constexpr int TL_AUTO_MIN_KC = 4096;   // automatic mode: quantizers whose exhaustive coarse stage is a visible share of a step
// ... and only where the self-probe computes at most this fraction of the kc distances.  Measured on a trained kc = 65 536, d = 96
// quantizer, 10 000 queries, w = 32 (profiles/r05_two_level_coarse.json): 0.1 % -> 0.18 ms against 0.63 ms for the matrix-core filter +
// refine + top-w; with a poorer grouping, 4.5 % -> 0.92 ms.  A visited centroid costs its d floats from L2 / MALL once per QUERY (the
// exhaustive kernels read a centroid once per 128-query tile), so the break-even sits near 2.5 %.
constexpr float TL_AUTO_MAX_FRACTION = 0.02f;

int build_twolevel(ivfadc_index *h)
{
    h->tl_tried = true;
    h->tl_use = false;
    const int kc = h->kc, d = h->d;
    if ((d & 3) != 0 || kc < 128) return IVFADC_OK;
    int G = std::max(16, std::min(2048, kc / 64));
    TRY(set_device(h));
    std::vector<float> cent((size_t)kc * d);
    std::vector<int> assign;
    TRY(h->tl_centres.ensure((size_t)G * d * 4));
    // k-means over the centroids themselves (the trainer's own code: k-means++ seeding, exact assignment, deterministic sums)
    TRY(twolevel_group(h, G, assign));
    TRY(d2h_copy(cent.data(), h->centroids.p, cent.size() * 4, h->stream));
    // ---- refinement on the host.  k-means++ over the centroids leaves some groups that span two natural clusters (a cluster that drew
    // no seed is shared out among its neighbours): their radius is the distance BETWEEN clusters, their bound is useless, and -- distances
    // between cluster centres concentrate in high dimension -- every query ends up visiting every such group (measured on a trained
    // kc = 65 536 quantizer: 46 of 1024 groups visited per query, 4.5 % of the distances).  So: groups whose radius stands out against
    // the median are split by 2-means until none does; centres are the members' means, radii are taken against those centres.
    std::vector<std::vector<int>> mem((size_t)G);
    for (int c = 0; c < kc; ++c) mem[assign[c]].push_back(c);
    auto centre_of = [&](const std::vector<int> &l, std::vector<float> &out) {
        std::vector<double> acc((size_t)d, 0.0);
        for (int c : l)
            for (int i = 0; i < d; ++i) acc[i] += (double)cent[(size_t)c * d + i];
        out.resize((size_t)d);
        for (int i = 0; i < d; ++i) out[i] = (float)(acc[i] / (double)std::max<size_t>(1, l.size()));
    };
    auto dist2 = [&](int c, const float *g) {
        double r2 = 0.0;
        for (int i = 0; i < d; ++i) { const double t = (double)cent[(size_t)c * d + i] - (double)g[i]; r2 += t * t; }
        return r2;
    };
    auto radius_of = [&](const std::vector<int> &l, const std::vector<float> &g) {
        double r2 = 0.0;
        for (int c : l) r2 = std::max(r2, dist2(c, g.data()));
        return std::sqrt(r2);
    };
    const size_t gmax = (size_t)std::min(8192, std::max(G, kc / 8));
    for (int round = 0; round < 6; ++round) {
        std::vector<double> rr;
        std::vector<std::vector<float>> ctr(mem.size());
        for (size_t g = 0; g < mem.size(); ++g) {
            if (mem[g].empty()) { rr.push_back(0.0); continue; }
            centre_of(mem[g], ctr[g]);
            rr.push_back(radius_of(mem[g], ctr[g]));
        }
        std::vector<double> nz;
        for (size_t g = 0; g < mem.size(); ++g)
            if (mem[g].size() >= 2) nz.push_back(rr[g]);
        if (nz.empty()) break;
        std::nth_element(nz.begin(), nz.begin() + nz.size() / 2, nz.end());
        const double med = nz[nz.size() / 2];
        bool any = false;
        const size_t ng0 = mem.size();
        for (size_t g = 0; g < ng0 && mem.size() < gmax; ++g) {
            if (mem[g].size() < 4 || rr[g] <= 1.3 * med) continue;
            // 2-means: seeds = the member farthest from the centre and the member farthest from that one
            int a = mem[g][0];
            double best = -1.0;
            for (int c : mem[g]) { const double v = dist2(c, ctr[g].data()); if (v > best) { best = v; a = c; } }
            int b = a;
            best = -1.0;
            for (int c : mem[g]) { const double v = dist2(c, &cent[(size_t)a * d]); if (v > best) { best = v; b = c; } }
            if (a == b) continue;
            std::vector<float> ca(cent.begin() + (size_t)a * d, cent.begin() + (size_t)(a + 1) * d), cb(cent.begin() + (size_t)b * d, cent.begin() + (size_t)(b + 1) * d);
            std::vector<int> la, lb;
            for (int it = 0; it < 8; ++it) {
                la.clear(); lb.clear();
                for (int c : mem[g]) (dist2(c, ca.data()) <= dist2(c, cb.data()) ? la : lb).push_back(c);
                if (la.empty() || lb.empty()) break;
                centre_of(la, ca);
                centre_of(lb, cb);
            }
            if (la.empty() || lb.empty()) continue;
            mem[g].swap(la);
            mem.push_back(lb);
            any = true;
        }
        if (!any) break;
    }
    mem.erase(std::remove_if(mem.begin(), mem.end(), [](const std::vector<int> &l) { return l.empty(); }), mem.end());
    const int G2 = (int)mem.size();
    std::vector<float> gc((size_t)G2 * d);
    std::vector<u32> off((size_t)G2 + 1, 0);
    for (int g = 0; g < G2; ++g) {
        std::vector<float> c_;
        centre_of(mem[g], c_);
        std::copy(c_.begin(), c_.end(), gc.begin() + (size_t)g * d);
        off[g + 1] = off[g] + (u32)mem[g].size();
    }
    // slots in group order (a group's members side by side, no padding: the kernel masks the lanes past a group's end); radii in
    // double against the float centres the device will use, rounded up
    const size_t slots = off[G2];
    std::vector<u32> slot_id(std::max<size_t>(slots, 1), 0xFFFFFFFFu);
    std::vector<float> grouped(std::max<size_t>(slots, 1) * d, 0.0f), rad((size_t)G2, 0.0f);
    for (int g = 0; g < G2; ++g) {
        const u32 ns = off[g + 1] - off[g];
        float *blk = grouped.data() + (size_t)off[g] * d;
        double r2max = 0.0;
        for (u32 sl = 0; sl < ns; ++sl) {
            const int c = mem[g][sl];
            slot_id[off[g] + sl] = (u32)c;
            for (int i = 0; i < d; ++i) blk[((size_t)(i >> 2) * ns + sl) * 4 + (i & 3)] = cent[(size_t)c * d + i];
            r2max = std::max(r2max, dist2(c, &gc[(size_t)g * d]));
        }
        rad[g] = std::nextafter((float)(std::sqrt(r2max) * (1.0 + 1e-6)), INFINITY);
    }
    TRY(h->tl_centres.ensure(gc.size() * 4));
    TRY(h->tl_off.ensure(off.size() * 4));
    TRY(h->tl_rad.ensure(rad.size() * 4));
    TRY(h->tl_cent.ensure(grouped.size() * 4 + 64));
    TRY(h->tl_slot.ensure(slot_id.size() * 4));
    TRY(h2d_copy(h->tl_centres.p, gc.data(), gc.size() * 4, h->stream));
    TRY(h2d_copy(h->tl_off.p, off.data(), off.size() * 4, h->stream));
    TRY(h2d_copy(h->tl_rad.p, rad.data(), rad.size() * 4, h->stream));
    TRY(h2d_copy(h->tl_cent.p, grouped.data(), grouped.size() * 4, h->stream));
    TRY(h2d_copy(h->tl_slot.p, slot_id.data(), slot_id.size() * 4, h->stream));
    G = G2;
    h->tl_G = G;
    h->tl_eps = (float)(d + 16) * 1.1920929e-7f;   // (d + 16) 2^-23
    // Self-probe: up to 1024 centroids as queries (what a query of a trained index looks like from the quantizer's side), w = 32: the
    // fraction of the kc distances the search still computes.  Automatic mode keeps the two-level search only if the bounds leave at
    // most TL_AUTO_MAX_FRACTION of them -- N(0,1) quantizers in high dimension show ~1.0 here (distance concentration) and stay exhaustive.
    {
        const int64_t ns = std::min<int64_t>(1024, kc);
        const int wp = std::min(32, kc);
        TRY(ensure_common_ws(h));
        DevBuf pl_, pd_, pb_;
        int rc = pl_.ensure((size_t)ns * wp * 4);
        if (rc == IVFADC_OK) rc = pd_.ensure((size_t)ns * wp * 4);
        if (rc == IVFADC_OK) rc = pb_.ensure((size_t)ns * wp * 4);
        u64 before[512], after[512];
        if (rc == IVFADC_OK) {
            HIP_TRY(hipStreamSynchronize(h->stream));
            HIP_TRY(hipMemcpy(before, h->misc.p, sizeof(before), hipMemcpyDeviceToHost));
            // (every 64th... a contiguous block of centroid rows is a valid query matrix: [ns][d])
            const bool prof = h->profiling;
            h->profiling = false;
            rc = run_twolevel(h, h->centroids.as<float>(), ns, wp, pl_.as<int>(), pd_.as<float>(), pb_.as<u32>(), nullptr, h->misc.as<u64>());
            h->profiling = prof;
        }
        if (rc == IVFADC_OK) {
            HIP_TRY(hipStreamSynchronize(h->stream));
            HIP_TRY(hipMemcpy(after, h->misc.p, sizeof(after), hipMemcpyDeviceToHost));
            u64 vis = 0;
            for (int i = 0; i < 64; ++i) vis += after[i * 8 + 3] - before[i * 8 + 3];
            // the probe's counts do not belong to any search: take them out again
            TRY(h2d_copy(h->misc.p, before, sizeof(before), h->stream));
            h->tl_probe_fraction = (float)((double)vis / ((double)ns * (double)kc));
        }
        pl_.release(); pd_.release(); pb_.release();
        if (rc != IVFADC_OK) return rc;
    }
    h->tl_use = h->tl_mode > 0 || (h->tl_mode == 0 && h->tl_probe_fraction >= 0.f && h->tl_probe_fraction <= TL_AUTO_MAX_FRACTION);
    return IVFADC_OK;
}

// The first lines of every search (search_dev, range_dev, coarse_dev).  Rows the previous search's riders left serve THIS search or none,
// whatever path it takes (small-batch, generic, sub-batched, failing): they are taken over here and forgotten.  take_rows (search_dev
// alone): they are offered when the caller declared this search's queries to be the very generation the rows were computed from (same
// token, != 0) -- a staging buffer refilled in between carries another token.  Otherwise avail_q is cleared; coarse_dev used to leave that
// to the HintScope of the search before it, which comes to the same: every search ends through a HintScope and nothing else sets avail_q.
// partial_nq: the probe arrays a pending ivfadc_merge_partials_device would read are about to be overwritten.  group_centroids: the
// grouping of a large quantizer is built on its first search with queries (automatic mode), or on request (ivfadc_set_coarse_mode(h, 6)).
int begin_search(ivfadc_index *h, int64_t nq, bool take_rows, bool group_centroids)
{
    const bool declared = take_rows && h->cur_token != 0 && h->cur_token == h->pf_token;
    h->avail_q = declared ? h->pf_q : nullptr;
    h->avail_nq = declared ? h->pf_nq : 0;
    h->pf_q = nullptr; h->pf_nq = 0; h->pf_token = 0; h->cur_token = 0;
    h->stats.coarse_prefetched = 0;
    h->stats.last_rider = 0;
    h->partial_nq = -1;
    TRY(set_device(h));
    if (h->dirty) TRY(upload_lists(h));
    if (nq > 0 && group_centroids && !h->tl_tried && !h->is_view && h->tl_mode >= 0 && (h->tl_mode > 0 || h->kc >= TL_AUTO_MIN_KC)) TRY(build_twolevel(h));
    return IVFADC_OK;
}

// Supplied probes (c.pre_list, ivfadc_search_preassigned): the search has no coarse stage of its own -- no latency path, no fused top-w,
// no matrix-core filter, no two-level search, no riders -- and everything behind the probe arrays runs as it does for a plain search.
// A mask set (c.mask_words, ivfadc_search_masked): the coarse stage is the plain search's own, in any form; behind it the masked list
// scan (make_plan_masked) or the masked generic path -- no latency path, no fused top-w, no riders.  Both together: there is no entry.
int search_dev(ivfadc_index *h, const SearchCall &c)
{
    HintScope hint_scope{h};
    const bool pre = c.pre(), masked = c.masked();
    const int64_t nq = c.nq;
    const int K = c.K, w = c.w;
    TRY(begin_search(h, nq, true, !pre));
    if (nq == 0) return IVFADC_OK;
    const bool parted = h->part_n > 1;
    if (masked && (pre || parted)) return fail(IVFADC_ERR_STATE, "a masked search takes neither supplied probes nor a list partition");
    if (!masked && !parted && !pre && sq_eligible(h, nq, K, w)) return search_small(h, c);
    if (K > IVFADC_MAX_K || w > IVFADC_MAX_W || h->force_qg == -2 || (h->u16 && (masked || (K > 64 && !h->u16_wide)))) {
        if (parted) return fail(IVFADC_ERR_INVALID, "list-partitioned mode reaches K <= %d and w <= %d", IVFADC_MAX_K, IVFADC_MAX_W);
        return search_generic(h, c);
    }
    TRY(fb_poll(h));
    const PlanFacts facts = plan_facts(h);
    Plan pl = masked ? make_plan_masked(facts, nq, K, w) : h->u16 ? make_plan_u16(facts, nq, K, w, pre) : make_plan(facts, nq, K, w, pre);
    if (!pl.fits) {
        if (parted) return fail(IVFADC_ERR_INVALID, "list-partitioned mode: the selection kernels' LDS need exceeds a CU for this m and K");
        return search_generic(h, c);   // "any K and w" holds for every m
    }
    TRY(plan_kernel(pl, h->m, h->dsub));
    if (parted && pl.nb < nq)
        return fail(IVFADC_ERR_INVALID, "list-partitioned mode: the batch must fit one sub-batch (raise ivfadc_set_workspace_limit or split the batch)");
    for (int64_t b0 = 0; b0 < nq; b0 += pl.nb) TRY(search_subbatch(h, pl, c.slice(b0, std::min(pl.nb, nq - b0))));
    return IVFADC_OK;
}

// ---- range search (range.hip.h; range_plan.h): count, scan, fill, sort the survivors, emit CSR -----------------------------------------
range_plan::Facts range_facts(const ivfadc_index *h)
{
    range_plan::Facts f;
    f.d = h->d; f.kc = h->kc; f.m = h->m; f.ksub = h->ksub;
    f.n = 0; f.maxlen = 0;
    for (int64_t v : h->mirror.h_len) { f.n += v; f.maxlen = std::max(f.maxlen, v); }
    f.force_chunk = h->force_chunk;
    f.ws_budget = h->ws_budget;
    f.lds_max = LDS_MAX;
    f.table_free = h->u16;   // 16-bit codes: range_u16_*_kernel, sums straight from the codebook
    return f;
}

// c.q, c.radii: the queries and their radii in device memory.  Blocking: the result is complete when this returns.
// c.mask_* (ivfadc_range_search_masked): the set and the batch's mask numbers on the device, every value in [-1, nmasks); no set: no
// query is filtered.  The kernel pair follows (16-bit codes, mask present): range_u16_* for a 16-bit handle with or without a set,
// range_masked_* for an 8-bit handle with one, the plain pair otherwise.
int range_dev(ivfadc_index *h, const SearchCall &c, int64_t max_total, ivfadc_range_result **out)
{
    HintScope hint_scope{h};
    TRY(begin_search(h, c.nq, false, false));
    const int64_t nq = c.nq; const int w = c.w;
    range_plan::Facts facts = range_facts(h);
    facts.masked = c.masked();
    const range_plan::Plan pl = range_plan::make_plan(facts, nq, w);
    if (!pl.fits) return fail(IVFADC_ERR_INVALID, "range search (d=%d, m=%d, w=%d): %s", h->d, h->m, w, pl.why);
    std::unique_ptr<ivfadc_range_result> res(new ivfadc_range_result);
    res->device = h->device;
    res->nq = nq;
    std::vector<uint64_t> tot((size_t)nq, 0);
    const IndexView ix = index_view(h);
    const bool with_mv = h->u16 || c.masked();   // the kernels that take a MaskView
    const range_masked_fn_t count_mv = h->u16 ? range_u16_count_kernel : range_masked_count_kernel;
    const range_masked_fn_t fill_mv = h->u16 ? range_u16_fill_kernel : range_masked_fill_kernel;
    if (nq > 0) {
        TRY(fn_raise_lds(h->device, with_mv ? (const void *)count_mv : (const void *)range_count_kernel, pl.lds, true));
        TRY(fn_raise_lds(h->device, with_mv ? (const void *)fill_mv : (const void *)range_fill_kernel, pl.lds, true));
        TRY(ensure_common_ws(h));
    }
    const int64_t items = pl.items;
    // what both passes hand their kernels: the queries of cs, their probes pr and their item counts from query i0 of the sub-batch on
    auto range_args = [&](const SearchCall &cs, const ProbeRows &pr, int64_t i0) {
        RangeArgs a{};
        a.ix = ix;
        a.queries = cs.q;
        a.radii = cs.radii;
        a.w = w; a.chunk = pl.chunk; a.maxch = (u32)pl.maxch;
        a.probe_list = pr.list; a.probe_dc = pr.dc; a.probe_base = pr.base;
        a.item_cnt = h->rng_cnt.as<u32>() + (size_t)i0 * (size_t)items;
        return a;
    };
    // stage A of the generic path (exact coarse distances, sorted rows, the w probes) and the count pass of the sub-batch ca
    auto count_batch = [&](const SearchCall &ca, u64 *d_scanned) -> int {
        const int64_t na = ca.nq;
        const size_t np = (size_t)na * w, ni = (size_t)na * (size_t)items;
        TRY(h->probe_list.ensure(np * 4));
        TRY(h->probe_dc.ensure(np * 4));
        TRY(h->probe_base.ensure(np * 4));
        TRY(h->gen_tot.ensure((size_t)na * 4));
        TRY(h->rng_tot.ensure((size_t)na * 4));
        TRY(h->rng_cnt.ensure(ni * 4));
        TRY(h->rng_off.ensure(ni * 4));
        TRY(gen_stage_a(h, ca.q, na, w, h->probe_list.as<int>(), h->probe_dc.as<float>(), h->probe_base.as<u32>(), d_scanned));
        const RangeArgs a = range_args(ca, probe_rows(h, w), 0);
        if (with_mv) hipLaunchKernelGGL(count_mv, dim3((unsigned)items, (unsigned)na), dim3(256), pl.lds, h->stream, a, mask_view(ca));
        else hipLaunchKernelGGL(range_count_kernel, dim3((unsigned)items, (unsigned)na), dim3(256), pl.lds, h->stream, a);
        HIP_TRY(hipGetLastError());
        hipLaunchKernelGGL(range_offsets_kernel, dim3((unsigned)na), dim3(256), 0, h->stream, h->rng_cnt.as<u32>(), (u32)items, h->rng_off.as<u32>(),
                           h->rng_tot.as<u32>());
        HIP_TRY(hipGetLastError());
        return IVFADC_OK;
    };
    const int64_t nbatches = nq == 0 ? 0 : (nq + pl.nb - 1) / pl.nb;
    std::vector<u32> tot32;
    for (int64_t a0 = 0; a0 < nq; a0 += pl.nb) {   // pass 1: every query's total, before anything of the result is allocated
        const int64_t na = std::min(pl.nb, nq - a0);
        TRY(count_batch(c.slice(a0, na), h->misc.as<u64>()));
        tot32.resize((size_t)na);
        TRY(d2h_copy(tot32.data(), h->rng_tot.p, (size_t)na * 4, h->stream));
        HIP_TRY(hipStreamSynchronize(h->stream));
        for (int64_t q = 0; q < na; ++q) tot[(size_t)(a0 + q)] = tot32[(size_t)q];
    }
    res->lims = range_plan::make_lims(tot);
    res->total = res->lims[(size_t)nq];
    if (max_total > 0 && res->total > max_total)
        return fail(IVFADC_ERR_INVALID, "the range search holds %lld results, more than max_total = %lld", (long long)res->total, (long long)max_total);
    HIP_TRY(hipMalloc((void **)&res->d_lims, ((size_t)nq + 1) * 8));
    HIP_TRY(hipMalloc((void **)&res->d_ids, (size_t)std::max<int64_t>(1, res->total) * 4));
    HIP_TRY(hipMalloc((void **)&res->d_dists, (size_t)std::max<int64_t>(1, res->total) * 4));
    TRY(h2d_copy(res->d_lims, res->lims.data(), ((size_t)nq + 1) * 8, h->stream));
    for (int64_t a0 = 0; a0 < nq && res->total > 0; a0 += pl.nb) {   // pass 2: fill, sort, emit
        const SearchCall ca = c.slice(a0, std::min(pl.nb, nq - a0));
        // several sub-batches: the probe arrays and item words of this one were overwritten; the same launches give the same words again
        // (their B_alg counts go to the lines nobody reads: the points were counted in pass 1)
        if (nbatches > 1) TRY(count_batch(ca, (u64 *)((char *)h->misc.p + MISC_SINK)));
        const std::vector<uint64_t> tb(tot.begin() + a0, tot.begin() + a0 + ca.nq);
        TRY(for_sort_groups(h, tb, pl.cap_keys, true, "holds", "results", [&](int64_t g0, int64_t ng, int64_t keys) -> int {
            const SearchCall cg = ca.slice(g0, ng);
            RangeArgs a = range_args(cg, probe_rows(h, w).slice(g0), g0);
            a.item_off = h->rng_off.as<u32>() + (size_t)g0 * (size_t)items;
            a.key_off = h->gen_off.as<u32>();
            a.keys = h->gen_a.as<u64>();
            if (with_mv) hipLaunchKernelGGL(fill_mv, dim3((unsigned)items, (unsigned)ng), dim3(256), pl.lds, h->stream, a, mask_view(cg));
            else hipLaunchKernelGGL(range_fill_kernel, dim3((unsigned)items, (unsigned)ng), dim3(256), pl.lds, h->stream, a);
            HIP_TRY(hipGetLastError());
            TRY(gen_sort(h, h->gen_a.as<u64>(), h->gen_b.as<u64>(), keys, (int)ng, h->gen_off.as<u32>()));
            const unsigned ey = (unsigned)std::max<int64_t>(1, std::min<int64_t>(64, (keys / ng + 1023) / 1024));
            hipLaunchKernelGGL(range_emit_kernel, dim3((unsigned)ng, ey), dim3(256), 0, h->stream, h->gen_b.as<u64>(), h->gen_off.as<u32>(), w,
                               a.probe_list, a.probe_base, h->list_pos.as<int64_t>(), ix.ids, res->d_lims + a0 + g0, res->d_ids, res->d_dists);
            HIP_TRY(hipGetLastError());
            return IVFADC_OK;
        }));
    }
    HIP_TRY(hipStreamSynchronize(h->stream));
    h->stats.queries += nq;
    *out = res.release();
    return IVFADC_OK;
}

// coarse_search(cq, point, w) (coarsequantizers.jl:33-37) for a batch, into the caller's device rows: the coarse stage a search plans --
// exact VALU kernel, matrix-core filter + certified refine, or the certified two-level search; the same bytes from each -- with the
// stand-alone top-w kernel (or the two-level kernel) writing lists and distances straight into d_lists / d_dists.  The visit-order
// bases go to the handle's own probe_base, the B_alg counts to the sink: nothing is scanned.  w > IVFADC_MAX_W: the generic path's sort.
// c.out_list / c.out_dc: the caller's device rows.
int coarse_dev(ivfadc_index *h, const SearchCall &c)
{
    HintScope hint_scope{h};
    const int64_t nq = c.nq;
    const int w = c.w;
    TRY(begin_search(h, nq, false, true));   // (partial_nq: probe_base is rewritten)
    if (nq == 0) return IVFADC_OK;
    TRY(ensure_common_ws(h));
    const int kc = h->kc;
    u64 *d_sink = (u64 *)((char *)h->misc.p + MISC_SINK);
    const bool generic = w > IVFADC_MAX_W;
    const CoarseForm cf = coarse_form(plan_facts(h), w, !generic, true);   // (any batch size: the sub-batches below are clamped to the two-level kernel's)
    const bool twolevel = cf.twolevel, mfma = cf.mfma;
    // sub-batches: the distance rows (generic: + two key rows) stay inside the workspace budget
    const size_t per_q = (twolevel ? (size_t)h->tl_G : (size_t)kc) * (generic ? 20 : 4) + (size_t)w * 4 + 64;
    int64_t nb = (int64_t)std::max<size_t>(generic ? 1 : 64, h->ws_budget / per_q);
    nb = std::min<int64_t>(nb, (int64_t)1 << 22);
    if (twolevel) nb = std::min<int64_t>(nb, std::max<int64_t>(1, ((int64_t)1 << 30) / std::max(1, h->tl_G)));
    if (generic) nb = std::min<int64_t>(nb, std::min<int64_t>(65535, ((int64_t)1 << 31) / std::max(1, kc)));
    nb = std::max<int64_t>(1, std::min<int64_t>(nb, nq));
    TRY(h->probe_base.ensure((size_t)nb * w * 4));
    h->stats.last_twolevel = twolevel ? 1 : 0;
    h->stats.coarse_mfma = mfma ? 1 : 0;
    for (int64_t b0 = 0; b0 < nq; b0 += nb) {
        const SearchCall cb = c.slice(b0, std::min(nb, nq - b0));
        const int64_t n = cb.nq; const float *q = cb.q; int *ol = cb.out_list; float *od = cb.out_dc;
        if (generic) {
            TRY(h->gen_tot.ensure((size_t)n * 4));
            TRY(gen_stage_a(h, q, n, w, ol, od, h->probe_base.as<u32>(), d_sink));
            continue;
        }
        if (twolevel) {
            TRY(run_twolevel(h, q, n, w, ol, od, h->probe_base.as<u32>(), nullptr, d_sink));
            h->tmin_tiles = 0;
            h->last_listed = false;
            continue;
        }
        const bool wpq4 = n < (int64_t)8 * h->num_cu * 4 && kc >= 512;   // (search_subbatch: a workgroup per query on small batches)
        TRY(run_coarse(h, q, n, mfma, mfma && !wpq4, !wpq4, w));
        TRY(launch_topw(h, q, n, w, sel_cap(w), mfma, wpq4, ol, od, h->probe_base.as<u32>(), nullptr, d_sink, 1, 0));
        h->stats.coarse_f16 = (mfma && h->last_coarse_f16) ? 1 : 0;
        h->stats.coarse_listed = h->last_listed ? 1 : 0;
    }
    return IVFADC_OK;
}

int encode_dev(ivfadc_index *h, int64_t n, const float *pts, int32_t *out_list, uint8_t *out_codes)
{
    // batches keep the n x kc distance matrix bounded
    const int64_t bmax = std::max<int64_t>(256, (int64_t)(((size_t)1 << 30) / ((size_t)h->kc * 4)));
    const size_t lds = align_up((size_t)h->d, 4) * 4 + (size_t)h->m * 8;
    for (int64_t b0 = 0; b0 < n; b0 += bmax) {
        const int64_t nb = std::min(bmax, n - b0);
        TRY(h->pts_stage.ensure((size_t)nb * h->d * 4));
        TRY(h->assign.ensure((size_t)nb * 4));
        TRY(h->enc_codes.ensure((size_t)nb * h->cb));
        TRY(h2d_copy(h->pts_stage.p, pts + (size_t)b0 * h->d, (size_t)nb * h->d * 4, h->stream));
        TRY(run_coarse(h, h->pts_stage.as<float>(), nb, false));   // push! path: exact distances
        hipLaunchKernelGGL(argmin_rows_kernel, dim3((unsigned)((nb + 3) / 4)), dim3(256), 0, h->stream, h->cdist.as<float>(), (int)nb,
                           h->kc, h->assign.as<int>());
        HIP_TRY(hipGetLastError());
        if (h->u16)   // codeword indices; the caller translates them to labels
            hipLaunchKernelGGL(encode_u16_kernel, dim3((unsigned)nb), dim3(256), lds, h->stream, h->pts_stage.as<float>(), h->assign.as<int>(),
                               h->d, h->m, h->ksub, h->dsub, h->centroids.as<float>(), h->codebooks.as<float>(), h->enc_codes.as<uint16_t>());
        else
        hipLaunchKernelGGL(encode_kernel, dim3((unsigned)nb), dim3(256), lds, h->stream, h->pts_stage.as<float>(), h->assign.as<int>(),
                           h->d, h->m, h->ksub, h->dsub, h->centroids.as<float>(), h->codebooks.as<float>(), h->labels.as<uint8_t>(),
                           h->enc_codes.as<uint8_t>());
        HIP_TRY(hipGetLastError());
        TRY(d2h_copy(out_list + b0, h->assign.p, (size_t)nb * 4, h->stream));
        TRY(d2h_copy(out_codes + (size_t)b0 * h->cb, h->enc_codes.p, (size_t)nb * h->cb, h->stream));
        HIP_TRY(hipStreamSynchronize(h->stream));
    }
    return IVFADC_OK;
}

}  // namespace

// ---- training (train.hip.h) ---------------------------------------------------------------------
namespace {

struct TrainCtx {
    hipStream_t stream = nullptr;
    DevBuf cdist, assign, mind, partial, acc, counts, flag, blockmax;
};

// k-means of the n x dcols window (leading dimension ld) of d_x into d_centres [k][dcols]
int kmeans_dev(TrainCtx &t, const float *d_x, int64_t n, int dcols, int ld, int k, int maxiter, uint64_t seed, float *d_centres)
{
    // ---- k-means++ over a strided subsample
    const int S = (int)std::min<int64_t>(n, std::max<int64_t>(32768, (int64_t)32 * k));
    const int nblk = (S + 255) / 256;
    TRY(t.mind.ensure((size_t)S * 4));
    TRY(t.partial.ensure((size_t)nblk * 8));
    for (int j = 0; j < k; ++j) {
        if (j > 0) {
            hipLaunchKernelGGL(tr_kmpp_update_kernel, dim3(nblk), dim3(256), 0, t.stream, d_x, n, dcols, ld, S,
                               d_centres + (size_t)(j - 1) * dcols, t.mind.as<float>(), t.partial.as<double>(), j == 1 ? 1 : 0);
            HIP_TRY(hipGetLastError());
        }
        hipLaunchKernelGGL(tr_kmpp_pick_kernel, dim3(1), dim3(64), 0, t.stream, d_x, n, dcols, ld, S, t.mind.as<float>(),
                           t.partial.as<double>(), nblk, (u64)seed, j, d_centres);
        HIP_TRY(hipGetLastError());
    }
    // ---- fixed-point scale 2^(61 - e), n * maxabs < 2^e exactly: |sum| <= n * maxabs * scale + n / 2 < 2^62, and the quantum
    // 1 / scale follows the data's binary magnitude, so training x * 2^j gives the centres of x times 2^j (all-zero data: e = 0)
    const int mb = 1024;
    TRY(t.blockmax.ensure((size_t)mb * 4));
    hipLaunchKernelGGL(tr_maxabs_kernel, dim3(mb), dim3(256), 0, t.stream, d_x, n, dcols, ld, t.blockmax.as<float>());
    HIP_TRY(hipGetLastError());
    std::vector<float> bm(mb);
    HIP_TRY(hipMemcpyAsync(bm.data(), t.blockmax.p, (size_t)mb * 4, hipMemcpyDeviceToHost, t.stream));
    HIP_TRY(hipStreamSynchronize(t.stream));
    double maxabs = 0.0;
    for (float v : bm) maxabs = std::max(maxabs, (double)v);
    int ex = 0;
    std::frexp((double)n * maxabs, &ex);
    const double scale = std::ldexp(1.0, 61 - ex);

    // ---- Lloyd
    const int64_t chunk = std::max<int64_t>(256, (int64_t)(((size_t)1 << 30) / ((size_t)k * 4)));
    TRY(t.cdist.ensure((size_t)std::min<int64_t>(n, chunk) * k * 4));
    TRY(t.assign.ensure((size_t)n * 4));
    TRY(t.acc.ensure((size_t)k * dcols * 8));
    TRY(t.counts.ensure((size_t)k * 4));
    TRY(t.flag.ensure(4));
    for (int it = 0; it < maxiter; ++it) {
        for (int64_t p0 = 0; p0 < n; p0 += chunk) {
            const int64_t nb = std::min(chunk, n - p0);
            dim3 grid((k + CO_T - 1) / CO_T, (unsigned)((nb + 63) / 64));
            hipLaunchKernelGGL(coarse_dist_kernel<64>, grid, dim3(256), 0, t.stream, d_x + (size_t)p0 * ld, d_centres,
                               t.cdist.as<float>(), (int)nb, k, dcols, ld);
            HIP_TRY(hipGetLastError());
            hipLaunchKernelGGL(argmin_rows_kernel, dim3((unsigned)((nb + 3) / 4)), dim3(256), 0, t.stream, t.cdist.as<float>(),
                               (int)nb, k, t.assign.as<int>() + p0);
            HIP_TRY(hipGetLastError());
        }
        HIP_TRY(hipMemsetAsync(t.acc.p, 0, (size_t)k * dcols * 8, t.stream));
        HIP_TRY(hipMemsetAsync(t.counts.p, 0, (size_t)k * 4, t.stream));
        HIP_TRY(hipMemsetAsync(t.flag.p, 0, 4, t.stream));
        hipLaunchKernelGGL(tr_accumulate_kernel, dim3(2048), dim3(256), 0, t.stream, d_x, n, dcols, ld, t.assign.as<int>(), scale,
                           t.acc.as<long long>(), t.counts.as<u32>());
        HIP_TRY(hipGetLastError());
        hipLaunchKernelGGL(tr_finalize_kernel, dim3((unsigned)(((size_t)k * dcols + 255) / 256)), dim3(256), 0, t.stream, d_x, n,
                           dcols, ld, k, t.acc.as<long long>(), t.counts.as<u32>(), 1.0 / scale, (u64)seed, it, d_centres,
                           t.flag.as<int>());
        HIP_TRY(hipGetLastError());
        int changed = 0;
        HIP_TRY(hipMemcpyAsync(&changed, t.flag.p, 4, hipMemcpyDeviceToHost, t.stream));
        HIP_TRY(hipStreamSynchronize(t.stream));
        if (!changed) break;   // Lloyd's fixed point
    }
    return IVFADC_OK;
}

// the centroids of an index grouped for the two-level coarse search: G centres into h->tl_centres, every centroid's group into `assign`
int twolevel_group(ivfadc_index *h, int G, std::vector<int> &assign)
{
    const int kc = h->kc, d = h->d;
    TrainCtx t;
    HIP_TRY(hipStreamCreateWithFlags(&t.stream, hipStreamNonBlocking));
    auto body = [&]() -> int {
        HIP_TRY(hipStreamSynchronize(h->stream));
        TRY(kmeans_dev(t, h->centroids.as<float>(), kc, d, d, G, 12, 0x7107ull, h->tl_centres.as<float>()));
        // final assignment against the final centres
        TRY(t.cdist.ensure((size_t)kc * G * 4));
        TRY(t.assign.ensure((size_t)kc * 4));
        dim3 grid((G + CO_T - 1) / CO_T, (unsigned)((kc + 63) / 64));
        hipLaunchKernelGGL(coarse_dist_kernel<64>, grid, dim3(256), 0, t.stream, h->centroids.as<float>(), h->tl_centres.as<float>(),
                           t.cdist.as<float>(), kc, G, d, d);
        HIP_TRY(hipGetLastError());
        hipLaunchKernelGGL(argmin_rows_kernel, dim3((unsigned)((kc + 3) / 4)), dim3(256), 0, t.stream, t.cdist.as<float>(), kc, G, t.assign.as<int>());
        HIP_TRY(hipGetLastError());
        assign.resize((size_t)kc);
        HIP_TRY(hipMemcpyAsync(assign.data(), t.assign.p, (size_t)kc * 4, hipMemcpyDeviceToHost, t.stream));
        HIP_TRY(hipStreamSynchronize(t.stream));
        for (int c = 0; c < kc; ++c)
            if (assign[c] < 0 || assign[c] >= G) return fail(IVFADC_ERR_STATE, "two-level grouping: centroid %d assigned to group %d", c, assign[c]);
        return IVFADC_OK;
    };
    const int rc = body();
    (void)hipStreamSynchronize(t.stream);
    DevBuf *bufs[] = {&t.cdist, &t.assign, &t.mind, &t.partial, &t.acc, &t.counts, &t.flag, &t.blockmax};
    for (DevBuf *b : bufs) b->release();
    (void)hipStreamDestroy(t.stream);
    return rc;
}

int train_impl(int device, int d, int64_t n, const float *data, int kc, int k, int m, int coarse_maxiter, int quant_maxiter,
               uint64_t seed, float *out_centroids, float *out_codebooks)
{
    if (d < 1 || n < 1 || !data || !out_centroids || !out_codebooks) return fail(IVFADC_ERR_INVALID, "bad argument");
    if (kc < 2) return fail(IVFADC_ERR_ASSERT, "Number of coarse clusters has to be >= 2");                   // index.jl:118
    if (k > n) return fail(IVFADC_ERR_ASSERT, "Number of quantization levels  has to be <= %lld", (long long)n);   // :119
    if (m < 1 || m > d) return fail(IVFADC_ERR_ASSERT, "Number of codebooks has to be between 1 and %d", d);       // :120
    if (coarse_maxiter < 1 || quant_maxiter < 1) return fail(IVFADC_ERR_ASSERT, "Number of clustering iterations has to be > 0");
    if (d % m != 0) return fail(IVFADC_ERR_INVALID, "d %% m != 0 is not supported");
    if (k < 1 || k > 65536) return fail(IVFADC_ERR_INVALID, "k must be in 1..65536 (UInt8 or UInt16 codes)");
    if (kc > n) return fail(IVFADC_ERR_INVALID, "kc > n");
    // the fixed-point scale and every distance assume finite data (fmaxf drops a NaN, an Inf has no binary exponent)
    for (int64_t e = 0; e < n * d; ++e)
        if (!std::isfinite(data[e]))
            return fail(IVFADC_ERR_INVALID, "training data is not finite: point %lld, component %d", (long long)(e / d), (int)(e % d));
    int ndev = 0;
    HIP_TRY(hipGetDeviceCount(&ndev));
    if (device < 0 || device >= ndev) return fail(IVFADC_ERR_HIP, "no such HIP device %d", device);
    HIP_TRY(hipSetDevice(device));
    TrainCtx t;
    HIP_TRY(hipStreamCreateWithFlags(&t.stream, hipStreamNonBlocking));
    DevBuf x, resid, cent, cbs;
    const int dsub = d / m;
    int rc = x.ensure((size_t)n * d * 4);
    if (rc == IVFADC_OK) rc = resid.ensure((size_t)n * d * 4);
    if (rc == IVFADC_OK) rc = cent.ensure((size_t)kc * d * 4);
    if (rc == IVFADC_OK) rc = cbs.ensure((size_t)k * dsub * 4);
    auto body = [&]() -> int {
        TRY(h2d_copy(x.p, data, (size_t)n * d * 4, t.stream));
        TRY(kmeans_dev(t, x.as<float>(), n, d, d, kc, coarse_maxiter, seed, cent.as<float>()));
        // final assignment -> residuals (index.jl:138,168-175): t.assign holds the last Lloyd assignment only if the
        // loop stopped at a fixed point, so assign once more against the final centres
        const int64_t chunk = std::max<int64_t>(256, (int64_t)(((size_t)1 << 30) / ((size_t)kc * 4)));
        for (int64_t p0 = 0; p0 < n; p0 += chunk) {
            const int64_t nb = std::min(chunk, n - p0);
            dim3 grid((kc + CO_T - 1) / CO_T, (unsigned)((nb + 63) / 64));
            hipLaunchKernelGGL(coarse_dist_kernel<64>, grid, dim3(256), 0, t.stream, x.as<float>() + (size_t)p0 * d, cent.as<float>(),
                               t.cdist.as<float>(), (int)nb, kc, d, d);
            HIP_TRY(hipGetLastError());
            hipLaunchKernelGGL(argmin_rows_kernel, dim3((unsigned)((nb + 3) / 4)), dim3(256), 0, t.stream, t.cdist.as<float>(),
                               (int)nb, kc, t.assign.as<int>() + p0);
            HIP_TRY(hipGetLastError());
        }
        hipLaunchKernelGGL(tr_residual_kernel, dim3(2048), dim3(256), 0, t.stream, x.as<float>(), n, d, t.assign.as<int>(),
                           cent.as<float>(), resid.as<float>());
        HIP_TRY(hipGetLastError());
        TRY(d2h_copy(out_centroids, cent.p, (size_t)kc * d * 4, t.stream));
        for (int i = 0; i < m; ++i) {
            TRY(kmeans_dev(t, resid.as<float>() + (size_t)i * dsub, n, dsub, d, k, quant_maxiter, seed + 1 + (uint64_t)i,
                           cbs.as<float>()));
            TRY(d2h_copy(out_codebooks + (size_t)i * k * dsub, cbs.p, (size_t)k * dsub * 4, t.stream));
            HIP_TRY(hipStreamSynchronize(t.stream));
        }
        HIP_TRY(hipStreamSynchronize(t.stream));
        return IVFADC_OK;
    };
    if (rc == IVFADC_OK) rc = body();
    (void)hipStreamSynchronize(t.stream);
    DevBuf *bufs[] = {&x, &resid, &cent, &cbs, &t.cdist, &t.assign, &t.mind, &t.partial, &t.acc, &t.counts, &t.flag, &t.blockmax};
    for (DevBuf *b : bufs) b->release();
    (void)hipStreamDestroy(t.stream);
    return rc;
}

}  // namespace

// =============================================================================================
extern "C" {

const char *ivfadc_last_error(void) { return g_err.c_str(); }

// ---- ivfadc_create: validate, then one step per operand family (the layouts themselves: pack_operands.h) --------------------------
struct CreateArgs {
    int d, kc, m, ksub;
    const float *centroids, *codebooks;
    const uint8_t *code_labels;   // one of code_labels (U = UInt8) and lab16 (U = UInt16) is given
    const uint16_t *lab16;
};

// `lm`: the handle's label map, made here (a duplicate label fails)
static int validate_create(const CreateArgs &a, list_mirror::LabelMap &lm)
{
    const int d = a.d, kc = a.kc, m = a.m, ksub = a.ksub;
    if (d < 1 || kc < 1 || m < 1 || ksub < 1) return fail(IVFADC_ERR_INVALID, "d, kc, m, ksub must be >= 1");
    if (m > d) return fail(IVFADC_ERR_ASSERT, "Number of codebooks has to be between 1 and %d", d);
    if (d % m != 0) return fail(IVFADC_ERR_INVALID, "d %% m != 0 is not supported (rowrange for ragged sub-spaces is unverifiable)");
    if (!a.lab16 && ksub > 256) return fail(IVFADC_ERR_INVALID, "ksub > 256 does not fit UInt8 codes");
    if (a.lab16 && ksub > 65536) return fail(IVFADC_ERR_INVALID, "ksub > 65536 does not fit UInt16 codes");
    if (!a.centroids || !a.codebooks || (!a.code_labels && !a.lab16)) return fail(IVFADC_ERR_INVALID, "null array");
    // Quantizers must be finite: every bound the filters certify (coarse score filter, lower-bound tables) is computed from their norms.
    // (Queries are not scanned -- that would cost the hot path a pass over every batch: a query with a NaN or infinite component gets
    // unspecified neighbours, valid ids and counts, and leaves the other queries of its batch untouched; tests/test_gpu_parity.py.)
    for (size_t i = 0; i < (size_t)d * kc; ++i)
        if (!std::isfinite(a.centroids[i])) return fail(IVFADC_ERR_INVALID, "centroid %zu has a non-finite component", i / (size_t)d);
    for (size_t i = 0; i < (size_t)d * ksub; ++i)
        if (!std::isfinite(a.codebooks[i])) return fail(IVFADC_ERR_INVALID, "codebook %zu has a non-finite component", i / ((size_t)(d / m) * ksub));
    return mirror_fail(a.lab16 ? lm.init16(a.lab16, m, ksub) : lm.init8(a.code_labels, m, ksub), a.lab16 != nullptr);
}

// the quantizers as given, the regrouped codebooks, the labels
static int create_quantizers(ivfadc_index *h, const CreateArgs &a)
{
    const int d = h->d, kc = h->kc, m = h->m, ksub = h->ksub, dsub = h->dsub;
    TRY(upload(h, h->centroids, a.centroids, (size_t)d * kc * 4));
    TRY(upload(h, h->codebooks, a.codebooks, (size_t)d * ksub * 4));
    // (a 16-bit handle keeps the plain layout: u16_scan_kernel reads it)
    TRY(upload(h, h->codebooks_t, pack::codebooks_t(a.codebooks, m, ksub, dsub, dsub == 6 && (m & 1) == 0 && !a.lab16)));
    if (m == 48 && dsub == 16) TRY(upload(h, h->codebooks_p, pack::codebooks_p(a.codebooks, m, ksub, dsub)));
    if (a.lab16) return upload(h, h->labels, a.lab16, (size_t)m * ksub * 2);
    TRY(upload(h, h->label_inv, pack::label_inverse(a.code_labels, m, ksub)));
    return upload(h, h->labels, a.code_labels, (size_t)m * ksub);
}

// what the filtering scans of 8-bit handles read: lower-bound operands (lbscan.hip.h), narrow-field operands (nfscan.hip.h)
static int create_filter_operands(ivfadc_index *h, const CreateArgs &a)
{
    const int m = h->m, ksub = h->ksub, dsub = h->dsub;
    if (a.lab16 || ksub != 256) return IVFADC_OK;
    if (lb_shape(m, dsub)) {
        const pack::LbOperands o = pack::lb_operands(a.codebooks, a.code_labels, m, ksub, dsub);
        TRY(upload(h, h->lb_f16, o.f16));
        TRY(upload(h, h->lb_isc, o.isc));
        TRY(upload(h, h->lb_split, o.split));
        TRY(upload(h, h->lb_n2, o.n2));
        TRY(upload(h, h->lb_lab, o.lab));
        TRY(upload(h, h->lb_maxn, o.maxn));
    }
    if (nf_shape(m, dsub)) {
        const pack::NfOperands o = pack::nf_operands(a.codebooks, a.code_labels, m, ksub, dsub);
        TRY(upload(h, h->nf_n2, o.n2));
        TRY(upload(h, h->nf_lab, o.lab));
    }
    return IVFADC_OK;
}

// what the coarse stage reads: norms, the latency path's regrouped copy, the bf16 and f16 forms of the matrix-core filter
static int create_coarse_operands(ivfadc_index *h, const CreateArgs &a)
{
    const int d = h->d, kc = h->kc;
    const pack::CentroidNorms cn = pack::centroid_norms(a.centroids, d, kc);
    h->cmaxn = cn.cmaxn;
    if ((d & 3) == 0 && (size_t)d * kc <= ((size_t)16 << 20)) TRY(upload(h, h->cent_t, pack::cent_t(a.centroids, d, kc)));
    if ((d & 3) == 0 && kc >= 2048) {
        const int dp = (d + 31) & ~31;
        h->dp32 = dp;
        const pack::CentroidF16 f = pack::centroid_f16(a.centroids, d, kc, dp);
        if (f.scale > 0.f) {
            TRY(upload(h, h->cent_f16, f.rows));
            h->f16_scale = f.scale;
        }
        const pack::CentroidBf16 b = pack::centroid_bf16(a.centroids, d, kc, dp);
        TRY(upload(h, h->cent_hi, b.hi));
        TRY(upload(h, h->cent_lo, b.lo));
    } else {
        h->allow_bf16 = false;
    }
    return upload(h, h->cnorm, cn.n2);
}

static int create_impl(ivfadc_t **out, int device, int d, int kc, int m, int ksub, const float *centroids, const float *codebooks,
                       const uint8_t *code_labels, const uint16_t *lab16)
{
    if (!out) return fail(IVFADC_ERR_INVALID, "out is null");
    *out = nullptr;
    const CreateArgs a{d, kc, m, ksub, centroids, codebooks, code_labels, lab16};
    list_mirror::LabelMap lm;
    TRY(validate_create(a, lm));
    int ndev = 0;
    HIP_TRY(hipGetDeviceCount(&ndev));
    if (ndev < 1) return fail(IVFADC_ERR_HIP, "no HIP device");
    if (device < 0 || device >= ndev) return fail(IVFADC_ERR_INVALID, "device %d out of range [0,%d)", device, ndev);
    struct Destroy { void operator()(ivfadc_index *p) const { ivfadc_destroy(p); } };
    std::unique_ptr<ivfadc_index, Destroy> h(new ivfadc_index());   // destroyed on every early return
    h->device = device;
    h->d = d; h->kc = kc; h->m = m; h->ksub = ksub; h->dsub = d / m;
    h->u16 = lab16 != nullptr;
    h->cb = h->u16 ? 2 * m : m;
    h->cs = code_stride(h->cb);
    h->labmap = std::move(lm);
    hipError_t e = hipSetDevice(device);
    if (e == hipSuccess) e = hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking);
    hipDeviceProp_t prop;
    if (e == hipSuccess) e = hipGetDeviceProperties(&prop, device);
    if (e != hipSuccess) return fail(IVFADC_ERR_HIP, "device init failed: %s", hipGetErrorString(e));
    h->num_cu = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
    TRY(create_quantizers(h.get(), a));
    TRY(create_filter_operands(h.get(), a));
    TRY(create_coarse_operands(h.get(), a));
    if (getenv("IVFADC_NO_PRUNE") != nullptr) h->allow_prune = false;
    h->allow_filt = getenv("IVFADC_EXACT_TABLES") == nullptr;
    h->allow_mfma = getenv("IVFADC_COARSE_EXACT") == nullptr;
    // an index starts with kc empty lists
    h->mirror.reset(kc);
    h->dirty = true;
    *out = h.release();
    return IVFADC_OK;
}


int ivfadc_create(ivfadc_t **out, int device, int d, int kc, int m, int ksub, const float *centroids, const float *codebooks,
                  const uint8_t *code_labels)
try {
    return create_impl(out, device, d, kc, m, ksub, centroids, codebooks, code_labels, nullptr);
} IVF_CATCH

int ivfadc_create_u16(ivfadc_t **out, int device, int d, int kc, int m, int ksub, const float *centroids, const float *codebooks,
                      const void *code_labels)
try {
    if (!code_labels) {
        if (out) *out = nullptr;
        return fail(IVFADC_ERR_INVALID, "null array");
    }
    return create_impl(out, device, d, kc, m, ksub, centroids, codebooks, nullptr, (const uint16_t *)code_labels);
} IVF_CATCH

int ivfadc_code_bits(ivfadc_t *h, int *bits)
try {
    HandleLock lk_(h);
    if (!h || !bits) return fail(IVFADC_ERR_INVALID, "null argument");
    *bits = h->u16 ? 16 : 8;
    return IVFADC_OK;
} IVF_CATCH

void ivfadc_destroy(ivfadc_t *h)
{
    if (!h) return;
    // (destroying a handle that another thread is still calling into is the caller's bug; what IS guarded is the topology: a view leaving
    // its index's list while a mutator of that index walks it, an index telling its views that it is gone)
    std::unique_lock<std::recursive_mutex> topo(g_topo_mu);
    h->mu.lock();
    h->mu.unlock();   // a call still running on this handle (a mutator holding a view's mutex) has finished
    (void)hipSetDevice(h->device);
    if (h->pipe_view) { ivfadc_destroy(h->pipe_view); h->pipe_view = nullptr; }
    if (h->fb_ev) { (void)hipEventSynchronize(h->fb_ev); (void)hipEventDestroy(h->fb_ev); }
    h->fb_pin.release();
    if (h->pipe_ev_in) (void)hipEventDestroy(h->pipe_ev_in);
    if (h->copy_stream) { (void)hipStreamSynchronize(h->copy_stream); (void)hipStreamDestroy(h->copy_stream); }
    for (hipEvent_t e : h->ingest_ev) (void)hipEventDestroy(e);
    // views that outlive the index keep dangling aliases: they are told, and refuse to search
    // (under each view's own mutex -- topology first, then the view, the order of every mutator: a view call reads its link and the
    // generation with nothing but its own mutex held)
    for (ivfadc_index *v : h->views) {
        std::lock_guard<std::recursive_mutex> vl(v->mu);
        v->orphan = true;
        v->view_of = nullptr;
    }
    if (h->is_view && h->view_of) {
        auto &vs = h->view_of->views;
        vs.erase(std::remove(vs.begin(), vs.end(), h), vs.end());
        h->view_of->n_views.store((int)vs.size());
    }
    if (h->stream) (void)hipStreamSynchronize(h->stream);
    if (h->comm || h->comm_stream) (void)ivfadc_comm_destroy(h);
    for (auto &ep : h->pending) { (void)hipEventDestroy(ep.a); (void)hipEventDestroy(ep.b); }
    for (auto &ep : h->free_ev) { (void)hipEventDestroy(ep.a); (void)hipEventDestroy(ep.b); }
    h->each_buf([](DevBuf &b) { b.release(); });
    h->pin_in.release();
    h->pin_out.release();
    if (h->stream && h->own_stream) (void)hipStreamDestroy(h->stream);
    delete h;
}

// ---- streams that really run side by side --------------------------------------------------------------------------------------
// The runtime maps the streams of a process onto a handful of hardware queues (GPU_MAX_HW_QUEUES, 4 by default): a new stream takes the
// queue with the fewest users, and two streams on one queue run their kernels one after the other.  Whether a view's stream lands beside
// its index's or behind it depends on what else the process has created -- measured in bench.py's process: ivfadc_search_batches 696 us
// per 16-batch call where a process with only the library's streams runs it in 615.  So a lane is PROBED when it is made: a 60 us spin
// kernel on each of the two streams; side by side they end after ~75 us, on one queue after 120 and more.  A stream that shares a queue
// with one it must overlap is replaced (the rejected ones are kept until the end, so the runtime hands out other queues) -- at most
// six tries, ~0.2 ms once per lane.  IVFADC_NO_STREAM_PROBE=1 skips it.
static int streams_serialised(hipStream_t a, hipStream_t b, bool &serial)
{
    serial = false;
    double best = 1e30;
    for (int rep = 0; rep < 2; ++rep) {
        HIP_TRY(hipStreamSynchronize(a));
        HIP_TRY(hipStreamSynchronize(b));
        const auto t0 = std::chrono::steady_clock::now();
        hipLaunchKernelGGL(spin_us_kernel, dim3(1), dim3(64), 0, a, 60u);
        hipLaunchKernelGGL(spin_us_kernel, dim3(1), dim3(64), 0, b, 60u);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipStreamSynchronize(a));
        HIP_TRY(hipStreamSynchronize(b));
        best = std::min(best, std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count());
    }
    serial = best > 105.0;
    return IVFADC_OK;
}

// *cand ends up on a hardware queue of its own with respect to every stream in fixed[] (as far as six tries reach)
static int ensure_overlap(const hipStream_t *fixed, int nfixed, hipStream_t *cand, int64_t *replaced)
{
    static const bool off = getenv("IVFADC_NO_STREAM_PROBE") != nullptr;
    if (off) return IVFADC_OK;
    std::vector<hipStream_t> rejected;
    int rc = IVFADC_OK;
    for (int attempt = 0; attempt < 6; ++attempt) {
        bool clash = false;
        for (int i = 0; i < nfixed && !clash && rc == IVFADC_OK; ++i) {
            if (!fixed[i] || fixed[i] == *cand) continue;
            rc = streams_serialised(fixed[i], *cand, clash);
        }
        if (rc != IVFADC_OK || !clash) break;
        hipStream_t next = nullptr;
        if (hipStreamCreateWithFlags(&next, hipStreamNonBlocking) != hipSuccess) { (void)hipGetLastError(); break; }
        rejected.push_back(*cand);
        *cand = next;
        if (replaced) ++*replaced;
    }
    for (hipStream_t s : rejected) (void)hipStreamDestroy(s);
    return rc;
}

// ---- views: clone_view (the index's lists, aliased) and clone_subset (lists of the view's own), from three shared steps ------------------
// what every view starts from: the index's device copy is current and at rest
static int view_source_ready(ivfadc_index *src, const char *of_a_view)
{
    if (src->is_view) return fail(IVFADC_ERR_STATE, "%s: take it from the index itself", of_a_view);
    TRY(set_device(src));
    if (src->dirty) TRY(upload_lists(src));   // the device copy is what the view shares (a subset view: reads)
    if (!src->have_lists) return fail(IVFADC_ERR_STATE, "no inverted lists set");
    HIP_TRY(hipStreamSynchronize(src->stream));   // uploads and in-place edits have landed
    return IVFADC_OK;
}

// everything a view is given except its lists
static void view_shell(ivfadc_index *src, ivfadc_index *v)
{
    static_cast<Dims &>(*v) = *src;
    static_cast<Quantizers &>(*v) = *src;
    v->Quantizers::each_buf([](DevBuf &b) { b.alias(); });
    static_cast<SearchConfig &>(*v) = *src;
    v->prune_est = src->prune_est;   // (a view has counters, snapshots and an event of its own; it starts from its index's estimate)
    v->fn_cfg = src->fn_cfg;         // what the index has already asked the runtime about its kernels holds for the view's launches
    // what the index's last coarse launch and partial search left behind has always come along
    v->tlist_ldq = src->tlist_ldq; v->tmin_tiles = src->tmin_tiles; v->tmin_tile_w = src->tmin_tile_w;
    v->last_coarse_f16 = src->last_coarse_f16; v->last_coarse_bf16 = src->last_coarse_bf16; v->last_listed = src->last_listed;
    v->partial_w = src->partial_w; v->partial_K = src->partial_K;
    v->is_view = true;
    v->view_of = src;
    v->view_gen = src->generation;
}

// the view's own stream, its place among the index's views, and out it goes
static int view_hand_out(ivfadc_index *src, std::unique_ptr<ivfadc_index> &v, ivfadc_index **out)
{
    const hipError_t e = hipStreamCreateWithFlags(&v->stream, hipStreamNonBlocking);
    if (e != hipSuccess) return fail(IVFADC_ERR_HIP, "hipStreamCreateWithFlags failed: %s", hipGetErrorString(e));
    // the point of a view is a second batch IN FLIGHT: its stream must not share a hardware queue with the index's
    {
        const hipStream_t fixed[1] = {src->stream};
        const int rc = ensure_overlap(fixed, 1, &v->stream, &src->hstats.streams_replaced);
        if (rc != IVFADC_OK) { (void)hipStreamDestroy(v->stream); return rc; }
    }
    {
        std::lock_guard<std::recursive_mutex> topo(g_topo_mu);
        src->views.push_back(v.get());
        src->n_views.fetch_add(1);
    }
    *out = v.release();
    return IVFADC_OK;
}

// A read-only view of `src`: the same device arrays (quantizers, derived tables, lists), a stream and a workspace of its own.
// The view is a fresh handle that is GIVEN what it shares: the shape, the quantizers and the device lists as aliases, the settings, and
// the few scalars view_shell names.  Its workspace and everything in HandleState start from their defaults; the host mirror is never touched.
static int clone_view(ivfadc_index *src, ivfadc_index **out)
{
    *out = nullptr;
    TRY(view_source_ready(src, "a view of a view"));
    std::unique_ptr<ivfadc_index> v(new ivfadc_index());   // (plain delete until it is handed out: it owns no device memory)
    view_shell(src, v.get());
    static_cast<Lists &>(*v) = *src;
    v->Lists::each_buf([](DevBuf &b) { b.alias(); });
    v->mirror.copy_lengths(src->mirror);
    return view_hand_out(src, v, out);
}

// ---- subset views (subset.hip.h, subset_plan.h; DESIGN.md "Subset views") -------------------------------------------------------------
// The view's OWN Lists group, filled from the index's device arrays: count per work item, one blocking copy of the counts, the layout
// every index gets (layout_from_caps: 256-byte aligned code blocks, the CODE_SLACK tail; capacity = length, a view never appends), a
// zeroed code buffer (alignment gaps and the tail are defined, as upload_lists' zeroed stage makes them), scatter.  Runs on the INDEX's
// stream, which is at rest (view_source_ready) and stays the caller's for the whole call (the index's lock is held); v->stream is lent
// that stream for the uploads and is given its own afterwards.  tmp: the call's scratch buffers, released by the caller on every path.
struct SubsetScratch {
    DevBuf bits, items, counts, bases;
    void release() { for (DevBuf *b : {&bits, &items, &counts, &bases}) b->release(); }
};

static int fill_subset_lists(ivfadc_index *src, ivfadc_index *v, const uint32_t *bits, bool bits_on_device, uint64_t nbits, SubsetScratch &tmp)
{
    const int kc = src->kc;
    hipStream_t s = src->stream;
    const std::vector<subset::Item> items = subset::make_items(src->mirror.h_len);
    std::vector<uint32_t> count(items.size(), 0), base;
    const uint32_t *d_bits = bits;
    const u32 *src_ids = src->synthetic ? (const u32 *)nullptr : src->ids.as<u32>();
    const bool scan = nbits > 0 && !items.empty();   // (nbits == 0: the empty subset, nothing to read)
    if (scan) {
        if (!bits_on_device) {
            const size_t words = (size_t)((nbits + 31) / 32);
            TRY(tmp.bits.ensure(words * 4));
            TRY(h2d_copy(tmp.bits.p, bits, words * 4, s));
            d_bits = tmp.bits.as<uint32_t>();
        }
        static_assert(sizeof(subset::Item) == 8, "the item list is uploaded as it is");
        TRY(tmp.items.ensure(items.size() * sizeof(subset::Item)));
        TRY(h2d_copy(tmp.items.p, items.data(), items.size() * sizeof(subset::Item), s));
        TRY(tmp.counts.ensure(items.size() * 4));
        hipLaunchKernelGGL(subset_count_kernel, dim3((unsigned)items.size()), dim3(256), 0, s, tmp.items.as<subset::Item>(),
                           src->list_pos.as<int64_t>(), src->list_len.as<u32>(), src_ids, d_bits, (uint64_t)nbits, tmp.counts.as<uint32_t>());
        HIP_TRY(hipGetLastError());
        TRY(d2h_copy(count.data(), tmp.counts.p, items.size() * 4, s));   // (blocking: the layout depends on it)
    }
    subset::make_bases(items, count, (size_t)kc, v->mirror.h_len, base);
    for (int l = 0; l < kc; ++l)
        if (v->mirror.h_len[l] > src->mirror.h_len[l]) return fail(IVFADC_ERR_HIP, "subset count of list %d exceeds the list", l);
    v->d_cap = v->mirror.h_len;
    list_mirror::LayoutTotals tot;
    TRY(layout_from_caps(v, tot));
    TRY(v->codes.alloc_exact(tot.code_bytes));
    TRY(v->ids.alloc_exact((size_t)std::max<int64_t>(1, tot.id_slots) * 4));
    HIP_TRY(hipMemsetAsync(v->codes.p, 0, tot.code_bytes, s));
    v->stream = s;
    const int rc = upload_list_tables(v);
    v->stream = nullptr;
    TRY(rc);
    if (v->mirror.n > 0) {
        TRY(tmp.bases.ensure(base.size() * 4));
        TRY(h2d_copy(tmp.bases.p, base.data(), base.size() * 4, s));
        hipLaunchKernelGGL(subset_scatter_kernel, dim3((unsigned)items.size()), dim3(256), 0, s, tmp.items.as<subset::Item>(),
                           src->list_pos.as<int64_t>(), src->list_len.as<u32>(), src->list_codeoff.as<int64_t>(), src_ids,
                           src->codes.as<uint8_t>(), d_bits, (uint64_t)nbits, tmp.bases.as<uint32_t>(), v->list_pos.as<int64_t>(),
                           v->list_codeoff.as<int64_t>(), v->ids.as<uint32_t>(), v->codes.as<uint8_t>(), v->cs / 4);
        HIP_TRY(hipGetLastError());
    }
    HIP_TRY(hipStreamSynchronize(s));
    v->have_lists = true;
    v->synthetic = false;   // (the kept entries of synthetic lists carry their ids like any others)
    v->dirty = false;
    return IVFADC_OK;
}

static int clone_subset(ivfadc_index *src, const uint32_t *bits, bool bits_on_device, uint64_t nbits, ivfadc_index **out, int64_t *out_n)
{
    *out = nullptr;
    TRY(view_source_ready(src, "a subset of a view"));
    std::unique_ptr<ivfadc_index> v(new ivfadc_index());
    view_shell(src, v.get());
    v->is_subset = true;
    SubsetScratch tmp;
    int rc = fill_subset_lists(src, v.get(), bits, bits_on_device, nbits, tmp);
    if (rc != IVFADC_OK) (void)hipStreamSynchronize(src->stream);   // nothing still reads the scratch
    tmp.release();
    const int64_t kept = v->mirror.n;
    ivfadc_index *raw = v.get();
    if (rc == IVFADC_OK) rc = view_hand_out(src, v, out);
    if (rc != IVFADC_OK) {   // (until it is handed out the view is deleted plainly: its lists go first)
        raw->Lists::each_buf([](DevBuf &b) { b.release(); });
        return rc;
    }
    if (out_n) *out_n = kept;
    return IVFADC_OK;
}

// settings that change how a search runs, copied to the internal second lane before every use
static void copy_search_config(ivfadc_index *dst, const ivfadc_index *src)
{
    static_cast<SearchConfig &>(*dst) = *src;
    dst->tl_use = src->tl_use && dst->tl_cent.p != nullptr;
}


int ivfadc_clone_view(ivfadc_t *h, ivfadc_t **out)
try {
    HandleLock lk_(h);
    if (!h || !out) return fail(IVFADC_ERR_INVALID, "null argument");
    return clone_view(h, out);
} IVF_CATCH

// the arguments of both subset entries, before the handle is looked at and before any device call
static int check_subset_args(ivfadc_t *h, const uint32_t *bits, uint64_t nbits, ivfadc_t **out)
{
    if (!out) return fail(IVFADC_ERR_INVALID, "ivfadc_clone_subset: null out_view");
    *out = nullptr;
    if (nbits > ((uint64_t)1 << 32)) return fail(IVFADC_ERR_INVALID, "ivfadc_clone_subset: nbits exceeds 2^32 (ids are UInt32)");
    if (nbits > 0 && !bits) return fail(IVFADC_ERR_INVALID, "ivfadc_clone_subset: null bitmap with nbits > 0");
    if (!h) return fail(IVFADC_ERR_INVALID, "ivfadc_clone_subset: null handle");
    return IVFADC_OK;
}

int ivfadc_clone_subset(ivfadc_t *h, const uint32_t *bits, uint64_t nbits, ivfadc_t **out_view, int64_t *out_n)
try {
    HandleLock lk_(h);
    TRY(check_subset_args(h, bits, nbits, out_view));
    return clone_subset(h, bits, false, nbits, out_view, out_n);
} IVF_CATCH

int ivfadc_clone_subset_device(ivfadc_t *h, const uint32_t *d_bits, uint64_t nbits, ivfadc_t **out_view, int64_t *out_n)
try {
    HandleLock lk_(h);
    TRY(check_subset_args(h, d_bits, nbits, out_view));
    return clone_subset(h, d_bits, true, nbits, out_view, out_n);
} IVF_CATCH

// ---- mask sets (maskset_plan.h, maskset.hip.h; DESIGN.md "Mask sets") -------------------------------------------------------------
static int search_enqueue(ivfadc_t *h, const SearchCall &hc);
static int search_finish(ivfadc_t *h, const SearchCall &hc);

// The way out of an entry once the device has been touched: whatever was enqueued before a failure may still be writing the staging
// buffers (or the caller's arrays) and ends first; the failure's message survives the drain.
static int finish_entry(ivfadc_index *h, int rc)
{
    if (rc != IVFADC_OK) {
        const std::string msg = g_err;
        if (h->stream && hipSetDevice(h->device) == hipSuccess) (void)hipStreamSynchronize(h->stream);
        g_err = msg;
    }
    return rc;
}
// the arguments of both creation entries, before the handle is looked at and before any device call
static int check_maskset_args(ivfadc_t *h, int nmasks, const uint32_t *bits, uint64_t nbits, ivfadc_maskset_t **out)
{
    if (!out) return fail(IVFADC_ERR_INVALID, "ivfadc_maskset_create: null out");
    *out = nullptr;
    if (nmasks < 1) return fail(IVFADC_ERR_INVALID, "ivfadc_maskset_create: nmasks = %d (at least one mask)", nmasks);
    if (nbits > ((uint64_t)1 << 32)) return fail(IVFADC_ERR_INVALID, "ivfadc_maskset_create: nbits exceeds 2^32 (ids are UInt32)");
    if (nbits > 0 && !bits) return fail(IVFADC_ERR_INVALID, "ivfadc_maskset_create: null bitmap with nbits > 0");
    if (!h) return fail(IVFADC_ERR_INVALID, "ivfadc_maskset_create: null handle");
    return IVFADC_OK;
}

// Runs on the index's stream, which is at rest (view_source_ready) and stays the caller's for the whole call (the index's lock is held).
static int maskset_fill(ivfadc_index *src, ivfadc_maskset *ms, int nmasks, const uint32_t *bits, bool bits_on_device, uint64_t nbits,
                        int64_t *out_kept, SubsetScratch &tmp)
{
    hipStream_t s = src->stream;
    const maskset::Layout lay = maskset::make_layout(src->mirror.h_len);
    ms->device = src->device;
    ms->nmasks = nmasks;
    ms->kc = src->kc;
    ms->W = lay.W;
    ms->index_serial = src->serial;
    ms->generation = src->generation;
    const size_t nwords = (size_t)nmasks * (size_t)lay.W;
    TRY(ms->words.alloc_exact(std::max<size_t>(8, nwords * 4)));
    TRY(ms->word_off.alloc_exact(lay.word_off.size() * 8));
    TRY(h2d_copy(ms->word_off.p, lay.word_off.data(), lay.word_off.size() * 8, s));
    const std::vector<subset::Item> items = subset::make_items(src->mirror.h_len);
    std::vector<unsigned long long> kept((size_t)nmasks, 0ull);
    if (!items.empty()) {
        const size_t stride = (size_t)((nbits + 31) / 32);
        const uint32_t *d_bits = bits;
        if (!bits_on_device && nbits > 0) {
            TRY(tmp.bits.ensure((size_t)nmasks * stride * 4));
            TRY(h2d_copy(tmp.bits.p, bits, (size_t)nmasks * stride * 4, s));
            d_bits = tmp.bits.as<uint32_t>();
        }
        TRY(tmp.items.ensure(items.size() * sizeof(subset::Item)));
        TRY(h2d_copy(tmp.items.p, items.data(), items.size() * sizeof(subset::Item), s));
        TRY(tmp.counts.ensure((size_t)nmasks * 8));
        HIP_TRY(hipMemsetAsync(tmp.counts.p, 0, (size_t)nmasks * 8, s));
        hipLaunchKernelGGL(maskset_build_kernel, dim3((unsigned)items.size()), dim3(256), 0, s, tmp.items.as<subset::Item>(),
                           src->list_pos.as<int64_t>(), src->list_len.as<u32>(), src->synthetic ? (const u32 *)nullptr : src->ids.as<u32>(), d_bits,
                           (uint64_t)nbits, (uint64_t)stride, nmasks, ms->word_off.as<uint64_t>(), (uint64_t)lay.W, ms->words.as<uint32_t>(),
                           out_kept ? tmp.counts.as<unsigned long long>() : (unsigned long long *)nullptr);
        HIP_TRY(hipGetLastError());
        if (out_kept) TRY(d2h_copy(kept.data(), tmp.counts.p, (size_t)nmasks * 8, s));
    }
    HIP_TRY(hipStreamSynchronize(s));
    if (out_kept)
        for (int r = 0; r < nmasks; ++r) out_kept[r] = (int64_t)kept[(size_t)r];
    return IVFADC_OK;
}

static int maskset_create(ivfadc_index *src, int nmasks, const uint32_t *bits, bool bits_on_device, uint64_t nbits, ivfadc_maskset_t **out,
                          int64_t *out_kept)
{
    TRY(view_source_ready(src, "a mask set of a view"));
    std::unique_ptr<ivfadc_maskset> ms(new ivfadc_maskset());
    SubsetScratch tmp;
    const int rc = maskset_fill(src, ms.get(), nmasks, bits, bits_on_device, nbits, out_kept, tmp);
    if (rc != IVFADC_OK) (void)hipStreamSynchronize(src->stream);   // nothing still reads the scratch
    tmp.release();
    if (rc != IVFADC_OK) {
        ms->words.release();
        ms->word_off.release();
        return rc;
    }
    *out = ms.release();
    return IVFADC_OK;
}

int ivfadc_maskset_create(ivfadc_t *h, int nmasks, const uint32_t *bits, uint64_t nbits, ivfadc_maskset_t **out, int64_t *out_kept)
try {
    HandleLock lk_(h);
    TRY(check_maskset_args(h, nmasks, bits, nbits, out));
    return maskset_create(h, nmasks, bits, false, nbits, out, out_kept);
} IVF_CATCH

int ivfadc_maskset_create_device(ivfadc_t *h, int nmasks, const uint32_t *d_bits, uint64_t nbits, ivfadc_maskset_t **out, int64_t *out_kept)
try {
    HandleLock lk_(h);
    TRY(check_maskset_args(h, nmasks, d_bits, nbits, out));
    return maskset_create(h, nmasks, d_bits, true, nbits, out, out_kept);
} IVF_CATCH

void ivfadc_maskset_destroy(ivfadc_maskset_t *s)
{
    if (!s) return;
    if (hipSetDevice(s->device) == hipSuccess) {
        s->words.release();
        s->word_off.release();
    }
    delete s;
}

// h and s of a masked entry (entry: its name): h is the index s was made from, unchanged since, or a plain view of it
static int check_mask_link(const ivfadc_index *h, const ivfadc_maskset *s, const char *entry)
{
    if (h->is_subset) return fail(IVFADC_ERR_STATE, "%s: a subset view has lists of its own; search the index the mask set was made from, or a plain view of it", entry);
    const ivfadc_index *root = h->is_view ? h->view_of : h;   // (check_view_current: the link stands)
    if (root->serial != s->index_serial) return fail(IVFADC_ERR_STATE, "%s: the mask set was made from another index", entry);
    if (root->generation != s->generation) return fail(IVFADC_ERR_STATE, "%s: the index has changed since the mask set was made: make a new one", entry);
    return IVFADC_OK;
}

// the mask numbers of a host entry, before any launch (null: every query takes mask 0)
static int check_mask_numbers(const ivfadc_maskset *s, int64_t nq, const int32_t *mask_of_query)
{
    for (int64_t q = 0; mask_of_query && q < nq; ++q)
        if (mask_of_query[q] < -1 || mask_of_query[q] >= s->nmasks)
            return fail(IVFADC_ERR_INVALID, "query %lld: mask %d is outside [-1, %d)", (long long)q, mask_of_query[q], s->nmasks);
    return IVFADC_OK;
}

// The set and the mask numbers of c's queries into the call, the numbers staged in mask_q on the handle's stream: from host memory a copy
// (zeros when there are none), from device memory clamped into [-1, nmasks), so that a violated precondition cannot read outside the set.
static int stage_mask_numbers(ivfadc_index *h, const ivfadc_maskset *s, const int32_t *mask_of_query, bool on_device, SearchCall &c)
{
    const size_t bytes = (size_t)c.nq * 4;
    TRY(h->mask_q.ensure(std::max<size_t>(bytes, 16)));
    if (c.nq > 0 && on_device) {
        hipLaunchKernelGGL(maskset_ingest_kernel, dim3((unsigned)std::min<int64_t>(4096, (c.nq + 255) / 256)), dim3(256), 0, h->stream, mask_of_query,
                           c.nq, (int32_t)s->nmasks, h->mask_q.as<int32_t>());
        HIP_TRY(hipGetLastError());
    } else if (c.nq > 0 && mask_of_query) {
        TRY(h2d_copy(h->mask_q.p, mask_of_query, bytes, h->stream));
    } else if (c.nq > 0) {
        HIP_TRY(hipMemsetAsync(h->mask_q.p, 0, bytes, h->stream));
    }
    c.mask_words = s->words.as<u32>(); c.mask_word_off = s->word_off.as<uint64_t>(); c.mask_W = s->W;
    c.mask_of_query = h->mask_q.as<int32_t>();
    return IVFADC_OK;
}

// Both masked K-nearest entries.  c: the call as the entry got it; host: everything the caller gave lies in host memory.
static int search_masked_entry(ivfadc_index *h, const ivfadc_maskset *s, SearchCall c, const int32_t *mask_of_query, bool host)
{
    if (!h) return fail(IVFADC_ERR_INVALID, "null handle");
    if (!s) return fail(IVFADC_ERR_INVALID, "null mask set");
    TRY(check_search_args(h, c.nq, c.K, c.w));
    TRY(check_mask_link(h, s, "ivfadc_search_masked"));
    if (h->part_n > 1) return fail(IVFADC_ERR_STATE, "a list partition is set (ivfadc_set_list_partition): masked searches serve whole indexes only");
    if (c.nq == 0) return IVFADC_OK;
    if (!c.q || !c.ids || !c.dists || !c.counts) return fail(IVFADC_ERR_INVALID, "null buffer");
    if (host) TRY(check_mask_numbers(s, c.nq, mask_of_query));
    TRY(set_device(h));
    h->dev_entry = false;
    c.d = h->d;
    int rc = stage_mask_numbers(h, s, mask_of_query, !host, c);
    if (rc == IVFADC_OK) rc = host ? search_enqueue(h, c) : search_dev(h, c);
    return rc != IVFADC_OK || !host ? finish_entry(h, rc) : search_finish(h, c);
}

int ivfadc_search_device_masked(ivfadc_t *h, const ivfadc_maskset_t *s, int64_t nq, const float *d_queries, int K, int w,
                                const int32_t *d_mask_of_query, uint32_t *d_out_ids, float *d_out_dists, int32_t *d_out_counts)
try {
    HandleLock lk_(h);
    return search_masked_entry(h, s, SearchCall{nq, 0, K, w, d_queries, d_out_ids, d_out_dists, d_out_counts}, d_mask_of_query, false);
} IVF_CATCH

int ivfadc_search_masked(ivfadc_t *h, const ivfadc_maskset_t *s, int64_t nq, const float *queries, int K, int w, const int32_t *mask_of_query,
                         uint32_t *out_ids, float *out_dists, int32_t *out_counts)
try {
    HandleLock lk_(h);
    return search_masked_entry(h, s, SearchCall{nq, 0, K, w, queries, out_ids, out_dists, out_counts}, mask_of_query, true);
} IVF_CATCH

// a 16-bit handle refuses the uint8_t entries, an 8-bit handle the _u16 ones
static int check_width(ivfadc_index *h, bool want_u16, const char *what)
{
    if (h->u16 && !want_u16) return fail(IVFADC_ERR_STATE, "%s: this index has UInt16 codes; use %s_u16", what, what);
    if (!h->u16 && want_u16) return fail(IVFADC_ERR_STATE, "%s: this index has UInt8 codes; use the entry without _u16", what);
    return IVFADC_OK;
}

// ---- the write side: one body per entry pair ----------------------------------------------------------------------------------------------
// A body takes the width it serves (wide: the _u16 entry).  check_width is the first difference between the twins, the label conversion
// at the boundary (list_mirror::LabelMap) the only other.  Every edit of the mirror is list_mirror.h's; what stays here is the order of
// the checks, the MutationScope, the StaleGuard and the device's half of each edit.

// mirror <- (offsets that passed check_offsets, codes in mirror form, ids), then the device copy: both set_lists entries and the loader
static int assign_lists(ivfadc_index *h, const int64_t *offsets, const uint8_t *codes, const uint32_t *ids, const char *what)
{
    TRY(set_device(h));
    MutationScope ms;
    TRY(ms.begin(h, what));
    StaleGuard stale(h);
    h->mirror.assign(offsets, codes, ids, h->cb);
    return upload_lists(h);   // (declares the copy current)
}

static int set_lists_entry(ivfadc_index *h, const int64_t *offsets, const void *codes, const uint32_t *ids, bool wide)
{
    if (!h || !offsets) return fail(IVFADC_ERR_INVALID, "null argument");
    TRY(check_width(h, wide, "ivfadc_set_lists"));
    const char *what = wide ? "ivfadc_set_lists_u16" : "ivfadc_set_lists";
    TRY(check_mutable(h, what));
    TRY(mirror_fail(list_mirror::ListMirror::check_offsets(h->kc, offsets, codes, ids), wide));
    const int64_t n = offsets[h->kc];
    if (!wide) {
        TRY(mirror_fail(h->labmap.check8(n, (const uint8_t *)codes), false));
        return assign_lists(h, offsets, (const uint8_t *)codes, ids, what);
    }
    std::vector<uint8_t> idx;
    TRY(mirror_fail(h->labmap.to_indices(n, (const uint16_t *)codes, idx), true));
    return assign_lists(h, offsets, idx.data(), ids, what);
}

int ivfadc_set_lists(ivfadc_t *h, const int64_t *offsets, const uint8_t *codes, const uint32_t *ids)
try {
    HandleLock lk_(h);
    return set_lists_entry(h, offsets, codes, ids, false);
} IVF_CATCH

int ivfadc_set_lists_u16(ivfadc_t *h, const int64_t *offsets, const void *codes, const uint32_t *ids)
try {
    HandleLock lk_(h);
    return set_lists_entry(h, offsets, codes, ids, true);
} IVF_CATCH

int ivfadc_synth_lists(ivfadc_t *h, const int64_t *offsets, uint64_t seed)
try {
    HandleLock lk_(h);
    if (!h || !offsets) return fail(IVFADC_ERR_INVALID, "null argument");
    TRY(check_width(h, false, "ivfadc_synth_lists"));
    TRY(check_mutable(h, "ivfadc_synth_lists"));
    if (h->ksub != 256) return fail(IVFADC_ERR_INVALID, "synthetic lists need ksub == 256");
    TRY(set_device(h));
    std::vector<uint8_t> lab((size_t)h->m * 256);
    HIP_TRY(hipMemcpy(lab.data(), h->labels.p, lab.size(), hipMemcpyDeviceToHost));
    for (size_t i = 0; i < lab.size(); ++i)
        if (lab[i] != (uint8_t)(i & 255)) return fail(IVFADC_ERR_INVALID, "synthetic lists need identity labels");
    const int kc = h->kc;
    for (int l = 0; l < kc; ++l)
        if (offsets[l + 1] < offsets[l]) return fail(IVFADC_ERR_INVALID, "offsets must be non-decreasing (list %d)", l);
    MutationScope ms;
    TRY(ms.begin(h, "ivfadc_synth_lists"));
    // no spare capacity: the id of a point is its canonical global position (ids == nullptr in the kernels)
    h->mirror.assign_lengths(offsets);
    h->d_cap = h->mirror.h_len;
    list_mirror::LayoutTotals tot;
    TRY(layout_from_caps(h, tot));
    TRY(h->codes.ensure(tot.code_bytes));
    TRY(upload_list_tables(h));
    HIP_TRY(hipMemsetAsync((uint8_t *)h->codes.p + (tot.code_bytes - CODE_SLACK), 0, CODE_SLACK, h->stream));
    const int64_t maxdw = h->mirror.maxlen * (h->cs / 4);
    const unsigned gy = (unsigned)std::max<int64_t>(1, std::min<int64_t>(1024, (maxdw + 256 * 8 - 1) / (256 * 8)));
    hipLaunchKernelGGL(synth_codes_kernel, dim3((unsigned)kc, gy), dim3(256), 0, h->stream, h->codes.as<uint8_t>(),
                       h->list_pos.as<int64_t>(), h->list_len.as<u32>(), h->list_codeoff.as<int64_t>(), kc, h->m, h->cs, (u64)seed);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(h->stream));
    h->have_lists = true;
    h->synthetic = true;
    h->dirty = false;   // (no StaleGuard: there is no mirror data a re-layout could be made from)
    return IVFADC_OK;
} IVF_CATCH

// The twins have always looked at the width at different places, and callers may rely on either: the 8-bit entry takes n == 0 from any
// handle and names a null argument before the width; the _u16 entry looks at the width first.
static int encode_entry(ivfadc_index *h, int64_t n, const float *pts, int32_t *out_list, void *out_codes, bool wide)
{
    if (!h) return fail(IVFADC_ERR_INVALID, "null handle");
    if (n < 0) return fail(IVFADC_ERR_INVALID, "n < 0");
    if (wide) TRY(check_width(h, true, "ivfadc_encode"));
    if (n == 0) return IVFADC_OK;
    if (!pts || !out_list || !out_codes) return fail(IVFADC_ERR_INVALID, "null argument");
    if (!wide) TRY(check_width(h, false, "ivfadc_encode"));
    if (!h->rot.empty())
        return fail(IVFADC_ERR_STATE, "ivfadc_encode%s: the residual quantizer carries a rotation (:opq); this index is served for search only", wide ? "_u16" : "");
    TRY(set_device(h));
    TRY(encode_dev(h, n, pts, out_list, (uint8_t *)out_codes));
    if (wide) h->labmap.to_labels(n, out_codes);
    return IVFADC_OK;
}

int ivfadc_encode(ivfadc_t *h, int64_t n, const float *pts, int32_t *out_list, uint8_t *out_codes)
try {
    HandleLock lk_(h);
    return encode_entry(h, n, pts, out_list, out_codes, false);
} IVF_CATCH

int ivfadc_encode_u16(ivfadc_t *h, int64_t n, const float *pts, int32_t *out_list, void *out_codes)
try {
    HandleLock lk_(h);
    return encode_entry(h, n, pts, out_list, out_codes, true);
} IVF_CATCH

// push! behind the encoder: `lst` / `cod` are the (already computed) assignment and codes (mirror form) of the new points.  In place when
// the device layout is current and every target list has room; otherwise the host mirror takes the points and the next search re-lays the
// lists out with fresh spare capacity.
static int append_encoded(ivfadc_t *h, int64_t nnew, const int32_t *lst, const uint8_t *cod, const uint32_t *ids)
{
    const int cb = h->cb;
    MutationScope ms;
    TRY(ms.begin(h, "ivfadc_append"));
    TRY(set_device(h));
    StaleGuard stale(h);
    std::vector<int64_t> dst;
    if (!h->mirror.append(nnew, lst, cod, ids, cb, stale.in_place() ? h : nullptr, h->cs, dst)) return IVFADC_OK;
    const size_t o_ids = (size_t)nnew * 16, o_codes = o_ids + align_up((size_t)nnew * 4, 16);
    const size_t bytes = o_codes + (size_t)nnew * cb;
    std::vector<uint8_t> stage(bytes);
    memcpy(stage.data(), dst.data(), (size_t)nnew * 16);
    memcpy(stage.data() + o_ids, ids, (size_t)nnew * 4);
    memcpy(stage.data() + o_codes, cod, (size_t)nnew * cb);
    TRY(h->app_stage.ensure(bytes));
    TRY(h2d_copy(h->app_stage.p, stage.data(), bytes, h->stream));
    const uint8_t *base = (const uint8_t *)h->app_stage.p;
    hipLaunchKernelGGL(append_scatter_kernel, dim3((unsigned)((nnew + 255) / 256)), dim3(256), 0, h->stream, nnew, cb,
                       (const int64_t *)base, base + o_codes, (const u32 *)(base + o_ids), h->codes.as<uint8_t>(), h->ids.as<u32>());
    HIP_TRY(hipGetLastError());
    // lengths: only the touched lists change, but kc u32 is a single small copy
    std::vector<uint32_t> len32((size_t)h->kc);
    for (int l = 0; l < h->kc; ++l) len32[l] = (uint32_t)h->mirror.h_len[l];
    TRY(h2d_copy(h->list_len.p, len32.data(), (size_t)h->kc * 4, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));   // staging vectors are stack-owned
    h->inplace_appends++;
    stale.current();
    return IVFADC_OK;
}

static int append_check(ivfadc_t *h, int64_t nnew, const float *pts, const uint32_t *ids)
{
    if (!h) return fail(IVFADC_ERR_INVALID, "null handle");
    if (h->synthetic) return fail(IVFADC_ERR_STATE, "append is not available on device-synthesised lists");
    if (nnew < 0) return fail(IVFADC_ERR_INVALID, "nnew < 0");
    if (nnew > 0 && (!pts || !ids)) return fail(IVFADC_ERR_INVALID, "null argument");
    if (h->mirror.ntotal() + nnew > list_mirror::ID_LIMIT) return fail(IVFADC_ERR_ASSERT, "Cannot index, exceeding index capacity of UInt32");
    return IVFADC_OK;
}

// (width before mutability, as the _u16 entry has always had it: both refusals are IVFADC_ERR_STATE)
static int append_entry(ivfadc_index *h, int64_t nnew, const float *pts, const uint32_t *ids, int32_t *out_list, void *out_codes, bool wide)
{
    const char *what = wide ? "ivfadc_append_u16" : "ivfadc_append";
    TRY(append_check(h, nnew, pts, ids));
    TRY(check_width(h, wide, "ivfadc_append"));
    TRY(check_mutable(h, what));
    if (!h->rot.empty()) return fail(IVFADC_ERR_STATE, "%s: the residual quantizer carries a rotation (:opq); this index is served for search only", what);
    if (nnew == 0) return IVFADC_OK;
    TRY(set_device(h));
    std::vector<int32_t> lst((size_t)nnew);
    std::vector<uint8_t> cod((size_t)nnew * h->cb);
    TRY(encode_dev(h, nnew, pts, lst.data(), cod.data()));   // (a 16-bit handle: codeword indices) nothing has changed yet if this fails
    TRY(append_encoded(h, nnew, lst.data(), cod.data(), ids));
    if (out_list) memcpy(out_list, lst.data(), (size_t)nnew * 4);
    if (out_codes) {
        memcpy(out_codes, cod.data(), cod.size());
        if (wide) h->labmap.to_labels(nnew, out_codes);
    }
    return IVFADC_OK;
}

int ivfadc_append(ivfadc_t *h, int64_t nnew, const float *pts, const uint32_t *ids, int32_t *out_list, uint8_t *out_codes)
try {
    HandleLock lk_(h);
    return append_entry(h, nnew, pts, ids, out_list, out_codes, false);
} IVF_CATCH

int ivfadc_append_u16(ivfadc_t *h, int64_t nnew, const float *pts, const uint32_t *ids, int32_t *out_list, void *out_codes)
try {
    HandleLock lk_(h);
    return append_entry(h, nnew, pts, ids, out_list, out_codes, true);
} IVF_CATCH

int ivfadc_delete_ids(ivfadc_t *h, int64_t ndel, const uint32_t *del_ids, int64_t *out_removed)
try {
    HandleLock lk_(h);
    if (!h) return fail(IVFADC_ERR_INVALID, "null handle");
    TRY(check_mutable(h, "ivfadc_delete_ids"));
    if (h->synthetic) return fail(IVFADC_ERR_STATE, "delete is not available on device-synthesised lists");
    if (ndel < 0 || (ndel > 0 && !del_ids)) return fail(IVFADC_ERR_INVALID, "bad argument");
    if (out_removed) *out_removed = 0;
    if (ndel == 0) return IVFADC_OK;
    TRY(set_device(h));
    // the ids that are really there, found without touching the mirror: nothing has changed yet if the scope cannot be opened
    const std::vector<uint32_t> rem = h->mirror.find_ids(ndel, del_ids);
    if (rem.empty()) return IVFADC_OK;   // nothing was stored under these ids: mirror unchanged, views stay valid
    MutationScope ms;
    TRY(ms.begin(h, "ivfadc_delete_ids"));
    StaleGuard stale(h);
    h->mirror.erase_ids(rem, h->cb);
    if (out_removed) *out_removed = (int64_t)rem.size();
    // device copy: the same compaction in place, one workgroup per list
    if (stale.in_place()) {
        TRY(h->app_stage.ensure(rem.size() * 4));
        TRY(h2d_copy(h->app_stage.p, rem.data(), rem.size() * 4, h->stream));
        hipLaunchKernelGGL(delete_compact_kernel, dim3((unsigned)h->kc), dim3(256), 0, h->stream, h->app_stage.as<u32>(), (u32)rem.size(),
                           h->list_pos.as<int64_t>(), h->list_codeoff.as<int64_t>(), h->list_len.as<u32>(), h->codes.as<uint8_t>(),
                           h->ids.as<u32>(), h->cs);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipStreamSynchronize(h->stream));   // rem is stack-owned
        stale.current();
    }
    return IVFADC_OK;
} IVF_CATCH

int ivfadc_shift_ids(ivfadc_t *h, int32_t delta)
try {
    HandleLock lk_(h);
    if (!h) return fail(IVFADC_ERR_INVALID, "null handle");
    TRY(check_mutable(h, "ivfadc_shift_ids"));
    if (h->synthetic) return fail(IVFADC_ERR_STATE, "not available on device-synthesised lists");
    if (delta == 0) return IVFADC_OK;
    TRY(set_device(h));
    MutationScope ms;
    TRY(ms.begin(h, "ivfadc_shift_ids"));
    StaleGuard stale(h);
    h->mirror.shift_ids((uint32_t)delta);
    if (stale.in_place()) {
        int64_t slots = 0;
        for (int l = 0; l < h->kc; ++l) slots += h->d_cap[l];
        if (slots > 0) {
            hipLaunchKernelGGL(shift_ids_kernel, dim3((unsigned)std::min<int64_t>(4096, (slots + 255) / 256)), dim3(256), 0, h->stream,
                               h->ids.as<u32>(), slots, (u32)delta);
            HIP_TRY(hipGetLastError());
        }
        stale.current();
    }
    return IVFADC_OK;
} IVF_CATCH

int ivfadc_search_device(ivfadc_t *h, int64_t nq, const float *d_queries, int K, int w, uint32_t *d_out_ids, float *d_out_dists,
                         int32_t *d_out_counts)
try {
    HandleLock lk_(h);
    TRY(check_search_args(h, nq, K, w));
    if (nq > 0 && (!d_queries || !d_out_ids || !d_out_dists || !d_out_counts)) return fail(IVFADC_ERR_INVALID, "null buffer");
    {
        // are several lanes of this replica in use side by side?  Every device-entry search takes a ticket from the root index; a handle
        // whose two consecutive tickets are more than one apart has had a neighbour search in between
        ivfadc_index *root = (h->is_view && h->view_of) ? h->view_of : h;
        const int t = root->lane_ticket.fetch_add_get(1);
        h->dev_entry = h->my_ticket >= 0 && t - h->my_ticket > 1;
        h->my_ticket = t;
    }
    struct Reset { ivfadc_index *h; ~Reset() { h->dev_entry = false; } } reset_{h};   // (also when an exception unwinds into IVF_CATCH)
    return search_dev(h, SearchCall{nq, h->d, K, w, d_queries, d_out_ids, d_out_dists, d_out_counts});
} IVF_CATCH

// ---- locate / reconstruct (reconstruct_plan.h, reconstruct.hip.h) ----------------------------------------------------
// "What is stored under this id": the reference's _pop! loop (utils.jl:49-55) and centre + _decode_point (utils.jl:58-59, 71-81) for a batch
// of ids, on the device copy of the lists -- no host mirror involved, so every handle that can be searched is served.

// the arguments of the four entries, before the handle is looked at and before any device call
static int check_recon_args(const char *fn, ivfadc_t *h, int64_t n, const uint32_t *ids, const void *out_a, const char *name_a, const void *out_b,
                            const char *name_b)
{
    if (!h) return fail(IVFADC_ERR_INVALID, "%s: null handle", fn);
    if (n < 0) return fail(IVFADC_ERR_INVALID, "%s: n = %lld < 0", fn, (long long)n);
    if (n > 0 && !ids) return fail(IVFADC_ERR_INVALID, "%s: null ids with n > 0", fn);
    if (!out_a) return fail(IVFADC_ERR_INVALID, "%s: null %s", fn, name_a);
    if (name_b && !out_b) return fail(IVFADC_ERR_INVALID, "%s: null %s", fn, name_b);
    return IVFADC_OK;
}

// the handle's state: a current view, lists, no list partition; pending list changes are laid out first, as a search does
static int recon_begin(ivfadc_index *h, const char *fn)
{
    TRY(check_view_current(h));
    if (!h->have_lists && !h->dirty) return fail(IVFADC_ERR_STATE, "no inverted lists set");
    if (h->part_n > 1) return fail(IVFADC_ERR_STATE, "%s: not served in the list-partitioned mode", fn);
    TRY(set_device(h));
    if (h->dirty) TRY(upload_lists(h));
    return IVFADC_OK;
}

// the way out of the four entries once the device has been touched: finish_entry's drain on failure
static int recon_exit(ivfadc_index *x, int rc) { return finish_entry(x, rc); }

// d_want: nwant wanted ids in device memory, ascending as unsigned numbers (repeats allowed) -> h->rc_best: one key per slot
static int locate_sorted(ivfadc_index *h, const uint32_t *d_want, uint64_t nwant, bool span_known, uint32_t want_lo, uint32_t want_hi)
{
    hipStream_t s = h->stream;
    TRY(h->rc_best.ensure(std::max<size_t>(8, (size_t)nwant * 8)));
    HIP_TRY(hipMemsetAsync(h->rc_best.p, 0, std::max<size_t>(8, (size_t)nwant * 8), s));
    uint64_t items = 0;
    for (int64_t len : h->mirror.h_len) items += recon::list_chunks((uint64_t)std::max<int64_t>(len, 0));
    const recon::Plan pl = recon::make_plan(nwant, span_known, want_lo, want_hi, items, (uint64_t)h->mirror.ntotal(), h->num_cu);
    if (pl.mode == recon::MODE_NONE) return IVFADC_OK;
    // the work items' prefix, from the device's own list_len (== h_len once pending changes are laid out): nothing is uploaded, nothing waited for
    TRY(h->rc_chunk.ensure(((size_t)h->kc + 1) * 8));
    hipLaunchKernelGGL(recon_chunk_prefix_kernel, dim3(1), dim3(256), 0, s, h->list_len.as<u32>(), (u32)h->kc, h->rc_chunk.as<uint64_t>());
    HIP_TRY(hipGetLastError());
    const u32 *ids = h->synthetic ? (const u32 *)nullptr : h->ids.as<u32>();
    if (pl.mode == recon::MODE_BITMAP) {
        TRY(h->rc_bitmap.ensure((size_t)pl.words * 4));
        if (pl.span_from_want) {
            hipLaunchKernelGGL(recon_bitmap_zero_kernel, dim3(2048), dim3(256), 0, s, d_want, nwant, h->rc_bitmap.as<u32>());
            HIP_TRY(hipGetLastError());
        } else {
            HIP_TRY(hipMemsetAsync(h->rc_bitmap.p, 0, (size_t)pl.words * 4, s));
        }
        const unsigned fill_grid = (unsigned)std::min<uint64_t>(2048, (nwant + 255) / 256);
        hipLaunchKernelGGL(recon_bitmap_fill_kernel, dim3(fill_grid), dim3(256), 0, s, d_want, nwant, pl.lo, pl.nbits, pl.span_from_want,
                           h->rc_bitmap.as<u32>());
        HIP_TRY(hipGetLastError());
        hipLaunchKernelGGL(recon_locate_kernel<false>, dim3(pl.grid), dim3(256), 0, s, h->rc_chunk.as<uint64_t>(), (u32)h->kc, items,
                           h->list_pos.as<int64_t>(), h->list_len.as<u32>(), ids, d_want, nwant, pl.lo, pl.nbits, pl.span_from_want,
                           h->rc_bitmap.as<u32>(), h->rc_best.as<unsigned long long>());
        HIP_TRY(hipGetLastError());
        return IVFADC_OK;
    }
    hipLaunchKernelGGL(recon_locate_kernel<true>, dim3(pl.grid), dim3(256), 0, s, h->rc_chunk.as<uint64_t>(), (u32)h->kc, items,
                       h->list_pos.as<int64_t>(), h->list_len.as<u32>(), ids, d_want, nwant, 0u, (uint64_t)0, false, (const u32 *)nullptr,
                       h->rc_best.as<unsigned long long>());
    HIP_TRY(hipGetLastError());
    return IVFADC_OK;
}

// request order: d_req (n ids, device) against the sorted wanted ids and their keys -> list, position, found (device; any may be null)
static int recon_resolve(ivfadc_index *h, const uint32_t *d_req, int64_t n, const uint32_t *d_want, uint64_t nwant, int32_t *d_list,
                         int64_t *d_pos, uint8_t *d_found)
{
    const unsigned grid = (unsigned)std::min<int64_t>(2048, (n + 255) / 256);
    hipLaunchKernelGGL(recon_resolve_kernel, dim3(grid), dim3(256), 0, h->stream, d_req, n, d_want, nwant, h->rc_best.as<unsigned long long>(),
                       d_list, d_pos, d_found);
    HIP_TRY(hipGetLastError());
    return IVFADC_OK;
}

static int recon_decode(ivfadc_index *h, int64_t n, const int32_t *d_list, const int64_t *d_pos, float *d_out)
{
    DecodeArgs a{};
    a.centroids = h->centroids.as<float>();
    a.codebooks = h->codebooks.as<float>();
    a.label_inv = h->u16 ? (const uint8_t *)nullptr : h->label_inv.as<uint8_t>();
    a.codes = h->codes.as<uint8_t>();
    a.list_codeoff = h->list_codeoff.as<int64_t>();
    a.d = h->d; a.m = h->m; a.dsub = h->dsub; a.ksub = h->ksub; a.cs = h->cs;
    if (!h->u16 && !a.label_inv) return fail(IVFADC_ERR_STATE, "the handle has no inverse labels");
    const unsigned grid = (unsigned)std::min<int64_t>(65536, n);
    hipLaunchKernelGGL(recon_decode_kernel, dim3(grid), dim3(256), 0, h->stream, a, n, d_list, d_pos, d_out);
    HIP_TRY(hipGetLastError());
    return IVFADC_OK;
}

// host entries: the requested ids sorted and made unique on the host (as ivfadc_delete_ids does), everything else on the device.
// d_list / d_pos / d_found: h->rc_list / rc_pos / rc_found, filled for the n requests.
static int locate_host(ivfadc_index *h, int64_t n, const uint32_t *ids)
{
    std::vector<uint32_t> want(ids, ids + n);
    std::sort(want.begin(), want.end());
    want.erase(std::unique(want.begin(), want.end()), want.end());
    TRY(h->rc_want.ensure(want.size() * 4));
    TRY(h2d_copy(h->rc_want.p, want.data(), want.size() * 4, h->stream));
    TRY(h->rc_req.ensure((size_t)n * 4));
    TRY(h2d_copy(h->rc_req.p, ids, (size_t)n * 4, h->stream));
    TRY(h->rc_list.ensure((size_t)n * 4));
    TRY(h->rc_pos.ensure((size_t)n * 8));
    TRY(h->rc_found.ensure((size_t)n));
    TRY(locate_sorted(h, h->rc_want.as<u32>(), want.size(), true, want.front(), want.back()));
    return recon_resolve(h, h->rc_req.as<u32>(), n, h->rc_want.as<u32>(), want.size(), h->rc_list.as<int32_t>(), h->rc_pos.as<int64_t>(),
                         h->rc_found.as<uint8_t>());
}

// device entries: the requested ids are sorted on the device (rocPRIM; repeats stay); every step is enqueued on the handle's stream, nothing
// is uploaded and nothing waited for (a workspace buffer that has to grow is reallocated, as by any search)
// (span_known: a caller that has seen the ids on the host passes their smallest and largest, and the bitmap covers that span alone)
static int locate_device(ivfadc_index *h, int64_t n, const uint32_t *d_ids, int32_t *d_list, int64_t *d_pos, uint8_t *d_found,
                         bool span_known = false, uint32_t want_lo = 0u, uint32_t want_hi = 0u)
{
    if (n > (int64_t)0x7FFFFFFF) return fail(IVFADC_ERR_INVALID, "n = %lld ids in one call (the device entries sort at most 2^31 - 1)", (long long)n);
    TRY(h->rc_want.ensure((size_t)n * 4));
    size_t tmp = 0;
    HIP_TRY(rocprim::radix_sort_keys(nullptr, tmp, d_ids, h->rc_want.as<u32>(), (unsigned)n, 0, 32, h->stream));
    TRY(h->rc_tmp.ensure(std::max<size_t>(tmp, 16)));
    HIP_TRY(rocprim::radix_sort_keys(h->rc_tmp.p, tmp, d_ids, h->rc_want.as<u32>(), (unsigned)n, 0, 32, h->stream));
    TRY(locate_sorted(h, h->rc_want.as<u32>(), (uint64_t)n, span_known, want_lo, want_hi));
    return recon_resolve(h, d_ids, n, h->rc_want.as<u32>(), (uint64_t)n, d_list, d_pos, d_found);
}

int ivfadc_locate(ivfadc_t *h, int64_t n, const uint32_t *ids, int32_t *out_list, int64_t *out_pos)
try {
    TRY(check_recon_args("ivfadc_locate", h, n, ids, out_list, "out_list", out_pos, "out_pos"));
    HandleLock lk_(h);
    TRY(recon_begin(h, "ivfadc_locate"));
    if (n == 0) return IVFADC_OK;
    int rc = locate_host(h, n, ids);
    if (rc == IVFADC_OK) rc = d2h_copy(out_list, h->rc_list.p, (size_t)n * 4, h->stream);
    if (rc == IVFADC_OK) rc = d2h_copy(out_pos, h->rc_pos.p, (size_t)n * 8, h->stream);
    return recon_exit(h, rc);
} IVF_CATCH

int ivfadc_reconstruct(ivfadc_t *h, int64_t n, const uint32_t *ids, float *out_vectors, uint8_t *out_found)
try {
    TRY(check_recon_args("ivfadc_reconstruct", h, n, ids, out_vectors, "out_vectors", nullptr, nullptr));
    HandleLock lk_(h);
    TRY(recon_begin(h, "ivfadc_reconstruct"));
    if (n == 0) return IVFADC_OK;
    const size_t vbytes = (size_t)n * h->d * 4;
    int rc = locate_host(h, n, ids);
    if (rc == IVFADC_OK) rc = h->rc_vec.ensure(vbytes);
    if (rc == IVFADC_OK) rc = recon_decode(h, n, h->rc_list.as<int32_t>(), h->rc_pos.as<int64_t>(), h->rc_vec.as<float>());
    if (rc == IVFADC_OK) rc = d2h_copy(out_vectors, h->rc_vec.p, vbytes, h->stream);
    if (rc == IVFADC_OK && out_found) rc = d2h_copy(out_found, h->rc_found.p, (size_t)n, h->stream);
    return recon_exit(h, rc);
} IVF_CATCH

int ivfadc_locate_device(ivfadc_t *h, int64_t n, const uint32_t *d_ids, int32_t *d_out_list, int64_t *d_out_pos)
try {
    TRY(check_recon_args("ivfadc_locate_device", h, n, d_ids, d_out_list, "out_list", d_out_pos, "out_pos"));
    HandleLock lk_(h);
    TRY(recon_begin(h, "ivfadc_locate_device"));
    if (n == 0) return IVFADC_OK;
    return recon_exit(h, locate_device(h, n, d_ids, d_out_list, d_out_pos, nullptr));
} IVF_CATCH

int ivfadc_reconstruct_device(ivfadc_t *h, int64_t n, const uint32_t *d_ids, float *d_out_vectors, uint8_t *d_out_found)
try {
    TRY(check_recon_args("ivfadc_reconstruct_device", h, n, d_ids, d_out_vectors, "out_vectors", nullptr, nullptr));
    HandleLock lk_(h);
    TRY(recon_begin(h, "ivfadc_reconstruct_device"));
    if (n == 0) return IVFADC_OK;
    int rc = h->rc_list.ensure((size_t)n * 4);
    if (rc == IVFADC_OK) rc = h->rc_pos.ensure((size_t)n * 8);
    if (rc == IVFADC_OK) rc = locate_device(h, n, d_ids, h->rc_list.as<int32_t>(), h->rc_pos.as<int64_t>(), d_out_found);
    if (rc == IVFADC_OK) rc = recon_decode(h, n, h->rc_list.as<int32_t>(), h->rc_pos.as<int64_t>(), d_out_vectors);
    return recon_exit(h, rc);
} IVF_CATCH

// ---- score caller-supplied candidate ids (score_plan.h, score.hip.h) --------------------------------------------------
// "What distance would knn_search report between this query and these stored ids": locate (above), then one lane per (query, id) pair
// runs the canonical Float32 chains of the distance.  No scan of the lists, no table.

// the arguments of both entries, before the handle is looked at and before any device call
static int check_score_args(const char *fn, ivfadc_t *h, int64_t nq, const float *queries, int64_t C, int64_t ids_stride, const uint32_t *ids,
                            const float *out_dists)
{
    if (!h) return fail(IVFADC_ERR_INVALID, "%s: null handle", fn);
    if (nq < 0) return fail(IVFADC_ERR_INVALID, "%s: nq = %lld < 0", fn, (long long)nq);
    if (C < 0) return fail(IVFADC_ERR_INVALID, "%s: C = %lld < 0", fn, (long long)C);
    if (score::stride_form(C, ids_stride) == score::FORM_BAD)
        return fail(IVFADC_ERR_INVALID, "%s: ids_stride = %lld (C = %lld for per-query rows, 0 for one shared row)", fn, (long long)ids_stride,
                    (long long)C);
    if (!score::pairs_fit(nq, C))
        return fail(IVFADC_ERR_INVALID, "%s: nq x C = %lld x %lld pairs in one call (at most 2^31 - 1)", fn, (long long)nq, (long long)C);
    if (nq == 0 || C == 0) return IVFADC_OK;
    if (!queries) return fail(IVFADC_ERR_INVALID, "%s: null queries", fn);
    if (!ids) return fail(IVFADC_ERR_INVALID, "%s: null ids", fn);
    if (!out_dists) return fail(IVFADC_ERR_INVALID, "%s: null out_dists", fn);
    return IVFADC_OK;
}

// every pointer in device memory; only enqueues.  span_known: the smallest and largest id of the live slots, where the host has seen them
static int score_enqueue(ivfadc_index *h, int64_t nq, const float *d_q, int64_t C, int64_t ids_stride, const uint32_t *d_ids,
                         const int32_t *d_counts, float *d_dists, uint8_t *d_found, bool span_known, uint32_t want_lo, uint32_t want_hi)
{
    const score::Plan pl = score::make_plan(nq, C, ids_stride, h->d, (uint64_t)h->ws_budget);
    DecodeArgs a{};
    a.centroids = h->centroids.as<float>();
    a.codebooks = h->codebooks.as<float>();
    a.label_inv = h->u16 ? (const uint8_t *)nullptr : h->label_inv.as<uint8_t>();
    a.codes = h->codes.as<uint8_t>();
    a.list_codeoff = h->list_codeoff.as<int64_t>();
    a.d = h->d; a.m = h->m; a.dsub = h->dsub; a.ksub = h->ksub; a.cs = h->cs;
    if (!h->u16 && !a.label_inv) return fail(IVFADC_ERR_STATE, "the handle has no inverse labels");
    TRY(h->rc_list.ensure((size_t)pl.locate_slots * 4));
    TRY(h->rc_pos.ensure((size_t)pl.locate_slots * 8));
    if (pl.shared) TRY(locate_device(h, C, d_ids, h->rc_list.as<int32_t>(), h->rc_pos.as<int64_t>(), nullptr, span_known, want_lo, want_hi));
    for (int64_t s = 0; s < pl.nslices; ++s) {
        const int64_t q0 = score::slice_begin(pl, s), nqs = score::slice_queries(pl, s);
        if (!pl.shared)
            TRY(locate_device(h, nqs * C, &d_ids[score::id_index(q0, ids_stride, 0)], h->rc_list.as<int32_t>(), h->rc_pos.as<int64_t>(), nullptr,
                              span_known, want_lo, want_hi));
        hipLaunchKernelGGL(score_pairs_kernel, dim3(pl.grid_x, (unsigned)nqs), dim3(score::TILE), pl.lds, h->stream, a, h->kc, d_q, q0, C, pl.shared,
                           d_counts, h->rc_list.as<int32_t>(), h->rc_pos.as<int64_t>(), d_dists, d_found);
        HIP_TRY(hipGetLastError());
    }
    return IVFADC_OK;
}

int ivfadc_score_ids(ivfadc_t *h, int64_t nq, const float *queries, int64_t C, int64_t ids_stride, const uint32_t *ids, const int32_t *counts,
                     float *out_dists, uint8_t *out_found)
try {
    TRY(check_score_args("ivfadc_score_ids", h, nq, queries, C, ids_stride, ids, out_dists));
    const bool shared = score::stride_form(C, ids_stride) == score::FORM_SHARED;
    // counts in [0, C], and the span of the ids of the live slots (the bitmap of the locate pass covers it alone)
    uint32_t lo = 0xFFFFFFFFu, hi = 0u;
    bool any = false;
    if (nq > 0 && C > 0) {
        int64_t longest = C;
        if (counts) {
            longest = 0;
            for (int64_t q = 0; q < nq; ++q) {
                if (counts[q] < 0 || (int64_t)counts[q] > C)
                    return fail(IVFADC_ERR_INVALID, "ivfadc_score_ids: query %lld: counts = %d outside [0, %lld]", (long long)q, (int)counts[q], (long long)C);
                longest = std::max<int64_t>(longest, counts[q]);
            }
        }
        const int64_t rows = shared ? 1 : nq;
        for (int64_t q = 0; q < rows; ++q) {
            const int64_t live = shared ? longest : score::live_slots(counts != nullptr, counts ? counts[q] : 0, C);
            const uint32_t *row = ids + score::id_index(q, ids_stride, 0);
            for (int64_t j = 0; j < live; ++j) {
                lo = std::min(lo, row[j]);
                hi = std::max(hi, row[j]);
                any = true;
            }
        }
    }
    if (nq == 0 || C == 0) return IVFADC_OK;   // (nothing to score: the handle is not looked at)
    HandleLock lk_(h);
    TRY(recon_begin(h, "ivfadc_score_ids"));
    const size_t pairs = (size_t)nq * (size_t)C, nid = shared ? (size_t)C : pairs;
    int rc = h->sc_q.ensure((size_t)nq * h->d * 4);
    if (rc == IVFADC_OK) rc = h->sc_ids.ensure(nid * 4);
    if (rc == IVFADC_OK) rc = h->sc_dist.ensure(pairs * 4);
    if (rc == IVFADC_OK) rc = h->sc_found.ensure(pairs);
    if (rc == IVFADC_OK && counts) rc = h->sc_cnt.ensure((size_t)nq * 4);
    if (rc == IVFADC_OK) rc = h2d_copy(h->sc_q.p, queries, (size_t)nq * h->d * 4, h->stream);
    if (rc == IVFADC_OK) rc = h2d_copy(h->sc_ids.p, ids, nid * 4, h->stream);
    if (rc == IVFADC_OK && counts) rc = h2d_copy(h->sc_cnt.p, counts, (size_t)nq * 4, h->stream);
    if (rc == IVFADC_OK)
        rc = score_enqueue(h, nq, h->sc_q.as<float>(), C, ids_stride, h->sc_ids.as<u32>(), counts ? h->sc_cnt.as<int32_t>() : (const int32_t *)nullptr,
                           h->sc_dist.as<float>(), h->sc_found.as<uint8_t>(), true, any ? lo : 0u, any ? hi : 0u);   // (no live slot: a span of one id)
    if (rc == IVFADC_OK) rc = d2h_copy(out_dists, h->sc_dist.p, pairs * 4, h->stream);
    if (rc == IVFADC_OK && out_found) rc = d2h_copy(out_found, h->sc_found.p, pairs, h->stream);
    return recon_exit(h, rc);
} IVF_CATCH

int ivfadc_score_ids_device(ivfadc_t *h, int64_t nq, const float *d_queries, int64_t C, int64_t ids_stride, const uint32_t *d_ids,
                            const int32_t *d_counts, float *d_out_dists, uint8_t *d_out_found)
try {
    TRY(check_score_args("ivfadc_score_ids_device", h, nq, d_queries, C, ids_stride, d_ids, d_out_dists));
    if (nq == 0 || C == 0) return IVFADC_OK;   // (nothing to score: the handle is not looked at)
    HandleLock lk_(h);
    TRY(recon_begin(h, "ivfadc_score_ids_device"));
    return recon_exit(h, score_enqueue(h, nq, d_queries, C, ids_stride, d_ids, d_counts, d_out_dists, d_out_found, false, 0u, 0u));
} IVF_CATCH

// ---- list-partitioned multi-GPU mode: strong scaling of a FIXED global batch --------------------------------------------------------------
// Queries sharded over replicas cannot scale a fixed batch past the point where every rank streams most of the index for its few
// queries (4.9x at 8 GPUs on the SIFT1B shape).  Here every rank keeps the replica and ALL queries, runs the
// coarse search (identical on every rank), scans only the probed lists l with l % nparts == part -- 1 / nparts of the code bytes, each list
// still shared by as many queries as on one GPU -- and leaves its K smallest KEYS per query (distance bits << 32 | visit order: probes are
// independent given the bound, index.jl:228-255, and visit orders are global).  ONE all-gather of nq x K keys per rank, then the K-way
// merge (partial_merge_kernel) on every rank.
int ivfadc_set_list_partition(ivfadc_t *h, int nparts, int part)
try {
    HandleLock lk_(h);
    if (!h) return fail(IVFADC_ERR_INVALID, "null handle");
    if (nparts < 1 || part < 0 || part >= nparts) return fail(IVFADC_ERR_INVALID, "part %d of %d", part, nparts);
    if (h->u16 && nparts > 1) return fail(IVFADC_ERR_INVALID, "the list-partitioned mode serves UInt8 codes only");
    h->part_n = nparts;
    h->part_i = part;
    h->partial_nq = -1;
    return IVFADC_OK;
} IVF_CATCH

int ivfadc_search_device_partial(ivfadc_t *h, int64_t nq, const float *d_queries, int K, int w, uint64_t *d_keys, int32_t *d_counts)
try {
    HandleLock lk_(h);
    TRY(check_search_args(h, nq, K, w));
    if (nq > 0 && (!d_queries || !d_keys || !d_counts)) return fail(IVFADC_ERR_INVALID, "null buffer");
    if (h->part_n < 2) return fail(IVFADC_ERR_STATE, "ivfadc_set_list_partition(h, nparts >= 2, part) first");
    h->partial_keys = d_keys;
    h->partial_nq = -1;
    const int rc = search_dev(h, SearchCall{nq, h->d, K, w, d_queries, nullptr, nullptr, d_counts});
    h->partial_keys = nullptr;
    if (rc == IVFADC_OK) { h->partial_nq = nq; h->partial_w = w; h->partial_K = K; }
    return rc;
} IVF_CATCH

static int merge_partials_dev(ivfadc_t *h, int64_t nq, int K, int nparts, const uint64_t *d_keys, size_t stride_u64, const int32_t *d_counts,
                              size_t stride_i32, uint32_t *d_ids, float *d_dists, int32_t *d_out_counts)
{
    if (h->partial_nq != nq || h->partial_K != K)
        return fail(IVFADC_ERR_STATE, "ivfadc_merge_partials_device: the handle's last partial search was on %lld queries with K = %d", (long long)h->partial_nq, h->partial_K);
    TRY(set_device(h));
    const bool small_k = K <= 64;
    const int cap = small_k ? 64 : std::max(128, pow2ceil(K + 64));
    const size_t mlds = small_k ? 0 : (size_t)4 * cap * 8;
    const u32 *idp = h->synthetic ? (const u32 *)nullptr : h->ids.as<u32>();
    if (mlds > (size_t)(32 << 10)) { int occ_unused = 0; TRY(fn_occupancy(h, (const void *)partial_merge_kernel<false>, mlds, occ_unused, false)); }
    hipLaunchKernelGGL(small_k ? partial_merge_kernel<true> : partial_merge_kernel<false>, dim3((unsigned)((nq + 3) / 4)), dim3(256), mlds, h->stream, (int)nq, h->partial_w, K, cap, nparts,
                           (const u64 *)d_keys, stride_u64, (const int *)d_counts, stride_i32, h->probe_list.as<int>(), h->probe_base.as<u32>(),
                           h->list_pos.as<int64_t>(), idp, d_ids, d_dists, d_out_counts);
    HIP_TRY(hipGetLastError());
    return IVFADC_OK;
}

int ivfadc_merge_partials_device(ivfadc_t *h, int64_t nq, int K, int nparts, const uint64_t *d_keys_all, const int32_t *d_counts_all,
                                 uint32_t *d_ids, float *d_dists, int32_t *d_counts)
try {
    HandleLock lk_(h);
    if (!h) return fail(IVFADC_ERR_INVALID, "null handle");
    if (nq < 0 || K < 1 || nparts < 1) return fail(IVFADC_ERR_INVALID, "nq, K, nparts");
    if (nq == 0) return IVFADC_OK;
    if (!d_keys_all || !d_counts_all || !d_ids || !d_dists || !d_counts) return fail(IVFADC_ERR_INVALID, "null buffer");
    return merge_partials_dev(h, nq, K, nparts, d_keys_all, (size_t)nq * K, d_counts_all, (size_t)nq, d_ids, d_dists, d_counts);
} IVF_CATCH

// ---- host-pointer entries ----------------------------------------------------------------------------------------------------
// The reference's contract is host arrays in, host arrays out (index.jl:261-265).  What that costs on top of the device-resident search
// (tools/micro/host_path.hip, one MI355X box, 1024 x 128 f32 queries in, 84 KB out): the copy into pinned memory 7 us, a copy-engine H2D
// 19 us alone and ~10 us more than a copy KERNEL inside a chain, a D2H copy 10 us, and every in-stream hand-off between the SDMA and the
// compute queue a few more.  So: queries are ingested by a kernel that reads page-locked host memory (the caller's own array when the
// library knows it -- ivfadc_host_register / ivfadc_host_alloc -- else pin_in), a handful of queries (latency path) are read in place,
// and the final kernel of the search writes ids / distances / counts straight into page-locked host memory (the caller's arrays when
// known, else pin_out): no device result block and no D2H copy in the chain.
static inline double now_us()
{
    return std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

// page-locked host rows -> device, on stream s
static int ingest_rows(ivfadc_index *h, hipStream_t s, const void *src, void *dst, size_t bytes)
{
    if (bytes == 0) return IVFADC_OK;
    if (bytes > ((size_t)256 << 20) || (bytes & 3) != 0) {
        HIP_TRY(hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, s));
        return IVFADC_OK;
    }
    const size_t nwords = bytes / 4;
    const bool vec = ((((uintptr_t)src) | ((uintptr_t)dst)) & 15) == 0;
    const size_t nvec = vec ? nwords / 4 : 0;
    const size_t items = vec ? nvec + 3 : nwords;
    const unsigned grid = (unsigned)std::max<size_t>(1, std::min<size_t>((items + 255) / 256, (size_t)4 * h->num_cu));
    hipLaunchKernelGGL(host_ingest_kernel, dim3(grid), dim3(256), 0, s, (const u32 *)src, (u32 *)dst, nvec, nwords);
    HIP_TRY(hipGetLastError());
    return IVFADC_OK;
}

// The staging of a host call.  The four time buckets of ivfadc_host_stats are laps of one clock per call.
struct HostClock {
    double t = now_us();
    double lap() { const double n = now_us(), dt = n - t; t = n; return dt; }
};

// src (null on entry: not decided yet) = where the kernels read a host array of rows: the caller's own array when the library knows it,
// else pin_in, which then takes bytes [off, off + len) of the rows
static int stage_queries(ivfadc_index *h, const void *rows, size_t bytes, size_t off, size_t len, const uint8_t *&src)
{
    if (!src && host_known(rows, bytes)) src = (const uint8_t *)rows;
    if (!src) {
        TRY(h->pin_in.ensure(bytes));
        src = (const uint8_t *)h->pin_in.p;
    }
    if (src != rows) memcpy((uint8_t *)h->pin_in.p + off, (const uint8_t *)rows + off, len);
    return IVFADC_OK;
}
// Where the kernels write: c keeps the caller's arrays when the library knows all three (the handle remembers: hc_out_direct), else it is
// pointed at the block carved out of pin_out, which copy_out hands over once the search has ended
static int stage_results(ivfadc_index *h, SearchCall &c)
{
    const batch_plan::ResultBlock b = batch_plan::result_bytes((size_t)c.nq, (size_t)c.K);
    h->hc_out_direct = host_known(c.ids, b.ids_len()) && host_known(c.dists, b.ids_len()) && host_known(c.counts, b.counts_len());
    if (h->hc_out_direct) return IVFADC_OK;
    TRY(h->pin_out.ensure(b.total));
    uint8_t *po = (uint8_t *)h->pin_out.p;
    c.ids = (uint32_t *)(po + b.ids);
    c.dists = (float *)(po + b.dists);
    c.counts = (int32_t *)(po + b.counts);
    return IVFADC_OK;
}
// the first to.nq rows of a packed block of block_rows rows, into the three arrays of `to`
static void copy_out(const SearchCall &to, const void *block, int64_t block_rows)
{
    const batch_plan::ResultBlock src = batch_plan::result_bytes((size_t)block_rows, (size_t)to.K), n = batch_plan::result_bytes((size_t)to.nq, (size_t)to.K);
    const uint8_t *p = (const uint8_t *)block;
    memcpy(to.ids, p + src.ids, n.ids_len());
    memcpy(to.dists, p + src.dists, n.ids_len());
    memcpy(to.counts, p + src.counts, n.counts_len());
}

// host-pointer search in two halves so several handles (devices) can be in flight at once (ivfadc_mg_search)
// hc: this handle's whole batch as a host entry has it: queries, results and supplied probes (validated by the caller) in host memory,
// mask rows on the device already (stage_mask_numbers)
static int search_enqueue(ivfadc_t *h, const SearchCall &hc)
try {
    TRY(set_device(h));
    h->dev_entry = false;
    HostClock clk;
    const int64_t nq = hc.nq;
    const size_t qbytes = (size_t)nq * h->d * 4;
    h->hstats.calls++;
    h->hstats.batches++;
    const uint8_t *src = nullptr;
    TRY(stage_queries(h, hc.q, qbytes, 0, qbytes, src));
    h->hstats.queries_direct += src == (const uint8_t *)hc.q;
    const double t_in = clk.lap();
    if (h->dirty) TRY(upload_lists(h));
    SearchCall c = hc;   // the same call in device terms
    c.whole_batch = true;
    c.q = (const float *)src;
    static const bool no_zero_copy = getenv("IVFADC_NO_ZERO_COPY") != nullptr;
    if (!no_zero_copy && !hc.pre() && !hc.masked() && h->part_n <= 1 && (((uintptr_t)src) & 15) == 0 && sq_eligible(h, nq, hc.K, hc.w)) {
        // the latency path: a handful of rows, read in place by the two launches (a few KB over PCIe; no ingest step in the chain)
        h->hstats.zero_copy++;
    } else {
        TRY(h->q_stage.ensure(qbytes));
        TRY(ingest_rows(h, h->stream, src, h->q_stage.p, qbytes));
        c.q = h->q_stage.as<float>();
    }
    TRY(stage_results(h, c));
    h->hstats.results_direct += h->hc_out_direct;
    if (hc.pre()) {
        const size_t pb = (size_t)nq * hc.w * 4;
        TRY(h->pre_list.ensure(pb));
        TRY(h->pre_dc.ensure(pb));
        TRY(h2d_copy(h->pre_list.p, hc.pre_list, pb, h->stream));
        TRY(h2d_copy(h->pre_dc.p, hc.pre_dc, pb, h->stream));
        c.pre_list = h->pre_list.as<int>();
        c.pre_dc = h->pre_dc.as<float>();
    }
    TRY(search_dev(h, c));
    h->hstats.stage_in_us += t_in;
    h->hstats.enqueue_us += clk.lap();
    return IVFADC_OK;
} IVF_CATCH

static int search_finish(ivfadc_t *h, const SearchCall &hc)
try {
    TRY(set_device(h));
    HostClock clk;
    TRY(wait_stream(h));
    h->hstats.wait_us += clk.lap();
    if (!h->hc_out_direct) copy_out(hc, h->pin_out.p, hc.nq);
    h->hstats.stage_out_us += clk.lap();
    return IVFADC_OK;
} IVF_CATCH

int ivfadc_search(ivfadc_t *h, int64_t nq, const float *queries, int K, int w, uint32_t *out_ids, float *out_dists,
                  int32_t *out_counts)
try {
    HandleLock lk_(h);
    TRY(check_search_args(h, nq, K, w));
    if (nq == 0) return IVFADC_OK;
    if (!queries || !out_ids || !out_dists || !out_counts) return fail(IVFADC_ERR_INVALID, "null buffer");
    const SearchCall hc{nq, h->d, K, w, queries, out_ids, out_dists, out_counts};
    const int rc = search_enqueue(h, hc);
    return rc != IVFADC_OK ? finish_entry(h, rc) : search_finish(h, hc);
} IVF_CATCH

// ---- range search (include/ivfadc_hip.h: "RANGE search"; no reference counterpart) -------------------------------------------------
// Every argument is judged before the handle is looked at or the device is touched; host_radii (the host entry's) are read for NaN.
// masked_entry: the masked entries serve 16-bit handles (range_u16_*_kernel), the plain entries keep refusing them; stray_moq: such an
// entry was given mask numbers and no set
static int check_range_args(ivfadc_index *h, int64_t nq, const float *queries, const float *radii, const float *host_radii, int &w,
                            int64_t max_total, ivfadc_range_result_t **out, bool masked_entry = false, bool stray_moq = false)
{
    if (!out) return fail(IVFADC_ERR_INVALID, "null out");
    *out = nullptr;
    if (max_total < 0) return fail(IVFADC_ERR_INVALID, "max_total < 0 (0: no cap)");
    if (w < 1) return fail(IVFADC_ERR_ASSERT, "Number of clusters to search in must be w >= 1");
    if (nq < 0) return fail(IVFADC_ERR_INVALID, "nq < 0");
    if (!radii) return fail(IVFADC_ERR_INVALID, "null radii (one radius per query)");
    if (nq > 0 && !queries) return fail(IVFADC_ERR_INVALID, "null queries");
    if (host_radii)
        for (int64_t q = 0; q < nq; ++q)
            if (host_radii[q] != host_radii[q]) return fail(IVFADC_ERR_INVALID, "the radius of query %lld is NaN", (long long)q);
    if (stray_moq) return fail(IVFADC_ERR_INVALID, "ivfadc_range_search_masked: mask_of_query without a mask set (a null set filters no query)");
    if (!h) return fail(IVFADC_ERR_INVALID, "null handle");
    TRY(check_view_current(h));
    if (h->u16 && !masked_entry)
        return fail(IVFADC_ERR_STATE, "range search serves handles with 8-bit codes only: this handle holds UInt16 codes (ivfadc_range_search_masked with a null set serves them)");
    if (h->part_n > 1) return fail(IVFADC_ERR_STATE, "a list partition is set (ivfadc_set_list_partition): range search serves whole indexes only");
    if (!h->have_lists && !h->dirty) return fail(IVFADC_ERR_STATE, "no inverted lists set");
    w = std::min(w, h->kc);
    return IVFADC_OK;
}

// The four range entries.  s null: no query is filtered; else h is the index s was made from, unchanged since, or a plain view of it.
// host: queries, radii and mask numbers lie in host memory, and go to q_stage / rng_radii / mask_q on the handle's stream.
static int range_entry(ivfadc_index *h, const ivfadc_maskset *s, int64_t nq, const float *queries, const float *radii, int w, int64_t max_total,
                       const int32_t *mask_of_query, ivfadc_range_result_t **out, bool host, bool masked_entry)
{
    TRY(check_range_args(h, nq, queries, radii, host ? radii : nullptr, w, max_total, out, masked_entry, !s && mask_of_query));
    if (s) TRY(check_mask_link(h, s, "ivfadc_range_search_masked"));
    if (s && host) TRY(check_mask_numbers(s, nq, mask_of_query));
    if (s || host) TRY(set_device(h));
    SearchCall c{nq, h->d, 0, w, queries, nullptr, nullptr, nullptr, radii};   // (no K, no result rows: the result is allocated once the totals are known)
    int rc = IVFADC_OK;
    if (host) {
        const size_t qbytes = (size_t)nq * h->d * 4, rbytes = (size_t)nq * 4;
        rc = h->q_stage.ensure(std::max<size_t>(qbytes, 16));
        if (rc == IVFADC_OK) rc = h->rng_radii.ensure(std::max<size_t>(rbytes, 16));
        if (rc == IVFADC_OK) rc = h2d_copy(h->q_stage.p, queries, qbytes, h->stream);
        if (rc == IVFADC_OK) rc = h2d_copy(h->rng_radii.p, radii, rbytes, h->stream);
        c.q = h->q_stage.as<float>(); c.radii = h->rng_radii.as<float>();
    }
    if (rc == IVFADC_OK && s) rc = stage_mask_numbers(h, s, mask_of_query, !host, c);
    if (rc == IVFADC_OK) rc = range_dev(h, c, max_total, out);
    return finish_entry(h, rc);
}

int ivfadc_range_search_device(ivfadc_t *h, int64_t nq, const float *d_queries, const float *d_radii, int w, int64_t max_total,
                               ivfadc_range_result_t **out)
try {
    HandleLock lk_(h);
    return range_entry(h, nullptr, nq, d_queries, d_radii, w, max_total, nullptr, out, false, false);
} IVF_CATCH

int ivfadc_range_search(ivfadc_t *h, int64_t nq, const float *queries, const float *radii, int w, int64_t max_total,
                        ivfadc_range_result_t **out)
try {
    HandleLock lk_(h);
    return range_entry(h, nullptr, nq, queries, radii, w, max_total, nullptr, out, true, false);
} IVF_CATCH

int ivfadc_range_search_device_masked(ivfadc_t *h, const ivfadc_maskset_t *s, int64_t nq, const float *d_queries, const float *d_radii, int w,
                                      int64_t max_total, const int32_t *d_mask_of_query, ivfadc_range_result_t **out)
try {
    HandleLock lk_(h);
    return range_entry(h, s, nq, d_queries, d_radii, w, max_total, d_mask_of_query, out, false, true);
} IVF_CATCH

int ivfadc_range_search_masked(ivfadc_t *h, const ivfadc_maskset_t *s, int64_t nq, const float *queries, const float *radii, int w,
                               int64_t max_total, const int32_t *mask_of_query, ivfadc_range_result_t **out)
try {
    HandleLock lk_(h);
    return range_entry(h, s, nq, queries, radii, w, max_total, mask_of_query, out, true, true);
} IVF_CATCH

int ivfadc_range_result_sizes(const ivfadc_range_result_t *r, int64_t *out_nq, int64_t *out_total)
try {
    if (!r) return fail(IVFADC_ERR_INVALID, "null result");
    if (out_nq) *out_nq = r->nq;
    if (out_total) *out_total = r->total;
    return IVFADC_OK;
} IVF_CATCH

int ivfadc_range_result_copy(const ivfadc_range_result_t *r, int64_t *lims, uint32_t *ids, float *dists)
try {
    if (!r) return fail(IVFADC_ERR_INVALID, "null result");
    if (lims) memcpy(lims, r->lims.data(), r->lims.size() * sizeof(int64_t));
    if (r->total > 0 && (ids || dists)) {
        // the calling thread's current device is the caller's: restored on every way out
        struct DeviceBack { int prev = -1; ~DeviceBack() { if (prev >= 0) (void)hipSetDevice(prev); } } back;
        if (hipGetDevice(&back.prev) != hipSuccess || back.prev == r->device) back.prev = -1;
        HIP_TRY(hipSetDevice(r->device));
        if (ids) HIP_TRY(hipMemcpy(ids, r->d_ids, (size_t)r->total * 4, hipMemcpyDeviceToHost));
        if (dists) HIP_TRY(hipMemcpy(dists, r->d_dists, (size_t)r->total * 4, hipMemcpyDeviceToHost));
    }
    return IVFADC_OK;
} IVF_CATCH

int ivfadc_range_result_device(const ivfadc_range_result_t *r, const int64_t **d_lims, const uint32_t **d_ids, const float **d_dists)
try {
    if (!r) return fail(IVFADC_ERR_INVALID, "null result");
    if (d_lims) *d_lims = r->d_lims;
    if (d_ids) *d_ids = r->d_ids;
    if (d_dists) *d_dists = r->d_dists;
    return IVFADC_OK;
} IVF_CATCH

void ivfadc_range_result_destroy(ivfadc_range_result_t *r)
{
    delete r;   // (null: a no-op, as free(NULL); the result holds nothing of the handle it came from)
}

// ---- the seam of the reference's knn_search (index.jl:204-258): coarse_search on one side, everything that reads its two vectors on
// the other ("Caller-supplied probes") ----------------------------------------------------------------------------------
static int check_coarse_args(ivfadc_index *h, int64_t nq, int w)
{
    if (!h) return fail(IVFADC_ERR_INVALID, "null handle");
    TRY(check_view_current(h));
    if (w < 1) return fail(IVFADC_ERR_ASSERT, "Number of clusters to search in must be w >= 1");
    if (nq < 0) return fail(IVFADC_ERR_INVALID, "nq < 0");
    if (w > h->kc) return fail(IVFADC_ERR_INVALID, "w = %d exceeds the %d cells of the coarse quantizer (sortperm(...)[1:w], coarsequantizers.jl:36)", w, h->kc);
    if (!h->have_lists && !h->dirty) return fail(IVFADC_ERR_STATE, "no inverted lists set");
    if ((int64_t)nq * w > ((int64_t)1 << 40)) return fail(IVFADC_ERR_INVALID, "nq x w = %lld probe slots", (long long)nq * w);
    return IVFADC_OK;
}

int ivfadc_coarse_search_device(ivfadc_t *h, int64_t nq, const float *d_queries, int w, int32_t *d_lists, float *d_dists)
try {
    HandleLock lk_(h);
    TRY(check_coarse_args(h, nq, w));
    if (nq > 0 && (!d_queries || !d_lists || !d_dists)) return fail(IVFADC_ERR_INVALID, "null buffer");
    SearchCall c{nq, h->d, 0, w, d_queries};
    c.out_list = d_lists; c.out_dc = d_dists;   // (a coarse call: the queries and where their w probes go)
    return coarse_dev(h, c);
} IVF_CATCH

int ivfadc_coarse_search(ivfadc_t *h, int64_t nq, const float *queries, int w, int32_t *out_lists, float *out_dists)
try {
    HandleLock lk_(h);
    TRY(check_coarse_args(h, nq, w));
    if (nq == 0) return IVFADC_OK;
    if (!queries || !out_lists || !out_dists) return fail(IVFADC_ERR_INVALID, "null buffer");
    TRY(set_device(h));
    const size_t qbytes = (size_t)nq * h->d * 4, pb = (size_t)nq * w * 4;
    TRY(h->q_stage.ensure(qbytes));
    TRY(h->pre_list.ensure(pb));
    TRY(h->pre_dc.ensure(pb));
    TRY(h2d_copy(h->q_stage.p, queries, qbytes, h->stream));
    SearchCall c{nq, h->d, 0, w, h->q_stage.as<float>()};
    c.out_list = h->pre_list.as<int32_t>(); c.out_dc = h->pre_dc.as<float>();
    int rc = coarse_dev(h, c);
    if (rc == IVFADC_OK) rc = d2h_copy(out_lists, h->pre_list.p, pb, h->stream);
    if (rc == IVFADC_OK) rc = d2h_copy(out_dists, h->pre_dc.p, pb, h->stream);
    return finish_entry(h, rc);
} IVF_CATCH

// K, w and the handle's state, shared by the two preassigned entries (w is NOT clamped: the probes are nq x w as given)
static int check_preassigned_args(ivfadc_index *h, int64_t nq, int K, int w)
{
    int wc = w;
    TRY(check_search_args(h, nq, K, wc));
    if (w > h->kc) return fail(IVFADC_ERR_INVALID, "w = %d exceeds the %d cells of the coarse quantizer: the probes of a query are distinct lists", w, h->kc);
    if (h->part_n > 1) return fail(IVFADC_ERR_STATE, "a list partition is set (ivfadc_set_list_partition): searches with supplied probes serve whole indexes only");
    if ((int64_t)nq * w > ((int64_t)1 << 40)) return fail(IVFADC_ERR_INVALID, "nq x w = %lld probe slots", (long long)nq * w);
    return IVFADC_OK;
}

int ivfadc_search_device_preassigned(ivfadc_t *h, int64_t nq, const float *d_queries, int K, int w, const int32_t *d_lists,
                                     const float *d_coarse_dists, uint32_t *d_out_ids, float *d_out_dists, int32_t *d_out_counts)
try {
    HandleLock lk_(h);
    TRY(check_preassigned_args(h, nq, K, w));
    if (nq > 0 && (!d_queries || !d_lists || !d_coarse_dists || !d_out_ids || !d_out_dists || !d_out_counts)) return fail(IVFADC_ERR_INVALID, "null buffer");
    h->dev_entry = false;
    SearchCall c{nq, h->d, K, w, d_queries, d_out_ids, d_out_dists, d_out_counts};
    c.pre_list = (const int *)d_lists; c.pre_dc = d_coarse_dists;
    return search_dev(h, c);
} IVF_CATCH

int ivfadc_search_preassigned(ivfadc_t *h, int64_t nq, const float *queries, int K, int w, const int32_t *lists, const float *coarse_dists,
                              uint32_t *out_ids, float *out_dists, int32_t *out_counts)
try {
    HandleLock lk_(h);
    TRY(check_preassigned_args(h, nq, K, w));
    if (nq == 0) return IVFADC_OK;
    if (!queries || !lists || !coarse_dists || !out_ids || !out_dists || !out_counts) return fail(IVFADC_ERR_INVALID, "null buffer");
    // the preconditions of the probes, before any launch: lists in [0, kc), pairwise distinct within a query; distances finite and >= +0
    // (exact pruning and the selectors compare float bits as unsigned)
    {
        const int kc = h->kc;
        std::vector<int64_t> seen((size_t)kc, -1);
        for (int64_t q = 0; q < nq; ++q)
            for (int j = 0; j < w; ++j) {
                const size_t o = (size_t)q * w + j;
                const int32_t l = lists[o];
                if (l < 0) return fail(IVFADC_ERR_INVALID, "query %lld, rank %d: negative list %d", (long long)q, j, l);
                if (l >= kc) return fail(IVFADC_ERR_INVALID, "query %lld, rank %d: list %d out of range (kc = %d)", (long long)q, j, l, kc);
                if (seen[l] == q) return fail(IVFADC_ERR_INVALID, "query %lld, rank %d: list %d repeated (the probes of a query are distinct lists)", (long long)q, j, l);
                seen[l] = q;
                uint32_t bits;
                memcpy(&bits, &coarse_dists[o], 4);
                if ((bits & 0x7FFFFFFFu) > 0x7F800000u) return fail(IVFADC_ERR_INVALID, "query %lld, rank %d: coarse distance is NaN", (long long)q, j);
                if ((bits & 0x7FFFFFFFu) == 0x7F800000u) return fail(IVFADC_ERR_INVALID, "query %lld, rank %d: coarse distance is infinite", (long long)q, j);
                if (bits & 0x80000000u) return fail(IVFADC_ERR_INVALID, "query %lld, rank %d: negative coarse distance (distances are >= +0)", (long long)q, j);
            }
    }
    SearchCall hc{nq, h->d, K, w, queries, out_ids, out_dists, out_counts};
    hc.pre_list = (const int *)lists; hc.pre_dc = coarse_dists;
    const int rc = search_enqueue(h, hc);
    return rc != IVFADC_OK ? finish_entry(h, rc) : search_finish(h, hc);
} IVF_CATCH

// the cumulative counters of an internal view that is about to be destroyed stay in its index's totals
static void fold_view_counters(ivfadc_index *h, ivfadc_index *v)
{
    ivfadc_stats st;
    const std::string keep = g_err;
    if (ivfadc_get_stats(v, &st) == IVFADC_OK) {
        h->carry_queries += st.queries;
        h->carry_scanned += st.scanned_points;
        h->carry_pruned += st.pruned_points;
        h->carry_surv += st.lb_survivors;
        h->carry_fallbacks += st.coarse_fallbacks;
        h->carry_launches += st.scan_launches;
    }
    g_err = keep;
}

// A run of consecutive batches from host memory: what a serving loop of knn_search(ivfadc, points, k; w) calls does (index.jl:261-273 once
// per batch), as ONE call.  Each batch's results are exactly ivfadc_search's.  The schedule is batch_plan.h's.

// The lanes: two batches in flight, even batches on this handle and odd ones on a view of it (second stream, second workspace) -- not
// while profiling (the statistics are this handle's), not for a view, not for a single batch -- and the copy lane beside them.
static int setup_batch_lanes(ivfadc_index *h, size_t nbat, ivfadc_index *&lane2)
{
    static const bool no_pipe = getenv("IVFADC_NO_PIPELINE") != nullptr;
    lane2 = nullptr;
    if (h->pipe_view && h->pipe_view->view_gen != h->generation) {
        fold_view_counters(h, h->pipe_view);
        ivfadc_destroy(h->pipe_view);
        h->pipe_view = nullptr;
    }
    if (h->dirty) TRY(upload_lists(h));
    if (!no_pipe && !h->is_view && !h->profiling && nbat >= 2) {
        if (!h->pipe_view) TRY(clone_view(h, &h->pipe_view));
        if (!h->pipe_ev_in) HIP_TRY(hipEventCreateWithFlags(&h->pipe_ev_in, hipEventDisableTiming));
        lane2 = h->pipe_view;
        copy_search_config(lane2, h);
        HIP_TRY(hipEventRecord(h->pipe_ev_in, h->stream));            // in-place edits of the lists queued on this handle's stream come first
        HIP_TRY(hipStreamWaitEvent(lane2->stream, h->pipe_ev_in, 0));
    }
    // (stream priorities do not help here -- measured: a copy lane or a second lane of another priority class is no faster in a process
    // that owns few streams and up to 65 % slower in one that owns many; profiles/r05_batches_stream_priorities.txt)
    if (!h->copy_stream) HIP_TRY(hipStreamCreateWithFlags(&h->copy_stream, hipStreamNonBlocking));
    // ... and the copy lane beside both search lanes (probed once per pair of lanes)
    const hipStream_t l2 = lane2 ? lane2->stream : nullptr;
    if (h->copy_probed_a != h->stream || h->copy_probed_b != l2) {
        const hipStream_t fixed[2] = {h->stream, l2};
        TRY(ensure_overlap(fixed, 2, &h->copy_stream, &h->hstats.streams_replaced));
        h->copy_probed_a = h->stream;
        h->copy_probed_b = l2;
    }
    return IVFADC_OK;
}

// However a run ends, nothing it enqueued is left running: a failing search returns with both lanes and the copy lane drained (the next
// call reuses the staging buffers, and the caller's arrays are the caller's again on return).
struct BatchDrain {
    ivfadc_index *h, *lane2;
    bool armed;
    ~BatchDrain()
    {
        if (!armed) return;
        const std::string keep = g_err;
        if (hipSetDevice(h->device) == hipSuccess) {
            if (h->copy_stream) (void)hipStreamSynchronize(h->copy_stream);
            if (lane2 && lane2->stream) (void)hipStreamSynchronize(lane2->stream);
            if (h->stream) (void)hipStreamSynchronize(h->stream);
        }
        g_err = keep;
    }
};

// From a lane's second search on, the HOST waits for a missing ingest (the lane still has its previous search to run, and the copy lane
// moves a batch in a third of the time a search takes, so this is rare and short): a wait in the search stream would cost the lane's queue
// ~6 us per search whether or not the event has fired by the time the queue gets there.  ev is null on return once it has fired.
static int host_wait(hipEvent_t &ev)
{
    if (!ev) return IVFADC_OK;
    const double t0 = now_us();
    for (;;) {
        const hipError_t q = hipEventQuery(ev);
        if (q == hipSuccess) { ev = nullptr; return IVFADC_OK; }
        if (q != hipErrorNotReady) return fail(IVFADC_ERR_HIP, "hipEventQuery failed: %s", hipGetErrorString(q));
        if (now_us() - t0 > 500.0) return IVFADC_OK;   // (something else owns the copy engine's attention: let the stream wait)
    }
}

// The issue loop of a run: batch_plan's schedule, in HIP calls and searches
struct BatchRun {
    ivfadc_index *h, *lane2;
    const batch_plan::Batches &bt;
    const batch_plan::Groups &gr;
    const void *queries;    // the caller's rows ...
    const uint8_t *qsrc;    // ... and where the copy lane reads them (stage_queries)
    SearchCall all;         // the whole run in device terms: rows in q_stage, results where the kernels write them (stage_results)
    uint64_t base;          // of the run's tokens
    batch_plan::IngestTracker tr;
    size_t up_next = 0;     // groups [0, up_next) are on their way
    double t_stage = 0.0;   // host time spent filling pin_in

    // the copy lane: one ingest launch and one event per group, until want_batches batches are on their way
    int upload_until(size_t want_batches)
    {
        const size_t last = std::min(want_batches, bt.size());
        for (; up_next < gr.size() && gr.first[up_next] < last; ++up_next) {
            const batch_plan::ByteRange r = batch_plan::group_bytes(bt, gr, up_next, (size_t)h->d * 4);
            if (qsrc != queries) {
                HostClock c;
                TRY(stage_queries(h, queries, 0, r.off, r.bytes, qsrc));
                t_stage += c.lap();
            }
            TRY(ingest_rows(h, h->copy_stream, qsrc + r.off, (uint8_t *)h->q_stage.p + r.off, r.bytes));
            HIP_TRY(hipEventRecord(h->ingest_ev[up_next], h->copy_stream));
        }
        return IVFADC_OK;
    }

    // ev: the event the lane still has to wait for before it reads `batch` (null: none; one that has fired costs the lane nothing)
    int pending_event(size_t lane, size_t batch, hipEvent_t &ev)
    {
        ev = nullptr;
        const size_t g = tr.needs(lane, batch);
        if (g == batch_plan::IngestTracker::NOTHING) return IVFADC_OK;
        if (!tr.seen(g)) {
            const hipError_t q = hipEventQuery(h->ingest_ev[g]);
            if (q == hipSuccess) tr.fired(g);
            else if (q != hipErrorNotReady) return fail(IVFADC_ERR_HIP, "hipEventQuery failed: %s", hipGetErrorString(q));
        }
        if (!tr.seen(g)) ev = h->ingest_ev[g];
        return IVFADC_OK;
    }

    int issue()
    {
        const size_t nbat = bt.size(), stride = lane2 ? 2 : 1;
        for (size_t i = 0; i < nbat; ++i) {
            const batch_plan::Step st = batch_plan::step_of(i, nbat, stride, base);
            ivfadc_index *ln = st.lane ? lane2 : h;
            TRY(upload_until(st.on_their_way));
            hipEvent_t ev = nullptr;
            TRY(pending_event(st.lane, i, ev));   // this batch's own rows: before the search's first launch
            if (i >= stride) TRY(host_wait(ev));  // (the first search of a lane must start the moment its rows land: its wait goes into the stream)
            if (ev) HIP_TRY(hipStreamWaitEvent(ln->stream, ev, 0));
            ln->cur_token = st.token;             // batch i's rows, if any stand, were hinted with this very token by the lane's step before
            ln->hint_ev = nullptr;
            if (st.has_next) {
                ln->hint_q = all.slice(bt.start[st.next], bt.cnt[st.next]).q;
                ln->hint_nq = bt.cnt[st.next];
                ln->hint_token = st.next_token;
                TRY(pending_event(st.lane, st.next, ev));   // (read by this search's riders only: waited for in front of the scan launch)
                if (i >= stride) TRY(host_wait(ev));
                ln->hint_ev = ev;
            }
            SearchCall cb = all.slice(bt.start[i], bt.cnt[i]);
            cb.whole_batch = true;   // (of its lane's search: the hint names its successor)
            TRY(search_dev(ln, cb));
        }
        return IVFADC_OK;
    }
};

int ivfadc_search_batches(ivfadc_t *h, int nbatches, const int64_t *batch_nq, const float *queries, int K, int w, uint32_t *out_ids,
                          float *out_dists, int32_t *out_counts)
try {
    HandleLock lk_(h);
    if (nbatches < 0 || (nbatches > 0 && !batch_nq)) return fail(IVFADC_ERR_INVALID, "nbatches < 0 or null batch sizes");
    batch_plan::Batches bt;
    const int bad = batch_plan::non_empty_batches(batch_nq, nbatches, bt);
    if (bad >= 0) return fail(IVFADC_ERR_INVALID, "batch %d: nq < 0", bad);
    TRY(check_search_args(h, bt.total, K, w));
    if (bt.total == 0) return IVFADC_OK;
    if (!queries || !out_ids || !out_dists || !out_counts) return fail(IVFADC_ERR_INVALID, "null buffer");
    TRY(set_device(h));
    HostClock clk;
    const size_t nbat = bt.size(), qbytes = (size_t)bt.total * h->d * 4;
    const SearchCall hc{bt.total, h->d, K, w, queries, out_ids, out_dists, out_counts};   // the run as the caller has it
    TRY(h->q_stage.ensure(qbytes));
    const uint8_t *qsrc = nullptr;
    TRY(stage_queries(h, queries, qbytes, 0, 0, qsrc));   // (decided here; pin_in is filled group by group)
    SearchCall all = hc;
    all.q = h->q_stage.as<float>();
    TRY(stage_results(h, all));
    h->hstats.calls++;
    h->hstats.queries_direct += qsrc == (const uint8_t *)queries;
    h->hstats.results_direct += h->hc_out_direct;
    h->hstats.batches += (int64_t)nbat;
    const uint64_t base = h->own_token;
    h->own_token += nbat;
    ivfadc_index *lane2;
    TRY(setup_batch_lanes(h, nbat, lane2));
    BatchDrain drain{h, lane2, true};
    const batch_plan::Groups gr = batch_plan::upload_groups(nbat, lane2 ? 2 : 1);
    while (h->ingest_ev.size() < gr.size()) {
        hipEvent_t e;
        HIP_TRY(hipEventCreateWithFlags(&e, hipEventDisableTiming));
        h->ingest_ev.push_back(e);
    }
    BatchRun run{h, lane2, bt, gr, queries, qsrc, all, base, batch_plan::IngestTracker(gr)};
    TRY(run.issue());
    const double t_issue = clk.lap();
    if (lane2) TRY(wait_stream(lane2));
    TRY(wait_stream(h));
    drain.armed = false;   // (the copy lane's work ended before the searches that read it)
    const double t_wait = clk.lap();
    if (!h->hc_out_direct) copy_out(hc, h->pin_out.p, hc.nq);
    h->hstats.stage_in_us += run.t_stage;
    h->hstats.enqueue_us += t_issue - run.t_stage;
    h->hstats.wait_us += t_wait;
    h->hstats.stage_out_us += clk.lap();
    return IVFADC_OK;
} IVF_CATCH

// ---- single-process multi-device front end: index replicated, contiguous query blocks per device -------------
// (queries are independent, index.jl:269-271.)  Result merge: by default every device's block is
// copied to the caller's host arrays as it completes; with ivfadc_mg_set_gather(g, 1) the packed per-device blocks are
// exchanged by ONE ncclAllGather (RCCL over xGMI, ncclCommInitAll, one stream per device) so that every device holds the
// whole batch's results, and the host reads device 0's copy.  RCCL is bound at run time (dlopen), so the library loads
// on hosts without it and in processes where torch has already loaded its own copy.
extern "C++" {
struct RcclApi {
    void *lib = nullptr;
    decltype(&ncclCommInitAll) CommInitAll = nullptr;
    decltype(&ncclCommDestroy) CommDestroy = nullptr;
    decltype(&ncclAllGather) AllGather = nullptr;
    decltype(&ncclGroupStart) GroupStart = nullptr;
    decltype(&ncclGroupEnd) GroupEnd = nullptr;
    decltype(&ncclGetErrorString) GetErrorString = nullptr;
    decltype(&ncclGetUniqueId) GetUniqueId = nullptr;
    decltype(&ncclCommInitRank) CommInitRank = nullptr;
    bool ok = false;
};

static RcclApi &rccl_api()
{
    static RcclApi api;
    static std::once_flag once;
    std::call_once(once, [] {
        for (const char *name : {"librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1"}) {
            api.lib = dlopen(name, RTLD_NOW | RTLD_LOCAL);
            if (api.lib) break;
        }
        if (!api.lib) return;
        api.CommInitAll = (decltype(api.CommInitAll))dlsym(api.lib, "ncclCommInitAll");
        api.CommDestroy = (decltype(api.CommDestroy))dlsym(api.lib, "ncclCommDestroy");
        api.AllGather = (decltype(api.AllGather))dlsym(api.lib, "ncclAllGather");
        api.GroupStart = (decltype(api.GroupStart))dlsym(api.lib, "ncclGroupStart");
        api.GroupEnd = (decltype(api.GroupEnd))dlsym(api.lib, "ncclGroupEnd");
        api.GetErrorString = (decltype(api.GetErrorString))dlsym(api.lib, "ncclGetErrorString");
        api.GetUniqueId = (decltype(api.GetUniqueId))dlsym(api.lib, "ncclGetUniqueId");
        api.CommInitRank = (decltype(api.CommInitRank))dlsym(api.lib, "ncclCommInitRank");
        api.ok = api.GetUniqueId && api.CommInitRank && api.CommInitAll && api.CommDestroy && api.AllGather && api.GroupStart && api.GroupEnd && api.GetErrorString;
    });
    return api;
}

#define NCCL_TRY(expr)                                                                                      \
    do {                                                                                                    \
        ncclResult_t r_ = (expr);                                                                           \
        if (r_ != ncclSuccess) return fail(IVFADC_ERR_HIP, "%s failed: %s", #expr, rccl_api().GetErrorString(r_)); \
    } while (0)

struct ivfadc_mg {
    std::recursive_mutex mu;             // calls on one multi-device handle are serialised (its replicas are only reached through it)
    std::vector<ivfadc_t *> dev;
    int gather_mode = 0;                 // 0: host gather; 1: ncclAllGather of the packed blocks
    std::vector<ncclComm_t> comms;       // one per device (gather_mode 1)
    std::vector<DevBuf> gath;            // per device: the gathered [G][block] results
    PinnedBuf host_gath;
    int64_t collectives = 0;             // statistics: all-gathers issued
};

// run f(r) for every replica on its own host thread (uploads and device-side synthesis of the replicas overlap);
// returns the first failure, with its message
template <class F> static int mg_parallel(ivfadc_mg *g, F f)
{
    const size_t G = g->dev.size();
    std::vector<int> rc(G, IVFADC_OK);
    std::vector<std::string> msg(G);
    std::vector<std::thread> th;
    for (size_t r = 0; r < G; ++r)
        th.emplace_back([&, r] {
            try { rc[r] = f(r); } catch (...) { rc[r] = on_exception(); }
            if (rc[r] != IVFADC_OK) msg[r] = g_err;   // g_err is thread-local
        });
    for (auto &t : th) t.join();
    for (size_t r = 0; r < G; ++r)
        if (rc[r] != IVFADC_OK) { g_err = msg[r]; return rc[r]; }
    return IVFADC_OK;
}

}  // extern "C++"

int ivfadc_mg_create(ivfadc_mg_t **out, int ndev, const int *devices, int d, int kc, int m, int ksub, const float *centroids,
                     const float *codebooks, const uint8_t *code_labels)
try {
    if (!out) return fail(IVFADC_ERR_INVALID, "out is null");
    *out = nullptr;
    if (ndev < 1 || !devices) return fail(IVFADC_ERR_INVALID, "ndev must be >= 1");
    ivfadc_mg *g = new ivfadc_mg();
    for (int r = 0; r < ndev; ++r) {
        ivfadc_t *h = nullptr;
        const int rc = ivfadc_create(&h, devices[r], d, kc, m, ksub, centroids, codebooks, code_labels);
        if (rc != IVFADC_OK) { ivfadc_mg_destroy(g); return rc; }
        g->dev.push_back(h);
    }
    g->gath.resize((size_t)ndev);
    *out = g;
    return IVFADC_OK;
} IVF_CATCH

void ivfadc_mg_destroy(ivfadc_mg_t *g)
{
    if (!g) return;
    for (size_t r = 0; r < g->comms.size(); ++r)
        if (g->comms[r]) { (void)hipSetDevice(g->dev[r]->device); (void)rccl_api().CommDestroy(g->comms[r]); }
    for (size_t r = 0; r < g->gath.size(); ++r) {
        if (r < g->dev.size()) (void)hipSetDevice(g->dev[r]->device);
        g->gath[r].release();
    }
    g->host_gath.release();
    for (ivfadc_t *h : g->dev) ivfadc_destroy(h);
    delete g;
}

int ivfadc_mg_num_devices(ivfadc_mg_t *g) { return g ? (int)g->dev.size() : 0; }

int ivfadc_mg_set_gather(ivfadc_mg_t *g, int mode)
try {
    std::unique_lock<std::recursive_mutex> lkg_;
    if (g) lkg_ = std::unique_lock<std::recursive_mutex>(g->mu);
    if (!g) return fail(IVFADC_ERR_INVALID, "null handle");
    if (mode != 0 && mode != 1) return fail(IVFADC_ERR_INVALID, "mode must be 0 (host gather) or 1 (RCCL all-gather)");
    if (mode == 1 && g->comms.empty()) {
        RcclApi &api = rccl_api();
        if (!api.ok) return fail(IVFADC_ERR_STATE, "librccl.so could not be loaded");
        std::vector<int> devs;
        for (ivfadc_t *h : g->dev) devs.push_back(h->device);
        std::vector<int> srt(devs);
        std::sort(srt.begin(), srt.end());
        if (std::adjacent_find(srt.begin(), srt.end()) != srt.end())
            return fail(IVFADC_ERR_INVALID, "RCCL needs distinct devices (a device is listed twice)");
        std::vector<ncclComm_t> comms(devs.size(), nullptr);
        NCCL_TRY(api.CommInitAll(comms.data(), (int)devs.size(), devs.data()));
        g->comms.swap(comms);
    }
    g->gather_mode = mode;
    return IVFADC_OK;
} IVF_CATCH

int ivfadc_mg_collectives(ivfadc_mg_t *g, int64_t *out)
{
    if (!g || !out) return fail(IVFADC_ERR_INVALID, "null argument");
    *out = g->collectives;
    return IVFADC_OK;
}

int ivfadc_mg_set_lists(ivfadc_mg_t *g, const int64_t *offsets, const uint8_t *codes, const uint32_t *ids)
try {
    std::unique_lock<std::recursive_mutex> lkg_;
    if (g) lkg_ = std::unique_lock<std::recursive_mutex>(g->mu);
    if (!g) return fail(IVFADC_ERR_INVALID, "null handle");
    return mg_parallel(g, [&](size_t r) { return ivfadc_set_lists(g->dev[r], offsets, codes, ids); });
} IVF_CATCH

int ivfadc_mg_synth_lists(ivfadc_mg_t *g, const int64_t *offsets, uint64_t seed)
try {
    std::unique_lock<std::recursive_mutex> lkg_;
    if (g) lkg_ = std::unique_lock<std::recursive_mutex>(g->mu);
    if (!g) return fail(IVFADC_ERR_INVALID, "null handle");
    return mg_parallel(g, [&](size_t r) { return ivfadc_synth_lists(g->dev[r], offsets, seed); });
} IVF_CATCH

// Mutators: a replica that fails does not stop the others -- every replica's host mirror takes the same edit (the
// mirrors never diverge) and a replica whose device-side update failed is left marked stale (re-laid out by its next
// search).  The first failure is reported.
int ivfadc_mg_append(ivfadc_mg_t *g, int64_t nnew, const float *pts, const uint32_t *ids, int32_t *out_list, uint8_t *out_codes)
try {
    std::unique_lock<std::recursive_mutex> lkg_;
    if (g) lkg_ = std::unique_lock<std::recursive_mutex>(g->mu);
    if (!g || g->dev.empty()) return fail(IVFADC_ERR_INVALID, "null handle");
    for (ivfadc_t *h : g->dev) TRY(append_check(h, nnew, pts, ids));   // nothing has changed yet if a check fails
    if (nnew == 0) return IVFADC_OK;
    ivfadc_t *h0 = g->dev[0];
    TRY(set_device(h0));
    std::vector<int32_t> lst((size_t)nnew);
    std::vector<uint8_t> cod((size_t)nnew * h0->m);
    TRY(encode_dev(h0, nnew, pts, lst.data(), cod.data()));             // one encode: every replica appends the same codes
    int first = IVFADC_OK;
    std::string first_msg;
    for (ivfadc_t *h : g->dev) {
        const int rc = append_encoded(h, nnew, lst.data(), cod.data(), ids);
        if (rc != IVFADC_OK && first == IVFADC_OK) { first = rc; first_msg = g_err; }
    }
    if (out_list) memcpy(out_list, lst.data(), (size_t)nnew * 4);
    if (out_codes) memcpy(out_codes, cod.data(), (size_t)nnew * h0->m);
    if (first != IVFADC_OK) g_err = first_msg;
    return first;
} IVF_CATCH

int ivfadc_mg_delete_ids(ivfadc_mg_t *g, int64_t ndel, const uint32_t *ids, int64_t *out_removed)
try {
    std::unique_lock<std::recursive_mutex> lkg_;
    if (g) lkg_ = std::unique_lock<std::recursive_mutex>(g->mu);
    if (!g) return fail(IVFADC_ERR_INVALID, "null handle");
    int first = IVFADC_OK;
    std::string first_msg;
    for (size_t r = 0; r < g->dev.size(); ++r) {
        const int rc = ivfadc_delete_ids(g->dev[r], ndel, ids, r == 0 ? out_removed : nullptr);
        if (rc != IVFADC_OK && first == IVFADC_OK) { first = rc; first_msg = g_err; }
    }
    if (first != IVFADC_OK) g_err = first_msg;
    return first;
} IVF_CATCH

int ivfadc_mg_shift_ids(ivfadc_mg_t *g, int32_t delta)
try {
    std::unique_lock<std::recursive_mutex> lkg_;
    if (g) lkg_ = std::unique_lock<std::recursive_mutex>(g->mu);
    if (!g) return fail(IVFADC_ERR_INVALID, "null handle");
    int first = IVFADC_OK;
    std::string first_msg;
    for (ivfadc_t *h : g->dev) {
        const int rc = ivfadc_shift_ids(h, delta);
        if (rc != IVFADC_OK && first == IVFADC_OK) { first = rc; first_msg = g_err; }
    }
    if (first != IVFADC_OK) g_err = first_msg;
    return first;
} IVF_CATCH

int ivfadc_mg_search(ivfadc_mg_t *g, int64_t nq, const float *queries, int K, int w, uint32_t *out_ids, float *out_dists,
                     int32_t *out_counts)
try {
    std::unique_lock<std::recursive_mutex> lkg_;
    if (g) lkg_ = std::unique_lock<std::recursive_mutex>(g->mu);
    if (!g || g->dev.empty()) return fail(IVFADC_ERR_INVALID, "null handle");
    int wc = w;
    TRY(check_search_args(g->dev[0], nq, K, wc));
    if (nq == 0) return IVFADC_OK;
    if (!queries || !out_ids || !out_dists || !out_counts) return fail(IVFADC_ERR_INVALID, "null buffer");
    const int64_t G = (int64_t)g->dev.size();
    const int d = g->dev[0]->d;
    const SearchCall all{nq, d, K, w, queries, out_ids, out_dists, out_counts};   // (host memory: every device takes a slice)
    if (g->gather_mode == 0) {
        // enqueue every device's block, then collect: the devices run concurrently
        for (int64_t r = 0; r < G; ++r) {
            const int64_t a = batch_plan::mg_lo(r, nq, G), b = batch_plan::mg_lo(r + 1, nq, G);
            if (b <= a) continue;
            const int rc = search_enqueue(g->dev[r], all.slice(a, b - a));
            if (rc != IVFADC_OK) {
                // the devices before r (and r itself, up to the failure) are writing the caller's arrays or the staging blocks: they end first
                const std::string msg = g_err;
                for (int64_t q = 0; q <= r; ++q)
                    if (hipSetDevice(g->dev[q]->device) == hipSuccess) (void)hipStreamSynchronize(g->dev[q]->stream);
                g_err = msg;
                return rc;
            }
        }
        for (int64_t r = 0; r < G; ++r) {
            const int64_t a = batch_plan::mg_lo(r, nq, G), b = batch_plan::mg_lo(r + 1, nq, G);
            if (b > a) TRY(search_finish(g->dev[r], all.slice(a, b - a)));
        }
        return IVFADC_OK;
    }
    // RCCL: every device leaves its packed block [ids nql*K | dists nql*K | counts nql] (nql = ceil(nq / G): equal
    // blocks, the collective's contract) in device memory; ONE all-gather per batch; the host reads device 0's copy
    RcclApi &api = rccl_api();
    const int64_t nql = (nq + G - 1) / G;
    const batch_plan::ResultBlock blk = batch_plan::result_words((size_t)nql, (size_t)K);   // (in 32-bit words, the collective's unit)
    const size_t blk_words = blk.total;
    // a failure on device r must not leave devices 0 .. r-1 with work in flight that nothing waits for, nor an RCCL group open (the
    // next collective of the process would be absorbed into it): remember the first failure, finish the bookkeeping, then report
    int first_rc = IVFADC_OK;
    std::string first_msg;
    auto note = [&](int rc) {
        if (rc != IVFADC_OK && first_rc == IVFADC_OK) { first_rc = rc; first_msg = g_err; }
    };
    int64_t enq = 0;
    for (int64_t r = 0; r < G && first_rc == IVFADC_OK; ++r) {
        ivfadc_t *h = g->dev[r];
        const int64_t a = batch_plan::mg_lo(r, nq, G), b = batch_plan::mg_lo(r + 1, nq, G);
        auto one = [&]() -> int {
            TRY(set_device(h));
            TRY(h->out_ids.ensure(blk_words * 4));
            TRY(g->gath[r].ensure(blk_words * 4 * (size_t)G));
            if (b > a) {
                const size_t qbytes = (size_t)(b - a) * d * 4;
                TRY(h->q_stage.ensure(qbytes));
                const float *rows = all.slice(a, b - a).q;
                const uint8_t *src = nullptr;
                TRY(stage_queries(h, rows, qbytes, 0, qbytes, src));
                TRY(ingest_rows(h, h->stream, src, h->q_stage.p, qbytes));
                uint32_t *o = h->out_ids.as<uint32_t>();
                TRY(search_dev(h, SearchCall{b - a, d, K, w, h->q_stage.as<float>(), o + blk.ids, (float *)(o + blk.dists), (int32_t *)(o + blk.counts)}));
            }
            return IVFADC_OK;
        };
        note(one());
        enq = r + 1;
    }
    if (first_rc != IVFADC_OK) {
        for (int64_t r = 0; r < enq; ++r)
            if (hipSetDevice(g->dev[r]->device) == hipSuccess) (void)hipStreamSynchronize(g->dev[r]->stream);
        g_err = first_msg;
        return first_rc;
    }
    NCCL_TRY(api.GroupStart());
    for (int64_t r = 0; r < G; ++r) {
        ivfadc_t *h = g->dev[r];
        auto one = [&]() -> int {
            TRY(set_device(h));
            NCCL_TRY(api.AllGather(h->out_ids.p, g->gath[r].p, blk_words, ncclInt32, g->comms[r], h->stream));
            return IVFADC_OK;
        };
        note(one());
    }
    {
        const ncclResult_t ge = api.GroupEnd();   // always closed, whatever happened inside
        if (ge != ncclSuccess && first_rc == IVFADC_OK) note(fail(IVFADC_ERR_HIP, "ncclGroupEnd failed: %s", api.GetErrorString(ge)));
    }
    if (first_rc != IVFADC_OK) {
        for (int64_t r = 0; r < G; ++r)
            if (hipSetDevice(g->dev[r]->device) == hipSuccess) (void)hipStreamSynchronize(g->dev[r]->stream);
        g_err = first_msg;
        return first_rc;
    }
    g->collectives++;
    ivfadc_t *h0 = g->dev[0];
    TRY(set_device(h0));
    TRY(g->host_gath.ensure(blk_words * 4 * (size_t)G));
    HIP_TRY(hipMemcpyAsync(g->host_gath.p, g->gath[0].p, blk_words * 4 * (size_t)G, hipMemcpyDeviceToHost, h0->stream));
    for (int64_t r = 0; r < G; ++r) {   // every device's stream: the collective has finished everywhere before we return
        TRY(set_device(g->dev[r]));
        TRY(wait_stream(g->dev[r]));
    }
    const uint32_t *hg = (const uint32_t *)g->host_gath.p;
    for (int64_t r = 0; r < G; ++r) {
        const int64_t a = batch_plan::mg_lo(r, nq, G), b = batch_plan::mg_lo(r + 1, nq, G);
        copy_out(all.slice(a, b - a), hg + (size_t)r * blk_words, nql);
    }
    return IVFADC_OK;
} IVF_CATCH

// ---- one process per GPU: the final top-k merge of a batch inside the library ------------------------------------------------
// (query batches partitioned across the GPUs of a node, index replicated, RCCL over xGMI only for the final
// merge.)  Every rank owns one handle on its GPU and a contiguous block of the batch's queries.  ivfadc_comm_init joins the
// ranks in an RCCL communicator (ncclCommInitRank; the 128-byte id comes from rank 0's ivfadc_comm_unique_id and travels
// by whatever the host framework uses to talk: torch.distributed's store, MPI, a file);
// ivfadc_search_device_allgather then searches the rank's block and issues ONE ncclAllGather of the packed result block on a
// side stream of the handle -- a few microseconds of host time per batch where a framework-level collective costs tens -- so
// the collective of batch i overlaps the kernels of batch i + 1.  `slot` names one of COMM_SLOTS result buffers in
// flight: a slot's previous collective is waited for (on the device) before the slot is reused.
int ivfadc_comm_unique_id(uint8_t *out_id128)
try {
    if (!out_id128) return fail(IVFADC_ERR_INVALID, "null argument");
    RcclApi &api = rccl_api();
    if (!api.ok) return fail(IVFADC_ERR_STATE, "librccl.so could not be loaded");
    ncclUniqueId id;
    NCCL_TRY(api.GetUniqueId(&id));
    static_assert(sizeof(id) == 128, "ncclUniqueId is 128 bytes");
    memcpy(out_id128, &id, sizeof(id));
    return IVFADC_OK;
} IVF_CATCH

int ivfadc_comm_destroy(ivfadc_t *h)
try {
    HandleLock lk_(h);
    if (!h) return fail(IVFADC_ERR_INVALID, "null handle");
    TRY(set_device(h));
    if (h->comm_stream) (void)hipStreamSynchronize(h->comm_stream);
    if (h->comm) { (void)rccl_api().CommDestroy((ncclComm_t)h->comm); h->comm = nullptr; }
    for (int i = 0; i < ivfadc_index::COMM_SLOTS; ++i)
        if (h->comm_done[i]) { (void)hipEventDestroy(h->comm_done[i]); h->comm_done[i] = nullptr; h->comm_busy[i] = false; }
    for (int i = 0; i < ivfadc_index::COMM_SLOTS; ++i) h->comm_slot_seq[i] = 0;   // (comm_seq stays: views compare their comm_waited with it)
    if (h->comm_ready) { (void)hipEventDestroy(h->comm_ready); h->comm_ready = nullptr; }
    if (h->comm_stream) { (void)hipStreamDestroy(h->comm_stream); h->comm_stream = nullptr; }
    h->comm_ranks = 0;
    return IVFADC_OK;
} IVF_CATCH

int ivfadc_comm_init(ivfadc_t *h, int nranks, int rank, const uint8_t *id128)
try {
    HandleLock lk_(h);
    if (!h || !id128) return fail(IVFADC_ERR_INVALID, "null argument");
    if (nranks < 1 || rank < 0 || rank >= nranks) return fail(IVFADC_ERR_INVALID, "rank %d of %d", rank, nranks);
    RcclApi &api = rccl_api();
    if (!api.ok) return fail(IVFADC_ERR_STATE, "librccl.so could not be loaded");
    if (h->comm) TRY(ivfadc_comm_destroy(h));
    TRY(set_device(h));
    ncclUniqueId id;
    memcpy(&id, id128, sizeof(id));
    ncclComm_t comm = nullptr;
    NCCL_TRY(api.CommInitRank(&comm, nranks, id, rank));
    h->comm = (void *)comm;
    h->comm_ranks = nranks;
    h->comm_rank = rank;
    auto rest = [&]() -> int {
        HIP_TRY(hipStreamCreateWithFlags(&h->comm_stream, hipStreamNonBlocking));
        // search -> collective: the event orders the search's writes to the send block before the all-gather, and a PEER GPU may read that
        // block directly over xGMI (RCCL's P2P-read and registered-buffer paths), so the record carries its system-scope release.  The
        // relaxed form (no system fence: 2-3 us less per step, measured with a single-rank communicator only) waits for a run with >= 2
        // ranks that passes bench.py's gather_check with it.
        HIP_TRY(hipEventCreateWithFlags(&h->comm_ready, hipEventDisableTiming));
        for (int i = 0; i < ivfadc_index::COMM_SLOTS; ++i) HIP_TRY(hipEventCreateWithFlags(&h->comm_done[i], hipEventDisableTiming));
        return IVFADC_OK;
    };
    const int rc = rest();
    if (rc != IVFADC_OK) {   // no half-initialised communicator is left behind
        const std::string msg = g_err;
        (void)ivfadc_comm_destroy(h);
        g_err = msg;
    }
    return rc;
} IVF_CATCH

int ivfadc_search_device_allgather(ivfadc_t *h, int64_t nq, const float *d_queries, int K, int w, int32_t *d_block, int32_t *d_gathered,
                                   int slot)
{
    return ivfadc_search_device_allgather_on(h, h, nq, d_queries, K, w, d_block, d_gathered, slot);
}

// The same with the SEARCH on `searcher` -- h itself or a view of it (two batches in flight per rank) -- and the collective where the
// communicator lives: on h's side stream, in call order, so every rank issues its all-gathers in the same order whatever the lanes do.
int ivfadc_search_device_allgather_on(ivfadc_t *h, ivfadc_t *searcher, int64_t nq, const float *d_queries, int K, int w, int32_t *d_block,
                                      int32_t *d_gathered, int slot)
try {
    HandleLock lk_(h);
    HandleLock lk2_(searcher != h ? searcher : nullptr);
    if (!h || !searcher) return fail(IVFADC_ERR_INVALID, "null handle");
    if (searcher != h && searcher->view_of != h) return fail(IVFADC_ERR_INVALID, "searcher must be the handle itself or a view of it");
    TRY(check_search_args(searcher, nq, K, w));
    if (!h->comm) return fail(IVFADC_ERR_STATE, "ivfadc_comm_init has not been called");
    if (slot < 0 || slot >= ivfadc_index::COMM_SLOTS) return fail(IVFADC_ERR_INVALID, "slot must be in [0, %d)", ivfadc_index::COMM_SLOTS);
    if (nq < 1 || !d_queries || !d_block || !d_gathered) return fail(IVFADC_ERR_INVALID, "null buffer / empty block");
    // ncclAllGather moves EQUAL blocks: every rank must pass the same nq and K within one call (a different count on one rank hangs the
    // collective or overruns d_gathered); nothing a single rank sees can detect a mismatch, so it is the caller's contract.  The
    // block size may change from call to call (a ragged final batch, another K) as long as every rank changes it alike, and
    // d_gathered must hold nranks x nq x (2K + 1) words.
    TRY(set_device(h));
    // The slot's buffers were read by its previous collective: that must have finished before the search overwrites them.  A wait in the
    // search stream costs the NEXT kernel ~6 us of idle queue, fired event or not (measured), so one wait serves several steps: it names
    // the newest collective that is at least COMM_SLOTS / 2 behind the head (never an older one than needed) -- collectives finish in
    // order, so every earlier one is covered -- and with the slots in rotation the next few searches find theirs already waited for.
    {
        const int64_t need = h->comm_slot_seq[slot];
        if (need > searcher->comm_waited) {
            const int64_t target = std::max<int64_t>(need, h->comm_seq - ivfadc_index::COMM_SLOTS / 2);
            int ts = slot;
            for (int i = 0; i < ivfadc_index::COMM_SLOTS; ++i)
                if (h->comm_slot_seq[i] == target) ts = i;
            HIP_TRY(hipStreamWaitEvent(searcher->stream, h->comm_done[ts], 0));
            searcher->comm_waited = h->comm_slot_seq[ts];
        }
    }
    uint32_t *ids = (uint32_t *)d_block;
    TRY(search_dev(searcher, SearchCall{nq, searcher->d, K, w, d_queries, ids, (float *)(ids + (size_t)nq * K), (int32_t *)(ids + 2 * (size_t)nq * K)}));
    HIP_TRY(hipEventRecord(h->comm_ready, searcher->stream));
    HIP_TRY(hipStreamWaitEvent(h->comm_stream, h->comm_ready, 0));
    RcclApi &api = rccl_api();
    NCCL_TRY(api.AllGather(d_block, d_gathered, (size_t)nq * (2 * (size_t)K + 1), ncclInt32, (ncclComm_t)h->comm, h->comm_stream));
    HIP_TRY(hipEventRecord(h->comm_done[slot], h->comm_stream));
    h->comm_busy[slot] = true;
    h->comm_slot_seq[slot] = ++h->comm_seq;
    h->comm_collectives++;
    return IVFADC_OK;
} IVF_CATCH

// List-partitioned step in ONE call (one process per GPU): partial search of ALL nq queries over this rank's lists into d_block
// ([keys nq x K u64 | counts nq i32], ivfadc_listpart_block_words(nq, K) int32 words), ONE ncclAllGather of the blocks into d_gathered
// (nranks blocks, rank order), then the K-way merge of the ranks' keys on this rank: every rank ends with the batch's full results.
// ivfadc_set_list_partition(h, nranks, rank) and ivfadc_comm_init first.
int64_t ivfadc_listpart_block_words(int64_t nq, int K) { return ((nq * (2 * (int64_t)K + 1)) + 1) & ~(int64_t)1; }

int ivfadc_search_device_listpart(ivfadc_t *h, int64_t nq, const float *d_queries, int K, int w, int32_t *d_block, int32_t *d_gathered,
                                  uint32_t *d_ids, float *d_dists, int32_t *d_counts)
try {
    HandleLock lk_(h);
    TRY(check_search_args(h, nq, K, w));
    if (!h->comm) return fail(IVFADC_ERR_STATE, "ivfadc_comm_init has not been called");
    if (h->part_n != h->comm_ranks || h->part_i != h->comm_rank)
        return fail(IVFADC_ERR_STATE, "ivfadc_set_list_partition(h, %d, %d) must name this rank of the communicator", h->comm_ranks, h->comm_rank);
    if (nq < 1 || !d_queries || !d_block || !d_gathered || !d_ids || !d_dists || !d_counts) return fail(IVFADC_ERR_INVALID, "null buffer / empty batch");
    const size_t words = (size_t)ivfadc_listpart_block_words(nq, K);
    uint64_t *keys = (uint64_t *)d_block;
    int32_t *cnts = d_block + (size_t)nq * K * 2;
    if (h->comm_ranks == 1) {
        // one rank owns every list: an ordinary search (ids straight away), no collective
        return ivfadc_search_device(h, nq, d_queries, K, w, d_ids, d_dists, d_counts);
    }
    TRY(ivfadc_search_device_partial(h, nq, d_queries, K, w, keys, cnts));
    HIP_TRY(hipEventRecord(h->comm_ready, h->stream));
    HIP_TRY(hipStreamWaitEvent(h->comm_stream, h->comm_ready, 0));
    RcclApi &api = rccl_api();
    NCCL_TRY(api.AllGather(d_block, d_gathered, words, ncclInt32, (ncclComm_t)h->comm, h->comm_stream));
    HIP_TRY(hipEventRecord(h->comm_done[0], h->comm_stream));
    HIP_TRY(hipStreamWaitEvent(h->stream, h->comm_done[0], 0));
    h->comm_collectives++;
    return merge_partials_dev(h, nq, K, h->comm_ranks, (const uint64_t *)d_gathered, words / 2, d_gathered + (size_t)nq * K * 2, words, d_ids, d_dists,
                              d_counts);
} IVF_CATCH

// makes the handle's search stream wait (on the device) for every collective issued so far; returns how many were issued
int ivfadc_comm_wait(ivfadc_t *h, int64_t *out_collectives)
try {
    HandleLock lk_(h);
    if (!h) return fail(IVFADC_ERR_INVALID, "null handle");
    TRY(set_device(h));
    // (the newest one covers them all: they finish in issue order)
    if (h->comm_seq > h->comm_waited) {
        for (int i = 0; i < ivfadc_index::COMM_SLOTS; ++i)
            if (h->comm_slot_seq[i] == h->comm_seq) HIP_TRY(hipStreamWaitEvent(h->stream, h->comm_done[i], 0));
        h->comm_waited = h->comm_seq;
    }
    for (int i = 0; i < ivfadc_index::COMM_SLOTS; ++i) h->comm_busy[i] = false;
    if (out_collectives) *out_collectives = h->comm_collectives;
    return IVFADC_OK;
} IVF_CATCH

int ivfadc_sync(ivfadc_t *h)
try {
    HandleLock lk_(h);
    if (!h) return fail(IVFADC_ERR_INVALID, "null handle");
    TRY(set_device(h));
    HIP_TRY(hipStreamSynchronize(h->stream));
    return IVFADC_OK;
} IVF_CATCH

int ivfadc_set_stream(ivfadc_t *h, void *stream)
try {
    HandleLock lk_(h);
    if (!h) return fail(IVFADC_ERR_INVALID, "null handle");
    TRY(set_device(h));
    TRY(ev_fold(h));
    HIP_TRY(hipStreamSynchronize(h->stream));
    if (h->own_stream && h->stream) (void)hipStreamDestroy(h->stream);
    h->stream = (hipStream_t)stream;
    h->own_stream = false;
    return IVFADC_OK;
} IVF_CATCH

int ivfadc_ntotal(ivfadc_t *h, int64_t *out_n, int64_t *list_sizes)
try {
    HandleLock lk_(h);
    if (!h) return fail(IVFADC_ERR_INVALID, "null handle");
    if (out_n) *out_n = h->mirror.ntotal();
    if (list_sizes)
        for (int l = 0; l < h->kc; ++l) list_sizes[l] = h->mirror.h_len[l];
    return IVFADC_OK;
} IVF_CATCH

static int get_lists_entry(ivfadc_index *h, int64_t *offsets, void *codes, uint32_t *ids, bool wide)
{
    if (!h) return fail(IVFADC_ERR_INVALID, "null handle");
    TRY(check_width(h, wide, "ivfadc_get_lists"));
    if (h->is_view) return fail(IVFADC_ERR_STATE, "a view keeps no host mirror of the lists");
    if (h->synthetic) return fail(IVFADC_ERR_STATE, "device-synthesised lists keep no host mirror");
    h->mirror.gather(offsets, (uint8_t *)codes, ids, h->cb);
    if (wide && codes) h->labmap.to_labels(h->mirror.ntotal(), codes);   // codeword indices -> labels
    return IVFADC_OK;
}

int ivfadc_get_lists(ivfadc_t *h, int64_t *offsets, uint8_t *codes, uint32_t *ids)
try {
    HandleLock lk_(h);
    return get_lists_entry(h, offsets, codes, ids, false);
} IVF_CATCH

int ivfadc_get_lists_u16(ivfadc_t *h, int64_t *offsets, void *codes, uint32_t *ids)
try {
    HandleLock lk_(h);
    return get_lists_entry(h, offsets, codes, ids, true);
} IVF_CATCH

int ivfadc_get_dims(ivfadc_t *h, int *d, int *kc, int *m, int *ksub)
try {
    HandleLock lk_(h);
    if (!h) return fail(IVFADC_ERR_INVALID, "null handle");
    if (d) *d = h->d;
    if (kc) *kc = h->kc;
    if (m) *m = h->m;
    if (ksub) *ksub = h->ksub;
    return IVFADC_OK;
} IVF_CATCH

static int get_quantizers_entry(ivfadc_index *h, float *centroids, float *codebooks, void *code_labels, bool wide)
{
    if (!h) return fail(IVFADC_ERR_INVALID, "null handle");
    TRY(check_width(h, wide, "ivfadc_get_quantizers"));
    TRY(set_device(h));
    HIP_TRY(hipStreamSynchronize(h->stream));
    if (centroids) TRY(d2h_copy(centroids, h->centroids.p, (size_t)h->d * h->kc * 4, h->stream));
    if (codebooks) TRY(d2h_copy(codebooks, h->codebooks.p, (size_t)h->d * h->ksub * 4, h->stream));
    if (code_labels && wide) memcpy(code_labels, h->labmap.lab16.data(), h->labmap.lab16.size() * 2);
    if (code_labels && !wide) HIP_TRY(hipMemcpy(code_labels, h->labels.p, (size_t)h->m * h->ksub, hipMemcpyDeviceToHost));
    return IVFADC_OK;
}

int ivfadc_get_quantizers(ivfadc_t *h, float *centroids, float *codebooks, uint8_t *code_labels)
try {
    HandleLock lk_(h);
    return get_quantizers_entry(h, centroids, codebooks, code_labels, false);
} IVF_CATCH

int ivfadc_get_quantizers_u16(ivfadc_t *h, float *centroids, float *codebooks, void *code_labels)
try {
    HandleLock lk_(h);
    return get_quantizers_entry(h, centroids, codebooks, code_labels, true);
} IVF_CATCH

int ivfadc_abi_version(void) { return IVFADC_ABI_VERSION; }

// ---- page-locked host memory the kernels address directly (see "host-pointer entries") -------------------------------------------
static int host_range_add(void *p, size_t bytes, bool owned)
{
    const uintptr_t a = (uintptr_t)p, b = a + bytes;
    std::lock_guard<std::mutex> lk(g_host_mu);
    for (const HostRange &r : g_host_ranges)
        if (a < r.hi && b > r.lo) return fail(IVFADC_ERR_INVALID, "host range overlaps one that is already registered");
    g_host_ranges.push_back({a, b, owned});
    return IVFADC_OK;
}

// removes the range that STARTS at p; found = 0 when there is none of the wanted kind
static bool host_range_take(void *p, bool owned)
{
    std::lock_guard<std::mutex> lk(g_host_mu);
    for (size_t i = 0; i < g_host_ranges.size(); ++i)
        if (g_host_ranges[i].lo == (uintptr_t)p && g_host_ranges[i].owned == owned) {
            g_host_ranges.erase(g_host_ranges.begin() + (ptrdiff_t)i);
            return true;
        }
    return false;
}

int ivfadc_host_alloc(size_t bytes, void **out)
try {
    if (!out) return fail(IVFADC_ERR_INVALID, "out is null");
    *out = nullptr;
    if (bytes == 0) return fail(IVFADC_ERR_INVALID, "bytes == 0");
    void *p = nullptr;
    const hipError_t e = hipHostMalloc(&p, bytes, hipHostMallocPortable | hipHostMallocMapped);
    if (e != hipSuccess) return fail(IVFADC_ERR_HIP, "hipHostMalloc(%zu) failed: %s", bytes, hipGetErrorString(e));
    const int rc = host_range_add(p, bytes, true);
    if (rc != IVFADC_OK) { (void)hipHostFree(p); return rc; }
    *out = p;
    return IVFADC_OK;
} IVF_CATCH

int ivfadc_host_free(void *p)
try {
    if (!p) return IVFADC_OK;
    if (!host_range_take(p, true)) return fail(IVFADC_ERR_INVALID, "not a pointer ivfadc_host_alloc returned");
    HIP_TRY(hipHostFree(p));
    return IVFADC_OK;
} IVF_CATCH

int ivfadc_host_register(void *p, size_t bytes)
try {
    if (!p || bytes == 0) return fail(IVFADC_ERR_INVALID, "null pointer or bytes == 0");
    {
        const uintptr_t a = (uintptr_t)p, b = a + bytes;
        std::lock_guard<std::mutex> lk(g_host_mu);
        for (const HostRange &r : g_host_ranges)
            if (a < r.hi && b > r.lo) return fail(IVFADC_ERR_INVALID, "host range overlaps one that is already registered");
    }
    const hipError_t e = hipHostRegister(p, bytes, hipHostRegisterPortable | hipHostRegisterMapped);
    if (e != hipSuccess) return fail(IVFADC_ERR_HIP, "hipHostRegister(%zu) failed: %s", bytes, hipGetErrorString(e));
    // the kernels use the HOST address: it must be the address the device sees too (it is, wherever the runtime maps host memory at
    // its own virtual address; checked rather than assumed)
    void *dp = nullptr;
    const hipError_t e2 = hipHostGetDevicePointer(&dp, p, 0);
    if (e2 != hipSuccess || dp != p) {
        (void)hipHostUnregister(p);
        (void)hipGetLastError();
        return fail(IVFADC_ERR_HIP, "registered host memory is not addressable by the device at its host address");
    }
    const int rc = host_range_add(p, bytes, false);
    if (rc != IVFADC_OK) { (void)hipHostUnregister(p); return rc; }
    return IVFADC_OK;
} IVF_CATCH

int ivfadc_host_unregister(void *p)
try {
    if (!p) return IVFADC_OK;
    if (!host_range_take(p, false)) return fail(IVFADC_ERR_INVALID, "not a pointer ivfadc_host_register took");
    HIP_TRY(hipHostUnregister(p));
    return IVFADC_OK;
} IVF_CATCH

int ivfadc_get_host_stats(ivfadc_t *h, ivfadc_host_stats *out)
try {
    HandleLock lk_(h);
    if (!h || !out) return fail(IVFADC_ERR_INVALID, "null argument");
    *out = h->hstats;
    return IVFADC_OK;
} IVF_CATCH

int ivfadc_reset_host_stats(ivfadc_t *h)
try {
    HandleLock lk_(h);
    if (!h) return fail(IVFADC_ERR_INVALID, "null handle");
    const int64_t keep = h->hstats.streams_replaced;   // (a fact about the handle's streams, not a per-interval counter)
    h->hstats = ivfadc_host_stats{};
    h->hstats.streams_replaced = keep;
    return IVFADC_OK;
} IVF_CATCH

int ivfadc_set_profiling(ivfadc_t *h, int on)
try {
    HandleLock lk_(h);
    if (!h) return fail(IVFADC_ERR_INVALID, "null handle");
    h->profiling = on != 0;
    h->profiling_level = on;
    return IVFADC_OK;
} IVF_CATCH

int ivfadc_reset_stats(ivfadc_t *h)
try {
    HandleLock lk_(h);
    if (!h) return fail(IVFADC_ERR_INVALID, "null handle");
    TRY(set_device(h));
    TRY(ev_fold(h));
    HIP_TRY(hipStreamSynchronize(h->stream));
    int64_t sp = 0, pp = 0, sv = 0, vis = 0;
    if (h->misc.p) {
        int64_t shards[512];
        HIP_TRY(hipMemcpy(shards, h->misc.p, sizeof(shards), hipMemcpyDeviceToHost));
        for (int i = 0; i < 64; ++i) sp += shards[i * 8];
        for (int i = 0; i < 64; ++i) pp += shards[i * 8 + 1];
        for (int i = 0; i < 64; ++i) sv += shards[i * 8 + 2];
        for (int i = 0; i < 64; ++i) vis += shards[i * 8 + 3];
        HIP_TRY(hipMemcpy(&h->fallback_base, (char *)h->misc.p + 4096 + 64, 8, hipMemcpyDeviceToHost));
    }
    h->scanned_base = sp;
    h->pruned_base = pp;
    h->surv_base = sv;
    h->visited_base = vis;
    const int qg = h->stats.last_qg, ch = h->stats.last_chunk, gr = h->stats.last_scan_grid, lds = h->stats.last_scan_lds;
    const int cm = h->stats.coarse_mfma, ls = h->stats.last_striped, cl = h->stats.coarse_listed, llb = h->stats.last_lb, lnf = h->stats.last_nf;
    const int ltl = h->stats.last_twolevel, lf16 = h->stats.coarse_f16;
    h->stats = ivfadc_stats{};
    h->stats.last_twolevel = ltl;
    h->stats.coarse_f16 = lf16;
    h->stats.last_lb = llb;
    h->stats.last_nf = lnf;
    h->stats.coarse_mfma = cm;
    h->stats.last_striped = ls;
    h->stats.coarse_listed = cl;
    h->stats.last_qg = qg; h->stats.last_chunk = ch; h->stats.last_scan_grid = gr; h->stats.last_scan_lds = lds;
    h->carry_queries = h->carry_scanned = h->carry_pruned = h->carry_surv = h->carry_fallbacks = h->carry_launches = 0;
    if (h->pipe_view) TRY(ivfadc_reset_stats(h->pipe_view));
    return IVFADC_OK;
} IVF_CATCH

int ivfadc_get_stats(ivfadc_t *h, ivfadc_stats *out)
try {
    HandleLock lk_(h);
    if (!h || !out) return fail(IVFADC_ERR_INVALID, "null argument");
    TRY(set_device(h));
    TRY(ev_fold(h));
    HIP_TRY(hipStreamSynchronize(h->stream));
    int64_t sp = 0, pp = 0, sv = 0, vis = 0;
    if (h->misc.p) {
        int64_t shards[512];
        HIP_TRY(hipMemcpy(shards, h->misc.p, sizeof(shards), hipMemcpyDeviceToHost));
        for (int i = 0; i < 64; ++i) sp += shards[i * 8];
        for (int i = 0; i < 64; ++i) pp += shards[i * 8 + 1];
        for (int i = 0; i < 64; ++i) sv += shards[i * 8 + 2];
        for (int i = 0; i < 64; ++i) vis += shards[i * 8 + 3];
        int64_t fb = 0;
        HIP_TRY(hipMemcpy(&fb, (char *)h->misc.p + 4096 + 64, 8, hipMemcpyDeviceToHost));
        h->stats.coarse_fallbacks = fb - h->fallback_base;
    }
    h->stats.scanned_points = sp - h->scanned_base;
    h->stats.pruned_points = pp - h->pruned_base;
    h->stats.lb_survivors = sv - h->surv_base;
    h->stats.coarse_visited = vis - h->visited_base;
    h->stats.twolevel_groups = h->tl_use ? h->tl_G : 0;
    h->stats.twolevel_probe_fraction = h->tl_probe_fraction;
    h->stats.inplace_appends = (int32_t)std::min<int64_t>(h->inplace_appends, 0x7fffffff);
    *out = h->stats;
    // (second lanes of ivfadc_search_batches that a push! or delete made stale and that are gone: their share stays in the totals)
    out->queries += h->carry_queries;
    out->scanned_points += h->carry_scanned;
    out->pruned_points += h->carry_pruned;
    out->lb_survivors += h->carry_surv;
    out->coarse_fallbacks += h->carry_fallbacks;
    out->scan_launches += h->carry_launches;
    if (h->pipe_view) {
        // the odd batches of ivfadc_search_batches ran on the internal view: its counters belong to this handle's totals
        ivfadc_stats v;
        TRY(ivfadc_get_stats(h->pipe_view, &v));
        out->queries += v.queries;
        out->scanned_points += v.scanned_points;
        out->pruned_points += v.pruned_points;
        out->lb_survivors += v.lb_survivors;
        out->coarse_fallbacks += v.coarse_fallbacks;
        out->scan_launches += v.scan_launches;
        out->coarse_visited += v.coarse_visited;
    }
    return IVFADC_OK;
} IVF_CATCH

int ivfadc_train(int device, int d, int64_t n, const float *data, int kc, int k, int m, int coarse_maxiter, int quant_maxiter,
                 uint64_t seed, float *out_centroids, float *out_codebooks)
try {
    return train_impl(device, d, n, data, kc, k, m, coarse_maxiter, quant_maxiter, seed, out_centroids, out_codebooks);
} IVF_CATCH

int ivfadc_set_coarse_mode(ivfadc_t *h, int mode)
try {
    HandleLock lk_(h);
    if (!h) return fail(IVFADC_ERR_INVALID, "null handle");
    if (mode < 0 || mode > 8) return fail(IVFADC_ERR_INVALID, "mode must be 0 ... 8");
    h->allow_f16 = mode != 8 && mode != 3;   // 8: as 0 with the three-product bf16 split (A/B, tests)
    // 6: the certified two-level search whatever the self-probe says (built on the next search); 7: never; anything else: automatic
    h->tl_mode = mode == 6 ? 1 : (mode == 7 ? -1 : 0);
    if (h->tl_tried) h->tl_use = h->tl_G > 0 && (h->tl_mode > 0 || (h->tl_mode == 0 && h->tl_probe_fraction >= 0.f && h->tl_probe_fraction <= 0.02f));
    if (h->tl_mode > 0 && h->tl_G == 0) h->tl_tried = false;   // (automatic mode did not build it for a small quantizer: build on request)
    h->sq_inside = mode == 5;
    h->allow_mfma = (mode != 1) && getenv("IVFADC_COARSE_EXACT") == nullptr;
    h->mfma_min_kc = (mode == 2) ? 128 : 2048;
    h->allow_bf16 = mode != 3 && h->cent_hi.p != nullptr;
    h->allow_listed = mode != 4;
    return IVFADC_OK;
} IVF_CATCH

int ivfadc_set_pruning(ivfadc_t *h, int on)
try {
    HandleLock lk_(h);
    if (!h) return fail(IVFADC_ERR_INVALID, "null handle");
    h->allow_prune = on != 0 && getenv("IVFADC_NO_PRUNE") == nullptr;
    return IVFADC_OK;
} IVF_CATCH

int ivfadc_set_next_queries(ivfadc_t *h, int64_t nq, const float *d_queries, uint64_t token)
try {
    HandleLock lk_(h);
    if (!h) return fail(IVFADC_ERR_INVALID, "null handle");
    if (nq < 0) return fail(IVFADC_ERR_INVALID, "nq < 0");
    h->hint_q = (nq > 0 && token != 0) ? d_queries : nullptr;
    h->hint_nq = h->hint_q ? nq : 0;
    h->hint_token = h->hint_q ? token : 0;
    return IVFADC_OK;
} IVF_CATCH

int ivfadc_set_query_token(ivfadc_t *h, uint64_t token)
try {
    HandleLock lk_(h);
    if (!h) return fail(IVFADC_ERR_INVALID, "null handle");
    h->cur_token = token;
    return IVFADC_OK;
} IVF_CATCH

int ivfadc_set_table_mode(ivfadc_t *h, int mode)
try {
    HandleLock lk_(h);
    if (!h) return fail(IVFADC_ERR_INVALID, "null handle");
    if (mode < 0 || mode > 10) return fail(IVFADC_ERR_INVALID, "mode must be 0 ... 10");
    h->allow_filt = mode != 1 && getenv("IVFADC_EXACT_TABLES") == nullptr;
    h->force_lb = mode == 2 || mode == 4;
    // 3 / 4: as 0 / 2 with the matrix-core tables built from the three-product bf16 split instead of one f16 product (A/B runs, tests)
    h->lb_use_f16 = mode != 3 && mode != 4;
    // 5 / 6: as 0 with the eight-wave list-major kernel (wg8scan.hip.h) never / wherever it is instantiated (A/B runs, tests);
    // 7: as 6 with its eight-query form (wg8_scan_kernel<8>) wherever that is instantiated
    // 8 / 9: as 6 / 7, and for 64 < K <= 128 the kernel's wide-pool form (wg8_wide_scan_kernel: two pool entries per lane) instead of the
    // four-wave kernel with LDS selectors; K <= 64 and K > 128 run exactly what 6 / 7 run
    h->wg8_mode = mode == 5 ? -1 : (mode == 6 || mode == 8 ? 1 : (mode == 7 || mode == 9 ? 2 : 0));
    h->wg8_wide = mode == 8 || mode == 9;
    // 10: as 0, and on a 16-bit handle 64 < K runs the scan kernel's LDS-selector form (u16_wide_scan_kernel) wherever its LDS need fits a
    // CU (K <= 1984 at small m x dsub: u16scan.hip.h) instead of the generic path; an 8-bit handle plans what mode 0 plans
    h->u16_wide = mode == 10;
    return IVFADC_OK;
} IVF_CATCH

int ivfadc_set_u16_tables(ivfadc_t *h, int mode)
try {
    HandleLock lk_(h);
    if (!h) return fail(IVFADC_ERR_INVALID, "null handle");
    if (mode < 0 || mode > 2) return fail(IVFADC_ERR_INVALID, "mode must be 0 ... 2");
    h->u16_tables = mode;   // (an 8-bit handle keeps it and never reads it: make_plan_u16 alone does)
    return IVFADC_OK;
} IVF_CATCH

int ivfadc_debug_lb_table(ivfadc_t *h, const float *query, int cell, uint8_t *out_table, float *out_consts)
try {
    HandleLock lk_(h);
    if (!h || !query || !out_table || !out_consts) return fail(IVFADC_ERR_INVALID, "null argument");
    if (cell < 0 || cell >= h->kc) return fail(IVFADC_ERR_INVALID, "cell out of range");
    if (h->u16) return fail(IVFADC_ERR_STATE, "ivfadc_debug_lb_table: this index has UInt16 codes (no 8-bit lower-bound tables)");
    if (!h->lb_split.p || !lb_shape(h->m, h->dsub)) return fail(IVFADC_ERR_STATE, "no matrix-core table kernels for m=%d dsub=%d", h->m, h->dsub);
    TRY(set_device(h));
    const int m = h->m;
    DevBuf dq, dt, df;
    int rc = dq.ensure((size_t)h->d * 4);
    if (rc == IVFADC_OK) rc = dt.ensure((size_t)m * 256);
    if (rc == IVFADC_OK) rc = df.ensure((size_t)(3 + 2 * m) * 4);
    if (rc == IVFADC_OK) {
        hipError_t e = hipMemcpyAsync(dq.p, query, (size_t)h->d * 4, hipMemcpyHostToDevice, h->stream);
        if (e == hipSuccess) {
            const size_t lds = lb_lds_bytes(m, h->dsub, 1);
            void (*dk)(const IndexView, const LbView, const float *, int, unsigned char *, float *) =
                (m == 48) ? lb_debug_kernel<48, 16> : lb_debug_kernel<16, 6>;
            rc = fn_raise_lds(h->device, (const void *)dk, lds, false);
            if (rc == IVFADC_OK) {
                hipLaunchKernelGGL(dk, dim3(1), dim3(256), lds, h->stream, index_view(h), lb_view(h), dq.as<float>(), cell, dt.as<unsigned char>(),
                                   df.as<float>());
                e = hipGetLastError();
            }
        }
        if (e == hipSuccess) e = hipMemcpyAsync(out_table, dt.p, (size_t)m * 256, hipMemcpyDeviceToHost, h->stream);
        if (e == hipSuccess) e = hipMemcpyAsync(out_consts, df.p, (size_t)(3 + 2 * m) * 4, hipMemcpyDeviceToHost, h->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
        if (e != hipSuccess && rc == IVFADC_OK) rc = fail(IVFADC_ERR_HIP, "debug table: %s", hipGetErrorString(e));
    }
    dq.release(); dt.release(); df.release();
    return rc;
} IVF_CATCH

int ivfadc_set_workspace_limit(ivfadc_t *h, uint64_t bytes)
try {
    HandleLock lk_(h);
    if (!h) return fail(IVFADC_ERR_INVALID, "null handle");
    h->ws_budget = (size_t)std::max<uint64_t>(bytes, 1 << 20);
    return IVFADC_OK;
} IVF_CATCH

int ivfadc_set_tuning(ivfadc_t *h, int qg, int chunk_points)
try {
    HandleLock lk_(h);
    if (!h) return fail(IVFADC_ERR_INVALID, "null handle");
    if (!(qg == 0 || qg == -1 || qg == -2 || qg == -3 || qg == 1 || qg == 2 || qg == 4 || qg == 8))
        return fail(IVFADC_ERR_INVALID, "qg must be 0, -1, -2, -3, 1, 2, 4 or 8");
    if (chunk_points < 0) return fail(IVFADC_ERR_INVALID, "chunk_points < 0");
    h->force_qg = qg;
    h->force_chunk = chunk_points;
    return IVFADC_OK;
} IVF_CATCH

}  // extern "C"

// ---- persistence: the reference's own on-disk format (src/persistency.jl:1-78 writer, :82-134 loader) ---------
// 9 text lines ("<nrows> <nclusters>" / "<n> <m> <k> <dsub>" / coarse quantizer / quantization / U / I / Dc / Dr / T),
// then raw little-endian binary: centroids column by column (:44-49); per codebook its `codes` (labels) and then
// `vectors` row j across all k codewords (:56-61); the nrows x nrows rotation matrix (:62-64, never read by
// knn_search); per list clsize::Int64, idxs, then every vector's m code bytes (:68-78).
namespace {

struct FileCloser {
    FILE *f;
    ~FileCloser() { if (f) fclose(f); }
};

bool read_exact(FILE *f, void *dst, size_t bytes) { return bytes == 0 || fread(dst, 1, bytes, f) == bytes; }

bool read_line(FILE *f, std::string &out)
{
    out.clear();
    int c;
    while ((c = fgetc(f)) != EOF && c != '\n') out.push_back((char)c);
    while (!out.empty() && (out.back() == '\r' || out.back() == ' ')) out.pop_back();
    return c != EOF || !out.empty();
}

std::string last_component(const std::string &s)
{
    const size_t p = s.rfind('.');
    return p == std::string::npos ? s : s.substr(p + 1);
}

}  // namespace

int ivfadc_save_index(ivfadc_t *h, const char *path, int index_bits)
try {
    HandleLock lk_(h);
    if (!h || !path) return fail(IVFADC_ERR_INVALID, "null argument");
    if (h->is_view) return fail(IVFADC_ERR_STATE, "a view keeps no host mirror of the lists");
    if (h->synthetic) return fail(IVFADC_ERR_STATE, "device-synthesised lists keep no host mirror");
    if (index_bits != 8 && index_bits != 16 && index_bits != 32) return fail(IVFADC_ERR_INVALID, "index_bits must be 8, 16 or 32");
    TRY(set_device(h));
    if (index_bits < 32) {   // the reference asserts the capacity of I (index.jl:124-125, utils.jl:134-135): never truncate an id
        uint32_t v = 0;
        if (h->mirror.first_id_above(index_bits == 8 ? 0xFFu : 0xFFFFu, v)) return fail(IVFADC_ERR_ASSERT, "id %u does not fit a %d-bit index type", v, index_bits);
    }
    const int d = h->d, kc = h->kc, m = h->m, k = h->ksub, dsub = h->dsub;
    std::vector<float> cent((size_t)kc * d), cbs((size_t)d * k);
    const int ub = h->u16 ? 2 : 1;   // bytes of U
    std::vector<uint8_t> lab((size_t)m * k * ub);
    HIP_TRY(hipStreamSynchronize(h->stream));
    TRY(d2h_copy(cent.data(), h->centroids.p, cent.size() * 4, h->stream));
    TRY(d2h_copy(cbs.data(), h->codebooks.p, cbs.size() * 4, h->stream));
    if (h->u16) memcpy(lab.data(), h->labmap.lab16.data(), lab.size());
    else HIP_TRY(hipMemcpy(lab.data(), h->labels.p, lab.size(), hipMemcpyDeviceToHost));
    // the lists one behind the other, codes as labels: what ivfadc_get_lists hands out
    const int cb = h->cb;
    const int64_t ntot = h->mirror.ntotal();
    std::vector<int64_t> off((size_t)kc + 1);
    std::vector<uint8_t> codes((size_t)ntot * cb), narrow;
    std::vector<uint32_t> all_ids((size_t)ntot);
    h->mirror.gather(off.data(), codes.data(), all_ids.data(), cb);
    if (h->u16) h->labmap.to_labels(ntot, codes.data());
    FileCloser fc{fopen(path, "wb")};
    FILE *f = fc.f;
    if (!f) return fail(IVFADC_ERR_INVALID, "cannot open %s for writing", path);
    const char *iname = index_bits == 8 ? "UInt8" : (index_bits == 16 ? "UInt16" : "UInt32");
    fprintf(f, "%d %d\n%lld %d %d %d\nNaiveQuantizer\nQuantizedArrays.OrthogonalQuantization\n%s\n%s\n"
               "Distances.SqEuclidean\nDistances.SqEuclidean\nFloat32\n", d, kc, (long long)ntot, m, k, dsub, h->u16 ? "UInt16" : "UInt8",
            iname);
    bool ok = fwrite(cent.data(), 4, cent.size(), f) == cent.size();                  // centroid c = column c
    std::vector<float> row((size_t)k);
    for (int i = 0; i < m && ok; ++i) {
        ok = fwrite(lab.data() + (size_t)i * k * ub, 1, (size_t)k * ub, f) == (size_t)k * ub;
        for (int j = 0; j < dsub && ok; ++j) {                                        // vectors[j, :]
            for (int c = 0; c < k; ++c) row[c] = cbs[((size_t)i * k + c) * dsub + j];
            ok = fwrite(row.data(), 4, (size_t)k, f) == (size_t)k;
        }
    }
    if (!h->rot.empty()) {                                                            // the rotation the index was loaded with (:opq)
        ok = ok && fwrite(h->rot.data(), 4, h->rot.size(), f) == h->rot.size();
    } else {
        std::vector<float> rot((size_t)d, 0.0f);
        for (int i = 0; i < d && ok; ++i) {                                           // identity rotation, column i
            rot[i] = 1.0f;
            ok = fwrite(rot.data(), 4, (size_t)d, f) == (size_t)d;
            rot[i] = 0.0f;
        }
    }
    for (int l = 0; l < kc && ok; ++l) {
        const int64_t len = off[l + 1] - off[l];
        ok = fwrite(&len, 8, 1, f) == 1;
        const uint32_t *ids = all_ids.data() + off[l];
        if (index_bits == 32) {
            ok = ok && (len == 0 || fwrite(ids, 4, (size_t)len, f) == (size_t)len);
        } else {
            const int bw = index_bits / 8;
            narrow.resize((size_t)len * bw);
            for (int64_t p = 0; p < len; ++p) {
                if (bw == 1) narrow[p] = (uint8_t)ids[p];
                else { const uint16_t v = (uint16_t)ids[p]; memcpy(&narrow[(size_t)p * 2], &v, 2); }
            }
            ok = ok && (len == 0 || fwrite(narrow.data(), 1, narrow.size(), f) == narrow.size());
        }
        ok = ok && (len == 0 || fwrite(codes.data() + (size_t)off[l] * cb, 1, (size_t)len * cb, f) == (size_t)len * cb);
    }
    if (!ok) return fail(IVFADC_ERR_INVALID, "short write to %s", path);
    return IVFADC_OK;
} IVF_CATCH

int ivfadc_load_index(ivfadc_t **out, int device, const char *path, int *out_index_bits)
try {
    if (!out || !path) return fail(IVFADC_ERR_INVALID, "null argument");
    *out = nullptr;
    FileCloser fc{fopen(path, "rb")};
    FILE *f = fc.f;
    if (!f) return fail(IVFADC_ERR_INVALID, "cannot open %s", path);
    struct stat sb;
    if (fstat(fileno(f), &sb) != 0 || sb.st_size < 0) return fail(IVFADC_ERR_INVALID, "%s: cannot stat", path);
    const unsigned long long fsize = (unsigned long long)sb.st_size;
    std::string ln[9];
    for (int i = 0; i < 9; ++i)
        if (!read_line(f, ln[i])) return fail(IVFADC_ERR_INVALID, "%s: truncated header", path);
    long long nrows = 0, nclusters = 0, n = 0, m = 0, k = 0, dsub = 0;
    if (sscanf(ln[0].c_str(), "%lld %lld", &nrows, &nclusters) != 2 || sscanf(ln[1].c_str(), "%lld %lld %lld %lld", &n, &m, &k, &dsub) != 4)
        return fail(IVFADC_ERR_INVALID, "%s: bad header", path);
    // What the HIP path can search with the reference's semantics, and nothing else: a file of another quantizer,
    // quantization or distance would load and then be searched with the wrong arithmetic.  Type names come as `X` or
    // `Module.X` (persistency.jl:14-19 writes string(T); :137-144 reads both spellings).
    if (last_component(ln[2]) != "NaiveQuantizer")
        return fail(IVFADC_ERR_INVALID, "only NaiveQuantizer files are supported, got %s", ln[2].c_str());
    if (last_component(ln[3]) != "OrthogonalQuantization")
        return fail(IVFADC_ERR_INVALID, "quantization %s is not supported (only OrthogonalQuantization, i.e. :pq)", ln[3].c_str());
    int ub = 0;   // bytes of U
    if (ln[4] == "UInt8") ub = 1; else if (ln[4] == "UInt16") ub = 2;
    else return fail(IVFADC_ERR_INVALID, "quantization element type %s (only UInt8 and UInt16)", ln[4].c_str());
    int ibytes = 0;
    if (ln[5] == "UInt8") ibytes = 1; else if (ln[5] == "UInt16") ibytes = 2; else if (ln[5] == "UInt32") ibytes = 4;
    else return fail(IVFADC_ERR_INVALID, "index type %s is not supported by the HIP path", ln[5].c_str());
    if (last_component(ln[6]) != "SqEuclidean")
        return fail(IVFADC_ERR_INVALID, "coarse distance %s is not supported (only SqEuclidean)", ln[6].c_str());
    if (last_component(ln[7]) != "SqEuclidean")
        return fail(IVFADC_ERR_INVALID, "residual distance %s is not supported (only SqEuclidean)", ln[7].c_str());
    int tbytes = 0;
    if (ln[8] == "Float32") tbytes = 4; else if (ln[8] == "Float64") tbytes = 8;
    else return fail(IVFADC_ERR_INVALID, "element type %s", ln[8].c_str());
    if (nrows < 1 || nclusters < 1 || m < 1 || k < 1 || k > (ub == 1 ? 256 : 65536) || dsub < 1 || n < 0)
        return fail(IVFADC_ERR_INVALID, "%s: inconsistent sizes", path);
    // every size is checked against what the file can hold BEFORE anything is allocated from it (a corrupt or hostile
    // header must come back as IVFADC_ERR_INVALID, not as std::bad_alloc); 128-bit products cannot wrap
    typedef unsigned __int128 u128;
    const long pos0 = ftell(f);
    if (pos0 < 0) return fail(IVFADC_ERR_INVALID, "%s: ftell failed", path);
    const u128 remain = (u128)(fsize - std::min<unsigned long long>(fsize, (unsigned long long)pos0));
    if (nrows > (1ll << 24) || nclusters > (1ll << 31) - 1 || m > nrows || dsub > nrows || (u128)m * (u128)dsub != (u128)nrows)
        return fail(IVFADC_ERR_INVALID, "%s: inconsistent sizes", path);
    if (n > (long long)0xFFFFFFFFll) return fail(IVFADC_ERR_INVALID, "%s: %lld vectors exceed UInt32 ids", path, n);
    const u128 quant_bytes = (u128)tbytes * (u128)nrows * (u128)nclusters + (u128)m * ((u128)k * ub + (u128)tbytes * (u128)dsub * (u128)k) +
                             (u128)tbytes * (u128)nrows * (u128)nrows;
    const u128 list_bytes = (u128)nclusters * 8 + (u128)n * (u128)(ibytes + m * ub);
    if (quant_bytes + list_bytes > remain)
        return fail(IVFADC_ERR_INVALID, "%s: header describes more data than the file holds (truncated or corrupt)", path);
    auto read_floats = [&](float *dst, size_t cnt) {
        if (tbytes == 4) return read_exact(f, dst, cnt * 4);
        std::vector<double> tmp(cnt);
        if (!read_exact(f, tmp.data(), cnt * 8)) return false;
        for (size_t i = 0; i < cnt; ++i) dst[i] = (float)tmp[i];
        return true;
    };
    std::vector<float> cent((size_t)nclusters * nrows), cbs((size_t)nrows * k), row((size_t)std::max(k, nrows));
    std::vector<uint8_t> lab((size_t)m * k * ub);
    if (!read_floats(cent.data(), cent.size())) return fail(IVFADC_ERR_INVALID, "%s: truncated centroids", path);
    for (long long i = 0; i < m; ++i) {
        if (!read_exact(f, lab.data() + (size_t)i * k * ub, (size_t)k * ub)) return fail(IVFADC_ERR_INVALID, "%s: truncated codebook", path);
        for (long long j = 0; j < dsub; ++j) {
            if (!read_floats(row.data(), (size_t)k)) return fail(IVFADC_ERR_INVALID, "%s: truncated codebook", path);
            for (long long c = 0; c < k; ++c) cbs[((size_t)i * k + c) * dsub + j] = row[c];
        }
    }
    // rotation matrix (persistency.jl:62-64).  knn_search never reads it (index.jl:204-258): an :opq index is searched as it is.
    // quantize_data -- push! -- does read it: the handle keeps the matrix (it is written back by ivfadc_save_index) and refuses to encode.
    std::vector<float> rotm((size_t)nrows * nrows);
    bool rot_identity = true;
    for (long long i = 0; i < nrows; ++i) {
        if (!read_floats(row.data(), (size_t)nrows)) return fail(IVFADC_ERR_INVALID, "%s: truncated rotation", path);
        for (long long j = 0; j < nrows; ++j) {
            if (!std::isfinite(row[j])) return fail(IVFADC_ERR_INVALID, "%s: non-finite rotation entry", path);
            rotm[(size_t)i * nrows + j] = row[j];
            rot_identity = rot_identity && row[j] == (i == j ? 1.0f : 0.0f);
        }
    }
    std::vector<int64_t> offsets((size_t)nclusters + 1, 0);
    std::vector<uint8_t> codes, raw;
    std::vector<uint32_t> ids;
    codes.reserve((size_t)n * m * ub);
    ids.reserve((size_t)n);
    for (long long l = 0; l < nclusters; ++l) {
        int64_t len = 0;
        if (!read_exact(f, &len, 8) || len < 0) return fail(IVFADC_ERR_INVALID, "%s: truncated list %lld", path, l);
        if (len > n - offsets[l]) return fail(IVFADC_ERR_INVALID, "%s: list %lld holds %lld entries, more than the header's n leaves", path, l, (long long)len);
        raw.resize((size_t)len * ibytes);
        if (!read_exact(f, raw.data(), raw.size())) return fail(IVFADC_ERR_INVALID, "%s: truncated list %lld", path, l);
        for (int64_t p = 0; p < len; ++p) {
            uint32_t v = 0;
            memcpy(&v, raw.data() + (size_t)p * ibytes, ibytes);   // little-endian narrow ids
            ids.push_back(v);
        }
        const size_t at = codes.size();
        codes.resize(at + (size_t)len * m * ub);
        if (!read_exact(f, codes.data() + at, (size_t)len * m * ub)) return fail(IVFADC_ERR_INVALID, "%s: truncated list %lld", path, l);
        offsets[l + 1] = offsets[l] + len;
    }
    if (offsets[nclusters] != n) return fail(IVFADC_ERR_INVALID, "%s: the lists hold %lld entries, the header says %lld", path, (long long)offsets[nclusters], n);
    ivfadc_t *h = nullptr;
    std::vector<uint8_t> idx;
    if (ub == 2) {
        // UInt16: labels distinct per block and every code a label of its block, checked here, before any device call
        const uint16_t *lab16 = (const uint16_t *)lab.data();
        const std::string prefix = std::string(path) + ": ";
        list_mirror::LabelMap lm;
        TRY(mirror_fail(lm.init16(lab16, (int)m, (int)k), true, prefix.c_str()));
        TRY(mirror_fail(lm.to_indices(n, (const uint16_t *)codes.data(), idx), true, prefix.c_str()));
        TRY(create_impl(&h, device, (int)nrows, (int)nclusters, (int)m, (int)k, cent.data(), cbs.data(), nullptr, lab16));
    } else {
        TRY(ivfadc_create(&h, device, (int)nrows, (int)nclusters, (int)m, (int)k, cent.data(), cbs.data(), lab.data()));
    }
    // (the offsets were built above and the 16-bit codes are in mirror form already; 8-bit codes are checked against the handle's labels)
    const int rc = ub == 2 ? assign_lists(h, offsets.data(), idx.data(), ids.data(), "ivfadc_set_lists_u16")
                           : set_lists_entry(h, offsets.data(), codes.data(), ids.data(), false);
    if (rc != IVFADC_OK) { ivfadc_destroy(h); return rc; }
    if (!rot_identity) h->rot = std::move(rotm);
    if (out_index_bits) *out_index_bits = ibytes * 8;
    *out = h;
    return IVFADC_OK;
} IVF_CATCH

int ivfadc_get_rotation(ivfadc_t *h, int *out_rotated, float *out_rot)
try {
    HandleLock lk_(h);
    if (!h) return fail(IVFADC_ERR_INVALID, "null handle");
    if (out_rotated) *out_rotated = h->rot.empty() ? 0 : 1;
    if (out_rot) {
        if (!h->rot.empty()) memcpy(out_rot, h->rot.data(), h->rot.size() * 4);
        else
            for (int i = 0; i < h->d; ++i)
                for (int j = 0; j < h->d; ++j) out_rot[(size_t)i * h->d + j] = i == j ? 1.0f : 0.0f;
    }
    return IVFADC_OK;
} IVF_CATCH
