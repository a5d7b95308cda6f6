/*
 * ivfadc_hip.h -- C ABI of libivfadc_hip.so: the MI355X (gfx950) implementation of
 * IVFADC.jl's knn_search hot path.
 *
 * The reference (pure Julia, /root/reference) has no FFI; its boundary for this path
 * is Julia multiple dispatch.  Each entry point below names the reference interface it
 * replaces.  A Julia shim or the Python mirror (ivfadc.jl_amd/) binds
 * exactly these symbols via ccall / ctypes.
 *
 * Conventions
 *   - every function returns 0 (IVFADC_OK) or a non-zero ivfadc_status; no C++
 *     exception crosses the boundary; ivfadc_last_error() gives the message of the
 *     last failure on the calling thread.
 *   - the caller owns every host buffer; the library owns device memory.
 *   - matrices are Julia-native column-major: "d x n" means n contiguous vectors of d.
 *   - T = Float32, U in {UInt8 (ksub <= 256), UInt16 (ksub <= 65536)}, I = UInt32, distance = SqEuclidean for both
 *     the coarse and the residual quantizer (defaults.jl:6,8), NaiveQuantizer only.
 *   - one HIP stream per handle.  Threads: every entry point locks its handle, so calls on ONE handle from several
 *     threads are serialised (correct, not concurrent); calls on DIFFERENT handles -- an index and its views
 *     (ivfadc_clone_view), unrelated indexes -- run concurrently.  A mutator (push! / delete / set_lists ...) first
 *     waits for the calls running on the index's views and keeps new ones out until it is done; the first view search
 *     afterwards refuses (the index changed).  Destroying a handle while another thread is inside a call on it is
 *     the caller's error.  (The reference is single-threaded, index.jl:269; tests: test_threads_index_view_and_a_mutator.)
 *   - IVFADC_ERR_ASSERT marks the conditions the reference raises AssertionError for.
 *
 * Environment.  The library reads these variables and no others (csrc/ivfadc_hip.hip: getenv); each is a switch a deployment may
 * need without a rebuild, none changes a result:
 *   IVFADC_EXACT_TABLES=1     reference-order f32 tables in every lane (= ivfadc_set_table_mode(h, 1) on every handle): validation
 *   IVFADC_COARSE_EXACT=1     exact coarse kernels only, no matrix-core filters (= ivfadc_set_coarse_mode(h, 1)): validation
 *   IVFADC_NO_PRUNE=1         scan every probed list (= ivfadc_set_pruning(h, 0)): the reference's own byte count
 *   IVFADC_NO_SMALLQ=1        no single-launch latency path for small batches
 *   IVFADC_NO_PIPELINE=1      ivfadc_search_batches keeps one batch in flight
 *   IVFADC_NO_ZERO_COPY=1     host-pointer entries stage through the library's pinned blocks even for known memory
 *   IVFADC_NO_STREAM_PROBE=1  no probing for streams that share a hardware queue (views, the batches entry)
 *   IVFADC_ABORT_TRACE=path   append a native backtrace to `path` when the process aborts inside the library (test infrastructure)
 */
#ifndef IVFADC_HIP_H
#define IVFADC_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct ivfadc_index ivfadc_t;

typedef enum {
    IVFADC_OK = 0,
    IVFADC_ERR_ASSERT = 1,      /* reference @assert would fail (k<1, w<1, wrong dim, capacity) */
    IVFADC_ERR_INVALID = 2,     /* argument the reference cannot express / library limit      */
    IVFADC_ERR_HIP = 3,         /* HIP runtime error (no device, out of memory, launch fail)  */
    IVFADC_ERR_STATE = 4        /* call not valid in the handle's state (e.g. no lists yet)   */
} ivfadc_status;

/* Bumped whenever an exported prototype changes in place or a struct grows (the round-4 change of ivfadc_set_next_queries, which gained
 * its token argument, was version 2 -> 3).  A binding built against another version must not call into this library: the Julia shim and
 * tests/c/abi_smoke.c compare ivfadc_abi_version() with the value they were written for before anything else.                           */
#define IVFADC_ABI_VERSION 4
int ivfadc_abi_version(void);

/* Reach of the selection kernels.  Beyond either (any K, any w <= kc) the library takes the generic path: every
 * (query, probed point) key is written out and sorted, the first K are the result -- same semantics, slower. */
#define IVFADC_MAX_K 2048
#define IVFADC_MAX_W 2048

/* Replaces: the data of IVFADCIndex.coarse_quantizer (NaiveQuantizer.vectors,
 * coarsequantizers.jl:18-20) and .residual_quantizer.codebooks (index.jl:39-48).
 *   centroids   d x kc column-major (centroid c at centroids + c*d)
 *   codebooks   m blocks; block i is codebooks[i].vectors, dsub x ksub column-major
 *   code_labels m x ksub: codebooks[i].codes (the byte that names codeword c of block i);
 *               labels of one block must be distinct (LittleDict keys, index.jl:235)
 * Requires d % m == 0 (QuantizedArrays.rowrange for other shapes is third-party and
 * unverifiable), 1 <= ksub <= 256 (ivfadc_create_u16 below: up to 65536), kc >= 1.     */
int ivfadc_create(ivfadc_t **out, int device, int d, int kc, int m, int ksub,
                  const float *centroids, const float *codebooks, const uint8_t *code_labels);

/* Code width.  A handle is created for U = UInt8 (ivfadc_create, ivfadc_load_index of a UInt8 file) or U = UInt16 (ivfadc_create_u16,
 * ivfadc_load_index of a UInt16 file: IVFADCIndex{UInt16,...}, persistency.jl:57,102-128).  On a 16-bit handle the entries that move
 * codes or labels are the _u16 ones below; their uint8_t counterparts (ivfadc_set_lists, _get_lists, _encode, _append, _get_quantizers,
 * _synth_lists, ivfadc_debug_lb_table) return IVFADC_ERR_STATE there, and the _u16 entries return IVFADC_ERR_STATE on an 8-bit handle.
 * Every other entry (the searches, views, delete / shift, dims, save / load, stats, tuning, pruning, coarse modes) serves both widths.
 * Code and label buffers of the _u16 entries are declared void * and hold uint16_t (little-endian, as the file stores them).
 * ivfadc_set_list_partition with nparts > 1 returns IVFADC_ERR_INVALID on a 16-bit handle.
 * Searches on a 16-bit handle run the list scan of u16scan.hip.h for K <= 64 and the generic path (any K and w) above; with
 * ivfadc_set_table_mode(h, 10) the scan kernel also serves 64 < K through LDS selectors wherever
 *     32 (m dsp + qg cap) + 32 912 B <= 160 KB,  dsp = dsub rounded up to 4, cap = max(128, pow2ceil(K + 64)), qg = pairs per work item,
 * holds at qg = 1 (the plan halves qg until it holds: m dsp + qg cap <= 4091).  That is K <= 1984 for m dsp <= 2040, K <= 960 up to 3064,
 * K <= 448 up to 3576, K <= 192 up to 3832; any other K > 64 takes the generic path as in mode 0 (stats.last_qg == -2).
 * ivfadc_set_u16_tables(h, 1 / 2) replaces the per-pass ADC tables by sums straight from the codebook (below); without a 32 KB table
 * area its wide form reaches m dsp + qg cap <= 5115: K <= 1984 for m dsp <= 3064, K <= 960 up to 4088, K <= 448 up to 4600,
 * K <= 192 up to 4856, and K <= IVFADC_MAX_K (cap = 4096) for m dsp <= 1016.                                                 */
/* As ivfadc_create, for U = UInt16: 1 <= ksub <= 65536, code_labels is m x ksub uint16_t (distinct within a block).  Validation runs
 * before any device call.                                                                                                  */
int ivfadc_create_u16(ivfadc_t **out, int device, int d, int kc, int m, int ksub,
                      const float *centroids, const float *codebooks, const void *code_labels);
/* The handle's code width in bits: 8 or 16. */
int ivfadc_code_bits(ivfadc_t *h, int *bits);
/* ivfadc_set_lists / _get_lists / _encode / _append / _get_quantizers with n x m uint16_t codes and m x ksub uint16_t labels. */
int ivfadc_set_lists_u16(ivfadc_t *h, const int64_t *offsets, const void *codes, const uint32_t *ids);
int ivfadc_get_lists_u16(ivfadc_t *h, int64_t *offsets, void *codes, uint32_t *ids);
int ivfadc_encode_u16(ivfadc_t *h, int64_t n, const float *pts, int32_t *out_list, void *out_codes);
int ivfadc_append_u16(ivfadc_t *h, int64_t nnew, const float *pts, const uint32_t *ids, int32_t *out_list, void *out_codes);
int ivfadc_get_quantizers_u16(ivfadc_t *h, float *centroids, float *codebooks, void *code_labels);

/* Replaces (statistically, not bit for bit: both are third-party and unseeded in the reference) the training half
 * of the IVFADCIndex constructor, index.jl:127-147: Clustering.kmeans(data, kc; init=:kmpp, maxiter) for the coarse
 * quantizer and QuantizedArrays.build_quantizer(residuals; k, m, method=:pq, maxiter), i.e. one k-means per sub-space.
 *   data d x n; out_centroids d x kc; out_codebooks m blocks of dsub x k (the layout ivfadc_create takes; labels are
 *   0..k-1).  Runs on the device: k-means++ seeding, exact-distance assignment (the search path's coarse kernel), and
 *   order-independent fixed-point sums, so the result is deterministic for a given seed.
 *   Guarantee: a centre that stops changing is the Float32-rounded mean of its points up to the fixed-point quantum
 *   2^(e-61) of its stage, where n * max|x| < 2^e over that stage's data (|c - mean| <= ulp(c)/2 + quantum); the
 *   quantum follows the data's binary magnitude, so training x * 2^j gives the quantizers of x times 2^j while the
 *   Float32 arithmetic stays normal.
 * Constructor checks of index.jl:118-123 (kc >= 2, k <= n, 1 <= m <= d, maxiter > 0) -> IVFADC_ERR_ASSERT; then 1 <= k <= 65536.
 * Data with a NaN or infinite component -> IVFADC_ERR_INVALID, before any device call (as ivfadc_create refuses such
 * quantizers).                                                                                                         */
int ivfadc_train(int device, int d, int64_t n, const float *data, int kc, int k, int m,
                 int coarse_maxiter, int quant_maxiter, uint64_t seed,
                 float *out_centroids, float *out_codebooks);

/* Replaces: IVFADCIndex.inverse_index (index.jl:8-11,23; built at index.jl:178-194).
 *   offsets kc+1 point offsets (list c = [offsets[c], offsets[c+1]))
 *   codes   n x m bytes, list order, m bytes per point (the order persistency.jl:74-76 writes)
 *   ids     n ids, 0-based as stored by the reference (index.jl:189)
 * Replaces any previous lists.  Every code byte must be a label of its block.           */
int ivfadc_set_lists(ivfadc_t *h, const int64_t *offsets, const uint8_t *codes, const uint32_t *ids);

/* Bench / test utility (no reference counterpart): fills the lists ON THE DEVICE with
 * counter-based pseudo-random code bytes (byte b of global position g is
 * mix64(seed + ((g*m+b)>>3)*0x9E3779B97F4A7C15) >> 8*((g*m+b)&7)), ids = global position.
 * The oracle regenerates any list from the same rule.  Requires ksub == 256 with identity
 * labels.  No host mirror is kept, so ivfadc_append / ivfadc_get_lists return ERR_STATE. */
int ivfadc_synth_lists(ivfadc_t *h, const int64_t *offsets, uint64_t seed);

/* Replaces: _encode_point (utils.jl:148-161): coarse_search(cq, point, 1) -> residual ->
 * quantize_data.  pts is d x n.  out_list: 0-based cluster per point; out_codes: n x m.
 * Does not modify the index.                                                             */
int ivfadc_encode(ivfadc_t *h, int64_t n, const float *pts, int32_t *out_list, uint8_t *out_codes);

/* Replaces: push!(ivfadc, point) (utils.jl:114, _push! :127-145) for a batch: encodes and
 * appends (ids[i], code_i) to the END of list out_list[i], in order i = 0..nnew-1.  The
 * caller chooses ids (push! uses id = length(ivfadc)); out_list / out_codes (may be NULL)
 * return the assignment so a host mirror stays coherent.  Device side: every list carries
 * spare capacity (max(32, len/8) points); when all target lists have room the codes and
 * ids are scattered in place (O(nnew)), otherwise the next search re-lays the lists out.  */
int ivfadc_append(ivfadc_t *h, int64_t nnew, const float *pts, const uint32_t *ids,
                  int32_t *out_list, uint8_t *out_codes);

/* Replaces: delete_from_index!(ivfadc, points) (utils.jl:90-105), and with a single id pop! / popfirst!
 * (utils.jl:29-68): removes the stored entries whose id is listed (0-based ids; unknown ids are ignored), keeps the
 * order of the survivors in every list, and lowers each surviving id by the number of removed ids below it
 * (_shift_inverse_index!, utils.jl:11-27).  Done in place on the device (one workgroup per list) and on the host
 * mirror.  out_removed (may be NULL): how many entries went.                                                  */
int ivfadc_delete_ids(ivfadc_t *h, int64_t ndel, const uint32_t *ids, int64_t *out_removed);

/* Replaces: _shift_up_inverse_index!(ivfadc, 1) of pushfirst! (utils.jl:1-9, 123): adds delta to every stored id. */
int ivfadc_shift_ids(ivfadc_t *h, int32_t delta);

/* Replaces: knn_search(ivfadc, points::Vector{Vector{T}}, k; w) (index.jl:261-273), i.e.
 * knn_search (index.jl:204-258) for every query.  queries is d x nq.
 *   out_ids / out_dists  K slots per query (query q at + q*K), ascending (distance, visit order)
 *   out_counts           neighbours found for query q (<= K; "at most k", index.jl:200)
 * K < 1 or w < 1 -> IVFADC_ERR_ASSERT (index.jl:210-211); w is clamped to kc (index.jl:216). */
int ivfadc_search(ivfadc_t *h, int64_t nq, const float *queries, int K, int w,
                  uint32_t *out_ids, float *out_dists, int32_t *out_counts);

/* Page-locked host memory for the host-pointer entries (ivfadc_search, ivfadc_search_batches, ivfadc_mg_search).
 * The reference's call takes and returns host arrays (index.jl:261-265: Vector{Vector{T}} in, Vector{Vector{I}} / Vector{Vector{T}} out),
 * so a binding packs the queries into one d x nq matrix and unpacks the results anyway.  When that matrix / those result arrays lie in
 * memory the GPU can address, the library needs no staging copy of its own:
 *   queries     are ingested from the caller's array by the first launch of the call (at most 64 queries on the latency path: read in
 *               place, no ingest at all);
 *   results     are written into the caller's out_ids / out_dists / out_counts by the final kernel of the search -- no device-side
 *               result block, no device-to-host copy (all three arrays must be known, otherwise the library's pinned block is used).
 * Arrays the library does not know are staged through its own pinned buffers as before; results are identical either way.
 *   ivfadc_host_alloc       page-locked memory owned by the library (any device may read / write it); free with ivfadc_host_free
 *   ivfadc_host_register    page-locks an array of the CALLER's (e.g. a Julia Matrix{Float32} that a serving loop refills): the caller
 *                           keeps it alive and unmoved until ivfadc_host_unregister(p).  Registering costs tens of microseconds per
 *                           megabyte: do it once per buffer, not per call.
 * Thread-safe (one process-wide table).  IVFADC_ERR_INVALID for a pointer the table does not hold / an overlapping registration. */
int ivfadc_host_alloc(size_t bytes, void **out);
int ivfadc_host_free(void *p);
int ivfadc_host_register(void *p, size_t bytes);
int ivfadc_host_unregister(void *p);

/* Where the host time of the host-pointer entries went (cumulative since creation / the last reset; microseconds of wall time on the
 * calling thread): stage_in = copies of unregistered queries into pinned memory, enqueue = issuing ingest + kernels, wait = polling for
 * completion, stage_out = copies of results out of the library's pinned block; and how many calls found their queries / results in
 * known memory.  ivfadc_reset_host_stats zeroes them.                                                                         */
typedef struct {
    double  stage_in_us, enqueue_us, wait_us, stage_out_us;
    int64_t calls;             /* ivfadc_search + ivfadc_search_batches calls */
    int64_t batches;           /* batches searched by them */
    int64_t queries_direct;    /* calls whose queries were read from the caller's own (known) array */
    int64_t results_direct;    /* calls whose results were written straight into the caller's arrays */
    int64_t zero_copy;         /* calls whose queries were read in place by the search kernels (latency path) */
    int64_t streams_replaced;  /* since creation: streams of this handle's views / copy lane that were found to share a hardware queue
                                * with a stream they must run beside, and were replaced (probe at ivfadc_clone_view / first batch run) */
} ivfadc_host_stats;
int ivfadc_get_host_stats(ivfadc_t *h, ivfadc_host_stats *out);
int ivfadc_reset_host_stats(ivfadc_t *h);

/* A read-only VIEW of an index: a second handle on the SAME device arrays (quantizers, derived tables, inverted lists -- nothing is copied)
 * with a stream and a workspace of its own, so that two batches can be in flight on one replica: searches on h and on the view overlap
 * on the device.  (The reference's knn_search is a pure function of the index, index.jl:261-273: concurrent searches are independent.)
 * A view cannot change anything (push!/delete/set_lists/save return IVFADC_ERR_STATE) and keeps no host mirror.  Any change to h
 * afterwards (ivfadc_append, ivfadc_delete_ids, ivfadc_shift_ids, ivfadc_set_lists, ivfadc_synth_lists) makes every view of it refuse to
 * search (IVFADC_ERR_STATE: take a new one); a mutator first waits for the searches still in flight on h's views (their streams).
 * Settings (pruning, tuning, table mode, ...) are copied when the view is taken and can be set on it separately afterwards.
 * Destroy views with ivfadc_destroy, before or after h (a view that outlives h refuses to search).                                  */
int ivfadc_clone_view(ivfadc_t *h, ivfadc_t **out_view);

/* A SUBSET view: filtered search (a tenant, a category, a time window, "everything except what I already showed") without touching h.
 * Stands for: deleteat! of utils.jl:98-99 applied, on a copy of the lists, to every entry that is NOT selected -- WITHOUT the
 * _shift_inverse_index! that delete_from_index! adds (utils.jl:101-104): the kept entries stay in their stored order within each list
 * and keep their stored ids; the quantizers are h's.  A search on the view is knn_search (index.jl:204-258) on those lists: it visits in
 * (probe rank, list position) order, breaks ties by that order and returns fewer than K results where the probed lists hold fewer
 * points.  The view behaves exactly as a handle that was given the filtered lists through ivfadc_set_lists, and every scan form serves it.
 *   bitmap      over STORED ids (the 0-based ones a search returns): id i is selected iff i < nbits and bit (i & 31) of word bits[i >> 5]
 *               is set; bits holds ceil(nbits / 32) words, little-endian within a word.  Entries that share an id are all kept or all
 *               dropped; ids at or above nbits are not selected.  nbits <= 2^32.  nbits == 0 is the empty subset (bits may be NULL):
 *               a valid index with n = 0, every query returns count 0.
 *   out_n       (may be NULL) the number of entries kept.
 *   _device     the bitmap lies in device memory of h's GPU and is complete when the call is made (the compaction runs on h's stream).
 * The compaction runs on the device from h's device arrays (two kernels, csrc/subset.hip.h; no host mirror involved), so it serves
 * UInt8 and UInt16 handles, :opq-loaded handles and device-synthesised lists alike; the call is blocking.  A list partition set on h
 * is copied, like every setting.
 * View rules, as for ivfadc_clone_view: the quantizers and derived tables are SHARED with h, the lists are the view's own (freed by
 * ivfadc_destroy), stream and workspace are its own.  The view is read-only: every mutator, ivfadc_get_lists and ivfadc_save_index
 * return IVFADC_ERR_STATE; ivfadc_ntotal reports the subset.  Any change to h afterwards makes it refuse to search, as does destroying h
 * (IVFADC_ERR_STATE); a mutator of h first waits for the view's stream.  Every search entry a plain view serves, a subset view serves.
 * IVFADC_ERR_STATE: h is itself a view (plain or subset: take the subset from the index).  (A handle that was never given lists is an
 * empty index, as for ivfadc_search, and so is every subset of it.)  IVFADC_ERR_INVALID, before any device call: NULL h, NULL out_view,
 * NULL bits with nbits > 0, nbits > 2^32.
 * Not covered: subsets of ivfadc_mg_* handles.  (Predicates evaluated per query inside the scan: ivfadc_search_masked, below.)          */
int ivfadc_clone_subset(ivfadc_t *h, const uint32_t *bits, uint64_t nbits, ivfadc_t **out_view, int64_t *out_n);
int ivfadc_clone_subset_device(ivfadc_t *h, const uint32_t *d_bits, uint64_t nbits, ivfadc_t **out_view, int64_t *out_n);

/* PER-QUERY filtered search: one batch whose queries carry different predicates (a tenant per query, a category per query, "not what this
 * user has already seen"), with no copy of the lists.  A MASK SET is nmasks bitmaps over STORED ids with the bit definition of
 * ivfadc_clone_subset: id i is selected by mask r iff i < nbits and bit (i & 31) of word bits[r * ceil(nbits / 32) + (i >> 5)] is set.
 * Entries that share an id are kept or dropped together; ids at or above nbits are never selected.  At creation the set is converted
 * once, on the device, into one bit per stored entry in list order (csrc/maskset_plan.h, csrc/maskset.hip.h), which the list scan tests.
 *
 * ivfadc_search_masked gives every query a mask number, mask_of_query[q]:
 *   r >= 0      the result of query q is knn_search (index.jl:204-258) on the lists with every entry mask r does not select removed by
 *               deleteat! (utils.jl:98-99, without _shift_inverse_index!).  The w probed cells, their order and their coarse distances
 *               are those of the UNFILTERED index (a filter does not move centroids); the visit order is (probe rank, stored position),
 *               ties go by visit order, the count is min(K, selected entries in the probed lists).  Byte for byte what
 *               ivfadc_clone_subset(h, mask r) returns for that query.
 *   -1          (the -1 rule) no filter: the bytes of a plain ivfadc_search of that query.
 *   NULL array  every query uses mask 0.
 * The host entry validates mask_of_query before any launch: a value outside [-1, nmasks) is IVFADC_ERR_INVALID naming the query.  The
 * device entry cannot validate without a synchronisation: its ingest clamps every value into [-1, nmasks), so a violated precondition
 * cannot read outside the set; that query's results are then unspecified.
 *
 * Mask set creation: 1 <= nmasks, nbits <= 2^32; nbits == 0 is the empty mask (bits may be NULL).  out_kept (nmasks values, may be NULL):
 * the entries each mask selects.  IVFADC_ERR_INVALID, before any device call: NULL h, NULL out, nmasks < 1, NULL bits with nbits > 0,
 * nbits > 2^32.  The set is made from the index itself: a view or a subset view is refused with IVFADC_ERR_STATE (take it from the index
 * itself).  Creation uploads pending list changes first and is blocking; _device: the bitmaps lie in device memory of h's GPU and are
 * complete when the call is made.  It reads only ids, so it serves UInt8 and UInt16 handles, :opq-loaded handles and device-synthesised
 * lists alike.  A mask set is immutable: any number of handles and threads may search with it at once; destroying it while a search with
 * it is in flight is the caller's error, as for ivfadc_destroy.
 *
 * h and s (the view rule): h is the index s was made from, or a plain view of it (ivfadc_clone_view: the same lists, so two masked batches
 * can be in flight on one replica).  IVFADC_ERR_STATE: a subset view; another index; an index that has changed since s was made (any
 * mutator, by the generation rule of views); a handle with a list partition set.  K < 1 or w < 1: IVFADC_ERR_ASSERT, as ivfadc_search;
 * w > kc is clamped as ivfadc_search clamps it.  Every K and w is served; batches are sub-batched under ivfadc_set_workspace_limit; a
 * pending hint is dropped, as by any search.  There is no latency path, no fused top-w and no riders.  The 8-bit list scan is
 * masked_scan_kernel (stats.last_striped == 8); K or w > 2048, ivfadc_set_tuning(h, -2, 0) and every UInt16 handle take the generic path,
 * where a rejected point's key sorts behind every real key.  The device entry is asynchronous on the handle's stream.
 * Not covered: masks in the query-major, eight-wave, narrow-field and UInt16 scan kernels; masks together with caller-supplied probes;
 * ivfadc_search_batches, ivfadc_mg_*, the list-partitioned mode and the all-gather entries; predicates other than id bitmaps.         */
typedef struct ivfadc_maskset ivfadc_maskset_t;
int ivfadc_maskset_create(ivfadc_t *h, int nmasks, const uint32_t *bits, uint64_t nbits, ivfadc_maskset_t **out, int64_t *out_kept);
int ivfadc_maskset_create_device(ivfadc_t *h, int nmasks, const uint32_t *d_bits, uint64_t nbits, ivfadc_maskset_t **out, int64_t *out_kept);
void ivfadc_maskset_destroy(ivfadc_maskset_t *s);
int ivfadc_search_masked(ivfadc_t *h, const ivfadc_maskset_t *s, int64_t nq, const float *queries, int K, int w,
                         const int32_t *mask_of_query, uint32_t *out_ids, float *out_dists, int32_t *out_counts);
int ivfadc_search_device_masked(ivfadc_t *h, const ivfadc_maskset_t *s, int64_t nq, const float *d_queries, int K, int w,
                                const int32_t *d_mask_of_query, uint32_t *d_out_ids, float *d_out_dists, int32_t *d_out_counts);

/* RANGE search: every stored point of the w probed lists within distance r of a query (NearestNeighbors.jl's inrange; other IVF
 * libraries' range_search).  NO REFERENCE COUNTERPART: IVFADC.jl has knn_search only, so the six entries below are DEFINED through it.
 * For a query q, a radius r (Float32, in the units of the index's distance: SQUARED Euclidean) and w probes, the result is
 * knn_search(index, q, K; w) (index.jl:204-258) with K at least the number of points in the w probed lists, cut after the last entry whose
 * Float32 distance d satisfies d <= r.  Hence: the same w cells (w > kc is clamped as ivfadc_search clamps it), the same sums (d = dc, then
 * += tab[ii] in ascending ii), the same order (ascending distance, then probe rank, then list position), the same stored ids; ids and
 * distance bits are those ivfadc_search returns for the same entries.  The comparison is INCLUSIVE: a run of ties at exactly r comes back
 * whole, in visit order.  r < 0: no results.  r = +inf: every probed point.  A NaN radius: the host entry returns IVFADC_ERR_INVALID naming
 * the query, before any launch; for the device entry "no NaN" is a precondition, and a NaN radius gives that query no results (d <= NaN is
 * false).  radii holds one radius per query (a caller with one radius fills the array).
 *
 * The result's size is known only after the counting pass, so the result is an object the LIBRARY owns: CSR rows -- lims (nq + 1 int64,
 * lims[0] = 0), ids and dists (lims[nq] each), query q's entries at [lims[q], lims[q + 1]) -- in device memory of the handle's GPU.
 * ivfadc_range_result_sizes gives nq and the total, _copy copies to host arrays of those sizes (any of the three may be NULL), _device
 * lends the device arrays (valid until the result is destroyed).  Both search entries are BLOCKING: the result is complete on return.
 * A result belongs to no handle: it outlives later searches, mutators and ivfadc_destroy of the handle it came from -- destroying it
 * after the handle is SAFE -- and is freed only by ivfadc_range_result_destroy (NULL: a no-op).
 *
 * max_total > 0 caps the result: when the counted total exceeds it the call returns IVFADC_ERR_INVALID with the needed total in
 * ivfadc_last_error(), before anything of the result is allocated; *out stays NULL and the handle serves the next call as usual.
 * max_total = 0: no cap.  IVFADC_ERR_INVALID, before the handle is looked at or the device is touched: NULL out, max_total < 0, nq < 0,
 * NULL radii, NULL queries with nq > 0, a NaN radius (host entry), NULL h.  w < 1: IVFADC_ERR_ASSERT with the text of index.jl:211.
 * IVFADC_ERR_STATE: a handle with UInt16 codes (8-bit handles only), a handle with a list partition set, no lists yet, a stale view.
 * Served: plain handles, ivfadc_clone_view views, subset views, file-loaded handles (:opq included: a search never reads the rotation),
 * stored ids and device-synthesised lists, indexes after push! / delete.  Batches are sub-batched under ivfadc_set_workspace_limit (queries
 * are independent: the rows concatenate); the calls run on the handle's stream (ivfadc_set_stream) under the handle's lock; a pending hint
 * is dropped, as by any search; the probed points count into stats.scanned_points and the queries into stats.queries, and that is ALL a
 * range search writes into ivfadc_stats: last_qg, last_chunk, last_striped and the other last_* fields go on describing the last
 * ivfadc_search-family call.  _copy and _destroy leave the calling thread's current device as they found it.  ivfadc_set_tuning's chunk_points, when not 0, is the
 * points of a work item (rounded up to a multiple of 64); limits: a query's probed points < 2^32, the tables of one probe within the LDS
 * of a compute unit (csrc/range_plan.h).
 * Not covered by these two entries: UInt16 handles and mask sets (both served by ivfadc_range_search_masked, below).  Not covered at all:
 * the list-partitioned mode, ivfadc_mg_* and the all-gather entries, ivfadc_search_batches.                                               */
typedef struct ivfadc_range_result ivfadc_range_result_t;
int ivfadc_range_search(ivfadc_t *h, int64_t nq, const float *queries, const float *radii, int w, int64_t max_total,
                        ivfadc_range_result_t **out);
int ivfadc_range_search_device(ivfadc_t *h, int64_t nq, const float *d_queries, const float *d_radii, int w, int64_t max_total,
                               ivfadc_range_result_t **out);
int ivfadc_range_result_sizes(const ivfadc_range_result_t *r, int64_t *out_nq, int64_t *out_total);
int ivfadc_range_result_copy(const ivfadc_range_result_t *r, int64_t *lims, uint32_t *ids, float *dists);
int ivfadc_range_result_device(const ivfadc_range_result_t *r, const int64_t **d_lims, const uint32_t **d_ids, const float **d_dists);
void ivfadc_range_result_destroy(ivfadc_range_result_t *r);

/* MASKED range search: "everything within r that this query is allowed to see", and the range search of handles with UInt16 codes.  NO
 * REFERENCE COUNTERPART.  Query q with mask r = mask_of_query[q] >= 0 of the set s gets what ivfadc_search_masked returns for it with K at
 * least the number of probed points, cut after the last entry with d <= radii[q]: the w cells, their order and their coarse distances are
 * those of the UNFILTERED index, the sums are the reference's (d = dc, then += tab_ii[code[ii]] in ascending ii), the order is (distance,
 * probe rank, stored position) with ORIGINAL visit numbers, ids are the stored ids; ids and distance bits match.  -1 gives what
 * ivfadc_range_search gives; mask_of_query == NULL with a set means mask 0 for every query.  Everything said above about the radius
 * (inclusive, r < 0, +inf, NaN, -0), about max_total, the result object (an ordinary ivfadc_range_result_t: _sizes, _copy, _device and
 * _destroy serve it), blocking, the stream, the lock, the dropped hint and ivfadc_stats (scanned_points -- every probed point once,
 * selected or not -- and queries; nothing else) holds unchanged.
 * s == NULL: no query is filtered; mask_of_query must then be NULL (IVFADC_ERR_INVALID otherwise), and the entry is ivfadc_range_search
 * on every handle state that entry serves PLUS handles with UInt16 codes (256 < k <= 65536): their sums come straight from the codebook
 * (no tables; csrc/range.hip.h), bit for bit what ivfadc_search returns.
 * With a set, served: what ivfadc_search_masked serves -- the index the set was made from, unchanged since, or a plain ivfadc_clone_view
 * view of it; 8-bit and UInt16 handles; file-loaded handles; after push! / delete with a set made after the change.  IVFADC_ERR_STATE: a
 * subset view together with a set, a set of another index, an index changed since the set was made, a list partition, a stale view.
 * Argument errors (IVFADC_ERR_INVALID, before the handle is looked at or the device is touched, in this order): NULL out, max_total < 0,
 * nq < 0, NULL radii, NULL queries with nq > 0, a NaN radius (host entry), NULL h; w < 1 is IVFADC_ERR_ASSERT as above; *out is cleared
 * on failure.  The host entry validates mask_of_query before any launch (a value outside [-1, nmasks): IVFADC_ERR_INVALID naming the
 * query); the device entry clamps it into that range.  Limits: csrc/range_plan.h (UInt16: the residual within the LDS of a compute unit;
 * a work item is 1024 points unless ivfadc_set_tuning's chunk_points says otherwise).
 * Not covered: the list-partitioned mode, ivfadc_mg_* and the all-gather entries, ivfadc_search_batches, the Julia shim.               */
int ivfadc_range_search_masked(ivfadc_t *h, const ivfadc_maskset_t *s, int64_t nq, const float *queries, const float *radii, int w,
                               int64_t max_total, const int32_t *mask_of_query, ivfadc_range_result_t **out);
int ivfadc_range_search_device_masked(ivfadc_t *h, const ivfadc_maskset_t *s, int64_t nq, const float *d_queries, const float *d_radii,
                                      int w, int64_t max_total, const int32_t *d_mask_of_query, ivfadc_range_result_t **out);

/* Same, with every buffer already resident in device memory of the handle's GPU.
 * Asynchronous on the handle's stream; pair with ivfadc_sync().                          */
int ivfadc_search_device(ivfadc_t *h, int64_t nq, const float *d_queries, int K, int w,
                         uint32_t *d_out_ids, float *d_out_dists, int32_t *d_out_counts);

/* LOCATE and RECONSTRUCT: "what is stored under this id", on the device copy of the lists.
 * Replaces: the search loop of _pop! (utils.jl:49-55) and _get_quantizer_vector(cq, cluster) + _decode_point(rq, codes) (utils.jl:58-59,
 * 71-81) for a batch of ids, WITHOUT the removal (pop! = ivfadc_reconstruct of one id, then ivfadc_delete_ids of it).  No host mirror is
 * involved (csrc/reconstruct_plan.h, csrc/reconstruct.hip.h).
 * For a requested id v, a stored entry counts only if it lies below its list's length (list_len: spare capacity behind it holds stale rows).
 *   location        locate(v) = (list l, position p), both 0-based, as the reference's loop finds them: l is the LAST list that holds v (the
 *                   loop does not break, so later lists overwrite), p is the FIRST position of v within that list (findfirst).  Ids are
 *                   unique in every index the reference can build; for caller-supplied lists with repeated ids this is still the rule.
 *   reconstruction  reconstruct(v)[t] = centroid_l[t] + codebooks[ii][c][t - ii * dsub], ii = t / dsub, c = the codeword the stored code of
 *                   sub-space ii names (an 8-bit code is a LABEL and is translated through code_labels; a 16-bit code likewise at the
 *                   boundary): ONE IEEE Float32 addition per component, bit-identical to the reference's sum in Float32 -- subnormal,
 *                   signed-zero and large-magnitude components included.
 *   rotation        the rotation of an :opq file is NOT applied: _decode_point does not apply it either (utils.jl:71-81).
 *   absent id       no list holds v: out_list = -1, out_pos = -1, found = 0 and the d floats of the vector are +0.0.  Not an error.
 *   requests        answered slot by slot, in request order; an id may be requested any number of times.  Ids are unsigned 32-bit numbers
 *                   everywhere (0xFFFFFFFF is an id).
 * out_vectors is d x n (vector j at + j * d); out_found (n bytes) may be NULL.
 * Served: 8-bit and UInt16 handles; plain views (ivfadc_clone_view); subset views (the view's OWN lists: an id the subset dropped is
 * absent, a kept id is located in the subset's lists); file-loaded handles, :opq included; device-synthesised lists; an index after
 * push! / delete / shift -- pending list changes (an append that overflowed a list) are laid out first, as a search does.  A view whose
 * index has changed refuses with IVFADC_ERR_STATE, as for searches; so do a handle that was never given lists and a handle with a list
 * partition set.
 * The host entries block.  The _device entries take every pointer in device memory of h's GPU and follow the stream semantics of
 * ivfadc_search_device: asynchronous on the handle's stream, pair with ivfadc_sync(); at most 2^31 - 1 ids per call.
 * Argument errors, IVFADC_ERR_INVALID before the handle is looked at or the device is touched, each named in ivfadc_last_error(): null
 * handle; n < 0; null ids with n > 0; a null output (out_found alone may be NULL).  n == 0 returns IVFADC_OK.
 * Cost: ONE pass over the stored ids (4 bytes per entry) behind an exact bitmap over the span of the wanted ids, or, for at most 16 384
 * ids that span more than 2^30 values or whose span the host does not know (_device entries), behind a hashed filter in LDS; then n
 * workgroups of decode.  A _device call with more ids sizes the bitmap's buffer for the whole id space (512 MB of workspace that stays
 * with the handle) and zeroes and reads only the ids' own span, which its kernels take from the sorted ids.  The _device entries upload
 * nothing and wait for nothing: every step is enqueued on the stream (a workspace buffer that must grow is reallocated, as by a search).
 * Not covered: ivfadc_mg_* handles and the list-partitioned mode.                                                                       */
int ivfadc_locate(ivfadc_t *h, int64_t n, const uint32_t *ids, int32_t *out_list, int64_t *out_pos);
int ivfadc_reconstruct(ivfadc_t *h, int64_t n, const uint32_t *ids, float *out_vectors, uint8_t *out_found);
int ivfadc_locate_device(ivfadc_t *h, int64_t n, const uint32_t *d_ids, int32_t *d_out_list, int64_t *d_out_pos);
int ivfadc_reconstruct_device(ivfadc_t *h, int64_t n, const uint32_t *d_ids, float *d_out_vectors, uint8_t *d_out_found);

/* SCORE caller-supplied candidate ids: "what distance would knn_search report between this query and these stored ids", with no scan of
 * the lists (csrc/score_plan.h, csrc/score.hip.h).  For candidates that come from elsewhere: a hybrid retriever's lexical hits, a rerank
 * stage, a seen-list, a consistency check between two indexes, the ADC distance of the true neighbours in a recall study.
 * For query q and candidate id v let (l, p) = locate(v), as ivfadc_locate finds them (utils.jl:49-55: the LAST list that holds v, the
 * FIRST position within it; entries at or behind list_len do not count).  Then, in Float32, one rounding per operation, nothing contracted:
 *   dc   = 0;  t = 0 .. d-1:            u = C_l[t] - q[t];          dc = dc + u * u        (coarsequantizers.jl:33-34)
 *   r[t] = q[t] - C_l[t]                                                                   (coarsequantizers.jl:40-45)
 *   s_ii = 0;  t of sub-space ii, ascending:  u = CB_ii[c_ii][t] - r[t];  s_ii = s_ii + u * u   (index.jl:232-236)
 *   dist = dc; ii = 0 .. m-1:           dist = dist + s_ii                                 (index.jl:242-246)
 * c_ii is the codeword the stored code names, read as ivfadc_reconstruct reads it (an 8-bit code is a LABEL and goes through the inverse
 * of code_labels; a 16-bit code is the codeword index).  dist is the number knn_search(index, q, K; w) -- ivfadc_search -- returns for v
 * whenever v is among its results, BIT FOR BIT, on 8-bit and UInt16 handles alike, so scored candidates merge with search results.
 *   rotation        the rotation of an :opq file is NOT applied: the scan does not apply it either.
 *   absent id       no list holds v (or a subset view dropped it): dist = +Inf (bits 0x7F800000), found = 0.  Not an error; absent ids
 *                   sort last.
 *   layout          queries is d x nq, as for ivfadc_search.  Row q of ids starts at ids + q * ids_stride and holds C slots:
 *                   ids_stride == C is one candidate list per query; ids_stride == 0 is ONE shared row scored against every query (all
 *                   pairs; its locate runs once, over C ids); any other stride is IVFADC_ERR_INVALID.  counts may be NULL: all C slots
 *                   are live.  Otherwise slot j >= counts[q] is dead: its id is not scored and it comes back as +Inf / 0.  The host entry
 *                   refuses a counts[q] outside [0, C], naming the query; the _device entry clamps it.  out_dists is nq x C (pair (q, j)
 *                   at q * C + j); out_found is nq x C bytes and may be NULL.
 *   requests        answered slot by slot; an id may repeat within a row and across rows.  Ids are unsigned 32-bit numbers (0xFFFFFFFF
 *                   is an id).  At most 2^31 - 1 pairs (nq x C) per call: more is IVFADC_ERR_INVALID.
 *   non-finite      queries are not scanned, as for ivfadc_search: a NaN or infinite component propagates into that query's distances.
 * Served: 8-bit and UInt16 handles; plain views (ivfadc_clone_view); subset views (the view's OWN lists: an id the subset dropped is
 * absent, a kept id has the distance it has on the index); file-loaded handles, :opq included; device-synthesised lists; an index after
 * push! / delete / shift -- pending list changes are laid out first, as a search or a locate does.  A view whose index has changed, a
 * handle that was never given lists and a handle with a list partition set refuse with IVFADC_ERR_STATE, as ivfadc_locate does.
 * The host entry blocks.  The _device entry takes every pointer in device memory of h's GPU and only enqueues on the handle's stream: it
 * uploads nothing and waits for nothing (asynchronous; pair with ivfadc_sync()).  Both take the per-handle lock.
 * Under ivfadc_set_workspace_limit the call is cut into slices of whole queries whose locate workspace (32 bytes per slot) fits; the
 * shared row is located once and only the pair kernel is sliced.
 * Argument errors, IVFADC_ERR_INVALID before the handle is looked at or the device is touched, each named in ivfadc_last_error(): null
 * handle; nq < 0; C < 0; a stride that is neither C nor 0; more than 2^31 - 1 pairs; with nq > 0 and C > 0, null queries, null ids or
 * null out_dists; (host entry) a counts[q] outside [0, C].  nq == 0 or C == 0 returns IVFADC_OK.
 * Cost: the locate pass (one pass over the stored ids, 4 bytes per entry, per slice) plus, per pair, two reads of a centre row and one
 * of m codewords, all cache-resident -- against n stored entries per QUERY for a masked search over the same ids.
 * Not covered: ivfadc_mg_* handles, the list-partitioned mode, ivfadc_search_batches.                                                  */
int ivfadc_score_ids(ivfadc_t *h, int64_t nq, const float *queries, int64_t C, int64_t ids_stride, const uint32_t *ids,
                     const int32_t *counts, float *out_dists, uint8_t *out_found);
int ivfadc_score_ids_device(ivfadc_t *h, int64_t nq, const float *d_queries, int64_t C, int64_t ids_stride, const uint32_t *d_ids,
                            const int32_t *d_counts, float *d_out_dists, uint8_t *d_out_found);

/* The seam of the reference's knn_search.  index.jl:204-258 calls coarse_search(cq, point, w) once (index.jl:219) and everything after it
 * -- residuals, ADC tables, the list scan seeded with dc, top-K (index.jl:220-257) -- reads only the two vectors it returns;
 * AbstractCoarseQuantizer (coarsequantizers.jl:6) is the reference's one plug-in interface.  The two halves are exported separately, so a
 * caller can take the coarse result out, or put ANY coarse result in: the reference's HNSW quantizer (coarsequantizers.jl:73-76, run on
 * the CPU by the Julia shim), a learned router, a cached assignment, one coarse search shared between several indexes.
 *
 * Replaces: coarse_search(cq, point, w) (coarsequantizers.jl:33-37, NaiveQuantizer) for a batch.  Row q of out_lists / out_dists (w slots
 * per query) holds the w closest cells of query q: 0-based, ascending distance, ties to the lower cell (sortperm is stable), in rank
 * order.  1 <= w <= kc: w < 1 -> IVFADC_ERR_ASSERT (the text of index.jl:211), w > kc -> IVFADC_ERR_INVALID (sortperm(...)[1:w] would
 * throw).  The bytes are the same in every coarse mode (ivfadc_set_coarse_mode) and are the probes a plain search of the same queries
 * visits.  Batches are cut into sub-batches under ivfadc_set_workspace_limit; a pending hint (ivfadc_set_next_queries) is dropped as by
 * any search.  The _device form takes device pointers and is asynchronous on the handle's stream: the selection kernel writes straight
 * into the caller's rows.                                                                                                      */
int ivfadc_coarse_search(ivfadc_t *h, int64_t nq, const float *queries, int w, int32_t *out_lists, float *out_dists);
int ivfadc_coarse_search_device(ivfadc_t *h, int64_t nq, const float *d_queries, int w, int32_t *d_lists, float *d_dists);

/* Replaces: index.jl:220-257 given the output of ANY coarse_search (coarsequantizers.jl:33-37 or :73-76).  Row q of lists /
 * coarse_dists = the w probes of query q in VISIT (rank) order; the outputs are laid out as ivfadc_search's.
 *   visit order   the supplied rank, NOT the order of the supplied distances: a key is (f32 bits of d) << 32 | (base of rank j + position
 *                 in the list), base = exclusive prefix sum of the list lengths over the supplied ranks (index.jl:228-255 visits the
 *                 clusters in the order coarse_search returned them)
 *   distance seed d starts at the supplied coarse_dists[q][j], not at a recomputed distance (index.jl:229,242)
 *   residual      q - centroid[lists[q][j]] (coarsequantizers.jl:40-45, 79-89)
 * Results do not depend on whether the supplied distances ascend: exact pruning judges every list against the bound by itself (a plain
 * search may stop at the first list above the bound because ITS probes ascend; here that list alone is skipped).
 * Fed with the output of ivfadc_coarse_search, the results are the bytes of ivfadc_search.
 * Preconditions on the probes: list numbers in [0, kc); the lists of one query pairwise distinct; distances finite and >= +0 (no -0:
 * pruning and selection compare float bits as unsigned).  1 <= w <= kc (w > kc -> IVFADC_ERR_INVALID; K < 1, w < 1 -> IVFADC_ERR_ASSERT
 * as ivfadc_search).
 *   ivfadc_search_preassigned         host pointers, blocking.  Validates every precondition on the host BEFORE any launch and returns
 *                                     IVFADC_ERR_INVALID naming the query, the rank and the reason.
 *   ivfadc_search_device_preassigned  device pointers, asynchronous on the handle's stream.  Cannot validate without a synchronisation:
 *                                     the preconditions are the caller's.  Its ingest kernel clamps every list number into [0, kc) and
 *                                     reads a distance outside [+0, FLT_MAX] as +0, so a violated precondition cannot index outside
 *                                     the index; the results of that query are then unspecified.
 * Both serve UInt8 and UInt16 handles, views, :opq-loaded handles and device-synthesised lists, every K and w <= kc (the plans of a plain
 * search minus its coarse stage: no latency path, no fused top-w, no riders; a pending hint is dropped as by any search), and
 * sub-batch under ivfadc_set_workspace_limit.  A handle with a list partition set (ivfadc_set_list_partition, nparts > 1) ->
 * IVFADC_ERR_STATE.                                                                                                            */
int ivfadc_search_preassigned(ivfadc_t *h, int64_t nq, const float *queries, int K, int w, const int32_t *lists, const float *coarse_dists,
                              uint32_t *out_ids, float *out_dists, int32_t *out_counts);
int ivfadc_search_device_preassigned(ivfadc_t *h, int64_t nq, const float *d_queries, int K, int w, const int32_t *d_lists,
                                     const float *d_coarse_dists, uint32_t *d_out_ids, float *d_out_dists, int32_t *d_out_counts);

/* Replaces: a loop of knn_search(ivfadc, points, k; w) calls over consecutive batches (index.jl:261-273 once per batch) -- ONE call for
 * the whole run.  batch_nq[b] queries per batch; queries is d x sum(batch_nq), the batches back to back; outputs are laid out like
 * ivfadc_search's for the concatenated queries (K slots per query).  Every batch's results are exactly what ivfadc_search returns
 * for it.  Inside, batch b is searched with batch b + 1 named as its successor (ivfadc_set_next_queries below, on device buffers and
 * tokens the library owns), so plans with the rider form run one launch per batch.  From two batches on, TWO are in flight: the odd
 * ones run on an internal view of the handle (ivfadc_clone_view: second stream, second workspace, same device arrays), each lane naming
 * its own next batch as the successor -- a launch's ramp and tail leave the chip half empty, a second stream fills them.  Results are
 * unchanged bit for bit; IVFADC_NO_PIPELINE=1 (environment) keeps one batch in flight, and so does profiling (ivfadc_set_profiling: the
 * kernel timings are this handle's).  The cumulative counters of ivfadc_get_stats include the view's share.                              */
int ivfadc_search_batches(ivfadc_t *h, int nbatches, const int64_t *batch_nq, const float *queries, int K, int w,
                          uint32_t *out_ids, float *out_dists, int32_t *out_counts);

int ivfadc_sync(ivfadc_t *h);

/* Single-process multi-device front end: one replica of the index per listed device, contiguous
 * query blocks per device, every device's block in flight at once; results come back in query order.  The
 * one-process-per-GPU form (torch.distributed / RCCL all-gather of the packed top-k) is ivfadc.jl_amd/distributed.py.
 * Same argument meaning and status codes as the single-device calls.                                         */
typedef struct ivfadc_mg ivfadc_mg_t;
int ivfadc_mg_create(ivfadc_mg_t **out, int ndev, const int *devices, int d, int kc, int m, int ksub,
                     const float *centroids, const float *codebooks, const uint8_t *code_labels);
int ivfadc_mg_set_lists(ivfadc_mg_t *g, const int64_t *offsets, const uint8_t *codes, const uint32_t *ids);   /* replicas upload concurrently */
/* every replica synthesises the same lists on its own device (see ivfadc_synth_lists): how the billion-point
 * benchmark shapes are loaded into the single-process front end                                              */
int ivfadc_mg_synth_lists(ivfadc_mg_t *g, const int64_t *offsets, uint64_t seed);
int ivfadc_mg_num_devices(ivfadc_mg_t *g);
/* Result merge of ivfadc_mg_search.  0 (default): each device's block is copied to the caller's arrays as it
 * completes.  1: the final top-k merge of the batch is ONE ncclAllGather (RCCL over xGMI; ncclCommInitAll, one
 * stream per device) of the packed per-device blocks [ids | dists | counts] -- no reduction: devices own disjoint
 * queries (index.jl:269-271) -- after which every device holds the batch's results and the host reads device
 * 0's copy.  Needs distinct devices; RCCL is bound at run time (dlopen) and IVFADC_ERR_STATE is returned if absent. */
int ivfadc_mg_set_gather(ivfadc_mg_t *g, int mode);
int ivfadc_mg_collectives(ivfadc_mg_t *g, int64_t *out);   /* all-gathers issued so far (mode 1) */
int ivfadc_mg_append(ivfadc_mg_t *g, int64_t nnew, const float *pts, const uint32_t *ids,
                     int32_t *out_list, uint8_t *out_codes);
int ivfadc_mg_delete_ids(ivfadc_mg_t *g, int64_t ndel, const uint32_t *ids, int64_t *out_removed);   /* every replica */
int ivfadc_mg_shift_ids(ivfadc_mg_t *g, int32_t delta);
int ivfadc_mg_search(ivfadc_mg_t *g, int64_t nq, const float *queries, int K, int w,
                     uint32_t *out_ids, float *out_dists, int32_t *out_counts);
void ivfadc_mg_destroy(ivfadc_mg_t *g);

/* One process per GPU: the final top-k merge of a batch inside the library.  Every rank holds a replica of the
 * index and a contiguous block of the batch's queries (index.jl:269-271: queries are independent).
 *   ivfadc_comm_unique_id   rank 0 creates the 128-byte RCCL id; the host framework carries it to the other ranks
 *   ivfadc_comm_init        ncclCommInitRank on the handle's device (collective: every rank calls it)
 *   ivfadc_search_device_allgather
 *                           ivfadc_search_device of this rank's nq queries into d_block -- packed [ids nq*K | dists nq*K |
 *                           counts nq] int32 -- followed by ONE ncclAllGather of that block into d_gathered (nranks blocks, rank
 *                           order) on a side stream of the handle: the collective overlaps the next batch's kernels.  Every
 *                           rank passes the same nq and K within one call (the collective's contract: equal blocks; a single rank
 *                           cannot detect a mismatch); the block size may change from call to call if every rank changes it alike.
 *                           d_gathered holds nranks x nq x (2K + 1) words.  slot in [0, 8) names the buffer pair; a
 *                           slot's previous collective is waited for on the device before the slot is written again -- rotate all
 *                           eight slots: one wait then serves several steps (collectives finish in issue order, and a wait in the
 *                           search stream costs the next kernel ~6 us of idle queue whether its event has fired or not).
 *   ivfadc_comm_wait        the search stream waits for every collective issued so far; out_collectives (may be NULL) counts them
 * RCCL is bound at run time (dlopen); IVFADC_ERR_STATE if it is absent or the communicator has not been set up.      */
int ivfadc_comm_unique_id(uint8_t *out_id128);
int ivfadc_comm_init(ivfadc_t *h, int nranks, int rank, const uint8_t *id128);
int ivfadc_search_device_allgather(ivfadc_t *h, int64_t nq, const float *d_queries, int K, int w,
                                   int32_t *d_block, int32_t *d_gathered, int slot);
/* The same with the search on `searcher` -- h itself or a view of it (ivfadc_clone_view: two batches in flight per rank) -- and the
 * collective where the communicator lives, on h's side stream, in call order.                                        */
int ivfadc_search_device_allgather_on(ivfadc_t *h, ivfadc_t *searcher, int64_t nq, const float *d_queries, int K, int w,
                                      int32_t *d_block, int32_t *d_gathered, int slot);
int ivfadc_comm_wait(ivfadc_t *h, int64_t *out_collectives);
int ivfadc_comm_destroy(ivfadc_t *h);

/* List-partitioned multi-GPU mode: strong scaling of a FIXED global batch.  Query shards over replicas stop scaling once a rank streams
 * most of the index for its few queries; here every rank keeps the replica and ALL nq queries, runs the coarse search (identical on every
 * rank: coarsequantizers.jl:33-37), scans only the probed lists l with l % nparts == part -- the probes of a query are independent given
 * the bound, index.jl:228-255 -- and leaves per query the K smallest KEYS of its lists (distance bits << 32 | visit order: visit orders are
 * global, so keys of different ranks compare and name one stored point each).  The index is still replicated and RCCL still carries only the
 * final top-k merge: ONE all-gather of nq x K keys per rank, then the K-way merge on every rank.
 *   ivfadc_set_list_partition      nparts = 1 switches the mode off.  While it is on, searches take the list-major plan, the batch must fit
 *                                  one sub-batch, K <= 2048 and w <= 2048 (IVFADC_ERR_INVALID otherwise); a plain ivfadc_search_device then
 *                                  returns the top-K of this rank's lists alone
 *   ivfadc_search_device_partial   d_keys nq x K (ascending per query), d_counts nq
 *   ivfadc_merge_partials_device   d_keys_all nparts x nq x K, d_counts_all nparts x nq -> ids, distances, counts of the whole scan; on the
 *                                  handle that ran the batch's partial search (its probe arrays translate visit orders into ids)
 *   ivfadc_search_device_listpart  the three steps in one call: partial search into d_block ([keys | counts], ivfadc_listpart_block_words
 *                                  int32 words), ncclAllGather into d_gathered (nranks blocks), merge.  Needs ivfadc_comm_init and
 *                                  ivfadc_set_list_partition(h, nranks, rank); every rank passes the same nq queries, K and w           */
int ivfadc_set_list_partition(ivfadc_t *h, int nparts, int part);
int ivfadc_search_device_partial(ivfadc_t *h, int64_t nq, const float *d_queries, int K, int w, uint64_t *d_keys, int32_t *d_counts);
int ivfadc_merge_partials_device(ivfadc_t *h, int64_t nq, int K, int nparts, const uint64_t *d_keys_all, const int32_t *d_counts_all,
                                 uint32_t *d_ids, float *d_dists, int32_t *d_counts);
int64_t ivfadc_listpart_block_words(int64_t nq, int K);
int ivfadc_search_device_listpart(ivfadc_t *h, int64_t nq, const float *d_queries, int K, int w, int32_t *d_block, int32_t *d_gathered,
                                  uint32_t *d_ids, float *d_dists, int32_t *d_counts);

/* Run on a caller-owned hipStream_t (e.g. the host framework's current stream) instead of the
 * handle's own stream, so searches order naturally with the caller's kernels and collectives. */
int ivfadc_set_stream(ivfadc_t *h, void *hip_stream);

/* Replaces: length(ivfadc) (index.jl:56) and the per-list lengths. list_sizes: kc entries or NULL. */
int ivfadc_ntotal(ivfadc_t *h, int64_t *out_n, int64_t *list_sizes);

/* Copies the host mirror of the lists back out (layout of ivfadc_set_lists).            */
int ivfadc_get_lists(ivfadc_t *h, int64_t *offsets, uint8_t *codes, uint32_t *ids);

/* The quantizers of a handle (what ivfadc_create took, or what ivfadc_load_index read: src/index.jl:39-48): dimensions first
 * (any pointer may be NULL), then the arrays in ivfadc_create's layout.                                               */
int ivfadc_get_dims(ivfadc_t *h, int *d, int *kc, int *m, int *ksub);
int ivfadc_get_quantizers(ivfadc_t *h, float *centroids /* kc x d */, float *codebooks /* m x ksub x dsub */, uint8_t *code_labels /* m x ksub */);

/* Replaces: save_ivfadc_index(filename, ivfadc) (persistency.jl:1-78) for a NaiveQuantizer / UInt8 / Float32 index:
 * byte for byte the reference's file (rotation matrix: identity, or the one the index was loaded with).  index_bits = width
 * of the reference's index type I (8, 16 or 32).                                                                 */
int ivfadc_save_index(ivfadc_t *h, const char *path, int index_bits);

/* Replaces: load_ivfadc_index(filename) (persistency.jl:82-134): reads a file written by IVFADC.jl (NaiveQuantizer,
 * U = UInt8, I <= 32 bits; Float64 values are narrowed) into a new handle, lists included.
 * out_index_bits (may be NULL) returns the width of I.                                                          */
int ivfadc_load_index(ivfadc_t **out, int device, const char *path, int *out_index_bits);

/* The rotation of the residual quantizer (QuantizedArrays' `rot`, persistency.jl:62-64, 110-117).  knn_search never reads it
 * (index.jl:204-258), so an index built with :opq is SEARCHED like any other: ivfadc_load_index keeps its matrix (and
 * ivfadc_save_index writes it back).  quantize_data -- push! (utils.jl:148-161) -- does read it, through third-party arithmetic
 * that cannot be verified here: ivfadc_encode / ivfadc_append return IVFADC_ERR_STATE on such a handle (delete / pop / shift are
 * fine: they touch ids only).  out_rotated: 0 = identity (:pq); out_rot (may be NULL): d x d floats, column by column.     */
int ivfadc_get_rotation(ivfadc_t *h, int *out_rotated, float *out_rot);

/* Measurement.  When profiling is on, every scan-kernel launch is bracketed by HIP events
 * on the handle's stream; ivfadc_get_stats synchronises and reports the totals since the
 * last ivfadc_reset_stats.                                                               */
typedef struct {
    double   scan_ms;          /* sum of scan-kernel durations (HIP events)               */
    double   coarse_ms;        /* sum of coarse-distance kernel durations                 */
    int64_t  scan_launches;
    int64_t  scanned_points;   /* sum over (query, probe) of len(list): x m = B_alg bytes  */
    int64_t  queries;
    int32_t  last_qg;          /* queries sharing one code stream in the last launch (0 = query-major kernel) */
    int32_t  last_chunk;       /* points per work item in the last launch                  */
    int32_t  last_scan_grid;
    int32_t  last_scan_lds;
    int64_t  coarse_fallbacks; /* queries whose MFMA-filter certificate failed (exact recompute taken)  */
    int32_t  coarse_mfma;      /* 1: the last batch used the MFMA filter + certified exact refine        */
    int32_t  inplace_appends;  /* ivfadc_append calls since creation that were written in place on the device (no re-layout) */
    int32_t  last_striped;     /* the last list-major launch: 0 = reference-order f32 tables in every lane; 1 = the four-wave kernel with
                                * bank-striped tables + rotated-order filter sums; 2 / 3 = the eight-wave kernel (wg8scan.hip.h:
                                * m = 8, dsub = 4 / 8 / 12 / 16, K <= 64; m = 16, dsub = 4 / 8, K <= 64 through table modes 6 / 7 only),
                                * four / eight queries per code stream; 4 / 5 = its wide-pool
                                * form (m = 8, 64 < K <= 128; table modes 8 / 9), four / eight queries per code stream -- also what a rank
                                * of the list-partitioned mode reports (ivfadc_set_list_partition); 6 / 7 = the table-free scan of a
                                * 16-bit handle (ivfadc_set_u16_tables), register selectors (K <= 64) / LDS selectors (64 < K); the
                                * table forms of a 16-bit handle report 0; 8 = the masked scan of ivfadc_search_masked
                                * (masked_scan_kernel, csrc/maskset.hip.h) */
    int32_t  coarse_listed;    /* 1: the last batch's coarse filter wrote per-tile records (four smallest keys of every
                                * (query, 64-centroid tile)) instead of the score matrix, and the top-w enumerated them */
    int64_t  pruned_points;    /* points of probed lists that were NOT scanned: the list's coarse distance already lay above
                                * the K-th best key (ivfadc_set_pruning).  scanned_points counts every probed list, as
                                * SURVEY.md 8(d) defines B_alg; scanned_points - pruned_points were actually read        */
    int64_t  lb_survivors;     /* points whose 8-bit lower-bound sum passed the filter of the matrix-core table rounds and got
                                * their reference-order sum from the f32 codebook (ivfadc_set_table_mode)  */
    int32_t  last_lb;          /* 1: the last query-major launch built its ADC tables on the matrix cores (lower bounds) */
    int32_t  last_rider;       /* 1: the last query-major scan launch also carried the exact coarse tiles of a hinted next batch
                                * (ivfadc_set_next_queries) */
    double   lb_build_ms;      /* profiling level 2 only: sum of the durations of the table build run ALONE (an extra launch per batch
                                * of the same build code over the same probes; results are unaffected)                      */
    int64_t  lb_build_launches;
    int32_t  coarse_prefetched; /* 1: the last search found its coarse distances already computed (by the riders of the search before it) */
    int32_t  last_nf;          /* 1: the last list-major launch was the narrow-field kernel (4-bit integer filter, eight queries per code
                                * stream, no resident f32 tables: nfscan.hip.h); lb_survivors then counts the (point, query) pairs that got
                                * their reference-order sum from the f32 codebook */
    int32_t  last_twolevel;    /* 1: the last batch's coarse stage was the certified two-level search (ivfadc_set_coarse_mode) */
    int32_t  twolevel_groups;  /* groups the centroids are in when that search is in use (0: it is not) */
    int64_t  coarse_visited;   /* two-level search: exact centroid distances computed (of queries x kc an exhaustive search computes) */
    float    twolevel_probe_fraction;   /* the self-probe's visited fraction when the grouping was built (-1: not built) */
    int32_t  coarse_f16;       /* 1: the last batch's matrix-core coarse filter used ONE f16 product per score (round 5) instead of the
                                * three-product bf16 split (ivfadc_set_coarse_mode(h, 8) asks for the split) */
} ivfadc_stats;

/* on: 0 off, 1 events around the coarse and scan kernels, 2 = 1 + the matrix-core table build timed alone (lb_build_ms) */
int ivfadc_set_profiling(ivfadc_t *h, int on);
int ivfadc_reset_stats(ivfadc_t *h);
int ivfadc_get_stats(ivfadc_t *h, ivfadc_stats *out);

/* Tuning knobs (0 = automatic).  qg: -1 forces the query-major scan kernel (one workgroup per
 * query), 1 / 2 / 4 force the list-major kernel with that many queries per code stream, 8 the narrow-field list-major kernel (eight
 * queries per code stream; m = 8, dsub = 16, ksub = 256, K <= 64 -- other shapes fall back to 4), -2 forces the generic
 * dump-and-sort path (an independent second implementation, used as a cross-check in the tests), -3 the query-major
 * kernel behind the stand-alone top-w selection whatever the batch size (what large batches take: tests);
 * chunk_points: points per list-major work item.  Results never depend on these.            */
int ivfadc_set_tuning(ivfadc_t *h, int qg, int chunk_points);

/* Coarse search implementation: 0 = automatic (matrix-core score filter + certified exact refine when w <= 48,
 * kc >= 2048 and d % 4 == 0 -- split-bf16 MFMA when the problem fills the chip with 128 x 128 tiles, f32 MFMA below
 * that; the 3-op VALU kernel otherwise), 1 = always the exact VALU kernel, 2 = the filter from kc >= 128 on (tests),
 * 3 = as 0 with the f32 MFMA filter only (A/B runs), 4 = as 0 but the split-bf16 filter always writes the whole score
 * matrix (no per-tile records: A/B runs and tests), 5 = as 0, and the small-batch path (at most 64 queries, nq x w <= 512, K and
 * w <= 64: ONE launch, a workgroup per (query, probe, chunk), last-arriver merge) also searches a coarse quantizer of at most 2048
 * cells inside that launch instead of running the exact coarse kernel first (measured slower: the default keeps the separate
 * kernel).  8 = as 0 with the three-product bf16 split in the large matrix-core filter instead of the one-product f16 form (A/B runs,
 * tests; the f16 form -- scaled f16 operands, 2^-11 relative score error, queries that leave the f16 range flagged and recomputed
 * exactly -- is the default where the bf16 kernel ran before).
 * 6 / 7 = the CERTIFIED TWO-LEVEL coarse search always / never (w <= 64, d % 4 == 0).  What the reference reaches for when the
 * quantizer is large is an HNSW graph (coarsequantizers.jl:58-92: approximate); this is the exact counterpart: the centroids are grouped
 * once (k-means over the centroids, kc / 64 groups, a radius per group), a query visits the groups in ascending order of the lower bound
 * max(0, ||q - g|| - r_g)^2 on its members' distances, computes the members' distances in the reference's order and stops at the first
 * group whose bound exceeds the w-th best distance found.  In automatic mode (0) the grouping is built on the first search of a
 * quantizer with kc >= 4096 and kept only if a self-probe (centroids as queries) computes at most 2 % of the kc distances (a visited
 * centroid is read once per query, not once per query tile: the break-even) -- a quantizer trained on clustered data: 0.1 %, three and a
 * half times faster than the matrix-core filter at kc = 65 536; N(0,1) centroids in high dimension: all of them, so the exhaustive kernels stay
 * (stats: last_twolevel, coarse_visited, twolevel_probe_fraction).  Results are identical in every mode (whatever a filter or a bound
 * lets through is recomputed in the reference's order, and what a bound skips cannot be in the result, ties included).              */
int ivfadc_set_coarse_mode(ivfadc_t *h, int mode);

/* Probe pruning in the query-major scan (default on): a point's ADC sum starts from its list's coarse distance and every
 * table entry is >= 0 (index.jl:242-244), so once the K-th best key found so far lies below the coarse distance of the next
 * probe -- probes come in ascending coarse distance (coarsequantizers.jl:35-36) -- no later list can contribute and the
 * query ends.  Exact: ids and distances are those of the full scan.  0 = scan every probed list.             */
int ivfadc_set_pruning(ivfadc_t *h, int on);

/* Hint: the search AFTER the next one on this handle (ivfadc_search_device / ivfadc_search_device_allgather) will search the nq
 * queries at d_queries (device memory, already holding them now and unchanged until that search has run).  A query-major scan launch
 * leaves CUs idle while its last workgroups finish; with the hint, the search made right after this call also computes the hinted
 * batch's exact coarse distances (coarsequantizers.jl:34, the same kernel code, tile by tile) behind its own scan in the same grid,
 * and the hinted search then starts at its top-w selection.
 *   token   the caller's generation number of the buffer's CONTENTS (any value != 0 that the caller changes whenever it refills the
 *           buffer).  The rows are picked up only by the very next search, only if that search's pointer and count equal the hint's,
 *           AND only if the caller declared the same token for it with ivfadc_set_query_token: a staging buffer that was refilled after
 *           the hint carries another token and its search computes its own rows.  Without a declared token (the default) no search
 *           ever picks prefetched rows up.
 * One hint serves one search; a search on other queries, on any other path (small batch, generic, sub-batched), a plan without the
 * rider form, or no further search simply leaves the rows unused.  Results are unchanged bit for bit (stats: last_rider,
 * coarse_prefetched).  nq = 0, d_queries = NULL or token = 0 withdraws the hint.
 * ivfadc_search_batches (below) drives both calls for host-resident batches, which is how the Julia shim reaches this path. */
int ivfadc_set_next_queries(ivfadc_t *h, int64_t nq, const float *d_queries, uint64_t token);
/* Declares the generation of the queries the NEXT search on this handle reads (see above); consumed by that search. */
int ivfadc_set_query_token(ivfadc_t *h, uint64_t token);

/* ADC tables: 0 = automatic -- list-major scan: bank-striped tables with rotated-order sums (m = 16) or 16-bit integer tables
 * (m = 8) as a filter where those forms exist (four queries per code stream), or 4-bit narrow-field tables with eight
 * queries per code stream and no resident f32 tables (m = 8, dsub = 16: nfscan.hip.h); query-major scan: 8-bit lower-bound
 * tables built on the matrix cores where that pays (m = 48, K <= 64, w <= 32: DESIGN.md 4.4).  1 = the reference's f32 tables and
 * sum order in every lane (round-1 kernels; A/B runs and an independent cross-check in the tests).  2 = as 0, and the matrix-core
 * rounds for every shape they are instantiated for (also m = 16 / dsub = 6, where they are slower than the exact tables:
 * measurement and tests).  3 / 4 = as 0 / 2 with the matrix-core tables built from the three-product bf16 split of rounds 3-4 instead
 * of ONE f16 product per entry (round 5: power-of-two-scaled f16 operands, half the codeword bytes; the bound is looser by up to half a
 * table unit per entry, which the survivors' exact sums absorb).  5 / 6 = as 0 with the eight-wave list-major kernel (wg8scan.hip.h:
 * m = 8, ksub = 256, K <= 64, dsub = 4 / 8 / 12 / 16, i.e. d = 32 / 64 / 96 / 128; with or without a list partition) never / wherever
 * it is instantiated; 7 = as 6 with its eight-query form (wg8_scan_kernel<8> and <8, DS>, same file).  8 / 9 = as 6 / 7, and for
 * 64 < K <= 128 the kernel's wide-pool form (wg8_wide_scan_kernel<NQ, DS>: two pool entries per lane) instead of the four-wave kernel with
 * LDS selectors; K <= 64 and K > 128 run what 6 / 7 run.  Modes 6 / 7 (and 8 / 9 at K <= 64) also take the kernel for m = 16 with
 * d = 128 or d = 64 (wg8_m16_scan_kernel<NQ, DS>: PQ16; K <= 64, lists below 2^27 points), which no other mode does: the default plan of
 * an m = 16 index is the four-wave kernel, as before.  Mode 0 takes that kernel on its own
 * for d = 128 without a list partition, on lists of 8192 points or more; the other widths and the list-partitioned
 * mode get it through 6 / 7, K up to 128 through 8 / 9 (stats.last_striped tells which kernel ran).  10 = as 0, and on a 16-bit handle
 * (ivfadc_create_u16) the scan kernel also serves 64 < K wherever its LDS need fits a CU (u16_wide_scan_kernel: K <= 1984 at small
 * m x dsub, see "Code width" above; stats.last_qg >= 1 and stats.last_scan_lds tell that it ran) instead of the generic path; on an 8-bit
 * handle 10 plans exactly what 0 plans.  Results are identical in every mode: whatever a filter lets through is recomputed in the reference's
 * order -- from the f32 tables or, in the matrix-core rounds, from the f32 codebook -- before it meets the bound.       */
int ivfadc_set_table_mode(ivfadc_t *h, int mode);

/* ADC tables of a 16-bit handle: 0 (default) = per-pass tables of all ksub codewords (u16_scan_kernel / u16_wide_scan_kernel);
 * 1 = table-free wherever it is served; 2 = table-free where the rule below expects it to win.  An 8-bit handle accepts the call and
 * plans what it planned before.  Results are identical in every mode.
 * Table-free (u16_direct_scan_kernel, K <= 64; u16_direct_wide_scan_kernel, 64 < K under ivfadc_set_table_mode(h, 10)): every point
 * gathers the codeword its code names and forms that one entry itself, in the entry's own accumulator and order (the same bits), so the
 * cost follows the points probed (len x d per pair and list), not the codebook (ksub x d per pair and pass of 1024 points).
 * Rule of mode 2: table-free iff min(n / kc, 1024) x U16_DIRECT_COST <= ksub (u16scan.hip.h; measured: DESIGN.md 4.7a).
 * stats.last_striped == 6 / 7 tells that it ran.  NULL handle or a mode outside 0 ... 2: IVFADC_ERR_INVALID, before any device call.
 * ivfadc_clone_view copies the setting; a view takes its own afterwards.  Not an environment variable.                     */
int ivfadc_set_u16_tables(ivfadc_t *h, int mode);

/* Test hook of the matrix-core table build: the 8-bit lower-bound table of ONE (query, cell) pair, built by
 * the code path the search uses (src/index.jl:232-236 is what it bounds).  out_table: m x 256 bytes (slot = code label);
 * out_consts: 3 + 2 m floats -- scale inv, sum of bases, sum of norms, base[m], ||residual_ii||^2[m].  The contract the tests
 * check: base[ii] + q / inv <= (reference entry)(1 + (dsub + 2) 2^-24) for every entry, and <= base[ii] + (q + 1) / inv + 2^-13.4 N
 * from above.  IVFADC_ERR_STATE when the handle's shape has no such kernels.                                  */
int ivfadc_debug_lb_table(ivfadc_t *h, const float *query, int cell, uint8_t *out_table, float *out_consts);

/* Upper bound of the per-batch device workspace (default 8 GiB).  Larger batches are processed in
 * sub-batches of queries; results never depend on it.                                               */
int ivfadc_set_workspace_limit(ivfadc_t *h, uint64_t bytes);

void ivfadc_destroy(ivfadc_t *h);

const char *ivfadc_last_error(void);

#ifdef __cplusplus
}
#endif
#endif /* IVFADC_HIP_H */
