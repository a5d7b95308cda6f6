"""Host-side mirror of the reference's public surface for the knn_search hot path.

Same names, argument meaning and error behaviour as /root/reference/src:
  IVFADCIndex(data; kc, k, m, ...)        index.jl:103-165
  knn_search(ivfadc, point|points, k; w)  index.jl:204-273
  push!/pushfirst!                        utils.jl:114-145   (push / pushfirst here)
  pop!/popfirst!/delete_from_index!       utils.jl:29-105    (host bookkeeping only)
  length / size / show                    index.jl:56-77

Layout note: Julia matrices are d x n column-major; the same memory is an (n, d)
row-major numpy array, which is what every function here takes (one vector per row).
All arithmetic of the search and of the push! encoding runs in the HIP library behind
the C ABI (include/ivfadc_hip.h); nothing here computes a distance.
"""
import ctypes as C
import math
import threading

import numpy as np

from . import _native as nat
from . import trainer

DEFAULT_COARSE_K = 2                     # defaults.jl:2-10
DEFAULT_QUANTIZATION_K = 256
DEFAULT_QUANTIZATION_M = 1
DEFAULT_QUANTIZATION_METHOD = "pq"
DEFAULT_COARSE_DISTANCE = "SqEuclidean"
DEFAULT_COARSE_QUANTIZER = "naive"
DEFAULT_QUANTIZATION_DISTANCE = "SqEuclidean"
DEFAULT_COARSE_MAXITER = 25
DEFAULT_QUANTIZATION_MAXITER = 25

_TYPE_TO_BITS = {np.dtype(np.uint8): 8, np.dtype(np.uint16): 16, np.dtype(np.uint32): 32}
_JULIA_NAMES = {np.dtype(np.uint8): "UInt8", np.dtype(np.uint16): "UInt16", np.dtype(np.uint32): "UInt32"}


class NaiveQuantizer:
    """coarsequantizers.jl:18-20: brute-force coarse quantizer; vectors is (kc, d)."""

    def __init__(self, vectors):
        self.vectors = vectors

    def __repr__(self):
        kc, d = self.vectors.shape
        return "NaiveQuantizer{SqEuclidean,Float32}, %d×%d cluster centres" % (d, kc)


class CodeBook:
    """QuantizedArrays.CodeBook(codes, vectors): vectors is (ksub, dsub) (== dsub x ksub column-major)."""

    def __init__(self, codes, vectors):
        self.codes = codes
        self.vectors = vectors


class ResidualQuantizer:
    def __init__(self, codebooks, k, dims):
        self.codebooks = codebooks
        self.k = k
        self.dims = dims


class InvertedList:
    """index.jl:8-11: idxs (0-based ids) and codes ((len, m) uint8 or uint16) of one Voronoi cell."""

    def __init__(self, idxs, codes):
        self.idxs = idxs
        self.codes = codes

    def __repr__(self):
        return "InvertedList{%s,%s}, %d vectors" % (_JULIA_NAMES[self.idxs.dtype], _JULIA_NAMES[self.codes.dtype], len(self.idxs))


class IVFADCIndex:
    def __init__(self, data, kc=DEFAULT_COARSE_K, k=DEFAULT_QUANTIZATION_K, m=DEFAULT_QUANTIZATION_M,
                 coarse_quantizer=DEFAULT_COARSE_QUANTIZER, coarse_distance=DEFAULT_COARSE_DISTANCE,
                 quantization_distance=DEFAULT_QUANTIZATION_DISTANCE, quantization_method=DEFAULT_QUANTIZATION_METHOD,
                 coarse_maxiter=DEFAULT_COARSE_MAXITER, quantization_maxiter=DEFAULT_QUANTIZATION_MAXITER,
                 index_type=np.uint32, seed=0, device=0):
        data = np.ascontiguousarray(data, np.float32)
        assert data.ndim == 2, "data must be a matrix (one vector per row)"
        nvectors, nrows = data.shape
        index_type = np.dtype(index_type)
        assert index_type in _TYPE_TO_BITS, "index_type must be uint8, uint16 or uint32"
        bits_required = int(math.ceil(math.log2(nvectors))) if nvectors > 1 else 0
        # index.jl:118-125
        assert kc >= 2, "Number of coarse clusters has to be >= 2"
        assert k <= nvectors, "Number of quantization levels  has to be <= %d" % nvectors
        assert 1 <= m <= nrows, "Number of codebooks has to be between 1 and %d" % nrows
        assert coarse_quantizer in ("naive", "hnsw"), "Coarse quantizer can be :naive or :hnsw only"
        assert coarse_maxiter > 0, "Number of clustering iterations has to be > 0"
        assert quantization_maxiter > 0, "Number of clustering iterations has to be > 0"
        assert _TYPE_TO_BITS[index_type] >= bits_required, \
            "%d vectors require at least %d index bits" % (nvectors, bits_required)
        # :hnsw (coarsequantizers.jl:58-92) asks for an APPROXIMATE search of the coarse centroids through a graph; here the
        # centroids are searched exhaustively on the GPU, which is what that graph approximates -- the request is
        # accepted and answered with the naive quantizer's (exact) cells.  A caller who has such a graph (or any other
        # coarse quantizer) searches with ITS cells through knn_search_preassigned
        self.requested_coarse_quantizer = coarse_quantizer
        if coarse_distance != "SqEuclidean" or quantization_distance != "SqEuclidean" or quantization_method != "pq":
            raise NotImplementedError("the HIP path implements SqEuclidean / :pq only (the reference defaults)")
        if nrows % m != 0:
            raise NotImplementedError("d % m != 0: QuantizedArrays.rowrange for ragged sub-spaces is unverifiable")
        if k > 65536:
            raise NotImplementedError("k > 65536 does not fit UInt16 codes")
        cent, cbs, labels = trainer.train_ivfadc_hip(data, kc, k, m, coarse_maxiter, quantization_maxiter, seed, device)
        self._init_native(cent, cbs, labels, index_type, device)
        if nvectors:
            self._append(data, np.arange(nvectors, dtype=np.uint32))

    # ---- construction from existing arrays (loaded index, tests) ------------------------------
    @classmethod
    def from_arrays(cls, centroids, codebooks, labels, offsets=None, codes=None, ids=None,
                    index_type=np.uint32, device=0):
        self = cls.__new__(cls)
        self._init_native(centroids, codebooks, labels, np.dtype(index_type), device)
        if offsets is not None:
            self.set_lists(offsets, codes, ids)
        return self

    @classmethod
    def from_file(cls, filename, device=0):
        """An index saved by IVFADC.jl (or by save_ivfadc_index) -- native reader, ivfadc_load_index."""
        self = cls.__new__(cls)
        h = C.c_void_p()
        bits = C.c_int(0)
        nat.check(nat.lib().ivfadc_load_index(C.byref(h), int(device), str(filename).encode(), C.byref(bits)))
        self._h = h
        self.index_type = np.dtype({8: np.uint8, 16: np.uint16, 32: np.uint32}[bits.value])
        cbits = C.c_int(0)
        nat.check(nat.lib().ivfadc_code_bits(h, C.byref(cbits)))
        self.code_type = np.dtype(np.uint16 if cbits.value == 16 else np.uint8)
        self.device = device
        # quantizer arrays for the reference-shaped views (host copies of what the native reader uploaded)
        dims = [C.c_int32(0) for _ in range(4)]
        nat.check(nat.lib().ivfadc_get_dims(h, *[C.byref(x) for x in dims]))
        d, kc, m, ksub = (int(x.value) for x in dims)
        self._centroids = np.zeros((kc, d), np.float32)
        self._codebooks = np.zeros((m, ksub, d // m), np.float32)
        self._labels = np.zeros((m, ksub), self.code_type)
        get_quantizers, labels = self._entry("get_quantizers", self._labels)
        nat.check(get_quantizers(h, nat.ptr(self._centroids, C.c_float), nat.ptr(self._codebooks, C.c_float), labels))
        self.kc, self.d = self._centroids.shape
        self.m, self.ksub, self.dsub = self._codebooks.shape
        self._mirror = None
        # an :opq index carries a rotation: searched as it is (knn_search never reads rot, index.jl:204-258); push! would need it
        rotated = C.c_int(0)
        nat.check(nat.lib().ivfadc_get_rotation(h, C.byref(rotated), None))
        self.rotated = bool(rotated.value)
        return self

    def rotation(self):
        """The residual quantizer's rotation matrix (d, d), column by column as persistency.jl:62-64 stores it (identity for :pq)."""
        out = np.zeros((self.d, self.d), np.float32)
        nat.check(nat.lib().ivfadc_get_rotation(self._h, None, out.ctypes.data_as(C.POINTER(C.c_float))))
        return out

    def _entry(self, name, codes=None):
        """The native entry `name` for this index's code width -- ivfadc_<name> for UInt8 codes, ivfadc_<name>_u16 for UInt16 -- and
        the array `codes` (codes or labels of the index's code type) as that entry takes it."""
        wide = self.code_type == np.uint16
        fn = getattr(nat.lib(), "ivfadc_" + name + ("_u16" if wide else ""))
        if codes is None:
            return fn, None
        return fn, (codes.ctypes.data_as(C.c_void_p) if wide else nat.ptr(codes, C.c_uint8))

    def _init_native(self, centroids, codebooks, labels, index_type, device):
        self._centroids = np.ascontiguousarray(centroids, np.float32)
        self._codebooks = np.ascontiguousarray(codebooks, np.float32)
        self.kc, self.d = self._centroids.shape
        self.m, self.ksub, self.dsub = self._codebooks.shape
        # U (the code type): UInt16 for uint16 labels or more than 256 codewords per sub-quantizer, UInt8 otherwise
        labels = np.asarray(labels)
        self.code_type = np.dtype(np.uint16 if (labels.dtype == np.uint16 or self.ksub > 256) else np.uint8)
        self._labels = np.ascontiguousarray(labels, self.code_type)
        assert self.m * self.dsub == self.d and self._labels.shape == (self.m, self.ksub)
        self.index_type = np.dtype(index_type)
        self._h = C.c_void_p()
        create, labels = self._entry("create", self._labels)
        nat.check(create(C.byref(self._h), int(device), self.d, self.kc, self.m, self.ksub, nat.ptr(self._centroids, C.c_float),
                         nat.ptr(self._codebooks, C.c_float), labels))
        self._mirror = None

    def clone_view(self):
        """A read-only view of this index (ivfadc_clone_view): the same device arrays, a stream and a workspace of its own, so that
        two batches can be in flight on one replica.  Any change to this index afterwards makes the view refuse to search."""
        h = C.c_void_p()
        nat.check(nat.lib().ivfadc_clone_view(self._h, C.byref(h)))
        return self._view(h)

    def _view(self, h):
        """The Python object of a view handle `h` of this index (plain or subset): the quantizer arrays and the shape are this index's."""
        v = IVFADCIndex.__new__(IVFADCIndex)
        v._h = h
        for name in ("_centroids", "_codebooks", "_labels", "kc", "d", "m", "ksub", "dsub", "index_type", "code_type"):
            setattr(v, name, getattr(self, name))
        v.device = getattr(self, "device", 0)
        v.requested_coarse_quantizer = getattr(self, "requested_coarse_quantizer", "naive")
        v._mirror = None
        v._view_of = self          # keeps the index alive as long as the view
        return v

    def subset(self, ids=None, mask=None):
        """A read-only SUBSET view of this index (ivfadc_clone_subset): the entries whose stored id is selected, in their stored order
        and with their stored ids, compacted on the device into lists of the view's own; quantizers, stream and workspace as for
        clone_view.  `ids`: an integer array of 0-based stored ids (the ones knn_search returns); `mask`: a boolean array indexed by
        id (ids at or above its length are not selected).  Exactly one of the two.  knn_search, coarse_search, knn_search_preassigned
        and knn_search_batches take the view as they take any index; any change to this index afterwards makes it refuse to search."""
        bits, nbits = pack_bitmap(ids=ids, mask=mask)
        return self._subset(nat.lib().ivfadc_clone_subset, nat.ptr(bits, C.c_uint32) if nbits else None, nbits)

    def subset_device(self, d_bits_ptr, nbits):
        """subset() from a bitmap that already lies in device memory of this index's GPU (ivfadc_clone_subset_device): `d_bits_ptr` is
        the raw device pointer (int) of ceil(nbits / 32) uint32 words, complete when the call is made."""
        return self._subset(nat.lib().ivfadc_clone_subset_device, C.c_void_p(int(d_bits_ptr)) if nbits else None, int(nbits))

    def _subset(self, entry, bits, nbits):
        h = C.c_void_p()
        kept = C.c_int64(0)
        nat.check(entry(self._h, bits, C.c_uint64(nbits), C.byref(h), C.byref(kept)))
        v = self._view(h)
        v._subset_n = int(kept.value)       # what out_n said; len() asks the handle
        return v

    # ---- per-query filtered search: mask sets (ivfadc_maskset_create, ivfadc_search_masked) ------------------------------------
    def maskset(self, masks=None, ids=None):
        """A MaskSet of this index (ivfadc_maskset_create): one bitmap over stored ids per entry of `masks` (boolean arrays indexed
        by id) or of `ids` (integer arrays of 0-based stored ids), exactly one of the two, each packed by pack_bitmap; nbits is the
        longest of them.  Made from the index itself (not from a view); any change to the index afterwards makes searches with it
        refuse.  search_masked_raw / knn_search_masked give every query one of the masks, or -1 for none."""
        assert (masks is None) != (ids is None), "maskset takes exactly one of masks and ids"
        src = masks if masks is not None else ids
        assert len(src) >= 1, "a mask set holds at least one mask"
        packed = [pack_bitmap(mask=np.asarray(x)) if masks is not None else pack_bitmap(ids=x) for x in src]
        nbits = max(nb for _, nb in packed)
        stride = (nbits + 31) // 32
        bits = np.zeros((len(packed), stride), np.uint32)
        for r, (words, _) in enumerate(packed):
            bits[r, :words.shape[0]] = words
        return self._maskset(nat.lib().ivfadc_maskset_create, nat.ptr(bits, C.c_uint32) if nbits else None, len(packed), nbits)

    def maskset_device(self, d_bits_ptr, nmasks, nbits):
        """maskset() from bitmaps that already lie in device memory of this index's GPU (ivfadc_maskset_create_device): `d_bits_ptr`
        is the raw device pointer (int) of nmasks rows of ceil(nbits / 32) uint32 words, complete when the call is made."""
        return self._maskset(nat.lib().ivfadc_maskset_create_device, C.c_void_p(int(d_bits_ptr)) if nbits else None, int(nmasks), int(nbits))

    def _maskset(self, entry, bits, nmasks, nbits):
        s = C.c_void_p()
        kept = np.zeros(max(nmasks, 1), np.int64)
        nat.check(entry(self._h, int(nmasks), bits, C.c_uint64(nbits), C.byref(s), nat.ptr(kept, C.c_int64)))
        return MaskSet(s, nmasks, kept[:nmasks], self)

    def search_masked_raw(self, queries, k, maskset, mask_of_query=None, w=1):
        """search_raw with a mask per query (ivfadc_search_masked): mask_of_query (nq,) int32 in [-1, len(maskset)), -1 = no filter;
        None = every query uses mask 0."""
        q = np.ascontiguousarray(queries, np.float32)
        assert q.ndim == 2 and q.shape[1] == self.d, "queries must be (nq, %d)" % self.d
        nq = q.shape[0]
        moq = None
        if mask_of_query is not None:
            moq = np.ascontiguousarray(mask_of_query, np.int32)
            assert moq.shape == (nq,), "mask_of_query must be (nq,)"
        ka = max(int(k), 1)
        ids = np.zeros((nq, ka), np.uint32)
        dists = np.full((nq, ka), np.inf, np.float32)
        counts = np.zeros(nq, np.int32)
        nat.check(nat.lib().ivfadc_search_masked(self._h, maskset._s, nq, nat.ptr(q, C.c_float), int(k), int(w), nat.ptr(moq, C.c_int32),
                                                 nat.ptr(ids, C.c_uint32), nat.ptr(dists, C.c_float), nat.ptr(counts, C.c_int32)))
        return ids, dists, counts

    def search_device_masked(self, maskset, nq, q_ptr, k, w, mask_of_query_ptr, ids_ptr, dists_ptr, counts_ptr):
        """Asynchronous masked search on raw device pointers (ints); see ivfadc_search_device_masked: mask_of_query_ptr may be 0
        (every query uses mask 0); out-of-range mask numbers are clamped."""
        nat.check(nat.lib().ivfadc_search_device_masked(self._h, maskset._s, int(nq), C.c_void_p(q_ptr), int(k), int(w),
                                                        C.c_void_p(mask_of_query_ptr) if mask_of_query_ptr else None, C.c_void_p(ids_ptr),
                                                        C.c_void_p(dists_ptr), C.c_void_p(counts_ptr)))

    def __del__(self):
        h = getattr(self, "_h", None)
        if h is not None and h.value:
            try:
                nat.lib().ivfadc_destroy(h)
            except Exception:
                pass
            self._h = C.c_void_p()

    # ---- lists -------------------------------------------------------------------------------
    def set_lists(self, offsets, codes, ids):
        offsets = np.ascontiguousarray(offsets, np.int64)
        n = int(offsets[-1])
        ids = np.ascontiguousarray(ids, np.uint32)
        codes = np.ascontiguousarray(codes, self.code_type).reshape(n, self.m)
        set_lists, codes_p = self._entry("set_lists", codes)
        nat.check(set_lists(self._h, nat.ptr(offsets, C.c_int64), codes_p, nat.ptr(ids, C.c_uint32)))
        self._mirror = None

    def synth_lists(self, offsets, seed):
        offsets = np.ascontiguousarray(offsets, np.int64)
        nat.check(nat.lib().ivfadc_synth_lists(self._h, nat.ptr(offsets, C.c_int64), C.c_uint64(int(seed))))
        self._mirror = None

    def _lists(self):
        if self._mirror is None:
            n = len(self)
            offsets = np.zeros(self.kc + 1, np.int64)
            codes = np.zeros((n, self.m), self.code_type)
            ids = np.zeros(n, np.uint32)
            get_lists, codes_p = self._entry("get_lists", codes)
            nat.check(get_lists(self._h, nat.ptr(offsets, C.c_int64), codes_p, nat.ptr(ids, C.c_uint32)))
            self._mirror = (offsets, codes, ids)
        return self._mirror

    def _append(self, pts, ids):
        pts = np.ascontiguousarray(pts, np.float32)
        ids = np.ascontiguousarray(ids, np.uint32)
        append, _ = self._entry("append")
        nat.check(append(self._h, pts.shape[0], nat.ptr(pts, C.c_float), nat.ptr(ids, C.c_uint32), None, None))
        self._mirror = None

    def _delete_ids(self, ids):
        """delete_from_index! on 0-based ids (ivfadc_delete_ids: in place on the device); returns how many went."""
        ids = np.ascontiguousarray(ids, np.uint32)
        removed = C.c_int64(0)
        nat.check(nat.lib().ivfadc_delete_ids(self._h, ids.shape[0], nat.ptr(ids, C.c_uint32), C.byref(removed)))
        self._mirror = None
        return int(removed.value)

    def _shift_ids(self, delta):
        nat.check(nat.lib().ivfadc_shift_ids(self._h, int(delta)))
        self._mirror = None

    def encode(self, pts):
        """_encode_point for a batch: (list (n,) int32 0-based, codes (n, m) of the index's code type)."""
        pts = np.ascontiguousarray(pts, np.float32)
        if pts.ndim == 1:
            pts = pts[None, :]
        assert pts.shape[1] == self.d
        lst = np.zeros(pts.shape[0], np.int32)
        codes = np.zeros((pts.shape[0], self.m), self.code_type)
        encode, codes_p = self._entry("encode", codes)
        nat.check(encode(self._h, pts.shape[0], nat.ptr(pts, C.c_float), nat.ptr(lst, C.c_int32), codes_p))
        return lst, codes

    # ---- reference-shaped views ----------------------------------------------------------------
    @property
    def coarse_quantizer(self):
        return NaiveQuantizer(self._centroids)

    @property
    def residual_quantizer(self):
        cbs = [CodeBook(self._labels[i], self._codebooks[i]) for i in range(self.m)]
        return ResidualQuantizer(cbs, self.ksub, (self.d, len(self)))

    @property
    def inverse_index(self):
        offsets, codes, ids = self._lists()
        return [InvertedList(ids[offsets[l]:offsets[l + 1]].astype(self.index_type),
                             codes[offsets[l]:offsets[l + 1]]) for l in range(self.kc)]

    def __len__(self):                                   # index.jl:56
        n = C.c_int64(0)
        nat.check(nat.lib().ivfadc_ntotal(self._h, C.byref(n), None))
        return int(n.value)

    @property
    def size(self):                                      # index.jl:65
        return (self.d, len(self))

    def list_sizes(self):
        n = C.c_int64(0)
        sizes = np.zeros(self.kc, np.int64)
        nat.check(nat.lib().ivfadc_ntotal(self._h, C.byref(n), nat.ptr(sizes, C.c_int64)))
        return sizes

    def __repr__(self):                                  # index.jl:69-77
        idxsize = self.index_type.itemsize
        # an index built with coarse_quantizer=:hnsw says so: the request is served by the exhaustive (exact) search of the
        # centroids, which is what the graph of coarsequantizers.jl:58-92 approximates
        req = getattr(self, "requested_coarse_quantizer", "naive")
        cq = "naive" if req == "naive" else "%s (requested; served by the exact naive search)" % req
        csize = getattr(self, "code_type", np.dtype(np.uint8)).itemsize
        what = "IVFADCIndex" if getattr(self, "_subset_n", None) is None else "Subset view of an IVFADCIndex"
        return ("%s, %s coarse quantizer, %d-byte encoding (%d + %d×%d), %d Float32 vectors"
                % (what, cq, csize * self.m + idxsize, idxsize, csize, self.m, len(self)))

    # ---- search --------------------------------------------------------------------------------
    def _io_lock(self):
        """The lock that goes with the page-locked blocks of _io: they belong to the index, ctypes releases the GIL during the native
        call, and a second Python thread calling knn_search on the same index would repack (or free and regrow) the query block the
        first call's kernels are reading.  Held from the packing to the last read of the result blocks."""
        lk = self.__dict__.get("_pin_lock")
        if lk is None:
            lk = self.__dict__.setdefault("_pin_lock", threading.Lock())
        return lk

    def _io(self, nq, ka):
        """Page-locked query / result arrays of this index (ivfadc_host_alloc; grown on demand) -- what the Julia shim keeps per
        index: knn_search packs the caller's vectors straight into the query block and reads ids / distances / counts out of the
        result blocks, so the library stages nothing (include/ivfadc_hip.h: ivfadc_host_alloc).  Call with _io_lock() held."""
        pin = getattr(self, "_pin", None)
        if pin is None or pin[0].a.size < nq * self.d or pin[1].a.size < nq * ka or pin[3].a.size < nq:
            grow = lambda old, need: max(need + need // 2, old)
            o = [0, 0, 0] if pin is None else [pin[0].a.size, pin[1].a.size, pin[3].a.size]
            self._pin = None                      # (frees the old blocks first)
            pin = (nat.PinnedArray(grow(o[0], nq * self.d), np.float32), nat.PinnedArray(grow(o[1], nq * ka), np.uint32),
                   nat.PinnedArray(grow(o[1], nq * ka), np.float32), nat.PinnedArray(grow(o[2], nq), np.int32))
            self._pin = pin
        return (pin[0].a[:nq * self.d].reshape(nq, self.d), pin[1].a[:nq * ka].reshape(nq, ka), pin[2].a[:nq * ka].reshape(nq, ka),
                pin[3].a[:nq])

    def search_raw(self, queries, k, w=1):
        """(nq, d) -> ids (nq, k) uint32, dists (nq, k) float32, counts (nq,) int32 via ivfadc_search."""
        q = np.ascontiguousarray(queries, np.float32)
        assert q.ndim == 2 and q.shape[1] == self.d, "queries must be (nq, %d)" % self.d
        nq = q.shape[0]
        ka = max(int(k), 1)
        ids = np.zeros((nq, ka), np.uint32)
        dists = np.full((nq, ka), np.inf, np.float32)
        counts = np.zeros(nq, np.int32)
        nat.check(nat.lib().ivfadc_search(self._h, nq, nat.ptr(q, C.c_float), int(k), int(w), nat.ptr(ids, C.c_uint32),
                                          nat.ptr(dists, C.c_float), nat.ptr(counts, C.c_int32)))
        return ids, dists, counts

    # ---- range search (no reference counterpart: knn_search cut at the radius, include/ivfadc_hip.h "RANGE search") ------------
    def range_search_raw(self, queries, radii, w=1, max_total=0):
        """(nq, d) queries and (nq,) radii (squared distances) -> lims (nq + 1,) int64, ids (total,) uint32, dists (total,) float32 via
        ivfadc_range_search: query q's entries are [lims[q], lims[q + 1]), in knn_search's order, every one with dist <= radii[q].
        max_total > 0 caps the total (IVFADCError with the needed total otherwise); 0: no cap."""
        q = np.ascontiguousarray(queries, np.float32)
        assert q.ndim == 2 and q.shape[1] == self.d, "queries must be (nq, %d)" % self.d
        r = np.ascontiguousarray(radii, np.float32).reshape(-1)
        assert r.shape[0] == q.shape[0], "one radius per query"
        L = nat.lib()
        res = C.c_void_p()
        nat.check(L.ivfadc_range_search(self._h, q.shape[0], nat.ptr(q, C.c_float), nat.ptr(r, C.c_float), int(w), int(max_total),
                                        C.byref(res)))
        try:
            nq, total = C.c_int64(), C.c_int64()
            nat.check(L.ivfadc_range_result_sizes(res, C.byref(nq), C.byref(total)))
            lims = np.zeros(nq.value + 1, np.int64)
            ids = np.zeros(total.value, np.uint32)
            dists = np.zeros(total.value, np.float32)
            nat.check(L.ivfadc_range_result_copy(res, nat.ptr(lims, C.c_int64), nat.ptr(ids, C.c_uint32), nat.ptr(dists, C.c_float)))
        finally:
            L.ivfadc_range_result_destroy(res)
        return lims, ids, dists

    def range_search_device(self, nq, q_ptr, radii_ptr, w=1, max_total=0):
        """ivfadc_range_search_device on device pointers: returns the result HANDLE (a c_void_p the caller frees with
        range_result_destroy; range_result_sizes / _copy / _device read it)."""
        res = C.c_void_p()
        nat.check(nat.lib().ivfadc_range_search_device(self._h, int(nq), C.c_void_p(q_ptr), C.c_void_p(radii_ptr), int(w), int(max_total),
                                                       C.byref(res)))
        return res

    def range_search_masked_raw(self, queries, radii, maskset=None, mask_of_query=None, w=1, max_total=0):
        """range_search_raw with a mask per query (ivfadc_range_search_masked): mask_of_query (nq,) int32 in [-1, len(maskset)), -1 = no
        filter; None with a set = every query uses mask 0.  maskset=None: no query is filtered (mask_of_query must then be None) -- the
        way to a range search on an index with UInt16 codes.  Returns (lims, ids, dists) as range_search_raw does."""
        q = np.ascontiguousarray(queries, np.float32)
        assert q.ndim == 2 and q.shape[1] == self.d, "queries must be (nq, %d)" % self.d
        r = np.ascontiguousarray(radii, np.float32).reshape(-1)
        assert r.shape[0] == q.shape[0], "one radius per query"
        moq = None
        if mask_of_query is not None:
            moq = np.ascontiguousarray(mask_of_query, np.int32)
            assert moq.shape == (q.shape[0],), "mask_of_query must be (nq,)"
        L = nat.lib()
        res = C.c_void_p()
        nat.check(L.ivfadc_range_search_masked(self._h, maskset._s if maskset is not None else None, q.shape[0], nat.ptr(q, C.c_float),
                                               nat.ptr(r, C.c_float), int(w), int(max_total), nat.ptr(moq, C.c_int32), C.byref(res)))
        try:
            return range_result_copy(res)
        finally:
            L.ivfadc_range_result_destroy(res)

    def range_search_device_masked(self, nq, q_ptr, radii_ptr, maskset=None, mask_of_query_ptr=0, w=1, max_total=0):
        """ivfadc_range_search_device_masked on device pointers (ints): returns the result HANDLE, as range_search_device does.
        mask_of_query_ptr may be 0 (with a set: every query uses mask 0); out-of-range mask numbers are clamped."""
        res = C.c_void_p()
        nat.check(nat.lib().ivfadc_range_search_device_masked(self._h, maskset._s if maskset is not None else None, int(nq), C.c_void_p(q_ptr),
                                                              C.c_void_p(radii_ptr), int(w), int(max_total),
                                                              C.c_void_p(mask_of_query_ptr) if mask_of_query_ptr else None, C.byref(res)))
        return res

    # ---- the seam of knn_search: coarse_search on one side, everything that reads its two vectors on the other ------------
    def coarse_search_raw(self, queries, w):
        """coarse_search(cq, point, w) (coarsequantizers.jl:33-37) for a batch: (nq, d) -> lists (nq, w) int32 (0-based cells,
        ascending distance, ties to the lower cell), dists (nq, w) float32, via ivfadc_coarse_search.  1 <= w <= kc."""
        q = np.ascontiguousarray(queries, np.float32)
        assert q.ndim == 2 and q.shape[1] == self.d, "queries must be (nq, %d)" % self.d
        nq, wa = q.shape[0], max(int(w), 1)
        lists = np.zeros((nq, wa), np.int32)
        dists = np.zeros((nq, wa), np.float32)
        nat.check(nat.lib().ivfadc_coarse_search(self._h, nq, nat.ptr(q, C.c_float), int(w), nat.ptr(lists, C.c_int32),
                                                 nat.ptr(dists, C.c_float)))
        return lists, dists

    def search_preassigned_raw(self, queries, k, lists, dists):
        """index.jl:220-257 given the output of ANY coarse_search: row q of lists / dists (nq, w) = the probes of query q in visit
        order (0-based cells, pairwise distinct; distances finite and >= +0).  Returns (ids, dists, counts) as search_raw does,
        via ivfadc_search_preassigned, which validates the probes on the host before anything is launched."""
        q = np.ascontiguousarray(queries, np.float32)
        assert q.ndim == 2 and q.shape[1] == self.d, "queries must be (nq, %d)" % self.d
        nq = q.shape[0]
        pl = np.ascontiguousarray(lists, np.int32)
        pd = np.ascontiguousarray(dists, np.float32)
        assert pl.ndim == 2 and pl.shape[0] == nq and pd.shape == pl.shape, "lists and dists must both be (nq, w)"
        ka = max(int(k), 1)
        ids = np.zeros((nq, ka), np.uint32)
        out = np.full((nq, ka), np.inf, np.float32)
        counts = np.zeros(nq, np.int32)
        nat.check(nat.lib().ivfadc_search_preassigned(self._h, nq, nat.ptr(q, C.c_float), int(k), int(pl.shape[1]), nat.ptr(pl, C.c_int32),
                                                      nat.ptr(pd, C.c_float), nat.ptr(ids, C.c_uint32), nat.ptr(out, C.c_float),
                                                      nat.ptr(counts, C.c_int32)))
        return ids, out, counts

    def coarse_search_device(self, nq, q_ptr, w, lists_ptr, dists_ptr):
        """Asynchronous coarse search on raw device pointers (ints); see ivfadc_coarse_search_device."""
        nat.check(nat.lib().ivfadc_coarse_search_device(self._h, int(nq), C.c_void_p(q_ptr), int(w), C.c_void_p(lists_ptr),
                                                        C.c_void_p(dists_ptr)))

    def search_device_preassigned(self, nq, q_ptr, k, w, lists_ptr, cdists_ptr, ids_ptr, dists_ptr, counts_ptr):
        """Asynchronous search with supplied probes on raw device pointers (ints); see ivfadc_search_device_preassigned: the
        preconditions on the probes are the caller's here."""
        nat.check(nat.lib().ivfadc_search_device_preassigned(self._h, int(nq), C.c_void_p(q_ptr), int(k), int(w), C.c_void_p(lists_ptr),
                                                             C.c_void_p(cdists_ptr), C.c_void_p(ids_ptr), C.c_void_p(dists_ptr),
                                                             C.c_void_p(counts_ptr)))

    # ---- measurement / tuning -------------------------------------------------------------------
    def set_profiling(self, on):
        """0 / False: off; 1 / True: HIP events around the coarse and scan kernels; 2: also the matrix-core table build alone."""
        nat.check(nat.lib().ivfadc_set_profiling(self._h, int(on)))

    def reset_stats(self):
        nat.check(nat.lib().ivfadc_reset_stats(self._h))

    def get_stats(self):
        st = nat.Stats()
        nat.check(nat.lib().ivfadc_get_stats(self._h, C.byref(st)))
        return {f: getattr(st, f) for f, _ in nat.Stats._fields_}

    def set_tuning(self, qg=0, chunk_points=0):
        nat.check(nat.lib().ivfadc_set_tuning(self._h, int(qg), int(chunk_points)))

    def set_coarse_mode(self, mode):
        """0: automatic (matrix-core score filter + certified exact refine for kc >= 2048; per-tile records instead of a score
        matrix where the stand-alone top-w reads them), 1: always the exact VALU kernel, 2: the filter from kc >= 128 on,
        3: f32 MFMA filter only, 4: as 0 but always with the full score matrix.  Results are identical in every mode."""
        nat.check(nat.lib().ivfadc_set_coarse_mode(self._h, int(mode)))

    def set_pruning(self, on):
        """Exact probe pruning of the query-major scan (default on): a list whose coarse distance exceeds the K-th best key
        so far cannot contribute (every ADC sum starts from it and only grows)."""
        nat.check(nat.lib().ivfadc_set_pruning(self._h, int(bool(on))))

    def set_next_queries(self, nq, d_queries_ptr, token):
        """Hint for the search made right after this call: the search after THAT one will be on the `nq` queries at device pointer
        `d_queries_ptr` (already there, unchanged until searched) -- their exact coarse distances are then computed behind the
        first search's scan launch (ivfadc_set_next_queries).  `token` (!= 0) is the caller's generation number of the buffer's
        contents: the hinted search picks the rows up only if it declares the same token (set_query_token).  Results are unchanged."""
        nat.check(nat.lib().ivfadc_set_next_queries(self._h, int(nq), C.c_void_p(d_queries_ptr) if d_queries_ptr else None,
                                                    C.c_uint64(int(token))))

    def set_query_token(self, token):
        """Declares the generation of the queries the NEXT search reads (ivfadc_set_query_token); consumed by that search."""
        nat.check(nat.lib().ivfadc_set_query_token(self._h, C.c_uint64(int(token))))

    def search_batches_raw(self, batches, k, w=1):
        """A run of consecutive batches (list of (nq_b, d) arrays) in ONE call (ivfadc_search_batches): batch b is searched with
        batch b + 1 named as its successor.  Returns per batch (ids, dists, counts) as search_raw does."""
        qs = [np.asarray(b, np.float32).reshape(-1, self.d) for b in batches]
        sizes = np.array([q.shape[0] for q in qs], np.int64)
        total = int(sizes.sum())
        ka = max(int(k), 1)
        # packed once, into the index's page-locked blocks (see _io); the results are copied out of them before they are reused
        with self._io_lock():
            allq, ids, dists, counts = self._io(total, ka)
            s = 0
            for q in qs:
                allq[s:s + q.shape[0]] = q
                s += q.shape[0]
            nat.check(nat.lib().ivfadc_search_batches(self._h, len(qs), nat.ptr(sizes, C.c_int64), nat.ptr(allq, C.c_float), int(k), int(w),
                                                      nat.ptr(ids, C.c_uint32), nat.ptr(dists, C.c_float), nat.ptr(counts, C.c_int32)))
            out, s = [], 0
            for n in sizes.tolist():
                out.append((ids[s:s + n].copy(), dists[s:s + n].copy(), counts[s:s + n].copy()))
                s += n
        return out

    def set_table_mode(self, mode):
        """0: automatic (filter tables where they exist and pay), 1: the reference's f32 tables in every lane, 2: as 0 plus the
        matrix-core lower-bound rounds for every shape they are instantiated for; 3 / 4: as 0 / 2 with those tables built from the
        three-product bf16 split instead of one f16 product per entry; 5 / 6: as 0 with the eight-wave list-major kernel never /
        wherever it is instantiated -- m = 8, ksub = 256, K <= 64, d = 32 / 64 / 96 / 128 (dsub = 4 / 8 / 12 / 16), with or without a list
        partition (set_list_partition); 7: as 6 with its eight-query form; 8 / 9: as 6 / 7, and for 64 < K <= 128 the kernel's wide-pool
        form (two pool entries per lane) instead of the four-wave kernel -- K <= 64 and K > 128 run what 6 / 7 run.  6 / 7 (8 / 9 at K <= 64)
        also take the kernel for m = 16 at d = 128 or 64 (PQ16; K <= 64), which no other mode does.  Mode 0 takes that
        kernel unasked for d = 128 without a list partition on lists of 8192 points or more; get_stats()["last_striped"] is 2 / 3 when
        its four- / eight-query form ran, 4 / 5 for the wide-pool form.  10: as 0, and an index with UInt16 codes runs 64 < K on its scan
        kernel's LDS-selector form (K <= 1984 at small m x dsub; get_stats()["last_qg"] >= 1) instead of the generic path (last_qg == -2).
        Results are the same bytes in every mode."""
        nat.check(nat.lib().ivfadc_set_table_mode(self._h, int(mode)))

    def set_u16_tables(self, mode):
        """ADC tables of an index with UInt16 codes.  0 (default): per-pass tables of all ksub codewords; 1: table-free wherever it is
        served -- every point's sums come straight from the codeword its code names, so the cost follows the lists probed, not the
        codebook size (K <= 64, and 64 < K under set_table_mode(10)); 2: table-free where min(n / kc, 1024) * U16_DIRECT_COST <= ksub.
        get_stats()["last_striped"] is 6 / 7 when the table-free scan ran (register / LDS selectors).  An index with UInt8 codes
        accepts the call and plans what it planned before.  Results are the same bytes in every mode."""
        nat.check(nat.lib().ivfadc_set_u16_tables(self._h, int(mode)))

    def debug_lb_table(self, query, cell):
        """Test hook: the 8-bit lower-bound ADC table of one (query, cell) pair as the matrix-core build makes it.
        Returns (table uint8 [m, 256], inv, sbase, nn, base [m], r2 [m])."""
        q = np.ascontiguousarray(query, np.float32)
        tab = np.zeros((self.m, 256), np.uint8)
        cf = np.zeros(3 + 2 * self.m, np.float32)
        nat.check(nat.lib().ivfadc_debug_lb_table(self._h, q.ctypes.data_as(C.POINTER(C.c_float)), int(cell),
                                                  tab.ctypes.data_as(C.POINTER(C.c_uint8)), cf.ctypes.data_as(C.POINTER(C.c_float))))
        return tab, float(cf[0]), float(cf[1]), float(cf[2]), cf[3:3 + self.m].copy(), cf[3 + self.m:].copy()

    def set_workspace_limit(self, nbytes):
        nat.check(nat.lib().ivfadc_set_workspace_limit(self._h, C.c_uint64(int(nbytes))))

    def sync(self):
        nat.check(nat.lib().ivfadc_sync(self._h))

    def set_stream(self, hip_stream):
        """Use a caller-owned hipStream_t (int handle), e.g. torch.cuda.current_stream().cuda_stream."""
        nat.check(nat.lib().ivfadc_set_stream(self._h, C.c_void_p(int(hip_stream))))

    def search_device(self, nq, q_ptr, k, w, ids_ptr, dists_ptr, counts_ptr):
        """Asynchronous search on raw device pointers (ints); see ivfadc_search_device."""
        nat.check(nat.lib().ivfadc_search_device(self._h, int(nq), C.c_void_p(q_ptr), int(k), int(w), C.c_void_p(ids_ptr),
                                                 C.c_void_p(dists_ptr), C.c_void_p(counts_ptr)))

    # ---- what is stored under an id (ivfadc_locate / ivfadc_reconstruct: on the device copy of the lists, no host mirror) ----
    def locate_raw(self, ids):
        """ids (n,) -> (lists (n,) int32, positions (n,) int64), 0-based; -1 / -1 for an id no list holds."""
        ids = np.ascontiguousarray(ids, np.uint32).reshape(-1)
        n = ids.shape[0]
        lists = np.full(n, -1, np.int32)
        pos = np.full(n, -1, np.int64)
        nat.check(nat.lib().ivfadc_locate(self._h, n, nat.ptr(ids, C.c_uint32), nat.ptr(lists, C.c_int32), nat.ptr(pos, C.c_int64)))
        return lists, pos

    def reconstruct_raw(self, ids):
        """ids (n,) -> (vectors (n, d) float32, found (n,) bool): centre + codewords of each stored point; an absent id gives +0.0."""
        ids = np.ascontiguousarray(ids, np.uint32).reshape(-1)
        n = ids.shape[0]
        vec = np.zeros((n, self.d), np.float32)
        found = np.zeros(n, np.uint8)
        nat.check(nat.lib().ivfadc_reconstruct(self._h, n, nat.ptr(ids, C.c_uint32), nat.ptr(vec, C.c_float), nat.ptr(found, C.c_uint8)))
        return vec, found.astype(bool)

    def locate_device(self, n, ids_ptr, lists_ptr, pos_ptr):
        """Asynchronous on raw device pointers (ints): n uint32 ids -> n int32 lists, n int64 positions; see ivfadc_locate_device."""
        nat.check(nat.lib().ivfadc_locate_device(self._h, int(n), C.c_void_p(ids_ptr), C.c_void_p(lists_ptr), C.c_void_p(pos_ptr)))

    def reconstruct_device(self, n, ids_ptr, vectors_ptr, found_ptr=None):
        """Asynchronous on raw device pointers (ints): n uint32 ids -> n x d float32 (and n found bytes unless found_ptr is None);
        see ivfadc_reconstruct_device."""
        nat.check(nat.lib().ivfadc_reconstruct_device(self._h, int(n), C.c_void_p(ids_ptr), C.c_void_p(vectors_ptr),
                                                      C.c_void_p(found_ptr) if found_ptr else None))

    # ---- the distance knn_search would report for given ids (ivfadc_score_ids: locate, then one lane per pair; no scan) ----
    def score_raw(self, queries, ids, counts=None):
        """queries (nq, d), ids (nq, C) -- or (C,): ONE shared row scored against every query -- and optional counts (nq,) of live slots
        per query -> (dists (nq, C) float32, found (nq, C) bool): the distance ivfadc_search reports for each id, bit for bit; +Inf /
        False for an id no list holds and for a slot at or behind counts[q]."""
        q = np.ascontiguousarray(queries, np.float32)
        assert q.ndim == 2 and q.shape[1] == self.d, "queries must be (nq, %d)" % self.d
        nq = q.shape[0]
        ids = np.ascontiguousarray(ids, np.uint32)
        assert ids.ndim in (1, 2), "ids must be (nq, C), or (C,) for one shared row"
        shared = ids.ndim == 1
        assert shared or ids.shape[0] == nq, "ids must hold one row per query"
        ncand = ids.shape[-1]
        if counts is not None:
            counts = np.ascontiguousarray(counts, np.int32).reshape(-1)
            assert counts.shape[0] == nq, "counts must hold one number per query"
        dists = np.full((nq, ncand), np.inf, np.float32)
        found = np.zeros((nq, ncand), np.uint8)
        nat.check(nat.lib().ivfadc_score_ids(self._h, nq, nat.ptr(q, C.c_float), ncand, 0 if shared else ncand, nat.ptr(ids, C.c_uint32),
                                             nat.ptr(counts, C.c_int32), nat.ptr(dists, C.c_float), nat.ptr(found, C.c_uint8)))
        return dists, found.astype(bool)

    def score_device(self, nq, q_ptr, ncand, ids_stride, ids_ptr, counts_ptr, dists_ptr, found_ptr=None):
        """Asynchronous on raw device pointers (ints): nq x d float32 queries, ids rows of ncand uint32 at ids_stride (ncand, or 0 for
        one shared row), optional nq int32 counts -> nq x ncand float32 distances (and found bytes unless found_ptr is None); see
        ivfadc_score_ids_device."""
        nat.check(nat.lib().ivfadc_score_ids_device(self._h, int(nq), C.c_void_p(q_ptr), int(ncand), int(ids_stride), C.c_void_p(ids_ptr),
                                                    C.c_void_p(counts_ptr) if counts_ptr else None, C.c_void_p(dists_ptr),
                                                    C.c_void_p(found_ptr) if found_ptr else None))


def _comm_methods():
    """one-process-per-GPU merge inside the library (ivfadc_comm_*): methods of IVFADCIndex"""
    def comm_init(self, nranks, rank, id128):
        buf = np.ascontiguousarray(id128, np.uint8)
        assert buf.shape == (128,)
        nat.check(nat.lib().ivfadc_comm_init(self._h, int(nranks), int(rank), nat.ptr(buf, C.c_uint8)))

    def search_device_allgather_on(self, searcher, nq, q_ptr, k, w, block_ptr, gathered_ptr, slot):
        """search on `searcher` (this index or a view of it), the collective on this index's communicator"""
        nat.check(nat.lib().ivfadc_search_device_allgather_on(self._h, searcher._h, int(nq), C.c_void_p(q_ptr), int(k), int(w),
                                                             C.c_void_p(block_ptr), C.c_void_p(gathered_ptr), int(slot)))

    def search_device_allgather(self, nq, q_ptr, k, w, block_ptr, gathered_ptr, slot):
        nat.check(nat.lib().ivfadc_search_device_allgather(self._h, int(nq), C.c_void_p(q_ptr), int(k), int(w), C.c_void_p(block_ptr),
                                                          C.c_void_p(gathered_ptr), int(slot)))

    def comm_wait(self):
        n = C.c_int64(0)
        nat.check(nat.lib().ivfadc_comm_wait(self._h, C.byref(n)))
        return int(n.value)

    def set_list_partition(self, nparts, part):
        """List-partitioned multi-GPU mode (ivfadc_set_list_partition): this handle scans the probed lists l with l % nparts == part."""
        nat.check(nat.lib().ivfadc_set_list_partition(self._h, int(nparts), int(part)))

    def search_device_partial(self, nq, q_ptr, k, w, keys_ptr, counts_ptr):
        nat.check(nat.lib().ivfadc_search_device_partial(self._h, int(nq), C.c_void_p(q_ptr), int(k), int(w), C.c_void_p(keys_ptr), C.c_void_p(counts_ptr)))

    def merge_partials_device(self, nq, k, nparts, keys_all_ptr, counts_all_ptr, ids_ptr, dists_ptr, counts_ptr):
        nat.check(nat.lib().ivfadc_merge_partials_device(self._h, int(nq), int(k), int(nparts), C.c_void_p(keys_all_ptr), C.c_void_p(counts_all_ptr),
                                                         C.c_void_p(ids_ptr), C.c_void_p(dists_ptr), C.c_void_p(counts_ptr)))

    def search_device_listpart(self, nq, q_ptr, k, w, block_ptr, gathered_ptr, ids_ptr, dists_ptr, counts_ptr):
        nat.check(nat.lib().ivfadc_search_device_listpart(self._h, int(nq), C.c_void_p(q_ptr), int(k), int(w), C.c_void_p(block_ptr),
                                                          C.c_void_p(gathered_ptr), C.c_void_p(ids_ptr), C.c_void_p(dists_ptr), C.c_void_p(counts_ptr)))

    def comm_destroy(self):
        nat.check(nat.lib().ivfadc_comm_destroy(self._h))

    IVFADCIndex.comm_destroy = comm_destroy
    IVFADCIndex.set_list_partition = set_list_partition
    IVFADCIndex.search_device_partial = search_device_partial
    IVFADCIndex.merge_partials_device = merge_partials_device
    IVFADCIndex.search_device_listpart = search_device_listpart
    IVFADCIndex.comm_init = comm_init
    IVFADCIndex.search_device_allgather = search_device_allgather
    IVFADCIndex.search_device_allgather_on = search_device_allgather_on
    IVFADCIndex.comm_wait = comm_wait


_comm_methods()


def comm_unique_id():
    """128-byte RCCL id for IVFADCIndex.comm_init (call on rank 0, hand to every rank)."""
    buf = np.zeros(128, np.uint8)
    nat.check(nat.lib().ivfadc_comm_unique_id(nat.ptr(buf, C.c_uint8)))
    return buf


class MaskSet:
    """nmasks bitmaps over the stored ids of one index, on the device in list order (ivfadc_maskset_t; IVFADCIndex.maskset).  Immutable;
    len() is the number of masks, `kept` the entries each selects.  Keeps its index alive; the native object goes with this one."""

    def __init__(self, s, nmasks, kept, index):
        self._s, self._n, self._kept, self._index = s, int(nmasks), np.asarray(kept, np.int64).copy(), index

    @property
    def kept(self):
        return self._kept.copy()

    def __len__(self):
        return self._n

    def __del__(self):
        s = getattr(self, "_s", None)
        if s is not None and s.value:
            try:
                nat.lib().ivfadc_maskset_destroy(s)
            except Exception:
                pass
            self._s = C.c_void_p()


def pack_bitmap(ids=None, mask=None):
    """The bitmap ivfadc_clone_subset takes, from a list of 0-based stored ids or from a boolean mask indexed by id: (uint32 words,
    nbits) with id i at bit (i & 31) of word i >> 5.  nbits is len(mask), or the largest id + 1."""
    assert (ids is None) != (mask is None), "subset takes exactly one of ids and mask"
    if mask is not None:
        mask = np.asarray(mask)
        assert mask.dtype == np.bool_ and mask.ndim == 1, "mask must be a 1-D boolean array indexed by id"
    else:
        ids = np.asarray(ids)
        assert ids.ndim == 1 and (ids.size == 0 or np.issubdtype(ids.dtype, np.integer)), "ids must be a 1-D integer array"
        ids = ids.astype(np.int64)
        assert ids.size == 0 or (ids.min() >= 0 and ids.max() < 2 ** 32), "ids are 0-based UInt32 values"
        mask = np.zeros(int(ids.max()) + 1 if ids.size else 0, np.bool_)
        mask[ids] = True
    nbits = int(mask.shape[0])
    assert nbits <= 2 ** 32, "ids are UInt32 values: at most 2^32 bits"
    by = np.packbits(mask, bitorder="little")                      # bit (i & 7) of byte i >> 3
    words = np.zeros((nbits + 31) // 32 * 4, np.uint8)
    words[:by.shape[0]] = by
    return np.ascontiguousarray(words.view("<u4")).astype(np.uint32), nbits


def knn_search(ivfadc, points, k, w=1):
    """knn_search(ivfadc, point, k; w=1) / knn_search(ivfadc, points, k; w=1)  (index.jl:204-273).

    A 1-D `points` is one query and returns (ids[I], dists[float32]), at most k long, ascending.
    A 2-D array or a list of vectors returns (list of ids arrays, list of dists arrays)."""
    assert k >= 1, "Number of neighbors must be k >= 1"                          # index.jl:210
    assert w >= 1, "Number of clusters to search in must be w >= 1"             # index.jl:211
    single = isinstance(points, np.ndarray) and points.ndim == 1
    if not single and not isinstance(points, np.ndarray):
        points = np.stack([np.asarray(p, np.float32) for p in points]) if len(points) else np.zeros((0, ivfadc.d), np.float32)
        single = points.ndim == 1
    pts = np.asarray(points)
    if single:
        pts = pts[None, :]
    assert pts.ndim == 2 and pts.shape[1] == ivfadc.d, "queries must be (nq, %d)" % ivfadc.d
    nq = pts.shape[0]
    # the vectors are packed ONCE, straight into page-locked memory the kernels read, and the results are read out of page-locked
    # memory the final kernel wrote: the reference's host-arrays-in / host-arrays-out contract with no staging copy in the library
    # (the blocks are the index's: one Python thread at a time packs, searches and reads them out -- see _io_lock)
    with ivfadc._io_lock():
        q, ids, dists, counts = ivfadc._io(nq, int(k))
        q[...] = pts
        if nq:
            nat.check(nat.lib().ivfadc_search(ivfadc._h, nq, nat.ptr(q, C.c_float), int(k), int(w), nat.ptr(ids, C.c_uint32),
                                              nat.ptr(dists, C.c_float), nat.ptr(counts, C.c_int32)))
        out_i = [ids[i, :counts[i]].astype(ivfadc.index_type) for i in range(nq)]
        out_d = [dists[i, :counts[i]].copy() for i in range(nq)]
    if single:
        return out_i[0], out_d[0]
    return out_i, out_d


def _as_points(ivfadc, points):
    """(matrix (nq, d), single) of a vector, a matrix or a list of vectors, as knn_search takes them"""
    single = isinstance(points, np.ndarray) and points.ndim == 1
    if not single and not isinstance(points, np.ndarray):
        points = np.stack([np.asarray(p, np.float32) for p in points]) if len(points) else np.zeros((0, ivfadc.d), np.float32)
        single = points.ndim == 1
    pts = np.asarray(points, np.float32)
    if single:
        pts = pts[None, :]
    assert pts.ndim == 2 and pts.shape[1] == ivfadc.d, "queries must be (nq, %d)" % ivfadc.d
    return pts, single


def coarse_search(ivfadc, points, w):
    """coarse_search(cq, point, w) (coarsequantizers.jl:33-37) on the index's coarse quantizer: (closest_clusters, coarse_distances),
    the w closest cells in ascending distance, ties to the lower cell.  Cells are 0-based, as in `encode`.  A 1-D `points` is one
    query and returns two (w,) arrays; a matrix or a list of vectors returns (nq, w) arrays."""
    assert w >= 1, "Number of clusters to search in must be w >= 1"             # index.jl:211
    pts, single = _as_points(ivfadc, points)
    lists, dists = ivfadc.coarse_search_raw(pts, w)
    if single:
        return lists[0], dists[0]
    return lists, dists


def knn_search_preassigned(ivfadc, points, k, clusters, distances):
    """knn_search (index.jl:204-258) behind its coarse_search call (index.jl:219): `clusters` / `distances` are what ANY
    coarse_search returned for each query -- 0-based cells in visit order and their distances, (w,) for one query or (nq, w).
    Returns what knn_search returns: (ids, dists) for one query, two lists of arrays otherwise."""
    assert k >= 1, "Number of neighbors must be k >= 1"                          # index.jl:210
    pts, single = _as_points(ivfadc, points)
    cl = np.asarray(clusters, np.int32)
    cd = np.asarray(distances, np.float32)
    if single:
        cl, cd = cl.reshape(1, -1), cd.reshape(1, -1)
    assert cl.ndim == 2 and cl.shape[0] == pts.shape[0] and cd.shape == cl.shape, "clusters and distances must both be (nq, w)"
    assert cl.shape[1] >= 1, "Number of clusters to search in must be w >= 1"   # index.jl:211
    ids, dists, counts = ivfadc.search_preassigned_raw(pts, k, cl, cd)
    out_i = [ids[i, :counts[i]].astype(ivfadc.index_type) for i in range(pts.shape[0])]
    out_d = [dists[i, :counts[i]].copy() for i in range(pts.shape[0])]
    if single:
        return out_i[0], out_d[0]
    return out_i, out_d


def knn_search_masked(ivfadc, points, k, maskset, mask_of_query=None, w=1):
    """knn_search (index.jl:204-258) with a predicate per query: query q sees only the entries whose stored id mask
    mask_of_query[q] of `maskset` (IVFADCIndex.maskset) selects -- the lists after deleteat! (utils.jl:98-99) of every other entry --
    or every entry for -1; None gives every query mask 0.  The probed cells are the unfiltered index's.  Returns what knn_search
    returns: (ids, dists) for one query (mask_of_query may then be a plain integer), two lists of arrays otherwise."""
    assert k >= 1, "Number of neighbors must be k >= 1"                          # index.jl:210
    assert w >= 1, "Number of clusters to search in must be w >= 1"             # index.jl:211
    pts, single = _as_points(ivfadc, points)
    moq = None if mask_of_query is None else np.asarray(mask_of_query, np.int32).reshape(-1)
    ids, dists, counts = ivfadc.search_masked_raw(pts, k, maskset, moq, w)
    out_i = [ids[i, :counts[i]].astype(ivfadc.index_type) for i in range(pts.shape[0])]
    out_d = [dists[i, :counts[i]].copy() for i in range(pts.shape[0])]
    if single:
        return out_i[0], out_d[0]
    return out_i, out_d


def range_result_sizes(res):
    """(nq, total) of a range-search result handle"""
    nq, total = C.c_int64(), C.c_int64()
    nat.check(nat.lib().ivfadc_range_result_sizes(res, C.byref(nq), C.byref(total)))
    return nq.value, total.value


def range_result_copy(res):
    """(lims, ids, dists) host arrays of a range-search result handle"""
    nq, total = range_result_sizes(res)
    lims, ids, dists = np.zeros(nq + 1, np.int64), np.zeros(total, np.uint32), np.zeros(total, np.float32)
    nat.check(nat.lib().ivfadc_range_result_copy(res, nat.ptr(lims, C.c_int64), nat.ptr(ids, C.c_uint32), nat.ptr(dists, C.c_float)))
    return lims, ids, dists


def range_result_device(res):
    """(d_lims, d_ids, d_dists) device addresses of a range-search result handle, valid until it is destroyed"""
    a, b, c = C.c_void_p(), C.c_void_p(), C.c_void_p()
    nat.check(nat.lib().ivfadc_range_result_device(res, C.byref(a), C.byref(b), C.byref(c)))
    return a.value, b.value, c.value


def range_result_destroy(res):
    nat.lib().ivfadc_range_result_destroy(res)


def range_search(ivfadc, points, r, w=1):
    """Every stored point of the w probed lists within distance r of a query: knn_search(ivfadc, point, k; w) (index.jl:204-258) with k at
    least the number of probed points, cut after the last entry with dist <= r.  NO REFERENCE COUNTERPART (IVFADC.jl has knn_search
    only; NearestNeighbors.jl calls this inrange).  r is in the units knn_search returns -- SQUARED Euclidean -- and inclusive; a scalar
    is broadcast over a batch, an array gives one radius per query.  A 1-D `points` is one query and returns (ids[I], dists[float32]),
    ascending; a 2-D array or a list of vectors returns (list of ids arrays, list of dists arrays)."""
    assert w >= 1, "Number of clusters to search in must be w >= 1"             # index.jl:211
    pts, single = _as_points(ivfadc, points)
    rr = np.asarray(r, np.float32)
    assert not np.isnan(rr).any(), "the radius must not be NaN"
    radii = np.ascontiguousarray(np.broadcast_to(rr.reshape(-1) if rr.ndim else rr, (pts.shape[0],)), np.float32)
    lims, ids, dists = ivfadc.range_search_raw(pts, radii, w)
    out_i = [ids[lims[i]:lims[i + 1]].astype(ivfadc.index_type) for i in range(pts.shape[0])]
    out_d = [dists[lims[i]:lims[i + 1]].copy() for i in range(pts.shape[0])]
    if single:
        return out_i[0], out_d[0]
    return out_i, out_d


def range_search_masked(ivfadc, points, r, maskset=None, mask_of_query=None, w=1):
    """range_search with a predicate per query: query q sees only the entries whose stored id mask mask_of_query[q] of `maskset`
    (IVFADCIndex.maskset) selects, or every entry for -1; None with a set gives every query mask 0.  The probed cells are the unfiltered
    index's.  maskset=None filters nothing (mask_of_query must then be None) and serves indexes with UInt16 codes, which range_search
    refuses.  NO REFERENCE COUNTERPART.  Returns what range_search returns (mask_of_query may be a plain integer for one query)."""
    assert w >= 1, "Number of clusters to search in must be w >= 1"             # index.jl:211
    pts, single = _as_points(ivfadc, points)
    rr = np.asarray(r, np.float32)
    assert not np.isnan(rr).any(), "the radius must not be NaN"
    assert maskset is not None or mask_of_query is None, "mask_of_query needs a maskset"
    radii = np.ascontiguousarray(np.broadcast_to(rr.reshape(-1) if rr.ndim else rr, (pts.shape[0],)), np.float32)
    moq = None if mask_of_query is None else np.asarray(mask_of_query, np.int32).reshape(-1)
    lims, ids, dists = ivfadc.range_search_masked_raw(pts, radii, maskset, moq, w)
    out_i = [ids[lims[i]:lims[i + 1]].astype(ivfadc.index_type) for i in range(pts.shape[0])]
    out_d = [dists[lims[i]:lims[i + 1]].copy() for i in range(pts.shape[0])]
    if single:
        return out_i[0], out_d[0]
    return out_i, out_d


def knn_search_batches(ivfadc, batches, k, w=1):
    """[knn_search(ivfadc, points, k; w) for points in batches] (index.jl:261-273 once per batch) as one native call
    (ivfadc_search_batches): the same results, batch by batch."""
    assert k >= 1, "Number of neighbors must be k >= 1"                          # index.jl:210
    assert w >= 1, "Number of clusters to search in must be w >= 1"             # index.jl:211
    out = []
    for ids, dists, counts in ivfadc.search_batches_raw(batches, k, w):
        out.append(([ids[i, :counts[i]].astype(ivfadc.index_type) for i in range(ids.shape[0])],
                    [dists[i, :counts[i]].copy() for i in range(ids.shape[0])]))
    return out


def _push(ivfadc, point, position):
    """utils.jl:127-145."""
    point = np.asarray(point, np.float32)
    nrows, nvectors = ivfadc.size
    assert point.ndim == 1 and nrows == point.shape[0], "Adding to index requires %d-element vectors" % nrows
    assert _TYPE_TO_BITS[ivfadc.index_type] >= math.log2(nvectors + 1), \
        "Cannot index, exceeding index capacity of %d points" % (2 ** _TYPE_TO_BITS[ivfadc.index_type])
    if position == "first":
        ivfadc._shift_ids(1)                                        # _shift_up_inverse_index! (utils.jl:1-6), on the device
        vecid = 0
    else:
        vecid = nvectors
    ivfadc._append(point[None, :], np.array([vecid], np.uint32))
    return None


def push(ivfadc, point):
    """push!(ivfadc, point) (utils.jl:114)."""
    return _push(ivfadc, point, "last")


def pushfirst(ivfadc, point):
    """pushfirst!(ivfadc, point) (utils.jl:123)."""
    return _push(ivfadc, point, "first")


def _decode_point(ivfadc, codes):
    """utils.jl:71-81."""
    out = np.empty(ivfadc.d, np.float32)
    for i in range(ivfadc.m):
        c = int(np.nonzero(ivfadc._labels[i] == codes[i])[0][0])
        out[i * ivfadc.dsub:(i + 1) * ivfadc.dsub] = ivfadc._codebooks[i, c]
    return out


def locate(ivfadc, ids):
    """Where each id is stored: (lists, positions), 0-based, by the rule of _pop!'s loop (utils.jl:49-55: the last list that holds the
    id, the first position within it); -1 / -1 for an id no list holds."""
    return ivfadc.locate_raw(ids)


def reconstruct(ivfadc, ids):
    """The stored points under `ids` as an n x d Float32 array: centre + _decode_point (utils.jl:58-59, 71-81), computed on the device.
    An id no list holds raises AssertionError naming the first such id."""
    ids = np.ascontiguousarray(ids, np.uint32).reshape(-1)
    vec, found = ivfadc.reconstruct_raw(ids)
    if not found.all():
        raise AssertionError("id %d is not stored in the index" % int(ids[int(np.argmin(found))]))
    return vec


def score(ivfadc, points, ids):
    """The distance knn_search(ivfadc, point, k; w) reports between each query and each of the given stored ids, bit for bit, whether or
    not the id's cell would have been probed: dc + the sub-space sums in the reference's order (coarsequantizers.jl:33-34, index.jl:232-246).
    `ids` is (nq, C), one row per query, or (C,), one row scored against every query; an id no list holds gives +Inf.
    A 1-D `points` is one query and returns a (C,) array; a matrix or a list of vectors returns (nq, C)."""
    pts, single = _as_points(ivfadc, points)
    ids = np.ascontiguousarray(ids, np.uint32)
    if single and ids.ndim == 2:
        assert ids.shape[0] == 1, "one query takes one row of ids"
    dists, _ = ivfadc.score_raw(pts, ids)
    return dists[0] if single else dists


def knn_among(ivfadc, points, ids, k):
    """The k best of the given candidate ids per query, by score(): (ids, dists), ordered by (distance, position in the row); ids no
    list holds are dropped, so a row may come back shorter than k.  One query returns two arrays, a batch two lists of arrays."""
    assert k >= 1, "Number of neighbors must be k >= 1"                          # index.jl:210
    pts, single = _as_points(ivfadc, points)
    ids = np.ascontiguousarray(ids, np.uint32)
    dists, found = ivfadc.score_raw(pts, ids)
    out_i, out_d = [], []
    for i in range(pts.shape[0]):
        row = ids if ids.ndim == 1 else ids[i]
        order = np.argsort(dists[i], kind="stable")                              # stable: equal distances keep their row order
        order = order[found[i][order]][:int(k)]
        out_i.append(row[order].astype(ivfadc.index_type))
        out_d.append(dists[i][order].copy())
    if single:
        return out_i[0], out_d[0]
    return out_i, out_d


def _pop(ivfadc, position):
    """utils.jl:41-68: reconstruct on the device, then delete."""
    n = len(ivfadc)
    assert n > 0, "Cannot pop element from empty index"
    vecid, shift = (n - 1, 0) if position == "last" else (0, 1)
    rec = reconstruct(ivfadc, np.array([vecid], np.uint32))[0]
    # deleteat! + _shift_down_inverse_index!(shift): removing id 0 lowers every other id by one, removing the
    # highest id lowers none -- exactly ivfadc_delete_ids' rule, applied in place on the device
    ivfadc._delete_ids(np.array([vecid], np.uint32))
    return rec


def pop(ivfadc):
    """pop!(ivfadc) (utils.jl:29)."""
    return _pop(ivfadc, "last")


def popfirst(ivfadc):
    """popfirst!(ivfadc) (utils.jl:37)."""
    return _pop(ivfadc, "first")


def delete_from_index(ivfadc, points):
    """delete_from_index!(ivfadc, points) (utils.jl:90-105): `points` are 1-based positions.  In place on the
    device (ivfadc_delete_ids); ids that are not stored are ignored, as in the reference."""
    shifted = np.unique(np.asarray(points, np.int64) - 1)
    shifted = shifted[(shifted >= 0) & (shifted < 2 ** 32)]
    ivfadc._delete_ids(shifted.astype(np.uint32))
    return None
