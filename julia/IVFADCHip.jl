# IVFADCHip.jl -- GPU methods for IVFADC.jl's knn_search hot path (libivfadc_hip.so, MI355X / gfx950).
#
# Drop-in: `include("IVFADCHip.jl")` after `using IVFADC` (or add the body as src/hip.jl and include it last in
# src/IVFADC.jl).  It adds MORE SPECIFIC methods of the reference's own generic functions -- knn_search
# (src/index.jl:204-273), push! / pushfirst! (src/utils.jl:114-145), pop! / popfirst! (src/utils.jl:29-68),
# delete_from_index! (src/utils.jl:90-105) -- for the element types the HIP library implements
# (U = UInt8 or UInt16, T = Float32, SqEuclidean for both distances; NaiveQuantizer, or HNSWQuantizer for knn_search: its own
# coarse_search runs on the CPU and the library searches the probes it returns); every other index keeps the CPU methods.
# Every C symbol is declared in include/ivfadc_hip.h, which cites the reference interface it replaces.
#
# The same text is shown in INTEGRATION.md section 3 (tests/test_abi.py checks that the two stay identical and that every
# symbol ccall'ed here is exported by the library).  julia is not part of the build image, so this file is exercised
# only through those checks; the calls themselves are the ones the Python/ctypes tests drive.
module IVFADCHip

using IVFADC
using IVFADC: IVFADCIndex, NaiveQuantizer, HNSWQuantizer, coarse_search
import IVFADC: knn_search, delete_from_index!
import Base: push!, pushfirst!, pop!, popfirst!
using Distances
using QuantizedArrays
import LinearAlgebra

export hip_sync!, hip_release!, hip_subset, hip_locate, hip_reconstruct

# GPU methods for the knn_search hot path; everything else falls through to the CPU methods.
const LIBIVFADC = get(ENV, "IVFADC_HIP_LIB", "libivfadc_hip.so")

# The C ABI this file was written for (include/ivfadc_hip.h: IVFADC_ABI_VERSION).  Checked once, before the first handle is made:
# a library with other prototypes must not be called through these ccall signatures.
const ABI_VERSION = 4
const _abi_checked = Ref(false)
function _check_abi()
    _abi_checked[] && return
    v = ccall((:ivfadc_abi_version, LIBIVFADC), Cint, ())
    v == ABI_VERSION || error("IVFADCHip: $LIBIVFADC has ABI version $v, this shim was written for $ABI_VERSION")
    _abi_checked[] = true
    return
end

# Page-locked pack buffers of a handle (ivfadc_host_alloc).  knn_search takes a Vector of Vectors (index.jl:261-265), so the queries
# must be packed into one d×nq matrix anyway: they are packed straight into memory the GPU reads, and the results are unpacked straight
# out of memory the final kernel wrote -- the library then stages nothing (include/ivfadc_hip.h, "Page-locked host memory").
mutable struct PinnedBlock
    ptr::Ptr{Cvoid}
    bytes::Int
end
PinnedBlock() = PinnedBlock(C_NULL, 0)

function _ensure!(b::PinnedBlock, bytes::Int)
    bytes <= b.bytes && return b.ptr
    b.ptr == C_NULL || _check(ccall((:ivfadc_host_free, LIBIVFADC), Cint, (Ptr{Cvoid},), b.ptr))
    b.ptr = C_NULL; b.bytes = 0
    want = bytes + bytes ÷ 2
    out = Ref{Ptr{Cvoid}}(C_NULL)
    _check(ccall((:ivfadc_host_alloc, LIBIVFADC), Cint, (Csize_t, Ref{Ptr{Cvoid}}), want, out))
    b.ptr = out[]; b.bytes = want
    return b.ptr
end

function _release!(b::PinnedBlock)
    b.ptr == C_NULL || ccall((:ivfadc_host_free, LIBIVFADC), Cint, (Ptr{Cvoid},), b.ptr)
    b.ptr = C_NULL; b.bytes = 0
    return
end

mutable struct HipHandle
    ptr::Ptr{Cvoid}
    q::PinnedBlock        # d×nq Float32
    ids::PinnedBlock      # k×nq UInt32
    dists::PinnedBlock    # k×nq Float32
    counts::PinnedBlock   # nq Int32
end
HipHandle(ptr::Ptr{Cvoid}) = HipHandle(ptr, PinnedBlock(), PinnedBlock(), PinnedBlock(), PinnedBlock())

# views of a handle's pack buffers for a call on nq queries (valid until the next call grows them)
function _io(h::HipHandle, d::Int, k::Int, nq::Int)
    q = unsafe_wrap(Array, Ptr{Float32}(_ensure!(h.q, 4 * d * max(nq, 1))), (d, nq))
    ids = unsafe_wrap(Array, Ptr{UInt32}(_ensure!(h.ids, 4 * k * max(nq, 1))), (k, nq))
    dists = unsafe_wrap(Array, Ptr{Float32}(_ensure!(h.dists, 4 * k * max(nq, 1))), (k, nq))
    counts = unsafe_wrap(Array, Ptr{Int32}(_ensure!(h.counts, 4 * max(nq, 1))), (nq,))
    return q, ids, dists, counts
end

function _check(rc::Cint)
    rc == 0 && return
    msg = unsafe_string(ccall((:ivfadc_last_error, LIBIVFADC), Cstring, ()))
    rc == 1 ? throw(AssertionError(msg)) : error("ivfadc_hip status $rc: $msg")
end

# U = UInt8 codes go through the uint8_t entries, U = UInt16 codes (k up to 65536) through the _u16 entries, whose code and label
# buffers are untyped (Ptr{Cvoid}) in the C ABI and hold UInt16.  (GpuIndex{I} binds the index type I.)
const GpuIndex = IVFADCIndex{U,I,Distances.SqEuclidean,Distances.SqEuclidean,Float32,
                             NaiveQuantizer{Distances.SqEuclidean,Float32}} where {I<:Unsigned, U<:Union{UInt8,UInt16}}
# An index built with coarse_quantizer=:hnsw (coarsequantizers.jl:58-92): its centroids live in cq.hnsw.data and its coarse_search is an
# APPROXIMATE graph search.  knn_search reads only what coarse_search returns (index.jl:219-257), so such an index is served with the
# reference's semantics: coarse_search(cq, point, w) runs here, on the CPU, and ivfadc_search_preassigned does the rest on the probes it
# returned.  Mutators keep the reference's CPU methods and drop the device copy (as on an :opq index).
const HnswIndex = IVFADCIndex{U,I,Distances.SqEuclidean,Distances.SqEuclidean,Float32,
                              <:HNSWQuantizer} where {I<:Unsigned, U<:Union{UInt8,UInt16}}
const AnyGpuIndex = Union{GpuIndex,HnswIndex}
_codetype(::IVFADCIndex{U}) where {U} = U
_centroids(cq::NaiveQuantizer) = cq.vectors                                          # d×kc
_centroids(cq::HNSWQuantizer) = Matrix{Float32}(reduce(hcat, cq.hnsw.data))          # the same matrix, from the graph's points

# IVFADCIndex is an immutable struct (src/index.jl:39): it can carry no finalizer, and a WeakKeyDict would compare its mutable fields by
# CONTENT.  Its inverse_index field is a Vector -- mutable, identity-stable, and exactly as long-lived as the index that holds it -- so
# the registry keys on that object's identity (objectid) and a finalizer on the vector drops the entry: when an index becomes garbage
# its lists do, the entry goes, and the HipHandle's finalizer frees the device replica and the pack buffers.  Code that builds and
# rebuilds indexes therefore leaks nothing; hip_release!(ivfadc) frees a replica at once.
const _handles = Dict{UInt,HipHandle}()
# A finalizer may run at any allocation -- in the middle of get! / pop! on _handles inside hip_sync! / hip_release! -- so it must not
# touch the Dict itself: it only QUEUES the key (a lock-free push onto a vector guarded by a SpinLock that no allocating code holds),
# and the queue is drained, under the registry's lock, at the next hip_sync! / hip_release! (the pattern of the Julia manual's
# "finalizers and locks").  _handles is only ever touched with _registry_lock held.
const _registry_lock = ReentrantLock()
const _dead_lock = Base.Threads.SpinLock()
const _dead_keys = UInt[]
_key(ivfadc::AnyGpuIndex) = objectid(ivfadc.inverse_index)
function _drop_handle(lists)
    k = objectid(lists)
    lock(_dead_lock)
    try
        push!(_dead_keys, k)
    finally
        unlock(_dead_lock)
    end
    return nothing
end
# with _registry_lock held
function _drain_dead!()
    ks = UInt[]
    lock(_dead_lock)
    try
        append!(ks, _dead_keys); empty!(_dead_keys)
    finally
        unlock(_dead_lock)
    end
    for k in ks
        h = pop!(_handles, k, nothing)
        h === nothing || finalize(h)
    end
    return nothing
end

# The residual quantizer of a :pq index carries an identity rotation; :opq carries a real one (QuantizedArrays).  knn_search never reads
# it (src/index.jl:204-258): an :opq index is SEARCHED on the GPU like any other.  quantize_data -- push! / pushfirst! -- does: those
# keep the reference's CPU methods on such an index and drop the device copy, so that the next search uploads the edited lists.
_gpu_ok(ivfadc::GpuIndex) = ivfadc.residual_quantizer.rot == LinearAlgebra.I

"Free the device copy of `ivfadc` now; the next GPU call uploads the Julia lists afresh."
function hip_release!(ivfadc::AnyGpuIndex)
    lock(_registry_lock) do
        _drain_dead!()
        h = pop!(_handles, _key(ivfadc), nothing)
        h === nothing || finalize(h)
    end
    return nothing
end

"Upload (or refresh) the device copy of `ivfadc` from the Julia lists."
function hip_sync!(ivfadc::AnyGpuIndex; device::Int=0)
    cq, rq = ivfadc.coarse_quantizer, ivfadc.residual_quantizer
    cent = _centroids(cq)
    d, kc = size(cent)
    m = length(rq.codebooks); ksub = length(rq.codebooks[1].codes)
    _check_abi()
    h = lock(_registry_lock) do
      _drain_dead!()
      get!(_handles, _key(ivfadc)) do
        cbs = reduce(hcat, [vec(cb.vectors) for cb in rq.codebooks])        # m blocks of dsub×ksub, column-major
        labels = reduce(vcat, [cb.codes for cb in rq.codebooks])            # m×ksub
        out = Ref{Ptr{Cvoid}}(C_NULL)
        if _codetype(ivfadc) === UInt16
            labels16 = Vector{UInt16}(labels)                               # block after block, ksub labels each
            _check(ccall((:ivfadc_create_u16, LIBIVFADC), Cint,
                         (Ref{Ptr{Cvoid}}, Cint, Cint, Cint, Cint, Cint, Ptr{Float32}, Ptr{Float32}, Ptr{Cvoid}),
                         out, device, d, kc, m, ksub, cent, cbs, labels16))
        else
            _check(ccall((:ivfadc_create, LIBIVFADC), Cint,
                         (Ref{Ptr{Cvoid}}, Cint, Cint, Cint, Cint, Cint, Ptr{Float32}, Ptr{Float32}, Ptr{UInt8}),
                         out, device, d, kc, m, ksub, cent, cbs, labels))
        end
        hh = HipHandle(out[])
        finalizer(hh) do x
            x.ptr == C_NULL || ccall((:ivfadc_destroy, LIBIVFADC), Cvoid, (Ptr{Cvoid},), x.ptr)
            x.ptr = C_NULL
            _release!(x.q); _release!(x.ids); _release!(x.dists); _release!(x.counts)
        end
        finalizer(_drop_handle, ivfadc.inverse_index)
        hh
      end
    end
    offsets = Int64[0; cumsum(length(l.idxs) for l in ivfadc.inverse_index)]
    U = _codetype(ivfadc)
    codes = isempty(ivfadc.inverse_index) ? U[] :
            reduce(vcat, (reduce(vcat, l.codes; init=U[]) for l in ivfadc.inverse_index))       # n×m, list order
    ids = UInt32.(reduce(vcat, (l.idxs for l in ivfadc.inverse_index)))                           # 0-based (index.jl:189)
    if U === UInt16
        _check(ccall((:ivfadc_set_lists_u16, LIBIVFADC), Cint, (Ptr{Cvoid}, Ptr{Int64}, Ptr{Cvoid}, Ptr{UInt32}),
                     h.ptr, offsets, codes, ids))
    else
        _check(ccall((:ivfadc_set_lists, LIBIVFADC), Cint, (Ptr{Cvoid}, Ptr{Int64}, Ptr{UInt8}, Ptr{UInt32}),
                     h.ptr, offsets, codes, ids))
    end
    return h
end

function _handle(ivfadc::AnyGpuIndex)
    h = lock(_registry_lock) do
        _drain_dead!()
        get(_handles, _key(ivfadc), nothing)
    end
    return h === nothing ? hip_sync!(ivfadc) : h
end

# ADC tables of a UInt16 index: 0 per-pass tables (default), 1 table-free, 2 table-free where it is expected to win; same results
hip_set_u16_tables!(ivfadc::AnyGpuIndex, mode::Integer) = (_check(ccall((:ivfadc_set_u16_tables, LIBIVFADC), Cint, (Ptr{Cvoid}, Cint), _handle(ivfadc).ptr, mode)); ivfadc)

# Every mutator edits the device copy IN PLACE next to the Julia lists.  Should a device edit fail half way, the handle is dropped, so
# that the next search uploads the Julia lists (the source of truth) afresh: a stale device copy cannot be searched.
function _on_device(f, ivfadc::GpuIndex)
    try
        return f()
    catch
        hip_release!(ivfadc)
        rethrow()
    end
end

# knn_search, batch (index.jl:261-273).  Asserts are raised BEFORE the ccall, as in index.jl:210-211.
function knn_search(ivfadc::GpuIndex{I}, points::Vector{Vector{Float32}}, k::Int; w::Int=1) where {I}
    @assert k >= 1 "Number of neighbors must be k >= 1"
    @assert w >= 1 "Number of clusters to search in must be w >= 1"
    h = _handle(ivfadc)
    nq = length(points)
    nq == 0 && return Vector{I}[], Vector{Float32}[]
    d = size(ivfadc.coarse_quantizer, 1)
    q, ids, dists, counts = _io(h, d, k, nq)
    for i in 1:nq
        @assert length(points[i]) == d "Searching requires $d-element vectors"
        copyto!(q, (i - 1) * d + 1, points[i], 1, d)           # d×nq column-major, packed once, into page-locked memory
    end
    _check(ccall((:ivfadc_search, LIBIVFADC), Cint,
                 (Ptr{Cvoid}, Int64, Ptr{Float32}, Cint, Cint, Ptr{UInt32}, Ptr{Float32}, Ptr{Int32}),
                 h.ptr, nq, q, k, min(w, size(ivfadc.coarse_quantizer, 2)), ids, dists, counts))
    return [I.(ids[1:counts[i], i]) for i in 1:nq], [dists[1:counts[i], i] for i in 1:nq]
end

knn_search(ivfadc::GpuIndex, point::Vector{Float32}, k::Int; w::Int=1) =
    first.(knn_search(ivfadc, [point], k; w=w))

# knn_search on an index with an HNSW coarse quantizer: the reference's own coarse_search (coarsequantizers.jl:73-76) per query, then
# index.jl:220-257 on the device for the probes it returned, in the order it returned them (ivfadc_search_preassigned: cells 0-based,
# pairwise distinct; distances finite and >= +0).  A coarse result that is shorter than w or repeats a cell cannot be expressed as one
# nq×w block: the call then falls back to the CPU method.
function knn_search(ivfadc::HnswIndex{I,U}, points::Vector{Vector{Float32}}, k::Int; w::Int=1) where {I,U}
    @assert k >= 1 "Number of neighbors must be k >= 1"
    @assert w >= 1 "Number of clusters to search in must be w >= 1"
    cpu() = invoke(knn_search, Tuple{IVFADCIndex{U,I,Distances.SqEuclidean,Distances.SqEuclidean,Float32},Vector{Vector{Float32}},Int},
                   ivfadc, points, k; w=w)
    nq = length(points)
    nq == 0 && return Vector{I}[], Vector{Float32}[]
    cq = ivfadc.coarse_quantizer
    d, kc = size(cq)
    wc = min(w, kc)                                                          # index.jl:216
    lists = Matrix{Int32}(undef, wc, nq); cds = Matrix{Float32}(undef, wc, nq)
    for i in 1:nq
        @assert length(points[i]) == d "Searching requires $d-element vectors"
        cl, cd = coarse_search(cq, points[i], wc)
        (length(cl) == wc && length(cd) == wc && allunique(cl) && all(x -> isfinite(x) && !signbit(x), cd)) || return cpu()
        lists[:, i] .= Int32.(cl .- 1)                                       # 0-based
        cds[:, i] .= cd
    end
    h = _handle(ivfadc)
    q, ids, dists, counts = _io(h, d, k, nq)
    for i in 1:nq
        copyto!(q, (i - 1) * d + 1, points[i], 1, d)
    end
    _check(ccall((:ivfadc_search_preassigned, LIBIVFADC), Cint,
                 (Ptr{Cvoid}, Int64, Ptr{Float32}, Cint, Cint, Ptr{Int32}, Ptr{Float32}, Ptr{UInt32}, Ptr{Float32}, Ptr{Int32}),
                 h.ptr, nq, q, k, wc, lists, cds, ids, dists, counts))
    return [I.(ids[1:counts[i], i]) for i in 1:nq], [dists[1:counts[i], i] for i in 1:nq]
end

knn_search(ivfadc::HnswIndex, point::Vector{Float32}, k::Int; w::Int=1) =
    first.(knn_search(ivfadc, [point], k; w=w))

# ... and its mutators: the reference's CPU methods, after which the device copy is dropped, so that the next search uploads the
# edited lists
function push!(ivfadc::HnswIndex, point::Vector{Float32})
    r = invoke(push!, Tuple{IVFADCIndex,Vector{Float32}}, ivfadc, point)
    hip_release!(ivfadc)
    return r
end

function pushfirst!(ivfadc::HnswIndex, point::Vector{Float32})
    r = invoke(pushfirst!, Tuple{IVFADCIndex,Vector{Float32}}, ivfadc, point)
    hip_release!(ivfadc)
    return r
end

function pop!(ivfadc::HnswIndex)
    rec = invoke(pop!, Tuple{IVFADCIndex}, ivfadc)
    hip_release!(ivfadc)
    return rec
end

function popfirst!(ivfadc::HnswIndex)
    rec = invoke(popfirst!, Tuple{IVFADCIndex}, ivfadc)
    hip_release!(ivfadc)
    return rec
end

function delete_from_index!(ivfadc::HnswIndex, points::Vector{<:Integer})
    invoke(delete_from_index!, Tuple{IVFADCIndex,Vector{<:Integer}}, ivfadc, points)
    hip_release!(ivfadc)
    return nothing
end

# A run of consecutive batches: `[knn_search(ivfadc, b, k; w=w) for b in batches]` as ONE native call (ivfadc_search_batches).  Inside,
# every batch is searched with its successor already named (the serving-loop hint, ivfadc_set_next_queries, on buffers the library
# owns), so the successor's coarse search runs behind the batch's scan launch.  Same results, batch by batch.
function knn_search(ivfadc::GpuIndex{I}, batches::Vector{Vector{Vector{Float32}}}, k::Int; w::Int=1) where {I}
    @assert k >= 1 "Number of neighbors must be k >= 1"
    @assert w >= 1 "Number of clusters to search in must be w >= 1"
    h = _handle(ivfadc)
    sizes = Int64[length(b) for b in batches]
    total = sum(sizes)
    total == 0 && return [(Vector{I}[], Vector{Float32}[]) for _ in batches]
    d = size(ivfadc.coarse_quantizer, 1)
    q, ids, dists, counts = _io(h, d, k, total)
    at = 0
    for b in batches, p in b                                                 # d×total, the batches back to back
        @assert length(p) == d "Searching requires $d-element vectors"
        copyto!(q, at * d + 1, p, 1, d)
        at += 1
    end
    _check(ccall((:ivfadc_search_batches, LIBIVFADC), Cint,
                 (Ptr{Cvoid}, Cint, Ptr{Int64}, Ptr{Float32}, Cint, Cint, Ptr{UInt32}, Ptr{Float32}, Ptr{Int32}),
                 h.ptr, length(sizes), sizes, q, k, min(w, size(ivfadc.coarse_quantizer, 2)), ids, dists, counts))
    ends = cumsum(sizes)
    return [([I.(ids[1:counts[i], i]) for i in (e - s + 1):e], [dists[1:counts[i], i] for i in (e - s + 1):e])
            for (s, e) in zip(sizes, ends)]
end

# push! / pushfirst! (utils.jl:114-145): encode on the GPU and append in place on the device; the Julia lists get the same edit.
function _gpu_push!(ivfadc::GpuIndex{I}, point::Vector{Float32}, position::Symbol) where {I}
    nrows, nvectors = size(ivfadc)
    @assert nrows == length(point) "Adding to index requires $nrows-element vectors"
    @assert QuantizedArrays.TYPE_TO_BITS[I] >= log2(nvectors + 1) "Cannot index, exceeding index capacity"
    h = _handle(ivfadc)
    m = length(ivfadc.residual_quantizer.codebooks)
    (vecid, shift) = position == :first ? (0, 1) : (nvectors, 0)            # utils.jl:139
    U = _codetype(ivfadc)
    lst = Ref{Int32}(0); code = Vector{U}(undef, m); id = UInt32[vecid]
    _on_device(ivfadc) do
        shift == 0 || _check(ccall((:ivfadc_shift_ids, LIBIVFADC), Cint, (Ptr{Cvoid}, Int32), h.ptr, shift))   # _shift_up_inverse_index!
        if U === UInt16
            _check(ccall((:ivfadc_append_u16, LIBIVFADC), Cint,
                         (Ptr{Cvoid}, Int64, Ptr{Float32}, Ptr{UInt32}, Ref{Int32}, Ptr{Cvoid}),
                         h.ptr, 1, point, id, lst, code))
        else
            _check(ccall((:ivfadc_append, LIBIVFADC), Cint,
                         (Ptr{Cvoid}, Int64, Ptr{Float32}, Ptr{UInt32}, Ref{Int32}, Ptr{UInt8}),
                         h.ptr, 1, point, id, lst, code))
        end
    end
    if shift != 0
        for l in ivfadc.inverse_index
            l.idxs .+= one(I)                                                # utils.jl:2-6
        end
    end
    push!(ivfadc.inverse_index[lst[] + 1].idxs, I(vecid))
    push!(ivfadc.inverse_index[lst[] + 1].codes, code)
    return nothing
end

function push!(ivfadc::GpuIndex, point::Vector{Float32})
    if !_gpu_ok(ivfadc)     # :opq: the CPU encoder applies the rotation; the device copy is dropped and re-uploaded by the next search
        r = invoke(push!, Tuple{IVFADCIndex,Vector{Float32}}, ivfadc, point)
        hip_release!(ivfadc)
        return r
    end
    return _gpu_push!(ivfadc, point, :last)
end

function pushfirst!(ivfadc::GpuIndex, point::Vector{Float32})
    if !_gpu_ok(ivfadc)
        r = invoke(pushfirst!, Tuple{IVFADCIndex,Vector{Float32}}, ivfadc, point)
        hip_release!(ivfadc)
        return r
    end
    return _gpu_push!(ivfadc, point, :first)
end

# pop! / popfirst! / delete_from_index! (utils.jl:29-105): the reference's own method edits the Julia lists (and makes its assertions
# and the reconstruction); ivfadc_delete_ids then removes the same 0-based ids from the device copy in place -- stable within every
# list, every surviving id lowered by the number of removed ids below it (_shift_inverse_index!, utils.jl:11-27).
function _gpu_delete!(ivfadc::GpuIndex, ids::Vector{UInt32})
    h = lock(_registry_lock) do
        _drain_dead!()
        get(_handles, _key(ivfadc), nothing)
    end
    h === nothing && return nothing                  # no device copy yet: the next search uploads the edited lists
    _on_device(ivfadc) do
        _check(ccall((:ivfadc_delete_ids, LIBIVFADC), Cint, (Ptr{Cvoid}, Int64, Ptr{UInt32}, Ptr{Int64}),
                     h.ptr, length(ids), ids, C_NULL))
    end
    return nothing
end

function pop!(ivfadc::GpuIndex)
    n = length(ivfadc)
    rec = invoke(pop!, Tuple{IVFADCIndex}, ivfadc)                  # asserts n > 0; removes id n - 1, shifts nothing
    _gpu_delete!(ivfadc, UInt32[n - 1])
    return rec
end

function popfirst!(ivfadc::GpuIndex)
    rec = invoke(popfirst!, Tuple{IVFADCIndex}, ivfadc)             # removes id 0, lowers every other id by one
    _gpu_delete!(ivfadc, UInt32[0])
    return rec
end

function delete_from_index!(ivfadc::GpuIndex, points::Vector{<:Integer})
    invoke(delete_from_index!, Tuple{IVFADCIndex,Vector{<:Integer}}, ivfadc, points)   # `points` are 1-based (utils.jl:93)
    _gpu_delete!(ivfadc, UInt32.(unique(points) .- 1))
    return nothing
end

# Filtered search: a SUBSET VIEW of the device copy (ivfadc_clone_subset) -- deleteat! of utils.jl:98-99 applied, on a copy of the device
# lists, to every entry that is NOT named, without the _shift_inverse_index! of delete_from_index!: the named points keep their order and
# their ids, `ivfadc` itself is untouched.  `points` are 1-based, as delete_from_index! takes them (point p = stored id p - 1 = bit p - 1).
# The view is read-only and refuses to search once `ivfadc` has changed on the device (take a new one); it holds `ivfadc` alive.
struct HipSubset{I}
    handle::HipHandle
    parent::IVFADCIndex
end

function hip_subset(ivfadc::GpuIndex{I}, points::Vector{<:Integer}) where {I}
    h = _handle(ivfadc)
    nbits = isempty(points) ? 0 : Int(maximum(points))
    bits = zeros(UInt32, cld(nbits, 32))
    for p in points
        @assert p >= 1 "points are 1-based"
        bits[((p - 1) >> 5) + 1] |= UInt32(1) << ((p - 1) & 31)
    end
    out = Ref{Ptr{Cvoid}}(C_NULL)
    _check(ccall((:ivfadc_clone_subset, LIBIVFADC), Cint, (Ptr{Cvoid}, Ptr{UInt32}, UInt64, Ref{Ptr{Cvoid}}, Ptr{Int64}),
                 h.ptr, bits, nbits, out, C_NULL))
    hh = HipHandle(out[])
    finalizer(hh) do x
        x.ptr == C_NULL || ccall((:ivfadc_destroy, LIBIVFADC), Cvoid, (Ptr{Cvoid},), x.ptr)
        x.ptr = C_NULL
        _release!(x.q); _release!(x.ids); _release!(x.dists); _release!(x.counts)
    end
    return HipSubset{I}(hh, ivfadc)
end

function knn_search(s::HipSubset{I}, points::Vector{Vector{Float32}}, k::Int; w::Int=1) where {I}
    @assert k >= 1 "Number of neighbors must be k >= 1"
    @assert w >= 1 "Number of clusters to search in must be w >= 1"
    nq = length(points)
    nq == 0 && return Vector{I}[], Vector{Float32}[]
    d, kc = size(_centroids(s.parent.coarse_quantizer))
    q, ids, dists, counts = _io(s.handle, d, k, nq)
    for i in 1:nq
        @assert length(points[i]) == d "Searching requires $d-element vectors"
        copyto!(q, (i - 1) * d + 1, points[i], 1, d)
    end
    _check(ccall((:ivfadc_search, LIBIVFADC), Cint,
                 (Ptr{Cvoid}, Int64, Ptr{Float32}, Cint, Cint, Ptr{UInt32}, Ptr{Float32}, Ptr{Int32}),
                 s.handle.ptr, nq, q, k, min(w, kc), ids, dists, counts))
    return [I.(ids[1:counts[i], i]) for i in 1:nq], [dists[1:counts[i], i] for i in 1:nq]
end

# What is stored under a point (ivfadc_locate / ivfadc_reconstruct): the search loop of _pop! (utils.jl:49-55: the LAST list that holds
# the id, the FIRST position within it) and centre + _decode_point (utils.jl:58-59, 71-81), for a batch of 1-based points, computed on
# the DEVICE copy of the lists without removing anything.  hip_locate returns (clusters, positions), 1-based, 0 where no list holds the
# point; hip_reconstruct returns one Vector{Float32} per point and asserts that every point is stored.  The rotation of an :opq index
# is not applied: the reference's _decode_point does not apply it either.  The library's other two entries, ivfadc_locate_device and
# ivfadc_reconstruct_device, take device pointers (ids a search left on the GPU become vectors on the GPU, asynchronously on the handle's
# stream); this shim works on Julia arrays and does not call them.
function hip_locate(ivfadc::AnyGpuIndex, points::Vector{<:Integer})
    h = _handle(ivfadc)
    ids = UInt32.(points .- 1)
    lists = fill(Int32(-1), length(ids))
    pos = fill(Int64(-1), length(ids))
    _check(ccall((:ivfadc_locate, LIBIVFADC), Cint, (Ptr{Cvoid}, Int64, Ptr{UInt32}, Ptr{Int32}, Ptr{Int64}),
                 h.ptr, length(ids), ids, lists, pos))
    return Int.(lists) .+ 1, Int.(pos) .+ 1
end

function hip_reconstruct(ivfadc::AnyGpuIndex, points::Vector{<:Integer})
    h = _handle(ivfadc)
    ids = UInt32.(points .- 1)
    d = size(_centroids(ivfadc.coarse_quantizer), 1)
    vecs = zeros(Float32, d, length(ids))
    found = zeros(UInt8, length(ids))
    _check(ccall((:ivfadc_reconstruct, LIBIVFADC), Cint, (Ptr{Cvoid}, Int64, Ptr{UInt32}, Ptr{Float32}, Ptr{UInt8}),
                 h.ptr, length(ids), ids, vecs, found))
    missing_at = findfirst(iszero, found)
    @assert missing_at === nothing "point $(missing_at === nothing ? 0 : points[missing_at]) is not stored in the index"
    return [vecs[:, j] for j in 1:length(ids)]
end

end # module
