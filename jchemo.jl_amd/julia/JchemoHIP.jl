"""
    JchemoHIP

Julia host side of the MI355X-native PLS engine: the same call shapes as Jchemo.jl
(`plskern`, `plskern!`, `plsnipals`, `plsnipals!`, `transform`, `coef`, `predict`, `summary`), implemented
as thin `ccall`s into `libjchemo_hip.so` (C ABI: include/jchemo_hip.h).  AMDGPU.jl is used only as a handle
for device buffers (`ROCArray`); there is no CUDA path and no CPU fallback.

What a fit returns
  * Jchemo.jl loaded in the session (`using Jchemo` before or after `using JchemoHIP`) and HOST arrays in:
    the reference's own record `Jchemo.Plsr(T, P, R, W, C, TT, xmeans, xscales, ymeans, yscales, weights, niter)`
    (src/plskern.jl:1-14), so every consumer of the reference (`Jchemo.transform / coef / predict / summary`,
    `gridscorelv(...; fun = JchemoHIP.plskern)`, `locwlv`, `plsrda`, ... SURVEY §3.5) accepts it unchanged.
  * otherwise (Jchemo not loaded, or device-resident `ROCArray` inputs whose scores stay on the GPU): the
    fallback record `JchemoHIP.Plsr` below — same field names, same shapes, `T` / `weights` of the input's
    array type.  `attach!(Jchemo)` (called automatically when Jchemo is found) adds
    `Jchemo.transform / coef / predict` methods for it.
The accessors of this module (`JchemoHIP.transform`, `coef`, `predict`, `explvarx`) take EITHER record (they only
read the fields) and run on the GPU.

NOT EXECUTED IN THIS REPOSITORY'S CI: the build image has no Julia toolchain (see DESIGN.md).  Every
behaviour below is exercised through the identical C entry points by the ctypes mirror in
`jchemo.jl_amd/jchemo_hip/` (tests/test_gpu_parity.py); tests/test_julia_wrapper.py checks every `ccall` of this
file against include/jchemo_hip.h (literal signatures, argument counts and types).
"""
module JchemoHIP

using LinearAlgebra
using Random

export Plsr, Lwplsr, plskern, plskern!, plsnipals, plsnipals!, plssimp, plssimp!, plsrosa, plsrosa!, plswold, plswold!,
       lwplsr, transform, coef, predict, explvarx, JchCtx, attach!, nipals_one_pass!,
       msep, rmsep, ssr, bias, r2, cor2, mpar, segmkf, segmts, gridscorelv, gridcvlv,
       Plsrda, dummy, plsrda, Mbplsr, mbplsr, vip, xfit, xresid,
       Dkplsr, dkplsr, dkplsr!, krbf, kpol, Kplsr, kplsr, kplsr!, Kpca, kpca,
       Krr, krr, krr!, gridscorelb, Krrda, krrda,
       snv, snv!, detrend, detrend!, savgol, savgol!, savgk, mavg, mavg!, mavg_runmean, fdif,
       Covsel, Covselr, covsel, covsel!, covselr,
       Pca, Pcr, pcasvd, pcasvd!, pcaeigen, pcaeigen!, pcaeigenk, pcaeigenk!, pcr, pcr!, xtdx,
       colmedspa, pcasph, pcasph!,
       Occsd, Occod, Occsdod, occsd, occod, occsdod, row_resid_ss, row_resid_ss_lv,
       Occstah, occstah, stah, colmad, col_median_mad,
       sampks, sampdp, sampsys, sampcla, farthest_pair, maxmin_select,
       Knnr, Knnda, Occknndis, Occlknndis, getknn, knnr, knnda, occknndis, occlknndis, knn_search, knn_wmean, knn_vote, knn_gather_median,
       Dmkern, Kernda, dmkern, kdeda, plskdeda, kde_dens,
       Lwmlr, LwmlrS, Lwmlrda, LwmlrdaS, lwmlr, lwmlr_s, lwmlrda, lwmlrda_s, knn_wls,
       Dmnorm, Lda, Qda, dmnorm, lda, qda, matW, matB, mahsqchol, class_cov, gauss_factor, mahsq_chol,
       Lwplsrda, LwplsLda, LwplsQda, LwplsrS, LwplsrdaS, lwplsrda, lwplslda, lwplsqda, lwplsr_s, lwplsrda_s, knn_gda,
       viperm, isel, perm_fill, perm_score_sums

const LIB = get(ENV, "JCHEMO_HIP_LIB", joinpath(@__DIR__, "..", "lib", "libjchemo_hip.so"))

# ---- status / context ---------------------------------------------------------------------------
mutable struct JchCtx
    h::Ptr{Cvoid}
    function JchCtx(device::Integer = 0; stream::Ptr{Cvoid} = C_NULL)
        r = Ref{Ptr{Cvoid}}(C_NULL)
        st = ccall((:jch_ctx_create, LIB), Int32, (Ref{Ptr{Cvoid}}, Int32, Ptr{Cvoid}, UInt32), r, device, stream, 0)
        st == 0 || error("jch_ctx_create: ", unsafe_string(ccall((:jch_last_error, LIB), Cstring, (Ptr{Cvoid},), C_NULL)))
        ctx = new(r[])
        finalizer(c -> ccall((:jch_ctx_destroy, LIB), Int32, (Ptr{Cvoid},), c.h), ctx)
        ctx
    end
end

check(ctx::JchCtx, st::Integer) =
    st == 0 || error("libjchemo_hip error $st: ", unsafe_string(ccall((:jch_last_error, LIB), Cstring, (Ptr{Cvoid},), ctx.h)))

const _default = Ref{Union{Nothing, JchCtx}}(nothing)
default_ctx() = (_default[] === nothing && (_default[] = JchCtx(0)); _default[])

"Join this process' context to a row-sharded multi-GPU fit (one Julia process per GPU; `uid` from rank 0's
`unique_id()`, exchanged with MPI.jl / Distributed)."
function unique_id()
    b = zeros(UInt8, 128)
    ccall((:jch_comm_unique_id, LIB), Int32, (Ptr{Cvoid},), b) == 0 || error("jch_comm_unique_id: RCCL not loadable")
    b
end
comm_init!(ctx::JchCtx, uid::Vector{UInt8}, rank::Integer, nranks::Integer) =
    check(ctx, ccall((:jch_ctx_comm_init, LIB), Int32, (Ptr{Cvoid}, Ptr{Cvoid}, Int32, Int32), ctx.h, uid, rank, nranks))

# ---- the reference package, when it is loaded --------------------------------------------------------
const _JCHEMO_ID = Base.PkgId(Base.UUID("fbca9394-dd0a-4d1c-b066-ae75f6ef1ad5"), "Jchemo")   # Project.toml:1-2 of the reference
const _jchemo = Ref{Union{Nothing, Module}}(nothing)

"The loaded `Jchemo` module, or `nothing`.  Found through its package id, so the load order does not matter."
function jchemo_module()
    if _jchemo[] === nothing
        m = get(Base.loaded_modules, _JCHEMO_ID, nothing)
        m === nothing || attach!(m)
    end
    _jchemo[]
end

# ---- tables: the reference returns DataFrames (gridscore.jl:196-220, gridcv.jl:211-227, plskern.jl:258-259) --------------------
const _DATAFRAMES_ID = Base.PkgId(Base.UUID("a93c6f00-e57d-5684-b7b6-d8193f3e46c0"), "DataFrames")   # Project.toml:8 of the reference
"The loaded `DataFrames` module (a dependency of Jchemo, so present whenever Jchemo is), or `nothing`."
dataframes_module() = get(Base.loaded_modules, _DATAFRAMES_ID, nothing)

"""
`_table(cols)`: `cols` is a NamedTuple of equal-length column vectors IN THE REFERENCE'S COLUMN ORDER.  With DataFrames loaded the
result is `DataFrame(cols)` — the type the reference returns —, otherwise the NamedTuple itself (a Tables.jl column table with the
same column names, so `DataFrame(t)` gives the reference's table).
"""
function _table(cols::NamedTuple)
    D = dataframes_module()
    D === nothing ? cols : Base.invokelatest(getfield(D, :DataFrame), cols)
end
_ynames(q) = Tuple(Symbol("y", i) for i in 1:q)                     # `namy = map(string, repeat(["y"], q), 1:q)`

# ---- fallback result record: field names / shapes of Jchemo.Plsr (src/plskern.jl:1-14) ---------------
struct Plsr{TT_, WT}
    T::TT_                      # n x nlv   (Matrix{Float64}, or ROCArray for device-resident fits)
    P::Matrix{Float64}
    R::Matrix{Float64}
    W::Matrix{Float64}
    C::Matrix{Float64}
    TT::Vector{Float64}
    xmeans::Vector{Float64}
    xscales::Vector{Float64}
    ymeans::Vector{Float64}
    yscales::Vector{Float64}
    weights::WT
    niter::Union{Array{Float64}, Nothing}
end

"""
    attach!(Jchemo)

Remember the reference module (fits on host arrays then return `Jchemo.Plsr` / `Jchemo.Lwplsr`) and give the
reference's generics methods for the fallback record, so `Jchemo.predict(fm, X)` also works on a device-resident fit.
"""
function attach!(J::Module)
    _jchemo[] === J && return J
    _jchemo[] = J
    Core.eval(J, :(transform(object::$Plsr, X; nlv = nothing) = $transform(object, X; nlv = nlv)))
    Core.eval(J, :(coef(object::$Plsr; nlv = nothing) = $coef(object; nlv = nlv)))
    Core.eval(J, :(predict(object::$Plsr, X; nlv = nothing) = $predict(object, X; nlv = nlv)))
    Core.eval(J, :(transform(object::$Dkplsr, X; nlv = nothing) = $transform(object, X; nlv = nlv)))
    Core.eval(J, :(coef(object::$Dkplsr; nlv = nothing) = $coef(object; nlv = nlv)))
    Core.eval(J, :(predict(object::$Dkplsr, X; nlv = nothing) = $predict(object, X; nlv = nlv)))
    for K in (Kplsr, getfield(J, :Kplsr))   # the fallback record and the reference's own (Kt / DKt empty, D = the weights)
        Core.eval(J, :(transform(object::$K, X; nlv = nothing) = $transform(object, X; nlv = nlv)))
        Core.eval(J, :(coef(object::$K; nlv = nothing) = $coef(object; nlv = nlv)))
        Core.eval(J, :(predict(object::$K, X; nlv = nothing) = $predict(object, X; nlv = nlv)))
    end
    J
end

# the record a fit hands back (see the module docstring)
function _record(T, P, R, W, C, TT, xm, xs, ym, ys, wn, niter)
    J = jchemo_module()
    if J !== nothing && T isa Matrix{Float64} && wn isa Vector{Float64}
        return Base.invokelatest(getfield(J, :Plsr), T, P, R, W, C, TT, xm, xs, ym, ys, wn, niter)
    end
    Plsr(T, P, R, W, C, TT, xm, xs, ym, ys, wn, niter)
end

struct PlsDesc                                          # == jch_pls_desc (include/jchemo_hip.h)
    n::Int64; p::Int64; q::Int64
    nlv::Int32; scal::Int32; dtype::Int32; loc::Int32; inplace::Int32; reserved::Int32
end

ensure_mat(X::AbstractMatrix) = X                       # src/utility.jl:544-548
ensure_mat(X::AbstractVector) = reshape(X, :, 1)
ensure_mat(X::Number) = reshape([X], 1, 1)

# Host arrays: loc = 0.  Device arrays (AMDGPU.ROCArray{Float64,2}): loc = 1; `pointer(A)` is the device address.
_loc(::Array) = Int32(0)
_loc(A) = Int32(1)                                      # any other strided column-major device array type
_similar(A::Array, dims...) = Array{Float64}(undef, dims...)
_similar(A, dims...) = similar(A, Float64, dims...)
_f64(A::Array{Float64}) = A
_f64(A::Array) = Float64.(A)
_f64(A) = A                                             # device arrays are taken as they are (Float64 required)
"`v` as a vector living where `like` lives (host Vector / device array of `like`'s type)"
_colocate(v, like::Array) = v isa Vector{Float64} ? v : Vector{Float64}(Array(v))
_colocate(v, like) = v isa Array ? copyto!(_similar(like, length(v)), vec(Float64.(v))) : v

# One method per entry point, each with its LITERAL argument-type tuple (`ccall` needs the tuple spelled out where it
# is called; a constant bound to the tuple is a lowering error).  jch_plskern_fit and its same-signature siblings:
for alg in (:plskern, :plsnipals, :plssimp, :plsrosa)
    cname = QuoteNode(Symbol(:jch_, alg, :_fit))
    @eval _fit_call(::Val{$(QuoteNode(alg))}, h, desc, X, ldx, Y, ldy, w, T, P, R, W, C, TT, xm, xs, ym, ys, wn, got) =
        ccall(($cname, LIB), Int32,
              (Ptr{Cvoid}, Ref{PlsDesc}, Ptr{Cvoid}, Int64, Ptr{Cvoid}, Int64, Ptr{Float64}, Ptr{Float64},
               Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64},
               Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ref{Int32}),
              h, desc, X, ldx, Y, ldy, w, T, P, R, W, C, TT, xm, xs, ym, ys, wn, got)
end

# sym: :plskern | :plsnipals | :plssimp | :plsrosa (one C signature) or :plswold (tol, maxit, niter in addition)
function _fit(sym::Symbol, X, Y, weights, nlv, scal, inplace, ctx::JchCtx; tol = sqrt(eps(1.)), maxit = 200, options = 0)
    n, p = size(X); q = size(Y, 2)
    size(Y, 1) == n || throw(DimensionMismatch("X has $n rows, Y has $(size(Y, 1))"))
    # min(n, p, nlv) as src/plskern.jl:116 — exactly the columns the library fills on one GPU, so T is handed back as
    # allocated (no n x nlv copy); a row shard smaller than nlv of a multi-GPU fit may come back with more (k > n)
    kmax = max(1, min(p, nlv, ctx_nranks(ctx) > 1 ? typemax(Int) : n))
    T = _similar(X, n, kmax); wn = _similar(X, n)
    P = zeros(p, kmax); R = zeros(p, kmax); W = zeros(p, kmax); C = zeros(q, kmax); TT = zeros(kmax)
    xm = zeros(p); xs = zeros(p); ym = zeros(q); ys = zeros(q); niter = zeros(kmax)
    desc = Ref(PlsDesc(n, p, q, nlv, scal ? 1 : 0, 0, _loc(X), inplace ? 1 : 0, options))
    got = Ref{Int32}(0)
    GC.@preserve X Y weights T wn begin
        w = weights === nothing ? Ptr{Float64}(C_NULL) : pointer(weights)
        st = if sym === :plswold
            ccall((:jch_plswold_fit, LIB), Int32,
                  (Ptr{Cvoid}, Ref{PlsDesc}, Ptr{Cvoid}, Int64, Ptr{Cvoid}, Int64, Ptr{Float64}, Float64, Int32, Ptr{Float64},
                   Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64},
                   Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ref{Int32}),
                  ctx.h, desc, pointer(X), stride(X, 2), pointer(Y), max(stride(Y, 2), n), w, tol, maxit, pointer(T),
                  P, R, W, C, TT, xm, xs, ym, ys, pointer(wn), niter, got)
        else
            _fit_call(Val(sym), ctx.h, desc, pointer(X), stride(X, 2), pointer(Y), max(stride(Y, 2), n), w, pointer(T),
                      P, R, W, C, TT, xm, xs, ym, ys, pointer(wn), got)
        end
        check(ctx, st)
    end
    k = Int(got[])
    cut(A) = k == size(A, 2) ? A : A[:, 1:k]
    _record(cut(T), cut(P), cut(R), cut(W), cut(C), k == length(TT) ? TT : TT[1:k], xm, xs, ym, ys, wn,
            sym === :plswold ? (k == length(niter) ? niter : niter[1:k]) : nothing)
end

function ctx_nranks(ctx::JchCtx)
    r = Ref{Int32}(0); nr = Ref{Int32}(1)
    ccall((:jch_ctx_comm_info, LIB), Int32, (Ptr{Cvoid}, Ref{Int32}, Ref{Int32}), ctx.h, r, nr)
    Int(nr[])
end

# Diagnostic counters of a ctx (include/jchemo_hip.h): 0 raw-mode fits repeated on the centred copy, 1 kNN-LWPLSR queries refitted per
# query after the neighbour-space kernel's pivot check, 2 queries whose neighbours the screened search found, 3 those of them the
# exact scan redid (the results do not depend on it; ENV["JCH_KNN_SCREEN"] = "0" selects the exact scan for every query)
const COUNTER_PIVOT_REFITS = Int32(0); const COUNTER_LOCW_REFITS = Int32(1)
const COUNTER_KNN_SCREENED = Int32(2); const COUNTER_KNN_SCREEN_REDONE = Int32(3)
function counter(ctx::JchCtx, which::Integer)
    v = Ref{Int64}(0)
    check(ctx, ccall((:jch_ctx_get_counter, LIB), Int32, (Ptr{Cvoid}, Int32, Ref{Int64}), ctx.h, Int32(which), v))
    Int(v[])
end

# weights where X lives (`nothing` = ones(n), as the reference's default argument)
_w(weights, X) = weights === nothing ? nothing : _colocate(vec(weights), X)
# non-`!` variants: any real matrix / vector / DataFrame-free input; the library never writes the inputs (inplace = 0),
# so the reference's `copy` (src/plskern.jl:108) is not needed
_in(X) = _f64(ensure_mat(X))

"`plskern(X, Y, weights = ones(n); nlv, scal = false)` — src/plskern.jl:106-110 (inputs untouched)."
plskern(X, Y, weights = nothing; nlv, scal = false, ctx = default_ctx()) =
    _fit(:plskern, _in(X), _in(Y), _w(weights, _in(X)), nlv, scal, false, ctx; options = _same_x[])
"`plskern!(X::Matrix, Y::Matrix, ...)` — src/plskern.jl:112-178: X, Y are overwritten (centred/scaled)."
plskern!(X, Y, weights = nothing; nlv, scal = false, ctx = default_ctx()) =
    _fit(:plskern, X, Y, _w(weights, X), nlv, scal, true, ctx)
"`plsnipals` — src/plsnipals.jl:31-35."
plsnipals(X, Y, weights = nothing; nlv, scal = false, ctx = default_ctx()) =
    _fit(:plsnipals, _in(X), _in(Y), _w(weights, _in(X)), nlv, scal, false, ctx; options = _nipals_options[] | _same_x[])
"`plsnipals!` — src/plsnipals.jl:37-97: X, Y end up centred/scaled and deflated."
plsnipals!(X, Y, weights = nothing; nlv, scal = false, ctx = default_ctx()) =
    _fit(:plsnipals, X, Y, _w(weights, X), nlv, scal, true, ctx)

# Sibling algorithms (same row kernels, different small state; include/jchemo_hip.h)
"`plssimp` — src/plssimp.jl:22-26 (`W` is returned equal to `R`, :85-87)."
plssimp(X, Y, weights = nothing; nlv, scal = false, ctx = default_ctx()) =
    _fit(:plssimp, _in(X), _in(Y), _w(weights, _in(X)), nlv, scal, false, ctx; options = _same_x[])
"`plssimp!` — src/plssimp.jl:28-88."
plssimp!(X, Y, weights = nothing; nlv, scal = false, ctx = default_ctx()) =
    _fit(:plssimp, X, Y, _w(weights, X), nlv, scal, true, ctx)
"`plsrosa` — src/plsrosa.jl:26-30."
plsrosa(X, Y, weights = nothing; nlv, scal = false, ctx = default_ctx()) =
    _fit(:plsrosa, _in(X), _in(Y), _w(weights, _in(X)), nlv, scal, false, ctx; options = _same_x[])
"`plsrosa!` — src/plsrosa.jl:32-96: X centred/scaled, Y centred/scaled and deflated."
plsrosa!(X, Y, weights = nothing; nlv, scal = false, ctx = default_ctx()) =
    _fit(:plsrosa, X, Y, _w(weights, X), nlv, scal, true, ctx)
"`plswold` — src/plswold.jl:30-34; `niter` filled as :93."
plswold(X, Y, weights = nothing; nlv, tol = sqrt(eps(1.)), maxit = 200, scal = false, ctx = default_ctx()) =
    _fit(:plswold, _in(X), _in(Y), _w(weights, _in(X)), nlv, scal, false, ctx; tol = tol, maxit = maxit, options = _wold_options[] | _nipals_options[] | _same_x[])
"`plswold!` — src/plswold.jl:36-111."
plswold!(X, Y, weights = nothing; nlv, tol = sqrt(eps(1.)), maxit = 200, scal = false, ctx = default_ctx()) =
    _fit(:plswold, X, Y, _w(weights, X), nlv, scal, true, ctx; tol = tol, maxit = maxit, options = _wold_options[])
# jch_pls_desc.reserved for plswold: 0 (default) = finite scores for zero-weight rows (what a zero-weight CV fold needs);
# 2 = JCH_WOLD_REF_ZERO_WEIGHT_NAN, the reference's NaN (src/plswold.jl:107).  A module switch, not a keyword: the keyword list of
# `plswold` stays the reference's (src/plswold.jl:30-31), so higher-order callers can pass it through unchanged.
const _wold_options = Ref{Int32}(0)
"`wold_zero_weight_nan!(true)`: `plswold` gives rows with weight 0 NaN scores as the reference does; `false` (default): finite."
wold_zero_weight_nan!(on::Bool) = (_wold_options[] = on ? Int32(2) : Int32(0); on)

# JCH_NIPALS_ONE_PASS (include/jchemo_hip.h): OPT-IN, never the default — plsnipals / plswold (the non-`!` forms) with ONE pass over X
# per LV: K_{a+1} = K_a - zp_raw c_raw' / tt instead of the reference's recomputation of X'DY from the deflated matrices
# (src/plsnipals.jl:71).  Same results up to rounding.  A module switch for the same reason as above.
const _nipals_options = Ref{Int32}(0)
"`nipals_one_pass!(true)`: `plsnipals` / `plswold` use the one-pass variant (q <= 16, p <= 2048); `false` (default): the reference's schedule."
nipals_one_pass!(on::Bool) = (_nipals_options[] = on ? Int32(4) : Int32(0); on)

# JCH_REUSE_XCOPY (include/jchemo_hip.h): the promise that X — pointer and contents — is what the previous fit on this ctx was given; a
# Float64 plskern-shaped fit then takes X'DY from the row-major copy that fit left in the workspace instead of staging and transposing
# X again.  Set by `gridcvlv` around its second and later fits (the same X, other weights); a module switch like the two above.
const _same_x = Ref{Int32}(0)

# out = ((X - 1*shift') ./ scale') * B .+ bias'   (shift, scale, B, bias on the host; X and out where X lives)
function _affine(X, shift, scale, B::Matrix{Float64}, bias, ctx)
    X = _in(X); m, p = size(X); k = size(B, 2)
    size(B, 1) == p || throw(DimensionMismatch("X has $p columns, the model has $(size(B, 1))"))
    out = _similar(X, m, k)
    GC.@preserve X out shift scale bias begin
        check(ctx, ccall((:jch_affine_gemm, LIB), Int32,
                         (Ptr{Cvoid}, Int32, Ptr{Float64}, Int64, Int64, Int64, Ptr{Float64}, Ptr{Float64}, Ptr{Float64},
                          Int64, Ptr{Float64}, Ptr{Float64}, Int64),
                         ctx.h, _loc(X), pointer(X), m, p, stride(X, 2),
                         shift === nothing ? Ptr{Float64}(C_NULL) : pointer(shift),
                         scale === nothing ? Ptr{Float64}(C_NULL) : pointer(scale), B, k,
                         bias === nothing ? Ptr{Float64}(C_NULL) : pointer(bias), pointer(out), m))
    end
    out
end

_nlv_fit(object) = size(object.P, 2)     # (== nco(object.T) of the reference; P is always a host matrix)

"`transform(object, X; nlv)` — src/plskern.jl:187-195 on the GPU; `object`: `Jchemo.Plsr` or `JchemoHIP.Plsr`."
function transform(object, X; nlv = nothing, ctx = default_ctx())
    hasproperty(object, :vtot) && return _transform_kplsr(object, X, nlv, ctx)
    hasproperty(object, :kern) && return _transform_dkplsr(object, X, nlv, ctx)
    hasproperty(object, :lev) && return transform(object.fm, X; nlv = nlv, ctx = ctx)          # Plsrda: src/plsrda.jl:86-88
    hasproperty(object, :bscales) && return _transform_mbplsr(object, X, nlv, ctx)
    a = _nlv_fit(object)
    nlv = nlv === nothing ? a : min(nlv, a)
    _affine(X, object.xmeans, object.xscales, nlv == a ? object.R : object.R[:, 1:nlv], nothing, ctx)
end

"`coef(object; nlv)` — src/plskern.jl:207-217 (p x q host glue, as in the reference)"
function coef(object; nlv = nothing)
    hasproperty(object, :vtot) && return _coef_kplsr(object, nlv)
    hasproperty(object, :kern) && return coef(object.fm; nlv = nlv)                            # Dkplsr: src/dkplsr.jl:146-148
    a = _nlv_fit(object)
    nlv = nlv === nothing ? a : min(nlv, a)
    beta = object.C[:, 1:nlv]'
    B = Diagonal(1 ./ object.xscales) * object.R[:, 1:nlv] * beta * Diagonal(object.yscales)
    int = object.ymeans' .- object.xmeans' * B
    (B = B, int = int)
end

# m x (q * (hi - lo + 1)) predictions for nlv = lo..hi, level-major columns: ONE library call (jch_predict) and one pass over X — up to two
# levels as one GEMM, more as the scores X_c R followed by running sums over the score columns (include/jchemo_hip.h)
function _predict_range(object, X, lo::Integer, hi::Integer, ctx)
    X = _in(X); m, p = size(X); q = size(object.C, 1)
    size(object.R, 1) == p || throw(DimensionMismatch("X has $p columns, the model has $(size(object.R, 1))"))
    out = _similar(X, m, q * (hi - lo + 1))
    R = Matrix{Float64}(object.R); Cm = Matrix{Float64}(object.C)
    xm = Vector{Float64}(vec(object.xmeans)); xs = Vector{Float64}(vec(object.xscales))
    ym = Vector{Float64}(vec(object.ymeans)); ys = Vector{Float64}(vec(object.yscales))
    GC.@preserve X out R Cm xm xs ym ys check(ctx, ccall((:jch_predict, LIB), Int32,
        (Ptr{Cvoid}, Int32, Ptr{Float64}, Int64, Int64, Int64, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64},
         Ptr{Float64}, Int64, Int32, Int32, Ptr{Float64}, Int64),
        ctx.h, _loc(X), pointer(X), m, p, stride(X, 2), pointer(xm), pointer(xs), pointer(ym), pointer(ys), pointer(R), pointer(Cm), q,
        lo, hi, pointer(out), max(m, 1)))
    out
end

"""`predict(object, X; nlv)` — src/plskern.jl:226-238 (a `Plsr` record) or src/lwplsr.jl:134-166 (an `Lwplsr` record).
PLSR: the whole nlv range in ONE pass over X (`jch_predict`)."""
function predict(object, X; nlv = nothing, ctx = default_ctx())
    hasproperty(object, :metric) && return _predict_lwplsr(object, X, nlv, ctx)
    hasproperty(object, :lev) && return _predict_plsrda(object, X, nlv, ctx)
    hasproperty(object, :bscales) && return _predict_mbplsr(object, X, nlv, ctx)
    hasproperty(object, :vtot) && return _predict_kplsr(object, X, nlv, ctx)
    hasproperty(object, :kern) && return _predict_dkplsr(object, X, nlv, ctx)
    a = _nlv_fit(object); q = size(object.C, 1)
    rng = nlv === nothing ? (a:a) : (max(0, minimum(nlv)):min(a, maximum(nlv)))
    out = _predict_range(object, X, first(rng), last(rng), ctx)
    pred = [out[:, (i - 1) * q + 1:i * q] for i in 1:length(rng)]
    (pred = length(rng) == 1 ? pred[1] : pred,)
end

"""
    explvarx(object, X)

The table of `summary(object::Plsr, X)` (src/plskern.jl:246-260): a `DataFrame` with the columns `nlv, var, pvar, cumpvar`
when DataFrames is loaded (it is whenever Jchemo is), the same columns as a NamedTuple otherwise; `sstot` computed on the GPU.  `object`: either record; X: the data the model was fitted on.
"""
function explvarx(object, X; ctx = default_ctx())
    X = _in(X); n, nlv = size(X, 1), _nlv_fit(object)
    d = _colocate(object.weights, X)          # the (normalised) weights where X lives
    ss = Ref{Float64}(0.0)
    GC.@preserve X d begin
        check(ctx, ccall((:jch_weighted_ss, LIB), Int32,
                         (Ptr{Cvoid}, Int32, Ptr{Float64}, Int64, Int64, Int64, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ref{Float64}),
                         ctx.h, _loc(X), pointer(X), n, size(X, 2), stride(X, 2), pointer(d),
                         object.xmeans, object.xscales, ss))
    end
    tt_adj = vec(sum(object.P .^ 2, dims = 1)) .* object.TT
    pvar = tt_adj / ss[]
    _table((nlv = collect(1:nlv), var = tt_adj / n, pvar = pvar, cumpvar = cumsum(pvar)))   # src/plskern.jl:258: DataFrame(nlv, var, pvar, cumpvar)
end

"`summary(object::JchemoHIP.Plsr, X)` — src/plskern.jl:246-260: `(explvarx = table,)`.  (A `Jchemo.Plsr` returned by a
fit has the reference's own `summary` method; `explvarx` is the GPU version for either record.)"
Base.summary(object::Plsr, X; ctx = default_ctx()) = (explvarx = explvarx(object, X; ctx = ctx),)

# ---- kNN-LWPLSR (src/lwplsr.jl) -------------------------------------------------------------------
struct Lwplsr                     # fallback record, same fields as the reference's struct (src/lwplsr.jl:1-12)
    X; Y; fm; metric::String; h::Real; k::Int; nlv::Int; tol::Real; scal::Bool; verbose::Bool
end

"`lwplsr(X, Y; nlvdis, metric, h, k, nlv, tol = 1e-4, scal = false)` — src/lwplsr.jl:114-126."
function lwplsr(X, Y; nlvdis, metric, h, k, nlv, tol = 1e-4, scal = false, verbose = false, ctx = default_ctx())
    X = _in(X); Y = _in(Y)
    fm = nlvdis == 0 ? nothing : plskern(X, Y; nlv = nlvdis, scal = scal, ctx = ctx)
    J = jchemo_module()
    if J !== nothing && X isa Array{Float64} && Y isa Array{Float64}
        return Base.invokelatest(getfield(J, :Lwplsr), X, Y, fm, metric, h, k, nlv, tol, scal, verbose)
    end
    Lwplsr(X, Y, fm, metric, h, k, nlv, tol, scal, verbose)
end

function _cov(A, ctx)             # Statistics.cov(A, corrected = false) on the device (src/getknn.jl:38)
    n, d = size(A); S = zeros(d, d)
    GC.@preserve A check(ctx, ccall((:jch_weighted_cov, LIB), Int32,
        (Ptr{Cvoid}, Int32, Ptr{Float64}, Int64, Int64, Int64, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}),
        ctx.h, _loc(A), pointer(A), n, d, stride(A, 2), Ptr{Float64}(C_NULL), S, Ptr{Float64}(C_NULL)))
    S
end

# ---- model-constant device data of an Lwplsr object, prepared once (include/jchemo_hip.h: jch_lwplsr_prepare) -------------
# The reference fits `Lwplsr` once and predicts from it many times (src/lwplsr.jl:1-12).  `prepare(fm)` keeps the row-major
# copy of Xtrain, Ytrain and the whitened training scores on the device; `predict(prepared, X)` then only ships the queries.
mutable struct LwplsrPrepared
    object                       # the Lwplsr record (either module's)
    h::Ptr{Cvoid}                # jch_lwplsr_model*
    qmap                         # query block -> coordinates of the neighbour search
    dd::Int
    ctx::JchCtx
    device_map::Bool             # the handle maps the queries itself (jch_lwplsr_add_query_map): predict passes Zq = C_NULL
end

"`prepare(object::Lwplsr; ctx)`: device handle of the model-constant data; release with `release!` (or let the GC do it)."
function prepare(object; ctx = default_ctx())
    Xt = _in(object.X); Yt = _colocate_mat(_in(object.Y), Xt)
    n, p = size(Xt); q = size(Yt, 2)
    Zt, qmap, stages = _knn_train_space(object, Xt, ctx)
    Zt = _colocate_mat(Zt, Xt)
    r = Ref{Ptr{Cvoid}}(C_NULL)
    GC.@preserve Xt Yt Zt check(ctx, ccall((:jch_lwplsr_prepare, LIB), Int32,
        (Ptr{Cvoid}, Int32, Ptr{Float64}, Int64, Int64, Int64, Ptr{Float64}, Int64, Int64, Ptr{Float64}, Int64, Int64, Ref{Ptr{Cvoid}}),
        ctx.h, _loc(Xt), pointer(Xt), n, p, stride(Xt, 2), pointer(Yt), q, max(stride(Yt, 2), n), pointer(Zt), stride(Zt, 2), size(Zt, 2), r))
    pm = LwplsrPrepared(object, r[], qmap, size(Zt, 2), ctx, false)
    finalizer(release!, pm)
    # the query map travels with the handle: two jch_affine_gemm calls per predict (each with an upload of its matrix and a
    # stream synchronisation) become two launches inside jch_lwplsr_predict_prepared
    for (shift, scale, B) in stages
        Bm = Matrix{Float64}(B)
        sh = shift === nothing ? Float64[] : Vector{Float64}(vec(shift))
        sc = scale === nothing ? Float64[] : Vector{Float64}(vec(scale))
        GC.@preserve Bm sh sc check(ctx, ccall((:jch_lwplsr_add_query_map, LIB), Int32,
            (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Int64, Int64, Ptr{Float64}),
            ctx.h, pm.h, shift === nothing ? Ptr{Float64}(C_NULL) : pointer(sh), scale === nothing ? Ptr{Float64}(C_NULL) : pointer(sc),
            pointer(Bm), size(Bm, 1), size(Bm, 2), Ptr{Float64}(C_NULL)))
    end
    pm.device_map = !isempty(stages)
    pm
end
function release!(pm::LwplsrPrepared)
    pm.h == C_NULL && return nothing
    ccall((:jch_lwplsr_release, LIB), Int32, (Ptr{Cvoid}, Ptr{Cvoid}), C_NULL, pm.h)
    pm.h = C_NULL
    nothing
end

# the space the neighbours are searched in (src/lwplsr.jl:139-150, src/getknn.jl:37-49): training coordinates + query map
function _knn_train_space(object, Xt, ctx)
    stages = Any[]                            # the query map as affine stages (shift, scale, B) for jch_lwplsr_add_query_map
    if object.fm === nothing
        if object.scal                        # :141-145  scale(object.X, colstd(object.X)) on both sides
            xs = col_stats(Xt; ctx = ctx).stds
            Dinv = Matrix(Diagonal(1 ./ xs))
            Zt = _affine(Xt, nothing, nothing, Dinv, nothing, ctx)
            qmap = Xq -> _affine(Xq, nothing, nothing, Dinv, nothing, ctx)
            push!(stages, (nothing, nothing, Dinv))
        else
            Zt = Xt
            qmap = Xq -> Xq
        end
    else
        fmg = object.fm
        Zt = _colocate_mat(fmg.T, Xt)
        qmap = Xq -> transform(fmg, Xq; ctx = ctx)
        push!(stages, (fmg.xmeans, fmg.xscales, fmg.R))
    end
    if object.metric == "mahal"               # src/getknn.jl:37-49
        S = _cov(Zt, ctx); d = size(S, 1)
        Uinv = d == 1 ? fill(1 / sqrt(S[1, 1]), 1, 1) : (isposdef(S) ? Matrix(inv(cholesky(Hermitian(S)).U)) : Matrix(Diagonal(1 ./ diag(S))))
        Zt = _affine(Zt, nothing, nothing, Uinv, nothing, ctx)
        inner = qmap
        qmap = Xq -> _affine(inner(Xq), nothing, nothing, Uinv, nothing, ctx)
        push!(stages, (nothing, nothing, Uinv))
    end
    Zt, qmap, stages
end

"`predict(pm::LwplsrPrepared, X; nlv)` — src/lwplsr.jl:134-166 on the prepared handle."
function predict(pm::LwplsrPrepared, X; nlv = nothing)
    object = pm.object; ctx = pm.ctx
    X = _in(X); m = size(X, 1); n, p = size(object.X); q = size(object.Y, 2)
    a = object.nlv
    rng = nlv === nothing ? (a:a) : (max(minimum(nlv), 0):min(maximum(nlv), a, p))
    Zq = pm.device_map ? X : _colocate_mat(pm.qmap(X), X)    # (device_map: Zq is not read, C_NULL goes down)
    k = min(object.k, n); le = length(rng)
    pred = zeros(q, le, m); ind = zeros(Int32, k, m); dist = zeros(k, m); w = zeros(k, m)   # C layout [m][le][q] == Julia (q, le, m)
    GC.@preserve Zq X check(ctx, ccall((:jch_lwplsr_predict_prepared, LIB), Int32,
        (Ptr{Cvoid}, Ptr{Cvoid}, Int32, Ptr{Float64}, Int64, Ptr{Float64}, Int64, Int64, Int32, Float64, Float64, Int32, Int32, Int32,
         Ptr{Float64}, Ptr{Int32}, Ptr{Float64}, Ptr{Float64}),
        ctx.h, pm.h, _loc(X), pm.device_map ? Ptr{Float64}(C_NULL) : pointer(Zq), stride(Zq, 2), pointer(X), m, stride(X, 2), k, object.h,
        object.tol, object.scal ? 1 : 0, first(rng), last(rng), pred, ind, dist, w))
    preds = [permutedims(pred[:, i, :]) for i in 1:le]
    (pred = le == 1 ? preds[1] : preds, listnn = [Int.(ind[:, i]) .+ 1 for i in 1:m], listd = [dist[:, i] for i in 1:m],
     listw = [w[:, i] for i in 1:m])
end

# `predict(object::Lwplsr, X; nlv)` — src/lwplsr.jl:134-166: neighbours, weights and the m local fits in one call.
function _predict_lwplsr(object, X, nlv, ctx)
    X = _in(X); m = size(X, 1); n, p = size(object.X); q = size(object.Y, 2)
    a = object.nlv
    rng = nlv === nothing ? (a:a) : (max(minimum(nlv), 0):min(maximum(nlv), a, p))
    Xt = _colocate_mat(_in(object.X), X)
    Zt, qmap, _ = _knn_train_space(object, Xt, ctx)
    Zt = _colocate_mat(Zt, X); Zq = _colocate_mat(qmap(X), X)
    k = min(object.k, n); le = length(rng)
    # (no shape limits: outside the batched kernels' envelope the library runs its per-query generic paths, include/jchemo_hip.h)
    pred = zeros(q, le, m); ind = zeros(Int32, k, m); dist = zeros(k, m); w = zeros(k, m)   # C layout [m][le][q] == Julia (q, le, m)
    Yt = _colocate_mat(_in(object.Y), X)
    GC.@preserve Xt Yt Zt Zq X check(ctx, ccall((:jch_lwplsr_predict, LIB), Int32,
        (Ptr{Cvoid}, Int32, Ptr{Float64}, Int64, Int64, Int64, Ptr{Float64}, Int64, Int64, Ptr{Float64}, Int64, Ptr{Float64}, Int64,
         Int64, Ptr{Float64}, Int64, Int64, Int32, Float64, Float64, Int32, Int32, Int32, Ptr{Float64}, Ptr{Int32}, Ptr{Float64}, Ptr{Float64}),
        ctx.h, _loc(Xt), pointer(Xt), n, p, stride(Xt, 2), pointer(Yt), q, max(stride(Yt, 2), n), pointer(Zt), stride(Zt, 2),
        pointer(Zq), stride(Zq, 2), size(Zt, 2), pointer(X), m, stride(X, 2), k, object.h, object.tol, object.scal ? 1 : 0,
        first(rng), last(rng), pred, ind, dist, w))
    preds = [permutedims(pred[:, i, :]) for i in 1:le]                                      # m x q per nlv
    (pred = le == 1 ? preds[1] : preds, listnn = [Int.(ind[:, i]) .+ 1 for i in 1:m], listd = [dist[:, i] for i in 1:m],
     listw = [w[:, i] for i in 1:m])
end
# every n-sized operand of one call must live on the same side (`loc` is one flag): bring A where `like` lives
_colocate_mat(A::Array, like::Array) = A
_colocate_mat(A, like::Array) = Array(A)
_colocate_mat(A::Array, like) = copyto!(_similar(like, size(A)...), A)
_colocate_mat(A, like) = A

# ---- caller-supplied column scales (multiblock PLSR, src/mbplsr.jl:77-113) and column statistics
"Weighted column means and uncorrected stds from the device (`colmean`, `colstd`: src/utility.jl:193-195,312-323)."
function col_stats(X, weights = nothing; ctx = default_ctx())
    X = _in(X); n, p = size(X); m = zeros(p); s = zeros(p)
    weights = _w(weights, X)
    GC.@preserve X weights check(ctx, ccall((:jch_col_stats, LIB), Int32,
        (Ptr{Cvoid}, Int32, Ptr{Float64}, Int64, Int64, Int64, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}),
        ctx.h, _loc(X), pointer(X), n, p, stride(X, 2), weights === nothing ? Ptr{Float64}(C_NULL) : pointer(weights), m, s))
    (means = m, stds = s)
end

"`plskern` with column divisors handed in (X centred by its weighted means, divided by `xscales`; Y by `yscales`)."
function plskern_scaled(X, Y, xscales::Vector{Float64}, yscales = nothing, weights = nothing; nlv, ctx = default_ctx())
    X = _in(X); Y = _in(Y); n, p = size(X); q = size(Y, 2); kmax = max(1, min(n, p, nlv))
    weights = _w(weights, X)
    T = _similar(X, n, kmax); wn = _similar(X, n)
    P = zeros(p, kmax); R = zeros(p, kmax); W = zeros(p, kmax); C = zeros(q, kmax); TT = zeros(kmax)
    xm = zeros(p); xs = zeros(p); ym = zeros(q); ys = zeros(q); got = Ref{Int32}(0)
    desc = Ref(PlsDesc(n, p, q, nlv, 0, 0, _loc(X), 0, 0))
    GC.@preserve X Y weights yscales T wn check(ctx, ccall((:jch_plskern_fit_scaled, LIB), Int32,
        (Ptr{Cvoid}, Ref{PlsDesc}, Ptr{Cvoid}, Int64, Ptr{Cvoid}, Int64, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64},
         Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64},
         Ptr{Float64}, Ptr{Float64}, Ref{Int32}),
        ctx.h, desc, pointer(X), stride(X, 2), pointer(Y), max(stride(Y, 2), n),
        weights === nothing ? Ptr{Float64}(C_NULL) : pointer(weights), xscales,
        yscales === nothing ? Ptr{Float64}(C_NULL) : pointer(yscales), pointer(T), P, R, W, C, TT, xm, xs, ym, ys, pointer(wn), got))
    k = Int(got[])
    cut(A) = k == size(A, 2) ? A : A[:, 1:k]
    _record(cut(T), cut(P), cut(R), cut(W), cut(C), k == length(TT) ? TT : TT[1:k], xm, xs, ym, ys, wn, nothing)
end

# ---- scores from device-side sums (src/scores.jl) ---------------------------------------------------------------------------
# sums[:, c] = (sum e, sum e^2, sum y e, sum y, sum y^2, rows) of prediction column c = level * q + j over the rows with mask != 0
function _score_sums(pred, Y, mask, ctx)
    pred = _in(pred); Y = _colocate_mat(_in(Y), pred)
    m, ncol = size(pred); q = size(Y, 2)
    (size(Y, 1) == m && ncol % q == 0) || throw(DimensionMismatch("predictions are $m x $ncol, Y is $(size(Y, 1)) x $q"))
    mask = mask === nothing ? nothing : _colocate(vec(Float64.(Array(mask))), pred)
    sums = zeros(6, ncol)
    GC.@preserve pred Y mask check(ctx, ccall((:jch_score_sums, LIB), Int32,
        (Ptr{Cvoid}, Int32, Ptr{Float64}, Int64, Int64, Int64, Ptr{Float64}, Int64, Int64, Ptr{Float64}, Ptr{Float64}),
        ctx.h, _loc(pred), pointer(pred), m, ncol, stride(pred, 2), pointer(Y), q, max(stride(Y, 2), m),
        mask === nothing ? Ptr{Float64}(C_NULL) : pointer(mask), sums))
    reshape(sums, 6, q, ncol ÷ q)            # [stat, response, level]
end

# the same sums for the predictions with nlv = lo..hi latent variables straight from the rows' scores T (m x k): running sums over the
# score columns inside the library (jch_score_sums_lv) — the m x (levels q) prediction matrix is never formed
function _score_sums_lv(T, fm, Y, mask, rng, ctx)
    T = _in(T); Y = _colocate_mat(_in(Y), T)
    m = size(T, 1); q = size(Y, 2); k = min(size(T, 2), size(fm.C, 2))
    (size(Y, 1) == m && size(fm.C, 1) == q) || throw(DimensionMismatch("scores are $m x $(size(T, 2)), Y is $(size(Y, 1)) x $q"))
    mask = mask === nothing ? nothing : _colocate(vec(Float64.(Array(mask))), T)
    lo, hi = first(rng), last(rng)
    Cm = Matrix{Float64}(fm.C[:, 1:k]); ym = Vector{Float64}(vec(fm.ymeans)); ys = Vector{Float64}(vec(fm.yscales))
    sums = zeros(6, (hi - lo + 1) * q)
    GC.@preserve T Y mask Cm ym ys check(ctx, ccall((:jch_score_sums_lv, LIB), Int32,
        (Ptr{Cvoid}, Int32, Ptr{Float64}, Int64, Int64, Int64, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Int64, Int64,
         Ptr{Float64}, Int32, Int32, Ptr{Float64}),
        ctx.h, _loc(T), pointer(T), m, k, max(stride(T, 2), m), pointer(Cm), pointer(ym), pointer(ys), pointer(Y), q, max(stride(Y, 2), m),
        mask === nothing ? Ptr{Float64}(C_NULL) : pointer(mask), lo, hi, sums))
    reshape(sums, 6, q, hi - lo + 1)         # [stat, response, level]
end

# one score from the sums: levels x q  (formulas: src/scores.jl:25-32,54-62,155-158,190-196,268,426-429)
function _score_from_sums(name::Symbol, S)
    se, see, sye, sy, syy, cnt = (permutedims(S[i, :, :]) for i in 1:6)
    name === :ssr && return see
    name === :msep && return see ./ cnt
    name === :rmsep && return sqrt.(see ./ cnt)
    name === :bias && return -se ./ cnt
    name === :r2 && return 1 .- (see ./ cnt) ./ (syy ./ cnt .- (sy ./ cnt) .^ 2)
    if name === :cor2
        sp = sy .- se; spp = syy .- 2 .* sye .+ see; spy = syy .- sye          # sums of pred, pred^2, pred * y
        cv = spy ./ cnt .- (sp ./ cnt) .* (sy ./ cnt)
        return cv .^ 2 ./ ((spp ./ cnt .- (sp ./ cnt) .^ 2) .* (syy ./ cnt .- (sy ./ cnt) .^ 2))
    end
    error("unknown score $name")
end

"A score of src/scores.jl as a callable: `rmsep(pred, Y)` -> 1 x q; the grid functions recognise it and use device-side sums."
struct ScoreFun
    name::Symbol
end
(s::ScoreFun)(pred, Y; ctx = default_ctx()) = _score_from_sums(s.name, _score_sums(pred, Y, nothing, ctx))[1:1, :]
const msep = ScoreFun(:msep); const rmsep = ScoreFun(:rmsep); const ssr = ScoreFun(:ssr)
const bias = ScoreFun(:bias); const r2 = ScoreFun(:r2); const cor2 = ScoreFun(:cor2)

# ---- grids (src/gridscore.jl, src/gridcv.jl, src/mpar.jl, src/segm.jl) ---------------------------------------------------------
"`mpar(; kwargs...)` — src/mpar.jl:15-24: all combinations of the parameter values (first keyword fastest), as a NamedTuple of vectors."
function mpar(; kwargs...)
    nam = keys(kwargs); vals = [v isa AbstractVector || v isa AbstractRange || v isa Tuple ? collect(v) : [v] for v in values(kwargs)]
    combs = vec(collect(Iterators.product(vals...)))
    NamedTuple{Tuple(nam)}(Tuple([c[i] for c in combs] for i in 1:length(nam)))
end
"`segmkf(n, K; rep = 1)` — src/segm.jl:44-57."
function segmkf(n::Integer, K::Integer; rep = 1)
    map(1:rep) do _
        perm = _randperm(n)
        [sort(perm[j:K:n]) for j in 1:K]
    end
end
"`segmts(n, m; rep = 1)` — src/segm.jl:135-149."
segmts(n::Integer, m::Integer; rep = 1) = [[sort(_randperm(n)[1:m])] for _ in 1:rep]
_randperm(n) = sortperm(rand(n))
_nlv_range(nlv, p) = max(0, minimum(nlv)):min(p, maximum(nlv))
_pars_rows(pars) = pars === nothing ? [NamedTuple()] : [NamedTuple{keys(pars)}(Tuple(v[i] for v in values(pars))) for i in 1:length(first(values(pars)))]

# m x (length(rng) * q) predictions [pred_rng[1] | pred_rng[2] | ...] (rng contiguous, src/plskern.jl:228): one library call
_pred_matrix(fm, X, rng, ctx) = _predict_range(fm, X, first(rng), min(last(rng), _nlv_fit(fm)), ctx)

# Columns of the reference's result table, in its order (src/gridscore.jl:196-220: `hcat(dat, res)` with dat = the `pars` columns,
# each combination repeated le_nlv times, then `nlv`; res = y1 ... yq), rows combination-major.
function _grid_cols(pars, rng, res::AbstractMatrix)
    rows = _pars_rows(pars)
    cols = NamedTuple()
    if pars !== nothing
        cols = NamedTuple{keys(pars)}(Tuple([r[nm] for r in rows for _ in rng] for nm in keys(pars)))
    end
    cols = merge(cols, (nlv = repeat(collect(rng), length(rows)),))
    merge(cols, NamedTuple{_ynames(size(res, 2))}(Tuple(res[:, j] for j in 1:size(res, 2))))
end

"""
    gridscorelv(Xtrain, Ytrain, X, Y; score, fun, nlv, pars = nothing, verbose = false)

src/gridscore.jl:167-221: one fit at `maximum(nlv)` per parameter combination, the predictions of the whole nlv range from ONE
pass over `X`, the scores from device-side sums.  Returns what the reference returns (:196-220): a `DataFrame` with the columns
`<pars...>, nlv, y1 ... yq`, one row per (combination, nlv), combination-major — as a NamedTuple of those columns when DataFrames
is not loaded.
"""
function gridscorelv(Xtrain, Ytrain, X, Y; score, fun, nlv, pars = nothing, verbose = false, ctx = default_ctx())
    pars === nothing || !(:nlv in keys(pars)) || error("Argument `pars` must not contain `nlv`")
    rng = _nlv_range(nlv, size(ensure_mat(Xtrain), 2))
    verbose && println(pars === nothing ? "-- Nb. combinations = 0." : "-- Nb. combinations = $(length(_pars_rows(pars)))")
    blocks = Matrix{Float64}[]
    for kw in _pars_rows(pars)
        verbose && pars !== nothing && println(pairs(kw)...)
        fm = fun(Xtrain, Ytrain; nlv = maximum(rng), kw...)
        if score isa ScoreFun && hasproperty(fm, :TT) && !hasproperty(fm, :lev)
            kmax = min(maximum(rng), _nlv_fit(fm))
            push!(blocks, kmax == 0 ? _score_from_sums(score.name, _score_sums(_pred_matrix(fm, X, rng, ctx), Y, nothing, ctx)) :
                          _score_from_sums(score.name, _score_sums_lv(transform(fm, X; nlv = kmax, ctx = ctx), fm, Y, nothing, rng, ctx)))
        else                                   # any score(pred, Y) / any model with a `predict`
            pr = predict(fm, X; nlv = rng).pred
            pr = length(rng) == 1 ? [pr] : pr
            push!(blocks, reduce(vcat, [reshape(collect(score(z, Y)), 1, :) for z in pr]))
        end
    end
    verbose && println("-- End.")
    _table(_grid_cols(pars, rng, reduce(vcat, blocks)))
end

"""
    gridcvlv(X, Y; segm, score, fun, nlv, pars = nothing, verbose = false)

src/gridcv.jl:187-228.  The reference copies `rmrow(X, s)` for every segment; here X stays where it is: each fold is ONE
weighted fit with weight 0 on the held-out rows (same means, X'DY and loadings as the fit on the remaining rows), whose scores on
the held-out rows already are their transformed rows, so the predictions for every nlv are running sums over the n x nlv scores.
`score`: one of `msep, rmsep, ssr, bias, r2, cor2`; `fun`: a PLS fit of this module taking `(X, Y, weights; nlv, ...)`.
Returns what the reference returns (:211-227): `(res = table, res_rep = table)` — `res_rep` with the columns
`repl, segm, <pars...>, nlv, y1 ... yq` (one row per replication, segment, combination and nlv), `res` the means of `y1 ... yq` over
replications and segments per `(nlv, <pars...>)` group in order of first appearance (`combine(groupby(res_rep, [:nlv; pars...]), mean)`);
DataFrames when that package is loaded, NamedTuples of the same columns otherwise.
"""
function gridcvlv(X, Y; segm, score, fun, nlv, pars = nothing, verbose = false, ctx = default_ctx())
    score isa ScoreFun || error("gridcvlv: score must be one of msep, rmsep, ssr, bias, r2, cor2")
    pars === nothing || !(:nlv in keys(pars)) || error("Argument `pars` must not contain `nlv`")
    X = _in(X); Y = _colocate_mat(_in(Y), X); n, p = size(X); q = size(Y, 2)
    rng = _nlv_range(nlv, p)
    _same_x[] = Int32(0)                                   # the FIRST fit of the call makes no promise about the workspace
    res_rep = Vector{Vector{Matrix{Float64}}}()
    for (i, listsegm) in enumerate(segm)
        verbose && print("/ repl=", i, " ")
        zres = Matrix{Float64}[]
        for (j, s) in enumerate(listsegm)
            verbose && print("segm=", j, " ")
            held = zeros(n); held[s] .= 1.0
            w = 1.0 .- held
            kfit = min(maximum(rng), n - length(s))                # the reference clamps with the TRAINING rows
            blocks = Matrix{Float64}[]
            for kw in _pars_rows(pars)
                fm = try fun(X, Y, w; nlv = kfit, kw...) catch; _same_x[] = Int32(0); rethrow() end
                _same_x[] = Int32(8)                       # every later fit of this call sees the same X (JCH_REUSE_XCOPY)
                # pred_a = ymeans + sum_{l <= min(a, k)} T_l (C_l .* yscales)' on the held-out rows, level by level inside the library
                push!(blocks, _score_from_sums(score.name, _score_sums_lv(fm.T, fm, Y, held, rng, ctx)))
            end
            push!(zres, reduce(vcat, blocks))
        end
        push!(res_rep, zres)
    end
    _same_x[] = Int32(0)
    verbose && println("/ End.")
    # res_rep: per replication the segments' tables stacked, behind the columns repl, segm (src/gridcv.jl:211-222)
    per = length(rng) * length(_pars_rows(pars))                    # rows per fold
    foldcols = [_grid_cols(pars, rng, z) for zres in res_rep for z in zres]
    repl = reduce(vcat, [fill(i, per * length(zres)) for (i, zres) in enumerate(res_rep)])
    segmc = reduce(vcat, [repeat(1:length(zres), inner = per) for zres in res_rep])
    stacked = NamedTuple{keys(first(foldcols))}(Tuple(reduce(vcat, [c[nm] for c in foldcols]) for nm in keys(first(foldcols))))
    rep_cols = merge((repl = repl, segm = segmc), stacked)
    # res: groupby(res_rep, [:nlv; keys(pars)...]) in order of first appearance = the row order of one fold, means of y1 ... yq (:223-226)
    allfolds = reduce(vcat, res_rep)
    g1 = _grid_cols(pars, rng, sum(allfolds) ./ length(allfolds))
    gkeys = pars === nothing ? (:nlv,) : (:nlv, keys(pars)...)
    res_cols = merge(NamedTuple{gkeys}(Tuple(g1[nm] for nm in gkeys)), NamedTuple{_ynames(q)}(Tuple(g1[nm] for nm in _ynames(q))))
    (res = _table(res_cols), res_rep = _table(rep_cols))
end

# ---- PLSR-DA (src/plsrda.jl) -----------------------------------------------------------------------------------------------------
struct Plsrda                     # fallback record, fields of the reference's struct (src/plsrda.jl:1-5)
    fm; lev; ni
end
"`dummy(y)` — src/utility.jl:509-519: `(Y = n x nlev 0/1 table, lev = sorted levels)`."
function dummy(y)
    y = vec(Array(y)); lev = sort(unique(y))
    (Y = Float64.(y .== permutedims(lev)), lev = lev)
end
"`plsrda(X, y, weights = ones(n); nlv, scal = false)` — src/plsrda.jl:71-77: `plskern` on the dummy table of the classes."
function plsrda(X, y, weights = nothing; nlv, scal = false, ctx = default_ctx())
    res = dummy(y); yv = vec(Array(y))
    ni = [count(==(l), yv) for l in res.lev]
    X = _in(X)
    fm = plskern(X, _colocate_mat(res.Y, X), weights; nlv = nlv, scal = scal, ctx = ctx)
    J = jchemo_module()
    (J !== nothing && fm isa getfield(J, :Plsr)) ? Base.invokelatest(getfield(J, :Plsrda), fm, res.lev, ni) : Plsrda(fm, res.lev, ni)
end
# `predict(object::Plsrda, X; nlv)` — src/plsrda.jl:95-120
function _predict_plsrda(object, X, nlv, ctx)
    a = _nlv_fit(object.fm)
    rng = nlv === nothing ? (a:a) : (max(minimum(nlv), 0):min(maximum(nlv), a))
    post = predict(object.fm, X; nlv = rng, ctx = ctx).pred
    posts = length(rng) == 1 ? [post] : post
    preds = [reshape(object.lev[[argmax(view(Array(z), i, :)) for i in 1:size(z, 1)]], :, 1) for z in posts]
    length(rng) == 1 ? (pred = preds[1], posterior = posts[1]) : (pred = preds, posterior = posts)
end

# ---- multiblock PLSR (src/mbplsr.jl, src/mbplswest.jl:220-254) ------------------------------------------------------------------
struct Mbplsr                     # fields of the reference's struct (src/mbplsr.jl:1-12)
    fm; T; R; C; bscales; xmeans; xscales; ymeans; yscales; weights
end
_hcat(Xbl) = reduce(hcat, [_in(b) for b in Xbl])
"""
    mbplsr(Xbl, Y, weights = ones(n); nlv, bscal = "none", scal = false)

src/mbplsr.jl:64-113.  The reference materialises every centred / scaled / block-scaled block; here the blocks are concatenated
RAW and the whole scaling is ONE vector of column divisors (column std x block scale) handed to `jch_plskern_fit_scaled`.
"""
function mbplsr(Xbl, Y, weights = nothing; nlv, bscal = "none", scal = false, ctx = default_ctx())
    bscal in ("none", "frob") || error("bscal must be \"none\" or \"frob\"")
    X = _hcat(Xbl); Y = _colocate_mat(_in(Y), X)
    widths = [size(ensure_mat(b), 2) for b in Xbl]; edges = cumsum([0; widths])
    st = col_stats(X, weights; ctx = ctx)
    blk(v, k) = v[edges[k] + 1:edges[k + 1]]
    xscales = [scal ? blk(st.stds, k) : ones(widths[k]) for k in 1:length(widths)]
    bscales = bscal == "frob" ? [sqrt(sum((blk(st.stds, k) ./ xscales[k]) .^ 2)) for k in 1:length(widths)] : ones(length(widths))
    div = reduce(vcat, [xscales[k] .* bscales[k] for k in 1:length(widths)])
    ysd = scal ? col_stats(Y, weights; ctx = ctx).stds : nothing
    fm = plskern_scaled(X, Y, div, ysd, weights; nlv = nlv, ctx = ctx)
    xmeans = [blk(fm.xmeans, k) for k in 1:length(widths)]
    # the reference's inner fit sees pre-scaled data with scal = false: its record carries zero means and unit scales
    inner = _record(fm.T, fm.P, fm.R, fm.W, fm.C, fm.TT, zero(fm.xmeans), one.(fm.xscales), zero(fm.ymeans), one.(fm.yscales), fm.weights, nothing)
    Mbplsr(inner, fm.T, fm.R, fm.C, bscales, xmeans, xscales, copy(fm.ymeans), copy(fm.yscales), fm.weights)
end
# `transform(object::Mbplsr, Xbl; nlv)` — src/mbplswest.jl:220-231 as one device GEMM on the raw concatenation
function _transform_mbplsr(object, Xbl, nlv, ctx)
    a = size(object.R, 2); k = nlv === nothing ? a : min(nlv, a)
    div = reduce(vcat, [object.xscales[i] .* object.bscales[i] for i in 1:length(object.xscales)])
    _affine(_hcat(Xbl), reduce(vcat, object.xmeans), div, object.R[:, 1:k], nothing, ctx)
end
# `predict(object::Mbplsr, Xbl; nlv)` — src/mbplswest.jl:239-254: ymeans .+ T[:, 1:nlv] * C[:, 1:nlv]' (no `yscales`, as the reference)
function _predict_mbplsr(object, Xbl, nlv, ctx)
    a = size(object.R, 2); q = size(object.C, 1)
    rng = nlv === nothing ? (a:a) : (max(0, minimum(nlv)):min(a, maximum(nlv)))
    T = _transform_mbplsr(object, Xbl, nothing, ctx)
    Bc = zeros(a, length(rng) * q)
    for (i, k) in enumerate(rng)
        k > 0 && (Bc[1:k, (i - 1) * q + 1:i * q] = object.C[:, 1:k]')
    end
    out = _affine(T, nothing, nothing, Bc, repeat(object.ymeans, length(rng)), ctx)
    preds = [out[:, (i - 1) * q + 1:i * q] for i in 1:length(rng)]
    (pred = length(rng) == 1 ? preds[1] : preds,)
end

# ---- vip / xfit / xresid (src/vip.jl:62-107, src/xfit.jl:37-93) ---------------------------------------------------------------
"`vip(object; nlv)` — src/vip.jl:62-89: from W, C and TT = t'Dt (p x nlv host glue)."
function vip(object; nlv = nothing)
    a = _nlv_fit(object); p = size(object.W, 1); k = nlv === nothing ? a : min(nlv, a)
    W2 = object.W[:, 1:k] .^ 2
    sst = vec(sum(object.C[:, 1:k] .^ 2, dims = 1)) .* object.TT[1:k]          # tr(C_a C_a') t_a'D t_a
    A = vec(sum(sst' .* W2, dims = 2))
    (imp = sqrt.(A ./ (sum(sst) / p)), W2 = W2, sst = sst)
end
"`vip(object, Y; nlv)` — src/vip.jl:91-107: the redundancies rd(Y, T, weights) from ONE weighted covariance of [Y | T] on the device."
function vip(object, Y; nlv = nothing, ctx = default_ctx())
    a = _nlv_fit(object); p = size(object.W, 1); k = nlv === nothing ? a : min(nlv, a)
    T = object.T[:, 1:k]; Y = _colocate_mat(_in(Y), T); q = size(Y, 2)
    A_ = hcat(Y, T); n = size(A_, 1); w = _colocate(object.weights, A_)
    S = zeros(q + k, q + k)
    GC.@preserve A_ w check(ctx, ccall((:jch_weighted_cov, LIB), Int32,
        (Ptr{Cvoid}, Int32, Ptr{Float64}, Int64, Int64, Int64, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}),
        ctx.h, _loc(A_), pointer(A_), n, q + k, stride(A_, 2), pointer(w), S, Ptr{Float64}(C_NULL)))
    # rd(Y, T, weights) (src/angles.jl:97-105): mean over the responses of the squared weighted correlations cor(y_j, t_a)^2
    cyt = S[1:q, q + 1:q + k]; vy = diag(S)[1:q]; vt = diag(S)[q + 1:q + k]
    rdd = vec(sum(cyt .^ 2 ./ (vy .* vt'), dims = 1)) ./ q
    W2 = object.W[:, 1:k] .^ 2
    Aimp = vec(sum(rdd' .* W2, dims = 2))
    (imp = sqrt.(Aimp ./ (sum(rdd) / p)), W2 = W2, rdd = rdd)
end
# the record xfit / xresid read P, xmeans and xscales from (a Pcr stands for its fm_pca, src/xfit.jl:40) and its R with T = cscale(X) R (a Pca: P)
_xmodel(object) = hasproperty(object, :fm_pca) ? _xmodel(object.fm_pca) : (object, hasproperty(object, :R) ? object.R : object.P)
"`xfit(object::Union{Pca, Pcr, Plsr}, X; nlv)` — src/xfit.jl:37-56: the scores pass over X, then a GEMM on the m x nlv scores, original scale."
function xfit(object, X; nlv = nothing, ctx = default_ctx())
    object, R = _xmodel(object)
    a = _nlv_fit(object); k = nlv === nothing ? a : min(nlv, a); p = size(object.P, 1)
    k == 0 && return _affine(X, nothing, nothing, zeros(p, p), object.xmeans, ctx)
    Tq = _affine(X, object.xmeans, object.xscales, R[:, 1:k], nothing, ctx)
    _affine(Tq, nothing, nothing, Matrix((object.P[:, 1:k] .* object.xscales)'), object.xmeans, ctx)
end
"`xresid(object::Union{Pca, Pcr, Plsr}, X; nlv)` — src/xfit.jl:86-93: E = X - xfit(X) = cscale(X) (I - R_k P_k') diag(xscales), one device GEMM."
function xresid(object, X; nlv = nothing, ctx = default_ctx())
    object, R = _xmodel(object)
    a = _nlv_fit(object); k = nlv === nothing ? a : min(nlv, a); p = size(object.P, 1)
    M = Matrix{Float64}(I, p, p) - R[:, 1:k] * object.P[:, 1:k]'
    _affine(X, object.xmeans, object.xscales, M .* object.xscales', nothing, ctx)
end

# ---- direct kernel PLS (src/dkplsr.jl): plskern! on a Gram matrix built on the device (include/jchemo_hip.h jch_dkplsr_*) ---------
struct Dkplsr                     # fallback record, fields of the reference's struct (src/dkplsr.jl:1-9); K is an empty matrix:
    X                             # the n x n Gram stays in the library's device workspace
    fm
    K::Matrix{Float64}
    kern
    xscales::Vector{Float64}
    yscales::Vector{Float64}
    dots
end

const _KERNS = Dict("krbf" => (Int32(0), (:gamma,)), "kpol" => (Int32(1), (:degree, :gamma, :coef0)))   # JCH_KERN_RBF / JCH_KERN_POL

# (kind, gamma, coef0, degree) of a kernel name and its keywords (defaults of src/kernels.jl:26, :59)
function _kern_args(kern, dots)
    haskey(_KERNS, kern) || throw(ArgumentError("unknown kernel \"$kern\" (krbf or kpol)"))
    kind, names = _KERNS[kern]
    for k in keys(dots)
        k in names || throw(ArgumentError("$kern: unknown keyword $k"))
    end
    (kind, Float64(get(dots, :gamma, 1)), Float64(get(dots, :coef0, 0)), Int32(get(dots, :degree, 1)))
end

function _gram(kern, X, Y, dots, ctx)
    kind, gamma, coef0, degree = _kern_args(kern, dots)
    same = X === Y
    X = _in(X); Y = same ? X : _in(Y)
    m, p = size(X); n = size(Y, 1)
    size(Y, 2) == p || throw(DimensionMismatch("X has $p columns, Y has $(size(Y, 2))"))
    K = _similar(X, m, n)
    GC.@preserve X Y K check(ctx, ccall((:jch_kernel_gram, LIB), Int32,
        (Ptr{Cvoid}, Int32, Int32, Ptr{Float64}, Int64, Int64, Ptr{Float64}, Ptr{Float64}, Int64, Int64, Ptr{Float64}, Int64, Float64,
         Float64, Int32, Ptr{Float64}, Int64),
        ctx.h, _loc(X), kind, pointer(X), m, stride(X, 2), Ptr{Float64}(C_NULL), pointer(Y), n, stride(Y, 2), Ptr{Float64}(C_NULL), p,
        gamma, coef0, degree, pointer(K), max(m, 1)))
    K
end

"`krbf(X, Y; gamma = 1)` — src/kernels.jl:26-30 on the GPU."
krbf(X, Y; gamma = 1, ctx = default_ctx()) = _gram("krbf", X, Y, (gamma = gamma,), ctx)
"`kpol(X, Y; degree = 1, gamma = 1, coef0 = 0)` — src/kernels.jl:59-70 on the GPU."
kpol(X, Y; degree = 1, gamma = 1, coef0 = 0, ctx = default_ctx()) = _gram("kpol", X, Y, (degree = degree, gamma = gamma, coef0 = coef0), ctx)

"`dkplsr(X, Y, weights; nlv, kern = \"krbf\", scal = false, kwargs...)` — src/dkplsr.jl:102-106 (on copies of X and Y)."
dkplsr(X, Y, weights = nothing; nlv, kern = "krbf", scal = false, ctx = default_ctx(), kwargs...) =
    dkplsr!(copy(_in(X)), copy(_in(Y)), weights; nlv = nlv, kern = kern, scal = scal, ctx = ctx, kwargs...)

"""`dkplsr!(X, Y, weights; nlv, kern = "krbf", scal = false, kwargs...)` — src/dkplsr.jl:108-123: with `scal`, X and Y are divided by
their weighted column stds in place; K = kern(X, X) and `plskern!(K, Y; nlv)` (no weights) run on the device (Y ends up centred, as
plskern! leaves it)."""
function dkplsr!(X, Y, weights = nothing; nlv, kern = "krbf", scal = false, ctx = default_ctx(), kwargs...)
    kind, gamma, coef0, degree = _kern_args(kern, kwargs)
    X = ensure_mat(X); Y = ensure_mat(Y)
    n, p = size(X); q = size(Y, 2)
    size(Y, 1) == n || throw(DimensionMismatch("X has $n rows, Y has $(size(Y, 1))"))
    weights = _w(weights, X)
    kmax = max(1, min(n, nlv))
    T = _similar(X, n, kmax); wn = _similar(X, n)
    P = zeros(n, kmax); R = zeros(n, kmax); W = zeros(n, kmax); C = zeros(q, kmax); TT = zeros(kmax)
    xm = zeros(n); xs = zeros(n); ym = zeros(q); ys = zeros(q); dxs = ones(p); dys = ones(q); got = Ref{Int32}(0)
    desc = Ref(PlsDesc(n, p, q, nlv, scal ? 1 : 0, 0, _loc(X), 1, 0))
    GC.@preserve X Y weights T wn check(ctx, ccall((:jch_dkplsr_fit, LIB), Int32,
        (Ptr{Cvoid}, Ref{PlsDesc}, Int32, Float64, Float64, Int32, Ptr{Cvoid}, Int64, Ptr{Cvoid}, Int64, Ptr{Float64}, Ptr{Float64},
         Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64},
         Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ref{Int32}),
        ctx.h, desc, kind, gamma, coef0, degree, pointer(X), stride(X, 2), pointer(Y), max(stride(Y, 2), n),
        weights === nothing ? Ptr{Float64}(C_NULL) : pointer(weights), Ptr{Float64}(C_NULL), pointer(T), P, R, W, C, TT, xm, xs, ym, ys,
        pointer(wn), dxs, dys, got))
    k = Int(got[])
    cut(A) = k == size(A, 2) ? A : A[:, 1:k]
    fm = _record(cut(T), cut(P), cut(R), cut(W), cut(C), k == length(TT) ? TT : TT[1:k], xm, xs, ym, ys, wn, nothing)
    J = jchemo_module()
    if J !== nothing && X isa Matrix{Float64} && fm isa getfield(J, :Plsr)
        return Base.invokelatest(getfield(J, :Dkplsr), X, fm, zeros(0, 0), kern, dxs, dys, kwargs)
    end
    Dkplsr(X, fm, zeros(0, 0), kern, dxs, dys, kwargs)
end

function _transform_dkplsr(object, X, nlv, ctx)
    kind, gamma, coef0, degree = _kern_args(object.kern, object.dots)
    fm = object.fm; a = _nlv_fit(fm)
    nlv = nlv === nothing ? a : min(nlv, a)
    X = _in(X); Xt = object.X; m, p = size(X); n = size(Xt, 1)
    out = _similar(X, m, nlv)
    R = Matrix{Float64}(fm.R); xm = Vector{Float64}(vec(fm.xmeans)); xs = Vector{Float64}(vec(fm.xscales))
    dxs = Vector{Float64}(object.xscales)
    GC.@preserve X Xt out R xm xs dxs check(ctx, ccall((:jch_dkplsr_transform, LIB), Int32,
        (Ptr{Cvoid}, Int32, Int32, Float64, Float64, Int32, Ptr{Float64}, Int64, Int64, Int64, Ptr{Float64}, Ptr{Float64}, Int64, Int64,
         Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Int32, Ptr{Float64}, Int64),
        ctx.h, _loc(X), kind, gamma, coef0, degree, pointer(X), m, p, stride(X, 2), pointer(dxs), pointer(Xt), n, stride(Xt, 2),
        pointer(xm), pointer(xs), pointer(R), nlv, pointer(out), max(m, 1)))
    out
end

function _predict_dkplsr(object, X, nlv, ctx)
    kind, gamma, coef0, degree = _kern_args(object.kern, object.dots)
    fm = object.fm; a = _nlv_fit(fm); q = size(fm.C, 1)
    rng = nlv === nothing ? (a:a) : (max(0, minimum(nlv)):min(a, maximum(nlv)))
    X = _in(X); Xt = object.X; m, p = size(X); n = size(Xt, 1)
    out = _similar(X, m, q * length(rng))
    R = Matrix{Float64}(fm.R); Cm = Matrix{Float64}(fm.C)
    xm = Vector{Float64}(vec(fm.xmeans)); xs = Vector{Float64}(vec(fm.xscales))
    ym = Vector{Float64}(vec(fm.ymeans)); ys = Vector{Float64}(vec(fm.yscales))
    dxs = Vector{Float64}(object.xscales); dys = Vector{Float64}(object.yscales)
    GC.@preserve X Xt out R Cm xm xs ym ys dxs dys check(ctx, ccall((:jch_dkplsr_predict, LIB), Int32,
        (Ptr{Cvoid}, Int32, Int32, Float64, Float64, Int32, Ptr{Float64}, Int64, Int64, Int64, Ptr{Float64}, Ptr{Float64}, Int64, Int64,
         Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Int64, Int32, Int32, Ptr{Float64},
         Ptr{Float64}, Int64),
        ctx.h, _loc(X), kind, gamma, coef0, degree, pointer(X), m, p, stride(X, 2), pointer(dxs), pointer(Xt), n, stride(Xt, 2),
        pointer(xm), pointer(xs), pointer(ym), pointer(ys), pointer(R), pointer(Cm), q, first(rng), last(rng), pointer(dys),
        pointer(out), max(m, 1)))
    pred = [out[:, (i - 1) * q + 1:i * q] for i in 1:length(rng)]
    (pred = length(rng) == 1 ? pred[1] : pred,)
end

# ---- kernel NIPALS PLS (src/kplsr.jl): one pass over the centred Gram per LV on the device (include/jchemo_hip.h jch_kplsr_*) ------
struct Kplsr                      # fallback record, fields of the reference's struct (src/kplsr.jl:1-18); Kt and DKt are empty
    X                             # matrices (the Gram stays in the library's device workspace), D holds the weight vector
    Kt::Matrix{Float64}
    T
    C::Matrix{Float64}
    U
    R
    D
    DKt::Matrix{Float64}
    vtot
    xscales::Vector{Float64}
    ymeans::Vector{Float64}
    yscales::Vector{Float64}
    weights
    kern
    dots
    iter::Vector{Int}
end

"`kplsr(X, Y, weights; nlv, kern = \"krbf\", tol = 1.5e-8, maxit = 100, scal = false, kwargs...)` — src/kplsr.jl:111-117 (on copies)."
kplsr(X, Y, weights = nothing; nlv, kern = "krbf", tol = 1.5e-8, maxit = 100, scal = false, ctx = default_ctx(), kwargs...) =
    kplsr!(copy(_in(X)), copy(_in(Y)), weights; nlv = nlv, kern = kern, tol = tol, maxit = maxit, scal = scal, ctx = ctx, kwargs...)

"""`kplsr!(X, Y, weights; nlv, kern = "krbf", tol = 1.5e-8, maxit = 100, scal = false, kwargs...)` — src/kplsr.jl:119-193: with `scal`,
X is divided by its weighted column stds in place; Y comes back centred (and scaled) and deflated, as the reference leaves it.  The
Gram, its centring and the NIPALS loop run on the device; nlv is clamped to n (the reference does not clamp)."""
function kplsr!(X, Y, weights = nothing; nlv, kern = "krbf", tol = 1.5e-8, maxit = 100, scal = false, ctx = default_ctx(), kwargs...)
    kind, gamma, coef0, degree = _kern_args(kern, kwargs)
    nlv >= 1 || throw(ArgumentError("nlv = $nlv must be >= 1"))
    maxit >= 1 || throw(ArgumentError("maxit = $maxit must be >= 1"))
    X = ensure_mat(X); Y = ensure_mat(Y)
    n, p = size(X); q = size(Y, 2)
    size(Y, 1) == n || throw(DimensionMismatch("X has $n rows, Y has $(size(Y, 1))"))
    weights = _w(weights, X)
    kmax = min(n, nlv)
    T = _similar(X, n, kmax); U = _similar(X, n, kmax); R = _similar(X, n, kmax); vt = _similar(X, 1, n); wn = _similar(X, n)
    C = zeros(q, kmax); xs = ones(p); ym = zeros(q); ys = ones(q); it = zeros(Int32, kmax); got = Ref{Int32}(0)
    desc = Ref(PlsDesc(n, p, q, nlv, scal ? 1 : 0, 0, _loc(X), 1, 0))
    GC.@preserve X Y weights T U R vt wn check(ctx, ccall((:jch_kplsr_fit, LIB), Int32,
        (Ptr{Cvoid}, Ref{PlsDesc}, Int32, Float64, Float64, Int32, Float64, Int32, Ptr{Cvoid}, Int64, Ptr{Cvoid}, Int64, Ptr{Float64},
         Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64},
         Ptr{Float64}, Ptr{Int32}, Ref{Int32}),
        ctx.h, desc, kind, gamma, coef0, degree, Float64(tol), Int32(maxit), pointer(X), stride(X, 2), pointer(Y), max(stride(Y, 2), n),
        weights === nothing ? Ptr{Float64}(C_NULL) : pointer(weights), Ptr{Float64}(C_NULL), pointer(T), pointer(U), pointer(R),
        pointer(vt), C, xs, ym, ys, pointer(wn), it, got))
    iter = Vector{Int}(it)
    J = jchemo_module()
    if J !== nothing && X isa Matrix{Float64} && T isa Matrix{Float64}
        return Base.invokelatest(getfield(J, :Kplsr), X, zeros(0, 0), T, C, U, R, wn, zeros(0, 0), vt, xs, ym, ys, wn, kern, kwargs, iter)
    end
    Kplsr(X, zeros(0, 0), T, C, U, R, wn, zeros(0, 0), vt, xs, ym, ys, wn, kern, kwargs, iter)
end

function _coef_kplsr(object, nlv)                       # src/kplsr.jl:221-228
    a = size(object.T, 2)
    nlv = nlv === nothing ? a : min(nlv, a)
    (beta = object.C[:, 1:nlv]', int = reshape(object.ymeans, 1, :))
end

function _transform_kplsr(object, X, nlv, ctx)          # src/kplsr.jl:202-212
    kind, gamma, coef0, degree = _kern_args(object.kern, object.dots)
    a = size(object.T, 2)
    nlv = nlv === nothing ? a : min(nlv, a)
    X = _in(X); Xt = object.X; m, p = size(X); n = size(Xt, 1)
    out = _similar(X, m, nlv)
    R = Matrix{Float64}(object.R); xs = Vector{Float64}(object.xscales)
    w = Vector{Float64}(vec(object.weights)); vt = Vector{Float64}(vec(object.vtot))
    GC.@preserve X Xt out R xs w vt check(ctx, ccall((:jch_kplsr_transform, LIB), Int32,
        (Ptr{Cvoid}, Int32, Int32, Float64, Float64, Int32, Ptr{Float64}, Int64, Int64, Int64, Ptr{Float64}, Ptr{Float64}, Int64, Int64,
         Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Int32, Ptr{Float64}, Int64),
        ctx.h, _loc(X), kind, gamma, coef0, degree, pointer(X), m, p, stride(X, 2), pointer(xs), pointer(Xt), n, stride(Xt, 2),
        pointer(w), pointer(vt), pointer(R), nlv, pointer(out), max(m, 1)))
    out
end

function _predict_kplsr(object, X, nlv, ctx)            # src/kplsr.jl:238-250
    kind, gamma, coef0, degree = _kern_args(object.kern, object.dots)
    a = size(object.T, 2); q = size(object.C, 1)
    rng = nlv === nothing ? (a:a) : (max(0, minimum(nlv)):min(a, maximum(nlv)))
    X = _in(X); Xt = object.X; m, p = size(X); n = size(Xt, 1)
    out = _similar(X, m, q * length(rng))
    R = Matrix{Float64}(object.R); Cm = Matrix{Float64}(object.C); xs = Vector{Float64}(object.xscales)
    w = Vector{Float64}(vec(object.weights)); vt = Vector{Float64}(vec(object.vtot))
    ym = Vector{Float64}(vec(object.ymeans)); ys = Vector{Float64}(vec(object.yscales))
    GC.@preserve X Xt out R Cm xs w vt ym ys check(ctx, ccall((:jch_kplsr_predict, LIB), Int32,
        (Ptr{Cvoid}, Int32, Int32, Float64, Float64, Int32, Ptr{Float64}, Int64, Int64, Int64, Ptr{Float64}, Ptr{Float64}, Int64, Int64,
         Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Int64, Int32, Int32, Ptr{Float64}, Int64),
        ctx.h, _loc(X), kind, gamma, coef0, degree, pointer(X), m, p, stride(X, 2), pointer(xs), pointer(Xt), n, stride(Xt, 2),
        pointer(w), pointer(vt), pointer(ym), pointer(ys), pointer(R), pointer(Cm), q, first(rng), last(rng), pointer(out), max(m, 1)))
    pred = [out[:, (i - 1) * q + 1:i * q] for i in 1:length(rng)]
    (pred = length(rng) == 1 ? pred[1] : pred,)
end

# ---- kernel PCA (src/kpca.jl): block subspace iteration on the centred Gram on the device (include/jchemo_hip.h jch_kpca_fit) ------
struct Kpca                       # fallback record, fields of the reference's struct (src/kpca.jl:1-15), then the eigensolver's
    X                             # report; Kt and DKt are empty matrices (the Gram stays in the library's device workspace), D
    Kt::Matrix{Float64}           # holds the weight vector, sv / eig the nlv leading values (the reference keeps all n)
    T
    P
    sv::Vector{Float64}
    eig::Vector{Float64}
    D
    DKt::Matrix{Float64}
    vtot
    xscales::Vector{Float64}
    weights
    kern
    dots
    sstot::Float64
    niter::Int
    resid::Vector{Float64}
    converged::Bool
end

"""`kpca(X, weights; nlv, kern = "krbf", scal = false, kwargs...)` — src/kpca.jl:82-115 on a copy of X: the nlv leading eigenpairs of
Kd = sqrtD Kc sqrtD come from block subspace iteration on the device (`eig_tol`, `eig_maxit`) instead of the full svd(Kd).  A fit
that did not converge warns and returns what it has."""
function kpca(X, weights = nothing; nlv, kern = "krbf", scal = false, ctx = default_ctx(), eig_tol = 1e-10, eig_maxit = 300, kwargs...)
    kind, gamma, coef0, degree = _kern_args(kern, kwargs)
    nlv >= 1 || throw(ArgumentError("nlv = $nlv must be >= 1"))
    eig_maxit >= 1 || throw(ArgumentError("eig_maxit = $eig_maxit must be >= 1"))
    eig_tol > 0 || throw(ArgumentError("eig_tol = $eig_tol must be > 0"))
    X = copy(_in(X))
    n, p = size(X)
    weights = _w(weights, X)
    weights === nothing || length(weights) == n || throw(DimensionMismatch("weights has $(length(weights)) entries, X has $n rows"))
    kmax = min(n, nlv)
    T = _similar(X, n, kmax); P = _similar(X, n, kmax); vt = _similar(X, 1, n); wn = _similar(X, n)
    xs = ones(p); sv = zeros(kmax); eig = zeros(kmax); res = zeros(kmax); sst = Ref{Float64}(0.0); nit = Ref{Int32}(0); got = Ref{Int32}(0)
    GC.@preserve X weights T P vt wn check(ctx, ccall((:jch_kpca_fit, LIB), Int32,
        (Ptr{Cvoid}, Int32, Int32, Float64, Float64, Int32, Ptr{Float64}, Int64, Int64, Int64, Ptr{Float64}, Int32, Int32, Float64, Int32,
         Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ref{Float64},
         Ref{Int32}, Ptr{Float64}, Ref{Int32}),
        ctx.h, _loc(X), kind, gamma, coef0, degree, pointer(X), n, p, stride(X, 2),
        weights === nothing ? Ptr{Float64}(C_NULL) : pointer(weights), Int32(nlv), Int32(scal ? 1 : 0), Float64(eig_tol), Int32(eig_maxit),
        Ptr{Float64}(C_NULL), pointer(T), pointer(P), pointer(vt), pointer(wn), xs, sv, eig, sst, nit, res, got))
    conv = all(res .<= eig_tol * eig[1])
    conv || @warn "kpca: the subspace iteration did not converge in $(nit[]) iterations" maxresid = maximum(res) tol = eig_tol * eig[1]
    Kpca(X, zeros(0, 0), T, P, sv, eig, wn, zeros(0, 0), vt, xs, wn, kern, kwargs, sst[], Int(nit[]), res, conv)
end

"`transform(object::Kpca, X; nlv)` — src/kpca.jl:123-132: Kc_new P[:, 1:nlv], which is jch_kplsr_transform with R = P."
function transform(object::Kpca, X; nlv = nothing, ctx = default_ctx())
    kind, gamma, coef0, degree = _kern_args(object.kern, object.dots)
    a = size(object.T, 2)
    nlv = nlv === nothing ? a : min(nlv, a)
    X = _in(X); Xt = object.X; m, p = size(X); n = size(Xt, 1)
    out = _similar(X, m, nlv)
    P = Matrix{Float64}(object.P); xs = Vector{Float64}(object.xscales)
    w = Vector{Float64}(vec(object.weights)); vt = Vector{Float64}(vec(object.vtot))
    GC.@preserve X Xt out P xs w vt check(ctx, ccall((:jch_kplsr_transform, LIB), Int32,
        (Ptr{Cvoid}, Int32, Int32, Float64, Float64, Int32, Ptr{Float64}, Int64, Int64, Int64, Ptr{Float64}, Ptr{Float64}, Int64, Int64,
         Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Int32, Ptr{Float64}, Int64),
        ctx.h, _loc(X), kind, gamma, coef0, degree, pointer(X), m, p, stride(X, 2), pointer(xs), pointer(Xt), n, stride(Xt, 2),
        pointer(w), pointer(vt), pointer(P), nlv, pointer(out), max(m, 1)))
    out
end

"""`summary(object::Kpca)` — src/kpca.jl:138-147: explvarx (lv, var = tt, pvar = tt / sstot, cumpvar), tt = colsum(D T^2) from the
device's weighted column statistics of T (tt = std^2 + mean^2).  sstot is only known for kernels that are PSD by construction."""
function Base.summary(object::Kpca; ctx = default_ctx())
    isfinite(object.sstot) || throw(ArgumentError("kpca summary: sstot (the sum of all n singular values of Kd) is only available for " *
        "kernels that are PSD by construction (krbf with gamma >= 0; kpol with gamma >= 0 and degree == 1 or coef0 >= 0)"))
    st = col_stats(object.T, object.weights; ctx = ctx)
    tt = st.stds .^ 2 .+ st.means .^ 2
    pvar = tt ./ object.sstot
    (explvarx = _table((lv = collect(1:length(tt)), var = tt, pvar = pvar, cumpvar = cumsum(pvar))),)
end

# ---- kernel ridge regression (src/krr.jl, src/krrda.jl, gridscorelb of src/gridscore.jl:235-284): Kd stays on the device and every lb
# is one Cholesky factorisation of Kd + lb^2 I there (include/jchemo_hip.h jch_krr_fit / jch_krr_solve; DESIGN.md §13) ------------------
struct Krr                        # the reference's struct (src/krr.jl:1-17) without U, UtDY and sv (no SVD is taken): Kd = sqrtD Kc sqrtD
    X                             # (n x n, always a device array) and B = sqrtD Y take their place; `solved` caches per lb what coef
    Kd                            # computed (A, alpha = sqrtD A, df)
    B
    vtot
    lb::Float64
    xscales::Vector{Float64}
    ymeans::Vector{Float64}
    weights
    kern
    dots
    solved::Dict{Float64, Any}
end

_check_lb(lb) = (isfinite(lb) && lb > 0) ? Float64(lb) : throw(ArgumentError("lb = $lb must be finite and > 0 (Kd is singular by construction)"))

# an n x n device matrix next to X: for a host X through AMDGPU.jl, which must be loaded (Kd never goes to the host)
function _device_square(X, n)
    X isa Array || return _similar(X, n, n)
    for (id, m) in Base.loaded_modules
        id.name == "AMDGPU" && return Base.invokelatest(getfield(m, :ROCArray){Float64}, undef, n, n)
    end
    error("krr: Kd (n x n) stays on the device; load AMDGPU.jl first (`using AMDGPU`) or pass device arrays")
end

function _krr_fit!(X, Y, weights, lb, kern, scal, ctx, kwargs)
    kind, gamma, coef0, degree = _kern_args(kern, kwargs)
    lb = _check_lb(lb)
    n, p = size(X); q = size(Y, 2)
    size(Y, 1) == n || throw(DimensionMismatch("X has $n rows, Y has $(size(Y, 1))"))
    weights = _w(weights, X)
    weights === nothing || length(weights) == n || throw(DimensionMismatch("weights has $(length(weights)) entries, X has $n rows"))
    Kd = _device_square(X, n)
    B = _similar(X, n, q); vt = _similar(X, 1, n); wn = _similar(X, n)
    xs = ones(p); ym = zeros(q)
    GC.@preserve X Y weights Kd B vt wn check(ctx, ccall((:jch_krr_fit, LIB), Int32,
        (Ptr{Cvoid}, Int32, Int32, Float64, Float64, Int32, Ptr{Float64}, Int64, Int64, Int64, Ptr{Float64}, Int64, Int64, Ptr{Float64}, Int32,
         Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}),
        ctx.h, _loc(X), kind, gamma, coef0, degree, pointer(X), n, p, stride(X, 2), pointer(Y), q, max(stride(Y, 2), n),
        weights === nothing ? Ptr{Float64}(C_NULL) : pointer(weights), Int32(scal ? 1 : 0), pointer(Kd), Ptr{Float64}(C_NULL),
        pointer(B), pointer(vt), pointer(wn), xs, ym))
    Krr(X, Kd, B, vt, lb, xs, ym, wn, kern, kwargs, Dict{Float64, Any}())
end

"""`krr(X, Y, weights; lb, kern = "krbf", scal = false, kwargs...)` — src/krr.jl:122-126 on copies (X and Y are left untouched).  No
SVD is taken: the record keeps Kd on the device instead of U, UtDY and sv, and `coef` / `predict` solve per lb by Cholesky."""
function krr(X, Y, weights = nothing; lb, kern = "krbf", scal = false, ctx = default_ctx(), kwargs...)
    X = copy(_in(X))
    _krr_fit!(X, _colocate_mat(_in(Y), X), weights, lb, kern, scal, ctx, kwargs)
end
"`krr!(X, Y, weights; lb, kern, scal, kwargs...)` — src/krr.jl:128-159: with `scal`, X is divided by its column stds in place; Y is not touched."
function krr!(X, Y, weights = nothing; lb, kern = "krbf", scal = false, ctx = default_ctx(), kwargs...)
    _krr_fit!(X, Y, weights, lb, kern, scal, ctx, kwargs)
end

function _krr_solve(object::Krr, lb, want_df, ctx)
    hit = get(object.solved, lb, nothing)
    hit === nothing || (want_df && hit.df === nothing) || return hit
    n, q = size(object.B)
    A = _similar(object.X, n, q); al = _similar(object.X, n, q)
    Kd = object.Kd; B = object.B; wn = object.weights
    df = Ref{Float64}(NaN); info = Ref{Int32}(0)
    GC.@preserve Kd B wn A al check(ctx, ccall((:jch_krr_solve, LIB), Int32,
        (Ptr{Cvoid}, Int32, Ptr{Float64}, Int64, Ptr{Float64}, Int64, Ptr{Float64}, Float64, Int32, Ptr{Float64}, Ptr{Float64}, Ref{Float64},
         Ref{Int32}),
        ctx.h, _loc(object.X), pointer(Kd), n, pointer(B), q, pointer(wn), lb, Int32(want_df ? 1 : 0), pointer(A), pointer(al), df, info))
    hit = (A = A, alpha = al, df = want_df ? df[] : nothing)
    object.solved[lb] = hit
    hit
end

"""`coef(object::Krr; lb = nothing)` — src/krr.jl:168-177: `(A, int, df)` with A = (Kd + lb^2 I)^-1 sqrtD Y and df = 1 + sum eig /
(eig + lb^2), computed as 1 + n - lb^2 |L^-1|_F^2 from the Cholesky factor."""
function coef(object::Krr; lb = nothing, ctx = default_ctx())
    lb = lb === nothing ? object.lb : _check_lb(lb)
    z = _krr_solve(object, lb, true, ctx)
    (A = z.A, int = reshape(object.ymeans, 1, :), df = z.df)
end

"""`predict(object::Krr, X; lb = nothing)` — src/krr.jl:187-202: ymeans + Kc_new sqrtD A(lb); one lb gives a matrix, a collection a
vector of matrices, all from ONE pass over the Gram blocks of the new rows (jch_kplsr_transform with the alphas side by side)."""
function predict(object::Krr, X; lb = nothing, ctx = default_ctx())
    lbs = lb === nothing ? [object.lb] : [_check_lb(v) for v in lb]
    kind, gamma, coef0, degree = _kern_args(object.kern, object.dots)
    X = _in(X); Xt = object.X; m, p = size(X); n = size(Xt, 1); q = size(object.B, 2)
    size(Xt, 2) == p || throw(DimensionMismatch("X has $p columns, the model has $(size(Xt, 2))"))
    R = reduce(hcat, [Matrix{Float64}(Array(_krr_solve(object, v, false, ctx).alpha)) for v in lbs])
    k = size(R, 2)
    T = _similar(X, m, k)
    xs = Vector{Float64}(object.xscales); w = Vector{Float64}(vec(object.weights)); vt = Vector{Float64}(vec(object.vtot))
    GC.@preserve X Xt T R xs w vt check(ctx, ccall((:jch_kplsr_transform, LIB), Int32,
        (Ptr{Cvoid}, Int32, Int32, Float64, Float64, Int32, Ptr{Float64}, Int64, Int64, Int64, Ptr{Float64}, Ptr{Float64}, Int64, Int64,
         Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Int32, Ptr{Float64}, Int64),
        ctx.h, _loc(X), kind, gamma, coef0, degree, pointer(X), m, p, stride(X, 2), pointer(xs), pointer(Xt), n, stride(Xt, 2),
        pointer(w), pointer(vt), pointer(R), k, pointer(T), max(m, 1)))
    out = _affine(T, nothing, nothing, Matrix{Float64}(I, k, k), repeat(object.ymeans, length(lbs)), ctx)   # + ymeans (:198)
    pred = [out[:, (i - 1) * q + 1:i * q] for i in 1:length(lbs)]
    (pred = length(lbs) == 1 ? pred[1] : pred,)
end

"""
    gridscorelb(Xtrain, Ytrain, X, Y; score, fun, lb, pars = nothing, verbose = false)

src/gridscore.jl:235-284: one fit (at `maximum(lb)`) per parameter combination and ONE `predict` over all lb (`mlev(lb)`: the sorted
distinct values).  Returns the reference's table: the columns `<pars...>, lb, y1 ... yq`, one row per (combination, lb),
combination-major (a `DataFrame` when DataFrames is loaded).  `pars` must not contain `lb`.
"""
function gridscorelb(Xtrain, Ytrain, X, Y; score, fun, lb, pars = nothing, verbose = false, ctx = default_ctx())
    pars === nothing || !(:lb in keys(pars)) || error("Argument `pars` must not contain `lb`")
    lbs = sort(unique([_check_lb(v) for v in lb]))
    rows = _pars_rows(pars)
    verbose && println(pars === nothing ? "-- Nb. combinations = 0." : "-- Nb. combinations = $(length(rows))")
    blocks = Matrix{Float64}[]
    for kw in rows
        verbose && pars !== nothing && println(pairs(kw)...)
        fm = fun(Xtrain, Ytrain; lb = maximum(lbs), kw...)
        pr = predict(fm, X; lb = lbs).pred
        pr = length(lbs) == 1 ? [pr] : pr
        push!(blocks, reduce(vcat, [reshape(collect(score(z, Y)), 1, :) for z in pr]))
    end
    verbose && println("-- End.")
    res = reduce(vcat, blocks)
    cols = NamedTuple()
    if pars !== nothing
        cols = NamedTuple{keys(pars)}(Tuple([r[nm] for r in rows for _ in lbs] for nm in keys(pars)))
    end
    cols = merge(cols, (lb = repeat(lbs, length(rows)),))
    _table(merge(cols, NamedTuple{_ynames(size(res, 2))}(Tuple(res[:, j] for j in 1:size(res, 2)))))
end

struct Krrda                      # what the reference's `krrda` returns (its Rrda, src/krrda.jl:65)
    fm; lev; ni
end
"`krrda(X, y, weights; lb, kern = \"krbf\", scal = false, kwargs...)` — src/krrda.jl:59-66: `krr` on `dummy(y)`."
function krrda(X, y, weights = nothing; lb, kern = "krbf", scal = false, ctx = default_ctx(), kwargs...)
    res = dummy(y); yv = vec(Array(y))
    ni = [count(==(l), yv) for l in res.lev]
    X = _in(X)
    Krrda(krr(X, _colocate_mat(res.Y, X), weights; lb = lb, kern = kern, scal = scal, ctx = ctx, kwargs...), res.lev, ni)
end
"`predict(object::Krrda, X; lb)` — src/rrda.jl:79-97: `(pred, posterior)`, pred the level of the largest posterior (the first on ties)."
function predict(object::Krrda, X; lb = nothing, ctx = default_ctx())
    post = predict(object.fm, X; lb = lb, ctx = ctx).pred
    posts = post isa AbstractMatrix ? [post] : post
    preds = [reshape(object.lev[[argmax(view(Array(z), i, :)) for i in 1:size(z, 1)]], :, 1) for z in posts]
    post isa AbstractMatrix ? (pred = preds[1], posterior = posts[1]) : (pred = preds, posterior = posts)
end

# ---- row-wise spectra preprocessing (src/preprocessing.jl): snv, detrend, savgol, savgk, mavg, mavg_runmean, fdif over
# jch_rows_standardize / jch_rows_project_out / jch_rows_fir (include/jchemo_hip.h; DESIGN.md §14).  A host Array in gives an Array out, a
# device array in gives a device array out; the `!` variants work in place.  `interpl` is not provided. ----------------------------------
const _FIR_SAME = Int32(0)
const _FIR_VALID = Int32(1)

function _rows_standardize!(out, X, cent, scal, ctx)
    n, p = size(X)
    GC.@preserve X out check(ctx, ccall((:jch_rows_standardize, LIB), Int32,
        (Ptr{Cvoid}, Int32, Ptr{Float64}, Int64, Int64, Int64, Int32, Int32, Ptr{Float64}, Int64),
        ctx.h, _loc(X), pointer(X), n, p, max(stride(X, 2), n), Int32(cent ? 1 : 0), Int32(scal ? 1 : 0), pointer(out), max(stride(out, 2), n)))
    out
end

function _rows_project_out!(out, X, A::Matrix{Float64}, V::Matrix{Float64}, ctx)
    n, p = size(X); k = size(A, 1)
    GC.@preserve X out check(ctx, ccall((:jch_rows_project_out, LIB), Int32,
        (Ptr{Cvoid}, Int32, Ptr{Float64}, Int64, Int64, Int64, Ptr{Float64}, Ptr{Float64}, Int32, Ptr{Float64}, Int64),
        ctx.h, _loc(X), pointer(X), n, p, max(stride(X, 2), n), A, V, Int32(k), pointer(out), max(stride(out, 2), n)))
    out
end

function _rows_fir!(out, X, taps::Vector{Float64}, lo, mode, ctx)
    n, p = size(X)
    GC.@preserve X out check(ctx, ccall((:jch_rows_fir, LIB), Int32,
        (Ptr{Cvoid}, Int32, Ptr{Float64}, Int64, Int64, Int64, Ptr{Float64}, Int64, Int64, Int32, Ptr{Float64}, Int64),
        ctx.h, _loc(X), pointer(X), n, p, max(stride(X, 2), n), taps, length(taps), lo, mode, pointer(out), max(stride(out, 2), n)))
    out
end

"`snv(X; cent = true, scal = true)` — src/preprocessing.jl:467-471: each row minus its mean, over its uncorrected standard deviation."
function snv(X; cent = true, scal = true, ctx = default_ctx())
    X = _in(X)
    _rows_standardize!(_similar(X, size(X)...), X, cent, scal, ctx)
end
"`snv!(X; cent = true, scal = true)` — src/preprocessing.jl:473-481, in place."
function snv!(X; cent = true, scal = true, ctx = default_ctx())
    _rows_standardize!(X, X, cent, scal, ctx)
    nothing
end

# Host coefficients of `detrend`: V holds the monomials z^0 ... z^pol of z = 1 ... p (in floating point, so a large p^pol cannot wrap),
# A = pinv(V'V) V' with the cut-off sqrt(eps) on the relative singular values.  That cut-off is part of the reference's result (for
# spectra-sized p the Gram of the monomials keeps rank 2, DESIGN.md §14), so the polynomial is never re-fitted on the device.
function _detrend_coef(p, pol)
    0 <= pol <= 7 || throw(ArgumentError("detrend: pol = $pol is outside 0 ... 7 (jch_rows_project_out takes k = pol + 1 <= 8)"))
    z = range(1.0, Float64(p), length = Int(p))
    V = Float64[zi^e for zi in z, e in 0:pol]
    A = pinv(V' * V, rtol = sqrt(eps(Float64))) * V'
    Matrix{Float64}(A), V
end
"`detrend(X; pol = 1)` — src/preprocessing.jl:27-31: each row minus vX A row, with the reference's truncating pinv."
function detrend(X; pol = 1, ctx = default_ctx())
    X = _in(X)
    A, V = _detrend_coef(size(X, 2), pol)
    _rows_project_out!(_similar(X, size(X)...), X, A, V, ctx)
end
"`detrend!(X; pol = 1)` — src/preprocessing.jl:32-47, in place."
function detrend!(X; pol = 1, ctx = default_ctx())
    A, V = _detrend_coef(size(X, 2), pol)
    _rows_project_out!(X, X, A, V, ctx)
    nothing
end

"""`savgk(m, pol, d)` — the Savitzky-Golay design on the window -m ... m, on the host: `S[i, j]` is the j-th monomial at the i-th window
point, `G = S inv(S'S)` (its column d + 1 gives the d-th Taylor coefficient of the least-squares polynomial at the centre), and
`kern = d! G[:, d + 1]`.  Returns `(S, G, kern)` under the reference's names."""
function savgk(m, pol, d)
    m, pol, d = Int(m), Int(pol), Int(d)
    m < 1 && throw(ArgumentError("savgk: the half-width m = $m must be at least 1"))
    1 <= pol <= 2m || throw(ArgumentError("savgk: pol = $pol is outside 1 ... 2m = $(2m)"))
    0 <= d <= pol || throw(ArgumentError("savgk: d = $d is outside 0 ... pol = $pol"))
    S = Float64[Float64(u)^e for u in -m:m, e in 0:pol]
    G = S * inv(S' * S)        # (an explicit inverse, not a solve: bitwise the same route as preproc.py and the restatement)
    (S = S, G = G, kern = factorial(d) .* G[:, d + 1])
end

# UNPINNED reading (DESIGN.md §6): imfilter is a correlation and the reference passes reflect(centered(kern))
# (src/preprocessing.jl:430-434), so the filter is a true convolution, out[j] = sum_{u=-m}^{m} kern[u] x[j - u]: as a correlation window
# that starts at j + lo, taps = reverse(kern) and lo = -m.  (Dropping the `reverse` gives the correlation reading.)
_savgol_taps(kern) = (Vector{Float64}(reverse(kern)), -(length(kern) >> 1))
# UNPINNED reading for even f (DESIGN.md §6): centered(ones(f) / f) (src/preprocessing.jl:250) has the axes
# -((f + 1) >> 1) + 1 : f - ((f + 1) >> 1), i.e. -m:m for odd f and -f/2 + 1 : f/2 for even f; imfilter correlates.
_mavg_window(f) = (fill(1.0 / f, f), 1 - ((f + 1) >> 1))

function _savgol_args(f, pol, d)
    f = Int64(f)
    (isodd(f) && f >= 3) || throw(ArgumentError("f must be odd and >= 3"))
    _savgol_taps(savgk((f - 1) >> 1, pol, d).kern)
end
"`savgol(X; f, pol, d)` — src/preprocessing.jl:418-422: Savitzky-Golay filter of each row, replicate padding."
function savgol(X; f, pol, d, ctx = default_ctx())
    taps, lo = _savgol_args(f, pol, d)
    X = _in(X)
    _rows_fir!(_similar(X, size(X)...), X, taps, lo, _FIR_SAME, ctx)
end
"`savgol!(X; f, pol, d)` — src/preprocessing.jl:424-441, in place."
function savgol!(X; f, pol, d, ctx = default_ctx())
    taps, lo = _savgol_args(f, pol, d)
    _rows_fir!(X, X, taps, lo, _FIR_SAME, ctx)
    nothing
end

"`mavg(X; f)` — src/preprocessing.jl:241-245: moving average of each row with the centred kernel ones(f) / f, replicate padding."
function mavg(X; f, ctx = default_ctx())
    f = Int64(f)
    f >= 1 || throw(ArgumentError("f must be >= 1"))
    taps, lo = _mavg_window(f)
    X = _in(X)
    _rows_fir!(_similar(X, size(X)...), X, taps, lo, _FIR_SAME, ctx)
end
"`mavg!(X; f)` — src/preprocessing.jl:247-260, in place."
function mavg!(X; f, ctx = default_ctx())
    f = Int64(f)
    f >= 1 || throw(ArgumentError("f must be >= 1"))
    taps, lo = _mavg_window(f)
    _rows_fir!(X, X, taps, lo, _FIR_SAME, ctx)
    nothing
end

"""`mavg_runmean(X; f)` — src/preprocessing.jl:299-335: moving average without padding, (n, p) -> (n, p - f + 1), each point on the first
unit of the kernel; every output is its own f-term sum (the reference's running sum carries its rounding along the row)."""
function mavg_runmean(X; f, ctx = default_ctx())
    X = _in(X); n, p = size(X); f = Int64(f)
    1 <= f <= p || throw(ArgumentError("f = $f must agree with: 1 <= f <= p = $p"))
    _rows_fir!(_similar(X, n, p - f + 1), X, fill(1.0 / f, f), 0, _FIR_VALID, ctx)
end

"`fdif(X; f = 2)` — src/preprocessing.jl:79-93: M[:, j] = X[:, j + f - 1] - X[:, j], (n, p) -> (n, p - f + 1)."
function fdif(X; f = 2, ctx = default_ctx())
    X = _in(X); n, p = size(X); f = Int64(f)
    2 <= f <= p || throw(ArgumentError("f = $f must agree with: 2 <= f <= p = $p"))
    taps = zeros(f); taps[1] = -1.0; taps[f] = 1.0
    _rows_fir!(_similar(X, n, p - f + 1), X, taps, 0, _FIR_VALID, ctx)
end

# ---- Covsel (src/covsel.jl, src/covselr.jl) over jch_covsel_fit (include/jchemo_hip.h; DESIGN.md §15): variable selection that only READS
# X, once per selected variable.  `sel` is 1-based here, as in the reference.  Deviations: a column whose deflated sum of squares fell to
# 1e-10 of its original one is exhausted (`cor` gives it 0; a selection that lands on one stops, so a rank-deficient X yields fewer than nlv
# rows); typ = "aic" is not provided. ----------------------------------------------------------------------------------------------------
const _COVSEL_TYP = Dict("cov" => Int32(0), "cor" => Int32(1))

struct Covsel                     # what the reference's `covsel` returns (src/covsel.jl:119-121): sel (the table sel, cov2, cumpvarx,
    sel                           # cumpvary), cov2, C; then what `covselr` is computed from: the completed steps, the means and scales,
    cov2::Vector{Float64}         # G = Xc'Q (p x nlv), QtY = Q'Yc (nlv x q, units of the scaled Y) and Q (n x nlv, where X lives)
    C::Matrix{Float64}
    nlv::Int
    xmeans::Vector{Float64}
    ymeans::Vector{Float64}
    yscales::Vector{Float64}
    G::Matrix{Float64}
    QtY::Matrix{Float64}
    Q
end

struct Mlr                        # the reference's Mlr as far as `covselr` uses it (src/mlr.jl): B (nlv x q), int (1 x q), raw Y units
    B::Matrix{Float64}
    int::Matrix{Float64}
end

struct Covselr                    # src/covselr.jl:1-5
    fm
    sel
    cov2::Vector{Float64}
end

function _covsel_fit!(X, Y, nlv, typ, inplace, ctx)
    haskey(_COVSEL_TYP, typ) || throw(ArgumentError("typ = $typ: \"cov\" or \"cor\" (\"aic\" is marked not useful in the reference and is not provided)"))
    n, p = size(X); q = size(Y, 2)
    size(Y, 1) == n || throw(DimensionMismatch("X has $n rows, Y has $(size(Y, 1))"))
    nlv = nlv === nothing ? p : Int(nlv)                       # src/covsel.jl:63
    nlv >= 1 || throw(ArgumentError("nlv = $nlv must be at least 1"))
    a = min(nlv, p)
    sel = zeros(Int32, a); selcov = zeros(a); cov2 = zeros(p); Cm = zeros(p, a); cpx = zeros(a); cpy = zeros(a)
    xm = zeros(p); ym = zeros(q); ys = zeros(q); G = zeros(p, a); QtY = zeros(a, q)
    Q = _similar(X, n, a)
    done = Ref{Int32}(0)
    GC.@preserve X Y Q check(ctx, ccall((:jch_covsel_fit, LIB), Int32,
        (Ptr{Cvoid}, Int32, Ptr{Float64}, Int64, Int64, Int64, Ptr{Float64}, Int64, Int64, Int32, Int32, Int32, Ptr{Int32}, Ptr{Float64}, Ptr{Float64},
         Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ref{Int32}),
        ctx.h, _loc(X), pointer(X), n, p, max(stride(X, 2), n), pointer(Y), q, max(stride(Y, 2), n), Int32(a), _COVSEL_TYP[typ], Int32(inplace ? 1 : 0),
        sel, selcov, cov2, Cm, cpx, cpy, xm, ym, ys, G, QtY, pointer(Q), done))
    k = Int(done[])
    tab = _table((sel = Int64.(sel)[1:k] .+ 1, cov2 = selcov[1:k], cumpvarx = cpx[1:k], cumpvary = cpy[1:k]))
    Covsel(tab, cov2, Cm[:, 1:k], k, xm, ym, ys, G[:, 1:k], QtY[1:k, :], Q[:, 1:k])
end

"""`covsel(X, Y; nlv = nothing, typ = "cov")` — src/covsel.jl:54-57: X and Y are left untouched (and, unlike the reference, not copied: the
selection only reads X).  nlv = nothing selects p variables."""
function covsel(X, Y; nlv = nothing, typ = "cov", ctx = default_ctx())
    X = _in(X)
    _covsel_fit!(X, _colocate_mat(_in(Y), X), nlv, typ, false, ctx)
end
"""`covsel!(X, Y; nlv = nothing, typ = "cov")` — src/covsel.jl:59-122: X and Y end up centred (Y scaled when q > 1) and orthogonalised to
every selected column, as the reference leaves them (:112-113)."""
function covsel!(X, Y; nlv = nothing, typ = "cov", ctx = default_ctx())
    _covsel_fit!(X, Y, nlv, typ, true, ctx)
end

"""`covselr(X, Y; nlv, typ = "cov")` — src/covselr.jl:48-53: `covsel`, then the MLR of Y on the selected columns.  With Xc[:, sel] = Q R and
R[k, i] = G[sel_i, k] the coefficients are B = R^-1 Q'Yc, a nlv x nlv triangular solve on the host, rescaled by yscales to the raw Y."""
function covselr(X, Y; nlv, typ = "cov", ctx = default_ctx())
    res = covsel(X, Y; nlv = nlv, typ = typ, ctx = ctx)
    s = res.sel.sel
    R = UpperTriangular(permutedims(res.G[s, :]))
    B = (R \ res.QtY) .* res.yscales'
    int = res.ymeans' .- res.xmeans[s]' * B
    Covselr(Mlr(B, Matrix(int)), res.sel, res.cov2)
end

"`coef(object::Covselr)` — `coef(object.fm)` of the reference's Mlr: (B, int)."
coef(object::Covselr) = (B = object.fm.B, int = object.fm.int)

"`predict(object::Covselr, X)` — src/covselr.jl:61-64: int + X[:, sel] B (jch_affine_gemm on the gathered columns)."
function predict(object::Covselr, X; ctx = default_ctx())
    X = _in(X)
    s = object.sel.sel
    (pred = _affine(X[:, s], nothing, nothing, object.fm.B, vec(object.fm.int), ctx),)
end

# ---- PCA and PCR (src/pcasvd.jl, src/pcaeigen.jl, src/pcaeigenk.jl, src/pcr.jl) over jch_pca_fit (include/jchemo_hip.h; DESIGN.md §16): P and
# sv^2 are the leading eigenpairs of G = Xs'D Xs, formed in one pass over the column-major X, from kpca's block subspace iteration.  Deviations:
# the three fit names run one algorithm; sv and eig hold nlv values; `summary` does not read X; the `!` forms do not leave a centred X behind;
# the iteration needs a gap behind the block (pure-noise data ends at eig_maxit with converged = false). ----------------------------------
struct Pca                        # the reference's fields (src/pcasvd.jl:100), then what the eigen route knows
    T
    P::Matrix{Float64}
    sv::Vector{Float64}
    xmeans::Vector{Float64}
    xscales::Vector{Float64}
    weights
    niter
    conv
    eig::Vector{Float64}
    sstot::Float64
    colvar::Vector{Float64}
    resid::Vector{Float64}
    converged::Bool
end

struct Pcr                        # src/pcr.jl:96; R = P and C = beta' have the shapes of a Plsr: transform, coef and predict are the generic ones
    fm_pca
    T
    R::Matrix{Float64}
    C::Matrix{Float64}
    xmeans::Vector{Float64}
    xscales::Vector{Float64}
    ymeans::Vector{Float64}
    yscales::Vector{Float64}
    weights
end
_nlv_fit(object::Pcr) = size(object.R, 2)

function _pca_fit(who, X, Y, weights, nlv, scal, eig_tol, eig_maxit, ctx)
    nlv >= 1 || throw(ArgumentError("nlv = $nlv must be >= 1"))
    eig_maxit >= 1 || throw(ArgumentError("eig_maxit = $eig_maxit must be >= 1"))
    eig_tol > 0 || throw(ArgumentError("eig_tol = $eig_tol must be > 0"))
    X = _in(X); n, p = size(X)
    weights = _w(weights, X)
    weights === nothing || length(weights) == n || throw(DimensionMismatch("weights has $(length(weights)) entries, X has $n rows"))
    q = Y === nothing ? 0 : size(Y, 2)
    Yd = Y === nothing ? _similar(X, 1, 1) : _colocate_mat(_in(Y), X)
    q == 0 || size(Yd, 1) == n || throw(DimensionMismatch("X has $n rows, Y has $(size(Yd, 1))"))
    a = min(nlv, n, p)                                                   # src/pcasvd.jl:82
    T = _similar(X, n, a); wn = _similar(X, n)
    P = zeros(p, a); sv = zeros(a); eig = zeros(a); res = zeros(a); xm = zeros(p); xs = zeros(p); cvar = zeros(p); ym = zeros(max(q, 1)); K = zeros(p, max(q, 1))
    sst = Ref{Float64}(0.0); nit = Ref{Int32}(0); got = Ref{Int32}(0); cvg = Ref{Int32}(0)
    GC.@preserve X weights Yd T wn check(ctx, ccall((:jch_pca_fit, LIB), Int32,
        (Ptr{Cvoid}, Int32, Ptr{Float64}, Int64, Int64, Int64, Ptr{Float64}, Ptr{Float64}, Int64, Int64, Int32, Int32, Float64, Int32,
         Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ref{Float64}, Ptr{Float64}, Ptr{Float64},
         Ptr{Float64}, Ref{Int32}, Ptr{Float64}, Ref{Int32}, Ref{Int32}),
        ctx.h, _loc(X), pointer(X), n, p, max(stride(X, 2), n), weights === nothing ? Ptr{Float64}(C_NULL) : pointer(weights),
        q == 0 ? Ptr{Float64}(C_NULL) : pointer(Yd), q, max(stride(Yd, 2), n), Int32(nlv), Int32(scal ? 1 : 0), Float64(eig_tol), Int32(eig_maxit),
        pointer(T), P, sv, eig, xm, xs, pointer(wn), sst, cvar, ym, K, nit, res, got, cvg))
    conv = cvg[] != 0
    conv || @warn "$who: the subspace iteration did not converge in $(nit[]) iterations" maxresid = maximum(res) tol = eig_tol * eig[1]
    (fm = Pca(T, P, sv, xm, xs, wn, Int(nit[]), conv, eig, sst[], cvar, res, conv), ymeans = ym[1:q], xtdy = K[:, 1:q])
end

"""`pcasvd(X, weights; nlv, scal = false)` — src/pcasvd.jl:73-101 through jch_pca_fit; X is only read.  `eig_tol`, `eig_maxit`: the subspace
iteration's stopping rule; a fit that did not converge warns and returns what it has."""
function pcasvd(X, weights = nothing; nlv, scal = false, ctx = default_ctx(), eig_tol = 1e-10, eig_maxit = 300)
    _pca_fit("pcasvd", X, nothing, weights, nlv, scal, eig_tol, eig_maxit, ctx).fm
end
"`pcaeigen(X, weights; nlv, scal = false)` — src/pcaeigen.jl: the eigen-decomposition of X'DX, which is what every fit here runs."
function pcaeigen(X, weights = nothing; nlv, scal = false, ctx = default_ctx(), eig_tol = 1e-10, eig_maxit = 300)
    _pca_fit("pcaeigen", X, nothing, weights, nlv, scal, eig_tol, eig_maxit, ctx).fm
end
"`pcaeigenk(X, weights; nlv, scal = false)` — src/pcaeigenk.jl (the n x n route for n < p): the same T, P and sv from the one algorithm."
function pcaeigenk(X, weights = nothing; nlv, scal = false, ctx = default_ctx(), eig_tol = 1e-10, eig_maxit = 300)
    _pca_fit("pcaeigenk", X, nothing, weights, nlv, scal, eig_tol, eig_maxit, ctx).fm
end
# the reference's `!` forms leave the centred (scaled) X in their argument; the fit here never writes X: aliases
const pcasvd! = pcasvd
const pcaeigen! = pcaeigen
const pcaeigenk! = pcaeigenk

# ---- spatial median and spherical PCA (src/colmedspa.jl, src/pcasph.jl) over jch_spatial_median and jch_pcasph_fit (DESIGN.md §28).  Deviations:
# `maxit` bounds the Weiszfeld loop (the reference has no bound); P comes from the Gram of the projected rows, not from an SVD of a transposed copy;
# a row AT the centre gets weight 0 and a warning instead of NaN; `pcasph!` does not leave the centred X behind. ----------------------------------
"""`colmedspa(X; delta = 1e-6)` — src/colmedspa.jl:4-33 through jch_spatial_median: the spatial median of the rows of X (a host vector); X is only
read, once per Weiszfeld step.  `maxit` bounds the steps; reaching it warns and returns the last centre."""
function colmedspa(X; delta = 1e-6, maxit = 1000, ctx = default_ctx())
    delta > 0 || throw(ArgumentError("delta = $delta must be > 0"))
    maxit >= 1 || throw(ArgumentError("maxit = $maxit must be >= 1"))
    X = _in(X); n, p = size(X)
    mu = zeros(p)
    nit = Ref{Int32}(0); h = Ref{Float64}(0.0); cvg = Ref{Int32}(0)
    GC.@preserve X check(ctx, ccall((:jch_spatial_median, LIB), Int32,
        (Ptr{Cvoid}, Int32, Ptr{Float64}, Int64, Int64, Int64, Float64, Int32, Ptr{Float64}, Ptr{Float64}, Ref{Int32}, Ref{Float64}, Ref{Int32}),
        ctx.h, _loc(X), pointer(X), n, p, max(stride(X, 2), n), Float64(delta), Int32(maxit), mu, Ptr{Float64}(C_NULL), nit, h, cvg))
    cvg[] != 0 || @warn "colmedspa: no convergence in $(nit[]) steps" last_step = h[] threshold = delta * sqrt(p)
    mu
end

"""`pcasph(X, weights; nlv, typc = "medspa", delta = .001, scal = false)` — src/pcasph.jl:54-92 through jch_pcasph_fit; X is only read.  Returns a
`Pca`: sv = the MADs of the projected scores, eig = the eigenvalues of the Gram of the projected rows, sstot its trace."""
function pcasph(X, weights = nothing; nlv, typc = "medspa", delta = .001, scal = false, ctx = default_ctx(), eig_tol = 1e-10, eig_maxit = 300)
    nlv >= 1 || throw(ArgumentError("nlv = $nlv must be >= 1"))
    typc in ("medspa", "mean") || throw(ArgumentError("typc = $typc must be \"medspa\" or \"mean\""))
    delta > 0 || throw(ArgumentError("delta = $delta must be > 0"))
    eig_maxit >= 1 || throw(ArgumentError("eig_maxit = $eig_maxit must be >= 1"))
    eig_tol > 0 || throw(ArgumentError("eig_tol = $eig_tol must be > 0"))
    X = _in(X); n, p = size(X)
    weights = _w(weights, X)
    weights === nothing || length(weights) == n || throw(DimensionMismatch("weights has $(length(weights)) entries, X has $n rows"))
    a = min(nlv, n, p)                                                   # src/pcasph.jl:63
    T = _similar(X, n, a); wn = _similar(X, n)
    P = zeros(p, a); sv = zeros(a); eig = zeros(a); res = zeros(a); xm = zeros(p); xs = zeros(p); cvar = zeros(p)
    sst = Ref{Float64}(0.0); nitm = Ref{Int32}(0); cvgm = Ref{Int32}(0); nit = Ref{Int32}(0); cvg = Ref{Int32}(0); got = Ref{Int32}(0); nz = Ref{Int64}(0)
    GC.@preserve X weights T wn check(ctx, ccall((:jch_pcasph_fit, LIB), Int32,
        (Ptr{Cvoid}, Int32, Ptr{Float64}, Int64, Int64, Int64, Ptr{Float64}, Int32, Int32, Float64, Int32, Int32, Float64, Int32,
         Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ref{Float64}, Ptr{Float64},
         Ref{Int32}, Ref{Int32}, Ref{Int32}, Ptr{Float64}, Ref{Int32}, Ref{Int32}, Ref{Int64}),
        ctx.h, _loc(X), pointer(X), n, p, max(stride(X, 2), n), weights === nothing ? Ptr{Float64}(C_NULL) : pointer(weights),
        Int32(nlv), Int32(typc == "medspa" ? 0 : 1), Float64(delta), Int32(1000), Int32(scal ? 1 : 0), Float64(eig_tol), Int32(eig_maxit),
        pointer(T), P, sv, eig, xm, xs, pointer(wn), sst, cvar, nitm, cvgm, nit, res, cvg, got, nz))
    cvgm[] != 0 || @warn "pcasph: the spatial median did not converge in $(nitm[]) steps"
    nz[] == 0 || @warn "pcasph: $(nz[]) row(s) lie at the centre (norm 0): they carry no direction and got weight 0"
    conv = cvg[] != 0
    conv || @warn "pcasph: the subspace iteration did not converge in $(nit[]) iterations" maxresid = maximum(res) tol = eig_tol * eig[1]
    Pca(T, P, sv, xm, xs, wn, Int(nit[]), conv, eig, sst[], cvar, res, conv)
end
function pcasph!(X, weights = nothing; kwargs...)      # src/pcasph.jl:60 centres X in place; the fit here never writes X
    pcasph(X, weights; kwargs...)
end

"`transform(object::Pca, X; nlv)` — src/pcasvd.jl:110-115: cscale(X, xmeans, xscales) * P[:, 1:nlv] (jch_affine_gemm)."
function transform(object::Pca, X; nlv = nothing, ctx = default_ctx())
    a = size(object.P, 2)
    nlv = nlv === nothing ? a : min(nlv, a)
    size(X, 2) == size(object.P, 1) || throw(DimensionMismatch("X has $(size(X, 2)) columns, the model has $(size(object.P, 1))"))
    _affine(X, object.xmeans, object.xscales, nlv == a ? object.P : object.P[:, 1:nlv], nothing, ctx)
end

"""`summary(object::Pca, X)` — src/pcasvd.jl:123-146 from the stored quantities (X is only checked for its shape): with G = Xs'D Xs and
G P = P diag(eig), sstot = trace(G), tt = eig, coord_var = P diag(sv), cor_circle = coord_var ./ colstd(Xs), contr_var from coord_var,
contr_ind = D T.^2 ./ tt (where T lives)."""
function Base.summary(object::Pca, X)
    size(X) == (size(object.T, 1), size(object.P, 1)) || throw(DimensionMismatch("X is not the matrix the model was fitted on"))
    a = size(object.P, 2)
    tt = object.eig[1:a]
    pvar = tt ./ object.sstot
    explvarx = _table((lv = collect(1:a), var = tt, pvar = pvar, cumpvar = cumsum(pvar)))
    contr_ind = object.weights .* object.T .^ 2 ./ _colocate_mat(reshape(tt, 1, a), object.T)
    coord_var = object.P .* object.sv[1:a]'
    cor_circle = coord_var ./ (sqrt.(object.colvar) ./ object.xscales)
    cc = coord_var .^ 2
    contr_var = cc ./ sum(cc, dims = 1)
    (explvarx = explvarx, contr_ind = contr_ind, contr_var = contr_var, coord_var = coord_var, cor_circle = cor_circle)
end

"""`pcr(X, Y, weights; nlv, scal = false)` — src/pcr.jl:76-97: the PCA fit plus one pass Xs'D Yc over X; beta = diag(1 / sv^2) P' Xs'D Yc on
the host.  `coef` and `predict` (one nlv or a range, 0 = intercept only) are the generic ones."""
function pcr(X, Y, weights = nothing; nlv, scal = false, ctx = default_ctx(), eig_tol = 1e-10, eig_maxit = 300)
    r = _pca_fit("pcr", X, Y, weights, nlv, scal, eig_tol, eig_maxit, ctx)
    fm = r.fm
    beta = (fm.P' * r.xtdy) ./ fm.eig
    Pcr(fm, fm.T, fm.P, Matrix(beta'), fm.xmeans, fm.xscales, r.ymeans, ones(length(r.ymeans)), fm.weights)
end
const pcr! = pcr    # src/pcr.jl:82: X and Y are not written here

"""`xtdx(X, weights)` — (G = (X - 1 mu')' D (X - 1 mu'), mu) as host arrays: jch_xtdx, one pass over the column-major X with the means and the
weights applied in registers."""
function xtdx(X, weights = nothing; ctx = default_ctx())
    X = _in(X); n, p = size(X)
    weights = _w(weights, X)
    G = zeros(p, p); mu = zeros(p)
    GC.@preserve X weights check(ctx, ccall((:jch_xtdx, LIB), Int32,
        (Ptr{Cvoid}, Int32, Ptr{Float64}, Int64, Int64, Int64, Ptr{Float64}, Ptr{Float64}, Int64, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}),
        ctx.h, _loc(X), pointer(X), n, p, max(stride(X, 2), n), weights === nothing ? Ptr{Float64}(C_NULL) : pointer(weights),
        Ptr{Float64}(C_NULL), p, Ptr{Float64}(C_NULL), G, mu))
    (G = G, mu = mu)
end

# ---- outlier distances (src/occsd.jl, src/occod.jl, src/occsdod.jl; DESIGN.md 17): no m x p residual is formed ---------------------
struct Occsd                      # src/occsd.jl:1-8 (e_cdf: the sorted training d), then Lc with Sinv = Lc Lc'
    d
    fm
    Sinv::Matrix{Float64}
    e_cdf
    cutoff::Float64
    nlv::Int
    Lc::Matrix{Float64}
end
struct Occod                      # src/occod.jl:1-7
    d
    fm
    e_cdf
    cutoff::Float64
    nlv::Int
end
struct Occsdod                    # src/occsdod.jl:1-5
    d
    fm_sd
    fm_od
end

"""`row_resid_ss(X, shift, Z, B)` — out[i] = sum_j (X[i, j] - shift[j] - sum_l Z[i, l] B[j, l])^2 where X lives (jch_row_resid_ss); shift and B
on the host; `Z = nothing`: k = 0, the centred row sums of squares."""
function row_resid_ss(X, shift = nothing, Z = nothing, B = nothing; ctx = default_ctx())
    X = _in(X); m, p = size(X)
    k = Z === nothing ? 0 : size(Z, 2)
    out = _similar(X, m)
    shift = shift === nothing ? nothing : Vector{Float64}(vec(shift))
    Bm = k == 0 ? zeros(1, 1) : Matrix{Float64}(B)
    k == 0 || size(Bm) == (p, k) || throw(DimensionMismatch("B is not $p x $k"))
    Zm = k == 0 ? X : Z
    GC.@preserve X Zm out shift begin
        check(ctx, ccall((:jch_row_resid_ss, LIB), Int32,
                         (Ptr{Cvoid}, Int32, Ptr{Float64}, Int64, Int64, Int64, Ptr{Float64}, Ptr{Float64}, Int64, Int64, Ptr{Float64}, Int64,
                          Ptr{Float64}),
                         ctx.h, _loc(X), pointer(X), m, p, max(stride(X, 2), m), shift === nothing ? Ptr{Float64}(C_NULL) : pointer(shift),
                         k == 0 ? Ptr{Float64}(C_NULL) : pointer(Zm), k, k == 0 ? 0 : max(stride(Zm, 2), m), Bm, p, pointer(out)))
    end
    out
end

"""`row_resid_ss_lv(X, shift, Z, B, a_lo, a_hi)` — out[i, a - a_lo + 1] = sum_j (X[i, j] - shift[j] - sum_{l <= a} Z[i, l] B[j, l])^2 for a = a_lo..a_hi
where X lives, from one read of X (jch_row_resid_ss_lv); shift and B on the host; 0 <= a_lo <= a_hi <= size(Z, 2)."""
function row_resid_ss_lv(X, shift, Z, B, a_lo::Integer, a_hi::Integer; ctx = default_ctx())
    X = _in(X); m, p = size(X)
    kz = Z === nothing ? 0 : size(Z, 2)
    0 <= a_lo <= a_hi <= kz || throw(ArgumentError("needs 0 <= a_lo <= a_hi <= $kz"))
    out = _similar(X, m, a_hi - a_lo + 1)
    shift = shift === nothing ? nothing : Vector{Float64}(vec(shift))
    Bm = kz == 0 ? zeros(1, 1) : Matrix{Float64}(B)
    kz == 0 || size(Bm) == (p, kz) || throw(DimensionMismatch("B is not $p x $kz"))
    Zm = kz == 0 ? X : Z
    GC.@preserve X Zm out shift begin
        check(ctx, ccall((:jch_row_resid_ss_lv, LIB), Int32,
                         (Ptr{Cvoid}, Int32, Ptr{Float64}, Int64, Int64, Int64, Ptr{Float64}, Ptr{Float64}, Int64, Int64, Ptr{Float64}, Int64,
                          Int32, Int32, Ptr{Float64}, Int64),
                         ctx.h, _loc(X), pointer(X), m, p, max(stride(X, 2), m), shift === nothing ? Ptr{Float64}(C_NULL) : pointer(shift),
                         kz == 0 ? Ptr{Float64}(C_NULL) : pointer(Zm), kz, kz == 0 ? 0 : max(stride(Zm, 2), m), Bm, p, a_lo, a_hi, pointer(out),
                         max(m, 1)))
    end
    out
end

const _MAD_CONSTANT = 1.4826022185056018      # StatsBase 0.33 / 0.34 `mad(x)`: normalize = true is the default (DESIGN.md 6)
_median_sorted(s) = (n = length(s); isodd(n) ? s[(n + 1) >> 1] : (s[n >> 1] + s[(n >> 1) + 1]) / 2)
function _quantile_sorted(s, q)   # Statistics._quantile with alpha = beta = 1 (type 7)
    n = length(s); aleph = n * q + (1 - q)
    j = clamp(trunc(Int, aleph), 1, max(n - 1, 1)); g = clamp(aleph - j, 0, 1)
    a = s[j]; b = s[min(j + 1, n)]
    a + g * (b - a)
end
function _occ_cutoff(s, typc, cri, alpha)      # s: the sorted d on the host
    typc == "mad" && (med = _median_sorted(s); return med + cri * _MAD_CONSTANT * _median_sorted(sort(abs.(s .- med))))
    typc == "q" && return _quantile_sorted(s, 1 - alpha)
    throw(ArgumentError("typc = $typc must be \"mad\" or \"q\""))
end
# pval(e_cdf, q) = 1 - #(d <= q) / n by a right-sided search in the sorted training d; the m values go through the host
_occ_pval(e_cdf, d) = (s = Array(e_cdf); _colocate([1 - searchsortedlast(s, v) / length(s) for v in Array(d)], d))
_occ_pred(dstand) = reshape(Int64.(Array(dstand) .> 1), :, 1)
_occ_loadings(object) = hasproperty(object, :R) ? object.R : object.P

"""`occsd(object; nlv, typc = "mad", cri = 3, alpha = .025)` — src/occsd.jl:129-145 for a Pca, Kpca or Plsr record (this module's or the reference's:
only the fields are read): S = cov(T[:, 1:nlv], corrected = false) (jch_weighted_cov), Sinv = Lc Lc' by a host Cholesky, d2 = |Lc' t|^2 from
U = T Lc (jch_affine_gemm) and jch_row_resid_ss with k = 0.  `kwargs` are not taken (the reference passes them to a `kde` it never calls)."""
function occsd(object; nlv = nothing, typc = "mad", cri = 3, alpha = .025, ctx = default_ctx())
    a = size(object.T, 2)
    k = nlv === nothing ? a : min(nlv, a)
    k >= 1 || throw(ArgumentError("nlv = $nlv must be >= 1"))
    T = k == a ? object.T : object.T[:, 1:k]      # a copy, as in `vip`: a view of a host Matrix is no Array, and `_loc` would take it for device memory
    S = _cov(T, ctx)
    Lc = Matrix(inv(cholesky(Symmetric(S)).L)')
    d2 = row_resid_ss(_affine(T, nothing, nothing, Lc, nothing, ctx); ctx = ctx)
    d = sqrt.(d2)
    e_cdf = sort(Array(d))
    cutoff = _occ_cutoff(e_cdf, typc, cri, alpha)
    tab = _table((d = d, dstand = d ./ cutoff, pval = _occ_pval(e_cdf, d), gh = d2 ./ k))
    Occsd(tab, object, Lc * Lc', e_cdf, cutoff, k, Lc)
end

function _occ_sd_cols(object::Occsd, X, ctx)
    fm = object.fm; k = object.nlv
    U = hasproperty(fm, :vtot) ? _affine(transform(fm, X; nlv = k, ctx = ctx), nothing, nothing, object.Lc, nothing, ctx) :
        _affine(X, fm.xmeans, fm.xscales, _occ_loadings(fm)[:, 1:k] * object.Lc, nothing, ctx)
    d2 = row_resid_ss(U; ctx = ctx)
    d = sqrt.(d2)
    (d = d, dstand = d ./ object.cutoff, pval = _occ_pval(object.e_cdf, d), gh = d2 ./ k)
end
"`predict(object::Occsd, X)` — src/occsd.jl:153-164: Lc folded into the loadings, one pass over X, then jch_row_resid_ss."
function predict(object::Occsd, X; ctx = default_ctx())
    cols = _occ_sd_cols(object, X, ctx)
    (pred = _occ_pred(cols.dstand), d = _table(cols))
end

function _occ_od2(fm, X, k, ctx)
    X = _in(X)
    k == 0 && return row_resid_ss(X, fm.xmeans; ctx = ctx)
    Tq = _affine(X, fm.xmeans, fm.xscales, _occ_loadings(fm)[:, 1:k], nothing, ctx)      # transform(fm, X; nlv = k): R of a Plsr, P of a Pca
    row_resid_ss(X, fm.xmeans, Tq, fm.P[:, 1:k] .* fm.xscales; ctx = ctx)
end
"""`occod(object, X; nlv, typc = "mad", cri = 3, alpha = .025)` — src/occod.jl:43-57: T = transform(object, X; nlv), then
jch_row_resid_ss with shift = xmeans, Z = T, B = diag(xscales) P[:, 1:nlv] (src/xfit.jl:48-51); nlv = 0 is k = 0.  A Pca or Plsr record."""
function occod(object, X; nlv = nothing, typc = "mad", cri = 3, alpha = .025, ctx = default_ctx())
    hasproperty(object, :vtot) && throw(ArgumentError("occod takes a Pca or Plsr model (src/occod.jl:43)"))
    a = size(object.T, 2)
    k = nlv === nothing ? a : min(nlv, a)
    k >= 0 || throw(ArgumentError("nlv = $nlv must be >= 0"))
    d = sqrt.(_occ_od2(object, X, k, ctx))
    e_cdf = sort(Array(d))
    cutoff = _occ_cutoff(e_cdf, typc, cri, alpha)
    Occod(_table((d = d, dstand = d ./ cutoff, pval = _occ_pval(e_cdf, d))), object, e_cdf, cutoff, k)
end
function _occ_od_cols(object::Occod, X, ctx)
    d = sqrt.(_occ_od2(object.fm, X, object.nlv, ctx))
    (d = d, dstand = d ./ object.cutoff, pval = _occ_pval(object.e_cdf, d))
end
"`predict(object::Occod, X)` — src/occod.jl:65-75."
function predict(object::Occod, X; ctx = default_ctx())
    cols = _occ_od_cols(object, X, ctx)
    (pred = _occ_pred(cols.dstand), d = _table(cols))
end

_occ_hcat(sd, od) = merge(NamedTuple{Tuple(Symbol(c, "_sd") for c in keys(sd))}(values(sd)), NamedTuple{Tuple(Symbol(c, "_od") for c in keys(od))}(values(od)),
                          (dstand = sqrt.(sd.dstand .* od.dstand),))
_occ_cols(tab) = tab isa NamedTuple ? tab : NamedTuple{Tuple(Symbol.(names(tab)))}(Tuple(tab[!, c] for c in names(tab)))
"""`occsdod(object, X; nlv_sd, nlv_od, typc = "mad", cri = 3, alpha = .025)` — src/occsdod.jl:35-52; `fm_sd.d` is not renamed in
place."""
function occsdod(object, X; nlv_sd = nothing, nlv_od = nothing, typc = "mad", cri = 3, alpha = .025, ctx = default_ctx())
    fm_sd = occsd(object; nlv = nlv_sd, typc = typc, cri = cri, alpha = alpha, ctx = ctx)
    fm_od = occod(object, X; nlv = nlv_od, typc = typc, cri = cri, alpha = alpha, ctx = ctx)
    Occsdod(_table(_occ_hcat(_occ_cols(fm_sd.d), _occ_cols(fm_od.d))), fm_sd, fm_od)
end
"`predict(object::Occsdod, X)` — src/occsdod.jl:60-74."
function predict(object::Occsdod, X; ctx = default_ctx())
    cols = _occ_hcat(_occ_sd_cols(object.fm_sd, X, ctx), _occ_od_cols(object.fm_od, X, ctx))
    (pred = _occ_pred(cols.dstand), d = _table(cols))
end

# ---- exact column medians / MADs and the Stahel-Donoho outlyingness (src/utility.jl:162, src/stah.jl, src/occstah.jl; DESIGN.md 18) ----------
struct Occstah                    # src/occstah.jl:1-6 (e_cdf: the sorted training d)
    d
    res_stah
    e_cdf
    cutoff::Float64
end

"""`col_median_mad(X)` — (med, mad) of the columns of X as host vectors, exact order statistics from the device (jch_col_median_mad): odd n the
middle value, even n `middle(lo, hi)`; mad = 1.4826022185056018 * median(|x - med|).  A column holding a NaN gives NaN for both."""
function col_median_mad(X; ctx = default_ctx())
    X = _in(X); n, p = size(X)
    med = zeros(p); md = zeros(p)
    GC.@preserve X med md begin
        check(ctx, ccall((:jch_col_median_mad, LIB), Int32,
                         (Ptr{Cvoid}, Int32, Ptr{Float64}, Int64, Int64, Int64, Ptr{Float64}, Ptr{Float64}, Int32),
                         ctx.h, _loc(X), pointer(X), n, p, max(stride(X, 2), n), pointer(med), pointer(md), Int32(0)))
    end
    (med, md)
end
"`colmad(X)` — src/utility.jl:162-170: the MAD of each column (jch_col_median_mad)."
colmad(X; ctx = default_ctx()) = col_median_mad(X; ctx = ctx)[2]

# one jch_stah call: d where X lives; mu and s are written when fit
function _stah_call(X, mu_scal, s_scal, P, fit::Bool, mu, s, ctx)
    n, p = size(X); a = size(P, 2)
    size(P, 1) == p || throw(DimensionMismatch("P is not $p x $a"))
    d = _similar(X, n)
    GC.@preserve X mu_scal s_scal P mu s d begin
        check(ctx, ccall((:jch_stah, LIB), Int32,
                         (Ptr{Cvoid}, Int32, Ptr{Float64}, Int64, Int64, Int64, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Int64, Int64, Int32,
                          Ptr{Float64}, Ptr{Float64}, Ptr{Float64}),
                         ctx.h, _loc(X), pointer(X), n, p, max(stride(X, 2), n), pointer(mu_scal), pointer(s_scal), pointer(P), a, p, Int32(fit),
                         pointer(mu), pointer(s), pointer(d)))
    end
    d
end

"""`stah(X, a; scal = true)` — src/stah.jl:37-58: (d, P, mu_scal, s_scal, mu, s).  mu_scal, s_scal: the column medians and MADs of X when `scal`;
T = cscale(X, mu_scal, s_scal) * P in column panels, mu and s its column medians and MADs, d[i] = max_j |(t_ij - mu_j) / s_j| (jch_stah).  `P`
(p x a) is drawn with `rand(0:1, p, a)` unless given: the reference's `sample(0:1, p * a)` comes from a stream it does not pin."""
function stah(X, a; scal = true, P = nothing, ctx = default_ctx())
    a >= 1 || throw(ArgumentError("a = $a must be >= 1"))
    X = _in(X); n, p = size(X)
    Pm = P === nothing ? Matrix{Float64}(rand(0:1, p, a)) : Matrix{Float64}(P)
    size(Pm) == (p, a) || throw(DimensionMismatch("P is not $p x $a"))
    mu_scal = zeros(p); s_scal = ones(p)
    if scal
        mu_scal, s_scal = col_median_mad(X; ctx = ctx)
    end
    mu = zeros(a); s = zeros(a)
    d = _stah_call(X, mu_scal, s_scal, Pm, true, mu, s, ctx)
    (d = d, P = Pm, mu_scal = mu_scal, s_scal = s_scal, mu = mu, s = s)
end

"""`occstah(X; a = 2000, typc = "mad", cri = 3, alpha = .025, scal = true)` — src/occstah.jl:28-47.  `kwargs` are not taken (the reference passes
them to a `kde` it never calls)."""
function occstah(X; a = 2000, typc = "mad", cri = 3, alpha = .025, scal = true, P = nothing, ctx = default_ctx())
    typc in ("mad", "q") || throw(ArgumentError("typc = $typc must be \"mad\" or \"q\""))
    res = stah(X, a; scal = scal, P = P, ctx = ctx)
    d = res.d
    e_cdf = sort(Array(d))
    cutoff = _occ_cutoff(e_cdf, typc, cri, alpha)
    Occstah(_table((d = d, dstand = d ./ cutoff, pval = _occ_pval(e_cdf, d))), res, e_cdf, cutoff)
end

"`predict(object::Occstah, X)` — src/occstah.jl:55-73: one jch_stah call with fit = 0."
function predict(object::Occstah, X; ctx = default_ctx())
    res = object.res_stah
    X = _in(X)
    d = _stah_call(X, Vector{Float64}(res.mu_scal), Vector{Float64}(res.s_scal), Matrix{Float64}(res.P), false, Vector{Float64}(res.mu),
                   Vector{Float64}(res.s), ctx)
    cols = (d = d, dstand = d ./ object.cutoff, pval = _occ_pval(object.e_cdf, d))
    (pred = _occ_pred(cols.dstand), d = _table(cols))
end

# ---- sampling of the calibration set (src/sampling.jl; DESIGN.md 19): Kennard-Stone and Duplex without an n x n matrix ---------------------
# All indices are 1-based here; the C ABI is 0-based.
"""`farthest_pair(X; skip = Int[])` — (row, col, d2), row > col: the two rows of X with the largest squared Euclidean distance among the rows not in
`skip` (jch_farthest_pair); ties go to the smallest col, then the smallest row, as `findall(D .== maximum(D))[1]` on the distance matrix."""
function farthest_pair(X; skip = Int[], ctx = default_ctx())
    X = _in(X); n, p = size(X)
    sk = Vector{Int64}(collect(skip) .- 1)
    pair = zeros(Int64, 2); d2 = zeros(1)
    GC.@preserve X sk pair d2 begin
        check(ctx, ccall((:jch_farthest_pair, LIB), Int32,
                         (Ptr{Cvoid}, Int32, Ptr{Float64}, Int64, Int64, Int64, Ptr{Int64}, Int32, Ptr{Int64}, Ptr{Float64}),
                         ctx.h, _loc(X), pointer(X), n, p, max(stride(X, 2), n), pointer(sk), Int32(length(sk)), pointer(pair), pointer(d2)))
    end
    (row = pair[1] + 1, col = pair[2] + 1, d2 = d2[1])
end

"""`maxmin_select(X, init, k; nsets = 1)` — (sel, dsel), k x nsets: the rows in the order they were taken and the min-distance at which each was taken,
from the starting pair(s) `init` (jch_maxmin_select).  nsets = 1: Kennard-Stone; nsets = 2: Duplex, one read of X per pair of rows."""
function maxmin_select(X, init, k; nsets = 1, ctx = default_ctx())
    X = _in(X); n, p = size(X)
    ini = Vector{Int64}(vec(collect(init)) .- 1)
    length(ini) == 2 * nsets || throw(ArgumentError("init must hold 2 nsets = $(2 * nsets) rows"))
    k >= 2 || throw(ArgumentError("k = $k must be >= 2"))
    sel = zeros(Int64, k, nsets); dsel = zeros(k, nsets)
    GC.@preserve X ini sel dsel begin
        check(ctx, ccall((:jch_maxmin_select, LIB), Int32,
                         (Ptr{Cvoid}, Int32, Ptr{Float64}, Int64, Int64, Int64, Int32, Ptr{Int64}, Int64, Ptr{Int64}, Ptr{Float64}),
                         ctx.h, _loc(X), pointer(X), n, p, max(stride(X, 2), n), Int32(nsets), pointer(ini), k, pointer(sel), pointer(dsel)))
    end
    (sel = sel .+ 1, dsel = dsel)
end

# X itself ("eucl"), or Z = X * Uinv where X lives ("mahal": S = U'U the uncorrected covariance, src/distances.jl:104-117; p = 1: 1 / sqrt(S))
function _samp_space(X, metric, ctx)
    metric in ("eucl", "mahal") || throw(ArgumentError("metric = $metric must be \"eucl\" or \"mahal\""))
    X = _in(X)
    metric == "eucl" && return X
    p = size(X, 2)
    S = _cov(X, ctx)
    if p == 1
        S[1, 1] > 0 || throw(ArgumentError("the covariance of X is not positive definite"))
        return _affine(X, nothing, nothing, fill(1 / sqrt(S[1, 1]), 1, 1), nothing, ctx)
    end
    Uinv = Matrix{Float64}(inv(cholesky(Hermitian(S)).U))          # throws PosDefException on a singular S
    _affine(X, nothing, nothing, Uinv, nothing, ctx)
end

"""`sampks(X; k, metric = "eucl")` — src/sampling.jl:40-60, Kennard-Stone: (train, test); train in selection order, starting with the farthest
pair [row, col], test ascending.  Nothing n x n is built: jch_farthest_pair, then one read of X per selected row (jch_maxmin_select)."""
function sampks(X; k, metric = "eucl", ctx = default_ctx())
    k = Int64(round(k))
    Z = _samp_space(X, metric, ctx); n = size(Z, 1)
    2 <= k <= n || throw(ArgumentError("k = $k must be >= 2 and <= n = $n"))
    pr = farthest_pair(Z; ctx = ctx)
    s = vec(maxmin_select(Z, [pr.row, pr.col], k; nsets = 1, ctx = ctx).sel)
    (train = s, test = setdiff(1:n, s))
end

"""`sampdp(X; k, metric = "eucl")` — src/sampling.jl:118-148, Duplex: (train, test, remain), k rows each.  The second pair is the farthest pair among
the rows outside the first (the masked reading of :133, DESIGN.md 6)."""
function sampdp(X; k, metric = "eucl", ctx = default_ctx())
    k = Int64(round(k))
    Z = _samp_space(X, metric, ctx); n = size(Z, 1)
    (2 <= k && 2 * k <= n && n >= 4) || throw(ArgumentError("k = $k must be >= 2 and <= n / 2 (n = $n)"))
    p1 = farthest_pair(Z; ctx = ctx)
    p2 = farthest_pair(Z; skip = [p1.row, p1.col], ctx = ctx)
    sel = maxmin_select(Z, [p1.row, p1.col, p2.row, p2.col], k; nsets = 2, ctx = ctx).sel
    s1 = sel[:, 1]; s2 = sel[:, 2]
    (train = s1, test = s2, remain = setdiff(1:n, vcat(s1, s2)))
end

"""`sampsys(y; k)` — src/sampling.jl:168-182: k ranks on a regular grid over the sorted y (the minimum and the maximum always); host only."""
function sampsys(y; k)
    k = Int64(round(k)); y = vec(y); n = length(y)
    k >= 2 || throw(ArgumentError("k = $k must be >= 2"))
    z = unique(Int64.(round.(range(1, n; length = k))))
    s = sortperm(y)[z]
    (train = s, test = setdiff(1:n, s))
end

"""`sampcla(x, y = nothing; k, seed = nothing)` — src/sampling.jl:218-243: k rows (one number, or one per class) from every class of x, clipped to
the class size; random without replacement when y is nothing (`seed` pins the stream), else `sampsys` over the class's y; host only."""
function sampcla(x, y = nothing; k, seed = nothing)
    x = vec(x); n = length(x)
    lev = sort(unique(x)); nlev = length(lev)
    ni = [count(==(l), x) for l in lev]
    kk = length(k) == 1 ? fill(Int64(round(k[1])), nlev) : Int64.(round.(collect(k)))
    length(kk) == nlev || throw(ArgumentError("k has $(length(kk)) entries: one, or one per class ($nlev)"))
    rng = seed === nothing ? Random.default_rng() : Random.MersenneTwister(seed)
    s = Int64[]
    for i in 1:nlev
        kk[i] = min(kk[i], ni[i])
        zs = findall(==(lev[i]), x)
        if y === nothing
            append!(s, Random.shuffle(rng, zs)[1:kk[i]])
        elseif kk[i] == 1
            push!(s, zs[argmin(vec(y)[zs])])
        else
            append!(s, zs[sampsys(vec(y)[zs]; k = kk[i]).train])
        end
    end
    (train = s, test = setdiff(1:n, s), lev = lev, ni = ni, k = kk)
end

# ---- the kNN search on its own and what the reference builds on it (src/getknn.jl, src/knnr.jl, src/knnda.jl, src/occknndis.jl,
# src/occlknndis.jl; DESIGN.md 20).  Row indices are 1-based here; the C ABI is 0-based.  NOT EXECUTED in the build image (no Julia toolchain).
mutable struct KnnHandle
    h::Ptr{Cvoid}                # jch_knn_model*
    n::Int
    ctx::JchCtx
end
function knn_release!(kh::KnnHandle)
    kh.h == C_NULL && return nothing
    ccall((:jch_knn_release, LIB), Int32, (Ptr{Cvoid}, Ptr{Cvoid}), C_NULL, kh.h)
    kh.h = C_NULL
    nothing
end
"`knn_prepare(Zt)`: the device handle of a search space (jch_knn_prepare); released by the GC or `knn_release!`."
function knn_prepare(Zt; ctx = default_ctx())
    Zt = _in(Zt); n, dd = size(Zt)
    r = Ref{Ptr{Cvoid}}(C_NULL)
    GC.@preserve Zt check(ctx, ccall((:jch_knn_prepare, LIB), Int32,
        (Ptr{Cvoid}, Int32, Ptr{Float64}, Int64, Int64, Int64, Ref{Ptr{Cvoid}}),
        ctx.h, _loc(Zt), pointer(Zt), n, dd, max(stride(Zt, 2), n), r))
    kh = KnnHandle(r[], n, ctx)
    finalizer(knn_release!, kh)
    kh
end

"""`knn_search(kh, Zq, k; self = nothing, h = Inf, tol = 0)` — jch_knn_search with host outputs: (ind, d, w, dmed); ind, d, w are k x m (one column
per query, the C layout [m][k]), rows 1-based.  `self`: one training row per query (0: none) that is taken out of that query's candidates."""
function knn_search(kh::KnnHandle, Zq, k; self = nothing, h = Inf, tol = 0.0)
    ctx = kh.ctx
    Zq = _in(Zq); m = size(Zq, 1)
    k = min(Int(k), self === nothing ? kh.n : kh.n - 1)
    k >= 1 || throw(ArgumentError("k = $k must be >= 1"))
    sr = self === nothing ? Int64[] : Vector{Int64}(collect(self) .- 1)
    srd = (self === nothing || Zq isa Array) ? sr : copyto!(similar(Zq, Int64, m), sr)
    ind = zeros(Int32, k, m); dist = zeros(k, m); w = zeros(k, m); dmed = zeros(m)
    GC.@preserve Zq srd ind dist w dmed begin
        check(ctx, ccall((:jch_knn_search, LIB), Int32,
                         (Ptr{Cvoid}, Ptr{Cvoid}, Int32, Ptr{Float64}, Int64, Int64, Int32, Ptr{Int64}, Float64, Float64, Int32, Ptr{Int32}, Ptr{Float64},
                          Ptr{Float64}, Ptr{Float64}),
                         ctx.h, kh.h, _loc(Zq), pointer(Zq), m, max(stride(Zq, 2), m), Int32(k), self === nothing ? Ptr{Int64}(C_NULL) : pointer(srd),
                         Float64(h), Float64(tol), Int32(0), pointer(ind), pointer(dist), pointer(w), pointer(dmed)))
    end
    (ind = Int.(ind) .+ 1, d = dist, w = w, dmed = dmed)
end

"`knn_wmean(Y, ind, w)` — jch_knn_wmean on host arrays: m x q, row i = sum_j (w[j, i] / sum_j w[j, i]) Y[ind[j, i], :]; ind, w: k x m."
function knn_wmean(Y, ind, w; ctx = default_ctx())
    Y = Matrix{Float64}(Array(_in(Y))); n, q = size(Y); k, m = size(ind)
    i0 = Matrix{Int32}(ind .- 1); wm = Matrix{Float64}(w); pred = zeros(m, q)
    GC.@preserve Y i0 wm pred begin
        check(ctx, ccall((:jch_knn_wmean, LIB), Int32,
                         (Ptr{Cvoid}, Int32, Ptr{Float64}, Int64, Int64, Int64, Ptr{Int32}, Ptr{Float64}, Int64, Int32, Ptr{Float64}),
                         ctx.h, Int32(0), pointer(Y), n, q, n, pointer(i0), pointer(wm), m, Int32(k), pointer(pred)))
    end
    pred
end

"`knn_vote(cls, ncls, ind, w)` — jch_knn_vote on host arrays: (pred, score); cls: class codes 1 .. ncls of the n training rows; ties go to the lowest code."
function knn_vote(cls, ncls, ind, w; ctx = default_ctx())
    c0 = Vector{Int32}(vec(cls) .- 1); n = length(c0); k, m = size(ind)
    i0 = Matrix{Int32}(ind .- 1); wm = Matrix{Float64}(w); pred = zeros(Int32, m); score = zeros(m, ncls)
    GC.@preserve c0 i0 wm pred score begin
        check(ctx, ccall((:jch_knn_vote, LIB), Int32,
                         (Ptr{Cvoid}, Int32, Ptr{Int32}, Int64, Int32, Ptr{Int32}, Ptr{Float64}, Int64, Int32, Ptr{Int32}, Ptr{Float64}),
                         ctx.h, Int32(0), pointer(c0), n, Int32(ncls), pointer(i0), pointer(wm), m, Int32(k), pointer(pred), pointer(score)))
    end
    (pred = Int.(pred) .+ 1, score = score)
end

"`knn_gather_median(v, ind)` — jch_knn_gather_median on host arrays: the median of v[ind[:, i]] per query, `middle` for even k, NaN last."
function knn_gather_median(v, ind; ctx = default_ctx())
    vv = Vector{Float64}(vec(v)); n = length(vv); k, m = size(ind)
    i0 = Matrix{Int32}(ind .- 1); out = zeros(m)
    GC.@preserve vv i0 out begin
        check(ctx, ccall((:jch_knn_gather_median, LIB), Int32,
                         (Ptr{Cvoid}, Int32, Ptr{Float64}, Int64, Ptr{Int32}, Int64, Int32, Ptr{Float64}),
                         ctx.h, Int32(0), pointer(vv), n, pointer(i0), m, Int32(k), pointer(out)))
    end
    out
end

_knn_lists(res) = (listnn = [res.ind[:, i] for i in 1:size(res.ind, 2)], listd = [res.d[:, i] for i in 1:size(res.d, 2)],
                   listw = [res.w[:, i] for i in 1:size(res.w, 2)])

"""`getknn(Xtrain, X; k = 1, metric = "eucl")` — src/getknn.jl:29-57: (ind, d) as lists, one vector per query, in (distance, row) order."""
function getknn(Xtrain, X; k = 1, metric = "eucl", ctx = default_ctx())
    Xt = _in(Xtrain); X = _in(X)
    Zt, qmap, _ = _knn_train_space((fm = nothing, scal = false, metric = metric), Xt, ctx)
    kh = knn_prepare(Zt; ctx = ctx)
    res = knn_search(kh, qmap(X), k)
    knn_release!(kh)
    l = _knn_lists(res)
    (ind = l.listnn, d = l.listd)
end

struct Knnr                       # src/knnr.jl:1-11
    X; Y; fm; nlvdis::Int; metric::String; h::Real; k::Int; tol::Real; scal::Bool
end
struct Knnda                      # src/knnda.jl:1-13
    X; y; fm; nlvdis::Int; metric::String; h::Real; k::Int; tol::Real; lev; ni; scal::Bool
end
"`knnr(X, Y; nlvdis = 0, metric = \"eucl\", h = Inf, k = 1, tol = 1e-4, scal = false)` — src/knnr.jl:119-130."
function knnr(X, Y; nlvdis = 0, metric = "eucl", h = Inf, k = 1, tol = 1e-4, scal = false, ctx = default_ctx())
    X = _in(X); Y = _in(Y)
    fm = nlvdis == 0 ? nothing : plskern(X, Y; nlv = nlvdis, scal = scal, ctx = ctx)
    Knnr(X, Y, fm, nlvdis, metric, h, k, tol, scal)
end
"`knnda(X, y; nlvdis = 0, metric = \"eucl\", h = Inf, k = 1, tol = 1e-4, scal = false)` — src/knnda.jl:87-100."
function knnda(X, y; nlvdis = 0, metric = "eucl", h = Inf, k = 1, tol = 1e-4, scal = false, ctx = default_ctx())
    X = _in(X); res = dummy(y); yv = vec(Array(y))
    ni = [count(==(l), yv) for l in res.lev]
    fm = nlvdis == 0 ? nothing : plskern(X, _colocate_mat(res.Y, X); nlv = nlvdis, scal = scal, ctx = ctx)
    Knnda(X, y, fm, nlvdis, metric, h, k, tol, res.lev, ni, scal)
end
function _knn_model_search(object, X, ctx)       # src/knnr.jl:142-160: the search space of lwplsr, one search with the weights
    Xt = _in(object.X); X = _in(X)
    Zt, qmap, _ = _knn_train_space(object, Xt, ctx)
    kh = knn_prepare(Zt; ctx = ctx)
    res = knn_search(kh, qmap(X), object.k; h = object.h, tol = object.tol)
    knn_release!(kh)
    res
end
"`predict(object::Knnr, X)` — src/knnr.jl:137-169."
function predict(object::Knnr, X; ctx = default_ctx())
    res = _knn_model_search(object, X, ctx)
    merge((pred = knn_wmean(object.Y, res.ind, res.w; ctx = ctx),), _knn_lists(res))
end
"`predict(object::Knnda, X)` — src/knnda.jl:108-138."
function predict(object::Knnda, X; ctx = default_ctx())
    res = _knn_model_search(object, X, ctx)
    yv = vec(Array(object.y))
    cls = [searchsortedfirst(object.lev, v) for v in yv]
    code = knn_vote(cls, length(object.lev), res.ind, res.w; ctx = ctx).pred
    merge((pred = reshape(object.lev[code], :, 1),), _knn_lists(res))
end

# ---- locally weighted MLR and MLR-DA (src/lwmlr.jl, src/lwmlr_s.jl, src/lwmlrda.jl, src/lwmlrda_s.jl through src/locw.jl, src/mlr.jl:69-86 and
# src/mlrda.jl; DESIGN.md 23): one search, then one jch_knn_wls.  NOT EXECUTED in the build image (no Julia toolchain).
"""`knn_wls(X, Y, Xq, ind, w)` — jch_knn_wls on host arrays: (pred, info).  Per query i the weighted least-squares fit (Householder QR) of
Y[ind[:, i], :] on X[ind[:, i], :] with the weights w[:, i] / sum(w[:, i]), evaluated at Xq[i, :]; ind, w: k x m, rows 1-based.  info: 0 fitted,
1 rank-deficient (the row of pred is NaN; the reference returns LAPACK's minimum-norm solution there), 2 the constant response of src/locw.jl:33-34."""
function knn_wls(X, Y, Xq, ind, w; ctx = default_ctx())
    Xm = Matrix{Float64}(Array(_in(X))); Ym = Matrix{Float64}(Array(_in(Y))); Qm = Matrix{Float64}(Array(_in(Xq)))
    n, d = size(Xm); q = size(Ym, 2); k, m = size(ind)
    (size(Ym, 1) == n && size(Qm, 2) == d && size(Qm, 1) == m && size(w) == size(ind)) || throw(DimensionMismatch("knn_wls: X, Y, Xq, ind and w do not fit"))
    i0 = Matrix{Int32}(ind .- 1); wm = Matrix{Float64}(w); pred = zeros(m, q); info = zeros(Int32, m)
    GC.@preserve Xm Ym Qm i0 wm pred info begin
        check(ctx, ccall((:jch_knn_wls, LIB), Int32,
                         (Ptr{Cvoid}, Int32, Ptr{Float64}, Int64, Int64, Int64, Ptr{Float64}, Int64, Int64, Ptr{Float64}, Int64, Int64, Ptr{Int32},
                          Ptr{Float64}, Int32, Ptr{Float64}, Ptr{Int32}),
                         ctx.h, Int32(0), pointer(Xm), n, d, n, pointer(Ym), q, n, pointer(Qm), m, m, pointer(i0), pointer(wm), Int32(k), pointer(pred),
                         pointer(info)))
    end
    (pred = pred, info = Int.(info))
end

struct Lwmlr                      # src/lwmlr.jl:1-9
    X; Y; metric::String; h::Real; k::Int; tol::Real; verbose::Bool
end
struct LwmlrS                     # src/lwmlr_s.jl:1-10
    T; Y; fm; metric::String; h::Real; k::Int; tol::Real; verbose::Bool
end
struct Lwmlrda                    # src/lwmlrda.jl:1-9
    X; y; metric::String; h::Real; k::Int; tol::Real; verbose::Bool
end
struct LwmlrdaS                   # src/lwmlrda_s.jl:1-10
    T; y; fm; metric::String; h::Real; k::Int; tol::Real; verbose::Bool
end
function _lw_check(metric, h, k)
    metric in ("eucl", "mahal") || throw(ArgumentError("metric must be \"eucl\" or \"mahal\""))
    (k isa Integer && k >= 1) || throw(ArgumentError("k = $k must be an integer >= 1"))
    h > 0 || throw(ArgumentError("h = $h must be > 0"))
    nothing
end
"`lwmlr(X, Y; metric = \"eucl\", h, k, tol = 1e-4, verbose = false)` — src/lwmlr.jl:64-70."
function lwmlr(X, Y; metric = "eucl", h, k, tol = 1e-4, verbose = false, ctx = default_ctx())
    _lw_check(metric, h, k)
    Lwmlr(_in(X), _in(Y), metric, h, k, tol, verbose)
end
"`lwmlrda(X, y; metric = \"eucl\", h, k, tol = 1e-4, verbose = false)` — src/lwmlrda.jl:58-64."
function lwmlrda(X, y; metric = "eucl", h, k, tol = 1e-4, verbose = false, ctx = default_ctx())
    _lw_check(metric, h, k)
    Lwmlrda(_in(X), ensure_mat(y), metric, h, k, tol, verbose)
end
_lw_transform(fm, X, ctx) = transform(fm, X; ctx = ctx)      # (Pca, Plsr, Plsrda through its inner fit, Dkplsr: the methods above)
function _lw_reduce(X, Y, yv, s, nlv, reduc, gamma, scal, ctx)      # src/lwmlr_s.jl:84-95, src/lwmlrda_s.jl:90-103
    reduc in ("pca", "pls", "dkpls") || throw(ArgumentError("reduc must be \"pca\", \"pls\" or \"dkpls\""))
    zX = s === nothing ? X : _colocate_mat(Array(X)[s, :], X)
    zY = Y === nothing ? nothing : (s === nothing ? Y : _colocate_mat(Array(Y)[s, :], X))
    fm = if reduc == "pca"
        pcasvd(zX; nlv = nlv, scal = scal, ctx = ctx)
    elseif reduc == "pls"
        yv === nothing ? plskern(zX, zY; nlv = nlv, scal = scal, ctx = ctx) : plsrda(zX, s === nothing ? yv : yv[s]; nlv = nlv, scal = scal, ctx = ctx)
    else
        dkplsr(zX, zY; nlv = nlv, kern = "krbf", gamma = gamma, scal = scal, ctx = ctx)
    end
    fm, _lw_transform(fm, X, ctx)
end
"""`lwmlr_s(X, Y; nlv, reduc = "pls", metric = "eucl", h, k, gamma = 1, psamp = 1, samp = "sys", tol = 1e-4, scal = false, verbose = false)` —
src/lwmlr_s.jl:73-98.  psamp = 1 takes every row; samp = "random" draws from `MersenneTwister(seed)`."""
function lwmlr_s(X, Y; nlv, reduc = "pls", metric = "eucl", h, k, gamma = 1, psamp = 1, samp = "sys", tol = 1e-4, scal = false, verbose = false,
                 seed = nothing, ctx = default_ctx())
    _lw_check(metric, h, k)
    samp in ("sys", "random") || throw(ArgumentError("samp must be \"sys\" or \"random\""))
    X = _in(X); Y = _in(Y); n = size(X, 1)
    ms = Int64(round(psamp * n))
    s = ms >= n ? nothing : (samp == "sys" ? sampsys(vec(sum(Array(Y); dims = 2)); k = ms).train : randperm(MersenneTwister(seed), n)[1:ms])
    fm, T = _lw_reduce(X, Y, nothing, s, nlv, reduc, gamma, scal, ctx)
    LwmlrS(T, Y, fm, metric, h, k, tol, verbose)
end
"""`lwmlrda_s(X, y; nlv, reduc = "pls", metric = "eucl", h, k, gamma = 1, psamp = 1, samp = "cla", tol = 1e-4, scal = false, verbose = false)` —
src/lwmlrda_s.jl:77-106.  reduc = "dkpls" is `dkplsr` on `dummy(y).Y`, which is what the reference's `dkplsrda` fits."""
function lwmlrda_s(X, y; nlv, reduc = "pls", metric = "eucl", h, k, gamma = 1, psamp = 1, samp = "cla", tol = 1e-4, scal = false, verbose = false,
                   seed = nothing, ctx = default_ctx())
    _lw_check(metric, h, k)
    samp in ("cla", "random") || throw(ArgumentError("samp must be \"cla\" or \"random\""))
    X = _in(X); yv = vec(Array(y)); n = size(X, 1)
    ms = Int64(round(psamp * n))
    nlev = length(unique(yv))
    s = ms >= n ? nothing : (samp == "cla" ? sampcla(yv; k = max(Int64(round(ms / nlev)), 1), seed = seed).train : randperm(MersenneTwister(seed), n)[1:ms])
    Yd = reduc == "dkpls" ? _colocate_mat(dummy(yv).Y, X) : nothing
    fm, T = _lw_reduce(X, Yd, yv, s, nlv, reduc, gamma, scal, ctx)
    LwmlrdaS(T, ensure_mat(y), fm, metric, h, k, tol, verbose)
end
function _lw_search(object, coords, Q, ctx)       # getknn(object.X, X; k, metric), then wdist and the clamp (src/lwmlr.jl:82-90)
    Zt, qmap, _ = _knn_train_space((fm = nothing, scal = false, metric = object.metric), coords, ctx)
    kh = knn_prepare(Zt; ctx = ctx)
    res = knn_search(kh, qmap(Q), object.k; h = object.h, tol = object.tol)
    knn_release!(kh)
    res
end
function _lw_warn(info, who)
    nbad = count(==(1), info)
    nbad > 0 && @warn "$who: $nbad of $(length(info)) neighbourhoods are rank-deficient; their predictions are NaN"
    info .== 1
end
function _lw_predict_reg(object, coords, Q, ctx, who)
    res = _lw_search(object, coords, Q, ctx)
    out = knn_wls(coords, object.Y, Q, res.ind, res.w; ctx = ctx)
    _lw_warn(out.info, who)
    object.verbose && println(join(1:size(Q, 1), " "))
    merge((pred = out.pred,), _knn_lists(res))
end
function _lw_predict_da(object, coords, Q, ctx, who)   # the global dummy table, then the row argmax: equal to `mlrda` on the local levels (DESIGN.md 23)
    res = _lw_search(object, coords, Q, ctx)
    yv = vec(Array(object.y)); dm = dummy(yv)
    out = knn_wls(coords, dm.Y, Q, res.ind, res.w; ctx = ctx)
    bad = _lw_warn(out.info, who)
    code = [argmax(replace(out.pred[i, :], NaN => -Inf)) for i in 1:size(out.pred, 1)]
    if any(bad)                                    # no fit there: the weighted vote of knnda
        cls = [searchsortedfirst(dm.lev, v) for v in yv]
        vote = knn_vote(cls, length(dm.lev), res.ind, res.w; ctx = ctx).pred
        code = [bad[i] ? vote[i] : code[i] for i in eachindex(code)]
    end
    object.verbose && println(join(1:size(Q, 1), " "))
    merge((pred = reshape(dm.lev[code], :, 1),), _knn_lists(res))
end
"`predict(object::Lwmlr, X)` — src/lwmlr.jl:78-97."
function predict(object::Lwmlr, X; ctx = default_ctx())
    _lw_predict_reg(object, object.X, _in(X), ctx, "predict(::Lwmlr)")
end
"`predict(object::LwmlrS, X)` — src/lwmlr_s.jl:106-125."
function predict(object::LwmlrS, X; ctx = default_ctx())
    _lw_predict_reg(object, object.T, _lw_transform(object.fm, _in(X), ctx), ctx, "predict(::LwmlrS)")
end
"`predict(object::Lwmlrda, X)` — src/lwmlrda.jl:72-91."
function predict(object::Lwmlrda, X; ctx = default_ctx())
    _lw_predict_da(object, object.X, _in(X), ctx, "predict(::Lwmlrda)")
end
"`predict(object::LwmlrdaS, X)` — src/lwmlrda_s.jl:114-133."
function predict(object::LwmlrdaS, X; ctx = default_ctx())
    _lw_predict_da(object, object.T, _lw_transform(object.fm, _in(X), ctx), ctx, "predict(::LwmlrdaS)")
end

struct Occknndis                  # src/occknndis.jl:1-9 (e_cdf: the sorted training d), then the search handle
    d; fm; T; tscales; k::Int; e_cdf; cutoff::Float64; kh
end
struct Occlknndis                 # src/occlknndis.jl:1-9, then the handle and the cache of the rows' leave-one-out medians (NaN: not yet computed)
    d; fm; T; tscales; k::Int; e_cdf; cutoff::Float64; kh; dk_train::Vector{Float64}
end
function _occ_knn_scores(X, nlv, scal, ctx)      # src/occknndis.jl:131-134
    fm = pcasvd(X; nlv = nlv, scal = scal, ctx = ctx)
    tscales = col_stats(fm.T; ctx = ctx).stds
    (fm, tscales, _affine(fm.T, nothing, nothing, Matrix(Diagonal(1 ./ tscales)), nothing, ctx))
end
_occ_knn_query(object, X, ctx) = _affine(transform(object.fm, X; ctx = ctx), nothing, nothing, Matrix(Diagonal(1 ./ object.tscales)), nothing, ctx)
_median_of_sorted_cols(D) = [_median_sorted(D[:, i]) for i in 1:size(D, 2)]
function _occ_knn_table(d, typc, cri, alpha)
    e_cdf = sort(d)
    cutoff = _occ_cutoff(e_cdf, typc, cri, alpha)
    (_table((d = d, dstand = d ./ cutoff, pval = _occ_pval(e_cdf, d))), e_cdf, cutoff)
end

"""`occknndis(X; nlv, nsamp, k, typc = "mad", cri = 3, alpha = .025, scal = false)` — src/occknndis.jl:125-149.  `samp` (rows) may be given: the
reference's `sample` draws from a stream it does not pin."""
function occknndis(X; nlv, nsamp = nothing, k, typc = "mad", cri = 3, alpha = .025, scal = false, samp = nothing, ctx = default_ctx())
    X = _in(X); k = Int64(k)
    fm, tscales, T = _occ_knn_scores(X, nlv, scal, ctx); n = size(T, 1)
    samp = samp === nothing ? Random.shuffle(1:n)[1:nsamp] : collect(samp)
    kh = knn_prepare(T; ctx = ctx)
    res = knn_search(kh, Array(T)[samp, :], k + 1)
    d = _median_of_sorted_cols(res.d[2:end, :])                          # :141
    tab, e_cdf, cutoff = _occ_knn_table(d, typc, cri, alpha)
    Occknndis(tab, fm, T, tscales, k, e_cdf, cutoff, kh)
end
"`predict(object::Occknndis, X)` — src/occknndis.jl:157-171."
function predict(object::Occknndis, X; ctx = default_ctx())
    d = knn_search(object.kh, _occ_knn_query(object, X, ctx), object.k).dmed
    cols = (d = d, dstand = d ./ object.cutoff, pval = _occ_pval(object.e_cdf, d))
    (pred = _occ_pred(cols.dstand), d = _table(cols))
end

# d = dmed / zd for the queries Zq: one search, the cache fill for the neighbour rows not in it yet (one search with `self` = the rows themselves,
# only dmed read), then zd = the median of dk_train over each neighbourhood (jch_knn_gather_median)
function _occl_ratio(kh, Th, dk_train, k, Zq, self, literal, ctx)
    res = knn_search(kh, Zq, k; self = self)
    ind = res.ind
    if literal                                                           # rows of the row-removed matrix, used unshifted (src/occlknndis.jl:152-153)
        ind = ind .- (ind .> permutedims(collect(self)))
    end
    need = [j for j in unique(vec(ind)) if isnan(dk_train[j])]
    if !isempty(need)
        dk_train[need] = knn_search(kh, Th[need, :], k; self = need).dmed
    end
    res.dmed ./ knn_gather_median(dk_train, ind; ctx = ctx)
end

"""`occlknndis(X; nlv, nsamp, k, typc = "mad", cri = 3, alpha = .025, scal = false, reading = "literal")` — src/occlknndis.jl:132-165.  "literal"
follows :146-157 with its two slips (the query is row i while row samp[i] is removed; the row-removed indices are used unshifted); "doc" does what the
docstring says."""
function occlknndis(X; nlv, nsamp = nothing, k, typc = "mad", cri = 3, alpha = .025, scal = false, samp = nothing, reading = "literal", ctx = default_ctx())
    reading in ("literal", "doc") || throw(ArgumentError("reading = $reading must be \"literal\" or \"doc\""))
    X = _in(X); k = Int64(k)
    fm, tscales, T = _occ_knn_scores(X, nlv, scal, ctx); n = size(T, 1)
    samp = samp === nothing ? Random.shuffle(1:n)[1:nsamp] : collect(samp)
    kh = knn_prepare(T; ctx = ctx)
    Th = Array(T); dk_train = fill(NaN, n); kk = min(k, n - 1)
    q = reading == "literal" ? collect(1:length(samp)) : samp
    d = _occl_ratio(kh, Th, dk_train, kk, Th[q, :], samp, reading == "literal", ctx)
    tab, e_cdf, cutoff = _occ_knn_table(d, typc, cri, alpha)
    Occlknndis(tab, fm, T, tscales, k, e_cdf, cutoff, kh, dk_train)
end
"`predict(object::Occlknndis, X)` — src/occlknndis.jl:173-199, from the cache."
function predict(object::Occlknndis, X; ctx = default_ctx())
    Th = Array(object.T); n = size(Th, 1)
    res = knn_search(object.kh, _occ_knn_query(object, X, ctx), object.k)
    need = [j for j in unique(vec(res.ind)) if isnan(object.dk_train[j])]
    if !isempty(need)
        object.dk_train[need] = knn_search(object.kh, Th[need, :], min(object.k, n - 1); self = need).dmed
    end
    d = res.dmed ./ knn_gather_median(object.dk_train, res.ind; ctx = ctx)
    cols = (d = d, dstand = d ./ object.cutoff, pval = _occ_pval(object.e_cdf, d))
    (pred = _occ_pred(cols.dstand), d = _table(cols))
end

# ---- kernel density estimation and the discrimination on it (src/dmkern.jl, src/kdeda.jl, src/plskdeda.jl) over jch_kde_dens; DESIGN.md §21.
# The inverse bandwidth of model a (the first dims[a] columns), class c, column j separates into u[j, c] * v[a, c]: one device pass over the
# (query, training row) pairs serves a dmkern, the classes of a kdeda, or the nlv x nlev densities of a plskdeda prediction.
struct Dmkern                     # src/dmkern.jl:1-6
    X; H; Hinv; detH
end
struct Kernda                     # src/kdeda.jl:1-6, then the rows grouped by class and the class offsets (0-based, nlev + 1)
    fm; wprior; lev; ni; Z; cs
end
struct Plslda                     # src/plslda.jl:1-5 (fm = (fm_pls, fm_da)), then what a plskdeda prediction needs: (Z, cs, u, v2)
    fm; lev; ni; kde
end

"""`kde_dens(Z, Xq, cls_start, u, v2, coef, dims)` — jch_kde_dens: out[i, c, a] = coef[a, c] * sum over the rows r of class c of
exp(-0.5 * v2[a, c] * sum_{j <= dims[a]} ((Xq[i, j] - Z[r, j]) * u[j, c])^2), an m x ncls x nmod array where Xq lives.  Z: the training rows
grouped by class, class c in rows cls_start[c] + 1 : cls_start[c + 1] (0-based offsets, ncls + 1 of them); u (d x ncls), v2 and coef
(nmod x ncls) and dims (nmod, non-decreasing within 1:d) are host arrays."""
function kde_dens(Z, Xq, cls_start, u, v2, coef, dims; ctx = default_ctx())
    Z = _in(Z); Xq = _in(Xq); n, d = size(Z); m = size(Xq, 1)
    size(Xq, 2) == d || throw(DimensionMismatch("Z has $d columns, Xq has $(size(Xq, 2))"))
    cs = Vector{Int64}(vec(cls_start)); dm = Vector{Int32}(vec(dims)); ncls = length(cs) - 1; nmod = length(dm)
    um = Matrix{Float64}(reshape(u, d, ncls)); vm = Matrix{Float64}(reshape(v2, nmod, ncls)); cm = Matrix{Float64}(reshape(coef, nmod, ncls))
    out = _similar(Xq, m, ncls, nmod)
    GC.@preserve Z Xq cs um vm cm dm out begin
        check(ctx, ccall((:jch_kde_dens, LIB), Int32,
                         (Ptr{Cvoid}, Int32, Ptr{Float64}, Int64, Int64, Int64, Ptr{Float64}, Int64, Int64, Ptr{Int64}, Int32, Ptr{Float64}, Ptr{Float64},
                          Ptr{Float64}, Ptr{Int32}, Int32, Ptr{Float64}, Int64),
                         ctx.h, _loc(Xq), pointer(Z), n, d, stride(Z, 2), pointer(Xq), m, stride(Xq, 2), pointer(cs), Int32(ncls), pointer(um),
                         pointer(vm), pointer(cm), pointer(dm), Int32(nmod), pointer(out), max(m, 1)))
    end
    out
end

_kde_bandwidths(std, n, p, h, a) = h === nothing ? a * n^(-1 / (p + 4)) .* std[1:p] : (h isa Real ? fill(Float64(h), p) : Vector{Float64}(vec(h)))
function _dm_record(X, hv)                       # src/dmkern.jl:135-142
    any(==(0), hv) && throw(LinearAlgebra.SingularException(1))
    detH = prod(hv)
    Dmkern(X, Matrix(Diagonal(hv)), Matrix(Diagonal(1 ./ hv)), detH == 0 ? 1e-20 : detH)
end
_kde_coef(n, p, detH) = 1 / n * (2 * pi)^(-p / 2) * (1 / detH)
function _kde_check_default(X, n)
    (n == 1 || any(maximum(Array(X); dims = 1) .== minimum(Array(X); dims = 1))) && throw(LinearAlgebra.SingularException(1))
end

"`dmkern(X; h = nothing, a = 1)` — src/dmkern.jl:124-143; the default bandwidth's colstd comes from the device."
function dmkern(X; h = nothing, a = 1, ctx = default_ctx())
    X = _in(X); n, p = size(X)
    (h === nothing || h isa Real || length(h) == p) || throw(DimensionMismatch("h has $(length(h)) entries, X has $p columns"))
    std = nothing
    if h === nothing
        _kde_check_default(X, n)
        std = col_stats(X; ctx = ctx).stds
    end
    _dm_record(X, _kde_bandwidths(std, n, p, h, a))
end
"`predict(object::Dmkern, X)` — src/dmkern.jl:151-163."
function predict(object::Dmkern, X; ctx = default_ctx())
    n, p = size(object.X)
    out = kde_dens(object.X, X, [0, n], reshape(diag(object.Hinv), p, 1), ones(1, 1), fill(_kde_coef(n, p, object.detH), 1, 1), [p]; ctx = ctx)
    (pred = reshape(out, :, 1),)
end

function _kde_prior(prior, ni)
    prior == "unif" && return ones(length(ni)) ./ length(ni)
    prior == "prop" && return ni ./ sum(ni)
    throw(ArgumentError("prior must be \"unif\" or \"prop\""))
end
# the rows grouped by level (stable), the 0-based class offsets, the per-class colstd (nlev x p) when the bandwidth is the default
function _kde_prepare(X, y, h, prior, ctx)
    yv = vec(Array(y)); n = size(X, 1)
    length(yv) == n || throw(DimensionMismatch("X has $n rows, y has $(length(yv))"))
    lev = sort(unique(yv)); ni = [count(==(l), yv) for l in lev]
    wprior = _kde_prior(prior, ni)
    (h === nothing && any(==(1), ni)) && throw(LinearAlgebra.SingularException(1))
    order = sortperm([searchsortedfirst(lev, v) for v in yv]; alg = MergeSort)
    (yv, lev, ni, wprior, order, vcat(0, cumsum(ni)))
end
function _kde_class_stds(Zg, cs, ctx)
    stds = zeros(length(cs) - 1, size(Zg, 2))
    for c in 1:length(cs) - 1
        blk = Zg[cs[c] + 1:cs[c + 1], :]
        _kde_check_default(blk, size(blk, 1))
        stds[c, :] = col_stats(blk; ctx = ctx).stds
    end
    stds
end
_kernda_model(Zg, cs, stds, p, h, a, wprior, lev, ni) =
    Kernda([_dm_record(Zg[cs[c] + 1:cs[c + 1], 1:p], _kde_bandwidths(stds === nothing ? nothing : stds[c, :], ni[c], p, h, a)) for c in 1:length(lev)],
           wprior, lev, ni, Zg[:, 1:p], cs)

"`kdeda(X, y; prior = \"unif\", h = nothing, a = 1)` — src/kdeda.jl:62-79: one dmkern per class on that class's rows."
function kdeda(X, y; prior = "unif", h = nothing, a = 1, ctx = default_ctx())
    X = _in(X); p = size(X, 2)
    (h === nothing || h isa Real || length(h) == p) || throw(DimensionMismatch("h has $(length(h)) entries, X has $p columns"))
    yv, lev, ni, wprior, order, cs = _kde_prepare(X, y, h, prior, ctx)
    Zg = X[order, :]
    stds = h === nothing ? _kde_class_stds(Zg, cs, ctx) : nothing
    _kernda_model(Zg, cs, stds, p, h, a, wprior, lev, ni)
end
function _kde_posterior(wprior, dens, lev)       # src/kdeda.jl:91-95 (argmax: the first level on ties and on a NaN row)
    A = Array(dens) .* permutedims(wprior)
    posterior = A ./ sum(A; dims = 2)
    z = [argmax(posterior[i, :]) for i in 1:size(posterior, 1)]
    (reshape(lev[z], :, 1), posterior)
end
"`predict(object::Kernda, X)` — src/kdeda.jl:81-97: (pred, dens, posterior), one jch_kde_dens call for all classes."
function predict(object::Kernda, X; ctx = default_ctx())
    p = size(object.Z, 2); nlev = length(object.lev)
    u = hcat([diag(f.Hinv) for f in object.fm]...)
    coef = reshape([_kde_coef(object.ni[c], p, object.fm[c].detH) for c in 1:nlev], 1, nlev)
    dens = reshape(kde_dens(object.Z, X, object.cs, u, ones(1, nlev), coef, [p]; ctx = ctx), :, nlev)
    pred, posterior = _kde_posterior(object.wprior, dens, object.lev)
    (pred = pred, dens = dens, posterior = posterior)
end

"""`plskdeda(X, y, weights = ones(n); nlv, prior = "unif", h = nothing, a = 1, scal = false)` — src/plskdeda.jl:52-64: plskern on `dummy(y)`,
then kdeda(T[:, 1:i], y) for i = 1:nlv.  `h`: nothing or a real (a vector fits the model of one nlv only)."""
function plskdeda(X, y, weights = nothing; nlv, prior = "unif", h = nothing, a = 1, scal = false, ctx = default_ctx())
    (h === nothing || h isa Real) || throw(DimensionMismatch("plskdeda: a vector h fits the model of one nlv only"))
    X = _in(X)
    yv, lev, ni, wprior, order, cs = _kde_prepare(X, y, h, prior, ctx)
    fm_pls = plskern(X, _colocate_mat(dummy(yv).Y, X), weights; nlv = nlv, scal = scal, ctx = ctx)
    k = size(fm_pls.T, 2); nlev = length(lev)
    Zg = fm_pls.T[order, :]
    stds = h === nothing ? _kde_class_stds(Zg, cs, ctx) : nothing
    fm_da = [_kernda_model(Zg, cs, stds, i, h, a, wprior, lev, ni) for i in 1:k]
    u = h === nothing ? permutedims(1 ./ stds) : fill(1 / h, k, nlev)
    v = h === nothing ? [ni[c]^(1 / (i + 4)) / a for i in 1:k, c in 1:nlev] : ones(k, nlev)
    Plslda((fm_pls = fm_pls, fm_da = fm_da), lev, ni, (Z = Zg, cs = cs, u = u, v2 = v .* v))
end
"""`predict(object::Plslda, X; nlv = nothing)` — src/plslda.jl:107-130 for a plskdeda model: one transform at the largest nlv, then one
jch_kde_dens call with dims = the clamped nlv range."""
function predict(object::Plslda, X; nlv = nothing, ctx = default_ctx())
    a = size(object.fm.fm_pls.T, 2)
    rng = nlv === nothing ? (a:a) : (max(minimum(nlv), 1):min(maximum(nlv), a))      # (:114 clamps to 0:a; there is no model 0)
    isempty(rng) && throw(BoundsError(object.fm.fm_da, 0))
    kmax = last(rng); nlev = length(object.lev); st = object.kde
    T = transform(object.fm.fm_pls, X; nlv = kmax, ctx = ctx)
    coef = [_kde_coef(object.ni[c], k, object.fm.fm_da[k].fm[c].detH) for k in rng, c in 1:nlev]
    dens = kde_dens(st.Z[:, 1:kmax], T, st.cs, st.u[1:kmax, :], st.v2[collect(rng), :], coef, collect(rng); ctx = ctx)
    res = [_kde_posterior(object.fm.fm_da[k].wprior, dens[:, :, i], object.lev) for (i, k) in enumerate(rng)]
    length(rng) == 1 ? (pred = res[1][1], posterior = res[1][2]) : (pred = [r[1] for r in res], posterior = [r[2] for r in res])
end

# ---- P2P inbox transport (include/jchemo_hip.h): export -> all-gather the handles (MPI) -> import -> agree -> enable
function p2p_export(ctx::JchCtx, nranks::Integer)
    h = zeros(UInt8, 64)
    check(ctx, ccall((:jch_ctx_p2p_export, LIB), Int32, (Ptr{Cvoid}, Int32, Ptr{Cvoid}), ctx.h, nranks, h))
    h
end
p2p_import(ctx::JchCtx, handles::Vector{UInt8}, rank::Integer, nranks::Integer) =
    ccall((:jch_ctx_p2p_import, LIB), Int32, (Ptr{Cvoid}, Ptr{Cvoid}, Int32, Int32, UInt32), ctx.h, handles, rank, nranks, 0) == 0
p2p_enable!(ctx::JchCtx, on::Bool) = check(ctx, ccall((:jch_ctx_p2p_enable, LIB), Int32, (Ptr{Cvoid}, Int32), ctx.h, on ? 1 : 0))

function __init__()
    ccall(:jl_generating_output, Cint, ()) == 1 && return nothing   # being precompiled into another image: hook up at run time
    m = get(Base.loaded_modules, _JCHEMO_ID, nothing)     # `using Jchemo` came first: hook up now; otherwise on first use
    m === nothing || attach!(m)
    nothing
end

# ---- Gaussian discrimination on raw X (src/dmnorm.jl, src/lda.jl, src/qda.jl, src/matW.jl, `mahsqchol` of src/distances.jl) over jch_class_cov,
# jch_gauss_factor and jch_mahsq_chol; DESIGN.md §24.  The densities are the reference's plain products: beyond roughly p = 130 they leave the
# Float64 range for all but well-conditioned data (densities of 0, a NaN posterior, the first level), as in the reference; the distances do not.
struct Dmnorm                     # src/dmnorm.jl:1-5
    mu; Uinv; detS
end
struct Lda                        # src/lda.jl:1-8; the nlev Dmnorm records share ONE Uinv
    fm; W; ct; wprior; lev; ni
end
struct Qda                        # src/qda.jl:1-8, then the p x p x nlev stack the records' Uinv are slices of
    fm; Wi; ct; wprior; lev; ni; Uinv
end

"""`class_cov(Z, cls_start; want_Wi = true, want_W = true)` — jch_class_cov on rows grouped by class (0-based offsets, ncls + 1 of them):
(Wi, W, ct).  Wi (p x p x ncls) and W (p x p) live where Z does (`nothing` when not wanted), ct (ncls x p) is a host matrix.  Wi[:, :, c] is the
uncorrected covariance of class c — of ALL rows for a class of one row (src/matW.jl:54-65) — and W = sum_c n_c / n Wi[:, :, c]."""
function class_cov(Z, cls_start; want_Wi = true, want_W = true, ctx = default_ctx())
    Z = _in(Z); n, p = size(Z)
    cs = Vector{Int64}(vec(cls_start)); ncls = length(cs) - 1
    Wi = want_Wi ? _similar(Z, p, p, ncls) : nothing
    W = want_W ? _similar(Z, p, p) : nothing
    ct = Matrix{Float64}(undef, ncls, p)
    GC.@preserve Z cs Wi W ct begin
        check(ctx, ccall((:jch_class_cov, LIB), Int32,
                         (Ptr{Cvoid}, Int32, Ptr{Float64}, Int64, Int64, Int64, Ptr{Int64}, Int32, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}),
                         ctx.h, _loc(Z), pointer(Z), n, p, stride(Z, 2), pointer(cs), Int32(ncls), Wi === nothing ? Ptr{Float64}(C_NULL) : pointer(Wi),
                         W === nothing ? Ptr{Float64}(C_NULL) : pointer(W), pointer(ct)))
    end
    (Wi = Wi, W = W, ct = ct)
end

"""`gauss_factor(S)` — jch_gauss_factor: S p x p or p x p x nfac, symmetric (one triangle is read) -> (Uinv, diagU, info).  Uinv has S's shape and
lives where S does: Uinv[:, :, f] = L_f^-T, upper triangular with exact zeros below the diagonal; diagU (p x nfac) and info (nfac) are host arrays;
info[f] != 0 (the column of the first pivot that is not > 0) marks a factor that failed."""
function gauss_factor(S; ctx = default_ctx())
    S3 = ndims(S) == 3 ? _f64(S) : reshape(_in(S), size(S, 1), size(S, 1), 1)
    p = size(S3, 1); nfac = size(S3, 3)
    size(S3, 2) == p || throw(DimensionMismatch("S must be p x p or p x p x nfac"))
    Uinv = _similar(S3, p, p, nfac); diagU = Matrix{Float64}(undef, p, nfac); info = zeros(Int32, nfac)
    GC.@preserve S3 Uinv diagU info begin
        check(ctx, ccall((:jch_gauss_factor, LIB), Int32,
                         (Ptr{Cvoid}, Int32, Ptr{Float64}, Int64, Int64, Int64, Int32, Ptr{Float64}, Int64, Int64, Ptr{Float64}, Ptr{Int32}),
                         ctx.h, _loc(S3), pointer(S3), p, stride(S3, 2), p * stride(S3, 2), Int32(nfac), pointer(Uinv), p, p * p, pointer(diagU), pointer(info)))
    end
    (Uinv = ndims(S) == 3 ? Uinv : reshape(Uinv, p, p), diagU = diagU, info = info)
end

"""`mahsq_chol(Xq, Mu, Uinv)` — jch_mahsq_chol: out[i, c] = |(Xq[i, :] - Mu[c, :]) Uinv_f|^2, f = 1 for one factor (Uinv p x p) or c for one per
centre (p x p x ncen); Mu (ncen x p) is taken to the host; out (m x ncen) lives where Xq does.  The difference is taken before the product."""
function mahsq_chol(Xq, Mu, Uinv; ctx = default_ctx())
    Xq = _in(Xq); m, p = size(Xq)
    Mh = Matrix{Float64}(Array(ensure_mat(Mu))); ncen = size(Mh, 1)
    size(Mh, 2) == p || throw(DimensionMismatch("Xq has $p columns, Mu has $(size(Mh, 2))"))
    U3 = ndims(Uinv) == 3 ? _f64(Uinv) : reshape(_in(Uinv), size(Uinv, 1), size(Uinv, 1), 1)
    nfac = size(U3, 3)
    (size(U3, 1) == p && size(U3, 2) == p) || throw(DimensionMismatch("Uinv is $(size(Uinv)), the data has $p columns"))
    (nfac == 1 || nfac == ncen) || throw(ArgumentError("$nfac factors for $ncen centres (one, or one per centre)"))
    out = _similar(Xq, m, ncen)
    GC.@preserve Xq Mh U3 out begin
        check(ctx, ccall((:jch_mahsq_chol, LIB), Int32,
                         (Ptr{Cvoid}, Int32, Ptr{Float64}, Int64, Int64, Int64, Ptr{Float64}, Int32, Ptr{Float64}, Int64, Int64, Int32, Ptr{Float64}, Int64),
                         ctx.h, _loc(Xq), pointer(Xq), m, p, stride(Xq, 2), pointer(Mh), Int32(ncen), pointer(U3), stride(U3, 2), p * stride(U3, 2), Int32(nfac),
                         pointer(out), max(m, 1)))
    end
    out
end

struct PosDefFailure <: Exception
    what::String
    info::Int
end
Base.showerror(io::IO, e::PosDefFailure) = print(io, "PosDefException: ", e.what, ": matrix is not positive definite; Cholesky factorization failed at column ", e.info)
_gda_posdef(info, what) = info == 0 ? nothing : throw(PosDefFailure(what, Int(info)))
function _gda_dets(diag)                      # det(U)^2 with det(U) the product of the diagonal in order; 0 -> 1e-20 (src/dmnorm.jl:121-122)
    d = 1.0
    for v in diag
        d *= v
    end
    d^2 == 0 ? 1e-20 : d^2
end
_gda_coef(p, detS) = (2 * pi)^(-p / 2) * (1 / sqrt(detS))

"`dmnorm(X = nothing; mu = nothing, S = nothing)` — src/dmnorm.jl:107-128; mean and `cov(X)` from one jch_class_cov call, the factor from jch_gauss_factor."
function dmnorm(X = nothing; mu = nothing, S = nothing, ctx = default_ctx())
    (X === nothing && (mu === nothing || S === nothing)) && throw(ArgumentError("dmnorm: give X, or both mu and S"))
    if X !== nothing && (mu === nothing || S === nothing)
        X = _in(X); n = size(X, 1)
        res = class_cov(X, [0, n]; want_Wi = S === nothing, want_W = false, ctx = ctx)
        mu === nothing && (mu = res.ct[1, :])
        S === nothing && (S = res.Wi[:, :, 1] .* (n / (n - 1)))
    end
    muv = Vector{Float64}(vec(Array(mu))); S = ensure_mat(S)
    (size(S, 1) == size(S, 2) == length(muv)) || throw(DimensionMismatch("mu has $(length(muv)) entries, S is $(size(S))"))
    f = gauss_factor(S; ctx = ctx)
    _gda_posdef(f.info[1], "dmnorm")
    Dmnorm(muv, f.Uinv, _gda_dets(f.diagU[:, 1]))
end
"`predict(object::Dmnorm, X)` — src/dmnorm.jl:136-143: one jch_mahsq_chol call."
function predict(object::Dmnorm, X; ctx = default_ctx())
    X = _in(X); p = size(X, 2)
    p == length(object.mu) || throw(DimensionMismatch("X has $p columns, the model has $(length(object.mu))"))
    d = mahsq_chol(X, reshape(object.mu, 1, :), object.Uinv; ctx = ctx)
    (pred = _gda_coef(p, object.detS) .* exp.(-.5 .* d),)
end

function _gda_prepare(X, y, prior)
    yv = vec(Array(y)); n = size(X, 1)
    length(yv) == n || throw(DimensionMismatch("X has $n rows, y has $(length(yv))"))
    lev = sort(unique(yv)); ni = [count(==(l), yv) for l in lev]
    wprior = _kde_prior(prior, ni)
    order = sortperm([searchsortedfirst(lev, v) for v in yv]; alg = MergeSort)
    (lev, ni, wprior, order, vcat(0, cumsum(ni)))
end

"`lda(X, y; prior = \"unif\")` — src/lda.jl:56-77: W of `matW` times n / (n - nlev), ONE factor, nlev Dmnorm records that share its Uinv."
function lda(X, y; prior = "unif", ctx = default_ctx())
    X = _in(X); n = size(X, 1)
    lev, ni, wprior, order, cs = _gda_prepare(X, y, prior)
    nlev = length(lev)
    res = class_cov(X[order, :], cs; want_Wi = false, ctx = ctx)
    W = res.W .* (n / (n - nlev))
    f = gauss_factor(W; ctx = ctx)
    _gda_posdef(f.info[1], "lda: the pooled W of $n rows in $nlev classes")
    detS = _gda_dets(f.diagU[:, 1])
    Lda([Dmnorm(res.ct[i, :], f.Uinv, detS) for i in 1:nlev], W, res.ct, wprior, lev, ni)
end

"`qda(X, y; prior = \"unif\")` — src/qda.jl:55-79: S_i = Wi[i] n_i / (n_i - 1) (Wi[i] itself for a class of one row), nlev factors in one call."
function qda(X, y; prior = "unif", ctx = default_ctx())
    X = _in(X)
    lev, ni, wprior, order, cs = _gda_prepare(X, y, prior)
    nlev = length(lev); p = size(X, 2)
    res = class_cov(X[order, :], cs; want_W = false, ctx = ctx)
    S = res.Wi .* _colocate_mat(reshape([k == 1 ? 1.0 : k / (k - 1) for k in ni], 1, 1, nlev), res.Wi)
    f = gauss_factor(S; ctx = ctx)
    for i in 1:nlev
        _gda_posdef(f.info[i], "qda: class $(lev[i]) ($(ni[i]) rows)")
    end
    Qda([Dmnorm(res.ct[i, :], f.Uinv[:, :, i], _gda_dets(f.diagU[:, i])) for i in 1:nlev], res.Wi, res.ct, wprior, lev, ni, f.Uinv)
end

function _gda_predict(fm, U, wprior, lev, X, ctx)
    X = _in(X); p = size(X, 2)
    p == length(fm[1].mu) || throw(DimensionMismatch("X has $p columns, the model has $(length(fm[1].mu))"))
    d = mahsq_chol(X, permutedims(hcat([f.mu for f in fm]...)), U; ctx = ctx)
    dens = d isa Array ? exp.(-.5 .* d) .* permutedims([_gda_coef(p, f.detS) for f in fm]) :
           exp.(-.5 .* d) .* _colocate_mat(reshape([_gda_coef(p, f.detS) for f in fm], 1, :), d)
    pred, posterior = _kde_posterior(wprior, dens, lev)
    (pred = pred, dens = dens, posterior = posterior)
end
"`predict(object::Lda, X)` — src/lda.jl:85-101: one jch_mahsq_chol call for all classes, with nfac = 1."
predict(object::Lda, X; ctx = default_ctx()) = _gda_predict(object.fm, object.fm[1].Uinv, object.wprior, object.lev, X, ctx)
"`predict(object::Qda, X)` — src/qda.jl:87-104: one jch_mahsq_chol call, one factor per class."
predict(object::Qda, X; ctx = default_ctx()) = _gda_predict(object.fm, object.Uinv, object.wprior, object.lev, X, ctx)

"`matW(X, y)` — src/matW.jl:44-75: (W, Wi, lev, ni); Wi p x p x nlev."
function matW(X, y; ctx = default_ctx())
    X = _in(X)
    lev, ni, _, order, cs = _gda_prepare(X, y, "unif")
    res = class_cov(X[order, :], cs; ctx = ctx)
    (W = res.W, Wi = res.Wi, lev = lev, ni = ni)
end
"`matB(X, y)` — src/matW.jl:23-29: (B, ct, lev, ni); the centres come from the device, B = covm(ct, mweight(ni)) is host work."
function matB(X, y; ctx = default_ctx())
    X = _in(X)
    lev, ni, _, order, cs = _gda_prepare(X, y, "unif")
    ct = class_cov(X[order, :], cs; want_Wi = false, want_W = false, ctx = ctx).ct
    w = ni ./ sum(ni)
    z = sqrt.(w) .* (ct .- permutedims(w) * ct)
    (B = transpose(z) * z, ct = ct, lev = lev, ni = ni)
end
"""`mahsqchol(X, Y[, Uinv])` — src/distances.jl:104-126, Y playing the centres (few rows): n x k where X lives.  Without Uinv: from the uncorrected
covariance of X, factored on the device.  x - y is taken before the product with Uinv."""
function mahsqchol(X, Y, Uinv = nothing; ctx = default_ctx())
    X = _in(X); Y = ensure_mat(Y)
    size(X, 2) == size(Y, 2) || throw(DimensionMismatch("X has $(size(X, 2)) columns, Y has $(size(Y, 2))"))
    if Uinv === nothing
        f = gauss_factor(class_cov(X, [0, size(X, 1)]; want_W = false, ctx = ctx).Wi[:, :, 1]; ctx = ctx)
        _gda_posdef(f.info[1], "mahsqchol")
        Uinv = f.Uinv
    end
    mahsq_chol(X, Y, ensure_mat(Uinv); ctx = ctx)
end

"""`lwplsravg_prepared(pm, q, Zq, X, k, h, tol, scal, lo, hi, typf)` — jch_lwplsravg_predict_prepared on a prepared handle `pm` (q responses; typf 0 = unif, 1 = shenk; `Zq`
= nothing: the handle's query map).  The levels are clamped as the library does (n = k).  Returns (pred q x m, pred_lv q x le x m, wlv le x m, rss_r hi x m,
rss_b hi x m, info m, ind k x m, dist k x m, w k x m) in the C layouts.  NOT EXECUTED in the build image (no Julia toolchain)."""
function lwplsravg_prepared(pm, q::Integer, Zq, X, k::Integer, h, tol, scal::Bool, lo::Integer, hi::Integer, typf::Integer; ctx = default_ctx())
    Q = _in(X); m, p = size(Q)
    kp = min(k, p); hic = min(hi, kp); loc_ = typf == 1 ? max(min(lo, kp), 1) : min(lo, kp); le = hic - loc_ + 1
    le >= 1 || throw(ArgumentError("no level left after the clamp"))
    pred = zeros(q, m); pred_lv = zeros(q, le, m); wlv = zeros(le, m); rss_r = zeros(max(hic, 1), m); rss_b = zeros(max(hic, 1), m); info = zeros(Int32, m)
    ind = zeros(Int32, k, m); dist = zeros(k, m); w = zeros(k, m)
    Zm = Zq === nothing ? Q : Zq
    GC.@preserve Zm Q pred pred_lv wlv rss_r rss_b info ind dist w begin
        check(ctx, ccall((:jch_lwplsravg_predict_prepared, LIB), Int32,
                         (Ptr{Cvoid}, Ptr{Cvoid}, Int32, Ptr{Float64}, Int64, Ptr{Float64}, Int64, Int64, Int32, Float64, Float64, Int32, Int32, Int32, Int32,
                          Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Int32}, Ptr{Int32}, Ptr{Float64}, Ptr{Float64}),
                         ctx.h, pm.h, _loc(Q), Zq === nothing ? Ptr{Float64}(C_NULL) : pointer(Zm), stride(Zm, 2), pointer(Q), m, stride(Q, 2), Int32(k),
                         Float64(h), Float64(tol), Int32(scal ? 1 : 0), Int32(lo), Int32(hi), Int32(typf), pointer(pred), pointer(pred_lv), pointer(wlv),
                         pointer(rss_r), pointer(rss_b), pointer(info), pointer(ind), pointer(dist), pointer(w)))
    end
    (pred = pred, pred_lv = pred_lv, wlv = wlv, rss_r = rss_r, rss_b = rss_b, info = info, ind = ind, dist = dist, w = w)
end

# ---- local PLS discrimination and the LWPLS models on global scores (src/lwplsrda.jl, src/lwplslda.jl, src/lwplsqda.jl, src/lwplsr_s.jl,
# src/lwplsrda_s.jl through src/locwlv.jl; DESIGN.md §25): one jch_lwplsda_predict_prepared per predict.  NOT EXECUTED in the build image (no
# Julia toolchain).
"""`knn_gda(T, tq, cls_nb, nlev; kind = "lda", prior = "unif", nlv)` — jch_knn_gda on host arrays: the Gaussian discriminants of m neighbourhoods
for all the nested score spaces 1:a, a in nlv, from one factorisation per covariance.  T: a_hi x k x m (the C layout [m][k][a_hi]), tq: a_hi x m,
cls_nb: k x m codes in 1:nlev.  Returns (post nlev x le x m, code le x m (1-based; 0 where info is 2), info le x m)."""
function knn_gda(T, tq, cls_nb, nlev; kind = "lda", prior = "unif", nlv = nothing, ctx = default_ctx())
    kind in ("lda", "qda") || throw(ArgumentError("kind must be \"lda\" or \"qda\""))
    prior in ("unif", "prop") || throw(ArgumentError("prior must be \"unif\" or \"prop\""))
    Tm = Array{Float64, 3}(T); qm = Matrix{Float64}(tq); c0 = Matrix{Int32}(cls_nb .- 1)
    a_hi, k, m = size(Tm)
    (size(qm) == (a_hi, m) && size(c0) == (k, m)) || throw(DimensionMismatch("knn_gda: T, tq and cls_nb do not fit"))
    rng = nlv === nothing ? (a_hi:a_hi) : (minimum(nlv):maximum(nlv))
    (first(rng) >= 1 && last(rng) <= a_hi) || throw(ArgumentError("nlv must lie in 1:$a_hi"))
    le = length(rng)
    post = zeros(nlev, le, m); code = zeros(Int32, le, m); info = zeros(Int32, le, m)
    GC.@preserve Tm qm c0 post code info begin
        check(ctx, ccall((:jch_knn_gda, LIB), Int32,
                         (Ptr{Cvoid}, Int32, Ptr{Float64}, Int64, Int32, Int32, Ptr{Float64}, Ptr{Int32}, Int32, Int32, Int32, Int32, Int32, Ptr{Float64},
                          Ptr{Int32}, Ptr{Int32}),
                         ctx.h, Int32(0), pointer(Tm), m, Int32(k), Int32(a_hi), pointer(qm), pointer(c0), Int32(nlev), Int32(kind == "lda" ? 1 : 2),
                         Int32(prior == "unif" ? 0 : 1), Int32(first(rng)), Int32(last(rng)), pointer(post), pointer(code), pointer(info)))
    end
    (post = post, code = Int.(code) .+ 1, info = Int.(info))
end

struct Lwplsrda                   # src/lwplsrda.jl:1-14
    X; y; fm; metric::String; h::Real; k::Int; nlv::Int; tol::Real; scal::Bool; verbose::Bool; lev; ni
end
struct LwplsLda                   # src/lwplslda.jl:1-15
    X; y; fm; metric::String; h::Real; k::Int; nlv::Int; prior::String; tol::Real; scal::Bool; verbose::Bool; lev; ni
end
struct LwplsQda                   # src/lwplsqda.jl:1-15
    X; y; fm; metric::String; h::Real; k::Int; nlv::Int; prior::String; tol::Real; scal::Bool; verbose::Bool; lev; ni
end
struct LwplsrS                    # src/lwplsr_s.jl:1-12
    T; Y; fm; metric::String; h::Real; k::Int; nlv::Int; tol::Real; scal::Bool; verbose::Bool
end
struct LwplsrdaS                  # src/lwplsrda_s.jl:1-12
    T; y; fm; metric::String; h::Real; k::Int; nlv::Int; tol::Real; scal::Bool; verbose::Bool
end
function _lwda_fit(X, y, nlvdis, metric, h, k, scal, ctx)
    _lw_check(metric, h, k)
    X = _in(X); yv = vec(Array(y)); dm = dummy(yv)
    size(X, 1) == length(yv) || throw(DimensionMismatch("X has $(size(X, 1)) rows, y has $(length(yv))"))
    fm = nlvdis == 0 ? nothing : plskern(X, _colocate_mat(dm.Y, X); nlv = nlvdis, scal = scal, ctx = ctx)   # src/lwplsrda.jl:89
    X, fm, dm.lev, [count(==(l), yv) for l in dm.lev]
end
"`lwplsrda(X, y; nlvdis, metric, h, k, nlv, tol = 1e-4, scal = false, verbose = false)` — src/lwplsrda.jl:81-94."
function lwplsrda(X, y; nlvdis, metric, h, k, nlv, tol = 1e-4, scal = false, verbose = false, ctx = default_ctx())
    X, fm, lev, ni = _lwda_fit(X, y, nlvdis, metric, h, k, scal, ctx)
    Lwplsrda(X, ensure_mat(y), fm, metric, h, k, nlv, tol, scal, verbose, lev, ni)
end
"`lwplslda(X, y; nlvdis, metric, h, k, nlv, prior = \"unif\", tol = 1e-4, scal = false, verbose = false)` — src/lwplslda.jl:84-97."
function lwplslda(X, y; nlvdis, metric, h, k, nlv, prior = "unif", tol = 1e-4, scal = false, verbose = false, ctx = default_ctx())
    prior in ("unif", "prop") || throw(ArgumentError("prior must be \"unif\" or \"prop\""))
    X, fm, lev, ni = _lwda_fit(X, y, nlvdis, metric, h, k, scal, ctx)
    LwplsLda(X, ensure_mat(y), fm, metric, h, k, nlv, prior, tol, scal, verbose, lev, ni)
end
"`lwplsqda(X, y; nlvdis, metric, h, k, nlv, prior = \"unif\", tol = 1e-4, scal = false, verbose = false)` — src/lwplsqda.jl:89-102."
function lwplsqda(X, y; nlvdis, metric, h, k, nlv, prior = "unif", tol = 1e-4, scal = false, verbose = false, ctx = default_ctx())
    prior in ("unif", "prop") || throw(ArgumentError("prior must be \"unif\" or \"prop\""))
    X, fm, lev, ni = _lwda_fit(X, y, nlvdis, metric, h, k, scal, ctx)
    LwplsQda(X, ensure_mat(y), fm, metric, h, k, nlv, prior, tol, scal, verbose, lev, ni)
end
"""`lwplsr_s(X, Y; nlv0, reduc = "pls", metric = "eucl", h, k, gamma = 1, psamp = 1, samp = "sys", nlv, tol = 1e-4, scal = false, verbose = false)` —
src/lwplsr_s.jl:115-141: kNN-LWPLSR on the n x nlv0 score table of a global reduction, nlv = min(nlv0, nlv)."""
function lwplsr_s(X, Y; nlv0, reduc = "pls", metric = "eucl", h, k, gamma = 1, psamp = 1, samp = "sys", nlv, tol = 1e-4, scal = false, verbose = false,
                  seed = nothing, ctx = default_ctx())
    _lw_check(metric, h, k)
    samp in ("sys", "random") || throw(ArgumentError("samp must be \"sys\" or \"random\""))
    X = _in(X); Y = _in(Y); n = size(X, 1)
    ms = Int64(round(psamp * n))
    s = ms >= n ? nothing : (samp == "sys" ? sampsys(vec(sum(Array(Y); dims = 2)); k = ms).train : randperm(MersenneTwister(seed), n)[1:ms])
    fm, T = _lw_reduce(X, Y, nothing, s, nlv0, reduc, gamma, scal, ctx)
    LwplsrS(T, Y, fm, metric, h, k, min(nlv0, nlv), tol, scal, verbose)
end
"""`lwplsrda_s(X, y; nlv0, reduc = "pls", metric = "eucl", h, k, gamma = 1, psamp = 1, samp = "cla", nlv, tol = 1e-4, scal = false, verbose = false)` —
src/lwplsrda_s.jl:77-105."""
function lwplsrda_s(X, y; nlv0, reduc = "pls", metric = "eucl", h, k, gamma = 1, psamp = 1, samp = "cla", nlv, tol = 1e-4, scal = false, verbose = false,
                    seed = nothing, ctx = default_ctx())
    _lw_check(metric, h, k)
    samp in ("cla", "random") || throw(ArgumentError("samp must be \"cla\" or \"random\""))
    X = _in(X); yv = vec(Array(y)); n = size(X, 1)
    ms = Int64(round(psamp * n))
    nlev = length(unique(yv))
    s = ms >= n ? nothing : (samp == "cla" ? sampcla(yv; k = max(Int64(round(ms / nlev)), 1), seed = seed).train : randperm(MersenneTwister(seed), n)[1:ms])
    Yd = reduc == "dkpls" ? _colocate_mat(dummy(yv).Y, X) : nothing
    fm, T = _lw_reduce(X, Yd, yv, s, nlv0, reduc, gamma, scal, ctx)
    LwplsrdaS(T, ensure_mat(y), fm, metric, h, k, min(nlv0, nlv), tol, scal, verbose)
end
# the engine: an Lwplsr record on the dummy table, prepared, then one call for search, weights, local fits and discriminants
function _lwda_predict(object, coords, fm, Q, nlv, kind, prior, ctx, who)
    yv = vec(Array(object.y)); dm = dummy(yv); nlev = length(dm.lev)
    cls = Vector{Int32}([searchsortedfirst(dm.lev, v) - 1 for v in yv])
    Q = _in(Q); m = size(Q, 1); n, p = size(coords)
    a = object.nlv
    rng = nlv === nothing ? (a:a) : (max(minimum(nlv), 0):min(maximum(nlv), a, p))
    (kind == 0 || first(rng) >= 1) || throw(ArgumentError("$who: a Gaussian discriminant needs at least one score column (nlv = 0 requested)"))
    eng = Lwplsr(coords, _colocate_mat(dm.Y, coords), fm, object.metric, object.h, object.k, object.nlv, object.tol, object.scal, false)
    pm = prepare(eng; ctx = ctx)
    Zq = pm.device_map ? Q : _colocate_mat(pm.qmap(Q), Q)
    cl = _colocate_vec(cls, Q)
    k = min(object.k, n); le = length(rng)
    code = zeros(Int32, le, m); info = zeros(Int32, le, m); post = zeros(nlev, le, m); ind = zeros(Int32, k, m); dist = zeros(k, m); w = zeros(k, m)
    GC.@preserve Zq Q cl code info post ind dist w begin
        check(ctx, ccall((:jch_lwplsda_predict_prepared, LIB), Int32,
                         (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Int32}, Int32, Int32, Int32, Int32, Ptr{Float64}, Int64, Ptr{Float64}, Int64, Int64, Int32, Float64,
                          Float64, Int32, Int32, Int32, Ptr{Int32}, Ptr{Float64}, Ptr{Int32}, Ptr{Float64}, Ptr{Float64}, Ptr{Int32}, Ptr{Float64},
                          Ptr{Float64}),
                         ctx.h, pm.h, pointer(cl), Int32(nlev), Int32(kind), Int32(prior == "unif" ? 0 : 1), _loc(Q),
                         pm.device_map ? Ptr{Float64}(C_NULL) : pointer(Zq), stride(Zq, 2), pointer(Q), m, stride(Q, 2), Int32(k), Float64(object.h),
                         Float64(object.tol), Int32(object.scal ? 1 : 0), Int32(first(rng)), Int32(last(rng)), pointer(code), pointer(post), pointer(info),
                         Ptr{Float64}(C_NULL), Ptr{Float64}(C_NULL), pointer(ind), pointer(dist), pointer(w)))
    end
    release!(pm)
    nbad = count(i -> any(==(2), info[:, i]), 1:m)
    nbad > 0 && @warn "$who: $nbad of $m neighbourhoods have a covariance that is not positive definite; their labels are the weighted vote"
    object.verbose && println(join(1:m, " "))
    preds = [reshape(dm.lev[Int.(code[i, :]) .+ 1], :, 1) for i in 1:le]
    posts = [permutedims(post[:, i, :]) for i in 1:le]
    (pred = le == 1 ? preds[1] : preds, listnn = [Int.(ind[:, i]) .+ 1 for i in 1:m], listd = [dist[:, i] for i in 1:m], listw = [w[:, i] for i in 1:m],
     posterior = le == 1 ? posts[1] : posts, info = permutedims(Int.(info)))
end
_colocate_vec(v::Vector{Int32}, like::Array) = v
_colocate_vec(v::Vector{Int32}, like) = copyto!(similar(like, Int32, length(v)), v)
"`predict(object::Lwplsrda, X; nlv)` — src/lwplsrda.jl:102-131."
predict(object::Lwplsrda, X; nlv = nothing, ctx = default_ctx()) = _lwda_predict(object, object.X, object.fm, X, nlv, 0, "unif", ctx, "predict(::Lwplsrda)")
"`predict(object::LwplsLda, X; nlv)` — src/lwplslda.jl:105-134."
predict(object::LwplsLda, X; nlv = nothing, ctx = default_ctx()) = _lwda_predict(object, object.X, object.fm, X, nlv, 1, object.prior, ctx, "predict(::LwplsLda)")
"`predict(object::LwplsQda, X; nlv)` — src/lwplsqda.jl:110-139."
predict(object::LwplsQda, X; nlv = nothing, ctx = default_ctx()) = _lwda_predict(object, object.X, object.fm, X, nlv, 2, object.prior, ctx, "predict(::LwplsQda)")
"`predict(object::LwplsrS, X; nlv)` — src/lwplsr_s.jl:149-178: `lwplsr` on the score table."
function predict(object::LwplsrS, X; nlv = nothing, ctx = default_ctx())
    eng = Lwplsr(object.T, object.Y, nothing, object.metric, object.h, object.k, object.nlv, object.tol, object.scal, object.verbose)
    _predict_lwplsr(eng, _lw_transform(object.fm, _in(X), ctx), nlv, ctx)
end
"`predict(object::LwplsrdaS, X; nlv)` — src/lwplsrda_s.jl:113-142."
function predict(object::LwplsrdaS, X; nlv = nothing, ctx = default_ctx())
    _lwda_predict(object, object.T, nothing, _lw_transform(object.fm, _in(X), ctx), nlv, 0, "unif", ctx, "predict(::LwplsrdaS)")
end

# ---- permutation importance and interval selection (src/viperm.jl, src/isel.jl) over jch_perm_fill / jch_perm_score_sums and jch_score_sums
# (include/jchemo_hip.h; DESIGN.md §26).  Row and column numbers are 1-based here; the C ABI, and the values of a permutation matrix, are
# 0-based.  NOT EXECUTED in the build image (no Julia toolchain).
_colocate_int(v::Array, like::Array) = v
_colocate_int(v::Array, like) = copyto!(similar(like, eltype(v), size(v)...), v)

"`perm_fill(m, ncols, seed)` — jch_perm_fill: m x ncols Int32 on the host, column j the permutation of 0 .. m - 1 for (seed, j - 1)."
function perm_fill(m::Integer, ncols::Integer, seed::Integer; ctx = default_ctx())
    (1 <= m < 2^31 && ncols >= 1) || throw(ArgumentError("perm_fill: 1 <= m < 2^31 and ncols >= 1"))
    perm = zeros(Int32, m, ncols)
    GC.@preserve perm check(ctx, ccall((:jch_perm_fill, LIB), Int32, (Ptr{Cvoid}, Int32, Ptr{Int32}, Int64, Int64, Int64, UInt64),
        ctx.h, Int32(0), pointer(perm), m, ncols, m, UInt64(seed)))
    perm
end

"""`perm_score_sums(X, Pred, Y, B; rows = nothing, perm = nothing, seed = 0)` — jch_perm_score_sums: 6 x q x (p + 1), [stat, response, column];
column j <= p holds the sums for the prediction in which column j of the held-out block was shuffled, column p + 1 the unshuffled ones.
`rows`: 1-based held-out rows (nothing: all rows); `perm`: m x p with 0-based values as `perm_fill` gives them (nothing: generated from `seed`)."""
function perm_score_sums(X, Pred, Y, B; rows = nothing, perm = nothing, seed = 0, ctx = default_ctx())
    X = _in(X); Pred = _colocate_mat(_in(Pred), X); Y = _colocate_mat(_in(Y), X)
    n, p = size(X); q = size(Y, 2)
    (size(Pred) == (n, q) && size(Y, 1) == n) || throw(DimensionMismatch("X is $n x $p, Pred $(size(Pred)), Y $(size(Y))"))
    Bm = Matrix{Float64}(ensure_mat(B))
    size(Bm) == (p, q) || throw(DimensionMismatch("B is $(size(Bm)), expected ($p, $q)"))
    rows0 = rows === nothing ? nothing : _colocate_int(Vector{Int64}(vec(Array(rows)) .- 1), X)
    m = rows0 === nothing ? n : length(rows0)
    perm0 = perm === nothing ? nothing : _colocate_int(Matrix{Int32}(Array(perm)), X)
    (perm0 === nothing || size(perm0) == (m, p)) || throw(DimensionMismatch("perm is $(size(perm0)), expected ($m, $p)"))
    sums = zeros(6, q, p + 1)
    GC.@preserve X Pred Y Bm rows0 perm0 check(ctx, ccall((:jch_perm_score_sums, LIB), Int32,
        (Ptr{Cvoid}, Int32, Ptr{Float64}, Int64, Int64, Int64, Ptr{Int64}, Int64, Ptr{Float64}, Int64, Ptr{Float64}, Int64, Int64, Ptr{Float64}, Int64,
         Ptr{Int32}, Int64, UInt64, Ptr{Float64}),
        ctx.h, _loc(X), pointer(X), n, p, stride(X, 2), rows0 === nothing ? Ptr{Int64}(C_NULL) : pointer(rows0), m, pointer(Pred), max(stride(Pred, 2), n),
        pointer(Y), q, max(stride(Y, 2), n), pointer(Bm), p, perm0 === nothing ? Ptr{Int32}(C_NULL) : pointer(perm0), m, UInt64(seed), sums))
    sums
end

# per replication (held-out rows, 64-bit permutation seed) from one stream; `s` pins the rows
function _vi_splits(n, nval, nrep, seed, s)
    (1 <= nval < n) || throw(ArgumentError("psamp leaves $nval of $n rows for the test set"))
    (s === nothing || length(s) == nrep) || throw(ArgumentError("s has $(length(s)) index vectors for $nrep replications"))
    rng = seed === nothing ? Random.default_rng() : MersenneTwister(seed)
    pseeds = rand(rng, UInt64, nrep)                        # the seeds first: pinning the rows leaves them what they were
    map(1:nrep) do i
        rows = s === nothing ? sort(randperm(rng, n)[1:nval]) : Vector{Int64}(vec(s[i]))
        (rows, pseeds[i])
    end
end
_vi_reuse(fun) = fun === plskern || fun === plsnipals || fun === plssimp || fun === plsrosa || fun === plswold
_vi_weights(fun) = _vi_reuse(fun) || fun === pcr
_vi_fast(fun) = _vi_weights(fun) || fun === covselr
function _vi_full_B(fm, p)
    B = Matrix{Float64}(coef(fm).B)
    hasproperty(fm, :sel) || return B
    full = zeros(p, size(B, 2)); full[fm.sel.sel, :] .= B
    full
end

"""
    viperm(X, Y; perm = 50, psamp = 1/3, score = rmsep, fun, seed = nothing, s = nothing, kwargs...)

src/viperm.jl:74-110.  Returns `(imp = p x q, res = p x q x perm)`.  `seed` seeds the stream the held-out rows and one 64-bit permutation
seed per replication are drawn from; `s`, a vector of `perm` index vectors, pins the rows.  Where `fun` is one of `plskern, plsnipals,
plssimp, plsrosa, plswold, pcr, covselr` and `score` one of `msep, rmsep, ssr, bias, r2, cor2`, a replication is one fit with weight 0 on the
held-out rows (X is never copied; `covselr` gets gathered rows), one `predict` over X and one jch_perm_score_sums.  Anything else runs the
reference's loop, on the same permutations.
"""
function viperm(X, Y; perm = 50, psamp = 1/3, score = rmsep, fun, seed = nothing, s = nothing, ctx = default_ctx(), kwargs...)
    X = _in(X); Y = _colocate_mat(_in(Y), X); n, p = size(X); q = size(Y, 2)
    nval = Int64(round(psamp * n))
    splits = _vi_splits(n, nval, perm, seed, s)
    fast = score isa ScoreFun && _vi_fast(fun)
    res = zeros(p, q, perm)
    _same_x[] = Int32(0)
    for (i, (rows, pseed)) in enumerate(splits)
        keep = setdiff(1:n, rows)
        if fast
            fm = if _vi_weights(fun)
                w = ones(n); w[rows] .= 0.0
                try fun(X, Y, w; kwargs...) catch; _same_x[] = Int32(0); rethrow() end
            else
                fun(X[keep, :], Y[keep, :]; kwargs...)
            end
            _vi_reuse(fun) && (_same_x[] = Int32(8))        # the later fits of this call see the same X (JCH_REUSE_XCOPY)
            S = perm_score_sums(X, predict(fm, X).pred, Y, _vi_full_B(fm, p); rows = rows, seed = pseed, ctx = ctx)
            res[:, :, i] .= _score_from_sums(score.name, S[:, :, 1:p]) .- _score_from_sums(score.name, S[:, :, (p + 1):(p + 1)])
        else
            Xval = X[rows, :]; Yval = Y[rows, :]
            fm = fun(X[keep, :], Y[keep, :]; kwargs...)
            score0 = vec(collect(score(predict(fm, Xval).pred, Yval)))
            zs = perm_fill(length(rows), p, pseed; ctx = ctx)
            for j in 1:p
                col = Xval[:, j]
                Xval[:, j] .= col[Int.(zs[:, j]) .+ 1]
                res[j, :, i] .= vec(collect(score(predict(fm, Xval).pred, Yval))) .- score0
                Xval[:, j] .= col
            end
        end
    end
    _same_x[] = Int32(0)
    (imp = reshape(sum(res; dims = 3) ./ perm, p, q), res = res)
end

"""
    isel(X, Y, wl = 1:nco(X); rep = 1, nint = 5, psamp = 1/3, score = rmsep, fun, seed = nothing, s = nothing, kwargs...)

src/isel.jl:76-129.  Returns `(res, res0, res_rep, res0_rep, int)` with the reference's columns `lo, up, mid, y1 ... yq`.  The split works as
in `viperm`.  Where `fun` takes weights and `score` is a named one, an interval is a view of the column-major X (same leading dimension, no
copy) fitted with weight 0 on the held-out rows and scored from jch_score_sums with the held-out mask.
"""
function isel(X, Y, wl = 1:size(ensure_mat(X), 2); rep = 1, nint = 5, psamp = 1/3, score = rmsep, fun, seed = nothing, s = nothing, ctx = default_ctx(), kwargs...)
    X = _in(X); Y = _colocate_mat(_in(Y), X); n, p = size(X); q = size(Y, 2)
    nint = Int64(nint)
    z = collect(round.(range(1, p + 1; length = nint + 1)))
    int = [z[1:nint] z[2:(nint + 1)] .- 1]
    int = Int64.(hcat(int, round.(sum(int; dims = 2) ./ 2)))
    nval = Int64(round(psamp * n))
    splits = _vi_splits(n, nval, rep, seed, s)
    masked = score isa ScoreFun && _vi_weights(fun)
    res_rep = zeros(nint, q, rep); res0_rep = zeros(1, q, rep)
    for (i, (rows, _)) in enumerate(splits)
        keep = setdiff(1:n, rows)
        held = zeros(n); held[rows] .= 1.0
        w = 1.0 .- held
        Xcal = masked ? nothing : X[keep, :]; Ycal = masked ? nothing : Y[keep, :]
        Xval = masked ? nothing : X[rows, :]; Yval = masked ? nothing : Y[rows, :]
        function one(u)
            if masked
                Xu = view(X, :, u)
                fm = fun(Xu, Y, w; kwargs...)
                return _score_from_sums(score.name, _score_sums(predict(fm, Xu).pred, Y, held, ctx))[1:1, :]
            end
            fm = fun(Xcal[:, u], Ycal; kwargs...)
            reshape(collect(score(predict(fm, Xval[:, u]).pred, Yval)), 1, :)
        end
        res0_rep[:, :, i] .= one(1:p)
        for j in 1:nint
            res_rep[j:j, :, i] .= one(int[j, 1]:int[j, 2])
        end
    end
    dat = (lo = wl[int[:, 1]], up = wl[int[:, 2]], mid = wl[int[:, 3]])
    zres = sum(res_rep; dims = 3)[:, :, 1] ./ rep; zres0 = sum(res0_rep; dims = 3)[:, :, 1] ./ rep
    ycols(A) = NamedTuple{_ynames(q)}(Tuple(A[:, k] for k in 1:q))
    (res = _table(merge(dat, ycols(zres))), res0 = _table(ycols(zres0)), res_rep = res_rep, res0_rep = res0_rep, int = int)
end

end # module
