# NEPMI355X.jl -- Julia binding of libnepmi355.so (include/nepmi355.h) for NonlinearEigenproblems.jl.
#
# This is the file INTEGRATION.md describes, shipped as source: `include` it from src/NonlinearEigenproblems.jl after
# NEPSolver (it refers to the parent package's modules with `..`).  It subtypes the reference's four plug-in seams
# (AbstractSPMF / LinSolver + LinSolverCreator / IterativeSolvers.OrthogonalizationMethod / MatrixIntegrator, SURVEY.md
# section 8b) and forwards to the C ABI with `ccall`; the solver drivers (iar, tiar, resinv, nleigs, contour_beyn) then run
# unchanged.  Julia is not installed in the build image of this repository, so the file has NOT been executed there; every C
# symbol it calls is exercised by the ctypes host (nonlineareigenproblems.jl_amd/_lib.py) in the `-m gpu` test suite, and
# tests/test_host_logic.py::test_julia_binding_symbols_exist checks that each `ccall` target below is exported by the
# library and declared in include/nepmi355.h; test_julia_ccall_signatures_match_the_header parses every `ccall` type tuple and
# compares arity, scalar widths and pointer-ness with the C prototype (Julia is absent from the GPU box as well: probed, round 4).
#
# Library search: put the directory of libnepmi355.so on LD_LIBRARY_PATH (or set `const LIB` to its absolute path).

# src/backends/MI355X.jl  -- to be `include`d from src/NonlinearEigenproblems.jl after NEPSolver
module MI355X
using ..NEPCore, ..NEPTypes, ..LinSolvers, ..NEPSolver
using SparseArrays, LinearAlgebra
import IterativeSolvers
import ..NEPCore: compute_Mlincomb, compute_Mlincomb!, compute_Mder, compute_MM, size, issparse
import ..NEPTypes: get_Av, get_fv
import ..LinSolvers: lin_solve, create_linsolver
import ..NEPSolver: integrate_interval, iar, tiar

const LIB = "libnepmi355"
chk(st) = st == 0 || error(unsafe_string(ccall((:nep_last_error, LIB), Cstring, ())))

# ---- device buffers (column-major ComplexF64, exactly Matrix{ComplexF64}) --------------------------------
mutable struct DevBuf; ptr::Ptr{Cvoid}; rows::Int; cols::Int; end
function DevBuf(rows, cols)
    p = Ref{Ptr{Cvoid}}(C_NULL); chk(ccall((:nep_dev_alloc, LIB), Cint, (Ref{Ptr{Cvoid}}, Csize_t), p, 16rows*cols))
    b = DevBuf(p[], rows, cols); finalizer(x -> ccall((:nep_dev_free, LIB), Cint, (Ptr{Cvoid},), x.ptr), b); b
end
upload!(b::DevBuf, A::StridedVecOrMat{ComplexF64}) =
    chk(ccall((:nep_upload, LIB), Cint, (Ptr{Cvoid}, Ptr{ComplexF64}, Csize_t, Ptr{Cvoid}), b.ptr, A, sizeof(A), C_NULL))
download(b::DevBuf) = (A = Matrix{ComplexF64}(undef, b.rows, b.cols);
    chk(ccall((:nep_download, LIB), Cint, (Ptr{ComplexF64}, Ptr{Cvoid}, Csize_t, Ptr{Cvoid}), A, b.ptr, sizeof(A), C_NULL)); A)

# ---- NEP seam: an AbstractSPMF whose compute_* run on the device ------------------------------------------
# replaces SPMF_NEP (src/NEPTypes.jl:162-170); wraps any AbstractSPMF (SPMF_NEP, PEP, DEP, SPMFSumNEP ...) via get_Av/get_fv.
# Julia's type parameters are invariant: PEP <: AbstractSPMF{AbstractMatrix} (src/types_poly.jl:31) and SPMFSumNEP <:
# AbstractSPMF{AbstractMatrix} (src/NEPTypes.jl:838) while eltype(get_Av(.)) is a concrete SparseMatrixCSC -- a field
# `org::AbstractSPMF{T}` with T = eltype(Av) cannot hold them (nlevp_native_gun IS an SPMFSumNEP(PEP, SPMF_NEP),
# src/gallery_extra/NLEVP_native.jl:4-18).  So the wrapper is declared the way those two are: no parameter, supertype
# AbstractSPMF{AbstractMatrix}, and the wrapped problem in an unparametrised field.
mutable struct DeviceSPMF <: AbstractSPMF{AbstractMatrix}
    org::AbstractSPMF             # kept for compute_Mder (host, one-off per shift) and get_fv
    handle::Ptr{Cvoid}
    n::Int
    refine_hint::Dict{ComplexF64,Int}   # refinement sweeps nep_iar_run settled on, per shift (nep_iar_result.refine_plan)
end
function DeviceSPMF(org::AbstractSPMF)
    Av = get_Av(org); n = size(org, 1); mt = length(Av)
    # Julia stores CSC; the CSR of A is the CSC of transpose(A)
    At = [SparseMatrixCSC(transpose(sparse(A))) for A in Av]
    rp = [Int32.(A.colptr .- 1) for A in At]; ci = [Int32.(A.rowval .- 1) for A in At]
    vals = [eltype(A) <: Real ? Float64.(A.nzval) : ComplexF64.(A.nzval) for A in At]
    isc  = Int32[eltype(A) <: Real ? 0 : 1 for A in At]
    h = Ref{Ptr{Cvoid}}(C_NULL)
    GC.@preserve rp ci vals chk(ccall((:nep_spmf_create, LIB), Cint,
        (Int64, Int32, Ptr{Ptr{Int32}}, Ptr{Ptr{Int32}}, Ptr{Ptr{Cvoid}}, Ptr{Int32}, Ref{Ptr{Cvoid}}),
        n, mt, pointer.(rp), pointer.(ci), [Ptr{Cvoid}(pointer(v)) for v in vals], isc, h))
    d = DeviceSPMF(org, h[], n, Dict{ComplexF64,Int}())
    finalizer(x -> ccall((:nep_spmf_destroy, LIB), Cint, (Ptr{Cvoid},), x.handle), d); d
end
size(d::DeviceSPMF) = (d.n, d.n); size(d::DeviceSPMF, i) = d.n
issparse(d::DeviceSPMF) = true
get_Av(d::DeviceSPMF) = get_Av(d.org); get_fv(d::DeviceSPMF) = get_fv(d.org)
compute_Mder(d::DeviceSPMF, λ::Number, i::Integer = 0) = compute_Mder(d.org, λ, i)   # host: feeds factorize

# coefficient block C[j,i] = a_j f_i^(j-1)(λ): f_i(S)[:,1] of the bidiagonal S of src/NEPTypes.jl:993-1004
function coeff_block(d::DeviceSPMF, λ, a::Vector)
    k = length(a); a = ComplexF64.(a); z = a .== 0; a1 = copy(a); a1[z] .= 1
    S = diagm(0 => fill(ComplexF64(λ), k), -1 => (a1[2:k] ./ a1[1:k-1]) .* (1:k-1))
    C = hcat([a1[1] .* (k == 1 ? [f(ComplexF64(λ))] : f(S)[:, 1]) for f in get_fv(d)]...)
    C[z, :] .= 0; Matrix{ComplexF64}(C)
end
function compute_Mlincomb(d::DeviceSPMF, λ::Number, V::AbstractVecOrMat, a::Vector = ones(size(V, 2)))
    Vm = Matrix{ComplexF64}(reshape(V, size(V, 1), :)); k = size(Vm, 2)
    dV = DevBuf(d.n, k); upload!(dV, Vm); dz = DevBuf(d.n, 1); C = coeff_block(d, λ, a)
    chk(ccall((:nep_mlincomb, LIB), Cint, (Ptr{Cvoid}, Int32, Ptr{ComplexF64}, Ptr{Cvoid}, Int64, Ptr{Cvoid}, Ptr{Cvoid}),
              d.handle, k, C, dV.ptr, d.n, dz.ptr, C_NULL))
    z = vec(download(dz))                       # a new Vector of length n, V untouched (test/spmf.jl:26-30)
    # the reference's element type (test/compute_types.jl; src/NEPTypes.jl:985-999: promote_type of λ, a, the SPMF's Ftype and V;
    # Ftype is ComplexF64 unless the problem was built with another one): the device computes in ComplexF64 throughout, a real
    # result type is returned as its real part
    TT = promote_type(eltype(V), typeof(λ), eltype(a), ftype(d.org))
    TT <: Real ? Vector{TT}(real.(z)) : (TT == ComplexF64 ? z : Vector{TT}(z))
end
ftype(::SPMF_NEP{T,Ftype}) where {T,Ftype} = Ftype
ftype(::AbstractSPMF) = ComplexF64
compute_Mlincomb!(d::DeviceSPMF, λ::Number, V::AbstractVecOrMat, a::Vector = ones(size(V, 2))) = compute_Mlincomb(d, λ, V, a)
# device-resident overload: V already lives in HBM (a DevBuf, e.g. the basis kept by DeviceDGKS below) -- nothing is uploaded,
# the result stays on the device; `cols` selects the leading columns (iar: column k of the basis *is* the n x k block)
function compute_Mlincomb(d::DeviceSPMF, λ::Number, V::DevBuf, a::Vector = ones(V.cols); z::DevBuf = DevBuf(d.n, 1), ldv = V.rows)
    C = coeff_block(d, λ, a)
    chk(ccall((:nep_mlincomb, LIB), Cint, (Ptr{Cvoid}, Int32, Ptr{ComplexF64}, Ptr{Cvoid}, Int64, Ptr{Cvoid}, Ptr{Cvoid}),
              d.handle, length(a), C, V.ptr, ldv, z.ptr, C_NULL)); z
end

# ---- LinSolver seam (src/LinSolvers.jl:64-91 is the reference's own extension recipe) ---------------------
# A DeviceLinSolver is what FactorizeLinSolver is in the reference (src/LinSolvers.jl:109-122): factors of M(λ) made once
# and, like `Afact \ x` with control[8] = umfpack_refinements, every solve followed by iterative refinement with UMFPACK's
# stopping rule.  `spmf` / `cf` / `cabs` (handle, f_t(λ), |f_t(λ)|) are what the refinement needs to form r = b - M(λ)x on the
# device; a solver made for a NEP that is not a DeviceSPMF has spmf == C_NULL and solves without refinement.
mutable struct DeviceLinSolver <: LinSolver
    handle::Ptr{Cvoid}; n::Int
    spmf::Ptr{Cvoid}; cf::Vector{ComplexF64}; cabs::Vector{Float64}; umfpack_refinements::Int
    resident::Bool                 # lin_solve returns a DevBuf (left in HBM) instead of a host array
    keep::Any                      # keeps the DeviceSPMF (owner of `spmf`) alive as long as the solver
end
DeviceLinSolver(h::Ptr{Cvoid}, n::Integer) = DeviceLinSolver(h, n, C_NULL, ComplexF64[], Float64[], 0, false, nothing)
struct DeviceLinSolverCreator <: LinSolverCreator
    umfpack_refinements::Int       # same meaning and default as FactorizeLinSolverCreator (src/LinSolverCreators.jl:62-75)
    resident::Bool
end
DeviceLinSolverCreator(; umfpack_refinements = 10, resident = false) = DeviceLinSolverCreator(umfpack_refinements, resident)
function create_linsolver(creator::DeviceLinSolverCreator, nep, λ)
    F = lu(SparseMatrixCSC{ComplexF64,Int}(compute_Mder(nep, λ)))     # UMFPACK on the host, one-off per shift
    # UMFPACK: F.L * F.U == (F.Rs .* A)[F.p, F.q].  nep_lu_create_csc takes SparseMatrixCSC as it is (0-based Int32 indices);
    # (Pr b)[perm_r[i]] = b[i] -> perm_r = invperm(p) - 1 ;  x[i] = y[perm_c[i]] -> perm_c = invperm(q) - 1 ;
    # the row scaling Rs is applied to every right-hand side inside the first kernel (nep_lu_set_row_scale)
    L, U = F.L, F.U; n = size(nep, 1)
    pr = Int32.(invperm(F.p) .- 1); pc = Int32.(invperm(F.q) .- 1); h = Ref{Ptr{Cvoid}}(C_NULL)
    chk(ccall((:nep_lu_create_csc, LIB), Cint, (Int64, Ptr{Int32}, Ptr{Int32}, Ptr{ComplexF64}, Ptr{Int32}, Ptr{Int32},
        Ptr{ComplexF64}, Ptr{Int32}, Ptr{Int32}, Ref{Ptr{Cvoid}}), n, Int32.(L.colptr .- 1), Int32.(L.rowval .- 1),
        L.nzval, Int32.(U.colptr .- 1), Int32.(U.rowval .- 1), U.nzval, pr, pc, h))
    chk(ccall((:nep_lu_set_row_scale, LIB), Cint, (Ptr{Cvoid}, Ptr{Float64}), h[], Float64.(F.Rs)))
    s = DeviceLinSolver(h[], n)
    if nep isa DeviceSPMF                                              # refinement needs M(λ)x on the device
        s.spmf = nep.handle; s.keep = nep; s.umfpack_refinements = creator.umfpack_refinements
        s.cf = ComplexF64[f(ComplexF64(λ)) for f in get_fv(nep)]; s.cabs = abs.(s.cf)
    end
    s.resident = creator.resident
    finalizer(x -> ccall((:nep_lu_destroy, LIB), Cint, (Ptr{Cvoid},), x.handle), s); s     # stream-ordered: safe with solves in flight
end
# Beyn factors N matrices of ONE sparsity pattern (method_beyncontour.jl:89-94): when UMFPACK returns the same L/U patterns and
# permutations (symmetric strategy, diagonal pivots) only the numeric part is repeated -- either implicitly (nep_lu_create_csc
# recognises the pattern by hash and reuses the symbolic analysis) or explicitly on an existing handle:
refactor!(s::DeviceLinSolver, F) = chk(ccall((:nep_lu_refactor, LIB), Cint, (Ptr{Cvoid}, Ptr{ComplexF64}, Ptr{ComplexF64}),
                                           s.handle, F.L.nzval, F.U.nzval))
# ... or without ANY further host factorisation: the numeric LU itself on the GPU.  From the first UMFPACK factorisation of a
# pattern (diagonal pivots: F.p == F.q) build the plan once; every later matrix of the pattern -- the next shift, the N nodes of
# contour_beyn in one batch -- needs only its values (Rs = 1 here: scale A yourself or call umfpack with scaling off):
function device_plan(s::DeviceLinSolver, F, A::SparseMatrixCSC)
    pr = Int32.(invperm(F.p) .- 1); pc = Int32.(invperm(F.q) .- 1); L, U = F.L, F.U; h = Ref{Ptr{Cvoid}}(C_NULL)
    chk(ccall((:nep_lu_refac_create, LIB), Cint, (Ptr{Cvoid}, Int64, Ptr{Int32}, Ptr{Int32}, Ptr{Int32}, Ptr{Int32}, Ptr{Int32},
        Ptr{Int32}, Ptr{Int32}, Ptr{Int32}, Ref{Ptr{Cvoid}}), s.handle, s.n, Int32.(L.colptr .- 1), Int32.(L.rowval .- 1),
        Int32.(U.colptr .- 1), Int32.(U.rowval .- 1), pr, pc, Int32.(A.colptr .- 1), Int32.(A.rowval .- 1), h))
    h[]                                                       # NEP_ERR_UNSUPPORTED (-5): keep factorising on the host
end
function factor_on_device(plan, A::SparseMatrixCSC{ComplexF64}; expected_solves = 50, growth = 1e6)
    h = Ref{Ptr{Cvoid}}(C_NULL); health = zeros(3)
    rc = ccall((:nep_lu_factor_dev, LIB), Cint, (Ptr{Cvoid}, Ptr{ComplexF64}, Int32, Float64, Ptr{Float64}, Ptr{Cvoid},
               Ref{Ptr{Cvoid}}, Ptr{Cvoid}), plan, A.nzval, expected_solves, growth, health, C_NULL, h, C_NULL)
    rc == -3 && return nothing                                # pivot breakdown / growth with the stored pivots: lu(A) on the host
    chk(rc); DeviceLinSolver(h[], size(A, 1))
end
# the N quadrature nodes of contour_beyn (method_beyncontour.jl:89-94) in ONE batched factorisation, M(λ_b) = Σ_t f_t(λ_b) A_t formed on
# the GPU: D = device copy (DevBuf) of the nnz(A) x m_t term values on the union pattern of A (entry-major: D[t, e] in Julia's
# column-major terms), uploaded once per NEP; per call only the m_t x N coefficient block travels
function factor_nodes_on_device(plan, D::DevBuf, fv, λs::Vector{ComplexF64}, n; growth = 1e6)
    Cf = ComplexF64[f(λ) for f in fv, λ in λs]               # m_t x N, column b = coefficients of node b
    hs = fill(C_NULL, length(λs)); health = zeros(3, length(λs))
    chk(ccall((:nep_lu_factor_dev_batch_terms, LIB), Cint, (Ptr{Cvoid}, Int32, Ptr{Cvoid}, Int32, Ptr{ComplexF64}, Int32, Float64,
        Ptr{Float64}, Ptr{Ptr{Cvoid}}, Ptr{Cvoid}), plan, length(λs), D.ptr, length(fv), Cf, 1, growth, health, hs, C_NULL))
    [h == C_NULL ? nothing : DeviceLinSolver(h, n) for h in hs]    # nothing: that node is factorised on the host (lu(M(λ_b)))
end
# lin_solve: a new array shaped like b, matrix right-hand sides allowed (method_beyncontour.jl:21-23,91-93); `tol` is a
# hint that direct solvers ignore (src/LinSolvers.jl:135-137).  A resident solver (DeviceLinSolverCreator(resident = true))
# returns the DevBuf instead; `*(::DevBuf, ::Number)` below keeps the unchanged integrand `Tv(g(t))*gp(t)` of
# method_beyncontour.jl:96-97 on the device, and integrate_interval accepts either kind of value.
const PROBE = Ref{Any}(nothing)                   # (objectid, size, host copy, DevBuf) of the last uploaded right-hand-side block
clear_probe!() = (PROBE[] = nothing)              # drop the cached block (frees its HBM at the next GC)
function upload_rhs(b::AbstractVecOrMat, n)
    B = Matrix{ComplexF64}(reshape(b, n, :)); dB = DevBuf(n, size(B, 2)); upload!(dB, B); dB
end
function lin_solve(s::DeviceLinSolver, b::AbstractVecOrMat; tol = 0)
    p = PROBE[]
    # the cached block is reused only for the same array WITH THE SAME CONTENTS.  Base.hash(::AbstractArray) is NOT a content check
    # (it samples O(log N) entries of arrays of 8192 or more elements): the kept host copy is compared entry by entry (`==` on two
    # 5 MB blocks: one pass over host memory, against an upload of the same 5 MB over PCIe) -- a caller that refills its matrix in
    # place, wholly or in part, gets the new values solved, not the old ones
    if s.resident && b isa AbstractMatrix && p !== nothing && p[1] == objectid(b) && p[2] == size(b) && p[3] == b
        dB = DevBuf(s.n, size(b, 2))               # contour solvers pass the SAME probe block Vh at every node: uploaded once
        chk(ccall((:nep_dev_copy, LIB), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Csize_t, Ptr{Cvoid}), dB.ptr, p[4].ptr, 16s.n*dB.cols, C_NULL))
    else
        dB = upload_rhs(b, s.n)
        if s.resident && b isa AbstractMatrix
            keep = DevBuf(s.n, dB.cols)
            chk(ccall((:nep_dev_copy, LIB), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Csize_t, Ptr{Cvoid}), keep.ptr, dB.ptr, 16s.n*dB.cols, C_NULL))
            PROBE[] = (objectid(b), size(b), copy(b), keep)
        end
    end
    lin_solve!(s, dB)
    s.resident && return dB
    X = download(dB); b isa AbstractVector ? vec(X) : X
end
# device-resident right-hand sides, solved in place: x = A^{-1} b, then per column UMFPACK's refinement loop
# (src/LinSolvers.jl:114-122: control[8] = umfpack_refinements).  r = b - M(λ)x and the componentwise backward error
# omega = max_i |r_i| / (Σ_t |f_t(λ)| (|A_t||x|)_i + |b_i|) come from nep_cw_backward_error in one pass over the matrices;
# the update x <- x + A^{-1} r is nep_lu_solve_add.  Stop when omega <= 2 eps, when omega stops halving (a step that made it
# worse is taken back) or after umfpack_refinements steps -- the rule nonlineareigenproblems.jl_amd/linsolvers.py:630-646 runs.
function lin_solve!(s::DeviceLinSolver, dB::DevBuf; scale = 1.0)
    n = s.n; nrhs = dB.cols
    if s.spmf == C_NULL || s.umfpack_refinements <= 0
        chk(ccall((:nep_lu_solve, LIB), Cint, (Ptr{Cvoid}, Int32, Ptr{Cvoid}, Int64, Ptr{Cvoid}, Int64, Float64, Ptr{Cvoid}),
                  s.handle, nrhs, dB.ptr, n, dB.ptr, n, scale, C_NULL))
        return dB
    end
    x = DevBuf(n, 1); xprev = DevBuf(n, 1); r = DevBuf(n, 1); ω = Ref{Float64}(0.0)
    for j in 1:nrhs
        b = dB.ptr + 16n*(j-1)                                        # column j of the right-hand sides, kept until the end
        chk(ccall((:nep_lu_solve, LIB), Cint, (Ptr{Cvoid}, Int32, Ptr{Cvoid}, Int64, Ptr{Cvoid}, Int64, Float64, Ptr{Cvoid}),
                  s.handle, 1, b, n, x.ptr, n, 1.0, C_NULL))
        ωprev = Inf
        for step in 0:s.umfpack_refinements
            chk(ccall((:nep_cw_backward_error, LIB), Cint, (Ptr{Cvoid}, Ptr{Float64}, Ptr{ComplexF64}, Ptr{Cvoid}, Ptr{Cvoid},
                      Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ref{Float64}, Ptr{Cvoid}),
                      s.spmf, s.cabs, s.cf, x.ptr, b, C_NULL, C_NULL, r.ptr, ω, C_NULL))
            ω[] <= 2eps(Float64) && break
            if ω[] > ωprev / 2
                ω[] > ωprev && chk(ccall((:nep_dev_copy, LIB), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Csize_t, Ptr{Cvoid}),
                                         x.ptr, xprev.ptr, 16n, C_NULL))       # the last step made it worse: take it back
                break
            end
            step == s.umfpack_refinements && break
            ωprev = ω[]
            chk(ccall((:nep_dev_copy, LIB), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Csize_t, Ptr{Cvoid}), xprev.ptr, x.ptr, 16n, C_NULL))
            chk(ccall((:nep_lu_solve_add, LIB), Cint, (Ptr{Cvoid}, Int32, Ptr{Cvoid}, Int64, Ptr{Cvoid}, Int64, Ptr{Cvoid}, Int64,
                      Float64, Ptr{Cvoid}), s.handle, 1, r.ptr, n, x.ptr, n, x.ptr, n, 1.0, C_NULL))     # x <- x + A^{-1} r
        end
        chk(ccall((:nep_dev_copy, LIB), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Csize_t, Ptr{Cvoid}), b, x.ptr, 16n, C_NULL))
    end
    scale == 1.0 || chk(ccall((:nep_scal, LIB), Cint, (Int64, ComplexF64, Ptr{Cvoid}, Ptr{Cvoid}), n*nrhs, ComplexF64(scale), dB.ptr, C_NULL))
    dB
end
# X * α on the device (a new DevBuf): what `Tv(g(t))*gp(t)` of method_beyncontour.jl:97 becomes for a resident solver
function Base.:*(X::DevBuf, α::Number)
    Y = DevBuf(X.rows, X.cols)
    chk(ccall((:nep_dev_copy, LIB), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Csize_t, Ptr{Cvoid}), Y.ptr, X.ptr, 16X.rows*X.cols, C_NULL))
    chk(ccall((:nep_scal, LIB), Cint, (Int64, ComplexF64, Ptr{Cvoid}, Ptr{Cvoid}), X.rows*X.cols, ComplexF64(α), Y.ptr, C_NULL)); Y
end
Base.size(X::DevBuf) = (X.rows, X.cols)

# ---- orthogonalisation seam: a new IterativeSolvers.OrthogonalizationMethod (cf. test/iar.jl:7-17) ----------
# The reference drivers pass HOST views (`view(V,1:nk,1:k)`, src/method_iar.jl:107; `Z[:,1:k]`, method_tiar.jl:128) and a
# method INSTANCE (`orthmethod=DGKS()`, src/method_iar.jl:50; the user recipe test/iar.jl:13-17 dispatches on `::DoubleGS`):
# `iar(nep, orthmethod=DeviceDGKS())`.  DeviceDGKS therefore owns a device mirror of the basis: the drivers only ever append one column per step (the
# normalised w of the previous call), so call k uploads that ONE column, never the basis (iar m=100: 16 MB instead of 1.6 GB).
struct DeviceDGKS <: IterativeSolvers.OrthogonalizationMethod end
mutable struct BasisMirror; buf::DevBuf; ld::Int; ncols::Int; w::DevBuf; end
const MIRROR = Ref{Union{Nothing,BasisMirror}}(nothing)
reset_basis!() = (MIRROR[] = nothing)                    # call before a new iar/tiar run
function IterativeSolvers.orthogonalize_and_normalize!(V::StridedMatrix{ComplexF64}, w::StridedVector{ComplexF64},
                                                        h::StridedVector{ComplexF64}, ::DeviceDGKS)
    rows, k = size(V); ldmax = size(parent(V), 1); kmax = size(parent(V), 2)
    (stride(V, 1) == 1 && stride(w, 1) == 1 && stride(h, 1) == 1) || error("DeviceDGKS: unit row stride expected")
    m = MIRROR[]
    if m === nothing || m.ld != ldmax || k < m.ncols
        m = BasisMirror(DevBuf(ldmax, kmax), ldmax, 0, DevBuf(ldmax, 1)); MIRROR[] = m
        chk(ccall((:nep_dev_memset, LIB), Cint, (Ptr{Cvoid}, Int32, Csize_t, Ptr{Cvoid}), m.buf.ptr, 0, 16ldmax*kmax, C_NULL))
    end
    # Column j of the view starts stride(V, 2) ELEMENTS of the parent after column j-1.  iar passes view(V, 1:1:n*(k+1), 1:k)
    # (method_iar.jl:96) with rows < ldmax: such a view is not contiguous, and `pointer(V, i::Int)` takes i as a linear index in
    # the VIEW's index space (rows per column), so a parent-space offset there addresses the wrong column.  Byte arithmetic on
    # the address of the view's first element has one meaning only.
    for j in m.ncols+1:k                                    # columns not yet mirrored (one per call after the first)
        chk(ccall((:nep_upload, LIB), Cint, (Ptr{Cvoid}, Ptr{ComplexF64}, Csize_t, Ptr{Cvoid}),
                  m.buf.ptr + 16ldmax*(j-1), pointer(V) + 16stride(V, 2)*(j-1), 16rows, C_NULL))
    end
    m.ncols = k
    chk(ccall((:nep_upload, LIB), Cint, (Ptr{Cvoid}, Ptr{ComplexF64}, Csize_t, Ptr{Cvoid}), m.w.ptr, w, 16rows, C_NULL))
    β = Ref{Float64}(0); np = Ref{Int32}(0)
    chk(ccall((:nep_orth, LIB), Cint, (Ptr{Cvoid}, Int64, Int64, Int32, Ptr{Int64}, Ptr{Cvoid}, Ptr{ComplexF64}, Ref{Float64},
        Int32, Ref{Int32}, Ptr{Cvoid}), m.buf.ptr, ldmax, rows, k, C_NULL, m.w.ptr, h, β, 0, np, C_NULL))
    chk(ccall((:nep_download, LIB), Cint, (Ptr{ComplexF64}, Ptr{Cvoid}, Csize_t, Ptr{Cvoid}), w, m.w.ptr, 16rows, C_NULL))
    β[]                                                   # w and h updated in place, returns ||w|| before normalisation
end

# ---- iar / tiar on the device pipeline: `iar(nep; ...)` / `tiar(nep; ...)` with nep::DeviceSPMF, caller unchanged ----------
# Julia dispatches on the NEP type: these two methods are more specific than the reference's `iar(::Type{T}, nep::NEP; ...)`
# (src/method_iar.jl:46-64) / `tiar(::Type{T}, nep::NEP; ...)` (src/method_tiar.jl:52-70), take the same keywords with the same
# defaults and return what those return.  iar is ONE ccall of nep_iar_run (csrc/iar_run.hip): recurrence, Hessenberg
# eigen-decompositions, Ritz blocks, residual batches, convergence test, sort and extraction all stay in the library on three
# streams -- the pipeline bench.py measures (the Python host calls the same entry point).  What the library cannot do is taken
# from the reference's own method: a request outside the fast path (T other than ComplexF64, proj_solve, an error measure that is
# a user function, MGS or a user orthogonalisation, another linear-solver creator, maxit > 128) or a run that reports
# NEP_ERR_RETRY goes to `invoke(iar, Tuple{Type{T},NEP}, ...)`, i.e. the reference's loop over the four seams above.
const NEP_ERR_RETRY = -6; const NEP_ERR_NOCONV = -7
struct IarOpts                       # nep_iar_opts, include/nepmi355.h (same field order and widths)
    maxit::Int32; check_error_every::Int32; orth_method::Int32; umfpack_refinements::Int32; errmeasure::Int32; refine_hint::Int32
    tol::Float64; neigs::Float64; sigma::ComplexF64; gamma::ComplexF64
end
struct IarResult                     # nep_iar_result
    k::Int32; nconv::Int32; nret::Int32; refine_plan::Int32; refine_hint_off::Int32; retry_reason::Int32
end
orth_code(::IterativeSolvers.DGKS) = Int32(0)
orth_code(::DeviceDGKS) = Int32(0)
orth_code(::IterativeSolvers.ClassicalGramSchmidt) = Int32(1)
orth_code(::IterativeSolvers.ModifiedGramSchmidt) = Int32(2)
orth_code(x) = nothing
# (kind, ||A_t||_F) of an error measure the library evaluates itself: src/errmeasure.jl:91-101 (Default), :114,128-130 (Residual),
# :174-190 (StandardSPMF); a user function or an error measure of another problem: nothing
native_errmeasure(e::DefaultErrmeasure, nep) = native_errmeasure(e.errm, nep)
native_errmeasure(e::StandardSPMFErrmeasure, nep) = e.nep === nep ? (Int32(1), Vector{Float64}(e.coeffs)) : nothing
native_errmeasure(e::ResidualErrmeasure, nep) = e.nep === nep ? (Int32(0), Float64[]) : nothing
native_errmeasure(e, nep) = nothing
# the reference's default creator (DefaultLinSolverCreator = FactorizeLinSolverCreator, src/LinSolverCreators.jl:62-122,196) asked
# of a DeviceSPMF means "factorise once, solve many, UMFPACK refinement": the device solver with the same umfpack_refinements
device_creator(c::DeviceLinSolverCreator) = c
device_creator(c::FactorizeLinSolverCreator) = (isempty(c.recycled_factorizations) && c.max_factorizations == 0) ?
    DeviceLinSolverCreator(umfpack_refinements = c.umfpack_refinements, resident = true) : nothing
device_creator(c) = nothing
# row j+1 = f_t^(j)(σ), j = 0..m: first column of f_t at the bidiagonal matrix σ I + subdiag(1..m) (the device the reference's
# DerSPMF uses, src/NEPTypes.jl:1108-1128)
function derivative_table(d::DeviceSPMF, σ::ComplexF64, m::Int)
    S = diagm(0 => fill(σ, m + 1), -1 => ComplexF64.(1:m))
    hcat([Vector{ComplexF64}(f(S)[:, 1]) for f in get_fv(d)]...)
end
# nep_fv_eval: F[t + (s-1) mt] = f_t(λ_s); runs on the calling thread, inside the ccall of nep_iar_run
function fv_eval(ctx::Ptr{Cvoid}, nlam::Int32, lam::Ptr{ComplexF64}, F::Ptr{ComplexF64})::Int32
    try
        fs = unsafe_pointer_to_objref(ctx)::Vector{Any}; mt = length(fs)
        for s in 1:nlam, t in 1:mt
            unsafe_store!(F, ComplexF64(fs[t](unsafe_load(lam, s))), t + (s - 1) * mt)
        end
        return Int32(0)
    catch
        return Int32(1)                # an exception must not unwind through the C frames: the run ends with NEP_ERR_ARG
    end
end
Base.Matrix(b::DevBuf) = download(b); Base.Array(b::DevBuf) = download(b)

iar(nep::DeviceSPMF; params...) = iar(ComplexF64, nep; params...)
function iar(::Type{T}, nep::DeviceSPMF;
             orthmethod = IterativeSolvers.DGKS(), maxit = 30, linsolvercreator = DefaultLinSolverCreator(),
             tol = eps(real(T)) * 10000, neigs = 6, errmeasure::ErrmeasureType = DefaultErrmeasure(nep), σ = zero(T), γ = one(T),
             v = randn(real(T), size(nep, 1)), logger = 0, check_error_every = 1, proj_solve = false,
             inner_solver_method = DefaultInnerSolver(), inner_logger = 0) where {T<:Number}
    reference() = invoke(iar, Tuple{Type{T},NEP}, T, nep; orthmethod = orthmethod, maxit = maxit,
                         linsolvercreator = linsolvercreator, tol = tol, neigs = neigs, errmeasure = errmeasure, σ = σ, γ = γ, v = v,
                         logger = logger, check_error_every = check_error_every, proj_solve = proj_solve,
                         inner_solver_method = inner_solver_method, inner_logger = inner_logger)
    ek = native_errmeasure(errmeasure, nep); oc = orth_code(orthmethod); dc = device_creator(linsolvercreator)
    if T != ComplexF64 || proj_solve || ek === nothing || oc === nothing || oc > 1 || dc === nothing || maxit > 128
        return reference()
    end
    n = nep.n; m = Int(maxit); σc = ComplexF64(σ); γc = ComplexF64(γ)
    M0inv = create_linsolver(dc, nep, σc)::DeviceLinSolver            # src/method_iar.jl:84
    fD = derivative_table(nep, σc, m); mt = size(fD, 2)
    Ctab = ComplexF64[γc^j / j * fD[j + 1, t] for j in 1:m, t in 1:mt]   # m x mt: α_j / j f_t^(j)(σ), α = γ.^(0:m) (:83,:101)
    v0 = Vector{ComplexF64}(v)
    refine = M0inv.umfpack_refinements > 0 && !isempty(M0inv.cf)
    opts = IarOpts(m, check_error_every, oc, refine ? M0inv.umfpack_refinements : 0, ek[1], get(nep.refine_hint, σc, -1),
                   Float64(tol), Float64(neigs), σc, γc)
    res = Ref(IarResult(0, 0, 0, -1, 0, 0))
    λ = zeros(ComplexF64, m); Q = Matrix{ComplexF64}(undef, n, m); err = fill(NaN, m, m)
    V = DevBuf(n * (m + 1), m + 1)                                     # the Krylov basis stays on the device (1.6 GB for gun, m = 100)
    fs = Any[f for f in get_fv(nep)]
    cb = @cfunction(fv_eval, Int32, (Ptr{Cvoid}, Int32, Ptr{ComplexF64}, Ptr{ComplexF64}))
    st = GC.@preserve fs ccall((:nep_iar_run, LIB), Cint,
        (Ptr{Cvoid}, Ptr{Cvoid}, Int64, Ref{IarOpts}, Ptr{ComplexF64}, Ptr{ComplexF64}, Int32, Ptr{Float64}, Ptr{ComplexF64},
         Ptr{Float64}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{ComplexF64}, Ptr{Cvoid}, Ptr{ComplexF64}, Ptr{Float64}, Ptr{Cvoid},
         Ref{IarResult}, Ptr{Cvoid}),
        nep.handle, M0inv.handle, n, Ref(opts), v0, Ctab, mt, refine ? M0inv.cabs : C_NULL, refine ? M0inv.cf : C_NULL,
        ek[1] == 1 ? ek[2] : C_NULL, cb, pointer_from_objref(fs), λ, C_NULL, Q, err, V.ptr, res, C_NULL)
    r = res[]
    if r.refine_hint_off != 0
        delete!(nep.refine_hint, σc)
    elseif r.refine_plan >= 0
        nep.refine_hint[σc] = r.refine_plan
    end
    st == NEP_ERR_RETRY && return reference()      # a step wanted more refinement sweeps / DGKS passes than were enqueued (rare)
    (st == 0 || st == NEP_ERR_NOCONV) || chk(st)
    k = Int(r.k); nret = Int(r.nret)
    if st == NEP_ERR_NOCONV                         # src/method_iar.jl:163-175
        msg = "Number of iterations exceeded. maxit=$(maxit)."
        r.nconv < 3 && (msg = string(msg, "Try to change the inner_solver_method for better performance."))
        throw(NoConvergenceException(λ[1:nret], Q[:, 1:nret], err[k, 1:nret], msg))
    end
    V.cols = k                                      # V[:,1:k] of src/method_iar.jl:181, left in HBM: Matrix(V) downloads it
    return λ[1:nret], Q[:, 1:nret], V
end

# tiar: the reference's loop (src/method_tiar.jl:116-239) with the basis Z resident in HBM.  Per step: K1 on Z with the k x k
# tensor slice folded into the coefficient block (z = Σ_t A_t Z (B diag(α) fD_t): no n x k product is formed), K5 with UMFPACK's
# refinement in place, K6 (DGKS / CGS / MGS) with h and β returned, the O(k³) tensor algebra on the host; per check: eig(H_k) on
# the host, ONE K7 GEMM Q = Z (a[1,1:k,1:k]ᵀ W) and ONE K2 residual batch for all k pairs.
tiar(nep::DeviceSPMF; params...) = tiar(ComplexF64, nep; params...)
function tiar(::Type{T}, nep::DeviceSPMF;
              orthmethod = IterativeSolvers.DGKS(), maxit = 30, linsolvercreator = DefaultLinSolverCreator(),
              tol = eps(real(T)) * 10000, neigs = 6, errmeasure::ErrmeasureType = DefaultErrmeasure(nep), σ = zero(T), γ = one(T),
              v = randn(real(T), size(nep, 1)), logger = 0, check_error_every = 1, proj_solve = false,
              inner_solver_method = DefaultInnerSolver(), inner_logger = 0) where {T}
    ek = native_errmeasure(errmeasure, nep); oc = orth_code(orthmethod); dc = device_creator(linsolvercreator)
    if T != ComplexF64 || proj_solve || ek === nothing || oc === nothing || dc === nothing
        return invoke(tiar, Tuple{Type{T},NEP}, T, nep; orthmethod = orthmethod, maxit = maxit,
                      linsolvercreator = linsolvercreator, tol = tol, neigs = neigs, errmeasure = errmeasure, σ = σ, γ = γ, v = v,
                      logger = logger, check_error_every = check_error_every, proj_solve = proj_solve,
                      inner_solver_method = inner_solver_method, inner_logger = inner_logger)
    end
    n = nep.n; m = Int(maxit); σc = ComplexF64(σ); γc = ComplexF64(γ)
    n < m && throw(LostOrthogonalityException("Loss of orthogonality in the matrix Z. The problem size is too small, use iar instead."))
    a = zeros(ComplexF64, m + 1, m + 1, m + 1); t = zeros(ComplexF64, m + 1); H = zeros(ComplexF64, m + 1, m)
    α = γc .^ (0:m); α[1] = 0
    M0inv = create_linsolver(dc, nep, σc)::DeviceLinSolver
    fD = derivative_table(nep, σc, m); fv = get_fv(nep); mt = length(fv)
    Z = DevBuf(n, m + 1)
    chk(ccall((:nep_dev_memset, LIB), Cint, (Ptr{Cvoid}, Int32, Csize_t, Ptr{Cvoid}), Z.ptr, 0, 16n * (m + 1), C_NULL))
    v0 = Vector{ComplexF64}(v); v0 ./= norm(v0)
    chk(ccall((:nep_upload, LIB), Cint, (Ptr{Cvoid}, Ptr{ComplexF64}, Csize_t, Ptr{Cvoid}), Z.ptr, v0, 16n, C_NULL))
    a[1, 1, 1] = 1
    z = DevBuf(n, 1); err = fill(NaN, m + 1, m + 1); conv_eig_hist = zeros(Int, m + 1)
    λ = ComplexF64[]; QT = DevBuf(1, 1); idx = Int[]; kq = 0
    k = 1; conv_eig = 0
    while k <= m && conv_eig < neigs
        # y[:,2:k+1] = Z[:,1:k] * transpose(a[1:k,k,1:k]) ./ (1:k)' and compute_Mlincomb!(nep, σ, y, α) in one K1 call (:120-125)
        B = transpose(a[1:k, k, 1:k]) ./ transpose(1:k)
        C = Matrix{ComplexF64}((B .* transpose(α[2:k+1])) * fD[2:k+1, :])              # k x mt
        chk(ccall((:nep_mlincomb, LIB), Cint, (Ptr{Cvoid}, Int32, Ptr{ComplexF64}, Ptr{Cvoid}, Int64, Ptr{Cvoid}, Ptr{Cvoid}),
                  nep.handle, k, C, Z.ptr, n, z.ptr, C_NULL))
        lin_solve!(M0inv, z; scale = -1.0)                                               # :126
        zk = Z.ptr + 16n * k                                                             # column k+1 of Z
        chk(ccall((:nep_dev_copy, LIB), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Csize_t, Ptr{Cvoid}), zk, z.ptr, 16n, C_NULL))
        hk = zeros(ComplexF64, k); β = Ref{Float64}(0); np = Ref{Int32}(0)               # :129-130
        chk(ccall((:nep_orth, LIB), Cint, (Ptr{Cvoid}, Int64, Int64, Int32, Ptr{Int64}, Ptr{Cvoid}, Ptr{ComplexF64}, Ref{Float64},
                  Int32, Ref{Int32}, Ptr{Cvoid}), Z.ptr, n, n, k, C_NULL, zk, hk, β, oc, np, C_NULL))
        t[1:k] = hk; t[k+1] = β[]
        # tensor orthogonalisation, twice (:131-183)
        g = zeros(ComplexF64, k + 1, k + 1)
        g[1, :] = t[1:k+1]
        for l in 1:k+1, i in 2:k+1
            g[i, l] = a[i-1, k, l] / (i - 1)
        end
        h = zeros(ComplexF64, k)
        for l in 1:k; h .+= a[1:k, 1:k, l]' * g[1:k, l]; end
        for l in 1:k; g[1:k+1, l] .-= a[1:k+1, 1:k, l] * h; end
        hh = zeros(ComplexF64, k)
        for l in 1:k; hh .+= a[1:k, 1:k, l]' * g[1:k, l]; end
        for l in 1:k; g[1:k+1, l] .-= a[1:k+1, 1:k, l] * hh; end
        h .+= hh; βt = norm(g)
        H[1:k, k] = h; H[k+1, k] = βt
        a[1:k+1, k+1, 1:k+1] = g ./ βt
        if rem(k, check_error_every) == 0 || k == m
            D, W = eigen(H[1:k, 1:k])                                                   # :185
            λ = σc .+ γc ./ D
            Bq = Matrix{ComplexF64}(transpose(a[1, 1:k, 1:k]) * W)                       # Q = Z[:,1:k] * Bq  (:186-187)
            QT = DevBuf(k, n); kq = k                                                    # k x n column-major = n x k ROW-major
            chk(ccall((:nep_gemm_ts, LIB), Cint, (Ptr{Cvoid}, Int64, Int64, Int32, Ptr{ComplexF64}, Int64, Int32, Ptr{Cvoid}, Int64,
                      Int32, Ptr{Cvoid}), Z.ptr, n, n, k, Bq, k, k, QT.ptr, k, 1, C_NULL))
            F = ComplexF64[f(λ[s]) for f in fv, s in 1:k]                                # mt x k
            rn = zeros(k); qn = zeros(k)
            chk(ccall((:nep_resid_batch, LIB), Cint, (Ptr{Cvoid}, Int32, Ptr{ComplexF64}, Ptr{Cvoid}, Int64, Ptr{Float64},
                      Ptr{Float64}, Ptr{Cvoid}), nep.handle, k, F, QT.ptr, k, rn, qn, C_NULL))
            e = ek[1] == 1 ? rn ./ (qn .* vec(transpose(ek[2]) * abs.(F))) : rn ./ qn  # src/errmeasure.jl:128-130,186-190
            conv_eig = count(<(tol), e)
            idx = sortperm(e); err[k, 1:k] = e[idx]                                      # :222-223
            if k == m || conv_eig >= neigs                                               # :225-229
                nrof = Int(min(length(λ), neigs)); λ = λ[idx[1:nrof]]; idx = idx[1:nrof]
            end
            conv_eig_hist[k] = conv_eig
        end
        k += 1
    end
    k -= 1
    function columns(cols)                        # the chosen columns of the row-major Ritz block as a host n x length(cols) matrix
        isempty(cols) && return Matrix{ComplexF64}(undef, n, 0)
        Qd = DevBuf(n, length(cols))
        chk(ccall((:nep_rowmajor_to_colmajor, LIB), Cint, (Int64, Int32, Ptr{Cvoid}, Int64, Ptr{Int32}, Int32, Ptr{Cvoid}, Int64,
                  Ptr{Cvoid}), n, kq, QT.ptr, kq, Int32.(cols .- 1), length(cols), Qd.ptr, n, C_NULL))
        download(Qd)
    end
    if conv_eig < neigs && neigs != Inf                                                  # :241-251
        msg = "Number of iterations exceeded. maxit=$(maxit)."
        conv_eig < 3 && (msg = string(msg, " Check that σ is not an eigenvalue."))
        throw(NoConvergenceException(λ, columns(idx[1:length(λ)]), err[k, 1:length(λ)], msg))
    end
    nc = min(length(λ), conv_eig)
    Z.cols = k
    return λ[1:nc], columns(idx[1:nc]), Z, conv_eig_hist
end

# ---- rectangular operators and plain dense products (low-rank NLEIGS factors, waveguide Schur complement) ---
struct DevCSR; handle::Ptr{Cvoid}; rows::Int; cols::Int; end
function DevCSR(A::SparseMatrixCSC{<:Number,Int})        # e.g. P.UU' and hcat(P.L...) of rk_nep.jl:128-152, nep.C1 / nep.C2T of the WEP
    At = SparseMatrixCSC{ComplexF64,Int}(transpose(A)); h = Ref{Ptr{Cvoid}}(C_NULL)       # CSC of A' = CSR of A
    chk(ccall((:nep_csr_create, LIB), Cint, (Int64, Int64, Ptr{Int32}, Ptr{Int32}, Ptr{ComplexF64}, Ref{Ptr{Cvoid}}),
              size(A, 1), size(A, 2), Int32.(At.colptr .- 1), Int32.(At.rowval .- 1), At.nzval, h))
    d = DevCSR(h[], size(A)...); finalizer(x -> ccall((:nep_csr_destroy, LIB), Cint, (Ptr{Cvoid},), x.handle), d); d
end
# y = α A x + β z   (method_nleigs.jl:430 `P.UU' * wc[i0b:i0e] + β[ii+1]/ξ[ii]*wc[i1b:i1e]`; Waveguide.jl:561 `x_int - nep.C1*Pinv(...)`)
csr_mv!(y::DevBuf, A::DevCSR, α, x::DevBuf, β, z::DevBuf) =
    chk(ccall((:nep_csr_mv, LIB), Cint, (Ptr{Cvoid}, ComplexF64, Ptr{Cvoid}, ComplexF64, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}),
              A.handle, ComplexF64(α), x.ptr, ComplexF64(β), z.ptr, y.ptr, C_NULL))
# C = α op(A) op(B) + β C  (op: 0 none, 1 transpose, 2 adjoint): the dense DFT / sine transforms that replace fft! / ifft! in
# waveguide_preconditioner.jl:163-219;  y = d .* (A' x): R(nep, Rinv(nep, v) ./ coeffs) of Waveguide.jl:270-294
zgemm!(C::DevBuf, ta, tb, α, A::DevBuf, B::DevBuf, β) =
    chk(ccall((:nep_zgemm, LIB), Cint, (Int32, Int32, Int32, Int32, Int32, ComplexF64, Ptr{Cvoid}, Int64, Ptr{Cvoid}, Int64,
              ComplexF64, Ptr{Cvoid}, Int64, Ptr{Cvoid}), ta, tb, C.rows, C.cols, ta == 0 ? A.cols : A.rows, ComplexF64(α),
              A.ptr, A.rows, B.ptr, B.rows, ComplexF64(β), C.ptr, C.rows, C_NULL))
gemv_hd!(y::DevBuf, A::DevBuf, x::DevBuf, d::Union{DevBuf,Nothing}) =
    chk(ccall((:nep_gemv_hd, LIB), Cint, (Ptr{Cvoid}, Int64, Int64, Int32, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}),
              A.ptr, A.rows, A.rows, A.cols, x.ptr, d === nothing ? C_NULL : d.ptr, y.ptr, C_NULL))
# C[:, e] = β C[:, e] + W F[:, e] for every column e of F (one column per matrix entry, its J samples or term values): the
# coefficients of ChebPEP (types_cheb_pep.jl:94-114, W = Tmat) and interpolate (types_poly.jl:121-164, W = inv(V)); W is K x J
interp_coeffs!(C::DevBuf, W::Matrix{ComplexF64}, F::DevBuf, β::Integer = 0) =
    chk(ccall((:nep_interp_coeffs, LIB), Cint, (Int64, Int32, Int32, Ptr{Cvoid}, Int64, Int32, Ptr{ComplexF64}, Ptr{Cvoid}, Int32,
              Ptr{Cvoid}, Int64, Ptr{Cvoid}), F.cols, F.rows, C.rows, F.ptr, F.rows, 1, W, C_NULL, β, C.ptr, C.rows, C_NULL))
# K14: F[i, j, t] = W[:, i]' * A_t * V[:, j] for every term of the SPMF in one pass over the stacked CSR: the loop of
# dot(y, nep.A[i]*x) in compute_rf (compute_rf_wrapper.jl:115-118), the forms behind y' M(λ) x = Σ_t f_t(λ) (y' A_t x), and the
# matrices W' A_t V of a projected NEP (src/NEPTypes.jl:724-741)
function biforms(d::DeviceSPMF, W::DevBuf, V::DevBuf)
    F = Array{ComplexF64,3}(undef, W.cols, V.cols, length(get_Av(d)))
    chk(ccall((:nep_spmf_biforms, LIB), Cint, (Ptr{Cvoid}, Int32, Ptr{Cvoid}, Int64, Int32, Ptr{Cvoid}, Int64, Ptr{ComplexF64},
              Ptr{Cvoid}, Ptr{Cvoid}), d.handle, W.cols, W.ptr, W.rows, V.cols, V.ptr, V.rows, F, C_NULL, C_NULL)); F
end

# ---- quadrature seam (src/method_contour_common.jl:46,61-94): nodes sharded over ranks, RCCL all-gather ------
# One Julia process per GPU (e.g. `mpiexec -n 8 julia ...` with MPI.jl only as the launcher / unique-id carrier).
abstract type MatrixTrapezoidalSharded <: MatrixIntegrator end
mutable struct Comm; handle::Ptr{Cvoid}; rank::Int; world::Int; end
const COMM = Ref{Union{Nothing,Comm}}(nothing)
function init_comm!(rank::Integer, world::Integer, bcast!)      # bcast!(buf::Vector{UInt8}) broadcasts from rank 0, e.g. MPI.Bcast!
    chk(ccall((:nep_set_device, LIB), Cint, (Int32,), rank))      # one GPU per rank of the node
    uid = zeros(UInt8, 128)
    rank == 0 && chk(ccall((:nep_comm_unique_id, LIB), Cint, (Ptr{UInt8},), uid))
    bcast!(uid); h = Ref{Ptr{Cvoid}}(C_NULL)
    chk(ccall((:nep_comm_create, LIB), Cint, (Int32, Int32, Ptr{UInt8}, Ref{Ptr{Cvoid}}), rank, world, uid, h))
    COMM[] = Comm(h[], rank, world)
end
# Same contract as the reference method (src/method_contour_common.jl:61-94): returns I[:,:,j] ~ int f g_j as an Array{T,3},
# for ANY integrand the unchanged drivers build -- `f(t) = Tv(g(t))*gp(t)` of method_beyncontour.jl:89-98 returns a host
# Matrix with the default (host-array) lin_solve and a DevBuf with a resident DeviceLinSolver; both are accepted, nothing else
# is asked of f.  Rank r owns the nodes i = r+1, r+1+P, ...; the shape of an integrand value comes from the first value a
# rank computes, and a rank without a node (N < P) learns it from the others through the same collective.
function integrate_interval(::Type{MatrixTrapezoidalSharded}, ::Type{T}, f, gv, a, b, N, logger) where {T<:Number}
    c = COMM[]; c === nothing && error("MI355X.init_comm! has not been called on this rank")
    h = (b - a) / N; t = range(a, stop = b - h, length = N); m = size(gv, 1)
    G = ComplexF64[gv[j](t[i]) for i in 1:N, j in 1:m]          # the cheap part (method_contour_common.jl:71-78)
    S = nothing                                                 # DevBuf (rows*cols) x m, partial sums of this rank
    shape = (0, 0)
    for i in (c.rank+1):c.world:N
        X = f(t[i])                                             # the expensive part: one factorisation + one block solve
        dX = X isa DevBuf ? X : upload_rhs(X, size(X, 1))       # host value: one upload per node (gun, k = 32: 5 MB)
        if S === nothing
            shape = (dX.rows, dX.cols); S = DevBuf(dX.rows * dX.cols, m)
            chk(ccall((:nep_dev_memset, LIB), Cint, (Ptr{Cvoid}, Int32, Csize_t, Ptr{Cvoid}), S.ptr, 0, 16S.rows*m, C_NULL))
        end
        for j in 1:m                                            # S[:,:,j] += X * g_j(t_i)   (method_contour_common.jl:88-90)
            chk(ccall((:nep_axpy, LIB), Cint, (Int64, ComplexF64, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}),
                      S.rows, G[i, j], dX.ptr, S.ptr + 16S.rows*(j-1), C_NULL))
        end
    end
    # every rank must enter the collective with a block of the same length: agree on the shape first.  Each rank that owns a
    # node contributes (rows, cols, 1), the others zeros; the rank-ordered sum divided by its last entry is the shape.
    meta = DevBuf(3, 1); upload!(meta, reshape(ComplexF64[shape[1], shape[2], S === nothing ? 0 : 1], 3, 1))
    chk(ccall((:nep_allgather_sum, LIB), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Int64, Ptr{Cvoid}, Ptr{Cvoid}), c.handle, meta.ptr, 3, meta.ptr, C_NULL))
    mt = real.(vec(download(meta))); mt[3] > 0 || error("integrate_interval: no rank owns a quadrature node (N = $N)")
    n = round(Int, mt[1] / mt[3]); k = round(Int, mt[2] / mt[3])
    if S === nothing                                            # a rank without a node contributes zeros
        S = DevBuf(n * k, m)
        chk(ccall((:nep_dev_memset, LIB), Cint, (Ptr{Cvoid}, Int32, Csize_t, Ptr{Cvoid}), S.ptr, 0, 16S.rows*m, C_NULL))
    end
    # the only exchange of data: all-gather of the partial block over xGMI + sum in rank order -> bit-identical on every rank
    chk(ccall((:nep_allgather_sum, LIB), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Int64, Ptr{Cvoid}, Ptr{Cvoid}),
              c.handle, S.ptr, S.rows * m, S.ptr, C_NULL))
    chk(ccall((:nep_scal, LIB), Cint, (Int64, ComplexF64, Ptr{Cvoid}, Ptr{Cvoid}), S.rows * m, ComplexF64(h), S.ptr, C_NULL))
    Array{T,3}(reshape(download(S), n, k, m))                   # S * h as src/method_contour_common.jl:93 returns it
end
end # module
