/*
 * nepmi355.h -- C ABI of libnepmi355.so, the MI355X (gfx950) inner linear-algebra backend
 * for NEP-PACK-style nonlinear eigensolvers.
 *
 * The reference (nep-pack/NonlinearEigenproblems.jl, 100 % Julia) has no FFI; its plug-in
 * seams are four small abstract types.  Every entry point below names
 * the reference interface it replaces (file:line under /root/reference).  A Julia binding
 * reaches these with `ccall((:nep_xxx, "libnepmi355"), Cint, (...), ...)` -- see INTEGRATION.md.
 *
 * Conventions
 *   - plain C types only; no C++/torch types cross this boundary.
 *   - every function returns int32 status: 0 = ok, <0 = error (nep_last_error() has text);
 *     nothing throws.
 *   - `d`-prefixed pointers are DEVICE pointers (from nep_dev_alloc, or any HIP allocation of
 *     the same process, e.g. a torch tensor's data_ptr()); `h`-prefixed pointers are HOST.
 *   - dense blocks are complex128 (re,im interleaved), COLUMN-MAJOR with explicit leading
 *     dimension, i.e. exactly Julia's Matrix{ComplexF64} layout -- unless a parameter says
 *     row-major.
 *   - `stream` is a hipStream_t passed as void* (NULL = default stream).  Functions whose
 *     results are written to host memory synchronise that stream before returning; all others
 *     are asynchronous with respect to the host.
 *   - a handle is used by one host thread at a time; distinct handles may be used concurrently.
 */
#ifndef NEPMI355_H
#define NEPMI355_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct { double re, im; } nep_cdouble;
typedef struct nep_spmf nep_spmf; /* device-resident SPMF: stacked CSR of A_1..A_mt */
typedef struct nep_lu nep_lu;     /* device-resident sparse LU factors + solve schedule */
typedef struct nep_comm nep_comm; /* one rank of the multi-GPU exchange (RCCL communicator) */
typedef void* nep_stream;

#define NEP_OK 0
#define NEP_ERR_HIP -1      /* a HIP runtime call failed (no device, OOM, launch failure) */
#define NEP_ERR_ARG -2      /* invalid argument */
#define NEP_ERR_SINGULAR -3 /* zero pivot met in the triangular solve (SingularException analogue) */
#define NEP_ERR_BREAKDOWN -4 /* orthogonalisation breakdown: ||w|| == 0 */
#define NEP_ERR_UNSUPPORTED -5 /* the request does not fit this code path (internal: callers fall back) */
#define NEP_ERR_RETRY -6       /* nep_iar_run: the recorded refinement / DGKS / eig status of a step asks for more than the
                                * enqueued work did -- re-run through the step-synchronous route (nep_iar_result.retry_reason) */
#define NEP_ERR_NOCONV -7      /* nep_iar_run: fewer than `neigs` pairs converged within maxit steps; the best pairs ARE returned
                                * (the reference throws NoConvergenceException(lambda, Q, err, msg), src/method_iar.jl:163-175) */

/* ---- library / device ---------------------------------------------------------------- */
int32_t nep_version(void);
/* digest (sha256 prefix) of the sources the library was built from; "unknown" for builds outside build.py */
const char* nep_src_digest(void);
const char* nep_last_error(void);
int32_t nep_device_count(int32_t* n);
int32_t nep_set_device(int32_t dev);
int32_t nep_device_name(char* buf, int32_t buflen);

/* ---- raw device memory (for hosts without their own HIP allocator, e.g. Julia) ------- */
int32_t nep_dev_alloc(void** dptr, size_t bytes);
int32_t nep_dev_free(void* dptr);
int32_t nep_dev_memset(void* dptr, int32_t value, size_t bytes, nep_stream stream);
int32_t nep_upload(void* ddst, const void* hsrc, size_t bytes, nep_stream stream);   /* sync */
int32_t nep_download(void* hdst, const void* dsrc, size_t bytes, nep_stream stream); /* sync */
int32_t nep_dev_copy(void* ddst, const void* dsrc, size_t bytes, nep_stream stream);
int32_t nep_stream_sync(nep_stream stream);
/* *out = 1 when kernels of the two streams execute one after the other (the streams share a hardware queue of the runtime's
 * pool), 0 when they overlap.  Measured (three ~0.4 ms probes; both streams are synchronised): a host that puts long
 * one-wavefront kernels (nep_hess_eig*_dev) on a side stream picks one that serialises with neither its main stream nor the
 * stream of its convergence checks. */
int32_t nep_stream_pair_serializes(nep_stream a, nep_stream b, int32_t* out);

/* ---- SPMF object: M(lambda) = sum_i f_i(lambda) A_i ------------------------------------
 * replaces: struct SPMF_NEP  src/NEPTypes.jl:162-170 (+ get_Av :103, DEP :427-443,
 *           PEP src/types_poly.jl:31-34, SPMFSumNEP src/NEPTypes.jl:845-847 -- all are
 *           "a list of matrices" to the device).
 * Input: mt matrices of size n x n in CSR (0-based, int32): rowptr[i] (n+1), colind[i], vals[i]
 * (double if val_is_complex[i]==0 else nep_cdouble).  Julia's CSC of A is the CSR of A^T; the
 * binding passes transpose(A_i) in CSC form, or uses nep_csc_to_csr below.
 * The library builds ONE stacked CSR over all terms (entries sorted by (col,term) per row). */
int32_t nep_spmf_create(int64_t n, int32_t mt, const int32_t* const* h_rowptr,
                        const int32_t* const* h_colind, const void* const* h_vals,
                        const int32_t* h_val_is_complex, nep_spmf** out);
int32_t nep_spmf_destroy(nep_spmf* s);
/* info[0]=n info[1]=mt info[2]=total nnz info[3]=value bytes (8|16) info[4]=lanes per row
 * chosen for the SpMV info[5]=algorithmic matrix bytes of one pass over the stacked CSR */
int32_t nep_spmf_info(const nep_spmf* s, int64_t info[6]);
/* footprint tiles of the one-launch compute_Mlincomb kernel (csrc/spmv_tile.hip; all zero when the matrix has none):
 * info[0]=blocks info[1]=largest column footprint info[2]=detected grid stride (0: consecutive rows) info[3],info[4]=patch
 * shape info[5]=padded entries info[6]=footprint slots info[7]=bytes one launch streams for the matrix side */
int32_t nep_spmf_tile_info(const nep_spmf* s, int64_t info[8]);
/* host-only dry run of those tiles for an SPMF given as in nep_spmf_create (nothing goes to the device; tests without a GPU,
 * sanitizer build): info as above, *maxerr = largest relative difference between z = sum_t A_t (V c_t) evaluated through the
 * tiles (footprint -> W -> entries -> row map, as the kernel walks them) and directly, deterministic V (n x k), C (k x mt) */
int32_t nep_spmf_tiles_analyze(int64_t n, int32_t mt, const int32_t* const* h_rowptr, const int32_t* const* h_colind,
                               const void* const* h_vals, const int32_t* h_val_is_complex, int32_t k, int64_t info[8],
                               double* maxerr);
/* tuning / A-B knob for compute_Mlincomb: 0 = automatic choice per (n, k), 1 = the tiled one-launch kernel whenever the
 * matrix has tiles, 2 = never (k_vc + SpMV / folded SpMV).  Process-wide. */
int32_t nep_k1_set_mode(int32_t mode);
/* K2 kernel choice (A/B knob): the super-panel residual kernel (csrc/spmv_tile.hip k_tile_resid_sp) 0 = never, 1 = on large matrices
 * (default), 2 = whenever the footprint tiles allow it, -1 = the environment variable NEP_K2_SP decides.  Reference: the residual of
 * all Ritz pairs, src/errmeasure.jl:128-130,186-190. */
int32_t nep_k2_set_sp_mode(int32_t mode);
/* Dispatch query: what the entry points below would launch for this handle and k under the current modes and environment.
 * Host-only, launches nothing; it evaluates the very predicates the launchers call, so it cannot drift from them (tests state
 * with it which kernel instantiation a case covered).
 * op: NEP_PLAN_K1 nep_mlincomb[_dev]; NEP_PLAN_K2_NORMS nep_resid_batch[_dev] / nep_resid_split_dev; NEP_PLAN_K2_BLOCK
 * nep_resid_block; NEP_PLAN_K2_CM nep_resid_batch_cm_dev.  The row-major K2 forms work in column panels of
 * P = min(256, max(1, 3072 / mt)) columns: the answer describes the first panel (min(k, P) columns, row stride ldq = k assumed
 * for the 32-bit-offset test of k_spmm_rm_g); a narrower last panel may choose differently and is queried with its own k.
 *   info[0] kernel, NEP_PLAN_K_* below
 *   info[1] value bytes of the stored matrices (8 | 16)
 *   info[2] terms unrolled in the kernel (template parameter M of the tiled kernels and of k_vc: min(mt, 4) -- k_vc takes the
 *           terms four at a time and the remainder in a last launch; mt elsewhere)
 *   info[3] flags, NEP_PLAN_F_* below
 *   info[4] threads per workgroup of the matrix kernel
 *   info[5] lanes per row (CSR kernels of K1; 64 = one row per lane of a SELL slice), 64-column chunks per row
 *           (k_spmm_rm[_g]) or columns per tile panel (tiled K2)
 *   info[6] flush mask of the slot layout (super-panel kernels: 0x80 one term, 0xD0 the 5 + 2 + 1 layout, 0xFF any other);
 *           NEP_PLAN_K_VC_SPMV: rows per workgroup of k_vc (16 | 32 | 64); 0 elsewhere
 *   info[7] number of column panels (passes over the matrix) of the call
 * NEP_ERR_UNSUPPORTED (info all zero) where the entry point itself would refuse: NEP_PLAN_K2_CM without tiles or with mt > 4.
 * NEP_ERR_ARG: k < 1, unknown op, NEP_PLAN_K2_BLOCK with k > 256. */
#define NEP_PLAN_K1 0
#define NEP_PLAN_K2_NORMS 1
#define NEP_PLAN_K2_BLOCK 2
#define NEP_PLAN_K2_CM 3
#define NEP_PLAN_K_SPMV_FOLD 1      /* k = 1: k_spmv_fold<lanes> / k_spmv_sell<fold> */
#define NEP_PLAN_K_SPMV_KFUSED 2    /* 2 <= k <= 16: k_spmv_kfused<lanes> / k_spmv_sell_kfused<k> */
#define NEP_PLAN_K_VC_SPMV 3        /* k_vc<M, rows> per four terms, then k_spmv<lanes> / k_spmv_sell */
#define NEP_PLAN_K_TILE_MLINCOMB 4  /* k_tile_mlincomb<M, non-temporal, prefetch> */
#define NEP_PLAN_K_SPMM_RM_G 5      /* k_spmm_rm_g<chunks = 1, 2> */
#define NEP_PLAN_K_SPMM_RM 6        /* k_spmm_rm<chunks = 1..4> */
#define NEP_PLAN_K_TILE_RESID 7     /* k_tile_resid<M, panel 4 | 8, non-temporal> */
#define NEP_PLAN_K_TILE_RESID_SP 8  /* k_tile_resid_sp<layout, threads, flush mask> */
#define NEP_PLAN_K_TILE_RESID_SPP 9 /* k_tile_resid_spp: the persistent form */
#define NEP_PLAN_K_TILE_RESID_CM 10 /* k_tile_resid_cm<M, panel 2 | 4 | 8, non-temporal> */
#define NEP_PLAN_K_TILE_RESID_SP4 11 /* k_tile_resid_sp4: ring of four half-tiles, column-major only */
#define NEP_PLAN_F_SELL 1
#define NEP_PLAN_F_NT 2             /* non-temporal loads of the matrix entries */
#define NEP_PLAN_F_PREFETCH 4       /* register prefetch of the next block's entries */
#define NEP_PLAN_F_COLSPLIT 8       /* the k columns split over thread groups */
#define NEP_PLAN_F_PERSISTENT 16
#define NEP_PLAN_F_RING 32
#define NEP_PLAN_F_XCD_ROWS 64      /* rows dealt to the XCDs in contiguous ranges (k_spmm_rm[_g]) */
int32_t nep_spmf_plan(const nep_spmf* s, int32_t op, int32_t k, int64_t info[8]);
int32_t nep_csc_to_csr(int64_t n, const int64_t* colptr, const int64_t* rowval, const void* nzval,
                       int32_t val_is_complex, int32_t one_based, int32_t* rowptr, int32_t* colind,
                       void* vals);

/* ---- rectangular CSR operator (complex values, 0-based int32 indices) ----------------------
 * replaces: the low-rank factors held by RKNEP, src/rk_helper/rk_nep.jl:19-32,128-152 -- UU (hcat of the U_i,
 *           applied as UU' at src/method_nleigs.jl:430,480,510) and the rows LL / iLr of [L_1 ... L_q]
 *           (scalar loop at :464-471).  nep_csr_mv:  y = alpha*A*x + beta*z   (x: cols entries, y, z: rows
 *           entries; z may alias y and is not read when beta == 0). */
typedef struct nep_csr nep_csr;
int32_t nep_csr_create(int64_t rows, int64_t cols, const int32_t* h_rowptr, const int32_t* h_colind,
                       const nep_cdouble* h_vals, nep_csr** out);
int32_t nep_csr_destroy(nep_csr* a);
int32_t nep_csr_mv(const nep_csr* a, nep_cdouble alpha, const nep_cdouble* dx, nep_cdouble beta,
                   const nep_cdouble* dz, nep_cdouble* dy, nep_stream stream);

/* K1  z = sum_i A_i * (V * C[:,i])          V: n x k (ldv), C: k x mt (host, column-major)
 * replaces: compute_Mlincomb!(::SPMF_NEP,...) src/NEPTypes.jl:972-1011 and
 *           compute_Mlincomb(::DerSPMF,...)   src/NEPTypes.jl:1130-1160 (VafD=V*(a.*fD); z+=Av[j]*VafD[:,j]),
 *           PEP :1016-1045, DEP :940-970, SumNEP :889-890 (all are this with other C).
 * The host forms C[j,i] = a_j * f_i^(j-1)(lambda) (NEPCore.jl:218-228 identity). dV is not modified. */
int32_t nep_mlincomb(nep_spmf* s, int32_t k, const nep_cdouble* hC, const nep_cdouble* dV,
                     int64_t ldv, nep_cdouble* dz, nep_stream stream);

/* same with the coefficient block already resident on the device (column stride ldc >= k): a
 * driver uploads the derivative table once (DerSPMF, src/NEPTypes.jl:1108-1128) and every iteration
 * uses its first k rows -- no host-to-device copy on the critical path. */
int32_t nep_mlincomb_dev(nep_spmf* s, int32_t k, const nep_cdouble* dC, int64_t ldc, const nep_cdouble* dV,
                         int64_t ldv, nep_cdouble* dz, nep_stream stream);

/* K11  c = - sum_t sum_{j<ma} sum_{i<mb} tau[i+j+1 + t*ldt] * w_j^H A_t b_i: the left-right scalar product of the infinite
 * bi-Lanczos method, the entrywise product of W^H A_t B with a Hankel matrix of Taylor coefficients.
 * replaces: left_right_scalar_prod src/method_infbilanczos.jl:229-246 (ma calls of compute_Mlincomb on B scaled by
 *           1/(j+i-1)!, each followed by dot(At[:,j], .)), called at :106, :151, :171.
 * dW: n x ma (ldw), dB: n x mb (ldb), column-major device blocks.  dTau: device (ma+mb) x mt column-major (ldt >= ma+mb),
 * tau[d + t*ldt] = f_t^(d)(sigma) / d! -- the layout of nep_mlincomb_dev's coefficient block (dTau + 1 with ldc = ldt gives
 * sum_i M^(i)(sigma)/i! v_i).  Two launches, fixed reduction order (two calls give the same bits), A_t B is never stored.
 * h_c != NULL: c to the host (synchronous); otherwise c to the device word d_c (asynchronous).
 * NEP_ERR_UNSUPPORTED when ma or mb exceeds 256. */
int32_t nep_lr_hankel(nep_spmf* s, int32_t ma, int32_t mb, const nep_cdouble* dW, int64_t ldw, const nep_cdouble* dB,
                      int64_t ldb, const nep_cdouble* dTau, int64_t ldt, nep_cdouble* h_c, nep_cdouble* d_c,
                      nep_stream stream);

/* K14  out[i + kw*(j + kv*t)] = w_i^H A_t v_j for every term t < mt: the unsummed bilinear forms of the SPMF.
 * replaces: the `dot(y, nep.A[i]*x)` loop of compute_rf src/compute_rf_wrapper.jl:115-118, the two compute_Mlincomb calls and
 *           dots per scalar Newton step of :31-39 (y^H M(lam) x = sum_t f_t(lam) y^H A_t x needs the forms once), and the
 *           per-term W' * (A_t * V) of set_projectmatrices! src/NEPTypes.jl:724-741.
 * dW: n x kw (ldw), dV: n x kv (ldv), column-major device blocks; dW == dV is allowed; rows >= n of a column are never read.
 * The stacked CSR is read once for all terms when mt*kv <= 32 (ceil(kv / floor(32 / mt)) times beyond; kw = kv = 1 is one pass
 * for every mt), two launches, no intermediate of size n x kv, no atomics, fixed summation order: two calls give the same bits.
 * h_out != NULL: the mt*kw*kv results to the host (synchronous); otherwise to the device block d_out (asynchronous).
 * NEP_ERR_UNSUPPORTED (nothing launched) unless 1 <= kw, kv <= 32 and mt*kw*kv <= 3072; NEP_ERR_ARG (nothing launched) for a
 * NULL handle or block, ldw < n, ldv < n, or both outputs NULL. */
int32_t nep_spmf_biforms(nep_spmf* s, int32_t kw, const nep_cdouble* dW, int64_t ldw, int32_t kv, const nep_cdouble* dV,
                         int64_t ldv, nep_cdouble* h_out, nep_cdouble* d_out, nep_stream stream);

/* Expansion step of compute_Mlincomb on a deflated NEP (Effenberger deflation).  With X = V0 (n0 x p), V = [V1; V2]
 * (k columns of n0 + p rows), s = startder, K = k + s, e_i = i + s:
 *   Vn[:, j] = [j >= s] a_{j-s} V1[:, j-s] + X sum_{i : e_i >= j} G[i, j] W_{e_i - j} V2[:, i],   j = 0..K-1
 *   zb       = a_0 X^H V1[:, 0] for s == 0, zeros for s > 0          (always written)
 * and sum_j M^(j)(lambda) Vn[:, j] (nep_mlincomb with a block of ones) is the top part of the deflated product.
 * replaces: compute_Mlincomb(::DeflatedGenericNEP, ...) src/nep_deflation.jl:65-107 (Q[i] by repeated solves with the factors of
 *           lambda I - S, Z[:, j] += factor * Xhat * Vnew, Vnew = V[1:n0, :] * Diagonal(a) + Z, z_bottom = X' * V[1:n0, 1] * a[1]).
 * The host supplies W_d = (lambda I - S0)^-(d+1) and G[i, j] = (-1)^(e_i - j) a_i e_i! / j!; the kernels use the tables as
 * given.  hA (k), hG (k x K, column-major), hW (p x p x K: W_d at hW + d p^2, column-major) are host arrays that may be freed
 * on return (staged like nep_mlincomb's hC).  dV is not modified; dVn (n0 x K, ldo) must not overlap dV; rows beyond n0
 * (n0 + p for dV) of a column are neither read nor written.  Asynchronous; at most three launches (two for K <= 8), fixed
 * reduction order, no atomics: two calls give the same bits.
 * NEP_ERR_UNSUPPORTED (nothing launched) unless 1 <= p <= 32 and k + s <= 64; NEP_ERR_ARG (nothing launched) for n0 < 1, k < 1,
 * s < 0, ldx < n0, ldo < n0, ldv < n0 + p. */
int32_t nep_defl_expand(int64_t n0, int32_t p, int32_t k, int32_t s, const nep_cdouble* dX, int64_t ldx,
                        const nep_cdouble* dV, int64_t ldv, const nep_cdouble* hA, const nep_cdouble* hG,
                        const nep_cdouble* hW, nep_cdouble* dVn, int64_t ldo, nep_cdouble* dzb, nep_stream stream);

/* Border step of a linear solve with the deflated matrix [M(lambda) U; X^H 0], U = M(lambda) X (lambda I - S0)^-1, X^H X = I.
 * Because M^-1 U = X (lambda I - S0)^-1 exactly, the Schur complement -X^H M^-1 U is -(lambda I - S0)^-1 and the solution of
 * [M U; X^H 0] [v1; v2] = [b1; b2] is
 *   y = M(lambda)^-1 b1 (ONE solve with the original matrix, the caller's),  c = b2 - X^H y,  v1 = y + X c,  v2 = -(lambda I - S0) c
 * (check: M v1 + U v2 = b1 + M X c - M X c = b1, X^H v1 = X^H y + c = b2).  This call computes, from y,
 *   c = b2 - X^H y,   out[0:n0] = scale (y + X c),   out[n0:n0+p] = scale (T c).
 * replaces: lin_solve(::DeflatedNEPLinSolver) src/LinSolvers.jl:221-252 (p + 1 solves with the original solver, Z = M^-1 U,
 *           S = -X' Z, v2 = S \ (b2 - X' b1tilde), v1 = b1tilde - Z v2).
 * dX: n0 x p column-major (ldx), dY: n0 entries, db2: p device entries or NULL (zeros), hT: p x p column-major HOST table (the
 * caller passes -(lambda I - S0); may be freed on return, staged like nep_defl_expand's tables; the kernels use it as given).
 * dOut: n0 + p entries; dY may be dOut itself (in place); db2 must not overlap dOut.  Asynchronous; three launches, fixed
 * reduction order, no atomics: two calls give the same bits.
 * NEP_ERR_UNSUPPORTED (nothing launched) unless 1 <= p <= 32; NEP_ERR_ARG (nothing launched) for n0 < 1, ldx < n0, a NULL
 * dX / dY / hT / dOut, or db2 overlapping dOut. */
int32_t nep_defl_border(int64_t n0, int32_t p, const nep_cdouble* dX, int64_t ldx, const nep_cdouble* dY,
                        const nep_cdouble* db2, const nep_cdouble* hT, double scale, nep_cdouble* dOut, nep_stream stream);

/* The small products of a compact rational Krylov (CORK) step:
 *   Out[rho, gam] = alpha u[rho] g[gam] + sum_{q < k} U[rho, q] G[q, gam],   rho < r, gam < c.
 * replaces: src/method_AAAeigs.jl:283-287,332-339 (u_c = U[1:r,1:k,j] * (compactB * [I; Y[2:end,:]]) after the k x k solve for Y,
 *           and W = [u1_hat  U[1:rnew,:,j] * compactB[:,l+1:end]], Uhat = W / MlNfact).  With the tables of a shift formed once
 *           on the host (C_sigma = B[:, :l] + B[:, l:] Y[1:, :];  g_sigma = (Mext^-1)[0, :], G_sigma = B[:, l:] (Mext^-1)[1:, :])
 *           u_c is the call with dG = C_sigma and du = NULL, Uhat the call with dG = G_sigma, dg = g_sigma and du = the row
 *           [Q^H v; ||v_perp||] that nep_orth_dev leaves on the device; alpha carries the scaling of :296-300.
 * dU: r x k column-major (ldu), dG: k x c column-major (ldg), du: r device entries or NULL (no rank-1 term), dg: c device
 * entries (read only with du), alpha by value, dOut: r x c column-major (ldo); dOut must not overlap dU, dG, du or dg.  Rows
 * >= r of a column and the padding behind a column are neither read nor written.  Asynchronous; ONE launch, no atomics, fixed
 * summation order (q ascending, then the rank-1 term): two calls give the same bits.
 * NEP_ERR_UNSUPPORTED (nothing launched) unless 1 <= k <= 256 and 1 <= c <= 256; NEP_ERR_ARG (nothing launched) for r < 1,
 * ldu < r, ldg < k, ldo < r, a NULL dU / dG / dOut, du without dg, or dOut overlapping an input. */
int32_t nep_cork_expand(int32_t r, int32_t k, int32_t c, const nep_cdouble* dU, int64_t ldu, const nep_cdouble* dG, int64_t ldg,
                        const nep_cdouble* du, const nep_cdouble* dg, nep_cdouble alpha, nep_cdouble* dOut, int64_t ldo,
                        nep_stream stream);

/* Interpolation coefficients of a sampled matrix function, entry by entry:
 *   C[r(e), i] = beta C[r(e), i] + sum_{j < J} W[i, j] F[e, j],   e < E, i < K,   r(e) = dpos ? dpos[e] : e.
 * replaces: src/types_cheb_pep.jl:94-114 (chebyshev_compute_coefficients: Ck = map(i -> sum(Fk .* Tmat[i,:]), 1:k), k sparse
 *           matrix sums per coefficient) and src/types_poly.jl:121-164 (interpolate: one Vandermonde solve per non-zero, or the
 *           Kronecker-product solves of the dense branch).  W is the weight table Tmat, the inverse Vandermonde matrix, or either
 *           of them times the function values of the terms of an SPMF at the nodes (then F is the term block D itself).
 * dF: E rows of J contiguous values, row stride ldf >= J (entry-major: the layout of the aligned term block of an SPMF),
 * complex128 when f_is_complex != 0, float64 otherwise.  hW: K x J column-major HOST table (hW[i + j K]; may be freed on return,
 * staged by the call).  dpos: E device int32 row numbers of dC or NULL; the caller guarantees that they are distinct and inside
 * dC.  dC: rows of K contiguous complex128 values, row stride ldc >= K.  beta is 0 or 1; with 0 dC is never read.  dC must not
 * overlap dF (checked when dpos is NULL).  Entries >= E, the padding of a row of dF or dC and rows of dC that dpos does not name
 * are neither read nor written.  Asynchronous; ONE launch, every value of dF is read once, no atomics, fixed summation order
 * (the old value, then j ascending): two calls give the same bits.  E = 0 is a no-op.
 * NEP_ERR_UNSUPPORTED (nothing launched, nothing written) unless 1 <= J <= 64 and 1 <= K <= 64; NEP_ERR_ARG (nothing launched)
 * for E < 0, ldf < J, ldc < K, beta outside {0, 1}, a NULL hW, a NULL dF / dC with E > 0, or dC overlapping dF without a map. */
int32_t nep_interp_coeffs(int64_t E, int32_t J, int32_t K, const void* dF, int64_t ldf, int32_t f_is_complex,
                          const nep_cdouble* hW, const int32_t* dpos, int32_t beta, nep_cdouble* dC, int64_t ldc,
                          nep_stream stream);

/* One pass over the approximate inverse Jacobian T of Broyden's method (n x n, column-major, ldt, device):
 *   T[i, j] += u0[i] a0[j]                     when du0 / da0 are given: the only write to T
 *   y[i]     = sum_j T_new[i, j] x[j]          when dx / dy are given
 *   g[j]     = sum_i conj(w[i]) T_new[i, j]    when dw / dg are given: the ROW w^H T_new, unconjugated
 * replaces: src/method_broyden.jl:69,101,107,117 (Trk = T*rk, Tztilde = T*ztilde, dv'*T and T = T + Tztilde*aH: four passes over
 *           T per inner iteration).  a0 holds the row aH as it stands (no conjugation here); with the update of iteration j kept
 *           pending, the sweep of iteration j + 1 applies it and returns T*ztilde and dv'*T of the updated matrix.
 * du0, da0, dx, dw: n device entries each; dy, dg: n device entries, written; dWork: nep_broyden_sweep_worksize(n) complex
 * device entries of scratch (per-tile partial sums).  dy and dg must not overlap each other, an input, dT or dWork; dWork must
 * not overlap dT.  Every entry of T is read once, written once with an update and never without; rows >= n of a column and the
 * padding behind it are neither read nor written.  Asynchronous; at most two launches, no atomics, fixed summation order: two
 * calls on equal inputs give the same bits.
 * NEP_ERR_ARG (nothing launched) for n < 1, ldt < n, a NULL dT / dWork, one half of a pair without the other, no work
 * requested, or an overlap named above. */
int64_t nep_broyden_sweep_worksize(int64_t n);
int32_t nep_broyden_sweep(int64_t n, nep_cdouble* dT, int64_t ldt, const nep_cdouble* du0, const nep_cdouble* da0,
                          const nep_cdouble* dx, nep_cdouble* dy, const nep_cdouble* dw, nep_cdouble* dg, nep_cdouble* dWork,
                          nep_stream stream);

/* K2  residual batch: r_s = sum_i F[i,s] A_i q_s, s=1..k; returns ||r_s||_2 and ||q_s||_2.
 * replaces: k calls of estimate_error -> compute_Mlincomb(nep,lambda_s,q_s)
 *           src/errmeasure.jl:128-130,186-190; call sites src/method_iar.jl:134-135,
 *           src/method_tiar.jl:211-212, src/method_beyncontour.jl:142-144.
 * dQT: the k vectors stored ROW-major (row r holds q_1[r]..q_k[r]; row stride ldq >= k), which is
 * what nep_gemm_ts(..., y_rowmajor=1) produces.  hF: mt x k column-major host.  Synchronous. */
int32_t nep_resid_batch(nep_spmf* s, int32_t k, const nep_cdouble* hF, const nep_cdouble* dQT,
                        int64_t ldq, double* h_rnorm, double* h_qnorm, nep_stream stream);
/* asynchronous variant: no host synchronisation, SQUARED norms stay on the device.  d_out (2k doubles), per panel of
 * kk <= P columns starting at column j0: d_out[2*j0 + j] = ||M(lam_j) q_j||^2, d_out[2*j0 + kk + j] = ||q_j||^2, where the
 * panel width is P = min(256, max(1, 3072 / mt)) (the mt x P coefficient block has to fit 48 KiB of LDS). */
int32_t nep_resid_batch_dev(nep_spmf* s, int32_t k, const nep_cdouble* hF, const nep_cdouble* dQT, int64_t ldq,
                            double* d_out, nep_stream stream);

/* K2 for operators with an extra term on their last rows (WEP: dense corner block on the 2 nz boundary rows,
 * src/gallery_extra/waveguide/Waveguide.jl:351-374): one pass gives d_out (device, 2k doubles) = squared column norms of the
 * SPMF residual over rows [0, row0) and of Q over all rows, and dRT_tail ((n - row0) x k row-major, ld ldt) = the residual
 * rows [row0, n); the caller adds its term to the tail and the tail's norms to d_out.  0 <= row0 <= n (row0 = n: no tail rows,
 * row0 = 0: no rows in the residual norms), ldt >= k, dRT_tail not NULL even when it has no rows; d_out in the panel layout of
 * nep_resid_batch_dev; the columns k .. ldt - 1 of the tail are not written.  NEP_ERR_ARG otherwise, nothing launched. */
int32_t nep_resid_split_dev(nep_spmf* s, int32_t k, const nep_cdouble* hF, const nep_cdouble* dQT, int64_t ldq, int64_t row0,
                            double* d_out, nep_cdouble* dRT_tail, int64_t ldt, nep_stream stream);
/* K2 with a COLUMN-major Ritz block (n x k, column s at dQ + s ldq, what nep_gemm_ts writes with y_rowmajor = 0): at
 * waveguide scale the panel loads of the tiled kernel are then contiguous per column and every byte of Q crosses HBM once
 * (csrc/spmv_tile.hip k_tile_resid_cm).  d_out: 2k squared norms (device).  row0 < 0: whole residual in the norms; row0 >= 0:
 * rows [0, row0) in the norms, rows [row0, n) written to dR_tail ((n - row0) x k column-major, ld ldt) as in
 * nep_resid_split_dev.  NEP_ERR_UNSUPPORTED when the matrix has no footprint tiles, more than 4 terms, or a largest column
 * footprint above 1200 (eight tile columns of it have to fit 150 KiB of LDS; nep_spmf_tile_info, info[1]).  Any k >= 1: the
 * kernels walk the columns in panels and read the coefficients from device memory, so there is no upper limit on k (k = 300 is
 * tested); d_out is ONE block of 2k doubles, ||r_s||^2 at d_out[s] and ||q_s||^2 at d_out[k + s], whatever k.
 * NEP_ERR_ARG, nothing launched: k < 1, ldq < n, row0 > n, or row0 >= 0 with dR_tail NULL or ldt < n - row0. */
int32_t nep_resid_batch_cm_dev(nep_spmf* s, int32_t k, const nep_cdouble* hF, const nep_cdouble* dQ, int64_t ldq, int64_t row0,
                               double* d_out, nep_cdouble* dR_tail, int64_t ldt, nep_stream stream);

/* same residuals, but the block R^T (row-major, row stride ldr >= k) is written instead of its norms --
 * for NEPs with an extra non-SPMF term (the WEP corner, src/gallery_extra/waveguide/Waveguide.jl:351-374)
 * whose contribution is added before the norms are taken.  Asynchronous.  1 <= k <= 256 (NEP_ERR_ARG above: callers split the
 * columns themselves); the columns k .. ldr - 1 of a row of dRT are not written, the columns k .. ldq - 1 of dQT never read. */
int32_t nep_resid_block(nep_spmf* s, int32_t k, const nep_cdouble* hF, const nep_cdouble* dQT, int64_t ldq,
                        nep_cdouble* dRT, int64_t ldr, nep_stream stream);

/* compute_MM building block: ZT = sum_i A_i * XT[:, i*p:(i+1)*p]  (row-major in and out)
 * replaces: compute_MM(::SPMF_NEP,S,V) src/NEPTypes.jl:276-319 (Z += AA[i]*(V*f_i(S))) after
 *           XT = (V*[F_1..F_mt])^T has been formed with nep_gemm_ts. */
int32_t nep_spmm_terms(nep_spmf* s, int32_t p, const nep_cdouble* dXT, int64_t ldx,
                       nep_cdouble* dZT, int64_t ldz, nep_stream stream);

/* K12  SPMF block product with per-term tables:
 *   Z[:, 0:q] = beta Z[:, 0:q] + alpha sum_{t < mt} A_t (Y G_t),     Y: n x r,  G_t: r x q,  Z: n x q  (column-major)
 * replaces: compute_MM(::SPMF_NEP,S,V) src/NEPTypes.jl:276-319 for G_t = f_t(S), and the term loops of the block Newton
 *           method, src/method_blocknewton.jl:173-179 (T12 = T12 + Av[j]*X*DF1) and :201-206 (RT[:,i+1:p] += -Av[j]*(Za+Zb)),
 *           where G_t is a block of f_t on an expanded matrix -- composed from nep_gemm_ts (row-major n x (mt q) block),
 *           nep_spmm_terms and a transpose back otherwise: three launches and 16 n mt q bytes written and read again.
 * dY (ldy >= n) is not modified.  hG: host array, G_t column-major at hG + t r q; it may be freed on return (staged through
 * the handle's pinned ring into a device slot of the handle that is not handed out again before the kernel that reads it has
 * finished: calls with different tables may follow each other at once, on any stream).  dZ (ldz >= n) must not overlap dY;
 * beta == 0: Z is not read (a NaN-filled Z comes back finite), otherwise every entry of Z is read at its own position only.
 * Rows >= n of a column and the padding behind it are neither read nor written.  Both value widths of the stacked CSR.
 * Asynchronous; ONE launch, the tables in LDS, no intermediate of size n x (mt q), no atomics, fixed summation order: two
 * calls on equal inputs give the same bits.
 * NEP_ERR_UNSUPPORTED (nothing launched) unless 1 <= r <= 32, 1 <= q <= 32 and mt r q <= 3072 (48 KiB of LDS, the budget of
 * nep_resid_batch_dev); NEP_ERR_ARG (nothing launched) for ldy < n, ldz < n, a NULL s, dY, hG or dZ, or dZ overlapping dY. */
int32_t nep_spmf_blockprod(nep_spmf* s, int32_t r, int32_t q, const nep_cdouble* dY, int64_t ldy, const nep_cdouble* hG,
                           nep_cdouble alpha, nep_cdouble beta, nep_cdouble* dZ, int64_t ldz, nep_stream stream);

/* ---- K6 Gram-Schmidt -------------------------------------------------------------------
 * replaces: IterativeSolvers.orthogonalize_and_normalize!(V,w,h,method) (third-party,
 *           IterativeSolvers 0.9.2) at src/method_iar.jl:107, src/method_tiar.jl:128,
 *           src/method_nleigs.jl:293.
 * h = V^H w; w -= V h; [DGKS: while ||w|| < ||corr||/sqrt(2): corr=V^H w; w-=V corr; h+=corr];
 * beta=||w||; w/=beta.   dV: rows x k (ldv).  h_active_rows (nullable, k entries): number of
 * leading rows of column j that can be non-zero (iar's block-triangular basis); rows beyond are
 * skipped.  Contract: column j of dV must HOLD zeros in the rows active[j] .. rows - 1 -- the projection masks them per row, the
 * update skips whole tiles only and reads them inside a partly active tile.  Entries above rows count as rows.
 * method: 0 = DGKS, 1 = classical GS (one pass), 2 = modified GS.  Synchronous.  A vector inside span(V) (||w|| == 0 after the
 * update) returns NEP_ERR_BREAKDOWN with h, *h_beta = 0 and *h_npasses set and w left at zero. */
int32_t nep_orth(const nep_cdouble* dV, int64_t ldv, int64_t rows, int32_t k,
                 const int64_t* h_active_rows, nep_cdouble* dw, nep_cdouble* h_h, double* h_beta,
                 int32_t method, int32_t* h_npasses, nep_stream stream);
/* asynchronous DGKS (method 0) / CGS (method 1): no host synchronisation.  The re-orthogonalisation passes are
 * always enqueued and gate themselves on the device with the same criterion (at most 2 passes, NEP_ORTH_DEV_PASSES); w is normalised on the
 * device.  d_active_rows: DEVICE array (or NULL), same contract as nep_orth: dV holds zeros at and below active[j].  d_out (k+2
 * complex, device): h[0..k), (beta, 0), (passes, 2*breakdown + another_pass_wanted).  method 2: NEP_ERR_ARG. */
int32_t nep_orth_dev(const nep_cdouble* dV, int64_t ldv, int64_t rows, int32_t k, const int64_t* d_active_rows,
                     nep_cdouble* dw, nep_cdouble* d_out, int32_t method, nep_stream stream);
/* h = V^H w for a rows x k block (w untouched, k host results, synchronous): the products W^H (A_i v) behind
 * set_projectmatrices! / expand_projectmatrices! of Proj_SPMF_NEP (src/NEPTypes.jl:724-790) and Gram matrices. */
int32_t nep_gemv_h(const nep_cdouble* dV, int64_t ldv, int64_t rows, int32_t k, const nep_cdouble* dw,
                   nep_cdouble* h_h, nep_stream stream);
/* K9  C = W^H Y (k x p, host, column-major) for two ROW-major device blocks WT (rows x k), YT (rows x p), k, p <= 256:
 * all of B_i = W^H (A_i V) at once (YT from nep_resid_block with F = e_i 1^T), FP64 MFMA with the row index as contraction
 * index, per-workgroup partial tiles summed in a fixed order.  Synchronous.  ldw >= k, ldy >= p: the padding behind the k (p)
 * entries of a row is never read; dWT and dYT may be the same block (Gram matrix). */
int32_t nep_gemm_h_rm(const nep_cdouble* dWT, int64_t ldw, const nep_cdouble* dYT, int64_t ldy, int64_t rows,
                      int32_t k, int32_t p, nep_cdouble* h_C, nep_stream stream);

/* ---- eigen-decomposition of the small Hessenberg matrix of a Krylov driver, on the device ---------------------------------
 * replaces: `D,Z = eigen(H[1:k,1:k])`  src/method_iar.jl:112, src/method_tiar.jl:182 (LAPACK zgeev on the host there).
 * dH: k x k upper Hessenberg, column-major with leading dimension ldh (entries below the first subdiagonal are not read --
 * the rows of nep_iar_step's device H block, leading dimension m + 4, are exactly this layout).
 * nep_hess_eigvals_dev: eigenvalues by the shifted QR iteration (two wavefronts, matrix packed in LDS; k <= 128, else
 *   NEP_ERR_UNSUPPORTED) -> d_w[0..k); d_w[k] = (0 | 1-based index of the eigenvalue the iteration gave up on, sweeps).
 * nep_hess_eigvecs_dev: right eigenvectors by inverse iteration (LAPACK zhsein's scheme, one wavefront per eigenvalue) ->
 *   dZ (k x k column-major, ldz), unit 2-norm, largest component real positive; d_w[k+1] = (vectors that failed, 0).
 *   Must follow nep_hess_eigvals_dev on the same stream with the same d_w / d_work.
 * d_w: k + 2 complex (device).  d_work: nep_hess_eig_worksize bytes (device).  h_mirror: NULL, or mapped pinned host memory
 * of k + 2 complex that receives a copy of d_w (eigenvalues + status as soon as the first kernel ends, the second status
 * word when the last eigenvector is done) -- a host that records an event behind each call reads them without a copy command.
 * A caller that finds a non-zero status falls back to LAPACK.  Asynchronous. */
int32_t nep_hess_eig_worksize(int32_t k, int64_t* bytes);
int32_t nep_hess_eigvals_dev(int32_t k, const nep_cdouble* dH, int64_t ldh, nep_cdouble* d_w, void* d_work,
                             nep_cdouble* h_mirror, nep_stream stream);
int32_t nep_hess_eigvecs_dev(int32_t k, nep_cdouble* d_w, nep_cdouble* dZ, int64_t ldz, void* d_work, nep_cdouble* h_mirror,
                             nep_stream stream);
/* the same for a batch of nb leading blocks of ONE Hessenberg matrix, sizes k0, k0 + kstep, ... (the Arnoldi matrices of
 * consecutive steps), one workgroup per block in a single launch -- the decompositions of a driver's steps then overlap each
 * other on one stream instead of queueing behind each other (a decomposition is a serial chain of ~50 k^2 rotations: 3 ms at
 * k = 100, while an Arnoldi step takes 0.3 ms).  Block b: results at d_w + b w_stride (w_stride >= kmax + 2), eigenvectors at
 * dZ + b z_stride with leading dimension ldz >= kmax, workspace d_work + b work_stride bytes (work_stride >=
 * nep_hess_eig_worksize(kmax), multiple of 16), mirror at h_mirror + b mirror_stride. */
int32_t nep_hess_eigvals_batch_dev(int32_t nb, int32_t k0, int32_t kstep, const nep_cdouble* dH, int64_t ldh, nep_cdouble* d_w,
                                   int64_t w_stride, void* d_work, int64_t work_stride, nep_cdouble* h_mirror,
                                   int64_t mirror_stride, nep_stream stream);
int32_t nep_hess_eigvecs_batch_dev(int32_t nb, int32_t k0, int32_t kstep, nep_cdouble* d_w, int64_t w_stride, nep_cdouble* dZ,
                                   int64_t ldz, int64_t z_stride, void* d_work, int64_t work_stride, nep_cdouble* h_mirror,
                                   int64_t mirror_stride, nep_stream stream);

/* ---- K7 tall-skinny GEMM on the FP64 matrix cores --------------------------------------
 * Y = Z * B,  Z: rows x k (ldz, device), B: k x p (host, column-major, ldb), Y: rows x p.
 * y_rowmajor=0: Y column-major (ldy >= rows); =1: Y row-major (ldy >= p).
 * replaces: Q=VV*Z src/method_iar.jl:115; Z[:,1:k]*transpose(a[1:k,k,1:k]) src/method_tiar.jl:119,
 *           :188-189; V*(H*S) src/method_nleigs.jl:318; V*(a.*fD) src/NEPTypes.jl:1154. */
int32_t nep_gemm_ts(const nep_cdouble* dZ, int64_t ldz, int64_t rows, int32_t k,
                    const nep_cdouble* hB, int64_t ldb, int32_t p, nep_cdouble* dY, int64_t ldy,
                    int32_t y_rowmajor, nep_stream stream);

/* same with B resident on the device: B[c,j] = dB[j*ldb + c] (b_rowmajor=0) or dB[c*ldb + j] (=1).
 * Used for the WEP corner term R*diag(s)*R^H (dense nz x nz scaled-DFT blocks, Waveguide.jl:53-65,351-374). */
int32_t nep_gemm_ts_dev(const nep_cdouble* dZ, int64_t ldz, int64_t rows, int32_t k,
                        const nep_cdouble* dB, int64_t ldb, int32_t b_rowmajor, int32_t p,
                        nep_cdouble* dY, int64_t ldy, int32_t y_rowmajor, nep_stream stream);

/* plain dense complex GEMM, column-major:  C = alpha op(A) op(B) + beta C,  op = 0 none | 1 transpose | 2 conjugate
 * transpose; A: m x k after op, B: k x n after op.  The library's own LDS-tiled kernel (csrc/gemm.hip k_gemm_general; no
 * vendor BLAS behind the ABI); C is not read when beta == 0.
 * replaces: the FFTW transforms of the waveguide Sylvester solver, src/gallery_extra/waveguide/waveguide_preconditioner.jl:
 *           120-219 (V!, Vh!, W, Wh as dense DFT / sine-transform matrices), and the small dense products of the
 *           Sylvester-SMW preconditioner (:221-421). */
/* Thin QR of a tall device block by column-wise DGKS (K6), no host synchronisation: dQ (rows x k, column-major, ld ldq) is
 * orthonormalised in place; row j of d_out (k rows of k + 2 complex, device) = R[0..j, j], (R[j, j], 0), (passes, 2 * breakdown +
 * another_pass_wanted).  A column inside the span of its predecessors leaves a tiny R[j, j] (the rank shows in R).
 * replaces: `V, S, W = svd(A0)` of the n x k moment block in Beyn's method, src/method_beyncontour.jl:114-121, which becomes
 *           svd(R) of the k x k factor (V = Q U_R). */
int32_t nep_orth_qr_dev(nep_cdouble* dQ, int64_t ldq, int64_t rows, int32_t k, nep_cdouble* d_out, nep_stream stream);
/* Dense complex inverse on the device (in-place Gauss-Jordan with partial pivoting, deterministic):
 *   dOut (n x n, column-major, ld ldo) = inv(M + add_identity * I)^H,   M n x n column-major (ld ldm), both on the device.
 * dWork: 2 n + 2 complex of device scratch.  *h_info = 0, or 1 + the step whose pivot was zero / not finite (the call synchronises
 * the stream once at its end to read it).
 * replaces: `inv(M)` of the mm x mm Sylvester-SMW matrix, src/gallery_extra/waveguide/waveguide_preconditioner.jl:221-313 (the
 *           adjoint of the inverse is what nep_gemv_hd applies). */
int32_t nep_zinv_h_dev(int32_t n, const nep_cdouble* dM, int64_t ldm, double add_identity, nep_cdouble* dOut, int64_t ldo,
                       nep_cdouble* dWork, int32_t* h_info, nep_stream stream);
/* nep_zgemm with the reduction split over `ksplit` workgroups per tile, slices summed in order (deterministic); dWork: ksplit * m * n
 * complex (device).  For products of a few tiles with a long K: the k x k block V0^H A1 of src/method_beyncontour.jl:123. */
int32_t nep_zgemm_sk(int32_t transa, int32_t transb, int32_t m, int32_t n, int32_t k, nep_cdouble alpha,
                     const nep_cdouble* dA, int64_t lda, const nep_cdouble* dB, int64_t ldb, nep_cdouble beta,
                     nep_cdouble* dC, int64_t ldc, int32_t ksplit, nep_cdouble* dWork, nep_stream stream);
int32_t nep_zgemm(int32_t transa, int32_t transb, int32_t m, int32_t n, int32_t k, nep_cdouble alpha,
                  const nep_cdouble* dA, int64_t lda, const nep_cdouble* dB, int64_t ldb, nep_cdouble beta,
                  nep_cdouble* dC, int64_t ldc, nep_stream stream);

/* real GEMM (same kernel, float64), op = 0 none | 1 transpose.  A complex column-major m x n block is a real 2m x n block, so
 * products X * W with a real W (the sine transform W of waveguide_preconditioner.jl:176-199) run at half the flops. */
int32_t nep_dgemm(int32_t transa, int32_t transb, int32_t m, int32_t n, int32_t k, double alpha,
                  const double* dA, int64_t lda, const double* dB, int64_t ldb, double beta,
                  double* dC, int64_t ldc, nep_stream stream);

/* Refinement criterion of the fixed-shift solve (replaces UMFPACK's internal iterative refinement behind
 * `Afact \ x`, src/LinSolvers.jl:114-122 with control[8] = umfpack_refinements): writes r = b - M(lam) x and, if
 * h_omega != NULL, returns the componentwise backward error
 *     max_i |r_i| / (sum_t h_cabs[t] * (|A_t| |x|)_i + |b_i|)          (Arioli/Demmel/Duff), h_cabs[t] = |f_t(lam)|
 * after a stream synchronisation; with h_omega == NULL nothing is read back (blind refinement step).  M(lam) x is
 * either given (dMx, e.g. from a NEP-specific compute_Mlincomb with non-SPMF terms; h_c == NULL) or formed in the same
 * pass over the matrices from the host coefficients h_c[t] = f_t(lam) (dMx == NULL).  d_den_extra (device, n complex,
 * real parts used, may be NULL) is added to the denominator: (|P||x|)_i of operator parts outside the SPMF terms (the
 * dense corner block of the waveguide problem). */
int32_t nep_cw_backward_error(nep_spmf* s, const double* h_cabs, const nep_cdouble* h_c, const nep_cdouble* dx,
                              const nep_cdouble* db, const nep_cdouble* dMx, const nep_cdouble* d_den_extra,
                              nep_cdouble* dr, double* h_omega, nep_stream stream);
/* out[i] = (|x[i]|, 0): feeds the non-SPMF part of the denominator above */
int32_t nep_absvec(int64_t len, const nep_cdouble* dx, nep_cdouble* dout, nep_stream stream);

/* ---- K5 fixed-shift solve with a host-computed sparse LU -------------------------------
 * replaces: FactorizeLinSolver / lin_solve src/LinSolvers.jl:109-137 (Afact \ x) and
 *           BackslashLinSolver :147-159; the factorisation (UMFPACK in the reference) stays on
 *           the host, one-off per shift (BASELINE.json north_star).
 * Factors satisfy Pr*A*Pc = L*U with L unit lower (diagonal stored or not), U upper.  L and U are
 * given in CSR (0-based int32, complex128 values).  perm_r/perm_c follow SciPy/SuperLU:
 * (Pr b)[perm_r[i]] = b[i],  x[i] = y[perm_c[i]].  NULL perms mean identity. */
int32_t nep_lu_create(int64_t n, const int32_t* hLp, const int32_t* hLi, const nep_cdouble* hLx,
                      const int32_t* hUp, const int32_t* hUi, const nep_cdouble* hUx,
                      const int32_t* h_perm_r, const int32_t* h_perm_c, nep_lu** out);
/* The same with L and U in CSC (compressed columns: colptr, rowidx, values) -- the layout UMFPACK (Julia's `F.L`, `F.U`,
 * SparseMatrixCSC) and SuperLU (SciPy's `lu.L`, `lu.U`) hand out, so the host never converts.  Row indices inside a
 * column need not be sorted. */
int32_t nep_lu_create_csc(int64_t n, const int32_t* hLp, const int32_t* hLi, const nep_cdouble* hLx,
                          const int32_t* hUp, const int32_t* hUi, const nep_cdouble* hUx,
                          const int32_t* h_perm_r, const int32_t* h_perm_c, nep_lu** out);
/* Same-pattern refactorisation (src/method_beyncontour.jl:89-94 factors N matrices M(sigma + g(t_i)) of one sparsity
 * pattern; src/LinSolverCreators.jl:62-122 recycles by lambda): new values for the factors `lu` was created with, in the
 * same entry order (and the same CSR/CSC layout).  Only the numeric part runs: value upload + the device kernels that
 * invert the diagonal blocks.  The symbolic analysis (elimination tree, block partition, index arrays) is also shared
 * automatically between nep_lu_create[_csc] calls whose L/U patterns and permutations coincide (pattern-hash cache). */
int32_t nep_lu_refactor(nep_lu* lu, const nep_cdouble* hLx, const nep_cdouble* hUx);
/* Row scaling of the factorised matrix: the factors are those of Pr*diag(rs)*A*Pc (Julia's UMFPACK wrapper:
 * F.L*F.U == (F.Rs .* A)[F.p, F.q], i.e. rs = F.Rs), so every right-hand side is multiplied by rs on the way in (inside the
 * first kernel of the solve).  h_rs: n doubles, NULL removes it. */
int32_t nep_lu_set_row_scale(nep_lu* lu, const double* h_rs);
int32_t nep_lu_destroy(nep_lu* lu);
/* X = A^{-T} B (conj = 0) or A^{-H} B (conj = 1) with the factors `lu` holds: the factor pair (U^T D^-1, D L^T), D = diag(U)
 * (conjugated for conj = 1), perm_r and perm_c swapped.  A row scale rs of `lu` (Pr diag(rs) A Pc = LU) becomes an OUTPUT scale:
 * x = rs .* y (the scale `lu` has at this call).  No factor value goes to the host and nothing is refactorised: the pair's values
 * are gathered on the device from those of `lu`, its symbolic analysis runs once per pattern (cached).  `lu` is only read.
 * The result is an ordinary handle (nep_lu_solve / _solve_add / _info / _schedule / _destroy; not nep_lu_refactor); either
 * handle may be destroyed first.  NEP_ERR_UNSUPPORTED for a level-schedule handle (NEP_LU_SCHED=old, refused patterns).
 * replaces: the second create_linsolver(..., nept, sigma) of src/method_infbilanczos.jl:62 and src/method_rfi.jl:63 */
int32_t nep_lu_transpose(nep_lu* lu, int32_t conj, nep_lu** out);
/* hint for the NEXT nep_lu_create of the calling thread: how many solves the factorisation will serve (default 50).
 * It sizes the dense tail block whose inverse is built at creation time (one-off ~T^2/256 us vs a shorter
 * dependency chain per solve): FactorizeLinSolver (iar/tiar: maxit solves) passes a large number,
 * BackslashLinSolver (one block solve per factorisation, src/LinSolvers.jl:157-159) passes 1. */
int32_t nep_lu_set_expected_solves(int32_t nsolves);
/* host threads of the plan enumeration of nep_lu_refac_create when it runs on the host (0 = default 6; the variable
 * NEP_LU_PLAN_THREADS overrides): a setter instead of an environment write from a running multi-threaded host */
int32_t nep_lu_set_plan_threads(int32_t n);
/* info[0]=n info[1]=nnz(L) info[2]=nnz(U) info[3]=dependent steps(L) info[4]=dependent steps(U)
 * info[5]=bytes one solve with one right-hand side moves under the schedule in use (the ALGORITHMIC bytes of SURVEY.md
 * section 8d are (nnz(L)+nnz(U))*20 + 8(n+1) + 48n, computable from info[0..2]) */
int32_t nep_lu_info(const nep_lu* lu, int64_t info[6]);
/* schedule introspection.  Block schedule (default, trsv_ml.hip): out[0]=rows of the dense apex (the top levels merged into one
 * inverted block; 0 = none), out[1]=kernel launches of the last solve,
 * out[2]=out[3]=levels of the block partition, out[4]=levels whose coupling product is a separate launch (L+U),
 * out[5]=number of diagonal blocks, out[6]=rows covered by inverted blocks (= n), out[7]=largest block size.
 * Level schedule (NEP_LU_SCHED=old, and the fallback): out[0]=dense tail size T, out[1]=launches, out[2]=levels(L),
 * out[3]=levels(U) of the plain level schedule, out[4]=wide, out[5]=narrow segments, out[6]=rows of the blocked mid
 * region, out[7]=its block size.  nep_lu_is_block_schedule tells which one a handle uses. */
int32_t nep_lu_schedule(const nep_lu* lu, int64_t out[8]);
int32_t nep_lu_is_block_schedule(const nep_lu* lu, int32_t* out);
/* host-only symbolic analysis of the block schedule for a pair of factor patterns (csc = 0: CSR, 1: CSC); touches no
 * device.  out[0]=levels, out[1]=diagonal blocks, out[2]=largest block, out[3]/out[4]=coupling non-zeros / packed inverse
 * entries of L, out[5]/out[6] the same for U, out[7]=levels with a separate coupling launch.  NEP_ERR_UNSUPPORTED when the
 * patterns have a dependency outside the elimination tree (the level schedule is used then). */
int32_t nep_lu_analyze(int64_t n, int32_t csc, const int32_t* hLp, const int32_t* hLi, const int32_t* hUp,
                       const int32_t* hUi, int64_t out[8]);
/* X = A^{-1} B for nrhs right-hand sides; dB, dX: n x nrhs column-major; dX may alias dB (then ldx = ldb).
 * scale is applied to the result (iar/tiar use -1: y = -lin_solve(...), src/method_iar.jl:103).
 * ldb, ldx >= n: the rows n .. ld - 1 of a column are neither read nor written.  NEP_ERR_ARG, with nothing written, for
 * nrhs < 1 (an empty block is not a no-op) or nrhs > 65535, a leading dimension below n, a NULL handle or buffer. */
int32_t nep_lu_solve(nep_lu* lu, int32_t nrhs, const nep_cdouble* dB, int64_t ldb, nep_cdouble* dX,
                     int64_t ldx, double scale, nep_stream stream);

/* X = scale * (Add + A^{-1} B): the update step of the iterative refinement (x + A^{-1} r, UMFPACK's solve behind
 * src/LinSolvers.jl:114-122) fused into the output permutation; dAdd may alias dX, NULL means zero.  The argument checks of nep_lu_solve apply;
 * ldadd >= n is required when dAdd is given and ignored when it is NULL. */
int32_t nep_lu_solve_add(nep_lu* lu, int32_t nrhs, const nep_cdouble* dB, int64_t ldb, const nep_cdouble* dAdd,
                         int64_t ldadd, nep_cdouble* dX, int64_t ldx, double scale, nep_stream stream);

/* ---- small BLAS-1 style helpers used by the drivers ------------------------------------ */
/* iar basis step (src/method_iar.jl:100-101,105): dst[(j+1)*n + r] = src[j*n + r]/(j+1), j=0..k-1 */
int32_t nep_iar_shift_scale(int64_t n, int32_t k, const nep_cdouble* dsrc, nep_cdouble* ddst,
                            nep_stream stream);
/* NLEIGS continuation-vector helpers (src/method_nleigs.jl:399-518, backslash):
 *   nep_rk_bw:       Bw[0:n] = 0; Bw[i n + r] = wc[(i-1) n + r] + c[i-1]*wc[i n + r], i = 1..N     (:418-435)
 *   nep_block_recur: x_i = a[i-1]*y_i + b[i-1]*x_{i-1}, i = 1..N, blocks of n entries, x_0 given   (:445-487, :496-515)
 * h_c, h_a, h_b are host arrays of N complex coefficients. */
int32_t nep_rk_bw(int64_t n, int32_t N, const nep_cdouble* dwc, const nep_cdouble* h_c, nep_cdouble* dBw,
                  nep_stream stream);
int32_t nep_block_recur(int64_t n, int32_t N, const nep_cdouble* h_a, const nep_cdouble* h_b, const nep_cdouble* dy,
                        nep_cdouble* dx, nep_stream stream);
/* HOST function (no device work): the boundary points of src/rk_helper/discretizepolygon.jl for a polygon of nz >= 3 vertices --
 * npts points at equal arc length, walked point by point exactly as the reference does (alph += remL / d per point; the Leja-Bagby
 * selection of nleigs takes an argmax over these candidates, so the walk is reproduced operation by operation, without contraction
 * into fused multiply-adds: bit-identical to the interpreted walk it replaces -- 10 000 iterations, 8 ms of a nleigs call).
 * h_z: nz vertices; h_out: npts points (the vertices the reference appends behind them are the caller's to add). */
int32_t nep_discretize_polygon(int32_t nz, const nep_cdouble* h_z, int32_t npts, nep_cdouble* h_out);
/* y += alpha * x   (len complex entries); K8 quadrature accumulation
 * src/method_contour_common.jl:88-90 (S[:,:,j] += temp*G[i,j]) */
int32_t nep_axpy(int64_t len, nep_cdouble alpha, const nep_cdouble* dx, nep_cdouble* dy,
                 nep_stream stream);
/* x *= alpha */
int32_t nep_scal(int64_t len, nep_cdouble alpha, nep_cdouble* dx, nep_stream stream);
/* ||x||_2 of len complex entries (synchronous).  The squares are summed unscaled (as in K6): entries whose squares overflow or
 * underflow (beyond about 1e+-150) are outside the contract of nep_nrm2 / nep_colnorms / nep_rowmajor_colnorms. */
int32_t nep_nrm2(int64_t len, const nep_cdouble* dx, double* h_out, nep_stream stream);
/* column norms of a column-major rows x k block (synchronous) */
int32_t nep_colnorms(int64_t rows, int32_t k, const nep_cdouble* dX, int64_t ldx, double* h_out,
                     nep_stream stream);
/* dot products d_j = x_j^H y_j of the columns of two rows x k blocks (synchronous); ldx = 0 (or ldy = 0) is accepted and means
 * one column against k columns */
int32_t nep_coldots(int64_t rows, int32_t k, const nep_cdouble* dX, int64_t ldx,
                    const nep_cdouble* dY, int64_t ldy, nep_cdouble* h_out, nep_stream stream);
/* same without conjugation, d_j = x_j^T y_j: the bilinear sums `mat_sum` of the infinite Lanczos three-term recurrence
 * for symmetric NEPs (src/method_ilan.jl:299-308) */
int32_t nep_coldotsu(int64_t rows, int32_t k, const nep_cdouble* dX, int64_t ldx,
                     const nep_cdouble* dY, int64_t ldy, nep_cdouble* h_out, nep_stream stream);
/* y = d .* (A^H x), result on the device (no synchronisation); A: rows x k column-major, d: k entries or NULL.
 * replaces: R(nep, Rinv(nep, v) ./ coeffs) -- the boundary-operator inverse of the waveguide problem,
 *           src/gallery_extra/waveguide/Waveguide.jl:159-170,270-294 (dense scaled-DFT matrix instead of FFTs), and
 *           `alpha = M\b` of the Sylvester-SMW preconditioner, waveguide_preconditioner.jl:378 (M^{-1} precomputed). */
int32_t nep_gemv_hd(const nep_cdouble* dA, int64_t lda, int64_t rows, int32_t k, const nep_cdouble* dx,
                    const nep_cdouble* dd, nep_cdouble* dy, nep_stream stream);
/* out[r] = sum_j A[r,j]*B[r,j] (column-major blocks, no conjugation); lda, ldb >= rows, else NEP_ERR_ARG */
int32_t nep_rowdot(int64_t rows, int32_t k, const nep_cdouble* dA, int64_t lda, const nep_cdouble* dB, int64_t ldb,
                   nep_cdouble* dout, nep_stream stream);
/* A[r,j] *= B[r,j] (column-major blocks); lda, ldb >= rows, else NEP_ERR_ARG; B may be A itself (squares in place) */
int32_t nep_hadamard(int64_t rows, int32_t k, nep_cdouble* dA, int64_t lda, const nep_cdouble* dB, int64_t ldb,
                     nep_stream stream);
/* column 2-norms of a ROW-major rows x k block (row stride ld); synchronous */
int32_t nep_rowmajor_colnorms(int64_t rows, int32_t k, const nep_cdouble* dXT, int64_t ld, double* h_out,
                              nep_stream stream);
/* out-of-place transpose: row-major (rows x k, ld lds) -> column-major (ldd), selected columns
 * cols[0..ncols) (host int32, NULL = all) */
int32_t nep_rowmajor_to_colmajor(int64_t rows, int32_t k, const nep_cdouble* dsrc, int64_t lds,
                                 const int32_t* h_cols, int32_t ncols, nep_cdouble* ddst,
                                 int64_t ldd, nep_stream stream);

/* ---- waveguide preconditioner: Sylvester solve and region operators --------------------------------------
 * replaces: solve_wg_sylvester_fft! src/gallery_extra/waveguide/waveguide_preconditioner.jl:120-219 (FFT along z, sine
 *           transform along x) and the region means / expansions of solve_smw :263-304,:382-412.
 * nep_wep_sylv: X <- solution of A(sigma) X + X B = X in place (nz x nx, column-major): prime-factor DFT along z (dense small
 * DFTs out of LDS), one tridiagonal solve along x per z-mode (d_i I + B, B = tridiag(1,-2,1)*b) by in-wave scans, inverse
 * DFT.  h_d: the nz eigenvalues d_i of the z-operator in the basis F^H X (including sigma^2 + k_bar).  nx <= 2048. */
typedef struct nep_wep_sylv nep_wep_sylv;
int32_t nep_wep_sylv_create(int32_t nz, int32_t nx, const nep_cdouble* h_d, double b, nep_wep_sylv** out);
int32_t nep_wep_sylv_destroy(nep_wep_sylv* s);
int32_t nep_wep_sylv_info(const nep_wep_sylv* s, int32_t out[4]);   /* N1, N2 (nz = N1 N2 coprime), columns per workgroup, SEG of k_tridiag_modes (x per lane) */
int32_t nep_wep_sylv_solve(nep_wep_sylv* s, nep_cdouble* dX, nep_stream stream);
/* Dispatch query of the waveguide kernels: which instantiation the entry points named by `op` launch on an nz x nx grid.  Host
 * only: touches no device, launches nothing; it evaluates the very functions the launchers call (tests assert with it that
 * their cases reach the instantiation they are named for).
 *   op = NEP_WEP_PLAN_SYLV  nep_wep_sylv_create / nep_wep_sylv_solve
 *        NEP_WEP_PLAN_PINV  nep_wep_pinv_create / nep_wep_pinv_apply and the boundary half of nep_wep_schur_matvec (nx ignored)
 *        NEP_WEP_PLAN_SMW   nep_wep_smw_apply / nep_wep_smw_matrix_modes
 *   info[0], info[1] N1, N2 (nz = N1 N2 coprime, smallest N1 + N2)
 *   info[2] NEP_WEP_PLAN_K_RB | _PLAIN | _SYM: k_dft_cols_rb, k_dft_cols, k_dft_cols_sym (SYLV, SMW); k_wep_pinv, k_wep_pinv_sym (PINV)
 *   info[3] grid columns per workgroup (PINV: 1)      info[4] outputs per thread of a dense stage (KB)
 *   info[5] threads per workgroup                     info[6] dynamic LDS bytes of that kernel; SMW: of the row buffer of
 *                                                             k_tridiag_modes<SEG, 1> (the transform is the one SYLV reports)
 *   info[7] SEG of k_tridiag_modes (PINV: 0)
 * NEP_ERR_UNSUPPORTED (info all zero) exactly where the entry point refuses: nz beyond the LDS staging of the transform (SYLV,
 * SMW) or of P^{-1} (PINV, SMW); SMW without the symmetric-half form or with a row buffer above 150 KiB.
 * NEP_ERR_ARG: info NULL, unknown op, nz < 1; SYLV and SMW: nx < 2 or nx > 2048; SMW: nx != nz + 4. */
#define NEP_WEP_PLAN_SYLV 0
#define NEP_WEP_PLAN_PINV 1
#define NEP_WEP_PLAN_SMW 2
#define NEP_WEP_PLAN_K_RB 1
#define NEP_WEP_PLAN_K_PLAIN 2
#define NEP_WEP_PLAN_K_SYM 3
int32_t nep_wep_plan(int32_t nz, int32_t nx, int32_t op, int64_t info[8]);
/* boundary operator of the waveguide: dOut (2 nz) = blkdiag(R, R) diag(d_sinv) blkdiag(R, R)^H dX with R x = reverse(bb .* fft(x))
 * (Waveguide.jl:53-65) and d_sinv = 1 / (nz s_j(lam)) (P_inv_m / P_inv_p, Waveguide.jl:159-170): two prime-factor DFTs per half
 * in ONE launch (replaces four dense nz x nz GEMVs).  dOut may alias dX. */
typedef struct nep_wep_pinv nep_wep_pinv;
int32_t nep_wep_pinv_create(int32_t nz, const nep_cdouble* h_bb, nep_wep_pinv** out);
int32_t nep_wep_pinv_destroy(nep_wep_pinv* p);
int32_t nep_wep_pinv_apply(nep_wep_pinv* p, const nep_cdouble* d_sinv, const nep_cdouble* dX, nep_cdouble* dOut, nep_stream stream);
/* Schur complement of the waveguide applied matrix-free (SchurMatVec, /root/reference/src/gallery_extra/waveguide/Waveguide.jl:394-425):
 * dOut (nz nx) = vec(A(lam) X + X B + K .* X) - C1 P(lam)^{-1} C2T v for X = reshape(dV, nz, nx).  The interior operator is a
 * five-point stencil: weights cp / cm on the z + 1 / z - 1 neighbours (periodic), cx on the x - 1 / x + 1 neighbours (Dirichlet), the
 * diagonal dD0 (nz nx entries: K + lam^2 - 2/hz^2 - 2/hx^2); C2T v = d1 X[:, 0] + d2 X[:, 1] (and the mirror image at the other
 * end), C1 = c1s times the first / last column (generate_fd_boundary_mat).  dP: 2 nz entries of work.  dV and dOut must differ. */
int32_t nep_wep_schur_matvec(nep_wep_pinv* p, const nep_cdouble* d_sinv, int32_t nx, const nep_cdouble* dV, const nep_cdouble* dD0,
                             nep_cdouble cp, nep_cdouble cm, double cx, double d1, double d2, double c1s, nep_cdouble* dP,
                             nep_cdouble* dOut, nep_stream stream);
/* Sylvester-SMW matrix (generate_smw_matrix, waveguide_preconditioner.jl:221-313): column kappa of dM (mm x mm column-major,
 * mm = N (N+4)) = region means of Linv(E_kappa); the caller adds the identity and inverts.  All mm columns in one call (1517
 * Sylvester solves at N = 37).  dWork: nz*nx + 4 nz + mm complex. */
int32_t nep_wep_smw_matrix(nep_wep_sylv* s, nep_wep_pinv* p, int32_t N, const nep_cdouble* dKsc, double dd1, double dd2,
                           const nep_cdouble* d_sinv, nep_cdouble* dWork, nep_cdouble* dM, nep_stream stream);
/* The same matrix in mode space (column kappa = G S(Tsolve(F^H E_kappa)), dG as in nep_wep_smw_apply): no back transform, the
 * interior-region columns batched and restricted to the L grid columns of their region.  NEP_ERR_UNSUPPORTED like nep_wep_smw_apply. */
int32_t nep_wep_smw_matrix_modes(nep_wep_sylv* s, nep_wep_pinv* p, int32_t N, const nep_cdouble* dKsc, double dd1, double dd2,
                                 const nep_cdouble* d_sinv, const nep_cdouble* dG, nep_cdouble* dM, nep_stream stream);
/* One application of the Sylvester-SMW preconditioner, in place on dR (nz nx) (solve_smw, waveguide_preconditioner.jl:323-421):
 * dR <- Linv dR - Linv(sum_k alpha_k E_k), alpha = M^{-1} f(Linv dR).  Three transforms instead of four: the region means f are
 * taken in mode space (f = G S, S = x-region sums of the tridiagonal solutions) and the second solve is subtracted in mode space;
 * the expansion sum_k alpha_k E_k is formed inside the transform's loader from dKsc.  dMinvH: (M^{-1})^H, mm x mm column-major;
 * dG (N x nz, row rz at dG + rz nz): G[rz, i] = mean over the z of region rz of exp(-2 pi i z i / nz) / sqrt(nz).
 * NEP_ERR_UNSUPPORTED when nz has no odd coprime factorisation that fits the symmetric-half DFT kernel (use the pieces above). */
int32_t nep_wep_smw_apply(nep_wep_sylv* s, nep_wep_pinv* p, int32_t N, const nep_cdouble* dKsc, double dd1, double dd2,
                          const nep_cdouble* d_sinv, const nep_cdouble* dMinvH, const nep_cdouble* dG, nep_cdouble* dR,
                          nep_stream stream);
/* dOut (N x (N+4), column-major) = means of X over the N x (N+4) regions (interior regions L x L with L = nz/N, the four
 * boundary columns of X are regions of their own); needs nx = nz + 4 */
int32_t nep_wep_region_means(int32_t nz, int32_t nx, int32_t N, const nep_cdouble* dX, nep_cdouble* dOut, nep_stream stream);
/* dY[z, x] = alpha[region(z), region(x)] * Ksc[z, x];  dEb (nz x 2): dd1/dd2 combinations of the boundary region columns */
int32_t nep_wep_region_expand(int32_t nz, int32_t nx, int32_t N, const nep_cdouble* dAlpha, const nep_cdouble* dKsc, double dd1,
                              double dd2, nep_cdouble* dY, nep_cdouble* dEb, nep_stream stream);

/* ---- numeric LU factorisation on the device for a known pattern ----------------------------------------------
 * replaces: the numeric phase of `lu(A)` / `factorize` behind FactorizeLinSolver (src/LinSolvers.jl:109-122) for the second
 *           and later matrices of one sparsity pattern: the N same-pattern factorisations of contour_beyn
 *           (src/method_beyncontour.jl:89-94), the shifts of nleigs, repeated solves of one problem.  The first matrix of a
 *           pattern is factorised on the host (ordering, pivot sequence, fill pattern); nep_lu_refac_create enumerates the
 *           updates of the right-looking factorisation for that pivot sequence once, nep_lu_factor_dev computes the values of
 *           L and U on the GPU (static pivoting, as KLU / PARDISO refactorisation) and returns an ordinary nep_lu handle.
 * ref: a handle created by nep_lu_create_csc from (Lp, Li, Up, Ui, perm_r, perm_c); Ap / Ai: CSC pattern of the matrices to
 * come (caller's numbering), perm_r[i] / perm_c[j]: position of row i / column j of A in the factored matrix.
 * NEP_ERR_UNSUPPORTED: level-schedule handle, or the stored pattern is not closed under the elimination.
 * nep_lu_factor_dev: h_Ax = the nnz(A) values in the order of (Ap, Ai); growth_limit: largest accepted value of BOTH max |L|
 * (|Re|+|Im|; a diagonally pivoted factor stays near 1) and the element growth max|U| / max|A| (the stored pivot sequence may
 * not suit the new values; growth in U is what bounds the backward error of a static-pivot factorisation);
 * h_health[3] (may be NULL): [0] pivot breakdown flag, [1] max |L|, [2] max|U| / max|A|; h_LUx_out (may be NULL): the nnz(L) + nnz(U)
 * computed values in the input entry order (tests).  NEP_ERR_SINGULAR: breakdown / growth -- factorise on the host instead. */
typedef struct nep_lu_refac nep_lu_refac;
int32_t nep_lu_refac_create(nep_lu* ref, int64_t n, const int32_t* Lp, const int32_t* Li, const int32_t* Up, const int32_t* Ui,
                            const int32_t* perm_r, const int32_t* perm_c, const int32_t* Ap, const int32_t* Ai,
                            nep_lu_refac** out);
int32_t nep_lu_refac_destroy(nep_lu_refac* r);
/* Host-only analysis of a plan (no device is touched): symbolic partition + the complete enumeration of nep_lu_refac_create with
 * the plan arrays hashed instead of uploaded.  out[0] = products, [1] internal, [2] external, [3] external destination segments,
 * [4] wide, [5] wide pivot steps, [6] levels, [7] hash of the plan arrays (independent of NEP_LU_PLAN_THREADS).  Sanitizer
 * build (tests/sanitize) and thread-count invariance test. */
int32_t nep_lu_refac_analyze(int64_t n, const int32_t* Lp, const int32_t* Li, const int32_t* Up, const int32_t* Ui,
                             const int32_t* perm_r, const int32_t* perm_c, const int32_t* Ap, const int32_t* Ai, int64_t out[8]);
/* out[0..5] = n, products, internal products, external products, external destination segments, symbolic time in ms */
int32_t nep_lu_refac_info(const nep_lu_refac* r, int64_t out[6]);
/* The "wide" levels (top of the elimination tree: few blocks, one long chain of pivots each) are factorised in panels of P
 * consecutive pivots per launch (round 4; NEP_LU_WIDE_P = 1..4, default 4; 1 = one launch per pivot step as before):
 * out[0] = P (1 for a plan whose wide levels hold no product: nothing to put in panels), [1] = pivot steps of the wide levels, [2] = launches they take per factorisation, [3] = destination records,
 * [4] = deferred products (updates into a panel's own later rows / columns, applied at the end of the level). */
int32_t nep_lu_refac_wide_info(const nep_lu_refac* r, int64_t out[5]);
/* out[0] = hash of the plan arrays as they sit on the device (the quantity nep_lu_refac_analyze returns in out[7] for the host
 * enumeration of the same inputs), out[1] = 1 when the products were enumerated on the device (the default), 0 when on
 * host threads (the fallback).  Round 3: the enumeration of nep_lu_refac_create runs on the GPU (0.10-0.18 s -> a few ms for the gun pattern). */
int32_t nep_lu_refac_hash(const nep_lu_refac* r, int64_t out[2]);
int32_t nep_lu_factor_dev(nep_lu_refac* r, const nep_cdouble* h_Ax, int32_t expected_solves, double growth_limit,
                          double* h_health, nep_cdouble* h_LUx_out, nep_lu** out, nep_stream stream);
/* B matrices of the plan's pattern in one pass (every launch carries all of them): h_Ax B x nnz(A), h_health B x 3 (required),
 * out[b] = NULL for a matrix whose factorisation was refused -- factorise that one on the host. */
int32_t nep_lu_factor_dev_batch(nep_lu_refac* r, int32_t B, const nep_cdouble* h_Ax, int32_t expected_solves, double growth_limit,
                                double* h_health, nep_cdouble* h_LUx_out, nep_lu** out, nep_stream stream);
/* The same for matrices that are combinations of `mt` terms on the plan's pattern, A_b = sum_t h_Cf[b*mt + t] A_t
 * (M(lam_b) = sum_t f_t(lam_b) A_t at the quadrature nodes of src/method_beyncontour.jl:89-94): d_D is a DEVICE array, nnz(A) x mt
 * entry-major, with the values of every term scattered onto the union pattern (uploaded once per NEP); the B x nnz(A) value
 * block is formed inside the scatter kernel instead of on the host. */
int32_t nep_lu_factor_dev_batch_terms(nep_lu_refac* r, int32_t B, const nep_cdouble* d_D, int32_t mt, const nep_cdouble* h_Cf,
                                      int32_t expected_solves, double growth_limit, double* h_health, nep_lu** out,
                                      nep_stream stream);

/* the library's own device-wide primitives (csrc/devprims.h: reduce-then-scan exclusive prefix sum; stable LSD radix sort, 8-bit
 * digits, wave-ballot ranking) that the one-off plan enumeration of nep_lu_refac_create runs on -- no hipCUB / rocPRIM behind the
 * ABI.  d_out[i] = sum_{j<i} d_in[j]; (d_keys, d_vals) sorted in place by the key bits [0, nbits), equal keys keep their order.
 * Asynchronous.  Entry points for tests and diagnostics. */
int32_t nep_devprim_exclusive_sum(const uint64_t* d_in, uint64_t* d_out, int64_t n, nep_stream stream);
int32_t nep_devprim_sort_pairs(uint64_t* d_keys, uint64_t* d_vals, int64_t n, int32_t nbits, nep_stream stream);

/* ---- one infinite-Arnoldi step as one call ------------------------------------------------------
 * replaces: the loop body of iar between two eigenvalue checks, src/method_iar.jl:94-109
 *           (compute_Mlincomb! at sigma through the DerSPMF table :1130-1160, lin_solve, the 1/j shift of the block
 *           structure, orthogonalize_and_normalize!).  Sequences nep_mlincomb_dev, nep_lu_solve[_add] (+ refine_steps blind
 *           refinement steps on nep_cw_backward_error's residual), nep_iar_shift_scale and nep_orth_dev, then copies row k-1 of
 *           the device H block ((m+4) complex per row: h[0..k), beta, flags, then 4 doubles = UMFPACK's componentwise backward
 *           error omega of the refinement iterates x_0..x_refine_steps when h_cabs/h_cf were given) to the caller's PINNED host
 *           block behind an event.  Nothing waits for the device; nep_iar_wait(k) blocks until H's column k has arrived; the
 *           host replays UMFPACK's stopping rule on the recorded omegas instead of reading them back inside the step.
 *           dH must be zero-filled by the caller (m rows of m+4).
 * dV: the basis, column j at dV + j*ldv (ldv >= n(m+1), zero-initialised, column 0 = start vector); dCtab: the DerSPMF
 * coefficient table (mt columns of ldc >= m entries, row j-1 = alpha_j/j f^(j)(sigma)); d_active: device int64[m+1], active
 * rows per basis column; dwork3n: 3n complex of scratch; h_cabs / h_cf: |f_t(sigma)| and f_t(sigma) for the refinement
 * (may be NULL when refine_steps is always 0); orth_method: 0 DGKS, 1 CGS. */
typedef struct nep_iar nep_iar;
int32_t nep_iar_create(nep_spmf* spmf, nep_lu* lu, int64_t n, int32_t m, nep_cdouble* dV, int64_t ldv,
                       const nep_cdouble* dCtab, int64_t ldc, const int64_t* d_active, nep_cdouble* dwork3n,
                       const double* h_cabs, const nep_cdouble* h_cf, int32_t mt, nep_cdouble* dH, nep_cdouble* h_pinnedH,
                       int32_t orth_method, nep_iar** out);
int32_t nep_iar_destroy(nep_iar* s);
/* refine_steps | 0x100: the backward error of the KEPT iterate is recorded only in steps whose index is a multiple of 8 (its slot
 * stays 0 otherwise) -- for callers whose refinement count has settled (the check costs one pass over the matrices per step).
 * What step k writes: rows 0 .. (k+1)n - 1 of column k of dV; row k-1 of dH and of the pinned block (entries 0 .. k+3, nothing
 * behind them); and, on the fused path only (mt <= 4 and NEP_IAR_FUSE_VC not 0 when the object was created) and only for k < m,
 * the shifted blocks of column k+1, rows n .. (k+2)n - 1 = column k divided blockwise by 1 .. k+1, which step k+1 then uses as
 * they are (together with a coefficient product the object keeps for it).  Rows 0 .. n-1 of column k+1, every later column,
 * the padding between n(m+1) and ldv and the columns < k are not written.  A caller that edits column k between step k and
 * step k+1 (a restart, a re-orthogonalisation of its own) must create a new object: the hand-over would be stale. */
int32_t nep_iar_step(nep_iar* s, int32_t k, int32_t refine_steps, nep_stream stream);
/* steps k0 .. k0+count-1 (same refine_steps) in one foreign call */
int32_t nep_iar_steps(nep_iar* s, int32_t k0, int32_t count, int32_t refine_steps, nep_stream stream);
int32_t nep_iar_wait(nep_iar* s, int32_t k);
/* device-side counterpart of nep_iar_wait: work enqueued on `stream` after this call starts only when column k of H is
 * complete (the eigen-decomposition of step k on a second stream: nep_hess_eigvals_dev on row block dH of nep_iar_create) */
int32_t nep_iar_stream_wait(nep_iar* s, int32_t k, nep_stream stream);
/* nep_iar_wait without the wait: *ready = 1 when column k of H has reached the pinned block, 0 while it has not */
int32_t nep_iar_ready(nep_iar* s, int32_t k, int32_t* ready);
/* Events only where something waits.  By default every step records an event (one more command on the stream per step); a
 * caller that knows which steps it will pass to nep_iar_wait / nep_iar_ready / nep_iar_stream_wait names them: mask holds m + 1
 * bytes indexed by the step (entry 0 unused, copied), step k records its event iff mask[k] != 0.  The three calls above return
 * NEP_ERR_ARG for a step that recorded none.  NULL: every step records.  To be called before the first step of the object:
 * NEP_ERR_ARG once a step has been issued. */
int32_t nep_iar_event_mask(nep_iar* s, const uint8_t* mask);

/* ---- a shift-and-invert Krylov-Schur eigensolver for a linear pencil A x = d B x (csrc/lineig.hip) ------------------------
 * K13  in-place basis rotation, the compression step of a Krylov-Schur restart:
 *   V[:, 0:p] <- V[:, 0:m] Q;   carry != 0: V[:, p] <- V[:, m]  (the residual vector v_{m+1} moves next to the kept block)
 * replaces: the basis update of ArnoldiMethod.jl's restart behind `partialschur(..., which=LM())`, src/LinSolvers.jl:409 (an
 *           out-of-place product V[:, 1:m] * Q[:, 1:p] and a copy back there; composed from nep_gemm_ts it would need a second
 *           rows x p block).
 * dV: rows x (m + 1) column-major device block (ldv); hQ: m x p complex column-major HOST table (ldq) that may be freed or
 * overwritten on return (staged through a pinned ring into a device slot that is not handed out again before the kernel that
 * reads it has finished: calls may follow each other at once).  Rows >= `rows` of a column, the padding between rows and ldv
 * and the columns > m are neither read nor written; column m is read only with carry; the columns p + (carry != 0) .. m - 1
 * are left unspecified.  Asynchronous; ONE launch, no scratch of the size of the basis, no atomics, fixed summation order (k
 * ascending): two calls on equal inputs give the same bits.  Bytes moved: 16 rows (m + p).
 * NEP_ERR_ARG (nothing launched, V unchanged) for a NULL dV / hQ, rows < 1, m < 1, p < 1, p > m, ldv < rows, ldq < m;
 * NEP_ERR_UNSUPPORTED (nothing launched) for m > 128. */
int32_t nep_basis_rotate(nep_cdouble* dV, int64_t ldv, int64_t rows, int32_t m, int32_t p, const nep_cdouble* hQ, int64_t ldq,
                         int32_t carry, nep_stream stream);

/* Arnoldi expansion for the operator C^-1 B of a pencil carried as an SPMF handle plus coefficient rows, B = sum_t cB_t A_t,
 * C = tau B - A = sum_t (tau cB_t - cA_t) A_t factorised by the caller (any nep_lu handle).
 * replaces: the shift-and-invert operator x -> Cfact \ (B x) of inner_eigs_solve, src/LinSolvers.jl:390-416, expanded by
 *           ArnoldiMethod.jl there; its caller is the loop of the method of successive linear problems, src/method_mslp.jl:61-70.
 * Step j (0-based): w = sum_t cB_t A_t v_j (nep_mlincomb_dev), w <- C^-1 w (nep_lu_solve), DGKS or CGS of w against
 * V[:, 0..j] (nep_orth_dev without an active-row table), w / beta to column j + 1, and row j of the device coefficient block dS
 * (maxdim rows of maxdim + 4 complex: the j + 1 projection coefficients -- a full column, not a Hessenberg one: after a restart
 * the kept block is not Hessenberg --, then (beta, 0), then the flag word (passes, 2 breakdown + another_pass_wanted)) is copied
 * to the caller's PINNED host block of the same layout behind an event.  The flag word is the one of nep_orth_dev, unchanged.  A
 * new vector inside span(V) is reported through it only: breakdown is set when beta is not a positive finite number, and
 * another_pass_wanted when the last DGKS pass still asked for another one (the vector lies in span(V) to working precision:
 * "twice is enough"), so a DGKS step with a non-zero second component of its flag word has found an invariant subspace.  Later
 * columns of the same call are then unspecified but every call returns NEP_OK.
 * dV: n x (maxdim + 1) column-major (ldv >= n), column 0 = the normalised start vector; d_cB: the mt coefficients of B on the
 * device; dwork_n: n complex of scratch; orth_method: 0 DGKS, 1 CGS.  nep_arnoldi_steps enqueues steps j0 .. j0 + count - 1 and
 * waits for nothing; nep_arnoldi_wait blocks until row j has arrived.  NEP_ERR_ARG for a NULL argument, n < 1, maxdim < 1,
 * ldv < n, steps outside 0 .. maxdim - 1, a wait for a step that was never enqueued. */
typedef struct nep_arnoldi nep_arnoldi;
int32_t nep_arnoldi_create(nep_spmf* spmf, nep_lu* lu, int64_t n, int32_t maxdim, nep_cdouble* dV, int64_t ldv,
                           const nep_cdouble* d_cB, nep_cdouble* dwork_n, nep_cdouble* dS, nep_cdouble* h_pinnedS,
                           int32_t orth_method, nep_arnoldi** out);
int32_t nep_arnoldi_destroy(nep_arnoldi* s);
int32_t nep_arnoldi_steps(nep_arnoldi* s, int32_t j0, int32_t count, nep_stream stream);
int32_t nep_arnoldi_wait(nep_arnoldi* s, int32_t j);

/* ---- the whole infinite-Arnoldi run as one call ---------------------------------------------
 * replaces: the body of `iar(::Type{T}, nep::NEP; orthmethod, maxit, linsolvercreator, tol, neigs, errmeasure, sigma, gamma, v, logger,
 *           check_error_every, ...)`, src/method_iar.jl:46-182, after `create_linsolver` (:84): recurrence (:94-109, nep_iar_step),
 *           `eigen(H[1:k,1:k])` (:112, nep_hess_eig*_batch_dev), `Q = VV*Z` (:115, nep_gemm_ts_dev), `estimate_error` for every Ritz
 *           pair (:133-135, nep_resid_batch_dev; StandardSPMFErrmeasure src/errmeasure.jl:174-190 / ResidualErrmeasure :114,128-130),
 *           convergence count, sort and extraction (:137-160), the NoConvergenceException (:163-175).  A Julia method
 *           `iar(::Type{T}, nep::DeviceSPMF; ...)` is one ccall of this (julia/NEPMI355X.jl); the Python host calls it too.
 * lu: the factors of M(sigma) (nep_lu_create_csc / nep_lu_factor_dev); h_v0: the start vector (n, not normalised);
 * h_Ctab: m x mt column-major, row j-1 = gamma^j / j * f_t^(j)(sigma) (the DerSPMF table src/NEPTypes.jl:1108-1128 with iar's
 * alpha_j / j scaling :83,101); h_cabs / h_cf: |f_t(sigma)|, f_t(sigma) (required when umfpack_refinements > 0);
 * h_fro: ||A_t||_F (errmeasure 1); fv(ctx, nlam, lam, F): the host evaluates F[t + s mt] = f_t(lam[s]) (the scalar functions of
 * the SPMF are closures of the host language), returns 0 -- called on the calling thread only.
 * Results: h_lam (capacity maxit), dQ (device, n x maxit column-major, ld n; may be NULL), h_Q (host, same shape; may be NULL:
 * pinned memory gets the link's rate), h_err (maxit x maxit column-major, err[k-1 + (s-1) maxit] = sorted error s of step k, NaN
 * where unset; may be NULL), dV_basis (device, maxit+1 columns of leading dimension n (maxit+1): the Krylov basis the reference
 * returns as V[:,1:k]; NULL: library-owned and released at return).  NEP_OK: res->nret converged pairs (all pairs below tol when neigs = INFINITY); NEP_ERR_NOCONV: the
 * res->nret best pairs; NEP_ERR_RETRY / NEP_ERR_UNSUPPORTED (maxit > 128): nothing returned, use the per-step entry points.
 * h_err == NULL says that nobody reads the error history.  With neigs = INFINITY the stop test cannot fire and everything the
 * call returns comes from the check of step maxit, so then ONLY that step is checked: one eigen-decomposition, one Ritz block,
 * one residual batch, one fv callback, whatever check_error_every says; h_lam, dQ / h_Q, dV_basis and res are bit for bit what
 * the call with a buffer returns.  With a finite neigs every check step is checked, buffer or not (the stop test needs them).
 * The recorded rows of H (breakdown, a wanted DGKS pass, the refinement record) are reviewed from the recurrence's loop at a
 * fixed distance behind the steps being enqueued, checks or no checks: a miss is reported when its row has arrived, and the
 * refinement sweeps every step takes do not depend on h_err.
 * nep_iar_run_stats: what the last run of the calling thread launched -- out[0] eigen-decompositions, out[1] checks (Ritz block
 * + residual batch + callback), out[2] step events recorded, out[3] rows of H reviewed. */
typedef struct nep_iar_opts {
    int32_t maxit;               /* m */
    int32_t check_error_every;
    int32_t orth_method;         /* 0 DGKS, 1 classical Gram-Schmidt */
    int32_t umfpack_refinements; /* <= 0: plain solves; else UMFPACK's refinement rule with this bound (control[8]) */
    int32_t errmeasure;          /* 0: ||M(lam) v|| / ||v||;  1: that / sum_t ||A_t||_F |f_t(lam)| */
    int32_t refine_hint;         /* sweeps a previous run at THIS shift settled on (nep_iar_result.refine_plan), -1: none */
    double tol;
    double neigs;                /* INFINITY: run to maxit, return every pair below tol */
    nep_cdouble sigma, gamma;
} nep_iar_opts;
typedef struct nep_iar_result {
    int32_t k;                   /* step whose check produced the returned pairs */
    int32_t nconv;               /* pairs below tol at that step */
    int32_t nret;                /* pairs written to h_lam / dQ / h_Q */
    int32_t refine_plan;         /* refinement sweeps the run settled on (-1: none) -- the next run's refine_hint */
    int32_t refine_hint_off;     /* 1: a miss withdrew the hint for this NEP */
    int32_t retry_reason;        /* NEP_ERR_RETRY: 1 refinement record, 2 DGKS pass, 3 device eigen-decomposition */
} nep_iar_result;
typedef int32_t (*nep_fv_eval)(void* ctx, int32_t nlam, const nep_cdouble* lam, nep_cdouble* F);
/* UMFPACK's refinement stopping rule (umfpack_solve behind `Afact \ x` with control[8] = umfpack_refinements, src/LinSolvers.jl:
 * 114-122) replayed on the omegas w4[0..plan] that nep_iar_step recorded for a solve that took `plan` sweeps without reading them
 * back (final_recorded = 0: omega of the kept iterate x_plan was not evaluated).  out[0] = 1: what the step kept is what the checked
 * loop keeps (or at least as good); 0: a miss -- re-run with checked solves.  out[1] = sweeps to plan from now on (-1: unchanged),
 * out[2] = hint for later solvers at this shift (-1: none), out[3] = 1: the hint is withdrawn for good. */
int32_t nep_refine_review(int32_t umfpack_refinements, int32_t plan, int32_t final_recorded, const double* w4, int32_t hint_in,
                          int32_t out[4]);
int32_t nep_iar_run(nep_spmf* spmf, nep_lu* lu, int64_t n, const nep_iar_opts* opts, const nep_cdouble* h_v0,
                    const nep_cdouble* h_Ctab, int32_t mt, const double* h_cabs, const nep_cdouble* h_cf, const double* h_fro,
                    nep_fv_eval fv, void* ctx, nep_cdouble* h_lam, nep_cdouble* dQ, nep_cdouble* h_Q, double* h_err,
                    nep_cdouble* dV_basis, nep_iar_result* res, nep_stream stream);
int32_t nep_iar_run_stats(int32_t out[4]);

/* ---- multi-GPU exchange of the contour integrators ----------------------------------------
 * replaces: the reduction inside `integrate_interval(::Type{<:MatrixIntegrator}, ...)` src/method_contour_common.jl:46,61-94
 *           when the N quadrature nodes of contour_beyn / contour_block_SS (src/method_beyncontour.jl:89-104,
 *           src/method_block_SS.jl:81-86,129-135) are sharded over the GPUs of one node: rank r owns the nodes
 *           i = r (mod P) and accumulates their moments locally; the only exchange is one all-gather of the partial
 *           moment block followed by a sum in fixed rank order (bit-identical result on every rank).
 * One process per GPU.  Rank 0 obtains a 128-byte unique id and hands it to the other ranks out of band (MPI.jl bcast,
 * torch.distributed, a shared file); every rank then creates its communicator on ITS current device (collective call).
 * RCCL (librccl.so) is loaded on first use. */
int32_t nep_comm_unique_id(void* h_out128);
int32_t nep_comm_create(int32_t rank, int32_t world, const void* h_unique_id128, nep_comm** out);
int32_t nep_comm_destroy(nep_comm* c);
int32_t nep_comm_info(const nep_comm* c, int32_t out[2]);     /* out[0] = rank, out[1] = world */
/* d_total[i] = sum_{r=0}^{world-1} partial_r[i], i < len (complex128), on every rank; ncclAllGather over xGMI into a
 * library-owned world x len block + one summation kernel, all on `stream` (asynchronous).  d_total may alias
 * d_partial. */
int32_t nep_allgather_sum(nep_comm* c, const nep_cdouble* d_partial, int64_t len, nep_cdouble* d_total, nep_stream stream);
/* the reduction half of nep_allgather_sum on a caller-provided gather buffer (world x len complex128, rank r's block at
 * r * len): d_total[i] = sum_r d_parts[r * len + i] in rank order r = 0 .. world-1 (bit-identical wherever it runs);
 * d_total may alias block 0.  For tests and for hosts that move the blocks themselves. */
int32_t nep_sum_ranks(const nep_cdouble* d_parts, int64_t len, int32_t world, nep_cdouble* d_total, nep_stream stream);

/* ---- boundary-element NEP (gallery "bem_fichera"): a dense M(lam) assembled on the device -------------------------------
 * replaces: src/gallery_extra/bem_hardcoded/ -- precompute_quad! and assemble_BEM (assemble_BEM.jl:4-89: an n^2 scalar loop that
 *           allocates per entry), deHoop (deHoop.jl:30-65), the auxiliary mesh data of genmesh.jl:95-111, and the
 *           compute_Mlincomb_from_Mder delegation of bem_hardcoded.jl:36 (one assembled matrix per derivative).
 * With the 3-point Gauss rule (points g_r[i], weights w_r[i] = area_r / 3), W_p = w_r[i] w_c[j], d_p = |g_r[i] - g_c[j]|, p = (i, j):
 *   M(lam)[r, c]     = sum_p W_p (exp(i lam d_p) - 1) / d_p / (4 pi) + S0[r, c],        r <= c,
 *   M^(m)(lam)[r, c] = sum_p W_p (i d_p)^m exp(i lam d_p) / d_p / (4 pi),   m >= 1;
 * a pair with d_p == 0 contributes i lam W_p (m = 0), i W_p (m = 1), 0 (m >= 2) inside the sum; the lower triangle is the
 * mirror of the upper one.  S0: the Gauss rule over triangle r of de Hoop's closed form for triangle c, / (4 pi), with |R| + R.tau
 * evaluated as h^2 / (|R| - R.tau) where R.tau < 0 (no cancellation).
 * nep_bem_create: h_vert = n x 9 doubles (P1, P2, P3 of each triangle), h_area = n doubles; uploads the mesh, derives Gauss
 *   points, tangents, normal and edge normals and fills S0 on the device; synchronous.  NEP_ERR_UNSUPPORTED: gauss_order != 3.
 * nep_bem_info: info = (n, gauss_order, device bytes, coefficients per pass of nep_bem_mlincomb).
 * nep_bem_static: d_out (n x n doubles, column-major, ldo >= n) = S0 (mirrored).
 * nep_bem_assemble: dOut + l stride = M^(der)(h_lam[l]), l < nlam, column-major n x n (ldo >= n); the 9 distances of an entry
 *   are formed once for the whole batch; the output is bitwise symmetric; nlam = 0 is a no-op.
 * nep_bem_mlincomb: dz = sum_{j < k} h_a[j] M^(j + startder)(lam) dV[:, j], matrix-free: one pass over the pairs with a Horner
 *   loop in (i d_p), no n^2 buffer except the read of S0; k > 64 in passes of 64.  h_a[j] == 0 drops column j (never read).
 * nep_bem_resid: dOut[:, s] = M(h_lam[s]) dQ[:, s], s < k, matrix-free (dQ, dOut column-major, ldq, ldo >= n).
 * All but create are asynchronous; host arrays may be freed on return (they travel as kernel arguments).  Padding (rows >= n of
 * a column, columns beyond n) is never written.  No atomics, fixed summation order: two calls give the same bits.
 * NEP_ERR_ARG (nothing launched) for a NULL handle or block, a leading dimension < n, k < 1, nlam < 0, der < 0, startder < 0. */
typedef struct nep_bem nep_bem;
int32_t nep_bem_create(int64_t n, const double* h_vert, const double* h_area, int32_t gauss_order, nep_bem** out);
int32_t nep_bem_destroy(nep_bem* b);
int32_t nep_bem_info(const nep_bem* b, int64_t info[4]);
int32_t nep_bem_static(const nep_bem* b, double* d_out, int64_t ldo, nep_stream stream);
int32_t nep_bem_assemble(const nep_bem* b, int32_t nlam, const nep_cdouble* h_lam, int32_t der, nep_cdouble* dOut, int64_t ldo,
                         int64_t stride, nep_stream stream);
int32_t nep_bem_mlincomb(const nep_bem* b, nep_cdouble lam, int32_t k, const nep_cdouble* h_a, int32_t startder,
                         const nep_cdouble* dV, int64_t ldv, nep_cdouble* dz, nep_stream stream);
int32_t nep_bem_resid(const nep_bem* b, int32_t k, const nep_cdouble* h_lam, const nep_cdouble* dQ, int64_t ldq, nep_cdouble* dOut,
                      int64_t ldo, nep_stream stream);

/* ---- time-periodic delay NEP (gallery "periodicdde"): M(lam) by a Runge-Kutta sweep on the device (K15) -----------------
 * replaces: src/gallery_extra/periodic_dde.jl -- ode_rk4 (:112-124) inside compute_MM (:203-218), the column-by-column
 *           compute_Mder (:247-259) and its central differences for the first derivative (:260-265).
 * x'(t) = A(t) x(t) + B(t) x(t - tau), A(t) = sum_{i < mA} alpha_i(t) A_i, B(t) = sum_{j < mB} beta_j(t) B_j, both tau-periodic.
 *   MM(S, V) = Y_N - V,   Y_0 = V (n x p),   Y_{k+1} = Y_k + (s1 + 2 s2 + 2 s3 + s4) / 6,   s_i = h F(.), h = tau / N,
 *   F(t, Y) = (sum_i alpha_i(t) A_i) Y + ((sum_j beta_j(t) B_j) Y) E - Y S,
 * the classical Runge-Kutta stages at t_k, t_k + h/2, t_k + h/2, t_k + h.  With E = exp(-tau S) this is the reference's
 * compute_MM; E is an input of its own and is not checked against S.
 * nep_pdde_create: h_A = mA matrices, h_B = mB matrices, each n x n column-major, one after the other; h_alpha ((2N + 1) x mA,
 *   row-major) and h_beta ((2N + 1) x mB) hold alpha_i and beta_j at the half-step times s tau / (2N): step k reads rows 2k, 2k+1,
 *   2k+1, 2k+2.  1 <= n <= 512, 1 <= mA, mB <= 64, N >= 1.  Synchronous.
 * nep_pdde_info: info = (n, N, device bytes, largest p).
 * nep_pdde_mm: nsys systems of p <= 8 columns in ONE launch; system s has S = h_S + s p p and E = h_E + s p p (p x p,
 *   column-major, host), V = dV + s strideV (n x p, ldv >= n, device, not modified) and writes MM(S, V) to dOut + s strideO (ldo >= n).
 * nep_pdde_mder: dOut + l stride = M^(der)(h_lam[l]) (n x n, column-major, ldo >= n), l < nlam, der <= 7: a front end of the same
 *   launch with S = J_{der+1}(lam) (ones above the diagonal), E = e^(-tau lam) Toeplitz((-tau)^k / k!) formed on the host in closed
 *   form and V = [e_j, 0, ..., 0] generated on the device; column j of the matrix is der! times column der of system (l, j).
 * mm and mder are asynchronous; host arrays may be freed on return.  Nothing outside the n x p blocks (mder: the n x n matrices)
 * is written.  The sum over the inner index runs in a fixed order that belongs to the row and column alone: a system has the same
 * bits alone, at any position of any batch, and from run to run.  nsys = 0 and nlam = 0 are no-ops.
 * NEP_ERR_ARG (nothing launched) for a NULL handle or block, n outside 1..512, mA or mB outside 1..64, N outside 1..2^24, a tau
 * that is not finite, p outside 1..8, der outside 0..7, a leading dimension < n, a stride smaller than a block (nsys, nlam > 1),
 * nlam n > 2^31 - 1. */
typedef struct nep_pdde nep_pdde;
int32_t nep_pdde_create(int32_t n, int32_t mA, int32_t mB, const nep_cdouble* h_A, const nep_cdouble* h_B, int32_t N, double tau,
                        const nep_cdouble* h_alpha, const nep_cdouble* h_beta, nep_pdde** out);
int32_t nep_pdde_destroy(nep_pdde* d);
int32_t nep_pdde_info(const nep_pdde* d, int64_t info[4]);
int32_t nep_pdde_mm(const nep_pdde* d, int32_t nsys, int32_t p, const nep_cdouble* h_S, const nep_cdouble* h_E, const nep_cdouble* dV,
                    int64_t ldv, int64_t strideV, nep_cdouble* dOut, int64_t ldo, int64_t strideO, nep_stream stream);
int32_t nep_pdde_mder(const nep_pdde* d, int32_t nlam, const nep_cdouble* h_lam, int32_t der, nep_cdouble* dOut, int64_t ldo,
                      int64_t stride, nep_stream stream);

#ifdef __cplusplus
}
#endif
#endif /* NEPMI355_H */
