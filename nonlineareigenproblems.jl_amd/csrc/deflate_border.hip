// libnepmi355: the border step of a linear solve with the deflated matrix (Effenberger deflation), for gfx950.
//
// With X = V0 (n0 x p, X^H X = I) and U = M(lam) X (lam I - S0)^-1 the solution of
//
//   [ M(lam)  U ] [v1]   [b1]          y  = M(lam)^-1 b1        (the caller's solve with the ORIGINAL matrix)
//   [ X^H     0 ] [v2] = [b2]    is    c  = b2 - X^H y
//                                      v1 = y + X c,     v2 = T c     with T = -(lam I - S0),
//
// because M^-1 U = X (lam I - S0)^-1 exactly: M v1 + U v2 = b1 + M X c - M X c = b1 and X^H v1 = X^H y + c = b2.  The table T is
// the caller's: the kernels know nothing of lam or S0.
//
// Three launches.  k_border_dot: per-workgroup partials of the p dot products X[:, q]^H y (DPP wave sums, then the four waves
// through LDS).  k_border_c: one workgroup per q adds the partials in a fixed order and subtracts from b2.  k_border_apply: one
// thread per row with a grid-stride loop, c broadcast from LDS, lanes of a wave read consecutive addresses of the column-major X;
// workgroup 0 also writes the p tail entries T c.  No atomics: two calls give the same bits.  A row of y is read by the thread
// that writes that row of the result and by nobody after it, so y and the result may be the same buffer.
#include "common.h"

namespace {

constexpr int DB_THREADS = 256;
constexpr int DB_MAXP = 32;
constexpr int DB_MAXBLOCKS = 2048;   // grid cap of the streaming passes; rows beyond it are reached by the grid stride

// partial[q * gridDim.x + blockIdx.x] = sum over this workgroup's rows of conj(X[r, q]) y[r]
__global__ __launch_bounds__(DB_THREADS) void k_border_dot(int64_t n0, int p, const cplx* __restrict__ X, int64_t ldx,
                                                           const cplx* __restrict__ y, cplx* __restrict__ partial) {
    __shared__ cplx red[DB_MAXP][DB_THREADS / 64];
    const int64_t stride = (int64_t)gridDim.x * DB_THREADS;
    const int64_t r0 = (int64_t)blockIdx.x * DB_THREADS + threadIdx.x;
    for (int q = 0; q < p; ++q) {
        cplx d = cmake(0.0, 0.0);
        for (int64_t r = r0; r < n0; r += stride) cfma_conj(d, X[r + (int64_t)q * ldx], y[r]);
        d = wave_sum_dpp(d);
        if ((threadIdx.x & 63) == 0) red[q][threadIdx.x >> 6] = d;
    }
    __syncthreads();
    if (threadIdx.x < p) {
        const int q = threadIdx.x;
        partial[(int64_t)q * gridDim.x + blockIdx.x] = cadd(cadd(red[q][0], red[q][1]), cadd(red[q][2], red[q][3]));
    }
}

// c[q] = b2[q] - sum_b partial[q * nb + b]: one workgroup per q, strided per-lane sums, then the fixed wave / LDS tree
__global__ __launch_bounds__(DB_THREADS) void k_border_c(int nb, const cplx* __restrict__ partial, const cplx* __restrict__ b2,
                                                         cplx* __restrict__ c) {
    __shared__ cplx sm[DB_THREADS / 64];
    const cplx* pq = partial + (int64_t)blockIdx.x * nb;
    cplx d = cmake(0.0, 0.0);
    for (int b = threadIdx.x; b < nb; b += DB_THREADS) d = cadd(d, pq[b]);
    d = wave_sum_dpp(d);
    if ((threadIdx.x & 63) == 0) sm[threadIdx.x >> 6] = d;
    __syncthreads();
    if (threadIdx.x == 0) {
        const cplx s = cadd(cadd(sm[0], sm[1]), cadd(sm[2], sm[3]));
        c[blockIdx.x] = csub(b2 ? b2[blockIdx.x] : cmake(0.0, 0.0), s);
    }
}

// out[r] = scale (y[r] + sum_l X[r, l] c[l]), r < n0;   out[n0 + q] = scale sum_l T[q, l] c[l]   (workgroup 0)
__global__ __launch_bounds__(DB_THREADS) void k_border_apply(int64_t n0, int p, const cplx* __restrict__ X, int64_t ldx,
                                                             const cplx* y, const cplx* __restrict__ c,
                                                             const cplx* __restrict__ T, double scale, cplx* out) {
    __shared__ cplx cs[DB_MAXP];
    if (threadIdx.x < p) cs[threadIdx.x] = c[threadIdx.x];
    __syncthreads();
    const int64_t stride = (int64_t)gridDim.x * DB_THREADS;
    for (int64_t r = (int64_t)blockIdx.x * DB_THREADS + threadIdx.x; r < n0; r += stride) {
        cplx acc = y[r];
        for (int l = 0; l < p; ++l) cfma(acc, X[r + (int64_t)l * ldx], cs[l]);
        out[r] = cscale(scale, acc);
    }
    if (blockIdx.x == 0 && threadIdx.x < p) {
        const int q = threadIdx.x;
        cplx acc = cmake(0.0, 0.0);
        for (int l = 0; l < p; ++l) cfma(acc, T[q + l * p], cs[l]);
        out[n0 + q] = cscale(scale, acc);
    }
}

thread_local NepScratch g_border_scratch;
thread_local PinnedRing g_border_ring;

}  // namespace

int32_t nep_defl_border(int64_t n0, int32_t p, const nep_cdouble* dX, int64_t ldx, const nep_cdouble* dY,
                        const nep_cdouble* db2, const nep_cdouble* hT, double scale, nep_cdouble* dOut, nep_stream stream) {
    if (p < 1 || p > DB_MAXP) {
        nep_set_error("nep_defl_border: p = %d (1 <= p <= %d)", p, DB_MAXP);
        return NEP_ERR_UNSUPPORTED;
    }
    ARGCHK(dX && dY && hT && dOut);
    ARGCHK(n0 >= 1 && ldx >= n0);
    const uintptr_t b2lo = (uintptr_t)db2, outlo = (uintptr_t)dOut;
    ARGCHK(!db2 || b2lo + (uintptr_t)p * sizeof(cplx) <= outlo || outlo + (uintptr_t)(n0 + p) * sizeof(cplx) <= b2lo);
    hipStream_t st = as_stream(stream);
    const int nb = (int)((n0 + DB_THREADS - 1) / DB_THREADS < DB_MAXBLOCKS ? (n0 + DB_THREADS - 1) / DB_THREADS : DB_MAXBLOCKS);
    // device block: [T (p p) | c (p) | partial (p nb)], T uploaded in one copy
    const size_t nT = (size_t)p * p;
    int rc = g_border_scratch.ensure((nT + (size_t)p + (size_t)p * nb) * sizeof(cplx));
    if (rc) return rc;
    cplx* dT = (cplx*)g_border_scratch.dptr;
    cplx *dc = dT + nT, *partial = dc + p;
    rc = g_border_ring.upload(dT, hT, nT * sizeof(cplx), st);
    if (rc) return rc;
    const cplx *X = (const cplx*)dX, *y = (const cplx*)dY;
    hipLaunchKernelGGL(k_border_dot, dim3(nb), dim3(DB_THREADS), 0, st, n0, p, X, ldx, y, partial);
    LAUNCHCHK();
    hipLaunchKernelGGL(k_border_c, dim3(p), dim3(DB_THREADS), 0, st, nb, (const cplx*)partial, (const cplx*)db2, dc);
    LAUNCHCHK();
    hipLaunchKernelGGL(k_border_apply, dim3(nb), dim3(DB_THREADS), 0, st, n0, p, X, ldx, y, (const cplx*)dc, (const cplx*)dT,
                       scale, (cplx*)dOut);
    LAUNCHCHK();
    return NEP_OK;
}
