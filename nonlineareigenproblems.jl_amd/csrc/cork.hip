// libnepmi355: the small products of a compact rational Krylov (CORK) step, for gfx950.
//
//   Out[rho, gam] = alpha u[rho] g[gam] + sum_{q < k} U[rho, q] G[q, gam],      rho < r, gam < c
//
// U is one slab of the coefficient tensor of the CORK basis (r x k, column-major), G a k x c table of the shift that the driver
// uploaded before its loop, u the row K6 leaves on the device ([Q^H v; ||v_perp||]) and g the first row of the inverse of the
// extended pencil.  Both small products of a step (u_c = U C_sigma without the rank-1 term, Uhat = (alpha u) g^T + U G_sigma with
// it) are this call, so the tensor never leaves the device between the two Gram-Schmidt passes of a step.
//
// One launch.  Lanes run along rho: a wave reads 64 consecutive entries of a column of U (1 KiB, coalesced).  A workgroup of four
// waves owns 64 rows and a panel of CK_PANEL = 8 columns of Out, two columns per wave; the k x 8 panel of G is staged in LDS once
// (at most 32 KiB) and every lane of a wave reads the same entry of it (a broadcast: no bank conflict).  Each thread keeps its two
// sums in registers and adds the products in the order q = 0, 1, ..., k - 1, then the rank-1 term: no atomics, no reduction across
// lanes, so two calls give the same bits.  Rows >= r and the padding of U, G and Out are neither read nor written.
#include "common.h"

namespace {

constexpr int CK_ROWS = 64;                    // rows of Out per workgroup = one wave
constexpr int CK_WAVES = 4;
constexpr int CK_COLS = 2;                     // columns of Out per wave
constexpr int CK_PANEL = CK_WAVES * CK_COLS;   // columns of G staged per workgroup
constexpr int CK_MAXK = 256;
constexpr int CK_MAXC = 256;

__global__ __launch_bounds__(CK_ROWS * CK_WAVES) void k_cork_expand(int r, int k, int c, const cplx* __restrict__ U, int64_t ldu,
                                                                    const cplx* __restrict__ G, int64_t ldg,
                                                                    const cplx* __restrict__ u, const cplx* __restrict__ g,
                                                                    cplx alpha, cplx* __restrict__ Out, int64_t ldo) {
    __shared__ cplx Gs[CK_MAXK * CK_PANEL];    // Gs[q * CK_PANEL + j] = G[q, c0 + j]
    const int c0 = blockIdx.y * CK_PANEL;
    const int pc = c - c0 < CK_PANEL ? c - c0 : CK_PANEL;           // columns of this panel that exist
    for (int i = threadIdx.x; i < pc * k; i += CK_ROWS * CK_WAVES) {
        const int j = i / k, q = i - j * k;                          // consecutive threads read consecutive q of one column
        Gs[q * CK_PANEL + j] = G[q + (int64_t)(c0 + j) * ldg];
    }
    __syncthreads();
    const int rho = blockIdx.x * CK_ROWS + (threadIdx.x & 63);
    const int j0 = (threadIdx.x >> 6) * CK_COLS;                     // wave-uniform
    if (rho >= r || j0 >= pc) return;
    const bool two = j0 + 1 < pc;                                    // wave-uniform
    cplx a0 = cmake(0.0, 0.0), a1 = cmake(0.0, 0.0);
    const cplx* Ur = U + rho;
    const cplx* Gq = Gs + j0;
#pragma unroll 4
    for (int q = 0; q < k; ++q) {
        const cplx x = Ur[(int64_t)q * ldu];
        cfma(a0, x, Gq[q * CK_PANEL]);
        cfma(a1, x, Gq[q * CK_PANEL + 1]);                           // (column j0 + 1 of a short panel holds stale LDS: never stored)
    }
    if (u) {
        const cplx t = cmul(alpha, u[rho]);
        cfma(a0, t, g[c0 + j0]);
        if (two) cfma(a1, t, g[c0 + j0 + 1]);
    }
    Out[rho + (int64_t)(c0 + j0) * ldo] = a0;
    if (two) Out[rho + (int64_t)(c0 + j0 + 1) * ldo] = a1;
}

// [p, p + n) of complex entries as an address range
struct CkRange {
    uintptr_t lo, hi;
};
inline CkRange ck_range(const void* p, int64_t n) { return CkRange{(uintptr_t)p, (uintptr_t)p + (uintptr_t)n * sizeof(cplx)}; }
inline bool ck_disjoint(CkRange a, CkRange b) { return a.hi <= b.lo || b.hi <= a.lo; }

}  // namespace

int32_t nep_cork_expand(int32_t r, int32_t k, int32_t c, const nep_cdouble* dU, int64_t ldu, const nep_cdouble* dG, int64_t ldg,
                        const nep_cdouble* du, const nep_cdouble* dg, nep_cdouble alpha, nep_cdouble* dOut, int64_t ldo,
                        nep_stream stream) {
    if (k < 1 || k > CK_MAXK || c < 1 || c > CK_MAXC) {
        nep_set_error("nep_cork_expand: k = %d, c = %d (1 <= k <= %d, 1 <= c <= %d)", k, c, CK_MAXK, CK_MAXC);
        return NEP_ERR_UNSUPPORTED;
    }
    ARGCHK(dU && dG && dOut);
    ARGCHK(r >= 1 && ldu >= r && ldg >= k && ldo >= r);
    ARGCHK(!du || dg);
    const CkRange out = ck_range(dOut, ldo * (c - 1) + r);
    ARGCHK(ck_disjoint(out, ck_range(dU, ldu * (k - 1) + r)));
    ARGCHK(ck_disjoint(out, ck_range(dG, ldg * (c - 1) + k)));
    ARGCHK(!du || (ck_disjoint(out, ck_range(du, r)) && ck_disjoint(out, ck_range(dg, c))));
    const dim3 grid((r + CK_ROWS - 1) / CK_ROWS, (c + CK_PANEL - 1) / CK_PANEL);
    cplx al;
    al.x = alpha.re; al.y = alpha.im;
    hipLaunchKernelGGL(k_cork_expand, grid, dim3(CK_ROWS * CK_WAVES), 0, as_stream(stream), (int)r, (int)k, (int)c,
                       (const cplx*)dU, ldu, (const cplx*)dG, ldg, (const cplx*)du, (const cplx*)(du ? dg : nullptr), al,
                       (cplx*)dOut, ldo);
    LAUNCHCHK();
    return NEP_OK;
}
