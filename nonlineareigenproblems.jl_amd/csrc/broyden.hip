// libnepmi355: one pass over the approximate inverse Jacobian T of Broyden's method, for gfx950.
//
//   T[i, j] += u0[i] a0[j]                    (the pending rank-one update; the only write to T)
//   y[i]     = sum_j T_new[i, j] x[j]
//   g[j]     = sum_i conj(w[i]) T_new[i, j]   (the ROW w^H T_new, unconjugated)
//
// T is n x n complex128, column-major.  An inner iteration of src/method_broyden.jl touches T four times (:69 T*rk, :101 T*ztilde,
// :107 dv'*T, :117 T += Tztilde*aH); with the update kept pending for one iteration all of them are this one pass.
//
// Streaming kernel: nothing of T is used twice, so every entry is loaded once (and stored once when there is an update), 16 bytes
// per lane, a wave reading 64 consecutive rows of a column (1 KiB).  A workgroup of four waves owns a tile of BS_TR = 1024 rows
// and BS_TC = 64 columns: thread t holds rows r0 + t + 256 q, q < 4.  Columns are taken four at a time, so 16 loads of a thread
// are in flight before the first is used (and no store to T stands between them: T may not be declared restrict against
// itself).  The row sums for y stay in four registers per thread over the 64 columns; the column sum for g is added over the
// thread's four rows, over the wave by data-parallel-primitive moves, and over the four waves through 4 KiB of LDS, always in
// the same order.  x[j] and a0[j] are wave-uniform.
//
// Partials: a tile writes its 1024 row sums to dWork[ct * n + i] and its 64 column sums to dWork[(nct + rt) * n + j]; a second
// small launch adds them in ascending tile order.  No atomics: two calls give the same bits.  Against the 16 n^2 bytes of T the
// partials are written and read once each, 2 * 16 n^2 (1 / BS_TC + 1 / BS_TR) bytes = 3.3 % (kernel section of the
// sweep).  Rows >= n of a column and the padding behind it are neither read nor written.
#include "common.h"

namespace {

constexpr int BS_THREADS = 256;
constexpr int BS_RK = 4;                         // rows per thread
constexpr int BS_TR = BS_THREADS * BS_RK;        // rows per tile
constexpr int BS_TC = 64;                        // columns per tile
constexpr int BS_CG = 4;                         // columns loaded before the first is used
constexpr int BS_FIN = 128;                      // threads of the finishing launch

template <bool UPD, bool HX, bool HW>
__global__ __launch_bounds__(BS_THREADS) void k_broyden_sweep(int64_t n, cplx* T, int64_t ldt, const cplx* __restrict__ u0,
                                                              const cplx* __restrict__ a0, const cplx* __restrict__ x,
                                                              const cplx* __restrict__ w, cplx* __restrict__ ypart,
                                                              cplx* __restrict__ gpart) {
    __shared__ cplx gs[BS_TC][BS_THREADS / 64];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int64_t r0 = (int64_t)blockIdx.x * BS_TR, c0 = (int64_t)blockIdx.y * BS_TC;
    const int nc = n - c0 < BS_TC ? (int)(n - c0) : BS_TC;                  // columns of this tile that exist
    int64_t row[BS_RK];
    bool ok[BS_RK];
    cplx uu[BS_RK], ww[BS_RK], ya[BS_RK];
#pragma unroll
    for (int q = 0; q < BS_RK; ++q) {
        row[q] = r0 + tid + (int64_t)q * BS_THREADS;
        ok[q] = row[q] < n;
        uu[q] = (UPD && ok[q]) ? u0[row[q]] : cmake(0.0, 0.0);
        ww[q] = (HW && ok[q]) ? w[row[q]] : cmake(0.0, 0.0);
        ya[q] = cmake(0.0, 0.0);
    }
    for (int cb = 0; cb < nc; cb += BS_CG) {
        cplx t[BS_CG][BS_RK];
#pragma unroll
        for (int cc = 0; cc < BS_CG; ++cc) {
            const cplx* col = T + (c0 + cb + cc) * ldt;
#pragma unroll
            for (int q = 0; q < BS_RK; ++q) t[cc][q] = (cb + cc < nc && ok[q]) ? col[row[q]] : cmake(0.0, 0.0);
        }
#pragma unroll
        for (int cc = 0; cc < BS_CG; ++cc) {
            if (cb + cc >= nc) break;                                       // uniform over the workgroup
            const int64_t j = c0 + cb + cc;
            if (UPD) {
                const cplx aj = a0[j];
                cplx* col = T + j * ldt;
#pragma unroll
                for (int q = 0; q < BS_RK; ++q)
                    if (ok[q]) {
                        cfma(t[cc][q], uu[q], aj);
                        col[row[q]] = t[cc][q];
                    }
            }
            if (HX) {
                const cplx xj = x[j];
#pragma unroll
                for (int q = 0; q < BS_RK; ++q) cfma(ya[q], t[cc][q], xj);
            }
            if (HW) {
                cplx s = cmake(0.0, 0.0);
#pragma unroll
                for (int q = 0; q < BS_RK; ++q) cfma_conj(s, ww[q], t[cc][q]);
                s = wave_sum_dpp(s);
                if (lane == 0) gs[cb + cc][wv] = s;
            }
        }
    }
    if (HX) {
#pragma unroll
        for (int q = 0; q < BS_RK; ++q)
            if (ok[q]) ypart[(int64_t)blockIdx.y * n + row[q]] = ya[q];
    }
    if (HW) {
        __syncthreads();
        if (tid < nc) {
            const cplx s = cadd(cadd(cadd(gs[tid][0], gs[tid][1]), gs[tid][2]), gs[tid][3]);
            gpart[(int64_t)blockIdx.x * n + c0 + tid] = s;
        }
    }
}

// y[i] = sum over the column tiles, g[i] = sum over the row tiles, in ascending tile order
__global__ __launch_bounds__(BS_FIN) void k_broyden_finish(int64_t n, int nct, int nrt, const cplx* __restrict__ ypart,
                                                           const cplx* __restrict__ gpart, cplx* __restrict__ y,
                                                           cplx* __restrict__ g) {
    const int64_t i = (int64_t)blockIdx.x * BS_FIN + threadIdx.x;
    if (i >= n) return;
    if (y) {
        cplx s = cmake(0.0, 0.0);
#pragma unroll 8
        for (int t = 0; t < nct; ++t) s = cadd(s, ypart[(int64_t)t * n + i]);
        y[i] = s;
    }
    if (g) {
        cplx s = cmake(0.0, 0.0);
#pragma unroll 8
        for (int t = 0; t < nrt; ++t) s = cadd(s, gpart[(int64_t)t * n + i]);
        g[i] = s;
    }
}

inline int64_t bs_nct(int64_t n) { return (n + BS_TC - 1) / BS_TC; }
inline int64_t bs_nrt(int64_t n) { return (n + BS_TR - 1) / BS_TR; }

// [p, p + n) of complex entries as an address range
struct BsRange {
    uintptr_t lo, hi;
};
inline BsRange bs_range(const void* p, int64_t n) { return BsRange{(uintptr_t)p, (uintptr_t)p + (uintptr_t)n * sizeof(cplx)}; }
inline bool bs_disjoint(BsRange a, BsRange b) { return a.hi <= b.lo || b.hi <= a.lo; }

template <bool UPD, bool HX, bool HW>
void bs_launch(dim3 grid, hipStream_t st, int64_t n, cplx* T, int64_t ldt, const cplx* u0, const cplx* a0, const cplx* x,
               const cplx* w, cplx* ypart, cplx* gpart) {
    hipLaunchKernelGGL((k_broyden_sweep<UPD, HX, HW>), grid, dim3(BS_THREADS), 0, st, n, T, ldt, u0, a0, x, w, ypart, gpart);
}

}  // namespace

int64_t nep_broyden_sweep_worksize(int64_t n) { return n < 1 ? 0 : n * (bs_nct(n) + bs_nrt(n)); }

int32_t nep_broyden_sweep(int64_t n, nep_cdouble* dT, int64_t ldt, const nep_cdouble* du0, const nep_cdouble* da0,
                          const nep_cdouble* dx, nep_cdouble* dy, const nep_cdouble* dw, nep_cdouble* dg, nep_cdouble* dWork,
                          nep_stream stream) {
    ARGCHK(n >= 1 && ldt >= n);
    ARGCHK(dT && dWork);
    ARGCHK(!du0 == !da0 && !dx == !dy && !dw == !dg);
    ARGCHK(du0 || dx || dw);
    const int64_t nct = bs_nct(n), nrt = bs_nrt(n);
    ARGCHK(nct <= 65535 && nrt <= 0x7fffffff);
    const BsRange rT = bs_range(dT, ldt * (n - 1) + n), rW = bs_range(dWork, n * (nct + nrt));
    ARGCHK(bs_disjoint(rT, rW));
    for (const nep_cdouble* out : {(const nep_cdouble*)dy, (const nep_cdouble*)dg}) {
        if (!out) continue;
        const BsRange ro = bs_range(out, n);
        ARGCHK(bs_disjoint(ro, rT) && bs_disjoint(ro, rW));
        for (const nep_cdouble* in : {du0, da0, dx, dw}) ARGCHK(!in || bs_disjoint(ro, bs_range(in, n)));
    }
    ARGCHK(!dy || !dg || bs_disjoint(bs_range(dy, n), bs_range(dg, n)));
    const dim3 grid((unsigned)nrt, (unsigned)nct);
    hipStream_t st = as_stream(stream);
    cplx* T = (cplx*)dT;
    const cplx *u0 = (const cplx*)du0, *a0 = (const cplx*)da0, *x = (const cplx*)dx, *w = (const cplx*)dw;
    cplx* ypart = (cplx*)dWork;
    cplx* gpart = ypart + n * nct;
    const int sel = (du0 ? 4 : 0) | (dx ? 2 : 0) | (dw ? 1 : 0);
    switch (sel) {
        case 1: bs_launch<false, false, true>(grid, st, n, T, ldt, u0, a0, x, w, ypart, gpart); break;
        case 2: bs_launch<false, true, false>(grid, st, n, T, ldt, u0, a0, x, w, ypart, gpart); break;
        case 3: bs_launch<false, true, true>(grid, st, n, T, ldt, u0, a0, x, w, ypart, gpart); break;
        case 4: bs_launch<true, false, false>(grid, st, n, T, ldt, u0, a0, x, w, ypart, gpart); break;
        case 5: bs_launch<true, false, true>(grid, st, n, T, ldt, u0, a0, x, w, ypart, gpart); break;
        case 6: bs_launch<true, true, false>(grid, st, n, T, ldt, u0, a0, x, w, ypart, gpart); break;
        default: bs_launch<true, true, true>(grid, st, n, T, ldt, u0, a0, x, w, ypart, gpart); break;
    }
    LAUNCHCHK();
    if (dx || dw) {
        hipLaunchKernelGGL(k_broyden_finish, dim3((unsigned)((n + BS_FIN - 1) / BS_FIN)), dim3(BS_FIN), 0, st, n, (int)nct,
                           (int)nrt, (const cplx*)ypart, (const cplx*)gpart, (cplx*)dy, (cplx*)dg);
        LAUNCHCHK();
    }
    return NEP_OK;
}
