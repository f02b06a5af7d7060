// libnepmi355: interpolation coefficients of a sampled matrix function, entry by entry, for gfx950.
//
//   C[r(e), i] = beta C[r(e), i] + sum_{j < J} W[i, j] F[e, j],      e < E, i < K,      r(e) = pos ? pos[e] : e
//
// F holds, for each of E matrix entries, J contiguous values (the samples of that entry at J nodes, or its J term values on the
// union pattern of an SPMF: the block D of aligned_terms_dev), W is a small K x J table (Chebyshev weights, an inverse Vandermonde
// matrix, or either of them times the function values of the terms) and C receives the K coefficients of every entry, again
// contiguous per entry.  This is the whole arithmetic of ChebPEP and interpolate.
//
// One launch.  A workgroup of 256 threads owns a tile of TE = g R consecutive entries.  It first copies W (J K values) and the
// tile of F into LDS: the tile is read with consecutive lanes on consecutive values of a row and row after row, so with ldf = J
// the workgroup streams one contiguous block, 16 B (complex) or 8 B (real) per lane; every value of F is read from memory once.
// Then thread (ei, i), ei < g, i < K, forms output i of the entries ei, ei + g, ..., ei + (R - 1) g: lanes run along i first, so a
// wave stores contiguous runs of K values (a whole contiguous block when ldc = K and there is no map), and for beta = 1 it reads
// the same addresses.  In LDS the lanes of one entry read the same F value (a broadcast) and consecutive W values (Ws[j K + i]);
// the rows of the F tile have an odd stride, so that the lanes of different entries fall on different banks when K is small.
// Four entries share one read of W.  The sum runs over j = 0, 1, ..., J - 1 from the old value (beta = 1) or from zero: no
// atomics, no reduction across lanes, two calls give the same bits.  With beta = 0 C is never read.  Entries >= E, the padding of
// F (ldf > J) and of C (ldc > K) and rows of C that the map does not name are neither read nor written.
#include "common.h"

namespace {

constexpr int IP_THREADS = 256;
constexpr int IP_MAXJK = 64;
constexpr int IP_TILE_VALUES = 2048;           // values of F per tile (32 KiB complex, 16 KiB real)
constexpr int IP_MAXR = 8;                     // entries per thread
constexpr int IP_UNROLL = 4;                   // entries that share one read of W
constexpr int IP_BATCH = 8;                    // loads per thread in flight while a tile is copied to LDS

__device__ __forceinline__ void ip_fma(cplx& acc, cplx w, cplx f) { cfma(acc, w, f); }
__device__ __forceinline__ void ip_fma(cplx& acc, cplx w, double f) { cfma(acc, f, w); }

struct IpShape {
    int g, R;                                  // entry groups per workgroup, entries per thread; the tile has g R entries
    size_t lds;
};

// the same arithmetic on the host (launch) and nowhere else: g K <= 256 threads are active, the F tile holds at most
// IP_TILE_VALUES values with rows of stride J | 1
inline IpShape ip_shape(int J, int K, size_t fbytes) {
    IpShape s;
    const int cap = IP_TILE_VALUES / (J | 1) > 0 ? IP_TILE_VALUES / (J | 1) : 1;      // entries whose rows fit the tile
    s.g = IP_THREADS / K < cap ? IP_THREADS / K : cap;
    s.R = cap / s.g < IP_MAXR ? cap / s.g : IP_MAXR;
    if (s.R < 1) s.R = 1;
    size_t fb = (size_t)s.g * s.R * (J | 1) * fbytes;
    fb = (fb + 15) & ~(size_t)15;
    s.lds = (size_t)J * K * sizeof(cplx) + fb;
    return s;
}

template <typename FT>
__global__ __launch_bounds__(IP_THREADS) void k_interp_coeffs(int64_t E, int J, int K, int g, int R, const FT* __restrict__ F,
                                                              int64_t ldf, const cplx* __restrict__ W,
                                                              const int32_t* __restrict__ pos, int beta, cplx* C, int64_t ldc) {
    extern __shared__ __attribute__((aligned(16))) char ip_smem[];
    cplx* Ws = (cplx*)ip_smem;                                   // Ws[j K + i] = W[i, j]: the table as it was uploaded
    FT* Fs = (FT*)(ip_smem + (size_t)J * K * sizeof(cplx));      // Fs[e lds_f + j] = F[e0 + e, j]
    const int lds_f = J | 1;
    const int tid = threadIdx.x;
    const int TE = g * R;
    const int64_t e0 = (int64_t)blockIdx.x * TE;
    const int nE = E - e0 < TE ? (int)(E - e0) : TE;             // >= 1: the grid has ceil(E / TE) workgroups
    // both copies in batches of IP_BATCH loads per thread that are issued before the first of them is waited for: one load per
    // pass would pay the memory latency once per pass (a full tile is exactly one batch)
    const int nW = J * K, nV = nE * J;
    const FT* Ft = F + e0 * ldf;
    for (int t0 = tid; t0 < nV; t0 += IP_BATCH * IP_THREADS) {
        FT v[IP_BATCH];
        int at[IP_BATCH];
#pragma unroll
        for (int u = 0; u < IP_BATCH; ++u) {                     // (past the end: the last value again, loaded and dropped)
            const int t = t0 + u * IP_THREADS < nV ? t0 + u * IP_THREADS : nV - 1;
            const int e = t / J, j = t - e * J;
            v[u] = Ft[(int64_t)e * ldf + j];
            at[u] = e * lds_f + j;
        }
#pragma unroll
        for (int u = 0; u < IP_BATCH; ++u)
            if (t0 + u * IP_THREADS < nV) Fs[at[u]] = v[u];
    }
    for (int t0 = tid; t0 < nW; t0 += IP_BATCH * IP_THREADS) {
        cplx v[IP_BATCH];
#pragma unroll
        for (int u = 0; u < IP_BATCH; ++u) v[u] = W[t0 + u * IP_THREADS < nW ? t0 + u * IP_THREADS : nW - 1];
#pragma unroll
        for (int u = 0; u < IP_BATCH; ++u)
            if (t0 + u * IP_THREADS < nW) Ws[t0 + u * IP_THREADS] = v[u];
    }
    __syncthreads();
    if (tid >= g * K) return;
    const int ei = tid / K, i = tid - ei * K;
    const cplx* Wi = Ws + i;
    for (int r0 = 0; r0 < R; r0 += IP_UNROLL) {
        if (ei + g * r0 >= nE) break;
        cplx acc[IP_UNROLL];
        cplx* dst[IP_UNROLL];
        const FT* src[IP_UNROLL];
#pragma unroll
        for (int u = 0; u < IP_UNROLL; ++u) {
            const int e = ei + g * (r0 + u);
            const bool live = r0 + u < R && e < nE;
            const int er = live ? e : ei;                        // a dead slot reads entry ei again and stores nothing
            src[u] = Fs + er * lds_f;
            dst[u] = nullptr;
            acc[u] = cmake(0.0, 0.0);
            if (live) {
                const int64_t row = pos ? (int64_t)pos[e0 + e] : e0 + e;
                dst[u] = C + row * ldc + i;
                if (beta) acc[u] = *dst[u];
            }
        }
        for (int j = 0; j < J; ++j) {
            const cplx w = Wi[j * K];
#pragma unroll
            for (int u = 0; u < IP_UNROLL; ++u) ip_fma(acc[u], w, src[u][j]);
        }
#pragma unroll
        for (int u = 0; u < IP_UNROLL; ++u)
            if (dst[u]) *dst[u] = acc[u];
    }
}

thread_local NepTableSlots g_interp_tables;
thread_local PinnedRing g_interp_ring;

template <typename FT>
int launch_interp(int64_t E, int J, int K, const void* dF, int64_t ldf, const cplx* dW, const int32_t* dpos, int beta, cplx* dC,
                  int64_t ldc, hipStream_t st) {
    const IpShape s = ip_shape(J, K, sizeof(FT));
    if (s.lds > 64 * 1024) {
        const int rc = nep_raise_lds((const void*)k_interp_coeffs<FT>, 160 * 1024);
        if (rc) return rc;
    }
    const int64_t TE = (int64_t)s.g * s.R;
    const int64_t nblk = (E + TE - 1) / TE;
    ARGCHK(nblk <= 0x7fffffffLL);
    hipLaunchKernelGGL((k_interp_coeffs<FT>), dim3((unsigned)nblk), dim3(IP_THREADS), s.lds, st, E, J, K, s.g, s.R, (const FT*)dF,
                       ldf, dW, dpos, beta, dC, ldc);
    LAUNCHCHK();
    return NEP_OK;
}

}  // namespace

int32_t nep_interp_coeffs(int64_t E, int32_t J, int32_t K, const void* dF, int64_t ldf, int32_t f_is_complex,
                          const nep_cdouble* hW, const int32_t* dpos, int32_t beta, nep_cdouble* dC, int64_t ldc,
                          nep_stream stream) {
    if (J < 1 || J > IP_MAXJK || K < 1 || K > IP_MAXJK) {
        nep_set_error("nep_interp_coeffs: J = %d, K = %d (1 <= J, K <= %d)", J, K, IP_MAXJK);
        return NEP_ERR_UNSUPPORTED;
    }
    ARGCHK(E >= 0 && ldf >= J && ldc >= K);
    ARGCHK(beta == 0 || beta == 1);
    ARGCHK(hW);
    if (E == 0) return NEP_OK;
    ARGCHK(dF && dC);
    if (!dpos) {   // without a map the rows of C are known: C must not overlap F
        const uintptr_t f0 = (uintptr_t)dF, f1 = f0 + ((uintptr_t)(E - 1) * ldf + J) * (f_is_complex ? sizeof(cplx) : sizeof(double));
        const uintptr_t c0 = (uintptr_t)dC, c1 = c0 + ((uintptr_t)(E - 1) * ldc + K) * sizeof(cplx);
        ARGCHK(f1 <= c0 || c1 <= f0);
    }
    hipStream_t st = as_stream(stream);
    void* dslot = nullptr;
    int which = 0;
    int rc = g_interp_tables.acquire((size_t)IP_MAXJK * IP_MAXJK * sizeof(cplx), &dslot, &which);
    if (rc) return rc;
    rc = g_interp_ring.upload(dslot, hW, (size_t)J * K * sizeof(cplx), st);
    if (rc) return rc;
    if (f_is_complex)
        rc = launch_interp<cplx>(E, J, K, dF, ldf, (const cplx*)dslot, dpos, beta, (cplx*)dC, ldc, st);
    else
        rc = launch_interp<double>(E, J, K, dF, ldf, (const cplx*)dslot, dpos, beta, (cplx*)dC, ldc, st);
    if (rc) return rc;
    return g_interp_tables.guard(which, st);
}
