// libnepmi355: the expansion step of compute_Mlincomb on a deflated NEP (Effenberger deflation), for gfx950.
//
// With X = V0 (n0 x p), V = [V1; V2] (k columns of n0 + p rows), s = startder, K = k + s and e_i = i + s:
//
//   C[:, j]  = sum_{i >= max(0, j - s)} G[i, j] * (W_{e_i - j} V2[:, i])                  (p x K, the small block)
//   Vn[:, j] = [j >= s] a_{j-s} V1[:, j-s] + X C[:, j],   j = 0..K-1                       (n0 x K)
//   zb       = a_0 X^H V1[:, 0]   (s == 0),   0   (s > 0)                                  (p)
//
// The tables a, G, W are the caller's (they hold the powers of (lam I - S0)^-1 and the binomial factors): the kernels know
// nothing of lam or S0.  The reference forms Z = Xhat * Vnew term by term on the host (nep_deflation.jl:65-107).
//
// k_defl_expand: one thread per row with a grid-stride loop.  C lives in LDS: every workgroup forms it itself when K <= 8
// (at most 256 entries, one per thread, each the same fixed-order sum -- a launch saved on the path a Newton step takes), and
// loads it from k_defl_C's result otherwise.  A row accumulates 8 columns of Vn at a time in registers while it walks its p
// entries of X once per 8 columns (lanes of a wave read consecutive addresses of the column-major X; C is an LDS broadcast).
// The p dot products of zb are per-workgroup partials (DPP wave sums, then the four waves through LDS) that k_defl_zb adds
// in a fixed order.  No atomics: two calls give the same bits.
#include "common.h"
#include <vector>

namespace {

constexpr int DF_THREADS = 256;
constexpr int DF_MAXP = 32;
constexpr int DF_MAXK = 64;
constexpr int DF_FORMK = 8;          // K <= DF_FORMK: the expand kernel forms C itself
constexpr int DF_JC = 8;             // columns of Vn a row holds in registers
constexpr int DF_MAXBLOCKS = 2048;   // grid cap of the streaming pass; rows beyond it are reached by the grid stride

// C[q, j] for one (q, j): i ascending, the inner product over l ascending
__device__ __forceinline__ cplx defl_C_entry(int q, int j, int p, int k, int s, const cplx* __restrict__ V2, int64_t ldv,
                                             const cplx* __restrict__ G, const cplx* __restrict__ W) {
    cplx acc = cmake(0.0, 0.0);
    for (int i = j > s ? j - s : 0; i < k; ++i) {
        const cplx* w = W + (int64_t)(i + s - j) * p * p + q;
        const cplx* v = V2 + (int64_t)i * ldv;
        cplx t = cmake(0.0, 0.0);
        for (int l = 0; l < p; ++l) cfma(t, w[(int64_t)l * p], v[l]);
        cfma(acc, G[i + (int64_t)j * k], t);
    }
    return acc;
}

__global__ __launch_bounds__(DF_THREADS) void k_defl_C(int p, int k, int s, const cplx* __restrict__ V2, int64_t ldv,
                                                       const cplx* __restrict__ G, const cplx* __restrict__ W,
                                                       cplx* __restrict__ Cout) {
    const int e = blockIdx.x * DF_THREADS + threadIdx.x;
    if (e < p * (k + s)) Cout[e] = defl_C_entry(e % p, e / p, p, k, s, V2, ldv, G, W);
}

template <bool FORM>
__global__ __launch_bounds__(DF_THREADS) void k_defl_expand(int64_t n0, int p, int k, int s, const cplx* __restrict__ X,
                                                            int64_t ldx, const cplx* __restrict__ V, int64_t ldv,
                                                            const cplx* __restrict__ a, const cplx* __restrict__ G,
                                                            const cplx* __restrict__ W, const cplx* __restrict__ Cin,
                                                            cplx* __restrict__ Vn, int64_t ldo, cplx* __restrict__ partial,
                                                            cplx* __restrict__ zb) {
    __shared__ cplx Cs[DF_MAXP * (FORM ? DF_FORMK : DF_MAXK)];
    __shared__ cplx red[DF_MAXP][DF_THREADS / 64];
    const int K = k + s;
    const int nC = p * K;
    for (int e = threadIdx.x; e < nC; e += DF_THREADS)
        Cs[e] = FORM ? defl_C_entry(e % p, e / p, p, k, s, V + n0, ldv, G, W) : Cin[e];
    __syncthreads();
    const int64_t stride = (int64_t)gridDim.x * DF_THREADS;
    const int64_t r0 = (int64_t)blockIdx.x * DF_THREADS + threadIdx.x;
    for (int64_t r = r0; r < n0; r += stride) {
        for (int j0 = 0; j0 < K; j0 += DF_JC) {
            cplx acc[DF_JC];
#pragma unroll
            for (int jj = 0; jj < DF_JC; ++jj) {
                const int j = j0 + jj;
                acc[jj] = (j < K && j >= s) ? cmul(a[j - s], V[r + (int64_t)(j - s) * ldv]) : cmake(0.0, 0.0);
            }
            for (int l = 0; l < p; ++l) {
                const cplx x = X[r + (int64_t)l * ldx];
#pragma unroll
                for (int jj = 0; jj < DF_JC; ++jj)
                    if (j0 + jj < K) cfma(acc[jj], x, Cs[l + (j0 + jj) * p]);
            }
#pragma unroll
            for (int jj = 0; jj < DF_JC; ++jj)
                if (j0 + jj < K) Vn[r + (int64_t)(j0 + jj) * ldo] = acc[jj];
        }
    }
    if (s > 0) {                              // zb = 0: nothing to reduce, no second launch
        if (blockIdx.x == 0 && threadIdx.x < p) zb[threadIdx.x] = cmake(0.0, 0.0);
        return;
    }
    // partial[q * gridDim.x + blockIdx.x] = sum over this workgroup's rows of conj(X[r, q]) V1[r, 0]
    for (int q = 0; q < p; ++q) {
        cplx d = cmake(0.0, 0.0);
        for (int64_t r = r0; r < n0; r += stride) cfma_conj(d, X[r + (int64_t)q * ldx], V[r]);
        d = wave_sum_dpp(d);
        if ((threadIdx.x & 63) == 0) red[q][threadIdx.x >> 6] = d;
    }
    __syncthreads();
    if (threadIdx.x < p) {
        const int q = threadIdx.x;
        partial[(int64_t)q * gridDim.x + blockIdx.x] = cadd(cadd(red[q][0], red[q][1]), cadd(red[q][2], red[q][3]));
    }
}

// zb[q] = a_0 * sum_b partial[q * nb + b]: one workgroup per q, strided per-lane sums, then the fixed wave / LDS tree
__global__ __launch_bounds__(DF_THREADS) void k_defl_zb(int nb, const cplx* __restrict__ partial, const cplx* __restrict__ a,
                                                        cplx* __restrict__ zb) {
    __shared__ cplx sm[DF_THREADS / 64];
    const cplx* pq = partial + (int64_t)blockIdx.x * nb;
    cplx d = cmake(0.0, 0.0);
    for (int b = threadIdx.x; b < nb; b += DF_THREADS) d = cadd(d, pq[b]);
    d = wave_sum_dpp(d);
    if ((threadIdx.x & 63) == 0) sm[threadIdx.x >> 6] = d;
    __syncthreads();
    if (threadIdx.x == 0) zb[blockIdx.x] = cmul(a[0], cadd(cadd(sm[0], sm[1]), cadd(sm[2], sm[3])));
}

thread_local NepScratch g_defl_scratch;
thread_local PinnedRing g_defl_ring;

}  // namespace

int32_t nep_defl_expand(int64_t n0, int32_t p, int32_t k, int32_t s, const nep_cdouble* dX, int64_t ldx,
                        const nep_cdouble* dV, int64_t ldv, const nep_cdouble* hA, const nep_cdouble* hG,
                        const nep_cdouble* hW, nep_cdouble* dVn, int64_t ldo, nep_cdouble* dzb, nep_stream stream) {
    ARGCHK(dX && dV && hA && hG && hW && dVn && dzb);
    ARGCHK(n0 >= 1 && k >= 1 && s >= 0);
    if (p < 1 || p > DF_MAXP || (int64_t)k + s > DF_MAXK) {
        nep_set_error("nep_defl_expand: p = %d, k + s = %lld (1 <= p <= %d, k + s <= %d)", p, (long long)k + s, DF_MAXP, DF_MAXK);
        return NEP_ERR_UNSUPPORTED;
    }
    ARGCHK(ldx >= n0 && ldo >= n0 && ldv >= n0 + p);
    hipStream_t st = as_stream(stream);
    const int K = k + s;
    const int nb = (int)((n0 + DF_THREADS - 1) / DF_THREADS < DF_MAXBLOCKS ? (n0 + DF_THREADS - 1) / DF_THREADS : DF_MAXBLOCKS);
    // device block: [a (k) | G (k K) | W (p p K) | C (p K) | partial (p nb)], the first three uploaded in one copy
    const size_t na = (size_t)k, nG = (size_t)k * K, nW = (size_t)p * p * K, nC = (size_t)p * K;
    int rc = g_defl_scratch.ensure((na + nG + nW + nC + (size_t)p * nb) * sizeof(cplx));
    if (rc) return rc;
    static thread_local std::vector<cplx> stage;
    stage.resize(na + nG + nW);
    memcpy(stage.data(), hA, na * sizeof(cplx));
    memcpy(stage.data() + na, hG, nG * sizeof(cplx));
    memcpy(stage.data() + na + nG, hW, nW * sizeof(cplx));
    cplx* da = (cplx*)g_defl_scratch.dptr;
    cplx *dG = da + na, *dW = dG + nG, *dC = dW + nW, *partial = dC + nC;
    rc = g_defl_ring.upload(da, stage.data(), stage.size() * sizeof(cplx), st);
    if (rc) return rc;
    const cplx *X = (const cplx*)dX, *V = (const cplx*)dV;
    if (K <= DF_FORMK) {
        hipLaunchKernelGGL(k_defl_expand<true>, dim3(nb), dim3(DF_THREADS), 0, st, n0, p, k, s, X, ldx, V, ldv, (const cplx*)da,
                           (const cplx*)dG, (const cplx*)dW, (const cplx*)nullptr, (cplx*)dVn, ldo, partial, (cplx*)dzb);
        LAUNCHCHK();
    } else {
        hipLaunchKernelGGL(k_defl_C, dim3((unsigned)((nC + DF_THREADS - 1) / DF_THREADS)), dim3(DF_THREADS), 0, st, p, k, s,
                           V + n0, ldv, (const cplx*)dG, (const cplx*)dW, dC);
        LAUNCHCHK();
        hipLaunchKernelGGL(k_defl_expand<false>, dim3(nb), dim3(DF_THREADS), 0, st, n0, p, k, s, X, ldx, V, ldv, (const cplx*)da,
                           (const cplx*)dG, (const cplx*)dW, (const cplx*)dC, (cplx*)dVn, ldo, partial, (cplx*)dzb);
        LAUNCHCHK();
    }
    if (s == 0) {
        hipLaunchKernelGGL(k_defl_zb, dim3(p), dim3(DF_THREADS), 0, st, nb, (const cplx*)partial, (const cplx*)da, (cplx*)dzb);
        LAUNCHCHK();
    }
    return NEP_OK;
}
