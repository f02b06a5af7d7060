// libnepmi355: the SPMF block product of the block Newton method (K12), for gfx950.
//
//   Z[:, 0:q] = beta Z[:, 0:q] + alpha sum_{t < mt} A_t (Y G_t)          Y: n x r, G_t: r x q (host tables), Z: n x q
//
// compute_MM is the case G_t = f_t(S) (src/NEPTypes.jl:276-319); the block Newton method also needs the products with the
// off-diagonal blocks of f_t on expanded matrices (src/method_blocknewton.jl:173-179, 201-206), whose tables differ in every
// call.  Composed from the existing primitives such a product is nep_gemm_ts into a row-major n x (mt q) block, nep_spmm_terms
// and a transpose back: three launches and an intermediate of 16 n mt q bytes.  Here it is one launch that never forms it.
//
// k_blockprod: the stacked CSR is walked row by row.  A row belongs to a group of G lanes = EL entry lanes x QL column lanes
// (QL = q rounded up to a power of two, G = 16, or 32 for q > 16; 256 / G rows per workgroup, grid-stride over row groups).
// Lane (es, j) takes the entries e0 + es, e0 + es + EL, ... of its row and, per entry, forms the r-term inner product
// d = Y[col, :] G_t[:, j] (Y gathered from HBM / L2 -- the lanes of one entry lane read the same address, G_t from LDS, stored
// [t][k][j] so that the column lanes read consecutive words) and adds val * d.  Four entries per trip: their index and value
// loads are issued together and their gathers together, as in k_spmv (two dependent round trips per ENTRY otherwise).  The EL
// partial sums of a row are added by a fixed xor tree; lane (0, j) writes alpha * sum (+ beta * Z).  No atomics: two calls on
// equal inputs give the same bits.  Rows without entries write beta * Z (or zero); rows longer than any lane count are just
// more trips of the entry loop.
//
// The tables of a call are staged through the handle's pinned ring into one of eight device slots of the handle; a slot is
// reused only after the kernel that read it has finished (an event behind every launch), so back-to-back calls with different
// tables, on one stream or several, never overwrite a table that is still to be read.
#include "common.h"

namespace {

constexpr int BP_THREADS = 256;
constexpr int BP_MAXRQ = 32;
constexpr int BP_MAXTAB = 3072;        // mt r q <= 3072 complex = 48 KiB of LDS (the budget nep_resid_batch_dev states)
constexpr int BP_MAXBLOCKS = 4096;

template <typename VT, int QL, int G>
__global__ __launch_bounds__(BP_THREADS) void k_blockprod(const int32_t* __restrict__ rowptr, const uint32_t* __restrict__ idx,
                                                          const VT* __restrict__ vals, int64_t n, int mt, int r, int q,
                                                          const cplx* __restrict__ Y, int64_t ldy, const cplx* __restrict__ Gt,
                                                          cplx alpha, cplx beta, int use_beta, cplx* __restrict__ Z, int64_t ldz) {
    extern __shared__ cplx Gs[];                       // Gs[(t r + k) q + j] = G_t[k, j]
    constexpr int EL = G / QL;
    constexpr int RPB = BP_THREADS / G;
    const int rq = r * q, ntab = mt * rq;
    for (int e = threadIdx.x; e < ntab; e += BP_THREADS) {
        const int t = e / rq, rem = e - t * rq, k = rem / q, j = rem - k * q;
        Gs[e] = Gt[(int64_t)t * rq + k + (int64_t)j * r];
    }
    __syncthreads();
    const int sub = threadIdx.x % G;
    const int j = sub % QL, es = sub / QL;
    const int jc = j < q ? j : 0;                      // idle column lanes of a group compute column 0 and write nothing
    for (int64_t row0 = (int64_t)blockIdx.x * RPB; row0 < n; row0 += (int64_t)gridDim.x * RPB) {
        const int64_t row = row0 + threadIdx.x / G;
        cplx acc = cmake(0.0, 0.0);
        if (row < n) {
            const int e0 = rowptr[row], e1 = rowptr[row + 1];
            for (int e = e0 + es; e < e1; e += 4 * EL) {
                uint32_t id[4]; VT v[4]; cplx d[4]; const cplx* yp[4]; const cplx* gp[4];
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const int ee = e + u * EL < e1 ? e + u * EL : e;
                    id[u] = idx[ee]; v[u] = vals[ee];
                }
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    yp[u] = Y + (int64_t)(id[u] & NEP_COL_MASK);
                    gp[u] = Gs + (int)(id[u] >> NEP_TERM_SHIFT) * rq + jc;
                    d[u] = cmake(0.0, 0.0);
                }
                for (int k = 0; k < r; ++k) {
                    cplx y[4];
#pragma unroll
                    for (int u = 0; u < 4; ++u) y[u] = yp[u][(int64_t)k * ldy];
#pragma unroll
                    for (int u = 0; u < 4; ++u) cfma(d[u], y[u], gp[u][k * q]);
                }
#pragma unroll
                for (int u = 0; u < 4; ++u)
                    if (e + u * EL < e1) cfma(acc, v[u], d[u]);
            }
        }
#pragma unroll
        for (int off = G / 2; off >= QL; off >>= 1) {  // the EL partial sums of a row, fixed order
            acc.x += shfl_xor_d(acc.x, off);
            acc.y += shfl_xor_d(acc.y, off);
        }
        if (row < n && es == 0 && j < q) {
            cplx* zp = Z + row + (int64_t)j * ldz;
            cplx z = cmul(alpha, acc);
            if (use_beta) z = cadd(z, cmul(beta, *zp));
            *zp = z;
        }
    }
}

template <typename VT, int QL, int G>
int launch_one(const NepSpmfView& v, int r, int q, const cplx* Y, int64_t ldy, const cplx* Gt, cplx alpha, cplx beta,
               cplx* Z, int64_t ldz, hipStream_t st) {
    constexpr int RPB = BP_THREADS / G;
    const int64_t groups = (v.n + RPB - 1) / RPB;
    const int grid = (int)(groups < BP_MAXBLOCKS ? groups : BP_MAXBLOCKS);
    const size_t lds = (size_t)v.mt * r * q * sizeof(cplx);
    const int use_beta = (beta.x != 0.0 || beta.y != 0.0) ? 1 : 0;
    hipLaunchKernelGGL((k_blockprod<VT, QL, G>), dim3(grid), dim3(BP_THREADS), lds, st, v.rowptr, v.idx, (const VT*)v.vals, v.n,
                       (int)v.mt, r, q, Y, ldy, Gt, alpha, beta, use_beta, Z, ldz);
    LAUNCHCHK();
    return NEP_OK;
}

template <typename VT>
int launch_blockprod(const NepSpmfView& v, int r, int q, const cplx* Y, int64_t ldy, const cplx* Gt, cplx alpha, cplx beta,
                     cplx* Z, int64_t ldz, hipStream_t st) {
    if (q == 1) return launch_one<VT, 1, 16>(v, r, q, Y, ldy, Gt, alpha, beta, Z, ldz, st);
    if (q == 2) return launch_one<VT, 2, 16>(v, r, q, Y, ldy, Gt, alpha, beta, Z, ldz, st);
    if (q <= 4) return launch_one<VT, 4, 16>(v, r, q, Y, ldy, Gt, alpha, beta, Z, ldz, st);
    if (q <= 8) return launch_one<VT, 8, 16>(v, r, q, Y, ldy, Gt, alpha, beta, Z, ldz, st);
    if (q <= 16) return launch_one<VT, 16, 16>(v, r, q, Y, ldy, Gt, alpha, beta, Z, ldz, st);
    return launch_one<VT, 32, 32>(v, r, q, Y, ldy, Gt, alpha, beta, Z, ldz, st);
}

}  // namespace

int NepTableSlots::acquire(size_t slot_bytes, void** dslot, int* which) {
    int rc = dev.ensure(NSLOT * slot_bytes);
    if (rc) return rc;
    const int i = next;
    next = (next + 1) % NSLOT;
    if (!ev[i]) HIPCHK(hipEventCreateWithFlags(&ev[i], hipEventDisableTiming));
    if (used[i]) HIPCHK(hipEventSynchronize(ev[i]));     // the kernel that read this slot has finished
    *dslot = (char*)dev.dptr + (size_t)i * slot_bytes;
    *which = i;
    return NEP_OK;
}
int NepTableSlots::guard(int which, hipStream_t st) {
    HIPCHK(hipEventRecord(ev[which], st));
    used[which] = true;
    return NEP_OK;
}
void NepTableSlots::release() {
    for (int i = 0; i < NSLOT; ++i) {
        if (ev[i] && used[i]) (void)hipEventSynchronize(ev[i]);
        if (ev[i]) (void)hipEventDestroy(ev[i]);
        ev[i] = nullptr; used[i] = false;
    }
    dev.release();
    next = 0;
}

int32_t nep_spmf_blockprod(nep_spmf* s, int32_t r, int32_t q, const nep_cdouble* dY, int64_t ldy, const nep_cdouble* hG,
                           nep_cdouble alpha, nep_cdouble beta, nep_cdouble* dZ, int64_t ldz, nep_stream stream) {
    ARGCHK(s && dY && hG && dZ);
    NepSpmfView v;
    int rc = nep_spmf_csr_view(s, &v);
    if (rc) return rc;
    if (r < 1 || r > BP_MAXRQ || q < 1 || q > BP_MAXRQ || (int64_t)v.mt * r * q > BP_MAXTAB) {
        nep_set_error("nep_spmf_blockprod: r = %d, q = %d, mt = %d (1 <= r, q <= %d, mt r q <= %d)", r, q, (int)v.mt, BP_MAXRQ,
                      BP_MAXTAB);
        return NEP_ERR_UNSUPPORTED;
    }
    ARGCHK(ldy >= v.n && ldz >= v.n);
    {   // Z must not overlap Y (a row of Z is written while other rows still gather Y)
        const uintptr_t y0 = (uintptr_t)dY, y1 = y0 + ((uintptr_t)(r - 1) * ldy + v.n) * sizeof(cplx);
        const uintptr_t z0 = (uintptr_t)dZ, z1 = z0 + ((uintptr_t)(q - 1) * ldz + v.n) * sizeof(cplx);
        ARGCHK(z1 <= y0 || y1 <= z0);
    }
    hipStream_t st = as_stream(stream);
    void* dslot = nullptr;
    int which = 0;
    rc = v.tables->acquire((size_t)BP_MAXTAB * sizeof(cplx), &dslot, &which);
    if (rc) return rc;
    rc = v.ring->upload(dslot, hG, (size_t)v.mt * r * q * sizeof(cplx), st);
    if (rc) return rc;
    const cplx a = {alpha.re, alpha.im}, b = {beta.re, beta.im};
    if (v.valbytes == 8)
        rc = launch_blockprod<double>(v, r, q, (const cplx*)dY, ldy, (const cplx*)dslot, a, b, (cplx*)dZ, ldz, st);
    else
        rc = launch_blockprod<cplx>(v, r, q, (const cplx*)dY, ldy, (const cplx*)dslot, a, b, (cplx*)dZ, ldz, st);
    if (rc) return rc;
    return v.tables->guard(which, st);
}
