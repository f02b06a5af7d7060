// libnepmi355: K11, the left-right scalar product of the infinite bi-Lanczos method, for gfx950.
//
//   c = - sum_t sum_{j<ma} sum_{i<mb} tau_t[i+j+1] w_j^H A_t b_i,     tau_t[d] = f_t^(d)(sigma) / d!
//
// i.e. the entrywise product of W^H A_t B with a Hankel matrix of Taylor coefficients, summed over the terms.  The reference
// forms it with ma calls of compute_Mlincomb (each reading all of B) and ma dot products.  Here, with
// Z_t = conj(W) H_t (H_t[j,i] = tau_t[i+j+1], an n x mb block),
//
//   c = - sum_r sum_{e in row r} val[e] sum_i Z_{term(e)}[r,i] B[col(e), i]
//
// k_lr_hankel: lane <-> row (64 rows per workgroup), one (term, chunk of IC columns of B) per blockIdx.y.  A lane forms its
// row's IC entries of Z_t in registers (it reads W[r, :] -- the lanes of a wave read consecutive addresses of the column-major
// block -- and the Hankel slice of tau_t, staged in LDS and read as a broadcast), then walks the row's entries of term t and
// gathers the IC columns of B at the entry's column.  Neither Z nor A_t B is stored anywhere; one complex partial per
// workgroup.  k_lr_sum adds the partials in a fixed order.  No atomics: two calls give the same bits.
#include "common.h"

namespace {

constexpr int LR_ROWS = 64;   // rows per workgroup (one wave, lane = row)
constexpr int LR_MAX = 256;   // ma, mb limit of the entry point

template <typename VT, int IC>
__global__ __launch_bounds__(LR_ROWS) void k_lr_hankel(const int32_t* __restrict__ rowptr, const uint32_t* __restrict__ idx,
                                                       const VT* __restrict__ vals, int64_t n, int ma, int mb,
                                                       const cplx* __restrict__ W, int64_t ldw, const cplx* __restrict__ B,
                                                       int64_t ldb, const cplx* __restrict__ tau, int64_t ldt, int nch,
                                                       cplx* __restrict__ partial) {
    __shared__ cplx ts[IC + LR_MAX];
    const int t = blockIdx.y / nch;
    const int i0 = (blockIdx.y % nch) * IC;
    // ts[q] = tau_t[i0 + 1 + q], q < IC + ma - 1 (zero past the table: those orders only meet columns i >= mb, never used)
    const int nts = IC + ma - 1;
    for (int q = threadIdx.x; q < nts; q += LR_ROWS) {
        const int d = i0 + 1 + q;
        ts[q] = d < ma + mb ? tau[d + (int64_t)t * ldt] : cmake(0.0, 0.0);
    }
    __syncthreads();
    const int64_t r = (int64_t)blockIdx.x * LR_ROWS + threadIdx.x;
    cplx acc = cmake(0.0, 0.0);
    if (r < n) {
        // z[ii] = sum_j conj(W[r, j]) tau_t[i0 + ii + j + 1]
        cplx z[IC];
#pragma unroll
        for (int ii = 0; ii < IC; ++ii) z[ii] = cmake(0.0, 0.0);
        const cplx* wp = W + r;
        for (int j = 0; j < ma; ++j) {
            const cplx w = wp[(int64_t)j * ldw];
#pragma unroll
            for (int ii = 0; ii < IC; ++ii) cfma_conj(z[ii], w, ts[ii + j]);
        }
        const int e1 = rowptr[r + 1];
        for (int e = rowptr[r]; e < e1; ++e) {
            const uint32_t id = idx[e];
            if ((int)(id >> NEP_TERM_SHIFT) != t) continue;
            const cplx* bp = B + (id & NEP_COL_MASK) + (int64_t)i0 * ldb;
            cplx s = cmake(0.0, 0.0);
#pragma unroll
            for (int ii = 0; ii < IC; ++ii)
                if (i0 + ii < mb) cfma(s, z[ii], bp[(int64_t)ii * ldb]);
            cfma(acc, vals[e], s);
        }
    }
    acc = wave_sum_dpp(acc);
    if (threadIdx.x == 0) partial[(int64_t)blockIdx.y * gridDim.x + blockIdx.x] = acc;
}

// out = -sum_b partial[b]: one workgroup, strided per-lane sums, then the fixed wave / LDS tree
__global__ __launch_bounds__(256) void k_lr_sum(int64_t np, const cplx* __restrict__ partial, cplx* __restrict__ out) {
    __shared__ cplx sm[4];
    cplx s = cmake(0.0, 0.0);
    for (int64_t b = threadIdx.x; b < np; b += 256) s = cadd(s, partial[b]);
    s = wave_sum_dpp(s);
    if ((threadIdx.x & 63) == 0) sm[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        const cplx v = cadd(cadd(sm[0], sm[1]), cadd(sm[2], sm[3]));
        out[0] = cmake(-v.x, -v.y);
    }
}

template <typename VT, int IC>
int launch_lr(const NepSpmfView& v, int ma, int mb, const cplx* W, int64_t ldw, const cplx* B, int64_t ldb, const cplx* tau,
              int64_t ldt, cplx* partial, cplx* out, hipStream_t st) {
    const int nch = (mb + IC - 1) / IC;
    const int64_t nrb = (v.n + LR_ROWS - 1) / LR_ROWS;
    hipLaunchKernelGGL((k_lr_hankel<VT, IC>), dim3((unsigned)nrb, (unsigned)(v.mt * nch)), dim3(LR_ROWS), 0, st, v.rowptr,
                       v.idx, (const VT*)v.vals, v.n, ma, mb, W, ldw, B, ldb, tau, ldt, nch, partial);
    LAUNCHCHK();
    hipLaunchKernelGGL(k_lr_sum, dim3(1), dim3(256), 0, st, nrb * v.mt * nch, (const cplx*)partial, out);
    LAUNCHCHK();
    return NEP_OK;
}

}  // namespace

int32_t nep_lr_hankel(nep_spmf* s, int32_t ma, int32_t mb, const nep_cdouble* dW, int64_t ldw, const nep_cdouble* dB,
                      int64_t ldb, const nep_cdouble* dTau, int64_t ldt, nep_cdouble* h_c, nep_cdouble* d_c,
                      nep_stream stream) {
    NepSpmfView v;
    int rc = nep_spmf_csr_view(s, &v);
    if (rc) return rc;
    ARGCHK(ma >= 1 && mb >= 1 && dW && dB && dTau && (h_c || d_c));
    if (ma > LR_MAX || mb > LR_MAX) {
        nep_set_error("nep_lr_hankel: ma = %d, mb = %d (at most %d each)", ma, mb, LR_MAX);
        return NEP_ERR_UNSUPPORTED;
    }
    ARGCHK(ldw >= v.n && ldb >= v.n && ldt >= (int64_t)ma + mb);
    hipStream_t st = as_stream(stream);
    const int IC = mb <= 8 ? 8 : 16;
    const int64_t np = (v.n + LR_ROWS - 1) / LR_ROWS * v.mt * ((mb + IC - 1) / IC);
    rc = v.scratch->ensure((size_t)(np + 1) * sizeof(cplx));
    if (rc) return rc;
    cplx* partial = (cplx*)v.scratch->dptr;
    cplx* out = d_c ? (cplx*)d_c : partial + np;
    const cplx *W = (const cplx*)dW, *B = (const cplx*)dB, *tau = (const cplx*)dTau;
    if (v.valbytes == 16)
        rc = IC == 8 ? launch_lr<cplx, 8>(v, ma, mb, W, ldw, B, ldb, tau, ldt, partial, out, st)
                     : launch_lr<cplx, 16>(v, ma, mb, W, ldw, B, ldb, tau, ldt, partial, out, st);
    else
        rc = IC == 8 ? launch_lr<double, 8>(v, ma, mb, W, ldw, B, ldb, tau, ldt, partial, out, st)
                     : launch_lr<double, 16>(v, ma, mb, W, ldw, B, ldb, tau, ldt, partial, out, st);
    if (rc) return rc;
    if (h_c) {
        HIPCHK(hipMemcpyAsync(h_c, out, sizeof(cplx), hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
    }
    return NEP_OK;
}
