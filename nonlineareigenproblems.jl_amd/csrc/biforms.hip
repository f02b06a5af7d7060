// libnepmi355: K14, the unsummed per-term bilinear forms of an SPMF, for gfx950.
//
//   out[i + kw (j + kv t)] = w_i^H A_t v_j          i < kw, j < kv, t < mt
//
// The Rayleigh functional of an SPMF (y^H M(lam) x = sum_t f_t(lam) y^H A_t x), the reference's `dot(y, A[i]*x)` loop
// (src/compute_rf_wrapper.jl:115-118) and a projected NEP W^H A_t V all need these numbers.  Composed from the existing
// primitives they are one one-hot nep_mlincomb and one dot / GEMM per term: mt passes over the stacked CSR, 2 mt launches.
// K11 walks the stacked CSR the same way but only returns the Hankel-weighted sum.
//
// k_biforms: lane <-> row, one wave (64 rows) per workgroup, grid-stride over the row tiles; blockIdx.y picks a chunk of JC
// columns of V.  A lane walks its row once and keeps acc[t][jj] += val V[col, j0 + jj] for EVERY term of the handle: the
// term of an entry is only known at run time (idx[e] >> NEP_TERM_SHIFT), and a run-time index cannot address the register
// file, so the mt JC accumulators of a lane live in LDS, laid out [slot][lane] with 65 words of 16 bytes per slot: the lanes
// of the walk touch consecutive words (no bank conflict), nobody but the lane itself touches its column.  Four entries per
// trip: their index / value loads are issued together and their gathers together, as in k_blockprod.
//
// Chunking: JC is the largest column count with mt JC <= 32 accumulators per lane (33 KiB of LDS per wave: four waves per
// CU stay resident and hide the gather latency; more accumulators per lane would trade that away for fewer passes).  So
// the stacked CSR is read ONCE for all terms whenever mt kv <= 32, and ceil(kv / JC) times beyond.  With mt > 32 a pass
// takes one column and all mt <= 128 terms (130 KiB of the CU's 160 KiB): kw = kv = 1 is one pass for every handle.
//
// Finish of a row tile: out[i, c] += sum_r conj(W[r, i]) acc[c][r].  Lanes <-> (16 outputs) x (4 row phases r = 4 q + p); the
// four phase sums are added by a fixed xor tree and the phase-0 lane adds the tile's value to the workgroup's own partial
// (plain read-modify-write of memory no other workgroup touches; the first tile writes).  No intermediate of size n x kv
// exists anywhere.  k_biforms_sum adds the per-workgroup partials of an output in a fixed order (as k_lr_sum).  No
// floating-point atomics: two calls on equal inputs give the same bits.  Rows >= n are never read.
#include "common.h"

namespace {

constexpr int BF_ROWS = 64;          // rows per tile (one wave, lane = row)
constexpr int BF_LDA = 65;           // words per accumulator slot (one of padding: the finish reads slots side by side)
constexpr int BF_MAXWV = 32;         // kw, kv limit
constexpr int BF_MAXOUT = 3072;      // mt kw kv limit (the budget nep_spmf_blockprod states)
constexpr int BF_ACC = 32;           // accumulators per lane and pass (unless mt alone is larger)
constexpr int BF_MAXBLOCKS = 8192;
constexpr int64_t BF_MAXPART = 1 << 20;   // complex words of partials (16 MiB)

template <typename VT>
__global__ __launch_bounds__(BF_ROWS) void k_biforms(const int32_t* __restrict__ rowptr, const uint32_t* __restrict__ idx,
                                                     const VT* __restrict__ vals, int64_t n, int mt, int kw, int kv, int JC,
                                                     const cplx* __restrict__ W, int64_t ldw, const cplx* __restrict__ V,
                                                     int64_t ldv, cplx* __restrict__ partial) {
    extern __shared__ cplx accs[];                     // accs[(t jc + jj) BF_LDA + lane]
    const int lane = threadIdx.x;
    const int j0 = blockIdx.y * JC;
    const int jc = kv - j0 < JC ? kv - j0 : JC;
    const int C = mt * jc;
    const int NOc = kw * C;                            // outputs of this chunk
    const int no = kw * kv * mt;
    cplx* mypart = partial + (int64_t)blockIdx.x * no;
    const int64_t ntile = (n + BF_ROWS - 1) / BF_ROWS;
    for (int64_t tile = blockIdx.x; tile < ntile; tile += gridDim.x) {
        const int64_t row0 = tile * BF_ROWS;
        const int64_t r = row0 + lane;
        for (int c = 0; c < C; ++c) accs[c * BF_LDA + lane] = cmake(0.0, 0.0);
        if (r < n) {
            const int e1 = rowptr[r + 1];
            for (int e = rowptr[r]; e < e1; e += 4) {
                uint32_t id[4]; VT v[4];
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const int ee = e + u < e1 ? e + u : e;
                    id[u] = idx[ee]; v[u] = vals[ee];
                }
                for (int jj = 0; jj < jc; ++jj) {
                    cplx x[4];
#pragma unroll
                    for (int u = 0; u < 4; ++u) x[u] = V[(int64_t)(id[u] & NEP_COL_MASK) + (int64_t)(j0 + jj) * ldv];
#pragma unroll
                    for (int u = 0; u < 4; ++u)
                        if (e + u < e1) {
                            cplx* ap = accs + ((int)(id[u] >> NEP_TERM_SHIFT) * jc + jj) * BF_LDA + lane;
                            cplx a = *ap;
                            cfma(a, v[u], x[u]);
                            *ap = a;
                        }
                }
            }
        }
        __syncthreads();
        // ---- the tile's contribution to the outputs of this chunk
        const int ph = lane >> 4;
        for (int o0 = 0; o0 < NOc; o0 += 16) {
            const int o = o0 + (lane & 15);
            cplx s = cmake(0.0, 0.0);
            int i = 0, c = 0;
            if (o < NOc) {
                i = o % kw; c = o / kw;
                const cplx* wp = W + (int64_t)i * ldw + row0;
                const cplx* ap = accs + c * BF_LDA;
                for (int rr = ph; rr < BF_ROWS; rr += 4)
                    if (row0 + rr < n) cfma_conj(s, wp[rr], ap[rr]);
            }
            s.x += shfl_xor_d(s.x, 16); s.y += shfl_xor_d(s.y, 16);
            s.x += shfl_xor_d(s.x, 32); s.y += shfl_xor_d(s.y, 32);
            if (ph == 0 && o < NOc) {
                const int t = c / jc, jj = c - t * jc;
                cplx* pp = mypart + i + kw * ((j0 + jj) + kv * t);
                *pp = tile == (int64_t)blockIdx.x ? s : cadd(*pp, s);
            }
        }
        __syncthreads();                               // the next tile clears the accumulators
    }
}

// out[o] = sum_b partial[b no + o]: one workgroup per output, strided per-lane sums, then the fixed wave / LDS tree
__global__ __launch_bounds__(256) void k_biforms_sum(int nb, int no, const cplx* __restrict__ partial, cplx* __restrict__ out) {
    __shared__ cplx sm[4];
    const int o = blockIdx.x;
    cplx s = cmake(0.0, 0.0);
    for (int b = threadIdx.x; b < nb; b += 256) s = cadd(s, partial[(int64_t)b * no + o]);
    s = wave_sum_dpp(s);
    if ((threadIdx.x & 63) == 0) sm[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) out[o] = cadd(cadd(sm[0], sm[1]), cadd(sm[2], sm[3]));
}

template <typename VT>
int launch_biforms(const NepSpmfView& v, int kw, int kv, int JC, int nb, const cplx* W, int64_t ldw, const cplx* V, int64_t ldv,
                   cplx* partial, cplx* out, hipStream_t st) {
    const int no = v.mt * kw * kv;
    const size_t lds = (size_t)v.mt * JC * BF_LDA * sizeof(cplx);
    if (lds > 64 * 1024) {
        const int rc = nep_raise_lds((const void*)k_biforms<VT>, 160 * 1024);
        if (rc) return rc;
    }
    hipLaunchKernelGGL((k_biforms<VT>), dim3((unsigned)nb, (unsigned)((kv + JC - 1) / JC)), dim3(BF_ROWS), lds, st, v.rowptr, v.idx,
                       (const VT*)v.vals, v.n, (int)v.mt, kw, kv, JC, W, ldw, V, ldv, partial);
    LAUNCHCHK();
    hipLaunchKernelGGL(k_biforms_sum, dim3((unsigned)no), dim3(256), 0, st, nb, no, (const cplx*)partial, out);
    LAUNCHCHK();
    return NEP_OK;
}

}  // namespace

int32_t nep_spmf_biforms(nep_spmf* s, int32_t kw, const nep_cdouble* dW, int64_t ldw, int32_t kv, const nep_cdouble* dV,
                         int64_t ldv, nep_cdouble* h_out, nep_cdouble* d_out, nep_stream stream) {
    ARGCHK(s && dW && dV && (h_out || d_out));
    NepSpmfView v;
    int rc = nep_spmf_csr_view(s, &v);
    if (rc) return rc;
    if (kw < 1 || kw > BF_MAXWV || kv < 1 || kv > BF_MAXWV || (int64_t)v.mt * kw * kv > BF_MAXOUT) {
        nep_set_error("nep_spmf_biforms: kw = %d, kv = %d, mt = %d (1 <= kw, kv <= %d, mt kw kv <= %d)", kw, kv, (int)v.mt,
                      BF_MAXWV, BF_MAXOUT);
        return NEP_ERR_UNSUPPORTED;
    }
    ARGCHK(ldw >= v.n && ldv >= v.n);
    hipStream_t st = as_stream(stream);
    const int no = v.mt * kw * kv;
    int JC = BF_ACC / v.mt;
    if (JC < 1) JC = 1;
    if (JC > kv) JC = kv;
    const int64_t ntile = (v.n + BF_ROWS - 1) / BF_ROWS;
    int64_t nb = BF_MAXPART / no;
    if (nb > BF_MAXBLOCKS) nb = BF_MAXBLOCKS;
    if (nb > ntile) nb = ntile;
    if (nb < 1) nb = 1;
    rc = v.scratch->ensure((size_t)(nb + 1) * no * sizeof(cplx));
    if (rc) return rc;
    cplx* partial = (cplx*)v.scratch->dptr;
    cplx* out = d_out ? (cplx*)d_out : partial + nb * no;
    if (v.valbytes == 16)
        rc = launch_biforms<cplx>(v, kw, kv, JC, (int)nb, (const cplx*)dW, ldw, (const cplx*)dV, ldv, partial, out, st);
    else
        rc = launch_biforms<double>(v, kw, kv, JC, (int)nb, (const cplx*)dW, ldw, (const cplx*)dV, ldv, partial, out, st);
    if (rc) return rc;
    if (h_out) {
        HIPCHK(hipMemcpyAsync(h_out, out, (size_t)no * sizeof(cplx), hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
    }
    return NEP_OK;
}
