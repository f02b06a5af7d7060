// libnepmi355: the device pieces of a shift-and-invert Krylov-Schur eigensolver for a linear pencil A x = d B x, for gfx950.
//
// K13 nep_basis_rotate: V[:, 0:p] <- V[:, 0:m] Q in place (the compression of a Krylov-Schur restart), no second basis.
//
//   A workgroup of 256 threads owns a tile of 64 rows.  It first stages ALL m entries of each of its rows in LDS
//   (tile[k][row], 64 m 16 bytes: 20 KiB at m = 20, 128 KiB at the limit m = 128 -- one workgroup per CU there, of 160 KiB),
//   waits, and only then writes its rows of the columns 0 .. p - 1: every output column is formed from the ORIGINAL columns, and
//   row tiles are disjoint, so no workgroup reads what another one writes.  Lane = row (a wave reads and writes 1 KiB runs of a
//   column), the output columns are dealt to the four waves in turn (wave w forms the columns w, w + 4, w + 8, ...: p = 10 is
//   3 + 3 + 2 + 2), up to four per pass over the tile; a tile entry is read from LDS once per pass (ds_read_b128,
//   conflict-free) and the entries of Q are wave-uniform loads of a row-major copy of the table.  Sums run over k ascending in
//   every lane: two calls give the same bits.  The carry column v_{m+1} is read before the tile is written and stored to column
//   p afterwards (p == m: it is where it belongs already).  At the sizes of a restart (m = 20, p = 10) the operation is bound
//   by its bytes, 16 rows (m + p): 8 m p / (16 (m + p)) = 3.3 flop per byte, about a quarter of the FP64 vector rate at the HBM
//   rate.  That ratio grows like m p / (m + p): at (128, 64) and (128, 128) it is 21 and 32 flop per byte and the kernel is bound
//   by its vector FMAs (and runs one workgroup per CU); the FP64 matrix cores would be the tool for such shapes -- not built,
//   no driver here restarts at that size.
//
//   The table is copied (transposed to row-major, compact) into the calling thread's pinned ring and from there into one of
//   eight device slots; a slot is handed out again only when the kernel that read it has finished (NepTableSlots, as
//   nep_spmf_blockprod does), so the caller may free or overwrite Q on return and issue calls back to back.
//
// nep_arnoldi_*: the expansion of an Arnoldi basis for the operator C^-1 B of a pencil given as an SPMF handle and coefficient
//   rows, B = sum_t cB_t A_t, C factorised by the caller (nep_lu).  One call enqueues `count` steps
//       w = sum_t cB_t A_t v_j (K1), w <- C^-1 w (K5), DGKS against V[:, 0..j] (K6), column j + 1 <- w / beta
//   and row j of the coefficient block (j + 1 projections, beta, flag word) travels to pinned host memory behind an event.
//   Modelled on nep_iar_* (driver.hip); the coefficients of a step are a FULL column (after a restart the kept block is not
//   Hessenberg).  The flag word is nep_orth_dev's, (passes, 2 breakdown + another_pass_wanted), as it stands.  A new vector
//   inside span(V) shows in it either way: bit 2 when beta is not a positive finite number, bit 1 when the last enqueued DGKS
//   pass still wanted another one -- "twice is enough" (Kahan / Parlett): a vector that keeps shrinking by more than sqrt(2)
//   after two passes lies in span(V) to working precision.  The caller reads a non-zero word of a DGKS step as the breakdown.
//   Nothing here divides by a quantity that can be zero (K6 normalises with 1 / beta only for beta > 0) and no index depends on
//   the data.
#include "common.h"
#include <time.h>
#include <vector>

namespace {

constexpr int ROT_ROWS = 64;            // rows of a tile = lanes of a wave
constexpr int ROT_THREADS = 256;
constexpr int ROT_WAVES = ROT_THREADS / 64;
constexpr int ROT_CB = 4;               // output columns per lane and pass over the tile
constexpr int ROT_MAXM = 128;
constexpr int ROT_MAXBLOCKS = 4096;

__global__ __launch_bounds__(ROT_THREADS) void k_basis_rotate(cplx* __restrict__ V, int64_t ldv, int64_t rows, int m, int p,
                                                              const cplx* __restrict__ Qt, int carry) {
    extern __shared__ cplx tile[];                     // tile[k * 64 + r] = V[row0 + r, k]
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int64_t ntiles = (rows + ROT_ROWS - 1) / ROT_ROWS;
    for (int64_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
        const int64_t row = t * ROT_ROWS + lane;
        const bool live = row < rows;
        cplx cv = cmake(0.0, 0.0);
        if (live) {
            for (int k = wave; k < m; k += ROT_WAVES) tile[k * ROT_ROWS + lane] = V[row + (int64_t)k * ldv];
            if (carry && wave == 0) cv = V[row + (int64_t)m * ldv];
        }
        __syncthreads();                               // the whole tile is staged: from here on columns 0 .. p - 1 may change
        if (live) {
            for (int c0 = wave; c0 < p; c0 += ROT_WAVES * ROT_CB) {       // columns c0, c0 + 4, c0 + 8, c0 + 12 of this wave
                cplx acc[ROT_CB];
                int cc[ROT_CB];
#pragma unroll
                for (int i = 0; i < ROT_CB; ++i) { acc[i] = cmake(0.0, 0.0); cc[i] = c0 + i * ROT_WAVES < p ? c0 + i * ROT_WAVES : c0; }
                for (int k = 0; k < m; ++k) {
                    const cplx v = tile[k * ROT_ROWS + lane];
                    const cplx* q = Qt + (int64_t)k * p;
#pragma unroll
                    for (int i = 0; i < ROT_CB; ++i) cfma(acc[i], v, q[cc[i]]);
                }
#pragma unroll
                for (int i = 0; i < ROT_CB; ++i)
                    if (c0 + i * ROT_WAVES < p) V[row + (int64_t)(c0 + i * ROT_WAVES) * ldv] = acc[i];
            }
            if (carry && wave == 0) V[row + (int64_t)p * ldv] = cv;
        }
        __syncthreads();                               // the tile is reused by the next row tile of this workgroup
    }
}

thread_local PinnedRing t_rot_ring;
thread_local NepTableSlots t_rot_slots;

}  // namespace

struct nep_arnoldi {
    nep_spmf* spmf; nep_lu* lu;
    int64_t n, ldv; int32_t maxdim, method;
    cplx* dV; const cplx* d_cB; cplx* dz;
    cplx* dS; nep_cdouble* hS; cplx* hS_dev;           // maxdim rows of (maxdim + 4): device / pinned host / its device address
    std::vector<hipEvent_t> ev;                        // ev[j]: row j is in pinned memory
};

extern "C" {

int32_t nep_basis_rotate(nep_cdouble* dV, int64_t ldv, int64_t rows, int32_t m, int32_t p, const nep_cdouble* hQ, int64_t ldq,
                         int32_t carry, nep_stream stream) {
    ARGCHK(dV && hQ);
    ARGCHK(rows >= 1 && m >= 1 && p >= 1 && p <= m && ldv >= rows && ldq >= m);
    if (m > ROT_MAXM) {
        nep_set_error("nep_basis_rotate: m = %d (1 <= p <= m <= %d)", m, ROT_MAXM);
        return NEP_ERR_UNSUPPORTED;
    }
    hipStream_t st = as_stream(stream);
    const size_t lds = (size_t)ROT_ROWS * m * sizeof(cplx);
    if (lds > 64 * 1024) { const int rc_ = nep_raise_lds((const void*)k_basis_rotate, 160 * 1024); if (rc_) return rc_; }
    std::vector<nep_cdouble> qt((size_t)m * p);        // row-major, compact: Qt[k p + c] = Q[k, c]
    for (int c = 0; c < p; ++c)
        for (int k = 0; k < m; ++k) qt[(size_t)k * p + c] = hQ[k + (int64_t)c * ldq];
    void* dslot = nullptr;
    int which = 0;
    int rc = t_rot_slots.acquire((size_t)ROT_MAXM * ROT_MAXM * sizeof(cplx), &dslot, &which);
    if (rc) return rc;
    rc = t_rot_ring.upload(dslot, qt.data(), qt.size() * sizeof(cplx), st);
    if (rc) return rc;                                 // (nothing was launched on the slot: it needs no guard and is handed out again in its turn)
    const int64_t ntiles = (rows + ROT_ROWS - 1) / ROT_ROWS;
    const int grid = (int)(ntiles < ROT_MAXBLOCKS ? ntiles : ROT_MAXBLOCKS);
    hipLaunchKernelGGL(k_basis_rotate, dim3(grid), dim3(ROT_THREADS), lds, st, (cplx*)dV, ldv, rows, (int)m, (int)p,
                       (const cplx*)dslot, carry ? 1 : 0);
    LAUNCHCHK();
    return t_rot_slots.guard(which, st);
}

int32_t nep_arnoldi_create(nep_spmf* spmf, nep_lu* lu, int64_t n, int32_t maxdim, nep_cdouble* dV, int64_t ldv,
                           const nep_cdouble* d_cB, nep_cdouble* dwork_n, nep_cdouble* dS, nep_cdouble* h_pinnedS,
                           int32_t orth_method, nep_arnoldi** out) {
    ARGCHK(out != nullptr);
    *out = nullptr;
    ARGCHK(spmf && lu && dV && d_cB && dwork_n && dS && h_pinnedS);
    ARGCHK(n > 0 && maxdim >= 1 && ldv >= n && (orth_method == 0 || orth_method == 1));
    nep_arnoldi* s = new nep_arnoldi();
    s->spmf = spmf; s->lu = lu; s->n = n; s->ldv = ldv; s->maxdim = maxdim; s->method = orth_method;
    s->dV = (cplx*)dV; s->d_cB = (const cplx*)d_cB; s->dz = (cplx*)dwork_n;
    s->dS = (cplx*)dS; s->hS = h_pinnedS; s->hS_dev = nullptr;
    void* dp = nullptr;
    if (hipHostGetDevicePointer(&dp, h_pinnedS, 0) == hipSuccess) s->hS_dev = (cplx*)dp; else (void)hipGetLastError();
    s->ev.assign(maxdim, nullptr);
    *out = s;
    return NEP_OK;
}

int32_t nep_arnoldi_destroy(nep_arnoldi* s) {
    if (!s) return NEP_OK;
    for (hipEvent_t e : s->ev) if (e) (void)hipEventDestroy(e);
    delete s;
    return NEP_OK;
}

// steps j0 .. j0 + count - 1: step j reads the columns 0 .. j of the basis and writes column j + 1 and row j
int32_t nep_arnoldi_steps(nep_arnoldi* s, int32_t j0, int32_t count, nep_stream stream) {
    ARGCHK(s && count >= 1 && j0 >= 0 && (int64_t)j0 + count <= s->maxdim);
    hipStream_t st = as_stream(stream);
    const int64_t n = s->n;
    const int ldS = s->maxdim + 4;
    for (int32_t j = j0; j < j0 + count; ++j) {
        const cplx* vj = s->dV + (int64_t)j * s->ldv;
        cplx* w = s->dV + (int64_t)(j + 1) * s->ldv;
        int rc = nep_mlincomb_dev(s->spmf, 1, (const nep_cdouble*)s->d_cB, 1, (const nep_cdouble*)vj, s->ldv, (nep_cdouble*)s->dz, stream);
        if (rc) return rc;
        rc = nep_lu_solve(s->lu, 1, (const nep_cdouble*)s->dz, n, (nep_cdouble*)w, n, 1.0, stream);
        if (rc) return rc;
        cplx* row = s->dS + (int64_t)j * ldS;
        // (the last kernel of the orthogonalisation writes the row to the mapped pinned block itself, as in nep_iar_step)
        cplx* mirror = s->hS_dev ? s->hS_dev + (int64_t)j * ldS : nullptr;
        rc = nep_orth_dev_mirror((const nep_cdouble*)s->dV, s->ldv, n, j + 1, nullptr, (nep_cdouble*)w, (nep_cdouble*)row, s->method,
                                 (nep_cdouble*)mirror, j + 3, stream);
        if (rc) return rc;
        if (!mirror)
            HIPCHK(hipMemcpyAsync(s->hS + (int64_t)j * ldS, row, (size_t)(j + 3) * sizeof(cplx), hipMemcpyDeviceToHost, st));
        if (!s->ev[j]) HIPCHK(hipEventCreateWithFlags(&s->ev[j], hipEventDisableTiming));
        HIPCHK(hipEventRecord(s->ev[j], st));
    }
    return NEP_OK;
}

// blocks the calling thread until row j has reached the pinned block (short naps, as nep_iar_wait)
int32_t nep_arnoldi_wait(nep_arnoldi* s, int32_t j) {
    ARGCHK(s && j >= 0 && j < s->maxdim && s->ev[j]);
    for (;;) {
        const hipError_t e = hipEventQuery(s->ev[j]);
        if (e == hipSuccess) return NEP_OK;
        if (e != hipErrorNotReady) HIPCHK(e);
        struct timespec ts = {0, 20000};
        nanosleep(&ts, nullptr);
    }
}

}  // extern "C"
