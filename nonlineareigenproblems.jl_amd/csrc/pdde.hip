// libnepmi355: K15, the NEP of a time-periodic delay-differential equation (gallery "periodicdde"), for gfx950.
//
// x'(t) = A(t) x(t) + B(t) x(t - tau) with tau-periodic A(t) = sum_i alpha_i(t) A_i and B(t) = sum_j beta_j(t) B_j (dense n x n
// complex terms, column-major).  The matrix function of the NEP is the solution of a matrix ODE over one period,
//
//   MM(S, V) = Y(tau) - V,    Y' = A(t) Y + (B(t) Y) E - Y S,    Y(0) = V (n x p),    E = exp(-tau S)  (an input of its own),
//
// integrated by N classical Runge-Kutta steps of size h = tau / N in the reference's form y <- y + (s1 + 2 s2 + 2 s3 + s4) / 6,
// s_i = h F(.).  The scalar tables are sampled by the host at the 2N + 1 half-step times; step k reads rows 2k, 2k+1, 2k+1, 2k+2.
//
// k_pdde: one launch per call, the whole time loop inside.  A workgroup owns G whole systems (C = G p <= 8 columns) and keeps the
// tile Y and the stage input Z (n x C each) in LDS; thread r owns row r of every column: its 2 C accumulators (A Z)[r, :] and
// (B Z)[r, :], the stage value K[r, :] and the running sum s1 + 2 s2 + ... are registers.  (The running sum is thread-private, so
// it does not need LDS: Y and Z of n = 512, p = 8 are 128 KiB, and a third buffer would not have fitted into 160 KiB.)  One
// thread per row, n rounded up to whole waves, at most 512 threads with at most 204 registers each.  Per
// stage, for k = 0 .. n-1 in this order: a = sum_i alpha_i A_i[r, k] and b = sum_j beta_j B_j[r, k] are formed element by element
// (coalesced reads of the term matrices, which stay in L2 / Infinity Cache; the table row is uniform), Z[k, c] is an LDS
// broadcast, and 2 C complex fused multiply-adds follow.  Then the right products with E and S (p x p, uniform) on the thread's
// own row, K = h F, two barriers around the in-place write of the next stage input.  The order of every sum is fixed and belongs
// to the row and the column alone: a system has the same bits alone, at any position of any batch, with any G.
//
// nep_pdde_mder is a front end of the same launch: system (l, j) has S = J_{der+1}(lam_l), E in closed form, V = [e_j, 0, ..., 0]
// generated in the kernel, and only column der, times der!, is stored, as column j of matrix l.
#include "common.h"
#include <complex>
#include <vector>

namespace {

constexpr int PDDE_NMAX = 512;
constexpr int PDDE_PMAX = 8;
constexpr int PDDE_MMAX = 64;         // terms per side
constexpr int PDDE_CMAX = 8;         // columns of a tile: 16 need 256 registers (one wave per SIMD) and ran at half the rate of 8
constexpr int PDDE_CUS = 256;         // a batch is cut into at least this many tiles where it can be

struct PddeArgs {
    int n, mA, mB, N, nsys;
    int group;                        // systems that share one (S, E) pair (mm: 1, mder: n)
    int unitV;                        // V = [e_(sys % group), 0, ...] instead of a block in memory
    int outcol;                       // >= 0: only this column is stored, times scale, at sys_in_group * ldo
    double h, scale;
    const cplx *A, *B, *alpha, *beta, *SE, *V;
    int64_t ldv, strideV;
    cplx* Out;
    int64_t ldo, strideO;             // strideO: between the groups
};

// Only the fused multiply-adds that are written out are fused: left to itself the compiler contracts h t + y and h t + sum in some
// instantiations and not in others, and a system then has other bits in a tile of 2 than in a tile of 1.  The pragma covers the
// operations written in this function, not those inside the helpers of common.h, which are compiled under the default mode and
// inlined: K = h t and the sums are written out here, and the only helpers used are cmake, cmul and cfma, which consist of
// explicit fma() calls and one bare product that feeds an fma().  RULE: a helper used in this kernel must contain no a * b + c (or
// a product whose result a caller adds to something) outside an explicit fma(); cadd / cscale of common.h must not be chained here.
#pragma clang fp contract(off)
template <int P, int G>
__global__ __launch_bounds__(PDDE_NMAX) void k_pdde(PddeArgs a) {
    constexpr int C = P * G;
    extern __shared__ __align__(16) unsigned char pdde_smem[];
    const int n = a.n;
    cplx* Ys = reinterpret_cast<cplx*>(pdde_smem);
    cplx* Zs = Ys + (size_t)C * n;
    const bool act = (int)threadIdx.x < n;
    const int r = act ? (int)threadIdx.x : n - 1;          // a thread past the end computes the last row and stores nothing
    const int64_t sys0 = (int64_t)blockIdx.x * G;
    const size_t nn = (size_t)n * n;

    int64_t sysg[G];
    bool valid[G];
#pragma unroll
    for (int g = 0; g < G; ++g) {
        valid[g] = sys0 + g < a.nsys;
        sysg[g] = valid[g] ? sys0 + g : (int64_t)a.nsys - 1;           // a padded slot: zero columns, the last system's S and E
    }
#pragma unroll
    for (int g = 0; g < G; ++g)
#pragma unroll
        for (int q = 0; q < P; ++q) {
            cplx v = cmake(0.0, 0.0);
            if (valid[g]) {
                if (a.unitV) { if (q == 0 && r == (int)(sysg[g] % a.group)) v.x = 1.0; }
                else v = a.V[sysg[g] * a.strideV + (int64_t)q * a.ldv + r];
            }
            if (act) { Ys[(size_t)(g * P + q) * n + r] = v; Zs[(size_t)(g * P + q) * n + r] = v; }
        }
    __syncthreads();

    cplx sum[C];
#pragma unroll
    for (int c = 0; c < C; ++c) sum[c] = cmake(0.0, 0.0);

    for (int step = 0; step < a.N; ++step) {
        for (int s = 0; s < 4; ++s) {
            const int trow = 2 * step + ((s + 1) >> 1);
            const cplx* al = a.alpha + (size_t)trow * a.mA;
            const cplx* be = a.beta + (size_t)trow * a.mB;
            cplx AZ[C], BZ[C];
#pragma unroll
            for (int c = 0; c < C; ++c) AZ[c] = BZ[c] = cmake(0.0, 0.0);
            for (int k = 0; k < n; ++k) {
                const size_t e = (size_t)r + (size_t)k * n;
                cplx ea = cmul(al[0], a.A[e]);
                for (int i = 1; i < a.mA; ++i) cfma(ea, al[i], a.A[(size_t)i * nn + e]);
                cplx eb = cmul(be[0], a.B[e]);
                for (int j = 1; j < a.mB; ++j) cfma(eb, be[j], a.B[(size_t)j * nn + e]);
#pragma unroll
                for (int c = 0; c < C; ++c) {
                    const cplx z = Zs[(size_t)c * n + k];
                    cfma(AZ[c], ea, z);
                    cfma(BZ[c], eb, z);
                }
            }
            // K = h ((A Z) + (B Z) E - Z S) on the thread's own row, system by system; K replaces AZ
#pragma unroll
            for (int g = 0; g < G; ++g) {
                const cplx* Sg = a.SE + (size_t)(sysg[g] / a.group) * (2 * P * P);
                const cplx* Eg = Sg + P * P;
                cplx zr[P], f[P];
#pragma unroll
                for (int q = 0; q < P; ++q) zr[q] = Zs[(size_t)(g * P + q) * n + r];
#pragma unroll
                for (int q = 0; q < P; ++q) {
                    cplx t = AZ[g * P + q];
#pragma unroll
                    for (int q2 = 0; q2 < P; ++q2) cfma(t, BZ[g * P + q2], Eg[q2 + q * P]);
#pragma unroll
                    for (int q2 = 0; q2 < P; ++q2) cfma(t, cmake(-zr[q2].x, -zr[q2].y), Sg[q2 + q * P]);
                    f[q] = cmake(a.h * t.x, a.h * t.y);
                }
#pragma unroll
                for (int q = 0; q < P; ++q) AZ[g * P + q] = f[q];
            }
#pragma unroll
            for (int c = 0; c < C; ++c) {
                if (s == 0) sum[c] = AZ[c];
                else if (s == 3) sum[c] = cmake(sum[c].x + AZ[c].x, sum[c].y + AZ[c].y);
                else sum[c] = cmake(sum[c].x + 2.0 * AZ[c].x, sum[c].y + 2.0 * AZ[c].y);
            }
            __syncthreads();                                 // every thread has read the stage input
            if (act) {
#pragma unroll
                for (int c = 0; c < C; ++c) {
                    const size_t o = (size_t)c * n + r;
                    const cplx y = Ys[o];
                    if (s == 3) {
                        const cplx yn = cmake(y.x + sum[c].x / 6.0, y.y + sum[c].y / 6.0);
                        Ys[o] = yn; Zs[o] = yn;
                    } else {
                        const double cz = s == 2 ? 1.0 : 0.5;
                        Zs[o] = cmake(y.x + cz * AZ[c].x, y.y + cz * AZ[c].y);
                    }
                }
            }
            __syncthreads();
        }
    }

    if (!act) return;
#pragma unroll
    for (int g = 0; g < G; ++g) {
        if (!valid[g]) continue;
        const int64_t grp = sysg[g] / a.group, ing = sysg[g] % a.group;
#pragma unroll
        for (int q = 0; q < P; ++q) {
            if (a.outcol >= 0 && q != a.outcol) continue;
            cplx v = cmake(0.0, 0.0);
            if (a.unitV) { if (q == 0 && r == (int)ing) v.x = 1.0; }
            else v = a.V[sysg[g] * a.strideV + (int64_t)q * a.ldv + r];
            const cplx y = Ys[(size_t)(g * P + q) * n + r];
            cplx d = cmake(y.x - v.x, y.y - v.y);
            if (a.outcol >= 0) {
                d = cscale(a.scale, d);
                a.Out[grp * a.strideO + ing * a.ldo + r] = d;
            } else {
                a.Out[grp * a.strideO + (int64_t)q * a.ldo + r] = d;
            }
        }
    }
}

template <int P, int G>
int pdde_launch(const PddeArgs& a, hipStream_t st) {
    const size_t lds = (size_t)2 * P * G * a.n * sizeof(cplx);
    if (lds > 64 * 1024) {
        const int rc = nep_raise_lds((const void*)k_pdde<P, G>, 160 * 1024);
        if (rc) return rc;
    }
    const unsigned tiles = (unsigned)(((int64_t)a.nsys + G - 1) / G);
    hipLaunchKernelGGL((k_pdde<P, G>), dim3(tiles), dim3(((a.n + 63) / 64) * 64), lds, st, a);
    LAUNCHCHK();
    return NEP_OK;
}

// G: the widest tile of {8, 4, 2, 1} systems with G p <= PDDE_CMAX columns that still cuts the batch into PDDE_CUS tiles; G = 1
// when none does.  The result does not depend on G.
template <int P>
int pdde_dispatch(const PddeArgs& a, hipStream_t st) {
    auto enough = [&](int g) { return g * P <= PDDE_CMAX && ((int64_t)a.nsys + g - 1) / g >= PDDE_CUS; };
    if constexpr (8 * P <= PDDE_CMAX) { if (enough(8)) return pdde_launch<P, 8>(a, st); }
    if constexpr (4 * P <= PDDE_CMAX) { if (enough(4)) return pdde_launch<P, 4>(a, st); }
    if constexpr (2 * P <= PDDE_CMAX) { if (enough(2)) return pdde_launch<P, 2>(a, st); }
    return pdde_launch<P, 1>(a, st);
}

}  // namespace

struct nep_pdde {
    int32_t n = 0, mA = 0, mB = 0, N = 0;
    double tau = 0.0;
    cplx *A = nullptr, *B = nullptr, *alpha = nullptr, *beta = nullptr;
    PinnedRing ring;                  // staging of the (S, E) blocks
};

int32_t nep_pdde_destroy(nep_pdde* d) {
    if (!d) return NEP_OK;
    cplx* blocks[] = {d->A, d->B, d->alpha, d->beta};
    for (cplx* p : blocks)
        if (p) (void)hipFree(p);
    delete d;
    return NEP_OK;
}

int32_t nep_pdde_create(int32_t n, int32_t mA, int32_t mB, const nep_cdouble* h_A, const nep_cdouble* h_B, int32_t N, double tau,
                        const nep_cdouble* h_alpha, const nep_cdouble* h_beta, nep_pdde** out) {
    ARGCHK(out);
    *out = nullptr;
    ARGCHK(n >= 1 && n <= PDDE_NMAX);
    ARGCHK(mA >= 1 && mA <= PDDE_MMAX && mB >= 1 && mB <= PDDE_MMAX);
    ARGCHK(N >= 1 && N <= (1 << 24));
    ARGCHK(tau == tau && tau - tau == 0.0);
    ARGCHK(h_A && h_B && h_alpha && h_beta);
    nep_pdde* d = new nep_pdde();
    d->n = n; d->mA = mA; d->mB = mB; d->N = N; d->tau = tau;
    const size_t nn = (size_t)n * n * sizeof(cplx), rows = (size_t)2 * N + 1;
#define PDDECHK(call) do { hipError_t e_ = (call); if (e_ != hipSuccess) { nep_set_error("%s:%d: %s: %s", __FILE__, __LINE__, #call, hipGetErrorString(e_)); nep_pdde_destroy(d); return NEP_ERR_HIP; } } while (0)
    PDDECHK(hipMalloc((void**)&d->A, nn * mA));
    PDDECHK(hipMalloc((void**)&d->B, nn * mB));
    PDDECHK(hipMalloc((void**)&d->alpha, rows * mA * sizeof(cplx)));
    PDDECHK(hipMalloc((void**)&d->beta, rows * mB * sizeof(cplx)));
    PDDECHK(hipMemcpy(d->A, h_A, nn * mA, hipMemcpyHostToDevice));
    PDDECHK(hipMemcpy(d->B, h_B, nn * mB, hipMemcpyHostToDevice));
    PDDECHK(hipMemcpy(d->alpha, h_alpha, rows * mA * sizeof(cplx), hipMemcpyHostToDevice));
    PDDECHK(hipMemcpy(d->beta, h_beta, rows * mB * sizeof(cplx), hipMemcpyHostToDevice));
#undef PDDECHK
    *out = d;
    return NEP_OK;
}

int32_t nep_pdde_info(const nep_pdde* d, int64_t info[4]) {
    ARGCHK(d && info);
    info[0] = d->n;
    info[1] = d->N;
    info[2] = (int64_t)(((size_t)d->n * d->n + (size_t)2 * d->N + 1) * (d->mA + d->mB) * sizeof(cplx));
    info[3] = PDDE_PMAX;
    return NEP_OK;
}

// the launch both entry points share: h_SE holds npair blocks of [S (p x p, column-major), E (p x p, column-major)]
static int pdde_run(const nep_pdde* d, PddeArgs& a, int p, const cplx* h_SE, size_t npair, hipStream_t st) {
    const size_t bytes = npair * 2 * p * p * sizeof(cplx);
    void* dSE = nullptr;
    int rc = nep_pool_alloc(&dSE, bytes);
    if (rc) return rc;
    rc = const_cast<nep_pdde*>(d)->ring.upload(dSE, h_SE, bytes, st);
    if (rc == NEP_OK) {
        a.n = d->n; a.mA = d->mA; a.mB = d->mB; a.N = d->N;
        a.h = d->tau / d->N;
        a.A = d->A; a.B = d->B; a.alpha = d->alpha; a.beta = d->beta;
        a.SE = (const cplx*)dSE;
        switch (p) {
            case 1: rc = pdde_dispatch<1>(a, st); break;
            case 2: rc = pdde_dispatch<2>(a, st); break;
            case 3: rc = pdde_dispatch<3>(a, st); break;
            case 4: rc = pdde_dispatch<4>(a, st); break;
            case 5: rc = pdde_dispatch<5>(a, st); break;
            case 6: rc = pdde_dispatch<6>(a, st); break;
            case 7: rc = pdde_dispatch<7>(a, st); break;
            default: rc = pdde_dispatch<8>(a, st); break;
        }
    }
    nep_pool_free_on(dSE, st, true);
    return rc;
}

int32_t nep_pdde_mm(const nep_pdde* d, int32_t nsys, int32_t p, const nep_cdouble* h_S, const nep_cdouble* h_E, const nep_cdouble* dV,
                    int64_t ldv, int64_t strideV, nep_cdouble* dOut, int64_t ldo, int64_t strideO, nep_stream stream) {
    ARGCHK(d);
    ARGCHK(nsys >= 0 && p >= 1 && p <= PDDE_PMAX);
    if (nsys == 0) return NEP_OK;
    ARGCHK(h_S && h_E && dV && dOut);
    ARGCHK(ldv >= d->n && ldo >= d->n);
    ARGCHK(nsys == 1 || (strideV >= 0 && strideO >= ldo * (p - 1) + d->n));
    const size_t pp = (size_t)p * p;
    std::vector<cplx> se((size_t)nsys * 2 * pp);
    for (size_t s = 0; s < (size_t)nsys; ++s) {
        memcpy(&se[s * 2 * pp], h_S + s * pp, pp * sizeof(cplx));
        memcpy(&se[s * 2 * pp + pp], h_E + s * pp, pp * sizeof(cplx));
    }
    PddeArgs a;
    a.nsys = nsys; a.group = 1; a.unitV = 0; a.outcol = -1; a.scale = 1.0;
    a.V = (const cplx*)dV; a.ldv = ldv; a.strideV = strideV;
    a.Out = (cplx*)dOut; a.ldo = ldo; a.strideO = strideO;
    return pdde_run(d, a, p, se.data(), (size_t)nsys, as_stream(stream));
}

int32_t nep_pdde_mder(const nep_pdde* d, int32_t nlam, const nep_cdouble* h_lam, int32_t der, nep_cdouble* dOut, int64_t ldo,
                      int64_t stride, nep_stream stream) {
    ARGCHK(d);
    ARGCHK(nlam >= 0 && der >= 0 && der < PDDE_PMAX);
    if (nlam == 0) return NEP_OK;
    ARGCHK(h_lam && dOut);
    ARGCHK(ldo >= d->n && (nlam == 1 || stride >= ldo * (int64_t)(d->n - 1) + d->n));
    ARGCHK((int64_t)nlam * d->n <= INT32_MAX);
    const int p = der + 1;
    const size_t pp = (size_t)p * p;
    std::vector<cplx> se((size_t)nlam * 2 * pp);
    double fact = 1.0;
    for (int k = 2; k <= der; ++k) fact *= k;
    for (int l = 0; l < nlam; ++l) {
        cplx* S = &se[(size_t)l * 2 * pp];
        cplx* E = S + pp;
        for (size_t i = 0; i < 2 * pp; ++i) { S[i].x = 0.0; S[i].y = 0.0; }
        // S = J_p(lam): lam on the diagonal, ones above it; E = exp(-tau S) = e^(-tau lam) Toeplitz((-tau)^k / k!)
        const std::complex<double> lam(h_lam[l].re, h_lam[l].im);
        const std::complex<double> e0 = std::exp(-d->tau * lam);
        double c = 1.0;
        for (int k = 0; k < p; ++k) {
            if (k > 0) c *= -d->tau / k;
            const std::complex<double> ek = e0 * c;
            for (int i = 0; i + k < p; ++i) { E[i + (size_t)(i + k) * p].x = ek.real(); E[i + (size_t)(i + k) * p].y = ek.imag(); }
        }
        for (int i = 0; i < p; ++i) {
            S[i + (size_t)i * p].x = lam.real(); S[i + (size_t)i * p].y = lam.imag();
            if (i + 1 < p) S[i + (size_t)(i + 1) * p].x = 1.0;
        }
    }
    PddeArgs a;
    a.nsys = nlam * d->n; a.group = d->n; a.unitV = 1; a.outcol = der; a.scale = fact;
    a.V = nullptr; a.ldv = 0; a.strideV = 0;
    a.Out = (cplx*)dOut; a.ldo = ldo; a.strideO = stride;
    return pdde_run(d, a, p, se.data(), (size_t)nlam, as_stream(stream));
}
