// libnepmi355: the boundary-element NEP of the Fichera corner (gallery "bem_fichera"), assembled on the device, for gfx950.
//
// M(lam) is dense, n x n for n flat triangles, and every entry depends on lam: with the 3-point Gauss rule on each triangle
// (points g_r[i], weights w_r[i] = area_r / 3), W_p = w_r[i] w_c[j] and d_p = |g_r[i] - g_c[j]| over the 9 pairs p = (i, j),
//
//   M(lam)[r, c]      = sum_p W_p (exp(i lam d_p) - 1) / d_p / (4 pi)  +  S0[r, c]                  (r <= c)
//   M^(m)(lam)[r, c]  = sum_p W_p (i d_p)^m exp(i lam d_p) / d_p / (4 pi),   m >= 1
//
// and a pair with d_p == 0 (the same Gauss point of the same triangle, exactly) contributes i lam W_p (m = 0), i W_p (m = 1),
// nothing (m >= 2) inside the sum.  S0 is the singular part, the Gauss rule over triangle r of de Hoop's closed form of the
// integral of 1 / |x - y| over triangle c, divided by 4 pi; it does not depend on lam and is computed once per handle.  The lower
// triangle is the MIRROR of the upper one: the quadrature is not symmetric in (r, c), so S0 is stored mirrored and the matrix-free
// kernels read the mirrored copy.
//
// de Hoop's formula holds log((|R_b| + R_b.tau) / (|R_a| + R_a.tau)) per edge, which cancels when R.tau ~ -|R|.  Here |R| + s is
// taken as h^2 / (|R| - s) for s = R.tau < 0, h^2 = (R_a.nu)^2 + (n.R_1)^2 the squared distance of the point from the edge's
// line, and as |R| + s for s >= 0; the term p log(.) is 0 when h^2 == 0 (its limit).
//
// Kernels.  k_bem_geom: one thread per triangle, Gauss points and weights (every operation rounded on its own, so that a host
// evaluation in the same order reproduces them bit for bit), tangents, normal and edge normals.  k_bem_s0: one thread per entry
// r <= c, lanes along r, writes both mirror images.  k_bem_assemble: a workgroup owns a 64 x 64 tile on or above the diagonal,
// lanes along the rows (their Gauss points in registers), the tile's column Gauss points and weights in LDS, a wave per column;
// the 9 distances of an entry are formed once and reused for every shift of the batch; both mirror images are written from the
// same register, so the result is bitwise symmetric.  k_bem_apply (mlincomb and resid): matrix-free, a workgroup owns BEM_ROWS
// rows, its lanes run along the columns (column data in registers, row data uniform), one pass over the pairs with a Horner loop
// in (i d_p) whose step is two fused multiply-adds because i d_p is purely imaginary; the row sums go through the DPP wave sum and
// the LDS tree of deflate_border.hip.  No atomics, fixed summation order: two calls give the same bits.  Shifts and coefficients
// travel as kernel arguments (at most BEM_LAM shifts, BEM_KMAX coefficients per launch; longer lists take several launches).
// exp(i lam d) = exp(-Im(lam) d) (cos, sin)(Re(lam) d): nothing overflows for |Im(lam)| d < 700.
#include "common.h"

namespace {

constexpr int BEM_THREADS = 256;
constexpr int BEM_TILE = 64;          // rows and columns of a tile of k_bem_assemble
constexpr int BEM_LAM = 32;           // shifts per launch
constexpr int BEM_KMAX = 64;          // Horner coefficients per launch
constexpr int BEM_ROWS = 1;           // rows per workgroup of k_bem_apply (2: 255 registers, one wave per SIMD; 1: 172, two)
constexpr int BEM_NAUX = 21;          // tau1, tau2, tau3, normal, nu1, nu2, nu3
constexpr double BEM_4PI = 12.566370614359172;

struct BemLams { double re[BEM_LAM], im[BEM_LAM]; };
struct BemCoef { double re[BEM_KMAX], im[BEM_KMAX]; };

struct v3 { double x, y, z; };
__device__ __forceinline__ v3 v3make(double x, double y, double z) { v3 r; r.x = x; r.y = y; r.z = z; return r; }
__device__ __forceinline__ v3 v3sub(v3 a, v3 b) { return v3make(a.x - b.x, a.y - b.y, a.z - b.z); }
__device__ __forceinline__ double v3dot(v3 a, v3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
__device__ __forceinline__ double v3norm(v3 a) { return sqrt(v3dot(a, a)); }
__device__ __forceinline__ v3 v3cross(v3 a, v3 b) {
    return v3make(a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x);
}
__device__ __forceinline__ v3 v3unit(v3 a) { const double l = v3norm(a); return v3make(a.x / l, a.y / l, a.z / l); }

// gp[(3 g + x) n + t]: coordinate x of Gauss point g of triangle t;  gw[g n + t];  aux[q n + t], q < 21
__global__ __launch_bounds__(BEM_THREADS) void k_bem_geom(int64_t n, const double* __restrict__ vert,
                                                          const double* __restrict__ area, double* __restrict__ gp,
                                                          double* __restrict__ gw, double* __restrict__ aux) {
    const int64_t t = (int64_t)blockIdx.x * BEM_THREADS + threadIdx.x;
    if (t >= n) return;
    double P[9];
    for (int q = 0; q < 9; ++q) P[q] = vert[t * 9 + q];
    const double c23 = 2.0 / 3.0, c16 = 1.0 / 6.0;
    for (int g = 0; g < 3; ++g) {
        for (int x = 0; x < 3; ++x) {
            // pt[g, :] * [P1; P2; P3], left to right, every product and sum rounded (no contraction)
            const double a = __dmul_rn(g == 0 ? c23 : c16, P[x]);
            const double b = __dmul_rn(g == 1 ? c23 : c16, P[3 + x]);
            const double c = __dmul_rn(g == 2 ? c23 : c16, P[6 + x]);
            gp[(int64_t)(3 * g + x) * n + t] = __dadd_rn(__dadd_rn(a, b), c);
        }
        gw[(int64_t)g * n + t] = __dmul_rn(area[t], 1.0 / 3.0);
    }
    const v3 P1 = v3make(P[0], P[1], P[2]), P2 = v3make(P[3], P[4], P[5]), P3 = v3make(P[6], P[7], P[8]);
    v3 u[7];
    u[0] = v3unit(v3sub(P2, P1));
    u[1] = v3unit(v3sub(P3, P2));
    u[2] = v3unit(v3sub(P1, P3));
    u[3] = v3unit(v3cross(u[0], u[1]));
    u[4] = v3unit(v3cross(u[0], u[3]));
    u[5] = v3unit(v3cross(u[1], u[3]));
    u[6] = v3unit(v3cross(u[2], u[3]));
    for (int q = 0; q < 7; ++q) {
        aux[(int64_t)(3 * q) * n + t] = u[q].x;
        aux[(int64_t)(3 * q + 1) * n + t] = u[q].y;
        aux[(int64_t)(3 * q + 2) * n + t] = u[q].z;
    }
}

// one edge of de Hoop's formula in the cancellation-free form: p log((|R_b| + s_b) / (|R_a| + s_a))
__device__ __forceinline__ double bem_edge(v3 Ra, v3 Rb, double na, double nb, v3 tau, v3 nu, double q2) {
    const double p = v3dot(Ra, nu);
    const double sa = v3dot(Ra, tau), sb = v3dot(Rb, tau);
    const double h2 = p * p + q2;
    if (h2 == 0.0) return 0.0;
    const double fa = sa >= 0.0 ? na + sa : h2 / (na - sa);
    const double fb = sb >= 0.0 ? nb + sb : h2 / (nb - sb);
    return p * log(fb / fa);
}

__device__ __forceinline__ double bem_dehoop(v3 x, v3 P1, v3 P2, v3 P3, const v3* u) {
    const v3 R1 = v3sub(P1, x), R2 = v3sub(P2, x), R3 = v3sub(P3, x);
    const double n1 = v3norm(R1), n2 = v3norm(R2), n3 = v3norm(R3);
    const double q = v3dot(u[3], R1);
    const double numer = fabs(R1.x * R2.y * R3.z - R1.x * R2.z * R3.y + R1.y * R2.z * R3.x - R1.y * R2.x * R3.z
                              + R1.z * R2.x * R3.y - R1.z * R2.y * R3.x);
    const double denom = n1 * n2 * n3 + n1 * v3dot(R2, R3) + n2 * v3dot(R1, R3) + n3 * v3dot(R1, R2);
    double solang = 2.0 * atan2(numer, denom);
    if (solang < 0.0) solang += 2.0 * 3.141592653589793;
    const double q2 = q * q;
    double F = -fabs(q) * solang;
    F += bem_edge(R1, R2, n1, n2, u[0], u[4], q2);
    F += bem_edge(R2, R3, n2, n3, u[1], u[5], q2);
    F += bem_edge(R3, R1, n3, n1, u[2], u[6], q2);
    return F;
}

// S0[r, c] = S0[c, r] = sum_g w_r[g] deHoop(g_r[g], triangle c) / (4 pi), r <= c: 64 rows x 4 columns per workgroup
__global__ __launch_bounds__(BEM_THREADS) void k_bem_s0(int64_t n, const double* __restrict__ vert, const double* __restrict__ gp,
                                                        const double* __restrict__ gw, const double* __restrict__ aux,
                                                        double* __restrict__ S0) {
    const int64_t r = (int64_t)blockIdx.x * 64 + (threadIdx.x & 63);
    const int64_t c = (int64_t)blockIdx.y * 4 + (threadIdx.x >> 6);
    if (r >= n || c >= n || r > c) return;
    const double* P = vert + c * 9;
    const v3 P1 = v3make(P[0], P[1], P[2]), P2 = v3make(P[3], P[4], P[5]), P3 = v3make(P[6], P[7], P[8]);
    v3 u[7];
    for (int q = 0; q < 7; ++q)
        u[q] = v3make(aux[(int64_t)(3 * q) * n + c], aux[(int64_t)(3 * q + 1) * n + c], aux[(int64_t)(3 * q + 2) * n + c]);
    double s = 0.0;
    for (int g = 0; g < 3; ++g) {
        const v3 x = v3make(gp[(int64_t)(3 * g) * n + r], gp[(int64_t)(3 * g + 1) * n + r], gp[(int64_t)(3 * g + 2) * n + r]);
        s += gw[(int64_t)g * n + r] * bem_dehoop(x, P1, P2, P3, u);
    }
    s /= BEM_4PI;
    S0[r + c * n] = s;
    S0[c + r * n] = s;
}

// E i^m for m mod 4
__device__ __forceinline__ cplx bem_rot(cplx E, int m) {
    switch (m & 3) {
        case 0: return E;
        case 1: return cmake(-E.y, E.x);
        case 2: return cmake(-E.x, -E.y);
        default: return cmake(E.y, -E.x);
    }
}
__device__ __forceinline__ double bem_pow(double d, int m) {          // d^m, m >= 1, by m - 1 products
    double v = d;
    for (int q = 1; q < m; ++q) v *= d;
    return v;
}
__device__ __forceinline__ cplx bem_expi(double lr, double li, double d) {      // exp(i (lr + i li) d)
    double s, c;
    sincos(lr * d, &s, &c);
    const double ex = li == 0.0 ? 1.0 : exp(-li * d);
    return cmake(ex * c, ex * s);
}

// out[l stride + r + c ldo] = out[l stride + c + r ldo] = M^(der)(lam_l)[r, c], r <= c < n, l < nlam <= BEM_LAM
__global__ __launch_bounds__(BEM_THREADS) void k_bem_assemble(int64_t n, const double* __restrict__ gp,
                                                              const double* __restrict__ gw, const double* __restrict__ S0,
                                                              BemLams lams, int nlam, int der, cplx* __restrict__ out, int64_t ldo,
                                                              int64_t stride) {
    if (blockIdx.x > blockIdx.y) return;                 // a tile below the diagonal: written as the mirror of its transpose
    __shared__ double cg[12][BEM_TILE];                  // rows 0..8: Gauss points, 9..11: weights of the tile's columns
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t r = (int64_t)blockIdx.x * BEM_TILE + lane;
    const int64_t c0 = (int64_t)blockIdx.y * BEM_TILE;
    for (int i = threadIdx.x; i < 12 * BEM_TILE; i += BEM_THREADS) {
        const int q = i / BEM_TILE, cc = i - q * BEM_TILE;
        const int64_t c = c0 + cc;
        cg[q][cc] = c < n ? (q < 9 ? gp[(int64_t)q * n + c] : gw[(int64_t)(q - 9) * n + c]) : 0.0;
    }
    double rg[9], rw[3];
    const int64_t rr = r < n ? r : n - 1;                // a lane past the end reads the last row and stores nothing
    for (int q = 0; q < 9; ++q) rg[q] = gp[(int64_t)q * n + rr];
    for (int q = 0; q < 3; ++q) rw[q] = gw[(int64_t)q * n + rr];
    __syncthreads();
    for (int cl = wave; cl < BEM_TILE; cl += BEM_THREADS / 64) {
        const int64_t c = c0 + cl;
        if (c >= n) break;
        if (r >= n || r > c) continue;
        double d[9], wd[9];
#pragma unroll
        for (int i = 0; i < 3; ++i)
#pragma unroll
            for (int j = 0; j < 3; ++j) {
                const double dx = rg[3 * i] - cg[3 * j][cl], dy = rg[3 * i + 1] - cg[3 * j + 1][cl], dz = rg[3 * i + 2] - cg[3 * j + 2][cl];
                const double dd = sqrt(dx * dx + dy * dy + dz * dz);
                const double w = rw[i] * cg[9 + j][cl];
                d[3 * i + j] = dd;
                wd[3 * i + j] = dd == 0.0 ? w : w / dd;
            }
        const double s0 = der == 0 ? S0[r + c * n] : 0.0;
        for (int l = 0; l < nlam; ++l) {
            const double lr = lams.re[l], li = lams.im[l];
            cplx acc = cmake(0.0, 0.0);
#pragma unroll
            for (int p = 0; p < 9; ++p) {
                if (d[p] == 0.0) {
                    if (der == 0) { acc.x -= li * wd[p]; acc.y += lr * wd[p]; }
                    else if (der == 1) acc.y += wd[p];
                    continue;
                }
                cplx E = bem_expi(lr, li, d[p]);
                double f = wd[p];
                if (der == 0) E.x -= 1.0;
                else { E = bem_rot(E, der); f *= bem_pow(d[p], der); }
                acc.x = fma(f, E.x, acc.x); acc.y = fma(f, E.y, acc.y);
            }
            const cplx v = cmake(acc.x / BEM_4PI + s0, acc.y / BEM_4PI);
            cplx* o = out + (int64_t)l * stride;
            o[r + c * ldo] = v;
            o[c + r * ldo] = v;
        }
    }
}

// Matrix-free products.  Batch b = blockIdx.y uses the shift lams[b], the block V + b vstride and writes out + b ostride:
//   out_b[r] = (beta ? out_b[r] : 0) + sum_c sum_{j < k} a_j M^(j + sd)(lam_b)[r, c] V_b[c, j]
// (nep_bem_mlincomb: one batch; nep_bem_resid: k = 1, sd = 0, a = 1, one batch per shift).  a_j == 0 drops column j unread.
__global__ __launch_bounds__(BEM_THREADS) void k_bem_apply(int64_t n, const double* __restrict__ gp, const double* __restrict__ gw,
                                                           const double* __restrict__ S0, BemLams lams, int k, int sd, BemCoef a,
                                                           const cplx* __restrict__ V, int64_t ldv, int64_t vstride, cplx* out,
                                                           int64_t ostride, int beta) {
    __shared__ cplx red[BEM_ROWS][BEM_THREADS / 64];
    const int b = blockIdx.y;
    const double lr = lams.re[b], li = lams.im[b];
    const cplx* Vb = V + (int64_t)b * vstride;
    const int64_t r0 = (int64_t)blockIdx.x * BEM_ROWS;
    double rg[BEM_ROWS][9], rw[BEM_ROWS][3];
#pragma unroll
    for (int q = 0; q < BEM_ROWS; ++q) {
        const int64_t r = r0 + q < n ? r0 + q : n - 1;   // a row past the end is computed as the last row and not stored
        for (int x = 0; x < 9; ++x) rg[q][x] = gp[(int64_t)x * n + r];
        for (int x = 0; x < 3; ++x) rw[q][x] = gw[(int64_t)x * n + r];
    }
    const int j0 = sd == 0 ? 1 : 0;                      // Horner runs over j >= j0; the term of M itself (E - 1, S0) is separate
    const int m0 = sd + j0;                              // power of (i d) in front of the Horner sum
    const int jz0 = -sd, jz1 = 1 - sd;                   // columns that meet derivative 0 and 1 (the d == 0 pairs)
    cplx accL[BEM_ROWS], accS[BEM_ROWS];
#pragma unroll
    for (int q = 0; q < BEM_ROWS; ++q) accL[q] = accS[q] = cmake(0.0, 0.0);
    for (int64_t c = threadIdx.x; c < n; c += BEM_THREADS) {
        double g[9], w[3];
        for (int x = 0; x < 9; ++x) g[x] = gp[(int64_t)x * n + c];
        for (int x = 0; x < 3; ++x) w[x] = gw[(int64_t)x * n + c];
        double d[BEM_ROWS][9], wd[BEM_ROWS][9];
        cplx H[BEM_ROWS][9];
#pragma unroll
        for (int q = 0; q < BEM_ROWS; ++q) {
            // The lam part of an entry is the same set of 9 terms for (r, c) and (c, r): |g_r[i] - g_c[j]| and w_r[i] w_c[j] do
            // not change bits when the roles are swapped, so below the diagonal only the order of the 9 additions differs from
            // the mirrored entry of k_bem_assemble.  (The singular part IS different: it is read from the mirrored S0.)
#pragma unroll
            for (int i = 0; i < 3; ++i)
#pragma unroll
                for (int j = 0; j < 3; ++j) {
                    const double dx = rg[q][3 * i] - g[3 * j], dy = rg[q][3 * i + 1] - g[3 * j + 1], dz = rg[q][3 * i + 2] - g[3 * j + 2];
                    const double dd = sqrt(dx * dx + dy * dy + dz * dz);
                    const double ww = rw[q][i] * w[j];
                    d[q][3 * i + j] = dd;
                    wd[q][3 * i + j] = dd == 0.0 ? ww : ww / dd;
                    H[q][3 * i + j] = cmake(0.0, 0.0);
                }
        }
        for (int j = k - 1; j >= j0; --j) {
            cplx bj = cmake(0.0, 0.0);
            if (a.re[j] != 0.0 || a.im[j] != 0.0) bj = cmul(cmake(a.re[j], a.im[j]), Vb[c + (int64_t)j * ldv]);
#pragma unroll
            for (int q = 0; q < BEM_ROWS; ++q)
#pragma unroll
                for (int p = 0; p < 9; ++p) {            // H <- H (i d) + b_j
                    const cplx h = H[q][p];
                    H[q][p] = cmake(fma(-d[q][p], h.y, bj.x), fma(d[q][p], h.x, bj.y));
                }
        }
        cplx b0 = cmake(0.0, 0.0), bz0 = cmake(0.0, 0.0), bz1 = cmake(0.0, 0.0);
        if (sd == 0 && (a.re[0] != 0.0 || a.im[0] != 0.0)) b0 = cmul(cmake(a.re[0], a.im[0]), Vb[c]);
        // the columns that meet derivative 0 and 1 belong to column c alone; they are loaded wherever a pair of this column has
        // d == 0 (on a Fichera mesh: the diagonal entry only; a mesh with coinciding Gauss points elsewhere is treated as
        // k_bem_assemble treats it)
        bool anyzero = false;
#pragma unroll
        for (int q = 0; q < BEM_ROWS; ++q)
#pragma unroll
            for (int p = 0; p < 9; ++p) anyzero = anyzero || d[q][p] == 0.0;
        if (anyzero) {
            if (jz0 >= 0 && jz0 < k && (a.re[jz0] != 0.0 || a.im[jz0] != 0.0))
                bz0 = cmul(cmake(a.re[jz0], a.im[jz0]), Vb[c + (int64_t)jz0 * ldv]);
            if (jz1 >= 0 && jz1 < k && (a.re[jz1] != 0.0 || a.im[jz1] != 0.0))
                bz1 = cmul(cmake(a.re[jz1], a.im[jz1]), Vb[c + (int64_t)jz1 * ldv]);
        }
#pragma unroll
        for (int q = 0; q < BEM_ROWS; ++q) {
#pragma unroll
            for (int p = 0; p < 9; ++p) {
                const double dd = d[q][p], f = wd[q][p];
                if (dd == 0.0) {                         // W (i lam b_[der 0] + i b_[der 1])
                    const cplx t = cadd(cmul(cmake(-li, lr), bz0), cmake(-bz1.y, bz1.x));
                    cfma(accL[q], f, t);
                    continue;
                }
                const cplx E = bem_expi(lr, li, dd);
                cplx t = cmake(0.0, 0.0);
                if (k > j0) t = cscale(bem_pow(dd, m0), cmul(bem_rot(E, m0), H[q][p]));
                if (sd == 0) cfma(t, cmake(E.x - 1.0, E.y), b0);
                cfma(accL[q], f, t);
            }
            if (sd == 0) {
                const int64_t r = r0 + q < n ? r0 + q : n - 1;
                cfma(accS[q], S0[c + r * n], b0);        // S0 is mirrored: column r read along c
            }
        }
    }
#pragma unroll
    for (int q = 0; q < BEM_ROWS; ++q) {
        const cplx s = wave_sum_dpp(cmake(accL[q].x / BEM_4PI + accS[q].x, accL[q].y / BEM_4PI + accS[q].y));
        if ((threadIdx.x & 63) == 0) red[q][threadIdx.x >> 6] = s;
    }
    __syncthreads();
    if (threadIdx.x < BEM_ROWS && r0 + threadIdx.x < n) {
        const int q = threadIdx.x;
        cplx* o = out + (int64_t)b * ostride + r0 + q;
        const cplx s = cadd(cadd(red[q][0], red[q][1]), cadd(red[q][2], red[q][3]));
        *o = beta ? cadd(*o, s) : s;
    }
}

}  // namespace

struct nep_bem {
    int64_t n = 0;
    int32_t gauss_order = 3;
    double *vert = nullptr, *area = nullptr, *gp = nullptr, *gw = nullptr, *aux = nullptr, *S0 = nullptr;
};

int32_t nep_bem_destroy(nep_bem* b) {
    if (!b) return NEP_OK;
    double* blocks[] = {b->vert, b->area, b->gp, b->gw, b->aux, b->S0};
    for (double* p : blocks)
        if (p) (void)hipFree(p);
    delete b;
    return NEP_OK;
}

int32_t nep_bem_create(int64_t n, const double* h_vert, const double* h_area, int32_t gauss_order, nep_bem** out) {
    ARGCHK(out);
    *out = nullptr;
    if (gauss_order != 3) {
        nep_set_error("nep_bem_create: Gauss order %d is not implemented (only 3)", gauss_order);
        return NEP_ERR_UNSUPPORTED;
    }
    ARGCHK(h_vert && h_area);
    ARGCHK(n >= 1 && n <= 65536);
    nep_bem* b = new nep_bem();
    b->n = n;
    b->gauss_order = gauss_order;
#define BEMCHK(call) do { hipError_t e_ = (call); if (e_ != hipSuccess) { nep_set_error("%s:%d: %s: %s", __FILE__, __LINE__, #call, hipGetErrorString(e_)); nep_bem_destroy(b); return NEP_ERR_HIP; } } while (0)
    BEMCHK(hipMalloc((void**)&b->vert, (size_t)n * 9 * sizeof(double)));
    BEMCHK(hipMalloc((void**)&b->area, (size_t)n * sizeof(double)));
    BEMCHK(hipMalloc((void**)&b->gp, (size_t)n * 9 * sizeof(double)));
    BEMCHK(hipMalloc((void**)&b->gw, (size_t)n * 3 * sizeof(double)));
    BEMCHK(hipMalloc((void**)&b->aux, (size_t)n * BEM_NAUX * sizeof(double)));
    BEMCHK(hipMalloc((void**)&b->S0, (size_t)n * n * sizeof(double)));
    BEMCHK(hipMemcpy(b->vert, h_vert, (size_t)n * 9 * sizeof(double), hipMemcpyHostToDevice));
    BEMCHK(hipMemcpy(b->area, h_area, (size_t)n * sizeof(double), hipMemcpyHostToDevice));
    hipLaunchKernelGGL(k_bem_geom, dim3((unsigned)((n + BEM_THREADS - 1) / BEM_THREADS)), dim3(BEM_THREADS), 0, 0, n, b->vert, b->area,
                       b->gp, b->gw, b->aux);
    BEMCHK(hipGetLastError());
    hipLaunchKernelGGL(k_bem_s0, dim3((unsigned)((n + 63) / 64), (unsigned)((n + 3) / 4)), dim3(BEM_THREADS), 0, 0, n, b->vert, b->gp,
                       b->gw, b->aux, b->S0);
    BEMCHK(hipGetLastError());
    BEMCHK(hipStreamSynchronize(0));                     // the handle is complete on return, whichever stream uses it next
#undef BEMCHK
    *out = b;
    return NEP_OK;
}

int32_t nep_bem_info(const nep_bem* b, int64_t info[4]) {
    ARGCHK(b && info);
    info[0] = b->n;
    info[1] = b->gauss_order;
    info[2] = (int64_t)((size_t)b->n * (9 + 1 + 9 + 3 + BEM_NAUX + (size_t)b->n) * sizeof(double));
    info[3] = BEM_KMAX;
    return NEP_OK;
}

int32_t nep_bem_static(const nep_bem* b, double* d_out, int64_t ldo, nep_stream stream) {
    ARGCHK(b && d_out);
    ARGCHK(ldo >= b->n);
    HIPCHK(hipMemcpy2DAsync(d_out, (size_t)ldo * sizeof(double), b->S0, (size_t)b->n * sizeof(double), (size_t)b->n * sizeof(double),
                            (size_t)b->n, hipMemcpyDeviceToDevice, as_stream(stream)));
    return NEP_OK;
}

int32_t nep_bem_assemble(const nep_bem* b, int32_t nlam, const nep_cdouble* h_lam, int32_t der, nep_cdouble* dOut, int64_t ldo,
                         int64_t stride, nep_stream stream) {
    ARGCHK(b);
    ARGCHK(nlam >= 0 && der >= 0);
    if (nlam == 0) return NEP_OK;
    ARGCHK(h_lam && dOut);
    ARGCHK(ldo >= b->n && (nlam == 1 || stride >= ldo * (b->n - 1) + b->n));
    hipStream_t st = as_stream(stream);
    const unsigned tiles = (unsigned)((b->n + BEM_TILE - 1) / BEM_TILE);
    for (int32_t l0 = 0; l0 < nlam; l0 += BEM_LAM) {
        const int nl = nlam - l0 < BEM_LAM ? nlam - l0 : BEM_LAM;
        BemLams L;
        for (int l = 0; l < BEM_LAM; ++l) {
            L.re[l] = l < nl ? h_lam[l0 + l].re : 0.0;
            L.im[l] = l < nl ? h_lam[l0 + l].im : 0.0;
        }
        hipLaunchKernelGGL(k_bem_assemble, dim3(tiles, tiles), dim3(BEM_THREADS), 0, st, b->n, (const double*)b->gp,
                           (const double*)b->gw, (const double*)b->S0, L, nl, der, (cplx*)dOut + (int64_t)l0 * stride, ldo, stride);
        LAUNCHCHK();
    }
    return NEP_OK;
}

static int bem_apply(const nep_bem* b, const BemLams& L, int nbatch, int k, int sd, const nep_cdouble* h_a, const cplx* V,
                     int64_t ldv, int64_t vstride, cplx* out, int64_t ostride, hipStream_t st) {
    const unsigned rows = (unsigned)((b->n + BEM_ROWS - 1) / BEM_ROWS);
    for (int j1 = 0; j1 < k; j1 += BEM_KMAX) {           // passes of BEM_KMAX coefficients: pass 2 adds to the result of pass 1
        const int kk = k - j1 < BEM_KMAX ? k - j1 : BEM_KMAX;
        BemCoef A;
        for (int j = 0; j < BEM_KMAX; ++j) {
            A.re[j] = j < kk ? h_a[j1 + j].re : 0.0;
            A.im[j] = j < kk ? h_a[j1 + j].im : 0.0;
        }
        hipLaunchKernelGGL(k_bem_apply, dim3(rows, (unsigned)nbatch), dim3(BEM_THREADS), 0, st, b->n, (const double*)b->gp,
                           (const double*)b->gw, (const double*)b->S0, L, kk, sd + j1, A, V + (int64_t)j1 * ldv, ldv, vstride, out,
                           ostride, j1 > 0 ? 1 : 0);
        LAUNCHCHK();
    }
    return NEP_OK;
}

int32_t nep_bem_mlincomb(const nep_bem* b, nep_cdouble lam, int32_t k, const nep_cdouble* h_a, int32_t startder,
                         const nep_cdouble* dV, int64_t ldv, nep_cdouble* dz, nep_stream stream) {
    ARGCHK(b && h_a && dV && dz);
    ARGCHK(k >= 1 && startder >= 0 && ldv >= b->n);
    BemLams L;
    for (int l = 0; l < BEM_LAM; ++l) { L.re[l] = lam.re; L.im[l] = lam.im; }
    return bem_apply(b, L, 1, k, startder, h_a, (const cplx*)dV, ldv, 0, (cplx*)dz, 0, as_stream(stream));
}

int32_t nep_bem_resid(const nep_bem* b, int32_t k, const nep_cdouble* h_lam, const nep_cdouble* dQ, int64_t ldq, nep_cdouble* dOut,
                      int64_t ldo, nep_stream stream) {
    ARGCHK(b);
    ARGCHK(k >= 0);
    if (k == 0) return NEP_OK;
    ARGCHK(h_lam && dQ && dOut);
    ARGCHK(ldq >= b->n && ldo >= b->n);
    const nep_cdouble one = {1.0, 0.0};
    for (int32_t s0 = 0; s0 < k; s0 += BEM_LAM) {
        const int ns = k - s0 < BEM_LAM ? k - s0 : BEM_LAM;
        BemLams L;
        for (int l = 0; l < BEM_LAM; ++l) {
            L.re[l] = l < ns ? h_lam[s0 + l].re : 0.0;
            L.im[l] = l < ns ? h_lam[s0 + l].im : 0.0;
        }
        const int rc = bem_apply(b, L, ns, 1, 0, &one, (const cplx*)dQ + (int64_t)s0 * ldq, ldq, ldq, (cplx*)dOut + (int64_t)s0 * ldo,
                                 ldo, as_stream(stream));
        if (rc) return rc;
    }
    return NEP_OK;
}
