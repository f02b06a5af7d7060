"""Reference, error bounds and case list for the boundary-element NEP (csrc/bem.hip, nep_bem_*; nep_amd/bem.py).  Host only.

Everything is restated here in NumPy, generic in the element type T: the Fichera mesh (genmesh.jl), the 3-point Gauss rule
(precompute_quad!), the singular part S0 (deHoop.jl in the cancellation-free form, or in the reference's own form), the matrices
M^(der)(lam) (assemble_BEM.jl:40-85) and the matrix-free products.  T = np.longdouble is the reference; T = np.float64 is "the same
formulas in working precision", which has to pass every check (test_host_bem.py), as do the device kernels (test_gpu_bem.py).

Inputs of the comparison.  The vertices and areas are float64 data.  The Gauss points and weights are float64 data too: they are
DEFINED as g = (c0 P1 + c1 P2) + c2 P3 and w = area (1/3), every operation rounded to float64 (`gauss_f64`); the kernel forms them
with the same operations without contraction, so both sides start from the same bits and d_p == 0 means the same on both.

Bounds, componentwise, u = 2^-53.  Nothing is fitted to a device result.

S0.  |got - ref| <= C_S0 u A with
    A[r, c] = sum_g w_g (dist (Omega + rho) + sum_edges (|p| (|log| + 1) + |R_a| + |R_b|)) / (4 pi),  rho = |R1||R2||R3| / hypot(numer, denom).
Where the terms come from: dist Omega and |p| |log| are the terms themselves (relative errors); |p| * 1 is the error of the
logarithm caused by a relative error of its argument; dist rho is the error of 2 atan2(numer, denom), whose operands carry
absolute errors proportional to |R1||R2||R3| (the triple product and the denominator cancel); |R_a| + |R_b| carries the
ABSOLUTE errors of dist = |n.R1|, p = R_a.nu and s = R.tau (projections with cancellation: an error of a few u |R|, which in the
cancellation-free form enters the logarithm as 2 sqrt(2) u |R| / h times |p| <= h).  C_S0 = 64 counts the longest chain of
roundings from the float64 inputs to one of these quantities: the components of tau (difference, norm of 3 squares, division:
<= 6), of n (cross product of two such, norm, division: <= 19), of nu (<= 32), the scalar product with R (3 products, 2 sums and
R's own rounding: <= 6), |R| (<= 5), h^2 and its quotient (<= 8), log and atan2 (<= 2 each), the products with w and the sums
over 3 edges and 3 Gauss points (<= 8): no chain is longer than 64.  The float64 evaluation sits at 0.5 u A.  The term dist rho
is not in the shape the issue gave for A; it adds at most 4.1 % to an entry of A on the case meshes (static_part(with_rho=False)
gives A without it), and the float64 evaluation is at 0.0084 of the bound either way.

lam part of M^(der).  |got - ref| <= C_LAM(der) u sum_p W_p (1 + |lam| d_p) (|E_p| + [der = 0]) / d_p / (4 pi), E_p = (i d_p)^der
exp(i lam d_p), with C_LAM = 32 + 6 der: d_p from 3 differences, 3 squares, 2 sums and a square root (<= 4 u relative); the phase
Re(lam) d_p and the exponent Im(lam) d_p inherit 5 u |lam| d_p each, sincos and exp are taken as 2 ulp, the product of the two
adds 1: (10 |lam| d + 6) u on E; W_p / d_p: 6; d^der: 5 der; the fused accumulation of 9 terms: 9; the division by 4 pi: 2;
together at most 27 (1 + |lam| d) + 5 der.  The d == 0 pairs contribute i lam W and i W with 2 roundings.  The whole entry adds
the S0 bound (der = 0) and 2 u |M| for the last sum.

Matrix-free results.  z = sum_j a_j M^(j + sd) v_j: sum_j |a_j| (bound of M^(j + sd)) |v_j| for the entries, and
(n + 3 k + 16) u sum_j |a_j| T_j |v_j| for the products a_j v_j (3), the Horner recurrence (2 per step, k steps, on the absolute
values of its terms) and the sum over the n columns in any order; T_j[r, c] is the sum of the absolute values of the terms of
entry (r, c) of M^(j + sd).
"""
import numpy as np
from numpy.polynomial import chebyshev as ch

import interp_checkers as ic

LD, CLD = np.longdouble, np.clongdouble
U = 2.0 ** -53
C_S0 = 64.0
RATIOS = {}

LAM_REF = 8.790558462139456 - 0.010815457827738698j        # test/gallery.jl:181: M(LAM_REF) is singular at N = 1 (n = 96)
LAM_REF2 = 6.273640140401934 - 0.0022695823093037j         # the eigenvalue augnewton reaches from lam = 7
LAMS = [0.0, 1.0, 5 + 0.3j, LAM_REF.real - 0.0108j, 20 - 2j, 3 + 4j]
DERS = [0, 1, 2, 5]
MESH_SIZES = [1, 2, 63, 64, 65, 130]                        # the first n triangles of gen_mesh(4); plus the full n = 96 and n = 384
MLINCOMB = [(1, 0), (1, 1), (3, 0), (5, 1), (50, 1)]
BATCHES = [1, 3, 20]
MESHES = ["first%d" % n for n in MESH_SIZES] + ["full96", "full384"]


def c_lam(der):
    return 32.0 + 6.0 * der


# ---- mesh (genmesh.jl:12-92) ----------------------------------------------------------------------------------------------------
def gen_mesh(N):
    """(vert (n, 3, 3), area (n,)): the reference's loop nest over 15 patches, cells and 4 triangles per cell"""
    N += N % 2
    nn = N // 2
    grid = np.arange(N + 1) / N
    fix = [0, 1, 2] + [0] * 4 + [1] * 4 + [2] * 4
    val = [0, 0, 0] + [1, 1, 1, 0.5] * 3
    free = [(1, 2), (2, 0), (0, 1)] + [(1, 2)] * 4 + [(2, 0)] * 4 + [(0, 1)] * 4
    rng_lo, rng_hi = range(1, nn + 1), range(nn + 1, N + 1)
    quad = [(rng_lo, rng_lo), (rng_hi, rng_lo), (rng_lo, rng_hi), (rng_hi, rng_hi)]
    spans = [(range(1, N + 1),) * 2] * 3 + quad * 3
    first = [(0, 0, 1, 0), (1, 0, 1, 1), (1, 1, 0, 1), (0, 1, 0, 0)]
    later = [(0, 0, 0, 1), (0, 1, 1, 1), (1, 1, 1, 0), (1, 0, 0, 0)]
    out = []
    for l in range(15):
        f1, f2 = free[l]
        for ii in spans[l][0]:
            for jj in spans[l][1]:
                ctr = np.zeros(3); ctr[fix[l]] = val[l]
                ctr[f1] = (grid[ii - 1] + grid[ii]) / 2; ctr[f2] = (grid[jj - 1] + grid[jj]) / 2
                for a, b, c, d in (first if l < 3 else later):
                    P1 = np.zeros(3); P1[fix[l]] = val[l]; P3 = P1.copy()
                    P1[f1], P1[f2] = grid[ii + a - 1], grid[jj + b - 1]
                    P3[f1], P3[f2] = grid[ii + c - 1], grid[jj + d - 1]
                    out.append([P1, ctr, P3])
    vert = np.array(out)
    return vert, np.full(len(vert), 0.25 / N / N)


_MESH = {}


def mesh(name):
    """the case meshes: "firstK" = the first K triangles of gen_mesh(4), "full96" = gen_mesh(2), "full384" = gen_mesh(4)"""
    if name not in _MESH:
        if name == "full96":
            _MESH[name] = gen_mesh(2)
        else:
            v, a = gen_mesh(4)
            k = len(a) if name == "full384" else int(name[5:])
            _MESH[name] = (v[:k].copy(), a[:k].copy())
    return _MESH[name]


def on_surface(p):
    """p lies on the surface of the unit cube with the corner [1/2, 1]^3 removed"""
    x = np.asarray(p, dtype=float)
    if np.any(x < 0) or np.any(x > 1) or np.all(x > 0.5):
        return False
    outer = np.any(x == 0) or any(x[i] == 1 and not (x[(i + 1) % 3] > 0.5 and x[(i + 2) % 3] > 0.5) for i in range(3))
    inner = any(x[i] == 0.5 and x[(i + 1) % 3] >= 0.5 and x[(i + 2) % 3] >= 0.5 for i in range(3))
    return bool(outer or inner)


# ---- quadrature (assemble_BEM.jl:4-25) ------------------------------------------------------------------------------------------
def gauss_f64(vert, area):
    """(G (n, 3, 3) = [triangle, Gauss point, coordinate], Wt (n, 3)) in float64, every operation rounded on its own"""
    c = np.array([[2 / 3, 1 / 6, 1 / 6], [1 / 6, 2 / 3, 1 / 6], [1 / 6, 1 / 6, 2 / 3]])
    P1, P2, P3 = vert[:, 0, :], vert[:, 1, :], vert[:, 2, :]
    G = np.stack([(c[i, 0] * P1 + c[i, 1] * P2) + c[i, 2] * P3 for i in range(3)], axis=1)
    Wt = np.repeat((area * (1 / 3))[:, None], 3, axis=1)
    return G, Wt


def _pi(T):
    return T(4) * np.arctan(T(1))


def _unit(v):
    return v / np.sqrt(np.sum(v * v, axis=-1, keepdims=True))


def _dot(a, b):
    return np.sum(a * b, axis=-1)


def geometry(vert, T):
    """tangents, normal and edge normals (genmesh.jl:95-111) in type T"""
    P = vert.astype(T)
    tau = [_unit(P[:, 1] - P[:, 0]), _unit(P[:, 2] - P[:, 1]), _unit(P[:, 0] - P[:, 2])]
    nrm = _unit(np.cross(tau[0], tau[1]))
    nu = [_unit(np.cross(t, nrm)) for t in tau]
    return P, tau, nrm, nu


# ---- S0 (deHoop.jl, assemble_BEM.jl:78-79) --------------------------------------------------------------------------------------
def static_part(vert, area, T=LD, form="stable", mirror=True, scale=True, want_A=False, with_rho=True):
    """S0 (n x n, type T), and with want_A the magnitude A of the bound (float64).  form = "stable": |R| + s as h^2 / (|R| - s) for
    s < 0; "dehoop": the reference's expression.  mirror = False: both triangles computed with their own roles (a mutant);
    scale = False: without the 1 / (4 pi) (a mutant)."""
    n = len(area)
    G, Wt = gauss_f64(vert, area)
    P, tau, nrm, nu = geometry(vert, T)
    x = G.astype(T)[:, :, None, :]                                    # (r, g, 1, 3)
    R = [P[None, None, :, v, :] - x for v in range(3)]                # (r, g, c, 3)
    nR = [np.sqrt(_dot(Rv, Rv)) for Rv in R]
    q = _dot(nrm[None, None], R[0])
    dist = np.abs(q)
    numer = np.abs(R[0][..., 0] * R[1][..., 1] * R[2][..., 2] - R[0][..., 0] * R[1][..., 2] * R[2][..., 1]
                   + R[0][..., 1] * R[1][..., 2] * R[2][..., 0] - R[0][..., 1] * R[1][..., 0] * R[2][..., 2]
                   + R[0][..., 2] * R[1][..., 0] * R[2][..., 1] - R[0][..., 2] * R[1][..., 1] * R[2][..., 0])
    denom = (nR[0] * nR[1] * nR[2] + nR[0] * _dot(R[1], R[2]) + nR[1] * _dot(R[0], R[2]) + nR[2] * _dot(R[0], R[1]))
    solang = 2 * np.arctan2(numer, denom)
    solang = np.where(solang < 0, solang + 2 * _pi(T), solang)
    F = -dist * solang
    hyp = np.hypot(numer, denom)
    with np.errstate(divide="ignore", invalid="ignore"):
        rho = np.where(hyp > 0, nR[0] * nR[1] * nR[2] / hyp, 0)
    A = dist * (solang + (rho if with_rho else 0))             # with_rho = False: the magnitude without the atan2 operand term
    for e, (a, b) in enumerate(((0, 1), (1, 2), (2, 0))):
        p = _dot(R[a], nu[e][None, None])
        sa, sb = _dot(R[a], tau[e][None, None]), _dot(R[b], tau[e][None, None])
        with np.errstate(divide="ignore", invalid="ignore"):
            if form == "stable":
                h2 = p * p + q * q
                fa = np.where(sa >= 0, nR[a] + sa, h2 / (nR[a] - sa))
                fb = np.where(sb >= 0, nR[b] + sb, h2 / (nR[b] - sb))
                lg = np.where(h2 == 0, T(0), np.log(fb / fa))
            else:
                lg = np.log((nR[b] + sb) / (nR[a] + sa))
        F = F + p * lg
        A = A + np.abs(p) * (np.abs(lg) + 1) + nR[a] + nR[b]
    w = Wt.astype(T)[:, :, None]
    S = np.sum(w * F, axis=1) / (4 * _pi(T) if scale else 1)
    Am = np.sum(w * A, axis=1).astype(np.float64) / (4 * np.pi)
    if mirror:
        S = np.triu(S) + np.triu(S, 1).T
        Am = np.triu(Am) + np.triu(Am, 1).T
    return (S, Am) if want_A else S


# ---- M^(der)(lam) (assemble_BEM.jl:27-89) ---------------------------------------------------------------------------------------
class Pairs:
    """the 9 pairs of every entry r <= c: d (m, 3, 3) [entry, i, j], W = w_r[i] w_c[j], zero = (d == 0), in type T; m = n (n + 1) / 2"""

    def __init__(self, vert, area, T=LD):
        G, Wt = gauss_f64(vert, area)
        g, w = G.astype(T), Wt.astype(T)
        self.T, self.n = T, len(area)
        self.r, self.c = np.triu_indices(self.n)
        diff = g[self.r][:, :, None, :] - g[self.c][:, None, :, :]
        self.d = np.sqrt(np.sum(diff * diff, axis=-1))
        self.W = w[self.r][:, :, None] * w[self.c][:, None, :]
        self.zero = self.d == 0
        self.fourpi = 4 * _pi(T)
        self.CT = CLD if T is LD else np.complex128
        # d == 0 exactly for the same Gauss point of the same triangle, and nowhere else
        assert np.array_equal(self.zero, (self.r == self.c)[:, None, None] & np.eye(3, dtype=bool)[None])
        self._E, self._P = {}, {}
        self.d1 = np.where(self.zero, self.T(1), self.d)

    def power(self, lam, der):
        """(i d)^der exp(i lam d), der >= 1, continued from the last power kept for this shift when that one is lower"""
        k, P = self._P.get(lam, (0, None))
        if P is None or k > der:
            k, P = 0, self.expi(lam)
        while k < der:
            P = P * (1j * self.d1)
            k += 1
        self._P[lam] = (der, P)
        return P

    def full(self, vec):
        """the symmetric matrix with the upper triangle `vec`: the lower triangle is its mirror"""
        M = np.zeros((self.n, self.n), dtype=vec.dtype)
        M[self.r, self.c] = vec
        M[self.c, self.r] = vec
        return M

    def expi(self, lam):
        """exp(i lam d) = exp(-Im(lam) d) (cos, sin)(Re(lam) d), kept per shift"""
        if lam not in self._E:
            lr, li = self.T(lam.real), self.T(lam.imag)
            ex = np.exp(-li * self.d)
            self._E[lam] = (ex * np.cos(lr * self.d)) + 1j * (ex * np.sin(lr * self.d))
        return self._E[lam]

    def lam_part(self, lam, der, mut=None):
        """(L, Labs, Lbound), n x n and mirrored: the lam part of M^(der)(lam), the sum of the absolute values of its terms, and
        the sum that the bound multiplies"""
        lam = complex(lam)
        d1 = self.d1
        if der == 0:
            E = self.expi(lam) - (0 if mut == "no_minus_one" else 1)
            Ez = 1j * self.CT(lam) if mut != "zero_d0" else 0
            extra = 1.0
        else:
            E = self.power(lam, der)
            Ez = (1j if (der == 1 and mut != "zero_d1") else 0)
            extra = 0.0
        E = np.where(self.zero, Ez, E)
        aa = self.W / d1
        L = np.sum(E * aa, axis=(1, 2)) / self.fourpi
        mag = np.abs(E).astype(np.float64) + np.where(self.zero, 0.0, extra)
        aa64 = aa.astype(np.float64)
        Labs = np.sum(mag * aa64, axis=(1, 2)) / (4 * np.pi)
        Lb = np.sum(mag * aa64 * (1 + abs(lam) * self.d.astype(np.float64)), axis=(1, 2)) / (4 * np.pi)
        return self.full(L), self.full(Labs), self.full(Lb)


class Reference:
    """per mesh: S0 with its bound and, on demand, M^(der)(lam) with bound and term magnitudes; computed once, shared, read-only"""

    def __init__(self, name):
        self.name = name
        self.vert, self.area = mesh(name)
        self.n = len(self.area)
        self.S0, self.A = static_part(self.vert, self.area, LD, want_A=True)
        self.S0_bound = C_S0 * U * self.A
        self.pairs = Pairs(self.vert, self.area, LD)
        self._M = {}

    def mder(self, lam, der):
        """(M, bound, T): the matrix (clongdouble), its componentwise bound, the sum of absolute values of its terms"""
        key = (complex(lam), int(der))
        if key not in self._M:
            L, Labs, Lb = self.pairs.lam_part(lam, der)
            M = L + (self.S0 if der == 0 else 0)
            T = Labs + (np.abs(self.S0).astype(np.float64) if der == 0 else 0)
            b = c_lam(der) * U * Lb + (self.S0_bound if der == 0 else 0) + 2 * U * np.abs(M).astype(np.float64)
            for a in (M, T, b):
                a.setflags(write=False)
            self._M[key] = (M, b, T)
        return self._M[key]

    def mlincomb(self, lam, a, sd, V):
        """(z, bound, entry_bound) of z = sum_j a_j M^(j + sd)(lam) V[:, j]; columns with a_j == 0 are dropped (never read).  bound is
        the one of the matrix-free kernels; entry_bound, its first part, is the bound of the same sum formed in long double from
        matrices that are each within their own bound (assemble, then a product)"""
        n, k = self.n, len(a)
        z = np.zeros(n, dtype=CLD); b = np.zeros(n); t = np.zeros(n)
        for j in range(k):
            if a[j] == 0:
                continue
            M, Mb, T = self.mder(lam, j + sd)
            z += CLD(a[j]) * (M @ V[:, j].astype(CLD))
            b += abs(a[j]) * (Mb @ np.abs(V[:, j]))
            t += abs(a[j]) * (T @ np.abs(V[:, j]))
        return z, b + (n + 3 * k + 16) * U * t, b


_REF = {}


def reference(name):
    if name not in _REF:
        _REF[name] = Reference(name)
    return _REF[name]


def batch_lams(nlam):
    """the shifts of a batch: the six case shifts, cycled (so that the references are shared)"""
    return [LAMS[i % len(LAMS)] for i in range(nlam)]


def operands(name, k, sd):
    """(lam, a, V) of the mlincomb case (k, sd) on a mesh: a seeded block, zeros among the a_j where k >= 3, NaN columns there"""
    ref = reference(name)
    rng = np.random.default_rng(1000 * ref.n + 10 * k + sd)
    V = rng.standard_normal((ref.n, k)) + 1j * rng.standard_normal((ref.n, k))
    a = (rng.standard_normal(k) + 1j * rng.standard_normal(k)) / np.array([float(np.prod(np.arange(1, j + 1))) ** 0.5 for j in range(k)])
    if k >= 3:
        a[1::3] = 0
        V[:, 1::3] = np.nan
    lam = LAMS[(2 + k + sd) % len(LAMS)]
    return lam, a, V


# ---- checks ---------------------------------------------------------------------------------------------------------------------
def _ratio(kind, name, got, ref, bound):
    got = np.asarray(got)
    assert got.shape == ref.shape, (kind, name, got.shape, ref.shape)
    assert np.all(np.isfinite(got)), "%s %s: non-finite result" % (kind, name)
    err = np.abs(got.astype(CLD if np.iscomplexobj(ref) else LD) - ref).astype(np.float64)
    assert np.all(err[bound == 0] == 0), "%s %s: entries with a zero bound must be exact" % (kind, name)
    r = float(np.max(err[bound > 0] / bound[bound > 0])) if np.any(bound > 0) else 0.0
    RATIOS[kind] = max(RATIOS.get(kind, 0.0), r)
    assert r <= 1.0, "%s %s: |impl - ref| / bound = %.3g (largest error %.3e)" % (kind, name, r, float(err.max()))
    return r


def check_static(name, got):
    ref = reference(name)
    return _ratio("static", name, got, ref.S0, ref.S0_bound)


def check_mder(name, lam, der, got):
    M, b, _ = reference(name).mder(lam, der)
    return _ratio("assemble", "%s lam=%s der=%d" % (name, lam, der), got, M, b)


def check_mlincomb(name, lam, a, sd, V, got, kind="mlincomb"):
    z, b, _ = reference(name).mlincomb(lam, a, sd, V)
    return _ratio(kind, "%s lam=%s k=%d sd=%d" % (name, lam, len(a), sd), got, z, b)


# ---- the float64 evaluation of the same formulas, and its mutants -----------------------------------------------------------------
def eval_static(name, T=np.float64, **kw):
    v, a = mesh(name)
    return static_part(v, a, T, **kw)


_PAIRS64 = {}


def eval_mder(name, lam, der, T=np.float64, mut=None):
    """M^(der)(lam) in type T.  mut: "swapped" (lower triangle computed with the roles of the two triangles swapped instead of
    mirrored: the lam part is the same set of terms either way, the singular part is not), "zero_d0", "zero_d1", "no_minus_one",
    "s0_no_4pi" """
    v, a = mesh(name)
    if (name, T) not in _PAIRS64:
        _PAIRS64[(name, T)] = (Pairs(v, a, T), {})
    pr, s0 = _PAIRS64[(name, T)]
    skey = mut if mut in ("swapped", "s0_no_4pi") else None
    if skey not in s0:
        s0[skey] = static_part(v, a, T, mirror=mut != "swapped", scale=mut != "s0_no_4pi")
    return pr.lam_part(lam, der, mut)[0] + (s0[skey] if der == 0 else 0)


def eval_mlincomb(name, lam, a, sd, V, T=np.float64, shift=0):
    """sum_j a_j M^(j + sd + shift)(lam) V[:, j] from the assembled matrices in type T (shift = 1: the Horner mutant)"""
    n = len(mesh(name)[1])
    z = np.zeros(n, dtype=np.complex128)
    for j in range(len(a)):
        if a[j] != 0:
            z = z + a[j] * (eval_mder(name, lam, j + sd + shift, T) @ V[:, j])
    return z


# ---- NumPy drivers on the restatement: what the device drivers are compared with --------------------------------------------------
def mfun(name, T=np.float64):
    return lambda lam, der=0: np.asarray(eval_mder(name, lam, der, T), dtype=np.complex128)


def augnewton_numpy(M, lam, v, maxit=30, tol=1e-15):
    """augmented Newton (method_newton.jl:262-345) in NumPy; M(lam, der).  Returns (lam, v, steps)."""
    n = len(v)
    v = np.asarray(v, dtype=complex) / np.linalg.norm(v)
    c = v.copy()
    for it in range(1, maxit + 1):
        u = np.linalg.solve(M(lam), M(lam, 1) @ v)
        dl = (c.conj() @ v) / (c.conj() @ u)
        lam = lam - dl
        v = dl * u
        v = v / np.linalg.norm(v)
        if np.linalg.norm(M(lam) @ v) <= tol * np.linalg.norm(M(lam), 1) or abs(dl) <= tol * abs(lam):
            return lam, v, it
    return lam, v, maxit


def chebpep_numpy(M, k, a, b):
    """the NumPy ChebPEP of interp_checkers: coefficient matrices, and evaluators of the interpolant and its derivative"""
    Bv = ic.ref_cheb_coefficients(lambda x: M(x), k, a, b)

    def P(lam, der=0):
        x = 2 * (lam - a) / (b - a) - 1
        if der == 0:
            return ic.ref_cheb_eval(Bv, a, b, lam)
        return sum(ch.chebval(x, ch.chebder(np.eye(k)[i])) * (2 / (b - a)) * B for i, B in enumerate(Bv) if i >= 1)
    return Bv, P


def beyn_numpy(M, n, sigma, radius, N, k, seed=0, rank_tol=1e-8):
    """Beyn's integral method with the trapezoidal rule on the circle sigma + radius e^{it}, N nodes, k probe columns: the eigenvalues
    found inside the contour"""
    rng = np.random.default_rng(seed)
    Vh = rng.standard_normal((n, k)) + 0j
    A0 = np.zeros((n, k), dtype=complex); A1 = np.zeros((n, k), dtype=complex)
    for t in 2 * np.pi * np.arange(N) / N:
        g, gp = radius * np.exp(1j * t), 1j * radius * np.exp(1j * t)
        X = np.linalg.solve(M(sigma + g), Vh)
        A0 += X * gp / N; A1 += X * g * gp / N
    A0 /= 1j; A1 /= 1j
    Uv, s, Wh = np.linalg.svd(A0, full_matrices=False)
    p = int(np.sum(s > rank_tol * s[0]))
    B = Uv[:, :p].conj().T @ A1 @ Wh[:p].conj().T / s[:p][None, :]
    lam = sigma + np.linalg.eigvals(B)
    return lam[np.abs(lam - sigma) < radius]
