"""Reference, error bound and case list for the periodic-delay NEP (csrc/pdde.hip, nep_pdde_*; nep_amd/pdde.py).  Host only.

The integrator is restated here in NumPy on (real, imaginary) pairs, generic in the element type: np.longdouble is the reference,
np.float64 is "the same formulas in working precision" (it has to pass every check, test_host_pdde.py, as does the device,
test_gpu_pdde.py), and Python integers over a common power-of-two denominator are the exact evaluation of the exact cases.

    Out = Y_N - V,   Y_0 = V,   Y_{k+1} = Y_k + (s1 + 2 s2 + 2 s3 + s4) / 6,
    s1 = h F(2k, Y), s2 = h F(2k+1, Y + s1/2), s3 = h F(2k+1, Y + s2/2), s4 = h F(2k+2, Y + s3),
    F(row, Y) = (sum_i alpha[row, i] A_i) Y + ((sum_j beta[row, j] B_j) Y) E - Y S       (per system: E, S are p x p)

Exact cases.  A_i, B_j, E, V are Gaussian integers, the tables and S are 6 x (Gaussian integers), h = 1/4: every stage is 6 x
(dyadic), the division by 6 is exact, and `exact_case` PROVES, per case, that the float64 evaluation makes no rounding error: it
carries the same recurrence in integers over the denominator 2^DEN_BITS (every division is checked to leave no remainder) and
compares the float64 result, converted with fractions.Fraction, entry by entry.  A case that fails this is a test error, not a
device error.  E is NOT exp(-tau S) in these cases.  The device has to reproduce them byte for byte.

Bounded cases.  |got - ref| <= c u Ybar, entry by entry (moduli), u = 2^-53.  Ybar is the same recurrence on absolute values
(|A_i|, |B_j|, |E|, |S|, |alpha|, |beta|, |V|, every sign +), which majorises every intermediate of every evaluation order.
c = 4 N c_stage (1 + 1/64), c_stage = n + max(mA, mB) + 2 p + 21, counted per stage from the operation chain, relative to the majorant
of each quantity (a complex product costs 3 u: sqrt(5) u without fused operations; a sum of k terms k - 1 in any order):
    the table combination sum_i alpha_i A_i[r, k]        products 3, sums m - 1                          m + 2
    the inner sum over k of length n                     products 3, sums n - 1                          n + 2
    the right products with E and with S                 (products 3, sums p - 1, joining sum 1) x 2     2 p + 6
    E as an input (mder: formed by the library in closed form, exp 2, power and factorial 2)             4
    the product with h                                                                                   1
    the stage combination: Y + c K (1), s1 + 2 s2 + 2 s3 + s4 (3), / 6 (1), Y + . (1)                    6
An error already present in the stage input passes through the stage with the majorant's own factor, so the stage errors add up
along the chain of 4 N dependent stages; (1 + 1/64) covers the second-order terms (4 N c_stage u < 2^-30 on every case).
nep_pdde_mder multiplies column der by der!: the bound times der!, one more rounding in c.  Nothing is fitted to a device result.
"""
import math
from fractions import Fraction

import numpy as np

LD = np.longdouble
U = 2.0 ** -53
RATIOS = {}

MUTANTS = ["stage2_time", "s2_from_full_s1", "s3_from_s1", "weights_1111", "beta_from_alpha", "E_transposed", "E_on_A",
           "S_transposed", "YS_sign", "N_minus_1", "V_not_subtracted", "row_offset"]


# ---- the integrator on (re, im) pairs ---------------------------------------------------------------------------------------------
class CA:
    """a complex array as a pair of real arrays of any element type (float64, longdouble, Python int)"""

    def __init__(self, re, im):
        self.re, self.im = re, im

    @staticmethod
    def of(z, T):
        z = np.asarray(z, dtype=np.complex128)
        if T is int:
            conv = np.frompyfunc(lambda x: int(x), 1, 1)
            assert np.all(z.real == np.round(z.real)) and np.all(z.imag == np.round(z.imag))
            return CA(conv(z.real).astype(object), conv(z.imag).astype(object))
        return CA(z.real.astype(T), z.imag.astype(T))

    def __add__(self, o):
        return CA(self.re + o.re, self.im + o.im)

    def __sub__(self, o):
        return CA(self.re - o.re, self.im - o.im)

    def __mul__(self, o):                      # elementwise / broadcasting, complex x complex
        return CA(self.re * o.re - self.im * o.im, self.re * o.im + self.im * o.re)

    def rscale(self, c):                       # by a real scalar
        return CA(self.re * c, self.im * c)

    def __getitem__(self, k):
        return CA(self.re[k], self.im[k])

    def c128(self):
        return np.asarray(self.re, dtype=np.float64) + 1j * np.asarray(self.im, dtype=np.float64)


def _mm_real(M, Z):
    if M.dtype != object:
        return (M @ Z.reshape(Z.shape[0], -1)).reshape((M.shape[0],) + Z.shape[1:])
    out = np.zeros((M.shape[0],) + Z.shape[1:], dtype=object)           # sparse rows: the exact cases have few entries per row
    for r, k in zip(*np.nonzero(M)):
        out[r] = out[r] + M[r, k] * Z[k]
    return out


def _matmul(M, Z):
    return CA(_mm_real(M.re, Z.re) - _mm_real(M.im, Z.im), _mm_real(M.re, Z.im) + _mm_real(M.im, Z.re))


def _right(Y, R, transposed=False):
    """Y: (n, nsys, p), R: (nsys, p, p): out[:, s, :] = Y[:, s, :] R[s]  (R[s]^T when transposed)"""
    p = R.re.shape[1]
    out = None
    for q in range(p):
        Rq = CA(R.re[None, :, :, q], R.im[None, :, :, q]) if transposed else CA(R.re[None, :, q, :], R.im[None, :, q, :])
        t = CA(Y.re[:, :, q:q + 1], Y.im[:, :, q:q + 1]) * Rq
        out = t if out is None else out + t
    return out


def sweep(prob, S, E, V, T=np.float64, mutant=None, majorant=False):
    """Out (n, nsys, p) as a CA of element type T.  prob: dict(A (mA, n, n), B (mB, n, n), alpha (2N+1, mA), beta (2N+1, mB), N,
    h); S, E: (nsys, p, p); V: (n, nsys, p).  T = int: every value is carried as an integer over 2^DEN_BITS.  majorant: all inputs
    replaced by their moduli and every sign +; returns Ybar_N (a real array) instead."""
    N, h = prob["N"], prob["h"]
    if majorant:
        A, B, al, be = (CA(np.abs(prob[k]), np.zeros(prob[k].shape)) for k in ("A", "B", "alpha", "beta"))
        S, E, V = (CA(np.abs(x), np.zeros(np.shape(x))) for x in (S, E, V))
        sgn = 1.0
    else:
        A, B, al, be = (CA.of(prob[k], T) for k in ("A", "B", "alpha", "beta"))
        S, E, V = CA.of(S, T), CA.of(E, T), CA.of(V, T)
        sgn = -1
    if T is int:
        V = V.rscale(1 << DEN_BITS)
        hnum, hden = Fraction(h).numerator, Fraction(h).denominator

        def div(X, d):
            assert all(x % d == 0 for x in X.re.ravel()) and all(x % d == 0 for x in X.im.ravel()), "inexact division by %d" % d
            return CA(X.re // d, X.im // d)
        times_h = lambda X: div(X.rscale(hnum), hden)
        half = lambda X: div(X, 2)
        div6 = lambda X: div(X, 6)
    else:
        hT = h if majorant else T(h)
        times_h = lambda X: X.rscale(hT)
        half = lambda X: X.rscale(0.5 if majorant else T(0.5))
        div6 = lambda X: CA(X.re / 6, X.im / 6) if majorant else CA(X.re / T(6), X.im / T(6))
    mA, mB = A.re.shape[0], B.re.shape[0]
    rows = 2 * N + 1

    def comb(M, tab, row, cols):
        out = None
        for i in range(M.re.shape[0]):
            c = cols[i]
            t = M[i] * CA(tab.re[row, c], tab.im[row, c])
            out = t if out is None else out + t
        return out

    def F(row, Y):
        if mutant == "row_offset":
            row = (row + 1) % rows
        At = comb(A, al, row, range(mA))
        Bt = comb(B, al, row, [j % mA for j in range(mB)]) if mutant == "beta_from_alpha" else comb(B, be, row, range(mB))
        AY, BY = _matmul(At, Y), _matmul(Bt, Y)
        if mutant == "E_on_A":
            AY, BY = BY, AY
        YS = _right(Y, S, transposed=(mutant == "S_transposed"))
        if sgn < 0 and mutant != "YS_sign":
            YS = YS.rscale(-1)
        return times_h(AY + _right(BY, E, transposed=(mutant == "E_transposed")) + YS)

    Y = V
    for k in range(N - 1 if mutant == "N_minus_1" else N):
        s1 = F(2 * k, Y)
        s2 = F(2 * k + (2 if mutant == "stage2_time" else 1), Y + (s1 if mutant == "s2_from_full_s1" else half(s1)))
        s3 = F(2 * k + 1, Y + half(s1 if mutant == "s3_from_s1" else s2))
        s4 = F(2 * k + 2, Y + s3)
        if mutant == "weights_1111":
            Y = Y + div6(((s1 + s2) + s3) + s4)
        else:
            Y = Y + div6(((s1 + s2.rscale(2)) + s3.rscale(2)) + s4)
    if majorant:
        return Y.re
    return Y if mutant == "V_not_subtracted" else Y - V


def abs_err(got, ref):
    """|got - ref| entry by entry in long double; got complex128 array, ref a CA of long doubles"""
    return np.hypot(got.real.astype(LD) - ref.re, got.imag.astype(LD) - ref.im).astype(np.float64)


# ---- cases ------------------------------------------------------------------------------------------------------------------------
NS = [1, 2, 3, 15, 16, 17, 63, 64, 65, 130]
DEN_BITS = 40                                   # 2 bits per stage (h = 1/4), 12 stages at most, one more for the half steps

# (n, p, nsys, N, mA, mB): every value of every list of the issue at least once; every n with p = 3 and nsys = 20
SHAPES = [(n, 3, 20, 1, 2, 1) for n in NS] + [
    (2, 1, 1, 3, 1, 1), (3, 2, 3, 2, 3, 2), (16, 8, 3, 1, 1, 1), (17, 1, 20, 2, 3, 2), (64, 2, 1, 1, 2, 1), (65, 8, 1, 1, 3, 2),
    (130, 1, 3, 1, 1, 1), (15, 2, 20, 1, 3, 2), (63, 1, 1, 2, 2, 1), (1, 8, 3, 3, 1, 1),
    (3, 3, 513, 1, 2, 1), (2, 1, 2049, 1, 1, 1)]        # batches of 257 tiles of 2 and of 8 systems, the last tile partly filled


def case_id(shape):
    return "n%d-p%d-s%d-N%d-m%d%d" % shape


def _gauss_units(rng, shape, density):
    """Gaussian integers with entries in {0, +-1, +-i}, about `density` of them nonzero"""
    units = np.array([1, -1, 1j, -1j])
    return np.where(rng.random(shape) < density, units[rng.integers(0, 4, shape)], 0)


def _sparse_rows(rng, m, n, per_row):
    M = np.zeros((m, n, n), dtype=np.complex128)
    units = np.array([1, -1, 1j, -1j])
    for i in range(m):
        for r in range(n):
            for k in rng.choice(n, size=min(per_row, n), replace=False):
                M[i, r, k] = units[rng.integers(0, 4)]
    return M


_EXACT = {}


def exact_case(shape):
    """(prob, S, E, V, ref complex128 (n, nsys, p)) with the proof that float64 evaluates it without rounding"""
    if shape in _EXACT:
        return _EXACT[shape]
    n, p, nsys, N, mA, mB = shape
    rng = np.random.default_rng(hash(shape) % (1 << 31))
    few = N == 1
    prob = dict(N=N, h=0.25, tau=0.25 * N,
                A=_sparse_rows(rng, mA, n, 2 if few else 1), B=_sparse_rows(rng, mB, n, 2 if few else 1),
                alpha=6.0 * _gauss_units(rng, (2 * N + 1, mA), 0.8 if few else 0.6),
                beta=6.0 * _gauss_units(rng, (2 * N + 1, mB), 0.8 if few else 0.6))
    prob["alpha"][0, 0] = 6.0                                            # the first stage never vanishes
    S = 6.0 * _gauss_units(rng, (nsys, p, p), (0.6 if few else 0.3) / p)
    E = _gauss_units(rng, (nsys, p, p), 1.0 / p if not few else min(1.0, 2.0 / p))
    S[0, 0, 0], E[0, 0, 0] = 6.0, -1j                                     # E is not exp(-tau S): the two cannot be confused
    V = _gauss_units(rng, (n, nsys, p), 0.7) * rng.integers(1, 4, (n, nsys, p))
    f64 = sweep(prob, S, E, V, np.float64)
    ex = sweep(prob, S, E, V, int)
    den = 1 << DEN_BITS
    same = all(Fraction(float(a)) == Fraction(int(b), den) for a, b in zip(f64.re.ravel(), ex.re.ravel())) and \
        all(Fraction(float(a)) == Fraction(int(b), den) for a, b in zip(f64.im.ravel(), ex.im.ravel()))
    if not same:
        raise AssertionError("exact case %s: the float64 evaluation is not exact; the case has to be made smaller" % case_id(shape))
    _EXACT[shape] = (prob, S, E, V, f64.c128())
    return _EXACT[shape]


def mutant_differs(shape, mutant):
    prob, S, E, V, ref = exact_case(shape)
    return not np.array_equal(sweep(prob, S, E, V, np.float64, mutant=mutant).c128(), ref)


# ---- bounded cases ----------------------------------------------------------------------------------------------------------------
BOUNDED_SHAPES = [(1, 1, 1, 7, 1, 1), (2, 2, 3, 7, 2, 1), (3, 3, 20, 2, 3, 2), (15, 8, 3, 2, 2, 1), (16, 3, 20, 1, 1, 1),
                  (17, 1, 20, 7, 3, 2), (63, 2, 3, 2, 2, 1), (64, 3, 20, 1, 3, 2), (65, 1, 3, 7, 1, 1), (130, 3, 20, 1, 2, 1),
                  (130, 8, 1, 2, 3, 2),
                  (257, 2, 3, 1, 1, 1), (512, 8, 1, 1, 2, 1),          # more than 256 rows; the largest tile in LDS (128 KiB)
                  (3, 3, 513, 1, 2, 1), (2, 2, 1025, 2, 1, 1), (2, 1, 2049, 1, 1, 1), (17, 4, 513, 1, 1, 1)]
# (the last four: V from memory in tiles of 2, 4, 8 and 2 systems -- a batch has to give 256 tiles before tiles are widened -- with
# the last tile partly filled)


def c_bound(n, p, N, mA, mB):
    return 4.0 * N * (n + max(mA, mB) + 2 * p + 21) * (1 + 1 / 64)


def _unit_norm(rng, shape):
    M = rng.standard_normal(shape) + 1j * rng.standard_normal(shape)
    return M / np.linalg.norm(M, 2)


def expm_ld(X, terms=60):
    """exp(X) for a small matrix in long double: scaling by 2^-8, Taylor series, 8 squarings"""
    Xr = X.real.astype(LD) / 256; Xi = X.imag.astype(LD) / 256
    p = X.shape[0]
    Tr, Ti = np.eye(p, dtype=LD), np.zeros((p, p), dtype=LD)
    Rr, Ri = Tr.copy(), Ti.copy()
    for k in range(1, terms):
        Tr, Ti = (Tr @ Xr - Ti @ Xi) / k, (Tr @ Xi + Ti @ Xr) / k
        Rr, Ri = Rr + Tr, Ri + Ti
    for _ in range(8):
        Rr, Ri = Rr @ Rr - Ri @ Ri, Rr @ Ri + Ri @ Rr
    return Rr, Ri


_BOUNDED = {}


def bounded_case(shape):
    """(prob, S, E, V, ref CA of long doubles, bound float64): random complex terms of 2-norm 1, S = lam I + (strictly upper part
    of norm <= 1/2) with |lam| <= 3, E = exp(-tau S) rounded to float64, tau = 1/2"""
    if shape in _BOUNDED:
        return _BOUNDED[shape]
    n, p, nsys, N, mA, mB = shape
    rng = np.random.default_rng(1000 + hash(shape) % (1 << 30))
    tau = 0.5
    prob = dict(N=N, h=tau / N, tau=tau, A=np.stack([_unit_norm(rng, (n, n)) for _ in range(mA)]),
                B=np.stack([_unit_norm(rng, (n, n)) for _ in range(mB)]),
                alpha=(rng.standard_normal((2 * N + 1, mA)) + 1j * rng.standard_normal((2 * N + 1, mA))) / np.sqrt(2 * mA),
                beta=(rng.standard_normal((2 * N + 1, mB)) + 1j * rng.standard_normal((2 * N + 1, mB))) / np.sqrt(2 * mB))
    S = np.zeros((nsys, p, p), dtype=np.complex128)
    E = np.zeros_like(S)
    for s in range(nsys):
        lam = 3 * np.sqrt(rng.random()) * np.exp(2j * np.pi * rng.random())
        up = np.triu(rng.standard_normal((p, p)) + 1j * rng.standard_normal((p, p)), 1)
        S[s] = lam * np.eye(p) + (0.5 * up / max(np.linalg.norm(up, 2), 1e-300) if p > 1 else 0)
        er, ei = expm_ld(-tau * S[s])
        E[s] = er.astype(np.float64) + 1j * ei.astype(np.float64)
    V = rng.standard_normal((n, nsys, p)) + 1j * rng.standard_normal((n, nsys, p))
    ref = sweep(prob, S, E, V, LD)
    bound = c_bound(n, p, N, mA, mB) * U * sweep(prob, S, E, V, majorant=True)
    _BOUNDED[shape] = (prob, S, E, V, ref, bound)
    return _BOUNDED[shape]


def check_bounded(shape, got, what):
    """the largest |got - ref| / bound; asserts it is <= 1 and records it in RATIOS[what]"""
    prob, S, E, V, ref, bound = bounded_case(shape)
    r = float(np.max(abs_err(np.asarray(got).reshape(ref.re.shape), ref) / bound))
    RATIOS[what] = max(RATIOS.get(what, 0.0), r)
    assert r <= 1.0, "%s %s: %.3g of the bound" % (what, case_id(shape), r)
    return r


# ---- M^(der)(lam) through Jordan blocks -------------------------------------------------------------------------------------------
def jordan_ld(lam, p, tau):
    """S = J_p(lam) and E = e^(-tau lam) Toeplitz((-tau)^k / k!) (float64-rounded from a long double evaluation)"""
    S = complex(lam) * np.eye(p, dtype=np.complex128) + np.diag(np.ones(p - 1), 1)
    er, ei = expm_ld(-tau * S)
    return S, er.astype(np.float64) + 1j * ei.astype(np.float64)


def mder_sweep(prob, lam, der, T=np.float64, majorant=False):
    """M^(der)(lam) (n x n) = der! x column der of the systems V = [e_j, 0, ..., 0], S = J_(der+1)(lam); CA of type T (majorant:
    der! Ybar, a real array)"""
    n, p = prob["A"].shape[1], der + 1
    S, E = jordan_ld(lam, p, prob["tau"])
    V = np.zeros((n, n, p), dtype=np.complex128)
    V[np.arange(n), np.arange(n), 0] = 1
    S, E = np.repeat(S[None], n, 0), np.repeat(E[None], n, 0)
    f = math.factorial(der)
    if majorant:
        return f * sweep(prob, S, E, V, majorant=True)[:, :, der]
    out = sweep(prob, S, E, V, T)
    return CA(out.re[:, :, der] * T(f), out.im[:, :, der] * T(f))


def mder_bound(prob, lam, der):
    n, mA, mB = prob["A"].shape[1], prob["A"].shape[0], prob["B"].shape[0]
    return (c_bound(n, der + 1, prob["N"], mA, mB) + 1) * U * mder_sweep(prob, lam, der, majorant=True)


def problem_of(nep):
    """the checker's view of a nep_amd PeriodicDDE_NEP: its terms and tables"""
    return dict(N=nep.N, h=nep.tau / nep.N, tau=nep.tau, A=nep.A_terms, B=nep.B_terms, alpha=nep.alpha, beta=nep.beta)


def mfun(prob):
    """lam, der -> M^(der)(lam) as a complex128 matrix (the float64 evaluation)"""
    return lambda lam, der=0: mder_sweep(prob, lam, der).c128()


# ---- Beyn's method and Newton polishing in NumPy (the rand0 fixture) --------------------------------------------------------------
def beyn_numpy(M, n, sigma, radius, N, k, seed=0, tol_rank=1e-8):
    rng = np.random.default_rng(seed)
    Vh = rng.standard_normal((n, k)) + 1j * rng.standard_normal((n, k))
    A0 = np.zeros((n, k), dtype=complex); A1 = np.zeros((n, k), dtype=complex)
    for j in range(N):
        w = np.exp(2j * np.pi * (j + 0.5) / N)
        X = np.linalg.solve(M(sigma + radius * w), Vh)
        A0 += X * (radius * w / N); A1 += X * (radius * w / N) * (radius * w)
    Uu, s, Wh = np.linalg.svd(A0, full_matrices=False)
    r = int(np.sum(s > tol_rank * s[0]))
    Bm = Uu[:, :r].conj().T @ A1 @ Wh[:r].conj().T / s[:r]
    ev, X = np.linalg.eig(Bm)
    return sigma + ev, Uu[:, :r] @ X


def newton_polish(M, lam, v, tol=1e-13, maxit=20):
    """Newton on [M(lam) v; c^H v - 1] from (lam, v) until |dlam| <= tol (1 + |lam|)"""
    n = len(v)
    c = v / np.vdot(v, v)
    for _ in range(maxit):
        J = np.zeros((n + 1, n + 1), dtype=complex)
        J[:n, :n] = M(lam); J[:n, n] = M(lam, 1) @ v; J[n, :n] = c.conj()
        d = -np.linalg.solve(J, np.concatenate([J[:n, :n] @ v, [np.vdot(c, v) - 1]]))
        v = v + d[:n]; lam = lam + d[n]
        if abs(d[n]) <= tol * (1 + abs(lam)):
            return lam, v
    raise AssertionError("newton_polish did not converge")


RAND0 = dict(n=24, N=64)
# chosen on the CPU: the disc holds 5 eigenvalues, the farthest 0.142 from the centre, the nearest outside 0.245 (rand0_eigs checks
# the count and the margin of 0.05); (0.194 / 0.245)^128 = 1e-13 is what the trapezoidal rule lets in from outside with 128 nodes.
# The problem has no real eigenvalue in [-1, 3] (det M(x) keeps its sign there), nor has the disc: the ChebPEP test runs on
# "mathieu", whose eigenvalue -0.2447... is real.
RAND0_DISC = dict(sigma=0.08 + 0.76j, radius=0.194)
RAND0_NODES = 128


def rand0_eigs(prob, sigma, radius, nodes=RAND0_NODES, k=12):
    """the eigenvalues of the problem inside the disc, polished, sorted by (real, imag); asserts 3 .. 8 of them and none within
    0.05 of the circle (for the raw Beyn values inside and outside alike)"""
    M = mfun(prob)
    n = prob["A"].shape[1]
    ev, X = beyn_numpy(M, n, sigma, radius, nodes, k, tol_rank=1e-6)
    out = []
    for l, x in zip(ev, X.T):
        if abs(l - sigma) < radius + 0.05:
            assert abs(abs(l - sigma) - radius) > 0.05, "an eigenvalue within 0.05 of the contour: %r" % l
            lp, _ = newton_polish(M, l, x)
            assert abs(lp - l) < 1e-4, (l, lp)
            if not any(abs(lp - o) < 1e-9 for o in out):
                out.append(lp)
    assert 3 <= len(out) <= 8, out
    return np.array(sorted(out, key=lambda z: (round(z.real, 9), z.imag)))


def rand0_problem():
    """the checker's view of nep_gallery("periodicdde", name="rand0", n=24, N=64) (built on the host, no device)"""
    from nep_amd.gallery import nep_gallery
    return problem_of(nep_gallery("periodicdde", name="rand0", **RAND0))
