"""Cases, references, criteria and mutants for the device Hessenberg eigensolver (csrc/hesseig.hip: k_hess_qr, k_hess_invit).

Two references, both in correctly rounded float64 arithmetic:
  lapack   numpy.linalg.eig (zgeev: what the reference project's `eigen(H)` calls), vectors scaled to unit 2-norm and rotated so
           that the largest component is real positive;
  hq       hq_ref + invit_ref, a NumPy restatement of the kernels' algorithm: explicit single-shift QR on the active window,
           zlahqr's deflation test as negligible_sub writes it, the Wilkinson shift in the kernel's form, exceptional shifts at
           every 10th and 20th sweep of an eigenvalue, 30 max(10, k) sweeps per eigenvalue, the exact power-of-two scaling at load;
           zlaein's inverse iteration (U x = eps3 (1, ..., 1)^T, growth test, alternative start vectors, zhsein's perturbation).

Criteria.  unit(H) = k u ||H||_2 with u = 2^-53; H is the upper Hessenberg part of what is stored (entries below the first
subdiagonal are not part of the matrix).  Vector norms, residuals, sums and the Frobenius norm are evaluated in np.clongdouble;
||H||_2 and the sigma_min of C2 come from float64 SVDs (NumPy has no extended-precision SVD; their relative error of a few u does
not show in a bound that is a multiple of u itself).
  C1  families with a closed-form spectrum: the eigenvalues match the exact spectrum (long double) as multisets within c1 unit
  C2  sigma_min(H - lambda I) <= c2 unit for every returned lambda (at most ten of the cases with k > 64 carry it: k SVDs each)
  C3  |sum lambda - tr H| <= c3 k u ||H||_F (one eigenvalue written over another); random, gun and graded cases keep the multiset
      comparison with LAPACK at the tolerance tests/test_gpu_kernels.py asserts (1e-12 of the spectral radius; graded: 1e-9)
  C4  ||H z - lambda z||_2 <= c4 unit; | ||z||_2 - 1 | < 1e-14, largest component real positive to 1e-14 (as asserted before)
A vector whose inverse iteration failed is exactly zero and counted in w[k + 1]; only cases that say so may have one.

The constants.  They cannot be derived tightly, so they are measured on the two references over the final case list (never on
the device): largest value of each criterion in its own unit, times 8, rounded up to a power of two.  The device differs from hq
in reciprocals and reciprocal roots good to a few ulp, in FMA contraction and in the order of operations: each rotation departs
from orthogonality by a few u instead of about one and the departures add along the chain -- a factor below 4 is expected, 8
leaves a factor of two.  test_host_hesseig.py measures both references again on every host case and asserts value <= c / 8.

    largest value over the case list     lapack              hq                 times 8    constant
    C1                                   2.47 (cyclic_8)     1.00 (cyclic_2)    19.7       c1 = 32
    C2                                   2.46 (cyclic_8)     3.06 (gun_2)       24.4       c2 = 32
    C3                                   2.92 (real_3)       2.37 (gun_3)       23.4       c3 = 32
    C4                                   2.90 (cyclic_8)     4.62 (gun_3)       37.0       64, raised to c4 = 256 (below)
(hq's vectors for C4: invit_lapack, inverse iteration with LAPACK's LU on hq_ref's eigenvalues.)

c4 on the cyclic matrices.  With c4 = 64 the device passed every case but cyclic_64 (83.1 units) and cyclic_128 (78.3); its
eigenvalues there are off by 0.745 and 0.337 units (C1, bound 32).  The cause is zlaein's algorithm, not the device's arithmetic:
the start vector (1, ..., 1)^T is an eigenvector of the cyclic matrix and orthogonal to all its others, so the growth test fails
and the alternative start vectors are used, L is never applied, and on this matrix one step then leaves a residual of about 2 k
times the eigenvalue's error (in these units: 128 per unit at k = 64, 256 per unit at k = 128), where a vector routine that applies
L and picks its start vector leaves about once the error.  invit_ref, the float64 restatement of k_hess_invit, shows it: on
hq_ref's eigenvalues (0.19 and 0.17 units off) it gives 19.9 and 38.4 units, and fed the exact spectrum displaced radially by the
device's 0.745 and 0.337 units it gives 97.0 and 89.7 units (zlaein_level(); device: 83.1 and 78.3; the same at k = 8, 63, 127: 53.3,
64.9, 65.3 against the device's 48.7, 36.9, 40.4).  The correctly rounded algorithm reaches the device's level as soon as its
eigenvalues are as far off as the device's, which C1 allows; so c4 is the next power of two above twice that level, 2 * 97.0 = 194
-> 256.  The largest device value outside the cyclic family stays far below the first constant.
On the matrices tests/test_gpu_kernels.py already checks (gun, random k = 40 and k = 128, graded, zero) the residual tolerance
asserted there (1e-12 or 1e-13 of ||H||_F) is asserted beside C4 and the LAPACK comparison keeps its tolerance, so no bound on a
shared case is looser than before.

Exact cases need no constant: E1 (triangular Gaussian-integer matrices, eigenvalues = diagonal bit for bit in position order, no
sweep, also for 2^s H), E2 (w(2^s H) == 2^s w(H) and equal sweep counts bit for bit: the iteration sees only the scaled matrix
and smlnum), E3 (a decoupled block has the eigenvalues of the block alone bit for bit: only the window is transformed and the
arithmetic per element does not depend on the window's offset l).  The relations E2 and E3 compare two runs of one
implementation; check_scale_pair and check_blocks state them."""
import warnings
from functools import lru_cache

import numpy as np

C128 = np.complex128
LD, CLD = np.longdouble, np.clongdouble
U = 2.0 ** -53
ULP = 2.0 ** -52                 # dlamch('P'), the kernel's HQ_ULP
SAFMIN = 2.2250738585072014e-308
SENT = -7.0e77 - 3.0e77j         # initial value of result words: no result equals it
CONST = dict(c1=32.0, c2=32.0, c3=32.0, c4=256.0)
DEVICE_C1 = {"cyclic_64": 0.745, "cyclic_128": 0.337}       # the device's eigenvalue errors (units) where it passed 64 units of C4
RATIOS_BY_FAMILY = {}            # (criterion, family) -> the same
RATIOS = {}                      # criterion -> (largest value / bound, case) of everything evaluate() has seen


def cabs1(z):
    return np.abs(np.real(z)) + np.abs(np.imag(z))


def hess(H):
    return np.triu(np.asarray(H, dtype=C128), -1)


# ---- reference (b): the kernels' algorithm in NumPy -----------------------------------------------------------------------------
def _deflation_point(A, l, i, k, smlnum, ulp):
    """largest kk in (l, i] whose subdiagonal entry negligible_sub calls negligible, l if none"""
    kk = np.arange(l + 1, i + 1)
    sub = cabs1(A[kk, kk - 1])
    d1, d2 = A[kk - 1, kk - 1], A[kk, kk]
    tst = cabs1(d1) + cabs1(d2)
    zero = tst == 0.0
    if zero.any():
        lo = np.where(kk - 2 >= 0, cabs1(A[kk - 1, np.maximum(kk - 2, 0)]), 0.0)
        hi = np.where(kk + 1 <= k - 1, cabs1(A[np.minimum(kk + 1, k - 1), kk]), 0.0)
        tst = np.where(zero, lo + hi, tst)
    sup = cabs1(A[kk - 1, kk])
    ab, ba = np.maximum(sub, sup), np.minimum(sub, sup)
    a2, dd = cabs1(d2), cabs1(d1 - d2)
    aa, bb = np.maximum(a2, dd), np.minimum(a2, dd)
    with np.errstate(all="ignore"):
        s = aa + ab
        second = ba * (ab / s) <= np.maximum(smlnum, ulp * (bb * (aa / s)))
    neg = (sub <= smlnum) | ((sub <= ulp * tst) & second)
    hit = np.nonzero(neg)[0]
    return int(kk[hit[-1]]) if len(hit) else l


def _shift(A, l, i, kdefl, exceptional):
    if exceptional and kdefl % 20 == 0:
        return A[i, i] + 0.75 * cabs1(A[i, i - 1])
    if exceptional and kdefl % 10 == 0:
        return A[l, l] + 0.75 * cabs1(A[l + 1, l])
    t = A[i, i]
    u = np.sqrt(A[i - 1, i]) * np.sqrt(A[i, i - 1])
    s = cabs1(u)
    if s != 0.0:
        x = 0.5 * (A[i - 1, i - 1] - t)
        sx = cabs1(x)
        s = max(s, sx)
        y = s * np.sqrt((x / s) ** 2 + (u / s) ** 2)
        if sx > 0.0 and (x.real * y.real + x.imag * y.imag) < 0.0:
            y = -y
        den = x + y
        if den != 0.0:
            t = t - u * (u / den)
    return t


def hq_ref(H, mut=None):
    """eigenvalues of the upper Hessenberg part of H as k_hess_qr computes them -> (w, info, sweeps); mut: one of
    no_exceptional, deflate_sqrt_u, shift_not_restored, below_read"""
    H = np.asarray(H, dtype=C128)
    k = H.shape[0]
    A = H.copy() if mut == "below_read" else hess(H)
    stored = hess(H)
    with np.errstate(invalid="ignore"):
        amax = max(np.abs(stored.real).max(), np.abs(stored.imag).max())
    if not amax < np.inf:                                    # Inf / NaN at a stored entry: nothing to iterate on
        return np.zeros(k, dtype=C128), k, 0
    sexp = int(np.frexp(amax)[1]) if amax > 0.0 else 0
    A = np.ldexp(A.real, -sexp) + 1j * np.ldexp(A.imag, -sexp)
    smlnum = SAFMIN * (k / ULP)
    ulp = np.sqrt(ULP) if mut == "deflate_sqrt_u" else ULP
    itmax = 30 * max(10, k)
    info = sweeps = 0
    i = k - 1
    while i >= 0 and info == 0:
        l = kdefl = 0
        conv = False
        for _ in range(itmax + 1):
            l = _deflation_point(A, l, i, k, smlnum, ulp) if i > l else l
            if l > 0:
                A[l, l - 1] = 0.0
            if l >= i:
                conv = True
                break
            kdefl += 1; sweeps += 1
            t = _shift(A, l, i, kdefl, mut != "no_exceptional")
            n = i - l + 1
            Q, R = np.linalg.qr(A[l:i + 1, l:i + 1] - t * np.eye(n))
            W = R @ Q
            if mut != "shift_not_restored":
                W = W + t * np.eye(n)
            A[l:i + 1, l:i + 1] = W if mut == "below_read" else np.triu(W, -1)
        if not conv:
            info = i + 1
            break
        i = l - 1
    if info:
        return np.zeros(k, dtype=C128), info, sweeps
    d = np.diag(A)
    return np.ldexp(d.real, sexp) + 1j * np.ldexp(d.imag, sexp), 0, sweeps


def _convention(x):
    """unit 2-norm, largest component real positive"""
    x = np.asarray(x, dtype=CLD)
    big = x[np.argmax(np.abs(x))]
    nrm = np.sqrt(np.sum(np.abs(x) ** 2))
    return (x * (np.conj(big) / np.abs(big)) / nrm).astype(C128)


def _perturbed(w, eps3):
    """zhsein: an eigenvalue closer than eps3 to an earlier one is moved by eps3 until it is not (independent vectors)"""
    wk = np.array(w, dtype=C128)
    k = len(wk)
    for e in range(1, k):
        for _ in range(4 * k):
            if not (cabs1(wk[:e] - wk[e]) < eps3).any():
                break
            wk[e] = wk[e] + eps3
    return wk


def invit_ref(H, w):
    """right eigenvectors as k_hess_invit computes them (zhsein / zlaein) -> (Z, number of failed vectors); a failed vector is zero"""
    import scipy.linalg as sla
    Ht = hess(H)
    k = Ht.shape[0]
    if k == 1:
        return np.ones((1, 1), dtype=C128), 0
    hn = np.abs(Ht).sum(axis=1).max()
    smlnum = SAFMIN * (k / ULP)
    eps3 = hn * ULP if hn > 0.0 else smlnum
    wk = _perturbed(w, eps3)
    Z = np.zeros((k, k), dtype=C128)
    rootn = np.sqrt(k)
    failed = 0
    for e in range(k):
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            lu, _ = sla.lu_factor(Ht - wk[e] * np.eye(k), check_finite=False)
        Um = np.triu(lu)
        d = np.arange(k)
        Um[d, d] = np.where(Um[d, d] == 0.0, eps3, Um[d, d])
        b = np.full(k, eps3, dtype=C128)
        ok = False
        for its in range(1, k + 1):
            with np.errstate(all="ignore"):
                x = sla.solve_triangular(Um, b, check_finite=False)
            vn = cabs1(x).sum()
            if not vn < np.inf:
                break
            if vn >= 0.1 / rootn:
                ok = True
                break
            b = np.full(k, eps3 / (rootn + 1.0), dtype=C128); b[0] = eps3
            b[k - its] -= eps3 * rootn
        if ok:
            Z[:, e] = _convention(x)
        else:
            failed += 1
    return Z, failed


def invit_lapack(H, w):
    """inverse iteration with LAPACK's LU (zgetrf / zgetrs, L applied) on H - w_e I -> (Z, failed): one step from each of four
    fixed random start vectors, the result that grew most is kept (zlaein changes the start vector when the growth is poor; a
    second step does not help a non-normal matrix: the first result is nearly orthogonal to the left singular
    vector the next one would have to grow along); a zero pivot (an exact eigenvalue) is replaced by eps3 as in zlaein,
    coincident eigenvalues are perturbed as in zhsein, a solve that overflows gives a zero vector that is counted"""
    import scipy.linalg as sla
    Ht = hess(H)
    k = Ht.shape[0]
    hn = np.abs(Ht).sum(axis=1).max()
    eps3 = hn * ULP if hn > 0.0 else SAFMIN * (k / ULP)
    if k == 1:
        return np.ones((1, 1), dtype=C128), 0
    wk = _perturbed(w, eps3)
    failed = 0
    rng = np.random.default_rng(k)
    x0 = rng.standard_normal((k, 4)) + 1j * rng.standard_normal((k, 4))
    Z = np.zeros((k, k), dtype=C128)
    d = np.arange(k)
    for e in range(k):
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            lu, piv = sla.lu_factor(Ht - wk[e] * np.eye(k), check_finite=False)
        lu[d, d] = np.where(lu[d, d] == 0.0, eps3, lu[d, d])
        with np.errstate(all="ignore"):
            X = sla.lu_solve((lu, piv), x0, check_finite=False)
            x = X[:, int(np.argmax(np.nan_to_num(np.abs(X).max(axis=0), nan=np.inf)))]
        if np.all(np.isfinite(x)) and np.abs(x).max() > 0:
            Z[:, e] = _convention(x / np.abs(x).max())
        else:
            failed += 1
    return Z, failed


# ---- cases ----------------------------------------------------------------------------------------------------------------------
class Case:
    """H: the stored k x k array (its upper Hessenberg part is the matrix).  kind: criteria | exact_diag | nonfinite.
    exact: closed-form spectrum (clongdouble) or None.  c2: carries C2.  lapack_tol: multiset comparison with LAPACK, relative to
    the spectral radius, or None.  res_tol: the residual tolerance tests/test_gpu_kernels.py asserts on this matrix, relative to
    ||H||_F: asserted beside C4, so that no bound on a shared case is looser than before.  may_fail: vectors may be zero if counted.  min_sweeps: the kernel's algorithm needs at least
    so many sweeps.  diag: exact eigenvalues in position order (exact_diag).  extra: what a relation between runs needs."""

    def __init__(self, name, family, H, kind="criteria", exact=None, c2=None, lapack_tol=None, res_tol=None, may_fail=False, min_sweeps=0, diag=None,
                 host=True, **extra):
        self.name, self.family, self.H, self.kind, self.exact = name, family, np.asarray(H, dtype=C128), kind, exact
        self.k = self.H.shape[0]
        self.c2 = (self.k <= 64) if c2 is None else c2
        self.lapack_tol, self.res_tol, self.may_fail, self.min_sweeps, self.diag, self.host, self.extra = lapack_tol, res_tol, may_fail, min_sweeps, diag, host, extra

    def __repr__(self):
        return "%s(k=%d)" % (self.name, self.k)


SIZES = (2, 3, 8, 63, 64, 65, 66, 127, 128)
RSIZES = (2, 3, 63, 64, 65, 66, 127, 128)
C2_LARGE = ("cyclic_65", "cyclic_128", "toeplitz_65", "toeplitz_128", "random_65", "random_128", "real_66", "real_127", "gun_100",
            "grcar_65")                                             # the ten cases with k > 64 that carry C2
E1_SIZES, E1_SCALES = (1, 2, 64, 65, 128), (0, -900, -40, 40, 900)
E3_SPLITS = ((3, (1,)), (5, (2,)), (66, (1,)), (70, (5,)), (70, (6,)), (128, (30,)), (128, (64,)), (128, (1, 64, 127)))
TOEP_A, TOEP_B = 0.3 - 0.2j, 0.6 + 0.35j


def _pi():
    return 4 * np.arctan(LD(1))


def cyclic(k):
    H = np.zeros((k, k), dtype=C128)
    H[np.arange(1, k), np.arange(k - 1)] = 1.0
    H[0, k - 1] = 1.0
    th = 2 * _pi() * np.arange(k).astype(LD) / k
    return H, (np.cos(th) + 1j * np.sin(th)).astype(CLD)


def toeplitz(k):
    H = TOEP_A * np.eye(k, dtype=C128)
    H[np.arange(k - 1), np.arange(1, k)] = TOEP_B
    H[np.arange(1, k), np.arange(k - 1)] = -np.conj(TOEP_B)
    absb = np.sqrt(LD(TOEP_B.real) ** 2 + LD(TOEP_B.imag) ** 2)
    c = np.cos(np.arange(1, k + 1).astype(LD) * _pi() / (k + 1))
    return H, (CLD(TOEP_A) + 1j * (2 * absb * c)).astype(CLD)


def _crand(rng, k):
    return np.triu(rng.standard_normal((k, k)) + 1j * rng.standard_normal((k, k)), -1)


@lru_cache(None)
def shared_matrices():
    """the matrices of test_hess_eig_dev_edge_matrices (same generator, same order of draws): random k = 40, graded k = 40,
    defective k = 40, random k = 128"""
    rng = np.random.default_rng(7)
    k = 40
    A = _crand(rng, k)
    d = np.logspace(-6, 6, k)
    graded = np.triu((d[:, None] * A) / d[None, :] * 1.0, -1)
    defective = np.triu(A); defective[np.arange(k), np.arange(k)] = 2.0 + 1j
    rng = np.random.default_rng(7); _crand(rng, k)
    return dict(random40=A, graded=graded, defective=defective, random128=_crand(rng, 128))


@lru_cache(None)
def gun():
    import os
    return np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "gun_iar_H100.npy"))


def frank(k):
    i, j = np.indices((k, k))
    return np.where(j >= i - 1, k - np.maximum(i, j), 0).astype(C128)


def grcar(k):
    H = -np.eye(k, k, -1)
    for q in range(4):
        H = H + np.eye(k, k, q)
    return H.astype(C128)


def gauss_triangular(k, seed):
    """upper triangular, Gaussian-integer entries with |re|, |im| <= 8, distinct diagonal"""
    rng = np.random.default_rng(seed)
    T = np.triu(rng.integers(-8, 9, (k, k)) + 1j * rng.integers(-8, 9, (k, k))).astype(C128)
    grid = np.array([a + 1j * b for a in range(-8, 9) for b in range(-8, 9)])
    T[np.arange(k), np.arange(k)] = rng.permutation(grid)[:k]
    d = np.diag(T)
    assert len(set(d.tolist())) == k and np.abs(T.real).max() <= 8 and np.abs(T.imag).max() <= 8
    assert np.array_equal(T.real, np.round(T.real)) and np.array_equal(T.imag, np.round(T.imag)) and np.array_equal(T, np.triu(T))
    return T


def amax_exp(H):
    H = hess(H)
    return int(np.frexp(max(np.abs(H.real).max(), np.abs(H.imag).max()))[1])


def block_triangular(k, cuts, seed):
    """upper Hessenberg, H[p, p - 1] = 0 at every cut p; every diagonal block has max(|re|, |im|) = 0.9 (one binade) and the
    coupling blocks stay below it, so that H and each block alone get the same power-of-two scaling at load"""
    rng = np.random.default_rng(seed)
    H = _crand(rng, k)
    H = H / max(np.abs(H.real).max(), np.abs(H.imag).max()) * 0.8
    edges = (0,) + tuple(cuts) + (k,)
    blocks = []
    for a, b in zip(edges[:-1], edges[1:]):
        T = _crand(rng, b - a)
        T = T / max(np.abs(T.real).max(), np.abs(T.imag).max()) * 0.9
        H[a:b, a:b] = T
        if a > 0:
            H[a, a - 1] = 0.0
        blocks.append((a, b))
    e = amax_exp(H)
    for a, b in blocks:
        assert amax_exp(H[a:b, a:b]) == e == 0, (k, cuts, a, b)
        assert np.abs(H[:a, a:b].real).max(initial=0) < 0.9 and np.abs(H[:a, a:b].imag).max(initial=0) < 0.9
    assert all(H[p, p - 1] == 0 for p in cuts) and np.array_equal(H, np.triu(H, -1))
    return H, blocks


def scaled(H, s):
    return np.ldexp(H.real, s) + 1j * np.ldexp(H.imag, s)


def nonfinite(k, bad):
    H = _crand(np.random.default_rng(50 + k), k)
    H[k // 2, k // 2 + 1] = bad                                      # a stored entry above the diagonal
    return H


@lru_cache(None)
def cases():
    out = []
    for k in SIZES:
        H, ex = cyclic(k)
        out.append(Case("cyclic_%d" % k, "cyclic", H, exact=ex, min_sweeps=10 if k >= 3 else 0, c2=k <= 64 or "cyclic_%d" % k in C2_LARGE))
        H, ex = toeplitz(k)
        out.append(Case("toeplitz_%d" % k, "toeplitz", H, exact=ex, c2=k <= 64 or "toeplitz_%d" % k in C2_LARGE))
    for k in E1_SIZES:
        T = gauss_triangular(k, 100 + k)
        for s in E1_SCALES:
            out.append(Case("e1_tri_%d_s%+d" % (k, s), "e1", scaled(T, s), kind="exact_diag", diag=scaled(np.diag(T), s), may_fail=abs(s) > 40,
                            c2=k <= 64))
    sh = shared_matrices()
    for tag, M in (("random40", sh["random40"]), ("gun22", gun()[:22, :22]), ("random65", _crand(np.random.default_rng(2065), 65))):
        for s in (0, -40, 40):
            out.append(Case("e2_%s_s%+d" % (tag, s), "e2", scaled(M, s), lapack_tol=1e-12, res_tol=1e-13 if tag == "random40" else (1e-12 if tag == "gun22" else None),
                            c2=M.shape[0] <= 64, base="e2_%s_s+0" % tag, s=s))
    for k, cuts in E3_SPLITS:
        H, blocks = block_triangular(k, cuts, 300 + k + cuts[0])
        out.append(Case("e3_%d_%s" % (k, "_".join(map(str, cuts))), "e3", H, c2=k <= 64, blocks=blocks))
    for k in RSIZES:
        H = sh["random128"] if k == 128 else _crand(np.random.default_rng(1000 + k), k)
        out.append(Case("random_%d" % k, "random", H, lapack_tol=1e-12, res_tol=1e-13 if k == 128 else None, c2=k <= 64 or "random_%d" % k in C2_LARGE))
        H = np.triu(np.random.default_rng(2000 + k).standard_normal((k, k)), -1)
        out.append(Case("real_%d" % k, "random", H, lapack_tol=1e-12, c2=k <= 64 or "real_%d" % k in C2_LARGE))
    for k in (1, 2, 3, 17, 64, 65, 100):
        out.append(Case("gun_%d" % k, "gun", gun()[:k, :k], lapack_tol=1e-12, res_tol=1e-12, c2=k <= 64 or "gun_%d" % k in C2_LARGE))
    out.append(Case("grcar_65", "gallery", grcar(65), c2=True))
    out.append(Case("frank_12", "gallery", frank(12)))
    out.append(Case("frank_24", "gallery", frank(24)))
    out.append(Case("graded_40", "gallery", sh["graded"], lapack_tol=1e-9, res_tol=1e-12))
    out.append(Case("zero_40", "gallery", np.zeros((40, 40)), res_tol=1e-13))
    J = (1.0 + 0.5j) * np.eye(8, dtype=C128) + np.eye(8, 8, -1); J[0, 7] = 2.0 ** -40
    out.append(Case("jordan_8", "gallery", J))
    D = sh["defective"]
    out.append(Case("defective_40", "gallery", D, kind="exact_diag", diag=np.diag(D).copy(), may_fail=True))
    junk = gun()[:22, :22].copy()
    junk = junk + np.tril(_crand(np.random.default_rng(22), 22).T * 1e6, -2)
    out.append(Case("junk_below_22", "status", junk, lapack_tol=1e-12))
    out.append(Case("inf_5", "status", nonfinite(5, np.inf), kind="nonfinite"))
    out.append(Case("inf_70", "status", nonfinite(70, complex(1.0, -np.inf)), kind="nonfinite"))
    out.append(Case("nan_5", "status", nonfinite(5, np.nan), kind="nonfinite"))
    names = [c.name for c in out]
    assert len(set(names)) == len(names)
    assert sorted(c.name for c in out if c.k > 64 and c.c2) == sorted(C2_LARGE)
    return tuple(out)


def by_name(name):
    return next(c for c in cases() if c.name == name)


def iar_row_layout(H, m, poison):
    """the (m, m + 4) block of nep_iar_step: row j = column j of H (rows 0 .. j + 1), `poison` everywhere else"""
    k = H.shape[0]
    blk = np.full((m, m + 4), poison, dtype=C128)
    for j in range(k):
        blk[j, :min(j + 2, k)] = H[:min(j + 2, k), j]
    return blk


# ---- criteria -------------------------------------------------------------------------------------------------------------------
def _div(a, b):
    a, b = float(a), float(b)
    return a / b if b > 0.0 else (0.0 if a == 0.0 else np.inf)


def _match(w, ref):
    """greedy multiset matching -> distance of every w to its partner"""
    ref = np.asarray(ref, dtype=CLD)
    used = np.zeros(len(ref), bool)
    dist = np.zeros(len(w), dtype=LD)
    for q, x in enumerate(np.asarray(w, dtype=CLD)):
        d = np.abs(ref - x); d[used] = np.inf
        j = int(np.argmin(d)); used[j] = True; dist[q] = d[j]
    return dist


def measure(c, w, Z, cols=None):
    """the values of C1 .. C4 in their own units for the eigenvalues w and the vector columns `cols` of Z"""
    Ht = hess(c.H)
    k = c.k
    n2 = float(np.linalg.norm(Ht, 2)) if k > 1 else float(np.abs(Ht[0, 0]))
    unit = k * U * n2
    Hl = Ht.astype(CLD)
    wl = np.asarray(w, dtype=CLD)
    v = {}
    if c.exact is not None:
        v["c1"] = _div(_match(w, c.exact).max(), unit)
    if c.c2:
        sv = np.linalg.svd(Ht[None, :, :] - np.asarray(w)[:, None, None] * np.eye(k)[None, :, :], compute_uv=False)
        v["c2"] = _div(sv[:, -1].max(), unit)
    nF = np.sqrt(np.sum(np.abs(Hl) ** 2))
    v["c3"] = _div(np.abs(np.sum(wl) - np.trace(Hl)), k * U * nF)
    cols = np.arange(k) if cols is None else cols
    if len(cols):
        Zl = np.asarray(Z, dtype=CLD)[:, cols]
        R = Hl @ Zl - Zl * wl[cols][None, :]
        v["c4"] = _div(np.sqrt(np.sum(np.abs(R) ** 2, axis=0)).max(), unit)
        v["res_F"] = _div(np.sqrt(np.sum(np.abs(R) ** 2, axis=0)).max(), nF)
        v["norm"] = float(np.abs(np.sqrt(np.sum(np.abs(Zl) ** 2, axis=0)) - 1).max())
        # the largest component real positive; components tied with it in modulus to 1e-14 (the Fourier vectors of the cyclic
        # matrix, the symmetric sine vectors of the Toeplitz matrix) may stand for it: rounding decides which one is largest
        mod = np.abs(Zl)
        off = np.where((mod >= mod.max(axis=0) * (1 - 1e-14)) & (Zl.real > 0), np.abs(Zl.imag), np.inf)
        v["phase"] = float(off.min(axis=0).max())
    return v


@lru_cache(None)
def lapack(name):
    c = by_name(name)
    lam, V = np.linalg.eig(hess(c.H))
    return lam, np.stack([_convention(V[:, j]) for j in range(c.k)], axis=1)


def evaluate(c, wf, Z, kernel_algorithm=True, record=None):
    """every violated assertion of case c by the result words wf (k + 2: eigenvalues, (info, sweeps), (failed vectors, 0)) and the
    vectors Z (k, k), as a list of strings; with record=dict the measured values go there.  kernel_algorithm=False (LAPACK) leaves
    out what only the kernel's algorithm promises: the sweep counts and E1's bit-for-bit diagonal in position order"""
    k = c.k
    wf, Z = np.asarray(wf), np.asarray(Z)
    w, st0, st1 = wf[:k], wf[k], wf[k + 1]
    bad = []
    if c.kind == "nonfinite":
        if not (st0.real == k and (not kernel_algorithm or st0.imag == 0)):
            bad.append("status: w[k] = %r, want (%d, 0)" % (st0, k))
        if st1 != 0:
            bad.append("status: w[k+1] = %r, want 0" % st1)
        if not (np.all(w == 0) and np.all(Z == 0)):
            bad.append("status: eigenvalues / vectors of a refused matrix are not zero")
        return bad
    if not (np.all(np.isfinite(w)) and np.all(np.isfinite(Z))):
        return ["non-finite result"]
    zero = ~np.any(Z != 0, axis=0)
    sweeps = st0.imag
    if st0.real != 0:
        bad.append("status: w[k].real = %r (QR gave up)" % st0.real)
    if kernel_algorithm and not (sweeps == np.floor(sweeps) and sweeps >= c.min_sweeps and (c.kind != "exact_diag" or sweeps == 0)):
        bad.append("status: %r sweeps (at least %d%s)" % (sweeps, c.min_sweeps, ", exactly 0" if c.kind == "exact_diag" else ""))
    if not (st1.real == zero.sum() and st1.imag == 0):
        bad.append("status: w[k+1] = %r, %d zero vectors" % (st1, zero.sum()))
    if zero.any() and not c.may_fail:
        bad.append("%d vectors are zero" % zero.sum())
    if bad and st0.real != 0:
        return bad
    if kernel_algorithm and c.kind == "exact_diag" and not np.array_equal(w, c.diag):
        bad.append("E1: eigenvalues differ from the diagonal (first at %d)" % int(np.nonzero(w != c.diag)[0][0]))
    v = measure(c, w, Z, np.nonzero(~zero)[0])
    for key in ("c1", "c2", "c3", "c4"):
        if key in v:
            _note(key, v[key] / CONST[key], c)
            if not v[key] <= CONST[key]:
                bad.append("%s: %.3g units, bound %g" % (key.upper(), v[key], CONST[key]))
    if "norm" in v and not (v["norm"] < 1e-14 and v["phase"] < 1e-14):
        bad.append("C4 convention: | ||z|| - 1 | = %.3g, phase %.3g" % (v["norm"], v["phase"]))
    if c.res_tol is not None and "res_F" in v and not v["res_F"] <= c.res_tol:
        bad.append("C4 (earlier tolerance): %.3g ||H||_F, tolerance %g" % (v["res_F"], c.res_tol))
    if c.lapack_tol is not None:
        ref = lapack(c.name)[0]
        d = float(_match(w, ref).max()) / max(float(np.abs(ref).max()), 1e-300)
        v["lapack"] = d
        if not d <= c.lapack_tol:
            bad.append("C3 (LAPACK multiset): %.3g of the spectral radius, tolerance %g" % (d, c.lapack_tol))
    if record is not None:
        record.update(v)
    return bad


def _note(key, ratio, c):
    if ratio > RATIOS.get(key, (-1.0, None))[0]:
        RATIOS[key] = (float(ratio), c.name)
    if ratio > RATIOS_BY_FAMILY.get((key, c.family), (-1.0, None))[0]:
        RATIOS_BY_FAMILY[(key, c.family)] = (float(ratio), c.name)


def zlaein_level():
    """largest C4 value of invit_ref on cyclic_64 and cyclic_128 when it is fed the exact spectrum displaced radially by the
    eigenvalue error the device has there: the level the correctly rounded algorithm reaches with the device's eigenvalues"""
    level = 0.0
    for name, size in DEVICE_C1.items():
        c = by_name(name)
        w = c.exact.astype(C128) * (1 + size * c.k * U)
        Z, failed = invit_ref(c.H, w)
        assert failed == 0
        level = max(level, measure(c, w, Z)["c4"])
    return level


def check(c, wf, Z, **kw):
    bad = evaluate(c, wf, Z, **kw)
    assert not bad, (c, bad)


def check_scale_pair(c0, cs, wf0, wfs):
    """E2: w(2^s H) == 2^s w(H) and equal sweep counts, bit for bit"""
    s, k = cs.extra["s"], c0.k
    assert np.array_equal(wfs[:k], scaled(wf0[:k], s)), ("E2 eigenvalues", cs, int(np.sum(wfs[:k] != scaled(wf0[:k], s))))
    assert wfs[k] == wf0[k], ("E2 sweeps", cs, wfs[k], wf0[k])


def check_blocks(c, wfH, wf_blocks):
    """E3: the eigenvalues of a decoupled diagonal block of H are those of the block alone, bit for bit and in position"""
    for (a, b), wfb in zip(c.extra["blocks"], wf_blocks):
        assert wfb[b - a].real == 0, (c, a, b, wfb[b - a])
        assert np.array_equal(wfH[a:b], wfb[:b - a]), ("E3", c, (a, b), int(np.sum(wfH[a:b] != wfb[:b - a])))
    assert wfH[c.k].imag == sum(wfb[b - a].imag for (a, b), wfb in zip(c.extra["blocks"], wf_blocks)), ("E3 sweeps", c)


# ---- the references as implementations, and their mutants ----------------------------------------------------------------------------
IN_ALGORITHM = ("no_exceptional", "deflate_sqrt_u", "shift_not_restored", "below_read")
ON_OUTPUT = ("scale_not_undone", "one_conjugated", "one_overwritten", "columns_permuted", "z_rows_64_zero", "offset_ignored",
             "phase_wrong", "zeroed_not_counted", "status_initial")
MUTANTS = IN_ALGORITHM + ON_OUTPUT


@lru_cache(None)
def _hq(name, mut=None):
    c = by_name(name)
    w, info, sweeps = hq_ref(c.H, mut)
    if info:
        return w, info, sweeps, np.zeros((c.k, c.k), dtype=C128), 0
    return w, info, sweeps, None, 0


def reference(c, which, mut=None):
    """(wf, Z) of reference `which` on case c: lapack | hq (hq_ref's eigenvalues, vectors by inverse iteration with LAPACK) |
    hq_zlaein (hq_ref's eigenvalues, vectors by invit_ref), with mutant `mut` applied"""
    k = c.k
    if which == "lapack":
        w, Z = lapack(c.name)
        info = sweeps = failed = 0
    else:
        w, info, sweeps, Z, failed = _hq(c.name, mut if mut in IN_ALGORITHM else None)
        if Z is None:
            Z, failed = invit_ref(c.H, w) if which == "hq_zlaein" else invit_lapack(c.H, w)
    wf = np.concatenate([w, [complex(info, sweeps), complex(failed, 0)]]).astype(C128)
    Z = Z.copy()
    if mut == "scale_not_undone":
        wf[:k] *= 2
    elif mut == "one_conjugated":
        j = int(np.argmax(np.abs(wf[:k].imag))); wf[j] = np.conj(wf[j])
    elif mut == "one_overwritten" and k >= 2:
        wf[1] = wf[0]
    elif mut == "columns_permuted":
        Z = np.roll(Z, 1, axis=1)
    elif mut == "z_rows_64_zero":
        Z[64:, :] = 0
    elif mut == "offset_ignored" and "blocks" in c.extra:
        a, b = c.extra["blocks"][-1]
        wf[a:b] = hq_ref(c.H[:b - a, :b - a])[0]                     # the bottom window's eigenvalues from the window at l = 0
    elif mut == "phase_wrong":
        Z = Z * np.exp(0.1j)
    elif mut == "zeroed_not_counted":
        Z[:, k - 1] = 0
    elif mut == "status_initial":
        wf[k] = wf[k + 1] = SENT
    return wf, Z
