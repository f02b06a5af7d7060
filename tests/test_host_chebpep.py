"""Host-side tests of the ChebPEP feature: the checker that test_gpu_chebpep.py runs on nep_interp_coeffs (it passes the NumPy
implementation and rejects its mutants), funcs.Chebyshev against numpy.polynomial.chebyshev, the Chebyshev weight table, the
colleague pencil and the companion form."""
import os
import re
from functools import partial
from itertools import product

import numpy as np
import pytest
import scipy.linalg as sla
from numpy.polynomial import chebyshev as ch

import nep_amd as na
from nep_amd import funcs
import interp_checkers as ic
import primitive_checkers as pc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = np.finfo(float).eps


# ---- the checker of nep_interp_coeffs -------------------------------------------------------------------------------------------
def test_numpy_implementation_passes_every_case():
    n = 0
    for c in ic.INTERP.cases():
        ic.INTERP.check(ic.INTERP.ref, c)
        n += 1
    assert n == len(ic.IP_E) * len(ic.IP_JK) * 2 * 2 * 3 * 2 == 1152
    print("%s: %d cases, largest |impl - ref| / bound = %.3g" % (ic.INTERP.name, n, pc.RATIOS.get(ic.INTERP.name, 0.0)))


@pytest.mark.parametrize("mut", ic.INTERP.mutants)
def test_checker_rejects_mutant(mut):
    """W transposed, W conjugated, the first row of W doubled (a lost halving of the Chebyshev table), beta ignored, the row map
    ignored, the last entry not written, the value behind a row written, a real F read as complex, one real part off by one ulp:
    some case fails on each"""
    ratios = dict(pc.RATIOS)
    impl = partial(ic.INTERP.ref, mut=mut)
    rejected = None
    for c in ic.INTERP.cases():
        if mut in ic.INTERP.exact_only_mutants and c.kind != "exact":
            continue
        try:
            ic.INTERP.check(impl, c)
        except AssertionError:
            rejected = c
            break
    pc.RATIOS.clear(); pc.RATIOS.update(ratios)
    assert rejected is not None, "no case rejects the mutant %r" % mut


def test_case_list_is_the_product_and_both_kinds_meet_every_pair_of_values():
    sh = list(ic.INTERP.shapes())
    assert [s[:7] for s in sh] == [(E, J, K, c, b, p, d) for E, (J, K), c, b, p, d in
                                   product(ic.IP_E, ic.IP_JK, (False, True), (0, 1), ic.IP_POS, (False, True))]
    seen = {}
    for s in sh:
        vals = (s[0], (s[1], s[2]), s[3], s[4], s[5], s[6])
        for i in range(len(vals)):
            for j in range(i + 1, len(vals)):
                seen.setdefault((i, vals[i], j, vals[j]), set()).add(s[7])
    assert all(v == {"exact", "rounded"} for v in seen.values())
    # the injection leaves rows of C untouched, the paddings exist
    assert ic.InterpCoeffs.rows_of(65, "inject") > 65 and ic.PAD_F > 0 and ic.PAD_C > 0


def test_symbol_is_declared_bound_and_wrapped():
    hdr = open(os.path.join(ROOT, "include", "nepmi355.h")).read()
    assert re.search(r"int32_t\s+nep_interp_coeffs\s*\(int64_t E, int32_t J, int32_t K,", hdr)
    assert "types_cheb_pep.jl:94-114" in hdr and "types_poly.jl:121-164" in hdr
    assert "nep_interp_coeffs" in na._lib.SIGNATURES
    assert "(:nep_interp_coeffs, LIB)" in open(os.path.join(ROOT, "julia", "NEPMI355X.jl")).read()
    from nep_amd import build
    assert "interp.hip" in build.SOURCES


# ---- funcs.Chebyshev ------------------------------------------------------------------------------------------------------------
DEGREES = [0, 1, 2, 5, 8, 19]
INTERVALS = [(-1.0, 1.0), (-0.9, 1.5)]
POINTS = [0.3, 0.2 + 0.4j, 2.1]                   # real, complex, outside both intervals
SCALES = [1.0, 0.3]


_abs_poly_deriv, _cheb_tol = ic.abs_poly_deriv, ic.cheb_tol


@pytest.mark.parametrize("j", DEGREES)
@pytest.mark.parametrize("ab", INTERVALS)
def test_chebyshev_values_derivs_taylor_against_numpy(j, ab):
    a, b = ab
    f = funcs.Chebyshev(j, a, b)
    assert f.real_on_reals() and isinstance(f, funcs.ScalarFun)
    ej = np.eye(j + 1)[j]
    K = j + 4
    for lam, scale in product(POINTS, SCALES):
        x = 2 * (lam - a) / (b - a) - 1
        chain = 2 * scale / (b - a)
        d = f.derivs(lam, K, scale)
        t = f.taylor(lam, K, scale)
        assert d.dtype == np.complex128 and d.shape == (K,) and t.shape == (K,)
        assert np.all(d[j + 1:] == 0) and np.all(t[j + 1:] == 0)                 # exactly zero above the degree
        fact = 1.0
        for m in range(j + 1):
            fact *= max(m, 1)
            want = ch.chebval(x, ch.chebder(ej, m) if m else ej) * chain ** m
            tol = _cheb_tol(j, m, abs(x), chain)
            assert abs(d[m] - want) <= tol, (j, ab, lam, scale, m, d[m], want, tol)
            assert abs(t[m] - want / fact) <= tol / fact, (j, ab, lam, scale, m)
        tol0 = _cheb_tol(j, 0, abs(x), 1.0)
        assert abs(f(lam) - ch.chebval(x, ej)) <= tol0
        assert abs(f.values(np.array([lam, lam]))[1] - ch.chebval(x, ej)) <= tol0


@pytest.mark.parametrize("j", DEGREES)
@pytest.mark.parametrize("ab", INTERVALS)
def test_chebyshev_matfun_on_a_jordan_block(j, ab):
    a, b = ab
    f = funcs.Chebyshev(j, a, b)
    for lam, scale in product(POINTS, SCALES):
        S = np.diag(np.full(4, lam)) + np.diag(scale * np.arange(1, 4), -1)       # first column of f(S): scale^m f^(m)(lam)
        FS = f.matfun(S)
        assert FS.shape == (4, 4)
        assert FS.dtype == (np.complex128 if np.iscomplexobj(S) else np.float64)  # a real S gives a real result
        d = f.derivs(lam, 4, scale)
        x = 2 * (lam - a) / (b - a) - 1
        for m in range(4):
            tol = _cheb_tol(j, m, abs(x), 2 * scale / (b - a), inner=4)
            assert abs(FS[m, 0] - d[m]) <= tol, (j, ab, lam, scale, m, FS[m, 0], d[m], tol)


def test_chebyshev_rejects_a_bad_interval():
    for a, b in ((1.0, 1.0), (2.0, -1.0), (0.0, 1j)):
        with pytest.raises(ValueError):
            funcs.Chebyshev(3, a, b)


def test_chebpep_rejects_no_nodes():
    with pytest.raises(ValueError):
        na.ChebPEP(na.nep_gallery("dep0", 5), 0)


# ---- nodes and weights ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [1, 2, 3, 7, 13, 16, 20])
@pytest.mark.parametrize("ab", INTERVALS)
def test_weights_invert_the_chebyshev_values_at_the_nodes(k, ab):
    """weights [T_i(x_j)]^T = I (discrete orthogonality, Mason and Handscomb ch. 8).  Bound 8 k eps: an entry is (2 / k) sum_j
    T_i(x_j) T_l(x_j), a sum of k products whose absolute values add up to at most 2 (2 k eps for the summation), and each factor
    carries the rounding of its node and of its recurrence, on average over the nodes a relative error of at most k eps each (both
    factors, times the sum 2: 4 k eps); 8 k eps leaves a factor 4 / 3."""
    a, b = ab
    x = na.chebyshev_nodes(a, b, k)
    assert x.shape == (k,) and np.all(np.diff(x) < 0) and a < x.min() and x.max() < b
    assert np.allclose(x, ic.ref_cheb_nodes(a, b, k), rtol=0, atol=4 * EPS * max(abs(a), abs(b)))
    W = na.chebyshev_weights(a, b, k)
    assert W.shape == (k, k) and W.dtype == np.float64
    T = np.array([ic.ref_cheb_T(a, b, x, i) for i in range(k)])                   # T[i, j] = T_i(x_j), the cosine formula
    assert np.max(np.abs(W @ T.T - np.eye(k))) <= 8 * k * EPS
    assert np.allclose(W[0], 1.0 / k, rtol=0, atol=2 * EPS)                       # the halved first row


# ---- colleague pencil and companion form ----------------------------------------------------------------------------------------
def test_colleague_pencil_eigenpairs_solve_the_polynomial():
    """n = 3, k = 5, random B: for every finite eigenpair (theta, z) of (L0, L1), ||P(theta) z_1|| <= bound, z_1 the normalised
    leading block.  Bound: LAPACK's QZ is backward stable, ||(L0 - theta L1) z|| <= p(N) eps (||L0|| + |theta| ||L1||) ||z|| with a
    modest p(N), taken as 10 N; P(theta) z_1 is a combination of that residual's blocks with weights bounded by the sum of absolute
    terms of the T_i(theta) times ||B_i||, and the residual is relative to ||z||, not ||z_1||:
        bound = 10 N eps (||z|| / ||z_1||) sum_i |T_i|(|theta|) ||B_i||_2."""
    n, k = 3, 5
    rng = np.random.default_rng(20)
    for cplx in (False, True):
        Bv = [rng.standard_normal((n, n)) + (1j * rng.standard_normal((n, n)) if cplx else 0) for _ in range(k)]
        L0, L1 = na.colleague_pencil(Bv)
        N = n * (k - 1)
        assert L0.shape == L1.shape == (N, N)
        L0s, L1s = na.colleague_pencil(Bv, sparse=True)
        assert np.array_equal(L0s.toarray(), L0) and np.array_equal(L1s.toarray(), L1)
        th, Z = sla.eig(L0, L1)
        fin = np.isfinite(th)
        assert fin.sum() >= N - n                                                 # at most n infinite ones (2 B_{k-1} singular: none here)
        for t, z in zip(th[fin], Z[:, fin].T):
            z1 = z[:n] / np.linalg.norm(z[:n])
            P = ic.ref_cheb_eval(Bv, -1.0, 1.0, t)
            mag = sum(_abs_poly_deriv(i, 0, abs(t)) * np.linalg.norm(B, 2) for i, B in enumerate(Bv))
            bound = 10 * N * EPS * (np.linalg.norm(z) / np.linalg.norm(z[:n])) * mag
            assert np.linalg.norm(P @ z1) <= bound, (t, np.linalg.norm(P @ z1), bound)
    for kk in (0, 1, 2):
        with pytest.raises(ValueError):
            na.colleague_pencil(Bv[:kk])


def test_companion_against_the_list_form_of_polyeig_on_a_cubic():
    """the eigenvalues of (A, E) = companion(pep) are those polyeig(list) returns: each within 2 p(N) eps kappa of one of them,
    kappa = ||y|| ||x|| (||A|| + |lam| ||E||) / |y^H E x| the condition number of the eigenvalue of the pencil and p(N) = 10 N the
    backward error constant taken for QZ, once for each of the two computations"""
    import scipy.sparse as sp
    n, d = 4, 3
    rng = np.random.default_rng(21)
    Av = [rng.standard_normal((n, n)) for _ in range(d + 1)]
    pep = na.PEP(Av)
    E, A = na.companion(pep)
    N = n * d
    assert E.shape == A.shape == (N, N) and not sp.issparse(E)
    lam_list, V_list = na.polyeig(Av)
    lam, Y, X = sla.eig(A, E, left=True, right=True)
    nA, nE = np.linalg.norm(A, 2), np.linalg.norm(E, 2)
    for l, y, x in zip(lam, Y.T, X.T):
        kappa = np.linalg.norm(y) * np.linalg.norm(x) * (nA + abs(l) * nE) / abs(np.vdot(y, E @ x))
        assert np.min(np.abs(lam_list - l)) <= 2 * 10 * N * EPS * kappa, (l, kappa)
        v = x[:n]                                                                  # the leading block is an eigenvector of the PEP
        M = sum(l ** i * Av[i] for i in range(d + 1))
        assert np.linalg.norm(M @ v) <= 10 * N * EPS * sum(abs(l) ** i * np.linalg.norm(Av[i], 2) for i in range(d + 1)) * np.linalg.norm(x)
    Es, As = na.companion(na.PEP([sp.csc_matrix(B) for B in Av]))
    assert sp.issparse(Es) and sp.issparse(As) and np.array_equal(Es.toarray(), E) and np.array_equal(As.toarray(), A)
    # polyeig of the PEP object goes through get_Av(): the same bits as the list
    lam_pep, V_pep = na.polyeig(pep)
    assert np.array_equal(lam_pep, lam_list) and np.array_equal(V_pep, V_list)
    with pytest.raises(TypeError):
        na.polyeig(Av, nev=2)
