"""Host-side tests of the EigSolver layer and mslp: the checker that test_gpu_lineig.py runs on nep_basis_rotate (it passes the
NumPy implementation and rejects its mutants), the dense restatement of the method of successive linear problems
(tests/lineig_checkers.py) against test/mslp.jl and the docstring example of src/method_mslp.jl, EigenEigSolver (pure host code),
and the declarations the feature adds."""
import inspect
import os
import re
from functools import partial
from itertools import combinations

import numpy as np
import pytest
import scipy.sparse as sp

import nep_amd as na
import lineig_checkers as lc
import primitive_checkers as pc

EPS = np.finfo(float).eps
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the checker of nep_basis_rotate --------------------------------------------------------------------------------------------
def test_numpy_implementation_passes_every_case():
    n = 0
    for c in lc.ROTATE.cases():
        lc.ROTATE.check(lc.ROTATE.ref, c)
        n += 1
    assert 150 <= n <= 400, n
    print("%s: %d cases, largest |impl - ref| / bound = %.3g" % (lc.ROTATE.name, n, pc.RATIOS.get(lc.ROTATE.name, 0.0)))


@pytest.mark.parametrize("mut", lc.ROTATE.mutants)
def test_checker_rejects_mutant(mut):
    """columns formed left to right from columns already overwritten, the carry column forgotten, the carry column copied before
    the rotation, the rows behind the last multiple of 64 dropped, `rows` used as the stride, Q conjugated, column p written
    without a carry, one real part off by one ulp: some case fails on each"""
    ratios = dict(pc.RATIOS)
    impl = partial(lc.ROTATE.ref, mut=mut)
    rejected = None
    for c in lc.ROTATE.cases():
        if mut in lc.ROTATE.exact_only_mutants and c.kind != "exact":
            continue
        try:
            lc.ROTATE.check(impl, c)
        except AssertionError:
            rejected = c
            break
    pc.RATIOS.clear(); pc.RATIOS.update(ratios)
    assert rejected is not None, "no case rejects the mutant %r" % mut


def test_case_list_covers_the_shapes():
    sh = list(lc.ROTATE.shapes())
    assert lc.ROT_ROWS == [1, 2, 63, 64, 65, 257, 1025] and lc.ROT_CARRY == [0, 1] and lc.ROT_PAD == [0, 3]
    assert lc.ROT_MP == [(1, 1), (2, 1), (5, 5), (17, 4), (20, 10), (64, 33), (128, 64), (128, 128)]
    for a, b in combinations(range(6), 2):                               # every pair of values of two different factors
        want = {(va, vb) for va in lc.ROT_FACTORS[a] for vb in lc.ROT_FACTORS[b]}
        assert want <= {(s[a], s[b]) for s in sh}, (a, b)
    assert {(s[0], s[1], s[2]) for s in sh} >= {(r, mp, c) for r in lc.ROT_ROWS for mp in lc.ROT_MP for c in (0, 1)}
    assert {s[6] > 0 for s in sh} == {True, False}                        # with and without a lead offset
    assert {s[7] is pc.NAN for s in sh} == {True, False}                  # NaN and sentinel padding


# ---- the restatement against the reference --------------------------------------------------------------------------------------
def _docstring_example():
    """src/method_mslp.jl:19-23: Av = [ones, I, triu(ones)], fv = [lam, lam^2, 1 / (lam - 10)]"""
    Av = [np.ones((3, 3)), np.eye(3), np.triu(np.ones((3, 3)))]
    f = [lambda l: l, lambda l: l ** 2, lambda l: 1.0 / (l - 10.0)]
    df = [lambda l: 1.0, lambda l: 2 * l, lambda l: -1.0 / (l - 10.0) ** 2]
    return lc.RefNep(Av, f, df)


def test_restatement_converges_on_the_docstring_example():
    nep = _docstring_example()
    lam, v, it, hist, ok = lc.ref_mslp(nep)
    print("iterations", it, "lam", lam, "residual %.3g" % nep.residual(lam, v))
    assert ok and np.linalg.norm(nep.M(lam) @ v) < 1e-10
    # the same iteration through the package's host pieces (compute_Mder of the SPMF and EigenEigSolver run without a device)
    from nep_amd import funcs
    pk = na.SPMF_NEP(nep.Av, [funcs.ident(), funcs.Monomial(2), funcs.Resolvent(funcs.one(), 10.0)])
    l2 = 0j
    for k in range(it):
        d, X = na.eig_solve(na.EigenEigSolver(pk.compute_Mder(l2, 0), pk.compute_Mder(l2, 1)), target=0, nev=1)
        l2 = l2 - d[0]
    assert abs(l2 - lam) <= 1e-10 * (1 + abs(lam))
    assert np.linalg.norm(nep.M(l2) @ (X[:, 0] / np.linalg.norm(X[:, 0]))) < 1e-10


def test_restatement_dense_and_sparse_beam_agree():
    """test/mslp.jl:10-22: beam(5) with dense and with sparse matrices gives the same eigenvalue"""
    nep = na.nep_gallery("beam", 5)
    assert all(sp.issparse(A) for A in nep.A)
    dense = lc.RefNep([np.eye(5)] + [A.toarray() for A in nep.A], lc.ref_dep_of(nep).f, lc.ref_dep_of(nep).df)
    l1, v1, it1, _, ok1 = lc.ref_mslp(lc.ref_dep_of(nep), lam=-1.0)
    l2, v2, it2, _, ok2 = lc.ref_mslp(dense, lam=-1.0)
    assert ok1 and ok2 and abs(l1 - l2) < 1e-12 * (1 + abs(l1))
    assert np.linalg.norm(dense.M(l1) @ v1) < 1e-10


def test_restatement_on_the_double_eigenvalue():
    """dep_double from lam = 9i: linear convergence to the double eigenvalue 3 pi i -- ten iterations do not reach eps * 100, a
    hundred do"""
    nep = lc.ref_dep_of(na.nep_gallery("dep_double"))
    lam, v, it, hist, ok = lc.ref_mslp(nep, lam=9j, maxit=10, measure="residual")
    assert not ok and it == 10 and hist[-1] > 100 * EPS
    lam, v, it, hist, ok = lc.ref_mslp(nep, lam=9j, maxit=100, measure="residual")
    print("iterations", it, "lam", lam, "|lam - 3 pi i| = %.3g" % abs(lam - 3j * np.pi))
    assert ok and it > 10 and abs(lam - 3j * np.pi) < 1e-6


def test_gallery_problems():
    nep = na.nep_gallery("beam", 7)
    A0, A1 = (A.toarray() for A in nep.A)
    want = np.diag(-2.0 * np.ones(7)) + np.diag(np.ones(6), 1) + np.diag(np.ones(6), -1)
    want[6, 6] = 7.0; want[6, 5] = -7.0
    assert np.array_equal(A0, want) and A1[6, 6] == 1.0 and np.count_nonzero(A1) == 1 and list(nep.tauv) == [0.0, 1.0]
    assert na.nep_gallery("beam").n == 100
    dd = lc.ref_dep_of(na.nep_gallery("dep_double"))
    s = np.linalg.svd(dd.M(3j * np.pi), compute_uv=False)
    assert dd.n == 3 and s[-1] < 1e-12 * s[0]                             # 3 pi i is an eigenvalue ...
    d, X, Y, kappa = lc.pencil_spectrum(dd.M(3j * np.pi), dd.dM(3j * np.pi))
    assert kappa[lc.nearest(d, 0.0, 1)[0]] > 1e6                          # ... and not a simple one: y^H M' x = 0


# ---- EigenEigSolver, DefaultEigSolver, eig_solve: host code ---------------------------------------------------------------------
def _pencil(n=6, seed=2):
    rng = np.random.default_rng(seed)
    return rng.standard_normal((n, n)), rng.standard_normal((n, n)) + 3 * np.eye(n)


def test_eigen_eigsolver_orders_by_distance_and_truncates():
    A, B = _pencil()
    for target in (0, 0.5 - 1j):
        D, V = na.eig_solve(na.EigenEigSolver(A, B), nev=4, target=target)
        assert D.shape == (4,) and V.shape == (6, 4)
        dist = np.abs(target - D)
        assert np.all(np.diff(dist) >= 0)
        allD = np.linalg.eigvals(np.linalg.solve(B, A))
        assert np.allclose(np.sort(np.abs(target - allD))[:4], dist, rtol=1e-9)
        for d, x in zip(D, V.T):
            assert np.linalg.norm(A @ x - d * (B @ x)) < 1e-10 * np.linalg.norm(x)
    D1, V1 = na.EigenEigSolver(A, B).eig_solve()                          # the default nev is 1
    assert D1.shape == (1,) and V1.shape == (6, 1)


def test_eigen_eigsolver_standard_form():
    A, _ = _pencil()
    D, V = na.eig_solve(na.EigenEigSolver(A), nev=6, target=1.0)
    assert np.allclose(np.sort_complex(D), np.sort_complex(np.linalg.eigvals(A)))
    for d, x in zip(D, V.T):
        assert np.linalg.norm(A @ x - d * x) < 1e-10 * np.linalg.norm(x)
    Ds, _ = na.eig_solve(na.EigenEigSolver(sp.csc_matrix(A)), nev=2, target=1.0)     # a sparse matrix is densified
    assert np.allclose(Ds, D[:2])


def test_default_eigsolver_dispatches_on_sparsity():
    A, B = _pencil()
    s = na.DefaultEigSolver(A, B)
    assert isinstance(s.subsolver, na.EigenEigSolver) and isinstance(s, na.EigSolver)
    D, V = na.eig_solve(s)                                                # the default nev is n
    assert D.shape == (6,) and V.shape == (6, 6)
    assert isinstance(na.DefaultEigSolver(A).subsolver, na.EigenEigSolver)
    assert inspect.signature(na.ArnoldiEigSolver.eig_solve).parameters["nev"].default == 6
    assert inspect.signature(na.EigenEigSolver.eig_solve).parameters["nev"].default == 1
    with pytest.raises(TypeError, match="sparse"):
        na.ArnoldiEigSolver(A, B)


def test_eig_solve_dispatches_to_a_user_class():
    class MyEigSolver:                                                    # src/LinSolvers.jl:290-306
        def __init__(self, A, E):
            self.A, self.E = A, E

        def eig_solve(self, nev=1, target=0):
            w, X = np.linalg.eig(np.linalg.solve(self.E, self.A))
            i = np.argmin(np.abs(w))
            return w[i], X[:, i]
    A, B = _pencil()
    d, x = na.eig_solve(MyEigSolver(A, B), target=0, nev=1)
    assert np.linalg.norm(A @ x - d * (B @ x)) < 1e-10


# ---- declarations ---------------------------------------------------------------------------------------------------------------
def test_header_build_and_exports_name_the_feature():
    hdr = open(os.path.join(ROOT, "include", "nepmi355.h")).read()
    for name in ("nep_basis_rotate", "nep_arnoldi_create", "nep_arnoldi_steps", "nep_arnoldi_wait", "nep_arnoldi_destroy"):
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert name in na._lib.SIGNATURES
    assert "src/LinSolvers.jl:390-416" in hdr and "src/method_mslp.jl:61-70" in hdr
    from nep_amd import build
    assert "lineig.hip" in build.SOURCES
    for name in ("mslp", "EigSolver", "EigenEigSolver", "ArnoldiEigSolver", "DefaultEigSolver", "eig_solve"):
        assert hasattr(na, name), name


def test_mslp_signature_matches_the_reference():
    sig = inspect.signature(na.mslp)
    assert list(sig.parameters) == ["nep", "errmeasure", "tol", "maxit", "lam", "logger", "eigsolvertype", "hist"]
    d = {k: v.default for k, v in sig.parameters.items()}
    assert d["tol"] == EPS * 100 and d["maxit"] == 100 and d["lam"] == 0 and d["eigsolvertype"] is na.DefaultEigSolver
    assert d["errmeasure"] is None and d["hist"] is None
