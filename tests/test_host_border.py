"""Host-side tests of the checker that test_gpu_jd_effenberger.py runs on nep_defl_border (it passes the NumPy implementation and
rejects its mutants), of the one-solve bordered solve against the reference's p + 1-solve algorithm, and of the dense restatement
of jd_effenberger that the device driver is compared with."""
import math
import os
import re
from functools import partial

import numpy as np
import pytest

import nep_amd as na
import border_checkers as bc
import deflation_checkers as dc
import primitive_checkers as pc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SQEPS = math.sqrt(np.finfo(float).eps)


# ---- the checker of nep_defl_border ---------------------------------------------------------------------------------------------
def test_numpy_implementation_passes_every_case():
    n = 0
    for c in bc.BORDER.cases():
        bc.BORDER.check(bc.BORDER.ref, c)
        n += 1
    assert 60 <= n <= 80, n
    print("%s: %d cases, largest |impl - ref| / bound = %.3g" % (bc.BORDER.name, n, pc.RATIOS.get(bc.BORDER.name, 0.0)))


@pytest.mark.parametrize("mut", bc.BORDER.mutants)
def test_checker_rejects_mutant(mut):
    """c with the wrong sign, X^T in place of X^H, T transposed, b2 ignored, one row skipped, the entry behind the result written,
    the tail not scaled, one real part off by one ulp: some case fails on each"""
    ratios = dict(pc.RATIOS)
    impl = partial(bc.BORDER.ref, mut=mut)
    rejected = None
    for c in bc.BORDER.cases():
        if c.args["n0"] > 5000 or (mut in bc.BORDER.exact_only_mutants and c.kind != "exact"):
            continue
        try:
            bc.BORDER.check(impl, c)
        except AssertionError:
            rejected = c
            break
    pc.RATIOS.clear(); pc.RATIOS.update(ratios)
    assert rejected is not None, "no case rejects the mutant %r" % mut


def test_case_list_covers_the_shapes():
    cs = list(bc.BORDER.cases())
    args = [(c.kind, c.args) for c in cs]
    assert {a["n0"] for _, a in args} == set(bc.DB_N0) | {bc.DB_GRID_ROWS}
    assert {(a["n0"], a["p"]) for _, a in args} >= {(n0, p) for n0 in bc.DB_N0 for p in bc.DB_P}
    for kind in ("exact", "rounded"):
        mine = [a for k, a in args if k == kind]
        assert {a["p"] for a in mine} == set(bc.DB_P)
        assert {a["ldx"] - a["n0"] for a in mine} == {0, 3}
        assert {a["Y"] is None for a in mine} == {True, False}             # in place and out of place
        assert {a["b2"] is None for a in mine} == {True, False}
        assert {a["scale"] for a in mine} == {1.0, -1.0}


# ---- the one-solve form and the reference's algorithm against a dense solve of the bordered matrix -----------------------------
@pytest.fixture(scope="module")
def dep60():
    """ref_dep0_sparse(60) with three eigenpairs found one after the other by ref_augnewton on the deflated problems"""
    A0, A1, _, _ = dc.ref_dep0_sparse(60)
    nep = dc.ref_dep(A0, A1)
    d, chain = nep, []
    for i in range(3):
        lam, v, _ = dc.ref_augnewton(d, 0.2 + 0.5j, np.ones(60 + i), 1e-11, maxit=100)
        d = dc.ref_deflate(d, lam, v, "Generic")
        chain.append(d)
    return nep, chain


@pytest.mark.parametrize("pairs", [1, 2, 3])
def test_one_solve_and_reference_solve_the_bordered_system(dep60, pairs):
    nep, chain = dep60
    d = chain[pairs - 1]
    sigma = 0.3 + 0.2j
    assert d.p == pairs and np.linalg.norm(d.V0.conj().T @ d.V0 - np.eye(pairs)) < 1e-13
    condM = np.linalg.cond(nep.Mder(sigma))
    assert condM <= 1e5, condM
    Mt = d.Mder(sigma)
    rng = np.random.default_rng(17 + pairs)
    b = rng.standard_normal(60 + pairs) + 1j * rng.standard_normal(60 + pairs)
    xd = np.linalg.solve(Mt, b)
    for name, f in (("one-solve", bc.ref_border_solve_onesolve), ("reference", bc.ref_border_solve_reference)):
        x = f(d, sigma, b)
        back = np.linalg.norm(Mt @ x - b) / (np.linalg.norm(Mt, 1) * np.linalg.norm(x))
        print("%d pairs, cond M = %.3g, %s: backward error %.3g, |x - dense| / |dense| = %.3g"
              % (pairs, condM, name, back, np.linalg.norm(x - xd) / np.linalg.norm(xd)))
        assert np.linalg.norm(Mt @ x - b) <= 1e-10 * np.linalg.norm(Mt, 1) * np.linalg.norm(x)


# ---- the dense restatement of jd_effenberger (mirror of test/jd.jl:64-74) -------------------------------------------------------
def _assert_distinct_eigenpairs(nep, D, V, count, tol):
    assert len(D) == count and V.shape == (nep.n, count)
    for i in range(count):
        for j in range(i):
            assert abs(D[i] - D[j]) / abs(D[i]) > SQEPS, (D[i], D[j])
    res = [np.linalg.norm(nep.Mlincomb(l, v)) / np.linalg.norm(v) for l, v in zip(D, V.T)]
    print("eigenvalues", D, "largest residual %.3g" % max(res))
    assert max(res) < tol


@pytest.mark.parametrize("solver", ["onesolve", "reference"])
def test_ref_jd_effenberger_dep0_sparse(solver):
    A0, A1, _, _ = dc.ref_dep0_sparse(60)
    nep = dc.ref_dep(A0, A1)
    np.random.seed(0)
    D, V, its = bc.ref_jd_effenberger(nep, neigs=3, maxit=55, lam=0.6, v=np.ones(60), tol=1e-10, solver=solver)
    print("%s: %d iterations" % (solver, its))
    _assert_distinct_eigenpairs(nep, D, V, 3, 1e-10)


def test_ref_jd_effenberger_pep0():
    from oracle import gallery as og
    nep = bc.ref_pep(og.pep0(250).A)
    np.random.seed(0)
    D, V, its = bc.ref_jd_effenberger(nep, neigs=5, maxit=80, lam=0.82 + 0.9j, v=np.ones(250), tol=1e-10)
    print("%d iterations" % its)
    _assert_distinct_eigenpairs(nep, D, V, 5, 1e-10)


# ---- the public surface ---------------------------------------------------------------------------------------------------------
def test_header_declares_the_border_kernel_and_the_package_exports_the_driver():
    hdr = open(os.path.join(ROOT, "include", "nepmi355.h")).read()
    assert re.search(r"int32_t\s+nep_defl_border\s*\(int64_t n0, int32_t p,", hdr)
    assert "nep_defl_border" in na._lib.SIGNATURES
    for name in ("jd_effenberger", "DeflatedNEPLinSolver", "DeflatedNEPLinSolverCreator"):
        assert hasattr(na, name), name
    assert issubclass(na.DeflatedNEPLinSolver, na.LinSolver)
    assert isinstance(na.DeflatedNEPLinSolverCreator().orglinsolvercreator, na.DefaultLinSolverCreator)
