"""Host-side tests of the deflation layer (nep_amd.deflation, funcs.Resolvent, gallery.dep0_sparse) and of the checker that
test_gpu_deflation.py runs on nep_defl_expand: the checker passes the NumPy implementation and rejects its mutants."""
import math
from functools import partial

import numpy as np
import pytest
import scipy.sparse as sp

import nep_amd as na
import deflation_checkers as dc
import primitive_checkers as pc

SQEPS = math.sqrt(np.finfo(float).eps)


# ---- the checker of nep_defl_expand ---------------------------------------------------------------------------------------------
def test_numpy_implementation_passes_every_case():
    n = 0
    for c in dc.DEFL.cases():
        dc.DEFL.check(dc.DEFL.ref, c)
        n += 1
    assert 55 <= n <= 70, n
    print("%s: %d cases, largest |impl - ref| / bound = %.3g" % (dc.DEFL.name, n, pc.RATIOS.get(dc.DEFL.name, 0.0)))


@pytest.mark.parametrize("mut", dc.DEFL.mutants)
def test_checker_rejects_mutant(mut):
    """a wrong sign of G, W_{d+1}, W_{d-1}, a dropped startder offset, z_bottom not zeroed for startder > 0, one row skipped, a
    padding row written, one result off by 1e-13 relative: some case fails on each"""
    ratios = dict(pc.RATIOS)
    impl = partial(dc.DEFL.ref, mut=mut)
    rejected = None
    for c in dc.DEFL.cases():
        if c.args["n0"] > 5000 or (mut in dc.DEFL.exact_only_mutants and c.kind != "exact"):
            continue
        try:
            dc.DEFL.check(impl, c)
        except AssertionError:
            rejected = c
            break
    pc.RATIOS.clear(); pc.RATIOS.update(ratios)
    assert rejected is not None, "no case rejects the mutant %r" % mut


def test_case_list_covers_the_shapes():
    cs = list(dc.DEFL.cases())
    assert {c.args["n0"] for c in cs} >= set(dc.DE_N0)
    assert {(c.args["p"], (c.args["k"], c.args["s"])) for c in cs} >= {(p, ks) for p in dc.DE_P for ks in dc.DE_KS}
    assert {c.kind for c in cs} == {"exact", "rounded"}
    pads = {(c.kind, c.args["ldo"] - c.args["n0"]) for c in cs}
    assert pads == {("exact", 0), ("exact", 3), ("rounded", 0), ("rounded", 3)}


# ---- funcs.Resolvent ------------------------------------------------------------------------------------------------------------
FS = {"one": na.funcs.one(), "ident": na.funcs.ident(), "exp": na.funcs.Exp(-1.0), "isqrt": na.funcs.ISqrt(1.0, 0.5)}


@pytest.mark.parametrize("name", sorted(FS))
def test_resolvent_derivs_vs_matrix_function(name):
    """closed recurrence vs g(S)[:, 0] of the bidiagonal matrix S = lam I + subdiag(1..k-1) (the reference's route to scaled
    derivatives, src/NEPTypes.jl:993-1004), 12 derivatives"""
    k, lam, mu = 12, 0.8 + 0.3j, 0.25 - 0.6j
    g = na.funcs.Resolvent(FS[name], mu)
    S = np.diag(np.full(k, lam)) + np.diag(np.arange(1.0, k), -1)
    want = g.matfun(S)[:, 0]
    got = g.derivs(lam, k)
    assert np.max(np.abs(got - want) / np.abs(want)) < 1e-9
    assert abs(g(lam) - FS[name](lam) / (lam - mu)) <= 1e-15 * abs(g(lam))
    np.testing.assert_allclose(g.values([lam, 2.0]), [g(lam), g(2.0)], rtol=1e-15)
    sc = 3.5
    np.testing.assert_allclose(g.derivs(lam, k, sc), got * sc ** np.arange(k), rtol=1e-12)
    fact = np.array([math.factorial(j) for j in range(k)], dtype=float)
    np.testing.assert_allclose(g.taylor(lam, k, sc) * fact, g.derivs(lam, k, sc), rtol=1e-12)


def test_resolvent_real_on_reals():
    assert na.funcs.Resolvent(na.funcs.Exp(-1.0), 0.5).real_on_reals()
    assert not na.funcs.Resolvent(na.funcs.Exp(-1.0), 0.5 + 1j).real_on_reals()
    assert not na.funcs.Resolvent(na.funcs.ISqrt(), 0.5).real_on_reals()


# ---- gallery.dep0_sparse --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [3, 100])
def test_dep0_sparse_equals_restatement(n):
    nep = na.nep_gallery("dep0_sparse", n, 0.25)
    A0, A1, m0, m1 = dc.ref_dep0_sparse(n, 0.25)
    assert sp.issparse(nep.A[0]) and nep.size() == (n, n)
    assert np.array_equal(nep.A[0].toarray(), A0) and np.array_equal(nep.A[1].toarray(), A1)
    assert nep.A[0].nnz == m0.sum() and nep.A[1].nnz == m1.sum()
    assert list(nep.tauv) == [0.0, 1.0]
    if n == 100:
        assert (nep.A[0].nnz, nep.A[1].nnz) == (2281, 2290)
        assert na.nep_gallery("dep0_sparse").A[0].nnz == 2281           # the defaults are (100, 0.25)


# ---- deflation: host layer ------------------------------------------------------------------------------------------------------
def _pairs3():
    """dep0_sparse(3) with two eigenpairs from the dense restatement (the second one of the once-deflated problem)"""
    nep = na.nep_gallery("dep0_sparse", 3)
    ref = dc.ref_dep(nep.A[0].toarray(), nep.A[1].toarray())
    lam1, v1, steps = dc.ref_augnewton(ref, 1.65, np.ones(3), 1e-11)
    assert abs(lam1 - 0.233998529813247) < 1e-9 and steps <= 8
    rd = dc.ref_deflate(ref, lam1, v1, "Generic")
    lam2, v2, _ = dc.ref_augnewton(rd, 0.2 + 0.5j, np.ones(4), 1e-11, maxit=50)
    return nep, ref, (lam1, v1), (lam2, v2)


def test_normalize_schur_pair():
    rng = np.random.default_rng(5)
    V = rng.standard_normal((7, 3)) + 1j * rng.standard_normal((7, 3))
    S = rng.standard_normal((3, 3)) + 1j * rng.standard_normal((3, 3))
    S0, V0 = S.copy(), V.copy()
    S2, V2 = na.normalize_schur_pair(S, V)
    assert np.array_equal(S, S0) and np.array_equal(V, V0)
    assert np.linalg.norm(V2.conj().T @ V2 - np.eye(3)) < 1e-14
    # the same invariant pair: V S = V2 S2 R with V = V2 R, i.e. V2 S2 = V S R^-1, and V f(S) spans the same
    R = V2.conj().T @ V
    assert np.linalg.norm(V2 @ S2 @ R - V @ S) < 1e-13 * np.linalg.norm(V @ S)
    assert np.allclose(np.sort_complex(np.linalg.eigvals(S2)), np.sort_complex(np.linalg.eigvals(S)), rtol=1e-12)
    with pytest.warns(UserWarning):
        na.normalize_schur_pair(np.eye(3), np.ones((2, 3)))


@pytest.mark.parametrize("mode", ["Generic", "SPMF", "MM"])
def test_deflating_a_deflated_nep_grows_p_by_one(mode):
    nep, ref, (lam1, v1), (lam2, v2) = _pairs3()
    d1 = na.deflate_eigpair(nep, lam1, v1, mode=mode)
    assert d1.size() == (4, 4) and d1.size(1) == 4 and d1.V0.shape == (3, 1) and d1.orgnep is nep
    assert type(d1) is {"Generic": na.DeflatedGenericNEP, "SPMF": na.DeflatedSPMF, "MM": na.DeflatedNEPMM}[mode]
    d2 = na.deflate_eigpair(d1, lam2, v2)                               # "Auto" on a deflated NEP keeps its mode
    assert type(d2) is type(d1) and d2.size() == (5, 5) and d2.V0.shape == (3, 2) and d2.S0.shape == (2, 2)
    assert d2.orgnep is nep                                             # built on the ORIGINAL problem
    assert np.linalg.norm(d2.V0.conj().T @ d2.V0 - np.eye(2)) < 1e-14
    D, V = na.get_deflated_eigpairs(d2)
    assert min(abs(D - lam1)) < 1e-10 and min(abs(D - lam2)) < 1e-10
    for l, v in zip(D, V.T):
        assert np.linalg.norm(ref.Mlincomb(l, v)) / np.linalg.norm(v) < 1e-9
    D1, V1 = na.get_deflated_eigpairs(d1, lam2, v2)                     # the three-argument form = deflate, then extract
    assert np.allclose(np.sort_complex(D1), np.sort_complex(D), rtol=1e-13)


def test_mode_errors_match_the_reference():
    nep, ref, (lam1, v1), _ = _pairs3()
    assert na.verify_deflate_mode(nep, "Auto") == "SPMF"
    generic = na.Mder_NEP(3, lambda lam: ref.Mder(lam))
    assert na.verify_deflate_mode(generic, "Auto") == "Generic"
    with pytest.raises(ValueError, match="SPMF-mode only possible for `AbstractSPMF`-NEPs"):
        na.deflate_eigpair(generic, lam1, v1, mode="SPMF")
    d = na.deflate_eigpair(nep, lam1, v1, mode="Generic")
    for bad in ("SPMF", "MM", "nonsense"):
        with pytest.raises(ValueError, match="Unknown mode / type"):
            na.deflate_eigpair(d, lam1, np.ones(4), mode=bad)
    assert na.verify_deflate_mode(d, "Generic") == "Generic"


def test_deflated_spmf_structure():
    nep, ref, (lam1, v1), (lam2, v2) = _pairs3()
    d = na.deflate_eigpair(na.deflate_eigpair(nep, lam1, v1, mode="SPMF"), lam2, v2)
    rd = dc.ref_deflate(dc.ref_deflate(ref, lam1, v1, "Generic"), lam2, v2, "Generic")
    m, p, n0 = 3, 2, 3
    Av, fv = d.get_Av(), d.get_fv()
    assert len(Av) == len(fv) == m + m * p + 1
    assert all(A.shape == (n0 + p, n0 + p) for A in Av)
    lam = 2 + 2j
    M = sum(f(lam) * A.toarray() for A, f in zip(Av, fv))
    want = rd.Mder(lam)
    assert np.linalg.norm(M - want) / np.linalg.norm(want) < 1e-13
    ws = dc.RefDeflated(rd.org, rd.S0, rd.V0, "SPMF").Mder(lam)          # the restatement's own SPMF form agrees with its Generic form
    assert np.linalg.norm(ws - want) / np.linalg.norm(want) < 1e-13
