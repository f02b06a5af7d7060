"""Host-side tests of blocknewton: the checker that test_gpu_blocknewton.py runs on nep_spmf_blockprod (it passes the NumPy
implementation and rejects its mutants), the dense restatement of the block Newton method (tests/blocknewton_checkers.py) against
test/blocknewton.jl and the docstring example of src/method_blocknewton.jl, the two ways of solving the bordered system against
each other, and the host pieces of the driver."""
import importlib
import math
from functools import lru_cache, partial
from itertools import combinations

import numpy as np
import pytest
import scipy.linalg as sla

import nep_amd as na
import blocknewton_checkers as bc
import primitive_checkers as pc

bn = importlib.import_module("nep_amd.blocknewton")        # (nep_amd.blocknewton itself is the driver function)
EPS = np.finfo(float).eps
SQEPS = math.sqrt(EPS)


# ---- the checker of nep_spmf_blockprod ------------------------------------------------------------------------------------------
def test_numpy_implementation_passes_every_case():
    n = 0
    for c in bc.BLOCKPROD.cases():
        bc.BLOCKPROD.check(bc.BLOCKPROD.ref, c)
        n += 1
    assert 250 <= n <= 350, n
    print("%s: %d cases, largest |impl - ref| / bound = %.3g" % (bc.BLOCKPROD.name, n, pc.RATIOS.get(bc.BLOCKPROD.name, 0.0)))


@pytest.mark.parametrize("mut", bc.BLOCKPROD.mutants)
def test_checker_rejects_mutant(mut):
    """G read transposed, the tables of terms 0 and 1 swapped, beta applied when it is zero (NaN leaks), beta ignored, alpha
    conjugated, the last partial row group dropped, the entries behind the first 64 of a row dropped, the entry behind the block
    written, one real part off by one ulp: some case fails on each"""
    ratios = dict(pc.RATIOS)
    impl = partial(bc.BLOCKPROD.ref, mut=mut)
    rejected = None
    for c in bc.BLOCKPROD.cases():
        if mut in bc.BLOCKPROD.exact_only_mutants and c.kind != "exact":
            continue
        try:
            bc.BLOCKPROD.check(impl, c)
        except AssertionError:
            rejected = c
            break
    pc.RATIOS.clear(); pc.RATIOS.update(ratios)
    assert rejected is not None, "no case rejects the mutant %r" % mut


def test_case_list_covers_the_shapes():
    sh = list(bc.BLOCKPROD.shapes())
    assert bc.BP_N == [1, 2, 63, 64, 65, 257, 1025] and bc.BP_MT == [1, 3, 5]
    assert bc.BP_RQ == [(1, 1), (2, 2), (3, 2), (5, 4), (9, 8)] and bc.BP_PAD == [0, 3]
    assert bc.BP_AB == [(1.0, 0.0), (-1.0, 1.0), (0.5 - 2.0j, 3.0 + 1.0j)]
    for a, b in combinations(range(7), 2):                               # every pair of values of two different factors
        want = {(va, vb) for va in bc.BP_FACTORS[a] for vb in bc.BP_FACTORS[b]}
        assert want <= {(s[a], s[b]) for s in sh}, (a, b)
    limit = [s for s in sh if s[2] == (32, 32)]
    assert limit and all(s[1] == 3 for s in limit) and 3 * 32 * 32 == 3072
    assert {s[4] for s in limit} == {"real", "complex"} and {s[6] for s in limit} == {"exact", "rounded"}
    assert {s[7] > 0 for s in sh} == {True, False}                        # with and without a lead offset
    assert {s[8] is pc.NAN for s in sh} == {True, False}                  # NaN and sentinel padding


def test_generated_matrices_have_the_special_rows():
    rng = np.random.default_rng(1)
    for n in (2, 65, 257, 1025):
        terms = bc.make_terms(rng, n, 3, "real", "rounded")
        counts = sum(np.diff(A.indptr) for A in terms)
        assert counts[1] == 0                                             # an empty row
        assert all(A[0, 0] != 0 for A in terms)                           # one (row, col) stored in every term
        if n >= bc.LONG_ROW:
            assert np.diff(terms[0].indptr)[n - 1] == bc.LONG_ROW == 130  # a row with 130 entries
    assert np.diff(bc.make_terms(rng, 1, 1, "complex", "exact")[0].indptr)[0] == 1


# ---- the restatement against the reference --------------------------------------------------------------------------------------
@lru_cache(maxsize=None)
def _run(name, size, p, bordered, refine, armijo_factor=1.0, armijo_max=5, maxit=10):
    nep = bc.ref_dep_of(na.nep_gallery(name, size))
    S, X, it, hist, ok = bc.ref_blocknewton(nep, np.zeros((p, p)), np.eye(nep.n, p), maxit=maxit, armijo_factor=armijo_factor,
                                            armijo_max=armijo_max, bordered=bordered, refine=refine)
    return nep, S, X, it, hist, ok


SPARSE_KW = dict(armijo_factor=0.5, armijo_max=10, maxit=30)


@pytest.mark.parametrize("bordered", ["whole", "eliminate"])
def test_restatement_satisfies_the_reference_test_on_dep0_4(bordered):
    """test/blocknewton.jl: dep0(4), p = 3, armijo_factor = 0.5, maxit = 20; every eigenvalue of S makes M singular"""
    nep, S, X, it, hist, ok = _run("dep0", 4, 3, bordered, 2, armijo_factor=0.5, maxit=20)
    lam = np.linalg.eigvals(S)
    print("iterations", it, "eig(S)", lam)
    assert ok and it == 7
    for l in lam:
        assert bc.sigma_min(nep, l) < SQEPS
    want = [0.099161 + 1.504045j, 0.099161 - 1.504045j, 0.296671]
    assert all(min(abs(l - w) for l in lam) < 1e-5 for w in want)


@pytest.mark.parametrize("bordered", ["whole", "eliminate"])
def test_restatement_runs_the_docstring_example(bordered):
    """dep0(3) with the defaults (src/method_blocknewton.jl:30-43)"""
    nep, S, X, it, hist, ok = _run("dep0", 3, 2, bordered, 2)
    assert ok and it == 6 and bc.pair_residual(nep, S, X) < 100 * EPS
    lam = np.linalg.eigvals(S)
    assert all(min(abs(l - w) for l in lam) < 1e-5 for w in (0.520449, 0.142785))
    assert np.linalg.norm(bc.Vl(X, S).conj().T @ bc.Vl(X, S) - np.eye(2)) < 1e-12


@pytest.mark.parametrize("size,p,count", [(100, 3, 10), (257, 2, 10), (257, 4, 20)])
def test_elimination_with_two_refinement_steps_needs_no_more_iterations(size, p, count):
    whole = _run("dep0_sparse", size, p, "whole", 2, **SPARSE_KW)
    elim = _run("dep0_sparse", size, p, "eliminate", 2, **SPARSE_KW)
    print("whole", whole[3], "eliminate + 2 refinement steps", elim[3])
    assert whole[5] and elim[5] and whole[3] == count and elim[3] <= whole[3]
    for r in (whole, elim):
        assert bc.pair_residual(r[0], r[1], r[2]) < 100 * EPS


def test_elimination_without_refinement_needs_more_iterations():
    """why refinement exists: M(s_i) becomes singular as s_i converges and plain block elimination stagnates"""
    whole = _run("dep0_sparse", 257, 2, "whole", 2, **SPARSE_KW)
    plain = _run("dep0_sparse", 257, 2, "eliminate", 0, **SPARSE_KW)
    print("whole", whole[3], "plain elimination", plain[3], ["%.1e" % h for h in plain[4]])
    assert plain[3] > whole[3]


@pytest.mark.parametrize("bordered", ["whole", "eliminate"])
def test_dep0_sparse_257_p3_does_not_converge(bordered):
    nep, S, X, it, hist, ok = _run("dep0_sparse", 257, 3, bordered, 2, **SPARSE_KW)
    print(bordered, "last errors", ["%.2e" % h for h in hist[-3:]])
    assert not ok and it == 30 and len(hist) == 30 and 1e-3 < hist[-1] < 1e-1


# ---- host pieces of the driver --------------------------------------------------------------------------------------------------
def _fv():
    return na.nep_gallery("dep0", 3).get_fv()


def test_T12_tables_are_divided_differences():
    """f([S I; 0 s I])[0:p, p:2p] = (f(S) - f(s) I) (S - s I)^-1 when s is no eigenvalue of S"""
    rng = np.random.default_rng(3)
    S = np.triu(rng.standard_normal((3, 3)) + 1j * rng.standard_normal((3, 3)))
    s = 0.3 - 0.2j
    tab = bn.tables_T12(_fv(), S, s)
    fS = bn.tables_fS(_fv(), S)
    assert tab.shape == (3, 3, 3)
    for t, f in enumerate(_fv()):
        want = (fS[t] - f(s) * np.eye(3)) @ np.linalg.inv(S - s * np.eye(3))
        assert np.linalg.norm(tab[t] - want) < 1e-12 * (1 + np.linalg.norm(want))
        assert np.linalg.norm(fS[t] - np.asarray(f.matfun(S))) == 0


def test_update21_tables_are_directional_derivatives():
    rng = np.random.default_rng(4)
    p, i = 4, 1
    S = np.triu(rng.standard_normal((p, p)) + 1j * rng.standard_normal((p, p)))
    ds = rng.standard_normal(p) + 1j * rng.standard_normal(p)
    fv = _fv()
    fS = bn.tables_fS(fv, S)
    tab = bn.tables_update21(fv, fS, S, ds, i)
    assert tab.shape == (3, p + 1, p - i - 1)
    Z = np.zeros((p, p), dtype=complex); Z[:, i] = ds
    h = 1e-5
    for t, f in enumerate(fv):
        fd = (np.asarray(f.matfun(S + h * Z)) - np.asarray(f.matfun(S - h * Z))) / (2 * h)
        assert np.linalg.norm(tab[t][:p] - fd[:, i + 1:]) < 1e-8 * (1 + np.linalg.norm(fd))
        assert np.array_equal(tab[t][p], fS[t][i, i + 1:])


def test_refinement_table_and_constraint_tables():
    rng = np.random.default_rng(5)
    p = 3
    S = np.triu(rng.standard_normal((p, p)) + 0j)
    s = S[1, 1]
    fv = _fv()
    T12 = bn.tables_T12(fv, S, s)
    x2 = rng.standard_normal(p) + 0j
    tab = bn.tables_refine(fv, T12, s, x2)
    assert tab.shape == (3, p + 1, 1)
    for t, f in enumerate(fv):
        assert np.allclose(tab[t][:p, 0], T12[t] @ x2) and tab[t][p, 0] == f(s)
    D, P = bn.constraint_tables(S, 1, p)
    Dr, Pr = bc.constraint_tables(S, 1, p)
    assert all(np.array_equal(a, b) for a, b in zip(D[1:], Dr[1:])) and all(np.array_equal(a, b) for a, b in zip(P[1:], Pr[1:]))
    assert np.array_equal(D[1], np.eye(p)) and np.array_equal(D[2], s * np.eye(p) + np.eye(p))
    E, Er = bn.update22_tables(S, x2, 0, p), bc.update22_tables(S, x2, 0, p)
    assert all(np.array_equal(a, b) for a, b in zip(E[1:], Er[1:])) and np.array_equal(E[1][:, 0], x2)


def test_argument_checks_need_no_device():
    nep = na.nep_gallery("dep0", 40)
    with pytest.raises(ValueError, match="1 <= p <= 32"):
        na.blocknewton(nep, S=np.zeros((33, 33)), X=np.eye(40, 33))
    with pytest.raises(ValueError, match="bordered"):
        na.blocknewton(nep, bordered="schur")
    with pytest.raises(ValueError, match="X must be"):
        na.blocknewton(nep, S=np.zeros((3, 3)), X=np.eye(40, 2))
    with pytest.raises(ValueError, match="square"):
        na.blocknewton(nep, S=np.zeros((2, 3)))
    other = na.Mder_NEP(40, lambda lam, i=0: np.eye(40) * lam)
    with pytest.raises(TypeError, match="SPMF"):
        na.blocknewton(other)
    S, X, n, p = bn.check_arguments(nep, None, None, "eliminate", 2)
    assert (n, p) == (40, 2) and np.array_equal(S, np.zeros((2, 2))) and np.array_equal(X, np.eye(40, 2)) and X.dtype == complex


def test_signature_matches_the_issue():
    import inspect
    sig = inspect.signature(na.blocknewton)
    names = list(sig.parameters)
    assert names[:10] == ["nep", "S", "X", "errmeasure", "tol", "maxit", "logger", "armijo_factor", "armijo_max", "linsolvercreator"]
    d = {k: v.default for k, v in sig.parameters.items()}
    assert d["tol"] == EPS * 100 and d["maxit"] == 10 and d["armijo_factor"] == 1 and d["armijo_max"] == 5
    assert d["bordered"] == "eliminate" and d["refine"] == 2 and d["info"] is None
    assert sig.parameters["linsolvercreator"].kind is inspect.Parameter.KEYWORD_ONLY
