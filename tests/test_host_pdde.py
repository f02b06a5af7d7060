"""Host-only tests of the periodic-delay NEP: the checker of tests/pdde_checkers.py on its own NumPy evaluations (exact cases proved
exact, twelve mutants caught, the float64 evaluation inside the bound on every bounded case, a 2^-40 perturbation outside it), the
host side of nep_amd/pdde.py (term form, callables split by SVD), the Jordan-block identities against 40-digit derivatives, the
gallery, and the rand0 fixture.  No GPU."""
import math
import os

import numpy as np
import pytest

import pdde_checkers as pc
from nep_amd.gallery import nep_gallery
from nep_amd.pdde import PeriodicDDE_NEP, terms_from_callable, jordan_pair

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pdde_rand0_eigs.npz")


# ---- the checker ------------------------------------------------------------------------------------------------------------------
def test_case_lists_cover_the_issue():
    for shapes in (pc.SHAPES, pc.BOUNDED_SHAPES):
        cols = list(zip(*shapes))
        assert set(pc.NS) <= set(cols[0]) and {1, 2, 3, 8} <= set(cols[1]) and {1, 3, 20} <= set(cols[2])
        assert {(1, 1), (2, 1), (3, 2)} <= set(zip(cols[4], cols[5]))
    assert {1, 2, 3} <= set(s[3] for s in pc.SHAPES) and {1, 2, 7} <= set(s[3] for s in pc.BOUNDED_SHAPES)
    for n in pc.NS:
        assert any(s[0] == n and s[1] == 3 and s[2] == 20 for s in pc.SHAPES)


@pytest.mark.parametrize("shape", pc.SHAPES, ids=pc.case_id)
def test_exact_cases_are_exact(shape):
    """exact_case raises unless the float64 evaluation equals the integer (Fraction) evaluation entry by entry; E != exp(-tau S)"""
    prob, S, E, V, ref = pc.exact_case(shape)
    assert ref.shape == (shape[0], shape[2], shape[1]) and np.any(ref != 0)
    assert abs(E[0, 0, 0] - np.exp(-prob["tau"] * S[0, 0, 0])) > 0.5
    assert np.all(np.mod(prob["alpha"].real, 6) == 0) and np.all(np.mod(S.imag, 6) == 0)


@pytest.mark.parametrize("mutant", pc.MUTANTS)
def test_every_mutant_differs_on_an_exact_case(mutant):
    hits = [pc.case_id(s) for s in pc.SHAPES if pc.mutant_differs(s, mutant)]
    print("%s: differs on %d of %d exact cases" % (mutant, len(hits), len(pc.SHAPES)))
    assert hits


def test_float64_evaluation_passes_and_a_perturbed_table_fails():
    """the float64 evaluation is inside c u Ybar on every bounded case (largest ratio printed); with one table entry changed by a
    relative 2^-40 at least one case is outside"""
    broke = []
    for shape in pc.BOUNDED_SHAPES:
        prob, S, E, V, ref, bound = pc.bounded_case(shape)
        pc.check_bounded(shape, pc.sweep(prob, S, E, V, np.float64).c128(), "float64")
        al = prob["alpha"].copy()
        al[1, 0] *= 1 + 2.0 ** -40
        got = pc.sweep(dict(prob, alpha=al), S, E, V, np.float64).c128()
        if np.max(pc.abs_err(got, ref) / bound) > 1.0:
            broke.append(pc.case_id(shape))
    print("float64 at %.3g of the bound at most; the perturbation breaks %s" % (pc.RATIOS["float64"], broke))
    assert broke


# ---- the host side of the NEP -----------------------------------------------------------------------------------------------------
def test_term_form_construction():
    import scipy.sparse as sp
    A0 = np.array([[0.0, 1.0], [-1.0, -1.0]])
    nep = PeriodicDDE_NEP([(A0, 1.0), (sp.csc_matrix(np.eye(2)), lambda t: np.cos(np.pi * t))], [(np.ones((2, 2)), 2.0)], 2.0, N=10)
    assert nep.size() == (2, 2) and nep.N == 10 and not nep.issparse()
    assert nep.A_terms.shape == (2, 2, 2) and nep.alpha.shape == (21, 2) and nep.beta.shape == (21, 1)
    t = np.arange(21) * 0.1
    assert np.array_equal(nep.alpha[:, 0], np.ones(21)) and np.array_equal(nep.alpha[:, 1], np.cos(np.pi * t)) and np.all(nep.beta == 2)
    nep.N = 4
    assert nep.N == 4 and nep.alpha.shape == (9, 2) and np.array_equal(nep.alpha[:, 1], np.cos(np.pi * np.arange(9) * 0.25))
    with pytest.raises(ValueError):
        nep.N = 0
    with pytest.raises(ValueError):
        PeriodicDDE_NEP([(np.eye(3), 1.0)], [(np.eye(2), 1.0)], 1.0, N=4)


def test_callables_are_split_into_terms():
    """the Mathieu coefficient as a callable has rank 2; the terms and tables reproduce every sample to 1e-14; a callable whose
    samples have rank 9 raises a ValueError that names the term form"""
    A = lambda t: np.array([[0.0, 1.0], [-(1 + 0.1 * np.cos(np.pi * t)), -1.0]])
    nep = PeriodicDDE_NEP(A, lambda t: np.array([[0.0, 0.0], [0.5, 0.0]]), 2.0, N=50)
    assert nep.A_terms.shape == (2, 2, 2) and nep.B_terms.shape == (1, 2, 2)
    for s in range(101):
        assert np.max(np.abs(np.einsum("i,ijk->jk", nep.alpha[s], nep.A_terms) - A(s * 0.02))) <= 1e-14
    prob_c, prob_t = pc.problem_of(nep), pc.problem_of(nep_gallery("periodicdde", name="mathieu", N=50))
    Mc, Mt = pc.mfun(prob_c)(-0.3 + 0.2j), pc.mfun(prob_t)(-0.3 + 0.2j)
    assert np.max(np.abs(Mc - Mt)) <= 1e-13
    n = 3
    rich = lambda t: np.array([[np.cos((3 * i + j + 1) * np.pi * t) for j in range(n)] for i in range(n)])
    mats, tab = terms_from_callable(lambda t: rich(t) * (np.arange(9).reshape(3, 3) < 8), np.arange(41) / 40, n)
    assert mats.shape == (8, 3, 3)
    with pytest.raises(ValueError, match="term form"):
        PeriodicDDE_NEP(rich, rich, 2.0, N=20)
    with pytest.raises(ValueError, match="term form"):              # a 2001 x 40000 sample matrix is refused before it is sampled
        terms_from_callable(lambda t: np.zeros((200, 200)), np.arange(2001) / 1000, 200)


def _mder_mp(nep, lam, der, v):
    """M^(der)(lam) v for n = 2 by differentiating the discrete map in 40-digit arithmetic (mpmath.diff on each component)"""
    import mpmath as mp
    mp.mp.dps = 40
    N, h = nep.N, mp.mpf(nep.tau) / nep.N
    tau = mp.mpf(nep.tau)
    At = [sum((mp.matrix(nep.A_terms[i].tolist()) * mp.mpmathify(complex(nep.alpha[s, i])) for i in range(len(nep.A_terms))), mp.zeros(2))
          for s in range(2 * N + 1)]
    Bt = [sum((mp.matrix(nep.B_terms[i].tolist()) * mp.mpmathify(complex(nep.beta[s, i])) for i in range(len(nep.B_terms))), mp.zeros(2))
          for s in range(2 * N + 1)]
    v0 = mp.matrix([mp.mpmathify(complex(x)) for x in v])

    def Mv(l):
        e = mp.exp(-tau * l)
        F = lambda s, y: h * (At[s] * y + Bt[s] * y * e - y * l)
        y = v0.copy()
        for k in range(N):
            s1 = F(2 * k, y); s2 = F(2 * k + 1, y + s1 / 2); s3 = F(2 * k + 1, y + s2 / 2); s4 = F(2 * k + 2, y + s3)
            y = y + (s1 + 2 * s2 + 2 * s3 + s4) / 6
        return y - v0
    lam = mp.mpmathify(complex(lam))
    return np.array([complex(mp.diff(lambda l: Mv(l)[r], lam, der)) if der else complex(Mv(lam)[r]) for r in range(2)])


def test_jordan_block_identities():
    """on n = 2 (mathieu, N = 8): der! x column der of the Jordan-block system is M^(der)(lam) e_j, and the last column of the
    compute_Mlincomb system is sum a_j M^(j + sd) v_j, against derivatives of the discrete map taken in 40-digit arithmetic;
    tolerance 1e-11 of the largest term (mpmath.diff differences at 40 digits: its own error is far below)"""
    nep = nep_gallery("periodicdde", name="mathieu", N=8)
    prob = pc.problem_of(nep)
    lam = -0.3 + 0.4j
    for der in (0, 1, 2, 3):
        M = pc.mder_sweep(prob, lam, der).c128()
        for j in range(2):
            want = _mder_mp(nep, lam, der, np.eye(2)[j])
            assert np.max(np.abs(M[:, j] - want)) <= 1e-11 * max(1.0, np.max(np.abs(want))), (der, j)
    rng = np.random.default_rng(1)
    k, sd = 2, 1
    Vv = rng.standard_normal((2, k)) + 1j * rng.standard_normal((2, k))
    a = np.array([2.0, -1j])
    p = k + sd
    S, E = jordan_pair(lam, p, nep.tau)
    S2, E2 = pc.jordan_ld(lam, p, nep.tau)
    assert np.array_equal(S, S2) and np.max(np.abs(E - E2)) <= 4 * np.finfo(float).eps * np.max(np.abs(E2))
    W = np.zeros((2, 1, p), dtype=complex)
    for j in range(k):
        W[:, 0, p - 1 - (j + sd)] = math.factorial(j + sd) * a[j] * Vv[:, j]
    z = pc.sweep(prob, S[None], E[None], W).c128()[:, 0, p - 1]
    want = sum(a[j] * _mder_mp(nep, lam, j + sd, Vv[:, j]) for j in range(k))
    assert np.max(np.abs(z - want)) <= 1e-11 * np.max(np.abs(want))


def test_gallery_problems():
    m = nep_gallery("periodicdde", name="mathieu")
    assert isinstance(m, PeriodicDDE_NEP) and m.n == 2 and m.N == 1000 and m.tau == 2.0
    assert isinstance(nep_gallery("periodicdde"), PeriodicDDE_NEP)
    assert nep_gallery(name="dep0").size() == nep_gallery("dep0").size() == (5, 5)      # the keyword of the other problems still works
    with pytest.raises(TypeError):
        nep_gallery()
    A1 = lambda t: np.einsum("i,ijk->jk", [1.0, np.cos(np.pi * t)], m.A_terms).real
    assert np.allclose(A1(0.3), [[0, 1], [-(1 + 0.1 * np.cos(0.3 * np.pi)), -1]])
    d = nep_gallery("periodicdde", name="discont", N=20)
    assert d.A_terms.shape[0] == 3 and d.alpha[2, 2] == 0 and np.isclose(d.alpha[20, 2], (1.0 - 0.3) ** 2, rtol=1e-14)
    mi = nep_gallery("periodicdde", name="milling1_rk4")
    assert mi.N == 50 and mi.tau == 1.0 and mi.n == 2 and np.all(mi.beta[50:] == 0) and mi.beta[5, 0] != 0
    r = nep_gallery("periodicdde", name="rand0", n=24, N=16)
    assert r.n == 24 and r.A_terms.shape == (2, 24, 24) and r.B_terms.shape == (2, 24, 24) and np.all(r.alpha[:, 0] == 1)
    from nep_amd.gallery import MSWS_RNG, gen_rng_spmat
    rng = MSWS_RNG()
    A0 = gen_rng_spmat(rng, 24, 24, 0.3).toarray() - np.eye(24)
    assert np.array_equal(r.A_terms[0].real, A0)                       # the first draw is A0
    for name in ("milling1_be", "milling0", "milling", "newmilling"):
        with pytest.raises(NotImplementedError):
            nep_gallery("periodicdde", name=name)
    with pytest.raises(KeyError):
        nep_gallery("periodicdde", name="nonsense")


def test_rand0_fixture_is_reproduced():
    """tests/golden/pdde_rand0_eigs.npz: the eigenvalues of rand0 (n = 24, N = 64) inside the checker's disc, from the checker's own
    integrator, Beyn's method in NumPy and Newton polishing; regenerated here and compared to 1e-11"""
    fix = np.load(GOLDEN)
    assert complex(fix["sigma"]) == pc.RAND0_DISC["sigma"] and float(fix["radius"]) == pc.RAND0_DISC["radius"]
    eigs = pc.rand0_eigs(pc.rand0_problem(), **pc.RAND0_DISC)
    assert len(eigs) == len(fix["eigs"]) and 3 <= len(eigs) <= 8
    assert np.max(np.abs(eigs - fix["eigs"])) <= 1e-11
    assert np.all(np.abs(np.abs(eigs - pc.RAND0_DISC["sigma"]) - pc.RAND0_DISC["radius"]) > 0.05)
