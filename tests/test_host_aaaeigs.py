"""Host-side tests of AAAeigs: the checker that test_gpu_aaaeigs.py runs on nep_cork_expand (it passes the NumPy implementation and
rejects its mutants), the compact pencils and the per-shift tables of the device iteration against the straightforward forms of
src/method_AAAeigs.jl, and svAAA / reval against a dense restatement (tests/cork_checkers.py)."""
import os
import re
from functools import partial

import numpy as np
import pytest
import scipy.sparse as sp

import nep_amd as na
from nep_amd import aaaeigs as aa, funcs
import cork_checkers as cc
import primitive_checkers as pc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = np.finfo(float).eps
TOL_APPR = EPS * 1e3
CIRCLE = np.exp(1j * np.pi * np.arange(0.0, 2.0 + 1e-9, 0.01))          # exp(i pi (0:0.01:2))


# ---- the checker of nep_cork_expand ---------------------------------------------------------------------------------------------
def test_numpy_implementation_passes_every_case():
    n = 0
    for c in cc.CORK.cases():
        cc.CORK.check(cc.CORK.ref, c)
        n += 1
    assert 200 <= n <= 260, n
    print("%s: %d cases, largest |impl - ref| / bound = %.3g" % (cc.CORK.name, n, pc.RATIOS.get(cc.CORK.name, 0.0)))


@pytest.mark.parametrize("mut", cc.CORK.mutants)
def test_checker_rejects_mutant(mut):
    """alpha taken as 1, the rank-1 term left out, g conjugated, G transposed, the last term of the sum dropped, the last row not
    written, the entry behind the block written, one real part off by one ulp: some case fails on each"""
    ratios = dict(pc.RATIOS)
    impl = partial(cc.CORK.ref, mut=mut)
    rejected = None
    for c in cc.CORK.cases():
        if mut in cc.CORK.exact_only_mutants and c.kind != "exact":
            continue
        try:
            cc.CORK.check(impl, c)
        except AssertionError:
            rejected = c
            break
    pc.RATIOS.clear(); pc.RATIOS.update(ratios)
    assert rejected is not None, "no case rejects the mutant %r" % mut


def test_case_list_covers_the_shapes():
    sh = list(cc.CORK.shapes())
    assert {(r, k, c) for r, k, c, *_ in sh} >= {(r, k, c) for r in cc.CK_R for k in cc.CK_K for c in (1, 3, 4, k)}
    for kind in ("exact", "rounded"):
        mine = [s for s in sh if s[3] == kind]
        assert {s[4] for s in mine} == {True, False}                      # with and without the rank-1 term
        assert {s[5] == 1.0 for s in mine if s[4]} == {True, False}       # alpha = 1 and a complex alpha, where alpha is used
        assert {s[6] > 0 for s in mine} == {True, False} and {s[7] > 0 for s in mine} == {True, False}      # ldu, ldo padding
        assert {s[0] for s in mine} == set(cc.CK_R) and {s[1] for s in mine} == set(cc.CK_K)


# ---- the compact pencil and the tables of a shift -------------------------------------------------------------------------------
PENCILS = {"no_polynomial": (0, []), "constant_only": (0, [0]), "linear": (1, [0, 1]), "cubic_with_a_gap": (3, [0, 2, 3]),
           "leading_only": (2, [2])}


def _random_pencil_data(seed, m, s):
    rng = np.random.default_rng(seed)
    g = lambda *sh: rng.standard_normal(sh) + 1j * rng.standard_normal(sh)
    w = g(m)
    return g(m), g(m, s), w / np.linalg.norm(w)


@pytest.mark.parametrize("shape", sorted(PENCILS))
def test_compact_pencil_against_the_restatement(shape):
    d, NNZ = PENCILS[shape]
    for m, s in ((2, 1), (7, 3), (19, 2)):
        z, fz, w = _random_pencil_data(5 + m, m, s)
        A, B = aa.get_compact_pencil(d, s, m, z, fz, w, NNZ)
        Ar, Br = cc.ref_compact_pencil(d, s, m, z, fz, w, NNZ)
        k = d + m + (1 if d == 0 and NNZ else 0)
        assert A.shape == B.shape == (k, len(NNZ) + s + k - 1)
        assert np.array_equal(np.asarray(A), Ar) and np.array_equal(np.asarray(B), Br)


@pytest.mark.parametrize("shape", sorted(PENCILS))
def test_fused_tables_against_the_solve_with_the_extended_pencil(shape):
    """u_c = U C_sigma and Uhat = u1 g_sigma^T + U G_sigma against U (B [I; Y[2:end, :]]) and [u1, U B[:, l+1:end]] / Mext of
    :276-287,332-339.  Both routes solve with Mext, one through its inverse: they agree to a small multiple of cond(Mext) eps."""
    d, NNZ = PENCILS[shape]
    m, s, r = 9, 2, 6
    z, fz, w = _random_pencil_data(31, m, s)
    A, B = cc.ref_compact_pencil(d, s, m, z, fz, w, NNZ)
    k, l = A.shape[0], len(NNZ) + s
    rng = np.random.default_rng(7)
    Uj = rng.standard_normal((r, k)) + 1j * rng.standard_normal((r, k))
    u1 = rng.standard_normal(r) + 1j * rng.standard_normal(r)
    for sigma in (0.3 - 0.2j, -1.5 + 0.0j):
        Cs, gs, Gs = aa.cork_shift_tables(A, B, l, sigma)
        assert Cs.shape == (k, l) and gs.shape == (k,) and Gs.shape == (k, k)
        Cfull, right_div = cc.ref_level2_tables(A, B, l, sigma)
        cond = np.linalg.cond(np.hstack([np.eye(k, 1), A[:, l:] - sigma * B[:, l:]]))
        W = np.hstack([u1[:, None], Uj @ B[:, l:]])
        for got, want in ((Uj @ Cs, Uj @ Cfull), (np.outer(u1, gs) + Uj @ Gs, right_div(W))):
            err = np.linalg.norm(got - want) / np.linalg.norm(want)
            print("%s sigma=%r cond %.3g: relative difference %.3g" % (shape, sigma, cond, err))
            assert err <= 100 * EPS * cond


def test_pencil_recognises_the_polynomial_part():
    rng = np.random.default_rng(3)
    Ms = [rng.standard_normal((4, 4)) for _ in range(4)]
    nl = na.SPMF_NEP([Ms[3]], [funcs.Exp(-1.0)])
    is_ = aa.AAACorkLinearization(2 * CIRCLE)
    for nep, swapped in ((na.SumNEP(na.PEP([Ms[0], Ms[1]]), nl), False), (na.SumNEP(nl, na.PEP([Ms[0], Ms[1]])), True)):
        L = aa.AAAPencil(nep, is_)
        assert (L.d, L.s, L.NNZ) == (1, 1, [0, 1]) and L.m == len(L.zfw[0]) and L.same_terms == (not swapped)
        assert L.PPCC[0] is nep.get_Av()[1 if swapped else 0] and L.PPCC[2] is nl.get_Av()[0]
    Zero = np.zeros((4, 4))
    L = aa.AAAPencil(na.SumNEP(na.PEP([Ms[0], Zero, Ms[2], Zero]), nl), is_)          # a gap and a trailing zero
    assert (L.d, L.NNZ, len(L.PPCC)) == (2, [0, 2], 3) and not L.same_terms
    assert L.compactA.shape == (2 + L.m, 2 + 1 + 2 + L.m - 1)
    L = aa.AAAPencil(na.SumNEP(na.PEP([Ms[0]]), nl), is_)                              # constant polynomial part only
    assert (L.d, L.NNZ) == (0, [0]) and L.compactA.shape == (1 + L.m, 1 + 1 + L.m)
    L = aa.AAAPencil(na.DEP([Ms[0], Ms[1]]), is_)                                      # every other AbstractSPMF: fully nonlinear
    assert (L.d, L.s, L.NNZ) == (0, 3, []) and L.compactA.shape == (L.m, 3 + L.m - 1) and L.same_terms


# ---- svAAA and reval ------------------------------------------------------------------------------------------------------------
DEP0_FV = [lambda l: -l, lambda l: np.ones_like(l), lambda l: np.exp(-l)]


@pytest.fixture(scope="module")
def dep0():
    nep = na.nep_gallery("dep0")
    return nep, [np.asarray(A.toarray() if sp.issparse(A) else A, dtype=complex) for A in nep.get_Av()]


def _interior_points():
    rng = np.random.default_rng(2022)
    return 1.8 * np.sqrt(rng.random(50)) * np.exp(2j * np.pi * rng.random(50))


def _relative_error(fvals, rvals, scale):
    return float(np.max(np.abs(rvals - fvals) / scale[None, :]))


@pytest.mark.parametrize("weighted", [False, True], ids=["set_valued", "weighted"])
def test_svAAA_on_dep0(dep0, weighted):
    nep, Av = dep0
    Z = 2 * CIRCLE
    z, fz, w, err, pol, rsd, zer = na.svAAA(nep, Z, weighted=weighted)
    m = len(z)
    assert fz.shape == (m, 3) and w.shape == (m,) and len(err) >= m and len(pol) == 0
    assert all(np.any(zz == Z) for zz in z)
    fz_direct = np.column_stack([f(z) for f in DEP0_FV])                  # (the samples are scaled and scaled back: two roundings)
    assert np.all(np.abs(fz - fz_direct) <= 4 * EPS * np.abs(fz_direct))
    print("m = %d, errors %s" % (m, err))
    assert err[-1] <= TOL_APPR
    zr, fzr, wr, errr = cc.ref_svAAA(DEP0_FV, Z, weighted=weighted, Av=Av)
    assert errr[-1] <= TOL_APPR
    lam = _interior_points()
    F = np.column_stack([f(lam) for f in DEP0_FV])
    scale = np.max(np.abs(np.column_stack([f(Z) for f in DEP0_FV])), axis=0)
    mine = _relative_error(F, aa.reval(lam, z, fz, w), scale)
    theirs = _relative_error(F, cc.ref_reval(lam, zr, fzr, wr), scale)
    print("relative error at 50 interior points: %.3g, restatement (m = %d) %.3g" % (mine, len(zr), theirs))
    assert mine <= 10 * theirs + TOL_APPR


def test_reval_at_a_support_point_and_at_infinity(dep0):
    nep, _ = dep0
    z, fz, w, *_ = na.svAAA(nep, 2 * CIRCLE)
    lam = np.array([z[2], np.inf, 0.3 + 0.1j, np.nan, z[0]])
    r = aa.reval(lam, z, fz, w)
    assert r.shape == (5, 3)
    assert np.array_equal(r[0], fz[2]) and np.array_equal(r[4], fz[0])
    assert np.allclose(r[1], np.sum(w[:, None] * fz, axis=0) / np.sum(w), rtol=1e-14, atol=0)
    assert np.allclose(r[2], cc.ref_reval(lam[2:3], z, fz, w)[0], rtol=1e-13, atol=0)
    assert np.all(np.isnan(r[3]))


@pytest.mark.parametrize("weighted", [False, True], ids=["set_valued", "weighted"])
def test_cleanup_removes_a_froissart_doublet(weighted):
    """1 / (lam - 3) is a rational function of type (0, 1): two support points represent it exactly.  With tol = 0 the iteration goes on;
    the third support point brings a pole whose residue is rounding noise (a Froissart doublet).  The cleanup detects it, removes
    the support point next to it, recomputes the weights from the Loewner matrix and stops; without the cleanup the iteration runs
    to mmax and leaves mmax - 2 spurious poles."""
    nep = na.SPMF_NEP([np.eye(2)], [funcs.Resolvent(funcs.one(), 3.0)])
    z, fz, w, err, pol, rsd, zer = na.svAAA(nep, 2 * CIRCLE, tol=0.0, cleanup=True, tol_cln=1e-8, mmax=12, return_details=True,
                                            weighted=weighted)
    print("with cleanup: m = %d, errors %s, poles %s" % (len(z), err, pol))
    assert len(z) == 2 and len(err) == 4 and err[-1] <= 1e-13
    assert len(pol) == 1 and abs(pol[0] - 3.0) <= 1e-10 and abs(rsd[0, 0] - 1.0) <= 1e-6 and zer.shape == (3, 1)
    lam = np.array([0.2 + 0.1j, -1.0 + 0.5j])
    assert np.allclose(aa.reval(lam, z, fz, w)[:, 0], 1.0 / (lam - 3.0), rtol=1e-12, atol=0)
    z2, fz2, w2, err2, pol2, rsd2, _ = na.svAAA(nep, 2 * CIRCLE, tol=0.0, cleanup=False, mmax=12, return_details=True, weighted=weighted)
    assert len(z2) == 12 and len(err2) == 13
    assert int(np.sum(np.abs(rsd2[:, 0]) < 1e-8)) == len(pol2) - 1 >= 8


# ---- the public surface ---------------------------------------------------------------------------------------------------------
def test_header_declares_the_cork_kernel_and_the_package_exports_the_solver():
    hdr = open(os.path.join(ROOT, "include", "nepmi355.h")).read()
    assert re.search(r"int32_t\s+nep_cork_expand\s*\(int32_t r, int32_t k, int32_t c,", hdr)
    assert "src/method_AAAeigs.jl:283-287,332-339" in hdr
    assert "nep_cork_expand" in na._lib.SIGNATURES
    for name in ("AAAeigs", "svAAA", "AAASolutionDetails"):
        assert hasattr(na, name), name
    d = na.AAASolutionDetails()
    assert d.m_appr == 0 and d.conv_it == 0 and d.Lam.shape == (0, 0)


def test_a_linearisation_wider_than_the_kernel_is_refused_by_name():
    """k = d + m > 256 (a polynomial part of degree 250 and some ten support points): refused on the host, before any device
    state exists"""
    I4, Zero = np.eye(4), np.zeros((4, 4))
    nep = na.SumNEP(na.PEP([I4] + [Zero] * 249 + [I4]), na.SPMF_NEP([np.diag([1.0, 2.0, 3.0, 4.0])], [funcs.Exp(-1.0)]))
    with pytest.raises(ValueError, match="mmax"):
        na.AAAeigs(nep, 2 * CIRCLE)
