"""Host-side tests of broyden: the checker that test_gpu_broyden.py runs on nep_broyden_sweep (it passes the NumPy implementation and
rejects its mutants), the dense restatement of src/method_broyden.jl (tests/broyden_checkers.py) against the values the reference
publishes and against test/broyden.jl, its two forms against each other, and the host logic of the driver."""
import math
import warnings
from functools import partial

import numpy as np
import pytest

import importlib

import nep_amd as na
import broyden_checkers as bc
import primitive_checkers as pc

bro = importlib.import_module("nep_amd.broyden")            # (nep_amd.broyden itself is the driver function)
EPS = np.finfo(float).eps
SQEPS = math.sqrt(EPS)


# ---- the checker of nep_broyden_sweep -------------------------------------------------------------------------------------------
def test_numpy_implementation_passes_every_case():
    n = 0
    for c in bc.SWEEP.cases():
        bc.SWEEP.check(bc.SWEEP.ref, c)
        n += 1
    assert n == len(bc.BS_N) * 2 * 7 * 2, n
    print("%s: %d cases, largest |impl - ref| / bound = %.3g" % (bc.SWEEP.name, n, pc.RATIOS.get(bc.SWEEP.name, 0.0)))


@pytest.mark.parametrize("mut", bc.SWEEP.mutants)
def test_checker_rejects_mutant(mut):
    """products taken with T before the update, a0 conjugated, w not conjugated, the last partial row tile dropped, the last
    column tile dropped, the entry behind a block written, one real part off by one ulp: some case fails on each"""
    ratios = dict(pc.RATIOS)
    impl = partial(bc.SWEEP.ref, mut=mut)
    rejected = None
    for c in bc.SWEEP.cases():
        if mut in bc.SWEEP.exact_only_mutants and c.kind != "exact":
            continue
        try:
            bc.SWEEP.check(impl, c)
        except AssertionError:
            rejected = c
            break
    pc.RATIOS.clear(); pc.RATIOS.update(ratios)
    assert rejected is not None, "no case rejects the mutant %r" % mut


def test_case_list_covers_the_shapes():
    sh = list(bc.SWEEP.shapes())
    for kind in ("exact", "rounded"):
        mine = [s for s in sh if s[5] == kind]
        assert {(s[0], s[1]) for s in mine} == {(n, pad) for n in (1, 2, 63, 64, 65, 128, 193, 257, 511, 1025) for pad in (0, 3)}
        for n in bc.BS_N:
            assert {s[2:5] for s in mine if s[0] == n} == set(bc.BS_WORK) and len(bc.BS_WORK) == 7
        assert {s[6] > 0 for s in mine} == {True, False}                  # with and without a lead offset
        assert {s[7] is pc.NAN for s in mine} == {True, False}            # NaN and sentinel padding


# ---- the restatement against the reference --------------------------------------------------------------------------------------
def _ref(name, *args):
    return bc.ref_dep_of(na.nep_gallery(name, *args))


def _sigma_min(nep, lam):
    return np.linalg.svd(nep.Mder(lam), compute_uv=False)[-1]


PUBLISHED_DEP0 = (-0.15955391823299253, -0.5032087003825461 + 1.1969823800738464j, 1.2699713558173726)     # method_broyden.jl:205-214


def test_restatement_reproduces_the_published_dep0_values():
    """The first value is the reference's to 1e-10.  dep0 is real, so its eigenvalues come in conjugate pairs, and which of a pair
    and in which order levels two and three find them depends on the eigenvectors LAPACK returns for the start pair: the three
    published values are matched up to conjugation and order."""
    nep = _ref("dep0")
    it = []
    S, X, *_ = bc.ref_broyden(nep, iters=it)
    d = np.diag(S)
    print("iterations", it, "diag(S)", d)
    assert it == [30, 40, 50]
    assert abs(d[0] - PUBLISHED_DEP0[0]) < 1e-10
    left = list(d)
    for want in PUBLISHED_DEP0:
        dist = [min(abs(x - want), abs(x - np.conj(want))) for x in left]
        i = int(np.argmin(dist))
        assert dist[i] < 1e-10, (want, d)
        left.pop(i)
    for lam in d:
        assert _sigma_min(nep, lam) < 1e-13
    assert bc.pair_residual(nep, S, X) < 2e-12


def test_restatement_satisfies_the_reference_test_on_dep1():
    """test/broyden.jl:6-15"""
    nep = _ref("dep1")
    it = []
    S, X, *_ = bc.ref_broyden(nep, iters=it)
    assert it == [120, 50, 70]
    assert 1e-15 < bc.pair_residual(nep, S, X) < SQEPS and abs(S[0, 0] - 1.0) < 1e-10
    S, X, *_ = bc.ref_broyden(nep, addconj=True, pmax=5)
    lam, Y = np.linalg.eig(S)
    V = X @ Y
    assert len(lam) == 4
    for l, v in zip(lam, V.T):
        assert nep.residual(l, v) < SQEPS


@pytest.mark.parametrize("n,approx,want", [(100, "eye", [250, 210, 180]), (257, "eye", [380, 450, 430]), (100, "nep", 100), (257, "nep", 100)])
def test_restatement_converges_on_dep0_sparse(n, approx, want):
    nep = _ref("dep0_sparse", n)
    it = []
    S, X, *_ = bc.ref_broyden(nep, approxnep=nep if approx == "nep" else "eye", iters=it)
    res = bc.pair_residual(nep, S, X)
    print("n = %d from %s: iterations %r, pair residual %.3g" % (n, approx, it, res))
    assert it == want if isinstance(want, list) else max(it) <= want
    assert 1e-15 < res < 2e-12
    assert np.linalg.norm(X.conj().T @ X - np.eye(3)) < 1e-10


def test_the_two_forms_agree_on_the_first_pair_of_dep1():
    """The pending form is the same arithmetic reordered; on the first level (120 iterations) both reach the same pair.  Later
    levels may legitimately differ: Broyden trajectories are sensitive to rounding."""
    nep = _ref("dep1")
    ia, ib, drift = [], [], []
    Sa, Xa, *_ = bc.ref_broyden(nep, pmax=1, iters=ia)
    Sb, Xb, *_ = bc.ref_broyden(nep, pmax=1, form="pending", iters=ib, drift=drift)
    assert ia == ib == [120]
    assert abs(Sa[0, 0] - Sb[0, 0]) < 1e-12 and np.linalg.norm(Xa - Xb) < 1e-10
    assert len(drift) == 12 and max(drift) < 1e-12
    S, X, *_ = bc.ref_broyden(nep, form="pending")
    assert bc.pair_residual(nep, S, X) < SQEPS


def test_add_nans_and_histories():
    nep = _ref("dep0")
    S, X, T1, eh, ih = bc.ref_broyden(nep, add_nans=True)
    assert np.array_equal(T1, np.eye(5)) and len(eh) == len(ih) == 30 + 1 + 40 + 1 + 50       # :385: a NaN before levels two and three
    assert np.isnan(ih[30]) and np.isnan(eh[30]) and np.isnan(ih[71]) and np.array_equal(ih[72:], np.arange(71, 121))
    assert np.array_equal(ih[31:71], np.arange(31, 71)) and eh[29] < 1e-12


# ---- host logic of the driver ---------------------------------------------------------------------------------------------------
def test_pmax_is_clamped_with_a_warning():
    with pytest.warns(UserWarning, match="Too many eigenvalues requested"):
        assert bro.clamp_pmax(5, 3) == 3
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        assert bro.clamp_pmax(3, 3) == 3 and bro.clamp_pmax(2, 100) == 2


def test_unknown_and_unsupported_eigmethods_raise_before_any_device_work():
    nep = na.nep_gallery("dep1")
    with pytest.raises(ValueError, match="sparse eigensolver"):
        na.broyden(nep, eigmethod="eigs")
    with pytest.raises(ValueError, match="Unknown eig method"):
        na.broyden(nep, eigmethod="qr")
    with pytest.raises(ValueError, match="approxnep"):
        na.broyden(nep, "identity")
    with pytest.raises(ValueError, match="3 x 3"):
        na.broyden(nep, np.eye(4))


def test_small_system_and_step_length():
    """the host scalars of an inner iteration against the restatement's expressions (:71-86, :104-107)"""
    rng = np.random.default_rng(3)
    g = lambda *s: rng.standard_normal(s) + 1j * rng.standard_normal(s)
    CHZ, CHT = g(3, 3), g(3)
    dul = bro.small_solve(CHZ, CHT)
    assert np.allclose(CHZ @ dul, -CHT, rtol=0, atol=1e-13)
    assert bro.step_length(0.1, 0.1, 0.2) == 1.0
    assert bro.step_length(3.0, 4.0, 0.2) == pytest.approx(0.2 / 5.0)
    du, dl = g(2), g(1)[0]
    bH, nrm2 = bro.w_update_row(du, dl, 2.0)
    assert nrm2 == pytest.approx(4.0 + np.linalg.norm(du) ** 2 + abs(dl) ** 2)
    assert np.allclose(bH, np.concatenate([du.conj(), [np.conj(dl)]]) / nrm2)


def test_sweep_error_codes_without_a_device():
    """the argument checks come before any launch, so they hold on a machine without a GPU; pointers are never dereferenced"""
    import ctypes as C
    from nep_amd import _lib
    f = _lib.lib.nep_broyden_sweep
    P = lambda i: C.c_void_p(0x100000 * i)
    n = 8
    T, W, u0, a0, x, y, w, g = (P(i) for i in range(1, 9))
    ARG = _lib.NEP_ERR_ARG
    assert _lib.lib.nep_broyden_sweep_worksize(1025) == 1025 * (17 + 2) and _lib.lib.nep_broyden_sweep_worksize(0) == 0
    assert f(0, T, 8, u0, a0, x, y, w, g, W, None) == ARG
    assert f(n, T, 7, u0, a0, x, y, w, g, W, None) == ARG
    assert f(n, None, 8, u0, a0, x, y, w, g, W, None) == ARG
    assert f(n, T, 8, u0, a0, x, y, w, g, None, None) == ARG
    assert f(n, T, 8, u0, None, x, y, w, g, W, None) == ARG
    assert f(n, T, 8, None, a0, x, y, w, g, W, None) == ARG
    assert f(n, T, 8, u0, a0, x, None, w, g, W, None) == ARG
    assert f(n, T, 8, u0, a0, None, y, w, g, W, None) == ARG
    assert f(n, T, 8, u0, a0, x, y, w, None, W, None) == ARG
    assert f(n, T, 8, u0, a0, x, y, None, g, W, None) == ARG
    assert f(n, T, 8, None, None, None, None, None, None, W, None) == ARG
    for out in ("y", "g"):
        for inside in (T, C.c_void_p(T.value + 16 * (8 * 7 + 7)), W, u0, a0, x, w, C.c_void_p(x.value + 16 * 7)):
            args = dict(y=y, g=g); args[out] = inside
            assert f(n, T, 8, u0, a0, x, args["y"], w, args["g"], W, None) == ARG, (out, inside)
    assert f(n, T, 8, u0, a0, x, y, w, C.c_void_p(y.value + 16 * 7), W, None) == ARG
    assert "invalid argument" in _lib.lib.nep_last_error().decode()
