"""sgiter on the device: the reference's own test (test/sgiter.jl), the sparse overdamped family on both routes of the eigen
step against the dense companion spectrum, the routes of compute_rf on one vector, and SGIterInnerSolver inside jd_betcke
(test/jd.jl:24-29)."""
import numpy as np
import pytest

import sgiter_checkers as sg

pytestmark = pytest.mark.gpu
EPS = np.finfo(float).eps


@pytest.fixture(scope="module")
def na():
    import nep_amd
    if nep_amd.device_count() < 1:
        pytest.skip("no GPU")
    return nep_amd


_SPECTRA = {}


def _spectrum(n):
    if n not in _SPECTRA:
        _SPECTRA[n] = np.sort(sg.companion_eigenvalues(sg.overdamped_matrices(n)).real)[::-1]
    return _SPECTRA[n]


def test_the_reference_test(na):
    nep = na.nep_gallery("real_quadratic")
    lam, v = na.sgiter(nep, 1, lam_min=-10, lam_max=0, lam=-10, tol=1e-12, maxit=100)
    assert isinstance(lam, float)
    assert np.linalg.norm(sg.M(sg.real_quadratic_matrices(), lam) @ v) < 1e-9
    assert abs(np.linalg.norm(v) - 1) < 1e-12
    assert lam == pytest.approx(-0.0037234422816, rel=1e-8)


@pytest.mark.parametrize("j", [1, 2])
def test_real_quadratic_without_an_interval(na, j):
    lam, v = na.sgiter(na.nep_gallery("real_quadratic"), j)
    assert lam == pytest.approx(sg.REAL_QUADRATIC_SMALLEST[j - 1], rel=1e-8)


@pytest.mark.parametrize("n,j", sorted(sg.OVERDAMPED))
def test_overdamped_family_on_both_routes(na, n, j):
    nep = na.nep_gallery("overdamped_qep_sparse", n)
    want = _spectrum(n)[j - 1]
    assert want == pytest.approx(sg.OVERDAMPED[(n, j)], rel=1e-8)
    out = {}
    for route, kw in (("device", {}), ("host", dict(eigsolvertype=na.EigenEigSolver))):
        hist = []
        lam, v = na.sgiter(nep, j, lam_min=-1.5, lam_max=0, lam=-0.5, hist=hist, **kw)
        print(route, n, j, lam, [(h["k"], "%.2e" % h["err"], h.get("steps"), h.get("device_factorized")) for h in hist])
        assert {h["route"] for h in hist} == {route} and len(hist) <= 8
        assert lam == pytest.approx(want, rel=1e-8)
        assert abs(np.linalg.norm(v) - 1) < 1e-12
        # the stopping rule: backward error ||M(lam) v|| / sum_i |lam|^i ||A_i||_F below the default tolerance 100 eps (rows of
        # at most 5 entries in 3 terms: the product itself is rounded by up to 6 eps of the same sum, here and on the device)
        Av = sg.overdamped_matrices(n)
        assert np.linalg.norm(sg.M(Av, lam) @ v) < (100 + 12) * EPS * sum(abs(lam) ** i * np.linalg.norm(A) for i, A in enumerate(Av))
        out[route] = (lam, hist)
    assert out["device"][0] == pytest.approx(out["host"][0], rel=1e-8)
    assert all(h["device_factorized"] for h in out["device"][1][1:]), [h["factorization"] for h in out["device"][1]]


def test_compute_rf_routes_on_one_vector(na):
    nep = na.nep_gallery("overdamped_qep_sparse", 65)
    Av = sg.overdamped_matrices(65)
    rng = np.random.default_rng(3)
    x = rng.standard_normal(65)
    a = np.array([x @ A @ x for A in Av])
    # PolyeigInnerSolver: all roots of the host forms, nearest the target first
    pp = na.compute_rf(nep, x, na.PolyeigInnerSolver(), target=-0.1)
    want = np.roots(a[::-1]); want = want[np.argsort(abs(want + 0.1))]
    assert pp.shape == (2,) and np.allclose(pp, want, rtol=1e-12, atol=0)
    xd = na.to_dev(x)[0]
    assert np.allclose(na.compute_rf(nep, xd, na.PolyeigInnerSolver(), target=-0.1), want, rtol=1e-12, atol=0)
    dense = na.PEP(Av)                                          # dense host matrices: plain NumPy
    assert np.allclose(na.compute_rf(dense, x, na.PolyeigInnerSolver(), target=-0.1), want, rtol=1e-12, atol=0)
    with pytest.raises(TypeError, match="PolyeigInnerSolver only handles the PEP type"):
        na.compute_rf(na.SPMF_NEP(nep.get_Av(), nep.get_fv()), x, na.PolyeigInnerSolver())
    # scalar Newton on the forms against the default path
    solver = na.ScalarNewtonInnerSolver()
    l0 = na.compute_rf(nep, x, solver)
    l1 = na.compute_rf(nep, x, solver, forms=True)
    assert l0.shape == l1.shape == (1,) and abs(l0[0] - l1[0]) <= 10 * solver.tol
    assert abs(np.polyval(a[::-1], l1[0])) <= 1e-10 * np.sum(np.abs(a) * np.abs(l1[0]) ** np.arange(3))
    y = rng.standard_normal(65)
    l2 = na.compute_rf(nep, x, solver, y=y, forms=True, lam=-0.2)
    assert abs(l2[0] - na.compute_rf(nep, x, solver, y=y, lam=-0.2)[0]) <= 10 * solver.tol
    # any other InnerSolver: the 1 x 1 projected problem
    b = np.array([y @ A @ x for A in Av])
    l3 = na.compute_rf(nep, x, na.NewtonInnerSolver(), y=y, lam=-0.2)
    assert len(l3) >= 1
    assert min(abs(np.polyval(b[::-1], l)) / np.sum(np.abs(b) * np.abs(l) ** np.arange(3)) for l in l3) <= 1e-10


def test_jd_betcke_with_sgiter_as_inner_solver(na):
    rq = na.nep_gallery("real_quadratic")
    nep = na.SPMF_NEP(rq.get_Av(), rq.get_fv())
    lam, u = na.jd_betcke(nep, projtype="Galerkin", inner_solver_method=na.SGIterInnerSolver(), v=np.ones(4), lam=0, tol=1e-10, maxit=4)
    assert lam.shape == (1,) and u.shape == (4, 1)
    # verify_lambdas(1, nep, lam, u, TOL) of test/jd.jl: one pair, ResidualErrmeasure below the tolerance
    res = np.linalg.norm(sg.M(sg.real_quadratic_matrices(), lam[0]) @ u[:, 0]) / np.linalg.norm(u[:, 0])
    print("jd_betcke + SGIterInnerSolver: lam = %r, residual %.3e" % (lam[0], res))
    assert res < 1e-10
    assert np.min(np.abs(sg.companion_eigenvalues(sg.real_quadratic_matrices()) - lam[0])) <= 1e-8 * abs(lam[0])
    with pytest.raises(ValueError, match="Need to use 'projtype' :Galerkin"):
        na.jd_betcke(nep, projtype="PetrovGalerkin", inner_solver_method=na.SGIterInnerSolver(), v=np.ones(4), maxit=4)
    with pytest.raises(ValueError, match="not accepted since deflated problem not min-max"):
        na.jd_effenberger(nep, inner_solver_method=na.SGIterInnerSolver(), v=np.ones(4), maxit=4)
