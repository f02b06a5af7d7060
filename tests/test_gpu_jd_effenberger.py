"""jd_effenberger on the device: nep_defl_border (csrc/deflate_border.hip) through the raw C ABI on the cases of
tests/border_checkers.py, DeflatedNEPLinSolver (one solve with the original matrix + the border kernel) against the bordered matrix
of the deflated NEP, and the driver as test/jd.jl:64-88 runs it, against the dense restatement of src/method_jd.jl:216-438."""
import ctypes as C
import math
import types

import numpy as np
import pytest
import scipy.sparse as sp
import torch

import border_checkers as bc
import deflation_checkers as dc
import primitive_checkers as pc

pytestmark = pytest.mark.gpu
SQEPS = math.sqrt(np.finfo(float).eps)
MODES = ["Generic", "SPMF", "MM"]
SIGMA = 0.3 + 0.2j


@pytest.fixture(scope="module")
def na():
    import nep_amd
    if nep_amd.device_count() < 1:
        pytest.skip("no GPU")
    return nep_amd


# ---- nep_defl_border through the C ABI ------------------------------------------------------------------------------------------
def _border_raw(n0, p, X, ldx, Y, b2, T, scale, out, null=(), b2_inside_out=False):
    from nep_amd import _lib
    from nep_amd.nep import stream_ptr
    up = lambda b: torch.from_numpy(np.ascontiguousarray(b)).to("cuda")
    Xd, outd = up(X), up(out)
    Yd = None if Y is None else up(Y)
    b2d = None if b2 is None else up(b2)
    pout = outd.data_ptr() + 16 * bc.LEAD
    py = pout if Y is None else Yd.data_ptr()
    pb2 = None if b2d is None else b2d.data_ptr()
    if b2_inside_out:
        pb2 = pout + 16 * (n0 - 1)
    ptr = lambda name, v: None if name in null else C.c_void_p(v)
    rc = _lib.lib.nep_defl_border(n0, p, ptr("X", Xd.data_ptr()), ldx, ptr("Y", py), None if pb2 is None else C.c_void_p(pb2),
                                  None if "T" in null else _lib.hptr(T), float(scale), ptr("out", pout), stream_ptr())
    torch.cuda.synchronize()
    assert np.array_equal(Xd.cpu().numpy(), X, equal_nan=True), "dX was modified"
    assert Yd is None or np.array_equal(Yd.cpu().numpy(), Y), "dY was modified"
    assert b2d is None or np.array_equal(b2d.cpu().numpy(), b2), "db2 was modified"
    return rc, outd.cpu().numpy()


def _impl(**a):
    rc, out = _border_raw(**a)
    assert rc == 0, rc
    return out


CASES = list(bc.BORDER.cases())


@pytest.mark.parametrize("case", CASES, ids=[repr(c) for c in CASES])
def test_defl_border_case(na, case):
    bc.BORDER.check(_impl, case)
    print("%r: largest |impl - ref| / bound so far = %.3g" % (case, pc.RATIOS.get(bc.BORDER.name, 0.0)))


def test_defl_border_two_calls_give_the_same_bits(na):
    picked = [c for c in CASES if c.kind == "rounded"][::4]
    assert len(picked) >= 5
    for c in picked:
        a = c.args
        assert _impl(**a).tobytes() == _impl(**a).tobytes(), c


def test_defl_border_error_codes_launch_nothing(na):
    from nep_amd import _lib
    base = bc.DeflBorder._build(65, 3, "exact", 3, False, True, -1.0)
    bad = [({"p": 0}, {}, _lib.NEP_ERR_UNSUPPORTED), ({"p": 33}, {}, _lib.NEP_ERR_UNSUPPORTED),
           ({"ldx": 64}, {}, _lib.NEP_ERR_ARG), ({"n0": 0}, {}, _lib.NEP_ERR_ARG),
           ({}, {"null": ("X",)}, _lib.NEP_ERR_ARG), ({}, {"null": ("Y",)}, _lib.NEP_ERR_ARG), ({}, {"null": ("T",)}, _lib.NEP_ERR_ARG),
           ({}, {"null": ("out",)}, _lib.NEP_ERR_ARG), ({}, {"b2_inside_out": True}, _lib.NEP_ERR_ARG)]
    for change, how, want in bad:
        rc, out = _border_raw(**dict(base, **change), **how)
        assert rc == want, (change, how, rc)
        assert np.array_equal(out, base["out"], equal_nan=True), (change, how)
    rc, out = _border_raw(**base)                                       # the unchanged call is accepted
    assert rc == 0 and not np.isnan(out[bc.LEAD: bc.LEAD + 68]).any()


# ---- the composed route (p > 32) ------------------------------------------------------------------------------------------------
def _composed_impl(na, n0, p, X, ldx, Y, b2, T, scale, out):
    """DeflatedNEPLinSolver._border_composed on the operands of a checker case (X without padding rows)"""
    assert ldx == n0
    stub = types.SimpleNamespace(n0=n0, p=p, n=n0 + p, V0=X.reshape(p, n0).T, S0=np.zeros((p, p)))
    solver = na.DeflatedNEPLinSolver(stub, 0.0, None)
    x = torch.from_numpy(out[bc.LEAD: bc.LEAD + n0 + p].copy()).to("cuda")
    if Y is not None:
        x[:n0] = torch.from_numpy(Y).to("cuda")
    b2d = None if b2 is None else torch.from_numpy(b2).to("cuda")
    solver._border_composed(x, b2d, T.reshape(p, p).T, scale)
    torch.cuda.synchronize()
    res = out.copy()
    res[bc.LEAD: bc.LEAD + n0 + p] = x.cpu().numpy()
    return res


def test_composed_route_against_the_reference_and_the_kernel(na):
    """p = 33 is outside nep_defl_border's limit: the composed route is held to the checker's bound (which allows any summation
    order, on the vector ALU or the matrix cores).  At p = 3 both routes lie within that bound of the exact result, so they differ
    by at most twice the bound."""
    big = pc.Case("n257", "p33_composed", "rounded", lambda: bc.DeflBorder._build(257, 33, "rounded", 0, False, True, -1.0))
    bc.BORDER.check(lambda **a: _composed_impl(na, **a), big)
    rc, out = _border_raw(**big.args)
    assert rc == na._lib.NEP_ERR_UNSUPPORTED and np.array_equal(out, big.args["out"], equal_nan=True)
    a = bc.DeflBorder._build(257, 3, "rounded", 0, True, True, -1.0)
    bc.BORDER.check(lambda **kw: _composed_impl(na, **kw), pc.Case("n257", "p3_composed", "rounded", lambda: a))
    blk = slice(bc.LEAD, bc.LEAD + 260)
    _, bound = bc.BORDER.reference_and_bound(a)
    diff = np.abs(_composed_impl(na, **a)[blk] - _impl(**a)[blk])
    print("composed vs kernel: largest difference / (2 bound) = %.3g" % float(np.max(diff / (2 * bound))))
    assert np.all(diff <= 2 * bound)


# ---- DeflatedNEPLinSolver -------------------------------------------------------------------------------------------------------
def _dense(M):
    return M.toarray() if sp.issparse(M) else np.asarray(M)


@pytest.fixture(scope="module")
def sparse100(na):
    """dep0_sparse(100) with 1, 2 and 3 pairs deflated in each of the three modes: the pairs by augnewton from 0.2 + 0.5i with
    v = ones on the "Generic" chain, the same pairs deflated in the other two modes"""
    nep = na.nep_gallery("dep0_sparse", 100)
    out = {"nep": nep, "Generic": [], "SPMF": [], "MM": []}
    g = s = m = nep
    for i in range(3):
        lam, v = na.augnewton(g, lam=0.2 + 0.5j, v=np.ones(100 + i), tol=1e-10, maxit=100)
        g = na.deflate_eigpair(g, lam, v, mode="Generic"); s = na.deflate_eigpair(s, lam, v, mode="SPMF")
        m = na.deflate_eigpair(m, lam, v, mode="MM")
        out["Generic"].append(g); out["SPMF"].append(s); out["MM"].append(m)
    return out


def _assert_solves(Mt, x, b, what):
    r = np.linalg.norm(Mt @ x - b)
    lim = 1e-10 * np.linalg.norm(Mt, 1) * np.linalg.norm(x)
    print("%s: residual %.3g, limit %.3g" % (what, r, lim))
    assert np.all(np.isfinite(x)) and r <= lim, what


@pytest.mark.parametrize("pairs", [1, 2, 3])
@pytest.mark.parametrize("mode", MODES)
def test_deflated_linsolver_solves_the_bordered_system(na, sparse100, mode, pairs):
    d = sparse100[mode][pairs - 1]
    n = 100 + pairs
    assert d.size(1) == n and d.p == pairs
    Mt = _dense(d.compute_Mder(SIGMA))
    rng = np.random.default_rng(23 + pairs)
    b = rng.standard_normal(n) + 1j * rng.standard_normal(n)
    solver = na.create_linsolver(na.DeflatedNEPLinSolverCreator(), d, SIGMA)
    assert isinstance(solver, na.DeflatedNEPLinSolver) and solver.deflated_nep is d
    x = na.lin_solve(solver, b)
    assert isinstance(x, np.ndarray) and x.shape == (n,)
    _assert_solves(Mt, x, b, "NumPy in")
    bd = na.to_dev(b)[0]
    before = bd.clone()
    xd = na.lin_solve(solver, bd)
    assert torch.is_tensor(xd) and xd.is_cuda and xd.shape == (n,) and torch.equal(bd, before)
    _assert_solves(Mt, xd.cpu().numpy(), b, "device tensor in")
    xm = na.lin_solve(solver, b, scale=-1.0)
    _assert_solves(Mt, -xm, b, "scale = -1")
    ret = solver.solve_dev(bd, out=bd)                                  # out aliasing b
    assert ret.data_ptr() == bd.data_ptr()
    _assert_solves(Mt, bd.cpu().numpy(), b, "out is b")


def test_one_lin_solve_is_one_solve_of_the_original_solver(na, sparse100):
    nep, d = sparse100["nep"], sparse100["SPMF"][2]

    class Counting(na.LinSolver):
        def __init__(self, inner):
            self.inner, self.calls = inner, 0

        def solve_dev(self, b, out=None, scale=1.0):
            self.calls += 1
            assert b.numel() == 100 and out is not None and out.numel() == 100
            return self.inner.solve_dev(b, out=out, scale=scale)

    org = Counting(na.create_linsolver(na.DefaultLinSolverCreator(), nep, SIGMA))
    solver = na.DeflatedNEPLinSolver(d, SIGMA, org)
    b = np.arange(1.0, 104.0) * (1 - 0.5j)
    x = na.lin_solve(solver, b)
    assert org.calls == 1
    _assert_solves(_dense(d.compute_Mder(SIGMA)), x, b, "counting stub")


def test_creator_refuses_a_plain_nep(na, sparse100):
    with pytest.raises(TypeError):
        na.create_linsolver(na.DeflatedNEPLinSolverCreator(), sparse100["nep"], SIGMA)


# ---- jd_effenberger: mirror of test/jd.jl:64-88 ---------------------------------------------------------------------------------
def _host_residual(nep, lam, x):
    """ResidualErrmeasure ||M(lam) x|| / ||x|| with M(lam) assembled on the host"""
    return np.linalg.norm(_dense(nep.compute_Mder(lam)) @ x) / np.linalg.norm(x)


def _assert_eigenpairs(nep, D, V, count, tol):
    n = nep.size(1)
    assert len(D) == count and V.shape == (n, count)
    for i in range(count):
        for j in range(i):
            assert abs(D[i] - D[j]) / abs(D[i]) > SQEPS, (D[i], D[j])
    res = [_host_residual(nep, l, v) for l, v in zip(D, V.T)]
    print("eigenvalues", D, "residuals", res)
    assert max(res) < tol


@pytest.fixture(scope="module")
def dep60(na):
    nep = na.nep_gallery("dep0_sparse", 60)
    np.random.seed(0)
    D, V = na.jd_effenberger(nep, neigs=3, maxit=55, lam=0.6, v=np.ones(60), tol=1e-10)
    return nep, D, V


def test_jd_effenberger_dep0_sparse(na, dep60):
    """test/jd.jl:70-74 on dep0_sparse(60).  The device run and the dense restatement find different, equally valid sets: the
    driver's default inner solvers (iar_chebyshev on the projected DEP, augnewton on the projected deflated problems) differ from
    the restatement's Newton from random starts, and Jacobi-Davidson converges to whichever Ritz value near the target the inner
    solver hands it.  Seen on an MI355X: 0.10648405, -0.07878992 - 0.23251491i, 0.56666615 + 0.13820884i (residuals <= 5.1e-11)
    against the restatement's 0.67329534, 0.10648405, 1.23876417.  So the pairs are held to the residual bound only, each set on
    its own; the restatement's set is printed beside the device's."""
    nep, D, V = dep60
    _assert_eigenpairs(nep, D, V, 3, 1e-10)
    np.random.seed(0)
    ref = dc.ref_dep(nep.A[0].toarray(), nep.A[1].toarray())
    Dr, Vr, its = bc.ref_jd_effenberger(ref, neigs=3, maxit=55, lam=0.6, v=np.ones(60), tol=1e-10)
    print("restatement (%d iterations):" % its, Dr)
    assert len(Dr) == 3 and max(_host_residual(nep, l, x) for l, x in zip(Dr, Vr.T)) < 1e-10


def test_jd_effenberger_pep0(na):
    """test/jd.jl:64-68 on pep0(250).  As on dep0_sparse, the device run and the dense restatement find different, equally valid
    sets (the driver solves the projected PEP with polyeig and the projected deflated problems with augnewton, the restatement
    uses Newton from random starts throughout): seen on an MI355X: 0.04639788,
    -0.04792986 + 0.08004332i, -0.46498026 + 0.19822252i, 0.24876713 - 0.13097057i, -0.41070351 - 0.80835009i (residuals <= 8.3e-11)
    against the restatement's 0.4961174 + 0.35761031i, -0.41166091 - 0.15740431i, 0.12736938 + 0.56019665i,
    -0.27233647 + 0.9745334i, -0.30280571 - 0.5568072i; no eigenvalue is common to the two sets.
    So the pairs are held to the residual bound only, each set on its own; the restatement's set is printed beside the device's."""
    nep = na.nep_gallery("pep0", 250)
    np.random.seed(0)
    D, V = na.jd_effenberger(nep, neigs=5, maxit=80, lam=0.82 + 0.9j, v=np.ones(250), tol=1e-10)
    _assert_eigenpairs(nep, D, V, 5, 1e-10)
    np.random.seed(0)
    Dr, Vr, its = bc.ref_jd_effenberger(bc.ref_pep([_dense(A) for A in nep.get_Av()]), neigs=5, maxit=80, lam=0.82 + 0.9j,
                                        v=np.ones(250), tol=1e-10)
    print("restatement (%d iterations):" % its, Dr)
    print("device eigenvalues with no restatement eigenvalue within 1e-8:", [l for l in D if min(abs(Dr - l)) >= 1e-8])
    assert len(Dr) == 5 and max(_host_residual(nep, l, x) for l, x in zip(Dr, Vr.T)) < 1e-10


def test_jd_effenberger_converged_start_returns_at_once(na, dep60):
    """test/jd.jl:76-78; maxit = 0 leaves no iteration to take: the start is deflated and handed back"""
    nep, D, V = dep60
    D1, V1 = na.jd_effenberger(nep, neigs=1, maxit=0, lam=D[0], v=V[:, 0], tol=1e-10)
    assert len(D1) == 1 and abs(D1[0] - D[0]) <= 1e-14 * abs(D[0])
    _assert_eigenpairs(nep, D1, V1, 1, 1e-10)


def test_jd_effenberger_errors(na):
    nep = na.nep_gallery("pep0", 50)
    with pytest.raises(ValueError, match="larger than size of NEP"):
        na.jd_effenberger(nep, tol=1e-10, maxit=51, v=np.ones(50))
    with pytest.raises(ValueError, match="SPMF"):
        na.jd_effenberger(nep, tol=1e-10, maxit=4, v=np.ones(50), deflation_mode="Generic")
    np.random.seed(0)
    with pytest.raises(na.NoConvergenceException) as ei:
        na.jd_effenberger(nep, neigs=1000, tol=1e-10, maxit=4, v=np.ones(50), lam=10.0)
    lam, v = np.atleast_1d(ei.value.lam), np.asarray(ei.value.v)
    print("found before the iterations ran out:", lam[:-1], "current iterate", lam[-1])
    assert len(lam) >= 1 and v.shape == (50, len(lam))                  # the pairs found so far, then the current iterate
    for l, x in zip(lam[:-1], v.T[:-1]):
        assert _host_residual(nep, l, x) < SQEPS
