"""ChebPEP on the device: nep_interp_coeffs (csrc/interp.hip) through the raw C ABI on the cases of tests/interp_checkers.py, the
reference's own test (test/chebpep.jl), both construction routes, the delegated compute functions, interpolate and polyeig."""
import ctypes as ct

import numpy as np
import pytest
import scipy.linalg as sla
import scipy.sparse as sp
import torch
from numpy.polynomial import chebyshev as ch

import interp_checkers as ic
import primitive_checkers as pc
from test_gpu_lineig import KS_TOL                  # the tolerance eig_solve_dev is held to there

pytestmark = pytest.mark.gpu
EPS = np.finfo(float).eps


@pytest.fixture(scope="module")
def na():
    import nep_amd
    if nep_amd.device_count() < 1:
        pytest.skip("no GPU")
    return nep_amd


# ---- nep_interp_coeffs through the C ABI ----------------------------------------------------------------------------------------
def _interp_raw(E, J, K, F, ldf, fcomplex, W, pos, beta, C, ldc, null=()):
    from nep_amd import _lib
    from nep_amd.nep import stream_ptr
    up = lambda b: torch.from_numpy(np.ascontiguousarray(b)).to("cuda")
    Fd, Cd = up(F), up(C)
    pd = None if pos is None else up(np.asarray(pos, dtype=np.int32))
    Wf = np.asfortranarray(np.asarray(W, dtype=np.complex128))                      # K x J column-major
    ptr = lambda name, t: None if (name in null or t is None) else C_vp(t.data_ptr())
    rc = _lib.lib.nep_interp_coeffs(E, J, K, ptr("F", Fd), ldf, 1 if fcomplex else 0,
                                    None if "W" in null else Wf.ctypes.data_as(C_vp), ptr("pos", pd), beta,
                                    None if "C" in null else C_vp(Cd.data_ptr() + 16 * ic.LEAD), ldc, stream_ptr())
    torch.cuda.synchronize()
    assert np.array_equal(Fd.cpu().numpy(), F, equal_nan=True), "dF was modified"
    assert pd is None or np.array_equal(pd.cpu().numpy(), pos), "dpos was modified"
    return rc, Cd.cpu().numpy()


C_vp = ct.c_void_p


def _impl(**a):
    rc, out = _interp_raw(**a)
    assert rc == 0, rc
    return out


CASES = list(ic.INTERP.cases())
GROUPS = sorted({c.group for c in CASES}, key=[c.group for c in CASES].index)


@pytest.mark.parametrize("group", GROUPS)
def test_interp_coeffs_cases(na, group):
    """the 24 cases of one (E, J, K): real and complex F, beta 0 and 1, no map / a permutation / an injection, with and without
    padding, exact and rounded"""
    mine = [c for c in CASES if c.group == group]
    assert len(mine) == 24
    for c in mine:
        ic.INTERP.check(_impl, c)
    print("%s: largest |impl - ref| / bound so far = %.3g" % (group, pc.RATIOS.get(ic.INTERP.name, 0.0)))


def test_interp_coeffs_two_calls_give_the_same_bits(na):
    picked = [c for c in CASES if c.kind == "rounded"][::37]
    assert len(picked) >= 12
    for c in picked:
        a = c.args
        assert _impl(**a).tobytes() == _impl(**a).tobytes(), c


def test_interp_coeffs_error_codes_launch_nothing(na):
    from nep_amd import _lib
    UNS, ARG = _lib.NEP_ERR_UNSUPPORTED, _lib.NEP_ERR_ARG
    for J, K in ((65, 5), (5, 65), (65, 65), (0, 5), (5, 0)):
        base = ic.oversize_case(max(J, 1), max(K, 1))
        rc, out = _interp_raw(**dict(base, J=J, K=K))
        assert rc == UNS, (J, K, rc)
        assert np.array_equal(out, base["C"], equal_nan=True), (J, K)               # NaN prefill and sentinels untouched
    base = ic.InterpCoeffs._build(65, 5, 7, True, 0, "none", True, "exact")
    bad = [({"ldf": 4}, {}), ({"ldc": 6}, {}), ({"beta": 2}, {}), ({"beta": -1}, {}), ({"E": -1}, {}),
           ({}, {"null": ("F",)}), ({}, {"null": ("C",)}), ({}, {"null": ("W",)})]
    for change, how in bad:
        rc, out = _interp_raw(**dict(base, **change), **how)
        assert rc == ARG, (change, how, rc)
        assert np.array_equal(out, base["C"], equal_nan=True), (change, how)
    rc, out = _interp_raw(**dict(base, E=0))                                        # E = 0: accepted, nothing happens
    assert rc == 0 and np.array_equal(out, base["C"], equal_nan=True)
    rc, out = _interp_raw(**base)
    assert rc == 0
    ic.INTERP.check(lambda **a: out, pc.Case("E65_J5_K7", "accepted", "exact", lambda: base))


# ---- helpers --------------------------------------------------------------------------------------------------------------------
def _dense(M):
    return np.asarray(M.toarray() if sp.issparse(M) else M)


def _dep_dense(nep):
    """lam -> M(lam) of a DEP with delays (0, 1) in NumPy, dense"""
    A0, A1 = _dense(nep.A[0]), _dense(nep.A[1])
    n = A0.shape[0]
    return lambda lam: -lam * np.eye(n) + A0 + A1 * np.exp(-lam)


def _cheb_deriv_values(k, a, b, lam, m):
    """[T_i^(m)(lam)] for the Chebyshev polynomials scaled to [a, b], by numpy.polynomial, and the tolerance of
    interp_checkers.cheb_tol on each"""
    x = 2 * (lam - a) / (b - a) - 1
    chain = 2 / (b - a)
    d = np.array([ch.chebval(x, ch.chebder(np.eye(k)[i], m) if m else np.eye(k)[i]) * chain ** m if m <= i else 0.0 for i in range(k)],
                 dtype=complex)
    tol = np.array([ic.cheb_tol(i, m, abs(x), chain) for i in range(k)])
    return d, tol


@pytest.fixture(scope="module")
def cp20(na):
    """ChebPEP(dep0_sparse(20), 8) with the seeded blocks as they left the constructor"""
    nep = na.nep_gallery("dep0_sparse", 20)
    cp = na.ChebPEP(nep, 8)
    return nep, cp, cp._aligned, cp._aligned_dev


# ---- the reference's own test (test/chebpep.jl) ---------------------------------------------------------------------------------
def test_reference_chebpep_test(na):
    """test/chebpep.jl with its tolerances on nep_gallery("dep0", 5) with both matrices divided by 10.
    Measured on an MI355X: see the figures printed below (recorded in DESIGN.md)."""
    nep = na.nep_gallery("dep0", 5)
    nep = na.DEP([A / 10 for A in nep.A])
    n = nep.size(1)
    chebpep = na.ChebPEP(nep, 13, -1, 1)
    assert (chebpep.n, chebpep.a, chebpep.b, chebpep.k) == (5, -1.0, 1.0, 13)
    assert not chebpep.issparse() and all(not np.iscomplexobj(B) for B in chebpep.get_Av())
    # k odd and a symmetric interval: 0 is an interpolation point
    e1 = np.linalg.norm(_dense(nep.compute_Mder(0)) - _dense(chebpep.compute_Mder(0)))
    print("||M(0) - P(0)|| = %.3g = %.3g of the bound" % (e1, e1 / (100 * EPS)))
    assert e1 < EPS * 100
    lam2, V2, _ = na.iar(chebpep, neigs=2, errmeasure=na.ResidualErrmeasure(chebpep), v=np.ones(n))
    e2 = np.linalg.norm(nep.compute_Mlincomb(lam2[0], V2[:, 0]))
    print("iar on the ChebPEP: ||M_org(lam_1) v_1|| = %.3g = %.3g of the bound" % (e2, e2 / (5000 * EPS)))
    assert e2 < EPS * 5000
    chebpep = na.ChebPEP(nep, 16, -0.9, 1.5)
    lam, V = na.polyeig(chebpep)
    assert lam.shape == (n * 15,) and V.shape == (n, n * 15)
    j = int(np.argmin(np.abs(lam)))
    e3 = np.linalg.norm(nep.compute_Mlincomb(lam[j], V[:, j] / np.linalg.norm(V[:, j])))
    print("polyeig: ||M_org(lam_j) v_j|| = %.3g = %.3g of the bound" % (e3, e3 / (1000 * EPS)))
    assert e3 < EPS * 1000
    for k in (1, 2):
        with pytest.raises(ValueError):
            na.polyeig(na.ChebPEP(nep, k))
    with pytest.raises(ValueError):
        na.ChebPEP(nep, 0)


# ---- the two construction routes ------------------------------------------------------------------------------------------------
def test_both_routes_agree(na, monkeypatch):
    """dep0_sparse(20): the table route (no compute_Mder call) against the sampling route of an Mder_NEP around the same
    compute_Mder.  Bound on the difference of a coefficient, with S = |D| (|W| |f(x)|)^T the sum of the absolute values of all its
    terms: the table route's kernel (m_t = 3 products) and its host table W f(x) (sums of k products), the sampling route's kernel
    (k products) and its host samples (sums of m_t products), each within cbound(number of terms, S)."""
    nep = na.nep_gallery("dep0_sparse", 20)
    k = 9
    nep._aligned_terms()
    calls = []
    orig = nep.compute_Mder                          # (on the instance: the type keeps AbstractSPMF's method, as the route test asks)
    monkeypatch.setattr(nep, "compute_Mder", lambda *a, **kw: (calls.append(a), orig(*a, **kw))[1])
    tab = na.ChebPEP(nep, k)
    assert calls == [], "the table route assembled a matrix"
    sam = na.ChebPEP(na.Mder_NEP(20, lambda lam: nep.compute_Mder(lam)), k)
    assert len(calls) == k
    monkeypatch.undo()
    for cp in (tab, sam):
        assert cp.issparse() and cp.is_real() and all(sp.issparse(B) and B.dtype == np.float64 for B in cp.get_Av())
        assert len(cp.get_Av()) == k and len(cp.get_fv()) == k and all(isinstance(f, na.funcs.Chebyshev) for f in cp.get_fv())
    (ip1, ix1, D1), (ip2, ix2, D2) = tab._aligned, sam._aligned
    ipn, ixn, Dn = nep._aligned_terms()
    assert np.array_equal(ip1, ip2) and np.array_equal(ix1, ix2) and np.array_equal(ip1, ipn) and np.array_equal(ix1, ixn)
    W = na.chebyshev_weights(-1, 1, k)
    Fx = np.column_stack([f.values(na.chebyshev_nodes(-1, 1, k)) for f in nep.get_fv()])
    S = np.abs(Dn) @ (np.abs(W) @ np.abs(Fx)).T
    bound = 2 * pc.cbound(3, S) + 2 * pc.cbound(k, S)
    ratio = float(np.max(np.abs(D1 - D2) / np.maximum(bound, np.finfo(float).tiny)))
    print("routes: largest |table - sampling| / bound = %.3g" % ratio)
    assert ratio <= 1.0
    assert np.all(D1.imag == 0) and np.all(D2.imag == 0)
    for cp in (tab, sam):                                                           # get_Av() holds the columns of the block
        for i, B in enumerate(cp.get_Av()):
            assert np.array_equal(B.indptr, ip1) and np.array_equal(B.indices, ix1) and np.array_equal(B.data, cp._aligned[2][:, i].real)


@pytest.mark.parametrize("node", [0, 2])
def test_differing_sample_patterns(na, node):
    """an Mder_NEP whose matrix lacks one entry at one node (the first one: the block starts from zeros; a later one: a row map):
    the result equals the dense NumPy route.  Bound: the kernel's and NumPy's sums of k products, cbound(k, S) each, S = sum_j
    |W[i, j]| |M(x_j)|, and the difference of the two weight tables (recurrence against the cosine formula; itself at most
    8 k eps, test_host_chebpep.py) times the samples."""
    n, k, a, b = 20, 7, -0.9, 1.5
    nep = na.nep_gallery("dep0_sparse", n)
    x = na.chebyshev_nodes(a, b, k)
    A0 = sp.csc_matrix(nep.A[0])
    r0, c0 = int(A0.indices[3]), int(np.searchsorted(A0.indptr, 3, side="right") - 1)

    def Mfun(lam):
        M = sp.lil_matrix(nep.compute_Mder(lam))
        if abs(lam - x[node]) < 1e-12:
            M[r0, c0] = 0.0
        M = sp.csc_matrix(M)
        M.eliminate_zeros()
        return M
    full = sp.csc_matrix(nep.compute_Mder(0.3))
    assert Mfun(x[node]).nnz == full.nnz - 1 and Mfun(x[(node + 1) % k]).nnz == full.nnz
    cp = na.ChebPEP(na.Mder_NEP(n, Mfun), k, a, b)
    ref = ic.ref_cheb_coefficients(lambda lam: Mfun(lam).toarray(), k, a, b)
    W, Wref = na.chebyshev_weights(a, b, k), np.array([ic.ref_cheb_T(a, b, x, i) * 2 / k for i in range(k)])
    Wref[0] *= 0.5
    assert np.max(np.abs(W - Wref)) <= 8 * k * EPS
    absS = [np.abs(Mfun(xj).toarray()) for xj in x]
    worst = 0.0
    for i, B in enumerate(cp.get_Av()):
        assert sp.issparse(B) and B.dtype == np.float64 and B.nnz == full.nnz           # the union pattern
        S = sum(abs(W[i, j]) * absS[j] for j in range(k))
        bound = 2 * pc.cbound(k, S) + sum(abs(W[i, j] - Wref[i, j]) * absS[j] for j in range(k))
        err = np.abs(B.toarray() - ref[i])
        assert np.all(err[S == 0] == 0)
        worst = max(worst, float(np.max(err[S > 0] / bound[S > 0])))
    print("differing patterns (node %d): largest |device - numpy| / bound = %.3g" % (node, worst))
    assert worst <= 1.0


# ---- delegated evaluations ------------------------------------------------------------------------------------------------------
def test_delegated_compute_functions(na, cp20):
    """compute_Mlincomb, compute_Mder, compute_MM and a factorised solve of a ChebPEP against NumPy formulas from get_Av() and
    numpy.polynomial.  Bounds: an entry of a result is a sum of N products whose absolute values add up to S, within cbound(N, S);
    the values T_i^(m)(lam) of product and reference differ by at most interp_checkers.cheb_tol, which enters through |B_i|."""
    nep, cp, aligned0, dev0 = cp20
    n, k, a, b = 20, 8, -1.0, 1.0
    Bv = [_dense(B) for B in cp.get_Av()]
    aB = [np.abs(B) for B in Bv]
    rng = np.random.default_rng(7)
    lam = 0.3 - 0.2j
    # compute_Mlincomb: sum_j a_j M^(j + 1)(lam) v_j
    V = rng.standard_normal((n, 4)) + 1j * rng.standard_normal((n, 4))
    av = np.array([1.0, -2.0, 0.5, 3.0])
    z = cp.compute_Mlincomb(lam, V, av, startder=1)
    want = np.zeros(n, dtype=complex); S = np.zeros(n); T = np.zeros(n)
    for j in range(4):
        d, tol = _cheb_deriv_values(k, a, b, lam, j + 1)
        for i in range(k):
            want += av[j] * d[i] * (Bv[i] @ V[:, j])
            S += abs(av[j]) * abs(d[i]) * (aB[i] @ np.abs(V[:, j]))
            T += abs(av[j]) * tol[i] * (aB[i] @ np.abs(V[:, j]))
    bound = 2 * pc.cbound(4 * k * (n + 1), S) + T
    r1 = float(np.max(np.abs(z - want) / bound))
    assert r1 <= 1.0, r1
    # compute_Mder(lam, 2)
    d, tol = _cheb_deriv_values(k, a, b, lam, 2)
    M2 = _dense(cp.compute_Mder(lam, 2))
    want = sum(d[i] * Bv[i] for i in range(k))
    S = sum(abs(d[i]) * aB[i] for i in range(k)); T = sum(tol[i] * aB[i] for i in range(k))
    bound = 2 * pc.cbound(k, S) + T
    assert np.all(M2[S == 0] == 0)
    r2 = float(np.max(np.abs(M2 - want)[S > 0] / bound[S > 0]))
    assert r2 <= 1.0, r2
    assert not np.iscomplexobj(cp.compute_Mder(0.25).data)                          # a real NEP at a real point
    # compute_MM with an upper-triangular, non-diagonal S: sum_i B_i V T_i(S)
    Sm = np.array([[0.2, 0.5, -0.3], [0.0, -0.4, 0.7], [0.0, 0.0, 0.1 + 0.3j]])
    Vm = rng.standard_normal((n, 3)) + 1j * rng.standard_normal((n, 3))
    Z = cp.compute_MM(Sm, Vm)
    X = (2 * Sm - (a + b) * np.eye(3)) / (b - a)
    want = np.zeros((n, 3), dtype=complex); S = np.zeros((n, 3))
    for i in range(k):
        c = ch.cheb2poly(np.eye(k)[i][:i + 1])
        TiX = sum(c[m] * np.linalg.matrix_power(X, m) for m in range(i + 1))
        absT = sum(abs(c[m]) * np.linalg.matrix_power(np.abs(X), m) for m in range(i + 1))
        want += Bv[i] @ Vm @ TiX
        S += aB[i] @ np.abs(Vm) @ absT
    bound = 2 * pc.cbound(3 * k * (n + k), S) + 2 * (3 + 3) * k * EPS * S                # the sums, and both matrix polynomials
    r3 = float(np.max(np.abs(Z - want) / bound))
    assert r3 <= 1.0, r3
    # a factorised solve at one shift: backward stable, ||P(s) x - b|| <= p(n) eps (||P(s)|| ||x|| + ||b||), p(n) taken as 10 n
    sig = 0.15
    solver = na.create_linsolver(na.FactorizeLinSolverCreator(), cp, sig)
    rhs = rng.standard_normal(n)
    xs = na.lin_solve(solver, rhs)
    P = ic.ref_cheb_eval(Bv, a, b, sig)
    res = np.linalg.norm(P @ xs - rhs)
    lim = 10 * n * EPS * (np.linalg.norm(P) * np.linalg.norm(xs) + np.linalg.norm(rhs))
    assert res <= lim, (res, lim)
    cp.compute_Mder_batch([0.1, 0.2])
    print("Mlincomb %.3g, Mder %.3g, MM %.3g of their bounds; solve residual %.3g of its bound" % (r1, r2, r3, res / lim))
    # the seeded blocks are the ones in use: nothing rebuilt a union pattern
    assert cp._aligned is aligned0 and cp._aligned_terms() is aligned0 and cp._aligned_terms()[2] is aligned0[2]
    assert cp._aligned_dev is dev0 and cp.aligned_terms_dev()[2] is dev0[0]
    assert aligned0[2].shape == (len(aligned0[1]), k) and dev0[0].shape == aligned0[2].shape
    assert np.array_equal(dev0[0].cpu().numpy(), aligned0[2])


# ---- the motivating case --------------------------------------------------------------------------------------------------------
def test_function_handle_nep_reaches_iar_through_chebpep(na):
    """an Mder_NEP without derivatives cannot run iar; its ChebPEP can.  For every returned pair
    ||M_org(lam) v|| / ||v|| <= tol_iar + 2 ||M_org(lam) - P_np(lam)||_2, P_np the interpolant built here in NumPy from the
    reference formula (the factor 2: the product's coefficients differ from NumPy's by rounding, test_both_routes_agree)."""
    n, k = 40, 20
    nep = na.nep_gallery("dep0_sparse", n)
    handle = na.Mder_NEP(n, lambda lam: nep.compute_Mder(lam))
    with pytest.raises((ValueError, NotImplementedError, AttributeError, TypeError)):
        na.iar(handle, neigs=2, v=np.ones(n), maxit=10)
    cp = na.ChebPEP(handle, k, -1, 1)
    tol_iar = 1e-10
    lam, V, _ = na.iar(cp, neigs=2, v=np.ones(n), tol=tol_iar, maxit=60, errmeasure=na.ResidualErrmeasure(cp))
    assert len(lam) >= 2 and V.shape == (n, len(lam))
    Mfun = _dep_dense(nep)
    Bnp = ic.ref_cheb_coefficients(Mfun, k, -1.0, 1.0)
    inside = 0
    for l, v in zip(lam, V.T):
        M = Mfun(l)
        gap = np.linalg.norm(M - ic.ref_cheb_eval(Bnp, -1.0, 1.0, l), 2)
        res = np.linalg.norm(M @ v) / np.linalg.norm(v)
        print("lam = %s: residual on the original %.3g, tol + 2 gap = %.3g" % (l, res, tol_iar + 2 * gap))
        assert res <= tol_iar + 2 * gap, (l, res, gap)
        if abs(l.imag) <= 1e-8 and -1 <= l.real <= 1:
            inside += 1
            assert gap <= 1e-12                                                     # k = 20 resolves exp(-lam) on [-1, 1] (coefficients fall below 1e-13)
    assert inside >= 1


# ---- interpolate ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sparse", [False, True])
def test_interpolate_recovers_a_cubic(na, sparse):
    """a cubic PEP, n = 6, from 4 points, against numpy.linalg.solve(V, samples).  The device applies the explicitly formed inverse
    of V: |device - numpy| <= cbound(4, sum_j |W[i, j]| |M(x_j)|) (the kernel) + 4 max |numpy - true| per coefficient."""
    n = 6
    rng = np.random.default_rng(11)
    Av = [rng.standard_normal((n, n)) * (rng.random((n, n)) < (0.4 if sparse else 2.0)) for _ in range(4)]
    pep = na.PEP([sp.csc_matrix(A) for A in Av] if sparse else Av)
    pts = np.array([-1.0, 0.5, 2.0, 3.5])
    got = na.interpolate(pep, pts)
    assert isinstance(got, na.PEP) and len(got.get_Av()) == 4 and got.issparse() == sparse
    assert all(np.iscomplexobj(_dense(B)) for B in got.get_Av())                    # T = complex
    gotr = na.interpolate(pep, pts, T=float)
    assert all(not np.iscomplexobj(_dense(B)) for B in gotr.get_Av())
    Vd = np.vander(pts, 4, increasing=True)
    samples = np.array([sum(x ** i * Av[i] for i in range(4)) for x in pts])        # 4 x n x n
    npc = np.linalg.solve(Vd, samples.reshape(4, -1)).reshape(4, n, n)
    W = sla.lu_solve(sla.lu_factor(Vd), np.eye(4))
    worst = 0.0
    for i in range(4):
        S = sum(abs(W[i, j]) * np.abs(samples[j]) for j in range(4))
        bound = pc.cbound(4, S) + 4 * np.max(np.abs(npc[i] - Av[i]))
        for G in (got, gotr):
            err = np.abs(_dense(G.get_Av()[i]) - npc[i])
            worst = max(worst, float(np.max(err / np.maximum(bound, np.finfo(float).tiny))))
    print("interpolate: largest |device - numpy| / bound = %.3g" % worst)
    assert worst <= 1.0
    with pytest.raises(ValueError):
        na.interpolate(pep, pts + 1j, T=float)


# ---- polyeig on the device ------------------------------------------------------------------------------------------------------
def test_polyeig_chebpep_with_the_arnoldi_eigsolver(na, cp20):
    """polyeig(chebpep, eigsolvertype=ArnoldiEigSolver, nev=4, target=0): every theta is one of the dense route's eigenvalues (first
    order perturbation theory, as tests/test_gpu_lineig.py bounds it) and its pencil residual stays within that file's tolerance"""
    nep, cp, _, _ = cp20
    n, k, a, b = 20, 8, -1.0, 1.0
    lam, V = na.polyeig(cp, eigsolvertype=na.ArnoldiEigSolver, nev=4, target=0)
    assert lam.shape == (4,) and V.shape == (n, 4)
    assert np.allclose(np.linalg.norm(V, axis=0), 1.0, rtol=0, atol=1e-12)
    theta = 2 * (lam - a) / (b - a) - 1
    L0, L1 = na.colleague_pencil(cp.get_Av(), sparse=True)
    L0d, L1d = na.colleague_pencil(cp.get_Av())
    assert np.array_equal(L0.toarray(), L0d) and np.array_equal(L1.toarray(), L1d)
    lam_d, V_d = na.polyeig(cp)
    th_d, Yl, Xr = sla.eig(L0d, L1d, left=True, right=True)
    assert np.allclose(np.sort_complex(lam_d[np.isfinite(lam_d)]), np.sort_complex(((b - a) * (th_d + 1) / 2 + a)[np.isfinite(th_d)]))
    fa, fb = np.linalg.norm(L0d), np.linalg.norm(L1d)
    normC = np.linalg.norm(0.0 * L1d - L0d)                                        # target theta = 0
    rl = np.diff(sp.csr_matrix(L0).indptr) + np.diff(sp.csr_matrix(L1).indptr)
    # the solver itself on the same pencil: the full vectors, for the pencil residual
    solver = na.ArnoldiEigSolver(L0, L1)
    D, X = solver.eig_solve(nev=4, target=0.0)
    for th in theta:
        assert np.min(np.abs(D - th)) <= 1e-8 * max(1.0, abs(th))                 # polyeig returns this solver's values
    used = set()
    for i, d in enumerate(D):
        x = X[:, i]
        res = float(np.linalg.norm(L0 @ x - d * (L1 @ x)))
        rnd = float(np.linalg.norm(np.array([pc.cbound(int(r) + 4, 1.0) for r in rl]) * (abs(L0) @ abs(x) + abs(d) * (abs(L1) @ abs(x)))))
        assert res <= 2 * KS_TOL * normC + rnd, (i, d, res, 2 * KS_TOL * normC, rnd)
        j = [q for q in np.argsort(np.abs(th_d - d)) if q not in used][0]
        used.add(j)
        kappa = np.linalg.norm(Yl[:, j]) * np.linalg.norm(Xr[:, j]) / abs(np.vdot(Yl[:, j], L1d @ Xr[:, j]))
        bound = 2 * kappa * (res + 100 * EPS * (fa + abs(d) * fb))
        assert abs(th_d[j] - d) <= bound, (i, d, th_d[j], bound)
    want = np.sort(np.abs(th_d[np.isfinite(th_d)]))[:4]                            # the 4 nearest theta = 0, none missed
    assert np.allclose(np.sort(np.abs(D)), want, rtol=1e-6)
