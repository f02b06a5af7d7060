"""The EigSolver layer and mslp on the device: nep_basis_rotate (K13, csrc/lineig.hip) through the raw C ABI on the cases of
tests/lineig_checkers.py, the Arnoldi expansion calls against the pencil in long double, ArnoldiEigSolver against the dense
spectrum with first-order bounds, and mslp as test/mslp.jl and test/deflation.jl run it, against the dense restatement."""
import ctypes as C
import math
from functools import lru_cache

import numpy as np
import pytest
import scipy.sparse as sp
import torch

import nep_amd as nap
import lineig_checkers as lc
import primitive_checkers as pc

pytestmark = pytest.mark.gpu
EPS = np.finfo(float).eps
SQEPS = math.sqrt(EPS)
LD = np.clongdouble
KS_TOL = 1e-10


@pytest.fixture(scope="module")
def na():
    import nep_amd
    if nep_amd.device_count() < 1:
        pytest.skip("no GPU")
    return nep_amd


# ---- nep_basis_rotate through the C ABI -----------------------------------------------------------------------------------------
def _rotate_raw(rows, m, p, carry, V, ldv, lead, Q, ldq, null=()):
    """uploads V, calls the library with the host table, poisons the table, downloads V"""
    from nep_amd import _lib
    from nep_amd.nep import stream_ptr
    Vd = torch.from_numpy(np.ascontiguousarray(V)).to("cuda")
    Qh = np.array(Q, dtype=np.complex128, copy=True)
    addr = dict(V=Vd.data_ptr() + 16 * lead, Q=Qh.ctypes.data)
    ptr = lambda k: None if k in null else C.c_void_p(addr[k])
    rc = _lib.lib.nep_basis_rotate(ptr("V"), ldv, rows, m, p, ptr("Q"), ldq, carry, stream_ptr())
    Qh[:] = pc.NAN                                                        # the table may be freed or overwritten on return
    torch.cuda.synchronize()
    return rc, Vd.cpu().numpy()


def _impl(**a):
    rc, V = _rotate_raw(**a)
    assert rc == 0, rc
    return V


CASES = list(lc.ROTATE.cases())


@pytest.mark.parametrize("case", CASES, ids=[repr(c) for c in CASES])
def test_rotate_case(na, case):
    lc.ROTATE.check(_impl, case)
    print("%r: largest |impl - ref| / bound so far = %.3g" % (case, pc.RATIOS.get(lc.ROTATE.name, 0.0)))


def test_rotate_two_calls_give_the_same_bits(na):
    picked = [c for c in CASES if c.kind == "rounded" and c.group in ("rows257", "rows1025")]
    assert len(picked) >= 20
    for c in picked[:30]:
        a = c.args
        assert _impl(**a).tobytes() == _impl(**a).tobytes(), c


def test_rotate_back_to_back_calls_keep_their_tables(na):
    """twenty calls with different tables without waiting, more than the table slots; every table is poisoned on return"""
    from nep_amd import _lib
    from nep_amd.nep import stream_ptr
    a = lc.Rotate._build(1025, 20, 10, 1, 3, "complex", "exact", 0, pc.SENT)
    rows, m, p, ldv, ldq = a["rows"], a["m"], a["p"], a["ldv"], a["ldq"]
    Vs, want = [], []
    for k in range(20):
        Q = a["Q"] * (k + 1)
        Vd = torch.from_numpy(a["V"].copy()).to("cuda")
        Qh = np.array(Q, copy=True)
        assert _lib.lib.nep_basis_rotate(C.c_void_p(Vd.data_ptr()), ldv, rows, m, p, Qh.ctypes.data_as(C.c_void_p), ldq, 1,
                                         stream_ptr()) == 0
        Qh[:] = pc.NAN
        Vs.append(Vd)
        want.append(lc.ROTATE.ref(**dict(a, Q=Q)))
    torch.cuda.synchronize()
    keep = np.ones(len(a["V"]), dtype=bool)                               # everything but the columns p + 1 .. m - 1
    lc.Rotate._block(keep, 0, rows, m + 2, ldv)[:, p + 1:m] = False
    for k in range(20):
        got = Vs[k].cpu().numpy()
        assert np.array_equal(got[keep], want[k][keep], equal_nan=True), k


def test_rotate_error_codes_launch_nothing(na):
    from nep_amd import _lib
    base = lc.Rotate._build(65, 17, 4, 1, 3, "complex", "exact", lc.LEAD, pc.SENT)
    bad = [({"ldv": 64}, {}), ({"ldq": 16}, {}), ({"rows": 0}, {}), ({"m": 0}, {}), ({"p": 0}, {}), ({"p": 18}, {}),
           ({"m": 3, "p": 4}, {}), ({}, {"null": ("V",)}), ({}, {"null": ("Q",)})]
    for change, how in bad:
        rc, V = _rotate_raw(**dict(base, **change), **how)
        assert rc == _lib.NEP_ERR_ARG, (change, how, rc)
        assert np.array_equal(V, base["V"], equal_nan=True), (change, how)
    big = dict(rows=65, m=129, p=2, carry=1, ldv=68, lead=0, ldq=129, V=np.full(68 * 131, pc.SENT, dtype=np.complex128),
               Q=np.ones(129 * 2, dtype=np.complex128))
    rc, V = _rotate_raw(**big)
    assert rc == _lib.NEP_ERR_UNSUPPORTED and np.array_equal(V, big["V"])
    rc, V = _rotate_raw(**base)                                           # the unchanged call is accepted
    assert rc == 0
    lc.ROTATE.check(lambda **a: V, pc.Case("rows65", "base", "exact", lambda: base))


# ---- the expansion calls --------------------------------------------------------------------------------------------------------
def _expand(nep, lam, maxdim, count, target=0.0):
    """count steps of nep_arnoldi_steps on the pencil (M(lam), M'(lam)) through the raw C ABI.  Returns (rc of the steps call,
    the pinned rows, the basis as a host n x (maxdim + 1) matrix, the solver object that holds the coefficient rows)"""
    from nep_amd import _lib
    from nep_amd.nep import stream_ptr
    lib = _lib.lib
    n = nep.n
    solver = nap.ArnoldiEigSolver.from_nep(nep, lam)
    lu = solver._factor(complex(target), 50)
    v0 = np.random.default_rng(5).standard_normal(n) + 0j
    V = torch.zeros((maxdim + 1, n), dtype=torch.complex128, device="cuda")
    V[0].copy_(torch.from_numpy(v0 / np.linalg.norm(v0)).to("cuda"))
    cBd = torch.from_numpy(solver.cB.copy()).to("cuda")
    work = torch.empty(n, dtype=torch.complex128, device="cuda")
    Sd = torch.zeros((maxdim, maxdim + 4), dtype=torch.complex128, device="cuda")
    Sh = torch.zeros((maxdim, maxdim + 4), dtype=torch.complex128, pin_memory=True)
    h = C.c_void_p()
    _lib.check(lib.nep_arnoldi_create(nep.dev.h, lu.h, n, maxdim, C.c_void_p(V.data_ptr()), n, C.c_void_p(cBd.data_ptr()),
                                      C.c_void_p(work.data_ptr()), C.c_void_p(Sd.data_ptr()), C.c_void_p(Sh.data_ptr()), 0, C.byref(h)))
    try:
        rc = lib.nep_arnoldi_steps(h, 0, count, stream_ptr())
        if rc == 0:
            _lib.check(lib.nep_arnoldi_wait(h, count - 1))
        torch.cuda.synchronize()
        rows = Sh.numpy().copy()
        assert np.array_equal(rows, Sd.cpu().numpy())                     # the device block and its pinned copy agree
        bad = [lib.nep_arnoldi_steps(h, maxdim, 1, stream_ptr()), lib.nep_arnoldi_steps(h, 0, 0, stream_ptr()),
               lib.nep_arnoldi_steps(h, -1, 1, stream_ptr()), lib.nep_arnoldi_wait(h, maxdim)]
        assert all(b == _lib.NEP_ERR_ARG for b in bad), bad
    finally:
        torch.cuda.synchronize()
        lib.nep_arnoldi_destroy(h)
    return rc, rows, V.cpu().numpy().T.copy(), solver


def _dense_pencil(nep, solver, target=0.0):
    """(B, C) = (sum_t cB_t A_t, sum_t (tau cB_t - cA_t) A_t) in long double"""
    Av = [np.asarray(A.toarray() if sp.issparse(A) else A).astype(LD) for A in nep.get_Av()]
    B = sum(LD(c) * A for c, A in zip(solver.cB, Av))
    Cm = sum(LD(target * cb - ca) * A for ca, cb, A in zip(solver.cA, solver.cB, Av))
    return B, Cm


def test_expansion_rows_satisfy_the_krylov_relation(na):
    """dep0_sparse(257) at lam = 0.2, twelve steps: with S the 13 x 12 matrix of the delivered rows, B V_12 = C V_13 S up to the
    rounding of one solve, one product and one orthogonalisation per column.  Bound (entrywise, compared in the Frobenius norm):
    cbound(N, |C| |V_13| |S| + |B| |V_12|) with N = 3 n + 12 + 8 -- the componentwise backward error gamma_{3n} |L| |U| of a
    triangular-factor solve (Higham, Theorem 9.4) taken at |L| |U| ~ |C|, a row of B (at most n terms, within the 3 n), the 13
    terms of the update w - V h and the slack of the other checkers."""
    nep = na.nep_gallery("dep0_sparse", 257)
    n, m = 257, 12
    rc, rows, V, solver = _expand(nep, 0.2, m, m)
    assert rc == 0
    S = np.zeros((m + 1, m), dtype=complex)
    for j in range(m):
        S[:j + 1, j] = rows[j, :j + 1]
        S[j + 1, j] = rows[j, j + 1]
        assert rows[j, j + 1].imag == 0 and rows[j, j + 1].real > 0
        assert rows[j, j + 2].real in (1.0, 2.0) and rows[j, j + 2].imag == 0                   # passes; no vector inside the span
        assert not rows[j, j + 3:].any()
    B, Cm = _dense_pencil(nep, solver)
    Vl = V.astype(LD)
    R = B @ Vl[:, :m] - (Cm @ Vl) @ S.astype(LD)
    E = pc.cbound(3 * n + m + 8, (np.abs(Cm) @ np.abs(Vl) @ np.abs(S).astype(np.longdouble)
                                  + np.abs(B) @ np.abs(Vl[:, :m])).astype(float))
    ratio = float(np.linalg.norm(np.abs(R).astype(float)) / np.linalg.norm(E))
    orth = float(np.linalg.norm(V.conj().T @ V - np.eye(m + 1)))
    print("||B V - C V S||_F / bound = %.3g, ||V^H V - I|| = %.3g" % (ratio, orth))
    pc.RATIOS["nep_arnoldi_steps"] = max(pc.RATIOS.get("nep_arnoldi_steps", 0.0), ratio)
    assert ratio <= 1.0
    assert orth < 1e-10


def test_expansion_reports_the_invariant_subspace_through_the_flag_word(na):
    """beam(5) at lam = -1: the fifth step completes the space; its flag word (2 breakdown + another_pass_wanted, a DGKS step: either
    bit reports a vector inside the span) is set, the words of the steps before it are zero, every call returns OK"""
    nep = na.nep_gallery("beam", 5)
    rc, rows, V, solver = _expand(nep, -1.0, 5, 5)
    assert rc == 0
    flags = [int(rows[j, j + 2].imag) for j in range(5)]
    print("flag words", flags, "beta", [rows[j, j + 1].real for j in range(5)])
    assert all(f == 0 for f in flags[:4]) and flags[4] in (1, 2, 3)
    assert np.linalg.norm(V[:, :5].conj().T @ V[:, :5] - np.eye(5)) < 1e-10
    assert np.all(np.isfinite(rows))


# ---- ArnoldiEigSolver against the dense spectrum --------------------------------------------------------------------------------
@lru_cache(maxsize=None)
def _pencil(size, lam0):
    """(A, B) = (M(lam0), M'(lam0)) of dep0_sparse(size) as complex csc matrices, and the dense spectrum with condition numbers"""
    nep = nap.nep_gallery("dep0_sparse", size)
    ref = lc.ref_dep_of(nep)
    A, B = ref.M(lam0), ref.dM(lam0)
    return sp.csc_matrix(A), sp.csc_matrix(B), lc.pencil_spectrum(A, B)


def _admissible_nev(d, target, start):
    """the first nev >= start at which the dense reference's distances at positions nev and nev + 1 differ by a relative gap
    >= 1e-3 (a conjugate pair is not split)"""
    dist = np.sort(np.abs(d - target))
    nev = start
    while dist[nev] - dist[nev - 1] < 1e-3 * dist[nev]:
        nev += 1
    return nev


ARNOLDI = []
for _size in (100, 257):
    for _lam0 in (0.0, 0.3 + 0.1j):
        for _target in (0.0, 0.5j):
            for _start in (1, 3, 6):
                ARNOLDI.append((_size, _lam0, _target, _admissible_nev(_pencil(_size, _lam0)[2][0], _target, _start)))
ARNOLDI = sorted(set(ARNOLDI), key=ARNOLDI.index)


def _rowlen(A, B):
    return np.diff(sp.csr_matrix(A).indptr) + (np.diff(sp.csr_matrix(B).indptr) if B is not None else 1)


def _check_pairs(D, X, info, A, B, spectrum, target, tol=KS_TOL):
    """the bounds of the stopping rule and of first-order perturbation theory, for unit eigenvectors X[:, i]"""
    n = A.shape[0]
    Bm = sp.identity(n, format="csc", dtype=complex) if B is None else B
    dref, Xr, Yr, kappa = spectrum
    normC = np.linalg.norm((target * Bm - A).toarray())
    fa, fb = np.linalg.norm(A.toarray()), np.linalg.norm(Bm.toarray())
    rl = _rowlen(A, B)
    used, worst = set(), 0.0
    assert np.all(np.diff(np.abs(1.0 / (target - D))) <= 1e-12 * np.abs(1.0 / (target - D[:-1])))     # sorted by decreasing |theta|
    for i, d in enumerate(D):
        x = X[:, i]
        assert abs(np.linalg.norm(x) - 1) < 1e-12
        res = float(np.linalg.norm(A @ x - d * (Bm @ x)))
        rnd = float(np.linalg.norm(np.array([pc.cbound(int(r) + 4, 1.0) for r in rl]) * (abs(A) @ abs(x) + abs(d) * (abs(Bm) @ abs(x)))))
        assert res <= 2 * tol * normC + rnd, (i, d, res, 2 * tol * normC, rnd)
        assert abs(info["residuals"][i] - res) <= 2 * rnd, (i, info["residuals"][i], res, rnd)
        cand = [j for j in np.argsort(np.abs(dref - d)) if j not in used]
        j = cand[0]
        used.add(j)
        bound = 2 * kappa[j] * (res + 100 * EPS * (fa + abs(d) * fb))
        worst = max(worst, abs(dref[j] - d) / bound)
        assert abs(dref[j] - d) <= bound, (i, d, dref[j], abs(dref[j] - d), bound, kappa[j])
    pc.RATIOS["ArnoldiEigSolver"] = max(pc.RATIOS.get("ArnoldiEigSolver", 0.0), worst)
    return worst


@pytest.mark.parametrize("size,lam0,target,nev", ARNOLDI, ids=["n%d_lam%s_t%s_nev%d" % a for a in ARNOLDI])
def test_arnoldi_eigsolver_against_the_dense_spectrum(na, size, lam0, target, nev):
    A, B, spectrum = _pencil(size, lam0)
    solver = na.ArnoldiEigSolver(A, B)
    D, X = na.eig_solve(solver, nev=nev, target=target)
    assert D.shape == (nev,) and X.shape == (size, nev)
    worst = _check_pairs(D, X, solver.info, A, B, spectrum, target)
    print("restarts %d, steps %d, route %r, largest |d - d_ref| / bound = %.3g" % (
        solver.info["restarts"], solver.info["steps"], solver.info["factorization"], worst))
    want = np.sort(np.abs(spectrum[0] - target))[:nev]                    # the nev nearest the target, none missed
    assert np.allclose(np.sort(np.abs(D - target)), want, rtol=1e-6)


def test_arnoldi_eigsolver_standard_problem(na):
    A, _, _ = _pencil(100, 0.0)
    solver = na.ArnoldiEigSolver(A)
    D, X = solver.eig_solve(nev=3, target=0.5j)
    _check_pairs(D, X, solver.info, A, None, lc.pencil_spectrum(A), 0.5j)
    D6, X6 = na.eig_solve(na.DefaultEigSolver(A), nev=2)                  # sparse: dispatched to the Arnoldi solver
    assert D6.shape == (2,) and np.allclose(D6, na.eig_solve(na.ArnoldiEigSolver(A), nev=2)[0])


def test_restart_goes_through_the_rotation_kernel(na):
    A, B, spectrum = _pencil(257, 0.0)
    solver = na.ArnoldiEigSolver(A, B)
    D, Xd = solver.eig_solve_dev(nev=3, target=0.0, _mindim=4, _maxdim=8)
    assert torch.is_tensor(Xd) and Xd.is_cuda and tuple(Xd.shape) == (3, 257)
    info = solver.info
    print(info)
    assert info["restarts"] >= 1 and info["rotations"] == info["restarts"] and info["maxdim"] == 8 and not info["breakdown"]
    _check_pairs(D, Xd.cpu().numpy().T, info, A, B, spectrum, 0.0)


def test_invariant_subspace_returns_all_requested_pairs(na):
    nep = na.nep_gallery("beam", 5)
    ref = lc.ref_dep_of(nep)
    A, B = sp.csc_matrix(ref.M(-1.0)), sp.csc_matrix(ref.dM(-1.0))
    for nev in (1, 3, 5):
        solver = na.ArnoldiEigSolver(A, B)
        D, X = solver.eig_solve(nev=nev, target=0)
        assert solver.info["breakdown"] and solver.info["steps"] == 5 and solver.info["restarts"] == 0
        _check_pairs(D, X, solver.info, A, B, lc.pencil_spectrum(A, B), 0.0)


def test_successive_solvers_on_one_pattern_take_the_device_factorisation(na):
    from nep_amd.linsolvers import _DeviceRefactor
    _DeviceRefactor.clear()
    nep = na.nep_gallery("gun_spmf_scaled", 1310)
    routes = []
    for lam in (0.0, 0.05, 0.1 + 0.02j):
        solver = na.ArnoldiEigSolver(nep.compute_Mder(lam, 0), nep.compute_Mder(lam, 1))
        D, X = solver.eig_solve(nev=1, target=0)
        routes.append(solver.info["factorization"])
        A, B = sp.csc_matrix(solver.A, dtype=complex), sp.csc_matrix(solver.B, dtype=complex)
        r = np.linalg.norm(A @ X[:, 0] - D[0] * (B @ X[:, 0]))
        assert r <= 2 * KS_TOL * np.linalg.norm((0 * B - A).toarray()) + 1e-12 * np.linalg.norm(A.toarray())
        _DeviceRefactor.wait()
    print(routes)
    assert not str(routes[0]).startswith("device") and all(str(r).startswith("device") for r in routes[1:])
    _DeviceRefactor.clear()


# ---- mslp -----------------------------------------------------------------------------------------------------------------------
def _mv(nep, lam, v):
    return np.linalg.norm(np.asarray(nep.compute_Mlincomb(lam, np.asarray(v, dtype=complex).reshape(-1, 1))))


def test_mslp_beam_dense_and_sparse(na):
    """test/mslp.jl:10-22"""
    nep2 = na.nep_gallery("beam", 5)
    nep1 = na.DEP([A.toarray() for A in nep2.A], nep2.tauv)
    h1, h2 = [], []
    l1, v1 = na.mslp(nep1, hist=h1)
    l2, v2 = na.mslp(nep2, hist=h2)
    print(l1, l2, len(h1), len(h2))
    assert _mv(nep1, l1, v1) < 1e-10 and _mv(nep2, l2, v2) < 1e-10
    assert abs(l1 - l2) <= 1e-10 * (1 + abs(l1))
    assert {h["route"] for h in h1} == {"host"} and {h["route"] for h in h2} == {"device"}


def _compare_with_restatement(na, nep, lam0, **kw):
    ref = lc.ref_dep_of(nep)
    hist = []
    lam, v = na.mslp(nep, lam=lam0, hist=hist, **kw)
    lr, vr, itr, histr, ok = lc.ref_mslp(ref, lam=lam0)
    assert ok
    if abs(lam.imag - lr.imag) > abs(lam.imag + lr.imag):
        # a real problem started at a real lam has its pencil's eigenvalues in conjugate pairs of equal modulus: which of the two
        # "the eigenvalue nearest zero" is, is a tie that LAPACK and the Krylov method may break differently; the conjugate
        # iteration is the same iteration (same counts, conjugate vectors)
        assert all(not np.iscomplexobj(A) for A in nep.A) and complex(lam0).imag == 0
        lr, vr = np.conj(lr), np.conj(vr)
    e_dev, e_ref = ref.residual(lam, v), ref.residual(lr, vr)            # ||M(lam) v|| of the two results, unit vectors
    kappa = lc.nep_condition(ref, lr)
    bound = 2 * kappa * (e_dev + e_ref)
    print("lam %r restatement %r, |diff| = %.3g, err_dev %.3g, err_ref %.3g, |diff| / bound = %.3g, iterations %d / %d, kappa %.3g"
          % (lam, lr, abs(lam - lr), e_dev, e_ref, abs(lam - lr) / bound, len(hist), itr, kappa))
    pc.RATIOS["mslp"] = max(pc.RATIOS.get("mslp", 0.0), abs(lam - lr) / bound)
    assert abs(lam - lr) <= bound
    assert abs(len(hist) - itr) <= 1
    assert hist[-1]["err"] < 100 * EPS and abs(np.linalg.norm(v) - 1) < 1e-12
    return hist


def test_mslp_dep0_dense_takes_the_host_route(na):
    hist = _compare_with_restatement(na, na.nep_gallery("dep0"), 0.0)
    assert {h["route"] for h in hist} == {"host"}


@pytest.mark.parametrize("size", [100, 257])
def test_mslp_dep0_sparse_stays_on_the_device(na, size, monkeypatch):
    nep = na.nep_gallery("dep0_sparse", size)
    calls = []
    orig = type(nep).compute_Mder
    # (on the instance: the class keeps the SPMF method, which is what the purity test of the device route looks at)
    monkeypatch.setattr(nep, "compute_Mder", lambda lam, i=0: (calls.append(i), orig(nep, lam, i))[1], raising=False)
    hist = _compare_with_restatement(na, nep, 0.0)
    print([(h["steps"], h["restarts"], h["factorization"]) for h in hist])
    assert {h["route"] for h in hist} == {"device"} and 1 not in calls
    assert all(h["steps"] >= 1 and h["restarts"] >= 0 and "factorization" in h for h in hist)


def test_mslp_on_the_double_eigenvalue(na):
    """test/mslp.jl:26-29"""
    nep = na.nep_gallery("dep_double")
    with pytest.raises(na.NoConvergenceException) as ei:
        na.mslp(nep, lam=9j, maxit=10)
    e = ei.value
    assert np.iscomplexobj(e.lam) and e.v.shape == (3,) and np.isfinite(e.errmeasure) and e.errmeasure >= 100 * EPS
    assert e.msg == "Number of iterations exceeded. maxit=10."
    hist = []
    lam, v = na.mslp(nep, lam=9j, maxit=100, errmeasure=na.ResidualErrmeasure(nep), hist=hist)
    ref = lc.ref_dep_of(nep)
    rnd = ref.n * EPS * sum(a * abs(f(lam)) for a, f in zip(ref.fro, ref.f))       # rounding of a second evaluation of M(lam) v
    print("iterations", len(hist), "err", hist[-1]["err"], "re-evaluated", _mv(nep, lam, v), "rounding", rnd)
    assert hist[-1]["err"] < 100 * EPS and 10 < len(hist) <= 100
    assert _mv(nep, lam, v) < 100 * EPS + 2 * rnd and abs(lam - 3j * np.pi) < 1e-6


def test_mslp_calls_a_user_defined_eigsolver(na):
    seen = []

    class MyEigSolver:                                                    # src/LinSolvers.jl:290-306
        def __init__(self, A, E):
            seen.append((A.shape, E.shape))
            self.A, self.E = A, E

        def eig_solve(self, nev=1, target=0):
            w, X = np.linalg.eig(np.linalg.solve(self.E, self.A))
            i = np.argmin(np.abs(w))
            return w[i], X[:, i]
    nep = na.nep_gallery("dep0", 50)
    hist = []
    lam, v = na.mslp(nep, eigsolvertype=MyEigSolver, tol=1e-5, hist=hist)
    assert len(seen) == len(hist) >= 1 and seen[0] == ((50, 50), (50, 50))
    assert hist[-1]["err"] < 1e-5 and {h["route"] for h in hist} == {"host"}
    assert lc.ref_dep_of(nep).backward_error(lam, v) < 2e-5


@pytest.mark.parametrize("mode", ["Auto", "Generic"])
def test_mslp_with_deflation_finds_distinct_eigenvalues(na, mode):
    """test/deflation.jl:7-40 with mslp itself: dep0 with delays [0, 0.8], two successive deflations, three eigenvalues.  The
    deflated NEP of mode "Generic" is no SPMF and goes through eigsolvertype(M(lam), M'(lam)) on the host; the default mode
    gives an SPMF whose route follows from its matrices (sparse terms: the device route)."""
    A = na.nep_gallery("dep0").A
    nep = na.DEP(A, [0.0, 0.8])
    ref = lc.ref_dep_of(nep)
    lam1, v1 = na.mslp(nep, lam=-0.1 + 0.1j)
    dnep = na.deflate_eigpair(nep, lam1, v1 / np.linalg.norm(v1), mode=mode)
    for k in range(2):
        hist = []
        lam2, v2 = na.mslp(dnep, maxit=1000, lam=-0.1 + 0.1j, hist=hist)
        routes = {h["route"] for h in hist}
        print(mode, type(dnep).__name__, routes, len(hist), "iterations")
        assert routes == ({"host"} if mode == "Generic" else {"device"})
        dnep = na.deflate_eigpair(dnep, lam2, v2 / np.linalg.norm(v2), mode=mode)
    D, V = na.get_deflated_eigpairs(dnep)
    print("eigenvalues", D)
    assert len(D) == 3 and min(abs(D[i] - D[j]) for i in range(3) for j in range(i)) > 1e-4
    for l in D:
        assert np.linalg.svd(ref.M(l), compute_uv=False)[-1] < SQEPS
