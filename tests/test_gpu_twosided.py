"""Two-sided methods on the device: transposed solves from the factors of A (nep_lu_transpose / DeviceLU.transpose), the nept
linear solver that shares them, and rfi (src/method_rfi.jl:30-76, test/newton.jl:69-104)."""
import numpy as np
import pytest
import scipy.sparse as sp
import torch

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def na():
    import nep_amd
    if nep_amd.device_count() < 1:
        pytest.skip("no GPU")
    return nep_amd


def _rand_unsym(n, seed):
    rng = np.random.default_rng(seed)
    A = sp.random(n, n, density=0.01, random_state=rng, format="csc")
    B = sp.random(n, n, density=0.01, random_state=rng, format="csc")
    return ((A + 1j * B) + sp.diags(2.0 + rng.standard_normal(n) + 1j * rng.standard_normal(n))).tocsc()


def _matrix(na, name):
    if name == "gun":                       # symmetric strategy
        return sp.csc_matrix(na.nep_gallery("gun_spmf", 2620).compute_Mder(250.0 ** 2 + 30j), dtype=complex)
    if name == "qdep0":                     # not structurally symmetric, zero diagonal entries: unsymmetric strategy
        return sp.csc_matrix(na.nep_gallery("qdep0").compute_Mder(0.0), dtype=complex)
    return _rand_unsym(600, 7)


def _solve(lu, B):
    X = lu.solve(torch.from_numpy(np.ascontiguousarray(B.T)).to("cuda"))
    return X.cpu().numpy().T


def _berr(A, X, B, conj):
    """largest normwise backward error ||op(A) x - b|| / (||A||_1 ||x|| + ||b||) over the columns, op = transpose / adjoint"""
    At = (A.conj().T if conj else A.T).tocsr()
    nA = abs(A).sum(axis=0).max()
    return max(np.linalg.norm(At @ X[:, j] - B[:, j]) / (nA * np.linalg.norm(X[:, j]) + np.linalg.norm(B[:, j]))
               for j in range(B.shape[1]))


def _check(A, X, B, conj, tol=1e-12):
    e = _berr(A, X, B, conj)
    assert e <= tol, e


@pytest.mark.parametrize("name", ["gun", "qdep0", "random"])
@pytest.mark.parametrize("conj", [0, 1])
def test_transposed_solves(na, name, conj):
    A = _matrix(na, name)
    n = A.shape[0]
    rng = np.random.default_rng(3)
    lu = na.DeviceLU(A)
    assert lu.block_schedule
    B32 = rng.standard_normal((n, 32)) + 1j * rng.standard_normal((n, 32))
    before = {k: _solve(lu, B32[:, :k]) for k in (1, 3, 32)}
    t = lu.transpose(conj=bool(conj))
    assert t.block_schedule and t.n == n
    for k in (1, 3, 32):
        _check(A, _solve(t, B32[:, :k]), B32[:, :k], conj)
    # the original handle is left as it was: bitwise the same output
    for k in (1, 3, 32):
        assert np.array_equal(_solve(lu, B32[:, :k]), before[k])
    # forward solves still solve A
    x = _solve(lu, B32[:, :1])
    assert np.linalg.norm(A @ x - B32[:, :1]) <= 1e-10 * np.linalg.norm(B32[:, :1]) * max(1.0, abs(A).sum(axis=0).max())


def test_transpose_either_handle_destroyed_first(na):
    A = _matrix(na, "random")
    n = A.shape[0]
    b = np.random.default_rng(1).standard_normal((n, 1)) + 0j
    lu = na.DeviceLU(A)
    t = lu.transpose()
    del lu
    _check(A, _solve(t, b), b, 0)
    lu2 = na.DeviceLU(A)
    t2 = lu2.transpose(conj=True)
    x = _solve(lu2, b)
    del t2
    assert np.array_equal(_solve(lu2, b), x)


def test_transpose_of_row_scaled_handle(na):
    """factors of diag(rs) A with rs as the handle's row scale solve A; the transposed handle solves A^T (rs as output scale)"""
    A = _matrix(na, "qdep0")
    n = A.shape[0]
    rng = np.random.default_rng(4)
    rs = 0.5 + rng.random(n)
    lu = na.DeviceLU(sp.diags(rs) @ A)
    lu.set_row_scale(rs)
    B = rng.standard_normal((n, 3)) + 1j * rng.standard_normal((n, 3))
    X = _solve(lu, B)
    assert np.linalg.norm(A @ X - B) <= 1e-9 * np.linalg.norm(B) * abs(A).sum(axis=0).max()
    for conj in (0, 1):
        t = lu.transpose(conj=bool(conj))
        _check(A, _solve(t, B), B, conj)
        # solve_add: out = scale * (add + A^-T b)
        Bd = torch.from_numpy(np.ascontiguousarray(B.T)).to("cuda")
        add = torch.from_numpy(np.ascontiguousarray(X.T)).to("cuda")
        out = torch.empty_like(Bd)
        t.solve_add(Bd, add, out, scale=-2.0)
        ref = -2.0 * (X + _solve(t, B))
        assert np.allclose(out.cpu().numpy().T, ref, rtol=0, atol=1e-13 * np.abs(ref).max())


def test_transpose_of_device_factorised_handle(na):
    from nep_amd.linsolvers import _DeviceRefactor
    nep = na.nep_gallery("gun_spmf", 2620)
    A0 = sp.csc_matrix(nep.compute_Mder(250.0 ** 2 + 30j), dtype=complex)
    A1 = sp.csc_matrix(nep.compute_Mder(260.0 ** 2 + 10j), dtype=complex)
    na.DeviceLU(A0)
    _DeviceRefactor.wait()
    lu1 = na.DeviceLU(A1)
    assert lu1.device_factorized
    b = np.random.default_rng(5).standard_normal((A1.shape[0], 3)) + 1j
    x0 = _solve(lu1, b)
    # static pivoting (the stored pivot sequence of another shift) makes the raw solves of these factors less accurate than
    # those of host-pivoted ones, forward and transposed alike: the transposed solves are held to the forward solves' level
    fwd = _berr(A1.T.tocsc(), x0, b, 0)
    for conj in (0, 1):
        _check(A1, _solve(lu1.transpose(conj=bool(conj)), b), b, conj, tol=max(1e-12, 10 * fwd))
    assert np.array_equal(_solve(lu1, b), x0)


def test_level_schedule_refused_and_fallback_solver(na, monkeypatch):
    monkeypatch.setenv("NEP_LU_SCHED", "old")
    nep = na.nep_gallery("qdep0")
    A = sp.csc_matrix(nep.compute_Mder(0.0), dtype=complex)
    lu = na.DeviceLU(A)
    assert not lu.block_schedule
    with pytest.raises(na.NepError) as ei:
        lu.transpose()
    assert ei.value.status == -5                 # NEP_ERR_UNSUPPORTED
    nept = na.SPMF_NEP([M.T.tocsc() for M in nep.get_Av()], nep.get_fv())
    ls, lst, shared = na.twosided_linsolvers(nep, nept, 0.0)
    assert not shared
    b = np.random.default_rng(6).standard_normal(A.shape[0]) + 0j
    y = na.lin_solve(lst, b)
    assert np.linalg.norm(A.T @ y - b) <= 1e-10 * np.linalg.norm(b)


class _Counter(dict):
    """"lu": factorisations (every DeviceLU that is not a transpose: host, device-LU and term-assembled routes alike),
    "transpose": DeviceLU.transpose calls"""

    def __getitem__(self, k):
        if k == "lu":
            return dict.__getitem__(self, "made") - dict.__getitem__(self, "transpose")
        return dict.__getitem__(self, k)

    def reset(self):
        dict.update(self, made=0, transpose=0)

    def __eq__(self, other):
        return all(self[k] == v for k, v in other.items())


def _count_factorisations(na, monkeypatch):
    cnt = _Counter(made=0, transpose=0)
    desc0, tr0 = na.DeviceLU._describe, na.DeviceLU.transpose

    def desc(self, *a, **k):          # every construction route of a DeviceLU ends here
        dict.__setitem__(cnt, "made", dict.__getitem__(cnt, "made") + 1)
        return desc0(self, *a, **k)

    def tr(self, *a, **k):
        dict.__setitem__(cnt, "transpose", dict.__getitem__(cnt, "transpose") + 1)
        return tr0(self, *a, **k)
    monkeypatch.setattr(na.DeviceLU, "_describe", desc)
    monkeypatch.setattr(na.DeviceLU, "transpose", tr)
    return cnt


def test_nept_solver_shares_the_factorisation(na, monkeypatch):
    """FactorizeLinSolver of nept on the transposed handle: one factorisation, nept's own residual in the refinement"""
    nep = na.nep_gallery("qdep0")
    nept = na.SPMF_NEP([M.T.tocsc() for M in nep.get_Av()], nep.get_fv())
    cnt = _count_factorisations(na, monkeypatch)
    ls, lst, shared = na.twosided_linsolvers(nep, nept, 0.3)
    assert shared and cnt == {"lu": 1, "transpose": 1}
    assert lst.nep is nept
    A = sp.csc_matrix(nep.compute_Mder(0.3), dtype=complex)
    b = np.random.default_rng(8).standard_normal((A.shape[0], 1)) + 0j
    _check(A, na.lin_solve(lst, b[:, 0])[:, None], b, 0)
    _check(A.T.tocsc(), na.lin_solve(ls, b[:, 0])[:, None], b, 0)
    # the reference's second creator kind: two factorisations
    cnt.reset()
    _, lst2, shared2 = na.twosided_linsolvers(nep, nept, 0.3, linsolvertcreator=na.BackslashLinSolverCreator())
    assert not shared2 and cnt["transpose"] == 0
    assert np.linalg.norm(A.T @ na.lin_solve(lst2, b) - b) <= 1e-10 * np.linalg.norm(b)


def test_H_relation_shares_only_at_real_shifts(na, monkeypatch):
    from nep_amd import funcs
    rng = np.random.default_rng(9)
    n = 300
    Av = [_rand_unsym(n, 10 + s) for s in range(3)]
    fv = [funcs.one(), funcs.ident(), funcs.Exp(-1.0)]
    nep = na.SPMF_NEP(Av, fv)
    nept = na.SPMF_NEP([A.conj().T.tocsc() for A in Av], fv)
    assert na.transpose_relation(nep, nept) == "H"
    b = rng.standard_normal(n) + 1j * rng.standard_normal(n)
    cnt = _count_factorisations(na, monkeypatch)
    for sigma, want in ((0.4, True), (0.4 + 0.2j, False)):
        cnt.reset()
        _, lst, shared = na.twosided_linsolvers(nep, nept, sigma)
        assert shared == want and cnt["transpose"] == (1 if want else 0) and cnt["lu"] == (1 if want else 2)
        Mt = sp.csc_matrix(nept.compute_Mder(sigma), dtype=complex)
        _check(Mt.T.tocsc(), na.lin_solve(lst, b)[:, None], b[:, None], 0)


def _dense(A):
    return A.toarray() if sp.issparse(A) else np.asarray(A)


def _dep_M(nep, lam):
    return -lam * np.eye(nep.n) + sum(_dense(A) * np.exp(-t * lam) for A, t in zip(nep.A, nep.tauv))


def test_rfi_dep0(na, monkeypatch):
    """test/newton.jl:69-104: both residuals below 100 eps, the derivative formula for the delay within 10 delta, one
    factorisation per iteration (nept recognised)"""
    eps = np.finfo(float).eps
    nep = na.nep_gallery("dep0")
    n = nep.n
    nept = na.DEP([_dense(A).T.copy() for A in nep.A], nep.tauv.copy())
    cnt = _count_factorisations(na, monkeypatch)
    hist = []
    lam, x, y = na.rfi(nep, nept, v=np.ones(n), u=np.ones(n), tol=1e-15, hist=hist)
    iters = len(hist) - 1
    assert iters >= 1 and cnt == {"lu": iters, "transpose": iters}
    M = _dep_M(nep, lam)
    assert np.linalg.norm(M @ x) / np.linalg.norm(x) < 100 * eps
    assert np.linalg.norm(M.T @ y) / np.linalg.norm(y) < 100 * eps
    tau = nep.tauv[1]
    A1 = _dense(nep.A[1])
    Ml = -np.eye(n) - tau * A1 * np.exp(-tau * lam)
    Mtau = -lam * A1 * np.exp(-tau * lam)
    lp = -(y @ Mtau @ x) / (y @ Ml @ x)             # y^T: y is a right eigenvector of M^T
    d = 1e-4
    nepp = na.DEP(list(nep.A), nep.tauv + np.array([0.0, d]))
    neptp = na.DEP(list(nept.A), nept.tauv + np.array([0.0, d]))
    lamd, _, _ = na.rfi(nepp, neptp, v=np.ones(n), u=np.ones(n))
    assert abs(lp - (lamd - lam) / d) < 10 * d
    # the reference's route (two factorisations per iteration, nept not recognised) gives the same eigenvalue
    from nep_amd import twosided
    monkeypatch.setattr(twosided, "transpose_relation", lambda *a, **k: None)
    cnt.reset()
    hist2 = []
    lam2, _, _ = na.rfi(nep, nept, v=np.ones(n), u=np.ones(n), tol=1e-15, hist=hist2)
    assert cnt == {"lu": 2 * (len(hist2) - 1), "transpose": 0}
    assert abs(lam2 - lam) <= 1e-12 * max(1.0, abs(lam))
