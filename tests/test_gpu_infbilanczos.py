"""infbilanczos on the device (src/method_infbilanczos.jl, test/infbilanczos.jl) and K11, its left-right scalar product
(nep_lr_hankel, csrc/lrprod.hip)."""
import functools

import numpy as np
import pytest
import scipy.sparse as sp
import torch

from mp_series import mp_taylor

pytestmark = pytest.mark.gpu

U = 2.0 ** -53


@pytest.fixture(scope="module")
def na():
    import nep_amd
    if nep_amd.device_count() < 1:
        pytest.skip("no GPU")
    return nep_amd


# ---- K11 against the reference loop ----------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _problem(name):
    import nep_amd
    return nep_amd.nep_gallery(name)


@functools.lru_cache(maxsize=None)
def _mp_tau(name, sigma, m):
    """(mt, m) Taylor table from mpmath, rounded to double"""
    return np.array([[complex(x) for x in mp_taylor(f, sigma, m)[0]] for f in _problem(name).get_fv()])


def _host_ref(Av, tau, W, B, ma, mb):
    """the reference's loop (src/method_infbilanczos.jl:235-244) with tau_t[d] = f_t^(d)/d! in place of the scaled derivatives:
    for j, z = sum_t A_t (B[:, :mb] tau_t[j+1 : j+1+mb]) and c -= dot(W[:, j], z) -- all j at once as columns.  Also
    S = sum_t sum_{j,i} |tau_t[i+j+1]| |w_j|^T |A_t| |b_i| and the largest row length of the stacked CSR."""
    c, S = 0j, 0.0
    rowlen = 0
    for t, A in enumerate(Av):
        A = sp.csr_matrix(A)
        H = np.array([tau[t, j + 1:j + 1 + mb] for j in range(ma)])          # ma x mb Hankel
        Z = A @ (B[:, :mb] @ H.T)                                            # column j: sum_i tau[i+j+1] A b_i
        c -= np.sum(np.conj(W[:, :ma]) * Z)
        S += np.sum(np.abs(W[:, :ma]) * (abs(A) @ (np.abs(B[:, :mb]) @ np.abs(H).T)))
        rowlen = rowlen + np.diff(A.indptr)
    return c, S, int(np.max(rowlen))


def _dev_block(X, ld):
    """host n x k -> device (k, ld) tensor (column-major ld x k block, rows >= n padded with NaN: never read)"""
    n, k = X.shape
    T = np.full((k, ld), np.nan + 0j)
    T[:, :n] = X.T
    return torch.from_numpy(T).to("cuda")


CASES = [("qdep0", 0.0), ("qdep0", 0.2), ("qdep0", 0.1 + 0.05j), ("gun_spmf_scaled", 0.0), ("gun_spmf_scaled", 0.3 + 0.1j),
         ("dep0", 0.0)]
SIZES = [(1, 1), (7, 8), (40, 41), (80, 80), (256, 256)]


@pytest.mark.parametrize("ma,mb", SIZES)
@pytest.mark.parametrize("name,sigma", CASES)
def test_k11_against_reference_loop(na, name, sigma, ma, mb):
    from nep_amd.infbilanczos import lr_hankel
    nep = _problem(name)
    n = nep.n
    rng = np.random.default_rng(ma * 1000 + mb)
    W = rng.standard_normal((n, ma)) + 1j * rng.standard_normal((n, ma))
    B = rng.standard_normal((n, mb)) + 1j * rng.standard_normal((n, mb))
    tau = _mp_tau(name, sigma, ma + mb)
    c_host, S, rowlen = _host_ref(nep.get_Av(), tau, W, B, ma, mb)
    ld = n + 3 if (ma, mb) == (7, 8) else n                  # one case with leading dimensions > n
    Wd, Bd = _dev_block(W, ld), _dev_block(B, ld)
    taud = torch.from_numpy(np.ascontiguousarray(tau)).to("cuda")
    c_dev = lr_hankel(nep, Wd, Bd, ma, mb, taud)
    N = n + ma * mb + rowlen
    gam = N * U / (1 - N * U)
    bound = 2 * gam * S
    print("K11 %s sigma=%s (%d,%d): |c_dev - c_host| = %.3e, bound %.3e, |c| = %.3e" % (name, sigma, ma, mb,
                                                                                       abs(c_dev - c_host), bound, abs(c_host)))
    assert abs(c_dev - c_host) <= bound, (abs(c_dev - c_host), bound)
    assert lr_hankel(nep, Wd, Bd, ma, mb, taud) == c_dev            # bitwise repeat


def test_k11_refuses_257_and_scalar_prod_falls_back(na):
    from nep_amd.infbilanczos import lr_hankel
    nep = _problem("qdep0")
    n = nep.n
    rng = np.random.default_rng(5)
    W = rng.standard_normal((n, 257)) + 1j * rng.standard_normal((n, 257))
    B = rng.standard_normal((n, 1)) + 1j * rng.standard_normal((n, 1))
    tau = _mp_tau("qdep0", 0.0, 258)
    taud = torch.from_numpy(np.ascontiguousarray(tau)).to("cuda")
    with pytest.raises(na.NepError) as ei:
        lr_hankel(nep, _dev_block(W, n), _dev_block(B, n), 257, 1, taud)
    assert ei.value.status == -5                                 # NEP_ERR_UNSUPPORTED
    c_host, S, rowlen = _host_ref(nep.get_Av(), tau, W, B, 257, 1)
    c = na.left_right_scalar_prod(nep, W, B, 257, 1, 0.0)
    N = n + 257 + rowlen
    bound = 2 * N * U / (1 - N * U) * S
    assert abs(c - c_host) <= bound, (abs(c - c_host), bound)


# ---- the driver ----------------------------------------------------------------------------------------------------------------
TSTAR = np.array([[-1.665117675679600, 5.780562035399026, 0, 0],
                  [5.780562035399026, 11.562308485001218, -18.839546184493731, 0],
                  [0, 18.839546184493734, -15.213756300995186, 9.788512505128466],
                  [0, 0, 9.788512505128464, -0.120825360586847]])


def _qdep0_pair(na):
    nep = na.nep_gallery("qdep0")
    nept = na.SPMF_NEP([A.T.tocsc() for A in nep.get_Av()], nep.get_fv())
    return nep, nept


def _kat(na, nep, nept, **kw):
    n = nep.n
    args = dict(maxit=40, neigs=3, sigma=0, v=np.ones(n), u=np.ones(n), check_error_every=3, tol=1e-7,
                errmeasure=na.ResidualErrmeasure(nep))
    args.update(kw)
    return na.infbilanczos(nep, nept, **args)


def _host_resid(nep, lam, v):
    return np.linalg.norm(nep.compute_Mder(lam) @ v)


def test_infbilanczos_reference_kat(na):
    """test/infbilanczos.jl:7-29"""
    nep, nept = _qdep0_pair(na)
    lam, V, T = _kat(na, nep, nept)
    d = np.linalg.norm(TSTAR - T[:4, :4], 2)
    res = [_host_resid(nep, l, V[:, i]) for i, l in enumerate(lam)]
    print("KAT: ||Tstar - T[:4,:4]|| = %.3e, size(T) = %d, lambda = %s, residuals = %s" % (d, T.shape[0], lam, res))
    assert d < 1e-10, "||Tstar - T[:4,:4]||_2 = %.3e on the device" % d
    assert len(lam) == 3
    assert all(r < 1e-7 for r in res), res


def test_infbilanczos_neigs_inf(na):
    """test/infbilanczos.jl:32-37"""
    nep, nept = _qdep0_pair(na)
    lam, V, T = _kat(na, nep, nept, maxit=30, neigs=np.inf)
    res = [_host_resid(nep, l, V[:, i]) / np.linalg.norm(V[:, i]) for i, l in enumerate(lam)]
    print("neigs=inf: lambda = %s, residuals = %s" % (lam, res))
    assert len(lam) == 3
    assert all(r < 1e-6 for r in res), res


def test_infbilanczos_no_convergence(na):
    """test/infbilanczos.jl:40-44"""
    nep, nept = _qdep0_pair(na)
    with pytest.raises(na.NoConvergenceException):
        _kat(na, nep, nept, maxit=9, neigs=8)


def test_infbilanczos_dep0_docstring_example(na):
    """src/method_infbilanczos.jl:18-27"""
    nep = na.nep_gallery("dep0")
    nept = na.SPMF_NEP([np.asarray(A).T.copy() for A in nep.get_Av()], nep.get_fv())
    lam, V, T = na.infbilanczos(nep, nept, neigs=3, v=np.ones(nep.n))
    r = _host_resid(nep, lam[0], V[:, 0])
    print("dep0: lambda = %s, ||M(lambda_1) v_1|| = %.3e" % (lam, r))
    assert len(lam) == 3
    assert r <= 1e-12, r


def test_infbilanczos_shares_the_factorisation(na, monkeypatch):
    from test_gpu_twosided import _count_factorisations
    nep, nept = _qdep0_pair(na)
    cnt = _count_factorisations(na, monkeypatch)
    _kat(na, nep, nept)
    assert cnt == {"lu": 1, "transpose": 1}, dict(cnt)
    cnt.reset()
    _kat(na, nep, nept, linsolvertcreator=na.BackslashLinSolverCreator())
    assert cnt["transpose"] == 0, dict(cnt)


def test_infbilanczos_loop_and_k11_agree(na):
    nep, nept = _qdep0_pair(na)
    la, _, _ = _kat(na, nep, nept, scalar_prod="auto")
    ll, _, _ = _kat(na, nep, nept, scalar_prod="loop")
    la, ll = np.sort_complex(la), np.sort_complex(ll)
    print("auto %s loop %s" % (la, ll))
    assert len(la) == len(ll) == 3
    assert np.all(np.abs(la - ll) <= 1e-10 * np.abs(ll)), (la, ll)


def test_infbilanczos_real_shift(na):
    """the KAT configuration (ResidualErrmeasure, v = u = ones, check every 3 steps) at sigma = 0.2 with neigs = 2.  (sigma =
    -0.1 is avoided: there the method returns the same eigenvalue twice, a Lanczos ghost.)"""
    nep, nept = _qdep0_pair(na)
    lam, V, T = _kat(na, nep, nept, neigs=2, sigma=0.2)
    res = [_host_resid(nep, l, V[:, i]) for i, l in enumerate(lam)]
    print("sigma=0.2: lambda = %s, residuals = %s" % (lam, res))
    assert len(lam) == 2
    assert all(r < 1e-7 for r in res), res
