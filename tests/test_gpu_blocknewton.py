"""blocknewton on the device: nep_spmf_blockprod (csrc/blockprod.hip) through the raw C ABI on the cases of
tests/blocknewton_checkers.py, and the driver as test/blocknewton.jl runs it, on dep0 and dep0_sparse, against the dense restatement
of the method."""
import ctypes as C
import math
from functools import lru_cache

import numpy as np
import pytest
import scipy.sparse as sp
import torch

import blocknewton_checkers as bc
import primitive_checkers as pc

pytestmark = pytest.mark.gpu
EPS = np.finfo(float).eps
SQEPS = math.sqrt(EPS)


@pytest.fixture(scope="module")
def na():
    import nep_amd
    if nep_amd.device_count() < 1:
        pytest.skip("no GPU")
    return nep_amd


# ---- nep_spmf_blockprod through the C ABI ---------------------------------------------------------------------------------------
def _handle(terms):
    from nep_amd.nep import SPMFDevice
    return SPMFDevice(list(terms))


def _blockprod_raw(n, terms, r, q, Y, ldy, ylead, G, alpha, beta, Z, ldz, zlead, null=(), alias=None, dev=None):
    """uploads the buffers, calls the library, downloads Z.  null: names passed as NULL; alias = offset (in entries) of dZ from the
    first entry of the block Y instead of its own buffer."""
    from nep_amd import _lib
    from nep_amd.nep import stream_ptr
    dev = _handle(terms) if dev is None else dev
    assert dev.valbytes == (16 if np.iscomplexobj(terms[0].data) else 8)
    Yd = torch.from_numpy(np.ascontiguousarray(Y)).to("cuda")
    Zd = torch.from_numpy(np.ascontiguousarray(Z)).to("cuda")
    Gh = np.array(G, dtype=np.complex128, copy=True)
    addr = dict(s=dev.h.value, Y=Yd.data_ptr() + 16 * ylead, G=Gh.ctypes.data, Z=Zd.data_ptr() + 16 * zlead)
    if alias is not None:
        addr["Z"] = addr["Y"] + 16 * alias
    ptr = lambda k: None if k in null else C.c_void_p(addr[k])
    rc = _lib.lib.nep_spmf_blockprod(ptr("s"), r, q, ptr("Y"), ldy, ptr("G"), _lib.cd(alpha), _lib.cd(beta), ptr("Z"), ldz, stream_ptr())
    Gh[:] = pc.NAN                                                        # the table may be freed on return
    torch.cuda.synchronize()
    assert np.array_equal(Yd.cpu().numpy(), Y, equal_nan=True), "dY was modified"
    return rc, Zd.cpu().numpy()


def _impl(**a):
    rc, Z = _blockprod_raw(**a)
    assert rc == 0, rc
    return Z


CASES = list(bc.BLOCKPROD.cases())


@pytest.mark.parametrize("case", CASES, ids=[repr(c) for c in CASES])
def test_blockprod_case(na, case):
    bc.BLOCKPROD.check(_impl, case)
    print("%r: largest |impl - ref| / bound so far = %.3g" % (case, pc.RATIOS.get(bc.BLOCKPROD.name, 0.0)))


def test_blockprod_two_calls_give_the_same_bits(na):
    picked = [c for c in CASES if c.kind == "rounded" and c.group in ("n257", "n1025")]
    assert len(picked) >= 20
    for c in picked[:30]:
        a = c.args
        assert _impl(**a).tobytes() == _impl(**a).tobytes(), c


def test_blockprod_back_to_back_calls_keep_their_tables(na):
    """the driver issues 2p + 2 calls with different tables without waiting: more calls than the handle has table slots"""
    from nep_amd import _lib
    from nep_amd.nep import stream_ptr
    a = bc.BlockProd._build(1025, 3, 3, 2, 1.0, 0.0, "real", 0, "exact", 0, pc.NAN)
    n, r, q = a["n"], a["r"], a["q"]
    dev = _handle(a["terms"])
    Yd = torch.from_numpy(a["Y"]).to("cuda")
    Zs, want = [], []
    for k in range(20):
        G = a["G"] * (k + 1)
        Zd = torch.full((q * n,), pc.NAN, dtype=torch.complex128, device="cuda")
        Gh = np.array(G, copy=True)
        assert _lib.lib.nep_spmf_blockprod(dev.h, r, q, C.c_void_p(Yd.data_ptr()), n, Gh.ctypes.data_as(C.c_void_p), _lib.cd(1.0),
                                           _lib.cd(0.0), C.c_void_p(Zd.data_ptr()), n, stream_ptr()) == 0
        Gh[:] = pc.NAN
        Zs.append(Zd)
        want.append(bc.BLOCKPROD.ref(**dict(a, G=G)))
    torch.cuda.synchronize()
    for k in range(20):
        assert np.array_equal(Zs[k].cpu().numpy(), want[k]), k


def test_blockprod_error_codes_launch_nothing(na):
    from nep_amd import _lib
    base = bc.BlockProd._build(65, 3, 3, 2, -1.0, 1.0, "complex", 3, "exact", bc.LEAD, pc.SENT)
    n, ld = 65, 68
    dev = _handle(base["terms"])
    bad = [({"ldy": 64}, {}), ({"ldz": 64}, {}), ({}, {"null": ("s",)}), ({}, {"null": ("Y",)}), ({}, {"null": ("G",)}),
           ({}, {"null": ("Z",)}), ({}, {"alias": 0}), ({}, {"alias": 5}), ({}, {"alias": 2 * ld + n - 1})]
    for change, how in bad:
        rc, Z = _blockprod_raw(**dict(base, **change), dev=dev, **how)
        assert rc == _lib.NEP_ERR_ARG, (change, how, rc)
        assert np.array_equal(Z, base["Z"], equal_nan=True), (change, how)
    # r, q outside 1 .. 32, and tables beyond 48 KiB (mt r q > 3072): unsupported, nothing launched
    big = bc.BlockProd._build(65, 5, 32, 32, 1.0, 0.0, "real", 0, "exact", 0, pc.NAN)
    rc, Z = _blockprod_raw(**big)
    assert rc == _lib.NEP_ERR_UNSUPPORTED and np.array_equal(Z, big["Z"], equal_nan=True)
    for r, q in ((0, 2), (3, 0), (33, 2), (3, 33)):
        Y = np.full(bc.LEAD + ld * max(r, 1), pc.SENT, dtype=np.complex128)
        Zb = np.full(bc.LEAD + ld * max(q, 1), pc.SENT, dtype=np.complex128)
        G = np.ones(3 * max(r, 1) * max(q, 1), dtype=np.complex128)
        rc, Z = _blockprod_raw(n, base["terms"], r, q, Y, ld, bc.LEAD, G, 1.0, 0.0, Zb, ld, bc.LEAD, dev=dev)
        assert rc == _lib.NEP_ERR_UNSUPPORTED and np.array_equal(Z, Zb), (r, q, rc)
    rc, Z = _blockprod_raw(**base, dev=dev)                               # the unchanged call is accepted
    assert rc == 0 and np.array_equal(Z, bc.BLOCKPROD.ref(**base), equal_nan=True)


def test_blockprod_with_f_of_S_agrees_with_compute_MM(na):
    """G_t = f_t(S): the product is compute_MM(S, X); both results lie within their bounds of the long double reference"""
    from nep_amd import _lib
    from nep_amd.nep import stream_ptr, to_dev, to_host
    bn = __import__("importlib").import_module("nep_amd.blocknewton")
    nep = na.nep_gallery("dep0_sparse", 257)
    rng = np.random.default_rng(7)
    p = 4
    S = 0.3 * (rng.standard_normal((p, p)) + 1j * rng.standard_normal((p, p)))
    X = rng.standard_normal((257, p)) + 1j * rng.standard_normal((257, p))
    G = bn.tables_fS(nep.get_fv(), S)
    Xd = to_dev(X)
    Zd = torch.full((p, 257), pc.NAN, dtype=torch.complex128, device="cuda")
    Gf = np.ascontiguousarray(np.transpose(G, (0, 2, 1)))
    assert _lib.lib.nep_spmf_blockprod(nep.dev.h, p, p, C.c_void_p(Xd.data_ptr()), 257, Gf.ctypes.data_as(C.c_void_p), _lib.cd(1.0),
                                       _lib.cd(0.0), C.c_void_p(Zd.data_ptr()), 257, stream_ptr()) == 0
    Z = to_host(Zd)
    MM = np.asarray(nep.compute_MM(S, X))
    Av = [sp.csr_matrix(A) for A in nep.get_Av()]
    ld = np.clongdouble
    ref = sum(A.toarray().astype(ld) @ (X.astype(ld) @ G[t].astype(ld)) for t, A in enumerate(Av))
    Sabs = sum(abs(A).toarray() @ (np.abs(X) @ np.abs(G[t])) for t, A in enumerate(Av))
    E_row = sum(np.diff(A.indptr) for A in Av)
    bound = np.array([pc.cbound(int(E) + p + 4, 1.0) for E in E_row])[:, None] * Sabs
    e1, e2 = np.abs(Z.astype(ld) - ref).astype(float), np.abs(MM.astype(ld) - ref).astype(float)
    print("blockprod error / bound %.3g, compute_MM error / bound %.3g" % ((e1 / bound).max(), (e2 / bound).max()))
    assert (e1 <= bound).all() and (e2 <= bound).all()
    assert (np.abs(Z - MM) <= 2 * bound).all()


# ---- the driver -----------------------------------------------------------------------------------------------------------------
SPARSE_KW = dict(armijo_factor=0.5, armijo_max=10, maxit=30)
PROBLEMS = [("dep0", 4, 3, dict(armijo_factor=0.5, maxit=20)), ("dep0", 3, 2, {}), ("dep0_sparse", 100, 3, SPARSE_KW),
            ("dep0_sparse", 257, 2, SPARSE_KW), ("dep0_sparse", 257, 4, SPARSE_KW)]


@lru_cache(maxsize=None)
def _restatement(name, size, p, kw):
    import nep_amd
    ref = bc.ref_dep_of(nep_amd.nep_gallery(name, size))
    S, X, it, hist, ok = bc.ref_blocknewton(ref, np.zeros((p, p)), np.eye(ref.n, p), bordered="whole", **dict(kw))
    return ref, it, ok


def _evaluation_rounding(ref, S, X):
    """bound on the rounding error of ||M(S, X)||_2 evaluated in double precision, on the device or on the host: the Frobenius norm
    of the entrywise bound cbound(n + p + 4, sum_t |A_t| |X| |f_t(S)|) of the block product (at most n entries in a row).  The
    driver stops on the device's evaluation being below tol; the host's evaluation of the same pair differs from it by at most
    twice this."""
    Sabs = sum(np.abs(A) @ np.abs(X) @ np.abs(f(S)) for A, f in zip(ref.Av, ref.fm))
    return float(np.linalg.norm(pc.cbound(ref.n + S.shape[0] + 4, Sabs)))


def _start(n, p):
    return np.zeros((p, p)), np.eye(n, p)


@pytest.mark.parametrize("name,size,p,kw", PROBLEMS, ids=["%s%d_p%d" % (a, b, c) for a, b, c, _ in PROBLEMS])
def test_driver_converges_like_the_restatement(na, name, size, p, kw):
    nep = na.nep_gallery(name, size)
    ref, it_whole, ok = _restatement(name, size, p, tuple(sorted(kw.items())))
    assert ok
    info = {}
    S0, X0 = _start(ref.n, p)
    S, X = na.blocknewton(nep, S=S0, X=X0, info=info, **kw)
    res = bc.pair_residual(ref, S, X)
    lam = np.linalg.eigvals(S)
    print("iters", info["iters"], "restatement (whole)", it_whole, "||M(S,X)|| %.3g" % res, "eig(S)", lam, info)
    assert S.shape == (p, p) and X.shape == (ref.n, p) and np.iscomplexobj(S) and np.iscomplexobj(X)
    for l in lam:                                                         # test/blocknewton.jl
        assert bc.sigma_min(ref, l) < SQEPS
    assert res < 100 * EPS + 2 * _evaluation_rounding(ref, S, X)
    V = bc.Vl(X, S)
    assert np.linalg.norm(V.conj().T @ V - np.eye(p)) < 1e-10
    assert info["iters"] <= it_whole + 2
    assert info["blockprod_calls"] > 0 and info["composed_calls"] == 0
    assert len(info["errhist"]) == info["iters"] + 1 and len(info["armijo"]) == info["iters"]
    assert info["factorizations"] >= p * info["iters"] - info["whole_fallbacks"] and info["refine"] == 2


def test_whole_and_composed_give_the_same_eigenvalues(na):
    nep = na.nep_gallery("dep0_sparse", 100)
    S0, X0 = _start(100, 3)
    out = {}
    for key, kw in (("eliminate", {}), ("whole", dict(bordered="whole")), ("composed", dict(_blockprod="composed"))):
        info = {}
        S, X = na.blocknewton(nep, S=S0, X=X0, info=info, **SPARSE_KW, **kw)
        out[key] = (np.sort_complex(np.linalg.eigvals(S)), info)
        print(key, out[key][0], info["iters"], info["blockprod_calls"], info["composed_calls"], info["factorizations"])
    assert out["composed"][1]["blockprod_calls"] == 0 and out["composed"][1]["composed_calls"] > 0
    for key in ("whole", "composed"):
        assert np.max(np.abs(out[key][0] - out["eliminate"][0])) < 1e-10, key


def test_maxit_raises_noconvergence_with_the_pair(na):
    nep = na.nep_gallery("dep0_sparse", 100)
    S0, X0 = _start(100, 3)
    info = {}
    with pytest.raises(na.NoConvergenceException) as ei:
        na.blocknewton(nep, S=S0, X=X0, maxit=3, armijo_factor=0.5, armijo_max=10, info=info)
    e = ei.value
    assert e.lam.shape == (3, 3) and e.v.shape == (100, 3) and np.isfinite(e.errmeasure) and e.errmeasure > 100 * EPS
    assert info["iters"] == 3 and len(info["errhist"]) == 3 and e.errmeasure == info["errhist"][-1]
    assert "maxit=3" in e.msg


def test_dep0_sparse_257_p3_does_not_converge(na):
    nep = na.nep_gallery("dep0_sparse", 257)
    S0, X0 = _start(257, 3)
    info = {}
    with pytest.raises(na.NoConvergenceException):
        na.blocknewton(nep, S=S0, X=X0, info=info, **SPARSE_KW)
    print("last errors", info["errhist"][-3:])
    assert info["iters"] == 30 and info["errhist"][-1] > 1e-4


def test_user_errmeasure_and_errhist_are_consistent(na):
    nep = na.nep_gallery("dep0", 3)
    ref = bc.ref_dep_of(nep)
    seen = []

    def measure(S, X):
        assert isinstance(S, np.ndarray) and isinstance(X, np.ndarray) and X.shape == (3, 2)
        seen.append(bc.pair_residual(ref, S, X))
        return seen[-1]
    info, info0 = {}, {}
    S, X = na.blocknewton(nep, errmeasure=measure, info=info)
    S1, X1 = na.blocknewton(nep, info=info0)
    assert info["errhist"] == seen and len(seen) == info["iters"] + 1
    m = min(len(seen), len(info0["errhist"])) - 1                        # the default measures the same quantity on the device
    assert m >= 3 and np.allclose(seen[:m], info0["errhist"][:m], rtol=1e-6, atol=1e-13)
    assert bc.pair_residual(ref, S, X) < 100 * EPS
