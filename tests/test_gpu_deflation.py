"""Deflation on the device: nep_defl_expand (csrc/deflate.hip) through the raw C ABI on the cases of
tests/deflation_checkers.py, parity of the three deflation modes with each other and with the dense restatement of
src/nep_deflation.jl (mirror of test/deflation.jl), and what deflation is for: Newton-type drivers that return NEW eigenpairs."""
import ctypes as C
import math

import numpy as np
import pytest
import scipy.sparse as sp
import torch

import deflation_checkers as dc
import primitive_checkers as pc
from primitive_checkers import C128

pytestmark = pytest.mark.gpu
SQEPS = math.sqrt(np.finfo(float).eps)
MODES = ["Generic", "SPMF", "MM"]


@pytest.fixture(scope="module")
def na():
    import nep_amd
    if nep_amd.device_count() < 1:
        pytest.skip("no GPU")
    return nep_amd


# ---- nep_defl_expand through the C ABI ------------------------------------------------------------------------------------------
def _expand_raw(n0, p, k, s, X, ldx, V, ldv, A, G, W, Vn, ldo, zb, sync=True):
    from nep_amd import _lib
    from nep_amd.nep import stream_ptr
    up = lambda b: torch.from_numpy(np.ascontiguousarray(b)).to("cuda")
    Xd, Vd, Vnd, zbd = up(X), up(V), up(Vn), up(zb)
    rc = _lib.lib.nep_defl_expand(n0, p, k, s, C.c_void_p(Xd.data_ptr()), ldx, C.c_void_p(Vd.data_ptr()), ldv, _lib.hptr(A), _lib.hptr(G),
                                  _lib.hptr(W), C.c_void_p(Vnd.data_ptr() + 16 * dc.LEAD), ldo, C.c_void_p(zbd.data_ptr() + 16),
                                  stream_ptr())
    torch.cuda.synchronize()
    assert np.array_equal(Vd.cpu().numpy(), V, equal_nan=True), "dV was modified"
    return rc, Vnd.cpu().numpy(), zbd.cpu().numpy()


def _impl(**a):
    rc, vn, zb = _expand_raw(**a)
    assert rc == 0, rc
    return vn, zb


CASES = list(dc.DEFL.cases())


@pytest.mark.parametrize("case", CASES, ids=[repr(c) for c in CASES])
def test_defl_expand_case(na, case):
    dc.DEFL.check(_impl, case)
    print("%r: largest |impl - ref| / bound so far = %.3g" % (case, pc.RATIOS.get(dc.DEFL.name, 0.0)))


def test_defl_expand_two_calls_give_the_same_bits(na):
    picked = [c for c in CASES if c.kind == "rounded"][::3] + [c for c in CASES if c.kind == "rounded" and c.args["k"] == 32]
    assert len(picked) >= 4
    for c in picked:
        a = c.args
        v1, z1 = _impl(**a)
        v2, z2 = _impl(**a)
        assert v1.tobytes() == v2.tobytes() and z1.tobytes() == z2.tobytes(), c


def test_defl_expand_error_codes_launch_nothing(na):
    from nep_amd import _lib
    base = dc.DeflExpand._build(65, 3, 2, 1, "exact", 3)
    bad = [({"p": 33}, _lib.NEP_ERR_UNSUPPORTED), ({"p": 0}, _lib.NEP_ERR_UNSUPPORTED), ({"k": 40, "s": 25}, _lib.NEP_ERR_UNSUPPORTED),
           ({"n0": 0}, _lib.NEP_ERR_ARG), ({"k": 0}, _lib.NEP_ERR_ARG), ({"s": -1}, _lib.NEP_ERR_ARG), ({"ldx": 64}, _lib.NEP_ERR_ARG),
           ({"ldo": 64}, _lib.NEP_ERR_ARG), ({"ldv": 67}, _lib.NEP_ERR_ARG)]
    for change, want in bad:
        a = dict(base, **change)
        rc, vn, zb = _expand_raw(**a)
        assert rc == want, (change, rc)
        assert np.array_equal(vn, base["Vn"], equal_nan=True) and np.array_equal(zb, base["zb"], equal_nan=True), change
    rc, vn, zb = _expand_raw(**base)                                    # the unchanged call is accepted
    assert rc == 0 and not np.isnan(zb[1:4]).any()


# ---- shared problems ------------------------------------------------------------------------------------------------------------
def _dense(M):
    return M.toarray() if sp.issparse(M) else np.asarray(M)


def _rel(A, B):
    A, B = _dense(A), _dense(B)
    assert A.shape == B.shape, (A.shape, B.shape)
    return np.linalg.norm(A - B) / np.linalg.norm(B)


def _resid(nep, lam, v):
    """||M(lam) v|| / ||v|| on the ORIGINAL problem"""
    v = np.asarray(v, dtype=complex)
    return np.linalg.norm(nep.compute_Mlincomb(lam, v.reshape(-1, 1))) / np.linalg.norm(v)


def _chain(na, nep, mode, lam0, count=4):
    """`count` deflations, each pair by augnewton from lam0 with v = ones; returns the deflated NEPs and the pairs"""
    d, neps, pairs = nep, [], []
    for i in range(count):
        lam, v = na.augnewton(d, lam=lam0, v=np.ones(nep.size(1) + i), tol=1e-10, maxit=100)
        d = na.deflate_eigpair(d, lam, v, mode=mode)
        neps.append(d); pairs.append((lam, v))
    return neps, pairs


def _assert_new_eigenpairs(na, nep, dnep, count):
    D, V = na.get_deflated_eigpairs(dnep)
    assert len(D) == count
    gaps = [abs(D[i] - D[j]) for i in range(count) for j in range(i)]
    res = [_resid(nep, l, v) for l, v in zip(D, V.T)]
    print("eigenvalues", D, "smallest gap %.3g" % min(gaps), "residuals", res)
    assert min(gaps) > 1e-4
    assert max(res) < SQEPS
    return D


@pytest.fixture(scope="module")
def sparse100(na):
    """dep0_sparse(100), deflated four times in the modes "Generic" and "SPMF" (augnewton from 0.2 + 0.5i)"""
    nep = na.nep_gallery("dep0_sparse", 100)
    out = {"nep": nep}
    for mode in ("Generic", "SPMF"):
        out[mode] = _chain(na, nep, mode, 0.2 + 0.5j)
    return out


@pytest.fixture(scope="module")
def small3(na):
    """test/deflation.jl:45-51: dep0_sparse(3), one pair by augnewton(v = ones, lam = 1.65, tol = 1e-11), deflated in three modes"""
    nep = na.nep_gallery("dep0_sparse", 3)
    ref = dc.ref_dep(nep.A[0].toarray(), nep.A[1].toarray())
    lam, v = na.augnewton(nep, v=np.ones(3), lam=1.65, tol=1e-11)
    rl, rv, steps = dc.ref_augnewton(ref, 1.65, np.ones(3), 1e-11)
    assert abs(lam - rl) < 1e-8, (lam, rl)                             # the restatement: 0.233998529813247 in 7 steps
    return {"nep": nep, "ref": ref, "pair": (lam, v), "d": {m: na.deflate_eigpair(nep, lam, v, mode=m) for m in MODES},
            "r": {m: dc.ref_deflate(ref, lam, v, m) for m in MODES}}


# ---- mode parity: mirror of test/deflation.jl "Deflation modes (new)" -----------------------------------------------------------
XT = np.array([[1, 2], [3, 4], [5, 5.0], [-1, -1]])
ST = np.array([[2, 4], [5, 6.0]])


@pytest.mark.parametrize("mode", MODES)
def test_modes_part_one_against_the_restatement(na, small3, mode):
    d, r, lam = small3["d"][mode], small3["r"][mode], 2 + 2j
    assert d.size() == (4, 4)
    assert _rel(d.compute_Mder(lam), r.Mder(lam)) <= SQEPS
    assert _rel(d.compute_Mder(lam, 1), r.Mder(lam, 1)) <= SQEPS
    assert _rel(d.compute_Mlincomb(lam, XT), r.Mlincomb(lam, XT)) <= SQEPS
    assert _rel(d.compute_MM(ST, XT), r.MM(ST, XT)) <= SQEPS
    a = np.array([0.5 - 1j, 2.0])
    assert _rel(d.compute_Mlincomb(lam, XT, a=a, startder=1), r.Mlincomb(lam, XT, a, 1)) <= SQEPS
    assert sp.issparse(d.compute_Mder(lam)) == (mode != "MM")          # sparse original NEP -> sparse bordered matrix


def test_modes_part_one_agree_with_each_other(na, small3):
    g, s, m = (small3["d"][k] for k in MODES)
    lam = 2 + 2j
    for other in (s, m):
        assert _rel(other.compute_Mder(lam), g.compute_Mder(lam)) <= SQEPS
        assert _rel(other.compute_Mlincomb(lam, XT), g.compute_Mlincomb(lam, XT)) <= SQEPS
        assert _rel(other.compute_MM(ST, XT), g.compute_MM(ST, XT)) <= SQEPS


@pytest.mark.parametrize("mode", MODES)
def test_device_tensor_in_device_tensor_out(na, small3, mode):
    d, lam = small3["d"][mode], 2 + 2j
    Vd = na.to_dev(XT)
    before = Vd.clone()
    z = d.compute_Mlincomb(lam, Vd, a=np.array([1.5, -0.5j]), startder=1)
    assert torch.is_tensor(z) and z.is_cuda and z.shape == (4,)
    assert torch.equal(Vd, before)
    want = d.compute_Mlincomb(lam, XT, a=np.array([1.5, -0.5j]), startder=1)
    assert isinstance(want, np.ndarray) and want.shape == (4,)
    assert _rel(z.cpu().numpy(), want) <= 1e-14
    z1 = d.compute_Mlincomb(lam, Vd[0])                                # a single device vector
    assert _rel(z1.cpu().numpy(), d.compute_Mlincomb(lam, XT[:, :1])) <= 1e-14


def test_modes_part_two_derivatives(na, sparse100):
    """dep0_sparse(100) deflated four times with the same pairs in the three modes: compute_Mder, der = 0..4"""
    nep = sparse100["nep"]
    pairs = sparse100["Generic"][1]
    g = sparse100["Generic"][0][-1]
    s = m = nep
    for lam, v in pairs:
        s = na.deflate_eigpair(s, lam, v, mode="SPMF")
        m = na.deflate_eigpair(m, lam, v, mode="MM")
    assert g.size() == s.size() == m.size() == (104, 104)
    lam = 2 + 2j
    for der in range(5):
        G = g.compute_Mder(lam, der)
        rs, rm = _rel(s.compute_Mder(lam, der), G), _rel(m.compute_Mder(lam, der), G)
        print("der %d: SPMF vs Generic %.3g, MM vs Generic %.3g" % (der, rs, rm))
        assert rs <= SQEPS and rm <= SQEPS


# ---- the capability -------------------------------------------------------------------------------------------------------------
def test_four_new_eigenpairs_generic_and_spmf(na, sparse100):
    nep = sparse100["nep"]
    D = {}
    for mode in ("Generic", "SPMF"):
        D[mode] = _assert_new_eigenpairs(na, nep, sparse100[mode][0][-1], 4)
    for l in D["Generic"]:
        assert min(abs(D["SPMF"] - l)) < 1e-8
    for neps, pairs in (sparse100["Generic"], sparse100["SPMF"]):     # each run started from the same point and found a new pair
        for i, (lam, v) in enumerate(pairs):
            assert len(v) == 100 + i and neps[i].size(1) == 101 + i


def test_four_new_eigenpairs_mm_on_dep0(na):
    nep = na.nep_gallery("dep0")
    Dm = _assert_new_eigenpairs(na, nep, _chain(na, nep, "MM", 0.2 + 0.5j)[0][-1], 4)
    Dg = _assert_new_eigenpairs(na, nep, _chain(na, nep, "Generic", 0.2 + 0.5j)[0][-1], 4)
    for l in Dg:
        assert min(abs(Dm - l)) < 1e-8


def test_mirror_of_the_reference_test_one(na):
    """test/deflation.jl:7-40 with augnewton in place of newton / mslp (not built here): DEP(dep0 matrices, [0, 0.8]), four pairs
    from -0.1 + 0.1i, default mode"""
    A = na.nep_gallery("dep0").A
    nep = na.DEP(A, [0.0, 0.8])
    neps, pairs = _chain(na, nep, "Auto", -0.1 + 0.1j)
    assert isinstance(neps[-1], na.DeflatedSPMF)
    _assert_new_eigenpairs(na, nep, neps[-1], 4)


@pytest.mark.parametrize("mode", ["Generic", "SPMF"])
def test_deflation_prevents_reconvergence(na, sparse100, mode):
    nep = sparse100["nep"]
    kw = dict(lam=0.9 + 0.2j, tol=1e-10, maxit=300)
    l1, v1 = na.resinv(nep, v=np.ones(100), **kw)
    l1b, _ = na.resinv(nep, v=np.ones(100), **kw)
    assert abs(l1 - l1b) < 1e-9                                        # the plain NEP gives the same eigenvalue again
    d = na.deflate_eigpair(nep, l1, v1, mode=mode)
    l2, v2 = na.resinv(d, v=np.ones(101), **kw)
    D, V = na.get_deflated_eigpairs(d, l2, v2)
    print("resinv:", l1, "then", l2)
    assert abs(l2 - l1) > 1e-4
    i2 = int(np.argmin(abs(D - l2)))
    assert abs(D[i2] - l2) < 1e-9 and _resid(nep, D[i2], V[:, i2]) < SQEPS       # (the eigenvector of the ORIGINAL problem)


@pytest.mark.parametrize("mode", ["Generic", "SPMF"])
def test_bordered_matrix_is_well_conditioned_at_a_deflated_eigenvalue(na, sparse100, mode):
    """what the design rests on: at a deflated eigenvalue M(lam_1) is singular to working precision, the bordered matrix is not,
    and the deflated NEP's own linear solver (the bordered matrix factorised as a whole) solves with it"""
    d = sparse100[mode][0][0]
    lam1 = sparse100[mode][1][0][0]
    sigma = lam1 + 1e-9
    rng = np.random.default_rng(11)
    b = rng.standard_normal(101) + 1j * rng.standard_normal(101)
    solver = na.create_linsolver(na.DefaultLinSolverCreator(), d, sigma)
    x = na.lin_solve(solver, b)
    Mt = _dense(d.compute_Mder(sigma))
    r = np.linalg.norm(Mt @ x - b)
    print("cond M = %.3g, cond Mt = %.3g, residual %.3g" % (np.linalg.cond(Mt[:100, :100]), np.linalg.cond(Mt), r))
    assert r <= 1e-10 * np.linalg.norm(Mt, 1) * np.linalg.norm(x)


# ---- sizes the kernel refuses ---------------------------------------------------------------------------------------------------
def test_composed_route_equals_the_kernel(na, sparse100):
    from nep_amd.deflation import expand_tables
    from nep_amd.nep import CDT
    d = sparse100["Generic"][0][-1]                                    # p = 4
    rng = np.random.default_rng(3)
    for k, s in ((1, 0), (3, 2)):
        V = rng.standard_normal((104, k)) + 1j * rng.standard_normal((104, k))
        a, G, W = expand_tables(0.3 + 0.2j, d.S0, rng.standard_normal(k) + 1j * rng.standard_normal(k), s)
        Vd = na.to_dev(V)
        outs = []
        for f in (d._expand_fused, d._expand_composed):
            Vn = torch.full((k + s, 100), float("nan"), dtype=CDT, device="cuda"); zb = torch.full((4,), float("nan"), dtype=CDT, device="cuda")
            assert f(Vd, a, G, W, s, Vn, zb) is not False
            outs.append((Vn.cpu().numpy(), zb.cpu().numpy()))
        # two float64 evaluations of sums of at most k p + p + 1 products of O(1) operands: a few hundred ulp at the very most
        assert _rel(outs[1][0], outs[0][0]) < 1e-13 and np.linalg.norm(outs[1][1] - outs[0][1]) <= 1e-13 * max(1.0, np.linalg.norm(outs[0][1]))


def test_more_than_64_derivatives_take_the_composed_route(na, small3):
    """k + startder = 65 is outside nep_defl_expand's limits: the result is composed on the device and agrees with the restatement.
    Columns scaled by 1 / j! keep the terms G[i, j] W_{i-j} V2[:, i] of comparable size, so that the two float64 evaluations
    (a few thousand terms, no cancellation beyond what random data give) agree far below 1e-9."""
    d, r = small3["d"]["Generic"], small3["r"]["Generic"]
    rng = np.random.default_rng(4)
    V = (rng.standard_normal((4, 65)) + 1j * rng.standard_normal((4, 65))) / np.array([float(math.factorial(j)) for j in range(65)])
    assert _rel(d.compute_Mlincomb(2 + 2j, V), r.Mlincomb(2 + 2j, V)) < 1e-9
    with pytest.raises(np.linalg.LinAlgError):
        d.compute_Mlincomb(d.S0[0, 0], XT)                             # singular lam I - S0 raises, as the reference's factorize
