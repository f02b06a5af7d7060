"""AAAeigs on the device: nep_cork_expand (csrc/cork.hip) through the raw C ABI on the cases of tests/cork_checkers.py, and the
driver as test/AAAeigs.jl runs it, on dep0_sparse and on the gun twin, against the dense restatement of src/method_AAAeigs.jl."""
import ctypes as C
import math

import numpy as np
import pytest
import scipy.sparse as sp
import torch

import cork_checkers as cc
import primitive_checkers as pc

pytestmark = pytest.mark.gpu
EPS = np.finfo(float).eps
SQEPS = math.sqrt(EPS)
TOL = EPS * 1e6
CIRC = np.exp(1j * np.pi * np.arange(0.0, 2.0 + 1e-9, 0.01))[:-1]       # test/AAAeigs.jl:7


@pytest.fixture(scope="module")
def na():
    import nep_amd
    if nep_amd.device_count() < 1:
        pytest.skip("no GPU")
    return nep_amd


# ---- nep_cork_expand through the C ABI ------------------------------------------------------------------------------------------
def _cork_raw(r, k, c, U, ldu, G, ldg, u, g, alpha, out, ldo, null=(), out_inside=None):
    from nep_amd import _lib
    from nep_amd.nep import stream_ptr
    up = lambda b: torch.from_numpy(np.ascontiguousarray(b)).to("cuda")
    Ud, Gd, outd = up(U), up(G), up(out)
    ud = None if u is None else up(u)
    gd = None if g is None else up(g)
    pout = outd.data_ptr() + 16 * cc.LEAD
    if out_inside == "U":
        pout = Ud.data_ptr() + 16 * (r - 1)
    elif out_inside == "G":
        pout = Gd.data_ptr()
    elif out_inside == "u":
        pout = ud.data_ptr() + 16 * (r - 1)
    elif out_inside == "g":
        pout = gd.data_ptr() + 16 * (c - 1)
    ptr = lambda name, t: None if (name in null or t is None) else C.c_void_p(t.data_ptr())
    rc = _lib.lib.nep_cork_expand(r, k, c, ptr("U", Ud), ldu, ptr("G", Gd), ldg, ptr("u", ud), ptr("g", gd), _lib.cd(alpha),
                                  None if "out" in null else C.c_void_p(pout), ldo, stream_ptr())
    torch.cuda.synchronize()
    assert np.array_equal(Ud.cpu().numpy(), U, equal_nan=True), "dU was modified"
    assert np.array_equal(Gd.cpu().numpy(), G, equal_nan=True), "dG was modified"
    assert ud is None or np.array_equal(ud.cpu().numpy(), u), "du was modified"
    assert gd is None or np.array_equal(gd.cpu().numpy(), g), "dg was modified"
    return rc, outd.cpu().numpy()


def _impl(**a):
    rc, out = _cork_raw(**a)
    assert rc == 0, rc
    return out


CASES = list(cc.CORK.cases())


@pytest.mark.parametrize("case", CASES, ids=[repr(c) for c in CASES])
def test_cork_expand_case(na, case):
    cc.CORK.check(_impl, case)
    print("%r: largest |impl - ref| / bound so far = %.3g" % (case, pc.RATIOS.get(cc.CORK.name, 0.0)))


def test_cork_expand_two_calls_give_the_same_bits(na):
    picked = [c for c in CASES if c.kind == "rounded"][::9]
    assert len(picked) >= 8
    for c in picked:
        a = c.args
        assert _impl(**a).tobytes() == _impl(**a).tobytes(), c


def test_cork_expand_error_codes_launch_nothing(na):
    from nep_amd import _lib
    base = cc.CorkExpand._build(65, 7, 4, "exact", True, 2.0 - 3.0j, 3, 2, 1)
    UNS, ARG = _lib.NEP_ERR_UNSUPPORTED, _lib.NEP_ERR_ARG
    bad = [({"k": 0}, {}, UNS), ({"k": 257}, {}, UNS), ({"c": 0}, {}, UNS), ({"c": 257}, {}, UNS),
           ({"r": 0}, {}, ARG), ({"ldu": 64}, {}, ARG), ({"ldg": 6}, {}, ARG), ({"ldo": 64}, {}, ARG),
           ({}, {"null": ("U",)}, ARG), ({}, {"null": ("G",)}, ARG), ({}, {"null": ("out",)}, ARG), ({}, {"null": ("g",)}, ARG),
           ({}, {"out_inside": "U"}, ARG), ({}, {"out_inside": "G"}, ARG), ({}, {"out_inside": "u"}, ARG),
           ({}, {"out_inside": "g"}, ARG)]
    for change, how, want in bad:
        rc, out = _cork_raw(**dict(base, **change), **how)
        assert rc == want, (change, how, rc)
        assert np.array_equal(out, base["out"], equal_nan=True), (change, how)
    rc, out = _cork_raw(**base)                                         # the unchanged call is accepted
    assert rc == 0 and not np.isnan(out[cc.LEAD: cc.LEAD + 65]).any()
    rc, out = _cork_raw(**dict(base, u=None), null=())                  # dg without du: no rank-1 term, accepted
    assert rc == 0
    cc.CORK.check(lambda **a: out, pc.Case("r65", "g_without_u", "exact", lambda: dict(base, u=None, g=None)))


# ---- the driver -----------------------------------------------------------------------------------------------------------------
def _dense(M):
    return M.toarray() if sp.issparse(M) else np.asarray(M)


def _host_residual(nep, lam, x):
    """ResidualErrmeasure ||M(lam) x|| / ||x|| with M(lam) assembled on the host in float64"""
    return np.linalg.norm(_dense(nep.compute_Mder(lam)) @ x) / np.linalg.norm(x)


def _assert_pairs(nep, lam, X, res, count, tol):
    assert len(lam) == count and X.shape == (nep.size(1), count) and len(res) == count
    hres = [_host_residual(nep, l, x) for l, x in zip(lam, X.T)]
    print("eigenvalues", lam, "\nresiduals on the host", hres, "\nerror measures of the driver", res)
    assert max(hres) < tol
    return hres


def test_dep0_general_nonlinear_problem(na):
    """test/AAAeigs.jl:6-15.  n = 5 <= maxit: the basis saturates at r = 5 and the steps after that add no column to Q."""
    nep = na.nep_gallery("dep0")
    info = {}
    lam, X, res, details = na.AAAeigs(nep, 2 * CIRC, v0=np.ones(5) / math.sqrt(5.0), info=info)
    _assert_pairs(nep, lam, X, res, 6, SQEPS)
    assert info["saturating"] and info["r"] == 5 and (info["d"], info["dt"]) == (0, 0)
    assert details.m_appr == 0 and details.conv_it == 0                  # the empty details


def test_dep0_as_sumnep_weighted_with_details(na):
    """test/AAAeigs.jl:17-22: the same problem as PEP + SPMF (d = 1, dt = 2), weighted AAA, return_details"""
    nep = na.nep_gallery("dep0")
    Av = nep.get_Av()
    nep2 = na.SumNEP(na.PEP([Av[1], -Av[0]]), na.SPMF_NEP([Av[2]], [na.funcs.Exp(-1.0)]))
    info = {}
    lam, X, res, details = na.AAAeigs(nep2, 2 * CIRC, weighted=True, v0=np.ones(5) / math.sqrt(5.0), return_details=True, info=info)
    _assert_pairs(nep, lam, X, res, 6, SQEPS)
    assert (info["d"], info["dt"], info["l"]) == (1, 2, 3) and not info["own_device_terms"]
    z, fz, w = details.zfw
    assert details.m_appr == len(z) == len(w) == fz.shape[0] == info["m"] and fz.shape[1] == 1
    it = details.conv_it
    assert it == info["it"] and details.Lam.shape == (it, it) and details.Res.shape == (it, it)
    last = details.Res[:it, it - 1]
    assert np.all(np.isnan(details.Res[1:, 0])) and np.all(last[:-1] <= last[1:])                    # sorted by residual
    pol, rsd, zer = details.prz
    assert len(pol) >= 1 and rsd.shape == (len(pol), 1) and zer.shape == (len(z) + 1, 1)
    assert len(details.err_appr) >= 1 and details.err_appr[-1] <= EPS * 1e3


def _compare_with_restatement(lam, ref):
    """the returned values are pairwise distinct and each lies within 1e-6 of a Ritz value that the restatement holds converged
    at maxit (a pairing condition: far below the eigenvalue gaps of these problems, far above tol)"""
    conv = np.asarray(ref["converged"])
    for i in range(len(lam)):
        for j in range(i):
            assert abs(lam[i] - lam[j]) > 1e-6, (lam[i], lam[j])
        dist = float(np.min(np.abs(conv - lam[i])))
        print("%r: distance to the restatement's converged values %.3g" % (lam[i], dist))
        assert dist <= 1e-6, (lam[i], conv)


def test_dep0_sparse_four_shifts(na):
    """dep0_sparse (n = 100 > maxit = 60): no saturation, nothing read back between the checks; four cyclic shifts.  The device
    run and the restatement may stop at different checks and return different valid sets, so each returned pair is held to the
    driver's own criterion (residual < tol, evaluated on the host) and paired with the restatement's converged Ritz values."""
    nep = na.nep_gallery("dep0_sparse", 100)
    Z = 0.5 * CIRC
    shifts = 0.25 * np.array([1.0, 1.0j, -1.0, -1.0j])
    info = {}
    lam, X, res, _ = na.AAAeigs(nep, Z, shifts=shifts, neigs=6, maxit=60, v0=np.ones(100), info=info)
    _assert_pairs(nep, lam, X, res, 6, TOL)
    assert not info["saturating"] and info["r"] == info["it"] + 1 and info["nfact"] == 4
    ref = cc.ref_AAAeigs(cc.ref_dep(_dense(nep.A[0]), _dense(nep.A[1])), Z, shifts=shifts, neigs=6, maxit=60, v0=np.ones(100),
                         to_maxit=True)
    print("device: %d steps, m = %d; restatement: m = %d, %d converged at maxit" % (info["it"], info["m"], ref["m"], ref["nconv"]))
    _compare_with_restatement(lam, ref)


def gun_samples():
    """the deterministic boundary part of the sample set of src/method_AAAeigs.jl:157-163 (250 real points and a 250-point
    semicircle) and its five shifts"""
    m, r = 250.0 ** 2, 300.0 ** 2 - 200.0 ** 2
    Z = np.concatenate([np.linspace(m - r + 1e-2, m + r - 1e-2, 250), m - r + 2 * r * (np.exp(1j * np.linspace(0.0, np.pi, 250)) / 2 + 0.5)])
    return Z, r * np.array([2.0 / 3, (1 + 1j) / 3, 0.0, (-1 + 1j) / 3, -2.0 / 3]) + m


def test_gun_twin_five_shifts(na):
    """nlevp_native_gun(1310): PEP + two square-root terms (the general pencil, d = 1, dt = 2), sparse M(sigma), five cached
    factorisations.  Assertions as on dep0_sparse."""
    nep = na.nep_gallery("nlevp_native_gun", 1310)
    Z, shifts = gun_samples()
    info = {}
    lam, X, res, _ = na.AAAeigs(nep, Z, shifts=shifts, neigs=6, maxit=60, v0=np.ones(1310), info=info)
    _assert_pairs(nep, lam, X, res, 6, TOL)
    assert (info["d"], info["dt"], info["l"]) == (1, 2, 4) and info["nfact"] == 5 and not info["own_device_terms"]
    beta = nep.nep2.get_fv()[1].beta
    ref_nep = cc.RefAAANep(nep.nep2.get_Av(), [lambda l: 1j * np.sqrt(l + 0j), lambda l: 1j * np.sqrt(l + beta + 0j)],
                           pep_Av=nep.nep1.get_Av())
    ref = cc.ref_AAAeigs(ref_nep, Z, shifts=shifts, neigs=6, maxit=60, v0=np.ones(1310), to_maxit=True)
    print("device: %d steps, m = %d; restatement: m = %d, %d converged at maxit" % (info["it"], info["m"], ref["m"], ref["nconv"]))
    _compare_with_restatement(lam, ref)


def test_no_convergence_raises_with_the_pairs_found(na):
    nep = na.nep_gallery("dep0_sparse", 100)
    with pytest.raises(na.NoConvergenceException) as ei:
        na.AAAeigs(nep, 0.5 * CIRC, neigs=6, maxit=12, v0=np.ones(100))
    e = ei.value
    assert "maxit=12" in str(e.msg if hasattr(e, "msg") else e) and np.asarray(e.v).shape == (100, 13)
    assert len(np.atleast_1d(e.lam)) == len(np.atleast_1d(e.errmeasure)) <= 6
