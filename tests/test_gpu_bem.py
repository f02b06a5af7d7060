"""The boundary-element NEP on the device: nep_bem_* (csrc/bem.hip) through the raw C ABI on the cases and within the bounds of
tests/bem_checkers.py, the reference's known-answer test through nep_gallery("bem_fichera"), and the drivers that have to run on a
BEM_NEP (augnewton, quasinewton, resinv, iar, ChebPEP, contour_beyn)."""
import ctypes as ct

import numpy as np
import pytest
import torch

import bem_checkers as bc
import interp_checkers as ic
import primitive_checkers as pc

pytestmark = pytest.mark.gpu
EPS = np.finfo(float).eps
C_vp = ct.c_void_p
NANC = complex(np.nan, np.nan)
LEAD, TRAIL = 5, 7


@pytest.fixture(scope="module")
def na():
    import nep_amd
    if nep_amd.device_count() < 1:
        pytest.skip("no GPU")
    return nep_amd


# ---- the raw ABI ----------------------------------------------------------------------------------------------------------------
_HANDLES = {}


def _handle(name):
    from nep_amd import _lib
    if name not in _HANDLES:
        vert, area = bc.mesh(name)
        n = len(area)
        v9 = np.ascontiguousarray(vert.reshape(n, 9))
        h = C_vp()
        rc = _lib.lib.nep_bem_create(n, v9.ctypes.data_as(C_vp), area.ctypes.data_as(C_vp), 3, ct.byref(h))
        assert rc == 0, rc
        _HANDLES[name] = (h, n)
    return _HANDLES[name]


def _stream():
    from nep_amd.nep import stream_ptr
    return stream_ptr()


def _untouched(buf, written):
    """every word of the NaN-filled buffer outside `written` (flat indices) still is NaN"""
    keep = np.ones(buf.shape[0], dtype=bool)
    keep[written] = False
    rest = buf[keep]
    return bool(np.all(np.isnan(rest.real))) and (not np.iscomplexobj(rest) or bool(np.all(np.isnan(rest.imag))))


def _static(name, ld):
    from nep_amd import _lib
    h, n = _handle(name)
    buf = torch.full((LEAD + ld * n + TRAIL,), np.nan, dtype=torch.float64, device="cuda")
    rc = _lib.lib.nep_bem_static(h, C_vp(buf.data_ptr() + 8 * LEAD), ld, _stream())
    assert rc == 0, rc
    torch.cuda.synchronize()
    b = buf.cpu().numpy()
    idx = (LEAD + np.arange(n)[None, :] * ld + np.arange(n)[:, None])            # [r, c]
    assert _untouched(b, idx.reshape(-1)), "%s: nep_bem_static wrote outside the matrix" % name
    return b[idx]


def _assemble(name, lams, der, ld, pad=3):
    """the list of matrices, after the checks every call gets: padding untouched, bitwise symmetric"""
    from nep_amd import _lib
    h, n = _handle(name)
    la = np.ascontiguousarray(lams, dtype=np.complex128)
    stride = ld * n + pad
    buf = torch.full((LEAD + stride * len(la) + TRAIL,), NANC, dtype=torch.complex128, device="cuda")
    rc = _lib.lib.nep_bem_assemble(h, len(la), la.ctypes.data_as(C_vp), der, C_vp(buf.data_ptr() + 16 * LEAD), ld, stride, _stream())
    assert rc == 0, rc
    torch.cuda.synchronize()
    b = buf.cpu().numpy()
    idx = LEAD + np.arange(len(la))[:, None, None] * stride + np.arange(n)[None, None, :] * ld + np.arange(n)[None, :, None]   # [l, r, c]
    assert _untouched(b, idx.reshape(-1)), "%s: nep_bem_assemble wrote outside the matrices" % name
    out = b[idx]
    for M in out:
        assert M.tobytes() == np.ascontiguousarray(M.T).tobytes(), "%s: the assembled matrix is not bitwise symmetric" % name
    return out


def _colbuf(M, ld):
    """column-major device image of the host block M (n x k) with NaN padding rows and guard words, and the flat indices of M"""
    n, k = M.shape
    buf = np.full(LEAD + ld * k + TRAIL, NANC, dtype=np.complex128)
    idx = LEAD + np.arange(k)[None, :] * ld + np.arange(n)[:, None]
    buf[idx] = M
    return torch.from_numpy(buf).to("cuda"), idx


def _mlincomb(name, lam, a, sd, V, ldv):
    from nep_amd import _lib
    h, n = _handle(name)
    Vd, _ = _colbuf(V, ldv)
    zd, zi = _colbuf(np.full((n, 1), NANC), n)
    av = np.ascontiguousarray(a, dtype=np.complex128)
    rc = _lib.lib.nep_bem_mlincomb(h, _lib.cd(lam), len(av), av.ctypes.data_as(C_vp), sd, C_vp(Vd.data_ptr() + 16 * LEAD), ldv,
                                   C_vp(zd.data_ptr() + 16 * LEAD), _stream())
    assert rc == 0, rc
    torch.cuda.synchronize()
    z = zd.cpu().numpy()
    assert _untouched(z, zi.reshape(-1)), "%s: nep_bem_mlincomb wrote outside z" % name
    return z[zi[:, 0]]


def _resid(name, lams, Q, ldq, ldo):
    from nep_amd import _lib
    h, n = _handle(name)
    k = len(lams)
    la = np.ascontiguousarray(lams, dtype=np.complex128)
    Qd, _ = _colbuf(Q, ldq)
    Od, oi = _colbuf(np.full((n, k), NANC), ldo)
    rc = _lib.lib.nep_bem_resid(h, k, la.ctypes.data_as(C_vp), C_vp(Qd.data_ptr() + 16 * LEAD), ldq, C_vp(Od.data_ptr() + 16 * LEAD), ldo,
                                _stream())
    assert rc == 0, rc
    torch.cuda.synchronize()
    o = Od.cpu().numpy()
    keep = np.ones(o.shape[0], dtype=bool); keep[oi.reshape(-1)] = False
    assert np.all(np.isnan(o[keep].real)), "%s: nep_bem_resid wrote outside the block" % name
    return o[oi]


@pytest.mark.parametrize("name", bc.MESHES)
def test_static_part(na, name):
    n = _handle(name)[1]
    S = _static(name, n)
    r = bc.check_static(name, S)
    assert S.tobytes() == np.ascontiguousarray(S.T).tobytes()                   # stored mirrored
    S3 = _static(name, n + 3)
    assert S3.tobytes() == S.tobytes()                                            # two calls, two leading dimensions: the same bits
    print("%s: S0 at %.3g of the bound" % (name, r))


@pytest.mark.parametrize("der", bc.DERS)
@pytest.mark.parametrize("name", bc.MESHES)
def test_assemble_cases(na, name, der):
    """every shift alone (batch 1), the batch of 3 and the batch of 20, leading dimensions n and n + 3; every matrix within the
    bound, symmetric bit for bit, padding untouched; a matrix has the same bits wherever in whichever batch it was computed"""
    n = _handle(name)[1]
    worst = 0.0
    single = {}
    for i, lam in enumerate(bc.LAMS):
        M = _assemble(name, [lam], der, n + 3 * (i % 2))[0]
        worst = max(worst, bc.check_mder(name, lam, der, M))
        single[lam] = M
    for nlam, ld in [(nl, n + 3 * (i % 2)) for i, nl in enumerate(bc.BATCHES[1:])] + [(bc.BATCHES[-1], n)]:
        lams = bc.batch_lams(nlam)
        out = _assemble(name, lams, der, ld)
        again = _assemble(name, lams, der, ld)
        assert out.tobytes() == again.tobytes(), "two calls differ"
        for lam, M in zip(lams, out):
            assert M.tobytes() == single[lam].tobytes(), (name, der, nlam, lam)
    print("%s der %d: assemble at %.3g of the bound" % (name, der, worst))


@pytest.mark.parametrize("ksd", bc.MLINCOMB)
@pytest.mark.parametrize("name", bc.MESHES)
def test_mlincomb_cases(na, name, ksd):
    """within the bound; columns with a_j = 0 hold NaN and are never read; two calls give the same bits; the result agrees with
    assemble followed by a long-double product within the sum of the two bounds: the matrix-free bound, and the bounds of the
    assembled matrices carried through |a_j| |v_j|"""
    k, sd = ksd
    n = _handle(name)[1]
    lam, a, V = bc.operands(name, k, sd)
    z = _mlincomb(name, lam, a, sd, V, n)
    r = bc.check_mlincomb(name, lam, a, sd, V, z)
    z3 = _mlincomb(name, lam, a, sd, V, n + 3)
    assert z3.tobytes() == z.tobytes()
    zref, bound, entry = bc.reference(name).mlincomb(lam, a, sd, V)
    zasm = np.zeros(n, dtype=bc.CLD)
    for j in range(k):
        if a[j] != 0:
            zasm += bc.CLD(a[j]) * (_assemble(name, [lam], j + sd, n)[0].astype(bc.CLD) @ V[:, j].astype(bc.CLD))
    gap = np.abs(z.astype(bc.CLD) - zasm).astype(np.float64)
    assert np.all(gap <= bound + entry), float(np.max(gap / (bound + entry)))
    print("%s k %d startder %d: mlincomb at %.3g of the bound, %.3g of the sum of both bounds from the assembled product"
          % (name, k, sd, r, float(np.max(gap / (bound + entry)))))


@pytest.mark.parametrize("name", bc.MESHES)
def test_resid_cases(na, name):
    """out[:, s] = M(lam_s) q_s for batches of 1, 3 and 20 shifts, leading dimensions n and n + 3"""
    n = _handle(name)[1]
    rng = np.random.default_rng(n)
    worst = 0.0
    for k, ldq, ldo in zip(bc.BATCHES, (n, n + 3, n), (n, n, n + 3)):
        lams = bc.batch_lams(k)
        Q = rng.standard_normal((n, k)) + 1j * rng.standard_normal((n, k))
        out = _resid(name, lams, Q, ldq, ldo)
        assert _resid(name, lams, Q, ldq, ldo).tobytes() == out.tobytes()
        for s, lam in enumerate(lams):
            worst = max(worst, bc.check_mlincomb(name, lam, np.ones(1), 0, Q[:, s:s + 1], out[:, s], kind="resid"))
            _, bound, entry = bc.reference(name).mlincomb(lam, np.ones(1), 0, Q[:, s:s + 1])
            zasm = _assemble(name, [lam], 0, n)[0].astype(bc.CLD) @ Q[:, s].astype(bc.CLD)
            assert np.all(np.abs(out[:, s].astype(bc.CLD) - zasm).astype(np.float64) <= bound + entry)
    print("%s: resid at %.3g of the bound" % (name, worst))


def test_more_shifts_than_one_launch_takes(na):
    """33 shifts: assemble and resid hand at most 32 to a launch, so the 33rd takes a second one, at its own offset"""
    name, nlam = "first65", 33
    n = _handle(name)[1]
    lams = bc.batch_lams(nlam)
    out = _assemble(name, lams, 0, n + 3)
    for lam, M in zip(lams, out):
        assert M.tobytes() == _assemble(name, [lam], 0, n)[0].tobytes()
        bc.check_mder(name, lam, 0, M)
    rng = np.random.default_rng(33)
    Q = rng.standard_normal((n, nlam)) + 1j * rng.standard_normal((n, nlam))
    res = _resid(name, lams, Q, n + 3, n)
    for s, lam in enumerate(lams):
        bc.check_mlincomb(name, lam, np.ones(1), 0, Q[:, s:s + 1], res[:, s], kind="resid")
        assert res[:, s].tobytes() == _resid(name, [lam], Q[:, s:s + 1], n, n)[:, 0].tobytes()


def test_coinciding_gauss_points_off_the_diagonal(na):
    """a mesh that holds one triangle twice has pairs with d = 0 off the diagonal; the matrix-free product treats them as
    assemble does.  Tolerance 1e-12 max|M| |v|: the two evaluations differ by roundings of a few u per term (n = 3), a dropped
    d = 0 term by W / (4 pi) against entries of the same order"""
    from nep_amd import _lib
    vert, area = bc.mesh("first2")
    v9 = np.ascontiguousarray(np.concatenate([vert, vert[:1]]).reshape(3, 9)); ar = np.ascontiguousarray(np.concatenate([area, area[:1]]))
    h = C_vp()
    assert _lib.lib.nep_bem_create(3, v9.ctypes.data_as(C_vp), ar.ctypes.data_as(C_vp), 3, ct.byref(h)) == 0
    _HANDLES["twice"] = (h, 3)
    try:
        rng = np.random.default_rng(3)
        V = rng.standard_normal((3, 2)) + 1j * rng.standard_normal((3, 2))
        lam = 5 + 0.3j
        M0, M1, M2 = (_assemble("twice", [lam], der, 3)[0] for der in (0, 1, 2))
        assert M0[0, 2] == M0[0, 0] and M1[0, 2] == M1[0, 0]
        for a, sd, want in (([1.0], 0, M0 @ V[:, 0]), ([1.0], 1, M1 @ V[:, 0]), ([2.0, -1j], 0, 2 * M0 @ V[:, 0] - 1j * M1 @ V[:, 1]),
                            ([2.0, -1j], 1, 2 * M1 @ V[:, 0] - 1j * M2 @ V[:, 1])):
            z = _mlincomb("twice", lam, np.array(a, dtype=complex), sd, V[:, :len(a)], 3)
            assert np.max(np.abs(z - want)) <= 1e-12 * max(np.abs(M0).max(), np.abs(M1).max()) * 3 * np.abs(V).max()
    finally:
        del _HANDLES["twice"]
        _lib.lib.nep_bem_destroy(h)


def test_mlincomb_in_passes(na):
    """k = 130 columns: three passes of the kernel (64 coefficients each), against the reference"""
    name, k, sd = "first65", 130, 0
    n = _handle(name)[1]
    rng = np.random.default_rng(5)
    V = rng.standard_normal((n, k)) + 1j * rng.standard_normal((n, k))
    a = (rng.standard_normal(k) + 1j * rng.standard_normal(k)) * 0.5 ** np.arange(k)
    z = _mlincomb(name, 1.0, a, sd, V, n)
    r = bc.check_mlincomb(name, 1.0, a, sd, V, z)
    print("k = 130: at %.3g of the bound" % r)


def test_error_codes(na):
    from nep_amd import _lib
    lib = _lib.lib
    vert, area = bc.mesh("first2")
    v9 = np.ascontiguousarray(vert.reshape(2, 9))
    for order in (1, 2, 4, 7):
        h = C_vp()
        rc = lib.nep_bem_create(2, v9.ctypes.data_as(C_vp), area.ctypes.data_as(C_vp), order, ct.byref(h))
        assert rc == _lib.NEP_ERR_UNSUPPORTED and not h.value, (order, rc)
    h = C_vp()
    assert lib.nep_bem_create(0, v9.ctypes.data_as(C_vp), area.ctypes.data_as(C_vp), 3, ct.byref(h)) == _lib.NEP_ERR_ARG
    assert lib.nep_bem_create(2, None, area.ctypes.data_as(C_vp), 3, ct.byref(h)) == _lib.NEP_ERR_ARG
    buf = torch.full((64,), NANC, dtype=torch.complex128, device="cuda")
    lam = np.array([1.0 + 0j]); one = np.ones(1, dtype=np.complex128)
    p, st = C_vp(buf.data_ptr()), _stream()
    ARG = _lib.NEP_ERR_ARG
    assert lib.nep_bem_static(None, p, 2, st) == ARG
    assert lib.nep_bem_assemble(None, 1, lam.ctypes.data_as(C_vp), 0, p, 2, 4, st) == ARG
    assert lib.nep_bem_mlincomb(None, _lib.cd(1.0), 1, one.ctypes.data_as(C_vp), 0, p, 2, p, st) == ARG
    assert lib.nep_bem_resid(None, 1, lam.ctypes.data_as(C_vp), p, 2, p, 2, st) == ARG
    info = (ct.c_int64 * 4)()
    assert lib.nep_bem_info(None, info) == ARG
    hh, n = _handle("first2")
    assert lib.nep_bem_info(hh, info) == 0 and (info[0], info[1]) == (2, 3) and info[3] >= 64
    assert lib.nep_bem_assemble(hh, 1, lam.ctypes.data_as(C_vp), 0, p, 1, 4, st) == ARG          # ldo < n
    assert lib.nep_bem_assemble(hh, 1, lam.ctypes.data_as(C_vp), -1, p, 2, 4, st) == ARG
    assert lib.nep_bem_mlincomb(hh, _lib.cd(1.0), 0, one.ctypes.data_as(C_vp), 0, p, 2, p, st) == ARG
    assert lib.nep_bem_mlincomb(hh, _lib.cd(1.0), 1, one.ctypes.data_as(C_vp), -1, p, 2, p, st) == ARG
    assert lib.nep_bem_resid(hh, 1, lam.ctypes.data_as(C_vp), p, 1, p, 2, st) == ARG
    assert lib.nep_bem_assemble(hh, 0, None, 0, None, 2, 4, st) == 0                              # an empty batch is a no-op
    torch.cuda.synchronize()
    assert np.all(np.isnan(buf.cpu().numpy().real))                                               # nothing was launched
    assert lib.nep_bem_destroy(None) == 0


# ---- the gallery problem and the drivers ----------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def nep(na):
    return na.nep_gallery("bem_fichera", 1)


def test_gallery_reference_kat(na, nep):
    """test/gallery.jl:178-183: n = 96 and M(lam_ref) is rank deficient by Julia's rank tolerance"""
    assert isinstance(nep, na.BEM_NEP) and nep.size() == (96, 96) and nep.size(1) == 96 and not nep.issparse()
    assert na.nep_gallery("bem_fichera").size(1) == 24 * 16 and na.nep_gallery("bem_fichera", N=2).size(1) == 96
    M = nep.compute_Mder(bc.LAM_REF)
    assert isinstance(M, np.ndarray) and M.dtype == np.complex128 and M.shape == (96, 96)
    s = np.linalg.svd(M, compute_uv=False)
    print("sigma_min / sigma_max = %.3g" % (s[-1] / s[0]))
    assert s[-1] <= 96 * EPS * s[0]
    bc.check_mder("full96", bc.LAM_REF, 0, M)
    bc.check_static("full96", nep.static_part())
    B = nep.compute_Mder_batch([1.0, bc.LAM_REF])
    assert B.shape == (2, 96, 96) and np.array_equal(B[1], M)
    with pytest.raises(na.NepError):
        na.BEM_NEP(na.gen_ficheramesh(1), gauss_order=4)
    with pytest.raises(NotImplementedError, match="terms outside its SPMF matrices"):
        na.ilan(nep, v=np.ones(96))


def test_compute_mlincomb_host_and_device(na, nep):
    lam, a, V = bc.operands("full96", 5, 1)
    z = nep.compute_Mlincomb(lam, np.nan_to_num(V), a, startder=1)
    bc.check_mlincomb("full96", lam, a, 1, V, z)
    zd = nep.compute_Mlincomb(lam, na.to_dev(np.nan_to_num(V)), a, startder=1)
    assert torch.is_tensor(zd) and np.array_equal(zd.cpu().numpy(), z)
    v = V[:, 0]
    bc.check_mlincomb("full96", lam, np.ones(1), 0, V[:, :1], nep.compute_Mlincomb(lam, v))
    rn, qn, _ = nep.resid_norms([lam, 1.0], torch.from_numpy(np.ascontiguousarray(V[:, [0, 2]])).to("cuda"))
    for s, (l, j) in enumerate(((lam, 0), (1.0, 2))):
        want = np.linalg.norm(np.asarray(bc.reference("full96").mder(l, 0)[0] @ V[:, j].astype(bc.CLD), dtype=np.complex128))
        assert abs(rn[s] - want) <= 1e-12 * want and abs(qn[s] - np.linalg.norm(V[:, j])) <= 1e-13 * qn[s]


def _close(lam, ref):
    return abs(lam - ref) <= 1e-10 * abs(ref)


def test_augnewton_reaches_the_reference_eigenvalue(na, nep):
    """from 8.8 to lam_ref within 1e-10 |lam_ref| (the CPU restatement lands 2e-17 away in 5 steps; the nearest other eigenvalues
    near the real axis are ~7.95 and ~9.4)"""
    lam, v = na.augnewton(nep, lam=8.8, v=np.ones(96))
    print("augnewton from 8.8: %r, |lam - lam_ref| = %.3g" % (lam, abs(lam - bc.LAM_REF)))
    assert _close(lam, bc.LAM_REF)


def test_augnewton_from_seven(na, nep):
    lam, v = na.augnewton(nep, lam=7.0, v=np.ones(96))
    print("augnewton from 7: %r, |lam - lam_ref2| = %.3g" % (lam, abs(lam - bc.LAM_REF2)))
    assert _close(lam, bc.LAM_REF2)


@pytest.mark.parametrize("method", ["quasinewton", "resinv"])
def test_quasinewton_and_resinv(na, nep, method):
    """from 8.8 to lam_ref, with the residual the driver's own (default) tolerance, 100 eps, demands.  To first order
    |lam - lam_ref| <= kappa ||M(lam) v|| / ||v|| with kappa = 1 / |w^H M'(lam_ref) v| = 360 for unit null vectors (NumPy, below): a
    residual of 100 eps puts lam within 1e-11, far inside the 1e-10 |lam_ref| of the augnewton tests"""
    tol = EPS * 100
    lam, v = getattr(na, method)(nep, lam=8.8, v=np.ones(96))
    res = np.linalg.norm(nep.compute_Mlincomb(lam, v)) / np.linalg.norm(v)
    M = bc.mfun("full96")
    U_, s_, Vh_ = np.linalg.svd(M(bc.LAM_REF))
    kappa = 1.0 / abs(U_[:, -1].conj() @ M(bc.LAM_REF, 1) @ Vh_[-1].conj())
    print("%s: %r, residual %.3g, kappa %.3g, |lam - lam_ref| = %.3g" % (method, lam, res, kappa, abs(lam - bc.LAM_REF)))
    assert res < tol
    assert 2 * kappa * tol < 1e-10 * abs(bc.LAM_REF)
    assert _close(lam, bc.LAM_REF)


def test_reference_iar_benchmark(na, nep):
    """test/gallery.jl:184-187 as written: iar(nep, sigma=9, v=ones, neigs=1, maxit=50, tol=1e-6), then ||M(lam) v|| < sqrt(eps) 100"""
    lam, V, _ = na.iar(nep, sigma=9.0, v=np.ones(96), neigs=1, maxit=50, tol=1e-6)
    assert na.iar.last_route in ("async", "sync")
    res = np.linalg.norm(nep.compute_Mlincomb(lam[0], V[:, 0]))
    print("iar: lam = %r, ||M(lam) v|| = %.3g" % (lam[0], res))
    assert res < np.sqrt(EPS) * 100


def test_tiar_runs_on_it(na, nep):
    lam, V, *_ = na.tiar(nep, sigma=9.0, v=np.ones(96), neigs=1, maxit=50, tol=1e-6)
    res = np.linalg.norm(nep.compute_Mlincomb(lam[0], V[:, 0]))
    assert res < np.sqrt(EPS) * 100


def test_chebpep_of_the_bem_problem(na, nep):
    """ChebPEP(nep, 20, 0, 10): the device-sample route.  Its coefficients against the NumPy formula on the same samples, with the
    bound test_gpu_chebpep.py uses for a dense sampled source (two sums of k products, cbound(k, S) each, and the difference of
    the two weight tables); the same against a ChebPEP of a wrapping Mder_NEP (the host-sample route); the nodes are reproduced
    within 100 eps (test/chebpep.jl); iar on it near 8.8 returns the eigenvalue of the NumPy interpolant, which is lam_ref to the
    interpolation error."""
    n, k, a, b = 96, 20, 0.0, 10.0
    calls = {"dev": [], "host": 0}
    dev0, host0 = nep.compute_Mder_dev, nep.compute_Mder
    nep.compute_Mder_dev = lambda lams, der=0: (calls["dev"].append(len(lams)), dev0(lams, der))[1]
    nep.compute_Mder = lambda lam, i=0: (calls.__setitem__("host", calls["host"] + 1), host0(lam, i))[1]
    try:
        cp = na.ChebPEP(nep, k, a, b)
    finally:
        del nep.compute_Mder_dev, nep.compute_Mder
    assert calls == {"dev": [k], "host": 0}, calls                                  # one batched assembly, no sample through the host
    x = na.chebyshev_nodes(a, b, k)
    samples = [nep.compute_Mder(xj) for xj in x]
    ref = ic.ref_cheb_coefficients(lambda lam: samples[int(np.argmin(np.abs(x - lam)))], k, a, b)
    W, Wref = na.chebyshev_weights(a, b, k), np.array([ic.ref_cheb_T(a, b, x, i) * 2 / k for i in range(k)])
    Wref[0] *= 0.5
    wrapped = na.ChebPEP(na.Mder_NEP(n, lambda lam: nep.compute_Mder(lam)), k, a, b)
    absS = [np.abs(S) for S in samples]
    worst = worst2 = 0.0
    for i, (B, B2) in enumerate(zip(cp.get_Av(), wrapped.get_Av())):
        assert isinstance(B, np.ndarray) and B.shape == (n, n) and np.iscomplexobj(B)
        S = sum(abs(W[i, j]) * absS[j] for j in range(k))
        bound = 2 * pc.cbound(k, S) + sum(abs(W[i, j] - Wref[i, j]) * absS[j] for j in range(k))
        worst = max(worst, float(np.max(np.abs(B - ref[i]) / bound)))
        worst2 = max(worst2, float(np.max(np.abs(B - B2) / bound)))
    print("coefficients: %.3g of the bound from NumPy, %.3g from the host-sample route" % (worst, worst2))
    assert worst <= 1.0 and worst2 <= 1.0
    # samples assembled in chunks (7 nodes at a time: 7, 7, 6) give the same calls in the same order: the same bits
    from nep_amd import nep as nepmod
    words = nepmod.INTERP_SAMPLE_WORDS
    nepmod.INTERP_SAMPLE_WORDS = 7 * n * n
    try:
        chunked = na.ChebPEP(nep, k, a, b)
    finally:
        nepmod.INTERP_SAMPLE_WORDS = words
    assert all(np.array_equal(B, Bc) for B, Bc in zip(cp.get_Av(), chunked.get_Av()))
    for xj, S in zip(x, samples):
        assert np.linalg.norm(S - cp.compute_Mder(xj)) < EPS * 100
    # iar on the interpolant
    tol = 1e-10
    lam, V, _ = na.iar(cp, sigma=8.8, v=np.ones(n), neigs=1, maxit=50, tol=tol, errmeasure=na.ResidualErrmeasure(cp))
    _, P = bc.chebpep_numpy(bc.mfun("full96"), k, a, b)
    lam_np, _, _ = bc.augnewton_numpy(P, 8.8, np.ones(n))
    U_, s_, Vh_ = np.linalg.svd(P(lam_np))
    kappa = 1.0 / abs(U_[:, -1].conj() @ P(lam_np, 1) @ Vh_[-1].conj())          # |d lam| <= kappa ||residual|| to first order
    print("iar on the ChebPEP: %r; NumPy interpolant: %r (%.3g from lam_ref); kappa = %.3g" % (lam[0], lam_np, abs(lam_np - bc.LAM_REF), kappa))
    assert abs(lam[0] - lam_np) <= 2 * tol * kappa + 1e-12 * abs(lam_np)
    assert abs(lam[0] - bc.LAM_REF) <= abs(lam_np - bc.LAM_REF) + 2 * tol * kappa + 1e-12 * abs(lam_np)


BEYN = dict(sigma=8.8, radius=0.3, N=32, k=3)


def test_contour_beyn_finds_the_one_eigenvalue_in_the_disc(na, nep):
    """the disc |lam - 8.8| < 0.3 holds exactly one eigenvalue, lam_ref.  Parameters: N = 32 nodes, k = 3 probe columns; the NumPy
    restatement of Beyn's method with the same parameters finds it on the CPU first.  Tolerance 1e-7 |lam_ref|: the trapezoidal
    rule lets the eigenvalues outside (the nearest ~0.6 from the centre) leak in with (0.3 / 0.6)^32 = 2e-10, three orders below."""
    found = bc.beyn_numpy(bc.mfun("full96"), 96, BEYN["sigma"], BEYN["radius"], BEYN["N"], BEYN["k"])
    assert len(found) == 1 and abs(found[0] - bc.LAM_REF) <= 1e-7 * abs(bc.LAM_REF), found
    lam, V = na.contour_beyn(nep, neigs=3, linsolvercreator=na.BackslashLinSolverCreator(workers=0), **BEYN)
    print("contour_beyn: %r (NumPy: %r)" % (lam, found))
    assert len(lam) == 1 and V.shape == (96, 1)
    assert abs(lam[0] - bc.LAM_REF) <= 1e-7 * abs(bc.LAM_REF)
