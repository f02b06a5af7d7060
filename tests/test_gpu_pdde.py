"""The periodic-delay NEP on the device: nep_pdde_* (csrc/pdde.hip, K15) through the raw C ABI on the cases and within the bounds
of tests/pdde_checkers.py, the answers the reference publishes for nep_gallery("periodicdde"), the drivers that have to run on a
PeriodicDDE_NEP (newton, augnewton, quasinewton, resinv, contour_beyn, ChebPEP + iar), and one test at the size of the benchmark."""
import ctypes as ct
import os

import numpy as np
import pytest
import torch

import pdde_checkers as pc

pytestmark = pytest.mark.gpu
EPS = np.finfo(float).eps
C_vp = ct.c_void_p
NANC = complex(np.nan, np.nan)
LEAD, TRAIL = 5, 7
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pdde_rand0_eigs.npz")


@pytest.fixture(scope="module")
def na():
    import nep_amd
    if nep_amd.device_count() < 1:
        pytest.skip("no GPU")
    return nep_amd


def _ptr(a):
    return a.ctypes.data_as(C_vp)


def _stream():
    from nep_amd.nep import stream_ptr
    return stream_ptr()


# ---- the raw ABI ------------------------------------------------------------------------------------------------------------------
_HANDLES = {}


def _handle(prob):
    """one handle per problem dict (kept alive for the module)"""
    from nep_amd import _lib
    key = id(prob)
    if key not in _HANDLES:
        mA, n = prob["A"].shape[0], prob["A"].shape[1]
        mB = prob["B"].shape[0]
        Ad = np.ascontiguousarray(prob["A"].transpose(0, 2, 1)); Bd = np.ascontiguousarray(prob["B"].transpose(0, 2, 1))
        al = np.ascontiguousarray(prob["alpha"], dtype=np.complex128); be = np.ascontiguousarray(prob["beta"], dtype=np.complex128)
        h = C_vp()
        rc = _lib.lib.nep_pdde_create(n, mA, mB, _ptr(Ad), _ptr(Bd), prob["N"], prob["tau"], _ptr(al), _ptr(be), ct.byref(h))
        assert rc == 0, rc
        _HANDLES[key] = (h, prob)
    return _HANDLES[key][0]


def _mm(prob, S, E, V, ldv=None, ldo=None, padV=3, padO=2):
    """nep_pdde_mm on host blocks S, E (nsys, p, p), V (n, nsys, p) -> Out (n, nsys, p), after the checks every call gets: the NaN
    guard words and padding rows of Out untouched, V unchanged"""
    from nep_amd import _lib
    n, nsys, p = V.shape
    ldv = n if ldv is None else ldv
    ldo = n if ldo is None else ldo
    sV, sO = ldv * p + padV, ldo * p + padO
    Sd = np.ascontiguousarray(S.transpose(0, 2, 1), dtype=np.complex128); Ed = np.ascontiguousarray(E.transpose(0, 2, 1), dtype=np.complex128)
    vbuf = np.full(LEAD + sV * nsys + TRAIL, NANC, dtype=np.complex128)
    vidx = LEAD + np.arange(nsys)[None, :, None] * sV + np.arange(p)[None, None, :] * ldv + np.arange(n)[:, None, None]
    vbuf[vidx] = V
    Vd = torch.from_numpy(vbuf).to("cuda")
    Od = torch.full((LEAD + sO * nsys + TRAIL,), NANC, dtype=torch.complex128, device="cuda")
    oidx = LEAD + np.arange(nsys)[None, :, None] * sO + np.arange(p)[None, None, :] * ldo + np.arange(n)[:, None, None]
    rc = _lib.lib.nep_pdde_mm(_handle(prob), nsys, p, _ptr(Sd), _ptr(Ed), C_vp(Vd.data_ptr() + 16 * LEAD), ldv, sV,
                              C_vp(Od.data_ptr() + 16 * LEAD), ldo, sO, _stream())
    assert rc == 0, rc
    torch.cuda.synchronize()
    o = Od.cpu().numpy()
    keep = np.ones(o.shape[0], dtype=bool); keep[oidx.reshape(-1)] = False
    assert np.all(np.isnan(o[keep].real)) and np.all(np.isnan(o[keep].imag)), "nep_pdde_mm wrote outside the blocks of Out"
    assert Vd.cpu().numpy().tobytes() == vbuf.tobytes(), "nep_pdde_mm modified V"
    return o[oidx]


def _mder(prob, lams, der, ld=None, pad=3):
    from nep_amd import _lib
    n = prob["A"].shape[1]
    ld = n if ld is None else ld
    la = np.ascontiguousarray(lams, dtype=np.complex128)
    stride = ld * n + pad
    buf = torch.full((LEAD + stride * len(la) + TRAIL,), NANC, dtype=torch.complex128, device="cuda")
    rc = _lib.lib.nep_pdde_mder(_handle(prob), len(la), _ptr(la), der, C_vp(buf.data_ptr() + 16 * LEAD), ld, stride, _stream())
    assert rc == 0, rc
    torch.cuda.synchronize()
    b = buf.cpu().numpy()
    idx = LEAD + np.arange(len(la))[:, None, None] * stride + np.arange(n)[None, None, :] * ld + np.arange(n)[None, :, None]   # [l, r, c]
    keep = np.ones(b.shape[0], dtype=bool); keep[idx.reshape(-1)] = False
    assert np.all(np.isnan(b[keep].real)), "nep_pdde_mder wrote outside the matrices"
    return b[idx]


@pytest.mark.parametrize("shape", pc.SHAPES, ids=pc.case_id)
def test_exact_cases(na, shape):
    """Gaussian-integer data, h = 1/4, tables and S multiples of 6 (E is not exp(-tau S)): the result has no rounding error in
    float64 (proved by the checker in integers) and the device reproduces it byte for byte, with leading dimensions n and n + 3"""
    prob, S, E, V, ref = pc.exact_case(shape)
    n = shape[0]
    out = _mm(prob, S, E, V)
    assert np.array_equal(out, ref), "%s: %d entries differ" % (pc.case_id(shape), int(np.sum(out != ref)))
    assert out.tobytes() == ref.tobytes()
    out3 = _mm(prob, S, E, V, ldv=n + 3, ldo=n + 2)
    assert out3.tobytes() == out.tobytes()


@pytest.mark.parametrize("shape", pc.BOUNDED_SHAPES, ids=pc.case_id)
def test_bounded_cases(na, shape):
    """random complex data, E = exp(-tau S): within c u Ybar of the long double evaluation; two runs of the batch give the same
    bits; a system gives the same bits alone as at its position in the batch"""
    prob, S, E, V, ref, bound = pc.bounded_case(shape)
    n, p, nsys = shape[:3]
    out = _mm(prob, S, E, V, ldv=n + 1, ldo=n + 3)
    r = pc.check_bounded(shape, out, "device mm")
    print("%s: device at %.3g of the bound" % (pc.case_id(shape), r))
    assert _mm(prob, S, E, V).tobytes() == out.tobytes(), "two runs differ"
    for s in {7 if nsys > 7 else nsys - 1, nsys - 1}:                           # (the last one sits in a partly filled tile)
        solo = _mm(prob, S[s:s + 1], E[s:s + 1], V[:, s:s + 1, :])
        assert solo[:, 0, :].tobytes() == np.ascontiguousarray(out[:, s, :]).tobytes(), "system %d differs from its solo run" % s


@pytest.mark.parametrize("der", [0, 1, 3])
@pytest.mark.parametrize("shape", [(3, 3, 20, 2, 3, 2), (17, 1, 20, 7, 3, 2), (65, 1, 3, 7, 1, 1)], ids=pc.case_id)
def test_mder_cases(na, shape, der):
    """nep_pdde_mder for 1 and 3 shifts against the checker's Jordan-block reference, under the bound times der!; the matrix of
    a shift has the same bits alone and in the batch"""
    prob = pc.bounded_case(shape)[0]
    lams = [0.3 - 0.2j, -1.5 + 2j, 2.5]
    out = _mder(prob, lams, der, ld=shape[0] + 2)
    worst = 0.0
    for lam, M in zip(lams, out):
        ref, bound = pc.mder_sweep(prob, lam, der, pc.LD), pc.mder_bound(prob, lam, der)
        worst = max(worst, float(np.max(pc.abs_err(M, ref) / bound)))
    print("%s der %d: mder at %.3g of the bound" % (pc.case_id(shape), der, worst))
    assert worst <= 1.0
    assert _mder(prob, lams[1:2], der)[0].tobytes() == out[1].tobytes()


@pytest.mark.parametrize("n,der,nlam", [(130, 0, 33), (130, 1, 8), (65, 3, 16), (65, 0, 16), (65, 0, 8), (257, 0, 8), (257, 1, 4)])
def test_wide_tiles_give_the_bits_of_narrow_ones(na, n, der, nlam):
    """batches large enough for tiles of 8, 4 and 2 systems (n nlam systems cut into at least 256 tiles; in this order: 8, 4, 2, 4, 2,
    8, 4 systems per tile), below and above 256 rows: the matrix of shift 5 (3 for the short batch) has the bits of its solo run,
    which takes tiles of one system and is inside the bound"""
    shape = {130: (130, 3, 20, 1, 2, 1), 65: (65, 1, 3, 7, 1, 1), 257: (257, 2, 3, 1, 1, 1)}[n]
    prob = pc.bounded_case(shape)[0]
    lams = [complex(0.1 * l - 1.0, 0.05 * l) for l in range(nlam)]
    l = 5 if nlam > 5 else 3
    out = _mder(prob, lams, der)
    solo = _mder(prob, lams[l:l + 1], der, ld=n + 1)[0]
    assert out[l].tobytes() == solo.tobytes()
    assert _mder(prob, lams, der).tobytes() == out.tobytes(), "two runs differ"
    if n != 257:
        ref, bound = pc.mder_sweep(prob, lams[l], der, pc.LD), pc.mder_bound(prob, lams[l], der)
        assert float(np.max(pc.abs_err(solo, ref) / bound)) <= 1.0


def test_error_codes(na):
    from nep_amd import _lib
    lib, ARG = _lib.lib, _lib.NEP_ERR_ARG
    prob, S, E, V, _ = pc.exact_case(pc.SHAPES[1])
    n = 2
    A = np.zeros((513 * 513,), dtype=np.complex128)
    tab = np.ones((3, 1), dtype=np.complex128)
    h = C_vp()
    assert lib.nep_pdde_create(513, 1, 1, _ptr(A), _ptr(A), 1, 1.0, _ptr(tab), _ptr(tab), ct.byref(h)) == ARG and not h.value
    assert lib.nep_pdde_create(0, 1, 1, _ptr(A), _ptr(A), 1, 1.0, _ptr(tab), _ptr(tab), ct.byref(h)) == ARG
    assert lib.nep_pdde_create(2, 0, 1, _ptr(A), _ptr(A), 1, 1.0, _ptr(tab), _ptr(tab), ct.byref(h)) == ARG
    assert lib.nep_pdde_create(2, 1, 0, _ptr(A), _ptr(A), 1, 1.0, _ptr(tab), _ptr(tab), ct.byref(h)) == ARG
    assert lib.nep_pdde_create(2, 1, 1, _ptr(A), _ptr(A), 0, 1.0, _ptr(tab), _ptr(tab), ct.byref(h)) == ARG
    assert lib.nep_pdde_create(2, 1, 1, None, _ptr(A), 1, 1.0, _ptr(tab), _ptr(tab), ct.byref(h)) == ARG
    hh = _handle(prob)
    info = (ct.c_int64 * 4)()
    assert lib.nep_pdde_info(hh, info) == 0 and (info[0], info[1], info[3]) == (n, prob["N"], 8) and info[2] > 0
    assert lib.nep_pdde_info(None, info) == ARG
    buf = torch.full((4096,), NANC, dtype=torch.complex128, device="cuda")
    p_, st = C_vp(buf.data_ptr()), _stream()
    S9 = np.zeros(81, dtype=np.complex128)
    lam = np.array([1.0 + 0j])
    assert lib.nep_pdde_mm(hh, 1, 9, _ptr(S9), _ptr(S9), p_, n, 18, p_, n, 18, st) == ARG          # p = 9
    assert lib.nep_pdde_mm(hh, 1, 0, _ptr(S9), _ptr(S9), p_, n, 18, p_, n, 18, st) == ARG
    assert lib.nep_pdde_mm(None, 1, 1, _ptr(S9), _ptr(S9), p_, n, 2, p_, n, 2, st) == ARG
    assert lib.nep_pdde_mm(hh, 1, 1, _ptr(S9), _ptr(S9), p_, n - 1, 2, p_, n, 2, st) == ARG        # ldv < n
    assert lib.nep_pdde_mm(hh, 1, 1, _ptr(S9), _ptr(S9), p_, n, 2, p_, n - 1, 2, st) == ARG
    assert lib.nep_pdde_mm(hh, 1, 1, None, _ptr(S9), p_, n, 2, p_, n, 2, st) == ARG
    assert lib.nep_pdde_mder(hh, 1, _ptr(lam), 8, p_, n, 4, st) == ARG                             # der = 8 needs p = 9
    assert lib.nep_pdde_mder(hh, 1, _ptr(lam), -1, p_, n, 4, st) == ARG
    assert lib.nep_pdde_mder(hh, 1, _ptr(lam), 0, p_, n - 1, 4, st) == ARG
    assert lib.nep_pdde_mm(hh, 0, 1, None, None, None, n, 2, None, n, 2, st) == 0                  # empty batches are no-ops
    assert lib.nep_pdde_mder(hh, 0, None, 0, None, n, 4, st) == 0
    torch.cuda.synchronize()
    assert np.all(np.isnan(buf.cpu().numpy().real))                                                # nothing was launched
    assert lib.nep_pdde_destroy(None) == 0


# ---- the answers the reference publishes for "mathieu" (periodic_dde.jl:280-296, test/newton.jl:57-64) --------------------------------
LAM0 = -0.24470143590830754
LAM1 = -0.561610418452567 - 1.511169478595549j


@pytest.fixture(scope="module")
def mathieu(na):
    return na.nep_gallery("periodicdde", name="mathieu")


def test_newton_reaches_the_published_eigenpair(na, mathieu):
    assert isinstance(mathieu, na.PeriodicDDE_NEP) and mathieu.size() == (2, 2) and mathieu.N == 1000 and not mathieu.issparse()
    lam, v = na.newton(mathieu, lam=-0.2, v=np.array([1.0, 1.0]))
    print("newton: %r, %.3g from the published value" % (lam, abs(lam - LAM0)))
    assert abs(lam - LAM0) <= 1e-12
    assert abs(np.exp(mathieu.tau * lam) - 0.6129923199095035) <= 1e-10
    w = np.array([0.970208, -0.242272])
    cosang = abs(np.vdot(w, v)) / (np.linalg.norm(w) * np.linalg.norm(v))
    assert np.sqrt(max(0.0, 1 - cosang ** 2)) <= 1e-5
    with pytest.raises(na.NoConvergenceException):
        na.newton(mathieu, lam=-0.2, v=np.array([1.0, 1.0]), maxit=1)


def test_newton_on_a_sparse_spmf(na):
    """the sparse branch of newton (bordered sparse LU) on dep0_sparse (n = 100).  The eigenpair nearest 0 is found on the host
    first (the eigenvalue of M(0) of smallest modulus as a guess, polished by the checker's NumPy Newton: sigma_min(M) / sigma_max
    is 3e-17 there, the next singular value 0.13); newton and augnewton, started 0.01 away with a perturbed eigenvector, both
    return it to 1e-10: they stop at a backward error < 100 eps, and 1 / (gap 0.13) of that is far inside"""
    nep = na.nep_gallery("dep0_sparse", 100)
    assert nep.issparse()
    M = lambda lam, der=0: nep.compute_Mder(lam, der).toarray()
    w, X = np.linalg.eig(M(0.0))
    j = int(np.argmin(abs(w)))
    lam_ref, v_ref = pc.newton_polish(M, complex(w[j]), X[:, j].astype(complex))
    sv = np.linalg.svd(M(lam_ref), compute_uv=False)
    assert sv[-1] <= 1e-14 * sv[0] and sv[-2] >= 0.05
    v0 = v_ref / np.linalg.norm(v_ref) + 0.01 * np.ones(100) / 10
    lam_n, vn = na.newton(nep, lam=lam_ref + 0.01, v=v0, maxit=20)
    lam_a, va = na.augnewton(nep, lam=lam_ref + 0.01, v=v0, maxit=20)
    print("dep0_sparse: host %r, newton %r, augnewton %r" % (lam_ref, lam_n, lam_a))
    assert abs(lam_n - lam_ref) <= 1e-10 and abs(lam_a - lam_ref) <= 1e-10
    assert nep.compute_resnorm(lam_n, vn) <= 1e-12 * sv[0]


def test_resinv_from_the_reference_start(na, mathieu):
    """test/newton.jl:57-64: resinv from lam = -0.2, v = [1, 1] until compute_resnorm < 100 eps"""
    lam, v = na.resinv(mathieu, lam=-0.2, v=np.array([1.0, 1.0]), maxit=30)
    res = mathieu.compute_resnorm(lam, v)
    print("resinv: %r, resnorm %.3g" % (lam, res))
    assert res < 100 * EPS
    assert abs(lam - LAM0) <= 1e-10


@pytest.mark.parametrize("method", ["augnewton", "quasinewton"])
def test_augnewton_and_quasinewton(na, mathieu, method):
    lam, v = getattr(na, method)(mathieu, lam=-0.2, v=np.array([1.0, 1.0]))
    print("%s: %r" % (method, lam))
    assert abs(lam - LAM0) <= 1e-10


def test_augnewton_reaches_a_complex_published_eigenvalue(na, mathieu):
    lam, v = na.augnewton(mathieu, lam=LAM1 + 0.03 + 0.04j, v=np.array([1.0, 1.0]))
    print("augnewton: %r, %.3g away" % (lam, abs(lam - LAM1)))
    assert abs(lam - LAM1) <= 1e-10


def test_mlincomb_and_mder_identities_on_the_device(na, mathieu):
    """compute_Mlincomb = sum a_j M^(j + sd) v_j with the matrices of compute_Mder, to 1e-12 of the sum of the terms' norms;
    k + startder > 8 names the interpolation route"""
    rng = np.random.default_rng(3)
    lam = -0.3 + 0.4j
    V = rng.standard_normal((2, 3)) + 1j * rng.standard_normal((2, 3))
    a = np.array([2.0, -1j, 0.5])
    for sd in (0, 1, 2):
        z = mathieu.compute_Mlincomb(lam, V, a, startder=sd)
        terms = [a[j] * mathieu.compute_Mder(lam, j + sd) @ V[:, j] for j in range(3)]
        assert np.linalg.norm(z - sum(terms)) <= 1e-12 * sum(np.linalg.norm(t) for t in terms)
    zd = mathieu.compute_Mlincomb(lam, na.to_dev(V), a, startder=1)
    assert torch.is_tensor(zd) and np.array_equal(zd.cpu().numpy(), mathieu.compute_Mlincomb(lam, V, a, startder=1))
    with pytest.raises(ValueError, match="ChebPEP"):
        mathieu.compute_Mlincomb(lam, np.ones((2, 8)), startder=1)
    MM = mathieu.compute_MM(np.array([[lam]]), V[:, :1])
    assert np.linalg.norm(MM[:, 0] - mathieu.compute_Mder(lam) @ V[:, 0]) <= 1e-13 * np.linalg.norm(V[:, 0]) * 10
    mathieu50 = na.nep_gallery("periodicdde", name="mathieu", N=50)
    M50 = mathieu50.compute_Mder(lam)
    mathieu50.N = 1000                                                  # settable, as in the reference
    assert mathieu50.N == 1000 and np.array_equal(mathieu50.compute_Mder(lam), mathieu.compute_Mder(lam))
    assert not np.array_equal(M50, mathieu.compute_Mder(lam))


# ---- rand0 ------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def rand0(na):
    return na.nep_gallery("periodicdde", name="rand0", **pc.RAND0)


def test_contour_beyn_returns_the_fixture_set(na, rand0):
    """the eigenvalues of rand0 (n = 24, N = 64) inside the disc of the fixture (computed on the CPU by the checker, regenerated and
    compared by test_host_pdde.py): contour_beyn returns exactly that set to 1e-8, every residual norm <= 1e-9"""
    fix = np.load(GOLDEN)
    want = fix["eigs"]
    calls = []
    dev0 = rand0.compute_Mder_dev
    rand0.compute_Mder_dev = lambda lams, der=0: (calls.append((len(lams), der)), dev0(lams, der))[1]
    try:
        lam, V = na.contour_beyn(rand0, neigs=len(want) + 4, sigma=complex(fix["sigma"]), radius=float(fix["radius"]),
                                 N=pc.RAND0_NODES, k=12, linsolvercreator=na.BackslashLinSolverCreator(workers=0))
    finally:
        del rand0.compute_Mder_dev
    assert calls == [(pc.RAND0_NODES, 0)], calls                       # the matrices of all nodes from ONE nep_pdde_mder call
    print("contour_beyn: %r\nfixture: %r" % (np.sort_complex(lam), np.sort_complex(want)))
    assert len(lam) == len(want)
    for w in want:
        assert np.min(np.abs(lam - w)) <= 1e-8, w
    for l, v in zip(lam, V.T):
        assert rand0.compute_resnorm(l, v) <= 1e-9


def test_chebpep_then_iar_finds_the_real_eigenvalue(na, mathieu):
    """rand0 (n = 24, N = 64) has no real eigenvalue in [-1, 3] (det M(x) keeps its sign there; pdde_checkers.py) and none in the
    disc of the fixture, so this runs on "mathieu": ChebPEP(nep, 24, -1, 0.5) takes its samples through compute_Mder_dev in one
    batched call, and iar on the polynomial finds -0.2447... to 1e-8"""
    calls = []
    dev0 = mathieu.compute_Mder_dev
    mathieu.compute_Mder_dev = lambda lams, der=0: (calls.append(len(lams)), dev0(lams, der))[1]
    try:
        cp = na.ChebPEP(mathieu, 24, -1.0, 0.5)
    finally:
        del mathieu.compute_Mder_dev
    assert calls == [24], calls
    x = na.chebyshev_nodes(-1.0, 0.5, 24)
    assert np.linalg.norm(cp.compute_Mder(x[3]) - mathieu.compute_Mder(x[3])) <= 1e-12
    lam, V, _ = na.iar(cp, sigma=-0.2, v=np.ones(2), neigs=1, maxit=40, tol=1e-11, errmeasure=na.ResidualErrmeasure(cp))
    print("iar on the ChebPEP: %r, %.3g from the published value" % (lam[0], abs(lam[0] - LAM0)))
    assert abs(lam[0] - LAM0) <= 1e-8


def test_full_size_mder(na):
    """compute_Mder_dev of rand0 at n = 200, N = 1000 (the benchmark's size) for 3 shifts; one of them against the float64 NumPy
    evaluation under the bounded-case bound"""
    nep = na.nep_gallery("periodicdde", name="rand0")
    assert nep.size(1) == 200 and nep.N == 1000
    lams = [0.5 + 0.5j, -0.2 + 1j, 1.0]
    D = nep.compute_Mder_dev(lams)
    assert tuple(D.shape) == (3, 200, 200)
    M = D[1].cpu().numpy()
    prob = pc.problem_of(nep)
    ref = pc.mder_sweep(prob, lams[1], 0)
    bound = pc.mder_bound(prob, lams[1], 0)
    r = float(np.max(pc.abs_err(M, pc.CA(ref.re.astype(pc.LD), ref.im.astype(pc.LD))) / bound))
    print("n = 200, N = 1000: device against float64 NumPy at %.3g of the bound" % r)
    assert r <= 1.0
    # The majorant grows like the exponential of the norms, so at this size the bound above admits any finite matrix.  What has teeth:
    # the two float64 evaluations differ by rounding only.  With rounding errors adding up like a random walk, a stage contributes
    # about (sqrt(n) + 5) u = 19 u relative to the largest entry (inner sums of n terms, the few operations around them) and the
    # 4 N = 4000 stages sqrt(4000) times that: 1.3e-13 per evaluation, 2.7e-13 for the difference of two.  The tolerance is 1e-12 of
    # the largest entry; a wrong table row, term or column mapping misses it by many orders.
    Mn = ref.c128()
    rel = float(np.max(np.abs(M - Mn)) / np.max(np.abs(Mn)))
    print("largest difference / largest entry: %.3g" % rel)
    assert rel <= 1e-12
    B = nep.compute_Mder_batch(lams)
    assert isinstance(B, np.ndarray) and B.shape == (3, 200, 200) and np.array_equal(B[1], M)
    assert np.array_equal(nep.compute_Mder(lams[2]), B[2])
