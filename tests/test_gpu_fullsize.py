"""Full-size (BASELINE.json configs) GPU checks: eigenpair counts + independently re-evaluated residuals, and
size-independent properties of the kernels (linearity, orthogonality, agreement with host SciPy where the host
finishes in seconds)."""
import numpy as np
import pytest
import scipy.sparse as sp

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def na():
    import nep_amd
    assert nep_amd.device_count() >= 1
    return nep_amd


def test_c2_gun_iar_m100_fullsize(na):
    """config C2: 46 eigenpairs with backward error < 1e-10 (SURVEY.md Appendix B.1 probe: 46 at k=100)"""
    nep = na.nep_gallery("gun_spmf_scaled"); n = nep.n
    hist = []
    lam, Q, V = na.iar(nep, sigma=0.0, gamma=1.0, maxit=100, neigs=np.inf, v=np.ones(n), tol=1e-10, errhist=hist)
    assert len(lam) == 46
    Av = nep.get_Av(); fv = nep.get_fv(); fro = nep.fro_norms()
    for s in range(len(lam)):                                     # host FP64 re-evaluation, reference criterion
        r = sum(f(lam[s]) * (A @ Q[:, s]) for A, f in zip(Av, fv))
        den = sum(c * abs(f(lam[s])) for c, f in zip(fro, fv)) * np.linalg.norm(Q[:, s])
        assert np.linalg.norm(r) / den < 1e-10
    # eigenvalues of the scaled problem map into the physical gun window (Re lam in [4.1e4, 8.5e4], Im > 0)
    phys = 250.0 ** 2 + (330.0 ** 2 - 220.0 ** 2) * lam
    assert np.all((phys.real > 4.0e4) & (phys.real < 8.6e4) & (phys.imag > 0))
    # Krylov basis orthonormal (test/iar.jl:41-47 criterion) -- checked on the device-resident V through host download of V^H V
    Vh = na.to_host(V[:20, :21 * n])[:21 * n]
    assert np.linalg.norm(Vh.conj().T @ Vh - np.eye(20), 2) < 1e-10
    # error history is monotone in the number of converged pairs
    conv = [int(np.sum(h < 1e-10)) for h in hist]
    assert conv[-1] == 46 and all(b >= a - 2 for a, b in zip(conv, conv[1:]))
    # SURVEY.md section 8d parity rules (i), (iii), (iv) against the CPU oracle ON THE SAME full-size configuration (about 10 s):
    # same count, eigenvalue multiset to 1e-8 relative, per-iteration error history within a factor 10 above 1e-12
    bc = _bc()
    lo, oh = _c2_oracle(n)
    par = bc.c2_parity(lam, hist, lo, oh)
    assert par["same_count"] and par["eigenvalues_match_1e-8"], par
    assert par["history_within_x10_above_1e-12"] and par["history_entries_compared"] > 100, par


_C2_ORACLE = {}


def _c2_oracle(n):
    """the CPU oracle on config C2 (about 10 s), once per test process"""
    if n not in _C2_ORACLE:
        oh = []
        lo, _ = _bc().c2_oracle(n, maxit=100, hist=oh)
        _C2_ORACLE[n] = (lo, oh)
    return _C2_ORACLE[n]


def test_c2_through_the_c_abi_only_in_the_julia_call_order(na):
    """config C2 driven through ctypes ONLY, in the call order of `iar(::Type{T}, nep::DeviceSPMF; ...)` of julia/NEPMI355X.jl
    (no iar.py, no linsolvers.py, no nep.py device wrappers): DeviceSPMF(org) = nep_spmf_create on the CSR of each term;
    create_linsolver(DeviceLinSolverCreator) = a host LU (SuperLU here, UMFPACK there) -> nep_lu_create_csc; derivative table,
    |f_t(sigma)|, ||A_t||_F on the host; ONE nep_iar_run with the f_t(lambda) callback.  46 pairs, parity with the CPU oracle by
    SURVEY section 8d rules (i), (iii), (iv); residuals re-evaluated on the host."""
    import ctypes as C
    import scipy.sparse.linalg as spla
    from nep_amd import _lib
    lib = _lib.lib
    nep = na.nep_gallery("gun_spmf_scaled"); n = nep.n
    Av = [sp.csr_matrix(A) for A in nep.get_Av()]; fv = nep.get_fv(); mt = len(Av)
    # ---- DeviceSPMF(org)
    keep = []
    rp = (C.c_void_p * mt)(); ci = (C.c_void_p * mt)(); vv = (C.c_void_p * mt)(); isc = (C.c_int32 * mt)()
    for t, A in enumerate(Av):
        A.sort_indices()
        r = np.ascontiguousarray(A.indptr, dtype=np.int32); c = np.ascontiguousarray(A.indices, dtype=np.int32)
        cplx = np.iscomplexobj(A.data) and np.any(A.data.imag != 0)
        v = np.ascontiguousarray(A.data, dtype=np.complex128 if cplx else np.float64)
        keep += [r, c, v]
        rp[t] = r.ctypes.data; ci[t] = c.ctypes.data; vv[t] = v.ctypes.data; isc[t] = 1 if cplx else 0
    spmf = C.c_void_p()
    _lib.check(lib.nep_spmf_create(n, mt, rp, ci, vv, isc, C.byref(spmf)))
    # ---- create_linsolver(DeviceLinSolverCreator(), nep, sigma): host factorisation of M(sigma), factors to the device as they are
    sigma = 0.0 + 0.0j; gamma = 1.0 + 0.0j; m = 100
    cf = np.ascontiguousarray([f(sigma) for f in fv], dtype=np.complex128); cabs = np.ascontiguousarray(np.abs(cf))
    M0 = sp.csc_matrix(sum(c * A for c, A in zip(cf, Av)), dtype=np.complex128)
    F = spla.splu(M0, permc_spec="MMD_AT_PLUS_A", diag_pivot_thresh=0.0, options=dict(SymmetricMode=True))
    L = sp.csc_matrix(F.L); U = sp.csc_matrix(F.U)
    arr = [np.ascontiguousarray(x, dtype=np.int32) for x in (L.indptr, L.indices, U.indptr, U.indices, F.perm_r, F.perm_c)]
    Lx = np.ascontiguousarray(L.data, dtype=np.complex128); Ux = np.ascontiguousarray(U.data, dtype=np.complex128)
    lu = C.c_void_p()
    _lib.check(lib.nep_lu_set_expected_solves(200))
    _lib.check(lib.nep_lu_create_csc(n, _lib.hptr(arr[0]), _lib.hptr(arr[1]), _lib.hptr(Lx), _lib.hptr(arr[2]), _lib.hptr(arr[3]),
                                     _lib.hptr(Ux), _lib.hptr(arr[4]), _lib.hptr(arr[5]), C.byref(lu)))
    # ---- host inputs of the run: Ctab[j-1, t] = gamma^j / j f_t^(j)(sigma), ||A_t||_F, the callback
    fD = np.column_stack([f.derivs(sigma, m + 1) for f in fv])
    Ctab = np.asfortranarray((gamma ** np.arange(1, m + 1) / np.arange(1, m + 1))[:, None] * fD[1:m + 1, :], dtype=np.complex128)
    fro = np.ascontiguousarray([np.sqrt((abs(A.data) ** 2).sum()) for A in Av])
    ncalls = [0]

    def fv_eval(ctx, nlam, lam_p, F_p):
        la = np.frombuffer((C.c_double * (2 * nlam)).from_address(lam_p), dtype=np.complex128)
        Fm = np.frombuffer((C.c_double * (2 * nlam * mt)).from_address(F_p), dtype=np.complex128).reshape(nlam, mt)
        for t, f in enumerate(fv):
            Fm[:, t] = [f(x) for x in la]
        ncalls[0] += 1
        return 0
    cb = _lib.FV_EVAL(fv_eval)
    o = _lib.IarOpts(m, 1, 0, 10, 1, -1, 1e-10, float("inf"), _lib.cdouble(0.0, 0.0), _lib.cdouble(1.0, 0.0))
    res = _lib.IarResult()
    lam = np.zeros(m, dtype=np.complex128); Q = np.zeros((m, n), dtype=np.complex128); err = np.full((m, m), np.nan, order="F")
    v0 = np.ones(n, dtype=np.complex128)
    st = lib.nep_iar_run(spmf, lu, n, C.addressof(o), _lib.hptr(v0), _lib.hptr(Ctab), mt, _lib.hptr(cabs), _lib.hptr(cf), _lib.hptr(fro),
                         C.cast(cb, C.c_void_p), None, _lib.hptr(lam), None, _lib.hptr(Q), _lib.hptr(err), None, C.addressof(res), None)
    _lib.check(st)
    assert res.k == m and res.nret == 46 and res.nconv == 46 and ncalls[0] == m and res.retry_reason == 0
    assert 1 <= res.refine_plan <= 2
    lam = lam[:res.nret]; Q = Q[:res.nret].T
    for s in range(len(lam)):                                     # host FP64 re-evaluation, the reference's criterion
        r = sum(f(lam[s]) * (A @ Q[:, s]) for A, f in zip(Av, fv))
        den = sum(c * abs(f(lam[s])) for c, f in zip(fro, fv)) * np.linalg.norm(Q[:, s])
        assert np.linalg.norm(r) / den < 1e-10
    hist = [err[kc - 1, :kc].copy() for kc in range(1, m + 1)]
    assert all(np.all(np.diff(h) >= 0) for h in hist)             # every row sorted (method_iar.jl:150-151)
    lo, oh = _c2_oracle(n)
    par = _bc().c2_parity(lam, hist, lo, oh)
    assert par["same_count"] and par["eigenvalues_match_1e-8"], par
    assert par["history_within_x10_above_1e-12"] and par["history_entries_compared"] > 100, par
    # a second run with the learnt refinement count as the hint, and a finite neigs: ends early with exactly neigs pairs
    o2 = _lib.IarOpts(m, 1, 0, 10, 1, res.refine_plan, 1e-10, 12.0, _lib.cdouble(0.0, 0.0), _lib.cdouble(1.0, 0.0))
    res2 = _lib.IarResult(); lam2 = np.zeros(m, dtype=np.complex128)
    _lib.check(lib.nep_iar_run(spmf, lu, n, C.addressof(o2), _lib.hptr(v0), _lib.hptr(Ctab), mt, _lib.hptr(cabs), _lib.hptr(cf), _lib.hptr(fro),
                               C.cast(cb, C.c_void_p), None, _lib.hptr(lam2), None, None, None, None, C.addressof(res2), None))
    assert res2.nret == 12 and res2.nconv >= 12 and res2.k < m
    assert max(np.min(abs(lam - x)) for x in lam2[:12]) < 1e-9
    # too few steps for the request: NEP_ERR_NOCONV, the best pairs are returned all the same
    o3 = _lib.IarOpts(20, 1, 0, 10, 1, res.refine_plan, 1e-10, 30.0, _lib.cdouble(0.0, 0.0), _lib.cdouble(1.0, 0.0))
    res3 = _lib.IarResult(); lam3 = np.zeros(20, dtype=np.complex128)
    st3 = lib.nep_iar_run(spmf, lu, n, C.addressof(o3), _lib.hptr(v0), _lib.hptr(Ctab[:20].copy(order="F")), mt, _lib.hptr(cabs), _lib.hptr(cf),
                          _lib.hptr(fro), C.cast(cb, C.c_void_p), None, _lib.hptr(lam3), None, None, None, None, C.addressof(res3), None)
    assert st3 == _lib.NEP_ERR_NOCONV and res3.k == 20 and res3.nret == 20 and res3.nconv < 30
    _lib.check(lib.nep_lu_destroy(lu)); _lib.check(lib.nep_spmf_destroy(spmf))


def test_c2_pipelined_iar_equals_step_synchronous(na, monkeypatch):
    """the asynchronous pipeline (device-side DGKS decision, event-ordered transfers) and the step-synchronous loop
    (NEP_IAR_SYNC=1) run the same arithmetic: same eigenpair count, eigenvalues to 1e-11 relative, same error history
    length; also with check_error_every=7 and with a finite neigs that stops the iteration early"""
    nep = na.nep_gallery("gun_spmf_scaled"); n = nep.n
    for kw in (dict(maxit=60, neigs=np.inf), dict(maxit=60, neigs=np.inf, check_error_every=7), dict(maxit=100, neigs=12)):
        out = []
        for sync in ("", "1"):
            if sync:
                monkeypatch.setenv("NEP_IAR_SYNC", "1")
            else:
                monkeypatch.delenv("NEP_IAR_SYNC", raising=False)
            hist = []
            lam, Q, _ = na.iar(nep, sigma=0.0, gamma=1.0, v=np.ones(n), tol=1e-10, errhist=hist, **kw)
            out.append((lam, hist))
        (la, ha), (ls, hs) = out
        assert len(la) == len(ls) and len(la) >= 12
        d = [np.min(abs(ls - x)) / max(1.0, abs(x)) for x in la]
        assert max(d) < 1e-11
        if kw["neigs"] == np.inf:
            assert len(ha) == len(hs)


def test_k5_blocked_solve_waveguide_91k(na):
    """K5 at n = 91 195 (WEP 303x299, 2610 plain levels): elimination-tree block schedule; raw solve relative residual
    < 1e-9, after the UMFPACK-style refinement the componentwise backward error is at round-off (< 20 eps)"""
    import scipy.sparse as sp
    nep = na.nep_gallery("WEP", nx=303, nz=299, benchmark_problem="JARLEBRING")
    lam = -3 - 3.5j
    A = sp.csc_matrix(nep.compute_Mder(lam))
    n = nep.n
    rng = np.random.default_rng(3)
    b = rng.standard_normal(n) + 1j * rng.standard_normal(n)
    ls = na.create_linsolver(na.FactorizeLinSolverCreator(), nep, lam)
    lu = ls.lu
    assert lu.block_schedule and lu.levels < 60            # 2610 plain levels -> one or two launches per block level
    x0 = na.to_host(lu.solve(na.to_dev(b)))[:, 0]
    assert np.linalg.norm(A @ x0 - b) <= 1e-9 * np.linalg.norm(b)
    x = na.lin_solve(ls, b)
    # (20 eps since round 4: the top levels are applied as one dense inverse from the FIRST solve of a factor on -- the dense apex build,
    # csrc/trsv_ml.hip -- and the refinement then stagnates at 5-13 eps on this matrix, run to run, where the level walk of the first
    # solves used to stop at 5-9 eps; UMFPACK's rule stops on the same stagnation.  scripts/diag/k5_wep91k_omega.py prints both.)
    assert ls.last_omega < 20 * np.finfo(float).eps and ls.refine_steps_taken <= 2
    assert np.linalg.norm(A @ x - b) <= np.linalg.norm(A @ x0 - b) * 1.01


def test_c5_wep_fullsize_kernels_vs_host(na):
    """config C5 size (nx=1003, nz=999, n=1 003 995): K1 against host SciPy SpMV, linearity, DGKS orthogonality"""
    from nep_amd import wep
    import torch
    wd = wep.WaveguideData(1003, 999, "JARLEBRING")
    Av = wd.big_matrices()
    fv = [na.funcs.one(), na.funcs.ident(), na.funcs.Monomial(2)]
    nep = na.SPMF_NEP(Av, fv)
    n = wd.n
    assert n == 1003995 and sum(A.nnz for A in Av) == 8019972
    rng = np.random.default_rng(0)
    lam = -3 - 3.5j
    v = rng.standard_normal(n) + 1j * rng.standard_normal(n)
    z = nep.compute_Mlincomb(lam, v)                                # SELL-64 folded SpMV
    ref = Av[0] @ v + lam * (Av[1] @ v) + lam ** 2 * (Av[2] @ v)
    assert np.linalg.norm(z - ref) <= 1e-13 * np.linalg.norm(ref)
    k = 6
    V = rng.standard_normal((n, k)) + 1j * rng.standard_normal((n, k))
    a = rng.standard_normal(k); b = rng.standard_normal(k)
    Vd = na.to_dev(V)
    za = na.to_host(nep.compute_Mlincomb(lam, Vd, a).reshape(1, -1))[:, 0]
    zb = na.to_host(nep.compute_Mlincomb(lam, Vd, b).reshape(1, -1))[:, 0]
    zab = na.to_host(nep.compute_Mlincomb(lam, Vd, a + b).reshape(1, -1))[:, 0]
    assert np.linalg.norm(zab - za - zb) <= 1e-13 * np.linalg.norm(zab)          # linearity in a
    refa = sum(a[j] * sum(fv[i].derivs(lam, k)[j] * (Av[i] @ V[:, j]) for i in range(3)) for j in range(k))
    assert np.linalg.norm(za - refa) <= 1e-12 * np.linalg.norm(refa)
    # DGKS at tiar shape: orthogonalise 8 vectors one after another, check Z^H Z = I
    Z = torch.zeros((8, n), dtype=torch.complex128, device="cuda")
    for j in range(8):
        Z[j] = torch.from_numpy(rng.standard_normal(n) + 1j * rng.standard_normal(n)).to("cuda")
        if j == 0:
            na.dense.scal(Z[0], 1.0 / na.dense.nrm2(Z[0]))
        else:
            na.orthogonalize_and_normalize(Z, Z[j], j)
    G = na.to_host(na.gemm_ts(Z, np.eye(8), rowmajor=False))                  # identity GEMM = copy through the MFMA path
    assert np.linalg.norm(G.conj().T @ G - np.eye(8), 2) < 1e-12


def test_c5_wep_fullsize_schur_gmres_round_trip(na):
    """config C5 size, the reference's own solver (Waveguide.jl:428-446,552-567 + waveguide_preconditioner.jl): solve
    M(sigma) x = b through the Schur complement with preconditioned GMRES (27 x 31 regions) and refinement sweeps, then
    apply M(sigma): ||M x - b|| <= 1e-11 ||b|| (size-independent round-trip property; no factorisation at n = 10^6), and the
    solve is linear in b"""
    import torch
    nep = na.nep_gallery("WEP", nx=1003, nz=999, benchmark_problem="JARLEBRING")
    n = nep.n
    sigma = -3 - 3.5j
    P = na.wep_generate_preconditioner(nep, 27, sigma)
    assert P.mm == 27 * 27 + 4 * 27
    cr = na.WEPLinSolverCreator(solver_type="gmres", kwargs=(("Pl", P), ("reltol", 1e-6), ("restart", 60), ("maxiter", 300)),
                                refinements=10)
    solver = na.create_linsolver(cr, nep, sigma)
    rng = np.random.default_rng(0)
    b1 = na.to_dev(rng.standard_normal(n) + 1j * rng.standard_normal(n))[0]
    b2 = na.to_dev(rng.standard_normal(n) + 1j * rng.standard_normal(n))[0]
    x1 = solver.solve_dev(b1).clone(); x2 = solver.solve_dev(b2).clone()
    r = nep.compute_Mlincomb(sigma, x1.reshape(1, n)).reshape(-1) - b1
    assert float(torch.linalg.norm(r) / torch.linalg.norm(b1)) <= 1e-11
    x12 = solver.solve_dev(b1 + 2.0 * b2)
    assert float(torch.linalg.norm(x12 - x1 - 2.0 * x2) / torch.linalg.norm(x12)) <= 1e-9


@pytest.mark.parametrize("k,p,rowmajor", [(60, 60, True), (60, 60, False), (37, 64, True), (80, 13, False), (52, 60, True), (3, 5, False),
                                          (70, 40, True), (93, 20, False), (64, 64, False), (61, 9, True)])
def test_k7_resident_variant_tall_blocks(na, k, p, rowmajor):
    """K7 on blocks tall enough for the B-resident persistent kernel (rows >= 524 288, all B fragments in LDS): against NumPy,
    1e-13 relative per entry scale; both output layouts, k not a multiple of 4, p not a multiple of 8, every N-tile count of the
    resident kernel with both register-buffer sizes (k-steps <= 16 and 17 ... 24; round 3: no k-step padding)"""
    rows = 600_003
    rng = np.random.default_rng(k * 100 + p)
    Z = rng.standard_normal((rows, k)) + 1j * rng.standard_normal((rows, k))
    B = rng.standard_normal((k, p)) + 1j * rng.standard_normal((k, p))
    Y = na.gemm_ts(na.to_dev(Z), B, rowmajor=rowmajor)
    Yh = Y.cpu().numpy() if rowmajor else na.to_host(Y)
    ref = Z @ B
    assert np.linalg.norm(Yh - ref) <= 1e-13 * np.linalg.norm(ref) * np.sqrt(k)


# ---- BASELINE configurations C3, C4, C5 at BASELINE size, through the definitions bench.py uses ---------------------------
def _bc():
    import os
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "scripts"))
    import baseline_configs
    return baseline_configs


def test_c3_gun_nleigs_r1_fullsize_vs_oracle(na):
    """config C3 at n = 9956: nleigs variant R1 (test/nleigs/nleigs_gun_variant_r1.jl arguments) on gun_nep() = PEP +
    LowRankFactorizedNEP; parity rule of SURVEY.md section 8d: same count as the CPU oracle, eigenvalues as multisets to 1e-8
    relative, every pair's backward error (host FP64 re-evaluation on the full SPMF) below the driver tolerance; 5 cached
    factorisations (reusefact = 2, 5 cyclic nodes)"""
    bc = _bc()
    nep = bc.c3_device_nep(na)
    info = {}
    lam, X, res = bc.c3_device(na, nep, info=info)
    assert info["nfact"] == 5 and info["lowrank_r"] == 84
    lo, Xo, ro = bc.c3_oracle(na)
    assert len(lam) == len(lo) >= 15
    ok, worst = bc.match(lam, lo, 1e-8)
    assert ok, worst
    errs = bc.c3_host_errors(nep.n, lam, X)
    assert max(errs) < 1e-10
    Sigma, _ = bc.c3_kwargs(nep.n)
    from nep_amd import rk_helper
    assert np.all(rk_helper.in_Sigma(np.asarray(lam), Sigma, 1e-10))


def test_c4_gun_beyn_n64_k32_fullsize_vs_oracle(na):
    """config C4 at n = 9956, N = 64 nodes, k = 32 (one GPU; the node solves are the ones the sharded integrator
    distributes): same count as the CPU oracle on the same probe block, eigenvalues to 1e-8 relative, inside-contour ones
    first, backward errors < 1e-6 (driver tolerance) re-evaluated on the host"""
    bc = _bc()
    nep = na.nep_gallery("gun_spmf"); nep.dev
    info = {}
    lam, V = bc.c4_device(na, nep, info=info)
    io = {}
    lo, Vo = bc.c4_oracle(na, info=io)
    assert len(lam) == len(lo) >= 20 and info["p"] == io["p"]
    ok, worst = bc.match(lam, lo, 1e-8)
    assert ok, worst
    # method_beyncontour.jl:153-163: accurate eigenvalues outside the contour are kept, moved behind the inside ones
    inside = abs(np.asarray(lam) - 250.0 ** 2) <= 1e4
    assert inside.sum() >= 20 and np.all(np.diff(inside.astype(int)) <= 0)
    assert max(bc.c4_host_errors(nep.n, lam, V)) < 1e-6


def test_c5_wep_tiar_m60_fullsize(na):
    """config C5 at nx = 1003, nz = 999 (n = 1 003 995): tiar m = 60 with the reference's solver for this problem (Schur
    complement + Sylvester-SMW preconditioned GMRES, no factorisation): >= 6 eigenpairs whose residual ||M(lam) v|| / ||v|| is
    below the driver tolerance both by the device's own K1 AND re-evaluated in FP64 on the host by the oracle's matrix-free
    operator (SURVEY.md section 8d rule ii); the 303 x 299 twin is compared with the CPU oracle's tiar on the same twin BY
    EIGENVALUE (rules i, iii), the full-size eigenvalues follow the twin's (discretisation trend: 0.05-0.17) AND equal, to 1e-8
    relative, the eigenvalues the CPU oracle found at full size (tests/golden/c5_full_oracle_eigs.json)"""
    bc = _bc()
    lam, Q, res, info = bc.c5_device(na, 1003, 999, solver="gmres")
    assert info["n"] == 1003995 and len(lam) >= 6
    assert max(res) < 1e-8
    Qh = na.to_host(Q) if not isinstance(Q, np.ndarray) else Q
    hres = bc.c5_host_residuals(1003, 999, lam, Qh)
    assert max(hres) < 1e-8, hres
    assert max(abs(a - b) for a, b in zip(res, hres)) < 1e-9, (res, hres)      # device K1 and host operator agree
    lt, Qt, rest, it = bc.c5_device(na, 303, 299, solver="lu")
    assert len(lt) >= 6 and max(rest) < 1e-8
    lo, Qo, _ = bc.c5_oracle_twin(303, 299)
    assert len(lo) == len(lt), (lo, lt)
    ok, worst = bc.match(lt, lo, 1e-8)
    assert ok, worst
    for l in lam:
        assert np.min(abs(np.asarray(lt) - l)) < 0.25, (l, lt)
    # rules (i) and (iii) at FULL size: the CPU oracle's run of the same call by the reference's own route (matrix-free Schur
    # complement + Sylvester-SMW preconditioned GMRES, oracle/wep_linsolvers.py; one 757 s run on the GPU box's host,
    # scripts/c5_oracle_full.py, record in profiles/r4_c5_oracle_full.json) found these eigenvalues
    import json
    import os
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "c5_full_oracle_eigs.json")) as f:
        gold = [complex(a, b) for a, b in json.load(f)["eigenvalues"]]
    assert len(lam) == len(gold), (lam, gold)
    ok, worst = bc.match(lam, gold, 1e-8)
    assert ok, worst


def test_c2_basis_needs_no_full_zero_fill(na, monkeypatch):
    """nep_iar_run clears only a slack of rows behind every basis column's active part (the Gram-Schmidt kernels mask at tile
    granularity) instead of the whole 1.6 GB block.  With the block poisoned by NaN patterns first (NEP_IAR_POISON) the run returns
    bit for bit what it returns after a full zero fill (NEP_IAR_FULL_ZERO): no kernel of the pipeline reads a row that no step wrote"""
    nep = na.nep_gallery("gun_spmf_scaled"); n = nep.n
    out = {}
    from nep_amd.linsolvers import _DeviceRefactor
    na.iar(nep, sigma=0.0, gamma=1.0, maxit=100, neigs=np.inf, v=np.ones(n), tol=1e-10)
    _DeviceRefactor.wait()            # (the device-LU plan exists from here on: both runs below take the same factorisation route ...)
    na.iar(nep, sigma=0.0, gamma=1.0, maxit=100, neigs=np.inf, v=np.ones(n), tol=1e-10)      # (... and the refinement count has settled)
    for mode in ("NEP_IAR_FULL_ZERO", "NEP_IAR_POISON"):
        monkeypatch.setenv(mode, "1")
        r0 = na.iar.native_runs
        hist = []
        lam, Q, _ = na.iar(nep, sigma=0.0, gamma=1.0, maxit=100, neigs=np.inf, v=np.ones(n), tol=1e-10, errhist=hist)
        assert na.iar.native_runs == r0 + 1
        monkeypatch.delenv(mode)
        out[mode] = (lam, Q, np.concatenate(hist))
    a, b = out["NEP_IAR_FULL_ZERO"], out["NEP_IAR_POISON"]
    assert np.all(np.isfinite(b[2])) and len(a[0]) == 46 and len(b[0]) == 46
    assert np.array_equal(a[2], b[2]), float(np.max(np.abs(a[2] - b[2]) / a[2]))
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


def test_c2_repeated_runs_are_stable(na):
    """config C2 ten times in a row (host LU for the first call, device numeric LU once the pattern's plan exists, checks on
    their own stream next to a recurrence that runs far ahead of the device): every run returns the same eigenpairs.  Guards
    the cross-stream buffer hazards this pipeline is exposed to (a scratch block changing hands while kernels enqueued with it
    were pending produced orthogonalisation 'breakdowns' in 2-6 of 8 runs before it was fixed)."""
    from nep_amd.linsolvers import _DeviceRefactor
    nep = na.nep_gallery("gun_spmf_scaled")
    ref = None
    used_device_lu = 0
    for rep in range(10):
        creator = na.FactorizeLinSolverCreator(max_factorizations=0)
        lam, Q, _ = na.iar(nep, sigma=0.0, gamma=1.0, maxit=100, neigs=np.inf, v=np.ones(nep.n), tol=1e-10, linsolvercreator=creator)
        if rep == 0:
            _DeviceRefactor.wait()
            ref = np.sort_complex(lam)
            assert len(ref) >= 40
        else:
            assert len(lam) == len(ref)
            assert np.abs(np.sort_complex(lam) - ref).max() <= 1e-9 * np.abs(ref).max()
    plans = [p for p in _DeviceRefactor.plans.values() if p["state"] == "ready"]
    assert plans and sum(p["uses"] for p in plans) >= 8        # the later runs were factorised on the device


def test_c2_device_memory_plateaus(na):
    """device memory in use does not grow from call to call of the headline configuration (it did by 9 MB per call: the
    library's thread-local scratch of iar's per-call checker thread had no destructor, and a fresh check stream per call
    made torch's caching allocator build one cache per stream)"""
    import torch
    nep = na.nep_gallery("gun_spmf_scaled"); nep.dev

    def used():
        torch.cuda.synchronize()
        free, total = torch.cuda.mem_get_info()
        return (total - free) / 2 ** 20
    marks = []
    for i in range(36):
        lam = na.iar(nep, maxit=100, neigs=np.inf, v=np.ones(nep.n), tol=1e-10)[0]
        assert len(lam) == 46
        if i in (11, 35):
            marks.append(used())
    assert marks[1] - marks[0] < 48.0, marks


def test_bench_plain_run_times_the_steps_and_dumps_the_last_one(na, tmp_path):
    """`bench.py --gpus 1 --steps 3 --warmup 1 --dump-outputs DIR`, no --full: ONE JSON line with the headline fields and none of
    the extras, `ms_per_step` = the time of one of the 3 timed steps, and in DIR the eigenpairs the last timed step returned (config
    C2: 46 pairs, host FP64 backward errors below the tolerance)"""
    import json
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
                        "--dump-outputs", str(tmp_path)], cwd=root, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    d = json.loads(lines[0])
    assert d["steps"] == 3 and d["unit"] == "eigenpairs/s" and d["higher_is_better"] is True and d["ms_per_step"] > 0
    assert abs(d["value"] * d["ms_per_step"] * 1e-3 - d["config"]["eigenpairs_per_step"]) < 1e-9 * d["value"]
    # what really ran: the calls counted by nep_iar_run inside the timed loop, and the warm-up calls timed one by one
    assert ": 3 of the 3 timed steps took it" in d["driver"], d["driver"]
    assert len(d["warmup_calls_ms"]) == 1
    assert not any(k in d for k in ("roofline", "cpu_baseline", "beyn_sharded", "c5_wep", "ms_per_step_host_lu"))
    e = np.load(tmp_path / "eigenvalues.npy")
    q = np.load(tmp_path / "eigenvectors.npy")
    assert e.dtype == np.float64 and q.dtype == np.float64
    lam = e[:, 0] + 1j * e[:, 1]
    Q = q[..., 0] + 1j * q[..., 1]
    nep = na.nep_gallery("gun_spmf_scaled")
    assert len(lam) == d["config"]["eigenpairs_per_step"] == 46 and Q.shape == (nep.n, 46)
    errs = _bc().host_backward_errors(nep.get_Av(), nep.get_fv(), lam, Q)
    assert max(errs) < 1e-10
