"""The routes of the waveguide linear solvers (nep_amd/wep_linsolvers.py) are fixed when an object is built: the preconditioner's
three-transform form exactly where nep_wep_plan has one, the piecewise form elsewhere, and -- on a WEP without a P^{-1} plan, which
grids below nz = 1921 reach only when the cached plan is set to "none" -- the column-by-column SMW matrix, the dense-R form of
P^{-1} and the assembled SchurMatVec, each against the normal instance on the same grid."""
import ctypes as C
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
LAM = -1.3 - 0.7j
PLAN_SMW = 2


@pytest.fixture(scope="module")
def na():
    import nep_amd
    if nep_amd.device_count() < 1:
        pytest.skip("no GPU")
    return nep_amd


def _apply(na, P, v):
    import torch
    r = na.to_dev(v)[0].clone()
    P(r); torch.cuda.synchronize()
    return na.to_host(r.reshape(1, -1))[:, 0]


def _rand(seed, n):
    rng = np.random.default_rng(seed)
    return rng.standard_normal(n) + 1j * rng.standard_normal(n)


@pytest.mark.parametrize("nz,N,three", [(15, 5, True), (7, 7, False), (25, 5, False)])
def test_preconditioner_route_is_fixed_at_setup(na, nz, N, three):
    """nz = 15 = 3 * 5 has the three-transform form; nz = 7 (prime, N2 = 1) and nz = 25 (no coprime factors) have a P^{-1} plan but
    not that form.  P._fused says what nep_wep_plan says, from construction on and whatever is applied; on nz = 15 the two forms
    agree to 1e-12"""
    nx = nz + 4
    nep = na.nep_gallery("WEP", nx=nx, nz=nz, benchmark_problem="JARLEBRING")
    info = (C.c_int64 * 8)()
    planned = na._lib.lib.nep_wep_plan(nz, nx, PLAN_SMW, info) == 0
    assert planned is three and nep._pinv_plan() is not None
    P = na.wep_generate_preconditioner(nep, N, LAM)
    assert P._fused is planned
    v = _rand(nz + N, nx * nz)
    a = _apply(na, P, v)
    assert np.array_equal(_apply(na, P, v), a)
    assert P._fused is planned
    if three:
        os.environ["NEP_WEP_SMW_FUSED"] = "0"
        try:
            P0 = na.wep_generate_preconditioner(nep, N, LAM)
        finally:
            del os.environ["NEP_WEP_SMW_FUSED"]
        assert P0._fused is False
        b = _apply(na, P0, v)
        rel = np.linalg.norm(a - b) / np.linalg.norm(b)
        print("three-transform against piecewise: %.3g" % rel)
        assert rel <= 1e-12 and P0._fused is False


def test_routes_without_a_pinv_plan(na):
    """nx = 19, nz = 15, N = 5 with the WEP's cached P^{-1} plan set to "none": assembled SchurMatVec (K1 + dense-R P^{-1} through
    nep_gemv_hd + C1), the SMW matrix column by column, the piecewise apply and the hipGraph-captured GMRES step, against the
    instance with a plan: SchurMatVec 1e-13, SMW matrix and P(r) 1e-12; lin_solve == M(lam)^{-1} to 1e-11.

    The TAUSCH waveguide at the shift of test_wep_linsolvers_small: there GMRES(20) with the 5 x 9 region preconditioner needs 13
    iterations.  (On the JARLEBRING waveguide regions of 3 grid rows do not resolve the wavenumber on this grid and GMRES(20)
    stagnates at a residual of 1.5 after 285 iterations -- with a P^{-1} plan just the same, so that says nothing about the
    route.)  Left-preconditioned GMRES controls the preconditioned residual (5.6e-12 true residual at reltol 1e-12 here), so
    the solve runs with the refinement sweeps of the solver, as tiar's does."""
    import torch
    from oracle import wep as ow
    wl = na.wep_linsolvers
    nx, nz, N = 19, 15, 5
    LAM = -1.3 - 0.31j
    nep = na.nep_gallery("WEP", nx=nx, nz=nz, benchmark_problem="TAUSCH")
    nep0 = na.nep_gallery("WEP", nx=nx, nz=nz, benchmark_problem="TAUSCH")
    nep0._pinv_h = None                                          # what nz >= 1921 gives: no P^{-1} plan
    ops, ops0 = wl.SchurOps(nep, LAM), wl.SchurOps(nep0, LAM)
    assert ops.stencil is not None and ops0.stencil is None and nep0._pinv_plan() is None
    v = _rand(1, nx * nz)
    vd = na.to_dev(v)[0]
    o1 = torch.empty_like(vd); o0 = torch.empty_like(vd)
    ops.matvec(vd, o1); ops0.matvec(vd, o0); torch.cuda.synchronize()
    a, b = na.to_host(o1.reshape(1, -1))[:, 0], na.to_host(o0.reshape(1, -1))[:, 0]
    rel = np.linalg.norm(b - a) / np.linalg.norm(a)
    print("SchurMatVec without a plan: %.3g" % rel)
    assert rel <= 1e-13
    P, P0 = na.wep_generate_preconditioner(nep, N, LAM), na.wep_generate_preconditioner(nep0, N, LAM)
    assert not P0._fused
    relM = np.linalg.norm(P0._M - P._M) / np.linalg.norm(P._M)
    pa, pb = _apply(na, P, v), _apply(na, P0, v)
    relP = np.linalg.norm(pb - pa) / np.linalg.norm(pa)
    print("SMW matrix without a plan: %.3g, P(r): %.3g" % (relM, relP))
    assert relM <= 1e-12 and relP <= 1e-12 and not P0._fused
    x = _rand(2, nep0.n)
    cr = na.WEPLinSolverCreator(solver_type="gmres", kwargs=(("Pl", P0), ("reltol", 1e-12)), refinements=10)
    solver = na.create_linsolver(cr, nep0, LAM)
    assert solver._graph is not None, getattr(solver, "_graph_error", None)      # the piecewise step runs as a captured graph
    y = na.lin_solve(solver, x)
    M = ow.WEP_FD(nx, nz, "TAUSCH").compute_Mder(LAM)
    res = np.linalg.norm(M @ y - x) / np.linalg.norm(x)
    print("lin_solve without a plan: %.3g, GMRES iterations %s" % (res, solver.iterations))
    assert res <= 1e-11 and 0 < max(solver.iterations) < solver.gmres.restart       # no solve needed a restart
