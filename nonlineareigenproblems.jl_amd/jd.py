"""Jacobi-Davidson on the device backend: jd_betcke (Betcke/Voss variant, keyword surface of src/method_jd.jl:52-66) and
jd_effenberger (deflation based, :216-438).

Per iteration (method_jd.jl:122-168): the projected NEP W^H M(lam) V gains one row and column
(`expand_projectmatrices`, K1 + nep_gemv_h), the inner solver returns its eigenpairs, u = V s (K7), the error measure
(K2), then the expansion v = M(lam)^{-1} M'(lam) u with a NEW host factorisation of M(lam) (K1 + K5), orthogonalised
against V (K6); with the Petrov-Galerkin projection the test space gains w = M(lam) u (K1 + K6).

jd_effenberger computes the pairs one after the other: each converged pair is deflated (deflation.deflate_eigpair, mode "SPMF")
and the iteration restarts on the deflated NEP of size n + p with a fresh basis.  Its linear solves go through
DeflatedNEPLinSolver: one solve with the ORIGINAL matrix M(lam) -- whose sparsity pattern, and so the device refactorisation
plan, is the same at every iteration and every deflation level -- and one border pass (nep_defl_border).
"""
import numpy as np
import torch

from . import dense
from .errmeasure import DefaultErrmeasure, estimate_error
from .exceptions import NoConvergenceException
from .deflation import deflate_eigpair, get_deflated_eigpairs, verify_deflate_mode
from .linsolvers import DefaultLinSolverCreator, DeflatedNEPLinSolverCreator, create_linsolver
from .nep import CDT, to_dev, to_host
from .projection import DefaultInnerSolver, SGIterInnerSolver, create_proj_NEP, inner_solve

EPS = np.finfo(float).eps


def jd_eig_sorter(lamv, V, N, target):
    """method_jd.jl:177-183: the N-th closest Ritz value to the target (N = converged + 1)"""
    lamv = np.asarray(lamv, dtype=np.complex128).reshape(-1)
    NN = min(N, len(lamv))
    c = np.argsort(np.abs(lamv - target), kind="stable")
    return lamv[c[NN - 1]], np.asarray(V)[:, c[NN - 1]].astype(np.complex128)


def jd_betcke(nep, maxit=100, neigs=1, projtype="PetrovGalerkin", inner_solver_method=None, orthmethod=dense.DGKS,
              errmeasure=None, linsolvercreator=None, tol=EPS * 100, lam=0.0, v=None, target=0.0, logger=0, inner_logger=0):
    n = nep.size(1)
    if maxit > n:
        raise ValueError("maxit = %d is larger than size of NEP = %d." % (maxit, n))
    if projtype not in ("Galerkin", "PetrovGalerkin"):
        raise ValueError("Only accepted values of 'projtype' are :Galerkin and :PetrovGalerkin.")
    if projtype != "Galerkin" and isinstance(inner_solver_method, SGIterInnerSolver):
        raise ValueError("Need to use 'projtype' :Galerkin in order to use SGITER as inner solver.")
    if inner_solver_method is None:
        inner_solver_method = DefaultInnerSolver()
    if errmeasure is None:
        errmeasure = DefaultErrmeasure(nep)
    if linsolvercreator is None:
        linsolvercreator = DefaultLinSolverCreator()
    if v is None:
        v = np.random.randn(n)
    lam = complex(lam); target = complex(target)
    lam_vec = np.zeros(neigs, dtype=np.complex128)
    u_vec = np.zeros((n, neigs), dtype=np.complex128)
    v0 = np.asarray(v, dtype=np.complex128)
    u = to_dev(v0 / np.linalg.norm(v0))[0].clone()
    conveig = 0
    err = estimate_error(errmeasure, lam, u)
    if err < tol:
        lam_vec[conveig] = lam; u_vec[:, conveig] = to_host(u.reshape(1, n))[:, 0]; conveig += 1
    if conveig == neigs:
        return lam_vec, u_vec
    proj_nep = create_proj_NEP(nep, maxit + 1)
    Vm = torch.zeros((maxit + 1, n), dtype=CDT, device="cuda")
    dense.copy(u, Vm[0], n)
    pg = projtype == "PetrovGalerkin"
    if pg:
        Wm = torch.zeros((maxit + 1, n), dtype=CDT, device="cuda")
        w0 = nep.compute_Mlincomb(lam, u.reshape(1, n))
        dense.copy(w0, Wm[0], n); dense.scal(Wm[0], 1.0 / dense.nrm2(Wm[0]), n)
    else:
        Wm = Vm
    one = np.ones(1)
    for k in range(1, maxit + 1):
        V = Vm[:k]; W = Wm[:k]
        proj_nep.expand_projectmatrices(W, V)
        lamv, sv = inner_solve(inner_solver_method, proj_nep, lamv=lam * np.ones(conveig + 1, dtype=complex), sigma=target,
                               neigs=conveig + 1)
        if len(np.atleast_1d(lamv)) == 0:
            raise NoConvergenceException(lam_vec[:conveig], u_vec[:, :conveig], err, "the inner solver returned no eigenpair")
        lam, s = jd_eig_sorter(lamv, np.asarray(sv).reshape(k, -1), conveig + 1, target)
        s = s / np.linalg.norm(s)
        u = dense.gemm_ts(V, s.reshape(k, 1), k=k, rows=n, ldz=n)[0]
        err = estimate_error(errmeasure, lam, u)
        if err < tol and (conveig == 0 or np.all(np.abs(lam - lam_vec[:conveig]) / np.abs(lam_vec[:conveig]) > np.sqrt(np.sqrt(EPS)))):
            lam_vec[conveig] = lam; u_vec[:, conveig] = to_host(u.reshape(1, n))[:, 0]; conveig += 1
        if conveig == neigs:
            return lam_vec, u_vec
        pk = nep.compute_Mlincomb(lam, u.reshape(1, n), one, 1)                   # M'(lam) u
        linsolver = create_linsolver(linsolvercreator, nep, lam)
        vnew = Vm[k]
        linsolver.solve_dev(pk, out=vnew.reshape(1, n))
        dense.orthogonalize_and_normalize(Vm, vnew, k, rows=n, ldv=n, method=orthmethod)
        if pg:
            wnew = Wm[k]
            dense.copy(nep.compute_Mlincomb(lam, u.reshape(1, n)), wnew, n)
            dense.orthogonalize_and_normalize(Wm, wnew, k, rows=n, ldv=n, method=orthmethod)
    msg = "Number of iterations exceeded. maxit=%d and only %d eigenvalues converged out of %d." % (maxit, conveig, neigs)
    raise NoConvergenceException(np.concatenate([lam_vec[:conveig], [lam]]),
                                 np.column_stack([u_vec[:, :conveig], to_host(u.reshape(1, n))[:, 0]]), err, msg)


def jd_effenberger(nep, maxit=100, neigs=1, inner_solver_method=None, orthmethod=dense.DGKS, linsolvercreator=None,
                   tol=EPS * 100, lam=None, v=None, target=0.0, deflation_mode="Auto", logger=0, inner_logger=0):
    """src/method_jd.jl:216-295: Jacobi-Davidson with Effenberger deflation.  Repeated eigenvalues are avoided by deflating
    every converged pair and restarting on the deflated NEP; `maxit` is the iteration budget over all levels.  Returns
    get_deflated_eigpairs of the last deflated NEP: (eigenvalues, n x neigs eigenvectors of `nep`).  Raises
    NoConvergenceException (holding the pairs found so far and the current iterate) when the budget runs out.

    Difference from the reference: the projected NEP of this backend needs an AbstractSPMF, so a `deflation_mode` that does
    not resolve to "SPMF" is refused up front (the reference fails with a MethodError after the first pair).  SGIterInnerSolver
    is refused as there (:239-241): a deflated problem has no min-max characterisation."""
    n = nep.size(1)
    if maxit > n:
        raise ValueError("maxit = %d is larger than size of NEP = %d." % (maxit, n))
    if isinstance(inner_solver_method, SGIterInnerSolver):
        raise ValueError("Inner solver 'SGIterInnerSolver' not accepted since deflated problem not min-max.")
    if verify_deflate_mode(nep, deflation_mode) != "SPMF":
        raise ValueError("jd_effenberger projects the deflated NEP, which needs deflation_mode \"SPMF\" (an AbstractSPMF)")
    if inner_solver_method is None:
        inner_solver_method = DefaultInnerSolver()
    if linsolvercreator is None:
        linsolvercreator = DefaultLinSolverCreator()
    lam = complex(np.random.rand() if lam is None else lam)
    target = complex(target)
    u = np.asarray(np.random.rand(n) if v is None else v, dtype=np.complex128).reshape(-1)
    u = u / np.linalg.norm(u)
    args = (maxit, inner_solver_method, orthmethod, tol, target, neigs)
    conveig = 0
    its = 0
    # initial check for convergence: a start that is good enough is deflated at once
    err = np.linalg.norm(nep.compute_Mlincomb(lam, u.reshape(n, 1)))
    if err < tol:
        lam_init = complex(np.random.rand()); u_init = np.random.rand(n + 1).astype(np.complex128)
    else:
        lam, u, its, u_init, lam_init = _jd_effenberger_inner(nep, nep, None, None, its, conveig, linsolvercreator, u, lam, *args)
    conveig += 1
    deflated_nep = deflate_eigpair(nep, lam, u, mode=deflation_mode)
    while True:                                  # left on convergence (return) or when the iterations run out (exception)
        if conveig == neigs:
            return get_deflated_eigpairs(deflated_nep)
        lam, u, its, u_init, lam_init = _jd_effenberger_inner(deflated_nep, nep, deflated_nep.V0, deflated_nep.S0, its, conveig,
                                                              DeflatedNEPLinSolverCreator(linsolvercreator), u_init, lam_init, *args)
        conveig += 1                             # minimality index 1: the pair grows by one
        deflated_nep = deflate_eigpair(deflated_nep, lam, u)


def _jd_effenberger_inner(target_nep, orgnep, X, Lam, nrof_its, conveig, linsolvercreator, u0, lam, maxit, inner_solver_method,
                          orthmethod, tol, target, neigs):
    """src/method_jd.jl:320-438: one level of deflation.  target_nep is the plain NEP (X = Lam = None) or a deflated NEP with the
    invariant pair (Lam, X).  Returns (lam, u (host), iterations used so far, continuation vector (host), continuation value).
    Bases, iterate, residual and Newton step are device vectors; only k x k matrices and scalars are on the host."""
    n = orgnep.size(1)
    m = 0 if Lam is None else Lam.shape[0]
    nn = n + m
    size = maxit + 1 - nrof_its
    u = to_dev(np.asarray(u0, dtype=np.complex128) / np.linalg.norm(u0))[0].clone()
    newton_step = to_dev(np.random.rand(nn))[0]
    proj_nep = create_proj_NEP(target_nep, size)
    Vm = torch.zeros((size, nn), dtype=CDT, device="cuda")
    Wm = torch.zeros((size, nn), dtype=CDT, device="cuda")
    dense.copy(u, Vm[0], nn)
    dense.copy(target_nep.compute_Mlincomb(lam, u.reshape(1, nn)), Wm[0], nn)
    dense.scal(Wm[0], 1.0 / dense.nrm2(Wm[0]), nn)
    one = np.ones(1)
    err = np.inf
    for loop_counter in range(nrof_its + 1, maxit + 1):
        k = loop_counter - nrof_its                       # the index on THIS level of deflation
        V = Vm[:k]; W = Wm[:k]
        proj_nep.expand_projectmatrices(W, V)
        lamv, sv = inner_solve(inner_solver_method, proj_nep, lamv=lam * np.ones(2, dtype=complex), sigma=target, neigs=2,
                               tol=tol / 10)
        lamv = np.atleast_1d(np.asarray(lamv, dtype=np.complex128)); sv = np.asarray(sv, dtype=np.complex128).reshape(k, -1)
        accept = False
        if len(lamv) > 0:
            lam_temp, s = jd_eig_sorter(lamv, sv, 1, target)              # always the closest to the target: the rest is deflated
            if np.isfinite(lam_temp) and np.all(np.isfinite(s)) and np.linalg.norm(s) > 0:
                s = s / np.linalg.norm(s)
                accept = np.linalg.norm(proj_nep.compute_Mlincomb(lam_temp, s.reshape(k, 1))) < tol * 50
        if accept:                                        # a solution of the projected problem: the Ritz pair
            u = dense.gemm_ts(V, s.reshape(k, 1), k=k, rows=nn, ldz=nn)[0]
            lam = complex(lam_temp)
        else:                                             # otherwise the "Newton step" (not exactly Effenberger's, but similar)
            dense.axpy(1.0, newton_step, u, nn)
            dense.scal(u, 1.0 / dense.nrm2(u), nn)
        rk = target_nep.compute_Mlincomb(lam, u.reshape(1, nn))
        err = dense.nrm2(rk)                              # (3.2) in Effenberger
        if err < tol:
            uh = to_host(u.reshape(1, nn))[:, 0]
            lam2 = None
            if len(lamv) > 1:
                lam2, s2 = jd_eig_sorter(lamv, sv, 2, target)
                if not abs(lam - lam2) / abs(lam) > np.sqrt(EPS):
                    lam2 = None
            if lam2 is not None:                          # a light continuation: the second Ritz pair starts the next level
                s2 = s2 / np.linalg.norm(s2)
                u2 = np.concatenate([to_host(dense.gemm_ts(V, s2.reshape(k, 1), k=k, rows=nn, ldz=nn))[:, 0], [0.0]])
            else:
                lam2 = complex(np.random.rand()); u2 = np.random.rand(nn + 1).astype(np.complex128)
            return lam, uh, loop_counter, u2, complex(lam2)
        # extend the bases: v = Mt(lam)^-1 Mt'(lam) u (top of page 367 of Betcke and Voss), w = the residual
        pk = target_nep.compute_Mlincomb(lam, u.reshape(1, nn), one, 1)
        linsolver = create_linsolver(linsolvercreator, target_nep, lam)
        vnew = Vm[k]
        linsolver.solve_dev(pk.reshape(1, nn), out=vnew.reshape(1, nn))
        newton_step = vnew.clone()
        dense.orthogonalize_and_normalize(Vm, vnew, k, rows=nn, ldv=nn, method=orthmethod)
        wnew = Wm[k]
        dense.copy(rk, wnew, nn)
        dense.orthogonalize_and_normalize(Wm, wnew, k, rows=nn, ldv=nn, method=orthmethod)
    msg = "Number of iterations exceeded. maxit=%d and only %d eigenvalues converged out of %d." % (maxit, conveig, neigs)
    uh = to_host(u.reshape(1, nn))[:, 0]
    if m > 0:                                             # the eigenpairs held in the invariant pair, and the current iterate
        D, Y = np.linalg.eig(Lam)
        raise NoConvergenceException(np.concatenate([D, [lam]]), np.column_stack([X @ Y, uh[:n]]), err, msg)
    raise NoConvergenceException(np.array([lam]), uh[:n].reshape(n, 1), err, msg)
