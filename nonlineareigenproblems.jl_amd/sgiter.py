"""sgiter: safeguarded iteration for the j-th eigenvalue of a Hermitian NEP with min-max numbering (src/method_sgiter.jl:33-115;
V. Mehrmann and H. Voss, Nonlinear eigenvalue problems: a challenge for modern eigenvalue methods, GAMM-Mitteilungen 27 (2004)).

Every iteration takes the eigenvector of the j-th smallest eigenvalue of the Hermitian matrix M(lam_k) and solves the Rayleigh
functional v^H M(lam) v = 0 for the next lam.  Two routes for the eigen step:

  host    dense NEPs, projected NEPs, any explicit eigsolvertype: eigsolvertype(compute_Mder(nep, lam)), eig_solve(nev=n), sorted
          by real part, column j -- the reference's semantics.
  device  the default eigsolvertype on a pure sparse SPMF: one augmented handle with the terms [A_1..A_m, I] is built per call;
          per iteration the pencil (M(lam_k), I) is the two coefficient rows cA = [f_t(lam_k).., 0], cB = [0.., 1] of
          ArnoldiEigSolver.from_terms, so C = tau I - M(lam_k) is factorised from term coefficients on the one pattern and
          nothing is assembled.  tau lies below the spectrum (a Gershgorin bound from the aligned term block, or
          eig_lower_bound), so the j dominant eigenvalues of C^-1 are the j algebraically smallest of M(lam_k).  The vector stays
          on the device for the Rayleigh functional (one pass of K14, nep_spmf_biforms, then a scalar solve on the host) and
          the error measure.
"""
import numpy as np
import scipy.sparse as sp

from . import dense, funcs
from .eigsolvers import ArnoldiEigSolver, DefaultEigSolver, EigenEigSolver, KS_MAXDIM, eig_solve
from .errmeasure import DefaultErrmeasure, Errmeasure, estimate_error
from .exceptions import NoConvergenceException
from .nep import AbstractSPMF, PEP, SPMF_NEP, to_host
from .newton import ScalarNewtonInnerSolver, compute_rf, rf_forms_ok

EPS = np.finfo(float).eps
HOST_EIG_MAX = 2000          # largest sparse problem whose eigen step may fall back to the dense host solver


def check_arguments(n, j, lam_min, lam_max, lam):
    """the four argument checks of method_sgiter.jl:50-65 (with no interval given every NaN comparison is false, as there)"""
    if j > n or j <= 0:
        raise ValueError("j must be a number between 1 and size(nep) = %d. You have selected j = %d." % (n, j))
    if not ((np.isnan(lam_min) and np.isnan(lam_max)) or (not np.isnan(lam_min) and not np.isnan(lam_max))):
        raise ValueError("A proper interval is not chosen.")
    if lam_max < lam_min:
        raise ValueError("The interval cannot be empty, λ_max >= λ_min is required. Supplied interval [λ_min,λ_max] = [%r,%r]."
                         % (lam_min, lam_max))
    if lam < lam_min or lam > lam_max:
        raise ValueError("The starting guess is outside the interval.")


def choose_correct_eigenvalue_from_rf(lam_vec, lam_min, lam_max):
    """method_sgiter.jl:101-115: without an interval the minimum, with one the single value inside it"""
    lam_vec = np.real(np.atleast_1d(lam_vec)).astype(float)
    if np.isnan(lam_min) and np.isnan(lam_max):
        return float(lam_vec.min())
    inside = (lam_vec <= lam_max) & (lam_vec >= lam_min)
    if inside.sum() > 1:
        raise ValueError("Multiple values of λ found in the interval.")
    if inside.sum() == 0:
        raise ValueError("No λ found in the prescribed interval.")
    return float(lam_vec[np.flatnonzero(inside)[0]])


def gershgorin_shift(indptr, indices, vals, n, lower=None):
    """tau = g - 0.01 max(|g|, ||M||_inf) for the Hermitian matrix with the CSC arrays (indptr, indices, vals):
    g = min_i (Re a_ii - sum_{j != i} |a_ij|) bounds the spectrum from below (`lower` replaces g when given)"""
    col = np.repeat(np.arange(n), np.diff(indptr))
    diag = np.asarray(indices) == col
    av = np.abs(vals)
    norm_inf = float(np.bincount(col, weights=av, minlength=n).max()) if len(av) else 0.0
    if lower is None:
        d = np.bincount(col[diag], weights=np.real(vals[diag]), minlength=n)
        r = np.bincount(col[~diag], weights=av[~diag], minlength=n)
        lower = float((d - r).min())
    lower = float(lower)
    return lower - 0.01 * max(abs(lower), norm_inf)


def _jth_eigenvector_host(solver, n, j):
    """compute_jth_eigenvector, method_sgiter.jl:89-98"""
    D, V = eig_solve(solver, nev=n)
    V = np.asarray(V, dtype=np.complex128).reshape(n, -1)
    x = V[:, np.argsort(np.real(D), kind="stable")[j - 1]] if n > 1 else V[:, 0]
    return x / np.linalg.norm(x)


def sgiter(nep, j, lam_min=np.nan, lam_max=np.nan, lam=0.0, errmeasure=None, tol=100 * EPS, maxit=100, inner_solver=None,
           logger=0, eigsolvertype=DefaultEigSolver, eig_lower_bound=None, hist=None):
    """(lam, v): the j-th eigenvalue (1-based, min-max numbering) of the Hermitian NEP and a unit eigenvector.  With an interval
    [lam_min, lam_max] the Rayleigh functional is assumed unique on it; without one the minimum solution is taken.
    eig_lower_bound (device route): a number, or a function of lam, known to lie at or below the spectrum of M(lam); it replaces
    the Gershgorin bound.  hist (a list) receives one dict per iteration: k, err, lam, route and, on the device route, tau and
    the eigensolver's steps, restarts, factorization and device_factorized."""
    from .projection import InnerSolver, PolyeigInnerSolver, Proj_SPMF_NEP
    if isinstance(nep, Proj_SPMF_NEP):                  # the small dense SPMF of the projection
        nep = nep.nep_proj
    n = nep.size(1)
    j = int(j)
    lam_min, lam_max, lam = float(lam_min), float(lam_max), float(np.real(lam))
    check_arguments(n, j, lam_min, lam_max, lam)
    if errmeasure is None:
        errmeasure = DefaultErrmeasure(nep)
    if inner_solver is None:
        inner_solver = PolyeigInnerSolver() if isinstance(nep, PEP) else ScalarNewtonInnerSolver(tol=tol / 10)
    rf_kw = {}
    if isinstance(inner_solver, ScalarNewtonInnerSolver):
        rf_kw["forms"] = rf_forms_ok(nep)
    elif isinstance(inner_solver, InnerSolver) and not isinstance(inner_solver, PolyeigInnerSolver):
        rf_kw["tol"] = tol / 10

    default_type = eigsolvertype is DefaultEigSolver
    sparse = isinstance(nep, AbstractSPMF) and nep.issparse()
    device_route = default_type and ArnoldiEigSolver.accepts(nep)
    if device_route and 2 * j > KS_MAXDIM:
        raise ValueError("sgiter: the device eigen step keeps a subspace of 2 j <= %d vectors (j = %d); "
                         "eigsolvertype=EigenEigSolver selects the host route" % (KS_MAXDIM, j))
    if default_type and sparse and not device_route and n > HOST_EIG_MAX:
        raise ValueError("sgiter: the device eigen step needs a pure sparse SPMF and the dense host eigen step is limited to "
                         "n <= %d (n = %d); an explicit eigsolvertype selects the host route" % (HOST_EIG_MAX, n))
    if device_route:
        from ._devicelu import _DeviceRefactor
        fv = nep.get_fv()
        aug = SPMF_NEP(list(nep.get_Av()) + [sp.identity(n, format="csc")], list(fv) + [funcs.one()])
        mt = len(fv)
        cB = np.zeros(mt + 1, dtype=np.complex128); cB[mt] = 1.0
        solver = ArnoldiEigSolver.from_terms(aug, np.zeros(mt + 1), cB)
        indptr, indices, D = aug._aligned_terms()
        vd = None
    elif default_type:
        eigsolvertype = EigenEigSolver                  # all n eigenvalues of a small matrix: dense LAPACK, sparse or not
    v = np.zeros(n, dtype=np.complex128)
    err = np.inf
    for k in range(1, maxit + 1):
        if device_route:
            cA = np.array([f.derivs(lam, 1)[0] for f in fv] + [0.0], dtype=np.complex128)
            lower = eig_lower_bound(lam) if callable(eig_lower_bound) else eig_lower_bound
            tau = gershgorin_shift(indptr, indices, np.einsum("ij,j->i", D, cA), n, lower)
            solver.cA = cA
            d, X = solver.eig_solve_dev(nev=j, target=tau, v0=vd)
            if k == 1:
                _DeviceRefactor.wait()                  # the pattern's plan is built behind the first factorisation: use it from now on
            vd = X[int(np.argsort(np.real(d), kind="stable")[j - 1])].clone()
            dense.scal(vd, 1.0 / dense.nrm2(vd))
            x = vd
        else:
            v = _jth_eigenvector_host(eigsolvertype(nep.compute_Mder(lam, 0)), n, j)
            x = v
        lam_vec = np.real(compute_rf(nep, x, inner_solver, **rf_kw))
        if logger >= 2:
            print("compute_rf: %r" % (lam_vec,))
        lam = choose_correct_eigenvalue_from_rf(lam_vec, lam_min, lam_max)
        user_fn = callable(errmeasure) and not isinstance(errmeasure, Errmeasure)          # a function sees a host vector
        if device_route and user_fn:
            x = to_host(vd.reshape(1, n))[:, 0]
        err = estimate_error(errmeasure, lam, x)
        if hist is not None:
            rec = dict(k=k, err=err, lam=lam, route="device" if device_route else "host")
            if device_route:
                rec.update(tau=tau, **{key: solver.info[key] for key in ("steps", "restarts", "factorization", "device_factorized")})
            hist.append(rec)
        if logger:
            print("sgiter iteration %d: err = %.3e, lam = %r" % (k, err, lam))
        if err < tol:
            return lam, (to_host(vd.reshape(1, n))[:, 0] if device_route else v)
    raise NoConvergenceException(lam, to_host(vd.reshape(1, n))[:, 0] if device_route else v, err,
                                 "Number of iterations exceeded. maxit = %d." % maxit)
