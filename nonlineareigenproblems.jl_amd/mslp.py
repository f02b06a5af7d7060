"""mslp: the method of successive linear problems (A. Ruhe, Algorithms for the nonlinear eigenvalue problem, SIAM J. Numer.
Anal. 10 (1973)), src/method_mslp.jl:38-87.

Every iteration solves the linear eigenvalue problem M(lam) v = d M'(lam) v for the eigenvalue d nearest zero and sets
lam <- lam - d.  For a pure sparse SPMF NEP with the default (or the Arnoldi) eigensolver the pencil never leaves the device:
ArnoldiEigSolver.from_nep works on the NEP's own stacked CSR with the coefficient rows f_t(lam), f_t'(lam), factorises
-M(lam) on the pattern's stored pivot sequence once the pattern has a plan, and hands the eigenvector to estimate_error as a
device tensor; the previous eigenvector is the start vector of the next Krylov-Schur run.  Every other case -- dense NEPs, NEPs
that are no SPMF (deflated problems), user-defined solver types -- builds eigsolvertype(M(lam), M'(lam)) as the reference does.
"""
import time

import numpy as np

from . import dense
from .eigsolvers import ArnoldiEigSolver, DefaultEigSolver, eig_solve
from .errmeasure import DefaultErrmeasure, Errmeasure, estimate_error
from .exceptions import NoConvergenceException
from .nep import to_host

EPS = np.finfo(float).eps


def mslp(nep, errmeasure=None, tol=EPS * 100, maxit=100, lam=0, logger=0, eigsolvertype=DefaultEigSolver, hist=None):
    """(lam, v) with estimate_error(errmeasure, lam, v) < tol.  hist (a list) receives one dict per iteration: k, err, lam, d,
    route ("device" or "host") and, on the device route, the eigensolver's info (steps, restarts, factorization, wall)."""
    n = nep.size(1)
    lam = complex(lam)
    if errmeasure is None:
        errmeasure = DefaultErrmeasure(nep)
    device_route = eigsolvertype in (DefaultEigSolver, ArnoldiEigSolver) and ArnoldiEigSolver.accepts(nep)
    vd = None
    v = np.zeros(n, dtype=np.complex128)
    err = np.inf
    for k in range(1, maxit + 1):
        t0 = time.perf_counter()
        if device_route:
            solver = ArnoldiEigSolver.from_nep(nep, lam)
            d, X = solver.eig_solve_dev(target=0, nev=1, v0=vd)
            vd = X[0]
            dense.scal(vd, 1.0 / dense.nrm2(vd))
            d = complex(d[0])
            lam -= d
            user_fn = callable(errmeasure) and not isinstance(errmeasure, Errmeasure)      # a function sees a host vector
            err = estimate_error(errmeasure, lam, to_host(vd.reshape(1, n))[:, 0] if user_fn else vd)
            rec = dict(k=k, err=err, lam=lam, d=d, route="device", wall=time.perf_counter() - t0, **{
                key: solver.info[key] for key in ("steps", "restarts", "factorization", "breakdown")})
        else:
            solver = eigsolvertype(nep.compute_Mder(lam, 0), nep.compute_Mder(lam, 1))
            d, X = eig_solve(solver, target=0, nev=1)
            d = complex(np.asarray(d).reshape(-1)[0])
            v = np.asarray(X, dtype=np.complex128).reshape(n, -1)[:, 0]
            lam -= d
            v = v / np.linalg.norm(v)
            err = estimate_error(errmeasure, lam, v)
            rec = dict(k=k, err=err, lam=lam, d=d, route="host", wall=time.perf_counter() - t0)
        if hist is not None:
            hist.append(rec)
        if logger:
            print("mslp iteration %d: err = %.3e, lam = %r" % (k, err, lam))
        if err < tol:
            return lam, (to_host(vd.reshape(1, n))[:, 0] if device_route else v)
    raise NoConvergenceException(lam, to_host(vd.reshape(1, n))[:, 0] if vd is not None else v, err,
                                 "Number of iterations exceeded. maxit=%d." % maxit)
