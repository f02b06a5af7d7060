"""Two-sided methods: the transposed problem `nept` next to `nep`.

The reference builds a second linear solver for nept at the same shift (src/method_rfi.jl:62-63,
src/method_infbilanczos.jl:61-62).  When nept is recognised as the transpose of nep (transpose_relation), its solver here
shares the factorisation of M(sigma): DeviceLU.transpose (nep_lu_transpose) turns the factors of M(sigma) into those of
M(sigma)^T or M(sigma)^H on the device.  Anything else gets the reference's second create_linsolver.
"""

import numpy as np
import scipy.sparse as sp

from . import dense, _lib
from ._lib import NepError, NEP_ERR_UNSUPPORTED
from .errmeasure import DefaultErrmeasure, estimate_error
from .exceptions import NoConvergenceException
from .linsolvers import (LinSolver, DeviceLU, FactorizeLinSolver, FactorizeLinSolverCreator, BackslashLinSolverCreator,
                         create_linsolver, lin_solve)
from .nep import pure_spmf, to_dev, to_host
from .newton import compute_rf, _mder_times

EPS = np.finfo(float).eps


def _same_functions(fa, fb, sigma, orders):
    """the same objects, or equal derivatives f^(d)(sigma), d < orders (hence equal Taylor coefficients up to that order)"""
    if len(fa) != len(fb):
        return False
    for f, g in zip(fa, fb):
        if f is g:
            continue
        if sigma is None:
            return False
        a = np.asarray(f.derivs(complex(sigma), orders)); b = np.asarray(g.derivs(complex(sigma), orders))
        if a.shape != b.shape or not np.array_equal(a, b):
            return False
    return True


def _equal(A, B):
    """exact entrywise equality of two matrices (sparse or dense)"""
    if A.shape != B.shape:
        return False
    if sp.issparse(A) or sp.issparse(B):
        D = sp.csr_matrix(A) - sp.csr_matrix(B)
        D.eliminate_zeros()
        return D.nnz == 0
    return np.array_equal(np.asarray(A), np.asarray(B))


def transpose_relation(nep, nept, sigma=None, orders=1):
    """"T" when nept.A_i == A_i^T for every term, "H" when nept.A_i == A_i^H (and not "T"), None otherwise.  Both must be SPMF
    problems with the same number of terms and the same functions: the same objects, or (with `sigma`) equal f^(d)(sigma) for
    d < orders.  O(nnz) host comparison, once per call."""
    if not (pure_spmf(nep, "Mlincomb") and pure_spmf(nept, "Mlincomb")):
        return None
    Av, At = nep.get_Av(), nept.get_Av()
    if len(Av) != len(At) or not _same_functions(nep.get_fv(), nept.get_fv(), sigma, orders):
        return None
    if all(_equal(A.T, B) for A, B in zip(Av, At)):
        return "T"
    if all(_equal(A.conj().T, B) for A, B in zip(Av, At)):
        return "H"
    return None


class _LUSolver(LinSolver):
    """one plain solve per lin_solve with a given DeviceLU (the shared factorisation of BackslashLinSolver's A \\ x)"""

    def __init__(self, lu):
        self.lu = lu

    def solve_dev(self, b, out=None, scale=1.0):
        return self.lu.solve(b, out=out, scale=scale)


def _conj_flag(rel, nep, sigma):
    """conj argument of nep_lu_transpose for a relation at sigma, None = no sharing.  "H": sum f_i(s) A_i^H = M(s)^H only when
    every f_i(s) is real (real_on_reals and a real shift)."""
    if rel == "T":
        return False
    if rel == "H" and complex(sigma).imag == 0 and all(f.real_on_reals() for f in nep.get_fv()):
        return True
    return None


def twosided_linsolvers(nep, nept, sigma, linsolvercreator=None, linsolvertcreator=None, rel=None, orders=1):
    """(solver of M(sigma), solver of nept's matrix at sigma, shared).  shared = True: the second one solves with the transposed
    factors of the first (one factorisation); otherwise create_linsolver(linsolvertcreator, nept, sigma) as the reference does:
    for an unrecognised nept, a creator that is not Factorize / Backslash, a refused transpose (level schedule)."""
    if linsolvercreator is None:
        linsolvercreator = FactorizeLinSolverCreator()
    if linsolvertcreator is None:
        linsolvertcreator = linsolvercreator
    if rel is None:
        rel = transpose_relation(nep, nept, sigma, orders)
    conj = _conj_flag(rel, nep, sigma)
    kinds = (FactorizeLinSolverCreator, BackslashLinSolverCreator)
    same_kind = (type(linsolvercreator) in kinds and type(linsolvertcreator) is type(linsolvercreator)
                 and not hasattr(linsolvercreator, "create_linsolver"))
    if conj is not None and same_kind:
        if isinstance(linsolvercreator, BackslashLinSolverCreator):
            lu = DeviceLU(nep.compute_Mder(sigma), permc_spec=linsolvercreator.permc_spec, expected_solves=1,
                          **linsolvercreator.lu_kw)
            ls = _LUSolver(lu)
        else:
            ls = create_linsolver(linsolvercreator, nep, sigma)
            lu = ls.lu
        try:
            lut = lu.transpose(conj)
        except NepError as e:
            if e.status != NEP_ERR_UNSUPPORTED:
                raise
            lut = None
        if lut is not None:
            if isinstance(linsolvercreator, BackslashLinSolverCreator):
                return ls, _LUSolver(lut), True
            # nept's own residual drives the refinement of its solves (its SPMF, nep_cw_backward_error)
            return ls, FactorizeLinSolver(nept, sigma, linsolvertcreator.umfpack_refinements, _lu=lut), True
        return ls, create_linsolver(linsolvertcreator, nept, sigma), False
    return (create_linsolver(linsolvercreator, nep, sigma), create_linsolver(linsolvertcreator, nept, sigma), False)


def rfi(nep, nept, errmeasure=None, tol=1000 * EPS, maxit=100, lam=0.0, v=None, u=None, linsolvercreator=None,
        inner_solver=None, logger=0, hist=None):
    """Two-sided Rayleigh functional iteration (src/method_rfi.jl:30-76; Schreiber 2008, Algorithm 4).  Returns (lam, u, v): the
    eigenvalue, the right eigenvector (of nep) and the left one (a right eigenvector of nept).  `u` / `v` are the start vectors
    of the right / left vector (random normal if omitted).  linsolvercreator defaults to BackslashLinSolverCreator() as in the
    reference.  When nept is recognised as nep's transpose (transpose_relation) every iteration makes ONE factorisation, whose
    transposed factors solve the nept system; otherwise two, as in the reference."""
    _lib.require_gpu()
    n = nep.size(1)
    lam = complex(lam)
    if linsolvercreator is None:
        linsolvercreator = BackslashLinSolverCreator()
    if errmeasure is None:
        errmeasure = DefaultErrmeasure(nep)
    if v is None:
        v = np.random.randn(n)
    if u is None:
        u = np.random.randn(n)
    ud = to_dev(np.asarray(u, dtype=np.complex128))[0]
    vd = to_dev(np.asarray(v, dtype=np.complex128))[0]
    dense.scal(ud, 1.0 / dense.nrm2(ud))
    dense.scal(vd, 1.0 / dense.nrm2(vd))
    z = ud.clone()
    err = np.inf
    for k in range(1, maxit + 1):
        err = estimate_error(errmeasure, lam, ud)
        if hist is not None:
            hist.append((k, err, lam))
        if err < tol:
            return lam, to_host(ud.reshape(1, n))[:, 0], to_host(vd.reshape(1, n))[:, 0]
        rel = transpose_relation(nep, nept, lam, 2)      # M(lam) and M'(lam) of both problems enter the step
        ls, lst, _ = twosided_linsolvers(nep, nept, lam, linsolvercreator, linsolvercreator, rel=rel)
        _mder_times(nep, lam, ud.reshape(1, n), z, 1)
        x = lin_solve(ls, z.reshape(1, n), tol=tol)
        dense.copy(x.reshape(n), ud)
        dense.scal(ud, 1.0 / dense.nrm2(ud))
        _mder_times(nept, lam, vd.reshape(1, n), z, 1)
        y = lin_solve(lst, z.reshape(1, n), tol=tol)
        dense.copy(y.reshape(n), vd)
        dense.scal(vd, 1.0 / dense.nrm2(vd))
        lam_vec = compute_rf(nep, ud, inner_solver, y=vd)
        lam = complex(lam_vec[np.argmin(np.abs(lam_vec - lam))])
    raise NoConvergenceException(lam, to_host(ud.reshape(1, n))[:, 0], err, "Number of iterations exceeded. maxit=%d." % maxit)
