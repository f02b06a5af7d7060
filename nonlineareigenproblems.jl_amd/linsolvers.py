"""Linear solvers for M(lam) x = b: host factorisation (one-off per shift), device triangular solves.

Mirrors src/LinSolvers.jl:100-159 and src/LinSolverCreators.jl:11-196:
`create_linsolver(creator, nep, lam)`, `lin_solve(solver, b; tol)`, `FactorizeLinSolver`,
`BackslashLinSolver`, `FactorizeLinSolverCreator(umfpack_refinements, max_factorizations, nep,
precomp_values)`, `BackslashLinSolverCreator`, `DefaultLinSolverCreator`; plus `LinSolverCache`
(src/rk_helper/linsolvercache.jl:7-26).

The reference factorises with UMFPACK on the host (`factorize(A)`, LinSolvers.jl:116).  Here the
host step is SuperLU (SciPy's bundled copy -- the only sparse LU in this image) and the factors
are uploaded once; every lin_solve is the HIP kernel k_lu_solve (csrc/trsv.hip).

This module is also the one address of everything a linear solver is made of: the host-LU process pool (_hostlu_pool.py),
the device factors and their per-pattern plans (_devicelu.py), the refinement rule and policy (_refine.py) and GMRES
(_gmres.py) are imported here under the names they have always had.
"""
import numpy as np
import scipy.sparse as sp
import torch

from . import _lib
from ._env import env_str
from ._lib import lib, check, hptr, c_vp
from .nep import CDT, to_dev, to_host, is_dev, pure_spmf, stream_ptr


class LinSolver:
    pass


class LinSolverCreator:
    pass


from ._hostlu_pool import HostLUPool, _nep_hostlu  # noqa: E402,F401
from ._devicelu import (DeviceLU, _DeviceRefactor, _Pattern, factor_term_rows, host_factor, lu_from_terms, reused,  # noqa: E402,F401
                        seed_plan_from_rank0, terms_route)
from ._refine import EPS, GO, TAKE_BACK, Refine, rule_step  # noqa: E402,F401
from ._gmres import GMRESLinSolver, GMRESLinSolverCreator  # noqa: E402


class FactorizeLinSolver(LinSolver):
    """src/LinSolvers.jl:109-137: factor M(lam) once, solve many right-hand sides.  Like UMFPACK's solve
    (control[8] = umfpack_refinements, LinSolvers.jl:118-120) each single-vector solve is followed by iterative
    refinement with UMFPACK's stopping rule: r = b - M(lam) x (kernel K1 through the NEP), componentwise backward error
    omega = max_i |r_i| / (|M||x| + |b|)_i (nep_cw_backward_error; |M| is bounded by sum_i |f_i(lam)| |A_i|); stop when
    omega < eps, when omega stops halving (reverting a step that made it worse) or after umfpack_refinements steps.
    The device factors use explicitly inverted diagonal blocks (trsv.hip), whose raw solves are a little less accurate
    than a plain substitution; the refinement makes the result independent of that.

    The rule and everything the solver remembers about its refinement live in `self.refine` (_refine.Refine)."""

    def __init__(self, nep, lam, umfpack_refinements=10, permc_spec=None, _lu=None, **lu_kw):
        self.nep = nep
        self.lam = lam
        self.refine = Refine(umfpack_refinements, nep, lam)
        lu_kw = reused(lu_kw)
        if _lu is None:
            _lu = lu_from_terms(nep, lam, permc_spec, lu_kw)
        self.lu = _lu if _lu is not None else DeviceLU(nep.compute_Mder(lam), permc_spec=permc_spec, **lu_kw)
        self._W = None
        self._cabs = None
        self._cf = None

    _lu_from_terms = staticmethod(lu_from_terms)

    umfpack_refinements = property(lambda self: self.refine.umf)
    last_omega = property(lambda self: self.refine.last_omega)
    solves = property(lambda self: self.refine.solves)
    refine_steps_taken = property(lambda self: self.refine.refine_steps_taken)
    refine_checks = property(lambda self: self.refine.refine_checks)

    def blind_plan_recorded(self):
        return self.refine.plan()

    def settled_plan(self):
        return self.refine.settled()

    def review_recorded(self, w, plan, final_recorded=True):
        return self.refine.review(w, plan, final_recorded)

    def note_blind_solve(self, plan):
        self.refine.note_blind_solve(plan)

    def _refine_setup(self):
        if self._W is None:
            n = self.lu.n
            self._W = torch.empty((4, n), dtype=CDT, device="cuda")                      # r, x, b, dx
            nep = self.nep
            if hasattr(nep, "get_fv") and hasattr(nep, "dev"):
                cf = np.ascontiguousarray([f.derivs(self.lam, 1)[0] for f in nep.get_fv()], dtype=np.complex128)
                self._cabs = np.ascontiguousarray(np.abs(cf))
                self._spmf = nep.dev.h
                # pure SPMF operator (compute_Mlincomb not overridden): M x is formed inside the criterion kernel
                self._cf = cf if pure_spmf(nep, "Mlincomb") else None

    def _residual(self, b, want_omega):
        """W[0] = b - M(lam) x  (x = W[1]); returns the backward error (None if not requested)."""
        W = self._W
        n = self.lu.n
        from . import dense
        if self._cabs is not None:
            om = np.zeros(1)
            fused = self._cf is not None
            Mx = None if fused else self.nep.compute_Mlincomb(self.lam, W[1].reshape(1, n))
            extra = None
            if want_omega and hasattr(self.nep, "refine_denominator_extra"):
                extra = self.nep.refine_denominator_extra(self.lam, W[1])          # (|P||x|) of non-SPMF operator parts
            check(lib.nep_cw_backward_error(self._spmf, hptr(self._cabs), hptr(self._cf) if fused else None,
                                            c_vp(W[1].data_ptr()), c_vp(b.data_ptr()),
                                            None if fused else c_vp(Mx.data_ptr()),
                                            c_vp(extra.data_ptr()) if extra is not None else None, c_vp(W[0].data_ptr()),
                                            hptr(om) if want_omega else None, stream_ptr()))
            return float(om[0]) if want_omega else None
        # NEP without an SPMF device handle: normwise backward error ||r|| / (||M||_F ||x|| + ||b||)
        Mx = self.nep.compute_Mlincomb(self.lam, W[1].reshape(1, n))
        dense.copy(b, W[2], n)
        dense.copy(Mx, W[0], n)
        dense.scal(W[0], -1.0, n)
        dense.axpy(1.0, W[2], W[0], n)
        if not want_omega:
            return None
        nr = np.empty(3)
        check(lib.nep_colnorms(n, 3, c_vp(W.data_ptr()), n, hptr(nr), stream_ptr()))
        return nr[0] / (self.lu.normA * nr[1] + nr[2]) if (nr[1] > 0 or nr[2] > 0) else 0.0

    def refine_coefficients(self):
        """(|f_t(lam)|, f_t(lam)) of a pure SPMF operator, or None when M x needs the NEP's own compute_Mlincomb"""
        self._refine_setup()
        return (self._cabs, self._cf) if (self._cabs is not None and self._cf is not None) else None

    def solve_dev(self, b, out=None, scale=1.0):
        """device solve; b: (n,) or (nrhs, n) tensor; out may alias b"""
        ref = self.refine
        blind = ref.next_solve()                 # sweeps to take on trust; None: omega is read back after every sweep
        single = b.dim() == 1 or b.shape[0] == 1
        if not single or blind == 0 or not hasattr(self.nep, "compute_Mlincomb"):
            return self.lu.solve(b, out=out, scale=scale)
        from . import dense
        self._refine_setup()
        n = self.lu.n
        W = self._W
        bd = b.reshape(1, n)
        x = W[1].reshape(1, n)
        r = W[0].reshape(1, n)
        X = torch.empty_like(b) if out is None else out
        self.lu.solve(bd, out=x)
        if blind is not None:
            for i in range(blind):
                self._residual(bd, False)
                if i == blind - 1:
                    self.lu.solve_add(r, x, X, scale)       # X = scale (x + A^{-1} r); b is not needed any more
                else:
                    self.lu.solve_add(r, x, x)
            ref.refine_steps_taken += blind
            return X.reshape(b.shape)
        steps = 0
        w_prev = np.inf
        while True:
            omega = self._residual(bd, True)
            verdict = rule_step(omega, w_prev, steps, ref.umf)
            if verdict != GO:
                break
            w_prev = omega
            self.lu.solve(r, out=W[3].reshape(1, n))
            dense.axpy(1.0, W[3], W[1], n)
            steps += 1
        if verdict == TAKE_BACK:
            dense.axpy(-1.0, W[3], W[1], n)
            omega = w_prev
        ref.checked_solve(steps, omega)
        dense.copy(W[1], X, n)
        if scale != 1.0:
            dense.scal(X, scale, n)
        return X.reshape(b.shape)


class BackslashLinSolver(LinSolver):
    """src/LinSolvers.jl:147-159: `A \\ x`, i.e. a fresh factorisation at every lin_solve."""

    def __init__(self, nep, lam, permc_spec=None, **lu_kw):
        self.A = nep.compute_Mder(lam)
        self.permc_spec = permc_spec
        self.lu_kw = lu_kw

    def solve_dev(self, b, out=None, scale=1.0):
        lu = DeviceLU(self.A, permc_spec=self.permc_spec, expected_solves=1, **self.lu_kw)
        self.last_lu = lu
        return lu.solve(b, out=out, scale=scale)


def lin_solve(solver, b, tol=0, scale=1.0):
    """src/LinSolvers.jl:125-137.  b: NumPy vector/matrix (-> NumPy result) or device tensor
    (nrhs, n) / (n,) (-> device result).  `scale` multiplies the result on the device."""
    host = not is_dev(b)
    bd = to_dev(b) if host else b
    if isinstance(solver, GMRESLinSolver) or getattr(solver, "accepts_tol", False):
        x = solver.solve_dev(bd, scale=scale, tol=tol)          # `tol` is a hint for iterative solvers (LinSolvers.jl:184)
    else:
        x = solver.solve_dev(bd, scale=scale)
    if host:
        xh = to_host(x if x.dim() == 2 else x.reshape(1, -1))
        return xh[:, 0] if np.ndim(b) == 1 else xh
    return x


class FactorizeLinSolverCreator(LinSolverCreator):
    """src/LinSolverCreators.jl:62-122 (factorisation recycling keyed by lam)."""

    def __init__(self, umfpack_refinements=10, max_factorizations=0, nep=None, precomp_values=(),
                 permc_spec=None, **lu_kw):
        if np.isscalar(precomp_values):
            precomp_values = [precomp_values]
        if len(precomp_values) > 0 and nep is None:
            raise ValueError("When you want to precompute factorizations you need to supply the keyword "
                             "argument `nep`")
        self.umfpack_refinements = umfpack_refinements
        self.max_factorizations = max_factorizations
        self.permc_spec = permc_spec
        self.lu_kw = lu_kw
        self.recycled_factorizations = {}
        for s in precomp_values:
            self.recycled_factorizations[complex(s)] = DeviceLU(nep.compute_Mder(s), permc_spec=permc_spec, **lu_kw)


class BackslashLinSolverCreator(LinSolverCreator):
    """`workers`: host processes used by drivers that know several shifts in advance (contour_beyn); None = auto,
    0 = factor in-process one node at a time."""

    def __init__(self, permc_spec=None, workers=None, **lu_kw):
        self.permc_spec = permc_spec
        self.workers = workers
        self.lu_kw = lu_kw


DefaultLinSolverCreator = FactorizeLinSolverCreator


def create_linsolver(creator, nep, lam):
    """src/LinSolverCreators.jl:107-122,143."""
    if hasattr(creator, "create_linsolver"):            # problem-specific creators (WEPLinSolverCreator, Waveguide.jl:504-519)
        return creator.create_linsolver(nep, lam)
    if isinstance(creator, BackslashLinSolverCreator):
        return BackslashLinSolver(nep, lam, creator.permc_spec, **creator.lu_kw)
    if isinstance(creator, GMRESLinSolverCreator):
        return GMRESLinSolver(nep, lam, creator.kwargs)
    key = complex(lam)
    if key in creator.recycled_factorizations:
        return FactorizeLinSolver(nep, lam, creator.umfpack_refinements, _lu=creator.recycled_factorizations[key])
    solver = FactorizeLinSolver(nep, lam, creator.umfpack_refinements, permc_spec=creator.permc_spec, **creator.lu_kw)
    if len(creator.recycled_factorizations) < creator.max_factorizations:
        creator.recycled_factorizations[key] = solver.lu
    return solver


class LinSolverCache:
    """src/rk_helper/linsolvercache.jl:7-26.

    `prefetch(shifts)`: a driver that knows its next shifts (nleigs: the node sequence sigma) announces them; their host
    factorisations (compute_Mder + SuperLU, which releases the GIL) then run on one background thread while the device
    works on the current step, and `_get` only builds the device schedule from the finished factors.  Only for the
    factorising creator; at most `ahead` factorisations are in flight or waiting to be used."""

    def __init__(self, nep, linsolvercreator, ahead=2):
        self.nep = nep
        self.linsolvercreator = linsolvercreator
        self.solvers = {}
        self.ahead = ahead
        self._pending = {}
        self._pool = None

    def _host_factors(self, sigma):
        c = self.linsolvercreator
        Ac = sp.csc_matrix(self.nep.compute_Mder(sigma), dtype=np.complex128)
        return host_factor(Ac, c.permc_spec, c.lu_kw.get("diag_pivot_thresh"), c.lu_kw.get("symmetric_mode"))

    def _device_plan_ready(self):
        """True when the sparsity pattern of this NEP's M(sigma) has a device-factorisation plan: the shifts are then factorised
        on the GPU when they are needed (3.5 ms each on gun) and nothing is prefetched on the host"""
        c = self.linsolvercreator
        if type(c) is not FactorizeLinSolverCreator or not _DeviceRefactor.enabled():
            return False
        if getattr(self, "_plan_key", None) is None:
            try:
                A = sp.csc_matrix(self.nep.compute_Mder(0.5 + 0.25j), dtype=np.complex128)   # any shift: the pattern is what counts
            except Exception:
                self._plan_key = False
                return False
            kw = c.lu_kw
            self._plan_key = _DeviceRefactor.key(A, (c.permc_spec, kw.get("diag_pivot_thresh"), kw.get("symmetric_mode")))
            self._pattern = _Pattern(A.indptr, A.indices, A.shape)
        return self._plan_key is not False and _DeviceRefactor.lookup(self._plan_key) is not None

    def prefetch(self, shifts, keep_all=None):
        """`keep_all` (optional): every distinct shift the driver WILL use and keep (nleigs with reusefact = 2).  When the pattern has a
        device-factorisation plan they are factorised in ONE batched pass (nep_lu_factor_dev_batch: each of the ~600 launches of the
        numeric factorisation carries all of them, and their solve schedules are built together) -- config C3: five shifts, 96 -> 88 ms."""
        c = self.linsolvercreator
        if type(c) is not FactorizeLinSolverCreator or env_str("NEP_LU_PREFETCH", "1") == "0":
            return
        if self._device_plan_ready():
            if keep_all is not None and not getattr(self, "_batched", False):
                self._batched = True
                todo = [complex(s) for s in keep_all if np.isfinite(complex(s)) and complex(s) not in self.solvers
                        and complex(s) not in c.recycled_factorizations]
                plan = _DeviceRefactor.lookup(self._plan_key)
                if len(todo) >= 2 and plan is not None:
                    mats = [sp.csc_matrix(self.nep.compute_Mder(k), dtype=np.complex128) for k in todo]
                    P = self._pattern
                    if all(M.shape == P.shape and np.array_equal(M.indptr, P.indptr) and np.array_equal(M.indices, P.indices) for M in mats):
                        lus = _DeviceRefactor.factor_batch(plan, mats[0].shape[0], np.stack([M.data for M in mats]),
                                                           expected_solves=reused(c.lu_kw)["expected_solves"])
                        for key, lu in zip(todo, lus):
                            if lu is not None:          # (a refused one is factorised on its own when it is needed)
                                self.solvers[key] = FactorizeLinSolver(self.nep, key, c.umfpack_refinements, _lu=lu)
            return
        for s in shifts:
            key = complex(s)
            if len(self._pending) >= self.ahead:
                break
            if not np.isfinite(key) or key in self.solvers or key in self._pending or key in c.recycled_factorizations:
                continue
            if self._pool is None:
                from concurrent.futures import ThreadPoolExecutor
                self._pool = ThreadPoolExecutor(max_workers=1, thread_name_prefix="nep-lu-prefetch")
            self._pending[key] = self._pool.submit(self._host_factors, key)

    def _get(self, sigma, add_to_cache):
        key = complex(sigma)
        if key in self.solvers:
            return self.solvers[key]
        c = self.linsolvercreator
        if key in self._pending:
            factors = self._pending.pop(key).result()
            lu_kw = reused(c.lu_kw)
            # (the prefetched host factors seed the pattern's device-factorisation plan like a factorisation made in place would:
            # a process that only runs nleigs factorises its shifts on the GPU from the second call on)
            lu = DeviceLU(factors=factors, permc_spec=c.permc_spec, diag_pivot_thresh=lu_kw.get("diag_pivot_thresh"),
                          symmetric_mode=lu_kw.get("symmetric_mode"), plan_pattern=getattr(self, "_pattern", None),
                          expected_solves=lu_kw["expected_solves"])
            solver = FactorizeLinSolver(self.nep, sigma, c.umfpack_refinements, _lu=lu)
            if len(c.recycled_factorizations) < c.max_factorizations:
                c.recycled_factorizations[key] = lu
        elif self._pool is not None and not self._device_plan_ready():
            # keep host factorisations on the one worker thread (they toggle the process-wide BLAS thread count)
            self._pending[key] = self._pool.submit(self._host_factors, key)
            return self._get(sigma, add_to_cache)
        else:
            solver = create_linsolver(c, self.nep, sigma)         # DeviceLU(A): device factorisation when the plan exists
        if add_to_cache:
            self.solvers[key] = solver
        return solver

    def close(self):
        if self._pool is not None:
            for f in self._pending.values():
                f.cancel()
            self._pool.shutdown(wait=True)
            self._pool = None
            self._pending = {}

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def solve(self, sigma, y, add_to_cache):
        return lin_solve(self._get(sigma, add_to_cache), y)

    def solve_dev(self, sigma, y, add_to_cache, out=None, scale=1.0):
        return self._get(sigma, add_to_cache).solve_dev(y, out=out, scale=scale)



class DeflatedNEPLinSolver(LinSolver):
    """src/LinSolvers.jl:194-252: solves with the bordered matrix Mt(lam) = [M U; X^H 0] of a deflated NEP, recycling the linear
    solver of the ORIGINAL NEP.  The reference forms the Schur complement S = -X^H M^-1 U with p + 1 solves; with X^H X = I
    (normalize_schur_pair) and U = M X (lam I - S0)^-1, M^-1 U = X (lam I - S0)^-1 exactly, so S = -(lam I - S0)^-1 and

        y = M^-1 b1,   c = b2 - X^H y,   v1 = y + X c,   v2 = -(lam I - S0) c

    is ONE solve with the original solver plus one pass over X (nep_defl_border, csrc/deflate_border.hip).  Works for the three
    deflation modes alike (only orgnep, S0 and V0 are used).  Like the reference's, the solve is as accurate as M(lam) is
    conditioned: the solver is for shifts away from the deflated eigenvalues (jd_effenberger's iterates); at a deflated
    eigenvalue use the deflated NEP's own solver, which factorises the bordered matrix as a whole."""

    def __init__(self, deflated_nep, lam, orglinsolver):
        self.deflated_nep = deflated_nep
        self.lam = complex(lam)
        self.orglinsolver = orglinsolver
        self._Xd = None

    @property
    def Xd(self):
        if self._Xd is None:
            d = self.deflated_nep
            self._Xd = d.Xd if hasattr(d, "Xd") else to_dev(d.V0)       # (p, n0): column-major n0 x p
        return self._Xd

    def _table(self):
        d = self.deflated_nep
        return _lib.as_c128(d.S0 - self.lam * np.eye(d.p), "F")         # -(lam I - S0)

    def _border_fused(self, x, b2, T, scale):
        """x (n0 + p entries, the first n0 holding y) -> scale [v1; v2] in place by nep_defl_border; False for p > 32"""
        d = self.deflated_nep
        rc = lib.nep_defl_border(d.n0, d.p, c_vp(self.Xd.data_ptr()), d.n0, c_vp(x.data_ptr()),
                                 c_vp(b2.data_ptr()) if b2 is not None else None, hptr(T), float(scale), c_vp(x.data_ptr()),
                                 stream_ptr())
        if rc == _lib.NEP_ERR_UNSUPPORTED:
            return False
        check(rc)
        return True

    def _border_composed(self, x, b2, T, scale):
        """the same result from existing device primitives, for p > 32: c = b2 - X^H y by nep_gemv_hd and nep_axpy, T c and
        X c by the GEMM with a device B, nep_axpy and nep_scal.  Nothing is copied to the host."""
        from . import dense
        d = self.deflated_nep
        n0, p = d.n0, d.p
        c = torch.empty(p, dtype=CDT, device="cuda")
        check(lib.nep_gemv_hd(c_vp(self.Xd.data_ptr()), n0, n0, p, c_vp(x.data_ptr()), None, c_vp(c.data_ptr()), stream_ptr()))
        dense.scal(c, -1.0, p)
        if b2 is not None:
            dense.axpy(1.0, b2, c, p)
        Xc = dense.gemm_ts_dev(self.Xd, c, 1, p, k=p, rows=n0, ldz=n0)             # (1, n0)
        dense.axpy(1.0, Xc, x, n0)
        Td = to_dev(T)                                                               # (p, p): column-major T
        dense.gemm_ts_dev(Td, c, 1, p, out=x[n0:].reshape(1, p), k=p, rows=p, ldz=p)
        if scale != 1.0:
            dense.scal(x, scale, n0 + p)

    def solve_dev(self, b, out=None, scale=1.0):
        """device solve; b: (n0 + p,) or (nrhs, n0 + p) tensor; out may alias b"""
        d = self.deflated_nep
        n0, p, n = d.n0, d.p, d.n
        if b.dim() == 2 and b.shape[0] > 1:
            X = torch.empty_like(b) if out is None else out
            for j in range(b.shape[0]):
                self.solve_dev(b[j], out=X[j], scale=scale)
            return X
        if b.numel() != n or not b.is_contiguous():
            raise ValueError("b must have %d entries" % n)
        X = torch.empty_like(b) if out is None else out
        bv, x = b.reshape(n), X.reshape(n)
        b2 = bv[n0:]
        if b2.data_ptr() + 16 * p > x.data_ptr() and x.data_ptr() + 16 * n > b2.data_ptr():
            b2 = b2.clone()                                   # out is b (or overlaps its tail): the p tail entries are kept first
        self.orglinsolver.solve_dev(bv[:n0], out=x[:n0])
        T = self._table()
        if not self._border_fused(x, b2, T, scale):
            self._border_composed(x, b2, T, scale)
        return X.reshape(b.shape)


class DeflatedNEPLinSolverCreator(LinSolverCreator):
    """src/LinSolverCreators.jl:149-181: creates the solver of the original NEP with `orglinsolvercreator` and wraps it"""

    def __init__(self, orglinsolvercreator=None):
        self.orglinsolvercreator = DefaultLinSolverCreator() if orglinsolvercreator is None else orglinsolvercreator

    def create_linsolver(self, nep, lam):
        from .deflation import DeflatedGenericNEP, DeflatedNEPMM, DeflatedSPMF
        if not isinstance(nep, (DeflatedGenericNEP, DeflatedNEPMM, DeflatedSPMF)):
            raise TypeError("DeflatedNEPLinSolverCreator needs a deflated NEP (deflate_eigpair), got %s" % type(nep).__name__)
        return DeflatedNEPLinSolver(nep, lam, create_linsolver(self.orglinsolvercreator, nep.orgnep, lam))
