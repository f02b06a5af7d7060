"""Infinite Arnoldi (iar) on the device backend -- same keyword surface as src/method_iar.jl:47-63.

Device-resident state: the basis V (n(m+1) x (m+1), 1.6 GB for gun m=100), z/y work vectors and the
Ritz block.  Per iteration only H's new column (k+1 numbers), the k x k eigenvector matrix of H, the
coefficient block and 2k norms cross PCIe.

Reference step (method_iar.jl:94-164)            device realisation
  y[:,2:k+1]=reshape(VV[1:nk,k],n,k)./(1:k)'      none: column k of V *is* an n x k block (ld n); the
                                                   1/j scaling is folded into the coefficient block
  y[:,1]=compute_Mlincomb!(nep,s,y,alpha)         K1 nep_mlincomb on that block
  y[:,1]=-lin_solve(M0inv,y[:,1])                 K5 nep_lu_solve(scale=-1) straight into V[0:n,k+1]
  vv=reshape(y[:,1:k+1])                          nep_iar_shift_scale (one pass over n*k entries)
  orthogonalize_and_normalize!(VV,vv,h,DGKS)      K6 nep_orth with the block-triangular row counts
  D,Z=eigen(H[1:k,1:k])                           host LAPACK (k x k)
  Q=VV[1:n,:]*Z                                   K7 nep_gemm_ts -> row-major Q^T
  err[k,s]=estimate_error(...) for s=1:k          K2 nep_resid_batch (one pass for all k pairs)
"""
import contextlib
import ctypes as _C
import queue
import threading
import time
from collections import deque
from concurrent.futures import ThreadPoolExecutor
from typing import NamedTuple

import numpy as np
import torch

from . import dense, _hosteig
from ._affinity import cpu_budget
from ._env import env_flag, env_float, env_int, env_str
from ._lib import (lib, check, c_vp, c_i32, hptr, cdouble, NepError, IarOpts, IarResult, FV_EVAL, NEP_ERR_BREAKDOWN, NEP_ERR_RETRY,
                   NEP_ERR_NOCONV)
from ._ritzchecks import RitzChecks
from ._streams import _check_stream, _eig_streams
from .errmeasure import (DefaultErrmeasure, ResidualErrmeasure, StandardSPMFErrmeasure, estimate_errors, estimate_errors_async)
from .exceptions import NoConvergenceException
from .linsolvers import DefaultLinSolverCreator, FactorizeLinSolver, create_linsolver
from .nep import CDT, AbstractSPMF, pure_spmf, to_host, to_host_cm, stream_ptr

EPS = np.finfo(float).eps


class _RefinementMiss(Exception):
    """a step's recorded backward errors show that UMFPACK's rule wanted more refinement than the step took"""


class _NativeRunMiss(Exception):
    """nep_iar_run returned NEP_ERR_RETRY for a reason the step-at-a-time pipeline handles itself (a device eigen-decomposition
    that reported a failure: that pipeline redoes the one decomposition with LAPACK)"""


class _OrthPassMiss(Exception):
    """the device-side DGKS of a step still met the re-orthogonalisation criterion after its last ENQUEUED pass (the
    reference's IterativeSolvers DGKS repeats while ||w|| < ||c|| / sqrt(2), without a bound): the call is re-run with the
    step-synchronous loop, whose nep_orth repeats until the criterion is no longer met"""


def iar(nep, orthmethod=dense.DGKS, maxit=30, linsolvercreator=None, tol=EPS * 10000, neigs=6,
        errmeasure=None, sigma=0.0, gamma=1.0, v=None, logger=0, check_error_every=1, proj_solve=False,
        errhist=None, timers=None, return_device=False, inner_solver_method=None):
    """src/method_iar.jl:56-141"""
    if v is None:
        v = np.random.randn(nep.size(1))
    kw = dict(orthmethod=orthmethod, maxit=maxit, linsolvercreator=linsolvercreator, tol=tol, neigs=neigs, errmeasure=errmeasure,
              sigma=sigma, gamma=gamma, v=v, logger=logger, check_error_every=check_error_every, proj_solve=proj_solve,
              errhist=errhist, timers=timers, return_device=return_device, inner_solver_method=inner_solver_method)
    flags = {}
    while True:                      # both downgrades may be needed in one call (each at most once)
        try:
            return _iar(nep, **kw, **flags)
        except _RefinementMiss:      # never observed; the checked path decides every refinement on the host
            if flags.get("_native_step") is False:
                raise
            iar.refinement_misses += 1
            flags["_native_step"] = False
        except _OrthPassMiss:        # "twice is enough" failed for a step: exact DGKS semantics through the synchronous loop
            if flags.get("_force_sync"):
                raise
            iar.orth_pass_misses += 1
            flags["_force_sync"] = True
        except _NativeRunMiss:
            if flags.get("_native_run") is False:
                raise
            iar.native_run_misses += 1
            flags["_native_run"] = False
        if errhist is not None:
            del errhist[:]


iar.refinement_misses = 0            # calls that were re-run with checked solves (diagnostics, tests)
iar.orth_pass_misses = 0             # calls that were re-run because a step wanted more DGKS passes than were enqueued
iar.native_run_misses = 0           # calls whose one-call native run (nep_iar_run) was re-run through the step-at-a-time pipeline
iar.native_runs = 0                 # calls served by nep_iar_run
iar.dev_eig_fallbacks = 0            # checks whose device eigen-decomposition reported a failure and was redone by LAPACK
iar.last_route = None                # the pipeline the last call took (_route; diagnostics, tests)


_EIG_WORK = {}
_EIG_WORK_LOCK = threading.Lock()
_EIG_WORK_KEEP = 2          # idle blocks kept per device (260 MB each at m = 100); more concurrent calls allocate and free their own


def _eig_work_acquire(need):
    """scratch of the device eigen-decompositions, CHECKED OUT for one iar call (its checker thread): the eigenvalue and the
    eigenvector kernels of a batch are two launches that share this block, so two calls that run on one GPU at the same time
    must not share it (call A's inverse iteration would read call B's matrices, status words clean).  Sequential calls get
    the same block back."""
    dev = torch.cuda.current_device()
    with _EIG_WORK_LOCK:
        free = _EIG_WORK.setdefault(dev, [])
        for i, w in enumerate(free):
            if w.numel() >= need:
                return free.pop(i)
        if free:
            free.pop()                      # too small for this call: let it go instead of keeping both
    return torch.empty(need, dtype=torch.uint8, device="cuda")


def _eig_work_release(w):
    """back to the pool; the caller has drained the streams that used it"""
    with _EIG_WORK_LOCK:
        free = _EIG_WORK.setdefault(w.device.index, [])
        if len(free) < _EIG_WORK_KEEP:
            free.append(w)


def _native_errmeasure(errmeasure, nep):
    """(kind, fro) of an error measure nep_iar_run evaluates itself (0: ||M(lam)v|| / ||v||, 1: the SPMF backward error), or None"""
    e = getattr(errmeasure, "errm", errmeasure) if isinstance(errmeasure, DefaultErrmeasure) else errmeasure
    if type(e) is StandardSPMFErrmeasure and e.nep is nep:
        return 1, np.ascontiguousarray(e.coeffs, dtype=np.float64)
    if type(e) is ResidualErrmeasure and e.nep is nep:
        return 0, None
    return None


def _plain_spmf(nep):
    """an SPMF operator whose products are the base class's own: what the native step and the one-call run compute themselves"""
    return pure_spmf(nep, "Mlincomb") and type(nep).lincomb_rowscale is AbstractSPMF.lincomb_rowscale


def _device_lu(M0inv):
    return type(M0inv) is FactorizeLinSolver and bool(getattr(M0inv.lu, "h", None))


class _Facts(NamedTuple):
    """what the choice of the route depends on, besides the NEP_IAR_* switches"""
    m: int
    orth: int                   # dense._orth_code(orthmethod)
    spmf_dev: bool              # _plain_spmf operator with a device handle
    dev_lu: bool                # _device_lu linear solver (with refinement coefficients, if it refines)
    native_err: bool            # an error measure nep_iar_run evaluates itself (_native_errmeasure)
    batch_async: bool           # an error measure with batch_async
    timed: bool = False         # `timers` given
    proj_solve: bool = False
    native_run: bool = True     # the private flags of _iar: False after the downgrade of iar()
    native_step: bool = True
    force_sync: bool = False

    def staged(self):
        """Asynchronous pipeline (default): nothing on the Arnoldi critical path waits for the device.  The DGKS decision
        is taken on the device (nep_orth_dev), H's new column travels to pinned host memory behind an event that the eigen
        worker waits for, the residual norms of the Ritz pairs come back the same way (nep_resid_batch_dev) -- the host
        enqueues step k+1.. while the device is still executing step k.  `timers` (instrumented run), MGS and
        NEP_IAR_SYNC=1 use the step-synchronous loop; both produce the same iterates."""
        return not (self.timed or self.orth not in (0, 1) or env_flag("NEP_IAR_SYNC") or self.proj_solve or self.force_sync)

    def native(self):
        """native step (csrc/driver.hip nep_iar_step): K1 -> K5 (+ refinement) -> shift -> K6 -> H row to pinned memory as
        ONE foreign call per Arnoldi step.  Needs a pure SPMF operator and a device LU."""
        return self.staged() and self.native_step and not env_flag("NEP_IAR_PYSTEP") and self.spmf_dev and self.dev_lu


def _route(f):
    """the pipeline a call takes (iar.last_route):
      run           nep_iar_run, one foreign call (_iar_native_run)
      step+deveig   nep_iar_steps, the checks with eig(H_k) on the device on their own thread (_DevEigChecker)
      step+hosteig  nep_iar_steps, the checks with LAPACK on host workers on their own thread (_host_eig_checker)
      async         one thread enqueues steps (native or Python) and checks, nothing waits for the device (_run_async)
      sync          the step-synchronous loop (_run_sync)"""
    if not f.staged():
        return "sync"
    if not f.native():
        return "async"
    # eigen-decompositions on the device (csrc/hesseig.hip) instead of LAPACK on host worker threads: no eig thread, no waiter
    # per step -- 133 ms of host CPU per headline call gone; NEP_IAR_EIG=host keeps the round-3 route (and is the fallback for
    # maxit beyond the LDS-resident limit, or when a decomposition reports a failure)
    dev_eig = f.m <= dense.HESS_EIG_KMAX and env_str("NEP_IAR_EIG", "dev") != "host"
    if (f.native_run and f.native_err and dev_eig and env_str("NEP_IAR_NATIVE_RUN", "1") != "0"
            and not any(env_flag(e) for e in ("NEP_IAR_TRACE", "NEP_IAR_ONE_STREAM", "NEP_IAR_PASSES"))):
        return "run"
    # The convergence checks (Ritz block K7 + residual batch K2 of step kc) read columns of V that are final by the time
    # eig(H_kc) exists -- the eigen worker waited for step kc's event -- and write only their own buffers, so they run on a
    # second stream next to the Arnoldi recurrence (latency-bound small kernels at gun size) instead of in line with it.
    # Only with the native step: there this thread touches none of the scratch the checks use (csrc/spmv.hip: coef / part /
    # ring belong to the residual batch, cwpart / cwring to the refinement inside the step).
    if env_flag("NEP_IAR_ONE_STREAM") or not f.batch_async:
        return "async"
    return "step+deveig" if dev_eig else "step+hosteig"


def _native_run_keeps_history(errhist, neigs, logger):
    """whether nep_iar_run gets an error-history buffer (h_err).  Without one, and with neigs = Inf, the run checks step m only
    (include/nepmi355.h): the errors of the steps before feed the history, the logger and the stop test, and nothing else
    (method_iar.jl:133-160).  So the buffer is left out exactly when nobody reads it: no errhist, no logger, and a stop test
    that cannot fire."""
    return errhist is not None or bool(logger) or not (np.isinf(neigs) and neigs > 0)


def _iar_native_run(nep, M0inv, orthmethod, m, tol, neigs, errkind, sigma, gamma, v, check_error_every, errhist, return_device,
                    logger=0):
    """the whole run as ONE foreign call (csrc/iar_run.hip nep_iar_run) -- what the Julia binding's `iar(nep::DeviceSPMF; ...)`
    method calls too (julia/NEPMI355X.jl); this host only marshals the inputs (derivative table, start vector, the f_t(lambda)
    callback) and shapes the outputs.  method_iar.jl:46-182."""
    n = nep.size(1)
    fv = nep.get_fv(); mt = len(fv)
    alpha = gamma ** np.arange(m + 1); alpha[0] = 0
    tab = nep.derivative_table(sigma, m)
    Ctab = np.asfortranarray((alpha[1:m + 1] / np.arange(1, m + 1))[:, None] * tab["fD"][1:m + 1, :], dtype=np.complex128)   # m x mt
    v0 = np.ascontiguousarray(v, dtype=np.complex128)
    rc_ = M0inv.refine_coefficients() if M0inv.umfpack_refinements > 0 else None
    if M0inv.umfpack_refinements > 0 and rc_ is None:
        return None
    o = IarOpts(m, int(check_error_every), dense._orth_code(orthmethod), int(max(0, M0inv.umfpack_refinements)), errkind[0],
                -1, float(tol), float(neigs), cdouble(sigma.real, sigma.imag), cdouble(gamma.real, gamma.imag))
    res = IarResult()

    def fv_eval(ctx, nlam, lam_p, F_p):
        try:
            la = np.frombuffer((_C.c_double * (2 * nlam)).from_address(lam_p), dtype=np.complex128)
            F = np.frombuffer((_C.c_double * (2 * nlam * mt)).from_address(F_p), dtype=np.complex128).reshape(nlam, mt)
            for t, f in enumerate(fv):
                F[:, t] = f.values(la)
            return 0
        except Exception:              # an exception must not cross the foreign frame: reported as a failed callback
            import traceback
            traceback.print_exc()
            return 1
    cb = FV_EVAL(fv_eval)
    ldv = n * (m + 1)
    V = torch.empty((m + 1, ldv), dtype=CDT, device="cuda")
    Qd = torch.empty((m, n), dtype=CDT, device="cuda") if return_device else None
    Qh = None if return_device else torch.empty((m, n), dtype=CDT, pin_memory=True)
    lam = np.zeros(m, dtype=np.complex128)
    err = np.full((m, m), np.nan, order="F") if _native_run_keeps_history(errhist, neigs, logger) else None
    # (M0inv.refine puts the refinement count the run starts with into o.refine_hint and takes what the run learnt from res)
    st = M0inv.refine.native_run(o, res, lambda: lib.nep_iar_run(
        nep.dev.h, M0inv.lu.h, n, _C.addressof(o), hptr(v0), hptr(Ctab), mt,
        hptr(rc_[0]) if rc_ else None, hptr(rc_[1]) if rc_ else None, hptr(errkind[1]) if errkind[1] is not None else None,
        _C.cast(cb, c_vp), None, hptr(lam), c_vp(Qd.data_ptr()) if Qd is not None else None,
        c_vp(Qh.data_ptr()) if Qh is not None else None, hptr(err) if err is not None else None, c_vp(V.data_ptr()),
        _C.addressof(res), stream_ptr()))
    if st == NEP_ERR_RETRY:
        if res.retry_reason == 1:
            raise _RefinementMiss(0)
        if res.retry_reason == 2:
            raise _OrthPassMiss(0)
        raise _NativeRunMiss(res.retry_reason)
    if st not in (0, NEP_ERR_NOCONV):
        check(st)
    iar.native_runs += 1
    iar.last_route = "run"
    k = int(res.k); nret = int(res.nret)
    M0inv.refine.solves += k
    if errhist is not None:
        for kc in range(1, k + 1):
            if kc % check_error_every == 0 or kc == m:
                errhist.append(err[kc - 1, :kc].copy())
    lam = lam[:nret].copy()
    Q = Qd[:nret] if return_device else Qh.numpy()[:nret].T
    if st == NEP_ERR_NOCONV:
        msg = "Number of iterations exceeded. maxit=%d." % m
        if res.nconv < 3:
            msg += "Try to change the inner_solver_method for better performance."
        raise NoConvergenceException(lam, to_host(Qd[:nret]) if return_device else Q, err[k - 1, :nret].copy(), msg)
    return lam, Q, V[:k]


def _iar(nep, orthmethod=dense.DGKS, maxit=30, linsolvercreator=None, tol=EPS * 10000, neigs=6,
         errmeasure=None, sigma=0.0, gamma=1.0, v=None, logger=0, check_error_every=1, proj_solve=False,
         errhist=None, timers=None, return_device=False, inner_solver_method=None, _native_step=True, _force_sync=False,
         _native_run=True):
    t_entry = time.perf_counter()
    n = nep.size(1); m = int(maxit)
    sigma = complex(sigma); gamma = complex(gamma)
    if linsolvercreator is None:
        linsolvercreator = DefaultLinSolverCreator()
    if errmeasure is None:
        errmeasure = DefaultErrmeasure(nep)
    if v is None:
        v = np.random.randn(n)
    errkind = _native_errmeasure(errmeasure, nep)
    f = _Facts(m=m, orth=dense._orth_code(orthmethod), dev_lu=True, native_err=errkind is not None,
               spmf_dev=_plain_spmf(nep) and type(nep).resid_norms is AbstractSPMF.resid_norms and hasattr(nep, "dev"),
               batch_async=hasattr(errmeasure, "batch_async"), timed=timers is not None, proj_solve=bool(proj_solve),
               native_run=_native_run, native_step=_native_step, force_sync=_force_sync)
    # ---- the one-call route: everything but the linear solver says `run`, so the solver is created here, ahead of the uploads
    M0inv = None
    if _route(f) == "run":
        M0inv = create_linsolver(linsolvercreator, nep, sigma)
        if _device_lu(M0inv):
            out = _iar_native_run(nep, M0inv, orthmethod, m, tol, neigs, errkind, sigma, gamma, v, check_error_every, errhist,
                                  return_device, logger)
            if out is not None:
                return out
    s = _State(t_entry, nep, orthmethod, m, linsolvercreator, M0inv, tol, neigs, errmeasure, sigma, gamma, v, check_error_every,
               proj_solve, errhist, timers, inner_solver_method, f.staged())
    f = f._replace(native_run=False, spmf_dev=_plain_spmf(nep) and "Cdev" in s.tab, dev_lu=_device_lu(s.M0inv))
    if f.native() and not s.create_native_step():
        f = f._replace(dev_lu=False)
    route = iar.last_route = _route(f)
    s.start(route)
    try:
        k = {"sync": _run_sync, "async": _run_async}.get(route, _run_steps)(s)
    finally:
        s.close()
    k = s.checks.k_checked if s.checks.k_checked > 0 else k - 1
    lam, Q = s.checks.finish(k, maxit, "Try to change the inner_solver_method for better performance.",
                             None if return_device else to_host_cm)
    return lam, Q, s.V[:k]


def _timed_eig(Hk):
    t = time.perf_counter()
    r = _hosteig.eig(Hk, hessenberg=True)       # LAPACK through ctypes: runs without the GIL (numpy/scipy hold it)
    return r, time.perf_counter() - t


class _State:
    """what the pipelines of one call share: the problem (nep, n, m, sigma, gamma, orthmethod, errmeasure, check_error_every, neigs,
    proj_solve, pnep, inner_solver_method), timing (tm, sync, trace, t_entry, t_marks, t_setup_done), the recurrence (V, ldv, H,
    tab, z, active, M0inv; staged pipelines: active_d, Hdev and its pinned mirror Hpin / Hnp, evs, filled; native step: cstep,
    work3, plans), the checks (checks, LAG, pool, pending, check_stream, eig_stream, dev_eig) and, on the step routes, the
    queue between the two threads (todo, slots, failure, unthrottled)"""

    def __init__(self, t_entry, nep, orthmethod, m, linsolvercreator, M0inv, tol, neigs, errmeasure, sigma, gamma, v,
                 check_error_every, proj_solve, errhist, timers, inner_solver_method, staged):
        """initialization (method_iar.jl:76-86), up to the linear solver"""
        self.t_entry = t_entry
        self.nep, self.orthmethod, self.m, self.neigs, self.errmeasure = nep, orthmethod, m, neigs, errmeasure
        self.sigma, self.gamma, self.check_error_every, self.proj_solve, self.staged = sigma, gamma, check_error_every, proj_solve, staged
        n = self.n = nep.size(1)
        self.tm = tm = timers if timers is not None else {}
        for key in ("mlincomb", "solve", "orth", "ritz", "resid", "host_eig"):
            tm.setdefault(key, 0.0)
        self.sync = torch.cuda.synchronize if timers is not None else (lambda: None)
        ldv = self.ldv = n * (m + 1)
        self.H = np.zeros((m + 1, m), dtype=np.complex128)
        alpha = gamma ** np.arange(m + 1); alpha[0] = 0
        # the synchronous little uploads below come BEFORE the linear solver: once the device is busy with the factorisation and
        # the apex build behind it, each of them waits for a slot between 300-600 us kernels (5 ms of host time for the lot) --
        # and the start vector BEFORE the 1.6 GB zero fill of the basis is enqueued (a pageable upload behind the fill held the host
        # for 0.46 ms; now the fill runs while the host assembles the call, the start vector goes in by a device copy behind it)
        v0 = np.asarray(v, dtype=np.complex128)
        v0d = torch.from_numpy(v0 / np.linalg.norm(v0)).to("cuda")
        self.t_marks = t_marks = [("v0", time.perf_counter())]
        # derivative table at sigma (DerSPMF, NEPTypes.jl:1108-1128).  The coefficient rows
        # C[j-1,:] = alpha_j/j * f^(j)(sigma) do not depend on k: uploaded once, each step uses the first k rows
        self.tab = nep.derivative_table(sigma, m, rowscale=alpha[1:m + 1] / np.arange(1, m + 1))
        t_marks.append(("tab", time.perf_counter()))
        self.z = torch.empty(n, dtype=CDT, device="cuda")
        self.active = (np.arange(1, m + 2) * n).astype(np.int64)   # column j has (j+1) non-zero blocks
        self.active_d = torch.from_numpy(self.active).to("cuda")
        self.V = torch.zeros((m + 1, ldv), dtype=CDT, device="cuda")     # the fill overlaps with the host side of the factorisation below
        self.V[0, :n].copy_(v0d)                                         # (the fill on a side stream next to the factorisation: no gain)
        t_marks.append(("V", time.perf_counter()))
        self.pnep = None; self.inner_solver_method = inner_solver_method
        if proj_solve:                                       # method_iar.jl:89-92
            from .projection import create_proj_NEP, DefaultInnerSolver
            self.pnep = create_proj_NEP(nep, maxsize=min(n, m + 1))
            if inner_solver_method is None:
                self.inner_solver_method = DefaultInnerSolver()
        if staged:
            self.Hdev = torch.zeros((m, m + 4), dtype=CDT, device="cuda")     # row k-1: h[0..k), beta, flags, 4 recorded omegas
            self.Hpin = torch.zeros((m, m + 4), dtype=CDT).pin_memory()
            self.Hnp = self.Hpin.numpy()
            self.evs = [None] * (m + 1)
            self.filled = [False] * (m + 1)
        t_ls = time.perf_counter()
        t_marks.append(("pre", t_ls))
        self.M0inv = M0inv if M0inv is not None else create_linsolver(linsolvercreator, nep, sigma)
        self.sync(); tm["linsolver_setup"] = tm.get("linsolver_setup", 0.0) + time.perf_counter() - t_ls
        self.t_setup_done = time.perf_counter()
        if timers is not None and hasattr(self.M0inv, "lu"):
            tm["host_factorization"] = tm.get("host_factorization", 0.0) + self.M0inv.lu.t_factor
        self.cstep = None
        self.checks = RitzChecks(m, tol, neigs, errhist, np.full((m, m), np.nan))

    def create_native_step(self):
        """nep_iar_create; False when the solver refines and has no refinement coefficients for this operator.  The refinement
        criterion is never read back inside a step: the step records omega of every iterate behind the H row and fill_H replays
        UMFPACK's stopping rule on the record (FactorizeLinSolver.review_recorded); a miss re-runs the call with checked solves."""
        nep, M0inv, tab, n, m = self.nep, self.M0inv, self.tab, self.n, self.m
        rc_ = M0inv.refine_coefficients() if M0inv.umfpack_refinements > 0 else None
        if M0inv.umfpack_refinements > 0 and rc_ is None:
            return False
        self.work3 = torch.empty(3 * n, dtype=CDT, device="cuda")
        hh = c_vp()
        check(lib.nep_iar_create(nep.dev.h, M0inv.lu.h, n, m, c_vp(self.V.data_ptr()), self.ldv, c_vp(tab["Cdev"].data_ptr()), tab["m"],
                                 c_vp(self.active_d.data_ptr()), c_vp(self.work3.data_ptr()),
                                 hptr(rc_[0]) if rc_ else None, hptr(rc_[1]) if rc_ else None, len(nep.get_fv()),
                                 c_vp(self.Hdev.data_ptr()), c_vp(self.Hpin.data_ptr()), dense._orth_code(self.orthmethod), _C.byref(hh)))
        self.cstep = hh
        return True

    def start(self, route):
        """the workers, streams and guards of the main loop.  The small dense eigenproblem of step k (host LAPACK,
        method_iar.jl:112; 7.5 ms at k=100, ~190 ms summed over a run) is solved on worker threads WHILE the device runs the
        following Arnoldi steps (mlincomb, solve, DGKS); the Ritz extraction + residuals of step k are enqueued as soon
        as its decomposition is available, at most LAG steps late and always in order.  The arithmetic and
        the returned quantities are those of the sequential loop; when the convergence test of step k ends
        the iteration, the (at most LAG+1) speculative Arnoldi steps beyond k are simply dropped."""
        self.t_marks += [("ls", self.t_setup_done), ("cstep", time.perf_counter())]
        # host eig of up to LAG+1 consecutive steps in flight: as many workers as the CPU budget of this rank allows (measured on
        # gun, 16-CPU budget: LAG 3 -> 86 ms per run, 5 -> 75, 9 -> 72, 15 -> 73)
        self.LAG = env_int("NEP_IAR_LAG", max(1, min(12, cpu_budget() - 3)))
        self.pool = ThreadPoolExecutor(max_workers=self.LAG + 1)
        self.pending = deque()         # (k, future) in increasing k; checks are always consumed in order
        self.trace = {} if env_flag("NEP_IAR_TRACE") else None
        self.plans = [0] * (self.m + 1)
        self.t_marks.append(("pool", time.perf_counter()))
        # ONE check stream per device for the life of the process: torch's caching allocator keeps freed blocks per stream, and a
        # fresh stream per call (32 of them in torch's pool) made every stream build its own cache of Ritz blocks
        self.check_stream = _check_stream() if route.startswith("step") else None
        self.dev_eig = route == "step+deveig"
        # its stream: one whose hardware queue is shared neither with this thread's stream nor with the check stream (probed once
        # per process and device, on this thread, before the first step is enqueued)
        self.eig_stream = _eig_streams(1, others=(torch.cuda.current_stream(), self.check_stream))[0] if self.dev_eig else None
        # the k x k eigenproblems gain nothing from a threaded BLAS (7.5 ms at k=100 with 1 or 64 threads) while its
        # spinning worker threads slow the launching thread down: pin BLAS to one thread for the duration of the loop
        import nep_amd_hostlu as _nep_hostlu
        ctl = _nep_hostlu.blas_controller()
        self.blas_guard = ctl.limit(limits=1) if ctl is not None else None
        if self.blas_guard is not None:
            self.blas_guard.__enter__()
        self.t_marks.append(("blas", time.perf_counter()))

    def close(self):
        for _, fut in self.pending:
            fut.cancel()
        self.pool.shutdown(wait=True)
        if self.check_stream is not None:
            self.check_stream.synchronize()       # dropped speculative checks may still read V / write their blocks
        if self.cstep is not None:
            lib.nep_iar_destroy(self.cstep)
        trace, t_entry, m = self.trace, self.t_entry, self.m
        if trace is not None:
            t_end = time.perf_counter()
            ks = [kk for kk in (1, 10, 25, 50, 75, 100) if "enq_%d" % kk in trace and "dev_done_%d" % kk in trace]
            print("iar trace (ms after entry): setup %.1f (%s) | " % ((self.t_setup_done - t_entry) * 1e3, " ".join("%s %.2f" % (a_, (b_ - t_entry) * 1e3) for a_, b_ in self.t_marks))
                  + " ".join("k=%d enq %.1f dev %.1f" % (kk, (trace["enq_%d" % kk] - t_entry) * 1e3, (trace["dev_done_%d" % kk] - t_entry) * 1e3) for kk in ks)
                  + " | end %.1f | native steps %d, %.1f ms inside nep_iar_step; checker: wait eig %.1f launch %.1f consume %.1f ms" % ((t_end - t_entry) * 1e3, trace.get("native_n", 0), trace.get("native_s", 0.0) * 1e3, trace.get("chk_wait", 0) * 1e3, trace.get("chk_launch", 0) * 1e3, trace.get("chk_consume", 0) * 1e3))
        if self.staged and env_flag("NEP_IAR_PASSES"):
            torch.cuda.synchronize()
            print("orth passes per step:", [int(self.Hnp[j - 1][j + 1].real) for j in range(1, m + 1)], "flags",
                  [int(self.Hnp[j - 1][j + 1].imag) for j in range(1, m + 1)])
        if self.blas_guard is not None:
            self.blas_guard.__exit__(None, None, None)

    def native_steps(self, k, nb):
        """steps k .. k+nb-1 as one foreign call, with the plan word of their solves"""
        M0inv, trace = self.M0inv, self.trace
        plan = M0inv.blind_plan_recorded()
        if plan > 0 and M0inv.settled_plan():
            plan |= 0x100                 # the kept iterate's backward error: recorded in every 8th step only
        t0 = time.perf_counter()
        check(lib.nep_iar_steps(self.cstep, k, nb, plan, stream_ptr()))
        if trace is not None:
            trace["native_s"] = trace.get("native_s", 0.0) + time.perf_counter() - t0
            trace["native_n"] = trace.get("native_n", 0) + nb
        for kk in range(k, k + nb):
            self.plans[kk] = plan
            M0inv.note_blind_solve(plan & 0xff)
            self.evs[kk] = "native"

    def arnoldi_step(self, k):
        if self.cstep is not None:
            return self.native_steps(k, 1)
        nep, V, ldv, n, z, M0inv, tm = self.nep, self.V, self.ldv, self.n, self.z, self.M0inv, self.tm
        t0 = time.perf_counter()
        # z = sum_{j=1..k} alpha_{j+1}/j * M^(j)(sigma) * V_k block j
        nep.lincomb_rowscale(self.tab, k, V.data_ptr() + 16 * (k - 1) * ldv, n, z)
        self.sync(); t1 = time.perf_counter()
        # new vector, block 0: -M(sigma)^{-1} z ; blocks 1..k: shifted/scaled old column
        vv = V[k]
        M0inv.solve_dev(z, out=vv[:n].reshape(1, n), scale=-1.0)
        self.sync(); t2 = time.perf_counter()
        check(lib.nep_iar_shift_scale(n, k, c_vp(V.data_ptr() + 16 * (k - 1) * ldv),
                                      c_vp(vv.data_ptr()), stream_ptr()))
        if self.staged:
            dense.orthogonalize_and_normalize_dev(V, vv, k, self.Hdev[k - 1], rows=n * (k + 1), ldv=ldv, active_dev=self.active_d,
                                                  method=self.orthmethod)
            self.Hpin[k - 1, :k + 2].copy_(self.Hdev[k - 1, :k + 2], non_blocking=True)
            self.evs[k] = torch.cuda.Event()
            self.evs[k].record()
            return
        h, beta, _ = dense.orthogonalize_and_normalize(V, vv, k, rows=n * (k + 1), ldv=ldv,
                                                       active_rows=self.active, method=self.orthmethod)
        self.H[:k, k - 1] = h; self.H[k, k - 1] = beta
        self.sync(); t3 = time.perf_counter()
        tm["mlincomb"] += t1 - t0; tm["solve"] += t2 - t1; tm["orth"] += t3 - t2

    def fill_H(self, kk):
        """columns 1..kk of H from the pinned buffer (their copies are complete once evs[kk] is)"""
        M0inv, plans = self.M0inv, self.plans
        for j in range(1, kk + 1):
            if not self.filled[j]:
                row = self.Hnp[j - 1]
                if int(row[j + 1].imag) & 2:
                    raise NepError(NEP_ERR_BREAKDOWN, "orthogonalisation breakdown in step %d: ||w|| = %g" % (j, row[j].real))
                if int(row[j + 1].imag) & 1 and dense._orth_code(self.orthmethod) == 0:
                    raise _OrthPassMiss(j)        # another DGKS pass was wanted after the last enqueued one
                if self.cstep is not None and M0inv.umfpack_refinements > 0:
                    if not M0inv.review_recorded(row[j + 2:j + 4].view(np.float64), plans[j] & 0xff,
                                                 final_recorded=not (plans[j] & 0x100 and j % 8 != 0)):
                        raise _RefinementMiss(j)
                self.H[:j, j - 1] = row[:j]
                self.H[j, j - 1] = row[j].real
                self.filled[j] = True

    def eig_async(self, kk):
        """eig(H_kk) on a pool worker, once the device has finished step kk"""
        if self.evs[kk] == "native":
            check(lib.nep_iar_wait(self.cstep, kk))      # ctypes releases the GIL
        else:
            self.evs[kk].synchronize()      # releases the GIL; H's columns <= kk are in pinned memory afterwards
        if self.trace is not None:
            self.trace["dev_done_%d" % kk] = time.perf_counter()
        self.fill_H(kk)
        return _timed_eig(self.H[:kk, :kk].copy())

    def due(self, k):
        return k % self.check_error_every == 0 or k == self.m

    def launch_check(self, kc, fut):
        """eigen-decomposition of step kc is available: enqueue Ritz block (K7) + residual batch (K2), no waiting"""
        (D, Z), t_eig = fut.result()
        laml = self.sigma + self.gamma / D
        with (torch.cuda.stream(self.check_stream) if self.check_stream is not None else contextlib.nullcontext()):
            QTl = dense.gemm_ts(self.V, Z, rowmajor=True, k=kc, rows=self.n, ldz=self.ldv)
            return kc, laml, QTl, estimate_errors_async(self.errmeasure, laml, QTl)

    def consume_check(self, kc, laml, QTl, perr):
        self.checks.record(kc, laml, QTl, perr.get())


def _run_sync(s):
    """the step-synchronous loop: `timers`, MGS, NEP_IAR_SYNC, proj_solve, or the re-run after an _OrthPassMiss"""
    k = 1
    pending, checks = s.pending, s.checks
    while k <= s.m and checks.conv_eig < s.neigs:
        s.arnoldi_step(k)
        if s.due(k):
            pending.append((k, s.pool.submit(_timed_eig, s.H[:k, :k].copy())))
        # consume finished eigen-decompositions; never let the check lag more than LAG steps
        while pending and checks.conv_eig < s.neigs and (len(pending) > s.LAG or pending[0][1].done()):
            _sync_check(s, *pending.popleft())
        k += 1
    while pending and checks.conv_eig < s.neigs:
        _sync_check(s, *pending.popleft())
    return k


def _sync_check(s, kc, fut):
    V, n, ldv, tm = s.V, s.n, s.ldv, s.tm
    (D, Z), t_eig = fut.result()
    tm["host_eig"] += t_eig
    t4 = time.perf_counter()
    laml = s.sigma + s.gamma / D
    if s.proj_solve:
        # method_iar.jl:118-131: orthonormal basis QQ of span(V[0:n, 0:kc]) (on the device: Gram matrix by K9,
        # scaling by K7, twice), Galerkin projection, inner solve started from RR*Z
        # (rank revealing: eigen-decomposition of the Gram matrix, directions below 1e-13 of the largest are dropped
        # -- the first-block rows of the Krylov basis become numerically dependent, and kc may exceed n)
        from .projection import inner_solve
        R_tot = np.eye(kc, dtype=complex)
        Qd = V; ldq = ldv; kq = kc
        for _ in range(2):
            QTm = dense.gemm_ts(Qd, np.eye(kq, dtype=complex), rowmajor=True, k=kq, rows=n, ldz=ldq)
            G = dense.gemm_h_rm(QTm, QTm, n, kq, kq)                             # K9 Gram matrix
            wg, Ug = np.linalg.eigh((G + G.conj().T) / 2)
            keep = wg > 1e-13 * wg[-1]
            T = Ug[:, keep] / np.sqrt(wg[keep])[None, :]                       # kq x r
            Rc = (np.sqrt(wg[keep])[:, None] * Ug[:, keep].conj().T)           # r x kq,  block = Q Rc
            Qd = dense.gemm_ts(Qd, T, k=kq, rows=n, ldz=ldq)                   # (r, n) column-major
            ldq = n; kq = int(np.sum(keep))
            R_tot = Rc @ R_tot
        s.pnep.set_projectmatrices(Qd, Qd)
        lamp, Qp = inner_solve(s.inner_solver_method, s.pnep, V=R_tot @ Z, lamv=laml.copy(), neigs=kc, sigma=np.mean(laml))
        laml = np.asarray(lamp); Qp = np.asarray(Qp)
        QTl = dense.gemm_ts(Qd, Qp, rowmajor=True, k=kq, rows=n, ldz=n)
    else:
        QTl = dense.gemm_ts(V, Z, rowmajor=True, k=kc, rows=n, ldz=ldv)       # (n, kc) row-major
    s.sync(); t5 = time.perf_counter()
    e = estimate_errors(s.errmeasure, laml, QTl) if len(laml) else np.zeros(0)
    t6 = time.perf_counter()
    tm["ritz"] += t5 - t4; tm["resid"] += t6 - t5
    s.checks.record(kc, laml, QTl, e)


def _run_async(s):
    """one thread enqueues the steps (native or Python), the eigen-decompositions run on pool workers, the checks are enqueued on the
    recurrence's stream and consumed when their norms have come back"""
    k = 1
    pending, checks, LAG = s.pending, s.checks, s.LAG
    pend_err = deque()         # checks whose device work is enqueued, in increasing k
    while k <= s.m and checks.conv_eig < s.neigs:
        s.arnoldi_step(k)
        if s.due(k):
            pending.append((k, s.pool.submit(s.eig_async, k)))
        # waiting for the oldest decomposition when more than LAG are in flight is what bounds how far the
        # host runs ahead of the device
        while pending and (len(pending) > LAG or pending[0][1].done()):
            pend_err.append(s.launch_check(*pending.popleft()))
        while pend_err and checks.conv_eig < s.neigs and (len(pend_err) > LAG or pend_err[0][3].ready()):
            s.consume_check(*pend_err.popleft())
        k += 1
    while (pending or pend_err) and checks.conv_eig < s.neigs:
        if pend_err:
            s.consume_check(*pend_err.popleft())
        else:
            pend_err.append(s.launch_check(*pending.popleft()))
    return k


def _run_steps(s):
    """native step: this thread only issues nep_iar_steps (one foreign call per chunk of steps, GIL released); the checker thread
    waits for the eigen-decompositions in order, enqueues their checks on check_stream and consumes the results.
    `slots` bounds how far the recurrence runs ahead of the checks (LAG + 1 decompositions in flight, as before)."""
    m, neigs, checks, LAG, trace = s.m, s.neigs, s.checks, s.LAG, s.trace
    s.todo = queue.Queue(); s.failure = failure = []
    # neigs = Inf: the iteration always runs to maxit, nothing the recurrence does ahead of the checks can be wasted,
    # so it is not throttled at all (the eigen-decompositions of the last steps -- half of all eig time -- then
    # queue up behind the device instead of pacing it)
    s.unthrottled = np.isinf(neigs)
    # (device decompositions go out in batches of up to NEP_IAR_EIG_BATCH steps: the look-ahead is that batch, whatever the CPU budget)
    s.slots = slots = threading.Semaphore(m + 1 if s.unthrottled else (max(LAG + 1, env_int("NEP_IAR_EIG_BATCH", 16)) if s.dev_eig else LAG + 1))
    th = threading.Thread(target=_DevEigChecker(s).run if s.dev_eig else (lambda: _host_eig_checker(s)), name="nep-iar-check", daemon=True)
    th.start()
    s.t_marks.append(("thread", time.perf_counter()))
    k = 1
    try:
        BATCH = 8 if s.unthrottled else max(1, min(4, LAG // 2))
        while k <= m and checks.conv_eig < neigs and not failure:
            # as many steps as there are free check slots (at most BATCH) go to the device in ONE foreign call: the
            # interpreter lock is released for all of it and re-acquired once (with one call per step this thread
            # queued for the lock behind the checker after every step: 330 us per step instead of 120)
            nb = 0
            while nb < BATCH and k + nb <= m:
                if s.due(k + nb):
                    if nb == 0:
                        while not slots.acquire(timeout=0.05):
                            if failure or not th.is_alive():
                                break
                    elif not slots.acquire(blocking=False):
                        break
                nb += 1
            if failure:
                break
            s.native_steps(k, nb)
            for kk in range(k, k + nb):
                if trace is not None:
                    trace["enq_%d" % kk] = time.perf_counter()
                if s.due(kk):
                    s.todo.put((kk, None if s.dev_eig else s.pool.submit(s.eig_async, kk)))
            k += nb
    finally:
        s.todo.put(None)
        th.join()
    if failure:
        raise failure[0]
    return k


def _host_eig_checker(s):
    """the checker thread of `step+hosteig`: waits for the decompositions of the pool workers in order"""
    checks, neigs, trace, LAG = s.checks, s.neigs, s.trace, s.LAG
    inflight = deque()
    try:
        while True:
            item = s.todo.get()
            if item is None:
                break
            if checks.conv_eig >= neigs:
                s.slots.release(); continue
            t0 = time.perf_counter()
            fut_ = item[1]; fut_.result(); t1 = time.perf_counter()
            inflight.append(s.launch_check(*item))
            s.slots.release()
            t2 = time.perf_counter()
            while inflight and checks.conv_eig < neigs and (len(inflight) > LAG or inflight[0][3].ready()):
                s.consume_check(*inflight.popleft())
            if trace is not None:
                t3 = time.perf_counter()
                trace["chk_wait"] = trace.get("chk_wait", 0.0) + t1 - t0
                trace["chk_launch"] = trace.get("chk_launch", 0.0) + t2 - t1
                trace["chk_consume"] = trace.get("chk_consume", 0.0) + t3 - t2
        while inflight and checks.conv_eig < neigs:
            s.consume_check(*inflight.popleft())
    except BaseException as exc:          # re-raised on the calling thread
        s.failure.append(exc)
        s.slots.release()
    finally:
        # the library's thread-local scratch of this thread goes back to the shared pool when the thread ends:
        # nothing this thread enqueued may still be pending then (dropped speculative checks)
        try:
            s.check_stream.synchronize()
        except Exception:
            pass


_EIG_TSTEP = 0.35                             # ms per Arnoldi step (gun, k ~ 100)


def _eig_batch_plan(m, check_error_every, bmax, lastb, t100):
    """Batch plan of the device eigen-decompositions for neigs = Inf: the check steps that END a batch.  A batch occupies the
    eig stream for the time of its LARGEST decomposition whatever its size, and cannot start before its last step has run:
    batches of about twice (decomposition time / step time) steps keep the stream half idle, so the last batch starts the
    moment step m is done; that last batch is kept smaller, because its checks (Ritz GEMM + residual batch, 0.17 ms each at
    k = 100) all come after its 3 ms.  Every check step is known in advance -> boundaries planned backwards from m.
    (csrc/iar_run.hip restates this plan; its comment knows this code by its earlier name, checker_dev.)"""
    allk = [kk for kk in range(1, m + 1) if kk % check_error_every == 0 or kk == m]
    ends = []; e_ = len(allk)
    size = min(lastb, e_)
    while e_ > 0:
        ends.append(allk[e_ - 1]); e_ -= size
        if e_ > 0:
            size = int(min(bmax, e_, max(1, np.ceil(2.0 * t100 * (allk[e_ - 1] / 100.0) ** 2 / (_EIG_TSTEP * check_error_every)))))
    return set(ends)


def _eig_batch_ready(pend, bmax, plan_end, done):
    """number of pending steps that form the next batch (0: wait for more).  plan_end None (the recurrence is throttled to
    LAG + 1 steps ahead of the checks): a batch is whatever is pending."""
    if not pend:
        return 0
    cnt = 1
    while cnt < len(pend) and cnt < bmax and pend[cnt] - pend[cnt - 1] == pend[1] - pend[0] and (plan_end is None or pend[cnt - 1] not in plan_end):
        cnt += 1
    if plan_end is None or pend[cnt - 1] in plan_end or cnt >= bmax or done:
        return cnt
    return 0


class _DevEigChecker:
    """the checker thread of `step+deveig`: the same checks with eig(H_kc) on the device.  (A) The decompositions of consecutive
    steps go out as BATCHES: one launch, one workgroup per step (a decomposition is a serial chain, 3 ms at k = 100, ten Arnoldi
    steps: the steps' decompositions have to overlap each other, and more than two or three extra streams stall the
    recurrence's own queue), on one of NS eig streams behind the event of the batch's last step -- nothing of it
    needs the host.  (B) When a batch's eigenvalues have reached the pinned mirror (an event behind the first
    kernel; only the inverse iterations are still running) the host forms lambda = sigma + gamma / D and f_t(lambda)
    per step and enqueues Ritz GEMM (B operand = the device eigenvector block) + residual batch on the check stream.
    (C) The 2 kc norms come back behind another event.  One thread polls the event queues; no LAPACK, no waiters."""

    def __init__(self, s):
        self.s = s

    def open(self):
        """scratch and plan, made on the checker thread"""
        s = self.s; m = s.m
        self.BMAX = max(1, env_int("NEP_IAR_EIG_BATCH", 16))
        self.wsz = (dense.hess_eig_worksize(m) + 15) // 16 * 16
        self.work = _eig_work_acquire(self.BMAX * self.wsz)
        self.wdev = torch.empty((m, m + 2), dtype=CDT, device="cuda")
        self.wpin = torch.zeros((m, m + 2), dtype=CDT).pin_memory()
        self.wnp = self.wpin.numpy()
        self.pendA = deque(); self.stA = deque(); self.stC = deque()
        self.force_fail = env_int("NEP_IAR_EIG_FAIL_AT", 0)   # tests: treat this step's decomposition as failed
        self.plan_end = None
        if s.unthrottled:
            self.plan_end = _eig_batch_plan(m, s.check_error_every, self.BMAX, max(1, env_int("NEP_IAR_EIG_LAST", 8)),
                                            env_float("NEP_IAR_EIG_MS100", 3.3))     # ms of one decomposition at k = 100 (scales as k^2)

    def host_redo(self, kc):
        """the device decomposition of step kc reported a failure: LAPACK on the host, Ritz block from its Z"""
        s = self.s
        iar.dev_eig_fallbacks += 1
        (D, Z), _ = _timed_eig(s.H[:kc, :kc].copy())
        with torch.cuda.stream(s.check_stream):
            QTl = dense.gemm_ts(s.V, Z, rowmajor=True, k=kc, rows=s.n, ldz=s.ldv)
        return D, QTl

    def launch_batch(self, count):
        s, m, wsz, work = self.s, self.s.m, self.wsz, self.work
        kcs = [self.pendA.popleft() for _ in range(count)]
        k0 = kcs[0]; nb = len(kcs); kmax = kcs[-1]
        kstep = (kcs[1] - k0) if nb > 1 else 0
        with torch.cuda.stream(s.eig_stream):
            sp_ = stream_ptr()
            check(lib.nep_iar_stream_wait(s.cstep, kmax, sp_))
            wrow = c_vp(self.wdev.data_ptr() + 16 * (k0 - 1) * (m + 2))
            mrow = c_vp(self.wpin.data_ptr() + 16 * (k0 - 1) * (m + 2))
            rc_ = lib.nep_hess_eigvals_batch_dev(nb, k0, kstep, c_vp(s.Hdev.data_ptr()), m + 4, wrow, kstep * (m + 2),
                                                c_vp(work.data_ptr()), wsz, mrow, kstep * (m + 2), sp_)
            if rc_ != 0 or env_flag("NEP_IAR_EIG_LAUNCH_FAIL"):
                # the launch itself was refused (e.g. a device that does not grant the kernel's 160 KB of LDS): not a
                # reason to abort the run -- the batch's decompositions go to LAPACK on the host (host_redo), behind an
                # event that says its last step has run
                evW = torch.cuda.Event(); evW.record()
                self.stA.append((kcs, None, kmax, evW, None))
                return
            evW = torch.cuda.Event(); evW.record()
            Zb = torch.empty((nb, kmax, kmax), dtype=CDT, device="cuda")
            check(lib.nep_hess_eigvecs_batch_dev(nb, k0, kstep, wrow, kstep * (m + 2), c_vp(Zb.data_ptr()), kmax, kmax * kmax,
                                                 c_vp(work.data_ptr()), wsz, mrow, kstep * (m + 2), sp_))
            evZ = torch.cuda.Event(); evZ.record()
        self.stA.append((kcs, Zb, kmax, evW, evZ))

    def run(self):
        self.open()
        s, checks, neigs, wnp, force_fail = self.s, self.s.checks, self.s.neigs, self.wnp, self.force_fail
        pendA, stA, stC, slots, check_stream = self.pendA, self.stA, self.stC, s.slots, s.check_stream
        done = False
        t_poll = 30e-6
        try:
            while True:
                progressed = False
                # ---- new steps
                while not done:
                    try:
                        item = s.todo.get_nowait() if (pendA or stA or stC) else s.todo.get()
                    except queue.Empty:
                        break
                    progressed = True
                    if item is None:
                        done = True
                    elif checks.conv_eig >= neigs:
                        slots.release()
                    else:
                        pendA.append(item[0])
                # ---- (A) batches onto the eig stream (its order is the order of the steps: nothing to wait for here)
                while checks.conv_eig < neigs:
                    cnt = _eig_batch_ready(pendA, self.BMAX, self.plan_end, done)
                    if not cnt:
                        break
                    self.launch_batch(cnt); progressed = True
                # ---- (B) eigenvalues on the host: Ritz values, coefficients, Ritz block + residual batch
                while stA and checks.conv_eig < neigs and stA[0][3].query():
                    progressed = True
                    kcs, Zb, kmax, evW, evZ = stA.popleft()
                    waited = False
                    for b_, kc in enumerate(kcs):
                        if s.trace is not None:
                            s.trace["dev_done_%d" % kc] = time.perf_counter()
                        s.fill_H(kc)
                        if Zb is None or wnp[kc - 1, kc].real != 0 or kc == force_fail:   # launch refused / QR iteration gave up (never observed)
                            D, QTl = self.host_redo(kc)
                        else:
                            D = wnp[kc - 1, :kc].copy()
                            with torch.cuda.stream(check_stream):
                                if not waited:
                                    check_stream.wait_event(evZ); waited = True
                                QTl = dense.gemm_ts_dev(s.V, Zb[b_], kc, kmax, rowmajor=True, k=kc, rows=s.n, ldz=s.ldv)
                        laml = s.sigma + s.gamma / D
                        with torch.cuda.stream(check_stream):
                            perr = estimate_errors_async(s.errmeasure, laml, QTl)
                        stC.append((kc, laml, QTl, perr, Zb))
                        slots.release()
                # ---- (C) norms on the host
                while stC and checks.conv_eig < neigs and stC[0][3].ready():
                    progressed = True
                    kc, laml, QTl, perr, Zb = stC.popleft()
                    if Zb is not None and (wnp[kc - 1, kc + 1].real != 0 or kc == -force_fail):   # an inverse iteration did not grow: redo on the host
                        D, QTl = self.host_redo(kc)
                        laml = s.sigma + s.gamma / D
                        with torch.cuda.stream(check_stream):
                            perr = estimate_errors_async(s.errmeasure, laml, QTl)
                    s.consume_check(kc, laml, QTl, perr)
                if checks.conv_eig >= neigs:
                    while pendA:
                        pendA.popleft(); slots.release()
                    while stA:
                        for _ in stA.popleft()[0]:
                            slots.release()
                    stC.clear()
                if done and not pendA and not stA and not stC:
                    break
                if not progressed:
                    time.sleep(t_poll)
        except BaseException as exc:          # re-raised on the calling thread
            s.failure.append(exc)
            slots.release()
        finally:
            try:
                s.eig_stream.synchronize()    # dropped speculative decompositions still read Hdev / write wdev
                check_stream.synchronize()
                _eig_work_release(self.work)  # (only behind a clean drain: a block with work pending is dropped, not shared)
            except Exception:
                pass
