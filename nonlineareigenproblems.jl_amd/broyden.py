"""Broyden's method with deflation (src/method_broyden.jl) on the device backend.

`broyden(nep, approxnep="eye", ...)` returns the reference's six values (S, X, T1, all_errhist, all_timehist, all_iterhist):
(S, X) is an invariant pair with the eigenvalues on the diagonal of S (get_deflated_eigpairs extracts eigenpairs), T1 = inv(M1)
stays a device tensor.

The inner iteration (broyden_T, :21-155) keeps the dense n x n approximate inverse Jacobian T on the device and touches it ONCE
per iteration, with nep_broyden_sweep (csrc/broyden.hip).  The reference reads T for T*rk (:69), T*ztilde (:101) and dv'*T (:107)
and rewrites it in T += Tztilde*aH (:117).  Here the rank-one update of iteration j stays pending as (Tztilde, aH) in two
ping-pong buffers and the sweep of iteration j + 1 applies it while it forms T*ztilde and dv'*T of the updated matrix.  T*rk
is not a pass over T at all: with rkp = gamma ztilde + (1 - gamma) rk,

    T_new rkp = gamma Tztilde + (1 - gamma) Trk + Tztilde (aH rkp).

Z and W (n x (p + 1)), the iterate and every residual stay on the device (nep_axpy / nep_scal / nep_gemm_ts, K1 for the
residual, nep_gemv_h for CH*[Z Trk]); the (p + 1) x (p + 1) solve, the step length gamma, beta and the error measure are host
scalars.  eigmethod: "eig" (dense eigen-decomposition of [M1 U1; X^H 0] on the host, a set-up step per level as in the
reference), "invpow" (the reference's inverse power iteration, applied on the device through T1 = inv(M1) and the k - 1 border:
no new factorisation); "eigs" raises ValueError, this backend has no sparse eigensolver.
"""
import math
import time
import warnings

import numpy as np
import scipy.sparse as sp
import torch

from . import _lib, dense, _hosteig
from ._lib import lib, check, hptr, c_vp
from .nep import NEP, CDT, to_dev, to_host, stream_ptr
from .newton import _mder_times

EPS = np.finfo(float).eps
EIGMETHODS = ("eig", "eigs", "invpow")


# ---- host scalars of an inner iteration -----------------------------------------------------------------------------------------
def clamp_pmax(pmax, n):
    """:257-260"""
    if pmax > n:
        warnings.warn("Too many eigenvalues requested. Reducing")
        return int(n)
    return int(pmax)


def small_solve(CHZ, CHTrk):
    """[du; dlam] = -(CH Z) \\ (CH Trk), :71"""
    return -np.linalg.solve(CHZ, CHTrk)


def step_length(abs_dlam, norm_dv, threshold):
    """:82-86: gamma = 1 unless the step is longer than `threshold`"""
    tt = math.sqrt(abs_dlam ** 2 + norm_dv ** 2)
    return threshold / tt if tt > threshold else 1.0


def w_update_row(du, dlam, norm_dv):
    """(bH, ||dv||^2 + ||du||^2 + |dlam|^2), :104"""
    nrm2 = norm_dv ** 2 + float(np.linalg.norm(du)) ** 2 + abs(dlam) ** 2
    return np.concatenate([np.conj(du), [np.conj(dlam)]]) / nrm2, nrm2


def broyden_default_errmeasure(lam, v, r):
    """:13-15"""
    return np.linalg.norm(r) / np.linalg.norm(v)


# ---- the sweep ------------------------------------------------------------------------------------------------------------------
def sweep_worksize(n):
    return int(lib.nep_broyden_sweep_worksize(int(n)))


def sweep(T, n, work, u0=None, a0=None, x=None, y=None, w=None, g=None, ldt=None):
    """one pass over T (device (n, ldt) tensor = column-major n x n): T += u0 a0 (a0 the row as it stands), y = T_new x,
    g = w^H T_new (the row, unconjugated); each pair is optional (nep_broyden_sweep).  Asynchronous."""
    p = lambda t: None if t is None else c_vp(t.data_ptr())
    check(lib.nep_broyden_sweep(int(n), p(T), int(T.shape[-1] if ldt is None else ldt), p(u0), p(a0), p(x), p(y), p(w), p(g),
                                p(work), stream_ptr()))


class _Counters:
    def __init__(self, n):
        self.n = n
        self.sweeps = self.setup_passes = self.drift_sweeps = self.syncs = self.t_bytes = 0

    def count(self, update, kind="sweeps"):
        setattr(self, kind, getattr(self, kind) + 1)
        self.t_bytes += (32 if update else 16) * self.n * self.n


# ---- T1 = inv(M1) ---------------------------------------------------------------------------------------------------------------
def inverse_on_device(M1):
    """inv(M1) as a device (n, n) tensor holding it column-major: dense M1 by the library's Gauss-Jordan inverse (nep_zinv_h_dev
    forms inv(.)^H, so it is given M1^H), sparse M1 by block solves of a DeviceLU against identity columns"""
    import ctypes as C
    n = M1.shape[0]
    out = torch.empty((n, n), dtype=CDT, device="cuda")
    if sp.issparse(M1):
        from .linsolvers import DeviceLU
        lu = DeviceLU(sp.csc_matrix(M1, dtype=np.complex128))
        nb = 64
        B = torch.empty((nb, n), dtype=CDT, device="cuda")
        for c0 in range(0, n, nb):
            k = min(nb, n - c0)
            B.zero_()
            B[:k, c0:c0 + k] = torch.eye(k, dtype=CDT, device="cuda")
            lu.solve(B[:k], out=out[c0:c0 + k])
        return out
    # column-major storage of M1^H = row-major storage of conj(M1)
    Md = torch.from_numpy(np.ascontiguousarray(np.conj(np.asarray(M1, dtype=np.complex128)))).to("cuda")
    work = torch.empty(2 * n + 2, dtype=CDT, device="cuda")
    info = C.c_int32(0)
    check(lib.nep_zinv_h_dev(n, c_vp(Md.data_ptr()), n, 0.0, c_vp(out.data_ptr()), n, c_vp(work.data_ptr()), C.byref(info), stream_ptr()))
    if info.value != 0:
        raise np.linalg.LinAlgError("SingularException: M1 is singular (pivot %d)" % (info.value - 1))
    return out


# ---- the inner iteration --------------------------------------------------------------------------------------------------------
def _vv(XV, p, lam, S, u, out):
    """out = v + X ((lam I - S) \\ u); XV (p + 1, n) holds the columns of X and v as its last column"""
    coef = np.ones(p + 1, dtype=np.complex128)
    if p:
        coef[:p] = np.linalg.solve(lam * np.eye(p) - S, u)
    dense.gemm_ts(XV, coef.reshape(p + 1, 1), out=out.reshape(1, -1))
    return out


def broyden_T(nep, v1, u1, lam1, CHd, T1, W1d, S, Xd, maxit=100, check_error_every=10, print_error_every=1, tol=1e-12,
              threshold=0.4, time0=None, errmeasure=None, logger=0, counters=None, drift=None):
    """broyden_T, :21-155, in the pending-update form of the module docstring.  v1: device vector; u1, lam1, S: host; CHd
    (p + 1, n): the columns of X and c (CH = CHd^H); T1 (n, n) device, copied; W1d (p + 1, n) device; Xd (p, n) device or None.
    Returns (lam, v (device), u, j, errhist, timehist)."""
    n = nep.size(1)
    p = S.shape[0]
    cnt = counters if counters is not None else _Counters(n)
    time0 = time.perf_counter() if time0 is None else time0
    lam = complex(lam1); u = np.array(u1, dtype=np.complex128)
    T = T1.clone()
    work = torch.empty(sweep_worksize(n), dtype=CDT, device="cuda")
    XV = torch.empty((p + 1, n), dtype=CDT, device="cuda")                # [X v]
    if p:
        XV[:p].copy_(Xd)
    XV[p].copy_(v1)
    v = XV[p]
    ZT = torch.empty((p + 2, n), dtype=CDT, device="cuda")                # [Z Trk]
    WZ = torch.empty((p + 3, n), dtype=CDT, device="cuda")                # [W ztilde rkp]
    WZ[:p + 1].copy_(W1d)
    zt, rkp = WZ[p + 1], WZ[p + 2]
    rk = torch.empty(n, dtype=CDT, device="cuda")
    vv = torch.empty(n, dtype=CDT, device="cuda")
    dv = torch.empty(n, dtype=CDT, device="cuda")
    Tz = [torch.empty(n, dtype=CDT, device="cuda") for _ in range(2)]
    aH = [torch.empty(n, dtype=CDT, device="cuda") for _ in range(2)]
    _mder_times(nep, lam, _vv(XV, p, lam, S, u, vv).reshape(1, n), rk, 0)
    for j in range(p + 1):                                                # Z = T W, Trk = T rk: set-up passes
        sweep(T, n, work, x=WZ[j], y=ZT[j]); cnt.count(False, "setup_passes")
    sweep(T, n, work, x=rk, y=ZT[p + 1]); cnt.count(False, "setup_passes")
    Trk = ZT[p + 1]
    errhist = np.full(maxit, np.nan); timehist = np.full(maxit, np.nan)
    pend = None                                                           # index of the ping-pong pair that holds (Tztilde, aH)
    cur = 0
    G = np.empty((p + 1, p + 2), dtype=np.complex128)
    dots = np.empty(p + 3, dtype=np.complex128); dot1 = np.empty(1, dtype=np.complex128)
    for j in range(1, maxit + 1):
        for q in range(p + 2):                                            # CH [Z Trk]
            G[:, q] = dense.gemv_h(CHd, ZT[q], p + 1, rows=n)
        dul = small_solve(G[:, :p + 1], G[:, p + 1])
        du, dl = dul[:p], dul[p]
        dense.gemm_ts(ZT, np.concatenate([-dul, [-1.0]]).reshape(p + 2, 1), out=dv.reshape(1, n))       # dv = -Z dul - Trk
        ndv = dense.nrm2(dv)
        gam = step_length(abs(dl), ndv, threshold)
        dense.axpy(gam, dv, v)
        u = u + gam * du; lam = lam + gam * dl
        _mder_times(nep, lam, _vv(XV, p, lam, S, u, vv).reshape(1, n), rkp, 0)
        dense.copy(rkp, zt)                                               # ztilde = (rkp - (1 - gamma) rk) / gamma
        if gam != 1.0:
            dense.axpy(-(1.0 - gam), rk, zt)
            dense.scal(zt, 1.0 / gam)
        if pend is None:
            sweep(T, n, work, x=zt, y=Tz[cur], w=dv, g=aH[cur])
        else:
            sweep(T, n, work, u0=Tz[pend], a0=aH[pend], x=zt, y=Tz[cur], w=dv, g=aH[cur])
        cnt.count(pend is not None)
        bH, nrm2 = w_update_row(du, dl, ndv)
        check(lib.nep_coldots(n, 1, c_vp(dv.data_ptr()), n, c_vp(Tz[cur].data_ptr()), n, hptr(dot1), stream_ptr()))
        beta = nrm2 + dot1[0]                                             # :106
        check(lib.nep_coldotsu(n, p + 3, c_vp(aH[cur].data_ptr()), 0, c_vp(WZ.data_ptr()), n, hptr(dots), stream_ptr()))
        dots *= -1.0 / beta                                               # aH W, aH ztilde, aH rkp
        dense.scal(aH[cur], -1.0 / beta)                                  # aH = -(dv' T) / beta, :107
        row = dots[:p + 1] + (1.0 + dots[p + 1]) * bH
        for q in range(p + 1):
            dense.axpy(row[q], Tz[cur], ZT[q])                            # Z += Tztilde (aH W + (1 + aH ztilde) bH), :110
            dense.axpy(bH[q], zt, WZ[q])                                  # W += ztilde bH, :113
        if gam != 1.0:
            dense.scal(Trk, 1.0 - gam)
            dense.axpy(gam + dots[p + 2], Tz[cur], Trk)                   # T_new rkp
        else:
            dense.copy(Tz[cur], Trk)
            dense.scal(Trk, 1.0 + dots[p + 2])
        pend, cur = cur, 1 - cur
        dense.copy(rkp, rk)
        cnt.syncs += p + 2 + 3
        if j % check_error_every == 0:
            if drift is not None:                                         # apply the pending update, compare a fresh T rk
                fresh = Tz[cur]
                sweep(T, n, work, u0=Tz[pend], a0=aH[pend], x=rk, y=fresh); cnt.count(True, "drift_sweeps")
                pend = None
                dense.axpy(-1.0, Trk, fresh)
                drift.append(dense.nrm2(fresh) / (dense.nrm2(T, n * n) * dense.nrm2(rk)))
            _vv(XV, p, lam, S, u, vv)
            if errmeasure is None:
                errhist[j - 1] = dense.nrm2(rk) / dense.nrm2(vv)
            else:
                errhist[j - 1] = errmeasure(lam, to_host(vv.reshape(1, n))[:, 0], to_host(rk.reshape(1, n))[:, 0])
            timehist[j - 1] = time.perf_counter() - time0
            if logger and j % print_error_every == 0:
                print("broyden_T: iteration %d, err = %.3e, lambda = %r" % (j, errhist[j - 1], lam))
            if errhist[j - 1] < tol:
                return lam, v.clone(), u, j, errhist[:j], timehist[:j]
    if logger:
        print("broyden_T: Too many iterations")
    return lam, v.clone(), u, maxit, errhist, timehist


# ---- the start pair -------------------------------------------------------------------------------------------------------------
def _start_eig(M1, U1, X):
    """:308-324 with eigmethod = :eig: the eigenvector of the smallest eigenvalue of [M1 U1; X^H 0], dense on the host"""
    n, k1 = X.shape
    M1d = M1.toarray() if sp.issparse(M1) else np.asarray(M1)
    MM = np.zeros((n + k1, n + k1), dtype=np.complex128)
    MM[:n, :n] = M1d; MM[:n, n:] = U1; MM[n:, :n] = X.conj().T
    d, V = _hosteig.eig(MM)
    return np.asarray(V)[:, int(np.argmin(np.abs(d)))]


def _start_invpow(T1, U1d, Xd, X, n, k1, cnt, maxit=4000):
    """:445-455 (eigs_invpow with sigma = 0) applied through T1 = inv(M1) and the border: [M1 U1; X^H 0] [a; b] = [f; g] is
    a = T1 f - (T1 U1) b with (X^H T1 U1) b = X^H T1 f - g.  z starts as ones and is normalised after every solve; the iteration
    stops early when a solve reproduces z bit for bit (further solves would change nothing)."""
    work = torch.empty(sweep_worksize(n), dtype=CDT, device="cuda")
    TU = torch.empty((max(k1, 1), n), dtype=CDT, device="cuda")
    for i in range(k1):
        sweep(T1, n, work, x=U1d[i], y=TU[i]); cnt.count(False, "setup_passes")
    Sc = dense.gram_h(Xd, TU, k1, k1, n) if k1 else None
    a = torch.ones(n, dtype=CDT, device="cuda"); b = np.ones(k1, dtype=np.complex128)
    y = torch.empty(n, dtype=CDT, device="cuda")
    prev = None
    for it in range(maxit):
        sweep(T1, n, work, x=a, y=y); cnt.count(False, "setup_passes")
        if k1:
            b = np.linalg.solve(Sc, dense.gemv_h(Xd, y, k1, rows=n) - b)
            dense.gemm_ts(TU, (-b).reshape(k1, 1), out=a.reshape(1, n), k=k1)
            dense.axpy(1.0, y, a)
        else:
            dense.copy(y, a)
        nz = math.sqrt(dense.nrm2(a) ** 2 + float(np.linalg.norm(b)) ** 2)
        dense.scal(a, 1.0 / nz); b = b / nz
        if it % 50 == 49:
            if prev is not None and torch.equal(prev[0], a) and np.array_equal(prev[1], b):
                break
            prev = (a.clone(), b.copy())
    return np.concatenate([to_host(a.reshape(1, n))[:, 0], b])


# ---- the driver -----------------------------------------------------------------------------------------------------------------
def broyden(nep, approxnep="eye", *, sigma=0, pmax=3, c=None, maxit=1000, addconj=False, check_error_every=10,
            print_error_every=1, threshold=0.2, tol=1e-12, errmeasure=None, add_nans=False, include_restart_timing=True,
            eigmethod="eig", logger=0, recompute_U=False, inner_logger=0, info=None, _drift=None):
    """Broyden's method with deflation, src/method_broyden.jl:235-439.  approxnep: "eye" (T1 = I, built on the device), an
    n x n array or a NEP (M1 = compute_Mder(approxnep, sigma)).  Returns (S, X, T1, all_errhist, all_timehist, all_iterhist):
    S, X and the histories on the host, T1 a device (n, n) tensor holding inv(M1) column-major.  errmeasure: None for the
    reference's default ||r|| / ||v|| (evaluated on the device) or a function (lam, v, r) of host arrays.  info (a dict)
    receives sweeps, iters, setup_passes, syncs_per_iteration and t_bytes."""
    time0 = time.perf_counter()
    n = int(nep.size(1))
    if eigmethod == "eigs":
        raise ValueError("eigmethod 'eigs' is not available: this backend has no sparse eigensolver (use 'eig' or 'invpow')")
    if eigmethod not in EIGMETHODS:
        raise ValueError("Unknown eig method %r" % (eigmethod,))
    if isinstance(approxnep, str) and approxnep != "eye":
        raise ValueError("approxnep must be 'eye', an n x n matrix or a NEP, not %r" % (approxnep,))
    if not isinstance(approxnep, (str, NEP)) and tuple(approxnep.shape) != (n, n):
        raise ValueError("approxnep: expected a %d x %d matrix, got %r" % (n, n, tuple(approxnep.shape)))
    pmax = clamp_pmax(pmax, n)
    sigma = complex(sigma)
    _lib.require_gpu()
    # Step 1: M1 and T1 = inv(M1)
    if isinstance(approxnep, str):
        M1 = sp.identity(n, dtype=np.complex128, format="csc")
        T1 = torch.eye(n, dtype=CDT, device="cuda")
    else:
        M1 = approxnep.compute_Mder(sigma) if isinstance(approxnep, NEP) else approxnep
        T1 = inverse_on_device(M1)
    cvec = np.ones(n, dtype=np.complex128) if c is None else np.asarray(c, dtype=np.complex128).reshape(n)
    cnt = _Counters(n)
    X = np.zeros((n, 0), dtype=np.complex128); S = np.zeros((0, 0), dtype=np.complex128)
    all_errhist, all_timehist, all_iterhist, iters = [], [], [], []
    UU = torch.zeros((pmax + 1, n), dtype=CDT, device="cuda")            # the columns of U1
    k, p_U1 = 1, 0
    while k <= pmax:
        k1 = k - 1
        Xd = to_dev(X) if k1 else None
        for i in range(0 if recompute_U else p_U1, k1):                  # Step 5, :300-305
            ei = np.zeros(k1, dtype=np.complex128); ei[i] = 1.0
            f = np.linalg.solve(sigma * np.eye(k1) - S, ei)
            _mder_times(nep, sigma, dense.gemm_ts(Xd, f.reshape(k1, 1)), UU[i], 0)
        p_U1 = k1
        U1 = to_host(UU[:k1]) if k1 else np.zeros((n, 0), dtype=np.complex128)
        if logger:
            print("broyden: running eigval comp for deflation")
        if eigmethod == "eig":                                           # Step 6
            x = _start_eig(M1, U1, X)
        else:
            x = _start_invpow(T1, UU, Xd, X, n, k1, cnt)
        v0, u0 = x[:n], x[n:]
        h = X.conj().T @ v0                                              # orthogonalise, :333-337
        v0 = v0 - X @ h
        u0 = u0 + (sigma * np.eye(k1) - S) @ h
        sc = np.vdot(cvec, v0)
        u0 = u0 / sc; v0 = v0 / sc
        if not include_restart_timing:
            time0 = time.perf_counter()
        d = math.sqrt(EPS)                                               # Step 7, :350-356
        v0d = to_dev(v0)
        W1d = torch.empty((k, n), dtype=CDT, device="cuda")
        if k1:
            W1d[:k1].copy_(UU[:k1])
        f1 = W1d[k1]
        tmp = torch.empty(n, dtype=CDT, device="cuda")
        _mder_times(nep, sigma + d, v0d, f1, 0)
        _mder_times(nep, sigma - d, v0d, tmp, 0)
        dense.axpy(-1.0, tmp, f1)
        dense.scal(f1, 1.0 / (2 * d))
        if k1:
            dense.gemm_ts(UU, (-np.linalg.solve(sigma * np.eye(k1) - S, u0)).reshape(k1, 1), out=tmp.reshape(1, n), k=k1)
            dense.axpy(1.0, tmp, f1)
        CHd = to_dev(np.column_stack([X, cvec]))
        if logger:
            print("broyden: Starting broyden n=%d" % n)
        lm, vmd, um, it, errhist, timehist = broyden_T(nep, v0d[0], u0, sigma, CHd, T1, W1d, S, Xd, maxit=maxit,
                                                      check_error_every=check_error_every, print_error_every=print_error_every,
                                                      threshold=threshold, tol=tol, errmeasure=errmeasure, time0=time0,
                                                      logger=inner_logger, counters=cnt, drift=_drift)
        iters.append(it)
        iterhist = np.arange(1, len(errhist) + 1) + (all_iterhist[-1] if len(all_iterhist) else 0)
        if add_nans and len(all_iterhist) > 1:                           # deflation book keeping, :385-393
            all_errhist.append(np.nan); all_timehist.append(np.nan); all_iterhist.append(np.nan)
        all_errhist += list(errhist); all_timehist += list(timehist); all_iterhist += list(iterhist)
        vm = to_host(vmd.reshape(1, n))[:, 0]
        nv = np.linalg.norm(vm)
        um = um / nv; vm = vm / nv
        if logger:
            print("broyden: Found an eigval %d:%r" % (k, lm))
        X = np.column_stack([X, vm])
        S = np.block([[S, um.reshape(k1, 1)], [np.zeros((1, k1)), np.array([[lm]])]])
        if abs(lm.imag) > tol * 10 and addconj:                          # :405-433
            v1 = np.conj(vm + (X[:, :k1] @ np.linalg.solve(lm * np.eye(k1) - S[:k1, :k1], um) if k1 else 0.0))
            l1 = np.conj(lm)
            rnorm = float(np.linalg.norm(to_host(nep.compute_Mlincomb(l1, to_dev(v1)).reshape(1, n))[:, 0]))
            if logger:
                print("broyden: Adding conjugate %d" % k)
            if rnorm > tol * 10:
                warnings.warn("Trying to add a conjugate pair which does not have a very small residual.")
            h = X.conj().T @ v1
            v1t = v1 - X @ h
            beta = np.linalg.norm(v1t)
            X = np.column_stack([X, v1t / beta])
            k += 1
            S1 = np.zeros((k, k), dtype=np.complex128)
            S1[:k - 1, :k - 1] = S
            S1[k - 1, k - 1] = l1
            R = np.eye(k, dtype=np.complex128)
            R[:k - 1, -1] = h; R[k - 1, k - 1] = beta
            S = np.linalg.solve(R.T, (R @ S1).T).T                       # (R S1) / R
        k += 1
    if logger:
        print("broyden: Iterations:%d" % (1 + sum(iters)))
    if info is not None:
        info.update(sweeps=cnt.sweeps, iters=list(iters), setup_passes=cnt.setup_passes, drift_sweeps=cnt.drift_sweeps,
                    syncs_per_iteration=cnt.syncs / max(sum(iters), 1), t_bytes=cnt.t_bytes, pmax=pmax, n=n)
    return S, X, T1, np.array(all_errhist), np.array(all_timehist), np.array(all_iterhist)
