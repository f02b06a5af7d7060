"""Infinite bi-Lanczos (src/method_infbilanczos.jl:33-246; Gaaf and Jarlebring, SIAM J. Sci. Comput. 39, 2017).

A host loop over device primitives, as rfi: the right and left blocks R, Q and R~, Q~ are device (k, n) tensors (column-major
n x k blocks), the two solves per step go through twosided_linsolvers (one factorisation of M(sigma) when nept is recognised
as nep's transpose), and the left-right scalar product -- the reference's "nasty double loop" of ma compute_Mlincomb calls
and ma dot products -- is one call of K11 (nep_lr_hankel, csrc/lrprod.hip):

    c = - sum_t sum_{j<ma} sum_{i<mb} tau_t[i+j+1] w_j^H A_t b_i,    tau_t[d] = f_t^(d)(sigma) / d!

with the Taylor table tau of nep's functions (ScalarFun.taylor) resident on the device.  The small tridiagonal eigenproblem
is solved on the host, as in the reference.
"""
import math

import numpy as np
import torch

from . import _lib, dense
from ._lib import lib, check, hptr, c_vp, NepError, NEP_ERR_UNSUPPORTED
from .errmeasure import DefaultErrmeasure, estimate_errors
from .exceptions import NoConvergenceException
from .linsolvers import lin_solve
from .nep import CDT, pure_spmf, to_dev, dptr, stream_ptr
from .twosided import twosided_linsolvers


def _standard_spmf(nep):
    return pure_spmf(nep, "Mlincomb")


def taylor_table(nep, sigma, m):
    """device (mt, m) tensor whose row t holds tau_t[d] = f_t^(d)(sigma) / d!, d < m: an m x mt column-major block, the layout
    of nep_lr_hankel's table and of nep_mlincomb_dev's coefficient block"""
    T = np.stack([np.asarray(f.taylor(complex(sigma), m), dtype=np.complex128) for f in nep.get_fv()])
    return torch.from_numpy(np.ascontiguousarray(T)).to("cuda")


def lr_hankel(nep, W, B, ma, mb, tau):
    """K11: c = - sum_t sum_{j<ma, i<mb} tau[t, i+j+1] w_j^H A_t b_i for device blocks W, B ((k, ld) tensors: column-major
    ld x k blocks, ld >= n) and a table from taylor_table with at least ma + mb orders.  NepError with status
    NEP_ERR_UNSUPPORTED when ma or mb exceeds 256."""
    assert W.dtype == CDT and B.dtype == CDT and tau.dtype == CDT
    assert W.is_contiguous() and B.is_contiguous() and tau.is_contiguous()
    assert W.shape[0] >= ma and B.shape[0] >= mb and tau.shape[0] == len(nep.get_fv()) and tau.shape[1] >= ma + mb
    out = np.zeros(1, dtype=np.complex128)
    check(lib.nep_lr_hankel(nep.dev.h, int(ma), int(mb), c_vp(W.data_ptr()), W.shape[1], c_vp(B.data_ptr()), B.shape[1],
                            c_vp(tau.data_ptr()), tau.shape[1], hptr(out), None, stream_ptr()))
    return complex(out[0])


def _lrsp_loop(nep, At, B, ma, mb, sigma):
    """the reference's loop (src/method_infbilanczos.jl:229-246): for j = 1..ma, compute_Mlincomb(nep, sigma, B[:, 1:mb], dd, j)
    with dd_i = 1/(j+i-1)! (the reference scales the columns of B by dd and passes ones: the same sum), then dot(At[:, j], .)"""
    c = 0j
    for j in range(1, ma + 1):
        dd = np.exp(-np.array([math.lgamma(j + i + 1) for i in range(mb)]))
        z = nep.compute_Mlincomb(sigma, B[:mb], dd, j)
        c -= complex(dense.gemv_h(At[j - 1:j], z.reshape(-1), 1)[0])
    return c


def left_right_scalar_prod(nep, At, B, ma, mb, sigma, tau=None, mode="auto"):
    """src/method_infbilanczos.jl:229-246.  At, B: device (k, n) tensors (column-major n x k blocks) or host n x k arrays.
    K11 for an SPMF whose compute_Mlincomb is the standard one (`tau`: its Taylor table at sigma, built when missing or
    short); the reference's loop over compute_Mlincomb for any other NEP, for mode="loop", and when K11 refuses the sizes
    (ma or mb above 256).  Only nep enters, as in the reference."""
    if not torch.is_tensor(At):
        At = to_dev(At)
    if not torch.is_tensor(B):
        B = to_dev(B)
    if mode == "auto" and _standard_spmf(nep):
        if tau is None or tau.shape[1] < ma + mb:
            tau = taylor_table(nep, sigma, ma + mb)
        try:
            return lr_hankel(nep, At, B, ma, mb, tau)
        except NepError as e:
            if e.status != NEP_ERR_UNSUPPORTED:
                raise
    return _lrsp_loop(nep, At, B, ma, mb, sigma)


def _lincomb_taylor(nep, tab, V, k, lam):
    """sum_{i=1..k} M^(i)(lam)/i! v_i, the compute_Mlincomb(nep, lam, Q1*Dk, ones(k), 1) of :125 and :132.  Standard SPMF: the
    Taylor table from row 1 on is the coefficient block (nep_mlincomb_dev), no scaled copy of V, no factorials"""
    if tab is not None:
        z = torch.empty(V.shape[1], dtype=CDT, device="cuda")
        check(lib.nep_mlincomb_dev(nep.dev.h, k, dptr(tab, 0, 1), tab.shape[1], c_vp(V.data_ptr()), V.shape[1],
                                   c_vp(z.data_ptr()), stream_ptr()))
        return z
    dk = np.exp(-np.array([math.lgamma(i + 2) for i in range(k)]))
    return nep.compute_Mlincomb(lam, V[:k], dk, 1).reshape(-1)


def infbilanczos(nep, nept, maxit=30, linsolvercreator=None, linsolvertcreator=None, v=None, u=None, tol=1e-12, neigs=5,
                 errmeasure=None, sigma=0.0, gamma=1.0, logger=0, check_error_every=1, scalar_prod="auto"):
    """Infinite bi-Lanczos (src/method_infbilanczos.jl:33-227).  nept is the transposed problem M(conj(lam))^H.  Returns
    (lam, Q, TT): the converged Ritz values, their normalised right Ritz vectors (host n x p) and the tridiagonal matrix of the
    last check.  Raises NoConvergenceException when fewer than `neigs` pairs converged within maxit steps (neigs = inf: run
    maxit steps and return what converged).

    As in the reference:
      - `u` is overwritten by `v` (:55), so the left start vector is nept's solver applied to v;
      - nept's solver is created at sigma while nept's compute_Mlincomb is evaluated at conj(sigma) (:62, :132); the two
        agree for real sigma;
      - `gamma` is accepted and has no effect.
    The solvers come from twosided_linsolvers: one factorisation when nept is recognised as nep's transpose, two otherwise.
    `scalar_prod`: "auto" (K11 where it applies) or "loop" (the reference's compute_Mlincomb loop), an A/B knob."""
    _lib.require_gpu()
    if scalar_prod not in ("auto", "loop"):
        raise ValueError("scalar_prod must be 'auto' or 'loop'")
    n = nep.size(1)
    m = int(maxit)
    sigma = complex(sigma)
    if errmeasure is None:
        errmeasure = DefaultErrmeasure(nep)
    if v is None:
        v = np.random.randn(n)
    u = v                                                      # u = Vector{T}(v), :55
    ls, lst, _ = twosided_linsolvers(nep, nept, sigma, linsolvercreator, linsolvertcreator)
    # Taylor tables: nep's at sigma up to the orders of the last check's scalar product (2m + 2), nept's at conj(sigma) for step 2
    tau = taylor_table(nep, sigma, 2 * m + 2) if _standard_spmf(nep) else None
    taut = taylor_table(nept, sigma.conjugate(), m + 1) if _standard_spmf(nept) else None

    def lrsp(A, B, ma, mb):
        return left_right_scalar_prod(nep, A, B, ma, mb, sigma, tau=tau, mode=scalar_prod)

    qt = lin_solve(lst, to_dev(np.asarray(u, dtype=np.complex128))).reshape(n)
    q = to_dev(np.asarray(v, dtype=np.complex128)).reshape(n)
    z = nep.compute_Mlincomb(sigma, q.reshape(1, n), np.ones(1), 1).reshape(n)
    dense.scal(q, 1.0 / complex(dense.gemv_h(qt.reshape(1, n), z, 1)[0]))

    def blk(cols):
        return torch.zeros((cols, n), dtype=CDT, device="cuda")
    R1, R2, Rt1, Rt2 = blk(m + 1), blk(m + 1), blk(m + 1), blk(m + 1)
    Q0, Q1, Qt0, Qt1 = blk(m), blk(m), blk(m), blk(m)
    Qb = blk(m + 1)                                            # Q_basis
    dense.copy(q, R1[0])
    dense.copy(qt, Rt1[0])
    alpha = np.zeros(m + 2, dtype=np.complex128)
    beta = np.zeros(m + 2, dtype=np.complex128)
    gam = np.zeros(m + 2, dtype=np.complex128)
    lam = np.zeros(m + 1, dtype=np.complex128)
    Q = None
    err = np.zeros(0)
    for k in range(1, m + 1):
        omega = np.conj(lrsp(Rt1, R1, k, k))
        beta[k] = np.sqrt(abs(omega))
        gam[k] = np.conj(omega) / beta[k]
        # steps 11-12
        dense.copy(R1[:k], Q1[:k])
        dense.scal(Q1[:k], 1.0 / beta[k])
        dense.copy(Rt1[:k], Qt1[:k])
        dense.scal(Qt1[:k], 1.0 / np.conj(gam[k]))
        dense.copy(Q1[0], Qb[k - 1])
        # steps 1-2: Z_{k+1}, Z~_{k+1}
        x = lin_solve(ls, _lincomb_taylor(nep, tau, Q1, k, sigma).reshape(1, n), scale=-1.0)
        xt = lin_solve(lst, _lincomb_taylor(nept, taut, Qt1, k, sigma.conjugate()).reshape(1, n), scale=-1.0)
        # steps 3-4: R_{k+1}, R~_{k+1}
        dense.copy(x.reshape(n), R2[0])
        dense.copy(Q1[:k], R2[1:k + 1])
        dense.copy(xt.reshape(n), Rt2[0])
        dense.copy(Qt1[:k], Rt2[1:k + 1])
        if k > 1:
            dense.axpy(-gam[k], Q0[:k - 1], R2[:k - 1])
            dense.axpy(-np.conj(beta[k]), Qt0[:k - 1], Rt2[:k - 1])
        # steps 5-7
        alpha[k + 1] = lrsp(Qt1, R2, k, k + 1)
        dense.axpy(-alpha[k + 1], Q1[:k], R2[:k])
        dense.axpy(-np.conj(alpha[k + 1]), Qt1[:k], Rt2[:k])
        # (the reference zeroes the swapped-out blocks; only columns written in the next step are read again)
        R1, R2 = R2, R1
        Rt1, Rt2 = Rt2, Rt1
        Q0, Q1 = Q1, Q0
        Qt0, Qt1 = Qt1, Qt0
        if k % check_error_every == 0 or k == m:
            omega = lrsp(Rt1, R1, k + 1, k + 1)
            beta[k + 1] = np.sqrt(abs(omega))
            gam[k + 1] = np.conj(omega) / beta[k + 1]
            # spdiagm(-1 => beta0[1:k], 0 => alpha0[1:k], 1 => gamma0[1:k]) is (k+1) x (k+1), its last diagonal entry 0
            TT = np.zeros((k + 1, k + 1), dtype=np.complex128)
            r = np.arange(k)
            TT[r + 1, r] = beta[2:k + 2]
            TT[r, r] = alpha[2:k + 2]
            TT[r, r + 1] = gam[2:k + 2]
            ev, Z = np.linalg.eig(TT)
            with np.errstate(divide="ignore", invalid="ignore"):
                lam = sigma + 1.0 / ev
            QT = dense.gemm_ts(Qb, Z, rowmajor=True)            # Q_basis[:, 1:k+1] * Z, (n, k+1) row-major
            err = np.asarray(estimate_errors(errmeasure, lam, QT), dtype=float)
            conv = int(np.sum(err < tol))
            if logger:
                print("infbilanczos k=%d: %d of %d Ritz pairs below tol" % (k, conv, len(lam)))
            idx = np.argsort(err[:k], kind="stable")
            err = err[idx]
            if conv >= neigs or k == m:
                nr = int(min(len(lam), neigs, conv))
                lam = lam[idx[:nr]]
                Q = QT.cpu().numpy()[:, idx[:nr]]
                Q = Q / np.linalg.norm(Q, axis=0, keepdims=True) if nr > 0 else Q
                if conv >= neigs or neigs == np.inf:
                    return lam, Q, TT
    raise NoConvergenceException(lam, Q, err, "Number of iterations exceeded. maxit=%d." % maxit)
