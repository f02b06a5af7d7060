"""The NEP of a time-periodic delay-differential equation x'(t) = A(t) x(t) + B(t) x(t - tau) (src/gallery_extra/periodic_dde.jl):
M(lam) = Phi_lam(tau) - I, where Phi_lam comes from N classical Runge-Kutta steps of a matrix ODE over one period.  The sweep
runs in one launch of K15 (csrc/pdde.hip, nep_pdde_*) for a whole batch of shifts and columns.

compute_MM(S, V) is itself the ODE Y' = A(t) Y + B(t) Y exp(-tau S) - Y S, Y(0) = V, with the result Y(tau) - V
(periodic_dde.jl:203-218).  With S a Jordan block it gives every derivative exactly, as the derivative of the discrete
Runge-Kutta map: compute_Mder(lam, i) works for any i <= 7 (the reference differences M for i = 1 and stops there), and
compute_Mlincomb is one system of k + startder columns.

The device takes A and B as sums of fixed matrices with scalar functions of t, A(t) = sum_i alpha_i(t) A_i.  Callables of t (the
reference's form) are sampled at the 2N + 1 half-step times and split by an SVD of the sample matrix into at most 8 such terms.
"""
import ctypes as C
import math

import numpy as np
import scipy.linalg
import scipy.sparse as sp
import torch

from . import _lib
from ._lib import lib, check, hptr, c_vp, c_i64
from .nep import NEP, CDT, is_dev, to_dev, to_host, stream_ptr

PMAX = 8            # columns of one system (nep_pdde_info[3])
RANK_MAX = 8        # terms a callable may split into
RANK_TOL = 1e-13
SAMPLE_WORDS = 1 << 25   # complex words of the sample matrix of a callable (512 MiB)


def _sample(fun, times, n):
    X = np.empty((len(times), n * n), dtype=np.complex128)
    for s, t in enumerate(times):
        M = fun(float(t))
        M = M.toarray() if sp.issparse(M) else np.asarray(M)
        X[s] = np.asarray(M, dtype=np.complex128).reshape(n, n).reshape(-1, order="F")
    return X


def terms_from_callable(fun, times, n):
    """(matrices (m, n, n), table (len(times), m)) with fun(t_s) = sum_i table[s, i] matrices[i]: the right singular vectors of
    the sample matrix are the terms and U Sigma the tables.  ValueError when more than RANK_MAX singular values exceed RANK_TOL
    times the largest.  The sample matrix is dense, len(times) x n^2 complex, and is decomposed at every call (construction and every
    assignment to N): 1.3 GB and minutes at n = 200, N = 1000, so beyond SAMPLE_WORDS complex words a ValueError asks for the term
    form, which costs nothing of the kind."""
    if len(times) * n * n > SAMPLE_WORDS:
        raise ValueError("PeriodicDDE_NEP: splitting a callable takes the SVD of a %d x %d sample matrix (%.1f GB); give the matrix "
                         "function in term form, a list [(A_i, alpha_i)] of fixed matrices and scalar functions of t"
                         % (len(times), n * n, len(times) * n * n * 16 / 1e9))
    X = _sample(fun, times, n)
    U, sv, Vh = np.linalg.svd(X, full_matrices=False)
    rank = max(1, int(np.sum(sv > RANK_TOL * sv[0]))) if sv[0] > 0 else 1
    if rank > RANK_MAX:
        raise ValueError("PeriodicDDE_NEP: the samples of the callable have numerical rank %d > %d; give the matrix function in "
                         "term form, a list [(A_i, alpha_i)] of fixed matrices and scalar functions of t" % (rank, RANK_MAX))
    mats = np.stack([Vh[i].reshape(n, n, order="F") for i in range(rank)])
    return mats, np.ascontiguousarray(U[:, :rank] * sv[:rank])


def _terms(spec, times, n, what):
    """(matrices (m, n, n) complex, table (len(times), m) complex) of a term list or a callable"""
    if callable(spec):
        return terms_from_callable(spec, times, n)
    spec = list(spec)
    if len(spec) < 1:
        raise ValueError("PeriodicDDE_NEP: %s needs at least one term" % what)
    mats = np.empty((len(spec), n, n), dtype=np.complex128)
    tab = np.empty((len(times), len(spec)), dtype=np.complex128)
    for i, (M, f) in enumerate(spec):
        M = M.toarray() if sp.issparse(M) else np.asarray(M)
        if M.shape != (n, n):
            raise ValueError("PeriodicDDE_NEP: term %d of %s is %r, not %d x %d" % (i, what, M.shape, n, n))
        mats[i] = M
        tab[:, i] = [f(float(t)) for t in times] if callable(f) else complex(f)
    return mats, tab


def _size_of(spec):
    if callable(spec):
        M = spec(0.0)
        return (M.shape if sp.issparse(M) else np.asarray(M).shape)[0]
    M = list(spec)[0][0]
    return M.shape[0]


def jordan_pair(lam, p, tau):
    """S = J_p(lam) (ones above the diagonal) and E = exp(-tau S) = e^(-tau lam) Toeplitz((-tau)^k / k!)"""
    lam = complex(lam)
    S = lam * np.eye(p, dtype=np.complex128) + np.diag(np.ones(p - 1), 1)
    E = np.zeros((p, p), dtype=np.complex128)
    e0 = np.exp(-tau * lam)
    for k in range(p):
        E += np.diag(np.full(p - k, e0 * (-tau) ** k / math.factorial(k)), k)
    return S, E


class PeriodicDDE_NEP(NEP):
    """periodic_dde.jl:51-66 (the ODE variant) on the device.  A, B: term lists [(A_i, alpha_i)] (A_i an ndarray or a scipy sparse
    matrix, alpha_i a callable of t or a number) or callables of t returning the matrix.  N (Runge-Kutta steps per period) can be
    set afterwards, as in the reference; the tables are sampled again and the device handle is rebuilt."""

    def __init__(self, A, B, tau, N=1000):
        self.A, self.B, self.tau = A, B, float(tau)
        self.n = int(_size_of(A))
        self.h = None
        self._N = None
        self.N = N

    # ---- set-up
    @property
    def N(self):
        return self._N

    @N.setter
    def N(self, N):
        N = int(N)
        if N < 1:
            raise ValueError("PeriodicDDE_NEP: N must be at least 1")
        times = np.arange(2 * N + 1) * (self.tau / (2 * N))
        self.A_terms, self.alpha = _terms(self.A, times, self.n, "A")
        self.B_terms, self.beta = _terms(self.B, times, self.n, "B")
        self._N = N
        self._drop_handle()

    def _drop_handle(self):
        if getattr(self, "h", None):
            lib.nep_pdde_destroy(self.h)
        self.h = None

    def __del__(self):
        try:
            self._drop_handle()
        except Exception:
            pass

    def _handle(self):
        if self.h is None:
            _lib.require_gpu()
            # (m, n, n) C-order of the transposes = m column-major matrices one after the other
            Ad = np.ascontiguousarray(self.A_terms.transpose(0, 2, 1))
            Bd = np.ascontiguousarray(self.B_terms.transpose(0, 2, 1))
            al, be = np.ascontiguousarray(self.alpha), np.ascontiguousarray(self.beta)
            h = c_vp()
            check(lib.nep_pdde_create(self.n, len(Ad), len(Bd), hptr(Ad), hptr(Bd), self._N, self.tau, hptr(al), hptr(be), C.byref(h)))
            self.h = h
            info = (c_i64 * 4)()
            check(lib.nep_pdde_info(self.h, info))
            self.device_bytes = int(info[2])
        return self.h

    def issparse(self):
        return False

    # ---- the sweep
    def _mm(self, S, E, Vd):
        """S, E: (nsys, p, p) host; Vd: device (nsys * p, n) = nsys column-major n x p blocks; returns the same shape"""
        nsys, p = S.shape[0], S.shape[1]
        n = self.n
        Sd = np.ascontiguousarray(np.asarray(S, dtype=np.complex128).transpose(0, 2, 1))
        Ed = np.ascontiguousarray(np.asarray(E, dtype=np.complex128).transpose(0, 2, 1))
        assert Vd.dtype == CDT and Vd.is_contiguous() and Vd.shape == (nsys * p, n)
        out = torch.empty((nsys * p, n), dtype=CDT, device="cuda")
        check(lib.nep_pdde_mm(self._handle(), nsys, p, hptr(Sd), hptr(Ed), c_vp(Vd.data_ptr()), n, n * p, c_vp(out.data_ptr()), n,
                              n * p, stream_ptr()))
        return out

    def compute_MM(self, S, V):
        """Y(tau) - V of the matrix ODE (periodic_dde.jl:203-218) for a p x p matrix S, p <= 8, and an n x p block V.  NumPy in ->
        NumPy out; device tensor (p, n) in -> device tensor out"""
        S = np.atleast_2d(np.asarray(S, dtype=np.complex128))
        p = S.shape[0]
        if p > PMAX:
            raise ValueError("PeriodicDDE_NEP.compute_MM: %d columns, the device sweep takes at most %d" % (p, PMAX))
        E = np.array([[np.exp(-self.tau * S[0, 0])]]) if p == 1 else scipy.linalg.expm(-self.tau * S)
        host = not is_dev(V)
        Vd = to_dev(V) if host else V.reshape(p, -1)
        if Vd.shape[0] != p:
            raise ValueError("compute_MM: V has %d columns, S is %d x %d" % (Vd.shape[0], p, p))
        out = self._mm(S[None], E[None], Vd.contiguous())
        return to_host(out) if host else out

    def compute_Mder_dev(self, lams, der=0):
        """the block (len(lams), n, n) of M^(der)(lam_l) on the device, [l] = the TRANSPOSED matrix in torch's row-major view
        (the library writes column-major); one nep_pdde_mder call"""
        la = np.ascontiguousarray(np.atleast_1d(lams), dtype=np.complex128)
        if der >= PMAX:
            raise ValueError("PeriodicDDE_NEP: derivative %d needs %d columns, the device sweep takes at most %d" % (der, der + 1, PMAX))
        n = self.n
        out = torch.empty((len(la), n, n), dtype=CDT, device="cuda")
        check(lib.nep_pdde_mder(self._handle(), len(la), hptr(la), int(der), c_vp(out.data_ptr()), n, n * n, stream_ptr()))
        return out.transpose(1, 2)

    def compute_Mder(self, lam, i=0):
        """M^(i)(lam), i <= 7, as a host ndarray"""
        return np.ascontiguousarray(self.compute_Mder_dev([lam], i)[0].cpu().numpy())

    def compute_Mder_batch(self, lams):
        """M(lam_b) of several shifts from ONE launch, as a host array (B, n, n)"""
        return np.ascontiguousarray(self.compute_Mder_dev(lams, 0).cpu().numpy())

    def compute_Mlincomb(self, lam, V, a=None, startder=0):
        """sum_j a_j M^(j + startder)(lam) v_j as ONE system of p = k + startder columns: S = J_p(lam), column p-1-i of the block is
        i! a_(i-sd) v_(i-sd) (zero for i < sd), and the last column of the result is the sum.  NumPy in -> NumPy out; device tensor
        ((k, n) block or (n,) vector) in -> device tensor out.  V is not modified."""
        host = not is_dev(V)
        Vd = to_dev(V) if host else (V if V.dim() == 2 else V.reshape(1, -1))
        k = Vd.shape[0]
        a = np.ones(k, dtype=np.complex128) if a is None else np.asarray(a, dtype=np.complex128)
        if len(a) != k:
            raise ValueError("length of a must equal the number of columns of V")
        p = k + int(startder)
        if p > PMAX:
            raise ValueError("PeriodicDDE_NEP.compute_Mlincomb: k + startder = %d columns, the device sweep takes at most %d; for iar / "
                             "tiar interpolate first (ChebPEP(nep, k, a, b) or interpolate) and run them on the polynomial" % (p, PMAX))
        n = self.n
        W = torch.zeros((p, n), dtype=CDT, device="cuda")
        for j in range(k):
            i = j + startder
            if a[j] != 0:
                W[p - 1 - i] = Vd[j, :n] * complex(math.factorial(i) * a[j])
        S, E = jordan_pair(lam, p, self.tau)
        z = self._mm(S[None], E[None], W)[p - 1]
        return to_host(z.reshape(1, -1))[:, 0] if host else z

    def resid_norms(self, lams, QT):
        """(||M(lam_s) q_s||, ||q_s||, None) for the columns of the row-major block QT: one nep_pdde_mm call of k systems, p = 1"""
        from . import dense
        la = np.ascontiguousarray(lams, dtype=np.complex128)
        k = len(la)
        cols = dense.rowmajor_to_cols(QT, np.arange(k, dtype=np.int32))          # (k, n') column-major
        Q = cols[:, :self.n].contiguous()
        S = la.reshape(k, 1, 1)
        Y = self._mm(S, np.exp(-self.tau * S), Q)
        nr = np.empty(k); nq = np.empty(k)
        check(lib.nep_colnorms(self.n, k, c_vp(Y.data_ptr()), self.n, hptr(nr), stream_ptr()))
        check(lib.nep_colnorms(self.n, k, c_vp(Q.data_ptr()), self.n, hptr(nq), stream_ptr()))
        return nr, nq, None
