"""The record of the convergence checks of the Arnoldi drivers (iar, tiar, iar_chebyshev): src/method_iar.jl:133-175,
src/method_tiar.jl:209-252.  One check of step k has Ritz values `lam`, a Ritz block `QT` and error estimates `e`; the record
sorts the errors into row k-1 of the caller's `err`, counts the converged pairs and keeps the pairs a return or a
NoConvergenceException carries."""
import numpy as np

from . import dense
from .exceptions import NoConvergenceException
from .nep import to_host


class RitzChecks:
    def __init__(self, m, tol, neigs, errhist, err):
        self.m, self.tol, self.neigs, self.errhist, self.err = m, tol, neigs, errhist, err
        self.lam = np.zeros(0, dtype=np.complex128); self.QT = None; self.idx = np.zeros(0, dtype=int)
        self.conv_eig = 0; self.k_checked = 0

    def record(self, k, lam, QT, e):
        ne = min(len(e), self.err.shape[1])
        conv = int(np.sum(e < self.tol))
        idx = np.argsort(e, kind="stable")
        self.err[k - 1, :ne] = e[idx][:ne]
        if self.errhist is not None:
            self.errhist.append(self.err[k - 1, :ne].copy())
        if k == self.m or conv >= self.neigs:
            nrof = int(min(len(lam), self.neigs))
            lam = lam[idx[:nrof]]
            idx = idx[:nrof]
        self.lam, self.QT, self.idx, self.k_checked = lam, QT, idx, k
        self.conv_eig = conv          # last: a thread that sees the count reach neigs finds the pairs that go with it

    def finish(self, k, maxit, hint, host=None):
        """the way out of a driver whose last check was step k: NoConvergenceException with the best pairs (`hint` is appended
        to its message when fewer than 3 converged), or (lam, Q) of the converged ones -- Q on the device, or through `host`"""
        lam, idx = self.lam, self.idx
        if self.conv_eig < self.neigs and self.neigs != np.inf:
            Q = to_host(dense.rowmajor_to_cols(self.QT, idx[:len(lam)])) if self.QT is not None else None
            msg = "Number of iterations exceeded. maxit=%d." % maxit
            if self.conv_eig < 3:
                msg += hint
            raise NoConvergenceException(lam, Q, self.err[k - 1, :len(lam)], msg)
        nc = min(len(lam), self.conv_eig)
        Qd = dense.rowmajor_to_cols(self.QT, idx[:nc])          # (nc, n) = column-major n x nc
        return lam[:nc], (Qd if host is None else host(Qd))
