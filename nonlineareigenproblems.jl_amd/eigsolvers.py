"""The EigSolver layer (src/LinSolvers.jl:313-469): linear eigensolvers for A x = d B x behind `eig_solve`.

  EigenEigSolver     dense LAPACK on the host (small dense linear algebra on the host, as projection.py and _hosteig.py do)
  ArnoldiEigSolver   sparse pencils: shift-and-invert Krylov-Schur on the device.  The pencil is an SPMF handle with two coefficient
                     rows (cA, cB), C = tau B - A is a DeviceLU, the expansion is nep_arnoldi_steps (K1, K5, K6 per step, one
                     host wait per restart cycle), the restart compresses the basis in place with nep_basis_rotate (K13), the Ritz
                     vectors are one nep_gemm_ts (K7) and the true pencil residuals one nep_resid_batch_dev (K2).  The host does
                     the arithmetic on the Rayleigh matrix (at most 128 x 128): its ordered Schur form and the residual estimates.
  DefaultEigSolver   sparse -> Arnoldi, dense -> Eigen

The reference's ArnoldiEigSolver calls `partialschur(C^-1 B, nev, tol=1e-10, which=LM())` of ArnoldiMethod.jl (:390-416); this is
the same method (G. W. Stewart, A Krylov-Schur algorithm for large eigenproblems, SIMAX 23 (2001)) written from the mathematics.
"""
import ctypes as C
import time

import numpy as np
import scipy.linalg as sla
import scipy.sparse as sp
import torch

from . import _lib, funcs
from ._lib import lib, check, hptr, c_vp
from .exceptions import NoConvergenceException

KS_TOL = 1e-10            # partialschur(..., tol=1e-10)
KS_RESTARTS = 200
KS_MAXDIM = 128           # nep_basis_rotate's limit


class EigSolver:
    """base class: a subclass is constructed as T(A, B) (or T(A)) and answers eig_solve(nev=, target=) with (values, vectors)"""

    def eig_solve(self, **kw):
        raise NotImplementedError


def eig_solve(solver, **kw):
    """eig_solve(solver; nev, target): the `nev` eigenvalues of the solver's pencil nearest `target` and their eigenvectors"""
    return solver.eig_solve(**kw)


def _dense(A):
    return np.asarray(A.toarray() if sp.issparse(A) else A)


class EigenEigSolver(EigSolver):
    """:331-359: scipy.linalg.eig of (A, B) (B = None: the standard problem), sorted by |target - d|"""

    def __init__(self, A, B=None):
        self.A, self.B = A, B

    def eig_solve(self, nev=1, target=0):
        D, V = sla.eig(_dense(self.A), None if self.B is None else _dense(self.B))
        order = np.argsort(np.abs(target - D), kind="stable")
        return D[order][:nev], V[:, order][:, :nev]


class ArnoldiEigSolver(EigSolver):
    """:376-416 on the device.  `info` describes the last call: restarts, steps, rotations (calls of K13), breakdown, the route
    of the factorisation, the true residuals ||(A - d_i B) x_i|| of the returned pairs (unit vectors) and the wall time."""

    def __init__(self, A, B=None):
        from .nep import SPMF_NEP
        if not sp.issparse(A):
            raise TypeError("ArnoldiEigSolver needs a sparse matrix (EigenEigSolver solves dense pencils)")
        n = A.shape[0]
        self.A, self.B = A, B
        Bm = sp.identity(n, format="csc") if B is None else sp.csc_matrix(B)
        # the pencil as a two-term SPMF: one device handle, one union pattern (every shifted matrix tau B - A of this pencil,
        # and of a later pencil on the same pattern, has the same index arrays: the pattern's factorisation plan applies)
        self._spmf = SPMF_NEP([sp.csc_matrix(A), Bm], [funcs.one(), funcs.one()])
        self.cA = np.array([1.0, 0.0], dtype=np.complex128)
        self.cB = np.array([0.0, 1.0], dtype=np.complex128)
        self._terms_first = False
        self.n = n
        self.info = {}

    @classmethod
    def from_nep(cls, nep, lam):
        """the pencil (M(lam), M'(lam)) of a pure sparse SPMF NEP on the NEP's own device handle: cA_t = f_t(lam),
        cB_t = f_t'(lam); neither matrix is assembled"""
        if not cls.accepts(nep):
            raise TypeError("ArnoldiEigSolver.from_nep needs a pure sparse SPMF NEP")
        self = cls.__new__(cls)
        d = np.array([f.derivs(lam, 2)[:2] for f in nep.get_fv()], dtype=np.complex128)
        self.A = self.B = None
        self._spmf = nep
        self.cA, self.cB = d[:, 0].copy(), d[:, 1].copy()
        self._terms_first = True
        self.n = nep.n
        self.info = {}
        return self

    @classmethod
    def from_terms(cls, spmf, cA, cB):
        """the pencil (sum_t cA_t A_t, sum_t cB_t A_t) on the device handle of the pure sparse SPMF `spmf`, the two coefficient
        rows given directly (sgiter: the terms [A_1..A_m, I] with cA = [f_t(lam).., 0], cB = [0.., 1]).  The rows may be replaced
        between calls of eig_solve_dev; neither matrix is assembled"""
        if not cls.accepts(spmf):
            raise TypeError("ArnoldiEigSolver.from_terms needs a pure sparse SPMF NEP")
        cA = np.array(cA, dtype=np.complex128).reshape(-1)
        cB = np.array(cB, dtype=np.complex128).reshape(-1)
        if len(cA) != len(spmf.get_fv()) or len(cB) != len(cA):
            raise ValueError("ArnoldiEigSolver.from_terms: one coefficient per term is needed in each row")
        self = cls.__new__(cls)
        self.A = self.B = None
        self._spmf = spmf
        self.cA, self.cB = cA, cB
        self._terms_first = True
        self.n = spmf.n
        self.info = {}
        return self

    @staticmethod
    def accepts(nep):
        """a pure SPMF (nep.pure_spmf) with sparse matrices"""
        from .nep import pure_spmf
        return (pure_spmf(nep, "Mder", "Mlincomb") and hasattr(nep, "aligned_terms_dev")
                and nep.issparse() and nep._aligned_terms() is not None)

    # ---- C = tau B - A = sum_t (tau cB_t - cA_t) A_t
    def _factor(self, target, expected_solves):
        from ._devicelu import DeviceLU, lu_from_term_coeffs
        cC = target * self.cB - self.cA
        if self._terms_first:
            lu = lu_from_term_coeffs(self._spmf, cC, dict(expected_solves=expected_solves))
            if lu is not None:
                return lu
        indptr, indices, D = self._spmf._aligned_terms()
        Cm = sp.csc_matrix((np.einsum("ij,j->i", D, cC), indices, indptr), shape=(self.n, self.n))
        return DeviceLU(Cm, expected_solves=expected_solves)

    def eig_solve(self, nev=6, target=0, **kw):
        D, Xd = self.eig_solve_dev(nev=nev, target=target, **kw)
        from .nep import to_host
        return D, to_host(Xd)

    def eig_solve_dev(self, nev=6, target=0, v0=None, tol=KS_TOL, _mindim=None, _maxdim=None, _orth=0):
        """(d, X): X the eigenvector block as a device (nev, n) tensor (unit columns)"""
        from .nep import CDT, stream_ptr, to_dev
        _lib.require_gpu()
        t0 = time.perf_counter()
        n = self.n
        nev = int(nev)
        if nev < 1 or nev > n:
            raise ValueError("ArnoldiEigSolver: 1 <= nev <= n is required (nev = %d, n = %d)" % (nev, n))
        mindim = min(max(10, nev), n) if _mindim is None else int(_mindim)
        maxdim = min(max(20, 2 * nev), n) if _maxdim is None else int(_maxdim)
        if maxdim > KS_MAXDIM or not (nev <= mindim <= maxdim <= n):
            raise ValueError("ArnoldiEigSolver: subspace sizes nev <= mindim <= maxdim <= min(n, %d) are required "
                             "(nev = %d, mindim = %d, maxdim = %d)" % (KS_MAXDIM, nev, mindim, maxdim))
        target = complex(target)
        dev = self._spmf.dev
        lu = self._factor(target, expected_solves=200)
        route = (getattr(lu, "strategy", None) or {}).get("numeric", "host")
        # ---- device objects: the basis, the coefficient row of B, the coefficient block and its pinned copy
        if v0 is None:
            v0 = np.random.default_rng(20011).standard_normal(n)
        V = torch.zeros((maxdim + 1, n), dtype=CDT, device="cuda")
        if torch.is_tensor(v0):
            V[0].copy_(v0.reshape(-1))
        else:
            V[0].copy_(to_dev(np.asarray(v0, dtype=np.complex128))[0])
        nrm0 = float(torch.linalg.vector_norm(V[0]))
        if not (nrm0 > 0 and np.isfinite(nrm0)):
            raise ValueError("ArnoldiEigSolver: the start vector must be finite and non-zero")
        V[0].mul_(1.0 / nrm0)
        cBd = torch.from_numpy(self.cB.copy()).to("cuda")
        work = torch.empty(n, dtype=CDT, device="cuda")
        ld = maxdim + 4
        Sd = torch.zeros((maxdim, ld), dtype=CDT, device="cuda")
        Sh = torch.zeros((maxdim, ld), dtype=CDT, pin_memory=True)
        rows = Sh.numpy()
        h = c_vp()
        check(lib.nep_arnoldi_create(dev.h, lu.h, n, maxdim, c_vp(V.data_ptr()), n, c_vp(cBd.data_ptr()), c_vp(work.data_ptr()),
                                     c_vp(Sd.data_ptr()), c_vp(Sh.data_ptr()), int(_orth), C.byref(h)))
        info = dict(restarts=0, steps=0, rotations=0, breakdown=False, factorization=route, mindim=mindim, maxdim=maxdim)
        S = np.zeros((maxdim + 1, maxdim), dtype=np.complex128)
        k = 0
        try:
            while True:
                check(lib.nep_arnoldi_steps(h, k, maxdim - k, stream_ptr()))
                check(lib.nep_arnoldi_wait(h, maxdim - 1))                     # the one wait of this cycle
                m = maxdim
                for j in range(k, maxdim):
                    S[:j + 1, j] = rows[j, :j + 1]
                    S[j + 1, j] = rows[j, j + 1].real
                    info["steps"] += 1
                    # the new vector lies in span(V) (an invariant subspace): the breakdown bit, or, in a DGKS step, a last
                    # pass that still wanted another one ("twice is enough")
                    if int(rows[j, j + 2].imag) & (3 if _orth == 0 else 2):
                        S[j + 1, j] = 0.0
                        m = j + 1
                        info["breakdown"] = True
                        break
                Bm = S[:m, :m]
                beta = S[m, m - 1].real
                theta, Y = sla.eig(Bm)
                Y = Y / np.linalg.norm(Y, axis=0)
                order = np.argsort(-np.abs(theta), kind="stable")
                theta, Y = theta[order], Y[:, order]
                est = beta * np.abs(Y[m - 1, :])                              # |b^H y|, b^H = beta e_m^T
                want = min(nev, m)
                conv = est[:want] <= tol * np.abs(theta[:want])
                if conv.all() or info["breakdown"] or info["restarts"] >= KS_RESTARTS:
                    break
                # ---- restart: ordered Schur form, keep the p dominant Schur vectors, compress the basis in place
                p = min(mindim, m - 1)
                thr = np.sort(np.abs(theta))[::-1][p - 1] * (1.0 - 1e-12)
                T, Z, sdim = sla.schur(Bm, output="complex", sort=lambda x: abs(x) >= thr)
                p = int(min(max(sdim, 1), m - 1))
                Q = np.asfortranarray(Z[:, :p])
                check(lib.nep_basis_rotate(c_vp(V.data_ptr()), n, n, m, p, hptr(Q), m, 1, stream_ptr()))
                S[:] = 0.0
                S[:p, :p] = T[:p, :p]
                S[p, :p] = beta * Z[m - 1, :p]
                k = p
                info["restarts"] += 1
                info["rotations"] += 1
            # ---- Ritz vectors, true residuals, back-transformation d = tau - 1 / theta
            keep = np.flatnonzero(conv)                                       # the converged pairs among the wanted ones
            theta, Y, est = theta[keep], Y[:, keep], est[keep]
            nret = len(keep)
            from .dense import gemm_ts
            d = target - 1.0 / theta if len(theta) else np.zeros(0, dtype=np.complex128)
            if len(theta):
                QT = gemm_ts(V, np.asfortranarray(Y), rowmajor=True, k=m, rows=n, ldz=n)
                F = np.asfortranarray(self.cA[:, None] - self.cB[:, None] * d[None, :])
                rn, qn, _ = dev.resid_batch_async(F, QT).get()
                Xd = (QT.t() / torch.from_numpy(qn).to("cuda")[:, None]).contiguous()
                info["residuals"] = rn / qn
                if info["breakdown"]:
                    # beta was taken as zero on the word of the orthogonalisation, so the estimates say nothing: the pairs
                    # stand on their true residuals, against what the stopping rule guarantees ((A - d B) x = -C r / theta)
                    ok = np.flatnonzero(info["residuals"] <= 2 * tol * float(lu.normA))
                    theta, est, d, nret = theta[ok], est[ok], d[ok], len(ok)
                    Xd = Xd[torch.from_numpy(ok).to("cuda")].contiguous()
                    info["residuals"] = info["residuals"][ok]
            else:
                Xd = torch.zeros((0, n), dtype=CDT, device="cuda")
                info["residuals"] = np.zeros(0)
        finally:
            torch.cuda.current_stream().synchronize()
            lib.nep_arnoldi_destroy(h)
        info.update(theta=theta, estimates=est, nconv=nret, wall=time.perf_counter() - t0,
                    device_factorized=bool(getattr(lu, "device_factorized", False)))
        self.info = info
        if nret < nev:
            from .nep import to_host
            raise NoConvergenceException(d, to_host(Xd), info["residuals"],
                                         "ArnoldiEigSolver: %d of %d eigenpairs converged after %d restarts"
                                         % (nret, nev, info["restarts"]))
        return d, Xd


class DefaultEigSolver(EigSolver):
    """:429-469: sparse -> ArnoldiEigSolver, dense -> EigenEigSolver; the default nev is the size of the problem"""

    def __init__(self, A, B=None):
        self.subsolver = ArnoldiEigSolver(A, B) if sp.issparse(A) else EigenEigSolver(A, B)

    def eig_solve(self, nev=None, target=0, **kw):
        if nev is None:
            nev = self.subsolver.A.shape[0]
        return self.subsolver.eig_solve(nev=nev, target=target, **kw)
