"""Matrix-free restarted GMRES as a linear solver (src/LinSolvers.jl:171-188, src/LinSolverCreators.jl:124-145)."""
import numpy as np
import torch

from ._env import env_str
from ._lib import lib, check, c_vp
from .linsolvers import LinSolver, LinSolverCreator        # (the base classes; linsolvers.py imports this module below them)
from .nep import CDT, to_dev, stream_ptr


class GMRESLinSolver(LinSolver):
    """src/LinSolvers.jl:171-188: matrix-free restarted GMRES on v -> compute_Mlincomb(nep, lam, v), i.e. every
    iteration is one K1 call (folded single-vector SpMV) + one K6 orthogonalisation (IterativeSolvers' default
    ModifiedGramSchmidt) on the device; only the (restart+1) x restart Hessenberg / Givens data live on the host.
    kwargs mirror IterativeSolvers.gmres!: Pl (left preconditioner: a vector/diagonal matrix d meaning Pl \\ r = r ./ d,
    or a callable acting on a device vector), reltol (alias tol), abstol, restart, maxiter."""

    def __init__(self, nep, lam, kwargs=None):
        kwargs = dict(kwargs or {})
        self.nep, self.lam = nep, lam
        self.n = nep.size(1)
        self.restart = int(kwargs.get("restart", min(20, self.n)))
        self.maxiter = int(kwargs.get("maxiter", self.n))
        self.reltol = kwargs.get("reltol", kwargs.get("tol", None))
        self.abstol = float(kwargs.get("abstol", 0.0))
        from . import dense as _d
        # IterativeSolvers' gmres orthogonalises with ModifiedGramSchmidt by default (orth_meth keyword)
        self.orth = {"mgs": _d.MGS, "cgs": _d.CGS, "dgks": _d.DGKS}[str(kwargs.get("orth_meth", env_str("NEP_GMRES_ORTH", "mgs"))).lower()]
        Pl = kwargs.get("Pl", None)
        self._Pl_call = None
        self._Pl_inv = None
        if Pl is not None:
            if callable(Pl):
                self._Pl_call = Pl
            else:
                d = np.asarray(Pl) if np.ndim(Pl) == 1 else (Pl.diagonal() if hasattr(Pl, "diagonal") else np.diag(np.asarray(Pl)))
                self._Pl_inv = to_dev(1.0 / np.asarray(d, dtype=np.complex128))[0]
        self.iterations = 0
        self.fused_step = None          # optional callable (v, w): w = Pl^{-1} A v  (e.g. a captured hipGraph)

    def _prec(self, r):
        if self._Pl_inv is not None:
            check(lib.nep_hadamard(self.n, 1, c_vp(r.data_ptr()), self.n, c_vp(self._Pl_inv.data_ptr()), self.n, stream_ptr()))
        elif self._Pl_call is not None:
            out = self._Pl_call(r)
            if out is not None and out.data_ptr() != r.data_ptr():
                from . import dense
                dense.copy(out, r, self.n)
        return r

    def solve_dev(self, b, out=None, scale=1.0, tol=None):
        from . import dense
        n, m = self.n, self.restart
        if b.dim() == 2 and b.shape[0] > 1:
            X = torch.empty_like(b) if out is None else out
            for j in range(b.shape[0]):
                self.solve_dev(b[j], out=X[j], scale=scale, tol=tol)
            return X
        reltol = tol if tol else (self.reltol if self.reltol is not None else np.sqrt(np.finfo(float).eps))
        bvec = b.reshape(n)
        x = torch.zeros(n, dtype=CDT, device="cuda")
        V = torch.empty((m + 1, n), dtype=CDT, device="cuda")
        r = torch.empty(n, dtype=CDT, device="cuda")
        dense.copy(bvec, r, n); self._prec(r)
        beta = dense.nrm2(r)
        tolabs = max(reltol * beta, self.abstol)
        its = 0
        # Arnoldi columns are orthogonalised on the device without reading anything back (nep_orth_dev: DGKS / CGS); the
        # Givens update of column j runs on the host while the device already works on column j+1, so the only cost of the
        # convergence test is ONE speculative iteration at the end of a cycle instead of a device stall in every iteration
        # (waveguide, n = 1e6: 3300 stalls of 50-100 us per tiar run).  MGS keeps the step-synchronous loop.
        pipelined = self.orth in (dense.DGKS, dense.CGS)
        if pipelined:
            Hdev = torch.zeros((m, m + 3), dtype=CDT, device="cuda")
            Hpin = torch.zeros((m, m + 3), dtype=CDT).pin_memory()
            Hnp = Hpin.numpy()
        while beta > tolabs and its < self.maxiter:
            dense.copy(r, V[0], n); dense.scal(V[0], 1.0 / beta, n)
            H = np.zeros((m + 1, m), dtype=np.complex128)
            cs = np.zeros(m, dtype=np.complex128); sn = np.zeros(m, dtype=np.complex128)
            g = np.zeros(m + 1, dtype=np.complex128); g[0] = beta
            j_done = 0

            def givens(j, h, hb):
                """column j of H (h: j+1 entries, hb: the subdiagonal) through the rotations; True = cycle finished"""
                nonlocal its, j_done
                H[:j + 1, j] = h; H[j + 1, j] = hb
                for i in range(j):                       # apply previous Givens rotations
                    t = cs[i] * H[i, j] + sn[i] * H[i + 1, j]
                    H[i + 1, j] = -np.conj(sn[i]) * H[i, j] + np.conj(cs[i]) * H[i + 1, j]
                    H[i, j] = t
                a_, b_ = H[j, j], H[j + 1, j]
                d = np.sqrt(abs(a_) ** 2 + abs(b_) ** 2)
                cs[j] = a_ / d; sn[j] = b_ / d
                cs[j] = np.conj(cs[j]); sn[j] = np.conj(sn[j])
                H[j, j] = d; H[j + 1, j] = 0.0
                g[j + 1] = -np.conj(sn[j]) * g[j]
                g[j] = cs[j] * g[j]
                its += 1; j_done = j + 1
                return abs(g[j + 1]) <= tolabs or its >= self.maxiter

            def apply_op(j):
                w = V[j + 1]
                if self.fused_step is not None:            # w = Pl^{-1} A v as one pre-recorded launch sequence
                    self.fused_step(V[j], w)
                else:
                    dense.copy(self.nep.compute_Mlincomb(self.lam, V[j].reshape(1, n)), w, n)
                    self._prec(w)
                return w

            if pipelined:
                evs = [None] * m
                done = False
                for j in range(m):
                    w = apply_op(j)
                    dense.orthogonalize_and_normalize_dev(V, w, j + 1, Hdev[j], rows=n, ldv=n, method=self.orth)
                    Hpin[j, :j + 3].copy_(Hdev[j, :j + 3], non_blocking=True)
                    evs[j] = torch.cuda.Event(); evs[j].record()
                    if j >= 1:                             # column j-1 while the device computes column j
                        evs[j - 1].synchronize()
                        row = Hnp[j - 1]
                        if givens(j - 1, row[:j].copy(), row[j].real):
                            done = True
                            break
                if not done and j_done < m and its < self.maxiter:
                    jl = j_done
                    evs[jl].synchronize()
                    row = Hnp[jl]
                    givens(jl, row[:jl + 1].copy(), row[jl + 1].real)
            else:
                for j in range(m):
                    w = apply_op(j)
                    h, hb, _ = dense.orthogonalize_and_normalize(V, w, j + 1, rows=n, ldv=n, method=self.orth)
                    if givens(j, h, hb):
                        break
            y = np.linalg.solve(np.triu(H[:j_done, :j_done]), g[:j_done])
            dx = dense.gemm_ts(V, y.reshape(-1, 1), k=j_done, rows=n, ldz=n)          # (1, n)
            dense.axpy(1.0, dx, x, n)
            if abs(g[j_done]) <= tolabs:
                # converged by the recurrence's residual norm: IterativeSolvers.gmres leaves here too (it evaluates the true
                # residual only when it restarts), which saves one operator + preconditioner application per solve
                beta = abs(g[j_done])
                break
            # true (preconditioned) residual for the restart
            dense.copy(self.nep.compute_Mlincomb(self.lam, x.reshape(1, n)), r, n)
            dense.scal(r, -1.0, n); dense.axpy(1.0, bvec, r, n); self._prec(r)
            beta = dense.nrm2(r)
        self.iterations = its
        X = torch.empty_like(b) if out is None else out
        dense.copy(x, X, n)
        if scale != 1.0:
            dense.scal(X, scale, n)
        return X.reshape(b.shape)


class GMRESLinSolverCreator(LinSolverCreator):
    """src/LinSolverCreators.jl:124-145"""

    def __init__(self, **kwargs):
        self.kwargs = kwargs
