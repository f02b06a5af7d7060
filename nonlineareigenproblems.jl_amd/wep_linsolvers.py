"""Waveguide-specific linear solvers on the device: the Schur-complement solvers and the Sylvester-SMW preconditioner of
src/gallery_extra/waveguide/Waveguide.jl:394-567 and waveguide_preconditioner.jl (Ringh, Mele, Karlsson, Jarlebring,
"Sylvester-based preconditioning for the waveguide eigenvalue problem").

  WEPLinSolverCreator(solver_type="factorized" | "backslash" | "gmres", kwargs=...)     Waveguide.jl:489-519
  lin_solve through the Schur complement of the boundary block (Ringh Prop. 2.1)        Waveguide.jl:552-567
  SchurMatVec, construct_WEP_schur_complement                                           Waveguide.jl:394-425, 523-550
  wep_generate_preconditioner(nep, N, sigma)                                            waveguide_preconditioner.jl:36-47

Device realisation.  The interior operator A(lam) X + X B + K .* X is the interior block of the three stacked sparse terms,
so SchurMatVec is ONE K1 call on the zero-padded vector (its last 2 nz rows are C2T v for free) + P(lam)^{-1} on 2 nz
entries + one rectangular CSR product with C1 (nep_csr_mv); with a P^{-1} plan the whole product is matrix-free (five-point
stencil, nep_wep_schur_matvec).  P(lam)^{-1} = R diag(1/s(lam)) R^H / nz with the scaled-DFT matrix R: a prime-factor DFT
plan (nep_wep_pinv_apply), or two nz x nz GEMVs with the dense R where nz is too large for the plan.

The reference diagonalises the Sylvester operator with FFTs along z (length nz) and sine transforms along x; here the
Sylvester solve (nep_wep_sylv_solve, csrc/wep.hip) is a prime-factor DFT along z plus one tridiagonal solve per z-mode along
x, and it takes every grid the constructor admits (nx = nz + 4 <= 2048).  The region means and the expansion of the SMW
correction are region kernels (nep_wep_region_means / nep_wep_region_expand); the mm x mm SMW matrix is inverted once on the
device and applied as a GEMV, so one preconditioner application never synchronises.  Which form of the correction runs is
fixed when the preconditioner is built (WEPPreconditioner._fused): the three-transform form (nep_wep_smw_apply, with the
set-up in mode space) where nep_wep_plan has one for the grid, otherwise the piecewise form (four transforms).
"""
import ctypes as C
import inspect

import numpy as np
import scipy.sparse as sp
import torch

from . import _lib, dense
from ._env import env_str
from ._lib import lib, check, c_vp
from .linsolvers import DeviceLU, FactorizeLinSolver, GMRESLinSolver, LinSolver, LinSolverCreator
from .nep import CDT, DeviceCSR, to_dev, to_host, stream_ptr
from .wep import WEP, _corner_derivs, _p

PLAN_SMW = 2                  # NEP_WEP_PLAN_SMW of nep_wep_plan


def _boundary_csr(nep):
    """C1 (N x 2nz) and C2T (2nz x N) of the stacked matrix A1 = [Q0 C1; C2T 0] as device operators (cached on the NEP)"""
    if getattr(nep, "_C1dev", None) is None:
        N = nep.N
        A1 = sp.csr_matrix(nep.A[0])
        nep._C1dev = DeviceCSR(A1[:N, N:])
        nep._C2Tdev = DeviceCSR(A1[N:, :N])
    return nep._C1dev, nep._C2Tdev


class SchurOps:
    """device pieces shared by the Schur-complement solvers for one shift: P(lam)^{-1}, SchurMatVec, the elimination /
    back-substitution of the boundary unknowns"""

    def __init__(self, nep, lam):
        if not isinstance(nep, WEP):
            raise TypeError("WEPLinSolver can only be used in combination with WEPs: type(nep)=%s" % type(nep).__name__)
        self.nep, self.lam = nep, complex(lam)
        self.n, self.N, self.nz, self.nx = nep.n, nep.N, nep.nz, nep.nx
        self.C1, self.C2T = _boundary_csr(nep)
        self.Rm, self.RmH = nep._corner_dev()
        s = _corner_derivs(nep.wd, self.lam, 1)[:, 0]
        self.sinv = to_dev(1.0 / (s * self.nz))[0]                     # 1 / (nz s_j(lam)), 2 nz entries
        self.coef = to_dev(np.array([[1.0, self.lam, self.lam ** 2]], dtype=np.complex128))    # 1 x 3, device resident
        # matrix-free form of the interior operator (five-point stencil, csrc/wep.hip nep_wep_schur_matvec): weights of
        # generate_fd_interior_mat / generate_fd_boundary_mat (Waveguide.jl:17-19), diagonal K + lam^2 - 2/hz^2 - 2/hx^2
        wd = nep.wd
        self.stencil = None
        if nep._pinv_plan() is not None and env_str("NEP_WEP_STENCIL", "1") != "0":
            lam_ = self.lam
            D0 = np.asarray(wd.K, dtype=np.complex128) + (lam_ ** 2 - 2.0 / wd.hz ** 2 - 2.0 / wd.hx ** 2)
            self.stencil = dict(D0=to_dev(D0), cp=_lib.cd(1.0 / wd.hz ** 2 + lam_ / wd.hz), cm=_lib.cd(1.0 / wd.hz ** 2 - lam_ / wd.hz),
                                cx=1.0 / wd.hx ** 2, d1=2.0 / wd.hx, d2=-1.0 / (2.0 * wd.hx), c1s=1.0 / wd.hx ** 2)
        self.pad = torch.zeros(self.n, dtype=CDT, device="cuda")
        self.z = torch.empty(self.n, dtype=CDT, device="cuda")
        self.t = torch.empty(2 * self.nz, dtype=CDT, device="cuda")
        self.u = torch.empty(2 * self.nz, dtype=CDT, device="cuda")
        self.w = torch.empty(2 * self.nz, dtype=CDT, device="cuda")

    def pinv(self, x, out, xskip=0, oskip=0):
        """out = blkdiag(R, R) diag(1/s(lam)) blkdiag(R, R)^H x / nz   (Waveguide.jl:159-162); x, out: tensors or device addresses,
        the 2 nz entries (minus block, plus block) start xskip / oskip entries in.  Without a P^{-1} plan: two A^H x products per
        block (nep_gemv_hd), the diagonal scaling fused into the first one; the work vector self.w is used"""
        nz = self.nz
        st = stream_ptr()
        plan = self.nep._pinv_plan()
        if plan is not None:
            check(lib.nep_wep_pinv_apply(plan, _p(self.sinv), _p(x, xskip), _p(out, oskip), st))
            return
        for half in (0, 1):
            o = half * nz
            check(lib.nep_gemv_hd(_p(self.Rm), nz, nz, nz, _p(x, xskip + o), _p(self.sinv, o), _p(self.w, o), st))    # w = (1/(nz s)) .* (R^H x)
            check(lib.nep_gemv_hd(_p(self.RmH), nz, nz, nz, _p(self.w, o), None, _p(out, oskip + o), st))     # (R^H)^H w

    def matvec(self, v, out):
        """out = vec(A(lam) X + X B + K .* X) - C1 P(lam)^{-1} C2T v   (SchurMatVec, Waveguide.jl:398-406)"""
        N, n = self.N, self.n
        if self.stencil is not None and v.data_ptr() != out.data_ptr():
            st = self.stencil
            check(lib.nep_wep_schur_matvec(self.nep._pinv_plan(), _p(self.sinv), self.nx, _p(v), _p(st["D0"]), st["cp"], st["cm"],
                                           st["cx"], st["d1"], st["d2"], st["c1s"], _p(self.t), _p(out), stream_ptr()))
            return out
        check(lib.nep_dev_copy(_p(self.pad), _p(v), 16 * N, stream_ptr()))
        self.nep.dev.mlincomb_dev(self.coef, 1, 1, self.pad.data_ptr(), n, self.z)      # no host->device copy: graph-safe
        self.pinv(self.z, self.t, xskip=N)
        self.C1.mv(-1.0, self.t, 1.0, self.z, out)
        return out

    def eliminate(self, x, rhs):
        """rhs = x_int - C1 P^{-1} x_ext   (Waveguide.jl:559-561)"""
        self.pinv(x, self.t, xskip=self.N)
        self.C1.mv(-1.0, self.t, 1.0, x, rhs)
        return rhs

    def recover(self, q, x, out):
        """out = [q; P^{-1}(x_ext - C2T q)]   (Waveguide.jl:565)"""
        self.C2T.mv(-1.0, q, 1.0, _p(x, self.N).value, self.u)
        self.pinv(self.u, out, oskip=self.N)
        if q.data_ptr() != _p(out).value:
            check(lib.nep_dev_copy(_p(out), _p(q), 16 * self.N, stream_ptr()))
        return out


def construct_WEP_schur_complement(nep, lam):
    """Waveguide.jl:523-550 (Ringh Prop. 3.1) on the host: interior block of M(lam) minus the two dense boundary couplings
    kron(E, P_-^{-1}) + kron(EE, P_+^{-1}) (four dense nz x nz blocks)"""
    wd = nep.wd; nz, nx, N = nep.nz, nep.nx, nep.N
    lam = complex(lam)
    S = sp.csr_matrix(nep.A[0], dtype=np.complex128)[:N, :N] + lam * sp.csr_matrix(nep.A[1])[:N, :N] + lam ** 2 * sp.csr_matrix(nep.A[2])[:N, :N]
    Rm = wd.Rmat()
    s = _corner_derivs(wd, lam, 1)[:, 0]
    Pm = (Rm / s[None, :nz]) @ Rm.conj().T / nz
    Pp = (Rm / s[None, nz:]) @ Rm.conj().T / nz
    d1 = (2 / wd.hx) / wd.hx ** 2; d2 = (-1 / (2 * wd.hx)) / wd.hx ** 2
    ii, jj = np.meshgrid(np.arange(nz), np.arange(nz), indexing="ij")
    rows = np.concatenate([ii.ravel(), ii.ravel(), (N - nz + ii).ravel(), (N - nz + ii).ravel()])
    cols = np.concatenate([jj.ravel(), (nz + jj).ravel(), (N - nz + jj).ravel(), (N - 2 * nz + jj).ravel()])
    vals = np.concatenate([d1 * Pm.ravel(), d2 * Pm.ravel(), d1 * Pp.ravel(), d2 * Pp.ravel()])
    return sp.csc_matrix(S - sp.csr_matrix((vals, (rows, cols)), shape=(N, N)))


class _SchurSolve:
    """`lu`-like object (n, solve, solve_add) whose solve eliminates the boundary unknowns, calls the inner solver on the
    Schur complement and recovers them -- what FactorizeLinSolver's refinement loop drives"""

    def __init__(self, ops, inner):
        self.ops, self.inner, self.n = ops, inner, ops.n
        self._sweep_kw = "sweep" in inspect.signature(inner).parameters      # the iterative inner solver is told which solves are sweeps
        self.rhs = torch.empty(ops.N, dtype=CDT, device="cuda")
        self.q = torch.empty(ops.N, dtype=CDT, device="cuda")
        self.tmp = torch.empty(ops.n, dtype=CDT, device="cuda")

    def _one(self, b, out, tol=None, sweep=False):
        self.ops.eliminate(b, self.rhs)
        if sweep and self._sweep_kw:
            self.inner(self.rhs, self.q, tol, sweep=True)
        else:
            self.inner(self.rhs, self.q, tol)
        self.ops.recover(self.q, b, out)

    def solve(self, B, out=None, scale=1.0, tol=None):
        Bd = B if B.dim() == 2 else B.reshape(1, -1)
        X = torch.empty_like(Bd) if out is None else (out if out.dim() == 2 else out.reshape(1, -1))
        for j in range(Bd.shape[0]):
            self._one(Bd[j], self.tmp, tol)
            dense.copy(self.tmp, X[j], self.n)
        if scale != 1.0:
            dense.scal(X, scale, X.numel())
        return X.reshape(B.shape)

    def solve_add(self, B, add, out, scale=1.0):
        Bd = B if B.dim() == 2 else B.reshape(1, -1)
        self._one(Bd[0], self.tmp, sweep=True)         # a refinement sweep: the right-hand side is a residual
        dense.axpy(1.0, add, self.tmp, self.n)
        dense.copy(self.tmp, out, self.n)
        if scale != 1.0:
            dense.scal(out, scale, self.n)
        return out


class WEPFactorizedLinSolver(FactorizeLinSolver):
    """Waveguide.jl:466-480: the Schur complement is assembled and factorised once (host SuperLU -> device schedule, K5);
    every lin_solve is followed by the refinement of FactorizeLinSolver on the full operator"""

    def __init__(self, nep, lam, kwargs=(), umfpack_refinements=10, expected_solves=200):
        self.ops = SchurOps(nep, lam)
        self.schur_lu = DeviceLU(construct_WEP_schur_complement(nep, lam), expected_solves=expected_solves)
        inner = lambda rhs, q, tol: self.schur_lu.solve(rhs.reshape(1, -1), out=q.reshape(1, -1))
        super().__init__(nep, lam, umfpack_refinements, _lu=_SchurSolve(self.ops, inner))


class WEPBackslashLinSolver(LinSolver):
    """Waveguide.jl:449-463: `schur_comp \\ rhs`, a fresh factorisation at every lin_solve"""

    def __init__(self, nep, lam, kwargs=()):
        self.nep, self.lam = nep, complex(lam)
        self.ops = SchurOps(nep, lam)
        self.schur_comp = construct_WEP_schur_complement(nep, lam)

    def solve_dev(self, b, out=None, scale=1.0):
        lu = DeviceLU(self.schur_comp, expected_solves=1)
        inner = lambda rhs, q, tol: lu.solve(rhs.reshape(1, -1), out=q.reshape(1, -1))
        return _SchurSolve(self.ops, inner).solve(b, out=out, scale=scale)


class _SchurOperator:
    """what GMRESLinSolver needs from a `nep`: size and the operator action"""

    def __init__(self, ops):
        self.ops = ops
        self.out = torch.empty(ops.N, dtype=CDT, device="cuda")

    def size(self, d=None):
        return self.ops.N

    def compute_Mlincomb(self, lam, V):
        return self.ops.matvec(V, self.out)


class WEPGMRESLinSolver(LinSolver):
    """Waveguide.jl:428-446: matrix-free restarted GMRES on the Schur complement (device basis, K6 orthogonalisation);
    kwargs as ((name, value), ...) or a dict: Pl (e.g. wep_generate_preconditioner), reltol / tol, restart, maxiter.

    `refinements` (not in the reference; 0 = its behaviour): iterative refinement of the full system around the GMRES solve
    with the stopping rule of FactorizeLinSolver (componentwise backward error).  Left-preconditioned GMRES controls the
    preconditioned residual; at n = 10^6 the true residual levels off near 5e-12 however small reltol is chosen, while
    a few cheap sweeps (reltol ~ 1e-6, each on the residual of the last) reach the accuracy of a direct solve.
    kwargs key `sweep_reltol`: the inner tolerance of those sweeps (a correction of relative size 1e-9 needs no nine
    digits of its own); default = reltol."""
    accepts_tol = True

    def __init__(self, nep, lam, kwargs=(), refinements=0):
        self.nep, self.lam = nep, complex(lam)
        self.ops = SchurOps(nep, lam)
        kw = dict(kwargs)
        kw.pop("log", None)
        self.sweep_reltol = kw.pop("sweep_reltol", None)
        self.gmres = GMRESLinSolver(_SchurOperator(self.ops), self.lam, kw)
        self.iterations = []

        self._graph = None
        # one operator step = 2 foreign calls (nep_wep_schur_matvec, nep_wep_smw_apply: 11 launches) when both fused forms apply:
        # issued directly, without the copy in / copy out of a graph on fixed buffers (measured on C5: 1.29 s against 1.35 s);
        # the graph remains for the piecewise routes (~30 launches from Python per step)
        Pl = self.gmres._Pl_call
        direct = self.ops.stencil is not None and isinstance(Pl, WEPPreconditioner) and Pl._fused
        if Pl is not None and not direct:
            self._capture_step()
        elif direct:
            # straight from basis vector j into basis vector j + 1: no operator-owned output block and no copy behind it
            ops_ = self.ops

            def direct_step(v, w):
                ops_.matvec(v, w)
                Pl(w)
            self.gmres.fused_step = direct_step

        def inner(rhs, q, tol, sweep=False):
            if sweep and self.sweep_reltol is not None:
                tol = float(self.sweep_reltol)
            elif self.gmres.reltol is not None:
                tol = None
            self.gmres.solve_dev(rhs, out=q, tol=tol)
            self.iterations.append(self.gmres.iterations)
        self.schur = _SchurSolve(self.ops, inner)
        self.refined = FactorizeLinSolver(nep, lam, refinements, _lu=self.schur) if refinements > 0 else None

    def _capture_step(self):
        """one GMRES operator step w = Pl^{-1} S v (1 K1 call, ~12 GEMMs, ~15 small kernels) recorded once as a hipGraph on
        fixed buffers; per iteration: copy in, replay, copy out.  Falls back to the eager sequence if capture fails."""
        N = self.ops.N
        vin = torch.empty(N, dtype=CDT, device="cuda"); wout = torch.empty(N, dtype=CDT, device="cuda")
        prec = self.gmres._Pl_call

        def step():
            self.ops.matvec(vin, wout)
            prec(wout)
        try:
            side = torch.cuda.Stream()
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):
                vin.zero_(); step()                      # warm-up outside the capture (lazy kernel loads)
            torch.cuda.current_stream().wait_stream(side)
            torch.cuda.synchronize()
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                step()
            torch.cuda.synchronize()
        except Exception as e:                           # keep the eager path
            self._graph_error = repr(e)
            return
        self._graph, self._vin, self._wout = g, vin, wout

        def fused(v, w):
            dense.copy(v, vin, N)
            g.replay()
            dense.copy(wout, w, N)
        self.gmres.fused_step = fused

    def solve_dev(self, b, out=None, scale=1.0, tol=None):
        if self.refined is not None:
            return self.refined.solve_dev(b, out=out, scale=scale)
        # lin_solve(solver, x; tol = eps(Float64)), Waveguide.jl:555
        return self.schur.solve(b, out=out, scale=scale, tol=tol if tol else np.finfo(float).eps)


class WEPLinSolverCreator(LinSolverCreator):
    """Waveguide.jl:489-519"""

    def __init__(self, solver_type="factorized", kwargs=(), refinements=0):
        self.solver_type, self.kwargs, self.refinements = str(solver_type).lstrip(":"), kwargs, refinements

    def create_linsolver(self, nep, lam):
        if not isinstance(nep, WEP):
            raise TypeError("WEPLinSolver can only be used in combination with WEPs: type(nep)=%s" % type(nep).__name__)
        if self.solver_type == "backslash":
            return WEPBackslashLinSolver(nep, lam, self.kwargs)
        if self.solver_type == "gmres":
            return WEPGMRESLinSolver(nep, lam, self.kwargs, refinements=self.refinements)
        if self.solver_type == "factorized":
            return WEPFactorizedLinSolver(nep, lam, self.kwargs)
        raise ValueError("Unknown type of solver_type in linsolvercreator:%s" % self.solver_type)


# ------------------------------------------------------------------------------------------------ preconditioner
class WEPPreconditioner:
    """waveguide_preconditioner.jl:10-421 on the device.  Callable on a device vector r of nx nz entries (in place):
    r <- Linv r - Linv(sum_k alpha_k E_k),  alpha = M^{-1} f(Linv r),  with Linv the Sylvester solve for A(sigma) X + X B,
    E_k the region-wise pieces of K .* X and of the boundary couplings, f the region means."""

    def __init__(self, nep, N, sigma):
        if not isinstance(nep, WEP):
            raise TypeError("the waveguide preconditioner needs a WEP")
        nz, nx = nep.nz, nep.nx
        if nz + 4 != nx:
            raise ValueError("This implementation requires nx = nz + 4. Provided NEP has nz = %d and nx = %d" % (nz, nx))
        if N < 1 or nz % N != 0:
            raise ValueError("This implementation is uniform in the blocking and therefore requires nz/N to be an integer. "
                             "Provided data is nz = %d with N = %d" % (nz, N))
        _lib.require_gpu()
        self.nep, self.N, self.sigma = nep, int(N), complex(sigma)
        wd = nep.wd
        L = nz // N
        self.L, self.mm = L, N * N + 4 * N
        self.ops = SchurOps(nep, self.sigma)
        Kmat = np.asarray(wd.K, dtype=np.complex128)
        k_bar = np.mean(Kmat)
        # ---- Sylvester operator: eigenvalues / transforms (waveguide_preconditioner.jl:127-140)
        v = np.zeros(nz, dtype=complex); v[0] = -2; v[1] = 1; v[nz - 1] = 1; v /= wd.hz ** 2
        w = np.zeros(nz, dtype=complex); w[1] = 1; w[nz - 1] = -1; w *= self.sigma / wd.hz
        D = np.fft.fft(v + w) + (self.sigma ** 2 + k_bar)
        # Sylvester solve: prime-factor DFT along z + one tridiagonal solve per z-mode along x (csrc/wep.hip); it takes every
        # nx = nz + 4 <= 2048 (tests/test_host_wep_checkers.py), a larger grid is refused here
        self.dd1 = (2 / wd.hx) / wd.hx ** 2; self.dd2 = (-1 / (2 * wd.hx)) / wd.hx ** 2
        h = c_vp()
        Dc = np.ascontiguousarray(D, dtype=np.complex128)
        check(lib.nep_wep_sylv_create(nz, nx, _lib.hptr(Dc), 1.0 / wd.hx ** 2, C.byref(h)))
        self.sylv = h
        self.Ksc = to_dev(Kmat - k_bar)                                                    # K_scaled (Waveguide.jl:229-230)
        # ---- work space of the piecewise route; regions: kappa = i + N j
        self.Y = torch.empty((nx, nz), dtype=CDT, device="cuda")
        self.fb = torch.empty((N + 4, N), dtype=CDT, device="cuda")        # N x (N+4): functionals
        self.al = torch.empty((N + 4, N), dtype=CDT, device="cuda")        # alpha
        self.eb = torch.empty((2, nz), dtype=CDT, device="cuda")           # nz x 2 = [e_minus, e_plus]
        self.pb = torch.empty(2 * nz, dtype=CDT, device="cuda")
        self.MinvH = None
        # ---- the route, fixed here: nep_wep_plan evaluates the predicates nep_wep_smw_apply / nep_wep_smw_matrix_modes test
        info = (C.c_int64 * 8)()
        self._fused = (env_str("NEP_WEP_SMW_FUSED", "1") != "0" and nep._pinv_plan() is not None
                       and lib.nep_wep_plan(nz, nx, PLAN_SMW, info) == _lib.NEP_OK)
        self._G = self._mode_means_matrix() if self._fused else None
        self._generate()

    def __del__(self):
        try:
            if getattr(self, "sylv", None):
                lib.nep_wep_sylv_destroy(self.sylv)
                self.sylv = None
        except Exception:
            pass

    # -- pieces
    def linv(self, X):
        """in place Sylvester solve on a device nz x nx matrix (column-major): prime-factor DFT along z, one tridiagonal solve
        per z-mode along x, back transform"""
        check(lib.nep_wep_sylv_solve(self.sylv, _p(X), stream_ptr()))
        return X

    def functionals(self, X, out):
        """out (N x (N+4)) = region means of X (waveguide_preconditioner.jl:297-304)"""
        check(lib.nep_wep_region_means(self.nep.nz, self.nep.nx, self.N, _p(X), _p(out), stream_ptr()))
        return out

    def expand(self, alpha, Y):
        """Y (nz x nx) = sum_k alpha_k E_k  (waveguide_preconditioner.jl:263-288, :382-412): K_scaled restricted to the regions,
        plus -P^{-1}(sigma) of the boundary pieces in the first and last column"""
        nz, nx, N = self.nep.nz, self.nep.nx, self.N
        check(lib.nep_wep_region_expand(nz, nx, N, _p(alpha), _p(self.Ksc), self.dd1, self.dd2, _p(Y), _p(self.eb), stream_ptr()))
        self.ops.pinv(self.eb, self.pb)
        dense.axpy(-1.0, self.pb, Y, nz)                                                     # column 1       -= P_-^{-1} e_-
        check(lib.nep_axpy(nz, _lib.cd(-1.0), _p(self.pb, nz), _p(Y, nz * (nx - 1)), stream_ptr()))    # column nx -= P_+^{-1} e_+
        return Y

    # -- the SMW matrix: one of three routes
    def _generate(self):
        """waveguide_preconditioner.jl:221-313: M[:, k] = f(Linv E_k) + identity, inverted once (mm x mm)"""
        Mdev = torch.empty((self.mm, self.mm), dtype=CDT, device="cuda")            # column kappa at Mdev[kappa]
        if self._fused:
            self._matrix_modes(Mdev)
        elif self.nep._pinv_plan() is not None:
            self._matrix_library(Mdev)
        else:
            self._matrix_by_columns(Mdev)
        self._set_inverse(Mdev, self.mm)

    def _matrix_modes(self, Mdev):
        """mode-space form (no back transforms, interior columns batched): the set-up of the three-transform form"""
        check(lib.nep_wep_smw_matrix_modes(self.sylv, self.nep._pinv_plan(), self.N, _p(self.Ksc), self.dd1, self.dd2, _p(self.ops.sinv),
                                           _p(self._G), _p(Mdev), stream_ptr()))

    def _matrix_library(self, Mdev):
        """all mm columns of the piecewise form inside the library (one foreign call instead of ~8 per column)"""
        work = torch.empty(self.nep.nz * self.nep.nx + 4 * self.nep.nz + self.mm, dtype=CDT, device="cuda")
        check(lib.nep_wep_smw_matrix(self.sylv, self.nep._pinv_plan(), self.N, _p(self.Ksc), self.dd1, self.dd2, _p(self.ops.sinv),
                                     _p(work), _p(Mdev), stream_ptr()))

    def _matrix_by_columns(self, Mdev):
        """column by column through the pieces: the grids without a P^{-1} plan (nz >= 1921)"""
        unit = torch.zeros((self.N + 4, self.N), dtype=CDT, device="cuda").reshape(-1)
        one = torch.ones(1, dtype=CDT, device="cuda")
        for kappa in range(self.mm):
            unit.zero_()
            unit[kappa:kappa + 1].copy_(one)
            self.expand(unit, self.Y)
            self.linv(self.Y)
            self.functionals(self.Y, Mdev[kappa])

    def _set_inverse(self, Mdev, mm):
        """MinvH = inv(I + M)^H (alpha = (MinvH)^H f through nep_gemv_hd).  On the device by the library's Gauss-Jordan inverse
        (nep_zinv_h_dev: 2 launches per column; 1517 x 1517 in ~35 ms against 0.14 s of numpy.linalg.inv on 8 BLAS threads + two
        36 MB transfers); the host route is the fallback for a zero pivot."""
        self._Mdev = Mdev
        self._M_host = None
        out = torch.empty((mm, mm), dtype=CDT, device="cuda")
        work = torch.empty(2 * mm + 2, dtype=CDT, device="cuda")
        info = C.c_int32(0)
        check(lib.nep_zinv_h_dev(mm, _p(Mdev), mm, 1.0, _p(out), mm, _p(work), C.byref(info), stream_ptr()))
        if info.value == 0:
            self.MinvH = out
            return
        self._M_host = to_host(Mdev) + np.eye(mm)
        self.MinvH = to_dev(np.linalg.inv(self._M_host).conj().T)

    @property
    def _M(self):
        if self._M_host is None:
            self._M_host = to_host(self._Mdev) + np.eye(self._Mdev.shape[0])
        return self._M_host

    @property
    def cond(self):
        """2-norm condition number of the SMW matrix (diagnostic: an SVD of the mm x mm matrix, 0.3 s at mm = 1517, so only
        computed when asked for)"""
        if getattr(self, "_cond", None) is None:
            self._cond = float(np.linalg.cond(self._M))
        return self._cond

    def _mode_means_matrix(self):
        """G (N x nz): mean over the z of region rz of column i of the inverse transform F[z, i] = exp(-2 pi i z i / nz) / sqrt(nz)
        (what nep_wep_sylv_solve's last kernel applies) -- the region means of F U are G (U summed over the x-regions)"""
        nz, N, L = self.nep.nz, self.N, self.L
        i = np.arange(nz)
        # mean over z = rz L + l of w^(z i), w = exp(-2 pi i / nz):  w^(rz L i) * (sum_l w^(l i)) / L  (exponents reduced mod nz)
        inner = np.exp(-2j * np.pi * (np.outer(np.arange(L), i) % nz) / nz).sum(axis=0) / L                 # nz
        outer = np.exp(-2j * np.pi * (np.outer(np.arange(N) * L, i) % nz) / nz)                              # N x nz
        G = outer * inner[None, :] / np.sqrt(nz)
        return to_dev(np.ascontiguousarray(G).T)                                       # to_dev stores (rows, cols) column-major

    def __call__(self, r):
        """solve_smw (waveguide_preconditioner.jl:323-421), in place on the device vector r"""
        return self._apply_fused(r) if self._fused else self._apply_piecewise(r)

    def _apply_fused(self, r):
        """three transforms, the region means and the second solve in mode space (one foreign call)"""
        check(lib.nep_wep_smw_apply(self.sylv, self.nep._pinv_plan(), self.N, _p(self.Ksc), self.dd1, self.dd2, _p(self.ops.sinv),
                                    _p(self.MinvH), _p(self._G), _p(r), stream_ptr()))
        return r

    def _apply_piecewise(self, r):
        """as the reference writes it: four transforms"""
        mm = self.mm
        self.linv(r)                                                           # C = Linv r
        self.functionals(r, self.fb)
        check(lib.nep_gemv_hd(_p(self.MinvH), mm, mm, mm, _p(self.fb), None, _p(self.al), stream_ptr()))
        self.expand(self.al, self.Y)
        self.linv(self.Y)
        dense.axpy(-1.0, self.Y, r, self.nep.nz * self.nep.nx)
        return r


def wep_generate_preconditioner(nep, N, sigma):
    """waveguide_preconditioner.jl:36-47"""
    return WEPPreconditioner(nep, N, sigma)
