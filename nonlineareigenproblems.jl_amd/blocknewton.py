"""Block Newton method for an invariant pair (S, X) (D. Kressner, Numer. Math. 114 (2009); src/method_blocknewton.jl) on the device.

`blocknewton(nep, S, X, ...)` returns (S, X) on the host with M(S, X) = sum_t A_t X f_t(S) = 0 and Vl(X, S) = [X; X S; ...; X S^(p-1)]
orthonormal.  X, Vl(X, S), its Q factor W, the right-hand sides and the correction stay on the device; the p x p and 2p x 2p
matrices (Schur form, f_t of the expanded matrices, the Schur complement of the bordered system) are host work.

Every product with the matrices of the NEP is one nep_spmf_blockprod (csrc/blockprod.hip): Z = beta Z + alpha sum_t A_t (Y G_t) with
per-term host tables G_t -- the residual (G_t = f_t(S)), T12 of column i (G_t = the upper right block of f_t([S I; 0 s_i I])), the
update (21) of the remaining right-hand sides (Y = [X dx_i]) and the residual of the refinement steps.  Sizes the kernel refuses
(r or q above 32, more than 48 KiB of tables) are composed from nep_gemm_ts + nep_spmm_terms as compute_MM does.  All products
W_j^H B come from ONE product of the stacked W (n x p l, a strided view of the np x p Q factor) with B; the powers of s_i and S
are applied to the small result on the host.

The bordered system [M(s_i) T12; T21 T22] [dx; ds] = [RT_i; RV_i] (method_blocknewton.jl:190-191) is solved by block elimination
through a linear solver of M(s_i) -- the NEP's own sparsity pattern, so the device numeric LU applies -- and the p x p Schur
complement.  M(s_i) becomes singular as s_i converges, and plain elimination then stagnates; `refine` steps of iterative refinement
on the bordered system (each correction by the same elimination) restore the iteration counts of a solve with the whole matrix
(DESIGN.md, K12).  bordered="whole" assembles and factorises the bordered matrix as the reference does; it is also the fallback of
a column whose M(s_i) is found exactly singular.
"""
import numpy as np
import scipy.linalg as sla
import scipy.sparse as sp
import torch

from . import _lib, dense
from ._lib import lib, check, hptr, c_vp, cd
from .exceptions import NoConvergenceException
from .nep import CDT, pure_spmf, to_dev, to_host, stream_ptr

EPS = np.finfo(float).eps
BORDERED = ("eliminate", "whole")
MAXP = 32
BP_MAXRQ, BP_MAXTAB = 32, 3072          # limits of nep_spmf_blockprod (include/nepmi355.h)


# ---- host tables ----------------------------------------------------------------------------------------------------------------
def _matfun(f, S):
    return np.asarray(f.matfun(S), dtype=np.complex128)


def tables_fS(fv, S):
    """G_t = f_t(S): the residual M(S, X) and compute_MM"""
    return np.stack([_matfun(f, S) for f in fv])


def tables_T12(fv, S, s):
    """G_t = f_t([S I; 0 s I])[0:p, p:2p] (:173-179): the divided difference of f_t at (S, s I)"""
    p = S.shape[0]
    Se = np.block([[S, np.eye(p)], [np.zeros((p, p)), s * np.eye(p)]])
    return np.stack([_matfun(f, Se)[:p, p:] for f in fv])


def tables_update21(fv, fS, S, ds, i):
    """update (21) of the columns behind i with Y = [X dx_i]: rows 0 .. p - 1 of G_t are f_t([S Z; 0 S])[0:p, p+i+1:2p] with
    Z = ds e_i^T (the derivative of f_t at S in the direction Z), row p is f_t(S)[i, i+1:] (:198-206)"""
    p = S.shape[0]
    Z = np.zeros((p, p), dtype=np.complex128)
    Z[:, i] = ds
    S2 = np.block([[S, Z], [np.zeros((p, p)), S]])
    return np.stack([np.vstack([_matfun(f, S2)[:p, p + i + 1:], fS[t][i:i + 1, i + 1:]]) for t, f in enumerate(fv)])


def tables_refine(fv, T12tab, s, x2):
    """the top residual of the bordered system with Y = [X x1]: G_t = [DF1_t x2; f_t(s)] ((p + 1) x 1)"""
    return np.stack([np.concatenate([T12tab[t] @ x2, [f(s)]]).reshape(-1, 1) for t, f in enumerate(fv)])


def constraint_tables(S, i, l):
    """D[j] multiplies W_j^H X in T22 (D[1] = I, D[j + 1] = s D[j] + S^(j-1), :184-189) and P[j] = S^(j-1) gives the row that
    multiplies W_j^H dx_i in update (22) (:208), j = 1 .. l - 1, as the reference forms them"""
    p = S.shape[0]
    s = S[i, i]
    D = [None, np.eye(p, dtype=np.complex128)]
    for j in range(1, l - 1):
        D.append(s * D[j] + np.linalg.matrix_power(S, j - 1))
    P = [None] + [np.linalg.matrix_power(S, j - 1) for j in range(1, l)]
    return D, P


def update22_tables(S, ds, i, l):
    """E[1] = ds e_i^T, E[j + 1] = E[j] S + S^(j-1) E[j] (:199, :211)"""
    p = S.shape[0]
    E = [None, np.zeros((p, p), dtype=np.complex128)]
    E[1][:, i] = ds
    for j in range(1, l - 1):
        E.append(E[j] @ S + np.linalg.matrix_power(S, j - 1) @ E[j])
    return E


def check_arguments(nep, S, X, bordered, refine, blockprod="fused"):
    """(S, X, n, p) as complex arrays with the reference's defaults (:49-50), or the exception the call deserves"""
    if not pure_spmf(nep, "MM"):
        raise TypeError("blocknewton needs an SPMF-type NEP (sum_t f_t(lam) A_t with compute_MM), not %s" % type(nep).__name__)
    if bordered not in BORDERED:
        raise ValueError("bordered must be one of %r, not %r" % (BORDERED, bordered))
    if blockprod not in ("fused", "composed"):
        raise ValueError("_blockprod must be 'fused' or 'composed'")
    if int(refine) < 0:
        raise ValueError("refine must be >= 0")
    n = int(nep.size(1))
    S = np.zeros((2, 2), dtype=np.complex128) if S is None else np.array(S, dtype=np.complex128)
    if S.ndim != 2 or S.shape[0] != S.shape[1]:
        raise ValueError("S must be square, got shape %r" % (S.shape,))
    p = S.shape[0]
    if not 1 <= p <= MAXP:
        raise ValueError("blocknewton: 1 <= p <= %d, got p = %d" % (MAXP, p))
    X = np.eye(n, 2, dtype=np.complex128) if X is None else np.array(X, dtype=np.complex128)
    if X.shape != (n, p):
        raise ValueError("X must be %d x %d, got shape %r" % (n, p, X.shape))
    return S, X, n, p


# ---- device pieces --------------------------------------------------------------------------------------------------------------
class _Work:
    """the NEP's device handle, the counters of `info` and the block products"""

    def __init__(self, nep, n, p, force_composed):
        self.nep, self.n, self.p = nep, n, p
        self.fv = nep.get_fv()
        self.mt = len(self.fv)
        self.force_composed = force_composed
        self.blockprod_calls = self.composed_calls = 0
        self.factorizations = self.device_factorizations = self.whole_fallbacks = 0
        self.ksplit = int(min(64, max(1, n // 512)))
        self.skwork = torch.empty(self.ksplit * p * p * (p + 1), dtype=CDT, device="cuda")

    def blockprod(self, Yd, G, out, alpha=1.0, beta=0.0):
        """out[:q] = beta out[:q] + alpha sum_t A_t (Y[:, :r] G_t); Yd: device (>= r, n), G: host (mt, r, q), out: device (>= q, n)"""
        mt, r, q = G.shape
        assert mt == self.mt and Yd.shape[0] >= r and out.shape[0] >= q and Yd.shape[1] == self.n == out.shape[1]
        if not self.force_composed:
            Gf = np.ascontiguousarray(np.transpose(G, (0, 2, 1)), dtype=np.complex128)           # G_t column-major at t r q
            rc = lib.nep_spmf_blockprod(self.nep.dev.h, r, q, c_vp(Yd.data_ptr()), self.n, hptr(Gf), cd(alpha), cd(beta),
                                        c_vp(out.data_ptr()), self.n, stream_ptr())
            if rc != _lib.NEP_ERR_UNSUPPORTED:
                check(rc)
                self.blockprod_calls += 1
                return out
        # composed: (Y [G_1 .. G_mt])^T row-major, one SpMM over the terms, back to column-major (compute_MM's route)
        B = np.hstack([G[t] for t in range(mt)])
        XT = dense.gemm_ts(Yd, B, rowmajor=True, k=r)
        ZT = torch.empty((self.n, q), dtype=CDT, device="cuda")
        check(lib.nep_spmm_terms(self.nep.dev.h, q, c_vp(XT.data_ptr()), q * mt, c_vp(ZT.data_ptr()), q, stream_ptr()))
        if beta == 0:
            out[:q].copy_(ZT.t())
            if alpha != 1:
                out[:q].mul_(complex(alpha))
        else:
            out[:q].mul_(complex(beta)).add_(ZT.t(), alpha=complex(alpha))
        self.composed_calls += 1
        return out

    def gram_norm(self, Rd):
        """||R||_2 of a device (p, n) block from its p x p Gram matrix"""
        p = self.p
        Gd = torch.empty((p, p), dtype=CDT, device="cuda")
        check(lib.nep_zgemm_sk(2, 0, p, p, self.n, cd(1.0), c_vp(Rd.data_ptr()), self.n, c_vp(Rd.data_ptr()), self.n, cd(0.0),
                               c_vp(Gd.data_ptr()), p, self.ksplit, c_vp(self.skwork.data_ptr()), stream_ptr()))
        G = Gd.cpu().numpy().T
        G = 0.5 * (G + G.conj().T)
        if not np.all(np.isfinite(G)):
            return np.inf
        return float(np.sqrt(max(np.linalg.eigvalsh(G)[-1], 0.0)))

    def wh(self, Wd, Bd, k):
        """T[j] = W_j^H B[:, :k] (host, (l, p, k)) for all j from one product of the stacked W = [W_0 .. W_(l-1)] with B: Wd is the
        device (p, n p) tensor of the np x p block; column c p + j of the n x (p l) view (leading dimension n) is W_j[:, c]"""
        p, n = self.p, self.n
        Cd = torch.empty((k, p * p), dtype=CDT, device="cuda")
        check(lib.nep_zgemm_sk(2, 0, p * p, k, n, cd(1.0), c_vp(Wd.data_ptr()), n, c_vp(Bd.data_ptr()), n, cd(0.0),
                               c_vp(Cd.data_ptr()), p * p, self.ksplit, c_vp(self.skwork.data_ptr()), stream_ptr()))
        return Cd.cpu().numpy().reshape(k, p, p).transpose(2, 1, 0)

    def residual(self, S, Xd, out):
        return self.blockprod(Xd, tables_fS(self.fv, S), out)


def _form_Vl(Xd, S, Vd):
    """Vd (p, n p) = [X; X S; ...; X S^(p-1)] on the device"""
    p, n = Xd.shape
    Sj = np.eye(p, dtype=np.complex128)
    V3 = Vd.view(p, p, n)                                                 # [column, block, row]
    for j in range(p):
        if j == 0:
            V3[:, 0, :].copy_(Xd)
        else:
            Sj = Sj @ S
            V3[:, j, :].copy_(dense.gemm_ts(Xd, Sj))
    return Vd


def _qr_inplace(Vd, p):
    """thin QR of the device (p, rows) block by nep_orth_qr_dev; returns the host R"""
    rows = Vd.shape[1]
    outs = torch.zeros((p, p + 2), dtype=CDT, device="cuda")
    check(lib.nep_orth_qr_dev(c_vp(Vd.data_ptr()), rows, rows, p, c_vp(outs.data_ptr()), stream_ptr()))
    oh = outs.cpu().numpy()
    R = np.zeros((p, p), dtype=np.complex128)
    for j in range(p):
        if int(oh[j, j + 1].imag) & 2:
            raise np.linalg.LinAlgError("blocknewton: Vl(X, S) lost rank in column %d" % j)
        R[:j, j] = oh[j, :j]
        R[j, j] = oh[j, j].real
    return R


def _newtonstep(w, S, XXd, Wd, RTd, linsolvercreator, bordered, refine, dXd):
    """one correction for the upper triangular S (Kressner (20)-(22), :147-216).  XXd: device (p + 1, n), rows 0 .. p - 1 = X (in
    the Schur basis), row p is scratch for dx_i; RTd (p, n) is overwritten; dXd (p, n) receives dX.  Returns the host dS."""
    from .linsolvers import create_linsolver, DeviceLU
    nep, n, p, fv = w.nep, w.n, w.p, w.fv
    l = p
    Xd = XXd[:p]
    RV = np.zeros((p, p), dtype=np.complex128)
    dS = np.zeros((p, p), dtype=np.complex128)
    fS = tables_fS(fv, S)
    WX = w.wh(Wd, Xd, p)                                                  # W_j^H X for all j, once per step
    solvers = [None] * p
    if bordered == "eliminate":
        for i in range(p):                                                # all up front: the numeric factorisations go out together
            try:
                solvers[i] = create_linsolver(linsolvercreator, nep, complex(S[i, i]))
                w.factorizations += 1
                w.device_factorizations += 1 if getattr(getattr(solvers[i], "lu", None), "device_factorized", False) else 0
            except np.linalg.LinAlgError:                                 # SingularException: this column takes the whole matrix
                solvers[i] = None
                w.whole_fallbacks += 1
    Wh = None
    Bd = torch.empty((p + 1, n), dtype=CDT, device="cuda")                # [RT_i T12], then [y1 Y2]
    r1 = torch.empty((1, n), dtype=CDT, device="cuda")
    for i in range(p):
        s = complex(S[i, i])
        D, P = constraint_tables(S, i, l)
        spow = s ** np.arange(l)
        T12tab = tables_T12(fv, S, s)
        T22 = sum((WX[j] @ D[j] for j in range(1, l)), np.zeros((p, p), dtype=np.complex128))
        Bd[0].copy_(RTd[i])
        w.blockprod(Xd, T12tab, Bd[1:])
        dx = XXd[p]
        if solvers[i] is not None:
            Yd = solvers[i].solve_dev(Bd)
            C = np.einsum("j,jck->ck", spow, w.wh(Wd, Yd, p + 1))         # T21 [y1 Y2]
            Sc = T22 - C[:, 1:]
            x2 = np.linalg.solve(Sc, RV[:, i] - C[:, 0])
            dense.gemm_ts(Yd, np.concatenate([[1.0], -x2]).reshape(p + 1, 1), out=dx.reshape(1, n))
            t21x1 = C[:, 0] - C[:, 1:] @ x2
            for _ in range(int(refine)):
                r1.copy_(RTd[i:i + 1])
                w.blockprod(XXd, tables_refine(fv, T12tab, s, x2), r1, alpha=-1.0, beta=1.0)
                r2 = RV[:, i] - t21x1 - T22 @ x2
                z1 = solvers[i].solve_dev(r1)
                Yd[0].copy_(z1.reshape(-1))
                c0 = np.einsum("j,jck->ck", spow, w.wh(Wd, Yd, 1))[:, 0]
                d2 = np.linalg.solve(Sc, r2 - c0)
                d1 = dense.gemm_ts(Yd, np.concatenate([[1.0], -d2]).reshape(p + 1, 1))
                dense.axpy(1.0, d1, dx, n)
                t21x1 = t21x1 + c0 - C[:, 1:] @ d2
                x2 = x2 + d2
        else:
            if Wh is None:
                Wh = to_host(Wd)                                          # np x p
            T21 = sum(spow[j] * Wh[j * n:(j + 1) * n].conj().T for j in range(l))
            M = nep.compute_Mder(s)
            TT = sp.bmat([[sp.csc_matrix(M), sp.csc_matrix(to_host(Bd[1:]))], [sp.csc_matrix(T21), sp.csc_matrix(T22)]], format="csc")
            lu = DeviceLU(TT.astype(np.complex128), expected_solves=1)
            w.factorizations += 1
            w.device_factorizations += 1 if getattr(lu, "device_factorized", False) else 0
            rhs = torch.cat([RTd[i], torch.from_numpy(np.ascontiguousarray(RV[:, i])).to("cuda")]).reshape(1, n + p)
            sol = lu.solve(rhs)
            dx.copy_(sol[0, :n])
            x2 = sol[0, n:].cpu().numpy()
        dS[:, i] = x2
        dXd[i].copy_(dx)
        if i < p - 1:
            w.blockprod(XXd, tables_update21(fv, fS, S, x2, i), RTd[i + 1:], alpha=-1.0, beta=1.0)          # (21)
            Wdx = w.wh(Wd, dx.reshape(1, n), 1)                           # W_j^H dx_i
            E = update22_tables(S, x2, i, l)
            for j in range(1, l):                                         # (22)
                RV[:, i + 1:] -= np.outer(Wdx[j][:, 0], P[j][i, i + 1:]) + WX[j] @ E[j][:, i + 1:]
    return dS


def blocknewton(nep, S=None, X=None, errmeasure=None, tol=EPS * 100, maxit=10, logger=0, armijo_factor=1, armijo_max=5, *,
                linsolvercreator=None, bordered="eliminate", refine=2, info=None, _blockprod="fused"):
    """Block Newton method, src/method_blocknewton.jl:48-140.  S (p x p) and X (n x p) start the iteration (defaults zeros(2, 2)
    and eye(n, 2)); errmeasure(S, X) receives host arrays (default ||compute_MM(S, X)||_2, evaluated on the device).  Returns
    (S, X) on the host; raises NoConvergenceException(S, X, err, msg) after maxit iterations.  bordered: "eliminate" (block
    elimination through a linear solver of M(s_i) with `refine` refinement steps) or "whole" (the bordered matrix factorised as
    the reference does).  info (a dict) receives iters, errhist, armijo, blockprod_calls, composed_calls, factorizations,
    device_factorizations, whole_fallbacks and refine."""
    S, X, n, p = check_arguments(nep, S, X, bordered, refine, _blockprod)
    _lib.require_gpu()
    from .linsolvers import FactorizeLinSolverCreator
    if linsolvercreator is None:
        linsolvercreator = FactorizeLinSolverCreator()
    w = _Work(nep, n, p, _blockprod == "composed")
    XXd = torch.empty((p + 1, n), dtype=CDT, device="cuda")               # [X dx]
    Xd = to_dev(X)
    Wd = _form_Vl(Xd, S, torch.empty((p, n * p), dtype=CDT, device="cuda"))          # :72-77: not orthonormalised before the first step
    Resd = torch.empty((p, n), dtype=CDT, device="cuda")
    dXd = torch.empty((p, n), dtype=CDT, device="cuda")
    Xtd = torch.empty((p, n), dtype=CDT, device="cuda")
    errhist, armijo = [], []

    def measure(S_, Xd_, out):
        if errmeasure is None:
            return w.gram_norm(w.residual(S_, Xd_, out))
        return float(errmeasure(S_.copy(), to_host(Xd_)))

    def fill_info(k):
        if info is not None:
            info.update(iters=k, errhist=list(errhist), armijo=list(armijo), blockprod_calls=w.blockprod_calls,
                        composed_calls=w.composed_calls, factorizations=w.factorizations,
                        device_factorizations=w.device_factorizations, whole_fallbacks=w.whole_fallbacks, refine=int(refine),
                        bordered=bordered, n=n, p=p)

    err0 = np.inf
    for k in range(maxit):
        err0 = measure(S, Xd, Resd)
        errhist.append(err0)
        if logger:
            print("blocknewton: iteration %d, err = %.6e" % (k + 1, err0))
        if err0 < tol:
            fill_info(k)
            return S, to_host(Xd)
        if errmeasure is not None:
            w.residual(S, Xd, Resd)
        RR, QQ = sla.schur(S, output="complex")
        dense.gemm_ts(Xd, QQ, out=XXd[:p])
        RTd = dense.gemm_ts(Resd, QQ)
        dSt = _newtonstep(w, RR, XXd, Wd, RTd, linsolvercreator, bordered, refine, dXd)
        DXd = dense.gemm_ts(dXd, -QQ.conj().T)                            # the step: -dX, -dS
        DS = -QQ @ dSt @ QQ.conj().T
        scale, j = 1.0, 0
        Xtd.copy_(Xd); dense.axpy(1.0, DXd, Xtd, n * p)
        if armijo_factor < 1:                                             # armijo_rule_block, :233-244
            while j < armijo_max and measure(S + scale * DS, Xtd, Resd) > err0:
                j += 1
                scale *= armijo_factor
                Xtd.copy_(Xd); dense.axpy(scale, DXd, Xtd, n * p)
            if logger and j:
                print("blocknewton:  Armijo scaling=%g" % scale)
        armijo.append(j)
        St = S + scale * DS
        _form_Vl(Xtd, St, Wd)
        R = _qr_inplace(Wd, p)
        Ri = np.linalg.inv(R)
        dense.gemm_ts(Xtd, Ri, out=Xd)
        S = R @ St @ Ri
    fill_info(maxit)
    raise NoConvergenceException(S, to_host(Xd), err0, "Number of iterations exceeded. maxit=%d." % maxit)
