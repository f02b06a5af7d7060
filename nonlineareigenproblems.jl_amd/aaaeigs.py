"""AAAeigs on the device backend: set-valued AAA rational approximation of the nonlinear part of an SPMF-type NEP, the compact
(CORK) linearisation built on it and a compact rational Krylov iteration -- keyword surface of src/method_AAAeigs.jl:183-202.

Host side (NumPy, not a hot path: about 10^3 sample points by a handful of functions): `svAAA` (:469-721), `reval` and `get_prz`
(:724-779), `AAACorkLinearization`, `AAAPencil`, `get_compact_pencil` (:5-120) and `AAASolutionDetails` (:782-800).

Device side, per step of the CORK iteration (:270-395), with the basis Q (n x r) and the coefficient tensor U (r x k x j) resident:
   u_c = U_j C_sigma                      nep_cork_expand without the rank-1 term      (:283-287)
   v   = sum_i A_i (Q u_c[:, i])          K1, nep_mlincomb_dev with dC = u_c            (:288-292)
   v   = M(sigma)^-1 v                    K5 with the cached factorisation of the shift (:294-295)
   level 1 Gram-Schmidt on Q              K6, nep_orth_dev: the row [Q^H v; ||v_perp||] stays on the device   (:301-328)
   Uhat = (alpha u1) g_sigma^T + U_j G_sigma      nep_cork_expand with the rank-1 term  (:332-339)
   level 2 Gram-Schmidt on U              K6 on U seen as an (R k) x j column-major matrix                   (:341-358)
The tables of a shift come from the pencil (A, B) = (compactA, compactB), l = dt + s, Mext = [e_1, A[:, l:] - sigma B[:, l:]]:
   Y = Mext^-1 (sigma B[:, :l] - A[:, :l]),   C_sigma = B[:, :l] + B[:, l:] Y[1:, :],
   g_sigma = (Mext^-1)[0, :],                 G_sigma = B[:, l:] (Mext^-1)[1:, :],
so that W / Mext of :332-339 with W = [u1, U_j B[:, l:]] is u1 g_sigma^T + U_j G_sigma.  They are formed once per distinct shift
on the host and uploaded before the loop.  The scaling alpha = phi0[0] / sum(phi0) of :296-300 is not applied to the n-vector:
alpha v = Q (alpha h) + q (alpha ||v_perp||), so it multiplies the rank-1 term inside the kernel (the new basis vector differs
from the reference's by the phase of alpha).

K6's DGKS rule (at most two passes, decided on the device) is not the reference's "up to three passes while the norm drops below
1/sqrt(2)": the iterates differ from the reference's in rounding, so error histories and iteration counts are not comparable.
"""
import numpy as np
import scipy.linalg as sla
import scipy.sparse as sp
import torch

from . import dense
from ._lib import lib, check, c_vp, cd
from .errmeasure import ResidualErrmeasure, estimate_errors
from .exceptions import NoConvergenceException
from .linsolvers import FactorizeLinSolverCreator, LinSolverCache
from .nep import CDT, AbstractSPMF, PEP, SumNEP, SPMFDevice, require_pure_spmf, to_dev, to_host, stream_ptr

EPS = np.finfo(float).eps
CORK_KMAX = 256                       # nep_cork_expand: 1 <= k, c <= 256


# ================================================================================================================================
# rational interpolants in barycentric form
def reval(lam, z, fz, w):
    """src/method_AAAeigs.jl:724-747: the rational interpolants defined by (z, fz, w) at the points lam; r(inf) = sum(w fz) / sum(w),
    a support point returns its function values, NaN stays NaN"""
    lam = np.atleast_1d(np.asarray(lam, dtype=np.complex128)).reshape(-1)
    z = np.asarray(z, dtype=np.complex128); w = np.asarray(w, dtype=np.complex128)
    fz = np.asarray(fz, dtype=np.complex128).reshape(len(z), -1)
    with np.errstate(all="ignore"):
        C = 1.0 / (lam[:, None] - z[None, :])
        r = (C @ (w[:, None] * fz)) / (C @ w)[:, None]
        inf = np.isinf(lam)
        if np.any(inf):
            r[inf, :] = (np.sum(w[:, None] * fz, axis=0) / np.sum(w))[None, :]
    for i, j in zip(*np.nonzero(np.isnan(r))):
        if not np.isnan(lam[i]) and np.any(lam[i] == z):          # NaN = inf / inf at a support point
            r[i, j] = fz[np.flatnonzero(lam[i] == z)[0], j]
    return r


def _finite_geneig(E, B):
    ev = sla.eig(E, B, right=False)
    return ev[np.isfinite(ev)]


def _poles_residues(z, fz, w):
    """poles by the generalised eigenvalue problem of :618-623 / :753-759, residues by the four-point Cauchy integral of :625-632"""
    m = len(z)
    B = np.eye(m + 1, dtype=np.complex128); B[0, 0] = 0.0
    E = np.zeros((m + 1, m + 1), dtype=np.complex128)
    E[0, 1:] = w; E[1:, 0] = 1.0; E[1:, 1:] = np.diag(z)
    pol = _finite_geneig(E, B)
    dz = 1e-5 * np.array([1j, -1.0, -1j, 1.0])
    rv = reval((pol[:, None] + dz[None, :]).reshape(-1), z, fz, w)             # row p * 4 + q
    rsd = np.einsum("pqs,q->ps", rv.reshape(len(pol), 4, -1), dz) / 4.0
    return pol, rsd, E, B


def get_prz(z, fz, w):
    """src/method_AAAeigs.jl:750-779: poles, residues (poles x s) and zeros ((m + 1) x s, infinite ones included) of the interpolants"""
    z = np.asarray(z, dtype=np.complex128); w = np.asarray(w, dtype=np.complex128)
    fz = np.asarray(fz, dtype=np.complex128).reshape(len(z), -1)
    pol, rsd, E, B = _poles_residues(z, fz, w)
    zer = np.empty((len(z) + 1, fz.shape[1]), dtype=np.complex128)
    for i in range(fz.shape[1]):
        E[0, 1:] = w * fz[:, i]
        with np.errstate(all="ignore"):
            zer[:, i] = sla.eig(E, B, right=False)
    return pol, rsd, zer


# ================================================================================================================================
def svAAA(nep, Z, mmax=100, tol=EPS * 1e3, cleanup=True, tol_cln=None, return_details=False, logger=0, weighted=False,
          u0_weight=None):
    """src/method_AAAeigs.jl:469-721: set-valued (or weighted) AAA approximation of the functions of `nep` on the sample points Z.
    Returns (z, fz, w, err, pol, rsd, zer): support points, function values there (m x s), barycentric weights, the error of every
    iteration, and poles, residues and zeros when `return_details`.

    As in the reference the QR factorisation of the Loewner matrix is updated per support point (:566-603: the rows of the new
    support point leave Q through a Cholesky factor of I - q^H q, the new column enters by Gram-Schmidt with the DGKS rule) and the
    weights are the last right singular vector of its m x m triangular factor.  Differences: when that Cholesky factor does not
    exist in floating point the factorisation is rebuilt from the Loewner matrix (the reference throws); generalised eigenvalues
    that are not finite are dropped (the reference drops NaN, which is what its complex division by zero gives); when several
    Froissart doublets are found in one iteration the support points are removed by their original index (:647-655 index into the
    shrinking vector, which is only right for one doublet)."""
    if tol_cln is None:
        tol_cln = min(EPS, tol)
    fv = nep.get_fv()
    Z = np.asarray(Z, dtype=np.complex128).reshape(-1)
    Z = Z[np.isfinite(Z)]
    M, s = len(Z), len(fv)
    F = np.column_stack([f.values(Z) for f in fv]).astype(np.complex128)
    if weighted:
        Av = nep.get_Av()
        n = nep.size(1)
        u = np.ones(n, dtype=np.complex128) if u0_weight is None else np.asarray(u0_weight, dtype=np.complex128)
        u = u / np.linalg.norm(u)
        uj = np.column_stack([np.asarray(A @ u).reshape(-1) for A in Av])
        beta = float(np.max(np.linalg.norm(uj @ F.T, axis=0)))
        nrm = np.array(nep.fro_norms(), dtype=float)                       # norm(Av[i]): Frobenius
        F = F * nrm[None, :]
        scaleF = 1.0 / nrm
        maxF = np.max(np.abs(F), axis=0)
    else:
        scaleF = np.max(np.abs(F), axis=0)
        F = F / scaleF[None, :]

    def error_of(R):
        res = np.abs(F - R)
        maxres = res.max(axis=0)
        col = int(np.argmax(maxres))
        row = int(np.argmax(res[:, col]))
        return (float(maxres.sum()) / beta if weighted else float(res[row, col])), row

    err = []
    z = []; ind = []
    w = np.zeros(0, dtype=np.complex128)
    fzs = np.zeros((mmax, s), dtype=np.complex128)
    H = np.zeros((mmax, mmax), dtype=np.complex128); S = np.zeros((mmax, mmax), dtype=np.complex128)
    Q = np.zeros((M * s, mmax), dtype=np.complex128)
    C = np.zeros((M, mmax), dtype=np.complex128)
    R = np.tile(F.mean(axis=0), (M, 1))
    fz = fzs[:0]
    rows_of = lambda i: np.arange(s) * M + i                               # rows of sample point i in the stacked (M s) vectors

    def loewner_column(mm):
        return (C[:, mm, None] * (F - fzs[mm][None, :])).reshape(-1, order="F")

    for m in range(1, mmax + 1):
        e, locz = error_of(R)
        err.append(e)
        if e <= tol:
            fz = scaleF[None, :] * fzs[:m - 1]
            break
        z.append(Z[locz]); ind.append(locz)
        fzs[m - 1] = F[locz]
        with np.errstate(all="ignore"):
            C[:, m - 1] = 1.0 / (Z - Z[locz])
        C[ind, m - 1] = 0.0
        v = loewner_column(m - 1)
        k = m - 1
        rebuilt = False
        if k > 0:
            # the rows of the new support point leave the factorisation (:567-576)
            q = Q[rows_of(locz), :k] @ S[:k, :k]
            ee = np.eye(k) - q.conj().T @ q
            try:
                Si = np.linalg.cholesky(ee).conj().T                       # upper factor: ee = Si^H Si
                H[:k, :k] = Si @ H[:k, :k]
                S[:k, :k] = sla.solve_triangular(Si.T, S[:k, :k].T, lower=True).T          # S / Si
                S[k, :k] = 0.0; S[:k, k] = 0.0
                Q[rows_of(locz), :k] = 0.0
            except np.linalg.LinAlgError:
                C[locz, :k] = 0.0
                Lm = np.column_stack([loewner_column(mm) for mm in range(m)])
                Qf, Rf = np.linalg.qr(Lm)
                Q[:, :m] = Qf; H[:m, :m] = Rf; S[:m, :m] = np.eye(m)
                rebuilt = True
        C[locz, :k] = 0.0                                                  # (C[ind, m] .= 0 of the earlier columns: the row is a support row now)
        if not rebuilt:
            S[k, k] = 1.0
            # Gram-Schmidt with the DGKS rule (:579-603)
            nv = np.linalg.norm(v)
            h = S[:k, :k].conj().T @ (Q[:, :k].conj().T @ v)
            H[:k, k] = h
            v = v - Q[:, :k] @ (S[:k, :k] @ h)
            H[k, k] = np.linalg.norm(v)
            ii = 0
            while ii < 3 and H[k, k].real < nv / np.sqrt(2.0):
                hh = S[:k, :k].conj().T @ (Q[:, :k].conj().T @ v)
                H[:k, k] += hh
                v = v - Q[:, :k] @ (S[:k, :k] @ hh)
                nv = H[k, k].real
                H[k, k] = np.linalg.norm(v)
                ii += 1
            Q[:, k] = v / H[k, k]
        w = np.linalg.svd(H[:m, :m])[2][-1].conj()
        with np.errstate(all="ignore"):
            R = (C[:, :m] @ (w[:, None] * fzs[:m])) / (C[:, :m] @ w)[:, None]
        R[ind, :] = F[ind, :]

        if cleanup and m > 1:                                              # Froissart doublets (:616-687)
            pol, rsd, _, _ = _poles_residues(np.array(z), fzs[:m], w)
            maxRsd = np.max(np.abs(rsd / maxF[None, :] if weighted else rsd), axis=1) if len(pol) else np.zeros(0)
            spurious = np.flatnonzero(maxRsd < tol_cln)
            if len(spurious) > 0:
                left = list(range(m))
                ind_sp = []
                for ip in spurious:
                    if len(left) <= 1:
                        break
                    locj = left[int(np.argmin(np.abs(np.array(z)[left] - pol[ip])))]
                    left.remove(locj); ind_sp.append(ind[locj])
                z = [z[i] for i in left]; ind = [ind[i] for i in left]
                zl = np.array(z)
                with np.errstate(all="ignore"):
                    C[np.ix_(ind_sp, left)] = 1.0 / (Z[ind_sp][:, None] - zl[None, :])
                ind_Z = np.setdiff1d(np.arange(M), ind)
                Cv = C[np.ix_(ind_Z, left)]
                Lm = np.vstack([Cv * (F[ind_Z, j][:, None] - fzs[left, j][None, :]) for j in range(s)])
                w = np.linalg.svd(Lm, full_matrices=False)[2][-1].conj()
                with np.errstate(all="ignore"):
                    R = (C[:, left] @ (w[:, None] * fzs[left])) / (C[:, left] @ w)[:, None]
                R[ind, :] = F[ind, :]
                err.append(error_of(R)[0])
                fz = scaleF[None, :] * fzs[left]
                break

        if m == mmax:
            err.append(error_of(R)[0])
            fz = scaleF[None, :] * fzs[:m]

    z = np.array(z, dtype=np.complex128); fz = np.array(fz, dtype=np.complex128)
    keep = w != 0                                                          # support points with zero weight (:704-710)
    if not np.all(keep):
        z, fz, w = z[keep], fz[keep], w[keep]
    if return_details:
        pol, rsd, zer = get_prz(z, fz, w)
    else:
        pol = np.zeros(0, dtype=np.complex128); rsd = np.zeros(0, dtype=np.complex128); zer = np.zeros(0, dtype=np.complex128)
    return z, fz, w, np.array(err), pol, rsd, zer


# ================================================================================================================================
class AAACorkLinearization:
    """src/method_AAAeigs.jl:5-27: the parameters of the svAAA call behind an AAAPencil"""

    def __init__(self, Z, mmax=100, tol=EPS * 1e3, cleanup=True, tol_cln=None, return_details=False, logger=0, weighted=False):
        self.Z, self.mmax, self.tol, self.cleanup = Z, mmax, tol, cleanup
        self.tol_cln = min(EPS, tol) if tol_cln is None else tol_cln
        self.return_details, self.logger, self.weighted = return_details, logger, weighted


def _iszero(A):
    return (A.count_nonzero() == 0) if sp.issparse(A) else not np.any(A)


def get_compact_pencil(d, s, m, z, fz, w, NNZ):
    """src/method_AAAeigs.jl:91-120: compactA = [P_A^T M^T], compactB = [P_B^T N^T] (dense, k x (dt + s + k - 1)) for the three
    shapes: no polynomial part, constant polynomial part only, polynomial plus nonlinear part"""
    z = np.asarray(z, dtype=np.complex128); w = np.asarray(w, dtype=np.complex128)
    fz = np.asarray(fz, dtype=np.complex128).reshape(m, s)
    dt = len(NNZ)

    def bidiag(dg, sub):                                                   # spdiagm(m, m-1, 0 => dg, -1 => sub)
        T = np.zeros((m, m - 1), dtype=np.complex128)
        i = np.arange(m - 1)
        T[i, i] = dg; T[i + 1, i] = sub
        return T
    TA = bidiag(-w[1:] * z[:-1], w[:-1] * z[1:])
    TB = bidiag(-w[1:], w[:-1])
    if dt == 0:
        A = np.hstack([fz, TA])
        B = np.hstack([np.zeros((m, s)), TB])
    elif d == 0:
        A = np.zeros((1 + m, 1 + s + m), dtype=np.complex128); B = np.zeros_like(A)
        A[1:, 1:1 + s] = fz; A[1:, 1 + s:s + m] = TA; A[1:, s + m] = 1.0
        A[0, 0] = 1.0; A[0, -1] = -1.0
        B[1:, 1 + s:s + m] = TB
    else:
        ncol = dt + s + d + m - 1
        A = np.zeros((d + m, ncol), dtype=np.complex128); B = np.zeros_like(A)
        for c_, deg in enumerate(NNZ[:-1]):                                # sparse(NNZ[1:end-1] .+ 1, 1:dt-1, ones, d, dt-1)
            A[deg, c_] = 1.0
        i = np.arange(d - 1)
        A[i + 1, dt + s + i] = 1.0                                         # spdiagm(d, d-1, -1 => ones) behind spzeros(d, s+1)
        A[d:, dt:dt + s] = fz
        A[d:, dt + s + d - 1:ncol - 1] = TA
        A[d:, ncol - 1] = 1.0
        A[0, ncol - 1] = -1.0
        B[i, dt + s + i] = 1.0                                             # spdiagm(d, d-1, 0 => ones) behind spzeros(d, dt+s)
        B[d:, dt + s + d - 1:ncol - 1] = TB
        B[d - 1, dt - 1] = -1.0
    return A, B


class AAAPencil:
    """src/method_AAAeigs.jl:30-88: the compact pencil of the AAA linearisation.  d: degree of the polynomial part, s: number of
    nonlinear terms, m: degree of the rational approximation, PPCC / ppff: the matrices and functions [polynomial terms in NNZ
    order; nonlinear terms], NNZ: the degrees of the non-zero polynomial coefficients.

    SumNEP(PEP, spmf) and SumNEP(spmf, PEP) are recognised as the reference recognises SPMFSumNEP{PEP, S} / {S, PEP}; every other
    AbstractSPMF is fully nonlinear (d = 0, NNZ empty).  Trailing zero coefficients of the PEP lower d (the loop of :56-59 pops a
    non-zero degree for every trailing zero; the degrees of the non-zero coefficients are what the pencil needs)."""

    def __init__(self, nep, is_):
        if not isinstance(nep, AbstractSPMF):
            raise TypeError("AAAPencil needs an AbstractSPMF")
        pep = None
        if isinstance(nep, SumNEP):
            if isinstance(nep.nep1, PEP):
                pep, nl = nep.nep1, nep.nep2
            elif isinstance(nep.nep2, PEP):
                pep, nl = nep.nep2, nep.nep1
        NNZ = []
        if pep is not None:
            Av_p, fv_p = pep.get_Av(), pep.get_fv()
            NNZ = [i for i, A in enumerate(Av_p) if not _iszero(A)]
        if NNZ:
            d = NNZ[-1]
            PPCC = [Av_p[i] for i in NNZ] + list(nl.get_Av())
            ppff = [fv_p[i] for i in NNZ] + list(nl.get_fv())
        else:
            nl = nep if pep is None else nl
            d = 0
            PPCC = list(nl.get_Av()); ppff = list(nl.get_fv())
        self.approximated = nl
        # PPCC is term by term what nep.get_Av() lists: the NEP's own device object serves the iteration
        self.same_terms = pep is None or (pep is nep.nep1 and NNZ == list(range(len(Av_p))))
        s = len(nl.get_Av())
        z, fz, w, err, pol, rsd, zer = svAAA(nl, is_.Z, mmax=is_.mmax, tol=is_.tol, cleanup=is_.cleanup, tol_cln=is_.tol_cln,
                                              return_details=is_.return_details, logger=is_.logger, weighted=is_.weighted)
        m = len(z)
        self.d, self.s, self.m, self.PPCC, self.ppff, self.NNZ = d, s, m, PPCC, ppff, NNZ
        self.zfw, self.err, self.prz = [z, fz, w], err, [pol, rsd, zer]
        self.compactA, self.compactB = get_compact_pencil(d, s, m, z, fz, w, NNZ)


class AAASolutionDetails:
    """src/method_AAAeigs.jl:782-800: degree of the approximation, [z, fz, w], [pol, rsd, zer], the errors of the svAAA iterations,
    Ritz values and residuals of every iteration (sorted by residual, NaN-padded columns) and the iteration count"""

    def __init__(self, m_appr=0, zfw=None, prz=None, err_appr=None, Lam=None, Res=None, conv_it=0):
        self.m_appr = m_appr
        self.zfw = [] if zfw is None else zfw
        self.prz = [] if prz is None else prz
        self.err_appr = np.zeros(0) if err_appr is None else err_appr
        self.Lam = np.zeros((0, 0), dtype=np.complex128) if Lam is None else Lam
        self.Res = np.zeros((0, 0)) if Res is None else Res
        self.conv_it = conv_it


def cork_shift_tables(A, B, l, sigma):
    """the tables of one shift (module docstring): (C_sigma (k x l), g_sigma (k), G_sigma (k x k)) with
    Mext = [e_1, A[:, l:] - sigma B[:, l:]]"""
    k = A.shape[0]
    Mext = np.zeros((k, k), dtype=np.complex128)
    Mext[0, 0] = 1.0
    Mext[:, 1:] = A[:, l:] - sigma * B[:, l:]
    Minv = np.linalg.inv(Mext)
    Y = Minv @ (sigma * B[:, :l] - A[:, :l])
    return B[:, :l] + B[:, l:] @ Y[1:, :], Minv[0, :].copy(), B[:, l:] @ Minv[1:, :]


def _cork_expand(r, k, c, U, ldu, G, ldg, u, g, alpha, out, ldo):
    check(lib.nep_cork_expand(r, k, c, c_vp(U.data_ptr()), ldu, c_vp(G.data_ptr()), ldg,
                              c_vp(u.data_ptr()) if u is not None else None, c_vp(g.data_ptr()) if g is not None else None,
                              cd(alpha), c_vp(out.data_ptr()), ldo, stream_ptr()))


# ================================================================================================================================
def AAAeigs(nep, Z, logger=0, mmax=100, neigs=6, maxit=None, shifts=(), linsolvercreator=None, tol=EPS * 1e6, tol_appr=EPS * 1e3,
            v0=None, errmeasure=None, weighted=False, cleanup_appr=True, tol_cln=None, return_details=False, check_error_every=10,
            inner_logger=0, info=None):
    """src/method_AAAeigs.jl:183-416.  Returns (Lam, X, res, details): the `neigs` Ritz pairs of smallest error measure once `neigs`
    of them are below `tol`, and an AAASolutionDetails (empty unless `return_details`).  Raises NoConvergenceException(Lam, Q, res,
    msg) when maxit steps do not give `neigs` converged pairs (neigs = inf: run maxit steps and return every Ritz pair).

    With n > maxit the basis cannot saturate and nothing is read back between two convergence checks; a breakdown flag of K6 found
    when its rows are read raises ArithmeticError.  With n <= maxit the row of the level-1 Gram-Schmidt is read in every step and
    r = n, or a new norm <= eps, means that Q gains no column (`rnew = r`, :316-328).  `info` (a dict) receives r, the number of
    cached factorisations and the launches per step.  k = d + m > 256 is refused with a ValueError (lower `mmax`)."""
    if not isinstance(nep, AbstractSPMF):
        raise TypeError("AAAeigs needs an AbstractSPMF")
    require_pure_spmf(nep, "AAAeigs")
    if maxit is None:
        maxit = int(min(max(10 * neigs, 30), 100))
    n = nep.size(1)
    shifts = np.asarray(shifts, dtype=np.complex128).reshape(-1)
    if len(shifts) == 0:
        shifts = np.zeros(1, dtype=np.complex128)
    sigma = np.resize(shifts, maxit)                                       # :215-219: the shifts repeated cyclically
    distinct = list(dict.fromkeys(complex(s_) for s_ in shifts))
    if linsolvercreator is None:
        linsolvercreator = FactorizeLinSolverCreator(max_factorizations=min(len(distinct), 10))
    if errmeasure is None:
        errmeasure = ResidualErrmeasure(nep)
    if tol_cln is None:
        tol_cln = min(EPS, tol_appr)

    is_ = AAACorkLinearization(Z, mmax=mmax, tol=tol_appr, weighted=weighted, cleanup=cleanup_appr, tol_cln=tol_cln,
                               return_details=return_details, logger=inner_logger)
    L = AAAPencil(nep, is_)
    d, dt, m, s = L.d, len(L.NNZ), L.m, L.s
    k = d + m + (1 if d == 0 and dt != 0 else 0)
    l = dt + s
    if k > CORK_KMAX or l > CORK_KMAX:
        raise ValueError("AAAeigs: the linearisation has k = d + m = %d columns (l = %d terms), the device kernel takes at most %d: "
                         "lower mmax (now %d)" % (k, l, CORK_KMAX, mmax))
    A, B = L.compactA, L.compactB
    z_, w_ = L.zfw[0], L.zfw[2]

    # ---- device state
    R = maxit + 1
    kdev = nep.dev if L.same_terms else SPMFDevice(L.PPCC)        # (a dropped zero coefficient, or SumNEP(spmf, PEP): own term order)
    Q = torch.zeros((R, n), dtype=CDT, device="cuda")
    U = torch.zeros((R, R * k), dtype=CDT, device="cuda")                 # slab j: entry (rho, c) at rho + R c
    uc = torch.zeros((l, R), dtype=CDT, device="cuda")
    tmp = torch.empty(n, dtype=CDT, device="cuda")
    HQ = torch.zeros((maxit, R + 2), dtype=CDT, device="cuda")            # rows of the level-1 Gram-Schmidt: [Q^H v; beta; flags]
    HU = torch.zeros((maxit, R + 2), dtype=CDT, device="cuda")            # rows of the level-2 Gram-Schmidt: column j of H
    H = np.zeros((R, maxit), dtype=np.complex128); K = np.zeros((R, maxit), dtype=np.complex128)
    tables = {}
    for sg in distinct:
        Cs, gs, Gs = cork_shift_tables(A, B, l, sg)
        if dt == 0:                                                        # first basis function phi0 != 1 (:296-300)
            phi0 = w_ / (sg - z_)
            alpha = complex(phi0[0] / np.sum(phi0))
        else:
            alpha = 1.0 + 0.0j
        if not (np.all(np.isfinite(Cs)) and np.all(np.isfinite(Gs)) and np.isfinite(alpha)):
            raise np.linalg.LinAlgError("AAAeigs: the extended pencil is singular at the shift %r" % (sg,))
        tables[sg] = (to_dev(Cs), to_dev(gs)[0], to_dev(Gs), alpha)
    if v0 is None or len(v0) != n:
        v0 = np.random.randn(n)
    v0 = np.asarray(v0, dtype=np.complex128)
    Q[0].copy_(to_dev(v0 / np.linalg.norm(v0))[0])
    U[0, 0] = 1.0

    saturating = n <= maxit
    cache = LinSolverCache(nep, linsolvercreator)
    max_fact = min(len(distinct), 10)
    pending = []                                                           # steps whose rows of HQ / HU have not been read
    if return_details:
        Lam = np.full((maxit, maxit), np.nan, dtype=np.complex128); Res = np.full((maxit, maxit), np.nan)
    st = {"Lam": np.zeros(0, dtype=np.complex128), "X": np.zeros((n, 0), dtype=np.complex128), "res": np.zeros(0)}

    def flush():
        if not pending:
            return
        j0, j1 = pending[0], pending[-1]
        rows_u = HU[j0:j1 + 1].cpu().numpy()                               # (synchronises)
        rows_q = None if saturating else HQ[j0:j1 + 1].cpu().numpy()       # (read step by step when the basis can saturate)
        for j in pending:
            row = rows_u[j - j0]
            bad = int(row[j + 2].imag) & 2 or (rows_q is not None and int(rows_q[j - j0][r_of[j] + 1].imag) & 2)
            if bad or not np.all(np.isfinite(row[:j + 2])):
                raise ArithmeticError("orthogonalisation breakdown in AAAeigs step %d" % (j + 1))
            H[:j + 1, j] = row[:j + 1]; H[j + 1, j] = row[j + 1].real
            K[:j + 1, j] = H[:j + 1, j] * sigma[j]                         # :359-361
            K[j, j] += 1.0
            K[j + 1, j] = H[j + 1, j] * sigma[j]
        pending.clear()

    r_of = {}
    r = 1
    nconv = 0
    it = 0
    try:
        cache.prefetch(sigma[:3], keep_all=distinct)
        while it < maxit and nconv < neigs:
            j = it                                                         # slab j holds the continuation vector of this step
            sg = complex(sigma[it])
            Cs, gs, Gs, alpha = tables[sg]
            r_of[j] = r
            # ---- level 1
            _cork_expand(r, k, l, U[j], R, Cs, k, None, None, 1.0, uc, R)
            kdev.mlincomb_dev(uc, R, r, Q, n, tmp)
            w = Q[r]
            cache.solve_dev(sg, tmp, sg in cache.solvers or len(cache.solvers) < max_fact, out=w)
            dense.orthogonalize_and_normalize_dev(Q, w, r, HQ[j], rows=n, ldv=n, method=dense.DGKS)
            rnew = r + 1
            if saturating:
                row = HQ[j, :r + 2].cpu().numpy()
                if r >= n or not abs(alpha) * row[r].real > EPS:
                    rnew = r                                               # no new column: u1 has r entries
                elif int(row[r + 1].imag) & 2:
                    raise ArithmeticError("orthogonalisation breakdown in AAAeigs step %d" % (it + 1))
            # ---- level 2
            _cork_expand(rnew, k, k, U[j], R, Gs, k, HQ[j], gs, alpha, U[j + 1], R)
            dense.orthogonalize_and_normalize_dev(U, U[j + 1], j + 1, HU[j], rows=R * k, ldv=R * k, method=dense.DGKS)
            pending.append(j)
            it += 1
            # ---- convergence (:364-390)
            if return_details or it % check_error_every == 0 or it == maxit:
                flush()
                jj = j + 1
                lam, S = sla.eig(K[:jj, :jj], H[:jj, :jj])
                ok = np.isfinite(lam)
                res = np.full(jj, np.inf)
                X = None
                if np.any(ok):
                    U1 = U[:jj + 1, :rnew].cpu().numpy().T                  # U[0:rnew, 0, 0:jj+1]
                    Bm = U1 @ (H[:jj + 1, :jj] @ S[:, ok])
                    X = dense.gemm_ts(Q, Bm, rowmajor=True, k=rnew, rows=n, ldz=n)
                    res[ok] = np.abs(estimate_errors(errmeasure, lam[ok], X))
                    res[~np.isfinite(res)] = np.inf
                nconv = int(np.sum(res < tol))
                idx = np.argsort(res, kind="stable")
                if return_details:
                    Lam[:jj, it - 1] = lam[idx]; Res[:jj, it - 1] = res[idx]
                if it == maxit or nconv >= neigs:                          # the Ritz pairs of smallest error (:384-389)
                    cols = np.cumsum(ok) - 1                               # column of X that belongs to Ritz value i
                    keep = [i for i in idx[:int(min(jj, neigs))] if ok[i]]
                    st["Lam"] = lam[keep]; st["res"] = res[keep]
                    st["X"] = (to_host(dense.rowmajor_to_cols(X, cols[keep])) if keep else np.zeros((n, 0), dtype=np.complex128))
            r = rnew
        flush()
    finally:
        cache.close()
    if info is not None:
        lus = [getattr(s_, "lu", None) for s_ in cache.solvers.values()]
        info.update(r=r, it=it, maxit=maxit, k=k, l=l, d=d, dt=dt, m=m, nfact=len(cache.solvers), saturating=saturating,
                    own_device_terms=kdev is not nep.dev,
                    k5_launches=max([lu.launches_last_solve() for lu in lus if lu is not None], default=None))
    if nconv < neigs and neigs != np.inf:
        raise NoConvergenceException(st["Lam"], to_host(Q[:r]), st["res"], "AAAeigs: Number of iterations exceeded. maxit=%d." % maxit)
    details = AAASolutionDetails()
    if return_details:
        details = AAASolutionDetails(m, L.zfw, L.prz, L.err, Lam[:it, :it], Res[:it, :it], it)
    return st["Lam"], st["X"], st["res"], details
