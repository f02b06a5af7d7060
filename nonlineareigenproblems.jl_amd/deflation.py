"""Effenberger deflation of computed eigenpairs: the host-side mirror of src/nep_deflation.jl.

`deflate_eigpair(nep, lam, v, mode=...)` returns a NEP of size n0 + p that has the solutions of `nep` except the p pairs
held in the invariant pair (S0, V0); `get_deflated_eigpairs` gives those pairs back.  With X = V0 the deflated problem is

    Mt(lam) = [ M(lam)   M(lam) X (lam I - S0)^-1 ]
              [ X^H      0                        ]

in three representations (the reference's `mode`):

  "Generic"  DeflatedGenericNEP: derivatives by the binomial expansion of nep_deflation.jl:65-107.  For V = [V1; V2] with k
             columns, s = startder, K = k + s, e_i = i + s and W_d = (lam I - S0)^-(d+1):
                 Vn[:, j] = [j >= s] a_{j-s} V1[:, j-s] + X sum_{i : e_i >= j} G[i, j] W_{e_i - j} V2[:, i],
                 G[i, j]  = (-1)^(e_i - j) a_i e_i! / j!,                                     j = 0..K-1,
                 z_top    = sum_j M^(j)(lam) Vn[:, j],       z_bottom = a_0 X^H V1[:, 0]  (s == 0; zeros otherwise).
             Vn and z_bottom are one call of nep_defl_expand (csrc/deflate.hip), z_top is kernel K1 on the original NEP with a
             coefficient block of ones.  The W_d and G tables are p x p and k x K host work; V2 never leaves the device.
  "SPMF"     DeflatedSPMF: the deflated problem written as an SPMF (create_spmf_dnep, :210-269) -- the original terms padded to
             n0 + p, m p rank-one terms with the functions f_r(.) / (. - lam_i) (funcs.Resolvent; lam_i, x_i from eig(S0)) and
             the constant border.  All compute functions are the existing SPMF kernels.
  "MM"       DeflatedNEPMM: everything through compute_MM of the original NEP on the extended pair (:183-202).

The linear systems of the Newton-type drivers are solved with the bordered matrix assembled and factorised as a whole
(compute_Mder + DeviceLU, like any NEP): at a deflated eigenvalue M(sigma) is singular while Mt(sigma) is not, so block
elimination on the factors of M(sigma) is not an option.  jd_effenberger, whose shifts head for a NEW eigenvalue,
opts into block elimination with one solve of M(sigma): linsolvers.DeflatedNEPLinSolver.
"""
import math
import warnings

import numpy as np
import scipy.sparse as sp
import torch

from . import _lib, dense, funcs
from ._lib import lib, check, hptr, c_vp
from .nep import (NEP, AbstractSPMF, SPMF_NEP, SumNEP, LowRankMatrixAndFunction, LowRankFactorizedNEP, CDT, to_dev, to_host,
                  is_dev, pure_spmf, stream_ptr)

MODES = ("Auto", "Generic", "SPMF", "MM")
MAX_P, MAX_K = 32, 64              # limits of nep_defl_expand (include/nepmi355.h)


def normalize_schur_pair(S, V):
    """nep_deflation.jl:278-286: the pair (R S R^-1, Q) of the thin QR factorisation V = Q R -- the same invariant pair with
    orthonormal columns.  Returns new arrays (the reference's `!` form overwrites its arguments)."""
    S = np.array(S, dtype=np.complex128); V = np.array(V, dtype=np.complex128)
    if V.shape[1] > V.shape[0]:
        warnings.warn("Cannot normalize short and skinny V-matrices.")
        return S, V
    Q, R = np.linalg.qr(V)
    return np.linalg.solve(R.T, (R @ S).T).T, Q


def verify_deflate_mode(nep, mode):
    """nep_deflation.jl:289-313: resolves "Auto" and refuses the combinations the reference refuses"""
    if isinstance(nep, (DeflatedSPMF, DeflatedNEPMM, DeflatedGenericNEP)):
        for cls, name in ((DeflatedSPMF, "SPMF"), (DeflatedNEPMM, "MM"), (DeflatedGenericNEP, "Generic")):
            if isinstance(nep, cls) and mode in (name, "Auto"):
                return name
        raise ValueError("Unknown mode / type")
    if mode == "Auto":
        mode = "SPMF" if isinstance(nep, AbstractSPMF) else "Generic"
    if mode == "SPMF" and not isinstance(nep, AbstractSPMF):
        raise ValueError("SPMF-mode only possible for `AbstractSPMF`-NEPs")
    if mode not in MODES:
        raise ValueError("Unknown mode / type")
    return mode


def _extended_pair(dnep, lam, v):
    """the invariant pair of `dnep` with the eigenpair (lam, v) of `dnep` appended (nep_deflation.jl:382-392, :441-450)"""
    n = dnep.orgnep.size(1); p0 = dnep.V0.shape[1]
    v = np.asarray(v, dtype=np.complex128).reshape(-1)
    V1 = np.zeros((n, p0 + 1), dtype=np.complex128); S1 = np.zeros((p0 + 1, p0 + 1), dtype=np.complex128)
    V1[:, :p0] = dnep.V0; V1[:, p0] = v[:n]
    S1[:p0, :p0] = dnep.S0
    S1[:p0, p0] = v[n:]; S1[p0, p0] = lam
    return S1, V1


def deflate_eigpair(nep, lam, v, mode="Auto"):
    """nep_deflation.jl:369-398: the NEP with the eigenpair (lam, v) of `nep` deflated.  When `nep` is itself a deflated NEP its
    invariant pair is extended and the new NEP is built on the ORIGINAL problem.  mode: "Auto", "Generic", "SPMF", "MM"."""
    mode = verify_deflate_mode(nep, mode)
    if isinstance(nep, (DeflatedSPMF, DeflatedNEPMM, DeflatedGenericNEP)):
        S1, V1 = _extended_pair(nep, lam, v)
        org = nep.orgnep
    else:
        S1 = np.array([[lam]], dtype=np.complex128)
        V1 = np.asarray(v, dtype=np.complex128).reshape(nep.size(1), 1)
        org = nep
    S1, V1 = normalize_schur_pair(S1, V1)
    return {"MM": DeflatedNEPMM, "SPMF": DeflatedSPMF, "Generic": DeflatedGenericNEP}[mode](org, S1, V1)


def get_deflated_eigpairs(dnep, lam=None, v=None):
    """nep_deflation.jl:433-455: eigenvalues D and eigenvectors V[:, i] of the ORIGINAL problem held in the invariant pair of
    `dnep`; with (lam, v), an eigenpair of `dnep`, that pair is included as if it had been deflated too."""
    S, V = (dnep.S0, dnep.V0) if lam is None else _extended_pair(dnep, lam, v)
    D, X = np.linalg.eig(S)
    return D, V[:dnep.orgnep.size(1), :] @ X


class _Deflated:
    """what the three representations share: the original NEP, the invariant pair, size n0 + p"""

    def _init_pair(self, orgnep, S0, V0):
        self.orgnep = orgnep
        self.S0 = np.array(S0, dtype=np.complex128)
        self.V0 = np.array(V0, dtype=np.complex128)
        self.n0 = int(orgnep.size(1))
        self.p = int(self.V0.shape[1])
        self.n = self.n0 + self.p


class _DeflatedMMBase(_Deflated, NEP):
    def __init__(self, orgnep, S0, V0):
        self._init_pair(orgnep, S0, V0)

    def compute_MM(self, S, V):
        """nep_deflation.jl:183-194: compute_MM of the original NEP on ([S0 V2; 0 S], [V0 V1]); NumPy in -> NumPy out, device
        tensor in -> device tensor out"""
        host = not is_dev(V)
        Vh = np.asarray(V if host else to_host(V), dtype=np.complex128)
        if Vh.ndim == 1:
            Vh = Vh.reshape(-1, 1)
        S = np.atleast_2d(np.asarray(S, dtype=np.complex128))
        n0, p0, p = self.n0, self.p, S.shape[0]
        V1, V2 = Vh[:n0, :], Vh[n0:, :]
        St = np.block([[self.S0, V2], [np.zeros((p, p0)), S]])
        R = self.orgnep.compute_MM(St, np.hstack([self.V0, V1]))
        R = np.asarray(to_host(R) if is_dev(R) else R)
        Z = np.vstack([R[:n0, p0:], self.V0.conj().T @ V1])
        return Z if host else to_dev(Z)

    def resid_norms(self, lams, QT):
        """(||Mt(lam_s) q_s||, ||q_s||, None) for the columns of the row-major block QT, one compute_Mlincomb per pair (as
        Mder_NEP.resid_norms: ResidualErrmeasure / DefaultErrmeasure work on these types)"""
        k = len(lams)
        cols = dense.rowmajor_to_cols(QT, np.arange(k, dtype=np.int32))          # (k, n): column-major n x k
        Y = torch.empty_like(cols)
        for s_ in range(k):
            dense.copy(self.compute_Mlincomb(lams[s_], cols[s_].reshape(1, self.n)), Y[s_], self.n)
        nr = np.empty(k); nq = np.empty(k)
        check(lib.nep_colnorms(self.n, k, c_vp(Y.data_ptr()), self.n, hptr(nr), stream_ptr()))
        check(lib.nep_colnorms(self.n, k, c_vp(cols.data_ptr()), self.n, hptr(nq), stream_ptr()))
        return nr, nq, None


class DeflatedNEPMM(_DeflatedMMBase):
    """nep_deflation.jl:17-21,195-202: every compute function through compute_MM (small dense problems)"""
    compute_Mlincomb = NEP.compute_Mlincomb_from_MM
    compute_Mder = NEP.compute_Mder_from_MM


def expand_tables(lam, S0, a, startder):
    """the host tables of nep_defl_expand for the pair's S0: (a, G, W) with W[d] = (lam I - S0)^-(d+1), d < K = k + startder,
    and G[i, j] = (-1)^(e_i - j) a_i e_i! / j! for e_i = i + startder >= j (zero otherwise).  A singular lam I - S0 raises
    numpy.linalg.LinAlgError, as the reference's `factorize` throws a SingularException."""
    a = np.asarray(a, dtype=np.complex128).reshape(-1)
    k = len(a); s = int(startder); K = k + s
    p = S0.shape[0]
    W = np.empty((K, p, p), dtype=np.complex128)
    W[0] = np.linalg.inv(complex(lam) * np.eye(p) - S0)
    for d in range(1, K):
        W[d] = W[d - 1] @ W[0]
    G = np.zeros((k, K), dtype=np.complex128)
    for i in range(k):
        e = i + s
        r = 1.0                                            # e! / j!, downwards from j = e
        for j in range(e, -1, -1):
            G[i, j] = (-1.0) ** (e - j) * r * a[i]
            r *= j
    return a, G, W


class DeflatedGenericNEP(_DeflatedMMBase):
    """nep_deflation.jl:46-50,65-170: derivatives by binomial expansion; the expansion runs on the device (nep_defl_expand)"""

    def __init__(self, orgnep, S0, V0):
        super().__init__(orgnep, S0, V0)
        self._Xd = None

    @property
    def Xd(self):
        if self._Xd is None:
            self._Xd = to_dev(self.V0)                     # (p, n0): column-major n0 x p
        return self._Xd

    def _expand_fused(self, Vd, a, G, W, s, Vn, zb):
        """Vn (K, n0) and zb (p entries) by nep_defl_expand; False when the sizes are outside the kernel's limits"""
        k = Vd.shape[0]
        Wc = np.ascontiguousarray(np.transpose(W, (0, 2, 1)))            # each W_d column-major
        rc = lib.nep_defl_expand(self.n0, self.p, k, s, c_vp(self.Xd.data_ptr()), self.n0, c_vp(Vd.data_ptr()), Vd.shape[1],
                                 hptr(a), hptr(_lib.as_c128(G, "F")), hptr(Wc), c_vp(Vn.data_ptr()), self.n0,
                                 c_vp(zb.data_ptr()), stream_ptr())
        if rc == _lib.NEP_ERR_UNSUPPORTED:
            return False
        check(rc)
        return True

    def _expand_composed(self, Vd, a, G, W, s, Vn, zb):
        """the same result from existing device primitives, for sizes nep_defl_expand refuses (p > 32 or k + s > 64):
        X W_d by the tall-skinny GEMM (host table), (X W_d) V2[:, i..] by the GEMM with a device B, axpy into Vn; z_bottom by
        nep_gemv_hd (zb = None: the caller forms z_bottom itself).  Nothing is copied to the host."""
        n0, p = self.n0, self.p
        k = Vd.shape[0]; K = k + s; ldv = Vd.shape[1]
        Vn.zero_()
        for j in range(s, K):
            if a[j - s] != 0:
                dense.axpy(a[j - s], Vd[j - s], Vn[j], n0)
        V2 = c_vp(Vd.data_ptr() + 16 * n0)
        for d in range(K):                                  # pairs (i, j) with e_i - j == d: j = i + s - d
            i0 = max(0, d - s)
            if i0 >= k:
                break
            XW = dense.gemm_ts(self.Xd, W[d])               # (p, n0): X W_d
            Y = torch.empty((k - i0, n0), dtype=CDT, device="cuda")
            check(lib.nep_gemm_ts_dev(c_vp(XW.data_ptr()), n0, n0, p, c_vp(V2.value + 16 * i0 * ldv), ldv, 0, k - i0,
                                      c_vp(Y.data_ptr()), n0, 0, stream_ptr()))
            for i in range(i0, k):
                j = i + s - d
                if G[i, j] != 0:
                    dense.axpy(G[i, j], Y[i - i0], Vn[j], n0)
        if zb is None:
            return
        if s == 0:
            check(lib.nep_gemv_hd(c_vp(self.Xd.data_ptr()), n0, n0, p, c_vp(Vd.data_ptr()), None, c_vp(zb.data_ptr()),
                                  stream_ptr()))
            dense.scal(zb, a[0], p)
        else:
            zb.zero_()

    def compute_Mlincomb(self, lam, V, a=None, startder=0):
        """sum_j a_j Mt^(j+startder)(lam) v_j.  NumPy in -> NumPy out; device tensor in -> device tensor out (no host
        synchronisation: only the p x p tables are formed on the host).  V is not modified."""
        host = not is_dev(V)
        Vd = to_dev(V) if host else (V if V.dim() == 2 else V.reshape(1, -1))
        k = Vd.shape[0]
        if Vd.shape[1] != self.n or not Vd.is_contiguous():
            raise ValueError("V must have %d rows" % self.n)
        a = np.ones(k, dtype=np.complex128) if a is None else np.asarray(a, dtype=np.complex128)
        if len(a) != k:
            raise ValueError("length of a must equal the number of columns of V")
        s = int(startder); K = k + s
        a, G, W = expand_tables(lam, self.S0, a, s)
        z = torch.empty(self.n, dtype=CDT, device="cuda")
        Vn = torch.empty((K, self.n0), dtype=CDT, device="cuda")
        zb = z[self.n0:]
        if not self._expand_fused(Vd, a, G, W, s, Vn, zb):
            self._expand_composed(Vd, a, G, W, s, Vn, zb)
        org = self.orgnep
        if pure_spmf(org, "Mlincomb"):
            org.dev.mlincomb(org.coeff_block(lam, np.ones(K)), Vn, z)                # K1 writes the first n0 entries of z
        else:
            dense.copy(org.compute_Mlincomb(lam, Vn), z, self.n0)
        return to_host(z.reshape(1, -1))[:, 0] if host else z

    def compute_Mder(self, lam, i=0):
        """[[M^(i), Q], [X^H or 0, 0]] (nep_deflation.jl:110-170): sparse when the original NEP's matrix is; column j of Q is
        this type's compute_Mlincomb on the unit vector e_{n0+j} with startder = i (= deflated_nep_compute_Q)"""
        n0, p = self.n0, self.p
        M0 = self.orgnep.compute_Mder(lam, i)
        Q = np.empty((n0, p), dtype=np.complex128)
        for j in range(p):
            e = np.zeros((self.n, 1), dtype=np.complex128); e[n0 + j, 0] = 1.0
            Q[:, j] = self.compute_Mlincomb(lam, e, startder=i)[:n0]
        XH = self.V0.conj().T
        if sp.issparse(M0):
            return sp.bmat([[M0, sp.csc_matrix(Q)], [sp.csc_matrix(XH) if i == 0 else sp.csc_matrix((p, n0)), sp.csc_matrix((p, p))]],
                           format="csc", dtype=np.complex128)
        return np.block([[np.asarray(M0, dtype=np.complex128), Q], [XH if i == 0 else np.zeros((p, n0)), np.zeros((p, p))]])


class DeflatedSPMF(_Deflated, AbstractSPMF):
    """nep_deflation.jl:31-36,172-179,210-269: the deflated NEP as an SPMF -- SumNEP(original terms padded to n0 + p,
    LowRankFactorizedNEP of the m p rank-one terms and the constant border).  A dense original NEP is held as full sparse
    matrices, so that every term goes through one stacked CSR."""

    def __init__(self, orgnep, S0, V0):
        if not isinstance(orgnep, AbstractSPMF):
            raise ValueError("SPMF-mode only possible for `AbstractSPMF`-NEPs")
        self._init_pair(orgnep, S0, V0)
        n0, p, n = self.n0, self.p, self.n
        Av, fv = orgnep.get_Av(), orgnep.get_fv()
        A1 = []
        for A in Av:
            C = sp.coo_matrix(A)
            A1.append(sp.csc_matrix((C.data, (C.row, C.col)), shape=(n, n)))
        lams, Xe = np.linalg.eig(self.S0)
        Xinv = np.linalg.inv(Xe)
        terms = []
        for i in range(p):
            y = self.V0 @ Xe[:, i]
            U = sp.csc_matrix((np.conj(Xinv[i, :]), (n0 + np.arange(p), np.zeros(p, dtype=int))), shape=(n, 1))
            for A, f in zip(Av, fv):
                L = sp.csc_matrix(np.concatenate([A @ y, np.zeros(p)]).reshape(n, 1))
                terms.append(LowRankMatrixAndFunction(None, funcs.Resolvent(f, lams[i]), L=L, U=U))
        L = sp.csc_matrix((np.ones(p), (n0 + np.arange(p), np.arange(p))), shape=(n, p), dtype=np.complex128)
        U = sp.vstack([sp.csc_matrix(self.V0), sp.csc_matrix((p, p))], format="csc")
        terms.append(LowRankMatrixAndFunction(None, funcs.one(), L=L, U=U))
        self.spmf = SumNEP(SPMF_NEP(A1, fv), LowRankFactorizedNEP(terms))

    def get_Av(self):
        return self.spmf.get_Av()

    def get_fv(self):
        return self.spmf.get_fv()
