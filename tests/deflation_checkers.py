"""Reference, error bound and case list for nep_defl_expand (csrc/deflate.hip), a dense NumPy restatement of the reference's
three deflation modes (src/nep_deflation.jl, written from that file and from src/NEPCore.jl / src/method_newton.jl, not from the
product), and dep0_sparse restated on the oracle's MSWS_RNG.

Style and helpers of tests/primitive_checkers.py: `DeflExpand.check(impl, case)` runs `impl` on flat complex128 buffers and
compares with a plain reference; test_gpu_deflation.py passes an adapter that calls the library, test_host_deflation.py passes
the float64 NumPy implementation and its mutants.

Error bound of the rounded cases.  With s = startder, K = k + s, e_i = i + s the kernel forms
    C[:, j]  = sum_{i >= max(0, j-s)} G[i, j] * (W_{e_i-j} V2[:, i])                      (p x K)
    Vn[r, j] = [j >= s] a_{j-s} V1[r, j-s] + sum_l X[r, l] C[l, j],          zb[q] = a_0 sum_r conj(X[r, q]) V1[r, 0].
Given the computed C, Vn[r, j] is a sum of p + 1 complex products: |error| <= cbound(p + 1, |a||V1| + |X|.|C|) to first order.
An entry of C is a sum over i of G[i, j] times an inner sum of p products: the inner sum is off by at most
sqrt(2) gamma_{2p} sum_l |W||V2|, the product with G adds one complex multiplication (sqrt(2) gamma_2 relative), the outer sum
over at most k terms gamma_{2k}: together below sqrt(2) gamma_{2p+2k+3} T with T = sum_i |G| (|W| |V2|), and
2p + 2k + 3 <= 2kp + 6 for all k, p >= 1 (2 (k-1)(p-1) + 1 >= 0).  So |dC| <= cbound(k p, T) and it reaches Vn[r, j] through
|X[r, :]| . cbound(k p, T[:, j]):
    |dVn[r, j]| <= cbound(p + 1, |a||V1| + |X|.|C|) + |X| . cbound(k p, sum |G||W||V2|)
    |dzb[q]|    <= cbound(n0, |a_0| sum_r |X||V1|)            (n0 products, the scale factor a_0 among cbound's six extra roundings)
Nothing is fitted to a device result.  The largest error / bound ratio seen is recorded in primitive_checkers.RATIOS.
"""
from functools import partial
import math

import numpy as np
import scipy.linalg as sla

from primitive_checkers import (C128, CLD, NAN, SENT, RATIOS, Case, Prim, _seed, gamma, cbound, gint, grand, operand,        # noqa: F401
                                colmajor_buf, cm_view, perturb, assert_exact, assert_bounded, assert_below_2_53)

# ================================================================================================================================
# nep_defl_expand
DE_N0 = [1, 2, 63, 64, 65, 255, 257, 1025, 4099]
DE_P = [1, 2, 3, 8, 32]
DE_KS = [(1, 0), (1, 1), (2, 0), (1, 4), (3, 2), (8, 0), (32, 32)]
DE_GRID_ROWS = 2048 * 256 + 77           # more rows than the capped grid of the streaming pass has threads: the grid-stride loop
LEAD, TRAIL = 3, 3


class DeflExpand(Prim):
    """impl(n0, p, k, s, X, ldx, V, ldv, A, G, W, Vn, ldo, zb) -> (Vn buffer, zb buffer) after the call.

    X: n0 x p (ldx), V: (n0 + p) x k (ldv), column-major flat buffers whose padding rows hold NaN.  A: k, G: k x K column-major
    (entries with e_i < j hold NaN: they must not be used), W: K blocks of p x p, column-major.  Vn: LEAD sentinels, the
    n0 x K block (ldo) prefilled with NaN and padding rows holding the sentinel, TRAIL sentinels; zb: one sentinel, p NaN, one
    sentinel.  The checker verifies that everything but the n0 x K block and the p entries kept its value."""
    name = "nep_defl_expand"
    mutants = ("g_sign", "w_plus", "w_minus", "drop_s", "zb_stale", "skip_row", "pad_write", "perturb")

    def cases(self):
        shapes = []
        combos = [(p, ks) for ks in DE_KS for p in DE_P]
        for t, (p, ks) in enumerate(combos):                       # every (p, (k, s)) on a rotating row count
            shapes.append((DE_N0[(2 * t + 1) % len(DE_N0)], p, ks, "exact"))
            if t % 3 == 0:
                shapes.append((DE_N0[(2 * t + 4) % len(DE_N0)], p, ks, "rounded"))
        for t, n0 in enumerate(DE_N0):                             # every row count on the two calls a Newton step makes
            shapes.append((n0, 3, (1, 0), "exact"))
            shapes.append((n0, DE_P[t % len(DE_P)], (1, 1), "exact" if t % 2 else "rounded"))
        for t, (n0, p, (k, s), kind) in enumerate(shapes):
            pad = 3 * (t % 2)
            yield Case("n%d" % n0, "p%d_k%d_s%d_pad%d" % (p, k, s, pad), kind, partial(self._build, n0, p, k, s, kind, pad))
        yield Case("n%d" % DE_GRID_ROWS, "p2_k1_s0_pad0", "exact", partial(self._build, DE_GRID_ROWS, 2, 1, 0, "exact", 0))

    @staticmethod
    def _build(n0, p, k, s, kind, pad):
        rng = np.random.default_rng(_seed("deflexpand%d.%d.%d.%d%s" % (n0, p, k, s, kind)))
        K = k + s
        X = operand(kind, rng, (n0, p)); V = operand(kind, rng, (n0 + p, k))
        A = operand(kind, rng, k)
        G = operand(kind, rng, (k, K)); W = operand(kind, rng, (K, p, p))
        for i in range(k):
            G[i, i + s + 1:] = NAN                                 # e_i < j: not part of the sum
        ldx, ldv, ldo = n0 + pad, n0 + p + pad, n0 + pad
        Vn = colmajor_buf(np.full((n0, K), NAN, dtype=C128), ldo, fill=SENT, lead=LEAD, trail=TRAIL)
        Vn[:LEAD] = SENT; Vn[len(Vn) - TRAIL:] = SENT
        zb = np.concatenate([[SENT], np.full(p, NAN, dtype=C128), [SENT]])
        return dict(n0=n0, p=p, k=k, s=s, X=colmajor_buf(X, ldx), ldx=ldx, V=colmajor_buf(V, ldv), ldv=ldv, A=A,
                    G=np.ascontiguousarray(G.T).reshape(-1), W=np.ascontiguousarray(np.transpose(W, (0, 2, 1))).reshape(-1),
                    Vn=Vn, ldo=ldo, zb=zb)

    @staticmethod
    def _operands(n0, p, k, s, X, ldx, V, ldv, A, G, W, dt):
        K = k + s
        Xm = cm_view(X, 0, n0, p, ldx).astype(dt); Vm = cm_view(V, 0, n0 + p, k, ldv).astype(dt)
        Gm = G.reshape(K, k).T.astype(dt)                          # G[i, j]
        Wm = np.transpose(W.reshape(K, p, p), (0, 2, 1)).astype(dt)      # W[d][row, col]
        return Xm, Vm[:n0], Vm[n0:], A.astype(dt), Gm, Wm

    def small_block(self, p, k, s, V2, Gm, Wm, mut=None, absolute=False):
        """C (p x K), or with `absolute` T = sum |G| (|W| |V2|)"""
        K = k + s
        Cm = np.zeros((p, K), dtype=Gm.dtype if not absolute else np.float64)
        for j in range(K):
            for i in range(max(0, j - s), k):
                d = i + s - j
                if mut == "drop_s":
                    d = max(i - j, 0)
                elif mut == "w_plus":
                    d = min(d + 1, K - 1)
                elif mut == "w_minus":
                    d = max(d - 1, 0)
                g = Gm[i, j]
                if mut == "g_sign" and (i + s - j) % 2:
                    g = -g
                if absolute:
                    Cm[:, j] += abs(g) * (np.abs(Wm[d]).astype(np.float64) @ np.abs(V2[:, i]).astype(np.float64))
                else:
                    Cm[:, j] += g * (Wm[d] @ V2[:, i])
        return Cm

    def ref(self, n0, p, k, s, X, ldx, V, ldv, A, G, W, Vn, ldo, zb, mut=None, dt=C128, parts=False):
        K = k + s
        Xm, V1, V2, a, Gm, Wm = self._operands(n0, p, k, s, X, ldx, V, ldv, A, G, W, dt)
        Cm = self.small_block(p, k, s, V2, Gm, Wm, mut)
        R = Xm @ Cm
        for j in range(s, K):
            R[:, j] += a[j - s] * V1[:, j - s]
        z = a[0] * (np.conj(Xm).T @ V1[:, 0]) if (s == 0 or mut == "zb_stale") else np.zeros(p, dtype=dt)
        if parts:
            return R, z, Cm
        out = np.array(Vn, copy=True); zo = np.array(zb, copy=True)
        for j in range(K):
            out[LEAD + j * ldo: LEAD + j * ldo + n0] = R[:, j]
        if mut == "skip_row":
            out[LEAD + (K - 1) * ldo + n0 // 2] = NAN
        if mut == "pad_write" and ldo > n0:
            out[LEAD + n0] = 0.0
        zo[1:1 + p] = z
        if mut == "perturb":
            out[LEAD: LEAD + n0] = perturb(out[LEAD: LEAD + n0])
        return out, zo

    def check(self, impl, c):
        a = c.args
        n0, p, k, s, ldo = a["n0"], a["p"], a["k"], a["s"], a["ldo"]
        K = k + s
        Vn0 = np.array(a["Vn"], copy=True); zb0 = np.array(a["zb"], copy=True)
        got_vn, got_zb = impl(**a)
        got_vn = np.asarray(got_vn); got_zb = np.asarray(got_zb)
        assert got_vn.shape == Vn0.shape and got_zb.shape == zb0.shape, (self.name, c)
        blk = np.zeros(len(Vn0), dtype=bool)
        for j in range(K):
            blk[LEAD + j * ldo: LEAD + j * ldo + n0] = True
        assert_exact(self.name + " (sentinels and padding rows of Vn)", c, got_vn[~blk], Vn0[~blk])
        assert_exact(self.name + " (sentinels around zb)", c, got_zb[[0, -1]], zb0[[0, -1]])
        R = np.stack([got_vn[LEAD + j * ldo: LEAD + j * ldo + n0] for j in range(K)], axis=1)
        z = got_zb[1:1 + p]
        Xm, V1, V2, av, Gm, Wm = self._operands(n0, p, k, s, a["X"], a["ldx"], a["V"], a["ldv"], a["A"], a["G"], a["W"], C128)
        aX = np.abs(Xm); T = self.small_block(p, k, s, V2, Gm, Wm, absolute=True)
        aV = np.zeros((n0, K))
        for j in range(s, K):
            aV[:, j] = abs(av[j - s]) * np.abs(V1[:, j - s])
        Sz = abs(av[0]) * (aX.T @ np.abs(V1[:, 0])) if s == 0 else np.zeros(p)
        if c.kind == "exact":
            assert_below_2_53(2 * (aV + aX @ T)); assert_below_2_53(2 * Sz)
            Rw, zw, _ = self.ref(parts=True, **a)
            assert_exact(self.name, c, R, Rw)
            assert_exact(self.name + " (zb)", c, z, zw)
        else:
            Rw, zw, Cw = self.ref(parts=True, dt=CLD, **a)
            bound = cbound(p + 1, aV + aX @ np.abs(Cw).astype(np.float64)) + aX @ cbound(k * p, T)
            assert_bounded(self.name, c, R, Rw, bound)
            if s == 0:
                assert_bounded(self.name, c, z, zw, cbound(n0, Sz))
            else:
                assert_exact(self.name + " (zb)", c, z, np.zeros(p, dtype=C128))


DEFL = DeflExpand()


# ================================================================================================================================
# dense restatement of the reference's deflation (src/nep_deflation.jl) on a dense SPMF
class RefFun:
    """scalar function with derivatives `der(lam, j)` and matrix function `mat(S)`"""

    def __init__(self, der, mat):
        self.der, self.mat = der, mat


def ref_minus_ident():
    return RefFun(lambda lam, j: -lam if j == 0 else (-1.0 if j == 1 else 0.0), lambda S: -np.asarray(S, dtype=complex))


def ref_one():
    return RefFun(lambda lam, j: 1.0 if j == 0 else 0.0, lambda S: np.eye(len(S), dtype=complex))


def ref_exp(c):
    return RefFun(lambda lam, j: c ** j * np.exp(c * lam), lambda S: sla.expm(c * np.asarray(S, dtype=complex)))


def ref_resolvent(f, mu):
    """f(.) / (. - mu) by Leibniz' rule in closed form: sum_i binom(j, i) f^(j-i)(lam) (-1)^i i! / (lam - mu)^(i+1);
    nep_deflation.jl:259 for the matrix function"""
    def der(lam, j):
        return sum(math.comb(j, i) * f.der(lam, j - i) * (-1.0) ** i * math.factorial(i) / (lam - mu) ** (i + 1) for i in range(j + 1))
    return RefFun(der, lambda S: np.linalg.solve(np.asarray(S, dtype=complex) - mu * np.eye(len(S)), f.mat(S)))


class RefSPMF:
    """M(lam) = sum_i f_i(lam) A_i with dense A_i (NEPTypes.jl: compute_Mder, compute_Mlincomb, compute_MM of an SPMF)"""

    def __init__(self, Av, fv):
        self.Av = [np.asarray(A.toarray() if hasattr(A, "toarray") else A, dtype=complex) for A in Av]
        self.fv = list(fv)
        self.n = self.Av[0].shape[0]

    def Mder(self, lam, der=0):
        return sum(f.der(lam, der) * A for A, f in zip(self.Av, self.fv))

    def Mlincomb(self, lam, V, a=None, startder=0):
        V = np.asarray(V, dtype=complex).reshape(self.n, -1)
        a = np.ones(V.shape[1]) if a is None else a
        return sum(a[j] * (self.Mder(lam, j + startder) @ V[:, j]) for j in range(V.shape[1]))

    def MM(self, S, V):
        S = np.atleast_2d(np.asarray(S, dtype=complex))
        return sum(A @ np.asarray(V, dtype=complex) @ f.mat(S) for A, f in zip(self.Av, self.fv))


def ref_dep(A0, A1, tau=1.0):
    n = A0.shape[0]
    return RefSPMF([np.eye(n), A0, A1], [ref_minus_ident(), ref_one(), ref_exp(-tau)])


def ref_normalize_schur_pair(S, V):
    Q, R = np.linalg.qr(V)                                         # nep_deflation.jl:282-284
    return (R @ S) @ np.linalg.inv(R), Q


class RefDeflated:
    """nep_deflation.jl in dense arithmetic; mode in ("Generic", "SPMF", "MM")"""

    def __init__(self, org, S0, V0, mode):
        self.org, self.S0, self.V0, self.mode = org, np.asarray(S0, dtype=complex), np.asarray(V0, dtype=complex), mode
        self.n0, self.p = org.n, self.V0.shape[1]
        self.n = self.n0 + self.p
        if mode == "SPMF":
            self.spmf = self._create_spmf()

    def _create_spmf(self):                                        # create_spmf_dnep, :210-269
        n0, p, n = self.n0, self.p, self.n
        Av, fv = [], []
        for A, f in zip(self.org.Av, self.org.fv):
            P = np.zeros((n, n), dtype=complex); P[:n0, :n0] = A
            Av.append(P); fv.append(f)
        lam, X = np.linalg.eig(self.S0)
        Xi = np.linalg.inv(X)
        for i in range(p):
            y = self.V0 @ X[:, i]
            for A, f in zip(self.org.Av, self.org.fv):
                L = np.concatenate([A @ y, np.zeros(p)]); U = np.concatenate([np.zeros(n0), np.conj(Xi[i, :])])
                Av.append(np.outer(L, np.conj(U))); fv.append(ref_resolvent(f, lam[i]))
        B = np.zeros((n, n), dtype=complex); B[n0:, :n0] = self.V0.conj().T
        Av.append(B); fv.append(ref_one())
        return RefSPMF(Av, fv)

    # ---- Generic: :65-170
    def _generic_Mlincomb(self, lam, V, a):
        X, S, n0, p = self.V0, self.S0, self.n0, self.p
        k = V.shape[1]
        F = lam * np.eye(p) - S
        Xhat = X @ np.linalg.inv(F)
        Q = []
        for i in range(k):
            QQ = np.zeros((p, k), dtype=complex)
            QQ[:, i] = V[n0:, i]
            for j in range(i - 1, -1, -1):
                QQ[:, j] = np.linalg.solve(F, QQ[:, j + 1])
            Q.append(QQ)
        Z = np.zeros((n0, k), dtype=complex)
        for j in range(k):
            for i in range(j, k):
                Z[:, j] += (-1.0) ** (i - j) * (a[i] * math.factorial(i) / math.factorial(j)) * (Xhat @ Q[i][:, j])
        Vnew = V[:n0, :] * a[None, :] + Z
        return np.concatenate([self.org.Mlincomb(lam, Vnew), X.conj().T @ V[:n0, 0] * a[0]])

    def _compute_Q(self, lam, der):                                # deflated_nep_compute_Q, :149-170
        Fi = np.linalg.inv(lam * np.eye(self.p) - self.S0)
        Q = np.zeros((self.n0, self.p), dtype=complex)
        Vnew = self.V0
        for i in range(der, -1, -1):
            Vnew = Vnew @ Fi
            Q += (-1.0) ** (der - i) * (math.factorial(der) / math.factorial(i)) * (self.org.Mder(lam, i) @ Vnew)
        return Q

    def MM(self, S, V):
        if self.mode == "SPMF":
            return self.spmf.MM(S, V)
        S = np.atleast_2d(np.asarray(S, dtype=complex)); V = np.asarray(V, dtype=complex)
        n0, p0, p = self.n0, self.p, S.shape[0]                    # :183-194
        V1, V2 = V[:n0, :], V[n0:, :]
        St = np.block([[self.S0, V2], [np.zeros((p, p0)), S]])
        R = self.org.MM(St, np.hstack([self.V0, V1]))
        return np.vstack([R[:n0, p0:], self.V0.conj().T @ V1])

    def Mlincomb(self, lam, V, a=None, startder=0):
        V = np.asarray(V, dtype=complex).reshape(self.n, -1)
        a = np.ones(V.shape[1], dtype=complex) if a is None else np.asarray(a, dtype=complex)
        if self.mode == "SPMF":
            return self.spmf.Mlincomb(lam, V, a, startder)
        if startder > 0:                                           # NEPCore.jl:156-160
            a = np.concatenate([np.zeros(startder), a]); V = np.hstack([np.zeros((self.n, startder)), V])
        if self.mode == "Generic":
            return self._generic_Mlincomb(lam, V, a)
        V = V.copy(); a = a.copy()                                 # MM: compute_Mlincomb_from_MM!, NEPCore.jl:218-228
        k = V.shape[1]
        V[:, a == 0] = 0; a[a == 0] = 1
        S = np.diag(np.full(k, complex(lam))) + np.diag((a[1:] / a[:-1]) * np.arange(1, k), -1)
        return a[0] * self.MM(S, V)[:, 0]

    def Mder(self, lam, der=0):
        if self.mode == "SPMF":
            return self.spmf.Mder(lam, der)
        n0, p, n = self.n0, self.p, self.n
        if self.mode == "Generic":                                 # :110-146
            B = self.V0.conj().T if der == 0 else np.zeros((p, n0))
            return np.block([[self.org.Mder(lam, der), self._compute_Q(lam, der)], [B, np.zeros((p, p))]])
        J = np.diag(np.full(der + 1, complex(lam))) + np.diag(np.ones(der), -1)      # compute_Mder_from_MM, NEPCore.jl:256-263
        e = np.zeros((1, der + 1)); e[0, -1] = 1.0
        W = self.MM(np.kron(J, np.eye(n)), math.factorial(der) * np.kron(e, np.eye(n)))
        return W[:n, :n]


def ref_deflate(nep, lam, v, mode):
    """deflate_eigpair, :369-398"""
    v = np.asarray(v, dtype=complex)
    if isinstance(nep, RefDeflated):
        n, p0 = nep.n0, nep.p
        V1 = np.zeros((n, p0 + 1), dtype=complex); S1 = np.zeros((p0 + 1, p0 + 1), dtype=complex)
        V1[:, :p0] = nep.V0; V1[:, p0] = v[:n]
        S1[:p0, :p0] = nep.S0; S1[:p0, p0] = v[n:]; S1[p0, p0] = lam
        org = nep.org
    else:
        S1 = np.array([[lam]], dtype=complex); V1 = v.reshape(-1, 1); org = nep
    S1, V1 = ref_normalize_schur_pair(S1, V1)
    return RefDeflated(org, S1, V1, mode)


def ref_get_deflated_eigpairs(dnep):
    D, X = np.linalg.eig(dnep.S0)
    return D, dnep.V0 @ X


def ref_augnewton(nep, lam, v, tol, maxit=30):
    """method_newton.jl:274-347 with the residual error measure ||M(lam) v|| / ||v||; returns (lam, v, steps)"""
    lam = complex(lam); v = np.asarray(v, dtype=complex).copy(); c = v.copy()
    v = v / np.vdot(c, v)
    for k in range(1, maxit + 1):
        if np.linalg.norm(nep.Mlincomb(lam, v)) / np.linalg.norm(v) < tol:
            return lam, v, k
        t = np.linalg.solve(nep.Mder(lam), nep.Mlincomb(lam, v, [1.0], 1))
        alpha = 1.0 / np.vdot(c, t)
        lam -= alpha; v = alpha * t
    raise RuntimeError("ref_augnewton: no convergence from the given start")


def ref_resinv(nep, lam, v, tol, maxit=100):
    """method_newton.jl:142-226 (c = v at the start, Rayleigh functional by scalar Newton as compute_rf_wrapper.jl:25-54)"""
    lam = complex(lam); v = np.asarray(v, dtype=complex).copy(); c = v.copy()
    Msig = nep.Mder(lam)
    for k in range(1, maxit + 1):
        v = v / np.linalg.norm(v)
        if np.linalg.norm(nep.Mlincomb(lam, v)) < tol:
            return lam, v, k
        l1 = lam
        for _ in range(80):
            d = -np.vdot(c, nep.Mlincomb(l1, v)) / np.vdot(c, nep.Mlincomb(l1, v, [1.0], 1))
            l1 += d
            if abs(d) <= 100 * np.finfo(float).eps:
                break
        v = v - np.linalg.solve(Msig, nep.Mlincomb(l1, v))
        lam = l1
    raise RuntimeError("ref_resinv: no convergence from the given start")


# ================================================================================================================================
# dep0_sparse on the oracle's generator (src/gallery_extra/basic_random_examples.jl:13-20,107-128)
def ref_gen_rng_spmat(rng, n, m, p):
    d = {}
    for _ in range(int(round(p * m * n))):
        r = rng.gen_int() % n
        c = rng.gen_int() % m
        d[(r, c)] = 1 - 2 * rng.gen_float()
    M = np.zeros((n, m)); mask = np.zeros((n, m), dtype=bool)
    for (r, c), x in d.items():
        M[r, c] = x; mask[r, c] = True
    return M, mask


def ref_dep0_sparse(n=100, p=0.25):
    """(A0, A1, stored-entry masks) as dense arrays"""
    from oracle import gallery as og
    rng = og.MSWS_RNG()
    out = []
    for _ in range(2):
        d = og.gen_rng_mat(rng, n, 1)[:, 0]
        M, mask = ref_gen_rng_spmat(rng, n, n, p)
        out.append((np.diag(d) + M, mask | np.eye(n, dtype=bool)))
    return out[0][0], out[1][0], out[0][1], out[1][1]
