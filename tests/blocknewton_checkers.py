"""Reference, error bound and case list for nep_spmf_blockprod (csrc/blockprod.hip), and a dense NumPy restatement of the block
Newton method written from the mathematics of src/method_blocknewton.jl, not from the product.

Style and helpers of tests/broyden_checkers.py: `BLOCKPROD.check(impl, case)` runs `impl` on flat complex128 buffers and compares
with a plain reference; test_gpu_blocknewton.py passes an adapter that calls the library, test_host_blocknewton.py passes the
NumPy implementation and its mutants.

The kernel computes, for mt sparse n x n matrices A_t, an n x r block Y and mt tables G_t (r x q),

    Z[:, 0:q] = beta Z[:, 0:q] + alpha sum_t A_t (Y G_t)            (Z is not read when beta == 0).

Error bound of the rounded cases (cbound of primitive_checkers.py).  Entry (i, j) is alpha * sum_e a_e d_e (+ beta Z[i, j]), the sum
running over the E_row stored entries e = (t, c) of row i in all terms, with d_e = sum_k Y[c, k] G_t[k, j] an r-term inner product.
The computed d_e is off by at most gamma_{2r}-sized relative to sum_k |Y[c, k]| |G_t[k, j]|; the outer sum of E_row products adds
gamma_{2 E_row} relative to sum_e |a_e| |d_e| in any summation order (a row split over lanes and added by a tree included), and its
terms carry the inner error: gamma_a + gamma_b + gamma_a gamma_b <= gamma_{a + b} (Higham, Lemma 3.3) gives a sum of E_row + r
products.  The same count holds in the other nesting order (u_t = sum over the entries of term t of a_e Y[c, :], then u_t G_t).  The
scale by alpha, the product beta Z and the final addition are the further roundings cbound already allows; four more terms are
allowed on top of them.  Hence

    |dZ[i, j]| <= cbound(E_row(i) + r + 4, S[i, j]),     S = |alpha| sum_t |A_t| (|Y| |G_t|) + |beta| |Z|.

Nothing is fitted to a device result.  The largest error / bound ratio seen is recorded in primitive_checkers.RATIOS.
"""
from functools import partial

import numpy as np
import scipy.linalg as sla
import scipy.sparse as sp

from primitive_checkers import (C128, CLD, NAN, SENT, RATIOS, Case, Prim, _seed, cbound, gint, grand, colmajor_buf,      # noqa: F401
                                drop_tail, assert_exact, assert_bounded, assert_below_2_53)

EPS = np.finfo(float).eps

# ================================================================================================================================
# nep_spmf_blockprod
BP_N = [1, 2, 63, 64, 65, 257, 1025]
BP_MT = [1, 3, 5]
BP_RQ = [(1, 1), (2, 2), (3, 2), (5, 4), (9, 8)]
BP_AB = [(1.0, 0.0), (-1.0, 1.0), (0.5 - 2.0j, 3.0 + 1.0j)]
BP_VAL = ["real", "complex"]
BP_PAD = [0, 3]
BP_KIND = ["exact", "rounded"]
BP_FACTORS = [BP_N, BP_MT, BP_RQ, BP_AB, BP_VAL, BP_PAD, BP_KIND]
BP_LIMIT = [(n, 3, (32, 32), ab, val, pad, kind) for n, ab, val, pad, kind in
            [(65, BP_AB[0], "real", 0, "exact"), (65, BP_AB[2], "complex", 3, "rounded"), (257, BP_AB[1], "complex", 0, "exact"),
             (257, BP_AB[0], "real", 3, "rounded"), (1, BP_AB[2], "real", 0, "rounded"), (1025, BP_AB[1], "real", 3, "exact")]]
LEAD = 3
LONG_ROW = 130                                       # entries of the long row (n >= 130): more than two waves' worth
GROUP = 16                                           # the quantum the group-dropping mutant forgets (rows of a workgroup)
ROW_CAP = 64


def covering_shapes():
    """every pair of values of two different factors occurs in some shape: for each pair of factors all their value pairs, the
    other factors filled by rotation; then every (n, (r, q), value width) triple the same way; duplicates removed.  Plus
    (r, q) = (32, 32) with mt = 3, exactly at the table limit."""
    seen, out = set(), []
    t = 0
    for a in range(len(BP_FACTORS)):
        for b in range(a + 1, len(BP_FACTORS)):
            for va in range(len(BP_FACTORS[a])):
                for vb in range(len(BP_FACTORS[b])):
                    ix = [(t + 3 * f) % len(F) for f, F in enumerate(BP_FACTORS)]
                    ix[a], ix[b] = va, vb
                    t += 1
                    if tuple(ix) not in seen:
                        seen.add(tuple(ix))
                        out.append(tuple(F[i] for F, i in zip(BP_FACTORS, ix)))
    for va in range(len(BP_N)):                                           # every (n, (r, q), value width) triple as well
        for vb in range(len(BP_RQ)):
            for vc in range(len(BP_VAL)):
                ix = [(t + 3 * f) % len(F) for f, F in enumerate(BP_FACTORS)]
                ix[0], ix[2], ix[4] = va, vb, vc
                t += 1
                if tuple(ix) not in seen:
                    seen.add(tuple(ix))
                    out.append(tuple(F[i] for F, i in zip(BP_FACTORS, ix)))
    return out + BP_LIMIT


def make_terms(rng, n, mt, val, kind):
    """mt sparse n x n CSR matrices: about five entries per row at random columns, row 1 empty in every term (n >= 2), the last row
    with LONG_ROW entries in term 0 (n >= LONG_ROW), entry (0, 0) stored in every term"""
    terms = []
    for t in range(mt):
        per = min(n, 5)
        rows = np.repeat(np.arange(n), per)
        cols = np.concatenate([rng.choice(n, per, replace=False) for _ in range(n)])
        if t == 0 and n >= LONG_ROW:
            keep = rows != n - 1
            rows = np.concatenate([rows[keep], np.full(LONG_ROW, n - 1)])
            cols = np.concatenate([cols[keep], rng.choice(n, LONG_ROW, replace=False)])
        keep = ~((rows == 0) & (cols == 0))
        rows = np.concatenate([rows[keep], [0]]); cols = np.concatenate([cols[keep], [0]])
        if n >= 2:
            keep = rows != 1
            rows, cols = rows[keep], cols[keep]
        m = len(rows)
        if kind == "exact":
            v = rng.integers(1, 9, m) * rng.choice([-1, 1], m) + (1j * rng.integers(-8, 9, m) if val == "complex" else 0)
        else:
            v = rng.standard_normal(m) + (1j * rng.standard_normal(m) if val == "complex" else 0)
        A = sp.csr_matrix((np.asarray(v, dtype=C128 if val == "complex" else np.float64), (rows, cols)), shape=(n, n))
        A.sort_indices()
        terms.append(A)
    return terms


def stacked_entries(terms):
    """(row, col, term, value) of every stored entry, sorted by (row, col, term): the order of the stacked CSR"""
    r = np.concatenate([np.repeat(np.arange(A.shape[0]), np.diff(A.indptr)) for A in terms])
    c = np.concatenate([A.indices for A in terms])
    t = np.concatenate([np.full(A.nnz, i) for i, A in enumerate(terms)])
    v = np.concatenate([A.data.astype(C128) for A in terms])
    o = np.lexsort((t, c, r))
    return r[o], c[o], t[o], v[o]


class BlockProd(Prim):
    """impl(n, terms, r, q, Y, ldy, ylead, G, alpha, beta, Z, ldz, zlead) -> the buffer Z after the call.

    terms: mt scipy CSR matrices (all float64 or all complex128).  Y: flat buffer, `ylead` sentinels, then the n x r column-major
    block (ldy) with NaN or sentinel padding.  G: flat, G_t (r x q, column-major) at t r q.  Z: flat, `zlead` sentinels, then the
    n x q block (ldz): NaN where beta == 0, operands otherwise; padding NaN or sentinels.  The checker verifies that the inputs
    and the lead and padding of Z kept their values."""
    name = "nep_spmf_blockprod"
    mutants = ("g_transposed", "table_swap", "beta_when_zero", "beta_ignored", "alpha_conj", "skip_last_group", "row_cap64",
               "pad_write", "perturb")

    def shapes(self):
        for t, (n, mt, rq, ab, val, pad, kind) in enumerate(covering_shapes()):
            yield n, mt, rq, ab, val, pad, kind, (LEAD if t % 2 == 0 else 0), (NAN if t % 3 == 0 else SENT)

    def cases(self):
        for n, mt, (r, q), (al, be), val, pad, kind, lead, fill in self.shapes():
            cid = "mt%d_r%dq%d_a%gb%g_%s_pad%d_lead%d_%s" % (mt, r, q, abs(al), abs(be), val, pad, lead, "nan" if fill is NAN else "sent")
            yield Case("n%d" % n, cid, kind, partial(self._build, n, mt, r, q, al, be, val, pad, kind, lead, fill))

    @staticmethod
    def _build(n, mt, r, q, al, be, val, pad, kind, lead, fill):
        rng = np.random.default_rng(_seed("blockprod%d.%d.%d.%d.%g.%s%d%s%d" % (n, mt, r, q, abs(al), val, pad, kind, lead)))
        op = (lambda shape: gint(rng, shape, -4, 4)) if kind == "exact" else (lambda shape: grand(rng, shape))
        terms = make_terms(rng, n, mt, val, kind)
        Y = colmajor_buf(op((n, r)), n + pad, fill=fill, lead=lead); Y[:lead] = SENT
        G = np.concatenate([op((r, q)).reshape(-1, order="F") for _ in range(mt)])
        Z0 = op((n, q)) if be != 0 else np.full((n, q), NAN, dtype=C128)
        Z = colmajor_buf(Z0, n + pad, fill=fill, lead=lead); Z[:lead] = SENT
        return dict(n=n, terms=terms, r=r, q=q, Y=Y, ldy=n + pad, ylead=lead, G=G, alpha=complex(al), beta=complex(be), Z=Z,
                    ldz=n + pad, zlead=lead)

    @staticmethod
    def _block(buf, lead, rows, k, ld):
        return np.lib.stride_tricks.as_strided(buf[lead:], shape=(rows, k), strides=(buf.itemsize, ld * buf.itemsize))

    def values(self, n, terms, r, q, Y, ldy, ylead, G, alpha, beta, Z, ldz, zlead, mut=None, dt=C128, absolute=False):
        """the n x q result in type dt; absolute: the same expression on absolute values (the S of the bound)"""
        ab = (lambda x: np.abs(x)) if absolute else (lambda x: x)
        Ym = ab(np.array(self._block(Y, ylead, n, r, ldy))).astype(dt)
        mt = len(terms)
        Gt = [ab(G[t * r * q: (t + 1) * r * q]).astype(dt) for t in range(mt)]
        Gm = [g.reshape(r, q) if mut == "g_transposed" else g.reshape(r, q, order="F") for g in Gt]
        if mut == "table_swap" and mt > 1:
            Gm[0], Gm[1] = Gm[1], Gm[0]
        er, ec, et, ev = stacked_entries(terms)
        if mut == "row_cap64":
            first = np.searchsorted(er, er, side="left")
            keep = np.arange(len(er)) - first < ROW_CAP
            er, ec, et, ev = er[keep], ec[keep], et[keep], ev[keep]
        acc = np.zeros((n, q), dtype=dt)
        for t in range(mt):
            m = et == t
            Wt = Ym @ Gm[t]
            np.add.at(acc, er[m], ab(ev[m]).astype(dt)[:, None] * Wt[ec[m]])
        al = ab(np.conj(alpha) if mut == "alpha_conj" else alpha)
        be = ab(beta)
        out = np.asarray(dt(al) * acc)
        if (beta != 0 and mut != "beta_ignored") or mut == "beta_when_zero":
            out = out + dt(be) * ab(np.array(self._block(Z, zlead, n, q, ldz))).astype(dt)
        return out

    def ref(self, n, terms, r, q, Y, ldy, ylead, G, alpha, beta, Z, ldz, zlead, mut=None):
        a = dict(n=n, terms=terms, r=r, q=q, Y=Y, ldy=ldy, ylead=ylead, G=G, alpha=alpha, beta=beta, Z=Z, ldz=ldz, zlead=zlead)
        with np.errstate(invalid="ignore"):
            val = self.values(mut=mut, **a)
        Zb = np.array(Z, copy=True)
        rows = drop_tail(n, GROUP) if mut == "skip_last_group" else n
        self._block(Zb, zlead, n, q, ldz)[:rows, :] = val[:rows]
        if mut == "pad_write":
            end = zlead + ldz * (q - 1) + n
            if end < len(Zb):
                Zb[end] = 0.0
            elif q > 1 and ldz > n:
                Zb[zlead + n] = 0.0
            elif zlead:
                Zb[zlead - 1] = 0.0
        if mut == "perturb":
            i = zlead + n // 2
            Zb[i] = complex(np.nextafter(Zb[i].real, np.inf), Zb[i].imag)
        return Zb

    def check(self, impl, c):
        a = c.args
        n, q, ldz, zlead = a["n"], a["q"], a["ldz"], a["zlead"]
        keep = {k: np.array(a[k], copy=True) for k in ("Y", "G", "Z")}
        keept = [(A.indptr.copy(), A.indices.copy(), A.data.copy()) for A in a["terms"]]
        got = np.asarray(impl(**a))
        for k in ("Y", "G", "Z"):
            assert np.array_equal(a[k], keep[k], equal_nan=True), "the caller's %s was modified" % k
        for A, (ip, ix, dv) in zip(a["terms"], keept):
            assert np.array_equal(A.indptr, ip) and np.array_equal(A.indices, ix) and np.array_equal(A.data, dv)
        assert got.shape == keep["Z"].shape, (self.name, c)
        mask = np.zeros(got.shape, dtype=bool)
        self._block(mask, zlead, n, q, ldz)[:, :] = True
        assert_exact(self.name + " (lead and padding of Z)", c, got[~mask], keep["Z"][~mask])
        val = np.array(self._block(got, zlead, n, q, ldz))
        want, bound = self.reference_and_bound(a, exact=c.kind == "exact")
        if c.kind == "exact":
            assert_exact(self.name, c, val, want)
        else:
            assert_bounded(self.name, c, val, want, bound)

    def reference_and_bound(self, a, exact=False):
        n, r = a["n"], a["r"]
        with np.errstate(invalid="ignore"):
            S = np.real(self.values(absolute=True, dt=CLD, **a)).astype(np.float64)
        E_row = sum(np.diff(A.indptr) for A in a["terms"])
        bound = np.array([cbound(int(E) + r + 4, 1.0) for E in E_row])[:, None] * S
        if exact:
            assert_below_2_53(2 * S)
            return self.values(**a), bound
        return self.values(dt=CLD, **a), bound


BLOCKPROD = BlockProd()


# ================================================================================================================================
# dense restatement of the block Newton method (D. Kressner, Numer. Math. 114 (2009); src/method_blocknewton.jl:60-243)
class RefBlockNep:
    """M(lam) = sum_t f_t(lam) A_t with dense matrices; fm[t](S) is the matrix function f_t(S)"""

    def __init__(self, Av, fm):
        dn = lambda A: np.asarray(A.toarray() if hasattr(A, "toarray") else A, dtype=complex)
        self.Av = [dn(A) for A in Av]
        self.fm = list(fm)
        self.n = self.Av[0].shape[0]

    def MM(self, S, X):
        S = np.atleast_2d(np.asarray(S, dtype=complex))
        return sum(A @ X @ f(S) for A, f in zip(self.Av, self.fm))

    def Mder(self, lam):
        return sum(A * f(np.array([[lam]], dtype=complex))[0, 0] for A, f in zip(self.Av, self.fm))


def ref_dep_of(nep, tau=1.0):
    """the dense restatement of a product DEP -lam I + A0 + A1 exp(-tau lam) (its matrices are inputs, not results)"""
    A = nep.A
    n = A[0].shape[0]
    return RefBlockNep([np.eye(n), A[0], A[1]], [lambda S: -S, lambda S: np.eye(S.shape[0], dtype=complex), lambda S: sla.expm(-tau * S)])


def Vl(X, S):
    """[X; X S; ...; X S^(p-1)], :221-228"""
    return np.vstack([X @ np.linalg.matrix_power(S, j) for j in range(S.shape[0])])


def pair_residual(nep, S, X):
    return np.linalg.norm(nep.MM(S, X), 2)


def sigma_min(nep, lam):
    return np.linalg.svd(nep.Mder(lam), compute_uv=False)[-1]


def constraint_tables(S, i, l):
    """the small matrices of the orthogonality rows for column i of the upper triangular S, as the reference forms them (:184-189,
    :207-212): D[j] multiplies W_j^H X in T22 (D[1] = I, D[j + 1] = s D[j] + S^(j-1)), P[j] = S^(j-1) gives the row that multiplies
    W_j^H dx_i in update (22).  Index 0 is unused (W_0 only enters T21)."""
    p = S.shape[0]
    s = S[i, i]
    D = [None, np.eye(p, dtype=complex)]
    for j in range(1, l - 1):
        D.append(s * D[j] + np.linalg.matrix_power(S, j - 1))
    P = [None] + [np.linalg.matrix_power(S, j - 1) for j in range(1, l)]
    return D, P


def update22_tables(S, ds, i, l):
    """E[j] (j = 1 .. l - 1) of update (22): E[1] = ds e_i^T, E[j + 1] = E[j] S + S^(j-1) E[j] (:199, :211)"""
    p = S.shape[0]
    E = [None, np.zeros((p, p), dtype=complex)]
    E[1][:, i] = ds
    for j in range(1, l - 1):
        E.append(E[j] @ S + np.linalg.matrix_power(S, j - 1) @ E[j])
    return E


def bordered_solve(T11, T12, T21, T22, b1, b2, bordered, refine):
    """[T11 T12; T21 T22] [x1; x2] = [b1; b2]: "whole" factorises the bordered matrix (:190-191); "eliminate" goes through the
    factors of T11 and the p x p Schur complement, followed by `refine` steps of iterative refinement on the bordered system, each
    correction by the same elimination"""
    n = T11.shape[0]
    if bordered == "whole":
        sol = np.linalg.solve(np.block([[T11, T12], [T21, T22]]), np.concatenate([b1, b2]))
        return sol[:n], sol[n:]
    solve11 = lambda B: np.linalg.solve(T11, B)                           # the same LU of T11 every time it is called
    Y2 = solve11(T12)
    Sc = T22 - T21 @ Y2

    def elim(c1, c2):
        y1 = solve11(c1)
        z2 = np.linalg.solve(Sc, c2 - T21 @ y1)
        return y1 - Y2 @ z2, z2
    x1, x2 = elim(b1, b2)
    for _ in range(refine):
        d1, d2 = elim(b1 - T11 @ x1 - T12 @ x2, b2 - T21 @ x1 - T22 @ x2)
        x1, x2 = x1 + d1, x2 + d2
    return x1, x2


def ref_newtonstep(nep, S, X, W, RT, RV, bordered="whole", refine=2):
    """one Newton correction (dS, dX) for an upper triangular S, column by column (Kressner (20)-(22), :147-216)"""
    n, p = X.shape
    l = len(W)
    RT = RT.copy(); RV = RV.copy()
    dX = np.zeros((n, p), dtype=complex); dS = np.zeros((p, p), dtype=complex)
    fS = [f(S) for f in nep.fm]
    I = np.eye(p)
    O = np.zeros((p, p))
    for i in range(p):
        s = S[i, i]
        D, P = constraint_tables(S, i, l)
        T11 = nep.Mder(s)
        Se = np.block([[S, I], [O, s * I]])
        T12 = sum(A @ X @ f(Se)[:p, p:] for A, f in zip(nep.Av, nep.fm))
        T21 = sum(s ** j * W[j].conj().T for j in range(l))
        T22 = sum((W[j].conj().T @ X @ D[j] for j in range(1, l)), np.zeros((p, p), dtype=complex))
        dX[:, i], dS[:, i] = bordered_solve(T11, T12, T21, T22, RT[:, i], RV[:, i], bordered, refine)
        if i < p - 1:
            Zi = np.zeros((p, p), dtype=complex); Zi[:, i] = dS[:, i]
            S2 = np.block([[S, Zi], [O, S]])
            for t, (A, f) in enumerate(zip(nep.Av, nep.fm)):              # (21)
                RT[:, i + 1:] -= A @ (np.outer(dX[:, i], fS[t][i, i + 1:]) + X @ f(S2)[:p, p + i + 1:])
            E = update22_tables(S, dS[:, i], i, l)
            for j in range(1, l):                                         # (22)
                RV[:, i + 1:] -= W[j].conj().T @ (np.outer(dX[:, i], P[j][i, i + 1:]) + X @ E[j][:, i + 1:])
    return dS, dX


def ref_blocknewton(nep, S=None, X=None, tol=EPS * 100, maxit=10, armijo_factor=1.0, armijo_max=5, bordered="whole", refine=2):
    """:60-140.  Returns (S, X, iterations, errhist, converged): after `maxit` corrections without ||M(S, X)||_2 < tol the last
    pair comes back with converged = False (the reference throws NoConvergenceException there)."""
    n = nep.n
    S = np.zeros((2, 2), dtype=complex) if S is None else np.array(S, dtype=complex)
    X = np.eye(n, 2, dtype=complex) if X is None else np.array(X, dtype=complex)
    p = S.shape[0]
    V = Vl(X, S)
    W = [V[j * n:(j + 1) * n] for j in range(p)]                          # :72-77: not orthonormalised before the first step
    hist = []
    for k in range(maxit):
        e0 = pair_residual(nep, S, X)
        hist.append(e0)
        if e0 < tol:
            return S, X, k, hist, True
        Res = nep.MM(S, X)
        RR, QQ = sla.schur(S, output="complex")
        dSt, dXt = ref_newtonstep(nep, RR, X @ QQ, W, Res @ QQ, np.zeros((p, p), dtype=complex), bordered=bordered, refine=refine)
        DX = -dXt @ QQ.conj().T; DS = -QQ @ dSt @ QQ.conj().T
        j = 0
        if armijo_factor < 1:                                             # :233-244
            while pair_residual(nep, S + DS, X + DX) > e0 and j < armijo_max:
                j += 1; DS = DS * armijo_factor; DX = DX * armijo_factor
        St, Xt = S + DS, X + DX
        Wq, R = np.linalg.qr(Vl(Xt, St))
        W = [Wq[j * n:(j + 1) * n] for j in range(p)]
        Ri = np.linalg.inv(R)
        X = Xt @ Ri; S = R @ St @ Ri
    return S, X, maxit, hist, False
