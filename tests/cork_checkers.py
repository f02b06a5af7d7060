"""Reference, error bound and case list for nep_cork_expand (csrc/cork.hip), and a dense NumPy restatement of svAAA, the three
compact pencils and AAAeigs written from the reference (src/method_AAAeigs.jl), not from the product.

Style and helpers of tests/border_checkers.py: `CorkExpand.check(impl, case)` runs `impl` on flat complex128 buffers and compares
with a plain reference; test_gpu_aaaeigs.py passes an adapter that calls the library, test_host_aaaeigs.py passes the float64 NumPy
implementation and its mutants.

The kernel forms, from U (r x k), G (k x c), u (r, optional), g (c) and a complex alpha,
    Out[rho, gam] = alpha u[rho] g[gam] + sum_{q < k} U[rho, q] G[q, gam].

Error bound of the rounded cases.  t = alpha u[rho] is one complex product: |dt| <= cbound(1, |alpha| |u[rho]|) (cbound's six extra
roundings are not needed and only widen it).  With the computed t, Out[rho, gam] is a sum of k + 1 complex products, the k of U G
and t g[gam], and the error of t reaches it through |g[gam]|:
    |dOut[rho, gam]| <= cbound(k + 1, sum_q |U[rho, q]| |G[q, gam]| + |t| |g[gam]|) + |g[gam]| |dt|,     |t| <= |alpha| |u[rho]| + |dt|.
Without the rank-1 term the bound is cbound(k, sum_q |U[rho, q]| |G[q, gam]|).  Nothing is fitted to a device result.  The largest
error / bound ratio seen is recorded in primitive_checkers.RATIOS.
"""
from functools import partial
from itertools import product

import numpy as np
import scipy.linalg as sla

from primitive_checkers import (C128, CLD, NAN, SENT, U as UNIT, RATIOS, Case, Prim, _seed, cbound, operand, colmajor_buf, cm_view,   # noqa: F401
                                assert_exact, assert_bounded, assert_below_2_53)

EPS = np.finfo(float).eps

# ================================================================================================================================
# nep_cork_expand
CK_R = [1, 2, 63, 64, 65, 101, 257]
CK_K = [1, 2, 7, 33, 64, 65, 105, 256]
LEAD, TRAIL = 3, 3


def ck_cols(k):
    return sorted({1, 3, 4, k})


class CorkExpand(Prim):
    """impl(r, k, c, U, ldu, G, ldg, u, g, alpha, out, ldo) -> the out buffer after the call.

    U: r x k (ldu) column-major flat buffer whose padding rows hold NaN.  G: k x c (ldg) column-major, padding NaN.  u: r entries or
    None (no rank-1 term; g is then None too).  out: LEAD sentinels, the r x c block (ldo) whose padding rows hold sentinels and
    whose entries are prefilled with NaN, TRAIL sentinels.  The checker verifies that everything but the r x c entries kept its
    value."""
    name = "nep_cork_expand"
    mutants = ("alpha_dropped", "rank1_dropped", "g_conj", "G_transposed", "k_minus_one", "skip_last_row", "pad_write", "perturb")

    def shapes(self):
        t = 0
        for r, k in product(CK_R, CK_K):
            for c in ck_cols(k):
                kind = "rounded" if t % 3 == 0 else "exact"
                rank1 = t % 2 == 0
                alpha = 1.0 if (t // 2) % 2 == 0 else ((2.0 - 3.0j) if kind == "exact" else (0.75 - 1.5j))
                pu, po, pg = 3 * ((t // 4) % 2), 2 * ((t // 8) % 2) + (t % 5 == 0), (t // 3) % 2
                yield r, k, c, kind, rank1, alpha, pu, po, pg
                t += 1
        for r, k, c in ((65, 33, 33), (257, 7, 4), (2, 256, 3), (101, 65, 65)):      # both kinds with the rank-1 term and a complex alpha
            for kind in ("exact", "rounded"):
                yield r, k, c, kind, True, ((2.0 - 3.0j) if kind == "exact" else (0.75 - 1.5j)), 3, 2, 1

    def cases(self):
        for r, k, c, kind, rank1, alpha, pu, po, pg in self.shapes():
            yield Case("r%d" % r, "k%d_c%d_%s_a%s_pad%d%d%d" % (k, c, "rank1" if rank1 else "plain", "1" if alpha == 1.0 else "c", pu, po, pg),
                       kind, partial(self._build, r, k, c, kind, rank1, alpha, pu, po, pg))

    @staticmethod
    def _build(r, k, c, kind, rank1, alpha, pu, po, pg):
        rng = np.random.default_rng(_seed("corkexpand%d.%d.%d%s%d%d%d%d" % (r, k, c, kind, rank1, pu, po, pg)))
        Um = operand(kind, rng, (r, k)); Gm = operand(kind, rng, (k, c))
        u = operand(kind, rng, r) if rank1 else None
        g = operand(kind, rng, c) if rank1 else None
        ldu, ldg, ldo = r + pu, k + pg, r + po
        out = np.full(LEAD + ldo * c + TRAIL, SENT, dtype=C128)
        blk = out[LEAD: LEAD + ldo * c].reshape(c, ldo)
        blk[:, :r] = NAN
        return dict(r=r, k=k, c=c, U=colmajor_buf(Um, ldu), ldu=ldu, G=colmajor_buf(Gm, ldg), ldg=ldg, u=u, g=g, alpha=complex(alpha),
                    out=out, ldo=ldo)

    @staticmethod
    def _operands(r, k, c, U, ldu, G, ldg, u, g, dt):
        Um = cm_view(U, 0, r, k, ldu).astype(dt); Gm = cm_view(G, 0, k, c, ldg).astype(dt)
        return Um, Gm, (None if u is None else u.astype(dt)), (None if g is None else g.astype(dt))

    def ref(self, r, k, c, U, ldu, G, ldg, u, g, alpha, out, ldo, mut=None, dt=C128, parts=False):
        Um, Gm, uv, gv = self._operands(r, k, c, U, ldu, G, ldg, u, g, dt)
        if mut == "G_transposed" and c == k:
            Gm = Gm.T
        kk = k - 1 if mut == "k_minus_one" else k
        val = Um[:, :kk] @ Gm[:kk, :] if kk > 0 else np.zeros((r, c), dtype=dt)
        if uv is not None and mut != "rank1_dropped":
            a = dt(1.0) if mut == "alpha_dropped" else dt(alpha)
            val = val + np.outer(a * uv, np.conj(gv) if mut == "g_conj" else gv)
        if parts:
            return val
        res = np.array(out, copy=True)
        blk = res[LEAD: LEAD + ldo * c].reshape(c, ldo)
        blk[:, :r] = val.T
        if mut == "skip_last_row":
            blk[:, r - 1] = out[LEAD: LEAD + ldo * c].reshape(c, ldo)[:, r - 1]
        if mut == "pad_write":
            res[LEAD + ldo * (c - 1) + r] = 0.0                        # the entry behind the last one: padding or the first trailing sentinel
        if mut == "perturb":                                           # one ulp in one real part
            i = (c // 2) * ldo + r // 2
            blk.reshape(-1)[i] = complex(np.nextafter(blk.reshape(-1)[i].real, np.inf), blk.reshape(-1)[i].imag)
        return res

    def check(self, impl, c):
        a = c.args
        r, k, cc, ldo = a["r"], a["k"], a["c"], a["ldo"]
        out0 = np.array(a["out"], copy=True)
        keep = [np.array(a[n], copy=True) for n in ("U", "G")]
        got = np.asarray(impl(**a))
        assert got.shape == out0.shape, (self.name, c)
        for n, b in zip(("U", "G"), keep):
            assert np.array_equal(a[n], b, equal_nan=True), "%s was modified" % n
        mask = np.zeros(out0.shape, dtype=bool)
        mask[LEAD: LEAD + ldo * cc].reshape(cc, ldo)[:, :r] = True
        assert_exact(self.name + " (sentinels and padding of out)", c, got[~mask], out0[~mask])
        val = got[LEAD: LEAD + ldo * cc].reshape(cc, ldo)[:, :r].T
        if c.kind == "exact":
            want, bound = self.reference_and_bound(a, exact=True)
            assert_exact(self.name, c, val, want)
        else:
            want, bound = self.reference_and_bound(a)
            assert_bounded(self.name, c, val, want, bound)

    def reference_and_bound(self, a, exact=False):
        """the r x c results (np.clongdouble, or complex128 for an exact case after the magnitudes are checked) and the bound of the
        module docstring on |computed - exact|"""
        r, k, cc = a["r"], a["k"], a["c"]
        Um, Gm, uv, gv = self._operands(r, k, cc, a["U"], a["ldu"], a["G"], a["ldg"], a["u"], a["g"], C128)
        S = np.abs(Um) @ np.abs(Gm)
        if uv is None:
            bound = cbound(k, S)
        else:
            at = abs(a["alpha"]) * np.abs(uv)
            dt_ = cbound(1, at)
            bound = cbound(k + 1, S + np.outer(at + dt_, np.abs(gv))) + np.outer(dt_, np.abs(gv))
            S = S + np.outer(at, np.abs(gv))
        if exact:
            assert_below_2_53(2 * S)
            return self.ref(parts=True, **a), bound
        return self.ref(parts=True, dt=CLD, **a), bound


CORK = CorkExpand()


# ================================================================================================================================
# dense restatement of src/method_AAAeigs.jl
class RefAAANep:
    """M(lam) = sum_i lam^i P_i + sum_i f_i(lam) A_i with dense matrices; fv are callables on NumPy arrays.  `pep_first` says on
    which side of the SumNEP the PEP stands (it changes nothing in the mathematics)."""

    def __init__(self, Av, fv, pep_Av=None):
        dn = lambda A: np.asarray(A.toarray() if hasattr(A, "toarray") else A, dtype=complex)
        self.Av = [dn(A) for A in Av]
        self.fv = list(fv)
        self.pep_Av = None if pep_Av is None else [dn(A) for A in pep_Av]
        self.n = self.Av[0].shape[0]

    def Mder(self, lam):
        M = sum(complex(f(np.array([lam], dtype=complex))[0]) * A for f, A in zip(self.fv, self.Av))
        if self.pep_Av is not None:
            M = M + sum(lam ** i * P for i, P in enumerate(self.pep_Av))
        return M

    def residual(self, lam, x):
        return np.linalg.norm(self.Mder(lam) @ x) / np.linalg.norm(x)

    def residuals(self, lams, X):
        """||M(lam_i) x_i|| / ||x_i|| for the columns of X: every matrix multiplies the whole block once"""
        lams = np.asarray(lams, dtype=complex)
        with np.errstate(all="ignore"):
            Rm = sum((A @ X) * f(lams)[None, :] for f, A in zip(self.fv, self.Av))
            if self.pep_Av is not None:
                Rm = Rm + sum((P @ X) * (lams ** i)[None, :] for i, P in enumerate(self.pep_Av))
            return np.linalg.norm(Rm, axis=0) / np.linalg.norm(X, axis=0)


def ref_dep(A0, A1, tau=1.0):
    n = A0.shape[0]
    return RefAAANep([np.eye(n), A0, A1], [lambda l: -l, lambda l: np.ones_like(l), lambda l: np.exp(-tau * l)])


def ref_reval(lam, z, fz, w):
    """:724-747 without the special cases: the barycentric formula at points that are neither support points nor infinite"""
    lam = np.atleast_1d(np.asarray(lam, dtype=complex))
    C = 1.0 / (lam[:, None] - np.asarray(z)[None, :])
    return (C @ (np.asarray(w)[:, None] * np.asarray(fz))) / (C @ np.asarray(w))[:, None]


def ref_svAAA(fv, Z, mmax=100, tol=EPS * 1e3, weighted=False, Av=None, u0=None):
    """:469-721 without the cleanup: greedy support points, weights from a FULL singular value decomposition of the Loewner matrix
    over the rows that are not support points (the reference updates a QR factorisation of the same matrix instead).
    Returns (z, fz, w, err)."""
    Z = np.asarray(Z, dtype=complex).reshape(-1)
    Z = Z[np.isfinite(Z)]
    M, s = len(Z), len(fv)
    F = np.column_stack([f(Z) for f in fv]).astype(complex)
    if weighted:
        n = Av[0].shape[0]
        u = np.ones(n, dtype=complex) if u0 is None else np.asarray(u0, dtype=complex)
        u = u / np.linalg.norm(u)
        uj = np.column_stack([A @ u for A in Av])
        beta = max(np.linalg.norm(uj @ F[i, :]) for i in range(M))
        nrm = np.array([np.linalg.norm(A) for A in Av])
        F = F * nrm[None, :]
        scaleF = 1.0 / nrm
    else:
        scaleF = np.max(np.abs(F), axis=0)
        F = F / scaleF[None, :]
    R = np.tile(F.mean(axis=0), (M, 1))
    z, ind, err = [], [], []
    w = np.zeros(0, dtype=complex)
    for m in range(1, mmax + 2):
        res = np.abs(F - R)
        maxres = res.max(axis=0)
        col = int(np.argmax(maxres))
        locz = int(np.argmax(res[:, col]))
        err.append(maxres.sum() / beta if weighted else res[locz, col])
        if err[-1] <= tol or m == mmax + 1:
            break
        z.append(Z[locz]); ind.append(locz)
        rest = np.setdiff1d(np.arange(M), ind)
        zs = np.array(z)
        C = 1.0 / (Z[rest][:, None] - zs[None, :])
        Lw = np.vstack([C * (F[rest, j][:, None] - F[ind, j][None, :]) for j in range(s)])
        w = np.linalg.svd(Lw, full_matrices=Lw.shape[0] < m)[2][-1].conj()
        R = F.copy()
        R[rest, :] = (C @ (w[:, None] * F[ind, :])) / (C @ w)[:, None]
    return np.array(z), scaleF[None, :] * F[ind, :], w, np.array(err)


def ref_compact_pencil(d, s, m, z, fz, w, NNZ):
    """get_compact_pencil, :91-120, block by block as the reference writes it"""
    z, w = np.asarray(z, dtype=complex), np.asarray(w, dtype=complex)
    fz = np.asarray(fz, dtype=complex).reshape(m, s)
    dt = len(NNZ)
    Z_ = lambda a, b: np.zeros((a, b), dtype=complex)

    def spdiagm(rows, cols, diags):
        T = Z_(rows, cols)
        for off, v in diags.items():
            for i, x in enumerate(np.atleast_1d(v)):
                T[i - min(off, 0), i + max(off, 0)] = x
        return T
    TA = spdiagm(m, m - 1, {0: -w[1:] * z[:-1], -1: w[:-1] * z[1:]})
    TB = spdiagm(m, m - 1, {0: -w[1:], -1: w[:-1]})
    if dt == 0:
        return np.hstack([fz, TA]), np.hstack([Z_(m, s), TB])
    if d == 0:
        A = np.vstack([Z_(1, 1 + s + m), np.hstack([Z_(m, 1), fz, TA, np.ones((m, 1))])])
        A[0, 0] = 1; A[0, -1] = -1
        B = np.vstack([Z_(1, 1 + s + m), np.hstack([Z_(m, 1 + s), TB, Z_(m, 1)])])
        return A, B
    P = Z_(d, dt - 1)
    for c_, deg in enumerate(NNZ[:-1]):
        P[deg, c_] = 1                                                  # sparse(NNZ[1:end-1] .+ 1, 1:dt-1, ones(dt-1), d, dt-1), 1-based rows
    A = np.vstack([np.hstack([P, Z_(d, s + 1), spdiagm(d, d - 1, {-1: np.ones(d - 1)}), Z_(d, m)]),
                   np.hstack([Z_(m, dt), fz, Z_(m, d - 1), TA, np.ones((m, 1))])])
    A[0, -1] = -1
    B = np.vstack([np.hstack([Z_(d, dt + s), spdiagm(d, d - 1, {0: np.ones(d - 1)}), Z_(d, m)]),
                   np.hstack([Z_(m, dt + s + d - 1), TB, Z_(m, 1)])])
    B[d - 1, dt - 1] = -1
    return A, B


def ref_pencil_of(nep, Z, mmax=100, tol_appr=EPS * 1e3, weighted=False):
    """AAAPencil, :42-88 (NNZ: degrees of the non-zero PEP coefficients, trailing zeros dropped)"""
    z, fz, w, err = ref_svAAA(nep.fv, Z, mmax=mmax, tol=tol_appr, weighted=weighted, Av=nep.Av)
    keep = w != 0
    z, fz, w = z[keep], fz[keep], w[keep]
    NNZ = [] if nep.pep_Av is None else [i for i, P in enumerate(nep.pep_Av) if np.any(P)]
    d = NNZ[-1] if NNZ else 0
    PPCC = ([nep.pep_Av[i] for i in NNZ] if NNZ else []) + nep.Av
    s, m = len(nep.Av), len(z)
    A, B = ref_compact_pencil(d, s, m, z, fz, w, NNZ)
    return dict(d=d, s=s, m=m, NNZ=NNZ, PPCC=PPCC, A=A, B=B, z=z, fz=fz, w=w, err=err)


def ref_level2_tables(A, B, l, sigma):
    """the straightforward form of :276-287,332-339: returns (compactB [I; Y[2:end, :]], lambda W: W / Mext)"""
    k = A.shape[0]
    Mext = np.hstack([np.eye(k, 1), A[:, l:] - sigma * B[:, l:]])
    Y = np.linalg.solve(Mext, sigma * B[:, :l] - A[:, :l])
    return B @ np.vstack([np.eye(l), Y[1:, :]]), (lambda W: np.linalg.solve(Mext.T, W.T).T)


def ref_AAAeigs(nep, Z, mmax=100, neigs=6, maxit=None, shifts=(), tol=EPS * 1e6, tol_appr=EPS * 1e3, v0=None, weighted=False,
                check_error_every=10, to_maxit=False):
    """AAAeigs, :183-416, in dense arithmetic: W / Mext as written, the reference's Gram-Schmidt rule (up to three more passes while
    the norm drops below 1/sqrt(2)), ResidualErrmeasure.  Returns a dict: lam, X, res (the `neigs` pairs of smallest residual at the
    check that stopped the run), it, m, and `converged`: every Ritz value with residual < tol at that check.  to_maxit: do not stop
    before maxit (the list of all converged Ritz values at maxit).  Raises RuntimeError without convergence (unless to_maxit)."""
    if maxit is None:
        maxit = int(min(max(10 * neigs, 30), 100))
    n = nep.n
    shifts = np.asarray(shifts, dtype=complex).reshape(-1)
    if len(shifts) == 0:
        shifts = np.zeros(1, dtype=complex)
    sig = np.array([shifts[i % len(shifts)] for i in range(maxit)])
    P = ref_pencil_of(nep, Z, mmax=mmax, tol_appr=tol_appr, weighted=weighted)
    d, dt, m, s, A, B = P["d"], len(P["NNZ"]), P["m"], P["s"], P["A"], P["B"]
    k = d + m + (1 if d == 0 and dt != 0 else 0)
    l = dt + s
    Q = np.zeros((n, maxit + 1), dtype=complex)
    v0 = np.asarray(v0, dtype=complex)
    Q[:, 0] = v0 / np.linalg.norm(v0)
    U = np.zeros((maxit + 1, k, maxit + 1), dtype=complex)
    U[0, 0, 0] = 1.0
    H = np.zeros((maxit + 1, maxit), dtype=complex); K = np.zeros((maxit + 1, maxit), dtype=complex)
    lus = {}
    r, j, nconv = 1, 1, 0
    out = None
    it = 1
    while it <= maxit and (nconv < neigs or to_maxit):
        sg = sig[it - 1]
        Cfull, right_div = ref_level2_tables(A, B, l, sg)
        u_c = U[:r, :, j - 1] @ Cfull
        v = np.zeros(n, dtype=complex)
        for i in range(l):
            v += P["PPCC"][i] @ (Q[:, :r] @ u_c[:, i])
        if sg not in lus:
            lus[sg] = sla.lu_factor(nep.Mder(sg))
        v = sla.lu_solve(lus[sg], v)
        if dt == 0:
            phi0 = P["w"] / (sg - P["z"])
            v = (phi0[0] / phi0.sum()) * v
        nv = np.linalg.norm(v)
        u1 = Q[:, :r].conj().T @ v
        v = v - Q[:, :r] @ u1
        ii = 0
        while ii < 3 and np.linalg.norm(v) < nv / np.sqrt(2):
            nv = np.linalg.norm(v)
            un = Q[:, :r].conj().T @ v
            v = v - Q[:, :r] @ un
            u1 = u1 + un
            ii += 1
        nv = np.linalg.norm(v)
        if nv > EPS:
            rnew = r + 1
            Q[:, rnew - 1] = v / nv
            u1 = np.concatenate([u1, [nv]])
        else:
            rnew = r
        W = np.zeros((rnew, k), dtype=complex)
        W[:, 0] = u1
        W[:, 1:] = U[:rnew, :, j - 1] @ B[:, l:]
        Uhat = right_div(W)
        Urs = U[:rnew, :, :j].reshape(rnew * k, j, order="F")
        uh = Uhat.reshape(rnew * k, order="F").copy()
        nu = np.linalg.norm(uh)
        h = Urs.conj().T @ uh
        uh = uh - Urs @ h
        hb = np.linalg.norm(uh)
        ii = 0
        while ii < 3 and hb < nu / np.sqrt(2):
            hn = Urs.conj().T @ uh
            uh = uh - Urs @ hn
            h = h + hn
            nu = hb
            hb = np.linalg.norm(uh)
            ii += 1
        H[:j, j - 1] = h; H[j, j - 1] = hb
        U[:rnew, :, j] = (uh / hb).reshape(rnew, k, order="F")
        K[:j, j - 1] = sg * h
        K[j - 1, j - 1] += 1
        K[j, j - 1] = hb * sg
        if it % check_error_every == 0 or it == maxit:
            lam, S = sla.eig(K[:j, :j], H[:j, :j])
            X = Q[:, :rnew] @ (U[:rnew, 0, :j + 1] @ (H[:j + 1, :j] @ S))
            res = nep.residuals(lam, X)
            res[~np.isfinite(res)] = np.inf
            conv = res < tol
            nconv = int(conv.sum())
            idx = np.argsort(res, kind="stable")
            if it == maxit or nconv >= neigs:
                nb = int(min(len(lam), neigs))
                out = dict(lam=lam[idx[:nb]], X=X[:, idx[:nb]], res=res[idx[:nb]], it=it, m=m, r=rnew, converged=lam[conv],
                           converged_res=res[conv], nconv=nconv)
        r = rnew
        j += 1
        it += 1
    if nconv < neigs and not to_maxit:
        raise RuntimeError("ref_AAAeigs: Number of iterations exceeded. maxit=%d." % maxit)
    return out
