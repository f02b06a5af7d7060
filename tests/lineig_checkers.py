"""Reference, error bound and case list for nep_basis_rotate (K13, csrc/lineig.hip), a dense NumPy restatement of the method of
successive linear problems written from the mathematics (A. Ruhe, SIAM J. Numer. Anal. 10 (1973): solve M(lam) x = d M'(lam) x for
the d of smallest modulus, lam <- lam - d), and helpers for the dense spectrum of a pencil with first-order condition numbers.

Style and helpers of tests/blocknewton_checkers.py: `ROTATE.check(impl, case)` runs `impl` on flat complex128 buffers and compares
with a plain reference; test_gpu_lineig.py passes an adapter that calls the library, test_host_lineig.py passes the NumPy
implementation and its mutants.

The kernel computes, in place, on a rows x (m + 1) column-major block V (leading dimension ldv) and an m x p table Q (ldq)

    V[:, 0:p] <- V[:, 0:m] Q;      carry: V[:, p] <- V[:, m].

What the checker holds fixed: the lead in front of the block, the padding rows .. ldv - 1 of every column, the column m + 1, and
column m itself (it is only ever a source; with carry = 0 it holds a sentinel and must be neither read nor written: a caller
without a residual vector has no such column).  The columns p + carry .. m - 1 are outside the contract and ignored.

Error bound of the rounded cases (cbound of primitive_checkers.py): entry (i, c) is an m-term inner product in any summation
order; four more terms are allowed as in the other checkers:  |dV[i, c]| <= cbound(m + 4, (|V| |Q|)[i, c]).  The carry column is a
copy and compared bit for bit.  Nothing is fitted to a device result; the largest error / bound ratio seen is recorded in
primitive_checkers.RATIOS.
"""
from functools import partial

import numpy as np
import scipy.linalg as sla

from primitive_checkers import (C128, CLD, NAN, SENT, RATIOS, Case, Prim, _seed, cbound, gint, grand, drop_tail,      # noqa: F401
                                assert_exact, assert_bounded, assert_below_2_53)

EPS = np.finfo(float).eps

# ================================================================================================================================
# nep_basis_rotate
ROT_ROWS = [1, 2, 63, 64, 65, 257, 1025]
ROT_MP = [(1, 1), (2, 1), (5, 5), (17, 4), (20, 10), (64, 33), (128, 64), (128, 128)]
ROT_CARRY = [0, 1]
ROT_PAD = [0, 3]
ROT_VAL = ["real", "complex"]
ROT_KIND = ["exact", "rounded"]
ROT_FACTORS = [ROT_ROWS, ROT_MP, ROT_CARRY, ROT_PAD, ROT_VAL, ROT_KIND]
LEAD = 3
TILE = 64                                            # the quantum the tail-dropping mutant forgets (rows of a workgroup's tile)


def covering_shapes():
    """every pair of values of two different factors occurs in some shape (the other factors filled by rotation), then every
    (rows, (m, p), carry) triple the same way; duplicates removed"""
    seen, out = set(), []
    t = 0

    def add(fixed):
        nonlocal t
        ix = [(t + 3 * f) % len(F) for f, F in enumerate(ROT_FACTORS)]
        for f, v in fixed.items():
            ix[f] = v
        t += 1
        if tuple(ix) not in seen:
            seen.add(tuple(ix))
            out.append(tuple(F[i] for F, i in zip(ROT_FACTORS, ix)))
    for a in range(len(ROT_FACTORS)):
        for b in range(a + 1, len(ROT_FACTORS)):
            for va in range(len(ROT_FACTORS[a])):
                for vb in range(len(ROT_FACTORS[b])):
                    add({a: va, b: vb})
    for va in range(len(ROT_ROWS)):
        for vb in range(len(ROT_MP)):
            for vc in range(len(ROT_CARRY)):
                add({0: va, 1: vb, 2: vc})
    return out


class Rotate(Prim):
    """impl(rows, m, p, carry, V, ldv, lead, Q, ldq) -> the buffer V after the call.

    V: flat buffer, `lead` sentinels, then m + 2 columns of ldv entries: the columns 0 .. m - 1 of the block, column m (the carry
    source, or a sentinel column when carry == 0), one sentinel column; rows .. ldv - 1 of every column NaN or sentinels.
    Q: flat, column c at c ldq, NaN in the rows m .. ldq - 1.  The checker verifies that Q and everything of V outside the contract
    kept their bits."""
    name = "nep_basis_rotate"
    mutants = ("left_to_right", "no_carry", "carry_first", "drop_tail64", "ld_as_rows", "conj_q", "pcol_write", "perturb")

    def shapes(self):
        for t, (rows, mp, carry, pad, val, kind) in enumerate(covering_shapes()):
            yield rows, mp, carry, pad, val, kind, (LEAD if t % 2 == 0 else 0), (NAN if t % 3 == 0 else SENT)

    def cases(self):
        for rows, (m, p), carry, pad, val, kind, lead, fill in self.shapes():
            cid = "m%dp%d_carry%d_pad%d_%s_lead%d_%s" % (m, p, carry, pad, val, lead, "nan" if fill is NAN else "sent")
            yield Case("rows%d" % rows, cid, kind, partial(self._build, rows, m, p, carry, pad, val, kind, lead, fill))

    @staticmethod
    def _build(rows, m, p, carry, pad, val, kind, lead, fill):
        rng = np.random.default_rng(_seed("rotate%d.%d.%d.%d.%d%s%s%d" % (rows, m, p, carry, pad, val, kind, lead)))
        op = (lambda shape: gint(rng, shape, -4, 4)) if kind == "exact" else (lambda shape: grand(rng, shape))
        if val == "real":
            full = op
            op = lambda shape: full(shape).real.astype(C128)
        ldv, ldq = rows + pad, m + (2 if pad else 0)
        V = np.full(lead + ldv * (m + 2), fill, dtype=C128)
        V[:lead] = SENT
        blk = Rotate._block(V, lead, rows, m + 2, ldv)
        blk[:, :m] = op((rows, m))
        blk[:, m] = op((rows, 1))[:, 0] if carry else SENT
        blk[:, m + 1] = SENT
        Q = np.full(ldq * p, NAN, dtype=C128)
        Rotate._block(Q, 0, m, p, ldq)[:, :] = op((m, p))
        return dict(rows=rows, m=m, p=p, carry=carry, V=V, ldv=ldv, lead=lead, Q=Q, ldq=ldq)

    @staticmethod
    def _block(buf, lead, rows, k, ld):
        return np.lib.stride_tricks.as_strided(buf[lead:], shape=(rows, k), strides=(buf.itemsize, ld * buf.itemsize))

    def values(self, rows, m, p, carry, V, ldv, lead, Q, ldq, dt=C128, absolute=False):
        """the rows x p product in type dt; absolute: the same expression on absolute values (the S of the bound)"""
        ab = (lambda x: np.abs(x)) if absolute else (lambda x: x)
        Vm = ab(np.array(self._block(V, lead, rows, m, ldv))).astype(dt)
        Qm = ab(np.array(self._block(Q, 0, m, p, ldq))).astype(dt)
        return Vm @ Qm

    def ref(self, rows, m, p, carry, V, ldv, lead, Q, ldq, mut=None):
        Vb = np.array(V, copy=True)
        ld = rows if mut == "ld_as_rows" else ldv
        if mut == "ld_as_rows" and ldv == rows:
            ld = ldv
        blk = self._block(Vb, lead, rows, m + 1, ld)
        Qm = np.array(self._block(Q, 0, m, p, ldq))
        if mut == "conj_q":
            Qm = Qm.conj()
        live = drop_tail(rows, TILE) if mut == "drop_tail64" else rows
        src = np.array(blk[:live, :])                                     # the original block
        if mut == "carry_first" and carry:
            blk[:live, p] = src[:, m]
        if mut == "left_to_right":
            for c in range(p):                                            # column c from a block whose columns < c are already new
                blk[:live, c] = blk[:live, :m] @ Qm[:, c]
        else:
            cur = np.array(blk[:live, :m])
            blk[:live, :p] = cur @ Qm
        if carry and mut not in ("no_carry", "carry_first"):
            blk[:live, p] = src[:, m]
        if mut == "pcol_write" and not carry:
            blk[:live, p] = 0.0
        if mut == "perturb":
            i = lead + rows // 2
            Vb[i] = complex(np.nextafter(Vb[i].real, np.inf), Vb[i].imag)
        return Vb

    def check(self, impl, c):
        a = c.args
        rows, m, p, carry, ldv, lead = a["rows"], a["m"], a["p"], a["carry"], a["ldv"], a["lead"]
        keep = {k: np.array(a[k], copy=True) for k in ("V", "Q")}
        got = np.asarray(impl(**a))
        assert np.array_equal(a["Q"], keep["Q"], equal_nan=True), "the caller's Q was modified"
        assert np.array_equal(a["V"], keep["V"], equal_nan=True), "the caller's V buffer was modified (the result is a fresh array)"
        assert got.shape == keep["V"].shape, (self.name, c)
        fixed = np.ones(got.shape, dtype=bool)                            # everything but the columns 0 .. m - 1 of the block
        self._block(fixed, lead, rows, m + 2, ldv)[:, :m] = False
        assert_exact(self.name + " (lead, padding, columns >= m)", c, got[fixed], keep["V"][fixed])
        val = np.array(self._block(got, lead, rows, m + 2, ldv))
        if carry:
            assert_exact(self.name + " (carry column)", c, val[:, p], np.array(self._block(keep["V"], lead, rows, m + 2, ldv))[:, m])
        want, bound = self.reference_and_bound(a, exact=c.kind == "exact")
        if c.kind == "exact":
            assert_exact(self.name, c, val[:, :p], want)
        else:
            assert_bounded(self.name, c, val[:, :p], want, bound)

    def reference_and_bound(self, a, exact=False):
        S = np.real(self.values(absolute=True, dt=CLD, **a)).astype(np.float64)
        bound = cbound(a["m"] + 4, S)
        if exact:
            assert_below_2_53(2 * S)
            return self.values(**a), bound
        return self.values(dt=CLD, **a), bound


ROTATE = Rotate()


# ================================================================================================================================
# dense restatement of the method of successive linear problems
class RefNep:
    """M(lam) = sum_t f_t(lam) A_t with dense matrices; f[t](lam), df[t](lam) the scalar functions and their derivatives"""

    def __init__(self, Av, f, df):
        dn = lambda A: np.asarray(A.toarray() if hasattr(A, "toarray") else A, dtype=complex)
        self.Av = [dn(A) for A in Av]
        self.f, self.df = list(f), list(df)
        self.n = self.Av[0].shape[0]
        self.fro = [np.linalg.norm(A) for A in self.Av]

    def M(self, lam):
        return sum(A * f(lam) for A, f in zip(self.Av, self.f))

    def dM(self, lam):
        return sum(A * f(lam) for A, f in zip(self.Av, self.df))

    def residual(self, lam, v):
        return float(np.linalg.norm(self.M(lam) @ v) / np.linalg.norm(v))

    def backward_error(self, lam, v):
        """||M(lam) v|| / (||v|| sum_t ||A_t||_F |f_t(lam)|): the default error measure of an SPMF"""
        return self.residual(lam, v) / sum(a * abs(f(lam)) for a, f in zip(self.fro, self.f))


def ref_dep_of(nep):
    """the restatement of a product DEP -lam I + sum_i A_i exp(-tau_i lam) (its matrices and delays are inputs, not results)"""
    n = nep.A[0].shape[0]
    f = [lambda l: -l] + [(lambda l, t=t: np.exp(-t * l)) for t in nep.tauv]
    df = [lambda l: -1.0] + [(lambda l, t=t: -t * np.exp(-t * l)) for t in nep.tauv]
    return RefNep([np.eye(n)] + list(nep.A), f, df)


def pencil_spectrum(A, B=None):
    """(d, X, Y, kappa) of the dense pencil A x = d B x: right and left eigenvectors (y^H A = d y^H B) and the first-order
    condition numbers kappa_i = ||y_i|| ||x_i|| / |y_i^H B x_i| (a perturbation E of A, F of B moves a simple d_i by at most
    kappa_i (||E|| + |d_i| ||F||) to first order)"""
    dn = lambda M: np.asarray(M.toarray() if hasattr(M, "toarray") else M, dtype=complex)
    A = dn(A)
    B = np.eye(A.shape[0], dtype=complex) if B is None else dn(B)
    d, Y, X = sla.eig(A, B, left=True, right=True)
    yBx = np.abs(np.einsum("ij,ij->j", Y.conj(), B @ X))
    kappa = np.linalg.norm(Y, axis=0) * np.linalg.norm(X, axis=0) / np.maximum(yBx, np.finfo(float).tiny)
    return d, X, Y, kappa


def nearest(d, target, k):
    """indices of the k entries of d nearest target (infinite eigenvalues last)"""
    dist = np.where(np.isfinite(d), np.abs(d - target), np.inf)
    return np.argsort(dist, kind="stable")[:k]


def nep_condition(nep, lam):
    """kappa(lam) = ||y|| ||x|| / |y^H M'(lam) x| from the left and right vectors of the pencil (M(lam), M'(lam)) at d ~ 0"""
    d, X, Y, kappa = pencil_spectrum(nep.M(lam), nep.dM(lam))
    return float(kappa[nearest(d, 0.0, 1)[0]])


def ref_mslp(nep, lam=0.0, tol=EPS * 100, maxit=100, measure="backward"):
    """Returns (lam, v, iterations, errhist, converged).  Each iteration: the eigenvalue d of smallest modulus of
    M(lam) x = d M'(lam) x, lam <- lam - d, v = x / ||x||, err = the chosen measure at the new lam."""
    lam = complex(lam)
    err_of = nep.backward_error if measure == "backward" else nep.residual
    hist = []
    v = np.zeros(nep.n, dtype=complex)
    for k in range(1, maxit + 1):
        d, X = sla.eig(nep.M(lam), nep.dM(lam))
        i = nearest(d, 0.0, 1)[0]
        lam = lam - d[i]
        v = X[:, i] / np.linalg.norm(X[:, i])
        hist.append(err_of(lam, v))
        if hist[-1] < tol:
            return lam, v, k, hist, True
    return lam, v, maxit, hist, False
