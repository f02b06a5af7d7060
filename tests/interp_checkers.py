"""Reference, error bound and case list for nep_interp_coeffs (csrc/interp.hip), and a dense NumPy restatement of the Chebyshev
interpolation of src/types_cheb_pep.jl written from the reference, not from the product.

Style and helpers of tests/cork_checkers.py: `INTERP.check(impl, case)` runs `impl` on flat NumPy buffers and compares with a plain
reference; test_gpu_chebpep.py passes an adapter that calls the library, test_host_chebpep.py passes the float64 NumPy
implementation and its mutants.

The kernel forms, from F (E x J, entry-major, real or complex), a K x J complex table W, an optional injective row map pos and
beta in {0, 1},
    C[r(e), i] = beta C[r(e), i] + sum_{j < J} W[i, j] F[e, j],      r(e) = pos ? pos[e] : e.

Error bound of the rounded cases: the result is a sum of J complex products, and with beta = 1 of one further term that enters
unrounded, so |dC| <= cbound(J, sum_j |W[i, j]| |F[e, j]|) without and cbound(J + 1, sum_j |W[i, j]| |F[e, j]| + |C_old|) with it
(primitive_checkers.cbound: any summation order, with or without fused multiply-adds).  A real F only removes roundings.  Nothing
is fitted to a device result.  The largest error / bound ratio seen is recorded in primitive_checkers.RATIOS.
"""
from functools import partial
from itertools import product

import numpy as np
from numpy.polynomial import chebyshev as ch
from numpy.polynomial import polynomial as pl

from primitive_checkers import (C128, CLD, NAN, SENT, RATIOS, Case, Prim, _seed, cbound, operand,   # noqa: F401
                                assert_exact, assert_bounded, assert_below_2_53)

EPS = np.finfo(float).eps

IP_E = [1, 63, 64, 65, 257, 4099]
IP_JK = [(1, 1), (1, 13), (2, 5), (5, 2), (13, 13), (20, 64), (64, 20), (64, 64)]
IP_POS = ["none", "perm", "inject"]
LEAD, TRAIL = 3, 3
PAD_F, PAD_C = 2, 3


class InterpCoeffs(Prim):
    """impl(E, J, K, F, ldf, fcomplex, W, pos, beta, C, ldc) -> the C buffer after the call.

    F: flat buffer of E rows of ldf values (float64 when fcomplex is false, complex128 otherwise) whose padding holds NaN.  W: K x J
    complex128 array.  pos: E distinct int32 row numbers or None.  C: LEAD sentinels, `rows` rows of ldc values, TRAIL sentinels;
    the K entries of the rows that are written hold NaN (beta = 0) or the old values (beta = 1), everything else -- padding, rows
    that pos does not name -- sentinels.  The checker verifies that everything but the written entries kept its value."""
    name = "nep_interp_coeffs"
    mutants = ("W_transposed", "W_conj", "first_row_doubled", "beta_ignored", "pos_ignored", "skip_last_entry", "pad_write",
               "real_as_complex", "perturb")

    def shapes(self):
        t = 0
        for E, (J, K), cplx, beta, posm, pad in product(IP_E, IP_JK, (False, True), (0, 1), IP_POS, (False, True)):
            # the parity of the bits of the running index: both kinds meet every PAIR of parameter values (test_host_chebpep.py)
            kind = "rounded" if bin(t).count("1") % 2 == 0 else "exact"
            yield E, J, K, cplx, beta, posm, pad, kind
            t += 1

    def cases(self):
        for E, J, K, cplx, beta, posm, pad, kind in self.shapes():
            yield Case("E%d_J%d_K%d" % (E, J, K), "%s_beta%d_%s_%s" % ("c" if cplx else "r", beta, posm, "pad" if pad else "tight"), kind,
                       partial(self._build, E, J, K, cplx, beta, posm, pad, kind))

    @staticmethod
    def rows_of(E, posm):
        return E + (E // 2 + 3 if posm == "inject" else 0)

    @staticmethod
    def _build(E, J, K, cplx, beta, posm, pad, kind):
        rng = np.random.default_rng(_seed("interp%d.%d.%d%d%d%s%d%s" % (E, J, K, cplx, beta, posm, pad, kind)))
        Fm = operand(kind, rng, (E, J))
        W = operand(kind, rng, (K, J))
        ldf, ldc = J + (PAD_F if pad else 0), K + (PAD_C if pad else 0)
        F = np.full(E * ldf, np.nan, dtype=C128 if cplx else np.float64)
        F.reshape(E, ldf)[:, :J] = Fm if cplx else Fm.real
        rows = InterpCoeffs.rows_of(E, posm)
        pos = None
        if posm == "perm":
            pos = rng.permutation(E).astype(np.int32)
        elif posm == "inject":
            pos = rng.choice(rows, size=E, replace=False).astype(np.int32)
        C = np.full(LEAD + rows * ldc + TRAIL, SENT, dtype=C128)
        blk = C[LEAD: LEAD + rows * ldc].reshape(rows, ldc)
        r = np.arange(E) if pos is None else pos
        blk[r, :K] = operand(kind, rng, (E, K)) if beta else NAN
        return dict(E=E, J=J, K=K, F=F, ldf=ldf, fcomplex=cplx, W=W, pos=pos, beta=beta, C=C, ldc=ldc)

    @staticmethod
    def _rows(E, pos):
        return np.arange(E) if pos is None else np.asarray(pos, dtype=np.int64)

    def ref(self, E, J, K, F, ldf, fcomplex, W, pos, beta, C, ldc, mut=None, dt=C128, parts=False):
        rows = (len(C) - LEAD - TRAIL) // ldc
        Fm = np.asarray(F).reshape(E, ldf)[:, :J]
        if mut == "real_as_complex" and not fcomplex:          # the float64 buffer read in pairs, as far as it goes
            flat = np.concatenate([np.asarray(F), np.full(len(F), np.nan)])
            idx = (np.arange(E)[:, None] * ldf + np.arange(J)[None, :])
            Fm = flat[2 * idx] + 1j * flat[2 * idx + 1]
        Fm = Fm.astype(dt)
        Wm = np.asarray(W).astype(dt)
        if mut == "W_transposed" and J == K:
            Wm = Wm.T
        if mut == "W_conj":
            Wm = np.conj(Wm)
        if mut == "first_row_doubled":
            Wm = Wm.copy(); Wm[0] = 2 * Wm[0]
        r = np.arange(E) if (pos is None or mut == "pos_ignored") else self._rows(E, pos)
        old = np.asarray(C)[LEAD: LEAD + rows * ldc].reshape(rows, ldc)
        val = Fm @ Wm.T
        if beta and mut != "beta_ignored":
            val = val + old[r, :K].astype(dt)
        if parts:
            return val
        res = np.array(C, copy=True)
        blk = res[LEAD: LEAD + rows * ldc].reshape(rows, ldc)
        n_ = E - 1 if mut == "skip_last_entry" else E
        blk[r[:n_], :K] = val[:n_]
        if mut == "pad_write":
            res[LEAD + int(r[E - 1]) * ldc + K] = 0.0                   # behind the last entry's row: padding, the next row or a trailing sentinel
        if mut == "perturb":
            i = LEAD + int(r[E // 2]) * ldc + K // 2
            res[i] = complex(np.nextafter(res[i].real, np.inf), res[i].imag)
        return res

    def check(self, impl, c):
        a = c.args
        E, K, ldc = a["E"], a["K"], a["ldc"]
        C0 = np.array(a["C"], copy=True)
        F0, W0 = np.array(a["F"], copy=True), np.array(a["W"], copy=True)
        got = np.asarray(impl(**a))
        assert got.shape == C0.shape, (self.name, c)
        assert np.array_equal(a["F"], F0, equal_nan=True) and np.array_equal(a["W"], W0), "an input was modified"
        rows = (len(C0) - LEAD - TRAIL) // ldc
        r = self._rows(E, a["pos"])
        mask = np.zeros(C0.shape, dtype=bool)
        m2 = mask[LEAD: LEAD + rows * ldc].reshape(rows, ldc)
        m2[r, :K] = True
        assert_exact(self.name + " (sentinels, padding and rows outside the map)", c, got[~mask], C0[~mask])
        val = got[LEAD: LEAD + rows * ldc].reshape(rows, ldc)[r, :K]
        want, bound = self.reference_and_bound(a, exact=c.kind == "exact")
        if c.kind == "exact":
            assert_exact(self.name, c, val, want)
        else:
            assert_bounded(self.name, c, val, want, bound)

    def reference_and_bound(self, a, exact=False):
        """the E x K results (np.clongdouble, or complex128 for an exact case after the magnitudes are checked) and the bound of the
        module docstring on |computed - exact|"""
        E, J, K, ldf, ldc, beta = a["E"], a["J"], a["K"], a["ldf"], a["ldc"], a["beta"]
        S = np.abs(np.asarray(a["F"]).reshape(E, ldf)[:, :J]) @ np.abs(np.asarray(a["W"])).T
        if beta:
            rows = (len(a["C"]) - LEAD - TRAIL) // ldc
            S = S + np.abs(np.asarray(a["C"])[LEAD: LEAD + rows * ldc].reshape(rows, ldc)[self._rows(E, a["pos"]), :K])
        bound = cbound(J + (1 if beta else 0), S)
        if exact:
            assert_below_2_53(2 * S)
            return self.ref(parts=True, **a), bound
        return self.ref(parts=True, dt=CLD, **a), bound


INTERP = InterpCoeffs()


def oversize_case(J, K):
    """a call outside 1 <= J, K <= 64: buffers as for any case, nothing may be written"""
    return InterpCoeffs._build(65, J, K, True, 0, "none", True, "exact")


# ================================================================================================================================
# dense restatement of src/types_cheb_pep.jl
def ref_cheb_nodes(a, b, k):
    """:6-9"""
    return (a + b) / 2 + (b - a) * np.cos((2 * np.arange(1, k + 1) - 1) * np.pi / (2 * k)) / 2


def ref_cheb_T(a, b, x, i):
    """:24-30, the cosine formula, for real x inside [a, b]"""
    return np.cos(i * np.arccos(np.clip(2 * (np.asarray(x, dtype=float) - a) / (b - a) - 1, -1.0, 1.0)))


def ref_cheb_coefficients(Mfun, k, a, b):
    """:94-114: the k dense coefficient matrices of the interpolant of lam -> Mfun(lam) (a dense matrix) in the Chebyshev nodes"""
    xk = ref_cheb_nodes(a, b, k)
    Fk = [np.asarray(Mfun(x)) for x in xk]
    Tmat = np.array([ref_cheb_T(a, b, xk, i) * 2 / k for i in range(k)])
    Tmat[0] *= 0.5
    return [sum(Fk[j] * Tmat[i, j] for j in range(k)) for i in range(k)]


def ref_cheb_eval(Bv, a, b, lam):
    """sum_i T_i(x(lam)) B_i by numpy.polynomial's Clenshaw evaluation, for real or complex lam"""
    x = 2 * (lam - a) / (b - a) - 1
    return sum(ch.chebval(x, np.eye(len(Bv))[i]) * np.asarray(B) for i, B in enumerate(Bv))


# ================================================================================================================================
# tolerances for values of Chebyshev polynomials computed by a three-term recurrence
def abs_poly_deriv(j, m, ax):
    """the m-th derivative at ax >= 0 of the polynomial whose monomial coefficients are the absolute values of T_j's: an upper
    bound on the sum of the absolute values of the terms of T_j^(m)(x), |x| = ax, however the terms are grouped"""
    c = np.abs(ch.cheb2poly(np.eye(j + 1)[j]))
    return float(pl.polyval(ax, pl.polyder(c, m))) if m <= j else 0.0


def cheb_tol(j, m, ax, chain, inner=1):
    """Tolerance on |computed - numpy| for the m-th (scaled) derivative.  The recurrence T_{i+1} = 2 x T_i - T_{i-1} on coefficient
    vectors (or matrices with inner products of `inner` terms) does at most 3 + inner roundings per step and entry, j steps, and every
    intermediate is bounded by the sum of absolute terms above; numpy's Clenshaw evaluation of the reference is a recurrence of the
    same length on the same terms.  So both are within (3 + inner) (j + 1) eps of the exact value times that sum: twice that."""
    return 2 * (3 + inner) * (j + 1) * EPS * abs_poly_deriv(j, m, ax) * abs(chain) ** m
