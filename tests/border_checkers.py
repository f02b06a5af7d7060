"""Reference, error bound and case list for nep_defl_border (csrc/deflate_border.hip), and two dense NumPy restatements written
from the reference (not from the product): the p + 1-solve Schur algorithm of lin_solve(::DeflatedNEPLinSolver)
(src/LinSolvers.jl:221-252) and jd_effenberger (src/method_jd.jl:216-438) on the RefSPMF / RefDeflated classes of
tests/deflation_checkers.py.

Style and helpers of tests/deflation_checkers.py: `DeflBorder.check(impl, case)` runs `impl` on flat complex128 buffers and compares
with a plain reference; test_gpu_jd_effenberger.py passes an adapter that calls the library, test_host_border.py passes the float64
NumPy implementation and its mutants.

The kernel forms, from y (n0), X (n0 x p), b2 (p, or zeros), T (p x p) and a real scale,
    c = b2 - X^H y,        out[0:n0] = scale (y + X c),        out[n0:n0+p] = scale (T c).

Error bound of the rounded cases.  c[q] is b2[q] minus a sum of n0 complex products (the subtraction is among cbound's six extra
roundings):
    |dc[q]| <= cbound(n0, |b2[q]| + sum_r |X[r, q]| |y[r]|).
Given the computed c, y[r] + sum_l X[r, l] c[l] is a sum of p + 1 complex terms, and the error of c reaches it through |X[r, :]|:
    |dv1[r]| <= cbound(p + 1, |y[r]| + |X[r, :]| . |c|) + |X[r, :]| . |dc|.
Likewise sum_l T[q, l] c[l] is a sum of p complex products:
    |dv2[q]| <= cbound(p, |T[q, :]| . |c|) + |T[q, :]| . |dc|.
The product with the real scale rounds each component once more (relative error u per component, so u |z| for the complex z):
    |d(scale z)| <= |scale| |dz| + u |scale| |z|.
Nothing is fitted to a device result.  The largest error / bound ratio seen is recorded in primitive_checkers.RATIOS.
"""
from functools import partial
from itertools import product

import numpy as np

from primitive_checkers import (C128, CLD, NAN, SENT, U, RATIOS, Case, Prim, _seed, cbound, operand, colmajor_buf, cm_view,        # noqa: F401
                                assert_exact, assert_bounded, assert_below_2_53)
from deflation_checkers import RefFun, RefSPMF, RefDeflated, ref_deflate, ref_get_deflated_eigpairs       # noqa: F401

# ================================================================================================================================
# nep_defl_border
DB_N0 = [1, 2, 63, 64, 65, 255, 257, 1025, 4099]
DB_P = [1, 2, 3, 8, 32]
DB_GRID_ROWS = 2048 * 256 + 77           # more rows than the capped grid of the streaming passes has threads: the grid-stride loop
LEAD, TRAIL = 3, 3


class DeflBorder(Prim):
    """impl(n0, p, X, ldx, Y, b2, T, scale, out) -> the out buffer after the call.

    X: n0 x p (ldx) column-major flat buffer whose padding rows hold NaN.  b2: p entries or None (zeros).  T: p x p column-major.
    out: LEAD sentinels, n0 + p entries, TRAIL sentinels.  Y is None for an in-place call: y then sits in the first n0 entries of
    the block of `out` (its p tail entries hold NaN); otherwise Y holds y and the whole block of `out` is prefilled with NaN.
    The checker verifies that everything but the n0 + p entries kept its value."""
    name = "nep_defl_border"
    mutants = ("c_sign", "no_conj", "t_transposed", "b2_ignored", "skip_row", "pad_write", "tail_unscaled", "perturb")

    def cases(self):
        shapes = []
        for t, (n0, p) in enumerate(product(DB_N0, DB_P)):         # every (n0, p) with rotating flags
            shapes.append((n0, p, "rounded" if t % 3 == 0 else "exact", 3 * (t & 1), bool((t >> 1) & 1), (t >> 2) & 1 == 0,
                           -1.0 if t % 5 in (1, 3) else 1.0))
        for t, p in enumerate(DB_P):                               # every p with b2, scale = -1, both kinds, in and out of place
            for kind in ("exact", "rounded"):
                shapes.append((257, p, kind, 3 * (t & 1), kind == "exact", True, -1.0))
                shapes.append((65, p, kind, 3 - 3 * (t & 1), kind != "exact", True, -1.0))
        for n0, p, kind, pad, inplace, has_b2, scale in shapes:
            yield Case("n%d" % n0, "p%d_pad%d_%s_%s_s%+d" % (p, pad, "inplace" if inplace else "outofplace", "b2" if has_b2 else "nob2", scale),
                       kind, partial(self._build, n0, p, kind, pad, inplace, has_b2, scale))
        yield Case("n%d" % DB_GRID_ROWS, "p2_pad0_inplace_b2_s-1", "exact", partial(self._build, DB_GRID_ROWS, 2, "exact", 0, True, True, -1.0))

    @staticmethod
    def _build(n0, p, kind, pad, inplace, has_b2, scale):
        rng = np.random.default_rng(_seed("deflborder%d.%d.%d%s%d%d" % (n0, p, pad, kind, inplace, has_b2)))
        X = operand(kind, rng, (n0, p)); y = operand(kind, rng, n0)
        b2 = operand(kind, rng, p) if has_b2 else None
        T = operand(kind, rng, (p, p))
        ldx = n0 + pad
        out = np.full(LEAD + n0 + p + TRAIL, NAN, dtype=C128)
        out[:LEAD] = SENT; out[LEAD + n0 + p:] = SENT
        if inplace:
            out[LEAD: LEAD + n0] = y
        return dict(n0=n0, p=p, X=colmajor_buf(X, ldx), ldx=ldx, Y=None if inplace else y, b2=b2,
                    T=np.ascontiguousarray(T.T).reshape(-1), scale=scale, out=out)

    @staticmethod
    def _operands(n0, p, X, ldx, Y, b2, T, out, dt):
        Xm = cm_view(X, 0, n0, p, ldx).astype(dt)
        y = (out[LEAD: LEAD + n0] if Y is None else Y).astype(dt)
        b = np.zeros(p, dtype=dt) if b2 is None else b2.astype(dt)
        return Xm, y, b, T.reshape(p, p).T.astype(dt)              # T[q, l]

    def ref(self, n0, p, X, ldx, Y, b2, T, scale, out, mut=None, dt=C128, parts=False):
        Xm, y, b, Tm = self._operands(n0, p, X, ldx, Y, b2, T, out, dt)
        if mut == "b2_ignored":
            b = np.zeros(p, dtype=dt)
        c = b - (Xm if mut == "no_conj" else np.conj(Xm)).T @ y
        if mut == "c_sign":
            c = -c
        v1 = y + Xm @ c
        v2 = (Tm.T if mut == "t_transposed" else Tm) @ c
        if parts:
            return v1, v2, c
        sc = dt(scale) if dt is CLD else scale
        res = np.array(out, copy=True)
        res[LEAD: LEAD + n0] = sc * v1
        res[LEAD + n0: LEAD + n0 + p] = v2 if mut == "tail_unscaled" else sc * v2
        if mut == "skip_row":
            res[LEAD + n0 // 2] = out[LEAD + n0 // 2]
        if mut == "pad_write":
            res[LEAD + n0 + p] = 0.0
        if mut == "perturb":                                       # one ulp in one real part
            i = LEAD + (n0 + p) // 2
            res[i] = complex(np.nextafter(res[i].real, np.inf), res[i].imag)
        return res

    def check(self, impl, c):
        a = c.args
        n0, p, scale = a["n0"], a["p"], a["scale"]
        out0 = np.array(a["out"], copy=True)
        got = np.asarray(impl(**a))
        assert got.shape == out0.shape, (self.name, c)
        blk = slice(LEAD, LEAD + n0 + p)
        assert_exact(self.name + " (sentinels around out)", c, np.concatenate([got[:LEAD], got[LEAD + n0 + p:]]),
                     np.concatenate([out0[:LEAD], out0[LEAD + n0 + p:]]))
        Xm, y, b, Tm = self._operands(n0, p, a["X"], a["ldx"], a["Y"], a["b2"], a["T"], a["out"], C128)
        aX, aT = np.abs(Xm), np.abs(Tm)
        Sc = np.abs(b) + aX.T @ np.abs(y)
        if c.kind == "exact":
            assert_below_2_53(2 * (np.abs(y) + aX @ Sc)); assert_below_2_53(2 * (aT @ Sc))
            v1, v2, _ = self.ref(parts=True, **a)
            assert_exact(self.name, c, got[blk], np.concatenate([scale * v1, scale * v2]))
        else:
            want, bound = self.reference_and_bound(a)
            assert_bounded(self.name, c, got[blk], want, bound)

    def reference_and_bound(self, a):
        """the n0 + p results in np.clongdouble and the bound of the module docstring on |computed - exact|"""
        n0, p, scale = a["n0"], a["p"], a["scale"]
        Xm, y, b, Tm = self._operands(n0, p, a["X"], a["ldx"], a["Y"], a["b2"], a["T"], a["out"], C128)
        aX, aT = np.abs(Xm), np.abs(Tm)
        Sc = np.abs(b) + aX.T @ np.abs(y)
        v1, v2, cw = self.ref(parts=True, dt=CLD, **a)
        ac = np.abs(cw).astype(np.float64)
        dc = cbound(n0, Sc)
        b1 = cbound(p + 1, np.abs(y) + aX @ ac) + aX @ dc
        b2_ = cbound(p, aT @ ac) + aT @ dc
        want = np.concatenate([v1, v2]) * CLD(scale)
        return want, abs(scale) * np.concatenate([b1, b2_]) + U * np.abs(want).astype(np.float64)


BORDER = DeflBorder()


# ================================================================================================================================
# lin_solve(::DeflatedNEPLinSolver), src/LinSolvers.jl:221-252, and the one-solve form, on a RefDeflated
def ref_border_solve_reference(dnep, lam, b, solve=np.linalg.solve):
    """p + 1 solves with the original matrix: b1tilde = M^-1 b1, Z = M^-1 U column by column, S = -X^H Z (formed explicitly),
    v2 = S \\ (b2 - X^H b1tilde), v1 = b1tilde - Z v2"""
    X, n0, p = dnep.V0, dnep.n0, dnep.p
    b = np.asarray(b, dtype=complex)
    b1, b2 = b[:n0], b[n0:]
    Uq = dnep._compute_Q(lam, 0)                                   # deflated_nep_compute_Q(deflated_nep, lam, 0)
    M = dnep.org.Mder(lam)
    b1t = solve(M, b1)
    Z = np.zeros((n0, p), dtype=complex)
    for i in range(p):
        Z[:, i] = solve(M, Uq[:, i])
    S = -X.conj().T @ Z
    v2 = np.linalg.solve(S, b2 - X.conj().T @ b1t)
    return np.concatenate([b1t - Z @ v2, v2])


def ref_border_solve_onesolve(dnep, lam, b, solve=np.linalg.solve):
    """one solve: y = M^-1 b1, c = b2 - X^H y, v1 = y + X c, v2 = -(lam I - S0) c (needs X^H X = I)"""
    X, n0, p = dnep.V0, dnep.n0, dnep.p
    b = np.asarray(b, dtype=complex)
    y = solve(dnep.org.Mder(lam), b[:n0])
    c = b[n0:] - X.conj().T @ y
    return np.concatenate([y + X @ c, -(lam * np.eye(p) - dnep.S0) @ c])


# ================================================================================================================================
# jd_effenberger, src/method_jd.jl:216-438, in dense arithmetic
def ref_monomial(i):
    import math

    def der(lam, j):
        return 0.0 if j > i else math.factorial(i) / math.factorial(i - j) * lam ** (i - j)
    return RefFun(der, lambda S: np.linalg.matrix_power(np.asarray(S, dtype=complex), i))


def ref_pep(Av):
    return RefSPMF(Av, [ref_monomial(i) for i in range(len(Av))])


def _ref_spmf_of(nep):
    return nep.spmf if isinstance(nep, RefDeflated) else nep


def _ref_newton_inner(pnep, lam, v0, tol=1e-13, maxit=80):
    """augnewton on the projected problem (method_newton.jl:274-347, c = v at the start, ResidualErrmeasure) as
    inner_solve(::NewtonInnerSolver) runs it (inner_solver.jl:258-296): without convergence the last iterate is kept"""
    lam = complex(lam); v = np.asarray(v0, dtype=complex).copy(); c = v.copy()
    v = v / np.vdot(c, v)
    for _ in range(maxit):
        if np.linalg.norm(pnep.Mlincomb(lam, v)) / np.linalg.norm(v) < tol:
            break
        try:
            t = np.linalg.solve(pnep.Mder(lam), pnep.Mlincomb(lam, v, [1.0], 1))
        except np.linalg.LinAlgError:
            break
        alpha = 1.0 / np.vdot(c, t)
        lam -= alpha; v = alpha * t
    return lam, v


def _ref_eig_sorter(lamv, V, N, target):
    NN = min(N, len(lamv))                                         # jd_eig_sorter, method_jd.jl:177-183
    cidx = np.argsort(np.abs(lamv - target), kind="stable")
    return lamv[cidx[NN - 1]], V[:, cidx[NN - 1]].copy()


def _ref_dgks(V, w):
    """orthogonalize_and_normalize!(V, w, h, DGKS()): classical Gram-Schmidt, repeated once when the norm drops below 1/sqrt(2)"""
    n0 = np.linalg.norm(w)
    w = w - V @ (V.conj().T @ w)
    if np.linalg.norm(w) < n0 / np.sqrt(2):
        w = w - V @ (V.conj().T @ w)
    return w / np.linalg.norm(w)


def _ref_jd_inner(target_nep, X, Lam, orgnep, maxit, nrof_its, conveig, solver, tol, target, neigs, u, lam):
    """jd_effenberger_inner!, :320-438"""
    eps = np.finfo(float).eps
    n, m = orgnep.n, Lam.shape[0]
    nn = n + m
    spmf = _ref_spmf_of(target_nep)
    u = np.asarray(u, dtype=complex) / np.linalg.norm(u)
    newton_step = np.random.rand(nn).astype(complex)
    size = maxit + 1 - nrof_its
    Vm = np.zeros((nn, size), dtype=complex); Wm = np.zeros((nn, size), dtype=complex)
    Vm[:, 0] = u
    w0 = target_nep.Mlincomb(lam, u)
    Wm[:, 0] = w0 / np.linalg.norm(w0)
    err = np.inf
    for loop_counter in range(nrof_its + 1, maxit + 1):
        k = loop_counter - nrof_its
        V, W = Vm[:, :k], Wm[:, :k]
        pnep = RefSPMF([W.conj().T @ A @ V for A in spmf.Av], spmf.fv)               # expand_projectmatrices!
        lamv = lam * np.ones(2, dtype=complex); sv = np.random.rand(k, 2).astype(complex)
        for j in range(2):                                                           # inner_solve(NewtonInnerSolver), :Vk
            lamv[j], sv[:, j] = _ref_newton_inner(pnep, lamv[j], sv[:, j])
        lam_temp, s = _ref_eig_sorter(lamv, sv, 1, target)
        s = s / np.linalg.norm(s)
        if np.isfinite(lam_temp) and np.all(np.isfinite(s)) and np.linalg.norm(pnep.Mlincomb(lam_temp, s)) < tol * 50:
            u = V @ s; lam = lam_temp
        else:
            u = u + newton_step; u = u / np.linalg.norm(u)
        rk = target_nep.Mlincomb(lam, u)
        err = np.linalg.norm(rk)
        if err < tol:
            lam2, s2 = _ref_eig_sorter(lamv, sv, 2, target)
            if abs(lam - lam2) / abs(lam) > np.sqrt(eps):
                u2 = np.concatenate([V @ (s2 / np.linalg.norm(s2)), [0.0]])
            else:
                lam2 = complex(np.random.rand()); u2 = np.random.rand(nn + 1).astype(complex)
            return lam, u, loop_counter, u2, lam2
        pk = target_nep.Mlincomb(lam, u, [1.0], 1)
        v = solver(target_nep, lam, pk)
        newton_step = v.copy()
        Vm[:, k] = _ref_dgks(V, v)
        Wm[:, k] = _ref_dgks(W, rk)
    D, Y = np.linalg.eig(Lam) if m > 0 else (np.zeros(0, dtype=complex), np.zeros((0, 0), dtype=complex))
    raise RuntimeError("ref_jd_effenberger: maxit=%d and only %d eigenvalues converged out of %d (found %r, err %.3g)"
                       % (maxit, conveig, neigs, np.concatenate([D, [lam]]), err))


def ref_jd_effenberger(nep, neigs, maxit, lam, v, tol, target=0.0, solver="onesolve"):
    """jd_effenberger, :216-295, on a RefSPMF with the Newton inner solver; the deflated solves by the one-solve form
    ("onesolve") or by the reference's p + 1-solve algorithm ("reference").  Random numbers from np.random (seed it first).
    Returns (eigenvalues, eigenvectors, iterations used)."""
    n = nep.n
    border = {"onesolve": ref_border_solve_onesolve, "reference": ref_border_solve_reference}[solver]
    plain_solver = lambda tn, l, b: np.linalg.solve(tn.Mder(l), b)
    defl_solver = lambda tn, l, b: border(tn, l, b)
    lam = complex(lam); u = np.asarray(v, dtype=complex) / np.linalg.norm(v)
    lam_init, u_init = lam, u
    conveig, its = 0, 0
    if np.linalg.norm(nep.Mlincomb(lam, u)) < tol:
        lam_init = complex(np.random.rand()); u_init = np.random.rand(n + 1).astype(complex)
    else:
        lam, u, its, u_init, lam_init = _ref_jd_inner(nep, np.zeros((n, 0), dtype=complex), np.zeros((0, 0), dtype=complex), nep,
                                                      maxit, its, conveig, plain_solver, tol, target, neigs, u_init, lam_init)
    conveig += 1
    dnep = ref_deflate(nep, lam, u, "SPMF")
    while True:
        if conveig == neigs:
            D, Vv = ref_get_deflated_eigpairs(dnep)
            return D, Vv, its
        lam, u, its, u_init, lam_init = _ref_jd_inner(dnep, dnep.V0, dnep.S0, nep, maxit, its, conveig, defl_solver, tol, target,
                                                      neigs, u_init, lam_init)
        conveig += 1
        dnep = ref_deflate(dnep, lam, u, "SPMF")
