"""Reference, error bound and case list for nep_broyden_sweep (csrc/broyden.hip), and a dense NumPy restatement of broyden /
broyden_T written from the reference (src/method_broyden.jl), not from the product.

Style and helpers of tests/cork_checkers.py: `SWEEP.check(impl, case)` runs `impl` on flat complex128 buffers and compares with a
plain reference; test_gpu_broyden.py passes an adapter that calls the library, test_host_broyden.py passes the float64 NumPy
implementation and its mutants.

The kernel makes one pass over T (n x n, column-major, leading dimension ldt):
    T[i, j] += u0[i] a0[j]                     (only with u0 / a0)
    y[i]     = sum_j T_new[i, j] x[j]          (only with x)
    g[j]     = sum_i conj(w[i]) T_new[i, j]    (only with w: the row w^H T_new, unconjugated)

Error bounds of the rounded cases (cbound of primitive_checkers.py; S is the expression with every operand replaced by its absolute
value).  An updated entry is one complex product added to T[i, j]: |dT| <= cbound(1, |T| + |u0| |a0|).  y[i] is a sum of n complex
products whose left factors carry that error, which is one more term of the same size: |dy| <= cbound(n + 1, (|T| + |u0| |a0|^T) |x|),
and likewise |dg| <= cbound(n + 1, |w|^T (|T| + |u0| |a0|^T)).  Without an update T must come back bit for bit and the same bounds hold
with u0 = 0.  Nothing is fitted to a device result.  The largest error / bound ratio seen is recorded in primitive_checkers.RATIOS.
"""
from functools import partial
from itertools import product

import numpy as np
import scipy.linalg as sla

from primitive_checkers import (C128, CLD, NAN, SENT, RATIOS, Case, Prim, _seed, cbound, operand, colmajor_buf, drop_tail,   # noqa: F401
                                assert_exact, assert_bounded, assert_below_2_53)
from cork_checkers import RefAAANep, ref_dep                                                                                 # noqa: F401

EPS = np.finfo(float).eps

# ================================================================================================================================
# nep_broyden_sweep
BS_N = [1, 2, 63, 64, 65, 128, 193, 257, 511, 1025]
BS_PAD = [0, 3]
BS_WORK = [(upd, hx, hw) for upd, hx, hw in product((True, False), repeat=3) if upd or hx or hw]
LEAD, TRAIL = 3, 2
TILE = 64                                           # the quantum the tile-dropping mutants forget (a wave, a column tile)


class BroydenSweep(Prim):
    """impl(n, T, ldt, lead, u0, a0, x, y, w, g) -> (T, y, g) after the call (y / g None where they were None).

    T: flat buffer of `lead` sentinels followed by the n x n column-major block (ldt) whose padding rows hold NaN or sentinels.
    u0, a0, x, w: n entries or None.  y, g: LEAD sentinels, n entries prefilled with NaN, TRAIL sentinels (None without x / w).
    The checker verifies that the inputs, the lead and padding of T and the sentinels of y and g kept their values, and that T
    comes back unchanged when there is no update."""
    name = "nep_broyden_sweep"
    mutants = ("stale_products", "a0_conj", "w_not_conj", "skip_last_row_tile", "skip_last_col_tile", "pad_write", "perturb")

    def shapes(self):
        t = 0
        for n, pad, (upd, hx, hw) in product(BS_N, BS_PAD, BS_WORK):
            for kind in ("exact", "rounded"):
                yield n, pad, upd, hx, hw, kind, (LEAD if t % 2 == 0 else 0), (NAN if t % 3 == 0 else SENT)
            t += 1

    def cases(self):
        for n, pad, upd, hx, hw, kind, lead, fill in self.shapes():
            cid = "ld%d_%s%s%s_lead%d_%s" % (n + pad, "u" if upd else "-", "x" if hx else "-", "w" if hw else "-", lead,
                                            "nan" if fill is NAN else "sent")
            yield Case("n%d" % n, cid, kind, partial(self._build, n, pad, upd, hx, hw, kind, lead, fill))

    @staticmethod
    def _build(n, pad, upd, hx, hw, kind, lead, fill):
        rng = np.random.default_rng(_seed("broydensweep%d.%d%d%d%d%s%d" % (n, pad, upd, hx, hw, kind, lead)))
        ldt = n + pad
        T = colmajor_buf(operand(kind, rng, (n, n)), ldt, fill=fill, lead=lead)
        T[:lead] = SENT
        vec = lambda on: operand(kind, rng, n) if on else None
        u0, a0, x, w = vec(upd), vec(upd), vec(hx), vec(hw)

        def out(on):
            if not on:
                return None
            b = np.full(LEAD + n + TRAIL, SENT, dtype=C128)
            b[LEAD: LEAD + n] = NAN
            return b
        return dict(n=n, T=T, ldt=ldt, lead=lead, u0=u0, a0=a0, x=x, y=out(hx), w=w, g=out(hw))

    @staticmethod
    def _block(T, n, ldt, lead):
        """the n x n entries of the flat buffer as a writable view (columns of the result are columns of T)"""
        return np.lib.stride_tricks.as_strided(T[lead:], shape=(n, n), strides=(T.itemsize, ldt * T.itemsize))

    def values(self, n, T, ldt, lead, u0, a0, x, y, w, g, mut=None, dt=C128):
        """(T_new, y, g) as n x n / n arrays of type dt (None where not requested)"""
        Tm = np.array(self._block(T, n, ldt, lead), dtype=dt)
        rows = drop_tail(n, TILE) if mut == "skip_last_row_tile" else n
        cols = drop_tail(n, TILE) if mut == "skip_last_col_tile" else n
        Tn = Tm
        if u0 is not None:
            a = np.conj(a0) if mut == "a0_conj" else a0
            Tn = Tm.copy()
            Tn[:rows, :cols] += np.outer(u0.astype(dt), a.astype(dt))[:rows, :cols]
        Tp = Tm if mut == "stale_products" else Tn
        yv = gv = None
        if x is not None:
            yv = np.full(n, NAN, dtype=dt)
            yv[:rows] = Tp[:rows, :cols] @ x.astype(dt)[:cols]
        if w is not None:
            ww = w.astype(dt)
            gv = np.full(n, NAN, dtype=dt)
            gv[:cols] = (ww if mut == "w_not_conj" else np.conj(ww))[:rows] @ Tp[:rows, :cols]
        return Tn, yv, gv

    def ref(self, n, T, ldt, lead, u0, a0, x, y, w, g, mut=None):
        Tn, yv, gv = self.values(n, T, ldt, lead, u0, a0, x, y, w, g, mut=mut)
        Tb = np.array(T, copy=True)
        self._block(Tb, n, ldt, lead)[:, :] = Tn
        yb = gb = None
        if y is not None:
            yb = np.array(y, copy=True); yb[LEAD: LEAD + n] = yv
        if g is not None:
            gb = np.array(g, copy=True); gb[LEAD: LEAD + n] = gv
        if mut == "pad_write":
            if lead + ldt * (n - 1) + n < len(Tb):
                Tb[lead + ldt * (n - 1) + n] = 0.0                      # the entry behind the last one of T
            elif yb is not None:
                yb[LEAD + n] = 0.0
            elif gb is not None:
                gb[LEAD + n] = 0.0
            else:
                Tb[lead - 1 if lead else 0] = 0.0
        if mut == "perturb":                                            # one ulp in one real part of the last result there is
            tgt = gb if gb is not None else yb if yb is not None else Tb
            i = (LEAD if tgt is not Tb else lead) + n // 2
            tgt[i] = complex(np.nextafter(tgt[i].real, np.inf), tgt[i].imag)
        return Tb, yb, gb

    def check(self, impl, c):
        a = c.args
        n, ldt, lead = a["n"], a["ldt"], a["lead"]
        keep = {k: np.array(a[k], copy=True) for k in ("T", "u0", "a0", "x", "w", "y", "g") if a[k] is not None}
        Tg, yg, gg = impl(**a)
        for k in ("T", "u0", "a0", "x", "w", "y", "g"):
            assert a[k] is None or np.array_equal(a[k], keep[k], equal_nan=True), "the caller's %s was modified" % k
        Tg = np.asarray(Tg)
        assert Tg.shape == keep["T"].shape, (self.name, c)
        mask = np.zeros(Tg.shape, dtype=bool)
        self._block(mask, n, ldt, lead)[:, :] = True
        assert_exact(self.name + " (lead and padding of T)", c, Tg[~mask], keep["T"][~mask])
        for nm, got in (("y", yg), ("g", gg)):
            assert (got is None) == (a[nm] is None), (self.name, c, nm)
            if got is not None:
                got = np.asarray(got)
                assert got.shape == keep[nm].shape, (self.name, c, nm)
                assert_exact(self.name + " (sentinels of %s)" % nm, c, np.concatenate([got[:LEAD], got[LEAD + n:]]),
                             np.concatenate([keep[nm][:LEAD], keep[nm][LEAD + n:]]))
        Tval = np.array(self._block(Tg, n, ldt, lead))
        if a["u0"] is None:
            assert_exact(self.name + " (T without an update)", c, Tval, self._block(keep["T"], n, ldt, lead))
        want, bound = self.reference_and_bound(a, exact=c.kind == "exact")
        for nm, got, wv, bv in (("T", Tval, want[0], bound[0]), ("y", None if yg is None else np.asarray(yg)[LEAD: LEAD + n], want[1], bound[1]),
                                ("g", None if gg is None else np.asarray(gg)[LEAD: LEAD + n], want[2], bound[2])):
            if got is None or (nm == "T" and a["u0"] is None):
                continue
            if c.kind == "exact":
                assert_exact("%s (%s)" % (self.name, nm), c, got, wv)
            else:
                assert_bounded(self.name, c, got, wv, bv)

    def reference_and_bound(self, a, exact=False):
        """((T_new, y, g), (bound_T, bound_y, bound_g)): np.clongdouble references, or complex128 for an exact case after the
        magnitudes are checked, and the bounds of the module docstring"""
        n = a["n"]
        Ta = np.abs(np.array(self._block(a["T"], n, a["ldt"], a["lead"])))
        if a["u0"] is not None:
            Ta = Ta + np.outer(np.abs(a["u0"]), np.abs(a["a0"]))
        Sy = None if a["x"] is None else Ta @ np.abs(a["x"])
        Sg = None if a["w"] is None else np.abs(a["w"]) @ Ta
        bound = (cbound(1, Ta), None if Sy is None else cbound(n + 1, Sy), None if Sg is None else cbound(n + 1, Sg))
        if exact:
            for S in (Ta, Sy, Sg):
                if S is not None:
                    assert_below_2_53(2 * S)
            return self.values(**a), bound
        return self.values(dt=CLD, **a), bound


SWEEP = BroydenSweep()


# ================================================================================================================================
# dense restatement of src/method_broyden.jl
class RefNep(RefAAANep):
    """M(lam) = sum_i f_i(lam) A_i with dense matrices, with what broyden needs: compute_Mlincomb (K1) and compute_MM"""

    def Mlincomb(self, lam, v):
        return self.Mder(lam) @ v

    def MM(self, S, V):
        raise NotImplementedError


class RefDep(RefNep):
    def __init__(self, A0, A1, tau=1.0):
        dn = lambda A: np.asarray(A.toarray() if hasattr(A, "toarray") else A, dtype=complex)
        A0, A1 = dn(A0), dn(A1)
        n = A0.shape[0]
        super().__init__([np.eye(n), A0, A1], [lambda l: -l, lambda l: np.ones_like(l), lambda l: np.exp(-tau * l)])
        self.tau = tau

    def MM(self, S, V):
        """sum_i A_i V f_i(S) = -V S + A0 V + A1 V expm(-tau S)"""
        S = np.atleast_2d(np.asarray(S, dtype=complex))
        return -V @ S + self.Av[1] @ V + self.Av[2] @ V @ sla.expm(-self.tau * S)


def ref_dep_of(nep):
    """the dense restatement of a product DEP (its matrices are inputs, not results)"""
    A = nep.A if hasattr(nep, "A") else nep.get_Av()[1:]
    return RefDep(A[0], A[1], tau=1.0)


def default_errmeasure(lam, v, r):
    return np.linalg.norm(r) / np.linalg.norm(v)                          # :13-15


def ref_broyden_T(nep, v, u, lam, CH, T1, W1, S, X, maxit=100, check_error_every=10, tol=1e-12, threshold=0.4,
                  errmeasure=default_errmeasure, form="four_pass", drift=None):
    """broyden_T, :21-155.  form = "four_pass": as the reference writes it (T*rk, T*ztilde, dv'*T and the update are four passes
    over T).  form = "pending": the update of iteration j is applied at the start of iteration j + 1, just before T*ztilde and
    dv'*T are taken, and T*rk follows from  T_new rkp = gamma Tztilde + (1 - gamma) Trk + Tztilde (aH rkp)  (rkp = gamma ztilde +
    (1 - gamma) rk).  drift (a list, pending form only): at every error check the pending update is applied and
    ||T rk - recurrence|| / (||T||_F ||rk||) is appended.  Returns (lam, v, u, T, W, j, errhist)."""
    v = np.array(v, dtype=complex); u = np.array(u, dtype=complex); lam = complex(lam)
    n = len(v); p = S.shape[0]
    II = np.eye(p)
    vv_of = lambda lam_, v_, u_: v_ + (X @ np.linalg.solve(lam_ * II - S, u_) if p else 0.0)
    rk = nep.Mlincomb(lam, vv_of(lam, v, u))
    T = np.array(T1, dtype=complex); W = np.array(W1, dtype=complex)
    errhist = np.full(maxit, np.nan)
    Z = T @ W
    pending = form == "pending"
    Trk = T @ rk
    pend = None
    for j in range(1, maxit + 1):
        if not pending:
            Trk = T @ rk                                                  # :69
        dul = -np.linalg.solve(CH @ Z, CH @ Trk)                          # :71
        du, dl = dul[:p], dul[-1]
        dv = -Z @ dul - Trk
        gam = 1.0
        tt = np.sqrt(abs(dl) ** 2 + np.linalg.norm(dv) ** 2)
        if tt > threshold:
            gam = threshold / tt
        v = v + gam * dv; u = u + gam * du; lam = lam + gam * dl
        rkp = nep.Mlincomb(lam, vv_of(lam, v, u))
        ztilde = (rkp - (1 - gam) * rk) / gam                             # :100
        if pend is not None:
            T = T + np.outer(pend[0], pend[1]); pend = None
        Tz = T @ ztilde                                                   # :101
        nrm2 = np.linalg.norm(dv) ** 2 + np.linalg.norm(du) ** 2 + abs(dl) ** 2
        bH = np.concatenate([du.conj(), [np.conj(dl)]]) / nrm2            # :104
        beta = nrm2 + np.vdot(dv, Tz)                                     # :106
        aH = -(dv.conj() @ T) / beta                                      # :107
        Z = Z + np.outer(Tz, aH @ W + (1 + aH @ ztilde) * bH)             # :110
        W = W + np.outer(ztilde, bH)                                      # :113
        if pending:
            pend = (Tz, aH)
            Trk = gam * Tz + (1 - gam) * Trk + Tz * (aH @ rkp)
        else:
            T = T + np.outer(Tz, aH)                                      # :117
        rk = rkp
        if j % check_error_every == 0:
            if pending and drift is not None:
                T = T + np.outer(pend[0], pend[1]); pend = None
                drift.append(np.linalg.norm(T @ rk - Trk) / (np.linalg.norm(T) * np.linalg.norm(rk)))
            errhist[j - 1] = errmeasure(lam, vv_of(lam, v, u), rk)
            if errhist[j - 1] < tol:
                if pend is not None:
                    T = T + np.outer(pend[0], pend[1])
                return lam, v, u, T, W, j, errhist[:j]
    if pend is not None:
        T = T + np.outer(pend[0], pend[1])
    return lam, v, u, T, W, maxit, errhist


def ref_broyden(nep, approxnep="eye", sigma=0.0, pmax=3, c=None, maxit=1000, addconj=False, check_error_every=10, threshold=0.2,
                tol=1e-12, errmeasure=default_errmeasure, add_nans=False, recompute_U=False, form="four_pass", drift=None,
                iters=None, eigmethod="eig"):
    """broyden, :235-439, with eigmethod = :eig or :invpow (eigs_invpow, :445-455: 4000 solves from a vector of ones).  approxnep: "eye", an n x n array or a RefNep.  Returns (S, X, T1, all_errhist,
    all_iterhist); iters (a list) receives the inner iteration count of every level."""
    n = nep.n
    pmax = min(pmax, n)
    sigma = complex(sigma)
    c = np.ones(n, dtype=complex) if c is None else np.asarray(c, dtype=complex)
    if isinstance(approxnep, str):
        assert approxnep == "eye"
        M1 = np.eye(n, dtype=complex)
    elif isinstance(approxnep, np.ndarray):
        M1 = approxnep.astype(complex)
    else:
        M1 = approxnep.Mder(sigma)
    T1 = np.linalg.inv(M1)
    X = np.zeros((n, 0), dtype=complex); S = np.zeros((0, 0), dtype=complex)
    all_errhist, all_iterhist = [], []
    UU = np.eye(n, pmax + 1, dtype=complex)
    k, p_U1 = 1, 0
    while k <= pmax:
        U1 = UU[:, :k - 1]
        for i in range(0 if recompute_U else p_U1, k - 1):                # :300-305
            ei = np.zeros(k - 1, dtype=complex); ei[i] = 1.0
            U1[:, i] = nep.Mlincomb(sigma, X @ np.linalg.solve(sigma * np.eye(k - 1) - S, ei))
        p_U1 = k - 1
        MM = np.block([[M1, U1], [X.conj().T, np.zeros((k - 1, k - 1))]])
        if eigmethod == "eig":
            d, V = np.linalg.eig(MM)
            x = V[:, np.argmin(np.abs(d))]
        else:
            lu = sla.lu_factor(MM)
            x = np.ones(n + k - 1, dtype=complex)
            for _ in range(4000):
                x = sla.lu_solve(lu, x)
                x = x / np.linalg.norm(x)
        v0, u0 = x[:n], x[n:]
        h = X.conj().T @ v0
        v0 = v0 - X @ h
        u0 = u0 + (sigma * np.eye(k - 1) - S) @ h
        CH = np.vstack([X.conj().T, c.conj()[None, :]])
        sc = np.vdot(c, v0)
        u0 = u0 / sc; v0 = v0 / sc
        dd = np.sqrt(EPS)
        f1 = (nep.Mlincomb(sigma + dd, v0) - nep.Mlincomb(sigma - dd, v0)) / (2 * dd)
        if k > 1:
            f1 = f1 - U1 @ np.linalg.solve(sigma * np.eye(k - 1) - S, u0)
        W1 = np.column_stack([U1, f1])
        lm, vm, um, _, _, it, errhist = ref_broyden_T(nep, v0, u0, sigma, CH, T1, W1, S, X, maxit=maxit,
                                                      check_error_every=check_error_every, tol=tol, threshold=threshold,
                                                      errmeasure=errmeasure, form=form, drift=drift)
        if iters is not None:
            iters.append(it)
        iterhist = np.arange(1, len(errhist) + 1) + (all_iterhist[-1] if len(all_iterhist) else 0)
        if add_nans and len(all_iterhist) > 1:
            all_errhist.append(np.nan); all_iterhist.append(np.nan)
        all_errhist += list(errhist); all_iterhist += list(iterhist)
        nv = np.linalg.norm(vm)
        um = um / nv; vm = vm / nv
        X = np.column_stack([X, vm])
        S = np.block([[S, um[:, None]], [np.zeros((1, k - 1)), np.array([[lm]])]])
        if abs(lm.imag) > tol * 10 and addconj:                           # :405-433
            v1 = np.conj(vm + X[:, :k - 1] @ np.linalg.solve(lm * np.eye(k - 1) - S[:k - 1, :k - 1], um))
            l1 = np.conj(lm)
            h = X.conj().T @ v1
            v1t = v1 - X @ h
            beta = np.linalg.norm(v1t)
            X = np.column_stack([X, v1t / beta])
            k += 1
            S1 = np.zeros((k, k), dtype=complex)
            S1[:k - 1, :k - 1] = S
            S1[k - 1, k - 1] = l1
            R = np.eye(k, dtype=complex)
            R[:k - 1, -1] = h; R[k - 1, k - 1] = beta
            S = np.linalg.solve(R.T, (R @ S1).T).T
        k += 1
    return S, X, T1, np.array(all_errhist), np.array(all_iterhist)


def pair_residual(nep, S, X):
    """||M(S, X)||_2 of an invariant pair (test/broyden.jl)"""
    return np.linalg.norm(nep.MM(S, X), 2)
