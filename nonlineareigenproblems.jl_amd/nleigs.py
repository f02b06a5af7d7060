"""NLEIGS (fully rational Krylov) on the device backend -- keyword surface of src/method_nleigs.jl:60-81.

Supported: SPMF-type NEPs (PEP, SPMF_NEP, PEP+SPMF SumNEP, DEP), dynamic and static variants, return_details
(NleigsSolutionDetails), divided differences by matrix functions (isfunm=true) or by differencing (isfunm=false),
leja in {0,1,2}, reusefact in {0,1,2}, non-SPMF NEP types through matrix-valued divided differences (`Mder_NEP`: the D_j become the
terms of an SPMF in the rational Newton basis), and the low-rank compression of PEP + LowRankFactorizedNEP problems
(rk_nep.jl:128-152; method_nleigs.jl:206-211,406-414,424-430,464-471,480,510: the blocks of the Krylov vectors beyond the
polynomial degree p hold r = sum rank(C_i) rows instead of n -- gun: 84 instead of 9956).

Device realisation of `backslash` (method_nleigs.jl:399-518).  The reference runs O(N) stacked SpMVs per step
(`sum(reshape(BBCC*z_block,n,:) .* transpose(sgdd[:,ii+1]),dims=2)`, :462).  The block recurrence for z does not
depend on z[1:n], so here
   Bw          one pass            (nep_rk_bw)
   z blocks    one pass, sequential over the N blocks inside each thread   (nep_block_recur)
   z0          ONE K1 call with k = N columns:  sum_j A_j (Z_blocks * sgdd[j,2:N+1]^T)   (nep_mlincomb)
   w0          K5 with the cached factorisation of the shift (LinSolverCache), scaled by -1/beta_1
   w blocks    one pass            (nep_block_recur)
With low-rank structure the same steps run over p blocks of n rows and N-p+1 blocks of r rows; the three seams
(Bw_p, z_p, w_p) apply UU^H and the tail of z0 applies [L_1 ... L_q] through the rectangular CSR operator (nep_csr_mv),
the weighted block sum in between is one nep_rowdot.
Every continuation solve is followed by K6 DGKS on the (N+1) n-row basis with per-column active row counts, and -- every
check_error_every steps -- by host `eig(K,H)`, one K7 GEMM for the Ritz block and K2 for all residuals.

Layout of the module: `_interpolation` and `_divided_differences` are the host set-up (no device access); `_State` holds what
the stages of one call share and freezes the linearisation (`grow`); `_step_coefficients` are the host tables of one step, read
by the two continuation solves `backslash` and `backslash_lowrank`; `_Pencil` owns (K, H) and the rows of the asynchronous
Gram-Schmidt that have not been read yet; `_check_due` / `check_convergence` are the Ritz check; `_nleigs` keeps the sequence.
"""
import warnings
from typing import NamedTuple

import numpy as np
import scipy.linalg as sla
import scipy.sparse as sp
import torch

from . import dense, rk_helper as rk
from ._lib import lib, check, hptr, c_vp
from .errmeasure import ResidualErrmeasure, estimate_errors
from .iar import _OrthPassMiss
from .linsolvers import DefaultLinSolverCreator, LinSolverCache
from .nep import CDT, to_dev, to_host, stream_ptr, require_pure_spmf, AbstractSPMF, SPMFDevice

EPS = np.finfo(float).eps
_DISTINCT_NODES = ("All interpolation nodes must be distinct when no matrix functions are used for computing "
                   "the generalized divided differences.")
_NONFINITE_DD = "The generalized divided differences must be finite."
_NOT_CONVERGED = "NLEIGS: Linearization not converged after %d iterations"


def _c128(x):
    return np.ascontiguousarray(x, dtype=np.complex128)


class NleigsSolutionDetails:
    """src/method_nleigs.jl:538-561: Ritz values / residuals per iteration, nodes, poles, scaling, divided-difference
    norms and the iteration at which the linearisation converged"""

    def __init__(self, Lam, Res, sigma, xi, beta, nrmD, kconv):
        self.Lam, self.Res, self.sigma, self.xi, self.beta, self.nrmD, self.kconv = Lam, Res, sigma, xi, beta, nrmD, kconv


def nleigs(nep, *args, **kw):
    """src/method_nleigs.jl (see _nleigs).  The host side of a call is a few hundred small dense operations (divided differences
    of matrix functions: 102 x 102 solves, the pencil's generalised eigenproblem, Leja-Bagby points): with a threaded BLAS each of
    them pays the wake-up of the pool -- 6 ms per 102 x 102 `solve` instead of 0.3 (gun R1: 23 of 86 ms) -- so BLAS runs on one
    thread for the duration of the call, as in iar's loop."""
    import nep_amd_hostlu as _nep_hostlu
    ctl = _nep_hostlu.blas_controller()

    def run():
        miss = False
        held = []                      # the run's LinSolverCache: closed on EVERY way out of it (its factors and prefetch pool are device memory)
        try:
            return _nleigs(nep, *args, _cache_holder=held, **kw)
        except _OrthPassMiss:          # "twice is enough" failed for a step of the asynchronous Gram-Schmidt: exact DGKS through the synchronous calls
            miss = True                # (the re-run starts AFTER this block: a live exception keeps the aborted run's frame -- basis, H, the
        finally:                       # cached factorisations -- alive, which would double the peak device memory of the fallback)
            for c_ in held:
                c_.close()
        assert miss
        nleigs.orth_misses += 1
        return _nleigs(nep, *args, _sync_orth=True, **kw)
    if ctl is None:
        return run()
    with ctl.limit(limits=1, user_api="blas"):
        return run()


nleigs.orth_misses = 0


# ---- host set-up: no device access --------------------------------------------------------------------------------------------
def _interpolation(Sigma, Xi, nodes, leja, static, maxit, maxdgr, p, isfunm):
    """interpolation nodes, poles, scaling (method_nleigs.jl:121-146): gamma, nodes, sigma, xi, beta"""
    if leja == 0:
        if len(nodes) == 0:
            raise ValueError("Interpolation nodes must be provided via 'nodes' when no Leja-Bagby points ('leja' == 0) are used.")
        gamma, _ = rk.discretizepolygon(Sigma)
        max_count = (maxit + maxdgr + 2) if static else max(maxit, maxdgr) + 2
        sigma = np.tile(nodes, int(np.ceil(max_count / len(nodes))))
        _, xi, beta = rk.lejabagby(sigma[:maxdgr + 2], Xi, gamma, maxdgr + 2, True, p)
    elif leja == 1:
        if len(nodes) == 0:
            gamma, nodes = rk.discretizepolygon(Sigma, True)
        else:
            gamma, _ = rk.discretizepolygon(Sigma)
        nodes = np.tile(nodes, int(np.ceil((maxit + 1) / len(nodes))))
        sigma, xi, beta = rk.lejabagby(gamma, Xi, gamma, maxdgr + 2, False, p)
    else:
        gamma, _ = rk.discretizepolygon(Sigma)
        max_count = (maxit + maxdgr + 2) if static else max(maxit, maxdgr) + 2
        sigma, xi, beta = rk.lejabagby(gamma, Xi, gamma, max_count, False, p)
    sigma = np.array(sigma, dtype=complex); xi = np.array(xi, dtype=float); beta = np.array(beta, dtype=float)
    xi[maxdgr + 1] = np.nan
    if not isfunm and len(np.unique(sigma)) != len(sigma):                          # method_nleigs.jl:142-145
        raise ValueError(_DISTINCT_NODES)
    return gamma, nodes, sigma, xi, beta


def _divided_differences(nep, newton_basis, sigma, xi, beta, maxdgr, mt, isfunm):
    """generalised divided differences on the first maxdgr+2 nodes (method_nleigs.jl:147-160): sgdd (mt x (maxdgr+2)), the
    matrices Dall of the Newton basis (None for an SPMF: its terms are the operator), their norms nrmD_all (None for an SPMF: the
    norm of step k is read off column k of sgdd) and nrmD = [norm of D_0]"""
    rng_ = slice(0, maxdgr + 2)
    if newton_basis:
        if len(np.unique(sigma[rng_])) != len(sigma[rng_]):
            raise ValueError(_DISTINCT_NODES)
        Dall = rk.ratnewtoncoeffs(lambda lam_: sp.csr_matrix(nep.compute_Mder(lam_), dtype=np.complex128), sigma[rng_], xi[rng_], beta[rng_])
        nrmD_all = [float(np.sqrt(abs(Dj.multiply(Dj.conj()).sum()))) for Dj in Dall]        # Frobenius norms (:152,225)
        sgdd = np.eye(mt, dtype=np.complex128)
        nrmD = [nrmD_all[0]]
    else:
        Dall = nrmD_all = None
        sgdd = rk.scgendivdiffs(sigma[rng_], xi[rng_], beta[rng_], nep.get_fv(), isfunm)   # mt x (maxdgr+2)
        nrmD = [float(np.max(abs(sgdd[:, 0])))]
    if not np.isfinite(nrmD[0]):
        raise ValueError(_NONFINITE_DD)
    return sgdd, Dall, nrmD_all, nrmD


class _State:
    """what the stages of one call share: the structure (n, p, r, LR, mt), the settings the freeze and the solves read (static,
    leja, reusefact, maxit, maxdgr, tollin, nodes), the linearisation (sgdd, nrmD_all, sigma, xi, beta, nrmD; N blocks, kn active
    rows, expand, kconv, kmax) and, after `alloc`, the device side (kdev = the operator of the z0 sum, cache, V with rows of ldv
    entries, Bw, zb, tmp, ylr, Wlr).  `grow` is the only place that changes the linearisation after the set-up."""

    def __init__(self, n, p, LR, mt, static, leja, reusefact, maxit, maxdgr, tollin, nodes, sigma, xi, beta, sgdd, nrmD_all, nrmD):
        self.n, self.p, self.LR, self.mt = n, p, LR, mt
        self.r = LR.r if LR is not None else n
        self.static, self.leja, self.reusefact, self.maxit, self.maxdgr, self.tollin = static, leja, reusefact, maxit, maxdgr, tollin
        self.nodes, self.sigma, self.xi, self.beta, self.sgdd, self.nrmD_all, self.nrmD = nodes, sigma, xi, beta, sgdd, nrmD_all, nrmD
        self.expand = True
        self.kconv = np.iinfo(np.int64).max // 2
        self.kn = n; self.N = 0
        # static variant (method_nleigs.jl:101-102,176,250-257): the linearisation is built first (no Krylov steps), then
        # maxit steps run on vectors of the frozen length (N+1) n; the start vector is zero-padded, which the zero-initialised V
        # provides for free.  At most maxdgr+1 blocks.
        self.kmax = maxit + maxdgr if static else maxit
        self.ldv = self.off(min(self.kmax, maxdgr + 1) + 2) if static else self.off(self.kmax + 2)

    def blk(self, j):
        """rows of block j (method_nleigs.jl:206-211)"""
        return self.n if (self.LR is None or j < self.p) else self.r

    def off(self, j):
        """first row of block j"""
        return j * self.n if (self.LR is None or j <= self.p) else self.p * self.n + (j - self.p) * self.r

    def alloc(self, kdev, cache):
        """device state: V ((maxit+2) x ldv, one Krylov vector per row), work vectors of ldv entries"""
        self.kdev, self.cache = kdev, cache
        self.V = torch.zeros((self.maxit + 2, self.ldv), dtype=CDT, device="cuda")
        self.Bw = torch.empty(self.ldv, dtype=CDT, device="cuda")
        self.zb = torch.empty(self.ldv, dtype=CDT, device="cuda")
        self.tmp = torch.empty(self.n, dtype=CDT, device="cuda")
        self.ylr = self.Wlr = None
        if self.LR is not None:
            self.ylr = torch.empty(self.r, dtype=CDT, device="cuda")
            self.Wlr = to_dev(self.sgdd[self.p + 1 + self.LR.iL, :])          # (maxdgr+2, r): column ii holds dd[iL] of method_nleigs.jl:464

    def grow(self, k):
        """step k of the expansion phase (method_nleigs.jl:204-262): one more block, the norm of its divided difference and --
        when the last five norms are below tollin, or at degree maxdgr -- the freeze of the linearisation: kconv, expand, the
        truncated xi / beta / nrmD, kmax and kn of the static variant, the cyclic nodes behind sigma[k] (leja = 1), N"""
        self.kn += self.blk(k)
        self.N += 1
        nrmD = self.nrmD
        nrmD.append(self.nrmD_all[k] if self.nrmD_all is not None else float(np.max(abs(self.sgdd[:, k]))))
        if not np.isfinite(nrmD[k]):
            raise ValueError(_NONFINITE_DD)
        if not (self.n > 1 and k >= 5 and k < self.kconv):
            return
        if sum(nrmD[k - 4:k + 1]) < 5 * self.tollin:
            self.kconv = k - 1
            self.xi = self.xi[:k]; self.beta = self.beta[:k]; self.nrmD = nrmD[:k]
            if self.static:
                self.kmax = self.maxit + self.kconv
                self.kn -= self.blk(k)
        elif k == self.maxdgr + 1:
            self.kconv = k
            warnings.warn(_NOT_CONVERGED % self.maxdgr)
        else:
            return
        self.expand = False
        if self.leja == 1:
            if len(self.sigma) < self.kmax + 1:
                self.sigma = np.concatenate([self.sigma, np.zeros(self.kmax + 1 - len(self.sigma), dtype=complex)])
            self.sigma[k:self.kmax + 1] = self.nodes[:self.kmax - k + 1]
        self.N -= 1


# ---- continuation solves ------------------------------------------------------------------------------------------------------
def _step_coefficients(shift, sigma, xi, beta, N):
    """host tables of one continuation solve with N blocks: cB_i = beta_i/xi_{i-1} (Bw), a_i = 1/nu_i, b_i = mu_i/nu_i with
    b_1 = 0 (z blocks: z_1 = Bw_1/nu_1 ; z_i = Bw_i/nu_i + (mu_i/nu_i) z_{i-1}) and bw_i = mu_{i-1}/nu_i (w blocks:
    w_i = (mu_i/nu_i) w_{i-1} + Bw_i/nu_i); nu_i = beta_i (1 - shift/xi_{i-1}), mu_i = shift - sigma_i.  The tables feed
    device kernels: the order of operations of every expression is part of the result."""
    with np.errstate(all="ignore"):
        cB = _c128(beta[1:N + 1] / xi[:N])                                    # beta[ii+1]/xi[ii]
        nu = beta[1:N + 1] * (1 - shift / xi[:N])
        a = _c128(1.0 / nu)
        b = np.zeros(N, dtype=np.complex128)
        if N > 1:
            b[1:] = (shift - sigma[1:N]) / nu[1:]
        mu = shift - sigma[:N]
        bw = _c128(mu / nu)
    return cB, a, b, bw


def _add_to_cache(s, k):
    """whether the factorisation of step k's shift is kept (method_nleigs.jl:474): after the freeze with reusefact = 1, always
    with reusefact = 2"""
    return ((not s.expand or k > s.kconv) and s.reusefact == 1) or s.reusefact == 2


def backslash(s, k, l):
    """w = continuation solve for column l-1 of V; result in V[l][:kn]"""
    n, N, Bw, zb = s.n, s.N, s.Bw, s.zb
    shift = s.sigma[k]
    wc = s.V[l - 1]; w = s.V[l]
    st = stream_ptr()
    cB, a, b, bw = _step_coefficients(shift, s.sigma, s.xi, s.beta, N)
    with np.errstate(all="ignore"):
        check(lib.nep_rk_bw(n, N, c_vp(wc.data_ptr()), hptr(cB), c_vp(Bw.data_ptr()), st))
        dense.copy(Bw, zb, (N + 1) * n)
        check(lib.nep_block_recur(n, N, hptr(a), hptr(b), c_vp(zb.data_ptr()), c_vp(zb.data_ptr()), st))
        # z0 = -sum_j A_j (Zblocks sgdd[j, 1:N+1]^T)   (Bw[0:n] = 0 without low-rank structure)
        Cm = np.asfortranarray(s.sgdd[:, 1:N + 1].T)                             # N x mt
        s.kdev.mlincomb(Cm, zb.data_ptr() + 16 * n, s.tmp, k=N, ldv=n)
        s.cache.solve_dev(shift, s.tmp, _add_to_cache(s, k), out=w[:n], scale=-1.0 / s.beta[0])
        check(lib.nep_block_recur(n, N, hptr(a), hptr(bw), c_vp(Bw.data_ptr()), c_vp(w.data_ptr()), st))
    return w


def backslash_lowrank(s, k, l):
    """the same solve over p blocks of n rows and N-p+1 blocks of r rows (low-rank branches of method_nleigs.jl:399-518);
    needs N >= p-1, which p <= 2 guarantees"""
    n, r, p, N, LR, Bw, zb, tmp, sgdd, off = s.n, s.r, s.p, s.N, s.LR, s.Bw, s.zb, s.tmp, s.sgdd, s.off
    shift = s.sigma[k]
    wc = s.V[l - 1]; w = s.V[l]
    st = stream_ptr()
    at = lambda T, j: T.data_ptr() + 16 * off(j)
    cB, a, b, bw = _step_coefficients(shift, s.sigma, s.xi, s.beta, N)
    with np.errstate(all="ignore"):
        nh = min(N, p - 1)                 # n-row blocks 1..p-1 follow the plain recurrences
        nr = N - p                         # r-row blocks p+1..N
        # ---- Bw (:417-436); its first block (:407-415) goes straight into the K1 call below
        if nh > 0:
            check(lib.nep_rk_bw(n, nh, c_vp(wc.data_ptr()), hptr(_c128(cB[:nh])), c_vp(Bw.data_ptr()), st))
        if nr > 0:
            check(lib.nep_rk_bw(r, nr, c_vp(at(wc, p)), hptr(_c128(cB[p:])), c_vp(at(Bw, p)), st))
        if nr >= 0:                        # seam: Bw_p = UU^H wc_{p-1} + beta_p/xi_{p-1} wc_p
            LR.UUH.mv(1.0, at(wc, p - 1), cB[p - 1], at(wc, p), at(Bw, p))
        # ---- z blocks (:438-491); block 0 of zb carries wc_{p-1} for the K1 call
        check(lib.nep_dev_copy(c_vp(zb.data_ptr()), c_vp(at(wc, p - 1)), 16 * n, st))
        check(lib.nep_dev_copy(c_vp(at(zb, 1)), c_vp(at(Bw, 1)), 16 * (off(N + 1) - n), st))
        if nh > 0:
            check(lib.nep_block_recur(n, nh, hptr(_c128(a[:nh])), hptr(_c128(b[:nh])), c_vp(zb.data_ptr()), c_vp(zb.data_ptr()), st))
        if nr >= 0:                        # seam: z_p = Bw_p/nu_p + mu_p/nu_p UU^H z_{p-1}   (mu_1/nu_1 := 0)
            LR.UUH.mv(b[p - 1], at(zb, p - 1), a[p - 1], at(zb, p), at(zb, p))
        if nr > 0:
            check(lib.nep_block_recur(r, nr, hptr(_c128(a[p:])), hptr(_c128(b[p:])), c_vp(at(zb, p)), c_vp(at(zb, p)), st))
        # ---- -z0 = D_p wc_{p-1}/beta_p + sum_{j<p} D_j z_j + [L_1..L_q] (sum_{j>p} dd_j o z_j)   (:407-415,455-471)
        Cm = np.zeros((p, s.mt), dtype=np.complex128, order="F")
        Cm[0, :] = sgdd[:, p] / s.beta[p]
        for j in range(1, p):
            Cm[j, :] = sgdd[:, j]
        if p >= 2 and N >= p:
            # (shift - sigma_{p-1})/beta_p D_p z_{p-1}: the elimination of block p-1 of the first block row leaves this
            # term; the reference omits it (its low-rank tests all have p = 1, where z_0 = 0) -- see oracle/nleigs.py
            Cm[p - 1, :] += b[p - 1] * sgdd[:, p]
        s.kdev.mlincomb(Cm, zb.data_ptr(), tmp, k=p, ldv=n)
        if nr > 0:
            check(lib.nep_rowdot(r, nr, c_vp(at(zb, p + 1)), r, c_vp(s.Wlr.data_ptr() + 16 * r * (p + 1)), r, c_vp(s.ylr.data_ptr()), st))
            LR.Lall.mv(1.0, s.ylr, 1.0, tmp, tmp)
        s.cache.solve_dev(shift, tmp, _add_to_cache(s, k), out=w[:n], scale=-1.0 / s.beta[0])
        # ---- w blocks (:496-515)
        if nh > 0:
            check(lib.nep_block_recur(n, nh, hptr(_c128(a[:nh])), hptr(_c128(bw[:nh])), c_vp(Bw.data_ptr()), c_vp(w.data_ptr()), st))
        if nr >= 0:                        # seam: w_p = mu_p/nu_p UU^H w_{p-1} + Bw_p/nu_p
            LR.UUH.mv(bw[p - 1], at(w, p - 1), a[p - 1], at(Bw, p), at(w, p))
        if nr > 0:
            check(lib.nep_block_recur(r, nr, hptr(_c128(a[p:])), hptr(_c128(bw[p:])), c_vp(at(Bw, p)), c_vp(at(w, p)), st))
    return w


# ---- the pencil (K, H) --------------------------------------------------------------------------------------------------------
class _Pencil:
    """H, K of the rational Krylov relation and the per-column active row counts.

    Asynchronous Gram-Schmidt (default): the rational Krylov recurrence itself never reads H -- the continuation vector is the last
    basis vector (method_nleigs.jl:287-288) and shifts, poles and block sizes are host data -- so the orthogonalisation of a step
    is enqueued with the DGKS decision on the device (nep_orth_dev: h, beta and the flags stay in row l - 1 of Hdev) and the rows
    are fetched in ONE copy when the pencil (K, H) is needed: at a convergence check and at the end.  The step-synchronous
    nep_orth (h and beta read back in every step: the host waited for the device and the device for the host, 100 times per call)
    remains as the fallback when a step still wanted a third pass; it writes its columns through `record` directly."""

    def __init__(self, s, ncol, async_orth, device="cuda"):
        self.s = s                                         # sigma is read at record time: the freeze may replace it
        self.H = np.zeros((ncol, ncol - 1), dtype=complex); self.K = np.zeros((ncol, ncol - 1), dtype=complex)
        self.active = np.zeros(ncol, dtype=np.int64)
        self.Hdev = self.active_d = None
        if async_orth:
            self.Hdev = torch.zeros((ncol, ncol + 2), dtype=CDT, device=device)
            self.active_d = torch.zeros(ncol, dtype=torch.int64, device=device)
        self.pending = []                                  # (l, k) of the steps whose row of Hdev has not been read yet

    def record(self, l, k, h, hb):
        """column l-1 of the pencil from the coefficients h[0:l], hb of step k: K = H sigma_k + e_l e_l^T"""
        H, K = self.H, self.K
        sigma_k = self.s.sigma[k]
        H[:l, l - 1] = h; H[l, l - 1] = hb
        K[:l, l - 1] = H[:l, l - 1] * sigma_k
        K[l - 1, l - 1] += 1.0
        K[l, l - 1] = H[l, l - 1] * sigma_k

    def enqueue(self, l, k, kn):
        """orthogonalise V[l] against V[0:l] on the device; its row of Hdev is read at the next flush"""
        s, pending, active_d = self.s, self.pending, self.active_d
        if not pending or pending[-1][0] != l - 1 or l == 1:
            active_d[:l + 1].copy_(torch.from_numpy(self.active[:l + 1]))        # (first step, or after a gap: the whole prefix)
        else:
            active_d[l:l + 1].fill_(int(kn))
        dense.orthogonalize_and_normalize_dev(s.V, s.V[l], l, self.Hdev[l - 1], rows=kn, ldv=s.ldv, active_dev=active_d, method=dense.DGKS)
        pending.append((l, k))

    def flush(self):
        """read the rows of Hdev of the pending steps and record their columns; a step that wanted a third Gram-Schmidt pass
        raises _OrthPassMiss"""
        pending = self.pending
        if not pending:
            return
        l0 = pending[0][0]; l1 = pending[-1][0]
        rows_ = self.Hdev[l0 - 1:l1].cpu().numpy()          # one device-to-host copy (synchronises)
        for (l_, k_) in pending:
            row = rows_[l_ - l0]
            flags = int(row[l_ + 1].imag)
            if flags & 2:
                raise ArithmeticError("orthogonalisation breakdown in nleigs step %d" % k_)
            if flags & 1:
                raise _OrthPassMiss(k_)
            self.record(l_, k_, row[:l_], row[l_].real)
        pending.clear()


# ---- Ritz check ---------------------------------------------------------------------------------------------------------------
class _Check(NamedTuple):
    """result of one convergence check: Ritz values lam = lambda_[ilam] (inside Sigma; with return_details every finite one),
    their Ritz block QT (row-major, device; None without candidates), residuals, the convergence mask and the two counts the
    stop test compares"""
    lam: np.ndarray
    QT: object
    ilam: np.ndarray
    res: np.ndarray
    conv: np.ndarray
    nblamin: int
    nbconv: int


_NO_CHECK = _Check(np.zeros(0, dtype=complex), None, np.zeros(0, dtype=int), np.zeros(0), np.zeros(0, dtype=bool), 0, 0)


def _check_due(k, N, kconv, expand, static, minit, check_error_every, kmax, return_details):
    """is a convergence check due at step k (method_nleigs.jl:300-306): every check_error_every steps from minit steps after the
    freeze on and at the last step; with return_details at every step that made a Krylov vector"""
    if return_details:
        return not static or not expand
    return ((not expand and k >= N + minit and (k - (N + minit)) % check_error_every == 0) or
            (k >= kconv + minit and (k - (kconv + minit)) % check_error_every == 0) or k == kmax)


def check_convergence(s, pen, l, Sigma, tol, errmeasure, all_=False, Lam=None, Res=None):
    """Ritz pairs of the l x l pencil and their residuals (method_nleigs.jl:307-340); all_ also fills column l-1 of the
    histories Lam, Res"""
    pen.flush()
    H, n = pen.H, s.n
    lambda_, S = sla.eig(pen.K[:l, :l], H[:l, :l])
    if not all_:
        lamin = rk.in_Sigma(lambda_, Sigma, tol)
        ilam = np.nonzero(lamin)[0]
        lam = lambda_[ilam]
    else:                                                   # method_nleigs.jl:309-313: every finite Ritz value
        ilam = np.nonzero(np.isfinite(lambda_))[0]
        lam = lambda_[ilam]
        lamin = rk.in_Sigma(lam, Sigma, tol)
    S = S.copy()
    for i in ilam:
        S[:, i] /= np.linalg.norm(H[:l + 1, :l] @ S[:, i])
    if len(ilam):
        QT = dense.gemm_ts(s.V, H[:l + 1, :l] @ S[:, ilam], rowmajor=True, k=l + 1, rows=n, ldz=s.ldv)
        res = estimate_errors(errmeasure, lam, QT)
    else:
        QT = None; res = np.zeros(0)
    conv = np.abs(res) < tol
    if all_:                                                # :328-336 history of all Ritz values / residuals
        resall = np.full(l, np.nan)
        resall[ilam] = res
        si = sorted(range(l), key=lambda i: (abs(lambda_[i]), np.angle(lambda_[i])))
        Res[:l, l - 1] = resall[si]
        Lam[:l, l - 1] = lambda_[si]
        conv = conv & lamin
    return _Check(lam, QT, ilam, res, conv, int(np.sum(lamin)), int(np.sum(conv)))


# ---- the driver ---------------------------------------------------------------------------------------------------------------
def _structure(nep, maxdgr):
    """newton_basis, p, mt, LR: degree of the polynomial part, number of terms and low-rank structure of the operator"""
    if not isinstance(nep, AbstractSPMF):
        # non-SPMF NEP type (method_nleigs.jl:149-153: `D = ratnewtoncoeffs(lam -> compute_Mder(nep, lam), ...)`): the
        # matrix-valued divided differences D_0..D_{maxdgr+1} ARE an SPMF in the rational Newton basis, M ~ sum_j b_j(lam) D_j,
        # whose scalar divided differences are the identity -- so the stacked-CSR kernels run unchanged on the D_j
        if not hasattr(nep, "compute_Mder"):
            raise TypeError("nleigs needs an SPMF-type NEP or one that provides compute_Mder")
        if maxdgr + 2 > 128:
            raise ValueError("nleigs on a non-SPMF NEP keeps maxdgr+2 divided-difference matrices on the device: maxdgr <= 126")
        return True, 0, maxdgr + 2, None
    require_pure_spmf(nep, "nleigs")
    p, _ = rk.rk_structure(nep)
    LR = rk.low_rank_structure(nep)
    if LR is not None and not 1 <= p <= 2:
        # the reference reads block p-1 of a two-block vector in its first step (method_nleigs.jl:408-414)
        raise ValueError("nleigs with low-rank structure needs a polynomial part of degree 1 or 2")
    return False, p, len(nep.get_Av()), LR


def _nleigs(nep, Sigma=(-1.0 - 1j, -1 + 1j, 1 + 1j, 1 - 1j), Xi=(np.inf,), logger=0, maxdgr=100, minit=20, maxit=200,
            linsolvercreator=None, tol=1e-10, tollin=None, v=None, errmeasure=None, isfunm=True, static=False, leja=1,
            nodes=(), reusefact=1, blksize=20, return_details=False, check_error_every=5, info=None, _sync_orth=False,
            _cache_holder=None):
    if tollin is None:
        tollin = max(tol / 10, 100 * EPS)
    if linsolvercreator is None:
        linsolvercreator = DefaultLinSolverCreator()
    if errmeasure is None:
        errmeasure = ResidualErrmeasure(nep)
    Sigma = np.asarray(Sigma, dtype=complex); Xi = np.asarray(Xi, dtype=float)
    nodes = np.asarray(nodes, dtype=complex)
    n = nep.size(1)
    newton_basis, p, mt, LR = _structure(nep, maxdgr)
    if n == 1:
        maxdgr = maxit + 1
    if v is None:
        v = np.random.randn(n) + 0j
    cache = LinSolverCache(nep, linsolvercreator)
    if _cache_holder is not None:
        _cache_holder.append(cache)

    gamma, nodes, sigma, xi, beta = _interpolation(Sigma, Xi, nodes, leja, static, maxit, maxdgr, p, isfunm)
    sgdd, Dall, nrmD_all, nrmD = _divided_differences(nep, newton_basis, sigma, xi, beta, maxdgr, mt, isfunm)
    s = _State(n, p, LR, mt, static, leja, reusefact, maxit, maxdgr, tollin, nodes, sigma, xi, beta, sgdd, nrmD_all, nrmD)
    s.alloc(SPMFDevice(Dall) if newton_basis else nep.dev, cache)                           # the operator of the z0 sum
    ncol = maxit + 2
    pen = _Pencil(s, ncol, not _sync_orth)
    Lam = np.zeros((ncol - 1, ncol - 1), dtype=complex); Res = np.zeros((ncol - 1, ncol - 1))
    solve = backslash_lowrank if LR is not None else backslash

    v0 = _c128(v) / np.linalg.norm(v)
    # host factorisations of the next shifts run ahead on a worker thread; with reusefact = 2 (every factorisation is kept) and a
    # device-factorisation plan for the pattern, ALL distinct shifts are factorised on the GPU in one batched pass instead
    cache.prefetch(sigma[:3], keep_all=list(dict.fromkeys(complex(s_) for s_ in sigma)) if reusefact == 2 else None)
    x0 = cache.solve(sigma[0], to_dev(v0)[0], reusefact == 2)
    nx0 = dense.nrm2(x0)
    dense.copy(x0, s.V[0], n); dense.scal(s.V[0], 1.0 / nx0, n)
    pen.active[0] = n

    chk = _NO_CHECK
    l = 0
    k = 1
    while k <= s.kmax:
        if s.expand:
            s.grow(k)
        l = k - s.N if static else k
        if not static or not s.expand:
            cache.prefetch(s.sigma[k:k + 3])
            w = solve(s, k, l)
            pen.active[l] = s.kn
            if _sync_orth:
                h, hb, _ = dense.orthogonalize_and_normalize(s.V, w, l, rows=s.kn, ldv=s.ldv, active_rows=pen.active, method=dense.DGKS)
                pen.record(l, k, h, hb)
            else:
                pen.enqueue(l, k, s.kn)
        if _check_due(k, s.N, s.kconv, s.expand, static, minit, check_error_every, s.kmax, return_details):
            chk = check_convergence(s, pen, l, Sigma, tol, errmeasure, return_details, Lam, Res)
        if ((not s.expand and k >= s.N + minit) or k >= s.kconv + minit) and chk.nblamin == chk.nbconv:
            break
        k += 1
    pen.flush()
    lam, conv, res = chk.lam, chk.conv, chk.res
    cache.close()
    if info is not None:
        info.update(kconv=s.kconv, N=s.N, k=min(k, s.kmax), nfact=len(cache.solvers), nrmD=s.nrmD, nblamin=chk.nblamin, vrows=s.ldv,
                    lowrank_r=(s.r if LR is not None else 0))
    if chk.QT is None or not np.any(conv):
        X = np.zeros((n, 0), dtype=complex)
    else:
        X = to_host(dense.rowmajor_to_cols(chk.QT, np.nonzero(conv)[0]))
        X = X / np.linalg.norm(X, axis=0)[None, :]
    if return_details:                                          # method_nleigs.jl:363-374
        kk = min(k, s.kmax)
        xi, beta, nrmD = s.xi, s.beta, s.nrmD
        if s.expand:
            xi = xi[:kk]; beta = beta[:kk]; nrmD = nrmD[:kk]
            warnings.warn(_NOT_CONVERGED % maxdgr)
        return lam[conv], X, res[conv], NleigsSolutionDetails(Lam[:l, :l], Res[:l, :l], s.sigma[:kk], xi, beta, nrmD, s.kconv)
    return lam[conv], X, res[conv]
