"""Sparse LU factors on the device: `DeviceLU` (host SuperLU factors uploaded once, every solve the HIP kernel k_lu_solve of
csrc/trsv.hip) and `_DeviceRefactor`, the per-pattern plans of the device-side numeric factorisation (csrc/lufac.hip)."""
import atexit
import ctypes as C
import os
import threading
import time

import numpy as np
import scipy.sparse as sp
import torch

from . import _lib
from ._env import env_float, env_int, env_str
from ._hostlu_pool import _nep_hostlu
from ._lib import lib, check, hptr, c_vp, c_i64
from .nep import pure_spmf, stream_ptr


def host_factor(Ac, permc_spec=None, diag_pivot_thresh=None, symmetric_mode=None):
    """SuperLU factors of the csc matrix Ac, in this process (the dict of _nep_hostlu.factor)"""
    try:
        return _nep_hostlu.factor(Ac.data, Ac.indices, Ac.indptr, Ac.shape, permc_spec=permc_spec,
                                  diag_pivot_thresh=diag_pivot_thresh, symmetric_mode=symmetric_mode)
    except RuntimeError as e:  # "Factor is exactly singular"
        raise np.linalg.LinAlgError("SingularException: " + str(e))


def reused(lu_kw):
    """lu_kw of a factorisation that exists to be reused (iar/tiar: maxit solves): scheduled for 200 solves unless it says otherwise"""
    return dict(lu_kw, expected_solves=lu_kw.get("expected_solves", 200))


class _Pattern:
    """what _DeviceRefactor.key / maybe_start read of a csc matrix (no values kept)"""

    def __init__(self, indptr, indices, shape):
        self.indptr, self.indices, self.shape = indptr, indices, shape


class _DeviceRefactor:
    """Per sparsity pattern: the plan of the device-side numeric factorisation (csrc/lufac.hip).  The first matrix of a pattern
    is factorised on the host; when that factorisation used the symmetric strategy with diagonal pivots only (perm_r ==
    perm_c) and landed on the block schedule, a background thread enumerates the updates of the right-looking LU for that
    pivot sequence (0.3 s for the gun pattern, once per pattern and process).  Later matrices with the same pattern -- the next
    iar call, the next shift of nleigs -- are factorised on the GPU with the stored pivot sequence (static pivoting); pivot
    breakdown or element growth above `GROWTH` sends that matrix back to the host path."""
    plans = {}           # key -> dict(state="building"|"ready"|"off", handle, thread, strategy, fails)
    lock = threading.Lock()
    GROWTH = env_float("NEP_LU_DEV_GROWTH", 1e6)
    # factors whose solves are NOT followed by iterative refinement (contour_beyn's node solves; the reference pivots afresh at
    # every node): accepted only with element growth max|U| / max|A| and max|L| up to 1e3 -- the growth a threshold-pivoted
    # factorisation with diag_pivot_thresh = 1e-3 tolerates per step -- otherwise that node goes to the host
    GROWTH_UNREFINED = env_float("NEP_LU_DEV_GROWTH_UNREFINED", 1e3)
    MAX = 4

    @classmethod
    def enabled(cls):
        return env_str("NEP_LU_DEV", "1") != "0" and env_str("NEP_LU_SCHED") != "old"

    _digests = []          # (indptr array, indices array, digest) of the last patterns hashed: see key()

    @staticmethod
    def _fingerprint(ip, ix):
        return (ip[::max(1, ip.shape[0] // 256)].tobytes(), ix[::max(1, ix.shape[0] // 768)].tobytes(),
                int(ip[-1]) if ip.shape[0] else 0)

    @classmethod
    def key(cls, Ac, opts):
        import hashlib
        # the matrices of one SPMF NEP share the index arrays of its union pattern (compute_Mder builds them around the NEP's
        # aligned terms without a copy): a pattern whose two arrays ARE arrays hashed before -- same memory, same length, and
        # the remembered arrays are kept alive here, so the address cannot have been recycled -- is not hashed again (0.54 ms
        # per linear solver on the gun pattern)
        ip, ix = Ac.indptr, Ac.indices
        dig = None
        fp = None
        if isinstance(ip, np.ndarray) and isinstance(ix, np.ndarray):
            a_ip = ip.__array_interface__["data"][0]; a_ix = ix.__array_interface__["data"][0]
            # ... and whose CONTENTS still look the same: keeping the arrays alive rules out a recycled address, not an in-place
            # edit (A.sort_indices(), a rewritten A.indices of equal length).  A strided sample of both arrays (about 1 k entries,
            # a few microseconds) travels with the digest; an edit that leaves every sampled entry alone would have to be aimed
            fp = cls._fingerprint(ip, ix)
            for rp, rx, d, f in cls._digests:
                if (rp.__array_interface__["data"][0] == a_ip and rx.__array_interface__["data"][0] == a_ix and rp.shape == ip.shape
                        and rx.shape == ix.shape and rp.dtype == ip.dtype and rx.dtype == ix.dtype
                        and rp.strides == ip.strides and rx.strides == ix.strides and f == fp):
                    dig = d
                    break
        if dig is None:
            h = hashlib.blake2b(digest_size=16)
            # (index dtype normalised: the same pattern arrives as int32 from scipy and as int64 from the NEP's aligned terms)
            h.update(np.ascontiguousarray(ip, dtype=np.int64)); h.update(np.ascontiguousarray(ix, dtype=np.int64))
            dig = h.digest()
            if isinstance(ip, np.ndarray) and isinstance(ix, np.ndarray):
                with cls.lock:
                    cls._digests.append((ip, ix, dig, fp))
                    del cls._digests[:-8]
        knobs = tuple(env_str(k) for k in ("NEP_ML_BMAX", "NEP_ML_SPLIT", "NEP_ML_CHUNK"))   # they change the partition
        return (dig, Ac.shape, opts, knobs)

    @classmethod
    def lookup(cls, key):
        with cls.lock:
            p = cls.plans.get(key)
            return p if (p is not None and p["state"] == "ready") else None

    @classmethod
    def maybe_start(cls, key, lu, F, Ac):
        """called after a host factorisation: start the plan of this pattern if the factor qualifies"""
        if not cls.enabled() or not lu.block_schedule or F.get("fmt") != "csc":
            return
        if not F["strategy"].get("symmetric_mode") or not np.array_equal(F["perm_r"], F["perm_c"]):
            return
        if int(F["Lp"][-1]) + int(F["Up"][-1]) > env_int("NEP_LU_DEV_MAXNNZ", 4000000):
            return        # factors of this size mean far more products than a plan may hold (the library would refuse it anyway)
        with cls.lock:
            if key in cls.plans:
                return
            while len(cls.plans) >= cls.MAX:
                old = next(iter(cls.plans))
                po = cls.plans[old]
                if po["state"] == "building":
                    return
                cls.plans.pop(old)
                if po.get("handle"):
                    lib.nep_lu_refac_destroy(po["handle"])
            plan = dict(state="building", handle=None, strategy=dict(F["strategy"]), fails=0, uses=0)
            cls.plans[key] = plan
        arrs = [np.array(F[k], dtype=np.int32, copy=True) for k in ("Lp", "Li", "Up", "Ui", "perm_r", "perm_c")]
        Ap = np.array(Ac.indptr, dtype=np.int32, copy=True); Ai = np.array(Ac.indices, dtype=np.int32, copy=True)
        n = int(F["n"])

        def build():
            h = c_vp()
            rc = lib.nep_lu_refac_create(lu.h, n, *[hptr(a) for a in arrs], hptr(Ap), hptr(Ai), C.byref(h))   # GIL released
            with cls.lock:
                if rc == 0:
                    plan["handle"] = h; plan["state"] = "ready"
                else:
                    plan["state"] = "off"
            plan.pop("keep", None)
        if "NEP_LU_PLAN_THREADS" not in os.environ:
            # enumeration threads from the CPU budget of this rank (8 ranks on a 16-CPU quota must not start 48 threads); through a
            # setter: writing the environment from here would race with getenv calls of plan threads already running
            from ._affinity import cpu_budget
            check(lib.nep_lu_set_plan_threads(max(1, min(6, cpu_budget() - 1))))
        plan["keep"] = lu                  # the reference factor must outlive the build
        t = threading.Thread(target=build, name="nep-lu-refac-plan", daemon=True)
        plan["thread"] = t
        t.start()

    @staticmethod
    def _wrap(plan, h, n, normA, numeric, health, into=None):
        """counts the outcome of one device factorisation on its plan and wraps the handle (a new DeviceLU, or `into`); None
        where the stored pivot sequence was refused for that matrix"""
        if not h:
            plan["fails"] += 1
            return None
        plan["uses"] += 1
        lu = DeviceLU.__new__(DeviceLU) if into is None else into
        # growth: max |L| and the element growth max|U| / max|A|
        return lu._adopt(c_vp(h), n, normA, dict(plan["strategy"], numeric=numeric), float(max(health[1], health[2])))

    @classmethod
    def factor_batch(cls, plan, n, vals, expected_solves=1, growth=None):
        """vals: (B, nnz) values of B matrices of the plan's pattern.  Returns a list of DeviceLU (None where the stored pivot
        sequence was refused for that matrix -- the caller factorises those on the host)."""
        B = int(vals.shape[0])
        vals = np.ascontiguousarray(vals, dtype=np.complex128)
        health = np.zeros((B, 3))
        outs = (c_vp * B)()
        check(lib.nep_lu_set_expected_solves(int(expected_solves)))
        check(lib.nep_lu_factor_dev_batch(plan["handle"], B, hptr(vals), int(expected_solves),
                                          cls.GROWTH if growth is None else float(growth), hptr(health), None, outs,
                                          stream_ptr()))
        return [cls._wrap(plan, outs[b], n, float(np.linalg.norm(vals[b])), "device (stored pivot sequence, batched)", health[b])
                for b in range(B)]

    @classmethod
    def factor_batch_terms(cls, plan, n, D_dev, Cf, normA, expected_solves=1, growth=None):
        """the same for B matrices A_b = sum_t Cf[b, t] A_t whose term values sit on the device (D_dev: nnz x m_t, the union
        pattern of the plan): nothing of size B x nnz is formed on the host or uploaded.  normA: the B Frobenius norms."""
        Cf = np.ascontiguousarray(Cf, dtype=np.complex128)
        B, mt = Cf.shape
        assert D_dev.is_contiguous() and D_dev.shape[1] == mt
        health = np.zeros((B, 3))
        outs = (c_vp * B)()
        check(lib.nep_lu_set_expected_solves(int(expected_solves)))
        check(lib.nep_lu_factor_dev_batch_terms(plan["handle"], B, c_vp(D_dev.data_ptr()), mt, hptr(Cf), int(expected_solves),
                                                cls.GROWTH if growth is None else float(growth), hptr(health), outs, stream_ptr()))
        return [cls._wrap(plan, outs[b], n, float(normA[b]), "device (stored pivot sequence, batched)", health[b])
                for b in range(B)]

    @classmethod
    def wait(cls):
        """block until every plan under construction is finished (tests, benchmarks)"""
        for p in list(cls.plans.values()):
            t = p.get("thread")
            if t is not None:
                t.join()

    @classmethod
    def clear(cls):
        cls.wait()
        with cls.lock:
            for p in cls.plans.values():
                if p.get("handle"):
                    lib.nep_lu_refac_destroy(p["handle"])
            cls.plans.clear()


GROWTH_UNREFINED = _DeviceRefactor.GROWTH_UNREFINED      # (read once per process, with the class: the name other modules use)
atexit.register(_DeviceRefactor.wait)      # a plan thread inside the HIP runtime must not be cut off by interpreter shutdown


class DeviceLU:
    """nep_lu handle built from a host sparse LU of A (CSC/CSR/dense).

    Pivoting strategy mirrors what UMFPACK (the reference's `factorize`, LinSolvers.jl:116) selects
    automatically: for a structurally symmetric matrix with a zero-free diagonal the *symmetric strategy*
    (fill-reducing ordering of A+A', diagonal pivots preferred with tolerance 0.001) -> SuperLU with
    permc_spec=MMD_AT_PLUS_A, SymmetricMode, diag_pivot_thresh=0.001; otherwise the unsymmetric strategy
    (column ordering, threshold partial pivoting) -> COLAMD with SuperLU's default threshold.  Explicit
    arguments override the choice.  `factors` (the dict returned by _nep_hostlu.factor, e.g. from a HostLUPool
    worker) skips the host factorisation."""

    def __init__(self, A=None, permc_spec=None, diag_pivot_thresh=None, symmetric_mode=None, expected_solves=50,
                 factors=None, plan_pattern=None):
        """plan_pattern (with `factors`): the csc pattern these host factors belong to -- lets a factorisation that was
        computed elsewhere (contour_beyn's worker processes) seed the pattern's device-factorisation plan"""
        _lib.require_gpu()
        t0 = time.perf_counter()
        self.device_factorized = False
        opts = (permc_spec, diag_pivot_thresh, symmetric_mode)
        # ---- which route: the pattern's plan on the device, or host factors (given, or computed here) that may start the plan
        rkey = None; Ac = None
        if factors is not None and plan_pattern is not None and _DeviceRefactor.enabled():
            k0 = _DeviceRefactor.key(plan_pattern, opts)
            with _DeviceRefactor.lock:
                known = k0 in _DeviceRefactor.plans
            if not known:
                rkey = k0; Ac = plan_pattern
        if factors is None:
            Ac = sp.csc_matrix(A, dtype=np.complex128)
            if _DeviceRefactor.enabled():
                rkey = _DeviceRefactor.key(Ac, opts)
                plan = _DeviceRefactor.lookup(rkey)
                if plan is not None and self._factor_on_device(plan, Ac, expected_solves, t0):
                    return
            factors = host_factor(Ac, *opts)
        Fplan = self._upload(factors, expected_solves, rkey is not None)
        self.t_setup = time.perf_counter() - t0
        if rkey is not None:
            _DeviceRefactor.maybe_start(rkey, self, Fplan, Ac)

    def _upload(self, F, expected_solves, for_plan):
        """host factors -> nep_lu handle.  Returns what _DeviceRefactor.maybe_start reads of the factors (for_plan: with index
        arrays of its own where F sits in a shared-memory block, which is released here)"""
        shm_backed = "shm_name" in F
        if shm_backed:
            F = _nep_hostlu.attach_shm(F)
        n = int(F["n"])
        self.n = n
        self.normA = F["normA"]          # ||A||_F, used by the refinement stopping test
        self.strategy = F["strategy"]
        self.t_factor = F["t_factor"]
        t_a = time.perf_counter()
        Lp, Li, Lx, Up, Ui, Ux, pr, pc = (F[k] for k in ("Lp", "Li", "Lx", "Up", "Ui", "Ux", "perm_r", "perm_c"))
        self.t_convert = time.perf_counter() - t_a
        t_b = time.perf_counter()
        check(lib.nep_lu_set_expected_solves(int(expected_solves)))
        h = c_vp()
        try:
            create = lib.nep_lu_create_csc if F.get("fmt", "csr") == "csc" else lib.nep_lu_create
            check(create(n, hptr(Lp), hptr(Li), hptr(Lx), hptr(Up), hptr(Ui), hptr(Ux), hptr(pr), hptr(pc), C.byref(h)))
        finally:
            Fplan = F
            if shm_backed:
                if for_plan:                # the plan builder reads the index arrays after the shared block is gone
                    Fplan = {k: (np.array(F[k], copy=True) if k in ("Lp", "Li", "Up", "Ui", "perm_r", "perm_c") else F[k])
                             for k in ("Lp", "Li", "Up", "Ui", "perm_r", "perm_c", "fmt", "strategy", "n") if k in F}
                del Lp, Li, Lx, Up, Ui, Ux, pr, pc
                _nep_hostlu.release_shm(F)
        self.h = h
        self.t_create = time.perf_counter() - t_b
        self._describe()
        return Fplan

    def _adopt(self, h, n, normA, strategy, growth):
        """take over an nep_lu handle produced by the device-side numeric factorisation"""
        self.device_factorized = True
        self.growth = growth
        self.n = int(n); self.normA = normA; self.strategy = strategy
        self.t_factor = 0.0; self.t_convert = 0.0; self.t_create = 0.0; self.t_setup = 0.0
        self.h = h
        self._describe()
        return self

    @classmethod
    def _from_handle(cls, h, n, normA, strategy, growth):
        return cls.__new__(cls)._adopt(h, n, normA, strategy, growth)

    def _factor_on_device(self, plan, Ac, expected_solves, t0):
        """numeric factorisation on the GPU with the pattern's stored pivot sequence; False -> the caller takes the host path"""
        health = np.zeros(3)
        h = c_vp()
        Ax = np.ascontiguousarray(Ac.data, dtype=np.complex128)
        check(lib.nep_lu_set_expected_solves(int(expected_solves)))
        rc = lib.nep_lu_factor_dev(plan["handle"], hptr(Ax), int(expected_solves), _DeviceRefactor.GROWTH, hptr(health), None,
                                   C.byref(h), stream_ptr())
        normA = float(np.linalg.norm(Ax))
        t_factor = time.perf_counter() - t0
        if _DeviceRefactor._wrap(plan, h.value if rc == 0 else None, Ac.shape[0], normA, "device (stored pivot sequence)", health,
                                 into=self) is None:
            if rc != _lib.NEP_ERR_SINGULAR or plan["fails"] >= 3:       # repeated breakdowns: the pivot sequence does not suit
                plan["state"] = "off"
            return False
        self.t_factor = t_factor
        self.t_setup = time.perf_counter() - t0
        return True

    def _describe(self):
        n = self.n
        info = (c_i64 * 6)()
        check(lib.nep_lu_info(self.h, info))
        self.nnzL, self.nnzU, self.levL, self.levU, self.solve_bytes = (int(info[1]), int(info[2]), int(info[3]),
                                                                        int(info[4]), int(info[5]))
        sch = (c_i64 * 8)()
        check(lib.nep_lu_schedule(self.h, sch))
        self.tail, self.levL_full, self.levU_full = int(sch[0]), int(sch[2]), int(sch[3])
        self.wide_segments, self.narrow_segments = int(sch[4]), int(sch[5])
        self.mid_rows, self.mid_block = int(sch[6]), int(sch[7])
        ib = C.c_int32(0)
        check(lib.nep_lu_is_block_schedule(self.h, C.byref(ib)))
        self.block_schedule = bool(ib.value)          # elimination-tree block schedule (trsv_ml.hip) vs level schedule
        if self.block_schedule:
            self.levels, self.split_levels, self.blocks = int(sch[2]), int(sch[4]), int(sch[5])
        # (nnz L + nnz U)(16 + 4) + 8(n + 1) + 3*16 n for one right-hand side
        self.algorithmic_bytes = (self.nnzL + self.nnzU) * 20 + 8 * (n + 1) + 48 * n

    def refactor(self, Lx, Ux):
        """same-pattern refactorisation (nep_lu_refactor): new values in the entry order of the factors this handle
        was created with"""
        Lx = np.ascontiguousarray(Lx, dtype=np.complex128); Ux = np.ascontiguousarray(Ux, dtype=np.complex128)
        assert Lx.shape[0] == self.nnzL and Ux.shape[0] == self.nnzU
        check(lib.nep_lu_refactor(self.h, hptr(Lx), hptr(Ux)))

    def set_row_scale(self, rs):
        rs = None if rs is None else np.ascontiguousarray(rs, dtype=np.float64)
        check(lib.nep_lu_set_row_scale(self.h, hptr(rs) if rs is not None else None))

    def transpose(self, conj=False):
        """factors of A^T (conj=False) or A^H (conj=True) from this handle's, without a host round trip or a refactorisation
        (nep_lu_transpose); this handle is left as it was.  NepError (NEP_ERR_UNSUPPORTED) for a level-schedule handle."""
        h = c_vp()
        check(lib.nep_lu_transpose(self.h, 1 if conj else 0, C.byref(h)))
        t = DeviceLU._from_handle(h, self.n, self.normA, dict(getattr(self, "strategy", None) or {}, transposed="H" if conj else "T"),
                                  getattr(self, "growth", None))
        t.device_factorized = getattr(self, "device_factorized", False)
        return t

    def launches_last_solve(self):
        sch = (c_i64 * 8)()
        check(lib.nep_lu_schedule(self.h, sch))
        return int(sch[1])

    def __del__(self):
        try:
            if getattr(self, "h", None):
                lib.nep_lu_destroy(self.h)
                self.h = None
        except Exception:
            pass

    def solve(self, B, out=None, scale=1.0):
        """B: device tensor (nrhs, n) (column-major n x nrhs block). Returns same-shaped tensor."""
        Bd = B if B.dim() == 2 else B.reshape(1, -1)
        nrhs, n = Bd.shape
        assert n == self.n
        X = torch.empty_like(Bd) if out is None else out
        check(lib.nep_lu_solve(self.h, nrhs, c_vp(Bd.data_ptr()), n, c_vp(X.data_ptr()), n, float(scale), stream_ptr()))
        return X.reshape(B.shape)

    def solve_add(self, B, add, out, scale=1.0):
        """out = scale * (add + A^{-1} B)  (refinement update; out may alias add)"""
        Bd = B if B.dim() == 2 else B.reshape(1, -1)
        nrhs, n = Bd.shape
        assert n == self.n
        check(lib.nep_lu_solve_add(self.h, nrhs, c_vp(Bd.data_ptr()), n, c_vp(add.data_ptr()), n, c_vp(out.data_ptr()), n,
                                   float(scale), stream_ptr()))
        return out


class TermsRoute:
    """where a pure SPMF NEP's matrices sum_t c_t A_t are factorised on the device: the union `pattern` of its terms, that pattern's
    ready `plan` (None: not planned yet, or switched off), the nnz x m_t term values `D_dev` on the device and their Gram matrix `G`"""

    def __init__(self, n, pattern, plan, D_dev, G):
        self.n, self.pattern, self.plan, self.D_dev, self.G = n, pattern, plan, D_dev, G


def terms_route(nep):
    """the TermsRoute of `nep`, or None: device factorisation switched off, a NEP with parts outside its SPMF terms (a plan keyed by
    the terms' pattern would factorise the terms alone), a dense term.  Nothing is uploaded for a NEP that is refused."""
    if not _DeviceRefactor.enabled():
        return None
    if not (pure_spmf(nep, "Mder") and hasattr(nep, "aligned_terms_dev")):
        return None
    al = nep.aligned_terms_dev()
    if al is None:
        return None
    indptr, indices, D_dev, G = al
    pattern = _Pattern(indptr, indices, (nep.n, nep.n))
    return TermsRoute(nep.n, pattern, _DeviceRefactor.lookup(_DeviceRefactor.key(pattern, (None, None, None))), D_dev, G)


def factor_term_rows(route, Cf, expected_solves, growth=None):
    """the matrices sum_t Cf[b, t] A_t (Cf: B x m_t) factorised in one batch with the stored pivot sequence of the route's plan:
    only the coefficients travel, the values are formed on the device (k_lu_init_terms) and ||.||_F comes from the Gram matrix.
    growth: the element growth accepted (None: _DeviceRefactor.GROWTH; GROWTH_UNREFINED for factors whose solves no refinement
    follows).  A list of DeviceLU with None where that matrix was refused; None without a ready plan."""
    if route is None or route.plan is None:
        return None
    Cf = np.asarray(Cf, dtype=np.complex128)
    normA = np.sqrt(np.maximum(np.einsum("bs,st,bt->b", Cf.conj(), route.G, Cf).real, 0.0))
    return _DeviceRefactor.factor_batch_terms(route.plan, route.n, route.D_dev, Cf, normA, expected_solves=expected_solves,
                                              growth=growth)


def _single_terms_route(nep, lu_kw):
    """the route of lu_from_terms and lu_from_term_coeffs (one matrix, a factorisation that is reused), or None"""
    if set(lu_kw) - {"expected_solves"} or env_str("NEP_LU_TERMS", "1") == "0":
        return None
    if not _DeviceRefactor.plans:                      # nothing planned yet: do not build the device term block for it
        return None
    route = terms_route(nep)
    return route if (route is not None and route.plan is not None) else None


def _single_from_row(route, Cf, lu_kw):
    """the one matrix sum_t Cf[0, t] A_t factorised on the route's plan for reuse, with the strategy note of a single factorisation"""
    lu = factor_term_rows(route, Cf, int(reused(lu_kw)["expected_solves"]))[0]
    if lu is not None:
        lu.strategy = dict(route.plan["strategy"], numeric="device (stored pivot sequence)")
    return lu


def lu_from_terms(nep, lam, permc_spec, lu_kw):
    """M(lam) = sum_t f_t(lam) A_t of a pure SPMF NEP whose pattern has a device-factorisation plan: the m_t coefficients go
    to the device, the values are assembled there (k_lu_init_terms) and factorised with the stored pivot sequence -- no
    compute_Mder on the host, no value upload, no pattern hash (1 ms of the 4.4 ms a gun linear solver took).  None: the
    caller takes the general route (no plan yet, other options, a refusal)."""
    route = _single_terms_route(nep, lu_kw) if permc_spec is None else None
    if route is None:
        return None
    return _single_from_row(route, [[f.derivs(lam, 1)[0] for f in nep.get_fv()]], lu_kw)


def lu_from_term_coeffs(nep, coef, lu_kw=None):
    """sibling of lu_from_terms for a matrix given by its coefficient row, C = sum_t coef[t] A_t on the terms of a pure SPMF NEP
    (the shifted pencil tau M'(lam) - M(lam) of an eigensolver: coef = tau f_t'(lam) - f_t(lam)): assembled and factorised on the
    device with the stored pivot sequence of the pattern's plan.  None: no plan (yet), a NEP with terms outside its SPMF sum, a
    refusal -- the caller takes the general route."""
    lu_kw = lu_kw or {}
    route = _single_terms_route(nep, lu_kw)
    if route is None:
        return None
    return _single_from_row(route, np.asarray(coef, dtype=np.complex128).reshape(1, -1), lu_kw)


def seed_plan_from_rank0(nep, lam, group=None, permc_spec=None, wait=True):
    """Collective over the ranks of a node (torch.distributed): the FIRST factorisation of a sparsity pattern -- the host SuperLU
    run that fixes ordering, pivot sequence and fill, and from which the pattern's device-factorisation plan is built -- is done
    by rank 0 alone and its factor arrays are broadcast; every rank uploads them, starts its plan (enumerated on its own GPU,
    21 ms for gun) and, with wait=True, returns when the plan is ready, so that no rank ever runs SuperLU for this pattern (8
    ranks on a shared CPU quota would otherwise start 8 concurrent host factorisations in their first call).  Returns the
    DeviceLU of M(lam) built from the broadcast factors.  Without an initialised process group: the plain local path."""
    import torch.distributed as dist
    A = sp.csc_matrix(nep.compute_Mder(lam), dtype=np.complex128)
    A.sort_indices()
    distd = dist.is_available() and dist.is_initialized() and dist.get_world_size(group) > 1
    rank = dist.get_rank(group) if distd else 0
    F = host_factor(A, permc_spec) if rank == 0 else None
    if distd:
        box = [F]
        dist.broadcast_object_list(box, src=dist.get_global_rank(group, 0) if group is not None else 0, group=group)
        F = box[0]
    seed_plan_from_rank0.host_factorisations += 1 if rank == 0 else 0
    lu = DeviceLU(factors=F, plan_pattern=A, permc_spec=permc_spec)
    if wait:
        _DeviceRefactor.wait()
    return lu


seed_plan_from_rank0.host_factorisations = 0
