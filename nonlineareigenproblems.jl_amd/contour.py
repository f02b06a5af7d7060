"""Beyn's contour-integral method on the device backend, with the quadrature nodes sharded over
the GPUs of one node (one process per GPU, torch.distributed backend "nccl" = RCCL over xGMI).

Mirrors src/method_beyncontour.jl:49-185 and the quadrature seam src/method_contour_common.jl:8-94:
`contour_beyn(nep, MIntegrator; tol, sigma, linsolvercreator, neigs, k, radius, N, errmeasure,
sanity_check, rank_drop_tol)` and `integrate_interval(::Type{<:MatrixIntegrator}, T, f, gv, a, b, N)`.

Per quadrature node (method_beyncontour.jl:89-94): M(sigma+g(t_i)) is assembled and factorised on
the host (new matrix per node -- BackslashLinSolverCreator is the reference default), its factors
are uploaded, and the n x k block solve runs on the device (K5 with grid.y = k).  The two moment
sums stay on the device (K8 = nep_axpy).  `MatrixTrapezoidalSharded` gives rank r the nodes
i = r (mod P); the only exchange is ONE all-gather of the 2 n k partial block, followed by a
fixed-order sum so that every rank holds bit-identical A0, A1.
"""

import numpy as np
import scipy.linalg as sla
import torch
import torch.distributed as dist

from . import dense
from ._env import env_flag, env_str
from .errmeasure import DefaultErrmeasure, estimate_errors
from .linsolvers import BackslashLinSolverCreator, DeviceLU, HostLUPool, create_linsolver, lin_solve, _DeviceRefactor
from .nep import CDT, to_dev, to_host

EPS = np.finfo(float).eps


class MatrixIntegrator:
    """src/method_contour_common.jl:46"""


class MatrixTrapezoidal(MatrixIntegrator):
    """trapezoidal rule on one GPU (src/method_contour_common.jl:55,61-94)"""
    sharded = False


class MatrixTrapezoidalSharded(MatrixIntegrator):
    """trapezoidal rule with the N nodes sharded over the ranks (one process per GPU): rank r owns the nodes i = r (mod P);
    the exchange is nep_allgather_sum of the C ABI (RCCL all-gather over xGMI + fixed-order sum, csrc/comm.hip).  `comm`: a
    comm.DeviceComm; None = the communicator spanning torch.distributed's default group (created on first use).  CPU
    tensors (the gloo test of the sharding logic) are exchanged through torch.distributed itself."""
    sharded = True
    comm = None


class _DeviceOps:
    """accumulation primitives of the quadrature: the library's HIP kernels"""
    axpy = staticmethod(dense.axpy)
    scal = staticmethod(dense.scal)


_SOLVE_STREAMS = {}

def integrate_interval(ST, f, gv, a, b, N, info=None, ops=_DeviceOps):
    """returns S with S[j] ~ int f(t) g_j(t) dt  as a device tensor (m, k, n) (m = len(gv)).
    f(t) returns (X, c): the integrand value is c*X with X a device (k, n) block.
    `ops` exists so that the sharding / all-gather / fixed-order-sum logic can be exercised by the
    world_size-2 gloo test on CPU tensors; the drivers always use the HIP kernels."""
    h = (b - a) / N
    t = a + h * np.arange(N)
    m = len(gv)
    G = np.array([[g(tt) for g in gv] for tt in t], dtype=np.complex128)    # N x m
    world, rank = 1, 0
    comm = getattr(ST, "comm", None) if getattr(ST, "sharded", False) else None
    if comm is not None:
        world, rank = comm.world, comm.rank
    elif getattr(ST, "sharded", False) and dist.is_available() and dist.is_initialized():
        world, rank = dist.get_world_size(), dist.get_rank()
    S = None
    mine = range(rank, N, world)
    # info["phases_s"] (a dict the caller put there): wall time of the pieces, each closed by a device synchronisation -- for the
    # record of what is sharded (factorise, solve) and what every rank repeats (the rest), also with one rank
    ph = info.get("phases_s") if (info is not None and isinstance(info.get("phases_s"), dict)) else None
    import time as _time

    def _tick(name, t0):
        if ph is not None:
            if torch.cuda.is_available() and (S is None or S.is_cuda):
                torch.cuda.synchronize()
            ph[name] = ph.get(name, 0.0) + _time.perf_counter() - t0
        return _time.perf_counter()
    tp = _time.perf_counter()
    if hasattr(f, "prefetch"):
        f.prefetch([t[i] for i in mine])
    tp = _tick("factorise_nodes", tp)
    # Node solves whose factors are all on the device already (the batched numeric LU): the solve of one node is a chain of ~15 kernels
    # that do not fill the chip (32 right-hand sides, 0.64 ms per node on gun), and the nodes are independent -- they go round robin
    # onto two side streams, each result into its own block, and are accumulated on the caller's stream IN NODE ORDER (the sum
    # is the same, to the bit, as with one stream).
    nstreams = 2    # measured on C4: 83.0 / 76.9 / 78-110 / 80.2 / 79.2 ms with 1 / 2 / 3 / 4 / 8 streams
    ready = getattr(f, "ready", None)
    if nstreams > 1 and ready and torch.cuda.is_available() and all(t[i] in ready for i in mine) and len(mine) > 1:
        cur = torch.cuda.current_stream()
        sts = _SOLVE_STREAMS.setdefault(torch.cuda.current_device(), [])
        if len(sts) < nstreams:
            # side streams that share a hardware queue with neither the caller's stream nor each other (probed once per process and
            # device, nep_stream_pair_serializes): the runtime maps streams onto a small pool of queues in creation order, and two
            # "concurrent" solve streams on ONE queue run one after the other (round 6: 21 instead of 13 ms for the 64 node solves of
            # C4, depending on which streams the process happened to create before)
            from .iar import _eig_streams
            sts[:] = list(_eig_streams(nstreams, others=(cur,)))
        for s_ in sts[:nstreams]:
            s_.wait_stream(cur)
        pend = []
        for q, i in enumerate(mine):
            s_ = sts[q % nstreams]
            with torch.cuda.stream(s_):
                X, c = f(t[i])
                ev = torch.cuda.Event(); ev.record(s_)
            pend.append((i, X, c, ev))
        for i, X, c, ev in pend:
            cur.wait_event(ev)
            if S is None:
                S = torch.zeros((m,) + tuple(X.shape), dtype=CDT, device=X.device)
            for j in range(m):
                ops.axpy(c * G[i, j], X, S[j])
            X.record_stream(cur)
        del pend
    else:
        for i in mine:
            X, c = f(t[i])
            if S is None:
                S = torch.zeros((m,) + tuple(X.shape), dtype=CDT, device=X.device)
            for j in range(m):
                ops.axpy(c * G[i, j], X, S[j])
    tp = _tick("solve_nodes_and_accumulate", tp)
    if S is None:
        raise ValueError("rank %d owns no quadrature node (N=%d < world size %d)" % (rank, N, world))
    if getattr(ST, "sharded", False) and S.is_cuda and (comm is not None or (dist.is_available() and dist.is_initialized())):
        if comm is None:
            from .comm import DeviceComm
            comm = DeviceComm.from_torch_distributed()
        comm.allgather_sum(S)                      # C ABI: RCCL all-gather over xGMI (2*n*k complex128 per rank) + fixed-order sum
    elif world > 1:
        parts = [torch.empty_like(S) for _ in range(world)]
        dist.all_gather(parts, S)                  # CPU tensors (gloo test of the sharding logic)
        S = torch.zeros_like(S)
        for p in parts:                            # fixed rank order -> identical on every rank
            ops.axpy(1.0, p, S)
    ops.scal(S, h)
    tp = _tick("exchange_and_sum", tp)
    if info is not None:
        info.update(world=world, rank=rank, nodes=len(mine))
        if comm is not None and getattr(comm, "last_exchange_s", None) is not None:
            info["exchange_s"] = float(comm.last_exchange_s)
    return S


class _NodeSolve:
    """f(t) = Tv(g(t)) * weight(t), Tv(lam) = lin_solve(create_linsolver(creator, nep, lam+sigma), Vh)
    (method_beyncontour.jl:89-98, method_block_SS.jl:81-86,129-132).  With the default BackslashLinSolverCreator every
    node needs a NEW host factorisation; `prefetch` starts all factorisations of this rank's nodes in worker processes
    so that they run concurrently with each other and with the device solves of the nodes already factored."""

    BUILDERS = 4   # threads turning host factors into device schedules (nep_lu_create releases the GIL)
    AHEAD = 8      # device factorisations built (or being built) ahead of the node being solved

    def __init__(self, nep, linsolvercreator, sigma, g, Vd, weight):
        self.nep, self.creator, self.sigma, self.g, self.Vd, self.weight = nep, linsolvercreator, sigma, g, Vd, weight
        self.host = {}        # t -> future of the host factorisation (worker process)
        self.built = {}       # t -> future of the DeviceLU (builder thread)
        self.order = []
        self.next = 0
        self.pool = None
        self._pattern = None  # csc pattern of M (all nodes share it) when the host path may seed a device plan

    def _build(self, host_future, dev):
        # host factors -> level analysis, upload, tail inverse (6 ms for gun): off the main thread, which only issues the
        # block solves and the moment updates
        torch.cuda.set_device(dev)
        try:
            F = host_future.result()
        except RuntimeError as e:
            raise np.linalg.LinAlgError("SingularException: " + str(e))
        # (the first host factorisation of a pattern seeds its device-factorisation plan: the NEXT contour_beyn call on this
        # pattern factorises all its nodes on the GPU in one batch)
        return DeviceLU(factors=F, expected_solves=1, plan_pattern=self._pattern)

    def _submit_builds(self):
        # never more than AHEAD builds outstanding; submitted in node order by the consuming thread (no blocking
        # primitives in the builders, so an exception in the consumer cannot leave a thread waiting)
        dev = torch.cuda.current_device()
        while self.next < len(self.order) and len(self.built) < self.AHEAD:
            t = self.order[self.next]
            self.built[t] = self.pool.submit(self._build, self.host.pop(t), dev)
            self.next += 1

    def prefetch(self, ts):
        c = self.creator
        workers = getattr(c, "workers", None)
        if not isinstance(c, BackslashLinSolverCreator) or workers == 0 or len(ts) < 2:
            return
        from concurrent.futures import ThreadPoolExecutor
        self.pool = ThreadPoolExecutor(max_workers=self.BUILDERS)
        self.order = list(ts)
        trace = env_flag("NEP_BEYN_TRACE")
        if trace:
            import time as _t
            self._t0 = _t.perf_counter(); self._host_done = []; self._host_meta = []
        # ---- all nodes on the GPU in one pass when the pattern has a device-factorisation plan (_devicelu._DeviceRefactor):
        # one B x m_t by m_t x nnz product for the values, one batched numeric LU (every launch carries all nodes); nodes
        # whose factorisation is refused with the stored pivot sequence take the host path below
        self.ready = {}
        ts_host = list(ts)
        if (_DeviceRefactor.enabled() and hasattr(self.nep, "aligned_terms_dev") and c.permc_spec is None and not c.lu_kw
                and not env_flag("NEP_BEYN_HOST_LU")):
            al = self.nep.aligned_terms_dev()
            if al is not None:
                indptr, indices, D_dev, G = al

                class _Pattern:             # what _DeviceRefactor.key / maybe_start read of a csc matrix
                    pass
                A0 = _Pattern(); A0.indptr = indptr; A0.indices = indices; A0.shape = (self.nep.n, self.nep.n)
                plan = _DeviceRefactor.lookup(_DeviceRefactor.key(A0, (None, None, None)))
                lu_first = None
                if plan is None and len(ts) >= 4 and env_str("NEP_BEYN_COLD_PLAN", "1") != "0":
                    # FIRST call on this sparsity pattern: instead of sending all N nodes to the host-factorisation worker pool (gun,
                    # N = 64: 0.67 s for the call, most of it the pool's start-up and 64 SuperLU runs) the first node is factorised on
                    # the host in this process, its device-LU plan is built right away (enumeration on the GPU, ~25 ms) and waited
                    # for, and the other N - 1 nodes take the batched device factorisation below like every later call
                    from .linsolvers import DeviceLU
                    try:
                        lu_first = DeviceLU(self.nep.compute_Mder(self.g(ts[0]) + self.sigma), expected_solves=1)
                        _DeviceRefactor.wait()
                        plan = _DeviceRefactor.lookup(_DeviceRefactor.key(A0, (None, None, None)))
                    except Exception:
                        lu_first = None; plan = None          # (singular node, refused plan ...: the host route below handles every node)
                    if plan is None:
                        lu_first = None
                if plan is None:
                    self._pattern = A0
                if plan is not None:
                    # M(lam_b) = sum_t f_t(lam_b) A_t: only the B x m_t coefficients travel, the values are formed on the GPU
                    fv = self.nep.get_fv()
                    tsb = list(ts[1:]) if lu_first is not None else list(ts)       # (the first node of a cold call keeps its host factors)
                    if lu_first is not None:
                        self.ready[ts[0]] = lu_first
                    Cf = np.array([[f.derivs(self.g(t) + self.sigma, 1)[0] for f in fv] for t in tsb], dtype=np.complex128)
                    normA = np.sqrt(np.maximum(np.einsum("bs,st,bt->b", Cf.conj(), G, Cf).real, 0.0))
                    lus = _DeviceRefactor.factor_batch_terms(plan, self.nep.n, D_dev, Cf, normA, expected_solves=1,
                                                             growth=_DeviceRefactor.GROWTH_UNREFINED)
                    ts_host = []
                    for t, lu in zip(tsb, lus):
                        if lu is None:
                            ts_host.append(t)
                        else:
                            self.ready[t] = lu
                    if trace:
                        print("[beyn trace] %d of %d nodes factorised on the device (batched) at %.0f ms" %
                              (len(self.ready), len(ts), 1e3 * (_t.perf_counter() - self._t0)), flush=True)
        self.order = list(ts_host)
        strat = None
        for t in ts_host:
            A = self.nep.compute_Mder(self.g(t) + self.sigma)
            if strat is None:
                # UMFPACK-like strategy (symmetric pattern + zero-free diagonal?) decided ONCE: all nodes share one pattern
                import nep_amd_hostlu as hl
                import scipy.sparse as sp_
                kw0 = dict(c.lu_kw)
                if c.permc_spec is None and "symmetric_mode" not in kw0:
                    sym = hl.pattern_symmetric(sp_.csc_matrix(A))
                    strat = dict(permc_spec="MMD_AT_PLUS_A" if sym else "COLAMD", symmetric_mode=bool(sym))
                else:
                    strat = dict(permc_spec=c.permc_spec)
            self.host[t] = HostLUPool.submit(A, workers=workers, **dict(c.lu_kw, **strat))
            if trace:
                self.host[t].add_done_callback(lambda f, s=self: (s._host_done.append(_t.perf_counter() - s._t0),
                                                                   s._host_meta.append(f.result() if not f.exception() else {})))
        if trace:
            self._t_submitted = _t.perf_counter() - self._t0
        self._submit_builds()

    def close(self):
        if self.pool is not None:
            for f in list(self.built.values()) + list(self.host.values()):
                f.cancel()
            self.pool.shutdown(wait=True)
            self.pool = None
            # host factorisations that finished (or still finish) but were never turned into a DeviceLU own a shared-memory
            # block nobody else will unlink (the worker handed ownership to this process): release it
            import nep_amd_hostlu as hl

            def _release(fut):
                try:
                    meta = fut.result()
                    if isinstance(meta, dict) and "shm_name" in meta:
                        hl.release_shm(hl.attach_shm(meta))
                except BaseException:
                    pass
            for f in self.host.values():
                if f.done():
                    _release(f)
                else:
                    f.add_done_callback(_release)
            self.built.clear(); self.host.clear()

    def __call__(self, t):
        if t in getattr(self, "ready", {}):
            lu = self.ready.pop(t)
            X = lu.solve(self.Vd)
            if not self.ready and not self.built and self.next >= len(self.order):
                self.close()
            return X, self.weight(t)
        if t in self.built:
            try:
                lu = self.built.pop(t).result()
                self._submit_builds()
                X = lu.solve(self.Vd)
            except BaseException:
                self.close()
                raise
            if not self.built and self.next >= len(self.order):
                if env_flag("NEP_BEYN_TRACE"):
                    import time as _t
                    hd = sorted(self._host_done)
                    mt_ = [m_ for m_ in self._host_meta if "t_worker" in m_]
                    if mt_:
                        print("[beyn trace] per factorisation in the worker: splu %.1f ms, factor() %.1f ms, whole task %.1f ms (means over %d)"
                              % (1e3 * np.mean([m_["t_factor"] for m_ in mt_]), 1e3 * np.mean([m_["t_worker_factor_call"] for m_ in mt_]),
                                 1e3 * np.mean([m_["t_worker"] for m_ in mt_]), len(mt_)), flush=True)
                    print("[beyn trace] submitted all at %.0f ms; host factorisations done: first %.0f ms, half %.0f ms, last %.0f ms; "
                          "last block solve issued at %.0f ms" % (1e3 * self._t_submitted, 1e3 * hd[0], 1e3 * hd[len(hd) // 2], 1e3 * hd[-1],
                                                                  1e3 * (_t.perf_counter() - self._t0)), flush=True)
                self.close()
            return X, self.weight(t)
        M0inv = create_linsolver(self.creator, self.nep, self.g(t) + self.sigma)
        return lin_solve(M0inv, self.Vd), self.weight(t)


def _beyn_tail_device(S, n, k, rank_drop_tol):
    """the dense tail of Beyn's method with the n x k moments left on the device (see contour_beyn).  S: device (2, k, n) block of the
    UNSCALED moments (A_j = S[j] / (2 pi i)).  Returns (singular values of A0, rank p, B (p x p, host), Q (device (k, n)), U_R[:, :p])
    or None when the device QR met a breakdown (the caller then takes the host route)."""
    Qd = S[0].clone()                                      # (k, n) = column-major n x k; orthonormalised in place, column by column
    from ._lib import lib, check, c_vp, cd
    from .nep import stream_ptr
    ksplit = int(min(64, max(1, n // 512)))
    buf = torch.zeros((k * (k + 2) + k * k + ksplit * k * k,), dtype=CDT, device=S.device)      # R rows | G | split-K slices
    outs = buf[:k * (k + 2)].view(k, k + 2); Gd = buf[k * (k + 2):k * (k + 2) + k * k].view(k, k); work = buf[k * (k + 2) + k * k:]
    check(lib.nep_orth_qr_dev(c_vp(Qd.data_ptr()), n, n, k, c_vp(outs.data_ptr()), stream_ptr()))
    # G = Q^H S[1] (k x k, column-major) on the library's own GEMM, the n-long reduction split over `ksplit` workgroups
    check(lib.nep_zgemm_sk(2, 0, k, k, n, cd(1.0), c_vp(Qd.data_ptr()), n, c_vp(S[1].data_ptr()), n, cd(0.0), c_vp(Gd.data_ptr()), k, ksplit,
                           c_vp(work.data_ptr()), stream_ptr()))
    bh = buf[:k * (k + 2) + k * k].cpu().numpy()             # ONE download: k (k + 2) + k^2 numbers
    oh = bh[:k * (k + 2)].reshape(k, k + 2)
    G = bh[k * (k + 2):].reshape(k, k).T                    # Gd[c, r] = G[r, c]
    R = np.zeros((k, k), dtype=np.complex128)
    for j in range(k):
        if int(oh[j, j + 1].imag) & 2:                      # breakdown flag (||w|| = 0 or not finite)
            return None
        R[:j, j] = oh[j, :j]
        R[j, j] = oh[j, j].real
    # svd(R) = svd(A0) and V = Q U_R hold for an ORTHONORMAL Q only.  A column whose last enqueued DGKS pass still met the
    # re-orthogonalisation criterion (flag bit 0) is not known to be orthogonal to its predecessors: harmless for a noise column (A0 is
    # rank deficient by design: R[j, j] at round-off of R[0, 0]), not for one that carries weight -- the host route then (svd of the
    # downloaded block, as the reference does it)
    r00 = abs(R[0, 0]) if k else 0.0
    for j in range(k):
        if (int(oh[j, j + 1].imag) & 1) and abs(R[j, j]) > 1e-10 * r00:
            return None
    c = 1.0 / (2j * np.pi)
    Ur, Sv, Wh = sla.svd(R * c)                             # A0 = Q (R / (2 pi i)): same singular values, V = Q U_R
    p = int(np.sum(Sv / Sv[0] > rank_drop_tol))
    W0 = Wh.conj().T[:, :p]
    UrP = Ur[:, :p]
    B = (UrP.conj().T @ (G * c) @ W0) @ np.diag(1.0 / Sv[:p])
    return Sv, p, B, Qd, UrP


def probe_block(n, k, seed=10):
    """deterministic standard-normal probe (the reference's `Random.seed!(10); randn(n,k)`,
    method_beyncontour.jl:85-86, is Julia-RNG specific; counter-based Philox here)"""
    rng = np.random.Generator(np.random.Philox(seed))
    return rng.standard_normal((n, k)).astype(np.complex128)


def contour_beyn(nep, MIntegrator=MatrixTrapezoidal, tol=np.sqrt(EPS), sigma=0.0, logger=0,
                 linsolvercreator=None, neigs=2, k=None, radius=1, N=1000, errmeasure=None,
                 sanity_check=True, rank_drop_tol=None, Vh=None, info=None):
    if k is None:
        if neigs >= np.iinfo(np.int64).max:
            raise ValueError("k must be positive. The kwarg k must be set if you use neigs=typemax")
        k = neigs + 1
    if rank_drop_tol is None:
        rank_drop_tol = tol
    if np.isscalar(radius):
        radius = (radius, radius)
    if linsolvercreator is None:
        linsolvercreator = BackslashLinSolverCreator()
    if errmeasure is None:
        errmeasure = DefaultErrmeasure(nep)
    sigma = complex(sigma)
    g = lambda t: complex(radius[0] * np.cos(t), radius[1] * np.sin(t))
    gp = lambda t: complex(-radius[0] * np.sin(t), radius[1] * np.cos(t))
    n = nep.size(1)
    if k > n:
        raise ValueError("Cannot compute more eigenvalues than the size of the NEP with contour_beyn() k=%d n=%d" % (k, n))
    if k <= 0:
        raise ValueError("k must be positive, k=%d." % k)
    import time as _time
    ph = info.get("phases_s") if (info is not None and isinstance(info.get("phases_s"), dict)) else None

    def _tick(name, t0):
        if ph is not None:
            torch.cuda.synchronize()
            ph[name] = ph.get(name, 0.0) + _time.perf_counter() - t0
        return _time.perf_counter()
    tp = _time.perf_counter()
    if Vh is None:
        Vh = probe_block(n, k)
    Vd = to_dev(Vh)
    tp = _tick("probe_generate_and_upload", tp)

    f = _NodeSolve(nep, linsolvercreator, sigma, g, Vd, gp)

    S = integrate_interval(MIntegrator, f, [lambda s: 1.0 + 0j, g], 0.0, 2 * np.pi, N, info=info)
    tp = _time.perf_counter()
    dev_tail = (S.is_cuda and k >= 2 and env_str("NEP_BEYN_DEVICE_TAIL", "1") != "0")
    A0 = A1 = None
    lam = None
    if dev_tail:
        # The moments stay on the device (method_beyncontour.jl:114-128 needs only k x k pieces of them on the host): A0 = Q R by
        # column-wise DGKS on the device (K6; the columns A0 has beyond its rank become orthonormalised noise, R shows the rank),
        # svd(R) on the host (k x k) gives the singular values of A0 and V = Q U_R; B = V0^H A1 W0 S^-1 = U_R^H (Q^H A1) W0 S^-1 with
        # the k x k Gram block Q^H A1 from the device; the eigenvectors V0 VB = Q (U_R VB) by K7.  Downloaded: two k x (k + 2)
        # blocks instead of two n x k ones; the n x k SVD (9 ms of host LAPACK on gun, repeated by every rank) is gone.
        got = _beyn_tail_device(S, n, k, rank_drop_tol)
        if got is not None:
            Sv, p, B, Qd, UrP = got
            lam, VB = sla.eig(B)
            lam = lam + sigma
            tp = _tick("svd_and_eig_host", tp)
            QT = dense.gemm_ts(Qd, UrP @ VB, rowmajor=True)        # (n, p) row-major
            tp = _tick("eigenvectors", tp)
            if info is not None and info.get("moments", True):      # (a caller that wants them; bench.py's timed call opts out)
                A0 = to_host(S[0]) / (2j * np.pi); A1 = to_host(S[1]) / (2j * np.pi)
    if lam is None:
        A0 = to_host(S[0]) / (2j * np.pi)
        A1 = to_host(S[1]) / (2j * np.pi)
        tp = _tick("moments_download", tp)
        V, Sv, Wh = sla.svd(A0, full_matrices=False)
        W = Wh.conj().T
        p = int(np.sum(Sv / Sv[0] > rank_drop_tol))
        V0 = V[:, :p]; W0 = W[:, :p]
        B = (V0.conj().T @ A1 @ W0) @ np.diag(1.0 / Sv[:p])
        lam, VB = sla.eig(B)
        lam = lam + sigma
        tp = _tick("svd_and_eig_host", tp)
        # eigenvectors V0*VB on the device (K7), normalised
        V0d = to_dev(V0)
        QT = dense.gemm_ts(V0d, VB, rowmajor=True)                 # (n, p) row-major
        tp = _tick("eigenvectors", tp)
    if info is not None:
        info.update(p=p, S=Sv, A0=A0, A1=A1)

    def inside(l):
        return ((l - sigma).real / radius[0]) ** 2 + ((l - sigma).imag / radius[1]) ** 2 <= 1

    def cols(sel):
        Q = to_host(dense.rowmajor_to_cols(QT, np.asarray(sel, dtype=np.int32)))
        return Q / np.linalg.norm(Q, axis=0)[None, :] if Q.shape[1] else Q

    if not sanity_check:
        si = np.argsort(abs(sigma - lam), kind="stable")
        perm = np.argsort(~inside(lam[si]), kind="stable")
        return lam[si[perm]], cols(si[perm])
    errs = estimate_errors(errmeasure, lam, QT)
    tp = _tick("residual_filter", tp)
    good = np.nonzero(errs < tol)[0]
    sgi = good[np.argsort(abs(sigma - lam[good]), kind="stable")]
    perm = np.argsort(~inside(lam[sgi]), kind="stable")
    sel = sgi[perm]
    if len(sel) > neigs:
        sel = sel[:neigs]
    if info is not None:
        info.update(errs=errs)
    return lam[sel], cols(sel)


def probe_block_uniform(n, L, seed=10):
    """deterministic stand-in for `Random.seed!(10); U = rand(T,n,L); V = rand(T,n,L)` (method_block_SS.jl:77-79):
    real and imaginary parts uniform in [0,1), U drawn before V (counter-based Philox)"""
    rng = np.random.Generator(np.random.Philox(seed))
    U = rng.random((n, L)) + 1j * rng.random((n, L))
    V = rng.random((n, L)) + 1j * rng.random((n, L))
    return U, V


def contour_block_SS(nep, MIntegrator=MatrixTrapezoidal, tol=np.sqrt(EPS), sigma=0.0, logger=0, linsolvercreator=None,
                     neigs=np.inf, k=3, radius=1, N=1000, K=3, errmeasure=None, sanity_check=True, Shat_mode="native",
                     rank_drop_tol=None, U=None, V=None, info=None):
    """Block SS (Asakura/Sakurai/Tadano/Ikegami/Kimura) contour method, src/method_block_SS.jl:47-214: the same
    node solves as contour_beyn (host factorisation per node, n x L block solve on the device, K5 with grid.y = L), but
    2K moment blocks accumulated on the device (K8) through the same `integrate_interval` seam -- so
    `MatrixTrapezoidalSharded` shards it over GPUs exactly like Beyn.  The small Hankel
    SVD / generalised eigenproblem run on the host; the eigenvector block S*(VV1*X) on the device (K7).
    `neigs`, `errmeasure`, `sanity_check` are accepted and unused, as in the reference (:57,:62-63)."""
    if rank_drop_tol is None:
        rank_drop_tol = tol
    if linsolvercreator is None:
        linsolvercreator = BackslashLinSolverCreator()
    sigma = complex(sigma)
    n = nep.size(1)
    L = int(k)
    if U is None or V is None:
        U, V = probe_block_uniform(n, L)
    Vd = to_dev(V)
    if Shat_mode == "JSIAM":
        if not np.isscalar(radius):
            raise ValueError("JSIAM Shat_mode does not support ellipses")
        # nodes omega_j = radius*exp(i t_j), t_j = 2 pi (j + 1/2)/N; Shat_k = (1/N) sum_j (omega_j/radius)^(k+1) F(omega_j)^-1 V
        g = lambda t: radius * np.exp(1j * t)
        f = _NodeSolve(nep, linsolvercreator, sigma, g, Vd, lambda t: 1.0 / (2 * np.pi))
        gv = [(lambda s, kk=kk: np.exp(1j * (kk + 1) * s)) for kk in range(2 * K)]
        a = np.pi / N
        factor = radius
    elif Shat_mode == "native":
        r1 = (radius, radius) if np.isscalar(radius) else tuple(radius)
        g = lambda t: complex(r1[0] * np.cos(t), r1[1] * np.sin(t))
        gp = lambda t: complex(-r1[0] * np.sin(t), r1[1] * np.cos(t))
        f = _NodeSolve(nep, linsolvercreator, sigma, g, Vd, lambda t: gp(t) / (2j * np.pi))
        gv = [(lambda s, kk=kk: g(s) ** kk) for kk in range(2 * K)]
        a = 0.0
        factor = 1.0
    else:
        raise ValueError("Unknown Shat_mode: %s" % Shat_mode)
    Sd = integrate_interval(MIntegrator, f, gv, a, a + 2 * np.pi, N, info=info)       # device (2K, L, n)
    Sh = [to_host(Sd[j]) for j in range(2 * K)]                                         # n x L each
    UH = np.asarray(U).conj().T
    Mhat = [UH @ Sh[j] for j in range(2 * K)]                                           # :151-153
    m = K * L
    Hhat = np.zeros((m, m), dtype=np.complex128); Hhat2 = np.zeros((m, m), dtype=np.complex128)   # :157-167
    for i in range(K):
        for j in range(K):
            Hhat[i * L:(i + 1) * L, j * L:(j + 1) * L] = Mhat[i + j]
            Hhat2[i * L:(i + 1) * L, j * L:(j + 1) * L] = Mhat[i + j + 1]
    UU, SS, VVh = sla.svd(Hhat)                                                        # :172-188
    VV = VVh.conj().T
    mprime = int(np.sum(SS / SS[0] > rank_drop_tol))
    UU1 = UU[:, :mprime]; VV1 = VV[:, :mprime]
    xi, X = sla.eig(UU1.conj().T @ Hhat2 @ VV1, UU1.conj().T @ Hhat @ VV1)             # :191-197
    # eigenvector block S * (VV1 X), S = [Shat_0 ... Shat_{K-1}] (n x KL) = the first K moment blocks, already contiguous
    S = Sd[:K].reshape(K * L, n)
    Vout = to_host(dense.gemm_ts(S, VV1 @ X, rowmajor=False))                           # :202-207
    if info is not None:
        info.update(mprime=mprime, SS=SS)
    return sigma + factor * xi, Vout
