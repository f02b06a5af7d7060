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

import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import scipy.linalg as sla
import scipy.sparse as sp
import torch
import torch.distributed as dist

from . import dense
from ._env import env_flag, env_str
from ._devicelu import GROWTH_UNREFINED
from ._streams import _eig_streams
from .errmeasure import DefaultErrmeasure, estimate_errors
from .linsolvers import (BackslashLinSolverCreator, DeviceLU, HostLUPool, create_linsolver, factor_term_rows, lin_solve, terms_route,
                         _DeviceRefactor, _nep_hostlu)
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


class _Phases:
    """info["phases_s"] (a dict the caller put there): wall time of a driver's pieces, each closed by a device synchronisation -- for
    the record of what is sharded (factorise, solve) and what every rank repeats (the rest), also with one rank.  Without that dict
    nothing is recorded and nothing synchronises."""

    def __init__(self, info):
        ph = info.get("phases_s") if info is not None else None
        self.ph = ph if isinstance(ph, dict) else None
        self.start()

    def start(self):
        self.t0 = time.perf_counter()

    def tick(self, name, block=None):
        """closes the piece `name`; block: the tensor the piece worked on (a CPU tensor needs no synchronisation)"""
        if self.ph is not None:
            if torch.cuda.is_available() and (block is None or block.is_cuda):
                torch.cuda.synchronize()
            self.ph[name] = self.ph.get(name, 0.0) + time.perf_counter() - self.t0
        self.start()


def _owned_nodes(ST):
    """(world, rank, comm) of the integrator type ST: rank r of `world` owns the nodes i = r (mod world).  comm: ST's DeviceComm if
    it carries one; otherwise torch.distributed's default group says who we are (and the exchange makes a DeviceComm on demand)"""
    sharded = getattr(ST, "sharded", False)
    comm = getattr(ST, "comm", None) if sharded else None
    if comm is not None:
        return comm.world, comm.rank, comm
    if sharded and dist.is_available() and dist.is_initialized():
        return dist.get_world_size(), dist.get_rank(), None
    return 1, 0, None


def _accumulate(S, X, c, Gi, ops):
    """S[j] += c Gi[j] X for the m moments (S is made on the first node)"""
    if S is None:
        S = torch.zeros((len(Gi),) + tuple(X.shape), dtype=CDT, device=X.device)
    for j in range(len(Gi)):
        ops.axpy(c * Gi[j], X, S[j])
    return S


_SOLVE_STREAMS = {}
NSTREAMS = 2    # measured on C4: 83.0 / 76.9 / 78-110 / 80.2 / 79.2 ms with 1 / 2 / 3 / 4 / 8 streams


def _solve_nodes_side_streams(f, t, mine, G, ops):
    """Node solves whose factors are all on the device already (the batched numeric LU): the solve of one node is a chain of ~15
    kernels that do not fill the chip (32 right-hand sides, 0.64 ms per node on gun), and the nodes are independent -- they go round
    robin onto NSTREAMS side streams, each result into its own block, and are accumulated on the caller's stream IN NODE ORDER (the
    sum is the same, to the bit, as with one stream)."""
    cur = torch.cuda.current_stream()
    sts = _SOLVE_STREAMS.setdefault(torch.cuda.current_device(), [])
    if len(sts) < NSTREAMS:
        # side streams from the cache the drivers share (_streams._eig_streams).  Streams MADE by this call were probed (once per
        # process and device, nep_stream_pair_serializes) to share a hardware queue with neither the caller's stream nor each other:
        # the runtime maps streams onto a small pool of queues in creation order, and two "concurrent" solve streams on ONE queue run
        # one after the other (21 instead of 13 ms for the 64 node solves of C4, depending on which streams the process happened
        # to create before).  Streams the cache held already -- iar's eig streams, after an iar call -- are handed out as they are:
        # they were probed against that call's streams, not against `cur`, and nothing is guaranteed about their queues.
        sts[:] = list(_eig_streams(NSTREAMS, others=(cur,)))
    for s_ in sts[:NSTREAMS]:
        s_.wait_stream(cur)
    pend = []
    for q, i in enumerate(mine):
        s_ = sts[q % NSTREAMS]
        with torch.cuda.stream(s_):
            X, c = f(t[i])
            ev = torch.cuda.Event(); ev.record(s_)
        pend.append((i, X, c, ev))
    S = None
    for i, X, c, ev in pend:
        cur.wait_event(ev)
        S = _accumulate(S, X, c, G[i], ops)
        X.record_stream(cur)
    return S


def _solve_nodes(f, t, mine, G, ops):
    """the plain node loop: solve and accumulate node by node on the caller's stream"""
    S = None
    for i in mine:
        X, c = f(t[i])
        S = _accumulate(S, X, c, G[i], ops)
    return S


def _exchange(ST, S, world, comm, ops):
    """the sum of the ranks' partial blocks, identical on every rank: (S, the DeviceComm used or None)"""
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
    return S, comm


def integrate_interval(ST, f, gv, a, b, N, info=None, ops=_DeviceOps):
    """returns S with S[j] ~ int f(t) g_j(t) dt  as a device tensor (m, k, n) (m = len(gv)).
    f(t) returns (X, c): the integrand value is c*X with X a device (k, n) block.
    `ops` exists so that the sharding / all-gather / fixed-order-sum logic can be exercised by the
    world_size-2 gloo test on CPU tensors; the drivers always use the HIP kernels."""
    h = (b - a) / N
    t = a + h * np.arange(N)
    G = np.array([[g(tt) for g in gv] for tt in t], dtype=np.complex128)    # N x m
    world, rank, comm = _owned_nodes(ST)
    mine = range(rank, N, world)
    phases = _Phases(info)
    if hasattr(f, "prefetch"):
        f.prefetch([t[i] for i in mine])
    phases.tick("factorise_nodes")
    ready = getattr(f, "ready", None)
    if ready and torch.cuda.is_available() and all(t[i] in ready for i in mine) and len(mine) > 1:
        S = _solve_nodes_side_streams(f, t, mine, G, ops)
    else:
        S = _solve_nodes(f, t, mine, G, ops)
    phases.tick("solve_nodes_and_accumulate", S)
    if S is None:
        raise ValueError("rank %d owns no quadrature node (N=%d < world size %d)" % (rank, N, world))
    S, comm = _exchange(ST, S, world, comm, ops)
    ops.scal(S, h)
    phases.tick("exchange_and_sum", S)
    if info is not None:
        info.update(world=world, rank=rank, nodes=len(mine))
        if comm is not None and getattr(comm, "last_exchange_s", None) is not None:
            info["exchange_s"] = float(comm.last_exchange_s)
    return S


def host_lu_strategy(creator, A):
    """keyword arguments of the host factorisation of A for `creator`: its own lu_kw, with the UMFPACK-like strategy (symmetric
    pattern + zero-free diagonal -> MMD_AT_PLUS_A in symmetric mode, else COLAMD) unless the creator names an ordering or a mode"""
    if creator.permc_spec is None and "symmetric_mode" not in creator.lu_kw:
        sym = _nep_hostlu.pattern_symmetric(sp.csc_matrix(A))
        return dict(creator.lu_kw, permc_spec="MMD_AT_PLUS_A" if sym else "COLAMD", symmetric_mode=bool(sym))
    return dict(creator.lu_kw, permc_spec=creator.permc_spec)


def _release_host_result(fut):
    """a host factorisation that finished but was never turned into a DeviceLU owns a shared-memory block nobody else will unlink
    (the worker handed ownership to this process): release it"""
    try:
        meta = fut.result()
        if isinstance(meta, dict) and "shm_name" in meta:
            _nep_hostlu.release_shm(_nep_hostlu.attach_shm(meta))
    except BaseException:
        pass


class _BeynTrace:
    """NEP_BEYN_TRACE=1: when the factorisations of one prefetch were submitted and finished, printed as the nodes are consumed"""

    def __init__(self):
        self.on = env_flag("NEP_BEYN_TRACE")
        self.t0 = time.perf_counter()
        self.host_done = []; self.host_meta = []
        self.t_submitted = 0.0

    def _ms(self):
        return 1e3 * (time.perf_counter() - self.t0)

    def device_batch(self, ndev, nall):
        if self.on:
            print("[beyn trace] %d of %d nodes factorised on the device (batched) at %.0f ms" % (ndev, nall, self._ms()), flush=True)

    def _host_finished(self, fut):
        self.host_done.append(time.perf_counter() - self.t0)
        self.host_meta.append(fut.result() if not fut.exception() else {})

    def host_submitted(self, fut):
        if self.on:
            fut.add_done_callback(self._host_finished)

    def all_submitted(self):
        self.t_submitted = time.perf_counter() - self.t0

    def last_solve_issued(self):
        if not self.on:
            return
        hd = sorted(self.host_done)
        mt_ = [m_ for m_ in self.host_meta if "t_worker" in m_]
        if mt_:
            print("[beyn trace] per factorisation in the worker: splu %.1f ms, factor() %.1f ms, whole task %.1f ms (means over %d)"
                  % (1e3 * np.mean([m_["t_factor"] for m_ in mt_]), 1e3 * np.mean([m_["t_worker_factor_call"] for m_ in mt_]),
                     1e3 * np.mean([m_["t_worker"] for m_ in mt_]), len(mt_)), flush=True)
        print("[beyn trace] submitted all at %.0f ms; host factorisations done: first %.0f ms, half %.0f ms, last %.0f ms; "
              "last block solve issued at %.0f ms" % (1e3 * self.t_submitted, 1e3 * hd[0], 1e3 * hd[len(hd) // 2], 1e3 * hd[-1],
                                                      self._ms()), flush=True)


class _BatchedMder:
    """the NEP as the node solvers see it once the matrices of all nodes have come from ONE compute_Mder_batch call (a NEP type that
    evaluates M on the device for a batch of shifts: PeriodicDDE_NEP, BEM_NEP): compute_Mder(lam) of a node hands out its matrix,
    everything else is the NEP's own"""

    BATCH_WORDS = 1 << 26      # complex words of one batch (1 GiB): more nodes than that take several calls

    def __init__(self, nep, shifts):
        self._nep = nep
        n = nep.size(1)
        step = max(1, self.BATCH_WORDS // (n * n))
        self._mats = {}
        for j0 in range(0, len(shifts), step):
            part = [complex(z) for z in shifts[j0:j0 + step]]
            self._mats.update(zip(part, nep.compute_Mder_batch(part)))

    def __getattr__(self, name):
        return getattr(self._nep, name)

    def compute_Mder(self, lam, i=0):
        M = self._mats.pop(complex(lam), None) if i == 0 else None       # (each node is factorised once)
        return self._nep.compute_Mder(lam, i) if M is None else M


class _NodeSolve:
    """f(t) = Tv(g(t)) * weight(t), Tv(lam) = lin_solve(create_linsolver(creator, nep, lam+sigma), Vh)
    (method_beyncontour.jl:89-98, method_block_SS.jl:81-86,129-132).  With the default BackslashLinSolverCreator every
    node needs a NEW factorisation; `prefetch` factorises all nodes of this rank at once on the device where the pattern has a
    plan, and otherwise starts their host factorisations in worker processes so that they run concurrently with each other and
    with the device solves of the nodes already factored."""

    BUILDERS = 4   # threads turning host factors into device schedules (nep_lu_create releases the GIL)
    AHEAD = 8      # device factorisations built (or being built) ahead of the node being solved

    def __init__(self, nep, linsolvercreator, sigma, g, Vd, weight):
        self.nep, self.creator, self.sigma, self.g, self.Vd, self.weight = nep, linsolvercreator, sigma, g, Vd, weight
        self.ready = {}       # t -> DeviceLU factorised on the device (or the first node of a cold call)
        self.host = {}        # t -> future of the host factorisation (worker process)
        self.built = {}       # t -> future of the DeviceLU (builder thread)
        self.order = []
        self.next = 0
        self.pool = None
        self.trace = None     # made by prefetch; without one (early return there) ready / built stay empty and no path below asks for it
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
        """device batch, cold first node, or host pool: where the nodes ts are factorised"""
        c = self.creator
        if (not isinstance(self.nep, _BatchedMder) and hasattr(self.nep, "compute_Mder_dev") and hasattr(self.nep, "compute_Mder_batch")
                and len(ts) >= 1):
            self.nep = _BatchedMder(self.nep, [self.g(t) + self.sigma for t in ts])      # M of every node from one device pass
        if not isinstance(c, BackslashLinSolverCreator) or getattr(c, "workers", None) == 0 or len(ts) < 2:
            return
        self.pool = ThreadPoolExecutor(max_workers=self.BUILDERS)
        self.trace = _BeynTrace()
        self.ready = {}
        route = None
        if c.permc_spec is None and not c.lu_kw and not env_flag("NEP_BEYN_HOST_LU"):
            route = terms_route(self.nep)
        if route is not None and route.plan is None and len(ts) >= 4 and env_str("NEP_BEYN_COLD_PLAN", "1") != "0":
            route = self._cold_first_node(ts[0]) or route
        if route is not None and route.plan is None:
            self._pattern = route.pattern               # (the first host factorisation that comes back seeds the plan)
        self._submit_host(self._factor_on_device(route, ts))

    def _factor_on_device(self, route, ts):
        """all nodes on the GPU in one pass when the pattern has a device-factorisation plan (_devicelu._DeviceRefactor): M(lam_b) =
        sum_t f_t(lam_b) A_t, only the B x m_t coefficients travel, one batched numeric LU (every launch carries all nodes).  Fills
        `ready`; returns the nodes left for the host: those whose factorisation is refused with the stored pivot sequence, or all"""
        if route is None or route.plan is None:
            return list(ts)
        tsb = [t for t in ts if t not in self.ready]       # (the first node of a cold call keeps its host factors)
        fv = self.nep.get_fv()
        Cf = np.array([[f.derivs(self.g(t) + self.sigma, 1)[0] for f in fv] for t in tsb], dtype=np.complex128)
        lus = factor_term_rows(route, Cf, expected_solves=1, growth=GROWTH_UNREFINED)
        self.ready.update((t, lu) for t, lu in zip(tsb, lus) if lu is not None)
        self.trace.device_batch(len(self.ready), len(ts))
        return [t for t, lu in zip(tsb, lus) if lu is None]

    def _cold_first_node(self, t0):
        """FIRST call on this sparsity pattern: instead of sending all N nodes to the host-factorisation worker pool (gun, N = 64:
        0.67 s for the call, most of it the pool's start-up and 64 SuperLU runs) the first node is factorised on the host in this
        process, its device-LU plan is built right away (enumeration on the GPU, ~25 ms) and waited for, and the other N - 1 nodes
        take the batched device factorisation like every later call.  Returns the route with its plan, the node in `ready`; None
        where that did not work (singular node, refused plan ...: the host route handles every node)"""
        try:
            lu = DeviceLU(self.nep.compute_Mder(self.g(t0) + self.sigma), expected_solves=1)
            _DeviceRefactor.wait()
            route = terms_route(self.nep)
        except Exception:
            return None
        if route is None or route.plan is None:
            return None
        self.ready[t0] = lu
        return route

    def _submit_host(self, ts):
        """host factorisations of the nodes ts in the worker pool, their uploads in the builder threads"""
        self.order = list(ts)
        kw = None
        for t in ts:
            A = self.nep.compute_Mder(self.g(t) + self.sigma)
            if kw is None:
                kw = host_lu_strategy(self.creator, A)         # decided ONCE: all nodes share one pattern
            self.host[t] = HostLUPool.submit(A, workers=getattr(self.creator, "workers", None), **kw)
            self.trace.host_submitted(self.host[t])
        self.trace.all_submitted()
        self._submit_builds()

    def close(self):
        if self.pool is not None:
            for f in list(self.built.values()) + list(self.host.values()):
                f.cancel()
            self.pool.shutdown(wait=True)
            self.pool = None
            for f in self.host.values():               # (finished, or still finishing)
                if f.done():
                    _release_host_result(f)
                else:
                    f.add_done_callback(_release_host_result)
            self.built.clear(); self.host.clear()

    def __call__(self, t):
        if t in self.ready:
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
                self.trace.last_solve_issued()
                self.close()
            return X, self.weight(t)
        M0inv = create_linsolver(self.creator, self.nep, self.g(t) + self.sigma)
        return lin_solve(M0inv, self.Vd), self.weight(t)


def _beyn_tail_device(S, n, k):
    """the device part of Beyn's dense tail.  The moments stay on the device (method_beyncontour.jl:114-128 needs only k x k pieces of
    them on the host): A0 = Q R by column-wise DGKS on the device (K6; the columns A0 has beyond its rank become orthonormalised noise,
    R shows the rank), svd(R) on the host (k x k) gives the singular values of A0 and V = Q U_R; B = V0^H A1 W0 S^-1 = U_R^H (Q^H A1) W0
    S^-1 with the k x k Gram block Q^H A1 from the device; the eigenvectors V0 VB = Q (U_R VB) by K7.  Downloaded: two k x (k + 2) blocks
    instead of two n x k ones; the n x k SVD (9 ms of host LAPACK on gun, repeated by every rank) is gone.
    S: device (2, k, n) block of the UNSCALED moments (A_j = S[j] / (2 pi i)).  Returns (oh, G, Q): the k x (k + 2) rows
    nep_orth_qr_dev wrote (row j: R[:j, j], the real R[j, j], the flags of column j in the imaginary part of entry j + 1), the k x k
    Gram block Q^H S[1] (host), Q as a device (k, n) tensor."""
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
    bh = buf[:k * (k + 2) + k * k].cpu().numpy()
    return bh[:k * (k + 2)].reshape(k, k + 2), bh[k * (k + 2):].reshape(k, k).T, Qd            # (Gd[c, r] = G[r, c])


def beyn_tail_from_qr(oh, G, rank_drop_tol):
    """host part of the device tail: (singular values of A0, rank p, B (p x p), U_R[:, :p]) from the rows `oh` of the device QR of
    the unscaled A0 and G = Q^H (unscaled A1); the eigenvector basis is V0 = Q U_R[:, :p].  None when the QR cannot be trusted (the
    caller then takes the host route)."""
    k = oh.shape[0]
    flags = [int(oh[j, j + 1].imag) for j in range(k)]
    if any(f & 2 for f in flags):                           # breakdown flag (||w|| = 0 or not finite)
        return None
    R = np.zeros((k, k), dtype=np.complex128)
    for j in range(k):
        R[:j, j] = oh[j, :j]
        R[j, j] = oh[j, j].real
    # svd(R) = svd(A0) and V = Q U_R hold for an ORTHONORMAL Q only.  A column whose last enqueued DGKS pass still met the
    # re-orthogonalisation criterion (flag bit 0) is not known to be orthogonal to its predecessors: harmless for a noise column (A0 is
    # rank deficient by design: R[j, j] at round-off of R[0, 0]), not for one that carries weight -- the host route then (svd of the
    # downloaded block, as the reference does it)
    r00 = abs(R[0, 0]) if k else 0.0
    if any((flags[j] & 1) and abs(R[j, j]) > 1e-10 * r00 for j in range(k)):
        return None
    c = 1.0 / (2j * np.pi)
    Ur, Sv, Wh = sla.svd(R * c)                             # A0 = Q (R / (2 pi i)): same singular values, V = Q U_R
    p = int(np.sum(Sv / Sv[0] > rank_drop_tol))
    W0 = Wh.conj().T[:, :p]
    UrP = Ur[:, :p]
    B = (UrP.conj().T @ (G * c) @ W0) @ np.diag(1.0 / Sv[:p])
    return Sv, p, B, UrP


def beyn_tail_host(A0, A1, rank_drop_tol):
    """the reference's tail (method_beyncontour.jl:114-128) on the downloaded moments: (singular values of A0, rank p, B, V0)"""
    V, Sv, Wh = sla.svd(A0, full_matrices=False)
    W = Wh.conj().T
    p = int(np.sum(Sv / Sv[0] > rank_drop_tol))
    V0 = V[:, :p]; W0 = W[:, :p]
    B = (V0.conj().T @ A1 @ W0) @ np.diag(1.0 / Sv[:p])
    return Sv, p, B, V0


def select_eigenpairs(lam, errs, tol, sigma, radius, neigs):
    """indices of the pairs contour_beyn returns, in its order: those with errs < tol, nearest to sigma first, those inside the
    ellipse (semi-axes `radius` around sigma) before the others, at most neigs.  errs None (sanity_check=False): all, in that order."""
    good = np.arange(len(lam)) if errs is None else np.nonzero(errs < tol)[0]
    sgi = good[np.argsort(abs(sigma - lam[good]), kind="stable")]
    d = lam[sgi] - sigma
    inside = (d.real / radius[0]) ** 2 + (d.imag / radius[1]) ** 2 <= 1
    sel = sgi[np.argsort(~inside, kind="stable")]
    if errs is not None and len(sel) > neigs:
        sel = sel[:neigs]
    return sel


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
    phases = _Phases(info)
    if Vh is None:
        Vh = probe_block(n, k)
    Vd = to_dev(Vh)
    phases.tick("probe_generate_and_upload")

    f = _NodeSolve(nep, linsolvercreator, sigma, g, Vd, gp)
    S = integrate_interval(MIntegrator, f, [lambda s: 1.0 + 0j, g], 0.0, 2 * np.pi, N, info=info)
    phases.start()
    A0 = A1 = tail = Qd = None
    if S.is_cuda and k >= 2 and env_str("NEP_BEYN_DEVICE_TAIL", "1") != "0":
        oh, G, Qd = _beyn_tail_device(S, n, k)
        tail = beyn_tail_from_qr(oh, G, rank_drop_tol)
    if tail is None:
        Qd = None
        A0 = to_host(S[0]) / (2j * np.pi)
        A1 = to_host(S[1]) / (2j * np.pi)
        phases.tick("moments_download")
        tail = beyn_tail_host(A0, A1, rank_drop_tol)
    Sv, p, B, U = tail
    lam, VB = sla.eig(B)
    lam = lam + sigma
    phases.tick("svd_and_eig_host")
    # eigenvectors V0 VB on the device (K7), (n, p) row-major: V0 = Q U_R[:, :p] after the device tail, the uploaded V0 otherwise
    QT = dense.gemm_ts(Qd, U @ VB, rowmajor=True) if Qd is not None else dense.gemm_ts(to_dev(U), VB, rowmajor=True)
    phases.tick("eigenvectors")
    if Qd is not None and info is not None and info.get("moments", True):      # (a caller that wants them; bench.py's timed call opts out)
        A0 = to_host(S[0]) / (2j * np.pi); A1 = to_host(S[1]) / (2j * np.pi)
    if info is not None:
        info.update(p=p, S=Sv, A0=A0, A1=A1)
    errs = None
    if sanity_check:
        errs = estimate_errors(errmeasure, lam, QT)
        phases.tick("residual_filter")
        if info is not None:
            info.update(errs=errs)
    sel = select_eigenpairs(lam, errs, tol, sigma, radius, neigs)
    Q = to_host(dense.rowmajor_to_cols(QT, np.asarray(sel, dtype=np.int32)))
    return lam[sel], (Q / np.linalg.norm(Q, axis=0)[None, :] if Q.shape[1] else Q)


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
