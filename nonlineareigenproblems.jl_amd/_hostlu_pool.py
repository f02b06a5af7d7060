"""The torch-free host-LU worker module and the spawn-safe process pool that runs it (SciPy's SuperLU)."""
import atexit
import os
import sys

import numpy as np
import scipy.sparse as sp

from ._env import env_int, env_str

# the torch-free worker module lives alone in _workers/ under a unique top-level name: only that directory goes on
# sys.path (spawned workers import it by name), so no module of this package can shadow a user's `build`, `nep`, ...
_WORKERS_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "_workers")
if _WORKERS_DIR not in sys.path:
    sys.path.insert(0, _WORKERS_DIR)
import nep_amd_hostlu as _nep_hostlu  # noqa: E402


class HostLUPool:
    """process pool for concurrent host factorisations (SciPy's splu holds the GIL).  Workers are spawned (never forked
    from a process with a live HIP context) and import only NumPy/SciPy."""
    _pool = None
    _workers = 0

    @classmethod
    def get(cls, workers=None):
        if workers is None and cls._pool is not None:
            return cls._pool                    # whatever size it was started with
        if workers is None:
            from ._affinity import cpu_budget
            workers = env_int("NEP_HOSTLU_WORKERS", min(16, max(1, cpu_budget() - 2)))
        if cls._pool is None or cls._workers != workers:
            cls.shutdown()
            import multiprocessing as mp
            from concurrent.futures import ProcessPoolExecutor
            # SuperLU is sequential: one BLAS thread per worker (the children read these variables when they load
            # NumPy; 16 workers x 64 spinning OpenBLAS threads made a factorisation 10x slower)
            keys = ("OPENBLAS_NUM_THREADS", "OMP_NUM_THREADS", "MKL_NUM_THREADS")
            saved = {k: os.environ.get(k) for k in keys}
            for k in keys:
                os.environ[k] = "1"
            # spawn re-imports the parent's __main__ in every child (multiprocessing.spawn.get_preparation_data); a user
            # script without an `if __name__ == "__main__":` guard would run again inside each worker.  The workers only
            # need _nep_hostlu (importable by name), so __main__ is hidden from the preparation data while they start.
            main = sys.modules.get("__main__")
            hidden = {}
            for attr in ("__file__", "__spec__"):
                if main is not None and getattr(main, attr, None) is not None:
                    hidden[attr] = getattr(main, attr)
                    try:
                        setattr(main, attr, None)
                    except Exception:
                        hidden.pop(attr)
            try:
                ctx = mp.get_context("spawn")
                # one physical core per worker, taken from the END of the allowed set (the launching thread, the eig and
                # builder threads of this process stay on the first cores); NEP_HOSTLU_PIN=0 leaves placement to the scheduler
                cores = _nep_hostlu.physical_cores() if env_str("NEP_HOSTLU_PIN", "1") != "0" else []
                cores = cores[::-1][:max(workers, 1)] if len(cores) >= 2 * workers else []
                cls._pool = ProcessPoolExecutor(max_workers=workers, mp_context=ctx, initializer=_nep_hostlu.pin_worker,
                                                initargs=(ctx.Value("i", 0), cores))
                cls._workers = workers
                list(cls._pool.map(_nep_hostlu.ping, range(4 * workers)))     # forces all workers to start now
            finally:
                for attr, val in hidden.items():
                    setattr(main, attr, val)
                for k_, v_ in saved.items():
                    if v_ is None:
                        os.environ.pop(k_, None)
                    else:
                        os.environ[k_] = v_
        return cls._pool

    @classmethod
    def shutdown(cls):
        if cls._pool is not None:
            cls._pool.shutdown(wait=False, cancel_futures=True)
            cls._pool = None

    @classmethod
    def warm(cls, workers=None):
        """start the workers and wait until each has imported SciPy (keeps the start-up out of timed regions)"""
        cls.get(workers)

    @classmethod
    def submit(cls, A, workers=None, **kw):
        """future of the factor METADATA; the arrays sit in a shared-memory block: DeviceLU(factors=meta) maps, uploads
        and unlinks it; a result that is never consumed must be released by its holder (contour._NodeSolve.close does)"""
        Ac = sp.csc_matrix(A, dtype=np.complex128)
        # `workers` (BackslashLinSolverCreator(workers=N)) sizes the pool when it has to be started; a running pool is kept
        pool = cls._pool if cls._pool is not None else cls.get(workers)
        return pool.submit(_nep_hostlu.factor_shm, Ac.data, Ac.indices, Ac.indptr, Ac.shape, **kw)


atexit.register(HostLUPool.shutdown)
