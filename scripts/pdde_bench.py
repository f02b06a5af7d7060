"""Times of nep_pdde_mder (csrc/pdde.hip, K15) on the device: "rand0" (n = 200, N = 1000) for 1, 8 and 64 shifts at der = 0 and 64
shifts at der = 1, "mathieu" (n = 2, N = 1000) for 1 shift; and of the reference's route restated in NumPy on the host (one matrix at
a time: the matrix ODE with Y(0) = I in complex128, zgemm for the products) for one shift of rand0: the median of NUMPY_RUNS
runs after a warm-up run, with the number of threads the BLAS reports.

Every device figure is the time per call of a window of `reps` calls between two device events, after one warm-up call; the window
is repeated REPEATS times and (min, median, max) over the windows is recorded.  The FP64 rate counts 8 flops per complex
multiply-add of the two products of a stage, 2 x 8 n^2 flops per column, stage and step; the traffic estimate is the term matrices read
once per tile and stage.  Prints one JSON line per figure; an argument names a file for the whole record.  Needs a GPU."""
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import nep_amd as na                                              # noqa: E402
from nep_amd._lib import lib, hptr, c_vp                          # noqa: E402
from nep_amd.nep import stream_ptr                                # noqa: E402

REPEATS = 5
NUMPY_RUNS = 3
CDT = torch.complex128


def blas_threads():
    """the threads NumPy's BLAS really uses (threadpoolctl), or None where that cannot be asked"""
    try:
        from threadpoolctl import threadpool_info
        return max((p.get("num_threads", 0) for p in threadpool_info() if p.get("user_api") == "blas"), default=None)
    except ImportError:
        return None


def window(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    t = sorted(window(fn, reps) for _ in range(REPEATS))
    return {"min_ms": t[0], "median_ms": t[REPEATS // 2], "max_ms": t[-1], "reps": reps}


def mder(nep, lams, der, buf):
    la = np.ascontiguousarray(lams, dtype=np.complex128)
    n = nep.n
    rc = lib.nep_pdde_mder(nep._handle(), len(la), hptr(la), der, c_vp(buf.data_ptr()), n, n * n, stream_ptr())
    assert rc == 0, rc


def tile_width(n, p, nsys):
    """the systems per tile pdde.hip picks (pdde_dispatch)"""
    for g in (8, 4, 2, 1):
        if g * p <= 8 and -(-nsys // g) >= 256:
            return g
    return 1


def figures(nep, nlam, der, t_ms):
    n, N, p = nep.n, nep.N, der + 1
    cols = nlam * n * p
    flops = cols * 4.0 * N * 2 * 8 * n * n
    g = tile_width(n, p, nlam * n)
    tiles = -(-nlam * n // g)
    terms = len(nep.A_terms) + len(nep.B_terms)
    traffic = tiles * 4.0 * N * terms * n * n * 16
    return {"tflops": flops / (t_ms * 1e-3) / 1e12, "tile_systems": g, "tiles": tiles, "term_bytes_read_TB": traffic / 1e12,
            "term_read_TB_per_s": traffic / (t_ms * 1e-3) / 1e12}


def numpy_mder(nep, lam):
    """M(lam) by the reference's route: compute_MM(lam, I) with ode_rk4 (periodic_dde.jl:112-124, 203-218), complex128"""
    n, N, tau = nep.n, nep.N, nep.tau
    h = tau / N
    e = np.exp(-tau * lam)
    A = lambda s: np.tensordot(nep.alpha[s], nep.A_terms, 1)
    B = lambda s: np.tensordot(nep.beta[s], nep.B_terms, 1)
    F = lambda s, Y: h * (A(s) @ Y + (B(s) @ Y) * e - Y * lam)
    Y0 = np.eye(n, dtype=np.complex128)
    Y = Y0.copy()
    for k in range(N):
        s1 = F(2 * k, Y); s2 = F(2 * k + 1, Y + s1 / 2); s3 = F(2 * k + 1, Y + s2 / 2); s4 = F(2 * k + 2, Y + s3)
        Y = Y + (s1 + 2 * s2 + 2 * s3 + s4) / 6
    return Y - Y0


def main():
    out = {}
    rand0 = na.nep_gallery("periodicdde", name="rand0")
    n = rand0.n
    lams = [complex(0.2 + 0.05 * i, 0.5 + 0.03 * i) for i in range(64)]
    buf = torch.empty((64, n, n), dtype=CDT, device="cuda")
    for nlam, der, reps in ((1, 0, 3), (8, 0, 2), (64, 0, 1), (64, 1, 1)):
        r = timed(lambda: mder(rand0, lams[:nlam], der, buf), reps)
        r.update(figures(rand0, nlam, der, r["median_ms"]))
        out["rand0_%d_shifts_der%d" % (nlam, der)] = r
        print("rand0 %d shifts der %d" % (nlam, der), json.dumps(r), flush=True)
    mathieu = na.nep_gallery("periodicdde", name="mathieu")
    b2 = torch.empty((1, 2, 2), dtype=CDT, device="cuda")
    out["mathieu_1_shift"] = timed(lambda: mder(mathieu, [-0.2], 0, b2), 5)
    print("mathieu 1 shift", json.dumps(out["mathieu_1_shift"]), flush=True)
    Mn = numpy_mder(rand0, lams[0])                                  # warm-up (thread pool, page faults)
    runs = []
    for _ in range(NUMPY_RUNS):
        t0 = time.perf_counter()
        Mn = numpy_mder(rand0, lams[0])
        runs.append(time.perf_counter() - t0)
    runs.sort()
    t_np = runs[NUMPY_RUNS // 2]
    mder(rand0, lams[:1], 0, buf)
    torch.cuda.synchronize()
    Md = buf[0].cpu().numpy().T
    out["numpy_rand0_1_shift"] = {"seconds": t_np, "min_s": runs[0], "max_s": runs[-1], "runs": NUMPY_RUNS, "blas_threads": blas_threads(),
                                  "device_vs_numpy_rel": float(np.max(np.abs(Md - Mn)) / np.max(np.abs(Mn)))}
    out["speedup_64_shifts"] = 64 * t_np / (out["rand0_64_shifts_der0"]["median_ms"] * 1e-3)
    print("numpy", json.dumps(out["numpy_rand0_1_shift"]), "64 x numpy / device:", out["speedup_64_shifts"], flush=True)
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
