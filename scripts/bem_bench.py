"""Times of the nep_bem kernels (csrc/bem.hip) on the device at n = 96, 2400 and 9600, and of a NumPy evaluation of the same
assembly on the host at n = 2400.

Every figure is the time per call of a window of `reps` calls between two device events, after one warm-up call; the window is
repeated REPEATS times and (min, median, max) over the windows is recorded.  The mlincomb and resid windows go through
BEM_NEP._mlincomb / the raw entry point, so they contain the host side of a call (argument marshalling, one launch).
Prints one JSON line per size; an argument names a file for the whole record (profiles/bem.json).  Needs a GPU."""
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
LAM = 8.79 - 0.0108j
CDT = torch.complex128


def window(fn, reps):
    """milliseconds per call of `reps` calls between two device events"""
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


def assemble(nep, lams, buf, der=0):
    la = np.ascontiguousarray(lams, dtype=np.complex128)
    n = nep.n
    rc = lib.nep_bem_assemble(nep.h, len(la), hptr(la), der, c_vp(buf.data_ptr()), n, n * n, stream_ptr())
    assert rc == 0, rc


def resid(nep, la, Q, Y):
    n = nep.n
    rc = lib.nep_bem_resid(nep.h, len(la), hptr(la), c_vp(Q.data_ptr()), n, c_vp(Y.data_ptr()), n, stream_ptr())
    assert rc == 0, rc


def bench_size(N, rng):
    t0 = time.perf_counter()
    nep = na.nep_gallery("bem_fichera", N)
    torch.cuda.synchronize()
    n = nep.size(1)
    res = {"create_s": time.perf_counter() - t0}
    # windows of at least a few milliseconds at every size
    reps = 2000 if n <= 96 else (40 if n <= 2400 else 4)
    lams20 = [LAM + 0.1 * i for i in range(20)]
    la10 = np.ascontiguousarray(lams20[:10], dtype=np.complex128)
    a50 = 1.0 / np.cumprod(np.arange(1, 51, dtype=float))
    one = np.ones(1)
    buf1 = torch.empty((1, n, n), dtype=CDT, device="cuda")
    buf20 = torch.empty((20, n, n), dtype=CDT, device="cuda")
    V = na.to_dev(rng.standard_normal((n, 50)) + 1j * rng.standard_normal((n, 50)))
    z = torch.empty(n, dtype=CDT, device="cuda")
    Y = torch.empty((10, n), dtype=CDT, device="cuda")
    res["assemble_1"] = timed(lambda: assemble(nep, [LAM], buf1), reps)
    res["assemble_1_real_lam"] = timed(lambda: assemble(nep, [LAM.real], buf1), reps)
    res["assemble_20"] = timed(lambda: assemble(nep, lams20, buf20), max(1, reps // 4))
    res["mlincomb_k1"] = timed(lambda: nep._mlincomb(LAM, 1, one, 0, V, n, z), reps)
    res["mlincomb_k50"] = timed(lambda: nep._mlincomb(LAM, 50, a50, 1, V, n, z), reps)
    res["resid_k10"] = timed(lambda: resid(nep, la10, V, Y), reps)
    # the results at the timed size: the matrix-free product against the assembled matrix
    assemble(nep, [LAM], buf1)
    zz = nep._mlincomb(LAM, 1, one, 0, V, n, z)
    ref = buf1[0] @ V[0]
    res["mlincomb_vs_assembled_rel"] = float((zz - ref).abs().max() / ref.abs().max())
    return n, res


def numpy_assemble(N):
    """the lam part of M(LAM) for the upper triangle in NumPy float64 (mesh and Gauss points from the product, on the host):
    seconds for the distances and weights, and for the exponentials and sums"""
    mesh = na.gen_ficheramesh(N)
    c = np.array([[2 / 3, 1 / 6, 1 / 6], [1 / 6, 2 / 3, 1 / 6], [1 / 6, 1 / 6, 2 / 3]])
    g = np.einsum("iv,tvx->tix", c, mesh.vert)
    w = np.repeat((mesh.area / 3)[:, None], 3, axis=1)
    t0 = time.perf_counter()
    r, cc = np.triu_indices(len(mesh))
    diff = g[r][:, :, None, :] - g[cc][:, None, :, :]
    d = np.sqrt(np.sum(diff * diff, axis=-1))
    W = w[r][:, :, None] * w[cc][:, None, :]
    zero = d == 0
    d1 = np.where(zero, 1.0, d)
    t1 = time.perf_counter()
    E = np.where(zero, 1j * LAM, np.exp(-LAM.imag * d) * (np.cos(LAM.real * d) + 1j * np.sin(LAM.real * d)) - 1)
    L = np.sum(E * (W / d1), axis=(1, 2)) / (4 * np.pi)
    t2 = time.perf_counter()
    assert np.all(np.isfinite(L))
    return {"pairs_s": t1 - t0, "assemble_s": t2 - t1}


def main():
    out = {}
    rng = np.random.default_rng(0)
    for N in (2, 10, 20):
        n, res = bench_size(N, rng)
        out[str(n)] = res
        print(n, json.dumps(res), flush=True)
        torch.cuda.empty_cache()
    out["numpy_n2400"] = numpy_assemble(10)
    print(json.dumps(out["numpy_n2400"]))
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
