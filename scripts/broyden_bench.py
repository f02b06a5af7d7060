"""The fused T-sweep of broyden against the same work composed from the plain dense GEMM, and one deflation level at gun size.

    python scripts/broyden_bench.py [--out profiles/broyden.json] [--sizes 9956 20000] [--reps 20] [--level-n 9956] [--level-maxit 200]

  sweep      nep_broyden_sweep on an n x n complex128 T (ldt = n), with the pending update (T += u0 a0, y = T x, g = w^H T: 32 n^2
             bytes of T traffic) and without it (16 n^2 bytes).  `reps` calls are enqueued back to back and the stream is
             synchronised once; the time per call is reported with GB/s of T traffic and the fraction of 6.3 TB/s.
  composed   the four passes of src/method_broyden.jl:69,101,107,117 from the entry points of the commit before the kernel: two
             nep_zgemm matrix-vector products (T rk, T ztilde), one conjugate-transposed product (dv^H T) and a rank-one
             nep_zgemm (T += Tztilde aH): 80 n^2 bytes.  By traffic the ratio composed / sweep-with-update should approach 2.5.
  The routes alternate in three rounds; the median is reported with all rounds.
  level      broyden(dep0_sparse(level_n, p), "eye", pmax=1, eigmethod="invpow", maxit=level_maxit): host clock around the call,
             ms per inner iteration, split into the sweep (the time measured above at that n), K1 (one nep_mlincomb call timed
             the same way) and the rest (host scalars, synchronisations, the small device updates).  The gallery's generator
             draws every entry in a Python loop, so the density p is chosen to give about the gun problem's number of entries;
             convergence at this size is not claimed, the number of iterations run is reported."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import importlib                                                       # noqa: E402

import nep_amd as na                                                   # noqa: E402
from nep_amd._lib import lib, check, c_vp, cd                          # noqa: E402
from nep_amd.nep import CDT, stream_ptr                                # noqa: E402

bro = importlib.import_module("nep_amd.broyden")
PEAK = 6.3e12


def timed(f, reps):
    f()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        f()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps


def sweep_rows(n, reps):
    g = torch.Generator(device="cuda").manual_seed(n)
    rnd = lambda *s: torch.complex(torch.randn(*s, generator=g, device="cuda", dtype=torch.float64),
                                   torch.randn(*s, generator=g, device="cuda", dtype=torch.float64))
    T = rnd(n, n) / n
    u0, a0 = rnd(n) * 1e-6, rnd(n) * 1e-6                                # small: reps updates do not change the scale of T
    x, w, rk = rnd(n), rnd(n), rnd(n)
    y, gg, y2 = (torch.empty(n, dtype=CDT, device="cuda") for _ in range(3))
    work = torch.empty(bro.sweep_worksize(n), dtype=CDT, device="cuda")
    one, zero = cd(1.0), cd(0.0)
    p = lambda t: c_vp(t.data_ptr())

    def with_update():
        bro.sweep(T, n, work, u0=u0, a0=a0, x=x, y=y, w=w, g=gg)

    def without_update():
        bro.sweep(T, n, work, x=x, y=y, w=w, g=gg)

    def composed():
        check(lib.nep_zgemm(0, 0, n, 1, n, one, p(T), n, p(rk), n, zero, p(y2), n, stream_ptr()))
        check(lib.nep_zgemm(0, 0, n, 1, n, one, p(T), n, p(x), n, zero, p(y), n, stream_ptr()))
        check(lib.nep_zgemm(2, 0, 1, n, n, one, p(w), n, p(T), n, zero, p(gg), 1, stream_ptr()))
        check(lib.nep_zgemm(0, 0, n, n, 1, one, p(u0), n, p(a0), 1, one, p(T), n, stream_ptr()))

    # the two routes agree: T x and w^H T of the same T
    without_update(); torch.cuda.synchronize(); ys, gs = y.clone(), gg.clone()
    check(lib.nep_zgemm(0, 0, n, 1, n, one, p(T), n, p(x), n, zero, p(y), n, stream_ptr()))
    check(lib.nep_zgemm(2, 0, 1, n, n, one, p(w), n, p(T), n, zero, p(gg), 1, stream_ptr()))
    torch.cuda.synchronize()
    diff = float(max((ys - y).norm() / y.norm(), (gs - gg).norm() / gg.norm()))
    routes = {"sweep_with_update": (with_update, reps, 32), "sweep_without_update": (without_update, reps, 16),
              "composed_four_passes": (composed, max(2, reps // 4), 80)}
    acc = {k: [] for k in routes}
    for _ in range(3):
        for k, (f, r, _) in routes.items():
            acc[k].append(timed(f, r))
    row = dict(n=n, t_gbytes=16.0 * n * n / 1e9, sweep_vs_zgemm_rel_diff=diff)
    for k, (_, _, bpe) in routes.items():
        s = float(np.median(acc[k]))
        row[k] = dict(seconds=s, rounds=[float(v) for v in acc[k]], gb_per_s=bpe * n * n / s / 1e9, fraction_of_6_3_tb_s=bpe * n * n / s / PEAK)
    row["ratio_composed_over_sweep_with_update"] = row["composed_four_passes"]["seconds"] / row["sweep_with_update"]["seconds"]
    return row


def level_row(n, maxit, sweep_s, reps):
    p = min(0.25, 100000.0 / (float(n) * n))
    nep = na.nep_gallery("dep0_sparse", n, p)
    info = {}
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    S, X, T1, eh, th, ih = na.broyden(nep, "eye", pmax=1, eigmethod="invpow", maxit=maxit, info=info)
    torch.cuda.synchronize()
    t_call = time.perf_counter() - t0
    it = sum(info["iters"])
    inner = float(th[np.isfinite(th)][-1] - th[np.isfinite(th)][0]) / max(it - 10, 1) if np.isfinite(th).sum() > 1 else float("nan")
    v = torch.ones((1, n), dtype=CDT, device="cuda"); z = torch.empty(n, dtype=CDT, device="cuda")
    Cm = nep.coeff_block(0.1 + 0.2j, np.ones(1))
    k1 = timed(lambda: nep.dev.mlincomb(Cm, v, z), reps)
    return dict(n=n, density=p, nnz=[int(A.nnz) for A in nep.A], iterations=it, converged=bool(np.nanmin(eh) < 1e-12),
                last_error=float(eh[np.isfinite(eh)][-1]), call_s=t_call, per_iteration_ms=inner * 1e3,
                sweep_ms=sweep_s * 1e3, k1_ms=k1 * 1e3, rest_ms=(inner - sweep_s - k1) * 1e3,
                syncs_per_iteration=info["syncs_per_iteration"], t_bytes=info["t_bytes"], setup_passes=info["setup_passes"])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "broyden.json"))
    ap.add_argument("--sizes", type=int, nargs="*", default=[9956, 20000])
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--level-n", type=int, default=9956)
    ap.add_argument("--level-maxit", type=int, default=200)
    a_ = ap.parse_args()
    rows = []
    for n in a_.sizes:
        rows.append(sweep_rows(n, a_.reps))
        print(json.dumps(rows[-1]), flush=True)
        torch.cuda.empty_cache()
    rec = dict(device=torch.cuda.get_device_name(0), peak_bytes_per_s=PEAK, sweep=rows)
    if a_.level_n > 0:
        same = [r for r in rows if r["n"] == a_.level_n]
        sweep_s = same[0]["sweep_with_update"]["seconds"] if same else sweep_rows(a_.level_n, a_.reps)["sweep_with_update"]["seconds"]
        rec["level"] = level_row(a_.level_n, a_.level_maxit, sweep_s, a_.reps)
        print(json.dumps(rec["level"]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a_.out)), exist_ok=True)
    with open(a_.out, "w") as f:
        json.dump(rec, f, indent=1)
    print("wrote", a_.out)


if __name__ == "__main__":
    main()
