"""The fused SPMF block product of blocknewton against the same product composed from the earlier primitives, and the driver on the
gun stand-in.

    python scripts/blocknewton_bench.py [--out profiles/blocknewton.json] [--reps 50] [--wep-nx 500] [--gun-maxit 20] [--no-driver]

  blockprod  Z = beta Z + alpha sum_t A_t (Y G_t) at the shapes the driver issues for p = 2 and p = 4 -- (r, q) = (p, p) (residual,
             T12), (p + 1, 1) (refinement residual, alpha = -1, beta = 1) and (p + 1, p - 1) (update (21), alpha = -1, beta = 1) --
             on the matrices of dep0_sparse(257), of the gun stand-in (n = 9956, 4 terms) and of the waveguide problem (3 real
             terms, n = nx nz + 2 nz).  fused: one nep_spmf_blockprod.  composed: nep_gemm_ts into the row-major n x (mt q) block,
             nep_spmm_terms, the transposing combine with Z (the driver's route for sizes the kernel refuses).  `reps` calls are
             enqueued back to back and the stream is synchronised once; the routes alternate in three rounds and the median is
             reported with all rounds, the derived byte counts (fused: matrix + 16 n r + 16 n q (+ 16 n q when Z is read);
             composed: that plus 2 * 16 n mt q for the intermediate and 2 * 16 n q for the transposed result) and the largest
             relative difference of the two results.
  driver     blocknewton on the gun stand-in (gun_spmf_scaled), p = 2, started from two Ritz pairs of a short iar run (the
             start of the reference's documentation diverges on the stand-in): iterations, error history, host clock, counters.
One JSON line on stdout; the same record goes to --out."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import nep_amd as na                                                   # noqa: E402
from nep_amd import dense                                              # noqa: E402
from nep_amd._lib import lib, check, c_vp, cd, hptr                    # noqa: E402
from nep_amd.nep import CDT, stream_ptr                                # noqa: E402


def timed(f, reps):
    f()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        f()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps


def blockprod_rows(name, dev, reps):
    n, mt = dev.n, dev.mt
    g = torch.Generator(device="cuda").manual_seed(n)
    rnd = lambda *s: torch.complex(torch.randn(*s, generator=g, device="cuda", dtype=torch.float64),
                                   torch.randn(*s, generator=g, device="cuda", dtype=torch.float64))
    rng = np.random.default_rng(n)
    rows = []
    for p in (2, 4):
        for r, q, alpha, beta in ((p, p, 1.0, 0.0), (p + 1, 1, -1.0, 1.0), (p + 1, p - 1, -1.0, 1.0)):
            Y = rnd(r, n)
            Z0 = rnd(q, n)
            G = (rng.standard_normal((mt, r, q)) + 1j * rng.standard_normal((mt, r, q))) / r
            Gf = np.ascontiguousarray(np.transpose(G, (0, 2, 1)))
            B = np.hstack([G[t] for t in range(mt)])
            Zf, Zc = Z0.clone(), Z0.clone()
            ZT = torch.empty((n, q), dtype=CDT, device="cuda")

            def fused():
                check(lib.nep_spmf_blockprod(dev.h, r, q, c_vp(Y.data_ptr()), n, hptr(Gf), cd(alpha), cd(beta), c_vp(Zf.data_ptr()), n,
                                             stream_ptr()))

            def composed():
                XT = dense.gemm_ts(Y, B, rowmajor=True, k=r)
                check(lib.nep_spmm_terms(dev.h, q, c_vp(XT.data_ptr()), q * mt, c_vp(ZT.data_ptr()), q, stream_ptr()))
                if beta == 0:
                    Zc.copy_(ZT.t())
                else:
                    Zc.mul_(complex(beta)).add_(ZT.t(), alpha=complex(alpha))

            fused(); composed(); torch.cuda.synchronize()
            diff = float((Zf - Zc).abs().max() / Zc.abs().max())
            acc = {"fused": [], "composed": []}
            for _ in range(3):
                acc["fused"].append(timed(fused, reps))
                acc["composed"].append(timed(composed, reps))
            zb = 16 * n * q * (2 if beta != 0 else 1)
            fused_bytes = dev.matrix_bytes + 16 * n * r + zb
            comp_bytes = fused_bytes + 2 * 16 * n * mt * q + 2 * 16 * n * q
            tf, tc = float(np.median(acc["fused"])), float(np.median(acc["composed"]))
            rows.append(dict(matrix=name, n=n, mt=mt, nnz=dev.nnz, p=p, r=r, q=q, alpha=alpha, beta=beta, fused_us=tf * 1e6,
                             composed_us=tc * 1e6, ratio_composed_over_fused=tc / tf, rel_diff=diff,
                             fused_rounds_us=[v * 1e6 for v in acc["fused"]], composed_rounds_us=[v * 1e6 for v in acc["composed"]],
                             derived_fused_bytes=fused_bytes, derived_composed_bytes=comp_bytes,
                             fused_gb_per_s_derived=fused_bytes / tf / 1e9))
    return rows


def driver_row(maxit):
    nep = na.nep_gallery("gun_spmf_scaled")
    n = nep.size(1)
    try:
        lam, Q = na.iar(nep, maxit=30, neigs=2, tol=1e-6, v=np.ones(n))[:2]
    except na.NoConvergenceException as e:
        lam, Q = np.asarray(e.lam), np.asarray(e.v)
    lam, Q = np.asarray(lam)[:2], np.asarray(Q)[:, :2]
    S0 = np.diag(lam)
    rec = dict(n=n, start_eigenvalues=[[float(l.real), float(l.imag)] for l in lam])
    info = {}
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    try:
        S, X = na.blocknewton(nep, S=S0, X=Q, maxit=maxit, armijo_factor=0.5, armijo_max=10, info=info)
        rec["converged"] = True
    except na.NoConvergenceException as e:
        S = e.lam
        rec["converged"] = False
    torch.cuda.synchronize()
    rec["seconds"] = time.perf_counter() - t0
    ev = np.linalg.eigvals(S)
    rec["eigenvalues"] = [[float(l.real), float(l.imag)] for l in ev]
    rec.update({k: info.get(k) for k in ("iters", "errhist", "armijo", "blockprod_calls", "composed_calls", "factorizations",
                                          "device_factorizations", "whole_fallbacks", "refine")})
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "blocknewton.json"))
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--wep-nx", type=int, default=500)
    ap.add_argument("--gun-maxit", type=int, default=20)
    ap.add_argument("--no-driver", action="store_true")
    a_ = ap.parse_args()
    rows = []
    rows += blockprod_rows("dep0_sparse(257)", na.nep_gallery("dep0_sparse", 257).dev, a_.reps)
    rows += blockprod_rows("gun", na.nep_gallery("gun_spmf_scaled").dev, a_.reps)
    if a_.wep_nx > 0:
        from nep_amd.wep import WEP
        rows += blockprod_rows("waveguide(%d)" % a_.wep_nx, WEP(nx=a_.wep_nx, nz=a_.wep_nx).dev, max(5, a_.reps // 5))
    rec = dict(device=torch.cuda.get_device_name(0), blockprod=rows)
    if not a_.no_driver:
        try:
            rec["driver_gun"] = driver_row(a_.gun_maxit)
        except Exception as e:                                            # the kernel figures above are kept
            rec["driver_gun"] = dict(error="%s: %s" % (type(e).__name__, e))
    os.makedirs(os.path.dirname(os.path.abspath(a_.out)), exist_ok=True)
    with open(a_.out, "w") as f:
        json.dump(rec, f, indent=1)
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
