"""K11 (nep_lr_hankel) against the loop form it replaces, and whole infbilanczos runs with scalar_prod="auto" / "loop".

    python scripts/lrprod_bench.py [--out profiles/infbilanczos_k11.json] [--calls 20] [--runs 5] [--ks 8,20,40,80]

Micro-benchmark: qdep0 and gun_spmf_scaled, ma = mb = k, seeded complex blocks, the same process and device.  The loop form is
the reference's left_right_scalar_prod restated with the existing primitives only (k calls of compute_Mlincomb, k dot
products, nep_amd.infbilanczos._lrsp_loop).  Both return the scalar to the host, so every call is timed on the host clock
around a finished result; median of `calls` calls after 3 warm-up calls.  Whole runs: the qdep0 configuration of
test/infbilanczos.jl (maxit 40, neigs 3, tol 1e-7, check every 3 steps), median of `runs` runs per mode, plus one
instrumented run per mode for the share of time spent in the scalar products."""
import argparse
import importlib
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import nep_amd as na                          # noqa: E402
ib = importlib.import_module("nep_amd.infbilanczos")   # the module (the package attribute of that name is the driver)


def _timed(fn, calls):
    for _ in range(3):
        fn()
    ts = []
    for _ in range(calls):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return float(np.median(ts)), ts


def micro(ks, calls):
    out = []
    for name in ("qdep0", "gun_spmf_scaled"):
        nep = na.nep_gallery(name)
        n = nep.n
        for k in ks:
            rng = np.random.default_rng(k)
            W = na.to_dev(rng.standard_normal((n, k)) + 1j * rng.standard_normal((n, k)))
            B = na.to_dev(rng.standard_normal((n, k)) + 1j * rng.standard_normal((n, k)))
            sigma = 0.0
            tau = ib.taylor_table(nep, sigma, 2 * k)
            c_k11 = ib.lr_hankel(nep, W, B, k, k, tau)
            c_loop = ib._lrsp_loop(nep, W, B, k, k, sigma)
            t_k11, _ = _timed(lambda: ib.lr_hankel(nep, W, B, k, k, tau), calls)
            t_loop, _ = _timed(lambda: ib._lrsp_loop(nep, W, B, k, k, sigma), calls)
            row = dict(problem=name, n=n, k=k, k11_us=t_k11 * 1e6, loop_us=t_loop * 1e6, ratio=t_loop / t_k11,
                       rel_diff=abs(c_k11 - c_loop) / max(abs(c_loop), 1e-300))
            print(json.dumps(row), flush=True)
            out.append(row)
    return out


def whole_runs(runs):
    nep = na.nep_gallery("qdep0")
    nept = na.SPMF_NEP([A.T.tocsc() for A in nep.get_Av()], nep.get_fv())
    n = nep.n

    def run(mode):
        return na.infbilanczos(nep, nept, maxit=40, neigs=3, sigma=0.0, v=np.ones(n), u=np.ones(n), check_error_every=3,
                               tol=1e-7, errmeasure=na.ResidualErrmeasure(nep), scalar_prod=mode)
    res = {}
    for mode in ("auto", "loop"):
        run(mode)
        ts = []
        for _ in range(runs):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            run(mode)
            torch.cuda.synchronize()
            ts.append(time.perf_counter() - t0)
        # one instrumented run: the device is drained around every scalar product
        spent = [0.0, 0]
        orig = ib.left_right_scalar_prod

        def wrapped(*a, **kw):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            r = orig(*a, **kw)
            spent[0] += time.perf_counter() - t0
            spent[1] += 1
            return r
        ib.left_right_scalar_prod = wrapped
        try:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            run(mode)
            torch.cuda.synchronize()
            total = time.perf_counter() - t0
        finally:
            ib.left_right_scalar_prod = orig
        res[mode] = dict(median_s=float(np.median(ts)), runs_s=ts, scalar_prod_calls=spent[1],
                         scalar_prod_s=spent[0], scalar_prod_share=spent[0] / total, instrumented_s=total)
        print(json.dumps({mode: res[mode]}), flush=True)
    res["speedup"] = res["loop"]["median_s"] / res["auto"]["median_s"]
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "infbilanczos_k11.json"))
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--ks", default="8,20,40,80")
    ap.add_argument("--micro-only", action="store_true")
    a = ap.parse_args()
    rec = dict(device=torch.cuda.get_device_name(0), micro=micro([int(x) for x in a.ks.split(",")], a.calls))
    if not a.micro_only:
        rec["whole_runs_qdep0_kat"] = whole_runs(a.runs)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(rec, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
