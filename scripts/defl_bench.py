"""compute_Mlincomb of a deflated NEP at gun size: through nep_defl_expand against the same product composed from the primitives
the library had before it.

    python scripts/defl_bench.py [--out profiles/defl_expand.json] [--calls 50] [--rounds 5]

gun_spmf_scaled (n0 = 9956) with p = 4 deflated pairs (a seeded invariant-pair stand-in: orthonormal V0, random S0 -- the cost
does not depend on the pair being invariant), (k, startder) = (1, 0) and (1, 1): the two calls a Newton step makes.  Routes:
  fused           DeflatedGenericNEP.compute_Mlincomb: tables on the host, nep_defl_expand, K1 with a block of ones
  composed        the same formulas from gemm_ts (X W_d), nep_gemm_ts_dev ((X W_d) V2), nep_axpy, nep_gemv_h (z_bottom comes back
                  to the host and is uploaded again) and K1
  composed_async  the product's own fallback for sizes the kernel refuses (z_bottom by nep_gemv_hd: no synchronisation)
Device tensor in, device tensor out; every call is timed on the host clock around the call and a device synchronise.  The routes
alternate in `rounds` rounds of `calls` calls after 5 warm-up calls each; the median over all calls of a route is reported, and
for the asynchronous routes the time per call of `calls` calls enqueued back to back."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import nep_amd as na                          # noqa: E402
from nep_amd import dense                     # noqa: E402
from nep_amd.deflation import expand_tables   # noqa: E402
from nep_amd.nep import CDT                   # noqa: E402


def _top(d, lam, Vn, z):
    org = d.orgnep
    org.dev.mlincomb(org.coeff_block(lam, np.ones(Vn.shape[0])), Vn, z)
    return z


def composed(d, lam, Vd, a, s, host_zb):
    a, G, W = expand_tables(lam, d.S0, a, s)
    z = torch.empty(d.n, dtype=CDT, device="cuda")
    Vn = torch.empty((Vd.shape[0] + s, d.n0), dtype=CDT, device="cuda")
    zb = z[d.n0:]
    if host_zb and s == 0:                                              # nep_gemv_h: the result crosses to the host and back
        d._expand_composed(Vd, a, G, W, s, Vn, None)
        zb.copy_(torch.from_numpy(a[0] * dense.gemv_h(d.Xd, Vd[0], d.p, rows=d.n0, ldv=d.n0)))
    else:
        d._expand_composed(Vd, a, G, W, s, Vn, zb)
    return _top(d, lam, Vn, z)


def _time_calls(fn, calls):
    ts = []
    for _ in range(calls):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    return ts


def _time_pipelined(fn, calls):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(calls):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / calls


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "defl_expand.json"))
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--n", type=int, default=9956)
    ap.add_argument("--p", type=int, default=4)
    a_ = ap.parse_args()
    nep = na.nep_gallery("gun_spmf_scaled", a_.n)
    n0, p = nep.n, a_.p
    rng = np.random.default_rng(0)
    V0 = np.linalg.qr(rng.standard_normal((n0, p)) + 1j * rng.standard_normal((n0, p)))[0]
    S0 = rng.standard_normal((p, p)) + 1j * rng.standard_normal((p, p))
    d = na.DeflatedGenericNEP(nep, S0, V0)
    lam = 0.3 + 0.1j
    rows = []
    for k, s in ((1, 0), (1, 1)):
        Vd = na.to_dev(rng.standard_normal((n0 + p, k)) + 1j * rng.standard_normal((n0 + p, k)))
        av = np.ones(k, dtype=np.complex128)
        routes = {"fused": lambda: d.compute_Mlincomb(lam, Vd, a=av, startder=s),
                  "composed": lambda: composed(d, lam, Vd, av, s, True),
                  "composed_async": lambda: composed(d, lam, Vd, av, s, False)}
        want = routes["fused"]().cpu().numpy()
        diffs = {r: float(np.linalg.norm(f().cpu().numpy() - want) / np.linalg.norm(want)) for r, f in routes.items()}
        for f in routes.values():
            for _ in range(5):
                f()
        ts = {r: [] for r in routes}
        for _ in range(a_.rounds):
            for r, f in routes.items():
                ts[r] += _time_calls(f, a_.calls)
        row = dict(n0=n0, p=p, k=k, startder=s, calls=a_.calls * a_.rounds, rel_diff_to_fused=diffs)
        for r in routes:
            row[r + "_us"] = float(np.median(ts[r])) * 1e6
            row[r + "_p10_p90_us"] = [float(np.percentile(ts[r], 10)) * 1e6, float(np.percentile(ts[r], 90)) * 1e6]
        for r in ("fused", "composed_async"):
            row[r + "_pipelined_us"] = min(_time_pipelined(routes[r], a_.calls) for _ in range(a_.rounds)) * 1e6
        row["ratio_composed_over_fused"] = row["composed_us"] / row["fused_us"]
        print(json.dumps(row), flush=True)
        rows.append(row)
    rec = dict(device=torch.cuda.get_device_name(0), rows=rows)
    os.makedirs(os.path.dirname(os.path.abspath(a_.out)), exist_ok=True)
    with open(a_.out, "w") as f:
        json.dump(rec, f, indent=1)
    print("wrote", a_.out)


if __name__ == "__main__":
    main()
