"""One linear solve with the bordered matrix of a deflated NEP at a NEW shift, at gun size: the one-solve DeflatedNEPLinSolver
against the deflated NEP's own solver (the bordered matrix assembled and factorised as a whole).

    python scripts/defl_border_bench.py [--out profiles/defl_border.json] [--calls 20] [--rounds 3]

gun_spmf_scaled (n0 = 9956) with p = 4 deflated pairs in mode "SPMF" (a seeded invariant-pair stand-in: orthonormal V0, random
S0 -- the cost does not depend on the pair being invariant).  Every repetition uses a shift that no repetition used before, as a
Jacobi-Davidson iteration does.  Routes:
  one_solve   create_linsolver(DeflatedNEPLinSolverCreator(), dnep, lam): factorisation of M(lam) (on the device once the plan of
              the original pattern exists), one solve with it, nep_defl_border
  whole       create_linsolver(DefaultLinSolverCreator(), dnep, lam): compute_Mder of the deflated NEP, factorisation of the
              (n0 + p) x (n0 + p) matrix, one solve with it
Each call (creation of the solver and one solve_dev of a device vector) is timed on the host clock around the call and a device
synchronise.  The routes alternate in `rounds` rounds of `calls` calls after `warmup` warm-up calls each (the plans of the two
sparsity patterns are built behind the first factorisations and waited for before the timed rounds); the median over all calls of
a route is reported, with the share of calls whose numeric factorisation ran on the device."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import nep_amd as na                                  # noqa: E402
from nep_amd.linsolvers import _DeviceRefactor        # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "defl_border.json"))
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--n", type=int, default=9956)
    ap.add_argument("--p", type=int, default=4)
    a_ = ap.parse_args()
    nep = na.nep_gallery("gun_spmf_scaled", a_.n)
    n0, p = nep.n, a_.p
    rng = np.random.default_rng(0)
    V0 = np.linalg.qr(rng.standard_normal((n0, p)) + 1j * rng.standard_normal((n0, p)))[0]
    S0 = rng.standard_normal((p, p)) + 1j * rng.standard_normal((p, p))
    d = na.DeflatedSPMF(nep, S0, V0)
    b = na.to_dev(rng.standard_normal(n0 + p) + 1j * rng.standard_normal(n0 + p))[0]
    x = torch.empty_like(b)
    creators = {"one_solve": na.DeflatedNEPLinSolverCreator(), "whole": na.DefaultLinSolverCreator()}
    shifts = iter(0.3 + 0.1j + 1e-3 * (rng.standard_normal(100000) + 1j * rng.standard_normal(100000)))
    on_device = {r: [] for r in creators}

    def call(route, lam, record=True):
        s = na.create_linsolver(creators[route], d, lam)
        s.solve_dev(b, out=x)
        if record:
            lu = (s.orglinsolver if route == "one_solve" else s).lu
            on_device[route].append(bool(getattr(lu, "device_factorized", False)))

    # the two routes solve the same system
    lam = next(shifts)
    call("one_solve", lam, False); x1 = x.cpu().numpy()
    call("whole", lam, False); x2 = x.cpu().numpy()
    rel = float(np.linalg.norm(x1 - x2) / np.linalg.norm(x2))
    _DeviceRefactor.wait()
    for r in creators:
        for _ in range(a_.warmup):
            call(r, next(shifts), False)
    _DeviceRefactor.wait()
    torch.cuda.synchronize()
    ts = {r: [] for r in creators}
    for _ in range(a_.rounds):
        for r in creators:
            for _ in range(a_.calls):
                lam = next(shifts)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                call(r, lam)
                torch.cuda.synchronize()
                ts[r].append(time.perf_counter() - t0)
    row = dict(n0=n0, p=p, calls=a_.calls * a_.rounds, rel_diff_one_solve_vs_whole=rel)
    for r in creators:
        row[r + "_ms"] = float(np.median(ts[r])) * 1e3
        row[r + "_p10_p90_ms"] = [float(np.percentile(ts[r], 10)) * 1e3, float(np.percentile(ts[r], 90)) * 1e3]
        row[r + "_device_factorized_share"] = float(np.mean(on_device[r]))
    row["ratio_whole_over_one_solve"] = row["whole_ms"] / row["one_solve_ms"]
    print(json.dumps(row), flush=True)
    rec = dict(device=torch.cuda.get_device_name(0), rows=[row])
    os.makedirs(os.path.dirname(os.path.abspath(a_.out)), exist_ok=True)
    with open(a_.out, "w") as f:
        json.dump(rec, f, indent=1)
    print("wrote", a_.out)


if __name__ == "__main__":
    main()
