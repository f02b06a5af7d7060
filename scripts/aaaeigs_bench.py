"""AAAeigs at gun size, and the two small products of a CORK step as one fused kernel call each against the same products
composed from the plain dense GEMM.

    python scripts/aaaeigs_bench.py [--out profiles/aaaeigs.json] [--calls 5] [--reps 200] [--n 9956]

nlevp_native_gun (n = 9956) with the deterministic boundary part of the sample set of src/method_AAAeigs.jl:157-163 (250 real
points and a 250-point semicircle) and its five cyclic shifts.  The gallery's n = 9956 problem uses stand-in K and M matrices
(the reference's data files are not part of this repository) and the residual tolerance eps 1e6 is absolute, so the run is not
asked for six converged pairs: neigs = inf runs maxit = 60 steps with a convergence check every ten and returns every Ritz pair;
the number of pairs below the tolerance is reported.

  whole call   AAAeigs(nep, Z, shifts=shifts, v0=ones): host clock around the call (the driver synchronises at its checks and at its
               end); the first call, which builds the device-factorisation plan of the pattern, is reported apart; the median of
               the following `calls` calls, per call and per iteration.
  level 2      what a step does between the two device phases, at the shapes of the middle of that run (r = j = it / 2, k and l of
               the pencil): u_c = U_j C_sigma, Uhat = (alpha u1) g^T + U_j G_sigma and the Gram-Schmidt pass on U.  `reps`
               repetitions are enqueued back to back and the stream is synchronised once; the time per repetition is reported for
                 fused     two nep_cork_expand calls (one launch each)
                 composed  nep_zgemm for U_j C_sigma, nep_zgemm for U_j G_sigma, nep_zgemm with inner dimension 1 and beta = 1 for
                           the rank-1 term (alpha as its scale factor): three launches, the entry points of the commit before
                           nep_cork_expand
               each followed by the same nep_orth_dev call on U, and for that call alone.  The routes alternate in three rounds.
               The level-2 share is the fused level-2 time over the time per iteration of the whole call.
Launches per step are counted from the entry points: nep_cork_expand is one launch per call by construction; the launches of the
triangular solves are read from the factorisation (DeviceLU.launches_last_solve); K1 and K6 are listed as calls."""
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
from nep_amd import aaaeigs as aa, dense                               # noqa: E402
from nep_amd._lib import lib, check, c_vp, cd                          # noqa: E402
from nep_amd.linsolvers import _DeviceRefactor                         # noqa: E402
from nep_amd.nep import CDT, to_dev, stream_ptr                        # noqa: E402


def gun_samples():
    m, r = 250.0 ** 2, 300.0 ** 2 - 200.0 ** 2
    Z = np.concatenate([np.linspace(m - r + 1e-2, m + r - 1e-2, 250), m - r + 2 * r * (np.exp(1j * np.linspace(0.0, np.pi, 250)) / 2 + 0.5)])
    return Z, r * np.array([2.0 / 3, (1 + 1j) / 3, 0.0, (-1 + 1j) / 3, -2.0 / 3]) + m


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "aaaeigs.json"))
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--n", type=int, default=9956)
    ap.add_argument("--maxit", type=int, default=60)
    a_ = ap.parse_args()
    nep = na.nep_gallery("nlevp_native_gun", a_.n)
    n = nep.size(1)
    Z, shifts = gun_samples()
    v0 = np.ones(n)

    def call():
        info = {}
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        lam, X, res, _ = na.AAAeigs(nep, Z, shifts=shifts, v0=v0, neigs=np.inf, maxit=a_.maxit, info=info)
        torch.cuda.synchronize()
        return time.perf_counter() - t0, lam, X, res, info

    t_first, lam, X, res, info = call()
    _DeviceRefactor.wait()
    ts = []
    for _ in range(a_.calls):
        t, lam, X, res, info = call()
        ts.append(t)
    best = np.argsort(res)[:6]
    hres = [float(np.linalg.norm(nep.compute_Mder(lam[i]) @ X[:, i]) / np.linalg.norm(X[:, i])) for i in best]
    it, k, l = info["it"], info["k"], info["l"]
    row = dict(n=n, iterations=it, ritz_pairs=len(lam), pairs_below_tol=int(np.sum(np.asarray(res) < np.finfo(float).eps * 1e6)), m=info["m"], k=k, l=l, r=info["r"], factorisations=info["nfact"],
               first_call_s=t_first, call_s=float(np.median(ts)), call_min_max_s=[float(min(ts)), float(max(ts))],
               per_iteration_ms=float(np.median(ts)) / it * 1e3, six_smallest_host_residuals=hres,
               their_eigenvalues=[[float(lam[i].real), float(lam[i].imag)] for i in best])

    # ---- level 2 at the shapes of the middle of the run
    R = info["maxit"] + 1
    r = j = max(2, it // 2)
    rng = np.random.default_rng(0)
    g = lambda *sh: rng.standard_normal(sh) + 1j * rng.standard_normal(sh)
    Uh = np.zeros((R, k, R), dtype=np.complex128)                       # orthonormal slabs 0 .. j - 1, a continuation slab j - 1
    Qf = np.linalg.qr(g(r * k, j))[0]
    Uh[:r, :, :j] = Qf.reshape(r, k, j, order="F")
    U = torch.from_numpy(np.ascontiguousarray(Uh.transpose(2, 1, 0).reshape(R, k * R))).to("cuda")      # slab j: rho + R c
    Cs, gs, Gs = to_dev(g(k, l) / k), to_dev(g(k))[0], to_dev(g(k, k) / k)
    u1 = to_dev(g(r + 1))[0]
    alpha = 0.75 - 0.5j
    uc = torch.zeros((l, R), dtype=CDT, device="cuda")
    row_out = torch.zeros(R + 2, dtype=CDT, device="cuda")
    slab, nxt = U[j - 1], U[j]
    one, zero = cd(1.0), cd(0.0)

    def fused():
        aa._cork_expand(r, k, l, slab, R, Cs, k, None, None, 1.0, uc, R)
        aa._cork_expand(r + 1, k, k, slab, R, Gs, k, u1, gs, alpha, nxt, R)

    def composed():
        check(lib.nep_zgemm(0, 0, r, l, k, one, c_vp(slab.data_ptr()), R, c_vp(Cs.data_ptr()), k, zero, c_vp(uc.data_ptr()), R, stream_ptr()))
        check(lib.nep_zgemm(0, 0, r + 1, k, k, one, c_vp(slab.data_ptr()), R, c_vp(Gs.data_ptr()), k, zero, c_vp(nxt.data_ptr()), R, stream_ptr()))
        check(lib.nep_zgemm(0, 0, r + 1, k, 1, cd(alpha), c_vp(u1.data_ptr()), r + 1, c_vp(gs.data_ptr()), 1, one, c_vp(nxt.data_ptr()), R,
                            stream_ptr()))

    def orth():
        dense.orthogonalize_and_normalize_dev(U, nxt, j, row_out, rows=R * k, ldv=R * k, method=dense.DGKS)

    fused(); torch.cuda.synchronize(); a1 = nxt.cpu().numpy().copy(); c1 = uc.cpu().numpy().copy()
    composed(); torch.cuda.synchronize(); a2 = nxt.cpu().numpy(); c2 = uc.cpu().numpy()
    row["fused_vs_composed_rel_diff"] = float(max(np.linalg.norm(a1 - a2) / np.linalg.norm(a2), np.linalg.norm(c1 - c2) / np.linalg.norm(c2)))

    def timed(*fs):
        for f in fs:
            f()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(a_.reps):
            for f in fs:
                f()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / a_.reps * 1e6

    routes = {"fused_products_us": (fused,), "composed_products_us": (composed,), "fused_level2_us": (fused, orth),
              "composed_level2_us": (composed, orth), "orth_on_U_us": (orth,)}
    acc = {name: [] for name in routes}
    for _ in range(3):
        for name, fs in routes.items():
            acc[name].append(timed(*fs))
    for name in routes:
        row[name] = float(np.median(acc[name]))
        row[name + "_rounds"] = [float(x) for x in acc[name]]
    row["level2_shape"] = dict(r=r, j=j, k=k, l=l, R=R)
    row["level2_share_of_iteration"] = row["fused_level2_us"] * 1e-3 / row["per_iteration_ms"]
    row["ratio_composed_over_fused_products"] = row["composed_products_us"] / row["fused_products_us"]
    row["per_step"] = dict(nep_cork_expand_calls=2, nep_cork_expand_launches=2, composed_products_launches=3, k1_calls=1,
                           k5_solves=1, k5_launches=info.get("k5_launches"), k6_calls=2)
    print(json.dumps(row), flush=True)
    rec = dict(device=torch.cuda.get_device_name(0), rows=[row])
    os.makedirs(os.path.dirname(os.path.abspath(a_.out)), exist_ok=True)
    with open(a_.out, "w") as f:
        json.dump(rec, f, indent=1)
    print("wrote", a_.out)


if __name__ == "__main__":
    main()
