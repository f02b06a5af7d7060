"""K14, nep_spmf_biforms (csrc/biforms.hip), against the composed route it replaces.

    python scripts/ub_biforms.py [--out profiles/biforms.json] [--grid 1000] [--calls 20]

out[t, j, i] = w_i^H A_t v_j for every term, at (kw, kv) = (1, 1), (4, 4), (1, 16), on the gun matrices (n = 9956, 4 terms) and on
a grid problem in the waveguide's 5 + 2 + 1 slot layout (five-point stencil, first difference, identity; n = grid^2 ~ 1e6).
Composed route, per term t and column j: nep_mlincomb with the one-hot coefficient e_t (y = A_t v_j), then the forms of that
column with nep_coldots (kw = 1) or nep_gemv_h (kw > 1) -- what Proj_SPMF_NEP.expand_projectmatrices does today.  Both
routes return their numbers to the host.  Device events around each call, median of `calls` calls after 5 warm-up calls.
Traffic model of K14: the stacked CSR once per pass (ceil(kv / floor(32 / mt)) passes) + 16 n (kw + kv) bytes of W and V; the
fraction of the HBM peak is that over the time over 8 TB/s."""
import argparse
import json
import os
import sys

import numpy as np
import scipy.sparse as sp
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import nep_amd as na                          # noqa: E402
from nep_amd import dense                     # noqa: E402
from nep_amd._lib import lib, check, hptr, c_vp   # noqa: E402
from nep_amd.nep import stream_ptr            # noqa: E402

HBM_PEAK = 8.0e12
SHAPES = [(1, 1), (4, 4), (1, 16)]


def _timed(fn, calls):
    for _ in range(5):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(calls):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ts.append(e0.elapsed_time(e1) * 1e-3)
    return float(np.median(ts)), float(min(ts)), float(max(ts))


def grid_nep(g):
    """g x g grid numbered along z: a five-point stencil, a first difference along z and the identity, random real values"""
    rng = np.random.default_rng(7)
    n = g * g
    T = sp.diags([rng.standard_normal(n - 1), rng.standard_normal(n), rng.standard_normal(n - 1)], [-1, 0, 1])
    X = sp.diags([rng.standard_normal(n - g), rng.standard_normal(n - g)], [-g, g])
    D = sp.diags([rng.standard_normal(n), rng.standard_normal(n - 1)], [0, 1])
    return na.PEP([sp.csc_matrix(T + X), sp.csc_matrix(D), sp.identity(n, format="csc")])


def composed(dev, Wd, Vd, Y):
    n, mt = dev.n, dev.mt
    kw, kv = Wd.shape[0], Vd.shape[0]
    out = np.empty((mt, kv, kw), dtype=np.complex128)
    for t in range(mt):
        Cm = np.zeros((1, mt), dtype=np.complex128, order="F"); Cm[0, t] = 1.0
        for j in range(kv):
            dev.mlincomb(Cm, Vd[j].reshape(1, n), Y[j], k=1, ldv=n)
        if kw == 1:
            check(lib.nep_coldots(n, kv, c_vp(Wd.data_ptr()), 0, c_vp(Y.data_ptr()), n, hptr(out[t, :, 0]), stream_ptr()))
        else:
            for j in range(kv):
                out[t, j, :] = dense.gemv_h(Wd, Y[j], kw, rows=n, ldv=n)
    return out


def rows_for(name, nep, calls):
    dev = nep.dev
    n, mt = dev.n, dev.mt
    g = torch.Generator(device="cuda"); g.manual_seed(11)
    rows = []
    for kw, kv in SHAPES:
        Wd = torch.view_as_complex(torch.randn((kw, n, 2), dtype=torch.float64, device="cuda", generator=g))
        Vd = torch.view_as_complex(torch.randn((kv, n, 2), dtype=torch.float64, device="cuda", generator=g))
        Y = torch.empty((kv, n), dtype=torch.complex128, device="cuda")
        a = dev.biforms(Wd, Vd)
        b = composed(dev, Wd, Vd, Y)
        diff = float(np.max(np.abs(a - b)) / max(np.max(np.abs(b)), 1e-300))
        tf, lo, hi = _timed(lambda: dev.biforms(Wd, Vd), calls)
        tc, clo, chi = _timed(lambda: composed(dev, Wd, Vd, Y), max(3, calls // 4))
        passes = -(-kv // max(1, min(kv, 32 // mt)))
        nbytes = passes * dev.matrix_bytes + 16 * n * (kw + kv)
        rows.append(dict(problem=name, n=n, mt=mt, nnz=dev.nnz, kw=kw, kv=kv, passes=passes, k14_median_s=tf, k14_min_s=lo, k14_max_s=hi,
                         composed_median_s=tc, composed_min_s=clo, composed_max_s=chi, speedup=tc / tf, model_bytes=nbytes,
                         bytes_per_s=nbytes / tf, hbm_peak_fraction=nbytes / tf / HBM_PEAK, max_rel_diff=diff))
        print(json.dumps(rows[-1]), flush=True)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "biforms.json"))
    ap.add_argument("--grid", type=int, default=1000)
    ap.add_argument("--calls", type=int, default=20)
    a = ap.parse_args()
    if na.device_count() < 1:
        raise SystemExit("ub_biforms.py needs a GPU")
    rows = rows_for("gun", na.nep_gallery("gun_spmf_scaled"), a.calls)
    rows += rows_for("grid5(%d)" % a.grid, grid_nep(a.grid), a.calls)
    rec = dict(device=torch.cuda.get_device_name(0), rows=rows)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(rec, f, indent=1)
    print("wrote %s" % a.out)


if __name__ == "__main__":
    main()
