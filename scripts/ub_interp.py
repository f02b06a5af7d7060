"""nep_interp_coeffs (csrc/interp.hip) at the size of a large union pattern, against nep_zgemm on the same product.

    python scripts/ub_interp.py [--out profiles/interp_coeffs.json] [--entries 4000000] [--jk 20] [--calls 20]

C[e, :] = beta C[e, :] + W F[e, :] for E = 4e6 entries, J = K = 20: complex and real F, beta 0 and 1, device events around each
call, median of `calls` calls after 5 warm-up calls (warm clocks, code objects loaded).  nep_zgemm forms the same numbers as the
column-major product C^T = W F^T (m = K, n = E, k = J; complex F only: it has no real-input form, no row map, and accumulates
through its own beta).  Traffic model: E J (8 | 16) + E K 16 bytes, plus E K 16 when beta = 1; the fraction of the HBM peak is
that over the time over 8 TB/s (the measured streaming-copy rate of the device is 6.3 TB/s)."""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import nep_amd as na                          # noqa: E402
from nep_amd import _lib                      # noqa: E402
from nep_amd.nep import interp_coeffs, stream_ptr   # noqa: E402

HBM_PEAK = 8.0e12


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "interp_coeffs.json"))
    ap.add_argument("--entries", type=int, default=4000000)
    ap.add_argument("--jk", type=int, default=20)
    ap.add_argument("--calls", type=int, default=20)
    a = ap.parse_args()
    if na.device_count() < 1:
        raise SystemExit("ub_interp.py needs a GPU")
    E, J = a.entries, a.jk
    K = J
    g = torch.Generator(device="cuda"); g.manual_seed(5)
    Fr = torch.randn((E, J), dtype=torch.float64, device="cuda", generator=g)
    Fc = torch.view_as_complex(torch.randn((E, J, 2), dtype=torch.float64, device="cuda", generator=g))
    rng = np.random.default_rng(5)
    W = rng.standard_normal((K, J)) + 1j * rng.standard_normal((K, J))
    Wd = torch.from_numpy(np.ascontiguousarray(W.T)).to("cuda")          # K x J column-major on the device, for nep_zgemm
    Cd = torch.zeros((E, K), dtype=torch.complex128, device="cuda")
    rows = []
    for name, F, fb in (("complex", Fc, 16), ("real", Fr, 8)):
        for beta in (0, 1):
            Cd.zero_()
            t, lo, hi = _timed(lambda: interp_coeffs(F, W, Cd, None, beta), a.calls)
            nbytes = E * J * fb + E * K * 16 * (1 + beta)
            rows.append(dict(kernel="nep_interp_coeffs", F=name, beta=beta, E=E, J=J, K=K, median_s=t, min_s=lo, max_s=hi,
                             model_bytes=nbytes, bytes_per_s=nbytes / t, hbm_peak_fraction=nbytes / t / HBM_PEAK))
            print(json.dumps(rows[-1]), flush=True)
    one, zero = _lib.cd(1.0), _lib.cd(0.0)
    for beta in (0, 1):
        Cd.zero_()

        def gemm():
            _lib.check(_lib.lib.nep_zgemm(0, 0, K, E, J, one, C.c_void_p(Wd.data_ptr()), K, C.c_void_p(Fc.data_ptr()), J,
                                          one if beta else zero, C.c_void_p(Cd.data_ptr()), K, stream_ptr()))
        t, lo, hi = _timed(gemm, a.calls)
        nbytes = E * J * 16 + E * K * 16 * (1 + beta)
        rows.append(dict(kernel="nep_zgemm", F="complex", beta=beta, E=E, J=J, K=K, median_s=t, min_s=lo, max_s=hi,
                         model_bytes=nbytes, bytes_per_s=nbytes / t, hbm_peak_fraction=nbytes / t / HBM_PEAK))
        print(json.dumps(rows[-1]), flush=True)
    # same numbers: the two kernels on the complex block, beta = 0
    ref = interp_coeffs(Fc, W, Cd, None, 0)
    Cg = torch.empty_like(Cd)
    _lib.check(_lib.lib.nep_zgemm(0, 0, K, E, J, one, C.c_void_p(Wd.data_ptr()), K, C.c_void_p(Fc.data_ptr()), J, zero,
                                  C.c_void_p(Cg.data_ptr()), K, stream_ptr()))
    diff = float((ref - Cg).abs().max())
    rec = dict(device=torch.cuda.get_device_name(0), rows=rows, max_abs_diff_interp_vs_zgemm=diff)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(rec, f, indent=1)
    print("max |interp - zgemm| = %.3g; wrote %s" % (diff, a.out))


if __name__ == "__main__":
    main()
