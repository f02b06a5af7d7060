"""The device Hessenberg eigensolver (csrc/hesseig.hip: nep_hess_eigvals[_batch]_dev, nep_hess_eigvecs[_batch]_dev) through the raw
C ABI against the cases and criteria of tests/hesseig_checkers.py: closed-form spectra (C1), sigma_min, trace and residual bounds
in units of k u ||H|| (C2 - C4), eigenvalues bit for bit on triangular Gaussian-integer matrices under power-of-two scalings (E1),
scale invariance (E2) and windows with an offset (E3) bit for bit between two runs, the status words on non-finite input, on
vectors given up and below the first subdiagonal, and the mapped host mirror.  test_host_hesseig.py shows that the criteria hold
for LAPACK and for a NumPy restatement of the kernel at an eighth of each constant, and that they reject mutants."""
import ctypes as C
from functools import lru_cache

import numpy as np
import pytest
import torch

import hesseig_checkers as hc
from hesseig_checkers import C128, SENT

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def na():
    import nep_amd
    if nep_amd.device_count() < 1:
        pytest.skip("no GPU")
    return nep_amd


def _L():
    from nep_amd import _lib
    from nep_amd.nep import stream_ptr
    return _lib, _lib.lib, stream_ptr


def _up(buf):
    return torch.from_numpy(np.ascontiguousarray(buf)).to("cuda")


def _p(t, off=0, itemsize=16):
    return C.c_void_p(t.data_ptr() + itemsize * off)


def _down(t):
    return t.cpu().numpy()


def _work(k, nb=1):
    from nep_amd import dense
    stride = (dense.hess_eig_worksize(k) + 15) // 16 * 16
    return torch.empty(nb * stride, dtype=torch.uint8, device="cuda"), stride


def _single(stored, k, ldh, mirror=None):
    """nep_hess_eigvals_dev + nep_hess_eigvecs_dev on `stored` (flat, column c of H at c ldh) -> (w[0 : k + 2], Z (k, k))"""
    _lib, lib, st = _L()
    Hd, wd, Zd = _up(stored), _up(np.full(k + 2, SENT, dtype=C128)), _up(np.full(k * k, SENT, dtype=C128))
    work, _ = _work(k)
    mp = C.c_void_p(mirror.data_ptr()) if mirror is not None else None
    _lib.check(lib.nep_hess_eigvals_dev(k, _p(Hd), ldh, _p(wd), _p(work, 0, 1), mp, st()))
    _lib.check(lib.nep_hess_eigvecs_dev(k, _p(wd), _p(Zd), k, _p(work, 0, 1), mp, st()))
    torch.cuda.synchronize()
    return _down(wd), _down(Zd).reshape(k, k).T


def _dense(H):
    H = np.asarray(H, dtype=C128)
    return _single(H.T.reshape(-1), H.shape[0], H.shape[0])


@lru_cache(None)
def _dev(name):
    """the device's result on a case, computed once and shared by the tests that look at it"""
    return _dense(hc.by_name(name).H)


@pytest.mark.parametrize("name", [c.name for c in hc.cases()])
def test_case(na, name):
    """every case of hesseig_checkers.cases() against its criteria (C1 - C4 with the module's constants, E1, the status words)"""
    c = hc.by_name(name)
    wf, Z = _dev(name)
    rec = {}
    bad = hc.evaluate(c, wf, Z, record=rec)
    print(name, "sweeps %g" % wf[c.k].imag, "failed vectors %g" % wf[c.k + 1].real, {k: float("%.3g" % v) for k, v in rec.items()})
    assert not bad, (c, bad)


@pytest.mark.parametrize("name", [c.name for c in hc.cases() if c.family == "e2" and c.extra["s"] != 0])
def test_e2_scale_invariance_bit_for_bit(na, name):
    """w(2^s H) == 2^s w(H) and equal sweep counts: the iteration sees only the matrix scaled to max |entry| in [1/2, 1) and
    smlnum.  Z is held to C4 and the convention by test_case; whether it is bitwise equal too is reported (eps3 comes from sums of
    hypot, which need not scale exactly)"""
    c = hc.by_name(name)
    c0 = hc.by_name(c.extra["base"])
    (wf0, Z0), (wfs, Zs) = _dev(c0.name), _dev(name)
    hc.check_scale_pair(c0, c, wf0, wfs)
    E2_Z_BITWISE[name] = bool(np.array_equal(Z0, Zs))
    print(name, "Z bitwise equal:", E2_Z_BITWISE[name])


E2_Z_BITWISE = {}


@pytest.mark.parametrize("name", [c.name for c in hc.cases() if c.family == "e3"])
def test_e3_window_with_an_offset_bit_for_bit(na, name):
    """H block upper triangular with H[p, p - 1] = 0: the eigenvalues of each diagonal block equal, in position and bit for bit,
    those of the block alone -- (70, 5) is a 65-long window at l = 5 (second column set), (70, 6) a 64-long one whose columns
    reach lane 63, (128, 64) a 64-long window at l = 64; the sweep counts add up"""
    c = hc.by_name(name)
    wfH, _ = _dev(name)
    assert wfH[c.k].real == 0
    hc.check_blocks(c, wfH, [_dense(c.H[a:b, a:b])[0] for a, b in c.extra["blocks"]])


def test_entries_below_the_first_subdiagonal_are_ignored(na):
    """k = 22 of an (m, m + 4) block in nep_iar_step's row layout with NaN (and then Inf) everywhere the kernel must not look:
    words and vectors bitwise equal to those of the clean call"""
    H = hc.gun()[:22, :22]
    m = 30
    clean = _single(hc.iar_row_layout(H, m, 0.0).reshape(-1), 22, m + 4)
    assert clean[0][22].real == 0 and clean[0][23] == 0
    for poison in (complex(np.nan, np.nan), complex(np.inf, -np.inf)):
        wf, Z = _single(hc.iar_row_layout(H, m, poison).reshape(-1), 22, m + 4)
        assert np.array_equal(wf, clean[0]) and np.array_equal(Z, clean[1]), poison


def test_mirror_single_call(na):
    """a pinned mapped tensor as h_mirror holds w[0 : k + 2] after a stream synchronisation, and nothing behind it"""
    k = 17
    H = hc.gun()[:k, :k]
    mirror = torch.full((k + 2 + 4,), SENT, dtype=torch.complex128).pin_memory()
    wf, _ = _single(H.T.reshape(-1), k, k, mirror=mirror)
    mh = mirror.numpy()
    assert wf[k].real == 0 and wf[k + 1] == 0
    assert np.array_equal(mh[:k + 2], wf) and np.all(mh[k + 2:] == SENT)
    assert np.array_equal(wf, _dev("gun_17")[0])                      # the mirror changes nothing


def test_mirror_batch_of_three(na):
    """nb = 3 leading blocks (k = 4, 6, 8) with mirror_stride > kmax + 2: every block's words arrive, the padding keeps its sentinel"""
    _lib, lib, st = _L()
    nb, k0, kstep, kmax = 3, 4, 2, 8
    H = hc.gun()[:kmax, :kmax]
    ws, ms, zs = kmax + 2 + 1, kmax + 2 + 3, kmax * kmax + 5
    Hd, wd, Zd = _up(H.T.reshape(-1)), _up(np.full(nb * ws, SENT, dtype=C128)), _up(np.full(nb * zs, SENT, dtype=C128))
    work, stride = _work(kmax, nb)
    mirror = torch.full((nb * ms,), SENT, dtype=torch.complex128).pin_memory()
    mp = C.c_void_p(mirror.data_ptr())
    _lib.check(lib.nep_hess_eigvals_batch_dev(nb, k0, kstep, _p(Hd), kmax, _p(wd), ws, _p(work, 0, 1), stride, mp, ms, st()))
    _lib.check(lib.nep_hess_eigvecs_batch_dev(nb, k0, kstep, _p(wd), ws, _p(Zd), kmax, zs, _p(work, 0, 1), stride, mp, ms, st()))
    torch.cuda.synchronize()
    w, mh = _down(wd), mirror.numpy()
    for b in range(nb):
        k = k0 + b * kstep
        wf = w[b * ws: b * ws + k + 2]
        assert wf[k].real == 0 and wf[k + 1] == 0
        assert np.array_equal(mh[b * ms: b * ms + k + 2], wf), b
        assert np.all(mh[b * ms + k + 2: (b + 1) * ms] == SENT) and np.all(w[b * ws + k + 2: (b + 1) * ws] == SENT), b
        assert np.array_equal(wf, _dense(H[:k, :k])[0]), b            # the block of a batch = the single call on it


def test_unpinned_mirror_is_refused(na):
    """an ordinary host pointer as h_mirror: NEP_ERR_ARG from both calls, nothing launched, w untouched"""
    _lib, lib, st = _L()
    k = 5
    Hd, wd, Zd = _up(hc.gun()[:k, :k].T.reshape(-1)), _up(np.full(k + 2, SENT, dtype=C128)), _up(np.full(k * k, SENT, dtype=C128))
    work, _ = _work(k)
    plain = np.full(k + 2, SENT, dtype=C128)
    assert lib.nep_hess_eigvals_dev(k, _p(Hd), k, _p(wd), _p(work, 0, 1), _lib.hptr(plain), st()) == _lib.NEP_ERR_ARG
    assert lib.nep_hess_eigvecs_dev(k, _p(wd), _p(Zd), k, _p(work, 0, 1), _lib.hptr(plain), st()) == _lib.NEP_ERR_ARG
    torch.cuda.synchronize()
    assert np.all(_down(wd) == SENT) and np.all(_down(Zd) == SENT) and np.all(plain == SENT)


def test_zz_report_largest_ratios(na):
    """the largest value / bound of every criterion over the cases that ran in this process (each was asserted <= 1 where it arose)"""
    for key in sorted(hc.RATIOS):
        r, name = hc.RATIOS[key]
        print("ratio %s %.3g of the bound = %.3g units (%s)" % (key.upper(), r, r * hc.CONST[key], name))
        assert r <= 1.0
    for key, fam in sorted(hc.RATIOS_BY_FAMILY):
        r, name = hc.RATIOS_BY_FAMILY[(key, fam)]
        print("  %s %-8s %.3g units (%s)" % (key.upper(), fam, r * hc.CONST[key], name))
    print("E2: Z bitwise equal under scaling:", E2_Z_BITWISE)
