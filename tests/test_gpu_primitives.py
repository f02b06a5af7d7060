"""Direct parity tests of the C-ABI primitives that only drivers reach (include/nepmi355.h: the BLAS-1 style helpers of
csrc/util.hip, nep_gemv_h / nep_orth_qr_dev of csrc/orth.hip, nep_zgemm_sk and nep_gemm_ts_dev with a caller-owned B of
csrc/gemm.hip, nep_spmm_terms beyond p = 7 of csrc/spmv.hip, the batch calls of csrc/hesseig.hip).

Every entry point runs the case list of tests/primitive_checkers.py through `nep_amd._lib.lib`: exact cases (Gaussian-integer
operands, bit-for-bit equality with NumPy) carry the shape sweep, rounded cases (random operands) are held to a running error
bound against an extended-precision reference.  test_host_primitive_checkers.py shows that these checkers reject mutants."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import primitive_checkers as pc
from primitive_checkers import C128, SENT

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def na():
    import nep_amd
    if nep_amd.device_count() < 1:
        pytest.skip("no GPU")
    return nep_amd


# ---- adapters: the argument list of a checker's `impl` -> one call of the library ----------------------------------------------
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


def _coldots(fname):
    def impl(rows, k, X, ldx, Y, ldy):
        _lib, lib, st = _L()
        Xd = _up(X); Yd = Xd if Y is X else _up(Y)
        out = np.full(k, SENT, dtype=C128)
        _lib.check(getattr(lib, fname)(rows, k, _p(Xd), ldx, _p(Yd), ldy, _lib.hptr(out), st()))
        return out
    return impl


def _colnorms(rows, k, X, ldx):
    _lib, lib, st = _L()
    Xd = _up(X)
    out = np.full(k, -1.0)
    _lib.check(lib.nep_colnorms(rows, k, _p(Xd), ldx, _lib.hptr(out), st()))
    return out


def _nrm2(len, x):
    _lib, lib, st = _L()
    xd = _up(x)
    out = C.c_double(-1.0)
    _lib.check(lib.nep_nrm2(len, _p(xd), C.byref(out), st()))
    return out.value


def _rowmajor_colnorms(rows, k, XT, ld):
    _lib, lib, st = _L()
    Xd = _up(XT)
    out = np.full(k, -1.0)
    _lib.check(lib.nep_rowmajor_colnorms(rows, k, _p(Xd), ld, _lib.hptr(out), st()))
    return out


def _rm2cm(rows, k, src, lds, cols, ncols, dst, ldd):
    _lib, lib, st = _L()
    sd, dd = _up(src), _up(dst)
    rc = lib.nep_rowmajor_to_colmajor(rows, k, _p(sd), lds, _lib.hptr(cols) if cols is not None else None, ncols, _p(dd), ldd, st())
    return rc, _down(dd)


def _rowdot(rows, k, A, lda, B, ldb):
    _lib, lib, st = _L()
    Ad, Bd = _up(A), _up(B)
    out = _up(np.full(rows, SENT, dtype=C128))
    _lib.check(lib.nep_rowdot(rows, k, _p(Ad), lda, _p(Bd), ldb, _p(out), st()))
    return _down(out)


def _hadamard(rows, k, A, lda, B, ldb):
    _lib, lib, st = _L()
    Ad = _up(A); Bd = Ad if B is A else _up(B)
    _lib.check(lib.nep_hadamard(rows, k, _p(Ad), lda, _p(Bd), ldb, st()))
    return _down(Ad)


def _axpy(len, alpha, x, y):
    _lib, lib, st = _L()
    xd, yd = _up(x), _up(y)
    _lib.check(lib.nep_axpy(len, _lib.cd(alpha), _p(xd), _p(yd), st()))
    return _down(yd)


def _scal(len, alpha, x):
    _lib, lib, st = _L()
    xd = _up(x)
    _lib.check(lib.nep_scal(len, _lib.cd(alpha), _p(xd), st()))
    return _down(xd)


def _absvec(len, x):
    _lib, lib, st = _L()
    xd = _up(x); od = _up(np.full(len + 2, SENT, dtype=C128))
    _lib.check(lib.nep_absvec(len, _p(xd), _p(od), st()))
    return _down(od)


def _iar_shift_scale(n, k, buf, src_off, dst_off):
    _lib, lib, st = _L()
    bd = _up(buf)
    _lib.check(lib.nep_iar_shift_scale(n, k, _p(bd, src_off), _p(bd, dst_off), st()))
    return _down(bd)


def _rk_bw(n, N, wc, wc_off, c, Bw, bw_off):
    _lib, lib, st = _L()
    wd, bd = _up(wc), _up(Bw)
    c = np.ascontiguousarray(c, dtype=C128)
    _lib.check(lib.nep_rk_bw(n, N, _p(wd, wc_off), _lib.hptr(c) if N else None, _p(bd, bw_off), st()))
    return _down(bd)


def _block_recur(n, N, a, b, y, y_off, x, x_off):
    _lib, lib, st = _L()
    xd = _up(x); yd = xd if y is x else _up(y)
    a = np.ascontiguousarray(a, dtype=C128); b = np.ascontiguousarray(b, dtype=C128)
    _lib.check(lib.nep_block_recur(n, N, _lib.hptr(a) if N else None, _lib.hptr(b) if N else None, _p(yd, y_off), _p(xd, x_off), st()))
    return _down(xd)


def _gemv_h(V, ldv, rows, k, w):
    _lib, lib, st = _L()
    Vd, wd = _up(V), _up(w)
    out = np.full(k, SENT, dtype=C128)
    _lib.check(lib.nep_gemv_h(_p(Vd), ldv, rows, k, _p(wd), _lib.hptr(out), st()))
    return out


def _gemm_ts_dev(Z, z_off, ldz, rows, k, B, b_off, ldb, b_rowmajor, p, Y, y_off, ldy, y_rowmajor):
    _lib, lib, st = _L()
    Zd, Bd, Yd = _up(Z), _up(B), _up(Y)
    _lib.check(lib.nep_gemm_ts_dev(_p(Zd, z_off), ldz, rows, k, _p(Bd, b_off), ldb, b_rowmajor, p, _p(Yd, y_off), ldy, y_rowmajor, st()))
    return _down(Yd)


def _zgemm(sk):
    def impl(transa, transb, m, n, k, alpha, A, lda, B, ldb, beta, C, ldc, ksplit):
        _lib, lib, st = _L()
        Ad, Bd, Cd = _up(A), _up(B), _up(C)
        if sk:
            work = torch.full((ksplit * m * n,), float("nan"), dtype=torch.complex128, device="cuda")
            _lib.check(lib.nep_zgemm_sk(transa, transb, m, n, k, _lib.cd(alpha), _p(Ad), lda, _p(Bd), ldb, _lib.cd(beta), _p(Cd), ldc, ksplit,
                                        _p(work), st()))
        else:
            _lib.check(lib.nep_zgemm(transa, transb, m, n, k, _lib.cd(alpha), _p(Ad), lda, _p(Bd), ldb, _lib.cd(beta), _p(Cd), ldc, st()))
        return _down(Cd)
    return impl


_SPMF = {}


def _spmm_terms(terms, p, XT, ldx, ZT, ldz):
    import nep_amd
    _lib, lib, st = _L()
    if id(terms) not in _SPMF:
        f = nep_amd.funcs
        fv = ([f.one(), f.ident(), f.Exp(-0.3), f.Monomial(2)] * len(terms))[:len(terms)]
        _SPMF[id(terms)] = (terms, nep_amd.SPMF_NEP([A.tocsc() for A in terms], fv))
    nep = _SPMF[id(terms)][1]
    info = (C.c_int64 * 6)()
    _lib.check(lib.nep_spmf_info(nep.dev.h, info))
    want_bytes = 16 if any(np.iscomplexobj(A.data) for A in terms) else 8
    assert info[0] == terms[0].shape[0] and info[1] == len(terms) and info[3] == want_bytes, list(info)
    Xd, Zd = _up(XT), _up(ZT)
    rc = lib.nep_spmm_terms(nep.dev.h, p, _p(Xd), ldx, _p(Zd), ldz, st())
    return rc, _down(Zd)


def _orth_qr(Q, ldq, rows, k, out):
    _lib, lib, st = _L()
    Qd, od = _up(Q), _up(out)
    _lib.check(lib.nep_orth_qr_dev(_p(Qd), ldq, rows, k, _p(od), st()))
    return _down(Qd), _down(od)


def _hess_batch(nb, k0, kstep, H, ldh, w, w_stride, Z, ldz, z_stride):
    from nep_amd import dense
    _lib, lib, st = _L()
    kmax = k0 + (nb - 1) * kstep
    work_stride = (dense.hess_eig_worksize(kmax) + 15) // 16 * 16 + 64
    Hd, wd, Zd = _up(H), _up(w), _up(Z)
    work = torch.empty(nb * work_stride, dtype=torch.uint8, device="cuda")
    _lib.check(lib.nep_hess_eigvals_batch_dev(nb, k0, kstep, _p(Hd), ldh, _p(wd), w_stride, _p(work, 0, 1), work_stride, None, 0, st()))
    _lib.check(lib.nep_hess_eigvecs_batch_dev(nb, k0, kstep, _p(wd), w_stride, _p(Zd), ldz, z_stride, _p(work, 0, 1), work_stride, None, 0, st()))
    return _down(wd), _down(Zd)


ADAPTERS = {"nep_coldots": _coldots("nep_coldots"), "nep_coldotsu": _coldots("nep_coldotsu"), "nep_colnorms": _colnorms, "nep_nrm2": _nrm2,
            "nep_rowmajor_colnorms": _rowmajor_colnorms, "nep_rowmajor_to_colmajor": _rm2cm, "nep_rowdot": _rowdot, "nep_hadamard": _hadamard,
            "nep_axpy": _axpy, "nep_scal": _scal, "nep_absvec": _absvec, "nep_iar_shift_scale": _iar_shift_scale, "nep_rk_bw": _rk_bw,
            "nep_block_recur": _block_recur, "nep_gemv_h": _gemv_h, "nep_gemm_ts_dev": _gemm_ts_dev, "nep_zgemm_sk": _zgemm(True),
            "nep_spmm_terms": _spmm_terms, "nep_orth_qr_dev": _orth_qr, "nep_hess_eig_batch_dev": _hess_batch}


def run_prim(name, group=None):
    """every case of a primitive (of one group of its cases) on the device; returns the number of cases"""
    prim = pc.BY_NAME[name]
    n = 0
    for c in prim.cases():
        if group is None or c.group == group:
            prim.check(ADAPTERS[prim.name], c)
            n += 1
    return n


# ---- the case lists -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,group", [(p.name, g) for p in pc.PRIMS for g in pc.groups(p)])
def test_primitive_against_reference(na, name, group):
    """exact cases: np.array_equal with NumPy on Gaussian-integer operands; rounded cases: |dev - ref| <= bound against
    np.clongdouble (bounds: primitive_checkers.cbound and the docstrings of the checkers).  Padding (NaN where it must not be
    read, sentinels where it must not be written), offset pointers and aliased operands are part of the cases."""
    n = run_prim(name, group)
    assert n >= 1
    print("%s %s: %d cases, largest |dev - ref| / bound so far %.3g" % (name, group, n, pc.RATIOS.get(name, 0.0)))


@pytest.mark.parametrize("group", pc.groups(pc.HESS))
def test_hess_eig_batch_dev(na, group):
    """nep_hess_eigvals_batch_dev + nep_hess_eigvecs_batch_dev on leading blocks of one Hessenberg matrix in nep_iar_step's row
    layout (ldh = m + 4, poison below the subdiagonal), strides larger than the minimum with sentinels between the blocks: every
    block meets the criteria of _hess_eig_check and has the eigenvalues of the single-block call on the same leading block"""
    from test_gpu_kernels import _hess_eig_check

    def single(Hb):
        return _hess_eig_check(na, np.ascontiguousarray(Hb), 1e-12, 1e-12)[0]

    n = 0
    for c in pc.HESS.cases():
        if c.group == group:
            pc.HESS.check(_hess_batch, c, single=single)
            n += 1
    assert n == 1


def test_hess_eig_batch_dev_argument_checks(na):
    """w_stride < kmax + 2, a work stride that is not a multiple of 16 or too small, z_stride < kmax ldz: NEP_ERR_ARG; kmax = 129:
    NEP_ERR_UNSUPPORTED from the eigenvalue call"""
    from nep_amd import dense
    _lib, lib, st = _L()
    nb, k0, kstep = 3, 4, 2
    kmax = 8
    ws = dense.hess_eig_worksize(kmax)
    ws16 = (ws + 15) // 16 * 16
    Hd = _up(np.triu(np.ones((kmax, kmax), dtype=C128), -1))
    wd = _up(np.zeros(nb * (kmax + 2), dtype=C128)); Zd = _up(np.zeros(nb * kmax * kmax, dtype=C128))
    work = torch.empty(nb * (ws16 + 16), dtype=torch.uint8, device="cuda")

    def vals(w_stride=kmax + 2, work_stride=ws16, nb_=nb, k0_=k0, kstep_=kstep, ldh=kmax):
        return lib.nep_hess_eigvals_batch_dev(nb_, k0_, kstep_, _p(Hd), ldh, _p(wd), w_stride, _p(work, 0, 1), work_stride, None, 0, st())

    assert vals() == 0
    assert vals(w_stride=kmax + 1) == _lib.NEP_ERR_ARG
    assert vals(work_stride=ws16 + 8) == _lib.NEP_ERR_ARG
    assert vals(work_stride=ws16 - 16) == _lib.NEP_ERR_ARG
    assert vals(ldh=kmax - 1) == _lib.NEP_ERR_ARG
    assert vals(nb_=2, k0_=128, kstep_=1, ldh=200) == _lib.NEP_ERR_UNSUPPORTED        # kmax = 129
    assert lib.nep_hess_eigvecs_batch_dev(nb, k0, kstep, _p(wd), kmax + 2, _p(Zd), kmax, kmax * kmax - 1, _p(work, 0, 1), ws16, None, 0,
                                          st()) == _lib.NEP_ERR_ARG
    assert lib.nep_hess_eigvecs_batch_dev(nb, k0, kstep, _p(wd), kmax + 2, _p(Zd), kmax - 1, kmax * kmax, _p(work, 0, 1), ws16, None, 0,
                                          st()) == _lib.NEP_ERR_ARG
    torch.cuda.synchronize()


def test_rowdot_hadamard_refuse_short_leading_dimensions(na):
    """lda / ldb < rows are refused (NEP_ERR_ARG) instead of reading across columns; nep_coldots keeps accepting ldx = 0 (one
    column against k columns -- the `edges` cases of nep_coldots[u])"""
    _lib, lib, st = _L()
    rows, k = 100, 3
    Ad = _up(np.ones(rows * k + 8, dtype=C128)); Bd = _up(np.ones(rows * k + 8, dtype=C128)); od = _up(np.zeros(rows, dtype=C128))
    assert lib.nep_rowdot(rows, k, _p(Ad), rows, _p(Bd), rows, _p(od), st()) == 0
    assert lib.nep_rowdot(rows, k, _p(Ad), rows - 1, _p(Bd), rows, _p(od), st()) == _lib.NEP_ERR_ARG
    assert lib.nep_rowdot(rows, k, _p(Ad), rows, _p(Bd), 0, _p(od), st()) == _lib.NEP_ERR_ARG
    assert lib.nep_hadamard(rows, k, _p(Ad), rows - 1, _p(Bd), rows, st()) == _lib.NEP_ERR_ARG
    assert lib.nep_hadamard(rows, k, _p(Ad), rows, _p(Bd), rows - 1, st()) == _lib.NEP_ERR_ARG
    assert lib.nep_hadamard(rows, k, _p(Ad), rows, _p(Bd), rows, st()) == 0
    assert lib.nep_absvec(0, _p(Ad), _p(Bd), st()) == _lib.NEP_ERR_ARG                 # the header allows no empty nep_absvec
    torch.cuda.synchronize()


def test_rk_helpers_back_to_back_and_low_rank_split(na):
    """(1) two calls with different N back to back on one stream: the coefficient scratch is shared and uploaded again by the
    second call, the first result must not change.  (2) the low-rank split as nleigs.backslash_lowrank issues it: n-row blocks
    1 .. p - 1 and r-row blocks p + 1 .. N through two calls on offset pointers of the same buffers.  Integer data, exact."""
    _lib, lib, st = _L()
    rk, br = pc.BY_NAME["nep_rk_bw"], pc.BY_NAME["nep_block_recur"]
    rng = np.random.default_rng(3)
    n = 9956
    jobs = []
    for N in (43, 2, 100, 1):
        a = dict(n=n, N=N, wc=pc.gint(rng, n * (N + 1)), wc_off=0, c=pc.gint(rng, N), Bw=np.full(n * (N + 1), SENT, dtype=C128), bw_off=0)
        coef = dict(a=pc.gint(rng, N, -2, 2), b=rng.choice(np.array([0, 1, -1, 1j, -1j]), N).astype(C128))
        xy = pc.gint(rng, n * (N + 1))
        jobs.append((a, dict(n=n, N=N, y=xy, y_off=0, x=xy, x_off=0, **coef), _up(a["wc"]), _up(a["Bw"]), _up(xy)))
    for a, b, wd, bd, xd in jobs:                                   # all eight calls enqueued before anything is read back
        _lib.check(lib.nep_rk_bw(n, a["N"], _p(wd), _lib.hptr(a["c"]), _p(bd), st()))
        _lib.check(lib.nep_block_recur(n, b["N"], _lib.hptr(b["a"]), _lib.hptr(b["b"]), _p(xd), _p(xd), st()))
    for a, b, wd, bd, xd in jobs:
        pc.assert_below_2_53(2 * br.bound_S(**b))
        pc.assert_exact("nep_rk_bw back to back", a["N"], _down(bd), rk.ref(**a))
        pc.assert_exact("nep_block_recur back to back", b["N"], _down(xd), br.ref(**b))
    # (2) n = 257, r = 84, p = 2, N = 43: blocks 0 .. p of n rows, blocks p + 1 .. N of r rows
    n, r, p, N = 257, 84, 2, 43
    off = lambda j: j * n if j <= p else p * n + (j - p) * r
    nh, nr = min(N, p - 1), N - p
    total = off(N + 1)
    wc = pc.gint(rng, total); cB = pc.gint(rng, N)
    a_ = pc.gint(rng, N, -2, 2); b_ = rng.choice(np.array([0, 1, -1, 1j, -1j]), N).astype(C128)
    Bw0 = np.full(total + 1, SENT, dtype=C128)
    zb0 = np.concatenate([pc.gint(rng, total), [SENT]])
    wd, bd, zd = _up(wc), _up(Bw0), _up(zb0)
    c1, c2 = np.ascontiguousarray(cB[:nh]), np.ascontiguousarray(cB[p:])
    _lib.check(lib.nep_rk_bw(n, nh, _p(wd), _lib.hptr(c1), _p(bd), st()))
    _lib.check(lib.nep_rk_bw(r, nr, _p(wd, off(p)), _lib.hptr(c2), _p(bd, off(p)), st()))
    a1, b1, a2, b2 = (np.ascontiguousarray(v) for v in (a_[:nh], b_[:nh], a_[p:], b_[p:]))
    _lib.check(lib.nep_block_recur(n, nh, _lib.hptr(a1), _lib.hptr(b1), _p(zd), _p(zd), st()))
    _lib.check(lib.nep_block_recur(r, nr, _lib.hptr(a2), _lib.hptr(b2), _p(zd, off(p)), _p(zd, off(p)), st()))
    want = rk.ref(n=n, N=nh, wc=wc, wc_off=0, c=c1, Bw=Bw0, bw_off=0)
    want = rk.ref(n=r, N=nr, wc=wc, wc_off=off(p), c=c2, Bw=want, bw_off=off(p))
    pc.assert_exact("nep_rk_bw low-rank split", (n, r, p, N), _down(bd), want)
    want = br.ref(n=n, N=nh, a=a1, b=b1, y=zb0, y_off=0, x=zb0, x_off=0)
    want = br.ref(n=r, N=nr, a=a2, b=b2, y=want, y_off=off(p), x=want, x_off=off(p))
    pc.assert_exact("nep_block_recur low-rank split", (n, r, p, N), _down(zd), want)


def test_zgemm_sk_equals_zgemm_on_integers_and_repeats_bitwise(na):
    sk, plain = _zgemm(True), _zgemm(False)
    prim = pc.BY_NAME["nep_zgemm_sk"]
    n_exact = n_rounded = 0
    for c in prim.cases():
        if c.group not in ("trans", "few_chunks", "K17", "K9956"):
            continue
        a = c.args
        if c.kind == "exact":
            if np.isnan(a["C"]).any():                             # (beta = 0 cases: C holds NaN, which nep_zgemm must not read either)
                assert a["beta"] == 0
            pc.assert_exact("nep_zgemm_sk against nep_zgemm", c, sk(**a), plain(**a))
            n_exact += 1
        else:
            pc.assert_exact("nep_zgemm_sk twice", c, sk(**a), sk(**a))
            n_rounded += 1
    assert n_exact >= 100 and n_rounded >= 10, (n_exact, n_rounded)


def test_spmm_terms_plain_kernels_in_a_child_process(na):
    """NEP_SPMM_GROUPED=0 sends every p through k_spmm_rm<1..4>; the switch is read once per process, so the cases run in a child"""
    here = os.path.dirname(os.path.abspath(__file__))
    code = ("import sys; sys.path[:0] = [%r, %r]; import test_gpu_primitives as t; n = t.run_prim('nep_spmm_terms'); "
            "print('spmm_terms cases passed:', n)" % (here, os.path.dirname(here)))
    env = dict(os.environ, NEP_SPMM_GROUPED="0")
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300, env=env)
    assert out.returncode == 0, (out.stdout[-2000:], out.stderr[-4000:])
    assert "spmm_terms cases passed: %d" % len(list(pc.BY_NAME["nep_spmm_terms"].cases())) in out.stdout, out.stdout[-2000:]


def test_zz_report_largest_ratios(na):
    """the largest |dev - ref| / bound of every rounded case family that ran in this process (each was asserted <= 1 where it arose)"""
    for name in sorted(pc.RATIOS):
        print("ratio %-28s %.3g" % (name, pc.RATIOS[name]))
        assert pc.RATIOS[name] <= 1.0
