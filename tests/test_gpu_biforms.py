"""K14 on the device: nep_spmf_biforms (csrc/biforms.hip) through the raw C ABI on the cases of tests/biforms_checkers.py, and
SPMFDevice.biforms on a gallery problem.  test_host_biforms.py shows that the checker rejects a dropped term and a conjugate on
the wrong operand."""
import ctypes as C

import numpy as np
import pytest
import torch

import biforms_checkers as bc
from primitive_checkers import C128, NAN, colmajor_buf

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


def _p(t, off=0):
    return C.c_void_p(t.data_ptr() + 16 * off)


class Handle:
    """nep_spmf handle of a recipe"""

    def __init__(self, rec):
        _lib, lib, _ = _L()
        self.rec = rec
        self.h = C.c_void_p()
        rp, ci, vv, isc = rec.ptr_arrays()
        _lib.check(lib.nep_spmf_create(rec.n, rec.mt, rp, ci, vv, isc, C.byref(self.h)))
        info = (C.c_int64 * 6)()
        _lib.check(lib.nep_spmf_info(self.h, info))
        assert list(info)[:4] == [rec.n, rec.mt, rec.nnz, 16 if rec.any_complex else 8], list(info)

    def close(self):
        _L()[1].nep_spmf_destroy(self.h)

    def forms(self, W, V, pad=0, same=False, lead=0):
        """host output, device output and a second device output of one call each; asserts that the three agree bit for bit
        and that the words around the device block are untouched.  pad: leading dimension n + pad with NaN in the padding;
        same: dW == dV (W is ignored); lead: words in front of the blocks"""
        _lib, lib, st = _L()
        n, mt = self.rec.n, self.rec.mt
        kv = V.shape[1]
        ld = n + pad
        Vd = _up(colmajor_buf(V, ld, NAN, lead=lead, trail=3))
        Wd, kw = (Vd, kv) if same else (_up(colmajor_buf(W, ld, NAN, lead=lead, trail=3)), W.shape[1])
        no = mt * kw * kv
        h = np.full(no + 2, NAN, dtype=C128)
        _lib.check(lib.nep_spmf_biforms(self.h, kw, _p(Wd, lead), ld, kv, _p(Vd, lead), ld, _lib.hptr(h[1:]), None, st()))
        outs = []
        for _ in range(2):
            d = _up(np.full(no + 2, NAN, dtype=C128))
            _lib.check(lib.nep_spmf_biforms(self.h, kw, _p(Wd, lead), ld, kv, _p(Vd, lead), ld, None, _p(d, 1), st()))
            torch.cuda.synchronize()
            outs.append(d.cpu().numpy())
        for o in outs + [h]:
            assert np.isnan(o[0]) and np.isnan(o[-1]), "a word beside the output block was written"
        assert outs[0][1:-1].tobytes() == h[1:-1].tobytes(), "host and device output differ"
        assert outs[0].tobytes() == outs[1].tobytes(), "two calls on equal inputs differ"
        return h[1:-1].reshape(mt, kv, kw).copy()


@pytest.mark.parametrize("case", bc.CASES, ids=repr)
def test_biforms_case(na, case):
    rec = case.recipe()
    hd = Handle(rec)
    try:
        worst = bc.check(case, lambda rec, W, V: hd.forms(W, V))
        # leading dimension above n with NaN behind the rows, blocks that do not start their allocation
        kw, kv = case.shapes[min(1, len(case.shapes) - 1)]
        W, V, ref, S, N = bc.reference(case, rec, kw, kv)
        got = hd.forms(W, V, pad=3, lead=2)
        worst = max(worst, bc.check_forms("%s ld = n + 3" % case.name, got, ref, S, N))
        assert got.tobytes() == hd.forms(W, V).tobytes(), "the leading dimension changed the bits"
        # dW == dV (on the narrow block of the case: its reference is computed here)
        if kv > 5:
            V = bc.reference(case, rec, *case.shapes[0])[1]
        ref2, S2, N2 = bc.ref_forms(rec, V, V)
        worst = max(worst, bc.check_forms("%s W = V" % case.name, hd.forms(None, V, same=True), ref2, S2, N2))
    finally:
        hd.close()
    print("%s: largest |K14 - ref| / bound = %.3g" % (case.name, worst))


def test_limit_violations_return_their_code_and_launch_nothing(na):
    _lib, lib, st = _L()
    case = next(c for c in bc.CASES if c.name == "degenerate/n65_mt5_cplx")
    rec = case.recipe()
    hd = Handle(rec)
    n, mt = rec.n, rec.mt
    try:
        Xd = _up(np.ones(32 * n, dtype=C128))
        for kw, kv, ldw, ldv, null, want in [
                (0, 1, n, n, (), -5), (1, 0, n, n, (), -5), (33, 1, n, n, (), -5), (1, 33, n, n, (), -5),
                (32, 32, n, n, (), -5),                              # mt kw kv = 5120 > 3072
                (25, 25, n, n, (), -5),                              # 3125
                (1, 1, n - 1, n, (), -2), (1, 1, n, n - 1, (), -2),
                (1, 1, n, n, ("W",), -2), (1, 1, n, n, ("V",), -2), (1, 1, n, n, ("out",), -2), (1, 1, n, n, ("s",), -2)]:
            d = _up(np.full(3072, NAN, dtype=C128))
            h = np.full(3072, NAN, dtype=C128)
            for host in (False, True):
                rc = lib.nep_spmf_biforms(None if "s" in null else hd.h, kw, None if "W" in null else _p(Xd), ldw, kv,
                                          None if "V" in null else _p(Xd), ldv, _lib.hptr(h) if host and "out" not in null else None,
                                          None if host or "out" in null else _p(d), st())
                assert rc == want, (kw, kv, ldw, ldv, null, host, rc)
            torch.cuda.synchronize()
            assert np.all(np.isnan(d.cpu().numpy())) and np.all(np.isnan(h))
        # the limits themselves are accepted: 24 x 25 x 5 = 3000, 32 columns on one side
        for kw, kv in ((24, 25), (32, 19), (19, 32)):
            d = _up(np.full(3072, NAN, dtype=C128))
            assert lib.nep_spmf_biforms(hd.h, kw, _p(Xd), n, kv, _p(Xd), n, None, _p(d), st()) == 0
            torch.cuda.synchronize()
            assert np.all(np.isfinite(d.cpu().numpy()[:mt * kw * kv]))
    finally:
        hd.close()


def test_spmfdevice_biforms_on_a_gallery_problem(na):
    """the method of the device object: the result layout [t, j, i], vectors and blocks, host and device output"""
    nep = na.nep_gallery("overdamped_qep_sparse", 65)
    rng = np.random.default_rng(5)
    W = rng.standard_normal((65, 2)) + 1j * rng.standard_normal((65, 2))
    V = rng.standard_normal((65, 3)) + 1j * rng.standard_normal((65, 3))
    want = np.array([[[np.vdot(W[:, i], A @ V[:, j]) for i in range(2)] for j in range(3)] for A in nep.get_Av()])
    Wd, Vd = na.to_dev(W), na.to_dev(V)
    got = nep.dev.biforms(Wd, Vd)
    assert got.shape == (3, 3, 2) and np.allclose(got, want, rtol=1e-13, atol=1e-12)
    out = torch.empty(18, dtype=torch.complex128, device="cuda")
    assert nep.dev.biforms(Wd, Vd, out=out) is out
    assert out.cpu().numpy().tobytes() == got.tobytes()
    q = nep.dev.biforms(Vd[1], Vd[1])                          # two vectors: the Rayleigh functional's forms
    assert q.shape == (3, 1, 1) and np.allclose(q.reshape(-1), want_diag(nep, V[:, 1]), rtol=1e-13, atol=1e-12)


def want_diag(nep, x):
    return np.array([np.vdot(x, A @ x) for A in nep.get_Av()])
