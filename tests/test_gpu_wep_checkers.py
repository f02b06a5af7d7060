"""Direct parity tests of the waveguide kernels (csrc/wep.hip: Sylvester solve, P(lam)^{-1}, matrix-free Schur product, region
means / expansion, SMW matrix and the three-transform SMW preconditioner) through the raw C ABI (`nep_amd._lib.lib`), driven by the
checkers of tests/wep_checkers.py: exact integer cases, entrywise-bounded cases, and cases measured per grid column against the
float64 restatement.  The adapters below turn a checker's `impl` argument list into one library call on uploaded buffers; every
output buffer is filled with pc.SENT first and has two entries of padding that must survive.  test_host_wep_checkers.py shows that
the checkers reject mutants and, with nep_wep_plan, that the cases reach every kernel instantiation; NEP_WEP_DFT_SYM (read once per
process) is varied in child processes."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import primitive_checkers as pc
import wep_checkers as wc
from primitive_checkers import C128, SENT

pytestmark = pytest.mark.gpu
PAD = 2


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


def _stop(what, e):
    pytest.exit("HIP error in %s: %s -- nothing more is started on this device" % (what, e), returncode=3)


def _ok(rc, what):
    """status 0, or the session ends: after a HIP error (-1) the device may have faulted"""
    if rc == -1:
        _stop(what, _L()[1].nep_last_error().decode(errors="replace"))
    assert rc == 0, (what, rc, _L()[1].nep_last_error().decode(errors="replace"))


def _up(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=C128).reshape(-1)).to("cuda")


def _up_padded(a):
    a = np.ascontiguousarray(a, dtype=C128).reshape(-1)
    return _up(np.concatenate([a, np.full(PAD, SENT, dtype=C128)]))


def _sent(n):
    return torch.full((n + PAD,), SENT, dtype=torch.complex128, device="cuda")


def _p(t):
    return C.c_void_p(t.data_ptr())


def _down(t, what="download"):
    try:
        torch.cuda.synchronize()
        return t.cpu().numpy()
    except RuntimeError as e:
        _stop(what, e)


def _body(buf, n, what):
    """the first n entries of a downloaded buffer whose padding has to be intact"""
    assert np.all(buf[n:] == SENT), "%s: written behind the end of the output" % what
    return buf[:n]


class Handles:
    """nep_wep_sylv and / or nep_wep_pinv handles of a grid, destroyed on exit"""

    def __init__(self, nz, nx=None, d=None, b=None, bb=None):
        _lib, lib, _ = _L()
        self.s, self.p = C.c_void_p(), C.c_void_p()
        try:
            if d is not None:
                self._d = np.ascontiguousarray(d, dtype=C128)
                _ok(lib.nep_wep_sylv_create(nz, nx, _lib.hptr(self._d), float(b), C.byref(self.s)), "nep_wep_sylv_create")
                info = (C.c_int32 * 4)()
                _ok(lib.nep_wep_sylv_info(self.s, info), "nep_wep_sylv_info")
                assert (info[0], info[1]) == wc.factor(nz) and info[3] == wc.seg_of(nx)
            if bb is not None:
                self._bb = np.ascontiguousarray(bb, dtype=C128)
                _ok(lib.nep_wep_pinv_create(nz, _lib.hptr(self._bb), C.byref(self.p)), "nep_wep_pinv_create")
        except BaseException:
            self.close()
            raise

    def close(self):
        lib = _L()[1]
        if self.s:
            lib.nep_wep_sylv_destroy(self.s); self.s = C.c_void_p()
        if self.p:
            lib.nep_wep_pinv_destroy(self.p); self.p = C.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


# ---- adapters: the argument list of a checker's impl -> library calls -----------------------------------------------------------
def sylv_impl(nz, nx, d, b, X):
    _, lib, st = _L()
    outs = []
    with Handles(nz, nx, d=d, b=b) as h:
        for _ in range(2):
            Xd = _up_padded(X)
            _ok(lib.nep_wep_sylv_solve(h.s, _p(Xd), st()), "nep_wep_sylv_solve %dx%d" % (nz, nx))
            outs.append(_body(_down(Xd, "nep_wep_sylv_solve %dx%d" % (nz, nx)), nz * nx, "nep_wep_sylv_solve").reshape(nx, nz))
    return outs[0], outs[1]


def pinv_impl(nz, bb, sinv, x):
    _, lib, st = _L()
    with Handles(nz, bb=bb) as h:
        sd, xd, od = _up(sinv), _up_padded(x), _sent(2 * nz)
        _ok(lib.nep_wep_pinv_apply(h.p, _p(sd), _p(xd), _p(od), st()), "nep_wep_pinv_apply nz=%d" % nz)
        out, x_after = _down(od, "nep_wep_pinv_apply nz=%d" % nz), _down(xd)
        _ok(lib.nep_wep_pinv_apply(h.p, _p(sd), _p(xd), _p(xd), st()), "nep_wep_pinv_apply (in place) nz=%d" % nz)
        return out, x_after, _down(xd, "nep_wep_pinv_apply (in place) nz=%d" % nz)


def schur_impl(nz, nx, bb, sinv, X, D0, cp, cm, cx, d1, d2, c1s):
    _lib, lib, st = _L()
    with Handles(nz, bb=bb) as h:
        sd, Xd, Dd, Pd, od = _up(sinv), _up(X), _up(D0), _sent(2 * nz), _sent(nz * nx)
        what = "nep_wep_schur_matvec %dx%d" % (nz, nx)
        _ok(lib.nep_wep_schur_matvec(h.p, _p(sd), nx, _p(Xd), _p(Dd), _lib.cd(cp), _lib.cd(cm), cx, d1, d2, c1s, _p(Pd), _p(od), st()), what)
        return _down(Pd, what), _down(od), _down(Xd)


def means_impl(nz, nx, N, X):
    _, lib, st = _L()
    Xd, od = _up(X), _sent(N * (N + 4))
    _ok(lib.nep_wep_region_means(nz, nx, N, _p(Xd), _p(od), st()), "nep_wep_region_means")
    return _down(od, "nep_wep_region_means")


def expand_impl(nz, nx, N, alpha, Ksc, dd1, dd2):
    _, lib, st = _L()
    ad, Kd, Yd, ed = _up(alpha), _up(Ksc), _sent(nz * nx), _sent(2 * nz)
    _ok(lib.nep_wep_region_expand(nz, nx, N, _p(ad), _p(Kd), dd1, dd2, _p(Yd), _p(ed), st()), "nep_wep_region_expand")
    return _down(Yd, "nep_wep_region_expand"), _down(ed)


def smw_matrix_impl(modes, o, N):
    _, lib, st = _L()
    nz = len(o["bb"]); nx = nz + 4; mm = N * (N + 4)
    with Handles(nz, nx, d=o["d"], b=o["b"], bb=o["bb"]) as h:
        Kd, sd, Md = _up(o["Ksc"]), _up(o["sinv"]), _sent(mm * mm)
        if modes:
            what = "nep_wep_smw_matrix_modes nz=%d N=%d" % (nz, N)
            Gd = _up(o["G"])
            _ok(lib.nep_wep_smw_matrix_modes(h.s, h.p, N, _p(Kd), o["dd1"], o["dd2"], _p(sd), _p(Gd), _p(Md), st()), what)
        else:
            what = "nep_wep_smw_matrix nz=%d N=%d" % (nz, N)
            work = torch.empty(nz * nx + 4 * nz + mm, dtype=torch.complex128, device="cuda")
            _ok(lib.nep_wep_smw_matrix(h.s, h.p, N, _p(Kd), o["dd1"], o["dd2"], _p(sd), _p(work), _p(Md), st()), what)
        return _body(_down(Md, what), mm * mm, what).reshape(mm, mm)


def smw_apply_impl(o, calls):
    _, lib, st = _L()
    nz = len(o["bb"]); nx = nz + 4
    outs = []
    with Handles(nz, nx, d=o["d"], b=o["b"], bb=o["bb"]) as h:
        Kd, sd = _up(o["Ksc"]), _up(o["sinv"])
        for N, MinvH, G, R in calls:
            what = "nep_wep_smw_apply nz=%d N=%d" % (nz, N)
            Md, Gd, Rd = _up(MinvH), _up(G), _up_padded(R)
            _ok(lib.nep_wep_smw_apply(h.s, h.p, N, _p(Kd), o["dd1"], o["dd2"], _p(sd), _p(Md), _p(Gd), _p(Rd), st()), what)
            outs.append(_body(_down(Rd, what), nz * nx, what).reshape(nx, nz))
    return outs


IMPL = {"nep_wep_sylv_solve": sylv_impl, "nep_wep_pinv_apply": pinv_impl, "nep_wep_schur_matvec": schur_impl,
        "nep_wep_region_means": means_impl, "nep_wep_region_expand": expand_impl,
        "nep_wep_smw_matrix": lambda o, N: smw_matrix_impl(False, o, N), "nep_wep_smw_matrix_modes": lambda o, N: smw_matrix_impl(True, o, N),
        "nep_wep_smw_apply": smw_apply_impl}
CASES = [(name, c) for name, k in wc.CHECKERS.items() for c in k.cases()]


@pytest.mark.parametrize("name,c", CASES, ids=["%s-%s-%s" % (n.replace("nep_wep_", ""), c.cid, c.kind) for n, c in CASES])
def test_case(na, name, c):
    """every case of every checker of tests/wep_checkers.py on the library"""
    if "form" in c.extra and name == "nep_wep_sylv_solve" and not os.environ.get("NEP_WEP_DFT_SYM"):
        info = (C.c_int64 * 8)()                             # the instantiation this very process launches
        assert _L()[1].nep_wep_plan(c.extra["nz"], c.extra["nx"], wc.OP_SYLV, info) == 0
        assert (wc.dft_form(list(info)), info[7]) == (c.extra["form"], c.extra["seg"])
    wc.CHECKERS[name].check(IMPL[name], c)


def test_refusals(na):
    """every NEP_ERR_ARG / NEP_ERR_UNSUPPORTED return of csrc/wep.hip with its code; outputs stay untouched"""
    _lib, lib, st = _L()
    ARG, UNS = -2, -5
    plan = lambda nz, nx, op: lib.nep_wep_plan(nz, nx, op, (C.c_int64 * 8)())
    d = np.full(4000, 1.0 + 2.0j, dtype=C128)
    for nz, nx in wc.REFUSE_SYLV_ARG:
        h = C.c_void_p(1)
        assert plan(nz, nx, wc.OP_SYLV) == ARG
        assert lib.nep_wep_sylv_create(nz, nx, _lib.hptr(d), 1.0, C.byref(h)) == ARG and not h
    big = wc.first_unstaged_nz(plan)
    h = C.c_void_p(1)
    assert lib.nep_wep_sylv_create(big, 5, _lib.hptr(d), 1.0, C.byref(h)) == UNS and not h
    h = C.c_void_p(1)
    assert lib.nep_wep_sylv_create(7, 11, None, 1.0, C.byref(h)) == ARG and not h
    assert lib.nep_wep_sylv_create(7, 11, _lib.hptr(d), 1.0, None) == ARG
    h = C.c_void_p(1)
    assert plan(wc.REFUSE_PINV_NZ, 0, wc.OP_PINV) == UNS
    assert lib.nep_wep_pinv_create(wc.REFUSE_PINV_NZ, _lib.hptr(d), C.byref(h)) == UNS and not h
    assert lib.nep_wep_pinv_create(7, None, C.byref(h)) == ARG and lib.nep_wep_pinv_create(0, _lib.hptr(d), C.byref(h)) == ARG
    assert lib.nep_wep_sylv_info(None, (C.c_int32 * 4)()) == ARG

    def smw_calls(hs, hp, N, nz, nx):
        """(status of nep_wep_smw_apply, of nep_wep_smw_matrix_modes); dR and dM must stay untouched"""
        mm = N * (N + 4)
        Kd, sd, Md, Gd = _sent(nz * nx), _sent(2 * nz), _sent(mm * mm), _sent(N * nz)
        Rd, Mo = _sent(nz * nx), _sent(mm * mm)
        r1 = lib.nep_wep_smw_apply(hs, hp, N, _p(Kd), 1.0, -0.5, _p(sd), _p(Md), _p(Gd), _p(Rd), st())
        r2 = lib.nep_wep_smw_matrix_modes(hs, hp, N, _p(Kd), 1.0, -0.5, _p(sd), _p(Gd), _p(Mo), st())
        assert np.all(_down(Rd) == SENT) and np.all(_down(Mo) == SENT)
        return r1, r2

    nz = wc.REFUSE_SMW_EVEN
    assert plan(nz, nz + 4, wc.OP_SMW) == UNS
    o = wc.smw_operands(nz)
    with Handles(nz, nz + 4, d=o["d"], b=o["b"], bb=o["bb"]) as h60:
        assert smw_calls(h60.s, h60.p, 3, nz, nz + 4) == (UNS, UNS)
    o15 = wc.smw_operands(15)
    with Handles(15, 19, d=o15["d"], b=o15["b"], bb=o15["bb"]) as h15, Handles(15, 20, d=o15["d"], b=o15["b"]) as h20, \
            Handles(21, bb=np.ones(21, dtype=C128)) as p21:
        assert smw_calls(h20.s, h15.p, 3, 15, 20) == (ARG, ARG)            # nx != nz + 4
        assert smw_calls(h15.s, h15.p, 4, 15, 19) == (ARG, ARG)            # N does not divide nz
        assert smw_calls(h15.s, p21.p, 3, 15, 19) == (ARG, ARG)            # a P^{-1} plan of another nz
        assert smw_calls(None, h15.p, 3, 15, 19) == (ARG, ARG) and smw_calls(h15.s, None, 3, 15, 19) == (ARG, ARG)
        Xd, od, sd, Pd = _sent(15 * 19), _sent(15 * 19), _sent(30), _sent(30)
        cz = _lib.cd(1.0)
        assert lib.nep_wep_schur_matvec(h15.p, _p(sd), 19, _p(Xd), _p(Xd), cz, cz, 1.0, 1.0, 1.0, 1.0, _p(Pd), _p(Xd), st()) == ARG   # dV == dOut
        assert lib.nep_wep_schur_matvec(h15.p, _p(sd), 1, _p(Xd), _p(Xd), cz, cz, 1.0, 1.0, 1.0, 1.0, _p(Pd), _p(od), st()) == ARG    # nx = 1
        assert lib.nep_wep_schur_matvec(None, _p(sd), 19, _p(Xd), _p(Xd), cz, cz, 1.0, 1.0, 1.0, 1.0, _p(Pd), _p(od), st()) == ARG
        assert lib.nep_wep_schur_matvec(h15.p, _p(sd), 19, _p(Xd), _p(Xd), cz, cz, 1.0, 1.0, 1.0, 1.0, None, _p(od), st()) == ARG
        assert lib.nep_wep_sylv_solve(None, _p(Xd), st()) == ARG and lib.nep_wep_sylv_solve(h15.s, None, st()) == ARG
        assert lib.nep_wep_pinv_apply(None, _p(sd), _p(sd), _p(Pd), st()) == ARG and lib.nep_wep_pinv_apply(h15.p, _p(sd), None, _p(Pd), st()) == ARG
        assert lib.nep_wep_pinv_apply(h15.p, None, _p(sd), _p(Pd), st()) == ARG and lib.nep_wep_pinv_apply(h15.p, _p(sd), _p(sd), None, st()) == ARG
        assert lib.nep_wep_region_means(15, 19, 3, None, _p(od), st()) == ARG and lib.nep_wep_region_means(15, 19, 3, _p(Xd), None, st()) == ARG
        assert lib.nep_wep_region_means(15, 20, 3, _p(Xd), _p(od), st()) == ARG and lib.nep_wep_region_means(15, 19, 4, _p(Xd), _p(od), st()) == ARG
        assert lib.nep_wep_region_expand(15, 19, 3, None, _p(Xd), 1.0, 1.0, _p(od), _p(Pd), st()) == ARG
        assert lib.nep_wep_region_expand(15, 19, 4, _p(sd), _p(Xd), 1.0, 1.0, _p(od), _p(Pd), st()) == ARG
        assert lib.nep_wep_smw_matrix(h15.s, h15.p, 3, _p(Xd), 1.0, 1.0, _p(sd), None, _p(od), st()) == ARG
        assert lib.nep_wep_smw_matrix(h15.s, h15.p, 4, _p(Xd), 1.0, 1.0, _p(sd), _p(Xd), _p(od), st()) == ARG
        for t in (Xd, od, sd, Pd):
            assert np.all(_down(t) == SENT)
    assert lib.nep_wep_sylv_destroy(None) == 0 and lib.nep_wep_pinv_destroy(None) == 0


# ---- NEP_WEP_DFT_SYM: read once per process -------------------------------------------------------------------------------------
SYM_VALUES = (0, 23, 42, 43)


def run_child():
    """in the child: assert through nep_wep_plan that the process got the form its NEP_WEP_DFT_SYM names, then the
    nep_wep_sylv_solve and SMW case groups"""
    lib = _L()[1]
    v = int(os.environ["NEP_WEP_DFT_SYM"])

    def plan(nz, nx, op=wc.OP_SYLV):
        info = (C.c_int64 * 8)()
        rc = lib.nep_wep_plan(nz, nx, op, info)
        assert (rc, list(info)) == wc.predict(nz, nx, op, symcfg=v), (nz, nx, op, rc, list(info))
        return rc, list(info)

    if v == 0:
        assert wc.dft_form(plan(105, 109)[1]) == "rb" and wc.dft_form(plan(999, 1003)[1]) == "rb"
        assert wc.dft_form(plan(1443, 7)[1]) == "plain<2>" and plan(1443, 7)[1][6] == 93568
        assert plan(15, 19, wc.OP_SMW)[0] == -5
        o = wc.smw_operands(15)
        with Handles(15, 19, d=o["d"], b=o["b"], bb=o["bb"]) as h:
            st = _L()[2]
            Kd, sd, Md, Gd, Rd, Mo = _up(o["Ksc"]), _up(o["sinv"]), _sent(21 * 21), _sent(45), _sent(15 * 19), _sent(21 * 21)
            assert lib.nep_wep_smw_apply(h.s, h.p, 3, _p(Kd), 1.0, -0.5, _p(sd), _p(Md), _p(Gd), _p(Rd), st()) == -5
            assert lib.nep_wep_smw_matrix_modes(h.s, h.p, 3, _p(Kd), 1.0, -0.5, _p(sd), _p(Gd), _p(Mo), st()) == -5
            assert np.all(_down(Rd) == SENT) and np.all(_down(Mo) == SENT)
        names = ("nep_wep_sylv_solve", "nep_wep_smw_matrix")
    else:
        form = "sym<%d,%d>" % (v // 10, v % 10)
        for nz, nx in ((105, 109), (999, 1003), (1443, 7)):
            assert wc.dft_form(plan(nz, nx)[1]) == form
        if v // 10 == 4:
            assert plan(1443, 7)[1][3] == 4 and plan(1443, 7)[1][6] == 93568 and plan(999, 1003)[1][6] == 64960
        assert plan(1443, 1447, wc.OP_SMW)[1][3:5] == [v // 10, v % 10]
        names = ("nep_wep_sylv_solve", "nep_wep_smw_matrix", "nep_wep_smw_matrix_modes", "nep_wep_smw_apply")
    n = 0
    for name in names:
        for c in wc.CHECKERS[name].cases():
            n += wc.CHECKERS[name].check(IMPL[name], c)
    for k in sorted(pc.RATIOS):
        print("ratio %-40s %.3g" % (k, pc.RATIOS[k]))
    return n


def child_main():
    """entry of a child process: exit 0 with the number of calls passed, 3 after a HIP error (_stop has no pytest session to end
    here), 1 after a failed assertion"""
    try:
        n = run_child()
    except pytest.exit.Exception as e:
        print(e.msg, file=sys.stderr)
        sys.exit(3)
    print("wep calls passed:", n)


def test_dft_sym_forms_in_child_processes(na):
    """NEP_WEP_DFT_SYM = 0 (k_dft_cols_rb at odd factor pairs, no three-transform form), 23, 42, 43 (k_dft_cols_sym<*, 2, 3>,
    <*, 4, 2>, <*, 4, 3>): one fresh child process per value, one after the other; the loop ends at the first child that does not
    exit 0; after a child that died on a signal, reported a HIP error (exit 3) or ran into the time limit, the session ends, so
    nothing more is started on the device"""
    here = os.path.dirname(os.path.abspath(__file__))
    code = ("import sys; sys.path[:0] = [%r, %r]; import test_gpu_wep_checkers as t; t.child_main()"
            % (here, os.path.dirname(here)))
    for v in SYM_VALUES:
        try:
            out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300,
                                 env=dict(os.environ, NEP_WEP_DFT_SYM=str(v)))
        except subprocess.TimeoutExpired as e:
            pytest.exit("the child process with NEP_WEP_DFT_SYM=%d hung (%s): nothing more is started on this device" % (v, e), returncode=3)
        print("NEP_WEP_DFT_SYM=%d\n%s" % (v, out.stdout[-1500:]))
        if out.returncode < 0 or out.returncode in (3, 124, 134, 137, 139):
            pytest.exit("the child process died (%d): nothing more is started on this device\n%s" % (out.returncode, out.stderr[-4000:]),
                        returncode=3)
        assert out.returncode == 0, (v, out.stdout[-2000:], out.stderr[-4000:])
        assert "wep calls passed:" in out.stdout and int(out.stdout.split("wep calls passed:")[1].split()[0]) >= 40, out.stdout[-2000:]
        for line in out.stdout.splitlines():
            if line.startswith("ratio "):
                key = "%s [NEP_WEP_DFT_SYM=%d]" % (line[6:].rsplit(None, 1)[0].strip(), v)
                pc.RATIOS[key] = max(pc.RATIOS.get(key, 0.0), float(line.split()[-1]))


def test_zz_report_wep_ratios(na):
    """the largest |impl - ref| / bound (rounded) and error / allowed error (measured) seen per entry point"""
    seen = {k: v for k, v in pc.RATIOS.items() if k.startswith("nep_wep")}
    for k in sorted(seen):
        print("ratio %-64s %.3g" % (k, seen[k]))
    assert seen and max(seen.values()) <= 1.0
