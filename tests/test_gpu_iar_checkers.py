"""The device infinite-Arnoldi step chain (csrc/driver.hip: nep_iar_create / nep_iar_step / nep_iar_steps / nep_iar_steps_graph /
nep_iar_wait / nep_iar_stream_wait) through the raw C ABI (`nep_amd._lib.lib`) at m = 24, on the chains of tests/iar_checkers.py:
matrices, LU handle, coefficient table and basis are the checker's own data, every delivered step is held to the Krylov relation in
np.clongdouble with the bounds derived there, and the buffers around it to the structure the header promises.
test_host_iar_checkers.py shows that the check passes the float64 model and rejects its mutants."""
import contextlib
import ctypes as ct
import os

import numpy as np
import pytest
import torch

import iar_checkers as ic
import primitive_checkers as pc
from primitive_checkers import C128, SENT

pytestmark = pytest.mark.gpu
CASES = ic.covering_cases()


@pytest.fixture(scope="module")
def na():
    import nep_amd
    if nep_amd.device_count() < 1:
        pytest.skip("no GPU")
    return nep_amd


_DECLARED = []


def _L():
    from nep_amd import _lib
    from nep_amd.nep import stream_ptr
    lib = _lib.lib
    if not _DECLARED:                       # exported, but internal (csrc/iar_run.hip declares it): not in _lib.SIGNATURES
        lib.nep_iar_steps_graph.argtypes = [ct.c_void_p, ct.c_int32, ct.c_int32, ct.c_int32, ct.c_void_p, ct.POINTER(ct.c_int32)]
        lib.nep_iar_steps_graph.restype = ct.c_int32
        _DECLARED.append(True)
    return _lib, lib, stream_ptr


def _stop(what, e):
    pytest.exit("HIP error in %s: %s -- nothing more is started on this device" % (what, e), returncode=3)


def _sync(what):
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:
        _stop(what, e)


def _ok(rc, what):
    _lib = _L()[0]
    if rc == _lib.NEP_ERR_HIP:
        _stop(what, _lib.lib.nep_last_error().decode(errors="replace"))
    assert rc == 0, "%s returned %d: %s" % (what, rc, _lib.lib.nep_last_error().decode(errors="replace"))


@contextlib.contextmanager
def _environment(env):
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


_HANDLES = {}


def _handles(na, n, mt, values):
    """(nep_spmf, nep_lu) of a problem, kept for the module: the real problems must be stored as real values"""
    key = (n, mt, values)
    if key not in _HANDLES:
        p = ic.problem(n, mt, values)
        spmf = na.SPMFDevice(p.A)
        info = (ct.c_int64 * 6)()
        _ok(_L()[1].nep_spmf_info(spmf.h, info), "nep_spmf_info")
        assert (info[0], info[1], info[3]) == (n, mt, 8 if values == "real" else 16), list(info)
        _HANDLES[key] = (spmf, na.DeviceLU(p.M0))
    return _HANDLES[key]


def _p(t):
    return None if t is None else ct.c_void_p(t.data_ptr())


class Chain:
    """the buffers of one nep_iar handle: V with a sentinel row behind its m + 1 columns, dH and the pinned block with a sentinel row
    behind their m rows, 3n of work with ic.TAIL sentinels behind it"""

    def __init__(self, na, c, inputs=None, null=(), change=None):
        _lib, lib, _ = _L()
        self.c, self.lib = c, lib
        p, Ctab, V0 = inputs or ic.case_inputs(c)
        n, m = c.n, c.m
        self.spmf, self.lu = _handles(na, c.n, c.mt, c.values)
        Vh = np.full((m + 2, c.ldv), SENT, dtype=C128); Vh[:m + 1] = V0
        Hh = np.zeros((m + 1, m + 4), dtype=C128); Hh[m] = SENT
        wh = np.full(3 * n + ic.TAIL, SENT, dtype=C128)
        self.host = dict(V=Vh, dH=Hh)
        try:
            self.V, self.H, self.work = (torch.from_numpy(a).to("cuda") for a in (Vh, Hh, wh))
            self.C = torch.from_numpy(np.ascontiguousarray(Ctab.T)).to("cuda")          # column t at t m: ldc = m
            self.act = torch.from_numpy((np.arange(1, m + 2) * n).astype(np.int64)).to("cuda")
        except RuntimeError as e:
            _stop("upload", e)
        self.pin = torch.zeros((m + 1, m + 4), dtype=torch.complex128).pin_memory()
        self.pin[m] = SENT
        self.cabs, self.cf = np.ascontiguousarray(p.cabs), np.ascontiguousarray(p.cf)
        _sync("upload")
        a = dict(spmf=self.spmf.h, lu=self.lu.h, n=n, m=m, dV=_p(self.V), ldv=c.ldv, dCtab=_p(self.C), ldc=m, act=_p(self.act),
                 work=_p(self.work), cabs=_lib.hptr(self.cabs) if c.record else None, cf=_lib.hptr(self.cf) if c.record else None,
                 mt=c.mt, dH=_p(self.H), pin=_p(self.pin), orth=c.orth)
        a.update(change or {})
        for k in null:
            a[k] = None
        self.h = ct.c_void_p(0xdead0)
        with _environment({} if c.fuse else {"NEP_IAR_FUSE_VC": "0"}):
            self.rc = lib.nep_iar_create(a["spmf"], a["lu"], a["n"], a["m"], a["dV"], a["ldv"], a["dCtab"], a["ldc"], a["act"], a["work"],
                                         a["cabs"], a["cf"], a["mt"], a["dH"], a["pin"], a["orth"], None if "out" in null else ct.byref(self.h))

    def close(self):
        _sync("the chain of %r" % (self.c,))
        if self.rc == 0 and self.h:
            assert self.lib.nep_iar_destroy(self.h) == 0
            self.h = None

    def buffers(self):
        _sync("the chain of %r" % (self.c,))
        n = self.c.n
        return dict(V=self.V.cpu().numpy(), dH=self.H.cpu().numpy(), pin=self.pin.numpy().copy(), tail=self.work.cpu().numpy()[3 * n:])

    def unchanged(self):
        b = self.buffers()
        return (ic._same(b["V"], self.host["V"]) and ic._same(b["dH"], self.host["dH"]) and ic._same(b["pin"], self.host["dH"])
                and ic._same(b["tail"], np.full(ic.TAIL, SENT, dtype=C128)))


def run_chain(na, c, route="steps", inputs=None, stream=None):
    """issues the chain of a case by `route` on torch's current stream (or `stream`), waits for every step in order and reads its
    pinned row right behind the wait.  Returns the buffers check_chain takes, plus `captured` for the graph routes."""
    _lib, lib, stream_ptr = _L()
    ch = Chain(na, c, inputs)
    _ok(ch.rc, "nep_iar_create")
    captured = []
    try:
        with (torch.cuda.stream(stream) if stream is not None else contextlib.nullcontext()):
            st, r, k0, cnt = stream_ptr(), c.refine, c.k0, c.count
            if route == "steps":
                _ok(lib.nep_iar_steps(ch.h, k0, cnt, r, st), "nep_iar_steps")
            elif route == "step":
                for k in c.steps:
                    _ok(lib.nep_iar_step(ch.h, k, r, st), "nep_iar_step")
            elif route.startswith("split"):                              # split5 / split4graph: the rest as a second call
                a = int(route[5])
                _ok(lib.nep_iar_steps(ch.h, k0, a, r, st), "nep_iar_steps")
                if route.endswith("graph"):
                    cap = ct.c_int32(-1)
                    _ok(lib.nep_iar_steps_graph(ch.h, k0 + a, cnt - a, r, st, ct.byref(cap)), "nep_iar_steps_graph")
                    captured.append(cap.value)
                else:
                    _ok(lib.nep_iar_steps(ch.h, k0 + a, cnt - a, r, st), "nep_iar_steps")
            elif route == "graph":
                cap = ct.c_int32(-1)
                _ok(lib.nep_iar_steps_graph(ch.h, k0, cnt, r, st, ct.byref(cap)), "nep_iar_steps_graph")
                captured.append(cap.value)
            else:
                raise ValueError(route)
        waited = {}
        for k in c.steps:
            _ok(lib.nep_iar_wait(ch.h, k), "nep_iar_wait")
            waited[k] = ch.pin.numpy()[k - 1].copy()
        out = ch.buffers()
    finally:
        ch.close()
    out.update(waited=waited, captured=captured)
    return out


# ---- the chains of the covering design ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES, ids=[repr(c) for c in CASES])
def test_chain(na, case):
    ic.check_chain(case, run_chain(na, case))
    print("%r: block-0 ratio so far %.3g, shifted-block ratio so far %.3g"
          % (case, pc.RATIOS.get(ic.TAG + " block0", 0.0), pc.RATIOS.get(ic.TAG + " shift", 0.0)))


# ---- one call, many calls, same bits --------------------------------------------------------------------------------------------
def _bits_equal(a, b):
    return all(ic._same(a[k], b[k]) for k in ("V", "dH", "pin", "tail")) and all(ic._same(a["waited"][k], b["waited"][k]) for k in a["waited"])


def test_one_call_many_calls_and_a_graph_give_the_same_bits(na):
    """n = 257, four terms, twelve steps from one seeded column, one refinement sweep with the record: nep_iar_steps(1, 12), twelve
    nep_iar_step calls, nep_iar_steps(1, 5) + nep_iar_steps(6, 7), nep_iar_steps_graph(1, 12) and nep_iar_steps(1, 4) +
    nep_iar_steps_graph(5, 8) on a side stream leave the same bits in dH, the pinned block and V (the wt_for hand-over across calls;
    a capture that is declined falls back to the plain steps from the state the chunk started with), and so does a second run"""
    c = ic.ChainCase(257, 4, "complex", (1, 12), 0, (1, True), 5, True)
    side = torch.cuda.Stream()
    base = run_chain(na, c, "steps", stream=side)
    ic.check_chain(c, base)
    got = {}
    for route in ("steps", "step", "split5", "graph", "split4graph"):
        got[route] = run_chain(na, c, route, stream=side)
        assert _bits_equal(base, got[route]), "route %r differs from nep_iar_steps(1, 12)" % route
    caps = {r: got[r]["captured"] for r in ("graph", "split4graph")}
    print("captured:", caps)
    assert all(v in ([0], [1]) for v in caps.values()), caps
    null = run_chain(na, c, "graph")                                     # the NULL stream cannot be captured
    assert null["captured"] == [0] and _bits_equal(base, null)
    u = ic.ChainCase(257, 5, "complex", (1, 12), 0, (1, True), 5, True)  # the same without the hand-over
    ub = run_chain(na, u, "steps", stream=side)
    ic.check_chain(u, ub)
    for route in ("step", "split5", "split4graph"):
        assert _bits_equal(ub, run_chain(na, u, route, stream=side)), "unfused route %r differs" % route


def test_stream_wait_orders_a_second_stream_behind_the_step(na):
    """twelve steps go out on one stream; a copy of row 11 of dH enqueued on a second stream behind nep_iar_stream_wait(12) reads the
    finished row although nothing else orders the two streams (without the wait the copy runs while step 1 is still in flight)"""
    _lib, lib, stream_ptr = _L()
    c = ic.ChainCase(257, 4, "complex", (1, 12), 0, (0, True), 0, True)
    a, b = torch.cuda.Stream(), torch.cuda.Stream()
    ch = Chain(na, c)
    _ok(ch.rc, "nep_iar_create")
    try:
        dst = torch.zeros(c.m + 4, dtype=torch.complex128, device="cuda")
        _sync("set-up")
        with torch.cuda.stream(a):
            _ok(lib.nep_iar_steps(ch.h, 1, 12, 0, stream_ptr()), "nep_iar_steps")
        with torch.cuda.stream(b):
            _ok(lib.nep_iar_stream_wait(ch.h, 12, stream_ptr()), "nep_iar_stream_wait")
            dst.copy_(ch.H[11], non_blocking=True)
        try:
            b.synchronize()
        except RuntimeError as e:
            _stop("the second stream", e)
        early = ch.pin.numpy()[11].copy()                                # the row was mirrored before the event
        out = ch.buffers()
        row = dst.cpu().numpy()
    finally:
        ch.close()
    assert row[12].real > 0 and ic._same(row, out["dH"][11]) and ic._same(early, out["dH"][11])
    out["waited"] = {k: out["pin"][k - 1] for k in c.steps}
    ic.check_chain(c, out)


# ---- status codes: nothing is launched ------------------------------------------------------------------------------------------
def test_argument_errors_launch_nothing(na):
    _lib, lib, stream_ptr = _L()
    c = ic.ChainCase(65, 4, "complex", (2, 2), 0, (0, False), 5, True)
    ARG = _lib.NEP_ERR_ARG
    n, m = c.n, c.m
    bad = [dict(change={"ldv": n * (m + 1) - 1}), dict(change={"ldc": m - 1}), dict(change={"mt": 0}), dict(change={"m": 0}),
           dict(change={"orth": 2}), dict(change={"n": 0})]
    bad += [dict(null=(k,)) for k in ("spmf", "lu", "dV", "dCtab", "work", "dH", "pin", "out")]
    for how in bad:
        ch = Chain(na, c, **how)
        assert ch.rc == ARG, (how, ch.rc)
        assert ch.h.value is None or "out" in how.get("null", ()), (how, ch.h)      # *out == NULL
        assert ch.unchanged(), how
    for cc in (c, ic.ChainCase(65, 4, "complex", (2, 2), 0, (1, True), 5, True)):
        ch = Chain(na, cc)
        _ok(ch.rc, "nep_iar_create")
        try:
            st = stream_ptr()
            calls = [("step k=0", lib.nep_iar_step(ch.h, 0, 0, st)), ("step k=m+1", lib.nep_iar_step(ch.h, m + 1, 0, st)),
                     ("step refine 4", lib.nep_iar_step(ch.h, 2, 4, st)), ("step refine 4|0x100", lib.nep_iar_step(ch.h, 2, 4 | 0x100, st)),
                     ("step refine -1", lib.nep_iar_step(ch.h, 2, -1, st)),
                     ("steps count 0", lib.nep_iar_steps(ch.h, 2, 0, 0, st)), ("steps count -1", lib.nep_iar_steps(ch.h, 2, -1, 0, st)),
                     ("steps k0=0", lib.nep_iar_steps(ch.h, 0, 1, 0, st)), ("steps k0=m+1", lib.nep_iar_steps(ch.h, m + 1, 1, 0, st)),
                     ("steps_graph count 0", lib.nep_iar_steps_graph(ch.h, 2, 0, 0, st, None)),
                     ("step NULL", lib.nep_iar_step(None, 2, 0, st)), ("steps NULL", lib.nep_iar_steps(None, 2, 1, 0, st)),
                     ("wait NULL", lib.nep_iar_wait(None, 2)), ("stream_wait NULL", lib.nep_iar_stream_wait(None, 2, st))]
            if not cc.record:
                calls += [("step refine 1 without h_cabs", lib.nep_iar_step(ch.h, 2, 1, st)),
                          ("step refine 1|0x100 without h_cabs", lib.nep_iar_step(ch.h, 2, 1 | 0x100, st))]
            for k in (0, m + 1, 2, m):                                   # out of range; never enqueued
                calls += [("wait k=%d" % k, lib.nep_iar_wait(ch.h, k)), ("stream_wait k=%d" % k, lib.nep_iar_stream_wait(ch.h, k, st))]
            for what, rc in calls:
                assert rc == ARG, (cc, what, rc)
            assert ch.unchanged(), cc
            # the handle is intact: the chain of the case goes through it and passes the check
            _ok(lib.nep_iar_steps(ch.h, cc.k0, cc.count, cc.refine, st), "nep_iar_steps")
            waited = {}
            for k in cc.steps:
                _ok(lib.nep_iar_wait(ch.h, k), "nep_iar_wait")
                waited[k] = ch.pin.numpy()[k - 1].copy()
            assert lib.nep_iar_wait(ch.h, cc.k0 + cc.count) == ARG
            out = ch.buffers()
        finally:
            ch.close()
        out["waited"] = waited
        ic.check_chain(cc, out)
    assert lib.nep_iar_destroy(None) == _lib.NEP_OK


def test_zz_report(na):
    print("chains checked per factor value:")
    for f, name in enumerate(ic.FACTOR_NAMES):
        print("  %-7s %s" % (name, "  ".join("%s: %d" % (v, ic.COUNTS.get((name, v), 0)) for v in ic.FACTORS[f])))
    b0, sh = pc.RATIOS.get(ic.TAG + " block0", 0.0), pc.RATIOS.get(ic.TAG + " shift", 0.0)
    print("largest ratios: block 0 %.3g, shifted blocks %.3g, ||V^H V - I||_2 / 1e-12 %.3g"
          % (b0, sh, pc.RATIOS.get(ic.TAG + " orthogonality / 1e-12", 0.0)))
    assert b0 <= 1.0 and sh <= 1.0
