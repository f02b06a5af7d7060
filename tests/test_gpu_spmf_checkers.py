"""Exact and bounded parity tests of the SPMF kernels (K1, K2, K11 and the componentwise backward error: csrc/spmv.hip,
csrc/spmv_tile.hip, csrc/lrprod.hip) on the synthetic recipes of tests/spmf_checkers.py, through the raw C ABI
(`nep_amd._lib.lib`).

One handle per recipe; all of its cases run on it through adapters that upload flat buffers, under the K1 modes 0 / 1 / 2 and the
super-panel modes 0 / 2.  After every call nep_spmf_plan says which kernel instantiation the dispatch chose; the closing test
compares the set of plans seen with the explicit table PLANS.  Knobs the library reads once per process run in child processes,
knobs read by nep_spmf_create are set around the create call.  test_host_spmf_checkers.py shows that these checkers reject
mutants and that the recipes have the tile structure they are named for."""
import ctypes as C
import json
import os
from functools import partial
import subprocess
import sys

import numpy as np
import pytest
import torch

import primitive_checkers as pc
import spmf_checkers as sc
from primitive_checkers import C128, SENT, NAN, colmajor_buf

pytestmark = pytest.mark.gpu
SEEN = set()                                                # plans recorded in this process and reported by the children
PANELS = {}                                                 # op -> largest number of column panels seen
TILE_ENV = ("NEP_K1_TILE_XP", "NEP_K1_TILE_ZP", "NEP_K1_TILE_LDS_KB", "NEP_K1_TILE_STRIDE", "NEP_TILE_SLOTTED", "NEP_SELL", "NEP_SPMV_LANES")
OP_K1, OP_NORMS, OP_BLOCK, OP_CM = 0, 1, 2, 3


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


def _down(t):
    torch.cuda.synchronize()
    return t.cpu().numpy()


class Handle:
    """nep_spmf handle of a recipe, created under `env` (the knobs nep_spmf_create reads), with the adapters of sc.check"""

    def __init__(self, rec, env, monkeypatch):
        _lib, lib, _ = _L()
        for k in TILE_ENV:
            monkeypatch.delenv(k, raising=False)
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        self.rec = rec
        self.h = C.c_void_p()
        rp, ci, vv, isc = rec.ptr_arrays()
        _lib.check(lib.nep_spmf_create(rec.n, rec.mt, rp, ci, vv, isc, C.byref(self.h)))
        info = (C.c_int64 * 6)()
        _lib.check(lib.nep_spmf_info(self.h, info))
        assert list(info)[:4] == [rec.n, rec.mt, rec.nnz, 16 if rec.any_complex else 8], list(info)
        self.lanes = int(info[4])
        ti = (C.c_int64 * 8)()
        _lib.check(lib.nep_spmf_tile_info(self.h, ti))
        dry, _ = sc.tiles_analyze(lib, rec, 3)                   # the same environment: the device tiles are the dry run's
        self.fcap_seen = dry[1]
        dry[1] = (dry[1] + 15) // 16 * 16                        # (the handle reports the footprint capacity, a multiple of 16)
        assert list(ti) == dry, (list(ti), dry)
        self.tiles = None if ti[0] == 0 else (int(ti[0]), int(ti[2]), int(ti[3]), int(ti[4]), self.fcap_seen)
        for k in env:
            monkeypatch.delenv(k, raising=False)
        sc._count("nep_spmf_create", "exact"); sc._count("nep_spmf_info", "exact"); sc._count("nep_spmf_tile_info", "exact")

    def close(self):
        _L()[1].nep_spmf_destroy(self.h)

    def plan(self, op, k):
        _lib, lib, _ = _L()
        info = (C.c_int64 * 8)()
        rc = lib.nep_spmf_plan(self.h, op, k, info)
        if rc == 0:
            SEEN.add((op,) + tuple(int(x) for x in info)[:7])
            PANELS[op] = max(PANELS.get(op, 0), int(info[7]))
        return rc, [int(x) for x in info]

    # ---- adapters: impl(op, rec, args) -> dict of host buffers ------------------------------------------------------------
    def __call__(self, op, rec, a):
        try:
            return getattr(self, "_" + op)(a)
        except RuntimeError as e:                                # a HIP error (the library's status -1, or torch's own): the device may
            if getattr(e, "status", -1) == -1:                   # have faulted, so nothing more is started on it in this session
                pytest.exit("HIP error in %s on %s: %s" % (op, rec.name, e), returncode=3)
            raise

    def _k1(self, a):
        _lib, lib, st = _L()
        n, k, lead = self.rec.n, a["k"], a["lead"]
        Vd = _up(a["V"])
        hC = np.ascontiguousarray(a["C"].T).reshape(-1)           # k x mt column-major
        dC = _up(colmajor_buf(a["C"], a["ldc"]))
        outs = {}
        for key in ("z", "z_dev", "z_again"):
            zd = _up(np.full(lead + n + 2, SENT, dtype=C128))
            if key == "z_dev":
                _lib.check(lib.nep_mlincomb_dev(self.h, k, _p(dC), a["ldc"], _p(Vd), a["ldv"], _p(zd, lead), st()))
            else:
                _lib.check(lib.nep_mlincomb(self.h, k, _lib.hptr(hC), _p(Vd), a["ldv"], _p(zd, lead), st()))
            outs[key] = _down(zd)
        outs["V_after"] = _down(Vd)
        self.plan(OP_K1, k)
        return outs

    def _k2(self, a):
        _lib, lib, st = _L()
        n, k, mt, row0 = self.rec.n, a["k"], self.rec.mt, a["row0"]
        Qd = _up(a["Q"])
        hF = np.ascontiguousarray(a["F"].T).reshape(-1)           # mt x k column-major
        rn = np.full(k, -1.0); qn = np.full(k, -1.0)
        _lib.check(lib.nep_resid_batch(self.h, k, _lib.hptr(hF), _p(Qd), a["ldq"], _lib.hptr(rn), _lib.hptr(qn), st()))
        d1 = torch.full((2 * k,), -1.0, dtype=torch.float64, device="cuda")
        _lib.check(lib.nep_resid_batch_dev(self.h, k, _lib.hptr(hF), _p(Qd), a["ldq"], C.c_void_p(d1.data_ptr()), st()))
        d2 = torch.full((2 * k,), -1.0, dtype=torch.float64, device="cuda")
        td = _up(np.full((n - row0) * a["ldt"] + 1, SENT, dtype=C128))
        _lib.check(lib.nep_resid_split_dev(self.h, k, _lib.hptr(hF), _p(Qd), a["ldq"], row0, C.c_void_p(d2.data_ptr()), _p(td), a["ldt"], st()))
        out = dict(rnorm=rn, qnorm=qn, d_out=_down(d1), split_out=_down(d2), tail=_down(td))
        bd = _up(np.full(n * a["ldr"], SENT, dtype=C128))
        out["block_status"] = lib.nep_resid_block(self.h, k, _lib.hptr(hF), _p(Qd), a["ldq"], _p(bd), a["ldr"], st())
        got = _down(bd)
        if out["block_status"] == 0:
            out["block"] = got
            self.plan(OP_BLOCK, k)
        else:
            assert np.array_equal(got, np.full(n * a["ldr"], SENT, dtype=C128)), "a refused nep_resid_block wrote"
            assert self.plan(OP_BLOCK, k)[0] == -2
        assert np.array_equal(_down(Qd), a["Q"], equal_nan=True), "K2 changed Q"
        self.plan(OP_NORMS, k)
        return out

    def _k2cm(self, a):
        _lib, lib, st = _L()
        n, k, row0 = self.rec.n, a["k"], a["row0"]
        Qd = _up(a["Q"])
        hF = np.ascontiguousarray(a["F"].T).reshape(-1)
        d1 = torch.full((2 * k,), -1.0, dtype=torch.float64, device="cuda")
        td = _up(np.full(a["ldt"] * k + 1, SENT, dtype=C128)) if row0 >= 0 else None
        rc = lib.nep_resid_batch_cm_dev(self.h, k, _lib.hptr(hF), _p(Qd), a["ldq"], row0, C.c_void_p(d1.data_ptr()),
                                        _p(td) if td is not None else None, a["ldt"], st())
        prc, _ = self.plan(OP_CM, k)
        assert prc == rc, (prc, rc)
        out = dict(status=rc)
        if rc == 0:
            out["d_out"] = _down(d1)
            if td is not None:
                out["tail"] = _down(td)
        else:
            assert np.array_equal(_down(d1), np.full(2 * k, -1.0))
        return out

    def _k11(self, a):
        _lib, lib, st = _L()
        Wd, Bd, Td = _up(a["W"]), _up(a["B"]), _up(a["tau"])
        hc = np.full(1, SENT, dtype=C128)
        _lib.check(lib.nep_lr_hankel(self.h, a["ma"], a["mb"], _p(Wd), a["ldw"], _p(Bd), a["ldb"], _p(Td), a["ldt"], _lib.hptr(hc), None, st()))
        dc = _up(np.full(3, SENT, dtype=C128))
        _lib.check(lib.nep_lr_hankel(self.h, a["ma"], a["mb"], _p(Wd), a["ldw"], _p(Bd), a["ldb"], _p(Td), a["ldt"], None, _p(dc, 1), st()))
        got = _down(dc)
        assert got[0] == SENT and got[2] == SENT
        return dict(c_host=complex(hc[0]), c_dev=complex(got[1]))

    def _cw(self, a):
        _lib, lib, st = _L()
        n = self.rec.n
        xd, bd, Md = _up(a["x"]), _up(a["b"]), _up(a["Mx"])
        ed = _up(a["extra"]) if a["extra"] is not None else None
        cabs = np.ascontiguousarray(a["cabs"], dtype=np.float64); cc = np.ascontiguousarray(a["c"], dtype=C128)
        out = {}
        for fused, rk, ok in ((True, "r_fused", "om_fused"), (False, "r_mx", "om_mx")):
            rd = _up(np.full(n + 2, SENT, dtype=C128))
            om = C.c_double(-1.0)
            _lib.check(lib.nep_cw_backward_error(self.h, _lib.hptr(cabs), _lib.hptr(cc) if fused else None, _p(xd), _p(bd), None if fused else _p(Md),
                                                 _p(ed) if ed is not None else None, _p(rd, 1), C.byref(om), st()))
            got = _down(rd)
            assert got[0] == SENT and got[-1] == SENT
            out[rk] = got[1:-1]; out[ok] = om.value
        return out


K1_MODES = (0, 1, 2)
K2_MODES = ((0, -1), (1, 0), (1, 2), (2, 0), (2, 2))


def run_recipe(name, monkeypatch, env=None, kinds=("exact", "rounded"), ops=sc.OPS, k1_modes=K1_MODES, k2_modes=K2_MODES, hook=None, cases=None):
    """every case of the recipe on one handle: K1 under the three K1 modes, K2 (row- and column-major) under automatic choice and
    under super-panel modes 0 / 2 crossed with K1 modes 1 / 2, K11 and the backward error once"""
    _lib, lib, _ = _L()
    spec = sc.RECIPES[name]
    hs = {}
    n = 0
    try:
        for c in (sc.cases(name) if cases is None else cases):
            op = c.extra["op"]
            if c.kind not in kinds or op not in ops:
                continue
            if c.kind not in hs:
                hs[c.kind] = Handle(sc.make_recipe(name, c.kind), spec.env if env is None else env, monkeypatch)
                if env is None:
                    assert hs[c.kind].tiles == spec.tiles, (name, hs[c.kind].tiles, spec.tiles)
                    lib.nep_k2_set_sp_mode(2)                    # the flush mask of the slot layout, or no super-panel kernel at all
                    rc, info = hs[c.kind].plan(OP_NORMS, 4)
                    lib.nep_k2_set_sp_mode(-1)
                    assert (info[6] if info[0] == 8 else None) == spec.slotted, (name, info, spec.slotted)
                if hook:
                    hook(hs[c.kind])
            h = hs[c.kind]
            a = c.args
            cache = {}
            modes = [(m, -1) for m in k1_modes] if op == "k1" else list(k2_modes) if op in ("k2", "k2cm") else [(0, -1)]
            for m1, m2 in modes:
                lib.nep_k1_set_mode(m1); lib.nep_k2_set_sp_mode(m2)
                n += sc.check(h, c, args=a, cache=cache)
    finally:
        lib.nep_k1_set_mode(0); lib.nep_k2_set_sp_mode(-1)
        for h in hs.values():
            h.close()
    return n


@pytest.mark.parametrize("name", list(sc.RECIPES))
def test_spmf_recipe(na, name, monkeypatch):
    n = run_recipe(name, monkeypatch)
    assert n >= 16, (name, n)


# ---- knobs read by nep_spmf_create ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lanes", [2, 4, 8, 16, 32, 64])
def test_spmv_lanes(na, lanes, monkeypatch):
    """NEP_SPMV_LANES = 2 .. 64: k_spmv_fold (k = 1), k_spmv_kfused (2 <= k <= 16), k_vc + k_spmv (k >= 17) and k_cw_resid with
    every lane count, real and complex values, on rows of 5 .. 8 and of 0 .. 300 entries"""
    def hook(h):
        assert h.lanes == lanes
    for name in ("grid5/61x37", "grid5/61x37_real", "wide/n403"):
        assert run_recipe(name, monkeypatch, env=dict(NEP_SPMV_LANES=str(lanes)), kinds=("exact",), ops=("k1", "cw"), k1_modes=(2,), hook=hook) >= 16


@pytest.mark.parametrize("name,env", [("grid5/61x37", dict(NEP_SELL="1")), ("grid5/61x37_real", dict(NEP_SELL="1")), ("wide/n403", dict(NEP_SELL="1")),
                                      ("degenerate/empty_rows", dict(NEP_SELL="1")), ("grid5/251x131", dict(NEP_SELL="0")),
                                      ("grid5/61x37", dict(NEP_TILE_SLOTTED="0")), ("grid5/251x131", dict(NEP_TILE_SLOTTED="0")),
                                      ("grid5/61x37", dict(NEP_K1_TILE_XP="8", NEP_K1_TILE_ZP="32")), ("grid5/251x131", dict(NEP_K1_TILE_LDS_KB="8")),
                                      ("grid5/61x37", dict(NEP_K1_TILE_LDS_KB="4"))],
                         ids=lambda v: v if isinstance(v, str) else ",".join("%s=%s" % (k.replace("NEP_", ""), x) for k, x in v.items()))
def test_create_time_knobs(na, name, env, monkeypatch):
    """the SELL copy forced on small matrices (k_spmv_sell in its three forms at every n of the recipe) and off on a large one (CSR
    kernels and no tiled K1 in automatic mode at n >= 32768), unslotted tiles (the super-panel kernels must be refused), other patch
    shapes and a smaller footprint budget (more, smaller blocks: the handle's tiles are asserted equal to the host dry run)"""
    seen = []
    n = run_recipe(name, monkeypatch, env=env, kinds=("exact",), hook=seen.append)
    assert n >= 16
    h = seen[0]
    if "NEP_K1_TILE_LDS_KB" in env:
        assert h.tiles is not None and h.tiles[0] > sc.RECIPES[name].tiles[0] and h.tiles[4] < sc.RECIPES[name].tiles[4], h.tiles
    if "NEP_K1_TILE_ZP" in env:
        assert h.tiles[2:4] == (8, 32), h.tiles


def test_argument_checks_launch_nothing(na, monkeypatch):
    """k < 1, leading dimensions below their minimum, row0 > n, NULL outputs: NEP_ERR_ARG and every output buffer untouched"""
    _lib, lib, st = _L()
    rec = sc.make_recipe("grid5/61x37", "exact")
    h = Handle(rec, {}, monkeypatch)
    n, mt, k = rec.n, rec.mt, 3
    try:
        Vd = _up(np.ones(n * k, dtype=C128)); zd = _up(np.full(n * k + 8, SENT, dtype=C128))
        dd = torch.full((2 * k,), -1.0, dtype=torch.float64, device="cuda")
        dp = C.c_void_p(dd.data_ptr())
        hC = np.ones(k * mt, dtype=C128); hp = _lib.hptr
        two = np.full(2 * k, -1.0)
        bad = [
            lib.nep_mlincomb(h.h, 0, hp(hC), _p(Vd), n, _p(zd), st()),
            lib.nep_mlincomb(h.h, k, hp(hC), _p(Vd), n - 1, _p(zd), st()),
            lib.nep_mlincomb(h.h, k, hp(hC), _p(Vd), n, None, st()),
            lib.nep_mlincomb(h.h, k, None, _p(Vd), n, _p(zd), st()),
            lib.nep_mlincomb_dev(h.h, k, _p(Vd), k - 1, _p(Vd), n, _p(zd), st()),
            lib.nep_mlincomb_dev(h.h, -1, _p(Vd), k, _p(Vd), n, _p(zd), st()),
            lib.nep_resid_batch(h.h, 0, hp(hC), _p(Vd), k, hp(two), hp(two[k:]), st()),
            lib.nep_resid_batch(h.h, k, hp(hC), _p(Vd), k - 1, hp(two), hp(two[k:]), st()),
            lib.nep_resid_batch(h.h, k, hp(hC), _p(Vd), k, None, hp(two[k:]), st()),
            lib.nep_resid_batch_dev(h.h, k, hp(hC), _p(Vd), k - 1, dp, st()),
            lib.nep_resid_batch_dev(h.h, k, hp(hC), _p(Vd), k, None, st()),
            lib.nep_resid_split_dev(h.h, k, hp(hC), _p(Vd), k, n + 1, dp, _p(zd), k, st()),
            lib.nep_resid_split_dev(h.h, k, hp(hC), _p(Vd), k, -1, dp, _p(zd), k, st()),
            lib.nep_resid_split_dev(h.h, k, hp(hC), _p(Vd), k, n - 2, dp, _p(zd), k - 1, st()),
            lib.nep_resid_split_dev(h.h, k, hp(hC), _p(Vd), k, n - 2, dp, None, k, st()),
            lib.nep_resid_batch_cm_dev(h.h, k, hp(hC), _p(Vd), n - 1, -1, dp, None, 0, st()),
            lib.nep_resid_batch_cm_dev(h.h, 0, hp(hC), _p(Vd), n, -1, dp, None, 0, st()),
            lib.nep_resid_batch_cm_dev(h.h, k, hp(hC), _p(Vd), n, n + 1, dp, _p(zd), 1, st()),
            lib.nep_resid_batch_cm_dev(h.h, k, hp(hC), _p(Vd), n, n - 2, dp, None, 2, st()),
            lib.nep_resid_batch_cm_dev(h.h, k, hp(hC), _p(Vd), n, n - 2, dp, _p(zd), 1, st()),
            lib.nep_resid_block(h.h, k, hp(hC), _p(Vd), k, _p(zd), k - 1, st()),
            lib.nep_resid_block(h.h, k, hp(hC), _p(Vd), k, None, k, st()),
            lib.nep_resid_block(h.h, 257, hp(hC), _p(Vd), 257, _p(zd), 257, st()),
            lib.nep_lr_hankel(h.h, 0, 1, _p(Vd), n, _p(Vd), n, _p(Vd), 4, None, _p(zd), st()),
            lib.nep_lr_hankel(h.h, 1, 1, _p(Vd), n - 1, _p(Vd), n, _p(Vd), 4, None, _p(zd), st()),
            lib.nep_lr_hankel(h.h, 1, 2, _p(Vd), n, _p(Vd), n, _p(Vd), 2, None, _p(zd), st()),
            lib.nep_lr_hankel(h.h, 1, 1, _p(Vd), n, _p(Vd), n, _p(Vd), 4, None, None, st()),
            lib.nep_cw_backward_error(h.h, hp(two), hp(hC), _p(Vd), _p(Vd), _p(Vd), None, _p(zd), None, st()),     # both forms of M x at once
            lib.nep_cw_backward_error(h.h, hp(two), None, _p(Vd), _p(Vd), None, None, _p(zd), None, st()),         # neither
            lib.nep_cw_backward_error(h.h, hp(two), hp(hC), _p(Vd), _p(Vd), None, None, None, None, st()),
            lib.nep_spmf_plan(h.h, 0, 0, (C.c_int64 * 8)()), lib.nep_spmf_plan(h.h, 4, 1, (C.c_int64 * 8)()),
            lib.nep_spmf_plan(h.h, OP_BLOCK, 257, (C.c_int64 * 8)()),
        ]
        assert bad == [-2] * len(bad), bad
        assert lib.nep_lr_hankel(h.h, 257, 1, _p(Vd), n, _p(Vd), n, _p(Vd), 300, None, _p(zd), st()) == -5
        torch.cuda.synchronize()
        assert np.array_equal(zd.cpu().numpy(), np.full(n * k + 8, SENT, dtype=C128)) and np.array_equal(dd.cpu().numpy(), two)
        assert np.array_equal(two, np.full(2 * k, -1.0))
    finally:
        h.close()


# ---- switches cached in a static on first use: a fresh child process per setting ------------------------------------------------
CHILD_RECIPES = ("grid5/61x37", "grid5/251x131")
CHILDREN = [dict(NEP_K2_TILE_PS="4", NEP_K2_CM_PS="4"), dict(NEP_K2_CM_PS="8", NEP_VC_ROWS="16"), dict(NEP_K2_SP_PERSIST="2"), dict(NEP_K2_SP_RING="4"),
            dict(NEP_K1_TILE_PF="0", NEP_XCD_SWIZZLE="0"), dict(NEP_K1_FUSE_MAX="0", NEP_SPMM_GROUPED="0"), dict(NEP_K1_FUSE_MAX="16")]


def run_child():
    """in the child: the exact cases of the two grid recipes; prints the plans it saw"""
    mp = pytest.MonkeyPatch()
    n = 0
    try:
        for name in CHILD_RECIPES:
            n += run_recipe(name, mp, kinds=("exact",), ops=("k1", "k2", "k2cm"))
        if os.environ.get("NEP_K1_FUSE_MAX") == "16":           # k_spmv_sell_kfused<K>: every K, real and complex values (mode 2: no tiles)
            for name in ("grid5/251x131", "grid5/251x131_real"):
                extra = [pc.Case(name, "k1/k%d_fused" % k, "exact", partial(sc._k1_args, name, "exact", k, "padded"), extra=dict(op="k1", k=k))
                         for k in range(2, 17)]
                n += run_recipe(name, mp, kinds=("exact",), ops=("k1",), k1_modes=(2,), cases=extra)
    finally:
        mp.undo()
    print("spmf plans:", json.dumps(sorted(SEEN)))
    print("spmf panels:", json.dumps(PANELS))
    return n


def _child(env):
    """one child process after another, each with a time limit; a child that died of a signal ends the session: nothing more is
    started on the device"""
    here = os.path.dirname(os.path.abspath(__file__))
    code = ("import sys; sys.path[:0] = [%r, %r]; import test_gpu_spmf_checkers as t; n = t.run_child(); print('spmf calls passed:', n)"
            % (here, os.path.dirname(here)))
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=600, env=dict(os.environ, **env))
    if out.returncode < 0 or out.returncode in (124, 134, 137, 139):
        pytest.exit("the child process died (%d): nothing more is started on this device\n%s" % (out.returncode, out.stderr[-4000:]), returncode=3)
    assert out.returncode == 0, (out.stdout[-2000:], out.stderr[-4000:])
    assert "spmf calls passed:" in out.stdout and int(out.stdout.split("spmf calls passed:")[1].split()[0]) >= 200, out.stdout[-2000:]
    return [tuple(p) for p in json.loads(out.stdout.split("spmf plans:")[1].splitlines()[0])]


@pytest.mark.parametrize("env", CHILDREN, ids=lambda e: ",".join("%s=%s" % (k.replace("NEP_", ""), v) for k, v in e.items()))
def test_process_wide_knobs_in_a_child_process(na, env):
    """NEP_K2_TILE_PS / NEP_K2_CM_PS (tile panels of 4 and 8 columns), NEP_VC_ROWS = 16, the persistent and the ring-of-four
    super-panel kernels, no register prefetch, no XCD swizzle, no fused K1, no grouped-gather SpMM: each is read once per process"""
    plans = _child(env)
    kernels = {p[1] for p in plans}
    width = {(p[0], p[1], p[6]) for p in plans}
    if env.get("NEP_K2_TILE_PS") == "4":
        assert {w for (o, kn, w) in width if kn == 7} == {4} and {w for (o, kn, w) in width if kn == 10} == {4}, sorted(width)
    if env.get("NEP_K2_CM_PS") == "8":
        assert {w for (o, kn, w) in width if kn == 10} == {8}, sorted(width)
    if "NEP_VC_ROWS" in env:
        assert {p[7] for p in plans if p[1] == 3} == {16}
    if "NEP_K2_SP_PERSIST" in env:
        assert 9 in kernels
    if "NEP_K2_SP_RING" in env:
        assert 11 in kernels
    if "NEP_K1_TILE_PF" in env:
        assert not any(p[4] & 4 for p in plans)
    if env.get("NEP_K1_FUSE_MAX") == "0":
        assert 2 not in kernels and any(p[1] == 6 and p[6] in (1, 2) for p in plans)
    if env.get("NEP_K1_FUSE_MAX") == "16":
        assert {p[2] for p in plans if p[1] == 2 and p[4] & 1} == {8, 16}, sorted(plans)      # the fused SELL kernel, both value types
    SEEN.update(plans)


# ---- what ran ------------------------------------------------------------------------------------------------------------------
# (op, kernel, value bytes, terms unrolled, flags, threads, lanes | chunks | panel width, flush mask | rows of k_vc): every
# instantiation the cases above are meant to reach (NEP_PLAN_* of include/nepmi355.h)
PLANS = {
    # K1: k_spmv_fold / k_spmv_sell (fold)
    (0, 1, 8, 1, 0, 256, 4, 0), (0, 1, 8, 1, 0, 256, 8, 0), (0, 1, 8, 1, 1, 256, 64, 0), (0, 1, 8, 2, 1, 256, 64, 0),
    (0, 1, 8, 3, 0, 256, 2, 0), (0, 1, 8, 3, 0, 256, 4, 0), (0, 1, 8, 3, 0, 256, 8, 0), (0, 1, 8, 3, 0, 256, 16, 0),
    (0, 1, 8, 3, 0, 256, 32, 0), (0, 1, 8, 3, 0, 256, 64, 0), (0, 1, 8, 3, 1, 256, 64, 0), (0, 1, 8, 4, 1, 256, 64, 0),
    (0, 1, 8, 5, 1, 256, 64, 0), (0, 1, 16, 1, 0, 256, 4, 0), (0, 1, 16, 1, 0, 256, 8, 0), (0, 1, 16, 1, 1, 256, 64, 0),
    (0, 1, 16, 2, 0, 256, 2, 0), (0, 1, 16, 2, 0, 256, 4, 0), (0, 1, 16, 2, 0, 256, 8, 0), (0, 1, 16, 2, 0, 256, 16, 0),
    (0, 1, 16, 2, 0, 256, 32, 0), (0, 1, 16, 2, 0, 256, 64, 0), (0, 1, 16, 2, 1, 256, 64, 0), (0, 1, 16, 3, 0, 256, 2, 0),
    (0, 1, 16, 3, 0, 256, 4, 0), (0, 1, 16, 3, 0, 256, 8, 0), (0, 1, 16, 3, 0, 256, 16, 0), (0, 1, 16, 3, 0, 256, 32, 0),
    (0, 1, 16, 3, 0, 256, 64, 0), (0, 1, 16, 3, 1, 256, 64, 0), (0, 1, 16, 4, 0, 256, 8, 0), (0, 1, 16, 4, 0, 256, 16, 0),
    (0, 1, 16, 4, 0, 256, 64, 0), (0, 1, 16, 4, 1, 256, 64, 0), (0, 1, 16, 5, 0, 256, 16, 0), (0, 1, 16, 7, 1, 256, 64, 0),
    (0, 1, 16, 8, 0, 256, 32, 0), (0, 1, 16, 9, 0, 256, 32, 0), (0, 1, 16, 16, 0, 256, 32, 0), (0, 1, 16, 33, 0, 256, 64, 0),
    (0, 1, 16, 128, 0, 256, 64, 0),
    # K1: k_spmv_kfused / k_spmv_sell_kfused
    (0, 2, 8, 1, 0, 256, 4, 0), (0, 2, 8, 1, 0, 256, 8, 0), (0, 2, 8, 3, 0, 256, 2, 0), (0, 2, 8, 3, 0, 256, 4, 0),
    (0, 2, 8, 3, 0, 256, 8, 0), (0, 2, 8, 3, 0, 256, 16, 0), (0, 2, 8, 3, 0, 256, 32, 0), (0, 2, 8, 3, 0, 256, 64, 0),
    (0, 2, 8, 3, 1, 256, 64, 0), (0, 2, 16, 1, 0, 256, 4, 0), (0, 2, 16, 1, 0, 256, 8, 0), (0, 2, 16, 2, 0, 256, 2, 0),
    (0, 2, 16, 2, 0, 256, 4, 0), (0, 2, 16, 2, 0, 256, 8, 0), (0, 2, 16, 2, 0, 256, 16, 0), (0, 2, 16, 2, 0, 256, 32, 0),
    (0, 2, 16, 2, 0, 256, 64, 0), (0, 2, 16, 3, 0, 256, 2, 0), (0, 2, 16, 3, 0, 256, 4, 0), (0, 2, 16, 3, 0, 256, 8, 0),
    (0, 2, 16, 3, 0, 256, 16, 0), (0, 2, 16, 3, 0, 256, 32, 0), (0, 2, 16, 3, 0, 256, 64, 0), (0, 2, 16, 3, 1, 256, 64, 0),
    (0, 2, 16, 4, 0, 256, 8, 0), (0, 2, 16, 4, 0, 256, 16, 0), (0, 2, 16, 4, 0, 256, 64, 0), (0, 2, 16, 5, 0, 256, 16, 0),
    (0, 2, 16, 8, 0, 256, 8, 0), (0, 2, 16, 8, 0, 256, 32, 0), (0, 2, 16, 9, 0, 256, 32, 0), (0, 2, 16, 16, 0, 256, 32, 0),
    (0, 2, 16, 33, 0, 256, 64, 0), (0, 2, 16, 128, 0, 256, 64, 0),
    # K1: k_vc + k_spmv / k_spmv_sell
    (0, 3, 8, 1, 0, 256, 4, 32), (0, 3, 8, 1, 0, 256, 8, 32), (0, 3, 8, 1, 1, 256, 64, 32), (0, 3, 8, 2, 1, 256, 64, 32),
    (0, 3, 8, 2, 1, 256, 64, 64), (0, 3, 8, 3, 0, 256, 2, 32), (0, 3, 8, 3, 0, 256, 4, 32), (0, 3, 8, 3, 0, 256, 8, 32),
    (0, 3, 8, 3, 0, 256, 16, 32), (0, 3, 8, 3, 0, 256, 32, 32), (0, 3, 8, 3, 0, 256, 64, 32), (0, 3, 8, 3, 1, 256, 64, 32),
    (0, 3, 8, 4, 1, 256, 64, 32), (0, 3, 8, 4, 1, 256, 64, 64), (0, 3, 16, 1, 0, 256, 4, 32), (0, 3, 16, 1, 0, 256, 8, 32),
    (0, 3, 16, 1, 1, 256, 64, 32), (0, 3, 16, 2, 0, 256, 2, 32), (0, 3, 16, 2, 0, 256, 4, 32), (0, 3, 16, 2, 0, 256, 8, 32),
    (0, 3, 16, 2, 0, 256, 16, 32), (0, 3, 16, 2, 0, 256, 32, 32), (0, 3, 16, 2, 0, 256, 64, 32), (0, 3, 16, 2, 1, 256, 64, 32),
    (0, 3, 16, 3, 0, 256, 2, 32), (0, 3, 16, 3, 0, 256, 4, 32), (0, 3, 16, 3, 0, 256, 8, 16), (0, 3, 16, 3, 0, 256, 8, 32),
    (0, 3, 16, 3, 0, 256, 16, 32), (0, 3, 16, 3, 0, 256, 32, 32), (0, 3, 16, 3, 0, 256, 64, 32), (0, 3, 16, 3, 1, 256, 64, 16),
    (0, 3, 16, 3, 1, 256, 64, 32), (0, 3, 16, 4, 0, 256, 8, 32), (0, 3, 16, 4, 0, 256, 16, 32), (0, 3, 16, 4, 0, 256, 32, 32),
    (0, 3, 16, 4, 0, 256, 64, 32), (0, 3, 16, 4, 1, 256, 64, 32), (0, 3, 16, 4, 1, 256, 64, 64),
    # K1: k_tile_mlincomb
    (0, 4, 8, 1, 0, 256, 0, 0), (0, 4, 8, 1, 3, 256, 0, 0), (0, 4, 8, 1, 7, 256, 0, 0), (0, 4, 8, 1, 8, 256, 0, 0),
    (0, 4, 8, 1, 8, 512, 0, 0), (0, 4, 8, 2, 3, 256, 0, 0), (0, 4, 8, 2, 7, 256, 0, 0), (0, 4, 8, 3, 0, 256, 0, 0),
    (0, 4, 8, 3, 1, 256, 0, 0), (0, 4, 8, 3, 3, 256, 0, 0), (0, 4, 8, 3, 8, 256, 0, 0), (0, 4, 8, 3, 8, 512, 0, 0),
    (0, 4, 8, 3, 8, 1024, 0, 0), (0, 4, 8, 3, 9, 256, 0, 0), (0, 4, 8, 3, 9, 512, 0, 0), (0, 4, 8, 3, 9, 1024, 0, 0),
    (0, 4, 8, 4, 7, 256, 0, 0), (0, 4, 16, 1, 0, 256, 0, 0), (0, 4, 16, 1, 0, 512, 0, 0), (0, 4, 16, 1, 0, 1024, 0, 0),
    (0, 4, 16, 1, 3, 256, 0, 0), (0, 4, 16, 1, 7, 256, 0, 0), (0, 4, 16, 1, 8, 256, 0, 0), (0, 4, 16, 1, 8, 512, 0, 0),
    (0, 4, 16, 1, 8, 1024, 0, 0), (0, 4, 16, 2, 0, 256, 0, 0), (0, 4, 16, 2, 0, 512, 0, 0), (0, 4, 16, 2, 1, 256, 0, 0),
    (0, 4, 16, 2, 1, 512, 0, 0), (0, 4, 16, 2, 3, 256, 0, 0), (0, 4, 16, 2, 7, 256, 0, 0), (0, 4, 16, 2, 8, 256, 0, 0),
    (0, 4, 16, 2, 8, 512, 0, 0), (0, 4, 16, 2, 8, 1024, 0, 0), (0, 4, 16, 2, 9, 1024, 0, 0), (0, 4, 16, 3, 0, 256, 0, 0),
    (0, 4, 16, 3, 0, 512, 0, 0), (0, 4, 16, 3, 0, 1024, 0, 0), (0, 4, 16, 3, 1, 256, 0, 0), (0, 4, 16, 3, 2, 256, 0, 0),
    (0, 4, 16, 3, 3, 256, 0, 0), (0, 4, 16, 3, 7, 256, 0, 0), (0, 4, 16, 3, 8, 256, 0, 0), (0, 4, 16, 3, 8, 512, 0, 0),
    (0, 4, 16, 3, 8, 1024, 0, 0), (0, 4, 16, 3, 9, 256, 0, 0), (0, 4, 16, 3, 9, 512, 0, 0), (0, 4, 16, 3, 9, 1024, 0, 0),
    (0, 4, 16, 4, 0, 256, 0, 0), (0, 4, 16, 4, 0, 512, 0, 0), (0, 4, 16, 4, 0, 1024, 0, 0), (0, 4, 16, 4, 7, 256, 0, 0),
    (0, 4, 16, 4, 8, 256, 0, 0), (0, 4, 16, 4, 8, 512, 0, 0), (0, 4, 16, 4, 8, 1024, 0, 0),
    # K2 norms / split: k_spmm_rm_g
    (1, 5, 8, 1, 0, 256, 1, 0), (1, 5, 8, 1, 0, 256, 2, 0), (1, 5, 8, 2, 0, 256, 1, 0), (1, 5, 8, 2, 64, 256, 1, 0),
    (1, 5, 8, 2, 64, 256, 2, 0), (1, 5, 8, 3, 0, 256, 1, 0), (1, 5, 8, 3, 0, 256, 2, 0), (1, 5, 8, 4, 0, 256, 1, 0),
    (1, 5, 8, 5, 64, 256, 1, 0), (1, 5, 8, 5, 64, 256, 2, 0), (1, 5, 16, 1, 0, 256, 1, 0), (1, 5, 16, 1, 0, 256, 2, 0),
    (1, 5, 16, 2, 0, 256, 1, 0), (1, 5, 16, 2, 0, 256, 2, 0), (1, 5, 16, 3, 0, 256, 1, 0), (1, 5, 16, 3, 0, 256, 2, 0),
    (1, 5, 16, 4, 0, 256, 1, 0), (1, 5, 16, 4, 0, 256, 2, 0), (1, 5, 16, 5, 0, 256, 1, 0), (1, 5, 16, 5, 0, 256, 2, 0),
    (1, 5, 16, 7, 64, 256, 1, 0), (1, 5, 16, 7, 64, 256, 2, 0), (1, 5, 16, 8, 0, 256, 1, 0), (1, 5, 16, 8, 0, 256, 2, 0),
    (1, 5, 16, 9, 0, 256, 1, 0), (1, 5, 16, 9, 0, 256, 2, 0), (1, 5, 16, 16, 0, 256, 1, 0), (1, 5, 16, 16, 0, 256, 2, 0),
    (1, 5, 16, 33, 0, 256, 1, 0), (1, 5, 16, 33, 0, 256, 2, 0), (1, 5, 16, 128, 0, 256, 1, 0),
    # K2 norms / split: k_spmm_rm
    (1, 6, 8, 2, 64, 256, 3, 0), (1, 6, 8, 3, 0, 256, 3, 0), (1, 6, 8, 3, 0, 256, 4, 0), (1, 6, 16, 1, 0, 256, 4, 0),
    (1, 6, 16, 2, 0, 256, 3, 0), (1, 6, 16, 2, 0, 256, 4, 0), (1, 6, 16, 3, 0, 256, 1, 0), (1, 6, 16, 3, 0, 256, 2, 0),
    (1, 6, 16, 3, 0, 256, 3, 0), (1, 6, 16, 3, 0, 256, 4, 0), (1, 6, 16, 16, 0, 256, 3, 0),
    # K2 norms / split: k_tile_resid
    (1, 7, 8, 1, 0, 256, 8, 0), (1, 7, 8, 1, 3, 256, 4, 0), (1, 7, 8, 1, 3, 256, 8, 0), (1, 7, 8, 2, 3, 256, 4, 0),
    (1, 7, 8, 2, 3, 256, 8, 0), (1, 7, 8, 3, 0, 256, 8, 0), (1, 7, 8, 3, 1, 256, 8, 0), (1, 7, 8, 3, 3, 256, 4, 0),
    (1, 7, 8, 4, 3, 256, 8, 0), (1, 7, 16, 1, 0, 256, 4, 0), (1, 7, 16, 1, 0, 256, 8, 0), (1, 7, 16, 1, 3, 256, 4, 0),
    (1, 7, 16, 1, 3, 256, 8, 0), (1, 7, 16, 2, 0, 256, 4, 0), (1, 7, 16, 2, 0, 256, 8, 0), (1, 7, 16, 2, 1, 256, 4, 0),
    (1, 7, 16, 2, 1, 256, 8, 0), (1, 7, 16, 2, 3, 256, 4, 0), (1, 7, 16, 2, 3, 256, 8, 0), (1, 7, 16, 3, 0, 256, 4, 0),
    (1, 7, 16, 3, 0, 256, 8, 0), (1, 7, 16, 3, 1, 256, 8, 0), (1, 7, 16, 3, 2, 256, 4, 0), (1, 7, 16, 3, 3, 256, 4, 0),
    (1, 7, 16, 3, 3, 256, 8, 0), (1, 7, 16, 4, 0, 256, 4, 0), (1, 7, 16, 4, 0, 256, 8, 0), (1, 7, 16, 4, 3, 256, 8, 0),
    # K2 norms / split: k_tile_resid_sp
    (1, 8, 8, 1, 0, 512, 4, 128), (1, 8, 8, 1, 1, 512, 4, 128), (1, 8, 8, 1, 1, 768, 4, 128), (1, 8, 8, 2, 1, 512, 4, 255),
    (1, 8, 8, 2, 1, 1024, 4, 255), (1, 8, 8, 3, 0, 512, 4, 208), (1, 8, 8, 3, 1, 512, 4, 208), (1, 8, 8, 3, 1, 768, 4, 208),
    (1, 8, 8, 3, 1, 1024, 4, 208), (1, 8, 8, 4, 1, 512, 4, 255), (1, 8, 8, 5, 1, 512, 4, 255), (1, 8, 16, 1, 0, 512, 4, 128),
    (1, 8, 16, 1, 1, 512, 4, 128), (1, 8, 16, 1, 1, 1024, 4, 128), (1, 8, 16, 2, 0, 512, 4, 255), (1, 8, 16, 2, 1, 512, 4, 255),
    (1, 8, 16, 2, 1, 768, 4, 255), (1, 8, 16, 3, 0, 512, 4, 208), (1, 8, 16, 3, 0, 512, 4, 255), (1, 8, 16, 3, 0, 768, 4, 208),
    (1, 8, 16, 3, 1, 512, 4, 208), (1, 8, 16, 3, 1, 512, 4, 255), (1, 8, 16, 3, 1, 768, 4, 208), (1, 8, 16, 3, 1, 1024, 4, 208),
    (1, 8, 16, 4, 0, 512, 4, 255), (1, 8, 16, 4, 1, 512, 4, 255), (1, 8, 16, 8, 0, 512, 4, 255),
    # K2 norms / split: k_tile_resid_spp
    (1, 9, 16, 3, 16, 512, 4, 208), (1, 9, 16, 3, 17, 768, 4, 208),
    # K2 block: k_spmm_rm_g
    (2, 5, 8, 1, 0, 256, 1, 0), (2, 5, 8, 1, 0, 256, 2, 0), (2, 5, 8, 2, 0, 256, 1, 0), (2, 5, 8, 2, 64, 256, 1, 0),
    (2, 5, 8, 2, 64, 256, 2, 0), (2, 5, 8, 3, 0, 256, 1, 0), (2, 5, 8, 3, 0, 256, 2, 0), (2, 5, 8, 4, 0, 256, 1, 0),
    (2, 5, 8, 5, 64, 256, 1, 0), (2, 5, 8, 5, 64, 256, 2, 0), (2, 5, 16, 1, 0, 256, 1, 0), (2, 5, 16, 1, 0, 256, 2, 0),
    (2, 5, 16, 2, 0, 256, 1, 0), (2, 5, 16, 2, 0, 256, 2, 0), (2, 5, 16, 3, 0, 256, 1, 0), (2, 5, 16, 3, 0, 256, 2, 0),
    (2, 5, 16, 4, 0, 256, 1, 0), (2, 5, 16, 4, 0, 256, 2, 0), (2, 5, 16, 5, 0, 256, 1, 0), (2, 5, 16, 5, 0, 256, 2, 0),
    (2, 5, 16, 7, 64, 256, 1, 0), (2, 5, 16, 7, 64, 256, 2, 0), (2, 5, 16, 8, 0, 256, 1, 0), (2, 5, 16, 8, 0, 256, 2, 0),
    (2, 5, 16, 9, 0, 256, 1, 0), (2, 5, 16, 9, 0, 256, 2, 0), (2, 5, 16, 16, 0, 256, 1, 0), (2, 5, 16, 16, 0, 256, 2, 0),
    (2, 5, 16, 33, 0, 256, 1, 0), (2, 5, 16, 33, 0, 256, 2, 0), (2, 5, 16, 128, 0, 256, 1, 0),
    # K2 block: k_spmm_rm
    (2, 6, 8, 2, 64, 256, 3, 0), (2, 6, 8, 3, 0, 256, 3, 0), (2, 6, 8, 3, 0, 256, 4, 0), (2, 6, 16, 2, 0, 256, 3, 0),
    (2, 6, 16, 2, 0, 256, 4, 0), (2, 6, 16, 3, 0, 256, 1, 0), (2, 6, 16, 3, 0, 256, 2, 0), (2, 6, 16, 3, 0, 256, 3, 0),
    (2, 6, 16, 3, 0, 256, 4, 0), (2, 6, 16, 16, 0, 256, 3, 0),
    # K2 block: k_tile_resid
    (2, 7, 8, 1, 0, 256, 8, 0), (2, 7, 8, 1, 3, 256, 4, 0), (2, 7, 8, 1, 3, 256, 8, 0), (2, 7, 8, 2, 3, 256, 4, 0),
    (2, 7, 8, 2, 3, 256, 8, 0), (2, 7, 8, 3, 0, 256, 8, 0), (2, 7, 8, 3, 1, 256, 8, 0), (2, 7, 8, 3, 3, 256, 4, 0),
    (2, 7, 8, 4, 3, 256, 8, 0), (2, 7, 16, 1, 0, 256, 4, 0), (2, 7, 16, 1, 0, 256, 8, 0), (2, 7, 16, 1, 3, 256, 4, 0),
    (2, 7, 16, 1, 3, 256, 8, 0), (2, 7, 16, 2, 0, 256, 8, 0), (2, 7, 16, 2, 1, 256, 8, 0), (2, 7, 16, 2, 3, 256, 4, 0),
    (2, 7, 16, 2, 3, 256, 8, 0), (2, 7, 16, 3, 0, 256, 4, 0), (2, 7, 16, 3, 0, 256, 8, 0), (2, 7, 16, 3, 1, 256, 8, 0),
    (2, 7, 16, 3, 2, 256, 4, 0), (2, 7, 16, 3, 3, 256, 4, 0), (2, 7, 16, 3, 3, 256, 8, 0), (2, 7, 16, 4, 0, 256, 4, 0),
    (2, 7, 16, 4, 0, 256, 8, 0), (2, 7, 16, 4, 3, 256, 8, 0),
    # K2 block: k_tile_resid_sp
    (2, 8, 8, 1, 0, 512, 4, 128), (2, 8, 8, 1, 1, 512, 4, 128), (2, 8, 8, 1, 1, 768, 4, 128), (2, 8, 8, 2, 1, 512, 4, 255),
    (2, 8, 8, 2, 1, 1024, 4, 255), (2, 8, 8, 3, 0, 512, 4, 208), (2, 8, 8, 3, 1, 512, 4, 208), (2, 8, 8, 3, 1, 768, 4, 208),
    (2, 8, 8, 3, 1, 1024, 4, 208), (2, 8, 8, 4, 1, 512, 4, 255), (2, 8, 8, 5, 1, 512, 4, 255), (2, 8, 16, 1, 0, 512, 4, 128),
    (2, 8, 16, 1, 1, 512, 4, 128), (2, 8, 16, 1, 1, 1024, 4, 128), (2, 8, 16, 2, 0, 512, 4, 255), (2, 8, 16, 2, 1, 512, 4, 255),
    (2, 8, 16, 2, 1, 768, 4, 255), (2, 8, 16, 3, 0, 512, 4, 208), (2, 8, 16, 3, 0, 512, 4, 255), (2, 8, 16, 3, 0, 768, 4, 208),
    (2, 8, 16, 3, 1, 512, 4, 208), (2, 8, 16, 3, 1, 512, 4, 255), (2, 8, 16, 3, 1, 768, 4, 208), (2, 8, 16, 3, 1, 1024, 4, 208),
    (2, 8, 16, 4, 0, 512, 4, 255), (2, 8, 16, 4, 1, 512, 4, 255), (2, 8, 16, 8, 0, 512, 4, 255),
    # K2 block: k_tile_resid_spp
    (2, 9, 16, 3, 16, 512, 4, 208), (2, 9, 16, 3, 17, 768, 4, 208),
    # K2 column-major: k_tile_resid_sp
    (3, 8, 8, 1, 0, 512, 4, 128), (3, 8, 8, 1, 1, 512, 4, 128), (3, 8, 8, 1, 1, 768, 4, 128), (3, 8, 8, 2, 1, 512, 4, 255),
    (3, 8, 8, 2, 1, 1024, 4, 255), (3, 8, 8, 3, 0, 512, 4, 208), (3, 8, 8, 3, 1, 512, 4, 208), (3, 8, 8, 3, 1, 768, 4, 208),
    (3, 8, 8, 3, 1, 1024, 4, 208), (3, 8, 8, 4, 1, 512, 4, 255), (3, 8, 16, 1, 0, 512, 4, 128), (3, 8, 16, 1, 1, 512, 4, 128),
    (3, 8, 16, 1, 1, 1024, 4, 128), (3, 8, 16, 2, 0, 512, 4, 255), (3, 8, 16, 2, 1, 512, 4, 255), (3, 8, 16, 2, 1, 768, 4, 255),
    (3, 8, 16, 3, 0, 512, 4, 208), (3, 8, 16, 3, 0, 512, 4, 255), (3, 8, 16, 3, 0, 768, 4, 208), (3, 8, 16, 3, 1, 512, 4, 208),
    (3, 8, 16, 3, 1, 512, 4, 255), (3, 8, 16, 3, 1, 768, 4, 208), (3, 8, 16, 3, 1, 1024, 4, 208), (3, 8, 16, 4, 0, 512, 4, 255),
    (3, 8, 16, 4, 1, 512, 4, 255),
    # K2 column-major: k_tile_resid_spp
    (3, 9, 16, 3, 16, 512, 4, 208), (3, 9, 16, 3, 17, 768, 4, 208),
    # K2 column-major: k_tile_resid_cm
    (3, 10, 8, 1, 0, 256, 2, 0), (3, 10, 8, 1, 3, 256, 2, 0), (3, 10, 8, 2, 3, 256, 2, 0), (3, 10, 8, 3, 0, 256, 2, 0),
    (3, 10, 8, 3, 1, 256, 2, 0), (3, 10, 8, 3, 3, 256, 2, 0), (3, 10, 8, 4, 3, 256, 2, 0), (3, 10, 16, 1, 0, 256, 2, 0),
    (3, 10, 16, 1, 3, 256, 2, 0), (3, 10, 16, 2, 0, 256, 2, 0), (3, 10, 16, 2, 1, 256, 2, 0), (3, 10, 16, 2, 3, 256, 2, 0),
    (3, 10, 16, 3, 0, 256, 2, 0), (3, 10, 16, 3, 0, 256, 4, 0), (3, 10, 16, 3, 0, 256, 8, 0), (3, 10, 16, 3, 1, 256, 2, 0),
    (3, 10, 16, 3, 2, 256, 2, 0), (3, 10, 16, 3, 3, 256, 2, 0), (3, 10, 16, 3, 3, 256, 4, 0), (3, 10, 16, 3, 3, 256, 8, 0),
    (3, 10, 16, 4, 0, 256, 2, 0), (3, 10, 16, 4, 3, 256, 2, 0),
    # K2 column-major: k_tile_resid_sp4
    (3, 11, 16, 3, 32, 512, 4, 208), (3, 11, 16, 3, 33, 768, 4, 208),
}


def test_zz_plan_coverage(na):
    """the set of (op, kernel, value bytes, terms unrolled, flags, threads, lanes | chunks | panel width, flush mask | k_vc rows)
    that nep_spmf_plan reported after the calls of this file equals the table PLANS: an instantiation that no case reaches any more
    fails here"""
    want = set(PLANS)
    dump = os.environ.get("NEP_SPMF_PLAN_DUMP")
    if dump:
        json.dump(sorted(SEEN), open(dump, "w"))
    missing, extra = sorted(want - SEEN), sorted(SEEN - want)
    assert not missing and not extra, "plans never reached: %s\nplans outside the table: %s" % (missing, extra)
    assert PANELS.get(OP_NORMS, 0) >= 2 and PANELS.get(OP_BLOCK, 0) >= 2, PANELS


def test_zz_report_counts_and_largest_ratios(na):
    for key in sorted(sc.COUNTS):
        print("calls %-44s exact %6d rounded %6d" % (key, sc.COUNTS[key][0], sc.COUNTS[key][1]))
    for name in sorted(pc.RATIOS):
        if "[" in name:
            print("ratio %-56s %.3g" % (name, pc.RATIOS[name]))
            assert pc.RATIOS[name] <= 1.0
    print("plans seen: %d" % len(SEEN))
