"""Exact and bounded parity tests of K6 (csrc/orth.hip: nep_orth, nep_orth_dev, nep_orth_dev_mirror, nep_orth_dev_iar_next) and K9
(nep_gemm_h_rm of csrc/gemm.hip) through the raw C ABI (`nep_amd._lib.lib`), on the case lists of tests/orth_checkers.py.

The exact tier (dyadic bases with disjoint supports, Gaussian-integer vectors) carries the shape sweep: every row count next to a
tile edge, the switch to the DPP reduction, the tile loops of both update kernels behind the ORTH_NPART cap, the column-group walk
and the non-temporal loads of the 0.8 GB case, all eight instantiations of k_orth_finish_vc (ROWS 32 / 64 x MT 1..4), six forms of
`active`.  The rounded tier
holds a few shapes to the bounds derived in the docstring of orth_checkers.  The switches that are cached in a static
(NEP_ORTH_ROWS_K, NEP_ORTH_DEV_PASSES) run in a child process each.  test_host_orth_checkers.py shows that the checkers reject
mutants."""
import ctypes as ct
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import orth_checkers as oc
import primitive_checkers as pc
from orth_checkers import ORTH, DEV, MIRROR, NEXT
from primitive_checkers import C128, SENT

pytestmark = pytest.mark.gpu


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
    if not _DECLARED:                       # exported, but internal (csrc/common.h): not in _lib.SIGNATURES
        vp, i32, i64 = ct.c_void_p, ct.c_int32, ct.c_int64
        lib.nep_orth_dev_mirror.argtypes = [vp, i64, i64, i32, vp, vp, vp, i32, vp, i32, vp]
        lib.nep_orth_dev_iar_next.argtypes = [vp, i64, i64, i32, vp, vp, vp, i32, vp, i32, vp, i64, i32, vp, vp, vp]
        lib.nep_orth_dev_mirror.restype = lib.nep_orth_dev_iar_next.restype = i32
        _DECLARED.append(True)
    return _lib, lib, stream_ptr


def _stop(what, e):
    pytest.exit("HIP error in %s: %s -- nothing more is started on this device" % (what, e), returncode=3)


def _up(buf):
    try:
        return None if buf is None else torch.from_numpy(np.ascontiguousarray(buf)).to("cuda")
    except RuntimeError as e:
        _stop("upload", e)


def _sync(what):
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:
        _stop(what, e)


def _p(t):
    return None if t is None else ct.c_void_p(t.data_ptr())


def _down(t, what="download"):
    try:
        return None if t is None else t.cpu().numpy()
    except RuntimeError as e:
        _stop(what, e)


_VDEV = []                                  # [the host buffer, its device copy]: the entries of a case share one upload of V


def _dev_V(V):
    if V is None:
        return None
    if not _VDEV or _VDEV[0] is not V:
        _VDEV.clear()
        _VDEV.extend([V, _up(V)])
    return _VDEV[1]


def k6_impl(entry, V, ldv, rows, k, active, w, out, method, mirror=None, nmirror=0, C=None, ldc=0, mt=0, WT=None, shift=None, n=0):
    _lib, lib, st = _L()
    Vd, wd = _dev_V(V), _up(w)
    res = dict(mirror=None, WT=None, shift=None)
    if entry == ORTH:
        act = None if active is None else np.ascontiguousarray(active, dtype=np.int64)
        h = None if out is None else np.full(max(k, 1), SENT, dtype=C128)
        beta, npass = ct.c_double(-1.0), ct.c_int32(-1)
        rc = lib.nep_orth(_p(Vd), ldv, rows, k, None if act is None else _lib.hptr(act), _p(wd), None if h is None else _lib.hptr(h),
                          ct.byref(beta), method, ct.byref(npass), st())
        o = None if out is None else out.copy()
        if rc in (oc.NEP_OK, oc.NEP_ERR_BREAKDOWN):
            o[:k] = h[:k]; o[k] = beta.value; o[k + 1] = complex(npass.value, 2 * int(rc == oc.NEP_ERR_BREAKDOWN))
        else:
            assert (out is None or np.array_equal(h, np.full(max(k, 1), SENT, dtype=C128))) and beta.value == -1.0 and npass.value == -1
        _sync(entry)
        res.update(status=rc, w=_down(wd, entry), out=o)
        return res
    ad = None if active is None else _up(np.ascontiguousarray(active, dtype=np.int64))
    od = _up(out)
    if entry == DEV:
        rc = lib.nep_orth_dev(_p(Vd), ldv, rows, k, _p(ad), _p(wd), _p(od), method, st())
    else:
        md = _up(mirror)
        if entry == MIRROR:
            rc = lib.nep_orth_dev_mirror(_p(Vd), ldv, rows, k, _p(ad), _p(wd), _p(od), method, _p(md), nmirror, st())
        else:
            Cd, Wd, sd = _up(C), _up(WT), _up(shift)
            rc = lib.nep_orth_dev_iar_next(_p(Vd), ldv, n, k, _p(ad), _p(wd), _p(od), method, _p(md), nmirror, _p(Cd), ldc, mt, _p(Wd), _p(sd), st())
            _sync(entry)
            res.update(WT=_down(Wd, entry), shift=_down(sd, entry))
        _sync(entry)
        res.update(mirror=_down(md, entry))
    _sync(entry)
    res.update(status=rc, w=_down(wd, entry), out=_down(od, entry))
    return res


def _same_bits(x, y):
    return (x is None and y is None) or np.array_equal(np.asarray(x).view(np.float64), np.asarray(y).view(np.float64), equal_nan=True)


def k6_twice(**kw):
    """two calls on the same operands give the same bits"""
    r1, r2 = k6_impl(**kw), k6_impl(**kw)
    assert r1["status"] == r2["status"]
    for key in ("w", "out", "mirror", "WT", "shift"):
        assert _same_bits(r1[key], r2[key]), "%s(method %d): %s differs between two calls" % (kw["entry"], kw["method"], key)
    return r1


def run_k6(group=None, only=None, max_passes=2, select=None, impl=k6_twice):
    n = calls = 0
    for c in oc.K6.cases():
        if (group is not None and c.group != group) or (select is not None and not select(c)):
            continue
        calls += oc.K6.check(impl, c, only=only, max_passes=max_passes)
        n += 1
    _VDEV.clear()
    return n, calls


def gemm_h_rm(WT, ldw, YT, ldy, rows, k, p):
    _lib, lib, st = _L()
    Wd = _up(WT); Yd = Wd if YT is WT else _up(YT)
    out = np.full(k * p, SENT, dtype=C128)
    rc = lib.nep_gemm_h_rm(_p(Wd), ldw, _p(Yd), ldy, rows, k, p, _lib.hptr(out), st())
    if rc == _lib.NEP_ERR_HIP:
        _stop("nep_gemm_h_rm", lib.nep_last_error())
    _lib.check(rc)
    return out


# ---- K6 ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("group", [g for g in oc.groups(oc.K6) if g != "big"])
def test_k6_against_reference(na, group):
    """every case of the group through every entry point it names, each call twice (same bits): exact cases bit for bit (beta and w of
    family G within 2u / 8u of the integer reference), rounded cases inside the bounds of orth_checkers; padding of w, d_out, the
    mirror row, WT and the shifted block survives; the mirror row equals the device row; the fused nep_orth_dev_iar_next returns
    the bits of nep_orth_dev"""
    n, calls = run_k6(group)
    assert n >= 1 and calls >= 2 * n
    print("K6 %s: %d cases, %d calls checked" % (group, n, calls))


def test_k6_big_case_column_group_walk_and_non_temporal_loads(na):
    """392 193 x 130 (0.8 GB), the one shape the host model does not run: gridDim.y = 16 < 17 column groups, both tile loops, and the
    non-temporal loads -- which have a threshold for full columns and one for the staircase, hence two operand sets at this shape
    (full columns with family G, staircase with family P); nep_orth_dev and nep_orth, each call twice with the same bits"""
    n, calls = run_k6("big")
    torch.cuda.empty_cache()
    assert n == 2 and calls == 4


def test_k6_argument_contract(na):
    """rows < 1, k < 1, ldv < rows, NULL buffers, method out of range (2 is refused by the device forms), mt outside 1..4, ldc < k + 1:
    NEP_ERR_ARG, nothing written"""
    c = next(c for c in oc.K6.cases() if c.group == "iar_next")
    a = c.args
    n_bad = 0
    for entry, method, mt in ((ORTH, 0, 0), (DEV, 0, 0), (MIRROR, 0, 0), (NEXT, 0, 3)):
        kw = oc.K6.buffers(a, entry, method, mt)
        bads = [dict(rows=0), dict(rows=-1), dict(k=0), dict(ldv=a["rows"] - 1), dict(V=None), dict(w=None), dict(out=None), dict(method=-1),
                dict(method=3)]
        bads += [dict(method=2)] if entry != ORTH else []
        bads += [dict(mt=0), dict(mt=5), dict(ldc=a["k"]), dict(C=None), dict(WT=None), dict(shift=None), dict(n=0)] if entry == NEXT else []
        for bad in bads:
            kw2 = dict(kw, **bad)
            if entry == NEXT and "rows" in bad:              # (the entry point takes n: rows = n (k + 1))
                kw2["n"] = bad["rows"]
            res = k6_impl(**kw2)
            assert res["status"] == oc.NEP_ERR_ARG, (entry, bad, res["status"])
            for key in ("w", "out", "mirror", "WT", "shift"):
                assert kw2.get(key) is None or _same_bits(res[key], kw2[key]), (entry, bad, key)
            n_bad += 1
    _lib, lib, st = _L()
    assert b"invalid argument" in lib.nep_last_error()
    assert n_bad >= 45


# ---- switches cached in a static on first use: a fresh child process per setting ------------------------------------------------
def child_main(mode):
    """entry of a child process: exit 0 with the number of calls checked, 3 after a HIP error (_stop has no pytest session to end
    here), 1 after a failed assertion"""
    try:
        n = run_child(mode)
    except pytest.exit.Exception as e:
        print(e.msg, file=sys.stderr)
        sys.exit(3)
    print("k6 calls checked:", n)


def run_child(mode):
    if mode == "rows_k0":                 # the wave-per-column-slice update on the asynchronous path, its tile loop at 70001 x 64
        n, calls = run_k6(only=(DEV, MIRROR, NEXT), select=lambda c: not c.extra.get("big"))
    else:                                 # one enqueued pass: passes == 1, another_pass_wanted == 1, h of the first pass
        two = lambda c: not c.extra.get("big") and (c.extra.get("nearspan") or c.cid.endswith(("P2", "G2", "BRK")))
        n, calls = run_k6(only=(DEV, MIRROR, NEXT), max_passes=1, select=two)
    for name in sorted(pc.RATIOS):
        print("ratio %-44s %.3g" % (name, pc.RATIOS[name]))
    return calls


@pytest.mark.parametrize("mode,env,least", [("rows_k0", dict(NEP_ORTH_ROWS_K="0"), 400), ("passes1", dict(NEP_ORTH_DEV_PASSES="1"), 100)])
def test_k6_static_switches_in_a_child_process(na, mode, env, least):
    here = os.path.dirname(os.path.abspath(__file__))
    code = ("import sys; sys.path[:0] = [%r, %r]; import test_gpu_orth_checkers as t; t.child_main(%r)"
            % (here, os.path.dirname(here), mode))
    try:
        out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=600, env=dict(os.environ, **env))
    except subprocess.TimeoutExpired as e:
        pytest.exit("the child process with %r hung (%s): nothing more is started on this device" % (env, e), returncode=3)
    if out.returncode < 0 or out.returncode in (3, 124, 134, 137, 139):
        pytest.exit("the child process died (%d): nothing more is started on this device\n%s" % (out.returncode, out.stderr[-4000:]), returncode=3)
    assert out.returncode == 0, (out.stdout[-2000:], out.stderr[-4000:])
    print(out.stdout[-3000:])
    assert "k6 calls checked:" in out.stdout and int(out.stdout.split("k6 calls checked:")[1].split()[0]) >= least, out.stdout[-2000:]


# ---- K9 ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("group", oc.groups(oc.K9))
def test_k9_against_reference(na, group):
    """C = W^H Y at the rows around every switch of rows_per_wg and of the two-stage reduce, ldw > k and ldy > p with NaN padding, W and
    Y in one buffer; every call twice: the same bits"""
    n = 0
    for c in oc.K9.cases():
        if c.group == group:
            oc.K9.check(gemm_h_rm, c)
            a = c.args
            assert _same_bits(gemm_h_rm(**a), gemm_h_rm(**a)), c
            n += 1
    assert n >= 2


def test_k9_argument_contract(na):
    _lib, lib, st = _L()
    rows, k, p = 40, 5, 7
    Wd = _up(np.ones(rows * 300, dtype=C128)); Yd = _up(np.ones(rows * 300, dtype=C128))
    out = np.full(300 * 300, SENT, dtype=C128)

    def call(rows=rows, k=k, p=p, ldw=k, ldy=p, W=Wd, Y=Yd, o=out):
        return lib.nep_gemm_h_rm(_p(W), ldw, _p(Y), ldy, rows, k, p, None if o is None else _lib.hptr(o), st())

    assert call() == 0
    out[:] = SENT
    for bad in (dict(k=0, ldw=1), dict(p=0, ldy=1), dict(k=257, ldw=257), dict(p=257, ldy=257), dict(ldw=k - 1), dict(ldy=p - 1), dict(rows=0),
                dict(rows=-3), dict(W=None), dict(Y=None), dict(o=None)):
        assert call(**bad) == oc.NEP_ERR_ARG, bad
    assert np.array_equal(out, np.full(300 * 300, SENT, dtype=C128))
    assert call(k=256, p=256, ldw=256, ldy=256, rows=40) == 0


def test_zz_report_counts_and_largest_ratios(na):
    """calls checked per entry point and tier in this process, and the largest error / bound of every rounded family (each was
    asserted <= 1 where it arose; the children print theirs)"""
    for key in sorted(oc.COUNTS):
        print("calls %-28s %-8s %6d" % (key[0], key[1], oc.COUNTS[key]))
    seen = 0
    for name in sorted(pc.RATIOS):
        if name.startswith(("nep_orth", "nep_gemm_h_rm")):
            print("ratio %-44s %.3g" % (name, pc.RATIOS[name]))
            assert pc.RATIOS[name] <= 1.0
            seen += 1
    assert not oc.COUNTS or seen >= 8 and all((e, "exact") in oc.COUNTS for e in (ORTH, DEV, MIRROR, NEXT, "nep_gemm_h_rm"))
