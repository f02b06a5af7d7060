"""Host side of iar without a GPU: the function that names the route of a call (`_route`), the record of the Ritz checks that
iar, tiar and iar_chebyshev share (`_ritzchecks.RitzChecks`) and the batch planner of the device eigen-decompositions."""
import itertools
import sys
from collections import deque

import numpy as np
import pytest
import torch

import nep_amd as na
from nep_amd._ritzchecks import RitzChecks

iar_mod = sys.modules["nep_amd.iar"]
SWITCHES = ("NEP_IAR_SYNC", "NEP_IAR_PYSTEP", "NEP_IAR_TRACE", "NEP_IAR_ONE_STREAM", "NEP_IAR_PASSES", "NEP_IAR_NATIVE_RUN",
            "NEP_IAR_EIG")
BOOLS = ("spmf_dev", "dev_lu", "native_err", "batch_async", "timed", "proj_solve", "native_run", "native_step", "force_sync")


def _facts(**kw):
    d = dict(m=20, orth=0, spmf_dev=True, dev_lu=True, native_err=True, batch_async=True)
    d.update(kw)
    return iar_mod._Facts(**d)


def _expected(f, env):
    """the conditions of the one-function driver, restated: the native-run test, use_async, cstep, check_thread, dev_eig"""
    flag = lambda name: bool(env.get(name))                       # noqa: E731
    if (f.native_run and f.native_step and not f.force_sync and not f.timed and not f.proj_solve and f.m <= 128
            and f.orth in (0, 1) and env.get("NEP_IAR_NATIVE_RUN", "1") != "0"
            and not any(flag(e) for e in ("NEP_IAR_SYNC", "NEP_IAR_PYSTEP", "NEP_IAR_TRACE", "NEP_IAR_ONE_STREAM", "NEP_IAR_PASSES"))
            and env.get("NEP_IAR_EIG", "dev") != "host" and f.native_err and f.spmf_dev and f.dev_lu):
        return "run"
    use_async = not f.timed and f.orth in (0, 1) and not flag("NEP_IAR_SYNC") and not f.proj_solve and not f.force_sync
    cstep = use_async and f.native_step and not flag("NEP_IAR_PYSTEP") and f.spmf_dev and f.dev_lu
    check_thread = cstep and not flag("NEP_IAR_ONE_STREAM") and f.batch_async
    dev_eig = check_thread and f.m <= 128 and env.get("NEP_IAR_EIG", "dev") != "host"
    if use_async and check_thread:
        return "step+deveig" if dev_eig else "step+hosteig"
    return "async" if use_async else "sync"


ENVS = [{}] + [{name: "1"} for name in SWITCHES[:5]] + [{"NEP_IAR_NATIVE_RUN": "0"}, {"NEP_IAR_EIG": "host"},
                                                         {"NEP_IAR_NATIVE_RUN": "0", "NEP_IAR_EIG": "host"},
                                                         {"NEP_IAR_NATIVE_RUN": "0", "NEP_IAR_ONE_STREAM": "1"}]


@pytest.mark.parametrize("env", ENVS, ids=lambda e: "+".join("%s=%s" % kv for kv in e.items()) or "default")
def test_route_equals_the_restated_conditions(monkeypatch, env):
    for name in SWITCHES:
        monkeypatch.delenv(name, raising=False)
    for name, val in env.items():
        monkeypatch.setenv(name, val)
    seen = set()
    for bits in itertools.product((False, True), repeat=len(BOOLS)):
        for m, orth in itertools.product((20, 128, 129), (0, 1, 2)):
            f = _facts(m=m, orth=orth, **dict(zip(BOOLS, bits)))
            r = iar_mod._route(f)
            assert r == _expected(f, env), (f, env)
            assert f.native() if r in ("run", "step+deveig", "step+hosteig") else (r == "async" or not f.native()), f
            seen.add(r)
    assert "sync" in seen and seen <= {"run", "step+deveig", "step+hosteig", "async", "sync"}
    assert ("run" in seen) == (env == {}) and ("async" in seen) == ("NEP_IAR_SYNC" not in env)


def test_route_table(monkeypatch):
    for name in SWITCHES:
        monkeypatch.delenv(name, raising=False)
    route = iar_mod._route
    assert route(_facts()) == "run"
    assert na.iar.last_route is None or isinstance(na.iar.last_route, str)
    # each of these keeps a call off `run`
    for name, val, to in (("NEP_IAR_SYNC", "1", "sync"), ("NEP_IAR_PYSTEP", "1", "async"), ("NEP_IAR_TRACE", "1", "step+deveig"),
                          ("NEP_IAR_ONE_STREAM", "1", "async"), ("NEP_IAR_PASSES", "1", "step+deveig"),
                          ("NEP_IAR_NATIVE_RUN", "0", "step+deveig"), ("NEP_IAR_EIG", "host", "step+hosteig")):
        monkeypatch.setenv(name, val)
        assert route(_facts()) == to, name
        monkeypatch.delenv(name)
    assert route(_facts(m=129)) == "step+hosteig"
    assert route(_facts(m=128)) == "run"
    assert route(_facts(orth=2)) == "sync"                                   # MGS
    assert route(_facts(orth=1)) == "run"                                    # CGS
    assert route(_facts(timed=True)) == route(_facts(proj_solve=True)) == route(_facts(force_sync=True)) == "sync"
    assert route(_facts(native_run=False)) == "step+deveig"                  # after a _NativeRunMiss
    assert route(_facts(native_step=False)) == "async"                       # after a _RefinementMiss: the Python step
    assert route(_facts(spmf_dev=False)) == route(_facts(dev_lu=False)) == "async"
    assert route(_facts(native_err=False)) == "step+deveig"                  # an error measure with batch_async the library does not know
    assert route(_facts(native_err=False, batch_async=False)) == "async"     # a callable error measure


# ---- the record of the Ritz checks

def _restated_record(err, errhist, m, tol, neigs, k, lam, e):
    """the bookkeeping of a check as the drivers spelled it out"""
    ne = min(len(e), err.shape[1])
    conv = int(np.sum(e < tol))
    idx = np.argsort(e, kind="stable")
    err[k - 1, :ne] = e[idx][:ne]
    errhist.append(err[k - 1, :ne].copy())
    if k == m or conv >= neigs:
        nrof = int(min(len(lam), neigs))
        lam = lam[idx[:nrof]]
        idx = idx[:nrof]
    return lam, idx, conv


@pytest.mark.parametrize("shape,fill", [((6, 6), np.nan), ((7, 7), np.nan), ((7, 10), np.nan), ((6, 6), 1.0)])
@pytest.mark.parametrize("neigs", [np.inf, 2, 30])
def test_record_equals_the_restatement(shape, fill, neigs):
    m, tol = 6, 1e-8
    rng = np.random.default_rng(3)
    err = np.full(shape, fill); err0 = err.copy()
    hist, hist0 = [], []
    rc = RitzChecks(m, tol, neigs, hist, err)
    assert rc.conv_eig == 0 and rc.k_checked == 0 and len(rc.lam) == 0 and rc.QT is None and len(rc.idx) == 0
    for k in range(1, m + 1):
        e = 10.0 ** rng.integers(-12, -4, size=k).astype(float)           # ties are frequent
        lam = rng.standard_normal(k) + 1j * rng.standard_normal(k)
        QT = object()
        rc.record(k, lam, QT, e)
        lam0, idx0, conv0 = _restated_record(err0, hist0, m, tol, neigs, k, lam, e)
        assert np.array_equal(rc.lam, lam0) and np.array_equal(rc.idx, idx0) and rc.conv_eig == conv0
        assert rc.QT is QT and rc.k_checked == k
        assert np.array_equal(err, err0, equal_nan=True)
    assert len(hist) == m and all(np.array_equal(a, b) for a, b in zip(hist, hist0))


def test_record_ties_width_empty_truncation_and_copies():
    m = 4
    err = np.full((m, m), np.nan)
    hist = []
    rc = RitzChecks(m, 1e-3, 2, hist, err)
    lam = np.array([10.0, 20.0, 30.0, 40.0, 50.0, 60.0], dtype=complex)
    # ties keep their order (stable sort); six errors into a row of four: the row write is capped, the order is of all six
    rc.record(1, lam, None, np.array([1.0, 0.5, 1.0, 0.5, 2.0, 1e-4]))
    assert list(rc.idx) == [5, 1, 3, 0, 2, 4] and list(err[0]) == [1e-4, 0.5, 0.5, 1.0] and len(hist[0]) == 4
    assert rc.conv_eig == 1 and len(rc.lam) == 6 and rc.lam is lam                    # conv < neigs, k < m: nothing truncated
    hist[0][:] = -1.0
    assert list(err[0]) == [1e-4, 0.5, 0.5, 1.0]                                      # errhist holds copies
    # empty check
    rc.record(2, lam[:0], None, np.zeros(0))
    assert rc.conv_eig == 0 and len(rc.lam) == 0 and len(hist[1]) == 0 and np.isnan(err[1]).all() and rc.k_checked == 2
    # truncation exactly at conv == neigs
    rc.record(3, lam[:3], None, np.array([1e-4, 1.0, 1e-5]))
    assert rc.conv_eig == 2 and list(rc.lam) == [30.0, 10.0] and list(rc.idx) == [2, 0]
    # ... and exactly at k == m, whatever converged
    rc = RitzChecks(m, 1e-3, 3, None, err)
    rc.record(3, lam[:3], None, np.array([3.0, 2.0, 1.0]))
    assert list(rc.lam) == [10.0, 20.0, 30.0] and list(rc.idx) == [2, 1, 0]          # k < m, conv < neigs: as they came
    rc.record(4, lam[:4], None, np.array([3.0, 2.0, 1.0, 4.0]))
    assert rc.conv_eig == 0 and list(rc.lam) == [30.0, 20.0, 10.0] and list(rc.idx) == [2, 1, 0]
    # neigs = inf never truncates before m, and keeps every pair at m
    rc = RitzChecks(m, 1e-3, np.inf, None, err)
    for k in (1, 2, 3):
        rc.record(k, lam[:k], None, np.full(k, 1e-9))
        assert rc.lam is not None and len(rc.lam) == k and rc.conv_eig == k and np.array_equal(rc.lam, lam[:k])
    rc.record(4, lam[:4], None, np.array([4.0, 3.0, 2.0, 1.0]))
    assert list(rc.lam) == [40.0, 30.0, 20.0, 10.0] and list(rc.idx) == [3, 2, 1, 0]


@pytest.fixture
def host_blocks(monkeypatch):
    """rowmajor_to_cols on host tensors: the finishing method's device call, restated"""
    import nep_amd._ritzchecks as mod
    monkeypatch.setattr(mod.dense, "rowmajor_to_cols", lambda QT, cols: torch.from_numpy(np.ascontiguousarray(QT[:, cols].T)))


HINTS = {"iar": ("Try to change the inner_solver_method for better performance.", "to_host_cm"),
         "tiar": (" Check that σ is not an eigenvalue.", "to_host_cm"),
         "iar_chebyshev": (" Check that σ is not an eigenvalue.", "to_host")}


@pytest.mark.parametrize("caller", list(HINTS))
def test_finish_raises_and_returns_as_each_caller_did(host_blocks, caller):
    from nep_amd import nep as nepmod
    hint, conv_name = HINTS[caller]
    host = getattr(nepmod, conv_name)
    n, m = 5, 4
    rng = np.random.default_rng(1)
    QT = rng.standard_normal((n, m)) + 1j * rng.standard_normal((n, m))
    lam = np.arange(1.0, m + 1).astype(complex)
    e = np.array([1e-2, 1e-9, 1e-1, 1e-10])
    # not enough pairs at k == m: lam (4), v n x 4 in the order of the errors, the error row (4)
    err = np.full((m, m), np.nan)
    rc = RitzChecks(m, 1e-8, 3, None, err)
    rc.record(m, lam, QT, e)
    with pytest.raises(na.NoConvergenceException) as ei:
        rc.finish(m, 17, hint, host)
    x = ei.value
    assert list(x.lam) == [4.0, 2.0, 1.0] and x.v.shape == (n, 3) and np.array_equal(x.v, QT[:, [3, 1, 0]])
    assert np.array_equal(x.errmeasure, [1e-10, 1e-9, 1e-2])
    assert x.msg == str(x) == "Number of iterations exceeded. maxit=17." + hint
    assert x.msg in ("Number of iterations exceeded. maxit=17.Try to change the inner_solver_method for better performance.",
                     "Number of iterations exceeded. maxit=17. Check that σ is not an eigenvalue.")
    # three converged but more wanted: no hint; all m pairs travel
    rc = RitzChecks(m, 1e-1, 30, None, err)
    rc.record(m, lam, QT, e)
    with pytest.raises(na.NoConvergenceException) as ei:
        rc.finish(m, 17, hint, host)
    assert ei.value.msg == "Number of iterations exceeded. maxit=17." and len(ei.value.lam) == m and ei.value.v.shape == (n, m)
    assert ei.value.errmeasure.shape == (m,)
    # no check was ever made: lam empty, v None, an empty error row
    rc = RitzChecks(m, 1e-8, 3, None, err)
    with pytest.raises(na.NoConvergenceException) as ei:
        rc.finish(m, 17, hint, host)
    assert len(ei.value.lam) == 0 and ei.value.v is None and ei.value.errmeasure.shape == (0,)
    # converged: the pairs below tol, on the host through the caller's conversion or as the device block
    rc = RitzChecks(m, 1e-8, 2, None, err)
    rc.record(3, lam[:3], QT[:, :3], np.array([1e-2, 1e-9, 1e-12]))
    l1, Q1 = rc.finish(3, 17, hint, host)
    assert list(l1) == [3.0, 2.0] and isinstance(Q1, np.ndarray) and np.array_equal(Q1, QT[:, [2, 1]])
    assert Q1.flags.f_contiguous == (conv_name == "to_host_cm")
    l2, Q2 = rc.finish(3, 17, hint, None)
    assert list(l2) == [3.0, 2.0] and isinstance(Q2, torch.Tensor) and Q2.shape == (2, n)
    # neigs = inf: returns the converged ones of the last check, never raises
    rc = RitzChecks(m, 1e-8, np.inf, None, err)
    rc.record(m, lam, QT, e)
    l3, Q3 = rc.finish(m, 17, hint, host)
    assert list(l3) == [4.0, 2.0] and np.array_equal(Q3, QT[:, [3, 1]])


# ---- the batch planner of the device eigen-decompositions

def _restated_plan(m, check_error_every, BMAX, LASTB, T100, TSTEP=0.35):
    allk = [kk for kk in range(1, m + 1) if kk % check_error_every == 0 or kk == m]
    ends = []; e_ = len(allk)
    size = min(LASTB, e_)
    while e_ > 0:
        ends.append(allk[e_ - 1]); e_ -= size
        if e_ > 0:
            size = int(min(BMAX, e_, max(1, np.ceil(2.0 * T100 * (allk[e_ - 1] / 100.0) ** 2 / (TSTEP * check_error_every)))))
    return allk, set(ends)


@pytest.mark.parametrize("bmax,lastb", [(16, 8), (4, 2), (16, 1)])
@pytest.mark.parametrize("every", [1, 3])
@pytest.mark.parametrize("m", [20, 100])
def test_eig_batch_plan(m, every, bmax, lastb):
    allk, ends = _restated_plan(m, every, bmax, lastb, 3.3)
    plan_end = iar_mod._eig_batch_plan(m, every, bmax, lastb, 3.3)
    assert plan_end == ends and m in plan_end
    # the checker's use of it: steps arrive one by one, a batch goes out as soon as _eig_batch_ready says so
    pend = deque(); batches = []
    for kk in allk + [None]:
        if kk is not None:
            pend.append(kk)
        while True:
            cnt = iar_mod._eig_batch_ready(pend, bmax, plan_end, kk is None)
            if not cnt:
                break
            batches.append([pend.popleft() for _ in range(cnt)])
    assert not pend
    assert [kk for b in batches for kk in b] == allk                         # every check step once, batches contiguous and in order
    assert max(len(b) for b in batches) <= bmax
    assert len(batches[-1]) <= lastb
    got = {b[-1] for b in batches}
    assert ends <= got
    stride = {allk[i] for i in range(1, len(allk) - 1) if allk[i + 1] - allk[i] != allk[i] - allk[i - 1]}
    assert got - ends <= stride | {b[-1] for b in batches if len(b) == bmax}  # further cuts: a change of stride (the last step), a full batch
    for b in batches:
        assert len(set(np.diff(b))) <= 1                                     # one stride per batch: the kernel's addressing
    # throttled runs have no plan: a batch is whatever is pending, up to bmax
    assert iar_mod._eig_batch_ready(deque(), bmax, None, False) == 0
    assert iar_mod._eig_batch_ready(deque(allk[:3]), bmax, None, False) == min(3, bmax)
