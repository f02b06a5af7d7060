"""Every host route of iar (`iar.last_route`: run, step+deveig, step+hosteig, async, sync) on one small problem, four settings each:
the route taken, the checks made, the step at which the run stops and the pairs it returns are those of the CPU oracle
(`oracle.solvers.iar` on `DerSPMF(gun_spmf_scaled(1310), 0, 20)`), and eigenvalues and error histories equal the default route's.

Oracle outcomes (every decision has at least a factor 3 of margin to tol):
  inf      neigs=inf tol=1e-10 every 1   20 checks, 7 pairs (step 20: 7th-best error 1.0e-12, 8th 5.0e-8)
  four     neigs=4   tol=1e-8  every 1   stops at step 12 with 4 pairs (4th-best error 3.1e-8 at step 11, 1.3e-9 at step 12)
  every5   neigs=4   tol=1e-10 every 5   checks at 5, 10, 15, stops at 15 with 4 pairs (4th-best 2.4e-7 at 10, 6.1e-13 at 15)
  noconv   neigs=30  tol=1e-10 every 3   NoConvergenceException after checks at 3, 6, ..., 18, 20; lam 20, v n x 20, errors 20
An exception carries all 20 Ritz values of the last step; the eigenvalue comparison takes those whose carried error is below
tol (the unconverged ones approximate nothing, and their sensitivity to the rounding of H is not bounded by any tolerance)."""
import contextlib
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N, M = 1310, 20
SETTINGS = {
    "inf": (dict(neigs=np.inf, tol=1e-10, check_error_every=1), list(range(1, 21)), 7),
    "four": (dict(neigs=4, tol=1e-8, check_error_every=1), list(range(1, 13)), 4),
    "every5": (dict(neigs=4, tol=1e-10, check_error_every=5), [5, 10, 15], 4),
    "noconv": (dict(neigs=30, tol=1e-10, check_error_every=3), [3, 6, 9, 12, 15, 18, 20], None),
}
# name: (environment, extra keywords, route, eigenvalue tolerance against the default route)
ROUTES = {
    "default": ({}, {}, "run", 1e-10),
    "native_run_off": ({"NEP_IAR_NATIVE_RUN": "0"}, {}, "step+deveig", 1e-10),
    "eig_host": ({"NEP_IAR_EIG": "host"}, {}, "step+hosteig", 1e-10),
    "one_stream": ({"NEP_IAR_ONE_STREAM": "1"}, {}, "async", 1e-10),
    "pystep": ({"NEP_IAR_PYSTEP": "1"}, {}, "async", 1e-10),
    "callable": ({}, {"errmeasure": "callable"}, "async", 1e-10),
    "sync_env": ({"NEP_IAR_SYNC": "1"}, {}, "sync", 1e-10),
    "timers": ({}, {"timers": "dict"}, "sync", 1e-10),
    "mgs": ({}, {"orthmethod": 2}, "sync", 1e-8),             # the tolerance of test_gpu_solvers.py against the oracle
    "run_device": ({}, {"return_device": True}, "run", 1e-10),
    "sync_device": ({"NEP_IAR_SYNC": "1"}, {"return_device": True}, "sync", 1e-10),
}


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


def run_route(na, nep, setting, route):
    """one iar call; (lam, Q on the host, basis rows, errhist, error row or None, raised)"""
    env, extra, _, _ = ROUTES[route]
    kw = dict(sigma=0, gamma=1, maxit=M, v=np.ones(N), **SETTINGS[setting][0])
    for key, val in extra.items():
        if val == "callable":
            E = na.StandardSPMFErrmeasure(nep)
            val = lambda lam, v: na.estimate_error(E, lam, v)        # noqa: E731
        elif val == "dict":
            val = {}
        kw[key] = val
    hist = []
    with _environment(env):
        try:
            lam, Q, V = na.iar(nep, errhist=hist, **kw)
        except na.NoConvergenceException as e:
            return np.asarray(e.lam), np.asarray(e.v), None, hist, np.asarray(e.errmeasure), True
    if extra.get("return_device"):
        assert Q.is_cuda and Q.shape == (len(lam), N)
        Q = na.to_host(Q)
    return np.asarray(lam), np.asarray(Q), V, hist, None, False


@pytest.fixture(scope="module")
def na():
    import nep_amd
    assert nep_amd.device_count() >= 1, "no GPU visible"
    return nep_amd


@pytest.fixture(scope="module")
def nep(na):
    from nep_amd.linsolvers import _DeviceRefactor
    nep = na.nep_gallery("gun_spmf_scaled", N)
    na.iar(nep, sigma=0, gamma=1, maxit=M, v=np.ones(N), neigs=np.inf, tol=1e-10)
    _DeviceRefactor.wait()
    return nep


@pytest.fixture(scope="module")
def default(na, nep):
    """the default route's result per setting: computed once, compared against by every other route"""
    return {s: run_route(na, nep, s, "default") for s in SETTINGS}


@pytest.mark.parametrize("setting", list(SETTINGS))
@pytest.mark.parametrize("route", list(ROUTES))
def test_route(na, nep, default, route, setting):
    kw, checks, pairs = SETTINGS[setting]
    lam, Q, V, hist, errrow, raised = run_route(na, nep, setting, route)
    assert na.iar.last_route == ROUTES[route][2]
    assert [len(h) for h in hist] == checks
    assert raised == (pairs is None)
    if raised:
        assert lam.shape == (M,) and Q.shape == (N, M) and errrow.shape == (M,)
        conv = errrow < kw["tol"]
    else:
        assert V.shape[0] == checks[-1] and lam.shape == (pairs,) and Q.shape == (N, pairs)
        conv = np.ones(pairs, dtype=bool)
    lam0, _, _, hist0, errrow0, _ = default[setting]
    conv0 = (errrow0 < kw["tol"]) if raised else np.ones(len(lam0), dtype=bool)
    assert conv.sum() == conv0.sum()
    left = list(lam0[conv0])
    for x in lam[conv]:
        j = int(np.argmin([abs(x - y) for y in left]))
        print(route, setting, "eigenvalue", x, "differs by", abs(x - left[j]))
        assert abs(x - left[j]) <= ROUTES[route][3] * max(1.0, abs(x))
        left.pop(j)
    # error histories within a factor 10 wherever both are above 1e-12 (SURVEY.md section 8d parity rule iv)
    for h, h0 in zip(hist, hist0):
        both = (h > 1e-12) & (h0 > 1e-12)
        if both.any():
            print(route, setting, "step", len(h), "error ratio", (h[both] / h0[both]).min(), (h[both] / h0[both]).max())
        assert np.all((h[both] > 0.1 * h0[both]) & (h[both] < 10 * h0[both]))
