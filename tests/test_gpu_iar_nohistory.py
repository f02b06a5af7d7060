"""nep_iar_run without a history buffer (h_err = NULL).  With neigs = Inf the stop test cannot fire and everything the call returns
comes from the check of step m, so the run makes that one check only (include/nepmi355.h); with a finite neigs nothing changes.
Every case runs twice through the raw C ABI, once with a buffer and once without, on the problems of tests/iar_checkers.py (the
matrices and the LU handle of test_gpu_iar_checkers.py) as delay problems M(lam) = sum_t cf_t exp(-tau_t lam) A_t at sigma = 0:
what is under test is the plan and the loop of csrc/iar_run.hip, not a kernel, so n is a few hundred.

What must hold: res.k, res.nret, the eigenvalues, the eigenvector block and the WHOLE basis buffer are equal bit for bit between
the two runs, in a first call (refine_hint = -1, where the reviewed rows decide the sweeps of the later chunks) and in a settled
one; nep_iar_run_stats counts one decomposition and one check without a buffer and one per check step with it; all m rows of H are
reviewed either way; a miss injected at an early step is reported before the late steps are enqueued."""
import ctypes as ct

import numpy as np
import pytest
import torch

import iar_checkers as ic
import test_gpu_iar_checkers as tc
from primitive_checkers import C128, SENT

pytestmark = pytest.mark.gpu

# csrc/iar_run.hip with neigs = Inf: steps per chunk, distance of the row review.  A pin of the library's internals on purpose: the
# event count of a run without history and the first chunk that a reported miss keeps from being enqueued follow from them, so
# a change of either constant has to be made here too, regression or not.
CHUNK, LAG = 8, 24


@pytest.fixture(scope="module")
def na():
    import nep_amd
    if nep_amd.device_count() < 1:
        pytest.skip("no GPU")
    return nep_amd


def _tau(mt):
    return np.arange(mt) / max(mt - 1, 1)


def _check_steps(m, cee):
    return [k for k in range(1, m + 1) if k % cee == 0 or k == m]


def run(na, case, m, cee, neigs, history, hint=-1, tol=1e-10, env=None):
    """one nep_iar_run on problem `case` = (n, mt, values); returns a dict of everything the call gave back"""
    _lib, lib, _ = tc._L()
    n, mt, values = case
    p = ic.problem(n, mt, values)
    spmf, lu = tc._handles(na, n, mt, values)
    tau = _tau(mt)
    Ctab = np.asfortranarray(ic.natural_table(m, mt, p.cf, tau))
    cabs, cf = np.ascontiguousarray(p.cabs), np.ascontiguousarray(p.cf)
    calls = []

    def fv_eval(ctx, nlam, lam_p, F_p):
        la = np.frombuffer((ct.c_double * (2 * nlam)).from_address(lam_p), dtype=C128)
        F = np.frombuffer((ct.c_double * (2 * nlam * mt)).from_address(F_p), dtype=C128).reshape(nlam, mt)
        with np.errstate(all="ignore"):
            F[:] = cf[None, :] * np.exp(-tau[None, :] * la[:, None])
        calls.append(nlam)
        return 0
    cb = _lib.FV_EVAL(fv_eval)
    o = _lib.IarOpts(m, cee, 0, 10, 0, hint, tol, float(neigs), _lib.cdouble(0.0, 0.0), _lib.cdouble(1.0, 0.0))
    res = _lib.IarResult()
    lam = np.zeros(m, dtype=C128)
    Q = np.full((m, n), SENT, dtype=C128)
    err = np.full((m, m), np.nan, order="F") if history else None
    V = torch.from_numpy(np.full((m + 1, n * (m + 1)), SENT, dtype=C128)).to("cuda")
    v0 = np.ones(n, dtype=C128)
    tc._sync("upload")
    with tc._environment(env or {}):
        st = lib.nep_iar_run(spmf.h, lu.h, n, ct.addressof(o), _lib.hptr(v0), _lib.hptr(Ctab), mt, _lib.hptr(cabs), _lib.hptr(cf), None,
                             ct.cast(cb, ct.c_void_p), None, _lib.hptr(lam), None, _lib.hptr(Q), _lib.hptr(err) if history else None,
                             tc._p(V), ct.addressof(res), None)
    if st == _lib.NEP_ERR_HIP:
        tc._stop("nep_iar_run", lib.nep_last_error().decode(errors="replace"))
    tc._sync("nep_iar_run")
    stats = (ct.c_int32 * 4)()
    assert lib.nep_iar_run_stats(stats) == 0
    return dict(st=st, k=res.k, nret=res.nret, nconv=res.nconv, plan=res.refine_plan, off=res.refine_hint_off, reason=res.retry_reason,
                lam=lam, Q=Q, err=err, V=V.cpu().numpy(), stats=list(stats), calls=calls,
                msg=lib.nep_last_error().decode(errors="replace"))


def _same_results(a, b):
    assert (a["st"], a["k"], a["nret"], a["nconv"]) == (b["st"], b["k"], b["nret"], b["nconv"])
    assert (a["plan"], a["off"]) == (b["plan"], b["off"])
    for name in ("lam", "Q", "V"):
        assert ic._same(a[name], b[name]), "%s differs between the run with a history buffer and the run without" % name


@pytest.mark.parametrize("cee", [1, 3])
@pytest.mark.parametrize("m", [9, 20, 40])
def test_one_check_without_a_buffer_and_the_same_bits(na, m, cee):
    """neigs = Inf: the pair of runs in a first call and, with what that learnt as the hint, in a settled one"""
    case = (257, 4, "complex")
    steps = _check_steps(m, cee)
    hint = -1
    for state in ("first", "settled"):
        a = run(na, case, m, cee, np.inf, True, hint=hint)
        b = run(na, case, m, cee, np.inf, False, hint=hint)
        print(state, "hint", hint, "stats with a buffer", a["stats"], "without", b["stats"], "k", a["k"], "nret", a["nret"], "plan", a["plan"])
        assert a["st"] == 0 and b["st"] == 0, (a["msg"], b["msg"])
        assert a["k"] == m and a["reason"] == 0 and a["off"] == 0
        _same_results(a, b)
        assert a["stats"] == [len(steps), len(steps), m, m] and a["calls"] == steps
        assert b["stats"] == [1, 1, len([k for k in range(1, m + 1) if k % CHUNK == 0 or k == m]), m] and b["calls"] == [m]
        # the history itself: one sorted row per check step, nothing elsewhere
        for k in range(1, m + 1):
            row = a["err"][k - 1]
            if k in steps:
                assert np.all(np.isfinite(row[:k])) and np.all(np.diff(row[:k]) >= 0) and np.all(np.isnan(row[k:]))
            else:
                assert np.all(np.isnan(row))
        # A first call starts with 2 sweeps per step (Refine::plan without a hint); the omegas of these well-conditioned problems
        # satisfy UMFPACK's rule after one, so the review must have CHANGED the plan: at m = 40 that happens at the gate in front
        # of the chunk 33 .. 40, which both runs then enqueue with one sweep -- the case in which a review that came at another
        # time, or not at all, in one of the two runs would give another basis.
        assert a["plan"] == 1, "the review did not change the plan of %d sweeps a first call starts with" % 2
        hint = a["plan"]


def test_a_finite_neigs_is_checked_at_every_check_step(na):
    """the rule must not touch a run whose stop test can fire.  tol is loose on purpose (these random problems have no isolated
    eigenvalue: the first Ritz pair passes 0.5 around step 25 of 40 in the float64 model): what matters is that the test fires mid-run"""
    case, m = (65, 5, "real"), 40
    a = run(na, case, m, 1, 1, True, tol=0.5)
    b = run(na, case, m, 1, 1, False, tol=0.5)
    print("k", a["k"], b["k"], "stats", a["stats"], b["stats"], "callbacks", len(a["calls"]), len(b["calls"]))
    assert a["st"] == 0 and b["st"] == 0, (a["msg"], b["msg"])
    assert 10 <= a["k"] < m and a["nret"] == 1 and a["nconv"] >= 1
    assert (a["k"], a["nret"], a["nconv"]) == (b["k"], b["nret"], b["nconv"])
    assert ic._same(a["lam"], b["lam"]) and ic._same(a["Q"], b["Q"])
    k = a["k"]
    assert ic._same(a["V"][:k + 1, :65 * (k + 1)], b["V"][:k + 1, :65 * (k + 1)])       # (later columns: speculative steps)
    for r in (a, b):                                     # every step up to the converged one was decomposed and checked, in order
        assert r["stats"][0] >= k and r["stats"][1] >= k and r["calls"][:k] == list(range(1, k + 1))
        assert r["stats"][3] >= k


def test_misses_are_reported_without_a_buffer(na):
    """kind 3 (the decomposition of step m gives up) and kind 2 (a DGKS flag at an early step) with h_err = NULL.  The rows are
    reviewed from the loop, LAG steps behind the chunk being enqueued: the flag of step 5 is seen in front of the chunk 33 .. 40,
    which is therefore never enqueued -- block 0 of the basis columns 34 .. 40 still holds what the caller put there."""
    _lib = tc._L()[0]
    case, m = (257, 4, "complex"), 40
    n = case[0]
    r3 = run(na, case, m, 1, np.inf, False, env={"NEP_IAR_RUN_FAIL_AT": "3:%d" % m})
    assert r3["st"] == _lib.NEP_ERR_RETRY and r3["reason"] == 3, r3["msg"]
    assert r3["stats"][:2] == [1, 0] and r3["calls"] == []
    for history in (False, True):
        r2 = run(na, case, m, 1, np.inf, history, env={"NEP_IAR_RUN_FAIL_AT": "2:5"})
        print("history", history, "stats", r2["stats"], r2["msg"])
        assert r2["st"] == _lib.NEP_ERR_RETRY and r2["reason"] == 2, r2["msg"]
        assert r2["stats"][3] <= 4
        first_not_enqueued = (5 + LAG + CHUNK - 1) // CHUNK * CHUNK + 1
        assert first_not_enqueued == 33
        untouched = r2["V"][first_not_enqueued + 1:, :n]
        assert ic._same(untouched, np.full(untouched.shape, SENT, dtype=C128))
    # a middle step: its row is reviewed by the loop once every step is enqueued, block by block as the rows arrive -- long before
    # the decomposition behind step m is there, so no check is launched
    rm = run(na, case, m, 1, np.inf, False, env={"NEP_IAR_RUN_FAIL_AT": "2:20"})
    print("middle step: stats", rm["stats"], rm["msg"])
    assert rm["st"] == _lib.NEP_ERR_RETRY and rm["reason"] == 2, rm["msg"]
    assert rm["stats"][1] == 0 and rm["calls"] == [] and rm["stats"][3] == 16 < m
    r1 = run(na, case, m, 1, np.inf, False, env={"NEP_IAR_RUN_FAIL_AT": "1:5"})
    assert r1["st"] == _lib.NEP_ERR_RETRY and r1["reason"] == 1 and r1["stats"][3] == 4, r1["msg"]


def test_python_iar_with_and_without_errhist(na):
    """na.iar(neigs = Inf) passes no buffer when no errhist is asked for: same eigenvalues and vectors bit for bit, one check
    instead of one per check step; errhist keeps one row per check step"""
    from nep_amd.linsolvers import _DeviceRefactor
    _lib, lib, _ = tc._L()
    n, m, cee = 333, 20, 3
    nep = na.nep_gallery("gun_spmf_scaled", n)
    kw = dict(sigma=0.0, gamma=1.0, maxit=m, neigs=np.inf, v=np.ones(n), tol=1e-10, check_error_every=cee)
    na.iar(nep, **kw)
    _DeviceRefactor.wait()            # (both runs below must take the same factorisation route, and a settled refinement count)
    na.iar(nep, **kw)
    stats = (ct.c_int32 * 4)()
    r0 = na.iar.native_runs
    h = []
    lam1, Q1, V1 = na.iar(nep, errhist=h, **kw)
    assert lib.nep_iar_run_stats(stats) == 0
    s1 = list(stats)
    lam0, Q0, V0 = na.iar(nep, **kw)
    assert lib.nep_iar_run_stats(stats) == 0
    s0 = list(stats)
    assert na.iar.native_runs == r0 + 2
    steps = _check_steps(m, cee)
    print("stats with errhist", s1, "without", s0)
    assert len(h) == len(steps) and [len(x) for x in h] == steps
    assert s1[:2] == [len(steps)] * 2 and s0[:2] == [1, 1] and s1[3] == s0[3] == m
    assert ic._same(lam0, lam1) and ic._same(np.ascontiguousarray(Q0), np.ascontiguousarray(Q1))
    assert torch.equal(V0, V1)
    lam2, _, _ = na.iar(nep, logger=1, **kw)             # a logger reads the errors of every check step: the buffer stays
    assert lib.nep_iar_run_stats(stats) == 0 and list(stats)[:2] == [len(steps)] * 2 and ic._same(lam2, lam1)
