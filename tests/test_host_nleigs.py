"""CPU tests of the stages of nep_amd.nleigs that need no device: the host set-up and the freeze of the linearisation against
the oracle, the step coefficients, the pencil record, the check schedule and the re-run wrapper."""
import importlib
import itertools
import types
import warnings

import numpy as np
import pytest
import torch

import nep_amd as na
from oracle import neps as oneps, nleigs as onl

nl = importlib.import_module("nep_amd.nleigs")

B = [np.array([[1., 3], [5, 6]]), np.array([[3., 4], [6, 6]]), np.eye(2)]
SIGMA = np.array([-10 - 2j, 10 - 2j, 10 + 2j, -10 + 2j])
NODES0 = np.array([0, 3 + 1j, -3 - 1j, 6, -6], dtype=complex)


@pytest.mark.parametrize("leja,static,maxdgr", list(itertools.product([0, 1, 2], [False, True], [100, 5])))
def test_setup_and_freeze_match_the_oracle(leja, static, maxdgr):
    """2 x 2 PEP of test_nleigs_basic_kat, maxit = 10: nodes, poles and scaling of the host set-up, then the expansion steps up to
    the freeze (fed with the package's own divided-difference norms), against the details of an oracle run: sigma, xi, beta
    element for element, kconv exactly, nrmD to the tolerance of test_rk_helper_matches_oracle"""
    maxit = 10
    nodes = NODES0 if leja == 0 else np.zeros(0, dtype=complex)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        lo, _, _, do = onl.nleigs(oneps.PEP(B), SIGMA, maxit=maxit, v=np.ones(2) + 0j, leja=leja, nodes=nodes, static=static,
                                  maxdgr=maxdgr, return_details=True)
        assert len(lo) == 4 and do.kconv == 6
        pep = na.PEP(B)
        p = na.rk_helper.rk_structure(pep)[0]
        gamma, nodes_, sigma, xi, beta = nl._interpolation(SIGMA, np.array([np.inf]), nodes, leja, static, maxit, maxdgr, p, True)
        sgdd, Dall, nrmD_all, nrmD = nl._divided_differences(pep, False, sigma, xi, beta, maxdgr, 3, True)
        assert Dall is None and nrmD_all is None
        s = nl._State(2, p, None, 3, static, leja, 1, maxit, maxdgr, max(1e-10 / 10, 100 * nl.EPS), nodes_, sigma, xi, beta, sgdd,
                      None, nrmD)
        k = 1
        while s.expand and k <= s.kmax:
            s.grow(k)
            k += 1
    assert not s.expand and s.kconv == do.kconv
    kk = len(do.sigma)
    assert s.sigma[:kk].shape == do.sigma.shape and np.array_equal(s.sigma[:kk], do.sigma)
    assert s.xi.shape == do.xi.shape and np.array_equal(np.isnan(s.xi), np.isnan(do.xi))
    assert np.array_equal(s.xi[~np.isnan(s.xi)], do.xi[~np.isnan(do.xi)])
    assert s.beta.shape == do.beta.shape and np.array_equal(s.beta, do.beta)
    assert len(s.nrmD) == len(do.nrmD)
    assert np.allclose(s.nrmD, do.nrmD, rtol=1e-10, atol=1e-14 * max(do.nrmD))
    # static: maxit steps after the freeze -- at kconv = 6 when the norms fell below tollin, at maxdgr + 1 when they did not
    assert s.kmax == (maxit + min(do.kconv, maxdgr) if static else maxit)


def test_setup_errors():
    """no nodes with leja = 0; repeated nodes with divided differences by differencing (one message for both places)"""
    with pytest.raises(ValueError, match="must be provided via 'nodes'"):
        nl._interpolation(SIGMA, np.array([np.inf]), np.zeros(0, dtype=complex), 0, False, 10, 100, 2, True)
    with pytest.raises(ValueError, match="must be distinct") as e1:         # 5 cyclic nodes tiled to 102: not distinct
        nl._interpolation(SIGMA, np.array([np.inf]), NODES0, 0, False, 10, 100, 2, False)
    gamma, nodes_, sigma, xi, beta = nl._interpolation(SIGMA, np.array([np.inf]), NODES0, 0, False, 10, 100, 0, True)
    with pytest.raises(ValueError, match="must be distinct") as e2:         # the Newton basis of a non-SPMF NEP differences too
        nl._divided_differences(None, True, sigma, xi, beta, 100, 102, True)
    assert str(e1.value) == str(e2.value)


def _coefficient_cases():
    rng = np.random.default_rng(7)
    for N in (1, 2, 7):
        sigma = rng.standard_normal(N + 3) + 1j * rng.standard_normal(N + 3)
        xi = 5 + rng.random(N + 3)
        beta = 0.5 + rng.random(N + 3)
        shift = complex(rng.standard_normal(), rng.standard_normal())
        yield N, "plain", shift, sigma, xi, beta
        xi_inf = xi.copy(); xi_inf[N - 1] = np.inf
        yield N, "inf", shift, sigma, xi_inf, beta
        yield N, "node", sigma[N - 1], sigma, xi, beta


@pytest.mark.parametrize("case", list(_coefficient_cases()), ids=lambda c: "N%d-%s" % (c[0], c[1]))
def test_step_coefficients(case):
    """cB_i = beta_i / xi_{i-1}; a_i = 1 / nu_i; b_1 = 0, b_i = (shift - sigma_{i-1}) / nu_i; bw_i = (shift - sigma_{i-1}) / nu_i with
    sigma_0 included; nu_i = beta_i (1 - shift / xi_{i-1}) -- with an infinite pole (cB = 0, nu = beta) and a shift on a node (mu = 0)"""
    N, kind, shift, sigma, xi, beta = case
    cB, a, b, bw = nl._step_coefficients(shift, sigma, xi, beta, N)
    with np.errstate(all="ignore"):
        nu = beta[1:N + 1] * (1 - shift / xi[:N])
        mu = shift - sigma[:N]
        cB_ref = beta[1:N + 1] / xi[:N]
        a_ref = 1.0 / nu
        b_ref = np.concatenate([[0], (shift - sigma[1:N]) / nu[1:]])
        bw_ref = mu / nu
    for got, ref in ((cB, cB_ref), (a, a_ref), (b, b_ref), (bw, bw_ref)):
        assert got.dtype == np.complex128 and got.flags.c_contiguous and got.shape == (N,)
        assert np.array_equal(got, ref.astype(np.complex128))
    if kind == "inf":
        assert cB[N - 1] == 0 and a[N - 1] == 1.0 / beta[N]
    if kind == "node":
        assert bw[N - 1] == 0 and (N == 1 or b[N - 1] == 0)


def _pencil_steps():
    rng = np.random.default_rng(3)
    sigma = rng.standard_normal(8) + 1j * rng.standard_normal(8)
    steps = [(l, l + 2, rng.standard_normal(l) + 1j * rng.standard_normal(l), float(rng.random() + 0.5)) for l in (1, 2, 3)]
    H = np.zeros((5, 4), dtype=complex); K = np.zeros((5, 4), dtype=complex)
    for l, k, h, hb in steps:                                  # K = H sigma_k + e_l e_l^T, column by column
        H[:l, l - 1] = h; H[l, l - 1] = hb
        K[:l + 1, l - 1] = H[:l + 1, l - 1] * sigma[k]
        K[l - 1, l - 1] += 1.0
    return types.SimpleNamespace(sigma=sigma), steps, H, K


def test_pencil_record():
    st, steps, H, K = _pencil_steps()
    pen = nl._Pencil(st, 5, False)
    assert pen.Hdev is None and pen.active_d is None
    for l, k, h, hb in steps:
        pen.record(l, k, h, hb)
    assert np.array_equal(pen.H, H) and np.array_equal(pen.K, K)


@pytest.mark.parametrize("flag", [0, 1, 2])
def test_pencil_flush(flag):
    """rows of Hdev as nep_orth_dev leaves them (h[0:l], beta, flags in the imaginary part of entry l+1), here in host memory:
    one flush records every pending column; flag 1 (a third pass wanted) raises _OrthPassMiss, flag 2 (breakdown) ArithmeticError"""
    st, steps, H, K = _pencil_steps()
    pen = nl._Pencil(st, 5, True, device="cpu")
    assert pen.Hdev.shape == (5, 7) and pen.active_d.shape == (5,)
    pen.flush()                                                # nothing pending: no copy, no change
    for l, k, h, hb in steps:
        row = np.zeros(7, dtype=complex)
        row[:l] = h; row[l] = hb; row[l + 1] = 1j * (flag if l == 2 else 0)
        pen.Hdev[l - 1].copy_(torch.from_numpy(row))
        pen.pending.append((l, k))
    if flag == 1:
        with pytest.raises(nl._OrthPassMiss):
            pen.flush()
    elif flag == 2:
        with pytest.raises(ArithmeticError, match="breakdown in nleigs step 4"):
            pen.flush()
    else:
        pen.flush()
        assert pen.pending == []
        assert np.array_equal(pen.H, H) and np.array_equal(pen.K, K)


def test_check_schedule():
    huge = np.iinfo(np.int64).max // 2
    minit, kmax = 4, 40
    count = 0
    for k, N, kconv, expand, static, rd, every in itertools.product(range(1, 41), (3, 6), (6, huge), (False, True), (False, True),
                                                                    (False, True), (1, 5)):
        if rd:
            due = not static or not expand
        else:
            due = ((not expand and k >= N + minit and (k - (N + minit)) % every == 0) or
                   (k >= kconv + minit and (k - (kconv + minit)) % every == 0) or k == kmax)
        assert nl._check_due(k, N, kconv, expand, static, minit, every, kmax, rd) == due
        count += due
    assert 0 < count < 40 * 64


class _FakeCache:
    closed = 0

    def close(self):
        self.closed += 1


def test_rerun_after_an_orth_pass_miss(monkeypatch):
    """the first run's cache is closed before the synchronous re-run starts; the re-run gets _sync_orth=True"""
    fake, sentinel, calls = _FakeCache(), object(), []

    def fake_nleigs(nep, *args, _cache_holder=None, _sync_orth=False, **kw):
        calls.append((_sync_orth, fake.closed, args, kw))
        if len(calls) == 1:
            _cache_holder.append(fake)
            raise nl._OrthPassMiss(3)
        return sentinel
    monkeypatch.setattr(nl, "_nleigs", fake_nleigs)
    misses = na.nleigs.orth_misses
    assert na.nleigs("nep", SIGMA, maxit=7) is sentinel
    assert calls == [(False, 0, (SIGMA,), {"maxit": 7}), (True, 1, (SIGMA,), {"maxit": 7})]
    assert fake.closed == 1 and na.nleigs.orth_misses == misses + 1


def test_cache_closed_when_the_run_raises(monkeypatch):
    fake, calls = _FakeCache(), []

    def fake_nleigs(nep, *args, _cache_holder=None, **kw):
        calls.append(kw)
        _cache_holder.append(fake)
        raise ValueError("from the run")
    monkeypatch.setattr(nl, "_nleigs", fake_nleigs)
    misses = na.nleigs.orth_misses
    with pytest.raises(ValueError, match="from the run"):
        na.nleigs("nep", SIGMA)
    assert len(calls) == 1 and fake.closed == 1 and na.nleigs.orth_misses == misses
