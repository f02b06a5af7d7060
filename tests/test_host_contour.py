"""Host-side tests of the contour drivers' stages (contour.py) and of the gates of the device-LU terms route (_devicelu.py): the
purity predicate, the gates ahead of any upload, the host LU strategy, Beyn's dense tail from the rows of the device QR, the
selection rule, the shared stream cache.  No GPU: nothing here launches a kernel or makes a stream."""
import sys

import numpy as np
import pytest
import scipy.linalg as sla
import scipy.sparse as sp

import nep_amd as na
from nep_amd import contour, funcs, _devicelu
from nep_amd.linsolvers import BackslashLinSolverCreator
from nep_amd.nep import pure_spmf, require_pure_spmf

OPS = ("Mlincomb", "Mder", "MM")


def _spmf(n=6):
    A = sp.identity(n, format="csc") * 2.0
    B = sp.diags([np.ones(n - 1), np.ones(n)], [1, 0], format="csc")
    return na.SPMF_NEP([A, B], [funcs.one(), funcs.ident()])


def _with_override(op):
    base = _spmf()
    sub = type("Override" + op, (type(base),), {"compute_" + op: lambda self, *a, **k: None})
    base.__class__ = sub
    return base


# ---- pure_spmf ------------------------------------------------------------------------------------------------------------------
def test_pure_spmf_of_the_plain_types():
    I3 = np.eye(3)
    for nep in (_spmf(), na.PEP([I3, 2 * I3, I3]), na.DEP([I3, 2 * I3], [0.0, 1.0])):
        assert pure_spmf(nep) and pure_spmf(nep, *OPS)
        for op in OPS:
            assert pure_spmf(nep, op)


@pytest.mark.parametrize("op", OPS)
def test_pure_spmf_override_is_impure_for_that_op_only(op):
    nep = _with_override(op)
    assert not pure_spmf(nep, op) and not pure_spmf(nep, *OPS)
    assert all(pure_spmf(nep, other) for other in OPS if other != op)
    assert pure_spmf(nep)                                   # still an AbstractSPMF


def test_pure_spmf_of_other_objects():
    for x in (None, object(), np.eye(2), na.nep.Mder_NEP.__new__(na.nep.Mder_NEP)):
        assert not pure_spmf(x) and not pure_spmf(x, "Mder")


def test_require_pure_spmf_message():
    require_pure_spmf(_spmf(), "nleigs")
    nep = _with_override("Mlincomb")
    with pytest.raises(NotImplementedError) as e:
        require_pure_spmf(nep, "nleigs")
    assert str(e.value) == ("nleigs: the operator has terms outside its SPMF matrices (type OverrideMlincomb); use iar / tiar / resinv / "
                            "quasinewton / augnewton, which go through the NEP's own compute_Mlincomb")
    with pytest.raises(NotImplementedError):
        require_pure_spmf(object(), "ilan")


# ---- the gates of the terms route: nothing is uploaded for a NEP that is refused ----------------------------------------------------
def _no_upload(nep, monkeypatch):
    def boom(self):
        raise AssertionError("aligned_terms_dev called: the term block would have been uploaded")
    monkeypatch.setattr(type(nep), "aligned_terms_dev", boom)
    return nep


def _lu_calls(nep):
    return (_devicelu.lu_from_terms(nep, 0.3, None, {}), _devicelu.lu_from_term_coeffs(nep, [1.0, 0.3]),
            _devicelu.lu_from_term_coeffs(nep, [1.0, 0.3], {"expected_solves": 3}))


def _default_switches(monkeypatch):
    for name in ("NEP_LU_DEV", "NEP_LU_SCHED", "NEP_LU_TERMS"):
        monkeypatch.delenv(name, raising=False)
    assert _devicelu._DeviceRefactor.enabled()


def test_terms_gate_switched_off(monkeypatch):
    _default_switches(monkeypatch)
    monkeypatch.setattr(_devicelu._DeviceRefactor, "plans", {"some pattern": dict(state="ready")})
    monkeypatch.setenv("NEP_LU_DEV", "0")
    nep = _no_upload(_spmf(), monkeypatch)
    assert _devicelu.terms_route(nep) is None and _lu_calls(nep) == (None,) * 3
    assert _devicelu.factor_term_rows(None, np.ones((1, 2)), 1) is None


def test_terms_gate_without_plans(monkeypatch):
    _default_switches(monkeypatch)
    monkeypatch.setattr(_devicelu._DeviceRefactor, "plans", {})
    assert _lu_calls(_no_upload(_spmf(), monkeypatch)) == (None,) * 3


def test_terms_gate_impure_nep(monkeypatch):
    _default_switches(monkeypatch)
    monkeypatch.setattr(_devicelu._DeviceRefactor, "plans", {"some pattern": dict(state="ready")})
    nep = _no_upload(_with_override("Mder"), monkeypatch)
    assert _devicelu.terms_route(nep) is None and _lu_calls(nep) == (None,) * 3
    # (a NEP that is pure for Mder gets as far as the upload: the gate is the purity, not something ahead of it)
    with pytest.raises(AssertionError, match="aligned_terms_dev called"):
        _devicelu.terms_route(_no_upload(_with_override("Mlincomb"), monkeypatch))


# ---- host LU strategy -------------------------------------------------------------------------------------------------------------
def test_host_lu_strategy():
    n = 5
    sym = sp.diags([np.ones(n - 1), 2 * np.ones(n), 3 * np.ones(n - 1)], [-1, 0, 1], format="csc")      # symmetric PATTERN only
    unsym = sp.diags([2 * np.ones(n), np.ones(n - 1)], [0, 1], format="csc")
    nodiag = sp.diags([np.ones(n - 1), np.ones(n - 1)], [-1, 1], format="csc")
    c = BackslashLinSolverCreator()
    assert contour.host_lu_strategy(c, sym) == dict(permc_spec="MMD_AT_PLUS_A", symmetric_mode=True)
    assert contour.host_lu_strategy(c, unsym) == dict(permc_spec="COLAMD", symmetric_mode=False)
    assert contour.host_lu_strategy(c, nodiag) == dict(permc_spec="COLAMD", symmetric_mode=False)
    assert contour.host_lu_strategy(BackslashLinSolverCreator(permc_spec="NATURAL"), sym) == dict(permc_spec="NATURAL")
    assert (contour.host_lu_strategy(BackslashLinSolverCreator(symmetric_mode=False, diag_pivot_thresh=0.5), sym)
            == dict(permc_spec=None, symmetric_mode=False, diag_pivot_thresh=0.5))
    assert (contour.host_lu_strategy(BackslashLinSolverCreator(diag_pivot_thresh=0.5), sym)
            == dict(permc_spec="MMD_AT_PLUS_A", symmetric_mode=True, diag_pivot_thresh=0.5))


# ---- Beyn's tail from the rows of the device QR ----------------------------------------------------------------------------------------
N_, K_, RANK, DROP = 40, 6, 3, 1e-8


def _moments_and_qr():
    """A0 = X Y (rank 3), A1 = X L Y, and (oh, G) of the UNSCALED moments 2 pi i A_j in the layout nep_orth_qr_dev writes: row j holds
    R[:j, j], the real R[j, j], and the flags of column j in the imaginary part of entry j + 1"""
    rng = np.random.default_rng(5)
    X = rng.standard_normal((N_, RANK)) + 1j * rng.standard_normal((N_, RANK))
    Y = rng.standard_normal((RANK, K_)) + 1j * rng.standard_normal((RANK, K_))
    A0 = X @ Y
    A1 = X @ np.diag([0.5, -0.3 + 0.2j, 1.1]) @ Y
    Q, R = np.linalg.qr(2j * np.pi * A0)
    ph = np.diag(R) / np.abs(np.diag(R))                       # Gram-Schmidt's sign convention: a real, positive diagonal
    Q = Q * ph[None, :]; R = R / ph[:, None]
    G = Q.conj().T @ (2j * np.pi * A1)
    oh = np.zeros((K_, K_ + 2), dtype=np.complex128)
    for j in range(K_):
        oh[j, :j] = R[:j, j]
        oh[j, j] = R[j, j].real
    return A0, A1, oh, G


def _flagged(oh, j, flag):
    oh = oh.copy()
    oh[j, j + 1] = 1j * flag
    return oh


def test_beyn_tail_from_qr_equals_the_host_tail():
    A0, A1, oh, G = _moments_and_qr()
    Sh, ph, Bh, V0 = contour.beyn_tail_host(A0, A1, DROP)
    Sq, pq, Bq, UrP = contour.beyn_tail_from_qr(oh, G, DROP)
    assert ph == pq == RANK and V0.shape == (N_, RANK) and UrP.shape == (K_, RANK) and Bq.shape == Bh.shape == (RANK, RANK)
    assert np.abs(Sq[:RANK] - Sh[:RANK]).max() <= 1e-12 * Sh[0]
    assert np.all(Sq[RANK:] <= DROP * Sq[0]) and np.all(Sh[RANK:] <= DROP * Sh[0])
    eh = np.sort_complex(sla.eigvals(Bh)); eq = np.sort_complex(sla.eigvals(Bq))
    print("eigenvalues of B, from the QR rows against the host tail: largest relative difference %.2e" % np.max(np.abs(eq - eh) / np.abs(eh)))
    assert np.all(np.abs(eq - eh) <= 1e-12 * np.abs(eh))
    assert np.all(np.abs(eh - np.sort_complex(np.array([0.5, -0.3 + 0.2j, 1.1]))) <= 1e-12 * np.abs(eh))


def test_beyn_tail_from_qr_flags():
    A0, A1, oh, G = _moments_and_qr()
    ref = contour.beyn_tail_from_qr(oh, G, DROP)
    assert abs(oh[K_ - 1, K_ - 1]) < 1e-10 * abs(oh[0, 0]) < abs(oh[1, 1])             # column 1 carries weight, the last is noise
    for j in range(K_):                                            # breakdown (bit 1) on any column
        assert contour.beyn_tail_from_qr(_flagged(oh, j, 2), G, DROP) is None
        assert contour.beyn_tail_from_qr(_flagged(oh, j, 3), G, DROP) is None
    for j in range(RANK):                                          # an unfinished re-orthogonalisation (bit 0) on a column with weight
        assert contour.beyn_tail_from_qr(_flagged(oh, j, 1), G, DROP) is None
    for j in range(RANK, K_):                                      # ... and on a noise column: ignored
        got = contour.beyn_tail_from_qr(_flagged(oh, j, 1), G, DROP)
        assert got is not None and got[1] == ref[1]
        assert all(np.array_equal(a, b) for a, b in zip((got[0], got[2], got[3]), (ref[0], ref[2], ref[3])))


# ---- selection --------------------------------------------------------------------------------------------------------------------
LAM = np.array([3.0, 0.5, -0.2, 2.0, 0.9j])


def test_select_inside_first_then_nearest_first():
    assert list(contour.select_eigenpairs(LAM, np.zeros(5), 0.5, 0j, (1, 1), 10)) == [2, 1, 4, 3, 0]
    assert list(contour.select_eigenpairs(LAM, np.zeros(5), 0.5, 0j, (2, 0.5), 10)) == [2, 1, 3, 4, 0]       # an ellipse; 2.0 on its boundary
    assert list(contour.select_eigenpairs(LAM, np.zeros(5), 0.5, 2.0 + 0j, (1.2, 1.2), 10)) == [3, 0, 1, 4, 2]
    assert list(contour.select_eigenpairs(LAM, np.array([0, 0, 1, 0, 0.5]), 0.5, 0j, (1, 1), 10)) == [1, 3, 0]   # errs < tol, strictly


def test_select_cap_and_no_sanity_check():
    assert list(contour.select_eigenpairs(LAM, np.zeros(5), 0.5, 0j, (1, 1), 2)) == [2, 1]
    assert list(contour.select_eigenpairs(LAM, np.zeros(5), 0.5, 0j, (1, 1), 5)) == [2, 1, 4, 3, 0]
    assert list(contour.select_eigenpairs(LAM, np.zeros(5), 0.5, 0j, (1, 1), np.inf)) == [2, 1, 4, 3, 0]
    assert list(contour.select_eigenpairs(LAM, None, 0.5, 0j, (1, 1), 2)) == [2, 1, 4, 3, 0]        # sanity_check=False: all pairs, no cap


def test_select_nothing_good():
    sel = contour.select_eigenpairs(LAM, np.ones(5), 0.5, 0j, (1, 1), 3)
    assert len(sel) == 0 and len(LAM[sel]) == 0
    assert len(contour.select_eigenpairs(LAM[:0], None, 0.5, 0j, (1, 1), 3)) == 0


# ---- one stream cache ---------------------------------------------------------------------------------------------------------------
def test_iar_and_contour_share_the_stream_cache():
    st = sys.modules["nep_amd._streams"]
    iar = sys.modules["nep_amd.iar"]
    assert iar._eig_streams is st._eig_streams is contour._eig_streams
    assert iar._check_stream is st._check_stream
    assert st._eig_streams.__globals__["_EIG_STREAMS"] is st._EIG_STREAMS
    assert st._check_stream.__globals__["_CHECK_STREAMS"] is st._CHECK_STREAMS
    assert not hasattr(iar, "_EIG_STREAMS") and not hasattr(iar, "_CHECK_STREAMS")          # no second cache
