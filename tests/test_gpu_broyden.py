"""broyden on the device: nep_broyden_sweep (csrc/broyden.hip) through the raw C ABI on the cases of tests/broyden_checkers.py, and
the driver as test/broyden.jl runs it, on dep1, dep0 and dep0_sparse, against the dense restatement of src/method_broyden.jl."""
import ctypes as C
import math

import numpy as np
import pytest
import scipy.sparse as sp
import torch

import broyden_checkers as bc
import primitive_checkers as pc

pytestmark = pytest.mark.gpu
EPS = np.finfo(float).eps
SQEPS = math.sqrt(EPS)


@pytest.fixture(scope="module")
def na():
    import nep_amd
    if nep_amd.device_count() < 1:
        pytest.skip("no GPU")
    return nep_amd


# ---- nep_broyden_sweep through the C ABI ----------------------------------------------------------------------------------------
def _sweep_raw(n, T, ldt, lead, u0, a0, x, y, w, g, null=(), alias=None):
    """uploads the buffers, calls the library, downloads T, y, g.  null: names passed as NULL; alias = (out, target, offset):
    the pointer of y or g is replaced by one inside another buffer."""
    from nep_amd import _lib
    from nep_amd.nep import stream_ptr
    up = lambda b: None if b is None else torch.from_numpy(np.ascontiguousarray(b)).to("cuda")
    d = dict(T=up(T), u0=up(u0), a0=up(a0), x=up(x), y=up(y), w=up(w), g=up(g))
    d["work"] = torch.full((max(int(_lib.lib.nep_broyden_sweep_worksize(max(n, 1))), 1),), pc.NAN, dtype=torch.complex128, device="cuda")
    off = dict(T=lead, y=bc.LEAD, g=bc.LEAD)
    addr = {k: (None if t is None else t.data_ptr() + 16 * off.get(k, 0)) for k, t in d.items()}
    if alias is not None:
        out, target, o = alias
        addr[out] = addr[target] + 16 * o
    ptr = lambda k: None if (k in null or addr[k] is None) else C.c_void_p(addr[k])
    rc = _lib.lib.nep_broyden_sweep(n, ptr("T"), ldt, ptr("u0"), ptr("a0"), ptr("x"), ptr("y"), ptr("w"), ptr("g"), ptr("work"),
                                    stream_ptr())
    torch.cuda.synchronize()
    for k, b in (("u0", u0), ("a0", a0), ("x", x), ("w", w)):
        assert b is None or np.array_equal(d[k].cpu().numpy(), b), "d%s was modified" % k
    dn = lambda k: None if d[k] is None else d[k].cpu().numpy()
    return rc, dn("T"), dn("y"), dn("g")


def _impl(**a):
    rc, T, y, g = _sweep_raw(**a)
    assert rc == 0, rc
    return T, y, g


CASES = list(bc.SWEEP.cases())


@pytest.mark.parametrize("case", CASES, ids=[repr(c) for c in CASES])
def test_broyden_sweep_case(na, case):
    bc.SWEEP.check(_impl, case)
    print("%r: largest |impl - ref| / bound so far = %.3g" % (case, pc.RATIOS.get(bc.SWEEP.name, 0.0)))


def test_broyden_sweep_two_calls_give_the_same_bits(na):
    picked = [c for c in CASES if c.kind == "rounded" and "uxw" in c.cid]
    assert len(picked) == 20
    for c in picked:
        a = c.args
        one, two = _impl(**a), _impl(**a)
        for p, q in zip(one, two):
            assert p.tobytes() == q.tobytes(), c


def test_broyden_sweep_error_codes_launch_nothing(na):
    from nep_amd import _lib
    base = bc.BroydenSweep._build(65, 3, True, True, True, "exact", bc.LEAD, pc.SENT)
    n, ldt = 65, 68
    bad = [({"n": 0}, {}), ({"ldt": 64}, {}), ({}, {"null": ("T",)}), ({}, {"null": ("work",)}),
           ({}, {"null": ("u0",)}), ({}, {"null": ("a0",)}), ({}, {"null": ("x",)}), ({}, {"null": ("y",)}),
           ({}, {"null": ("w",)}), ({}, {"null": ("g",)}), ({}, {"null": ("u0", "a0", "x", "y", "w", "g")}),
           ({}, {"alias": ("y", "T", 0)}), ({}, {"alias": ("y", "T", ldt * (n - 1) + n - 1)}), ({}, {"alias": ("g", "T", 5)}),
           ({}, {"alias": ("y", "work", 0)}), ({}, {"alias": ("g", "work", n)}),
           ({}, {"alias": ("y", "u0", 0)}), ({}, {"alias": ("y", "a0", n - 1)}), ({}, {"alias": ("y", "x", 0)}),
           ({}, {"alias": ("y", "w", 1)}), ({}, {"alias": ("g", "u0", 0)}), ({}, {"alias": ("g", "a0", 0)}),
           ({}, {"alias": ("g", "x", n - 1)}), ({}, {"alias": ("g", "w", 0)}), ({}, {"alias": ("g", "y", 1 - n)})]
    for change, how in bad:
        rc, T, y, g = _sweep_raw(**dict(base, **change), **how)
        assert rc == _lib.NEP_ERR_ARG, (change, how, rc)
        assert np.array_equal(T, base["T"], equal_nan=True), (change, how)
        assert np.array_equal(y, base["y"], equal_nan=True) and np.array_equal(g, base["g"], equal_nan=True), (change, how)
    rc, T, y, g = _sweep_raw(**base)                                     # the unchanged call is accepted
    assert rc == 0 and not np.isnan(y[bc.LEAD: bc.LEAD + n]).any() and not np.isnan(g[bc.LEAD: bc.LEAD + n]).any()


# ---- the driver -----------------------------------------------------------------------------------------------------------------
def _dense(M):
    return M.toarray() if sp.issparse(M) else np.asarray(M)


def _host_residual(nep, lam, x):
    return np.linalg.norm(_dense(nep.compute_Mder(lam)) @ x) / np.linalg.norm(x)


def _sigma_min(nep, lam):
    return np.linalg.svd(_dense(nep.compute_Mder(lam)), compute_uv=False)[-1]


def _pair_residual(nep, S, X):
    """||M(S, X)||_2 on the host, from the dense restatement of the problem"""
    return bc.pair_residual(bc.ref_dep_of(nep), S, X)


def test_dep1_invariant_pair(na):
    """test/broyden.jl:6-9"""
    nep = na.nep_gallery("dep1")
    info = {}
    S, X, T1, eh, th, ih = na.broyden(nep, info=info)
    res = _pair_residual(nep, S, X)
    print("diag(S)", np.diag(S), "pair residual %.3g" % res, info)
    assert S.shape == (3, 3) and X.shape == (3, 3) and res < SQEPS
    assert torch.is_tensor(T1) and T1.is_cuda and torch.equal(T1.cpu(), torch.eye(3, dtype=torch.complex128))
    assert info["sweeps"] == sum(info["iters"]) and len(eh) == len(th) == len(ih) == sum(info["iters"])
    # the product's own compute_MM agrees with the host residual
    assert np.linalg.norm(np.asarray(nep.compute_MM(S, X)), 2) < SQEPS


def test_dep1_addconj_with_clamped_pmax(na):
    """test/broyden.jl:11-15: pmax = 5 is clamped to n = 3; the third pair is complex, its conjugate is added"""
    nep = na.nep_gallery("dep1")
    info = {}
    with pytest.warns(UserWarning, match="Too many eigenvalues requested"):
        S, X, *_ = na.broyden(nep, addconj=True, pmax=5, info=info)
    assert info["pmax"] == 3 and S.shape == (4, 4) and X.shape == (3, 4)
    lam, Y = np.linalg.eig(S)
    V = X @ Y
    res = [_host_residual(nep, l, v) for l, v in zip(lam, V.T)]
    print("eigenvalues", lam, "residuals", res)
    assert len(lam) == 4 and max(res) < SQEPS


def test_dep0_published_values(na):
    """method_broyden.jl:203-216"""
    nep = na.nep_gallery("dep0")
    S, X, *_ = na.broyden(nep)
    d = np.diag(S)
    sm = [_sigma_min(nep, l) for l in d]
    print("diag(S)", d, "sigma_min", sm)
    assert abs(d[0] - (-0.15955391823299253)) < 1e-10
    assert len(d) == 3 and max(sm) < SQEPS


def _assert_converged_pair(nep, S, X, info, eh, p):
    res = _pair_residual(nep, S, X)
    print("iterations", info["iters"], "diag(S)", np.diag(S), "pair residual %.3g" % res,
          "host synchronisations per iteration %.1f" % info["syncs_per_iteration"], "T traffic %.3g GB" % (info["t_bytes"] / 1e9))
    assert S.shape == (p, p) and X.shape[1] == p
    assert max(info["iters"]) < 1000 and np.nanmin(eh) < 1e-12          # every level stopped on its error measure
    last = np.cumsum(info["iters"]) - 1
    assert len(eh) == sum(info["iters"]) and np.all(eh[last] < 1e-12)
    assert res < SQEPS
    assert np.linalg.norm(X.conj().T @ X - np.eye(p)) < 1e-10
    assert info["sweeps"] == sum(info["iters"])


def test_dep0_sparse_from_the_identity(na):
    nep = na.nep_gallery("dep0_sparse", 100)
    info = {}
    S, X, T1, eh, th, ih = na.broyden(nep, "eye", info=info)
    _assert_converged_pair(nep, S, X, info, eh, 3)


def test_dep0_sparse_257_from_the_problem_itself(na):
    """approxnep = nep: M1 = M(0) is sparse, T1 = inv(M1) by block solves of its device LU; more than one column tile"""
    nep = na.nep_gallery("dep0_sparse", 257)
    info = {}
    S, X, T1, eh, th, ih = na.broyden(nep, nep, info=info)
    _assert_converged_pair(nep, S, X, info, eh, 3)
    M1 = _dense(nep.compute_Mder(0.0))
    assert np.linalg.norm(T1.cpu().numpy().T @ M1 - np.eye(257)) < 1e-9
    assert max(info["iters"]) <= 200


def test_dep0_sparse_addconj(na):
    nep = na.nep_gallery("dep0_sparse", 100)
    info = {}
    S, X, T1, eh, th, ih = na.broyden(nep, addconj=True, pmax=4, info=info)
    p = S.shape[0]
    assert p in (4, 5)                                                   # a conjugate added at the last level gives pmax + 1
    res = _pair_residual(nep, S, X)
    print("iterations", info["iters"], "eig(S)", np.linalg.eigvals(S), "pair residual %.3g" % res)
    assert max(info["iters"]) < 1000 and res < SQEPS
    assert np.linalg.norm(X.conj().T @ X - np.eye(p)) < 1e-10
    assert info["sweeps"] == sum(info["iters"])
    assert len(info["iters"]) < p                                        # at least one column came from a conjugate


def test_dense_matrix_as_approxnep(na):
    """approxnep as an n x n array: T1 by the library's dense inverse"""
    nep = na.nep_gallery("dep0")
    M1 = _dense(nep.compute_Mder(0.0)).astype(complex)
    info = {}
    S, X, T1, *_ = na.broyden(nep, M1, pmax=2, info=info)
    assert np.linalg.norm(T1.cpu().numpy().T @ M1 - np.eye(5)) < 1e-12
    assert _pair_residual(nep, S, X) < SQEPS and max(info["iters"]) < 1000


def test_invpow_finds_an_invariant_pair(na):
    nep = na.nep_gallery("dep0_sparse", 100)
    info = {}
    S, X, *_ = na.broyden(nep, eigmethod="invpow", pmax=2, info=info)
    res = _pair_residual(nep, S, X)
    print("iterations", info["iters"], "diag(S)", np.diag(S), "pair residual %.3g" % res, "set-up passes", info["setup_passes"])
    assert max(info["iters"]) < 1000 and res < SQEPS


def test_eigs_raises(na):
    with pytest.raises(ValueError, match="sparse eigensolver"):
        na.broyden(na.nep_gallery("dep1"), eigmethod="eigs")


def test_custom_errmeasure_and_histories(na):
    nep = na.nep_gallery("dep0")
    seen = []

    def em(lam, v, r):
        seen.append((lam, v.shape, r.shape))
        return np.linalg.norm(r) / np.linalg.norm(v)
    info = {}
    S, X, T1, eh, th, ih = na.broyden(nep, pmax=2, errmeasure=em, add_nans=True, check_error_every=5, info=info)
    i1, tot = info["iters"][0], sum(info["iters"])
    assert len(seen) == tot // 5 and seen[0][1:] == ((5,), (5,))
    assert len(eh) == len(th) == len(ih) == tot + 1                      # :385: one NaN in front of the second level
    assert np.isnan(ih[i1]) and np.isnan(eh[i1]) and np.isnan(th[i1])
    assert np.array_equal(np.delete(ih, i1), np.arange(1, tot + 1)) and np.all(np.diff(th[np.isfinite(th)]) > 0)
    assert np.count_nonzero(np.isfinite(eh)) == len(seen)


def test_recurrence_drift(na):
    """T*rk is never recomputed: it follows the recurrence  T_new rkp = gamma Tztilde + (1 - gamma) Trk + Tztilde (aH rkp).  With
    the private keyword the driver applies the pending update at every error check and compares a fresh T*rk (a sweep) with the
    recurrence, relative to ||T||_F ||rk||.  The largest value may be at most 100 times the same quantity of the pending-update
    restatement on the same input (computed here): the margin covers another summation order and diverging trajectories."""
    nep = na.nep_gallery("dep0_sparse", 100)
    ref_drift = []
    bc.ref_broyden(bc.ref_dep_of(nep), form="pending", drift=ref_drift)
    drift, info = [], {}
    S, X, *_ = na.broyden(nep, "eye", info=info, _drift=drift)
    print("device: %d checks, largest drift %.3g; restatement: %d checks, largest drift %.3g"
          % (len(drift), max(drift), len(ref_drift), max(ref_drift)))
    assert len(drift) == sum(info["iters"]) // 10 == info["drift_sweeps"]
    assert max(drift) <= 100 * max(ref_drift)
    assert _pair_residual(nep, S, X) < SQEPS
