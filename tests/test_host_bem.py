"""Host-only tests of the boundary-element NEP: the mesh generator of nep_amd/bem.py, the NumPy restatement of tests/bem_checkers.py
against the reference's own known-answer test, and the checker itself (it accepts the float64 evaluation of the formulas and
rejects six mutants).  No GPU."""
import numpy as np
import pytest

import bem_checkers as bc
from nep_amd.bem import gen_ficheramesh, TriMesh

EPS = np.finfo(float).eps


# ---- gen_ficheramesh --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [1, 2, 3, 4])
def test_ficheramesh_counts_areas_and_surface(N):
    """n = 24 N_even^2 triangles of area 0.25 / N_even^2 each, every centre on the surface of the cube with the corner removed, and
    the total area is that surface's (6 faces of the cube: the three cut faces lose a quarter, the corner adds three quarters)"""
    m = gen_ficheramesh(N)
    Ne = N + N % 2
    assert isinstance(m, TriMesh) and len(m) == 24 * Ne * Ne
    assert m.vert.shape == (len(m), 3, 3) and m.area.shape == (len(m),)
    assert np.all(m.area == 0.25 / Ne / Ne)
    for t in range(len(m)):
        ctr = m.vert[t].sum(axis=0) / 3
        assert bc.on_surface(m.vert[t, 1]), t                       # P2 is the cell centre
        assert bc.on_surface(np.round(ctr, 12)), t
        P1, P2, P3 = m.vert[t]
        assert abs(np.linalg.norm(np.cross(P2 - P1, P3 - P1)) / 2 - m.area[t]) <= 4 * EPS
    assert abs(m.area.sum() - 6.0) <= 1e-13


@pytest.mark.parametrize("N", [1, 2, 4])
def test_ficheramesh_is_the_reference_order(N):
    """the same triangles in the same order with the same vertex order as the checker's restatement of genmesh.jl, bit for bit;
    spot values of the first patch (l = 1: x = 0, first cell) and of a patch with the other vertex order"""
    m = gen_ficheramesh(N)
    v, a = bc.gen_mesh(N)
    assert np.array_equal(m.vert, v) and np.array_equal(m.area, a)
    h = 1.0 / (N + N % 2)
    assert np.array_equal(m.vert[0], [[0, 0, 0], [0, h / 2, h / 2], [0, h, 0]])            # addtri(0, 0, 1, 0)
    first_high = 3 * 4 * (N + N % 2) ** 2
    assert np.array_equal(m.vert[first_high], [[1, 0, 0], [1, h / 2, h / 2], [1, 0, h]])   # addtri(0, 0, 0, 1)
    assert len(m[:5]) == 5 and np.array_equal(m[:5].vert, v[:5])


def test_ficheramesh_spot_triangles_worked_out_from_genmesh():
    """triangles of the N = 2 mesh worked out by hand from genmesh.jl:31-92 (grid = [0, 1/2, 1], nn = 1), independent of both ports:
    the first of patch l = 2 (y = 0, free dimensions (3, 1): the z index runs slower), the first two of patch l = 5 (x = 1, cell
    ii = 2, jj = 1, the vertex order of l >= 4) and the very last one (patch l = 15, z = 1/2, addtri(1, 0, 0, 0))"""
    m = gen_ficheramesh(2)
    assert np.array_equal(m.vert[16], [[0, 0, 0], [0.25, 0, 0.25], [0, 0, 0.5]])
    assert np.array_equal(m.vert[52], [[1, 0.5, 0], [1, 0.75, 0.25], [1, 0.5, 0.5]])
    assert np.array_equal(m.vert[53], [[1, 0.5, 0.5], [1, 0.75, 0.25], [1, 1, 0.5]])
    assert np.array_equal(m.vert[95], [[1, 0.5, 0.5], [0.75, 0.75, 0.5], [0.5, 0.5, 0.5]])


# ---- the restatement against the reference's KAT ----------------------------------------------------------------------------------
def test_restatement_reproduces_the_reference_kat():
    """test/gallery.jl:181-183: at n = 96, M(8.790558462139456 - 0.010815457827738698i) is rank deficient by Julia's rank tolerance,
    sigma_min <= n eps sigma_max (measured: sigma_min / sigma_max = 1.5e-16)"""
    M = bc.mfun("full96")(bc.LAM_REF)
    assert M.shape == (96, 96) and np.array_equal(M, M.T)
    s = np.linalg.svd(M, compute_uv=False)
    print("sigma_min / sigma_max = %.3g" % (s[-1] / s[0]))
    assert s[-1] <= 96 * EPS * s[0]
    assert s[-2] > 1e3 * 96 * EPS * s[0]                           # exactly one
    # and the same in the reference's own form of the singular part (long double: it cancels in float64)
    S_ref = bc.eval_static("full96", bc.LD, form="dehoop")
    assert float(np.max(np.abs(S_ref - bc.reference("full96").S0))) <= 1e-19


def test_singular_part_is_not_symmetric_before_mirroring():
    """max |S0 - S0^T| = 1.1e-5 against max |S0| = 3.6e-3 at n = 96: the mirror is a choice, not a symmetry"""
    S = bc.eval_static("full96", mirror=False)
    asym, big = float(np.max(np.abs(S - S.T))), float(np.max(np.abs(S)))
    print("max |S0 - S0^T| = %.3g, max |S0| = %.3g" % (asym, big))
    assert 1.0e-5 < asym < 1.2e-5 and 3.5e-3 < big < 3.7e-3


def test_newton_on_the_restatement_finds_both_eigenvalues():
    M = bc.mfun("full96")
    lam, _, steps = bc.augnewton_numpy(M, 8.8, np.ones(96))
    assert abs(lam - bc.LAM_REF) <= 1e-14 * abs(bc.LAM_REF) and steps <= 6, (lam, steps)
    lam, _, steps = bc.augnewton_numpy(M, 7.0, np.ones(96))
    assert abs(lam - bc.LAM_REF2) <= 1e-13 * abs(bc.LAM_REF2) and steps <= 10, (lam, steps)


# ---- the checker accepts the float64 evaluation ---------------------------------------------------------------------------------
@pytest.mark.parametrize("name", bc.MESHES)
def test_checker_accepts_float64_static(name):
    r = bc.check_static(name, bc.eval_static(name))
    print("%s: S0 in float64 at %.3g of the bound" % (name, r))


@pytest.mark.parametrize("der", bc.DERS)
@pytest.mark.parametrize("name", bc.MESHES)
def test_checker_accepts_float64_matrices(name, der):
    worst = max(bc.check_mder(name, lam, der, bc.eval_mder(name, lam, der)) for lam in bc.LAMS)
    print("%s der %d: float64 at %.3g of the bound" % (name, der, worst))


@pytest.mark.parametrize("ksd", bc.MLINCOMB)
@pytest.mark.parametrize("name", bc.MESHES)
def test_checker_accepts_float64_mlincomb(name, ksd):
    k, sd = ksd
    lam, a, V = bc.operands(name, k, sd)
    assert k < 3 or (np.count_nonzero(a == 0) >= 1 and np.all(np.isnan(V[:, a == 0])))
    r = bc.check_mlincomb(name, lam, a, sd, np.nan_to_num(V), bc.eval_mlincomb(name, lam, a, sd, V))
    print("%s k %d startder %d: float64 at %.3g of the bound" % (name, k, sd, r))


# ---- and rejects the mutants ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mut,der", [("swapped", 0), ("zero_d0", 0), ("zero_d1", 1), ("no_minus_one", 0), ("s0_no_4pi", 0)])
def test_checker_rejects_matrix_mutants(mut, der):
    """lower triangle with the roles swapped instead of mirrored; the d = 0 pairs of der = 0 set to 0 instead of i lam W; those of
    der = 1 set to 0; the -1 of der = 0 dropped; 1 / (4 pi) missing on S0 only"""
    for name in ("first65", "full96"):
        lam = 5 + 0.3j
        M, b, _ = bc.reference(name).mder(lam, der)
        with pytest.raises(AssertionError):
            bc._ratio("mutant", name, bc.eval_mder(name, lam, der, mut=mut), M, b)


def test_checker_rejects_static_mutants():
    for name in ("first65", "full96"):
        ref = bc.reference(name)
        for kw in ({"mirror": False}, {"scale": False}):
            with pytest.raises(AssertionError):
                bc._ratio("mutant", name, bc.eval_static(name, **kw), ref.S0, ref.S0_bound)


@pytest.mark.parametrize("ksd", [(1, 0), (1, 1), (5, 1)])
def test_checker_rejects_horner_shifted_by_one(ksd):
    k, sd = ksd
    lam, a, V = bc.operands("full96", k, sd)
    with pytest.raises(AssertionError):
        bc.check_mlincomb("full96", lam, a, sd, np.nan_to_num(V), bc.eval_mlincomb("full96", lam, a, sd, V, shift=1), kind="mutant")
