"""The checkers of tests/wep_checkers.py can fail, and their cases are what they are named for: driven on the host with the float64
NumPy restatement `ref` (which has to pass every case the host affords) and with its mutants, each of which some case has to reject;
nep_wep_plan (host-only) confirms the instantiation named in every case, that the case list reaches every instantiation, the refusal
sizes, and agrees with the Python restatement of the launch predicates for every nz <= 2500.  test_gpu_wep_checkers.py runs the same
checkers on the library."""
import ctypes as C

import numpy as np
import pytest

import primitive_checkers as pc
import wep_checkers as wc

HOST_MAX_COST = 600 * 600 * 40                              # larger cases reach their reference on the device run only
PASSED, REJECTED = [0], []


def _plan(nz, nx, op):
    import nep_amd as na
    info = (C.c_int64 * 8)()
    rc = na._lib.lib.nep_wep_plan(nz, nx, op, info)
    return rc, [int(v) for v in info]


def _host_cases(k):
    return [c for c in k.cases() if wc._cost(c) <= HOST_MAX_COST]


def test_extended_fft_is_extended():
    """np.fft keeps np.clongdouble (else xfft falls back to the dense extended DFT) and agrees with that dense DFT to 1e-17 relative"""
    rng = np.random.default_rng(3)
    for nz in (15, 105, 1199):
        a = pc.grand(rng, (3, nz)).astype(wc.CLD)
        for sign in (-1, +1):
            f, g = wc.xfft(a, sign), wc.xfft(a, sign, dense=True)
            assert f.dtype == wc.CLD and g.dtype == wc.CLD
            assert float(np.abs(f - g).max()) <= 1e-17 * float(np.abs(g).max()) * np.log2(nz)
    x = pc.grand(rng, (2, 15))
    assert np.allclose(wc.xfft(x, -1), np.fft.fft(x, axis=1)) and np.allclose(wc.xfft(x, +1), np.fft.ifft(x, axis=1) * 15)


@pytest.mark.parametrize("name", list(wc.CHECKERS))
def test_restatement_passes_every_case(name):
    k = wc.CHECKERS[name]
    n = 0
    for c in _host_cases(k):
        n += k.check(k.ref, c)
    assert n >= 3, (name, n)
    PASSED[0] += n
    print("%s: %d calls passed" % (name, n))


def test_sylvester_reference_solves_the_equation():
    """the restated solve against the equation it is named for, A X + X B = C with the circulant A of eigenvalues d_i in the basis F
    and B = b tridiag(1, -2, 1), formed densely"""
    nz, nx = 15, 19
    rng = np.random.default_rng(5)
    o = wc.sylv_operands(rng, nz, nx)
    Cm = pc.grand(rng, (nx, nz))
    X = wc.sylv(o["d"], o["b"], Cm)                            # (nx, nz)
    F = np.fft.fft(np.eye(nz), axis=0) / np.sqrt(nz)
    A = F @ np.diag(o["d"]) @ F.conj().T
    B = o["b"] * (np.diag(np.full(nx - 1, 1.0), 1) + np.diag(np.full(nx - 1, 1.0), -1) - 2 * np.eye(nx))
    res = A @ X.T + X.T @ B - Cm.T
    assert np.linalg.norm(res) <= 1e-12 * np.linalg.norm(Cm)


def _rejecting_case(k, mut):
    kinds = ("exact", "rounded") if mut == "perturb" else ("exact", "rounded", "measured")
    for c in sorted(_host_cases(k), key=wc._cost):
        if c.kind not in kinds:
            continue
        try:
            k.check(partial_mut(k, mut), c)
        except AssertionError:
            return c
    return None


def partial_mut(k, mut):
    return lambda *a, **kw: k.ref(*a, mut=mut, **kw)


@pytest.mark.parametrize("name,mut", [(n, m) for n, k in wc.CHECKERS.items() for m in k.mutants])
def test_every_mutant_is_rejected(name, mut):
    """stencil / boundary: no periodic wrap, the wrap to the wrong end, the x-neighbour applied at x = 0, c1s on the wrong column, d1
    and d2 swapped, the plus half gathered in swapped order; P^{-1}: no reversal, bb not conjugated, halves of sinv swapped; regions:
    x offset 2 dropped, boundary regions weighted 1/L, last row of a z-region dropped, rx off by one for x >= nx - 2, dd1 / dd2 swapped
    on the plus half; Thomas: last x not solved, sign of b, the carry across a lane boundary, the last partial column group; SMW:
    alpha = MinvH f, pb not subtracted from the last column, the second solve added, the second batch at the first batch's offset;
    one result off by 1e-13 (exact and entrywise-bounded cases)"""
    k = wc.CHECKERS[name]
    ratios = dict(pc.RATIOS)
    c = _rejecting_case(k, mut)
    pc.RATIOS.clear(); pc.RATIOS.update(ratios)
    assert c is not None, "no case rejects the mutant %r of %s" % (mut, name)
    REJECTED.append((name, mut))
    print("%s/%s rejected by %r" % (name, mut, c))


def test_plan_confirms_every_case_and_the_cases_cover_every_instantiation():
    """nep_wep_plan says which instantiation every case runs; the union has to be the full set: {rb, plain<2>, plain<1>, sym<2,2>}
    and SEG {1 .. 32} for MODE 0 (every SEG, and every form under both layouts of the transposed block: plain and TLay pieces), SEG
    {1 .. 32} for MODE 1 / 2, P^{-1} {plain 256 / 512 / 1024, sym}.  A case list that loses one fails here."""
    seen0, seen12, seenp = set(), set(), set()
    for c in wc.CHECKERS["nep_wep_sylv_solve"].cases():
        e = c.extra
        rc, info = _plan(e["nz"], e["nx"], wc.OP_SYLV)
        assert rc == 0 and (wc.dft_form(info), info[7]) == (e["form"], e["seg"]), (c, info)
        assert (rc, info) == wc.predict(e["nz"], e["nx"], wc.OP_SYLV)
        seen0.add((wc.dft_form(info), info[7]))
    forms0 = {f for f, _ in seen0}
    assert forms0 == {"rb", "plain<2>", "plain<1>", "sym<2,2>"}, forms0
    assert {s for _, s in seen0} == {1, 2, 4, 8, 16, 32}, seen0
    for f in forms0:                                          # the transform meets the tridiagonal kernel in the layout of T only
        assert {s >= 4 for g, s in seen0 if g == f} == {False, True}, "%s: not under both layouts of the transposed block" % f
    # the sizes the issue names for their thread counts and partial groups
    assert _plan(1443, 7, wc.OP_SYLV)[1][5] == 384 and _plan(2055, 6, wc.OP_SYLV)[1][:2] == [137, 15]
    assert _plan(2400, 5, wc.OP_SYLV)[1][:2] == [75, 32] and _plan(2401, 5, wc.OP_SYLV)[1][:2] == [2401, 1] and _plan(7, 2, wc.OP_SYLV)[1][1] == 1
    assert any(c.extra["nx"] % _plan(c.extra["nz"], c.extra["nx"], wc.OP_SYLV)[1][3] for c in wc.CHECKERS["nep_wep_sylv_solve"].cases())
    for name in ("nep_wep_pinv_apply", "nep_wep_schur_matvec"):
        for c in wc.CHECKERS[name].cases():
            if "form" not in c.extra:
                continue
            rc, info = _plan(c.extra["nz"], 0, wc.OP_PINV)
            assert rc == 0 and wc.pinv_form(info) == c.extra["form"], (c, info)
            seenp.add(wc.pinv_form(info))
    assert _plan(1001, 0, wc.OP_PINV)[1][5] == 512 and _plan(1155, 0, wc.OP_PINV)[1][2] == wc.K_PLAIN
    for c in wc.CHECKERS["nep_wep_smw_apply"].cases():
        e = c.extra
        rc, info = _plan(e["nz"], e["nx"], wc.OP_SMW)
        assert rc == 0 and info[7] == e["seg"] and info[2] == wc.K_SYM and info[6] == 4 * e["nx"] * 16, (c, info)
        rcp, ip = _plan(e["nz"], 0, wc.OP_PINV)
        assert rcp == 0 and wc.pinv_form(ip) == e["pinv"], (c, ip)
        seen12.add(info[7]); seenp.add(wc.pinv_form(ip))
    assert seen12 == {1, 2, 4, 8, 16, 32}, seen12
    assert _plan(1443, 1447, wc.OP_SMW)[1][6] == 92608 > 64 * 1024 and _plan(1023, 0, wc.OP_PINV)[1][5] == 512
    for k in (wc.CHECKERS["nep_wep_smw_matrix"], wc.CHECKERS["nep_wep_smw_matrix_modes"]):
        for c in k.cases():
            rc, info = _plan(c.extra["nz"], c.extra["nx"], wc.OP_SMW)
            assert rc == 0 and info[7] == c.extra["seg"], (c, info)
    assert seenp == {"plain256", "plain512", "plain1024", "sym"}, seenp
    print("MODE 0: %d (form, SEG) pairs %s; MODE 1/2: SEG %s; P^-1: %s" % (len(seen0), sorted(seen0), sorted(seen12), sorted(seenp)))


def test_plan_refusals():
    """the refusal sizes of test_gpu_wep_checkers.py, with their codes and info all zero"""
    Z = [0] * 8
    for nz, nx in wc.REFUSE_SYLV_ARG:
        assert _plan(nz, nx, wc.OP_SYLV) == (-2, Z)
    big = wc.first_unstaged_nz(lambda nz, nx, op: _plan(nz, nx, op)[0])
    assert _plan(big, 5, wc.OP_SYLV) == (-5, Z) and _plan(big - 1, 5, wc.OP_SYLV)[0] == 0
    assert (2 * big + sum(wc.factor(big))) * 16 > wc.LDS_MAX
    assert _plan(wc.REFUSE_PINV_NZ, 0, wc.OP_PINV) == (-5, Z) and _plan(wc.REFUSE_PINV_NZ - 1, 0, wc.OP_PINV)[0] == 0
    assert _plan(wc.REFUSE_SMW_EVEN, wc.REFUSE_SMW_EVEN + 4, wc.OP_SMW) == (-5, Z)
    assert _plan(15, 20, wc.OP_SMW) == (-2, Z) and _plan(0, 4, wc.OP_SYLV) == (-2, Z) and _plan(15, 19, 3) == (-2, Z)
    import nep_amd as na
    assert na._lib.lib.nep_wep_plan(15, 19, 0, None) == -2
    print("first nz beyond the transform staging: %d" % big)


def test_plan_equals_the_restated_predicates():
    """for every nz <= 2500 at nx = 2 and nz + 4, all three ops"""
    n = 0
    for nz in range(1, 2501):
        for nx in (2, nz + 4):
            for op in (wc.OP_SYLV, wc.OP_PINV, wc.OP_SMW):
                assert _plan(nz, nx, op) == wc.predict(nz, nx, op), (nz, nx, op, _plan(nz, nx, op), wc.predict(nz, nx, op))
                n += 1
    print("plans compared: %d" % n)


def test_sylvester_plan_takes_every_grid_the_preconditioner_admits():
    """WEPPreconditioner insists on nx = nz + 4 and a WEP on odd nz: for every such grid up to nx = 2048 the Sylvester solve has a
    plan, and nx = 2049 is refused as an argument error -- so nep_wep_sylv_create never answers "unsupported" to the preconditioner,
    which therefore keeps no dense-transform route"""
    for nz in range(1, 2045, 2):
        assert _plan(nz, nz + 4, wc.OP_SYLV)[0] == 0, nz
    assert _plan(2045, 2049, wc.OP_SYLV) == (-2, [0] * 8)


def test_zz_report():
    total = sum(len(k.mutants) for k in wc.CHECKERS.values())
    print("calls passed by the restatement: %d; mutants rejected: %d of %d" % (PASSED[0], len(REJECTED), total))
    for k in sorted(pc.RATIOS):
        if k.startswith("nep_wep"):
            print("ratio %-44s %.3g" % (k, pc.RATIOS[k]))
