"""The criteria of tests/hesseig_checkers.py on the host: both references (LAPACK; hq_ref, the NumPy restatement of k_hess_qr)
meet every case at or below an eighth of each constant, the constants follow from those measurements, the builders' preconditions
hold, and every mutant is rejected by at least one case.  test_gpu_hesseig.py runs the same criteria on the library."""
from functools import lru_cache

import numpy as np
import pytest

import hesseig_checkers as hc

KEYS = ("c1", "c2", "c3", "c4")


@lru_cache(None)
def _measured():
    """(largest value of every criterion, its case) per reference over every host case, and all violations"""
    best, bad = {}, []
    for which in ("lapack", "hq"):
        for c in hc.cases():
            if not c.host or (c.kind == "nonfinite" and which == "lapack"):      # (numpy.linalg.eig refuses non-finite input)
                continue
            wf, Z = hc.reference(c, which)
            rec = {}
            bad += [(which, c.name, b) for b in hc.evaluate(c, wf, Z, kernel_algorithm=which == "hq", record=rec)]
            for key in KEYS:
                if key in rec and rec[key] > best.get((key, which), (-1.0, None))[0]:
                    best[(key, which)] = (rec[key], c.name)
    hc.RATIOS.clear(); hc.RATIOS_BY_FAMILY.clear()                    # (the ratios are the device's report)
    return best, bad


@pytest.mark.parametrize("which", ["lapack", "hq"])
def test_reference_meets_every_case_at_an_eighth_of_the_constants(which):
    best, bad = _measured()
    assert not [b for b in bad if b[0] == which], bad
    for key in KEYS:
        v, name = best[(key, which)]
        print("%s %-6s largest value %.3g units (%s), constant %g" % (key.upper(), which, v, name, hc.CONST[key]))
        assert v <= hc.CONST[key] / 8, (key, which, v, name)


def test_constants_are_eight_times_the_measurement_rounded_up_to_a_power_of_two():
    best, _ = _measured()
    for key in KEYS:
        v = max(best[(key, "lapack")][0], best[(key, "hq")][0])
        first = 2.0 ** np.ceil(np.log2(8 * v))
        if key == "c4":
            # raised once: the float64 restatement of k_hess_invit, fed eigenvalues as far off as the device's, reaches the device's
            # level on the cyclic matrices (hesseig_checkers' docstring); next power of two above twice that level
            level = hc.zlaein_level()
            print("C4: first constant %g, zlaein level %.3g units" % (first, level))
            assert first == 64.0 and 83.1 <= level and hc.CONST[key] == 2.0 ** (np.floor(np.log2(2 * level)) + 1) == 256.0
        else:
            assert hc.CONST[key] == first, (key, v, hc.CONST[key])


def test_case_list_and_builder_preconditions():
    cs = hc.cases()
    assert len([c for c in cs if c.k > 64 and c.c2]) == 10
    for c in cs:
        if c.family == "e1":
            T = c.H * 2.0 ** -int(c.name.split("_s")[1])              # exact: a power of two
            assert np.abs(T.real).max() <= 8 and np.abs(T.imag).max() <= 8 and np.array_equal(T, np.round(T.real) + 1j * np.round(T.imag))
            assert np.array_equal(T, np.triu(T)) and len(set(np.diag(T).tolist())) == c.k
        if c.family == "e3":
            e = hc.amax_exp(c.H)
            for a, b in c.extra["blocks"]:
                assert hc.amax_exp(c.H[a:b, a:b]) == e
                assert a == 0 or c.H[a, a - 1] == 0
    assert {(c.k, c.extra["blocks"][1][0]) for c in cs if c.family == "e3"} >= {(3, 1), (5, 2), (66, 1), (70, 5), (70, 6), (128, 30), (128, 64)}
    assert [b for b in hc.by_name("e3_128_1_64_127").extra["blocks"]] == [(0, 1), (1, 64), (64, 127), (127, 128)]
    # shared with tests/test_gpu_kernels.py: the tolerances asserted there ride along
    for name, eig_tol, res_tol in (("gun_100", 1e-12, 1e-12), ("random_128", 1e-12, 1e-13), ("e2_random40_s+0", 1e-12, 1e-13),
                                   ("graded_40", 1e-9, 1e-12)):
        c = hc.by_name(name)
        assert (c.lapack_tol, c.res_tol) == (eig_tol, res_tol)


def test_hq_ref_needs_the_exceptional_shifts_on_the_cyclic_matrix():
    """the Wilkinson shift of the cyclic shift matrix is 0 and a QR step with shift 0 on a unitary Hessenberg matrix is a fixed point"""
    for k, sweeps in ((3, 14), (8, 30), (64, 163)):
        w, info, n = hc.hq_ref(hc.cyclic(k)[0])
        assert (info, n) == (0, sweeps)
    w, info, n = hc.hq_ref(hc.cyclic(8)[0], "no_exceptional")
    assert (info, n) == (8, 301) and np.all(w == 0)


def test_hq_ref_is_scale_invariant_bit_for_bit_and_refuses_non_finite_input():
    for c in hc.cases():
        if c.family == "e2" and c.extra["s"] != 0:
            c0 = hc.by_name(c.extra["base"])
            hc.check_scale_pair(c0, c, hc.reference(c0, "hq")[0], hc.reference(c, "hq")[0])
    for name in ("inf_5", "inf_70", "nan_5"):
        c = hc.by_name(name)
        assert hc.hq_ref(c.H)[1:] == (c.k, 0)
        hc.check(c, *hc.reference(c, "hq"))


def test_zlaein_restatement_report():
    """invit_ref (k_hess_invit's algorithm in float64): its C4 values are reported, not part of the constants; every vector it
    gives up on is zero and counted"""
    worst = (0.0, None)
    for c in hc.cases():
        if c.kind == "nonfinite" or not (c.k <= 66 or c.name == "cyclic_128"):
            continue
        wf, Z = hc.reference(c, "hq_zlaein")
        zero = ~np.any(Z != 0, axis=0)
        assert wf[c.k + 1].real == zero.sum() and (c.may_fail or not zero.any()), c
        v = hc.measure(c, wf[:c.k], Z, np.nonzero(~zero)[0])
        assert v.get("norm", 0.0) < 1e-14 and v.get("phase", 0.0) < 1e-14, (c, v)
        if v.get("c4", 0.0) > worst[0]:
            worst = (v["c4"], c.name)
    print("invit_ref: largest C4 value %.3g units (%s)" % worst)
    assert worst[0] <= hc.CONST["c4"] / 4, worst                      # (38.4 on cyclic_128: see the module's docstring)


MUTANT_CASES = tuple(c.name for c in hc.cases() if c.k <= 24) + ("cyclic_65", "e3_70_5")


@pytest.mark.parametrize("mut", hc.MUTANTS)
def test_mutant_is_rejected(mut):
    """each mutant of the references is rejected by at least one case; printed: how many assertions it misses on how many cases"""
    missed, rejecting = 0, []
    for name in MUTANT_CASES:
        c = hc.by_name(name)
        for which in (("hq",) if (mut in hc.IN_ALGORITHM or c.kind == "nonfinite") else ("lapack", "hq")):
            bad = hc.evaluate(c, *hc.reference(c, which, mut), kernel_algorithm=which == "hq")
            if bad:
                missed += len(bad); rejecting.append("%s/%s" % (name, which))
    hc.RATIOS.clear(); hc.RATIOS_BY_FAMILY.clear()
    print("%s: %d assertions missed on %d runs (%d cases), first %s" % (mut, missed, len(rejecting), len(MUTANT_CASES), rejecting[:3]))
    assert rejecting, mut
    if mut == "no_exceptional":
        assert any(r.startswith("cyclic") for r in rejecting)
    if mut == "below_read":
        assert "junk_below_22/hq" in rejecting
    if mut == "offset_ignored":
        assert any(r.startswith("e3") for r in rejecting)
    if mut == "z_rows_64_zero":
        assert any(r.startswith("cyclic_65") for r in rejecting)
