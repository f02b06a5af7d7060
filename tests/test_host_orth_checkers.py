"""The checkers of tests/orth_checkers.py can fail: driven on the host with the float64 NumPy model of K6 (nep_orth, nep_orth_dev,
nep_orth_dev_mirror, nep_orth_dev_iar_next) and of K9 (nep_gemm_h_rm), which has to pass every host case (the builders assert the
exactness and the criterion margins of every case on the way), and with a fixed list of mutants, each of which a named case has to
reject.  test_gpu_orth_checkers.py runs the same checkers on the library."""
from functools import partial

import numpy as np
import pytest

import orth_checkers as oc
import primitive_checkers as pc


@pytest.mark.parametrize("group", oc.groups(oc.K6))
def test_k6_numpy_model_passes_every_host_case(group):
    n = calls = 0
    for c in oc.K6.cases():
        if c.group == group and c.host:
            calls += oc.K6.check(oc.K6.ref, c)
            n += 1
    if group == "big":
        assert n == 0
        return
    assert n >= 1 and calls >= 2 * n, (group, n, calls)
    print("K6 %s: %d host cases, %d calls" % (group, n, calls))


def test_one_k6_shape_with_two_operand_sets_and_no_k9_case_is_left_to_the_device():
    """the host model runs everything but the 0.8 GB shape.  That shape has two operand sets, because the non-temporal loads it is there
    for switch on at one threshold for full columns and at another for the staircase: both must be reached, at one (rows, k)"""
    left = [c for c in oc.K6.cases() if not c.host]
    assert [c.group for c in left] == ["big", "big"] and {c.cid for c in left} == {"null_G2", "stair_P2"}
    assert {(c.args["rows"], c.args["k"]) for c in left} == {(oc.BIG_ROWS, oc.BIG_K)}
    assert all(c.host for c in oc.K9.cases())
    assert oc.BIG_ROWS == 383 * 1024 + 1 and oc.dots_grid_y(oc.BIG_ROWS, oc.BIG_K) == 16


def test_k6_one_enqueued_pass_reports_that_another_is_wanted():
    """NEP_ORTH_DEV_PASSES=1 as the model sees it: the two-pass cases stop after one pass with `another_pass_wanted` set"""
    n = 0
    for c in oc.K6.cases():
        if c.host and c.group in ("rows257", "breakdown", "rounded") and ("P2" in c.cid or "G2" in c.cid or "BRK" in c.cid or c.extra.get("nearspan")):
            n += oc.K6.check(partial(oc.K6.ref, max_passes=1), c, only=(oc.DEV, oc.MIRROR, oc.NEXT), max_passes=1)
    assert n >= 10, n


def _rejecting_case(prim, mut, cases):
    impl = partial(prim.ref, mut=mut)
    for c in cases:
        if not c.host or (mut in prim.exact_only_mutants and c.kind != "exact"):
            continue
        try:
            prim.check(impl, c)
        except AssertionError:
            return c
    return None


K6_MUTANT_GROUPS = ("rows1025", "k_edges", "iar_next", "rounded")


def test_every_k6_mutant_is_rejected():
    ratios, counts = dict(pc.RATIOS), dict(oc.COUNTS)
    cases = [c for c in oc.K6.cases() if c.group in K6_MUTANT_GROUPS and (c.group != "rounded" or c.cid.startswith(("1025x9", "2800x13")))]
    rejected = {}
    for mut in oc.K6.mutants:
        c = _rejecting_case(oc.K6, mut, cases)
        assert c is not None, "K6: no case rejects the mutant %r" % mut
        rejected[mut] = repr(c)
    pc.RATIOS.clear(); pc.RATIOS.update(ratios); oc.COUNTS.clear(); oc.COUNTS.update(counts)
    print("K6: %d mutants rejected: %s" % (len(rejected), rejected))
    assert len(rejected) >= 6


def test_k6_rounded_checks_reject_mutants_on_their_own():
    """the bounds of the rounded tier are tight enough to see a dropped row, a skipped column group, the wrong conjugate and a stale
    beta without the help of an exact case"""
    ratios, counts = dict(pc.RATIOS), dict(oc.COUNTS)
    cases = [c for c in oc.K6.cases() if c.group == "rounded" and c.cid.startswith(("1025x9", "2800x13"))]
    for mut in ("drop_last", "skip_group", "conj_wrong", "beta_stale", "h_not_accumulated", "wt_cols_swapped"):
        assert _rejecting_case(oc.K6, mut, cases) is not None, mut
    pc.RATIOS.clear(); pc.RATIOS.update(ratios); oc.COUNTS.clear(); oc.COUNTS.update(counts)


def test_k6_argument_contract_of_the_model():
    c = next(c for c in oc.K6.cases() if c.group == "iar_next")
    a = c.args
    kw = oc.K6.buffers(a, oc.NEXT, 0, 3)
    for bad in (dict(rows=0), dict(k=0), dict(ldv=a["rows"] - 1), dict(V=None), dict(w=None), dict(out=None), dict(method=2), dict(method=-1),
                dict(mt=0), dict(mt=5), dict(ldc=a["k"]), dict(C=None), dict(WT=None), dict(shift=None)):
        res = oc.K6.ref(**dict(kw, **bad))
        assert res["status"] == oc.NEP_ERR_ARG, bad
        for key in ("w", "out", "mirror", "WT", "shift"):
            assert res[key] is None or np.array_equal(res[key], kw[key]), (bad, key)
    assert oc.K6.ref(**dict(oc.K6.buffers(a, oc.ORTH, 3)))["status"] == oc.NEP_ERR_ARG


def test_k9_numpy_implementation_passes_every_case():
    n = 0
    for c in oc.K9.cases():
        oc.K9.check(oc.K9.ref, c)
        n += 1
    assert n >= 100, n
    print("K9: %d host cases, largest |impl - ref| / bound = %.3g" % (n, pc.RATIOS.get(oc.K9.name, 0.0)))


def test_every_k9_mutant_is_rejected():
    ratios, counts = dict(pc.RATIOS), dict(oc.COUNTS)
    cases = [c for c in oc.K9.cases() if c.group in ("rows17", "rows65", "rows4033", "edges")]
    rejected = {}
    for mut in oc.K9.mutants:
        c = _rejecting_case(oc.K9, mut, cases)
        assert c is not None, "K9: no case rejects the mutant %r" % mut
        rejected[mut] = repr(c)
    pc.RATIOS.clear(); pc.RATIOS.update(ratios); oc.COUNTS.clear(); oc.COUNTS.update(counts)
    print("K9: %d mutants rejected: %s" % (len(rejected), rejected))
    assert len(rejected) >= 4


def test_checked_entry_points_have_checkers_with_mutants():
    for name in oc.CHECKED:
        assert len(oc.BY_NAME[name].mutants) >= (6 if name != "nep_gemm_h_rm" else 4), name
    assert set(oc.CHECKED) <= set(pc.TABLE) and all(pc.BY_NAME[name] is oc.BY_NAME[name] for name in oc.CHECKED)


def test_all_eight_finish_vc_instantiations_are_in_the_case_list():
    seen = {(64 if n >= 65536 else 32, mt) for n, k, mt in oc.NEXT_EXACT}
    assert seen == {(r, mt) for r in (32, 64) for mt in (1, 2, 3, 4)}
    assert {n for n, k, mt in oc.NEXT_EXACT} >= {70, 65535, 65536} and any(k + 1 > 128 for n, k, mt in oc.NEXT_EXACT)
