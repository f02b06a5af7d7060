"""The checkers of tests/primitive_checkers.py can fail: driven on the host with the float64 NumPy implementation of every
primitive (which has to pass every exact and every rounded case that fits a few seconds of host time) and with a fixed list of
mutants of it, each of which at least one case has to reject.  test_gpu_primitives.py runs the same checkers on the library."""
from functools import partial

import pytest

import primitive_checkers as pc

ALL = pc.PRIMS + [pc.HESS]


@pytest.mark.parametrize("prim", ALL, ids=lambda p: p.name)
def test_numpy_implementation_passes_every_host_case(prim):
    n = 0
    for c in prim.cases():
        if c.host:
            prim.check(prim.ref, c)
            n += 1
    assert n >= 3, (prim.name, n)
    print("%s: %d host cases, largest |impl - ref| / bound = %.3g" % (prim.name, n, pc.RATIOS.get(prim.name, 0.0)))


def _rejecting_case(prim, mut):
    impl = partial(prim.ref, mut=mut)
    for c in prim.cases():
        if not c.host or (mut in prim.exact_only_mutants and c.kind != "exact"):
            continue
        try:
            prim.check(impl, c)
        except AssertionError:
            return c
    return None


@pytest.mark.parametrize("prim", ALL, ids=lambda p: p.name)
def test_every_mutant_is_rejected(prim):
    """last row dropped, tail behind the last multiple of 16 / 64 / 256 dropped, conjugate on the wrong operand, leading dimension
    replaced by the row count, last column left at its initial value, beta ignored, column gather ignored, padding overwritten,
    one result off by 1e-13 relative (exact cases only), a batch block that reads the first block's size, ...: whatever a
    primitive's list names, one of its cases fails on it -- and no primitive has fewer than three such mutants"""
    ratios = dict(pc.RATIOS)
    rejected = {}
    for mut in prim.mutants:
        c = _rejecting_case(prim, mut)
        assert c is not None, "%s: no case rejects the mutant %r" % (prim.name, mut)
        rejected[mut] = repr(c)
    pc.RATIOS.clear(); pc.RATIOS.update(ratios)                   # (the mutants' ratios are not the implementation's)
    print("%s: %d mutants rejected: %s" % (prim.name, len(rejected), rejected))
    assert len(rejected) >= 3, (prim.name, rejected)


def test_every_entry_point_of_the_table_has_a_checker_with_three_mutants():
    for name in pc.TABLE:
        prim = pc.BY_NAME[name]
        assert len(prim.mutants) >= 3, name
    assert {"last_block_stale", "block_reads_k0"} <= set(pc.HESS.mutants)


def test_bound_helpers():
    import numpy as np
    assert pc.gamma(1) == pc.U / (1 - pc.U)
    assert abs(pc.cbound(1000, 1.0) / (2 * np.sqrt(2) * pc.gamma(1000)) - 1) < 0.01       # c = 2 sqrt(2) up to the six extra roundings
    with pytest.raises(AssertionError):
        pc.assert_below_2_53(np.array([2.0 ** 53]))
    # the case the sizes of the exact reductions rest on: a 3 000 017-term Gaussian-integer dot with entries in [-8, 8] stays below
    # 3 000 017 * 2 * 64 = 3.9e8 in every partial sum of either component
    assert 3000017 * 2 * 64 < 2 ** 53
