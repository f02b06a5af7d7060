"""Host-side tests of K14 (nep_spmf_biforms): the checker that test_gpu_biforms.py runs on the kernel passes a dense evaluation
and rejects two mutants, the argument checks that run before any device work, and the declarations the feature adds."""
import ctypes as C
import os
import re
from functools import partial

import numpy as np
import pytest

import nep_amd as na
import biforms_checkers as bc
import primitive_checkers as pc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL = [c for c in bc.CASES if "band/" not in c.name]           # (a dense 22001 x 22001 matrix is out of reach)


def test_case_list_covers_what_the_kernel_distinguishes():
    names = {c.name for c in bc.CASES}
    assert len(names) == len(bc.CASES)
    for n in (1, 63, 64, 65, 257):
        for mt in (1, 3, 5):
            assert {"degenerate/n%d_mt%d_real" % (n, mt), "degenerate/n%d_mt%d_cplx" % (n, mt)} <= names
    shapes = {s for c in bc.CASES for s in c.shapes}
    assert {(1, 1), (2, 5), (5, 2), (32, 32)} <= shapes
    assert all(c.mt == 3 for c in bc.CASES if (32, 32) in c.shapes)
    for c in bc.CASES:
        assert all(1 <= kw <= bc.MAX_WV and 1 <= kv <= bc.MAX_WV and c.mt * kw * kv <= bc.MAX_OUT for kw, kv in c.shapes), c
    big = next(c for c in bc.CASES if c.name == "band/n22001")
    assert -(-22001 // 64) > (1 << 20) // (3 * 32 * 32)        # more row tiles than workgroups: the grid-stride loop runs twice
    assert any(c.mt > 64 for c in bc.CASES) and any(32 < c.mt <= 64 for c in bc.CASES)
    rec = next(c for c in bc.CASES if c.name == "degenerate/empty_term").recipe()
    assert len(rec.terms[1][1]) == 0
    rec = next(c for c in bc.CASES if c.name == "degenerate/empty_rows").recipe()
    assert np.any(rec.L == 0)
    assert big.recipe().n == 22001


@pytest.mark.parametrize("case", SMALL, ids=repr)
def test_reference_against_a_dense_evaluation(case):
    shapes = [s for s in case.shapes if s != (32, 32) or case.recipe().n <= 300]
    worst = bc.check(case, bc.dense_forms, shapes)
    print("%s: largest |dense - ref| / bound = %.3g" % (case.name, worst))


@pytest.mark.parametrize("mut", ["drop_term", "conj_V"])
def test_checker_rejects_mutant(mut):
    """a term that is left out and a conjugate on the wrong operand: every case with complex operands fails on each"""
    ratios = dict(pc.RATIOS)
    rejected = 0
    cases = [c for c in SMALL if c.recipe().n <= 300][:12]
    for case in cases:
        try:
            bc.check(case, partial(bc.dense_forms, mut=mut), case.shapes[:2])
        except AssertionError:
            rejected += 1
    pc.RATIOS.clear(); pc.RATIOS.update(ratios)
    assert rejected == len(cases), (mut, rejected, len(cases))


def test_reference_mutants_differ_from_the_reference():
    case = next(c for c in bc.CASES if c.name == "degenerate/n65_mt3_cplx")
    rec = case.recipe()
    W, V, ref, S, N = bc.reference(case, rec, 2, 5)
    for mut in ("drop_term", "conj_V"):
        bad = bc.ref_forms(rec, W, V, mut=mut)[0]
        with pytest.raises(AssertionError):
            bc.check_forms(mut, bad.astype(np.complex128), ref, S, N)
    # exact zeros are demanded of a term without entries
    case = next(c for c in bc.CASES if c.name == "degenerate/empty_term")
    rec = case.recipe()
    W, V, ref, S, N = bc.reference(case, rec, 1, 1)
    assert N[1] == 0 and np.all(S[1] == 0)
    got = ref.astype(np.complex128); got[1] += 1e-300
    with pytest.raises(AssertionError, match="exact zeros"):
        bc.check_forms("empty", got, ref, S, N)


def test_argument_checks_before_any_device_work():
    """a NULL handle or block and two NULL outputs are refused before the handle is looked at: NEP_ERR_ARG without a GPU"""
    lib = na._lib.lib
    buf = np.zeros(4, dtype=np.complex128)
    p = buf.ctypes.data_as(C.c_void_p)
    assert lib.nep_spmf_biforms(None, 1, p, 4, 1, p, 4, p, None, None) == na._lib.NEP_ERR_ARG
    assert lib.nep_spmf_biforms(None, 1, None, 4, 1, p, 4, p, None, None) == na._lib.NEP_ERR_ARG
    assert lib.nep_spmf_biforms(None, 1, p, 4, 1, p, 4, None, None, None) == na._lib.NEP_ERR_ARG
    assert b"invalid argument" in lib.nep_last_error()
    assert np.all(buf == 0)


def test_header_build_binding_and_julia_name_the_kernel():
    hdr = open(os.path.join(ROOT, "include", "nepmi355.h")).read()
    assert re.search(r"\bnep_spmf_biforms\s*\(", hdr) and "src/compute_rf_wrapper.jl:115-118" in hdr
    assert na._lib.SIGNATURES["nep_spmf_biforms"] == [C.c_void_p, C.c_int32, C.c_void_p, C.c_int64, C.c_int32, C.c_void_p, C.c_int64,
                                                      C.c_void_p, C.c_void_p, C.c_void_p]
    from nep_amd import build
    assert "biforms.hip" in build.SOURCES
    assert "(:nep_spmf_biforms, LIB)" in open(os.path.join(ROOT, "julia", "NEPMI355X.jl")).read()
    assert hasattr(na.SPMFDevice, "biforms")
