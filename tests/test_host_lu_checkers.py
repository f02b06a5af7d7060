"""The checkers of tests/lu_checkers.py can fail, and their cases are what they are named for: driven on the host with the float64
substitution `ref_impl` (which has to pass every case) and with a fixed list of mutants of it, each of which some case has to
reject; nep_lu_analyze (host-only) confirms level count, largest block and split coupling launches of every family; a float64
block-inverse emulation of the device schedule measures the constant of the rounded bound.  test_gpu_lu_checkers.py runs the
same checkers on the library."""
import ctypes as C
from functools import partial

import numpy as np
import pytest

import lu_checkers as lc
import primitive_checkers as pc

ALL = list(lc.cases())
REFS = {}                                                   # case -> its reference: built once, used by the reference run and by every mutant


def _by_family():
    out = {}
    for c in ALL:
        out.setdefault(c.group, []).append(c)
    return out


@pytest.mark.parametrize("fam", list(lc.FAMILIES))
def test_reference_passes_every_case_and_exact_cases_are_exact(fam):
    """float64 substitution against the clongdouble reference inside the bound (rounded) and bit for bit against the integers the
    right-hand sides were formed from (exact; check() asserts the 2^53 bound of every call first)"""
    n = 0
    kinds = set()
    for c in _by_family()[fam]:
        n += lc.check(lc.ref_impl, c, cache=REFS)
        kinds.add(c.kind)
    assert kinds == {"exact", "rounded"} and n >= 16, (fam, n)
    print("%s: %d calls" % (fam, n))


def _rejecting_case(mut):
    impl = partial(lc.ref_impl, mut=mut)
    order = sorted(ALL, key=lambda c: lc.FAMILIES[c.group][0].args[0] if not c.group.startswith("tree") else 10 ** 6)
    for c in order:
        if mut in lc.EXACT_ONLY_MUTANTS and c.kind != "exact":
            continue
        if mut == "conj_wrong" and not c.cid.split("/")[1].startswith("trans"):
            continue
        try:
            lc.check(impl, c, cache=REFS)
        except AssertionError:
            return c
    return None


@pytest.mark.parametrize("mut", lc.MUTANTS)
def test_every_mutant_is_rejected(mut):
    """a coupling entry dropped in the last row of a chunk, perm_c ignored, leading dimensions taken as n, the row scale on the first
    right-hand side only, the last right-hand side stale when nrhs % 4 != 0, conjugation wrong in the transposed solve, a stored
    unit diagonal of L applied twice, scale ignored when dX aliases dB, one result off by 1e-13 (exact cases)"""
    ratios = dict(pc.RATIOS)
    c = _rejecting_case(mut)
    pc.RATIOS.clear(); pc.RATIOS.update(ratios)
    assert c is not None, "no case rejects the mutant %r" % mut
    print("%s rejected by %r" % (mut, c))


@pytest.mark.parametrize("kind", ["exact", "rounded"])
@pytest.mark.parametrize("mut", [m for m in lc.MUTANTS if m not in lc.EXACT_ONLY_MUTANTS])
def test_structural_mutants_are_rejected_in_both_kinds(mut, kind):
    impl = partial(lc.ref_impl, mut=mut)
    ratios = dict(pc.RATIOS)
    hit = None
    for c in ALL:
        if c.kind != kind or lc.FAMILIES[c.group][0].args[0] > 300 or c.group.startswith("tree"):
            continue
        try:
            lc.check(impl, c, cache=REFS)
        except AssertionError:
            hit = c
            break
    pc.RATIOS.clear(); pc.RATIOS.update(ratios)
    assert hit is not None, (mut, kind)


@pytest.mark.parametrize("fam", list(lc.FAMILIES))
def test_families_have_the_structure_they_are_named_for(fam, monkeypatch):
    """nep_lu_analyze (no device) on every variant of the family: levels, diagonal blocks and largest block equal the NumPy
    restatement of the partition, CSR and CSC (sorted or shuffled, diagonal of L stored or not) agree, and the named property
    holds: the level count, a largest block exactly at the forced block maximum, a level with a separate coupling launch"""
    import nep_amd as na
    lib, hp = na._lib.lib, na._lib.hptr
    gen, bmax, (levels, maxblk), split = lc.FAMILIES[fam]
    if bmax is None:
        monkeypatch.delenv("NEP_ML_BMAX", raising=False)
    else:
        monkeypatch.setenv("NEP_ML_BMAX", str(bmax))
    for k in ("NEP_ML_SPLIT", "NEP_ML_CHUNK"):
        monkeypatch.delenv(k, raising=False)
    seen = None
    for variant in lc.VARIANTS:
        rec = lc.make_recipe(fam, variant, "plain", "exact")
        out = (C.c_int64 * 8)()
        assert lib.nep_lu_analyze(rec.n, rec.csc, hp(rec.Lp), hp(rec.Li), hp(rec.Up), hp(rec.Ui), out) == 0, na._lib.lib.nep_last_error()
        out = list(out)
        if seen is None:
            seen = out
            L, U = rec.matrices(pattern=True)
            _, lvl, bid = lc.reference_partition(rec.n, L, U, bmax or lc.ML_BMAX)
            assert out[0] == lvl.max() + 1 and out[1] == len(np.unique(bid)) and out[2] == np.bincount(bid).max()
            Lc = (L - lc.sp.identity(rec.n)).tocoo()
            assert out[3] == out[5] == int(np.sum(bid[Lc.row] != bid[Lc.col]))          # U has the transposed pattern
        # explicit zeros and the stored diagonal change neither partition nor coupling counts; packed inverse sizes follow the blocks
        assert out == seen, (variant, out, seen)
    if levels is not None:
        assert seen[0] == levels, seen
    assert seen[2] == maxblk and (bmax is None or maxblk == bmax or seen[0] == 1 and maxblk < bmax), seen
    assert (seen[7] >= 1) == split, seen
    print(fam, seen)


def test_block_inverse_emulation_sets_the_constant():
    """r = largest |block-inverse host solve - reference| / cbound(N, W) over every rounded case at block maxima 8 and 256; the
    constant of the bound is the smallest power of two >= 4 r, and the emulation alone stays inside the bound"""
    r, where = 0.0, None
    for c in ALL:
        if c.kind != "rounded":
            continue
        a = c.args
        rec, ops = a["rec"], a["ops"][:3]
        _, parts, pair = lc.ref_impl(rec, ops, dt=lc.CLD, want_parts=True)
        (Lm, lx), (Um, ux) = pair
        N = lc.n_terms(rec)
        for (Y, Z, W, x, addm) in parts:
            _, Wb, _ = lc.magnitudes(rec, pair, Y, Z, W)
            for bmax in (8, 256):
                zh = lc.emulate_block_solve(Lm, lx.astype(lc.C128), Um, ux.astype(lc.C128), W.astype(lc.C128), bmax)
                ratio = float(np.max(np.abs(zh.astype(lc.CLD) - Z).astype(np.float64) / np.maximum(lc.cbound(N, Wb), 1e-300)))
                if ratio > r:
                    r, where = ratio, (repr(c), bmax)
    cmin = 2.0 ** np.ceil(np.log2(4 * r))
    print("block-inverse emulation: r = %.4g at %s -> c = 2^%d; C_BLOCK = 2^%d" % (r, where, int(np.log2(cmin)), int(np.log2(lc.C_BLOCK))))
    # (4 r <= c: the emulation justifies the constant with its factor 4; c < 16 r: the constant is the rule's or one step above it,
    # so that another LAPACK behind np.linalg.inv does not flip the assertion at a power of two)
    assert 4 * r <= lc.C_BLOCK < 16 * r, (r, cmin, lc.C_BLOCK, lc.R_MEASURED)


def test_zz_report_largest_ratios():
    for k in sorted(pc.RATIOS):
        if k.startswith("nep_lu"):
            print("%-28s largest |impl - ref| / bound = %.3g" % (k, pc.RATIOS[k]))
    print("measured r = %.4g, c = 2^%d" % (lc.R_MEASURED, int(np.log2(lc.C_BLOCK))))
