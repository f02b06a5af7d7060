"""The checkers of tests/lu_checkers.py can fail, and their cases are what they are named for: driven on the host with the float64
substitution `ref_impl` (which has to pass every case) and with a fixed list of mutants of it, each of which some case has to
reject; nep_lu_analyze (host-only) confirms level count, largest block and split coupling launches of every family; a float64
block-inverse emulation of the device schedule measures the constant of the rounded bound.  The same for the device numeric
factorisation: nep_lu_refac_analyze (host-only) against the NumPy classification of the closed families, `ref_refactor` in step
and panel order, its mutants, the constant of the residual bound.  test_gpu_lu_checkers.py runs the same checkers on the library."""
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


# ---- the device numeric factorisation: closed families, classification, reference and mutants ------------------------------------
CLOSED = list(lc.REFAC_CLOSED)


def _host_refac(mut=None):
    def impl(name, rec, data, P):
        return lc.ref_refactor(rec, data, P=P, mut=mut, plan=lc.classify_products(rec.fam))
    return impl


@pytest.mark.parametrize("fam", CLOSED)
def test_closed_families_are_accepted_and_classified_as_restated(fam, monkeypatch):
    """nep_lu_refac_analyze (no device) accepts the closed pattern, and its counts [products, internal, external, segments, wide,
    wide steps, levels] are those of classify_products; products = sum_k |L(:,k)| |U(k,:)|; closing the pattern again adds nothing"""
    import nep_amd as na
    lib, hp = na._lib.lib, na._lib.hptr
    bmax = lc.REFAC_CLOSED[fam][2]
    if bmax is None:
        monkeypatch.delenv("NEP_ML_BMAX", raising=False)
    else:
        monkeypatch.setenv("NEP_ML_BMAX", str(bmax))
    rec = lc.make_closed_recipe(fam, "exact")
    pl = lc.classify_products(fam)
    out = (C.c_int64 * 8)()
    rc = lib.nep_lu_refac_analyze(rec.n, hp(rec.Lp), hp(rec.Li), hp(rec.Up), hp(rec.Ui), hp(rec.perm_r), hp(rec.perm_c), hp(pl.Ap), hp(pl.Ai), out)
    assert rc == 0, lib.nep_last_error()
    assert list(out)[:7] == pl.counts, (list(out), pl.counts)
    nl = np.diff(rec.Lp) - 1
    nu = np.bincount(rec.Ui, minlength=rec.n) - 1
    assert pl.counts[0] == int(np.sum(nl.astype(np.int64) * nu)) and pl.counts[0] < 10 ** 6
    assert pl.counts[0] == pl.counts[1] + pl.counts[2] + pl.counts[4]
    n, lr, lc_, ur, uc = lc.closed_pattern(fam)
    again = lc.close_pattern(n, lr, lc_, ur, uc)
    assert all(np.array_equal(a, b) for a, b in zip(again, (lr, lc_, ur, uc)))
    print(fam, pl.counts, "lanes per level", pl.lanes)


def test_closed_families_together_reach_every_path():
    """internal and wide products, every lane count of k_lu_ext (mean segment length <= 6, <= 48, above), wide levels whose blocks
    have pivot counts in every residue mod 4 (short last panels for every P), a level above 0 that is not wide, an unsymmetric
    pattern (U != L^T), absent operands (a banded top) and deferred products for every P >= 2"""
    lanes, residues, narrow_upper, internal, wide, unsym, absent = set(), set(), [], 0, 0, [], []
    for fam in CLOSED:
        pl = lc.classify_products(fam)
        internal += pl.counts[1]; wide += pl.counts[4]
        lanes |= {g for g in pl.lanes if g}
        for l in range(pl.nlev):
            if pl.wide[l]:
                residues |= {len(b) % 4 for b in pl.blocks[l]}
            elif l >= 1:
                narrow_upper.append((fam, l, len(pl.blocks[l])))
        if not np.array_equal(np.sort(pl.Lrow * pl.n + pl.Lcol), np.sort(pl.Ucol * pl.n + pl.Urow)):
            unsym.append(fam)
        for P in (2, 3, 4):
            info = pl.panels(P)["info"]
            assert info["records"] > 0 and info["deferred"] > 0, (fam, P, info)
            assert info["launches"] <= info["panel_steps"] + (P - 1) * info["wide_levels"], (fam, P, info)
            if any((pn["lr"][:len(pn["ks"])] < 0).any() or (pn["hdr"][:len(pn["ks"]), :len(pn["ks"])] < 0).any()
                   for l in range(pl.nlev) if pl.wide[l] for pn in pl.panels(P)[l][0]):
                absent.append((fam, P))
    assert internal > 0 and wide > 0
    assert lanes == {1, 4, 16}, lanes
    assert residues == {0, 1, 2, 3}, residues
    assert narrow_upper and all(nb > lc.LU_WIDE_MAXBLK for _, _, nb in narrow_upper), narrow_upper
    assert unsym and {P for _, P in absent} == {2, 3, 4}, (unsym, absent)


@pytest.mark.parametrize("fam", lc.REFAC_NOT_CLOSED)
def test_refused_families_are_not_closed(fam):
    """the patterns test_lu_device_factorisation_refuses_patterns_that_are_not_closed expects NEP_ERR_UNSUPPORTED for do gain
    entries under close_pattern"""
    n, rows, cols = lc.FAMILIES[fam][0](np.random.default_rng(pc._seed("pattern" + fam)))
    o = np.lexsort((rows, cols))
    lr, lc_, ur, uc = lc.close_pattern(n, rows[o], cols[o])
    assert len(lr) > len(rows) and len(ur) > len(rows), (fam, len(rows), len(lr))
    assert not lc.Products(lc.make_recipe(fam, "csc", "plain", "exact")).closed


@pytest.mark.parametrize("fam", CLOSED)
def test_refactor_reference_passes_every_closed_case(fam):
    """float64 ref_refactor, step by step and in panels of 2, 3, 4: the three entry forms return the generated factors bit for bit
    (exact) or inside the residual bound (rounded), with the health words of the header; every breakdown case sets health[0]"""
    m = 0
    for P in lc.LU_WIDE_PS:
        for kind in ("exact", "rounded"):
            m += lc.refac_check(_host_refac(), fam, kind, P)
        m += lc.breakdown_check(_host_refac(), fam, P)
    assert m == 4 * (2 * 7 + 5)


def _refac_rejecting_case(mut):
    order = sorted(CLOSED, key=lambda f: lc.classify_products(f).counts[0])
    for fam in order:
        for P in lc.LU_WIDE_PS:
            for what, fn in (("refac_check", partial(lc.refac_check, _host_refac(mut), fam, "exact", P)),
                             ("breakdown_check", partial(lc.breakdown_check, _host_refac(mut), fam, P))):
                try:
                    fn()
                except AssertionError as e:
                    return "%s exact %s P=%d: %s" % (what, fam, P, str(e)[:160])
    return None


@pytest.mark.parametrize("mut", lc.REFAC_MUTANTS)
def test_every_refactorisation_mutant_is_rejected_by_an_exact_case(mut):
    """a panel's updates into its own later rows and columns never applied; an operand F(i, k_r) taken as 0 when k_r has no product of
    its own for the destination; a short last panel eliminated as a full one; the products of an external segment behind the last
    multiple of the lane count lost; the last column of a wide level left unscaled; matrix b of a batch eliminated with the panel block
    of matrix 0; the coefficients of matrix 0 for every matrix of a terms call; the growth word taken over L; a broken pivot not
    reported; one value off by 1e-13"""
    hit = _refac_rejecting_case(mut)
    assert hit is not None, "no exact case rejects the mutant %r" % mut
    print("%s rejected by %s" % (mut, hit))


def test_refactor_emulation_sets_the_constant():
    """r = largest |A - L^ U^| / cbound(N + 1, |L^||U^|) of the float64 reference in step order and in panel order over every
    rounded case; the constant of the bound is the smallest power of two >= 4 r"""
    r, where = 0.0, None
    for fam in CLOSED:
        pl = lc.classify_products(fam)
        for P in lc.LU_WIDE_PS:
            for name in ("nep_lu_factor_dev", "nep_lu_factor_dev_batch"):
                data, want = lc.refac_forms(fam, "rounded")[name]
                Lx, Ux, _ = _host_refac()(name, want[0][0], data, P)
                for b, (_, Ab) in enumerate(want):
                    ratio = lc.refac_ratio(pl, Ab, np.atleast_2d(Lx)[b], np.atleast_2d(Ux)[b])
                    if ratio > r:
                        r, where = ratio, (fam, P, name, b)
    cmin = 2.0 ** np.ceil(np.log2(4 * r))
    print("refactorisation emulation: r = %.4g at %s -> c = 2^%d; C_REFAC = 2^%d" % (r, where, int(np.log2(cmin)), int(np.log2(lc.C_REFAC))))
    assert 4 * r <= lc.C_REFAC < 16 * r, (r, cmin, lc.C_REFAC, lc.R_REFAC_MEASURED)


def test_zz_report_largest_ratios():
    for k in sorted(pc.RATIOS):
        if k.startswith("nep_lu"):
            print("%-28s largest |impl - ref| / bound = %.3g" % (k, pc.RATIOS[k]))
    print("measured r = %.4g, c = 2^%d" % (lc.R_MEASURED, int(np.log2(lc.C_BLOCK))))
