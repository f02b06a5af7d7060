"""The checkers of tests/spmf_checkers.py can fail, and their recipes are what they are named for: driven on the host with the
NumPy implementation `ref_impl` (which has to pass every case) and with a fixed list of mutants of it, each of which some exact
case has to reject; nep_spmf_tiles_analyze (host-only) confirms blocks, stride, patch shape and largest footprint of every recipe
and the no-tiles verdicts; nep_csc_to_csr is checked exactly.  test_gpu_spmf_checkers.py runs the same checkers on the library."""
import numpy as np
import pytest

import primitive_checkers as pc
import spmf_checkers as sc

PASSED, REJECTED = [0], []
HOST_MAX_N = 3000                                           # larger recipes reach the reference on the device run only


def _host_cases(name):
    return [c for c in sc.cases(name) if sc.make_recipe(name, c.kind).n <= HOST_MAX_N or c.extra["op"] in ("k11", "cw") or c.extra.get("k", 0) <= 9]


@pytest.mark.parametrize("name", list(sc.RECIPES))
def test_reference_passes_every_case_and_exact_cases_are_exact(name):
    """float64 NumPy implementation against the clongdouble reference inside the bounds (rounded) and bit for bit against itself on
    integers (exact: check() asserts the 2^53 bound of every call first)"""
    n = 0
    for c in _host_cases(name):
        n += sc.check(sc.ref_impl, c)
    assert n >= 8, (name, n)
    PASSED[0] += n
    print("%s: %d calls passed" % (name, n))


ORDER = sorted(sc.RECIPES, key=lambda nm: (sc.RECIPES[nm].gen(0, sc.RECIPES[nm].mt, 0, "exact", **sc.RECIPES[nm].kw)[0], nm))


def _rejecting_case(op, mut):
    impl = lambda o, rec, a: sc.ref_impl(o, rec, a, mut)
    for name in ORDER:
        rec = sc.make_recipe(name, "exact")
        if rec.n > HOST_MAX_N:
            break
        for c in sc.cases(name):
            if c.kind != "exact" or c.extra["op"] != op:
                continue
            try:
                sc.check(impl, c)
            except AssertionError:
                return c
    return None


@pytest.mark.parametrize("op,mut", [(op, m) for op in sc.OPS for m in sc.MUTANTS[op]])
def test_every_mutant_is_rejected_by_an_exact_case(op, mut):
    """a row entry dropped, the last row dropped, terms >= 4 ignored, an entry moved to the neighbouring term, duplicates merged by
    overwriting, conj(C), V or Q read with the wrong leading dimension, a column of the ldq padding read, no j0 offset on F or on
    the tail in the second panel, the norm over all rows, the tail from row0 + 1, ||q||^2 over [0, row0), the last k mod 4 / k mod 8
    columns skipped, Hankel index i + j, tau read with ldt = ma + mb, the sign of K11 dropped, omega without |b_i|, one result
    off by 1e-13"""
    ratios = dict(pc.RATIOS); counts = {k: list(v) for k, v in sc.COUNTS.items()}
    c = _rejecting_case(op, mut)
    pc.RATIOS.clear(); pc.RATIOS.update(ratios); sc.COUNTS.clear(); sc.COUNTS.update(counts)
    assert c is not None, "no exact case rejects the mutant %r of %s" % (mut, op)
    REJECTED.append((op, mut))
    print("%s/%s rejected by %r" % (op, mut, c))


@pytest.mark.parametrize("name", list(sc.RECIPES))
def test_recipes_have_the_tiles_they_are_named_for(name, monkeypatch):
    """nep_spmf_tiles_analyze (no device): blocks, grid stride, patch shape and largest footprint equal the case table, the walk
    through the tiles agrees with the direct evaluation inside cbound of the dry run's own sum (its deterministic V and C are
    restated here), and the no-tiles verdicts hold (n < 64, mt > 8, a row wider than the footprint budget)"""
    import nep_amd as na
    lib = na._lib.lib
    spec = sc.RECIPES[name]
    for k in ("NEP_K1_TILE_XP", "NEP_K1_TILE_ZP", "NEP_K1_TILE_LDS_KB", "NEP_K1_TILE_STRIDE", "NEP_TILE_SLOTTED"):
        monkeypatch.delenv(k, raising=False)
    for k, v in spec.env.items():
        monkeypatch.setenv(k, v)
    for kind in ("exact", "rounded") if spec.rounded else ("exact",):
        rec = sc.make_recipe(name, kind)
        info, err = sc.tiles_analyze(lib, rec, 3)
        got = None if info[0] == 0 else (info[0], info[2], info[3], info[4], info[1])
        assert got == spec.tiles, (name, got, spec.tiles)
        if got is not None:
            r = np.arange(rec.n)[:, None]; j = np.arange(3)[None, :]
            V = (np.sin(0.37 * (r % 1009) + 1.3 * j) + 0.1) + 1j * np.cos(0.11 * (r % 2003) - 0.7 * j)           # the dry run's own operands
            Cm = np.array([[1.0 / (1.0 + jj + 2 * t) + 0.25j * (t - jj % 3) for t in range(rec.mt)] for jj in range(3)])
            W = V @ Cm
            z = sc.spmm(rec, [W[:, t: t + 1] for t in range(rec.mt)])[:, 0]
            S = sc.spmm(rec, [np.abs(W[:, t: t + 1]) for t in range(rec.mt)], absval=True)[:, 0]
            zmax = max(np.abs(z.real).max(), np.abs(z.imag).max())
            # two summation orders of the same L_i products: each within cbound(L_i, S_i) of the exact sum
            assert err * zmax <= 2 * float(np.max(sc.cbound_n(np.maximum(rec.L, 1), S))) * (1 + 1e-9), (err, zmax)
        else:
            assert err == 0.0
    if rec.n < 64 or rec.mt > 8:
        assert spec.tiles is None
    print(name, spec.tiles)


def test_named_tile_facts():
    """the facts the recipes were chosen for"""
    T = {k: v.tiles for k, v in sc.RECIPES.items()}
    assert T["grid5/61x37"] == (48, 37, 4, 16, 104) and T["grid5/61x37+5"][0] == 49 and T["grid5/7x11"][:4] == (2, 11, 4, 11)
    assert T["grid5/251x131"] == (69, 131, 11, 64, 854) and sc.make_recipe("grid5/251x131", "exact").n == 32881
    assert T["grid5/520x64"][2:4] == (11, 64) and T["grid5/520x64_xp8"][2:4] == (8, 64) and T["grid5/520x64_xp13"][2:4] == (13, 64)
    assert T["grid5/520x64_xp13"][4] <= 1024                  # the row-major super-panel form stays allowed
    for mt in (1, 2, 4, 5, 8):
        assert T["grid5/mt%d" % mt][0] == 48
    assert T["grid5/mt9"] is None
    assert T["band/n40000"] == (79, 0, 8, 64, 514)
    assert T["arrow/mt1"][4] == 2000 and T["arrow/mt4"] is None
    assert T["wide/n2257_mt4"][4] <= 1024 < T["wide/n2257"][4]          # four terms: blocks split at the footprint budget
    assert T["degenerate/n63"] is None and T["degenerate/n64"][0] == 1 and T["degenerate/n65"][0] == 2
    dup = sc.make_recipe("degenerate/dups", "exact")
    rows, cols, _ = dup.coo(0)
    key = rows * dup.n + cols
    assert len(np.unique(key)) < len(key) and np.any(np.diff(cols[rows == 5]) < 0)          # duplicates kept, columns unsorted


def test_csc_to_csr_is_exact():
    import nep_amd as na
    n = 0
    for case in sc.csc_to_csr_cases():
        sc.check_csc_to_csr(na._lib.lib, case)
        n += 1
    assert n == 12
    print("nep_csc_to_csr: %d cases" % n)


def test_zz_report():
    total = sum(len(m) for m in sc.MUTANTS.values())
    print("calls passed by the reference: %d; mutants rejected: %d of %d" % (PASSED[0], len(REJECTED), total))
    for k in sorted(sc.COUNTS):
        print("calls %-44s exact %5d rounded %5d" % (k, sc.COUNTS[k][0], sc.COUNTS[k][1]))
    for k in sorted(pc.RATIOS):
        if "[" in k:
            print("ratio %-52s %.3g" % (k, pc.RATIOS[k]))
