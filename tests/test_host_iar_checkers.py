"""Host-side tests of the checker that test_gpu_iar_checkers.py runs on the device infinite-Arnoldi step chain
(tests/iar_checkers.py): the float64 NumPy model passes every case and stays a factor 4 inside both bounds, every mutant fails on
every case where it applies, the seeded basis keeps its staircase, the case list covers its factors, and a natural run shows why
the cases are seeded."""
from itertools import combinations

import numpy as np
import pytest

import iar_checkers as ic
import primitive_checkers as pc

CASES = ic.covering_cases()
REF_TAG, MUT_TAG = "iar model", "iar mutant"


def test_case_list_is_a_covering_design():
    assert 35 <= len(CASES) <= 60, len(CASES)                            # 35: the pairs of the two largest factors
    assert len({c.key for c in CASES}) == len(CASES)
    for a, b in combinations(range(len(ic.FACTORS)), 2):                 # every pair of values of two different factors
        want = {(va, vb) for va in ic.FACTORS[a] for vb in ic.FACTORS[b]}
        assert want <= {(c.key[a], c.key[b]) for c in CASES}, (ic.FACTOR_NAMES[a], ic.FACTOR_NAMES[b])
    fused = {(c.mt, (c.k0, c.count)) for c in CASES if c.fused}          # the hand-over at every chain, one term and four
    assert fused >= {(mt, ch) for mt in (1, 4) for ch in ic.F_CHAIN}
    assert {(c.mt, (c.k0, c.count)) for c in CASES if c.fuse} >= {(mt, ch) for mt in ic.F_MT for ch in ic.F_CHAIN}
    assert {(c.mt, (c.k0, c.count)) for c in CASES if not c.fuse} >= {(mt, ch) for mt in (1, 4) for ch in ic.F_CHAIN}
    for f, F in enumerate(ic.FACTORS):                                   # no value carries the list: an even spread within a factor 2
        n_ = [sum(c.key[f] == v for c in CASES) for v in F]
        assert max(n_) <= 2 * min(n_), (ic.FACTOR_NAMES[f], n_)
    assert any(c.k0 + c.count - 1 == c.m and c.fused for c in CASES) and any(c.k0 + c.count - 1 == c.m and not c.fused for c in CASES)
    assert [c.key for c in ic.covering_cases()] == [c.key for c in CASES]      # the same list in every process
    assert all(c.refine == 0 for c in CASES if not c.record)


def test_problem_is_what_the_docstring_says():
    for n in ic.F_N:
        for mt in ic.F_MT:
            for values in ic.F_VAL:
                p = ic.problem(n, mt, values)
                assert len(p.A) == mt and all(A.shape == (n, n) for A in p.A)
                assert all(A.dtype == (np.float64 if values == "real" else np.complex128) for A in p.A)
                assert all(A.nnz <= (6 * n if n > 4 else n * n) for A in p.A[1:]) and all(A.nnz >= min(n * n, 2 * n) for A in p.A)
                assert np.all(np.abs(p.A[0].diagonal()) > 3)
                assert p.cf[0] == 1 and np.all(np.abs(p.cf[1:]) * mt >= 0.5) and np.all(np.abs(p.cf[1:]) * mt <= 1.5)
                assert np.array_equal(p.cabs, np.abs(p.cf))
                assert abs(p.M0 - sum(c * A for c, A in zip(p.cf, p.A))).max() < 1e-14
                assert np.linalg.cond(p.M0.toarray()) < 1e3
    T = ic.table(ic.M, 5)
    assert T.shape == (ic.M, 5) and np.all(np.abs(T) > 1e-3) and 0.8 < np.mean(np.abs(T)) < 1.8


def test_seeded_basis_keeps_its_staircase_and_is_orthonormal():
    for c in CASES:
        V = ic.seeded_basis(c.n, c.m, c.k0, c.ldv)
        assert V.shape == (c.m + 1, c.ldv)
        assert ic.staircase_ok(V, c.n, c.k0), c
        G = np.conj(V[:c.k0]) @ V[:c.k0].T
        assert np.linalg.norm(G - np.eye(c.k0), 2) < 1e-14, c
        assert np.abs(V[c.k0 - 1, :c.n * c.k0].reshape(c.k0, c.n)).max(axis=1).min() > 1e-3 / np.sqrt(c.n * c.k0), c     # every block carries weight
    broken = ic.seeded_basis(65, ic.M, 8, 65 * 25)
    broken[3, 65 * 4] = 1e-300
    assert not ic.staircase_ok(broken, 65, 8)


@pytest.mark.parametrize("case", CASES, ids=[repr(c) for c in CASES])
def test_model_passes(case):
    ic.check_chain(case, ic.ref_out(case), tag=REF_TAG)


def test_model_stays_a_factor_four_inside_the_bounds():
    """a condition on the inputs, not a number fitted to the device: the plain float64 model alone uses at most a quarter of either bound"""
    for c in CASES:
        ic.check_chain(c, ic.ref_out(c), tag=REF_TAG)
    b0, sh, orth = (pc.RATIOS[REF_TAG + " " + w] for w in ("block0", "shift", "orthogonality / 1e-12"))
    print("float64 model over %d chains: block-0 ratio %.3g, shifted-block ratio %.3g, ||V^H V - I|| / 1e-12 = %.3g" % (len(CASES), b0, sh, orth))
    assert b0 <= 0.25 and sh <= 0.25


@pytest.mark.parametrize("mut", ic.MUTANTS)
def test_checker_rejects_mutant_on_every_case_where_it_applies(mut):
    """not applicable: stale_wt on a chain of one step (the list has none)"""
    ratios = dict(pc.RATIOS)
    applied, passed = 0, []
    try:
        for c in CASES:
            if not ic.mutant_applies(mut, c):
                continue
            applied += 1
            try:
                with np.errstate(all="ignore"):
                    ic.check_chain(c, ic.ref_out(c, mut=mut), tag=MUT_TAG)
                passed.append(c)
            except AssertionError:
                pass
        worst = {k: v for k, v in pc.RATIOS.items() if k.startswith(MUT_TAG)}
    finally:
        pc.RATIOS.clear(); pc.RATIOS.update(ratios)
    print("%s: rejected on %d of %d chains; largest ratios seen %r" % (mut, applied - len(passed), applied, worst))
    assert applied == len(CASES)
    assert not passed, "the mutant %r passes %r" % (mut, passed)


def test_mutant_applicability():
    one = ic.ChainCase(65, 4, "complex", (1, 1), 0, (0, True), 0, True)
    assert not ic.mutant_applies("stale_wt", one)
    assert all(ic.mutant_applies(m, one) for m in ic.MUTANTS if m != "stale_wt")
    ic.check_chain(one, ic.ref_out(one), tag=REF_TAG)
    a, b = ic.ref_out(one, mut="stale_wt"), ic.ref_out(one)              # there it IS the model
    assert all(np.array_equal(a[k], b[k]) for k in ("V", "dH", "pin"))
    for mut in ic.MUTANTS:
        if mut != "stale_wt":
            with pytest.raises(AssertionError), np.errstate(all="ignore"):
                ic.check_chain(one, ic.ref_out(one, mut=mut), tag=MUT_TAG)
    for k in list(pc.RATIOS):
        if k.startswith(MUT_TAG):
            del pc.RATIOS[k]


def test_structural_violations_are_rejected():
    """one defect each on the model's buffers: a touched seeded column, a write into the padding, a write beyond column k + 1, a
    missing / spurious side effect in column k + 1, a row behind the record, a row of a step never issued, each omega rule, the
    sentinels, a pinned row that arrived late"""
    c = ic.ChainCase(65, 4, "complex", (9, 2), 0, (1, True), 5, True)
    u = ic.ChainCase(65, 5, "real", (2, 2), 1, (0, True), 5, True)
    s = ic.ChainCase(65, 4, "complex", (8, 2), 0, (2 | ic.SKIP_FINAL, True), 5, True)
    nr = ic.ChainCase(65, 1, "real", (2, 2), 0, (0, False), 0, True)
    k, n = c.k0, c.n

    def om(o, cc, kk, slot, v):
        o["dH"][kk - 1, kk + 2:kk + 4].view(np.float64)[slot] = v
        o["pin"][kk - 1] = o["dH"][kk - 1]; o["waited"][kk] = o["dH"][kk - 1].copy()

    defects = [
        (c, lambda o: o["V"].__setitem__((0, 0), o["V"][0, 0] * (1 + 2e-16))),
        (c, lambda o: o["V"].__setitem__((k, c.ldv - 1), 1e-300)),
        (c, lambda o: o["V"].__setitem__((k, n * (k + 1)), 1e-300)),
        (c, lambda o: o["V"].__setitem__((c.k0 + c.count + 1, 0), 1e-300)),
        (c, lambda o: o["V"].__setitem__((c.k0 + c.count, 0), 1e-300)),
        (c, lambda o: o["V"][c.k0 + c.count].__setitem__(slice(None), 0)),
        (c, lambda o: o["V"][c.k0 + c.count].__imul__(1 + 1e-13)),
        (u, lambda o: o["V"].__setitem__((u.k0 + u.count, u.n), 1e-300)),
        (c, lambda o: (o["dH"].__setitem__((k - 1, k + 4), 1e-300), o["pin"].__setitem__((k - 1, k + 4), 1e-300),
                       o["waited"][k].__setitem__(k + 4, 1e-300))),
        (c, lambda o: o["dH"].__setitem__((c.k0 + c.count, 0), 1e-300)),
        (c, lambda o: o["pin"].__setitem__((c.k0 + c.count, 0), 1e-300)),
        (c, lambda o: o["waited"].__setitem__(k, np.zeros_like(o["waited"][k]))),
        (c, lambda o: o["tail"].__setitem__(0, 0)),
        (c, lambda o: om(o, c, k, 2, 1e-17)),
        (c, lambda o: om(o, c, k, 1, 0.0)),
        (c, lambda o: om(o, c, k, 0, 1.0)),
        (s, lambda o: om(o, s, 9, 2, 1e-17)),
        (s, lambda o: om(o, s, 8, 2, 0.0)),
        (nr, lambda o: om(o, nr, nr.k0, 0, 1e-17)),
        (c, lambda o: (o["dH"].__setitem__((k - 1, k + 1), 3.0), o["pin"].__setitem__((k - 1, k + 1), 3.0), o["waited"][k].__setitem__(k + 1, 3.0))),
        (c, lambda o: (o["dH"].__setitem__((k - 1, k + 1), 1 + 1j), o["pin"].__setitem__((k - 1, k + 1), 1 + 1j), o["waited"][k].__setitem__(k + 1, 1 + 1j))),
    ]
    ratios = dict(pc.RATIOS)
    try:
        for i, (cc, hurt) in enumerate(defects):
            o = ic.ref_out(cc)
            ic.check_chain(cc, o, tag=MUT_TAG)
            hurt(o)
            with pytest.raises(AssertionError):
                ic.check_chain(cc, o, tag=MUT_TAG)
                print("defect %d passes on %r" % (i, cc))
    finally:
        pc.RATIOS.clear(); pc.RATIOS.update(ratios)


def test_natural_run_passes_and_its_late_blocks_are_tiny():
    """20 steps from one start vector on n = 65 with the table of f_t(lam) = cf_t exp(-tau_t lam) at 0 (what derivative_table
    delivers; delays of 8 .. 16, so that M0^-1 M'(0) is of order one as in a run with eigenvalues near the shift): the chain passes
    the check, and block k of column k has decayed like 1 / k! -- whatever a step does to the late blocks of such a run is
    invisible in H.  This is why the cases of the list are seeded."""
    c = ic.ChainCase(65, 4, "complex", (1, 20), 0, (1, True), 0, True)
    p = ic.problem(c.n, c.mt, c.values)
    tau = 8.0 + 8.0 * np.random.default_rng(7).random(c.mt)
    inputs = (p, ic.natural_table(c.m, c.mt, p.cf, tau), ic.seeded_basis(c.n, c.m, 1, c.ldv))
    out = ic.ref_steps(*inputs, 1, 20, 0, refine=c.refine, record=True, fused=True)
    ic.check_chain(c, out, tag="iar natural run", inputs=inputs)
    late = [float(np.abs(out["V"][k, c.n * k:c.n * (k + 1)]).max()) for k in range(21)]
    print("max |block k| of column k, k = 0 .. 20: " + " ".join("%.1e" % v for v in late))
    print("max |row j-1| of the table: " + " ".join("%.1e" % v for v in np.abs(inputs[1]).max(axis=1)))
    assert late[20] < 1e-12 and late[10] < 1e-4 and all(late[k + 1] < late[k] for k in range(2, 20))
    seeded = ic.seeded_basis(c.n, c.m, 20, c.ldv)
    assert np.abs(seeded[19, c.n * 19:c.n * 20]).max() > 1e-3
