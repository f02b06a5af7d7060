"""Exact and bounded parity tests of the fixed-shift sparse LU solve (K5: csrc/trsv_ml.hip, csrc/trsv.hip, csrc/lufac.hip) on the
synthetic factors of tests/lu_checkers.py, through the raw C ABI (`nep_amd._lib.lib`).

Every case builds one handle from generated factor arrays (nep_lu_create / nep_lu_create_csc, optionally refactored, row-scaled,
transposed) and runs at least eight solves on it (the solve numbers around the graph capture and the apex switch included):
exact cases (Gaussian-integer factors and solutions) must match the substitution reference bit for bit at every solve, rounded
cases stay inside the componentwise bound of lu_checkers.check.  The device numeric factorisation (csrc/lufac.hip) runs on the
closed fill patterns of lu_checkers.REFAC_CLOSED: factors bit for bit (exact) or inside the componentwise residual bound (rounded),
pivot breakdown, a batch with broken members, the growth limit.  test_host_lu_checkers.py shows that these checkers reject mutants
and that the families have the block structure and the product classes they are named for."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import lu_checkers as lc
import primitive_checkers as pc
from primitive_checkers import C128, SENT, NAN

pytestmark = pytest.mark.gpu
REFS = {}                                                   # case -> its reference (the same case runs under many shapes)
COUNTS = {}                                                 # (entry point / shape) -> [exact calls, rounded calls]


@pytest.fixture(scope="module")
def na():
    import nep_amd
    if nep_amd.device_count() < 1:
        pytest.skip("no GPU")
    return nep_amd


def _L():
    from nep_amd import _lib
    from nep_amd.nep import stream_ptr
    return _lib, _lib.lib, stream_ptr


def _up(buf):
    return torch.from_numpy(np.ascontiguousarray(buf)).to("cuda")


def _p(t):
    return C.c_void_p(t.data_ptr())


def _count(key, kind, k):
    COUNTS.setdefault(key, [0, 0])[0 if kind == "exact" else 1] += k


def create(rec, Lx=None, Ux=None):
    _lib, lib, _ = _L()
    h = C.c_void_p()
    f = lib.nep_lu_create_csc if rec.csc else lib.nep_lu_create
    hp = _lib.hptr
    Lx = np.ascontiguousarray(rec.Lx if Lx is None else Lx); Ux = np.ascontiguousarray(rec.Ux if Ux is None else Ux)
    _lib.check(f(rec.n, hp(rec.Lp), hp(rec.Li), hp(Lx), hp(rec.Up), hp(rec.Ui), hp(Ux), hp(rec.perm_r) if rec.perm_r is not None else None,
                 hp(rec.perm_c) if rec.perm_c is not None else None, C.byref(h)))
    return h


def run_op(h, op):
    """one nep_lu_solve / nep_lu_solve_add call on fresh device copies of the buffers; returns the X buffer"""
    _lib, lib, st = _L()
    Bd = _up(op.B)
    Xd = Bd if op.alias else _up(op.X)
    if op.add is None:
        _lib.check(lib.nep_lu_solve(h, op.nrhs, _p(Bd), op.ldb, _p(Xd), op.ldx, op.scale, st()))
    else:
        Ad = Xd if op.add == "alias" else _up(op.Add) if op.add == "own" else None
        _lib.check(lib.nep_lu_solve_add(h, op.nrhs, _p(Bd), op.ldb, _p(Ad) if Ad is not None else None,
                                        op.ldx if op.add == "alias" else op.ldadd, _p(Xd), op.ldx, op.scale, st()))
    torch.cuda.synchronize()
    return Xd.cpu().numpy()


def device_impl(rec, ops, expect_block=True, sched_check=None):
    """one handle for the recipe: create (with the first values when the recipe refactors), refactor, row scale, transpose; all
    calls on it.  A transposed recipe also solves on the source handle before the transposition and after all transposed
    solves: bitwise the same result"""
    _lib, lib, st = _L()
    first = rec.first
    h = create(rec, *(first if first else (None, None)))
    ht = None
    try:
        blk = C.c_int32(-1)
        _lib.check(lib.nep_lu_is_block_schedule(h, C.byref(blk)))
        assert blk.value == (1 if expect_block else 0), blk.value
        if first:
            # the old values are in use (and, with a graph, captured) before they change -- and solve like any others
            op0 = lc.Op(ops[0].nrhs, ops[0].B, ops[0].ldb, ops[0].X, ops[0].ldx, ops[0].scale, ops[0].add, ops[0].Add, ops[0].ldadd)
            op0.truth = None
            got0 = run_op(h, op0)
            lc.check(lambda r_, o_: [got0], pc.Case(rec.fam, "first values", rec.kind, None), args=dict(rec=lc.first_recipe(rec), ops=[op0]))
            _lib.check(lib.nep_lu_refactor(h, _lib.hptr(np.ascontiguousarray(rec.Lx)), _lib.hptr(np.ascontiguousarray(rec.Ux))))
        if rec.rs is not None:
            rs = np.ascontiguousarray(rec.rs, dtype=np.float64)
            _lib.check(lib.nep_lu_set_row_scale(h, _lib.hptr(rs)))
        hs = h
        if rec.trans is not None:
            probe = lc.Op(ops[0].nrhs, ops[0].B, ops[0].ldb, ops[0].X if not ops[0].alias else ops[0].B, ops[0].ldx, ops[0].scale)
            before = run_op(h, probe)
            ht = C.c_void_p()
            _lib.check(lib.nep_lu_transpose(h, rec.trans, C.byref(ht)))
            hs = ht
        outs = [run_op(hs, op) for op in ops]
        if sched_check is not None:
            sc = (C.c_int64 * 8)()
            _lib.check(lib.nep_lu_schedule(hs, sc))
            sched_check(list(sc))
        # (NEP_ML_APEX_AT=0 moves a handle to its apex at the first solve that finds the build finished: by design the two paths
        # round differently, so only integer results are the same before and after in that mode)
        if rec.trans is not None and not (os.environ.get("NEP_ML_APEX_AT") == "0" and rec.kind == "rounded"):
            after = run_op(h, probe)
            assert np.array_equal(before.view(np.float64), after.view(np.float64), equal_nan=True), "the source handle changed"
        return outs
    finally:
        if ht is not None:
            lib.nep_lu_destroy(ht)
        lib.nep_lu_destroy(h)


def run_family(fam, key=None, only=None, impl=device_impl, kinds=("exact", "rounded")):
    n = 0
    for c in lc.cases():
        if c.group != fam or c.kind not in kinds or (only is not None and c.cid not in only):
            continue
        k = lc.check(impl, c, cache=REFS if c.group in SHAPE_FAMS else None)
        _count(key or ("create%s/%s" % ("_csc" if c.cid.startswith("csc") else "", c.cid.split("/")[1])), c.kind, k)
        n += k
    return n


@pytest.mark.parametrize("fam", list(lc.FAMILIES))
def test_lu_family_default_schedule(na, fam, monkeypatch):
    """every case of the family (CSR and CSC input, shuffled columns, L with and without its diagonal, NULL and random permutations;
    plain, refactored, row-scaled and transposed handles; nrhs 1 .. 33 with ragged groups, leading dimensions above n, aliased
    buffers, three scales, solve_add) under the default schedule"""
    for k in ("NEP_ML_BMAX", "NEP_ML_SPLIT", "NEP_ML_CHUNK", "NEP_ML_BLK_RHS", "NEP_ML_BLK_RHS_MIN", "NEP_ML_APEX", "NEP_NO_GRAPH", "NEP_ML_FUSE",
              "NEP_LU_SCHED"):
        monkeypatch.delenv(k, raising=False)
    n = run_family(fam)
    assert n >= 16, (fam, n)


SHAPES = [dict(NEP_ML_BMAX="8"), dict(NEP_ML_BMAX="32"), dict(NEP_ML_BMAX="96"),
          dict(NEP_ML_SPLIT="1"), dict(NEP_ML_SPLIT="0", NEP_ML_CHUNK="4"), dict(NEP_ML_CHUNK="16", NEP_ML_BMAX="32"), dict(NEP_ML_CHUNK="32"),
          dict(NEP_ML_BLK_RHS="0", NEP_ML_BLK_RHS_MIN="0"), dict(NEP_ML_BLK_RHS="4", NEP_ML_BLK_RHS_MIN="0", NEP_ML_BMAX="96"),
          dict(NEP_ML_BLK_RHS="8", NEP_ML_BLK_RHS_MIN="0"),
          dict(NEP_ML_APEX="0"), dict(NEP_ML_APEX="1"), dict(NEP_ML_APEX="2", NEP_ML_BMAX="32"),
          dict(NEP_NO_GRAPH="1"), dict(NEP_ML_FUSE="1")]
SHAPE_FAMS = ["chain/n3000", "tree/bin11_p0.6", "tree/20ary3_full", "two_tier/m3000_t32", "arrow/m1500_t64", "dense/n65", "dense/n257"]


_PART = {}


def expected_apex(fam, bmax, la):
    """rows of the dense apex nep_lu_schedule has to report in out[0] for NEP_ML_APEX = la: the rows of the levels >= la of the
    reference partition (every variant, treatment and the transposed pair of a family share its pattern), 0 unless
    0 < la < levels and that size is at most 4096"""
    if (fam, bmax) not in _PART:
        rec = lc.make_recipe(fam, "csc", "plain", "exact")
        _PART[fam, bmax] = lc.reference_partition(rec.n, *rec.matrices(pattern=True), bmax)[1]
    lvl = _PART[fam, bmax]
    T = int(np.sum(lvl >= la))
    return T if 0 < la <= lvl.max() and T <= 4096 else 0


def _shape_id(spec):
    return ",".join("%s=%s" % (k.replace("NEP_", ""), v) for k, v in spec.items())


@pytest.mark.parametrize("spec", SHAPES, ids=_shape_id)
def test_lu_schedule_shapes(na, spec, monkeypatch):
    """the block schedule forced into other shapes (all switches are read per create or per solve, see the getenv sites of
    csrc/trsv_ml.hip): block maxima 8 / 32 / 96, coupling always split or always fused, chunk sizes, the block-of-right-hand-sides
    form on every level in both widths and off, the apex from level 1 / 2 and off, no graph, the single-launch form.  Every shape
    runs the csc/plain cases (whole nrhs list) and the handle treatments of each family in both kinds, and nep_lu_schedule has to
    report the shape"""
    for k in ("NEP_ML_BMAX", "NEP_ML_SPLIT", "NEP_ML_CHUNK", "NEP_ML_BLK_RHS", "NEP_ML_BLK_RHS_MIN", "NEP_ML_APEX", "NEP_NO_GRAPH", "NEP_ML_FUSE",
              "NEP_LU_SCHED"):
        monkeypatch.delenv(k, raising=False)
    for k, v in spec.items():
        monkeypatch.setenv(k, v)
    bmax = int(spec.get("NEP_ML_BMAX", lc.ML_BMAX))
    for fam in SHAPE_FAMS:
        seen = []

        def sched_check(sc):
            seen.append(sc)
            assert sc[6] == lc.FAMILIES[fam][0](np.random.default_rng(0))[0] and 1 <= sc[7] <= bmax, sc
            if fam.startswith(("chain", "dense")):
                assert sc[7] == min(bmax, sc[6]) and sc[2] == -(-sc[6] // bmax), sc      # a chain fills every block to the maximum
            if spec.get("NEP_ML_SPLIT") == "0":
                assert sc[4] == 0, sc
            if spec.get("NEP_ML_SPLIT") == "1" and sc[2] > 1:
                assert sc[4] >= 2, sc
            if "NEP_ML_APEX" in spec:
                assert sc[0] == expected_apex(fam, bmax, int(spec["NEP_ML_APEX"])), sc
            if spec.get("NEP_ML_FUSE") == "1":
                assert sc[1] >= 1, sc
        n = run_family(fam, key="shape " + _shape_id(spec), impl=lambda rec, ops: device_impl(rec, ops, sched_check=sched_check))
        assert n >= 16 and seen, (fam, n)


@pytest.mark.parametrize("spec", [dict(), dict(NEP_LU_BLOCK="64", NEP_LU_MID="512", NEP_LU_TAIL="0"),
                                  dict(NEP_LU_BLOCK="128", NEP_LU_MID="384", NEP_LU_TAIL="100"), dict(NEP_LU_MID="0")], ids=_shape_id)
def test_lu_level_schedule(na, spec, monkeypatch):
    """NEP_LU_SCHED=old: the level schedule of csrc/trsv.hip (the fallback of the block schedule) with the mid-region shapes of
    test_lu_blocked_mid_region, on the plain handles (refactor, row scale and transpose need the block schedule: status checked)"""
    _lib, lib, st = _L()
    monkeypatch.setenv("NEP_LU_SCHED", "old")
    for k, v in spec.items():
        monkeypatch.setenv(k, v)
    for fam in ["chain/n1", "chain/n257", "chain/n3000", "tree/bin11_p0.3", "two_tier/m3000_t32", "arrow/m1500_t64", "dense/n65", "dense/n257"]:
        n = lc.FAMILIES[fam][0](np.random.default_rng(0))[0]

        def sched_check(sc):
            if "NEP_LU_BLOCK" in spec and n >= 1100:
                assert sc[7] == int(spec["NEP_LU_BLOCK"]) and sc[6] == int(spec["NEP_LU_MID"]) and sc[0] == int(spec["NEP_LU_TAIL"]), sc
            if spec.get("NEP_LU_MID") == "0":
                assert sc[6] == 0, sc
        k = run_family(fam, key="level schedule " + _shape_id(spec), only=("csc/plain",),
                       impl=lambda rec, ops: device_impl(rec, ops, expect_block=False, sched_check=sched_check))
        assert k >= 16, (fam, k)
    rec = lc.make_recipe("chain/n257", "csc", "plain", "exact")
    h = create(rec)
    out = C.c_void_p()
    assert lib.nep_lu_transpose(h, 0, C.byref(out)) == -5 and not out.value
    assert lib.nep_lu_refactor(h, _lib.hptr(rec.Lx), _lib.hptr(rec.Ux)) == -5
    assert lib.nep_lu_set_row_scale(h, _lib.hptr(np.ones(rec.n))) == -5
    lib.nep_lu_destroy(h)


def test_lu_solve_argument_contract(na):
    """nrhs < 1, a leading dimension below n (dB, dX, and dAdd when given) and NULL buffers: NEP_ERR_ARG, nothing written"""
    _lib, lib, st = _L()
    rec = lc.make_recipe("chain/n257", "csc", "plain", "exact")
    n = rec.n
    h = create(rec)
    Bd = _up(np.ones(2 * n, dtype=C128)); Xd = _up(np.full(2 * n, SENT, dtype=C128))
    try:
        assert lib.nep_lu_solve(h, 0, _p(Bd), n, _p(Xd), n, 1.0, st()) == -2
        assert lib.nep_lu_solve(h, -1, _p(Bd), n, _p(Xd), n, 1.0, st()) == -2
        assert lib.nep_lu_solve(h, 2, _p(Bd), n - 1, _p(Xd), n, 1.0, st()) == -2
        assert lib.nep_lu_solve(h, 2, _p(Bd), n, _p(Xd), n - 1, 1.0, st()) == -2
        assert lib.nep_lu_solve(h, 1, None, n, _p(Xd), n, 1.0, st()) == -2
        assert lib.nep_lu_solve(h, 1, _p(Bd), n, None, n, 1.0, st()) == -2
        assert lib.nep_lu_solve_add(h, 2, _p(Bd), n, _p(Bd), n - 1, _p(Xd), n, 1.0, st()) == -2
        assert lib.nep_lu_solve_add(h, 0, _p(Bd), n, None, 0, _p(Xd), n, 1.0, st()) == -2
        assert b"invalid argument" in lib.nep_last_error()
        torch.cuda.synchronize()
        assert np.array_equal(Xd.cpu().numpy(), np.full(2 * n, SENT, dtype=C128))
        assert lib.nep_lu_solve_add(h, 2, _p(Bd), n, None, 0, _p(Xd), n, 1.0, st()) == 0       # ldadd is not looked at without dAdd
    finally:
        lib.nep_lu_destroy(h)


# ---- switches cached in a static on first use: a fresh child process per setting ------------------------------------------------
def run_child(fams):
    """the cases of the families with the apex forced on from level 1 (the parent sets NEP_ML_APEX=1): every handle has to report it"""
    n = 0
    for fam in fams:
        want = expected_apex(fam, lc.ML_BMAX, 1)
        assert want > 0, (fam, want)

        def sched_check(sc):
            assert sc[0] == want, (fam, sc, want)
        n += run_family(fam, impl=lambda rec, ops: device_impl(rec, ops, sched_check=sched_check))
    return n


@pytest.mark.parametrize("spec", [dict(NEP_ML_APEX_DENSE="0", NEP_ML_APEX_AT="2"), dict(NEP_ML_APEX_DENSE="1"), dict(NEP_ML_APEX_SYNC="1", NEP_ML_APEX_DENSE="0"),
                                  dict(NEP_ML_APEX_AT="0")], ids=_shape_id)
def test_lu_apex_build_forms_in_a_child_process(na, spec):
    """NEP_ML_APEX_DENSE / _SYNC / _AT are read once per process (static): the sparse apex build, the dense build finished before the
    first solve, the synchronous build and the switch at the first query that finds the build done, each with the apex forced on"""
    here = os.path.dirname(os.path.abspath(__file__))
    fams = ["tree/bin11_p0.6", "arrow/m1500_t64", "dense/n257"]
    code = ("import sys; sys.path[:0] = [%r, %r]; import test_gpu_lu_checkers as t; n = t.run_child(%r); print('lu cases passed:', n)"
            % (here, os.path.dirname(here), fams))
    env = dict(os.environ, NEP_ML_APEX="1", **spec)
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=600, env=env)
    if out.returncode < 0 or out.returncode in (124, 134, 137, 139):
        pytest.exit("the child process died (%d): nothing more is started on this device\n%s" % (out.returncode, out.stderr[-4000:]), returncode=3)
    assert out.returncode == 0, (out.stdout[-2000:], out.stderr[-4000:])
    assert "lu cases passed:" in out.stdout and int(out.stdout.split("lu cases passed:")[1].split()[0]) >= 3 * 86, out.stdout[-2000:]


# ---- device numeric factorisation (csrc/lufac.hip) ---------------------------------------------------------------------------------
REFAC_FAMS = ["chain/n2", "chain/n257", "chain/n3000", "tree/20ary3_full", "dense/n63", "dense/n65", "dense/n257"]


@pytest.mark.parametrize("P", [1, 4])
@pytest.mark.parametrize("fam", REFAC_FAMS)
def test_lu_device_factorisation_is_exact_on_integers(na, fam, P, monkeypatch):
    """A = L U formed in integer arithmetic on a closed pattern (chains, full-ancestor trees, dense triangles): nep_lu_factor_dev, the
    batch form and the batch-from-terms form return L and U exactly (the pivots are units: a division swaps components and signs),
    report max |L| = 1 and the true growth max |U| / max |A|, and the handles they return solve exactly"""
    _lib, lib, st = _L()
    hp = _lib.hptr
    monkeypatch.setenv("NEP_LU_WIDE_P", str(P))
    rec = lc.make_recipe(fam, "csc", "plain", "exact")
    n = rec.n
    A = lc.matrix_of(rec)
    Ap = np.ascontiguousarray(A.indptr, dtype=np.int32); Ai = np.ascontiguousarray(A.indices, dtype=np.int32)
    Ax = np.ascontiguousarray(A.data, dtype=C128)
    one = lambda z: np.abs(z.real) + np.abs(z.imag)
    growth = one(rec.Ux).max() / one(Ax).max()
    nL, nU = len(rec.Lx), len(rec.Ux)
    ref = create(lc.make_recipe(fam, "csc", "plain", "rounded"))           # any values of the pattern: the plan is symbolic
    plan = C.c_void_p()
    outs_all = []
    try:
        _lib.check(lib.nep_lu_refac_create(ref, n, hp(rec.Lp), hp(rec.Li), hp(rec.Up), hp(rec.Ui), hp(rec.perm_r), hp(rec.perm_c), hp(Ap), hp(Ai),
                                           C.byref(plan)))
        wi = (C.c_int64 * 5)(); _lib.check(lib.nep_lu_refac_wide_info(plan, wi))
        ri = (C.c_int64 * 6)(); _lib.check(lib.nep_lu_refac_info(plan, ri))
        wide_products = ri[1] - ri[2] - ri[3]
        # (panels of P pivots are built from the products of the wide levels: a plan without any -- no wide level, or one whose only
        # pivot step is the last pivot, which updates nothing, as in chain/n257 -- reports the step-by-step form)
        assert wi[0] == (P if wide_products > 0 else 1), (list(wi), list(ri))
        ops = lc.make_ops(rec, "exact", 11, [1, 5, 8, 33, 2, 3, 9, 4])
        case = pc.Case(fam, "csc/plain", "exact", None)

        rec_i = lc.Recipe(n, 1, rec.Lp, rec.Li, rec.Lx, rec.Up, rec.Ui, 1j * rec.Ux, rec.perm_r, rec.perm_c, absinv=rec.absinv)   # i A = L (i U)
        ops_i = lc.make_ops(rec_i, "exact", 12, [2, 7, 9, 1, 32, 3, 5, 8])

        def verify(h, LU, health, key, rec=rec, ops=ops):
            assert health[0] == 0 and health[1] == (1.0 if nL > n else health[1]) and health[2] == growth, (list(health), growth)
            if LU is not None:
                pc.assert_exact(key + " L", case, LU[:nL], rec.Lx)
                pc.assert_exact(key + " U", case, LU[nL:], rec.Ux)
            k = lc.check(lambda r_, o_: [run_op(h, op) for op in o_], case, name=key, args=dict(rec=rec, ops=ops))
            _count(key + " P=%d" % P, "exact", k)
        # one matrix
        LU = np.full(nL + nU, SENT, dtype=C128); health = np.zeros(3); out = C.c_void_p()
        _lib.check(lib.nep_lu_factor_dev(plan, hp(Ax), 10, 1e8, hp(health), hp(LU), C.byref(out), st()))
        outs_all.append(out)
        verify(out, LU, health, "nep_lu_factor_dev")
        # a batch of two: the matrix and its image under multiplication by i (L the same, U times i)
        Axb = np.ascontiguousarray(np.stack([Ax, 1j * Ax]))
        LUb = np.full((2, nL + nU), SENT, dtype=C128); hb = np.zeros((2, 3)); outs = (C.c_void_p * 2)()
        _lib.check(lib.nep_lu_factor_dev_batch(plan, 2, hp(Axb), 10, 1e8, hp(hb), hp(LUb), outs, st()))
        outs_all += [C.c_void_p(outs[0]), C.c_void_p(outs[1])]
        assert outs[0] and outs[1]
        verify(outs[0], LUb[0], hb[0], "nep_lu_factor_dev_batch")
        verify(outs[1], LUb[1], hb[1], "nep_lu_factor_dev_batch", rec=rec_i, ops=ops_i)
        # from terms: A = (1 + i) A1 + 1 A0 with Gaussian-integer A1 on the pattern
        rng = np.random.default_rng(3)
        A1 = pc.gint(rng, len(Ax), -3, 3)
        A0 = Ax - (1 + 1j) * A1
        D = np.ascontiguousarray(np.stack([A0, A1], axis=1))                # nnz(A) x mt, entry-major
        Cf = np.ascontiguousarray(np.array([[1.0, 1 + 1j], [1.0, 1 + 1j]], dtype=C128))
        Dd = _up(D.reshape(-1))
        ht = np.zeros((2, 3)); outs2 = (C.c_void_p * 2)()
        _lib.check(lib.nep_lu_factor_dev_batch_terms(plan, 2, _p(Dd), 2, hp(Cf), 10, 1e8, hp(ht), outs2, st()))
        outs_all += [C.c_void_p(outs2[0]), C.c_void_p(outs2[1])]
        assert outs2[0] and outs2[1]
        verify(outs2[0], None, ht[0], "nep_lu_factor_dev_batch_terms")
        verify(outs2[1], None, ht[1], "nep_lu_factor_dev_batch_terms")
    finally:
        for o in outs_all:
            if o.value:
                lib.nep_lu_destroy(o)
        if plan.value:
            lib.nep_lu_refac_destroy(plan)
        lib.nep_lu_destroy(ref)


@pytest.mark.parametrize("fam", ["arrow/m1500_t64", "two_tier/m3000_t32", "tree/bin11_p0.3"])
def test_lu_device_factorisation_refuses_patterns_that_are_not_closed(na, fam):
    """eliminating a leaf of these patterns fills entries between its ancestors that the factors do not store: NEP_ERR_UNSUPPORTED"""
    _lib, lib, st = _L()
    hp = _lib.hptr
    rec = lc.make_recipe(fam, "csc", "plain", "exact")
    A = lc.matrix_of(rec)
    Ap = np.ascontiguousarray(A.indptr, dtype=np.int32); Ai = np.ascontiguousarray(A.indices, dtype=np.int32)
    ref = create(rec)
    plan = C.c_void_p()
    try:
        rc = lib.nep_lu_refac_create(ref, rec.n, hp(rec.Lp), hp(rec.Li), hp(rec.Up), hp(rec.Ui), hp(rec.perm_r), hp(rec.perm_c), hp(Ap), hp(Ai), C.byref(plan))
        assert rc == -5 and not plan.value, rc
    finally:
        if plan.value:
            lib.nep_lu_refac_destroy(plan)
        lib.nep_lu_destroy(ref)


# ---- the device factorisation on closed fill patterns (lu_checkers.REFAC_CLOSED): wide levels with sparse tops ----------------------
CLOSED = list(lc.REFAC_CLOSED)
SCHED_ENV = ("NEP_ML_BMAX", "NEP_ML_SPLIT", "NEP_ML_CHUNK", "NEP_ML_BLK_RHS", "NEP_ML_BLK_RHS_MIN", "NEP_ML_APEX", "NEP_NO_GRAPH", "NEP_ML_FUSE",
             "NEP_LU_SCHED", "NEP_LU_WIDE_P", "NEP_LU_DEV_MAXPROD")
NSOLVES = 10                                                # expected_solves of every factor call and of the handles they are compared with
_OPS = {}


class RefacPlan:
    """one plan of a closed family for panels of P (NEP_LU_WIDE_P and the family's block maximum are read when the reference handle
    and the plan are created), the three factor calls on it, and the handles they return (destroyed on exit)"""

    def __init__(self, fam, P, monkeypatch):
        for k in SCHED_ENV:
            monkeypatch.delenv(k, raising=False)
        if P is not None:
            monkeypatch.setenv("NEP_LU_WIDE_P", str(P))
        if lc.REFAC_CLOSED[fam][2]:
            monkeypatch.setenv("NEP_ML_BMAX", str(lc.REFAC_CLOSED[fam][2]))
        self.fam, self.P = fam, P
        self.inp = lc.refac_inputs(fam, "exact")
        self.rec, self.pl = self.inp["rec"], self.inp["plan"]
        self.nL, self.nU = len(self.rec.Lx), len(self.rec.Ux)
        self.ref, self.plan, self.handles = None, C.c_void_p(), []

    def __enter__(self):
        _lib, lib, st = _L()
        hp, rec, pl = _lib.hptr, self.rec, self.pl
        _lib.check(lib.nep_lu_set_expected_solves(NSOLVES))
        self.ref = create(lc.make_closed_recipe(self.fam, "rounded"))      # any values of the pattern: the plan is symbolic
        _lib.check(lib.nep_lu_refac_create(self.ref, rec.n, hp(rec.Lp), hp(rec.Li), hp(rec.Up), hp(rec.Ui), hp(rec.perm_r), hp(rec.perm_c),
                                           hp(pl.Ap), hp(pl.Ai), C.byref(self.plan)))
        return self

    def __exit__(self, *exc):
        _lib, lib, st = _L()
        for h in self.handles:
            if h.value:
                lib.nep_lu_destroy(h)
        if self.plan.value:
            lib.nep_lu_refac_destroy(self.plan)
        if self.ref is not None:
            lib.nep_lu_destroy(self.ref)
        lib.nep_lu_set_expected_solves(50)                   # the default of the header
        return False

    def assert_not_vacuous(self):
        """the plan holds the product classes of classify_products and, for P >= 2, its records, deferred products and launches"""
        _lib, lib, st = _L()
        pl, P = self.pl, self.P
        ri = (C.c_int64 * 6)(); _lib.check(lib.nep_lu_refac_info(self.plan, ri))
        wi = (C.c_int64 * 5)(); _lib.check(lib.nep_lu_refac_wide_info(self.plan, wi))
        ri, wi = list(ri), list(wi)
        assert ri[0] == pl.n and ri[1:5] == pl.counts[:4] and ri[1] - ri[2] - ri[3] == pl.counts[4] > 0, (ri, pl.counts)
        assert wi[0] == P and wi[1] == pl.counts[5], (wi, pl.counts)
        if P >= 2:
            info = pl.panels(P)["info"]
            assert wi[3] == info["records"] > 0 and wi[4] == info["deferred"] > 0 and wi[2] == info["launches"], (wi, info)
            assert wi[2] <= info["panel_steps"] + (P - 1) * info["wide_levels"], (wi, info)
        else:
            assert wi[2] == wi[1] and wi[3] == wi[4] == 0, wi

    def factor(self, name, data, limit=1e8, want_rc=0):
        """one call: (Lx, Ux, health, handles), a batch axis first; Lx, Ux None for the terms call"""
        _lib, lib, st = _L()
        hp = _lib.hptr
        nF = self.nL + self.nU
        if name == "nep_lu_factor_dev":
            LU = np.full(nF, SENT, dtype=C128); health = np.full(3, -1.0); out = C.c_void_p()
            rc = lib.nep_lu_factor_dev(self.plan, hp(np.ascontiguousarray(data)), NSOLVES, limit, hp(health), hp(LU), C.byref(out), st())
            outs, LU, health = [out], LU[None, :], health[None, :]
        else:
            B = len(data[1]) if isinstance(data, tuple) else len(data)
            health = np.full((B, 3), -1.0); arr = (C.c_void_p * B)()
            if isinstance(data, tuple):
                D, Cf = data
                Dd = _up(np.ascontiguousarray(D).reshape(-1))                 # nnz(A) x mt, entry-major
                rc = lib.nep_lu_factor_dev_batch_terms(self.plan, B, _p(Dd), D.shape[1], hp(np.ascontiguousarray(Cf)), NSOLVES, limit, hp(health), arr, st())
                LU = None
            else:
                LU = np.full((B, nF), SENT, dtype=C128)
                rc = lib.nep_lu_factor_dev_batch(self.plan, B, hp(np.ascontiguousarray(data)), NSOLVES, limit, hp(health), hp(LU), arr, st())
            outs = [C.c_void_p(arr[b]) for b in range(B)]
        self.handles += outs
        assert rc == want_rc, (name, rc, lib.nep_last_error())
        return (None if LU is None else LU[:, :self.nL]), (None if LU is None else LU[:, self.nL:]), health, outs

    def assert_solves_like_created(self, h, rec, Lx, Ux, kind, key):
        """eight solves on the returned handle and on a handle nep_lu_create_csc builds from the same arrays: the same bits"""
        _lib, lib, st = _L()
        assert h.value, key
        if (self.fam, kind) not in _OPS:
            _OPS[self.fam, kind] = lc.make_ops(lc.refac_inputs(self.fam, kind)["rec"], kind, 11, [1, 5, 8, 33, 2, 3, 9, 4])
        hc = create(rec, Lx, Ux)
        try:
            for k, op in enumerate(_OPS[self.fam, kind]):
                got, want = run_op(h, op), run_op(hc, op)
                assert np.array_equal(got.view(np.float64), want.view(np.float64), equal_nan=True), \
                    "%s %s P=%s: solve %d (nrhs %d) differs from the created handle's in %d values" % (
                        key, self.fam, self.P, k, op.nrhs, int(np.sum(got.view(np.float64) != want.view(np.float64))))
        finally:
            lib.nep_lu_destroy(hc)
        _count("refac %s %s" % (self.fam, key), kind, len(_OPS[self.fam, kind]))


@pytest.mark.parametrize("P", lc.LU_WIDE_PS)
@pytest.mark.parametrize("fam", CLOSED)
def test_lu_device_factorisation_on_closed_fill_patterns(na, fam, P, monkeypatch):
    """closures of an arrow, a two-tier pattern and a random-ancestor tree (symmetric and with U != L^T), banded grids, a tree whose
    level 1 is not wide: nep_lu_factor_dev, the batch of three and the batch from three terms, step by step and in panels of 2, 3, 4.
    Exact values: L, U and the health words bit for bit, the same bits from a second call; rounded values: the componentwise
    residual bound of lu_checkers.refac_check.  Every returned handle solves bit for bit like a handle created from the same
    values, and the plan reports the product classes, records, deferred products and launches of the NumPy restatement"""
    with RefacPlan(fam, P, monkeypatch) as rp:
        rp.assert_not_vacuous()
        for kind in ("exact", "rounded"):
            forms = lc.refac_forms(fam, kind)
            last = {}

            def impl(name, rec, data, P_):
                Lx, Ux, health, outs = rp.factor(name, data)
                want = forms[name][1]
                if Lx is not None:
                    Lx2, Ux2, health2, _ = rp.factor(name, data)
                    assert all(np.array_equal(a.view(np.float64), b.view(np.float64)) for a, b in ((Lx, Lx2), (Ux, Ux2), (health, health2))), \
                        "%s: a second call on the plan returned other bits" % name
                    last["LU"] = (Lx, Ux)
                elif kind == "rounded":
                    # the assembly of these terms is exact: the very matrices of the batch, so the very factors and health words
                    hb = last["health"]
                    assert np.array_equal(health.view(np.int64), hb.view(np.int64)), (name, health, hb)
                for b, (rb, _) in enumerate(want):
                    vals = (Lx[b], Ux[b]) if Lx is not None else (rb.Lx, rb.Ux) if kind == "exact" else (last["LU"][0][b], last["LU"][1][b])
                    rp.assert_solves_like_created(outs[b], rb, vals[0], vals[1], kind, name)
                last["health"] = health
                return Lx, Ux, health
            assert lc.refac_check(impl, fam, kind, P) == 7


BREAK_FAMS = ["arrow/m300_t41/unsym", "tree/bin11_p0.3/bmax8", "grid/24x24"]


@pytest.mark.parametrize("P", lc.LU_WIDE_PS)
@pytest.mark.parametrize("fam", BREAK_FAMS)
def test_lu_device_factorisation_reports_a_broken_pivot_and_keeps_the_rest_of_the_batch(na, fam, P, monkeypatch):
    """exact factors with one U_kk = 0 -- k inside a level-0 block (k_lu_int), the first pivot and a later slot of a panel (k_lu_scale
    after the panel's own elimination), pivot n - 1 -- and a matrix with a NaN entry.  The single call: NEP_ERR_SINGULAR, no handle,
    health[0] = 1.  A batch with the broken matrix in the middle: its handle NULL, the two others exact in values, health and solves
    (the batched schedule build with two accepted members that are not adjacent); a batch with one good member in the middle: that
    one exact (the single-factor build).  A zero pivot is a floating-point division by zero: nothing here faults"""
    with RefacPlan(fam, P, monkeypatch) as rp:
        inp = rp.inp
        rec, rec2, Ax, Ax2 = inp["rec"], inp["rec2"], inp["Ax"], inp["Ax2"]
        case = pc.Case(fam, "P=%d" % P, "exact", None)

        def good(tag, b, Lx, Ux, health, outs, r_, A_):
            pc.assert_exact(tag + " L", case, Lx[b], r_.Lx)
            pc.assert_exact(tag + " U", case, Ux[b], r_.Ux)
            pc.assert_exact(tag + " health", case, health[b], lc.expected_health(r_, A_))
            rp.assert_solves_like_created(outs[b], r_, Lx[b], Ux[b], "exact", "batch with a broken member")
        for label, k, Abad in lc.breakdown_cases(fam, P):
            tag = "%s (pivot %d)" % (label, k)
            _, _, health, outs = rp.factor("nep_lu_factor_dev", Abad, want_rc=-3)          # NEP_ERR_SINGULAR
            assert not outs[0].value and health[0][0] == 1.0, (tag, health)
            Lx, Ux, health, outs = rp.factor("nep_lu_factor_dev_batch", np.stack([Ax, Abad, Ax2]))
            assert not outs[1].value and health[1][0] == 1.0, (tag, health)
            good(tag + " batch[0]", 0, Lx, Ux, health, outs, rec, Ax)
            good(tag + " batch[2]", 2, Lx, Ux, health, outs, rec2, Ax2)
            Lx, Ux, health, outs = rp.factor("nep_lu_factor_dev_batch", np.stack([Abad, Ax2, Abad]))
            assert not outs[0].value and not outs[2].value and health[0][0] == 1.0 and health[2][0] == 1.0, (tag, health)
            good(tag + " the one good member", 1, Lx, Ux, health, outs, rec2, Ax2)


@pytest.mark.parametrize("kind", ["exact", "rounded"])
def test_lu_device_factorisation_growth_limit_between_the_health_words(na, kind, monkeypatch):
    """a factor is refused when max |L| or max |U| / max |A| exceeds the limit: with the limit at the larger of the two words the
    factor is accepted, one unit in the last place below it is refused (NEP_ERR_SINGULAR, no handle, the same health words, no
    broken pivot) -- exact values: max |L| = 1 above the growth; rounded (dominant diagonal): the growth above max |L|"""
    fam = "arrow/m300_t41/unsym"
    with RefacPlan(fam, None, monkeypatch) as rp:
        data, want = lc.refac_forms(fam, kind)["nep_lu_factor_dev"]
        Lx, Ux, health, outs = rp.factor("nep_lu_factor_dev", data)
        h = health[0]
        pc.assert_exact("health", pc.Case(fam, "growth", kind, None), h, lc.expected_health(lc.with_values(want[0][0], Lx[0], Ux[0]), data))
        assert (h[1] > h[2]) == (kind == "exact") and h[1] != h[2], h
        hi = float(max(h[1], h[2]))
        _, _, h2, outs = rp.factor("nep_lu_factor_dev", data, limit=hi)
        assert outs[0].value and np.array_equal(h2[0], h)
        below = float(np.nextafter(hi, 0.0))
        assert below > min(h[1], h[2])
        _, _, h3, outs = rp.factor("nep_lu_factor_dev", data, limit=below, want_rc=-3)
        assert not outs[0].value and np.array_equal(h3[0], h) and h3[0][0] == 0.0, (h3, h)
        _, _, h4, outs = rp.factor("nep_lu_factor_dev_batch", np.stack([data, data]), limit=below)
        assert not outs[0].value and not outs[1].value and np.array_equal(h4[0], h) and np.array_equal(h4[1], h)


def test_zz_report_counts_and_largest_ratios(na):
    """calls checked per entry point / handle treatment / schedule shape (exact, rounded), and the largest |dev - ref| / bound of the
    rounded cases of every family that ran in this process (each was asserted <= 1 where it arose)"""
    for key in sorted(COUNTS):
        print("calls %-70s exact %5d rounded %5d" % (key, COUNTS[key][0], COUNTS[key][1]))
    for name in sorted(pc.RATIOS):
        if name.startswith("nep_lu"):
            print("ratio %-28s %.3g" % (name, pc.RATIOS[name]))
            assert pc.RATIOS[name] <= 1.0
    print("bound constant: measured r = %.4g, c = 2^%d" % (lc.R_MEASURED, int(np.log2(lc.C_BLOCK))))
    print("factorisation residual constant: measured r = %.4g, c = 2^%d" % (lc.R_REFAC_MEASURED, int(np.log2(lc.C_REFAC))))
