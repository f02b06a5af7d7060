"""References, error bounds and case lists for K6 (Gram-Schmidt, csrc/orth.hip: nep_orth, nep_orth_dev, nep_orth_dev_mirror,
nep_orth_dev_iar_next) and K9 (nep_gemm_h_rm of csrc/gemm.hip).  Style and helpers of tests/primitive_checkers.py.

`OrthK6.check(impl, case)` runs `impl` once per entry point / method the case names;
    impl(entry, V, ldv, rows, k, active, w, out, method, mirror, nmirror, C, ldc, mt, WT, shift, n) -> dict(status, w, out, mirror,
    WT, shift)
takes flat complex128 buffers in place of device pointers (`active`: int64 array or None) and returns fresh arrays.  For nep_orth
the adapter writes the host results into `out` in the layout of nep_orth_dev: h[0..k), (beta, 0), (passes, 2 breakdown).
test_gpu_orth_checkers.py passes adapters over the library, test_host_orth_checkers.py the float64 NumPy model `ref` and its mutants.

Exact tier (carries the shape sweep).  Column j of V has 4^m non-zeros unit * 2^-m (unit in {1, -1, i, -i}) on a support disjoint
from every other column's, so V^H V = I exactly (columns that find no free row inside their active range are zero columns: h_j = 0).
The supports hold the first and last row, the rows next to every multiple of 64 (hence of 256 and 1024) and the rows next to
every active[j], handed out in turn to the columns that are active there and to z, and are filled up to 4^m with rows spread evenly
over the active range.
  family P   w = V c + z, c dyadic Gaussian integers, z = 4^q unit entries on rows no column touches:
             h == c, beta == 2^q, w_out == z 2^-q bit for bit, after one pass or two.
  family G   w Gaussian integers on every row: h bit-exact (a dyadic sum), w - V h exact, its sum of squares S exact; beta within 2u
             of sqrt(S) (S formed in integers scaled by 4^(2m)); |w_out - w_exact / beta_exact| <= 8u |w_exact| / beta_exact (sqrt
             within one ulp, reciprocal, product, and the 2u of beta).
Every builder asserts that all partial sums of the projection, the update and the final norm stay below 2^53 in units of the smallest
dyadic step (the two norms that only feed the criterion need not be exact), and that the exact criterion ratio
||w_new||^2 / (||c||^2 / 2) lies outside [1/4, 4] at every pass: the pass count does not depend on rounding.

Rounded tier.  V from np.linalg.qr of a random block (full or staircase), E = ||V^H V - I||_2 measured in np.clongdouble.  With
g_d = sqrt(2) gamma_{2 rows + 6} (a projection, primitive_checkers.cbound), g_u = sqrt(2) gamma_{2 k + 6} (an update of k terms),
nV = sqrt(1 + E) >= ||V||_2, nA = sqrt(k) nV >= ||V||_F >= || |V| ||_2, a = ||w_in||_2, pass p of classical Gram-Schmidt computes
    c_p = V^H w_{p-1} + delta_p,   |delta_p| <= cbound(active rows, |V|^H |w_{p-1}|): evaluated entry by entry for p = 1 (w_0 is known);
                                   for p = 2 (w_1 is not) ||delta_2|| <= g_d nA ||w_1||  (Cauchy-Schwarz per column, all rows)
    w_p = w_{p-1} - V c_p + e_p,   |e_p| <= cbound(k, |w_{p-1}| + |V| |c_p|),   ||e_p|| <= g_u (||w_{p-1}|| + nA ||c_p||)
  orthogonality   V^H w_p = -delta_p - (V^H V - I) c_p + V^H e_p, so ||V^H w_p|| <= ||delta_p|| + E ||c_p|| + nV ||e_p||, with
                  ||c_p|| <= nV ||w_{p-1}|| + ||delta_p||.  w_0 = w_in is known; the device's w_1 is not: w_1 = w_1ref - V delta_1 + e_1
                  with w_1ref = (I - V V^H) w_in formed in extended precision, so ||w_1|| <= ||w_1ref|| + nV ||delta_1|| + ||e_1||, and
                  never more than the norm chain of OrthQr, ||w_1|| <= 2.02 a.  q = fl(w_p fl(1 / beta)) adds 2u nV 1.01:
                  ||V^H q|| <= (||delta_p|| + E ||c_p|| + nV ||e_p||) / beta + 2.02 u nV.
  reconstruction  whatever coefficients the projections return, w_in - V h - beta q = -(e_1 + e_2) + V (fl(c_1 + c_2) - c_1 - c_2) +
                  (w_2 - beta q).  With ||c_1|| <= 1.01 a, ||w_1|| <= 2.02 a, ||c_2|| <= 2.03 a, ||w_2|| <= 4.1 a (OrthQr's chain, nA <=
                  1.01 sqrt(k)): ||e_1|| + ||e_2|| <= g_u (3.02 + 3.1 sqrt(k)) a, the other two terms <= 12 u a <= 1.1 g_u a:
                  two passes <= g_u (8 + 7 sqrt(k)) a (OrthQr's constants, k columns); one pass <= g_u (2 + 2 sqrt(k)) a.
  modified GS     (nep_orth, method 2) k updates of one term: ||sum e_i|| <= k sqrt(2) gamma_8 2.1 a; V_j^H w_k = -delta_j -
                  (triu(V^H V - I) h)_j + V_j^H (e_j + .. + e_k): ||V^H w_k|| <= g_d nA 1.02 a + sqrt(k) E ||h|| + sqrt(k) nV ||sum e_i||.
  normalisation   | ||q|| - 1 | <= gamma_{2 rows + 6}  (the sum of squares, its root, the reciprocal and the product).
  pass count      equals the extended-precision reference's; the cases keep its criterion ratio outside [1/2, 2] at every pass.
Nothing is fitted to a device result.  The largest error / bound ratios are recorded in primitive_checkers.RATIOS.

K9: `GemmHRm.check(impl, case)`, impl(WT, ldw, YT, ldy, rows, k, p) -> C (k x p, column-major, flat): C = W^H Y.
"""
from functools import partial

import numpy as np

from primitive_checkers import (C128, CLD, NAN, SENT, SQ2, U, RATIOS, Case, Prim, _seed, gamma, cbound, gint, grand, operand,   # noqa: F401
                                assert_exact, assert_bounded, assert_below_2_53, colmajor_buf, rowmajor_buf, cm_view, rm_view, drop_tail,
                                perturb, groups)

NEP_OK, NEP_ERR_ARG, NEP_ERR_BREAKDOWN = 0, -2, -4
UNITS = np.array([1, -1, 1j, -1j], dtype=C128)
COUNTS = {}                                    # (entry point, tier) -> calls checked

# the launch shapes of csrc/orth.hip the case list is built around
DOT_RB, DOT_CG, DOTS_TARGET, ORTH_NPART, ORTH_DPP_ROWS = 1024, 8, 6144, 1024, 32768


def dots_grid_y(rows, k):
    nchunks, ngroups = -(-rows // DOT_RB), -(-k // DOT_CG)
    return max(1, min(-(-DOTS_TARGET // nchunks), ngroups))


def orth_use_nt(rows, k, staircase):
    return 16.0e-6 * rows * k * (0.5 if staircase else 1.0) > (192.0 if staircase else 512.0)


BIG_K = 130
BIG_ROWS = next(r for r in range(1, 1 << 20, DOT_RB) if dots_grid_y(r, BIG_K) < -(-BIG_K // DOT_CG))   # 392193: 384 row chunks, 16 < 17
assert dots_grid_y(BIG_ROWS - 1, BIG_K) == 17 and orth_use_nt(BIG_ROWS, BIG_K, False) and orth_use_nt(BIG_ROWS, BIG_K, True)
assert not orth_use_nt(70001, 64, False) and -(-70001 // 64) > ORTH_NPART and 70001 >= ORTH_DPP_ROWS

ORTH, DEV, MIRROR, NEXT = "nep_orth", "nep_orth_dev", "nep_orth_dev_mirror", "nep_orth_dev_iar_next"


def _count(entry, kind):
    COUNTS[entry, kind] = COUNTS.get((entry, kind), 0) + 1


def sumsq(x):
    return np.sum(x.real * x.real + x.imag * x.imag)


def act_array(kind, rows, k):
    j = np.arange(k, dtype=np.int64)
    if kind == "null":
        return None
    if kind.startswith("stair"):
        return int(kind[5:]) * (j + 1)
    if kind == "above":                                     # entries above rows are clamped
        return np.where(j % 2 == 0, rows + 1 + 1000 * j, rows).astype(np.int64)
    if kind == "lead0":                                     # a leading run of columns without any active row
        a = np.full(k, rows, dtype=np.int64); a[:(k + 2) // 3] = 0
        return a
    if kind == "nonmono":
        return ((j * 7919 + 13) % rows + 1).astype(np.int64)
    raise ValueError(kind)


def _supports(rows, k, actc, want_z):
    """disjoint row sets: one per column (inside [0, actc[j])) and one for z (anywhere), sizes powers of 4; see the module docstring"""
    mult = np.arange(64, rows, 64, dtype=np.int64)
    E = np.concatenate([np.array([0, rows - 1], dtype=np.int64), mult - 1, mult, mult + 1, actc - 1, actc])
    E = np.unique(E[(E >= 0) & (E < rows)])
    owner = np.full(rows, -1, dtype=np.int32)
    order = np.argsort(actc, kind="stable")
    sorted_act = actc[order]
    first = np.searchsorted(sorted_act, E, side="right")      # the columns order[first:] are active on row E[i]
    lists = [[] for _ in range(k + 1)]
    t = 0
    for r, f in zip(E.tolist(), first.tolist()):
        nopt = k - f + (1 if want_z else 0)
        if nopt == 0:
            continue
        i = t % nopt; t += 1
        o = k if (want_z and i == 0) else int(order[f + i - (1 if want_z else 0)])
        lists[o].append(r); owner[r] = o

    def complete(o, limit):
        have = lists[o]
        free = np.flatnonzero(owner[:limit] == -1)
        total = len(have) + len(free)
        if total == 0:
            return np.zeros(0, dtype=np.int64), 0
        m = 0
        while 4 ** m < len(have):
            m += 1
        while 4 ** m > total:
            m -= 1
        need = 4 ** m
        if len(have) > need:
            owner[np.array(have[need:], dtype=np.int64)] = -1
            have = have[:need]
        fill = free[np.linspace(0, len(free) - 1, need - len(have)).astype(np.int64)] if need > len(have) else np.zeros(0, dtype=np.int64)
        owner[fill] = o
        s = np.sort(np.concatenate([np.array(have, dtype=np.int64), fill]))
        assert len(np.unique(s)) == need
        return s, m

    zs, q = complete(k, rows) if want_z else (np.zeros(0, dtype=np.int64), 0)
    supp, ms = [None] * k, [0] * k
    for j in order.tolist():
        supp[j], ms[j] = complete(j, int(actc[j]))
    return supp, ms, zs, q


class Expect:
    pass


def build_exact(rows, k, actkind, fam, ldv=None, n=0):
    """operands and expected results of one exact case; fam in P1, P2 (a second pass is needed), G1, G2, BRK (w inside span(V))"""
    rng = np.random.default_rng(_seed("k6%d.%d%s%s" % (rows, k, actkind, fam)))
    ldv = rows + 3 if ldv is None else ldv
    active = act_array(actkind, rows, k)
    actc = np.full(k, rows, dtype=np.int64) if active is None else np.minimum(active, rows)
    supp, ms, zs, q = _supports(rows, k, actc, want_z=fam in ("P1", "P2"))
    Vb = np.full(ldv * k, SENT, dtype=C128)
    Vv = []
    for j in range(k):
        Vb[j * ldv: j * ldv + rows] = 0
        Vv.append(rng.choice(UNITS, len(supp[j])) * 2.0 ** -ms[j])
        Vb[j * ldv + supp[j]] = Vv[j]
        assert len(supp[j]) == 0 or (supp[j][-1] < actc[j] and sumsq(Vv[j]) == 1.0)
    nz = np.array([len(s) > 0 for s in supp])
    mmax = max(ms)
    e = Expect()
    w = np.zeros(rows, dtype=C128)
    if fam in ("P1", "P2", "BRK"):
        if fam == "P1":                                      # ||c||^2 <= 128 k 4^cexp < 4^q / 8
            cexp = -int(np.ceil(np.log2(1024.0 * k) / 2)) - 1 + q
        else:                                                # every non-zero |c_j|^2 >= 16 4^q
            cexp = q + 2
        c = gint(rng, k) * 2.0 ** cexp
        if fam != "P1":
            c[c == 0] = (3 - 2j) * 2.0 ** cexp
        for j in range(k):
            w[supp[j]] = Vv[j] * c[j]
        z = rng.choice(UNITS, len(zs))
        w[zs] = z
        wstep = min(1.0, 2.0 ** (cexp - mmax))
        e.h = np.where(nz, c, 0)
        w_new = np.zeros(rows, dtype=C128); w_new[zs] = z
        S = float(len(zs))
        e.beta, e.beta_exact = (2.0 ** q if len(zs) else 0.0), True
        e.w, e.w_exact = w_new * (2.0 ** -q if len(zs) else 0.0), True
        norm_units = S
    else:
        if fam == "G1":
            w = gint(rng, rows)
        else:                                                # V (2^m C) + e: Gaussian integers, nearly inside span(V)
            t = int(np.ceil(np.log2(64.0 * rows) / 2))
            w = gint(rng, rows, -1, 1)
            for j in range(k):
                Cj = gint(rng, 1)[0]
                Cj = (3 - 2j) if Cj == 0 else Cj
                w[supp[j]] += Vv[j] * (2.0 ** ms[j]) * (Cj * 2.0 ** t)
        wstep = 1.0
        e.h = np.array([np.sum(np.conj(Vv[j]) * w[supp[j]]) for j in range(k)], dtype=C128).reshape(k)
        w_new = w.copy()
        for j in range(k):
            w_new[supp[j]] -= Vv[j] * e.h[j]
        wi = w_new * 4.0 ** mmax
        assert np.array_equal(wi, np.round(wi.real) + 1j * np.round(wi.imag)) and float(np.abs(wi).max(initial=0)) ** 2 * rows < 2.0 ** 62
        S_int = int(np.sum(wi.real.astype(np.int64) ** 2)) + int(np.sum(wi.imag.astype(np.int64) ** 2))
        norm_units = float(S_int)
        S = S_int / 16.0 ** mmax
        beta_l = np.sqrt(np.longdouble(S_int)) / np.longdouble(4.0 ** mmax)
        e.beta, e.beta_exact = beta_l, False
        e.w, e.w_exact = (w_new.astype(CLD) / beta_l if S_int else w_new.astype(CLD)), S_int == 0
        if S_int == 0:
            e.beta, e.beta_exact = 0.0, True
    # exactness: every partial sum of the projection, of the update and of the final norm, in units of the smallest dyadic step
    for j in range(k):
        if len(supp[j]):
            vstep = 2.0 ** -ms[j]
            Sj = float(np.sum(np.abs(Vv[j]) * np.abs(w[supp[j]])))
            assert_below_2_53(2 * Sj / (vstep * wstep))
            assert_below_2_53(2 * (np.abs(w[supp[j]]).max() + vstep * abs(e.h[j])) / (vstep * vstep * wstep))
    assert_below_2_53(norm_units)
    # criterion margin: pass 1 exactly; a second pass projects an exact zero (h2 == 0: ratio infinite)
    c2 = float(sumsq(e.h))
    ratio = S / (c2 / 2) if c2 > 0 else np.inf
    assert not (0.25 <= ratio <= 4.0), "criterion ratio %.3g of %s is inside the margin" % (ratio, fam)
    e.needs2 = bool(ratio < 0.25)
    e.brk = S == 0
    e.ratio = ratio
    # (on fewer than 4 rows a family may degenerate: no column finds a row, or w has no component outside span(V))
    assert e.needs2 == (fam in ("P2", "G2", "BRK")) or not nz.any() or rows < 4, (fam, ratio)
    assert e.brk == (fam == "BRK") or rows < 4, (fam, S)
    a = dict(V=Vb, ldv=ldv, rows=rows, k=k, active=active, w=np.concatenate([w, [SENT, SENT]]), expect=e)
    if n:                                                    # nep_orth_dev_iar_next: coefficient table with Gaussian integers
        assert rows == n * (k + 1)
        a.update(n=n, ldc=k + 4, C=colmajor_buf(gint(rng, (k + 1, 4)), k + 4))
        y = np.abs(np.asarray(e.w, dtype=C128)).reshape(k + 1, n).T
        assert_below_2_53(2 * float((y @ np.abs(np.array(cm_view(a["C"], 0, k + 1, 4, k + 4)))).max(initial=0)) * 2.0 ** q)
    return a


_BASIS = {}


def _rounded_basis(rows, k, stair):
    key = (rows, k, stair)
    if key not in _BASIS:
        rng = np.random.default_rng(_seed("k6basis%d.%d.%d" % key))
        A = grand(rng, (rows, k))
        if stair:
            for j in range(k):
                A[stair * (j + 1):, j] = 0
        Q, _ = np.linalg.qr(A)
        if stair:                                            # QR keeps the staircase profile
            for j in range(k):
                assert np.all(Q[stair * (j + 1):, j] == 0)
        Ql = Q.astype(CLD)
        G = (np.conj(Ql.T) @ Ql - np.eye(k)).astype(C128)
        E = float(np.linalg.norm(G, 2)) * (1 + 1e-8)
        assert E < 1e-12
        _BASIS.clear()                                       # (one basis at a time: the cases of a shape follow each other)
        _BASIS[key] = (np.asfortranarray(Q), Ql, E)
    return _BASIS[key]


def build_rounded(rows, k, stair, variant, n=0):
    Q, Ql, E = _rounded_basis(rows, k, stair)
    rng = np.random.default_rng(_seed("k6w%d.%d.%d%s" % (rows, k, stair, variant)))
    if variant == "random":
        w = grand(rng, rows)
    else:                                                    # V c + 1e-9 noise: a second pass is needed
        w = Q @ grand(rng, k) + 1e-9 * grand(rng, rows)
    # extended-precision reference: pass count and the norm of the intermediate vector
    e = Expect()
    wl = w.astype(CLD)
    c1 = np.conj(Ql.T) @ wl
    w1 = wl - Ql @ c1
    r1 = float(sumsq(w1) / (sumsq(c1) / 2))
    assert not (0.5 <= r1 <= 2.0), r1
    e.needs2 = r1 < 1.0
    e.c1, e.w1norm = c1, float(np.sqrt(sumsq(w1)))
    if e.needs2:
        c2 = np.conj(Ql.T) @ w1
        w2 = w1 - Ql @ c2
        r2 = float(sumsq(w2) / (sumsq(c2) / 2))
        assert r2 > 2.0, r2
    e.E, e.Ql, e.brk = E, Ql, False
    ldv = rows + 3
    active = (stair * (np.arange(k) + 1)).astype(np.int64) if stair else None
    a = dict(V=colmajor_buf(Q, ldv, fill=SENT), ldv=ldv, rows=rows, k=k, active=active, w=np.concatenate([w, [SENT, SENT]]), expect=e)
    if n:
        assert rows == n * (k + 1)
        a.update(n=n, ldc=k + 4, C=colmajor_buf(grand(rng, (k + 1, 4)), k + 4))
    return a


SMALL_ROWS = [1, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025]
SMALL_K = [1, 7, 8, 9]
ACTIVE_KINDS = ["null", "stair37", "stair1024", "above", "lead0", "nonmono"]
FAMS = ["P1", "P2", "G1", "G2"]
SMALL_ENTRIES = [(ORTH, 0), (ORTH, 1), (ORTH, 2), (DEV, 0), (DEV, 1), (MIRROR, 0)]
MID_ENTRIES = [(ORTH, 0), (DEV, 0), (DEV, 1)]
ROUNDED = [(1025, 9, 0, 0), (2800, 13, 200, 200), (33001, 17, 0, 0), (40000, 24, 1600, 1600)]     # rows, k, staircase, n of iar_next
# n, k, mt: k_orth_finish_vc<MT, 32> below n = 65536 and <MT, 64> from there on, every MT on both sides; k + 1 = 131 takes the KC loop twice
NEXT_EXACT = [(n, 3, mt) for n in (70, 65535, 65536) for mt in (1, 2, 3, 4)] + [(70, 130, 3), (70, 130, 4)]


class OrthK6(Prim):
    name = "nep_orth"
    mutants = ("drop_last", "drop_tail1024_proj", "skip_group", "conj_wrong", "h_not_accumulated", "no_second_pass", "beta_stale",
               "shift_div_j", "wt_cols_swapped", "perturb")
    # ("active applied per tile in the projection", the update's rule, is no mutant under the contract: V holds zeros below active[j],
    # so the rows it adds contribute exact zeros; include/nepmi355.h states the contract instead)
    exact_only_mutants = ("perturb",)

    def cases(self):
        i = 0
        shapes = [(r, k) for r in SMALL_ROWS for k in SMALL_K] + [(1025, k) for k in (63, 64, 65, 130)]
        for rows, k in shapes:
            for act in ACTIVE_KINDS:
                fam = FAMS[i % 4]; i += 1
                yield Case("rows%d" % rows if k < 10 else "k_edges", "k%d_%s_%s" % (k, act, fam), "exact",
                           partial(build_exact, rows, k, act, fam), extra=dict(entries=SMALL_ENTRIES))
        for rows, k, act in [(257, 8, "null"), (1025, 9, "stair37"), (1025, 65, "nonmono")]:
            yield Case("breakdown", "%dx%d_%s" % (rows, k, act), "exact", partial(build_exact, rows, k, act, "BRK"),
                       extra=dict(entries=SMALL_ENTRIES))
        for rows, acts in [(32767, ["null", "stair1024", "nonmono"]), (32768, ["null", "stair1024", "nonmono"])]:
            for act in acts:
                fam = FAMS[i % 4]; i += 1
                yield Case("dpp_switch", "%dx9_%s_%s" % (rows, act, fam), "exact", partial(build_exact, rows, 9, act, fam),
                           extra=dict(entries=MID_ENTRIES))
        for rows in (65537, 262145):
            for act in ("null", "nonmono"):
                fam = FAMS[i % 4]; i += 1
                yield Case("update_caps", "%dx9_%s_%s" % (rows, act, fam), "exact", partial(build_exact, rows, 9, act, fam),
                           extra=dict(entries=MID_ENTRIES))
        for act in ACTIVE_KINDS:
            fam = FAMS[i % 4]; i += 1
            yield Case("70001x64", "%s_%s" % (act, fam), "exact", partial(build_exact, 70001, 64, act, fam),
                       extra=dict(entries=[(ORTH, 0), (DEV, 0), (MIRROR, 0)]))
        yield Case("70001x64", "null_BRK", "exact", partial(build_exact, 70001, 64, "null", "BRK"), extra=dict(entries=[(ORTH, 0), (DEV, 0)]))
        for n, k, mt in NEXT_EXACT:
            for fam in ("P1", "P2"):
                yield Case("iar_next", "n%d_k%d_mt%d_%s" % (n, k, mt, fam), "exact",
                           partial(build_exact, n * (k + 1), k, "stair%d" % n, fam, n=n), extra=dict(entries=[(DEV, 0), (NEXT, 0, mt)]))
        # the big case: column-group walk (gridDim.y < ceil(k / 8)) and non-temporal loads, full columns and staircase
        yield Case("big", "null_G2", "exact", partial(build_exact, BIG_ROWS, BIG_K, "null", "G2", ldv=BIG_ROWS), host=False,
                   extra=dict(entries=[(DEV, 0), (ORTH, 0)], big=True))
        yield Case("big", "stair_P2", "exact", partial(build_exact, BIG_ROWS, BIG_K, "stair%d" % (BIG_ROWS // (BIG_K + 1)), "P2", ldv=BIG_ROWS),
                   host=False, extra=dict(entries=[(DEV, 0), (ORTH, 0)], big=True))
        for rows, k, stair, n in ROUNDED:
            ents = [(ORTH, 0), (ORTH, 1), (ORTH, 2), (DEV, 0), (DEV, 1)] + ([(NEXT, 0, 1 + (k % 4))] if n else [])
            yield Case("rounded", "%dx%d_s%d_random" % (rows, k, stair), "rounded", partial(build_rounded, rows, k, stair, "random", n=n),
                       extra=dict(entries=ents))
            ents = [(ORTH, 0), (DEV, 0), (MIRROR, 0)] + ([(NEXT, 0, 4 - (k % 4))] if n else [])
            yield Case("rounded", "%dx%d_s%d_nearspan" % (rows, k, stair), "rounded", partial(build_rounded, rows, k, stair, "nearspan", n=n),
                       extra=dict(entries=ents, nearspan=True))

    # ---- float64 NumPy model of the entry points, with mutants ---------------------------------------------------------------------
    def ref(self, entry, V, ldv, rows, k, active, w, out, method, mirror=None, nmirror=0, C=None, ldc=0, mt=0, WT=None, shift=None, n=0,
            mut=None, max_passes=2):
        res = dict(status=NEP_OK, w=None if w is None else w.copy(), out=None if out is None else out.copy(),
                   mirror=None if mirror is None else mirror.copy(), WT=None if WT is None else WT.copy(),
                   shift=None if shift is None else shift.copy())
        bad = V is None or w is None or out is None or rows < 1 or k < 1 or ldv < rows
        bad = bad or method not in ((0, 1, 2) if entry == ORTH else (0, 1))
        if entry == NEXT:
            bad = bad or C is None or WT is None or shift is None or not 1 <= mt <= 4 or ldc < k + 1 or n < 1
        if bad:
            res["status"] = NEP_ERR_ARG
            return res
        Vm = cm_view(V, 0, rows, k, ldv)
        if active is not None:                                 # rows at and beyond active[j] are not part of column j
            Vm = np.where(np.arange(rows)[:, None] < np.minimum(active, rows)[None, :], Vm, 0)
        rp = ru = rows
        if mut == "drop_last":
            rp = ru = rows - 1
        if mut == "drop_tail1024_proj":
            rp = drop_tail(rows, 1024)
        wv = w[:rows].copy()
        h = np.zeros(k, dtype=C128)
        passes, more = 0, 0
        cap = 1 if method else (8 if entry == ORTH else max_passes)
        while True:
            before = np.sqrt(sumsq(wv))
            if method == 2:
                c = np.zeros(k, dtype=C128)
                for j in range(k):
                    c[j] = np.sum(np.conj(Vm[:rp, j]) * wv[:rp])
                    wv[:ru] = wv[:ru] - Vm[:ru, j] * c[j]
            else:
                c = (Vm[:rp].T @ np.conj(wv[:rp])) if mut == "conj_wrong" else (np.conj(Vm[:rp]).T @ wv[:rp])
                if mut == "skip_group":
                    c[8:16] = 0
                wv[:ru] = wv[:ru] - Vm[:ru] @ c
            h = c if mut == "h_not_accumulated" else h + c
            passes += 1
            nrm = before if mut == "beta_stale" else np.sqrt(sumsq(wv))
            again = method == 0 and bool(nrm < np.sqrt(0.5) * np.sqrt(sumsq(c)))
            if mut == "no_second_pass" or not again or passes >= cap:
                more = int(again) if entry != ORTH else 0
                break
        brk = int(not (nrm > 0.0) or not np.isfinite(nrm))
        if mut == "perturb":
            h = perturb(h)
        o = res["out"]
        o[:k] = h; o[k] = nrm; o[k + 1] = complex(passes, 2 * brk + more)
        if brk and entry == ORTH:
            res["status"] = NEP_ERR_BREAKDOWN
        else:
            inv = 0.0 if brk else 1.0 / nrm
            wv = wv.real * inv + 1j * (wv.imag * inv)
        res["w"][:rows] = wv
        if mirror is not None:
            res["mirror"][:nmirror] = o[:nmirror]
        if entry == NEXT:
            y = wv.reshape(k + 1, n)
            with np.errstate(divide="ignore", invalid="ignore"):
                sc = 1.0 / (np.arange(k + 1) + (0.0 if mut == "shift_div_j" else 1.0))
                res["shift"][:rows] = (y.real * sc[:, None] + 1j * (y.imag * sc[:, None])).reshape(-1)
            Cm = cm_view(C, 0, k + 1, mt, ldc)
            P = y.T @ Cm
            res["WT"][:n * mt] = (P[:, ::-1] if mut == "wt_cols_swapped" else P).reshape(-1)
        return res

    # ---- the checks ----------------------------------------------------------------------------------------------------------------
    @staticmethod
    def buffers(a, entry, method, mt=0):
        k, rows = a["k"], a["rows"]
        kw = dict(entry=entry, V=a["V"], ldv=a["ldv"], rows=rows, k=k, active=a["active"], w=a["w"], out=np.full(k + 5, SENT, dtype=C128),
                  method=method)
        if entry in (MIRROR, NEXT):
            kw.update(mirror=np.full(k + 5, SENT, dtype=C128), nmirror=k + 3)
        if entry == NEXT:
            kw.update(C=a["C"], ldc=a["ldc"], mt=mt, WT=np.full(a["n"] * mt + 2, SENT, dtype=C128), shift=np.full(rows + 2, SENT, dtype=C128),
                      n=a["n"])
        return kw

    @staticmethod
    def expected_flags(e, entry, method, max_passes):
        if method != 0:
            passes, more = 1, 0
        elif entry == ORTH:
            passes, more = (2 if e.needs2 else 1), 0
        else:
            passes = min(2 if e.needs2 else 1, max_passes)
            more = 1 if (e.needs2 and max_passes < 2) else 0
        return passes, 2 * int(e.brk) + more

    def check(self, impl, c, only=None, max_passes=2, args=None):
        """every entry of the case (only: the entry points to keep); returns the number of calls checked"""
        a = args if args is not None else c.args
        e = a["expect"]
        k, rows = a["k"], a["rows"]
        done = {}
        for ent in c.extra["entries"]:
            entry, method = ent[0], ent[1]
            mt = ent[2] if len(ent) > 2 else 0
            if only is not None and entry not in only:
                continue
            kw = self.buffers(a, entry, method, mt)
            res = impl(**kw)
            tag = "%s(method %d)" % (entry, method)
            want_status = NEP_ERR_BREAKDOWN if (e.brk and entry == ORTH) else NEP_OK
            assert res["status"] == want_status, "%s %r: status %d, want %d" % (tag, c, res["status"], want_status)
            out, wo = res["out"], res["w"]
            assert_exact(tag + " (padding of w)", c, wo[rows:], kw["w"][rows:])
            assert_exact(tag + " (padding of d_out)", c, out[k + 2:], kw["out"][k + 2:])
            assert np.all(np.isfinite(out[:k + 2])) and np.all(np.isfinite(wo[:rows])), "%s %r: non-finite result" % (tag, c)
            assert out[k].imag == 0, (tag, c, out[k])
            passes, flags = self.expected_flags(e, entry, method, max_passes)
            assert (out[k + 1].real, out[k + 1].imag) == (passes, flags), \
                "%s %r: (passes, flags) = %r, want %r" % (tag, c, out[k + 1], (passes, flags))
            if c.kind == "exact":
                self._exact(tag, c, e, k, rows, out, wo)
            else:
                self._rounded(tag, c, a, e, entry, method, out, wo, int(passes))
            if entry in (MIRROR, NEXT):
                nm = kw["nmirror"]
                assert_exact(tag + " (mirror row)", c, res["mirror"][:nm], out[:nm])
                assert_exact(tag + " (padding of the mirror)", c, res["mirror"][nm:], kw["mirror"][nm:])
            if entry == NEXT:
                self._next(tag, c, a, e, mt, res, kw)
                # the fused last kernel: the same bits as the two-kernel form (every case lists nep_orth_dev in front of it)
                assert (DEV, method) in done, "%s %r: no nep_orth_dev result to compare with" % (tag, c)
                assert_exact(tag + " against nep_orth_dev: w", c, wo, done[DEV, method]["w"])
                assert_exact(tag + " against nep_orth_dev: d_out", c, out[:k + 2], done[DEV, method]["out"][:k + 2])
            done[entry, method] = res
            _count(entry, c.kind)
        return len(done)

    def _exact(self, tag, c, e, k, rows, out, wo):
        assert_exact(tag + " h", c, out[:k], e.h)
        if e.beta_exact:
            assert_exact(tag + " beta", c, out[k:k + 1].real, np.array([e.beta]))
        else:
            assert_bounded("nep_orth exact tier: beta", c, out[k:k + 1].real.astype(np.longdouble), np.array([e.beta]), 2 * U * float(e.beta))
        if e.w_exact:
            assert_exact(tag + " w", c, wo[:rows], np.asarray(e.w, dtype=C128))
        else:
            assert_bounded("nep_orth exact tier: w", c, wo[:rows].astype(CLD), e.w, 8 * U * np.abs(e.w).astype(np.float64))

    def _rounded(self, tag, c, a, e, entry, method, out, wo, passes):
        k, rows = a["k"], a["rows"]
        Ql, E = e.Ql, e.E
        w_in = a["w"][:rows].astype(CLD)
        an = float(np.sqrt(sumsq(w_in)))
        h, beta, q = out[:k].astype(CLD), float(out[k].real), wo[:rows].astype(CLD)
        sk, nV = np.sqrt(k), np.sqrt(1 + E)
        nA = sk * nV
        assert nA <= 1.01 * sk
        g_d, g_u = SQ2 * gamma(2 * rows + 6), SQ2 * gamma(2 * k + 6)
        fam = "nep_orth" if entry == ORTH else "nep_orth_dev"
        # reconstruction
        rec = float(np.sqrt(sumsq(w_in - Ql @ h - beta * q)))
        if method == 2:
            esum = k * SQ2 * gamma(8) * 2.1 * an
            b_rec = esum + 2.1 * U * an
        else:
            b_rec = g_u * ((8 + 7 * sk) if passes == 2 else (2 + 2 * sk)) * an
        assert_bounded(fam + ": ||w - V h - beta q||", c, np.array([rec]), np.zeros(1), b_rec)
        # orthogonality
        orth = float(np.sqrt(sumsq(np.conj(Ql.T) @ q)))
        if method == 2:
            num = g_d * nA * 1.02 * an + sk * E * float(np.sqrt(sumsq(h))) + sk * nV * esum
        else:
            # pass 1: w_0 is known, so |delta_1| <= cbound(active rows of the column, |V|^H |w_0|) entry by entry
            act = np.full(k, rows) if a["active"] is None else np.minimum(a["active"], rows)
            S1 = np.abs(np.asarray(Ql, dtype=C128)).T @ np.abs(a["w"][:rows])
            d1 = float(np.sqrt(np.sum(np.array([cbound(int(act[j]), S1[j]) for j in range(k)]) ** 2)))
            c1 = nV * an + d1
            e1 = g_u * (an + nA * c1)
            num = d1 + E * c1 + nV * e1
            if passes == 2:
                w1 = min(e.w1norm + nV * d1 + e1, 2.02 * an)
                d2 = g_d * nA * w1
                c2 = nV * w1 + d2
                e2 = g_u * (w1 + nA * c2)
                num = d2 + E * c2 + nV * e2
        assert_bounded(fam + ": ||V^H q||", c, np.array([orth]), np.zeros(1), num / beta + 2.02 * U * nV)
        assert_bounded(fam + ": | ||q|| - 1 |", c, np.array([float(np.sqrt(sumsq(q)))]), np.ones(1), gamma(2 * rows + 6))
        if passes == 1 and method != 2:                        # the coefficients of the first (only) pass
            S = np.abs(np.asarray(Ql, dtype=C128)).T @ np.abs(a["w"][:rows])
            assert_bounded(fam + ": first-pass h", c, h, e.c1, cbound(rows, S))

    def _next(self, tag, c, a, e, mt, res, kw):
        k, rows, n = a["k"], a["rows"], a["n"]
        v = res["w"][:rows].reshape(k + 1, n)
        assert_exact(tag + " (padding of the shifted block)", c, res["shift"][rows:], kw["shift"][rows:])
        assert_exact(tag + " (padding of WT)", c, res["WT"][n * mt:], kw["WT"][n * mt:])
        sc = 1.0 / (np.arange(k + 1) + 1.0)
        assert_exact(tag + " shifted block", c, res["shift"][:rows], (v.real * sc[:, None] + 1j * (v.imag * sc[:, None])).reshape(-1))
        Cm = cm_view(a["C"], 0, k + 1, mt, a["ldc"])
        got = res["WT"][:n * mt].reshape(n, mt)
        if c.kind == "exact":
            assert_exact(tag + " WT", c, got, v.T @ Cm)
        else:
            assert_bounded("nep_orth_dev_iar_next: WT", c, got, v.T.astype(CLD) @ Cm.astype(CLD), cbound(k + 1, np.abs(v.T) @ np.abs(Cm)))


# ================================================================================================================================
H_ROWS = [1, 15, 16, 17, 63, 64, 65, 4032, 4033, 16383, 16384, 16385, 262143, 262144, 262145]
H_KP = [(1, 1), (15, 17), (16, 16), (17, 33), (33, 5)]


def h_rows_per_wg(rows):
    return 1024 if rows >= 262144 else (128 if rows >= 16384 else 64)


class GemmHRm(Prim):
    """impl(WT, ldw, YT, ldy, rows, k, p) -> k p complex (column-major): C = W^H Y for two row-major blocks; W and Y may be the same
    buffer (Gram matrix).  Exact: Gaussian integers in [-8, 8]; rounded: cbound(rows, |W|^T |Y|) against np.clongdouble."""
    name = "nep_gemm_h_rm"
    mutants = ("drop_tail16", "drop_last_wg", "conj_y", "transposed", "ld_as_k", "perturb")

    def cases(self):
        def build(rows, k, p, kind, same=False):
            rng = np.random.default_rng(_seed("ghrm%d.%d.%d%s" % (rows, k, p, kind)))
            W = operand(kind, rng, (rows, k))
            Wb = rowmajor_buf(W, k + 3)
            if same:
                return dict(WT=Wb, ldw=k + 3, YT=Wb, ldy=k + 3, rows=rows, k=k, p=k)
            return dict(WT=Wb, ldw=k + 3, YT=rowmajor_buf(operand(kind, rng, (rows, p)), p + 1), ldy=p + 1, rows=rows, k=k, p=p)

        for rows in H_ROWS:
            for k, p in (H_KP if rows < 16384 else [(17, 5)]) + ([(256, 256), (1, 256)] if rows == 65 else []):
                for kind in ("exact", "rounded"):
                    yield Case("rows%d" % rows, "k%d_p%d" % (k, p), kind, partial(build, rows, k, p, kind))
        for kind in ("exact", "rounded"):
            yield Case("edges", "same_buffer_4033x17", kind, partial(build, 4033, 17, 17, kind, True))

    def ref(self, WT, ldw, YT, ldy, rows, k, p, mut=None, dt=C128):
        if mut == "ld_as_k":
            ldw, ldy = k, p
        r = rows
        if mut == "drop_tail16":
            r = drop_tail(rows, 16)
        if mut == "drop_last_wg":
            r = drop_tail(rows, h_rows_per_wg(rows))
        W = rm_view(WT, 0, rows, k, ldw)[:r].astype(dt); Y = rm_view(YT, 0, rows, p, ldy)[:r].astype(dt)
        Cm = np.conj(W.T) @ (np.conj(Y) if mut == "conj_y" else Y)
        out = Cm.reshape(-1) if mut == "transposed" else Cm.reshape(-1, order="F")      # (row-major in place of column-major)
        return perturb(out) if mut == "perturb" else out

    def check(self, impl, c):
        a = c.args
        got = impl(**a)
        rows, k, p = a["rows"], a["k"], a["p"]
        S = (np.abs(rm_view(a["WT"], 0, rows, k, a["ldw"])).T @ np.abs(rm_view(a["YT"], 0, rows, p, a["ldy"]))).reshape(-1, order="F")
        _count(self.name, c.kind)
        if c.kind == "exact":
            assert_below_2_53(2 * S)
            assert_exact(self.name, c, got, self.ref(**a))
        else:
            assert_bounded(self.name, c, got, self.ref(dt=CLD, **a), cbound(rows, S))


K6 = OrthK6()
K9 = GemmHRm()
CHECKED = ["nep_orth", "nep_orth_dev", "nep_gemm_h_rm"]          # public entry points of include/nepmi355.h checked here
BY_NAME = {"nep_orth": K6, "nep_orth_dev": K6, "nep_gemm_h_rm": K9}
# (primitive_checkers.TABLE, the list of checked entry points, names the three as well and finds their checkers here)
