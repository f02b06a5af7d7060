"""Reference, error bound and case list for K14, nep_spmf_biforms (csrc/biforms.hip): out[t, j, i] = w_i^H A_t v_j for every term
of a stacked CSR.  The operands come from the recipes of spmf_checkers.py (grid5, band, wide, arrow, degenerate), kept as raw CSR
arrays so that duplicate entries, unsorted columns, empty rows and empty terms reach the library as they are.

`check(case, impl)` runs `impl(rec, W, V) -> array (mt, kv, kw)` and compares with the reference in np.clongdouble.
test_gpu_biforms.py passes an adapter that calls the library, test_host_biforms.py passes a dense evaluation (which has to pass)
and two mutants (which have to be rejected).

The bound, in the style of the K11 check: |got - ref| <= 2 gamma(N) S componentwise with S[t, j, i] = (|W|^T |A_t| |V|)[i, j] and
N = nnz_t + 2, nnz_t the number of stored entries of term t (0 for a term without entries: exact zeros are asserted).  Where the
count comes from: an entry is the sum of nnz_t triple products conj(w) val v.  Summed in any order (rows without entries add
exact zeros) that is at most nnz_t - 1 roundings u per product; each of the two complex multiplications of a triple product has
relative error at most sqrt(2) gamma_2 (Higham, Accuracy and Stability, section 3.6; a fused multiply-add only removes
roundings).  Together (nnz_t - 1 + 4 sqrt(2)) u S < 2 (nnz_t + 2) u S for every nnz_t >= 1.  Nothing is fitted to a device result.
"""
import numpy as np
import scipy.sparse as sp

import spmf_checkers as sc
from primitive_checkers import gamma, grand, C128, CLD, NAN, RATIOS, _seed, colmajor_buf

MAX_WV, MAX_OUT = 32, 3072                       # limits of nep_spmf_biforms (include/nepmi355.h)
SHAPES = [(1, 1), (2, 5), (5, 2)]
ALLC = sc.ALLC


class Case:
    def __init__(self, name, gen, mt, cmask, shapes, **kw):
        self.name, self.gen, self.mt, self.cmask, self.shapes, self.kw = name, gen, mt, cmask, list(shapes), kw

    def __repr__(self):
        return self.name

    def recipe(self):
        n, terms = self.gen(_seed(self.name), self.mt, self.cmask, "rounded", **self.kw)
        return sc.Recipe(self.name, "rounded", n, terms)


def _cases():
    out = []
    # the sizes around one row tile (64 rows) and a few tiles, every term count, real and complex stored values
    for n in (1, 63, 64, 65, 257):
        for mt in (1, 3, 5):
            for cmask, tag in ((0, "real"), (ALLC, "cplx")):
                shapes = SHAPES + ([(32, 32)] if mt == 3 and n in (65, 257) else [])
                out.append(Case("degenerate/n%d_mt%d_%s" % (n, mt, tag), sc.degenerate, mt, cmask, shapes, n=n))
    out.append(Case("degenerate/mixed", sc.degenerate, 3, 0b010, SHAPES, n=200))                       # one complex term: 16-byte values
    out.append(Case("degenerate/empty_rows", sc.degenerate, 3, ALLC, SHAPES, n=200, what="empty_rows"))
    out.append(Case("degenerate/empty_term", sc.degenerate, 3, ALLC, SHAPES, n=200, what="empty_term"))
    out.append(Case("degenerate/dups", sc.degenerate, 2, ALLC, SHAPES, n=200, what="dups"))
    # more than 32 terms: one column per pass, all terms (33: static-size LDS; 70, 128: more than 64 KiB of accumulators)
    out.append(Case("degenerate/mt33", sc.degenerate, 33, 0b101, [(1, 1), (2, 3)], n=130))
    out.append(Case("degenerate/mt70", sc.degenerate, 70, 0, [(1, 1), (3, 2)], n=130))
    out.append(Case("degenerate/mt128", sc.degenerate, 128, ALLC, [(1, 1), (4, 3)], n=130))
    out.append(Case("arrow/n2000_mt1", sc.arrow, 1, ALLC, SHAPES, n=2000))                               # a row and a column of 2000 entries
    out.append(Case("arrow/n2000_mt3_real", sc.arrow, 3, 0, SHAPES + [(32, 32)], n=2000))
    out.append(Case("grid5/17x11", sc.grid5, 3, ALLC, SHAPES + [(32, 32)], X=17, Z=11))
    out.append(Case("grid5/17x11_mt5_real", sc.grid5, 5, 0, SHAPES + [(8, 16)], X=17, Z=11, shuffle=True))   # 5 x 16 accumulators: 3 passes
    out.append(Case("wide/n403", sc.wide, 2, ALLC, SHAPES + [(3, 32)], n=403))                             # rows of up to 300 entries; 2 passes
    # 3072 outputs cap the number of workgroups at 341: with 344 row tiles some workgroups take a second tile
    out.append(Case("band/n22001", sc.band, 3, 0, [(1, 1), (32, 32)], n=22001))
    return out


CASES = _cases()


def operands(case, rec, kw, kv):
    rng = np.random.default_rng(_seed("%s/%dx%d" % (case.name, kw, kv)))
    return grand(rng, (rec.n, kw)), grand(rng, (rec.n, kv))


def ref_forms(rec, W, V, mut=None):
    """(ref, S, N): the forms in clongdouble as an array (mt, kv, kw), the same expression with absolute values, and the count N
    of the bound per term.  mut: "drop_term" (the last term with entries comes out as zero), "conj_V" (v conjugated, not w)"""
    n, mt = rec.n, rec.mt
    kw, kv = W.shape[1], V.shape[1]
    ref = np.zeros((mt, kv, kw), dtype=CLD); S = np.zeros((mt, kv, kw)); N = np.zeros(mt, dtype=np.int64)
    Wc = (W if mut == "conj_V" else W.conj()).astype(CLD)
    Vl = (V.conj() if mut == "conj_V" else V).astype(CLD)
    last = max((t for t in range(mt) if len(rec.terms[t][1])), default=-1)
    for t in range(mt):
        rows, cols, vals = rec.coo(t)
        N[t] = len(vals) + 2 if len(vals) else 0
        if len(vals) == 0 or (mut == "drop_term" and t == last):
            continue
        o = np.argsort(rows, kind="stable")
        rows, cols, v = rows[o], cols[o], vals[o].astype(CLD)
        starts = np.flatnonzero(np.r_[True, rows[1:] != rows[:-1]])
        Y = np.add.reduceat(v[:, None] * Vl[cols], starts, axis=0)                   # the non-empty rows of A_t V
        ref[t] = np.einsum("rj,ri->ji", Y, Wc[rows[starts]])
        A = sp.csr_matrix((np.abs(vals), (rows, cols)), shape=(n, n))
        S[t] = (np.abs(W).T @ (A @ np.abs(V))).T
    return ref, S, N


def bound(S, N):
    return np.array([2 * gamma(int(m)) if m else 0.0 for m in N])[:, None, None] * S


def check_forms(name, got, ref, S, N):
    """asserts the bound, returns the largest |got - ref| / bound"""
    got = np.asarray(got)
    assert got.shape == ref.shape, (name, got.shape, ref.shape)
    assert np.all(np.isfinite(got)), "%s: non-finite result" % name
    err = np.abs(got.astype(CLD) - ref).astype(np.float64)
    b = bound(S, N)
    assert np.all(err[b == 0] == 0), "%s: a term without entries must give exact zeros" % name
    ratio = float(np.max(err[b > 0] / b[b > 0])) if np.any(b > 0) else 0.0
    RATIOS["nep_spmf_biforms"] = max(RATIOS.get("nep_spmf_biforms", 0.0), ratio)
    assert ratio <= 1.0, "%s: |impl - ref| / bound = %.3g (largest error %.3e)" % (name, ratio, float(err.max()))
    return ratio


_REFS = {}


def reference(case, rec, kw, kv):
    """operands and reference of one (case, shape), computed once per process"""
    key = (case.name, kw, kv)
    if key not in _REFS:
        W, V = operands(case, rec, kw, kv)
        _REFS[key] = (W, V) + ref_forms(rec, W, V)
    return _REFS[key]


def check(case, impl, shapes=None):
    """every shape of the case through impl(rec, W, V); returns the largest ratio"""
    rec = case.recipe()
    worst = 0.0
    for kw, kv in (shapes or case.shapes):
        W, V, ref, S, N = reference(case, rec, kw, kv)
        worst = max(worst, check_forms("%s (%d, %d)" % (case.name, kw, kv), impl(rec, W, V), ref, S, N))
    return worst


def dense_forms(rec, W, V, mut=None):
    """complex128 evaluation with dense matrices (duplicate entries add up)"""
    out = np.zeros((rec.mt, V.shape[1], W.shape[1]), dtype=C128)
    last = max((t for t in range(rec.mt) if len(rec.terms[t][1])), default=-1)
    for t in range(rec.mt):
        rows, cols, vals = rec.coo(t)
        if mut == "drop_term" and t == last:
            continue
        A = np.zeros((rec.n, rec.n), dtype=C128)
        np.add.at(A, (rows, cols), vals)
        out[t] = (W.T @ A @ V.conj()).T if mut == "conj_V" else (W.conj().T @ A @ V).T
    return out
