"""Synthetic factors, a plain-substitution reference, error bounds and mutants for the fixed-shift sparse LU solve (K5:
nep_lu_create[_csc] / nep_lu_solve[_add] / nep_lu_set_row_scale / nep_lu_refactor / nep_lu_transpose of include/nepmi355.h).

The factors are handed to the library as they are generated, with no host factorisation in between, so tree shape, block sizes
against the block maximum, level count, chunk boundaries and the stored diagonal of L are chosen, not inherited from a matrix.

`check(impl, case)` runs `impl(recipe, ops)` and compares every result buffer with the reference.  `impl` receives the factor
arrays of the case (`Recipe`) and a list of solve calls (`Op`) with flat complex128 buffers in place of device pointers and returns
the X buffer of every call; test_gpu_lu_checkers.py passes an adapter that builds ONE handle per recipe and runs all calls on it,
test_host_lu_checkers.py passes `ref_impl` (float64) and its mutants.  The last section holds the same for the device numeric
factorisation (csrc/lufac.hip): closed fill patterns, the plan's classification restated, `ref_refactor` and its mutants.

Two kinds of case (as in primitive_checkers.py):
  exact    L unit lower with off-diagonal entries in {0, +-1, +-i}, diag(U) in {+-1, +-i}, X Gaussian integers, B = A X formed in
           integer arithmetic, row scales powers of two.  Substitution, the explicit inverses of the diagonal blocks and the dense
           apex inverse only multiply and add (a division by a unit is a swap of components and signs), so the result is the same
           in any order provided every partial sum stays below 2^53.  Asserted per case: every quantity the schedule can form is
           bounded componentwise by  G = M(U)^-1 (|U||x| + M(L)^-1 (|L||y| + |w|))  (M = comparison matrix; |T^-1| <= M(T)^-1 for a
           triangular T, and a diagonal block of T^-1 is the inverse of that block of T), and the entries of the apex inverse by
           M(U)^-1 M(L)^-1 1.  The `dense` family replaces M(.)^-1 by the exact |T^-1| (its comparison matrix grows like 2^n; its
           inverse is bidiagonal by construction).
  rounded  random complex factors with dominant diagonal, reference in np.clongdouble, assertion
           |impl - ref| <= |scale| (C_BLOCK cbound(N, W) + cbound(1, |x| + |add|)),  W = M(U)^-1 (|U||x| + M(L)^-1 |L||y|).
"""
from bisect import bisect_right
from functools import lru_cache, partial

import numpy as np
import scipy.sparse as sp
from scipy.sparse.linalg import spsolve_triangular

from primitive_checkers import (Case, assert_exact, assert_bounded, assert_below_2_53, cbound, colmajor_buf, cm_view, gint, grand,
                                perturb, RATIOS, SENT, NAN, C128, CLD, SQ2, _seed)
from primitive_checkers import U as UNIT_ROUNDOFF

ML_BMAX = 256                 # largest diagonal block of csrc/trsv_ml.hip
NRHS = [1, 2, 3, 4, 5, 7, 8, 9, 13, 32, 33]
UNITS = np.array([1, -1, 1j, -1j], dtype=C128)

# C_BLOCK: the constant c of the rounded bound c gamma_N W.  It pays for solving with explicitly inverted diagonal blocks instead
# of substitution.  Measured on the host (test_host_lu_checkers.py::test_block_inverse_emulation_sets_the_constant): a float64 NumPy
# block-inverse solve over the reference partition at block maxima 8 and 256, over every rounded case, gives
#     r = max |host - ref| / cbound(N, W) = 0.00673       (largest at chain/n3000, block maximum 256)
# and c is the smallest power of two >= 4 r (the factor 4: other summation order, fused multiply-adds, the dense apex).
R_MEASURED = 0.00673
C_BLOCK = 2.0 ** -5


def n_terms(rec):
    """N of the bound: the largest number of terms one result component accumulates in one sweep: the longest row of a factor
    (coupling product plus in-block part) plus the block width ML_BMAX (product with a row of an explicit block inverse)."""
    L, U = rec.matrices(pattern=True)
    return int(max(np.diff(L.tocsr().indptr).max(), np.diff(U.tocsr().indptr).max())) + ML_BMAX


# ================================================================================================================================
# trees (postordered: parent[j] > j) and the factor patterns on them
def complete_tree(depth, arity):
    """parent array of the complete `arity`-ary tree with `depth` levels of nodes, numbered in postorder"""
    parent = []

    def walk(d):
        kids = [walk(d + 1) for _ in range(arity)] if d < depth else []
        parent.append(-1)
        me = len(parent) - 1
        for k in kids:
            parent[k] = me
        return me
    walk(1)
    return np.array(parent, dtype=np.int64)


def ancestor_pairs(parent, extra, rng):
    """(ancestor i, descendant j) pairs: the parent always (the elimination tree is then the tree itself), every further ancestor
    with probability `extra`"""
    rows, cols = [], []
    for j in range(len(parent)):
        a = parent[j]
        first = True
        while a >= 0:
            if first or extra >= 1.0 or rng.random() < extra:
                rows.append(a); cols.append(j)
            first = False
            a = parent[a]
    return np.array(rows, dtype=np.int64), np.array(cols, dtype=np.int64)


def _values(kind, rng, rows, cols, n, upper_diag):
    """values on a strictly triangular pattern + diagonal.  exact: units (one entry in ten an explicit zero, never on the
    parent edge -- the first pair of a column -- ); rounded: rows scaled so that sum_j |t_ij| <= |t_ii| / 2"""
    m = len(rows)
    if kind == "exact":
        v = UNITS[rng.integers(0, 4, m)]
        if m:
            firstofcol = np.r_[True, cols[1:] != cols[:-1]]
            v[(rng.random(m) < 0.1) & ~firstofcol] = 0
        d = UNITS[rng.integers(0, 4, n)] if upper_diag else np.ones(n, dtype=C128)
    else:
        v = grand(rng, m)
        d = np.exp(2j * np.pi * rng.random(n)) * (0.5 + rng.random(n)) if upper_diag else np.ones(n, dtype=C128)
    return v, d


class Recipe:
    """the arrays handed to nep_lu_create[_csc] (+ what is done to the handle before the solves) of one case

    csc, Lp, Li, Lx, Up, Ui, Ux, perm_r, perm_c   as in the header (perms may be None)
    first       (Lx0, Ux0) or None: the handle is created with these values and then refactored with (Lx, Ux)
    rs          row scale (n doubles) or None
    trans       None, 0 (A^-T) or 1 (A^-H): the solves run on nep_lu_transpose(handle, trans)
    absinv      None, or (|L^-1|, |U^-1|) as sparse matrices where the family knows them exactly (dense)"""

    def __init__(self, n, csc, Lp, Li, Lx, Up, Ui, Ux, perm_r=None, perm_c=None, first=None, rs=None, trans=None, absinv=None,
                 kind="exact", ldiag=True):
        self.n, self.csc = n, csc
        self.Lp, self.Li, self.Lx, self.Up, self.Ui, self.Ux = Lp, Li, Lx, Up, Ui, Ux
        self.perm_r, self.perm_c, self.first, self.rs, self.trans, self.absinv = perm_r, perm_c, first, rs, trans, absinv
        self.kind, self.ldiag = kind, ldiag

    def matrices(self, dt=C128, absval=False, pattern=False):
        """(L with its unit diagonal, U) as CSC matrices from the arrays as given (unsorted columns, diagonal of L stored or not)"""
        def mat(p, i, x, unit):
            M = (sp.csc_matrix if self.csc else sp.csr_matrix)((np.ones(len(x)) if pattern else np.abs(x) if absval else x.astype(dt), i.copy(), p.copy()),
                                                               shape=(self.n, self.n)).tocsc()
            M.sort_indices()
            if unit:
                M = (sp.tril(M, -1) + sp.identity(self.n, dtype=M.dtype)).tocsc()
            return M
        return mat(self.Lp, self.Li, self.Lx, True), mat(self.Up, self.Ui, self.Ux, False)


def emit(n, rows, cols, lv, uv, ud, rng, csc=True, ldiag=True, shuffle=False, perms=True, **kw):
    """factor arrays from the strict pattern (rows > cols) of L with values lv; U has the transposed pattern, values uv, diagonal ud"""
    ones = np.ones(n, dtype=C128)
    di = np.arange(n)
    L = sp.coo_matrix((np.r_[lv, ones] if ldiag else lv, (np.r_[rows, di] if ldiag else rows, np.r_[cols, di] if ldiag else cols)), shape=(n, n))
    U = sp.coo_matrix((np.r_[uv, ud], (np.r_[cols, di], np.r_[rows, di])), shape=(n, n))

    def arrays(M):
        # (explicit zeros are kept: coo -> csc/csr sums duplicates only)
        M = M.tocsc() if csc else M.tocsr()
        M.sort_indices()
        p, i, x = M.indptr.astype(np.int32), M.indices.astype(np.int32), M.data.astype(C128)
        if shuffle and csc:                                   # the header: row indices inside a column need not be sorted
            for c in range(n):
                q = rng.permutation(p[c + 1] - p[c]) + p[c]
                i[p[c]:p[c + 1]] = i[q]; x[p[c]:p[c + 1]] = x[q]
        return p, i, x
    Lp, Li, Lx = arrays(L); Up, Ui, Ux = arrays(U)
    pr = rng.permutation(n).astype(np.int32) if perms else None
    pc = rng.permutation(n).astype(np.int32) if perms else None
    return Recipe(n, int(csc), Lp, Li, Lx, Up, Ui, Ux, pr, pc, ldiag=ldiag, **kw)


# ---- families: each returns (n, rows, cols) of the strict pattern of L and, optionally, exact |T^-1| ----------------------------
def fam_diag(n, rng):
    z = np.zeros(0, dtype=np.int64)
    return n, z, z


def fam_chain(n, rng):
    return n, np.arange(1, n, dtype=np.int64), np.arange(0, n - 1, dtype=np.int64)


def fam_tree(depth, arity, extra, rng):
    parent = complete_tree(depth, arity)
    r, c = ancestor_pairs(parent, extra, rng)
    return len(parent), r, c


def fam_two_tier(m, t, rng):
    """m leaves under a chain of t top nodes; L = I - N with entries (top, leaf) only, so N^2 = 0.  Every leaf has an entry in top row
    0 (its parent) and in the others with probability 1/2; the elimination tree chains the top nodes although L has no entry
    between them.  Level 0: m blocks of one row; level 1: one block of t rows with coupling rows of about m / 2 entries"""
    rows, cols = [], []
    for j in range(m):
        tops = [0] + [a for a in range(1, t) if rng.random() < 0.5]
        rows += [m + a for a in tops]; cols += [j] * len(tops)
    return m + t, np.array(rows, dtype=np.int64), np.array(cols, dtype=np.int64)


def fam_arrow(m, t, rng):
    """m leaves under a chain of t top nodes; every leaf has an entry in every top row (the last t rows of L are full in the leaf
    columns: an arrow), the top nodes only in their parent's (a dense unit triangle there would grow like 2^t)"""
    r = np.r_[np.repeat(np.arange(m, m + t), m), np.arange(m + 1, m + t)]
    c = np.r_[np.tile(np.arange(m), t), np.arange(m, m + t - 1)]
    return m + t, r.astype(np.int64), c.astype(np.int64)


def fam_dense(n, rng):
    i, j = np.nonzero(np.tri(n, n, -1))
    return n, i.astype(np.int64), j.astype(np.int64)


def dense_exact_values(n, rows, cols, rng):
    """L = D T D^-1, U = Du E T^T E^-1 with T the all-ones lower triangle and D, E, Du diagonal matrices of units: every entry is a
    unit, L^-1 = D T^-1 D^-1 and U^-1 are bidiagonal with unit entries"""
    d = UNITS[rng.integers(0, 4, n)]; e = UNITS[rng.integers(0, 4, n)]; du = UNITS[rng.integers(0, 4, n)]
    lv = d[rows] * np.conj(d[cols])
    uv = du[cols] * e[cols] * np.conj(e[rows])                 # U[c, r], r > c
    bid = sp.identity(n) + sp.diags(np.ones(n - 1), -1)
    return lv, uv, du, (bid.tocsc(), bid.T.tocsc())


FAMILIES = {
    # name: (generator, forced block maximum of the structure check (None: default), expected (levels, largest block), needs split)
    "diag/n300": (partial(fam_diag, 300), None, (1, 1), False),
    "chain/n1": (partial(fam_chain, 1), None, (1, 1), False),
    "chain/n2": (partial(fam_chain, 2), None, (1, 2), False),
    "chain/n257": (partial(fam_chain, 257), None, (2, 256), False),
    "chain/n3000": (partial(fam_chain, 3000), 96, (32, 96), False),
    "tree/bin11_p0.3": (partial(fam_tree, 11, 2, 0.3), 255, (2, 255), True),
    "tree/bin11_p0.6": (partial(fam_tree, 11, 2, 0.6), 31, (3, 31), True),
    "tree/6ary5_p0.5": (partial(fam_tree, 5, 6, 0.5), 43, (2, 43), True),
    "tree/20ary3_full": (partial(fam_tree, 3, 20, 1.0), 21, (None, 21), True),
    "two_tier/m3000_t32": (partial(fam_two_tier, 3000, 32), 32, (2, 32), True),
    "arrow/m1500_t64": (partial(fam_arrow, 1500, 64), 64, (2, 64), True),
    "dense/n63": (partial(fam_dense, 63), None, (1, 63), False),
    "dense/n64": (partial(fam_dense, 64), 64, (1, 64), False),
    "dense/n65": (partial(fam_dense, 65), 64, (2, 64), True),
    "dense/n255": (partial(fam_dense, 255), None, (1, 255), False),
    "dense/n256": (partial(fam_dense, 256), None, (1, 256), False),
    "dense/n257": (partial(fam_dense, 257), None, (2, 256), True),
}
VARIANTS = {
    # name: emit() switches.  Every family runs "csc" and one further variant (rotating), the small ones all of them.
    "csc": dict(csc=True, ldiag=True, shuffle=False, perms=True),
    "csc_shuffled_nodiag": dict(csc=True, ldiag=False, shuffle=True, perms=True),
    "csr_noperm": dict(csc=False, ldiag=True, shuffle=False, perms=False),
    "csr_nodiag": dict(csc=False, ldiag=False, shuffle=False, perms=True),
    "csc_shuffled_noperm": dict(csc=True, ldiag=True, shuffle=True, perms=False),
}
HANDLE = {
    # what happens to the handle before the solves
    "plain": dict(),
    "rowscale": dict(rs=True),
    "refactor": dict(refactor=True),
    "refactor_rowscale": dict(refactor=True, rs=True),
    "transT": dict(trans=0),
    "transH": dict(trans=1),
    "transH_rowscale": dict(trans=1, rs=True),
    "transT_refactor": dict(trans=0, refactor=True),
}


def make_recipe(fam, variant, handle, kind):
    gen = FAMILIES[fam][0]
    rng = np.random.default_rng(_seed("lu%s%s%s%s" % (fam, variant, handle, kind)))
    n, rows, cols = gen(np.random.default_rng(_seed("pattern" + fam)))      # one pattern per family, whatever the variant
    o = np.lexsort((rows, cols)); rows, cols = rows[o], cols[o]          # column-major: the first pair of a column is the parent edge
    h = HANDLE[handle]
    absinv = None

    def vals():
        nonlocal absinv
        if kind == "exact" and fam.startswith("dense"):
            lv, uv, ud, absinv = dense_exact_values(n, rows, cols, rng)
            return lv, uv, ud
        lv, _ = _values(kind, rng, rows, cols, n, False)
        uv, ud = _values(kind, rng, rows, cols, n, True)
        if kind == "rounded" and len(rows):
            cntL = np.bincount(rows, minlength=n)[rows]                    # entries of L's row
            cntU = np.bincount(cols, minlength=n)[cols]                    # entries of U's row (U[c, r])
            lv = lv * 0.35 / cntL
            uv = uv * 0.35 * np.abs(ud[cols]) / cntU
        return lv, uv, ud
    lv, uv, ud = vals()
    erng = np.random.default_rng(_seed("emit%s%s" % (fam, variant)))     # same arrays' layout and permutations for a family + variant
    rec = emit(n, rows, cols, lv, uv, ud, erng, kind=kind, absinv=absinv, **VARIANTS[variant])
    if h.get("refactor"):
        lv0, uv0, ud0 = vals()                                            # the handle is created with other values of the pattern
        r0 = emit(n, rows, cols, lv0, uv0, ud0, np.random.default_rng(_seed("emit%s%s" % (fam, variant))), **VARIANTS[variant])
        assert np.array_equal(r0.Li, rec.Li) and np.array_equal(r0.Ui, rec.Ui)
        rec.first = (r0.Lx, r0.Ux)
    if h.get("rs"):
        rec.rs = 2.0 ** rng.integers(-3, 4, n) if kind == "exact" else 0.5 + 1.5 * rng.random(n)
    rec.trans = h.get("trans")
    rec.fam = fam
    return rec


def first_recipe(rec):
    """the recipe of the handle as it is created, before nep_lu_refactor, the row scale and the transposition: the first values"""
    r0 = Recipe(rec.n, rec.csc, rec.Lp, rec.Li, rec.first[0], rec.Up, rec.Ui, rec.first[1], rec.perm_r, rec.perm_c, absinv=rec.absinv,
                kind=rec.kind, ldiag=rec.ldiag)
    r0.fam = rec.fam
    return r0


# ================================================================================================================================
# reference
def _substitute(T, W, lower, unit, dt, ldiag_twice=None):
    """plain column-oriented substitution T Y = W (T in CSC with sorted columns), all columns of W at once, in dtype dt"""
    n = T.shape[0]
    p, idx = T.indptr, T.indices
    x = T.data.astype(dt)
    Y = np.array(W, dtype=dt, copy=True)
    order = range(n) if lower else range(n - 1, -1, -1)
    for j in order:
        a, b = p[j], p[j + 1]
        if lower:                                       # diagonal first
            dpos, lo, hi = a, a + 1, b
        else:
            dpos, lo, hi = b - 1, a, b - 1
        if not unit:
            Y[j] = Y[j] / x[dpos]
        elif ldiag_twice is not None and ldiag_twice[j]:
            Y[j] = Y[j] - x[dpos] * Y[j]
        if hi > lo:
            Y[idx[lo:hi]] -= x[lo:hi, None] * Y[j][None, :]
    return Y


def factor_pair(rec, dt, conj_wrong=False):
    """the triangular pair the solves run on, in dtype dt: (L, U) or, for a transposed handle, (U^T D^-1, D L^T) with D = diag(U),
    conjugated for trans = 1; plus the permutations and the input / output scale that go with it"""
    L, U = rec.matrices(C128)
    L = L.astype(C128); U = U.astype(C128)
    Lx, Ux = L.data.astype(dt), U.data.astype(dt)
    if rec.trans is None:
        return (L, Lx), (U, Ux), rec.perm_r, rec.perm_c, rec.rs, None
    conj = (rec.trans == 1) != conj_wrong
    d = U.diagonal().astype(dt)
    Lt = U.T.tocsc(); Lt.sort_indices()                  # U^T: lower; entry (i, j) = U[j, i], scaled by 1 / d_j (column j)
    Ut = L.T.tocsc(); Ut.sort_indices()                  # L^T: upper; entry (i, j) = L[j, i], scaled by d_i (row i)
    # values in extended precision: repeat the transposition on an index matrix
    def tvals(M, vals):
        I = sp.csc_matrix((np.arange(1, M.nnz + 1, dtype=np.float64), M.indices, M.indptr), shape=M.shape).T.tocsc()
        I.sort_indices()
        return vals[I.data.astype(np.int64) - 1], I
    lx, It = tvals(U, Ux)
    cols_of = np.repeat(np.arange(rec.n), np.diff(It.indptr))
    lx = lx / d[cols_of]
    ux, Jt = tvals(L, Lx)
    ux = ux * d[Jt.indices]
    if conj:
        lx, ux = np.conj(lx), np.conj(ux)
    return (It, lx), (Jt, ux), rec.perm_c, rec.perm_r, None, rec.rs


def _csc_with(M, vals):
    return sp.csc_matrix((vals.astype(C128), M.indices, M.indptr), shape=M.shape)


class Op:
    """one nep_lu_solve / nep_lu_solve_add call: B (buffer, ldb), X (buffer, ldx; the object B when aliased), scale,
    add: None (nep_lu_solve), "null" (nep_lu_solve_add with dAdd = NULL), "alias" (dAdd = dX), "own" (a third buffer, ldadd)"""

    def __init__(self, nrhs, B, ldb, X, ldx, scale, add=None, Add=None, ldadd=0):
        self.nrhs, self.B, self.ldb, self.X, self.ldx, self.scale, self.add, self.Add, self.ldadd = nrhs, B, ldb, X, ldx, scale, add, Add, ldadd

    @property
    def alias(self):
        return self.X is self.B


def _perm_in(perm_r, rs, Bm, dt, rs_first_only=False):
    W = np.array(Bm, dtype=dt)
    if rs is not None:
        if rs_first_only:
            W[:, 0] = W[:, 0] * rs.astype(W.real.dtype)
        else:
            W = W * rs.astype(W.real.dtype)[:, None]
    if perm_r is None:
        return W
    out = np.empty_like(W)
    out[perm_r] = W                                      # (Pr b)[perm_r[i]] = b[i]
    return out


def ref_impl(rec, ops, mut=None, dt=C128, want_parts=False):
    """the X buffers of every call after it, computed by plain substitution with the given factors (all right-hand sides of all
    calls in one sweep).  `mut` names a wrong implementation (see MUTANTS)"""
    n = rec.n
    (Lm, lx), (Um, ux), pr, pc, rs_in, rs_out = factor_pair(rec, dt, conj_wrong=(mut == "conj_wrong"))
    if mut == "drop_coupling":
        lx = lx.copy(); lx[_coupling_entry_at_chunk_end(rec, Lm)] = 0
    twice = None
    if mut == "ldiag_twice" and rec.ldiag and rec.trans is None:
        twice = np.ones(n, bool)
    cols, Ws = [], []
    for op in ops:
        ldb = n if mut == "ld_as_n" else op.ldb
        Bm = np.array(cm_view(op.B, 0, n, op.nrhs, ldb))
        if mut == "ld_as_n" and op.ldb > n:
            Bm = np.nan_to_num(Bm, nan=1.0)               # (a kernel that reads padding reads garbage, not necessarily NaN)
        Ws.append(_perm_in(pr, rs_in, Bm, dt, rs_first_only=(mut == "rs_first_rhs_only")))
        cols.append(op.nrhs)
    W = np.concatenate(Ws, axis=1)
    Y = _substitute(_Holder(Lm, lx), W, True, True, dt, twice)
    Z = _substitute(_Holder(Um, ux), Y, False, False, dt)
    Xs = Z if (pc is None or mut == "perm_c_ignored") else Z[pc]          # x[i] = y[perm_c[i]]
    if rs_out is not None:
        Xs = Xs * rs_out.astype(Xs.real.dtype)[:, None]
    outs, parts, c0 = [], [], 0
    for op in ops:
        x = Xs[:, c0:c0 + op.nrhs]
        addm = None
        if op.add == "alias":
            addm = np.array(cm_view(op.X, 0, n, op.nrhs, op.ldx)).astype(dt)
        elif op.add == "own":
            addm = np.array(cm_view(op.Add, 0, n, op.nrhs, op.ldadd)).astype(dt)
        scale = 1.0 if (mut == "scale_ignored_alias" and op.alias) else op.scale
        res = (x + addm if addm is not None else x) * x.real.dtype.type(scale)
        out = op.X.astype(dt)
        ldx = n if mut == "ld_as_n" else op.ldx
        nc = op.nrhs - 1 if (mut == "last_rhs_stale" and op.nrhs % 4) else op.nrhs
        for j in range(nc):
            out[j * ldx: j * ldx + n] = res[:, j]
        if mut == "perturb":
            out[:n] = perturb(out[:n])
        outs.append(out)
        parts.append((Y[:, c0:c0 + op.nrhs], Z[:, c0:c0 + op.nrhs], W[:, c0:c0 + op.nrhs], x, addm))
        c0 += op.nrhs
    return (outs, parts, ((Lm, lx), (Um, ux))) if want_parts else outs


class _Holder:
    """CSC index arrays of a matrix with values of another dtype (SciPy has no extended-precision sparse type)"""

    def __init__(self, M, data):
        self.indptr, self.indices, self.data, self.shape = M.indptr, M.indices, data, M.shape


MUTANTS = ("drop_coupling", "perm_c_ignored", "ld_as_n", "rs_first_rhs_only", "last_rhs_stale", "conj_wrong", "ldiag_twice",
           "scale_ignored_alias", "perturb")
EXACT_ONLY_MUTANTS = ("perturb",)


# ================================================================================================================================
# the partition of csrc/trsv_ml.hip restated (elimination tree of struct(L) + struct(U)^T, one ascending pass)
def reference_partition(n, L, U, bmax=ML_BMAX):
    S = (sp.tril(sp.csr_matrix(L), -1) + sp.triu(sp.csr_matrix(U), 1).T).tocsr()
    S.sort_indices()
    parent = np.full(n, -1); anc = np.full(n, -1)
    ip, ix = S.indptr, S.indices
    for i in range(n):
        for k in ix[ip[i]:ip[i + 1]]:
            while 0 <= k < i:
                nx = anc[k]; anc[k] = i
                if nx < 0:
                    parent[k] = i
                    break
                k = nx
    lvl = np.zeros(n, int); rsz = np.ones(n, int); pmax = np.full(n, -1); psum = np.zeros(n, int)
    for j in range(n):
        M = max(pmax[j], 0); s_ = psum[j] if pmax[j] >= 0 else 0
        if s_ + 1 <= bmax:
            lvl[j], rsz[j] = M, s_ + 1
        else:
            lvl[j], rsz[j] = M + 1, 1
        p = parent[j]
        if p >= 0:
            if lvl[j] > pmax[p]:
                pmax[p], psum[p] = lvl[j], rsz[j]
            elif lvl[j] == pmax[p]:
                psum[p] += rsz[j]
    bid = np.arange(n)
    for j in range(n - 1, -1, -1):
        if parent[j] >= 0 and lvl[parent[j]] == lvl[j]:
            bid[j] = bid[parent[j]]
    return parent, lvl, bid


def _coupling_entry_at_chunk_end(rec, Lm):
    """index (into the CSC values of Lm) of a coupling entry of L whose row is the last of a 4-row chunk of its diagonal block (or
    the last row of the block) under the default partition; any coupling entry where no row is; none where there is no coupling"""
    n = rec.n
    if rec.trans is None:
        _, lvl, bid = reference_partition(n, *rec.matrices(pattern=True))
    else:                                                    # (U of every family has the transposed pattern of L)
        Lt = _csc_with(Lm, np.ones(Lm.nnz))
        _, lvl, bid = reference_partition(n, Lt, Lt.T)
    order = np.lexsort((np.arange(n), bid, lvl))
    pos = np.empty(n, int); pos[order] = np.arange(n)
    start = {}
    for q, j in enumerate(order):
        start.setdefault(bid[j], q)
    size = np.bincount(bid, minlength=n)
    cols_of = np.repeat(np.arange(n), np.diff(Lm.indptr))
    rows = Lm.indices
    off = np.flatnonzero(rows != cols_of)
    if off.size == 0:
        return np.zeros(0, int)
    coup = off[bid[rows[off]] != bid[cols_of[off]]]
    for e in coup:
        i = rows[e]
        k = pos[i] - start[bid[i]]
        if k % 4 == 3 or k == size[bid[i]] - 1:
            return np.array([e])
    return coup[:1]


def emulate_block_solve(Lm, lx, Um, ux, W, bmax):
    """float64 solve with explicitly inverted diagonal blocks over the reference partition, level by level (what the device kernels
    do): y_B = inv(L_BB) (w_B - L_B,prev y_prev), then the same upwards with U"""
    n = Lm.shape[0]
    L = _csc_with(Lm, lx); U = _csc_with(Um, ux)
    _, lvl, bid = reference_partition(n, L, U, bmax)
    order = np.lexsort((np.arange(n), bid, lvl))
    P = sp.csr_matrix((np.ones(n), (np.arange(n), order)), shape=(n, n))
    Lo = (P @ L @ P.T).tocsr(); Uo = (P @ U @ P.T).tocsr()
    bnew = bid[order]
    starts = np.flatnonzero(np.r_[True, bnew[1:] != bnew[:-1]]); ends = np.r_[starts[1:], n]
    w = np.asarray(W, dtype=C128)[order]
    y = np.zeros_like(w); x = np.zeros_like(w)
    for s_, e_ in zip(starts, ends):
        R = Lo[s_:e_]
        r = w[s_:e_] - (R[:, :s_] @ y[:s_] if s_ else 0)
        y[s_:e_] = np.linalg.inv(R[:, s_:e_].toarray()) @ r
    for s_, e_ in zip(starts[::-1], ends[::-1]):
        R = Uo[s_:e_]
        r = y[s_:e_] - (R[:, e_:] @ x[e_:] if e_ < n else 0)
        x[s_:e_] = np.linalg.inv(R[:, s_:e_].toarray()) @ r
    out = np.empty_like(x); out[order] = x
    return out


# ================================================================================================================================
# magnitudes: growth bound of the exact cases, W of the rounded ones
def _minv(T, lower, absinv):
    """v -> M(T)^-1 v (or |T^-1| v where the family knows it)"""
    if absinv is not None:
        return lambda V: absinv @ V
    A = abs(T).tocsr()
    D = sp.diags(A.diagonal())
    M = (2 * D - A).tocsr()
    return lambda V: spsolve_triangular(M, np.asarray(V, dtype=np.float64), lower=lower)


def magnitudes(rec, pair, Y, Z, W):
    """(G, Wb, apex): G = M(U)^-1 (|U||x| + M(L)^-1 (|L||y| + |w|)), Wb = M(U)^-1 (|U||x| + M(L)^-1 |L||y|), both in the order of the
    factor rows; apex = max M(U)^-1 M(L)^-1 1"""
    (Lm, lx), (Um, ux) = pair
    aL = abs(_csc_with(Lm, np.abs(lx).astype(np.float64))); aU = abs(_csc_with(Um, np.abs(ux).astype(np.float64)))
    ai = rec.absinv
    if ai is not None and rec.trans is not None:
        ai = (ai[1].T.tocsc(), ai[0].T.tocsc())
    mL = _minv(aL, True, ai[0] if ai else None); mU = _minv(aU, False, ai[1] if ai else None)
    aY, aZ, aW = (np.abs(M).astype(np.float64) for M in (Y, Z, W))
    ly = aL @ aY; uz = aU @ aZ
    G = mU(uz + mL(ly + aW)); Wb = mU(uz + mL(ly))
    apex = float(np.max(mU(mL(np.ones((rec.n, 1))))))
    return G, Wb, apex


# ================================================================================================================================
# cases
def make_ops(rec, kind, seed, nrhs_list=NRHS):
    """the calls of one handle: every nrhs of the list, cycling through leading dimensions above n (B padded with NaN, X with SENT),
    dX aliasing dB, scales 1, -1, -0.5, nep_lu_solve_add with dAdd aliasing dX, NULL and apart.  In exact cases B = A X is formed
    in integer arithmetic from a Gaussian-integer X (kept in op.truth)"""
    n = rec.n
    rng = np.random.default_rng(seed)
    ops = []
    for t, nrhs in enumerate(nrhs_list):
        scale = (1.0, -1.0, -0.5)[t % 3]
        ldb = n + (0, 3, 1)[t % 3] if t % 4 else n + 2
        ldx = n + (2, 0, 5)[t % 3] if t % 5 else n + 1
        alias = t % 4 == 1
        add = (None, None, "alias", "null", None, "own")[t % 6]
        Xt = gint(rng, (n, nrhs)) if kind == "exact" else None
        Bm = apply_A(rec, Xt) if kind == "exact" else grand(rng, (n, nrhs))
        if alias:
            ldx = ldb
            B = colmajor_buf(Bm, ldb, fill=SENT)              # padding that must neither be read nor change
            X = B
            add = None if add == "alias" else add
        else:
            B = colmajor_buf(Bm, ldb, fill=NAN)
            X = np.full(len(colmajor_buf(Bm, ldx)), SENT, dtype=C128)
        Add, ldadd = None, 0
        if add == "alias":
            X[:] = colmajor_buf(gint(rng, (n, nrhs)) if kind == "exact" else grand(rng, (n, nrhs)), ldx, fill=SENT)
        elif add == "own":
            ldadd = n + 4
            Add = colmajor_buf(gint(rng, (n, nrhs)) if kind == "exact" else grand(rng, (n, nrhs)), ldadd, fill=NAN)
        op = Op(nrhs, B, ldb, X, ldx, scale, add, Add, ldadd)
        op.truth = Xt
        ops.append(op)
    return ops


def apply_A(rec, X):
    """B with A^-1 B = X (A^-T / A^-H for a transposed handle), in complex128 on integers: exact below 2^53 (asserted by check)"""
    n = rec.n
    L, U = rec.matrices(C128)
    rs = rec.rs
    pr, pc = rec.perm_r, rec.perm_c
    if rec.trans is None:
        z = np.empty_like(X)
        z[pc if pc is not None else np.arange(n)] = X           # x[i] = z[perm_c[i]]
        w = L @ (U @ z)
        b = w[pr] if pr is not None else w                       # w[perm_r[i]] = rs[i] b[i]
        return b / rs[:, None] if rs is not None else b
    # x = rs .* (Pr^T s), L'^ U' s = Pc^T b  <=>  b[i] = (U^T L^T s)[perm_c[i]] (conjugated factors for trans = 1)
    y = X / rs[:, None] if rs is not None else X
    s = np.empty_like(X)
    s[pr if pr is not None else np.arange(n)] = y               # y[i] = s[perm_r[i]]
    Lt, Ut = (L.conj(), U.conj()) if rec.trans == 1 else (L, U)
    v = Ut.T @ (Lt.T @ s)
    return v[pc] if pc is not None else v


SHORT_NRHS = ([3, 8, 33, 1, 5, 13, 2, 9], [1, 7, 32, 4, 9, 2, 5, 3], [2, 5, 9, 1, 13, 4, 8, 3], [4, 13, 1, 33, 7, 2, 8, 5])


def cases():
    """family x variant x handle x kind: every family runs every variant in both kinds.  `csc` + `plain` carries the whole nrhs
    list; each of the other four variants runs eight calls on a handle whose treatment (row scale, refactor, transposition, ...)
    rotates with the family, so every treatment meets every variant over the families"""
    vnames = list(VARIANTS); hnames = list(HANDLE)
    for fi, fam in enumerate(FAMILIES):
        for kind in ("exact", "rounded"):
            combos = [("csc", "plain", NRHS)]
            for vi in range(1, len(vnames)):
                combos.append((vnames[vi], hnames[1 + (fi + 2 * vi) % 7], SHORT_NRHS[vi - 1]))
            for variant, handle, nl in combos:
                yield Case(fam, "%s/%s" % (variant, handle), kind, partial(_build, fam, variant, handle, kind, tuple(nl)),
                           extra=dict(fam=fam, variant=variant, handle=handle))


def _build(fam, variant, handle, kind, nl):
    rec = make_recipe(fam, variant, handle, kind)
    return dict(rec=rec, ops=make_ops(rec, kind, _seed("ops%s%s%s%s" % (fam, variant, handle, kind)), nl))


def expected(c, a, c_block=C_BLOCK):
    """per call of the case: (block mask of the X buffer, reference values there, bound there or None for an exact case); the
    exactness assertions of an exact case are made here"""
    rec, ops = a["rec"], a["ops"]
    dt = C128 if c.kind == "exact" else CLD
    want, parts, pair = ref_impl(rec, ops, dt=dt, want_parts=True)
    n = rec.n
    N = n_terms(rec)
    out = []
    for k, (op, wnt, (Y, Z, W, x, addm)) in enumerate(zip(ops, want, parts)):
        blk = np.zeros(len(op.X), bool)
        for j in range(op.nrhs):
            blk[j * op.ldx: j * op.ldx + n] = True
        G, Wb, apex = magnitudes(rec, pair, Y, Z, W)
        extra = (np.abs(addm).astype(np.float64) if addm is not None else 0.0)
        xo = np.abs(x).astype(np.float64)
        # rows of the factor -> entries of x: x[i] = z[perm_c[i]] (and the output scale of a transposed handle)
        pc = rec.perm_c if rec.trans is None else rec.perm_r
        osc = rec.rs if rec.trans is not None else None
        rowsel = (lambda M: M[pc] if pc is not None else M)
        if c.kind == "exact":
            Gx = rowsel(G) * (osc[:, None] if osc is not None else 1.0)
            assert_below_2_53(16 * (Gx + extra))
            assert_below_2_53(16 * apex * np.abs(W).max())
            if op.truth is not None:                              # the reference itself recovers the integers B was formed from
                ref_res = (op.truth + (addm if addm is not None else 0)) * op.scale
                assert_exact("call %d (reference against the integers B was formed from)" % k, c, wnt[blk], ref_res.T.reshape(-1))
            out.append((blk, wnt[blk], None))
        else:
            Wx = rowsel(Wb) * (osc[:, None] if osc is not None else 1.0)
            bound = abs(op.scale) * (c_block * cbound(N, Wx) + cbound(1, xo + extra))
            out.append((blk, wnt[blk], bound.T.reshape(-1)))
    return out


def check(impl, c, name="nep_lu_solve", args=None, cache=None):
    """run impl on the case and hold every call's X buffer to the reference; returns the number of calls checked.  `cache`: a dict
    that keeps the reference of a case for its next run (the same case under another schedule shape)"""
    a = args or c.args
    rec, ops = a["rec"], a["ops"]
    key = (repr(c), name)
    exp = cache.get(key) if cache is not None else None
    if exp is None:
        exp = expected(c, a)
        if cache is not None:
            cache[key] = exp
    got = impl(rec, ops)
    assert len(got) == len(ops)
    for k, (op, g, (blk, wnt, bound)) in enumerate(zip(ops, got, exp)):
        tag = "%s call %d (nrhs %d%s%s)" % (name, k, op.nrhs, ", aliased" if op.alias else "", ", add " + op.add if op.add else "")
        assert_exact(tag + " (padding)", c, np.asarray(g)[~blk], op.X[~blk])
        if bound is None:
            assert_exact(tag, c, np.asarray(g)[blk], wnt)
        else:
            assert_bounded("%s %s" % (name, c.group.split("/")[0]), c, np.asarray(g)[blk], wnt, bound)
    return len(ops)


# ================================================================================================================================
# the device numeric factorisation (csrc/lufac.hip: nep_lu_refac_create / nep_lu_factor_dev[_batch[_terms]]): patterns closed under
# fill, the plan's classification of the products restated, a right-looking reference in step and in panel order, its mutants
#
# Exact cases: units on a closed pattern (one entry in ten an explicit zero, never the parent edge), A = L U on integers.  Every
# partial sum of any elimination order is A_ij minus a subset of the products L_ik U_kj, a Gaussian integer bounded by
# 2 (|L||U|)_ij (asserted < 2^53 per case); a division by a unit pivot is exact.  The device factor therefore equals the generated
# one bit for bit, step by step or in panels.  Rounded cases: the diagonally dominant scaling of make_recipe, assertion
#     |A - L^ U^|_ij <= C_REFAC cbound(N_ij + 1, (|L^||U^|)_ij),   N_ij = stored products of the entry (+ 1: its closing term),
# evaluated in np.clongdouble.
#
# C_REFAC: cbound(N + 1, .) is already the bound of a sum of N + 1 rounded products subtracted from a_ij in any order; the panel
# form needs a margin over it because its multiplier F(i,k) / pivot is recomputed per product (and the in-panel eliminations are
# repeated per destination) and may differ in the last bit from the stored L^ the residual is formed with.  Measured on the host
# (test_host_lu_checkers.py::test_refactor_emulation_sets_the_constant): float64 ref_refactor in step order and in panel order
# P = 2, 3, 4 over every rounded case gives
#     r = max |A - L^ U^| / cbound(N + 1, |L^||U^|) = 0.2963       (largest at arrow/m300_t41/unsym, nep_lu_factor_dev, step order)
# and c is the smallest power of two >= 4 r (the factor 4 as for C_BLOCK: other summation order -- 4 / 16 lanes per external
# segment --, fused multiply-adds, the device's division).
R_REFAC_MEASURED = 0.2963
C_REFAC = 2.0


def close_pattern(n, Lrows, Lcols, Urows=None, Ucols=None):
    """symbolic right-looking fill: pivot k adds (i, j) for every i in L(:,k), j in U(k,:) -- to L where i > j, to U where i < j.
    Returns (Lrows, Lcols) of the strict pattern of L by columns and (Urows, Ucols) of the strict pattern of U by rows; U
    defaults to the transposed pattern of L"""
    if Urows is None:
        Urows, Ucols = Lcols, Lrows
    Lc = [set() for _ in range(n)]; Ur = [set() for _ in range(n)]
    for i, j in zip(np.asarray(Lrows).tolist(), np.asarray(Lcols).tolist()):
        assert i > j
        Lc[j].add(i)
    for i, j in zip(np.asarray(Urows).tolist(), np.asarray(Ucols).tolist()):
        assert i < j
        Ur[i].add(j)
    for k in range(n):
        if not Lc[k] or not Ur[k]:
            continue
        ls, us = sorted(Lc[k]), sorted(Ur[k])
        for j in us:
            Lc[j].update(ls[bisect_right(ls, j):])
        for i in ls:
            Ur[i].update(us[bisect_right(us, i):])
    lr = np.array([i for k in range(n) for i in sorted(Lc[k])], dtype=np.int64)
    lc_ = np.repeat(np.arange(n, dtype=np.int64), [len(s) for s in Lc])
    uc = np.array([j for k in range(n) for j in sorted(Ur[k])], dtype=np.int64)
    ur = np.repeat(np.arange(n, dtype=np.int64), [len(s) for s in Ur])
    return lr, lc_, ur, uc


def fam_grid(nx, ny, rng):
    """five-point grid in natural order (node = x + nx y): closed, it is the full band of width nx; its elimination tree is a chain"""
    node = np.arange(nx * ny, dtype=np.int64)
    x = node % nx
    east = node[x < nx - 1]; north = node[node < nx * (ny - 1)]
    return nx * ny, np.r_[east + 1, north + nx], np.r_[east, north]


# name: (generator of the pattern that is closed, U != L^T before closing, forced block maximum or None).  Wide levels (<= 16
# blocks, level >= 1) and their pivot counts at the block maximum 256: arrow 41 (1 mod 4), two_tier 30 (2 mod 4), bin11 7 (3 mod 4),
# the grids 256 + 64 and 256 + 8 (0 mod 4; banded tops).  bin11 at block maximum 8: levels of 256 / 32 / 4 / 1 blocks of 7, 7, 7, 3
# pivots -- level 1 is NOT wide and runs k_lu_int on external input.
REFAC_CLOSED = {
    "arrow/m300_t41": (partial(fam_arrow, 300, 41), False, None),
    "arrow/m300_t41/unsym": (partial(fam_arrow, 300, 41), True, None),
    "two_tier/m1500_t30": (partial(fam_two_tier, 1500, 30), False, None),
    "two_tier/m1500_t30/unsym": (partial(fam_two_tier, 1500, 30), True, None),
    "tree/bin11_p0.3": (partial(fam_tree, 11, 2, 0.3), False, None),
    "tree/bin11_p0.3/unsym": (partial(fam_tree, 11, 2, 0.3), True, None),
    "tree/bin11_p0.3/bmax8": (partial(fam_tree, 11, 2, 0.3), False, 8),
    "grid/24x24": (partial(fam_grid, 24, 24), False, None),
    "grid/13x40": (partial(fam_grid, 13, 40), False, None),
}
REFAC_NOT_CLOSED = ("arrow/m1500_t64", "two_tier/m3000_t32", "tree/bin11_p0.3")      # of FAMILIES: refused by the plan builder
LU_WIDE_MAXBLK = 16                       # csrc/lufac.hip: a level >= 1 with at most 16 blocks is wide
LU_WIDE_PS = (1, 2, 3, 4)                 # NEP_LU_WIDE_P


@lru_cache(maxsize=None)
def closed_pattern(fam):
    """(n, Lrows, Lcols, Urows, Ucols) of the family: the closure of its generator's pattern; the unsymmetric variant keeps in U only
    the parent edge of every column and a random half of the other entries before closing"""
    gen, unsym, _ = REFAC_CLOSED[fam]
    base = fam[:-len("/unsym")] if unsym else fam
    n, rows, cols = gen(np.random.default_rng(_seed("pattern" + base.replace("/bmax8", ""))))
    o = np.lexsort((rows, cols)); rows, cols = rows[o], cols[o]
    if unsym:
        rng = np.random.default_rng(_seed("unsym" + fam))
        keep = np.r_[True, cols[1:] != cols[:-1]] | (rng.random(len(rows)) < 0.5)
        return (n,) + close_pattern(n, rows, cols, cols[keep], rows[keep])
    return (n,) + close_pattern(n, rows, cols)


def make_closed_recipe(fam, kind, vset=0):
    """factor arrays (CSC, diagonal of L stored, random permutations) with values of `kind` on the closed pattern of the family;
    `vset` numbers independent value sets of the same pattern, layout and permutations (exact sets after the first: U times 4)"""
    n, lr, lc_, ur, uc = closed_pattern(fam)
    rng = np.random.default_rng(_seed("closed%s%s%d" % (fam, kind, vset)))
    lv, _ = _values(kind, rng, lr, lc_, n, False)
    uv, ud = _values(kind, rng, uc, ur, n, True)             # (rows of U play the part of the columns of L: first entry = parent edge)
    if kind == "exact" and vset:                                  # max |U| != max |L|; a division by 4 u, u a unit, is as exact
        uv, ud = 4 * uv, 4 * ud
    if kind == "rounded":
        if len(lr):
            lv = lv * 0.35 / np.bincount(lr, minlength=n)[lr]
        if len(ur):
            uv = uv * 0.35 * np.abs(ud[ur]) / np.bincount(ur, minlength=n)[ur]
    di = np.arange(n)
    L = sp.coo_matrix((np.r_[lv, np.ones(n, dtype=C128)], (np.r_[lr, di], np.r_[lc_, di])), shape=(n, n)).tocsc()
    U = sp.coo_matrix((np.r_[uv, ud], (np.r_[ur, di], np.r_[uc, di])), shape=(n, n)).tocsc()
    L.sort_indices(); U.sort_indices()
    erng = np.random.default_rng(_seed("emit" + fam))
    rec = Recipe(n, 1, L.indptr.astype(np.int32), L.indices.astype(np.int32), L.data.astype(C128), U.indptr.astype(np.int32),
                 U.indices.astype(np.int32), U.data.astype(C128), erng.permutation(n).astype(np.int32), erng.permutation(n).astype(np.int32),
                 kind=kind)
    assert len(rec.Lx) == len(lr) + n and len(rec.Ux) == len(ur) + n      # (explicit zeros are kept)
    rec.fam = fam
    rec.bmax = REFAC_CLOSED[fam][2]
    return rec


def matrix_of(rec):
    """A in the caller's numbering with Pr A Pc = L U, formed on integers: A[i, j] = (L U)[perm_r[i], perm_c[j]]; its CSC pattern is
    the structural product (entries that cancel stay, as explicit zeros)"""
    n = rec.n
    L, U = rec.matrices(C128)
    Lp_, Up_ = rec.matrices(pattern=True)
    P = (Lp_ @ Up_).tocsc(); P.sort_indices()
    V = (L @ U).tocsc()
    pr, pc = np.asarray(rec.perm_r), np.asarray(rec.perm_c)
    ipr = np.empty(n, int); ipr[pr] = np.arange(n); ipc = np.empty(n, int); ipc[pc] = np.arange(n)
    Pc = P.tocoo()
    A = sp.csc_matrix((np.ones(Pc.nnz), (ipr[Pc.row], ipc[Pc.col])), shape=(n, n)); A.sort_indices()
    Ac = A.tocoo()
    vals = np.asarray(V[pr[Ac.row], pc[Ac.col]]).reshape(-1).astype(C128)
    A = sp.csc_matrix((vals + 0, (Ac.row, Ac.col)), shape=(n, n))
    # (csc_matrix from COO drops nothing: explicit zeros are kept)
    A.sort_indices()
    return A


def one_norm(z):
    return np.abs(z.real) + np.abs(z.imag)


class Products:
    """every update F(i,j) -= L(i,k) U(k,j) of the factorisation of a pattern, classified as refac_build of csrc/lufac.hip does.
    Positions are those of the device array F: entry e of the given L at e, entry e of the given U at nnz(L) + e.

    k, i, j, gL, gU, gd   per product, pivots ascending, within a pivot by (column j, row i)
    kind                  0 internal (destination pivot min(i,j) in the block of k, level not wide), 2 wide (the same on a wide level),
                          1 external (destination pivot in a block of a higher level)
    dlev, seg             level of the destination pivot; segment of an external product (-1 otherwise)
    ext                   the external products ordered by (dlev, gd, k); ext_seg / ext_dst: first product / destination of every
                          segment (one per destination), ext_lev[l]: segment range of level l, lanes[l]: lane count k_lu_ext runs with
    counts                [products, internal, external, segments, wide, wide steps, levels] as nep_lu_refac_analyze reports them"""

    def __init__(self, rec, bmax=None):
        n = self.n = rec.n
        Lp, Li, Up, Ui = (np.asarray(a, dtype=np.int64) for a in (rec.Lp, rec.Li, rec.Up, rec.Ui))
        nnzL, nnzU = len(Li), len(Ui)
        self.nnzL, self.nnzU, self.nF = nnzL, nnzU, nnzL + nnzU
        lcol = np.repeat(np.arange(n), np.diff(Lp)); ucol = np.repeat(np.arange(n), np.diff(Up))
        assert np.all(Li >= lcol) and np.all(Ui <= ucol)
        self.ldiag = np.flatnonzero(Li == lcol); self.udiag = nnzL + np.flatnonzero(Ui == ucol)
        assert len(self.ldiag) == n and len(self.udiag) == n
        ls = np.flatnonzero(Li > lcol)
        ls = ls[np.lexsort((Li[ls], lcol[ls]))]                      # strict L by (column, row)
        us = np.flatnonzero(Ui < ucol)
        us = us[np.lexsort((ucol[us], Ui[us]))]                      # strict U by (row, column)
        self.Lrow, self.Lcol, self.Lpos = Li[ls], lcol[ls], ls
        self.Urow, self.Ucol, self.Upos = Ui[us], ucol[us], nnzL + us
        self.Lptr = np.r_[0, np.cumsum(np.bincount(self.Lcol, minlength=n))]
        self.Uptr = np.r_[0, np.cumsum(np.bincount(self.Urow, minlength=n))]
        # (i, j) -> position: the strict entries and the diagonal of U
        keys = np.r_[self.Lrow * n + self.Lcol, self.Urow * n + self.Ucol, np.arange(n) * (n + 1)]
        poss = np.r_[self.Lpos, self.Upos, self.udiag]
        o = np.argsort(keys)
        self._keys, self._poss = keys[o], poss[o]
        # products
        nl, nu = np.diff(self.Lptr), np.diff(self.Uptr)
        cnt = nl * nu
        pbase = np.r_[0, np.cumsum(cnt)]
        k = np.repeat(np.arange(n), cnt)
        local = np.arange(pbase[-1]) - pbase[k]
        a, b = local // np.maximum(nl[k], 1), local % np.maximum(nl[k], 1)
        ue, le = self.Uptr[k] + a, self.Lptr[k] + b
        self.k, self.i, self.j, self.gL, self.gU = k, self.Lrow[le], self.Ucol[ue], self.Lpos[le], self.Upos[ue]
        self.gd = self.pos(self.i, self.j)
        self.closed = bool(np.all(self.gd >= 0))
        if not self.closed:                                         # (an update without a slot: nothing further is defined)
            return
        # partition and classes
        Lpat, Upat = rec.matrices(pattern=True)
        _, lvl, bid = reference_partition(n, Lpat, Upat, bmax or getattr(rec, "bmax", None) or ML_BMAX)
        self.lvl, self.bid = lvl, bid
        nlev = self.nlev = int(lvl.max()) + 1
        self.blocks = [[np.flatnonzero(bid == r) for r in np.unique(bid[lvl == l])] for l in range(nlev)]     # by root index; pivots ascending
        self.wide = np.array([l >= 1 and len(self.blocks[l]) <= LU_WIDE_MAXBLK for l in range(nlev)])
        self.steps = int(sum(max(len(b) for b in self.blocks[l]) for l in range(nlev) if self.wide[l]))
        p = np.minimum(self.i, self.j)
        same = bid[p] == bid[k]
        assert np.all(same | (lvl[p] > lvl[k])), "an update crosses blocks of one level"
        self.kind = np.where(same, np.where(self.wide[lvl[k]], 2, 0), 1)
        self.dlev = lvl[p]
        self.pptr = pbase                                           # products of pivot k: pptr[k] : pptr[k + 1]
        e = np.flatnonzero(self.kind == 1)
        self.ext = e[np.lexsort((self.k[e], self.gd[e], self.dlev[e]))]
        ge, de = self.gd[self.ext], self.dlev[self.ext]
        first = np.r_[True, ge[1:] != ge[:-1]] if len(ge) else np.zeros(0, bool)
        self.ext_seg = np.r_[np.flatnonzero(first), len(ge)]
        self.ext_dst = ge[first]
        seglev = de[first]
        self.ext_lev = [np.searchsorted(seglev, [l, l + 1]) for l in range(nlev)]
        self.seg = np.full(len(k), -1)
        self.seg[self.ext] = np.cumsum(first) - 1
        self.lanes = []
        for l in range(nlev):
            s0, s1 = self.ext_lev[l]
            avg = self.mean_segment_length(l)
            self.lanes.append(0 if s1 == s0 else 16 if avg > 48.0 else 4 if avg > 6.0 else 1)
        self.counts = [len(k), int(np.sum(self.kind == 0)), len(self.ext), len(self.ext_dst), int(np.sum(self.kind == 2)), self.steps, nlev]
        self._panels = {}
        # A: the structural product in the caller's numbering -> positions (amap), as nep_lu_refac_create is given it
        A = matrix_of(rec)
        self.Ap, self.Ai = A.indptr.astype(np.int32), A.indices.astype(np.int32)
        acol = np.repeat(np.arange(n), np.diff(A.indptr))
        fi, fj = np.asarray(rec.perm_r, dtype=np.int64)[A.indices], np.asarray(rec.perm_c, dtype=np.int64)[acol]
        self.amap = self.pos(fi, fj)
        assert np.all(self.amap >= 0)
        self.by_dst = np.argsort(self.gd, kind="stable")
        gs = self.gd[self.by_dst]
        self.dst_first = np.flatnonzero(np.r_[True, gs[1:] != gs[:-1]]) if len(gs) else np.zeros(0, int)
        self.dst_pos = gs[self.dst_first]

    def pos(self, i, j):
        """position of F(i, j), -1 where the entry is not stored"""
        key = np.asarray(i, dtype=np.int64) * self.n + np.asarray(j, dtype=np.int64)
        q = np.minimum(np.searchsorted(self._keys, key), len(self._keys) - 1)
        return np.where(self._keys[q] == key, self._poss[q], -1)

    def mean_segment_length(self, l):
        """external products per destination of level l: what lu_factor_batch_impl picks the lane count of k_lu_ext from"""
        s0, s1 = self.ext_lev[l]
        return (self.ext_seg[s1] - self.ext_seg[s0]) / (s1 - s0) if s1 > s0 else 0.0

    def pivot_products(self, k, kind):
        t = np.arange(self.pptr[k], self.pptr[k + 1])
        return t[self.kind[t] == kind]

    def panels(self, P):
        """the panel form of the wide levels (refac_build_fused) for panels of P pivots: per wide level the panels
        (pivots, hdr = positions of their P x P diagonal block, dst, lr, ur = record operands P x records, own = the pivot has a
        product of its own for the record) and the deferred products of every round (gL, gU, gd, position of the pivot)"""
        if P in self._panels:
            return self._panels[P]
        out = {}
        nrec = nfix = launches = nsteps = 0
        for l in range(self.nlev):
            if not self.wide[l]:
                continue
            pans, defer, step_rec = [], [[] for _ in range(P - 1)], {}
            for blk in self.blocks[l]:
                for s, q0 in enumerate(range(0, len(blk), P)):
                    ks = blk[q0:q0 + P]
                    hdr = np.full((P, P), -1, dtype=np.int64)
                    hdr[:len(ks), :len(ks)] = self.pos(ks[:, None], ks[None, :])
                    rest = []
                    for r, kk in enumerate(ks):
                        t = self.pivot_products(kk, 2)
                        later = ks[r + 1:]
                        d = np.isin(self.i[t], later) | np.isin(self.j[t], later)
                        if d.any():
                            defer[r].append(t[d])
                        rest.append(t[~d])
                    rest = np.concatenate(rest) if rest else np.zeros(0, int)
                    dst, ix = np.unique(self.gd[rest], return_index=True)
                    di, dj = self.i[rest][ix], self.j[rest][ix]
                    lr = np.full((P, len(dst)), -1, dtype=np.int64); ur = lr.copy()
                    lr[:len(ks)] = self.pos(di[None, :], ks[:, None]); ur[:len(ks)] = self.pos(ks[:, None], dj[None, :])
                    pans.append(dict(ks=ks, hdr=hdr, dst=dst, lr=lr, ur=ur, own=(lr >= 0) & (ur >= 0)))
                    step_rec[s] = step_rec.get(s, 0) + len(dst)
                    nrec += len(dst)
            defer = [np.concatenate(d) if d else np.zeros(0, int) for d in defer]
            for t in defer:
                assert len(np.unique(self.gd[t])) == len(t)           # one launch, one product per destination
            nfix += sum(len(t) for t in defer)
            launches += sum(c > 0 for c in step_rec.values()) + sum(len(t) > 0 for t in defer)
            nsteps += len(step_rec)
            out[l] = (pans, defer)
        self._panels[P] = out
        out["info"] = dict(records=nrec, deferred=nfix, launches=launches, panel_steps=nsteps, wide_levels=int(self.wide.sum()))
        return out


@lru_cache(maxsize=None)
def classify_products(fam_or_rec, bmax=None):
    """the plan's classification (Products) of a closed family, or of a recipe; `bmax`: block maximum of the partition (default: the
    family's forced one, or 256)"""
    rec = make_closed_recipe(fam_or_rec, "exact") if isinstance(fam_or_rec, str) else fam_or_rec
    return Products(rec, bmax)


REFAC_MUTANTS = ("deferred_dropped", "chain_operand_missing", "short_panel_as_full", "ext_tail_dropped", "last_wide_column_unscaled",
                 "batch_reads_first_matrix", "terms_first_coefficients", "growth_from_L", "breakdown_unreported", "perturb")


def ref_refactor(rec, Ax_or_terms, P=1, mut=None, dt=C128, plan=None):
    """right-looking elimination of A on the stored pattern with the stored pivot order, in dtype dt, level by level as
    lu_factor_batch_impl: the external products of a level summed per destination, then its pivots -- one by one (block levels;
    wide levels at P = 1, the column of L divided at the end of the level) or in panels of P (wide levels, P >= 2: one
    destination's P products summed first from a bordered elimination of its own, the products into the panel's own later rows and
    columns deferred to P - 1 rounds at the end of the level).

    Ax_or_terms: the values of A in the CSC order of matrix_of(rec) (nnz, or B x nnz for a batch), or a pair (D, Cf) of term values
    (nnz x mt) and coefficients (mt, or B x mt).  Returns (Lx, Ux, health) -- with a leading batch axis where the input had one --,
    health = [broken pivot, max (|Re| + |Im|) over L, max |U| / max |A| in the same norm].  `mut` names a defect (REFAC_MUTANTS)"""
    pl = plan if plan is not None else Products(rec)
    if isinstance(Ax_or_terms, tuple):
        D, Cf = Ax_or_terms
        single = np.ndim(Cf) == 1
        Cf = np.atleast_2d(Cf)
        if mut == "terms_first_coefficients":
            Cf = np.repeat(Cf[:1], len(Cf), axis=0)
        A = np.zeros((len(Cf), D.shape[0]), dtype=dt)
        for t in range(D.shape[1]):
            A += Cf[:, t].astype(dt)[:, None] * D[:, t].astype(dt)[None, :]
    else:
        single = np.ndim(Ax_or_terms) == 1
        A = np.atleast_2d(Ax_or_terms).astype(dt)
    B = len(A)
    F = np.zeros((B, pl.nF), dtype=dt)
    F[:, pl.amap] = A
    F[:, pl.ldiag] = 1
    broken = np.zeros(B, bool)
    gL, gU, gd, ud = pl.gL, pl.gU, pl.gd, pl.udiag
    lmax = np.zeros(B)

    def scale_column(k):
        piv = F[:, ud[k]]
        ap = one_norm(piv).astype(np.float64)
        broken[:] |= ~(ap > 0.0) | ~np.isfinite(ap)
        e = pl.Lpos[pl.Lptr[k]:pl.Lptr[k + 1]]
        if len(e):
            F[:, e] = F[:, e] / piv[:, None]

    with np.errstate(all="ignore"):
        for l in range(pl.nlev):
            s0, s1 = pl.ext_lev[l]
            if s1 > s0:
                t = pl.ext[pl.ext_seg[s0]:pl.ext_seg[s1]]
                prod = F[:, gL[t]] * F[:, gU[t]]
                starts = pl.ext_seg[s0:s1] - pl.ext_seg[s0]
                if mut == "ext_tail_dropped" and pl.lanes[l] > 1:
                    lens = np.diff(pl.ext_seg[s0:s1 + 1])
                    within = np.arange(len(t)) - np.repeat(starts, lens)
                    prod[:, within >= np.repeat(lens // pl.lanes[l] * pl.lanes[l], lens)] = 0
                F[:, pl.ext_dst[s0:s1]] -= np.add.reduceat(prod, starts, axis=1)
            pivots = np.sort(np.concatenate(pl.blocks[l]))
            if not pl.wide[l]:
                for k in pivots:
                    scale_column(k)
                    t = pl.pivot_products(k, 0)
                    if len(t):
                        F[:, gd[t]] -= F[:, gL[t]] * F[:, gU[t]]
                continue
            if P == 1:
                for k in pivots:
                    t = pl.pivot_products(k, 2)
                    if len(t):
                        F[:, gd[t]] -= (F[:, gL[t]] / F[:, ud[k]][:, None]) * F[:, gU[t]]
            else:
                pans, defer = pl.panels(P)[l]
                # (short_panel_as_full: a short last panel never has records -- every later pivot of its block lies inside it, so all its
                # products are deferred -- and the np < P branch of k_lu_widep cannot show in a result; the form of the defect that can is
                # a plan that counts only full panels, steps / P, and so loses the short panel's products)
                short = [pn["ks"] for pn in pans if len(pn["ks"]) < P] if mut == "short_panel_as_full" else []
                short = np.concatenate(short) if short else np.zeros(0, int)
                for pn in pans:
                    npv = len(pn["ks"])
                    if not len(pn["dst"]) or (mut == "short_panel_as_full" and npv < P):
                        continue
                    Fd = F[:1] if mut == "batch_reads_first_matrix" else F
                    Dv = np.where(pn["hdr"] >= 0, Fd[:, np.maximum(pn["hdr"], 0)], 0) + np.zeros((B, 1, 1), dtype=dt)
                    lr, ur = pn["lr"], pn["ur"]
                    if mut == "chain_operand_missing":
                        lr, ur = np.where(pn["own"], lr, -1), np.where(pn["own"], ur, -1)
                    LR = np.where(lr >= 0, F[:, np.maximum(lr, 0)], 0)            # B x P x records
                    UR = np.where(ur >= 0, F[:, np.maximum(ur, 0)], 0)
                    acc = np.zeros((B, len(pn["dst"])), dtype=dt)
                    for q in range(npv):
                        pv = Dv[:, q, q]
                        for r2 in range(q + 1, P):
                            m = Dv[:, r2, q] / pv
                            Dv[:, r2, q + 1:] -= m[:, None] * Dv[:, q, q + 1:]
                            UR[:, r2] -= m[:, None] * UR[:, q]
                        ml = LR[:, q] / pv[:, None]
                        for c in range(q + 1, P):
                            LR[:, c] -= ml * Dv[:, q, c][:, None]
                        acc += ml * UR[:, q]
                    F[:, pn["dst"]] -= acc
                if mut != "deferred_dropped":
                    for r, t in enumerate(defer):
                        t = t[~np.isin(pl.k[t], short)]
                        if len(t):
                            F[:, gd[t]] -= (F[:, gL[t]] / F[:, ud[pl.k[t]]]) * F[:, gU[t]]
            for k in (pivots[:-1] if mut == "last_wide_column_unscaled" else pivots):
                scale_column(k)
        Lx, Ux = F[:, :pl.nnzL], F[:, pl.nnzL:]
        health = np.zeros((B, 3))
        amax = one_norm(A).astype(np.float64).max(axis=1) if A.shape[1] else np.zeros(B)
        lmax = one_norm(F[:, pl.Lpos]).astype(np.float64).max(axis=1) if len(pl.Lpos) else np.zeros(B)
        uabs = one_norm(Ux).astype(np.float64)
        umax = np.where(np.isnan(uabs).any(axis=1), 1.0e300, np.nan_to_num(uabs, nan=0.0).max(axis=1))
        health[:, 0] = 0.0 if mut == "breakdown_unreported" else broken
        health[:, 1] = lmax
        top = lmax if mut == "growth_from_L" else umax
        health[:, 2] = np.where(amax > 0.0, top / np.where(amax > 0.0, amax, 1.0), np.where(top > 0.0, 1.0e300, 0.0))
    if mut == "perturb":
        Ux = Ux.copy(); Ux[-1] = perturb(Ux[-1])
    return (Lx[0], Ux[0], health[0]) if single else (Lx, Ux, health)


def factor_residual(pl, Ax, Lx, Ux):
    """(|A - L U| per stored position, (|L||U|) there, number of stored products there) for factor values in the entry order of the
    recipe, the products summed in np.clongdouble; the unit diagonal of L is taken as exact"""
    Fv = np.r_[Lx, Ux].astype(CLD)
    Fv[pl.ldiag] = 1
    Fa = np.abs(Fv).astype(np.float64)
    S = np.zeros(pl.nF, dtype=CLD); Sa = np.zeros(pl.nF); N = np.zeros(pl.nF, dtype=np.int64)
    if len(pl.gd):
        o = pl.by_dst
        S[pl.dst_pos] = np.add.reduceat(Fv[pl.gL[o]] * Fv[pl.gU[o]], pl.dst_first)
        Sa[pl.dst_pos] = np.add.reduceat(Fa[pl.gL[o]] * Fa[pl.gU[o]], pl.dst_first)
        N[pl.dst_pos] = np.diff(np.r_[pl.dst_first, len(o)])
    # closing term: L(i,j) U(j,j) below the diagonal, 1 U(i,j) on and above it
    S[pl.Lpos] += Fv[pl.Lpos] * Fv[pl.udiag[pl.Lcol]]; Sa[pl.Lpos] += Fa[pl.Lpos] * Fa[pl.udiag[pl.Lcol]]
    up = np.r_[pl.Upos, pl.udiag]
    S[up] += Fv[up]; Sa[up] += Fa[up]
    Af = np.zeros(pl.nF, dtype=CLD); Af[pl.amap] = np.asarray(Ax).astype(CLD)
    keep = np.ones(pl.nF, bool); keep[pl.ldiag] = False
    return np.abs(Af - S).astype(np.float64)[keep], Sa[keep], N[keep]


def refac_ratio(pl, Ax, Lx, Ux):
    """largest |A - L U|_ij / cbound(N_ij + 1, (|L||U|)_ij); infinite for a non-finite factor"""
    if not (np.all(np.isfinite(Lx)) and np.all(np.isfinite(Ux))):
        return np.inf
    res, Sa, N = factor_residual(pl, Ax, Lx, Ux)
    g = (2.0 * (N + 1) + 6.0) * UNIT_ROUNDOFF                    # cbound(N + 1, S) with N an array
    return float(np.max(res / np.maximum(SQ2 * g / (1.0 - g) * Sa, np.finfo(np.float64).tiny)))


def assert_refac_bounded(name, c, pl, Ax, Lx, Ux, c_refac=None):
    ratio = refac_ratio(pl, Ax, Lx, Ux) / (C_REFAC if c_refac is None else c_refac)
    RATIOS[name] = max(RATIOS.get(name, 0.0), ratio)
    assert ratio <= 1.0, "%s %r: |A - L U| / bound = %.3g" % (name, c, ratio)
    return ratio


@lru_cache(maxsize=None)
def refac_inputs(fam, kind):
    """what one closed family's tests share: the recipe, a second value set of its pattern, A and its values for both, the plan's
    classification, and (exact) the assertion that every partial sum of any elimination order is exact"""
    rec, rec2 = make_closed_recipe(fam, kind, 0), make_closed_recipe(fam, kind, 1)
    pl = classify_products(fam)
    assert pl.closed
    A, A2 = matrix_of(rec), matrix_of(rec2)
    assert np.array_equal(A.indptr, pl.Ap) and np.array_equal(A.indices, pl.Ai) and np.array_equal(A2.indices, pl.Ai)
    if kind == "exact":
        for r_, A_ in ((rec, A), (rec2, A2)):
            aL, aU = r_.matrices(absval=True)
            assert_below_2_53(2.0 * (aL @ aU).max() + one_norm(A_.data).max())
    return dict(rec=rec, rec2=rec2, Ax=np.ascontiguousarray(A.data, dtype=C128), Ax2=np.ascontiguousarray(A2.data, dtype=C128), plan=pl)


def with_values(rec, Lx, Ux):
    r = Recipe(rec.n, 1, rec.Lp, rec.Li, np.ascontiguousarray(Lx, dtype=C128), rec.Up, rec.Ui, np.ascontiguousarray(Ux, dtype=C128),
               rec.perm_r, rec.perm_c, kind=rec.kind)
    r.fam, r.bmax = rec.fam, rec.bmax
    return r


REFAC_FORMS = ("nep_lu_factor_dev", "nep_lu_factor_dev_batch", "nep_lu_factor_dev_batch_terms")


@lru_cache(maxsize=None)
def refac_forms(fam, kind):
    """the three calls of a family: name -> (input of ref_refactor, [(recipe with the factor the call has to return, values of A)
    per matrix]).  The batch: the matrix, i times the matrix (L the same, U times i), a second value set of the pattern.  The terms
    (mt = 3, term 1 all zero, coefficients that differ per matrix): exact  A = T0 + (1 + i) T2 with Gaussian-integer T2, the matrices
    A, i A, -A;  rounded  T0 = A, T2 = the second value set with coefficients (1, ., 0), (i, ., 0), (0, ., 1) -- every product and sum
    of the assembly is exact, so the terms call factorises the very matrices of the batch"""
    inp = refac_inputs(fam, kind)
    rec, rec2, Ax, Ax2 = inp["rec"], inp["rec2"], inp["Ax"], inp["Ax2"]
    rec_i = with_values(rec, rec.Lx, 1j * rec.Ux)
    batch = [(rec, Ax), (rec_i, 1j * Ax), (rec2, Ax2)]
    zero = np.zeros(len(Ax), dtype=C128)
    if kind == "exact":
        T2 = gint(np.random.default_rng(_seed("terms" + fam)), len(Ax), -3, 3)
        D = np.stack([Ax - (1 + 1j) * T2, zero, T2], axis=1)
        Cf = np.array([[1, 5, 1 + 1j], [1j, -2, 1j - 1], [-1, 3j, -1 - 1j]], dtype=C128)
        tb = [(rec, Ax), (rec_i, 1j * Ax), (with_values(rec, rec.Lx, -rec.Ux), -Ax)]
    else:
        D = np.stack([Ax, zero, Ax2], axis=1)
        Cf = np.array([[1, 7, 0], [1j, -3, 0], [0, 2, 1]], dtype=C128)
        tb = batch
    return {"nep_lu_factor_dev": (Ax, [(rec, Ax)]),
            "nep_lu_factor_dev_batch": (np.ascontiguousarray(np.stack([a for _, a in batch])), batch),
            "nep_lu_factor_dev_batch_terms": ((np.ascontiguousarray(D), np.ascontiguousarray(Cf)), tb)}


def expected_health(rec, Ax):
    """(0, max (|Re| + |Im|) over the strict part of L, max |U| / max |A|) of the factor of the recipe"""
    L, _ = rec.matrices()
    Ls = sp.tril(L, -1).tocsc()                                   # (explicit zeros stay: they count as 0)
    return np.array([0.0, one_norm(Ls.data).max() if Ls.nnz else 0.0, one_norm(rec.Ux).max() / one_norm(Ax).max()])


def refac_check(impl, fam, kind, P, c_refac=None, forms=REFAC_FORMS):
    """impl(name, rec, input, P) -> (Lx, Ux, health), batch axis first (Lx, Ux None where the call returns no values); every matrix
    of every call: health[0] == 0; exact: L and U bit for bit, health == (0, max |L|, max |U| / max |A|); rounded: the residual
    bound, and the health words equal what the returned values give.  Returns the number of matrices checked"""
    pl = refac_inputs(fam, kind)["plan"]
    c = Case(fam, "P=%d" % P, kind, None)
    m = 0
    for name in forms:
        data, want = refac_forms(fam, kind)[name]
        Lx, Ux, health = impl(name, want[0][0], data, P)
        Lx, Ux, health = (None if Lx is None else np.atleast_2d(Lx)), (None if Ux is None else np.atleast_2d(Ux)), np.atleast_2d(health)
        assert len(health) == len(want)
        for b, (rb, Ab) in enumerate(want):
            tag = "%s[%d]" % (name, b)
            if kind == "exact":
                if Lx is not None:
                    assert_exact(tag + " L", c, Lx[b], rb.Lx)
                    assert_exact(tag + " U", c, Ux[b], rb.Ux)
                assert_exact(tag + " health", c, health[b], expected_health(rb, Ab))
            else:
                assert health[b][0] == 0.0, (tag, c, health[b])
                if Lx is not None:
                    assert_refac_bounded("nep_lu_factor_dev %s" % fam, c, pl, Ab, Lx[b], Ux[b], c_refac)
                    assert_exact(tag + " health", c, health[b], expected_health(with_values(rb, Lx[b], Ux[b]), Ab))
            m += 1
    return m


def breakdown_cases(fam, P):
    """exact factors with one U_kk = 0 (A = L U is exactly singular at pivot k; every earlier quantity stays an integer), k in turn
    inside a level-0 block, the first pivot of a panel of P, a later slot of a panel (any other pivot at P = 1), pivot n - 1; and the
    matrix itself with one NaN at an entry (i, j), i > j, whose transposed entry is stored: the product L(i,j) U(j,i) takes it to
    pivot i.  Yields (label, pivot, values of A)"""
    inp = refac_inputs(fam, "exact")
    rec, pl = inp["rec"], inp["plan"]
    b0 = max(pl.blocks[0], key=len)
    wl = int(np.flatnonzero(pl.wide)[0])
    ks = max(pl.blocks[wl], key=len)
    q_first = 12 if len(ks) > 12 else 0                           # 12: slot 0 for P = 1, 2, 3, 4;  11: the last slot for P = 2, 3, 4
    q_later = 11 if len(ks) > 12 else 1
    assert q_first % P == 0 and (P == 1 or q_later % P != 0) and len(ks) > max(q_first, q_later)
    picks = [("level-0 block", int(b0[len(b0) // 2])), ("first pivot of a panel", int(ks[q_first])), ("later slot of a panel", int(ks[q_later])),
             ("last pivot", rec.n - 1)]
    assert pl.lvl[picks[0][1]] == 0
    for label, k in picks:
        Ux = rec.Ux.copy()
        Ux[pl.udiag[k] - pl.nnzL] = 0
        yield label, k, np.ascontiguousarray(matrix_of(with_values(rec, rec.Lx, Ux)).data, dtype=C128)
    low = np.flatnonzero(pl.amap < pl.nnzL)                        # entries of A that land in L
    e = low[np.isin(pl.amap[low], pl.Lpos)]
    pos = pl.amap[e]
    srt = np.argsort(pl.Lpos)
    at = srt[np.searchsorted(pl.Lpos[srt], pos)]
    ok = pl.pos(pl.Lcol[at], pl.Lrow[at]) >= 0
    e = e[ok][len(e[ok]) // 2]
    Ax = inp["Ax"].copy()
    Ax[e] = complex(np.nan, 0.0)
    yield "NaN entry", -1, Ax


def breakdown_check(impl, fam, P):
    """every breakdown case through the single call: health[0] == 1 (the other words and the values are not specified then)"""
    rec = refac_inputs(fam, "exact")["rec"]
    m = 0
    for label, k, Ax in breakdown_cases(fam, P):
        _, _, health = impl("nep_lu_factor_dev", rec, Ax, P)
        assert np.atleast_2d(health)[0][0] == 1.0, "%s P=%d: %s (pivot %d) not reported: health %r" % (fam, P, label, k, health)
        m += 1
    return m
