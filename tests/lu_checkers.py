"""Synthetic factors, a plain-substitution reference, error bounds and mutants for the fixed-shift sparse LU solve (K5:
nep_lu_create[_csc] / nep_lu_solve[_add] / nep_lu_set_row_scale / nep_lu_refactor / nep_lu_transpose of include/nepmi355.h).

The factors are handed to the library as they are generated, with no host factorisation in between, so tree shape, block sizes
against the block maximum, level count, chunk boundaries and the stored diagonal of L are chosen, not inherited from a matrix.

`check(impl, case)` runs `impl(recipe, ops)` and compares every result buffer with the reference.  `impl` receives the factor
arrays of the case (`Recipe`) and a list of solve calls (`Op`) with flat complex128 buffers in place of device pointers and returns
the X buffer of every call; test_gpu_lu_checkers.py passes an adapter that builds ONE handle per recipe and runs all calls on it,
test_host_lu_checkers.py passes `ref_impl` (float64) and its mutants.

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
from functools import partial

import numpy as np
import scipy.sparse as sp
from scipy.sparse.linalg import spsolve_triangular

from primitive_checkers import (Case, assert_exact, assert_bounded, assert_below_2_53, cbound, colmajor_buf, cm_view, gint, grand,
                                perturb, RATIOS, SENT, NAN, C128, CLD, _seed)

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
