"""Synthetic SPMF operands, references, error bounds and case lists for the SPMF kernels (K1, K2, K11 and the componentwise
backward error: csrc/spmv.hip, csrc/spmv_tile.hip, csrc/lrprod.hip) behind nep_spmf_create, nep_spmf_info, nep_spmf_tile_info,
nep_mlincomb[_dev], nep_resid_batch[_dev], nep_resid_split_dev, nep_resid_batch_cm_dev, nep_resid_block, nep_lr_hankel,
nep_cw_backward_error and nep_csc_to_csr of include/nepmi355.h.

A `Recipe` is a list of CSR terms whose STRUCTURE is chosen (RECIPES: grid stencils in the waveguide's 5 + 2 + 1 slot layout and
other term counts, bands, wide random rows, arrows, degenerate shapes), kept as raw arrays so that duplicate entries and unsorted
columns reach the library as they are.  `check(impl, case)` runs one operation through `impl(op, rec, args) -> dict of flat
buffers`: test_gpu_spmf_checkers.py passes adapters that upload the buffers and call the library on one handle per recipe,
test_host_spmf_checkers.py passes `ref_impl` (which has to pass every case) and its mutants (each of which some exact case has to
reject).

Two kinds of case (see primitive_checkers):
  exact    matrix entries are integers in [-8, 8] (Gaussian integers for complex terms), V, Q, W, B, C, F, tau, x, b Gaussian
           integers.  Every partial sum is an integer; check() asserts that the largest sum of absolute values of the call,
           the squared-norm sums included, is below 2^53, so the result is the same in any order with or without fused
           multiply-adds and the comparison is np.array_equal (norms: np.sqrt of the exact integers, sqrt being correctly rounded).
  rounded  Gaussian operands, reference in np.clongdouble, componentwise |impl - ref| <= bound.  The bounds (cbound(N, S) =
           sqrt(2) gamma_{2N + 6} S of primitive_checkers, nothing fitted):
    K1     z_i is a sum of L_i k triple products val * C[j, t] * V[col, j], L_i the stacked row length (entries of all terms in
           row i).  A kernel may add them in one chain (k_spmv_kfused) or form V c_t first (k_vc): the order-free count is
           N = L_i k, S_i the same sum with absolute values.  (A worst-case analysis of a triple product allows a factor sqrt(2)
           more than cbound's two-factor constant; it is not claimed: the assertion is the stricter cbound(N, S).)
    K2     R[i, s] = sum of L_i triple products val * F[t, s] * Q[col, s]: N = L_i, S[i, s] with absolute values.
    norms  s = sum_i |R[i, s]|^2 from computed R = R_ref + d, |d| <= b componentwise: |s^ - s| <= 2 ||r|| ||b|| + ||b||^2 (propagated,
           Cauchy-Schwarz) + gamma_{2 n + 4} (||r|| + ||b||)^2 (the sum of 2 n squares in any order, each square one rounding
           more).  ||q||^2 has b = 0.  nep_resid_batch returns sqrt: |sqrt(s^) - sqrt(s)| <= |s^ - s| / sqrt(s) + 2 u sqrt(s).
    K11    the form of tests/test_gpu_infbilanczos.py: |c^ - c| <= 2 gamma_N S, N = n + ma mb + L_max,
           S = sum_t sum_{j, i} |tau_t[i + j + 1]| |w_j|^T |A_t| |b_i|.
    omega  r_i = b_i - (M x)_i: cbound(L_i, S_i) with S_i = |b_i| + sum |c_t| |val| |x| (fused form), or one subtraction of the
           given M x (SQ2 gamma_2 (|b_i| + |Mx_i|)).  omega = max_i num_i / den_i: num_i = |r_i| carries the bound of r_i and the
           3 ulp allowed for absval of a complex number (a square root and a fused multiply-add; an assumption like HYPOT_ULP),
           den_i is a sum of L_i + 2 non-negative terms, each a product of up to three factors of which two are absval results:
           relative error gamma_{L_i + 12}; the quotient adds one rounding.  |max_i a_i - max_i b_i| <= max_i |a_i - b_i|, so the
           bound of omega is max_i [(rb_i + 3 u |r_i|) / den_i + (num_i / den_i) gamma_{L_i + 16}] (1 + gamma_{L_i + 16}).
"""
import ctypes as C
import functools
from functools import partial

import numpy as np
import scipy.sparse as sp

from primitive_checkers import (Case, cbound, gamma, U, SQ2, assert_exact, assert_bounded, assert_below_2_53, colmajor_buf,
                                rowmajor_buf, cm_view, rm_view, gint, grand, operand, SENT, NAN, RATIOS, C128, CLD, _seed)

OPS = ("k1", "k2", "k2cm", "k11", "cw")
K1_K = [1, 2, 3, 4, 7, 8, 12, 13, 15, 16, 17, 33, 47, 48, 100, 300]
K2_K = [1, 3, 4, 5, 7, 8, 9, 20, 21, 63, 64, 65, 128, 129, 192, 193, 256, 257, 300]
CM_K = [1, 2, 3, 4, 5, 8, 9, 60, 61]
K11_SHAPES = [(1, 1), (2, 8), (3, 9), (5, 16), (4, 17), (2, 33), (256, 1), (1, 256)]


def cbound_n(N, S):
    """cbound with a term count per component: cbound(N_i, 1) S_i"""
    N = np.asarray(N, dtype=np.int64)
    u, inv = np.unique(N, return_inverse=True)
    c = np.array([float(cbound(int(m), 1.0)) for m in u])[inv].reshape(N.shape)
    return c * np.asarray(S, dtype=np.float64)


def panel_width(mt):
    """columns per pass of the row-major K2 entry points (include/nepmi355.h, nep_resid_batch_dev)"""
    return min(256, max(1, 3072 // mt))


# ================================================================================================================================
# recipes
class Recipe:
    """terms: list of (rowptr int32 (n + 1), colind int32, vals float64 | complex128), passed to nep_spmf_create as they are"""

    def __init__(self, name, kind, n, terms):
        self.name, self.kind, self.n, self.terms, self.mt = name, kind, n, terms, len(terms)
        self.any_complex = any(np.iscomplexobj(v) for _, _, v in terms)
        self.L = sum(np.diff(rp).astype(np.int64) for rp, _, _ in terms)          # stacked row lengths
        self.nnz = int(self.L.sum())

    def coo(self, t):
        rp, ci, v = self.terms[t]
        return np.repeat(np.arange(self.n), np.diff(rp)), ci.astype(np.int64), v

    def ptr_arrays(self):
        """argument arrays of nep_spmf_create / nep_spmf_tiles_analyze (the recipe keeps the NumPy arrays alive)"""
        mt = self.mt
        rp = (C.c_void_p * mt)(); ci = (C.c_void_p * mt)(); vv = (C.c_void_p * mt)(); isc = (C.c_int32 * mt)()
        for i, (r, c, v) in enumerate(self.terms):
            rp[i] = r.ctypes.data; ci[i] = c.ctypes.data; vv[i] = v.ctypes.data; isc[i] = 1 if np.iscomplexobj(v) else 0
        return rp, ci, vv, isc


def _vals(rng, m, kind, cplx):
    if kind == "exact":
        def nz(m):
            v = rng.integers(1, 9, m) * rng.choice([-1, 1], m)
            return v.astype(np.float64)
        return (nz(m) + 1j * rng.integers(-8, 9, m)).astype(C128) if cplx else nz(m)
    return grand(rng, m) if cplx else rng.standard_normal(m)


def _csr(n, rows, cols, vals, rng=None, shuffle=False):
    """COO -> CSR keeping the given order inside a row (duplicates stay; shuffle: column order inside the rows is random)"""
    rows = np.asarray(rows, dtype=np.int64); cols = np.asarray(cols, dtype=np.int64)
    if shuffle:
        p = rng.permutation(len(rows)); rows, cols, vals = rows[p], cols[p], vals[p]
    o = np.argsort(rows, kind="stable")
    rp = np.zeros(n + 1, dtype=np.int32); rp[1:] = np.cumsum(np.bincount(rows, minlength=n))
    return rp, np.ascontiguousarray(cols[o], dtype=np.int32), np.ascontiguousarray(vals[o])


def _mask(cmask, t):
    return bool((cmask >> t) & 1)


DEFAULT_LAYOUT = {1: "5", 2: "52", 3: "521", 4: "5215", 5: "52152", 8: "52152152", 9: "521521521"}


def grid5(seed, mt, cmask, kind, X=61, Z=37, extra=0, layout=None, shuffle=False):
    """X x Z grid numbered along z (row = x Z + z).  Term kinds: '5' five-point stencil, '2' first difference along z (diagonal and
    the next point), '1' identity; the default for mt = 3 is the waveguide's 5 + 2 + 1.  `extra` rows behind the grid carry a
    diagonal entry in every term (n is then no multiple of the stride)."""
    rng = np.random.default_rng(seed); vrng = np.random.default_rng(seed + (kind == "rounded") + 1)      # pattern / values
    layout = layout or DEFAULT_LAYOUT[mt]
    assert len(layout) == mt
    n = X * Z + extra
    x, z = np.divmod(np.arange(X * Z), Z)
    ext = np.arange(X * Z, n)
    terms = []
    for t, ch in enumerate(layout):
        i = np.arange(X * Z)
        if ch == "5":
            rows = [i, i[z > 0], i[z < Z - 1], i[x > 0], i[x < X - 1]]
            cols = [i, i[z > 0] - 1, i[z < Z - 1] + 1, i[x > 0] - Z, i[x < X - 1] + Z]
        elif ch == "2":
            rows = [i, i[z < Z - 1]]; cols = [i, i[z < Z - 1] + 1]
        else:
            rows = [i]; cols = [i]
        rows = np.concatenate(rows + [ext]); cols = np.concatenate(cols + [ext])
        terms.append(_csr(n, rows, cols, _vals(vrng, len(rows), kind, _mask(cmask, t)), rng, shuffle))
    return n, terms


def band(seed, mt, cmask, kind, n=40000):
    """tridiagonal first term, diagonal further terms: consecutive rows, no grid stride"""
    rng = np.random.default_rng(seed); vrng = np.random.default_rng(seed + (kind == "rounded") + 1)      # pattern / values
    i = np.arange(n)
    terms = []
    for t in range(mt):
        rows = np.concatenate([i, i[1:], i[:-1]]) if t == 0 else i
        cols = np.concatenate([i, i[1:] - 1, i[:-1] + 1]) if t == 0 else i
        terms.append(_csr(n, rows, cols, _vals(vrng, len(rows), kind, _mask(cmask, t))))
    return n, terms


def wide(seed, mt, cmask, kind, n=403):
    """rows of 0 or 65 .. 300 stacked entries at random columns, dealt to the terms at random (a column may repeat across terms)"""
    rng = np.random.default_rng(seed); vrng = np.random.default_rng(seed + (kind == "rounded") + 1)      # pattern / values
    L = np.where(rng.random(n) < 0.15, 0, rng.integers(65, min(300, n) + 1, n))
    L[0] = 0; L[1] = min(300, n); L[2] = 65
    rows, cols, term = [], [], []
    for r in range(n):
        if L[r]:
            tt = np.sort(rng.integers(0, mt, L[r]))
            for t in range(mt):
                m = int(np.sum(tt == t))
                rows.append(np.full(m, r)); cols.append(rng.choice(n, m, replace=False)); term.append(np.full(m, t))
    rows, cols, term = np.concatenate(rows), np.concatenate(cols), np.concatenate(term)
    terms = []
    for t in range(mt):
        s = term == t
        terms.append(_csr(n, rows[s], cols[s], _vals(vrng, int(s.sum()), kind, _mask(cmask, t))))
    return n, terms


def arrow(seed, mt, cmask, kind, n=2000):
    """diagonal plus one dense row and one dense column in the first term, diagonal further terms"""
    rng = np.random.default_rng(seed); vrng = np.random.default_rng(seed + (kind == "rounded") + 1)      # pattern / values
    i = np.arange(n)
    r0, c0 = n // 3, (2 * n) // 3
    terms = []
    for t in range(mt):
        if t == 0:
            oth = i[i != r0]; othc = i[(i != c0) & (i != r0)]
            rows = np.concatenate([oth, np.full(n, r0), othc]); cols = np.concatenate([oth, i, np.full(len(othc), c0)])
            keep = ~((rows == cols) & (rows == c0))                     # (c0, c0) comes with the dense column
            keep[np.flatnonzero((rows == c0) & (cols == c0))[:1]] = True
            rows, cols = rows[keep], cols[keep]
        else:
            rows, cols = i, i
        terms.append(_csr(n, rows, cols, _vals(vrng, len(rows), kind, _mask(cmask, t))))
    return n, terms


def degenerate(seed, mt, cmask, kind, n=65, what="plain"):
    """small and odd shapes: `what` = plain (bidiagonal first term, diagonal others), empty_term (term 1 has no entries),
    empty_rows (rows 3 mod 7 and the last row empty in every term), first_row_only, dups (every entry of term 0 stored twice plus
    a third copy on some, columns unsorted), real_and_complex (cmask picks the complex terms; the others stay real)"""
    rng = np.random.default_rng(seed); vrng = np.random.default_rng(seed + (kind == "rounded") + 1)      # pattern / values
    i = np.arange(n)
    terms = []
    for t in range(mt):
        if t == 0:
            rows = np.concatenate([i, i[1:]]); cols = np.concatenate([i, i[1:] - 1])
        else:
            rows = i; cols = (i + t) % n if t % 3 == 2 else i
        if what == "empty_term" and t == 1:
            rows = cols = np.zeros(0, dtype=np.int64)
        if what == "empty_rows":
            k = (rows % 7 != 3) & (rows != n - 1); rows, cols = rows[k], cols[k]
        if what == "first_row_only":
            k = rows == 0; rows, cols = rows[k], cols[k]
            if t == 0:
                rows = np.concatenate([rows, np.zeros(min(n, 5) - 1, dtype=np.int64)]); cols = np.concatenate([cols, np.arange(1, min(n, 5))])
        shuffle = False
        if what == "dups" and t == 0:
            third = rows % 3 == 0
            rows = np.concatenate([rows, rows, rows[third]]); cols = np.concatenate([cols, cols, cols[third]]); shuffle = True
        terms.append(_csr(n, rows, cols, _vals(vrng, len(rows), kind, _mask(cmask, t)), rng, shuffle))
    return n, terms


class Spec:
    """one recipe of the table: generator, create-time environment, expected footprint tiles (blocks, stride, patch x, patch z,
    largest footprint; None: the matrix gets no tiles; tile facts marked + in the table were stated before the code ran, the others
    are what nep_spmf_tiles_analyze returned when the table was written) and the operation sweep it carries"""

    def __init__(self, gen, mt, cmask=0, tiles=None, env=None, slotted=None, k1=(), k2=(), cm=(), k11=(), cw=True, rounded=False, **kw):
        self.gen, self.mt, self.cmask, self.kw, self.tiles, self.env = gen, mt, cmask, kw, tiles, env or {}
        self.slotted = slotted
        self.k1, self.k2, self.cm, self.k11, self.cw, self.rounded = list(k1), list(k2), list(cm), list(k11), cw, rounded

    @property
    def cm_ok(self):
        """nep_resid_batch_cm_dev: tiles, at most 4 terms, a footprint of at most 1200 columns (8 tile columns in 150 KiB of LDS)"""
        return self.tiles is not None and self.mt <= 4 and self.tiles[4] <= 1200


ALLC = 0xFFFFFFFF
SMALL_K1 = [1, 2, 4, 13, 16, 17, 48]
SMALL_K2 = [1, 4, 5, 8, 9, 21, 65]
BIG_K1 = [1, 2, 4, 12, 13, 17]
BIG_K2 = [1, 4, 8, 9, 20, 21, 65]
RECIPES = {
    # ---- grid5: the waveguide's slot layout ------------------------------------------------------------------------------------
    "grid5/61x37": Spec(grid5, 3, ALLC, tiles=(48, 37, 4, 16, 104), slotted=0xD0, k1=K1_K, k2=K2_K, cm=CM_K + [300], k11=K11_SHAPES, rounded=True),   # +
    "grid5/61x37_real": Spec(grid5, 3, 0, tiles=(48, 37, 4, 16, 104), slotted=0xD0, k1=K1_K, k2=SMALL_K2 + [129, 193, 257], cm=CM_K,
                             k11=[(2, 8), (5, 16)], rounded=True, shuffle=True),
    "grid5/61x37+5": Spec(grid5, 3, ALLC, tiles=(49, 37, 4, 16, 104), slotted=0xD0, k1=SMALL_K1, k2=SMALL_K2, cm=[1, 3, 8, 9], extra=5),                # +
    "grid5/7x11": Spec(grid5, 3, ALLC, tiles=(2, 11, 4, 11, 55), slotted=0xD0, k1=SMALL_K1, k2=SMALL_K2, cm=[1, 2, 5, 9], k11=[(3, 9)], X=7, Z=11, rounded=True),  # +
    "grid5/251x131": Spec(grid5, 3, ALLC, tiles=(69, 131, 11, 64, 854), slotted=0xD0, k1=BIG_K1 + [48], k2=BIG_K2, cm=[1, 2, 8, 9, 61], k11=[(2, 8)],
                          X=251, Z=131),                                                                                                     # +
    "grid5/251x131_real": Spec(grid5, 3, 0, tiles=(69, 131, 11, 64, 854), slotted=0xD0, k1=[1, 3, 12, 13], k2=[1, 8, 21], cm=[3, 9], X=251, Z=131),
    "grid5/520x64": Spec(grid5, 3, ALLC, tiles=(48, 64, 11, 64, 832), slotted=0xD0, k1=BIG_K1, k2=[1, 4, 8, 9, 21], cm=[1, 4, 9], X=520, Z=64),
    "grid5/520x64_xp8": Spec(grid5, 3, ALLC, tiles=(65, 64, 8, 64, 640), slotted=0xD0, env=dict(NEP_K1_TILE_XP="8"), k1=[2, 12], k2=[1, 4, 8, 9],
                             cm=[1, 9], cw=False, X=520, Z=64),
    "grid5/520x64_xp13": Spec(grid5, 3, ALLC, tiles=(40, 64, 13, 64, 960), slotted=0xD0, env=dict(NEP_K1_TILE_XP="13"), k1=[2, 12], k2=[1, 4, 8, 9],
                              cm=[1, 9], cw=False, X=520, Z=64),
    # (the 768- and 1024-thread super-panel kernels with the other two flush masks and real values)
    "grid5/520x64_mt1_real": Spec(grid5, 1, 0, tiles=(48, 64, 11, 64, 832), slotted=0x80, env=dict(NEP_K1_TILE_XP="11"), k1=[2, 12], k2=[1, 4, 8, 9], cm=[1, 9], cw=False, X=520, Z=64),
    "grid5/520x64_mt2": Spec(grid5, 2, ALLC, tiles=(48, 64, 11, 64, 832), slotted=0xFF, env=dict(NEP_K1_TILE_XP="11"), k1=[2, 12], k2=[1, 4, 8, 9], cm=[1, 9], cw=False, X=520, Z=64),
    "grid5/520x64_xp13_mt1": Spec(grid5, 1, ALLC, tiles=(40, 64, 13, 64, 960), slotted=0x80, env=dict(NEP_K1_TILE_XP="13"), k1=[2, 12], k2=[1, 4, 8, 9], cm=[1, 9],
                                  cw=False, X=520, Z=64),
    "grid5/520x64_xp13_mt2_real": Spec(grid5, 2, 0, tiles=(40, 64, 13, 64, 960), slotted=0xFF, env=dict(NEP_K1_TILE_XP="13"), k1=[2, 12], k2=[1, 4, 8, 9], cm=[1, 9],
                                       cw=False, X=520, Z=64),
    "grid5/520x64_xp13_real": Spec(grid5, 3, 0, tiles=(40, 64, 13, 64, 960), slotted=0xD0, env=dict(NEP_K1_TILE_XP="13"), k1=[2, 12], k2=[1, 4, 8, 9], cm=[1, 9],
                                   cw=False, X=520, Z=64),
    # ---- grid5: term counts ----------------------------------------------------------------------------------------------------
    "grid5/mt1": Spec(grid5, 1, ALLC, tiles=(48, 37, 4, 16, 104), slotted=0x80, k1=SMALL_K1, k2=SMALL_K2 + [257], cm=[1, 2, 5, 8, 9], k11=[(2, 8)], rounded=True),  # +
    "grid5/mt1_real": Spec(grid5, 1, 0, tiles=(48, 37, 4, 16, 104), slotted=0x80, k1=[1, 4, 17], k2=[1, 5, 9], cm=[3, 9]),
    "grid5/mt2": Spec(grid5, 2, ALLC, tiles=(48, 37, 4, 16, 104), slotted=0xFF, k1=SMALL_K1, k2=SMALL_K2, cm=[1, 2, 5, 8, 9]),                      # +
    "grid5/mt4": Spec(grid5, 4, ALLC, tiles=(48, 37, 4, 16, 104), slotted=None, k1=SMALL_K1, k2=SMALL_K2, cm=[1, 2, 5, 8, 9], rounded=True),         # +
    "grid5/mt4_sum9": Spec(grid5, 4, ALLC, tiles=(48, 37, 4, 16, 104), slotted=None, k1=SMALL_K1, k2=SMALL_K2, cm=[1, 4, 9], layout="5211"),
    "grid5/mt5": Spec(grid5, 5, ALLC, tiles=(48, 37, 4, 16, 104), slotted=None, k1=SMALL_K1, k2=SMALL_K2, cm=[3]),                                   # +
    "grid5/mt4_z": Spec(grid5, 4, ALLC, tiles=(36, 0, 4, 16, 65), slotted=0xFF, k1=[2, 4, 16], k2=[1, 4, 5, 9], cm=[1, 5, 9], layout="2221"),
    "grid5/mt8_diag": Spec(grid5, 8, ALLC, tiles=(36, 0, 4, 16, 64), slotted=0xFF, k1=[2, 4, 16], k2=[1, 4, 5, 9], cm=[3], layout="11111111"),
    "grid5/mt8": Spec(grid5, 8, ALLC, tiles=(48, 37, 4, 16, 104), slotted=None, k1=SMALL_K1, k2=SMALL_K2, cm=[3], k11=[(2, 8)]),                     # +
    "grid5/mt9": Spec(grid5, 9, ALLC, tiles=None, k1=[1, 4, 17], k2=[1, 5, 65], cm=[3]),                                                            # +
    # ---- band ------------------------------------------------------------------------------------------------------------------
    "band/n40000": Spec(band, 2, ALLC, tiles=(79, 0, 8, 64, 514), slotted=0xFF, k1=BIG_K1, k2=BIG_K2, cm=[1, 2, 8, 9], n=40000),                    # +
    "band/n65537": Spec(band, 2, 0, tiles=(129, 0, 8, 64, 514), slotted=0xFF, k1=[1, 2, 12, 13, 17], k2=[1, 8, 21, 65, 129], cm=[2, 9], n=65537),        # +
    # (large matrices with 1, 4, 5 and 7 terms: the non-temporal instantiations of the tiled kernels for M = 1 and 4, k_vc<1 | 3 | 4, 64>)
    "band/n33000_mt1": Spec(band, 1, 0, tiles=(65, 0, 8, 64, 514), slotted=0x80, k1=[1, 2, 12, 13], k2=[1, 4, 8, 9, 21], cm=[1, 2, 9], n=33000),
    "band/n33000_mt1c": Spec(band, 1, ALLC, tiles=(65, 0, 8, 64, 514), slotted=0x80, k1=[1, 2, 12, 13], k2=[1, 4, 8, 9, 21], cm=[1, 2, 9], cw=False, n=33000),
    "band/n33000_mt4": Spec(band, 4, ALLC, tiles=(65, 0, 8, 64, 514), slotted=0xFF, k1=[1, 2, 12, 13], k2=[1, 4, 8, 9, 21], cm=[1, 2, 9], n=33000),
    "band/n33000_mt4_real": Spec(band, 4, 0, tiles=(65, 0, 8, 64, 514), slotted=0xFF, k1=[1, 2, 12, 13], k2=[1, 4, 8, 9, 21], cm=[1, 2, 9], cw=False, n=33000),
    "band/n65537_mt5": Spec(band, 5, 0, tiles=(129, 0, 8, 64, 514), slotted=0xFF, k1=[1, 2, 13, 17], k2=[1, 21, 65], cm=[3], cw=False, n=65537),
    "band/n65537_mt7": Spec(band, 7, ALLC, tiles=(129, 0, 8, 64, 514), slotted=None, k1=[1, 2, 13, 17], k2=[1, 21, 65], cm=[3], cw=False, n=65537),
    # ---- wide ------------------------------------------------------------------------------------------------------------------
    "wide/n403": Spec(wide, 2, ALLC, tiles=(16, 7, 4, 7, 403), k1=SMALL_K1 + [300], k2=SMALL_K2 + [129, 193, 257], cm=[1, 5], k11=[(2, 8), (4, 17)], rounded=True, n=403),
    "wide/n2257": Spec(wide, 3, 2, tiles=(268, 0, 4, 16, 1360), k1=SMALL_K1, k2=SMALL_K2, cm=[3], n=2257),
    "wide/n2257_mt4": Spec(wide, 4, ALLC, tiles=(366, 0, 4, 16, 1022), k1=SMALL_K1, k2=[1, 5, 9, 65], cm=[3], n=2257),
    # ---- arrow -----------------------------------------------------------------------------------------------------------------
    "arrow/mt1": Spec(arrow, 1, ALLC, tiles=(32, 0, 4, 16, 2000), slotted=None, k1=SMALL_K1, k2=SMALL_K2, cm=[3], k11=[(2, 8)], n=2000),            # +
    "arrow/mt4": Spec(arrow, 4, ALLC, tiles=None, k1=SMALL_K1, k2=SMALL_K2, cm=[3], n=2000),                                                        # +
    "arrow/n33000": Spec(arrow, 1, 0, tiles=None, k1=[1, 2, 12, 13, 17], k2=[1, 8, 21, 65], cm=[3], n=33000),
    # ---- degenerate ------------------------------------------------------------------------------------------------------------
    "degenerate/n1": Spec(degenerate, 2, ALLC, tiles=None, k1=[1, 2, 17], k2=[1, 5, 65], cm=[1], k11=[(1, 1), (2, 8)], n=1),
    "degenerate/n2": Spec(degenerate, 2, ALLC, tiles=None, k1=[1, 2, 17], k2=[1, 5, 65], cm=[1], n=2),
    "degenerate/n63": Spec(degenerate, 2, ALLC, tiles=None, k1=SMALL_K1, k2=SMALL_K2, cm=[1], k11=[(3, 9)], n=63, rounded=True),                   # +
    "degenerate/n64": Spec(degenerate, 2, ALLC, tiles=(1, 0, 4, 16, 64), slotted=0xFF, k1=SMALL_K1, k2=SMALL_K2, cm=[1, 5, 9], n=64),               # +
    "degenerate/n65": Spec(degenerate, 2, ALLC, tiles=(2, 0, 4, 16, 64), slotted=0xFF, k1=SMALL_K1, k2=SMALL_K2, cm=[1, 5, 9], n=65),               # +
    "degenerate/empty_term": Spec(degenerate, 3, ALLC, tiles=(25, 2, 4, 2, 11), slotted=0xFF, k1=SMALL_K1, k2=SMALL_K2, cm=[1, 9], k11=[(2, 8)], n=200, what="empty_term"),
    "degenerate/empty_rows": Spec(degenerate, 3, ALLC, tiles=(25, 2, 4, 2, 11), slotted=0xFF, k1=SMALL_K1, k2=SMALL_K2, cm=[1, 9], k11=[(2, 8)], n=200, what="empty_rows"),
    "degenerate/first_row_only": Spec(degenerate, 2, ALLC, tiles=(4, 0, 4, 16, 64), slotted=0xFF, k1=SMALL_K1, k2=SMALL_K2, cm=[1, 9], n=200, what="first_row_only"),
    "degenerate/dups": Spec(degenerate, 2, ALLC, tiles=(4, 0, 4, 16, 65), slotted=0xFF, k1=SMALL_K1, k2=SMALL_K2, cm=[1, 9], k11=[(2, 8)], n=200, what="dups", rounded=True),
    "degenerate/real_and_complex": Spec(degenerate, 3, 0b010, tiles=(25, 2, 4, 2, 11), slotted=0xFF, k1=SMALL_K1, k2=SMALL_K2, cm=[1, 9], n=200),
    "degenerate/mt16": Spec(degenerate, 16, ALLC, tiles=None, k1=SMALL_K1, k2=SMALL_K2 + [192, 193], cm=[1], k11=[(2, 8)], n=200),
    "degenerate/mt33": Spec(degenerate, 33, 0b101, tiles=None, k1=[1, 2, 17], k2=[1, 93, 94], cm=[1], n=130),
    "degenerate/mt128": Spec(degenerate, 128, ALLC, tiles=None, k1=[1, 2, 17, 33], k2=[1, 24, 25, 49], cm=[1], k11=[(2, 8)], n=130),
}


@functools.lru_cache(maxsize=None)
def make_recipe(name, kind):
    sp_ = RECIPES[name]
    n, terms = sp_.gen(_seed(name), sp_.mt, sp_.cmask, kind, **sp_.kw)
    return Recipe(name, kind, n, terms)


def tiles_analyze(lib, rec, k=3):
    """nep_spmf_tiles_analyze on the raw arrays of the recipe: (info[8], maxerr)"""
    rp, ci, vv, isc = rec.ptr_arrays()
    info = (C.c_int64 * 8)(); err = C.c_double(0.0)
    rc = lib.nep_spmf_tiles_analyze(rec.n, rec.mt, rp, ci, vv, isc, int(k), info, C.byref(err))
    assert rc == 0, rc
    return [int(x) for x in info], float(err.value)


# ================================================================================================================================
# reference
PATTERN_MUTANTS = ("drop_last_entry", "drop_last_row", "ignore_terms_ge4", "move_entry_term", "merge_dups_overwrite")
MUTANTS = {
    "k1": PATTERN_MUTANTS + ("conj_C", "ld_wrong", "perturb"),
    "k2": PATTERN_MUTANTS + ("ld_wrong", "pad_col", "no_j0_F", "no_j0_tail", "norm_all_rows", "tail_row0p1", "qnorm_row0", "skip_last_cols4",
                             "skip_last_cols8", "perturb"),
    "k2cm": ("drop_last_entry", "ld_wrong", "norm_all_rows", "tail_row0p1", "qnorm_row0", "skip_last_cols4", "skip_last_cols8", "perturb"),
    "k11": ("drop_last_entry", "hankel_ij", "tau_ld", "no_minus", "perturb"),
    "cw": ("drop_last_entry", "omega_no_b", "perturb"),
}


def _terms(rec, mut=None):
    """per term (rows, cols, vals) with a pattern mutant applied"""
    out = [list(rec.coo(t)) for t in range(rec.mt)]
    if mut == "drop_last_entry":                            # the last stored entry of the middle non-empty row
        ne = np.flatnonzero(rec.L > 0)
        r = int(ne[len(ne) // 2])
        for t in reversed(range(rec.mt)):
            hit = np.flatnonzero(out[t][0] == r)
            if hit.size:
                out[t] = [np.delete(a, hit[-1]) for a in out[t]]
                break
    elif mut == "drop_last_row":
        out = [[a[tm[0] != rec.n - 1] for a in tm] for tm in out]
    elif mut == "ignore_terms_ge4":
        out = [tm if t < 4 else [a[:0] for a in tm] for t, tm in enumerate(out)]
    elif mut == "move_entry_term" and rec.mt > 1:
        t = max(range(rec.mt), key=lambda t: len(out[t][0]))
        e = len(out[t][0]) // 2
        t2 = (t + 1) % rec.mt
        v = np.asarray(out[t][2][e: e + 1])
        out[t2] = [np.concatenate([out[t2][0], out[t][0][e: e + 1]]), np.concatenate([out[t2][1], out[t][1][e: e + 1]]),
                   np.concatenate([out[t2][2], v.astype(out[t2][2].dtype) if np.iscomplexobj(out[t2][2]) or not np.iscomplexobj(v) else v])]
        out[t] = [np.delete(a, e) for a in out[t]]
    elif mut == "merge_dups_overwrite":
        res = []
        for rows, cols, vals in out:
            key = rows * rec.n + cols
            _, last = np.unique(key[::-1], return_index=True)
            keep = np.sort(len(key) - 1 - last)
            res.append([rows[keep], cols[keep], vals[keep]])
        out = res
    return out


def spmm(rec, Xs, mut=None, dt=C128, absval=False):
    """sum_t A_t X_t for per-term n x k blocks Xs[t] (duplicate entries add up).  dt = clongdouble: by hand, columns in chunks."""
    n = rec.n
    k = Xs[0].shape[1]
    out = np.zeros((n, k), dtype=(np.float64 if absval else dt))
    for t, (rows, cols, vals) in enumerate(_terms(rec, mut)):
        if len(rows) == 0:
            continue
        if absval:
            out += sp.csr_matrix((np.abs(vals), (rows, cols)), shape=(n, n)) @ Xs[t]
        elif dt is C128:
            out += sp.csr_matrix((vals.astype(C128), (rows, cols)), shape=(n, n)) @ Xs[t]
        else:
            o = np.argsort(rows, kind="stable")
            rows, cols, v = rows[o], cols[o], vals[o].astype(dt)
            starts = np.flatnonzero(np.r_[True, rows[1:] != rows[:-1]])
            for c0 in range(0, k, 16):
                prod = v[:, None] * Xs[t][cols, c0: c0 + 16]
                out[rows[starts], c0: c0 + 16] += np.add.reduceat(prod, starts, axis=0)
    return out


def _perturb(x):
    x = np.array(x, copy=True)
    f = x.reshape(-1)
    if f.size:
        i = f.size // 2
        f[i] = f[i] * (1 + 1e-13) if f[i] != 0 else 1e-13
    return x


def ref_k1(rec, a, mut=None, dt=C128):
    n, k = rec.n, a["k"]
    V = cm_view(a["V"], 0, n, k, n if (mut == "ld_wrong" and a["ldv"] > n) else a["ldv"]).astype(dt)
    Cm = a["C"].astype(dt)
    if mut == "conj_C":
        Cm = np.conj(Cm)
    W = V @ Cm                                               # n x mt
    z = spmm(rec, [W[:, t: t + 1] for t in range(rec.mt)], mut, dt)[:, 0]
    return _perturb(z) if mut == "perturb" else z


def ref_k2(rec, a, mut=None, dt=C128, cm=False):
    """R (n x k): R[:, s] = sum_t F[t, s] A_t q_s"""
    n, k = rec.n, a["k"]
    ldq = a["ldq"]
    if mut == "ld_wrong":
        ldq = n if cm else k
    Q = np.array(cm_view(a["Q"], 0, n, k, ldq) if cm else rm_view(a["Q"], 0, n, k, ldq)).astype(dt)
    if mut == "pad_col" and not cm and a["ldq"] > k:
        Q[:, k - 1] = rm_view(a["Q"], 0, n, k + 1, ldq)[:, k]
    F = a["F"].astype(dt)
    if mut == "no_j0_F" and not cm:
        P = panel_width(rec.mt)
        F = F[:, np.arange(k) % P]
    R = spmm(rec, [Q * F[t][None, :] for t in range(rec.mt)], mut, dt)
    if mut in ("skip_last_cols4", "skip_last_cols8"):
        q = 4 if mut.endswith("4") else 8
        R[:, k - k % q:] = 0
    return _perturb(R) if mut == "perturb" else R, Q


def dout_layout(rn2, qn2, mt):
    k = len(rn2)
    P = panel_width(mt)
    out = np.zeros(2 * k, dtype=rn2.dtype)
    for j0 in range(0, k, P):
        kk = min(P, k - j0)
        out[2 * j0: 2 * j0 + kk] = rn2[j0: j0 + kk]; out[2 * j0 + kk: 2 * j0 + 2 * kk] = qn2[j0: j0 + kk]
    return out


def _sq(X, dt):
    rt = np.longdouble if dt is CLD else np.float64
    return np.sum(X.real.astype(rt) ** 2 + X.imag.astype(rt) ** 2, axis=0)


def _split_parts(rec, a, R, Q, mut, dt, cm):
    """(rn2 over [0, row0), qn2, tail rows) with the split mutants"""
    n, k = rec.n, a["k"]
    row0 = a["row0"]
    r0 = n if row0 < 0 else row0
    rn2 = _sq(R if mut == "norm_all_rows" else R[:r0], dt)
    qn2 = _sq(Q[:r0] if mut == "qnorm_row0" else Q, dt)
    tail = R[r0:]
    if mut == "tail_row0p1" and n - r0 > 0:
        tail = np.concatenate([R[r0 + 1:], np.zeros((1, k), dtype=R.dtype)])
    return rn2, qn2, tail


def ref_impl(op, rec, a, mut=None, dt=C128):
    """float64 (or clongdouble) NumPy implementation with the output protocol of the device adapters"""
    n, mt = rec.n, rec.mt
    if op == "k1":
        z = ref_k1(rec, a, mut, dt)
        buf = np.concatenate([np.full(a["lead"], SENT, dtype=dt), z, np.full(2, SENT, dtype=dt)])
        return dict(z=buf, z_dev=buf.copy(), z_again=buf.copy(), V_after=a["V"].copy())
    if op == "k2":
        k = a["k"]
        R, Q = ref_k2(rec, a, mut, dt)
        rn2, qn2 = _sq(R, dt), _sq(Q, dt)
        srn2, sqn2, tail = _split_parts(rec, a, R, Q, mut, dt, False)
        tbuf = np.full((n - a["row0"]) * a["ldt"] + 1, SENT, dtype=dt)
        tv = tbuf[:-1].reshape(n - a["row0"], a["ldt"])
        if mut == "no_j0_tail":
            P = panel_width(mt)
            for j0 in range(0, k, P):
                tv[:, : min(P, k - j0)] = tail[:, j0: j0 + P]
        else:
            tv[:, :k] = tail
        out = dict(rnorm=np.sqrt(rn2), qnorm=np.sqrt(qn2), d_out=dout_layout(rn2, qn2, mt), split_out=dout_layout(srn2, sqn2, mt), tail=tbuf)
        if k <= 256:
            out["block_status"] = 0
            out["block"] = rowmajor_buf(R, a["ldr"], fill=SENT).astype(dt)
        else:
            out["block_status"] = -2
        return out
    if op == "k2cm":
        if not a["supported"]:
            return dict(status=-5)
        k = a["k"]
        R, Q = ref_k2(rec, a, mut, dt, cm=True)
        rn2, qn2, tail = _split_parts(rec, a, R, Q, mut, dt, True)
        out = dict(status=0, d_out=np.concatenate([rn2, qn2]))
        if a["row0"] >= 0:
            out["tail"] = np.concatenate([colmajor_buf(tail, a["ldt"], fill=SENT).astype(dt), np.full(1, SENT, dtype=dt)])
        return out
    if op == "k11":
        ma, mb = a["ma"], a["mb"]
        W = cm_view(a["W"], 0, n, ma, a["ldw"]).astype(dt); B = cm_view(a["B"], 0, n, mb, a["ldb"]).astype(dt)
        ldt = ma + mb if (mut == "tau_ld" and a["ldt"] > ma + mb) else a["ldt"]
        tau = cm_view(a["tau"], 0, ma + mb, mt, ldt).astype(dt)
        off = 0 if mut == "hankel_ij" else 1
        Xs = []
        for t in range(mt):
            H = np.array([[tau[i + j + off, t] for i in range(mb)] for j in range(ma)], dtype=dt).reshape(ma, mb)
            Xs.append(B @ H.T)
        Z = spmm(rec, Xs, mut, dt)
        c = -np.sum(np.conj(W) * Z)
        if mut == "no_minus":
            c = -c
        if mut == "perturb":
            c = c * (1 + 1e-13) if c != 0 else 1e-13
        return dict(c_host=c, c_dev=c)
    if op == "cw":
        r, om = _cw_ref(rec, a, mut, dt, fused=True)
        r2, om2 = _cw_ref(rec, a, mut, dt, fused=False)
        return dict(r_fused=r, om_fused=om, r_mx=r2, om_mx=om2)
    raise ValueError(op)


def _cw_den(rec, a, mut=None):
    x = a["x"][:, None]
    den = np.zeros(rec.n)
    for t, (rows, cols, vals) in enumerate(_terms(rec, mut)):
        den += a["cabs"][t] * np.bincount(rows, weights=np.abs(vals) * np.abs(x[cols, 0]), minlength=rec.n)
    if mut != "omega_no_b":
        den = den + np.abs(a["b"])
    if a["extra"] is not None:
        den = den + a["extra"].real
    return den


def _cw_ref(rec, a, mut, dt, fused):
    x = a["x"].astype(dt)[:, None]
    if fused:
        Mx = spmm(rec, [x * dt(a["c"][t]) for t in range(rec.mt)], mut, dt)[:, 0]
    else:
        Mx = a["Mx"].astype(dt)
    r = a["b"].astype(dt) - Mx
    if mut == "perturb":
        r = _perturb(r)
    den = _cw_den(rec, a, mut)
    num = np.abs(r).astype(np.float64)
    ratio = np.where(den > 0, num / np.where(den > 0, den, 1.0), np.where(num > 0, 1e300, 0.0))
    return r, float(ratio.max())


# ================================================================================================================================
# cases
def _k1_args(name, kind, k, edge):
    rec = make_recipe(name, kind)
    rng = np.random.default_rng(_seed("k1%s%d%s" % (name, k, edge)))
    n = rec.n
    V = operand(kind, rng, (n, k)); Cm = operand(kind, rng, (k, rec.mt))
    if edge == "zero_rows":
        Cm[::2, :] = 0
    ldv = n if edge == "tight" else n + 3
    ldc = k if edge == "tight" else k + 2
    return dict(k=k, C=Cm, V=colmajor_buf(V, ldv), ldv=ldv, ldc=ldc, lead=0 if edge == "tight" else 3)


def _k2_args(name, kind, k, row0, edge):
    rec = make_recipe(name, kind)
    rng = np.random.default_rng(_seed("k2%s%d.%d%s" % (name, k, row0, edge)))
    n = rec.n
    Q = operand(kind, rng, (n, k)); F = operand(kind, rng, (rec.mt, k))
    pad = 0 if edge == "tight" else 1
    ldq = k + 3 * pad
    return dict(k=k, F=F, Q=rowmajor_buf(Q, ldq), ldq=ldq, row0=row0, ldr=k + 2 * pad, ldt=k + pad)


def _cm_args(name, kind, k, row0, edge):
    rec = make_recipe(name, kind)
    rng = np.random.default_rng(_seed("cm%s%d.%d%s" % (name, k, row0, edge)))
    n = rec.n
    Q = operand(kind, rng, (n, k)); F = operand(kind, rng, (rec.mt, k))
    pad = 0 if edge == "tight" else 1
    ldq = n + 5 * pad
    return dict(k=k, F=F, Q=colmajor_buf(Q, ldq), ldq=ldq, row0=row0, ldt=max(n - max(row0, 0), 1) + 2 * pad, supported=RECIPES[name].cm_ok)


def _k11_args(name, kind, ma, mb):
    rec = make_recipe(name, kind)
    rng = np.random.default_rng(_seed("k11%s%d.%d" % (name, ma, mb)))
    n, mt = rec.n, rec.mt
    lo = 2 if kind == "exact" else None
    W = gint(rng, (n, ma), -lo, lo) if lo else grand(rng, (n, ma))
    B = gint(rng, (n, mb), -lo, lo) if lo else grand(rng, (n, mb))
    tau = gint(rng, (ma + mb, mt), -lo, lo) if lo else grand(rng, (ma + mb, mt))
    ldw, ldb, ldt = n + 2, n + 7, ma + mb + 3
    return dict(ma=ma, mb=mb, W=colmajor_buf(W, ldw), ldw=ldw, B=colmajor_buf(B, ldb), ldb=ldb, tau=colmajor_buf(tau, ldt), ldt=ldt)


def _cw_args(name, kind, extra):
    rec = make_recipe(name, kind)
    rng = np.random.default_rng(_seed("cw%s%d" % (name, extra)))
    n, mt = rec.n, rec.mt
    c = operand(kind, rng, mt); x = operand(kind, rng, n); b = operand(kind, rng, n)
    a = dict(c=c, cabs=np.abs(c), x=x, b=b, extra=(np.abs(grand(rng, n)) + 0j) if extra else None)
    Mx = spmm(rec, [x[:, None].astype(CLD if kind == "rounded" else C128) * c[t] for t in range(mt)], None, CLD if kind == "rounded" else C128)[:, 0]
    a["Mx"] = Mx.astype(C128)
    return a


def row0_list(n):
    return sorted(set(r for r in (0, 1, n - 37, n - 1, n) if 0 <= r <= n))


def cases(name):
    """the cases of one recipe, in the order the device file runs them on its handle"""
    s = RECIPES[name]
    kinds = ("exact", "rounded") if s.rounded else ("exact",)
    for kind in kinds:
        rk = 65 if kind == "rounded" else 10 ** 9                 # the rounded cases repeat the small shapes only
        for i, k in enumerate(s.k1):
            if k <= rk:
                edge = ("padded", "tight", "zero_rows")[i % 3]
                yield Case(name, "k1/k%d_%s" % (k, edge), kind, partial(_k1_args, name, kind, k, edge), extra=dict(op="k1", k=k))
        n = make_recipe(name, kind).n
        r0s = row0_list(n)
        for i, k in enumerate(s.k2):
            if k <= rk:
                edge = "tight" if i % 3 == 1 else "padded"
                row0 = r0s[i % len(r0s)]
                yield Case(name, "k2/k%d_row%d_%s" % (k, row0, edge), kind, partial(_k2_args, name, kind, k, row0, edge), extra=dict(op="k2", k=k))
        if s.k2 and kind == "exact":                                # the whole row0 list at one ragged k
            for row0 in r0s:
                yield Case(name, "k2/k5_row%d_sweep" % row0, kind, partial(_k2_args, name, kind, 5, row0, "padded"), extra=dict(op="k2", k=5))
        for i, k in enumerate(s.cm):
            if k <= rk:
                edge = "tight" if i % 3 == 1 else "padded"
                row0 = ([-1] + r0s)[i % (len(r0s) + 1)]
                yield Case(name, "k2cm/k%d_row%d_%s" % (k, row0, edge), kind, partial(_cm_args, name, kind, k, row0, edge), extra=dict(op="k2cm", k=k))
        if s.cm_ok and kind == "exact":
            for row0 in [-1] + r0s:
                yield Case(name, "k2cm/k3_row%d_sweep" % row0, kind, partial(_cm_args, name, kind, 3, row0, "padded"), extra=dict(op="k2cm", k=3))
        for ma, mb in s.k11:
            if kind == "exact" or ma + mb <= 40:
                yield Case(name, "k11/%dx%d" % (ma, mb), kind, partial(_k11_args, name, kind, ma, mb), extra=dict(op="k11"))
        if s.cw:
            for extra in (0, 1):
                yield Case(name, "cw/extra%d" % extra, kind, partial(_cw_args, name, kind, extra), extra=dict(op="cw"))


def all_cases():
    for name in RECIPES:
        yield from cases(name)


# ================================================================================================================================
# checks
COUNTS = {}                                                 # entry point -> [exact calls, rounded calls]


def _count(entry, kind, k=1):
    COUNTS.setdefault(entry, [0, 0])[0 if kind == "exact" else 1] += k


def _absS(rec, Xs):
    return spmm(rec, Xs, None, absval=True)


def check(impl, c, args=None, cache=None):
    """run case c through impl and assert; returns the number of library calls checked.  `cache` (a dict the caller drops with the
    case) keeps the reference and the bound sums when the same case runs again, under another kernel choice"""
    op = c.extra["op"]
    rec = make_recipe(c.group, c.kind)
    a = args if args is not None else c.args
    fam = c.group.split("/")[0]
    exact = c.kind == "exact"
    dt = C128 if exact else CLD
    n, mt = rec.n, rec.mt
    def memo(what, f):
        if cache is None:
            return f()
        if what not in cache:
            cache[what] = f()
        return cache[what]

    out = impl(op, rec, a)
    ref = memo("ref", lambda: ref_impl(op, rec, a, None, dt))

    def tag(entry):
        return "%s [%s]" % (entry, fam)

    if op == "k1":
        k = a["k"]
        S = memo("S", lambda: _absS(rec, [(np.abs(cm_view(a["V"], 0, n, k, a["ldv"])) @ np.abs(a["C"]))[:, t: t + 1] for t in range(mt)])[:, 0])
        lead = a["lead"]
        assert_exact("nep_mlincomb (V unchanged)", c, out["V_after"], a["V"])
        for key, entry in (("z", "nep_mlincomb"), ("z_dev", "nep_mlincomb_dev")):
            got = out[key]
            pad = np.r_[got[:lead], got[lead + n:]]
            assert_exact(entry + " (padding)", c, pad, np.full(lead + 2, SENT))
            if exact:
                assert_below_2_53(2 * S)
                assert_exact(entry, c, got[lead: lead + n], ref["z"][lead: lead + n])
            else:
                assert_bounded(tag(entry), c, got[lead: lead + n], ref["z"][lead: lead + n], cbound_n(np.maximum(rec.L, 1) * k, S))
            _count(entry, c.kind)
        assert_exact("nep_mlincomb_dev (same bits as nep_mlincomb)", c, out["z_dev"].view(np.float64), out["z"].view(np.float64))
        assert_exact("nep_mlincomb (repeated call)", c, out["z_again"].view(np.float64), out["z"].view(np.float64))
        return 3
    if op in ("k2", "k2cm"):
        cmf = op == "k2cm"
        if cmf:
            assert out["status"] == ref["status"], "nep_resid_batch_cm_dev %r: status %d, want %d" % (c, out["status"], ref["status"])
            _count("nep_resid_batch_cm_dev", c.kind)
            if ref["status"] != 0:
                return 1
        k = a["k"]
        R, Q = memo("RQ", lambda: ref_k2(rec, a, None, dt, cm=cmf))
        Qa = memo("Qa", lambda: np.abs(Q).astype(np.float64))
        S = memo("S", lambda: _absS(rec, [Qa * np.abs(a["F"][t])[None, :] for t in range(mt)]))
        row0 = a["row0"]
        r0 = n if row0 < 0 else row0
        if exact:
            assert_below_2_53(2 * S)
            assert_below_2_53(np.sum(S * S, axis=0)); assert_below_2_53(np.sum(Qa * Qa, axis=0))
        Rb = memo("Rb", lambda: cbound_n(np.maximum(rec.L, 1)[:, None], S))                 # componentwise bound of R

        def sq_bound(rows):
            rr = np.sqrt(np.sum(np.abs(R[rows]).astype(np.float64) ** 2, axis=0)); bb = np.sqrt(np.sum(Rb[rows] ** 2, axis=0))
            return 2 * rr * bb + bb * bb + gamma(2 * n + 4) * (rr + bb) ** 2
        qb = gamma(2 * n + 4) * np.sum(Qa * Qa, axis=0)

        def cmp_dout(entry, got, want, rows):
            if exact:
                assert_exact(entry, c, got, want)
            else:
                rb = sq_bound(rows)
                assert_bounded(tag(entry), c, got, want, np.concatenate([rb, qb]) if cmf else dout_layout(rb, qb, mt))
            _count(entry, c.kind)

        def cmp_block(entry, got, want, mask, bound):
            assert_exact(entry + " (padding)", c, got[~mask], np.full(int((~mask).sum()), SENT))
            if exact:
                assert_exact(entry, c, got[mask], want[mask])
            else:
                assert_bounded(tag(entry), c, got[mask], want[mask], bound)
            _count(entry, c.kind)

        if cmf:
            cmp_dout("nep_resid_batch_cm_dev", out["d_out"], ref["d_out"], slice(0, r0))
            if row0 >= 0:
                mask = np.zeros(len(ref["tail"]), bool)
                for j in range(k):
                    mask[j * a["ldt"]: j * a["ldt"] + n - r0] = True
                cmp_block("nep_resid_batch_cm_dev (tail)", out["tail"], ref["tail"], mask, Rb[r0:].T.reshape(-1))
            return 1
        if exact:
            assert_exact("nep_resid_batch (rnorm)", c, out["rnorm"], ref["rnorm"])
            assert_exact("nep_resid_batch (qnorm)", c, out["qnorm"], ref["qnorm"])
        else:
            sr = ref["rnorm"].astype(np.float64); sq_ = ref["qnorm"].astype(np.float64)
            tiny = np.finfo(np.float64).tiny
            assert_bounded(tag("nep_resid_batch"), c, out["rnorm"], ref["rnorm"], sq_bound(slice(0, n)) / np.maximum(sr, tiny) + 2 * U * sr)
            assert_bounded(tag("nep_resid_batch"), c, out["qnorm"], ref["qnorm"], qb / np.maximum(sq_, tiny) + 2 * U * sq_)
        _count("nep_resid_batch", c.kind)
        cmp_dout("nep_resid_batch_dev", out["d_out"], ref["d_out"], slice(0, n))
        cmp_dout("nep_resid_split_dev", out["split_out"], ref["split_out"], slice(0, r0))
        mask = np.zeros(len(ref["tail"]), bool)
        mask[:-1].reshape(n - r0, a["ldt"])[:, :k] = True
        cmp_block("nep_resid_split_dev (tail)", out["tail"], ref["tail"], mask, Rb[r0:].reshape(-1))
        assert out["block_status"] == ref["block_status"], "nep_resid_block %r: status %d, want %d" % (c, out["block_status"], ref["block_status"])
        if ref["block_status"] == 0:
            mask = np.zeros(len(ref["block"]), bool)
            mask.reshape(n, a["ldr"])[:, :k] = True
            cmp_block("nep_resid_block", out["block"], ref["block"], mask, Rb.reshape(-1))
        return 4
    if op == "k11":
        ma, mb = a["ma"], a["mb"]
        Wa = np.abs(cm_view(a["W"], 0, n, ma, a["ldw"])); Ba = np.abs(cm_view(a["B"], 0, n, mb, a["ldb"]))
        ta = np.abs(cm_view(a["tau"], 0, ma + mb, mt, a["ldt"]))
        Xs = [Ba @ np.array([[ta[i + j + 1, t] for i in range(mb)] for j in range(ma)]).reshape(ma, mb).T for t in range(mt)]
        S = float(np.sum(Wa * _absS(rec, Xs)))
        for key in ("c_host", "c_dev"):
            if exact:
                assert_below_2_53(2 * S)
                assert_exact("nep_lr_hankel (%s)" % key, c, np.array([out[key]]), np.array([ref[key]]))
            else:
                N = n + ma * mb + int(rec.L.max())
                assert_bounded(tag("nep_lr_hankel"), c, np.array([out[key]]), np.array([ref[key]]), 2 * gamma(N) * S)
            _count("nep_lr_hankel", c.kind)
        assert np.array([out["c_host"]]).view(np.float64).tolist() == np.array([out["c_dev"]]).view(np.float64).tolist(), \
            "nep_lr_hankel %r: h_c and d_c differ" % (c,)
        return 2
    if op == "cw":
        xa = np.abs(a["x"])
        Sx = _absS(rec, [(xa * a["cabs"][t])[:, None] for t in range(mt)])[:, 0]
        den = _cw_den(rec, a)
        Lr = np.maximum(rec.L, 1)
        for fused, rk, ok in ((True, "r_fused", "om_fused"), (False, "r_mx", "om_mx")):
            entry = "nep_cw_backward_error (%s)" % ("fused" if fused else "dMx")
            rref = ref[rk]
            if fused:
                S = np.abs(a["b"]) + Sx
                rb = cbound_n(Lr, S)
            else:
                S = np.abs(a["b"]) + np.abs(a["Mx"])
                rb = SQ2 * gamma(2) * S
            if exact:
                assert_below_2_53(2 * S)
                assert_exact(entry + " r", c, out[rk], rref)
                rb = np.zeros(n)
            else:
                assert_bounded(tag(entry + " r"), c, out[rk], rref, rb)
            num = np.abs(rref).astype(np.float64)
            g = np.array([gamma(int(l) + 16) for l in Lr])
            safe = np.where(den > 0, den, 1.0)
            ob = np.where(den > 0, ((rb + 3 * U * num) / safe + num / safe * g) * (1 + g), 0.0)
            assert_bounded(tag(entry + " omega"), c, np.array([out[ok]]), np.array([ref[ok]]), float(ob.max()) + np.finfo(np.float64).tiny)
            _count(entry, c.kind)
        return 2
    raise ValueError(op)


# ================================================================================================================================
# nep_csc_to_csr (host only)
def csc_to_csr_cases():
    """(n, colptr int64, rowval int64, nzval, one_based) with empty columns, real and complex values"""
    for n in (1, 7, 200):
        for cplx in (False, True):
            for one in (0, 1):
                rng = np.random.default_rng(_seed("csc%d%d%d" % (n, cplx, one)))
                A = sp.random(n, n, density=min(1.0, 3.0 / n), random_state=int(rng.integers(1 << 30)), format="csc")
                A.data = _vals(rng, A.nnz, "exact", cplx)
                if n > 3:
                    A = sp.csc_matrix(A @ sp.diags(np.where(np.arange(n) % 5 == 2, 0.0, 1.0)))                  # empty columns
                    A.eliminate_zeros()
                A.sort_indices()
                yield n, (A.indptr + one).astype(np.int64), (A.indices + one).astype(np.int64), np.ascontiguousarray(A.data), cplx, one, A


def check_csc_to_csr(lib, case):
    n, colptr, rowval, nzval, cplx, one, A = case
    nnz = len(rowval)
    rp = np.full(n + 1, -7, dtype=np.int32); ci = np.full(nnz + 1, -7, dtype=np.int32)
    vals = np.full(nnz + 1, SENT if cplx else -7.25e77, dtype=C128 if cplx else np.float64)
    vp = lambda x: x.ctypes.data_as(C.c_void_p)
    rc = lib.nep_csc_to_csr(n, vp(colptr), vp(rowval), vp(nzval), int(cplx), one, vp(rp), vp(ci), vp(vals))
    assert rc == 0, rc
    R = sp.csr_matrix(A); R.sort_indices()
    assert_exact("nep_csc_to_csr rowptr", case[:1], rp, R.indptr.astype(np.int32))
    assert ci[nnz] == -7 and vals[nnz] == (SENT if cplx else -7.25e77)
    for r in range(n):                                       # the order inside a row is not part of the contract
        o = np.argsort(ci[rp[r]: rp[r + 1]], kind="stable")
        assert_exact("nep_csc_to_csr colind", (n, r), ci[rp[r]: rp[r + 1]][o], R.indices[R.indptr[r]: R.indptr[r + 1]].astype(np.int32))
        assert_exact("nep_csc_to_csr vals", (n, r), vals[rp[r]: rp[r + 1]][o], R.data[R.indptr[r]: R.indptr[r + 1]])
    _count("nep_csc_to_csr", "exact")
