"""References, error bounds and case lists for the C-ABI primitives of include/nepmi355.h that only drivers reach.

One `Prim` per entry point.  Its `check(impl, case)` runs `impl` on the operands of `case` and compares the result with a plain
reference.  `impl` has the argument list of the C function with flat complex128 NumPy buffers (plus element offsets) in place of
device pointers and returns fresh arrays; test_gpu_primitives.py passes adapters that upload the buffers and call the library,
test_host_primitive_checkers.py passes the float64 NumPy implementations `Prim.ref` and their mutants (`ref(..., mut=name)`).

Two kinds of case:
  exact    operands are Gaussian integers, every product and partial sum is an integer below 2^53 (asserted per case from the
           operand magnitudes), so the result is the same in any summation order, with or without fused multiply-adds: the
           comparison is np.array_equal.
  rounded  random complex operands, reference in np.clongdouble (64-bit mantissa), assertion |impl - ref| <= cbound(N, S).
"""
from functools import partial

import numpy as np

U = 2.0 ** -53
SQ2 = float(np.sqrt(2.0))
C128, CLD = np.complex128, np.clongdouble
NAN = complex(np.nan, np.nan)
SENT = complex(-7.25e77, 3.5e-66)              # sentinel for padding that must survive a call
RATIOS = {}                                    # primitive -> largest |impl - ref| / bound seen in its rounded cases


def gamma(n):
    assert n * U < 0.01
    return n * U / (1.0 - n * U)


def cbound(nterms, S):
    """Bound on |computed - exact| for a complex result that is a sum of `nterms` complex products (any summation order, with or
    without FMA contraction, vector ALU or FP64 matrix core), S being the same expression with every operand replaced by its
    absolute value (sum |x_i| |y_i|, |alpha| |x| + |y|, ...).

    Real and imaginary part are real sums of 2 nterms products each, so each is off by at most gamma_{2 nterms} times its sum of
    absolute values (Higham, Accuracy and Stability, (3.5); a fused multiply-add only removes roundings), and that sum is at most
    S because |xr yr| + |xi yi| <= |x| |y|.  Two components: sqrt(2) gamma_{2 nterms} S.  Six further roundings are allowed for a
    scale factor applied to the sum, a second scaled operand added to it and the final addition.  In the form c gamma_N S this
    is c = 2 sqrt(2) (1 + O(N u)): the constant 2 sqrt(2) of one complex multiply-add.  Nothing is fitted to a device result."""
    return SQ2 * gamma(2 * nterms + 6) * np.asarray(S, dtype=np.float64)


class Case:
    """one call: `build()` makes the operands when the case runs (listing the cases costs nothing)"""

    def __init__(self, group, cid, kind, build, host=True, extra=None):
        self.group, self.cid, self.kind, self.build, self.host = group, cid, kind, build, host
        self.extra = extra or {}

    @property
    def args(self):
        return self.build()

    def __repr__(self):
        return "%s/%s[%s]" % (self.group, self.cid, self.kind)


def _seed(s):
    return sum((i + 1) * ord(ch) for i, ch in enumerate(s)) % (1 << 30)


def gint(rng, shape, lo=-8, hi=8):
    return (rng.integers(lo, hi + 1, shape) + 1j * rng.integers(lo, hi + 1, shape)).astype(C128)


def grand(rng, shape):
    return (rng.standard_normal(shape) + 1j * rng.standard_normal(shape)).astype(C128)


def operand(kind, rng, shape):
    return gint(rng, shape) if kind == "exact" else grand(rng, shape)


def colmajor_buf(M, ld, fill=NAN, lead=0, trail=0):
    """rows x k matrix -> flat column-major buffer with leading dimension ld (padding = fill), `lead` elements in front"""
    rows, k = M.shape
    buf = np.full(lead + max(ld * (k - 1) + rows, 0) + (ld - rows if ld >= rows else 0) + trail, fill, dtype=C128)
    for j in range(k):
        buf[lead + j * ld: lead + j * ld + rows] = M[:, j]
    return buf


def rowmajor_buf(M, ld, fill=NAN, lead=0, trail=0):
    rows, k = M.shape
    buf = np.full(lead + rows * ld + trail, fill, dtype=C128)
    buf[lead: lead + rows * ld].reshape(rows, ld)[:, :k] = M
    return buf


def cm_view(buf, off, rows, k, ld):
    """rows x k view of a column-major block inside a flat buffer (ld = 0: one column repeated)"""
    return np.lib.stride_tricks.as_strided(buf[off:], shape=(rows, k), strides=(buf.itemsize, ld * buf.itemsize), writeable=False) \
        if ld * (k - 1) + rows <= len(buf) - off else _fail("block outside its buffer")


def rm_view(buf, off, rows, k, ld):
    return np.lib.stride_tricks.as_strided(buf[off:], shape=(rows, k), strides=(ld * buf.itemsize, buf.itemsize), writeable=False) \
        if (rows - 1) * ld + k <= len(buf) - off else _fail("block outside its buffer")


def _fail(msg):
    raise AssertionError(msg)


def drop_tail(rows, q):
    """rows a kernel processes when it forgets the block behind the last multiple of q"""
    return rows if rows % q == 0 else rows // q * q


def perturb(out):
    """one result off by 1e-13 relative (or absolute, where it is zero)"""
    out = np.array(out, copy=True)
    flat = out.reshape(-1)
    if flat.size:
        i = flat.size // 2
        flat[i] = flat[i] * (1 + 1e-13) if flat[i] != 0 else 1e-13
    return out


def assert_exact(name, c, got, want):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, (name, c, got.shape, want.shape)
    if not np.array_equal(got, want, equal_nan=True):
        g, w = got.reshape(-1), want.reshape(-1)
        bad = np.flatnonzero(~((g == w) | (np.isnan(g) & np.isnan(w))))
        i = int(bad[0])
        raise AssertionError("%s %r: %d of %d entries differ, first at %d: got %r, want %r"
                             % (name, c, bad.size, want.size, i, got.reshape(-1)[i], want.reshape(-1)[i]))


def assert_bounded(name, c, got, ref, bound):
    got = np.asarray(got)
    ref = np.asarray(ref)
    bound = np.broadcast_to(np.asarray(bound, dtype=np.float64), ref.shape)
    assert got.shape == ref.shape, (name, c, got.shape, ref.shape)
    assert np.all(np.isfinite(got)), "%s %r: non-finite result" % (name, c)
    err = np.abs(got.astype(ref.dtype) - ref).astype(np.float64)
    tiny = np.finfo(np.float64).tiny
    ratio = float(np.max(err / np.maximum(bound, tiny))) if err.size else 0.0
    RATIOS[name] = max(RATIOS.get(name, 0.0), ratio)
    assert ratio <= 1.0, "%s %r: |impl - ref| / bound = %.3g (largest error %.3e)" % (name, c, ratio, float(err.max()))
    return ratio


def assert_below_2_53(S):
    S = np.asarray(S, dtype=np.float64)
    assert S.size == 0 or float(S.max()) < 2.0 ** 53, "the exact reference would not be exact: magnitude %.3g" % float(S.max())


class Prim:
    name = None
    mutants = ()
    exact_only_mutants = ("perturb",)

    def cases(self):
        raise NotImplementedError

    def ref(self, mut=None, **a):
        raise NotImplementedError

    def check(self, impl, c):
        raise NotImplementedError


# ================================================================================================================================
# column reductions: nep_coldots, nep_coldotsu, nep_colnorms, nep_nrm2
RED_ROWS = [1, 63, 64, 65, 255, 256, 257, 2047, 2048, 2049, 1048577, 3000017]
RED_K = [1, 2, 64, 65, 130]


def _red_shapes():
    out = [(r, k) for r in RED_ROWS for k in (1, 2)]
    out += [(r, k) for r in (1, 65, 257, 2049) for k in (64, 65, 130)]
    return out


class ColDots(Prim):
    """impl(rows, k, X, ldx, Y, ldy) -> k complex: d_j = x_j^H y_j (conj) or x_j^T y_j; Y may be the object X (same buffer)"""

    def __init__(self, conj):
        self.conj = conj
        self.name = "nep_coldots" if conj else "nep_coldotsu"
        self.mutants = ("drop_last", "drop_tail256", "conj_wrong", "ld_as_rows", "last_col_stale", "perturb")

    def cases(self):
        def build(rows, k, kind, edge=None):
            rng = np.random.default_rng(_seed("%s%d.%d%s%s" % (self.name, rows, k, kind, edge)))
            pad = 0 if rows > 100000 else 3
            X = operand(kind, rng, (rows, 1 if edge == "ldx0" else k)); Y = operand(kind, rng, (rows, k))
            if edge == "ldx0":                                  # one column against k columns (newton.py relies on it)
                return dict(rows=rows, k=k, X=colmajor_buf(X, rows), ldx=0, Y=colmajor_buf(Y, rows + 5), ldy=rows + 5)
            if edge == "same_buffer":
                Xb = colmajor_buf(Y, rows + 1)
                return dict(rows=rows, k=k, X=Xb, ldx=rows + 1, Y=Xb, ldy=rows + 1)
            return dict(rows=rows, k=k, X=colmajor_buf(X, rows + pad), ldx=rows + pad, Y=colmajor_buf(Y, rows + 2 * pad), ldy=rows + 2 * pad)

        for rows, k in _red_shapes():
            for kind in ["exact"] + (["rounded"] if rows <= 100000 else []):
                yield Case("rows%d" % rows, "k%d" % k, kind, partial(build, rows, k, kind), host=rows <= 1100000)
        for kind in ("exact", "rounded"):
            for edge in ("ldx0", "same_buffer"):
                yield Case("edges", edge, kind, partial(build, 2049, 65, kind, edge))

    def ref(self, rows, k, X, ldx, Y, ldy, mut=None, dt=C128):
        if mut == "ld_as_rows":
            ldx = rows if ldx else 0; ldy = rows
        r = rows - 1 if mut == "drop_last" else drop_tail(rows, 256) if mut == "drop_tail256" else rows
        Xm = cm_view(X, 0, rows, k, ldx)[:r].astype(dt); Ym = cm_view(Y, 0, rows, k, ldy)[:r].astype(dt)
        cx = self.conj != (mut == "conj_wrong")
        out = np.sum((np.conj(Xm) if cx else Xm) * Ym, axis=0)
        if mut == "last_col_stale":
            out[-1] = 0
        return perturb(out) if mut == "perturb" else out

    def check(self, impl, c):
        a = c.args
        got = impl(**a)
        S = np.sum(np.abs(cm_view(a["X"], 0, a["rows"], a["k"], a["ldx"])) * np.abs(cm_view(a["Y"], 0, a["rows"], a["k"], a["ldy"])), axis=0)
        if c.kind == "exact":
            assert_below_2_53(2 * S)
            assert_exact(self.name, c, got, self.ref(**a))
        else:
            assert_bounded(self.name, c, got, self.ref(dt=CLD, **a), cbound(a["rows"], S))


class ColNorms(Prim):
    """impl(rows, k, X, ldx) -> k doubles (nep_colnorms) / impl(len, x) -> one double (nep_nrm2).  The sum of squares runs through
    the same reduction as nep_coldots; sqrt is correctly rounded, so an exact integer sum gives np.sqrt of it, and a rounded one
    |s^ - s| <= gamma_{2 rows + 6} s, hence |sqrt(s^) - sqrt(s)| <= gamma_{2 rows + 6} sqrt(s) with the rounding of sqrt itself."""

    def __init__(self, nrm2):
        self.nrm2 = nrm2
        self.name = "nep_nrm2" if nrm2 else "nep_colnorms"
        self.mutants = ("drop_last", "drop_tail256", "perturb") + (() if nrm2 else ("ld_as_rows", "last_col_stale"))

    def cases(self):
        def build(rows, k, kind):
            rng = np.random.default_rng(_seed("%s%d.%d%s" % (self.name, rows, k, kind)))
            pad = 0 if (rows > 100000 or self.nrm2) else 3
            X = operand(kind, rng, (rows, k))
            if self.nrm2:
                return dict(len=rows, x=colmajor_buf(X, rows))
            return dict(rows=rows, k=k, X=colmajor_buf(X, rows + pad), ldx=rows + pad)

        for rows, k in _red_shapes():
            if self.nrm2 and k != 1:
                continue
            for kind in ["exact"] + (["rounded"] if rows <= 100000 else []):
                yield Case("rows%d" % rows, "k%d" % k, kind, partial(build, rows, k, kind), host=rows <= 1100000)

    def ref(self, mut=None, dt=C128, **a):
        if self.nrm2:
            rows, k, X, ldx = a["len"], 1, a["x"], a["len"]
        else:
            rows, k, X, ldx = a["rows"], a["k"], a["X"], a["ldx"]
        if mut == "ld_as_rows":
            ldx = rows
        r = rows - 1 if mut == "drop_last" else drop_tail(rows, 256) if mut == "drop_tail256" else rows
        Xm = cm_view(X, 0, rows, k, ldx)[:r]
        rt = np.longdouble if dt is CLD else np.float64
        s = np.sum(Xm.real.astype(rt) ** 2 + Xm.imag.astype(rt) ** 2, axis=0)
        out = np.sqrt(s)
        if mut == "last_col_stale":
            out[-1] = 0
        out = perturb(out) if mut == "perturb" else out
        return out[0] if self.nrm2 else out

    def check(self, impl, c):
        a = c.args
        got = np.atleast_1d(impl(**a))
        ref = np.atleast_1d(self.ref(dt=C128 if c.kind == "exact" else CLD, **a))
        if c.kind == "exact":
            assert_below_2_53(ref.astype(np.float64) ** 2)
            assert_exact(self.name, c, got, ref)
        else:
            rows = a["len"] if self.nrm2 else a["rows"]
            assert_bounded(self.name, c, got, ref, gamma(2 * rows + 6) * ref.astype(np.float64))


class RowMajorColNorms(Prim):
    """impl(rows, k, XT, ld) -> k doubles: column 2-norms of a row-major block"""
    name = "nep_rowmajor_colnorms"
    mutants = ("drop_last", "drop_tail64_cols", "ld_as_k", "last_col_stale", "drop_phase", "perturb")

    def cases(self):
        shapes = [(r, k) for r in (1, 3, 4, 5, 4095, 4096, 4097) for k in (1, 63, 64, 65, 128, 130, 200)]
        shapes += [(200003, 1), (200003, 65), (200003, 130)]
        def build(rows, k, kind):
            rng = np.random.default_rng(_seed("rmcn%d.%d%s" % (rows, k, kind)))
            pad = 0 if (rows, k) == (4096, 64) else 3
            return dict(rows=rows, k=k, XT=rowmajor_buf(operand(kind, rng, (rows, k)), k + pad), ld=k + pad)

        for rows, k in shapes:
            for kind in ["exact"] + (["rounded"] if rows <= 100000 else []):
                yield Case("rows%d" % rows, "k%d" % k, kind, partial(build, rows, k, kind), host=rows * k < 2e7)

    def ref(self, rows, k, XT, ld, mut=None, dt=C128):
        if mut == "ld_as_k":
            ld = k
        Xm = rm_view(XT, 0, rows, k, ld)
        if mut == "drop_last":
            Xm = Xm[:rows - 1]
        if mut == "drop_phase":                              # one of the four row phases of a workgroup is never added
            Xm = Xm[np.arange(Xm.shape[0]) % 4 != 3]
        rt = np.longdouble if dt is CLD else np.float64
        s = np.sum(Xm.real.astype(rt) ** 2 + Xm.imag.astype(rt) ** 2, axis=0)
        out = np.sqrt(s)
        if mut == "drop_tail64_cols":                        # the column group behind the last multiple of 64 is never written
            out[drop_tail(k, 64):] = 0
        if mut == "last_col_stale":
            out[-1] = 0
        return perturb(out) if mut == "perturb" else out

    def check(self, impl, c):
        a = c.args
        got = impl(**a)
        ref = self.ref(dt=C128 if c.kind == "exact" else CLD, **a)
        if c.kind == "exact":
            assert_below_2_53(ref.astype(np.float64) ** 2)
            assert_exact(self.name, c, got, ref)
        else:
            assert_bounded(self.name, c, got, ref, gamma(2 * a["rows"] + 6) * ref.astype(np.float64))


# ================================================================================================================================
class RowMajorToColMajor(Prim):
    """impl(rows, k, src, lds, cols, ncols, dst, ldd) -> (status, dst'): dst'[:, i] = src[:, cols[i]] (cols None: all k columns)"""
    name = "nep_rowmajor_to_colmajor"
    mutants = ("drop_last", "drop_tail64", "gather_ignored", "ld_as_rows", "last_col_stale", "perturb", "pad_clobbered")
    exact_only_mutants = ()

    def cases(self):
        def build(rows, k, cid):
            rng = np.random.default_rng(_seed("rm2cm%d.%d" % (rows, k)))
            M = gint(rng, (rows, k))
            perm = rng.permutation(k)[:max(1, (2 * k) // 3)].astype(np.int32)
            rep = rng.integers(0, k, k + 3).astype(np.int32)
            cols, ncols = dict(all=(None, k), perm=(perm, len(perm)), repeat=(rep, len(rep)), none=(perm, 0),
                               badcol=(np.append(perm, k).astype(np.int32), len(perm) + 1),
                               negcol=(np.append(perm, -1).astype(np.int32), len(perm) + 1))[cid]
            lds, ldd = k + 2, rows + 3
            dst = np.full(ldd * max(ncols, 1) + 5, SENT, dtype=C128)
            return dict(rows=rows, k=k, src=rowmajor_buf(M, lds), lds=lds, cols=cols, ncols=ncols, dst=dst, ldd=ldd)

        for rows in (1, 63, 64, 65, 1000):
            for k in (1, 15, 16, 17, 100):
                for cid in ("all", "perm", "repeat", "none", "badcol", "negcol"):
                    yield Case("rows%d" % rows, "k%d_%s" % (k, cid), "exact", partial(build, rows, k, cid))

    def ref(self, rows, k, src, lds, cols, ncols, dst, ldd, mut=None, dt=C128):
        out = dst.copy()
        if cols is None:
            ncols = k
        sel = np.arange(k) if cols is None else np.asarray(cols[:ncols])
        if sel.size and (sel.min() < 0 or sel.max() >= k):
            return -2, out
        if mut == "gather_ignored":
            sel = np.arange(ncols) % k
        if mut == "ld_as_rows":
            lds, ldd = k, rows
        S = rm_view(src, 0, rows, k, lds)
        r = rows - 1 if mut == "drop_last" else drop_tail(rows, 64) if mut == "drop_tail64" else rows
        nc = ncols - 1 if mut == "last_col_stale" else ncols
        for i in range(nc):
            out[i * ldd: i * ldd + r] = S[:r, sel[i]]
        if mut == "pad_clobbered" and ncols:
            out[rows if ldd > rows else 0] = 0
        if mut == "perturb" and ncols:
            out[:rows] = perturb(out[:rows])
        return 0, out

    def check(self, impl, c):
        a = c.args
        st, got = impl(**a)
        st_ref, want = self.ref(**a)
        assert st == st_ref, "%s %r: status %d, want %d" % (self.name, c, st, st_ref)
        assert_exact(self.name, c, got, want)


# ================================================================================================================================
ELT_ROWS = [1, 255, 256, 257, 100003]
ELT_K = [1, 2, 7, 60]


class RowDot(Prim):
    """impl(rows, k, A, lda, B, ldb) -> rows complex: out[r] = sum_j A[r, j] B[r, j] (no conjugation)"""
    name = "nep_rowdot"
    mutants = ("drop_last", "drop_tail256", "conj_wrong", "ld_as_rows", "last_col_dropped", "perturb")

    def cases(self):
        def build(rows, k, kind):
            rng = np.random.default_rng(_seed("rowdot%d.%d%s" % (rows, k, kind)))
            A = operand(kind, rng, (rows, k)); B = operand(kind, rng, (rows, k))
            lda, ldb = rows + 1, 2 * rows + 3                      # the waveguide caller passes ldb = 2 nz
            return dict(rows=rows, k=k, A=colmajor_buf(A, lda), lda=lda, B=colmajor_buf(B, ldb), ldb=ldb)

        for rows in ELT_ROWS:
            for k in ELT_K:
                for kind in ("exact", "rounded"):
                    yield Case("rows%d" % rows, "k%d" % k, kind, partial(build, rows, k, kind))

    def ref(self, rows, k, A, lda, B, ldb, mut=None, dt=C128):
        if mut == "ld_as_rows":
            lda = ldb = rows
        Am = cm_view(A, 0, rows, k, lda).astype(dt); Bm = cm_view(B, 0, rows, k, ldb).astype(dt)
        kk = k - 1 if mut == "last_col_dropped" else k
        out = np.sum((np.conj(Am) if mut == "conj_wrong" else Am)[:, :kk] * Bm[:, :kk], axis=1)
        r = rows - 1 if mut == "drop_last" else drop_tail(rows, 256) if mut == "drop_tail256" else rows
        out[r:] = 0
        return perturb(out) if mut == "perturb" else out

    def check(self, impl, c):
        a = c.args
        got = impl(**a)
        S = np.sum(np.abs(cm_view(a["A"], 0, a["rows"], a["k"], a["lda"])) * np.abs(cm_view(a["B"], 0, a["rows"], a["k"], a["ldb"])), axis=1)
        if c.kind == "exact":
            assert_below_2_53(2 * S)
            assert_exact(self.name, c, got, self.ref(**a))
        else:
            assert_bounded(self.name, c, got, self.ref(dt=CLD, **a), cbound(a["k"], S))


class Hadamard(Prim):
    """impl(rows, k, A, lda, B, ldb) -> A' (whole buffer): A[r, j] *= B[r, j]; B may be the object A (squares in place)"""
    name = "nep_hadamard"
    mutants = ("drop_last", "drop_tail256", "conj_wrong", "ld_as_rows", "last_col_stale", "perturb", "pad_clobbered")

    def cases(self):
        def build(rows, k, kind, same=False):
            rng = np.random.default_rng(_seed("hadamard%d.%d%s" % (rows, k, kind)))
            A = operand(kind, rng, (rows, k)); B = operand(kind, rng, (rows, k))
            lda, ldb = rows + 2, 2 * rows + 1
            Ab = colmajor_buf(A, lda, fill=SENT)
            if same:
                return dict(rows=rows, k=k, A=Ab, lda=lda, B=Ab, ldb=lda)
            return dict(rows=rows, k=k, A=Ab, lda=lda, B=colmajor_buf(B, ldb), ldb=ldb)

        for rows, k in [(r, k) for r in ELT_ROWS for k in ELT_K] + [(4096 * 256 + 1, 1)]:
            for kind in ("exact", "rounded"):
                yield Case("rows%d" % rows, "k%d" % k, kind, partial(build, rows, k, kind))
        for kind in ("exact", "rounded"):
            yield Case("edges", "same_buffer", kind, partial(build, 257, 7, kind, True))

    def ref(self, rows, k, A, lda, B, ldb, mut=None, dt=C128):
        out = A.astype(dt)
        l_a, l_b = (rows, rows) if mut == "ld_as_rows" else (lda, ldb)
        r = rows - 1 if mut == "drop_last" else drop_tail(rows, 256) if mut == "drop_tail256" else rows
        for j in range(k - 1 if mut == "last_col_stale" else k):
            b = B[j * l_b: j * l_b + r].astype(dt)
            out[j * l_a: j * l_a + r] = A[j * l_a: j * l_a + r].astype(dt) * (np.conj(b) if mut == "conj_wrong" else b)
        if mut == "pad_clobbered":
            out[rows] = 0
        if mut == "perturb":
            out[:rows] = perturb(out[:rows])
        return out

    def check(self, impl, c):
        a = c.args
        got = impl(**a)
        pad = np.ones(len(a["A"]), bool)
        for j in range(a["k"]):
            pad[j * a["lda"]: j * a["lda"] + a["rows"]] = False
        assert_exact(self.name + " (padding)", c, got[pad], a["A"][pad])
        if c.kind == "exact":
            assert_below_2_53(2 * np.abs(a["A"][~pad]).max() * np.abs(cm_view(a["B"], 0, a["rows"], a["k"], a["ldb"])).max())
            assert_exact(self.name, c, got[~pad], self.ref(**a)[~pad])
        else:
            ref = self.ref(dt=CLD, **a)[~pad]
            S = np.abs(a["A"][~pad]) * np.abs(cm_view(a["B"], 0, a["rows"], a["k"], a["ldb"]).T.reshape(-1))
            assert_bounded(self.name, c, got[~pad], ref, cbound(1, S))


# ================================================================================================================================
VEC_LENS = [0, 1, 255, 256, 257, 4096 * 256 + 1]
ALPHAS = [0.0, 1.0, -1.0, 0.3 - 0.7j]


class Axpy(Prim):
    """impl(len, alpha, x, y) -> y': y += alpha x on the first len entries"""
    name = "nep_axpy"
    mutants = ("drop_last", "drop_tail256", "conj_wrong", "alpha_ignored", "perturb", "pad_clobbered")

    def cases(self):
        for n in VEC_LENS:
            for kind, alphas in (("exact", [0.0, 1.0, -1.0, 3 - 2j]), ("rounded", ALPHAS)):
                for al in alphas:
                    yield Case("len%d" % n, "alpha%s" % al, kind, partial(self._build, n, al, kind))

    @staticmethod
    def _build(n, al, kind):
        rng = np.random.default_rng(_seed("axpy%d%s%s" % (n, al, kind)))
        x = operand(kind, rng, n); y = np.concatenate([operand(kind, rng, n), [SENT, SENT]])
        return dict(len=n, alpha=complex(al), x=np.concatenate([x, [NAN]]), y=y)

    def ref(self, len, alpha, x, y, mut=None, dt=C128):
        n = len
        out = y.astype(dt)
        r = max(n - 1, 0) if mut == "drop_last" else drop_tail(n, 256) if mut == "drop_tail256" else n
        al = dt(1.0) if mut == "alpha_ignored" else dt(alpha)
        xs = x[:r].astype(dt)
        out[:r] = out[:r] + al * (np.conj(xs) if mut == "conj_wrong" else xs)
        if mut == "pad_clobbered":
            out[n] = 0
        if mut == "perturb":
            out[:n] = perturb(out[:n])
        return out

    def check(self, impl, c):
        a = c.args
        n = a["len"]
        got = impl(**a)
        assert_exact(self.name + " (padding)", c, got[n:], a["y"][n:])
        if c.kind == "exact":
            assert_exact(self.name, c, got[:n], self.ref(**a)[:n])
        else:
            S = abs(a["alpha"]) * np.abs(a["x"][:n]) + np.abs(a["y"][:n])
            assert_bounded(self.name, c, got[:n], self.ref(dt=CLD, **a)[:n], cbound(1, S))


class Scal(Prim):
    """impl(len, alpha, x) -> x': x *= alpha on the first len entries"""
    name = "nep_scal"
    mutants = ("drop_last", "drop_tail256", "conj_wrong", "perturb", "pad_clobbered")

    def cases(self):
        for n in VEC_LENS:
            for kind, alphas in (("exact", [0.0, 1.0, -1.0, 3 - 2j]), ("rounded", ALPHAS)):
                for al in alphas:
                    yield Case("len%d" % n, "alpha%s" % al, kind, partial(self._build, n, al, kind))

    @staticmethod
    def _build(n, al, kind):
        rng = np.random.default_rng(_seed("scal%d%s%s" % (n, al, kind)))
        return dict(len=n, alpha=complex(al), x=np.concatenate([operand(kind, rng, n), [SENT, SENT]]))

    def ref(self, len, alpha, x, mut=None, dt=C128):
        n = len
        out = x.astype(dt)
        r = max(n - 1, 0) if mut == "drop_last" else drop_tail(n, 256) if mut == "drop_tail256" else n
        out[:r] = dt(alpha) * (np.conj(out[:r]) if mut == "conj_wrong" else out[:r])
        if mut == "pad_clobbered":
            out[n] = 0
        if mut == "perturb":
            out[:n] = perturb(out[:n])
        return out

    def check(self, impl, c):
        a = c.args
        n = a["len"]
        got = impl(**a)
        assert_exact(self.name + " (padding)", c, got[n:], a["x"][n:])
        if c.kind == "exact":
            # (-0.0 == 0.0 under array_equal: the sign of a zero product is not part of the contract)
            assert_exact(self.name, c, got[:n], self.ref(**a)[:n])
        else:
            assert_bounded(self.name, c, got[:n], self.ref(dt=CLD, **a)[:n], cbound(1, abs(a["alpha"]) * np.abs(a["x"][:n])))


HYPOT_ULP = 2        # assumption: no accuracy figure for the device library's double hypot is available offline; 2 ulp is taken


class AbsVec(Prim):
    """impl(len, x) -> len results and the two entries behind them: out[i] = (|x[i]|, 0), computed with hypot.  Exact cases: integer
    entries with one zero component, where |x| is the other component.  Rounded cases: |out - |x|| <= HYPOT_ULP ulp against sqrt in
    extended precision, one ulp being at most 2 u |x| (HYPOT_ULP = 2 is an assumption, see above); magnitudes 1e-150 .. 1e150."""
    name = "nep_absvec"
    mutants = ("drop_last", "drop_tail256", "imag_kept", "real_only", "perturb", "pad_clobbered")

    def cases(self):
        def build(n, kind):
            rng = np.random.default_rng(_seed("absvec%d" % n))
            if kind == "exact":
                v = rng.integers(-8, 9, n).astype(np.float64)
                v[v == 0] = 3.0
                return dict(len=n, x=np.where(rng.integers(0, 2, n) == 0, v + 0j, 1j * v).astype(C128))
            return dict(len=n, x=grand(rng, n) * (10.0 ** rng.integers(-150, 150, n) if n > 1 else 1.0))

        for n in VEC_LENS[1:]:
            yield Case("len%d" % n, "axes", "exact", partial(build, n, "exact"))
            yield Case("len%d" % n, "random", "rounded", partial(build, n, "rounded"))

    def ref(self, len, x, mut=None, dt=C128):
        n = len
        rt = np.longdouble if dt is CLD else np.float64
        m = np.sqrt(x.real.astype(rt) ** 2 + x.imag.astype(rt) ** 2) if dt is CLD else np.hypot(x.real, x.imag)
        if mut == "real_only":
            m = np.abs(x.real.astype(rt))
        out = np.concatenate([m.astype(dt), [dt(SENT)] * 2])
        if mut == "imag_kept":
            out[:n] = m + 1j * x.imag
        r = n - 1 if mut == "drop_last" else drop_tail(n, 256) if mut == "drop_tail256" else n
        out[r:n] = dt(SENT)
        if mut == "pad_clobbered":
            out[n] = 0
        if mut == "perturb":
            out[:n] = perturb(out[:n])
        return out

    def check(self, impl, c):
        a = c.args
        n = a["len"]
        got = impl(**a)                                          # n results + 2 entries of padding the adapter put behind them
        assert_exact(self.name + " (padding)", c, got[n:], np.array([SENT, SENT]))
        assert_exact(self.name + " (imaginary part)", c, got[:n].imag, np.zeros(n))
        if c.kind == "exact":
            assert_exact(self.name, c, got[:n], self.ref(**a)[:n])
        else:
            ref = self.ref(dt=CLD, **a)[:n]
            assert_bounded(self.name, c, got[:n], ref, HYPOT_ULP * 2 * U * np.abs(ref).astype(np.float64))


class IarShiftScale(Prim):
    """impl(n, k, buf, src_off, dst_off) -> buf': buf[dst_off + (j + 1) n + r] = buf[src_off + j n + r] / (j + 1), j < k.  The
    library multiplies by the rounded reciprocal 1 / (j + 1): the exact cases compare with x * (1.0 / (j + 1)) (one rounding of
    an integer times the same double on both sides), the rounded ones with x / (j + 1) under two roundings per component."""
    name = "nep_iar_shift_scale"
    mutants = ("drop_last", "drop_tail256", "no_shift", "scale_off_by_one", "perturb", "pad_clobbered")

    def cases(self):
        def build(n, k, kind, contiguous=False):
            rng = np.random.default_rng(_seed("iss%d.%d%s" % (n, k, kind)))
            ldv = n * k if contiguous else n * (k + 1) + 3       # iar: column k - 1 of V -> column k (rows n .. n (k + 1))
            buf = np.full(ldv + n * (k + 1) + 3, SENT, dtype=C128)
            buf[:n * k] = operand(kind, rng, n * k)
            return dict(n=n, k=k, buf=buf, src_off=0, dst_off=ldv)

        for n, k in ((1, 1), (1, 255), (255, 1), (64, 4), (257, 1), (85, 3), (9, 0), (4097, 256)):
            for kind in ("exact", "rounded"):
                yield Case("n%d" % n, "k%d" % k, kind, partial(build, n, k, kind))
        for kind in ("exact", "rounded"):                             # destination right behind the source in one allocation
            yield Case("edges", "contiguous", kind, partial(build, 100, 7, kind, True))

    def ref(self, n, k, buf, src_off, dst_off, mut=None, dt=C128):
        out = buf.astype(dt)
        rt = np.longdouble if dt is CLD else np.float64
        tot = n * k
        r = max(tot - 1, 0) if mut == "drop_last" else drop_tail(tot, 256) if mut == "drop_tail256" else tot
        j = (np.arange(tot) // n + (2 if mut == "scale_off_by_one" else 1)).astype(rt)
        src = buf[src_off: src_off + tot].astype(dt)
        val = src / j if dt is CLD else src * (1.0 / j)
        sh = 0 if mut == "no_shift" else n
        out[dst_off + sh: dst_off + sh + r] = val[:r]
        if mut == "pad_clobbered":
            out[dst_off] = 0
        if mut == "perturb":
            out[dst_off + n: dst_off + n + tot] = perturb(out[dst_off + n: dst_off + n + tot])
        return out

    def check(self, impl, c):
        a = c.args
        got = impl(**a)
        lo, hi = a["dst_off"] + a["n"], a["dst_off"] + a["n"] * (a["k"] + 1)
        keep = np.ones(len(got), bool); keep[lo:hi] = False
        assert_exact(self.name + " (outside the destination)", c, got[keep], a["buf"][keep])
        if c.kind == "exact":
            assert_exact(self.name, c, got[lo:hi], self.ref(**a)[lo:hi])
        else:
            ref = self.ref(dt=CLD, **a)[lo:hi]
            assert_bounded(self.name, c, got[lo:hi], ref, SQ2 * gamma(2) * np.abs(ref).astype(np.float64))


# ================================================================================================================================
RK_N = [1, 257, 9956]
RK_NN = [0, 1, 2, 43, 100]


class RkBw(Prim):
    """impl(n, N, wc, wc_off, c, Bw, bw_off) -> Bw': Bw[0:n] = 0, Bw[i n + r] = wc[(i - 1) n + r] + c[i - 1] wc[i n + r], i = 1..N"""
    name = "nep_rk_bw"
    mutants = ("drop_last", "drop_tail256", "conj_wrong", "first_block_not_zeroed", "coef_shifted", "perturb", "pad_clobbered")

    def cases(self):
        shapes = [(n, N, 0) for n in RK_N for N in RK_NN] + [(84, 41, 2 * 257)]      # low-rank split: r-row blocks behind 2 n-row blocks
        def build(n, N, off, kind):
            rng = np.random.default_rng(_seed("rkbw%d.%d%s" % (n, N, kind)))
            wc = np.concatenate([np.full(off, NAN), operand(kind, rng, n * (N + 1)), [NAN]])
            Bw = np.full(off + n * (N + 1) + 2, SENT, dtype=C128)
            return dict(n=n, N=N, wc=wc, wc_off=off, c=operand(kind, rng, N), Bw=Bw, bw_off=off)

        for n, N, off in shapes:
            for kind in ("exact", "rounded"):
                yield Case("n%d" % n, "N%d_off%d" % (N, off), kind, partial(build, n, N, off, kind))

    def ref(self, n, N, wc, wc_off, c, Bw, bw_off, mut=None, dt=C128):
        out = Bw.astype(dt)
        w = wc[wc_off: wc_off + n * (N + 1)].astype(dt).reshape(N + 1, n)
        cc = np.asarray(c).astype(dt)
        if mut == "coef_shifted" and N > 1:
            cc = np.roll(cc, 1)
        if mut == "conj_wrong":
            cc = np.conj(cc)
        res = np.zeros((N + 1, n), dtype=dt)
        res[1:] = w[:-1] + cc[:, None] * w[1:]
        res = res.reshape(-1)
        tot = n * (N + 1)
        r = tot - 1 if mut == "drop_last" else drop_tail(tot, 256) if mut == "drop_tail256" else tot
        lo = n if mut == "first_block_not_zeroed" else 0
        out[bw_off + lo: bw_off + r] = res[lo:r]
        if mut == "pad_clobbered":
            out[bw_off + tot] = 0
        if mut == "perturb":
            out[bw_off: bw_off + tot] = perturb(out[bw_off: bw_off + tot])
        return out

    def check(self, impl, c):
        a = c.args
        got = impl(**a)
        n, N, off = a["n"], a["N"], a["bw_off"]
        lo, hi = off, off + n * (N + 1)
        keep = np.ones(len(got), bool); keep[lo:hi] = False
        assert_exact(self.name + " (outside the destination)", c, got[keep], a["Bw"][keep])
        if c.kind == "exact":
            assert_exact(self.name, c, got[lo:hi], self.ref(**a)[lo:hi])
        else:
            w = np.abs(a["wc"][a["wc_off"]: a["wc_off"] + n * (N + 1)]).reshape(N + 1, n)
            S = np.zeros((N + 1, n)); S[1:] = w[:-1] + np.abs(a["c"])[:, None] * w[1:]
            assert_bounded(self.name, c, got[lo:hi], self.ref(dt=CLD, **a)[lo:hi], cbound(1, S.reshape(-1)))


class BlockRecur(Prim):
    """impl(n, N, a, b, y, y_off, x, x_off) -> x': x_i = a[i-1] y_i + b[i-1] x_{i-1}, i = 1..N, blocks of n entries, x_0 given; y may
    be the object x with the same offset (in place).  Bound of the rounded cases, following the recurrence: with
    S_0 = |x_0|, S_i = |a_{i-1}| |y_i| + |b_{i-1}| S_{i-1} the error of block i is at most sqrt(2) gamma_{4 i + 2} S_i (two complex
    products and one addition per step: at most four roundings per component and step, and the error of x_{i-1} is carried
    through |b_{i-1}|, Higham (3.4) applied to the unrolled sum)."""
    name = "nep_block_recur"
    mutants = ("drop_last", "drop_tail256", "conj_wrong", "coef_swapped", "last_block_stale", "uses_y_prev", "perturb")

    def cases(self):
        shapes = [(n, N, 0) for n in RK_N for N in RK_NN] + [(84, 41, 2 * 257)]
        def build(n, N, off, kind, inplace):
            rng = np.random.default_rng(_seed("brec%d.%d%s%d" % (n, N, kind, inplace)))
            if kind == "exact":                                # |b| <= 1 keeps |x_i| <= |x_0| + 32 i: integers far below 2^53
                a = gint(rng, N, -2, 2)
                b = rng.choice(np.array([0, 1, -1, 1j, -1j]), N).astype(C128)
            else:
                a = grand(rng, N); b = grand(rng, N) * 0.7
            y = np.concatenate([np.full(off, SENT), operand(kind, rng, n * (N + 1)), [SENT]])
            x0 = operand(kind, rng, n)
            if inplace:
                y[off: off + n] = x0
                x = y
            else:
                y[off: off + n] = NAN                           # y_0 is never read
                x = np.full(off + n * (N + 1) + 1, SENT, dtype=C128)
                x[off: off + n] = x0
            return dict(n=n, N=N, a=a, b=b, y=y, y_off=off, x=x, x_off=off)

        for n, N, off in shapes:
            for inplace in (False, True):
                for kind in ("exact", "rounded"):
                    yield Case("n%d" % n, "N%d_off%d_%s" % (N, off, "inplace" if inplace else "outofplace"), kind,
                               partial(build, n, N, off, kind, inplace))

    def ref(self, n, N, a, b, y, y_off, x, x_off, mut=None, dt=C128):
        out = x.astype(dt)
        aa, bb = (np.asarray(b), np.asarray(a)) if mut == "coef_swapped" else (np.asarray(a), np.asarray(b))
        aa = aa.astype(dt); bb = bb.astype(dt)
        if mut == "conj_wrong":
            bb = np.conj(bb)
        r = n - 1 if mut == "drop_last" else drop_tail(n, 256) if mut == "drop_tail256" else n
        yb = y.astype(dt)
        prev = out[x_off: x_off + n].copy()
        for i in range(1, (N if mut == "last_block_stale" else N + 1)):
            yi = yb[y_off + i * n: y_off + (i + 1) * n]
            carry = yb[y_off + (i - 1) * n: y_off + i * n] if (mut == "uses_y_prev" and i > 1) else prev
            cur = aa[i - 1] * yi + bb[i - 1] * carry
            out[x_off + i * n: x_off + i * n + r] = cur[:r]
            prev = cur
        if mut == "perturb":
            out[x_off + n: x_off + n * (N + 1)] = perturb(out[x_off + n: x_off + n * (N + 1)])
        return out

    def bound_S(self, n, N, a, b, y, y_off, x, x_off):
        S = np.zeros((N + 1, n))
        S[0] = np.abs(x[x_off: x_off + n])
        for i in range(1, N + 1):
            S[i] = abs(a[i - 1]) * np.abs(y[y_off + i * n: y_off + (i + 1) * n]) + abs(b[i - 1]) * S[i - 1]
        return S

    def check(self, impl, c):
        a = c.args
        got = impl(**a)
        n, N, off = a["n"], a["N"], a["x_off"]
        lo, hi = off + n, off + n * (N + 1)
        keep = np.ones(len(got), bool); keep[lo:hi] = False
        assert_exact(self.name + " (outside the destination)", c, got[keep], a["x"][keep])
        S = self.bound_S(**a)
        if c.kind == "exact":
            assert_below_2_53(2 * S)
            assert_exact(self.name, c, got[lo:hi], self.ref(**a)[lo:hi])
        elif N:
            g = np.array([SQ2 * gamma(4 * i + 2) for i in range(1, N + 1)])[:, None]
            assert_bounded(self.name, c, got[lo:hi], self.ref(dt=CLD, **a)[lo:hi], (g * S[1:]).reshape(-1))


# ================================================================================================================================
class GemvH(Prim):
    """impl(V, ldv, rows, k, w) -> k complex: h = V^H w"""
    name = "nep_gemv_h"
    mutants = ("drop_last", "drop_tail256", "conj_wrong", "ld_as_rows", "last_col_stale", "perturb")

    def cases(self):
        for rows in (1, 64, 1000, 40000):
            for k in (1, 3, 64, 65, 130):
                for kind in ("exact", "rounded"):
                    yield Case("rows%d" % rows, "k%d" % k, kind, partial(self._build, rows, k, kind))

    @staticmethod
    def _build(rows, k, kind):
        rng = np.random.default_rng(_seed("gemvh%d.%d%s" % (rows, k, kind)))
        V = operand(kind, rng, (rows, k))
        return dict(V=colmajor_buf(V, rows + 5), ldv=rows + 5, rows=rows, k=k, w=np.concatenate([operand(kind, rng, rows), [NAN]]))

    def ref(self, V, ldv, rows, k, w, mut=None, dt=C128):
        if mut == "ld_as_rows":
            ldv = rows
        r = rows - 1 if mut == "drop_last" else drop_tail(rows, 256) if mut == "drop_tail256" else rows
        Vm = cm_view(V, 0, rows, k, ldv)[:r].astype(dt); ww = w[:r].astype(dt)
        out = (Vm.T @ np.conj(ww)) if mut == "conj_wrong" else np.sum(np.conj(Vm) * ww[:, None], axis=0)
        if mut == "last_col_stale":
            out[-1] = 0
        return perturb(out) if mut == "perturb" else out

    def check(self, impl, c):
        a = c.args
        got = impl(**a)
        S = np.abs(cm_view(a["V"], 0, a["rows"], a["k"], a["ldv"])).T @ np.abs(a["w"][:a["rows"]])
        if c.kind == "exact":
            assert_below_2_53(2 * S)
            assert_exact(self.name, c, got, self.ref(**a))
        else:
            assert_bounded(self.name, c, got, self.ref(dt=CLD, **a), cbound(a["rows"], S))


GTS_K = [1, 3, 4, 5, 61, 100]
GTS_P = [1, 8, 9, 16, 17, 32, 33, 48, 49, 64, 65, 80, 81, 104, 105, 130, 208, 209]
GTS_ROWS = [1, 15, 16, 17, 1000]
GTS_TALL = 524288 + 5


class GemmTsDev(Prim):
    """impl(Z, z_off, ldz, rows, k, B, b_off, ldb, b_rowmajor, p, Y, y_off, ldy, y_rowmajor) -> Y': Y = Z B with B a caller-owned
    device block in either layout; Z, B and Y are passed as offsets into larger allocations"""
    name = "nep_gemm_ts_dev"
    mutants = ("drop_last", "drop_tail16", "b_layout_swapped", "ld_as_min", "last_col_stale", "panel_seam", "conj_wrong", "perturb")

    def _case(self, rows, k, p, brm, yrm, kind, tag=""):
        return Case("b%d_y%d_p%d%s" % (brm, yrm, p, tag), "rows%d_k%d" % (rows, k), kind, partial(self._build, rows, k, p, brm, yrm, kind),
                    host=rows <= 100000)

    @staticmethod
    def _build(rows, k, p, brm, yrm, kind):
        rng = np.random.default_rng(_seed("gts%d.%d.%d.%d%d%s" % (rows, k, p, brm, yrm, kind)))
        Z = operand(kind, rng, (rows, k)); B = operand(kind, rng, (k, p))
        big = rows > 100000
        ldz = rows + (0 if big else 2)
        ldb = (p if brm else k) + 3
        ldy = (p if yrm else rows) + (0 if big else 1)
        z_off, b_off, y_off = (0, 5, 0) if big else (3, 5, 2)
        Zb = colmajor_buf(Z, ldz, lead=z_off, trail=1)
        Bb = rowmajor_buf(B, ldb, lead=b_off, trail=2) if brm else colmajor_buf(B, ldb, lead=b_off, trail=2)
        Yb = np.full(y_off + (rows * ldy if yrm else p * ldy) + 2, SENT, dtype=C128)
        return dict(Z=Zb, z_off=z_off, ldz=ldz, rows=rows, k=k, B=Bb, b_off=b_off, ldb=ldb, b_rowmajor=brm, p=p, Y=Yb, y_off=y_off,
                    ldy=ldy, y_rowmajor=yrm)

    def cases(self):
        for brm in (0, 1):
            for yrm in (0, 1):
                for p in GTS_P:
                    for k in GTS_K:
                        for rows in GTS_ROWS:
                            yield self._case(rows, k, p, brm, yrm, "exact")
                    yield self._case(1000, 61, p, brm, yrm, "rounded")
                    yield self._case(17, 100, p, brm, yrm, "rounded")
        for brm in (0, 1):                                     # the B-resident kernel of tall blocks, both layouts of B and of Y
            yield self._case(GTS_TALL, 16, 33, brm, brm, "exact", tag="_tall")
            yield self._case(GTS_TALL, 5, 16, brm, 1 - brm, "exact", tag="_tall")

    def ref(self, Z, z_off, ldz, rows, k, B, b_off, ldb, b_rowmajor, p, Y, y_off, ldy, y_rowmajor, mut=None, dt=C128):
        out = Y.astype(dt)
        if mut == "ld_as_min":
            ldb = p if b_rowmajor else k
        brm = b_rowmajor
        if mut == "b_layout_swapped" and (k - 1 if brm else p - 1) * ldb + (p if brm else k) <= len(B) - b_off - ldb:
            brm = not brm                                      # (where the other layout stays inside the allocation)
        Bm = np.array(rm_view(B, b_off, k, p, ldb) if brm else cm_view(B, b_off, k, p, ldb)).astype(dt)
        if mut == "conj_wrong":
            Bm = np.conj(Bm)
        if mut == "panel_seam" and p > 104:                    # second 104-column panel reads B from column 0 again
            Bm[:, 104:] = Bm[:, :p - 104]
        Zm = cm_view(Z, z_off, rows, k, ldz).astype(dt)
        R = Zm @ Bm
        r = rows - 1 if mut == "drop_last" else drop_tail(rows, 16) if mut == "drop_tail16" else rows
        pc = p - 1 if mut == "last_col_stale" else p
        if y_rowmajor:
            v = out[y_off: y_off + rows * ldy].reshape(rows, ldy)
            v[:r, :pc] = R[:r, :pc]
        else:
            for j in range(pc):
                out[y_off + j * ldy: y_off + j * ldy + r] = R[:r, j]
        if mut == "perturb":
            out[y_off: y_off + rows] = perturb(out[y_off: y_off + rows]) if not y_rowmajor else perturb(out[y_off: y_off + p])
        return out

    def _mask(self, a):
        m = np.zeros(len(a["Y"]), bool)
        if a["y_rowmajor"]:
            m[a["y_off"]: a["y_off"] + a["rows"] * a["ldy"]].reshape(a["rows"], a["ldy"])[:, :a["p"]] = True
        else:
            for j in range(a["p"]):
                m[a["y_off"] + j * a["ldy"]: a["y_off"] + j * a["ldy"] + a["rows"]] = True
        return m

    def check(self, impl, c):
        a = c.args
        got = impl(**a)
        m = self._mask(a)
        assert_exact(self.name + " (padding)", c, got[~m], a["Y"][~m])
        if c.kind == "exact":
            assert 2 * a["k"] * 128 < 2.0 ** 53
            assert_exact(self.name, c, got[m], self.ref(**a)[m])
        else:
            Bm = rm_view(a["B"], a["b_off"], a["k"], a["p"], a["ldb"]) if a["b_rowmajor"] else cm_view(a["B"], a["b_off"], a["k"], a["p"], a["ldb"])
            S = np.abs(cm_view(a["Z"], a["z_off"], a["rows"], a["k"], a["ldz"])) @ np.abs(Bm)
            Sb = np.zeros(len(a["Y"]))
            if a["y_rowmajor"]:
                Sb[a["y_off"]: a["y_off"] + a["rows"] * a["ldy"]].reshape(a["rows"], a["ldy"])[:, :a["p"]] = S
            else:
                for j in range(a["p"]):
                    Sb[a["y_off"] + j * a["ldy"]: a["y_off"] + j * a["ldy"] + a["rows"]] = S[:, j]
            assert_bounded(self.name, c, got[m], self.ref(dt=CLD, **a)[m], cbound(a["k"], Sb[m]))


def _op(M, t):
    return M if t == 0 else M.T if t == 1 else np.conj(M).T


class ZgemmSk(Prim):
    """impl(transa, transb, m, n, k, alpha, A, lda, B, ldb, beta, C, ldc, ksplit) -> C': C = alpha op(A) op(B) + beta C"""
    name = "nep_zgemm_sk"
    mutants = ("drop_last_k", "drop_tail16_k", "conj_wrong", "beta_ignored", "ld_as_min", "last_col_stale", "last_slice_dropped",
               "perturb", "pad_clobbered")

    def _case(self, group, ta, tb, m, n, k, ksplit, alpha, beta, kind, nan_c=False):
        return Case(group, "t%d%d_m%d_n%d_k%d_s%d_b%s" % (ta, tb, m, n, k, ksplit, beta), kind,
                    partial(self._build, ta, tb, m, n, k, ksplit, alpha, beta, kind, nan_c))

    @staticmethod
    def _build(ta, tb, m, n, k, ksplit, alpha, beta, kind, nan_c):
        rng = np.random.default_rng(_seed("zsk%d%d.%d.%d.%d.%d%s" % (ta, tb, m, n, k, ksplit, kind)))
        A = operand(kind, rng, (m, k) if ta == 0 else (k, m)); B = operand(kind, rng, (k, n) if tb == 0 else (n, k))
        lda, ldb, ldc = A.shape[0] + 1, B.shape[0] + 2, m + 3
        Cm = np.full((m, n), NAN) if nan_c else operand(kind, rng, (m, n))
        return dict(transa=ta, transb=tb, m=m, n=n, k=k, alpha=complex(alpha), A=colmajor_buf(A, lda), lda=lda, B=colmajor_buf(B, ldb),
                    ldb=ldb, beta=complex(beta), C=colmajor_buf(Cm, ldc, fill=SENT, trail=1), ldc=ldc, ksplit=ksplit)

    def cases(self):
        for ta in (0, 1, 2):
            for tb in (0, 1, 2):
                yield self._case("trans", ta, tb, 65, 63, 1000, 7, 2 - 1j, 1 + 2j, "exact")
                yield self._case("trans", ta, tb, 65, 63, 1000, 7, 0.3 - 0.7j, -0.4 + 0.1j, "rounded")
        for k in (1, 15, 16, 17, 1000, 9956):
            for m in (1, 63, 64, 65):
                for n in (1, 63, 64, 65):
                    for ks in (1, 2, 7, 64):
                        ta, tb = ((2, 0), (0, 0), (0, 1), (1, 2))[(m + n + ks) % 4]
                        beta0 = (m + n + ks + k) % 2 == 0
                        yield self._case("K%d" % k, ta, tb, m, n, k, ks, 1 - 2j, 0 if beta0 else 2 + 1j, "exact", nan_c=beta0)
            yield self._case("K%d" % k, 2, 0, 64, 65, k, 7, 0.3 - 0.7j, 0.0, "rounded", nan_c=True)
            yield self._case("K%d" % k, 0, 1, 65, 1, k, 64, 0.3 - 0.7j, 1.5 + 0.5j, "rounded")
        # more slices asked for than there are 16-wide chunks of K: fewer slices are produced
        for k, ks in ((17, 64), (40, 5), (100, 64), (16, 2)):
            yield self._case("few_chunks", 2, 0, 33, 32, k, ks, 1 - 2j, 2 + 1j, "exact")

    def ref(self, transa, transb, m, n, k, alpha, A, lda, B, ldb, beta, C, ldc, ksplit, mut=None, dt=C128):
        out = C.astype(dt)
        ra, rb = (m if transa == 0 else k), (k if transb == 0 else n)
        if mut == "ld_as_min":
            lda, ldb = ra, rb
        Am = _op(cm_view(A, 0, ra, (k if transa == 0 else m), lda).astype(dt), 1 if (mut == "conj_wrong" and transa == 2) else transa)
        Bm = _op(cm_view(B, 0, rb, (n if transb == 0 else k), ldb).astype(dt), transb)
        if mut == "conj_wrong" and transa != 2:
            Bm = np.conj(Bm)
        kk = k - 1 if mut == "drop_last_k" else drop_tail(k, 16) if mut == "drop_tail16_k" else k
        if mut == "last_slice_dropped" and ksplit > 1:
            kchunk = (-(-k // ksplit) + 15) // 16 * 16
            nz = -(-k // kchunk)
            kk = (nz - 1) * kchunk if nz > 1 else k
        P = Am[:, :kk] @ Bm[:kk, :]
        Cv = cm_view(out, 0, m, n, ldc)
        R = dt(alpha) * P
        if beta != 0 and mut != "beta_ignored":
            R = R + dt(beta) * Cv
        nn = n - 1 if mut == "last_col_stale" else n
        for j in range(nn):
            out[j * ldc: j * ldc + m] = R[:, j]
        if mut == "pad_clobbered" and ldc > m:
            out[m] = 0
        if mut == "perturb":
            out[:m] = perturb(out[:m])
        return out

    def check(self, impl, c):
        a = c.args
        got = impl(**a)
        m, n, ldc = a["m"], a["n"], a["ldc"]
        mask = np.zeros(len(a["C"]), bool)
        for j in range(n):
            mask[j * ldc: j * ldc + m] = True
        assert_exact(self.name + " (padding)", c, got[~mask], a["C"][~mask])
        if c.kind == "exact":
            assert (2 * a["k"] * 128 * 3 + 24) * 3 < 2.0 ** 53
            assert_exact(self.name, c, got[mask], self.ref(**a)[mask])
        else:
            ra, rb = (m if a["transa"] == 0 else a["k"]), (a["k"] if a["transb"] == 0 else n)
            Aa = np.abs(_op(cm_view(a["A"], 0, ra, (a["k"] if a["transa"] == 0 else m), a["lda"]), a["transa"]))
            Ba = np.abs(_op(cm_view(a["B"], 0, rb, (n if a["transb"] == 0 else a["k"]), a["ldb"]), a["transb"]))
            S = abs(a["alpha"]) * (Aa @ Ba)
            if a["beta"] != 0:
                S = S + abs(a["beta"]) * np.abs(cm_view(a["C"], 0, m, n, ldc))
            assert_bounded(self.name, c, got[mask], self.ref(dt=CLD, **a)[mask], cbound(a["k"], S.T.reshape(-1)))


# ================================================================================================================================
def spmm_terms_matrices(n, mt, cplx, seed):
    """integer-valued n x n CSR terms: empty rows, one row with more than 64 stacked entries, the last row empty"""
    import scipy.sparse as sp
    rng = np.random.default_rng(seed)
    out = []
    for t in range(mt):
        D = np.zeros((n, n), dtype=C128)
        nnz = 4 * n
        r = rng.integers(0, n, nnz); cidx = rng.integers(0, n, nnz)
        D[r, cidx] = rng.integers(1, 5, nnz) * rng.choice([-1, 1], nnz)
        if cplx and t % 2 == 1 or (cplx and mt == 1):
            D[r, cidx] += 1j * rng.integers(-4, 5, nnz)
        D[5 % n, :] = rng.integers(1, 4, n) + (1j if (cplx and (t % 2 == 1 or mt == 1)) else 0)       # dense row: n * mt > 64 stacked entries
        D[[0, n // 2, n - 1], :] = 0                                                # empty rows, first and last among them
        out.append(sp.csr_matrix(D if cplx and (t % 2 == 1 or mt == 1) else D.real.astype(np.float64)))
    return out


class SpmmTerms(Prim):
    """impl(terms, p, XT, ldx, ZT, ldz) -> (status, ZT'): ZT[:, :p] = sum_t A_t XT[:, t p:(t + 1) p], row-major blocks"""
    name = "nep_spmm_terms"
    mutants = ("drop_last", "last_col_stale", "xoff_zero", "ld_as_min", "drop_tail64_cols", "long_row_truncated", "perturb", "pad_clobbered")
    N = 97

    def cases(self):
        for cplx in (False, True):
            for mt in (1, 4):
                terms = spmm_terms_matrices(self.N, mt, cplx, 11 + mt + 2 * cplx)
                for p in (1, 7, 64, 65, 128, 129, 192, 193, 256, 257):
                    for kind in ("exact",) + (("rounded",) if p in (7, 129, 256) else ()):
                        yield Case("%s_mt%d" % ("complex" if cplx else "real", mt), "p%d" % p, kind,
                                   partial(self._build, terms, cplx, mt, p, kind))

    def _build(self, terms, cplx, mt, p, kind):
        rng = np.random.default_rng(_seed("spmm%d.%d.%d%s" % (cplx, mt, p, kind)))
        ldx, ldz = p * mt + 3, p + 2
        X = operand(kind, rng, (self.N, p * mt))
        return dict(terms=terms, p=p, XT=rowmajor_buf(X, ldx), ldx=ldx, ZT=np.full(self.N * ldz + 1, SENT, dtype=C128), ldz=ldz)

    def ref(self, terms, p, XT, ldx, ZT, ldz, mut=None, dt=C128):
        out = ZT.astype(dt)
        if p > 256:
            return -2, out
        n, mt = terms[0].shape[0], len(terms)
        if mut == "ld_as_min":
            ldx, ldz = p * mt, p
        X = rm_view(XT, 0, n, p * mt, ldx)
        Z = np.zeros((n, p), dtype=dt)
        for t, A in enumerate(terms):
            D = A.toarray().astype(dt)
            if mut == "long_row_truncated":
                for i in range(n):
                    nzc = np.flatnonzero(D[i])
                    D[i, nzc[64 // mt:]] = 0
            xo = 0 if mut == "xoff_zero" else t * p
            Z += D @ X[:, xo: xo + p].astype(dt)
        r = n - 1 if mut == "drop_last" else n
        pc = p - 1 if mut == "last_col_stale" else drop_tail(p, 64) if mut == "drop_tail64_cols" else p
        out[: n * ldz].reshape(n, ldz)[:r, :pc] = Z[:r, :pc]
        if mut == "pad_clobbered":
            out[p if ldz > p else 0] = 0
        if mut == "perturb":
            out[:p] = perturb(out[:p])
        return 0, out

    def check(self, impl, c):
        a = c.args
        st, got = impl(**a)
        st_ref, want = self.ref(**a)
        assert st == st_ref, "%s %r: status %d, want %d" % (self.name, c, st, st_ref)
        n, p, ldz = a["terms"][0].shape[0], a["p"], a["ldz"]
        if st_ref:
            return assert_exact(self.name + " (refused call)", c, got, a["ZT"])
        m = np.zeros(len(a["ZT"]), bool)
        m[: n * ldz].reshape(n, ldz)[:, :p] = True
        assert_exact(self.name + " (padding)", c, got[~m], a["ZT"][~m])
        mt = len(a["terms"])
        X = np.abs(rm_view(a["XT"], 0, n, p * mt, a["ldx"]))
        S = sum(np.abs(A.toarray()) @ X[:, t * p:(t + 1) * p] for t, A in enumerate(a["terms"]))
        if c.kind == "exact":
            assert_below_2_53(2 * S)
            assert_exact(self.name, c, got[m], want[m])
        else:
            rowlen = int(max(sum(np.diff(A.indptr) for A in a["terms"])))
            assert_bounded(self.name, c, got[m], self.ref(dt=CLD, **a)[1][m], cbound(rowlen, S.reshape(-1)))


# ================================================================================================================================
QR_SHAPES = [(1, 1), (5, 3), (1000, 1), (4099, 17), (70001, 64)]


class OrthQr(Prim):
    """impl(Q, ldq, rows, k, out) -> (Q', out'): thin QR by column-wise DGKS; row j of out (k rows of k + 2 complex) holds R[0..j, j],
    (R[j, j], 0), (passes, 2 breakdown + another_pass_wanted), the rest of the row is not written.

    Bound on ||a_j - Q R[:, j]||_2 (two Gram-Schmidt passes).  Whatever coefficients h1, h2 the projections return, the updates
    compute w1 = a - Q h1 + e1, w2 = w1 - Q h2 + e2 with |e| <= sqrt(2) gamma_{2 j + 6} (|w| + |Q| |h|) componentwise, R[:j, j] =
    fl(h1 + h2), q_j = fl(w2 / beta).  So a - Q R[:, j] = -(e1 + e2) + Q (fl(h1 + h2) - h1 - h2) + (w2 - q_j beta), and with
    || |Q| ||_2 <= sqrt(j) (1 + 1e-12) (unit columns, asserted separately), ||h1|| <= 1.01 ||a||, ||w1|| <= 2.02 ||a||, ||h2|| <=
    2.03 ||a||, ||w2|| <= 4.1 ||a||, ||R[:j, j]|| <= 3.1 ||a||:   ||a_j - (Q R)_j|| <= sqrt(2) gamma_{2 j + 6} (8 + 7 sqrt(j)) ||a_j||."""
    name = "nep_orth_qr_dev"
    mutants = ("drop_last", "r_diag_negative", "one_pass_sloppy", "row_layout_shifted", "conj_wrong", "last_col_stale")
    exact_only_mutants = ()

    def cases(self):
        def build(rows, k, dep=None):
            rng = np.random.default_rng(_seed("qr%d.%d" % (rows, k)))
            A = grand(rng, (rows, k))
            if dep is not None:
                A[:, dep] = A[:, :dep] @ grand(rng, dep)                # column dep inside the span of its predecessors
            ldq = rows + (3 if dep is None else 0)
            return dict(Q=colmajor_buf(A, ldq, fill=SENT), ldq=ldq, rows=rows, k=k, out=np.full(k * (k + 2), SENT, dtype=C128))

        for rows, k in QR_SHAPES:
            yield Case("%dx%d" % (rows, k), "random", "rounded", partial(build, rows, k))
        yield Case("4099x9", "dependent_column", "rounded", partial(build, 4099, 9, 5), extra=dict(dependent=5))

    def ref(self, Q, ldq, rows, k, out, mut=None, dt=C128):
        Qo, oo = Q.copy(), out.copy()
        A = np.array(cm_view(Q, 0, rows, k, ldq))
        Qm = np.zeros((rows, k), dtype=C128)
        r_used = rows - 1 if (mut == "drop_last" and rows > 1) else rows
        for j in range(k if mut != "last_col_stale" or k == 1 else k - 1):
            w = A[:, j].copy()
            h = np.zeros(j, dtype=C128)
            passes = 0
            for _ in range(1 if mut == "one_pass_sloppy" else 2):
                if j:
                    Qj = Qm[:r_used, :j]
                    c = (Qj.T @ w[:r_used]) if mut == "conj_wrong" else (np.conj(Qj).T @ w[:r_used])
                    if mut == "one_pass_sloppy":
                        c = c * (1 + 1e-9)
                    w[:r_used] = w[:r_used] - Qj @ c
                    h += c
                passes += 1
            beta = np.linalg.norm(w[:r_used])
            if mut == "drop_last" and rows > 1:
                w[-1] = A[-1, j]
            Qm[:, j] = w / beta
            row = oo[j * (k + 2): (j + 1) * (k + 2)]
            sh = 1 if (mut == "row_layout_shifted" and j + 3 <= k + 2) else 0
            row[sh: sh + j] = h
            row[sh + j] = -beta if mut == "r_diag_negative" else beta
            row[sh + j + 1] = complex(passes, 0)
            if mut == "r_diag_negative":
                Qm[:, j] = -Qm[:, j]
            Qo[j * ldq: j * ldq + rows] = Qm[:, j]
        return Qo, oo

    def check(self, impl, c):
        a = c.args
        rows, k, ldq = a["rows"], a["k"], a["ldq"]
        Qb, ob = impl(**a)
        A = np.array(cm_view(a["Q"], 0, rows, k, ldq))
        pad = np.ones(len(Qb), bool)
        for j in range(k):
            pad[j * ldq: j * ldq + rows] = False
        assert_exact(self.name + " (padding of Q)", c, Qb[pad], a["Q"][pad])
        Qm = np.array(cm_view(Qb, 0, rows, k, ldq))
        assert np.all(np.isfinite(Qm)), "%s %r: NaN / Inf in Q" % (self.name, c)
        R = np.zeros((k, k), dtype=C128)
        dep = c.extra.get("dependent")
        for j in range(k):
            row = ob[j * (k + 2): (j + 1) * (k + 2)]
            assert np.all(np.isfinite(row[:j + 2])), (self.name, c, j, row[:j + 2])
            assert_exact(self.name + " (row %d of d_out behind its j + 2 entries)" % j, c, row[j + 2:], np.full(k - j, SENT))
            R[:j, j] = row[:j]
            assert row[j].imag == 0 and row[j].real > 0, "%s %r: R[%d, %d] = %r is not real positive" % (self.name, c, j, j, row[j])
            R[j, j] = row[j]
            passes, flags = row[j + 1].real, row[j + 1].imag
            assert passes in (1.0, 2.0) and flags in (0.0, 1.0, 2.0, 3.0), (self.name, c, j, row[j + 1])
            if j != dep:
                assert flags == 0.0, "%s %r: column %d reports flags %r" % (self.name, c, j, flags)
            else:                                                   # inside the span: two passes ran, no breakdown (the norm is tiny, not 0)
                assert passes == 2.0 and flags in (0.0, 1.0), (self.name, c, row[j + 1])
                assert abs(R[j, j]) <= 1e-10 * np.linalg.norm(A[:, j]), "%s %r: R[%d, %d] = %r is not tiny" % (self.name, c, j, j, R[j, j])
        G = np.conj(Qm).T @ Qm - np.eye(k)
        if dep is not None:                                         # a normalised noise vector need not be orthogonal to the rest
            keep = [j for j in range(k) if j != dep]
            assert abs(G[dep, dep]) <= 1e-12
            G = G[np.ix_(keep, keep)]
        assert np.linalg.norm(G, 2) <= 1e-12, "%s %r: ||Q^H Q - I|| = %.3e" % (self.name, c, np.linalg.norm(G, 2))
        QR = Qm.astype(CLD) @ R.astype(CLD)
        err = np.linalg.norm((QR - A.astype(CLD)).astype(C128), axis=0)
        cols = np.arange(k)
        bound = SQ2 * np.array([gamma(2 * j + 6) for j in cols]) * (8 + 7 * np.sqrt(cols)) * np.linalg.norm(A, axis=0)
        if dep is not None:                                         # columns behind the noise vector project on it as well: same bound
            pass
        assert_bounded(self.name, c, err, np.zeros(k, dtype=np.longdouble), bound)


# ================================================================================================================================
HESS_CASES = [(1, 22, 0), (4, 5, 1), (8, 3, 4), (3, 100, 0), (5, 64, 16)]


def eig_block_check(name, c, b, H, lam, Z, st_qr, st_vec, lam_single, eig_tol=1e-12, res_tol=1e-12):
    """the criteria of test_gpu_kernels._hess_eig_check for one block of a batch, plus: the same eigenvalue multiset as the
    single-block call on the same leading block, to eig_tol of the spectral radius"""
    k = H.shape[0]
    assert st_qr.real == 0 and st_vec.real == 0, (name, c, b, st_qr, st_vec)
    ref = np.linalg.eigvals(H)
    for other, what in ((ref, "LAPACK"), (lam_single, "the single-block call")):
        if other is None:
            continue
        used = np.zeros(k, bool)
        for x in lam:
            d = np.abs(other - x); d[used] = np.inf; j = int(np.argmin(d)); used[j] = True
            assert d[j] <= eig_tol * max(np.abs(ref).max(), 1e-300), "%s %r block %d: eigenvalue %r against %s (%r)" % (name, c, b, x, what, other[j])
    nH = max(np.linalg.norm(H), 1e-300)
    res = np.linalg.norm(H @ Z - Z * lam[None, :], axis=0) / nH
    assert res.max() <= res_tol, "%s %r block %d: residual %.3e" % (name, c, b, res.max())
    assert np.abs(np.linalg.norm(Z, axis=0) - 1).max() < 1e-14
    big = Z[np.argmax(np.abs(Z), axis=0), np.arange(k)]
    assert np.abs(big.imag).max() < 1e-14 and big.real.min() > 0


class HessEigBatch(Prim):
    """impl(nb, k0, kstep, H, ldh, w, w_stride, Z, ldz, z_stride) -> (w', Z'): eigen-decompositions of the leading blocks of sizes
    k0 + b kstep of one Hessenberg matrix stored in nep_iar_step's row layout; `single(H_block)` (argument of check) gives the
    eigenvalues of the single-block call"""
    name = "nep_hess_eig_batch_dev"
    mutants = ("block_reads_k0", "last_block_stale", "stride_as_min", "ld_as_min", "vectors_not_normalised")
    exact_only_mutants = ()

    def __init__(self):
        import os
        self.H100 = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "gun_iar_H100.npy"))

    def cases(self):
        def build(nb, k0, kstep, H):
            kmax = k0 + (nb - 1) * kstep
            m = kmax + 3
            ldh = m + 4
            blk = np.full((m, ldh), 7e300 + 3e300j)                  # poison everywhere the kernel must not look
            for j in range(kmax):
                blk[j, :min(j + 2, kmax)] = H[:min(j + 2, kmax), j]
            w_stride, ldz = kmax + 2 + 3, kmax + 1
            z_stride = kmax * ldz + 7
            return dict(nb=nb, k0=k0, kstep=kstep, H=blk.reshape(-1), ldh=ldh, w=np.full(nb * w_stride + 1, SENT, dtype=C128),
                        w_stride=w_stride, Z=np.full(nb * z_stride + 1, SENT, dtype=C128), ldz=ldz, z_stride=z_stride)

        for nb, k0, kstep in HESS_CASES:
            kmax = k0 + (nb - 1) * kstep
            if kmax > 100:                 # the fixture has 100 columns: a random Hessenberg matrix, as test_hess_eig_dev_edge_matrices[k128]
                H = np.triu(grand(np.random.default_rng(7), (kmax, kmax)), -1)
            else:
                H = self.H100[:kmax, :kmax]
            yield Case("nb%d_k%d_step%d" % (nb, k0, kstep), "iar_row_layout", "rounded", partial(build, nb, k0, kstep, H), extra=dict(H=H),
                       host=kmax <= 40)

    def ref(self, nb, k0, kstep, H, ldh, w, w_stride, Z, ldz, z_stride, mut=None, dt=C128):
        wo, Zo = w.copy(), Z.copy()
        if mut == "stride_as_min":
            kmax = k0 + (nb - 1) * kstep
            w_stride, z_stride = kmax + 2, kmax * ldz
        for b in range(nb - 1 if (mut == "last_block_stale" and nb > 1) else nb):
            k = k0 if mut == "block_reads_k0" else k0 + b * kstep
            kk = k0 + b * kstep
            Hb = np.array(cm_view(H, 0, k, k, ldh))
            Hb = np.triu(Hb, -1)
            lam, V = np.linalg.eig(Hb)
            V = V / np.linalg.norm(V, axis=0)
            V = V * np.exp(-1j * np.angle(V[np.argmax(np.abs(V), axis=0), np.arange(k)]))
            if mut == "vectors_not_normalised":
                V = V * 1.0000001
            lam_f = np.zeros(kk, dtype=C128); lam_f[:k] = lam
            Vf = np.zeros((kk, kk), dtype=C128); Vf[:k, :k] = V
            wo[b * w_stride: b * w_stride + kk] = lam_f
            wo[b * w_stride + kk: b * w_stride + kk + 2] = 0
            l = kk if mut == "ld_as_min" else ldz
            for j in range(kk):
                Zo[b * z_stride + j * l: b * z_stride + j * l + kk] = Vf[:, j]
        return wo, Zo

    def check(self, impl, c, single=None):
        a = c.args
        nb, k0, kstep, ws, ldz, zs = a["nb"], a["k0"], a["kstep"], a["w_stride"], a["ldz"], a["z_stride"]
        wb, Zb = impl(**a)
        wm = np.zeros(len(wb), bool); zm = np.zeros(len(Zb), bool)
        for b in range(nb):
            k = k0 + b * kstep
            wm[b * ws: b * ws + k + 2] = True
            for j in range(k):
                zm[b * zs + j * ldz: b * zs + j * ldz + k] = True
        assert_exact(self.name + " (between the result blocks)", c, wb[~wm], a["w"][~wm])
        assert_exact(self.name + " (between the vector blocks)", c, Zb[~zm], a["Z"][~zm])
        for b in range(nb):
            k = k0 + b * kstep
            Hb = c.extra["H"][:k, :k]
            lam = wb[b * ws: b * ws + k]
            Zm = np.array(cm_view(Zb, b * zs, k, k, ldz))
            assert np.all(np.isfinite(lam)) and np.all(np.isfinite(Zm)), (self.name, c, b)
            eig_block_check(self.name, c, b, Hb, lam, Zm, wb[b * ws + k], wb[b * ws + k + 1], single(Hb) if single else None)


PRIMS = [ColDots(True), ColDots(False), ColNorms(False), ColNorms(True), RowMajorColNorms(), RowMajorToColMajor(), RowDot(), Hadamard(),
         Axpy(), Scal(), AbsVec(), IarShiftScale(), RkBw(), BlockRecur(), GemvH(), GemmTsDev(), ZgemmSk(), SpmmTerms(), OrthQr()]
# nep_hess_eigvals_batch_dev and nep_hess_eigvecs_batch_dev are one pair of calls: one checker, listed under both names
HESS = HessEigBatch()
TABLE = ["nep_axpy", "nep_scal", "nep_nrm2", "nep_colnorms", "nep_coldots", "nep_coldotsu", "nep_rowdot", "nep_hadamard", "nep_absvec",
         "nep_rowmajor_colnorms", "nep_rowmajor_to_colmajor", "nep_rk_bw", "nep_block_recur", "nep_iar_shift_scale", "nep_gemv_h",
         "nep_orth_qr_dev", "nep_zgemm_sk", "nep_gemm_ts_dev", "nep_spmm_terms", "nep_hess_eigvals_batch_dev", "nep_hess_eigvecs_batch_dev",
         "nep_orth", "nep_orth_dev", "nep_gemm_h_rm"]


class _ByName(dict):
    """the checkers of K6 and K9 (nep_orth, nep_orth_dev, nep_gemm_h_rm) live in orth_checkers.py, which imports this module"""

    def __missing__(self, name):
        import orth_checkers
        return orth_checkers.BY_NAME[name]


BY_NAME = _ByName({p.name: p for p in PRIMS})
BY_NAME["nep_hess_eigvals_batch_dev"] = BY_NAME["nep_hess_eigvecs_batch_dev"] = HESS


def groups(prim):
    """case groups of a primitive, in order (the GPU tests are parametrised by group; operands are built when a case runs)"""
    seen = []
    for c in prim.cases():
        if c.group not in seen:
            seen.append(c.group)
    return seen
