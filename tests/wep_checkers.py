"""References, error bounds, case lists and mutants for the waveguide kernels of csrc/wep.hip (the whole C5 operator step): one
checker per entry point of include/nepmi355.h,

    nep_wep_sylv_solve, nep_wep_pinv_apply, nep_wep_schur_matvec, nep_wep_region_means, nep_wep_region_expand,
    nep_wep_smw_matrix, nep_wep_smw_matrix_modes, nep_wep_smw_apply.

`CHECKERS[name].check(impl, case)` runs `impl` on the operands of `case` and compares with a reference that is restated here from
the operation definitions in the header (and waveguide_preconditioner.jl:120-421, Waveguide.jl:53-65, 159-170, 394-425) in
np.clongdouble.  `impl` takes the operands as NumPy arrays and returns fresh arrays: test_gpu_wep_checkers.py passes adapters that
upload and call the library, test_host_wep_checkers.py passes the float64 NumPy restatement `ref` and its mutants (`mut=name`).
Operands are arbitrary, not a physical waveguide.  A block of nz x nx values, z fastest, is an array of shape (nx, nz) here: A[x] is
grid column x and A.reshape(-1) is the device buffer.

Three kinds of case:
  exact     Gaussian-integer operands; every intermediate is an integer below 2^53 (asserted), comparison np.array_equal.
  rounded   entrywise a-priori bound |impl - ref| <= cbound(nterms, S) (P^{-1} and the boundary term of the Schur product).
  measured  the affine scans of the tridiagonal kernel admit no useful entrywise a-priori bound, so the yardstick is computed per
            case: the error of the float64 restatement (np.fft in float64, sequential Thomas sweep) against the extended
            reference, per grid column (per matrix column for the SMW matrix) relative to that column's norm; the implementation
            has to stay within MARGIN * max(that error, 4 u) on every column.  MARGIN = 8: a float64 emulation of the kernel's scan
            order (segment composites + a 64-lane Hillis-Steele scan) stays within 1.5 x the sequential sweep; the rest is room
            for FMA contraction and the dense DFT stages.  Nothing is fitted to a device result.
"""
from functools import partial

import numpy as np

import primitive_checkers as pc
from primitive_checkers import C128, CLD, SENT, U, Case, assert_exact, assert_bounded, assert_below_2_53, gint, grand, _seed

LD = np.longdouble
MARGIN = 8.0
LDS_MAX = 150 * 1024
K_RB, K_PLAIN, K_SYM = 1, 2, 3                              # info[2] of nep_wep_plan
OP_SYLV, OP_PINV, OP_SMW = 0, 1, 2
KNAME = {K_RB: "rb", K_PLAIN: "plain", K_SYM: "sym"}


# ================================================================================================================================
# the launch predicates of csrc/wep.hip, restated (test_host_wep_checkers.py compares nep_wep_plan with this for every nz <= 2500)
def factor(nz):
    N1, N2 = nz, 1
    a = 2
    while a * a <= nz:
        if nz % a == 0 and np.gcd(a, nz // a) == 1 and a + nz // a < N1 + N2:
            N1, N2 = nz // a, a
        a += 1
    return N1, N2


def seg_of(nx):
    seg = 1
    while 64 * seg < nx:
        seg *= 2
    return seg


def _sym(nz, N1, N2, symcfg):
    cols, kb = symcfg // 10, symcfg % 10
    if not (symcfg and N1 % 2 and N2 % 2 and N1 >= 3 and N2 >= 3 and cols in (2, 4) and kb in (2, 3)):
        return None
    H1, H2 = (N1 - 1) // 2, (N2 - 1) // 2
    items = max(-(-H1 // kb) * N2, -(-H2 // kb) * N1)
    threads = -(-items // 64) * 64
    shm = (cols * nz + N1 + N2) * 16
    if threads > 512 or shm > LDS_MAX:
        return None
    return cols, kb, threads, shm


def predict(nz, nx, op, symcfg=22):
    """(status, info[8]) of nep_wep_plan"""
    zero = [0] * 8
    if nz < 1 or op not in (OP_SYLV, OP_PINV, OP_SMW):
        return -2, zero
    N1, N2 = factor(nz)
    if op == OP_PINV:
        if 5 * nz * 16 > LDS_MAX:
            return -5, zero
        if N1 % 2 and N2 % 2 and N1 >= 3 and N2 >= 3 and max((N1 - 1) // 2 * N2, (N2 - 1) // 2 * N1) <= 512:
            items = max((N1 - 1) // 2 * N2, (N2 - 1) // 2 * N1)
            return 0, [N1, N2, K_SYM, 1, 1, -(-items // 64) * 64, (2 * nz + N1 + N2) * 16, 0]
        return 0, [N1, N2, K_PLAIN, 1, 1, 1024 if nz >= 768 else (512 if nz >= 256 else 256), (3 * nz + N1 + N2) * 16, 0]
    if nx < 2 or nx > 2048 or (op == OP_SMW and nx != nz + 4):
        return -2, zero
    cols = 4
    while cols > 1 and (2 * cols * nz + N1 + N2) * 16 > LDS_MAX:
        cols //= 2
    if (2 * cols * nz + N1 + N2) * 16 > LDS_MAX:
        return -5, zero
    s = _sym(nz, N1, N2, symcfg)
    seg = seg_of(nx)
    if op == OP_SMW:
        if 5 * nz * 16 > LDS_MAX or s is None or 4 * nx * 16 > LDS_MAX:
            return -5, zero
        return 0, [N1, N2, K_SYM, s[0], s[1], s[2], 4 * nx * 16, seg]
    if s is not None:
        return 0, [N1, N2, K_SYM, s[0], s[1], s[2], s[3], seg]
    threads = 384 if cols == 4 else (1024 if nz >= 768 else (512 if nz >= 384 else 256))
    return 0, [N1, N2, K_RB if cols == 4 else K_PLAIN, cols, 3 if cols == 4 else 1, threads, (2 * cols * nz + N1 + N2) * 16, seg]


def dft_form(info):
    """'rb' | 'plain<2>' | 'plain<1>' | 'sym<2,2>' ... of a SYLV / SMW plan"""
    k = info[2]
    return "rb" if k == K_RB else ("plain<%d>" % info[3] if k == K_PLAIN else "sym<%d,%d>" % (info[3], info[4]))


def pinv_form(info):
    return "sym" if info[2] == K_SYM else "plain%d" % info[5]


# ================================================================================================================================
# transforms and sweeps, in the precision of their argument (C128: the float64 restatement, CLD: the reference)
def _pi(dt):
    return LD(4) * np.arctan(LD(1)) if dt == CLD else np.pi


def _dense_dft(nz, sign, dt):
    k = np.arange(nz)
    ang = k.astype(LD if dt == CLD else np.float64) * (2 * _pi(dt) / nz)
    roots = (np.cos(ang) + sign * 1j * np.sin(ang)).astype(dt)              # the nz roots once; entry (z, i) is root z i mod nz
    return roots[np.outer(k, k) % nz]


def xfft(a, sign, dense=False):
    """unnormalised DFT along the last axis, exponent sign * 2 pi i z k / nz.  np.fft keeps extended precision (the result dtype is
    asserted to be that of the argument); where it does not, a dense extended DFT matrix takes its place"""
    a = np.asarray(a)
    if not dense:
        r = np.fft.fft(a, axis=-1) if sign < 0 else np.fft.ifft(a, axis=-1, norm="forward")
        if r.dtype == a.dtype:
            return r
    assert not dense or a.shape[-1] <= 4096
    return a @ _dense_dft(a.shape[-1], sign, a.dtype.type).T


def thomas(d, b, T, mut=None, seg=1):
    """(d_i I + b tridiag(1, -2, 1)) u_i = T[:, i] for every mode i: T, result of shape (nx, nz); sequential in x, vectorised over
    the modes -- the recurrences of k_tridiag_factor / k_tridiag_modes"""
    nx = T.shape[0]
    a = d - 2 * b
    bb = -b if mut == "b_sign" else b
    piv = np.empty_like(T); y = np.empty_like(T); u = np.empty_like(T)
    piv[0] = a; y[0] = T[0]
    for j in range(1, nx):
        m = b / piv[j - 1]
        piv[j] = a - b * m
        prev = y[j - 1] if not (mut == "lane_carry" and j % seg == 0) else 0
        y[j] = T[j] - (bb / piv[j - 1]) * prev
    u[nx - 1] = y[nx - 1] / piv[nx - 1]
    if mut == "last_x":
        u[nx - 1] = y[nx - 1]
    for j in range(nx - 2, -1, -1):
        u[j] = (y[j] - bb * u[j + 1]) / piv[j]
    return u


def sylv(d, b, X, mut=None, seg=1, cols=4):
    """nep_wep_sylv_solve: X <- F Tsolve(F^H X), F[z, i] = exp(-2 pi i z i / nz) / sqrt(nz)"""
    dt = X.dtype.type
    nz = X.shape[1]
    sq = np.sqrt(LD(nz)) if dt == CLD else np.sqrt(float(nz))
    out = xfft(thomas(d.astype(dt), LD(b) if dt == CLD else b, xfft(X, +1) / sq, mut, seg), -1) / sq
    if mut == "tail_group" and X.shape[0] % cols:
        out[X.shape[0] // cols * cols:] = X[X.shape[0] // cols * cols:]
    return out


def pinv(bb, sinv, x, mut=None):
    """nep_wep_pinv_apply: out_half = R diag(sinv_half) R^H x_half, R x = reverse(bb .* fft(x))"""
    nz = len(bb)
    out = np.empty_like(x)
    for h in range(2):
        xh = x[h * nz:(h + 1) * nz]
        sh = sinv[(1 - h) * nz:(2 - h) * nz] if mut == "sinv_halves" else sinv[h * nz:(h + 1) * nz]
        u = (bb if mut == "bb_conj" else np.conj(bb)) * (xh if mut == "no_reverse" else xh[::-1])
        w = bb * xfft(xfft(u, +1) * sh, -1)
        out[h * nz:(h + 1) * nz] = w if mut == "no_reverse" else w[::-1]
    return out


def regions_x(nx, N, L, mut=None):
    """region index of every grid column: 0, 1 | 2 + (x - 2) / L | N + 2, N + 3"""
    x = np.arange(nx)
    off = 0 if mut == "x_offset" else 2
    rx = 2 + np.minimum(np.maximum(x - off, 0) // L, N - 1)
    rx[:2] = [0, 1]
    rx[nx - 2:] = [N + 2, N + 3] if mut != "rx_plus" else [N + 1, N + 2]
    return rx


def means(X, N, mut=None):
    """nep_wep_region_means: out[rx, rz] (the device's N x (N+4) column-major block) = mean of X over region (rz, rx)"""
    nx, nz = X.shape
    L = nz // N
    rx = regions_x(nx, N, L, mut)
    Xz = X.reshape(nx, N, L)
    if mut == "z_last_row":
        Xz = Xz[:, :, :L - 1] if L > 1 else Xz * 0
    sz = Xz.sum(axis=2)                                                   # (nx, N)
    out = np.zeros((N + 4, N), dtype=X.dtype)
    np.add.at(out, rx, sz)
    w = np.full(N + 4, out.real.dtype.type(1) / L)                        # 1 / L for the z mean ...
    w[2:N + 2] /= L                                                       # ... and 1 / L for the x mean of the interior regions
    if mut == "boundary_weight":
        w[:2] /= L; w[N + 2:] /= L
    return out * w[:, None]


def expand(alpha, Ksc, dd1, dd2, mut=None):
    """nep_wep_region_expand: Y[x, z] = alpha[rx, rz] Ksc[x, z]; eb = (dd1 a[0] + dd2 a[1], dd2 a[N+2] + dd1 a[N+3]) over rz(z)"""
    nx, nz = Ksc.shape
    N = alpha.shape[1]
    L = nz // N
    rx = regions_x(nx, N, L, mut)
    az = np.repeat(alpha, L, axis=1)                                      # (N+4, nz)
    Y = az[rx] * Ksc
    p1, p2 = (dd1, dd2) if mut == "dd_plus" else (dd2, dd1)
    eb = np.concatenate([dd1 * az[0] + dd2 * az[1], p1 * az[N + 2] + p2 * az[N + 3]])
    return Y, eb


def stencil(X, D0, cp, cm, cx, c1s, pb, mut=None):
    nx, nz = X.shape
    up, dn = np.roll(X, -1, axis=1), np.roll(X, 1, axis=1)
    if mut == "no_wrap":
        up = up.copy(); dn = dn.copy(); up[:, nz - 1] = 0; dn[:, 0] = 0
    if mut == "wrap_end":
        up = up.copy(); dn = dn.copy(); up[:, nz - 1] = X[:, nz - 1]; dn[:, 0] = X[:, 0]
    r = D0 * X + cp * up + cm * dn
    r[1:] += cx * X[:-1]
    r[:-1] += cx * X[1:]
    if mut == "x_periodic":
        r[0] += cx * X[nx - 1]
    c0, c1 = (min(1, nx - 1), max(nx - 2, 0)) if mut == "c1s_column" else (0, nx - 1)
    if c1s != 0:
        r[c0] -= c1s * pb[:nz]
        r[c1] -= c1s * pb[nz:]
    return r


def gather(X, d1, d2, mut=None):
    """C2T v: d1 X[0] + d2 X[1] | d1 X[nx-1] + d2 X[nx-2]"""
    nx = X.shape[0]
    if mut == "d_swapped":
        d1, d2 = d2, d1
    plus = d1 * X[nx - 2] + d2 * X[nx - 1] if mut == "plus_order" else d1 * X[nx - 1] + d2 * X[nx - 2]
    return np.concatenate([d1 * X[0] + d2 * X[1], plus])


def schur(bb, sinv, X, D0, cp, cm, cx, d1, d2, c1s, mut=None):
    """nep_wep_schur_matvec -> (P, out)"""
    pb = pinv(bb, sinv, gather(X, d1, d2, mut), mut)
    return pb, stencil(X, D0, cp, cm, cx, c1s, pb, mut)


def mode_means_matrix(nz, N):
    """dG of nep_wep_smw_apply from its definition, in extended precision, rounded: G[rz, i] = mean over the z of region rz of
    exp(-2 pi i z i / nz) / sqrt(nz)"""
    L = nz // N
    F = _dense_dft(nz, -1, CLD) / np.sqrt(LD(nz))                          # F[z, i]
    return (F.reshape(N, L, nz).sum(axis=1) / LD(L)).astype(C128)


def smw_column_block(o, N, kappa, mut=None):
    """E_kappa after the boundary pieces: expansion of the unit vector e_kappa, minus P^{-1} eb in the first / last grid column"""
    dt = o["Ksc"].dtype.type
    alpha = np.zeros((N + 4) * N, dtype=dt); alpha[kappa] = 1
    Y, eb = expand(alpha.reshape(N + 4, N), o["Ksc"], o["dd1"], o["dd2"], mut)
    pb = pinv(o["bb"], o["sinv"], eb, mut)
    nz = len(o["bb"])
    Y[0] -= pb[:nz]
    if mut != "pb_last":
        Y[-1] -= pb[nz:]
    return Y


def smw_matrix(o, N, mut=None):
    """nep_wep_smw_matrix[_modes]: column kappa (row kappa of the returned (mm, mm) array) = region means of Linv(E_kappa)"""
    mm = N * (N + 4)
    M = np.empty((mm, mm), dtype=o["Ksc"].dtype)
    for kappa in range(mm):
        col = means(sylv(o["d"], o["b"], smw_column_block(o, N, kappa, mut), mut, o.get("seg", 1)), N, mut).reshape(-1)
        dst = kappa
        if mut == "batch_offset" and 2 * N + 16 <= kappa < (N + 2) * N:
            dst = kappa - 16
        M[dst] = col
    return M


def smw_apply(o, N, MinvH, R, mut=None, C=None):
    """nep_wep_smw_apply: R <- C - Linv(sum_k alpha_k E_k), C = Linv R (may be handed in), alpha = (MinvH)^H f(C)"""
    nz = len(o["bb"])
    if C is None:
        C = sylv(o["d"], o["b"], R, mut, o.get("seg", 1))
    f = means(C, N, mut).reshape(-1)
    A = MinvH.reshape(len(f), len(f))                                      # A[i] = column i of MinvH
    alpha = (A.T if mut == "alpha_plain" else np.conj(A)) @ f
    Y, eb = expand(alpha.reshape(N + 4, N), o["Ksc"], o["dd1"], o["dd2"], mut)
    pb = pinv(o["bb"], o["sinv"], eb, mut)
    Y[0] -= pb[:nz]
    if mut != "pb_last":
        Y[-1] -= pb[nz:]
    W = sylv(o["d"], o["b"], Y, mut, o.get("seg", 1))
    return C + W if mut == "second_sign" else C - W


def _as(dt, o):
    """the operand dict in precision dt (real scalars widened as well)"""
    out = {}
    for k, v in o.items():
        if isinstance(v, np.ndarray) and np.iscomplexobj(v):
            out[k] = v.astype(dt)
        elif isinstance(v, float) and dt == CLD:
            out[k] = LD(v)
        else:
            out[k] = v
    return out


def col_err(got, ref):
    """per-row (= per grid column / matrix column) relative error in the 2-norm, float64"""
    diff = np.asarray(got).astype(ref.dtype) - ref
    nrm = np.sqrt((np.abs(ref) ** 2).sum(axis=1)).astype(np.float64)
    return np.sqrt((np.abs(diff) ** 2).sum(axis=1)).astype(np.float64) / np.maximum(nrm, np.finfo(np.float64).tiny)


def assert_measured(name, c, got, ref, ref64):
    got = np.asarray(got)
    assert got.shape == ref.shape, (name, c, got.shape, ref.shape)
    assert np.all(np.isfinite(got)), "%s %r: non-finite result" % (name, c)
    yard = MARGIN * np.maximum(col_err(ref64, ref), 4 * U)
    err = col_err(got, ref)
    ratio = float(np.max(err / yard))
    pc.RATIOS[name] = max(pc.RATIOS.get(name, 0.0), ratio)
    i = int(np.argmax(err / yard))
    assert ratio <= 1.0, "%s %r: column %d: error %.3e, %g x the float64 restatement's %.3e (allowed %g)" % (
        name, c, i, err[i], err[i] / max(yard[i] / MARGIN, 1e-300), yard[i] / MARGIN, MARGIN)
    return ratio


def _tail_intact(name, c, buf, n):
    assert len(buf) > n and np.all(buf[n:] == SENT), "%s %r: written behind the end of the output" % (name, c)


# ================================================================================================================================
# operands
def _rng(*key):
    return np.random.default_rng(_seed(".".join(str(k) for k in key)))


def sylv_operands(rng, nz, nx):
    """random h_d with the imaginary offset of sigma = -3 - 3.5j (|Im d| >= b / 2 keeps every d_i + s_j, s_j in (-4 b, 0), away from
    zero: the tridiagonal systems are well conditioned)"""
    b = 1.0 / 0.37 ** 2
    d = b * (rng.uniform(-3.0, 1.0, nz) + 1j * np.sign(-3.5) * rng.uniform(0.5, 1.5, nz))
    return dict(d=d.astype(C128), b=b)


def pinv_operands(rng, nz):
    ph = rng.uniform(0, 2 * np.pi, nz)
    return dict(bb=np.exp(1j * ph).astype(C128), sinv=grand(rng, 2 * nz) / nz)


def smw_operands(nz):
    rng = _rng("smw", nz)
    nx = nz + 4
    o = sylv_operands(rng, nz, nx)
    o.update(pinv_operands(rng, nz))
    o.update(Ksc=grand(rng, (nx, nz)), dd1=float(rng.uniform(0.5, 2.0)), dd2=float(-rng.uniform(0.1, 1.0)), seg=seg_of(nx))
    return o


# ================================================================================================================================
class Checker:
    name = None
    mutants = ()
    kind_of_mutant_cases = ("exact", "rounded", "measured")

    def cases(self):
        raise NotImplementedError


def _cost(c):
    return c.extra.get("cost", 0)


class SylvSolve(Checker):
    """impl(nz, nx, d, b, X) -> (X1, X2): two solves on one handle, each from a fresh copy of X (shape (nx, nz))"""
    name = "nep_wep_sylv_solve"
    mutants = ("last_x", "b_sign", "lane_carry", "tail_group")
    # nz x nx -> DFT form, SEG (confirmed with nep_wep_plan by test_host_wep_checkers.py)
    SIZES = [(7, 2, "rb", 1), (7, 11, "rb", 1), (60, 64, "rb", 1), (60, 65, "rb", 2), (15, 128, "sym<2,2>", 2), (15, 129, "sym<2,2>", 4),
             (35, 256, "sym<2,2>", 4), (35, 257, "sym<2,2>", 8), (35, 512, "sym<2,2>", 8), (35, 513, "sym<2,2>", 16),
             (35, 1024, "sym<2,2>", 16), (35, 1025, "sym<2,2>", 32), (35, 2048, "sym<2,2>", 32), (1199, 5, "sym<2,2>", 1),
             (1200, 5, "plain<2>", 1), (1216, 6, "plain<2>", 1), (2055, 6, "plain<2>", 1), (2400, 5, "plain<1>", 1),
             (2401, 5, "plain<1>", 1), (1443, 7, "sym<2,2>", 1),
             # every form but sym is listed above with SEG < 4 only: here with the [piece][lane][4] layout of the transposed block (TLay)
             (60, 129, "rb", 4), (1200, 130, "plain<2>", 4), (2400, 130, "plain<1>", 4)]

    def cases(self, sizes=None):
        def build(nz, nx):
            rng = _rng(self.name, nz, nx)
            o = sylv_operands(rng, nz, nx)
            o.update(nz=nz, nx=nx, X=grand(rng, (nx, nz)))
            return o
        for nz, nx, form, seg in (sizes or self.SIZES):
            yield Case("sylv", "%dx%d" % (nz, nx), "measured", partial(build, nz, nx), extra=dict(nz=nz, nx=nx, form=form, seg=seg, cost=nz * nx))

    def ref(self, nz, nx, d, b, X, mut=None):
        st, info = predict(nz, nx, OP_SYLV)
        out = sylv(d, b, X.astype(C128), mut, info[7], info[3])
        return out, out.copy()

    def check(self, impl, c):
        a = c.args
        X1, X2 = impl(**a)
        ref = sylv(a["d"].astype(CLD), a["b"], a["X"].astype(CLD))
        ref64 = sylv(a["d"], a["b"], a["X"])
        assert_measured(self.name, c, X1, ref, ref64)
        assert_exact(self.name + " (repeat)", c, X2, X1)
        return 2


def pinv_terms(N1, N2):
    """terms of pc.cbound for one application of P^{-1}: the two transforms are two dense stages of N1 and N2 complex multiply-adds
    each (2 (N1 + N2) terms); the three pointwise complex products (conj(bb), sinv, bb) are one term each; the tabulated roots
    carry a relative error of up to 2 u in each of the four stages (as much as one more term per stage: 4); the symmetric form
    adds one rounding per pair (s_n, d_n) and one for A +- B in each of the four stages (as much as one term per stage: 4)"""
    return 2 * (N1 + N2) + 3 + 4 + 4


class PinvApply(Checker):
    """impl(nz, bb, sinv, x) -> (out, x_after, inplace): out of place (with the input buffer read back), and in place

    Bound: every output is bb_k sum_j W_kj sinv_j sum_m conj(W_jm bb_m) x_m; with every operand replaced by its modulus that is
    S = (sum |sinv|)(sum |x|) for |bb| = 1, the same for every output of a half; |impl - ref| <= cbound(pinv_terms(N1, N2), S)."""
    name = "nep_wep_pinv_apply"
    mutants = ("no_reverse", "bb_conj", "sinv_halves", "perturb")
    SIZES = [(1, "plain256"), (2, "plain256"), (7, "plain256"), (11, "plain256"), (25, "plain256"), (15, "sym"), (105, "sym"), (256, "plain512"), (768, "plain1024"),
             (1000, "plain1024"), (1001, "sym"), (1155, "plain1024"), (1920, "plain1024")]

    def cases(self):
        def build(nz):
            rng = _rng(self.name, nz)
            o = pinv_operands(rng, nz)
            o.update(nz=nz, x=grand(rng, 2 * nz))
            return o
        for nz, form in self.SIZES:
            yield Case("pinv", "nz%d" % nz, "rounded", partial(build, nz), extra=dict(nz=nz, form=form, cost=nz))

    def ref(self, nz, bb, sinv, x, mut=None):
        out = pinv(bb, sinv, x, None if mut == "perturb" else mut)
        if mut == "perturb":
            out = pc.perturb(out)
        return out, x.copy(), out.copy()

    @staticmethod
    def bound(nz, bb, sinv, xabs, extra_terms=0):
        N1, N2 = factor(nz)
        S = np.concatenate([np.full(nz, np.abs(sinv[h * nz:(h + 1) * nz]).sum() * xabs[h * nz:(h + 1) * nz].sum()) for h in range(2)])
        return pc.cbound(pinv_terms(N1, N2) + extra_terms, S * np.abs(bb).max() ** 2)

    def check(self, impl, c):
        a = c.args
        out, x_after, inplace = impl(**a)
        ref = pinv(a["bb"].astype(CLD), a["sinv"].astype(CLD), a["x"].astype(CLD))
        bnd = self.bound(a["nz"], a["bb"], a["sinv"], np.abs(a["x"]))
        n = 2 * a["nz"]
        assert_bounded(self.name, c, out[:n], ref, bnd)
        assert_bounded(self.name, c, inplace[:n], ref, bnd)
        assert_exact(self.name + " (input)", c, x_after[:n], a["x"])
        for buf in (out, inplace):
            if len(buf) > n:
                _tail_intact(self.name, c, buf, n)
        return 2


class SchurMatvec(Checker):
    """impl(nz, nx, bb, sinv, X, D0, cp, cm, cx, d1, d2, c1s) -> (P, out, X_after)

    exact: c1s = 0 and Gaussian-integer cp, cm, D0, X, integer cx -- the stencil alone, bit for bit (periodic wrap in z, Dirichlet
    ends in x).  rounded: c1s != 0; the stencil is a sum of five products (pc.cbound(5 + ..., S_st), S_st in moduli), the boundary
    term adds c1s P^{-1}(d1 X[0] + d2 X[1]) -- the bound of PinvApply with two more terms for the gathered input and one for the
    product with c1s, on S_p = (sum |sinv|)(sum (|d1| |X[0]| + |d2| |X[1]|)).  One cbound over the sum of both S covers both."""
    name = "nep_wep_schur_matvec"
    mutants = ("no_wrap", "wrap_end", "x_periodic", "c1s_column", "d_swapped", "plus_order", "no_reverse", "bb_conj", "sinv_halves", "perturb")
    EXACT_NZ = [1, 2, 11, 255, 256, 257, 513]
    NX = [2, 3, 7]

    def cases(self):
        def build(nz, nx, kind):
            rng = _rng(self.name, nz, nx, kind)
            o = pinv_operands(rng, nz)
            op = partial(pc.operand, kind, rng)
            o.update(nz=nz, nx=nx, X=op((nx, nz)), D0=op((nx, nz)), cp=complex(op(1)[0]), cm=complex(op(1)[0]))
            if kind == "exact":
                o.update(cx=3.0, d1=0.75, d2=-0.25, c1s=0.0)
            else:
                o.update(cx=float(rng.uniform(1, 8)), d1=float(rng.uniform(1, 8)), d2=float(-rng.uniform(1, 8)), c1s=float(rng.uniform(1, 8)))
            return o
        for nx in self.NX:
            for nz in self.EXACT_NZ:
                yield Case("schur", "%dx%d" % (nz, nx), "exact", partial(build, nz, nx, "exact"), extra=dict(nz=nz, cost=nz * nx))
            for nz, form in PinvApply.SIZES:
                yield Case("schur", "%dx%d" % (nz, nx), "rounded", partial(build, nz, nx, "rounded"), extra=dict(nz=nz, form=form, cost=nz * nx))

    def ref(self, mut=None, **a):
        nz, nx = a.pop("nz"), a.pop("nx")
        pb, out = schur(mut=None if mut == "perturb" else mut, **a)
        if mut == "perturb":
            out = pc.perturb(out)
        return pb, out, a["X"].copy()

    def check(self, impl, c):
        a = c.args
        nz, nx = a["nz"], a["nx"]
        P, out, X_after = impl(**a)
        out = np.asarray(out).reshape(-1); P = np.asarray(P).reshape(-1)
        assert_exact(self.name + " (input)", c, np.asarray(X_after).reshape(-1)[:nz * nx], a["X"].reshape(-1))
        ops = {k: v for k, v in a.items() if k not in ("nz", "nx")}
        aX, aD = np.abs(a["X"]), np.abs(a["D0"])
        S_st = stencil(aX, aD, abs(a["cp"]), abs(a["cm"]), abs(a["cx"]), 0.0, None)
        if c.kind == "exact":
            assert_below_2_53(S_st)
            _, want = schur(**ops)
            assert_exact(self.name, c, out[:nz * nx], want.reshape(-1))
        else:
            pb, want = schur(**_as(CLD, ops))
            g_abs = gather(aX, abs(a["d1"]), abs(a["d2"]))
            bp = PinvApply.bound(nz, a["bb"], a["sinv"], g_abs, extra_terms=2)
            assert_bounded(self.name + " (P)", c, P[:2 * nz], pb, bp)
            S = S_st.copy()
            N1, N2 = factor(nz)
            Sp = bp / pc.cbound(pinv_terms(N1, N2) + 2, 1.0)
            S[0] += abs(a["c1s"]) * Sp[:nz]; S[nx - 1] += abs(a["c1s"]) * Sp[nz:]
            assert_bounded(self.name, c, out[:nz * nx].reshape(nx, nz), want, pc.cbound(pinv_terms(N1, N2) + 2 + 1 + 5, S))
        for buf, n in ((out, nz * nx), (P, 2 * nz)):
            if len(buf) > n:
                _tail_intact(self.name, c, buf, n)
        return 1


REGION_SIZES = [(64, 4), (64, 64), (96, 3), (8, 1)]


class RegionMeans(Checker):
    """impl(nz, nx, N, X) -> out (N + 4, N).  exact: L a power of two, so both weights 1 / L are exact and so is their product
    with an integer sum below 2^53"""
    name = "nep_wep_region_means"
    mutants = ("x_offset", "boundary_weight", "z_last_row", "perturb")

    def cases(self):
        def build(nz, N):
            rng = _rng(self.name, nz, N)
            return dict(nz=nz, nx=nz + 4, N=N, X=gint(rng, (nz + 4, nz), -64, 64))
        for nz, N in REGION_SIZES:
            yield Case("means", "nz%d_N%d" % (nz, N), "exact", partial(build, nz, N), extra=dict(cost=nz * nz))

    def ref(self, nz, nx, N, X, mut=None):
        out = means(X, N, None if mut == "perturb" else mut)
        return pc.perturb(out) if mut == "perturb" else out

    def check(self, impl, c):
        a = c.args
        L = a["nz"] // a["N"]
        assert L & (L - 1) == 0
        assert_below_2_53(np.abs(a["X"]).sum())
        got = np.asarray(impl(**a)).reshape(-1)
        n = a["N"] * (a["N"] + 4)
        assert_exact(self.name, c, got[:n], means(a["X"], a["N"]).reshape(-1))
        if len(got) > n:
            _tail_intact(self.name, c, got, n)
        return 1


class RegionExpand(Checker):
    """impl(nz, nx, N, alpha, Ksc, dd1, dd2) -> (Y (nx, nz), eb (2 nz)); integer alpha, Ksc, dd1, dd2: every product is exact"""
    name = "nep_wep_region_expand"
    mutants = ("x_offset", "rx_plus", "dd_plus", "perturb")

    def cases(self):
        def build(nz, N):
            rng = _rng(self.name, nz, N)
            return dict(nz=nz, nx=nz + 4, N=N, alpha=gint(rng, (N + 4, N), -64, 64), Ksc=gint(rng, (nz + 4, nz), -64, 64), dd1=5.0, dd2=-3.0)
        for nz, N in REGION_SIZES + [(15, 5)]:
            yield Case("expand", "nz%d_N%d" % (nz, N), "exact", partial(build, nz, N), extra=dict(cost=nz * nz))

    def ref(self, nz, nx, N, alpha, Ksc, dd1, dd2, mut=None):
        Y, eb = expand(alpha, Ksc, dd1, dd2, None if mut == "perturb" else mut)
        return (pc.perturb(Y) if mut == "perturb" else Y), eb

    def check(self, impl, c):
        a = c.args
        nz, nx = a["nz"], a["nx"]
        l1 = lambda z: np.abs(np.real(z)) + np.abs(np.imag(z))              # |Re|, |Im| of a product <= the product of these
        for S in expand(l1(a["alpha"]), l1(a["Ksc"]), abs(a["dd1"]), abs(a["dd2"])):
            assert_below_2_53(S)
        Y, eb = impl(**a)
        Y = np.asarray(Y).reshape(-1); eb = np.asarray(eb).reshape(-1)
        wY, web = expand(a["alpha"], a["Ksc"], a["dd1"], a["dd2"])
        assert_exact(self.name + " (Y)", c, Y[:nz * nx], wY.reshape(-1))
        assert_exact(self.name + " (eb)", c, eb[:2 * nz], web)
        for buf, n in ((Y, nz * nx), (eb, 2 * nz)):
            if len(buf) > n:
                _tail_intact(self.name, c, buf, n)
        return 1


SMW_MUTANTS = ("last_x", "b_sign", "lane_carry", "x_offset", "boundary_weight", "z_last_row", "rx_plus", "dd_plus", "no_reverse", "bb_conj",
               "sinv_halves", "pb_last")


class SmwMatrix(Checker):
    """impl(o, N) -> M, (mm, mm) with M[kappa] = column kappa of the device matrix; o: the operands of smw_operands (+ G for the mode
    form).  Yardstick per matrix column."""
    mutants = SMW_MUTANTS
    SIZES = [(15, 3), (15, 15), (165, 3), (255, 5)]

    def __init__(self, modes):
        self.modes = modes
        self.name = "nep_wep_smw_matrix_modes" if modes else "nep_wep_smw_matrix"
        if modes:
            self.mutants = SMW_MUTANTS + ("batch_offset",)

    def cases(self):
        for nz, N in self.SIZES:
            yield Case("smw_matrix", "nz%d_N%d" % (nz, N), "measured", partial(smw_operands, nz),
                       extra=dict(nz=nz, nx=nz + 4, N=N, seg=seg_of(nz + 4), cost=nz * nz * N * (N + 4)))

    def ref(self, o, N, mut=None):
        return smw_matrix(o, N, mut)

    def check(self, impl, c):
        o, N = c.args, c.extra["N"]
        if self.modes:
            o["G"] = mode_means_matrix(c.extra["nz"], N)
        M = impl(o, N)
        ref, ref64 = _matrix_refs(c.extra["nz"], N, o)
        assert_measured(self.name, c, M, ref, ref64)
        return 1


_REFS = {}


def _matrix_refs(nz, N, o):
    """extended and float64 SMW matrix of a case, computed once and shared by the two checkers (never modified)"""
    if (nz, N) not in _REFS:
        ref = smw_matrix(_as(CLD, o), N); ref64 = smw_matrix(_as(C128, o), N)
        ref.setflags(write=False); ref64.setflags(write=False)
        _REFS[(nz, N)] = (ref, ref64)
    return _REFS[(nz, N)]


class SmwApply(Checker):
    """impl(o, calls) -> list of results; o: operands of the grid (one sylv / pinv handle pair serves every call), calls: list of
    (N, MinvH (mm, mm) with row i = column i of the device block, G (N, nz), R (nx, nz)).  Yardstick per grid column."""
    name = "nep_wep_smw_apply"
    mutants = SMW_MUTANTS + ("alpha_plain", "second_sign")
    # nz -> the sequence of N on one handle (1443: N = 3, 13, 3 -- d_T2 is reallocated on a change of N), SEG, form of P^{-1}
    SIZES = [(15, (3, 5, 15), 1, "sym"), (105, (7,), 2, "sym"), (165, (3, 11), 4, "sym"), (255, (5,), 8, "sym"), (525, (5,), 16, "sym"),
             (1023, (3,), 32, "sym"), (1443, (3, 13, 3), 32, "plain1024")]

    def cases(self):
        for nz, Ns, seg, pform in self.SIZES:
            yield Case("smw_apply", "nz%d" % nz, "measured", partial(smw_operands, nz),
                       extra=dict(nz=nz, nx=nz + 4, Ns=Ns, seg=seg, pinv=pform, cost=nz * nz * 40))

    @staticmethod
    def calls(nz, Ns):
        """one right-hand side block per grid (its first solve C = Linv R is shared by the references of every N)"""
        out = []
        made = {}
        R = grand(_rng("smw_rhs", nz), (nz + 4, nz))
        for N in Ns:
            if N not in made:
                mm = N * (N + 4)
                made[N] = (N, grand(_rng("smw_call", nz, N), (mm, mm)) / np.sqrt(mm), mode_means_matrix(nz, N), R)
            out.append(made[N])
        return out

    def ref(self, o, calls, mut=None):
        return [smw_apply(o, N, MinvH, R, mut) for N, MinvH, G, R in calls]

    def check(self, impl, c):
        o = c.args
        calls = self.calls(c.extra["nz"], c.extra["Ns"])
        outs = impl(o, calls)
        assert len(outs) == len(calls)
        refs = {}
        R = calls[0][3]
        oL = _as(CLD, o)
        CL, C64 = sylv(oL["d"], oL["b"], R.astype(CLD)), sylv(o["d"], o["b"], R)
        for (N, MinvH, G, R), got in zip(calls, outs):
            if N not in refs:
                refs[N] = (smw_apply(oL, N, MinvH.astype(CLD), None, C=CL), smw_apply(o, N, MinvH, None, C=C64), got)
            else:
                assert_exact(self.name + " (repeat after another N)", c, got, refs[N][2])
            assert_measured(self.name, c, got, refs[N][0], refs[N][1])
        return len(calls)


CHECKERS = {k.name: k for k in (SylvSolve(), PinvApply(), SchurMatvec(), RegionMeans(), RegionExpand(), SmwMatrix(False), SmwMatrix(True),
                                SmwApply())}

# refusals (test_gpu_wep_checkers.py asserts them on the library, test_host_wep_checkers.py on nep_wep_plan)
REFUSE_SYLV_ARG = [(7, 1), (7, 2049)]
REFUSE_PINV_NZ = 1921
REFUSE_SMW_EVEN = 60


def first_unstaged_nz(plan):
    """the smallest nz whose transform staging does not fit (plan(nz, nx, op) -> status)"""
    nz = 1
    while plan(nz, 5, OP_SYLV) != -5:
        nz += 1
        assert nz < 100000
    return nz
