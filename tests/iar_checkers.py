"""Problem generator, float64 reference, mutants and the check for the device infinite-Arnoldi step chain (csrc/driver.hip:
nep_iar_create / nep_iar_step / nep_iar_steps / nep_iar_steps_graph / nep_iar_wait / nep_iar_stream_wait).  Style and helpers of
tests/lineig_checkers.py: `check_chain(case, out)` judges what a chain of steps left behind (`out` = the buffers after the chain);
test_gpu_iar_checkers.py fills `out` through the raw C ABI, test_host_iar_checkers.py from the NumPy model `ref_steps` and its mutants.

All inputs are data.  The C ABI takes the matrices, the LU handle, the coefficient table and the basis as data, and the checker
chooses all four: in a natural run block j of a basis column decays like 1 / j!, the late rows of a derivative table vanish, and a
step that drops the last coefficient row or mis-scales the last shifted block changes nothing a driver-level test can see.  Here
  problem(n, mt, values)   seeded sparse A_0 .. A_{mt-1} (about 4 entries per row, A_0 with the diagonal 8 + N(0, 1)), cf_0 = 1,
                           |cf_t| in [0.5, 1.5] / mt with a random phase, M0 = sum_t cf_t A_t (what the LU handle factorises)
  table(m, mt)             Ctab, m x mt random complex of modulus about 1 (row j-1 multiplies block j-1 of the source column)
  seeded_basis(...)        columns 0 .. k0-1 random, column j non-zero only in the rows < (j + 1) n, orthonormalised by two passes
                           of Gram-Schmidt (which keeps the staircase); everything else in the (m + 1) x ldv buffer exactly zero
so that every row of the table, every block of the source column and every term carries weight at every step.

The relation of step k, evaluated in np.clongdouble from the device's own V and H.  Y = reshape(V[0:nk, k-1], n, k) (block j of
column k-1 is column j of Y), (h, beta) the delivered row k-1, W = V[0:n(k+1), 0:k+1] [h; beta]:
    block 0                 R0 = M0 W[0:n] + sum_t A_t (Y Ctab[0:k, t])
    block j, 1 <= j <= k    Rj = W[jn:(j+1)n] - Y[:, j-1] / j
Bounds (cbound of primitive_checkers.py; nothing is fitted to a device result):
    block 0, Frobenius norm per step:   ||R0|| <= ||cbound(3n + k + mt + 8, |M0| (|V| |[h; beta]|)[0:n] + sum_t |A_t| |Y| |Ctab[0:k, t]|)||
        3n: Higham's componentwise backward error gamma_{3n} |L| |U| of a triangular-factor solve (Theorem 9.4), taken at
        |L| |U| ~ |M0| as test_expansion_rows_satisfy_the_krylov_relation does; k: the coefficient product; mt: the terms; 8: the
        update and the usual slack.
    shifted blocks, entrywise:          |Rj| <= cbound(k + 5, (|V| |[h; beta]|)[block j] + |Y[:, j-1]| / j)
The largest ratios seen are recorded in primitive_checkers.RATIOS["<tag> block0"] and ["<tag> shift"].

Structure the check holds fixed: beta real and positive; passes in {1, 2} and flags == 0; row k-1 of dH exactly zero beyond entry
k + 3; rows of steps never issued exactly zero; the pinned row as read right behind nep_iar_wait(k) equal to the device row bit for
bit; column k of V exactly zero in the rows >= (k + 1) n and in the ldv padding; the seeded columns bit-identical; the sentinels behind
the 3n work block, behind V and behind dH unchanged; ||V^H V - I||_2 <= 1e-12 over the columns present (the level of orth_checkers).

The one write beyond column k (decided from csrc/driver.hip, and stated in the header): on the fused path -- NEP_IAR_FUSE_VC != 0 and
mt <= 4, where step k's last kernel nep_orth_dev_iar_next forms step k + 1's coefficient product and block shift -- every step
k < m leaves the shifted blocks of column k + 1, rows n .. (k + 2) n - 1, equal to V[0:(k+1)n, k] divided blockwise by 1 .. k + 1
within cbound(1, .); rows 0 .. n - 1 of that column and every later column stay exactly zero.  On the unfused path (mt > 4 or
NEP_IAR_FUSE_VC=0) and behind the last step k = m every column beyond k is exactly zero.  The check requires exactly this.

Omega record (four doubles at the complex entries k + 2, k + 3 of the row).  With h_cabs / h_cf and refine_steps = r: the slots
0 .. r hold finite values in (0, 1), the later slots exactly 0; with r | 0x100 slot r is exactly 0 for k % 8 != 0 and non-zero for
k % 8 == 0; without h_cabs / h_cf all four are 0.  Values are not compared (nep_cw_backward_error has its own checker).
One exception, found with the float64 model: at n = 3 a refined iterate can solve the system with a residual that is exactly zero in
all three rows, so its omega IS 0 (the model records 0 in several chains of the list, and so does the device: slot 1 of step 9 of
n3_mt1_real_k9+2_orth0_r2s_pad0_nofuse, and slots of two more n = 3 chains, while the other slots of those chains are positive).
For n < 64 a recorded slot may therefore be +0; from n = 64 on (no set of 64 residuals is ever all zero) it must be positive.  The slot of the kept iterate under 0x100 at
k % 8 == 0 ("non-zero") falls under the same rule.
"""
from functools import lru_cache

import numpy as np
import scipy.sparse as sp
import scipy.sparse.linalg as spla

from primitive_checkers import C128, CLD, SENT, RATIOS, _seed, cbound, grand      # noqa: F401

M = 24                                              # steps the handles are created for
SKIP_FINAL = 0x100
ORTH_TOL = 1e-12
TAIL = 8                                            # sentinels behind the 3n work block
TAG = "nep_iar_step"
OMEGA_POSITIVE_FROM = 64                            # see "Omega record" above

# ---- the case list ---------------------------------------------------------------------------------------------------------------
F_N = [3, 65, 257]                                  # below a wave; column ends inside tiles; odd
F_MT = [1, 4, 5]                                    # 4 / 5 bracket the fused hand-over
F_VAL = ["real", "complex"]                         # nep_cw_resid_dev forks on valbytes == 8
F_CHAIN = [(1, 3), (2, 2), (8, 2), (9, 2), (16, 2), (17, 2), (23, 2)]      # the first step on both sides of K1's k = 1 / 2..8 / 9..16 / > 16
F_ORTH = [0, 1]                                     # DGKS / CGS
F_REFINE = [(0, False), (0, True), (1, True), (3, True), (2 | SKIP_FINAL, True)]      # (refine_steps, h_cabs / h_cf given)
F_PAD = [0, 5]                                      # ldv = n (m + 1) + pad
F_FUSE = [True, False]                              # NEP_IAR_FUSE_VC default / 0 (read at create time)
FACTORS = [F_N, F_MT, F_VAL, F_CHAIN, F_ORTH, F_REFINE, F_PAD, F_FUSE]
FACTOR_NAMES = ["n", "mt", "values", "chain", "orth", "refine", "pad", "fuse"]


class ChainCase:
    def __init__(self, n, mt, values, chain, orth, refine, pad, fuse, m=M):
        self.n, self.mt, self.values, (self.k0, self.count), self.orth = n, mt, values, chain, orth
        (self.refine, self.record), self.pad, self.fuse, self.m = refine, pad, fuse, m
        self.ldv = n * (m + 1) + pad
        self.key = (n, mt, values, chain, orth, refine, pad, fuse)

    @property
    def fused(self):
        """the handle keeps dWT: step k < m ends in nep_orth_dev_iar_next and hands its products over"""
        return self.fuse and self.mt <= 4

    @property
    def steps(self):
        return range(self.k0, self.k0 + self.count)

    def fork(self, k):
        """the branches step k of this chain takes, for assertion messages"""
        entry = "nep_spmv_wt on the hand-over" if self.fused and k > self.k0 else "nep_mlincomb_dev_shift"
        last = "nep_orth_dev_iar_next" if self.fused and k < self.m else ("nep_orth_dev_mirror (last step)" if k == self.m else "nep_orth_dev_mirror")
        return "%s -> %s, %s, refine_steps %d%s, %s" % (entry, last, "fused" if self.fused else "unfused", self.refine & 0xff,
                                                         "|0x100" if self.refine & SKIP_FINAL else "", "omegas recorded" if self.record else "no h_cabs")

    def __repr__(self):
        return "n%d_mt%d_%s_k%d+%d_orth%d_r%s%s_pad%d_%s" % (self.n, self.mt, self.values, self.k0, self.count, self.orth,
                                                             "%d" % (self.refine & 0xff) + ("s" if self.refine & SKIP_FINAL else ""),
                                                             "" if self.record else "n", self.pad, "fuse" if self.fuse else "nofuse")


def covering_cases():
    """a covering design, not the full product of 5040.  First the forks of the chain itself: every (mt, chain) with the default
    NEP_IAR_FUSE_VC, and mt 1 and 4 with every chain under NEP_IAR_FUSE_VC=0 (the other factors filled by rotation).  Then, until
    every pair of values of two different factors occurs, the chain that holds the most pairs not yet seen; among equals the
    one whose values have been used least (so that the list does not pile up on the first value of every factor)"""
    sizes = [len(F) for F in FACTORS]
    grid = np.stack(np.meshgrid(*[np.arange(s) for s in sizes], indexing="ij"), axis=-1).reshape(-1, len(sizes))
    off, cols = 0, []
    for a in range(len(sizes)):
        for b in range(a + 1, len(sizes)):
            cols.append(off + grid[:, a] * sizes[b] + grid[:, b])
            off += sizes[a] * sizes[b]
    cols = np.stack(cols, axis=1)                                        # candidate x factor pair -> index of the value pair
    open_ = np.ones(off, dtype=bool)
    used = [np.zeros(s, dtype=np.int64) for s in sizes]
    picked = []

    def take(i):
        picked.append(tuple(int(v) for v in grid[i]))
        open_[cols[i]] = False
        for f, v in enumerate(grid[i]):
            used[f][v] += 1

    t = 0
    for fuse, mts in ((0, (0, 1, 2)), (1, (0, 1))):
        for mt in mts:
            for ch in range(len(F_CHAIN)):
                ix = [(t + 3 * f) % s for f, s in enumerate(sizes)]
                ix[1], ix[3], ix[7] = mt, ch, fuse
                take(int(np.ravel_multi_index(ix, sizes)))
                t += 1
    while open_.any():
        gain = open_[cols].sum(axis=1)
        load = sum(used[f][grid[:, f]] * sizes[f] for f in range(len(sizes)))      # usage relative to an even spread
        take(int(np.lexsort((load, -gain))[0]))
    seen, out = set(), []
    for ix in picked:
        if ix not in seen:
            seen.add(ix)
            out.append(ChainCase(*[F[i] for F, i in zip(FACTORS, ix)]))
    return out


# ---- inputs ----------------------------------------------------------------------------------------------------------------------
class Problem:
    pass


@lru_cache(maxsize=None)
def problem(n, mt, values):
    """seeded A_0 .. A_{mt-1} (csr; float64 data for values == "real"), cf, cabs = |cf|, M0 = sum_t cf_t A_t (csc, complex)"""
    assert values in ("real", "complex")
    rng = np.random.default_rng(_seed("iar problem %d.%d.%s" % (n, mt, values)))
    p = Problem()
    p.n, p.mt, p.values = n, mt, values
    p.A = []
    for t in range(mt):
        A = sp.random(n, n, density=min(1.0, 4.0 / n), random_state=rng, data_rvs=rng.standard_normal, format="csr")
        if values == "complex":
            A = A.astype(C128)
            A.data = A.data + 1j * rng.standard_normal(A.nnz)
        if t == 0:
            A = (A + sp.diags(8.0 + rng.standard_normal(n))).tocsr()
        A.sum_duplicates(); A.sort_indices()
        assert A.dtype == (np.float64 if values == "real" else C128)
        p.A.append(A)
    cf = (0.5 + rng.random(mt)) / mt * np.exp(2j * np.pi * rng.random(mt))
    cf[0] = 1.0
    p.cf = cf.astype(C128)
    p.cabs = np.abs(p.cf)
    p.M0 = sp.csc_matrix(sum(c * A.astype(C128) for c, A in zip(p.cf, p.A)))
    return p


@lru_cache(maxsize=None)
def _dense(n, mt, values):
    """(M0, |M0|, [A_t], [|A_t|]) dense in extended precision, and the float64 factorisation of the reference"""
    p = problem(n, mt, values)
    Ad = [A.toarray().astype(CLD) for A in p.A]
    M0 = sum(CLD(c) * A for c, A in zip(p.cf, Ad))
    return M0, np.abs(M0), Ad, [np.abs(A) for A in Ad], spla.splu(p.M0)


def table(m, mt, seed="iar table"):
    """Ctab (m x mt); the device block is its column-major image with ldc = m"""
    return grand(np.random.default_rng(_seed("%s %d.%d" % (seed, m, mt))), (m, mt))


def seeded_basis(n, m, k0, ldv):
    """(m + 1) x ldv buffer, row j = basis column j: the columns 0 .. k0-1 random in their rows < (j + 1) n and orthonormal"""
    rng = np.random.default_rng(_seed("iar basis %d.%d.%d.%d" % (n, m, k0, ldv)))
    V = np.zeros((m + 1, ldv), dtype=C128)
    for j in range(k0):
        V[j, :(j + 1) * n] = grand(rng, (j + 1) * n)
        for _ in range(2):
            V[j] -= (np.conj(V[:j]) @ V[j]) @ V[:j]
        V[j] /= np.linalg.norm(V[j])
    return V


def staircase_ok(V, n, k0):
    rows = np.arange(V.shape[1])[None, :]
    limit = np.where(np.arange(V.shape[0]) < k0, (np.arange(V.shape[0]) + 1) * n, 0)[:, None]
    return not V[rows >= limit].any() and all(V[j, (j + 1) * n - 1] != 0 for j in range(k0))


def case_inputs(c):
    """(problem, Ctab, V0) of a case; the same arrays for equal arguments"""
    return problem(c.n, c.mt, c.values), table(c.m, c.mt), seeded_basis(c.n, c.m, c.k0, c.ldv)


def natural_table(m, mt, cf, tau):
    """the table of f_t(lam) = cf_t exp(-tau_t lam) at sigma = 0: row j-1 = f_t^(j)(0) / j (what derivative_table delivers)"""
    j = np.arange(1, m + 1)[:, None]
    return (cf[None, :] * (-tau[None, :]) ** j / j).astype(C128)


# ---- the float64 model and its mutants -------------------------------------------------------------------------------------------
MUTANTS = ("drop_last_row", "no_minus", "div_off", "last_block_unshifted", "stale_wt", "active_short", "h_row_shifted", "mirror_stale")


def mutant_applies(mut, c):
    """where a mutant can differ from the model: stale_wt needs a second step (the first step of a chain has no earlier product);
    every other mutant applies to every chain (drop_last_row at k = 1 forms no product at all, active_short at k = 1 projects
    on nothing)"""
    return c.count >= 2 if mut == "stale_wt" else True


def _omega(p, x, z, res):
    den = sum(ca * (abs(A) @ np.abs(x)) for ca, A in zip(p.cabs, p.A)) + np.abs(z)
    return float(np.max(np.abs(res) / den))


def ref_steps(prob, Ctab, V, k0, count, orth, mut=None, refine=0, record=True, fused=False):
    """the steps k0 .. k0 + count - 1 in float64 NumPy on a copy of V.  Returns dict(V, dH, pin, waited, tail): the basis buffer, the
    device H block, the pinned block, the pinned rows as read behind the wait for each step, the sentinels behind the work block"""
    p, n = prob, prob.n
    m = V.shape[0] - 1
    lu = _dense(p.n, p.mt, p.values)[4]
    V = V.copy()
    dH = np.zeros((m, m + 4), dtype=C128)
    pin = np.zeros((m, m + 4), dtype=C128)
    waited = {}
    skip, r = bool(refine & SKIP_FINAL), refine & 0xff
    WT_prev = None
    for k in range(k0, k0 + count):
        Y = V[k - 1, :n * k].reshape(k, n).T
        kk = k - 1 if mut == "drop_last_row" else k
        WT = Y[:, :kk] @ Ctab[:kk, :]
        if mut == "stale_wt" and WT_prev is not None:
            WT = WT_prev
        WT_prev = WT
        z = sum(A @ WT[:, t] for t, A in enumerate(p.A))
        x = lu.solve(z)
        om = np.zeros(4)
        for i in range(r):
            res = z - p.M0 @ x
            om[i] = _omega(p, x, z, res)
            x = x + lu.solve(res)
        if record and not (skip and k % 8 != 0):
            om[r] = _omega(p, x, z, z - p.M0 @ x)
        w = np.zeros(n * (k + 1), dtype=C128)
        w[:n] = x if mut == "no_minus" else -x
        for j in range(1, k + 1):
            if not (mut == "last_block_unshifted" and j == k):
                w[j * n:(j + 1) * n] = Y[:, j - 1] * (1.0 / (j + 1 if mut == "div_off" else j))
        Vk = V[:k, :n * (k + 1)]
        if mut == "active_short":                                        # the last block of every column is left out of the projections
            Vk = np.where(np.arange(n * (k + 1))[None, :] < (np.arange(k) * n)[:, None], Vk, 0)
        h = np.zeros(k, dtype=C128)
        passes = 0
        while True:
            cc = np.conj(Vk) @ w
            w = w - cc @ V[:k, :n * (k + 1)]
            h += cc
            passes += 1
            beta = np.linalg.norm(w)
            if orth != 0 or passes == 2 or not beta < np.sqrt(0.5) * np.linalg.norm(cc):
                break
        q = w * (1.0 / beta)
        V[k, :n * (k + 1)] = q
        row = np.zeros(m + 5, dtype=C128)
        s = 1 if mut == "h_row_shifted" else 0
        row[s:s + k] = h; row[s + k] = beta; row[s + k + 1] = passes
        if record:
            row[s + k + 2:s + k + 4] = om.view(C128)
        row = row[:m + 4]
        dH[k - 1] = row
        if mut != "mirror_stale":
            pin[k - 1] = row
        elif k > k0:
            pin[k - 1, :] = dH[k - 2]
        waited[k] = pin[k - 1].copy()
        if fused and k < m:
            sc = 1.0 / np.arange(1, k + 2)
            V[k + 1, n:n * (k + 2)] = (q.reshape(k + 1, n) * sc[:, None]).reshape(-1)
    return dict(V=V, dH=dH, pin=pin, waited=waited, tail=np.full(TAIL, SENT, dtype=C128))


def ref_out(c, mut=None):
    p, Ctab, V0 = case_inputs(c)
    return ref_steps(p, Ctab, V0, c.k0, c.count, c.orth, mut=mut, refine=c.refine, record=c.record, fused=c.fused)


# ---- the check -------------------------------------------------------------------------------------------------------------------
COUNTS = {}                                         # (factor, value) -> chains checked


def _bits(x):
    return np.ascontiguousarray(x).view(np.float64)


def _same(x, y):
    return np.array_equal(_bits(x), _bits(y))


def _note(tag, what, ratio):
    RATIOS["%s %s" % (tag, what)] = max(RATIOS.get("%s %s" % (tag, what), 0.0), ratio)


def step_ratios(c, inputs, V, row, k):
    """(block-0 ratio, (largest shifted-block ratio, its block, its row)) of step k from the delivered basis and row"""
    p, Ctab, _ = inputs
    n, mt = c.n, c.mt
    M0, M0a, Ad, Aa, _ = _dense(p.n, p.mt, p.values)
    hb = row[:k + 1].astype(CLD)
    Vk = V[:k + 1, :n * (k + 1)].astype(CLD)
    W = hb @ Vk
    Wa = np.abs(hb) @ np.abs(Vk)
    Y = V[k - 1, :n * k].reshape(k, n).T.astype(CLD)
    Ct = Ctab[:k].astype(CLD)
    R0 = M0 @ W[:n] + sum(Ad[t] @ (Y @ Ct[:, t]) for t in range(mt))
    S0 = M0a @ Wa[:n] + sum(Aa[t] @ (np.abs(Y) @ np.abs(Ct[:, t])) for t in range(mt))
    b0 = cbound(3 * n + k + mt + 8, S0.astype(np.float64))
    r0 = float(np.linalg.norm(np.abs(R0).astype(np.float64)) / np.linalg.norm(b0))
    jj = np.arange(1, k + 1).astype(np.longdouble)[:, None]
    Rj = W[n:].reshape(k, n) - Y.T / jj
    Sj = Wa[n:].reshape(k, n) + np.abs(Y.T) / jj
    rat = np.abs(Rj).astype(np.float64) / np.maximum(cbound(k + 5, Sj.astype(np.float64)), np.finfo(float).tiny)
    j, i = np.unravel_index(int(np.argmax(rat)), rat.shape)
    return r0, (float(rat[j, i]), int(j) + 1, int(i))


def check_chain(c, out, tag=TAG, inputs=None):
    """everything the module docstring lists, on the buffers a chain left behind.  out: V (m + 1 [+ sentinel rows]) x ldv, dH and pin
    m [+ sentinel rows] x (m + 4), waited {k: the pinned row read right behind the wait for step k}, tail (behind the work block)"""
    inputs = inputs or case_inputs(c)
    p, Ctab, V0 = inputs
    n, m, ldv, k0 = c.n, c.m, c.ldv, c.k0
    V, dH, pin = np.asarray(out["V"]), np.asarray(out["dH"]), np.asarray(out["pin"])
    klast = k0 + c.count - 1
    where = lambda k: "%r step k=%d (%s)" % (c, k, c.fork(k))
    assert V.shape[0] >= m + 1 and V.shape[1] == ldv and dH.shape[0] >= m and dH.shape[1] == m + 4 and pin.shape == dH.shape
    for name, buf, rows in (("V", V, m + 1), ("dH", dH, m), ("pinned block", pin, m)):
        assert _same(buf[rows:], np.full(buf[rows:].shape, SENT, dtype=C128)), "%r: the sentinels behind %s changed" % (c, name)
    assert _same(out["tail"], np.full(TAIL, SENT, dtype=C128)), "%r: the sentinels behind the 3n work block changed" % (c,)
    assert np.all(np.isfinite(_bits(V[:m + 1]))) and np.all(np.isfinite(_bits(dH[:m]))), "%r: non-finite results" % (c,)
    # ---- the basis outside the relation
    assert _same(V[:k0], V0[:k0]), "%r: a seeded column changed" % (c,)
    for k in c.steps:
        assert not V[k, n * (k + 1):].any(), "%s: column k non-zero at or beyond row (k + 1) n, or in the ldv padding" % where(k)
    if klast < m:
        nxt, src = V[klast + 1], V[klast, :n * (klast + 1)].reshape(klast + 1, n)
        assert not nxt[:n].any() and not nxt[n * (klast + 2):].any(), "%s: column k + 1 written outside its shifted blocks" % where(klast)
        got = nxt[n:n * (klast + 2)].reshape(klast + 1, n)
        if c.fused:
            jj = np.arange(1, klast + 2)[:, None]
            err = np.abs(got.astype(CLD) - src.astype(CLD) / jj.astype(np.longdouble)).astype(np.float64)
            bad = err > cbound(1, np.abs(src) / jj)
            assert not bad.any(), "%s: the shifted blocks left in column k + 1 are off in block %d (largest error %.3g)" \
                % (where(klast), int(np.argwhere(bad)[0][0]) + 1, float(err.max()))
            assert got.any(), "%s: the fused path left no shifted blocks in column k + 1" % where(klast)
        else:
            assert not got.any(), "%s: the unfused path wrote into column k + 1" % where(klast)
        assert not V[klast + 2:m + 1].any(), "%r: a column beyond k + 1 was written" % (c,)
    # ---- the rows
    for j in range(m):
        if j + 1 not in c.steps:
            assert not dH[j].any() and not pin[j].any(), "%r: row %d of a step never issued is not zero" % (c, j)
    r, skip = c.refine & 0xff, bool(c.refine & SKIP_FINAL)
    for k in c.steps:
        row = dH[k - 1]
        assert _same(out["waited"][k], row), "%s: the pinned row behind the wait differs from the device row" % where(k)
        assert _same(pin[k - 1], row), "%s: the pinned row differs from the device row" % where(k)
        assert not row[k + 4:].any(), "%s: row k-1 non-zero beyond entry k + 3" % where(k)
        beta, word = row[k], row[k + 1]
        assert beta.imag == 0 and beta.real > 0, "%s: beta = %r is not real and positive" % (where(k), beta)
        assert word.real in (1.0, 2.0) and word.imag == 0, "%s: (passes, flags) = %r" % (where(k), word)
        om = _bits(row[k + 2:k + 4])
        if not c.record:
            assert not om.any(), "%s: omegas %r recorded without h_cabs / h_cf" % (where(k), om)
        else:
            kept_skipped = skip and k % 8 != 0
            for i in range(4):
                if i < r or (i == r and not kept_skipped):
                    lo_ok = om[i] > 0.0 or (n < OMEGA_POSITIVE_FROM and om[i] == 0.0 and not np.signbit(om[i]))
                    assert lo_ok and om[i] < 1.0, "%s: omega slot %d = %r is not in (0, 1)" % (where(k), i, om[i])
                else:
                    assert om[i] == 0 and not np.signbit(om[i]), "%s: omega slot %d = %r, want exactly 0" % (where(k), i, om[i])
    # ---- the relation, step by step (the first failing step is the message)
    for k in c.steps:
        r0, (rs, blk, i) = step_ratios(c, inputs, V[:m + 1], dH[k - 1], k)
        _note(tag, "block0", r0)
        _note(tag, "shift", rs)
        assert r0 <= 1.0, "%s: block 0, ||M0 W_0 + sum_t A_t (Y c_t)||_F / bound = %.3g" % (where(k), r0)
        assert rs <= 1.0, "%s: shifted block %d, row %d: |W_j - Y_{j-1} / j| / bound = %.3g" % (where(k), blk, i, rs)
    Vp = V[:klast + 1, :n * (klast + 1)].astype(CLD)
    G = (np.conj(Vp) @ Vp.T).astype(C128) - np.eye(klast + 1)
    orth = float(np.linalg.norm(G, 2))
    _note(tag, "orthogonality / 1e-12", orth / ORTH_TOL)
    if orth > ORTH_TOL:
        jbad = int(np.argmax(np.abs(G).max(axis=0)))
        raise AssertionError("%r: ||V^H V - I||_2 = %.3g over the columns 0 .. %d, worst column %d%s"
                             % (c, orth, klast, jbad, " (%s)" % c.fork(jbad) if jbad in c.steps else " (seeded)"))
    if tag == TAG:
        for name, v in zip(FACTOR_NAMES, c.key):
            COUNTS[name, v] = COUNTS.get((name, v), 0) + 1
