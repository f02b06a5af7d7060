import sys, os; sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
for _v in ("OPENBLAS_NUM_THREADS", "OMP_NUM_THREADS"): os.environ.setdefault(_v, "8")
import numpy as np, scipy.sparse as sp, scipy.sparse.linalg as spla, torch, nep_amd as na
# randomized parity sweep of the C-ABI kernels against NumPy on ragged / degenerate sizes
rng = np.random.default_rng(int(sys.argv[1]) if len(sys.argv) > 1 else 0)
f = na.funcs
bad = 0
def chk(name, err, tol, info):
    global bad
    if not (err <= tol):
        bad += 1; print("FAIL", name, err, info, flush=True)
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))), "tests"))
import primitive_checkers as pc, test_gpu_primitives as tg
def prim_sweep(n, k, p, kk, mt):
    """one exact case per primitive at the iteration's sizes (n rows, k / p / kk columns), padded leading dimensions"""
    g = lambda *shape: pc.gint(rng, shape)
    run = lambda name, **a: pc.BY_NAME[name].check(tg.ADAPTERS[name], pc.Case("fuzz", "n%d_k%d_p%d_kk%d" % (n, k, p, kk), "exact", lambda: a))
    for name in ("nep_coldots", "nep_coldotsu"):
        run(name, rows=n, k=kk, X=pc.colmajor_buf(g(n, kk), n + 1), ldx=n + 1, Y=pc.colmajor_buf(g(n, kk), n + 2), ldy=n + 2)
    run("nep_colnorms", rows=n, k=kk, X=pc.colmajor_buf(g(n, kk), n + 1), ldx=n + 1)
    run("nep_nrm2", len=n, x=g(n))
    run("nep_rowmajor_colnorms", rows=n, k=kk, XT=pc.rowmajor_buf(g(n, kk), kk + 1), ld=kk + 1)
    cols = rng.integers(0, kk, kk + 1).astype(np.int32)
    run("nep_rowmajor_to_colmajor", rows=n, k=kk, src=pc.rowmajor_buf(g(n, kk), kk + 1), lds=kk + 1, cols=cols, ncols=len(cols),
        dst=np.full((n + 1) * len(cols) + 1, pc.SENT), ldd=n + 1)
    run("nep_rowdot", rows=n, k=k, A=pc.colmajor_buf(g(n, k), n + 1), lda=n + 1, B=pc.colmajor_buf(g(n, k), 2 * n), ldb=2 * n)
    run("nep_hadamard", rows=n, k=k, A=pc.colmajor_buf(g(n, k), n + 1, fill=pc.SENT), lda=n + 1, B=pc.colmajor_buf(g(n, k), 2 * n), ldb=2 * n)
    run("nep_axpy", len=n, alpha=complex(2, -3), x=np.append(g(n), pc.NAN), y=np.append(g(n), [pc.SENT] * 2))
    run("nep_scal", len=n, alpha=complex(2, -3), x=np.append(g(n), [pc.SENT] * 2))
    buf = np.full(2 * n * (k + 1) + 3, pc.SENT); buf[:n * k] = g(n * k)
    run("nep_iar_shift_scale", n=n, k=k, buf=buf, src_off=0, dst_off=n * (k + 1) + 1)
    N = int(rng.choice([0, 1, 2, 43]))
    run("nep_rk_bw", n=n, N=N, wc=np.append(g(n * (N + 1)), pc.NAN), wc_off=0, c=g(N), Bw=np.full(n * (N + 1) + 2, pc.SENT), bw_off=0)
    xy = np.append(g(n * (N + 1)), pc.SENT)
    run("nep_block_recur", n=n, N=N, a=pc.gint(rng, N, -2, 2), b=rng.choice(np.array([0, 1, -1, 1j, -1j]), N).astype(complex), y=xy, y_off=0,
        x=xy, x_off=0)
    run("nep_gemv_h", V=pc.colmajor_buf(g(n, k), n + 3), ldv=n + 3, rows=n, k=k, w=np.append(g(n), pc.NAN))
    for brm in (0, 1):
        ldb = (p if brm else k) + 2
        Bb = pc.rowmajor_buf(g(k, p), ldb, lead=3, trail=1) if brm else pc.colmajor_buf(g(k, p), ldb, lead=3, trail=1)
        yrm = int(rng.integers(0, 2))
        ldy = (p if yrm else n) + 1
        run("nep_gemm_ts_dev", Z=pc.colmajor_buf(g(n, k), n + 1, lead=2), z_off=2, ldz=n + 1, rows=n, k=k, B=Bb, b_off=3, ldb=ldb, b_rowmajor=brm,
            p=p, Y=np.full(1 + (n if yrm else p) * ldy + 1, pc.SENT), y_off=1, ldy=ldy, y_rowmajor=yrm)
    ta, tb = int(rng.integers(0, 3)), int(rng.integers(0, 3))
    m_, n_ = min(n, 130), p
    A = g(m_, n) if ta == 0 else g(n, m_); B = g(n, n_) if tb == 0 else g(n_, n)
    run("nep_zgemm_sk", transa=ta, transb=tb, m=m_, n=n_, k=n, alpha=complex(1, -2), A=pc.colmajor_buf(A, A.shape[0] + 1), lda=A.shape[0] + 1,
        B=pc.colmajor_buf(B, B.shape[0] + 1), ldb=B.shape[0] + 1, beta=complex(2, 1), C=pc.colmajor_buf(g(m_, n_), m_ + 1, fill=pc.SENT), ldc=m_ + 1,
        ksplit=int(rng.choice([1, 2, 7, 64])))
    if n >= 8:
        terms = pc.spmm_terms_matrices(min(n, 300), mt, bool(rng.integers(0, 2)), int(rng.integers(1 << 30)))
        nn, pp = terms[0].shape[0], int(rng.choice([1, 7, 64, 65, 129, 200, 256]))
        run("nep_spmm_terms", terms=terms, p=pp, XT=pc.rowmajor_buf(g(nn, pp * mt), pp * mt + 1), ldx=pp * mt + 1,
            ZT=np.full(nn * (pp + 1) + 1, pc.SENT), ldz=pp + 1)
for it in range(int(sys.argv[2]) if len(sys.argv) > 2 else 60):
    n = int(rng.choice([1, 2, 3, 5, 17, 64, 65, 257, 1000, 4099]))
    mt = int(rng.integers(1, 6))
    dens = float(rng.choice([0.0, 0.01, 0.2, 1.0])) if n < 300 else float(rng.choice([0.0, 0.002, 0.02]))
    cp = bool(rng.integers(0, 2))
    AA = []
    for i in range(mt):
        A = sp.random(n, n, dens, random_state=int(rng.integers(1 << 30)), format="csc")
        if cp and i % 2:
            A = A + 1j * sp.random(n, n, dens, random_state=int(rng.integers(1 << 30)), format="csc")
        AA.append(sp.csc_matrix(A))
    fv = [f.one(), f.ident(), f.Exp(-0.3), f.Monomial(2), f.ISqrt(1.0, 2.0)][:mt]
    nep = na.SPMF_NEP(AA, fv)
    k = int(rng.choice([1, 2, 7, 33, 100]))
    V = rng.standard_normal((n, k)) + 1j * rng.standard_normal((n, k))
    a = rng.standard_normal(k); a[rng.random(k) < 0.2] = 0
    lam = 0.3 + 0.2j
    z = nep.compute_Mlincomb(lam, V, a)
    ref = sum(sum(a[j] * fv[i].derivs(lam, k)[j] * (AA[i] @ V[:, j]) for j in range(k)) for i in range(mt))
    chk("K1", np.linalg.norm(z - ref), 1e-11 * max(1.0, np.linalg.norm(ref)), (n, mt, k, dens, cp))
    # K2
    kk = int(rng.choice([1, 3, 64, 130]))
    Q = rng.standard_normal((n, kk)) + 1j * rng.standard_normal((n, kk))
    lams = rng.standard_normal(kk) * 0.3 + 0.1j
    E = na.ResidualErrmeasure(nep)
    e = E.batch(list(lams), torch.from_numpy(np.ascontiguousarray(Q)).to("cuda"))
    er = np.array([np.linalg.norm(sum(fv[i].derivs(lams[s], 1)[0] * (AA[i] @ Q[:, s]) for i in range(mt))) / np.linalg.norm(Q[:, s]) for s in range(kk)])
    chk("K2", np.max(abs(e - er)), 1e-11 * max(1.0, er.max()), (n, mt, kk))
    # K6
    kq = min(k, n)
    Vq, _ = np.linalg.qr(rng.standard_normal((n, kq)) + 1j * rng.standard_normal((n, kq)))
    w = rng.standard_normal(n) + 1j * rng.standard_normal(n)
    Vd = na.to_dev(Vq); wd = na.to_dev(w)[0]
    h, beta, _ = na.orthogonalize_and_normalize(Vd, wd, kq) if n > kq else (None, None, None)
    if h is not None:
        wr = w - Vq @ (Vq.conj().T @ w); wr = wr - Vq @ (Vq.conj().T @ wr)
        chk("K6", abs(beta - np.linalg.norm(wr)), 1e-10 * max(1.0, np.linalg.norm(w)), (n, kq))
    # K7 / K9
    p = int(rng.choice([1, 2, 16, 17, 100]))
    B = rng.standard_normal((k, p)) + 1j * rng.standard_normal((k, p))
    Y = na.to_host(na.gemm_ts(na.to_dev(V), B))
    chk("K7", np.linalg.norm(Y - V @ B), 1e-11 * max(1.0, np.linalg.norm(V @ B)), (n, k, p))
    WT = torch.from_numpy(np.ascontiguousarray(V)).to("cuda"); YT = torch.from_numpy(np.ascontiguousarray(V @ B)).to("cuda")
    Cm = na.dense.gemm_h_rm(WT, YT, n, k, p)
    Cr = V.conj().T @ (V @ B)
    chk("K9", np.linalg.norm(Cm - Cr), 1e-11 * max(1.0, np.linalg.norm(Cr)), (n, k, p))
    # K5
    if n >= 2:
        A = sp.csc_matrix(sum(AA) + sp.identity(n) * (3.0 + mt), dtype=complex)
        nr = int(rng.choice([1, 3, 32]))
        Bm = rng.standard_normal((n, nr)) + 1j * rng.standard_normal((n, nr))
        try:
            lu = na.DeviceLU(A)
            X = na.to_host(lu.solve(na.to_dev(Bm)))
            chk("K5", np.linalg.norm(A @ X - Bm), 1e-9 * np.linalg.norm(Bm), (n, nr, lu.tail, lu.mid_rows))
        except np.linalg.LinAlgError:
            pass
    # ---- the driver-only primitives (BLAS-1 helpers, rk helpers, gemv_h, gemm_ts_dev, zgemm_sk, spmm_terms): Gaussian-integer
    # operands on the same ragged sizes, bit-for-bit against NumPy (tests/primitive_checkers.py has the references)
    try:
        prim_sweep(n, k, p, kk, mt)
    except AssertionError as e:
        bad += 1; print("FAIL primitive", str(e)[:300], flush=True)
print("done, failures:", bad)
