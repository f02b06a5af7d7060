"""A NumPy restatement of safeguarded iteration (src/method_sgiter.jl:33-115) for Hermitian polynomial problems, built on dense
`eigh` and polynomial roots only, and the dense companion spectrum to compare with.  No part of the package under test is used."""
import numpy as np
import scipy.linalg as sla
import scipy.sparse as sp

EPS = np.finfo(float).eps

# the four smallest eigenvalues of real_quadratic as published in src/gallery_extra/gallery_examples.jl:53-54
REAL_QUADRATIC_SMALLEST = 1.0e3 * np.array([-2.051741417993845, -0.182101627437811, -0.039344930222838, -0.004039879577113])

# overdamped_qep_sparse: the j-th largest eigenvalue (computed on the CPU: dense eigh and a Gershgorin-shifted shift-and-invert
# Lanczos in the eigen step gave the same values)
OVERDAMPED = {(65, 1): -0.06521566997472, (65, 2): -0.08359853261594, (65, 5): -0.11836368575992,
              (257, 1): -0.05510149433645, (257, 2): -0.06029368757883, (257, 5): -0.07620493876868}


def dense(A):
    return np.asarray(A.toarray() if sp.issparse(A) else A, dtype=float)


def real_quadratic_matrices():
    A0 = np.array([[4.0, 0, 1, 1], [0, 2, 1, 1], [1, 1, 6, -2], [1, 1, -2, 3]])
    A1 = np.array([[167.0, -140, 95, -131], [-140, 327, 54, 85], [95, 54, 235, -81], [-131, 85, -81, 181]])
    A2 = np.array([[2.0, 1, -1, -1], [1, 5, -3, 2], [-1, -3, 3, 0], [-1, 2, 0, 3]])
    return [A0, A1, A2]


def overdamped_matrices(n):
    """the recipe of the gallery problem overdamped_qep_sparse, written out again"""
    i = np.arange(n, dtype=float)
    A0 = np.diag(2.5 + 2.0 * i / n) - np.diag(np.ones(n - 1), 1) - np.diag(np.ones(n - 1), -1)
    A1 = np.diag(9.0 + 3.0 * np.sin(0.37 * i) ** 2)
    for r in range(n - 2):
        A1[r, r + 2] = A1[r + 2, r] = 0.7 * np.cos(r)
    return [A0, A1, np.eye(n)]


def companion_eigenvalues(Av):
    """all eigenvalues of sum_i lam^i A_i from the dense first companion form"""
    Av = [dense(A) for A in Av]
    d, n = len(Av) - 1, Av[0].shape[0]
    A = np.zeros((n * d, n * d)); E = np.eye(n * d)
    A[:n * (d - 1), n:] = np.eye(n * (d - 1))
    for i in range(d):
        A[n * (d - 1):, n * i:n * (i + 1)] = -Av[i]
    E[n * (d - 1):, n * (d - 1):] = Av[d]
    return sla.eigvals(A, E)


def M(Av, lam):
    return sum(lam ** i * dense(A) for i, A in enumerate(Av))


def choose(lam_vec, lam_min, lam_max):
    lam_vec = np.real(lam_vec)
    if np.isnan(lam_min) and np.isnan(lam_max):
        return float(lam_vec.min())
    inside = lam_vec[(lam_vec <= lam_max) & (lam_vec >= lam_min)]
    assert len(inside) == 1, (lam_vec, lam_min, lam_max)
    return float(inside[0])


def sgiter_dense(Av, j, lam_min=np.nan, lam_max=np.nan, lam=0.0, tol=100 * EPS, maxit=100):
    """(lam, v, iterations): the eigenvector of the j-th smallest eigenvalue of M(lam_k) by eigh, all roots of the Rayleigh
    functional v^T M(lam) v by np.roots, the minimum root (no interval) or the one root inside the interval; stops on
    ||M(lam) v|| / (sum_i |lam|^i ||A_i||_F) < tol, the backward error of an SPMF"""
    Av = [dense(A) for A in Av]
    fro = [np.linalg.norm(A) for A in Av]
    lam = float(lam)
    for k in range(1, maxit + 1):
        w, V = np.linalg.eigh(M(Av, lam))
        v = V[:, j - 1]
        a = np.array([v @ A @ v for A in Av])
        lam = choose(np.roots(a[::-1]), lam_min, lam_max)
        err = np.linalg.norm(M(Av, lam) @ v) / sum(abs(lam) ** i * f for i, f in enumerate(fro))
        if err < tol:
            return lam, v, k
    raise AssertionError("the restatement did not converge: lam = %r, err = %.3e" % (lam, err))
