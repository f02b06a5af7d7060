"""The boundary-element NEP of the reference's gallery (src/gallery_extra/bem_hardcoded/): the Laplace eigenvalue problem on the
unit cube with a Fichera corner, discretised with one constant basis function per flat triangle.  M(lam) is dense and every entry
depends on lam, so the NEP is not a sum of a few fixed matrices: it is assembled, differentiated and applied by the kernels of
csrc/bem.hip (nep_bem_*), and only the mesh generator runs on the host.

`gen_ficheramesh(N)` ports genmesh.jl (same triangle order, same vertex order); `BEM_NEP(mesh)` is the reference's BEM_NEP
(bem_hardcoded.jl:15-37) with the interface the drivers here use: compute_Mder (host matrix, for the factorisations),
compute_Mder_dev (a batch of matrices that stays on the device), compute_Mlincomb and resid_norms (matrix-free), and the
derivative_table / lincomb_rowscale / lincomb_general hooks of the Krylov drivers.
"""
import ctypes as C

import numpy as np
import torch

from . import _lib
from ._lib import lib, check, hptr, c_vp, c_i64
from .nep import NEP, CDT, is_dev, to_dev, to_host, stream_ptr


class TriMesh:
    """n flat triangles: `vert` (n, 3, 3) = [triangle, vertex P1 / P2 / P3, coordinate], `area` (n,).  len() and slices work."""

    def __init__(self, vert, area):
        self.vert = np.ascontiguousarray(vert, dtype=np.float64).reshape(-1, 3, 3)
        self.area = np.ascontiguousarray(area, dtype=np.float64).reshape(-1)
        if len(self.area) != len(self.vert):
            raise ValueError("TriMesh: %d triangles but %d areas" % (len(self.vert), len(self.area)))

    def __len__(self):
        return len(self.area)

    def __getitem__(self, s):
        if not isinstance(s, slice):
            raise TypeError("TriMesh supports slices only")
        return TriMesh(self.vert[s], self.area[s])


# genmesh.jl:31-48 (1-based there): the fixed coordinate of each of the 15 patches, its value, the two free coordinates
_FIXDIM = (0, 1, 2, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2)
_FIXVAL = (0, 0, 0, 1, 1, 1, 0.5, 1, 1, 1, 0.5, 1, 1, 1, 0.5)
_FREE = ((1, 2), (2, 0), (0, 1)) + ((1, 2),) * 4 + ((2, 0),) * 4 + ((0, 1),) * 4
_TRI_LOW = ((0, 0, 1, 0), (1, 0, 1, 1), (1, 1, 0, 1), (0, 1, 0, 0))            # l < 4
_TRI_HIGH = ((0, 0, 0, 1), (0, 1, 1, 1), (1, 1, 1, 0), (1, 0, 0, 0))           # "for consistency with Effenberger"


def gen_ficheramesh(N):
    """genmesh.jl:12-113: the surface of the unit cube with the corner [1/2, 1]^3 cut out, N cells per edge (odd N is rounded up
    to even), four triangles around the centre of every cell: n = 24 N^2 triangles of area 1 / (4 N^2), in the reference's order"""
    N = int(N)
    if N % 2:
        N += 1
    nn = N // 2
    area = 0.25 / N / N
    grid = np.arange(N + 1) / N
    lo, hi, full = (1, nn), (nn + 1, N), (1, N)
    quads = [(lo, lo), (hi, lo), (lo, hi), (hi, hi)]
    nvals = [(full, full)] * 3 + quads * 3
    vert = []
    for l in range(15):
        f1, f2 = _FREE[l]
        (i0, i1), (j0, j1) = nvals[l]
        for ii in range(i0, i1 + 1):
            for jj in range(j0, j1 + 1):
                center = np.zeros(3)
                center[_FIXDIM[l]] = _FIXVAL[l]
                center[f1] = (grid[ii - 1] + grid[ii]) / 2
                center[f2] = (grid[jj - 1] + grid[jj]) / 2
                for a, b, c, d in (_TRI_LOW if l < 3 else _TRI_HIGH):
                    P1 = np.zeros(3); P1[_FIXDIM[l]] = _FIXVAL[l]
                    P3 = P1.copy()
                    P1[f1] = grid[ii + a - 1]; P1[f2] = grid[jj + b - 1]
                    P3[f1] = grid[ii + c - 1]; P3[f2] = grid[jj + d - 1]
                    vert.append((P1, center, P3))
    return TriMesh(np.array(vert), np.full(len(vert), area))


class BEM_NEP(NEP):
    """bem_hardcoded.jl:15-37 on the device.  `mesh`: a TriMesh (gen_ficheramesh, or any triangle list wrapped in one)."""

    def __init__(self, mesh, gauss_order=3):
        _lib.require_gpu()
        self.mesh = mesh
        self.gauss_order = int(gauss_order)
        self.n = len(mesh)
        vert = np.ascontiguousarray(mesh.vert, dtype=np.float64).reshape(self.n, 9)
        area = np.ascontiguousarray(mesh.area, dtype=np.float64)
        h = c_vp()
        check(lib.nep_bem_create(self.n, hptr(vert), hptr(area), self.gauss_order, C.byref(h)))
        self.h = h
        info = (c_i64 * 4)()
        check(lib.nep_bem_info(self.h, info))
        self.device_bytes = int(info[2])

    def __del__(self):
        try:
            if getattr(self, "h", None):
                lib.nep_bem_destroy(self.h)
                self.h = None
        except Exception:
            pass

    def issparse(self):
        return False

    def static_part(self):
        """S0, the lam-independent singular part (n x n, real, mirrored), on the host"""
        out = torch.empty((self.n, self.n), dtype=torch.float64, device="cuda")
        check(lib.nep_bem_static(self.h, c_vp(out.data_ptr()), self.n, stream_ptr()))
        return out.cpu().numpy().T.copy()

    # ---- matrices
    def compute_Mder_dev(self, lams, der=0):
        """the block (len(lams), n, n) of M^(der)(lam_l) on the device; [l] is the matrix in either storage order (it is
        symmetric bit for bit)"""
        la = np.ascontiguousarray(np.atleast_1d(lams), dtype=np.complex128)
        n = self.n
        out = torch.empty((len(la), n, n), dtype=CDT, device="cuda")
        check(lib.nep_bem_assemble(self.h, len(la), hptr(la), int(der), c_vp(out.data_ptr()), n, n * n, stream_ptr()))
        return out

    def compute_Mder(self, lam, i=0):
        """M^(i)(lam) as a host ndarray: what every linear-solver route takes"""
        return self.compute_Mder_dev([lam], i)[0].cpu().numpy()

    def compute_Mder_batch(self, lams):
        """M(lam_b) of several shifts from one assembly pass, as a host array (B, n, n)"""
        return self.compute_Mder_dev(lams, 0).cpu().numpy()

    # ---- matrix-free products
    def _mlincomb(self, lam, k, a, startder, V, ldv, z):
        av = np.ascontiguousarray(a, dtype=np.complex128)
        assert len(av) >= k
        check(lib.nep_bem_mlincomb(self.h, _lib.cd(lam), int(k), hptr(av), int(startder),
                                   c_vp(V.data_ptr() if is_dev(V) else V), int(ldv), c_vp(z.data_ptr()), stream_ptr()))
        return z

    def compute_Mlincomb(self, lam, V, a=None, startder=0):
        """sum_j a_j M^(j + startder)(lam) v_j  (NEPCore.jl:111-160) in one matrix-free pass.  NumPy in -> NumPy out; device
        tensor ((k, n) column block or (n,) vector) in -> device tensor out.  V is not modified."""
        host = not is_dev(V)
        Vd = to_dev(V) if host else (V if V.dim() == 2 else V.reshape(1, -1))
        k = Vd.shape[0]
        a = np.ones(k) if a is None else np.asarray(a)
        if len(a) != k:
            raise ValueError("length of a must equal the number of columns of V")
        assert Vd.dtype == CDT and Vd.is_contiguous() and Vd.shape[1] >= self.n
        z = torch.empty(self.n, dtype=CDT, device="cuda")
        self._mlincomb(lam, k, a, startder, Vd, Vd.shape[1], z)
        return to_host(z.reshape(1, -1))[:, 0] if host else z

    def resid_norms(self, lams, QT):
        """(||M(lam_s) q_s||, ||q_s||, None) for the columns of the row-major block QT: one nep_bem_resid call"""
        from . import dense
        la = np.ascontiguousarray(lams, dtype=np.complex128)
        k = len(la)
        cols = dense.rowmajor_to_cols(QT, np.arange(k, dtype=np.int32))          # (k, n) column-major n x k
        Y = torch.empty((k, self.n), dtype=CDT, device="cuda")
        check(lib.nep_bem_resid(self.h, k, hptr(la), c_vp(cols.data_ptr()), cols.shape[1], c_vp(Y.data_ptr()), self.n, stream_ptr()))
        nr = np.empty(k); nq = np.empty(k)
        check(lib.nep_colnorms(self.n, k, c_vp(Y.data_ptr()), self.n, hptr(nr), stream_ptr()))
        check(lib.nep_colnorms(self.n, k, c_vp(cols.data_ptr()), cols.shape[1], hptr(nq), stream_ptr()))
        return nr, nq, None

    # ---- the hooks of the Krylov drivers (AbstractSPMF has the same three): nothing is tabulated, the derivatives at sigma come
    # out of the Horner loop of the kernel
    def derivative_table(self, sigma, m, rowscale=None):
        return {"sigma": complex(sigma), "m": int(m),
                "rowscale": None if rowscale is None else np.ascontiguousarray(rowscale, dtype=np.complex128)}

    def lincomb_rowscale(self, tab, k, V, ldv, z):
        """z = sum_{j=1..k} rowscale_j M^(j)(sigma) V[:, j-1]   (V: device address or tensor, leading dimension ldv)"""
        return self._mlincomb(tab["sigma"], k, tab["rowscale"][:k], 1, V, ldv, z)

    def lincomb_general(self, tab, G, V, k, ldv, z):
        """z = sum_{j<k} sum_q G[j, q] M^(q+1)(sigma) V[:, j]   (G: k x q host matrix): a diagonal G is one call on V itself,
        any other G one call on the q columns V G"""
        G = np.atleast_2d(np.asarray(G, dtype=np.complex128))
        if G.shape[0] == G.shape[1] and np.count_nonzero(G - np.diag(np.diag(G))) == 0:
            return self._mlincomb(tab["sigma"], k, np.diag(G), 1, V, ldv, z)
        from . import dense
        Y = dense.gemm_ts(V, G, k=k, rows=self.n, ldz=ldv)                      # (q, n)
        return self._mlincomb(tab["sigma"], G.shape[1], np.ones(G.shape[1]), 1, Y, Y.shape[1], z)
