"""Two-sided methods, host side: recognising the transposed problem (transpose_relation) and no CPU fallback."""
import numpy as np
import pytest
import scipy.sparse as sp

import nep_amd as na
from nep_amd import funcs


def _rand_sparse(n, density, seed, cplx=True):
    rng = np.random.default_rng(seed)
    A = sp.random(n, n, density=density, random_state=rng, format="csc")
    if cplx:
        B = sp.random(n, n, density=density, random_state=rng, format="csc")
        A = (A + 1j * B).tocsc()
    return A + sp.identity(n, format="csc")


def test_relation_qdep0_transposed():
    nep = na.nep_gallery("qdep0")
    nept = na.SPMF_NEP([A.T.tocsc() for A in nep.get_Av()], nep.get_fv())
    assert na.transpose_relation(nep, nept) == "T"
    assert na.transpose_relation(nep, nep) is None            # M(0) of qdep0 is not symmetric


def test_relation_complex_T_and_H():
    fv = [funcs.one(), funcs.ident(), funcs.Exp(-1.0)]
    Av = [_rand_sparse(30, 0.1, s) for s in range(3)]
    nep = na.SPMF_NEP(Av, fv)
    assert na.transpose_relation(nep, na.SPMF_NEP([A.T for A in Av], fv)) == "T"
    assert na.transpose_relation(nep, na.SPMF_NEP([A.conj().T for A in Av], fv)) == "H"
    # dense matrices are compared the same way
    Ad = [A.toarray() for A in Av]
    assert na.transpose_relation(na.SPMF_NEP(Ad, fv), na.SPMF_NEP([A.conj().T for A in Ad], fv)) == "H"


def test_relation_refuses_perturbed_reordered_or_other_functions():
    fv = [funcs.one(), funcs.ident(), funcs.Exp(-1.0)]
    Av = [_rand_sparse(30, 0.1, s) for s in range(3)]
    nep = na.SPMF_NEP(Av, fv)
    At = [A.T.tocsr() for A in Av]
    P = At[1].copy().tolil()
    P[3, 4] = P[3, 4] + 1e-15 * (1 + abs(P[3, 4]))
    assert na.transpose_relation(nep, na.SPMF_NEP([At[0], P.tocsr(), At[2]], fv)) is None          # one perturbed entry
    assert na.transpose_relation(nep, na.SPMF_NEP([At[1], At[0], At[2]], [fv[1], fv[0], fv[2]])) is None   # terms reordered
    other = [funcs.one(), funcs.ident(), funcs.Exp(-1.5)]
    assert na.transpose_relation(nep, na.SPMF_NEP(At, other)) is None                                # a different function
    assert na.transpose_relation(nep, na.SPMF_NEP(At, other), sigma=0.3, orders=2) is None
    assert na.transpose_relation(nep, na.SPMF_NEP(At[:2], fv[:2])) is None                           # fewer terms


def test_relation_equal_functions_by_value():
    """DEP builds new function objects on every get_fv call: equal derivatives at sigma recognise them"""
    nep = na.nep_gallery("dep0")
    nept = na.DEP([A.T.copy() for A in nep.A], nep.tauv)
    assert na.transpose_relation(nep, nept) is None                    # no shift: only identical objects count
    assert na.transpose_relation(nep, nept, sigma=0.2 + 0.1j, orders=2) == "T"
    nepd = na.DEP([A.T.copy() for A in nep.A], nep.tauv + np.array([0.0, 1e-4]))
    assert na.transpose_relation(nep, nepd, sigma=0.2 + 0.1j, orders=2) is None


def test_twosided_no_cpu_fallback_without_gpu():
    if na.device_count() > 0:
        pytest.skip("GPU present")
    nep = na.nep_gallery("dep0")
    nept = na.DEP([A.T.copy() for A in nep.A], nep.tauv)
    with pytest.raises((na.NepError, RuntimeError)):
        na.rfi(nep, nept, u=np.ones(5), v=np.ones(5))
    with pytest.raises((na.NepError, RuntimeError)):
        na.twosided_linsolvers(nep, nept, 0.0)
    with pytest.raises((na.NepError, RuntimeError)):
        na.DeviceLU(nep.compute_Mder(0.0)).transpose()
