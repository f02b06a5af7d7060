"""Scalar functions f_i(lambda) of an SPMF with closed-form derivative tables.

The reference passes Julia closures that must work on scalars AND matrices and obtains scaled
derivatives by evaluating the matrix function of a bidiagonal matrix at every call
(src/NEPTypes.jl:993-1004, O(k^3) host work on the critical path; DerSPMF :1108-1128 caches it).
Here every function knows its derivatives in closed form, so the coefficient block
C[j,i] = a_j f_i^(j-1)(lambda) handed to the device kernel (include/nepmi355.h nep_mlincomb) costs
O(k) per function.  `matfun` gives the matrix function needed by compute_MM with a general S.
Dynamic range: derivatives reach 1e164 for gun at order 100 -> float64 only, and all
recurrences below are arranged to avoid intermediate overflow/underflow.
"""
import math

import numpy as np
import scipy.linalg as sla


class ScalarFun:
    """f: C -> C with derivatives."""

    def __call__(self, lam):
        return self.derivs(lam, 1)[0]

    def derivs(self, lam, k, scale=1.0):
        """array [scale^j * f^(j)(lam), j = 0..k-1] (complex128).  `scale` (chain-rule factor of an
        affine change of variable) is folded into the recurrences so that scale^j never appears alone:
        for gun, scale^j = 60500^j overflows at j = 65 while scale^j f^(j) stays below 1e165."""
        raise NotImplementedError

    def taylor(self, lam, k, scale=1.0):
        """array [scale^j f^(j)(lam) / j!, j = 0..k-1] (complex128): the Taylor coefficients of h -> f(lam + scale*h).  The
        closed-form classes below run recurrences that never form f^(j) or j! on their own -- derivs of gun overflows near
        order 170, where f^(j) grows like j!; the Taylor coefficients stay bounded.  Generic fallback: derivs, with the
        factorial divided in step by step."""
        d = np.array(self.derivs(lam, k, scale), dtype=np.complex128)
        for j in range(2, k):
            d[j:] /= j
        return d

    def matfun(self, S):
        """f(S) for a square matrix S (host, small)."""
        raise NotImplementedError

    def values(self, lams):
        """vectorised f(lam) over an array of points"""
        return np.array([self(l) for l in np.asarray(lams, dtype=np.complex128)], dtype=np.complex128)

    def affine(self, scale, shift):
        """g(lam) = f(scale*lam + shift)  (shift_and_scale, src/NEPTransformations.jl:92-105)"""
        return Affine(self, scale, shift)

    def __mul__(self, c):
        return Scaled(c, self)

    __rmul__ = __mul__

    def __neg__(self):
        return Scaled(-1.0, self)

    def real_on_reals(self):
        """True when f maps real arguments (scalars and real matrices) to real values with real derivatives -- what decides the
        element type of compute_Mder / compute_Mlincomb / compute_MM results for real input (test/compute_types.jl)"""
        return False


class Monomial(ScalarFun):
    """lam^p  (p=0: one(S); p=1: S)   src/types_poly.jl:83-98"""

    def __init__(self, p):
        self.p = int(p)

    def real_on_reals(self):
        return True

    def derivs(self, lam, k, scale=1.0):
        lam = complex(lam)
        out = np.zeros(k, dtype=np.complex128)
        for j in range(min(k, self.p + 1)):
            out[j] = (math.factorial(self.p) // math.factorial(self.p - j)) * lam ** (self.p - j) * scale ** j
        return out

    def taylor(self, lam, k, scale=1.0):
        lam = complex(lam)
        out = np.zeros(k, dtype=np.complex128)
        for j in range(min(k, self.p + 1)):
            out[j] = math.comb(self.p, j) * lam ** (self.p - j) * scale ** j
        return out

    def matfun(self, S):
        return np.linalg.matrix_power(np.asarray(S, dtype=complex), self.p)

    def values(self, lams):
        return np.asarray(lams, dtype=np.complex128) ** self.p


class Exp(ScalarFun):
    """exp(c*lam)   (DEP: c = -tau, src/NEPTypes.jl:505-509)"""

    def __init__(self, c):
        self.c = c

    def real_on_reals(self):
        return not np.iscomplexobj(self.c)

    def derivs(self, lam, k, scale=1.0):
        return np.exp(self.c * complex(lam)) * np.power(complex(self.c * scale), np.arange(k))

    def taylor(self, lam, k, scale=1.0):
        # tau_{j+1} = tau_j * (c scale) / (j+1)
        out = np.empty(k, dtype=np.complex128)
        d = complex(np.exp(self.c * complex(lam)))
        cs = complex(self.c * scale)
        for j in range(k):
            out[j] = d
            d = d * (cs / (j + 1))
        return out

    def matfun(self, S):
        return sla.expm(self.c * np.asarray(S, dtype=complex))

    def values(self, lams):
        return np.exp(self.c * np.asarray(lams, dtype=np.complex128))


class ISqrt(ScalarFun):
    """1im*sqrt(alpha*lam + beta), principal branch   (gun: src/gallery_extra/NLEVP_native.jl:13-14)"""

    def __init__(self, alpha=1.0, beta=0.0):
        self.alpha, self.beta = alpha, beta

    def derivs(self, lam, k, scale=1.0):
        u = complex(self.alpha * complex(lam) + self.beta)
        out = np.zeros(k, dtype=np.complex128)
        d = 1j * np.sqrt(u)
        out[0] = d
        r = scale * self.alpha / u
        for j in range(k - 1):
            # scale^(j+1) f^(j+1) = scale^j f^(j) * scale*alpha*(1/2 - j)/u
            d = d * (r * (0.5 - j))
            out[j + 1] = d
        return out

    def taylor(self, lam, k, scale=1.0):
        # binomial series: tau_{j+1} = tau_j * scale*alpha/u * (1/2 - j)/(j + 1)
        u = complex(self.alpha * complex(lam) + self.beta)
        out = np.empty(k, dtype=np.complex128)
        d = complex(1j * np.sqrt(u))
        r = complex(scale * self.alpha / u)
        for j in range(k):
            out[j] = d
            d = d * (r * ((0.5 - j) / (j + 1)))
        return out

    def matfun(self, S):
        S = np.asarray(S, dtype=complex)
        return 1j * sla.sqrtm(self.alpha * S + self.beta * np.eye(S.shape[0]))

    def values(self, lams):
        return 1j * np.sqrt(self.alpha * np.asarray(lams, dtype=np.complex128) + self.beta)


class Scaled(ScalarFun):
    def __init__(self, c, f):
        self.c, self.f = c, f

    def real_on_reals(self):
        return not np.iscomplexobj(self.c) and self.f.real_on_reals()

    def derivs(self, lam, k, scale=1.0):
        return self.c * self.f.derivs(lam, k, scale)

    def taylor(self, lam, k, scale=1.0):
        return self.c * self.f.taylor(lam, k, scale)

    def matfun(self, S):
        return self.c * self.f.matfun(S)

    def values(self, lams):
        return self.c * self.f.values(lams)


class Affine(ScalarFun):
    """lam -> f(scale*lam + shift)"""

    def __init__(self, f, scale, shift):
        self.f, self.scale, self.shift = f, scale, shift

    def derivs(self, lam, k, scale=1.0):
        # chain rule: d^j/dlam^j f(scale*lam+shift) = scale^j f^(j)(.)
        return self.f.derivs(self.scale * complex(lam) + self.shift, k, scale * self.scale)

    def taylor(self, lam, k, scale=1.0):
        return self.f.taylor(self.scale * complex(lam) + self.shift, k, scale * self.scale)

    def matfun(self, S):
        S = np.asarray(S, dtype=complex)
        return self.f.matfun(self.scale * S + self.shift * np.eye(S.shape[0]))

    def values(self, lams):
        return self.f.values(self.scale * np.asarray(lams, dtype=np.complex128) + self.shift)


class Resolvent(ScalarFun):
    """g(lam) = f(lam) / (lam - mu): the functions of the rank-one terms of a deflated SPMF (the reference's closure
    `S -> (S - mu*one(S)) \\ f(S)`, src/nep_deflation.jl:259).  Differentiating (lam - mu) g = f j times gives
    (lam - mu) g^(j) + j g^(j-1) = f^(j), so with G_j = scale^j g^(j) and F_j = scale^j f^(j)

        G_j = (F_j - j scale G_{j-1}) / (lam - mu),        T_j = G_j / j! = (F_j / j! - scale T_{j-1}) / (lam - mu):

    Leibniz' rule as a two-term recurrence in which neither j!, scale^j nor a power of (lam - mu) appears on its own."""

    def __init__(self, f, mu):
        self.f, self.mu = f, mu

    def real_on_reals(self):
        return self.f.real_on_reals() and complex(self.mu).imag == 0

    def derivs(self, lam, k, scale=1.0):
        F = self.f.derivs(lam, k, scale)
        w = complex(lam) - self.mu
        out = np.empty(k, dtype=np.complex128)
        g = 0j
        for j in range(k):
            g = (F[j] - (j * scale) * g) / w
            out[j] = g
        return out

    def taylor(self, lam, k, scale=1.0):
        F = self.f.taylor(lam, k, scale)
        w = complex(lam) - self.mu
        out = np.empty(k, dtype=np.complex128)
        g = 0j
        for j in range(k):
            g = (F[j] - scale * g) / w
            out[j] = g
        return out

    def matfun(self, S):
        S = np.asarray(S, dtype=complex)
        return np.linalg.solve(S - self.mu * np.eye(S.shape[0]), self.f.matfun(S))

    def values(self, lams):
        lams = np.asarray(lams, dtype=np.complex128)
        return self.f.values(lams) / (lams - self.mu)


class Sum(ScalarFun):
    def __init__(self, *fs):
        self.fs = fs

    def real_on_reals(self):
        return all(f.real_on_reals() for f in self.fs)

    def derivs(self, lam, k, scale=1.0):
        return sum(f.derivs(lam, k, scale) for f in self.fs)

    def taylor(self, lam, k, scale=1.0):
        return sum(f.taylor(lam, k, scale) for f in self.fs)

    def matfun(self, S):
        return sum(f.matfun(S) for f in self.fs)

    def values(self, lams):
        return sum(f.values(lams) for f in self.fs)


class WEPSqrt(ScalarFun):
    """Waveguide corner functions  f(lam) = 1im*sqrt(lam^2 + b*lam + c)*sign-rule + d0
    with the branch Im sqrt >= 0 (src/gallery_extra/waveguide/Waveguide.jl:143-157) and derivatives
    by the three-term recurrence of sqrt_derivative (:580-616), restated here from the ODE
    g^2 = q(lam): with g = sqrt(q), g*g' = q'/2 and Leibniz' rule gives all higher derivatives."""

    def __init__(self, b, c, d0=0.0):
        self.b, self.c, self.d0 = complex(b), complex(c), complex(d0)

    def _sqrt(self, lam):
        a = lam * lam + self.b * lam + self.c
        s = np.sqrt(complex(a))
        # branch rule: multiply by sign(imag(a)) unless imag(a) == 0
        if a.imag != 0:
            s = s * np.sign(a.imag)
        return s

    def derivs(self, lam, k, scale=1.0):
        lam = complex(lam)
        # Taylor coefficients t_j = scale^j g^(j)/j! of g = sqrt(q) around lam, q = q0 + q1 h + q2 h^2
        q1 = (2 * lam + self.b) * scale
        q2 = 1.0 * scale * scale
        t = np.zeros(max(k, 1), dtype=np.complex128)
        t[0] = self._sqrt(lam)
        # g^2 = q  ->  sum_{i=0..m} t_i t_{m-i} = q_m
        for m in range(1, k):
            qm = q1 if m == 1 else (q2 if m == 2 else 0.0)
            s = 0.0 + 0j
            for i in range(1, m):
                s += t[i] * t[m - i]
            t[m] = (qm - s) / (2 * t[0])
        out = np.empty(k, dtype=np.complex128)
        fact = 1.0
        for j in range(k):
            if j > 0:
                fact *= j
            out[j] = 1j * t[j] * fact
        out[0] += self.d0
        return out

    def taylor(self, lam, k, scale=1.0):
        # g = sqrt(q) satisfies 2 q g' = q' g; with q = q0 + q1 h + q2 h^2 the coefficients of h^m give the three-term
        # recurrence (m+1) q0 t_{m+1} = (1/2 - m) q1 t_m + (2 - m) q2 t_{m-1}.  Its other solution decays like the
        # reciprocal of the farther root of q, so the forward recurrence is stable.
        lam = complex(lam)
        q0 = lam * lam + self.b * lam + self.c
        a1 = (2 * lam + self.b) * scale / q0
        a2 = scale * scale / q0
        t = np.zeros(k, dtype=np.complex128)
        if k == 0:
            return t
        t[0] = self._sqrt(lam)
        tm1, tm = 0j, complex(t[0])
        for m in range(k - 1):
            nxt = ((0.5 - m) / (m + 1)) * a1 * tm + ((2.0 - m) / (m + 1)) * a2 * tm1
            t[m + 1] = nxt
            tm1, tm = tm, nxt
        out = 1j * t
        out[0] += self.d0
        return out

    def matfun(self, S):
        raise NotImplementedError("WEPSqrt.matfun (compute_MM with non-diagonal S) is not supported")


class Chebyshev(ScalarFun):
    """T_j(x), x = 2 (lam - a) / (b - a) - 1: the Chebyshev polynomial of the first kind scaled to [a, b], the basis of ChebPEP
    (src/types_cheb_pep.jl:24-58).  Everything goes through T_{i+1} = 2 x T_i - T_{i-1}, which holds for complex lam, for lam
    outside [a, b] and for matrices alike; the reference's cos(j acos x) needs a work-around to stay real on real matrices
    (types_cheb_pep.jl:11-23) and leaves the reals for |x| > 1.  Applied to the polynomials h -> T_i(x + c h), c = 2 scale / (b - a),
    as coefficient vectors in h, the same recurrence gives the Taylor coefficients in closed form (no Jordan block): the entries of
    order > j are exact zeros."""

    def __init__(self, j, a=-1.0, b=1.0):
        if np.iscomplexobj(a) or np.iscomplexobj(b) or not float(a) < float(b):
            raise ValueError("Chebyshev: the interval [a, b] needs real a < b")
        if int(j) != j or j < 0:
            raise ValueError("Chebyshev: the degree must be a non-negative integer")
        self.j, self.a, self.b = int(j), float(a), float(b)

    def real_on_reals(self):
        return True

    def _x(self, lam):
        return 2.0 * (lam - self.a) / (self.b - self.a) - 1.0

    def values(self, lams):
        x = self._x(np.asarray(lams, dtype=np.complex128))
        t0, t1 = np.ones_like(x), x
        if self.j == 0:
            return t0
        for _ in range(self.j - 1):
            t0, t1 = t1, 2.0 * x * t1 - t0
        return t1

    def __call__(self, lam):
        return complex(self.values(np.array([lam]))[0])

    def taylor(self, lam, k, scale=1.0):
        x = complex(self._x(complex(lam)))
        c = 2.0 * scale / (self.b - self.a)                  # chain factor of h -> x + c h
        m = self.j + 1
        p0 = np.zeros(m, dtype=np.complex128); p0[0] = 1.0   # T_0
        p1 = np.zeros(m, dtype=np.complex128); p1[0] = x     # T_1 = x + c h
        if m > 1:
            p1[1] = c
        cur = p0 if self.j == 0 else p1
        for _ in range(self.j - 1):
            nxt = 2.0 * x * p1 - p0
            nxt[1:] += 2.0 * c * p1[:-1]
            p0, p1 = p1, nxt
            cur = p1
        out = np.zeros(k, dtype=np.complex128)
        out[:min(k, m)] = cur[:k]
        return out

    def derivs(self, lam, k, scale=1.0):
        out = self.taylor(lam, k, scale)
        f = 1.0
        for i in range(2, min(k, self.j + 1)):               # i! <= j!: no overflow below degree 170
            f *= i
            out[i] *= f
        return out

    def matfun(self, S):
        S = np.asarray(S)
        S = S.astype(np.complex128 if np.iscomplexobj(S) else np.float64)
        I = np.eye(S.shape[0], dtype=S.dtype)
        X = (2.0 / (self.b - self.a)) * (S - self.a * I) - I
        T0, T1 = I, X
        if self.j == 0:
            return T0
        for _ in range(self.j - 1):
            T0, T1 = T1, 2.0 * (X @ T1) - T0
        return T1


class FromMatrixFunction(ScalarFun):
    """Generic fallback for user functions given the reference way: a callable valid for scalars
    and square matrices.  Derivatives via the Jordan-matrix trick of src/NEPTypes.jl:376-388
    (host, O(k^3)); use only for functions without a closed form."""

    def __init__(self, f):
        self.fun = f

    def derivs(self, lam, k, scale=1.0):
        if k == 1:
            return np.array([self.fun(complex(lam))], dtype=np.complex128)
        S = np.zeros((k, k), dtype=complex)
        S[np.arange(k), np.arange(k)] = lam
        S[np.arange(1, k), np.arange(k - 1)] = scale * np.arange(1, k)
        return np.asarray(self.fun(S), dtype=np.complex128)[:, 0].copy()

    def matfun(self, S):
        return np.asarray(self.fun(np.asarray(S, dtype=complex)))


class ExpSqrt(FromMatrixFunction):
    """lam -> exp(gamma * sqrt(alpha * lam + beta)): the wave-number functions of the "particle in a canyon" example,
    test/nleigs/particle_test_utils.jl:148-155 -- exp(i sqrt(m (lam - c))) for branch points c below the interval of
    interest (gamma = i, alpha = m, beta = -m c) and exp(-sqrt(m (c - lam))) from there on (gamma = -1, alpha = -m,
    beta = m c).  Value and matrix function in closed form (principal square root), higher derivatives through the
    Jordan-block evaluation of the base class."""

    def __init__(self, gamma, alpha, beta):
        self.gamma, self.alpha, self.beta = complex(gamma), float(alpha), float(beta)
        super().__init__(self._eval)

    def _eval(self, S):
        if isinstance(S, np.ndarray) and S.ndim == 2:
            return sla.expm(self.gamma * sla.sqrtm(self.alpha * S.astype(complex) + self.beta * np.eye(S.shape[0])))
        return np.exp(self.gamma * np.sqrt(self.alpha * complex(S) + self.beta))

    def values(self, lams):
        return np.exp(self.gamma * np.sqrt(self.alpha * np.asarray(lams, dtype=np.complex128) + self.beta))


def one():
    return Monomial(0)


def ident():
    return Monomial(1)
