"""Taylor coefficients tau_j = scale^j f^(j)(lam) / j! of the package's scalar functions in mpmath (50 digits), from closed-form
series (polynomial, exponential, binomial series of the square root) and, for WEPSqrt, the power-series recurrence of
g^2 = q.  Shared by the taylor tests and the K11 tests.  mpmath.taylor is not used: its numerical differentiation is not
accurate at high order."""
import mpmath as mp

from nep_amd import funcs

mp.mp.dps = 50


def mp_taylor(f, lam, k, scale=1):
    """(values, magnitudes): mpc coefficients and the scale each is held to -- |value|, or for a Sum the sum of the
    parts' magnitudes"""
    lam = mp.mpc(lam)
    scale = mp.mpc(scale)
    if isinstance(f, funcs.Monomial):
        v = [mp.binomial(f.p, j) * lam ** (f.p - j) * scale ** j if j <= f.p else mp.mpc(0) for j in range(k)]
    elif isinstance(f, funcs.Exp):
        c = mp.mpc(f.c)
        e = mp.exp(c * lam)
        v = [e * (c * scale) ** j / mp.factorial(j) for j in range(k)]
    elif isinstance(f, funcs.ISqrt):
        u = mp.mpc(f.alpha) * lam + mp.mpc(f.beta)
        s = mp.sqrt(u)
        r = mp.mpc(f.alpha) * scale / u
        v = [1j * s * mp.binomial(mp.mpf(1) / 2, j) * r ** j for j in range(k)]
    elif isinstance(f, funcs.Scaled):
        v, a = mp_taylor(f.f, lam, k, scale)
        c = mp.mpc(f.c)
        return [c * x for x in v], [abs(c) * x for x in a]
    elif isinstance(f, funcs.Affine):
        return mp_taylor(f.f, mp.mpc(f.scale) * lam + mp.mpc(f.shift), k, scale * mp.mpc(f.scale))
    elif isinstance(f, funcs.Sum):
        parts = [mp_taylor(g, lam, k, scale) for g in f.fs]
        return ([sum(p[0][j] for p in parts) for j in range(k)], [sum(p[1][j] for p in parts) for j in range(k)])
    elif isinstance(f, funcs.WEPSqrt):
        b, c, d0 = mp.mpc(f.b), mp.mpc(f.c), mp.mpc(f.d0)
        a = lam * lam + b * lam + c
        t0 = mp.sqrt(a)
        if mp.im(a) != 0:
            t0 = t0 * mp.sign(mp.im(a))
        q = [None, (2 * lam + b) * scale, scale * scale]
        t = [t0]
        for m in range(1, k):
            s = sum((t[i] * t[m - i] for i in range(1, m)), mp.mpc(0))
            qm = q[m] if m <= 2 else 0
            t.append((qm - s) / (2 * t0))
        v = [1j * x for x in t]
        v[0] = v[0] + d0
    else:
        raise TypeError(type(f).__name__)
    return v, [abs(x) for x in v]
