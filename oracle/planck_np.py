"""Vectorised numpy restatement of rt_oracle.c planck_cell / planck_cell_dBdT with a dtype
argument -- TEST INFRASTRUCTURE ONLY (like fused_np.py).

The same algorithm: per cell the three branches of Planck::integrate_B / integrate_dBdT (12-point
Gauss-Legendre for z2 <= 0.7, the Bose series for z1 >= 0.5, Gauss to z = 0.6 plus the series
beyond it otherwise), the series length by the oracle's rule, the last group the grey remainder
a c T^4 - (ONE integral over [e_0, e_{G-1}]) kept only where positive, and 0 for T <= 0, T not
finite and equal edges.  The branch and the series length are decided in fp64 from the fp64
inputs, exactly as the oracle decides them; the arithmetic runs in `dtype`.

dtype np.longdouble is the truth of the material regime sweep (tests/material_regime_cases.py):
"this algorithm on these fp64 inputs".  There exp(x) - 1 is np.expm1 and e^{-n z} one np.exp per
term -- the same values in exact arithmetic, without the cancellation at small x.  The physical
constants are fp64 inputs (h, c, k_B, pi as the reference rounds them, a c from fp64 pow as
rad_a_long forms it); the Gauss nodes are the oracle's long double Newton iteration restated.

`planck_device_form` is an fp64 emulation of planck_cells_kernel's evaluation order (one exp and
a running product per series, ascending sums, 1 / T once, a reciprocal table, the stop rule
without divisions): what the metric's K must leave room for.
"""
from __future__ import annotations

import math

import numpy as np

C_PLANCK = 4.141895e-10
C_BOLTZ_JPK = 1.601558e-25
C_LIGHT = 299.79245800
C_PI = 3.1415926546
DBL_EPS = float(np.finfo(np.float64).eps)
DBL_MIN = float(np.finfo(np.float64).tiny)
RAD_A = (8.0 * math.pow(C_PI, 5) * 1.0) / (15.0 * math.pow(C_PLANCK, 3) * math.pow(C_LIGHT, 3))
A_C = RAD_A * C_LIGHT  # fp64, as planck_cell forms rad_a_long() * C_LIGHT

ZERO, GAUSS, SERIES, SPLIT = 0, 1, 2, 3  # the branch of one (cell, integral)


def _gauss_nodes():
    """planck_setup: 12 Gauss-Legendre nodes and weights, Newton from a double cos in long double."""
    L = np.longdouble
    order, pts, wts = 12, [L(0)] * 12, [L(0)] * 12
    weight_sum = L(0)
    for i in range(6):
        mu = L(math.cos(C_PI * (i + 0.75) / (order + 0.5)))
        while True:
            p_jm1, p_j = L(0), L(1)
            for j in range(1, order + 1):
                p_jm2, p_jm1 = p_jm1, p_j
                p_j = ((2 * j - 1) * mu * p_jm1 - (j - 1) * p_jm2) / j
            p_deriv = (order + 1) * (mu * p_j - p_jm1) / (mu * mu - 1)  # j == order + 1, as written
            old = mu
            mu = old - p_j / p_deriv
            if abs(mu - old) < DBL_EPS:
                break
        pts[i], pts[order - 1 - i] = -mu, mu
        wts[i] = wts[order - 1 - i] = 1 / ((1 - mu * mu) * p_deriv * p_deriv)
        weight_sum += wts[i] + wts[order - 1 - i]
    wts = [w * (2 / weight_sum) for w in wts]
    return np.array(pts, dtype=np.longdouble), np.array(wts, dtype=np.longdouble)


NODES, WEIGHTS = _gauss_nodes()


def _p_equal(l, r):
    d = np.abs(l - r)
    return (d <= DBL_EPS * np.abs(l + r) * 2) | (d < DBL_MIN)


def _density(T, E, f, deriv):
    """planck_get_B / planck_get_dBdT (k_B = 1) at (T, E), arrays of dtype f."""
    h, c = f(C_PLANCK), f(C_LIGHT)
    x = E / T
    ext = f is np.longdouble
    em1 = np.expm1(x) if ext else np.exp(x) - f(1)
    if not deriv:
        return f(2) * np.power(E, f(3)) * np.power(h, f(-3)) * np.power(c, f(-2)) / em1
    return (f(2) * np.power(h, f(-3)) * np.power(c, f(-2)) * f(1) * np.power(E, f(4)) * np.power(T, f(-2))
            * np.exp(x) * np.power(em1, f(-2)))


def _gauss_sum(T, mid, hw, f, deriv):
    acc = np.zeros_like(T)
    pts, wts = NODES.astype(f), WEIGHTS.astype(f)
    for i in range(12):
        E = mid + hw * pts[i]
        acc = acc + hw * wts[i] * _density(T, E, f, deriv)
    return acc


def _poly(x, f, deriv):
    if not deriv:
        return np.power(x, f(3)) + f(3) * np.power(x, f(2)) + f(6) * x + f(6)
    return np.power(x, f(4)) + f(4) * np.power(x, f(3)) + f(12) * np.power(x, f(2)) + f(24) * x + f(24)


def series_length(z1, deriv):
    """The oracle's rule, in fp64 on the fp64 z1 (an array): the first N >= 32 whose next term is
    at most the accuracy relative to the leading one."""
    z1 = np.asarray(z1, dtype=np.float64)
    F = np.float64
    with np.errstate(all="ignore"):
        lead = np.exp(-z1) * (_poly(z1, F, deriv) if deriv else (z1 * z1 * z1 + 3.0 * z1 * z1 + 6.0 * z1 + 6.0))
        lead = np.maximum(lead, DBL_EPS)
        N = np.full(z1.shape, 32, dtype=np.int64)
        live = np.ones(z1.shape, dtype=bool)
        while live.any():
            n1 = N + 1.0
            val = (np.exp(-n1 * z1) / (1.0 - np.exp(-z1)) * np.power(n1, -4.0) * _poly(n1 * z1, F, deriv) / lead)
            live &= val > DBL_EPS
            N[live] += 1
    return N


def _series(z1, z2, N, f, deriv):
    """sum1 - sum2 of series_B / series_dBdT, n descending from each cell's N."""
    s1, s2 = np.zeros_like(z1), np.zeros_like(z1)
    with np.errstate(under="ignore"):
        for n in range(int(N.max()) if N.size else 0, 0, -1):
            on = N >= n
            nf = f(n)
            t1 = np.exp(-nf * z1) / np.power(nf, f(4)) * _poly(nf * z1, f, deriv)
            t2 = np.exp(-nf * z2) / np.power(nf, f(4)) * _poly(nf * z2, f, deriv)
            s1 = np.where(on, s1 + t1, s1)
            s2 = np.where(on, s2 + t2, s2)
    return s1 - s2, s1


def integrate(T, e_min, e_max, dtype=np.float64, deriv=False, n_adjust=0, info=None):
    """Planck::integrate_B (deriv: integrate_dBdT) x 4 pi for the cells T (an array; where it is
    held in a wider format than fp64 its fp64 rounding decides the branch, itself enters the
    arithmetic) over
    [e_min, e_max]; returns (values in dtype, branch per cell).  n_adjust: added to the series
    length (a defect for the metric's own test; 0 is the algorithm).  info receives 'scale': per
    cell the size of the operands whose rounding bounds the result's -- the larger series sum of
    the final subtraction (times its prefactor), and for a Gauss sum its value over min(z2, 1)
    (exp(x) - 1 loses 1 / x of its relative precision at the nodes)."""
    f = np.dtype(dtype).type
    Tf = np.atleast_1d(np.asarray(T)).astype(f)
    T64 = Tf.astype(np.float64)
    e_min, e_max = float(e_min), float(e_max)
    out = np.zeros(T64.shape, dtype=f)
    branch = np.zeros(T64.shape, dtype=np.int64)
    scale = np.zeros(T64.shape)
    if info is not None:
        info["scale"] = scale
    live = (T64 > 0.0) & np.isfinite(T64) & ~_p_equal(T64, 0.0)
    if _p_equal(np.float64(e_min), np.float64(e_max)) or not live.any():
        return out, branch
    with np.errstate(all="ignore"):
        z1_64 = np.where(live, e_min / T64, 0.0)
        z2_64 = np.where(live, e_max / T64, 0.0)
    branch[live] = np.where(z2_64 <= 0.7, GAUSS, np.where(z1_64 >= 0.5, SERIES, SPLIT))[live]
    h, c, emin, emax = f(C_PLANCK), f(C_LIGHT), f(e_min), f(e_max)
    for br in (GAUSS, SERIES, SPLIT):
        m = branch == br
        if not m.any():
            continue
        Tb = Tf[m]
        if br == GAUSS:
            v = _gauss_sum(Tb, f(0.5) * (emax + emin), f(0.5) * (emax - emin), f, deriv)
            sc = np.abs(v) / np.minimum(z2_64[m], 1.0).astype(f)
        else:
            z1 = emin / (f(1) * Tb) if br == SERIES else np.full(Tb.shape, f(0.6))
            z2 = emax / (f(1) * Tb)
            z1_rule = z1_64[m] if br == SERIES else np.full(Tb.shape, 0.6)
            N = series_length(z1_rule, deriv) + n_adjust
            s, s1 = _series(z1, z2, N, f, deriv)
            if deriv:
                pref = f(2) * np.power(f(1), f(4)) * np.power(Tb, f(3)) / (np.power(h, f(3)) * np.power(c, f(2)))
                v = f(2) * np.power(f(1), f(4)) * np.power(Tb, f(3)) * s / (np.power(h, f(3)) * np.power(c, f(2)))
            else:
                pref = f(2) * np.power(f(1) * Tb, f(4)) / (np.power(h, f(3)) * np.power(c, f(2)))
                v = f(2) * np.power(f(1) * Tb, f(4)) * s / (np.power(h, f(3)) * np.power(c, f(2)))
            sc = pref * s1
            if br == SPLIT:
                e6 = f(0.6) * f(1) * Tb
                gs = _gauss_sum(Tb, f(0.5) * (e6 + emin), f(0.5) * (e6 - emin), f, deriv)
                v = gs + v
                sc = sc + gs
        out[m] = v * f(4) * f(C_PI)
        scale[m] = np.asarray(sc * f(4) * f(C_PI), dtype=np.float64)
    return out, branch


def planck_cell(T, e_edge, g, dtype=np.float64, deriv=False, n_adjust=0, clamp=True, info=None):
    """kcon B_g(T) (deriv: kcon dB_g/dT) of group g for the cells T, in dtype.  clamp=False leaves
    the remainder's sign alone (a defect for the metric's own test).  info: a dict that receives
    'branch' (per cell) and, for the remainder group, 'clamped' (cells where the clamp acted)."""
    f = np.dtype(dtype).type
    e = np.asarray(e_edge, dtype=np.float64)
    G = e.size - 1
    Tf = np.atleast_1d(np.asarray(T)).astype(f)
    T64 = Tf.astype(np.float64)
    if g < G - 1:
        sc = {}
        v, br = integrate(Tf, e[g], e[g + 1], f, deriv, n_adjust, sc)
        if info is not None:
            info.update(branch=br, clamped=np.zeros(T64.shape, dtype=bool), scale=C_BOLTZ_JPK * sc["scale"])
        return f(C_BOLTZ_JPK) * v
    v, br = integrate(Tf, e[0], e[G - 1], f, deriv, n_adjust)
    live = (T64 > 0.0) & np.isfinite(T64)
    Tl = np.where(live, Tf, f(0))
    grey = f(4) * f(RAD_A) * f(C_LIGHT) * np.power(Tl, f(3)) if deriv else f(RAD_A) * f(C_LIGHT) * np.power(Tl, f(4))
    rest = grey - v
    cl = live & ~(rest > 0)
    if info is not None:
        info.update(branch=br, clamped=cl, scale=np.asarray(f(C_BOLTZ_JPK) * grey, dtype=np.float64))
    if clamp:
        rest = np.where(rest > 0, rest, f(0))
    return np.where(live, f(C_BOLTZ_JPK) * rest, f(0))


def planck_cell_dBdT(T, e_edge, g, dtype=np.float64, **kw):
    return planck_cell(T, e_edge, g, dtype, deriv=True, **kw)


def planck_cells(T, e_edge, g_lo, g_hi, dtype=np.float64, deriv=False):
    """(N, g_hi - g_lo) in dtype."""
    return np.stack([planck_cell(T, e_edge, g, dtype, deriv) for g in range(g_lo, g_hi)], axis=1)


# ---------------------------------------------------------------------------
# fp64 emulation of the device's evaluation order (kernels.hip planck_series_pair,
# planck_gauss_pair, planck_integral_pair, cell_group_planck) -- scalar, Python floats
# ---------------------------------------------------------------------------
_PRE = 2.0 / ((C_PLANCK * C_PLANCK * C_PLANCK) * (C_LIGHT * C_LIGHT))
_NODE64 = [float(x) for x in NODES]
_WEIGHT64 = [float(x) for x in WEIGHTS]


def _exp(x):
    try:
        return math.exp(x)
    except OverflowError:
        return math.inf


def _dev_series(z1, z2):
    e1, f1 = _exp(-z1), _exp(-z2)
    a1, b1, c1 = z1 * z1 * z1, 3.0 * (z1 * z1), 6.0 * z1
    a2, b2, c2 = z2 * z2 * z2, 3.0 * (z2 * z2), 6.0 * z2
    qa1, qb1, qc1, qd1 = (z1 * z1) * (z1 * z1), 4.0 * (z1 * z1 * z1), 12.0 * (z1 * z1), 24.0 * z1
    qa2, qb2, qc2, qd2 = (z2 * z2) * (z2 * z2), 4.0 * (z2 * z2 * z2), 12.0 * (z2 * z2), 24.0 * z2
    pr = lambda r, a, b, c: r * (a + r * (b + r * (c + 6.0 * r)))  # noqa: E731
    pq = lambda r, a, b, c, d: a + r * (b + r * (c + r * (d + 24.0 * r)))  # noqa: E731
    lead = max(e1 * (a1 + b1 + c1 + 6.0), DBL_EPS)
    qlead = max(e1 * (qa1 + qb1 + qc1 + qd1 + 24.0), DBL_EPS)
    stop, qstop = DBL_EPS * (1.0 - e1) * lead, DBL_EPS * (1.0 - e1) * qlead
    n, em = 32, _exp(-33.0 * z1)
    while n < 4096 and em * pr(1.0 / (n + 1), a1, b1, c1) > stop:
        n, em = n + 1, em * e1
    qn, em = 32, _exp(-33.0 * z1)
    while qn < 4096 and em * pq(1.0 / (qn + 1), qa1, qb1, qc1, qd1) > qstop:
        qn, em = qn + 1, em * e1
    s1 = s2 = t1 = t2 = 0.0
    p1 = p2 = 1.0
    for k in range(1, max(n, qn) + 1):
        p1 *= e1
        p2 *= f1
        if p1 == 0.0:
            break
        r = 1.0 / k
        if k <= n:
            s1 += p1 * pr(r, a1, b1, c1)
            s2 += p2 * pr(r, a2, b2, c2)
        if k <= qn:
            t1 += p1 * pq(r, qa1, qb1, qc1, qd1)
            t2 += p2 * pq(r, qa2, qb2, qc2, qd2)
    return s1 - s2, t1 - t2


def _dev_gauss(inv_T, mid, hw):
    acc = dacc = 0.0
    for r in range(12):
        E = mid + hw * _NODE64[r]
        ex = _exp(E * inv_T)
        em1 = ex - 1.0
        acc += hw * _WEIGHT64[r] * (_PRE * (E * E * E) / em1)
        dacc += hw * _WEIGHT64[r] * (_PRE * ((E * E) * (E * E)) * (inv_T * inv_T) * ex / (em1 * em1))
    return acc, dacc


def _dev_integral(T, e_min, e_max):
    if _p_equal(np.float64(e_min), np.float64(e_max)):
        return 0.0, 0.0
    inv_T = 1.0 / T
    z1, z2 = e_min * inv_T, e_max * inv_T
    t3, t4 = (T * T) * T, (T * T) * (T * T)
    if z2 <= 0.7:
        b, db = _dev_gauss(inv_T, 0.5 * (e_max + e_min), 0.5 * (e_max - e_min))
    elif z1 >= 0.5:
        sb, sdb = _dev_series(z1, z2)
        b, db = _PRE * t4 * sb, _PRE * t3 * sdb
    else:
        e6 = 0.6 * T
        gb, gdb = _dev_gauss(inv_T, 0.5 * (e6 + e_min), 0.5 * (e6 - e_min))
        sb, sdb = _dev_series(0.6, z2)
        b, db = gb + _PRE * t4 * sb, gdb + _PRE * t3 * sdb
    return b * 4.0 * C_PI, db * 4.0 * C_PI


def planck_device_form(T, e_edge, g):
    """(B, dB/dT) arrays over the cells T of group g, fp64, in the device's evaluation order."""
    e = [float(x) for x in np.asarray(e_edge, dtype=np.float64)]
    G = len(e) - 1
    T64 = np.atleast_1d(np.asarray(T, dtype=np.float64))
    B, dB = np.zeros(T64.shape), np.zeros(T64.shape)
    for i, t in enumerate(T64.tolist()):
        if not (t > 0.0 and math.isfinite(t) and not _p_equal(np.float64(t), np.float64(0.0))):
            continue
        if g < G - 1:
            b, db = _dev_integral(t, e[g], e[g + 1])
            B[i], dB[i] = C_BOLTZ_JPK * b, C_BOLTZ_JPK * db
        else:
            b, db = _dev_integral(t, e[0], e[G - 1])
            rest, drest = A_C * ((t * t) * (t * t)) - b, 4.0 * A_C * ((t * t) * t) - db
            B[i] = C_BOLTZ_JPK * rest if rest > 0.0 else 0.0
            dB[i] = C_BOLTZ_JPK * drest if drest > 0.0 else 0.0
    return B, dB
