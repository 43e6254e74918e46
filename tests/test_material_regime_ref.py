"""Regime sweep of the material coupling, CPU side: the extended-precision truth
(oracle/planck_np.py, RegionMaterialReference in np.longdouble) against the C oracle and a
40-digit evaluation, the conditions that keep a case of tests/material_regime_cases.py from
passing vacuously -- asserted on the truth alone, at every grid point -- and the metric's own
tests: the margin an fp64 emulation of the device's evaluation order leaves under K, and the
defects the bound sees where the fixed tolerances of tests/test_material_gpu.py do not.
"""
import numpy as np
import pytest

import material_regime_cases as mc
import planck_np
from regime_cases import EPS, HAVE_EXTENDED, K, ORACLE_ERR_MAX, SKIP_REASON, check_conditions

needs_extended = pytest.mark.skipif(not HAVE_EXTENDED, reason=SKIP_REASON)

NP_VS_C_ULPS = 4.0  # measured: 2.0 (log grid, dB/dT of group 9 at T = 0.0274)


# ---------------------------------------------------------------------------
# planck_np against the C oracle and against 40 digits
# ---------------------------------------------------------------------------
def test_planck_np_fp64_matches_c_oracle(oracle_mod):
    """planck_np in float64 against orc_planck_cell / orc_planck_cell_dBdT over the whole Planck
    sweep, in ulps of the operand scale planck_np reports (the larger series sum, a Gauss sum over
    min(z2, 1), the grey total for the remainder): the two differ by the oracle's long double
    Gauss nodes and accumulation and by nothing else."""
    worst = (0.0, None)
    for name in mc.PLANCK_GRIDS:
        for deriv in (False, True):
            t = mc.planck_truth(oracle_mod, name, deriv)
            for g in range(t.edges.size - 1):
                info = {}
                planck_np.planck_cell(t.T, t.edges, g, deriv=deriv, info=info)
                d = np.abs(t.npform[:, g] - t.oracle[:, g])
                dead = EPS * info["scale"] == 0  # underflowed with everything else of the cell
                assert (d[dead] == 0).all(), (name, deriv, g)
                u = np.max(d[~dead] / (EPS * info["scale"][~dead]), initial=0.0)
                worst = max(worst, (float(u), (name, deriv, g)))
    print(f"planck_np fp64 against the C oracle: {worst[0]:.2f} ulps of the operand scale at {worst[1]}")
    assert worst[0] <= NP_VS_C_ULPS, worst


def _mpf(mp, x):
    """An np.longdouble exactly: its fp64 rounding plus the rest."""
    m, e = np.frexp(np.longdouble(x))  # the mantissa apart: float() of a value below 1e-308 drops bits
    hi = float(m)
    return mp.ldexp(mp.mpf(hi) + mp.mpf(float(m - np.longdouble(hi))), int(e))


def _mp_planck(mp, T, e, g, deriv):
    """The same algorithm at 40 digits on the fp64 inputs (the branch and the series length by
    planck_np's fp64 rule; the nodes planck_np's)."""
    h, c, kcon, pi = (mp.mpf(x) for x in (planck_np.C_PLANCK, planck_np.C_LIGHT, planck_np.C_BOLTZ_JPK, planck_np.C_PI))
    nodes, wts = [_mpf(mp, x) for x in planck_np.NODES], [_mpf(mp, x) for x in planck_np.WEIGHTS]
    T = mp.mpf(T)
    G = len(e) - 1

    def density(E):
        x = E / T
        if deriv:
            return 2 * h ** -3 * c ** -2 * E ** 4 * T ** -2 * mp.exp(x) * mp.expm1(x) ** -2
        return 2 * E ** 3 * h ** -3 * c ** -2 / mp.expm1(x)

    def gauss(lo, hi):
        mid, hw = (hi + lo) / 2, (hi - lo) / 2
        return sum(hw * w * density(mid + hw * x) for x, w in zip(nodes, wts))

    def series(z1, z2, n_terms):
        def poly(x):
            return x ** 4 + 4 * x ** 3 + 12 * x ** 2 + 24 * x + 24 if deriv else x ** 3 + 3 * x ** 2 + 6 * x + 6
        s = sum(mp.exp(-n * z1) / mp.mpf(n) ** 4 * poly(n * z1) - mp.exp(-n * z2) / mp.mpf(n) ** 4 * poly(n * z2)
                for n in range(n_terms, 0, -1))
        return 2 * T ** (3 if deriv else 4) * s / (h ** 3 * c ** 2)

    def integral(lo, hi):
        br = planck_np.integrate(np.array([float(T)]), lo, hi)[1][0]
        lo, hi = mp.mpf(lo), mp.mpf(hi)
        if br == planck_np.ZERO:
            return mp.mpf(0)
        if br == planck_np.GAUSS:
            v = gauss(lo, hi)
        elif br == planck_np.SERIES:
            v = series(lo / T, hi / T, int(planck_np.series_length(np.array([float(lo) / float(T)]), deriv)[0]))
        else:
            z = mp.mpf(0.6)
            v = gauss(lo, z * T) + series(z, hi / T, int(planck_np.series_length(np.array([0.6]), deriv)[0]))
        return v * 4 * pi

    if g < G - 1:
        return kcon * integral(e[g], e[g + 1])
    grey = mp.mpf(planck_np.RAD_A) * c * (4 * T ** 3 if deriv else T ** 4)
    rest = grey - integral(e[0], e[G - 1])
    return kcon * rest if rest > 0 else mp.mpf(0)


@needs_extended
def test_planck_np_longdouble_matches_40_digits(oracle_mod):
    """The truth against mpmath at 40 digits, to 1e-17 relative (of the operand scale where the
    branch ends in a subtraction): every group of the log, wide, narrow and straddle grids at a
    subset of the temperatures, 1e-8 and the cells where e^{-z} underflows in fp64 among them.
    Beyond z1 = 64 the bound is 1e-17 z1 / 64: the argument of e^{-z} is itself rounded to 64
    bits, which the exponential turns into a relative error of 2^-64 z (1.5e-17 at z = 276, where
    this was measured as 1.2e-17; 6e-16 where the result is 1e-4900) -- the format's, not the
    restatement's."""
    mp = pytest.importorskip("mpmath")
    mp.mp.dps = 40
    worst = 0.0
    for name in ("log", "wide", "narrow", "straddle"):
        for deriv in (False, True):
            t = mc.planck_truth(oracle_mod, name, deriv)
            G = t.edges.size - 1
            under = np.flatnonzero(((t.oracle == 0) & (t.truth > 0)).any(axis=1))
            cells = sorted(set(range(0, mc.PLANCK_N, 9)) | {48, 66} | set(under[:3].tolist()) | set(under[-2:].tolist()))
            for g in range(G):
                info = {}
                planck_np.planck_cell(t.T, t.edges, g, deriv=deriv, info=info)
                for x in cells:
                    want = _mp_planck(mp.mp, t.T[x], t.edges, g, deriv) if t.T[x] > 0 else mp.mpf(0)
                    got = _mpf(mp.mp, t.truth[x, g])
                    scale = abs(want)  # a Gauss sum: relative; else of the operands of the final subtraction
                    if g == G - 1 or info["branch"][x] != planck_np.GAUSS:
                        scale = max(scale, mp.mpf(float(info["scale"][x])))
                    if want == 0:
                        assert got == 0, (name, deriv, g, x)
                        continue
                    if abs(want) < mp.mpf(10) ** -4900:  # below np.longdouble's normal range
                        continue
                    err = float(abs(got - want) / scale)
                    worst = max(worst, err)
                    z1 = (t.edges[0] if g == G - 1 else t.edges[g]) / t.T[x]
                    if info["branch"][x] == planck_np.SPLIT:
                        z1 = 0.6
                    assert err <= 1e-17 * max(1.0, z1 / 64.0), (name, deriv, g, float(t.T[x]), err)
    print(f"planck_np longdouble against 40 digits: {worst:.2e}")


# ---------------------------------------------------------------------------
# conditions on the truth: the Planck sweep
# ---------------------------------------------------------------------------
@needs_extended
def test_planck_conditions(oracle_mod):
    """Every branch and the underflow-to-zero case occur in some (grid, decade); the truth is
    finite and >= 0, exactly 0 at T <= 0.  The remainder's clamp never acts -- see the cases
    module: a c is formed with a pi above pi -- which this pins for both precisions."""
    seen, under = set(), 0
    for name in mc.PLANCK_GRIDS:
        for deriv in (False, True):
            t = mc.planck_truth(oracle_mod, name, deriv)
            assert np.isfinite(t.truth).all() and (t.truth >= 0).all() and np.isfinite(t.oracle).all()
            dead = ~(t.T > 0)
            assert (t.truth[dead] == 0).all() and (t.oracle[dead] == 0).all() and dead.sum() == 2
            assert not t.clamped.any(), name
            for cells in t.bins.values():
                seen |= set(np.unique(t.branch[cells]).tolist())
                under += int(((t.oracle[cells] == 0) & (t.truth[cells] > 0)).any())
    assert {planck_np.GAUSS, planck_np.SERIES, planck_np.SPLIT} <= seen and under > 0
    t = mc.planck_truth(oracle_mod, "straddle", False)
    x = int(np.flatnonzero(t.T == 1.0)[0])
    assert t.branch[x].tolist() == [planck_np.GAUSS] * 3 + [planck_np.SERIES] * 2 + [planck_np.SPLIT]
    assert sorted(t.bins) == [-8, -3, -2, -1, 0, 1, 2, 3]


# ---------------------------------------------------------------------------
# the metric's own tests
# ---------------------------------------------------------------------------
def _planck_ratio(x, t):
    return mc.group_ratio(x, t.oracle, t.truth, t.floor, t.bins)


@needs_extended
def test_emulation_margin(oracle_mod):
    """planck_np.planck_device_form -- the device's evaluation order in fp64 -- against the bound
    on every (grid, group, decade) of the Planck sweep, B and dB/dT: within K / 4."""
    worst = (0.0, None)
    for name in mc.PLANCK_GRIDS:
        tb, td = mc.planck_truth(oracle_mod, name, False), mc.planck_truth(oracle_mod, name, True)
        G = tb.edges.size - 1
        dev = [planck_np.planck_device_form(tb.T, tb.edges, g) for g in range(G)]
        for t, k in ((tb, 0), (td, 1)):
            r = _planck_ratio(np.stack([d[k] for d in dev], axis=1), t)
            worst = max(worst, (float(r.max()), (name, "dB/dT" if k else "B")))
    print(f"fp64 emulation of the device's order: largest ratio {worst[0]:.2f} at {worst[1]}")
    assert worst[0] <= K / 4, worst


def _old_planck_check(x, ref, T, deriv):
    """tests/test_material_gpu.check_planck's limits (dB/dT: the same with 4 a c T^3)."""
    Tp = np.where(T > 0, T, 0.0)
    grey = mc.KCON_AC * (4 * Tp ** 3 if deriv else Tp ** 4)
    d = np.abs(x - ref)
    ok = (d[:, :-1] <= 1e-12 * np.abs(ref[:, :-1]) + 1e-14 * grey[:, None]).all()
    return bool(ok and (d[:, -1] <= 1e-13 * grey + 1e-300).all())


@needs_extended
def test_metric_sees_what_fixed_tolerances_miss(oracle_mod):
    """Four defects applied to the fp64 restatement; what the bound sees, and what the old checks
    (check_planck's limits; compare's T 1e-12, Beff 1e-10 with planck_rel's floors) let through,
    is printed and pinned.
      * the update with the explicit denominator (dT = dt q / rho_cv), and a root stopped at
        1e-10: each breaks the bound on the update test's rows;
      * the series one term short of its rule: stays UNDER the bound, as it must -- the rule stops
        where the next term is eps of the leading one, so the last term kept is about eps of the
        series sum, and the sum is one of the two operands whose rounding the bound grants
        (16 eps a c T^4); a series 8 terms short breaks it.  Cutting at the rule is sound, not
        merely unseen;
      * a remainder dB/dT without its clamp: NOT a defect -- it changes no value of the sweep,
        bit for bit (the clamp never acts, see the cases module), so no bound can see it."""
    from regions_material_ref import RegionMaterialReference
    missed = {}
    # the series one term short
    short1, short8, old_ok = 0.0, 0.0, True
    for name in ("log", "wide", "narrow", "straddle"):
        for deriv in (False, True):
            t = mc.planck_truth(oracle_mod, name, deriv)
            G = t.edges.size - 1
            x = np.stack([planck_np.planck_cell(t.T, t.edges, g, deriv=deriv, n_adjust=-1) for g in range(G)], axis=1)
            short1 = max(short1, float(_planck_ratio(x, t).max()))
            x8 = np.stack([planck_np.planck_cell(t.T, t.edges, g, deriv=deriv, n_adjust=-8) for g in range(G)], axis=1)
            short8 = max(short8, float(_planck_ratio(x8, t).max()))
            old_ok = old_ok and _old_planck_check(x, t.oracle, t.T, deriv)
            # no clamp: the same bits
            y = np.stack([planck_np.planck_cell(t.T, t.edges, g, deriv=deriv, clamp=False) for g in range(G)], axis=1)
            assert np.array_equal(y, t.npform), (name, deriv)
    print(f"series one term short: largest ratio {short1:.2f}; 8 terms short: {short8:.1f}")
    assert short1 <= K / 4 and short8 > K
    missed["series one term short"] = old_ok
    # the update's defects
    c = mc.update_case(oracle_mod)
    p, N = c.p, mc.UPDATE_N

    class Explicit(RegionMaterialReference):
        def material_update(self, qb):
            qb = np.array(qb)
            qb[N:] = 0.0
            super().material_update(qb)

    class LooseRoot(RegionMaterialReference):
        def _solve_cell(self, cc, q):
            exact = super()._solve_cell(cc, q)
            return exact * (1.0 + 1e-10)

    for name, cls in (("explicit denominator", Explicit), ("root stopped at 1e-10", LooseRoot)):
        s = cls(oracle_mod, p, mc.single_region(p), [c.rho_cv], c.T0)
        s.material_update(c.qb)
        got = mc.readouts(s)
        r = mc.update_ratios(got, c)
        assert max(float(v.max()) for v in r.values()) > K, name
        Terr = np.abs(got["T"] - c.oracle["T"]) / np.abs(c.oracle["T"])
        grey = mc.KCON_AC * c.oracle["T"].max() ** 4
        den = np.maximum(np.abs(c.oracle["Beff"]).max(axis=0), np.r_[[1e-4 * grey] * (mc.UPDATE_G - 1), 1e-3 * grey])
        Berr = (np.abs(got["Beff"] - c.oracle["Beff"]).max(axis=0) / den).max()
        missed[name] = bool(Terr.max() <= 1e-12 and Berr <= 1e-10)
    print("defects the fixed tolerances let through:", [k for k, v in missed.items() if v])
    assert missed == {"series one term short": True, "explicit denominator": False, "root stopped at 1e-10": False}


# ---------------------------------------------------------------------------
# conditions on the truth: the update test and the coupled steps
# ---------------------------------------------------------------------------
def _material_conditions(case, what, negative=None):
    """negative: {step: the truth's min T} of the steps listed in mc.NEGATIVE_T for this point --
    T > 0 after every other step, and after a listed one the listed minimum, to 1e-3 of it."""
    negative = negative or {}
    for k, v in case.truth.items():
        assert np.isfinite(np.asarray(v, dtype=np.float64)).all() and np.isfinite(case.oracle[k]).all(), (what, k)
    assert case.branch_same, what
    hist = case.history if isinstance(case.history, list) else [case.history]
    assert set(negative) <= set(range(1, len(hist) + 1)), what
    for k, h in enumerate(hist, start=1):
        assert np.isfinite(h["T"]).all() and (h["T"] != 0).all(), (what, k)
        if k in negative:
            assert negative[k] < 0 and abs(h["T"].min() - negative[k]) <= 1e-3 * abs(negative[k]), (what, k, h["T"].min())
        else:
            assert (h["T"] > 0).all(), (what, k, float(h["T"].min()))
        assert not (np.abs(h["ratio"] - 0.25) < 1e-6).any(), what
    assert np.array_equal(hist[-1]["T"], np.asarray(case.truth["T"], dtype=np.float64)), what
    assert ((case.oracle["T"] > 0) == (case.truth["T"] > 0)).all(), what
    Terr = np.abs(case.oracle["T"] - case.truth["T"]) / np.abs(case.truth["T"])
    assert Terr.max() <= ORACLE_ERR_MAX, (what, float(Terr.max()))
    return hist


@needs_extended
def test_update_conditions(oracle_mod):
    c = mc.update_case(oracle_mod)
    (h,) = _material_conditions(c, "update")
    rows = np.arange(mc.UPDATE_N - 25).reshape(len(mc.UPDATE_T0), len(mc.UPDATE_RATIOS), len(mc.UPDATE_STIFF))
    want = np.array(mc.UPDATE_RATIOS)
    for j, r in enumerate(want):  # the rows sit where they are meant to: 4e-4 either side of the switch
        got = h["ratio"][rows[:, j, :]]
        assert np.allclose(got, r, rtol=1e-12, atol=0), r
        assert h["solved"][rows[:, j, :]].all() == (r > 0.25) and h["solved"][rows[:, j, :]].any() == (r > 0.25)
    assert h["solved"][-25:].all() and (c.T0[-25:] == 0).all() and (c.qb[:mc.UPDATE_N][-25:] > 0).all()
    b, dtW = c.qb[mc.UPDATE_N:], c.w_sigma[0, 0] / (c.p["rho"] * c.p["kappa_grey"])
    got = (dtW * b / c.rho_cv).reshape(-1, len(mc.UPDATE_STIFF))
    assert np.allclose(got, np.array(mc.UPDATE_STIFF)[None, :], rtol=1e-12)
    assert (np.asarray(c.truth["Beff"]) >= 0).all() and (np.asarray(c.truth["Beff"]) == 0).any()  # a paid-out group
    r = mc.update_ratios(c.oracle, c)
    assert all(float(v.max()) <= 1.0 for v in r.values())  # the reference against its own bound


def _check_coupled(oracle_mod, cells, pt):
    c = mc.coupled_case(oracle_mod, cells, pt)
    what = (cells, mc.point_id(pt))
    hist = _material_conditions(c, what, mc.NEGATIVE_T.get((cells, pt)))
    check_conditions(c.truth["ends"], c.oracle["ends"])
    solved = [int(h["solved"].sum()) for h in hist]
    ts, cfl, bc, state, stiff = pt
    if state == "cold":
        assert sum(solved) > 0, what
    else:  # the linear update throughout, but at the points listed: there, the listed cells per step
        assert solved == list(mc.ROOT_SOLVED.get((cells, pt), [0] * mc.STEPS)), (what, solved)
    assert (c.stiffness0 >= stiff / 2).all() and (c.stiffness0 <= stiff * 2).all(), (what, c.stiffness0.min())
    assert c.steps == len(hist) == mc.STEPS
    return c


@needs_extended
@pytest.mark.parametrize("N", mc.UNIFORM_N)
@pytest.mark.parametrize("pt", mc.UNIFORM_GRID, ids=[mc.point_id(p) for p in mc.UNIFORM_GRID])
def test_uniform_conditions(oracle_mod, pt, N):
    _check_coupled(oracle_mod, N, pt)


@needs_extended
@pytest.mark.parametrize("pt", mc.REGION_GRID, ids=[mc.point_id(p) for p in mc.REGION_GRID])
def test_region_conditions(oracle_mod, pt):
    _check_coupled(oracle_mod, mc.REGION_CELLS, pt)


def test_case_lists_are_fixed():
    assert len(mc.UNIFORM_GRID) == 3 * 5 * 3 + 3 * (3 * 4 - 1) and len(set(mc.UNIFORM_GRID)) == len(mc.UNIFORM_GRID)
    assert len(mc.REGION_GRID) == 3 * 3 * 2 + (3 * 4 - 1) and len(set(mc.REGION_GRID)) == len(mc.REGION_GRID)
    assert len(mc.PLANCK_HANDLES) == 8 and len(mc.DBDT_SHARDS) == 36 and mc.planck_T().size == 130
