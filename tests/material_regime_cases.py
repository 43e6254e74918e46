"""Regime sweep of the material-temperature coupling: cases and metric, shared by
tests/test_material_regime_ref.py (CPU) and tests/test_material_regime_gpu.py.  No GPU import.

Truth: the coupling's own algorithm in np.longdouble on the fp64 inputs -- oracle/planck_np.py
for the Planck terms, tests/regions_material_ref.py (RegionMaterialReference, dtype
np.longdouble) for the update, the root and the sweep.  fp64 reference: the C oracle
(orc_planck_cell*, orc_material_*) on a uniform slab, RegionMaterialReference in fp64 on regions.

Metric.  A cell-indexed group quantity (B, dB/dT, Beff), per group g over a set of cells (a
decade of T in the Planck sweep and the update test, the whole slab in a coupled step):

    E(x)[g] = max_cells |x - truth| / max_cells |truth|

T per cell, relative; psi / ends by regime_cases.line_err; and the code under test must satisfy

    E(gpu) <= K max(E(fp64 reference), 16 eps),  K = 32 (regime_cases.K)

with no other floor but one: for the remainder group and for a group evaluated by the series or
the split branch at some cell of the set, E(reference) is taken as no less than
16 eps kcon a c T^4 (dB/dT: 16 eps kcon 4 a c T^3, the same statement differentiated) at that
cell over max|truth| -- both operands of the branch's final subtraction s(z1) - s(z2), and of
a c T^4 - (rest), are rounded at that scale, whatever is left of them.  The transit energy
dt W sum_g sigma_g (...) is a sum over the groups of such terms: it is measured like a group
quantity (over the same cell sets) with the groups' floors summed with its weights dt W sigma_g.
Where every truth of a set is 0 the value must be 0 too (E = 0, else inf).

Why the bound adapts (measured against a 40-digit evaluation of the same algorithm): the fp64
oracle's own relative error in B_g, dB_g/dT is 5.6e-9, 1.1e-8 at T = 1000 on edges from 1e-6
(z ~ 1e-9, exp(x) - 1 cancels), 3e-10 at T = 50 there, 2.5e-11 in groups of relative width 1e-4
at T = 0.1, 3e-7 in a remainder group that is 1.3e-10 of a c T^4, and 1 where e^{-z} underflows
(it returns 0 for a tiny positive truth).  K: the device's evaluation order emulated in fp64
(planck_np.planck_device_form) stays within 1.8x of the bound's right-hand side on every (grid,
group, decade) of the Planck sweep (G = 34, dB/dT) -- test_emulation_margin of
tests/test_material_regime_ref.py asserts K / 4 = 8 -- leaving the rest for FMA contraction, the
device's exp and, in the coupled steps, the sweep (regime_cases: 4.9x of its own).

The remainder's positivity clamp never acts on this case list, in either precision: a c carries
the reference's pi = 3.1415926546 (> pi) to the fifth power, so the grey total exceeds the full
Bose integral by 1.3e-10 of itself and a c T^4 - (any partial integral) stays positive for every
T whose fourth power is a normal number.  test_material_regime_ref.test_planck_conditions pins
that; a remainder without its clamp is therefore no defect any input can show.
"""
from collections import namedtuple

import numpy as np

import planck_np
import regime_cases as rc
from regime_cases import EPS, FLOOR, K, line_err

KCON_AC = planck_np.C_BOLTZ_JPK * planck_np.A_C

# ---------------------------------------------------------------------------
# 1: the Planck sweep
# ---------------------------------------------------------------------------
PLANCK_N = 130  # three 64-cell tiles, the last with two live lanes


def planck_T():
    """16 values per decade from 1e-3 to 1e3 (T = 1 exactly), 30 more between them, and 0, -1,
    1e-8 -- the three at the head of the second tile, the last tile's two lanes ordinary."""
    T = 10.0 ** (np.arange(97) / 16.0 - 3.0)
    T[48] = 1.0
    out = np.concatenate([T[:64], [0.0, -1.0, 1e-8], T[64:], T[1::3][:30] * 1.37])
    assert out.size == PLANCK_N
    return out


def log_edges(G, efirst, elast):
    """generate_group_edges as the oracle restates it."""
    if G == 1:
        return np.array([0.0, efirst])
    fac = np.exp((np.log(elast) - np.log(efirst)) / (G - 1.0))
    e = [0.0, efirst]
    for _ in range(1, G):
        e.append(e[-1] * fac)
    return np.array(e)


# name: (G, efirst, elast) of a log grid, or the edges themselves (G + 1)
PLANCK_GRIDS = {
    "log": (12, 1e-3, 30.0),
    "wide": (12, 1e-6, 1e4),
    "narrow": 0.1 * (1.0 + 1e-4) ** np.arange(13),
    # at T = 1: [.45, .55] straddles z = 0.5, [.55, .65] 0.6, [.65, .75] 0.7 (Gauss, Gauss, series);
    # [.1, .45] splits at T = 0.5; the remainder's joint integral [.1, 1.2] splits at T = 1
    "straddle": np.array([0.1, 0.45, 0.55, 0.65, 0.75, 1.2, 3.0]),
    "G1": (1, 0.1, 10.0),
    "G2": (2, 0.1, 10.0),
    "G34": (34, 1e-3, 30.0),  # two 32-group tiles, the second with two groups
}
PLANCK_HANDLES = [(name, 0, 0) for name in PLANCK_GRIDS] + [("G34", 31, 34)]
DBDT_SHARDS = [(name, g, g + 1) for name in ("log", "wide", "narrow") for g in range(12)]


def grid_edges(name):
    g = PLANCK_GRIDS[name]
    return log_edges(*g) if isinstance(g, tuple) else np.asarray(g, dtype=np.float64)


def planck_params(oracle_mod, name, N=PLANCK_N):
    """sigma_g = 1 in every group (rho = kappa = 1), so a one-group shard's b is dB_g/dT itself."""
    g = PLANCK_GRIDS[name]
    p = oracle_mod.default_params()
    G = g[0] if isinstance(g, tuple) else len(g) - 1
    p.update(M=2, G=G, N=N, X=1.0, dx=1.0 / N, bc_left=0, bc_right=0, use_mg_equilib=0, rho=1.0, kappa_grey=1.0,
             T=1.0, V=0.0, use_correction=0, ts_method=1, dt=1e-6, max_timesteps=1, include_validation=0)
    if isinstance(g, tuple):
        p.update(efirst=g[1], elast=g[2])
    else:
        p.update(group_bounds=np.asarray(g, dtype=np.float64), have_group_bounds=1)
    p["psi_source"] = np.zeros((2, G))
    return p


def decade_bins(T):
    """{decade: cell indices} of the cells with T > 0."""
    T = np.asarray(T, dtype=np.float64)
    live = np.flatnonzero((T > 0) & np.isfinite(T))
    dec = np.floor(np.log10(T[live]) + 1e-9).astype(int)
    return {int(d): live[dec == d] for d in np.unique(dec)}


PlanckTruth = namedtuple("PlanckTruth", "T edges truth oracle npform branch floor clamped bins")
_planck = {}


def planck_truth(oracle_mod, name, deriv):
    """Every group of one grid at planck_T(): truth, the C oracle, planck_np in fp64 (each (N, G)),
    the branch per (cell, group), the exception's floor 16 eps kcon a c T^4 where it applies."""
    key = (name, deriv)
    if key not in _planck:
        T, e = planck_T(), grid_edges(name)
        G = e.size - 1
        fn = oracle_mod.planck_cell_dBdT if deriv else oracle_mod.planck_cell
        truth = np.empty((T.size, G), dtype=np.longdouble)
        npf, orc = np.empty((T.size, G)), np.empty((T.size, G))
        branch, clamped = np.zeros((T.size, G), dtype=int), np.zeros((T.size, G), dtype=bool)
        for g in range(G):
            info = {}
            truth[:, g] = planck_np.planck_cell(T, e, g, np.longdouble, deriv=deriv, info=info)
            npf[:, g] = planck_np.planck_cell(T, e, g, np.float64, deriv=deriv)
            orc[:, g] = [fn(t, e, g) for t in T]
            branch[:, g], clamped[:, g] = info["branch"], info["clamped"]
        _planck[key] = PlanckTruth(T, e, truth, orc, npf, branch, rounding_floor(T, e, 0, G, deriv), clamped,
                                   decade_bins(T))
    return _planck[key]


def rounding_floor(T, edges, g_lo, g_hi, deriv=False):
    """(N, g_hi - g_lo): 16 eps kcon a c T^4 (deriv: 4 a c T^3) where group g at cell x is the
    remainder or takes the series or the split branch, else 0."""
    T64 = np.asarray(T, dtype=np.float64)
    G = len(edges) - 1
    Tp = np.where((T64 > 0) & np.isfinite(T64), T64, 0.0)
    scale = 16.0 * EPS * KCON_AC * (4.0 * Tp ** 3 if deriv else Tp ** 4)
    out = np.zeros((T64.size, g_hi - g_lo))
    for g in range(g_lo, g_hi):
        if g == G - 1:
            out[:, g - g_lo] = scale
        else:
            br = planck_np.integrate(T64, edges[g], edges[g + 1], np.float64)[1]
            out[:, g - g_lo] = np.where(br >= planck_np.SERIES, scale, 0.0)
    return out


# ---------------------------------------------------------------------------
# the metric
# ---------------------------------------------------------------------------
def group_err(x, truth, cells=slice(None)):
    """(G,): E over the cells of x, truth (N, G); all-zero truth: 0 where x is 0 too, else inf."""
    t = np.asarray(truth, dtype=np.longdouble)[cells]
    d = np.abs(np.asarray(x, dtype=np.longdouble)[cells] - t).max(axis=0)
    s = np.abs(t).max(axis=0)
    with np.errstate(all="ignore"):
        e = np.where(s > 0, d / np.where(s > 0, s, 1), np.where(d > 0, np.inf, 0))
    return np.asarray(e, dtype=np.float64)


def group_bound(ref, truth, floor, cells=slice(None)):
    """(G,): max(E(ref), 16 eps, the exception's floor over max|truth|) over the cells."""
    s = np.asarray(np.abs(np.asarray(truth, dtype=np.longdouble)[cells]).max(axis=0), dtype=np.float64)
    with np.errstate(all="ignore"):
        fl = np.where(s > 0, np.asarray(floor)[cells].max(axis=0) / np.where(s > 0, s, 1.0), 0.0)
    return np.maximum(np.maximum(group_err(ref, truth, cells), FLOOR), fl)


def group_ratio(x, ref, truth, floor, bins):
    """(bins, G): E(x) / bound per cell set of bins (a dict of index arrays)."""
    x = np.asarray(x)
    assert np.isfinite(x).all()
    return np.array([group_err(x, truth, c) / group_bound(ref, truth, floor, c) for c in bins.values()])


def cell_ratio(x, ref, truth):
    """(N,): per cell |x - truth| / |truth| over max(the reference's, 16 eps)."""
    t = np.asarray(truth, dtype=np.longdouble)
    assert np.isfinite(np.asarray(x)).all() and (t != 0).all()
    ex = np.abs(np.asarray(x, dtype=np.longdouble) - t) / np.abs(t)
    er = np.abs(np.asarray(ref, dtype=np.longdouble) - t) / np.abs(t)
    return np.asarray(ex / np.maximum(er, FLOOR), dtype=np.float64)


def assert_bound(r, what):
    r = np.asarray(r)
    assert (r <= K).all(), (what, float(np.max(r)), np.argwhere(r > K)[:8].tolist())
    return float(np.max(r)) if r.size else 0.0


# ---------------------------------------------------------------------------
# 2: the update kernel alone
# ---------------------------------------------------------------------------
UPDATE_N, UPDATE_G = 300, 5
UPDATE_RATIOS = (-0.9, -1e-6, 0.0, 1e-6, 0.2, 0.2499, 0.2501, 0.3, 3.0, 1e3, 1e6)   # dT / T0 of the linear update
UPDATE_STIFF = (1e-4, 1.0, 1e4, 1e8, 1e12)                                         # dt W b / rho_cv
UPDATE_T0 = (1e-3, 1.7e-2, 0.3, 5.0, 1e2)
UPDATE_COLD = (1e-3, 0.1, 1.0, 30.0, 1e4)  # a cell at T0 = 0: the T it would reach without emitting

UpdateCase = namedtuple("UpdateCase", "p rho_cv T0 qb truth oracle bins floor w_sigma history branch_same")
_update = {}


def readouts(s):
    return {"T": s.temperature(), "Beff": s.cell_emission().T, "transit": s.material_transit()}


def single_region(p):
    return [dict(cells=p["N"], width=p["X"], rho=p["rho"], kappa_grey=p["kappa_grey"], T=p["T"],
                 group_kappa=p.get("group_kappa"))]


def update_case(oracle_mod):
    """One handle, N = 300: rows (T0, dT / T0, stiffness) and 25 cells at T0 = 0 with q > 0.  One
    rho_cv = dt W S(1) (the emission matters from T ~ 1 on, so a cell told to heat a million-fold
    ends at a finite T), b = stiffness rho_cv / (dt W), q = ratio T0 (rho_cv + dt W b) / dt."""
    if "case" not in _update:
        from regions_material_ref import RegionMaterialReference
        from test_material import params
        p = params(oracle_mod, ts=1, M=4, G=UPDATE_G, N=UPDATE_N, kappa=1.0, dt=1e-3, bc_left=0, bc_right=0)
        o = oracle_mod.OracleSolver(p)
        W, dt = float(o.quad()[1].sum()), p["dt"]
        e, sigma = o.groups()["e_edge"], p["rho"] * o.groups()["kappa"]
        rho_cv = dt * W * float(sum(sigma[g] * oracle_mod.planck_cell(1.0, e, g) for g in range(UPDATE_G)))
        rows = [(t, r, s) for t in UPDATE_T0 for r in UPDATE_RATIOS for s in UPDATE_STIFF]
        rows += [(0.0, t1, s) for t1 in UPDATE_COLD for s in UPDATE_STIFF]
        assert len(rows) == UPDATE_N
        T0 = np.array([r[0] for r in rows])
        b = np.array([r[2] for r in rows]) * rho_cv / (dt * W)
        q = np.array([(r[1] * r[0] if r[0] > 0 else r[1]) * (rho_cv + dt * W * bb) / dt for r, bb in zip(rows, b)])
        qb = np.concatenate([q, b])
        orc = oracle_mod.OracleSolver(p)
        orc.material_enable(rho_cv, T0)
        orc.material_update(qb)
        out = []
        for dtype in (np.longdouble, np.float64):
            ref = RegionMaterialReference(oracle_mod, p, single_region(p), [rho_cv], T0, dtype=dtype)
            ref.material_update(qb)
            out.append(ref)
        truth = readouts(out[0])
        same = np.array_equal(out[0].history[0]["solved"], out[1].history[0]["solved"])
        Tn = np.asarray(truth["T"], dtype=np.float64)
        floor = rounding_floor(Tn, e, 0, UPDATE_G)
        _update["case"] = UpdateCase(p, rho_cv, T0, qb, truth, readouts(orc), decade_bins(Tn), floor,
                                     np.tile(dt * W * sigma, (UPDATE_N, 1)), out[0].history[0], same)
    return _update["case"]


def transit_ratio(x, case):
    """(sets,): the transit energy as a one-column group quantity, the groups' floors summed with
    its weights dt W sigma_g(x)."""
    col = lambda a: np.asarray(a)[:, None]  # noqa: E731
    fl = (case.floor * case.w_sigma).sum(axis=1)
    return group_ratio(col(x), col(case.oracle["transit"]), col(case.truth["transit"]), col(fl), case.bins)[:, 0]


def update_ratios(got, case):
    """{"T", "Beff", "transit"}: the ratios of a solver's read-outs (T (N), Beff (N, G), transit
    (N)) against an UpdateCase or a CoupledCase."""
    return {"T": cell_ratio(got["T"], case.oracle["T"], case.truth["T"]),
            "Beff": group_ratio(got["Beff"], case.oracle["Beff"], case.truth["Beff"], case.floor, case.bins),
            "transit": transit_ratio(got["transit"], case)}


# ---------------------------------------------------------------------------
# 3: coupled steps
# ---------------------------------------------------------------------------
STEPS = 6
UNIFORM_N = (70, 320)
STATES = ("equilibrium", "hot", "cold")
STIFF = (1e-3, 1.0, 1e3, 1e6)
# (scheme, c dt / dx, boundary pair, start state, stiffness)
UNIFORM_GRID = ([(ts, cfl, bc, "hot", 1.0) for ts in rc.SCHEMES for cfl in rc.CFL for bc in rc.BCS]
                + [(ts, 1.0, (2, 1), st, sf) for ts in rc.SCHEMES for st in STATES for sf in STIFF
                   if (st, sf) != ("hot", 1.0)])
REGION_CELLS = (16, 32, 16)
REGION_CFL = (1e-2, 1.0, 1e2)
REGION_GRID = ([(ts, cfl, (bl, 1), "hot", 1.0) for ts in rc.SCHEMES for cfl in REGION_CFL for bl in (1, 2)]
               + [(1, 1.0, (2, 1), st, sf) for st in STATES for sf in STIFF if (st, sf) != ("hot", 1.0)])
# Every point takes all six steps: none has the fp64 reference's error pass ORACLE_ERR_MAX (the
# largest error in T over the grids is 4.6e-12).
#
# Where the truth itself has T < 0 after a step -- (cells, point): {step: min T}, measured, and
# asserted step by step by test_material_regime_ref (T > 0 after every step not listed here).  The
# issue's cases and its condition "T > 0 after every step" do not meet at these points; the cases
# are kept as set and compared like every other (T per cell, relative), since the device has to
# follow the reference's algorithm there too.
#  * CN and BDF2 from the cold start, at every stiffness: neither scheme is positive, and with
#    c dt sigma up to 1e4 the first step throws psi -- which starts at B(T_rad), 1.6e5 above the
#    cold emission -- below zero in the opaque groups.  q = sum_g sigma_g (phi_g - W B_g) < 0, no
#    cell solves the root in that step, and the linear update leaves every cell at T < 0 (B = 0
#    for a step); the second update solves the root in every cell and returns to T > 0, except at
#    the largest heat capacity (stiffness 1e-3), where CN dips again after step 3 and BDF2 stays
#    negative in all cells but one.  "Cold solves the root" therefore holds from step 2 on; BE
#    (positive) solves it in step 1 and keeps T > 0 throughout.
#  * BDF2 at c dt / dx = 1e4 on 320 cells: the reference's BDF2 grows the state step by step there
#    (regime_cases.LONG_GRID) and turns phi, and with it T, negative in the sixth step.
_COLD_NEG = {
    (2, 1e-3): {1: -49103, 3: -104.8},
    (2, 1.0): {1: -2.4576e+07},
    (2, 1e3): {1: -4.9104e+07},
    (2, 1e6): {1: -4.9153e+07},
    (3, 1e-3): {1: -49070, 2: -32.322, 3: -49012, 4: -107.07, 5: -48958, 6: -176.79},
    (3, 1.0): {1: -2.4559e+07},
    (3, 1e3): {1: -4.907e+07},
    (3, 1e6): {1: -4.9119e+07},
}
NEGATIVE_T = {(N, (ts, 1.0, (2, 1), "cold", sf)): v  # a uniform slab: the same at both N
              for N in UNIFORM_N for (ts, sf), v in _COLD_NEG.items()}
NEGATIVE_T.update({
    (320, (3, 1e4, (1, 1), "hot", 1.0)): {6: -149.69},
    (320, (3, 1e4, (2, 1), "hot", 1.0)): {6: -336.2},
    (320, (3, 1e4, (0, 0), "hot", 1.0)): {6: -48.062},
})
# Where a hot or an equilibrium start solves the root all the same -- (cells, point): cells per
# step, measured and asserted; everywhere else these states take the linear update in every cell
# of every step.  All are BDF2 at large c dt / dx (1e4 on 320 cells, where the same growth ends in
# the three points above; 1e2 on the regions).
ROOT_SOLVED = {
    (320, (3, 1e4, (1, 1), "hot", 1.0)): (0, 0, 0, 0, 47, 0),
    (320, (3, 1e4, (2, 1), "hot", 1.0)): (0, 0, 0, 0, 320, 0),
    (320, (3, 1e4, (0, 0), "hot", 1.0)): (0, 0, 0, 0, 0, 57),
    (REGION_CELLS, (3, 1e2, (1, 1), "hot", 1.0)): (0, 0, 0, 0, 1, 1),
    (REGION_CELLS, (3, 1e2, (2, 1), "hot", 1.0)): (5, 2, 4, 5, 14, 9),
}

CoupledCase = namedtuple("CoupledCase", "p q regions rho_cv T0 steps truth oracle bins floor w_sigma history "
                                        "branch_same stiffness0")
_coupled = {}


def point_id(pt):
    ts, cfl, bc, st, sf = pt
    return f"{ts}-{cfl:g}-{bc[0]}{bc[1]}-{st}-{sf:g}"


def start_T(state, T_rad, N):
    T_rad = np.broadcast_to(np.asarray(T_rad, dtype=np.float64), (N,))
    if state == "equilibrium":
        return T_rad.copy()
    if state == "cold":
        return T_rad / 20.0
    return 3.0 * T_rad * (1.0 + 0.1 * np.sin(2.0 * np.pi * (np.arange(N) + 0.5) / N))


def _base_T(state, T_rad):
    return {"equilibrium": T_rad, "cold": T_rad / 20.0, "hot": 3.0 * T_rad}[state]


def coupled_readouts(s):
    return dict(readouts(s), ends=s.ends())


def coupled_case(oracle_mod, cells, pt):
    """cells: N of a uniform slab, or the cells of the three regions (regime_cases' contrasts).
    rho_cv (per region) = dt W b0 / stiffness, b0 = sum_g sigma_g dB_g/dT at the state's base T."""
    key = (cells, pt)
    if key in _coupled:
        return _coupled[key]
    from regions_material_ref import RegionMaterialReference
    ts, cfl, bc, state, stiff = pt
    steps = STEPS
    uniform = isinstance(cells, int)
    N = cells if uniform else int(sum(cells))
    p = rc.medium(oracle_mod, N, ts, cfl, bc, 0.0, steps)
    if uniform:
        regions = single_region(p)
    else:
        widths = [c * d for c, d in zip(cells, rc.REGION_DX)]
        p["X"] = float(sum(widths))
        p["dx"] = p["X"] / N
        regions = [dict(cells=int(c), width=float(w), rho=1.0, kappa_grey=p["kappa_grey"], T=float(T),
                        group_kappa=s * np.array(rc.SIGMA_DX) / d)
                   for c, w, s, d, T in zip(cells, widths, rc.REGION_SIGMA_DX, rc.REGION_DX, rc.REGION_T)]
    o = oracle_mod.OracleSolver(p)
    W, e = float(o.quad()[1].sum()), o.groups()["e_edge"]
    rho_cv = []
    for r in regions:
        b0 = sum(r["rho"] * r["group_kappa"][g] * oracle_mod.planck_cell_dBdT(_base_T(state, r["T"]), e, g)
                 for g in range(rc.G))
        rho_cv.append(p["dt"] * W * float(b0) / stiff)
    T0 = start_T(state, np.repeat([r["T"] for r in regions], [r["cells"] for r in regions]), N)
    truth = RegionMaterialReference(oracle_mod, p, regions, rho_cv, T0, dtype=np.longdouble)
    stiff0 = np.asarray(p["dt"] * truth.W * truth.bpart / truth.rho_cv_cells, dtype=np.float64)
    truth.material_step(steps)
    if uniform:
        ref = oracle_mod.OracleSolver(p)
        ref.material_enable(rho_cv[0], T0)
        same = True
        for k in range(steps):
            qb = ref.material_sweep()
            dT = p["dt"] * qb[:N] / (rho_cv[0] + p["dt"] * W * qb[N:])  # orc_material_update's own test
            same = same and np.array_equal(~(dT <= 0.25 * ref.temperature()), truth.history[k]["solved"])
            ref.material_update(qb)
    else:
        ref = RegionMaterialReference(oracle_mod, p, regions, rho_cv, T0)
        ref.material_step(steps)
        same = all(np.array_equal(a["solved"], b["solved"]) for a, b in zip(ref.history, truth.history))
    tr = coupled_readouts(truth)
    Tn = np.asarray(tr["T"], dtype=np.float64)
    w_sigma = p["dt"] * W * np.asarray(truth.sigma_cells, dtype=np.float64)  # (N, G): per cell on regions
    case = CoupledCase(p, rc.to_rt(p), None if uniform else regions, rho_cv, T0, steps, tr, coupled_readouts(ref),
                       {"slab": np.arange(N)}, rounding_floor(Tn, e, 0, rc.G), w_sigma, truth.history, same, stiff0)
    _coupled[key] = case
    return case


def coupled_ratios(got, case):
    """{"T", "ends", "Beff", "transit"} of a solver's read-outs (T (N), ends (M, G, N, 2), Beff
    (N, G), transit (N)) against a CoupledCase."""
    err_o = rc.check_conditions(case.truth["ends"], case.oracle["ends"])
    assert np.isfinite(np.asarray(got["ends"])).all()
    return {"T": cell_ratio(got["T"], case.oracle["T"], case.truth["T"]),
            "ends": line_err(got["ends"], case.truth["ends"]) / np.maximum(err_o, FLOOR),
            "Beff": group_ratio(got["Beff"], case.oracle["Beff"], case.truth["Beff"], case.floor, case.bins),
            "transit": transit_ratio(got["transit"], case)}
