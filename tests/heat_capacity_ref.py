"""Numpy restatement of the tabulated internal energy e(T) of the material coupling
(include/rtsn.h rt_material_set_energy_table) -- TEST INFRASTRUCTURE ONLY.

HeatCapacityMixin over any of regions_material_ref.RegionMaterialReference,
opacity_law_ref.OpacityLawReference and opacity_table_ref.OpacityTableReference
(HeatCapacityReference is the last, which is also the other two with nothing set): region k's cells
hold the material energy per volume e_k(T) in place of rho_cv T, given at the nodes
T_0 < ... < T_{nT-1} as energy[k, j].  From the first node on, between the nodes and above the last,

    t = log(T / T_j) r_j,   r_j = 1 / log(T_{j+1} / T_j),   e = exp(t (ln e_{j+1} - ln e_j) + ln e_j),
    c_v = s_j e / T,        s_j = (ln e_{j+1} - ln e_j) r_j,

j the bracket of T (the last one above the last node); below the first node, T <= 0 included,
e = c_0 T and c_v = c_0 = e_0 / T_0.  (The header's fma written as a product and a sum: numpy has
no fma.)  r_j, ln e_j, s_j and c_0 are formed in np.longdouble and rounded once to the reference's
dtype, as the library forms them in long double on the host.

material_update is the header's step 3 with a table: T' the root of
g(T') = e(T') - e(T) + dt W b (T' - T) - dt q (q = 0: T' = T), and where T' - T > T / 4 the root of
e(T') - e(T) = dt (A - W S(T')).  Both roots by bisection, all cells at once, from a bracket found by
doubling a step away from T in the direction g's sign at T gives (no closed-form inverse: the
device's brackets are not restated here), until the bracket is at most 1e-15 relative in fp64 and
4 ulp in other dtypes, as the parents do.  Everything else -- the sweep, q, b, the owed emission,
_planck, the opacity law and table -- is the parent's.  Every update records the parent's history
(solved, ratio, T) and each cell's piece of the table before and after (-1 below the first node).

With the table off every operation is the parent's, bitwise.  The case the CPU and the GPU tests
share, and one cached reference run per case, are at the end of the file.
"""
from __future__ import annotations

import numpy as np

import opacity_law_ref as olr
import opacity_table_ref as otr
from opacity_table_ref import OpacityTableReference
from regions_material_ref import NEWTON_FRAC


class HeatCapacityMixin:
    eos = None

    # ---- the table ----
    def set_energy_table(self, T_grid, energy):
        """The table set, changed or (T_grid None) cleared: T(x) stays, nothing is rescaled."""
        if T_grid is None:
            self.eos = None
            return
        f, L = self.dtype, np.longdouble
        Tg = np.asarray(T_grid, dtype=np.float64)
        en = np.atleast_2d(np.asarray(energy, dtype=np.float64))
        assert en.shape == (len(self.tables), Tg.size) and Tg.size >= 2
        assert (np.diff(Tg) > 0).all() and Tg[0] > 0 and np.isfinite(Tg).all()
        assert (en > 0).all() and np.isfinite(en).all() and (np.diff(en, axis=1) > 0).all()
        rl = L(1) / np.log(Tg[1:].astype(L) / Tg[:-1].astype(L))
        le = np.log(en.astype(L))
        self.eos = (Tg.astype(f), rl.astype(f), le.astype(f), ((le[:, 1:] - le[:, :-1]) * rl[None, :]).astype(f),
                    (en[:, 0].astype(L) / L(Tg[0])).astype(f))

    def piece(self, T):
        """Each cell's piece of the table: -1 below the first node, else the bracket."""
        Tg = self.eos[0]
        with np.errstate(all="ignore"):
            up = np.asarray(T >= Tg[0])
        j = np.clip(np.searchsorted(Tg, np.where(up, T, Tg[0]), side="right") - 1, 0, len(Tg) - 2)
        return np.where(up, j, -1)

    def _energy(self, T, reg):
        """(e, c_v) at the temperatures T of cells of the regions reg, in self.dtype."""
        f = self.dtype
        Tg, r, le, s, c0 = self.eos
        T = np.asarray(T, dtype=f)
        with np.errstate(all="ignore"):
            up = T >= Tg[0]
            Ts = np.where(up, T, Tg[0])
            j = np.clip(np.searchsorted(Tg, Ts, side="right") - 1, 0, len(Tg) - 2)
            t = np.log(Ts / Tg[j]) * r[j]
            l0, l1 = le[reg, j], le[reg, j + 1]
            eh = np.exp(t * (l1 - l0) + l0)
            return (np.where(up, eh, c0[reg] * T).astype(f), np.where(up, s[reg, j] * eh / Ts, c0[reg]).astype(f))

    def _bisect(self, g, T):
        """The root of the increasing g(t, idx) (idx: positions in T) per entry of T: a bracket by
        doubling a step away from T, then bisection until it is below the dtype's tolerance."""
        f = self.dtype
        n = T.size
        if n == 0:
            return T.copy()
        idx = np.arange(n)
        g0 = g(T, idx)
        up = g0 < 0                                # the root lies above T
        step = np.maximum(np.abs(T), f(1e-3))
        lo, hi = np.where(up, T, T - step), np.where(up, T + step, T)
        for _ in range(2000):
            bad = np.where(up, g(hi, idx) < 0, g(lo, idx) > 0) & (g0 != 0)
            if not bad.any():
                break
            step = np.where(bad, f(2) * step, step)
            hi = np.where(bad & up, T + step, hi)
            lo = np.where(bad & ~up, T - step, lo)
        else:
            raise AssertionError("no bracket")
        tol = f(1e-15) if f is np.float64 else 4 * np.finfo(f).eps
        live = g0 != 0
        for _ in range(40000):
            mid = f(0.5) * (lo + hi)
            live = live & (hi - lo > tol * np.abs(hi)) & (lo < mid) & (mid < hi)
            if not live.any():
                break
            k = np.flatnonzero(live)
            gm = np.zeros(n, dtype=f)
            gm[k] = g(mid[k], k)
            upm = live & (gm > 0)
            hi = np.where(upm, mid, hi)
            lo = np.where(live & ~upm, mid, lo)
        return np.where(g0 == 0, T, f(0.5) * (lo + hi))

    def _emission(self, cells, t):
        """S(t) = sum over ALL groups of sigma_g B_g(t) with the cells' (lagged) opacities."""
        if self.native:
            return np.array([self._emission_all(c, tc) for c, tc in zip(cells, t)], dtype=self.dtype)
        return (self.sigma_all_cells[cells] * self._planck_terms(t, 0, self.G)).sum(axis=1)

    # ---- step 3 ----
    def material_update(self, qb):
        if self.eos is None:
            return super().material_update(qb)
        f = self.dtype
        N, dt, W, reg = self.N, f(self.p["dt"]), self.W, self.cell_region
        qb = np.asarray(qb, dtype=f)
        q, b, T = qb[:N], qb[N:], self.T
        e0, _ = self._energy(T, reg)
        dtWb = dt * W * b
        move = np.flatnonzero(q != 0)

        def g_lin(t, idx):
            c = move[idx]
            return (self._energy(t, reg[c])[0] - e0[c]) + dtWb[c] * (t - T[c]) - dt * q[c]

        Tl = T.copy()
        Tl[move] = self._bisect(g_lin, T[move])
        dT = Tl - T
        solve = ~(dT <= f(NEWTON_FRAC) * T)
        with np.errstate(all="ignore"):
            ratio = np.where(T != 0, np.asarray(dT / np.where(T != 0, T, 1), dtype=np.float64), np.copysign(np.inf, dT))
        self.history.append(dict(solved=solve.copy(), ratio=np.asarray(ratio, dtype=np.float64),
                                 before=self.piece(T)))
        Tn, dTl = Tl.copy(), dT.copy()
        cells = np.flatnonzero(solve)
        if cells.size:
            A = q[cells] + W * self._emission(cells, T[cells])

            def g_full(t, idx):
                c = cells[idx]
                return (self._energy(t, reg[c])[0] - e0[c]) + dt * W * self._emission(c, t) - dt * A[idx]

            Tr = self._bisect(g_full, T[cells])
            self.owed[cells] += self._planck_terms(Tr, self.g_lo, self.g_lo + self.Gl) - self.Bcell[cells]
            Tn[cells], dTl[cells] = Tr, 0
            self.newton_cells += int(cells.size)
        self.T, self.dTlast = Tn, dTl
        self.history[-1]["T"] = np.asarray(Tn, dtype=np.float64)
        self.history[-1]["after"] = self.piece(Tn)
        self._planck()

    # ---- read-outs ----
    def material_energy(self):
        """(N) e(T(x)) with the table, rho_cv(x) T(x) without."""
        if self.eos is None:
            return self.rho_cv_cells * self.T
        return self._energy(self.T, self.cell_region)[0]

    def heat_capacity(self):
        """(N) c_v(T(x)) with the table, rho_cv(x) without."""
        if self.eos is None:
            return self.rho_cv_cells.copy()
        return self._energy(self.T, self.cell_region)[1]


class HeatCapacityReference(HeatCapacityMixin, OpacityTableReference):
    def __init__(self, oracle_mod, p, regions, rho_cv, T_cells=None, g_lo=0, g_hi=0, dtype=np.float64, table=None,
                 law=None, energy_table=None):
        """energy_table: None, or (T_grid (nT), energy (regions, nT)), set before any step; table, law:
        the parent's opacity table and law."""
        super().__init__(oracle_mod, p, regions, rho_cv, T_cells, g_lo, g_hi, dtype, table=table, law=law)
        if energy_table is not None:
            self.set_energy_table(*energy_table)


def energy(s, dx_cells):
    """sum_x dx(x) (sum_g phi_g / c + e(T(x)) + transit) of a solver or a reference: the BE energy
    statement with the material's internal energy in it (material_energy())."""
    phi = s.moments()[0]
    return float((dx_cells * (phi.sum(axis=0) / olr.C_LIGHT + np.asarray(s.material_energy(), dtype=np.float64)
                              + s.material_transit())).sum())


# ---------------------------------------------------------------------------
# the shared case
# ---------------------------------------------------------------------------
STEPS, BCS, SCHEME_DT = olr.STEPS, olr.BCS, olr.SCHEME_DT
# per layout: the nodes, e at the first node per region, the exponents s_j per region and bracket.
# (16, 16) cells heat through the (32, 48) table's last bracket within three steps, after which no
# cell changes its piece and, for BE, none solves the full emission: its nodes were moved (two more
# between 0.1 and 2.0, other exponents) until test_heat_capacity.test_case_conditions held for every
# scheme and boundary pair
ENERGY_TABLES = {
    "n80": dict(T_grid=(0.03, 0.1, 0.4, 2.0), e_first=(0.15, 0.015), exponents=((1.5, 1.0, 2.5), (0.6, 1.8, 1.2))),
    "n32": dict(T_grid=(0.03, 0.1, 0.3, 0.6, 0.9, 1.2, 2.0), e_first=(0.0132, 0.0872),
                exponents=((0.7, 1.6, 1.2, 2.7, 2.4, 3.9), (1.3, 0.9, 0.6, 1.2, 3.6, 2.7))),
}
ENERGY_TABLES["plain"] = ENERGY_TABLES["n80"]        # (a plain handle: region 0's row)
COLD_CELLS, COLD_T = 8, 0.02                         # the last cells start below the first node


def power_nodes(T_grid, e_first, exponents):
    """e_{j+1} = e_j (T_{j+1} / T_j)^(s_j) per region: (T_grid, energy (regions, nT))."""
    Tg = np.asarray(T_grid, dtype=np.float64)
    rows = []
    for e0, s in zip(e_first, exponents):
        row = [float(e0)]
        for j, sj in enumerate(s):
            row.append(row[-1] * (Tg[j + 1] / Tg[j]) ** sj)
        rows.append(row)
    return Tg, np.array(rows)


def energy_table(layout="n80", nregions=2):
    t = ENERGY_TABLES[layout]
    Tg, en = power_nodes(t["T_grid"], t["e_first"], t["exponents"])
    return Tg, en[:nregions]


def case(oracle_mod, layout, ts, bc):
    """opacity_law_ref.case (its rho_cv only what the handle falls back to) with the last 8 cells
    at 0.02, below the first node."""
    p, regions, rho_cv, T0 = olr.case(oracle_mod, layout, ts, bc)
    T0 = T0.copy()
    T0[-COLD_CELLS:] = COLD_T
    return p, regions, rho_cv, T0


def plain_case(oracle_mod, ts, bc):
    """A plain handle's case: layout n32's parameters as one medium of 32 cells, region 0's row
    of the table.  (p, the one-region list the reference takes, rho_cv, T0)."""
    p, regions, rho_cv, T0 = case(oracle_mod, "n32", ts, bc)
    one = [dict(cells=p["N"], width=p["X"], rho=p["rho"], kappa_grey=p["kappa_grey"], T=p["T"], group_kappa=None)]
    return p, one, rho_cv[0], T0


_runs = {}


def reference_run(oracle_mod, layout, ts, bc, law=None, table=None, g_lo=0, g_hi=0):
    """One fp64 reference run of STEPS steps per case, computed once and left unchanged: the
    reference after the last step and per step the BE residual relative to the total, min T and
    min Beff (the pieces and paths are in ref.history).  layout "plain": plain_case."""
    key = (layout, ts, bc, law, table, g_lo, g_hi)
    if key not in _runs:
        from test_material import net_outflow
        if layout == "plain":
            p, regions, rho_cv, T0 = plain_case(oracle_mod, ts, bc)
            rho_cv = [rho_cv]
        else:
            p, regions, rho_cv, T0 = case(oracle_mod, layout, ts, bc)
        ref = HeatCapacityReference(oracle_mod, p, regions, rho_cv, T0, g_lo=g_lo, g_hi=g_hi,
                                    law=olr.law_args(law) if law else None,
                                    table=otr.table_args(table, p["G"]) if table else None,
                                    energy_table=energy_table(layout, len(regions)))
        rec = dict(ref=ref, p=p, regions=regions, rho_cv=rho_cv, T0=T0, resid=[], Tmin=[], Tmax=[], Bmin=[])
        view = olr._RefView(ref)
        for _ in range(STEPS):
            e0 = energy(ref, ref.dx_cells)
            ref.material_step(1)
            e1 = energy(ref, ref.dx_cells)
            rec["resid"].append(((e1 - e0) + p["dt"] * net_outflow(view, p)) / e1)
            rec["Tmin"].append(float(ref.temperature().min()))
            rec["Tmax"].append(float(ref.temperature().max()))
            rec["Bmin"].append(float(ref.cell_emission().min()))
        _runs[key] = rec
    return _runs[key]
