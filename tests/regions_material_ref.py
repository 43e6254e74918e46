"""Numpy restatement of the material-temperature coupling on a slab of regions
(include/rtsn.h rt_material_enable_regions) -- TEST INFRASTRUCTURE ONLY.

One coupled step, per cell x with its own sigma_g(x), rho_cv(x) and dx(x):

* the sweep is regions_reference.RegionReference's (fused_np.LineSet's cell algebra, the mu < 0
  half mirrored), on the LineSets of the UNIT source -- B_g = 1, correction off -- one per
  region, with the constant Sc multiplied per cell by the step's emission Beff[x, g];
* B_g(T), dB_g/dT(T) per cell from the C oracle's planck_cell / planck_cell_dBdT (the last
  group the grey remainder); q(x) = sum_g sigma_g(x) (phi_g - W B_g), b(x) = sum_g sigma_g(x)
  dB_g/dT over the solver's groups;
* dT = dt q / (rho_cv(x) + dt W b); where dT > T / 4 the root of
  rho_cv (T' - T) = dt (A - W S(T')), A = q + W S(T), S over ALL groups with the cell's
  opacities, by bisection on [0, T + dt A / rho_cv] until the bracket is below 1e-15 relative;
* the owed / paid emission as the header states it: owed grows by dB/dT(T_old) dT (or by
  B(T') - B(T) where the root was solved, dT then 0), the next sweep pays p = max(owed, -B),
  Beff = B + p.

With identical regions this is the uniform coupling, which tests/test_regions_material.py
pins to the C oracle's orc_material_*.  The accessors carry the names
test_material_gpu.compare reads (temperature, psi, ends, moments, cell_planck,
cell_emission, material_transit, g_lo, Gl, G).

dtype (default np.float64: the above, unchanged): another format, np.longdouble for the material
regime sweep's truth (tests/material_regime_cases.py), runs the whole step in it -- T, owed, dB,
Beff, q, b, the update and the root, the sweep as RegionReference's in that dtype -- on the fp64
inputs cast exactly, with the Planck terms from oracle/planck_np.py in that dtype (the fp64 path
keeps the C oracle's calls: planck_np in fp64 agrees with them to 2 ulps of the operands, not
bitwise) and the root bisected, all solving cells at once, until the bracket is at most 4 ulp of
the dtype.  Every update records which cells solved the root, each cell's dT / T and the T it leaves (history).
"""
from __future__ import annotations

import copy

import numpy as np

from regions_reference import RegionReference

NEWTON_FRAC = 0.25


class _CellSets:
    """sets[k] for RegionReference._sweep: the unit LineSet of upwind cell k's region with its
    constant scaled by that cell's emission."""

    def __init__(self, ref, half):
        self.ref, self.half = ref, half

    def __getitem__(self, k):
        ref = self.ref
        x = ref.N - 1 - k if self.half == 0 else k
        base = ref.unit_lines[self.half][ref.cell_region[x]]
        ls = copy.copy(base)
        ls.Sc = base.Sc * ref.Beff[x, ref.idx[self.half][1]]
        return ls


class RegionMaterialReference(RegionReference):
    def __init__(self, oracle_mod, p, regions, rho_cv, T_cells=None, g_lo=0, g_hi=0, dtype=np.float64):
        import fused_np
        assert not (p["use_correction"] and p["V"] != 0.0)
        self.om, self.p = oracle_mod, p
        f = self.dtype = np.dtype(dtype).type
        self.native = f is np.float64  # the C oracle's Planck terms and the scalar root, as before
        M, N = p["M"], p["N"]
        self.M, self.N, self.G = M, N, p["G"]
        self.g_lo, g_hi = g_lo, (g_hi or p["G"])
        self.Gl = g_hi - g_lo
        sl = slice(g_lo, g_hi)
        h = M // 2
        cells = [r["cells"] for r in regions]
        self.cell_region = np.repeat(np.arange(len(regions)), cells)
        assert self.cell_region.size == N and len(rho_cv) == len(regions)
        self.dx = np.array([r["width"] / r["cells"] for r in regions])
        self.dx_cells = self.dx[self.cell_region]
        self.rho_cv_cells = np.asarray(rho_cv, dtype=np.float64)[self.cell_region].astype(f)
        tables = []
        for r in regions:
            pr = dict(p, rho=r["rho"], kappa_grey=r["kappa_grey"], T=r["T"], group_kappa=r["group_kappa"],
                      N=r["cells"], X=r["width"], dx=r["width"] / r["cells"])
            o = oracle_mod.OracleSolver(pr, g_lo=g_lo, g_hi=g_hi)
            g = o.groups()
            self.mu, self.wt = o.quad()
            self.psi_source = o.psi_source()[:, sl]
            self.e_edge = g["e_edge"].copy()
            tables.append(dict(B=g["B"][sl], sigma=r["rho"] * g["kappa"][sl], sigma_all=r["rho"] * g["kappa"]))
        self.tables = tables
        self.sigma_cells = np.stack([tables[r]["sigma"] for r in self.cell_region]).astype(f)          # (N, Gl)
        self.sigma_all_cells = np.stack([tables[r]["sigma_all"] for r in self.cell_region]).astype(f)  # (N, G)
        self.psi_source = np.asarray(self.psi_source, dtype=f)
        self.W = f(float(self.wt.sum()))
        self.idx, self.unit_lines, self.lines, self.E = {}, {}, {}, {}
        zeros = np.zeros(h * self.Gl)
        for half in (0, 1):
            I = np.tile([(h - 1 - ip) if half == 0 else (h + ip) for ip in range(h)], self.Gl)
            Gi = np.repeat(np.arange(self.Gl), h)
            self.idx[half] = (I, Gi)
            self.unit_lines[half] = [fused_np.LineSet(self.mu[I], t["sigma"][Gi], np.ones(h * self.Gl), zeros, zeros,
                                                      zeros, 0.0, dx, p["dt"], p["ts_method"], False, dtype=f)
                                     for t, dx in zip(tables, self.dx)]
            self.lines[half] = _CellSets(self, half)
            reg = self.cell_region[::-1] if half == 0 else self.cell_region
            B_cells = np.stack([tables[r]["B"][Gi] for r in reg], axis=1)  # (lines, N): psi = its region's B_g
            self.E[half] = np.repeat(B_cells[:, :, None], 2, axis=2).astype(f)
        self.nsub = 4 if p["ts_method"] == 3 else 1
        # the material state
        self.T = (np.array([regions[r]["T"] for r in self.cell_region], dtype=np.float64) if T_cells is None
                  else np.array(T_cells, dtype=np.float64)).astype(f)
        self.dTlast = np.zeros(N, dtype=f)
        self.owed = np.zeros((N, self.Gl), dtype=f)
        self.dB = np.zeros((N, self.Gl), dtype=f)
        self.Bcell = np.zeros((N, self.Gl), dtype=f)
        self.Beff = np.zeros((N, self.Gl), dtype=f)
        self.bpart = np.zeros(N, dtype=f)
        self.newton_cells = 0  # cells that solved the full emission, over all updates
        # per update: dict(solved=(N) bool, ratio=(N) dT / T of the linear update, T=(N) after the update)
        self.history = []
        self._planck()

    def _upwind_regions(self, half):
        return np.arange(self.N)  # _sweep's sets[reg[k]]: _CellSets is indexed by the upwind cell

    # ---- Planck terms and the owed emission at the current T ----
    def _planck_terms(self, T, g_lo, g_hi, deriv=False):
        """(cells, g_hi - g_lo) of kcon B_g (deriv: dB_g/dT) at the temperatures T, in self.dtype."""
        if self.native:
            fn = self.om.planck_cell_dBdT if deriv else self.om.planck_cell
            return np.array([[fn(t, self.e_edge, g) for g in range(g_lo, g_hi)] for t in np.atleast_1d(T)])
        import planck_np
        # the cells' T in fp64 decide the branches; T held in a wider dtype enters the arithmetic
        return planck_np.planck_cells(np.atleast_1d(T), self.e_edge, g_lo, g_hi, self.dtype, deriv)

    def _planck(self):
        if not self.native:
            f = self.dtype
            owed = self.owed + self.dB * self.dTlast[:, None]
            B = self._planck_terms(self.T, self.g_lo, self.g_lo + self.Gl)
            dB = self._planck_terms(self.T, self.g_lo, self.g_lo + self.Gl, deriv=True)
            pay = np.where(owed > -B, owed, -B)
            self.Bcell, self.Beff, self.owed, self.dB = B, B + pay, owed - pay, dB
            b = np.zeros(self.N, dtype=f)
            for gl in range(self.Gl):
                b = b + self.sigma_cells[:, gl] * dB[:, gl]
            self.bpart = b
            return
        for c in range(self.N):
            b = 0.0
            for gl in range(self.Gl):
                g = self.g_lo + gl
                owed = self.owed[c, gl] + self.dB[c, gl] * self.dTlast[c]
                B = self.om.planck_cell(self.T[c], self.e_edge, g)
                dB = self.om.planck_cell_dBdT(self.T[c], self.e_edge, g)
                pay = owed if owed > -B else -B
                self.Bcell[c, gl] = B
                self.Beff[c, gl] = B + pay
                self.owed[c, gl] = owed - pay
                self.dB[c, gl] = dB
                b = b + self.sigma_cells[c, gl] * dB
            self.bpart[c] = b

    def _emission_all(self, c, T):
        return float(sum(self.sigma_all_cells[c, g] * self.om.planck_cell(T, self.e_edge, g) for g in range(self.G)))

    def _solve_cell(self, c, q):
        T, dt, W, rc = self.T[c], self.p["dt"], self.W, self.rho_cv_cells[c]
        A = q + W * self._emission_all(c, T)
        hi0 = T + dt * A / rc
        if not hi0 > 0.0:
            return hi0
        lo, hi = 0.0, hi0
        for _ in range(400):
            if hi - lo <= 1e-15 * hi:
                break
            mid = 0.5 * (lo + hi)
            if not lo < mid < hi:
                break
            f = rc * (mid - T) + dt * W * self._emission_all(c, mid) - dt * A
            if f > 0.0:
                hi = mid
            else:
                lo = mid
        return 0.5 * (lo + hi)

    def _solve_cells(self, cells, q):
        """_solve_cell for the cells (indices) at once, in self.dtype: bisection until every
        bracket is at most 4 ulp of the dtype."""
        f = self.dtype
        T, dt, W, rc = self.T[cells], f(self.p["dt"]), self.W, self.rho_cv_cells[cells]
        sig = self.sigma_all_cells[cells]

        def emission(t):
            return (sig * self._planck_terms(t, 0, self.G)).sum(axis=1)

        A = q + W * emission(T)
        hi0 = T + dt * A / rc
        out = hi0.copy()
        live = hi0 > 0
        lo, hi = np.zeros_like(hi0), np.where(live, hi0, f(1))
        tol = 4 * np.finfo(f).eps
        for _ in range(40000):
            mid = f(0.5) * (lo + hi)
            live = live & (hi - lo > tol * hi) & (lo < mid) & (mid < hi)
            if not live.any():
                break
            fm = rc * (mid - T) + dt * W * emission(np.where(live, mid, f(1))) - dt * A
            up = live & (fm > 0)
            hi = np.where(up, mid, hi)
            lo = np.where(live & ~up, mid, lo)
        return np.where(hi0 > 0, f(0.5) * (lo + hi), out)

    # ---- the coupled step ----
    def material_sweep(self):
        """One coupled full step with the emission Beff; returns this solver's [q, b] (2N)."""
        self.step()
        phi = self.moments()[0]  # (Gl, N)
        q = (self.sigma_cells * (phi.T - self.W * self.Bcell)).sum(axis=1)
        return np.concatenate([q, self.bpart])

    def material_update(self, qb):
        N, dt, W = self.N, self.p["dt"], self.W
        if not self.native:
            f = self.dtype
            qb = np.asarray(qb, dtype=f)
            q, b, T = qb[:N], qb[N:], self.T
            dT = f(dt) * q / (self.rho_cv_cells + f(dt) * W * b)
            solve = ~(dT <= f(NEWTON_FRAC) * T)
            with np.errstate(all="ignore"):
                self.history.append(dict(solved=solve.copy(), ratio=np.asarray(dT / T, dtype=np.float64)))
            Tn, dTl = T + dT, dT.copy()
            cells = np.flatnonzero(solve)
            if cells.size:
                Tr = self._solve_cells(cells, q[cells])
                self.owed[cells] += self._planck_terms(Tr, self.g_lo, self.g_lo + self.Gl) - self.Bcell[cells]
                Tn[cells], dTl[cells] = Tr, 0
                self.newton_cells += int(cells.size)
            self.T, self.dTlast = Tn, dTl
            self.history[-1]["T"] = np.asarray(Tn, dtype=np.float64)
            self._planck()
            return
        solved, ratio = np.zeros(N, dtype=bool), np.zeros(N)
        self.history.append(dict(solved=solved, ratio=ratio))
        for c in range(N):
            q, b, T = qb[c], qb[N + c], self.T[c]
            dT = dt * q / (self.rho_cv_cells[c] + dt * W * b)
            ratio[c] = dT / T if T != 0 else np.copysign(np.inf, dT)
            solved[c] = not dT <= NEWTON_FRAC * T
            if dT <= NEWTON_FRAC * T:
                self.T[c] = T + dT
                self.dTlast[c] = dT
            else:
                Tn = self._solve_cell(c, q)
                for gl in range(self.Gl):
                    self.owed[c, gl] += self.om.planck_cell(Tn, self.e_edge, self.g_lo + gl) - self.Bcell[c, gl]
                self.T[c] = Tn
                self.dTlast[c] = 0.0
                self.newton_cells += 1
        self.history[-1]["T"] = self.T.copy()
        self._planck()

    def material_step(self, n=1):
        for _ in range(n):
            self.material_update(self.material_sweep())

    # ---- read-outs (test_material_gpu.compare's names) ----
    def ends(self):
        out = np.empty((self.M, self.Gl, self.N, 2), dtype=self.dtype)
        for half in (0, 1):
            I, Gi = self.idx[half]
            E = self.E[half]
            if half == 0:
                out[I, Gi, :, 1] = E[:, ::-1, 0]
                out[I, Gi, :, 0] = E[:, ::-1, 1]
            else:
                out[I, Gi, :, 0] = E[:, :, 0]
                out[I, Gi, :, 1] = E[:, :, 1]
        return out

    def psi(self):
        e = self.ends()
        return self.dtype(0.5) * (e[..., 0] + e[..., 1])

    def moments(self):
        psi = self.psi()
        wt = np.asarray(self.wt, dtype=self.dtype)
        mw = np.asarray(self.mu, dtype=self.dtype) * wt
        return (np.einsum("i,igc->gc", wt, psi), np.einsum("i,igc->gc", mw, psi),
                np.einsum("i,igc->gc", wt[self.mu > 0], psi[self.mu > 0]))

    def quad(self):
        return self.mu, self.wt

    def temperature(self):
        return self.T.copy()

    def cell_planck(self):
        return self.Bcell.T.copy()

    def cell_emission(self):
        return self.Beff.T.copy()

    def material_transit(self):
        return self.dtype(self.p["dt"]) * self.W * (self.sigma_cells * ((self.Beff - self.Bcell) + self.owed)).sum(axis=1)


def region_energy(s, dx_cells, rho_cv_cells, c_light):
    """sum_x dx(x) (sum_g phi_g / c + rho_cv(x) T + transit) of a solver or the reference."""
    phi = s.moments()[0]
    return float((dx_cells * (phi.sum(axis=0) / c_light + rho_cv_cells * s.temperature() + s.material_transit())).sum())


def plan_rule(cells, reflective, max_waves, nsteps, tick_vacuum, tick_reflective):
    """rt_regions_plan_steps' rule restated: C of 1, 2, 4, 8 is admissible when it divides every
    region's first cell and N; among those whose chain fits max_waves waves, the least
    (nsteps + lanes - 1) x tick cost, the smaller C on a tie.  (C, waves, lanes per line)."""
    edges = np.concatenate([[0], np.cumsum(cells)])
    N, best = int(edges[-1]), None
    for ci, C in enumerate((1, 2, 4, 8)):
        if (edges % C).any():
            continue
        used = N // C * (2 if reflective else 1)
        w = -(-used // 64)
        if w > max_waves:
            continue
        cost = (float(nsteps) + used - 1) * (tick_reflective if reflective else tick_vacuum)[ci][w - 1]
        if best is None or cost < best[0]:
            best = (cost, C, w, N // C)
    return best[1:] if best else (0, 0, 0)
