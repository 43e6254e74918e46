"""The numpy reference of multi-region slabs (tests/test_regions_gpu.py, the regime sweep's
region cases, tests/regions_material_ref.py): oracle/fused_np.py with a LineSet per region.
A plain module: no GPU import, usable from CPU tests."""
import numpy as np

LO, HI = 40, 50  # the handle's groups of llnl_slab_test's 124 (tests/test_regions_gpu.py)


class RegionReference:
    """oracle/fused_np.py's FusedSolver with a LineSet per region: sweep_step's loop with the
    cell's own LineSet, mirrored for the mu < 0 half (upwind cell k is physical cell N-1-k).
    dtype np.longdouble: the C oracle's fp64 tables (mu, B, kappa, cor1..3, psi_source) and
    the parameters are cast exactly and every operation runs in extended precision."""

    dtype = np.float64  # (a subclass with a constructor of its own: regions_material_ref.py)

    def __init__(self, oracle_mod, p, regions, g_lo=LO, g_hi=HI, dtype=np.float64):
        import fused_np
        self.fn = fused_np
        self.p = p
        f = self.dtype = np.dtype(dtype).type
        M, N = p["M"], p["N"]
        self.M, self.N, self.G = M, N, g_hi - g_lo
        sl = slice(g_lo, g_hi)
        h = M // 2
        self.cell_region = np.repeat(np.arange(len(regions)), [r["cells"] for r in regions])
        assert self.cell_region.size == N
        self.dx = np.array([r["width"] / r["cells"] for r in regions])
        self.mu = self.wt = None
        self.tables = []
        for r in regions:
            pr = dict(p, rho=r["rho"], kappa_grey=r["kappa_grey"], T=r["T"], group_kappa=r["group_kappa"],
                      have_group_kappa=int(r["group_kappa"] is not None),  # None: the region's kappa_grey
                      N=r["cells"], X=r["width"], dx=r["width"] / r["cells"])
            o = oracle_mod.OracleSolver(pr, g_lo=g_lo, g_hi=g_hi)
            g, c = o.groups(), o.correction_coeffs()
            self.mu, self.wt = o.quad()
            # the solver-owned table (zero unless a boundary is "source"); no medium enters it
            self.psi_source = o.psi_source()[:, sl]
            self.tables.append(dict(B=g["B"][sl], kappa=g["kappa"][sl],
                                    sigma=f(r["rho"]) * np.asarray(g["kappa"][sl], dtype=f),
                                    dBdT=g["dBdT"][sl], de_ave=g["de_ave"][sl],
                                    cor=[c[k][sl] for k in ("cor1", "cor2", "cor3")]))
        self.idx, self.lines, self.E = {}, {}, {}
        for half in (0, 1):
            I = np.tile([(h - 1 - ip) if half == 0 else (h + ip) for ip in range(h)], self.G)
            Gi = np.repeat(np.arange(self.G), h)
            self.idx[half] = (I, Gi)
            self.lines[half] = [fused_np.LineSet(self.mu[I], t["sigma"][Gi], t["B"][Gi], t["cor"][0][Gi],
                                                 t["cor"][1][Gi], t["cor"][2][Gi], p["V"], dx, p["dt"],
                                                 p["ts_method"], bool(p["use_correction"]), dtype=f)
                                for t, dx in zip(self.tables, self.dx)]
            B_cells = np.stack([self.tables[r]["B"][Gi] for r in self._upwind_regions(half)], axis=1)  # (lines, N)
            self.E[half] = np.repeat(B_cells[:, :, None], 2, axis=2).astype(f)
        self.psi_source = np.asarray(self.psi_source, dtype=f)
        self.nsub = 4 if p["ts_method"] == 3 else 1

    def _upwind_regions(self, half):
        return self.cell_region[::-1] if half == 0 else self.cell_region

    def set_ends(self, ends):
        ends = np.asarray(ends, dtype=self.dtype)
        for half in (0, 1):
            I, Gi = self.idx[half]
            if half == 0:
                self.E[0][:, :, 0] = ends[I, Gi, ::-1, 1]
                self.E[0][:, :, 1] = ends[I, Gi, ::-1, 0]
            else:
                self.E[1][:, :, 0] = ends[I, Gi, :, 0]
                self.E[1][:, :, 1] = ends[I, Gi, :, 1]

    def _sweep(self, half, bdry):
        """fused_np.sweep_step with ls = the cell's own LineSet."""
        E, sets, reg, neg = self.E[half], self.lines[half], self._upwind_regions(half), half == 0
        ts, N = self.p["ts_method"], self.N
        bdry = np.asarray(bdry, dtype=self.dtype)
        if ts == 1:
            x = bdry[0].copy()
            for k in range(N):
                ls = sets[reg[k]]
                e_in, e_out = ls.be_cell(E[:, k, 0], E[:, k, 1], x)
                E[:, k, 0], E[:, k, 1] = e_in, e_out
                x = e_out
            return x[None]
        if ts == 2:
            xh, pup = bdry[0].copy(), bdry[0].copy()
            for k in range(N):
                ls = sets[reg[k]]
                p_out = E[:, k, 1].copy()
                e_in, e_out = ls.cn_cell(E[:, k, 0], E[:, k, 1], pup, xh)
                E[:, k, 0], E[:, k, 1] = e_in, e_out
                xh, pup = e_out, p_out
            return xh[None]
        x0, xh, x2, x3 = (bdry[k].copy() for k in range(4))
        pup = None
        for k in range(N):
            ls = sets[reg[k]]
            p_in, p_out = E[:, k, 0].copy(), E[:, k, 1].copy()
            if k == 0:
                xp1, xp3, hup = bdry[1], bdry[3], bdry[3]
            else:
                xp1 = xp3 = pup
                hup = xh if neg else x0
            e1 = ls.be_cell(p_in, p_out, x0)
            e2 = ls.cn_cell(e1[0], e1[1], xp1, xh)
            h = e2 if neg else e1
            e3 = ls.be_cell(e2[0], e2[1], x2)
            e4 = ls.bdf_cell(e3[0], e3[1], h[0], h[1], p_in, p_out, x3, hup, xp3)
            E[:, k, 0], E[:, k, 1] = e4
            x0, xh, x2, x3, pup = e1[1], e2[1], e3[1], e4[1], p_out
        return np.stack([x0, xh, x2, x3])

    def step(self):
        p, nsub = self.p, self.nsub
        I, Gi = self.idx[0]
        b = self.psi_source[I, Gi] if p["bc_right"] == 1 else np.zeros(len(I), dtype=self.dtype)
        out_neg = self._sweep(0, np.repeat(b[None], nsub, axis=0))
        I, Gi = self.idx[1]
        bd = out_neg if p["bc_left"] == 2 else np.repeat(self.psi_source[I, Gi][None], nsub, axis=0)
        self._sweep(1, bd)

    def ends(self):
        out = np.empty((self.M, self.G, self.N, 2), dtype=self.dtype)
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
