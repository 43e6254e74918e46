"""Region handles on the GPU on seeded random configurations, every region with its own opacity.

test_regions_gpu.py and test_regions_material_gpu.py run a fixed grid whose regions share one
opacity table (only rho tells the media apart), on two boundary pairs, one M, one group window
and 5 coupled groups.  Here:

* test_random_region_configuration -- tests/regions_cases.region_case draws the layout, each
  region's dx, rho, T and opacity (its own table, the shared table, or its own kappa_grey), M,
  the group window, scheme, boundary pair, correction, dt, run length, psi_source and the
  schedule (forced cells per lane, a wave cap, a random initial state, chunked advances) at
  once.  The plan against the plan rule, rt_get_region_data against the reference's tables, and
  after every chunk psi, ends, phi, phi_plus (1e-10 per group), F and the group ends against
  test_regions_gpu.RegionReference (compare_region_handle); the balance partials and the group
  absorption against numpy sums over the REFERENCE's ends and phi, to 1e-10 of the summed
  magnitudes (test_gpu_parity.compare_all's scaling);
* test_random_region_material_configuration -- regions_cases.region_material_case: the coupled
  handle against tests/regions_material_ref.RegionMaterialReference through
  test_material_gpu.compare (T 1e-12, fields 1e-10), the initial emission per group (the
  remainder group by compare's own metric), and for backward Euler the per-step energy
  residual on the device;
* test_same_medium_three_ways_bitwise -- one medium written as (kappa_g, rho), (2 kappa_g,
  rho / 2) and (None, kappa_grey): the same sigma bits reach the arithmetic, so every read-out
  is array_equal to the plain handle's; only the table plumbing can break that;
* test_region_opacity_arrays_outlive_their_caller -- the handle owns its regions' opacities;
* test_coupled_regions_past_one_group_tile -- the region forms of planck_cells_kernel (tiles of
  32 groups) and of the q and transit kernels (lanes over groups, 64 a round) at 40 and 70
  groups, against the reference (pinned to the oracle at these sizes by
  tests/test_regions_cases.py), and two group shards against the full handle.

The references' per-region tables are pinned to the C oracle by tests/test_regions_cases.py,
which also asserts that the seeds run here reach every kernel form.
"""
from __future__ import annotations

import gc

import numpy as np
import pytest

import regions_cases as rc
from parity import per_group_rel
from regions_material_ref import RegionMaterialReference, region_energy
from test_material import C_LIGHT, net_outflow, t_profile
from test_material_gpu import GpuView, compare, planck_rel, to_rt
from test_regions_gpu import C_LIGHT as C_LIGHT_BALANCE
from test_regions_gpu import RegionReference, _readouts, compare_region_handle, region_plan
from test_regions_material_gpu import _coupled_readouts, coupled_steps, one_step_plan

pytestmark = pytest.mark.gpu

SUM_TOL = 1e-10  # of the summed magnitudes: the arguments are the reference's, not the GPU's own phi


def compare_region_sums(s, ref, regions):
    """rt_get_balance_partials' three terms and rt_group_absorption_device against numpy sums
    over the reference's ends and phi (test_regions_gpu.test_balance_and_absorption's
    expressions, and the inflow currents of rt_get_balance_terms)."""
    import torch
    mu, wt = ref.mu, ref.wt
    ends = ref.ends()
    phi = np.einsum("i,igc->gc", wt, 0.5 * (ends[..., 0] + ends[..., 1]))
    creg = ref.cell_region
    sigma = np.stack([ref.tables[k]["sigma"] for k in creg], axis=1)  # (Gl, N)
    dx = ref.dx[creg]
    Tc = np.array([regions[k]["T"] for k in creg])
    w = (mu * wt)[:, None]
    jout = np.concatenate([-(ends[mu < 0, :, 0, 0] * w[mu < 0]), ends[mu > 0, :, -1, 1] * w[mu > 0]])
    jin = np.concatenate([-(ends[mu < 0, :, -1, 0] * w[mu < 0]), ends[mu > 0, :, 0, 1] * w[mu > 0]])
    ab = sigma * phi * dx
    em = sigma * (1.3653104e-2 * C_LIGHT_BALANCE) * Tc ** 4 * dx
    inflow, out_abs, emission = s.balance_partials()
    a_dev = torch.empty(ref.N, dtype=torch.float64, device="cuda")
    s.group_absorption(a_dev)
    s.synchronize()
    a_dev = a_dev.cpu().numpy()

    def rel(got, want, scale):
        return float(np.max(np.abs(got - want) / np.maximum(scale, 1e-300)))

    err = {"inflow": rel(inflow, jin.sum(axis=0), np.abs(jin).sum(axis=0)),
           "outflow_absorption": rel(out_abs, jout.sum(axis=0) + ab.sum(axis=1),
                                     np.abs(jout).sum(axis=0) + np.abs(ab).sum(axis=1)),
           "emission": rel(emission, em.sum(axis=1), np.abs(em).sum(axis=1)),
           "absorption_device": rel(a_dev, (sigma * phi).sum(axis=0), np.abs(sigma * phi).sum(axis=0))}
    print(err)
    for k, v in err.items():
        assert v <= SUM_TOL, (k, v, err)


@pytest.mark.parametrize("seed", rc.REGION_SEEDS)
def test_random_region_configuration(rtsn_mod, oracle_mod, seed):
    c = rc.region_case(seed)
    p, regions, cells, g_lo, g_hi = c["p"], c["regions"], c["cells"], c["g_lo"], c["g_hi"]
    ref = RegionReference(oracle_mod, p, regions, g_lo=g_lo, g_hi=g_hi)
    with rtsn_mod.Solver(to_rt(p), g_lo=g_lo, g_hi=g_hi, regions=regions) as s:
        if c["wave_cap"]:
            s.wavefront_waves = c["wave_cap"]
        if c["want"]:
            s.set_wavefront_cells(c["want"])
        st = s.wavefront_state()
        plan = region_plan(cells, p["bc_left"] == 2, c["wave_cap"] or 8, c["want"])
        print(seed, {k: p[k] for k in ("N", "M", "ts_method", "bc_left", "bc_right", "V")}, cells, c["kinds"], st)
        assert st["active"] and st["mode"] == 2 and (st["cells_per_lane"], st["waves"]) == plan
        assert s.regions() == [0] + [int(e) for e in np.cumsum(cells)]
        for k, t in enumerate(ref.tables):
            d = s.region_data(k)
            assert np.array_equal(d["kappa"][g_lo:g_hi], t["kappa"]), k
            assert per_group_rel(d["B"][g_lo:g_hi], t["B"], 0) <= 1e-13, k
            assert d["dx"] == regions[k]["width"] / cells[k]
        if c["ends_factor"] is not None:  # B of the cell's region x U(0.5, 1.5)
            B_cells = np.stack([ref.tables[k]["B"] for k in ref.cell_region], axis=1)  # (Gl, N)
            ends0 = B_cells[None, :, :, None] * c["ends_factor"]
            s.set_ends(ends0)
            ref.set_ends(ends0)
        for n in c["chunks"] or [None]:
            if n is None:
                s.solve()
                n = c["steps"]
            else:
                s.advance(n)
            for _ in range(n):
                ref.step()
            assert np.isfinite(ref.ends()).all()
            compare_region_handle(s, ref)
            compare_region_sums(s, ref, regions)


@pytest.mark.parametrize("seed", rc.MATERIAL_SEEDS)
def test_random_region_material_configuration(rtsn_mod, oracle_mod, seed):
    c = rc.region_material_case(seed)
    p, regions, cells, rho_cv, (g_lo, g_hi) = c["p"], c["regions"], c["cells"], c["rho_cv"], c["shard"]
    ref = RegionMaterialReference(oracle_mod, p, regions, rho_cv, c["T_cells"], g_lo, g_hi)
    creg = ref.cell_region
    dx, rcv = ref.dx[creg], np.asarray(rho_cv)[creg]
    energy = p["ts_method"] == 1 and (g_lo, g_hi) == (0, 0)
    with rtsn_mod.Solver(to_rt(p), g_lo=g_lo, g_hi=g_hi, regions=regions) as s:
        s.set_wavefront_cells(c["want"])
        s.material_enable_regions(rho_cv, c["T_cells"])
        st = s.wavefront_state()
        print(seed, {k: p[k] for k in ("N", "M", "G", "ts_method", "bc_left", "bc_right")}, cells, c["kinds"],
              c["profile"], (g_lo, g_hi), st)
        assert st["active"] and st["cells_per_lane"] == c["want"]
        assert (st["cells_per_lane"], st["waves"]) == one_step_plan(cells, p["bc_left"] == 2, c["want"])
        # the initial emission at 1e-10 per group -- but the remainder group (the last: a c T^4
        # minus the integral over the others, which cancels where it is a small share: seed 12's
        # shard holds it alone at 2e-9 of a c T^4) by compare's metric for B and Beff
        em_g, em_r = s.cell_emission(), ref.cell_emission()
        last = ref.g_lo + ref.Gl == ref.G
        e_em = {"groups": per_group_rel(em_g[:ref.Gl - last], em_r[:ref.Gl - last], 0) if ref.Gl > last else 0.0,
                "remainder": planck_rel(em_g, em_r, ref.temperature(), last)}
        print("emission", e_em)
        assert max(e_em.values()) <= 1e-10
        for n in range(c["steps"]):
            e0 = region_energy(s, dx, rcv, C_LIGHT) if energy else 0.0
            coupled_steps(s, 1)  # a shard on its own [q, b], as the reference's
            ref.material_step(1)
            if energy:  # test_regions_material_gpu.test_backward_euler_energy_on_device's residual
                e1 = region_energy(s, dx, rcv, C_LIGHT)
                resid = (e1 - e0) + p["dt"] * net_outflow(GpuView(s), p)
                print("energy", n, resid / e1, ref.newton_cells)
                assert abs(resid) <= (1e-11 if ref.newton_cells > 0 else 1e-12) * abs(e1), (n, resid, e1)
        T = ref.temperature()
        assert np.isfinite(T).all() and (T > 0).all() and np.isfinite(ref.ends()).all()
        print(compare(s, ref))


# ---------------------------------------------------------------------------
# one medium written three ways
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("bc", [(0, 0), (2, 1)])
def test_same_medium_three_ways_bitwise(rtsn_mod, oracle_mod, bc):
    lo, hi = 40, 50
    p, regions = rc.three_ways(3, bc)
    q = to_rt(p)
    B = oracle_mod.OracleSolver(p, g_lo=lo, g_hi=hi).groups()["B"][lo:hi]
    ends0 = B[None, :, None, None] * np.random.default_rng(11 + bc[0]).uniform(0.5, 1.5, size=(6, hi - lo, p["N"], 2))
    with rtsn_mod.Solver(q, g_lo=lo, g_hi=hi) as s:
        s.wavefront = 2
        s.set_ends(ends0)
        s.advance(7)
        plain = _readouts(s)
    with rtsn_mod.Solver(q, g_lo=lo, g_hi=hi, regions=regions) as s:
        assert s.wavefront_state()["active"]
        for k in range(3):
            assert np.array_equal(regions[k]["rho"] * s.region_data(k)["kappa"], p["rho"] * p["group_kappa"])
        s.set_ends(ends0)
        s.advance(7)
        got = _readouts(s)
    assert not np.array_equal(plain["ends"], ends0)
    for k, v in plain.items():
        assert np.array_equal(got[k], v), k
    # coupled: against the slab of three regions all written the first way
    p, regions = rc.three_ways_material(3, bc, 1e-4)
    same = [dict(regions[0], cells=r["cells"], width=r["width"]) for r in regions]
    T0 = t_profile(p["N"])
    out = []
    for regs in (same, regions):
        with rtsn_mod.Solver(to_rt(p), regions=regs) as s:
            s.material_enable_regions([5.0] * 3, T0)
            coupled_steps(s, 6)
            out.append(_coupled_readouts(s))
    assert not np.array_equal(out[0]["T"], T0)
    for k, v in out[0].items():
        assert np.array_equal(out[1][k], v), k


# ---------------------------------------------------------------------------
# the handle owns its regions' opacities
# ---------------------------------------------------------------------------
def _own_tables(seed):
    """Three regions with their own opacity arrays (fresh arrays on every call)."""
    p = rc.llnl_params()
    rng = np.random.default_rng(seed)
    cells, dxs, rho = (20, 10, 20), (0.004, 0.016, 0.008), (1.0, 10.0, 0.2)
    p.update(N=50, M=6, ts_method=3, bc_left=2, bc_right=1, use_correction=1, V=5.994, dt=1e-6)
    p["psi_source"] = np.linspace(0.5, 2.0, 6 * p["G"]).reshape(6, p["G"])
    regions = [dict(cells=c, width=c * d, rho=r, kappa_grey=1.0, T=1.0,
                    group_kappa=p["group_kappa"] * 10.0 ** rng.uniform(-1, 1, size=p["G"]))
               for c, d, r in zip(cells, dxs, rho)]
    return to_rt(p), regions


def _handle_from_temporaries(rtsn_mod, seed):
    q, regions = _own_tables(seed)
    return rtsn_mod.Solver(q, g_lo=40, g_hi=50, regions=regions)  # the arrays die with this frame


def test_region_opacity_arrays_outlive_their_caller(rtsn_mod):
    q, regions = _own_tables(5)
    with rtsn_mod.Solver(q, g_lo=40, g_hi=50, regions=regions) as s:
        s.advance(5)
        held = _readouts(s)
        kappa = [s.region_data(k)["kappa"] for k in range(3)]
    s = _handle_from_temporaries(rtsn_mod, 5)
    gc.collect()
    junk = [np.full(q["G"], float("nan")) for _ in range(16)]  # the freed arrays' size, overwritten
    for a in junk:
        a[:] = -1.0
    with s:
        for k in range(3):
            assert np.array_equal(s.region_data(k)["kappa"], kappa[k])
            assert np.array_equal(kappa[k], regions[k]["group_kappa"])
        s.advance(5)
        got = _readouts(s)
    assert np.isfinite(held["ends"]).all()
    for k, v in held.items():
        assert np.array_equal(got[k], v), k


# ---------------------------------------------------------------------------
# the coupled region kernels past one tile of 32 groups and one round of 64 lanes
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("Gl", [40, 70])
def test_coupled_regions_past_one_group_tile(rtsn_mod, oracle_mod, Gl):
    """Two regions (rho x50, one grey, one with its own table, rho_cv x10, dx x4), N = 64,
    reflective left, a cold block of 8 cells on the full-emission path; BE and BDF2, 3 steps,
    against RegionMaterialReference; then groups [0, 33) and [33, Gl) as two handles coupled
    through their summed [q, b] against the full handle (1e-12).  Gl = 40 reaches the second
    32-group tile of planck_cells_kernel<true>, Gl = 70 also the second lane round of
    material_q_kernel<true> and material_transit_kernel<true>."""
    import torch
    for ts in (1, 3):
        p, regions, rho_cv, T0 = rc.tile_case(Gl, ts)
        q = to_rt(p)
        ref = RegionMaterialReference(oracle_mod, p, regions, rho_cv, T0)
        with rtsn_mod.Solver(q, regions=regions) as full:
            full.material_enable_regions(rho_cv, T0)
            assert full.G == Gl and full.wavefront_state()["active"]
            assert per_group_rel(full.cell_emission(), ref.cell_emission(), 0) <= 1e-10
            coupled_steps(full, 3)
            ref.material_step(3)
            assert ref.newton_cells > 0 and (ref.temperature() > 0).all() and np.isfinite(ref.ends()).all()
            print(Gl, ts, compare(full, ref))
            T_full, psi_full, transit_full = full.temperature(), full.psi(), full.material_transit()
        shards = [rtsn_mod.Solver(q, g_lo=lo, g_hi=hi, regions=regions) for lo, hi in ((0, 33), (33, Gl))]
        qb = [torch.zeros(2 * p["N"], dtype=torch.float64, device="cuda") for _ in shards]
        for s in shards:
            s.material_enable_regions(rho_cv, T0)
        for _ in range(3):
            for s, x in zip(shards, qb):
                s.material_sweep(x)
            for s in shards:
                s.synchronize()
            tot = qb[0] + qb[1]
            torch.cuda.synchronize()
            for s in shards:
                s.material_update(tot)
            for s in shards:
                s.synchronize()
        for s in shards:
            np.testing.assert_allclose(s.temperature(), T_full, rtol=1e-12)
        psi = np.concatenate([s.psi() for s in shards], axis=1)
        transit = shards[0].material_transit() + shards[1].material_transit()
        e_psi = per_group_rel(psi, psi_full, 1)
        e_tr = float(np.abs(transit - transit_full).max() / max(np.abs(transit_full).max(), 1e-300))
        print(Gl, ts, "shards", e_psi, e_tr)
        for s in shards:
            s.close()
        assert e_psi <= 1e-12 and e_tr <= 1e-10
