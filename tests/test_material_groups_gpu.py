"""Material-temperature coupling on the GPU at 31-128 groups per handle against the oracle
(closes VERDICT.md weakness #3, "next round" item 1: the benchmark's `material` legs run 128
groups per handle, the earlier GPU tests of the coupled step at most 16).

What runs here that no earlier test compared with orc_material_*: planck_cells_kernel past its
first 32-group tile (owed / dB / pay and the bpart sum over waves in the later chunks);
material_q_kernel and material_transit_kernel on the second lap of their group loop;
phi_correction_geo_kernel (BE, CN) and phi_correction_rows_kernel (BDF2) on more than one block
of 8 groups; phi_correction_geo_kernel's second 2048-cell range (the rows kernel's range is 8192
cells: its second range needs N > 16384 at 64 line groups and is still run by no test); the
fused angular sums of sweep_block_kernel<S,1,0,true> when H x Gl is no multiple of 64;
material_update_kernel's serial S(T) over 128 groups on a full handle and on shards; the REG
forms of the Planck, q and transit kernels at 72 groups.

Part A (tests/material_group_cases.py, grid 0.1..10 keV): test_material_gpu.compare unchanged,
T 1e-12 and the fields 1e-10.  Part B, the benchmark's own grid 1e-3..30 keV, 128 groups:
compare(..., field_floor=True) -- the grey remainder group holds ~1e-9 of a c T^4 there and one
ulp of T moves it by 4e-8 of itself, so its fields are measured against
planck_rel's floor for it; every other group stays measured against its own maximum.  Each case
asserts the premise that makes it run the path it names (segments from sweep_geometry, the
Newton cells from the oracle's first linear dT).  tests/test_material_groups.py holds the two
CPU evaluations of every case to a quarter of these tolerances.
"""
from __future__ import annotations

import json

import numpy as np
import pytest

import material_group_cases as mc
from parity import per_group_rel
from test_material import net_outflow, total_energy
from test_material_gpu import GpuView, compare, to_rt

pytestmark = pytest.mark.gpu


def run_device(rtsn_mod, c, p, rho_cv, T0, walk=False):
    """The case's shard handles after its steps, coupled through the summed [q, b] on the device."""
    import torch
    q = to_rt(p)
    shards = [rtsn_mod.Solver(q, g_lo=lo, g_hi=hi) for lo, hi in c["shards"]]
    for s in shards:
        if c["wgs"]:
            s.set_segmentation(c["wgs"])
        if walk:
            s.set_phi_correction_form(1)
        s.material_enable(rho_cv, T0)
    if len(shards) == 1:
        for _ in range(c["steps"]):
            shards[0].material_sweep()
            shards[0].material_update()
        return shards
    qb = [torch.zeros(2 * p["N"], dtype=torch.float64, device="cuda") for _ in shards]
    for _ in range(c["steps"]):
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
    return shards


def check_segments(s, c):
    """The case's premise on the coupled pass's segments (rt_sweep_geometry after the enable)."""
    sg = s.sweep_geometry()[1]
    if c["seg"] == "multi3":
        assert sg >= 3, sg  # the correction is pending: the closed-form kernels run
    elif c["seg"] == "multi":
        assert sg >= 2, sg
    elif c["seg"] == "one":
        assert sg == 1, sg  # no correction: the pass's own sums alone
    elif c["seg"] == "long":
        # Ls is a multiple of 16; the closed forms correct segments 1..: the last one's real length
        ls = 16 * -(-(-(-c["N"] // sg)) // 16)
        assert sg >= 2 and -(-c["N"] // ls) == sg and c["N"] - (sg - 1) * ls > 2048, (sg, ls, c["N"])
    return sg


@pytest.mark.parametrize("c", mc.CASES, ids=[c["id"] for c in mc.CASES])
def test_case_matches_oracle(rtsn_mod, oracle_mod, c):
    p, rho_cv, T0 = mc.build(oracle_mod, c)
    orcs = mc.oracle_run(oracle_mod, c)
    mc.check_start_premise(oracle_mod, c)  # (from the run's first update)
    devs = run_device(rtsn_mod, c, p, rho_cv, T0)
    try:
        segs = [check_segments(s, c) for s in devs]
        for s, o in zip(devs, orcs):
            err = compare(s, o, field_floor=c["floor"])
            print("MG_ERR", c["part"], c["id"], json.dumps(err))
        if c["floor"]:
            mc.check_floor_conditions(orcs)
        T_dev, phi_dev = devs[0].temperature(), devs[0].moments()[0]
        if len(devs) > 1:
            # both are within compare's 1e-12 of the oracle's T; the group sum's order differs
            one = dict(c, shards=((0, 0),))
            full = run_device(rtsn_mod, one, p, rho_cv, T0)[0]
            with full:
                for s in devs:
                    np.testing.assert_allclose(s.temperature(), full.temperature(), rtol=1e-12)
        if c["walk"]:  # the closed forms against the cell-by-cell walk (test_be_correction_closed_form's bounds)
            walk = run_device(rtsn_mod, c, p, rho_cv, T0, walk=True)[0]
            with walk:
                assert walk.sweep_geometry()[1] == segs[0]
                np.testing.assert_allclose(T_dev, walk.temperature(), rtol=1e-13)
                assert per_group_rel(phi_dev, walk.moments()[0], 0) <= 1e-12
        if c["energy"]:  # the device's energy balance of one more BE step (test_stiff_coupling_matches_oracle's)
            gpu = devs[0]
            T = gpu.temperature()
            assert np.isfinite(T).all() and (T > 0).all() and (gpu.cell_emission() >= 0).all()
            e0 = total_energy(gpu, p, rho_cv)
            gpu.material_step(1)
            resid = (total_energy(gpu, p, rho_cv) - e0) + p["dt"] * net_outflow(GpuView(gpu), p)
            print("MG_ENERGY", c["id"], resid / e0)
            assert abs(resid) <= 1e-12 * abs(e0), (resid, e0)
    finally:
        for s in devs:
            s.close()


@pytest.mark.parametrize("c", mc.QB_CASES, ids=[c["id"] for c in mc.QB_CASES])
def test_exchange_terms_match_oracle(rtsn_mod, oracle_mod, c):
    """[q, b] of the first coupled sweep read from the device: b (a sum of non-negative terms) to
    1e-12 relative; q cancels near equilibrium, so |dq(x)| <= 1e-10 sum_g sigma_g (max_x phi_g +
    W max_x B_g) -- what compare's field tolerances imply for it and nothing tighter."""
    import torch
    p, rho_cv, T0 = mc.build(oracle_mod, c)
    N = p["N"]
    orc = mc.make_oracle(oracle_mod, p, rho_cv, T0, 0, 0)
    want = orc.material_sweep()
    with rtsn_mod.Solver(to_rt(p)) as s:
        s.set_segmentation(c["wgs"])
        s.material_enable(rho_cv, T0)
        check_segments(s, c)
        q = torch.zeros(2 * N, dtype=torch.float64, device="cuda")
        s.material_sweep(q)
        s.synchronize()
        got = q.cpu().numpy()
    err_b = float(np.max(np.abs(got[N:] - want[N:]) / want[N:]))
    bound = mc.q_bound(orc)
    err_q = float(np.max(np.abs(got[:N] - want[:N])) / bound)
    print("MG_QB", c["id"], json.dumps({"b": err_b, "q_over_bound_scale": err_q}))
    assert (want[N:] > 0).all() and err_b <= 1e-12, err_b
    assert err_q <= 1e-10, err_q


@pytest.mark.parametrize("ts,bc_left", mc.REGION_CASES)
def test_region_handle_matches_reference(rtsn_mod, oracle_mod, ts, bc_left):
    """One coupled region handle at 72 groups (the REG forms' second lap over the groups, three
    Planck tiles) against the numpy reference: each region its own opacity table (x1, x30, x0.1),
    heat capacity and cell width."""
    from regions_material_ref import RegionMaterialReference
    p, regions, rho_cv, T0 = mc.region_case(oracle_mod, ts, bc_left)
    ref = RegionMaterialReference(oracle_mod, p, regions, rho_cv, T0)
    ref.material_step(3)
    assert np.isfinite(ref.ends()).all() and (ref.temperature() > 0).all()
    with rtsn_mod.Solver(to_rt(p), regions=regions) as s:
        s.material_enable_regions(rho_cv, T0)
        assert s.wavefront_state()["active"] and s.G == mc.REGION_G > 64
        for _ in range(3):
            s.material_sweep()
            s.material_update()
        print("MG_ERR", "A7", f"regions-ts{ts}-bc{bc_left}", json.dumps(compare(s, ref)))
