"""Regime sweep of the material-temperature coupling on the device against an
extended-precision truth (tests/material_regime_cases.py: the cases, the truth, the metric;
tests/test_material_regime_ref.py checks the truth and the conditions on the CPU).

planck_cells_kernel (B through rt_get_cell_planck, dB/dT through one-group shards whose b is
sigma_g dB_g/dT with sigma_g = 1), material_update_kernel alone on a caller-built [q, b], and
six coupled steps of the uniform pass, the region chain and the one-launch walk, each under

    E(gpu) <= 32 max(E(fp64 reference), 16 eps)

per group and cell set (T per cell, ends per line), the reference's error floored at
16 eps a c T^4 where the group's value ends in a subtraction at that scale.  Every test prints
its largest ratio.
"""
import numpy as np
import pytest

import material_regime_cases as mc
import regime_cases as rc

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not rc.HAVE_EXTENDED, reason=rc.SKIP_REASON)]


# ---------------------------------------------------------------------------
# planck_cells_kernel
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("handle", mc.PLANCK_HANDLES, ids=[f"{n}-{lo}-{hi}" for n, lo, hi in mc.PLANCK_HANDLES])
def test_planck_B(rtsn_mod, oracle_mod, handle):
    """B_g(T(x)) of every group of the handle, per decade of T; exactly 0 at T <= 0."""
    name, g_lo, g_hi = handle
    t = mc.planck_truth(oracle_mod, name, False)
    with rtsn_mod.Solver(rc.to_rt(mc.planck_params(oracle_mod, name)), g_lo=g_lo, g_hi=g_hi) as s:
        assert np.array_equal(s.groups()["e_edge"], t.edges)  # the truth's inputs are the handle's
        s.material_enable(1.0, t.T)
        B = s.cell_planck().T
    sl = slice(g_lo, g_hi or t.edges.size - 1)
    assert B.shape == t.truth[:, sl].shape and (B[~(t.T > 0)] == 0).all()
    r = mc.group_ratio(B, t.oracle[:, sl], t.truth[:, sl], t.floor[:, sl], t.bins)
    print(f"material-regime planck B {name} [{g_lo}, {g_hi}): largest ratio {r.max():.3g}")
    mc.assert_bound(r, handle)


@pytest.mark.parametrize("name", ["log", "wide", "narrow"])
def test_planck_dBdT(rtsn_mod, oracle_mod, name):
    """dB_g/dT(T(x)) of every group, the remainder's among them: the second half of a one-group
    shard's [q, b] after a coupled sweep (sigma_g = 1, so b is the derivative itself)."""
    import torch
    t = mc.planck_truth(oracle_mod, name, True)
    N, G = t.T.size, t.edges.size - 1
    q = rc.to_rt(mc.planck_params(oracle_mod, name))
    dB = np.empty((N, G))
    for shard in [sh for sh in mc.DBDT_SHARDS if sh[0] == name]:
        with rtsn_mod.Solver(q, g_lo=shard[1], g_hi=shard[2]) as s:
            assert s.groups()["kappa"][shard[1]] * q["rho"] == 1.0
            s.material_enable(1.0, t.T)
            qb = torch.empty(2 * N, dtype=torch.float64, device="cuda")
            s.material_sweep(qb)
            s.synchronize()
            dB[:, shard[1]] = qb[N:].cpu().numpy()
    assert (dB[~(t.T > 0)] == 0).all()
    r = mc.group_ratio(dB, t.oracle, t.truth, t.floor, t.bins)
    print(f"material-regime planck dB/dT {name}: largest ratio {r.max():.3g}")
    mc.assert_bound(r, name)


# ---------------------------------------------------------------------------
# material_update_kernel alone
# ---------------------------------------------------------------------------
def test_update_alone(rtsn_mod, oracle_mod):
    """rt_material_update on the caller's [q, b]: dT / T0 from -0.9 to 1e6 (4e-4 either side of
    the switch to the root), stiffness 1e-4 .. 1e12, cells at T0 = 0 heated -- T per cell, the
    next emission per group and the transit per decade of the new T."""
    import torch
    c = mc.update_case(oracle_mod)
    with rtsn_mod.Solver(rc.to_rt(c.p)) as s:
        s.material_enable(c.rho_cv, c.T0)
        s.material_update(torch.from_numpy(c.qb).cuda())
        got = mc.readouts(s)
    r = mc.update_ratios(got, c)
    print("material-regime update: largest ratio " + ", ".join(f"{k} {v.max():.3g}" for k, v in r.items()))
    for k, v in r.items():
        mc.assert_bound(v, k)


# ---------------------------------------------------------------------------
# coupled steps
# ---------------------------------------------------------------------------
def _coupled(s, case, what):
    for _ in range(case.steps):  # the handle's own [q, b], as the references do
        s.material_sweep()
        s.material_update()
    got = mc.coupled_readouts(s)
    r = mc.coupled_ratios(got, case)
    print(f"material-regime {what}: largest ratio " + ", ".join(f"{k} {v.max():.3g}" for k, v in r.items()))
    for k, v in r.items():
        mc.assert_bound(v, (what, k))


@pytest.mark.parametrize("N", mc.UNIFORM_N)
@pytest.mark.parametrize("pt", mc.UNIFORM_GRID, ids=[mc.point_id(p) for p in mc.UNIFORM_GRID])
def test_uniform_pass(rtsn_mod, oracle_mod, pt, N):
    """sweep_block_kernel with the per-cell emission, then the update: N = 70 and 320."""
    case = mc.coupled_case(oracle_mod, N, pt)
    with rtsn_mod.Solver(case.q) as s:
        s.material_enable(case.rho_cv[0], case.T0)
        _coupled(s, case, f"uniform N={N} {mc.point_id(pt)}")


@pytest.mark.parametrize("pt", mc.REGION_GRID, ids=[mc.point_id(p) for p in mc.REGION_GRID])
def test_region_chain_and_walk(rtsn_mod, oracle_mod, pt):
    """The slab (16, 32, 16) as a chain and, after rt_set_wavefront(0), as the walk over four
    16-cell segments: both against one truth."""
    case = mc.coupled_case(oracle_mod, mc.REGION_CELLS, pt)
    with rtsn_mod.Solver(case.q, regions=case.regions) as s:
        s.material_enable_regions(case.rho_cv, case.T0)
        assert s.wavefront_state()["active"]
        _coupled(s, case, f"chain {mc.point_id(pt)}")
    with rtsn_mod.Solver(case.q, regions=case.regions) as s:
        s.wavefront = 0
        s.time_block = 4
        s.set_segmentation(8)
        s.debug_set_segment_cells(16)
        assert s.sweep_geometry()[1] == 4 and not s.wavefront_state()["active"]
        s.material_enable_segments(case.rho_cv, case.T0)
        assert not s.wavefront_state()["active"]
        _coupled(s, case, f"walk {mc.point_id(pt)}")
