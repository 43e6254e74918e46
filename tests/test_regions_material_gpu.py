"""Material-temperature coupling on multi-region slabs on the GPU
(rt_material_enable_regions; kernels_wave.hip, the REG && CB forms of wavefront_kernel and
chain_kernel; the region forms of the material kernels).

* identical regions against the C oracle's uniform coupling (test_material_gpu.compare: T
  1e-12, fields 1e-10);
* the same uniform coupled slab however it is cut and whatever cells per lane: bitwise;
* heterogeneous slabs (rho x50, T x3, dx x4, rho_cv x10) against the numpy restatement
  tests/regions_material_ref.py, which tests/test_regions_material.py pins to the oracle --
  the shapes are the smallest at which each kernel form can go wrong: a one-wave pair, a
  region edge on a wave edge of a 3-wave chain, the wide pair's cell-0 map W0 at C = 1 on six
  waves, and the head lane's redone rows at C = 8 on five waves;
* BE energy on the device; group shards; the interface.
"""
from __future__ import annotations

import numpy as np
import pytest

from parity import per_group_rel
from regions_material_ref import RegionMaterialReference, plan_rule, region_energy
from test_material import C_LIGHT, net_outflow, params, t_profile
from test_material_gpu import GpuView, compare, to_rt
from test_regions_gpu import HETERO, TICK_REFLECTIVE, TICK_VACUUM
from test_regions_material import uniform_regions

pytestmark = pytest.mark.gpu

SCHEME_DT = {1: 1e-3, 2: 1e-3, 3: 1e-4}


def one_step_plan(cells, reflective, want=0):
    """(C, waves) of a coupled handle: `want` when admissible and fitting, else the nsteps = 1 rule."""
    edges = np.concatenate([[0], np.cumsum(cells)])
    if want and not (edges % want).any():
        used = int(edges[-1]) // want * (2 if reflective else 1)
        if -(-used // 64) <= 8:
            return want, -(-used // 64)
    return plan_rule(cells, reflective, 8, 1, TICK_VACUUM, TICK_REFLECTIVE)[:2]


def coupled_steps(s, n):
    for _ in range(n):  # a shard's own [q, b], as the references do
        s.material_sweep()
        s.material_update()


# ---------------------------------------------------------------------------
# 4: the uniform limit against the oracle
# ---------------------------------------------------------------------------
_oracle_cache = {}


def _oracle_run(oracle_mod, ts, bc, M):
    if (ts, bc, M) not in _oracle_cache:
        p = params(oracle_mod, ts=ts, dt=SCHEME_DT[ts], M=M, G=5, N=128, bc_left=bc[0], bc_right=bc[1])
        p["psi_source"] = np.linspace(0.5, 2.0, M * p["G"]).reshape(M, p["G"])
        orc = oracle_mod.OracleSolver(p)
        orc.material_enable(5.0, t_profile(p["N"]))
        orc.material_step(6)
        _oracle_cache[(ts, bc, M)] = (p, orc)
    return _oracle_cache[(ts, bc, M)]


@pytest.mark.parametrize("cuts", [(40, 24, 64), (8, 72, 48)])
@pytest.mark.parametrize("M", [6, 8])
@pytest.mark.parametrize("ts", [1, 2, 3])
@pytest.mark.parametrize("bc", [(0, 0), (2, 1), (1, 1)])
def test_uniform_limit_matches_oracle(rtsn_mod, oracle_mod, bc, ts, M, cuts):
    p, orc = _oracle_run(oracle_mod, ts, bc, M)
    with rtsn_mod.Solver(to_rt(p), regions=uniform_regions(p, cuts)) as s:
        s.material_enable_regions([5.0] * len(cuts), t_profile(p["N"]))
        coupled_steps(s, 6)
        print(compare(s, orc))


# ---------------------------------------------------------------------------
# 5: cut and C invariance, bitwise
# ---------------------------------------------------------------------------
def _coupled_readouts(s):
    return {"T": s.temperature(), "psi": s.psi(), "ends": s.ends(), "Beff": s.cell_emission(),
            "transit": s.material_transit()}


@pytest.mark.parametrize("bc", [(0, 0), (2, 1)])
def test_cut_and_cells_per_lane_invariance_bitwise(rtsn_mod, oracle_mod, bc):
    N, X = 128, 4.0  # dx = 1/32: width / cells is bitwise X / N for any cut
    p = params(oracle_mod, ts=3, dt=1e-4, M=6, G=5, N=N, bc_left=bc[0], bc_right=bc[1], X=X, dx=X / N)
    p["psi_source"] = np.linspace(0.5, 2.0, p["M"] * p["G"]).reshape(p["M"], p["G"])
    T0 = t_profile(N)
    first, seen = None, set()
    for cuts, c_max in (((1, 64, 127), 1), ((2, 66), 2), ((4, 68), 4), ((8, 72, 120), 8)):
        cells = [int(c) for c in np.diff([0] + list(cuts) + [N])]
        for want in (0, c_max):
            with rtsn_mod.Solver(to_rt(p), regions=uniform_regions(p, cells)) as s:
                if want:
                    s.set_wavefront_cells(want)
                s.material_enable_regions([5.0] * len(cells), T0)
                st = s.wavefront_state()
                assert (st["cells_per_lane"], st["waves"]) == one_step_plan(cells, bc[0] == 2, want)
                seen.add(st["cells_per_lane"])
                coupled_steps(s, 6)
                got = _coupled_readouts(s)
            assert np.isfinite(got["ends"]).all() and (got["T"] > 0).all()
            if first is None:
                first = got
            for k, v in first.items():
                assert np.array_equal(got[k], v), (k, cuts, want)
    assert seen == {1, 2, 4, 8}


# ---------------------------------------------------------------------------
# 6: heterogeneous slabs against the numpy reference
# ---------------------------------------------------------------------------
RHO_CV = {2: (5.0, 0.5), 3: (5.0, 0.5, 2.0)}  # x10 between regions


def _hetero_case(oracle_mod, name, ts, T=None):
    cells, dxs, rho, T_reg, bc_left, want, _ = HETERO[name]
    T_reg = T_reg if T is None else T
    p = params(oracle_mod, ts=ts, dt=SCHEME_DT[ts], M=6, G=5, N=int(sum(cells)), bc_left=bc_left,
               bc_right=1 if bc_left == 2 else 0)
    p["psi_source"] = np.linspace(0.5, 2.0, p["M"] * p["G"]).reshape(p["M"], p["G"])
    regions = [dict(cells=int(c), width=float(c * d), rho=float(r), kappa_grey=p["kappa_grey"], T=float(t),
                    group_kappa=None) for c, d, r, t in zip(cells, dxs, rho, T_reg)]
    return p, regions, RHO_CV[len(cells)], want


COLD = (1.0, 0.05, 1.5)  # n50's middle region, dense (rho = 10), cold under its neighbours' radiation


def _hetero(rtsn_mod, oracle_mod, name, ts, steps, T=None):
    p, regions, rho_cv, want = _hetero_case(oracle_mod, name, ts, T)
    cells = [r["cells"] for r in regions]
    ref = RegionMaterialReference(oracle_mod, p, regions, rho_cv)
    with rtsn_mod.Solver(to_rt(p), regions=regions) as s:
        if want:
            s.set_wavefront_cells(want)
        s.material_enable_regions(rho_cv)  # every cell at its region's T
        st = s.wavefront_state()
        assert st["active"] and (st["cells_per_lane"], st["waves"]) == one_step_plan(cells, p["bc_left"] == 2, want)
        assert per_group_rel(s.cell_emission(), ref.cell_emission(), 0) <= 1e-10
        coupled_steps(s, steps)
        ref.material_step(steps)
        assert np.isfinite(ref.ends()).all() and (ref.temperature() > 0).all()
        print(name, ts, st, compare(s, ref))
    return ref


@pytest.mark.parametrize("name", ["n32_reflective", "n50", "n130_wave_edge", "n168_wide_pair", "n1088_head_redo"])
def test_heterogeneous_reference_bdf2(rtsn_mod, oracle_mod, name):
    """BDF2, 4 steps (2 on the 1088-cell pair).  n168_wide_pair runs C = 1 on six waves (the
    pair's cell-0 map W0), n1088_head_redo C = 8 on five waves (the head lane's redone rows
    with the emission scale)."""
    if name == "n168_wide_pair":
        assert one_step_plan(HETERO[name][0], True, 1) == (1, 6)
    if name == "n1088_head_redo":
        assert one_step_plan(HETERO[name][0], True, 8) == (8, 5)
    if name == "n130_wave_edge":
        assert one_step_plan(HETERO[name][0], False) == (1, 3)
    ref = _hetero(rtsn_mod, oracle_mod, name, 3, 2 if name == "n1088_head_redo" else 4, COLD if name == "n50" else None)
    if name == "n50":
        assert ref.newton_cells > 0  # the cold region's cells solve the full emission


@pytest.mark.parametrize("ts", [1, 2])
def test_heterogeneous_reference_schemes(rtsn_mod, oracle_mod, ts):
    """BE and CN on the reflective two-region pair."""
    _hetero(rtsn_mod, oracle_mod, "n32_reflective", ts, 4)


# ---------------------------------------------------------------------------
# 7: energy on the device, BE
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("name,T,tol", [("n50", None, 1e-12), ("n50", COLD, 1e-11), ("n32_reflective", None, 1e-12)])
def test_backward_euler_energy_on_device(rtsn_mod, oracle_mod, name, T, tol):
    """Per step: the change of sum_x dx(x) (sum_g phi_g / c + rho_cv(x) T + transit) plus dt x
    the net boundary outflow, against the total (test_material_gpu.py's figures: 1e-12, and
    1e-11 where cells solve the full emission)."""
    p, regions, rho_cv, _ = _hetero_case(oracle_mod, name, 1, T)
    creg = np.repeat(np.arange(len(regions)), [r["cells"] for r in regions])
    dx = np.array([r["width"] / r["cells"] for r in regions])[creg]
    rcv = np.asarray(rho_cv)[creg]
    with rtsn_mod.Solver(to_rt(p), regions=regions) as s:
        s.material_enable_regions(rho_cv)
        for n in range(5):
            e0 = region_energy(s, dx, rcv, C_LIGHT)
            s.material_step(1)
            e1 = region_energy(s, dx, rcv, C_LIGHT)
            resid = (e1 - e0) + p["dt"] * net_outflow(GpuView(s), p)
            print(name, n, resid / e1)
            assert abs(resid) <= tol * abs(e1), (n, resid, e1)
            assert (s.temperature() > 0).all() and (s.cell_emission() >= 0).all()


# ---------------------------------------------------------------------------
# 8: group shards
# ---------------------------------------------------------------------------
def test_group_shards_on_one_gpu(rtsn_mod, oracle_mod):
    """Groups [0, 3) and [3, 5) as two region handles, their [q, b] summed on the device, equal
    the full handle."""
    import torch
    p, regions, rho_cv, _ = _hetero_case(oracle_mod, "n32_reflective", 2)
    q = to_rt(p)
    with rtsn_mod.Solver(q, regions=regions) as full:
        full.material_enable_regions(rho_cv)
        full.material_step(5)
        T_full, psi_full = full.temperature(), full.psi()
    shards = [rtsn_mod.Solver(q, g_lo=lo, g_hi=hi, regions=regions) for lo, hi in ((0, 3), (3, 5))]
    qb = [torch.zeros(2 * p["N"], dtype=torch.float64, device="cuda") for _ in shards]
    for s in shards:
        s.material_enable_regions(rho_cv)
        with pytest.raises(rtsn_mod.RtError) as e:
            s.material_step(1)  # a shard holds part of q
        assert e.value.status == 9
    for _ in range(5):
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
    assert per_group_rel(psi, psi_full, 1) <= 1e-12
    for s in shards:
        s.close()


# ---------------------------------------------------------------------------
# 9: the interface
# ---------------------------------------------------------------------------
def test_interface(rtsn_mod, oracle_mod):
    p, regions, rho_cv, _ = _hetero_case(oracle_mod, "n50", 3)
    q = to_rt(p)
    cells = [r["cells"] for r in regions]

    def status(fn):
        with pytest.raises(rtsn_mod.RtError) as e:
            fn()
        return e.value.status

    with rtsn_mod.Solver(q, regions=regions) as s:
        assert status(lambda: s.material_enable(1.0)) == 9
        assert "rt_material_enable_regions" in str(pytest.raises(rtsn_mod.RtError, s.material_enable, 1.0).value)
        assert status(lambda: s.material_enable_regions(rho_cv[:2])) == 8
        assert status(lambda: s.material_enable_regions(list(rho_cv) + [1.0])) == 8
        for bad in (0.0, -1.0, float("nan"), float("inf")):
            assert status(lambda: s.material_enable_regions([rho_cv[0], bad, rho_cv[2]])) == 8
        assert status(lambda: s.material_sweep()) == 9  # still off
        before = s.wavefront_state()
        assert (before["cells_per_lane"], before["waves"]) == plan_rule(cells, False, 8, 1000, TICK_VACUUM,
                                                                       TICK_REFLECTIVE)[:2]
        number = s.material_enable_regions(rho_cv)
        assert number > 0.0 and number == s.material_stability()
        after = s.wavefront_state()
        assert after["active"] and (after["cells_per_lane"], after["waves"]) == one_step_plan(cells, False)
        assert after["cells_per_lane"] != before["cells_per_lane"]  # this layout: C = 2 for one step, 1 for 1000
        assert status(lambda: s.advance(1)) == 9
        assert status(lambda: s.solve()) == 9
        s.material_step(2)
        assert np.isfinite(s.temperature()).all()
    with rtsn_mod.Solver(dict(q, V=2.0, use_correction=1), regions=regions) as s:
        assert status(lambda: s.material_enable_regions(rho_cv)) == 3
    # a plain handle: one region's worth, the call is rt_material_enable
    T0 = t_profile(p["N"])
    out = []
    for regional_call in (False, True):
        with rtsn_mod.Solver(q) as s:
            if regional_call:
                assert status(lambda: s.material_enable_regions([4.0, 4.0])) == 8
                s.material_enable_regions([4.0], T0)
            else:
                s.material_enable(4.0, T0)
            s.material_step(3)
            out.append((s.temperature(), s.ends(), s.cell_emission()))
    for a, b in zip(*out):
        assert np.array_equal(a, b)


def test_stability_is_the_stiffest_regions(rtsn_mod, oracle_mod):
    """rt_material_stability on a region handle: the largest over the regions r of dt W sum_g
    sigma_{r,g} dB_g/dT(T_max,r) / rho_cv,r, T_max,r region r's hottest cell."""
    p, regions, rho_cv, _ = _hetero_case(oracle_mod, "n50", 1)
    T0 = np.concatenate([np.linspace(0.3, 0.9, 20), np.linspace(1.2, 0.2, 10), np.linspace(0.5, 1.4, 20)])
    with rtsn_mod.Solver(to_rt(p), regions=regions) as s:
        got = s.material_enable_regions(rho_cv, T0)
        W = s.quad()[1].sum()
        e = s.groups()["e_edge"]
        want = 0.0
        for k, (lo, hi) in enumerate(((0, 20), (20, 30), (30, 50))):
            _, dB = rtsn_mod.planck_groups(float(T0[lo:hi].max()), e)
            want = max(want, p["dt"] * W * float((regions[k]["rho"] * s.region_data(k)["kappa"] * dB).sum()) / rho_cv[k])
    assert got == pytest.approx(want, rel=1e-12)
