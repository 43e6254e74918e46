"""Material-temperature coupling on multi-region slabs in SEGMENT mode on the GPU
(rt_material_enable_segments; kernels.hip sweep_walk_kernel, the one-launch line walk).

* the chain-mode coupled handle against the walk, BITWISE: both apply the same map with the same
  emission scale to exact inputs, and phi comes from the same moments kernels;
* independence of the segment plan (2, 5, 20 segments, a re-plan in mid-run) and of
  material_step against sweep + update, bitwise;
* identical regions against the C oracle's uniform coupling (test_material_gpu.compare: T 1e-12,
  the rest 1e-10);
* lines no chain admits (N = 4112; 2064 reflective, the head cell's region one 16-cell
  segment) against the numpy restatement tests/regions_material_ref.py;
* the Newton path; two workgroups per half with the second partly filled; BE energy on the
  device; group shards; the interface.

Every segment-mode handle asserts its premise: not on the wavefront, the planned number of
segments, and (but for the deliberate two-segment plan of the two-region slab) more segments
than regions, so that the walk crosses segment edges inside a region as well as region edges.
"""
from __future__ import annotations

import numpy as np
import pytest

from parity import per_group_rel
from regions_material_ref import RegionMaterialReference, region_energy
from test_material import C_LIGHT, net_outflow, params
from test_material_gpu import GpuView, compare, to_rt
from test_regions_material import uniform_regions
from test_regions_material_gpu import COLD, RHO_CV, SCHEME_DT, _coupled_readouts, _oracle_run, coupled_steps
from test_regions_segments_gpu import SLABS, _segment_mode, _status

pytestmark = pytest.mark.gpu

# the segment tests' slabs: rho x50, T x3, dx x4 between regions; rho_cv x10 (RHO_CV)
#       name: cells per segment to plan for (0: rt_set_segmentation(8) alone), segments
PLAN = {"three": (64, 6), "two": (0, 20)}


def _case(oracle_mod, cells, dxs, rho, T, ts, bc, M=6, G=5):
    """test_regions_material_gpu._hetero_case's parameters on a layout of this file."""
    p = params(oracle_mod, ts=ts, dt=SCHEME_DT[ts], M=M, G=G, N=int(sum(cells)), bc_left=bc[0], bc_right=bc[1])
    p["psi_source"] = np.linspace(0.5, 2.0, M * G).reshape(M, G)
    regions = [dict(cells=int(c), width=float(c * d), rho=float(r), kappa_grey=p["kappa_grey"], T=float(t),
                    group_kappa=None) for c, d, r, t in zip(cells, dxs, rho, T)]
    return p, regions, RHO_CV[len(cells)]


def _slab(oracle_mod, name, ts, bc, **kw):
    cells, dxs, rho, T = SLABS[name][:4]
    return _case(oracle_mod, cells, dxs, rho, T, ts, bc, **kw)


def _walk_handle(s, regions, cells, segments, more_than_regions=True):
    """Chain mode -> segment mode with the plan asked for; the premise of a walk test."""
    Sg = _segment_mode(s, 4, cells=cells)
    assert Sg == segments and Sg >= len(regions)
    assert Sg > len(regions) or not more_than_regions
    assert not s.wavefront_state()["active"]
    return Sg


def _chain_run(rtsn_mod, p, regions, rho_cv, steps):
    with rtsn_mod.Solver(to_rt(p), regions=regions) as s:
        s.material_enable_regions(rho_cv)
        assert s.wavefront_state()["active"]
        coupled_steps(s, steps)
        return _coupled_readouts(s)


# ---------------------------------------------------------------------------
# 1: the chain against the walk, bitwise
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("ts", [1, 2, 3])
@pytest.mark.parametrize("bc", [(0, 0), (2, 1), (1, 1)])
@pytest.mark.parametrize("name", sorted(PLAN))
def test_chain_against_walk_bitwise(rtsn_mod, oracle_mod, name, bc, ts):
    """6 coupled steps on a chain-mode handle and on a handle taken to segment mode first:
    (96, 160, 64) at 64 cells per segment (48, 48 | 64, 48, 48 | 64) and (48, 272) in 20
    segments of 16.  T, psi, ends, Beff and transit are array_equal."""
    p, regions, rho_cv = _slab(oracle_mod, name, ts, bc)
    chain = _chain_run(rtsn_mod, p, regions, rho_cv, 6)
    with rtsn_mod.Solver(to_rt(p), regions=regions) as s:
        _walk_handle(s, regions, *PLAN[name])
        s.material_enable_segments(rho_cv)
        assert not s.wavefront_state()["active"] and s.sweep_geometry()[1] == PLAN[name][1]
        coupled_steps(s, 6)
        walk = _coupled_readouts(s)
    assert np.isfinite(walk["ends"]).all() and (walk["T"] > 0).all()
    for k, v in chain.items():
        assert np.array_equal(walk[k], v), k


# ---------------------------------------------------------------------------
# 2: independence of the plan and of how the steps are driven, bitwise
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("bc", [(0, 0), (2, 1)])
def test_independence_bitwise(rtsn_mod, oracle_mod, bc):
    """BDF2 on (48, 272), 6 steps: plans of 2, 5 and 20 segments (targets 272, 80, 16), a
    re-plan from 5 to 20 segments between steps 3 and 4 (rt_debug_set_segment_cells, then
    rt_set_time_block and rt_set_segmentation, all accepted while coupled), and material_step(6)
    against 6 x (material_sweep, material_update): every read-out array_equal to the first
    run's."""
    p, regions, rho_cv = _slab(oracle_mod, "two", 3, bc)

    def run(cells, segments, drive):
        with rtsn_mod.Solver(to_rt(p), regions=regions) as s:
            _walk_handle(s, regions, cells, segments, more_than_regions=segments > 2)
            s.material_enable_segments(rho_cv)
            drive(s)
            assert not s.wavefront_state()["active"]
            return _coupled_readouts(s)

    def replan(s):
        coupled_steps(s, 3)
        s.debug_set_segment_cells(16)
        assert s.sweep_geometry()[1] == 20
        s.time_block = 8
        s.set_segmentation(4)
        assert s.sweep_geometry()[1] == 20 and not s.wavefront_state()["active"]
        coupled_steps(s, 3)

    ref = run(16, 20, lambda s: coupled_steps(s, 6))
    variants = [(272, 2, lambda s: coupled_steps(s, 6)), (80, 5, lambda s: coupled_steps(s, 6)),
                (80, 5, replan), (80, 5, lambda s: s.material_step(6)), (16, 20, lambda s: s.material_step(6))]
    for n, v in enumerate(variants):
        got = run(*v)
        for k, want in ref.items():
            assert np.array_equal(got[k], want), (k, n, v[:2])


# ---------------------------------------------------------------------------
# 3: the uniform limit against the C oracle
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("ts", [1, 2, 3])
@pytest.mark.parametrize("bc", [(0, 0), (2, 1)])
def test_uniform_limit_matches_oracle(rtsn_mod, oracle_mod, bc, ts):
    """N = 128 cut into identical regions (48, 80), 8 segments of 16, 6 steps, against the
    oracle run tests/test_regions_material_gpu.py computes once per (scheme, boundaries)."""
    from test_material import t_profile
    p, orc = _oracle_run(oracle_mod, ts, bc, 6)
    regions = uniform_regions(p, (48, 80))
    with rtsn_mod.Solver(to_rt(p), regions=regions) as s:
        _walk_handle(s, regions, 16, 8)
        s.material_enable_segments([5.0, 5.0], t_profile(p["N"]))
        coupled_steps(s, 6)
        print(compare(s, orc))


# ---------------------------------------------------------------------------
# 4: lines no chain admits, against the numpy restatement
# ---------------------------------------------------------------------------
LONG = {
    # name: (cells, boundary pair, scheme)
    "n4112_vacuum_bdf2": ((1040, 3072), (0, 0), 3),
    "n2064_reflective_bdf2": ((16, 2048), (2, 1), 3),
    "n2064_reflective_be": ((16, 2048), (2, 1), 1),
}
LONG_STEPS = 2


@pytest.mark.parametrize("name", sorted(LONG))
def test_beyond_the_chain(rtsn_mod, oracle_mod, name):
    """The smallest layouts no chain admits (4112 > 4096 cells; 2064 > 2048 reflective, region 0
    a single 16-cell segment that holds the head cell): the handle comes up in segment mode from
    rt_create_regions, 2 coupled steps against RegionMaterialReference (compare: T 1e-12, the
    rest 1e-10)."""
    cells, bc, ts = LONG[name]
    dxs, rho, T = SLABS["two"][1:4]
    p, regions, rho_cv = _case(oracle_mod, cells, dxs, rho, T, ts, bc)
    assert _status(rtsn_mod, lambda: rtsn_mod.regions_plan(regions, bc[0] == 2)) == 3  # no chain
    ref = RegionMaterialReference(oracle_mod, p, regions, rho_cv)
    with rtsn_mod.Solver(to_rt(p), regions=regions) as s:
        st = s.wavefront_state()
        assert not st["active"] and st["mode"] == 0 and s.pipeline == 2  # segment mode from create
        Sg = s.sweep_geometry()[1]
        assert Sg > len(regions)
        if cells[0] == 16:  # the head cell's region is one segment
            plan = rtsn_mod.regions_plan_segments(regions, 16)
            assert plan["first_cell"][:2] == [0, 16]
        s.material_enable_segments(rho_cv)
        assert per_group_rel(s.cell_emission(), ref.cell_emission(), 0) <= 1e-10
        coupled_steps(s, LONG_STEPS)
        ref.material_step(LONG_STEPS)
        assert np.isfinite(ref.ends()).all() and (ref.temperature() > 0).all()
        print(name, Sg, compare(s, ref))


# ---------------------------------------------------------------------------
# 5: the Newton path
# ---------------------------------------------------------------------------
def test_newton_path(rtsn_mod, oracle_mod):
    """N = 80 in (32, 16, 32), the middle region dense (rho = 10) and cold (0.05 keV) under its
    neighbours' radiation: cells solve the full emission.  BDF2, 4 steps, 5 segments."""
    p, regions, rho_cv = _case(oracle_mod, (32, 16, 32), (0.004, 0.016, 0.008), (1.0, 10.0, 0.2), COLD, 3, (0, 0))
    ref = RegionMaterialReference(oracle_mod, p, regions, rho_cv)
    with rtsn_mod.Solver(to_rt(p), regions=regions) as s:
        _walk_handle(s, regions, 16, 5)
        s.material_enable_segments(rho_cv)
        coupled_steps(s, 4)
        ref.material_step(4)
        assert np.isfinite(ref.ends()).all() and (ref.temperature() > 0).all()
        print(compare(s, ref))
    assert ref.newton_cells > 0


# ---------------------------------------------------------------------------
# 6: more than one workgroup per half, the last one partly filled
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("bc", [(0, 0), (2, 1)])
def test_two_workgroups_per_half_bitwise(rtsn_mod, oracle_mod, bc):
    """M = 16 (8 lines per group and half) x 9 groups = 72 lines: two workgroups per half, the
    second with 8 live lanes (the emission scale's group index clamped on the padding lanes).
    (48, 272), BDF2, 3 steps, chain against walk, array_equal."""
    p, regions, rho_cv = _slab(oracle_mod, "two", 3, bc, M=16, G=9)
    chain = _chain_run(rtsn_mod, p, regions, rho_cv, 3)
    with rtsn_mod.Solver(to_rt(p), regions=regions) as s:
        assert (p["M"] // 2) * p["G"] == 72
        Sg = _segment_mode(s, 4, cells=16)
        assert Sg == 20 and s.sweep_geometry()[0] == 2 * 2 * Sg  # Q = 2 workgroups per half and segment
        s.material_enable_segments(rho_cv)
        assert not s.wavefront_state()["active"]
        coupled_steps(s, 3)
        walk = _coupled_readouts(s)
    assert np.isfinite(walk["ends"]).all() and (walk["T"] > 0).all()
    for k, v in chain.items():
        assert np.array_equal(walk[k], v), k


# ---------------------------------------------------------------------------
# 7: energy on the device, BE
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("bc", [(0, 0), (2, 1)])
def test_backward_euler_energy_on_device(rtsn_mod, oracle_mod, bc):
    """Per step on (96, 160, 64): the change of sum_x dx(x) (sum_g phi_g / c + rho_cv(x) T +
    transit) plus dt x the net boundary outflow is at most 1e-12 of the total (the figure of
    tests/test_regions_material_gpu.py); T > 0 and Beff >= 0."""
    p, regions, rho_cv = _slab(oracle_mod, "three", 1, bc)
    creg = np.repeat(np.arange(len(regions)), [r["cells"] for r in regions])
    dx = np.array([r["width"] / r["cells"] for r in regions])[creg]
    rcv = np.asarray(rho_cv)[creg]
    with rtsn_mod.Solver(to_rt(p), regions=regions) as s:
        _walk_handle(s, regions, *PLAN["three"])
        s.material_enable_segments(rho_cv)
        for n in range(5):
            e0 = region_energy(s, dx, rcv, C_LIGHT)
            s.material_step(1)
            e1 = region_energy(s, dx, rcv, C_LIGHT)
            resid = (e1 - e0) + p["dt"] * net_outflow(GpuView(s), p)
            print(bc, n, resid / e1)
            assert abs(resid) <= 1e-12 * abs(e1), (n, resid, e1)
            assert (s.temperature() > 0).all() and (s.cell_emission() >= 0).all()


# ---------------------------------------------------------------------------
# 8: group shards
# ---------------------------------------------------------------------------
def test_group_shards_on_one_gpu(rtsn_mod, oracle_mod):
    """Groups [0, 3) and [3, 5) as two segment-mode handles on (48, 272), reflective, CN, their
    [q, b] summed on the device, 5 steps: T equals the full segment-mode handle's at rtol 1e-12,
    psi at 1e-12 per group; material_step on a shard returns RT_ERR_STATE."""
    import torch
    p, regions, rho_cv = _slab(oracle_mod, "two", 2, (2, 1))
    q = to_rt(p)
    with rtsn_mod.Solver(q, regions=regions) as full:
        _walk_handle(full, regions, *PLAN["two"])
        full.material_enable_segments(rho_cv)
        full.material_step(5)
        T_full, psi_full = full.temperature(), full.psi()
    shards = [rtsn_mod.Solver(q, g_lo=lo, g_hi=hi, regions=regions) for lo, hi in ((0, 3), (3, 5))]
    try:
        qb = [torch.zeros(2 * p["N"], dtype=torch.float64, device="cuda") for _ in shards]
        for s in shards:
            _walk_handle(s, regions, *PLAN["two"])
            s.material_enable_segments(rho_cv)
            assert _status(rtsn_mod, lambda: s.material_step(1)) == 9  # a shard holds part of q
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
            assert not s.wavefront_state()["active"]
            np.testing.assert_allclose(s.temperature(), T_full, rtol=1e-12)
        psi = np.concatenate([s.psi() for s in shards], axis=1)
        assert per_group_rel(psi, psi_full, 1) <= 1e-12
    finally:
        for s in shards:
            s.close()


# ---------------------------------------------------------------------------
# 9: the interface
# ---------------------------------------------------------------------------
def test_interface(rtsn_mod, oracle_mod):
    p, regions, rho_cv = _slab(oracle_mod, "three", 3, (0, 0))
    q = to_rt(p)
    L = rtsn_mod.lib()

    def status(fn):
        return _status(rtsn_mod, fn)

    def message(s):
        return L.rt_last_error(s._h).decode()

    # a plain handle and a chain-mode region handle: RT_ERR_STATE, naming the call that applies
    with rtsn_mod.Solver(q) as s:
        assert status(lambda: s.material_enable_segments([1.0])) == 9
        assert "rt_material_enable" in message(s) and "rt_material_enable_regions" not in message(s)
        assert status(lambda: s.material_enable_segments([1.0, 1.0])) == 8  # the arguments come first
    with rtsn_mod.Solver(q, regions=regions) as s:
        assert s.wavefront_state()["active"]
        assert status(lambda: s.material_enable_segments(rho_cv)) == 9
        assert "rt_material_enable_regions" in message(s)
        assert status(lambda: s.material_sweep()) == 9  # still off
    with rtsn_mod.Solver(q, regions=regions) as s:
        _walk_handle(s, regions, *PLAN["three"])
        # the arguments, as rt_material_enable_regions checks them
        assert L.rt_material_enable_segments(s._h, None, 3, None) == 8
        assert status(lambda: s.material_enable_segments(rho_cv[:2])) == 8
        assert status(lambda: s.material_enable_segments(list(rho_cv) + [1.0])) == 8
        for bad in (0.0, -1.0, float("nan"), float("inf")):
            assert status(lambda: s.material_enable_segments([rho_cv[0], bad, rho_cv[2]])) == 8
        # rt_material_enable_regions stays refused here, and names the new call
        assert status(lambda: s.material_enable_regions(rho_cv)) == 9
        assert "segment mode" in message(s) and "rt_material_enable_segments" in message(s)
        assert status(lambda: s.material_enable(1.0)) == 9
        assert status(lambda: s.material_sweep()) == 9  # still off
        number = s.material_enable_segments(rho_cv)
        assert number > 0.0 and number == s.material_stability()
        # while the coupling is on
        for mode in (0, 1, 2):
            assert status(lambda: setattr(s, "wavefront", mode)) == 9
        assert not s.wavefront_state()["active"]
        assert status(lambda: s.advance(1)) == 9
        assert status(lambda: s.solve()) == 9
        # one launch per coupled sweep
        s.set_profiling(True)
        n0 = s.sweep_time()[1]
        for n in range(1, 4):
            s.material_sweep()
            s.material_update()
            assert s.sweep_time()[1] == n0 + n
        s.set_profiling(False)
        before = _coupled_readouts(s)
        # the setters of the plan are accepted and re-plan
        s.set_segmentation(8)
        s.time_block = 12
        assert s.time_block == 12
        s.debug_set_segment_cells(16)
        assert s.sweep_geometry()[1] == 20
        after = _coupled_readouts(s)
        for k, v in before.items():
            assert np.array_equal(after[k], v), k  # a re-plan touches no state
        s.material_step(2)
        assert np.isfinite(s.temperature()).all() and np.isfinite(s.ends()).all()
    with rtsn_mod.Solver(dict(q, V=2.0, use_correction=1), regions=regions) as s:
        _segment_mode(s, 4, cells=64)
        assert status(lambda: s.material_enable_segments(rho_cv)) == 3
