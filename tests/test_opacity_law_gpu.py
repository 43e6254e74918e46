"""The temperature-dependent opacity of the material coupling on the GPU
(rt_material_set_opacity_law; kernels.hip sweep_walk_law_kernel, the law form of the line walk).

* parity with the fp64 restatement tests/opacity_law_ref.py (test_material_gpu.compare: T 1e-12,
  the rest 1e-10) over 6 steps, BE / CN / BDF2 at SCHEME_DT, boundary pairs (0,0), (2,1), (1,1):
  (32, 48) cells at 16 per segment (5 segments: edges inside regions and at the region edge),
  (16, 16) (the reflective head cell's region a single chunk), exponents (3, 1.5) and (-1, 0),
  a case with both clamps active, and M = 8, G = 17 (68 lines per half: the second workgroup
  partly filled); f(x) against the reference at 1e-14 relative;
* BE energy on the device at 1e-12 per step, and across a law set in mid-run with owed emission
  outstanding;
* independence of the segment plan and of material_step against sweep + update, bitwise;
* the law set and cleared before any step: bitwise the plain walk; exponent 0: the plain walk
  within compare's tolerances;
* group shards (0,2), (2,5) with [q, b] summed by the test; the statuses;
* one family against the reference in np.longdouble (tests/test_opacity_law.py law_regime_case).

The conditions the cases rest on (f spans a decade, both update paths taken, no cell at the
switch between them, T > 0) are asserted on the reference alone in tests/test_opacity_law.py.
"""
from __future__ import annotations

import numpy as np
import pytest

import opacity_law_ref as olr
from parity import per_group_rel
from test_material import net_outflow
from test_material_gpu import GpuView, compare, to_rt
from test_regions_material_gpu import _coupled_readouts, coupled_steps
from test_regions_segments_gpu import _segment_mode, _status

pytestmark = pytest.mark.gpu


def _open(rtsn_mod, oracle_mod, layout, ts, bc, law=None, seg=None, segments=None, **shard):
    """A coupled segment-mode handle of a layout on its plan (seg cells per segment), the law set."""
    p, regions, rho_cv, T0 = olr.case(oracle_mod, layout, ts, bc)
    L = olr.LAYOUTS[layout]
    s = rtsn_mod.Solver(to_rt(p), regions=regions, **shard)
    try:
        Sg = _segment_mode(s, 4, cells=seg or L["seg"])
        assert Sg == (segments or L["segments"]) and not s.wavefront_state()["active"]
        s.material_enable_segments(rho_cv, T0)
        if law:
            s.material_set_opacity_law(*olr.law_args(law))
    except BaseException:
        s.close()
        raise
    return s, p


def _f_rel(s, ref):
    """opacity_scale() against the reference's law at the handle's own T(x), relative: the device
    pow against numpy's.  (Against the reference's own f the difference carries |exponent| times
    the difference in T, which compare holds to 1e-12: asserted at 1e-11 here, exponents <= 3.)"""
    got = s.opacity_scale()
    if ref.law is None:
        assert np.array_equal(got, np.ones(s.N))
        return 0.0
    f = np.asarray(ref.opacity_scale(), dtype=np.float64)
    assert np.max(np.abs(got - f) / f) <= 1e-11
    own = np.asarray(ref._scale(s.temperature().astype(ref.dtype)), dtype=np.float64)
    return float(np.max(np.abs(got - own) / own))


# ---------------------------------------------------------------------------
# 1: parity with the reference
# ---------------------------------------------------------------------------
PARITY = [(lay, law, ts, bc) for lay, law in olr.PARITY for ts in (1, 2, 3) for bc in olr.BCS] + [olr.WIDE_CASE]


@pytest.mark.parametrize("layout,law,ts,bc", PARITY, ids=lambda v: str(v).replace(" ", ""))
def test_parity(rtsn_mod, oracle_mod, layout, law, ts, bc):
    r = olr.reference_run(oracle_mod, layout, law, ts, bc)
    s, p = _open(rtsn_mod, oracle_mod, layout, ts, bc, law)
    with s:
        if layout == "n32_wide":
            assert (p["M"] // 2) * p["G"] == 68 and s.sweep_geometry()[0] == 2 * 2 * olr.LAYOUTS[layout]["segments"]
        assert np.max(np.abs(s.opacity_scale() - r["f0"]) / r["f0"]) <= 1e-14  # the same T0: the device pow alone
        coupled_steps(s, olr.STEPS)
        assert not s.wavefront_state()["active"]
        err = compare(s, r["ref"])
        err["f"] = _f_rel(s, r["ref"])
        print(layout, law, ts, bc, err)
        assert err["f"] <= 1e-14, err


# ---------------------------------------------------------------------------
# 2: energy, BE
# ---------------------------------------------------------------------------
def _energy_terms(p, regions, rho_cv):
    creg = np.repeat(np.arange(len(regions)), [r["cells"] for r in regions])
    return (np.array([r["width"] / r["cells"] for r in regions])[creg], np.asarray(rho_cv)[creg])


@pytest.mark.parametrize("bc", olr.BCS)
@pytest.mark.parametrize("law", ["marshak", "clamped"])
def test_backward_euler_energy_on_device(rtsn_mod, oracle_mod, law, bc):
    """Per step on (32, 48): the change of sum_x dx(x) (sum_g phi_g / c + rho_cv(x) T + transit)
    plus dt x the net boundary outflow is at most 1e-12 of the total; T > 0 and Beff >= 0."""
    s, p = _open(rtsn_mod, oracle_mod, "n80", 1, bc, law)
    _, regions, rho_cv, _ = olr.case(oracle_mod, "n80", 1, bc)
    dx, rcv = _energy_terms(p, regions, rho_cv)
    with s:
        for n in range(olr.STEPS):
            e0 = olr.energy(s, dx, rcv)
            s.material_step(1)
            e1 = olr.energy(s, dx, rcv)
            resid = (e1 - e0) + p["dt"] * net_outflow(GpuView(s), p)
            print(law, bc, n, resid / e1)
            assert abs(resid) <= 1e-12 * abs(e1), (n, resid, e1)
            assert (s.temperature() > 0).all() and (s.cell_emission() >= 0).all()


@pytest.mark.parametrize("bc", [(0, 0), (2, 1)])
def test_law_set_in_mid_run_conserves_energy(rtsn_mod, oracle_mod, bc):
    """BE on (32, 48): 3 steps without the law, so that emission is owed; the law set, changed
    and cleared between steps.  The energy sum is unchanged across each call at 1e-12 (the owed
    rescale), every later step balances at 1e-12, and the run equals the reference driven the
    same way (compare's tolerances)."""
    s, p = _open(rtsn_mod, oracle_mod, "n80", 1, bc)
    _, regions, rho_cv, T0 = olr.case(oracle_mod, "n80", 1, bc)
    dx, rcv = _energy_terms(p, regions, rho_cv)
    ref = olr.OpacityLawReference(oracle_mod, p, regions, rho_cv, T0)
    calls = [olr.law_args("marshak"), olr.law_args("clamped"), (None, None, 1.0, 1.0), olr.law_args("mixed")]
    with s:
        s.material_step(3)
        ref.material_step(3)
        assert np.abs(s.material_transit()).max() > 0.0  # emission is in transit when the law arrives
        for args in calls:
            e0 = olr.energy(s, dx, rcv)
            s.material_set_opacity_law(*args)
            ref.set_law(*args)
            e1 = olr.energy(s, dx, rcv)
            print(bc, args[0], (e1 - e0) / e1)
            assert abs(e1 - e0) <= 1e-12 * abs(e1), (args, e0, e1)
            assert _f_rel(s, ref) <= 1e-14
            for n in range(2):
                e0 = e1
                s.material_step(1)
                ref.material_step(1)
                e1 = olr.energy(s, dx, rcv)
                resid = (e1 - e0) + p["dt"] * net_outflow(GpuView(s), p)
                assert abs(resid) <= 1e-12 * abs(e1), (args, n, resid, e1)
        print(compare(s, ref))


# ---------------------------------------------------------------------------
# 3: independence of the plan and of how the steps are driven, bitwise
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("bc", [(0, 0), (2, 1)])
def test_independence_bitwise(rtsn_mod, oracle_mod, bc):
    """BDF2 on (32, 48) with exponents (3, 1.5), 6 steps: plans of 2, 3 and 5 segments (targets
    48, 32, 16), a re-plan from 2 to 5 segments between steps 3 and 4, and material_step(6)
    against 6 x (material_sweep, material_update): every read-out and f array_equal."""

    def run(seg, segments, drive):
        s, _ = _open(rtsn_mod, oracle_mod, "n80", 3, bc, "marshak", seg=seg, segments=segments)
        with s:
            drive(s)
            assert not s.wavefront_state()["active"]
            return dict(_coupled_readouts(s), f=s.opacity_scale())

    def replan(s):
        coupled_steps(s, 3)
        s.debug_set_segment_cells(16)
        assert s.sweep_geometry()[1] == 5
        coupled_steps(s, 3)

    first = run(16, 5, lambda s: coupled_steps(s, 6))
    variants = [(48, 2, lambda s: coupled_steps(s, 6)), (32, 3, lambda s: coupled_steps(s, 6)), (48, 2, replan),
                (16, 5, lambda s: s.material_step(6)), (32, 3, lambda s: s.material_step(6))]
    for n, v in enumerate(variants):
        got = run(*v)
        for k, want in first.items():
            assert np.array_equal(got[k], want), (k, n, v[:2])


# ---------------------------------------------------------------------------
# 4: the law off, and exponent 0
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("ts", [1, 3])
def test_law_cleared_before_any_step_is_the_plain_walk_bitwise(rtsn_mod, oracle_mod, ts):
    bc = (2, 1)
    plain, _ = _open(rtsn_mod, oracle_mod, "n80", ts, bc)
    with plain:
        coupled_steps(plain, 4)
        want = _coupled_readouts(plain)
    s, _ = _open(rtsn_mod, oracle_mod, "n80", ts, bc, "marshak")
    with s:
        assert s.opacity_scale().max() > 10.0
        s.material_set_opacity_law(None, None, 1.0, 1.0)
        assert np.array_equal(s.opacity_scale(), np.ones(s.N))
        coupled_steps(s, 4)
        got = _coupled_readouts(s)
    for k, v in want.items():
        assert np.array_equal(got[k], v), k


class _AsReference:
    """A full-group solver with the attributes compare reads from a reference."""

    def __init__(self, s):
        self.s, self.g_lo, self.Gl, self.G = s, 0, s.G, s.G

    def __getattr__(self, name):
        return getattr(self.s, name)


@pytest.mark.parametrize("ts", [1, 2, 3])
@pytest.mark.parametrize("bc", [(0, 0), (2, 1)])
def test_exponent_zero_is_the_plain_walk_to_rounding(rtsn_mod, oracle_mod, bc, ts):
    """The law kernel with f = 1 against the map walk, compare's tolerances: not bitwise, the
    maps are derived in long double and the law kernel's constants in fp64."""
    plain, _ = _open(rtsn_mod, oracle_mod, "n80", ts, bc)
    s, _ = _open(rtsn_mod, oracle_mod, "n80", ts, bc, "zero")
    with plain, s:
        assert np.array_equal(s.opacity_scale(), np.ones(s.N))
        coupled_steps(plain, olr.STEPS)
        coupled_steps(s, olr.STEPS)
        print(bc, ts, compare(s, _AsReference(plain)))


# ---------------------------------------------------------------------------
# 5: read-outs
# ---------------------------------------------------------------------------
def test_readouts(rtsn_mod, oracle_mod):
    """rt_group_absorption_device and rt_material_stability with the law on: the absorption
    against the reference's sum_g sigma0_g f phi_g at 1e-10; the stability number of a one-region
    slab is the unscaled number times f at the hottest cell."""
    import torch
    r = olr.reference_run(oracle_mod, "n80", "marshak", 1, (2, 1))
    s, p = _open(rtsn_mod, oracle_mod, "n80", 1, (2, 1), "marshak")
    with s:
        coupled_steps(s, olr.STEPS)
        out = torch.zeros(p["N"], dtype=torch.float64, device="cuda")
        s.group_absorption(out)
        s.synchronize()
        want = r["ref"].group_absorption()
        assert np.abs(out.cpu().numpy() - want).max() <= 1e-10 * np.abs(want).max()
    # one region, taken to segment mode with rt_set_wavefront(s, 0)
    q = olr.case(oracle_mod, "n32", 1, (0, 0))[0]
    one = [dict(cells=32, width=32 * 0.004, rho=10.0, kappa_grey=q["kappa_grey"], T=0.5, group_kappa=None)]
    T0 = np.linspace(0.2, 0.8, 32)
    with rtsn_mod.Solver(to_rt(q), regions=one) as u:
        _segment_mode(u, 4, cells=16)
        number = u.material_enable_segments([0.5], T0)
        u.material_set_opacity_law([2.0], [0.4], 1e-3, 1e3)
        assert u.material_stability() == pytest.approx(number * (0.8 / 0.4) ** -2.0, rel=1e-13)
        assert np.max(np.abs(u.opacity_scale() / (T0 / 0.4) ** -2.0 - 1.0)) <= 1e-14
        u.material_step(2)
        assert np.isfinite(u.ends()).all() and (u.temperature() > 0).all()


# ---------------------------------------------------------------------------
# 6: group shards
# ---------------------------------------------------------------------------
def test_group_shards_on_one_gpu(rtsn_mod, oracle_mod):
    """Groups [0, 2) and [2, 5) as two handles on (32, 48), reflective, BDF2, exponents (3, 1.5),
    their [q, b] summed by the test, 6 steps: T equals the full handle's at rtol 1e-12, f at
    1e-12, psi at 1e-10 per group."""
    import torch
    ts, bc = 3, (2, 1)
    full, p = _open(rtsn_mod, oracle_mod, "n80", ts, bc, "marshak")
    with full:
        full.material_step(olr.STEPS)
        T_full, psi_full, f_full = full.temperature(), full.psi(), full.opacity_scale()
    shards = [_open(rtsn_mod, oracle_mod, "n80", ts, bc, "marshak", g_lo=lo, g_hi=hi)[0] for lo, hi in ((0, 2), (2, 5))]
    try:
        qb = [torch.zeros(2 * p["N"], dtype=torch.float64, device="cuda") for _ in shards]
        for _ in range(olr.STEPS):
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
            np.testing.assert_allclose(s.opacity_scale(), f_full, rtol=1e-12)
        psi = np.concatenate([s.psi() for s in shards], axis=1)
        assert per_group_rel(psi, psi_full, 1) <= 1e-10
    finally:
        for s in shards:
            s.close()


# ---------------------------------------------------------------------------
# 7: the statuses
# ---------------------------------------------------------------------------
def test_statuses(rtsn_mod, oracle_mod):
    p, regions, rho_cv, T0 = olr.case(oracle_mod, "n80", 3, (0, 0))
    q = to_rt(p)
    L = rtsn_mod.lib()
    law = olr.law_args("marshak")

    def status(fn):
        return _status(rtsn_mod, fn)

    def message(s):
        return L.rt_last_error(s._h).decode()

    with rtsn_mod.Solver(q) as s:  # a plain handle
        assert status(lambda: s.material_set_opacity_law(*law)) == 9
        assert "rt_create_regions" in message(s)
        s.material_enable(1.0)
        assert status(lambda: s.material_set_opacity_law(*law)) == 9
    with rtsn_mod.Solver(q, regions=regions) as s:  # chain mode, uncoupled and coupled
        assert s.wavefront_state()["active"]
        assert status(lambda: s.material_set_opacity_law(*law)) == 9
        assert "rt_set_wavefront" in message(s) and "rt_material_enable_segments" in message(s)
        s.material_enable_regions(rho_cv)
        assert status(lambda: s.material_set_opacity_law(*law)) == 9
        assert "chain mode" in message(s)
    with rtsn_mod.Solver(q, regions=regions) as s:  # segment mode
        _segment_mode(s, 4, cells=16)
        assert status(lambda: s.material_set_opacity_law(*law)) == 9  # uncoupled
        assert "rt_material_enable_segments first" in message(s)
        assert status(lambda: s.opacity_scale()) == 9
        s.material_enable_segments(rho_cv, T0)
        assert np.array_equal(s.opacity_scale(), np.ones(s.N))  # the law off
        n, tr = law[0], law[1]
        assert status(lambda: s.material_set_opacity_law(n[:1], tr[:1], 1e-3, 1e3)) == 8
        assert status(lambda: s.material_set_opacity_law(list(n) + [1.0], list(tr) + [1.0], 1e-3, 1e3)) == 8
        dp = np.zeros(2)
        assert L.rt_material_set_opacity_law(s._h, None, dp.ctypes.data_as(L.rt_get_opacity_scale.argtypes[1]), 2,
                                             1e-3, 1e3) == 8
        for bad in (0.0, -1.0, float("nan"), float("inf")):
            assert status(lambda: s.material_set_opacity_law(n, [tr[0], bad], 1e-3, 1e3)) == 8
        for bad in (float("nan"), float("inf"), -float("inf")):
            assert status(lambda: s.material_set_opacity_law([n[0], bad], tr, 1e-3, 1e3)) == 8
        for lo, hi in ((0.0, 1.0), (-1.0, 1.0), (2.0, 1.0), (1.0, float("inf")), (float("nan"), 1.0),
                       (1.0, float("nan"))):
            assert status(lambda: s.material_set_opacity_law(n, tr, lo, hi)) == 8
        assert np.array_equal(s.opacity_scale(), np.ones(s.N))  # a refused call changes nothing
        s.material_set_opacity_law(None, None, 0.0, 0.0)  # off while off: accepted
        s.material_set_opacity_law(n, tr, 1.0, 1.0)  # scale_min == scale_max is allowed
        assert np.array_equal(s.opacity_scale(), np.ones(s.N))
        s.material_set_opacity_law(*law)
        # one launch per coupled sweep with the law on
        s.set_profiling(True)
        n0 = s.sweep_time()[1]
        s.material_sweep()
        s.material_update()
        assert s.sweep_time()[1] == n0 + 1
        s.set_profiling(False)
        assert np.isfinite(s.ends()).all()


# ---------------------------------------------------------------------------
# 8: against extended precision
# ---------------------------------------------------------------------------
def _regime_points():
    from test_opacity_law import REGIME_POINTS
    return REGIME_POINTS


def _needs_extended():
    import regime_cases as rc
    return pytest.mark.skipif(not rc.HAVE_EXTENDED, reason=rc.SKIP_REASON)


@_needs_extended()
@pytest.mark.parametrize("pt", _regime_points(), ids=lambda pt: f"{pt[0]}-{pt[1]:g}-n{pt[2]:g}")
def test_regime_against_extended_precision(rtsn_mod, oracle_mod, pt):
    """The (16, 32, 16) slab of tests/material_regime_cases.py with the law on every region:
    E(gpu) <= K max(E(fp64 reference), 16 eps), K = 32, by the project's own metrics (T per cell,
    ends per line, Beff per group and decade, transit)."""
    import material_regime_cases as mc
    from test_opacity_law import law_regime_case
    case, law = law_regime_case(oracle_mod, pt)
    with rtsn_mod.Solver(case.q, regions=case.regions) as s:
        _segment_mode(s, 4, cells=16)
        s.material_enable_segments(case.rho_cv, case.T0)
        s.material_set_opacity_law(*law)
        coupled_steps(s, case.steps)
        ratios = mc.coupled_ratios(mc.coupled_readouts(s), case)
    print(pt, {k: float(np.max(v)) for k, v in ratios.items()})
    for k, v in ratios.items():
        mc.assert_bound(v, f"{pt} {k}")
