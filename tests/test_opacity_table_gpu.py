"""Tabulated per-group opacities of the material coupling on the GPU
(rt_material_set_opacity_table; kernels.hip opacity_table_kernel and the table forms of the law
walk and of the material kernels).

* parity with the fp64 restatement tests/opacity_table_ref.py (test_material_gpu.compare: T 1e-12,
  the rest 1e-10) over 6 steps: the table `edge` on (32, 48) and (16, 16) cells, BE / CN / BDF2,
  boundary pairs (0,0), (2,1), (1,1); M = 8, G = 17 (68 lines per half) and M = 2, G = 70 (more
  groups than a wave has lanes: the table kernel's group loop, a wave across a group edge) once;
* opacity_scale_groups() against the reference's expression at 1e-14 relative, at the shared T0
  and at the device's own T; probe temperatures below, above, on and one ulp beside the nodes;
* the clamped power law written as a table against the device's own power-law run;
* BE energy on the device at 1e-12 per step, also across the table set, changed, replaced by
  the law, the law replaced by the table and the table cleared in mid-run;
* independence of the segment plan and of material_step against sweep + update, bitwise; set and
  cleared before any step: bitwise the plain walk; the all-ones table against exponent 0;
* group shards (0,2), (2,5) with [q, b] summed by the test; the read-outs; the statuses;
* one family against the reference in np.longdouble (tests/test_opacity_table.py
  table_regime_case).

The conditions the cases rest on are asserted on the reference alone in tests/test_opacity_table.py.
"""
from __future__ import annotations

import numpy as np
import pytest

import opacity_law_ref as olr
import opacity_table_ref as otr
from parity import per_group_rel
from test_material import net_outflow
from test_material_gpu import GpuView, compare, to_rt
from test_opacity_law_gpu import _AsReference, _energy_terms
from test_regions_material_gpu import _coupled_readouts, coupled_steps
from test_regions_segments_gpu import _segment_mode, _status

pytestmark = pytest.mark.gpu


def _open(rtsn_mod, oracle_mod, layout, ts, bc, table=None, law=None, seg=None, segments=None, **shard):
    """A coupled segment-mode handle of a layout on its plan (seg cells per segment), the table
    (a name of opacity_table_ref.TABLES) or the law (a name of opacity_law_ref.LAWS) set."""
    p, regions, rho_cv, T0 = otr.case(oracle_mod, layout, ts, bc)
    L = otr.LAYOUTS[layout]
    s = rtsn_mod.Solver(to_rt(p), regions=regions, **shard)
    try:
        Sg = _segment_mode(s, 4, cells=seg or L["seg"])
        assert Sg == (segments or L["segments"]) and not s.wavefront_state()["active"]
        s.material_enable_segments(rho_cv, T0)
        if table:
            s.material_set_opacity_table(*otr.table_args(table, p["G"]))
        if law:
            s.material_set_opacity_law(*olr.law_args(law))
    except BaseException:
        s.close()
        raise
    return s, p


def _f_rel(s, ref):
    """opacity_scale_groups() against the reference's expression at the handle's own T(x),
    relative: the device's log, fma and exp against numpy's (test_opacity_law_gpu._f_rel's rule;
    against the reference's own f the difference carries |d ln f / d ln T| <= 3.5 + the kink's
    slope times the difference in T, which compare holds to 1e-12: asserted at 1e-11)."""
    got = s.opacity_scale_groups()
    if ref.table is None and ref.law is None:
        assert np.array_equal(got, np.ones((s.N, s.G)))
        return 0.0
    f = np.asarray(ref.opacity_scale_groups(), dtype=np.float64)
    assert np.max(np.abs(got - f) / f) <= 1e-11
    T = s.temperature().astype(ref.dtype)
    own = ref._own(np.asarray(ref._scale_table(T) if ref.table is not None else ref._scale(T), dtype=np.float64))
    return float(np.max(np.abs(got - own) / own))


# ---------------------------------------------------------------------------
# 1: parity with the reference
# ---------------------------------------------------------------------------
PARITY = [(lay, ts, bc) for lay in ("n80", "n32") for ts in (1, 2, 3) for bc in otr.BCS] + [otr.WIDE_CASE, otr.G70_CASE]


@pytest.mark.parametrize("layout,ts,bc", PARITY, ids=lambda v: str(v).replace(" ", ""))
def test_parity(rtsn_mod, oracle_mod, layout, ts, bc):
    r = otr.reference_run(oracle_mod, layout, "edge", ts, bc)
    s, p = _open(rtsn_mod, oracle_mod, layout, ts, bc, "edge")
    with s:
        if layout == "g70":
            assert p["G"] == 70 and s.G == 70
        f0 = s.opacity_scale_groups()
        err0 = float(np.max(np.abs(f0 - r["f0"]) / r["f0"]))  # the same T0: the device's expression alone
        print(layout, ts, bc, "f at T0", err0)
        assert err0 <= 1e-14
        coupled_steps(s, otr.STEPS)
        assert not s.wavefront_state()["active"]
        err = compare(s, r["ref"])
        err["f"] = _f_rel(s, r["ref"])
        print(layout, ts, bc, err)
        assert err["f"] <= 1e-14, err


def test_probe_temperatures(rtsn_mod, oracle_mod):
    """T0 placed below the first node, above the last, exactly on each node, one ulp to either
    side of the interior nodes: f against the table's rule stated in long double
    (test_opacity_table.probe_rule) at 1e-14; on and outside the end nodes f is exp(log(scale))."""
    from test_opacity_table import probe_rule, probe_temperatures
    p, regions, rho_cv, _ = otr.case(oracle_mod, "n32", 1, (0, 0))
    Tg, sc = otr.table_args("edge", p["G"])
    probes = probe_temperatures(Tg)
    probes = probes[np.isfinite(probes) & (probes > 0)]   # a handle starts from finite T > 0
    for shift in (0, 16):  # every probe in either region
        T0 = np.roll(np.resize(probes, p["N"]), shift)
        with rtsn_mod.Solver(to_rt(p), regions=regions) as s:
            _segment_mode(s, 4, cells=16)
            s.material_enable_segments(rho_cv, T0)
            s.material_set_opacity_table(Tg, sc)
            got = s.opacity_scale_groups()
        want = probe_rule(Tg, sc, T0, np.repeat([0, 1], 16))
        err = float(np.max(np.abs(got - want) / want))
        print(shift, err)
        assert err <= 1e-14


# ---------------------------------------------------------------------------
# 2: the power law as a table, and the all-ones table
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("ts", [1, 3])
def test_clamped_law_as_a_table(rtsn_mod, oracle_mod, ts):
    """`as_law` against the device's own `clamped` power-law run, compare's tolerances."""
    bc = (2, 1)
    law, _ = _open(rtsn_mod, oracle_mod, "n80", ts, bc, law="clamped")
    s, _ = _open(rtsn_mod, oracle_mod, "n80", ts, bc, "as_law")
    with law, s:
        coupled_steps(law, otr.STEPS)
        coupled_steps(s, otr.STEPS)
        print(ts, compare(s, _AsReference(law)))
        f = law.opacity_scale()
        assert np.max(np.abs(s.opacity_scale_groups() - f[:, None]) / f[:, None]) <= 1e-11
        assert np.array_equal(law.opacity_scale_groups(), np.repeat(f[:, None], s.G, axis=1))  # the broadcast f(x)


@pytest.mark.parametrize("ts", [1, 3])
def test_all_ones_table_is_exponent_zero(rtsn_mod, oracle_mod, ts):
    bc = (2, 1)
    zero, _ = _open(rtsn_mod, oracle_mod, "n80", ts, bc, law="zero")
    s, _ = _open(rtsn_mod, oracle_mod, "n80", ts, bc, "ones")
    with zero, s:
        assert np.array_equal(s.opacity_scale_groups(), np.ones((s.N, s.G)))
        coupled_steps(zero, otr.STEPS)
        coupled_steps(s, otr.STEPS)
        print(ts, compare(s, _AsReference(zero)))


# ---------------------------------------------------------------------------
# 3: energy, BE
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("bc", otr.BCS)
def test_backward_euler_energy_on_device(rtsn_mod, oracle_mod, bc):
    s, p = _open(rtsn_mod, oracle_mod, "n80", 1, bc, "edge")
    _, regions, rho_cv, _ = otr.case(oracle_mod, "n80", 1, bc)
    dx, rcv = _energy_terms(p, regions, rho_cv)
    with s:
        for n in range(otr.STEPS):
            e0 = olr.energy(s, dx, rcv)
            s.material_step(1)
            e1 = olr.energy(s, dx, rcv)
            resid = (e1 - e0) + p["dt"] * net_outflow(GpuView(s), p)
            print(bc, n, resid / e1)
            assert abs(resid) <= 1e-12 * abs(e1), (n, resid, e1)
            assert (s.temperature() > 0).all() and (s.cell_emission() >= 0).all()


class _Calls:
    """A solver under the reference's set_table / set_law names (test_opacity_table.transitions)."""

    def __init__(self, s):
        self.s = s

    def set_table(self, T_grid, scale):
        self.s.material_set_opacity_table(T_grid, scale)

    def set_law(self, *args):
        self.s.material_set_opacity_law(*args)


@pytest.mark.parametrize("bc", [(0, 0), (2, 1)])
def test_transitions_in_mid_run_conserve_energy(rtsn_mod, oracle_mod, bc):
    """BE on (32, 48): 3 steps with nothing set, so that emission is owed; then the table set,
    changed, replaced by the law, the law replaced by the table, the table cleared.  The energy
    sum is unchanged across each call at 1e-12, every later step balances at 1e-12, f follows the
    reference at 1e-14 and the run equals the reference driven the same way."""
    from test_opacity_table import transitions
    s, p = _open(rtsn_mod, oracle_mod, "n80", 1, bc)
    _, regions, rho_cv, T0 = otr.case(oracle_mod, "n80", 1, bc)
    dx, rcv = _energy_terms(p, regions, rho_cv)
    ref = otr.OpacityTableReference(oracle_mod, p, regions, rho_cv, T0)
    with s:
        s.material_step(3)
        ref.material_step(3)
        assert np.abs(s.material_transit()).max() > 0.0
        for k, call in enumerate(transitions(p["G"])):
            e0 = olr.energy(s, dx, rcv)
            call(_Calls(s))
            call(ref)
            e1 = olr.energy(s, dx, rcv)
            print(bc, k, (e1 - e0) / e1)
            assert abs(e1 - e0) <= 1e-12 * abs(e1), (k, e0, e1)
            assert _f_rel(s, ref) <= 1e-14
            for n in range(2):
                e0 = e1
                s.material_step(1)
                ref.material_step(1)
                e1 = olr.energy(s, dx, rcv)
                resid = (e1 - e0) + p["dt"] * net_outflow(GpuView(s), p)
                assert abs(resid) <= 1e-12 * abs(e1), (k, n, resid, e1)
        print(compare(s, ref))


# ---------------------------------------------------------------------------
# 4: independence of the plan and of how the steps are driven, bitwise; the table off
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("bc", [(0, 0), (2, 1)])
def test_independence_bitwise(rtsn_mod, oracle_mod, bc):
    """BDF2 on (32, 48) with `edge`, 6 steps: plans of 2, 3 and 5 segments (targets 48, 32, 16)
    and material_step(6) against 6 x (material_sweep, material_update): every read-out and f
    array_equal."""

    def run(seg, segments, drive):
        s, _ = _open(rtsn_mod, oracle_mod, "n80", 3, bc, "edge", seg=seg, segments=segments)
        with s:
            drive(s)
            return dict(_coupled_readouts(s), f=s.opacity_scale_groups())

    first = run(16, 5, lambda s: coupled_steps(s, 6))
    variants = [(48, 2, lambda s: coupled_steps(s, 6)), (32, 3, lambda s: coupled_steps(s, 6)),
                (16, 5, lambda s: s.material_step(6)), (32, 3, lambda s: s.material_step(6))]
    for n, v in enumerate(variants):
        got = run(*v)
        for k, want in first.items():
            assert np.array_equal(got[k], want), (k, n, v[:2])


@pytest.mark.parametrize("ts", [1, 3])
def test_set_and_cleared_before_any_step_is_the_plain_walk_bitwise(rtsn_mod, oracle_mod, ts):
    bc = (2, 1)
    plain, _ = _open(rtsn_mod, oracle_mod, "n80", ts, bc)
    with plain:
        coupled_steps(plain, 4)
        want = _coupled_readouts(plain)
    s, _ = _open(rtsn_mod, oracle_mod, "n80", ts, bc, "edge")
    with s:
        assert s.opacity_scale_groups().max() > 10.0
        s.material_set_opacity_table(None, None)
        assert np.array_equal(s.opacity_scale_groups(), np.ones((s.N, s.G)))
        assert np.array_equal(s.opacity_scale(), np.ones(s.N))
        coupled_steps(s, 4)
        got = _coupled_readouts(s)
    for k, v in want.items():
        assert np.array_equal(got[k], v), k


# ---------------------------------------------------------------------------
# 5: group shards
# ---------------------------------------------------------------------------
def test_group_shards_on_one_gpu(rtsn_mod, oracle_mod):
    """Groups [0, 2) and [2, 5) as two handles on (32, 48), reflective, BDF2, `edge` (every group
    its own f: a missed g_lo offset into the all-G table shows), their [q, b] summed by the test,
    6 steps: T equals the full handle's at rtol 1e-12, f at 1e-11, psi at 1e-10 per group."""
    import torch
    ts, bc = 3, (2, 1)
    full, p = _open(rtsn_mod, oracle_mod, "n80", ts, bc, "edge")
    with full:
        full.material_step(otr.STEPS)
        T_full, psi_full, f_full = full.temperature(), full.psi(), full.opacity_scale_groups()
    bounds = ((0, 2), (2, 5))
    shards = [_open(rtsn_mod, oracle_mod, "n80", ts, bc, "edge", g_lo=lo, g_hi=hi)[0] for lo, hi in bounds]
    try:
        qb = [torch.zeros(2 * p["N"], dtype=torch.float64, device="cuda") for _ in shards]
        for _ in range(otr.STEPS):
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
        for s, (lo, hi) in zip(shards, bounds):
            np.testing.assert_allclose(s.temperature(), T_full, rtol=1e-12)
            np.testing.assert_allclose(s.opacity_scale_groups(), f_full[:, lo:hi], rtol=1e-11)
        psi = np.concatenate([s.psi() for s in shards], axis=1)
        assert per_group_rel(psi, psi_full, 1) <= 1e-10
    finally:
        for s in shards:
            s.close()


# ---------------------------------------------------------------------------
# 6: read-outs
# ---------------------------------------------------------------------------
def test_readouts(rtsn_mod, oracle_mod):
    """rt_group_absorption_device against the reference's sum_g sigma0_g f_g phi_g at 1e-10 (the
    transit is compare's); rt_material_stability of a one-region slab against the sum with f_g
    at the hottest cell inside it."""
    import torch
    r = otr.reference_run(oracle_mod, "n80", "edge", 1, (2, 1))
    s, p = _open(rtsn_mod, oracle_mod, "n80", 1, (2, 1), "edge")
    with s:
        coupled_steps(s, otr.STEPS)
        out = torch.zeros(p["N"], dtype=torch.float64, device="cuda")
        s.group_absorption(out)
        s.synchronize()
        want = r["ref"].group_absorption()
        assert np.abs(out.cpu().numpy() - want).max() <= 1e-10 * np.abs(want).max()
        tr = r["ref"].material_transit()
        assert np.abs(s.material_transit() - tr).max() <= 1e-10 * np.abs(tr).max()
    q = otr.case(oracle_mod, "n32", 1, (0, 0))[0]
    G = q["G"]
    one = [dict(cells=32, width=32 * 0.004, rho=10.0, kappa_grey=q["kappa_grey"], T=0.5, group_kappa=None)]
    T0 = np.linspace(0.2, 0.8, 32)
    Tg = np.array([0.1, 0.4, 1.0])
    with rtsn_mod.Solver(to_rt(q), regions=one) as u:
        _segment_mode(u, 4, cells=16)
        u.material_enable_segments([0.5], T0)
        # f_g = c_g at every node: the number is linear in c, so two tables give it per group
        numbers = []
        for g in range(G):
            sc = np.ones((1, 3, G))
            sc[0, :, g] = 3.0
            u.material_set_opacity_table(Tg, sc)
            numbers.append(u.material_stability())
        u.material_set_opacity_table(Tg, np.ones((1, 3, G)))
        base = u.material_stability()
        share = (np.array(numbers) - base) / 2.0           # group g's share of the all-ones number
        assert share.sum() == pytest.approx(base, rel=1e-12)
        n = np.linspace(2.0, 0.0, G)
        sc = (Tg[None, :, None] / 0.4) ** (-n[None, None, :])
        u.material_set_opacity_table(Tg, sc)
        f_hot = (0.8 / 0.4) ** (-n)                          # T_max = 0.8, between nodes 0.4 and 1.0
        assert u.material_stability() == pytest.approx(float((share * f_hot).sum()), rel=1e-12)
        assert np.max(np.abs(u.opacity_scale_groups() / (T0[:, None] / 0.4) ** (-n[None, :]) - 1.0)) <= 1e-14
        u.material_step(2)
        assert np.isfinite(u.ends()).all() and (u.temperature() > 0).all()


# ---------------------------------------------------------------------------
# 7: the statuses
# ---------------------------------------------------------------------------
def test_statuses(rtsn_mod, oracle_mod):
    p, regions, rho_cv, T0 = otr.case(oracle_mod, "n80", 3, (0, 0))
    q = to_rt(p)
    L = rtsn_mod.lib()
    Tg, sc = otr.table_args("edge", p["G"])

    def status(fn):
        return _status(rtsn_mod, fn)

    def message(s):
        return L.rt_last_error(s._h).decode()

    with rtsn_mod.Solver(q) as s:  # a plain handle
        assert status(lambda: s.material_set_opacity_table(Tg, sc)) == 9
        assert "rt_create_regions" in message(s)
        s.material_enable(1.0)
        assert status(lambda: s.material_set_opacity_table(Tg, sc)) == 9
    with rtsn_mod.Solver(q, regions=regions) as s:  # chain mode, uncoupled and coupled
        assert status(lambda: s.material_set_opacity_table(Tg, sc)) == 9
        assert "rt_set_wavefront" in message(s) and "rt_material_enable_segments" in message(s)
        s.material_enable_regions(rho_cv)
        assert status(lambda: s.material_set_opacity_table(Tg, sc)) == 9
        assert "chain mode" in message(s)
    with rtsn_mod.Solver(q, regions=regions) as s:  # segment mode
        _segment_mode(s, 4, cells=16)
        assert status(lambda: s.material_set_opacity_table(Tg, sc)) == 9  # uncoupled
        assert "rt_material_enable_segments first" in message(s)
        assert status(lambda: s.opacity_scale_groups()) == 9
        s.material_enable_segments(rho_cv, T0)
        ones = np.ones((s.N, s.G))
        assert np.array_equal(s.opacity_scale_groups(), ones)  # nothing set
        dp = L.rt_get_opacity_scale_groups.argtypes[1]
        tg, scc = np.ascontiguousarray(Tg), np.ascontiguousarray(sc)
        raw = L.rt_material_set_opacity_table
        assert raw(s._h, tg.ctypes.data_as(dp), 5, scc.ctypes.data_as(dp), 1) == 8   # nregions not the handle's
        assert raw(s._h, tg.ctypes.data_as(dp), 5, scc.ctypes.data_as(dp), 3) == 8
        assert raw(s._h, tg.ctypes.data_as(dp), 1, scc.ctypes.data_as(dp), 2) == 8   # nT < 2
        assert raw(s._h, None, 5, scc.ctypes.data_as(dp), 2) == 8                    # NULL arrays, not off
        assert raw(s._h, tg.ctypes.data_as(dp), 5, None, 2) == 8
        assert raw(s._h, None, 0, None, 2) == 8
        for j, bad in ((1, Tg[0]), (1, 0.5 * Tg[0]), (0, 0.0), (0, -1.0), (2, float("nan")), (4, float("inf"))):
            g = Tg.copy()
            g[j] = bad
            assert status(lambda: s.material_set_opacity_table(g, sc)) == 8, (j, bad)
        for bad in (0.0, -1.0, float("nan"), float("inf")):
            c = sc.copy()
            c[1, 4, p["G"] - 1] = bad
            assert status(lambda: s.material_set_opacity_table(Tg, c)) == 8, bad
        assert np.array_equal(s.opacity_scale_groups(), ones)  # a refused call changes nothing
        s.material_set_opacity_table(None, None)  # off while off: accepted
        s.material_set_opacity_table(Tg, sc)
        assert status(lambda: s.opacity_scale()) == 9   # one f per cell and group: the group getter
        assert "rt_get_opacity_scale_groups" in message(s)
        s.material_set_opacity_law(None, None, 1.0, 1.0)  # the law off while the table is on: the table stays
        assert s.opacity_scale_groups().max() > 10.0
        s.material_set_opacity_law(*olr.law_args("marshak"))  # the law replaces the table
        f = s.opacity_scale()
        assert np.array_equal(s.opacity_scale_groups(), np.repeat(f[:, None], s.G, axis=1))
        s.material_set_opacity_table(Tg, sc)  # ... and the table the law
        # one launch per coupled sweep with the table on
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
    from test_opacity_table import REGIME_POINTS
    return REGIME_POINTS


def _needs_extended():
    import regime_cases as rc
    return pytest.mark.skipif(not rc.HAVE_EXTENDED, reason=rc.SKIP_REASON)


@_needs_extended()
@pytest.mark.parametrize("pt", _regime_points(), ids=lambda pt: f"{pt[0]}-{pt[1]:g}")
def test_regime_against_extended_precision(rtsn_mod, oracle_mod, pt):
    """The (16, 32, 16) slab of tests/material_regime_cases.py with `edge`'s rule on every region:
    E(gpu) <= K max(E(fp64 reference), 16 eps), K = 32, by the project's own metrics (T per cell,
    ends per line, Beff per group and decade, transit)."""
    import material_regime_cases as mc
    from test_opacity_table import table_regime_case
    case, table = table_regime_case(oracle_mod, pt)
    with rtsn_mod.Solver(case.q, regions=case.regions) as s:
        _segment_mode(s, 4, cells=16)
        s.material_enable_segments(case.rho_cv, case.T0)
        s.material_set_opacity_table(*table)
        coupled_steps(s, case.steps)
        ratios = mc.coupled_ratios(mc.coupled_readouts(s), case)
    print(pt, {k: float(np.max(v)) for k, v in ratios.items()})
    for k, v in ratios.items():
        mc.assert_bound(v, f"{pt} {k}")
