"""The tabulated internal energy e(T) of the material coupling on the GPU
(rt_material_set_energy_table; kernels.hip material_energy and the EOS forms of
material_update_kernel).

* parity with the fp64 restatement tests/heat_capacity_ref.py (test_material_gpu.compare: T 1e-12,
  the rest 1e-10) over 6 steps: a plain handle (N = 32, one region's table), a region handle in
  chain mode on (16, 16) cells, in segment mode on (32, 48) and (16, 16) cells for BE / CN / BDF2 and
  the boundary pairs (0,0), (2,1), (1,1), with the opacity law `marshak` and with the opacity table
  `edge` once per scheme; the path every cell took in the last update (rt_get_material_last_dt: 0
  where the full emission was solved) against the reference's, where the reference's dT / T is not
  within 1e-9 of 1/4;
* material_energy() and heat_capacity() against the table's rule stated in long double
  (test_heat_capacity.probe_rule) at 1e-14, at probes below the first node (one T < 0, one T = 0:
  rt_material_enable* admits them), on the nodes, one ulp beside the interior ones, above the last;
* BE energy on the device at 1e-12 per step with e(T) in the statement, with and without the law;
* the table c x T_grid against the device's own constant-rho_cv run (not bitwise); e ~ T^4 as a
  two-node and as a five-node table against each other;
* bitwise: set and cleared before any step; chain against segment mode; material_step against
  sweep + update;
* group shards (0,2), (2,5) with [q, b] summed by the test; a table set in mid-run; the stability
  number; the statuses and their messages;
* one family against the reference in np.longdouble (test_opacity_table.table_regime_case's slab,
  rule and margins).

The conditions the cases rest on are asserted on the reference alone in tests/test_heat_capacity.py.
"""
from __future__ import annotations

import numpy as np
import pytest

import heat_capacity_ref as hcr
import opacity_law_ref as olr
import opacity_table_ref as otr
from test_material import net_outflow
from test_material_gpu import GpuView, compare, to_rt
from test_opacity_law_gpu import _AsReference
from test_regions_material_gpu import _coupled_readouts, coupled_steps
from test_regions_segments_gpu import _segment_mode, _status

pytestmark = pytest.mark.gpu


def _open(rtsn_mod, oracle_mod, layout, ts, bc, mode="segment", law=None, table=None, energy=True, **shard):
    """A coupled handle of a layout with its energy table set: mode "segment" (16 cells per
    segment), "chain", or layout "plain" (one medium, region 0's row)."""
    if layout == "plain":
        p, _, rho_cv, T0 = hcr.plain_case(oracle_mod, ts, bc)
        s = rtsn_mod.Solver(to_rt(p), **shard)
    else:
        p, regions, rho_cv, T0 = hcr.case(oracle_mod, layout, ts, bc)
        s = rtsn_mod.Solver(to_rt(p), regions=regions, **shard)
    try:
        if layout == "plain":
            s.material_enable(rho_cv, T0)
        elif mode == "chain":
            assert s.wavefront_state()["active"]
            s.material_enable_regions(rho_cv, T0)
        else:
            L = olr.LAYOUTS[layout]
            assert _segment_mode(s, 4, cells=L["seg"]) == L["segments"]
            s.material_enable_segments(rho_cv, T0)
        if law:
            s.material_set_opacity_law(*olr.law_args(law))
        if table:
            s.material_set_opacity_table(*otr.table_args(table, p["G"]))
        if energy:
            s.material_set_energy_table(*hcr.energy_table(layout, 1 if layout == "plain" else 2))
    except BaseException:
        s.close()
        raise
    return s, p


def _paths(s, ref):
    """The path each cell took in the last update, where the reference's dT / T is clear of 1/4 --
    and of 0: a cell deep in the cold region whose linear dT is below an ulp of T also reads 0."""
    h = ref.history[-1]
    clear = (np.abs(h["ratio"] - 0.25) > 1e-9) & (np.abs(h["ratio"]) > 1e-12)
    assert clear.sum() >= ref.N // 2
    got = s.material_last_dT() == 0.0
    assert np.array_equal(got[clear], h["solved"][clear]), (np.flatnonzero(got != h["solved"]), h["ratio"])
    return int(got.sum())


# ---------------------------------------------------------------------------
# 1: parity with the reference
# ---------------------------------------------------------------------------
SEGMENT = [(lay, ts, bc) for lay in ("n80", "n32") for ts in (1, 2, 3) for bc in hcr.BCS]
ONCE = [(1, (2, 1)), (2, (0, 0)), (3, (1, 1))]   # once per scheme


@pytest.mark.parametrize("layout,ts,bc", SEGMENT, ids=lambda v: str(v).replace(" ", ""))
def test_parity_segment_mode(rtsn_mod, oracle_mod, layout, ts, bc):
    r = hcr.reference_run(oracle_mod, layout, ts, bc)
    s, _ = _open(rtsn_mod, oracle_mod, layout, ts, bc)
    with s:
        coupled_steps(s, hcr.STEPS)
        err = compare(s, r["ref"])
        print(layout, ts, bc, err, "full", _paths(s, r["ref"]))


@pytest.mark.parametrize("ts,bc", ONCE, ids=lambda v: str(v).replace(" ", ""))
def test_parity_plain_handle(rtsn_mod, oracle_mod, ts, bc):
    r = hcr.reference_run(oracle_mod, "plain", ts, bc)
    s, p = _open(rtsn_mod, oracle_mod, "plain", ts, bc)
    with s:
        assert p["N"] == 32
        s.material_step(hcr.STEPS)
        print(ts, bc, compare(s, r["ref"]), "full", _paths(s, r["ref"]))


@pytest.mark.parametrize("ts,bc", ONCE, ids=lambda v: str(v).replace(" ", ""))
def test_parity_chain_mode(rtsn_mod, oracle_mod, ts, bc):
    r = hcr.reference_run(oracle_mod, "n32", ts, bc)
    s, _ = _open(rtsn_mod, oracle_mod, "n32", ts, bc, mode="chain")
    with s:
        coupled_steps(s, hcr.STEPS)
        assert s.wavefront_state()["active"]
        print(ts, bc, compare(s, r["ref"]), "full", _paths(s, r["ref"]))


@pytest.mark.parametrize("ts,bc", ONCE, ids=lambda v: str(v).replace(" ", ""))
def test_parity_with_the_opacity_law(rtsn_mod, oracle_mod, ts, bc):
    r = hcr.reference_run(oracle_mod, "n80", ts, bc, law="marshak")
    s, _ = _open(rtsn_mod, oracle_mod, "n80", ts, bc, law="marshak")
    with s:
        coupled_steps(s, hcr.STEPS)
        print(ts, bc, compare(s, r["ref"]), "full", _paths(s, r["ref"]))


@pytest.mark.parametrize("ts,bc", ONCE, ids=lambda v: str(v).replace(" ", ""))
def test_parity_with_the_opacity_table(rtsn_mod, oracle_mod, ts, bc):
    r = hcr.reference_run(oracle_mod, "n80", ts, bc, table="edge")
    s, _ = _open(rtsn_mod, oracle_mod, "n80", ts, bc, table="edge")
    with s:
        coupled_steps(s, hcr.STEPS)
        print(ts, bc, compare(s, r["ref"]), "full", _paths(s, r["ref"]))


# ---------------------------------------------------------------------------
# 2: the read-outs against the rule
# ---------------------------------------------------------------------------
def test_probe_temperatures(rtsn_mod, oracle_mod):
    """T0 = the probes of test_heat_capacity.probe_temperatures, T < 0 and T = 0 among them (the
    enable calls admit any T_cells), every probe in either region: e and c_v from the device's own
    material_energy() against the rule in long double at 1e-14; e(0) = 0 exactly."""
    from test_heat_capacity import probe_rule, probe_temperatures
    p, regions, rho_cv, _ = hcr.case(oracle_mod, "n32", 1, (0, 0))
    Tg, en = hcr.energy_table("n32")
    probes = probe_temperatures(Tg)
    assert probes.size <= 32 and (probes < 0).any() and (probes == 0).any()
    for shift in (0, 16):
        T0 = np.roll(np.resize(probes, p["N"]), shift)
        with rtsn_mod.Solver(to_rt(p), regions=regions) as s:
            _segment_mode(s, 4, cells=16)
            s.material_enable_segments(rho_cv, T0)
            assert np.array_equal(s.heat_capacity(), np.repeat(rho_cv, 16))          # no table yet
            assert np.array_equal(s.material_energy(), np.repeat(rho_cv, 16) * T0)
            s.material_set_energy_table(Tg, en)
            e, cv = s.material_energy(), s.heat_capacity()
        we, wc = probe_rule(Tg, en, T0, np.repeat([0, 1], 16))
        err_e = float(np.max(np.abs(e - we) / np.maximum(np.abs(we), 1e-300)))
        err_c = float(np.max(np.abs(cv - wc) / wc))
        print(shift, err_e, err_c)
        assert err_e <= 1e-14 and err_c <= 1e-14
        assert (e[T0 == 0.0] == 0.0).all()


# ---------------------------------------------------------------------------
# 3: energy, BE
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("law", [None, "marshak"])
@pytest.mark.parametrize("bc", hcr.BCS)
def test_backward_euler_energy_on_device(rtsn_mod, oracle_mod, bc, law):
    """Per step on (32, 48): the change of sum_x dx(x) (sum_g phi_g / c + e(T(x)) + transit) plus
    dt x the net boundary outflow is at most 1e-12 of the total; T > 0 and Beff >= 0."""
    s, p = _open(rtsn_mod, oracle_mod, "n80", 1, bc, law=law)
    dx = np.repeat(olr.DXS, olr.LAYOUTS["n80"]["cells"])
    with s:
        for n in range(hcr.STEPS):
            e0 = hcr.energy(s, dx)
            s.material_step(1)
            e1 = hcr.energy(s, dx)
            resid = (e1 - e0) + p["dt"] * net_outflow(GpuView(s), p)
            print(bc, law, n, resid / e1)
            assert abs(resid) <= 1e-12 * abs(e1), (n, resid, e1)
            assert (s.temperature() > 0).all() and (s.cell_emission() >= 0).all()


# ---------------------------------------------------------------------------
# 4, 5: the constant heat capacity and the power law as tables
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("ts", [1, 3])
def test_linear_table_is_the_constant_heat_capacity(rtsn_mod, oracle_mod, ts):
    """energy = c x T_grid against the device's own run enabled with rho_cv = c, at compare's
    tolerances.  NOT bitwise: the table's e(T) goes through log and exp, its linear-emission step is
    a root solve stopped at 1e-15 where the constant-rho_cv form is one division, and e(T') - e(T)
    is a difference of two rounded energies where rho_cv (T' - T) is one product."""
    bc, c = (2, 1), (5.0, 0.5)
    Tg = hcr.energy_table("n80")[0]
    const, _ = _open(rtsn_mod, oracle_mod, "n80", ts, bc, energy=False)
    s, _ = _open(rtsn_mod, oracle_mod, "n80", ts, bc, energy=False)
    with const, s:
        assert olr.RHO_CV == c
        s.material_set_energy_table(Tg, np.outer(c, Tg))
        np.testing.assert_allclose(s.heat_capacity(), const.heat_capacity(), rtol=1e-14)
        coupled_steps(const, hcr.STEPS)
        coupled_steps(s, hcr.STEPS)
        print(ts, compare(s, _AsReference(const)))
        assert (s.material_last_dT() == 0).sum() == (const.material_last_dT() == 0).sum() > 0
        np.testing.assert_allclose(s.material_energy(), const.material_energy(), rtol=1e-12)


@pytest.mark.parametrize("ts", [1, 3])
def test_power_law_as_two_and_as_five_nodes(rtsn_mod, oracle_mod, ts):
    """e = a_k T^4 (c_v ~ T^3) as a two-node table and as a five-node table on the same curve,
    against each other at compare's tolerances."""
    bc, a = (2, 1), np.array([2.0, 0.3])
    two = np.array([0.01, 1.0])
    five = np.array([0.01, 0.07, 0.3, 0.9, 3.0])
    a2, _ = _open(rtsn_mod, oracle_mod, "n80", ts, bc, energy=False)
    a5, _ = _open(rtsn_mod, oracle_mod, "n80", ts, bc, energy=False)
    with a2, a5:
        for s, Tg in ((a2, two), (a5, five)):
            s.material_set_energy_table(Tg, a[:, None] * Tg[None, :] ** 4)
            T0 = s.temperature()
            np.testing.assert_allclose(s.heat_capacity(), 4.0 * np.repeat(a, (32, 48)) * T0 ** 3, rtol=1e-14)
            np.testing.assert_allclose(s.material_energy(), np.repeat(a, (32, 48)) * T0 ** 4, rtol=1e-14)
            coupled_steps(s, hcr.STEPS)
        print(ts, compare(a5, _AsReference(a2)))
        assert (a5.material_last_dT() == 0).sum() == (a2.material_last_dT() == 0).sum() > 0


# ---------------------------------------------------------------------------
# 6: bitwise
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("layout,ts", [("n80", 1), ("n80", 3), ("plain", 3)])
def test_set_and_cleared_before_any_step_is_bitwise(rtsn_mod, oracle_mod, layout, ts):
    bc = (2, 1)
    plain, _ = _open(rtsn_mod, oracle_mod, layout, ts, bc, energy=False)
    with plain:
        plain.material_step(4)
        want = _coupled_readouts(plain)
    s, _ = _open(rtsn_mod, oracle_mod, layout, ts, bc)
    with s:
        cv = s.heat_capacity()
        s.material_set_energy_table(None, None)
        assert not np.array_equal(cv, s.heat_capacity())
        s.material_step(4)
        got = _coupled_readouts(s)
    for k, v in want.items():
        assert np.array_equal(got[k], v), k


@pytest.mark.parametrize("ts", [1, 3])
def test_chain_against_segment_mode_bitwise(rtsn_mod, oracle_mod, ts):
    """The update does not know the mode: (16, 16) cells with the same table, every read-out."""
    bc = (2, 1)
    runs = []
    for mode in ("chain", "segment"):
        s, _ = _open(rtsn_mod, oracle_mod, "n32", ts, bc, mode=mode)
        with s:
            coupled_steps(s, hcr.STEPS)
            runs.append(dict(_coupled_readouts(s), e=s.material_energy(), cv=s.heat_capacity(), dT=s.material_last_dT()))
    for k, v in runs[0].items():
        assert np.array_equal(runs[1][k], v), k


@pytest.mark.parametrize("ts", [1, 3])
def test_material_step_against_sweep_and_update_bitwise(rtsn_mod, oracle_mod, ts):
    bc = (0, 0)
    runs = []
    for drive in (lambda s: s.material_step(hcr.STEPS), lambda s: coupled_steps(s, hcr.STEPS)):
        s, _ = _open(rtsn_mod, oracle_mod, "n80", ts, bc)
        with s:
            drive(s)
            runs.append(dict(_coupled_readouts(s), e=s.material_energy(), dT=s.material_last_dT()))
    for k, v in runs[0].items():
        assert np.array_equal(runs[1][k], v), k


# ---------------------------------------------------------------------------
# 7: group shards
# ---------------------------------------------------------------------------
def test_group_shards_on_one_gpu(rtsn_mod, oracle_mod):
    """Groups [0, 2) and [2, 5) as two handles on (32, 48), BDF2, their [q, b] summed by the test:
    every rank holds the same table and the same summed [q, b], so both end with bitwise-equal T,
    equal to the full handle's at compare's 1e-12."""
    import torch
    ts, bc = 3, (2, 1)
    full, p = _open(rtsn_mod, oracle_mod, "n80", ts, bc)
    with full:
        full.material_step(hcr.STEPS)
        T_full = full.temperature()
    shards = [_open(rtsn_mod, oracle_mod, "n80", ts, bc, g_lo=lo, g_hi=hi)[0] for lo, hi in ((0, 2), (2, 5))]
    try:
        qb = [torch.zeros(2 * p["N"], dtype=torch.float64, device="cuda") for _ in shards]
        for _ in range(hcr.STEPS):
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
        T = [s.temperature() for s in shards]
        assert np.array_equal(T[0], T[1])
        assert np.array_equal(shards[0].material_energy(), shards[1].material_energy())
        err = float(np.max(np.abs(T[0] - T_full) / np.abs(T_full)))
        print(err)
        assert err <= 1e-12
    finally:
        for s in shards:
            s.close()


# ---------------------------------------------------------------------------
# 8: a table set in mid-run
# ---------------------------------------------------------------------------
def test_table_set_in_mid_run(rtsn_mod, oracle_mod):
    """BE on (32, 48): three steps with the constant rho_cv, the table set, three more.  T(x) is
    bitwise unchanged by the call (and by clearing it), the BE residual with the new e(T) holds at
    1e-12 from the next step on, the run equals the reference driven the same way, and cleared
    again heat_capacity() is rho_cv."""
    bc = (2, 1)
    s, p = _open(rtsn_mod, oracle_mod, "n80", 1, bc, energy=False)
    _, regions, rho_cv, T0 = hcr.case(oracle_mod, "n80", 1, bc)
    ref = hcr.HeatCapacityReference(oracle_mod, p, regions, rho_cv, T0)
    dx, rcv = ref.dx_cells, np.repeat(rho_cv, (32, 48))
    tab = hcr.energy_table("n80")
    with s:
        s.material_step(3)
        ref.material_step(3)
        T, tr, Beff = s.temperature(), s.material_transit(), s.cell_emission()
        assert np.abs(tr).max() > 0.0
        s.material_set_energy_table(*tab)
        ref.set_energy_table(*tab)
        assert np.array_equal(s.temperature(), T) and np.array_equal(s.material_transit(), tr)
        assert np.array_equal(s.cell_emission(), Beff)
        assert not np.array_equal(s.heat_capacity(), rcv)
        for n in range(3):
            e0 = hcr.energy(s, dx)
            s.material_step(1)
            ref.material_step(1)
            e1 = hcr.energy(s, dx)
            resid = (e1 - e0) + p["dt"] * net_outflow(GpuView(s), p)
            print(n, resid / e1)
            assert abs(resid) <= 1e-12 * abs(e1), (n, resid, e1)
        print(compare(s, ref))
        T = s.temperature()
        s.material_set_energy_table(None, None)
        assert np.array_equal(s.temperature(), T)
        assert np.array_equal(s.heat_capacity(), rcv) and np.array_equal(s.material_energy(), rcv * T)


# ---------------------------------------------------------------------------
# 9: the stability number
# ---------------------------------------------------------------------------
def test_material_stability_uses_the_heat_capacity_of_the_hottest_cell(rtsn_mod, oracle_mod):
    """number x c_v at each region's hottest cell is the table-free number x rho_cv there: the
    largest over the regions, with c_v from the reference."""
    bc = (2, 1)
    s, p = _open(rtsn_mod, oracle_mod, "n80", 1, bc, energy=False)
    _, regions, rho_cv, T0 = hcr.case(oracle_mod, "n80", 1, bc)
    ref = hcr.HeatCapacityReference(oracle_mod, p, regions, rho_cv, T0, energy_table=hcr.energy_table("n80"))
    with s:
        per_region = []
        for k in range(2):   # region k's own number: the other region made far stiffer in rho_cv
            with rtsn_mod.Solver(to_rt(p), regions=regions) as u:
                _segment_mode(u, 4, cells=16)
                rc = [1e30, 1e30]
                rc[k] = rho_cv[k]
                per_region.append(u.material_enable_segments(rc, T0) * rho_cv[k])
        assert s.material_stability() == pytest.approx(max(n / c for n, c in zip(per_region, rho_cv)), rel=1e-13)
        s.material_set_energy_table(*hcr.energy_table("n80"))
        cv = np.asarray(ref.heat_capacity())
        hot = [int(np.argmax(np.where(ref.cell_region == k, T0, -np.inf))) for k in range(2)]
        want = max(per_region[k] / cv[hot[k]] for k in range(2))
        assert s.material_stability() == pytest.approx(want, rel=1e-13)
        np.testing.assert_allclose(s.heat_capacity()[hot], cv[hot], rtol=1e-14)


# ---------------------------------------------------------------------------
# 10: the statuses
# ---------------------------------------------------------------------------
def test_statuses(rtsn_mod, oracle_mod):
    p, regions, rho_cv, T0 = hcr.case(oracle_mod, "n80", 3, (0, 0))
    q = to_rt(p)
    L = rtsn_mod.lib()
    Tg, en = hcr.energy_table("n80")

    def status(fn):
        return _status(rtsn_mod, fn)

    def message(s):
        return L.rt_last_error(s._h).decode()

    with rtsn_mod.Solver(q) as s:  # a plain handle: uncoupled, then one region's row
        assert status(lambda: s.material_set_energy_table(Tg, en[:1])) == 9
        assert "rt_material_enable first" in message(s)
        assert status(lambda: s.material_energy()) == 9 and status(lambda: s.heat_capacity()) == 9
        s.material_enable(1.5)
        assert status(lambda: s.material_set_energy_table(Tg, en)) == 8   # two rows on a handle without regions
        assert "nregions must be the handle's 1" in message(s)
        s.material_set_energy_table(Tg, en[0])
        assert (s.heat_capacity() != 1.5).all()
        s.material_enable(1.5)                                            # enabled again: the table is cleared
        assert np.array_equal(s.heat_capacity(), np.full(s.N, 1.5))
    with rtsn_mod.Solver(q, regions=regions) as s:  # chain mode
        assert status(lambda: s.material_set_energy_table(Tg, en)) == 9
        s.material_enable_regions(rho_cv, T0)
        s.material_set_energy_table(Tg, en)
        s.material_set_energy_table(None, None)
        s.material_set_energy_table(None, None)      # off while off: accepted
        dp = L.rt_get_heat_capacity.argtypes[1]
        tg, enc = np.ascontiguousarray(Tg), np.ascontiguousarray(en)
        raw = L.rt_material_set_energy_table
        for args, text in (((tg.ctypes.data_as(dp), 4, enc.ctypes.data_as(dp), 1), "nregions must be the handle's 2"),
                           ((tg.ctypes.data_as(dp), 4, enc.ctypes.data_as(dp), 3), "nregions must be the handle's 2"),
                           ((tg.ctypes.data_as(dp), 1, enc.ctypes.data_as(dp), 2), "at least 2 nodes"),
                           ((None, 4, enc.ctypes.data_as(dp), 2), "NULL T_grid or energy"),
                           ((tg.ctypes.data_as(dp), 4, None, 2), "NULL T_grid or energy"),
                           ((None, 0, None, 2), "NULL T_grid or energy")):
            assert raw(s._h, *args) == 8, text
            assert text in message(s), (text, message(s))
        for j, bad in ((1, Tg[0]), (1, 0.5 * Tg[0]), (0, 0.0), (0, -1.0), (2, float("nan")), (3, float("inf"))):
            g = Tg.copy()
            g[j] = bad
            assert status(lambda: s.material_set_energy_table(g, en)) == 8, (j, bad)
            assert "T_grid must be finite, > 0 and strictly increasing" in message(s)
        for bad in (0.0, -1.0, float("nan"), float("inf")):
            c = en.copy()
            c[1, 3] = bad
            assert status(lambda: s.material_set_energy_table(Tg, c)) == 8, bad
            assert "every energy entry must be finite and > 0" in message(s)
        for j, bad in ((2, en[1, 1]), (2, 0.5 * en[1, 1]), (0, 2.0 * en[1, 1])):
            c = en.copy()
            c[1, j] = bad
            assert status(lambda: s.material_set_energy_table(Tg, c)) == 8, (j, bad)
            assert "strictly increasing along T_grid" in message(s)
        assert np.array_equal(s.heat_capacity(), np.repeat(rho_cv, (32, 48)))   # a refused call changes nothing


# ---------------------------------------------------------------------------
# 11: against extended precision
# ---------------------------------------------------------------------------
_regime = {}
REGIME_GRID = (0.5, 0.85, 0.95, 3.2, 8.5, 12.0)
REGIME_EXPONENTS = (1.5, 2.5, 4.0, 2.0, 1.0)


def energy_regime_case(oracle_mod, pt):
    """test_opacity_table.table_regime_case's slab, start and rho_cv with an energy table per region
    in place of the opacity table: nodes among the start's temperatures (0.81 to 0.99, 3.0 to 3.3,
    8.1 to 9.0 keV), so that cells of one region lie in different brackets, e = rho_cv_k T at the first
    node and the exponents (1.5, 2.5, 4, 2, 1) per bracket from there.  The truth in np.longdouble, the
    fp64 reference beside it.  (CoupledCase, the table)."""
    if pt in _regime:
        return _regime[pt]
    import material_regime_cases as mc
    import regime_cases as rc
    from test_opacity_table import table_regime_case
    base, _ = table_regime_case(oracle_mod, pt)
    p, regions, rho_cv, T0 = base.p, base.regions, base.rho_cv, base.T0
    Tg = np.array(REGIME_GRID)
    assert len(set(np.searchsorted(Tg, T0).tolist())) >= 5 and T0.min() > Tg[0]   # the start holds five brackets
    _, en = hcr.power_nodes(Tg, [c * Tg[0] for c in rho_cv], [REGIME_EXPONENTS] * len(regions))
    table = (Tg, en)
    truth = hcr.HeatCapacityReference(oracle_mod, p, regions, rho_cv, T0, dtype=np.longdouble, energy_table=table)
    stiff0 = np.asarray(p["dt"] * truth.W * truth.bpart / truth.heat_capacity(), dtype=np.float64)
    truth.material_step(mc.STEPS)
    ref = hcr.HeatCapacityReference(oracle_mod, p, regions, rho_cv, T0, energy_table=table)
    ref.material_step(mc.STEPS)
    same = all(np.array_equal(a["solved"], b["solved"]) for a, b in zip(ref.history, truth.history))
    tr = mc.coupled_readouts(truth)
    Tn = np.asarray(tr["T"], dtype=np.float64)
    W = float(truth.W)
    w_sigma = p["dt"] * W * np.asarray(truth.sigma_cells, dtype=np.float64)
    e = truth.e_edge
    case = mc.CoupledCase(p, rc.to_rt(p), regions, rho_cv, T0, mc.STEPS, tr, mc.coupled_readouts(ref),
                          {"slab": np.arange(p["N"])}, mc.rounding_floor(Tn, e, 0, rc.G), w_sigma, truth.history, same,
                          stiff0)
    _regime[pt] = (case, table)
    return _regime[pt]


def _needs_extended():
    import regime_cases as rc
    return pytest.mark.skipif(not rc.HAVE_EXTENDED, reason=rc.SKIP_REASON)


@_needs_extended()
@pytest.mark.parametrize("pt", [(1, 1.0), (2, 1.0), (3, 1.0), (1, 1e2), (3, 1e-2)], ids=lambda pt: f"{pt[0]}-{pt[1]:g}")
def test_regime_against_extended_precision(rtsn_mod, oracle_mod, pt):
    """E(gpu) <= K max(E(fp64 reference), 16 eps), K = 32, by the project's own metrics (T per cell,
    ends per line, Beff per group and decade, transit), where the fp64 reference takes the truth's
    branches; the device's error is judged beside the reference's own against the same truth."""
    import material_regime_cases as mc
    case, table = energy_regime_case(oracle_mod, pt)
    assert case.branch_same
    with rtsn_mod.Solver(case.q, regions=case.regions) as s:
        _segment_mode(s, 4, cells=16)
        s.material_enable_segments(case.rho_cv, case.T0)
        s.material_set_energy_table(*table)
        coupled_steps(s, case.steps)
        ratios = mc.coupled_ratios(mc.coupled_readouts(s), case)
    print(pt, {k: float(np.max(v)) for k, v in ratios.items()})
    for k, v in ratios.items():
        mc.assert_bound(v, f"{pt} {k}")
