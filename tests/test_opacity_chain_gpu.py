"""The temperature-dependent opacity of the material coupling in chain mode on the GPU
(rt_material_set_opacity_law_chain, rt_material_set_opacity_table_chain; kernels_wave.hip
the LAW forms of wavefront_kernel / chain_kernel, the law form of the wavefront chain).

The layouts and cases are tests/opacity_chain_cases.py's; the conditions they rest on are asserted
on the references alone in tests/test_opacity_chain.py.

 1 parity with the fp64 restatement (test_material_gpu.compare: T 1e-12, the rest 1e-10; f against
   the law at the device's own T at 1e-14), the handle in chain mode throughout;
 2 chains of several waves on (160, 176): the plan's cells per lane and every admissible override,
   the waves per chain asserted;
 3 independence of the cells per lane, of the wave cap and of how the steps are driven, bitwise;
 4 against the line walk of a segment-mode handle, at compare's tolerances (not bitwise: see the test);
 5 the law set and cleared before any step: bitwise the plain coupled chain; exponent 0: the plain
   chain within compare's tolerances;
 6 BE energy on the device at 1e-12 per step, and across a law set, changed and cleared in mid-run;
 7 the table: parity, the clamped power law as a table, BE energy across the transitions;
 8 with the energy table; 9 group shards; 10 the read-outs; 11 the statuses.
"""
from __future__ import annotations

import numpy as np
import pytest

import opacity_chain_cases as occ
import opacity_law_ref as olr
import opacity_table_ref as otr
from parity import per_group_rel
from test_material import net_outflow
from test_material_gpu import GpuView, compare, to_rt
from test_opacity_law_gpu import _AsReference
from test_opacity_law_gpu import _f_rel as _law_f_rel
from test_opacity_table_gpu import _f_rel as _table_f_rel
from test_regions_material_gpu import _coupled_readouts, coupled_steps
from test_regions_segments_gpu import _segment_mode, _status

pytestmark = pytest.mark.gpu

_ids = lambda v: str(v).replace(" ", "")  # noqa: E731


def _open(rtsn_mod, oracle_mod, layout, ts, bc, law=None, table=None, cells=0, waves=0, **shard):
    """A coupled chain-mode handle of a layout, the law (a name of opacity_law_ref.LAWS) or the table
    (a name of opacity_table_ref.TABLES) set; cells / waves: rt_set_wavefront_cells / _waves."""
    p, regions, rho_cv, T0 = occ.case(oracle_mod, layout, ts, bc)
    s = rtsn_mod.Solver(to_rt(p), regions=regions, **shard)
    try:
        assert s.wavefront_state()["active"]
        if waves:
            s.wavefront_waves = waves
        if cells:
            s.set_wavefront_cells(cells)
        s.material_enable_regions(rho_cv, T0)
        if law:
            s.material_set_opacity_law_chain(*olr.law_args(law))
        if table:
            s.material_set_opacity_table_chain(*otr.table_args(table, p["G"]))
    except BaseException:
        s.close()
        raise
    return s, p


def _open_walk(rtsn_mod, oracle_mod, layout, ts, bc, law):
    """The same case on a segment-mode handle through the existing calls (16 cells per segment)."""
    p, regions, rho_cv, T0 = occ.case(oracle_mod, layout, ts, bc)
    s = rtsn_mod.Solver(to_rt(p), regions=regions)
    try:
        _segment_mode(s, 4, cells=16)
        assert not s.wavefront_state()["active"]
        s.material_enable_segments(rho_cv, T0)
        s.material_set_opacity_law(*olr.law_args(law))
    except BaseException:
        s.close()
        raise
    return s


def _admissible(layout, bc):
    """The law chain's cells per lane that divide the layout's region edges and fit 8 waves."""
    cells = occ.LAYOUTS[layout]["cells"]
    N, out = sum(cells), []
    for C in (1, 2, 4):
        if all(c % C == 0 for c in cells) and -(-(2 if bc[0] == 2 else 1) * (N // C) // 64) <= 8:
            out.append(C)
    return out


# ---------------------------------------------------------------------------
# 1: parity with the reference
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("layout,law,ts,bc", occ.LAW_PARITY, ids=_ids)
def test_parity(rtsn_mod, oracle_mod, layout, law, ts, bc):
    r = occ.reference_run(oracle_mod, layout, law, ts, bc)
    s, p = _open(rtsn_mod, oracle_mod, layout, ts, bc, law)
    with s:
        if layout == "c12_wide":
            assert (p["M"] // 2) * p["G"] == 68
        if layout.startswith("c12"):
            assert s.wavefront_state()["cells_per_lane"] == 1 and s.wavefront_state()["waves"] == 1
        assert np.max(np.abs(s.opacity_scale() - r["f0"]) / r["f0"]) <= 1e-14  # the same T0: the device pow alone
        for _ in range(occ.STEPS):
            coupled_steps(s, 1)
            assert s.wavefront_state()["active"]
        err = compare(s, r["ref"])
        err["f"] = _law_f_rel(s, r["ref"])
        print(layout, law, ts, bc, err)
        assert err["f"] <= 1e-14, err


# ---------------------------------------------------------------------------
# 2: chains of several waves
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("layout,law,ts,bc", occ.MULTI_WAVE, ids=_ids)
def test_multi_wave_chains(rtsn_mod, oracle_mod, layout, law, ts, bc):
    r = occ.reference_run(oracle_mod, layout, law, ts, bc)
    refl = bc[0] == 2
    want_waves = {1: 6, 2: 6 if refl else 3, 4: 3 if refl else 2}
    adm = _admissible(layout, bc)
    assert adm == ([2, 4] if refl else [1, 2, 4])
    seen = set()
    for cells in [0] + adm:
        s, _ = _open(rtsn_mod, oracle_mod, layout, ts, bc, law, cells=cells)
        with s:
            st = s.wavefront_state()
            assert st["active"] and st["cells_per_lane"] in adm
            if cells:
                assert st["cells_per_lane"] == cells
            assert st["waves"] == want_waves[st["cells_per_lane"]], st
            seen.add(st["cells_per_lane"])
            coupled_steps(s, occ.STEPS)
            err = compare(s, r["ref"])
            err["f"] = _law_f_rel(s, r["ref"])
            print(layout, ts, bc, st, err)
            assert err["f"] <= 1e-14, err
    assert seen == set(adm)


# ---------------------------------------------------------------------------
# 3: independence of the chain and of how the steps are driven, bitwise
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("bc", [(0, 0), (2, 1)], ids=_ids)
@pytest.mark.parametrize("layout", ["c44", "c336"])
def test_independence_bitwise(rtsn_mod, oracle_mod, layout, bc):
    """BDF2, exponents (3, 1.5), 6 steps: every admissible cells per lane, wave caps that change the
    chain (the plan then takes more cells per lane), a re-plan between steps 3 and 4, and
    material_step(6) against 6 x (material_sweep, material_update): every read-out and f array_equal."""
    refl = bc[0] == 2
    adm = _admissible(layout, bc)

    def run(cells, waves, drive, want=None):
        s, _ = _open(rtsn_mod, oracle_mod, layout, 3, bc, "marshak", cells=cells, waves=waves)
        with s:
            st = s.wavefront_state()
            if want:
                assert (st["cells_per_lane"], st["waves"]) == want, (st, want)
            drive(s)
            assert s.wavefront_state()["active"]
            return dict(_coupled_readouts(s), f=s.opacity_scale()), st

    def replan(s):
        coupled_steps(s, 3)
        s.set_wavefront_cells(adm[-1] if s.wavefront_state()["cells_per_lane"] != adm[-1] else adm[0])
        coupled_steps(s, 3)

    steps = lambda s: coupled_steps(s, 6)  # noqa: E731
    first, st0 = run(adm[0], 0, steps)
    # wave caps under which fewer cells per lane no longer fit: (cap, the only chain left or None)
    caps = {("c44", False): [], ("c44", True): [(1, None)],
            ("c336", False): [(3, None), (2, (4, 2))], ("c336", True): [(3, (4, 3))]}[(layout, refl)]
    variants = [(C, 0, steps, None) for C in adm[1:]] + [(0, w, steps, want) for w, want in caps]
    variants += [(adm[0], 0, replan, None), (0, 0, lambda s: s.material_step(6), None)]
    chains = {(st0["cells_per_lane"], st0["waves"])}
    for n, v in enumerate(variants):
        got, st = run(*v)
        chains.add((st["cells_per_lane"], st["waves"]))
        for k, want in first.items():
            assert np.array_equal(got[k], want), (k, n, v[:2], st)
    assert len(chains) >= len(adm)


# ---------------------------------------------------------------------------
# 4: against the line walk
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("layout,law,ts,bc", occ.WALK, ids=_ids)
def test_against_the_walk(rtsn_mod, oracle_mod, layout, law, ts, bc):
    """The same case on a segment-mode handle through the existing calls, 6 steps: T, psi, ends, B,
    Beff and transit agree with the line walk's at compare's tolerances (T 1e-12, the rest 1e-10).
    NOT array_equal: both kernels run the same functions of cell.hpp on the same inputs, but the
    walk's expressions are contracted into FMAs as the compiler chooses in that kernel, and the
    chain's are rounded operation by operation (kernels_wave.hip Unfused), which is what makes the
    chain independent of its cells per lane, bitwise (test_independence_bitwise).  The largest
    differences seen are printed in units of the last place (DESIGN.md §9 records them)."""
    walk = _open_walk(rtsn_mod, oracle_mod, layout, ts, bc, law)
    s, _ = _open(rtsn_mod, oracle_mod, layout, ts, bc, law)
    with walk, s:
        assert np.array_equal(s.opacity_scale(), walk.opacity_scale())  # the same T0, the same kernel
        coupled_steps(walk, occ.STEPS)
        coupled_steps(s, occ.STEPS)
        assert s.wavefront_state()["active"] and not walk.wavefront_state()["active"]
        got = dict(_coupled_readouts(s), B=s.cell_planck())
        want = dict(_coupled_readouts(walk), B=walk.cell_planck())
        ulps = {k: float((np.abs(got[k] - v) / np.spacing(np.maximum(np.abs(v), 1e-300))).max()) for k, v in want.items()}
        print("ulps", layout, ts, bc, ulps)
        print(layout, ts, bc, compare(s, _AsReference(walk)))


# ---------------------------------------------------------------------------
# 5: neutral elements
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("ts", [1, 2, 3])
def test_law_cleared_before_any_step_is_the_plain_chain_bitwise(rtsn_mod, oracle_mod, ts):
    bc = (2, 1)
    plain, _ = _open(rtsn_mod, oracle_mod, "c44", ts, bc)
    with plain:
        plan = plain.wavefront_state()
        coupled_steps(plain, 4)
        want = _coupled_readouts(plain)
    s, _ = _open(rtsn_mod, oracle_mod, "c44", ts, bc, "marshak")
    with s:
        assert s.opacity_scale().max() > 10.0
        s.material_set_opacity_law_chain(None, None, 1.0, 1.0)
        assert np.array_equal(s.opacity_scale(), np.ones(s.N))
        assert s.wavefront_state() == plan  # the unrestricted plan again
        coupled_steps(s, 4)
        got = _coupled_readouts(s)
    for k, v in want.items():
        assert np.array_equal(got[k], v), k


@pytest.mark.parametrize("ts", [1, 2, 3])
@pytest.mark.parametrize("bc", [(0, 0), (2, 1)], ids=_ids)
def test_exponent_zero_is_the_plain_chain_to_rounding(rtsn_mod, oracle_mod, bc, ts):
    """The law form with f = 1 against the map form, compare's tolerances: not bitwise, the maps are
    derived in long double and the law form's constants in fp64."""
    plain, _ = _open(rtsn_mod, oracle_mod, "c44", ts, bc)
    s, _ = _open(rtsn_mod, oracle_mod, "c44", ts, bc, "zero")
    with plain, s:
        assert np.array_equal(s.opacity_scale(), np.ones(s.N))
        coupled_steps(plain, occ.STEPS)
        coupled_steps(s, occ.STEPS)
        print(bc, ts, compare(s, _AsReference(plain)))


# ---------------------------------------------------------------------------
# 6: energy, BE
# ---------------------------------------------------------------------------
def _step_balances(s, p, dx, rcv, e0, tag):
    s.material_step(1)
    e1 = olr.energy(s, dx, rcv)
    resid = (e1 - e0) + p["dt"] * net_outflow(GpuView(s), p)
    print(tag, resid / e1)
    assert abs(resid) <= 1e-12 * abs(e1), (tag, resid, e1)
    return e1


@pytest.mark.parametrize("bc", [(0, 0), (2, 1)], ids=_ids)
@pytest.mark.parametrize("layout,law", [("c12", "marshak"), ("c44", "marshak"), ("c44", "clamped")])
def test_backward_euler_energy_on_device(rtsn_mod, oracle_mod, layout, law, bc):
    """Per step: the change of sum_x dx(x) (sum_g phi_g / c + rho_cv(x) T + transit) plus dt x the net
    boundary outflow is at most 1e-12 of the total; T > 0 and Beff >= 0.  (`clamped` on (20, 24) only:
    on (5, 7) the reference does not keep both clamps active.)"""
    s, p = _open(rtsn_mod, oracle_mod, layout, 1, bc, law)
    _, regions, rho_cv, _ = occ.case(oracle_mod, layout, 1, bc)
    dx, rcv = occ.energy_terms(regions, rho_cv)
    with s:
        e = olr.energy(s, dx, rcv)
        for n in range(occ.STEPS):
            e = _step_balances(s, p, dx, rcv, e, (layout, law, bc, n))
            assert (s.temperature() > 0).all() and (s.cell_emission() >= 0).all()


@pytest.mark.parametrize("bc", [(0, 0), (2, 1)], ids=_ids)
def test_law_set_in_mid_run_conserves_energy(rtsn_mod, oracle_mod, bc):
    """BE on (20, 24): 3 steps of the plain chain, so that emission is owed; the law set, changed and
    cleared between steps.  The energy sum is unchanged across each call at 1e-12 (the owed rescale),
    every later step balances at 1e-12, and the run equals the reference driven the same way."""
    s, p = _open(rtsn_mod, oracle_mod, "c44", 1, bc)
    _, regions, rho_cv, T0 = occ.case(oracle_mod, "c44", 1, bc)
    dx, rcv = occ.energy_terms(regions, rho_cv)
    ref = olr.OpacityLawReference(oracle_mod, p, regions, rho_cv, T0)
    calls = [olr.law_args("marshak"), olr.law_args("clamped"), (None, None, 1.0, 1.0), olr.law_args("mixed")]
    with s:
        s.material_step(3)
        ref.material_step(3)
        assert np.abs(s.material_transit()).max() > 0.0  # emission is in transit when the law arrives
        for args in calls:
            e0 = olr.energy(s, dx, rcv)
            s.material_set_opacity_law_chain(*args)
            ref.set_law(*args)
            e1 = olr.energy(s, dx, rcv)
            print(bc, args[0], (e1 - e0) / e1)
            assert abs(e1 - e0) <= 1e-12 * abs(e1), (args, e0, e1)
            assert _law_f_rel(s, ref) <= 1e-14
            for n in range(2):
                ref.material_step(1)
                e1 = _step_balances(s, p, dx, rcv, e1, (bc, args[0], n))
        print(compare(s, ref))


# ---------------------------------------------------------------------------
# 7: the table
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("layout,table,ts,bc", occ.TABLE_PARITY, ids=_ids)
def test_table_parity(rtsn_mod, oracle_mod, layout, table, ts, bc):
    r = occ.reference_run(oracle_mod, layout, table, ts, bc, kind="table")
    s, p = _open(rtsn_mod, oracle_mod, layout, ts, bc, table=table)
    with s:
        f0 = s.opacity_scale_groups()
        assert float(np.max(np.abs(f0 - r["f0"]) / r["f0"])) <= 1e-14  # the same T0: the device's expression alone
        coupled_steps(s, occ.STEPS)
        assert s.wavefront_state()["active"]
        err = compare(s, r["ref"])
        err["f"] = _table_f_rel(s, r["ref"])
        print(layout, ts, bc, err)
        assert err["f"] <= 1e-14, err


@pytest.mark.parametrize("ts", [1, 3])
def test_clamped_law_as_a_table(rtsn_mod, oracle_mod, ts):
    """`as_law` against the device's own `clamped` power-law run, compare's tolerances."""
    bc = (2, 1)
    law, _ = _open(rtsn_mod, oracle_mod, "c44", ts, bc, law="clamped")
    s, _ = _open(rtsn_mod, oracle_mod, "c44", ts, bc, table="as_law")
    with law, s:
        coupled_steps(law, occ.STEPS)
        coupled_steps(s, occ.STEPS)
        print(ts, compare(s, _AsReference(law)))
        f = law.opacity_scale()
        assert np.max(np.abs(s.opacity_scale_groups() - f[:, None]) / f[:, None]) <= 1e-11
        assert np.array_equal(law.opacity_scale_groups(), np.repeat(f[:, None], s.G, axis=1))


class _Calls:
    """A solver under the reference's set_table / set_law names (test_opacity_table.transitions)."""

    def __init__(self, s):
        self.s = s

    def set_table(self, T_grid, scale):
        self.s.material_set_opacity_table_chain(T_grid, scale)

    def set_law(self, *args):
        self.s.material_set_opacity_law_chain(*args)


@pytest.mark.parametrize("bc", [(0, 0), (2, 1)], ids=_ids)
def test_table_transitions_in_mid_run_conserve_energy(rtsn_mod, oracle_mod, bc):
    """BE on (20, 24): 3 steps with nothing set; then the table set, changed, replaced by the law,
    the law replaced by the table, the table cleared.  The energy sum is unchanged across each call
    at 1e-12, every later step balances at 1e-12, f follows the reference at 1e-14."""
    from test_opacity_table import transitions
    s, p = _open(rtsn_mod, oracle_mod, "c44", 1, bc)
    _, regions, rho_cv, T0 = occ.case(oracle_mod, "c44", 1, bc)
    dx, rcv = occ.energy_terms(regions, rho_cv)
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
            assert _table_f_rel(s, ref) <= 1e-14
            assert s.wavefront_state()["active"]
            for n in range(2):
                ref.material_step(1)
                e1 = _step_balances(s, p, dx, rcv, e1, (bc, k, n))
        print(compare(s, ref))


# ---------------------------------------------------------------------------
# 8: with the energy table
# ---------------------------------------------------------------------------
def test_with_the_energy_table(rtsn_mod, oracle_mod):
    """BE on (20, 24), reflective, the law and heat_capacity_ref's (32, 48) energy table: compare's
    tolerances (test_heat_capacity_gpu's) against HeatCapacityReference, and the energy statement
    with e(T) in it at 1e-12 per step."""
    import heat_capacity_ref as hcr
    ts, bc = 1, (2, 1)
    p, regions, rho_cv, T0 = occ.case(oracle_mod, "c44", ts, bc)
    et = hcr.energy_table("n80", 2)
    ref = hcr.HeatCapacityReference(oracle_mod, p, regions, rho_cv, T0, law=olr.law_args("marshak"), table=None,
                                    energy_table=et)
    dx = ref.dx_cells
    s, _ = _open(rtsn_mod, oracle_mod, "c44", ts, bc, "marshak")
    with s:
        s.material_set_energy_table(*et)
        e0 = hcr.energy(s, dx)
        for n in range(occ.STEPS):
            s.material_step(1)
            ref.material_step(1)
            e1 = hcr.energy(s, dx)
            resid = (e1 - e0) + p["dt"] * net_outflow(GpuView(s), p)
            print(n, resid / e1)
            assert abs(resid) <= 1e-12 * abs(e1), (n, resid, e1)
            e0 = e1
        near = min(float(np.abs(h["ratio"] - 0.25).min()) for h in ref.history)
        assert near > 1e-6, near  # the device and the reference take the same branch
        err = compare(s, ref)
        print(err)
        np.testing.assert_allclose(s.material_energy(), np.asarray(ref.material_energy(), dtype=np.float64),
                                   rtol=1e-12)


# ---------------------------------------------------------------------------
# 9: group shards
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["law", "table"])
def test_group_shards_on_one_gpu(rtsn_mod, oracle_mod, kind):
    """Groups [0, 2) and [2, 5) as two handles on (20, 24), reflective, BDF2, their [q, b] summed by
    the test, 6 steps: T equals the full handle's at rtol 1e-12, psi at 1e-10 per group."""
    import torch
    ts, bc = 3, (2, 1)
    kw = dict(law="marshak") if kind == "law" else dict(table="edge")
    full, p = _open(rtsn_mod, oracle_mod, "c44", ts, bc, **kw)
    with full:
        full.material_step(occ.STEPS)
        T_full, psi_full, f_full = full.temperature(), full.psi(), full.opacity_scale_groups()
    bounds = ((0, 2), (2, 5))
    shards = [_open(rtsn_mod, oracle_mod, "c44", ts, bc, g_lo=lo, g_hi=hi, **kw)[0] for lo, hi in bounds]
    try:
        qb = [torch.zeros(2 * p["N"], dtype=torch.float64, device="cuda") for _ in shards]
        for _ in range(occ.STEPS):
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
            assert s.wavefront_state()["active"]
            np.testing.assert_allclose(s.temperature(), T_full, rtol=1e-12)
            np.testing.assert_allclose(s.opacity_scale_groups(), f_full[:, lo:hi], rtol=1e-11)
        psi = np.concatenate([s.psi() for s in shards], axis=1)
        assert per_group_rel(psi, psi_full, 1) <= 1e-10
    finally:
        for s in shards:
            s.close()


# ---------------------------------------------------------------------------
# 10: read-outs
# ---------------------------------------------------------------------------
def test_readouts(rtsn_mod, oracle_mod):
    """With the law on, against the reference after 6 steps: opacity_scale, opacity_scale_groups (the
    law's f repeated over the groups), rt_group_absorption_device (sum_g sigma0_g f phi_g at 1e-10);
    the stability number of a one-region slab of 30 cells (a uniform slab in chain mode) is the
    unscaled number times f at the hottest cell."""
    import torch
    r = occ.reference_run(oracle_mod, "c44", "marshak", 1, (2, 1))
    s, p = _open(rtsn_mod, oracle_mod, "c44", 1, (2, 1), "marshak")
    with s:
        coupled_steps(s, occ.STEPS)
        f = s.opacity_scale()
        want_f = np.asarray(r["ref"].opacity_scale(), dtype=np.float64)
        assert np.max(np.abs(f - want_f) / want_f) <= 1e-11
        assert np.array_equal(s.opacity_scale_groups(), np.repeat(f[:, None], s.G, axis=1))
        out = torch.zeros(p["N"], dtype=torch.float64, device="cuda")
        s.group_absorption(out)
        s.synchronize()
        want = r["ref"].group_absorption()
        assert np.abs(out.cpu().numpy() - want).max() <= 1e-10 * np.abs(want).max()
    from test_material import params
    q = params(oracle_mod, ts=1, dt=occ.SCHEME_DT[1], M=6, G=5, N=30, bc_left=0, bc_right=0)
    q["psi_source"] = np.linspace(0.5, 2.0, 30).reshape(6, 5)
    one = [dict(cells=30, width=30 * 0.004, rho=10.0, kappa_grey=q["kappa_grey"], T=0.5, group_kappa=None)]
    T0 = np.linspace(0.2, 0.8, 30)
    with rtsn_mod.Solver(to_rt(q), regions=one) as u:
        number = u.material_enable_regions([0.5], T0)
        u.material_set_opacity_law_chain([2.0], [0.4], 1e-3, 1e3)
        assert u.wavefront_state()["active"]
        assert u.material_stability() == pytest.approx(number * (0.8 / 0.4) ** -2.0, rel=1e-13)
        assert np.max(np.abs(u.opacity_scale() / (T0 / 0.4) ** -2.0 - 1.0)) <= 1e-14
        u.material_step(2)
        assert np.isfinite(u.ends()).all() and (u.temperature() > 0).all()


# ---------------------------------------------------------------------------
# 11: the statuses
# ---------------------------------------------------------------------------
def test_statuses(rtsn_mod, oracle_mod):
    p, regions, rho_cv, T0 = occ.case(oracle_mod, "n80", 3, (0, 0))
    q = to_rt(p)
    L = rtsn_mod.lib()
    law = olr.law_args("marshak")
    tab = otr.table_args("edge", p["G"])

    def status(fn):
        return _status(rtsn_mod, fn)

    def message(s):
        return L.rt_last_error(s._h).decode()

    with rtsn_mod.Solver(q) as s:  # a handle without regions
        assert status(lambda: s.material_set_opacity_law_chain(*law)) == 9
        assert "rt_create_regions" in message(s)
        assert status(lambda: s.material_set_opacity_table_chain(*tab)) == 9
    with rtsn_mod.Solver(q, regions=regions) as s:  # segment mode
        _segment_mode(s, 4, cells=16)
        assert status(lambda: s.material_set_opacity_law_chain(*law)) == 9
        assert "segment mode" in message(s) and "rt_material_set_opacity_law" in message(s)
        assert "rt_material_set_opacity_law_chain: " in message(s)
        s.material_enable_segments(rho_cv, T0)
        assert status(lambda: s.material_set_opacity_table_chain(*tab)) == 9
        assert "which takes rt_material_set_opacity_table" in message(s)
    with rtsn_mod.Solver(q, regions=regions) as s:  # chain mode
        assert s.wavefront_state()["active"]
        assert status(lambda: s.material_set_opacity_law_chain(*law)) == 9  # uncoupled
        assert "rt_material_enable_regions first" in message(s)
        assert status(lambda: s.material_set_opacity_table_chain(*tab)) == 9
        assert "rt_material_enable_regions first" in message(s)
        s.material_enable_regions(rho_cv, T0)
        # the segment-mode calls on a chain-mode handle: RT_ERR_STATE, as before
        assert status(lambda: s.material_set_opacity_law(*law)) == 9
        assert "chain mode" in message(s) and "rt_material_enable_segments" in message(s)
        assert status(lambda: s.material_set_opacity_table(*tab)) == 9
        assert "chain mode" in message(s)
        assert np.array_equal(s.opacity_scale(), np.ones(s.N))  # the law off
        # the segment-mode calls' RT_ERR_ARG rules
        n, tr = law[0], law[1]
        assert status(lambda: s.material_set_opacity_law_chain(n[:1], tr[:1], 1e-3, 1e3)) == 8
        for bad in (0.0, -1.0, float("nan"), float("inf")):
            assert status(lambda: s.material_set_opacity_law_chain(n, [tr[0], bad], 1e-3, 1e3)) == 8
        for lo, hi in ((0.0, 1.0), (2.0, 1.0), (1.0, float("inf")), (float("nan"), 1.0)):
            assert status(lambda: s.material_set_opacity_law_chain(n, tr, lo, hi)) == 8
        assert status(lambda: s.material_set_opacity_table_chain(tab[0][:1], tab[1][:, :1])) == 8
        assert status(lambda: s.material_set_opacity_table_chain(tab[0][::-1], tab[1])) == 8
        assert np.array_equal(s.opacity_scale_groups(), np.ones((s.N, s.G)))  # a refused call changes nothing
        s.material_set_opacity_law_chain(None, None, 0.0, 0.0)  # off while off: accepted
        s.material_set_opacity_table_chain(None, None)
        # 8 cells per lane falls back to the plan's choice while a law or table is on
        s.set_wavefront_cells(8)
        assert s.wavefront_state()["cells_per_lane"] == 8  # (32, 48): admissible for the map form
        s.material_set_opacity_law_chain(*law)
        assert s.wavefront_state()["cells_per_lane"] in (1, 2, 4) and s.wavefront_state()["active"]
        # one launch per coupled sweep with the law on
        s.set_profiling(True)
        n0 = s.sweep_time()[1]
        s.material_sweep()
        s.material_update()
        assert s.sweep_time()[1] == n0 + 1
        s.set_profiling(False)
        assert np.isfinite(s.ends()).all()
        # rt_material_enable_regions called again clears the law
        s.material_enable_regions(rho_cv, T0)
        assert np.array_equal(s.opacity_scale(), np.ones(s.N))
        s.set_wavefront_cells(8)
        assert s.wavefront_state()["cells_per_lane"] == 8


def test_no_law_chain_fits(rtsn_mod, oracle_mod):
    """N = 4096 with the edge on a multiple of 8, M = 2, G = 1: the only chain that fits 8 waves has 8
    cells per lane, so the set calls return RT_ERR_PARAM with a message that names segment mode, and
    the handle then steps as the plain coupled chain, unchanged.  And on (160, 176) with the law on,
    a wave cap of 1 (336 cells need 2 waves even at 4 per lane) is refused, nothing changed."""
    from test_material import params
    L = rtsn_mod.lib()
    cells = (2048, 2048)
    p = params(oracle_mod, ts=1, dt=1e-3, M=2, G=1, N=4096, bc_left=0, bc_right=0)
    p["psi_source"] = np.ones((2, 1))
    regions = [dict(cells=c, width=c * d, rho=r, kappa_grey=p["kappa_grey"], T=t, group_kappa=None)
               for c, d, r, t in zip(cells, olr.DXS, olr.RHO, olr.T_REGION)]
    T0 = olr.t_cells(cells)
    Tg, sc = np.array([0.1, 1.0]), np.ones((2, 2, 1))

    def run(try_law):
        with rtsn_mod.Solver(to_rt(p), regions=regions) as s:
            s.material_enable_regions(olr.RHO_CV, T0)
            assert s.wavefront_state()["cells_per_lane"] == 8 and s.wavefront_state()["waves"] == 8
            if try_law:
                assert _status(rtsn_mod, lambda: s.material_set_opacity_law_chain(*olr.law_args("marshak"))) == 3
                msg = L.rt_last_error(s._h).decode()
                assert "segment mode" in msg and "rt_material_enable_segments" in msg
                assert _status(rtsn_mod, lambda: s.material_set_opacity_table_chain(Tg, sc)) == 3
                assert np.array_equal(s.opacity_scale(), np.ones(s.N))
                assert s.wavefront_state()["cells_per_lane"] == 8 and s.wavefront_state()["active"]
            coupled_steps(s, 2)
            return _coupled_readouts(s)

    want, got = run(False), run(True)
    for k, v in want.items():
        assert np.array_equal(got[k], v), k
    s, _ = _open(rtsn_mod, oracle_mod, "c336", 1, (0, 0), waves=1)  # the wave cap first: 8 cells per lane
    with s:
        assert s.wavefront_state()["cells_per_lane"] == 8 and s.wavefront_state()["waves"] == 1
        assert _status(rtsn_mod, lambda: s.material_set_opacity_law_chain(*olr.law_args("marshak"))) == 3
        assert "segment mode" in L.rt_last_error(s._h).decode()
        assert np.array_equal(s.opacity_scale(), np.ones(s.N)) and s.wavefront_state()["cells_per_lane"] == 8
        s.wavefront_waves = 2
        s.material_set_opacity_law_chain(*olr.law_args("marshak"))  # 84 lanes at 4 cells per lane
        assert s.wavefront_state()["cells_per_lane"] == 4
        coupled_steps(s, 1)
        assert np.isfinite(s.ends()).all()
    s, _ = _open(rtsn_mod, oracle_mod, "c336", 1, (0, 0), "marshak")
    with s:
        before = s.wavefront_state()
        with pytest.raises(rtsn_mod.RtError) as e:
            s.wavefront_waves = 1
        assert e.value.status == 3
        assert s.wavefront_state() == before and s.wavefront_waves == 8
        s.wavefront_waves = 2
        assert s.wavefront_state()["cells_per_lane"] == 4 and s.wavefront_state()["waves"] == 2
