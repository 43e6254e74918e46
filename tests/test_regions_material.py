"""Material-temperature coupling on multi-region slabs, CPU side.

* tests/regions_material_ref.py (the numpy restatement the GPU tests compare a heterogeneous
  slab against) is pinned to the C oracle: with identical regions it must equal
  OracleSolver.material_* -- T to 1e-12 relative, the fields by test_material_gpu.compare's
  metrics to 1e-10 -- including cells that take the full-emission (Newton) path;
* rt_regions_plan_steps against a Python restatement of its rule;
* the new entry points' declarations and ctypes signatures.
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

from regions_material_ref import RegionMaterialReference, plan_rule
from test_material import params, t_profile
from test_material_gpu import compare
from test_regions_gpu import TICK_REFLECTIVE, TICK_VACUUM

CUTS = (40, 24, 64)  # identical regions of N = 128


def uniform_regions(p, cells):
    dx = p["X"] / p["N"]
    return [dict(cells=int(c), width=float(c * dx), rho=p["rho"], kappa_grey=p["kappa_grey"], T=p["T"],
                 group_kappa=p["group_kappa"]) for c in cells]


def _pin(oracle_mod, p, rho_cv, T0, steps, cuts=CUTS):
    orc = oracle_mod.OracleSolver(p)
    orc.material_enable(rho_cv, T0)
    ref = RegionMaterialReference(oracle_mod, p, uniform_regions(p, cuts), [rho_cv] * len(cuts), T0)
    np.testing.assert_array_equal(ref.ends(), orc.ends())  # psi = B_g at the start, both
    for _ in range(steps):
        orc.material_step(1)
        ref.material_step(1)
    err = compare(ref, orc)  # T 1e-12; psi, ends, phi, B, Beff, transit 1e-10
    print(err)
    return ref, orc


@pytest.mark.parametrize("ts,dt", [(1, 1e-3), (2, 1e-3), (3, 1e-4)])
@pytest.mark.parametrize("bc", [(2, 0), (0, 0)])
def test_reference_equals_oracle_on_identical_regions(oracle_mod, ts, dt, bc):
    p = params(oracle_mod, ts=ts, dt=dt, M=6, G=5, N=128, bc_left=bc[0], bc_right=bc[1])
    p["psi_source"] = np.linspace(0.5, 2.0, p["M"] * p["G"]).reshape(p["M"], p["G"])
    _pin(oracle_mod, p, 5.0, t_profile(p["N"]), 6)


def test_reference_equals_oracle_cold_start_newton_path(oracle_mod):
    """0.05 keV material under 1 keV radiation with a small heat capacity: the linearised
    update would heat cells by more than T / 4, so they solve the full emission -- the oracle by
    Newton's method, the reference by bisection."""
    p = params(oracle_mod, ts=1, dt=1e-3, M=6, G=5, N=128, bc_left=2, bc_right=0)
    T0 = np.full(p["N"], 0.05)
    # the test's own premise, from the first update's linear dT
    orc = oracle_mod.OracleSolver(p)
    orc.material_enable(0.5, T0)
    qb = orc.material_sweep()
    W = orc.quad()[1].sum()
    dT = p["dt"] * qb[:p["N"]] / (0.5 + p["dt"] * W * qb[p["N"]:])
    assert (dT > 0.25 * T0).any()
    ref, _ = _pin(oracle_mod, p, 0.5, T0, 6)
    assert ref.newton_cells > 0


# ---------------------------------------------------------------------------
# rt_regions_plan_steps
# ---------------------------------------------------------------------------
def _random_layout(rng):
    """A slab whose region edges are multiples of a random C0 of 1, 2, 4, 8."""
    C0 = int(rng.choice([1, 2, 4, 8]))
    n_units = int(rng.integers(2, 4096 // C0 + 1)) if rng.random() < 0.5 else int(rng.integers(2, 600 // C0 + 2))
    R = int(rng.integers(1, min(4, n_units) + 1))
    cuts = np.sort(rng.choice(np.arange(1, n_units), size=R - 1, replace=False)) if R > 1 else np.array([], dtype=int)
    return [int(c) * C0 for c in np.diff(np.concatenate([[0], cuts, [n_units]]))]


def test_regions_plan_steps_rule(rtsn_mod):
    rng = np.random.default_rng(20240611)
    picked_larger = 0
    for _ in range(200):
        cells = _random_layout(rng)
        regions = [dict(cells=c, width=0.01 * c, rho=1.0, kappa_grey=1.0, T=1.0, group_kappa=None) for c in cells]
        for reflective in (False, True):
            for max_waves in (1, 4, 8):
                plans = {}
                for nsteps in (1, 1000):
                    want = plan_rule(cells, reflective, max_waves, nsteps, TICK_VACUUM, TICK_REFLECTIVE)
                    if want[0] == 0:
                        with pytest.raises(rtsn_mod.RtError) as e:
                            rtsn_mod.regions_plan(regions, reflective, max_waves, nsteps)
                        assert e.value.status == 3
                        continue
                    got = rtsn_mod.regions_plan(regions, reflective, max_waves, nsteps)
                    assert (got["cells_per_lane"], got["waves"], got["lanes"]) == want, (cells, reflective, max_waves,
                                                                                         nsteps)
                    plans[nsteps] = got
                if 1000 in plans:  # nsteps = 1000 is rt_regions_plan
                    keep: list = []
                    arr = rtsn_mod.api._region_structs(regions, 0, keep)
                    c, w, n = C.c_int(), C.c_int(), C.c_int()
                    assert rtsn_mod.lib().rt_regions_plan(arr, len(regions), int(reflective), max_waves, C.byref(c),
                                                          C.byref(w), C.byref(n)) == 0
                    assert (c.value, w.value, n.value) == tuple(plans[1000][k] for k in ("cells_per_lane", "waves", "lanes"))
                    picked_larger += plans[1]["cells_per_lane"] > plans[1000]["cells_per_lane"]
    assert picked_larger > 0  # the one-step rule does differ from the 1000-step one somewhere


def test_new_entry_points_declared_and_exported(rtsn_mod):
    names = rtsn_mod.exported_symbols()
    L = rtsn_mod.lib()
    for f in ("rt_material_enable_regions", "rt_regions_plan_steps"):
        assert f in names and hasattr(L, f)
    # the host-only one through bare ctypes argtypes, no GPU
    fn = L.rt_regions_plan_steps
    assert fn.argtypes[4] is C.c_longlong and len(fn.argtypes) == 8
    keep: list = []
    arr = rtsn_mod.api._region_structs([dict(cells=64, width=1.0, rho=1.0, kappa_grey=1.0, T=1.0, group_kappa=None),
                                        dict(cells=64, width=2.0, rho=2.0, kappa_grey=1.0, T=0.5, group_kappa=None)],
                                       0, keep)
    c, w, n = C.c_int(), C.c_int(), C.c_int()
    assert fn(arr, 2, 0, 8, 1, C.byref(c), C.byref(w), C.byref(n)) == 0
    assert c.value * n.value == 128 and w.value == -(-n.value // 64)
    assert fn(arr, 2, 0, 8, 0, C.byref(c), C.byref(w), C.byref(n)) == 8  # nsteps < 1: RT_ERR_ARG
    assert fn(arr, 2, 0, 9, 1, None, None, None) == 8
