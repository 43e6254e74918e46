"""The regime sweep's references, checked on the CPU before any GPU time is spent
(tests/regime_cases.py; the GPU side is tests/test_regime_gpu.py).

On every grid point the GPU tests use -- uniform slabs of 70 and 320 cells at 6 steps, the
22- and 26-step BDF2 runs, the three-region slabs -- the conditions that keep a case from
passing vacuously: truth and oracle finite, every |truth| in [1e-250, 1e250], the fp64
oracle's own line-wise error against the extended-precision truth at most 1e-6.  Then the
plumbing of the truth itself: the dtype reaches every array, the batched truth equals a
FusedSolver of its own, fused_np in fp64 equals the C oracle, and the metric sees what
parity.per_group_rel does not.
"""
import numpy as np
import pytest

import fused_np
import regime_cases as rc
from parity import per_group_rel

pytestmark = pytest.mark.skipif(not rc.HAVE_EXTENDED, reason=rc.SKIP_REASON)

_seen = {}


def _conditions(case, tag):
    err_o = rc.check_conditions(case.truth, case.oracle)
    assert case.truth.dtype == np.longdouble and case.oracle.dtype == np.float64
    # the truth is not the oracle in a wider format: rounded to fp64 it differs from it
    assert not np.array_equal(np.asarray(case.truth, dtype=np.float64), case.oracle)
    _seen[tag] = (min(_seen.get(tag, (1.0, 0.0))[0], float(err_o.min())),
                  max(_seen.get(tag, (1.0, 0.0))[1], float(err_o.max())))
    return err_o


@pytest.mark.parametrize("N", [70, 320])
@pytest.mark.parametrize("ts,cfl,bc,V", rc.GRID, ids=rc.ids(rc.GRID))
def test_uniform_grid_conditions(oracle_mod, N, ts, cfl, bc, V):
    for start in rc.STARTS:
        case = rc.uniform_case(oracle_mod, N, ts, cfl, bc, V, start)
        assert case.steps == rc.STEPS and case.truth.shape == (rc.M, rc.G, N, 2)
        _conditions(case, ("uniform", N))
    print("oracle's own error (min, max over lines) so far:", _seen[("uniform", N)])


@pytest.mark.parametrize("ts,cfl,bc,V", rc.LONG_GRID, ids=rc.ids(rc.LONG_GRID))
def test_long_grid_conditions(oracle_mod, ts, cfl, bc, V):
    for start in rc.STARTS:
        for steps in rc.LONG_STEPS:
            _conditions(rc.uniform_case(oracle_mod, 320, ts, cfl, bc, V, start, steps), ("long", steps))
    print("oracle's own error (min, max over lines) so far:", _seen[("long", rc.LONG_STEPS[-1])])


@pytest.mark.parametrize("cells", rc.REGION_CELLS, ids=lambda c: "x".join(map(str, c)))
@pytest.mark.parametrize("ts,cfl,bc_left,V", rc.REGION_GRID, ids=rc.ids(rc.REGION_GRID))
def test_region_grid_conditions(oracle_mod, cells, ts, cfl, bc_left, V):
    for start in rc.STARTS:
        case = rc.region_case(oracle_mod, cells, ts, cfl, bc_left, V, start)
        assert [r["cells"] for r in case.regions] == list(cells) and case.truth.shape == (rc.M, rc.G, 64, 2)
        _conditions(case, ("regions", cells))
    print("RegionReference fp64's own error (min, max over lines) so far:", _seen[("regions", cells)])


def test_regime_spans_the_decades(oracle_mod):
    """The medium is what the issue states: sigma dx over ten decades in one handle, c dt / dx
    over eight, the inflow over six decades around B."""
    p = rc.medium(oracle_mod, 70, 3, 1e4, (1, 1), 5.994)
    o = oracle_mod.OracleSolver(p)
    np.testing.assert_allclose(p["rho"] * o.groups()["kappa"] * p["dx"], rc.SIGMA_DX, rtol=1e-12)
    assert fused_np.C_LIGHT * p["dt"] / p["dx"] == pytest.approx(1e4, rel=1e-12)
    assert p["use_correction"] == 1 and rc.medium(oracle_mod, 70, 3, 1.0, (1, 1), 0.0)["use_correction"] == 0
    r = p["psi_source"] / o.groups()["B"][None, :]
    assert r.min() >= 1e-3 and r.max() <= 1e3 and r.max() / r.min() > 1e4
    np.testing.assert_array_equal(o.psi_source(), p["psi_source"])


@pytest.mark.parametrize("ts", rc.SCHEMES)
@pytest.mark.parametrize("bc", rc.BCS, ids=rc.ids([(b,) for b in rc.BCS]))
def test_dtype_reaches_every_array(oracle_mod, ts, bc):
    p = rc.medium(oracle_mod, 9, ts, 1.0, bc, 5.994, 2)
    o = oracle_mod.OracleSolver(p)
    g, c = o.groups(), o.correction_coeffs()
    for dtype in (np.float64, np.longdouble):
        f = fused_np.FusedSolver(p, o.quad()[0], g["B"], g["kappa"], c["cor1"], c["cor2"], c["cor3"], o.psi_source(),
                                 dtype=dtype)
        for half in (0, 1):
            ls = f.lines[half]
            arrays = [ls.mu, ls.m, ls.sigma, ls.B, ls.Sc, ls.Sl, ls.be["b"], *ls.be["inv"], ls.cn["A"], ls.cn["k1"],
                      ls.cn["k2"], *ls.cn["inv"], *[ls.bdf[k] for k in ("Bc", "q1", "q2", "q3", "q4")], *ls.bdf["inv"],
                      f.E[half]]
            assert all(a.dtype == np.dtype(dtype) for a in arrays)
            assert all(type(x) is np.dtype(dtype).type for x in (ls.dx, ls.dt, ls.tau, ls.hd))
        f.step()
        f.step()
        assert f.ends().dtype == np.dtype(dtype) and all(f.E[h].dtype == np.dtype(dtype) for h in (0, 1))


@pytest.mark.parametrize("ts,cfl,bc,V", rc.GRID[::7], ids=rc.ids(rc.GRID[::7]))
def test_batched_truth_equals_direct(oracle_mod, ts, cfl, bc, V):
    """The four (V, start) variants computed as copies of the groups are the bits a
    FusedSolver of the case alone gives (correction off included: use_correction = 0)."""
    for start in rc.STARTS:
        case = rc.uniform_case(oracle_mod, 70, ts, cfl, bc, V, start)
        assert np.array_equal(rc.direct_truth(oracle_mod, case), case.truth)


@pytest.mark.parametrize("N", [70, 320])
@pytest.mark.parametrize("ts,cfl,bc,V", rc.GRID, ids=rc.ids(rc.GRID))
def test_fused_fp64_matches_oracle(oracle_mod, N, ts, cfl, bc, V):
    """fused_np in fp64 (the truth's algebra in the oracle's format) against the C oracle at
    tests/test_oracle.py's 1e-13 per group, on every grid point but two: BE and CN at
    c dt / dx = 1e4 on the reflective 320-cell lines, where one step carries the inflow through
    the whole chain of 2 N = 640 cells.  Each of the two evaluations may gather one eps per
    cell on the way, so they may differ by 2 x 640 eps = 2.84e-13, the bound asserted there
    (measured: BE 1.51e-13, CN 1.95e-13; every other point at most 8.0e-14)."""
    chain = N == 320 and cfl == 1e4 and bc[0] == 2 and ts in (1, 2)
    bound = 2 * (2 * N) * rc.EPS if chain else 1e-13
    for start in rc.STARTS:
        case = rc.uniform_case(oracle_mod, N, ts, cfl, bc, V, start)
        o = oracle_mod.OracleSolver(case.p)
        g, c = o.groups(), o.correction_coeffs()
        f = fused_np.FusedSolver(case.p, case.mu, g["B"], g["kappa"], c["cor1"], c["cor2"], c["cor3"], o.psi_source())
        if case.ends0 is not None:
            f.set_ends(case.ends0)
        for _ in range(case.steps):
            f.step()
        assert f.ends().dtype == np.float64
        assert per_group_rel(f.ends(), case.oracle, 1) < bound


def test_metric_sees_what_the_group_metric_misses(oracle_mod):
    """An error of 1e-8 relative in the faintest node of a group (the random start spreads a
    group's nodes over four decades): parity.per_group_rel, which divides by the group's
    largest value, stays under the project's 1e-10, while the line-wise bound is missed by
    orders of magnitude; so is it by one whole line off by 1e-9 relative."""
    case = rc.uniform_case(oracle_mod, 70, 1, 1e-2, (1, 1), 0.0, "random")
    assert rc.check(case.oracle, case) <= 1.0
    rel = np.abs(case.oracle) / np.abs(case.oracle).max(axis=(0, 2, 3))[None, :, None, None]
    at = np.unravel_index(rel.argmin(), rel.shape)
    assert rel[at] < 1e-3
    x = case.oracle.copy()
    x[at] *= 1.0 + 1e-8
    assert per_group_rel(x, case.oracle, 1) <= 1e-10
    with pytest.raises(AssertionError):
        rc.check(x, case)
    assert rc.ratio(x, case).max() > 1e4
    y = case.oracle.copy()
    y[1, 2] *= 1.0 + 1e-9
    with pytest.raises(AssertionError):
        rc.check(y, case)
