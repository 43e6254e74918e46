"""The lean cell maps of the level-split pipelined BDF2 pass (rt_set_map_form; cell.hpp
MAP_NOPSI_NEG / MAP_NOPSI_POS): on a handle whose source has no psi term (use_correction off, or
V = 0) the split kernels skip the map rows that feed nothing.  Bitwise the full map on every
shape of the existing split tests (tests/test_gpu_parity.test_level_split_pass): one line
group partly padding with a ragged last chunk, two line groups per half, vacuum and reflective
chains, the tail launch, and a handle that changes between the forms and kernels mid-run."""
import numpy as np
import pytest

from test_gpu_parity import SEED, compare_all, load, to_rt

pytestmark = pytest.mark.gpu

# FMAs per cell and level of the lean split pass, averaged over the two halves' patterns
# (20 on mu < 0 lines, 13 on mu > 0 lines), against the full map's 28
LEAN_FMAS, FULL_FMAS = 16.5, 28.0


def _setup(oracle_mod, steps, bc_left, N=4099, M=4, V=0.0, use_correction=1):
    p = load(oracle_mod, "llnl_slab_test.prm", N=N, M=M, max_timesteps=steps, use_correction=use_correction, V=V,
             bc_left=bc_left)
    p["dx"] = p["X"] / p["N"]
    p["psi_source"] = np.full((p["M"], p["G"]), 0.5)
    return p


def _ends0(oracle_mod, p, lo, hi, seed):
    B = oracle_mod.OracleSolver(p, g_lo=lo, g_hi=hi).groups()["B"][lo:hi]
    rng = np.random.default_rng(seed)
    return B[None, :, None, None] * rng.uniform(0.5, 1.5, size=(p["M"], hi - lo, p["N"], 2))


def _run(rtsn_mod, p, lo, hi, ends, T, steps, form, lean):
    """`steps` pipelined steps at time block T under rt_set_map_form(form); `lean`: the form
    rt_get_map_form must then report.  Returns the ends and the moments."""
    with rtsn_mod.Solver(to_rt(p), g_lo=lo, g_hi=hi) as s:
        s.map_form = form
        assert s.map_form == lean
        s.time_block = T
        s.pipeline = 2
        s.set_ends(ends)
        s.advance(steps)
        return (s.ends(),) + tuple(s.moments())


def _same(a, b):
    for x, y in zip(a, b):
        assert np.isfinite(x).all()
        assert np.array_equal(x, y)


@pytest.mark.parametrize("T,bc_left,V,use_correction",
                         [(T, bc, 0.0, 1) for T in (8, 20, 40) for bc in (0, 2)] + [(20, 0, 5.994, 0)])
def test_lean_one_line_group(rtsn_mod, oracle_mod, T, bc_left, V, use_correction):
    """N = 4099 (a ragged last chunk), M = 4, groups 30-46 (one line group per half, partly
    padding), random initial ends: the default form (lean) gives the ends and the moments of
    the full form bitwise over 3 T + 1 steps (fill, plateau, drain, remainder) and, on vacuum
    lines, over 2 T + T/2 steps (the tail launch where T has a tail kernel); the lean run
    matches the oracle over T + 3 steps to the project's 1e-10."""
    lo, hi = 30, 46
    p = _setup(oracle_mod, 3 * T + 1, bc_left, V=V, use_correction=use_correction)
    ends = _ends0(oracle_mod, p, lo, hi, SEED + 11 * T + bc_left)
    for steps in [3 * T + 1] + ([2 * T + T // 2] if bc_left == 0 else []):
        _same(_run(rtsn_mod, p, lo, hi, ends, T, steps, 0, 1), _run(rtsn_mod, p, lo, hi, ends, T, steps, 1, 0))
    q = _setup(oracle_mod, T + 3, bc_left, V=V, use_correction=use_correction)
    orc = oracle_mod.OracleSolver(q, g_lo=lo, g_hi=hi)
    orc.set_ends(ends)
    orc.solve()
    with rtsn_mod.Solver(to_rt(q), g_lo=lo, g_hi=hi) as s:
        assert s.map_form == 1
        s.time_block = T
        s.pipeline = 2
        s.set_ends(ends)
        s.advance(T + 3)
        compare_all(s, orc, plus_vs_group=True)


@pytest.mark.parametrize("T", [20, 40])
@pytest.mark.parametrize("bc_left", [0, 2])
def test_lean_two_line_groups(rtsn_mod, oracle_mod, T, bc_left):
    """Two line groups per half (M = 8, groups 30-50: 84 lines, the second group partly
    padding), N = 8000, 2 T + 2 steps: the workgroups' decode of half, position and line group."""
    lo, hi = 30, 50
    p = _setup(oracle_mod, 2 * T + 2, bc_left, N=8000, M=8)
    ends = _ends0(oracle_mod, p, lo, hi, SEED + 13 * T + bc_left)
    _same(_run(rtsn_mod, p, lo, hi, ends, T, 2 * T + 2, 0, 1), _run(rtsn_mod, p, lo, hi, ends, T, 2 * T + 2, 1, 0))


def test_not_eligible(rtsn_mod, oracle_mod):
    """A source with a psi term (use_correction with V != 0): the handle stays on the full map
    under auto, and the results are the full form's."""
    lo, hi = 30, 46
    p = _setup(oracle_mod, 41, 0, V=5.994)
    ends = _ends0(oracle_mod, p, lo, hi, SEED + 17)
    _same(_run(rtsn_mod, p, lo, hi, ends, 20, 41, 0, 0), _run(rtsn_mod, p, lo, hi, ends, 20, 41, 1, 0))


def test_mixed_forms(rtsn_mod, oracle_mod):
    """A handle that leaves the lean split kernels with its pipeline in flight: T steps at
    T = 20 (two waves, lean), then one wave per segment (the full-form sweep_block_kernel, lean
    fill and drain launches around it) for 2 T + 1 more -- the full-form kernels read the zeros
    the lean ones stored into the dead rows of the aggregates.  Bitwise the full form throughout."""
    lo, hi = 30, 46
    T = 20
    p = _setup(oracle_mod, 3 * T + 1, 0)
    ends = _ends0(oracle_mod, p, lo, hi, SEED + 19)
    out = []
    for form in (0, 1):
        with rtsn_mod.Solver(to_rt(p), g_lo=lo, g_hi=hi) as s:
            s.map_form = form
            assert s.map_form == 1 - form
            s.time_block = T
            s.pipeline = 2
            s.set_ends(ends)
            s.advance(T)
            assert s.pipeline_state()["lag_steps"] > 0  # in flight
            s.level_waves = 1
            s.advance(2 * T + 1)
            out.append((s.ends(),) + tuple(s.moments()))
    _same(*out)


def test_sweep_flops_counts_the_form(rtsn_mod, oracle_mod):
    """rt_sweep_flops reports the FMAs of the form the pass at the handle's (T, level waves)
    runs: the lean patterns' mean at T = 40 (four waves), the full map's 28 at T = 16 (the
    one-wave kernel keeps the full form)."""
    p = _setup(oracle_mod, 1, 0)
    with rtsn_mod.Solver(to_rt(p), g_lo=30, g_hi=46) as s:
        s.time_block = 40
        lean = s.sweep_flops()
        s.map_form = 1
        full = s.sweep_flops()
        assert lean * FULL_FMAS == full * LEAN_FMAS and full > 0
        s.map_form = 0
        s.time_block = 16
        assert s.map_form == 1 and s.level_waves == 1
        lean16 = s.sweep_flops()
        s.map_form = 1
        assert lean16 == s.sweep_flops() == full * 16 / 40
