"""Regime-sweep parity of the plain (uncoupled) sweep against an extended-precision truth
(tests/regime_cases.py: the medium, the grid, the metric; tests/test_regime_ref.py checks
the references on the CPU).

Every kernel form of the sweep -- the wavefront chain (two waves with an LDS hand-off, one
wave with a ragged last lane), the pipelined segment passes (time blocks 1 and 4 with a
remainder, 20 on one and two waves, 24 level-split), the aligned schedule (the fold and the
propagators A^Ls) and the region chain with per-lane cell maps -- runs one handle whose five
groups span sigma dx = 1e-6 .. 1e4, at c dt / dx = 1e-4 .. 1e4, three boundary pairs, the
correction off and on, an inflow of B 10^U(-3, 3) and two start states.  On every line
(direction, group)

    max over nodes |gpu - truth| / |truth|  <=  32 max(the fp64 oracle's same error, 16 eps)

so a node far below its group's maximum counts as much as the largest one, and the bound
follows the conditioning of the reference's own recurrence.  The moments are array_equal to
the sequential sums over the device's own psi (exact: no regime tolerance).
"""
import numpy as np
import pytest

import regime_cases as rc

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not rc.HAVE_EXTENDED, reason=rc.SKIP_REASON)]

SHARD = (1, 4)


def _run(rtsn_mod, case, setup, what, shard=None):
    """One handle on the case: `setup` chooses the path and asserts that it is taken; the
    conditions on truth and oracle, the moments against the sums of the handle's own psi.
    Returns (what, the error ratio of every line) for _verdict."""
    kw = {} if shard is None else dict(g_lo=shard[0], g_hi=shard[1])
    sl = slice(None) if shard is None else slice(*shard)
    if case.regions is not None:
        kw["regions"] = case.regions
    with rtsn_mod.Solver(case.q, **kw) as s:
        setup(s)
        if case.ends0 is not None:
            s.set_ends(case.ends0[:, sl])
        s.advance(case.steps)
        ends, psi, moments = s.ends(), s.psi(), s.moments()
    assert np.isfinite(ends).all(), what
    for got, want in zip(moments, rc.sequential_moments(psi, case.mu, case.wt)):
        assert np.array_equal(got, want), what
    return what, rc.ratio(ends, case, sl)


def _verdict(path, runs, cases):
    """The figures, then the bound on every line of every run."""
    err_o = np.concatenate([rc.line_err(c.oracle, c.truth).ravel() for c in cases])
    worst = max(float(r.max()) for _, r in runs)
    print(f"regime-ratio {path} max gpu/oracle error ratio {worst:.3g} "
          f"oracle error {err_o.min():.2e} .. {err_o.max():.2e}")
    missed = [(what, float(r.max()), np.argwhere(r > rc.K).tolist()) for what, r in runs if (r > rc.K).any()]
    assert not missed, missed


# ---------------------------------------------------------------------------
# the paths
# ---------------------------------------------------------------------------
def wavefront(N, cells, bc_left):
    """The wavefront chain at `cells` per lane: N = 70 at 1 is a chain of two waves (three
    for a reflective pair, which carries both halves), at 8 one wave with a ragged last lane."""
    lanes = -(-N // cells) * (2 if bc_left == 2 else 1)

    def setup(s):
        s.wavefront = 2
        s.set_wavefront_cells(cells)
        st = s.wavefront_state()
        assert st["active"] and st["cells_per_lane"] == cells and st["waves"] == -(-lanes // 64), st
        assert st["waves"] == {1: 3 if bc_left == 2 else 2, 8: 1}[cells]
    return setup


def segments(pipeline, time_block, level_waves=None):
    """The segment schedules on lines cut into at least two segments: pipelined (2) or
    aligned (0) passes of time_block steps."""
    def setup(s):
        s.wavefront = 0
        s.pipeline = pipeline
        s.time_block = time_block
        s.set_segmentation(16)
        if level_waves is not None:
            s.level_waves = level_waves
            assert s.level_waves == level_waves
        assert not s.wavefront_state()["active"] and s.pipeline == pipeline and s.time_block == time_block
        if time_block == 24:  # the level-split pass: four waves share the levels
            assert s.level_waves == 4
        assert s.sweep_geometry()[1] >= 2, s.sweep_geometry()
    return setup


def region_chain(cells, bc_left, want):
    from test_regions_gpu import region_plan

    def setup(s):
        if want:
            s.set_wavefront_cells(want)
        st = s.wavefront_state()
        assert st["active"], st
        assert (st["cells_per_lane"], st["waves"]) == region_plan(cells, bc_left == 2, want=want), st
        assert not want or st["cells_per_lane"] == want
        assert s.regions() == [0] + list(np.cumsum(cells))
    return setup


# ---------------------------------------------------------------------------
# the grid, path by path
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("ts,cfl,bc,V", rc.GRID, ids=rc.ids(rc.GRID))
def test_wavefront(rtsn_mod, oracle_mod, ts, cfl, bc, V):
    """70 cells at 1 and at 8 cells per lane (largest ratio measured on the MI355X: 8.0).
    With the cell map's coefficients formed in fp64, [2-10000-21-5.994] had 34.3: at
    c dt / dx = 1e4 the CN coefficients cancel and were up to 2e3 eps off."""
    cases = [rc.uniform_case(oracle_mod, 70, ts, cfl, bc, V, start) for start in rc.STARTS]
    runs = [_run(rtsn_mod, c, wavefront(70, cells, bc[0]), (start, cells))
            for c, start in zip(cases, rc.STARTS) for cells in (1, 8)]
    _verdict("wavefront", runs, cases)


@pytest.mark.parametrize("ts,cfl,bc,V", rc.GRID, ids=rc.ids(rc.GRID))
def test_pipelined(rtsn_mod, oracle_mod, ts, cfl, bc, V):
    """Time blocks 1 and 4 over 6 steps: a 4-step pass and a 2-step remainder."""
    cases = [rc.uniform_case(oracle_mod, 320, ts, cfl, bc, V, start) for start in rc.STARTS]
    runs = [_run(rtsn_mod, c, segments(2, tb), (start, tb)) for c, start in zip(cases, rc.STARTS) for tb in (1, 4)]
    _verdict("pipelined", runs, cases)


@pytest.mark.parametrize("ts,cfl,bc,V", rc.GRID, ids=rc.ids(rc.GRID))
def test_aligned(rtsn_mod, oracle_mod, ts, cfl, bc, V):
    """The aligned schedule: every segment swept from its stale inflow, the fold adding
    A^k delta through the propagators A^Ls (largest ratio measured on the MI355X: 27.6; 56.8 at
    [2-1-*-5.994] while the map's coefficients were formed in fp64)."""
    cases = [rc.uniform_case(oracle_mod, 320, ts, cfl, bc, V, start) for start in rc.STARTS]
    runs = [_run(rtsn_mod, c, segments(0, tb), (start, tb)) for c, start in zip(cases, rc.STARTS) for tb in (1, 4)]
    _verdict("aligned", runs, cases)


@pytest.mark.parametrize("ts,cfl,bc,V", rc.LONG_GRID, ids=rc.ids(rc.LONG_GRID))
def test_pipelined_long_blocks(rtsn_mod, oracle_mod, ts, cfl, bc, V):
    """BDF2 passes of 20 steps on one and on two waves (22 steps) and the level-split pass of
    24 (26 steps), each with a 2-step remainder (largest ratio measured on the MI355X: 10.9;
    36.3 at [3-1-*-5.994] while the map's coefficients were formed in fp64)."""
    runs, cases = [], []
    for start in rc.STARTS:
        for steps, tb, lws in ((22, 20, (1, 2)), (26, 24, (None,))):
            c = rc.uniform_case(oracle_mod, 320, ts, cfl, bc, V, start, steps)
            cases.append(c)
            runs += [_run(rtsn_mod, c, segments(2, tb, lw), (start, tb, lw)) for lw in lws]
    _verdict("pipelined-long", runs, cases)


def test_level_split_is_taken(rtsn_mod, oracle_mod):
    """What test_pipelined_long_blocks relies on: a pass of 24 steps runs level-split over
    four waves unless told otherwise."""
    c = rc.uniform_case(oracle_mod, 320, 3, 1.0, (1, 1), 0.0, "B", 22)
    with rtsn_mod.Solver(c.q) as s:
        s.wavefront = 0
        s.pipeline = 2
        s.time_block = 24
        assert s.level_waves == 4
        s.time_block = 20
        assert s.level_waves == 2


@pytest.mark.parametrize("cells", rc.REGION_CELLS, ids=lambda c: "x".join(map(str, c)))
@pytest.mark.parametrize("ts,cfl,bc_left,V", rc.REGION_GRID, ids=rc.ids(rc.REGION_GRID))
def test_regions(rtsn_mod, oracle_mod, cells, ts, cfl, bc_left, V):
    """Three regions of sigma dx = (1e-4, 1e3, 1e-2) x the group table, dx differing 4x and
    T = (1, 0.3, 3), at the plan's cells per lane and at 8, against RegionReference."""
    cases = [rc.region_case(oracle_mod, cells, ts, cfl, bc_left, V, start) for start in rc.STARTS]
    runs = [_run(rtsn_mod, c, region_chain(cells, bc_left, want), (start, want))
            for c, start in zip(cases, rc.STARTS) for want in (0, 8)]
    _verdict("regions", runs, cases)


@pytest.mark.parametrize("family", ["wavefront", "pipelined", "pipelined-long", "aligned", "regions"])
def test_group_shard(rtsn_mod, oracle_mod, family):
    """A handle of the groups [1, 4) of each path family, against the same truth's slice."""
    bc, V, start = (2, 1), 5.994, "random"
    if family == "wavefront":
        c, setup = rc.uniform_case(oracle_mod, 70, 3, 1e2, bc, V, start), wavefront(70, 1, 2)
    elif family == "pipelined":
        c, setup = rc.uniform_case(oracle_mod, 320, 3, 1e2, bc, V, start), segments(2, 4)
    elif family == "pipelined-long":
        c, setup = rc.uniform_case(oracle_mod, 320, 3, 1.0, bc, V, start, 22), segments(2, 20, 2)
    elif family == "aligned":
        c, setup = rc.uniform_case(oracle_mod, 320, 3, 1e2, bc, V, start), segments(0, 4)
    else:
        cells = rc.REGION_CELLS[0]
        c, setup = rc.region_case(oracle_mod, cells, 3, 1e2, 2, V, start), region_chain(cells, 2, 8)
    _verdict(family + "-shard", [_run(rtsn_mod, c, setup, family, shard=SHARD)], [c])


@pytest.mark.parametrize("cfl", [1e-4, 1e4])
@pytest.mark.parametrize("M", [16, 32, 64])
def test_moments_forms(rtsn_mod, oracle_mod, M, cfl):
    """Where M / 2 is 8, 16 or 32 both moments forms exist: on a state spread over the
    regime's decades each is array_equal to the sequential sums over the device's own psi."""
    p = rc.medium(oracle_mod, 70, 3, cfl, (2, 1), 5.994)
    q = dict(rc.to_rt(p), M=M, psi_source=np.tile(p["psi_source"], (M // rc.M, 1)))
    ends0 = np.tile(rc.start_state("random", 70), (M // rc.M, 1, 1, 1))
    with rtsn_mod.Solver(q) as s:
        s.set_ends(ends0)
        s.advance(rc.STEPS)
        psi = s.psi()
        assert np.isfinite(psi).all() and np.abs(psi).max() / np.abs(psi).min() > 1e6
        want = rc.sequential_moments(psi, *s.quad())
        for form in (1, 0):
            s.set_moments_form(form)
            for got, w in zip(s.moments(), want):
                assert np.array_equal(got, w), form
