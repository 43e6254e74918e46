"""Multi-region slabs on long lines (include/rtsn.h "multi-region slabs", segment mode;
kernels.hip, the REG form of sweep_block_kernel): a region handle on the pipelined segment pass
with every segment inside one region.

* the chain (the default handle) against segment mode, BITWISE: every (cell, level) applies the
  same map to exact inputs in both;
* independence of the time block, the segmentation and how a run is cut into advances, bitwise;
* identical regions equal a plain handle on the pipelined schedule bitwise;
* lines beyond the chain (N = 4112; 2064 reflective) against the numpy reference of
  tests/regions_reference.py at the project's 1e-10 per group, a group shard, the balance;
* an interrupted launch resumes exactly; the statuses of segment mode; bin/transfer on a long
  three-region .prm.

Shapes: N = 320 in regions (96, 160, 64) and (48, 272) -- several segments per region, unequal
segment lengths (96 at target 64: 48 + 48; 272 at 80: 80 + 64 + 64 + 64), region edges on segment
edges, BDF2 at C = 8 (T = 3, 4, 8, 10) and C = 16 (T = 1, 12, 16), BE and CN at C = 16.
"""
import os
import subprocess

import numpy as np
import pytest

from conftest import PRM_DIR, SEED
from parity import per_group_rel
from regions_reference import LO, RegionReference
from test_regions_gpu import C_LIGHT, _params, _readouts, _regions, compare_region_handle

pytestmark = pytest.mark.gpu

G3 = (LO, LO + 3)  # three of llnl_slab_test's 124 groups
N320 = 320
# regions differ in rho by x50, in T by x3 and in dx by x4 (the contrasts of HETERO["n320_wide"])
SLABS = {
    # name: (cells, dx per region, rho, T, cells per segment to plan for (0: the segmentation's), segments)
    "three": ((96, 160, 64), (0.016, 0.004, 0.008), (0.2, 10.0, 1.0), (1.5, 0.5, 1.0), 64, 6),
    "two": ((48, 272), (0.016, 0.004), (0.2, 10.0), (1.5, 0.5), 0, 20),
}


def _slab(oracle_mod, name, ts, bc, N=N320):
    cells, dxs, rho, T = SLABS[name][:4]
    p, q = _params(oracle_mod, N, ts, bc[0], bc[1])
    return p, q, _regions(q, cells, [c * d for c, d in zip(cells, dxs)], rho, T)


def _ends0(oracle_mod, p, q, seed):
    B = oracle_mod.OracleSolver(p, g_lo=G3[0], g_hi=G3[1]).groups()["B"][G3[0]:G3[1]]
    rng = np.random.default_rng(seed)
    return B[None, :, None, None] * rng.uniform(0.5, 1.5, size=(q["M"], 3, q["N"], 2))


def _segment_mode(s, T, cells=0, wgs=8):
    """Chain mode -> segment mode at time block T; cells: rt_debug_set_segment_cells."""
    s.wavefront = 0
    st = s.wavefront_state()
    assert not st["active"] and st["mode"] == 0 and s.pipeline == 2
    s.time_block = T
    s.set_segmentation(wgs)
    if cells:
        s.debug_set_segment_cells(cells)
    return s.sweep_geometry()[1]


def _status(rtsn_mod, fn):
    with pytest.raises(rtsn_mod.RtError) as e:
        fn()
    return e.value.status


# ---------------------------------------------------------------------------
# 1: the chain against segments, bitwise
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("ts", [1, 2, 3])
@pytest.mark.parametrize("bc", [(1, 1), (0, 0), (2, 1)])
@pytest.mark.parametrize("name", sorted(SLABS))
def test_chain_against_segments_bitwise(rtsn_mod, oracle_mod, name, bc, ts):
    """11 steps from a random state on the chain, and on a second handle in segment mode at
    T = 4 (two passes and a remainder of 3): ends, psi, moments, group ends and every balance
    term are array_equal.  The three-region slab is planned at 64 cells per segment
    (48, 48 | 64, 48, 48 | 64), the two-region one by rt_set_segmentation alone (20 segments of 16)."""
    p, q, regions = _slab(oracle_mod, name, ts, bc)
    ends0 = _ends0(oracle_mod, p, q, SEED + 31 * ts + 5 * bc[0] + bc[1])
    with rtsn_mod.Solver(q, g_lo=G3[0], g_hi=G3[1], regions=regions) as s:
        assert s.wavefront_state()["active"]
        s.set_ends(ends0)
        s.advance(11)
        chain = _readouts(s)
    with rtsn_mod.Solver(q, g_lo=G3[0], g_hi=G3[1], regions=regions) as s:
        Sg = _segment_mode(s, 4, cells=SLABS[name][4])
        assert Sg == SLABS[name][5] and Sg >= 4 and Sg > len(regions)
        s.set_ends(ends0)
        s.advance(11)
        got = _readouts(s)
        assert s.pipeline_state() == {"lag_steps": 0, "queued_steps": 0, "pending": False}
    for k, v in chain.items():
        assert np.array_equal(got[k], v), k


# ---------------------------------------------------------------------------
# 2: independence of T, segmentation and cutting, bitwise
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("bc", [(0, 0), (2, 1)])
def test_independence_bitwise(rtsn_mod, oracle_mod, bc):
    """BDF2 on the (48, 272) slab, 27 steps: T of 1, 3, 8, 12, 16 (at 16: one pass and a
    remainder of 11 = 10 + 1), plans of 2, 5 and 20 segments (targets 272, 80, 16), and the run
    as 27 at once, 5 + 22 and 27 x 1 -- every read-out array_equal to the first run's."""
    p, q, regions = _slab(oracle_mod, "two", 3, bc)
    ends0 = _ends0(oracle_mod, p, q, SEED + 77 + bc[0])

    def run(T, cells, cuts, segments=None):
        with rtsn_mod.Solver(q, g_lo=G3[0], g_hi=G3[1], regions=regions) as s:
            Sg = _segment_mode(s, T, cells=cells)
            assert segments is None or Sg == segments
            s.set_ends(ends0)
            for n in cuts:
                s.advance(n)
            return _readouts(s)

    ref = run(16, 0, [27])
    variants = [(T, 0, [27], None) for T in (1, 3, 8, 12)]
    variants += [(8, 272, [27], 2), (8, 80, [27], 5), (8, 16, [27], 20), (16, 80, [27], 5)]
    variants += [(8, 80, [5, 22], 5), (8, 80, [1] * 27, 5), (16, 0, [5, 22], None), (3, 272, [1] * 27, 2)]
    for v in variants:
        got = run(*v)
        for k, want in ref.items():
            assert np.array_equal(got[k], want), (k, v)


# ---------------------------------------------------------------------------
# 3: the uniform limit
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("ts", [3, 1])
@pytest.mark.parametrize("bc", [(0, 0), (2, 1)])
def test_uniform_limit_bitwise(rtsn_mod, oracle_mod, ts, bc):
    """N = 320 cut into three identical regions (96, 160, 64) equal to the rt_params values, in
    segment mode, against the plain handle at rt_set_pipeline(2) with the same T = 4, the v/c
    correction on: 12 steps (whole passes: the plain handle's remainder would run aligned passes,
    equal only to rounding), every read-out array_equal.  dx = 1/32: width / cells is X / N
    bitwise."""
    X = 10.0
    p, q = _params(oracle_mod, N320, ts, bc[0], bc[1], X=X)
    ends0 = _ends0(oracle_mod, p, q, SEED + 91 + ts + bc[0])
    with rtsn_mod.Solver(q, g_lo=G3[0], g_hi=G3[1]) as s:
        s.wavefront = 0
        s.time_block = 4
        s.pipeline = 2
        s.set_ends(ends0)
        s.advance(12)
        plain = _readouts(s)
    cells = (96, 160, 64)
    with rtsn_mod.Solver(q, g_lo=G3[0], g_hi=G3[1], regions=_regions(q, cells, [c * X / N320 for c in cells])) as s:
        assert _segment_mode(s, 4, cells=64) == 6
        s.set_ends(ends0)
        s.advance(12)
        got = _readouts(s)
    for k, v in plain.items():
        assert np.array_equal(got[k], v), k


# ---------------------------------------------------------------------------
# 4: beyond the chain
# ---------------------------------------------------------------------------
LONG = {"n4112": ((2064, 2048), 0), "n2064_reflective": ((1040, 1024), 2)}


def _long(oracle_mod, name):
    cells, bc_left = LONG[name]
    dxs, rho, T = SLABS["two"][1:4]
    p, q = _params(oracle_mod, sum(cells), 3, bc_left, 1 if bc_left == 2 else 0)
    return p, q, _regions(q, cells, [c * d for c, d in zip(cells, dxs)], rho, T), cells, rho, T


@pytest.mark.parametrize("name", sorted(LONG))
def test_beyond_the_chain(rtsn_mod, oracle_mod, name):
    """Lines no chain admits: rt_create_regions enters segment mode by itself.  BDF2, 5 steps
    at T = 4 from the regions' own B_g against RegionReference (psi, ends, phi, phi_plus at 1e-10
    per group, F by parity.flux_rel, the group ends); the balance's outflow + absorption and
    emission shares of the vacuum slab against numpy sums of the GPU's own phi and ends (1e-12 of
    the summands' magnitudes, as tests/test_regions_gpu.py); the state finite; a group shard [1, 3) equal to
    the full handle's slice bitwise."""
    p, q, regions, cells, rho, T = _long(oracle_mod, name)
    assert _status(rtsn_mod, lambda: rtsn_mod.regions_plan(regions, q["bc_left_indicator"] == 2)) == 3
    ref = RegionReference(oracle_mod, p, regions, g_lo=G3[0], g_hi=G3[1])
    with rtsn_mod.Solver(q, g_lo=G3[0], g_hi=G3[1], regions=regions) as s:
        st = s.wavefront_state()
        assert not st["active"] and s.pipeline == 2 and s.time_block == 16
        assert s.sweep_geometry()[1] >= 2
        assert per_group_rel(s.ends(), ref.ends(), 1) <= 1e-14
        s.time_block = 4
        s.advance(5)
        for _ in range(5):
            ref.step()
        compare_region_handle(s, ref)
        assert s.state_finite()
        full = _readouts(s)
        # balance: the GPU's own phi, ends and region data in numpy sums
        mu, wt = s.quad()
        creg = np.repeat(np.arange(len(cells)), cells)
        data = [s.region_data(k) for k in range(len(cells))]
        sigma = np.stack([rho[k] * data[k]["kappa"][G3[0]:G3[1]] for k in creg], axis=1)  # (Gl, N)
        dx = np.array([data[k]["dx"] for k in creg])
        Tc = np.array([T[k] for k in creg])
    if q["bc_left_indicator"] == 0:  # (tests/test_regions_gpu.py's balance check is the vacuum slab's)
        w = (mu * wt)[:, None]
        ends = full["ends"]
        jout = np.concatenate([-(ends[mu < 0, :, 0, 0] * w[mu < 0]), ends[mu > 0, :, -1, 1] * w[mu > 0]])
        ab = sigma * full["phi"] * dx
        want = jout.sum(axis=0) + ab.sum(axis=1)
        scale = np.abs(jout).sum(axis=0) + np.abs(ab).sum(axis=1)
        e_ab = float(np.max(np.abs(full["outflow_absorption"] - want) / scale))
        em = sigma * (1.3653104e-2 * C_LIGHT) * Tc ** 4 * dx
        e_em = float(np.max(np.abs(full["emission"] - em.sum(axis=1)) / np.abs(em).sum(axis=1)))
        print({"outflow_absorption": e_ab, "emission": e_em})
        assert e_ab <= 1e-12 and e_em <= 1e-12
    with rtsn_mod.Solver(q, g_lo=G3[0] + 1, g_hi=G3[1], regions=regions) as s:
        assert not s.wavefront_state()["active"]
        s.time_block = 4
        s.advance(5)
        part = _readouts(s)
    for k in ("ends", "psi"):
        assert np.array_equal(part[k], full[k][:, 1:3]), k
    for k in ("phi", "F", "phi_plus", "left", "right", "balance", "sources", "sinks", "outflow_absorption"):
        assert np.array_equal(part[k], full[k][1:3]), k


# ---------------------------------------------------------------------------
# 5: an interrupted launch
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("bc", [(0, 0), (2, 1)])
def test_interrupted_launch_resumes(rtsn_mod, oracle_mod, bc):
    """rt_debug_fail_launch(2) during a 24-step T = 4 run on the (96, 160, 64) slab (6 segments):
    the advance returns RT_ERR_DEVICE (6), the next read-out runs the positions still owed, and
    the result is bitwise the undisturbed run's."""
    p, q, regions = _slab(oracle_mod, "three", 3, bc)
    ends0 = _ends0(oracle_mod, p, q, SEED + 55 + bc[0])

    def run(fail):
        with rtsn_mod.Solver(q, g_lo=G3[0], g_hi=G3[1], regions=regions) as s:
            assert _segment_mode(s, 4, cells=64) == 6
            s.set_ends(ends0)
            if fail:
                s.debug_fail_launch(2)
                with pytest.raises(rtsn_mod.RtError) as e:
                    s.advance(24)
                assert e.value.status == 6 and "pipelined launch" in str(e.value)
            else:
                s.advance(24)
            out = _readouts(s)
            assert s.pipeline_state() == {"lag_steps": 0, "queued_steps": 0, "pending": False}
            return out

    want, got = run(False), run(True)
    for k, v in want.items():
        assert np.array_equal(got[k], v), k


# ---------------------------------------------------------------------------
# 6: statuses in segment mode
# ---------------------------------------------------------------------------
def test_segment_mode_statuses(rtsn_mod, oracle_mod):
    """The refused and accepted calls of segment mode (9 RT_ERR_STATE), the way back to the
    chain, and a layout admissible for neither mode (3 RT_ERR_PARAM)."""
    p, q, regions = _slab(oracle_mod, "three", 3, (0, 0))
    ends0 = _ends0(oracle_mod, p, q, SEED + 66)

    def status(fn):
        return _status(rtsn_mod, fn)

    with rtsn_mod.Solver(q, g_lo=G3[0], g_hi=G3[1], regions=regions) as s:
        s.set_ends(ends0)
        s.advance(5)
        s.ends()
        s.advance(4)
        chain = _readouts(s)
    with rtsn_mod.Solver(q, g_lo=G3[0], g_hi=G3[1], regions=regions) as s:
        assert status(lambda: setattr(s, "time_block", 4)) == 9  # chain mode, as before
        assert status(lambda: s.debug_set_segment_cells(64)) == 9
        s.advance(2)
        assert status(lambda: setattr(s, "wavefront", 0)) == 9  # steps are queued on the chain
        s.finish()
        s.wavefront = 0
        assert not s.wavefront_state()["active"]
        assert status(lambda: setattr(s, "pipeline", 0)) == 9
        assert status(lambda: setattr(s, "time_block", 20)) == 9
        assert status(lambda: setattr(s, "level_waves", 2)) == 9
        assert status(lambda: s.plan_schedule(100)) == 9
        assert status(lambda: s.material_enable_regions([1.0] * 3)) == 9
        assert "segment mode" in rtsn_mod.lib().rt_last_error(s._h).decode()
        assert status(lambda: s.material_enable(1.0)) == 9
        s.time_block = 12
        assert s.time_block == 12
        s.set_segmentation(8)
        s.pipeline = 1
        assert s.pipeline == 2
        s.pipeline = 2
        assert s.map_form == 0
        s.time_block = 4
        s.set_ends(ends0)
        s.advance(5)
        s.ends()
        s.wavefront = 1
        st = s.wavefront_state()
        assert st["active"] and st["mode"] == 1
        assert status(lambda: setattr(s, "time_block", 4)) == 9  # chain mode again
        s.advance(4)
        back = _readouts(s)
    for k, v in chain.items():
        assert np.array_equal(back[k], v), k
    # admissible for neither a chain nor segments
    odd = _regions(q, (5, 508), (0.1, 0.3))
    assert status(lambda: rtsn_mod.Solver(dict(q, N=513), g_lo=G3[0], g_hi=G3[1], regions=odd)) == 3
    assert status(lambda: rtsn_mod.regions_plan_segments(odd, 64)) == 3
    # a chain-only layout (N = 50) stays refused
    cells50 = (20, 10, 20)
    with rtsn_mod.Solver(dict(q, N=50), g_lo=G3[0], g_hi=G3[1], regions=_regions(q, cells50, (0.1, 0.1, 0.1))) as s:
        assert status(lambda: setattr(s, "wavefront", 0)) == 9
        assert s.wavefront_state()["active"]


# ---------------------------------------------------------------------------
# 7: the CLI on a long three-region .prm
# ---------------------------------------------------------------------------
def test_transfer_long_regions_csv(rtsn_mod, tmp_path):
    """bin/transfer on a three-region .prm of N = 4112 cells (1024 / 2048 / 1040: no chain), 2
    steps, written beside a copy of the fixtures: exit 0 and phi.csv the Python handle's array
    through tests/test_cli.py's text path."""
    from test_cli import _bin, _run_tree, eigen_text
    run = _run_tree(tmp_path)
    text = (PRM_DIR / "regions/llnl_slab_regions.prm").read_text()
    for a, b in (("N=50", "N=4112"), ("regions/llnl_slab_regions_table.txt", "regions/long_table.txt")):
        assert a in text
        text = text.replace(a, b)
    prm_dir = tmp_path / "prm"
    (prm_dir / "regions/long.prm").write_text(text)
    (prm_dir / "regions/long_table.txt").write_text("1024 0.1 1.0 1.0 1.0\n2048 0.1 5.0 1.0 0.5\n1040 0.2 0.2 1.0 1.5\n")
    r = subprocess.run([str(_bin("transfer")), "../prm/regions/long.prm"], cwd=run, capture_output=True, text=True,
                       timeout=600, env=dict(os.environ, RTSN_QUIET="1"))
    assert r.returncode == 0, r.stderr
    ph = rtsn_mod.ParameterHandler(prm_dir / "regions/long.prm", table_dir=prm_dir)
    assert [g["cells"] for g in ph.regions] == [1024, 2048, 1040]
    with rtsn_mod.Solver(ph) as s:
        assert s.regions() == [0, 1024, 3072, 4112] and not s.wavefront_state()["active"]
        s.solve()
        phi = s.moments()[0]
    assert (run / "phi.csv").read_text() == eigen_text(phi)
