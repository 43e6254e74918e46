"""Multi-region slabs (include/rtsn.h rt_create_regions; kernels_wave.hip, the REG forms):
a slab of piecewise-constant regions, each with its own rho, kappa_g, T and dx, on the
short-line wavefront with a per-lane cell map.

* identical regions equal a plain handle BITWISE (the same map values reach the same tick
  loop; the region read-outs run the uniform kernels' operations per cell), however the slab
  is cut and whatever cells per lane the cut admits;
* heterogeneous slabs against a numpy reference (tests/regions_reference.py) built from oracle/fused_np.py: one
  LineSet per region (B, kappa, cor1..3 from the C oracle's tables at the region's rho,
  kappa, T) and sweep_step's loop with the cell's own LineSet (mirrored for mu < 0); the
  per-cell algebra of LineSet is pinned to the C oracle by tests/test_oracle.py.  Tolerance:
  the project's 1e-10 per group;
* the balance and absorption read-outs against numpy sums of the GPU's own phi;
* the interface: group shards, rt_solve, the refused calls; and bin/transfer on the
  three-region .prm fixture.
"""
import os
import subprocess

import numpy as np
import pytest

from conftest import PRM_DIR, SEED
from parity import flux_rel, per_group_rel
from regions_reference import HI, LO, RegionReference  # noqa: F401  (others import it from here)

pytestmark = pytest.mark.gpu

TOL = 1e-10
C_LIGHT = 299.79245800

TICK_VACUUM = [[79, 141, 166, 185, 225, 248, 259, 272], [126, 194, 217, 238, 306, 343, 356, 368],
               [220, 300, 323, 341, 441, 541, 560, 579], [410, 500, 532, 555, 800, 880, 910, 943]]
TICK_REFLECTIVE = [[83, 156, 173, 191, 230, 255, 266, 278], [131, 203, 222, 244, 321, 349, 363, 388],
                   [227, 307, 330, 351, 515, 551, 570, 587], [421, 529, 559, 579, 927, 977, 1001, 1046]]


def region_plan(cells, reflective, max_waves=8, want=0):
    """The plan rule: C of 1, 2, 4, 8 is admissible when it divides every region's first cell
    and N; among those whose chain (N / C lanes per line, twice that reflective) fits
    max_waves waves, `want` if it is one, else the least (1000 + lanes - 1) x tick cost."""
    edges = np.concatenate([[0], np.cumsum(cells)])
    N, best = int(edges[-1]), None
    for ci, C in enumerate((1, 2, 4, 8)):
        if (edges % C).any():
            continue
        used = N // C * (2 if reflective else 1)
        w = -(-used // 64)
        if w > max_waves:
            continue
        if C == want:
            return C, w
        cost = (1000.0 + used - 1) * (TICK_REFLECTIVE if reflective else TICK_VACUUM)[ci][w - 1]
        if best is None or cost < best[0]:
            best = (cost, C, w)
    return (best[1], best[2]) if best else (0, 0)


def _params(oracle_mod, N, ts, bc_left, bc_right, X=0.4, M=6, V=5.994, dt=1e-6):
    p = oracle_mod.parse_prm(PRM_DIR / "llnl_slab_test.prm", table_dir=PRM_DIR)
    p.update(N=N, X=X, M=M, ts_method=ts, bc_left=bc_left, bc_right=bc_right, use_correction=1, V=V, dt=dt)
    p["dx"] = p["X"] / p["N"]
    p["psi_source"] = np.linspace(0.5, 2.0, M * p["G"]).reshape(M, p["G"])
    q = dict(p, bc_left_indicator=bc_left, bc_right_indicator=bc_right)
    return p, q


def _regions(q, cells, widths, rho=None, T=None):
    R = len(cells)
    rho = [q["rho"]] * R if rho is None else rho
    T = [q["T"]] * R if T is None else T
    return [dict(cells=int(c), width=float(w), rho=float(r), kappa_grey=q["kappa_grey"], T=float(t),
                 group_kappa=q["group_kappa"]) for c, w, r, t in zip(cells, widths, rho, T)]


def _random_ends(q, B, seed):
    rng = np.random.default_rng(seed)
    return B[None, :, None, None] * rng.uniform(0.5, 1.5, size=(q["M"], HI - LO, q["N"], 2))


def _readouts(s):
    """Everything the uniform limit compares bitwise."""
    out = {"ends": s.ends(), "psi": s.psi()}
    out["phi"], out["F"], out["phi_plus"] = s.moments()
    out["left"], out["right"] = (a.copy() for a in s.compute_group_ends())
    out["balance"], out["sources"], out["sinks"] = s.compute_balance_terms()
    out["inflow"], out["outflow_absorption"], out["emission"] = s.balance_partials()
    return out


# ---------------------------------------------------------------------------
# 1, 2: identical regions -- bitwise a plain handle, however the slab is cut
# ---------------------------------------------------------------------------
UNIFORM_N, UNIFORM_X = 128, 4.0  # dx = 1/32: width / cells is bitwise X / N for any cut
_plain_cache = {}


def _plain(rtsn_mod, oracle_mod, ts, bc):
    """The plain handle's read-outs after 7 steps from a random state (computed once)."""
    if (ts, bc) not in _plain_cache:
        p, q = _params(oracle_mod, UNIFORM_N, ts, bc[0], bc[1], X=UNIFORM_X)
        B = oracle_mod.OracleSolver(p, g_lo=LO, g_hi=HI).groups()["B"][LO:HI]
        ends0 = _random_ends(q, B, SEED + 7 * ts + 3 * bc[0] + bc[1])
        with rtsn_mod.Solver(q, g_lo=LO, g_hi=HI) as s:
            s.wavefront = 2
            s.set_ends(ends0)
            s.advance(7)
            _plain_cache[(ts, bc)] = (q, ends0, _readouts(s))
    return _plain_cache[(ts, bc)]


def _run_cut(rtsn_mod, q, ends0, cells, want=0):
    widths = [c * UNIFORM_X / UNIFORM_N for c in cells]
    with rtsn_mod.Solver(q, g_lo=LO, g_hi=HI, regions=_regions(q, cells, widths)) as s:
        if want:
            s.set_wavefront_cells(want)
        st = s.wavefront_state()
        assert st["active"] and st["mode"] == 2
        assert (st["cells_per_lane"], st["waves"]) == region_plan(cells, q["bc_left_indicator"] == 2, want=want)
        assert s.regions() == [0] + list(np.cumsum(cells))
        s.set_ends(ends0)
        s.advance(7)
        return st["cells_per_lane"], _readouts(s)


@pytest.mark.parametrize("ts", [1, 2, 3])
@pytest.mark.parametrize("bc", [(0, 0), (2, 1), (1, 1)])
def test_uniform_limit_bitwise(rtsn_mod, oracle_mod, ts, bc):
    """Three identical regions equal to the rt_params values: ends, psi, moments, group ends
    and every balance term are array_equal to a plain handle on the wavefront."""
    q, ends0, ref = _plain(rtsn_mod, oracle_mod, ts, bc)
    _, got = _run_cut(rtsn_mod, q, ends0, (40, 24, 64))
    for k, v in ref.items():
        assert np.array_equal(got[k], v), k


@pytest.mark.parametrize("cuts,c_max", [((1, 64, 127), 1), ((2, 66), 2), ((4, 68), 4), ((8, 72, 120), 8)])
@pytest.mark.parametrize("bc", [(0, 0), (2, 1)])
def test_split_invariance_bitwise(rtsn_mod, oracle_mod, cuts, c_max, bc):
    """The same uniform slab cut at `cuts`: the largest admissible cells per lane is c_max; the
    plan's choice among the admissible and the forced c_max both report the C the rule
    predicts and give the plain handle's results bitwise (BDF2)."""
    q, ends0, ref = _plain(rtsn_mod, oracle_mod, 3, bc)
    cells = list(np.diff([0] + list(cuts) + [UNIFORM_N]))
    seen = set()
    for want in (0, c_max, 2 * c_max if c_max < 8 else 0):  # (2 c_max: not admissible, falls back to the plan's)
        C, got = _run_cut(rtsn_mod, q, ends0, cells, want)
        assert C <= c_max
        seen.add(C)
        for k, v in ref.items():
            assert np.array_equal(got[k], v), (k, want)
    assert c_max in seen


# ---------------------------------------------------------------------------
# 3: heterogeneous slabs against the numpy reference
# ---------------------------------------------------------------------------
def compare_region_handle(s, ref):
    """psi, ends, phi, phi_plus per group at 1e-10, F by parity.flux_rel, the group ends by
    test_gpu_parity.compare_all's metric; each figure printed before it is asserted."""
    mu, wt = ref.mu, ref.wt
    ends_r = ref.ends()
    psi_r = 0.5 * (ends_r[..., 0] + ends_r[..., 1])
    phi_r = np.einsum("i,igc->gc", wt, psi_r)
    F_r = np.einsum("i,igc->gc", mu * wt, psi_r)
    pp_r = np.einsum("i,igc->gc", wt[mu > 0], psi_r[mu > 0])
    den = ref.tables[0]["de_ave"] * C_LIGHT
    l_r = ends_r[mu < 0, :, 0, 0].sum(axis=0) / den
    r_r = ends_r[mu > 0, :, -1, 1].sum(axis=0) / den
    phi, F, pp = s.moments()
    l_g, r_g = s.compute_group_ends()
    err = {"psi": per_group_rel(s.psi(), psi_r, 1), "ends": per_group_rel(s.ends(), ends_r, 1),
           "phi": per_group_rel(phi, phi_r, 0), "phi_plus": per_group_rel(pp, pp_r, 0),
           "F": flux_rel(F, F_r, psi_r, mu, wt),
           "left_ends": float(np.max(np.abs(l_g - l_r) / np.maximum(np.abs(l_r), 1e-300))),
           "right_ends": float(np.max(np.abs(r_g - r_r) / np.maximum(np.abs(r_r), 1e-300)))}
    print(err)
    assert np.isfinite(ends_r).all()
    for k, v in err.items():
        assert v <= TOL, (k, v, err)


# regions differ in rho by x50, in T by x3 and in dx by x4
HETERO = {
    # name: (cells, dx per region, rho, T, bc_left, cells per lane to set (0: the plan's), expected (C, waves))
    "n50": ((20, 10, 20), (0.004, 0.016, 0.008), (1.0, 10.0, 0.2), (1.0, 0.5, 1.5), 0, 0, (1, 1)),
    "n32_reflective": ((5, 27), (0.004, 0.016), (10.0, 0.2), (0.5, 1.5), 2, 0, (1, 1)),
    "n130_wave_edge": ((63, 2, 65), (0.004, 0.016, 0.008), (0.2, 10.0, 1.0), (1.5, 0.5, 1.0), 0, 0, (1, 3)),
    "n320_wide": ((100, 220), (0.016, 0.004), (0.2, 10.0), (1.5, 0.5), 0, 1, (1, 5)),
    "n168_wide_pair": ((40, 128), (0.004, 0.016), (10.0, 0.2), (0.5, 1.5), 2, 1, (1, 6)),
    "n1088_head_redo": ((544, 544), (0.004, 0.016), (0.2, 10.0), (1.5, 0.5), 2, 8, (8, 5)),
}


def _hetero(rtsn_mod, oracle_mod, name, ts, V, steps, dt):
    cells, dxs, rho, T, bc_left, want, plan = HETERO[name]
    N = int(sum(cells))
    p, q = _params(oracle_mod, N, ts, bc_left, 1 if bc_left == 2 else 0, V=V, dt=dt)
    regions = _regions(q, cells, [c * d for c, d in zip(cells, dxs)], rho, T)
    ref = RegionReference(oracle_mod, p, regions)
    with rtsn_mod.Solver(q, g_lo=LO, g_hi=HI, regions=regions) as s:
        if want:
            s.set_wavefront_cells(want)
        st = s.wavefront_state()
        assert (st["cells_per_lane"], st["waves"]) == plan == region_plan(cells, bc_left == 2, want=want)
        # the initial state: every cell at its own region's B_g
        assert per_group_rel(s.ends(), ref.ends(), 1) <= 1e-14
        for k, t in enumerate(ref.tables):
            d = s.region_data(k)
            assert per_group_rel(d["B"][LO:HI], t["B"], 0) <= 1e-13 and d["dx"] == regions[k]["width"] / cells[k]
            assert np.array_equal(d["kappa"][LO:HI], t["kappa"])
        s.advance(steps)
        for _ in range(steps):
            ref.step()
        compare_region_handle(s, ref)


@pytest.mark.parametrize("V", [5.994, 0.0])
@pytest.mark.parametrize("name", sorted(HETERO))
def test_heterogeneous_reference(rtsn_mod, oracle_mod, name, V):
    """BDF2, 5 steps (3 on the 1088-cell pair) from the regions' own B_g: one wave, the
    mirrored table with the region-0 head, a region edge at a wave edge, the wide chain, the
    wide pair, and the head-redo form at C = 8 on five waves."""
    _hetero(rtsn_mod, oracle_mod, name, 3, V, 3 if name == "n1088_head_redo" else 5, 1e-6)


@pytest.mark.parametrize("ts", [1, 2])
def test_heterogeneous_reference_schemes(rtsn_mod, oracle_mod, ts):
    """BE and CN on the reflective two-region pair."""
    _hetero(rtsn_mod, oracle_mod, "n32_reflective", ts, 5.994, 7, 1e-6)


def test_heterogeneous_unmasked_ticks(rtsn_mod, oracle_mod):
    """150 steps at dt = 1e-9 on the N = 50 shape: more steps than the chain has lanes, so the
    ticks between its fill and drain run unmasked."""
    _hetero(rtsn_mod, oracle_mod, "n50", 3, 5.994, 150, 1e-9)


# ---------------------------------------------------------------------------
# 4: balance and absorption
# ---------------------------------------------------------------------------
def test_balance_and_absorption(rtsn_mod, oracle_mod):
    """On the heterogeneous N = 50 case, from the GPU's own phi, ends and region_data: the
    outflow + absorption share of rt_get_balance_partials equals the boundary outflow currents
    plus sum_c sigma_g(c) phi_g(c) dx(c), the emission share sum_c sigma_g(c) a c T(c)^4 dx(c),
    and rt_group_absorption_device sum_g sigma_g(c) phi_g(c) -- each to 1e-12 of the sum of
    the magnitudes of its summands (sums of at most 56 terms in another order: a few ulps)."""
    import torch
    cells, dxs, rho, T, bc_left, _, _ = HETERO["n50"]
    p, q = _params(oracle_mod, 50, 3, 0, 1)
    regions = _regions(q, cells, [c * d for c, d in zip(cells, dxs)], rho, T)
    with rtsn_mod.Solver(q, g_lo=LO, g_hi=HI, regions=regions) as s:
        s.advance(5)
        phi = s.moments()[0]  # (Gl, N)
        ends = s.ends()
        mu, wt = s.quad()
        fc = s.regions()
        creg = np.repeat(np.arange(len(cells)), np.diff(fc))
        data = [s.region_data(k) for k in range(len(cells))]
        sigma = np.stack([rho[k] * data[k]["kappa"][LO:HI] for k in creg], axis=1)  # (Gl, N)
        dx = np.array([data[k]["dx"] for k in creg])
        Tc = np.array([T[k] for k in creg])
        inflow, out_abs, emission = s.balance_partials()
        a_dev = torch.empty(50, dtype=torch.float64, device="cuda")
        s.group_absorption(a_dev)
        s.synchronize()
        a_dev = a_dev.cpu().numpy()
    w = (mu * wt)[:, None]
    jout_terms = np.concatenate([-(ends[mu < 0, :, 0, 0] * w[mu < 0]), ends[mu > 0, :, -1, 1] * w[mu > 0]])
    ab_terms = sigma * phi * dx
    want = jout_terms.sum(axis=0) + ab_terms.sum(axis=1)
    scale = np.abs(jout_terms).sum(axis=0) + np.abs(ab_terms).sum(axis=1)
    e_ab = float(np.max(np.abs(out_abs - want) / scale))
    em_terms = sigma * (1.3653104e-2 * C_LIGHT) * Tc ** 4 * dx
    e_em = float(np.max(np.abs(emission - em_terms.sum(axis=1)) / np.abs(em_terms).sum(axis=1)))
    e_dev = float(np.max(np.abs(a_dev - (sigma * phi).sum(axis=0)) / np.abs(sigma * phi).sum(axis=0)))
    print({"outflow_absorption": e_ab, "emission": e_em, "absorption_device": e_dev})
    assert e_ab <= 1e-12 and e_em <= 1e-12 and e_dev <= 1e-12


# ---------------------------------------------------------------------------
# 5: interface and refusals
# ---------------------------------------------------------------------------
def test_group_shard_and_solve(rtsn_mod, oracle_mod):
    """A group shard equals the full handle's slice bitwise, and rt_solve equals
    advance(max_timesteps)."""
    cells, dxs, rho, T, _, _, _ = HETERO["n32_reflective"]
    p, q = _params(oracle_mod, 32, 3, 2, 1)
    q["max_timesteps"] = 6
    regions = _regions(q, cells, [c * d for c, d in zip(cells, dxs)], rho, T)
    with rtsn_mod.Solver(q, g_lo=LO, g_hi=HI, regions=regions) as s:
        s.solve()
        full = _readouts(s)
    with rtsn_mod.Solver(q, g_lo=LO, g_hi=HI, regions=regions) as s:
        s.advance(6)
        assert np.array_equal(s.ends(), full["ends"])
    with rtsn_mod.Solver(q, g_lo=LO + 3, g_hi=LO + 7, regions=regions) as s:
        s.solve()
        part = _readouts(s)
    for k in ("ends", "psi"):
        assert np.array_equal(part[k], full[k][:, 3:7]), k
    for k in ("phi", "F", "phi_plus", "left", "right", "balance", "sources", "sinks", "outflow_absorption"):
        assert np.array_equal(part[k], full[k][3:7]), k


def test_refusals(rtsn_mod, oracle_mod):
    """The refused calls and conditions, each with its status (3 RT_ERR_PARAM, 9 RT_ERR_STATE)."""
    cells, dxs, rho, T, _, _, _ = HETERO["n50"]
    p, q = _params(oracle_mod, 50, 3, 0, 0)
    regions = _regions(q, cells, [c * d for c, d in zip(cells, dxs)], rho, T)

    def status(fn):
        with pytest.raises(rtsn_mod.RtError) as e:
            fn()
        return e.value.status

    assert status(lambda: rtsn_mod.Solver(dict(q, use_mg_equilib=1), g_lo=LO, g_hi=HI, regions=regions)) == 3
    assert status(lambda: rtsn_mod.Solver(dict(q, N=51), g_lo=LO, g_hi=HI, regions=regions)) == 3
    # N = 513 with a boundary at an odd cell: only C = 1 is admissible, and it needs 9 waves
    odd = _regions(q, (5, 508), (0.1, 0.3))
    assert status(lambda: rtsn_mod.Solver(dict(q, N=513), g_lo=LO, g_hi=HI, regions=odd)) == 3
    assert status(lambda: rtsn_mod.regions_plan(odd)) == 3
    with rtsn_mod.Solver(q, g_lo=LO, g_hi=HI, regions=regions) as s:
        assert status(lambda: s.material_enable(1.0)) == 9
        assert status(lambda: setattr(s, "time_block", 4)) == 9
        assert status(lambda: setattr(s, "pipeline", 2)) == 9
        assert status(lambda: s.set_segmentation(4)) == 9
        assert status(lambda: setattr(s, "level_waves", 2)) == 9
        assert status(lambda: setattr(s, "wavefront", 0)) == 9
        assert status(lambda: s.plan_schedule(100)) == 9
        s.wavefront = 2
        s.advance(3)  # still a working handle
        assert s.state_finite()
        assert s.wavefront_state()["active"]
    # rt_set_wavefront_waves re-plans: 128 cells cut at 1 fit one wave only as a vacuum line
    two = _regions(q, (1, 127), (0.01, 1.27))
    with rtsn_mod.Solver(dict(q, N=128), g_lo=LO, g_hi=HI, regions=two) as s:
        assert s.wavefront_state()["waves"] == 2
        assert status(lambda: setattr(s, "wavefront_waves", 1)) == 3
        assert s.wavefront_waves == 8
        s.wavefront_waves = 2
        assert s.wavefront_state()["waves"] == 2


# ---------------------------------------------------------------------------
# 6: the CLI on the three-region fixture
# ---------------------------------------------------------------------------
def test_transfer_regions_csv(rtsn_mod, tmp_path):
    """bin/transfer on tests/golden/prm/regions/llnl_slab_regions.prm writes the eight CSV files of the
    Python handle's arrays, through tests/test_cli.py's text path."""
    from test_cli import _bin, _run_tree, eigen_text, tensor_text
    run = _run_tree(tmp_path)
    prm = "../prm/regions/llnl_slab_regions.prm"
    r = subprocess.run([str(_bin("transfer")), prm], cwd=run, capture_output=True, text=True, timeout=600,
                       env=dict(os.environ, RTSN_QUIET="1"))
    assert r.returncode == 0, r.stderr
    ph = rtsn_mod.ParameterHandler(PRM_DIR / "regions/llnl_slab_regions.prm", table_dir=PRM_DIR)
    assert [g["cells"] for g in ph.regions] == [20, 10, 20]
    with rtsn_mod.Solver(ph) as s:
        assert s.regions() == [0, 20, 30, 50]
        s.solve()
        phi, F, phi_plus = s.moments()
        left, right = s.compute_group_ends()
        psi, e_ave = s.psi(), s.get_e_ave()
    x = np.concatenate([lo + (np.arange(g["cells"]) + 0.5) * (g["width"] / g["cells"])
                        for g, lo in zip(ph.regions, np.cumsum([0.0] + [g["width"] for g in ph.regions]))])
    expect = {"phi.csv": eigen_text(phi), "phi_plus.csv": eigen_text(phi_plus), "F.csv": eigen_text(F),
              "psi.csv": tensor_text(psi), "x.csv": eigen_text(x[:, None]), "e_ave.csv": eigen_text(e_ave[:, None]),
              "left_ends.csv": eigen_text(left[:, None]), "right_ends.csv": eigen_text(right[:, None])}
    for fname, text in expect.items():
        assert (run / fname).read_text() == text, fname
