"""Seeded case generators for multi-region slabs -- TEST INFRASTRUCTURE ONLY (no GPU, no
reference run: plain dicts and arrays).

tests/test_regions_gpu.py and tests/test_regions_material_gpu.py run a fixed grid in which
only rho tells the regions' opacities apart; here every case draws all the axes at once, and
every region its own opacity:

* region_case(seed) -- an uncoupled region handle on a window of llnl_slab_test's 124 groups:
  the layout (an edge unit C0 of 1, 2, 4, 8; N log-uniform up to what fits 8 waves; 1..6
  regions cut at multiples of C0, a quarter of the multi-wave cases with an edge where lane
  64 k starts), each region's dx, rho, T and opacity (its own group_kappa array: the llnl
  table times a per-group factor; the shared llnl table; or None with its own kappa_grey),
  M, the group window, the scheme, the boundary pair, the v/c correction, dt, the run length, a
  random psi_source, and the schedule: a forced cells per lane, a cap on the chain's waves, a
  random initial state, one solve() or chunked advances.  The work N x steps (x 4 for BDF2) is
  capped at 40 000 so the numpy reference takes about a second.
* region_material_case(seed) -- a coupled region handle on test_material.params' group grid:
  the same layout rule (N <= 600), G 1..8, each region's kappa_grey or its own group_kappa
  array, rho, rho_cv, the cells' temperatures (each region's own, or a noisy, sorted or flat
  profile over the slab), the scheme and dt as test_random_gpu._material_case draws them, the
  boundary pair, 1..4 steps, a forced cells per lane and sometimes a group shard.
* three_ways / three_ways_material -- one medium written three ways (table kappa with rho,
  table 2 kappa with rho / 2, None with kappa_grey: the products rho kappa_g are bitwise
  equal), with the uniform slab they must reproduce.
* tile_case(G, ts) -- the smallest heterogeneous coupled slab past one 32-group tile (G = 40)
  and past one round of 64 lanes over groups (G = 70).

REGION_SEEDS and MATERIAL_SEEDS are the seeds the GPU tests run;
tests/test_regions_cases.py asserts that they reach every kernel form.
"""
from __future__ import annotations

import numpy as np

from conftest import PRM_DIR

BC_PAIRS = [(0, 0), (1, 1), (2, 1), (2, 0), (1, 2), (0, 1), (2, 2)]  # test_random_gpu.BC_PAIRS
REGION_SEEDS = range(60)
MATERIAL_SEEDS = range(30)
WORK_CAP = 40_000
OPACITY_KINDS = ("own_table", "shared_table", "grey")

_llnl = None


def llnl_params():
    """llnl_slab_test.prm through the oracle's reader (124 groups with bounds and opacities)."""
    global _llnl
    if _llnl is None:
        import oracle
        _llnl = oracle.parse_prm(PRM_DIR / "llnl_slab_test.prm", table_dir=PRM_DIR)
    return {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in _llnl.items()}


def admissible(cells, reflective, max_waves=8):
    """{C: waves} of the chains of C = 1, 2, 4, 8 cells per lane that divide every region edge
    and fit max_waves waves (N / C lanes per line, twice that reflective)."""
    edges = np.concatenate([[0], np.cumsum(cells)])
    out = {}
    for C in (1, 2, 4, 8):
        if (edges % C).any():
            continue
        w = -(-(int(edges[-1]) // C * (2 if reflective else 1)) // 64)
        if w <= max_waves:
            out[C] = w
    return out


def _units(rng, reflective, max_cells):
    """(C0, N / C0): the edge unit and N log-uniform from C0 up to what fits 8 waves."""
    C0 = int(rng.choice([1, 2, 4, 8]))
    top = min(256 if reflective else 512, max(1, max_cells // C0))
    return C0, min(max(int(np.exp(rng.uniform(0.0, np.log(top + 1.0)))), 1), top)


def wave_edge_units(units, reflective):
    """The cell edges (in units of C cells) at which a lane 64 k of the chain starts: lane j of
    a line holds the cells from j C on; a reflective pair's chain is the mu < 0 line (lane j from
    cell N - 1 - j C down) and then the mu > 0 line."""
    used = units * (2 if reflective else 1)
    out = set()
    for lane in range(64, used, 64):
        e = lane if not reflective else (units - lane if lane < units else lane - units)
        if 0 < e < units:
            out.add(e)
    return sorted(out)


def _cut(rng, units, reflective):
    """1..6 regions cut at random units; a quarter of the multi-wave slabs with an edge exactly
    where a lane 64 k starts.  (region sizes in units, that edge placed?)"""
    R = min(int(rng.integers(1, 7)), units)
    cuts = set(int(c) for c in rng.choice(np.arange(1, units), size=R - 1, replace=False)) if R > 1 else set()
    at = wave_edge_units(units, reflective)
    wave_edge = bool(rng.random() < 0.25 and at and R > 1)
    if wave_edge:
        cuts.pop()
        cuts.add(at[int(rng.integers(len(at)))])
    edges = [0] + sorted(cuts) + [units]
    return [b - a for a, b in zip(edges[:-1], edges[1:])], wave_edge


def region_case(seed: int) -> dict:
    rng = np.random.default_rng(52000 + seed)
    p = llnl_params()
    table = p["group_kappa"]
    G = p["G"]
    M = int(rng.choice([2, 4, 6, 8, 16]))
    width = int(rng.integers(1, 13))
    g_lo = int(rng.integers(0, G - width + 1))
    g_hi = g_lo + width
    ts = int(rng.integers(1, 4))
    bc_left, bc_right = BC_PAIRS[int(rng.integers(len(BC_PAIRS)))]
    corr = bool(rng.random() < 0.5)
    V = float(rng.choice([0.0, 1.0, 5.994])) if corr else 0.0
    dt = float(10.0 ** rng.uniform(-7, -5))
    steps = int(rng.integers(1, 41))
    sub = 4 if ts == 3 else 1
    C0, units = _units(rng, bc_left == 2, 4096)
    while units * C0 * steps * sub > WORK_CAP and steps > 1:  # the reference's share: about a second
        steps = max(1, steps // 2)
    while units * C0 * steps * sub > WORK_CAP and units > 1:
        units //= 2
    sizes, wave_edge = _cut(rng, units, bc_left == 2)
    cells = [C0 * u for u in sizes]
    N = int(sum(cells))
    regions, kinds = [], []
    for c in cells:
        kind = OPACITY_KINDS[int(rng.integers(3))]
        kinds.append(kind)
        dx = float(np.exp(rng.uniform(np.log(0.002), np.log(0.03))))
        r = dict(cells=int(c), width=float(c * dx), rho=float(np.exp(rng.uniform(np.log(0.1), np.log(20.0)))),
                 T=float(np.exp(rng.uniform(np.log(0.3), np.log(3.0)))), kappa_grey=float(p["kappa_grey"]),
                 group_kappa=None)
        if kind == "own_table":  # a different array per region
            r["group_kappa"] = table * 10.0 ** rng.uniform(-1, 1, size=G)
        elif kind == "shared_table":
            r["group_kappa"] = table
        else:
            r["kappa_grey"] = float(10.0 ** rng.uniform(-1, 3))
        regions.append(r)
    p.update(N=N, X=float(sum(r["width"] for r in regions)), M=M, ts_method=ts, bc_left=bc_left, bc_right=bc_right,
             use_correction=int(corr), V=V, dt=dt, max_timesteps=steps)
    p["dx"] = p["X"] / N
    p["psi_source"] = rng.uniform(0.2, 3.0, size=(M, G))
    ok = admissible(cells, bc_left == 2)
    want = int(rng.choice(sorted(ok))) if rng.random() < 0.5 else 0
    wave_cap = int(rng.integers(min(ok.values()), 9)) if rng.random() < 0.25 else 0
    ends_factor = rng.uniform(0.5, 1.5, size=(M, width, N, 2)) if rng.random() < 0.5 else None
    chunks = None
    if rng.random() < 0.4 and steps > 1:
        cuts = sorted(set(int(c) for c in rng.integers(1, steps, size=int(rng.integers(1, 4)))))
        chunks = [b - a for a, b in zip([0] + cuts, cuts + [steps])]
    return dict(p=p, regions=regions, kinds=kinds, cells=cells, C0=C0, wave_edge=wave_edge, g_lo=g_lo, g_hi=g_hi,
                want=want, wave_cap=wave_cap, ends_factor=ends_factor, chunks=chunks, steps=steps)


def region_material_case(seed: int) -> dict:
    import oracle
    from test_material import params
    # (the stream: CN and BDF2 are not positive, and about one draw in ten of theirs rings phi and
    # then T below zero in the reference itself -- no physical state to compare; this stream's
    # MATERIAL_SEEDS all stay at T > 0, which tests/test_regions_cases.py asserts)
    rng = np.random.default_rng(53500 + seed)
    M = int(rng.choice([2, 4, 6, 8, 16]))
    G = int(rng.integers(1, 9))
    ts = int(rng.choice([1, 1, 2, 3]))
    bc_left, bc_right = BC_PAIRS[int(rng.integers(len(BC_PAIRS)))]
    dt = float(10.0 ** rng.uniform(-5, -4 if ts == 3 else -3))
    C0, units = _units(rng, bc_left == 2, 600)
    sizes, wave_edge = _cut(rng, units, bc_left == 2)
    cells = [C0 * u for u in sizes]
    N = int(sum(cells))
    regions, kinds, rho_cv = [], [], []
    for c in cells:
        kind = ("own_table", "grey")[int(rng.integers(2))]
        kinds.append(kind)
        dx = float(np.exp(rng.uniform(np.log(0.002), np.log(0.03))))
        r = dict(cells=int(c), width=float(c * dx), rho=float(np.exp(rng.uniform(np.log(0.1), np.log(20.0)))),
                 T=float(10.0 ** rng.uniform(-0.5, 1.5)), kappa_grey=float(10.0 ** rng.uniform(-1, 3)),
                 group_kappa=None)
        if kind == "own_table":
            r["group_kappa"] = 10.0 ** rng.uniform(-1, 3, size=G)
        regions.append(r)
        rho_cv.append(float(10.0 ** rng.uniform(-2, 2)))
    X = float(sum(r["width"] for r in regions))
    p = params(oracle, ts=ts, dt=dt, M=M, G=G, N=N, bc_left=bc_left, bc_right=bc_right, X=X, dx=X / N,
               efirst=float(10.0 ** rng.uniform(-2, -0.3)), elast=float(10.0 ** rng.uniform(0.7, 2)))
    p["psi_source"] = rng.uniform(0.0, 2.0, size=(M, G))
    T_cells, profile = None, "regions"
    if rng.random() < 0.5:  # a per-cell profile over the slab instead of each region's own T
        T_cells = 10.0 ** rng.uniform(-0.5, 1.5, size=N)
        profile = ("noisy", "sorted", "flat")[int(rng.integers(3))]
        if profile == "sorted":
            T_cells = np.sort(T_cells)
        elif profile == "flat":
            T_cells = np.full(N, float(T_cells[0]))
    shard = (0, 0)
    if G > 1 and rng.random() < 0.3:  # a group shard run on its own [q, b], as the reference shard is
        lo = int(rng.integers(0, G))
        shard = (lo, int(rng.integers(lo + 1, G + 1)))
    want = int(rng.choice(sorted(admissible(cells, bc_left == 2))))
    return dict(p=p, regions=regions, kinds=kinds, cells=cells, C0=C0, wave_edge=wave_edge, rho_cv=rho_cv,
                T_cells=T_cells, profile=profile, shard=shard, want=want, steps=int(rng.integers(1, 5)))


# ---------------------------------------------------------------------------
# one medium written three ways
# ---------------------------------------------------------------------------
THREE_CELLS = (40, 24, 64)
THREE_N, THREE_X = 128, 4.0  # dx = 1/32: width / cells is bitwise X / N for any cut
THREE_KAPPA, THREE_RHO = 3.0, 1.5


def _three_regions(p, G):
    k, rho = THREE_KAPPA, THREE_RHO
    dx = THREE_X / THREE_N
    media = [dict(rho=rho, kappa_grey=7.0, group_kappa=np.full(G, k)),            # table kappa_g with rho
             dict(rho=rho / 2, kappa_grey=11.0, group_kappa=np.full(G, 2 * k)),   # table 2 kappa_g with rho / 2
             dict(rho=rho, kappa_grey=k, group_kappa=None)]                       # the grey grid: kappa_grey
    return [dict(cells=c, width=c * dx, T=p["T"], **m) for c, m in zip(THREE_CELLS, media)]


def three_ways(ts, bc):
    """(p of the uniform slab on llnl's group bounds with the grey table kappa_g = THREE_KAPPA,
    V = 0; the three regions)."""
    p = llnl_params()
    G = p["G"]
    p.update(N=THREE_N, X=THREE_X, dx=THREE_X / THREE_N, M=6, ts_method=ts, bc_left=bc[0], bc_right=bc[1],
             use_correction=1, V=0.0, dt=1e-6, rho=THREE_RHO, kappa_grey=7.0)
    p["group_kappa"] = np.full(G, THREE_KAPPA)
    p["psi_source"] = np.linspace(0.5, 2.0, 6 * G).reshape(6, G)
    return p, _three_regions(p, G)


def three_ways_material(ts, bc, dt):
    import oracle
    from test_material import params
    p = params(oracle, ts=ts, dt=dt, M=6, G=5, N=THREE_N, bc_left=bc[0], bc_right=bc[1], X=THREE_X,
               dx=THREE_X / THREE_N, kappa=THREE_KAPPA, rho=THREE_RHO)
    p["psi_source"] = np.linspace(0.5, 2.0, 6 * 5).reshape(6, 5)
    return p, _three_regions(p, 5)


# ---------------------------------------------------------------------------
# coupled regions past one 32-group tile and one round of 64 lanes
# ---------------------------------------------------------------------------
def tile_case(G, ts):
    """Two regions of 32 cells (N = 64, reflective left): rho x50, one with its own table and one
    grey, rho_cv x10, dx x4; t_profile with a cold block of 8 cells in the dense region."""
    import oracle
    from test_material import params, t_profile
    p = params(oracle, ts=ts, dt={1: 1e-3, 2: 1e-3, 3: 1e-4}[ts], M=6, G=G, N=64, bc_left=2, bc_right=1)
    p["psi_source"] = np.linspace(0.5, 2.0, 6 * G).reshape(6, G)
    # (region 0 the table and a kappa_grey it does not use: region 1 cannot borrow either unnoticed)
    regions = [dict(cells=32, width=32 * 0.004, rho=10.0, kappa_grey=1.0, T=1.0,
                    group_kappa=np.geomspace(3.0, 0.3, G) * (1.0 + 0.5 * np.cos(np.arange(G)))),
               dict(cells=32, width=32 * 0.016, rho=0.2, kappa_grey=40.0, T=1.0, group_kappa=None)]
    p.update(X=float(sum(r["width"] for r in regions)))
    p["dx"] = p["X"] / 64
    T0 = t_profile(64)
    T0[12:20] = 0.05
    return p, regions, (0.5, 5.0), T0
