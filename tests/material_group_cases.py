"""Case builders of the material coupling at 31-128 groups per handle -- TEST INFRASTRUCTURE ONLY
(no GPU import): tests/test_material_groups.py runs every case on the CPU pair (the C oracle
against tests/regions_material_ref.py with one region), tests/test_material_groups_gpu.py runs
the device against the oracle.

A case is a dict: its parameters in the oracle's key names (`p`), the heat capacity, the start
temperatures, the group shards (coupled through the summed [q, b]), the segmentation it asks
for and the premise it states ("seg": "multi3" >= 3 segments, "multi" >= 2, "one" == 1, "long" a
corrected segment past phi_correction_geo_kernel's 2048-cell range; "start": "warm" both heating and cooling
cells, "newton" every cell solves the full emission).

Grid A is test_material.params' 0.1..10 keV, on which the grey remainder group G-1 holds
>= 1e-6 of a c T^4; the benchmark's grid 1e-3..30 keV leaves it ~1e-9, which is
why part B is measured with compare(..., field_floor=True).
"""
from __future__ import annotations

import os
import sys

import numpy as np

from conftest import REPO
from test_material import params, t_profile

sys.path.insert(0, str(REPO))
import bench  # noqa: E402  (slab_params, material_params, KAPPA_TABLE: read, never edited)

KAPPA_LLNL = np.loadtxt(bench.KAPPA_TABLE)
RHO_CV_WARM, RHO_CV_NEWTON = 5.0, 0.5
# the Newton start: material this cold under radiation at B(1 keV).  With the llnl table the
# opaque low groups thermalise within the step and at 0.05 keV the first linear dT stays below
# T / 4 in every cell (0.13-0.23 T), so no cell would solve the full emission; at 0.02 keV all do
T_COLD = {"grey": 0.05, "llnl": 0.02}
ORACLE_THREADS = min(16, len(os.sched_getaffinity(0)))
SCHEMES = ((1, 1e-3), (2, 1e-3), (3, 1e-6))
EDGE_GROUPS = (31, 32, 33, 63, 64, 65, 96, 97, 128)


def resampled_kappa(G):
    """bench.slab_params' resampling of the llnl opacity table to G groups."""
    return KAPPA_LLNL[(np.arange(G) * len(KAPPA_LLNL)) // G]


def case(cid, part, G, M, N, ts=1, dt=1e-3, bc=(2, 0), opacity="grey", start="warm", steps=3, shards=((0, 0),),
         wgs=0, seg=None, walk=False, energy=False, floor=False, grid="A"):
    return dict(id=cid, part=part, G=G, M=M, N=N, ts=ts, dt=dt, bc=bc, opacity=opacity, start=start, steps=steps,
                shards=shards, wgs=wgs, seg=seg, walk=walk, energy=energy, floor=floor, grid=grid)


def build(oracle_mod, c):
    """(p, rho_cv, T0) of a case."""
    G, M, N = c["G"], c["M"], c["N"]
    if c["grid"] == "bench":
        b = bench.material_params(bench.slab_params(G, "v0", N=N, M=M))
        p = oracle_mod.default_params()
        p.update({k: v for k, v in b.items() if k not in ("bc_left_indicator", "bc_right_indicator")})
        p.update(bc_left=b["bc_left_indicator"], bc_right=b["bc_right_indicator"], dx=b["X"] / N)
        rho_cv = 1.0
        T0 = np.full(N, 0.1) if c["start"] == "newton" else t_profile(N)
        return p, rho_cv, T0
    p = params(oracle_mod, ts=c["ts"], dt=c["dt"], M=M, G=G, N=N, bc_left=c["bc"][0], bc_right=c["bc"][1])
    p["psi_source"] = np.linspace(0.5, 2.0, M * G).reshape(M, G)
    if c["opacity"] == "llnl":
        p["group_kappa"] = resampled_kappa(G)
        p["have_group_kappa"] = 1
    if c["start"] == "newton":
        return p, RHO_CV_NEWTON, np.full(N, T_COLD[c["opacity"]])
    return p, RHO_CV_WARM, t_profile(N)


def _cases():
    out = []
    # 1: group-count edges on a full handle
    for G in EDGE_GROUPS:
        for op in ("grey", "llnl"):
            out.append(case(f"edge-G{G}-{op}", "A1", G, 8, 130, opacity=op, wgs=64, seg="multi3"))
    # 2: schemes x quadrature x boundaries at G = 128 and 65, several segments and one
    for G in (128, 65):
        for ts, dt in SCHEMES:
            for M in (4, 16, 64, 6):
                for bc in ((0, 0), (2, 1)):
                    for seg, N, wgs in (("multi", 100, 64), ("one", 16, 1)):
                        out.append(case(f"scheme-G{G}-ts{ts}-M{M}-bc{bc[0]}{bc[1]}-{seg}", "A2", G, M, N, ts=ts, dt=dt,
                                        bc=bc, wgs=wgs, seg=seg))
    # 3: a corrected segment longer than phi_correction_geo_kernel's 2048-cell range.  A line is
    # cut into at least CUs / (2 x line groups of 64) segments of Ls cells, Ls a multiple of 16,
    # and only segments 1.. are corrected: N = 4128 with 64 line groups (M = 64, H = 32, G = 128)
    # gives Ls = 2064 and a second segment of 2064 cells, so the kernel's second range runs
    for ts, dt in ((1, 1e-3), (3, 1e-6)):
        out.append(case(f"long-ts{ts}-M64", "A3", 128, 64, 4128, ts=ts, dt=dt, bc=(2, 0), wgs=1, seg="long", walk=True))
    # 4: the Newton path over 128 groups
    for op in ("grey", "llnl"):
        out.append(case(f"newton-G128-{op}", "A4", 128, 8, 70, opacity=op, start="newton", energy=True))
    # 5: group shards coupled through the summed [q, b]
    for G, cut in ((128, 64), (128, 65), (97, 33)):
        for start in ("warm", "newton"):
            out.append(case(f"shards-G{G}-cut{cut}-{start}", "A5", G, 8, 70 if start == "newton" else 130,
                            opacity="llnl", start=start, shards=((0, cut), (cut, G)), wgs=64, seg="multi3"))
    # B: the benchmark's own configuration
    out.append(case("bench-a", "B", 128, 8, 192, start="warm", floor=True, grid="bench"))
    out.append(case("bench-a-M64", "B", 128, 64, 192, start="warm", floor=True, grid="bench"))
    out.append(case("bench-b-newton", "B", 128, 8, 192, start="newton", floor=True, grid="bench"))
    out.append(case("bench-c-shards", "B", 128, 8, 192, start="warm", shards=((0, 64), (64, 128)), floor=True,
                    grid="bench"))
    return out


CASES = _cases()
QB_CASES = [case(f"qb-G{G}-{op}", "A6", G, 8, 130, opacity=op, wgs=64, seg="multi3")
            for G in (64, 65, 128) for op in ("grey", "llnl")]


# ---------------------------------------------------------------------------
# running a case on CPU solvers (the oracle, or the numpy reference with one region)
# ---------------------------------------------------------------------------
def make_oracle(oracle_mod, p, rho_cv, T0, lo, hi):
    s = oracle_mod.OracleSolver(p, g_lo=lo, g_hi=hi)
    s.set_threads(ORACLE_THREADS)  # over lines and cells: the results do not depend on it
    s.material_enable(rho_cv, T0)
    return s


def make_reference(oracle_mod, p, rho_cv, T0, lo, hi):
    from regions_material_ref import RegionMaterialReference
    from test_regions_material import uniform_regions
    return RegionMaterialReference(oracle_mod, p, uniform_regions(p, [p["N"]]), [rho_cv], T0, g_lo=lo, g_hi=hi)


def step_coupled(solvers, steps):
    """CPU solvers (shards of one slab) stepped together, their [q, b] summed."""
    for _ in range(steps):
        qb = sum(s.material_sweep() for s in solvers)
        for s in solvers:
            s.material_update(qb)


def check_start_premise(oracle_mod, c):
    """The case's start from the oracle's first update, linearised: dT = dt q / (rho_cv + dt W b)."""
    if c["id"] not in _first_dT:
        oracle_run(oracle_mod, c)
    dT, T0 = _first_dT[c["id"]]
    if c["start"] == "newton":
        assert (dT > 0.25 * T0).all(), (c["id"], float((dT / T0).min()))  # every cell solves the full emission
    else:
        assert (dT > 0).any() and (dT < 0).any(), c["id"]  # heating and cooling cells


def q_bound(orc):
    """sum_g sigma_g (max_x phi_g + W max_x B_g) of an oracle solver after its sweep: the scale
    of q's summands, against which its error is measured (q itself cancels near equilibrium)."""
    sigma = orc.params["rho"] * orc.groups()["kappa"][orc.g_lo:orc.g_lo + orc.Gl]
    W = orc.quad()[1].sum()
    return float((sigma * (orc.moments()[0].max(axis=1) + W * orc.cell_planck().max(axis=1))).sum())


_oracle_runs, _first_dT = {}, {}


def oracle_run(oracle_mod, c):
    """The case's oracle shards after its steps (computed once, shared, left unchanged; the
    4128-cell cases' solvers, ~1 GB each, are not kept)."""
    if c["id"] in _oracle_runs:
        return _oracle_runs[c["id"]]
    p, rho_cv, T0 = build(oracle_mod, c)
    N = p["N"]
    parts = [make_oracle(oracle_mod, p, rho_cv, T0, lo, hi) for lo, hi in c["shards"]]
    W = parts[0].quad()[1].sum()
    for n in range(c["steps"]):
        qb = sum(s.material_sweep() for s in parts)
        if n == 0:
            _first_dT[c["id"]] = (p["dt"] * qb[:N] / (rho_cv + p["dt"] * W * qb[N:]), T0)
        for s in parts:
            s.material_update(qb)
    if N <= 1000:
        _oracle_runs[c["id"]] = parts
    return parts


# ---------------------------------------------------------------------------
# the field floor's conditions (part B)
# ---------------------------------------------------------------------------
def floor_conditions(solvers):
    """Of a slab's groups (the shards of one slab) under compare(..., field_floor=True): the
    share of sum_g max_x B_g carried by the groups whose psi is still measured against its own
    maximum, and the slab's groups whose floor exceeds 1e3 x their own maximum."""
    from test_material_gpu import field_floor_of
    kept, total, far = 0.0, 0.0, []
    for s in solvers:
        floor = field_floor_of(s.temperature(), s.Gl, s.g_lo + s.Gl == s.G)
        own = np.abs(s.psi()).max(axis=(0, 2))
        Bmax = s.cell_planck().max(axis=1)
        kept += float(Bmax[own >= floor].sum())
        total += float(Bmax.sum())
        far += [s.g_lo + int(g) for g in np.nonzero(floor > 1e3 * own)[0]]
    return kept / total, far


def check_floor_conditions(solvers):
    """What keeps the floor from hiding a failure: the groups measured against their own maximum
    carry >= 99% of the emission, and no group but the remainder is floored far above itself."""
    share, far = floor_conditions(solvers)
    assert share >= 0.99, share
    assert far in ([], [solvers[0].G - 1]), far


# ---------------------------------------------------------------------------
# regions (item 7)
# ---------------------------------------------------------------------------
REGION_CELLS, REGION_SCALE, REGION_RHO_CV, REGION_DX = (40, 24, 32), (1.0, 30.0, 0.1), (5.0, 0.5, 2.0), (1.0, 4.0, 0.5)
REGION_G = 72
# CN amplifies by ~ -1 where sigma c dt >> 1: with the x30 table (kappa to 3e7) the reference's own T
# goes negative within three steps at dt >= 1e-5; at 1e-6 it stays within 0.65..1.3 keV
REGION_DT = {1: 1e-3, 2: 1e-6}
REGION_CASES = [(ts, bc_left) for ts in (1, 2) for bc_left in (0, 2)]


def region_case(oracle_mod, ts, bc_left):
    """(p, regions, rho_cv, T0): three regions, each its own resampled kappa table, rho_cv and dx."""
    N = int(sum(REGION_CELLS))
    p = params(oracle_mod, ts=ts, dt=REGION_DT[ts], M=8, G=REGION_G, N=N, bc_left=bc_left, bc_right=1 if bc_left == 2 else 0)
    p["psi_source"] = np.linspace(0.5, 2.0, p["M"] * p["G"]).reshape(p["M"], p["G"])
    dx0 = p["X"] / N
    regions = [dict(cells=int(c), width=float(c * dx0 * d), rho=1.0, kappa_grey=p["kappa_grey"], T=1.0,
                    group_kappa=k * resampled_kappa(REGION_G)) for c, k, d in zip(REGION_CELLS, REGION_SCALE, REGION_DX)]
    return p, regions, REGION_RHO_CV, t_profile(N)
