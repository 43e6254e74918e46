"""Time of one material-coupled step on a region handle (the REG && CB wavefront chain: a
one-step launch is all fill, lanes x tick), beside a plain coupled handle of the same uniform
slab (the segment pass) for context.  G = 16, M = 8, backward Euler; the slab is cut into two
identical regions:
  (i)  N = 512  at C = 8 on one wave,
  (ii) N = 4096 at C = 8 on eight waves.
Per handle: 10 warm-up steps, then 200 steps (rt_material_step) -- ms per coupled sweep from
rt_set_profiling / rt_get_sweep_time (the sweep's launches alone) and wall time per step over
the 200 (sweep, moments, q, update, Planck).
  python tools/regions_coupled_step.py  -> one JSON line per (N, kind)"""
import json
import sys
import time
from pathlib import Path

import numpy as np

REPO = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(REPO / "radiative-transfer_amd"))
import rtsn  # noqa: E402

STEPS, WARM, G, M = 200, 10, 16, 8
X_PER_CELL = 0.4 / 512


def params(N):
    q = rtsn.params_default()
    q.update(M=M, G=G, N=N, X=X_PER_CELL * N, efirst=0.1, elast=10.0, bc_left_indicator=0, bc_right_indicator=0,
             use_mg_equilib=0, rho=1.0, kappa_grey=10.0, T=1.0, V=0.0, use_correction=0, ts_method=1, dt=1e-3,
             max_timesteps=1, include_validation=0)
    q["psi_source"] = np.zeros((M, G))
    return q


def profile(N):
    x = (np.arange(N) + 0.5) / N
    return 1.0 + 0.3 * np.sin(2.0 * np.pi * x)


def run(N, kind):
    q = params(N)
    kw = {}
    if kind == "regions":
        kw["regions"] = [dict(cells=N // 2, width=X_PER_CELL * N / 2, rho=q["rho"], kappa_grey=q["kappa_grey"],
                              T=q["T"], group_kappa=None)] * 2
    with rtsn.Solver(q, **kw) as s:
        if kind == "regions":
            s.set_wavefront_cells(8)
            s.material_enable_regions([5.0, 5.0], profile(N))
        else:
            s.material_enable(5.0, profile(N))
        st = s.wavefront_state()
        s.material_step(WARM)
        s.synchronize()
        s.set_profiling(True)
        t0 = time.perf_counter()
        s.material_step(STEPS)
        s.synchronize()
        wall = time.perf_counter() - t0
        ms, launches = s.sweep_time()
        s.set_profiling(False)
        T = s.temperature()
        assert np.isfinite(T).all() and (T > 0).all()
    out = {"N": N, "kind": kind, "G": G, "M": M, "scheme": "BE", "steps": STEPS,
           "sweep_ms_per_step": round(ms / STEPS, 5), "sweep_launches_per_step": launches / STEPS,
           "wall_ms_per_step": round(1e3 * wall / STEPS, 5)}
    if kind == "regions":
        out.update(cells_per_lane=st["cells_per_lane"], waves=st["waves"])
    return out


for N in (512, 4096):
    for kind in ("regions", "plain"):
        print(json.dumps(run(N, kind)), flush=True)
