"""Tick time of a region chain against the uniform chain at the same (N, C, waves), measured
as tools/chain_plan.py measures ticks: 1000 BDF2 steps of llnl_slab_test's material on N-cell
vacuum lines (4 groups, M = 2: 8 lines), advance + finish + sync after an 8-step warm start,
median of 5 runs.  N = 50 (one wave, C = 1) and N = 1024 (four waves, C = 4), uniform or cut
into three regions that differ in rho (x50), T (x3) and dx (x4).
  python tools/regions_tick.py uniform|regions [--pkg DIR]  -> one JSON line per N
--pkg: the radiative-transfer_amd directory to import rtsn from (another build's uniform
handle, e.g. the parent commit's, measured by the same script)."""
import json
import sys
import time
from pathlib import Path

import numpy as np

REPO = Path(__file__).resolve().parents[1]
ARGS = sys.argv[1:]
PKG = REPO / "radiative-transfer_amd"
if "--pkg" in ARGS:
    PKG = Path(ARGS[ARGS.index("--pkg") + 1]).resolve()
    del ARGS[ARGS.index("--pkg"):ARGS.index("--pkg") + 2]
KIND = ARGS[0] if ARGS else "uniform"
sys.path.insert(0, str(PKG))
import rtsn  # noqa: E402

STEPS = 1000
pdir = REPO / "tests" / "golden" / "prm"
base = rtsn.ParameterHandler(pdir / "llnl_slab_test.prm", table_dir=str(pdir) + "/").params
CASES = {50: ((20, 10, 20), 1), 1024: ((512, 256, 256), 4)}  # N: (cells per region, C)
MEDIA = [(1.0, 1.0, 0.004), (10.0, 0.5, 0.016), (0.2, 1.5, 0.008)]  # rho, T, dx


def params(N, G=4):
    q = dict(base, N=N, max_timesteps=STEPS, dt=1e-9, bc_left_indicator=0, bc_right_indicator=0, G=G,
             group_bounds=None, group_kappa=None)
    q["psi_source"] = np.ones((q["M"], G))
    return q


def run(N):
    cells, C = CASES[N]
    q = params(N)
    kw = {}
    if KIND == "regions":
        kw["regions"] = [dict(cells=c, width=c * dx, rho=rho, kappa_grey=q["kappa_grey"], T=T, group_kappa=None)
                         for c, (rho, T, dx) in zip(cells, MEDIA)]
    with rtsn.Solver(q, **kw) as s:
        s.wavefront = 2
        s.set_wavefront_cells(C)
        st = s.wavefront_state()
        assert st["cells_per_lane"] == C and st["active"], st
        s.advance(8)
        s.finish()
        s.synchronize()
        ts = []
        for _ in range(5):
            t0 = time.perf_counter()
            s.advance(STEPS)
            s.finish()
            s.synchronize()
            ts.append(time.perf_counter() - t0)
        assert s.state_finite()
    dt = sorted(ts)[2]
    ticks = STEPS + N // C - 1
    return {"N": N, "kind": KIND, "C": C, "waves": st["waves"], "us": round(1e6 * dt, 2), "ticks": ticks,
            "ns_per_tick": round(1e9 * dt / ticks, 2), "runs_us": [round(1e6 * t, 1) for t in ts]}


for N in sorted(CASES):
    print(json.dumps(run(N)), flush=True)
