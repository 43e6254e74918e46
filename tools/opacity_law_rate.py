"""Cost of the opacity law's line walk (sweep_walk_law_kernel, rt_material_set_opacity_law) beside
the map walk (sweep_walk_kernel) on the same handle shape: ms per coupled sweep and per whole
coupled step.  The map walk applies a cell map held in registers; the law walk forms each cell's
line constants from sigma0 f(x) (one to three fp64 divisions per cell and scheme) and runs the
reference algebra.  The shapes are tools/regions_coupled_segments_rate.py's:
  a   G = 16, M = 8 (64 lines per half: one walk workgroup per half), N = 4096
  c   G = 128, M = 16 (1024 lines per half: 16 walk workgroups per half), N = 4096
each with BE, CN and BDF2, the slab cut into two identical regions, T(x) a sine profile.  The law
handle takes exponent 0 (f = 1: the cost does not depend on f), so both handles compute the same
steps and their T(x) must agree to rounding (rtol 1e-9 asserted where the map walk's own T stays
finite and positive over the run, "T_compared"; the tests hold 1e-12).
Per case ONE process holds both handles and alternates them: 10 warm-up steps each, then 5 rounds
of 200 steps per handle -- the sweep's launch alone from rt_set_profiling / rt_get_sweep_time
(median, least and most of the 5 rounds) and the wall time per whole step.  No threshold is set.

  python tools/opacity_law_rate.py          every case, each in a child process of its own under
                                            `timeout -k 10`, stopping at the first that fails; one
                                            JSON line per case appended to profiles/opacity_law_rate.jsonl
  python tools/opacity_law_rate.py CASE     that case alone, its JSON line on stdout"""
import json
import statistics
import subprocess
import sys
import time
from pathlib import Path

import numpy as np

REPO = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(REPO / "radiative-transfer_amd"))

STEPS, WARM, ROUNDS = 200, 10, 5
X_PER_CELL = 0.4 / 512
SHAPES = {"a": (16, 8, 4096), "c": (128, 16, 4096)}  # name: (G, M, N)
SCHEMES = {"be": (1, 1e-3), "cn": (2, 1e-3), "bdf2": (3, 1e-4)}
CASES = {f"{sh}_{sc}": (sh, sc, 240) for sh in SHAPES for sc in SCHEMES}  # ... the child's time limit in seconds
OUT = REPO / "profiles" / "opacity_law_rate.jsonl"


def params(rtsn, G, M, N, ts, dt):
    q = rtsn.params_default()
    q.update(M=M, G=G, N=N, X=X_PER_CELL * N, efirst=0.1, elast=10.0, bc_left_indicator=0, bc_right_indicator=0,
             use_mg_equilib=0, rho=1.0, kappa_grey=10.0, T=1.0, V=0.0, use_correction=0, ts_method=ts, dt=dt,
             max_timesteps=1, include_validation=0)
    q["psi_source"] = np.zeros((M, G))
    return q


def profile(N):
    x = (np.arange(N) + 0.5) / N
    return 1.0 + 0.3 * np.sin(2.0 * np.pi * x)


def timed_round(s):
    s.set_profiling(True)  # (zeroes the handle's sweep time and launch count)
    t0 = time.perf_counter()
    s.material_step(STEPS)
    s.synchronize()
    wall = time.perf_counter() - t0
    ms, launches = s.sweep_time()
    s.set_profiling(False)
    assert launches == STEPS, launches  # one launch per coupled sweep, map or law
    return ms / STEPS, 1e3 * wall / STEPS


def run_case(name):
    import rtsn
    shape, scheme, _ = CASES[name]
    G, M, N = SHAPES[shape]
    ts, dt = SCHEMES[scheme]
    q = params(rtsn, G, M, N, ts, dt)
    regions = [dict(cells=N // 2, width=X_PER_CELL * N / 2, rho=q["rho"], kappa_grey=q["kappa_grey"], T=q["T"],
                    group_kappa=None)] * 2
    handles = {}
    try:
        for k in ("map", "law"):
            s = handles[k] = rtsn.Solver(q, regions=regions)
            if s.wavefront_state()["active"]:
                s.wavefront = 0  # chain mode -> segment mode
            assert not s.wavefront_state()["active"]
            s.material_enable_segments([5.0, 5.0], profile(N))
            if k == "law":
                s.material_set_opacity_law([0.0, 0.0], [1.0, 1.0], 1e-3, 1e3)
        segments = handles["law"].sweep_geometry()[1]
        for s in handles.values():
            s.material_step(WARM)
            s.synchronize()
        sweep = {k: [] for k in handles}
        wall = {k: [] for k in handles}
        for _ in range(ROUNDS):  # alternating: what disturbs one handle's round disturbs the other's neighbour
            for k, s in handles.items():
                a, b = timed_round(s)
                sweep[k].append(a)
                wall[k].append(b)
        T = {k: s.temperature() for k, s in handles.items()}
    finally:
        for s in handles.values():
            s.close()
    # the state is compared where the map walk (the parent's kernel) itself stays physical: over the
    # run's 1010 steps CN and BDF2 at c dt / dx = 38 .. 380 need not (neither scheme is positive)
    physical = bool(np.isfinite(T["map"]).all() and (T["map"] > 0).all())
    if physical:
        np.testing.assert_allclose(T["law"], T["map"], rtol=1e-9)
    out = {"case": name, "G": G, "M": M, "N": N, "scheme": scheme, "steps": STEPS, "rounds": ROUNDS,
           "segments": segments, "workgroups": (M // 2 * G + 63) // 64 * 2, "T_compared": physical}
    for k in handles:
        out[k] = dict(sweep_ms=round(statistics.median(sweep[k]), 5), sweep_ms_min=round(min(sweep[k]), 5),
                      sweep_ms_max=round(max(sweep[k]), 5), wall_ms_per_step=round(statistics.median(wall[k]), 5))
    out["law_over_map_sweep"] = round(out["law"]["sweep_ms"] / out["map"]["sweep_ms"], 4)
    out["law_over_map_step"] = round(out["law"]["wall_ms_per_step"] / out["map"]["wall_ms_per_step"], 4)
    return out


def main():
    if len(sys.argv) > 1:
        print(json.dumps(run_case(sys.argv[1])), flush=True)
        return 0
    for name, case in CASES.items():  # a fresh child per case, each under its own time limit
        r = subprocess.run(["timeout", "-k", "10", str(case[2]), sys.executable, __file__, name], capture_output=True,
                           text=True)
        sys.stderr.write(r.stderr[-2000:])
        if r.returncode != 0:
            print(f"case {name}: exit status {r.returncode}; stopping", flush=True)
            return r.returncode
        line = r.stdout.strip().splitlines()[-1]
        json.loads(line)
        print(line, flush=True)
        with open(OUT, "a") as f:
            f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
