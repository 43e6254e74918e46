"""Time of one material-coupled sweep on a region handle: the chain-mode step (the REG && CB
wavefront chain, rt_material_enable_regions) against the segment-mode step (the one-launch line
walk sweep_walk_kernel, rt_material_enable_segments) on the same slab.  Backward Euler, the slab
cut into two identical regions, T(x) a sine profile:
  a512, a4096   G = 16, M = 8 (64 lines per half: one walk workgroup per half), chain against walk
  b             the same slab at N = 65536: the walk alone, no chain fits
  c             G = 128, M = 16 (1024 lines per half: 16 walk workgroups per half), N = 4096,
                chain against walk
Per case ONE process holds both handles and alternates them: 10 warm-up steps each, then 5
rounds of 200 steps (rt_material_step) per handle -- ms per coupled sweep from rt_set_profiling /
rt_get_sweep_time (the sweep's launch alone; median, least and most of the 5 rounds) and the wall
time per whole step (sweep, moments, q, update, Planck).  Both handles have then run the same
steps, and their T(x) must be array_equal.

  python tools/regions_coupled_segments_rate.py          every case, each in a child process of its
                                                         own under `timeout -k 10`, stopping at the
                                                         first that fails; one JSON line per case
                                                         appended to profiles/regions_coupled_segments_rate.jsonl
  python tools/regions_coupled_segments_rate.py CASE     that case alone, its JSON line on stdout"""
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
CASES = {  # name: (G, M, N, chain too, the child's time limit in seconds)
    "a512": (16, 8, 512, True, 120),
    "a4096": (16, 8, 4096, True, 120),
    "b": (16, 8, 65536, False, 240),
    "c": (128, 16, 4096, True, 240),
}
OUT = REPO / "profiles" / "regions_coupled_segments_rate.jsonl"


def params(rtsn, G, M, N):
    q = rtsn.params_default()
    q.update(M=M, G=G, N=N, X=X_PER_CELL * N, efirst=0.1, elast=10.0, bc_left_indicator=0, bc_right_indicator=0,
             use_mg_equilib=0, rho=1.0, kappa_grey=10.0, T=1.0, V=0.0, use_correction=0, ts_method=1, dt=1e-3,
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
    assert launches == STEPS, launches  # one launch per coupled sweep, chain or walk
    return ms / STEPS, 1e3 * wall / STEPS


def run_case(name):
    import rtsn
    G, M, N, with_chain, _ = CASES[name]
    q = params(rtsn, G, M, N)
    regions = [dict(cells=N // 2, width=X_PER_CELL * N / 2, rho=q["rho"], kappa_grey=q["kappa_grey"], T=q["T"],
                    group_kappa=None)] * 2
    handles, info = {}, {}
    try:
        if with_chain:
            s = handles["chain"] = rtsn.Solver(q, regions=regions)
            s.material_enable_regions([5.0, 5.0], profile(N))
            st = s.wavefront_state()
            assert st["active"]
            info["chain"] = {"cells_per_lane": st["cells_per_lane"], "waves": st["waves"]}
        s = handles["walk"] = rtsn.Solver(q, regions=regions)
        if s.wavefront_state()["active"]:
            s.wavefront = 0  # chain mode -> segment mode
        assert not s.wavefront_state()["active"]
        s.material_enable_segments([5.0, 5.0], profile(N))
        info["walk"] = {"segments": s.sweep_geometry()[1], "workgroups": (M // 2 * G + 63) // 64 * 2}
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
    for v in T.values():
        assert np.isfinite(v).all() and (v > 0).all()
    if with_chain:
        assert np.array_equal(T["chain"], T["walk"]), "chain and walk differ"
    out = {"case": name, "G": G, "M": M, "N": N, "scheme": "BE", "steps": STEPS, "rounds": ROUNDS}
    for k in handles:
        out[k] = dict(info[k], sweep_ms=round(statistics.median(sweep[k]), 5), sweep_ms_min=round(min(sweep[k]), 5),
                      sweep_ms_max=round(max(sweep[k]), 5), wall_ms_per_step=round(statistics.median(wall[k]), 5))
    if with_chain:
        out["walk_over_chain"] = round(out["walk"]["sweep_ms"] / out["chain"]["sweep_ms"], 4)
        out["T_bitwise_equal"] = True
    return out


def main():
    if len(sys.argv) > 1:
        print(json.dumps(run_case(sys.argv[1])), flush=True)
        return 0
    for name, case in CASES.items():  # a fresh child per case, each under its own time limit
        r = subprocess.run(["timeout", "-k", "10", str(case[4]), sys.executable, __file__, name], capture_output=True,
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
