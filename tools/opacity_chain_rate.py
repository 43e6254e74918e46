"""Cost of the opacity law's coupled step in chain mode (the law form of the wavefront chain,
rt_material_set_opacity_law_chain) beside the two steps it stands between, on the same slabs and law:
  chain   the chain-mode law step (kernels_wave.hip, the LAW forms of wavefront_kernel / chain_kernel)
  walk    the segment-mode law walk (sweep_walk_law_kernel, rt_material_set_opacity_law)
  map     the map chain with no law (the coupled chain as it was before the law form: the yardstick)
ms per coupled sweep (the one launch) and per whole coupled step.  Shapes:
  a   G = 16, M = 8    64 lines per half
  c   G = 128, M = 16  1024 lines per half
with 80 cells (regions of 32 and 48) and 336 cells (160 and 176), BE, CN and BDF2, T(x) a sine
profile.  The law handles take exponent 0 (f = 1: the cost does not depend on f), so all three
compute the same steps: their T(x) must agree to rounding (rtol 1e-9 asserted where the map chain's
own T stays finite and positive, "T_compared"; the tests hold 1e-12), and chain against walk exactly
("chain_equals_walk" records whether T is array_equal; nothing is asserted on it here).
Per case ONE process holds the three handles and alternates them: 10 warm-up steps each, then 5
rounds of 200 steps per handle -- the sweep's launch alone from rt_set_profiling / rt_get_sweep_time
(median, least and most of the 5 rounds) and the wall time per whole step.  No threshold is set.

  python tools/opacity_chain_rate.py [--out FILE]   every case, each in a child process of its own
                                            under `timeout -k 10`, stopping at the first that fails;
                                            one JSON line per case appended to FILE (default
                                            profiles/opacity_chain_rate.jsonl)
  python tools/opacity_chain_rate.py CASE   that case alone, its JSON line on stdout"""
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
SHAPES = {"a": (16, 8), "c": (128, 16)}  # name: (G, M)
CELLS = {80: (32, 48), 336: (160, 176)}
SCHEMES = {"be": (1, 1e-3), "cn": (2, 1e-3), "bdf2": (3, 1e-4)}
CASES = {f"{sh}{n}_{sc}": (sh, n, sc, 120) for sh in SHAPES for n in CELLS for sc in SCHEMES}  # ... the child's time limit, s
OUT = REPO / "profiles" / "opacity_chain_rate.jsonl"


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
    assert launches == STEPS, launches  # one launch per coupled sweep, every form
    return ms / STEPS, 1e3 * wall / STEPS


def run_case(name):
    import rtsn
    shape, N, scheme, _ = CASES[name]
    G, M = SHAPES[shape]
    ts, dt = SCHEMES[scheme]
    q = params(rtsn, G, M, N, ts, dt)
    regions = [dict(cells=c, width=X_PER_CELL * c, rho=q["rho"], kappa_grey=q["kappa_grey"], T=q["T"],
                    group_kappa=None) for c in CELLS[N]]
    law = ([0.0, 0.0], [1.0, 1.0], 1e-3, 1e3)
    handles, plan = {}, {}
    try:
        for k in ("map", "chain", "walk"):
            s = handles[k] = rtsn.Solver(q, regions=regions)
            assert s.wavefront_state()["active"]
            if k == "walk":
                s.wavefront = 0  # chain mode -> segment mode
                assert not s.wavefront_state()["active"]
                s.material_enable_segments([5.0, 5.0], profile(N))
                s.material_set_opacity_law(*law)
                continue
            s.material_enable_regions([5.0, 5.0], profile(N))
            if k == "chain":
                s.material_set_opacity_law_chain(*law)
            st = s.wavefront_state()
            assert st["active"]
            plan[k] = dict(cells_per_lane=st["cells_per_lane"], waves=st["waves"])
        for s in handles.values():
            s.material_step(WARM)
            s.synchronize()
        sweep = {k: [] for k in handles}
        wall = {k: [] for k in handles}
        for _ in range(ROUNDS):  # alternating: what disturbs one handle's round disturbs the others' neighbours
            for k, s in handles.items():
                a, b = timed_round(s)
                sweep[k].append(a)
                wall[k].append(b)
        T = {k: s.temperature() for k, s in handles.items()}
    finally:
        for s in handles.values():
            s.close()
    # the state is compared where the map chain itself stays physical over the run's 1010 steps
    physical = bool(np.isfinite(T["map"]).all() and (T["map"] > 0).all())
    if physical:
        np.testing.assert_allclose(T["chain"], T["map"], rtol=1e-9)
        np.testing.assert_allclose(T["walk"], T["map"], rtol=1e-9)
    out = {"case": name, "G": G, "M": M, "N": N, "scheme": scheme, "steps": STEPS, "rounds": ROUNDS,
           "lines_per_half": M // 2 * G, "plan": plan, "T_compared": physical,
           "chain_equals_walk": bool(np.array_equal(T["chain"], T["walk"]))}
    for k in handles:
        out[k] = dict(sweep_ms=round(statistics.median(sweep[k]), 5), sweep_ms_min=round(min(sweep[k]), 5),
                      sweep_ms_max=round(max(sweep[k]), 5), wall_ms_per_step=round(statistics.median(wall[k]), 5))
    for k in ("walk", "map"):
        out[f"chain_over_{k}_sweep"] = round(out["chain"]["sweep_ms"] / out[k]["sweep_ms"], 4)
        out[f"chain_over_{k}_step"] = round(out["chain"]["wall_ms_per_step"] / out[k]["wall_ms_per_step"], 4)
    return out


def main():
    args = sys.argv[1:]
    out_file = OUT
    if args[:1] == ["--out"]:
        out_file = Path(args[1])
        args = args[2:]
    if args:
        print(json.dumps(run_case(args[0])), flush=True)
        return 0
    for name, case in CASES.items():  # a fresh child per case, each under its own time limit
        r = subprocess.run(["timeout", "-k", "10", str(case[3]), sys.executable, __file__, name], capture_output=True,
                           text=True)
        sys.stderr.write(r.stderr[-2000:])
        if r.returncode != 0:
            print(f"case {name}: exit status {r.returncode}; stopping", flush=True)
            return r.returncode
        line = r.stdout.strip().splitlines()[-1]
        json.loads(line)
        print(line, flush=True)
        with open(out_file, "a") as f:
            f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
