"""Cost of the opacity table (rt_material_set_opacity_table: opacity_table_kernel ahead of the Planck
pass, the table forms of the law walk and of the material kernels) beside the power law's step and
the map walk's on the same handle shape: ms per coupled sweep and per whole coupled step.  The
table form of the walk loads one more double per row and lane (f of the lane's group, cell-major
like the emission) where the law's f is one wave-uniform load per row; the step adds the table
kernel, N G exps.  The shapes, media and timing rule are tools/opacity_law_rate.py's:
  a   G = 16, M = 8 (64 lines per half), N = 4096
  c   G = 128, M = 16 (1024 lines per half), N = 4096
each with BE, CN and BDF2.  The law handle takes exponent 0 and the table handle the all-ones
table (f = 1: the cost does not depend on f; 5 nodes, the tests' count), so all three handles
compute the same steps and their T(x) must agree to rounding (rtol 1e-9 where the map walk's own
T stays physical).  Per case ONE process holds the three handles and alternates them: 10 warm-up
steps each, then 5 rounds of 200 steps per handle.  No threshold is set.

Another commit's build (RTSN_PARENT_PKG=path/to/its/radiative-transfer_amd, lib/librtsn.so built
there) is timed by a second child per case that imports rtsn from it: its `law` step on the same
box and handle shape, the figure the table's step stands beside ("parent_law").

  python tools/opacity_table_rate.py          every case, each in a child process of its own under
                                              `timeout -k 10`, stopping at the first that fails; one
                                              JSON line per case appended to profiles/opacity_table_rate.jsonl
  python tools/opacity_table_rate.py CASE     that case alone, its JSON line on stdout"""
import json
import os
import statistics
import subprocess
import sys
from pathlib import Path

import numpy as np

REPO = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(REPO / "tools"))

from opacity_law_rate import CASES, ROUNDS, SCHEMES, SHAPES, STEPS, WARM, X_PER_CELL, params, profile, timed_round  # noqa: E402

# (after the import above, which puts this commit's package first)  RTSN_PKG: see above
sys.path.insert(0, os.environ.get("RTSN_PKG", str(REPO / "radiative-transfer_amd")))

OUT = REPO / "profiles" / "opacity_table_rate.jsonl"
NODES = np.array([0.03, 0.06, 0.3, 1.3, 2.0])


def run_case(name):
    import rtsn
    shape, scheme, _ = CASES[name]
    G, M, N = SHAPES[shape]
    ts, dt = SCHEMES[scheme]
    q = params(rtsn, G, M, N, ts, dt)
    regions = [dict(cells=N // 2, width=X_PER_CELL * N / 2, rho=q["rho"], kappa_grey=q["kappa_grey"], T=q["T"],
                    group_kappa=None)] * 2
    kinds = ("map", "law", "table") if hasattr(rtsn.Solver, "material_set_opacity_table") else ("map", "law")
    handles = {}
    try:
        for k in kinds:
            s = handles[k] = rtsn.Solver(q, regions=regions)
            if s.wavefront_state()["active"]:
                s.wavefront = 0  # chain mode -> segment mode
            assert not s.wavefront_state()["active"]
            s.material_enable_segments([5.0, 5.0], profile(N))
            if k == "law":
                s.material_set_opacity_law([0.0, 0.0], [1.0, 1.0], 1e-3, 1e3)
            if k == "table":
                s.material_set_opacity_table(NODES, np.ones((2, NODES.size, G)))
        for s in handles.values():
            s.material_step(WARM)
            s.synchronize()
        sweep = {k: [] for k in handles}
        wall = {k: [] for k in handles}
        for _ in range(ROUNDS):  # alternating: what disturbs one handle's round disturbs its neighbours'
            for k, s in handles.items():
                a, b = timed_round(s)
                sweep[k].append(a)
                wall[k].append(b)
        T = {k: s.temperature() for k, s in handles.items()}
    finally:
        for s in handles.values():
            s.close()
    physical = bool(np.isfinite(T["map"]).all() and (T["map"] > 0).all())
    if physical:
        for k in kinds[1:]:
            np.testing.assert_allclose(T[k], T["map"], rtol=1e-9)
    out = {"case": name, "G": G, "M": M, "N": N, "scheme": scheme, "steps": STEPS, "rounds": ROUNDS,
           "package": os.environ.get("RTSN_PKG", "this commit"), "T_compared": physical}
    for k in handles:
        out[k] = dict(sweep_ms=round(statistics.median(sweep[k]), 5), sweep_ms_min=round(min(sweep[k]), 5),
                      sweep_ms_max=round(max(sweep[k]), 5), wall_ms_per_step=round(statistics.median(wall[k]), 5))
    if "table" in out:
        out["table_over_law_sweep"] = round(out["table"]["sweep_ms"] / out["law"]["sweep_ms"], 4)
        out["table_over_law_step"] = round(out["table"]["wall_ms_per_step"] / out["law"]["wall_ms_per_step"], 4)
    return out


def child(name, limit, env=None):
    r = subprocess.run(["timeout", "-k", "10", str(limit), sys.executable, __file__, name], capture_output=True,
                       text=True, env=env)
    sys.stderr.write(r.stderr[-2000:])
    if r.returncode != 0:
        print(f"case {name}: exit status {r.returncode}; stopping", flush=True)
        return r.returncode, None
    return 0, json.loads(r.stdout.strip().splitlines()[-1])


def main():
    if len(sys.argv) > 1:
        print(json.dumps(run_case(sys.argv[1])), flush=True)
        return 0
    parent = os.environ.get("RTSN_PARENT_PKG")
    for name, case in CASES.items():  # a fresh child per case and library, each under its own time limit
        rc, line = child(name, case[2])
        if rc:
            return rc
        if parent:
            rc, old = child(name, case[2], dict(os.environ, RTSN_PKG=parent))
            if rc:
                return rc
            line["parent_law"] = old["law"]
            line["table_over_parent_law_sweep"] = round(line["table"]["sweep_ms"] / old["law"]["sweep_ms"], 4)
            line["table_over_parent_law_step"] = round(line["table"]["wall_ms_per_step"] / old["law"]["wall_ms_per_step"], 4)
            line["law_over_parent_law_step"] = round(line["law"]["wall_ms_per_step"] / old["law"]["wall_ms_per_step"], 4)
        print(json.dumps(line), flush=True)
        with open(OUT, "a") as f:
            f.write(json.dumps(line) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
