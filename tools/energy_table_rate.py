"""Cost of the energy table (rt_material_set_energy_table: the EOS forms of material_update_kernel)
beside the same handle's update with the constant rho_cv: ms per rt_material_update (the update
kernel and the Planck pass behind it, host call to stream idle) on a coupled region handle in
segment mode, G = 16, M = 8, N = 16384 cells in two regions, BE.  [q, b] is the tool's own, so that
every cell takes one path:
  linear   q = 1, b = 1: dT ~ 2e-4 T, every cell on the linear emission (with the table: a root
           solve, log and exp per iteration, in place of one division)
  full     q = 5000, b = 1: dT ~ T, every cell solves the full emission (the Planck sums over all G
           groups per iteration either way; the table adds e(t) and c_v(t))
The table is energy = rho_cv x T_grid on 4 nodes, the constant heat capacity, so both handles compute
the same update and their T(x) must agree (rtol 1e-9); the paths are checked by
rt_get_material_last_dt.  Per case ONE process holds both handles and alternates them: per
repetition the handle is enabled again from the same T0 (which clears the table: it is set again),
then one update is timed; 5 warm-up repetitions, then 40.  No threshold is set.

  python tools/energy_table_rate.py          every case, each in a child process of its own under
                                             `timeout -k 10`, stopping at the first that fails; one
                                             JSON line per case appended to profiles/energy_table_rate.jsonl
  python tools/energy_table_rate.py CASE     that case alone, its JSON line on stdout"""
import json
import statistics
import subprocess
import sys
import time
from pathlib import Path

import numpy as np

REPO = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(REPO / "tools"))

from opacity_law_rate import X_PER_CELL, params, profile  # noqa: E402  (puts this commit's package on the path)

OUT = REPO / "profiles" / "energy_table_rate.jsonl"
G, M, N = 16, 8, 16384
WARM, REPS = 5, 40
RHO_CV = (5.0, 5.0)
NODES = np.array([0.03, 0.1, 0.4, 2.0])
CASES = {"linear": (1.0, 120), "full": (5000.0, 120)}  # name: (q, the child's time limit in seconds)


def run_case(name):
    import torch

    import rtsn
    qv, _ = CASES[name]
    q = params(rtsn, G, M, N, 1, 1e-3)
    regions = [dict(cells=N // 2, width=X_PER_CELL * N / 2, rho=q["rho"], kappa_grey=q["kappa_grey"], T=q["T"],
                    group_kappa=None)] * 2
    T0 = profile(N)
    qb = torch.cat([torch.full((N,), qv, dtype=torch.float64, device="cuda"),
                    torch.ones(N, dtype=torch.float64, device="cuda")])
    torch.cuda.synchronize()
    table = (NODES, np.outer(RHO_CV, NODES))
    handles, ms, T, full = {}, {"constant": [], "table": []}, {}, {}
    try:
        for k in ms:
            s = handles[k] = rtsn.Solver(q, regions=regions)
            if s.wavefront_state()["active"]:
                s.wavefront = 0  # chain mode -> segment mode
        for rep in range(WARM + REPS):  # alternating: what disturbs one handle disturbs its neighbour
            for k, s in handles.items():
                s.material_enable_segments(RHO_CV, T0)
                if k == "table":
                    s.material_set_energy_table(*table)
                s.synchronize()
                t0 = time.perf_counter()
                s.material_update(qb)
                s.synchronize()
                if rep >= WARM:
                    ms[k].append(1e3 * (time.perf_counter() - t0))
        for k, s in handles.items():
            T[k] = s.temperature()
            full[k] = int((s.material_last_dT() == 0.0).sum())
    finally:
        for s in handles.values():
            s.close()
    want = N if name == "full" else 0
    assert full["constant"] == want and full["table"] == want, full
    np.testing.assert_allclose(T["table"], T["constant"], rtol=1e-9)
    out = {"case": name, "G": G, "M": M, "N": N, "reps": REPS, "cells_on_full_emission": want}
    for k, v in ms.items():
        out[k] = dict(update_ms=round(statistics.median(v), 5), update_ms_min=round(min(v), 5),
                      update_ms_max=round(max(v), 5))
    out["table_over_constant"] = round(out["table"]["update_ms"] / out["constant"]["update_ms"], 4)
    return out


def main():
    if len(sys.argv) > 1:
        print(json.dumps(run_case(sys.argv[1])), flush=True)
        return 0
    for name, case in CASES.items():  # a fresh child per case, each under its own time limit
        r = subprocess.run(["timeout", "-k", "10", str(case[1]), sys.executable, __file__, name], capture_output=True,
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
