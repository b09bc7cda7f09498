"""Measurements of DESIGN.md 3.24 (the enthalpy form of the capacity) at 1.04 M DOF; needs an MI355X.

    python scripts/enthalpy_profile.py steps [out.json]
        ms per step (device events, hf_last_gpu_ms over one hf_run of 100 steps) and PCG iterations per step, multigrid, of: the
        lagged form at p = 1 and p = 3, the enthalpy form at 8 fixed sweeps and at tol = 1e-6 (cap 32); the
        tables are the tests' bump on the pressure media next to their 1/T conductivity tables
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o enthalpy -- python scripts/enthalpy_profile.py kernels [out.json]
        a run of its own: 20 alternated launches of k_assemble_rows_hT (hf_enthalpy_revalue) and k_assemble_rows_cT (one lagged
        step at p = 1 values M and A once), and 20 of k_stored_heat (hf_stored_heat) and k_monitor (hf_monitor_now)

MEASURE_SCALE (default 0.43: 1.04 M DOF) scales the mesh sizes; 8 gives the small test mesh for a rehearsal.
"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

from conftest import build_case  # noqa: E402
from enthalpy_oracle import bump_tables  # noqa: E402
from helpers import make_problem  # noqa: E402
from kappa_T_oracle import problem_inputs  # noqa: E402

SCALE = float(os.environ.get("MEASURE_SCALE", "0.43"))
STEPS = int(os.environ.get("MEASURE_STEPS", "100"))
mode = sys.argv[1]
out = {"mode": mode, "scale": SCALE}
t0 = time.time()
cfg, stack, mesh = build_case("geballe_with_diamond", SCALE)
n = len(mesh.coords)
out["n"] = n
print(f"mesh: {n} nodes in {time.time() - t0:.1f} s", flush=True)
tk, trc, dt, dofs, u0, g = problem_inputs(cfg, stack, mesh, 1)
ins = [mesh.material_tags[m.name] for m in stack.materials if m.name.endswith("ins")]
ctab = bump_tables(trc, ins)
T = 300.0 + 10.0 * np.arange(51)
ktab = {t: (300.0, 10.0, tk[t] * 300.0 / T) for t in ins}
tables = dict(rhoc_tables=ctab, kappa_tables=ktab)

if mode == "steps":
    runs = {"lagged p=1": dict(picard=1), "lagged p=3": dict(picard=3),
            "enthalpy 8 sweeps": dict(capacity_form="enthalpy", picard=8),
            "enthalpy tol=1e-6": dict(capacity_form="enthalpy", picard=32, picard_tol=1e-6)}
    for name, kw in runs.items():
        prob = make_problem(cfg, stack, mesh, precond=1, **tables, **kw)
        try:
            _, _, iters = prob.run(STEPS, time_varying=[prob.bcs[3]])
            ms = prob.backend.last_gpu_ms()
            rec = {"ms_per_step": ms / STEPS, "pcg_iterations_per_step": float(np.mean(iters)),
                   "jacobi_fallbacks": prob.backend.amg_info()["jacobi_fallbacks"]}
            if "capacity_form" in kw:
                h = prob.picard_history()
                rec.update(sweeps_mean=float(np.mean(h["sweeps"])), sweeps_max=int(np.max(h["sweeps"])),
                           last_change_max=float(np.max(h["change"])))
        finally:
            prob.close()
        out[name] = rec
        print(name, rec, flush=True)
elif mode == "kernels":
    rng = np.random.default_rng(5)
    un = 250.0 + 700.0 * rng.random(n)
    e = 250.0 + 700.0 * rng.random(n)
    enth = make_problem(cfg, stack, mesh, capacity_form="enthalpy", picard=1, **tables)
    lag = make_problem(cfg, stack, mesh, picard=1, monitors={"all": {"tags": sorted(trc), "above": 400.0}}, **tables)
    try:
        gl = lag.bc_values(lag.dt)
        for _ in range(20):           # alternated: one launch of each assembly kernel, one of each reduction
            enth.backend.enthalpy_revalue(un, e)
            lag.backend.set_state(e)
            lag.backend.step(gl, 1e-2, 0.0, 20000)     # (a loose solve: the step is here for its one k_assemble_rows_cT launch)
            enth.backend.stored_heat(300.0)
            lag.backend.monitor_now()
    finally:
        enth.close()
        lag.close()
else:
    raise SystemExit(f"unknown mode {mode!r} (steps, kernels)")

text = json.dumps(out, indent=1)
if len(sys.argv) > 2:
    with open(sys.argv[2], "w") as f:
        f.write(text + "\n")
print(text)
