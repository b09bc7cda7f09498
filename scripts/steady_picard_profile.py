"""usage (GPU box): python scripts/steady_picard_profile.py [scale]             cost of the Picard steady state at C3, multigrid
                 python scripts/steady_picard_profile.py trace [scale]       one set-up of each kind + a Picard solve + 5 steps,
                                                                             to be run under rocprofv3 --kernel-trace --stats
                 python scripts/steady_picard_profile.py kernel STATS.csv    the assembly kernels' time per launch from its stats
Steady state under kappa(T) tables (hf_steady_picard_setup / hf_steady_picard_solve) at C3 (geballe_with_diamond
refined to 1.04 M DOF at scale 0.43), multigrid, rtol 1e-10, picard_tol 1e-6.  Tables: 1/T on the pressure media, 300..800 K at 51
knots; steady boundary: the outer boundary at ic_temp, the p-side line at ic + 400 K, the o-side line at ic + 250 K.
  - constant-k yardstick: hf_steady_setup + hf_steady_solve (GPU ms of each, iterations), REPEATS times, alternated with
  - the Picard solve: sweeps, PCG iterations of every sweep, GPU ms in total and per sweep, wall seconds of set-up and solve;
  - the first 10 transient steps from the held state: iterations per step with the transient hierarchy as built at u0 and after
    a fresh hf_assemble at u_ss.
Prints one JSON line."""
import csv
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
REPEATS = 3
RTOL, PICARD_TOL, MAX_SWEEPS, MAX_IT = 1e-10, 1e-6, 30, 20000


def _setup(scale):
    from conftest import build_case
    from helpers import material_tables
    from test_steady_cpu import steady_bcs

    from heatflow_amd.bc import gather_bc_values, merge_bcs

    case = build_case("geballe_with_diamond", scale)
    cfg, stack, mesh = case
    ic = float(cfg["heating"]["ic_temp"])
    tk, trc = material_tables(stack, mesh)
    T = 300.0 + 10.0 * np.arange(51)
    tables = {mesh.material_tags[m.name]: (300.0, 10.0, tk[mesh.material_tags[m.name]] * 300.0 / T)
              for m in stack.materials if m.name.endswith("ins")}
    sb = steady_bcs(cfg, stack, mesh, ic + 400.0, ic + 250.0)
    dofs, owner, pos = merge_bcs(sb)
    for bc in sb:
        bc.update(0.0)
    return case, tk, trc, tables, sb, np.asarray(dofs), gather_bc_values(sb, owner, pos)


def _problem(case, tk, trc, bcs, **kw):
    from heatflow_amd.solver import HeatProblem

    cfg, _, mesh = case
    dt = float(cfg["timing"]["t_final"]) / int(cfg["timing"]["num_steps"])
    return HeatProblem(mesh.coords, mesh.tris, mesh.tags, tk, trc, dt, bcs, float(cfg["heating"]["ic_temp"]), precond=1, rtol=RTOL,
                       max_it=MAX_IT, **kw)


def _linear(case, tk, trc, sb, dofs, g):
    prob = _problem(case, tk, trc, sb[:3])
    try:
        be = prob.backend
        t0 = time.perf_counter()
        be.steady_setup(dofs, 1)
        t1 = time.perf_counter()
        ms_setup = be.last_gpu_ms()
        it, res = be.steady_solve(g, False, RTOL, 0.0, MAX_IT)
        t2 = time.perf_counter()
        return {"setup_gpu_ms": ms_setup, "setup_wall_s": t1 - t0, "solve_gpu_ms": be.last_gpu_ms(), "solve_wall_s": t2 - t1,
                "iters": int(it), "resid": float(res), "fallbacks": int(be.amg_info()["jacobi_fallbacks"])}
    finally:
        prob.close()


def _steps(prob, n):
    its = []
    for k in range(n):
        it, _ = prob.step((k + 1) * prob.dt)
        its.append(int(it))
    return its


def _picard(case, tk, trc, tables, sb, dofs, g, transient=False):
    prob = _problem(case, tk, trc, sb[:3], kappa_tables=tables)
    try:
        be = prob.backend
        t0 = time.perf_counter()
        be.steady_picard_setup(dofs, 1)
        t1 = time.perf_counter()
        ms_setup = be.last_gpu_ms()
        info = be.steady_picard_solve(g, False, RTOL, 0.0, MAX_IT, PICARD_TOL, MAX_SWEEPS)
        t2 = time.perf_counter()
        ms = be.last_gpu_ms()
        out = dict(info, setup_gpu_ms=ms_setup, setup_wall_s=t1 - t0, solve_gpu_ms=ms, solve_wall_s=t2 - t1,
                   gpu_ms_per_sweep=ms / max(info["sweeps"], 1))
        if transient:
            u_ss = be.get_state()
            be.hold_load()
            out["steps_hierarchy_at_u0"] = _steps(prob, 10)
            out["drift_hierarchy_at_u0_K"] = float(np.abs(be.get_state() - u_ss).max())
            be.set_state(u_ss)
            be.assemble(prob.dt, prob.assembly_mode)        # tables: valued at u_ss, hierarchy rebuilt there
            out["steps_fresh_assemble_at_uss"] = _steps(prob, 10)
            out["drift_fresh_assemble_K"] = float(np.abs(be.get_state() - u_ss).max())
        out["fallbacks"] = int(be.amg_info()["jacobi_fallbacks"])
        return out
    finally:
        prob.close()


def cost(scale):
    case, tk, trc, tables, sb, dofs, g = _setup(scale)
    out = {"n": int(len(case[2].coords)), "scale": scale, "precond": "multigrid", "rtol": RTOL, "picard_tol": PICARD_TOL,
           "repeats": REPEATS, "linear": [], "picard": []}
    _linear(case, tk, trc, sb, dofs, g)                                     # warm-up (code objects, pools)
    for r in range(REPEATS):                                                # alternate the two
        out["linear"].append(_linear(case, tk, trc, sb, dofs, g))
        out["picard"].append(_picard(case, tk, trc, tables, sb, dofs, g, transient=(r == REPEATS - 1)))
    print(json.dumps(out))


def trace(scale):
    case, tk, trc, tables, sb, dofs, g = _setup(scale)
    lin = _linear(case, tk, trc, sb, dofs, g)                               # k_assemble_rows<true>
    prob = _problem(case, tk, trc, sb[:3], kappa_tables=tables)            # k_assemble_rows_kT (hf_assemble and 5 steps)
    try:
        be = prob.backend
        be.steady_picard_setup(dofs, 1)                                    # k_assemble_rows_kT_K
        info = be.steady_picard_solve(g, False, RTOL, 0.0, MAX_IT, PICARD_TOL, MAX_SWEEPS)
        be.hold_load()
        its = _steps(prob, 5)
    finally:
        prob.close()
    print(json.dumps({"linear_iters": lin["iters"], "sweeps": info["sweeps"], "iters": info["iters"], "step_iters": its}))


def kernel(stats_csv):
    with open(stats_csv) as f:
        stats = list(csv.DictReader(f))
    out = {}
    for r in stats:
        name = r["Name"].replace("(anonymous namespace)::", "").split("(")[0]
        if name.startswith("void "):
            name = name[5:]
        if "k_assemble_rows" in name:
            out[name] = {"calls": int(r["Calls"]), "avg_us": float(r["AverageNs"]) / 1e3, "min_us": float(r["MinNs"]) / 1e3,
                         "max_us": float(r["MaxNs"]) / 1e3}
    print(json.dumps(out))


def main():
    if len(sys.argv) > 1 and sys.argv[1] == "trace":
        return trace(float(sys.argv[2]) if len(sys.argv) > 2 else 0.43)
    if len(sys.argv) > 1 and sys.argv[1] == "kernel":
        return kernel(sys.argv[2])
    cost(float(sys.argv[1]) if len(sys.argv) > 1 else 0.43)


if __name__ == "__main__":
    main()
