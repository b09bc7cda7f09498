"""usage (GPU box): python scripts/steady_profile.py [scale] [steps]
Steady state and pre-heated transient at C3 (geballe_with_diamond refined to 1.04M DOF at scale 0.43): times of the
steady operator's assembly + elimination, of the multigrid set-up on K_hat, of the steady solve (Jacobi and multigrid:
time and iterations), of the hold-load kernel and of one time step with and without a load.  GPU times are HIP events on
the context's stream (last_gpu_ms); set-up times are wall clock.  Prints one JSON line.  Kernel-level times: run the same
command under rocprofv3 --kernel-trace --stats."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    scale = float(sys.argv[1]) if len(sys.argv) > 1 else 0.43
    steps = int(sys.argv[2]) if len(sys.argv) > 2 else 20
    from conftest import build_case
    from heatflow_amd.bc import P1Space, RowDirichletBC, gather_bc_values, merge_bcs
    from helpers import material_tables
    from heatflow_amd.solver import HeatProblem

    cfg, stack, mesh = build_case("geballe_with_diamond", scale)
    ic = float(cfg["heating"]["ic_temp"])
    V = P1Space(mesh.coords)
    line = dict(length=abs(stack.r_sample) * 2, center=0.0)
    outer = [RowDirichletBC(V, loc, value=ic) for loc in ("left", "right", "top")]
    sb = outer + [RowDirichletBC(V, "x", coord=stack.heated_z, value=ic + 5.0, **line),
                  RowDirichletBC(V, "x", coord=stack.heated_z_oside, value=ic + 2.0, **line)]
    dofs, owner, pos = merge_bcs(sb)
    for bc in sb:
        bc.update(0.0)
    g_s = gather_bc_values(sb, owner, pos)
    tag_to_k, tag_to_rc = material_tables(stack, mesh)
    dt = float(cfg["timing"]["t_final"]) / int(cfg["timing"]["num_steps"])
    out = {"n": int(len(mesh.coords)), "steps": steps}
    prob = HeatProblem(mesh.coords, mesh.tris, mesh.tags, tag_to_k, tag_to_rc, dt, outer, ic, precond=1, max_it=400000)
    be = prob.backend
    out["nnz"] = int(be.nnz)
    try:
        for name, pc in (("jacobi", 0), ("amg", 1)):
            be.set_state(np.full(be.n, ic))
            t0 = time.perf_counter()
            be.steady_setup(dofs, pc)
            out[f"setup_{name}_s"] = time.perf_counter() - t0
            out["steady_assembly_ms"] = be.last_gpu_ms()          # K assembly + elimination + D^-1 (HIP events)
            t0 = time.perf_counter()
            it, res = be.steady_solve(g_s, False, 1e-10, 0.0, 400000)
            out[f"solve_{name}_s"] = time.perf_counter() - t0
            out[f"solve_{name}_gpu_ms"] = be.last_gpu_ms()
            out[f"solve_{name}_iters"] = it
        out["amg_hierarchy_setup_s"] = out["setup_amg_s"] - out["setup_jacobi_s"]
        u_ss = be.get_state()
        be.hold_load()
        out["hold_load_gpu_ms"] = be.last_gpu_ms()
        F_hold = be.get_load()
        g_all = np.tile(prob.bc_values(0.0), (steps, 1))
        # "load": the held state (its steps need no iteration); "half_load" and "no_load" both move away from it
        for label in ("load", "half_load", "no_load"):
            if label == "half_load":
                be.set_load(0.5 * F_hold)
            if label == "no_load":
                be.set_load(None)
            be.set_state(u_ss)
            be.run(g_all[:3], 1e-10, 0.0, 20000)                  # warm-up
            be.set_state(u_ss)
            _, iters = be.run(g_all, 1e-10, 0.0, 20000)
            out[f"step_{label}_ms"] = be.last_gpu_ms() / steps
            out[f"step_{label}_iters"] = float(np.mean(iters))
            if label == "load":
                out["drift_K"] = float(np.abs(be.get_state() - u_ss).max())
    finally:
        prob.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
