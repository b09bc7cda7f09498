"""usage (GPU box): python scripts/tangent_profile.py [scale] [steps]      |      python scripts/tangent_profile.py fit
Tangent runs at C3 (geballe_with_diamond refined to 1.04M DOF at scale 0.43; scale 1.0 = the stock C5 mesh): GPU ms per step
(HIP events on the context's stream, last_gpu_ms) of hf_run against hf_run_tangent with 1, 2, 4 and 8 conductivity columns,
with the primal's and the tangents' mean PCG iterations per step, multigrid preconditioner.  Prints one JSON line.
Then a few steps of per-column batches (nv = 2 and 8, HF_BATCH_PER_COLUMN: nv operator values interleaved per nonzero), so
that a kernel trace holds kb_spmv<9, nv, per-column>: a stream of nv x nnz values, the traffic an assembled-K_j alternative to
k_tangent_load would need per step.  Kernel-level times: run the same command under rocprofv3 --kernel-trace --stats.
`fit`: on the stock mesh, the wall time of the 64-point kappa_sample sweep (batches of 16, 2 in flight, as bench.py runs
it) next to a kappa_sample fit to the same experiment, with both answers."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def fit_vs_sweep():
    import tempfile
    import time

    from conftest import HEATING_CSV, load_cfg
    from heatflow_amd.driver import prepare_mesh
    from heatflow_amd.fit import fit_parameters
    from heatflow_amd.geometry import build_stack
    from heatflow_amd.parameter_sweep import get_k_values, run_kappa_sweep

    cfg = load_cfg("geballe_with_diamond")
    with tempfile.TemporaryDirectory() as tmp:
        mesh = prepare_mesh(cfg, os.path.join(tmp, "mesh"), True, build_stack(cfg))
        ks = get_k_values(count=64)
        run_kappa_sweep(cfg, os.path.join(tmp, "mesh"), ks[:16], os.path.join(tmp, "warm"), exp_csv=HEATING_CSV, batch=16)
        t0 = time.perf_counter()
        rows = run_kappa_sweep(cfg, os.path.join(tmp, "mesh"), ks, os.path.join(tmp, "sweep"), exp_csv=HEATING_CSV, batch=16,
                               concurrent=2)
        sweep_s = time.perf_counter() - t0
        best = min((r for r in rows if r["status"] == "success"), key=lambda r: r["rmse"])
        out = fit_parameters(cfg, None, ("p_sample",), HEATING_CSV, mesh=mesh)
    print(json.dumps({"sweep64": {"wall_s": sweep_s, "best_k": best["k"], "best_rmse": best["rmse"], "grid_step": float(ks[1] - ks[0])},
                      "fit": {k: out[k] for k in ("values", "stderr", "rmse", "converged", "iterations", "runs", "tangent_runs", "seconds")}}))


def main():
    if len(sys.argv) > 1 and sys.argv[1] == "fit":
        return fit_vs_sweep()
    scale = float(sys.argv[1]) if len(sys.argv) > 1 else 0.43
    steps = int(sys.argv[2]) if len(sys.argv) > 2 else 20
    from conftest import build_case
    from helpers import make_problem

    cfg, stack, mesh = build_case("geballe_with_diamond", scale)
    tags = [mesh.material_tags[m] for m in ("p_sample", "p_coupler", "o_coupler", "p_ins", "o_ins", "p_diam", "o_diam", "gasket")]
    out = {"n": int(len(mesh.coords)), "steps": steps, "scale": scale}
    prob = make_problem(cfg, stack, mesh, precond=1)
    try:
        ic = float(cfg["heating"]["ic_temp"])
        prob.run(steps, [0], time_varying=[prob.bcs[3]])                       # warm-up: code objects, pools
        prob.set_state(ic)
        _, _, it = prob.run(steps, [0], time_varying=[prob.bcs[3]])
        out["hf_run"] = {"ms_per_step": prob.backend.last_gpu_ms() / steps, "iters_mean": float(np.mean(it))}
        for n_par in (1, 2, 4, 8):
            cond = [[t] for t in tags[:n_par]]
            prob.set_state(ic)
            prob.run_tangent(2, [0], conductivity=cond, time_varying=[prob.bcs[3]])   # set-up and warm-up of this width
            prob.set_state(ic)
            _, _, _, it, tit = prob.run_tangent(steps, [0], conductivity=cond, time_varying=[prob.bcs[3]])
            out[f"hf_run_tangent_{n_par}"] = {"nv": int(prob.backend.tangent_nv), "ms_per_step": prob.backend.last_gpu_ms() / steps,
                                              "iters_mean": float(np.mean(it)), "tangent_iters_mean": float(np.mean(tit))}
    finally:
        prob.close()
    prob = make_problem(cfg, stack, mesh, precond=1, amg_reuse=True)
    try:
        be = prob.backend
        g = np.stack([prob.bc_values((k + 1) * prob.dt) for k in range(3)])
        for nv in (2, 8):
            be.batch_begin(nv, True)
            for j in range(nv):
                be.batch_load_column(j)
                be.batch_set_state(j, np.full(prob.n, ic))
            be.batch_run(np.repeat(g[:, :, None], nv, axis=2))
            out[f"per_column_batch_{nv}_ms_per_step"] = be.last_gpu_ms() / 3
            be.batch_end()
    finally:
        prob.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
