"""usage (GPU box): python scripts/capacity_tangent_profile.py [scale] [steps]     ms per step of a capacity tangent run
                 python scripts/capacity_tangent_profile.py trace REPS [scale]    load probes, to be run under
                                                                                  rocprofv3 --kernel-trace --stats
                 python scripts/capacity_tangent_profile.py kernel STATS.csv      the load kernels' time per launch from that run
Capacity columns of tangent runs (hf_tangent_set_capacity) at C3 (geballe_with_diamond refined to 1.04M DOF at
scale 0.43).
  - default: GPU ms per step (HIP events, last_gpu_ms) and mean PCG iterations of hf_run, of hf_run_tangent with one conductivity
    column (p_sample, the figures of DESIGN.md 3.7), with one rho_c column (p_sample.rho_c), and with both in two columns of one
    run, multigrid, in one process.
  - trace: at the state after five steps of a tangent run, REPS times each: one hf_tangent_load with one rho_c column
    (k_tangent_load<2> followed by k_tangent_load_cap<2>) and one with sixteen columns, every cell tag's rho_c in one of them
    (k_tangent_load<16> followed by k_tangent_load_cap<16>).
  - kernel: calls, mean, minimum and maximum duration per launch of every k_tangent_load / k_tangent_load_cap instantiation from
    the kernel_stats.csv of a `trace` run.
Prints one JSON line."""
import csv
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "scripts"))


def cost(scale, steps):
    from conftest import build_case
    from helpers import make_problem

    cfg, stack, mesh = build_case("geballe_with_diamond", scale)
    out = {"n": int(len(mesh.coords)), "steps": steps, "scale": scale}
    prob = make_problem(cfg, stack, mesh, precond=1)
    try:
        ic = float(cfg["heating"]["ic_temp"])
        prob.run(steps, [0], time_varying=[prob.bcs[3]])                       # warm-up: code objects, pools
        prob.set_state(ic)
        _, _, it = prob.run(steps, [0], time_varying=[prob.bcs[3]])
        out["hf_run"] = {"ms_per_step": prob.backend.last_gpu_ms() / steps, "iters_mean": float(np.mean(it))}
        tag = mesh.material_tags["p_sample"]
        runs = [("k_1", dict(conductivity=[[tag]])), ("rho_c_1", dict(capacity=[[tag]])),
                ("k_1_rho_c_1", dict(conductivity=[[tag], []], capacity=[[], [tag]]))]
        for label, kw in runs:
            prob.set_state(ic)
            prob.run_tangent(2, [0], time_varying=[prob.bcs[3]], **kw)          # set-up and warm-up of this width
            prob.set_state(ic)
            _, _, _, it, tit = prob.run_tangent(steps, [0], time_varying=[prob.bcs[3]], **kw)
            out[label] = {"nv": int(prob.backend.tangent_nv), "ms_per_step": prob.backend.last_gpu_ms() / steps,
                          "iters_mean": float(np.mean(it)), "tangent_iters_mean": float(np.mean(tit)),
                          "tangent_iters_per_column": [float(v) for v in np.mean(tit, axis=0)]}
    finally:
        prob.close()
    print(json.dumps(out))


def trace(reps, scale):
    from conftest import build_case
    from helpers import make_problem

    cfg, stack, mesh = build_case("geballe_with_diamond", scale)
    tags = sorted(mesh.material_tags.values())
    prob = make_problem(cfg, stack, mesh, precond=1)
    try:
        for cap in ([[mesh.material_tags["p_sample"]]], [[t] for t in tags] + [[] for _ in range(16 - len(tags))]):
            prob.set_state(float(cfg["heating"]["ic_temp"]))
            prob.run_tangent(5, [0], capacity=cap, time_varying=[prob.bcs[3]])
            for _ in range(reps):
                prob.tangent_load(0)
    finally:
        prob.close()
    print(json.dumps({"n": int(len(mesh.coords)), "reps": reps}))


def kernel(stats_csv):
    from aniso_profile import _kernel_name

    with open(stats_csv) as f:
        stats = list(csv.DictReader(f))
    out = {}
    for r in stats:
        name = _kernel_name(r["Name"])
        if name.startswith("k_tangent_load"):
            out[name] = {"calls": int(r["Calls"]), "avg_us": float(r["AverageNs"]) / 1e3, "min_us": float(r["MinNs"]) / 1e3,
                         "max_us": float(r["MaxNs"]) / 1e3}
    print(json.dumps(dict(sorted(out.items()))))


def main():
    if len(sys.argv) > 1 and sys.argv[1] == "trace":
        return trace(int(sys.argv[2]), float(sys.argv[3]) if len(sys.argv) > 3 else 0.43)
    if len(sys.argv) > 1 and sys.argv[1] == "kernel":
        return kernel(sys.argv[2])
    cost(float(sys.argv[1]) if len(sys.argv) > 1 else 0.43, int(sys.argv[2]) if len(sys.argv) > 2 else 20)


if __name__ == "__main__":
    main()
