"""usage (GPU box): python scripts/shape_tangent_profile.py [scale] [steps]       ms per step of a thickness tangent run
                 python scripts/shape_tangent_profile.py trace REPS [scale]      load probes, to be run under
                                                                                rocprofv3 --kernel-trace --stats
                 python scripts/shape_tangent_profile.py kernel STATS.csv        the load kernels' time per launch from that run
Shape columns of tangent runs (hf_tangent_set_shape) at C3 (geballe_with_diamond refined to 1.04M DOF at scale
0.43).
  - default: GPU ms per step (HIP events, last_gpu_ms) and mean PCG iterations of hf_run, of hf_run_tangent with one conductivity
    column (p_sample, the figures of DESIGN.md 3.7), with one thickness column (p_sample.thickness), with both in two columns, and
    with four thickness columns (the four-slot kernel), multigrid.
  - trace: at the state after five steps of a tangent run, REPS times and per NS = 1, 2, 4 shape columns: one hf_tangent_load
    (k_tangent_load<NV> followed by k_tangent_load_shape<NS>).
  - kernel: calls, mean, minimum and maximum duration per launch of every k_tangent_load / k_tangent_load_shape instantiation
    from the kernel_stats.csv of a `trace` run.
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

THICK = ("p_sample", "p_ins", "o_ins", "p_coupler")


def _shape(cfg, mesh, count, first=0):
    from heatflow_amd.geometry import thickness_velocity

    return {first + j: thickness_velocity(cfg, m, mesh.coords[:, 0]) for j, m in enumerate(THICK[:count])}


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
        k_col = [[mesh.material_tags["p_sample"]]]
        runs = [("k_1", dict(conductivity=k_col)), ("thickness_1", dict(shape=_shape(cfg, mesh, 1))),
                ("k_1_thickness_1", dict(conductivity=k_col, shape=_shape(cfg, mesh, 1, first=1))),
                ("thickness_4", dict(shape=_shape(cfg, mesh, 4)))]
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
    prob = make_problem(cfg, stack, mesh, precond=1)
    try:
        for count in (1, 2, 4):
            prob.set_state(float(cfg["heating"]["ic_temp"]))
            prob.run_tangent(5, [0], shape=_shape(cfg, mesh, count), time_varying=[prob.bcs[3]])
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
