"""Measurements of the region monitors for DESIGN.md 3.17 (profiles/monitor_*), at C3 (1.04 M DOF, multigrid).

    python scripts/monitor_profile.py --mode steps     hf_run of 60 steps without monitors, with them, without, with (one process,
                                                       alternated, three rounds): ms per step from HIP events, and the cost of a record
    python scripts/monitor_profile.py --mode kernel    200 hf_monitor_now calls on the same mesh, for the kernel trace:
        rocprofv3 --kernel-trace --stats -d outputs/monitor_profile/trace -o monitor -- python scripts/monitor_profile.py --mode kernel
                                                       (a run of its own; k_monitor and k_monitor_final in the *_kernel_stats.csv)
Every mode prints one JSON line.

The alternated benchmark against the parent commit (the flagship run sets no monitors, so it launches what the parent launches):
    git worktree add ../parent HEAD~1 && (cd ../parent && python -c "import __graft_entry__ as g; g.build()")
    for i in 1 2 3; do (cd ../parent && python bench.py --gpus 1 --steps 60 --warmup 5); python bench.py --gpus 1 --steps 60 --warmup 5; done
"""
import argparse, json, os, sys, time
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ap = argparse.ArgumentParser()
ap.add_argument("--mode", required=True, choices=["steps", "kernel"])
ap.add_argument("--steps", type=int, default=60)
ap.add_argument("--scale", type=float, default=0.43, help="mesh-size factor of geballe_with_diamond (0.43: 1.04 M DOF)")
a = ap.parse_args()
sys.path.insert(0, ROOT)

import yaml
from heatflow_amd import hip_backend
from heatflow_amd.bc import P1Space, RowDirichletBC
from heatflow_amd.geometry import build_stack, scale_mesh_sizes
from heatflow_amd.heating import HeatingCurve
from heatflow_amd.mesh import Mesh
from heatflow_amd.solver import HeatProblem

with open(os.path.join(ROOT, "cfgs", "geballe_with_diamond.yaml")) as f:
    cfg = scale_mesh_sizes(yaml.safe_load(f), a.scale)
stack = build_stack(cfg)
mesh = Mesh("mesh.msh", stack.bounds, stack.materials).build_mesh()
tags = mesh.material_tags
# the questions of the README's example: the sample and the p-side insulation against a melting line, both couplers, the diamonds
thresholds = {tags["p_sample"]: 2000.0, tags["p_ins"]: 1500.0, tags["p_coupler"]: None, tags["o_coupler"]: None,
              tags["p_diam"]: None, tags["o_diam"]: None}

if a.mode == "kernel":
    rng = np.random.default_rng(1)
    with hip_backend.HeatflowHIP() as be:
        be.set_mesh(mesh.coords, mesh.tris, mesh.tags)
        be.set_state(300.0 + 2000.0 * rng.random(len(mesh.coords)))
        be.set_monitors(thresholds)
        t0 = time.perf_counter()
        for _ in range(200):
            rec = be.monitor_now()
        wall = (time.perf_counter() - t0) / 200
    print(json.dumps({"mode": "kernel", "n": len(mesh.coords), "n_e": len(mesh.tris), "monitored_tags": len(thresholds),
                      "wall_ms_per_monitor_now": 1e3 * wall, "volume_sample_m3": float(2 * np.pi * rec[tags["p_sample"], 4])}))
    sys.exit(0)

tk = {tags[m.name]: m.properties["k"] for m in stack.materials}
trc = {tags[m.name]: m.properties["rho_cv"] for m in stack.materials}
dt = float(cfg["timing"]["t_final"]) / int(cfg["timing"]["num_steps"])
ic = float(cfg["heating"]["ic_temp"])
heat = HeatingCurve(os.path.join(ROOT, "experimental_data", "geballe_heat_data.csv"), ic, float(cfg["heating"]["fwhm"]))
V = P1Space(mesh.coords)
bcs = [RowDirichletBC(V, "left", value=ic), RowDirichletBC(V, "right", value=ic), RowDirichletBC(V, "top", value=ic),
       RowDirichletBC(V, "x", coord=stack.heated_z, length=abs(stack.r_sample) * 2, center=0.0, value=heat.gaussian)]
prob = HeatProblem(mesh.coords, mesh.tris, mesh.tags, tk, trc, dt, bcs, ic, precond=1, amg_reuse=True)
be = prob.backend
per = {"without": [], "with": []}
iters = {}
prob.run(5, time_varying=[prob.bcs[3]])          # warm-up: code objects, the projection basis' buffers
for rnd in range(3):
    for label in ("without", "with"):
        be.set_monitors(thresholds if label == "with" else {})
        prob.set_state(ic)
        _, _, it = prob.run(a.steps, time_varying=[prob.bcs[3]])
        per[label].append(be.last_gpu_ms() / a.steps)
        iters[label] = float(np.mean(it))
        if label == "with":
            assert be.monitor_count() == a.steps
hist = be.get_monitors()
prob.close()
med = {k: float(np.median(v)) for k, v in per.items()}
print(json.dumps({"mode": "steps", "lib": os.path.relpath(hip_backend.LIB_PATH, ROOT), "n": len(mesh.coords), "n_e": len(mesh.tris), "steps": a.steps,
                  "ms_per_step": per, "median_ms_per_step": med, "record_us": 1e3 * (med["with"] - med["without"]),
                  "iters_mean": iters, "sample_T_max_last": float(hist[-1, tags["p_sample"], 0])}))
