"""Measurements of the monitor derivatives for DESIGN.md 3.18 (profiles/monitor_tangent_*), at C3 (1.04 M DOF, multigrid).

    python scripts/monitor_tangent_profile.py --mode steps --nv 2    hf_run_tangent of 30 steps with monitors, the derivative
                                                       records off, on, off, on (one process, alternated, three rounds): ms per
                                                       step from HIP events, and the cost of a derivative record (--nv 2 or 8)
    python scripts/monitor_tangent_profile.py --mode kernel    100 hf_monitor_tangent_eval calls per nv = 2, 4, 8, 16 on the same
                                                       mesh with six monitored tags and one shape slot, for the kernel trace:
        rocprofv3 --kernel-trace --stats --output-format csv -d outputs/monitor_tangent_profile/trace -o montan -- \\
            python scripts/monitor_tangent_profile.py --mode kernel
                                                       (a run of its own; k_monitor_tan<NV> and k_monitor_tan_final in the
                                                       *_kernel_stats.csv, next to k_monitor, which every call launches too)
Every mode prints one JSON line.

The flagship benchmark (it sets no monitors, so it launches what the parent launches), against the spans of
profiles/capacity_tangent_bench_alternated.txt:
    python bench.py --gpus 1 --steps 60 --warmup 5
"""
import argparse, json, os, sys, time
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ap = argparse.ArgumentParser()
ap.add_argument("--mode", required=True, choices=["steps", "kernel"])
ap.add_argument("--steps", type=int, default=30)
ap.add_argument("--nv", type=int, default=2, choices=[2, 8], help="steps: columns of the tangent set-up")
ap.add_argument("--scale", type=float, default=0.43, help="mesh-size factor of geballe_with_diamond (0.43: 1.04 M DOF)")
a = ap.parse_args()
sys.path.insert(0, ROOT)

import yaml
from heatflow_amd import hip_backend
from heatflow_amd.bc import P1Space, RowDirichletBC
from heatflow_amd.geometry import build_stack, scale_mesh_sizes, thickness_velocity
from heatflow_amd.heating import HeatingCurve
from heatflow_amd.mesh import Mesh
from heatflow_amd.solver import HeatProblem

with open(os.path.join(ROOT, "cfgs", "geballe_with_diamond.yaml")) as f:
    cfg = scale_mesh_sizes(yaml.safe_load(f), a.scale)
stack = build_stack(cfg)
mesh = Mesh("mesh.msh", stack.bounds, stack.materials).build_mesh()
tags = mesh.material_tags
# the six tags of scripts/monitor_profile.py
thresholds = {tags["p_sample"]: 2000.0, tags["p_ins"]: 1500.0, tags["p_coupler"]: None, tags["o_coupler"]: None,
              tags["p_diam"]: None, tags["o_diam"]: None}
vel = thickness_velocity(cfg, "p_sample", mesh.coords[:, 0])

if a.mode == "kernel":
    rng = np.random.default_rng(1)
    wall = {}
    with hip_backend.HeatflowHIP() as be:
        be.set_mesh(mesh.coords, mesh.tris, mesh.tags)
        be.set_state(300.0 + 2000.0 * rng.random(len(mesh.coords)))
        be.set_monitors(thresholds)
        for nv in (2, 4, 8, 16):
            s = rng.standard_normal((len(mesh.coords), nv))
            be.monitor_tangent_eval(s, {0: vel})
            t0 = time.perf_counter()
            for _ in range(100):
                row = be.monitor_tangent_eval(s, {0: vel})
            wall[nv] = 1e3 * (time.perf_counter() - t0) / 100
    print(json.dumps({"mode": "kernel", "n": len(mesh.coords), "n_e": len(mesh.tris), "monitored_tags": len(thresholds),
                      "wall_ms_per_eval_with_upload": wall, "dI1_sample_last": float(row[tags["p_sample"], 0, 3])}))
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
be.set_monitors(thresholds)
mats = ["p_sample", "p_ins", "o_ins", "p_coupler", "o_coupler", "p_diam", "o_diam"][:a.nv - 1]
# nv - 1 conductivity columns, then one column that carries the sample's rho_c and its thickness
kw = {"conductivity": [[tags[m]] for m in mats] + [[]], "capacity": [[] for _ in mats] + [[tags["p_sample"]]],
      "shape": {len(mats): vel}, "time_varying": [prob.bcs[3]]}
per = {"off": [], "on": []}
prob.run_tangent(3, None, **kw)                  # warm-up: code objects, the tangent state's buffers
for rnd in range(3):
    for label in ("off", "on"):
        be.set_monitor_tangents(label == "on")
        be.clear_monitor_records()
        prob.set_state(ic)
        prob._tangent_spec = None                # a fresh set-up: the tangents start at zero, as the state does
        prob.run_tangent(a.steps, None, **kw)
        per[label].append(be.last_gpu_ms() / a.steps)
        assert be.monitor_tangent_count()[0] == (a.steps if label == "on" else 0) and be.monitor_count() == a.steps
drec, _ = be.get_monitor_tangents()
prob.close()
med = {k: float(np.median(v)) for k, v in per.items()}
print(json.dumps({"mode": "steps", "lib": os.path.relpath(hip_backend.LIB_PATH, ROOT), "n": len(mesh.coords), "n_e": len(mesh.tris),
                  "steps": a.steps, "nv": be.tangent_nv, "ms_per_step": per, "median_ms_per_step": med,
                  "derivative_record_us": 1e3 * (med["on"] - med["off"]), "dI1_sample_last": float(drec[-1, tags["p_sample"], 0, 3])}))
