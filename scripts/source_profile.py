"""Measurements of the volumetric source for DESIGN.md 3.14 (profiles/source_*), at C3 (1.04 M DOF, multigrid).

    python scripts/source_profile.py --mode source    60 steps driven by hf_set_source at a constant amplitude, three repeats:
                                                      ms per step from HIP events; writes F1 to <out>/F1_c3.npy
    python scripts/source_profile.py --mode load      the same steps driven by hf_set_load(p * F1) with F1 read from that file
    python scripts/source_profile.py --mode kernel    30 hf_set_source calls, for rocprofv3 --kernel-trace --stats
    python scripts/source_profile.py --mode example   cfgs/geballe_with_diamond_source.yaml end to end: how far the watchers rise
Every mode prints one JSON line."""
import argparse, json, math, os, sys, time
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ap = argparse.ArgumentParser()
ap.add_argument("--mode", required=True, choices=["source", "load", "kernel", "example"])
ap.add_argument("--steps", type=int, default=60)
ap.add_argument("--out", default=os.path.join(ROOT, "outputs", "source_profile"))
a = ap.parse_args()
sys.path.insert(0, ROOT)
os.makedirs(a.out, exist_ok=True)

if a.mode == "example":
    import yaml
    from heatflow_amd.driver import run_simulation_impl
    from heatflow_amd.parameter_sweep import get_watcher_points
    with open(os.path.join(ROOT, "cfgs", "geballe_with_diamond_source.yaml")) as f:
        cfg = yaml.safe_load(f)
    wp = get_watcher_points(cfg)
    out = os.path.join(a.out, "example_run")
    res = run_simulation_impl("with_diamond", cfg, os.path.join(a.out, "example_mesh"), rebuild_mesh=True, output_folder=out,
                              watcher_points=wp, write_xdmf=False, suppress_print=True)
    rec = {"mode": "example", "n_dof": int(res["n_dof"]), "loop_time_s": res["loop_time"],
           "iters_mean": float(np.mean(res["iters"])),
           "rise": {k: float(np.max(v) - 300.0) for k, v in res["watchers"].items()},
           "t_peak": {k: float(res["times"][int(np.argmax(v))]) for k, v in res["watchers"].items()}}
    print(json.dumps(rec))
    sys.exit(0)

import yaml
from heatflow_amd import hip_backend
from heatflow_amd.bc import P1Space, RowDirichletBC
from heatflow_amd.geometry import build_stack, scale_mesh_sizes
from heatflow_amd.heating import HeatingCurve
from heatflow_amd.mesh import Mesh
from heatflow_amd.solver import HeatProblem

with open(os.path.join(ROOT, "cfgs", "geballe_with_diamond.yaml")) as f:
    cfg = scale_mesh_sizes(yaml.safe_load(f), 0.43)
stack = build_stack(cfg)
mesh = Mesh("mesh.msh", stack.bounds, stack.materials).build_mesh()
tk = {mesh.material_tags[m.name]: m.properties["k"] for m in stack.materials}
trc = {mesh.material_tags[m.name]: m.properties["rho_cv"] for m in stack.materials}
dt = float(cfg["timing"]["t_final"]) / int(cfg["timing"]["num_steps"])
ic = float(cfg["heating"]["ic_temp"])
heat = HeatingCurve(os.path.join(ROOT, "experimental_data", "geballe_heat_data.csv"), ic, float(cfg["heating"]["fwhm"]))
V = P1Space(mesh.coords)
bcs = [RowDirichletBC(V, "left", value=ic), RowDirichletBC(V, "right", value=ic), RowDirichletBC(V, "top", value=ic),
       RowDirichletBC(V, "x", coord=stack.heated_z, length=abs(stack.r_sample) * 2, center=0.0, value=heat.gaussian)]
tag = mesh.material_tags["p_coupler"]
z0 = float(stack.by_name("p_coupler").boundaries[0])
src = dict(tags=[tag], fwhm=1.32e-5, z0=z0, depth=2.0e-8)
f1_path = os.path.join(a.out, "F1_c3.npy")

if a.mode == "kernel":
    with hip_backend.HeatflowHIP() as be:
        be.set_mesh(mesh.coords, mesh.tris, mesh.tags)
        ms = []
        for _ in range(30):
            be.set_source(src["tags"], src["fwhm"], src["z0"], src["depth"])
            ms.append(be.last_gpu_ms())
        print(json.dumps({"mode": "kernel", "n": len(mesh.coords), "event_ms_first": ms[0], "event_ms_median": float(np.median(ms[5:])),
                          "event_ms_min": float(np.min(ms[5:]))}))
    sys.exit(0)

prob = HeatProblem(mesh.coords, mesh.tris, mesh.tags, tk, trc, dt, bcs, ic, precond=1, amg_reuse=True,
                   **({"source": src} if a.mode == "source" else {}))
be = prob.backend
steps = a.steps
if a.mode == "source":
    F1 = prob.source_vector()
    np.save(f1_path, F1)
    p = 0.2 / (2.0 * math.pi * math.fsum(F1))
    amp = np.full(steps, p)
else:
    F1 = np.load(f1_path)
    p = 0.2 / (2.0 * math.pi * math.fsum(F1))
    prob.set_load(p * F1)
    amp = None
per = []
for rep in range(3):
    prob.set_state(ic)
    _, _, iters = prob.run(steps, time_varying=[prob.bcs[3]], **({"source_amplitude": amp} if amp is not None else {}))
    per.append(be.last_gpu_ms() / steps)
u = prob.state()
print(json.dumps({"mode": a.mode, "lib": hip_backend.LIB_PATH, "n": prob.n, "steps": steps, "ms_per_step": per,
                  "iters_mean": float(np.mean(iters)), "u_max": float(u.max())}))
prob.close()
