"""usage (GPU box): python scripts/kappa_T_profile.py [scale]        cost of kappa(T) at C3 for both preconditioners
                 python scripts/kappa_T_profile.py trace STEPS [scale]   STEPS kappa(T) steps (p = 1, multigrid) under rocprofv3
                 python scripts/kappa_T_profile.py kernel STATS.csv [scale]   the re-valuation kernel's time, bytes, HBM fraction
Temperature-dependent conductivities (hf_set_kappa_tables) at C3 (geballe_with_diamond refined to 1.04M DOF at scale 0.43),
the tables of cfgs/geballe_with_diamond_kT.yaml:
  - GPU ms per step (HIP events, last_gpu_ms) and mean PCG iterations per step over 100 steps, for constant kappa (hf_run),
    kappa(T) with p = 1 and with p = 3 Picard sweeps, with Jacobi and with multigrid;
  - the o-side and p-side watcher difference between the kappa(T) configuration and the constant one at 100 steps.
Prints one JSON line.  `kernel` reads the kernel_stats.csv of a `trace` run and reports k_assemble_rows_kT's mean duration,
its algorithmic bytes (A written, column positions, triangle lists, coordinates, column ids and u* of every block's column
list read once; the halo of the column lists is not counted) and the fraction of the HBM peak (8 TB/s) that makes."""
import csv
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
HBM_PEAK = 8.0e12


def _case(scale):
    from conftest import build_case

    return build_case("geballe_with_diamond_kT", scale)


def _tables(case):
    _, stack, mesh = case
    return {mesh.material_tags[m.name]: m.properties["k_table"] for m in stack.materials if "k_table" in m.properties}


def _nodes(case):
    from heatflow_amd.driver import _parse_watchers
    from heatflow_amd.parameter_sweep import get_watcher_points
    from heatflow_amd.solver import nearest_nodes

    names, pts = _parse_watchers(get_watcher_points(case[0]))
    return names, nearest_nodes(case[2].coords, pts)


def _run(case, precond, tables, picard, nsteps, nodes):
    from helpers import make_problem

    cfg, stack, mesh = case
    prob = make_problem(cfg, stack, mesh, precond=precond, kappa_tables=tables, picard=picard)
    try:
        _, s, it = prob.run(nsteps, watcher_nodes=nodes, time_varying=[prob.bcs[3]])
        return s, np.asarray(it), prob.backend.last_gpu_ms(), prob.backend.amg_info()["jacobi_fallbacks"] if precond else 0
    finally:
        prob.close()


def cost(scale):
    case = _case(scale)
    names, nodes = _nodes(case)
    tables = _tables(case)
    out = {"n": int(len(case[2].coords)), "scale": scale, "steps": 100}
    for precond, pname in ((0, "jacobi"), (1, "multigrid")):
        _run(case, precond, None, 1, 10, nodes)                          # warm-up (code objects, pools)
        row = {}
        for label, tab, p in (("constant", None, 1), ("kT_p1", tables, 1), ("kT_p3", tables, 3)):
            s, it, ms, fb = _run(case, precond, tab, p, 100, nodes)
            row[label] = {"ms_per_step": ms / 100, "pcg_iters_per_step": float(it.mean()), "fallbacks": int(fb)}
            row[label]["_samples"] = s
        d = np.abs(row["kT_p1"].pop("_samples") - row["constant"]["_samples"])
        row["kT_p3"].pop("_samples")
        row["constant"].pop("_samples")
        out[pname] = row
        out[f"{pname}_watcher_diff_kT_vs_constant_K"] = {nm: float(d[:, q].max()) for q, nm in enumerate(names)}
    print(json.dumps(out))


def trace(nsteps, scale):
    case = _case(scale)
    _, nodes = _nodes(case)
    _, it, ms, _ = _run(case, 1, _tables(case), 1, nsteps, nodes)
    print(json.dumps({"steps": nsteps, "pcg_iters": int(it.sum()), "ms": ms}))


def kernel(stats_csv, scale):
    case = _case(scale)
    _, _, mesh = case
    n, ne = len(mesh.coords), len(mesh.tris)
    with open(stats_csv) as f:
        rows = [r for r in csv.DictReader(f) if "k_assemble_rows_kT" in r["Name"]]
    from heatflow_amd.hip_backend import HeatflowHIP

    b = HeatflowHIP(0)
    try:
        b.set_mesh(mesh.coords, mesh.tris, mesh.tags)
        nnz = b.nnz
    finally:
        b.close()
    nbytes = nnz * (8 + 2) + 3 * ne * 2 + n * (16 + 4 + 8 + 4)
    out = {"n": n, "nnz": int(nnz), "algorithmic_bytes": int(nbytes)}
    if rows:
        r = rows[0]
        avg_ns = float(r["AverageNs"])
        out.update({"calls": int(r["Calls"]), "avg_us": avg_ns / 1e3, "hbm_fraction": nbytes / (avg_ns * 1e-9) / HBM_PEAK})
    print(json.dumps(out))


def main():
    if len(sys.argv) > 1 and sys.argv[1] == "trace":
        return trace(int(sys.argv[2]), float(sys.argv[3]) if len(sys.argv) > 3 else 0.43)
    if len(sys.argv) > 1 and sys.argv[1] == "kernel":
        return kernel(sys.argv[2], float(sys.argv[3]) if len(sys.argv) > 3 else 0.43)
    cost(float(sys.argv[1]) if len(sys.argv) > 1 else 0.43)


if __name__ == "__main__":
    main()
