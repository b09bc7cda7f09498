"""usage (GPU box): python scripts/rhoc_T_profile.py [scale]            cost of cv(T) at C3 with multigrid
                 python scripts/rhoc_T_profile.py trace KIND STEPS [scale]   STEPS steps (p = 1, multigrid) under rocprofv3;
                                                                  KIND = kT (conductivity tables only), cT (capacity tables
                                                                  only) or both
                 python scripts/rhoc_T_profile.py kernel STATS.csv [scale]   the re-valuation kernels' time, bytes, HBM fraction
Temperature-dependent heat capacities (hf_set_rhoc_tables) at C3 (geballe_with_diamond refined to 1.04M DOF at scale 0.43).
Conductivity tables: those of cfgs/geballe_with_diamond_kT.yaml (as scripts/kappa_T_profile.py); capacity tables: those of
cfgs/geballe_with_diamond_cvT.yaml (Einstein, theta = 600 K, on the pressure media).
  - GPU ms per step (HIP events, last_gpu_ms) and mean PCG iterations per step over 100 steps with multigrid, p = 1, for
    constant coefficients, conductivity tables only, capacity tables only and both, each measured `REPEATS` times in
    alternation (the spread of the repeats is the run-to-run spread); capacity tables also with p = 3;
  - the watcher differences of the cv(T) runs against the constant one.
Prints one JSON line.  `kernel` reads the kernel_stats.csv of a `trace` run and reports, for k_assemble_rows_cT,
k_assemble_rows_kT and k_assemble_rows<false> (whichever ran), the mean duration, the algorithmic bytes (the value arrays
written, column positions, triangle lists, coordinates, column ids and u* of every block's column list read once; the halo of
the column lists is not counted) and the fraction of the HBM peak (8 TB/s) that makes."""
import csv
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "scripts"))
HBM_PEAK = 8.0e12
REPEATS = 3


def _setup(scale):
    from conftest import build_case, load_cfg
    from kappa_T_profile import _nodes

    from heatflow_amd.geometry import build_stack, scale_mesh_sizes

    case = build_case("geballe_with_diamond", scale)
    _, _, mesh = case
    tabs = {}
    for kind, name, prop in (("k", "geballe_with_diamond_kT", "k_table"), ("c", "geballe_with_diamond_cvT", "rho_cv_table")):
        stack = build_stack(scale_mesh_sizes(load_cfg(name), scale))
        tabs[kind] = {mesh.material_tags[m.name]: m.properties[prop] for m in stack.materials if prop in m.properties}
    names, nodes = _nodes(case)
    return case, tabs, names, nodes


def _run(case, ktab, ctab, picard, nsteps, nodes):
    from helpers import make_problem

    cfg, stack, mesh = case
    kw = {}
    if ktab:
        kw["kappa_tables"] = ktab
    if ctab:
        kw["rhoc_tables"] = ctab
    prob = make_problem(cfg, stack, mesh, precond=1, picard=picard, **kw)
    try:
        _, s, it = prob.run(nsteps, watcher_nodes=nodes, time_varying=[prob.bcs[3]])
        return s, np.asarray(it), prob.backend.last_gpu_ms(), prob.backend.amg_info()["jacobi_fallbacks"]
    finally:
        prob.close()


KINDS = {"constant": (False, False), "kT": (True, False), "cT": (False, True), "both": (True, True)}


def cost(scale):
    case, tabs, names, nodes = _setup(scale)
    out = {"n": int(len(case[2].coords)), "scale": scale, "steps": 100, "precond": "multigrid", "repeats": REPEATS}
    _run(case, None, None, 1, 10, nodes)                                  # warm-up (code objects, pools)
    _run(case, tabs["k"], tabs["c"], 1, 10, nodes)
    rows = {k: {"ms_per_step": [], "pcg_iters_per_step": None, "fallbacks": 0} for k in KINDS}
    samples = {}
    for _ in range(REPEATS):                                              # alternate the four runs
        for label, (k, c) in KINDS.items():
            s, it, ms, fb = _run(case, tabs["k"] if k else None, tabs["c"] if c else None, 1, 100, nodes)
            rows[label]["ms_per_step"].append(ms / 100)
            rows[label]["pcg_iters_per_step"] = float(it.mean())
            rows[label]["fallbacks"] += int(fb)
            samples[label] = s
    s, it, ms, fb = _run(case, None, tabs["c"], 3, 100, nodes)
    rows["cT_p3"] = {"ms_per_step": [ms / 100], "pcg_iters_per_step": float(it.mean()), "fallbacks": int(fb)}
    samples["cT_p3"] = s
    out["runs"] = rows
    for label in ("cT", "cT_p3", "both"):
        d = np.abs(samples[label] - samples["constant"])
        out[f"watcher_diff_{label}_vs_constant_K"] = {nm: float(d[:, q].max()) for q, nm in enumerate(names)}
    print(json.dumps(out))


def trace(kind, nsteps, scale):
    case, tabs, _, nodes = _setup(scale)
    k, c = KINDS[kind]
    _, it, ms, _ = _run(case, tabs["k"] if k else None, tabs["c"] if c else None, 1, nsteps, nodes)
    print(json.dumps({"kind": kind, "steps": nsteps, "pcg_iters": int(it.sum()), "ms": ms}))


def kernel(stats_csv, scale):
    case, _, _, _ = _setup(scale)
    _, _, mesh = case
    n, ne = len(mesh.coords), len(mesh.tris)
    with open(stats_csv) as f:
        stats = list(csv.DictReader(f))
    from heatflow_amd.hip_backend import HeatflowHIP

    b = HeatflowHIP(0)
    try:
        b.set_mesh(mesh.coords, mesh.tris, mesh.tags)
        nnz = b.nnz
    finally:
        b.close()
    lists = nnz * 2 + 3 * ne * 2 + n * (16 + 4)            # column positions, triangle lists, coordinates and column ids
    out = {"n": n, "nnz": int(nnz)}
    for key, pat, nbytes in (("k_assemble_rows_cT", "k_assemble_rows_cT", lists + nnz * 16 + n * (8 + 4)),
                             ("k_assemble_rows_kT", "k_assemble_rows_kT", lists + nnz * 8 + n * (8 + 4)),
                             ("k_assemble_rows<false>", "k_assemble_rows<false>", lists + nnz * 16)):
        rows = [r for r in stats if pat in r["Name"].replace("(anonymous namespace)::", "")]
        row = {"algorithmic_bytes": int(nbytes)}
        if rows:
            avg_ns = float(rows[0]["AverageNs"])
            row.update({"calls": int(rows[0]["Calls"]), "avg_us": avg_ns / 1e3,
                        "hbm_fraction": nbytes / (avg_ns * 1e-9) / HBM_PEAK})
        out[key] = row
    out["launches"] = {r["Name"].replace("(anonymous namespace)::", "").split("(")[0]: int(r["Calls"]) for r in stats}
    print(json.dumps(out))


def main():
    if len(sys.argv) > 1 and sys.argv[1] == "trace":
        return trace(sys.argv[2], int(sys.argv[3]), float(sys.argv[4]) if len(sys.argv) > 4 else 0.43)
    if len(sys.argv) > 1 and sys.argv[1] == "kernel":
        return kernel(sys.argv[2], float(sys.argv[3]) if len(sys.argv) > 3 else 0.43)
    cost(float(sys.argv[1]) if len(sys.argv) > 1 else 0.43)


if __name__ == "__main__":
    main()
