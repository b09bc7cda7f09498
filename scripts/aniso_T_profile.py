"""usage (GPU box): python scripts/aniso_T_profile.py [scale]                iterations and ms per step at C3 with multigrid
                 python scripts/aniso_T_profile.py trace REPS [scale]     REPS re-valuations by each of the six table kernels,
                                                                          alternated, to be run under rocprofv3 --kernel-trace --stats
                 python scripts/aniso_T_profile.py kernel STATS.csv       the six kernels' time per launch from that run
                 python scripts/aniso_T_profile.py db RESULTS.db [CSV]    the same from the run's database (rocprofv3's default output)
Tables on anisotropic materials (hf_set_aniso_tables) at C3 (geballe_with_diamond refined to 1.04M DOF at scale
0.43).
  - default: GPU ms per step (HIP events, last_gpu_ms), mean PCG iterations per step and multigrid fallbacks over 100 steps with
    multigrid for the three example configurations - cfgs/geballe_with_diamond_kT.yaml, geballe_with_diamond_aniso.yaml and
    geballe_with_diamond_aniso_kT.yaml - each measured `REPEATS` times in alternation, and how far the watchers of the combined
    example are from the two others.
  - trace: hf_assemble under conductivity tables (k_assemble_rows_kT / _kT_an), under both kinds (k_assemble_rows_cT / _cT_an) and
    hf_steady_picard_setup with Jacobi (k_assemble_rows_kT_K / _kT_K_an) REPS times each at a heated state, isotropic and
    anisotropic alternated in one process; prints the HIP-event time of the calls (kernel + elimination + D^-1).
        rocprofv3 --kernel-trace --stats -d OUT -- python scripts/aniso_T_profile.py trace 20
  - kernel: mean, minimum and maximum duration per launch of the six kernels from the kernel_stats.csv of a `trace` run
    (rocprofv3 --output-format csv).
  - db: the same from the `kernels` view of the run's SQLite database, over the last REPS = 20 launches of each kernel - the
    alternated ones: the warm-up steps of `trace` launch k_assemble_rows_kT_an too - with grid and dynamic LDS bytes; CSV, if
    given, receives one row per kernel.
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
REPEATS = 3
KERNELS = ("k_assemble_rows_kT", "k_assemble_rows_kT_an", "k_assemble_rows_cT", "k_assemble_rows_cT_an", "k_assemble_rows_kT_K",
           "k_assemble_rows_kT_K_an")
EXAMPLES = {"kT": "geballe_with_diamond_kT", "aniso": "geballe_with_diamond_aniso", "aniso_kT": "geballe_with_diamond_aniso_kT"}


def _example_problem(name, scale, mesh, precond=1):
    """The HeatProblem of an example configuration on the mesh of the stock one (the examples share its geometry)."""
    from conftest import load_cfg
    from helpers import material_tables, reference_bcs

    from heatflow_amd.aniso import aniso_tables
    from heatflow_amd.geometry import build_stack, scale_mesh_sizes
    from heatflow_amd.solver import HeatProblem

    cfg = scale_mesh_sizes(load_cfg(name), scale)
    stack = build_stack(cfg)
    tk, trc = material_tables(stack, mesh)
    kt = {mesh.material_tags[m.name]: m.properties["k_table"] for m in stack.materials if "k_table" in m.properties}
    an = {mesh.material_tags[m.name]: m.properties["k_aniso"] for m in stack.materials if "k_aniso" in m.properties}
    bcs, ic, _ = reference_bcs(cfg, stack, mesh)
    dt = float(cfg["timing"]["t_final"]) / int(cfg["timing"]["num_steps"])
    return HeatProblem(mesh.coords, mesh.tris, mesh.tags, tk, trc, dt, bcs, ic, precond=precond,
                       **({"kappa_tables": kt} if kt else {}), **({"k_aniso": an} if an else {}),
                       **({"aniso_tables": True} if aniso_tables(cfg) else {}))


def cost(scale):
    from conftest import build_case
    from kappa_T_profile import _nodes

    case = build_case("geballe_with_diamond", scale)
    mesh = case[2]
    names, nodes = _nodes(case)
    out = {"n": int(len(mesh.coords)), "scale": scale, "steps": 100, "precond": "multigrid", "repeats": REPEATS}

    def run(name, nsteps):
        prob = _example_problem(name, scale, mesh)
        try:
            _, s, it = prob.run(nsteps, watcher_nodes=nodes, time_varying=[prob.bcs[3]])
            info = prob.backend.amg_info()
            return s, np.asarray(it), prob.backend.last_gpu_ms(), info["jacobi_fallbacks"], info["levels"], info["op_complexity"]
        finally:
            prob.close()

    for name in EXAMPLES.values():                                          # warm-up (code objects, pools)
        run(name, 10)
    rows = {k: {"ms_per_step": [], "fallbacks": 0} for k in EXAMPLES}
    samples = {}
    for _ in range(REPEATS):                                                # alternate the three runs
        for label, name in EXAMPLES.items():
            s, it, ms, fb, lev, opc = run(name, 100)
            rows[label]["ms_per_step"].append(ms / 100)
            rows[label].update(pcg_iters_per_step=float(it.mean()), pcg_iters_max=int(it.max()), levels=int(lev),
                               op_complexity=float(opc))
            rows[label]["fallbacks"] += int(fb)
            samples[label] = s
    out["runs"] = rows
    for other in ("kT", "aniso"):
        d = np.abs(samples["aniso_kT"] - samples[other])
        out[f"watcher_diff_aniso_kT_vs_{other}_K"] = {nm: float(d[:, q].max()) for q, nm in enumerate(names)}
    print(json.dumps(out))


def trace(reps, scale):
    from conftest import build_case
    from helpers import make_problem, material_tables

    from heatflow_amd.hip_backend import ASM_ROW_GATHER, PC_JACOBI
    from rhoc_T_oracle import einstein_tables

    case = build_case("geballe_with_diamond", scale)
    cfg, stack, mesh = case
    tk, trc = material_tables(stack, mesh)
    ins = [mesh.material_tags[m.name] for m in stack.materials if m.name.endswith("ins")]
    T = 300.0 + 10.0 * np.arange(51)
    kt = {t: (300.0, 10.0, tk[t] * 300.0 / T) for t in ins}                  # the tables of the tests: 1/T and Einstein on the insulators
    ct = einstein_tables(trc, ins)
    aniso = {t: (4.0, 0.25) for t in ins + [mesh.material_tags["p_sample"]]}
    prob = make_problem(cfg, stack, mesh, precond=0, kappa_tables=kt, k_aniso=aniso, aniso_tables=True)
    ms = {k: [] for k in KERNELS}
    try:
        be = prob.backend
        prob.run(30, time_varying=[prob.bcs[3]])                            # a heated state: the tables are crossed
        u = prob.state()
        dofs = np.asarray(prob.bc_dofs)
        for _ in range(reps):                                               # alternated: every kernel sees the same session
            for cap, kname in ((False, "k_assemble_rows_kT"), (True, "k_assemble_rows_cT")):
                be.set_rhoc_tables(ct if cap else {})
                for label, an in ((kname, {}), (kname + "_an", aniso)):
                    be.set_anisotropy(an)
                    be.set_state(u)
                    be.assemble(prob.dt, ASM_ROW_GATHER)                     # the constant kernel for M, A, then the re-valuation at u
                    ms[label].append(be.last_gpu_ms())
            be.set_rhoc_tables({})
            for label, an in (("k_assemble_rows_kT_K", {}), ("k_assemble_rows_kT_K_an", aniso)):
                be.set_anisotropy(an)
                be.set_state(u)
                be.steady_picard_setup(dofs, PC_JACOBI)
                ms[label].append(be.last_gpu_ms())
    finally:
        prob.close()
    print(json.dumps({"n": int(len(mesh.coords)), "reps": reps,
                      "ms_call_with_elimination": {k: {"first": v[0], "median_rest": float(np.median(v[1:]))} for k, v in ms.items()}}))


def kernel(stats_csv):
    from aniso_profile import _kernel_name

    with open(stats_csv) as f:
        stats = list(csv.DictReader(f))
    out = {}
    for key in KERNELS:
        rows = [r for r in stats if _kernel_name(r["Name"]) == key]
        if rows:
            r = rows[0]
            out[key] = {"calls": int(r["Calls"]), "avg_us": float(r["AverageNs"]) / 1e3, "min_us": float(r["MinNs"]) / 1e3,
                        "max_us": float(r["MaxNs"]) / 1e3}
    print(json.dumps(out))


def db(path, csv_out=None, reps=20):
    import sqlite3

    con = sqlite3.connect(path)
    out = {}
    rows = [("Name", "Calls", "TotalDurationNs", "AverageNs", "MinNs", "MaxNs", "grid_x", "workgroup_x", "lds_size", "scratch_size")]
    for key in KERNELS:
        r = con.execute("select end - start, grid_x, workgroup_x, lds_size, scratch_size, name from kernels where name like ? "
                        "order by start desc limit ?", (f"%::{key}(%", reps)).fetchall()
        if not r:
            continue
        d = [x[0] for x in r]
        out[key] = {"calls": len(d), "avg_us": sum(d) / len(d) / 1e3, "min_us": min(d) / 1e3, "max_us": max(d) / 1e3,
                    "grid": r[0][1] // r[0][2], "lds_bytes": r[0][3], "scratch": r[0][4]}
        rows.append((r[0][5], len(d), sum(d), sum(d) / len(d), min(d), max(d), r[0][1], r[0][2], r[0][3], r[0][4]))
    if csv_out:
        with open(csv_out, "w", newline="") as f:
            csv.writer(f).writerows(rows)
    print(json.dumps(out))


def main():
    if len(sys.argv) > 1 and sys.argv[1] == "db":
        return db(sys.argv[2], sys.argv[3] if len(sys.argv) > 3 else None)
    if len(sys.argv) > 1 and sys.argv[1] == "trace":
        return trace(int(sys.argv[2]), float(sys.argv[3]) if len(sys.argv) > 3 else 0.43)
    if len(sys.argv) > 1 and sys.argv[1] == "kernel":
        return kernel(sys.argv[2])
    cost(float(sys.argv[1]) if len(sys.argv) > 1 else 0.43)


if __name__ == "__main__":
    main()
