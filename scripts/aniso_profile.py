"""usage (GPU box): python scripts/aniso_profile.py [scale]                 iterations and ms per step at C3 with multigrid
                 python scripts/aniso_profile.py trace REPS [scale]      REPS assemblies and steady set-ups, isotropic and
                                                                         anisotropic, to be run under rocprofv3 --kernel-trace --stats
                 python scripts/aniso_profile.py kernel STATS.csv        the four assembly kernels' time per launch from that run
                 python scripts/aniso_profile.py observable [OUTDIR]     the o-side watcher and the kappa_sample a sweep picks, stock mesh
Anisotropic conductivities (hf_set_anisotropy) at C3 (geballe_with_diamond refined to 1.04M DOF at scale 0.43).
  - default: GPU ms per step (HIP events, last_gpu_ms), mean PCG iterations per step and multigrid fallbacks over 100 steps with
    multigrid, for the isotropic configuration, the example of cfgs/geballe_with_diamond_aniso.yaml (insulators r: 2, z: 0.25) and
    two stronger cases on the insulators and the sample, m_z / m_r = 1/16 and 16, each measured `REPEATS` times in alternation
    (the spread of the repeats is the run-to-run spread); and how far the watchers move against the isotropic run.
  - trace: hf_assemble (k_assemble_rows<false> / k_assemble_rows_an<false>) and hf_steady_setup with Jacobi (k_assemble_rows<true>
    / k_assemble_rows_an<true>) REPS times each, alternated, in one process; HEATFLOW_ANISO_INFO=1 prints the LDS footprint, the
    workgroups per CU the occupancy query returns and the grid.
  - kernel: mean, minimum and maximum duration per launch of the four kernels from the kernel_stats.csv of a `trace` run.
  - observable: the stock with-diamond configuration (scale 1) at 100 steps: the largest movement of the o-side watcher under the
    example anisotropy, and the kappa_sample the 64-point sweep of run_kappa_sweep picks (smallest rmse against the experiment)
    with and without it.
Prints one JSON line."""
import contextlib
import copy
import csv
import json
import os
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "scripts"))
REPEATS = 3


def _multipliers(mesh, names, m_r, m_z):
    return {mesh.material_tags[n]: (m_r, m_z) for n in names if n in mesh.material_tags}


def _cases(mesh):
    ins = ("p_ins", "o_ins", "g_ins")
    return {"isotropic": None,
            "example": _multipliers(mesh, ins, 2.0, 0.25),
            "mz_over_mr_1_16": _multipliers(mesh, ins + ("p_sample",), 4.0, 0.25),
            "mz_over_mr_16": _multipliers(mesh, ins + ("p_sample",), 0.25, 4.0)}


def _run(case, aniso, nsteps, nodes):
    from helpers import make_problem

    cfg, stack, mesh = case
    prob = make_problem(cfg, stack, mesh, precond=1, **({"k_aniso": aniso} if aniso else {}))
    try:
        _, s, it = prob.run(nsteps, watcher_nodes=nodes, time_varying=[prob.bcs[3]])
        info = prob.backend.amg_info()
        return s, np.asarray(it), prob.backend.last_gpu_ms(), info["jacobi_fallbacks"], info["levels"], info["op_complexity"]
    finally:
        prob.close()


def cost(scale):
    from conftest import build_case
    from kappa_T_profile import _nodes

    case = build_case("geballe_with_diamond", scale)
    names, nodes = _nodes(case)
    cases = _cases(case[2])
    out = {"n": int(len(case[2].coords)), "scale": scale, "steps": 100, "precond": "multigrid", "repeats": REPEATS}
    _run(case, None, 10, nodes)                                           # warm-up (code objects, pools)
    _run(case, cases["example"], 10, nodes)
    rows = {k: {"ms_per_step": [], "fallbacks": 0} for k in cases}
    samples = {}
    for _ in range(REPEATS):                                              # alternate the four runs
        for label, an in cases.items():
            s, it, ms, fb, lev, opc = _run(case, an, 100, nodes)
            rows[label]["ms_per_step"].append(ms / 100)
            rows[label].update(pcg_iters_per_step=float(it.mean()), pcg_iters_max=int(it.max()), levels=int(lev),
                               op_complexity=float(opc))
            rows[label]["fallbacks"] += int(fb)
            samples[label] = s
    out["runs"] = rows
    for label in cases:
        if label != "isotropic":
            d = np.abs(samples[label] - samples["isotropic"])
            out[f"watcher_diff_{label}_vs_isotropic_K"] = {nm: float(d[:, q].max()) for q, nm in enumerate(names)}
    print(json.dumps(out))


def trace(reps, scale):
    from conftest import build_case
    from helpers import material_tables, reference_bcs

    from heatflow_amd.bc import merge_bcs
    from heatflow_amd.hip_backend import ASM_ROW_GATHER, PC_JACOBI, HeatflowHIP

    cfg, stack, mesh = build_case("geballe_with_diamond", scale)
    tk, trc = material_tables(stack, mesh)
    tags = sorted(tk)
    dt = float(cfg["timing"]["t_final"]) / int(cfg["timing"]["num_steps"])
    bcs, _, _ = reference_bcs(cfg, stack, mesh)
    dofs = merge_bcs(bcs)[0]
    aniso = _cases(mesh)["mz_over_mr_1_16"]
    ms = {"isotropic": [], "anisotropic": [], "isotropic_steady": [], "anisotropic_steady": []}
    with HeatflowHIP(0) as be:
        be.set_mesh(mesh.coords, mesh.tris, mesh.tags)
        be.set_materials(tags, [tk[t] for t in tags], [trc[t] for t in tags])
        be.set_dirichlet(dofs)
        be.set_precond(PC_JACOBI)
        for _ in range(reps):                                             # alternated: both kernels see the same session
            for label, an in (("isotropic", {}), ("anisotropic", aniso)):
                be.set_anisotropy(an)
                be.assemble(dt, ASM_ROW_GATHER)
                ms[label].append(be.last_gpu_ms())                        # (assembly + elimination + D^-1, HIP events)
                be.steady_setup(dofs, PC_JACOBI)
                ms[label + "_steady"].append(be.last_gpu_ms())
    print(json.dumps({"n": int(len(mesh.coords)), "reps": reps,
                      "ms_assemble_with_elimination": {k: {"first": v[0], "median_rest": float(np.median(v[1:]))} for k, v in ms.items()}}))


def _kernel_name(name):
    """'k_assemble_rows_an<false>' of 'void (anonymous namespace)::k_assemble_rows_an<false>(int, ...)' (or '<(bool)0>')."""
    name = name.replace("(anonymous namespace)::", "").replace("void ", "").strip()
    name = name.replace("<(bool)0>", "<false>").replace("<(bool)1>", "<true>")
    depth = 0
    for i, ch in enumerate(name):                                         # cut at the argument list, not inside the template list
        depth += ch == "<"
        depth -= ch == ">"
        if ch == "(" and depth == 0:
            return name[:i]
    return name


def kernel(stats_csv):
    with open(stats_csv) as f:
        stats = list(csv.DictReader(f))
    out = {}
    for key in ("k_assemble_rows<false>", "k_assemble_rows<true>", "k_assemble_rows_an<false>", "k_assemble_rows_an<true>"):
        rows = [r for r in stats if _kernel_name(r["Name"]) == key]
        if rows:
            r = rows[0]
            out[key] = {"calls": int(r["Calls"]), "avg_us": float(r["AverageNs"]) / 1e3, "min_us": float(r["MinNs"]) / 1e3,
                        "max_us": float(r["MaxNs"]) / 1e3}
    print(json.dumps(out))


def observable(outdir):
    from conftest import HEATING_CSV, load_cfg

    from heatflow_amd import parameter_sweep as ps

    ks = ps.get_k_values(count=64)
    out = {"k_grid_step": float(ks[1] - ks[0]), "steps": 100}
    curves = {}
    for label, name in (("isotropic", "geballe_with_diamond"), ("example", "geballe_with_diamond_aniso")):
        cfg = load_cfg(name)
        cfg["heating"]["file"] = HEATING_CSV
        folder = os.path.join(outdir, label)
        with contextlib.redirect_stdout(sys.stderr):                       # (the sweep reports its progress)
            rows = ps.run_kappa_sweep(copy.deepcopy(cfg), os.path.join(outdir, "mesh"), ks, folder, rebuild_mesh=(label == "isotropic"),
                                      concurrent=2, batch=16, exp_csv=HEATING_CSV)
        ok = [r for r in rows if r["status"] == "success"]
        best = min(ok, key=lambda r: r["rmse"])
        out[label] = {"points": len(ok), "kappa_sample": best["k"], "rmse": best["rmse"],
                      "pcg_iters_mean": float(np.mean([r["pcg_iters_mean"] for r in ok]))}
        k0 = min(ks, key=lambda k: abs(k - float(cfg["mats"]["p_sample"]["k"])))
        digits = 2 if len({f"{k:.2f}" for k in ks}) == len(ks) else 4
        curves[label] = np.genfromtxt(os.path.join(folder, f"{k0:.{digits}f}", "watcher_points.csv"), delimiter=",", names=True)
        out[label]["k_of_curve"] = float(k0)
    for w in ("pside", "oside"):
        out[f"{w}_watcher_moves_K"] = float(np.abs(curves["example"][w] - curves["isotropic"][w]).max())
    print(json.dumps(out))


def main():
    if len(sys.argv) > 1 and sys.argv[1] == "trace":
        return trace(int(sys.argv[2]), float(sys.argv[3]) if len(sys.argv) > 3 else 0.43)
    if len(sys.argv) > 1 and sys.argv[1] == "kernel":
        return kernel(sys.argv[2])
    if len(sys.argv) > 1 and sys.argv[1] == "observable":
        if len(sys.argv) > 2:
            return observable(sys.argv[2])
        with tempfile.TemporaryDirectory() as tmp:
            return observable(tmp)
    cost(float(sys.argv[1]) if len(sys.argv) > 1 else 0.43)


if __name__ == "__main__":
    main()
