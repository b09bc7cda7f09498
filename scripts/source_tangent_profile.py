"""usage (GPU box): python scripts/source_tangent_profile.py [scale] [steps] [reps]   set-up kernels and ms per tangent step
                 python scripts/source_tangent_profile.py trace REPS [scale] [coupler]   load probes, to be run under
                                                                                   rocprofv3 --kernel-trace --stats
                 python scripts/source_tangent_profile.py kernel STATS.csv         the load kernels' time per launch from that run
Tangent runs under the volumetric source (hf_source_derivatives, hf_tangent_set_source) at C3
(geballe_with_diamond refined to 1.04M DOF at scale 0.43), the heated line kept (it drives the primal of every variant, so the
variants differ by the source alone), the p-side coupler and the insulation behind it absorbing over 0.5 um.
  - default: GPU ms (HIP events, last_gpu_ms) of hf_set_source (k_source_load) and of hf_source_derivatives (k_source_load_d and
    the one-off read-back that builds the row list: the call's wall time is reported next to the kernel's), REPS times each,
    alternated; then GPU ms per step and mean iterations of hf_run_tangent over eight columns, multigrid, alternated REPS times in
    one process: `plain` - the k and rho_c of p_sample and p_ins, no source on the problem at all (the path of before);
    `source_on` - the same columns under a differentiable source with its pulse (no source column: no new launch per step);
    `source_columns` - the same plus source.power, source.fwhm, source.depth and source.pulse.t0 in the other four columns.
  - trace: at the state after five steps of the `source_columns` run, REPS times one hf_tangent_load (k_tangent_load<8>,
    k_tangent_load_cap<8>, kb_source_columns<8>), and REPS times hf_set_source followed by hf_source_derivatives.  With
    `coupler` the p-side coupler alone absorbs, over 20 nm: the intended use, about a fiftieth of the rows.
  - kernel: calls, mean, minimum and maximum duration per launch of those kernels from the kernel_stats.csv of a `trace` run.
Prints one JSON line."""
import csv
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "scripts"))

KERNELS = ("k_source_load", "k_source_load_d", "k_tangent_load<8>", "k_tangent_load_cap<8>", "kb_source_columns<8>")


def _columns(mesh):
    t = mesh.material_tags
    cond = [[t["p_sample"]], [], [t["p_ins"]], []] + [[] for _ in range(4)]
    cap = [[], [t["p_sample"]], [], [t["p_ins"]]] + [[] for _ in range(4)]
    return cond, cap


def _source_kw(prob, P, steps, with_columns):
    import source_tangent_oracle as sto

    times = (np.arange(steps) + 1) * prob.dt
    F1 = prob.source_vector()
    kw = {"source": {}, "source_amplitude": sto.amplitudes(P, times, F1)}
    if with_columns:
        table = sto.coefficient_table(P["power"], P["t0"], P["w"], times, F1, prob.source_derivative("fwhm"),
                                      prob.source_derivative("depth"))
        names = ("source.power", "source.fwhm", "source.depth", "source.pulse.t0")
        kw["source"] = {4 + q: {"amplitude": table[nm][:, 0], "fwhm": table[nm][:, 1], "depth": table[nm][:, 2]}
                        for q, nm in enumerate(names)}
    return kw


def _problems(scale, coupler=False):
    import source_tangent_oracle as sto
    from conftest import build_case

    case = build_case("geballe_with_diamond", scale)
    P = sto.beam(case) if coupler else sto.beam(case, names=("p_coupler", "p_ins"), depth=5.0e-7, power=0.5)
    return case, P, sto.problem(case, P, True, precond=1)


def cost(scale, steps, reps):
    from helpers import material_tables, reference_bcs
    from heatflow_amd.solver import HeatProblem

    case, P, prob = _problems(scale)
    cfg, stack, mesh = case
    out = {"n": int(len(mesh.coords)), "steps": steps, "reps": reps, "scale": scale}
    bcs, ic, _ = reference_bcs(cfg, stack, mesh)
    tk, trc = material_tables(stack, mesh)
    plain = HeatProblem(mesh.coords, mesh.tris, mesh.tags, tk, trc, prob.dt, bcs, ic, precond=1)
    try:
        be = prob.backend
        src = prob.source
        setup = {"k_source_load_ms": [], "k_source_load_d_ms": [], "hf_source_derivatives_wall_ms": []}
        for _ in range(reps + 1):                                          # the first pair is the warm-up
            be.set_source(src["tags"], src["fwhm"], src["z0"], src["depth"])
            setup["k_source_load_ms"].append(be.last_gpu_ms())
            t0 = time.perf_counter()
            be.source_derivatives(True)
            setup["hf_source_derivatives_wall_ms"].append(1e3 * (time.perf_counter() - t0))
            setup["k_source_load_d_ms"].append(be.last_gpu_ms())
        out["setup"] = {k: {"median": float(np.median(v[1:])), "all": [float(x) for x in v[1:]]} for k, v in setup.items()}
        out["absorbing_rows"] = int(np.count_nonzero(be.get_source()))
        cond, cap = _columns(mesh)
        variants = {"plain": (plain, lambda: {}), "source_on": (prob, lambda: _source_kw(prob, P, steps, False)),
                    "source_columns": (prob, lambda: _source_kw(prob, P, steps, True))}
        res = {k: {"ms_per_step": [], "iters_mean": [], "tangent_iters_mean": []} for k in variants}
        for rep in range(reps + 1):                                        # the first round is the warm-up of every variant
            for label, (p, kw) in variants.items():
                p.set_state(ic)
                _, _, _, it, tit = p.run_tangent(steps, [0], conductivity=cond, capacity=cap, time_varying=[p.bcs[3]], **kw())
                if rep:
                    res[label]["ms_per_step"].append(p.backend.last_gpu_ms() / steps)
                    res[label]["iters_mean"].append(float(np.mean(it)))
                    res[label]["tangent_iters_mean"].append(float(np.mean(tit)))
                res[label]["nv"] = int(p.backend.tangent_nv)
        for label, r in res.items():
            r["ms_per_step_median"] = float(np.median(r["ms_per_step"]))
        out["tangent_step"] = res
    finally:
        prob.close()
        plain.close()
    print(json.dumps(out))


def trace(reps, scale, coupler=False):
    case, P, prob = _problems(scale, coupler)
    _, _, mesh = case
    try:
        cond, cap = _columns(mesh)
        prob.run_tangent(5, [0], conductivity=cond, capacity=cap, time_varying=[prob.bcs[3]], **_source_kw(prob, P, 5, True))
        for _ in range(reps):
            prob.tangent_load(4)
        be, src = prob.backend, prob.source
        for _ in range(reps):
            be.set_source(src["tags"], src["fwhm"], src["z0"], src["depth"])
            be.source_derivatives(True)
    finally:
        prob.close()
    print(json.dumps({"n": int(len(mesh.coords)), "reps": reps, "absorbing": list(P["names"])}))


def kernel(stats_csv):
    from aniso_profile import _kernel_name

    with open(stats_csv) as f:
        stats = list(csv.DictReader(f))
    out = {}
    for r in stats:
        name = _kernel_name(r["Name"])
        if name in KERNELS:
            out[name] = {"calls": int(r["Calls"]), "avg_us": float(r["AverageNs"]) / 1e3, "min_us": float(r["MinNs"]) / 1e3,
                         "max_us": float(r["MaxNs"]) / 1e3}
    print(json.dumps(dict(sorted(out.items()))))


def main():
    if len(sys.argv) > 1 and sys.argv[1] == "trace":
        return trace(int(sys.argv[2]), float(sys.argv[3]) if len(sys.argv) > 3 else 0.43, "coupler" in sys.argv[4:])
    if len(sys.argv) > 1 and sys.argv[1] == "kernel":
        return kernel(sys.argv[2])
    cost(float(sys.argv[1]) if len(sys.argv) > 1 else 0.43, int(sys.argv[2]) if len(sys.argv) > 2 else 20,
         int(sys.argv[3]) if len(sys.argv) > 3 else 3)


if __name__ == "__main__":
    main()
