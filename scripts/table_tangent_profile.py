"""usage (GPU box): python scripts/table_tangent_profile.py [scale] [steps] [repeats]
Tangent runs under kappa(T) / rho_c(T) tables at C3 (geballe_with_diamond refined to 1.04M DOF at scale 0.43):
GPU ms per step (HIP events on the context's stream, last_gpu_ms) and mean PCG iterations of
  hf_run and hf_run_tangent with 2 columns on the linear problem (the parent's path: k of p_sample and of p_coupler),
  hf_run under 1/T conductivity tables on both insulators (the k(T) primal step of DESIGN.md 3.9),
  hf_run_tangent under those tables with 2 columns (the table scale of both insulators, k of p_sample) and with 8 columns (the same,
  a p_ins exponent, k of both couplers, of the gasket and of both diamonds, fwhm left out), and the 2-column run again with
  Einstein capacity tables on both insulators as well (their table scale in the place of p_sample's k),
multigrid preconditioner, the variants alternated ``repeats`` (default 3) times in one process after a warm-up pass.  Prints one JSON line.
Kernel-level times of k_tangent_load_T<2> and <8>: run the same command (repeats = 1 is enough) under
rocprofv3 --kernel-trace --stats, a run of its own."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    scale = float(sys.argv[1]) if len(sys.argv) > 1 else 0.43
    steps = int(sys.argv[2]) if len(sys.argv) > 2 else 20
    repeats = int(sys.argv[3]) if len(sys.argv) > 3 else 3
    from conftest import build_case
    from helpers import make_problem, material_tables
    from rhoc_T_oracle import einstein_tables

    cfg, stack, mesh = build_case("geballe_with_diamond", scale)
    t = mesh.material_tags
    tk, trc = material_tables(stack, mesh)
    ins = [t["p_ins"], t["o_ins"]]
    T = 300.0 + 10.0 * np.arange(51)
    kt = {tg: (300.0, 10.0, tk[tg] * 300.0 / T) for tg in ins}
    ct = einstein_tables(trc, ins)
    ic = float(cfg["heating"]["ic_temp"])
    scale_k = {"kappa": {tg: kt[tg][2] for tg in ins}}
    wide = [[], [t["p_sample"]], [], [t["p_coupler"]], [t["o_coupler"]], [t["gasket"]], [t["p_diam"]], [t["o_diam"]]]
    variants = {
        "linear": ({}, [
            ("hf_run", None),
            ("hf_run_tangent_2", dict(conductivity=[[t["p_sample"]], [t["p_coupler"]]])),
        ]),
        "kT": (dict(kappa_tables=kt), [
            ("hf_run", None),
            ("hf_run_tangent_2", dict(conductivity=[[], [t["p_sample"]]], tables={0: scale_k})),
            ("hf_run_tangent_8", dict(conductivity=wide, tables={0: scale_k, 2: {"kappa": {ins[0]: kt[ins[0]][2] * np.log(300.0 / T)}}})),
        ]),
        "kT_cT": (dict(kappa_tables=kt, rhoc_tables=ct), [
            ("hf_run", None),
            ("hf_run_tangent_2", dict(tables={0: scale_k, 1: {"rhoc": {tg: ct[tg][2] for tg in ins}}})),
        ]),
    }
    out = {"n": int(len(mesh.coords)), "steps": steps, "scale": scale, "repeats": repeats}
    for name, (kw, runs) in variants.items():
        prob = make_problem(cfg, stack, mesh, precond=1, **kw)
        try:
            res = {label: {"ms_per_step": []} for label, _ in runs}
            for rep in range(repeats + 1):                       # the first pass warms up: code objects, pools, set-ups
                for label, tkw in runs:
                    prob.set_state(ic)
                    if tkw is None:
                        _, _, it = prob.run(steps, [0], time_varying=[prob.bcs[3]])
                        tit = None
                    else:
                        _, _, _, it, tit = prob.run_tangent(steps, [0], time_varying=[prob.bcs[3]], **tkw)
                    if rep == 0:
                        continue
                    r = res[label]
                    r["ms_per_step"].append(prob.backend.last_gpu_ms() / steps)
                    r["iters_mean"] = float(np.mean(it))
                    if tit is not None:
                        r["tangent_iters_mean"] = float(np.mean(tit))
                        r["nv"] = int(prob.backend.tangent_nv)
            out[name] = res
        finally:
            prob.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
