"""usage (GPU box): python scripts/dir_tangent_profile.py [scale] [steps]          ms per step of directional tangent runs
                 python scripts/dir_tangent_profile.py trace VARIANT REPS [scale]  load probes, to be run under
                                                                                  rocprofv3 --kernel-trace --stats
                 python scripts/dir_tangent_profile.py kernel STATS.csv           the load kernels' time per launch from that run
Directional tangents (hf_tangent_setup_dir) at C3 (geballe_with_diamond refined to 1.04M DOF at scale 0.43) with
the example anisotropy of cfgs/geballe_with_diamond_aniso.yaml (insulators r: 2, z: 0.25).
  - default: GPU ms per step (HIP events, last_gpu_ms) and mean PCG iterations of hf_run and of hf_run_tangent with 2, 4 and 8
    directional columns (p_sample.k_r, p_sample.k_z; + p_ins.k_r, p_ins.k_z; + o_ins.k_r, o_ins.k_z, g_ins.k, p_coupler.k), and
    with 2 plain columns on isotropic tags through hf_tangent_setup for comparison, multigrid.
  - trace: at the state after five steps, REPS times in alternation and per NV = 2, 4, 8: one hf_tangent_load under a plain set-up
    (k_tangent_load<NV>: kappa columns on the isotropic tags p_sample, p_coupler, o_coupler, p_diam, o_diam, gasket - the first
    2, 4, 6) and one under a directional set-up (k_tangent_load_dir<NV>).  VARIANT picks the directional columns:
      kz     k_z columns of the same tags: the same element visits as the plain set-up, each through the directional branch
      kappa  kappa columns of the same tags: the same visits through the isotropic branch (the bits of k_tangent_load)
      use    the columns of the default mode: k_r and k_z of one tag in two columns, kappa of an anisotropic tag
  - kernel: calls, mean, minimum and maximum duration per launch of every k_tangent_load / k_tangent_load_dir instantiation from the
    kernel_stats.csv of a `trace` run.
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

ISO_TAGS = ("p_sample", "p_coupler", "o_coupler", "p_diam", "o_diam", "gasket")
USE = ("p_sample.k_r", "p_sample.k_z", "p_ins.k_r", "p_ins.k_z", "o_ins.k_r", "o_ins.k_z", "g_ins.k", "p_coupler.k")


def _example(mesh):
    return {mesh.material_tags[n]: (2.0, 0.25) for n in ("p_ins", "o_ins", "g_ins")}


def _use_columns(mesh, n_par):
    kind = {"k": "k", "k_r": "r", "k_z": "z"}
    return [[(mesh.material_tags[nm.rsplit(".", 1)[0]], kind[nm.rsplit(".", 1)[1]])] for nm in USE[:n_par]]


def cost(scale, steps):
    from conftest import build_case
    from helpers import make_problem

    cfg, stack, mesh = build_case("geballe_with_diamond", scale)
    out = {"n": int(len(mesh.coords)), "steps": steps, "scale": scale, "k_aniso": "insulators r 2, z 0.25"}
    prob = make_problem(cfg, stack, mesh, precond=1, k_aniso=_example(mesh))
    try:
        ic = float(cfg["heating"]["ic_temp"])
        prob.run(steps, [0], time_varying=[prob.bcs[3]])                       # warm-up: code objects, pools
        prob.set_state(ic)
        _, _, it = prob.run(steps, [0], time_varying=[prob.bcs[3]])
        out["hf_run"] = {"ms_per_step": prob.backend.last_gpu_ms() / steps, "iters_mean": float(np.mean(it))}
        runs = [("plain_2", [[mesh.material_tags[t]] for t in ISO_TAGS[:2]])] + [(f"directional_{n}", _use_columns(mesh, n)) for n in (2, 4, 8)]
        for label, cond in runs:
            prob.set_state(ic)
            prob.run_tangent(2, [0], conductivity=cond, time_varying=[prob.bcs[3]])   # set-up and warm-up of this width
            prob.set_state(ic)
            _, _, _, it, tit = prob.run_tangent(steps, [0], conductivity=cond, time_varying=[prob.bcs[3]])
            out[label] = {"nv": int(prob.backend.tangent_nv), "ms_per_step": prob.backend.last_gpu_ms() / steps,
                          "iters_mean": float(np.mean(it)), "tangent_iters_mean": float(np.mean(tit)),
                          "tangent_iters_per_column": [float(v) for v in np.mean(tit, axis=0)]}
    finally:
        prob.close()
    print(json.dumps(out))


def trace(variant, reps, scale):
    from conftest import build_case
    from helpers import make_problem

    cfg, stack, mesh = build_case("geballe_with_diamond", scale)
    t = mesh.material_tags
    prob = make_problem(cfg, stack, mesh, precond=1, k_aniso=_example(mesh))
    try:
        be = prob.backend
        prob.run(5, [0], time_varying=[prob.bcs[3]])
        worst = 0.0
        for n_par in (2, 4, 6):
            tags = [t[m] for m in ISO_TAGS[:n_par]]
            cols = {tag: j for j, tag in enumerate(tags)}
            for _ in range(reps):                                              # alternated: both kernels see the same session
                be.tangent_setup(n_par, cols)
                plain = be.tangent_load(0)
                if variant == "kz":
                    be.tangent_setup_dir(n_par, z=cols)
                elif variant == "kappa":
                    be.tangent_setup_dir(n_par, k=cols)
                else:
                    kinds = {"k": {}, "r": {}, "z": {}}
                    for j, ((tag, kind),) in enumerate(_use_columns(mesh, 8 if n_par == 6 else n_par)):
                        kinds[kind][tag] = j
                    be.tangent_setup_dir(8 if n_par == 6 else n_par, kinds["k"], kinds["r"], kinds["z"])
                got = be.tangent_load(0)
                if variant == "kappa":
                    worst = max(worst, float(np.max(np.abs(got - plain))))
    finally:
        prob.close()
    print(json.dumps({"n": int(len(mesh.coords)), "variant": variant, "reps": reps,
                      **({"max_abs_difference_to_plain": worst} if variant == "kappa" else {})}))


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
        return trace(sys.argv[2], int(sys.argv[3]), float(sys.argv[4]) if len(sys.argv) > 4 else 0.43)
    if len(sys.argv) > 1 and sys.argv[1] == "kernel":
        return kernel(sys.argv[2])
    cost(float(sys.argv[1]) if len(sys.argv) > 1 else 0.43, int(sys.argv[2]) if len(sys.argv) > 2 else 20)


if __name__ == "__main__":
    main()
