"""usage (GPU box): python scripts/time_scheme_profile.py [scale]            accuracy and cost of both time schemes
                 python scripts/time_scheme_profile.py trace SCHEME STEPS [scale]   STEPS steps of one scheme (under rocprofv3)
                 python scripts/time_scheme_profile.py launches BE_STATS.csv BDF2_STATS.csv STEPS   launches per step
Backward Euler against BDF2 (hf_set_time_scheme) at C3 (geballe_with_diamond refined to 1.04M DOF at scale 0.43), multigrid
preconditioner, default start vector:
  - GPU ms per step (HIP events on the context's stream, last_gpu_ms) and mean PCG iterations per step, 100 steps each;
  - max error of the o-side and p-side watchers against a 1600-step BDF2 run, for backward Euler with 100 / 200 / 400 steps
    and BDF2 with 25 / 50 / 100 steps.
Prints one JSON line.  `trace` runs a set-up and STEPS steps of one scheme, for rocprofv3 --kernel-trace --stats; `launches`
reads the two kernel_stats.csv files of such runs and prints the launches of each scheme with the per-kernel differences."""
import csv
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def _problem(case, scheme, nsteps):
    from helpers import make_problem

    cfg, stack, mesh = case
    c = dict(cfg, timing=dict(cfg["timing"], num_steps=int(nsteps)))
    return make_problem(c, stack, mesh, precond=1, scheme=scheme)


def _watchers(case):
    from heatflow_amd.driver import _parse_watchers
    from heatflow_amd.parameter_sweep import get_watcher_points
    from heatflow_amd.solver import nearest_nodes

    names, pts = _parse_watchers(get_watcher_points(case[0]))
    return names, nearest_nodes(case[2].coords, pts)


def _run(case, scheme, nsteps, nodes):
    prob = _problem(case, scheme, nsteps)
    try:
        _, s, it = prob.run(nsteps, watcher_nodes=nodes, time_varying=[prob.bcs[3]])
        return s, np.asarray(it), prob.backend.last_gpu_ms()
    finally:
        prob.close()


def accuracy(scale):
    from conftest import build_case

    case = build_case("geballe_with_diamond", scale)
    names, nodes = _watchers(case)
    out = {"n": int(len(case[2].coords)), "scale": scale}
    for scheme in ("backward_euler", "bdf2"):
        _run(case, scheme, 20, nodes)                                    # warm-up (code objects, pools)
        _, it, ms = _run(case, scheme, 100, nodes)
        out[scheme] = {"ms_per_step": ms / 100, "pcg_iters_per_step": float(it.mean())}
    out["bdf2_over_be_ms"] = out["bdf2"]["ms_per_step"] / out["backward_euler"]["ms_per_step"]
    ref, _, _ = _run(case, "bdf2", 1600, nodes)
    err = {}
    for scheme, ns in (("backward_euler", (100, 200, 400)), ("bdf2", (25, 50, 100))):
        for n in ns:
            s, _, _ = _run(case, scheme, n, nodes)
            d = np.abs(s - ref[1600 // n - 1::1600 // n]).max(axis=0)
            err[f"{scheme}_{n}"] = {nm: float(d[q]) for q, nm in enumerate(names)}
    out["max_error_vs_bdf2_1600_K"] = err
    out["oside_rise_K"] = float(ref[:, names.index("oside")].max() - ref[0, names.index("oside")])
    print(json.dumps(out))


def trace(scheme, nsteps, scale):
    from conftest import build_case

    case = build_case("geballe_with_diamond", scale)
    _, nodes = _watchers(case)
    s, it, ms = _run(case, scheme, nsteps, nodes)
    print(json.dumps({"scheme": scheme, "steps": nsteps, "pcg_iters": int(it.sum()), "ms": ms}))


def launches(be_csv, bdf2_csv, nsteps):
    def read(path):
        with open(path) as f:
            return {r["Name"]: int(r["Calls"]) for r in csv.DictReader(f)}

    a, b = read(be_csv), read(bdf2_csv)
    diff = {k: [a.get(k, 0), b.get(k, 0)] for k in sorted(set(a) | set(b)) if a.get(k, 0) != b.get(k, 0)}
    print(json.dumps({"steps": nsteps, "launches_backward_euler": sum(a.values()), "launches_bdf2": sum(b.values()),
                      "per_kernel_differences_[be,bdf2]": diff}))


def main():
    if len(sys.argv) > 1 and sys.argv[1] == "trace":
        return trace(sys.argv[2], int(sys.argv[3]), float(sys.argv[4]) if len(sys.argv) > 4 else 0.43)
    if len(sys.argv) > 1 and sys.argv[1] == "launches":
        return launches(sys.argv[2], sys.argv[3], int(sys.argv[4]))
    accuracy(float(sys.argv[1]) if len(sys.argv) > 1 else 0.43)


if __name__ == "__main__":
    main()
