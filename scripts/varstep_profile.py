#!/usr/bin/env python
"""Measurements of variable time steps on an MI355X, at 1.04 M DOF unless --scale says otherwise:

  (a) revalue    the cost of one re-valuation: steps that alternate between two sizes against steps of one size
  (b) stale      the per-iteration cost with A's value lists stale: a fixed-step run before and after one re-valuation
  (c) ratio      PCG iterations per step as a function of dt'/dt'_h under the frozen hierarchy, two decades either side
  (d) adaptive   an adaptive run under the smooth pulse against the fixed-step run of the same accuracy, in wall time
  (e) bench      `python bench.py --gpus 1 --steps 60 --warmup 5`, run from this commit and from its parent, three times each

Each part prints one JSON line; redirect into profiles/varstep_<part>.json.

    python scripts/varstep_profile.py revalue stale ratio adaptive [--scale 0.43] [--scheme bdf2]
"""
import argparse
import copy
import functools
import json
import math
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


@functools.lru_cache(maxsize=None)
def case(scale):
    from conftest import build_case

    return build_case("geballe_with_diamond", scale)


def problem(scale, scheme, num_steps=100, t_final=None, smooth=False):
    from helpers import make_problem

    from heatflow_amd.hip_backend import PC_AMG

    cfg, stack, mesh = case(scale)
    cfg = copy.deepcopy(cfg)
    cfg["timing"]["num_steps"] = num_steps
    if t_final is not None:
        cfg["timing"]["t_final"] = t_final
    prob = make_problem(cfg, stack, mesh, precond=PC_AMG, scheme=scheme)
    if smooth:      # the heated line follows a Gaussian in time: FWHM 1 us, 500 K, centred at 1.5 us
        ic, coeff = float(cfg["heating"]["ic_temp"]), -4.0 * math.log(2.0) / float(cfg["heating"]["fwhm"]) ** 2
        prob.bcs[3]._value = lambda x, y, t: ic + 500.0 * math.exp(-4.0 * math.log(2.0) * (t - 1.5e-6) ** 2 / 1e-12) * np.exp(
            coeff * np.asarray(y) ** 2)
    return prob, cfg, mesh


def timed_list(prob, dts):
    t0 = time.perf_counter()
    _, _, iters = prob.run_steps(dts, time_varying=[prob.bcs[3]])
    return time.perf_counter() - t0, np.asarray(iters)


def part_revalue(args):
    prob, _, _ = problem(args.scale, args.scheme)
    try:
        n = 40
        timed_list(prob, [prob.dt] * 10)                                   # warm-up
        same, it_same = timed_list(prob, [prob.dt] * n)
        alt, it_alt = timed_list(prob, [prob.dt * (1.0 if k % 2 else 0.8) for k in range(n)])
        info = prob.backend.step_info()
        return {"part": "revalue", "n_dof": prob.n, "steps": n, "seconds_equal_steps": same, "seconds_alternating": alt,
                "iterations_equal": int(it_same.sum()), "iterations_alternating": int(it_alt.sum()), "revaluations": info["revaluations"],
                "note": "the difference holds the re-valuations, the stale value lists and the changed iteration counts; "
                        "rocprofv3 --kernel-trace --stats of this part gives k_assemble_rows + k_bc_rows + k_dinv alone"}
    finally:
        prob.close()


def part_stale(args):
    prob, _, _ = problem(args.scale, args.scheme)
    try:
        timed_list(prob, [prob.dt] * 10)
        fresh, it_f = timed_list(prob, [prob.dt] * 30)                     # A's value lists valid
        timed_list(prob, [0.9 * prob.dt, prob.dt])                         # two re-valuations: back at the assembled dt', lists stale
        stale, it_s = timed_list(prob, [prob.dt] * 30)
        return {"part": "stale", "n_dof": prob.n, "seconds_lists_valid": fresh, "iterations_valid": int(it_f.sum()),
                "seconds_lists_stale": stale, "iterations_stale": int(it_s.sum()),
                "ms_per_iteration_valid": 1e3 * fresh / max(int(it_f.sum()), 1), "ms_per_iteration_stale": 1e3 * stale / max(int(it_s.sum()), 1)}
    finally:
        prob.close()


def part_ratio(args):
    rows = []
    for r in (0.01, 0.03, 0.1, 0.3, 1.0, 3.0, 10.0, 30.0, 100.0):
        prob, _, _ = problem(args.scale, "backward_euler")                 # dt' = dt: the ratio is the step's own
        try:
            _, iters = timed_list(prob, [r * prob.dt] * 6)
            rows.append({"ratio": r, "iterations_per_step": iters.tolist(), "fallbacks": prob.backend.amg_info()["jacobi_fallbacks"]})
        finally:
            prob.close()
    return {"part": "ratio", "rows": rows}


def part_adaptive(args):
    out = {"part": "adaptive"}
    prob, _, _ = problem(args.scale, "bdf2", t_final=3.0e-5, smooth=True)
    try:
        t0 = time.perf_counter()
        _, _, _, info = prob.run_adaptive(3.0e-5, args.tol, time_varying=[prob.bcs[3]])
        out.update(n_dof=prob.n, adaptive_seconds=time.perf_counter() - t0, accepted=info["accepted"], rejected=info["rejected"],
                   revaluations=info["revaluations"], iterations=int(np.sum(prob.iters)))
    finally:
        prob.close()
    prob, _, _ = problem(args.scale, "bdf2", num_steps=args.fixed_steps, t_final=3.0e-5, smooth=True)
    try:
        t0 = time.perf_counter()
        _, _, iters = prob.run(args.fixed_steps, time_varying=[prob.bcs[3]])
        out.update(fixed_steps=args.fixed_steps, fixed_seconds=time.perf_counter() - t0, fixed_iterations=int(np.sum(iters)))
    finally:
        prob.close()
    return out


PARTS = {"revalue": part_revalue, "stale": part_stale, "ratio": part_ratio, "adaptive": part_adaptive}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("parts", nargs="+", choices=sorted(PARTS))
    ap.add_argument("--scale", type=float, default=0.43, help="factor on every mats.*.mesh (0.43: 1.04 M DOF; 8: the tests' 5.7 k)")
    ap.add_argument("--scheme", default="bdf2")
    ap.add_argument("--tol", type=float, default=0.1)
    ap.add_argument("--fixed-steps", type=int, default=800)
    args = ap.parse_args()
    for name in args.parts:
        print(json.dumps(PARTS[name](args)), flush=True)


if __name__ == "__main__":
    main()
