"""Cost and shape of the value lists (hf_set_value_lists) on one mesh:
python scripts/value_lists_profile.py [mesh scale = 0.43] [steps = 100]

Per mode 0 / 1: GPU time of hf_assemble (HIP events around assembly, elimination, D^-1 and - mode 1 - the builder; median of 7
calls after a first one), then `steps` time steps of the multigrid-PCG loop (hf_run, GPU ms per step by events, iterations), and
hf_time_kernel of the three SpMV launches it knows (y = A x, b = M u, iteration head).  HEATFLOW_VALUE_LISTS_VCAP=<entries> moves
the share of a list that is staged in LDS (see value_lists_vcap in hf_pattern.hpp)."""
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from conftest import build_case          # noqa: E402
from helpers import make_problem        # noqa: E402
from heatflow_amd import hip_backend as hb   # noqa: E402


def main():
    scale = float(sys.argv[1]) if len(sys.argv) > 1 else 0.43
    steps = int(sys.argv[2]) if len(sys.argv) > 2 else 100
    cfg, stack, mesh = build_case("geballe_with_diamond", scale)
    fields = {}
    for mode in (0, 1):
        be = hb.HeatflowHIP(0)
        be.set_value_lists(mode)
        prob = make_problem(cfg, stack, mesh, backend=be, precond=1)
        try:
            asm = []
            for _ in range(8):
                be.assemble(prob.dt, hb.ASM_ROW_GATHER)
                asm.append(be.last_gpu_ms())
            info = [be.get_value_lists(w) for w in (0, 1)]
            prob.set_state(float(cfg["heating"]["ic_temp"]))
            _, _, iters = prob.run(steps)
            run_ms = be.last_gpu_ms()
            fields[mode] = prob.state()
            kern = {name: be.time_kernel(code, 50) * 1e3 for name, code in
                    (("y=Ax", hb.K_SPMV), ("b=Mu", hb.K_RHS), ("head", hb.K_PCG_SPMV))}
            print(f"scale {scale} n {prob.n} nnz {be.nnz} mode {mode}: hf_assemble {statistics.median(asm[1:]) * 1e3:.1f} us (median of 7) | "
                  f"{steps} steps {run_ms:.2f} ms = {run_ms / steps * 1e3:.1f} us per step, {np.mean(iters):.2f} iterations per step | "
                  + " ".join(f"{k} {v:.1f} us" for k, v in kern.items())
                  + " | " + " ".join(f"{'AM'[w]}: valid {int(t['valid'])} share {t['sum_vlist'] / be.nnz:.4f} longest {t['max_vlist']} vcap {t['vcap']}"
                                     for w, t in enumerate(info)), flush=True)
        finally:
            be.close()
    print("fields of the two modes bit-identical:", bool(np.array_equal(fields[0], fields[1])), flush=True)


if __name__ == "__main__":
    main()
