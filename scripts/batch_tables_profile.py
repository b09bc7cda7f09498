"""Measurements of DESIGN.md 3.23 (batches under tables) at 1.04 M DOF; needs an MI355X.

    python scripts/batch_tables_profile.py steps [out.json]
        ms per step (device events, hf_last_gpu_ms) and PCG iterations of the single run under the tables of
        cfgs/geballe_with_diamond_kT.yaml, of the batch of 8 columns under them, and of the constant-coefficient per-column batch
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o batch_tables -- python scripts/batch_tables_profile.py kernels [out.json]
        a run of its own: 22 alternated launches of kb_assemble_rows_T<8, false>, <16, false>, <8, true> and of the parent's
        alternative (k_assemble_rows_kT / _cT, eliminate(), the three kb_put_column of hf_batch_load_column)

MEASURE_SCALE (default 0.43: 1.04 M DOF) scales the mesh sizes; 8 gives the small test mesh for a rehearsal.
"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

from conftest import build_case  # noqa: E402
from helpers import make_problem, material_tables  # noqa: E402
from kappa_T_oracle import problem_inputs  # noqa: E402
from rhoc_T_oracle import einstein_tables  # noqa: E402

SCALE = float(os.environ.get("MEASURE_SCALE", "0.43"))
mode = sys.argv[1]
out = {"mode": mode, "scale": SCALE}
t0 = time.time()
cfg, stack, mesh = build_case("geballe_with_diamond_kT", SCALE)
n = len(mesh.coords)
out["n"] = n
print(f"mesh: {n} nodes in {time.time() - t0:.1f} s", flush=True)
tk, trc = material_tables(stack, mesh)
ktab = {mesh.material_tags[m.name]: m.properties["k_table"] for m in stack.materials if "k_table" in m.properties}
ctab = einstein_tables(trc, [mesh.material_tags[m.name] for m in stack.materials if m.name.endswith("ins")])
sample = mesh.material_tags["p_sample"]
hip = __import__("heatflow_amd.hip_backend", fromlist=["x"])


def open_tables(prob, nv, states):
    be = prob.backend
    be.set_batch_tables(True)
    be.batch_begin(nv, 1)
    for j in range(nv):
        be.batch_set_state(j, states[j])
        be.batch_set_column_kappa(j, [sample], [3.8 + 0.02 * j])


if mode == "kernels":
    _, _, dt, dofs, u0, g = problem_inputs(cfg, stack, mesh, 1)
    rng = np.random.default_rng(5)
    states = []
    for j in range(16):
        u = 250.0 + 700.0 * rng.random(n)
        u[dofs] = g[0]
        states.append(u)
    sk = make_problem(cfg, stack, mesh, kappa_tables=ktab)
    sc = make_problem(cfg, stack, mesh, kappa_tables=ktab, rhoc_tables=ctab)
    b8 = make_problem(cfg, stack, mesh, kappa_tables=ktab)
    b16 = make_problem(cfg, stack, mesh, kappa_tables=ktab)
    c8 = make_problem(cfg, stack, mesh, kappa_tables=ktab, rhoc_tables=ctab)
    pl = make_problem(cfg, stack, mesh)
    open_tables(b8, 8, states)
    open_tables(b16, 16, states)
    open_tables(c8, 8, states)
    pl.backend.batch_begin(8, 1)
    sk.backend.set_state(states[0])
    sc.backend.set_state(states[0])
    for it in range(22):                      # 2 warm + 20
        sk.backend.assemble(dt, hip.ASM_ROW_GATHER)      # k_assemble_rows, k_assemble_rows_kT, k_take_lift, k_bc_rows, k_dinv
        b8.backend.batch_revalue()
        sc.backend.assemble(dt, hip.ASM_ROW_GATHER)      # ... k_assemble_rows_cT
        b16.backend.batch_revalue()
        pl.backend.batch_load_column(it % 8)             # three kb_put_column
        c8.backend.batch_revalue()
    a = b8.backend.batch_get_operator(3)["A"]
    sk.set_materials({**tk, sample: 3.8 + 0.02 * 3}, trc, assemble=False)
    sk.backend.set_state(states[3])
    sk.backend.assemble(dt, hip.ASM_ROW_GATHER)
    out["column_3_bits_equal_single_run"] = bool(np.array_equal(a.view(np.uint64), sk.backend.get_csr()[2].view(np.uint64)))
    out["nnz"] = int(b8.backend.nnz)
    for p in (sk, sc, b8, b16, c8, pl):
        p.close()
else:
    W, K = 10, 20
    _, _, dt, dofs, u0, g = problem_inputs(cfg, stack, mesh, W + K)
    nodes = np.arange(0, n, 1000, dtype=np.int32)
    one = make_problem(cfg, stack, mesh, precond=1, kappa_tables=ktab)
    one.run(W, watcher_nodes=nodes, time_varying=[one.bcs[3]])
    _, s1, it1 = one.run(K, watcher_nodes=nodes, time_varying=[one.bcs[3]], first_step=W)
    out["single_tables_ms_per_step"] = one.backend.last_gpu_ms() / K
    out["single_tables_iters_mean"] = float(np.mean(it1))
    one.close()
    nv = 8
    g_all = np.stack([g] * nv, axis=2)
    bt = make_problem(cfg, stack, mesh, precond=1, amg_reuse=True, kappa_tables=ktab)
    open_tables(bt, nv, [u0] * nv)
    bt.backend.batch_run(g_all[:W], bt.rtol, 0.0, bt.max_it, nodes)
    s8, it8 = bt.backend.batch_run(g_all[W:], bt.rtol, 0.0, bt.max_it, nodes)
    out["batch8_tables_ms_per_step"] = bt.backend.last_gpu_ms() / K
    out["batch8_tables_iters_mean_per_column"] = [float(x) for x in np.mean(it8, axis=0)]
    out["batch8_column0_minus_single_K"] = float(np.abs(s8[:, 0] - np.asarray(s1)).max())
    out["amg_fallbacks"] = int(bt.backend.amg_info()["jacobi_fallbacks"])
    bt.close()
    pc = make_problem(cfg, stack, mesh, precond=1, amg_reuse=True)
    be = pc.backend
    be.batch_begin(nv, 1)
    for j in range(nv):
        be.update_kappa([sample], [3.8 + 0.02 * j])
        be.batch_load_column(j)
        be.batch_set_state(j, u0)
    be.batch_run(g_all[:W], pc.rtol, 0.0, pc.max_it, nodes)
    _, itc = be.batch_run(g_all[W:], pc.rtol, 0.0, pc.max_it, nodes)
    out["batch8_constant_percol_ms_per_step"] = be.last_gpu_ms() / K
    out["batch8_constant_percol_iters_mean_per_column"] = [float(x) for x in np.mean(itc, axis=0)]
    pc.close()
with open(sys.argv[2] if len(sys.argv) > 2 else f"batch_tables_{mode}.json", "w") as f:
    json.dump(out, f, indent=1)
print(json.dumps(out))
