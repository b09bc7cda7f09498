#!/usr/bin/env python
"""Measurements for the sweeps under the laser-power source with per-point monitors.  Run from the repository root on
an MI355X; nothing in the tests or bench.py runs it.

    python scripts/batch_source_profile.py monitors [--scale 0.43] [--repeat 50]
        (a) wall time per record: batch_monitor_now at nv = 8 and 16 against nv monitor_now calls, six monitored tags
    python scripts/batch_source_profile.py step [--scale 0.43] [--steps 20]
        (b) per-step time of a 16-column batch (hf_batch_run's own GPU clock) without and with the source, and with source and monitors
    python scripts/batch_source_profile.py sweep [--scale 0.43] [--steps 100] [--points 16]
        (c) wall time of a 16-point beam-width sweep under cfgs/geballe_with_diamond_source.yaml through
            run_parameter_sweep --batch 16 and --batch 1

Kernel times come from a trace of their own, e.g.
    rocprofv3 --kernel-trace --stats -d profiles/batch_source_trace -- python scripts/batch_source_profile.py monitors --repeat 20
(kb_monitor<8>, kb_monitor<16>, kb_monitor_final, k_monitor, k_monitor_final; with `step`: kb_source_load<16>).  Counters are
collected in runs of their own, never together with a trace.
"""
import argparse
import copy
import json
import os
import sys
import tempfile
import time

import numpy as np
import yaml

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

MONITORED = ("p_sample", "p_ins", "p_coupler", "o_coupler", "o_ins", "g_ins")


def _config(scale, steps):
    from heatflow_amd.geometry import scale_mesh_sizes

    with open(os.path.join(ROOT, "cfgs", "geballe_with_diamond_source.yaml")) as f:
        cfg = scale_mesh_sizes(yaml.safe_load(f), scale)
    dt = float(cfg["timing"]["t_final"]) / int(cfg["timing"]["num_steps"])
    cfg["timing"] = dict(cfg["timing"], num_steps=steps, t_final=steps * dt, sweep_monitors=True)
    cfg["heating"]["source"]["sweeps"] = True
    cfg["heating"]["source"].pop("fwhm", None)               # the beam follows heating.fwhm: the sweep's fwhm axis scans it
    cfg["heating"]["source"]["pulse"] = {"t0": 0.5 * steps * dt, "fwhm": 0.4 * steps * dt}
    cfg["monitors"] = {"sample": {"material": "p_sample", "above": 320.0}, "layers": {"material": list(MONITORED[1:])}}
    return cfg


def _session(cfg):
    from heatflow_amd.driver import SimulationSession
    from heatflow_amd.geometry import build_stack
    from heatflow_amd.mesh import Mesh

    stack = build_stack(cfg)
    mesh = Mesh("mesh.msh", stack.bounds, stack.materials).build_mesh()
    return SimulationSession(mesh.coords, mesh.tris, mesh.tags, mesh.material_tags), stack, mesh


def _columns(cfg, nv):
    out = []
    for f in np.geomspace(8.0e-6, 3.0e-5, nv):
        c = copy.deepcopy(cfg)
        c["heating"]["fwhm"] = float(f)
        out.append(c)
    return out


def monitors(args):
    cfg = _config(args.scale, 4)
    session, stack, mesh = _session(cfg)
    out = {"n_dof": int(len(mesh.coords)), "n_triangles": int(len(mesh.tris)), "monitored_tags": len(MONITORED)}
    try:
        single = copy.deepcopy(cfg)
        del single["heating"]["source"]
        del single["monitors"]
        session.prepare(single, stack)
        be = session.problem.backend
        rng = np.random.default_rng(3)
        be.set_monitors({mesh.material_tags[m]: (320.0 if m == "p_sample" else None) for m in MONITORED})
        u = 300.0 + 50.0 * rng.random(len(mesh.coords))
        be.set_state(u)
        be.monitor_now()
        t0 = time.perf_counter()
        for _ in range(args.repeat):
            be.monitor_now()
        out["monitor_now_us"] = (time.perf_counter() - t0) / args.repeat * 1e6
        for nv in (8, 16):
            be.batch_begin(nv)
            for j in range(nv):
                be.batch_set_state(j, u + j)
            be.batch_set_monitors(True)
            be.batch_monitor_now()
            t0 = time.perf_counter()
            for _ in range(args.repeat):
                be.batch_monitor_now()
            out[f"batch_monitor_now_nv{nv}_us"] = (time.perf_counter() - t0) / args.repeat * 1e6
            out[f"nv{nv}_single_records_us"] = nv * out["monitor_now_us"]
            be.batch_end()
    finally:
        session.close()
    print(json.dumps(out))


def step(args):
    from heatflow_amd.parameter_sweep import get_watcher_points

    nv = 16
    cfg = _config(args.scale, args.steps)
    session, stack, mesh = _session(cfg)
    out = {"n_dof": int(len(mesh.coords)), "nv": nv, "steps": args.steps}
    try:
        for label, with_source, with_monitors in (("plain", False, False), ("source", True, False), ("source_monitors", True, True)):
            c = copy.deepcopy(cfg)
            if not with_monitors:
                del c["monitors"]
            if not with_source:
                del c["heating"]["source"]
            cols = _columns(c, nv)
            for _ in range(2):                                # the second run is the warm one
                t0 = time.perf_counter()
                res = session.run_batch(cols, [stack] * nv, get_watcher_points(c))
                wall = time.perf_counter() - t0
            out[label] = {"gpu_ms_per_step": session.problem.backend.last_gpu_ms() / args.steps, "wall_s": wall,
                          "iters_mean": float(np.mean([r["iters"].mean() for r in res]))}
    finally:
        session.close()
    print(json.dumps(out))


def sweep(args):
    from heatflow_amd import parameter_sweep as ps

    cfg = _config(args.scale, args.steps)
    out = {"points": args.points, "steps": args.steps}
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "base.yaml")
        with open(path, "w") as f:
            yaml.safe_dump(cfg, f)
        width = float(cfg["mats"]["p_sample"]["z"])
        k = float(cfg["mats"]["p_sample"]["k"])
        for batch in (16, 1):
            t0 = time.perf_counter()
            ok, failed = ps.run_parameter_sweep(path, os.path.join(tmp, f"out{batch}"), (8.0e-6, 3.0e-5), (k, k), (width, width),
                                                (args.points, 1, 1), base_mesh_folder=os.path.join(tmp, "meshes"), batch=batch)
            out[f"batch{batch}_wall_s"] = time.perf_counter() - t0
            out[f"batch{batch}_ok"] = len(ok)
            out[f"batch{batch}_runtime_sum_s"] = float(sum(r["runtime"] for r in ok))
    out["ratio_batch1_over_batch16"] = out["batch1_runtime_sum_s"] / max(out["batch16_runtime_sum_s"], 1e-12)
    print(json.dumps(out))


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("what", choices=["monitors", "step", "sweep"])
    ap.add_argument("--scale", type=float, default=0.43, help="factor on every mats.*.mesh (0.43: 1.04 M DOF, as bench.py)")
    ap.add_argument("--repeat", type=int, default=50)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--points", type=int, default=16)
    args = ap.parse_args(argv)
    {"monitors": monitors, "step": step, "sweep": sweep}[args.what](args)
    return 0


if __name__ == "__main__":
    sys.exit(main())
