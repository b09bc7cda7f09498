"""The bits on both sides of every seam between "the system being solved" and "the batch state being stepped" in the native library:
the steady operator (hf_ctx::Steady::sys) next to the transient one (hf_ctx::sys), and the tangent, read-flux and batched read-flux
states (tanb, fluxb, fluxnb) next to the caller's batch.  Output arrays are pinned as SHA-256 digests and iteration counts as
integers in tests/golden/seam_bits.json, recorded with scripts/seam_bits_record.py from the library of the commit before the
operator and the batch state became arguments (then fields traded in and out of the context); the recorder was run twice, in two
separate processes, and wrote the same file both times.  No tolerance anywhere.

Per small case, through the backend's public calls only, from the seeded state and the tables of tests/test_gpu_rowgather_bits.py:
  steady.*    a transient assembled with one preconditioner on one Dirichlet set and a steady set-up with the other preconditioner
              on another set, (transient, steady) = (0, 1), (1, 0) and (1, 0) with amg_reuse: steady_solve without and with a load,
              hold_load, three run steps with non-zero boundary values, a second steady_solve, three more steps
  picard.*    kappa tables, steady_picard_setup / steady_picard_solve with max_sweeps 3 for both preconditioners (the transient has
              the other one), then two transient steps
  tangent.*   run_tangent for three steps on a non-empty Dirichlet set with non-zero h_all (the lifting of the columns), nv 2 and 4,
              both preconditioners, both schemes; then a caller's batch on the same context (two batch_run steps) and one run step
  flux.*      flux_solve for the pair and each component alone, and batch_run with flux_components=3, nv 2, two steps, for the
              shared, per-column and affine operator kinds under the multigrid preconditioner
A wrong system, preconditioner choice, lifting or batch state changes bits or counts.  The mesh arrays are pinned too: if they move,
the digests mean nothing and the failure names the mesher."""
import hashlib
import json
import os

import numpy as np
import pytest

from test_gpu_rowgather_bits import _inputs

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "seam_bits.json")
CASES = {"geballe_with_diamond": "case_with_diamond_small", "geballe_no_diamond": "case_no_diamond_small"}
GROUPS = ("steady", "picard", "tangent", "flux")
MESH_KEYS = ("coords", "tris", "tags")
SCHEMES = ("be", "bdf2")


def _context(hip, mesh, p, precond=0, reuse=False, scheme="be", ktab=False):
    """An assembled transient on the Dirichlet set p["dofs"] with the given preconditioner."""
    tags = sorted(p["tk"])
    be = hip.HeatflowHIP(0)
    be.set_mesh(mesh.coords, mesh.tris, mesh.tags)
    be.set_materials(tags, [p["tk"][t] for t in tags], [p["trc"][t] for t in tags])
    be.set_dirichlet(p["dofs"])
    be.set_precond(precond, reuse)
    if scheme == "bdf2":
        be.set_time_scheme(hip.TIME_BDF2)
    if ktab:
        be.set_kappa_tables(p["ktab"])
    be.set_state(p["u"])
    be.assemble(p["dt"], hip.ASM_ROW_GATHER)
    return be


def _seam_inputs(case):
    """_inputs plus a transient Dirichlet set other than the steady one, and boundary values for both (sums and products of small
    integers and powers of two: the same numbers on every host)."""
    p = dict(_inputs(case))
    n = len(p["u"])
    p["dofs"] = np.arange(3, n, 37, dtype=np.int32)
    nb, nsb = len(p["dofs"]), len(p["steady_dofs"])
    p["g"] = np.stack([300.0 + 4.0 * (k + 1) + 0.5 * (np.arange(nb) % 5) for k in range(6)])
    p["gs"] = [320.0 + 2.0 * (np.arange(nsb) % 11), 290.0 + 3.0 * (np.arange(nsb) % 7)]
    p["all"] = np.arange(n, dtype=np.int32)
    return p


def _steady(hip, mesh, p, out):
    for pt, ps, reuse in ((0, 1, False), (1, 0, False), (1, 0, True)):
        name = f"steady.t{pt}_s{ps}{'.reuse' if reuse else ''}"
        with _context(hip, mesh, p, precond=pt, reuse=reuse) as be:
            be.steady_setup(p["steady_dofs"], ps)
            be.hold_load()                                                   # a load of physical size: K u of the seeded state
            be.set_state(p["u"])
            it0, res0 = be.steady_solve(p["gs"][0], use_load=False)
            out[name + ".solve_noload"] = be.get_state()
            be.set_state(p["u"])
            it1, res1 = be.steady_solve(p["gs"][0], use_load=True)
            out[name + ".solve_load"] = be.get_state()
            be.hold_load()
            out[name + ".run_a"], ita = be.run(p["g"][:3], nodes=p["all"])   # every state of three steps
            it2, res2 = be.steady_solve(p["gs"][1], use_load=True)
            out[name + ".solve_again"] = be.get_state()
            out[name + ".run_b"], itb = be.run(p["g"][3:], nodes=p["all"])
            out[name + ".resid"] = np.array([res0, res1, res2])
            out[name + ".iters"] = [int(it0), int(it1), int(it2)] + [int(v) for v in ita] + [int(v) for v in itb]


def _picard(hip, mesh, p, out):
    for ps in (0, 1):
        name = f"picard.s{ps}"
        with _context(hip, mesh, p, precond=1 - ps, ktab=True) as be:
            be.steady_picard_setup(p["steady_dofs"], ps)
            try:
                be.steady_picard_solve(p["gs"][0], max_sweeps=3)
            except hip.NotConverged:                                         # three sweeps: the figures of the last one are pinned
                pass
            info = be.last_picard
            out[name + ".state"] = be.get_state()
            out[name + ".change"] = np.array([info["change"], info["nl_resid"]])
            out[name + ".run"], it = be.run(p["g"][:2], nodes=p["all"])
            out[name + ".iters"] = [int(info["sweeps"])] + [int(v) for v in info["iters"]] + [int(v) for v in it]


def _tangent(hip, mesh, p, out):
    tags = sorted(p["tk"])
    nb = len(p["dofs"])
    for scheme in SCHEMES:
        for precond in (0, 1):
            with _context(hip, mesh, p, precond=precond, scheme=scheme) as be:
                for nv in (2, 4):
                    name = f"tangent.nv{nv}.p{precond}.{scheme}"
                    be.set_state(p["u"])
                    be.tangent_setup(nv, {tag: q % nv for q, tag in enumerate(tags)})
                    h = np.stack([[(0.25 * (k + 1) + 0.125 * (q % 3)) * (j + 1.0) for j in range(nv)] for k in range(3) for q in range(nb)])
                    s, it, ts, tit = be.run_tangent(p["g"][:3], h.reshape(3, nb, nv), nodes=p["all"])
                    out[name + ".samples"], out[name + ".tangent_samples"] = s, ts
                    for j in range(nv):
                        out[f"{name}.col{j}"] = be.get_tangent(j)
                    out[name + ".iters"] = [int(v) for v in it] + [int(v) for v in tit.ravel()]
                    # the caller's batch after the tangent state, then a plain step: nothing of either is left behind
                    be.batch_begin(2, per_column_operator=hip.BATCH_SHARED)
                    be.batch_set_state(0, p["u"])
                    be.batch_set_state(1, p["u"][::-1])
                    bs, bit = be.batch_run(np.repeat(p["g"][3:5, :, None], 2, axis=2), nodes=p["all"])
                    be.batch_end()
                    out[name + ".batch"] = bs
                    out[name + ".run"], rit = be.run(p["g"][5:], nodes=p["all"])
                    out[name + ".iters_after"] = [int(v) for v in bit.ravel()] + [int(v) for v in rit]


def _flux(hip, mesh, p, out):
    nodes = np.arange(0, len(p["u"]), 7, dtype=np.int32)
    with hip.HeatflowHIP(0) as be:
        be.set_mesh(mesh.coords, mesh.tris, mesh.tags)
        be.flux_setup()
        its = []
        for name, wz, wr, w in (("pair", True, True, 1.0), ("z", True, False, 0.0), ("r", False, True, 0.75)):
            be.set_state(w * p["u"] + (1.0 - w) * p["u"][::-1])               # a state of its own each: no solve starts converged
            its +=[int(v) for v in be.flux_solve(1e-8, 5000, want_z=wz, want_r=wr)]
            gz, gr = be.flux_sample(nodes, want_z=wz, want_r=wr)
            out[f"flux.{name}"] = np.stack([a for a in (gz, gr) if a is not None])
        out["flux.iters"] = its
    tag = mesh.material_tags["p_sample"]
    k0 = p["tk"][tag]
    for kind, code in (("shared", hip.BATCH_SHARED), ("percol", hip.BATCH_PER_COLUMN), ("affine", hip.BATCH_AFFINE)):
        with _context(hip, mesh, p, precond=1, reuse=True) as be:
            be.flux_setup()
            be.batch_begin(2, per_column_operator=code)
            if code == hip.BATCH_PER_COLUMN:
                for j in range(2):
                    be.update_kappa([tag], [k0 * (1.0 + 0.25 * j)])
                    be.batch_load_column(j)
            elif code == hip.BATCH_AFFINE:
                be.batch_set_affine([tag], [-0.25 * k0, 0.125 * k0])
            be.batch_set_state(0, p["u"])
            be.batch_set_state(1, p["u"][::-1])
            s, it, fl = be.batch_run(np.repeat(p["g"][:2, :, None], 2, axis=2), nodes=p["all"], flux_nodes=nodes, flux_components=3,
                                     flux_rtol=1e-8)
            out[f"flux.batch.{kind}.states"], out[f"flux.batch.{kind}.flux"] = s, fl
            out[f"flux.batch.{kind}.iters"] = [int(v) for v in it.ravel()] + [int(v) for v in be.last_flux_iters.ravel()]
            be.batch_end()


RUNNERS = {"steady": _steady, "picard": _picard, "tangent": _tangent, "flux": _flux}


def results(hip, case, group):
    """{name: array | list of int} of the mesh arrays and of what the group's calls return."""
    mesh = case[2]
    out = {"coords": np.asarray(mesh.coords, dtype=np.float64), "tris": np.asarray(mesh.tris, dtype=np.int32),
           "tags": np.asarray(mesh.tags, dtype=np.int32)}
    RUNNERS[group](hip, mesh, _seam_inputs(case), out)
    return out


def digests(hip, case, group):
    """{name: SHA-256 | list of int} of results(); refuses an array that is all zeros (it would pin nothing)."""
    got = results(hip, case, group)
    dead = [k for k, a in got.items() if not isinstance(a, list) and not np.any(a)]
    assert not dead, f"all zeros: {dead}"
    return {k: a if isinstance(a, list) else hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest() for k, a in got.items()}


def _differ(got, group):
    """Digests that must not coincide: they would if a call had run on the other side of its seam."""
    arrays = [k for k, v in got.items() if not isinstance(v, list) and k not in MESH_KEYS and not k.endswith((".resid", ".change"))]
    if group == "steady":
        for name in {k.rsplit(".", 1)[0] for k in arrays}:                   # steady states against transient states
            states = [got[f"{name}.{s}"] for s in ("solve_noload", "solve_load", "run_a", "solve_again", "run_b")]
            assert len(set(states)) == len(states), name
        a, b = "steady.t0_s1", "steady.t1_s0"                                # preconditioner 0 against 1
        for lo, hi, keys in ((0, 3, ("solve_noload", "solve_load", "solve_again")), (3, 9, ("run_a", "run_b"))):
            if got[a + ".iters"][lo:hi] != got[b + ".iters"][lo:hi]:
                assert all(got[f"{a}.{k}"] != got[f"{b}.{k}"] for k in keys)
    elif group == "picard":
        assert got["picard.s0.state"] != got["picard.s0.run"] and got["picard.s1.state"] != got["picard.s1.run"]
        if got["picard.s0.iters"] != got["picard.s1.iters"]:
            assert got["picard.s0.state"] != got["picard.s1.state"]
    elif group == "tangent":
        for k in arrays:
            if k.endswith(".col0"):
                assert got[k] != got[k[:-1] + "1"], k                        # column 0 against column 1
        for scheme in SCHEMES:
            for nv in (2, 4):
                a, b = f"tangent.nv{nv}.p0.{scheme}", f"tangent.nv{nv}.p1.{scheme}"
                if got[a + ".iters"] != got[b + ".iters"]:
                    assert got[a + ".tangent_samples"] != got[b + ".tangent_samples"]
    else:
        kinds = [got[f"flux.batch.{k}.flux"] for k in ("shared", "percol", "affine")]
        assert len(set(kinds)) == 3 and len({got["flux.pair"], got["flux.z"], got["flux.r"]}) == 3


@pytest.mark.parametrize("group", GROUPS)
@pytest.mark.parametrize("case", sorted(CASES))
def test_every_seam_gives_the_recorded_bits(hip, request, case, group):
    with open(GOLDEN) as f:
        want = json.load(f)[case][group]
    got = digests(hip, request.getfixturevalue(CASES[case]), group)          # (asserts that no pinned array is all zeros)
    assert sorted(got) == sorted(want)
    moved = [k for k in MESH_KEYS if got[k] != want[k]]
    assert not moved, f"the mesher gives other {moved} for {case} than when the fixture was recorded: the library was not compared"
    _differ(got, group)
    wrong = [k for k in got if got[k] != want[k]]
    assert not wrong, f"{case}: other bits or counts than recorded in {wrong}"
