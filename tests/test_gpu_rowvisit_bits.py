"""The bits of the eight row-visit load kernels (k_grad_rows, k_tangent_load<2,4,8,16>, k_tangent_load_dir<2,4>, k_tangent_load_cap<2,4>,
k_tangent_load_shape<1,2,4>, k_source_load, k_source_load_d and k_tangent_load_T<2,4>; k_grad_rows, k_source_load and
k_tangent_load_shape share the body rowgather_visit in hf_kernels.hpp) and of the launch site of kb_source_columns, pinned as
SHA-256 digests in tests/golden/rowvisit_bits.json.  The file was recorded with scripts/rowvisit_bits_record.py from the library of
the commit before any of them was touched; the recorder was run twice, in two separate processes, and wrote the same file both
times.  No tolerance anywhere.

Per small case, through the backend's public calls only, from the seeded state and the tables of tests/test_gpu_rowgather_bits.py
(IEEE basic operations only, so the inputs are the same numbers on every host):
  load.*      tangent_setup with 2, 3, 5 and 9 parameters, every column of tangent_load
  dir.*       set_anisotropy, tangent_setup_dir with k, r and z columns (a tag with equal and one with unequal multipliers)
  cap.*       tangent_set_capacity: columns and loads after one run_tangent step (backward Euler) and after two (BDF2)
  shape.*     tangent_set_shape on 1, 2 and 3 columns, with and without multipliers set, both schemes
  source.*    get_source() for a uniform and a finite depth, get_source_derivative(0 / 1), and the columns after one step with
              tangent_set_source
  tables.*    kappa tables alone and with rho_c tables, table_derivatives and tangent_set_tables with an entry of each kind, both
              schemes
  grad.*      the right-hand sides of flux_system() after flux_solve for z alone, r alone and the pair, and the flux samples of one
              batch_run step with nv = 2
The mesh arrays are pinned too: if they move, the digests mean nothing and the failure names the mesher."""
import hashlib
import json
import os

import numpy as np
import pytest

from test_gpu_rowgather_bits import _inputs

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "rowvisit_bits.json")
CASES = {"geballe_with_diamond": "case_with_diamond_small", "geballe_no_diamond": "case_no_diamond_small"}
MESH_KEYS = ("coords", "tris", "tags")
SCHEMES = ("be", "bdf2")


def _sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def _context(hip, mesh, p, scheme="be", aniso=False, ktab=False, ctab=False, source=None):
    tags = sorted(p["tk"])
    be = hip.HeatflowHIP(0)
    be.set_mesh(mesh.coords, mesh.tris, mesh.tags)
    be.set_materials(tags, [p["tk"][t] for t in tags], [p["trc"][t] for t in tags])
    if aniso:
        be.set_anisotropy(p["aniso"])
    if source is not None:
        be.set_source(*source)
    be.set_dirichlet(np.zeros(0, dtype=np.int32))
    if scheme == "bdf2":
        be.set_time_scheme(hip.TIME_BDF2)
    if ktab:
        be.set_kappa_tables(p["ktab"])
    if ctab:
        be.set_rhoc_tables(p["ctab"])
    be.set_state(p["u"])
    be.assemble(p["dt"], hip.ASM_ROW_GATHER)
    return be


def _loads(be):
    return np.stack([be.tangent_load(j) for j in range(be.tangent_nv)], axis=1)


def _columns(be):
    return np.stack([be.get_tangent(j) for j in range(be.tangent_nv)], axis=1)


def _run(be, scheme):
    """One step under backward Euler, two under BDF2 (the second one has u^{n-1}); the columns and the loads at the state reached."""
    be.run_tangent(np.zeros((2 if scheme == "bdf2" else 1, 0)))
    return _columns(be), _loads(be)


def arrays(hip, case):
    """{name: array} of the mesh arrays and of what each of the eight kernels writes."""
    cfg, stack, mesh = case
    p = _inputs(case)
    t = mesh.material_tags
    tags = sorted(p["tk"])
    ins = sorted(v for name, v in t.items() if name.endswith("ins"))
    sample, coupler = t["p_sample"], t["p_coupler"]
    z, r = mesh.coords[:, 0], mesh.coords[:, 1]
    zn, rn = (z - z.min()) / (z.max() - z.min()), r / r.max()
    vz = [(zn * (1.0 - zn)) * (1.0 + (s + 1.0) * rn) + 0.25 * (s + 1.0) * zn for s in range(3)]   # nodal velocities of the shape columns
    out = {"coords": np.asarray(mesh.coords, dtype=np.float64), "tris": np.asarray(mesh.tris, dtype=np.int32),
           "tags": np.asarray(mesh.tags, dtype=np.int32)}

    with _context(hip, mesh, p) as be:                                             # k_tangent_load<2, 4, 8, 16>
        for npar in (2, 3, 5, 9):
            be.tangent_setup(npar, {tag: q % npar for q, tag in enumerate(tags)})
            out[f"load.nv{be.tangent_nv}"] = _loads(be)

    with _context(hip, mesh, p, aniso=True) as be:                                 # k_tangent_load_dir<2, 4>: both branches of the visit
        for npar in (2, 3):
            be.tangent_setup_dir(npar, k={sample: 0, ins[0]: 1}, r={ins[1]: 0, coupler: npar - 1}, z={ins[1]: 1})
            out[f"dir.nv{be.tangent_nv}"] = _loads(be)

    for scheme in SCHEMES:                                                         # k_tangent_load_cap<2, 4>
        with _context(hip, mesh, p, scheme=scheme) as be:
            for npar in (2, 3):
                be.set_state(p["u"])
                be.tangent_setup(npar, {coupler: 0})
                be.tangent_set_capacity({sample: 0, ins[0]: 1, ins[1]: npar - 1})
                out[f"cap.nv{be.tangent_nv}.{scheme}.cols"], out[f"cap.nv{be.tangent_nv}.{scheme}.load"] = _run(be, scheme)

    for scheme in SCHEMES:                                                         # k_tangent_load_shape<1, 2, 4>
        for mult in (False, True):
            with _context(hip, mesh, p, scheme=scheme, aniso=mult) as be:
                for ncol in (1, 2, 3):
                    be.set_state(p["u"])
                    be.tangent_setup(3, {coupler: 0})
                    for j in range(ncol):
                        be.tangent_set_shape(j, vz[j])
                    name = f"shape.ns{(1, 2, 4)[ncol - 1]}.{'multipliers' if mult else 'plain'}.{scheme}"
                    out[name + ".cols"], out[name + ".load"] = _run(be, scheme)

    fwhm, z0 = float(cfg["heating"]["fwhm"]), float(stack.heated_z)                 # k_source_load, k_source_load_d, kb_source_columns
    absorbing = [sample, ins[0]]
    with _context(hip, mesh, p, source=(absorbing, fwhm, z0, float("inf"))) as be:
        out["source.uniform"] = be.get_source()
        be.set_source(absorbing, fwhm, z0, 2.0e-6)
        out["source.finite"] = be.get_source()
        be.source_derivatives(True)
        out["source.d_fwhm"], out["source.d_depth"] = be.get_source_derivative(0), be.get_source_derivative(1)
        be.set_source_amplitudes([1.0e12])
        be.tangent_setup(2, {coupler: 0})
        be.tangent_set_source(np.array([[[1.0e12, 0.0, 0.0], [0.0, 2.0e17, -3.0e17]]]))
        be.run_tangent(np.zeros((1, 0)))
        out["source.cols"] = _columns(be)

    nk = len(p["ktab"][ins[0]][2])                                                 # k_tangent_load_T<2, 4>
    ramp = np.arange(nk) / float(nk - 1)
    for scheme in SCHEMES:
        for both in (False, True):
            with _context(hip, mesh, p, scheme=scheme, ktab=True, ctab=both) as be:
                be.table_derivatives(True)
                for npar in (2, 3):
                    be.set_state(p["u"])
                    be.tangent_setup(npar, {sample: 0})
                    be.tangent_set_tables(0, {(npar - 1, ins[0]): p["ktab"][ins[0]][2] * (1.0 - 0.5 * ramp),
                                              (0, ins[1]): p["ktab"][ins[1]][2] * (0.25 + ramp)})
                    if both:
                        be.tangent_set_tables(1, {(1, ins[1]): p["ctab"][ins[1]][2] * (0.5 + ramp * ramp)})
                    name = f"tables.nv{be.tangent_nv}.{'both' if both else 'kappa'}.{scheme}"
                    out[name + ".cols"], out[name + ".load"] = _run(be, scheme)

    with hip.HeatflowHIP(0) as be:                                                 # k_grad_rows: stride 1 and stride 2
        be.set_mesh(mesh.coords, mesh.tris, mesh.tags)
        be.flux_setup()
        be.set_state(p["u"])
        be.flux_solve(1e-2, 5000, want_z=True, want_r=False)
        out["grad.z"] = be.flux_system(want_r=False)["bz"]
        be.flux_solve(1e-2, 5000, want_z=False, want_r=True)
        out["grad.r"] = be.flux_system(want_z=False)["br"]
        be.flux_solve(1e-2, 5000)
        s = be.flux_system()
        out["grad.pair.z"], out["grad.pair.r"] = s["bz"], s["br"]
    with _context(hip, mesh, p) as be:                                             # ... and the column stride of a batch
        be.flux_setup()
        be.batch_begin(2, per_column_operator=hip.BATCH_SHARED)
        be.batch_set_state(0, p["u"])
        be.batch_set_state(1, p["u"][::-1])
        nodes = np.arange(0, len(z), 7, dtype=np.int32)
        out["grad.batch"] = be.batch_run(np.zeros((1, 0, 2)), flux_nodes=nodes, flux_components=3, flux_rtol=1e-6)[2]
        be.batch_end()
    return out


def digests(hip, case):
    """{name: SHA-256} of arrays(); refuses an array that is all zeros (it would pin nothing)."""
    got = arrays(hip, case)
    dead = [k for k, a in got.items() if not np.any(a)]
    assert not dead, f"all zeros: {dead}"
    return {k: _sha(a) for k, a in got.items()}


@pytest.mark.parametrize("case", sorted(CASES))
def test_every_row_visit_kernel_writes_the_recorded_bits(hip, request, case):
    with open(GOLDEN) as f:
        want = json.load(f)[case]
    got = digests(hip, request.getfixturevalue(CASES[case]))                   # (asserts that no pinned array is all zeros)
    assert sorted(got) == sorted(want)
    moved = [k for k in MESH_KEYS if got[k] != want[k]]
    assert not moved, f"the mesher gives other {moved} for {case} than when the fixture was recorded: the kernels were not compared"
    ops = [k for k in got if k not in MESH_KEYS and not k.startswith("grad.pair.")]
    assert len({got[k] for k in ops}) == len(ops)                              # every entry pins something of its own ...
    assert got["grad.pair.z"] == got["grad.z"] and got["grad.pair.r"] == got["grad.r"]   # ... but the pair: stride 2 writes the plain arrays' bits
    wrong = [k for k in got if got[k] != want[k]]
    assert not wrong, f"{case}: other bits than recorded in {wrong}"
