"""The bits of the ten row-gather assembly kernels (rowgather_assemble in hf_kernels.hpp behind k_assemble_rows<false/true>,
k_assemble_rows_an<false/true>, k_assemble_rows_kT, k_assemble_rows_cT, k_assemble_rows_kT_K and the three table kernels on
anisotropic tags, k_assemble_rows_kT_an, k_assemble_rows_cT_an and k_assemble_rows_kT_K_an), pinned as SHA-256 digests in
tests/golden/rowgather_bits.json.  The file was recorded with scripts/rowgather_bits_record.py: the first seven kernels' entries
from the library of the commit before the five kernels were folded into one body, the *_an entries from the library of the
commit before the coefficient policies were folded into RowsTable and RowsConst<K, AN>; no tolerance anywhere.

Per small case: a seeded state that over- and undershoots the tables' 300..800 K, 1/T conductivity tables and linear capacity
tables on the pressure media (IEEE basic operations only, so the tables are the same numbers on every host), the sample
anisotropic and one pressure medium with equal multipliers 3.
  A, M     plain | multipliers | kappa tables, after one step | both tables, after one step
           | kappa tables and multipliers (set_aniso_tables), after one step | both tables and multipliers, after one step
  load     K u of hold_load() after steady_setup | steady_setup with multipliers | steady_picard_setup with kappa tables
           | steady_picard_setup with kappa tables and multipliers
The mesh arrays are pinned too: if they move, the digests of the operators mean nothing and the failure names the mesher."""
import hashlib
import json
import os

import numpy as np
import pytest

from helpers import material_tables

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "rowgather_bits.json")
CASES = {"geballe_with_diamond": "case_with_diamond_small", "geballe_no_diamond": "case_no_diamond_small"}
MESH_KEYS = ("coords", "tris", "tags")


def _sha(a, dtype):
    return hashlib.sha256(np.ascontiguousarray(a, dtype=dtype).tobytes()).hexdigest()


def _inputs(case):
    cfg, stack, mesh = case
    tk, trc = material_tables(stack, mesh)
    n = len(mesh.coords)
    ins = sorted(t for name, t in mesh.material_tags.items() if name.endswith("ins"))
    T = 300.0 + 10.0 * np.arange(51)
    return {"dt": float(cfg["timing"]["t_final"]) / int(cfg["timing"]["num_steps"]), "tk": tk, "trc": trc,
            "u": 250.0 + 700.0 * np.random.default_rng(20261017).random(n),
            "ktab": {t: (300.0, 10.0, tk[t] * 300.0 / T) for t in ins},
            "ctab": {t: (300.0, 10.0, trc[t] * (0.6 + 0.4 * (T / 800.0))) for t in ins},
            "aniso": {mesh.material_tags["p_sample"]: (2.0, 0.25), ins[0]: (3.0, 3.0)},
            "steady_dofs": np.arange(0, n, 50, dtype=np.int32)}


def _context(hip, mesh, p, aniso=False, ktab=False, ctab=False):
    tags = sorted(p["tk"])
    be = hip.HeatflowHIP(0)
    be.set_mesh(mesh.coords, mesh.tris, mesh.tags)
    be.set_materials(tags, [p["tk"][t] for t in tags], [p["trc"][t] for t in tags])
    if aniso:
        if ktab:
            be.set_aniso_tables(True)
        be.set_anisotropy(p["aniso"])
    if ktab:
        be.set_kappa_tables(p["ktab"])
    if ctab:
        be.set_rhoc_tables(p["ctab"])
    be.set_dirichlet(np.zeros(0, dtype=np.int32))
    be.set_state(p["u"])
    be.assemble(p["dt"], hip.ASM_ROW_GATHER)
    return be


def digests(hip, case):
    """{name: SHA-256} of the mesh arrays and of what each of the ten kernels writes."""
    mesh = case[2]
    p = _inputs(case)
    out = {"coords": _sha(mesh.coords, np.float64), "tris": _sha(mesh.tris, np.int32), "tags": _sha(mesh.tags, np.int32)}
    for name, kw, step in (("plain", {}, False), ("multipliers", {"aniso": True}, False), ("kappa_tables", {"ktab": True}, True),
                           ("both_tables", {"ktab": True, "ctab": True}, True),
                           ("kappa_tables_an", {"aniso": True, "ktab": True}, True),
                           ("both_tables_an", {"aniso": True, "ktab": True, "ctab": True}, True)):
        with _context(hip, mesh, p, **kw) as be:
            if step:                                                           # the step re-values at the state set above
                be.step(np.zeros(0), 1e-10, 0.0, 20000)
            _, _, A, M = be.get_csr()
        out[f"{name}.A"], out[f"{name}.M"] = _sha(A, np.float64), _sha(M, np.float64)
    for name, kw in (("steady", {}), ("steady_multipliers", {"aniso": True}), ("steady_picard", {"ktab": True}),
                     ("steady_picard_an", {"aniso": True, "ktab": True})):
        with _context(hip, mesh, p, **kw) as be:
            if kw.get("ktab"):
                be.steady_picard_setup(p["steady_dofs"])
            else:
                be.steady_setup(p["steady_dofs"])
            be.hold_load()
            out[f"{name}.load"] = _sha(be.get_load(), np.float64)
    return out


@pytest.mark.parametrize("case", sorted(CASES))
def test_every_row_gather_kernel_writes_the_recorded_bits(hip, request, case):
    with open(GOLDEN) as f:
        want = json.load(f)[case]
    got = digests(hip, request.getfixturevalue(CASES[case]))
    assert sorted(got) == sorted(want)
    moved = [k for k in MESH_KEYS if got[k] != want[k]]
    assert not moved, f"the mesher gives other {moved} for {case} than when the fixture was recorded: the kernels were not compared"
    ops = [k for k in got if k.endswith((".A", ".load"))]
    assert len(ops) == 10 and len({got[k] for k in ops}) == 10                # every set-up is a different operator
    assert got["both_tables.M"] != got["plain.M"] and got["both_tables_an.M"] == got["both_tables.M"]   # the multipliers leave rho_c alone
    wrong = [k for k in got if got[k] != want[k]]
    assert not wrong, f"{case}: other bits than recorded in {wrong}"
