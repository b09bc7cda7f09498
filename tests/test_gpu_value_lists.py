"""Value lists of the fine operators (hf_set_value_lists / hf_get_value_lists, k_spmv's VC path): the tables are a lossless,
minimal second encoding of A and M, and every product, field and iteration count with them is bit for bit that of the raw arrays.
No tolerance anywhere: the kernel multiplies the same doubles in the same order, so any difference is a bug.

Meshes: the fixture mesh of tests/golden/with_diamond_tiny.npz (1960 nodes: three full 512-row chunks and a partial one), the
coarse quadtree mesh of the suite (nine materials), a structured lattice below 512 nodes (one chunk), and a jittered
general-triangle lattice of 900 nodes, where hardly a value repeats: mode 1 leaves the raw path there, and under mode 2 its
lists are as long as the chunks and go past what the kernel stages in LDS, which is the branch that reads the list in place."""
import os

import numpy as np
import pytest

from conftest import HEATING_CSV, ROOT, load_cfg
from helpers import make_problem, material_tables

pytestmark = pytest.mark.gpu

RPC = 512


def _lattice(nz, nr, jitter, seed=7):
    from test_gpu_parity import _unit_square_mesh

    rng = np.random.default_rng(seed)
    coords, tris = _unit_square_mesh(nz, nr)
    coords = coords.copy()
    if jitter:
        inner = (coords[:, 0] > 0) & (coords[:, 0] < 1.0e-6) & (coords[:, 1] > 0) & (coords[:, 1] < 2.0e-6)
        coords[inner, 0] += rng.uniform(-0.3, 0.3, inner.sum()) * 1.0e-6 / nz
        coords[inner, 1] += rng.uniform(-0.3, 0.3, inner.sum()) * 2.0e-6 / nr
    tags = rng.integers(1, 5, len(tris)).astype(np.int32)
    if not jitter:
        tags[:] = 1                                        # one material: stencils repeat along z
    tk = {t: float(10.0 ** rng.uniform(0, 3)) for t in range(1, 5)}
    trc = {t: float(10.0 ** rng.uniform(5.5, 7)) for t in range(1, 5)}
    dofs = np.sort(rng.choice(len(coords), size=17, replace=False)).astype(np.int32)
    return {"coords": coords, "tris": tris, "tags": tags, "tk": tk, "trc": trc, "dofs": dofs, "dt": 3e-9}


def _fixture_mesh():
    from heatflow_amd.bc import P1Space, RowDirichletBC
    from heatflow_amd.geometry import build_stack, scale_mesh_sizes
    from heatflow_amd.heating import HeatingCurve

    g = np.load(os.path.join(ROOT, "tests", "golden", "with_diamond_tiny.npz"))
    cfg = scale_mesh_sizes(load_cfg("geballe_with_diamond"), float(g["mesh_scale"]))
    stack = build_stack(cfg)
    mtags = {str(k): int(v) for k, v in zip(g["material_names"], g["material_tag_values"])}
    ic = float(cfg["heating"]["ic_temp"])
    heat = HeatingCurve(HEATING_CSV, ic, float(cfg["heating"]["fwhm"]))
    V = P1Space(g["coords"])
    bcs = [RowDirichletBC(V, "left", value=ic), RowDirichletBC(V, "right", value=ic), RowDirichletBC(V, "top", value=ic),
           RowDirichletBC(V, "x", coord=stack.heated_z, length=abs(stack.r_sample) * 2, center=0.0, value=heat.gaussian)]
    return {"coords": g["coords"], "tris": g["tris"], "tags": g["tags"], "dofs": g["bc_dofs"], "bcs": bcs, "ic": ic,
            "tk": {mtags[m.name]: m.properties["k"] for m in stack.materials},
            "trc": {mtags[m.name]: m.properties["rho_cv"] for m in stack.materials},
            "dt": float(cfg["timing"]["t_final"]) / int(cfg["timing"]["num_steps"])}


def _quadtree_mesh(case):
    cfg, stack, mesh = case
    tk, trc = material_tables(stack, mesh)
    n = len(mesh.coords)
    return {"coords": mesh.coords, "tris": mesh.tris, "tags": mesh.tags, "tk": tk, "trc": trc,
            "dofs": np.arange(0, n, 37, dtype=np.int32), "dt": float(cfg["timing"]["t_final"]) / int(cfg["timing"]["num_steps"])}


@pytest.fixture(scope="module")
def meshes(case_with_diamond_small):
    return {"fixture": _fixture_mesh(), "quadtree": _quadtree_mesh(case_with_diamond_small), "one_chunk": _lattice(15, 20, False),
            "jittered": _lattice(29, 29, True)}


def _context(hip, m, mode, precond=0, mode_asm=None):
    be = hip.HeatflowHIP(0)
    be.set_value_lists(mode)
    be.set_mesh(m["coords"], m["tris"], m["tags"])
    tags = sorted(m["tk"])
    be.set_materials(tags, [m["tk"][t] for t in tags], [m["trc"][t] for t in tags])
    be.set_dirichlet(m["dofs"])
    be.set_precond(precond)
    be.assemble(m["dt"], hip.ASM_ROW_GATHER if mode_asm is None else mode_asm)
    return be


def _check_tables(be, which):
    rowptr, colidx, A, M = be.get_csr()
    vals = (M if which else A).view(np.uint64)
    t = be.get_value_lists(which, arrays=True)
    vptr, vlist, cv = t["vptr"], t["vlist"].view(np.uint64), t["cv"]
    n = len(rowptr) - 1
    assert t["valid"] and len(vptr) == (n + RPC - 1) // RPC + 1 and vptr[0] == 0 and vptr[-1] == t["sum_vlist"] == len(vlist)
    longest = 0
    for c, r0 in enumerate(range(0, n, RPC)):
        k0, k1 = rowptr[r0], rowptr[min(n, r0 + RPC)]
        lst = vlist[vptr[c]:vptr[c + 1]]
        assert np.array_equal(lst, np.unique(vals[k0:k1])), f"chunk {c}: the list is not the sorted set of the chunk's patterns"
        assert np.array_equal(lst[(cv[k0:k1] >> 16).astype(np.int64)], vals[k0:k1]), f"chunk {c}: a value id names another pattern"
        cols = np.unique(colidx[k0:k1])
        assert np.array_equal(cv[k0:k1] & 0xFFFF, np.searchsorted(cols, colidx[k0:k1])), f"chunk {c}: column positions"
        longest = max(longest, len(lst))
    assert t["max_vlist"] == longest
    return t


@pytest.mark.parametrize("name", ["fixture", "quadtree", "one_chunk"])
def test_tables_are_lossless_and_minimal(hip, meshes, name):
    with _context(hip, meshes[name], 1) as be:
        for which in (0, 1):
            t = _check_tables(be, which)
            assert 2 * t["sum_vlist"] <= be.nnz


def test_tables_of_a_mesh_without_repeated_values(hip, meshes):
    """Mode 1 keeps the raw arrays (lists longer than nnz / 2); mode 2 builds lists nearly as long as the chunks, longer than the
    share of LDS the kernel stages them in."""
    m = meshes["jittered"]
    with _context(hip, m, 1, mode_asm=hip.ASM_LDS_COLORED) as be:
        for which in (0, 1):
            t = be.get_value_lists(which)
            assert not t["valid"] and 2 * t["sum_vlist"] > be.nnz
    with _context(hip, m, 2, mode_asm=hip.ASM_LDS_COLORED) as be:
        for which in (0, 1):
            t = _check_tables(be, which)
            assert t["max_vlist"] > t["vcap"]            # the list of some chunk is read in place
            assert 2 * t["sum_vlist"] > be.nnz


@pytest.mark.parametrize("name", ["fixture", "quadtree", "one_chunk", "jittered"])
def test_products_are_bit_identical(hip, meshes, name):
    m = meshes[name]
    x = np.random.default_rng(3).standard_normal(len(m["coords"]))
    x[::7] = 0.0
    asm = hip.ASM_LDS_COLORED if name == "jittered" else None
    out = {}
    for mode in (0, 1, 2):
        with _context(hip, m, mode, mode_asm=asm) as be:
            for which in (0, 1):
                t = be.get_value_lists(which)
                assert t["valid"] == (mode == 2 or (mode == 1 and 2 * t["sum_vlist"] <= be.nnz))
                assert t["valid"] == (mode > 0 and (mode == 2 or name != "jittered"))
            out[mode] = be.spmv(x, 0), be.spmv(x, 1)
    for mode in (1, 2):
        assert np.array_equal(out[mode][0], out[0][0]) and np.array_equal(out[mode][1], out[0][1])
    assert np.abs(out[0][0]).max() > 0.0


def _fixture_run(hip, f, mode, nsteps, **kw):
    from heatflow_amd.solver import HeatProblem

    be = hip.HeatflowHIP(0)
    be.set_value_lists(mode)
    prob = HeatProblem(f["coords"], f["tris"], f["tags"], f["tk"], f["trc"], f["dt"], f["bcs"], f["ic"], backend=be, **kw)
    try:
        assert be.get_value_lists(0)["valid"] == (mode > 0)
        if "load" in f and kw.get("scheme") == "bdf2":
            prob.set_load(f["load"])
        for b in prob.bcs:
            b.update(0.0)
        fields = []
        for k in range(nsteps):
            prob.step((k + 1) * prob.dt, only=[prob.bcs[3]])
            fields.append(prob.state())
        return np.array(fields), list(prob.iters)
    finally:
        be.close()


@pytest.mark.parametrize("precond", [0, 1])
def test_time_loop_is_bit_identical(hip, meshes, precond):
    """Twelve steps on the fixture mesh: right-hand side (mode 0), start residual (2 / 5), Jacobi sweeps (4), residual (3) and
    iteration head (9) all read A or M through the lists."""
    runs = {mode: _fixture_run(hip, meshes["fixture"], mode, 12, precond=precond) for mode in (0, 1, 2)}
    assert runs[0][0][-1].max() > 302.0 and sum(runs[0][1]) > 12
    for mode in (1, 2):
        assert runs[mode][1] == runs[0][1]
        for k in range(12):
            assert np.array_equal(runs[mode][0][k], runs[0][0][k]), f"mode {mode}, step {k}"


def test_bdf2_with_a_load_is_bit_identical(hip, meshes):
    f = dict(meshes["fixture"])
    f["load"] = 1e-6 * (1.0 + np.cos(np.arange(len(f["coords"]))))
    runs = {mode: _fixture_run(hip, f, mode, 5, scheme="bdf2") for mode in (0, 1)}
    assert runs[1][1] == runs[0][1] and np.array_equal(runs[1][0], runs[0][0])
    plain = _fixture_run(hip, meshes["fixture"], 0, 5, scheme="bdf2")
    assert not np.array_equal(plain[0], runs[0][0])       # the load took part


def test_stale_tables_are_never_used(hip, meshes, case_with_diamond_small):
    """Re-valuation between runs, and kappa(T) tables (no lists while they are set): a stale list would reproduce the old operator."""
    cfg, stack, mesh = case_with_diamond_small
    tk, _ = material_tables(stack, mesh)
    sample = mesh.material_tags["p_sample"]
    ins = sorted(t for name, t in mesh.material_tags.items() if name.endswith("ins"))
    T = 300.0 + 10.0 * np.arange(51)
    out = {}
    for mode in (0, 1):
        be = hip.HeatflowHIP(0)
        be.set_value_lists(mode)
        prob = make_problem(cfg, stack, mesh, backend=be, precond=1)
        try:
            for b in prob.bcs:
                b.update(0.0)
            fields = []
            for k in range(3):
                prob.step((k + 20) * prob.dt, only=[prob.bcs[3]])
                fields.append(prob.state())
            be.update_kappa([sample], [3.0 * tk[sample]])
            assert be.get_value_lists(0)["valid"] == (mode > 0)
            for k in range(3, 6):
                prob.step((k + 20) * prob.dt, only=[prob.bcs[3]])
                fields.append(prob.state())
            be.assemble(0.5 * prob.dt, hip.ASM_ROW_GATHER)
            for k in range(6, 8):
                prob.step((k + 20) * prob.dt, only=[prob.bcs[3]])
                fields.append(prob.state())
            out[mode] = np.array(fields), list(prob.iters)
        finally:
            be.close()
        be = hip.HeatflowHIP(0)
        be.set_value_lists(mode)
        prob = make_problem(cfg, stack, mesh, backend=be, kappa_tables={t: (300.0, 10.0, tk[t] * 300.0 / T) for t in ins})
        try:
            assert not be.get_value_lists(0)["valid"] and not be.get_value_lists(1)["valid"]
            for b in prob.bcs:
                b.update(0.0)
            fields = []
            for k in range(4):
                prob.step((k + 20) * prob.dt, only=[prob.bcs[3]])
                fields.append(prob.state())
            out[mode] += (np.array(fields),)
        finally:
            be.close()
    assert out[1][1] == out[0][1]
    assert np.array_equal(out[1][0], out[0][0]) and np.array_equal(out[1][2], out[0][2])
    assert not np.array_equal(out[0][0][3], out[0][0][2]) and out[0][0].max() > 300.5


def test_mode_is_checked(hip, meshes):
    with _context(hip, meshes["one_chunk"], 1) as be:
        with pytest.raises(ValueError):
            be.set_value_lists(3)
        be.set_value_lists(0)
        assert be.get_value_lists(0)["valid"]               # effective from the next assemble
        be.assemble(meshes["one_chunk"]["dt"], hip.ASM_ROW_GATHER)
        assert not be.get_value_lists(0)["valid"]
        with pytest.raises(hip.HipError):
            be.get_value_lists(0, arrays=True)
