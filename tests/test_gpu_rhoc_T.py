"""Temperature-dependent heat capacities on the GPU (hf_set_rhoc_tables): fields at every step against the restatement of
tests/rhoc_T_oracle.py (both small meshes, both preconditioners, both schemes, 1 and 3 Picard sweeps, hf_step then hf_run,
capacity tables alone and with conductivity tables), the re-valued M and A entry by entry, constant tables against the path
without tables, clearing, the Picard change, the error returns, run_simulation end to end and 1.04 M DOF."""
import copy
import ctypes
import os

import numpy as np
import pytest
import scipy.sparse as sp

from conftest import build_case, load_cfg
from helpers import csr_values_on_pattern, make_problem
from kappa_T_oracle import linear_fields, problem_inputs
from rhoc_T_oracle import BDF2, BE, einstein_tables, operators, rhoc_t_fields
from test_gpu_kappa_T import FIELD_TOL_K, STEPS, _ins_tables, _plain_run

pytestmark = pytest.mark.gpu


def _cv_tables(stack, mesh, tag_to_rc):
    """Einstein tables (theta = 600 K) for the pressure media, 300..800 K at 51 knots: the heated run crosses them."""
    return einstein_tables(tag_to_rc, [mesh.material_tags[m.name] for m in stack.materials if m.name.endswith("ins")])


def _gpu_fields(case, precond, scheme, picard, steps=STEPS, **tables):
    cfg, stack, mesh = case
    prob = make_problem(cfg, stack, mesh, precond=precond, scheme=scheme, picard=picard, **tables)
    try:
        nodes = np.arange(prob.n, dtype=np.int32)
        for bc in prob.bcs:                       # every boundary at t = 0, then the heated line per step (as run())
            bc.update(0.0)
        fields, changes = [], []
        for k in range(steps[0]):
            prob.step((k + 1) * prob.dt, [prob.bcs[3]])
            fields.append(prob.state())
            changes.append(prob.picard_change())
        first = steps[0]
        for n in steps[1:]:
            _, s, _ = prob.run(n, watcher_nodes=nodes, time_varying=[prob.bcs[3]], first_step=first)
            fields.extend(s)
            changes.extend([np.nan] * (n - 1) + [prob.picard_change()])      # hf_run keeps the change of its last step
            first += n
        return np.array(fields), np.array(changes)
    finally:
        prob.close()


@pytest.mark.parametrize("kinds", ["capacity", "both"])
@pytest.mark.parametrize("picard", [1, 3])
@pytest.mark.parametrize("scheme", ["backward_euler", "bdf2"])
@pytest.mark.parametrize("precond", [0, 1])
@pytest.mark.parametrize("case", ["geballe_with_diamond", "geballe_no_diamond"])
def test_fields_match_the_restatement_at_every_step(hip, case, precond, scheme, picard, kinds):
    c = build_case(case, 8.0)
    cfg, stack, mesh = c
    nsteps = sum(STEPS)
    tk, trc, dt, dofs, u0, g = problem_inputs(cfg, stack, mesh, nsteps)
    ct = _cv_tables(stack, mesh, trc)
    kt = _ins_tables(stack, mesh, tk) if kinds == "both" else {}
    code = BDF2 if scheme == "bdf2" else BE
    ref, ref_ch = rhoc_t_fields(mesh.coords, mesh.tris, mesh.tags, tk, trc, dt, dofs, u0, g, ct, kt, code, picard)
    lin = linear_fields(mesh.coords, mesh.tris, mesh.tags, tk, trc, dt, dofs, u0, g, code)
    gpu, ch = _gpu_fields(c, precond, scheme, picard, rhoc_tables=ct, **({"kappa_tables": kt} if kt else {}))
    worst = np.abs(gpu - ref).max()
    moved = np.abs(ref - lin).max()
    print(f"{case} precond={precond} {scheme} p={picard} {kinds}: worst |dT| {worst:.3e} K, tables move the field by {moved:.4g} K")
    assert worst <= FIELD_TOL_K, f"{case} precond={precond} {scheme} p={picard} {kinds}: worst |dT| {worst:.3e} K"
    assert np.abs(ref[-1] - ref[0]).max() > 100.0                         # the run heats ...
    assert moved > 100 * FIELD_TOL_K                                      # ... and the tables change the answer
    # hf_get_picard_change against the restatement: a difference of two states, the later one within FIELD_TOL_K of the
    # restatement's and the earlier one within 3 FIELD_TOL_K (BDF2's 2 u^n - u^{n-1} of two such fields at worst)
    have = np.isfinite(ch)
    assert have.sum() == STEPS[0] + len(STEPS) - 1
    assert np.abs(ch[have] - ref_ch[have]).max() <= 4 * FIELD_TOL_K, (ch[have], ref_ch[have])


@pytest.mark.parametrize("kinds", ["capacity", "both"])
def test_revalued_M_and_A_are_symmetric_and_match_the_restatement(hip, case_with_diamond_small, kinds):
    """M and A after a re-valuation at a random state, entry by entry against the restatement.

    capacity: relative to each entry, 1e-13, for M and for A (measured on the MI355X: M 4.7e-16, A 3.2e-15).
    both: M the same (measured 4.7e-16).  With kappa(T) as well, this state has entries of A = M + dt' K whose two summands
    cancel: the worst is A_ij = -6.4e-16 from summands of 4.5e-13, 705 : 1 (under capacity tables alone the worst is 32 : 1).
    One rounding of the summands (2.2e-16) is then 1.6e-13 of the entry, so no double-precision evaluation that differs from
    the restatement's by a rounding can meet 1e-13 of the entry there; measured 1.30e-13 at that entry, i.e. 1.8e-16 of its
    summands.  For this case A is therefore held to 1e-13 of |M_ij| + dt' |K_ij| (the entry-relative figure is printed),
    and to 1e-13 of the entry wherever the summands cancel by less than 100 : 1."""
    from oracle import heat_oracle as ho

    cfg, stack, mesh = case_with_diamond_small
    tk, trc, dt, dofs, u0, g = problem_inputs(cfg, stack, mesh, 1)
    ct = _cv_tables(stack, mesh, trc)
    kt = _ins_tables(stack, mesh, tk) if kinds == "both" else {}
    rng = np.random.default_rng(7)
    u_set = 150.0 + 900.0 * rng.random(len(mesh.coords))                  # spans and overshoots 300..800 K on both sides
    u_set[dofs] = g[0]
    prob = make_problem(cfg, stack, mesh, rhoc_tables=ct, **({"kappa_tables": kt} if kt else {}))
    try:
        prob.set_state(u_set)
        prob.backend.step(g[0], 1e-10, 0.0, 20000)                         # one sweep: M and A valued at u_set
        rowptr, colidx, A, M = prob.backend.get_csr()
    finally:
        prob.close()
    n = len(mesh.coords)
    M_ref, A_ref = operators(mesh.coords, mesh.tris, mesh.tags, tk, trc, dt, u_set, kt, ct)
    worst = {}
    for name, vals, ref_mat in (("A", A, ho.eliminate_dirichlet(A_ref, dofs)), ("M", M, M_ref)):
        S = sp.csr_matrix((vals, colidx, rowptr), shape=(n, n))
        assert (S != S.T).nnz == 0, name                                    # bitwise symmetric
        ref = csr_values_on_pattern(ref_mat, rowptr, colidx)
        rel = np.abs(vals - ref) / np.maximum(np.abs(ref), 1e-300)
        rel[ref == 0.0] = np.abs(vals[ref == 0.0])
        worst[name] = rel
        print(name, "worst difference relative to the entry", rel.max())
    assert worst["M"].max() <= 1e-13, worst["M"].max()
    if kinds == "capacity":
        assert worst["A"].max() <= 1e-13, worst["A"].max()
    # |M_ij| + dt' |K_ij| from the same element matrices (the free block: eliminated rows and columns hold 0 and 1)
    from kappa_T_oracle import element_kappa

    coords, tris = np.asarray(mesh.coords, dtype=np.float64), np.asarray(mesh.tris, dtype=np.int64)
    Me, Ke = ho.element_matrices(coords, tris, element_kappa(u_set, tris, mesh.tags, trc, ct),
                                 element_kappa(u_set, tris, mesh.tags, tk, kt))
    mag = csr_values_on_pattern(ho.assemble_csr(n, tris, np.abs(Me) + dt * np.abs(Ke)), rowptr, colidx)
    ref = csr_values_on_pattern(ho.eliminate_dirichlet(A_ref, dofs), rowptr, colidx)
    mag = np.maximum(mag, np.abs(ref))
    print("A: worst difference relative to the summands", (np.abs(A - ref) / mag).max(), "worst cancellation",
          (mag[ref != 0.0] / np.abs(ref[ref != 0.0])).max())
    assert (np.abs(A - ref) / mag).max() <= 1e-13
    mild = mag < 100.0 * np.abs(ref)
    assert worst["A"][mild].max() <= 1e-13
    # the capacity tables are in M: entries inside the pressure media move by a good part of the Einstein factor (1.32 at 800 K)
    M_lin, _ = operators(mesh.coords, mesh.tris, mesh.tags, tk, trc, dt, u_set)
    lin = csr_values_on_pattern(M_lin, rowptr, colidx)
    assert (np.abs(M - lin) / np.abs(lin)).max() > 0.1


def _const_tables(stack, mesh, trc):
    return {t: (300.0, 10.0, [trc[t]] * 51) for t in _cv_tables(stack, mesh, trc)}


def test_constant_capacity_tables_give_the_operators_of_hf_assemble_bitwise(hip, case_with_diamond_small):
    cfg, stack, mesh = case_with_diamond_small
    _, trc, *_ = problem_inputs(cfg, stack, mesh, 1)
    plain = make_problem(cfg, stack, mesh)
    try:
        _, _, A0, M0 = plain.backend.get_csr()
    finally:
        plain.close()
    prob = make_problem(cfg, stack, mesh, rhoc_tables=_const_tables(stack, mesh, trc))
    try:
        _, _, A1, M1 = prob.backend.get_csr()                               # hf_assemble's re-valuation at u0
        prob.run(3, time_varying=[prob.bcs[3]])
        _, _, A2, M2 = prob.backend.get_csr()                               # and a step's
    finally:
        prob.close()
    assert np.array_equal(M0, M1) and np.array_equal(A0, A1)
    assert np.array_equal(M0, M2) and np.array_equal(A0, A2)


@pytest.mark.parametrize("precond", [0, 1])
def test_constant_capacity_tables_reproduce_the_linear_run(hip, case_with_diamond_small, precond):
    cfg, stack, mesh = case_with_diamond_small
    _, trc, *_ = problem_inputs(cfg, stack, mesh, 1)
    s0, u0 = _plain_run(case_with_diamond_small, precond, 1, 20)
    prob = make_problem(cfg, stack, mesh, precond=precond, rhoc_tables=_const_tables(stack, mesh, trc))
    try:
        _, s1, _ = prob.run(20, watcher_nodes=np.arange(0, prob.n, 7, dtype=np.int32), time_varying=[prob.bcs[3]])
        u1 = prob.state()
    finally:
        prob.close()
    if precond == 0:
        assert np.array_equal(s0, s1) and np.array_equal(u0, u1)
    else:
        assert np.abs(s0 - s1).max() <= 1e-5 and np.abs(u0 - u1).max() <= 1e-5


@pytest.mark.parametrize("precond", [0, 1])
def test_clearing_the_tables_restores_the_linear_path(hip, case_with_diamond_small, precond):
    cfg, stack, mesh = case_with_diamond_small
    tk, trc, *_ = problem_inputs(cfg, stack, mesh, 1)
    s0, u0 = _plain_run(case_with_diamond_small, precond, 3, 20)
    prob = make_problem(cfg, stack, mesh, precond=precond, rhoc_tables=_cv_tables(stack, mesh, trc),
                        kappa_tables=_ins_tables(stack, mesh, tk))
    try:
        prob.run(12, time_varying=[prob.bcs[3]])
        prob.backend.set_kappa_tables({})                                   # capacity tables stay: still the nonlinear loop
        prob.backend.set_state(np.full(prob.n, float(cfg["heating"]["ic_temp"])))
        prob.backend.assemble(prob.dt, hip.ASM_ROW_GATHER)
        prob.run(12, time_varying=[prob.bcs[3]])
        assert prob.picard_change() > 0.0
        prob.backend.set_rhoc_tables({})
        with pytest.raises(hip.HipError):                                 # the assembly is invalid until re-assembled
            prob.backend.step(prob.bc_values(0.0), 1e-10, 0.0, 100)
        prob.backend.set_state(np.full(prob.n, float(cfg["heating"]["ic_temp"])))
        prob.backend.assemble(prob.dt, hip.ASM_ROW_GATHER)
        _, s1, _ = prob.run(20, watcher_nodes=np.arange(0, prob.n, 7, dtype=np.int32), time_varying=[prob.bcs[3]])
        u1 = prob.state()
        with pytest.raises(hip.HipError):                                 # no tables: no Picard change, no Picard count
            prob.picard_change()
        with pytest.raises(hip.HipError):
            prob.backend.set_picard(2)
    finally:
        prob.close()
    assert np.array_equal(s0, s1) and np.array_equal(u0, u1)


def test_error_returns_and_refusals(hip, case_with_diamond_small):
    cfg, stack, mesh = case_with_diamond_small
    _, trc, *_ = problem_inputs(cfg, stack, mesh, 1)
    tables = _cv_tables(stack, mesh, trc)
    t_ins = sorted(tables)[0]
    prob = make_problem(cfg, stack, mesh, rhoc_tables=tables)           # capacity tables only
    b = prob.backend
    try:
        for bad in ({999: (300.0, 10.0, [1.0, 2.0])},               # not a cell tag
                    {t_ins: (300.0, 10.0, [1.0])},                   # one knot
                    {t_ins: (300.0, 10.0, [1.0] * 257)},             # too many knots
                    {t_ins: (300.0, 0.0, [1.0, 2.0])},               # dT <= 0
                    {t_ins: (300.0, 10.0, [1.0, -2.0])},             # value <= 0
                    {t_ins: (np.nan, 10.0, [1.0, 2.0])}):
            with pytest.raises(ValueError, match="hf_set_rhoc_tables"):
                b.set_rhoc_tables(bad)
        for p in (0, 9):
            with pytest.raises(ValueError, match="hf_set_picard"):
                b.set_picard(p)
        b.update_kappa([t_ins], [5.0])                               # no conductivity table on the tag: allowed
        with pytest.raises(ValueError, match="row-gather"):
            b.assemble(prob.dt, hip.ASM_LDS_COLORED)
        b.assemble(prob.dt, hip.ASM_ROW_GATHER)
        for call in (lambda: b.batch_begin(2), lambda: b.tangent_setup(1, {t_ins: 0}),
                     lambda: b.steady_setup(prob.bc_dofs)):
            with pytest.raises(hip.HipError, match=r"rho_c\(T\) tables are set") as e:
                call()
            assert e.value.code == hip.HF_ERR_STATE
        g = np.zeros(4)
        assert b._lib.hf_steady_solve(b._ctx, g.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), 0, 1e-10, 0.0, 100, None,
                                      None) == hip.HF_ERR_STATE
        b.set_load(np.zeros(prob.n))                                # a load keeps working
        prob.step(prob.dt, [prob.bcs[3]])
        b.set_load(None)
    finally:
        prob.close()
    # a tangent set up before the tables is refused at run time
    prob = make_problem(cfg, stack, mesh)
    try:
        prob.backend.tangent_setup(1, {t_ins: 0})
        prob.backend.set_rhoc_tables(tables)
        prob.backend.assemble(prob.dt, hip.ASM_ROW_GATHER)
        with pytest.raises(hip.HipError) as e:
            prob.backend.run_tangent(np.zeros((1, len(prob.bc_dofs))))
        assert e.value.code == hip.HF_ERR_STATE
        # after an assembly in another mode, tables are refused
        prob.backend.set_rhoc_tables({})
        prob.backend.assemble(prob.dt, hip.ASM_LDS_COLORED)
        with pytest.raises(ValueError, match="row-gather"):
            prob.backend.set_rhoc_tables(tables)
    finally:
        prob.close()


def test_run_simulation_end_to_end_with_tables(hip, tmp_path):
    import yaml

    from heatflow_amd.geometry import build_stack, scale_mesh_sizes
    from heatflow_amd.driver import prepare_mesh
    from heatflow_amd.parameter_sweep import get_watcher_points
    from heatflow_amd.run_with_diamond import run_simulation
    from heatflow_amd.solver import nearest_nodes

    cfg = scale_mesh_sizes(load_cfg("geballe_with_diamond_cvT"), 8.0)
    cfg["timing"]["num_steps"] = 40
    out = str(tmp_path / "out")
    wp = get_watcher_points(cfg)
    res = run_simulation(cfg, str(tmp_path / "mesh"), rebuild_mesh=True, output_folder=out, watcher_points=wp,
                         write_xdmf=False, suppress_print=True)
    assert os.path.isfile(os.path.join(out, "watcher_points.csv"))
    with open(os.path.join(out, "used_config.yaml")) as f:
        used = yaml.safe_load(f)
    assert set(used["rhoc_tables"]) == set(used["kappa_tables"]) == {"p_ins", "o_ins", "g_ins"}
    assert used["timing"]["picard_sweeps"] == 2
    # the watcher curves against the restatement on the mesh the run wrote
    stack = build_stack(cfg)
    coords, tris, tags, material_tags = prepare_mesh(cfg, str(tmp_path / "mesh"), False, stack)

    class _M:
        pass
    mesh = _M()
    mesh.coords, mesh.tris, mesh.tags, mesh.material_tags = coords, tris, tags, material_tags
    tk, trc, dt, dofs, u0, g = problem_inputs(cfg, stack, mesh, 40)
    kt = {material_tags[m.name]: m.properties["k_table"] for m in stack.materials if "k_table" in m.properties}
    ct = {material_tags[m.name]: m.properties["rho_cv_table"] for m in stack.materials if "rho_cv_table" in m.properties}
    ref, _ = rhoc_t_fields(coords, tris, tags, tk, trc, dt, dofs, u0, g, ct, kt, BE, 2)
    lin = linear_fields(coords, tris, tags, tk, trc, dt, dofs, u0, g)
    names = list(wp) if isinstance(wp, dict) else None
    nodes = nearest_nodes(coords, [wp[k] for k in names] if names else wp)
    for j, name in enumerate(names or sorted(res["watchers"])):
        w = np.asarray(res["watchers"][name])
        print(name, "worst |dT|", np.abs(w - ref[:, nodes[j]]).max(), "tables move it by", np.abs(ref[:, nodes[j]] - lin[:, nodes[j]]).max())
        assert np.abs(w - ref[:, nodes[j]]).max() <= FIELD_TOL_K, name
    assert np.abs(ref[:, nodes] - lin[:, nodes]).max() > 100 * FIELD_TOL_K


def test_one_million_dof_with_multigrid(hip):
    from heatflow_amd.parameter_sweep import get_watcher_points
    from heatflow_amd.solver import nearest_nodes

    cfg, stack, mesh = build_case("geballe_with_diamond", 0.43)
    assert len(mesh.coords) > 1_000_000
    cfg = copy.deepcopy(cfg)
    cfg["timing"]["num_steps"] = 20                                         # 10 steps reach the heating pulse
    nsteps = 10
    tk, trc, *_ = problem_inputs(cfg, stack, mesh, 1)
    wp = get_watcher_points(cfg)
    nodes = nearest_nodes(mesh.coords, [v for v in wp.values()] if isinstance(wp, dict) else wp)
    runs = {}
    for name, kw in (("plain", {}), ("tables", {"rhoc_tables": _cv_tables(stack, mesh, trc), "kappa_tables": _ins_tables(stack, mesh, tk)})):
        prob = make_problem(cfg, stack, mesh, precond=1, **kw)
        try:
            _, samples, iters = prob.run(nsteps, watcher_nodes=nodes, time_varying=[prob.bcs[3]])   # raises unless every step converges
            fallbacks = prob.backend.amg_info()["jacobi_fallbacks"]
        finally:
            prob.close()
        print(name, "PCG iterations per step:", list(int(i) for i in iters))
        assert fallbacks == 0
        assert np.all(np.isfinite(samples))
        runs[name] = samples
    assert np.abs(runs["tables"][-1] - runs["tables"][0]).max() > 1.0
    assert np.abs(runs["tables"] - runs["plain"]).max() > 100 * FIELD_TOL_K
