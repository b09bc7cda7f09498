"""Temperature-dependent conductivities on the GPU (hf_set_kappa_tables): fields at every step against the restatement of
tests/kappa_T_oracle.py (both small meshes, both preconditioners, both schemes, 1 and 3 Picard sweeps, hf_step then hf_run),
the re-valued operator entry by entry, constant tables against the linear path, clearing, the Picard change, 1.04 M DOF,
the error returns and run_simulation end to end."""
import copy
import ctypes
import os

import numpy as np
import pytest
import scipy.sparse as sp

from conftest import build_case, load_cfg
from helpers import csr_values_on_pattern, make_problem
from kappa_T_oracle import BDF2, BE, KappaTOperator, kappa_t_fields, linear_fields, problem_inputs

pytestmark = pytest.mark.gpu

FIELD_TOL_K = 1e-4
STEPS = (4, 8, 8)          # hf_step calls, then two hf_run calls: the heating starts around step 10 of 100


def _ins_tables(stack, mesh, tag_to_k):
    """1/T tables for the pressure media, 300..800 K at 51 knots: the heated run crosses them."""
    tags = [mesh.material_tags[m.name] for m in stack.materials if m.name.endswith("ins")]
    T = 300.0 + 10.0 * np.arange(51)
    return {t: (300.0, 10.0, tag_to_k[t] * 300.0 / T) for t in tags}


def _gpu_fields(case, tables, precond, scheme, picard, steps=STEPS, kind=None):
    cfg, stack, mesh = case
    prob = make_problem(cfg, stack, mesh, precond=precond, scheme=scheme, kappa_tables=tables, picard=picard)
    try:
        if kind is not None:
            prob.backend.set_start_vector(kind)
        nodes = np.arange(prob.n, dtype=np.int32)
        for bc in prob.bcs:                       # every boundary at t = 0, then the heated line per step (as run())
            bc.update(0.0)
        fields, iters = [], []
        for k in range(steps[0]):
            it, _ = prob.step((k + 1) * prob.dt, [prob.bcs[3]])
            fields.append(prob.state())
            iters.append(it)
        first = steps[0]
        for n in steps[1:]:
            _, s, its = prob.run(n, watcher_nodes=nodes, time_varying=[prob.bcs[3]], first_step=first)
            fields.extend(s)
            iters.extend(its)
            first += n
        return np.array(fields), iters
    finally:
        prob.close()


@pytest.mark.parametrize("picard", [1, 3])
@pytest.mark.parametrize("scheme", ["backward_euler", "bdf2"])
@pytest.mark.parametrize("precond", [0, 1])
@pytest.mark.parametrize("case", ["geballe_with_diamond", "geballe_no_diamond"])
def test_fields_match_the_restatement_at_every_step(hip, case, precond, scheme, picard):
    c = build_case(case, 8.0)
    cfg, stack, mesh = c
    nsteps = sum(STEPS)
    tk, trc, dt, dofs, u0, g = problem_inputs(cfg, stack, mesh, nsteps)
    tables = _ins_tables(stack, mesh, tk)
    code = BDF2 if scheme == "bdf2" else BE
    ref, _ = kappa_t_fields(mesh.coords, mesh.tris, mesh.tags, tk, trc, dt, dofs, u0, g, tables, code, picard)
    lin = linear_fields(mesh.coords, mesh.tris, mesh.tags, tk, trc, dt, dofs, u0, g, code)
    gpu, _ = _gpu_fields(c, tables, precond, scheme, picard)
    worst = np.abs(gpu - ref).max()
    assert worst <= FIELD_TOL_K, f"{case} precond={precond} {scheme} p={picard}: worst |dT| {worst:.3e} K"
    assert np.abs(ref[-1] - ref[0]).max() > 100.0                         # the run heats ...
    assert np.abs(ref - lin).max() > 100 * FIELD_TOL_K                    # ... and kappa(T) changes the answer


def test_revalued_operator_is_symmetric_and_matches_the_restatement(hip, case_with_diamond_small):
    cfg, stack, mesh = case_with_diamond_small
    tk, trc, dt, dofs, u0, g = problem_inputs(cfg, stack, mesh, 1)
    tables = _ins_tables(stack, mesh, tk)
    rng = np.random.default_rng(7)
    u_set = 150.0 + 900.0 * rng.random(len(mesh.coords))                  # spans and overshoots 300..800 K on both sides
    u_set[dofs] = g[0]
    prob = make_problem(cfg, stack, mesh, kappa_tables=tables)
    try:
        prob.set_state(u_set)
        prob.backend.step(g[0], 1e-10, 0.0, 20000)
        rowptr, colidx, A, _ = prob.backend.get_csr()
    finally:
        prob.close()
    n = len(mesh.coords)
    S = sp.csr_matrix((A, colidx, rowptr), shape=(n, n))
    assert (S != S.T).nnz == 0                                              # bitwise symmetric
    op = KappaTOperator(mesh.coords, mesh.tris, mesh.tags, tk, trc, dt, tables)
    Ahat, _ = op.eliminated(u_set, dofs)
    ref = csr_values_on_pattern(Ahat, rowptr, colidx)
    rel = np.abs(A - ref) / np.maximum(np.abs(ref), 1e-300)
    rel[ref == 0.0] = np.abs(A[ref == 0.0])
    assert rel.max() <= 1e-13, rel.max()


def _plain_run(case, precond, kind, nsteps):
    cfg, stack, mesh = case
    prob = make_problem(cfg, stack, mesh, precond=precond)
    try:
        prob.backend.set_start_vector(kind)
        _, s, _ = prob.run(nsteps, watcher_nodes=np.arange(0, prob.n, 7, dtype=np.int32), time_varying=[prob.bcs[3]])
        return s, prob.state()
    finally:
        prob.close()


@pytest.mark.parametrize("precond", [0, 1])
def test_constant_tables_reproduce_the_linear_run(hip, case_with_diamond_small, precond):
    cfg, stack, mesh = case_with_diamond_small
    tk, *_ = problem_inputs(cfg, stack, mesh, 1)
    tables = {t: (300.0, 10.0, [tk[t]] * 51) for t in _ins_tables(stack, mesh, tk)}
    s0, u0 = _plain_run(case_with_diamond_small, precond, 1, 20)
    prob = make_problem(cfg, stack, mesh, precond=precond, kappa_tables=tables)
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
    tk, *_ = problem_inputs(cfg, stack, mesh, 1)
    s0, u0 = _plain_run(case_with_diamond_small, precond, 3, 20)
    prob = make_problem(cfg, stack, mesh, precond=precond, kappa_tables=_ins_tables(stack, mesh, tk))
    try:
        prob.run(12, time_varying=[prob.bcs[3]])
        prob.backend.set_kappa_tables({})
        with pytest.raises(hip.HipError):                                 # the assembly is invalid until re-assembled
            prob.backend.step(prob.bc_values(0.0), 1e-10, 0.0, 100)
        prob.backend.set_state(np.full(prob.n, float(cfg["heating"]["ic_temp"])))
        prob.backend.assemble(prob.dt, hip.ASM_ROW_GATHER)
        _, s1, _ = prob.run(20, watcher_nodes=np.arange(0, prob.n, 7, dtype=np.int32), time_varying=[prob.bcs[3]])
        u1 = prob.state()
    finally:
        prob.close()
    assert np.array_equal(s0, s1) and np.array_equal(u0, u1)


def test_picard_change_shrinks_with_more_sweeps(hip, case_with_diamond_small):
    cfg, stack, mesh = case_with_diamond_small
    tk, *_ = problem_inputs(cfg, stack, mesh, 1)
    ch = {}
    for p in (1, 3, 5):
        prob = make_problem(cfg, stack, mesh, kappa_tables=_ins_tables(stack, mesh, tk), picard=p)
        try:
            with pytest.raises(hip.HipError):
                prob.picard_change()                                        # no step yet
            prob.run(20, time_varying=[prob.bcs[3]])
            ch[p] = prob.picard_change()
        finally:
            prob.close()
    print(ch)
    assert ch[1] > ch[3] > ch[5] >= 0.0


def test_one_million_dof_with_multigrid(hip):
    from heatflow_amd.parameter_sweep import get_watcher_points
    from heatflow_amd.solver import nearest_nodes

    cfg, stack, mesh = build_case("geballe_with_diamond", 0.43)
    assert len(mesh.coords) > 1_000_000
    cfg = copy.deepcopy(cfg)
    cfg["timing"]["num_steps"] = 20                                         # 10 steps reach the heating pulse
    nsteps = 10
    tk, trc, dt, dofs, u0, g = problem_inputs(cfg, stack, mesh, nsteps)
    tables = _ins_tables(stack, mesh, tk)
    wp = get_watcher_points(cfg)
    nodes = nearest_nodes(mesh.coords, [v for v in wp.values()] if isinstance(wp, dict) else wp)
    prob = make_problem(cfg, stack, mesh, precond=1, kappa_tables=tables)
    try:
        _, samples, iters = prob.run(nsteps, watcher_nodes=nodes, time_varying=[prob.bcs[3]])
        fallbacks = prob.backend.amg_info()["jacobi_fallbacks"]
    finally:
        prob.close()
    print("PCG iterations per step:", list(int(i) for i in iters))
    assert fallbacks == 0
    ref, _ = kappa_t_fields(mesh.coords, mesh.tris, mesh.tags, tk, trc, dt, dofs, u0, g, tables, BE, 1)
    worst = np.abs(samples - ref[:, nodes]).max()
    assert worst <= FIELD_TOL_K, worst
    assert np.abs(ref[-1, nodes] - ref[0, nodes]).max() > 1.0


def test_error_returns_and_refusals(hip, case_with_diamond_small):
    cfg, stack, mesh = case_with_diamond_small
    tk, *_ = problem_inputs(cfg, stack, mesh, 1)
    tables = _ins_tables(stack, mesh, tk)
    t_ins = sorted(tables)[0]
    prob = make_problem(cfg, stack, mesh, kappa_tables=tables)
    b = prob.backend
    try:
        for bad in ({999: (300.0, 10.0, [1.0, 2.0])},               # not a cell tag
                    {t_ins: (300.0, 10.0, [1.0])},                   # one knot
                    {t_ins: (300.0, 10.0, [1.0] * 257)},             # too many knots
                    {t_ins: (300.0, 0.0, [1.0, 2.0])},               # dT <= 0
                    {t_ins: (300.0, 10.0, [1.0, -2.0])},             # value <= 0
                    {t_ins: (np.nan, 10.0, [1.0, 2.0])}):
            with pytest.raises(ValueError):
                b.set_kappa_tables(bad)
        for p in (0, 9):
            with pytest.raises(ValueError, match="picard"):
                b.set_kappa_tables(tables, picard=p)
        with pytest.raises(ValueError, match="table"):
            b.update_kappa([t_ins], [5.0])
        with pytest.raises(ValueError, match="row-gather"):
            b.assemble(prob.dt, hip.ASM_LDS_COLORED)
        b.assemble(prob.dt, hip.ASM_ROW_GATHER)
        for call in (lambda: b.batch_begin(2), lambda: b.tangent_setup(1, {t_ins: 0}),
                     lambda: b.steady_setup(prob.bc_dofs)):
            with pytest.raises(hip.HipError) as e:
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
        prob.backend.set_kappa_tables(tables)
        prob.backend.assemble(prob.dt, hip.ASM_ROW_GATHER)
        with pytest.raises(hip.HipError) as e:
            prob.backend.run_tangent(np.zeros((1, len(prob.bc_dofs))))
        assert e.value.code == hip.HF_ERR_STATE
        # after an assembly in another mode, tables are refused
        prob.backend.set_kappa_tables({})
        prob.backend.assemble(prob.dt, hip.ASM_LDS_COLORED)
        with pytest.raises(ValueError, match="row-gather"):
            prob.backend.set_kappa_tables(tables)
    finally:
        prob.close()


def test_run_simulation_end_to_end_with_tables(hip, tmp_path):
    import yaml

    from heatflow_amd.geometry import scale_mesh_sizes
    from heatflow_amd.parameter_sweep import get_watcher_points
    from heatflow_amd.run_with_diamond import run_simulation

    cfg = scale_mesh_sizes(load_cfg("geballe_with_diamond_kT"), 8.0)
    cfg["timing"]["num_steps"] = 40
    out = str(tmp_path / "out")
    res = run_simulation(cfg, str(tmp_path / "mesh"), rebuild_mesh=True, output_folder=out, watcher_points=get_watcher_points(cfg),
                         write_xdmf=False, suppress_print=True)
    assert os.path.isfile(os.path.join(out, "watcher_points.csv"))
    with open(os.path.join(out, "used_config.yaml")) as f:
        used = yaml.safe_load(f)
    assert set(used["kappa_tables"]) == {"p_ins", "o_ins", "g_ins", "p_diam", "o_diam"}
    assert used["timing"]["picard_sweeps"] == 1
    base = scale_mesh_sizes(load_cfg("geballe_with_diamond"), 8.0)
    base["timing"]["num_steps"] = 40
    res0 = run_simulation(base, str(tmp_path / "mesh"), output_folder=str(tmp_path / "out0"), watcher_points=get_watcher_points(base),
                          write_xdmf=False, suppress_print=True)
    w, w0 = res["watchers"], res0["watchers"]
    assert np.abs(np.asarray(w["oside"]) - np.asarray(w0["oside"])).max() > 1e-3
