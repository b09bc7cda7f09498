"""BDF2 time stepping on the GPU (hf_set_time_scheme): fields at every step against the restatement of tests/bdf2_oracle.py
(both meshes, both preconditioners, every start-vector kind, with and without a load, hf_step and hf_run), the convergence
order, the accuracy at 1.04 M DOF, a held steady state, the batched loop, tangents, switching schemes, and the error returns."""
import copy

import numpy as np
import pytest

from bdf2_oracle import BDF2OracleBackend
from conftest import HEATING_CSV, build_case
from helpers import make_problem

pytestmark = pytest.mark.gpu

FIELD_TOL_K = 1e-4


def _fields_hip_and_oracle(case, precond, kind, load=False, steps=(4, 5, 3)):
    """Fields after every step: `steps[0]` hf_step calls, then two hf_run calls, on the GPU and on the restatement."""
    cfg, stack, mesh = case
    out = []
    for backend in (None, BDF2OracleBackend()):
        prob = make_problem(cfg, stack, mesh, backend=backend, precond=precond, scheme="bdf2")
        try:
            if backend is None:
                prob.backend.set_start_vector(kind)
            if load:
                ob = BDF2OracleBackend()
                make_problem(cfg, stack, mesh, backend=ob, scheme="bdf2")
                rng = np.random.default_rng(1)
                F = (ob.M @ (2.0 + rng.random(prob.n))) / prob.dt           # dt' F ~ 2/3 M (2..3 K): a strong heat source
                prob.set_load(F)
            nodes = np.arange(prob.n, dtype=np.int32)
            fields = []
            for k in range(steps[0]):
                prob.step((k + 1) * prob.dt, [prob.bcs[3]])
                fields.append(prob.state())
            first = steps[0]
            for n in steps[1:]:
                _, s, _ = prob.run(n, watcher_nodes=nodes, time_varying=[prob.bcs[3]], first_step=first)
                fields.extend(s)
                first += n
            out.append(np.array(fields))
        finally:
            prob.close()
    return out


@pytest.mark.parametrize("kind", [0, 1, 2, 3])
@pytest.mark.parametrize("precond", [0, 1])
@pytest.mark.parametrize("case", ["geballe_with_diamond", "geballe_no_diamond"])
def test_bdf2_fields_match_the_restatement_at_every_step(hip, case, precond, kind):
    gpu, ref = _fields_hip_and_oracle(build_case(case, 8.0), precond, kind)
    worst = np.abs(gpu - ref).max()
    assert worst <= FIELD_TOL_K, f"{case} precond={precond} kind={kind}: worst |dT| {worst:.3e} K"
    assert np.abs(ref[-1] - ref[0]).max() > 1.0       # the run really heats


@pytest.mark.parametrize("kind", [1, 3])
@pytest.mark.parametrize("precond", [0, 1])
def test_bdf2_with_a_load_matches_the_restatement(hip, case_with_diamond_small, precond, kind):
    gpu, ref = _fields_hip_and_oracle(case_with_diamond_small, precond, kind, load=True)
    worst = np.abs(gpu - ref).max()
    assert worst <= FIELD_TOL_K, f"precond={precond} kind={kind}: worst |dT| {worst:.3e} K"


def _oside(session, cfg, n, scheme):
    from heatflow_amd.parameter_sweep import build_stack, get_watcher_points

    c = copy.deepcopy(cfg)
    c["timing"]["num_steps"] = int(n)
    c["timing"]["scheme"] = scheme
    res = session.run(c, build_stack(c), get_watcher_points(c))
    return res["watchers"]["oside"], res


def _errors(case, plan, n_ref=1600):
    from heatflow_amd.driver import SimulationSession

    cfg, stack, mesh = case
    s = SimulationSession(mesh.coords, mesh.tris, mesh.tags, mesh.material_tags)
    try:
        ref, _ = _oside(s, cfg, n_ref, "bdf2")
        out = {}
        for scheme, n in plan:
            w, res = _oside(s, cfg, n, scheme)
            out[(scheme, n)] = float(np.max(np.abs(w - ref[n_ref // n - 1::n_ref // n])))
        return out
    finally:
        s.close()


def test_convergence_order_on_the_gpu(hip, case_with_diamond_small):
    e = _errors(case_with_diamond_small, [("bdf2", 100), ("bdf2", 200), ("backward_euler", 100), ("backward_euler", 200)])
    print(e)
    assert e[("bdf2", 100)] / e[("bdf2", 200)] >= 3.0
    assert e[("backward_euler", 100)] / e[("backward_euler", 200)] <= 2.3


def test_accuracy_at_one_million_dof(hip):
    case = build_case("geballe_with_diamond", 0.43)
    assert len(case[2].coords) > 1_000_000
    e = _errors(case, [("backward_euler", 100), ("bdf2", 50), ("bdf2", 100)])
    print(e)
    assert e[("bdf2", 50)] < e[("backward_euler", 100)]
    assert 5.0 * e[("bdf2", 100)] <= e[("backward_euler", 100)]


@pytest.mark.parametrize("precond", [0, 1])
def test_held_steady_state_does_not_drift_under_bdf2(hip, case_with_diamond_small, precond):
    from test_gpu_steady import problem, two_line_steady

    sb = two_line_steady(case_with_diamond_small)
    prob = problem(case_with_diamond_small, sb[:3], precond, scheme="bdf2")
    try:
        u_ss, _, _ = prob.solve_steady(sb)
        prob.hold_load()
        for k in range(10):
            prob.step((k + 1) * prob.dt)
            assert np.abs(prob.state() - u_ss).max() <= 1e-5, k
        _, _, _ = prob.run(5, first_step=10)
        assert np.abs(prob.state() - u_ss).max() <= 1e-5
    finally:
        prob.close()


def _single_bdf2(prob, g_one, ic):
    prob.set_state(ic)
    prob.backend.run(g_one, prob.rtol, 0.0, prob.max_it, None)
    return prob.state()


@pytest.mark.parametrize("precond", [0, 1])
@pytest.mark.parametrize("kind", ["shared", "per_column", "affine"])
def test_batched_bdf2_equals_single_bdf2_runs(hip, case_with_diamond_small, kind, precond):
    from heatflow_amd.heating import HeatingCurve

    cfg, stack, mesh = case_with_diamond_small
    nsteps, nv = 10, 4
    tag_s = mesh.material_tags["p_sample"]
    ic = float(cfg["heating"]["ic_temp"])
    prob = make_problem(cfg, stack, mesh, precond=precond, amg_reuse=True, scheme="bdf2")
    be = prob.backend
    try:
        for bc in prob.bcs:
            bc.update(0.0)
        if kind == "shared":           # columns differ in the heated line's fwhm
            fw = [1.0e-5, 1.2e-5, 1.4e-5, 1.6e-5]
            g_cols = []
            for f in fw:
                prob.bcs[3]._value = HeatingCurve(HEATING_CSV, ic, f).gaussian
                g_cols.append(np.array([prob.bc_values((k + 1) * prob.dt, [prob.bcs[3]]) for k in range(nsteps)]))
            singles = [_single_bdf2(prob, g, ic) for g in g_cols]
            g_all = np.stack(g_cols, axis=2)
            be.batch_begin(nv, per_column_operator=hip.BATCH_SHARED)
        else:
            ks = [3.3 + 0.2 * j for j in range(nv)]
            g_one = np.array([prob.bc_values((k + 1) * prob.dt, [prob.bcs[3]]) for k in range(nsteps)])
            singles = []
            for kap in ks:
                be.update_kappa([tag_s], [kap])
                singles.append(_single_bdf2(prob, g_one, ic))
            g_all = np.repeat(g_one[:, :, None], nv, axis=2)
            if kind == "affine":
                be.update_kappa([tag_s], [ks[nv // 2]])
                be.batch_begin(nv, per_column_operator=hip.BATCH_AFFINE)
                be.batch_set_affine([tag_s], [kap - ks[nv // 2] for kap in ks])
            else:
                be.batch_begin(nv, per_column_operator=hip.BATCH_PER_COLUMN)
                for j, kap in enumerate(ks):
                    be.update_kappa([tag_s], [kap])
                    be.batch_load_column(j)
        for j in range(nv):
            be.batch_set_state(j, np.full(prob.n, ic))
        be.batch_run(g_all[:4], prob.rtol, 0.0, prob.max_it, None)          # two calls: the history continues
        be.batch_run(g_all[4:], prob.rtol, 0.0, prob.max_it, None)
        for j in range(nv):
            d = np.abs(be.batch_get_state(j) - singles[j]).max()
            assert d <= 1e-5, f"{kind} column {j}: {d:.3e} K"
        assert np.abs(singles[0] - singles[-1]).max() > 1e-3
        be.batch_end()
    finally:
        prob.close()


def test_batched_bdf2_with_the_flux_projection(hip, case_no_diamond_small):
    """hf_batch_run_flux in BDF2: every column's state and gradient samples equal a single BDF2 run's."""
    cfg, stack, mesh = case_no_diamond_small
    nsteps, nv = 6, 2
    ic = float(cfg["heating"]["ic_temp"])
    prob = make_problem(cfg, stack, mesh, precond=1, scheme="bdf2")
    be = prob.backend
    try:
        for bc in prob.bcs:
            bc.update(0.0)
        g_one = np.array([prob.bc_values((k + 1) * prob.dt, [prob.bcs[3]]) for k in range(nsteps)])
        be.flux_setup()
        single = _single_bdf2(prob, g_one, ic)
        be.flux_solve(1e-10, 5000, want_z=False, want_r=True)
        fnodes = np.arange(0, prob.n, max(1, prob.n // 40), dtype=np.int32)
        _, gr_single = be.flux_sample(fnodes, want_z=False, want_r=True)
        be.batch_begin(nv, per_column_operator=hip.BATCH_SHARED)
        for j in range(nv):
            be.batch_set_state(j, np.full(prob.n, ic))
        _, _, flux = be.batch_run(np.repeat(g_one[:, :, None], nv, axis=2), prob.rtol, 0.0, prob.max_it, None,
                                  flux_nodes=fnodes, flux_components=2, flux_rtol=1e-10)
        for j in range(nv):
            assert np.abs(be.batch_get_state(j) - single).max() <= 1e-5
            scale = np.abs(gr_single).max()
            assert np.abs(flux[-1, 0, j] - gr_single).max() <= 1e-5 * scale
        be.batch_end()
    finally:
        prob.close()


def test_kappa_sweep_batch_equals_single_runs_under_bdf2(hip, tmp_path):
    from conftest import load_cfg
    from heatflow_amd.fit import DEFAULT_EXP_CSV
    from heatflow_amd.geometry import scale_mesh_sizes
    from heatflow_amd.parameter_sweep import run_kappa_sweep

    cfg = scale_mesh_sizes(load_cfg("geballe_with_diamond"), 8.0)
    cfg["timing"]["scheme"] = "bdf2"
    cfg["timing"]["num_steps"] = 40
    ks = [3.2 + 0.1 * j for j in range(8)]
    exp = DEFAULT_EXP_CSV
    one = run_kappa_sweep(cfg, str(tmp_path / "m"), ks, str(tmp_path / "o1"), exp_csv=exp, batch=1, rebuild_mesh=True)
    eight = run_kappa_sweep(cfg, str(tmp_path / "m"), ks, str(tmp_path / "o8"), exp_csv=exp, batch=8)
    r1 = np.array([r["rmse"] for r in sorted(one, key=lambda r: r["k"])])
    r8 = np.array([r["rmse"] for r in sorted(eight, key=lambda r: r["k"])])
    assert np.all(np.isfinite(r1)) and np.abs(r1 - r8).max() <= 1e-6 * np.abs(r1).max()


@pytest.mark.parametrize("precond", [0, 1])
def test_bdf2_tangents_match_the_restatement_and_finite_differences(hip, case_with_diamond_small, precond):
    from heatflow_amd.heating import HeatingCurve

    cfg, stack, mesh = case_with_diamond_small
    heat = HeatingCurve(HEATING_CSV, float(cfg["heating"]["ic_temp"]), float(cfg["heating"]["fwhm"]))
    nodes = np.arange(0, len(mesh.coords), 97, dtype=np.int32)
    cond = [[mesh.material_tags["p_sample"]], [mesh.material_tags["p_coupler"], mesh.material_tags["o_coupler"]], []]
    bnd = {2: {3: heat.gaussian_dfwhm}}
    out = []
    for backend in (BDF2OracleBackend(), None):
        prob = make_problem(cfg, stack, mesh, backend=backend, precond=precond, rtol=1e-12, scheme="bdf2")
        try:
            _, _, ts1, _, _ = prob.run_tangent(6, nodes, conductivity=cond, boundary=bnd, time_varying=[prob.bcs[3]])
            _, _, ts2, _, _ = prob.run_tangent(6, nodes, conductivity=cond, boundary=bnd, time_varying=[prob.bcs[3]], first_step=6)
            out.append(np.concatenate([ts1, ts2]))
        finally:
            prob.close()
    ref, gpu = out
    for j in range(3):
        scale = np.abs(ref[:, j]).max()
        assert scale > 0 and np.abs(gpu[:, j] - ref[:, j]).max() <= 1e-6 * scale, j
    # central differences of GPU BDF2 runs in the conductivity of p_sample
    tag = mesh.material_tags["p_sample"]
    k0 = float(cfg["mats"]["p_sample"]["k"])
    curves = []
    for sgn in (1, -1):
        c = copy.deepcopy(cfg)
        c["mats"]["p_sample"]["k"] = k0 * (1 + sgn * 1e-3)
        from heatflow_amd.geometry import build_stack

        prob = make_problem(c, build_stack(c), mesh, precond=precond, rtol=1e-12, scheme="bdf2")
        try:
            _, s, _ = prob.run(12, watcher_nodes=nodes, time_varying=[prob.bcs[3]])
            curves.append(s)
        finally:
            prob.close()
    fd = (curves[0] - curves[1]) / (2e-3 * k0)
    assert tag >= 0
    assert np.abs(gpu[:, 0] - fd).max() <= 1e-4 * np.abs(gpu[:, 0]).max()


@pytest.mark.parametrize("precond", [0, 1])
def test_switching_scheme_leaves_no_residue(hip, case_with_diamond_small, precond):
    cfg, stack, mesh = case_with_diamond_small
    nodes = np.arange(0, len(mesh.coords), 53, dtype=np.int32)

    def be_run(prob):
        prob.set_state(float(cfg["heating"]["ic_temp"]))
        _, s, it = prob.run(8, watcher_nodes=nodes, time_varying=[prob.bcs[3]])
        return s, np.asarray(it), prob.state()

    fresh = make_problem(cfg, stack, mesh, precond=precond)
    try:
        want = be_run(fresh)
    finally:
        fresh.close()
    prob = make_problem(cfg, stack, mesh, precond=precond, scheme="bdf2")
    try:
        prob.run(8, watcher_nodes=nodes, time_varying=[prob.bcs[3]])
        prob.backend.set_time_scheme(0)
        prob.backend.assemble(prob.dt, prob.assembly_mode)
        got = be_run(prob)
    finally:
        prob.close()
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[2], want[2])


def test_scheme_errors_come_back_before_any_launch(hip, case_with_diamond_small):
    from heatflow_amd.hip_backend import HF_ERR_ARG, HF_ERR_STATE, HipError

    cfg, stack, mesh = case_with_diamond_small
    prob = make_problem(cfg, stack, mesh, precond=1)
    be = prob.backend
    try:
        with pytest.raises(ValueError, match="unknown scheme"):
            be.set_time_scheme(2)
        assert hip.load_library().hf_set_time_scheme(be._ctx, -1) == HF_ERR_ARG
        be.set_time_scheme(0)                       # the current scheme: nothing changes, still assembled
        prob.step(prob.dt)
        u0 = prob.state()
        be.set_time_scheme(1)
        g = prob.bc_values(prob.dt)
        for call in (lambda: be.step(g), lambda: be.run(g[None, :]), lambda: be.batch_begin(2),
                     lambda: prob.run_tangent(1, [0], conductivity=[[mesh.material_tags["p_sample"]]])):
            with pytest.raises(HipError) as e:
                call()
            assert e.value.code == HF_ERR_STATE
        assert np.array_equal(prob.state(), u0)
        be.assemble(prob.dt, prob.assembly_mode)    # BDF2 now assembled: steps run
        prob.step(2 * prob.dt)
    finally:
        prob.close()
