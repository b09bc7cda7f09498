"""Tangent runs on the GPU (hf_tangent_setup / hf_run_tangent / hf_get_tangent): against the exact recursion restated with
sparse LU (TangentOracleBackend of test_tangent_cpu.py), against finite differences of primal runs, bitwise-unchanged
primal and sweeps, padded columns, error returns, and the fit built on them."""
import copy

import numpy as np
import pytest

from conftest import HEATING_CSV, build_case
from helpers import make_problem
from test_tangent_cpu import TangentOracleBackend

pytestmark = pytest.mark.gpu

NSTEPS = 20


def _columns(mesh, n_par):
    """n_par = 1: p_sample; 3: p_sample, {p_coupler, o_coupler} together, p_ins; 5: those, fwhm, gasket + fwhm."""
    t = mesh.material_tags
    cond = [[t["p_sample"]], [t["p_coupler"], t["o_coupler"]], [t["p_ins"]], [], [t["gasket"]] if "gasket" in t else [t["o_ins"]]]
    return cond[:n_par]


def _tangent_run(prob, mesh, n_par, heat, nodes, nsteps=NSTEPS, first_step=0):
    cond = _columns(mesh, n_par)
    bnd = {3: {3: heat.gaussian_dfwhm}, 4: {3: heat.gaussian_dfwhm}} if n_par == 5 else {}
    return prob.run_tangent(nsteps, nodes, conductivity=cond, boundary=bnd, time_varying=[prob.bcs[3]], first_step=first_step)


def _heat(cfg):
    from heatflow_amd.heating import HeatingCurve

    return HeatingCurve(HEATING_CSV, float(cfg["heating"]["ic_temp"]), float(cfg["heating"]["fwhm"]))


@pytest.mark.parametrize("case", ["geballe_with_diamond", "geballe_no_diamond"])
def test_tangents_match_the_exact_recursion(hip, case):
    cfg, stack, mesh = build_case(case, 8.0)
    heat = _heat(cfg)
    rng = np.random.default_rng(0)
    nodes = np.sort(rng.choice(len(mesh.coords), 12, replace=False)).astype(np.int32)
    for n_par in (1, 3, 5):
        ref = make_problem(cfg, stack, mesh, backend=TangentOracleBackend())
        _, _, ts_ref, _, _ = _tangent_run(ref, mesh, n_par, heat, nodes)
        fields_ref = [ref.tangent(j) for j in range(n_par)]
        for precond in (0, 1):
            prob = make_problem(cfg, stack, mesh, precond=precond)
            try:
                _, _, ts, _, tit = _tangent_run(prob, mesh, n_par, heat, nodes)
                for j in range(n_par):
                    scale = np.max(np.abs(fields_ref[j]))
                    assert scale > 0
                    err_s = np.max(np.abs(ts[:, j] - ts_ref[:, j]))
                    err_f = np.max(np.abs(prob.tangent(j) - fields_ref[j]))
                    assert err_s <= 1e-6 * scale and err_f <= 1e-6 * scale, (case, n_par, precond, j, err_s / scale, err_f / scale)
                assert tit.shape == (NSTEPS, n_par)
                print(f"{case} n_par={n_par} precond={precond}: tangent iterations/step {tit.mean(axis=0)}, primal {np.mean(prob.iters):.1f}")
            finally:
                prob.close()


def _fd_check(cfg, stack, mesh, precond, nsteps, tol):
    heat = _heat(cfg)
    nodes = np.arange(0, len(mesh.coords), max(1, len(mesh.coords) // 50), dtype=np.int32)
    prob = make_problem(cfg, stack, mesh, precond=precond, rtol=1e-12)
    try:
        cond = [[mesh.material_tags["p_sample"]], []]
        _, _, ts, _, tit = prob.run_tangent(nsteps, nodes, conductivity=cond, boundary={1: {3: heat.gaussian_dfwhm}},
                                            time_varying=[prob.bcs[3]])
    finally:
        prob.close()
    k0, f0 = float(cfg["mats"]["p_sample"]["k"]), float(cfg["heating"]["fwhm"])
    for j, (name, base) in enumerate((("k", k0), ("fwhm", f0))):
        runs = []
        for sgn in (1, -1):
            c = copy.deepcopy(cfg)
            if name == "k":
                c["mats"]["p_sample"]["k"] = base * (1 + sgn * 1e-3)
            else:
                c["heating"]["fwhm"] = base * (1 + sgn * 1e-3)
            from heatflow_amd.geometry import build_stack

            p = make_problem(c, build_stack(c), mesh, precond=precond, rtol=1e-12)
            try:
                runs.append(p.run(nsteps, nodes, time_varying=[p.bcs[3]])[1])
            finally:
                p.close()
        fd = (runs[0] - runs[1]) / (2e-3 * base)
        scale = np.max(np.abs(ts[:, j]))
        assert scale > 0
        err = np.max(np.abs(ts[:, j] - fd))
        print(f"n={len(mesh.coords)} {name}: |tangent - FD| / max|s| = {err / scale:.2e}; tangent iterations/step {tit[:, j].mean():.1f}")
        assert err <= tol * scale


def test_tangents_match_finite_differences_of_gpu_runs(hip):
    cfg, stack, mesh = build_case("geballe_with_diamond", 8.0)
    _fd_check(cfg, stack, mesh, 1, NSTEPS, 1e-4)


def check_primal_bitwise(preconds=(0, 1), kinds=(0, 1, 2, 3)):
    """hf_run_tangent's primal samples, iterations and final state against hf_run's, bit for bit."""
    cfg, stack, mesh = build_case("geballe_with_diamond", 8.0)
    nodes = np.arange(0, len(mesh.coords), 97, dtype=np.int32)
    heat = _heat(cfg)
    for precond in preconds:
        for kind in kinds:
            out = []
            for tangent in (False, True):
                prob = make_problem(cfg, stack, mesh, precond=precond)
                try:
                    prob.backend.set_start_vector(kind)
                    if tangent:
                        _, s1, _, it1, _ = _tangent_run(prob, mesh, 3, heat, nodes, 12)
                        _, s2, _, it2, _ = _tangent_run(prob, mesh, 3, heat, nodes, 6, 12)    # continues both
                    else:
                        _, s1, it1 = prob.run(12, nodes, time_varying=[prob.bcs[3]])
                        _, s2, it2 = prob.run(6, nodes, time_varying=[prob.bcs[3]], first_step=12)
                    out.append((s1, it1, s2, it2, prob.state()))
                finally:
                    prob.close()
            for a, b in zip(*out):
                assert np.array_equal(a, b), (precond, kind)


def test_primal_is_bitwise_that_of_hf_run(hip):
    check_primal_bitwise()


@pytest.mark.parametrize("env", [{"HEATFLOW_HOLD_BACK": "0"}, {"HEATFLOW_POLL": "0"}])
def test_primal_is_bitwise_that_of_hf_run_without_hold_back_or_polling(hip, env):
    """The library reads these switches once per process: a fresh child process per setting (multigrid, where they act)."""
    import os
    import subprocess
    import sys

    here = os.path.dirname(os.path.abspath(__file__))
    code = f"import sys; sys.path[:0] = [{here!r}, {os.path.dirname(here)!r}]; import test_gpu_tangent as t; t.check_primal_bitwise((1,))"
    r = subprocess.run([sys.executable, "-c", code], env={**os.environ, **env}, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]


def test_padded_columns_stay_zero_and_a_sweep_is_unchanged(hip):
    cfg, stack, mesh = build_case("geballe_with_diamond", 8.0)
    nodes = np.arange(0, len(mesh.coords), 53, dtype=np.int32)
    prob = make_problem(cfg, stack, mesh, precond=1, amg_reuse=True)
    try:
        be = prob.backend
        g = np.stack([prob.bc_values((k + 1) * prob.dt) for k in range(8)])
        tag = mesh.material_tags["p_sample"]

        def sweep():
            be.set_state(np.full(prob.n, float(cfg["heating"]["ic_temp"])))
            be.batch_begin(4, 2)
            be.batch_set_affine([tag], np.array([-0.2, 0.0, 0.1, 0.3]))
            for j in range(4):
                be.batch_set_state(j, np.full(prob.n, float(cfg["heating"]["ic_temp"])))
            out = be.batch_run(np.repeat(g[:, :, None], 4, axis=2), nodes=nodes)
            state = be.batch_get_state(3)
            be.batch_end()
            return out + (state,)

        before = sweep()
        be.set_state(np.full(prob.n, float(cfg["heating"]["ic_temp"])))
        _, _, ts, _, tit = prob.run_tangent(8, nodes, conductivity=[[tag]], time_varying=[prob.bcs[3]])
        # n_par = 1 is padded to 2 columns: the padding is zero with no iterations
        samples, iters, tsamp, titers = be.run_tangent(g, None, nodes=nodes)
        assert titers.shape == (8, 2) and np.all(titers[:, 1] == 0) and np.all(tsamp[:, 1] == 0)
        assert np.all(be.get_tangent(1) == 0) and np.max(np.abs(be.get_tangent(0))) > 0
        after = sweep()
        for a, b in zip(before, after):
            assert np.array_equal(a, b)
    finally:
        prob.close()


def test_error_returns(hip):
    from heatflow_amd import hip_backend as hb

    cfg, stack, mesh = build_case("geballe_with_diamond", 8.0)
    prob = make_problem(cfg, stack, mesh)
    be = prob.backend
    try:
        lib, ctx = be._lib, be._ctx
        g = np.stack([prob.bc_values((k + 1) * prob.dt) for k in range(2)])
        tab = np.full(be.tab_len, -1, dtype=np.int32)
        pi = hb._pi

        def run():
            return lib.hf_run_tangent(ctx, 2, hb._pd(g), None, 1e-10, 0.0, 1000, 0, None, None, None, None, None)

        assert run() == hb.HF_ERR_STATE                                  # before hf_tangent_setup
        assert lib.hf_get_tangent(ctx, 0, hb._pd(np.zeros(prob.n))) == hb.HF_ERR_STATE
        assert lib.hf_tangent_setup(ctx, 0, pi(tab)) == hb.HF_ERR_ARG
        assert lib.hf_tangent_setup(ctx, 17, pi(tab)) == hb.HF_ERR_ARG
        bad = tab.copy()
        bad[mesh.material_tags["p_sample"]] = 2
        assert lib.hf_tangent_setup(ctx, 2, pi(bad)) == hb.HF_ERR_ARG   # column >= n_par
        ok = tab.copy()
        ok[mesh.material_tags["p_sample"]] = 0
        assert lib.hf_tangent_setup(ctx, 1, pi(ok)) == hb.HF_OK
        assert lib.hf_get_tangent(ctx, 2, hb._pd(np.zeros(prob.n))) == hb.HF_ERR_ARG
        be.batch_begin(2, 0)
        assert run() == hb.HF_ERR_STATE                                  # a batch is open
        assert lib.hf_tangent_setup(ctx, 1, pi(ok)) == hb.HF_ERR_STATE
        be.batch_end()
        be.set_load(np.zeros(prob.n))
        assert run() == hb.HF_ERR_STATE                                  # a load is set
        be.set_load(None)
        assert run() == hb.HF_OK
        be.steady_setup(prob.bc_dofs)
        be.steady_solve(prob.bc_values(0.0))
        assert run() == hb.HF_ERR_STATE                                  # the state is a steady state (depends on kappa)
        assert "hf_steady_solve" in lib.hf_last_error(ctx).decode()
        assert lib.hf_tangent_setup(ctx, 1, pi(ok)) == hb.HF_OK
        assert run() == hb.HF_ERR_STATE                                  # ... also after a new set-up
        be.set_state(np.full(prob.n, 300.0))
        assert run() == hb.HF_OK
        be.assemble(prob.dt, hb.ASM_LDS_COLORED)
        assert run() == hb.HF_ERR_ARG                                    # not a row-gather operator
        assert lib.hf_tangent_setup(ctx, 1, pi(ok)) == hb.HF_ERR_ARG
    finally:
        prob.close()
    # a tag value below the largest that no cell carries: a mesh of two triangles with tags 0 and 2
    be = hb.HeatflowHIP()
    try:
        be.set_mesh(np.array([[0.0, 0.0], [1.0, 0.0], [1.0, 1.0], [0.0, 1.0]]), np.array([[0, 1, 2], [0, 2, 3]]), np.array([0, 2]))
        lib, ctx = be._lib, be._ctx
        assert lib.hf_tangent_setup(ctx, 1, pi(np.array([-1, 0, -1], dtype=np.int32))) == hb.HF_ERR_ARG
        assert "not a cell tag" in lib.hf_last_error(ctx).decode()
    finally:
        be.close()


def test_c3_one_million_dof_kappa_tangent_matches_finite_differences(hip):
    cfg, stack, mesh = build_case("geballe_with_diamond", 0.43)
    assert 0.9e6 < len(mesh.coords) < 1.2e6
    _fd_check(cfg, stack, mesh, 1, 20, 1e-3)


@pytest.fixture(scope="module")
def stock(tmp_path_factory):
    from conftest import load_cfg
    from heatflow_amd.driver import prepare_mesh
    from heatflow_amd.geometry import build_stack

    cfg = load_cfg("geballe_with_diamond")
    folder = str(tmp_path_factory.mktemp("mesh"))
    return cfg, prepare_mesh(cfg, folder, True, build_stack(cfg)), folder


def test_fit_recovers_kappa_from_synthetic_data_on_the_stock_mesh(hip, stock):
    from heatflow_amd.driver import SimulationSession
    from heatflow_amd.fit import fit_parameters, set_params
    from heatflow_amd.parameter_sweep import build_stack, get_watcher_points

    cfg, mesh, folder = stock
    s = SimulationSession(*mesh)
    try:
        c = set_params(cfg, ("p_sample",), [4.07])
        res = s.run(c, build_stack(c), get_watcher_points(c))
        exp = {"time": res["times"], "temp": res["watchers"]["pside"], "oside": res["watchers"]["oside"]}
        out = fit_parameters(cfg, folder, ("p_sample",), exp, x0=[3.8], max_iter=10, session=s)
    finally:
        s.close()
    print(f"synthetic fit: {out['values']} in {out['iterations']} iterations, {out['runs']} runs, {out['seconds']:.2f} s")
    assert abs(out["values"][0] / 4.07 - 1) <= 1e-5


def test_fit_on_the_experiment_agrees_with_the_kappa_sweep(hip, stock, tmp_path):
    from heatflow_amd.fit import fit_parameters
    from heatflow_amd.parameter_sweep import get_k_values, run_kappa_sweep

    cfg, mesh, folder = stock
    ks = get_k_values()
    rows = run_kappa_sweep(cfg, folder, ks, str(tmp_path / "sweep"), exp_csv=HEATING_CSV)
    ok = [r for r in rows if r["status"] == "success"]
    best = min(ok, key=lambda r: r["rmse"])
    if best["k"] in (min(ks), max(ks)):           # the best point on the grid's edge: widen the grid
        ks = get_k_values(k0=best["k"], half_width=1.0)
        rows = run_kappa_sweep(cfg, folder, ks, str(tmp_path / "sweep2"), exp_csv=HEATING_CSV)
        best = min((r for r in rows if r["status"] == "success"), key=lambda r: r["rmse"])
    out = fit_parameters(cfg, folder, ("p_sample",), HEATING_CSV, x0=[float(cfg["mats"]["p_sample"]["k"])], max_iter=20,
                         mesh=mesh)
    print(f"fit {out['values'][0]:.5f} +- {out['stderr'][0]:.5f} rmse {out['rmse']:.6e}; sweep best {best['k']} rmse {best['rmse']:.6e};"
          f" {out['runs']} runs, {out['seconds']:.2f} s")
    assert abs(out["values"][0] - best["k"]) <= 0.02
    assert out["rmse"] <= best["rmse"] + 1e-6
