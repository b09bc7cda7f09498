"""The opt-in BDF2 time scheme without a GPU: the restatement's convergence order, the host layers (HeatProblem, Session.run,
run_batch, tangent runs, the fit) on a scipy backend in BDF2 mode against the restatement, the config key and CLI flags, and
the C ABI entry point hf_set_time_scheme."""
import copy
import os

import numpy as np
import pytest
import yaml

from bdf2_oracle import BDF2, BE, BDF2OracleBackend, reference_run
from conftest import build_case, load_cfg
from test_cabi import _declared_symbols


@pytest.fixture(scope="module")
def small():
    cfg, stack, mesh = build_case("geballe_with_diamond", 8.0)
    cfg = copy.deepcopy(cfg)
    cfg["timing"]["num_steps"] = 30
    return cfg, stack, mesh


def _bdf2(cfg):
    c = copy.deepcopy(cfg)
    c["timing"]["scheme"] = "bdf2"
    return c


def _nodes(cfg, mesh):
    from heatflow_amd.driver import _parse_watchers
    from heatflow_amd.parameter_sweep import get_watcher_points
    from heatflow_amd.solver import nearest_nodes

    names, pts = _parse_watchers(get_watcher_points(cfg))
    return names, nearest_nodes(mesh.coords, pts)


def _session(mesh, backend=None):
    from heatflow_amd.driver import SimulationSession

    return SimulationSession(mesh.coords, mesh.tris, mesh.tags, mesh.material_tags, backend=backend or BDF2OracleBackend())


def test_set_time_scheme_is_declared_exported_and_bound():
    from heatflow_amd import hip_backend

    assert "hf_set_time_scheme" in _declared_symbols()
    assert "hf_set_time_scheme" in hip_backend.EXPORTS
    assert hasattr(hip_backend.load_library(), "hf_set_time_scheme")
    assert (hip_backend.TIME_BACKWARD_EULER, hip_backend.TIME_BDF2) == (0, 1)
    assert hip_backend.time_scheme_code("bdf2") == 1 and hip_backend.time_scheme_code("backward_euler") == 0
    with pytest.raises(ValueError):
        hip_backend.time_scheme_code("crank_nicolson")


def test_restatement_converges_at_second_order(case_with_diamond_small):
    """o-side watcher error against 1600-step BDF2 on the real heating curve: per halving of dt BDF2 gains >= 3x, backward
    Euler <= 2.3x (measured 3.50 and 1.91)."""
    cfg, stack, mesh = case_with_diamond_small
    names, nodes = _nodes(cfg, mesh)
    o = names.index("oside")
    ref = reference_run(cfg, mesh, 1600, watcher_nodes=nodes)["watchers"][:, o]

    def err(n, scheme):
        w = reference_run(cfg, mesh, n, watcher_nodes=nodes, scheme=scheme)["watchers"][:, o]
        return np.max(np.abs(w - ref[1600 // n - 1::1600 // n]))

    e_bdf = [err(100, BDF2), err(200, BDF2)]
    e_be = [err(100, BE), err(200, BE)]
    assert e_bdf[0] / e_bdf[1] >= 3.0, e_bdf
    assert e_be[0] / e_be[1] <= 2.3, e_be
    assert e_bdf[0] < e_be[1]          # BDF2 at 100 steps beats backward Euler at 200


def test_heat_problem_matches_the_restatement_across_two_runs(small):
    from helpers import make_problem

    cfg, stack, mesh = small
    names, nodes = _nodes(cfg, mesh)
    ref = reference_run(cfg, mesh, 30, watcher_nodes=nodes, keep_fields=True)
    be = BDF2OracleBackend()
    prob = make_problem(cfg, stack, mesh, backend=be, scheme="bdf2")
    assert be.scheme == BDF2
    _, s1, _ = prob.run(12, watcher_nodes=nodes)
    _, s2, _ = prob.run(18, watcher_nodes=nodes, first_step=12)     # continues with the true u^{n-1}
    np.testing.assert_allclose(np.vstack([s1, s2]), ref["watchers"], rtol=0, atol=1e-9)
    np.testing.assert_allclose(prob.state(), ref["fields"][-1], rtol=0, atol=1e-9)
    # backward Euler stays the default and makes no scheme call
    be2 = BDF2OracleBackend()
    make_problem(cfg, stack, mesh, backend=be2)
    assert getattr(be2, "set_time_scheme_calls", 0) == 0
    with pytest.raises(ValueError):
        make_problem(cfg, stack, mesh, backend=BDF2OracleBackend(), scheme="bdf3")


def test_session_run_and_run_batch_match_the_restatement(small):
    from heatflow_amd.parameter_sweep import build_stack, get_watcher_points

    cfg, stack, mesh = small
    c = _bdf2(cfg)
    names, nodes = _nodes(c, mesh)
    s = _session(mesh)
    try:
        res = s.run(c, build_stack(c), get_watcher_points(c))
        ref = reference_run(cfg, mesh, 30, watcher_nodes=nodes)["watchers"]
        for q, nm in enumerate(names):
            np.testing.assert_allclose(res["watchers"][nm], ref[:, q], rtol=0, atol=1e-9)
        cfgs = []
        for k in (3.6, 4.4):
            ck = copy.deepcopy(c)
            ck["mats"]["p_sample"]["k"] = k
            cfgs.append(ck)
        batch = s.run_batch(cfgs, [build_stack(ck) for ck in cfgs], get_watcher_points(c))
        for ck, rb in zip(cfgs, batch):
            single = s.run(ck, build_stack(ck), get_watcher_points(ck))
            for nm in names:
                np.testing.assert_allclose(rb["watchers"][nm], single["watchers"][nm], rtol=0, atol=1e-9)
        with pytest.raises(ValueError):        # one scheme per batch
            s.run_batch([cfgs[0], cfg], [build_stack(cfgs[0]), build_stack(cfg)], get_watcher_points(c))
    finally:
        s.close()


def test_session_never_shares_a_problem_between_schemes(small):
    from heatflow_amd.parameter_sweep import build_stack, get_watcher_points

    cfg, stack, mesh = small
    be = BDF2OracleBackend()
    s = _session(mesh, be)
    try:
        r_be = s.run(cfg, stack, get_watcher_points(cfg))
        assert be.scheme == BE and getattr(be, "set_time_scheme_calls", 0) == 0
        r_bdf = s.run(_bdf2(cfg), stack, get_watcher_points(cfg))
        assert be.scheme == BDF2 and be.set_mesh_calls == 2        # a new problem, not the backward-Euler one
        assert np.max(np.abs(r_be["watchers"]["oside"] - r_bdf["watchers"]["oside"])) > 1e-3
        bad = copy.deepcopy(cfg)
        bad["timing"]["scheme"] = "rk4"
        with pytest.raises(ValueError):
            s.run(bad, build_stack(bad), get_watcher_points(bad))
    finally:
        s.close()


def test_bdf2_tangents_match_finite_differences_of_bdf2_runs(small):
    from heatflow_amd.parameter_sweep import build_stack, get_watcher_points

    cfg, stack, mesh = small
    c = _bdf2(cfg)
    s = _session(mesh)
    try:
        res = s.run(c, stack, get_watcher_points(c), tangents=("p_sample", "fwhm"))
        for name in ("p_sample", "fwhm"):
            base = float(c["heating"]["fwhm"]) if name == "fwhm" else float(c["mats"][name]["k"])
            curves = []
            for sgn in (1, -1):
                cc = copy.deepcopy(c)
                if name == "fwhm":
                    cc["heating"]["fwhm"] = base * (1 + sgn * 1e-4)
                else:
                    cc["mats"][name]["k"] = base * (1 + sgn * 1e-4)
                curves.append(s.run(cc, build_stack(cc), get_watcher_points(cc))["watchers"]["oside"])
            fd = (curves[0] - curves[1]) / (2e-4 * base)
            tan = res["tangents"][name]["oside"]
            assert np.max(np.abs(tan)) > 0
            assert np.max(np.abs(tan - fd)) <= 1e-4 * np.max(np.abs(tan))
    finally:
        s.close()


def test_fit_on_bdf2_recovers_kappa_of_bdf2_data(small):
    from heatflow_amd.fit import fit_parameters
    from heatflow_amd.parameter_sweep import build_stack, get_watcher_points

    cfg, stack, mesh = small
    c = _bdf2(cfg)
    c["mats"]["p_sample"]["k"] = 4.07
    s = _session(mesh)
    try:
        res = s.run(c, build_stack(c), get_watcher_points(c))
    finally:
        s.close()
    exp = {"time": res["times"], "temp": res["watchers"]["pside"], "oside": res["watchers"]["oside"]}
    out = fit_parameters(_bdf2(cfg), None, ("p_sample",), exp, x0=[3.8], max_iter=40, backend=BDF2OracleBackend(),
                         mesh=(mesh.coords, mesh.tris, mesh.tags, mesh.material_tags))
    assert out["scheme"] == "bdf2"
    assert abs(out["values"][0] / 4.07 - 1) <= 1e-6, out["history"]
    assert out["converged"] and out["rmse"] < 1e-8


def test_config_key_and_cli_flags_pass_the_scheme(tmp_path, monkeypatch):
    from heatflow_amd import fit, parameter_sweep
    from heatflow_amd.driver import _with_scheme, time_scheme

    cfg = load_cfg("geballe_with_diamond")
    assert time_scheme(cfg) == "backward_euler"
    assert time_scheme(_bdf2(cfg)) == "bdf2"
    assert _with_scheme(cfg)["timing"]["scheme"] == "backward_euler" and "scheme" not in cfg["timing"]
    with pytest.raises(ValueError):
        time_scheme({"timing": {"scheme": "BDF2 "}})

    path = tmp_path / "cfg.yaml"
    path.write_text(yaml.safe_dump(cfg))
    seen = {}

    def fake_fit(c, mesh_folder, *a, **k):
        seen["fit"] = time_scheme(c)
        return {"params": ["p_sample"], "values": [1.0], "stderr": [0.0], "rmse": 0.0, "converged": True, "iterations": 0,
                "runs": 0, "seconds": 0.0, "scheme": seen["fit"]}

    monkeypatch.setattr(fit, "fit_parameters", fake_fit)
    assert fit.main(["--config", str(path), "--output-dir", str(tmp_path / "f1")]) == 0
    assert seen["fit"] == "backward_euler"
    assert fit.main(["--config", str(path), "--output-dir", str(tmp_path / "f2"), "--scheme", "bdf2"]) == 0
    assert seen["fit"] == "bdf2"

    def fake_sweep(*a, **k):
        seen["sweep"] = k.get("scheme")

    monkeypatch.setattr(parameter_sweep, "run_parameter_sweep", fake_sweep)
    base = ["--config", str(path), "--output-dir", str(tmp_path / "s"), "--fwhm-range", "1e-5", "1e-5", "--k-range", "3", "4",
            "--width-range", "1e-6", "1e-6", "--num-points", "1", "2", "1"]
    parameter_sweep.main(base + ["--scheme", "bdf2"])
    assert seen["sweep"] == "bdf2"
    parameter_sweep.main(base)
    assert seen["sweep"] is None
    with pytest.raises(SystemExit):
        parameter_sweep.main(base + ["--scheme", "euler"])


def test_run_parameter_sweep_rejects_an_unknown_scheme_before_any_work(tmp_path):
    from heatflow_amd.parameter_sweep import run_kappa_sweep, run_parameter_sweep

    cfg = load_cfg("geballe_with_diamond")
    path = tmp_path / "cfg.yaml"
    path.write_text(yaml.safe_dump(cfg))
    with pytest.raises(ValueError):
        run_parameter_sweep(str(path), str(tmp_path / "out"), (1e-5, 1e-5), (3, 4), (1e-6, 1e-6), (1, 2, 1), scheme="bdf3")
    assert not os.path.exists(tmp_path / "out")
    bad = copy.deepcopy(cfg)
    bad["timing"]["scheme"] = "leapfrog"
    with pytest.raises(ValueError):
        run_kappa_sweep(bad, str(tmp_path / "mesh"), [3.0], str(tmp_path / "out2"))


def test_used_config_records_the_scheme(small, tmp_path):
    from heatflow_amd.driver import run_simulation_impl
    from heatflow_amd.mesh import Mesh  # noqa: F401  (the mesh folder is built by prepare_mesh)
    from heatflow_amd.parameter_sweep import get_watcher_points

    cfg, stack, mesh = small
    out = tmp_path / "run"
    res = run_simulation_impl("with_diamond", _bdf2(cfg), str(tmp_path / "mesh"), rebuild_mesh=True, output_folder=str(out),
                              watcher_points=get_watcher_points(cfg), write_xdmf=False, suppress_print=True,
                              backend=BDF2OracleBackend())
    assert len(res["times"]) == 30
    with open(out / "used_config.yaml") as f:
        assert yaml.safe_load(f)["timing"]["scheme"] == "bdf2"


def test_run_1d_refuses_bdf2(tmp_path):
    from heatflow_amd.run_no_diamond_1d import run_1d

    cfg = load_cfg("geballe_1d")
    cfg.setdefault("timing", {})["scheme"] = "bdf2"
    with pytest.raises(ValueError, match="1-D model"):
        run_1d(cfg, str(tmp_path / "no_mesh_here"))
