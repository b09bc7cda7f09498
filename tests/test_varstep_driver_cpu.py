"""The drivers under ``timing.steps`` and ``timing.adaptive`` without a GPU: parsing of the two keys, every
refusal by message, SimulationSession.run and run_simulation on the restatement backend of tests/varstep_oracle.py, and the
replay of an adaptive run's ``steps_taken`` as a list, bit for bit."""
import copy
import csv
import warnings

import numpy as np
import pytest
import yaml

from conftest import load_cfg
from helpers import make_problem
from varstep_oracle import VarstepOracleBackend

from heatflow_amd import stepping

SEGMENTS = [{"until": 1.5e-6, "num_steps": 5}, {"until": 7.5e-6, "num_steps": 9}]


def _cfg(cfg, **timing):
    c = copy.deepcopy(cfg)
    c["timing"].pop("num_steps", None)
    c["timing"].update(timing)
    return c


def _session(mesh):
    from heatflow_amd.driver import SimulationSession

    return SimulationSession(mesh.coords, mesh.tris, mesh.tags, mesh.material_tags, backend=VarstepOracleBackend())


def test_timing_plan_parses_the_keys():
    base = {"timing": {"t_final": 7.5e-6, "num_steps": 100}}
    assert stepping.timing_plan(base) == ("uniform", 100) and stepping.assembled_step(base) == 7.5e-6 / 100
    c = _cfg(base, steps=SEGMENTS)
    kind, dts = stepping.timing_plan(c)
    assert kind == "steps" and len(dts) == 14 and dts[:5] == [1.5e-6 / 5] * 5 and dts[5:] == [(7.5e-6 - 1.5e-6) / 9] * 9
    assert stepping.assembled_step(c) == dts[0]
    a = _cfg(base, adaptive={"tol": 0.1, "dt_min": 1e-12})
    assert stepping.timing_plan(a) == ("adaptive", {"tol": 0.1, "dt_min": 1e-12}) and stepping.assembled_step(a) == 7.5e-6 / 400
    assert stepping.assembled_step(_cfg(base, adaptive={"tol": 0.1, "dt_init": 2e-8})) == 2e-8
    with pytest.warns(RuntimeWarning, match="num_steps is ignored next to timing.steps"):
        stepping.timing_plan(dict(timing=dict(c["timing"], num_steps=7)))
    with pytest.raises(ValueError, match="num_steps is required"):
        stepping.timing_plan({"timing": {"t_final": 1.0}})
    with pytest.raises(ValueError, match="timing.steps together with timing.adaptive"):
        stepping.timing_plan(_cfg(base, steps=SEGMENTS, adaptive={"tol": 0.1}))
    for bad, text in (([], "non-empty"), ([{"until": 7.5e-6}], "until and num_steps"),
                      ([{"until": 7.5e-6, "num_steps": 0}], "num_steps must be"), ([{"until": 7.0e-6, "num_steps": 3}], "must equal timing.t_final"),
                      ([{"until": 2e-6, "num_steps": 2}, {"until": 1e-6, "num_steps": 2}], "does not lie beyond")):
        with pytest.raises(ValueError, match=text):
            stepping.timing_plan(_cfg(base, steps=bad))
    for bad, text in (({}, "with tol"), ({"tol": 0.0}, "adaptive.tol must be positive"), ({"tol": 0.1, "safety": 1}, "unknown key 'safety'"),
                      ({"tol": 0.1, "dt_min": -1.0}, "adaptive.dt_min")):
        with pytest.raises(ValueError, match=text):
            stepping.timing_plan(_cfg(base, adaptive=bad))


@pytest.mark.parametrize("key", ["steps", "adaptive"])
def test_every_other_path_refuses_the_keys_by_name(case_with_diamond_small, tmp_path, key):
    from heatflow_amd.fit import fit_parameters as fit
    from heatflow_amd.parameter_sweep import build_stack, get_watcher_points, run_kappa_sweep, run_parameter_sweep
    from heatflow_amd.run_no_diamond_1d import run_1d

    cfg, stack, mesh = case_with_diamond_small
    c = _cfg(cfg, **({"steps": SEGMENTS} if key == "steps" else {"adaptive": {"tol": 0.5}}))
    both = r"timing\.steps / timing\.adaptive"
    path = tmp_path / "cfg.yaml"
    path.write_text(yaml.safe_dump(c))
    with pytest.raises(ValueError, match="run_parameter_sweep together with timing." + key + ".*" + both):
        run_parameter_sweep(str(path), str(tmp_path / "out"), (1e-5, 1e-5), (3, 4), (1e-6, 1e-6), (1, 2, 1))
    with pytest.raises(ValueError, match="run_kappa_sweep together with timing." + key + ".*" + both):
        run_kappa_sweep(c, str(tmp_path / "mesh"), [3.0], str(tmp_path / "out2"))
    with pytest.raises(ValueError, match=r"heatflow_amd\.fit together with timing." + key + ".*" + both):
        fit(c, str(tmp_path / "mesh"), ["p_sample"])
    one_d = load_cfg("geballe_1d")
    one_d["timing"].update({k: v for k, v in c["timing"].items() if k in ("steps", "adaptive")})
    with pytest.raises(ValueError, match="1-D model.* together with timing." + key + ".*" + both):
        run_1d(one_d, str(tmp_path / "no_mesh_here"))
    s = _session(mesh)
    try:
        wp = get_watcher_points(c)
        with pytest.raises(ValueError, match="run_batch.* together with timing." + key + ".*" + both):
            s.run_batch([c, c], [build_stack(c), build_stack(c)], wp)
        with pytest.raises(ValueError, match="tangents= together with timing." + key + ".*" + both):
            s.run(c, build_stack(c), wp, tangents=["p_sample"])
        with pytest.raises(ValueError, match="the read-flux run together with timing." + key + ".*" + both):
            s.run(c, build_stack(c), wp, read_flux=True)
        mon = copy.deepcopy(c)
        mon["monitors"] = {"sample": {"material": "p_sample"}}
        with pytest.raises(ValueError, match="monitor_sigma= together with timing." + key + ".*" + both):
            s.run(mon, build_stack(mon), wp, monitor_sigma={"p_sample": 0.05})
    finally:
        s.close()


def test_session_run_with_a_step_list_matches_run_steps(case_with_diamond_small):
    from heatflow_amd.driver import _parse_watchers
    from heatflow_amd.parameter_sweep import build_stack, get_watcher_points
    from heatflow_amd.solver import nearest_nodes

    cfg, stack, mesh = case_with_diamond_small
    c = _cfg(cfg, steps=SEGMENTS, scheme="bdf2")
    names, pts = _parse_watchers(get_watcher_points(c))
    nodes = nearest_nodes(mesh.coords, pts)
    kind, dts = stepping.timing_plan(c)
    s = _session(mesh)
    try:
        res = s.run(c, build_stack(c), get_watcher_points(c))
        fields = []
        sunk = s.run(c, build_stack(c), get_watcher_points(c), field_sink=lambda t, u: fields.append((t, u[nodes].copy())))
    finally:
        s.close()
    assert np.array_equal(res["times"], np.cumsum(dts)) and res["times"][-1] == pytest.approx(7.5e-6, rel=1e-14)
    cu = copy.deepcopy(c)
    cu["timing"]["num_steps"] = 1
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        prob = make_problem(dict(cu, timing=dict(cu["timing"], t_final=dts[0])), stack, mesh, backend=VarstepOracleBackend(), scheme="bdf2")
    _, want, _ = prob.run_steps(dts, watcher_nodes=nodes, time_varying=[prob.bcs[3]])
    for q, nm in enumerate(names):
        assert np.array_equal(res["watchers"][nm], want[:, q])
        assert np.array_equal(sunk["watchers"][nm], want[:, q])                 # the step-wise path (a field sink) takes the same steps
    assert [t for t, _ in fields] == list(np.cumsum(dts)) and np.array_equal(np.array([u for _, u in fields]), want)
    assert np.abs(want[-1] - 300.0).max() > 1.0


def test_run_simulation_adaptive_writes_the_times_and_replays_bit_for_bit(case_with_diamond_small, tmp_path):
    from heatflow_amd.driver import _parse_watchers, run_simulation_impl
    from heatflow_amd.parameter_sweep import get_watcher_points
    from heatflow_amd.solver import nearest_nodes

    cfg, stack, mesh = case_with_diamond_small
    c = _cfg(cfg, adaptive={"tol": 2.0, "dt_min": 1e-13}, scheme="bdf2")
    out = tmp_path / "run"
    res = run_simulation_impl("with_diamond", c, str(tmp_path / "mesh"), rebuild_mesh=True, output_folder=str(out),
                              watcher_points=get_watcher_points(c), write_xdmf=False, suppress_print=True,
                              backend=VarstepOracleBackend())
    taken = res["steps_taken"]
    assert res["times"][-1] == 7.5e-6 and len(taken) == len(res["times"]) == res["adaptive"]["accepted"]
    assert np.abs(np.cumsum(taken)[:-1] - res["times"][:-1]).max() <= 1e-18
    with open(out / "used_config.yaml") as f:
        used = yaml.safe_load(f)
    assert used["timing"]["adaptive"] == {"tol": 2.0, "dt_min": 1e-13} and used["timing"]["steps_taken"] == taken
    assert "num_steps" not in used["timing"] and "steps" not in used["timing"]
    with open(out / "watcher_points.csv") as f:
        rows = list(csv.reader(f))
    assert len(rows) == len(taken) + 1 and float(rows[-1][0]) == pytest.approx(7.5e-6, rel=1e-12)
    assert float(rows[1][0]) == pytest.approx(taken[0], rel=1e-12)
    # the replay of steps_taken as a list, on a problem of the run's own mesh
    from heatflow_amd.driver import prepare_mesh
    from heatflow_amd.geometry import build_stack

    st = build_stack(c)
    coords, tris, tags, tag_map = prepare_mesh(c, str(tmp_path / "mesh"), False, st)
    m2 = type("M", (), dict(coords=coords, tris=tris, tags=tags, material_tags=tag_map))
    names, pts = _parse_watchers(get_watcher_points(c))
    nodes = nearest_nodes(coords, pts)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        prob = make_problem(dict(c, timing=dict(c["timing"], t_final=7.5e-6 / 400, num_steps=1)), st, m2,
                            backend=VarstepOracleBackend(), scheme="bdf2")
    _, want, _ = prob.run_steps(used["timing"]["steps_taken"], watcher_nodes=nodes, time_varying=[prob.bcs[3]], consistent_start=True)
    for q, nm in enumerate(names):
        assert np.array_equal(res["watchers"][nm], want[:, q])


def test_a_fixed_step_configuration_writes_no_new_key(case_with_diamond_small, tmp_path):
    from heatflow_amd.driver import _with_scheme

    cfg, _, _ = case_with_diamond_small
    used = _with_scheme(cfg)
    assert "steps" not in used["timing"] and "adaptive" not in used["timing"] and "steps_taken" not in used["timing"]
    assert _with_scheme(_cfg(cfg, steps=SEGMENTS))["timing"]["steps"] == SEGMENTS
