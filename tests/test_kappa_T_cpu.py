"""Temperature-dependent conductivities without a GPU: the restatement of tests/kappa_T_oracle.py against the linear loop,
table and power-law tabulation, the configuration keys, HeatProblem's call order, the refusals, and the header."""
import copy
import os
import re

import numpy as np
import pytest

from conftest import ROOT, build_case, load_cfg
from kappa_T_oracle import BDF2, BE, element_temperature, kappa_t_fields, linear_fields, problem_inputs, table_eval


@pytest.fixture(scope="module")
def small():
    return build_case("geballe_with_diamond", 8.0)


def _insulator_tags(stack, mesh):
    return [mesh.material_tags[m] for m in ("p_ins", "o_ins", "g_ins")]


@pytest.mark.parametrize("scheme", [BE, BDF2])
@pytest.mark.parametrize("picard", [1, 2])
def test_constant_tables_equal_the_linear_oracle(small, scheme, picard):
    cfg, stack, mesh = small
    tk, trc, dt, dofs, u0, g = problem_inputs(cfg, stack, mesh, 20)
    tables = {t: (250.0, 100.0, [tk[t]] * 5) for t in _insulator_tags(stack, mesh)}
    kt, _ = kappa_t_fields(mesh.coords, mesh.tris, mesh.tags, tk, trc, dt, dofs, u0, g, tables, scheme, picard)
    lin = linear_fields(mesh.coords, mesh.tris, mesh.tags, tk, trc, dt, dofs, u0, g, scheme)
    assert np.abs(lin[-1] - lin[0]).max() > 1.0
    assert np.abs(kt - lin).max() <= 1e-9


def test_kappa_of_T_changes_the_answer_and_picard_converges(small):
    cfg, stack, mesh = small
    tk, trc, dt, dofs, u0, g = problem_inputs(cfg, stack, mesh, 20)
    tables = {t: (300.0, 10.0, tk[t] * 300.0 / (300.0 + 10.0 * np.arange(61))) for t in _insulator_tags(stack, mesh)}
    lin = linear_fields(mesh.coords, mesh.tris, mesh.tags, tk, trc, dt, dofs, u0, g)
    ch = {}
    for p in (1, 3, 5):
        f, c = kappa_t_fields(mesh.coords, mesh.tris, mesh.tags, tk, trc, dt, dofs, u0, g, tables, BE, p)
        ch[p] = c[-1]
        assert np.abs(f - lin).max() > 1e-2
    assert ch[1] > ch[3] > ch[5]


def test_table_eval_interpolates_and_clamps():
    v = np.array([4.0, 2.0, 1.0])
    T = np.array([-1e9, 0.0, 5.0, 10.0, 15.0, 20.0, 25.0, 1e9, np.nan])
    out = table_eval(T, 0.0, 10.0, v)
    np.testing.assert_array_equal(out[:8], [4.0, 4.0, 3.0, 2.0, 1.5, 1.0, 1.0, 1.0])


def test_element_temperature_is_order_independent():
    rng = np.random.default_rng(3)
    u = rng.random(3) * 1000 + 300
    for perm in ([0, 1, 2], [1, 2, 0], [2, 0, 1], [0, 2, 1]):
        assert element_temperature(u, np.array([perm]))[0] == element_temperature(u, np.array([[0, 1, 2]]))[0]


def test_power_law_and_uniform_tables():
    from heatflow_amd.kappa_t import power_law_table, uniform_table

    T0, dT, v = power_law_table(10.0, 300.0, 1.0, 300.0, 900.0, knots=7)
    assert (T0, dT, len(v)) == (300.0, 100.0, 7)
    np.testing.assert_allclose(v, 10.0 * 300.0 / (300.0 + 100.0 * np.arange(7)), rtol=1e-15)
    assert len(power_law_table(1.0, 300.0, 0.5, 100.0, 200.0)[2]) == 256
    T0, dT, v = uniform_table(300.0, 700.0, [3.0, 2.0, 1.0])
    assert (T0, dT) == (300.0, 200.0) and list(v) == [3.0, 2.0, 1.0]
    for bad in (lambda: power_law_table(1.0, 300.0, 1.0, 300.0, 900.0, knots=257),
                lambda: power_law_table(1.0, 300.0, 1.0, 900.0, 300.0),
                lambda: uniform_table(300.0, 700.0, [1.0]),
                lambda: uniform_table(300.0, 700.0, [1.0, -1.0])):
        with pytest.raises(ValueError):
            bad()


def test_config_keys_are_parsed_into_the_stack():
    from heatflow_amd.geometry import build_stack
    from heatflow_amd.kappa_t import picard_sweeps, table_keys

    cfg = load_cfg("geballe_with_diamond_kT")
    stack = build_stack(cfg)
    tabled = {m.name for m in stack.materials if "k_table" in m.properties}
    assert tabled == {"p_ins", "o_ins", "g_ins", "p_diam", "o_diam"}
    T0, dT, v = stack.by_name("p_ins").properties["k_table"]
    assert T0 == 300.0 and len(v) == 64 and v[0] == 10.0 and abs(v[-1] - 10.0 / 3.0) < 1e-12
    assert picard_sweeps(cfg) == 1
    assert "mats.p_ins.k_power" in table_keys(cfg)
    c = copy.deepcopy(load_cfg("geballe_with_diamond"))
    c["mats"]["p_sample"]["k_table"] = {"T_min": 300.0, "T_max": 700.0, "k": [4.0, 3.0]}
    assert build_stack(c).by_name("p_sample").properties["k_table"][1] == 400.0
    c["timing"]["picard_sweeps"] = 9
    with pytest.raises(ValueError, match="picard_sweeps"):
        picard_sweeps(c)
    c["mats"]["p_sample"]["k_power"] = {"T_ref": 300.0, "exponent": 1.0, "T_min": 300.0, "T_max": 900.0}
    with pytest.raises(ValueError, match="exclusive"):
        build_stack(c)


class RecordingBackend:
    """Records the HeatflowHIP calls HeatProblem makes."""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        if name.startswith("_"):
            raise AttributeError(name)

        def rec(*a, **k):
            self.calls.append(name)
            return None
        return rec


def _problem(small, backend, **kw):
    from helpers import make_problem

    cfg, stack, mesh = small
    return make_problem(cfg, stack, mesh, backend=backend, **kw)


def test_heat_problem_sets_the_state_before_assembling_with_tables(small):
    with_t, without = RecordingBackend(), RecordingBackend()
    _problem(small, with_t, kappa_tables={3: (300.0, 10.0, [1.0, 2.0])}, picard=2)
    _problem(small, without)
    assert without.calls == ["set_mesh", "set_materials", "set_dirichlet", "set_precond", "assemble", "set_state"]
    assert with_t.calls == ["set_mesh", "set_materials", "set_dirichlet", "set_precond", "set_kappa_tables", "set_state", "assemble"]


def _kt_cfg():
    return load_cfg("geballe_with_diamond_kT")


def test_sweeps_fit_and_1d_refuse_kappa_tables(tmp_path):
    import yaml

    from heatflow_amd import fit, parameter_sweep, run_no_diamond_1d

    cfg = _kt_cfg()
    with pytest.raises(ValueError, match=r"mats\.\w+\.k_power"):
        parameter_sweep.run_kappa_sweep(cfg, str(tmp_path), [3.8], str(tmp_path))
    p = tmp_path / "c.yaml"
    p.write_text(yaml.safe_dump(cfg))
    with pytest.raises(ValueError, match=r"mats\.\w+\.k_power"):
        parameter_sweep.run_parameter_sweep(str(p), str(tmp_path), [1e-5, 1e-5], [3.8, 3.8], [1.84e-6, 1.84e-6], 1)
    with pytest.raises(ValueError, match=r"mats\.\w+\.k_power"):
        fit.fit_parameters(cfg, str(tmp_path))
    with pytest.raises(ValueError, match=r"mats\.\w+\.k_power"):
        run_no_diamond_1d.run_1d(cfg, str(tmp_path))


def test_session_refuses_tangents_and_batches_with_tables(small):
    from oracle_backend import OracleBackend

    from heatflow_amd.driver import SimulationSession
    from heatflow_amd.geometry import build_stack
    from heatflow_amd.parameter_sweep import get_watcher_points

    _, _, mesh = small
    cfg = copy.deepcopy(_kt_cfg())
    cfg["mats"] = {k: dict(v, mesh=v["mesh"] * 8.0) for k, v in cfg["mats"].items()}
    s = SimulationSession(mesh.coords, mesh.tris, mesh.tags, mesh.material_tags, backend=OracleBackend())
    stack = build_stack(cfg)
    with pytest.raises(ValueError, match=r"tangents.*k_power"):
        s.run(cfg, stack, get_watcher_points(cfg), tangents=["p_sample"])
    with pytest.raises(ValueError, match=r"run_batch.*k_power"):
        s.run_batch([cfg, cfg], [stack, stack], get_watcher_points(cfg))


def test_used_config_records_the_tables():
    from heatflow_amd.driver import _with_scheme

    out = _with_scheme(_kt_cfg())
    assert out["timing"]["picard_sweeps"] == 1
    assert set(out["kappa_tables"]) == {"p_ins", "o_ins", "g_ins", "p_diam", "o_diam"}
    assert len(out["kappa_tables"]["p_ins"]["k"]) == 64
    assert "kappa_tables" not in _with_scheme(load_cfg("geballe_with_diamond"))


def test_header_declares_and_backend_lists_the_kappa_T_entry_points():
    from heatflow_amd import hip_backend

    with open(os.path.join(ROOT, "include", "heatflow_hip.h")) as f:
        text = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    for name in ("hf_set_kappa_tables", "hf_get_picard_change"):
        assert re.search(rf"\b{name}\s*\(", text)
        assert name in hip_backend.EXPORTS
    assert hasattr(hip_backend.HeatflowHIP, "set_kappa_tables") and hasattr(hip_backend.HeatflowHIP, "picard_change")
