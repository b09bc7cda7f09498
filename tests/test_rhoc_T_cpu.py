"""Temperature-dependent heat capacities without a GPU: the restatement of tests/rhoc_T_oracle.py against the linear and the
kappa(T) loops, the Einstein tabulation, the configuration keys, HeatProblem's call order, the refusals, and the header."""
import copy
import os
import re

import numpy as np
import pytest

from conftest import ROOT, build_case, load_cfg
from kappa_T_oracle import kappa_t_fields, linear_fields, problem_inputs
from rhoc_T_oracle import BDF2, BE, einstein, einstein_tables, rhoc_t_fields


@pytest.fixture(scope="module")
def small():
    return build_case("geballe_with_diamond", 8.0)


def _insulator_tags(mesh):
    return [mesh.material_tags[m] for m in ("p_ins", "o_ins", "g_ins")]


def _args(small, steps=20):
    cfg, stack, mesh = small
    tk, trc, dt, dofs, u0, g = problem_inputs(cfg, stack, mesh, steps)
    return mesh, (mesh.coords, mesh.tris, mesh.tags, tk, trc, dt, dofs, u0, g), tk, trc


@pytest.mark.parametrize("scheme", [BE, BDF2])
def test_no_tables_is_the_linear_oracle_exactly(small, scheme):
    _, a, _, _ = _args(small)
    f, _ = rhoc_t_fields(*a, scheme=scheme)
    np.testing.assert_array_equal(f, linear_fields(*a, scheme))


@pytest.mark.parametrize("scheme", [BE, BDF2])
@pytest.mark.parametrize("picard", [1, 2])
def test_conductivity_tables_only_is_the_kappa_oracle_exactly(small, scheme, picard):
    mesh, a, tk, _ = _args(small, 10)
    kt = {t: (300.0, 10.0, tk[t] * 300.0 / (300.0 + 10.0 * np.arange(51))) for t in _insulator_tags(mesh)}
    f, c = rhoc_t_fields(*a, kappa_tables=kt, scheme=scheme, picard=picard)
    fk, ck = kappa_t_fields(*a, kt, scheme, picard)
    np.testing.assert_array_equal(f, fk)
    np.testing.assert_array_equal(c, ck)


@pytest.mark.parametrize("scheme", [BE, BDF2])
@pytest.mark.parametrize("picard", [1, 2])
def test_constant_capacity_tables_equal_the_linear_oracle(small, scheme, picard):
    mesh, a, _, trc = _args(small)
    tables = {t: (250.0, 100.0, [trc[t]] * 5) for t in _insulator_tags(mesh)}
    f, _ = rhoc_t_fields(*a, rhoc_tables=tables, scheme=scheme, picard=picard)
    lin = linear_fields(*a, scheme)
    assert np.abs(lin[-1] - lin[0]).max() > 1.0
    assert np.abs(f - lin).max() <= 1e-9


def test_capacity_tables_change_the_answer_and_picard_converges(small):
    mesh, a, _, trc = _args(small)
    tables = einstein_tables(trc, _insulator_tags(mesh))
    lin = linear_fields(*a)
    ch = {}
    for p in (1, 3, 6):
        f, c = rhoc_t_fields(*a, rhoc_tables=tables, picard=p)
        ch[p] = c.max()
        print(f"p = {p}: field moved by {np.abs(f - lin).max():.4g} K, largest last Picard change {ch[p]:.3g} K")
        assert np.abs(f - lin).max() > 1.0
    assert ch[1] > ch[3] > ch[6]


def test_einstein_and_cv_tables():
    from heatflow_amd.kappa_t import einstein_function, einstein_table, material_cv_table

    np.testing.assert_allclose(einstein_function(np.array([2.0, 0.75])), einstein(np.array([300.0, 800.0]), 600.0), rtol=1e-14)
    assert abs(float(einstein_function(600.0 / 800.0) / einstein_function(2.0)) - 1.32) < 0.01   # + 32 % from 300 K to 800 K
    T0, dT, v = einstein_table(1000.0, 600.0, 300.0, 300.0, 800.0, knots=51)
    assert (T0, dT, len(v)) == (300.0, 10.0, 51)
    assert v[0] == 1000.0                                   # the constant is the value at T_ref
    np.testing.assert_allclose(v, 1000.0 * einstein(300.0 + 10.0 * np.arange(51), 600.0) / einstein(300.0, 600.0), rtol=1e-14)
    assert len(einstein_table(1.0, 600.0, 300.0, 100.0, 200.0)[2]) == 256
    mat = {"rho": 2.0, "cv": 5.0, "cv_table": {"T_min": 300.0, "T_max": 700.0, "cv": [5.0, 6.0, 7.0]}}
    T0, dT, v = material_cv_table("m", mat)
    assert (T0, dT) == (300.0, 200.0) and list(v) == [10.0, 12.0, 14.0]        # rho * cv is handed down
    mat = {"rho": 2.0, "cv": 5.0, "cv_einstein": {"theta": 600.0, "T_ref": 400.0, "T_min": 300.0, "T_max": 500.0, "knots": 3}}
    T0, dT, v = material_cv_table("m", mat)
    assert (T0, dT) == (300.0, 100.0) and v[1] == 10.0 and v[0] < v[1] < v[2]
    assert material_cv_table("m", {"rho": 2.0, "cv": 5.0}) is None
    for bad in (lambda: einstein_table(1.0, 600.0, 300.0, 300.0, 800.0, knots=257),
                lambda: einstein_table(1.0, 600.0, 300.0, 800.0, 300.0),
                lambda: einstein_table(1.0, -1.0, 300.0, 300.0, 800.0),
                lambda: material_cv_table("m", {"rho": 1.0, "cv": 1.0, "cv_table": {"T_min": 300.0, "T_max": 700.0, "cv": [1.0]}}),
                lambda: material_cv_table("m", {"rho": 1.0, "cv": 1.0, "cv_table": {"T_min": 300.0, "T_max": 700.0, "cv": [1.0, -1.0]}}),
                lambda: material_cv_table("m", {"rho": 1.0, "cv": 1.0, "cv_table": {"T_min": 700.0, "T_max": 300.0, "cv": [1.0, 2.0]}})):
        with pytest.raises(ValueError):
            bad()


def test_config_keys_are_parsed_into_the_stack():
    from heatflow_amd.geometry import build_stack
    from heatflow_amd.kappa_t import picard_sweeps, table_keys

    cfg = load_cfg("geballe_with_diamond_cvT")
    stack = build_stack(cfg)
    assert {m.name for m in stack.materials if "rho_cv_table" in m.properties} == {"p_ins", "o_ins", "g_ins"}
    assert {m.name for m in stack.materials if "k_table" in m.properties} == {"p_ins", "o_ins", "g_ins"}
    props = stack.by_name("p_ins").properties
    T0, dT, v = props["rho_cv_table"]
    assert T0 == 300.0 and len(v) == 64 and v[0] == props["rho_cv"] == 4131 * 668
    assert abs(v[-1] / v[0] - float(einstein(900.0, 600.0) / einstein(300.0, 600.0))) < 1e-12
    assert picard_sweeps(cfg) == 2
    assert {"mats.p_ins.k_power", "mats.p_ins.cv_einstein"} <= set(table_keys(cfg))
    c = copy.deepcopy(load_cfg("geballe_with_diamond"))
    assert table_keys(c) == []
    assert all("rho_cv_table" not in m.properties for m in build_stack(c).materials)
    c["mats"]["p_sample"]["cv_table"] = {"T_min": 300.0, "T_max": 700.0, "cv": [400.0, 500.0]}
    t = build_stack(c).by_name("p_sample").properties["rho_cv_table"]
    assert t[1] == 400.0 and t[2][1] == c["mats"]["p_sample"]["rho"] * 500.0
    c["mats"]["p_sample"]["cv_einstein"] = {"theta": 600.0, "T_ref": 300.0, "T_min": 300.0, "T_max": 900.0}
    with pytest.raises(ValueError, match="cv_table and cv_einstein are exclusive"):
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


def test_heat_problem_sets_the_state_before_assembling_with_capacity_tables(small):
    head = ["set_mesh", "set_materials", "set_dirichlet", "set_precond"]
    only_c, both, without = RecordingBackend(), RecordingBackend(), RecordingBackend()
    _problem(small, only_c, rhoc_tables={3: (300.0, 10.0, [1.0, 2.0])}, picard=2)
    _problem(small, both, rhoc_tables={3: (300.0, 10.0, [1.0, 2.0])}, kappa_tables={3: (300.0, 10.0, [1.0, 2.0])}, picard=2)
    _problem(small, without)
    assert without.calls == head + ["assemble", "set_state"]
    assert only_c.calls == head + ["set_rhoc_tables", "set_picard", "set_state", "assemble"]
    assert both.calls == head + ["set_kappa_tables", "set_rhoc_tables", "set_picard", "set_state", "assemble"]


def _cv_cfg():
    """The stock configuration with capacity tables only (no k_* key anywhere)."""
    cfg = copy.deepcopy(load_cfg("geballe_with_diamond"))
    cfg["mats"]["p_ins"]["cv_einstein"] = {"theta": 600.0, "T_ref": 300.0, "T_min": 300.0, "T_max": 900.0, "knots": 16}
    cfg["mats"]["o_ins"]["cv_table"] = {"T_min": 300.0, "T_max": 900.0, "cv": [668.0, 800.0]}
    return cfg


def test_sweeps_fit_and_1d_refuse_capacity_tables(tmp_path):
    import yaml

    from heatflow_amd import fit, parameter_sweep, run_no_diamond_1d

    cfg = _cv_cfg()
    pat = r"heat capacities \(mats\.o_ins\.cv_table, mats\.p_ins\.cv_einstein\)"
    with pytest.raises(ValueError, match=pat):
        parameter_sweep.run_kappa_sweep(cfg, str(tmp_path), [3.8], str(tmp_path))
    p = tmp_path / "c.yaml"
    p.write_text(yaml.safe_dump(cfg))
    with pytest.raises(ValueError, match=pat):
        parameter_sweep.run_parameter_sweep(str(p), str(tmp_path), [1e-5, 1e-5], [3.8, 3.8], [1.84e-6, 1.84e-6], 1)
    with pytest.raises(ValueError, match=pat):
        fit.fit_parameters(cfg, str(tmp_path))
    with pytest.raises(ValueError, match=pat):
        run_no_diamond_1d.run_1d(cfg, str(tmp_path))
    # a configuration with both kinds keeps the conductivity message of before
    with pytest.raises(ValueError, match=r"temperature-dependent conductivities \(mats\.\w+\.k_power"):
        fit.fit_parameters(load_cfg("geballe_with_diamond_cvT"), str(tmp_path))


def test_session_refuses_tangents_and_batches_with_capacity_tables(small):
    from oracle_backend import OracleBackend

    from heatflow_amd.driver import SimulationSession
    from heatflow_amd.geometry import build_stack
    from heatflow_amd.parameter_sweep import get_watcher_points

    _, _, mesh = small
    cfg = _cv_cfg()
    cfg["mats"] = {k: dict(v, mesh=v["mesh"] * 8.0) for k, v in cfg["mats"].items()}
    s = SimulationSession(mesh.coords, mesh.tris, mesh.tags, mesh.material_tags, backend=OracleBackend())
    stack = build_stack(cfg)
    with pytest.raises(ValueError, match=r"tangents.*cv_einstein"):
        s.run(cfg, stack, get_watcher_points(cfg), tangents=["p_sample"])
    with pytest.raises(ValueError, match=r"run_batch.*cv_einstein"):
        s.run_batch([cfg, cfg], [stack, stack], get_watcher_points(cfg))


def test_session_hands_the_capacity_tables_to_the_problem(small):
    from heatflow_amd.driver import SimulationSession
    from heatflow_amd.geometry import build_stack

    _, _, mesh = small
    s = SimulationSession(mesh.coords, mesh.tris, mesh.tags, mesh.material_tags, backend=RecordingBackend())
    cfg = _cv_cfg()
    spec = s.spec(cfg, build_stack(cfg))
    assert spec.kappa_tables == {} and spec.picard == 1
    assert set(spec.rhoc_tables) == {mesh.material_tags["p_ins"], mesh.material_tags["o_ins"]}
    assert spec.rhoc_tables[mesh.material_tags["o_ins"]][2][1] == 4131 * 800.0
    kw = spec.problem_kwargs()
    assert kw["kappa_tables"] == {} and kw["picard"] == 1 and kw["rhoc_tables"] is spec.rhoc_tables
    plain = load_cfg("geballe_with_diamond")
    none = s.spec(plain, build_stack(plain))
    assert not none.tabled and none.kappa_tables == {} and none.rhoc_tables == {}
    assert not {"kappa_tables", "rhoc_tables", "picard"} & set(none.problem_kwargs())


def test_used_config_records_the_capacity_tables():
    from heatflow_amd.driver import _with_scheme

    out = _with_scheme(load_cfg("geballe_with_diamond_cvT"))
    assert out["timing"]["picard_sweeps"] == 2
    assert set(out["rhoc_tables"]) == set(out["kappa_tables"]) == {"p_ins", "o_ins", "g_ins"}
    assert len(out["rhoc_tables"]["p_ins"]["rho_cv"]) == 64 and out["rhoc_tables"]["p_ins"]["rho_cv"][0] == 4131 * 668
    only = _with_scheme(_cv_cfg())
    assert set(only["rhoc_tables"]) == {"p_ins", "o_ins"} and "kappa_tables" not in only and only["timing"]["picard_sweeps"] == 1
    for name in ("geballe_with_diamond", "geballe_with_diamond_kT"):      # files written today keep their content
        assert "rhoc_tables" not in _with_scheme(load_cfg(name))


def test_header_declares_and_backend_lists_the_rhoc_T_entry_points():
    from heatflow_amd import hip_backend

    with open(os.path.join(ROOT, "include", "heatflow_hip.h")) as f:
        text = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    for name in ("hf_set_rhoc_tables", "hf_set_picard"):
        assert re.search(rf"\b{name}\s*\(", text)
        assert name in hip_backend.EXPORTS
    assert hasattr(hip_backend.HeatflowHIP, "set_rhoc_tables") and hasattr(hip_backend.HeatflowHIP, "set_picard")
