"""The enthalpy form of the capacity without a GPU: the table mean of tests/enthalpy_oracle.py against the integral, the identity
E(x) - E(u) = 1^T M (x - u) the scheme rests on, the balance defect against the iterated lagged scheme's, the stop rule,
HeatProblem's arguments and call order against a stub backend, and the header."""
import os
import re

import numpy as np
import pytest
from scipy.integrate import quad

from conftest import ROOT, build_case
from enthalpy_oracle import Enthalpy, H, bump_tables, table_mean
from kappa_T_oracle import problem_inputs, table_eval
from rhoc_T_oracle import rhoc_t_fields

STEPS = 20
TABLE = (300.0, 10.0, 2.0e6 * (1.0 + 0.3 * np.sin(np.arange(51) * 0.7) + 0.01 * np.arange(51)))       # nothing special about it


def _ins_tags(stack, mesh):
    return [mesh.material_tags[m.name] for m in stack.materials if m.name.endswith("ins")]


@pytest.fixture(scope="module", params=["geballe_with_diamond", "geballe_no_diamond"])
def setup(request):
    cfg, stack, mesh = build_case(request.param, 8.0)
    tk, trc, dt, dofs, u0, g = problem_inputs(cfg, stack, mesh, STEPS)
    ct = bump_tables(trc, _ins_tags(stack, mesh))
    return request.param, mesh, tk, trc, dt, dofs, u0, g, ct


PAIRS = {
    "one segment": [(401.0, 407.5), (300.5, 309.5), (790.25, 799.75)],
    "many segments": [(305.0, 795.0), (333.3, 512.7), (409.0, 411.0), (400.0, 430.0)],
    "below": [(150.0, 299.0), (-20.0, 300.0)],
    "above": [(801.0, 1050.0), (800.0, 900.0)],
    "straddling": [(250.0, 340.0), (760.0, 880.0), (120.0, 1000.0)],
    "tiny": [(404.0, 404.0 + 1e-12), (410.0 - 5e-13, 410.0 + 5e-13), (300.0, 300.0 + 1e-12), (800.0 - 1e-12, 800.0)],
}


@pytest.mark.parametrize("kind", sorted(PAIRS))
def test_table_mean_is_the_integral_over_the_interval(kind):
    """1e-13 relative against scipy's quadrature piece by piece (break points at the knots), and against (H(Tb) - H(Ta)) /
    (Tb - Ta) wherever that difference is itself good to 1e-13: H is ~1e9 here and carries 2.2e-16 of that, so the quotient
    is trusted where |H(Tb) - H(Ta)| >= 1e-2 |H| (a 20 K interval and wider) and only printed for narrower ones."""
    T0, dT, v = TABLE
    knots = T0 + dT * np.arange(len(v))
    for Ta, Tb in PAIRS[kind]:
        m = float(table_mean(Ta, Tb, T0, dT, v))
        assert float(table_mean(Tb, Ta, T0, dT, v)) == m                       # swapped arguments: equal bits
        inside = [float(k) for k in knots if Ta < k < Tb]
        edges = [Ta] + inside + [Tb]
        integral = sum(quad(lambda T: float(table_eval(T, T0, dT, v)), a, b, epsabs=0.0, epsrel=2e-14)[0]
                       for a, b in zip(edges[:-1], edges[1:]))
        ref = integral / (Tb - Ta)
        print(kind, Ta, Tb, "mean", m, "quadrature", ref)
        assert abs(m - ref) <= 1e-13 * abs(ref)
        Ha, Hb = float(H(Ta, T0, dT, v)), float(H(Tb, T0, dT, v))
        if abs(Hb - Ha) >= 1e-2 * max(abs(Ha), abs(Hb)):
            assert abs(m - (Hb - Ha) / (Tb - Ta)) <= 1e-13 * abs(m)


def test_table_mean_of_equal_arguments_is_the_table():
    T0, dT, v = TABLE
    T = np.array([120.0, 300.0, 304.0, 410.0, 555.5, 800.0, 930.0])
    np.testing.assert_array_equal(table_mean(T, T, T0, dT, v), table_eval(T, T0, dT, v))


def test_stored_heat_difference_is_the_chord_mass_matrix_product(setup):
    """E(x) - E(u) = 1^T M(chord capacity between u and x) (x - u) at random states that overshoot the tables, to 1e-12 of
    sum |terms| (the element terms of both sides)."""
    _, mesh, tk, trc, dt, dofs, u0, g, ct = setup
    en = Enthalpy(mesh.coords, mesh.tris, mesh.tags, tk, trc, dt, dofs, ct)
    rng = np.random.default_rng(11)
    for _ in range(3):
        u = 150.0 + 900.0 * rng.random(en.n)
        x = 150.0 + 900.0 * rng.random(en.n)
        tu, tx = en.stored_heat_terms(u), en.stored_heat_terms(x)
        M, _ = en.operators(u, x)
        prod = M @ (x - u)
        scale = np.abs(tu).sum() + np.abs(tx).sum() + np.abs(prod).sum()
        defect = abs((tx.sum() - tu.sum()) - prod.sum())
        print("identity defect", defect / scale)
        assert defect <= 1e-12 * scale


def _defects(en, fields, u0, g):
    prev, out, dE = u0, [], []
    for k, u in enumerate(fields):
        d, rhs = en.balance(prev, u, g[k])
        out.append(abs(d - rhs))
        dE.append(abs(d))
        prev = u
    return np.array(out), max(dE)


def test_balance_defect_against_the_iterated_lagged_scheme(setup):
    """At 8 sweeps the enthalpy form's worst balance defect is <= 1e-4 of the iterated lagged scheme's on the same inputs."""
    name, mesh, tk, trc, dt, dofs, u0, g, ct = setup
    en = Enthalpy(mesh.coords, mesh.tris, mesh.tags, tk, trc, dt, dofs, ct)
    f, sweeps, ch = en.enthalpy_fields(u0, g, sweeps=8)
    lag, _ = rhoc_t_fields(mesh.coords, mesh.tris, mesh.tags, tk, trc, dt, dofs, u0, g, ct, None, picard=8)
    d_en, scale = _defects(en, f, u0, g)
    d_lag, _ = _defects(en, lag, u0, g)
    print(f"{name}: defect / largest dE: enthalpy {d_en.max() / scale:.3g}, lagged {d_lag.max() / scale:.3g}, "
          f"ratio {d_en.max() / d_lag.max():.3g}")
    assert d_lag.max() / scale > 1e-3                                          # the lagged form does not conserve ...
    assert d_en.max() <= 1e-4 * d_lag.max()                                    # ... the chord capacity does, to the change


def test_stop_rule_ends_every_step_below_the_cap(setup):
    name, mesh, tk, trc, dt, dofs, u0, g, ct = setup
    en = Enthalpy(mesh.coords, mesh.tris, mesh.tags, tk, trc, dt, dofs, ct)
    f, sweeps, ch = en.enthalpy_fields(u0, g, sweeps=64, tol=1e-7)
    print(name, "sweeps per step", list(sweeps), "largest last change", ch.max())
    assert sweeps.max() < 64 and ch.max() <= 1e-7
    d, scale = _defects(en, f, u0, g)
    print(name, "defect / largest dE", d.max() / scale)
    f5, s5, c5 = en.enthalpy_fields(u0, g, sweeps=64, tol=1e-7, relax=0.5)
    assert s5.max() < 64 and np.abs(f5 - f).max() <= 1e-5                      # the relaxed iteration reaches the same steps


# ---- HeatProblem against a stub backend -------------------------------------------------------------------------------------

class _Stub:
    """Records the calls HeatProblem makes; answers what the constructor asks."""

    def __init__(self):
        self.calls = []
        self.tab_len = 8

    def __getattr__(self, name):
        def call(*a, **k):
            self.calls.append((name, a))
            if name == "picard_history":
                return np.array([3, 4], dtype=np.int32), np.array([1e-8, 2e-8])
            if name == "stored_heat":
                return np.arange(8.0)
            if name == "get_heat":
                return np.arange(16.0).reshape(2, 8)
            return None
        return call


def _problem(**kw):
    from heatflow_amd.solver import HeatProblem

    coords = np.array([[0.0, 0.0], [1.0, 0.0], [0.0, 1.0], [1.0, 1.0]])
    tris = np.array([[0, 1, 2], [1, 3, 2]])
    tags = np.array([1, 2])
    stub = _Stub()
    prob = HeatProblem(coords, tris, tags, {1: 1.0, 2: 2.0}, {1: 10.0, 2: 20.0}, 0.1, [], 300.0, backend=stub, **kw)
    return prob, [c[0] for c in stub.calls], stub


RT = {1: (300.0, 10.0, [10.0, 12.0, 11.0])}


def test_default_and_lagged_make_the_calls_of_before():
    _, a, _ = _problem(rhoc_tables=RT, picard=2)
    _, b, _ = _problem(rhoc_tables=RT, picard=2, capacity_form="lagged")
    assert a == b
    assert "set_capacity_form" not in a and "set_picard_control" not in a and "set_picard" in a
    _, c, _ = _problem()
    assert "set_capacity_form" not in c


def test_enthalpy_call_order_and_accessors():
    prob, calls, stub = _problem(rhoc_tables=RT, kappa_tables={2: (300.0, 10.0, [1.0, 2.0])}, capacity_form="enthalpy", picard=32,
                                 picard_tol=1e-6, picard_relax=0.5)
    i = calls.index
    assert i("set_kappa_tables") < i("set_rhoc_tables") < i("set_capacity_form") < i("set_picard_control") < i("set_state") < i("assemble")
    assert "set_picard" not in calls
    args = dict((c[0], c[1]) for c in stub.calls)
    assert args["set_kappa_tables"][1] == 1                                    # the cap goes through set_picard_control
    assert args["set_picard_control"] == (1e-6, 0.5, 32)
    h = prob.picard_history()
    assert list(h["sweeps"]) == [3, 4] and list(h["change"]) == [1e-8, 2e-8]
    assert prob.stored_heat() == {1: 2.0 * np.pi * 1.0, 2: 2.0 * np.pi * 2.0}
    assert stub.calls[-1] == ("stored_heat", (300.0,))
    prob.record_heat()
    assert stub.calls[-1] == ("set_heat_records", (True, 300.0))
    hh = prob.heat_history()
    np.testing.assert_array_equal(hh[2], 2.0 * np.pi * np.array([2.0, 10.0]))


@pytest.mark.parametrize("kw, word", [
    (dict(capacity_form="chord"), "capacity_form"),
    (dict(capacity_form="enthalpy", rhoc_tables=None), "rhoc_tables"),
    (dict(capacity_form="enthalpy", scheme="bdf2"), "scheme"),
    (dict(capacity_form="enthalpy", k_aniso={1: (2.0, 1.0)}, aniso_tables=True), "k_aniso"),
    (dict(capacity_form="enthalpy", picard=0), "picard"),
    (dict(capacity_form="enthalpy", picard=65), "picard"),
    (dict(capacity_form="enthalpy", picard_tol=-1e-6), "picard_tol"),
    (dict(capacity_form="enthalpy", picard_relax=0.0), "picard_relax"),
    (dict(capacity_form="enthalpy", picard_relax=1.5), "picard_relax"),
    (dict(picard_tol=1e-6), "capacity_form"),
    (dict(picard_relax=0.5), "capacity_form"),
])
def test_value_errors_name_the_argument(kw, word):
    kw = dict({"rhoc_tables": RT}, **kw)
    with pytest.raises(ValueError, match=word) as e:
        _problem(**kw)
    if kw.get("capacity_form") == "enthalpy":
        assert "enthalpy" in str(e.value) or word.startswith("picard")


def test_picard_history_needs_the_enthalpy_form():
    prob, _, _ = _problem(rhoc_tables=RT)
    with pytest.raises(ValueError, match="enthalpy"):
        prob.picard_history()


def test_header_declares_what_the_backend_exports():
    from heatflow_amd import hip_backend

    with open(os.path.join(ROOT, "include", "heatflow_hip.h")) as f:
        declared = re.findall(r"^(?:int|const char\*)\s+(hf_\w+)\(", f.read(), flags=re.M)
    for name in ("hf_set_capacity_form", "hf_set_picard_control", "hf_get_picard_history", "hf_clear_picard_history", "hf_stored_heat",
                 "hf_set_heat_records", "hf_heat_count", "hf_get_heat", "hf_clear_heat_records"):
        assert name in declared and name in hip_backend.EXPORTS, name
    assert sorted(declared) == sorted(hip_backend.EXPORTS)


# ---- configuration: the latent block, the timing keys, their refusals, used_config.yaml, the drivers ------------------------------

def _latent_cfg():
    """The stock configuration with a latent block alone on p_ins (its own grid) and one next to an Einstein table on o_ins."""
    import copy

    from conftest import load_cfg

    cfg = copy.deepcopy(load_cfg("geballe_with_diamond"))
    cfg["mats"]["p_ins"]["latent"] = {"T_melt": 400.0, "heat": 6.68e4, "width": 100.0, "T_min": 300.0, "T_max": 800.0, "knots": 51}
    cfg["mats"]["o_ins"]["cv_einstein"] = {"theta": 600.0, "T_ref": 300.0, "T_min": 300.0, "T_max": 900.0, "knots": 61}
    cfg["mats"]["o_ins"]["latent"] = {"T_melt": 500.0, "heat": 3.0e4, "width": 60.0}
    cfg["timing"].update(capacity_form="enthalpy", picard_sweeps=32, picard_tol=1e-6)
    return cfg


def test_latent_table_carries_rho_times_heat():
    from heatflow_amd.kappa_t import material_cv_table

    cfg = _latent_cfg()
    for name, heat in (("p_ins", 6.68e4), ("o_ins", 3.0e4)):
        mat = cfg["mats"][name]
        T0, dT, v = material_cv_table(name, mat)
        base = material_cv_table(name, {k: x for k, x in mat.items() if k != "latent"})
        base = np.full(len(v), mat["rho"] * mat["cv"]) if base is None else base[2]
        add = v - base
        integral = np.sum(0.5 * (add[1:] + add[:-1]) * dT)
        want = mat["rho"] * heat
        print(name, "knots", len(v), "integral of the added part / (rho heat) - 1 =", integral / want - 1.0)
        assert abs(integral - want) <= 1e-12 * want                            # to rounding (the base cancels to ~1e-16 of 3e6)
        assert np.all(add >= 0.0) and add.max() > 0.0 and add[0] == 0.0 and add[-1] == 0.0
    assert material_cv_table("p_ins", cfg["mats"]["p_ins"])[:2] == (300.0, 10.0)
    assert len(material_cv_table("o_ins", cfg["mats"]["o_ins"])[2]) == 61          # the Einstein table's grid


def _set(cfg, path, value):
    import copy

    cfg = copy.deepcopy(cfg)
    node = cfg
    for key in path[:-1]:
        node = node.setdefault(key, {})
    if value is None:
        node.pop(path[-1], None)
    else:
        node[path[-1]] = value
    return cfg


@pytest.mark.parametrize("path, value, words", [
    (("timing", "capacity_form"), None, ["mats.o_ins.latent", "timing.capacity_form"]),                    # latent without the form
    (("timing", "capacity_form"), "lagged", ["mats.o_ins.latent", "timing.capacity_form"]),
    (("timing", "capacity_form"), "chord", ["timing.capacity_form", "chord"]),
    (("timing", "scheme"), "bdf2", ["timing.capacity_form", "timing.scheme"]),
    (("mats", "p_sample", "k_aniso"), {"r": 2.0, "z": 1.0}, ["timing.capacity_form", "mats.p_sample.k_aniso"]),
    (("timing", "sweep_tables"), True, ["timing.capacity_form", "timing.sweep_tables"]),
    (("timing", "table_tangents"), True, ["timing.capacity_form", "timing.table_tangents"]),
    (("timing", "picard_sweeps"), 0, ["timing.picard_sweeps"]),
    (("timing", "picard_sweeps"), 65, ["timing.picard_sweeps"]),
    (("timing", "picard_tol"), -1e-6, ["timing.picard_tol"]),
    (("timing", "picard_relax"), 0.0, ["timing.picard_relax"]),
    (("timing", "picard_relax"), 1.5, ["timing.picard_relax"]),
    (("mats", "p_ins", "latent", "width"), 15.0, ["width", "spacing"]),                                    # fewer than three knots
    (("mats", "o_ins", "latent", "knots"), 51, ["mats.o_ins.latent.knots", "mats.o_ins.cv_einstein"]),     # a grid next to a table's
    (("mats", "o_ins", "latent", "T_min"), 300.0, ["mats.o_ins.latent.T_min", "mats.o_ins.cv_einstein"]),
    (("mats", "p_ins", "latent", "T_melt"), 790.0, ["mats.p_ins.latent", "grid"]),
])
def test_configuration_value_errors_name_their_keys(path, value, words):
    from heatflow_amd.geometry import build_stack
    from heatflow_amd.kappa_t import check_capacity_form

    cfg = _set(_latent_cfg(), path, value)
    if path[-1] == "k_aniso":        # (without timing.aniso_tables the stack refuses k_aniso next to any table, as before)
        cfg["timing"]["aniso_tables"] = True
    with pytest.raises(ValueError) as e:
        build_stack(cfg)
        check_capacity_form(cfg)
    for w in words:
        assert w in str(e.value), (w, str(e.value))


def test_lagged_keys_without_the_form_are_refused():
    from conftest import load_cfg
    from heatflow_amd.kappa_t import check_capacity_form

    cfg = load_cfg("geballe_with_diamond_cvT")
    assert check_capacity_form(cfg) == "lagged"
    for key, v in (("picard_tol", 1e-6), ("picard_relax", 0.5)):
        with pytest.raises(ValueError) as e:
            check_capacity_form(_set(cfg, ("timing", key), v))
        assert f"timing.{key}" in str(e.value) and "timing.capacity_form" in str(e.value)
    with pytest.raises(ValueError, match=r"timing\.picard_sweeps must be 1\.\.8"):
        check_capacity_form(_set(cfg, ("timing", "picard_sweeps"), 9))
    plain = _set(load_cfg("geballe_with_diamond"), ("timing", "capacity_form"), "enthalpy")
    with pytest.raises(ValueError, match=r"timing\.capacity_form: enthalpy needs a capacity table"):
        check_capacity_form(plain)


def test_sweeps_fit_1d_tangents_and_batches_refuse_the_form(tmp_path):
    import yaml

    from heatflow_amd import fit, parameter_sweep, run_no_diamond_1d

    cfg = _latent_cfg()
    calls = {
        "run_kappa_sweep": lambda c: parameter_sweep.run_kappa_sweep(c, str(tmp_path), [3.8], str(tmp_path)),
        "heatflow_amd.fit": lambda c: fit.fit_parameters(c, str(tmp_path)),
        "run_1d": lambda c: run_no_diamond_1d.run_1d(c, str(tmp_path)),
    }
    for where, call in calls.items():
        with pytest.raises(ValueError) as e:
            call(cfg)
        assert where in str(e.value) and "timing.capacity_form" in str(e.value), str(e.value)
        with pytest.raises(ValueError) as e:                                   # a latent block without the form: both keys as well
            call(_set(cfg, ("timing", "capacity_form"), None))
        assert where in str(e.value) and "latent" in str(e.value) and "timing.capacity_form" in str(e.value), str(e.value)
    p = tmp_path / "c.yaml"
    p.write_text(yaml.safe_dump(cfg))
    with pytest.raises(ValueError, match=r"run_parameter_sweep.*timing\.capacity_form"):
        parameter_sweep.run_parameter_sweep(str(p), str(tmp_path), [1e-5, 1e-5], [3.8, 3.8], [1.84e-6, 1.84e-6], 1)


class _StubProblem:
    """Stands in for HeatProblem under SimulationSession: records its arguments and calls, answers with fixed arrays."""
    made = []

    def __init__(self, coords, tris, tags, tag_to_k, tag_to_rc, dt, bcs, u0, **kw):
        self.kw, self.calls, self.n, self.iters, self.bcs = kw, [], len(coords), [], bcs
        self.dt = dt
        _StubProblem.made.append(self)

    def __getattr__(self, name):
        if name.startswith("_"):
            raise AttributeError(name)

        def call(*a, **k):
            self.calls.append(name)
        return call

    def run(self, num_steps, watcher_nodes=None, **k):
        self.calls.append("run")
        ns = 0 if watcher_nodes is None else len(watcher_nodes)
        return (np.arange(num_steps) + 1) * self.dt, np.full((num_steps, ns), 300.0), np.full(num_steps, 7)

    def monitor_history(self):
        nsteps = 5
        return {r: {"T_max": np.full(nsteps, 300.0), **({} if any(t in self.kw.get("rhoc_tables", {}) for t in spec["tags"])
                                                         else {"energy": np.zeros(nsteps)})}
                for r, spec in self.kw["monitors"].items()}

    def heat_history(self):
        return {t: np.full(5, float(t)) for t in range(1, 12)}

    def picard_history(self):
        return {"sweeps": np.array([2, 3, 4, 4, 2], dtype=np.int32), "change": np.array([0.0, 1e-8, 5e-6, 1e-7, 0.0])}


def _session_run(monkeypatch, cfg):
    from heatflow_amd import driver
    from heatflow_amd.geometry import build_stack, scale_mesh_sizes
    from heatflow_amd.parameter_sweep import get_watcher_points

    cfg = scale_mesh_sizes(cfg, 8.0)
    cfg["timing"]["num_steps"] = 5
    _, stack, mesh = build_case("geballe_with_diamond", 8.0)
    monkeypatch.setattr(driver, "HeatProblem", _StubProblem)
    _StubProblem.made.clear()
    s = driver.SimulationSession(mesh.coords, mesh.tris, mesh.tags, mesh.material_tags, backend=object())
    return s, cfg, build_stack(cfg), get_watcher_points(cfg), mesh


def test_the_driver_carries_the_keys_and_reports_picard_and_energy(monkeypatch):
    import warnings

    cfg = _latent_cfg()
    cfg["timing"]["picard_sweeps"] = 4
    cfg["monitors"] = {"ins": {"material": "p_ins"}, "sample": {"material": "p_sample"}}
    s, cfg, stack, wp, mesh = _session_run(monkeypatch, cfg)
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        res = s.run(cfg, stack, wp)
    prob = _StubProblem.made[-1]
    assert prob.kw["capacity_form"] == "enthalpy" and prob.kw["picard"] == 4 and prob.kw["picard_tol"] == 1e-6 and prob.kw["picard_relax"] == 1.0
    assert set(prob.kw["rhoc_tables"]) == {mesh.material_tags["p_ins"], mesh.material_tags["o_ins"]}
    assert prob.calls.index("record_heat") < prob.calls.index("run")
    assert list(res["picard"]["sweeps"]) == [2, 3, 4, 4, 2]
    # one warning, naming the first step that ended at the cap above the tolerance (step 3: 4 sweeps, 5e-6 K)
    msgs = [str(w.message) for w in caught if "picard" in str(w.message)]
    assert len(msgs) == 1 and "step 3" in msgs[0] and "timing.picard_sweeps" in msgs[0] and "timing.picard_tol" in msgs[0]
    # energy for every region, the tabled one included, from the heat records
    np.testing.assert_array_equal(res["monitors"]["ins"]["energy"], np.full(5, float(mesh.material_tags["p_ins"])))
    np.testing.assert_array_equal(res["monitors"]["sample"]["energy"], np.full(5, float(mesh.material_tags["p_sample"])))
    # tangents= and run_batch are refused, naming both
    with pytest.raises(ValueError, match=r"tangents=.*timing\.capacity_form"):
        s.run(cfg, stack, wp, tangents=["p_sample"])
    with pytest.raises(ValueError, match=r"monitor_sigma=.*timing\.capacity_form"):
        s.run(cfg, stack, wp, monitor_sigma={"p_sample": 0.1})
    with pytest.raises(ValueError, match=r"run_batch.*timing\.capacity_form"):
        s.run_batch([cfg, cfg], [stack, stack], wp)


def test_the_driver_under_the_lagged_form_passes_what_it_passed(monkeypatch):
    from conftest import load_cfg

    cfg = load_cfg("geballe_with_diamond_cvT")
    cfg["monitors"] = {"ins": {"material": "p_ins"}, "sample": {"material": "p_sample"}}
    s, cfg, stack, wp, mesh = _session_run(monkeypatch, cfg)
    res = s.run(cfg, stack, wp)
    prob = _StubProblem.made[-1]
    assert not {"capacity_form", "picard_tol", "picard_relax"} & set(prob.kw) and prob.kw["picard"] == 2
    assert "record_heat" not in prob.calls and "picard" not in res
    assert "energy" not in res["monitors"]["ins"] and "energy" in res["monitors"]["sample"]      # omissions as before


def test_used_config_round_trip():
    import yaml

    from conftest import load_cfg
    from heatflow_amd.driver import _with_scheme
    from heatflow_amd.kappa_t import check_capacity_form, material_cv_table

    cfg = _latent_cfg()
    cfg["timing"]["picard_relax"] = 0.5
    out = yaml.safe_load(yaml.safe_dump(_with_scheme(cfg)))
    assert out["timing"]["capacity_form"] == "enthalpy" and out["timing"]["picard_sweeps"] == 32
    assert out["timing"]["picard_tol"] == 1e-6 and out["timing"]["picard_relax"] == 0.5
    assert out["mats"]["p_ins"]["latent"] == cfg["mats"]["p_ins"]["latent"]
    assert check_capacity_form(out) == "enthalpy"
    np.testing.assert_array_equal(out["rhoc_tables"]["p_ins"]["rho_cv"], material_cv_table("p_ins", cfg["mats"]["p_ins"])[2])
    again = _with_scheme(out)                                                  # the file that was written runs the same run
    assert again["rhoc_tables"] == out["rhoc_tables"] and again["timing"] == out["timing"]
    for name in ("geballe_with_diamond", "geballe_with_diamond_cvT"):      # written only when set
        t = _with_scheme(load_cfg(name))["timing"]
        assert not {"capacity_form", "picard_tol", "picard_relax"} & set(t)
    shipped = _with_scheme(load_cfg("geballe_with_diamond_latent"))
    assert shipped["timing"]["capacity_form"] == "enthalpy" and set(shipped["rhoc_tables"]) == {"p_ins", "o_ins", "g_ins"}
