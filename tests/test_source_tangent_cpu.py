"""Tangents under the laser-power source without a GPU: the restated derivative vectors G_f, G_d and the
coefficient table against central differences, power conservation, the restated recursion against central differences of restated
runs (where FD_REL_STEP is found), get_param / set_params, the ``tangents`` key and used_config, every new ValueError, and the
driver and the fit on the scipy stand-in: their call order, and that without the key the backend sees no new call."""
import copy
import functools
import math

import numpy as np
import pytest

import source_oracle as so
import source_tangent_oracle as sto
from conftest import build_case, load_cfg

from heatflow_amd import source as src_mod

CASES = {"with_diamond": "geballe_with_diamond", "no_diamond": "geballe_no_diamond"}
KEY = {"source.power": "power", "source.fwhm": "fwhm", "source.depth": "depth", "source.pulse.t0": "t0", "source.pulse.fwhm": "w"}
KEPT = dict(names=("p_coupler", "p_ins"), depth=5.0e-7, power=0.5)      # as tests/test_gpu_source.py's KEPT_LINE_*
FD_TOL = 1e-4


@functools.lru_cache(maxsize=None)
def small(which):
    return build_case(CASES[which], 8.0)


def _vectors(case, P):
    _, _, mesh = case
    tags = [mesh.material_tags[n] for n in P["names"]]
    F1 = so.source_vector(mesh.coords, mesh.tris, mesh.tags, tags, P["fwhm"], P["z0"], P["depth"])[0]
    Gf, Tf, Gd, Td = sto.derivative_vectors(mesh.coords, mesh.tris, mesh.tags, tags, P["fwhm"], P["z0"], P["depth"])
    return F1, Gf, Tf, Gd, Td


# ---- G_f, G_d --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which, kw", [("with_diamond", {}), ("with_diamond", KEPT), ("no_diamond", {}), ("no_diamond", KEPT)])
def test_restated_derivative_vectors_match_central_differences_of_the_restated_source_vector(which, kw):
    """F1 is smooth in fwhm and depth: a central difference at the relative step h has the truncation error h^2 theta^2 F1''' / 6,
    about h^2 |G| theta-independent factors of order 10, so h = 1e-4 leaves 1e-7 of the row's scale."""
    case = small(which)
    P = sto.beam(case, **kw)
    F1, Gf, Tf, Gd, Td = _vectors(case, P)
    for key, G, T in (("fwhm", Gf, Tf), ("depth", Gd, Td)):
        h = 1e-4 * P[key]
        Fp = _vectors(case, dict(P, **{key: P[key] + h}))[0]
        Fm = _vectors(case, dict(P, **{key: P[key] - h}))[0]
        fd = (Fp - Fm) / (2.0 * h)
        scale = np.abs(G).max()
        err = np.abs(G - fd).max() / scale
        print(f"{which} {P['names']} d/d{key}: |G - FD| / max|G| = {err:.2e}")
        assert scale > 0.0 and err <= 1e-6
        assert np.all(G[T == 0.0] == 0.0) and np.all(G[F1 == 0.0] == 0.0)
    uniform = _vectors(case, dict(P, depth=math.inf))
    assert not uniform[3].any() and uniform[1].any()                       # a uniform layer: G_d is exactly zero


# ---- the coefficient table -------------------------------------------------------------------------------------------------------
def _spec(P, **over):
    cfg = copy.deepcopy(load_cfg("geballe_with_diamond"))
    block = {"material": list(P["names"]), "power": P["power"], "fwhm": P["fwhm"], "pulse": {"t0": P["t0"], "fwhm": P["w"]},
             "tangents": True}
    if math.isfinite(P["depth"]):
        block["depth"] = P["depth"]
    block.update(over)
    cfg["heating"]["source"] = block
    return src_mod.parse_source(cfg)


@pytest.mark.parametrize("kw", [{}, KEPT])
def test_coefficient_table_matches_central_differences_of_the_amplitudes_and_conserves_the_power(kw):
    case = small("with_diamond")
    P = sto.beam(case, **kw)
    F1, Gf, _, Gd, _ = _vectors(case, P)
    times = (np.arange(sto.NSTEPS) + 1) * 7.5e-8
    table = src_mod.tangent_coefficients(_spec(P), src_mod.SOURCE_PARAMS, times, F1, Gf, Gd)
    restated = sto.coefficient_table(P["power"], P["t0"], P["w"], times, F1, Gf, Gd)
    assert list(table) == list(src_mod.SOURCE_PARAMS) == list(sto.SOURCE_PARAMS)
    for nm in table:
        assert table[nm].shape == (sto.NSTEPS, 3)
        assert np.allclose(table[nm], restated[nm], rtol=1e-13, atol=0.0), nm

    def load(Q):                                                           # p_k F1 of every step, n_steps x n
        F = _vectors(case, Q)[0]
        return src_mod.amplitudes(_spec(Q), times, F)[:, None] * F[None, :]

    for nm, c in table.items():
        key, h = KEY[nm], 1e-4 * P[KEY[nm]]
        fd = (load(dict(P, **{key: P[key] + h})) - load(dict(P, **{key: P[key] - h}))) / (2.0 * h)
        got = c[:, 0, None] * F1 + c[:, 1, None] * Gf + c[:, 2, None] * Gd
        err = np.abs(got - fd).max() / np.abs(got).max()
        print(f"{nm}: |c0 F1 + c1 G_f + c2 G_d - FD of p_k F1| / max = {err:.2e}")
        assert err <= 1e-6, nm
    # the configured power stays the discrete power: the fwhm and depth columns add no net load, within rounding
    for nm in ("source.fwhm", "source.depth"):
        c = table[nm][9]
        terms = np.concatenate([c[0] * F1, c[1] * Gf, c[2] * Gd])
        assert abs(math.fsum(terms)) <= 1e-13 * math.fsum(np.abs(terms)), nm
    # a file pulse has no pulse parameters, a uniform layer no depth, and nothing is a parameter without a source
    with pytest.raises(ValueError, match=r"source\.depth: the source has no depth"):
        src_mod.tangent_coefficients(_spec(dict(P, depth=math.inf)), ["source.depth"], times, F1, Gf, Gd)
    with pytest.raises(ValueError, match=r"source\.pulse\.t0: the pulse comes from a file"):
        src_mod.check_source_param(_spec(P, pulse={"file": "x.csv"}), "source.pulse.t0")
    with pytest.raises(ValueError, match=r"source\.power: the configuration has no volumetric source"):
        src_mod.check_source_param(None, "source.power")
    with pytest.raises(ValueError, match=r"source\.colour: unknown source parameter"):
        src_mod.check_source_param(_spec(P), "source.colour")


# ---- the recursion -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("keep_line", [False, True])
@pytest.mark.parametrize("scheme", ["backward_euler", "bdf2"])
def test_restated_recursion_matches_central_differences_of_restated_runs(scheme, keep_line):
    """The step rule of DESIGN.md 3.15: start at 1e-3, halve until the float64 difference is within a quarter of 1e-4 of max|s|;
    the step it finds is the one recorded in FD_REL_STEP (and the GPU test uses)."""
    case = small("with_diamond")
    _, _, mesh = case
    nodes = np.arange(len(mesh.coords), dtype=np.int32)
    P = sto.beam(case, **(KEPT if keep_line else {}))
    prob = sto.problem(case, P, keep_line, backend=sto.SourceTangentOracleBackend(), scheme=scheme)
    names, _, s, ts, _ = sto.tangent_run(prob, case, P, nodes, keep_line=keep_line)
    assert s.max() - 300.0 >= 10.0
    for j, nm in enumerate(names):
        if nm not in KEY:
            continue
        rel = 1e-3
        while True:
            runs = []
            for sg in (1.0, -1.0):
                Q = dict(P, **{KEY[nm]: P[KEY[nm]] * (1.0 + sg * rel)})
                runs.append(sto.primal_run(sto.problem(case, Q, keep_line, backend=sto.SourceTangentOracleBackend(), scheme=scheme),
                                           Q, nodes, keep_line=keep_line)[1])
            fd = (runs[0] - runs[1]) / (2.0 * rel * P[KEY[nm]])
            scale = np.abs(ts[:, j]).max()
            err = np.abs(ts[:, j] - fd).max() / scale
            if err <= 0.25 * FD_TOL or rel < 1e-5:
                break
            rel *= 0.5
        print(f"{scheme} keep_line={keep_line} {nm}: relative step {rel:g}, |s - FD| / max|s| = {err:.2e}, max|s| theta = "
              f"{scale * P[KEY[nm]]:.3g} K")
        assert scale > 0.0 and err <= 0.25 * FD_TOL
        assert rel == sto.FD_REL_STEP[nm], "the step recorded in FD_REL_STEP is the one the rule finds"


# ---- get_param / set_params ----------------------------------------------------------------------------------------------------------
def _source_cfg(tangents=True, **over):
    cfg = copy.deepcopy(load_cfg("geballe_with_diamond"))
    cfg["mats"] = {k: dict(v, mesh=float(v["mesh"]) * 8.0) for k, v in cfg["mats"].items()}
    block = {"material": "p_coupler", "power": 0.2, "depth": 2.0e-8, "pulse": {"t0": 7.5e-7, "fwhm": 6.0e-7}}
    if tangents is not None:
        block["tangents"] = tangents
    block.update(over)
    cfg["heating"]["source"] = {k: v for k, v in block.items() if v is not None}
    cfg["timing"] = dict(cfg["timing"], num_steps=sto.NSTEPS, t_final=sto.NSTEPS * 7.5e-8)
    return cfg


def test_get_param_and_set_params_know_the_source_names():
    from heatflow_amd.fit import get_param, set_params

    cfg = _source_cfg()
    assert get_param(cfg, "source.power") == 0.2 and get_param(cfg, "source.depth") == 2.0e-8
    assert get_param(cfg, "source.fwhm") == 1.32e-5                         # heating.fwhm: the block has none
    assert get_param(cfg, "source.pulse.t0") == 7.5e-7 and get_param(cfg, "source.pulse.fwhm") == 6.0e-7
    names = list(src_mod.SOURCE_PARAMS)
    c = set_params(cfg, names + ["p_sample"], [0.3, 1.0e-5, 3.0e-8, 8.0e-7, 5.0e-7, 4.0])
    assert [get_param(c, nm) for nm in names] == [0.3, 1.0e-5, 3.0e-8, 8.0e-7, 5.0e-7] and c["mats"]["p_sample"]["k"] == 4.0
    assert c["heating"]["source"]["fwhm"] == 1.0e-5 and c["heating"]["fwhm"] == 1.32e-5      # written explicitly, the line's stays
    assert "fwhm" not in cfg["heating"]["source"] and cfg["heating"]["source"]["power"] == 0.2      # the input is not touched
    with pytest.raises(ValueError, match=r"source\.depth: the source has no depth"):
        get_param(_source_cfg(depth=None), "source.depth")
    with pytest.raises(ValueError, match=r"source\.pulse\.fwhm: the pulse comes from a file"):
        set_params(_source_cfg(pulse={"file": "x.csv"}), ["source.pulse.fwhm"], [1.0])
    with pytest.raises(ValueError, match=r"source\.power: the configuration has no volumetric source"):
        get_param(load_cfg("geballe_with_diamond"), "source.power")


# ---- the key ---------------------------------------------------------------------------------------------------------------------
def test_the_tangents_key_parses_and_used_config_writes_it_only_when_true():
    from heatflow_amd.driver import _with_scheme

    assert "tangents" in src_mod.SOURCE_KEYS
    assert src_mod.parse_source(_source_cfg()).tangents is True
    assert src_mod.parse_source(_source_cfg(tangents=False)).tangents is False
    assert src_mod.parse_source(_source_cfg(tangents=None)).tangents is False
    for bad in ("yes", 1, 0.0, "true"):
        with pytest.raises(ValueError, match=r"heating\.source\.tangents must be true or false"):
            src_mod.parse_source(_source_cfg(tangents=bad))
    assert _with_scheme(_source_cfg())["heating"]["source"]["tangents"] is True
    assert "tangents" not in _with_scheme(_source_cfg(tangents=False))["heating"]["source"]
    assert "tangents" not in _with_scheme(_source_cfg(tangents=None))["heating"]["source"]
    assert "tangents" not in _with_scheme(load_cfg("geballe_with_diamond_source"))["heating"]["source"]
    assert src_mod.source_permits_tangents(_source_cfg()) and not src_mod.source_permits_tangents(_source_cfg(tangents=False))
    assert not src_mod.source_permits_tangents(load_cfg("geballe_with_diamond"))
    src_mod.refuse_source_tangents(_source_cfg(), "x")                    # permitted
    src_mod.refuse_source_tangents(load_cfg("geballe_with_diamond"), "x")    # no source: nothing to refuse
    with pytest.raises(ValueError, match=r"x does not support the volumetric source \(heating\.source\)"):
        src_mod.refuse_source_tangents(_source_cfg(tangents=False), "x")
    shipped, plain = load_cfg("geballe_with_diamond_source_tangents"), load_cfg("geballe_with_diamond_source")
    assert src_mod.parse_source(shipped).tangents is True and "coupler" in shipped["monitors"]
    block = dict(shipped["heating"]["source"])
    assert block.pop("tangents") is True and block == plain["heating"]["source"] and shipped["mats"] == plain["mats"]


# ---- the driver and the fit on the stand-in ------------------------------------------------------------------------------------------
MONITORS = {"coupler": {"material": "p_coupler", "above": 320.0}, "cell": {"material": ["p_sample", "p_ins", "p_coupler"]}}


def _session(mesh, backend=None):
    from heatflow_amd.driver import SimulationSession

    return SimulationSession(mesh.coords, mesh.tris, mesh.tags, mesh.material_tags,
                             backend=backend or sto.SourceMonitorOracleBackend(), precond=0)


def test_every_new_value_error_names_its_parameter():
    from heatflow_amd import fit
    from heatflow_amd.geometry import build_stack
    from heatflow_amd.parameter_sweep import get_watcher_points

    _, _, mesh = small("with_diamond")
    cfg = _source_cfg()
    stack, wp = build_stack(cfg), get_watcher_points(cfg)
    be = sto.SourceMonitorOracleBackend()
    s = _session(mesh, be)
    plain = copy.deepcopy(cfg)
    del plain["heating"]["source"]
    for c, names, pat in (
            (_source_cfg(depth=None), ["source.depth"], r"tangents: source\.depth: the source has no depth"),
            (_source_cfg(pulse={"file": "x.csv"}), ["source.pulse.t0"], r"tangents: source\.pulse\.t0: the pulse comes from a file"),
            (_source_cfg(pulse={"file": "x.csv"}), ["source.pulse.fwhm"], r"tangents: source\.pulse\.fwhm: the pulse comes from a file"),
            (plain, ["source.power"], r"tangents: source\.power: the configuration has no volumetric source"),
            (plain, ["p_sample", "source.fwhm"], r"tangents: source\.fwhm: the configuration has no volumetric source"),
            (cfg, ["source.width"], r"tangents: source\.width: unknown source parameter"),
            (cfg, ["p_ins.thickness"], r"tangents: parameter 'p_ins\.thickness': a layer thickness under a volumetric source"),
            (cfg, ["fwhm"], r"tangents: parameter 'fwhm': the heated line is off \(heating\.source\.keep_line: false\)"),
            (_source_cfg(tangents=False), ["source.power"], r"tangents=.*heating\.source"),
            (_source_cfg(tangents=None), ["p_sample"], r"tangents=.*heating\.source")):
        with pytest.raises(ValueError, match=pat):
            s.run(c, build_stack(c), wp, tangents=names)
    assert getattr(be, "source_calls", []) == [] and be.set_mesh_calls == 0       # every refusal comes before any backend call
    with pytest.raises(ValueError, match="tangents: not combined with a field sink or the read-flux projection"):
        s.run(cfg, stack, wp, tangents=["source.power"], field_sink=lambda t, u: None)
    with pytest.raises(ValueError, match=r"two_sided=True.*heating\.source"):
        s.run(cfg, stack, wp, tangents=["source.power"], two_sided=True)
    s.close()
    with pytest.raises(ValueError, match=r"'source\.power' cannot be fitted.*identically zero"):
        fit.fit_parameters(cfg, "unused", params=("p_sample", "source.power"))
    with pytest.raises(ValueError, match=r"heatflow_amd\.fit does not support the volumetric source"):
        fit.fit_parameters(_source_cfg(tangents=False), "unused")
    with pytest.raises(ValueError, match=r"nuisance 'source\.depth': source\.depth: the source has no depth"):
        fit.fit_parameters(_source_cfg(depth=None), "unused", nuisance={"source.depth": 0.1})
    with pytest.raises(ValueError, match=r"source\.fwhm: the configuration has no volumetric source"):
        fit.fit_parameters(plain, "unused", params=("source.fwhm",))
    # HeatProblem
    case = small("with_diamond")
    P = sto.beam(case)
    prob = sto.problem(case, P, False, backend=sto.SourceTangentOracleBackend())
    t = mesh.material_tags
    with pytest.raises(ValueError, match="source_amplitude needs source="):
        prob.run_tangent(2, None, conductivity=[[t["p_sample"]]], source_amplitude=[1.0, 1.0])
    with pytest.raises(ValueError, match="shape columns under a source are not supported"):
        prob.run_tangent(2, None, conductivity=[[t["p_sample"]]], source={}, shape={0: np.zeros(prob.n)})
    with pytest.raises(ValueError, match=r"source column 0: unknown key 'power' \(amplitude, fwhm, depth\)"):
        prob.run_tangent(2, None, source={0: {"power": [1.0, 1.0]}})
    with pytest.raises(ValueError, match="2 values expected, got 3"):
        prob.run_tangent(2, None, source={0: {"amplitude": [1.0, 1.0, 1.0]}})
    with pytest.raises(ValueError, match="'fwhm' or 'depth' expected"):
        prob.source_derivative("power")
    from helpers import make_problem
    cfg0, stack0, _ = case
    bare = make_problem(cfg0, stack0, mesh, backend=sto.SourceTangentOracleBackend())
    with pytest.raises(ValueError, match=r"source= needs a source"):
        bare.run_tangent(2, None, conductivity=[[t["p_sample"]]], source={})
    with pytest.raises(ValueError, match="the problem has no source"):
        bare.source_derivative("fwhm")


def test_without_the_key_the_backend_sees_no_new_call_and_with_it_the_calls_come_in_order():
    from heatflow_amd.geometry import build_stack
    from heatflow_amd.parameter_sweep import get_watcher_points

    _, _, mesh = small("with_diamond")
    new_calls = {"source_derivatives", "get_source_derivative", "tangent_set_source"}
    # no key: a primal run under the source, as before
    cfg = _source_cfg(tangents=None)
    be = sto.SourceMonitorOracleBackend()
    s = _session(mesh, be)
    s.run(cfg, build_stack(cfg), get_watcher_points(cfg))
    assert be.source_calls == ["set_source", "get_source", "set_source_amplitudes"] and not new_calls & set(be.source_calls)
    s.close()
    # the key alone changes nothing either
    cfg = _source_cfg()
    be = sto.SourceMonitorOracleBackend()
    s = _session(mesh, be)
    primal = s.run(cfg, build_stack(cfg), get_watcher_points(cfg))
    assert be.source_calls == ["set_source", "get_source", "set_source_amplitudes"]
    # conductivity and capacity columns only: the source becomes differentiable, and no column table is set
    del be.source_calls[:]
    res = s.run(cfg, build_stack(cfg), get_watcher_points(cfg), tangents=["p_sample", "p_sample.rho_c"])
    assert be.source_calls == ["source_derivatives", "set_source_amplitudes"]
    for nm in ("pside", "oside"):
        assert np.array_equal(res["watchers"][nm], primal["watchers"][nm])
    # source columns: the derivative vectors are read back once per problem, the table is set for every run
    del be.source_calls[:]
    names = ["p_sample"] + list(src_mod.SOURCE_PARAMS)
    res = s.run(cfg, build_stack(cfg), get_watcher_points(cfg), tangents=names)
    assert be.source_calls == ["get_source_derivative", "get_source_derivative", "set_source_amplitudes", "tangent_set_source"]
    del be.source_calls[:]
    s.run(cfg, build_stack(cfg), get_watcher_points(cfg), tangents=names)
    assert be.source_calls == ["set_source_amplitudes", "tangent_set_source"]
    assert list(res["tangents"]) == names
    for nm in names:
        assert np.abs(res["tangents"][nm]["pside"]).max() > 0.0, nm
    # linear in the power: d u / d power = (u - ic) / power
    rise = primal["watchers"]["pside"] - 300.0
    assert rise.max() > 10.0 and np.allclose(res["tangents"]["source.power"]["pside"] * 0.2, rise, rtol=1e-9, atol=1e-9 * rise.max())
    s.close()


def test_session_tangents_match_central_differences_and_monitor_sigma_writes_bands(tmp_path):
    import importlib

    from heatflow_amd.fit import get_param, set_params
    from heatflow_amd.geometry import build_stack
    from heatflow_amd.parameter_sweep import get_watcher_points

    _, _, mesh = small("with_diamond")
    cfg = _source_cfg()
    cfg["monitors"] = copy.deepcopy(MONITORS)
    wp = get_watcher_points(cfg)
    sigma = {"source.power": 0.05, "source.fwhm": 0.1, "p_sample.rho_c": 0.15}
    mod = importlib.import_module("heatflow_amd.run_with_diamond")
    s = _session(mesh)
    try:
        res = mod.run_simulation(cfg, str(tmp_path / "mesh"), output_folder=str(tmp_path / "out"), session=s,
                                 tangents=list(src_mod.SOURCE_PARAMS), monitor_sigma=sigma, watcher_points=wp, write_xdmf=False,
                                 suppress_print=True)
        band, mt, m = res["monitor_uncertainty"], res["monitor_tangents"], res["monitors"]
        assert (tmp_path / "out" / "monitor_uncertainty.csv").is_file()
        tmax = band["coupler"]["T_max"]
        assert np.all(np.isfinite(tmax)) and tmax.max() > 0.0
        want = np.sqrt(sum((mt[q]["coupler"]["T_max"] * sg * get_param(cfg, q)) ** 2 for q, sg in sigma.items()))
        assert np.allclose(tmax, want, rtol=1e-14, atol=0.0)
        # d energy / d power = energy / power over the whole cell's monitored part while the outer edges stay at ic_temp
        e = m["cell"]["energy"]
        assert e.max() > 0.0 and np.allclose(mt["source.power"]["cell"]["energy"] * 0.2, e, rtol=1e-9, atol=1e-9 * e.max())
        for nm in src_mod.SOURCE_PARAMS:
            rel = sto.FD_REL_STEP[nm]
            sides = []
            for sg in (1.0, -1.0):
                c = set_params(cfg, (nm,), (get_param(cfg, nm) * (1.0 + sg * rel),))
                sides.append(s.run(c, build_stack(c), wp))
            for w in ("pside", "oside"):
                d = res["tangents"][nm][w]
                fd = (sides[0]["watchers"][w] - sides[1]["watchers"][w]) / (2.0 * rel * get_param(cfg, nm))
                assert np.abs(d - fd).max() <= FD_TOL * np.abs(d).max(), (nm, w)
            d = mt[nm]["coupler"]["T_mean"]
            fd = (sides[0]["monitors"]["coupler"]["T_mean"] - sides[1]["monitors"]["coupler"]["T_mean"]) / (2.0 * rel * get_param(cfg, nm))
            assert np.abs(d - fd).max() <= FD_TOL * np.abs(d).max(), nm
    finally:
        s.close()


def test_fit_recovers_p_sample_under_a_source_with_a_nuisance_budget():
    """Synthetic data made by the stand-in at 1.1 k; the fit starts at k and comes back to 1.1 k; the budget is finite."""
    from heatflow_amd import fit
    from heatflow_amd.geometry import build_stack
    from heatflow_amd.parameter_sweep import get_watcher_points

    _, _, mesh = small("with_diamond")
    cfg = _source_cfg()
    k0 = float(cfg["mats"]["p_sample"]["k"])
    truth = fit.set_params(cfg, ("p_sample",), (1.1 * k0,))
    s = _session(mesh, sto.SourceTangentOracleBackend())
    try:
        res = s.run(truth, build_stack(truth), get_watcher_points(truth))
        ps, os_ = res["watchers"]["pside"], res["watchers"]["oside"]
        exp = {"time": res["times"], "temp": ps, "oside": os_}
        out = fit.fit_parameters(cfg, "unused", ("p_sample",), exp, session=s, max_iter=40, xtol=1e-13, ftol=1e-16,
                                 nuisance={"source.fwhm": 0.1, "source.depth": 0.2})
    finally:
        s.close()
    print(f"fit under a source: {out['values'][0]:.8f} (truth {1.1 * k0:.8f}), iterations {out['iterations']}, "
          f"systematic {out['systematic']}")
    assert out["converged"] and abs(out["values"][0] - 1.1 * k0) <= 1e-5 * 1.1 * k0
    assert set(out["systematic"]) == {"source.fwhm", "source.depth"}
    assert np.isfinite(out["systematic_total"]["p_sample"]) and out["systematic_total"]["p_sample"] > 0.0


def test_the_lines_fwhm_column_carries_the_beams_term_where_the_block_has_no_fwhm():
    """keep_line: true and no heating.source.fwhm: heating.fwhm is the width of the heated line and of the beam, so the ``fwhm``
    column has the line's boundary derivative and the source.fwhm load; with a width of its own the beam stays out of it."""
    from heatflow_amd.fit import get_param, set_params
    from heatflow_amd.geometry import build_stack
    from heatflow_amd.parameter_sweep import get_watcher_points

    _, _, mesh = small("with_diamond")
    rel = sto.FD_REL_STEP["source.fwhm"]
    for own_width in (False, True):
        cfg = _source_cfg(keep_line=True, material=["p_coupler", "p_ins"], depth=5.0e-7, power=0.5,
                          fwhm=1.32e-5 if own_width else None)
        wp = get_watcher_points(cfg)
        be = sto.SourceMonitorOracleBackend()
        s = _session(mesh, be)
        try:
            res = s.run(cfg, build_stack(cfg), wp, tangents=["fwhm"])
            assert ("tangent_set_source" in be.source_calls) == (not own_width)
            sides = []
            for sg in (1.0, -1.0):
                c = set_params(cfg, ("fwhm",), (get_param(cfg, "fwhm") * (1.0 + sg * rel),))
                sides.append(s.run(c, build_stack(c), wp))
        finally:
            s.close()
        d = res["tangents"]["fwhm"]["oside"]      # (the p-side watcher sits on the heated line at r = 0, where nothing moves)
        fd = (sides[0]["watchers"]["oside"] - sides[1]["watchers"]["oside"]) / (2.0 * rel * get_param(cfg, "fwhm"))
        assert np.abs(d).max() > 0.0 and np.abs(d - fd).max() <= FD_TOL * np.abs(d).max(), own_width
