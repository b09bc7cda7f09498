"""Tangents and fits in layer thickness, without a GPU: the velocity fields of the stack builders, the element
derivatives against central differences of the oracle's element matrices on moved coordinates, the restated recursion
(shape_tangent_oracle.py) against central differences of oracle runs on moved meshes, HeatProblem's calls, the parameter names of
the drivers and the fit, and a synthetic fit of p_sample.thickness on the deformed mesh."""
import copy
import json
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest

from aniso_oracle import mixed_multipliers
from conftest import ROOT, load_cfg
from dir_tangent_oracle import directional_element_matrices
from helpers import make_problem, material_tables
from oracle import heat_oracle as ho
from shape_tangent_oracle import FD_REL_STEP, ShapeTangentOracleBackend, shape_element_matrices

NSTEPS = 20
THICKNESS_NAMES = {"geballe_with_diamond": ("p_sample", "p_ins", "o_ins", "p_coupler", "p_diam"),
                   "geballe_no_diamond": ("p_sample", "p_ins", "o_ins", "p_coupler")}


# 1. velocity fields ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(THICKNESS_NAMES))
def test_velocity_moves_the_break_points_as_the_stack_builder_does(name):
    from heatflow_amd.fit import set_params
    from heatflow_amd.geometry import build_stack, thickness_velocity

    cfg = load_cfg(name)
    boxes = [b for m in build_stack(cfg).materials for b in m.boundaries[:2]]
    span = max(boxes) - min(boxes)
    for mat in THICKNESS_NAMES[name]:
        t = float(cfg["mats"][mat]["z"])
        v = thickness_velocity(cfg, mat, np.array(boxes))
        assert np.max(np.abs(v)) > 0
        for rel in (0.05, -0.3):
            moved = set_params(cfg, (f"{mat}.thickness",), (t * (1 + rel),))
            assert float(moved["mats"][mat]["z"]) == t * (1 + rel)
            got = np.array([b for m in build_stack(moved).materials for b in m.boundaries[:2]])
            assert np.max(np.abs(got - (np.array(boxes) + v * t * rel))) <= 1e-14 * span, (mat, rel)
        assert abs(float(thickness_velocity(cfg, mat, 0.0))) <= 1e-14          # the mid-plane stays
        # a function of z alone, piecewise linear: the midpoint of two break points has the mean velocity
        zs = np.unique(boxes)
        mid = 0.5 * (zs[:-1] + zs[1:])
        vz = thickness_velocity(cfg, mat, zs)
        np.testing.assert_allclose(thickness_velocity(cfg, mat, mid), 0.5 * (vz[:-1] + vz[1:]), rtol=0, atol=1e-12)


def test_refused_thickness_names():
    from heatflow_amd.fit import get_param, set_params
    from heatflow_amd.geometry import thickness_velocity

    cfg = load_cfg("geballe_with_diamond")
    for bad in ("gasket", "g_ins", "o_coupler", "o_diam", "nothing"):
        with pytest.raises(ValueError, match=rf"{bad}\.thickness"):
            thickness_velocity(cfg, bad, np.zeros(3))
    with pytest.raises(ValueError, match=r"gasket\.thickness"):
        get_param(cfg, "gasket.thickness")
    with pytest.raises(ValueError, match=r"o_coupler\.thickness"):
        set_params(cfg, ("o_coupler.thickness",), (1e-6,))
    with pytest.raises(ValueError, match=r"p_diam\.thickness"):
        thickness_velocity(load_cfg("geballe_no_diamond"), "p_diam", np.zeros(3))


# 2. element derivatives --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("aniso", [False, True])
def test_element_derivatives_match_central_differences_on_moved_coordinates(case_with_diamond_small, aniso):
    _, _, mesh = case_with_diamond_small
    rng = np.random.default_rng(3)
    coords, tris = mesh.coords, np.asarray(mesh.tris, dtype=np.int64)
    ne = len(tris)
    rho_c, kappa = rng.uniform(1e6, 4e6, ne), rng.uniform(1.0, 400.0, ne)
    m_r = rng.uniform(0.3, 3.0, ne) if aniso else np.ones(ne)
    m_z = rng.uniform(0.3, 3.0, ne) if aniso else np.ones(ne)
    # a random velocity, scaled so that one unit of theta moves a node by at most 5 % of the shortest edge at it
    p = coords[tris]
    edge = np.minimum.reduce([np.linalg.norm(p[:, a] - p[:, b], axis=1) for a, b in ((0, 1), (1, 2), (2, 0))])
    hmin = np.full(len(coords), np.inf)
    np.minimum.at(hmin, tris.ravel(), np.repeat(edge, 3))
    v = rng.uniform(-1.0, 1.0, len(coords)) * 0.05 * hmin
    Md, Kd = shape_element_matrices(coords, tris, rho_c, kappa, m_r, m_z, v)
    h = 1e-3

    def at(step):
        c = coords.copy()
        c[:, 0] += step * v
        if aniso:
            Kr, Kz = directional_element_matrices(c, tris)
            Me = ho.element_matrices(c, tris, rho_c, kappa)[0]
            return Me, (kappa * m_r)[:, None, None] * Kr + (kappa * m_z)[:, None, None] * Kz
        return ho.element_matrices(c, tris, rho_c, kappa)

    (Mp, Kp), (Mm, Km) = at(h), at(-h)
    M0, K0 = at(0.0)
    for what, d, fd, ref in (("Mdot", Md, (Mp - Mm) / (2 * h), M0), ("Kdot", Kd, (Kp - Km) / (2 * h), K0)):
        scale = np.max(np.abs(ref), axis=(1, 2))
        err = np.max(np.abs(d - fd), axis=(1, 2)) / scale
        size = np.max(np.abs(d), axis=(1, 2)) / scale
        print(f"{what} aniso={aniso}: max |d - FD| / max|entry| = {err.max():.2e}; max |d| / max|entry| = {size.max():.2e}")
        # delta is at most ~0.1 here; the central quotient's error is h^2 delta^3-ish, far below 1e-6
        assert size.max() > 1e-2 and err.max() <= 1e-6
    # the closed forms agree with the anisotropic oracle matrices where they must: a rigid velocity gives exact zeros
    Md0, Kd0 = shape_element_matrices(coords, tris, rho_c, kappa, m_r, m_z, np.full(len(coords), 0.7))
    assert not Md0.any() and not Kd0.any()


# 3. the recursion against central differences of oracle runs on moved meshes ----------------------------------------------------------
def _nodes(mesh):
    return np.linspace(0, len(mesh.coords) - 1, 50).astype(np.int32)


def _moved_case(cfg, mesh, name, value, v):
    """(cfg, stack, mesh) with ``name`` set to ``value`` and the nodes moved by v (value - cfg's value): the triangles kept."""
    from heatflow_amd.fit import get_param, set_params
    from heatflow_amd.geometry import build_stack

    c = set_params(cfg, (name,), (value,))
    coords = np.array(mesh.coords, dtype=np.float64)
    coords[:, 0] += v * (value - get_param(cfg, name))
    return c, build_stack(c), SimpleNamespace(coords=coords, tris=mesh.tris, tags=mesh.tags, material_tags=mesh.material_tags)


def _primal_samples(case, aniso, scheme, nodes, nsteps=NSTEPS, tag_to_k=None):
    cfg, stack, mesh = case
    prob = make_problem(cfg, stack, mesh, backend=ShapeTangentOracleBackend(), scheme=scheme, **({"k_aniso": aniso} if aniso else {}))
    if tag_to_k:
        tk, trc = material_tables(stack, mesh)
        prob.set_materials({**tk, **tag_to_k}, trc)
    return prob.run(nsteps, nodes, time_varying=[prob.bcs[3]])[1]


def find_step(fd_error, start=1e-3, bound=1e-4):
    """The issue's rule: the relative step starts at 1e-3 and is halved until the float64 difference is within a quarter of the
    bound.  Returns (step, error at it)."""
    rel = start
    for _ in range(8):
        err = fd_error(rel)
        if err <= 0.25 * bound:
            return rel, err
        rel *= 0.5
    raise AssertionError(f"no step down to {rel:.2e} brings the central difference within {0.25 * bound:.1e} (last {err:.2e})")


@pytest.mark.parametrize("scheme", ["backward_euler", "bdf2"])
@pytest.mark.parametrize("name", ["p_sample.thickness", "p_ins.thickness"])
def test_recursion_matches_central_differences_on_moved_meshes(case_with_diamond_small, name, scheme):
    from heatflow_amd.fit import get_param
    from heatflow_amd.geometry import thickness_velocity

    cfg, stack, mesh = case_with_diamond_small
    nodes = _nodes(mesh)
    v = thickness_velocity(cfg, name.rsplit(".", 1)[0], mesh.coords[:, 0])
    prob = make_problem(cfg, stack, mesh, backend=ShapeTangentOracleBackend(), scheme=scheme)
    _, _, ts, _, _ = prob.run_tangent(NSTEPS, nodes, shape={0: v}, time_varying=[prob.bcs[3]])
    s = ts[:, 0]
    scale = np.max(np.abs(s))
    t0 = get_param(cfg, name)
    assert scale > 0

    def fd_error(rel):
        runs = [_primal_samples(_moved_case(cfg, mesh, name, t0 * (1 + sg * rel), v), None, scheme, nodes) for sg in (1, -1)]
        return float(np.max(np.abs(s - (runs[0] - runs[1]) / (2 * rel * t0))) / scale)

    rel, err = find_step(fd_error)
    print(f"{name} {scheme}: max|s| t = {scale * t0:.3g} K; central difference at relative step {rel:.3g} off by {err:.2e} of max|s|")
    assert rel == FD_REL_STEP[name], "the step the GPU test uses (shape_tangent_oracle.FD_REL_STEP) is the one found here"
    assert err <= 1e-4


@pytest.mark.parametrize("scheme", ["backward_euler", "bdf2"])
def test_a_column_that_is_shape_and_conductivity_is_the_sum_of_both(case_with_diamond_small, scheme):
    """theta moves the thickness of p_sample by v theta and its conductivity by theta W/m/K per metre ... i.e. the column
    d/dtheta = d/dthickness + c d/dk with c = k / t: checked against central differences along that direction, on the anisotropic
    configuration, and against the sum of the two single columns."""
    from heatflow_amd.fit import get_param
    from heatflow_amd.geometry import thickness_velocity

    cfg, stack, mesh = case_with_diamond_small
    aniso = mixed_multipliers(mesh)
    nodes = _nodes(mesh)
    tag = mesh.material_tags["p_sample"]
    t0, k0 = get_param(cfg, "p_sample.thickness"), get_param(cfg, "p_sample")
    c = k0 / t0                                                    # W/m/K per metre of thickness: the two parts comparable
    v = thickness_velocity(cfg, "p_sample", mesh.coords[:, 0])
    prob = make_problem(cfg, stack, mesh, backend=ShapeTangentOracleBackend(), scheme=scheme, k_aniso=aniso)
    # column 0: both (s_t + c s_k needs the loads of v and of c K: the shape part carries v / c and the result is multiplied by c);
    # column 1: the thickness alone; a second set-up: the conductivity alone
    _, _, ts, _, _ = prob.run_tangent(NSTEPS, nodes, conductivity=[[(tag, "k")], []], shape={0: v / c, 1: v / c},
                                      time_varying=[prob.bcs[3]])
    both, t_alone = c * ts[:, 0], c * ts[:, 1]
    prob.set_state(float(cfg["heating"]["ic_temp"]))
    k_alone = c * prob.run_tangent(NSTEPS, nodes, conductivity=[[(tag, "k")]], time_varying=[prob.bcs[3]])[2][:, 0]
    scale = np.max(np.abs(both))
    assert np.max(np.abs(both - (k_alone + t_alone))) <= 1e-12 * (np.max(np.abs(k_alone)) + np.max(np.abs(t_alone)))

    def fd_error(rel):
        runs = []
        for sg in (1, -1):
            case = _moved_case(cfg, mesh, "p_sample.thickness", t0 * (1 + sg * rel), v)
            runs.append(_primal_samples(case, aniso, scheme, nodes, tag_to_k={tag: k0 + c * sg * rel * t0}))
        return float(np.max(np.abs(both - (runs[0] - runs[1]) / (2 * rel * t0))) / scale)

    rel, err = find_step(fd_error)
    print(f"shape + conductivity {scheme}: central difference at relative step {rel:.3g} off by {err:.2e} of max|s|")
    assert scale > 0 and err <= 1e-4


# 4. the Python layers ------------------------------------------------------------------------------------------------------------------
class RecordingBackend(ShapeTangentOracleBackend):
    def __init__(self):
        super().__init__()
        self.calls = []

    def tangent_setup(self, n_par, tag_col):
        self.calls.append(("tangent_setup", n_par, dict(tag_col)))
        super().tangent_setup(n_par, tag_col)

    def tangent_setup_dir(self, n_par, k=None, r=None, z=None):
        self.calls.append(("tangent_setup_dir", n_par, dict(k or {}), dict(r or {}), dict(z or {})))
        super().tangent_setup_dir(n_par, k, r, z)

    def tangent_set_shape(self, j, vz):
        self.calls.append(("tangent_set_shape", j, None if vz is None else np.array(vz)))
        super().tangent_set_shape(j, vz)

    def run_tangent(self, *a, **kw):
        self.calls.append(("run_tangent",))
        return super().run_tangent(*a, **kw)


def test_heat_problem_call_order_with_and_without_shape(case_with_diamond_small):
    cfg, stack, mesh = case_with_diamond_small
    t = mesh.material_tags
    be = RecordingBackend()
    prob = make_problem(cfg, stack, mesh, backend=be)
    nodes = [0, 5]
    v = np.linspace(0.0, 1.0, prob.n)
    # without shape: exactly the calls test_dir_tangent_cpu.py records
    prob.run_tangent(2, nodes, conductivity=[[t["p_coupler"], t["o_coupler"]], [t["gasket"]]])
    assert [c[0] for c in be.calls] == ["tangent_setup", "run_tangent"]
    assert be.calls[0] == ("tangent_setup", 2, {t["p_coupler"]: 0, t["o_coupler"]: 0, t["gasket"]: 1})
    prob.run_tangent(2, nodes, conductivity=[[t["p_coupler"], t["o_coupler"]], [t["gasket"]]])
    assert [c[0] for c in be.calls] == ["tangent_setup", "run_tangent", "run_tangent"]
    # with shape: the set-up, then the velocities in column order, then the run; a second call with the same spec continues
    del be.calls[:]
    prob.run_tangent(2, nodes, conductivity=[[t["gasket"]]], shape={2: 2 * v, 0: v})
    assert [c[:2] for c in be.calls] == [("tangent_setup", 3), ("tangent_set_shape", 0), ("tangent_set_shape", 2), ("run_tangent",)]
    assert be.calls[0][2] == {t["gasket"]: 0} and np.array_equal(be.calls[1][2], v) and np.array_equal(be.calls[2][2], 2 * v)
    prob.run_tangent(2, nodes, conductivity=[[t["gasket"]]], shape={2: 2 * v, 0: v})
    assert [c[0] for c in be.calls[4:]] == ["run_tangent"]
    # other velocities are another spec; a shape-only run makes the set-up of only -1 entries; pairs go to the directional one
    prob.run_tangent(2, nodes, conductivity=[[t["gasket"]]], shape={2: v, 0: v})
    assert [c[0] for c in be.calls[5:]] == ["tangent_setup", "tangent_set_shape", "tangent_set_shape", "run_tangent"]
    del be.calls[:]
    prob.run_tangent(2, nodes, shape={0: v})
    assert be.calls[0] == ("tangent_setup", 1, {}) and be.calls[1][:2] == ("tangent_set_shape", 0)
    prob.run_tangent(2, nodes, conductivity=[[(t["p_ins"], "z")]], shape={0: v})
    assert be.calls[3][:2] == ("tangent_setup_dir", 1) and be.calls[4][:2] == ("tangent_set_shape", 0)
    # dropping the shape is a new set-up (which removes the velocities), not a call that clears them
    del be.calls[:]
    prob.run_tangent(2, nodes, conductivity=[[(t["p_ins"], "z")]])
    assert [c[0] for c in be.calls] == ["tangent_setup_dir", "run_tangent"]
    with pytest.raises(ValueError, match="velocities expected"):
        prob.run_tangent(2, nodes, shape={0: v[:-1]})
    with pytest.raises(ValueError, match="no parameter"):
        prob.run_tangent(2, nodes)


def _session(mesh, backend=None):
    from heatflow_amd.driver import SimulationSession

    return SimulationSession(mesh.coords, mesh.tris, mesh.tags, mesh.material_tags, backend=backend or ShapeTangentOracleBackend(),
                             precond=0)


@pytest.fixture(scope="module")
def small_cfg(case_with_diamond_small):
    cfg = copy.deepcopy(case_with_diamond_small[0])
    cfg["timing"]["num_steps"] = 30
    return cfg


@pytest.mark.parametrize("driver", ["run_with_diamond", "run_no_diamond"])
def test_run_simulation_fills_the_tangents_of_thickness_names(request, tmp_path, driver):
    import importlib

    case = request.getfixturevalue("case_with_diamond_small" if driver == "run_with_diamond" else "case_no_diamond_small")
    cfg, _, mesh = case
    cfg = copy.deepcopy(cfg)
    cfg["timing"]["num_steps"] = 10
    cfg["io"] = dict(cfg.get("io") or {}, output_folder=str(tmp_path / "out"))
    names = ("p_sample.thickness", "p_sample")
    s = _session(mesh)
    try:
        mod = importlib.import_module(f"heatflow_amd.{driver}")
        from heatflow_amd.parameter_sweep import get_watcher_points

        res = mod.run_simulation(cfg, str(tmp_path / "mesh"), output_folder=str(tmp_path / "out"), session=s, tangents=names,
                                 watcher_points=get_watcher_points(cfg), write_xdmf=False, suppress_print=True, read_flux=False)
    finally:
        s.close()
    assert list(res["tangents"]) == list(names)
    for nm in names:
        assert np.max(np.abs(res["tangents"][nm]["oside"])) > 0


def test_session_names_tangent_and_refusals(case_with_diamond_small, small_cfg):
    from heatflow_amd.fit import get_param, set_params
    from heatflow_amd.geometry import build_stack, thickness_velocity
    from heatflow_amd.parameter_sweep import get_watcher_points

    _, _, mesh = case_with_diamond_small
    cfg = small_cfg
    stack, wp = build_stack(cfg), get_watcher_points(cfg)
    s = _session(mesh)
    try:
        names = ["p_sample.thickness", "p_sample", "p_coupler.thickness", "fwhm", "o_ins.thickness"]
        res = s.run(cfg, stack, wp, tangents=names)
        assert list(res["tangents"]) == names and res["tangent_iters"].shape == (30, len(names))
        for nm in names:
            assert np.max(np.abs(res["tangents"][nm]["oside"])) > 0
        for bad in ("gasket.thickness", "o_coupler.thickness"):
            with pytest.raises(ValueError, match=rf"tangents:.*{bad}"):
                s.run(cfg, stack, wp, tangents=[bad])
        with pytest.raises(ValueError, match=r"unknown parameter 'nothing\.thickness'"):
            s.run(cfg, stack, wp, tangents=["nothing.thickness"])
        with pytest.raises(ValueError, match="fifth shape column"):
            s.run(cfg, stack, wp, tangents=[f"{m}.thickness" for m in ("p_sample", "p_ins", "o_ins", "p_coupler", "p_diam")])
        # the whole chain for one name, watchers that move with the interfaces included: set_params -> stack -> moved mesh -> run
        name = "p_sample.thickness"
        t0, rel = get_param(cfg, name), FD_REL_STEP[name]
        v = thickness_velocity(cfg, "p_sample", mesh.coords[:, 0])
        curves = []
        for sg in (1, -1):
            c, st, m = _moved_case(cfg, mesh, name, t0 * (1 + sg * rel), v)
            s2 = _session(m)
            try:
                # (the coupler is one element thick on this mesh: its mid-plane, the watcher point, lies half-way between two
                # nodes and rounding decides which is nearest - the quotient follows the nodes of the unmoved run)
                moved_wp = {nm: tuple(m.coords[i]) for nm, i in zip(*s._watcher_nodes(wp))}
                curves.append(s2.run(c, st, moved_wp)["watchers"]["oside"])
            finally:
                s2.close()
        fd = (curves[0] - curves[1]) / (2 * rel * t0)
        tan = res["tangents"][name]["oside"]
        assert np.max(np.abs(tan - fd)) <= 1e-4 * np.max(np.abs(tan))
    finally:
        s.close()
    c = set_params(cfg, ("p_ins.thickness", "p_sample"), (2.5e-6, 7.0))
    assert c["mats"]["p_ins"]["z"] == 2.5e-6 and get_param(c, "p_ins.thickness") == 2.5e-6 and c["mats"]["p_sample"]["k"] == 7.0
    assert float(cfg["mats"]["p_ins"]["z"]) != 2.5e-6                      # the input is left alone


def test_header_declares_and_backend_lists_the_entry_point():
    from heatflow_amd import hip_backend
    from test_cabi import _declared_symbols

    declared = _declared_symbols()
    assert "hf_tangent_set_shape" in declared and "hf_tangent_set_shape" in hip_backend.EXPORTS
    assert sorted(declared) == sorted(hip_backend.EXPORTS)
    with open(os.path.join(ROOT, "include", "heatflow_hip.h")) as f:
        text = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    assert re.search(r"int\s+hf_tangent_set_shape\(hf_ctx\*\s*ctx,\s*int32_t\s+j,\s*const double\*\s*vz\);", text)
    assert callable(hip_backend.HeatflowHIP.tangent_set_shape)


def _synthetic(cfg, mesh, name, value):
    """Experiment columns of a run at ``name`` = value on the mesh deformed to it."""
    from heatflow_amd.geometry import thickness_velocity
    from heatflow_amd.parameter_sweep import get_watcher_points

    from heatflow_amd.solver import nearest_nodes

    c, st, m = _moved_case(cfg, mesh, name, value, thickness_velocity(cfg, name.rsplit(".", 1)[0], mesh.coords[:, 0]))
    wp = get_watcher_points(cfg)          # the watcher nodes of the unmoved mesh, followed (as the fit follows them)
    nodes = nearest_nodes(mesh.coords, [tuple(p) for p in wp.values()])
    s = _session(m)
    try:
        res = s.run(c, st, {nm: tuple(m.coords[i]) for nm, i in zip(wp, nodes)})
    finally:
        s.close()
    return {"time": res["times"], "temp": res["watchers"]["pside"], "oside": res["watchers"]["oside"]}


def test_fit_recovers_the_sample_thickness_on_the_deformed_mesh(case_with_diamond_small, small_cfg):
    from heatflow_amd.fit import fit_parameters, get_param

    _, _, mesh = case_with_diamond_small
    cfg = small_cfg
    t0 = get_param(cfg, "p_sample.thickness")
    exp = _synthetic(cfg, mesh, "p_sample.thickness", 1.1 * t0)
    out = fit_parameters(cfg, None, ("p_sample.thickness",), exp, x0=[t0], max_iter=40, backend=ShapeTangentOracleBackend(),
                         mesh=(mesh.coords, mesh.tris, mesh.tags, mesh.material_tags))
    print(f"fit of p_sample.thickness: {out['values'][0] / (1.1 * t0) - 1:.2e} off, {out['iterations']} iterations, "
          f"{out['runs']} runs, rmse {out['rmse']:.2e}")
    assert abs(out["values"][0] / (1.1 * t0) - 1) <= 1e-6, out["history"]
    assert out["converged"] and out["rmse"] < 1e-8 and np.isfinite(out["stderr"][0])
    assert out["params"] == ["p_sample.thickness"] and out["deformed_mesh"] is True


def test_fit_cli_writes_the_fitted_thickness(case_with_diamond_small, small_cfg, tmp_path):
    import yaml

    from heatflow_amd.fit import get_param, main

    cfg = copy.deepcopy(small_cfg)
    path = tmp_path / "cfg.yaml"
    path.write_text(yaml.safe_dump(cfg))
    out_dir = tmp_path / "out"
    assert main(["--config", str(path), "--params", "p_sample.thickness", "fwhm", "--output-dir", str(out_dir), "--max-iter", "2"],
                backend=ShapeTangentOracleBackend()) == 0
    summary = json.loads((out_dir / "fit_summary.json").read_text())
    assert summary["params"] == ["p_sample.thickness", "fwhm"] and len(summary["values"]) == 2 and summary["deformed_mesh"] is True
    used = yaml.safe_load((out_dir / "used_config.yaml").read_text())
    assert get_param(used, "p_sample.thickness") == pytest.approx(summary["values"][0], rel=1e-12)
    assert float(used["mats"]["p_sample"]["z"]) == pytest.approx(summary["values"][0], rel=1e-12)
    assert used["heating"]["fwhm"] == pytest.approx(summary["values"][1], rel=1e-12)
    assert float(used["mats"]["p_ins"]["z"]) == float(cfg["mats"]["p_ins"]["z"])
