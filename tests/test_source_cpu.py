"""Laser-power heating without a GPU: the restated source vector F1 (its exact sum for s = 1 and its h^2 convergence to a
high-order quadrature of the true source), the amplitudes (Gaussian and CSV pulses, the W -> W/m^3 normalisation), the
``heating.source`` block (parsing, defaults, face, used_config.yaml, the three-edge boundary set), every Python refusal,
HeatProblem's call order, the session end to end on a scipy stand-in, and the header against EXPORTS."""
import copy
import dataclasses
import math
import os
import re

import numpy as np
import pytest

import source_oracle as so
from conftest import ROOT, build_case, load_cfg
from helpers import material_tables
from oracle_backend import OracleBackend

from heatflow_amd import source as src_mod


@pytest.fixture(scope="module")
def small():
    return build_case("geballe_with_diamond", 8.0)


def _source_cfg(**over):
    cfg = copy.deepcopy(load_cfg("geballe_with_diamond"))
    block = {"material": "p_coupler", "power": 0.2, "pulse": {"t0": 7.5e-7, "fwhm": 6.0e-7}}
    block.update(over)
    cfg["heating"]["source"] = {k: v for k, v in block.items() if v is not None}
    return cfg


def _small_cfg(cfg):
    cfg["mats"] = {k: dict(v, mesh=float(v["mesh"]) * 8.0) for k, v in cfg["mats"].items()}
    return cfg


# ---- F1 -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("names", [("p_coupler",), ("p_coupler", "p_ins"), ("gasket",)])
def test_unit_shape_sums_to_the_r_weighted_area(small, names):
    """s = 1 (a huge fwhm, depth = inf): sum_i F1_i = sum_e area_e (r_0 + r_1 + r_2) / 3, exact for the r-weighted P1 mass."""
    _, _, mesh = small
    tags = [mesh.material_tags[n] for n in names]
    F1, scale = so.source_vector(mesh.coords, mesh.tris, mesh.tags, tags, 1e30, 0.0, math.inf)
    sel = np.isin(mesh.tags, tags)
    p = mesh.coords[mesh.tris[sel]]
    d = (p[:, 1, 0] - p[:, 0, 0]) * (p[:, 2, 1] - p[:, 0, 1]) - (p[:, 2, 0] - p[:, 0, 0]) * (p[:, 1, 1] - p[:, 0, 1])
    want = math.fsum(0.5 * np.abs(d) * p[:, :, 1].sum(axis=1) / 3.0)
    got = math.fsum(F1)
    assert abs(got - want) <= 1e-13 * want, (got, want)
    touched = np.zeros(len(mesh.coords), dtype=bool)
    touched[mesh.tris[sel].ravel()] = True
    assert np.all(F1[~touched] == 0.0) and np.all(F1[touched] > 0.0) and np.array_equal(F1, scale)


def _grid(nz, nr, Lz=2.0, Lr=1.0):
    """A structured triangulation of [0, Lz] x [0, Lr]; tag 1 for z < Lz / 2 (the grid resolves the interface), tag 2 beyond."""
    z, r = np.meshgrid(np.linspace(0.0, Lz, nz + 1), np.linspace(0.0, Lr, nr + 1), indexing="ij")
    coords = np.stack([z.ravel(), r.ravel()], axis=1)
    idx = np.arange((nz + 1) * (nr + 1)).reshape(nz + 1, nr + 1)
    a, b, c, d = idx[:-1, :-1].ravel(), idx[1:, :-1].ravel(), idx[1:, 1:].ravel(), idx[:-1, 1:].ravel()
    tris = np.concatenate([np.stack([a, b, c], axis=1), np.stack([a, c, d], axis=1)])
    zc = coords[tris][:, :, 0].mean(axis=1)
    return coords, tris, np.where(zc < Lz / 2, 1, 2)


def test_restated_vector_converges_to_the_quadrature_of_the_true_source_as_h_squared():
    """F1 interpolates s in every absorbing element: against int s phi_i r by a high-order rule the summed difference falls as
    h^2 (a factor 4 per refinement; a wrong r-weight or a wrong tag mask leaves a difference that does not fall at all)."""
    fwhm, z0, depth = 0.9, 0.0, 0.4

    def shape(z, r):
        return np.exp(-4.0 * math.log(2.0) * r * r / fwhm ** 2) * np.exp(-np.abs(z - z0) / depth)

    errs, total = [], None
    for nz in (8, 16, 32):
        coords, tris, tags = _grid(nz, nz // 2)
        F1, _ = so.source_vector(coords, tris, tags, [1], fwhm, z0, depth)
        ref = so.quadrature_load(coords, tris, tags, [1], shape, levels=2)
        errs.append(np.abs(F1 - ref).sum())
        total = ref.sum()
        assert np.all(F1[coords[:, 0] > 1.0 + 1e-12] == 0.0)                 # nothing beyond the material boundary
    print("h^2 convergence: relative l1 differences", [e / total for e in errs])
    assert 3.0 <= errs[0] / errs[1] <= 5.0 and 3.0 <= errs[1] / errs[2] <= 5.0, errs
    # the exact integral of the true source over the absorbing half: the sum of the reference approaches it
    c = 4.0 * math.log(2.0) / fwhm ** 2
    exact = (1.0 - math.exp(-c)) / (2.0 * c) * depth * (1.0 - math.exp(-1.0 / depth))
    assert abs(total - exact) <= 1e-5 * exact


def test_shape_of_the_restatement():
    zr = np.array([[0.0, 0.0], [0.0, 0.5], [2.0, 0.0], [-2.0, 1.0]])
    s = so.source_shape(zr, 1.0, 0.0, math.inf)
    assert s[0] == 1.0 and abs(s[1] - 0.5) < 1e-15 and s[2] == 1.0 and abs(s[3] - 1.0 / 16.0) < 1e-15
    s = so.source_shape(zr, 1.0, 2.0, 1.0)
    assert abs(s[2] - 1.0) < 1e-15 and abs(s[0] - math.exp(-2.0)) < 1e-15 and abs(s[3] - math.exp(-4.0) / 16.0) < 1e-15


# ---- amplitudes -------------------------------------------------------------------------------------------------------------
def test_gaussian_pulse_csv_pulse_and_the_power_normalisation(small, tmp_path):
    _, stack, mesh = small
    spec = src_mod.parse_source(_source_cfg())
    times = (np.arange(20) + 1) * 7.5e-8
    pulse = src_mod.pulse_values(spec, times)
    assert pulse[9] == 1.0 and abs(pulse[5] - 0.5) < 1e-12 and abs(pulse[13] - 0.5) < 1e-12     # t0 = 10 dt, fwhm = 8 dt
    assert np.allclose(pulse, so.gaussian_pulse(times, 7.5e-7, 6.0e-7), rtol=0, atol=1e-15)
    tag = mesh.material_tags["p_coupler"]
    F1, _ = so.source_vector(mesh.coords, mesh.tris, mesh.tags, [tag], spec.fwhm, spec.z0(stack), spec.depth)
    amp = src_mod.amplitudes(spec, times, F1)
    assert abs(2.0 * math.pi * amp.max() * math.fsum(F1) - spec.power) <= 1e-14 * spec.power
    assert np.allclose(amp, so.peak_density(spec.power, F1) * pulse, rtol=1e-15, atol=0)
    # a CSV pulse: linear interpolation, 0 outside, rows sorted by time, non-numeric rows dropped
    p = tmp_path / "pulse.csv"
    p.write_text("time,power\n2e-7,1.0\n1e-7,0.0\nnote,\n4e-7,0.5\n")
    fspec = src_mod.parse_source(_source_cfg(pulse={"file": str(p)}))
    got = src_mod.pulse_values(fspec, [0.5e-7, 1e-7, 1.5e-7, 2e-7, 3e-7, 4e-7, 4.1e-7])
    assert np.allclose(got, [0.0, 0.0, 0.5, 1.0, 0.75, 0.5, 0.0], rtol=0, atol=1e-15)
    (tmp_path / "bad.csv").write_text("time,temp\n0,1\n")
    with pytest.raises(ValueError, match="'power' column"):
        src_mod.pulse_values(src_mod.parse_source(_source_cfg(pulse={"file": str(tmp_path / "bad.csv")})), [0.0])
    with pytest.raises(ValueError, match=r"heating\.source.*sums to"):
        src_mod.power_density(1.0, np.zeros(4))


# ---- the configuration block -------------------------------------------------------------------------------------------------
def test_parsing_defaults_and_faces(small):
    _, stack, mesh = small
    assert src_mod.parse_source(load_cfg("geballe_with_diamond")) is None
    spec = src_mod.parse_source(_source_cfg())
    assert spec.materials == ("p_coupler",) and spec.power == 0.2 and spec.fwhm == 1.32e-5      # heating.fwhm
    assert math.isinf(spec.depth) and spec.face == "outer" and spec.keep_line is False
    assert spec.pulse == ("gaussian", 7.5e-7, 6.0e-7)
    box_p, box_o = stack.by_name("p_coupler").boundaries, stack.by_name("o_coupler").boundaries
    assert spec.z0(stack) == box_p[0]                                       # away from the sample on the p side: zmin
    assert src_mod.parse_source(_source_cfg(face="inner")).z0(stack) == box_p[1]
    assert src_mod.parse_source(_source_cfg(material="o_coupler")).z0(stack) == box_o[1]
    assert src_mod.parse_source(_source_cfg(material="o_coupler", face="inner")).z0(stack) == box_o[0]
    two = src_mod.parse_source(_source_cfg(material=["p_coupler", "p_ins"], fwhm="5e-6", depth="2e-8", keep_line=True))
    assert two.materials == ("p_coupler", "p_ins") and two.fwhm == 5e-6 and two.depth == 2e-8 and two.keep_line is True
    ps = two.problem_source(stack, mesh.material_tags)
    assert ps == {"tags": [mesh.material_tags["p_coupler"], mesh.material_tags["p_ins"]], "fwhm": 5e-6, "z0": box_p[0], "depth": 2e-8}


@pytest.mark.parametrize("over, pat", [
    ({"colour": "red"}, r"heating\.source: unknown key 'colour'"),
    ({"material": "unobtainium"}, r"heating\.source\.material: unknown material 'unobtainium'"),
    ({"material": ["p_coupler", "p_coupler"]}, r"heating\.source\.material lists a material twice"),
    ({"material": []}, r"heating\.source\.material names no material"),
    ({"power": 0.0}, r"heating\.source\.power must be positive"),
    ({"power": None}, r"heating\.source\.power is missing"),
    ({"fwhm": -1e-5}, r"heating\.source\.fwhm must be positive"),
    ({"depth": 0}, r"heating\.source\.depth must be positive"),
    ({"depth": "thin"}, r"heating\.source\.depth: a number is expected"),
    ({"face": "left"}, r"heating\.source\.face must be one of outer, inner"),
    ({"pulse": None}, r"heating\.source\.pulse is missing"),
    ({"pulse": {"t0": 1e-6, "fwhm": 5e-7, "file": "x.csv"}}, r"heating\.source\.pulse needs exactly one form"),
    ({"pulse": {}}, r"heating\.source\.pulse needs exactly one form"),
    ({"pulse": {"t0": 1e-6}}, r"heating\.source\.pulse: a Gaussian pulse needs both t0 and fwhm"),
    ({"pulse": {"t0": 1e-6, "fwhm": 0.0}}, r"heating\.source\.pulse\.fwhm must be positive"),
    ({"pulse": {"t0": 1e-6, "width": 1.0}}, r"heating\.source\.pulse: unknown key 'width'"),
    ({"keep_line": "yes"}, r"heating\.source\.keep_line must be true or false"),
])
def test_a_malformed_block_names_the_key(over, pat):
    with pytest.raises(ValueError, match=pat):
        src_mod.parse_source(_source_cfg(**over))


def test_used_config_writes_the_block_exactly_when_it_is_set():
    from heatflow_amd.driver import _with_scheme

    for name in ("geballe_with_diamond", "geballe_with_diamond_kT", "geballe_no_diamond"):
        assert "source" not in _with_scheme(load_cfg(name))["heating"]
    cfg = _source_cfg(depth=2e-8)
    out = _with_scheme(cfg)["heating"]
    assert out["source"] == {"material": ["p_coupler"], "power": 0.2, "fwhm": 1.32e-5, "face": "outer", "keep_line": False,
                             "depth": 2e-8, "pulse": {"t0": 7.5e-7, "fwhm": 6.0e-7}}
    assert out["file"] == cfg["heating"]["file"] and cfg["heating"]["source"].get("face") is None      # the input is not touched
    assert "depth" not in _with_scheme(_source_cfg())["heating"]["source"]                             # uniform stays absent
    shipped = load_cfg("geballe_with_diamond_source")
    assert src_mod.parse_source(shipped) is not None and _with_scheme(shipped)["heating"]["source"]["material"] == ["p_coupler"]


class RecordingBackend:
    """Records the HeatflowHIP calls HeatProblem makes."""

    def __init__(self):
        self.calls, self.args = [], []

    def __getattr__(self, name):
        if name.startswith("_"):
            raise AttributeError(name)

        def rec(*a, **k):
            self.calls.append(name)
            self.args.append(a)
            return (np.zeros((len(a[0]), 0)), np.zeros(len(a[0]), dtype=np.int32)) if name == "run" else None
        return rec


def _session(small, backend):
    from heatflow_amd.driver import SimulationSession

    _, _, mesh = small
    return SimulationSession(mesh.coords, mesh.tris, mesh.tags, mesh.material_tags, backend=backend)


def test_boundary_set_problem_key_and_optional_heating_file(small):
    from heatflow_amd.geometry import build_stack

    s = _session(small, RecordingBackend())
    cfg = _small_cfg(_source_cfg())
    del cfg["heating"]["file"]                                   # only the experiment scripts' RMSE needs it
    stack = build_stack(cfg)
    three = s._boundary_conditions(cfg, stack)
    assert [b.location for b in three] == ["left", "right", "top"] and s._heats == []
    kept = _small_cfg(_source_cfg(keep_line=True))
    four = s._boundary_conditions(kept, stack)
    assert [b.location for b in four] == ["left", "right", "top", "x"] and len(s._heats) == 1
    plain = _small_cfg(copy.deepcopy(load_cfg("geballe_with_diamond")))
    assert len(s._boundary_conditions(plain, stack)) == 4
    with pytest.raises(KeyError):
        s._boundary_conditions(_small_cfg({**_source_cfg(keep_line=True), "heating": {k: v for k, v in kept["heating"].items() if k != "file"}}), stack)
    src = s._source(cfg, stack)
    tk, trc = s._tables(stack)
    from heatflow_amd.driver import ProblemSpec

    base = ProblemSpec(7.5e-8, "backward_euler", trc, three)
    assert s._source(plain, stack) is None and dataclasses.replace(base, source=None).key == base.key
    k1 = dataclasses.replace(base, source=src).key
    k2 = dataclasses.replace(base, source=s._source(_small_cfg(_source_cfg(depth=2e-8)), stack)).key
    k3 = dataclasses.replace(base, source=s._source(_small_cfg(_source_cfg(power=0.4)), stack)).key
    assert k1 != base.key and k1 != k2 and k1 == k3              # the shape is part of the key, the power is an amplitude
    # the session's own spec of the configuration carries that source, in the key and in the problem's keywords
    spec = s.spec(cfg, stack)
    assert spec.source == src and spec.problem_kwargs()["source"] == src and "source" not in s.spec(plain, stack).problem_kwargs()
    assert spec.key != dataclasses.replace(spec, source=None).key


# ---- refusals ---------------------------------------------------------------------------------------------------------------
def test_sweeps_fit_and_1d_refuse_the_source(tmp_path):
    import yaml

    from heatflow_amd import fit, parameter_sweep, run_no_diamond_1d

    cfg = _source_cfg()
    pat = r"does not support the volumetric source \(heating\.source\)"
    with pytest.raises(ValueError, match="run_kappa_sweep " + pat):
        parameter_sweep.run_kappa_sweep(cfg, str(tmp_path), [3.8], str(tmp_path))
    p = tmp_path / "c.yaml"
    p.write_text(yaml.safe_dump(cfg))
    with pytest.raises(ValueError, match="run_parameter_sweep " + pat):
        parameter_sweep.run_parameter_sweep(str(p), str(tmp_path), [1e-5, 1e-5], [3.8, 3.8], [1.84e-6, 1.84e-6], 1)
    with pytest.raises(ValueError, match=r"heatflow_amd\.fit " + pat):
        fit.fit_parameters(cfg, str(tmp_path))
    with pytest.raises(ValueError, match=r"run_1d \(the 1-D model\) " + pat):
        run_no_diamond_1d.run_1d(cfg, str(tmp_path))


def test_session_refuses_batches_tangents_and_two_sided_runs(small):
    from heatflow_amd.geometry import build_stack
    from heatflow_amd.parameter_sweep import get_watcher_points

    be = RecordingBackend()
    s = _session(small, be)
    cfg = _small_cfg(_source_cfg())
    stack = build_stack(cfg)
    wp = get_watcher_points(cfg)
    with pytest.raises(ValueError, match=r"run_batch.*heating\.source"):
        s.run_batch([cfg, cfg], [stack, stack], wp)
    with pytest.raises(ValueError, match=r"tangents=.*heating\.source"):
        s.run(cfg, stack, wp, tangents=["p_sample"])
    with pytest.raises(ValueError, match=r"two_sided=True.*heating\.source"):
        s.run(cfg, stack, wp, two_sided=True)
    assert be.calls == []                                       # every refusal comes before any backend call


# ---- HeatProblem -------------------------------------------------------------------------------------------------------------
def _problem(small, backend, **kw):
    from helpers import make_problem

    cfg, stack, mesh = small
    return make_problem(cfg, stack, mesh, backend=backend, **kw)


def test_heat_problem_call_order_and_amplitudes(small):
    head = ["set_mesh", "set_materials"]
    tail = ["set_dirichlet", "set_precond", "assemble", "set_state"]
    without, with_src, with_an = RecordingBackend(), RecordingBackend(), RecordingBackend()
    _problem(small, without)
    source = dict(tags=[3], fwhm=1.4e-5, z0=-9.82e-7, depth=2e-8)
    prob = _problem(small, with_src, source=source)
    _problem(small, with_an, source=dict(tags=3, fwhm=1.4e-5, z0=-9.82e-7), k_aniso={3: (2.0, 1.0)})
    assert without.calls == head + tail                          # no source: the call sequence of before
    assert with_src.calls == head + ["set_source"] + tail
    assert with_an.calls == head + ["set_anisotropy", "set_source"] + tail
    assert with_src.args[2] == ([3], 1.4e-5, -9.82e-7, 2e-8) and with_an.args[3] == ([3], 1.4e-5, -9.82e-7, math.inf)
    n0 = len(with_src.calls)
    prob.run(3, source_amplitude=lambda t: t / prob.dt)
    assert with_src.calls[n0:] == ["set_source_amplitudes", "run"]
    assert np.allclose(with_src.args[n0][0], [1.0, 2.0, 3.0])    # evaluated at (k + 1) dt
    prob.run(2, source_amplitude=[5.0, 6.0], first_step=3)
    assert np.array_equal(with_src.args[n0 + 2][0], [5.0, 6.0])
    prob.run(2)                                                  # no amplitude: an empty list, i.e. amplitude 0
    assert with_src.calls[-2:] == ["set_source_amplitudes", "run"] and len(with_src.args[-2][0]) == 0
    prob.source_vector()
    assert with_src.calls[-1] == "get_source"
    with pytest.raises(ValueError, match="3 values expected, got 2"):
        prob.run(3, source_amplitude=[1.0, 2.0])
    with pytest.raises(ValueError, match="must be finite"):
        prob.run(1, source_amplitude=[math.nan])
    n1 = len(without.calls)
    with pytest.raises(ValueError, match="the problem has no source"):
        _problem(small, without).run(1, source_amplitude=[1.0])
    assert "set_source_amplitudes" not in without.calls[n1:]


@pytest.mark.parametrize("source, pat", [
    (dict(tags=[3], fwhm=1e-5), "z0 is missing"),
    (dict(tags=[], fwhm=1e-5, z0=0.0), "at least one cell tag"),
    (dict(tags=[3, 3], fwhm=1e-5, z0=0.0), "each once"),
    (dict(tags=[3], fwhm=0.0, z0=0.0), "fwhm must be positive"),
    (dict(tags=[3], fwhm=1e-5, z0=math.inf), "z0 must be finite"),
    (dict(tags=[3], fwhm=1e-5, z0=0.0, depth=-1.0), "depth must be positive"),
    (dict(tags=[3], fwhm=1e-5, z0=0.0, power=1.0), "unknown key 'power'"),
])
def test_heat_problem_checks_the_source_before_any_backend_call(small, source, pat):
    be = RecordingBackend()
    with pytest.raises(ValueError, match=pat):
        _problem(small, be, source=source)
    assert be.calls == []


# ---- the session end to end on a scipy stand-in ---------------------------------------------------------------------------------
class SourceOracleBackend(OracleBackend):
    """OracleBackend with the source: F1 from the restatement, b = M u^n + dt p_k F1."""

    F1 = None
    amp = ()
    pos = 0

    def set_source(self, tags, fwhm=1.0, z0=0.0, depth=math.inf):
        self.F1 = so.source_vector(self.coords, self.tris, self.tags, list(tags), fwhm, z0, depth)[0]
        self.amp, self.pos = (), 0

    def get_source(self):
        return self.F1.copy()

    def set_source_amplitudes(self, p):
        self.amp, self.pos = tuple(float(v) for v in p), 0

    def step(self, g, rtol=1e-10, atol=0.0, max_it=20000):
        p = 0.0
        if self.amp:
            p = self.amp[self.pos]
            self.pos += 1
        b = self.M @ self.u + self._dt * p * self.F1
        if self.n_bc:
            b -= self.A_lift @ g
            b[self.bc_dofs] = g
        self.u = self._lu.solve(b)
        return 1, 0.0


def test_session_run_carries_the_source_and_deposits_the_configured_energy(small):
    """Through SimulationSession.run on the stand-in: the run equals the restated loop, and while no heat has reached a
    Dirichlet row sum_i (M (u - u0))_i = dt sum_k p_k sum_i F1_i, i.e. 2 pi times it is the pulse's energy in joules."""
    from heatflow_amd.geometry import build_stack
    from heatflow_amd.parameter_sweep import get_watcher_points

    _, _, mesh = small
    dt = 1.0e-9          # short steps: within 8 of them no heat reaches the neighbours of a Dirichlet row (asserted below)
    cfg = _small_cfg(_source_cfg(fwhm=4.0e-6, pulse={"t0": 4 * dt, "fwhm": 3 * dt}))
    cfg["timing"] = dict(cfg["timing"], num_steps=8, t_final=8 * dt)
    stack = build_stack(cfg)
    be = SourceOracleBackend()
    s = _session(small, be)
    res = s.run(cfg, stack, get_watcher_points(cfg))
    spec = src_mod.parse_source(cfg)
    tk, trc = material_tables(stack, mesh)
    tag = mesh.material_tags["p_coupler"]
    F1, _ = so.source_vector(mesh.coords, mesh.tris, mesh.tags, [tag], spec.fwhm, spec.z0(stack), spec.depth)
    times = (np.arange(8) + 1) * dt
    amp = so.peak_density(spec.power, F1) * so.gaussian_pulse(times, 4 * dt, 3 * dt)
    dofs = np.asarray(s.problem.bc_dofs, dtype=np.int64)
    ref = so.sourced_fields(mesh.coords, mesh.tris, mesh.tags, tk, trc, dt, dofs, np.full(len(mesh.coords), 300.0),
                            [np.full(len(dofs), 300.0)] * 8, F1, amp)
    assert np.abs(be.u - ref[-1]).max() <= 1e-9 and ref[-1].max() > 310.0
    assert res["watchers"]["pside"][-1] > 305.0                  # the free p-side face responds
    near = np.unique(be.A[dofs].indices)
    assert np.abs(ref[-1][near] - 300.0).max() <= 1e-9
    energy = 2.0 * math.pi * (be.M @ (be.u - 300.0)).sum()
    want = spec.power * dt * so.gaussian_pulse(times, 4 * dt, 3 * dt).sum()
    assert abs(energy - want) <= 1e-9 * want, (energy, want)
    # the step-wise path (a field sink) hands over the same amplitudes, one per step
    fields = []
    s.run(cfg, stack, get_watcher_points(cfg), field_sink=lambda t, u: fields.append(u.copy()))
    assert np.abs(np.array(fields) - ref).max() <= 1e-9


# ---- the C interface ------------------------------------------------------------------------------------------------------------
def test_header_declares_and_backend_lists_the_source_entry_points():
    from heatflow_amd import hip_backend

    with open(os.path.join(ROOT, "include", "heatflow_hip.h")) as f:
        text = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    declared = set(re.findall(r"\b(hf_\w+)\s*\(", text))
    assert declared == set(hip_backend.EXPORTS)                  # the header and EXPORTS agree, name for name
    for name in ("hf_set_source", "hf_get_source", "hf_set_source_amplitudes"):
        assert name in declared
    for method in ("set_source", "get_source", "set_source_amplitudes"):
        assert hasattr(hip_backend.HeatflowHIP, method)
    with open(os.path.join(ROOT, "heatflow_amd", "csrc", "heatflow_hip.hip")) as f:
        impl = f.read()
    for name in ("hf_set_source", "hf_get_source", "hf_set_source_amplitudes"):
        assert re.search(rf"^int {name}\(", impl, flags=re.M)
