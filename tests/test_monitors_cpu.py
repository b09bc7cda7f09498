"""Region monitors without a GPU: the float64 restatement (tests/monitor_oracle.py) against analytic volumes, hot volumes and
means on both small meshes, the edge rules, the ``monitors`` block (parsing, used_config.yaml, monitors.csv), the combination
into regions, every refusal by name, HeatProblem's call order on a recording stand-in, run_simulation end to end on a scipy
stand-in with the energy identity, and the header against EXPORTS."""
import copy
import csv
import functools
import math
import os
import re

import numpy as np
import pytest
import yaml

import monitor_oracle as mo
import source_oracle as so
from conftest import ROOT, build_case, load_cfg
from oracle_backend import OracleBackend

from heatflow_amd import monitors as mon_mod

CASES = {"with_diamond": "geballe_with_diamond", "no_diamond": "geballe_no_diamond"}
MATS = ("p_sample", "p_ins", "p_coupler")
REL = 1e-12          # analytic checks: the restatement sums exactly, a term carries a few roundings - ne * eps covers the largest tag


@functools.lru_cache(maxsize=None)
def small(which):
    return build_case(CASES[which], 8.0)


def _box(stack, name):
    z0, z1, r0, r1 = (float(v) for v in stack.by_name(name).boundaries[:4])
    return z0, z1, r0, r1


# ---- the restatement against analytic values -------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", MATS)
@pytest.mark.parametrize("which", sorted(CASES))
def test_volume_hot_volume_and_mean_of_linear_fields(which, name):
    _, stack, mesh = small(which)
    tag = mesh.material_tags[name]
    z0, z1, r0, r1 = _box(stack, name)
    assert np.count_nonzero(mesh.tags == tag) * mo.EPS < REL
    z, r = mesh.coords[:, 0], mesh.coords[:, 1]
    vol = math.pi * (r1 * r1 - r0 * r0) * (z1 - z0)
    # linear in z: above 300 K beyond z*
    zs, cz = z0 + 0.37 * (z1 - z0), 1.0e8
    rec, _, _, br = mo.per_tag(mesh.coords, mesh.tris, mesh.tags, 300.0 + cz * (z - zs), {tag: 300.0})
    assert abs(2.0 * math.pi * rec[tag, 4] - vol) <= REL * vol
    hot = math.pi * (r1 * r1 - r0 * r0) * (z1 - zs)
    assert abs(2.0 * math.pi * rec[tag, 6] - hot) <= REL * hot, (2.0 * math.pi * rec[tag, 6], hot)
    mean = 300.0 + cz * (0.5 * (z0 + z1) - zs)
    assert abs(rec[tag, 5] / rec[tag, 4] - mean) <= REL * abs(mean)
    assert br[tag, 1] > 0 and br[tag, 2] > 0                   # the cut runs through the layer (a coupler is one element thick)
    # linear in r: above 300 K inside r*
    rstar, cr = r0 + 0.41 * (r1 - r0), 1.0e7
    rec, _, _, br = mo.per_tag(mesh.coords, mesh.tris, mesh.tags, 300.0 - cr * (r - rstar), {tag: 300.0})
    hot = math.pi * (rstar * rstar - r0 * r0) * (z1 - z0)
    assert abs(2.0 * math.pi * rec[tag, 6] - hot) <= REL * hot, (2.0 * math.pi * rec[tag, 6], hot)
    rbar = (2.0 / 3.0) * (r1 ** 3 - r0 ** 3) / (r1 * r1 - r0 * r0)
    mean = 300.0 - cr * (rbar - rstar)
    assert abs(rec[tag, 5] / rec[tag, 4] - mean) <= REL * abs(mean)
    assert br[tag, 1] > 0 and br[tag, 2] > 0


def test_edge_rules_of_the_restatement():
    _, _, mesh = small("with_diamond")
    tag = mesh.material_tags["p_sample"]
    other = mesh.material_tags["p_ins"]
    nodes = np.unique(mesh.tris[mesh.tags == tag])
    rng = np.random.default_rng(5)
    u = 300.0 + 50.0 * rng.random(len(mesh.coords))
    u[nodes] = 1234.5                                         # the whole tag held at exactly theta: nothing is above
    rec, _, _, br = mo.per_tag(mesh.coords, mesh.tris, mesh.tags, u, {tag: 1234.5, other: None})
    assert rec[tag, 6] == 0.0 and br[tag, 0] == np.count_nonzero(mesh.tags == tag)
    assert rec[other, 6] == 0.0 and rec[other, 4] > 0.0       # no threshold: H = 0
    assert rec[tag, 0] == 1234.5 and rec[tag, 1] == nodes.min() and rec[tag, 3] == nodes.min()     # ties: the smallest id
    u[nodes] = np.nextafter(1234.5, math.inf)                 # one ulp above: the whole tag
    rec, _, _, _ = mo.per_tag(mesh.coords, mesh.tris, mesh.tags, u, {tag: 1234.5})
    assert rec[tag, 6] == rec[tag, 4]
    # a plateau of equal maxima inside a varying field
    u = 300.0 + 50.0 * rng.random(len(mesh.coords))
    plateau = np.sort(rng.choice(nodes, 7, replace=False))
    u[plateau] = 400.0
    rec, _, _, _ = mo.per_tag(mesh.coords, mesh.tris, mesh.tags, u, {tag: None})
    assert rec[tag, 0] == 400.0 and rec[tag, 1] == plateau[0]
    with pytest.raises(ValueError, match="tag 0 is not a cell tag"):
        mo.per_tag(mesh.coords, mesh.tris, mesh.tags, u, {0: None})


def test_every_branch_of_the_cut_on_one_triangle():
    """A right triangle with legs 1 at r in [1, 2], u = z: the part with z > 0.25, by hand."""
    coords = np.array([[0.0, 1.0], [1.0, 1.0], [0.0, 2.0]])
    tris = np.array([[0, 1, 2]])
    u = coords[:, 0].copy()

    def strip(c):   # int r dA over {z > c} of the triangle: r from 1 to 2 - z
        f = lambda z: (2.0 - z) ** 3 / -6.0 - 0.5 * z                                   # noqa: E731 - antiderivative of ((2 - z)^2 - 1) / 2
        return f(1.0) - f(c)

    for perm in ([0, 1, 2], [1, 2, 0], [2, 0, 1], [0, 2, 1]):
        t = tris[:, perm]
        for c, cnt in ((0.25, 1), (-1.0, 3), (1.5, 0)):
            I0, I1, H, n = mo.triangle_terms(coords, t, u, c)
            assert n[0] == cnt and abs(H[0] - (strip(max(c, 0.0)) if c < 1.0 else 0.0)) <= 1e-15
        I0, I1, H, n = mo.triangle_terms(coords, t, -u, -0.25)                          # two nodes above: z < 0.25
        assert n[0] == 2 and abs(H[0] - (strip(0.0) - strip(0.25))) <= 1e-15
        assert abs(I0[0] - strip(0.0)) <= 1e-15 and abs(I1[0] + 5.0 / 24.0) <= 1e-15      # int z r dA = 5 / 24, of -u here


# ---- the configuration block ---------------------------------------------------------------------------------------------------------
def _cfg(block=None, base="geballe_with_diamond"):
    cfg = copy.deepcopy(load_cfg(base))
    cfg["monitors"] = {"sample": {"material": "p_sample", "above": 2000.0},
                       "coupler": {"material": ["p_coupler", "o_coupler"]}} if block is None else block
    return cfg


def _small_cfg(cfg):
    cfg["mats"] = {k: dict(v, mesh=float(v["mesh"]) * 8.0) for k, v in cfg["mats"].items()}
    return cfg


def test_parsing_and_used_config():
    from heatflow_amd.driver import _with_scheme

    assert mon_mod.parse_monitors(load_cfg("geballe_with_diamond")) is None
    for name in ("geballe_with_diamond", "geballe_with_diamond_source", "geballe_no_diamond"):
        assert "monitors" not in _with_scheme(load_cfg(name))
    spec = mon_mod.parse_monitors(_cfg())
    assert list(spec) == ["sample", "coupler"]
    assert spec["sample"] == {"materials": ("p_sample",), "above": 2000.0}
    assert spec["coupler"] == {"materials": ("p_coupler", "o_coupler"), "above": None}
    assert _with_scheme(_cfg())["monitors"] == {"sample": {"material": ["p_sample"], "above": 2000.0},
                                                "coupler": {"material": ["p_coupler", "o_coupler"]}}
    assert mon_mod.parse_monitors(_cfg({"s": {"material": "p_sample", "above": "1.5e3"}}))["s"]["above"] == 1500.0
    tags = {"p_sample": 4, "p_coupler": 3, "o_coupler": 5}
    assert mon_mod.problem_monitors(spec, tags) == {"sample": {"tags": [4], "above": 2000.0}, "coupler": {"tags": [3, 5], "above": None}}


@pytest.mark.parametrize("block, pat", [
    ({"s": {"material": "p_sample", "colour": 1}}, r"monitors\.s: unknown key 'colour'"),
    ({"s": {"material": "unobtainium"}}, r"monitors\.s\.material: unknown material 'unobtainium'"),
    ({"s": {"material": ["p_sample", "p_sample"]}}, r"monitors\.s\.material lists a material twice"),
    ({"s": {"material": []}}, r"monitors\.s\.material names no material"),
    ({"s": {"above": 1.0}}, r"monitors\.s\.material is missing"),
    ({"s": {"material": "p_sample", "above": math.inf}}, r"monitors\.s\.above must be finite"),
    ({"s": {"material": "p_sample", "above": math.nan}}, r"monitors\.s\.above must be finite"),
    ({"s": {"material": "p_sample", "above": "hot"}}, r"monitors\.s\.above: a number is expected"),
    ({"s": "p_sample"}, r"monitors\.s must be a mapping"),
    ({"a.b": {"material": "p_sample"}}, r"monitors: region name 'a\.b'"),
    ([], r"monitors must be a mapping"),
])
def test_a_malformed_block_names_the_key(block, pat):
    with pytest.raises(ValueError, match=pat):
        mon_mod.parse_monitors(_cfg(block))


def test_regions_thresholds_and_the_two_region_conflict():
    regions = mon_mod.check_regions({"a": {"tags": [4, 2], "above": 1000}, "b": {"tags": 4}, "c": {"tags": [2, 7], "above": 1000.0}})
    assert regions == {"a": {"tags": [2, 4], "above": 1000.0}, "b": {"tags": [4], "above": None}, "c": {"tags": [2, 7], "above": 1000.0}}
    assert mon_mod.tag_thresholds(regions) == {2: 1000.0, 4: 1000.0, 7: 1000.0}
    assert mon_mod.tag_thresholds(mon_mod.check_regions({"b": {"tags": [4]}, "a": {"tags": [4], "above": 5.0}})) == {4: 5.0}
    assert mon_mod.check_regions(None) is None and mon_mod.check_regions({}) is None
    with pytest.raises(ValueError, match=r"monitors: cell tag 4 is in region 'a' with above = 1000.0 and in region 'd' with above = 1500.0"):
        mon_mod.tag_thresholds(mon_mod.check_regions({"a": {"tags": [2, 4], "above": 1000.0}, "d": {"tags": [4], "above": 1500.0}}))
    for bad, pat in (({"a": {"tags": []}}, "monitors: region 'a': tags must name at least one"),
                     ({"a": {"tags": [3, 3]}}, "each once"), ({"a": {"tags": [3], "above": math.inf}}, "above must be finite"),
                     ({"a": {"tags": [3], "below": 1.0}}, "monitors: region 'a': unknown key 'below'")):
        with pytest.raises(ValueError, match=pat):
            mon_mod.check_regions(bad)


def test_combination_into_regions_energy_and_csv(tmp_path):
    coords = np.array([[0.0, 0.0], [1.0, 0.5], [2.0, 1.0], [3.0, 1.5]])
    rec = np.zeros((2, 6, 7))
    #               T_max node T_min node I0   I1     H
    rec[0, 2] = [400.0, 1, 300.0, 0, 2.0, 700.0, 0.5]
    rec[0, 5] = [450.0, 3, 310.0, 2, 1.0, 400.0, 0.25]
    rec[1, 2] = [500.0, 2, 300.0, 0, 2.0, 800.0, 1.0]
    rec[1, 5] = [500.0, 1, 290.0, 3, 1.0, 420.0, 0.5]
    regions = mon_mod.check_regions({"both": {"tags": [5, 2], "above": 350.0}, "one": {"tags": [5]}})
    out = mon_mod.combine(rec, regions, coords, rho_c={2: 10.0, 5: 100.0}, T_ref=300.0)
    b = out["both"]
    assert b["T_max"].tolist() == [450.0, 500.0] and b["z_max"].tolist() == [3.0, 2.0] and b["r_max"].tolist() == [1.5, 1.0]   # ties: the lower tag
    assert b["T_min"].tolist() == [300.0, 290.0] and b["z_min"].tolist() == [0.0, 3.0]
    assert np.allclose(b["volume"], 2 * math.pi * 3.0) and np.allclose(b["T_mean"], [1100.0 / 3.0, 1220.0 / 3.0])
    assert np.allclose(b["hot_volume"], [2 * math.pi * 0.75, 2 * math.pi * 1.5]) and np.allclose(b["hot_fraction"], [0.25, 0.5])
    assert np.allclose(b["energy"], [2 * math.pi * (10.0 * 100.0 + 100.0 * 100.0), 2 * math.pi * (10.0 * 200.0 + 100.0 * 120.0)])
    assert "hot_volume" not in out["one"] and "hot_fraction" not in out["one"] and "energy" in out["one"]
    # a capacity table on a tag of the region: the constant is not the run's, the key is absent
    tab = mon_mod.combine(rec, regions, coords, rho_c={2: 10.0, 5: 100.0}, T_ref=300.0, tabled={2: None})
    assert "energy" not in tab["both"] and "energy" in tab["one"]
    assert "energy" not in mon_mod.combine(rec, regions, coords)["both"]
    one = mon_mod.combine(rec[1], regions, coords, rho_c={2: 10.0, 5: 100.0}, T_ref=300.0)          # a single record: scalars
    assert one["both"]["T_max"] == 500.0 and one["both"]["energy"] == b["energy"][1]
    path = tmp_path / "monitors.csv"
    mon_mod.write_monitors_csv(str(path), [0.1, 0.2], out)
    with open(path, newline="") as f:
        rows = list(csv.reader(f))
    assert rows[0][0] == "time" and rows[0][1:4] == ["both.T_max", "both.z_max", "both.r_max"]
    assert "both.hot_fraction" in rows[0] and "one.hot_fraction" not in rows[0] and "one.energy" in rows[0]
    assert len(rows) == 3 and float(rows[2][0]) == 0.2 and float(rows[2][rows[0].index("both.T_mean")]) == b["T_mean"][1]


# ---- refusals ------------------------------------------------------------------------------------------------------------------------
def test_sweeps_fit_batches_and_1d_refuse_monitors(tmp_path):
    from heatflow_amd import fit, parameter_sweep, run_no_diamond_1d
    from heatflow_amd.driver import SimulationSession
    from heatflow_amd.geometry import build_stack
    from heatflow_amd.parameter_sweep import get_watcher_points

    cfg = _cfg()
    pat = r"does not support region monitors \(monitors\)"
    with pytest.raises(ValueError, match="run_kappa_sweep " + pat):
        parameter_sweep.run_kappa_sweep(cfg, str(tmp_path), [3.8], str(tmp_path))
    p = tmp_path / "c.yaml"
    p.write_text(yaml.safe_dump(cfg))
    with pytest.raises(ValueError, match="run_parameter_sweep " + pat):
        parameter_sweep.run_parameter_sweep(str(p), str(tmp_path), [1e-5, 1e-5], [3.8, 3.8], [1.84e-6, 1.84e-6], 1)
    with pytest.raises(ValueError, match=r"heatflow_amd\.fit " + pat):
        fit.fit_parameters(cfg, str(tmp_path))
    with pytest.raises(ValueError, match=r"run_1d \(the 1-D model\) " + pat):
        run_no_diamond_1d.run_1d(_cfg(base="geballe_no_diamond"), str(tmp_path))
    _, _, mesh = small("with_diamond")
    be = RecordingBackend()
    s = SimulationSession(mesh.coords, mesh.tris, mesh.tags, mesh.material_tags, backend=be)
    scfg = _small_cfg(_cfg())
    stack = build_stack(scfg)
    with pytest.raises(ValueError, match=r"run_batch \(the batched loop\) " + pat):
        s.run_batch([scfg, scfg], [stack, stack], get_watcher_points(scfg))
    assert be.calls == []


# ---- HeatProblem -----------------------------------------------------------------------------------------------------------------------
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
            if name == "run":
                return np.zeros((len(a[0]), 0)), np.zeros(len(a[0]), dtype=np.int32)
            if name == "step":
                return 1, 0.0
            if name == "monitor_now":
                return np.zeros((8, 7))
            if name == "get_monitors":
                return np.zeros((2, 8, 7))
            return None
        return rec


def test_heat_problem_call_order_with_and_without_monitors():
    from helpers import make_problem

    cfg, stack, mesh = small("with_diamond")
    head = ["set_mesh", "set_materials"]
    tail = ["set_dirichlet", "set_precond", "assemble", "set_state"]
    without, with_mon, with_all = RecordingBackend(), RecordingBackend(), RecordingBackend()
    plain = make_problem(cfg, stack, mesh, backend=without)
    regions = {"sample": {"tags": [4], "above": 2000.0}, "pair": {"tags": [3, 4]}}
    prob = make_problem(cfg, stack, mesh, backend=with_mon, monitors=regions)
    make_problem(cfg, stack, mesh, backend=with_all, monitors=regions, source=dict(tags=[3], fwhm=1.4e-5, z0=-9.82e-7),
                 k_aniso={3: (2.0, 1.0)})
    assert without.calls == head + tail                          # no monitors: the call sequence of before
    assert with_mon.calls == head + ["set_monitors"] + tail
    assert with_all.calls == head + ["set_anisotropy", "set_source", "set_monitors"] + tail
    assert with_mon.args[2] == ({3: None, 4: 2000.0},) or with_mon.args[2] == ({4: 2000.0, 3: None},)
    n0 = len(with_mon.calls)
    prob.run(3)
    prob.step(prob.dt)
    assert with_mon.calls[n0:] == ["run", "step"]                # run and step keep their calls: the backend records by itself
    now = prob.monitors_now()
    hist = prob.monitor_history()
    prob.clear_monitor_history()
    assert with_mon.calls[n0 + 2:] == ["monitor_now", "get_monitors", "clear_monitor_records"]
    assert set(now) == {"sample", "pair"} and "hot_volume" in now["sample"] and "hot_volume" not in now["pair"]
    assert hist["pair"]["T_max"].shape == (2,)
    n1 = len(without.calls)
    for fn in (plain.monitors_now, plain.monitor_history):
        with pytest.raises(ValueError, match="monitors: the problem has no monitors"):
            fn()
    plain.clear_monitor_history()
    assert without.calls[n1:] == []
    be = RecordingBackend()
    with pytest.raises(ValueError, match="region 'a'.*region 'b'"):
        make_problem(cfg, stack, mesh, backend=be, monitors={"a": {"tags": [4], "above": 1.0}, "b": {"tags": [4], "above": 2.0}})
    assert be.calls == []


# ---- run_simulation end to end on a scipy stand-in -----------------------------------------------------------------------------------------
class MonitorOracleBackend(OracleBackend):
    """OracleBackend with a volumetric source (b = M u^n + dt p_k F1) and the monitors of the restatement."""

    F1 = None
    amp = ()
    pos = 0
    thresholds = None

    def set_mesh(self, coords, tris, tags, pattern=None):
        super().set_mesh(coords, tris, tags, pattern)
        self.tab_len = int(np.max(tags)) + 1
        self.thresholds, self.records, self.fields = None, [], []

    def set_source(self, tags, fwhm=1.0, z0=0.0, depth=math.inf):
        self.F1 = so.source_vector(self.coords, self.tris, self.tags, list(tags), fwhm, z0, depth)[0]
        self.amp, self.pos = (), 0

    def get_source(self):
        return self.F1.copy()

    def set_source_amplitudes(self, p):
        self.amp, self.pos = tuple(float(v) for v in p), 0

    def set_monitors(self, thresholds):
        self.thresholds, self.records = dict(thresholds), []

    def monitor_now(self):
        return mo.per_tag(self.coords, self.tris, self.tags, self.u, self.thresholds, self.tab_len)[0]

    def monitor_count(self):
        return len(self.records)

    def get_monitors(self, first=0, count=None):
        return np.array(self.records[first:None if count is None else first + count]).reshape(-1, self.tab_len, 7)

    def clear_monitor_records(self):
        self.records = []

    def step(self, g, rtol=1e-10, atol=0.0, max_it=20000):
        p = 0.0
        if self.amp:
            p = self.amp[self.pos]
            self.pos += 1
        b = self.M @ self.u + (self._dt * p * self.F1 if self.F1 is not None else 0.0)
        if self.n_bc:
            b -= self.A_lift @ g
            b[self.bc_dofs] = g
        self.u = self._lu.solve(b)
        if self.thresholds:
            self.records.append(self.monitor_now())
            self.fields.append(self.u.copy())
        return 1, 0.0


def test_run_simulation_returns_and_writes_the_monitors_and_the_energy_is_the_mass_weighted_rise(tmp_path):
    from heatflow_amd.parameter_sweep import get_watcher_points
    from heatflow_amd.run_with_diamond import run_simulation

    cfg = _small_cfg(copy.deepcopy(load_cfg("geballe_with_diamond_source")))
    nsteps = 12
    cfg["timing"] = dict(cfg["timing"], num_steps=nsteps, t_final=nsteps * 7.5e-8)
    cfg["heating"]["source"].update(power=2.0, pulse={"t0": 4.5e-7, "fwhm": 4.0e-7})
    mats = sorted(cfg["mats"])
    cfg["monitors"] = {"coupler": {"material": ["p_coupler", "o_coupler"]}, "sample": {"material": "p_sample", "above": 300.5},
                       "all": {"material": mats}}
    be = MonitorOracleBackend()
    out = tmp_path / "out"
    res = run_simulation(cfg, str(tmp_path / "mesh"), rebuild_mesh=True, output_folder=str(out), watcher_points=get_watcher_points(cfg),
                         write_xdmf=False, suppress_print=True, backend=be)
    m = res["monitors"]
    assert list(m) == ["coupler", "sample", "all"] and all(len(v) == nsteps for f in m.values() for v in f.values())
    assert "hot_volume" in m["sample"] and "hot_volume" not in m["coupler"] and "energy" in m["all"]
    # the coupler absorbs: its peak is the run's peak, above every watcher, and it rises by tens of kelvin
    assert np.array_equal(m["coupler"]["T_max"], m["all"]["T_max"]) and m["coupler"]["T_max"].max() > 310.0
    for name, w in res["watchers"].items():
        assert np.all(m["all"]["T_max"] >= w) and np.all(m["all"]["T_min"] <= w), name
    assert 0.0 < m["sample"]["hot_fraction"].max() <= 1.0 and np.all(np.diff(m["sample"]["hot_volume"][:6]) >= 0.0)
    # energy over all materials = 2 pi sum_i (M (u - T_ref))_i of the stand-in's own fields, after the last step, within
    # (3 ne + 16) eps sum_ij |M_ij| |u_j - T_ref|.  The bound scales with the rise while `energy` is a difference of the cell's
    # whole heat content (1.07e-3 J at 300 K, one ulp of which is 2e-19 J): the identity can be resolved to that bound only once
    # the deposited energy has grown, hence the 2 W pulse (8e-7 J by the last step) and the last step.
    ne = len(be.tris)
    du = be.fields[-1] - 300.0
    want = 2.0 * math.pi * math.fsum(be.M @ du)
    bound = 2.0 * math.pi * (3 * ne + 16) * mo.EPS * math.fsum(abs(be.M) @ np.abs(du))
    got = m["all"]["energy"][-1]
    print(f"energy {got:.12e} J against 2 pi sum M (u - T_ref) = {want:.12e} J: difference {abs(got - want):.2e}, bound {bound:.2e}")
    assert want > 5e-7 and abs(got - want) <= bound, (got, want, bound)
    # monitors.csv equals the result, at the watcher CSV's times; used_config.yaml carries the block
    with open(out / "monitors.csv", newline="") as f:
        rows = list(csv.reader(f))
    with open(out / "watcher_points.csv", newline="") as f:
        wrows = list(csv.reader(f))
    assert [r[0] for r in rows[1:]] == [r[0] for r in wrows[1:]] and len(rows) == nsteps + 1
    for j, col in enumerate(rows[0][1:], start=1):
        region, field = col.split(".")
        assert [float(r[j]) for r in rows[1:]] == m[region][field].tolist(), col
    with open(out / "used_config.yaml") as f:
        used = yaml.safe_load(f)
    assert used["monitors"]["sample"] == {"material": ["p_sample"], "above": 300.5}
    # a capacity table on the sample: its regions lose `energy`, the others keep it
    from heatflow_amd.monitors import combine

    regions = {"sample": {"tags": [4], "above": None}}
    assert "energy" not in combine(np.zeros((1, 8, 7)) + 1.0, regions, np.zeros((2, 2)), rho_c={4: 1.0}, T_ref=300.0, tabled={4})["sample"]


def test_a_second_run_of_a_session_returns_its_own_records_only():
    from heatflow_amd.driver import SimulationSession
    from heatflow_amd.geometry import build_stack
    from heatflow_amd.parameter_sweep import get_watcher_points

    _, _, mesh = small("with_diamond")
    cfg = _small_cfg(_cfg({"sample": {"material": "p_sample", "above": 301.0}}))
    cfg["timing"] = dict(cfg["timing"], num_steps=5, t_final=5 * 7.5e-8)
    stack = build_stack(cfg)
    be = MonitorOracleBackend()
    s = SimulationSession(mesh.coords, mesh.tris, mesh.tags, mesh.material_tags, backend=be)
    first = s.run(cfg, stack, get_watcher_points(cfg))
    second = s.run(cfg, stack, get_watcher_points(cfg))
    assert be.set_mesh_calls == 1 and len(second["monitors"]["sample"]["T_max"]) == 5
    assert np.array_equal(first["monitors"]["sample"]["T_mean"], second["monitors"]["sample"]["T_mean"])
    fields = []
    third = s.run(cfg, stack, get_watcher_points(cfg), field_sink=lambda t, u: fields.append(u))      # the step-wise path records too
    assert np.array_equal(third["monitors"]["sample"]["T_max"], first["monitors"]["sample"]["T_max"]) and len(fields) == 5
    plain = copy.deepcopy(cfg)
    del plain["monitors"]
    assert "monitors" not in s.run(plain, stack, get_watcher_points(plain))


# ---- the C interface -------------------------------------------------------------------------------------------------------------------
def test_header_declares_and_backend_lists_the_monitor_entry_points():
    from heatflow_amd import hip_backend

    with open(os.path.join(ROOT, "include", "heatflow_hip.h")) as f:
        text = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    declared = set(re.findall(r"\b(hf_\w+)\s*\(", text))
    assert declared == set(hip_backend.EXPORTS)
    names = ("hf_set_monitors", "hf_monitor_now", "hf_monitor_count", "hf_get_monitors", "hf_monitor_clear")
    with open(os.path.join(ROOT, "heatflow_amd", "csrc", "heatflow_hip.hip")) as f:
        impl = f.read()
    for name in names:
        assert name in declared and re.search(rf"^int {name}\(", impl, flags=re.M)
    for method in ("set_monitors", "monitor_now", "monitor_count", "get_monitors", "clear_monitor_records"):
        assert hasattr(hip_backend.HeatflowHIP, method)
    assert "hf_batch" in text and re.search(r"batched loop\s*\n?.*records nothing", open(os.path.join(ROOT, "include", "heatflow_hip.h")).read())
