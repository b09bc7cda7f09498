"""Sweeps under kappa(T) / cv(T) tables without a GPU: the opt-in key ``timing.sweep_tables``, the refusals that stay
without it (word for word) and with it (naming both keys), what the configurations of a batch must share, the calls run_batch makes
under the key, the problem key, used_config.yaml, and the header / backend lists of the new entry points."""
import copy
import dataclasses
import os
import re

import numpy as np
import pytest
import yaml

from conftest import ROOT, build_case, load_cfg

from heatflow_amd import kappa_t

NSTEPS = 3


@pytest.fixture(scope="module")
def small():
    return build_case("geballe_with_diamond", 8.0)


def _cfg(key=True, **timing):
    cfg = copy.deepcopy(load_cfg("geballe_with_diamond_kT"))
    cfg["mats"] = {k: dict(v, mesh=float(v["mesh"]) * 8.0) for k, v in cfg["mats"].items()}
    cfg["timing"] = dict(cfg["timing"], num_steps=NSTEPS, t_final=NSTEPS * 7.5e-8, **timing)
    if key:
        cfg["timing"]["sweep_tables"] = True
    return cfg


class Recorder:
    """Records the HeatflowHIP calls a session makes, with their arguments; answers have the shapes of the real ones."""

    def __init__(self, n):
        self.calls, self.args, self.kwargs, self.n, self.batch_nv = [], [], [], n, 0

    def __getattr__(self, name):
        if name.startswith("_"):
            raise AttributeError(name)

        def rec(*a, **k):
            self.calls.append(name)
            self.args.append(a)
            self.kwargs.append(k)
            if name == "batch_begin":
                self.batch_nv = int(a[0])
            if name == "batch_run":
                g = a[0]
                ns = 0 if len(a) < 5 or a[4] is None else len(a[4])
                return np.zeros((g.shape[0], g.shape[2], ns)), np.ones((g.shape[0], g.shape[2]), dtype=np.int32)
            return None
        return rec


def _session(mesh, backend):
    from heatflow_amd.driver import SimulationSession

    return SimulationSession(mesh.coords, mesh.tris, mesh.tags, mesh.material_tags, backend=backend)


def _stacks(cfgs):
    from heatflow_amd.geometry import build_stack

    return [build_stack(c) for c in cfgs]


def test_the_key_is_a_boolean_and_defaults_to_false():
    assert kappa_t.sweep_tables(_cfg()) is True and kappa_t.sweep_tables(_cfg(key=False)) is False
    assert kappa_t.sweep_tables({}) is False and kappa_t.sweep_tables(load_cfg("geballe_with_diamond")) is False
    for bad in (1, "yes", None, 0):
        with pytest.raises(ValueError, match=r"timing\.sweep_tables must be true or false"):
            kappa_t.sweep_tables(_cfg(sweep_tables=bad, key=False))


def test_without_the_key_the_three_entry_points_refuse_word_for_word(small, tmp_path):
    from heatflow_amd import parameter_sweep as ps

    _, _, mesh = small
    cfg = _cfg(key=False)
    keys = ", ".join(f"mats.{m}.k_power" for m in ("g_ins", "o_diam", "o_ins", "p_diam", "p_ins"))

    def message(where):
        return re.escape(f"{where} does not support temperature-dependent conductivities ({keys})") + "$"

    with pytest.raises(ValueError, match=message("run_kappa_sweep")):
        ps.run_kappa_sweep(cfg, str(tmp_path), [3.8], str(tmp_path))
    p = tmp_path / "c.yaml"
    p.write_text(yaml.safe_dump(cfg))
    with pytest.raises(ValueError, match=message("run_parameter_sweep")):
        ps.run_parameter_sweep(str(p), str(tmp_path), [1e-5, 1e-5], [3.8, 3.8], [1.84e-6, 1.84e-6], 1)
    be = Recorder(len(mesh.coords))
    with pytest.raises(ValueError, match=message("run_batch (the batched loop)")):
        _session(mesh, be).run_batch([cfg, cfg], _stacks([cfg, cfg]), ps.get_watcher_points(cfg))
    assert be.calls == []
    cv = _cfg(key=False)
    cv["mats"]["p_sample"]["cv_einstein"] = {"theta": 300.0, "T_ref": 300.0, "T_min": 300.0, "T_max": 900.0}
    for m in cv["mats"].values():
        m.pop("k_power", None)
    with pytest.raises(ValueError, match=r"^run_kappa_sweep does not support temperature-dependent heat capacities "
                                         r"\(mats\.p_sample\.cv_einstein\)$"):
        ps.run_kappa_sweep(cv, str(tmp_path), [3.8], str(tmp_path))
    # refuse_tables itself keeps its signature and messages
    with pytest.raises(ValueError, match=message("somewhere")):
        kappa_t.refuse_tables(_cfg(), "somewhere")


def _refusals():
    aniso = _cfg()
    aniso["mats"]["p_sample"]["k_aniso"] = {"r": 2.0}
    aniso2 = copy.deepcopy(aniso)
    aniso2["timing"]["aniso_tables"] = True
    src = _cfg()
    src["heating"]["source"] = {"material": ["p_coupler"], "power": 1.0, "keep_line": True}
    src2 = copy.deepcopy(src)
    src2["heating"]["source"]["sweeps"] = True
    mon = _cfg()
    mon["monitors"] = {"sample": {"material": "p_sample"}}
    mon2 = _cfg(sweep_monitors=True)
    mon2["monitors"] = {"sample": {"material": "p_sample"}}
    return [(_cfg(picard_sweeps=2), r"timing\.picard_sweeps = 2 together with timing\.sweep_tables"),
            (aniso, r"mats\.p_sample\.k_aniso together with timing\.sweep_tables"),
            (aniso2, r"mats\.p_sample\.k_aniso together with timing\.sweep_tables.*timing\.aniso_tables"),
            (src, r"heating\.source together with timing\.sweep_tables"),
            (src2, r"heating\.source together with timing\.sweep_tables.*heating\.source\.sweeps"),
            (mon, r"monitors together with timing\.sweep_tables"),
            (mon2, r"monitors together with timing\.sweep_tables.*timing\.sweep_monitors"),
            (_cfg(table_tangents=True), r"timing\.table_tangents together with timing\.sweep_tables")]


def test_with_the_key_every_refusal_names_both_keys(small, tmp_path):
    from heatflow_amd import parameter_sweep as ps

    _, _, mesh = small
    for cfg, pat in _refusals():
        with pytest.raises(ValueError, match="run_kappa_sweep: " + pat):
            ps.run_kappa_sweep(cfg, str(tmp_path), [3.8], str(tmp_path))
        p = tmp_path / "c.yaml"
        p.write_text(yaml.safe_dump(cfg))
        with pytest.raises(ValueError, match="run_parameter_sweep: " + pat):
            ps.run_parameter_sweep(str(p), str(tmp_path), [1e-5, 1e-5], [3.8, 3.8], [1.84e-6, 1.84e-6], 1)
        be = Recorder(len(mesh.coords))
        with pytest.raises(ValueError, match=r"run_batch \(the batched loop\): " + pat):
            _session(mesh, be).run_batch([cfg, cfg], [None, None], None)
        assert be.calls == []
    # a k range over a material that carries its own conductivity table
    tab = _cfg()
    tab["mats"]["p_sample"]["k_power"] = {"T_ref": 300.0, "exponent": 1.0, "T_min": 300.0, "T_max": 900.0, "knots": 64}
    pat = r"a k range over p_sample together with mats\.p_sample\.k_power is not supported under timing\.sweep_tables"
    with pytest.raises(ValueError, match="run_kappa_sweep: " + pat):
        ps.run_kappa_sweep(tab, str(tmp_path), [3.8], str(tmp_path))
    p = tmp_path / "t.yaml"
    p.write_text(yaml.safe_dump(tab))
    with pytest.raises(ValueError, match="run_parameter_sweep: " + pat):
        ps.run_parameter_sweep(str(p), str(tmp_path), [1e-5, 1e-5], [3.8, 3.8], [1.84e-6, 1.84e-6], 1)
    # a configuration without tables is untouched by the key
    plain = copy.deepcopy(load_cfg("geballe_with_diamond"))
    plain["timing"]["sweep_tables"] = True
    plain["monitors"] = {"sample": {"material": "p_sample"}}
    kappa_t.check_sweep_tables(plain, "anywhere")


def test_run_batch_names_the_material_whose_tables_differ(small):
    from heatflow_amd.parameter_sweep import get_watcher_points

    _, _, mesh = small
    a, b = _cfg(), _cfg()
    b["mats"]["o_ins"]["k_power"]["exponent"] = 0.5
    be = Recorder(len(mesh.coords))
    with pytest.raises(ValueError, match=r"run_batch: .*timing\.sweep_tables.*material o_ins"):
        _session(mesh, be).run_batch([a, b], _stacks([a, b]), get_watcher_points(a))
    assert "batch_begin" not in be.calls
    c = _cfg()
    c["mats"]["p_ins"]["k"] = 12.0                  # the constant of a k_power material is the table's value at T_ref
    with pytest.raises(ValueError, match=r"run_batch: .*material p_ins"):
        _session(mesh, Recorder(len(mesh.coords))).run_batch([a, c], _stacks([a, c]), get_watcher_points(a))
    d = _cfg(key=False)
    with pytest.raises(ValueError, match=r"run_batch \(the batched loop\) does not support temperature-dependent conductivities"):
        _session(mesh, Recorder(len(mesh.coords))).run_batch([a, d], _stacks([a, d]), get_watcher_points(a))


def test_the_calls_of_a_batch_under_the_key(small):
    from heatflow_amd.parameter_sweep import get_watcher_points

    _, _, mesh = small
    cfgs = [_cfg(), _cfg(), _cfg(), _cfg()]
    cfgs[1]["heating"]["fwhm"] = 9.0e-6
    cfgs[2]["mats"]["p_sample"]["k"] = 4.4
    cfgs[3]["mats"]["p_sample"]["k"] = 3.2
    cfgs[3]["heating"]["fwhm"] = 9.0e-6
    be = Recorder(len(mesh.coords))
    res = _session(mesh, be).run_batch(cfgs, _stacks(cfgs), get_watcher_points(cfgs[0]))
    assert len(res) == 4 and res[0]["batch"] == 4
    k = be.calls.index("set_batch_tables")
    assert be.args[k] == (True,)
    assert be.calls[k:] == (["set_batch_tables", "batch_begin"] + ["batch_set_column_kappa"] * 4 + ["batch_set_state"] * 4 +
                            ["batch_run", "batch_end"])
    assert be.args[k + 1] == (4,) and be.kwargs[k + 1] == {"per_column_operator": 1}
    assert "batch_load_column" not in be.calls and "batch_set_affine" not in be.calls and "update_kappa" not in be.calls
    # tables before the assembly, on the problem the batch opens on
    assert be.calls.index("set_kappa_tables") < be.calls.index("assemble") < k
    tabled = {mesh.material_tags[m] for m in ("g_ins", "o_diam", "o_ins", "p_diam", "p_ins")}
    sample = mesh.material_tags["p_sample"]
    for j, want in enumerate((3.8, 3.8, 4.4, 3.2)):
        col, tags, ks = be.args[k + 2 + j]
        assert col == j and not tabled & set(tags) and sample in tags
        assert dict(zip(tags, ks))[sample] == want
    # without tables the key changes nothing: the calls of before
    plain = copy.deepcopy(load_cfg("geballe_with_diamond"))
    plain["mats"] = {k_: dict(v, mesh=float(v["mesh"]) * 8.0) for k_, v in plain["mats"].items()}
    plain["timing"] = dict(plain["timing"], num_steps=NSTEPS, t_final=NSTEPS * 7.5e-8, sweep_tables=True)
    be = Recorder(len(mesh.coords))
    _session(mesh, be).run_batch([plain, plain], _stacks([plain, plain]), get_watcher_points(plain))
    k = be.calls.index("batch_begin")
    assert be.calls[k:] == ["batch_begin", "batch_set_state", "batch_set_state", "batch_run", "batch_end"]
    assert "set_batch_tables" not in be.calls


def test_the_problem_key_carries_the_switch(small):
    _, _, mesh = small
    cfg = _cfg()
    s = _session(mesh, Recorder(len(mesh.coords)))
    stack = _stacks([cfg])[0]
    spec = s.spec(cfg, stack)
    assert spec.tabled and not spec.batch_tables
    off, on = spec.key, dataclasses.replace(spec, batch_tables=True).key
    assert on != off and on[:len(off)] == off and on[-1] == ("batch_tables",)
    # the switch is the batch's to set: it is no keyword of the problem
    assert dataclasses.replace(spec, batch_tables=True).problem_kwargs() == spec.problem_kwargs()
    # a problem made for a single run under the same tables is not reused by the batch
    from heatflow_amd.parameter_sweep import get_watcher_points

    be = Recorder(len(mesh.coords))
    sess = _session(mesh, be)
    sess.prepare(cfg, stack)
    first = be.calls.count("set_mesh")
    sess.run_batch([cfg, cfg], [stack, stack], get_watcher_points(cfg))
    assert be.calls.count("set_mesh") == first + 1


def test_used_config_round_trips_the_key():
    from heatflow_amd.driver import _with_scheme

    on, off = _with_scheme(_cfg()), _with_scheme(_cfg(key=False))
    assert on["timing"]["sweep_tables"] is True and "sweep_tables" not in off["timing"]
    again = yaml.safe_load(yaml.safe_dump(on))
    assert kappa_t.sweep_tables(again) is True and again["timing"]["picard_sweeps"] == 1
    assert _with_scheme(again)["timing"] == on["timing"]


def test_header_and_backend_list_the_new_entry_points():
    from heatflow_amd import hip_backend

    with open(os.path.join(ROOT, "include", "heatflow_hip.h")) as f:
        header = f.read()
    for name, args in (("hf_set_batch_tables", r"hf_ctx\* ctx, int32_t on"),
                       ("hf_batch_set_column_kappa", r"hf_ctx\* ctx, int32_t j, int32_t n_tags, const int32_t\* tags, const double\* k"),
                       ("hf_batch_revalue", r"hf_ctx\* ctx, int32_t max_workgroups"),
                       ("hf_batch_get_operator", r"hf_ctx\* ctx, int32_t j, double\* A, double\* dinv, double\* lift, double\* M")):
        assert re.search(r"int " + name + r"\(" + args + r"\);", header), name
        assert name in hip_backend.EXPORTS
    for method in ("set_batch_tables", "batch_set_column_kappa", "batch_revalue", "batch_get_operator"):
        assert callable(getattr(hip_backend.HeatflowHIP, method))
