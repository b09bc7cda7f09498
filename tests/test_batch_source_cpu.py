"""Sweeps under the laser-power source with per-point region monitors, without a GPU: the opt-in keys
``heating.source.sweeps`` and ``timing.sweep_monitors``, the refusals that stay without them, what the configurations of a batch must
share, the per-column amplitudes, every column of SimulationSession.run_batch against a single run on the same scipy stand-in, the
calls a batch makes, and run_parameter_sweep's monitors.csv per point."""
import copy
import csv
import os

import numpy as np
import pytest
import yaml

from batch_source_backends import BatchSourceOracleBackend, RecordingBatchBackend
from conftest import build_case, load_cfg

from heatflow_amd import monitors as mon_mod
from heatflow_amd import source as src_mod

NSTEPS = 8
MONITORS = {"sample": {"material": "p_sample", "above": 300.5}, "coupler": {"material": ["p_coupler", "o_coupler"]}}


@pytest.fixture(scope="module")
def small():
    return build_case("geballe_with_diamond", 8.0)


def _cfg(sweeps=True, monitors=True, sweep_monitors=True, **source):
    cfg = copy.deepcopy(load_cfg("geballe_with_diamond_source"))
    cfg["mats"] = {k: dict(v, mesh=float(v["mesh"]) * 8.0) for k, v in cfg["mats"].items()}
    cfg["timing"] = dict(cfg["timing"], num_steps=NSTEPS, t_final=NSTEPS * 7.5e-8)
    cfg["heating"]["source"].update(power=2.0, pulse={"t0": 3.0e-7, "fwhm": 3.0e-7})
    cfg["heating"]["source"].update(source)
    if sweeps:
        cfg["heating"]["source"]["sweeps"] = True
    if monitors:
        cfg["monitors"] = copy.deepcopy(MONITORS)
    if sweep_monitors:
        cfg["timing"]["sweep_monitors"] = True
    return cfg


def _session(mesh, backend=None):
    from heatflow_amd.driver import SimulationSession

    return SimulationSession(mesh.coords, mesh.tris, mesh.tags, mesh.material_tags, backend=backend or BatchSourceOracleBackend())


def _stacks(cfgs):
    from heatflow_amd.geometry import build_stack

    return [build_stack(c) for c in cfgs]


# ---- the keys ---------------------------------------------------------------------------------------------------------------------
def test_parse_source_takes_sweeps_and_writes_it_only_when_true():
    assert "sweeps" in src_mod.SOURCE_KEYS
    on, off = src_mod.parse_source(_cfg()), src_mod.parse_source(_cfg(sweeps=False))
    assert on.sweeps is True and off.sweeps is False
    assert on.used_config()["sweeps"] is True and "sweeps" not in off.used_config()
    explicit = _cfg(sweeps=False)
    explicit["heating"]["source"]["sweeps"] = False
    assert "sweeps" not in src_mod.parse_source(explicit).used_config()
    explicit["heating"]["source"]["sweeps"] = "yes"
    with pytest.raises(ValueError, match=r"heating\.source\.sweeps must be true or false"):
        src_mod.parse_source(explicit)
    assert src_mod.source_permits_sweeps(_cfg()) and not src_mod.source_permits_sweeps(_cfg(sweeps=False))
    assert not src_mod.source_permits_sweeps(load_cfg("geballe_with_diamond"))
    assert mon_mod.sweep_monitors(_cfg()) is True and mon_mod.sweep_monitors(_cfg(sweep_monitors=False)) is False
    bad = _cfg()
    bad["timing"]["sweep_monitors"] = 1
    with pytest.raises(ValueError, match=r"timing\.sweep_monitors must be true or false"):
        mon_mod.sweep_monitors(bad)


def test_the_sweeps_and_run_batch_refuse_without_the_keys_and_accept_with_them(small, tmp_path):
    from heatflow_amd import parameter_sweep as ps

    _, _, mesh = small
    src_pat = r" does not support the volumetric source \(heating\.source\)"
    mon_pat = r" does not support region monitors \(monitors\)"
    for cfg, pat in ((_cfg(sweeps=False, monitors=False, sweep_monitors=False), src_pat), (_cfg(sweep_monitors=False), mon_pat)):
        with pytest.raises(ValueError, match="run_kappa_sweep" + pat):
            ps.run_kappa_sweep(cfg, str(tmp_path), [3.8], str(tmp_path))
        p = tmp_path / "c.yaml"
        p.write_text(yaml.safe_dump(cfg))
        with pytest.raises(ValueError, match="run_parameter_sweep" + pat):
            ps.run_parameter_sweep(str(p), str(tmp_path), [1e-5, 1e-5], [3.8, 3.8], [1.84e-6, 1.84e-6], 1)
        be = RecordingBatchBackend(len(mesh.coords), int(mesh.tags.max()) + 1)
        with pytest.raises(ValueError, match=r"run_batch \(the batched loop\)" + pat):
            _session(mesh, be).run_batch([cfg, cfg], _stacks([cfg, cfg]), ps.get_watcher_points(cfg))
        assert be.calls == []
    # with the keys: run_batch runs, and so do both sweeps (below: test_run_parameter_sweep_..., and the kappa sweep here)
    cfg = _cfg()
    res = _session(mesh).run_batch([cfg, cfg], _stacks([cfg, cfg]), ps.get_watcher_points(cfg))
    assert len(res) == 2 and "monitors" in res[0]
    rows = ps.run_kappa_sweep(cfg, str(tmp_path / "mesh"), [3.6, 4.0], str(tmp_path / "kappa"), rebuild_mesh=True, batch=2,
                              session_factory=lambda c, t, g, m, pattern=None: _session_from(c, t, g, m))
    assert [r["status"] for r in rows] == ["success", "success"] and all(r.get("batch") == 2 for r in rows)
    for k in ("3.60", "4.00"):
        assert os.path.isfile(tmp_path / "kappa" / k / "monitors.csv")
    # the remaining refusals stay: tables, tangents=, the fit with monitors, the 1-D model, two_sided
    from heatflow_amd import fit, run_no_diamond_1d

    mcfg = copy.deepcopy(load_cfg("geballe_with_diamond"))
    mcfg["monitors"] = copy.deepcopy(MONITORS)
    mcfg["timing"]["sweep_monitors"] = True
    with pytest.raises(ValueError, match=r"heatflow_amd\.fit" + mon_pat):
        fit.fit_parameters(mcfg, str(tmp_path))
    nd = copy.deepcopy(load_cfg("geballe_no_diamond"))
    nd["monitors"] = {"sample": {"material": "p_sample"}}
    nd["timing"]["sweep_monitors"] = True
    with pytest.raises(ValueError, match=r"run_1d \(the 1-D model\)" + mon_pat):
        run_no_diamond_1d.run_1d(nd, str(tmp_path))
    with pytest.raises(ValueError, match=r"tangents=" + src_pat):
        _session(mesh).run(cfg, _stacks([cfg])[0], ps.get_watcher_points(cfg), tangents=["p_sample"])
    with pytest.raises(ValueError, match=r"two_sided=True.*" + src_pat):
        _session(mesh).run(cfg, _stacks([cfg])[0], ps.get_watcher_points(cfg), two_sided=True)
    tab = _cfg()
    tab["mats"]["p_sample"]["k_power"] = {"T_ref": 300.0, "exponent": 1.0, "T_min": 300.0, "T_max": 900.0, "knots": 64}
    with pytest.raises(ValueError, match=r"run_batch \(the batched loop\) does not support temperature-dependent conductivities"):
        _session(mesh).run_batch([tab, tab], _stacks([cfg, cfg]), ps.get_watcher_points(cfg))


def _session_from(coords, tris, tags, tag_map):
    from heatflow_amd.driver import SimulationSession

    return SimulationSession(coords, tris, tags, tag_map, backend=BatchSourceOracleBackend())


def test_run_batch_names_what_the_configurations_do_not_share(small):
    from heatflow_amd.parameter_sweep import get_watcher_points

    _, _, mesh = small
    a = _cfg()
    wp = get_watcher_points(a)

    def refused(b, pat):
        be = RecordingBatchBackend(len(mesh.coords), int(mesh.tags.max()) + 1)
        with pytest.raises(ValueError, match=pat):
            _session(mesh, be).run_batch([a, b], _stacks([a, b]), wp)
        assert "batch_begin" not in be.calls

    refused(_cfg(material=["p_coupler", "p_ins"]), r"run_batch: .*heating\.source\.material")
    refused(_cfg(face="inner"), r"run_batch: .*heating\.source\.face")
    refused(_cfg(keep_line=True), r"run_batch: .*heating\.source\.keep_line")
    other = _cfg()
    other["monitors"]["sample"]["above"] = 301.0
    refused(other, r"run_batch: .*monitors block")
    none = _cfg(monitors=False)
    refused(none, r"run_batch: .*monitors block")
    plain = copy.deepcopy(load_cfg("geballe_with_diamond"))
    plain["mats"] = a["mats"]
    plain["timing"] = dict(a["timing"])
    plain["monitors"] = copy.deepcopy(MONITORS)
    refused(plain, r"run_batch: .*heating\.source block")


# ---- run_batch against single runs on the same stand-in -----------------------------------------------------------------------------
def _columns():
    """Four columns that differ in power, beam fwhm (two share it), depth and pulse."""
    return [_cfg(), _cfg(power=4.0, pulse={"t0": 2.0e-7, "fwhm": 2.5e-7}), _cfg(fwhm=9.0e-6, depth=4.0e-8), _cfg(fwhm=2.0e-5, power=8.0)]


def test_every_column_equals_a_single_run_and_the_amplitudes_are_each_columns_own(small):
    from heatflow_amd.parameter_sweep import get_watcher_points

    _, _, mesh = small
    cfgs = _columns()
    stacks = _stacks(cfgs)
    wp = get_watcher_points(cfgs[0])
    be = BatchSourceOracleBackend()
    res = _session(mesh, be).run_batch(cfgs, stacks, wp)
    # the calls: one source of four columns, then one table of amplitudes; equal (fwhm, depth) download once
    (name, tags, fwhm, z0, depth), (name2, amp) = [c for c in be.calls if c[0].startswith("batch_set_source")]
    assert name == "batch_set_source" and tags == [mesh.material_tags["p_coupler"]]
    assert list(fwhm) == [1.32e-5, 1.32e-5, 9.0e-6, 2.0e-5] and list(depth) == [2.0e-8, 2.0e-8, 4.0e-8, 2.0e-8]
    assert be.batch_source_downloads == 3
    assert name2 == "batch_set_source_amplitudes" and amp.shape == (NSTEPS, 4)
    times = (np.arange(NSTEPS) + 1) * 7.5e-8
    import source_oracle as so
    for j, (c, st) in enumerate(zip(cfgs, stacks)):
        spec = src_mod.parse_source(c)
        F1 = so.source_vector(mesh.coords, mesh.tris, mesh.tags, tags, spec.fwhm, spec.z0(st), spec.depth)[0]
        assert np.array_equal(amp[:, j], src_mod.amplitudes(spec, times, F1)), j
    assert amp[:, 1].max() != amp[:, 0].max() and np.argmax(amp[:, 1]) != np.argmax(amp[:, 0])
    # every column against its own single run on a fresh stand-in of the same kind: the same arithmetic, the same bits
    for j, (c, st) in enumerate(zip(cfgs, stacks)):
        one = _session(mesh).run(c, st, wp)
        assert res[j]["watcher_names"] == one["watcher_names"] and np.array_equal(res[j]["times"], one["times"])
        for nm in one["watchers"]:
            assert np.array_equal(res[j]["watchers"][nm], one["watchers"][nm]), (j, nm)
        assert list(res[j]["monitors"]) == list(one["monitors"]) == ["sample", "coupler"]
        for region, fields in one["monitors"].items():
            assert set(res[j]["monitors"][region]) == set(fields)
            for field, v in fields.items():
                assert np.array_equal(res[j]["monitors"][region][field], v), (j, region, field)
        assert "energy" in res[j]["monitors"]["coupler"] and "hot_volume" in res[j]["monitors"]["sample"]
    peaks = [r["monitors"]["coupler"]["T_max"].max() for r in res]
    assert min(peaks) > 301.0 and len(set(peaks)) == 4


def test_columns_that_differ_in_k_of_the_sample_too(small):
    from heatflow_amd.parameter_sweep import get_watcher_points

    _, _, mesh = small
    cfgs = [_cfg(), _cfg(power=3.0)]
    cfgs[1]["mats"]["p_sample"]["k"] = 4.4
    stacks = _stacks(cfgs)
    wp = get_watcher_points(cfgs[0])
    be = BatchSourceOracleBackend()
    res = _session(mesh, be).run_batch(cfgs, stacks, wp)
    assert getattr(be, "batch_affine_calls", 0) == 1
    for j in range(2):
        one = _session(mesh).run(cfgs[j], stacks[j], wp)
        for nm in one["watchers"]:
            assert np.allclose(res[j]["watchers"][nm], one["watchers"][nm], rtol=0, atol=1e-9), (j, nm)
        assert np.allclose(res[j]["monitors"]["sample"]["T_mean"], one["monitors"]["sample"]["T_mean"], rtol=0, atol=1e-9)


def test_the_calls_of_a_batch_with_and_without_the_new_blocks(small):
    from heatflow_amd.parameter_sweep import get_watcher_points

    _, _, mesh = small
    ntab = int(mesh.tags.max()) + 1
    cfgs = _columns()[:2]
    be = RecordingBatchBackend(len(mesh.coords), ntab)
    res = _session(mesh, be).run_batch(cfgs, _stacks(cfgs), get_watcher_points(cfgs[0]))
    assert "set_source" not in be.calls and be.calls.count("set_monitors") == 1        # the batch's own source; the context's table
    k = be.calls.index("batch_begin")
    assert be.calls.index("set_monitors") < k
    assert be.calls[k:] == ["batch_begin", "batch_set_state", "batch_set_state", "batch_set_source", "batch_get_source",
                            "batch_set_source_amplitudes", "batch_set_monitors", "batch_run", "batch_get_monitors", "batch_end"]
    assert be.args[k + 6] == (True,) and set(res[0]["monitors"]) == {"sample", "coupler"}
    # keep_line: false - the three outer edges only; heating.file is not read
    nofile = [copy.deepcopy(c) for c in cfgs]
    for c in nofile:
        c["heating"]["file"] = "does/not/exist.csv"
    _session(mesh, RecordingBatchBackend(len(mesh.coords), ntab)).run_batch(nofile, _stacks(nofile), get_watcher_points(cfgs[0]))
    # a batch without either block makes the calls of before
    plain = copy.deepcopy(load_cfg("geballe_with_diamond"))
    plain["mats"] = cfgs[0]["mats"]
    plain["timing"] = dict(plain["timing"], num_steps=3, t_final=3 * 7.5e-8)
    be = RecordingBatchBackend(len(mesh.coords), ntab)
    res = _session(mesh, be).run_batch([plain, plain], _stacks([plain, plain]), get_watcher_points(plain))
    k = be.calls.index("batch_begin")
    assert be.calls[k:] == ["batch_begin", "batch_set_state", "batch_set_state", "batch_run", "batch_end"]
    assert "set_monitors" not in be.calls and "monitors" not in res[0]


# ---- the sweep ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("batch", [2, 1])
def test_run_parameter_sweep_writes_monitors_csv_per_point(tmp_path, batch):
    from heatflow_amd import parameter_sweep as ps

    cfg = _cfg()
    del cfg["heating"]["source"]["fwhm"]          # the beam follows heating.fwhm: --fwhm-range scans the beam width
    cfg_path = str(tmp_path / "base.yaml")
    with open(cfg_path, "w") as f:
        yaml.safe_dump(cfg, f)
    out = str(tmp_path / "sweep")
    ok, failed = ps.run_parameter_sweep(cfg_path, out, (8e-6, 2e-5), (3.4, 4.2), (1.84e-6, 1.84e-6), (2, 2, 1),
                                        base_mesh_folder=str(tmp_path / "meshes"), batch=batch,
                                        session_factory=lambda c, t, g, m, pattern=None: _session_from(c, t, g, m))
    assert len(ok) == 4 and not failed, failed
    with open(os.path.join(out, "successful_runs.csv"), newline="") as f:
        rows = list(csv.DictReader(f))
    assert len(rows) == 4 and [int(r["run_id"]) for r in rows] == [1, 2, 3, 4]
    assert all((r.get("batch") or "") == ("2" if batch == 2 else "") for r in rows)
    peaks = {}
    for r in rows:
        path = os.path.join(r["output_dir"], "monitors.csv")
        assert os.path.isfile(path) and os.path.isfile(os.path.join(r["output_dir"], "watcher_points.csv"))
        with open(path, newline="") as f:
            m = list(csv.reader(f))
        assert len(m) == NSTEPS + 1 and "coupler.T_max" in m[0] and "sample.hot_volume" in m[0]
        peaks[(float(r["fwhm"]), float(r["k"]))] = max(float(x[m[0].index("coupler.T_max")]) for x in m[1:])
        with open(os.path.join(r["output_dir"], "used_config.yaml")) as f:
            used = yaml.safe_load(f)
        assert used["heating"]["source"]["sweeps"] is True and used["heating"]["source"]["fwhm"] == float(r["fwhm"])
        assert used["timing"]["sweep_monitors"] is True
    # the same power through a narrower beam heats the coupler's peak more, at either k
    fw, ks = sorted({k[0] for k in peaks}), sorted({k[1] for k in peaks})
    assert len(peaks) == 4 and all(peaks[(fw[0], k)] > peaks[(fw[1], k)] > 300.0 for k in ks)
