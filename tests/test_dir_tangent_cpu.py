"""Tangents and fits in k_r and k_z of anisotropic materials, without a GPU: the restated recursion
(dir_tangent_oracle.py) against its own identities and finite differences, the parameter names of the drivers and the fit,
HeatProblem's calls, every Python refusal, the header, and a synthetic fit of p_sample.k_z."""
import copy
import json
import os
import re

import numpy as np
import pytest

from aniso_oracle import mixed_multipliers
from conftest import ROOT, load_cfg
from dir_tangent_oracle import DirTangentOracleBackend, directional_element_matrices
from helpers import make_problem
from oracle import heat_oracle as ho

NSTEPS = 40
DIRECTIONAL = ("p_sample.k_r", "p_sample.k_z", "p_ins.k_r", "p_ins.k_z")


def _nodes(mesh):
    return np.linspace(0, len(mesh.coords) - 1, 50).astype(np.int32)


def _kind_tag(mesh, name):
    mat, suffix = name.rsplit(".", 1)
    return mesh.material_tags[mat], {"k": "k", "k_r": "r", "k_z": "z"}[suffix]


def _problem(case, aniso, **kw):
    cfg, stack, mesh = case
    return make_problem(cfg, stack, mesh, backend=DirTangentOracleBackend(), **({"k_aniso": aniso} if aniso else {}), **kw)


def _tangents(case, aniso, names, nsteps=NSTEPS, **kw):
    """(samples, {name: tangent samples n_steps x n_s}) of one run of the restated recursion."""
    _, _, mesh = case
    prob = _problem(case, aniso, **kw)
    cond = [[_kind_tag(mesh, nm)] for nm in names]
    _, s, ts, _, _ = prob.run_tangent(nsteps, _nodes(mesh), conductivity=cond, time_varying=[prob.bcs[3]])
    return s, {nm: ts[:, j] for j, nm in enumerate(names)}


def _primal(case, aniso, nsteps=NSTEPS):
    _, _, mesh = case
    prob = _problem(case, aniso)
    return prob.run(nsteps, _nodes(mesh), time_varying=[prob.bcs[3]])[1]


def test_euler_identity_on_the_restatement(case_with_diamond_small):
    """kappa d/dkappa = k_r d/dk_r + k_z d/dk_z, i.e. s_kappa = m_r s_kr + m_z s_kz, per anisotropic tag."""
    _, _, mesh = case_with_diamond_small
    aniso = mixed_multipliers(mesh)
    for mat in ("p_sample", "p_ins"):
        m_r, m_z = aniso[mesh.material_tags[mat]]
        # (two runs: a tag's kappa column and its directional ones do not share a set-up)
        _, t = _tangents(case_with_diamond_small, aniso, (f"{mat}.k",))
        t.update(_tangents(case_with_diamond_small, aniso, (f"{mat}.k_r", f"{mat}.k_z"))[1])
        sk, sr, sz = t[f"{mat}.k"], t[f"{mat}.k_r"], t[f"{mat}.k_z"]
        err = np.max(np.abs(sk - (m_r * sr + m_z * sz))) / np.max(np.abs(sk))
        print(f"{mat}: Euler identity off by {err:.2e} of max|s_kappa|")
        assert np.max(np.abs(sk)) > 0 and err <= 1e-12        # (measured 1.4e-14: two LU solves' rounding)


def test_recursion_matches_the_fourth_order_quotient_of_primal_runs(case_with_diamond_small):
    """(8 (u(+h) - u(-h)) - (u(+2h) - u(-2h))) / (12 h m k) of runs at multipliers m (1 +- h), m (1 +- 2h), h = 1e-2."""
    cfg, _, mesh = case_with_diamond_small
    aniso = mixed_multipliers(mesh)
    _, tan = _tangents(case_with_diamond_small, aniso, DIRECTIONAL)
    h = 1e-2
    for name in DIRECTIONAL:
        tag, kind = _kind_tag(mesh, name)
        q = 0 if kind == "r" else 1
        runs = {}
        for f in (-2, -1, 1, 2):
            a = dict(aniso)
            m = list(a[tag])
            m[q] *= 1.0 + f * h
            a[tag] = tuple(m)
            runs[f] = _primal(case_with_diamond_small, a)
        k_dir = float(cfg["mats"][name.rsplit(".", 1)[0]]["k"]) * aniso[tag][q]
        fd4 = (8.0 * (runs[1] - runs[-1]) - (runs[2] - runs[-2])) / (12.0 * h * k_dir)
        fd2 = (runs[1] - runs[-1]) / (2.0 * h * k_dir)
        scale = np.max(np.abs(tan[name]))
        e4, e2 = np.max(np.abs(tan[name] - fd4)) / scale, np.max(np.abs(tan[name] - fd2)) / scale
        print(f"{name}: max|s| k_dir = {scale * k_dir:.3g} K; 4th-order quotient off by {e4:.2e}, 2nd-order by {e2:.2e} of max|s|")
        assert scale > 0 and e4 <= 1e-7        # (measured <= 1.5e-8; the truncation error of the quotient at h = 1e-2)


def test_directional_stiffness_annihilates_fields_linear_in_the_other_coordinate(case_with_diamond_small):
    """K^r u = 0 for u linear in z, K^z u = 0 for u linear in r, to rounding: the P1 gradient of a linear field is exact."""
    _, _, mesh = case_with_diamond_small
    Ke_r, Ke_z = directional_element_matrices(mesh.coords, mesh.tris)
    n = len(mesh.coords)
    z, r = mesh.coords[:, 0], mesh.coords[:, 1]
    for Ke, lin, other in ((Ke_r, 300.0 + 2e7 * z, 300.0 + 2e7 * r), (Ke_z, 300.0 + 2e7 * r, 300.0 + 2e7 * z)):
        K, Kabs = ho.assemble_csr(n, mesh.tris, Ke), ho.assemble_csr(n, mesh.tris, np.abs(Ke))
        bound = 1e-13 * (Kabs @ np.abs(lin))
        assert np.all(np.abs(K @ lin) <= bound)
        assert np.max(np.abs(K @ other) / (Kabs @ np.abs(other))) > 1e-6      # ... and does see the other one


def test_parameter_names_are_parsed():
    from heatflow_amd.aniso import split_param

    assert split_param("p_sample") == ("p_sample", None)
    assert split_param("p_sample.k") == ("p_sample", "k")
    assert split_param("p_sample.k_r") == ("p_sample", "r")
    assert split_param("o_ins.k_z") == ("o_ins", "z")
    with pytest.raises(ValueError, match=r"p_sample\.k_x"):
        split_param("p_sample.k_x")


def test_get_param_and_set_params_round_trip():
    from heatflow_amd.fit import get_param, set_params

    cfg = load_cfg("geballe_with_diamond_aniso")
    k = float(cfg["mats"]["p_ins"]["k"])
    assert cfg["mats"]["p_ins"]["k_aniso"] == {"r": 2.0, "z": 0.25}
    assert get_param(cfg, "p_ins.k_r") == k * 2.0 and get_param(cfg, "p_ins.k_z") == k * 0.25 and get_param(cfg, "p_ins.k") == k
    c = set_params(cfg, ("p_ins.k_z", "p_sample.k_r", "o_ins.k"), (3.0, 5.0, 7.0))
    assert c["mats"]["p_ins"]["k_aniso"] == {"r": 2.0, "z": 3.0 / k} and c["mats"]["p_ins"]["k"] == k
    ks = float(cfg["mats"]["p_sample"]["k"])
    assert "k_aniso" not in cfg["mats"]["p_sample"]                       # the block is created, the input left alone
    assert c["mats"]["p_sample"]["k_aniso"] == {"r": 5.0 / ks}
    assert get_param(c, "p_sample.k_r") == pytest.approx(5.0, rel=1e-15) and get_param(c, "p_sample.k_z") == ks
    assert c["mats"]["o_ins"]["k"] == 7.0 and c["mats"]["o_ins"]["k_aniso"] == {"r": 2.0, "z": 0.25}
    # k and a direction of one material in either order: the directional value holds
    for order in ((("p_ins.k", 20.0), ("p_ins.k_r", 30.0)), (("p_ins.k_r", 30.0), ("p_ins.k", 20.0))):
        c = set_params(cfg, [o[0] for o in order], [o[1] for o in order])
        assert get_param(c, "p_ins.k") == 20.0 and get_param(c, "p_ins.k_r") == pytest.approx(30.0, rel=1e-15)
    with pytest.raises(ValueError, match=r"p_ins\.k_y"):
        get_param(cfg, "p_ins.k_y")
    with pytest.raises(ValueError, match="nothing"):
        set_params(cfg, ("nothing.k_r",), (1.0,))
    assert get_param(cfg, "fwhm") == float(cfg["heating"]["fwhm"]) and get_param(cfg, "p_sample") == ks


class RecordingBackend(DirTangentOracleBackend):
    def __init__(self):
        super().__init__()
        self.calls = []

    def tangent_setup(self, n_par, tag_col):
        self.calls.append(("tangent_setup", n_par, dict(tag_col)))
        super().tangent_setup(n_par, tag_col)

    def tangent_setup_dir(self, n_par, k=None, r=None, z=None):
        self.calls.append(("tangent_setup_dir", n_par, dict(k or {}), dict(r or {}), dict(z or {})))
        super().tangent_setup_dir(n_par, k, r, z)


def test_heat_problem_makes_todays_call_for_plain_tags_and_the_directional_one_for_pairs(case_with_diamond_small):
    cfg, stack, mesh = case_with_diamond_small
    t = mesh.material_tags
    be = RecordingBackend()
    prob = make_problem(cfg, stack, mesh, backend=be, k_aniso=mixed_multipliers(mesh))
    nodes = [0, 5]
    prob.run_tangent(2, nodes, conductivity=[[t["p_coupler"], t["o_coupler"]], [t["gasket"]]])
    assert be.calls == [("tangent_setup", 2, {t["p_coupler"]: 0, t["o_coupler"]: 0, t["gasket"]: 1})]
    prob.run_tangent(2, nodes, conductivity=[[t["p_coupler"], t["o_coupler"]], [t["gasket"]]])     # the same spec: no new set-up
    assert len(be.calls) == 1
    cond = [[(t["p_sample"], "r")], [(t["p_sample"], "z")], [(t["p_ins"], "z"), (t["o_ins"], "z")], [t["p_coupler"]], [(t["g_ins"], "k")]]
    prob.run_tangent(2, nodes, conductivity=cond)
    assert be.calls[1] == ("tangent_setup_dir", 5, {t["p_coupler"]: 3, t["g_ins"]: 4}, {t["p_sample"]: 0},
                           {t["p_sample"]: 1, t["p_ins"]: 2, t["o_ins"]: 2})
    prob.run_tangent(2, nodes, conductivity=cond)
    assert len(be.calls) == 2
    prob.run_tangent(2, nodes, conductivity=[[t["gasket"]]])
    assert be.calls[2] == ("tangent_setup", 1, {t["gasket"]: 0})
    assert prob.tangent_load(0).shape == (prob.n,)
    for bad, msg in (([[(t["p_ins"], "r")], [(t["p_ins"], "r")]], "two conductivity columns"),
                     ([[(t["p_ins"], "k")], [(t["p_ins"], "z")]], "kappa column and a directional"),
                     ([[(t["p_ins"], "z")], [t["p_ins"]]], "kappa column and a directional"),
                     ([[(t["p_ins"], "x")]], "unknown kind")):
        with pytest.raises(ValueError, match=msg):
            prob.run_tangent(2, nodes, conductivity=bad)
    assert len(be.calls) == 3


def _session(mesh, backend=None):
    from heatflow_amd.driver import SimulationSession

    return SimulationSession(mesh.coords, mesh.tris, mesh.tags, mesh.material_tags, backend=backend or DirTangentOracleBackend(),
                             precond=0)


@pytest.fixture(scope="module")
def aniso_cfg():
    from heatflow_amd.geometry import scale_mesh_sizes

    cfg = scale_mesh_sizes(load_cfg("geballe_with_diamond_aniso"), 8.0)
    cfg["timing"]["num_steps"] = 30
    return cfg


def test_session_names_and_refusals(case_with_diamond_small, aniso_cfg, tmp_path):
    from heatflow_amd import fit
    from heatflow_amd.geometry import build_stack
    from heatflow_amd.parameter_sweep import get_watcher_points

    _, _, mesh = case_with_diamond_small
    cfg = aniso_cfg
    stack, wp = build_stack(cfg), get_watcher_points(cfg)
    s = _session(mesh)
    try:
        names = ["p_sample.k_z", "p_ins.k_r", "p_ins.k_z", "o_ins.k", "p_coupler.k", "fwhm"]
        res = s.run(cfg, stack, wp, tangents=names)
        assert list(res["tangents"]) == names and res["tangent_iters"].shape == (30, len(names))
        for nm in names:
            assert set(res["tangents"][nm]) == set(res["watcher_names"])
            assert np.max(np.abs(res["tangents"][nm]["oside"])) > 0
        # "<m>.k" of an isotropic material is the bare name's derivative
        iso = s.run(cfg, stack, wp, tangents=["p_coupler"])
        np.testing.assert_allclose(iso["tangents"]["p_coupler"]["oside"], res["tangents"]["p_coupler.k"]["oside"], rtol=0,
                                   atol=1e-12 * np.max(np.abs(iso["tangents"]["p_coupler"]["oside"])))
        # the refusals: a bare anisotropic material as before, an unknown suffix, an unknown material
        with pytest.raises(ValueError, match=r"tangent.*mats\.p_ins\.k_aniso"):
            s.run(cfg, stack, wp, tangents=["p_sample", "p_ins"])
        with pytest.raises(ValueError, match=r"p_ins\.k_q"):
            s.run(cfg, stack, wp, tangents=["p_ins.k_q"])
        with pytest.raises(ValueError, match=r"unknown parameter 'nothing\.k_r'"):
            s.run(cfg, stack, wp, tangents=["nothing.k_r"])
        with pytest.raises(ValueError, match="kappa column and a directional"):
            s.run(cfg, stack, wp, tangents=["p_ins.k", "p_ins.k_z"])
    finally:
        s.close()
    with pytest.raises(ValueError, match=r"fit.*mats\.o_ins\.k_aniso"):
        fit.fit_parameters(cfg, str(tmp_path), params=("o_ins",))
    with pytest.raises(ValueError, match=r"o_ins\.k_q"):
        fit.fit_parameters(cfg, str(tmp_path), params=("o_ins.k_q",))
    with pytest.raises(ValueError, match=r"nothing"):
        fit.fit_parameters(cfg, str(tmp_path), params=("nothing.k_z",))


def test_session_tangent_matches_central_differences_of_session_runs(case_with_diamond_small, aniso_cfg):
    """The driver's whole chain for one name: set_params -> stack -> k_aniso of the problem -> run, against the tangent."""
    from heatflow_amd.fit import get_param, set_params
    from heatflow_amd.geometry import build_stack
    from heatflow_amd.parameter_sweep import get_watcher_points

    _, _, mesh = case_with_diamond_small
    cfg = aniso_cfg
    s = _session(mesh)
    try:
        for name in ("p_ins.k_z", "p_sample.k_z"):           # the second creates the k_aniso block
            res = s.run(cfg, build_stack(cfg), get_watcher_points(cfg), tangents=[name])
            base = get_param(cfg, name)
            curves = []
            for sgn in (1, -1):
                c = set_params(cfg, (name,), (base * (1 + sgn * 1e-4),))
                curves.append(s.run(c, build_stack(c), get_watcher_points(c))["watchers"]["oside"])
            fd = (curves[0] - curves[1]) / (2e-4 * base)
            tan = res["tangents"][name]["oside"]
            assert np.max(np.abs(tan)) > 0 and np.max(np.abs(tan - fd)) <= 1e-4 * np.max(np.abs(tan))
    finally:
        s.close()


def test_header_declares_and_backend_lists_the_entry_points():
    from heatflow_amd import hip_backend
    from test_cabi import _declared_symbols

    declared = _declared_symbols()
    for name in ("hf_tangent_setup_dir", "hf_tangent_load"):
        assert name in declared and name in hip_backend.EXPORTS
    assert sorted(declared) == sorted(hip_backend.EXPORTS)
    with open(os.path.join(ROOT, "include", "heatflow_hip.h")) as f:
        text = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    assert re.search(r"int\s+hf_tangent_setup_dir\(hf_ctx\*\s*ctx,\s*int32_t\s+n_par,\s*const int32_t\*\s*tag_col_k,\s*"
                     r"const int32_t\*\s*tag_col_r,\s*const int32_t\*\s*tag_col_z\);", text)
    assert re.search(r"int\s+hf_tangent_load\(hf_ctx\*\s*ctx,\s*int32_t\s+j,\s*double\*\s*F\);", text)
    assert callable(hip_backend.HeatflowHIP.tangent_setup_dir) and callable(hip_backend.HeatflowHIP.tangent_load)


def _synthetic(cfg, mesh, name, value):
    from heatflow_amd.fit import set_params
    from heatflow_amd.parameter_sweep import build_stack, get_watcher_points

    s = _session(mesh)
    try:
        c = set_params(cfg, (name,), (value,))
        res = s.run(c, build_stack(c), get_watcher_points(c))
    finally:
        s.close()
    return {"time": res["times"], "temp": res["watchers"]["pside"], "oside": res["watchers"]["oside"]}


def test_fit_recovers_k_z_of_the_sample_from_synthetic_data(case_with_diamond_small, aniso_cfg):
    """p_sample.k_z is identifiable from the normalised o-side curve: data made at 1.2 x the configured value come back."""
    from heatflow_amd.fit import fit_parameters, get_param

    _, _, mesh = case_with_diamond_small
    cfg = aniso_cfg
    k0 = get_param(cfg, "p_sample.k_z")
    exp = _synthetic(cfg, mesh, "p_sample.k_z", 1.2 * k0)
    out = fit_parameters(cfg, None, ("p_sample.k_z",), exp, x0=[k0], max_iter=40, backend=DirTangentOracleBackend(),
                         mesh=(mesh.coords, mesh.tris, mesh.tags, mesh.material_tags))
    print(f"fit of p_sample.k_z: {out['values'][0] / (1.2 * k0) - 1:.2e} off, {out['iterations']} iterations, rmse {out['rmse']:.2e}")
    assert abs(out["values"][0] / (1.2 * k0) - 1) <= 1e-6, out["history"]
    assert out["converged"] and out["rmse"] < 1e-8 and np.isfinite(out["stderr"][0])
    assert out["params"] == ["p_sample.k_z"]


def test_fit_cli_writes_the_fitted_k_aniso(case_with_diamond_small, aniso_cfg, tmp_path):
    import yaml

    from heatflow_amd.fit import get_param, main

    _, _, mesh = case_with_diamond_small
    cfg = copy.deepcopy(aniso_cfg)
    path = tmp_path / "cfg.yaml"
    path.write_text(yaml.safe_dump(cfg))
    out_dir = tmp_path / "out"
    assert main(["--config", str(path), "--params", "p_sample.k_z", "fwhm", "--output-dir", str(out_dir), "--max-iter", "2"],
                backend=DirTangentOracleBackend()) == 0
    summary = json.loads((out_dir / "fit_summary.json").read_text())
    assert summary["params"] == ["p_sample.k_z", "fwhm"] and len(summary["values"]) == 2
    used = yaml.safe_load((out_dir / "used_config.yaml").read_text())
    assert get_param(used, "p_sample.k_z") == pytest.approx(summary["values"][0], rel=1e-12)
    assert used["mats"]["p_sample"]["k_aniso"]["z"] == pytest.approx(summary["values"][0] / float(cfg["mats"]["p_sample"]["k"]), rel=1e-12)
    assert used["heating"]["fwhm"] == pytest.approx(summary["values"][1], rel=1e-12)
    assert used["mats"]["p_ins"]["k_aniso"] == {"r": 2.0, "z": 0.25}
