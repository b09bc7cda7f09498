"""Heat-capacity tangents and the fit's systematic-error budget, without a GPU: the unit-capacity mass against the
oracle's element matrices, the restated recursion (capacity_tangent_oracle.py) against central differences of oracle runs, the
scaling identity sum_t (k_t s_{k_t} + c_t s_{c_t}) = 0 of Dirichlet-driven runs, the parameter names of the drivers and the fit,
HeatProblem's calls, a synthetic fit of p_sample.cv, and the budget against brute-force refits."""
import copy
import json
import os
import re

import numpy as np
import pytest

from aniso_oracle import mixed_multipliers
from capacity_tangent_oracle import FD_REL_STEP, CapacityTangentOracleBackend, identity_terms, unit_mass_matrix
from conftest import ROOT
from helpers import make_problem, material_tables
from oracle import heat_oracle as ho
from test_shape_tangent_cpu import find_step

NSTEPS = 20


def _nodes(mesh):
    return np.linspace(0, len(mesh.coords) - 1, 50).astype(np.int32)


# 1. M^1_j ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["case_with_diamond_small", "case_no_diamond_small"])
def test_unit_mass_is_the_slope_of_the_oracle_mass_in_rho_c(request, case):
    """M is linear in rho_c: the difference of the oracle's mass at two capacities of the column's tags, divided by the difference of
    the capacities, is M^1_j to rounding - 1e-14 of the largest entry."""
    cfg, stack, mesh = request.getfixturevalue(case)
    t = mesh.material_tags
    tags = np.asarray(mesh.tags)
    _, trc = material_tables(stack, mesh)
    for tag_set in ([t["p_sample"]], [t["p_ins"], t["o_ins"]]):
        M1 = unit_mass_matrix(mesh.coords, mesh.tris, tags, tag_set)
        c1, c2 = 2.0 ** 21, 2.0 ** 22          # (a power of two apart: the slope's division is exact)
        Ms = []
        for c in (c1, c2):
            rc = ho.cell_coefficients(tags, {k: 1.0 for k in trc}, {k: (c if k in tag_set else v) for k, v in trc.items()})[1]
            Ms.append(ho.assemble_csr(len(mesh.coords), mesh.tris, ho.element_matrices(mesh.coords, mesh.tris, rc, np.ones(len(tags)))[0]))
        slope = (Ms[1] - Ms[0]) / (c2 - c1)
        big = float(abs(M1).max())
        err = float(abs(slope - M1).max())
        print(f"{case} tags {tag_set}: max |slope - M1| = {err / big:.2e} of the largest entry")
        assert big > 0 and err <= 1e-14 * big
        # rows none of whose triangles carry one of the tags are empty
        touched = np.zeros(len(mesh.coords), dtype=bool)
        touched[np.asarray(mesh.tris)[np.isin(tags, tag_set)].ravel()] = True
        assert (~touched).sum() > 100 and not abs(M1)[~touched].sum()


# 2. the recursion against central differences of oracle runs ------------------------------------------------------------------------
def _primal(cfg, stack, mesh, scheme, nodes, tag_to_k=None, tag_to_rc=None, aniso=None):
    prob = make_problem(cfg, stack, mesh, backend=CapacityTangentOracleBackend(), scheme=scheme, **({"k_aniso": aniso} if aniso else {}))
    tk, trc = material_tables(stack, mesh)
    prob.set_materials({**tk, **(tag_to_k or {})}, {**trc, **(tag_to_rc or {})})
    return prob.run(NSTEPS, nodes, time_varying=[prob.bcs[3]])[1]


@pytest.mark.parametrize("scheme", ["backward_euler", "bdf2"])
@pytest.mark.parametrize("name", ["p_sample.rho_c", "p_ins.cv"])
def test_recursion_matches_central_differences_in_the_capacity(case_with_diamond_small, name, scheme):
    """p_sample.rho_c: the column itself.  p_ins.cv: rho times the column, against differences of runs at cv (1 +- step)."""
    cfg, stack, mesh = case_with_diamond_small
    nodes = _nodes(mesh)
    mat, suffix = name.split(".")
    tag = mesh.material_tags[mat]
    rho, cv = float(cfg["mats"][mat]["rho"]), float(cfg["mats"][mat]["cv"])
    assert material_tables(stack, mesh)[1][tag] == rho * cv
    prob = make_problem(cfg, stack, mesh, backend=CapacityTangentOracleBackend(), scheme=scheme)
    _, _, ts, _, _ = prob.run_tangent(NSTEPS, nodes, capacity=[[tag]], time_varying=[prob.bcs[3]])
    theta0, factor = (rho * cv, 1.0) if suffix == "rho_c" else (cv, rho)
    s = factor * ts[:, 0]
    scale = float(np.max(np.abs(s)))
    assert scale > 0

    def fd_error(rel):
        runs = [_primal(cfg, stack, mesh, scheme, nodes, tag_to_rc={tag: rho * cv * (1 + sg * rel)}) for sg in (1, -1)]
        return float(np.max(np.abs(s - (runs[0] - runs[1]) / (2 * rel * theta0))) / scale)

    rel, err = find_step(fd_error)
    print(f"{name} {scheme}: max|s| theta = {scale * theta0:.3g} K; central difference at relative step {rel:.3g} off by {err:.2e} of max|s|")
    assert rel == FD_REL_STEP[name], "the step the GPU test uses (capacity_tangent_oracle.FD_REL_STEP) is the one found here"
    assert err <= 1e-4


@pytest.mark.parametrize("scheme", ["backward_euler", "bdf2"])
def test_a_column_that_is_conductivity_and_capacity_is_the_sum_of_both(case_with_diamond_small, scheme):
    """Column 0 carries k and rho_c of p_sample, columns 1 and 2 each alone, on the anisotropic configuration: the loads add, so the
    column is the sum of the two to rounding.  The central difference runs along (dk, drho_c) = (1, 1) step; per unit, the capacity
    part is some 1e-6 of the conductivity part (rho_c is 6e6 J/m^3/K, k 3.8 W/m/K), so the sum is what holds it to account and the
    difference checks the direction as a whole."""
    cfg, stack, mesh = case_with_diamond_small
    aniso = mixed_multipliers(mesh)
    nodes = _nodes(mesh)
    tag = mesh.material_tags["p_sample"]
    tk, trc = material_tables(stack, mesh)
    prob = make_problem(cfg, stack, mesh, backend=CapacityTangentOracleBackend(), scheme=scheme, k_aniso=aniso)
    _, _, ts, _, _ = prob.run_tangent(NSTEPS, nodes, conductivity=[[(tag, "k")]], capacity=[[tag]], time_varying=[prob.bcs[3]])
    both = ts[:, 0]
    prob.set_state(float(cfg["heating"]["ic_temp"]))
    _, _, t2, _, _ = prob.run_tangent(NSTEPS, nodes, conductivity=[[(tag, "k")], []], capacity=[[], [tag]], time_varying=[prob.bcs[3]])
    k_alone, c_alone = t2[:, 0], t2[:, 1]
    assert np.max(np.abs(c_alone)) > 0
    gap = float(np.max(np.abs(both - (k_alone + c_alone))))
    print(f"k + rho_c {scheme}: |both - (k alone + rho_c alone)| = {gap / np.max(np.abs(k_alone)):.2e} of max|s_k| = "
          f"{gap / np.max(np.abs(c_alone)):.2e} of max|s_c|")
    assert gap <= 1e-12 * (np.max(np.abs(k_alone)) + np.max(np.abs(c_alone)))
    scale = float(np.max(np.abs(both)))

    def fd_error(rel):
        h = rel * tk[tag]
        runs = [_primal(cfg, stack, mesh, scheme, nodes, tag_to_k={tag: tk[tag] + sg * h}, tag_to_rc={tag: trc[tag] + sg * h}, aniso=aniso)
                for sg in (1, -1)]
        return float(np.max(np.abs(both - (runs[0] - runs[1]) / (2 * h))) / scale)

    rel, err = find_step(fd_error)
    print(f"k + rho_c {scheme}: central difference at relative step {rel:.3g} off by {err:.2e} of max|s|")
    assert rel == FD_REL_STEP["p_sample.k+rho_c"] and err <= 1e-4


# 3. the scaling identity ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scheme", ["backward_euler", "bdf2"])
@pytest.mark.parametrize("case", ["case_with_diamond_small", "case_no_diamond_small"])
def test_scaling_every_k_and_every_rho_c_together_changes_nothing(request, case, scheme):
    cfg, stack, mesh = request.getfixturevalue(case)
    prob = make_problem(cfg, stack, mesh, backend=CapacityTangentOracleBackend(), scheme=scheme)
    ks, cs = identity_terms(prob, *material_tables(stack, mesh), _nodes(mesh), NSTEPS, float(cfg["heating"]["ic_temp"]))
    scale = max(float(np.max(np.abs(v))) for v in ks)
    resid = float(np.max(np.abs(sum(ks) + sum(cs))))
    print(f"{case} {scheme}: |sum_t k_t s_k + c_t s_c| = {resid / scale:.2e} of max_t |k_t s_k_t| = {scale:.3g} K")
    assert scale > 0 and max(float(np.max(np.abs(v))) for v in cs) > 1e-3 * scale
    assert resid <= 1e-9 * scale


# 4. the Python layers ------------------------------------------------------------------------------------------------------------------
class RecordingBackend(CapacityTangentOracleBackend):
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
        self.calls.append(("tangent_set_shape", j))
        super().tangent_set_shape(j, vz)

    def tangent_set_capacity(self, tag_col):
        self.calls.append(("tangent_set_capacity", dict(tag_col)))
        super().tangent_set_capacity(tag_col)

    def run_tangent(self, *a, **kw):
        self.calls.append(("run_tangent",))
        return super().run_tangent(*a, **kw)


def test_heat_problem_call_order_with_and_without_capacity(case_with_diamond_small):
    cfg, stack, mesh = case_with_diamond_small
    t = mesh.material_tags
    be = RecordingBackend()
    prob = make_problem(cfg, stack, mesh, backend=be)
    nodes = [0, 5]
    v = np.linspace(0.0, 1.0, prob.n)
    # without capacity: exactly the calls of before, in their order
    prob.run_tangent(2, nodes, conductivity=[[t["p_coupler"], t["o_coupler"]], [t["gasket"]]])
    assert be.calls == [("tangent_setup", 2, {t["p_coupler"]: 0, t["o_coupler"]: 0, t["gasket"]: 1}), ("run_tangent",)]
    del be.calls[:]
    prob.run_tangent(2, nodes, conductivity=[[t["gasket"]]], shape={0: v}, capacity=[])
    assert [c[0] for c in be.calls] == ["tangent_setup", "tangent_set_shape", "run_tangent"]
    # with capacity: the set-up, the table, the velocities, the run; the same spec continues; another table is another spec
    del be.calls[:]
    prob.run_tangent(2, nodes, conductivity=[[t["gasket"]]], capacity=[[], [t["p_ins"], t["o_ins"]], [t["p_sample"]]], shape={1: v})
    assert be.calls == [("tangent_setup", 3, {t["gasket"]: 0}), ("tangent_set_capacity", {t["p_ins"]: 1, t["o_ins"]: 1, t["p_sample"]: 2}),
                        ("tangent_set_shape", 1), ("run_tangent",)]
    prob.run_tangent(2, nodes, conductivity=[[t["gasket"]]], capacity=[[], [t["p_ins"], t["o_ins"]], [t["p_sample"]]], shape={1: v})
    assert be.calls[4:] == [("run_tangent",)]
    del be.calls[:]
    prob.run_tangent(2, nodes, conductivity=[[t["gasket"]]], capacity=[[], [t["p_ins"]], [t["p_sample"]]], shape={1: v})
    assert [c[0] for c in be.calls] == ["tangent_setup", "tangent_set_capacity", "tangent_set_shape", "run_tangent"]
    # a capacity-only run makes the set-up of only -1 entries; pairs go to the directional set-up, capacity columns as before
    del be.calls[:]
    prob.run_tangent(2, nodes, capacity=[[t["p_sample"]]])
    assert be.calls[:2] == [("tangent_setup", 1, {}), ("tangent_set_capacity", {t["p_sample"]: 0})]
    prob.run_tangent(2, nodes, conductivity=[[(t["p_ins"], "z")]], capacity=[[t["p_ins"]]])
    assert be.calls[3][:2] == ("tangent_setup_dir", 1) and be.calls[4] == ("tangent_set_capacity", {t["p_ins"]: 0})
    # dropping the capacity is a new set-up (which removes the table), not a call that clears it
    del be.calls[:]
    prob.run_tangent(2, nodes, conductivity=[[(t["p_ins"], "z")]])
    assert [c[0] for c in be.calls] == ["tangent_setup_dir", "run_tangent"]
    with pytest.raises(ValueError, match=rf"cell tag {t['p_ins']} is listed in two capacity columns"):
        prob.run_tangent(2, nodes, capacity=[[t["p_ins"]], [t["p_sample"], t["p_ins"]]])
    with pytest.raises(ValueError, match="no parameter"):
        prob.run_tangent(2, nodes, capacity=[])


def _session(mesh, backend=None):
    from heatflow_amd.driver import SimulationSession

    return SimulationSession(mesh.coords, mesh.tris, mesh.tags, mesh.material_tags, backend=backend or CapacityTangentOracleBackend(),
                             precond=0)


@pytest.fixture(scope="module")
def small_cfg(case_with_diamond_small):
    cfg = copy.deepcopy(case_with_diamond_small[0])
    cfg["timing"]["num_steps"] = 30
    return cfg


def test_get_param_and_set_params_for_the_three_suffixes(small_cfg):
    from heatflow_amd.aniso import split_param
    from heatflow_amd.fit import get_param, set_params

    cfg = small_cfg
    rho, cv = float(cfg["mats"]["p_sample"]["rho"]), float(cfg["mats"]["p_sample"]["cv"])
    assert split_param("p_sample.rho_c") == ("p_sample", "c") and split_param("a.cv") == ("a", "cv") and split_param("a.rho") == ("a", "rho")
    assert get_param(cfg, "p_sample.rho_c") == rho * cv and get_param(cfg, "p_sample.cv") == cv and get_param(cfg, "p_sample.rho") == rho
    c = set_params(cfg, ("p_sample.rho_c", "p_ins.cv", "o_ins.rho", "p_sample"), (1.1 * rho * cv, 700.0, 3000.0, 5.0))
    assert float(c["mats"]["p_sample"]["rho"]) == rho and float(c["mats"]["p_sample"]["cv"]) == 1.1 * rho * cv / rho
    assert get_param(c, "p_sample.rho_c") == pytest.approx(1.1 * rho * cv, rel=1e-15)
    assert c["mats"]["p_ins"]["cv"] == 700.0 and c["mats"]["p_ins"]["rho"] == cfg["mats"]["p_ins"]["rho"]
    assert c["mats"]["o_ins"]["rho"] == 3000.0 and c["mats"]["o_ins"]["cv"] == cfg["mats"]["o_ins"]["cv"] and c["mats"]["p_sample"]["k"] == 5.0
    assert float(cfg["mats"]["p_sample"]["cv"]) == cv                      # the input is left alone
    for a, b in (("p_sample.rho_c", "p_sample.cv"), ("p_sample.cv", "p_sample.rho"), ("p_sample.rho", "p_sample.rho_c")):
        with pytest.raises(ValueError, match=rf"{re.escape(a)}.*{re.escape(b)}"):
            set_params(cfg, (a, "fwhm", b), (1.0, 1.0, 1.0))
    set_params(cfg, ("p_sample.cv", "p_ins.cv"), (1.0, 1.0))              # two materials are independent
    with pytest.raises(ValueError, match=r"nothing\.cv"):
        get_param(cfg, "nothing.cv")
    with pytest.raises(ValueError, match=r"p_ins\.k_q"):                   # any other suffix stays refused
        get_param(cfg, "p_ins.k_q")


def test_session_names_tangents_and_refusals(case_with_diamond_small, small_cfg):
    from heatflow_amd.fit import set_params
    from heatflow_amd.geometry import build_stack
    from heatflow_amd.parameter_sweep import get_watcher_points

    _, _, mesh = case_with_diamond_small
    cfg = small_cfg
    stack, wp = build_stack(cfg), get_watcher_points(cfg)
    rho, cv = float(cfg["mats"]["p_ins"]["rho"]), float(cfg["mats"]["p_ins"]["cv"])
    s = _session(mesh)
    try:
        names = ["p_sample.rho_c", "p_sample", "p_ins.cv", "fwhm", "o_ins.rho", "p_sample.thickness"]
        res = s.run(cfg, stack, wp, tangents=names)
        assert list(res["tangents"]) == names and res["tangent_iters"].shape == (30, len(names))
        for nm in names:
            assert np.max(np.abs(res["tangents"][nm]["oside"])) > 0
        # cv and rho of one material are the same column times rho and times cv
        a = s.run(cfg, stack, wp, tangents=["p_ins.cv"])["tangents"]["p_ins.cv"]["oside"]
        b = s.run(cfg, stack, wp, tangents=["p_ins.rho"])["tangents"]["p_ins.rho"]["oside"]
        c = s.run(cfg, stack, wp, tangents=["p_ins.rho_c"])["tangents"]["p_ins.rho_c"]["oside"]
        np.testing.assert_allclose(a, rho * c, rtol=1e-13, atol=0)
        np.testing.assert_allclose(b, cv * c, rtol=1e-13, atol=0)
        # the whole chain for one name: set_params -> stack -> run
        rel = FD_REL_STEP["p_ins.cv"]
        curves = []
        for sg in (1, -1):
            cc = set_params(cfg, ("p_ins.cv",), (cv * (1 + sg * rel),))
            curves.append(s.run(cc, build_stack(cc), wp)["watchers"]["oside"])
        fd = (curves[0] - curves[1]) / (2 * rel * cv)
        assert np.max(np.abs(a - fd)) <= 1e-4 * np.max(np.abs(a))
        with pytest.raises(ValueError, match=r"tangents:.*'p_ins\.cv'.*'p_ins\.rho'"):
            s.run(cfg, stack, wp, tangents=["p_ins.cv", "p_sample", "p_ins.rho"])
        with pytest.raises(ValueError, match=r"unknown parameter 'nothing\.rho_c'"):
            s.run(cfg, stack, wp, tangents=["nothing.rho_c"])
        with pytest.raises(ValueError, match=r"p_ins\.k_q"):
            s.run(cfg, stack, wp, tangents=["p_ins.k_q"])
    finally:
        s.close()
    # the refusal of capacity tables stays the existing one
    from heatflow_amd.fit import fit_parameters

    ct = copy.deepcopy(cfg)
    ct["mats"]["p_sample"]["cv_einstein"] = {"theta": 500.0, "T_ref": 300.0, "T_min": 250.0, "T_max": 3000.0}
    with pytest.raises(ValueError, match=r"mats\.p_sample\.cv_einstein"):
        fit_parameters(ct, None, ("p_sample.cv",), {"time": np.zeros(2), "temp": np.zeros(2), "oside": np.zeros(2)})


def test_header_declares_and_backend_lists_the_entry_point():
    from heatflow_amd import hip_backend
    from test_cabi import _declared_symbols

    declared = _declared_symbols()
    assert "hf_tangent_set_capacity" in declared and "hf_tangent_set_capacity" in hip_backend.EXPORTS
    assert sorted(declared) == sorted(hip_backend.EXPORTS)
    with open(os.path.join(ROOT, "include", "heatflow_hip.h")) as f:
        text = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    assert re.search(r"int\s+hf_tangent_set_capacity\(hf_ctx\*\s*ctx,\s*int32_t\s+tab_len,\s*const int32_t\*\s*tag_col_c\);", text)
    assert callable(hip_backend.HeatflowHIP.tangent_set_capacity)


# 5. the fit and its budget ---------------------------------------------------------------------------------------------------------------
def _synthetic(cfg, mesh, names=(), values=()):
    """Experiment columns of a run of ``cfg`` with the parameters ``names`` set to ``values``."""
    from heatflow_amd.fit import set_params
    from heatflow_amd.geometry import build_stack
    from heatflow_amd.parameter_sweep import get_watcher_points

    c = set_params(cfg, names, values)
    s = _session(mesh)
    try:
        res = s.run(c, build_stack(c), get_watcher_points(cfg))
    finally:
        s.close()
    return {"time": res["times"], "temp": res["watchers"]["pside"], "oside": res["watchers"]["oside"]}


def _mesh_tuple(mesh):
    return (mesh.coords, mesh.tris, mesh.tags, mesh.material_tags)


def test_fit_recovers_the_sample_cv(case_with_diamond_small, small_cfg):
    from heatflow_amd.fit import fit_parameters, get_param

    _, _, mesh = case_with_diamond_small
    cfg = small_cfg
    cv0 = get_param(cfg, "p_sample.cv")
    exp = _synthetic(cfg, mesh, ("p_sample.cv",), (1.1 * cv0,))
    out = fit_parameters(cfg, None, ("p_sample.cv",), exp, x0=[cv0], max_iter=40, backend=CapacityTangentOracleBackend(),
                         mesh=_mesh_tuple(mesh))
    print(f"fit of p_sample.cv: {out['values'][0] / (1.1 * cv0) - 1:.2e} off, {out['iterations']} iterations, {out['runs']} runs, "
          f"rmse {out['rmse']:.2e}")
    assert abs(out["values"][0] / (1.1 * cv0) - 1) <= 1e-6, out["history"]
    assert out["converged"] and out["rmse"] < 1e-8 and np.isfinite(out["stderr"][0])
    assert out["params"] == ["p_sample.cv"] and "systematic" not in out and "systematic_total" not in out


@pytest.mark.parametrize("q", ["p_sample.rho_c", "fwhm"])
def test_budget_matches_brute_force_refits_to_second_order(case_with_diamond_small, small_cfg, q):
    """Data made at the configuration; p_sample's k fitted with one nuisance (its own rho_c; the beam width).  The brute-force
    answer: set the nuisance to (1 + sigma) times its value, refit, take the difference of the fitted k.  The linear prediction
    misses it by a term of second order in sigma, so halving sigma divides the disagreement by 4 (between 3 and 5 with the third
    order's share).  sigma = 0.04: both refits converge in 5 iterations on the CPU, and the shift (about 0.34 sigma k for rho_c,
    -0.47 sigma k for fwhm) is far above the fits' own resolution."""
    from heatflow_amd.fit import fit_parameters, get_param, set_params

    _, _, mesh = case_with_diamond_small
    cfg = small_cfg
    exp = _synthetic(cfg, mesh)
    sigma = 0.04
    q0, k0 = get_param(cfg, q), get_param(cfg, "p_sample")
    kw = dict(max_iter=40, backend=CapacityTangentOracleBackend(), mesh=_mesh_tuple(mesh), xtol=1e-13, ftol=1e-16)
    miss = []
    for sg in (sigma, sigma / 2):
        out = fit_parameters(cfg, None, ("p_sample",), exp, x0=[1.05 * k0], nuisance={q: sg}, **kw)
        assert out["converged"] and abs(out["values"][0] / k0 - 1) <= 1e-8
        assert set(out["systematic"]) == {q} and set(out["systematic"][q]) == {"p_sample"} and set(out["systematic_total"]) == {"p_sample"}
        assert out["systematic_total"]["p_sample"] == abs(out["systematic"][q]["p_sample"])
        predicted = out["systematic"][q]["p_sample"]
        brute = fit_parameters(set_params(cfg, (q,), (q0 * (1 + sg),)), None, ("p_sample",), exp, x0=[k0], **kw)
        assert brute["converged"]
        actual = brute["values"][0] - out["values"][0]
        print(f"{q} sigma {sg:g}: predicted shift {predicted / k0:+.4e} k, brute force {actual / k0:+.4e} k, disagreement "
              f"{abs(actual - predicted) / k0:.3e} k")
        assert abs(predicted) > 1e-3 * k0
        miss.append(abs(actual - predicted))
    ratio = miss[0] / miss[1]
    print(f"{q}: disagreement falls by {ratio:.3f} when sigma is halved")
    assert 3.0 <= ratio <= 5.0


def test_budget_keys_refusals_and_total(case_with_diamond_small, small_cfg):
    from heatflow_amd.fit import fit_parameters

    _, _, mesh = case_with_diamond_small
    cfg = small_cfg
    exp = _synthetic(cfg, mesh)
    kw = dict(max_iter=3, backend=CapacityTangentOracleBackend(), mesh=_mesh_tuple(mesh))
    plain = fit_parameters(cfg, None, ("p_sample",), exp, **kw)
    nz = {"p_ins.rho_c": 0.15, "p_sample.cv": 0.1, "p_sample.thickness": 0.05, "fwhm": 0.1, "p_ins": 0.2}
    out = fit_parameters(cfg, None, ("p_sample", "p_coupler"), exp, nuisance=nz, **kw)
    assert set(out) == set(plain) | {"systematic", "systematic_total"}
    assert list(out["systematic"]) == list(nz)
    for q in nz:
        assert set(out["systematic"][q]) == {"p_sample", "p_coupler"}
        assert all(np.isfinite(v) and v != 0.0 for v in out["systematic"][q].values())
    for p in ("p_sample", "p_coupler"):
        assert out["systematic_total"][p] == pytest.approx(np.sqrt(sum(out["systematic"][q][p] ** 2 for q in nz)), rel=1e-14)
    assert out["tangent_runs"] >= 2 and len(out["stderr"]) == 2
    for bad, pat in (({"p_sample": 0.1}, r"'p_sample'.*fitted"), ({"nothing.cv": 0.1}, r"nothing\.cv"), ({"p_ins.k_q": 0.1}, r"p_ins\.k_q"),
                     ({"p_ins.cv": 0.0}, r"'p_ins\.cv'.*sigma"), ({"p_ins.cv": -0.1}, r"'p_ins\.cv'.*sigma"),
                     ({"p_ins.cv": float("nan")}, r"'p_ins\.cv'.*sigma"), ({"gasket.thickness": 0.1}, r"gasket\.thickness")):
        with pytest.raises(ValueError, match=pat):
            fit_parameters(cfg, None, ("p_sample",), exp, nuisance=bad, **kw)
    with pytest.raises(ValueError, match=r"'p_sample\.cv'.*'p_sample\.rho'"):
        fit_parameters(cfg, None, ("p_sample.cv",), exp, nuisance={"p_sample.rho": 0.1}, **kw)


def test_fit_cli_writes_the_budget_and_the_fitted_cv(case_with_diamond_small, small_cfg, tmp_path):
    import yaml

    from heatflow_amd.fit import get_param, main

    cfg = copy.deepcopy(small_cfg)
    path = tmp_path / "cfg.yaml"
    path.write_text(yaml.safe_dump(cfg))
    out_dir = tmp_path / "out"
    assert main(["--config", str(path), "--params", "p_sample.rho_c", "--nuisance", "p_ins.cv=0.15", "fwhm=0.1", "--output-dir", str(out_dir),
                 "--max-iter", "2"], backend=CapacityTangentOracleBackend()) == 0
    summary = json.loads((out_dir / "fit_summary.json").read_text())
    assert summary["params"] == ["p_sample.rho_c"] and list(summary["systematic"]) == ["p_ins.cv", "fwhm"]
    assert set(summary["systematic_total"]) == {"p_sample.rho_c"} and summary["systematic_total"]["p_sample.rho_c"] > 0
    used = yaml.safe_load((out_dir / "used_config.yaml").read_text())
    assert get_param(used, "p_sample.rho_c") == pytest.approx(summary["values"][0], rel=1e-12)
    assert float(used["mats"]["p_sample"]["rho"]) == float(cfg["mats"]["p_sample"]["rho"])
    assert float(used["mats"]["p_sample"]["cv"]) == pytest.approx(summary["values"][0] / float(cfg["mats"]["p_sample"]["rho"]), rel=1e-12)
    assert float(used["mats"]["p_ins"]["cv"]) == float(cfg["mats"]["p_ins"]["cv"])
    with pytest.raises(SystemExit):
        main(["--config", str(path), "--params", "p_sample", "--nuisance", "p_ins.cv", "--output-dir", str(out_dir)],
             backend=CapacityTangentOracleBackend())
