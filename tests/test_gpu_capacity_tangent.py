"""Capacity columns of tangent runs on the GPU (hf_tangent_set_capacity / k_tangent_load_cap): the load row by row
against the restatement (capacity_tangent_oracle.py), exact zeros and untouched columns, the bitwise promises, the exact recursion,
the scaling identity of Dirichlet-driven runs, central differences of GPU primal runs, every error return, and a fit of
p_sample.cv."""
import json

import numpy as np
import pytest

from aniso_oracle import mixed_multipliers
from capacity_tangent_oracle import FD_REL_STEP, CapacityTangentOracleBackend, identity_terms
from conftest import HEATING_CSV
from helpers import make_problem, material_tables

pytestmark = pytest.mark.gpu

NSTEPS = 20


def _heat(cfg):
    from heatflow_amd.heating import HeatingCurve

    return HeatingCurve(HEATING_CSV, float(cfg["heating"]["ic_temp"]), float(cfg["heating"]["fwhm"]))


def _start_field(mesh):
    """A field that varies everywhere (the heating curve has hardly begun after three steps), so that every row of M^1 w has
    something to multiply."""
    z, r = mesh.coords[:, 0], mesh.coords[:, 1]
    return 300.0 + 40.0 * np.sin(9.0 * (z - z.min()) / (z.max() - z.min()) + 1.0) * np.cos(3.0 * r / r.max())


def _three_steps(prob, mesh, **kw):
    """Three tangent steps from the start field, one call each; returns the four states."""
    prob.set_state(_start_field(mesh))
    states = [prob.state()]
    for k in range(3):
        prob.run_tangent(1, None, time_varying=[prob.bcs[3]], first_step=k, **kw)
        states.append(prob.state())
    return states


def _load_columns(mesh, nv):
    """(conductivity, capacity, {column: tags}) of the load test: nv = 2: p_sample's rho_c and that of both insulation layers; nv =
    16: the same and both couplers' in columns 0, 5 and 15 of sixteen, next to a k_r column (the directional set-up's kernel
    runs first)."""
    t = mesh.material_tags
    if nv == 2:
        cap = {0: [t["p_sample"]], 1: [t["p_ins"], t["o_ins"]]}
        return [], [cap[0], cap[1]], cap
    cap = {0: [t["p_sample"]], 5: [t["p_ins"], t["o_ins"]], 15: [t["p_coupler"], t["o_coupler"]]}
    return [[], [(t["p_ins"], "r")]], [cap.get(j, []) for j in range(16)], cap


# 1. the load ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nv,aniso", [(2, False), (16, True)])
@pytest.mark.parametrize("scheme", ["backward_euler", "bdf2"])
@pytest.mark.parametrize("case", ["case_with_diamond_small", "case_no_diamond_small"])
def test_load_after_three_steps_row_by_row(hip, request, case, scheme, nv, aniso):
    """hf_tangent_load after three steps against -M^1_j w of the restatement at the GPU's own states, every row within 1e-13 of its
    sum of absolute terms, sum_k |M^1_jk w_k| (DESIGN.md 3.15 holds the same arithmetic to it and measured 5.8e-16)."""
    cfg, stack, mesh = request.getfixturevalue(case)
    kw = {"k_aniso": mixed_multipliers(mesh)} if aniso else {}
    cond, cap, cols = _load_columns(mesh, nv)
    prob = make_problem(cfg, stack, mesh, precond=1, scheme=scheme, **kw)
    try:
        states = _three_steps(prob, mesh, conductivity=cond, capacity=cap)
        assert prob.backend.tangent_nv == nv
        got = {j: prob.tangent_load(j) for j in cols}
    finally:
        prob.close()
    ref = make_problem(cfg, stack, mesh, backend=CapacityTangentOracleBackend(), scheme=scheme, **kw)
    ref.backend.tangent_setup(nv, {})
    ref.backend.tangent_set_capacity({t: j for j, ts in cols.items() for t in ts})
    worst = 0.0
    for j in cols:
        Mw, T = ref.backend.capacity_terms(j, (states[3], states[2], states[1]))
        F = -Mw
        assert np.all(T[np.abs(F) > 0] > 0)
        with np.errstate(divide="ignore", invalid="ignore"):
            ratio = np.where(T > 0, np.abs(got[j] - F) / T, np.where(got[j] == 0, 0.0, np.inf))
        worst = max(worst, float(ratio.max()))
        # the load is not small against its terms everywhere: the comparison sees it
        assert np.max(np.abs(F) / np.where(T > 0, T, np.inf)) > 1e-3, j
    print(f"{case} {scheme} aniso={aniso} nv={nv}: max |F - ref| / sum |M1 w| = {worst:.2e}")
    assert worst <= 1e-13


# 2. exact zeros and untouched columns ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scheme", ["backward_euler", "bdf2"])
def test_untouched_rows_are_zero_and_other_columns_keep_their_bits(hip, case_with_diamond_small, scheme):
    """Columns 0 and 1 carry conductivities only, column 2 a conductivity and a capacity, column 3 a capacity only: 0 and 1 have the
    bits of the set-up without hf_tangent_set_capacity, and the rows of column 3 none of whose triangles carry its tag are exact
    zeros.  Before any step (w = 0) no column changes."""
    cfg, stack, mesh = case_with_diamond_small
    t = mesh.material_tags
    cond = [[t["p_sample"]], [t["p_ins"], t["o_ins"]], [t["gasket"]], []]
    cap = [[], [], [t["p_coupler"]], [t["p_sample"]]]
    loads = {}
    for with_cap in (False, True):
        prob = make_problem(cfg, stack, mesh, precond=1, scheme=scheme)
        try:
            kw = dict(conductivity=cond, **({"capacity": cap} if with_cap else {}))
            prob.run_tangent(1, None, time_varying=[prob.bcs[3]], **kw)
            prob.set_state(_start_field(mesh))                  # resets the tangents: no step taken since
            at_rest = [prob.tangent_load(j) for j in range(4)]
            _three_steps(prob, mesh, **kw)
            loads[with_cap] = (at_rest, [prob.tangent_load(j) for j in range(4)])
        finally:
            prob.close()
    for a, b in zip(loads[False][0], loads[True][0]):
        assert np.array_equal(a, b)
    plain, capped = loads[False][1], loads[True][1]
    for j in (0, 1):
        assert plain[j].any() and np.array_equal(plain[j], capped[j])
    assert not plain[3].any() and capped[3].any() and not np.array_equal(plain[2], capped[2])
    tris, tags = np.asarray(mesh.tris, dtype=np.int64), np.asarray(mesh.tags)
    touched = np.zeros(len(mesh.coords), dtype=bool)
    touched[tris[tags == t["p_sample"]].ravel()] = True
    assert touched.any() and (~touched).sum() > 100
    assert not capped[3][~touched].any() and np.count_nonzero(capped[3][touched]) > 0.9 * touched.sum()
    # column 2 differs from the plain one only at the rows of the coupler's triangles
    touched2 = np.zeros(len(mesh.coords), dtype=bool)
    touched2[tris[tags == t["p_coupler"]].ravel()] = True
    assert np.array_equal(plain[2][~touched2], capped[2][~touched2])


# 3. reproducibility ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scheme", ["backward_euler", "bdf2"])
def test_two_calls_and_two_contexts_give_the_same_bits(hip, case_with_diamond_small, scheme):
    cfg, stack, mesh = case_with_diamond_small
    t = mesh.material_tags
    nodes = np.arange(0, len(mesh.coords), 97, dtype=np.int32)
    out = []
    for _ in range(2):
        prob = make_problem(cfg, stack, mesh, precond=1, scheme=scheme, k_aniso=mixed_multipliers(mesh))
        try:
            _, s, ts, it, tit = prob.run_tangent(5, nodes, capacity=[[t["p_sample"]], [t["p_ins"], t["o_ins"]]], time_varying=[prob.bcs[3]])
            first = [prob.tangent_load(j) for j in range(2)]
            second = [prob.tangent_load(j) for j in range(2)]
            for a, b in zip(first, second):
                assert np.array_equal(a, b) and a.any()
            out.append([s, ts, it, tit] + first + [prob.tangent(0), prob.tangent(1)])
        finally:
            prob.close()
    for a, b in zip(*out):
        assert np.array_equal(a, b)


# 4. the exact recursion ------------------------------------------------------------------------------------------------------------------
def _recursion_run(prob, cfg, mesh, nodes):
    """Columns: p_sample's rho_c alone, p_coupler's k, fwhm, p_ins.thickness, p_ins's k and rho_c in one column."""
    from heatflow_amd.geometry import thickness_velocity

    t = mesh.material_tags
    cond = [[], [t["p_coupler"]], [], [], [t["p_ins"]]]
    cap = [[t["p_sample"]], [], [], [], [t["p_ins"]]]
    shape = {3: thickness_velocity(cfg, "p_ins", mesh.coords[:, 0])}
    _, _, ts, _, _ = prob.run_tangent(NSTEPS, nodes, conductivity=cond, capacity=cap, boundary={2: {3: _heat(cfg).gaussian_dfwhm}},
                                      shape=shape, time_varying=[prob.bcs[3]])
    names = ["p_sample.rho_c", "p_coupler", "fwhm", "p_ins.thickness", "p_ins + p_ins.rho_c"]
    return [(nm, ts[:, j], prob.tangent(j)) for j, nm in enumerate(names)]


@pytest.mark.parametrize("scheme", ["backward_euler", "bdf2"])
@pytest.mark.parametrize("case", ["case_with_diamond_small", "case_no_diamond_small"])
def test_tangents_match_the_exact_recursion(hip, request, case, scheme):
    cfg, stack, mesh = request.getfixturevalue(case)
    nodes = np.sort(np.random.default_rng(0).choice(len(mesh.coords), 12, replace=False)).astype(np.int32)
    ref = _recursion_run(make_problem(cfg, stack, mesh, backend=CapacityTangentOracleBackend(), scheme=scheme), cfg, mesh, nodes)
    for precond in (0, 1):
        prob = make_problem(cfg, stack, mesh, precond=precond, scheme=scheme)
        try:
            got = _recursion_run(prob, cfg, mesh, nodes)
        finally:
            prob.close()
        for (nm, ts, field), (_, ts_ref, field_ref) in zip(got, ref):
            scale = np.max(np.abs(field_ref))
            assert scale > 0
            err_s, err_f = np.max(np.abs(ts - ts_ref)) / scale, np.max(np.abs(field - field_ref)) / scale
            print(f"{case} {scheme} precond={precond} {nm}: samples off by {err_s:.2e}, final field by {err_f:.2e} of max|s|")
            assert err_s <= 1e-6 and err_f <= 1e-6, (case, scheme, precond, nm)


# 5. the scaling identity -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scheme", ["backward_euler", "bdf2"])
@pytest.mark.parametrize("case", ["case_with_diamond_small", "case_no_diamond_small"])
def test_scaling_every_k_and_every_rho_c_together_changes_nothing(hip, request, case, scheme):
    """With Dirichlet data only, u does not change when every k and every rho_c is scaled by one factor: sum_t (k_t s_{k_t} + c_t
    s_{c_t}) = 0 at every step, within (number of terms) x 1e-6 of max_t |k_t s_{k_t}| - what the recursion test's bound implies."""
    cfg, stack, mesh = request.getfixturevalue(case)
    nodes = np.arange(0, len(mesh.coords), 53, dtype=np.int32)
    prob = make_problem(cfg, stack, mesh, precond=1, scheme=scheme)
    try:
        ks, cs = identity_terms(prob, *material_tables(stack, mesh), nodes, NSTEPS, float(cfg["heating"]["ic_temp"]))
    finally:
        prob.close()
    scale = max(float(np.max(np.abs(v))) for v in ks)
    resid = float(np.max(np.abs(sum(ks) + sum(cs))))
    terms = len(ks) + len(cs)
    print(f"{case} {scheme}: |sum_t k_t s_k + c_t s_c| = {resid / scale:.2e} of max_t |k_t s_k_t| = {scale:.3g} K ({terms} terms)")
    assert scale > 0 and max(float(np.max(np.abs(v))) for v in cs) > 1e-3 * scale
    assert resid <= terms * 1e-6 * scale


# 6. central differences of GPU primal runs -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["p_sample.rho_c", "p_ins.cv"])
def test_tangents_match_central_differences_of_gpu_runs(hip, case_with_diamond_small, name):
    """Multigrid at rtol = 1e-12; the relative step is the one tests/test_capacity_tangent_cpu.py found in float64."""
    cfg, stack, mesh = case_with_diamond_small
    nodes = np.arange(0, len(mesh.coords), max(1, len(mesh.coords) // 50), dtype=np.int32)
    mat, suffix = name.split(".")
    tag = mesh.material_tags[mat]
    rho, cv = float(cfg["mats"][mat]["rho"]), float(cfg["mats"][mat]["cv"])
    theta0, factor = (rho * cv, 1.0) if suffix == "rho_c" else (cv, rho)
    rel = FD_REL_STEP[name]
    tk, trc = material_tables(stack, mesh)
    prob = make_problem(cfg, stack, mesh, precond=1, rtol=1e-12)
    try:
        _, _, ts, _, _ = prob.run_tangent(NSTEPS, nodes, capacity=[[tag]], time_varying=[prob.bcs[3]])
        s = factor * ts[:, 0]
        runs = []
        for sg in (1, -1):
            prob.set_materials(tk, {**trc, tag: rho * cv * (1 + sg * rel)})
            prob.set_state(float(cfg["heating"]["ic_temp"]))
            runs.append(prob.run(NSTEPS, nodes, time_varying=[prob.bcs[3]])[1])
    finally:
        prob.close()
    fd = (runs[0] - runs[1]) / (2 * rel * theta0)
    scale = float(np.max(np.abs(s)))
    err = float(np.max(np.abs(s - fd)))
    print(f"{name}: max |s| theta = {scale * theta0:.3e} K; |s - FD| / max|s| = {err / scale:.2e} at relative step {rel:g}")
    assert scale > 0 and err <= 1e-4 * scale


# 7. the primal ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scheme", ["backward_euler", "bdf2"])
def test_primal_with_a_capacity_column_is_bitwise_that_of_hf_run(hip, case_with_diamond_small, scheme):
    cfg, stack, mesh = case_with_diamond_small
    t = mesh.material_tags
    nodes = np.arange(0, len(mesh.coords), 97, dtype=np.int32)
    cond, cap = [[t["p_sample"]], []], [[t["p_sample"]], [t["p_ins"]]]
    for precond in (0, 1):
        out = []
        for tangent in (False, True):
            prob = make_problem(cfg, stack, mesh, precond=precond, scheme=scheme)
            try:
                if tangent:
                    _, s1, _, it1, _ = prob.run_tangent(12, nodes, conductivity=cond, capacity=cap, time_varying=[prob.bcs[3]])
                    _, s2, _, it2, _ = prob.run_tangent(6, nodes, conductivity=cond, capacity=cap, time_varying=[prob.bcs[3]], first_step=12)
                else:
                    _, s1, it1 = prob.run(12, nodes, time_varying=[prob.bcs[3]])
                    _, s2, it2 = prob.run(6, nodes, time_varying=[prob.bcs[3]], first_step=12)
                out.append((s1, it1, s2, it2, prob.state()))
            finally:
                prob.close()
        for a, b in zip(*out):
            assert np.array_equal(a, b), precond


def test_a_removed_capacity_table_leaves_the_run_that_never_had_one(hip, case_with_diamond_small):
    cfg, stack, mesh = case_with_diamond_small
    t = mesh.material_tags
    nodes = np.arange(0, len(mesh.coords), 97, dtype=np.int32)
    tag_col = {t["p_sample"]: 0, t["p_ins"]: 1}
    out = []
    for cleared in (False, True):
        prob = make_problem(cfg, stack, mesh, precond=1)
        try:
            if cleared:
                prob.backend.tangent_setup(2, tag_col)
                prob.backend.tangent_set_capacity({t["p_sample"]: 1, t["gasket"]: 0})
                prob.backend.tangent_set_capacity({})
                prob._tangent_spec = (2, tuple(sorted(tag_col.items())))
            _, s, ts, it, tit = prob.run_tangent(8, nodes, conductivity=[[t["p_sample"]], [t["p_ins"]]], time_varying=[prob.bcs[3]])
            out.append([s, ts, it, tit, prob.tangent(0), prob.tangent(1), prob.tangent_load(0), prob.tangent_load(1)])
        finally:
            prob.close()
    assert out[0][1].any()
    for a, b in zip(*out):
        assert np.array_equal(a, b)


# 8. errors and state rules ---------------------------------------------------------------------------------------------------------------
def test_error_returns_and_state_rules(hip, case_with_diamond_small):
    hb = hip
    cfg, stack, mesh = case_with_diamond_small
    t = mesh.material_tags
    prob = make_problem(cfg, stack, mesh, precond=1)
    be = prob.backend
    try:
        lib, ctx, pi, pd = be._lib, be._ctx, hb._pi, hb._pd
        n_tab = be.tab_len

        def table(entries, length=n_tab):
            tab = np.full(length, -1, dtype=np.int32)
            for tag, j in entries.items():
                tab[tag] = j
            return tab

        def err():
            return lib.hf_last_error(ctx).decode()

        def run(n=2):
            g = np.stack([prob.bc_values((k + 1) * prob.dt) for k in range(n)])
            return lib.hf_run_tangent(ctx, n, pd(g), None, 1e-10, 0.0, 1000, 0, None, None, None, None, None)

        u0 = _start_field(mesh)          # (two steps into the heating curve a uniform state has not moved everywhere)
        be.set_state(u0)
        one = table({t["p_sample"]: 0})
        # before a set-up
        assert lib.hf_tangent_set_capacity(ctx, n_tab, pi(one)) == hb.HF_ERR_STATE
        assert "hf_tangent_set_capacity before hf_tangent_setup" in err()
        # a set-up of only -1 entries: its columns may all become capacity columns (no cap but n_par)
        assert lib.hf_tangent_setup(ctx, 6, pi(table({}))) == hb.HF_OK
        for j in (-2, 6, 7, 16):
            assert lib.hf_tangent_set_capacity(ctx, n_tab, pi(table({t["p_ins"]: j}))) == hb.HF_ERR_ARG
            assert f"tag {t['p_ins']} maps its rho_c to column {j} outside [-1,6)" in err()
        unused = [q for q in range(n_tab) if q not in set(t.values())]
        assert unused, "tag 0 is no cell tag of these meshes"
        assert lib.hf_tangent_set_capacity(ctx, n_tab, pi(table({unused[0]: 1}))) == hb.HF_ERR_ARG
        assert f"tag {unused[0]} is not a cell tag of the mesh" in err()
        assert lib.hf_tangent_set_capacity(ctx, n_tab + 3, pi(table({n_tab + 1: 1}, n_tab + 3))) == hb.HF_ERR_ARG
        assert f"tag {n_tab + 1} is not a cell tag of the mesh" in err()
        assert lib.hf_tangent_set_capacity(ctx, -1, pi(one)) == hb.HF_ERR_ARG
        # a refused call changes nothing: still no capacity column
        assert run() == hb.HF_OK
        assert not any(be.tangent_load(j).any() for j in range(6))
        # NULL and all -1 are fine with nothing to remove; a shorter table covers the tags it has; six columns at once
        assert lib.hf_tangent_set_capacity(ctx, 0, None) == hb.HF_OK
        assert lib.hf_tangent_set_capacity(ctx, n_tab, pi(table({}))) == hb.HF_OK
        assert lib.hf_tangent_set_capacity(ctx, t["p_ins"] + 1, pi(table({t["p_ins"]: 2}, t["p_ins"] + 1))) == hb.HF_OK
        six = dict(zip([t[m] for m in ("p_sample", "p_ins", "o_ins", "p_coupler", "o_coupler", "gasket")], range(6)))
        assert lib.hf_tangent_set_capacity(ctx, n_tab, pi(table(six))) == hb.HF_OK
        assert run() == hb.HF_OK
        assert all(be.tangent_load(j).any() and be.get_tangent(j).any() for j in range(6))
        # it resets every tangent; what only resets the tangents keeps the table
        assert lib.hf_tangent_set_capacity(ctx, n_tab, pi(table(six))) == hb.HF_OK
        assert not any(be.get_tangent(j).any() for j in range(6))
        assert run() == hb.HF_OK and be.get_tangent(0).any()
        be.set_state(u0)
        assert not be.get_tangent(0).any() and not be.tangent_load(0).any()       # w = 0 until a step is taken
        assert run() == hb.HF_OK and be.get_tangent(0).any() and be.tangent_load(0).any()
        be.assemble(prob.dt, prob.assembly_mode)
        assert not be.get_tangent(0).any()
        assert run() == hb.HF_OK and be.get_tangent(0).any()
        # a batch open
        be.batch_begin(2, 0)
        assert lib.hf_tangent_set_capacity(ctx, n_tab, pi(one)) == hb.HF_ERR_STATE and "a batch is open" in err()
        be.batch_end()
        # hf_run_tangent keeps its refusals with capacity columns set
        be.set_load(np.zeros(prob.n))
        assert run() == hb.HF_ERR_STATE and "a load is set" in err()
        be.set_load(None)
        be.set_source([t["p_coupler"]], 1e-5, 0.0)
        assert run() == hb.HF_ERR_STATE and "a source is set" in err()
        be.set_source(None)
        assert run() == hb.HF_OK
        # NULL removes the columns: the loads of the set-up of only -1 entries are zero again
        assert lib.hf_tangent_set_capacity(ctx, 0, None) == hb.HF_OK
        assert run() == hb.HF_OK
        assert not any(be.tangent_load(j).any() for j in range(6))
        # either set-up removes the table
        be.tangent_set_capacity({t["p_sample"]: 0})
        be.tangent_setup(2, {})
        assert run() == hb.HF_OK and not be.tangent_load(0).any() and not be.tangent_load(1).any()
        be.tangent_set_capacity({t["p_sample"]: 0})
        be.tangent_setup_dir(2, k={t["p_sample"]: 1})
        assert run() == hb.HF_OK and not be.tangent_load(0).any() and be.tangent_load(1).any()
        # a shape column and a capacity column share the kept states: removing one keeps the other's load
        be.tangent_set_capacity({t["p_sample"]: 0})
        z = mesh.coords[:, 0]
        be.tangent_set_shape(1, (z - z.min()) / (z.max() - z.min()))
        assert run() == hb.HF_OK
        with_both = be.tangent_load(0)
        be.tangent_set_shape(1, None)
        assert run() == hb.HF_OK and be.tangent_load(0).any() and with_both.any()
        be.tangent_set_shape(1, (z - z.min()) / (z.max() - z.min()))
        be.tangent_set_capacity({})
        assert run() == hb.HF_OK and not be.tangent_load(0).any() and be.tangent_load(1).any()
        # the steady state stays refused
        be.tangent_set_capacity({t["p_sample"]: 0})
        be.steady_setup(prob.bc_dofs)
        be.steady_solve(prob.bc_values(0.0))
        assert run() == hb.HF_ERR_STATE and "hf_steady_solve" in err()
        be.set_state(u0)
        assert run() == hb.HF_OK
        # hf_set_mesh removes the set-up
        be.set_mesh(mesh.coords, mesh.tris, mesh.tags)
        assert lib.hf_tangent_set_capacity(ctx, n_tab, pi(one)) == hb.HF_ERR_STATE
    finally:
        prob.close()


def test_tables_refuse_the_set_up_a_capacity_column_needs(hip, case_with_diamond_small):
    """Capacity tables (cv(T)) and conductivity tables refuse the tangent set-up and the run as before: there is no way to a
    capacity column under them."""
    cfg, stack, mesh = case_with_diamond_small
    t = mesh.material_tags
    prob = make_problem(cfg, stack, mesh, precond=1)
    be = prob.backend
    try:
        be.tangent_setup(1, {})
        be.tangent_set_capacity({t["p_sample"]: 0})
        _, trc = material_tables(stack, mesh)
        be.set_rhoc_tables({t["p_sample"]: (250.0, 500.0, np.full(8, trc[t["p_sample"]]))})
        g = np.stack([prob.bc_values((k + 1) * prob.dt) for k in range(2)])
        rc = be._lib.hf_run_tangent(be._ctx, 2, hip._pd(g), None, 1e-10, 0.0, 1000, 0, None, None, None, None, None)
        assert rc == hip.HF_ERR_STATE and "tables are set" in be._lib.hf_last_error(be._ctx).decode()
    finally:
        prob.close()


# 9. the driver and the fit ---------------------------------------------------------------------------------------------------------------
def test_session_and_fit_of_the_sample_cv(hip, tmp_path):
    import yaml

    from conftest import load_cfg
    from heatflow_amd.driver import SimulationSession, prepare_mesh
    from heatflow_amd.fit import get_param, main, set_params
    from heatflow_amd.geometry import build_stack, scale_mesh_sizes
    from heatflow_amd.parameter_sweep import get_watcher_points

    cfg = scale_mesh_sizes(load_cfg("geballe_with_diamond"), 8.0)
    cfg["timing"]["num_steps"] = 30
    folder = str(tmp_path / "mesh")
    prepare_mesh(cfg, folder, True, build_stack(cfg))
    coords, tris, tags, tag_map = prepare_mesh(cfg, folder, False, build_stack(cfg))      # as the command line will load it
    names = ["p_sample.cv", "p_sample", "p_ins.rho_c", "fwhm"]
    cv0 = get_param(cfg, "p_sample.cv")
    wp = get_watcher_points(cfg)
    s = SimulationSession(coords, tris, tags, tag_map)
    try:
        res = s.run(cfg, build_stack(cfg), wp, tangents=names)
        assert list(res["tangents"]) == names and res["tangent_iters"].shape == (30, 4)
        for nm in names:
            assert np.max(np.abs(res["tangents"][nm]["oside"])) > 0
        c = set_params(cfg, ("p_sample.cv",), (1.1 * cv0,))          # data made 10 % above the configured value
        syn = s.run(c, build_stack(c), wp)
    finally:
        s.close()
    exp_csv = tmp_path / "synthetic.csv"
    np.savetxt(exp_csv, np.column_stack([syn["times"], syn["watchers"]["pside"], syn["watchers"]["oside"]]), delimiter=",",
               header="time,temp,oside", comments="", fmt="%.17g")
    cfg_path, out_dir = tmp_path / "cfg.yaml", tmp_path / "out"
    cfg_path.write_text(yaml.safe_dump(cfg))
    assert main(["--config", str(cfg_path), "--params", "p_sample.cv", "--x0", repr(cv0), "--exp-csv", str(exp_csv),
                 "--nuisance", "p_ins.rho_c=0.15", "fwhm=0.1", "--mesh-folder", folder, "--output-dir", str(out_dir), "--max-iter", "20"]) == 0
    summary = json.loads((out_dir / "fit_summary.json").read_text())
    print(f"fit of p_sample.cv: {summary['values'][0]} (data made at {1.1 * cv0}), off by {summary['values'][0] / (1.1 * cv0) - 1:.2e}, "
          f"stderr {summary['stderr'][0]:.2e}, systematic {summary['systematic_total']['p_sample.cv']:.3e}, "
          f"{summary['iterations']} iterations, {summary['runs']} runs")
    assert summary["params"] == ["p_sample.cv"] and summary["deformed_mesh"] is False
    assert abs(summary["values"][0] / (1.1 * cv0) - 1) <= 1e-5
    assert np.isfinite(summary["stderr"][0])
    assert list(summary["systematic"]) == ["p_ins.rho_c", "fwhm"] and summary["systematic_total"]["p_sample.cv"] > 0
    used = yaml.safe_load((out_dir / "used_config.yaml").read_text())
    assert float(used["mats"]["p_sample"]["cv"]) == pytest.approx(summary["values"][0], rel=1e-12)
    assert float(used["mats"]["p_sample"]["rho"]) == float(cfg["mats"]["p_sample"]["rho"])
