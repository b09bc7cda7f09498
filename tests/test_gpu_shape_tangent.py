"""Shape columns of tangent runs on the GPU (hf_tangent_set_shape / k_tangent_load_shape): the load row by row
against the restatement (shape_tangent_oracle.py), exact zeros where the velocity is rigid, the bitwise promises, the exact
recursion, central differences of GPU primal runs on moved meshes, every error return, and a fit of p_sample.thickness."""
import json
from types import SimpleNamespace

import numpy as np
import pytest

from aniso_oracle import mixed_multipliers
from conftest import HEATING_CSV
from helpers import make_problem
from shape_tangent_oracle import FD_REL_STEP, ShapeTangentOracleBackend

pytestmark = pytest.mark.gpu

NSTEPS = 20


def _heat(cfg):
    from heatflow_amd.heating import HeatingCurve

    return HeatingCurve(HEATING_CSV, float(cfg["heating"]["ic_temp"]), float(cfg["heating"]["fwhm"]))


def _velocities(cfg, mesh, count):
    """A smooth field that deforms every triangle (the heated ones too, three steps into a run), the thickness velocity of p_ins
    (whose face carries the heated line), the thickness velocity of p_sample."""
    from heatflow_amd.geometry import thickness_velocity

    z, r = mesh.coords[:, 0], mesh.coords[:, 1]
    span = z.max() - z.min()
    smooth = 0.3 * np.sin(7.0 * (z - z.min()) / span + 0.3) * np.cos(2.0 * r / max(r.max(), 1e-30)) + 0.1 * (z / span) ** 2
    return [smooth, thickness_velocity(cfg, "p_ins", z), thickness_velocity(cfg, "p_sample", z)][:count]


def _moved_case(cfg, mesh, name, value, v):
    from heatflow_amd.fit import get_param, set_params
    from heatflow_amd.geometry import build_stack

    c = set_params(cfg, (name,), (value,))
    coords = np.array(mesh.coords, dtype=np.float64)
    coords[:, 0] += v * (value - get_param(cfg, name))
    return c, build_stack(c), SimpleNamespace(coords=coords, tris=mesh.tris, tags=mesh.tags, material_tags=mesh.material_tags)


# 1. the load ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ncol", [1, 2])
@pytest.mark.parametrize("aniso", [False, True])
@pytest.mark.parametrize("scheme", ["backward_euler", "bdf2"])
@pytest.mark.parametrize("case", ["case_with_diamond_small", "case_no_diamond_small"])
def test_load_after_three_steps_row_by_row(hip, request, case, scheme, aniso, ncol):
    """hf_tangent_load after three steps against -Kdot u - Mdot w of the restatement at the GPU's own states, every row within
    1e-13 of its sum of absolute terms, sum_j |Kdot_ij u_j| + sum_j |Mdot_ij w_j|."""
    cfg, stack, mesh = request.getfixturevalue(case)
    kw = {"k_aniso": mixed_multipliers(mesh)} if aniso else {}
    vs = _velocities(cfg, mesh, ncol)
    shape = dict(enumerate(vs))
    # (the heating curve has hardly begun after three steps: the run starts from a field that varies everywhere instead, so that
    # every row of Kdot u and Mdot w has something to multiply)
    z, r = mesh.coords[:, 0], mesh.coords[:, 1]
    u0 = 300.0 + 40.0 * np.sin(9.0 * (z - z.min()) / (z.max() - z.min()) + 1.0) * np.cos(3.0 * r / r.max())
    prob = make_problem(cfg, stack, mesh, precond=1, scheme=scheme, **kw)
    try:
        prob.set_state(u0)
        states = [prob.state()]
        for k in range(3):
            prob.run_tangent(1, None, shape=shape, time_varying=[prob.bcs[3]], first_step=k)
            states.append(prob.state())
        got = [prob.tangent_load(j) for j in range(2)]
    finally:
        prob.close()
    ref = make_problem(cfg, stack, mesh, backend=ShapeTangentOracleBackend(), scheme=scheme, **kw)
    ref.backend.tangent_setup(ncol, {})
    for j, v in shape.items():
        ref.backend.tangent_set_shape(j, v)
    worst = 0.0
    for j in range(ncol):
        F, T = ref.backend.tangent_load_terms(j, state=(states[3], states[2], states[1]))
        assert np.all(T[np.abs(F) > 0] > 0)
        with np.errstate(divide="ignore", invalid="ignore"):
            ratio = np.where(T > 0, np.abs(got[j] - F) / T, np.where(got[j] == 0, 0.0, np.inf))
        worst = max(worst, float(ratio.max()))
        # the load is not small against its terms everywhere: the comparison sees it
        assert np.max(np.abs(F) / np.where(T > 0, T, np.inf)) > 1e-3, j
    if ncol == 1:
        assert not got[1].any()           # the padded column
    print(f"{case} {scheme} aniso={aniso} {ncol} shape column(s): max |F - ref| / (sum |Kdot u| + sum |Mdot w|) = {worst:.2e}")
    assert worst <= 1e-13


# 2. exact zeros --------------------------------------------------------------------------------------------------------------------------
def test_rows_whose_triangles_move_rigidly_are_exactly_zero(hip, case_with_diamond_small):
    """Three shape columns (the four-slot kernel): a rigid motion gives a zero column; the thickness velocities are constant
    outside their layer, and every row whose triangles all have a constant velocity is exactly zero."""
    from heatflow_amd.geometry import thickness_velocity

    cfg, stack, mesh = case_with_diamond_small
    z = mesh.coords[:, 0]
    vs = {0: thickness_velocity(cfg, "p_ins", z), 1: np.full(len(z), 0.75), 2: thickness_velocity(cfg, "p_sample", z)}
    tris = np.asarray(mesh.tris, dtype=np.int64)
    prob = make_problem(cfg, stack, mesh, precond=1)
    try:
        prob.run_tangent(3, None, shape=vs, time_varying=[prob.bcs[3]])
        loads = {j: prob.tangent_load(j) for j in range(4)}
    finally:
        prob.close()
    assert not loads[1].any() and not loads[3].any()
    for j in (0, 2):
        v = vs[j][tris]
        deforms = ~((v[:, 0] == v[:, 1]) & (v[:, 1] == v[:, 2]))
        touched = np.zeros(len(z), dtype=bool)
        touched[tris[deforms].ravel()] = True
        assert touched.any() and (~touched).sum() > 100
        assert not loads[j][~touched].any()
        assert loads[j][touched].any()


# 3. reproducibility ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scheme", ["backward_euler", "bdf2"])
def test_two_calls_and_two_contexts_give_the_same_bits(hip, case_with_diamond_small, scheme):
    cfg, stack, mesh = case_with_diamond_small
    shape = dict(enumerate(_velocities(cfg, mesh, 2)))
    nodes = np.arange(0, len(mesh.coords), 97, dtype=np.int32)
    out = []
    for _ in range(2):
        prob = make_problem(cfg, stack, mesh, precond=1, scheme=scheme, k_aniso=mixed_multipliers(mesh))
        try:
            _, s, ts, it, tit = prob.run_tangent(5, nodes, shape=shape, time_varying=[prob.bcs[3]])
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
    """Columns: p_sample.thickness alone, p_coupler's k, fwhm, p_ins.thickness and p_ins's k in one column."""
    from heatflow_amd.geometry import thickness_velocity

    t = mesh.material_tags
    z = mesh.coords[:, 0]
    cond = [[], [t["p_coupler"]], [], [t["p_ins"]]]
    shape = {0: thickness_velocity(cfg, "p_sample", z), 3: thickness_velocity(cfg, "p_ins", z) * 1e6}
    _, _, ts, _, _ = prob.run_tangent(NSTEPS, nodes, conductivity=cond, boundary={2: {3: _heat(cfg).gaussian_dfwhm}}, shape=shape,
                                      time_varying=[prob.bcs[3]])
    names = ["p_sample.thickness", "p_coupler", "fwhm", "p_ins.thickness x 1e6 + p_ins"]
    return [(nm, ts[:, j], prob.tangent(j)) for j, nm in enumerate(names)]


@pytest.mark.parametrize("scheme", ["backward_euler", "bdf2"])
@pytest.mark.parametrize("case", ["case_with_diamond_small", "case_no_diamond_small"])
def test_tangents_match_the_exact_recursion(hip, request, case, scheme):
    cfg, stack, mesh = request.getfixturevalue(case)
    nodes = np.sort(np.random.default_rng(0).choice(len(mesh.coords), 12, replace=False)).astype(np.int32)
    ref = _recursion_run(make_problem(cfg, stack, mesh, backend=ShapeTangentOracleBackend(), scheme=scheme), cfg, mesh, nodes)
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


# 5. central differences of GPU primal runs on moved meshes ------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["p_sample.thickness", "p_ins.thickness"])
def test_tangents_match_central_differences_of_gpu_runs_on_moved_meshes(hip, case_with_diamond_small, name):
    """Multigrid at rtol = 1e-12; the relative step is the one tests/test_shape_tangent_cpu.py found in float64."""
    from heatflow_amd.fit import get_param
    from heatflow_amd.geometry import thickness_velocity

    cfg, stack, mesh = case_with_diamond_small
    nodes = np.arange(0, len(mesh.coords), max(1, len(mesh.coords) // 50), dtype=np.int32)
    v = thickness_velocity(cfg, name.rsplit(".", 1)[0], mesh.coords[:, 0])
    t0, rel = get_param(cfg, name), FD_REL_STEP[name]
    prob = make_problem(cfg, stack, mesh, precond=1, rtol=1e-12)
    try:
        _, _, ts, _, _ = prob.run_tangent(NSTEPS, nodes, shape={0: v}, time_varying=[prob.bcs[3]])
    finally:
        prob.close()
    runs = []
    for sg in (1, -1):
        c, st, m = _moved_case(cfg, mesh, name, t0 * (1 + sg * rel), v)
        p = make_problem(c, st, m, precond=1, rtol=1e-12)
        try:
            runs.append(p.run(NSTEPS, nodes, time_varying=[p.bcs[3]])[1])
        finally:
            p.close()
    fd = (runs[0] - runs[1]) / (2 * rel * t0)
    scale = float(np.max(np.abs(ts[:, 0])))
    err = float(np.max(np.abs(ts[:, 0] - fd)))
    print(f"{name}: max |s| t = {scale * t0:.3e} K; |s - FD| / max|s| = {err / scale:.2e} at relative step {rel:g}")
    assert scale > 0 and err <= 1e-4 * scale


# 6. the primal ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scheme", ["backward_euler", "bdf2"])
def test_primal_with_a_shape_column_is_bitwise_that_of_hf_run(hip, case_with_diamond_small, scheme):
    cfg, stack, mesh = case_with_diamond_small
    nodes = np.arange(0, len(mesh.coords), 97, dtype=np.int32)
    shape = dict(enumerate(_velocities(cfg, mesh, 2)))
    cond = [[mesh.material_tags["p_sample"]]]
    for precond in (0, 1):
        out = []
        for tangent in (False, True):
            prob = make_problem(cfg, stack, mesh, precond=precond, scheme=scheme)
            try:
                if tangent:
                    _, s1, _, it1, _ = prob.run_tangent(12, nodes, conductivity=cond, shape=shape, time_varying=[prob.bcs[3]])
                    _, s2, _, it2, _ = prob.run_tangent(6, nodes, conductivity=cond, shape=shape, time_varying=[prob.bcs[3]], first_step=12)
                else:
                    _, s1, it1 = prob.run(12, nodes, time_varying=[prob.bcs[3]])
                    _, s2, it2 = prob.run(6, nodes, time_varying=[prob.bcs[3]], first_step=12)
                out.append((s1, it1, s2, it2, prob.state()))
            finally:
                prob.close()
        for a, b in zip(*out):
            assert np.array_equal(a, b), precond


# 7. errors and state rules ---------------------------------------------------------------------------------------------------------------
def test_error_returns_and_state_rules(hip, case_with_diamond_small):
    hb = hip
    cfg, stack, mesh = case_with_diamond_small
    t = mesh.material_tags
    prob = make_problem(cfg, stack, mesh, precond=1)
    be = prob.backend
    nodes = np.arange(0, prob.n, 97, dtype=np.int32)
    try:
        lib, ctx, pi, pd = be._lib, be._ctx, hb._pi, hb._pd
        v = np.ascontiguousarray(_velocities(cfg, mesh, 1)[0])
        none = np.full(be.tab_len, -1, dtype=np.int32)

        def err():
            return lib.hf_last_error(ctx).decode()

        # before a set-up
        assert lib.hf_tangent_set_shape(ctx, 0, pd(v)) == hb.HF_ERR_STATE and "hf_tangent_set_shape before hf_tangent_setup" in err()
        # a set-up of only -1 entries: boundary-only columns, which may get a shape part
        assert lib.hf_tangent_setup(ctx, 6, pi(none)) == hb.HF_OK
        for j in (-1, 6, 7):
            assert lib.hf_tangent_set_shape(ctx, j, pd(v)) == hb.HF_ERR_ARG and f"column {j} outside [0,6)" in err()
            assert lib.hf_tangent_set_shape(ctx, j, None) == hb.HF_ERR_ARG
        for bad in (np.nan, np.inf, -np.inf):
            w = v.copy()
            w[17] = bad
            assert lib.hf_tangent_set_shape(ctx, 0, pd(w)) == hb.HF_ERR_ARG and "node 17 is not finite" in err()
        assert lib.hf_tangent_set_shape(ctx, 3, None) == hb.HF_OK                 # no shape part: nothing to remove
        for j in (0, 1, 2, 3):
            assert lib.hf_tangent_set_shape(ctx, j, pd(v)) == hb.HF_OK
        assert lib.hf_tangent_set_shape(ctx, 4, pd(v)) == hb.HF_ERR_ARG and "fifth shape column" in err()
        assert lib.hf_tangent_set_shape(ctx, 2, pd(2.0 * v)) == hb.HF_OK           # replacing one of the four is fine
        assert lib.hf_tangent_set_shape(ctx, 1, None) == hb.HF_OK
        assert lib.hf_tangent_set_shape(ctx, 4, pd(v)) == hb.HF_OK                 # ... and so is a new one after a removal
        # a batch open
        be.batch_begin(2, 0)
        assert lib.hf_tangent_set_shape(ctx, 0, pd(v)) == hb.HF_ERR_STATE and "a batch is open" in err()
        be.batch_end()
        # hf_run_tangent keeps its refusals with shape columns set
        be.set_load(np.zeros(prob.n))
        g = np.stack([prob.bc_values((k + 1) * prob.dt) for k in range(2)])
        assert lib.hf_run_tangent(ctx, 2, pd(g), None, 1e-10, 0.0, 1000, 0, None, None, None, None, None) == hb.HF_ERR_STATE
        assert "a load is set" in err()
        be.set_load(None)
        # either set-up removes the velocities: the loads of the new set-up have no shape part
        be.tangent_setup(2, {})
        assert lib.hf_run_tangent(ctx, 2, pd(g), None, 1e-10, 0.0, 1000, 0, None, None, None, None, None) == hb.HF_OK
        assert not be.tangent_load(0).any() and not be.tangent_load(1).any()
        be.tangent_set_shape(0, v)
        be.tangent_setup_dir(2, k={t["p_sample"]: 1})
        assert not be.tangent_load(0).any() and be.tangent_load(1).any()
        # the tangent resets keep the velocities and zero the tangents
        be.tangent_set_shape(0, v)
        be.set_state(np.full(prob.n, 300.0))
        assert lib.hf_run_tangent(ctx, 2, pd(g), None, 1e-10, 0.0, 1000, 0, None, None, None, None, None) == hb.HF_OK
        assert be.get_tangent(0).any() and be.tangent_load(0).any()
        be.set_state(np.full(prob.n, 300.0))
        assert not be.get_tangent(0).any()
        assert lib.hf_run_tangent(ctx, 2, pd(g), None, 1e-10, 0.0, 1000, 0, None, None, None, None, None) == hb.HF_OK
        assert be.get_tangent(0).any()
        # hf_set_mesh removes the set-up
        be.set_mesh(mesh.coords, mesh.tris, mesh.tags)
        assert lib.hf_tangent_set_shape(ctx, 0, pd(v)) == hb.HF_ERR_STATE
    finally:
        prob.close()
    # a cleared column's tangents are bitwise those of the run that never had one
    out = []
    for cleared in (False, True):
        prob = make_problem(cfg, stack, mesh, precond=1)
        try:
            if cleared:
                prob.backend.tangent_setup(2, {t["p_sample"]: 0, t["p_ins"]: 1})
                prob.backend.tangent_set_shape(1, v)
                prob.backend.tangent_set_shape(1, None)
                prob._tangent_spec = (2, tuple(sorted({t["p_sample"]: 0, t["p_ins"]: 1}.items())))
            _, s, ts, it, tit = prob.run_tangent(8, nodes, conductivity=[[t["p_sample"]], [t["p_ins"]]], time_varying=[prob.bcs[3]])
            out.append([s, ts, it, tit, prob.tangent(0), prob.tangent(1), prob.tangent_load(1)])
        finally:
            prob.close()
    assert out[0][1].any()
    for a, b in zip(*out):
        assert np.array_equal(a, b)


# 8. the driver and the fit ---------------------------------------------------------------------------------------------------------------
def test_session_and_fit_of_the_sample_thickness(hip, tmp_path):
    import yaml

    from conftest import load_cfg
    from heatflow_amd.driver import SimulationSession, prepare_mesh
    from heatflow_amd.fit import get_param, main
    from heatflow_amd.geometry import build_stack, scale_mesh_sizes, thickness_velocity
    from heatflow_amd.parameter_sweep import get_watcher_points
    from heatflow_amd.solver import nearest_nodes

    cfg = scale_mesh_sizes(load_cfg("geballe_with_diamond"), 8.0)
    cfg["timing"]["num_steps"] = 30
    folder = str(tmp_path / "mesh")
    prepare_mesh(cfg, folder, True, build_stack(cfg))
    coords, tris, tags, tag_map = prepare_mesh(cfg, folder, False, build_stack(cfg))      # as the command line will load it
    names = ["p_sample.thickness", "p_sample", "fwhm"]
    t0 = get_param(cfg, "p_sample.thickness")
    wp = get_watcher_points(cfg)
    s = SimulationSession(coords, tris, tags, tag_map)
    try:
        res = s.run(cfg, build_stack(cfg), wp, tangents=names)
        assert list(res["tangents"]) == names and res["tangent_iters"].shape == (30, 3)
        for nm in names:
            assert np.max(np.abs(res["tangents"][nm]["oside"])) > 0
    finally:
        s.close()
    # data made 10 % above the configuration's thickness, on the mesh deformed to it, at the watcher nodes followed
    mesh = SimpleNamespace(coords=np.asarray(coords), tris=tris, tags=tags, material_tags=tag_map)
    c, st, m = _moved_case(cfg, mesh, "p_sample.thickness", 1.1 * t0, thickness_velocity(cfg, "p_sample", mesh.coords[:, 0]))
    w_nodes = nearest_nodes(mesh.coords, [tuple(p) for p in wp.values()])
    s = SimulationSession(m.coords, tris, tags, tag_map)
    try:
        syn = s.run(c, st, {nm: tuple(m.coords[i]) for nm, i in zip(wp, w_nodes)})
    finally:
        s.close()
    exp_csv = tmp_path / "synthetic.csv"
    np.savetxt(exp_csv, np.column_stack([syn["times"], syn["watchers"]["pside"], syn["watchers"]["oside"]]), delimiter=",",
               header="time,temp,oside", comments="", fmt="%.17g")
    cfg_path, out_dir = tmp_path / "cfg.yaml", tmp_path / "out"
    cfg_path.write_text(yaml.safe_dump(cfg))
    assert main(["--config", str(cfg_path), "--params", "p_sample.thickness", "--x0", repr(t0), "--exp-csv", str(exp_csv),
                 "--mesh-folder", folder, "--output-dir", str(out_dir), "--max-iter", "20"]) == 0
    summary = json.loads((out_dir / "fit_summary.json").read_text())
    print(f"fit of p_sample.thickness: {summary['values'][0]} (data made at {1.1 * t0}), stderr {summary['stderr'][0]:.2e}, "
          f"{summary['iterations']} iterations, {summary['runs']} runs")
    assert summary["params"] == ["p_sample.thickness"] and summary["deformed_mesh"] is True
    assert abs(summary["values"][0] / (1.1 * t0) - 1) <= 1e-5
    assert np.isfinite(summary["stderr"][0])
    used = yaml.safe_load((out_dir / "used_config.yaml").read_text())
    assert float(used["mats"]["p_sample"]["z"]) == pytest.approx(summary["values"][0], rel=1e-12)
