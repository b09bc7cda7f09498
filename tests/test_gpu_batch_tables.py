"""Batches under kappa(T) / cv(T) tables on the GPU (hf_set_batch_tables): the re-valued operators of every column
bit for bit against the single run's re-valuation, fields at every step against the float64 restatements and against each
column's own single run, constant tables against the per-column batch without tables, reproducibility, the switch and its
refusals, the read-flux projection, and run_parameter_sweep end to end."""
import copy
import os

import numpy as np
import pytest
import scipy.sparse as sp
import yaml

from conftest import build_case, load_cfg
from helpers import csr_values_on_pattern, make_problem, material_tables
from kappa_T_oracle import BDF2, BE, KappaTOperator, kappa_t_fields, linear_fields, problem_inputs
from rhoc_T_oracle import einstein_tables
from table_tangent_oracle import primal_fields

pytestmark = pytest.mark.gpu

FIELD_TOL_K = 1e-4          # against the restatement
PARITY_TOL_K = 1e-5         # against the column's own single run
STEPS = (4, 8, 8)           # three batch_run calls: the heating starts around step 10 of 100


def _ins_tables(stack, mesh, tag_to_k):
    """1/T tables for the pressure media, 300..800 K at 51 knots: the heated run crosses them."""
    tags = [mesh.material_tags[m.name] for m in stack.materials if m.name.endswith("ins")]
    T = 300.0 + 10.0 * np.arange(51)
    return {t: (300.0, 10.0, tag_to_k[t] * 300.0 / T) for t in tags}


def _cv_tables(stack, mesh, tag_to_rc):
    return einstein_tables(tag_to_rc, [mesh.material_tags[m.name] for m in stack.materials if m.name.endswith("ins")])


def _tables(stack, mesh, tk, trc, kinds):
    kw = {"kappa_tables": _ins_tables(stack, mesh, tk)}
    if kinds == "k+cv":
        kw["rhoc_tables"] = _cv_tables(stack, mesh, trc)
    return kw


def _random_state(n, dofs, g0, seed):
    u = 150.0 + 900.0 * np.random.default_rng(seed).random(n)            # spans and overshoots 300..800 K on both sides
    u[dofs] = g0
    return u


def _open(be, nv, states=None, kcols=None, sample=None):
    be.set_batch_tables(True)
    be.batch_begin(nv, 1)
    for j in range(nv):
        if states is not None:
            be.batch_set_state(j, states[j])
        if kcols is not None:
            be.batch_set_column_kappa(j, [sample], [kcols[j]])


def _same_bits(a, b):
    return np.array_equal(np.asarray(a).view(np.uint64), np.asarray(b).view(np.uint64))


# ---- 1. operator bits ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kinds", ["k", "k+cv"])
@pytest.mark.parametrize("nv", [2, 8, 16])
def test_every_columns_operator_is_the_single_runs_bit_for_bit(hip, case_with_diamond_small, nv, kinds):
    """A, D^-1, the lifting values (and M) of every column after one batch_revalue against the single-run context at that column's
    state and constants: A and M through get_csr after set_state + assemble (one re-valuation and eliminate()), D^-1 as 1 / diag of
    that A (k_dinv's division), the lifting values as the entries (free row, Dirichlet column) of the same re-valuation on a context
    without a Dirichlet set.  Again with the grid capped so that a workgroup takes at least 3 row blocks.  The last column is also
    held to the restatement (KappaTOperator.eliminated, 1e-13 of the entry; conductivity tables only: it keeps M constant)."""
    from heatflow_amd.solver import HeatProblem

    cfg, stack, mesh = case_with_diamond_small
    tk, trc, dt, dofs, u0, g = problem_inputs(cfg, stack, mesh, 1)
    tables = _tables(stack, mesh, tk, trc, kinds)
    cap = "rhoc_tables" in tables
    n = len(mesh.coords)
    states = [_random_state(n, dofs, g[0], 100 + j) for j in range(nv)]
    sample = mesh.material_tags["p_sample"]
    kcols = [tk[sample]] * nv
    kcols[0], kcols[nv - 1] = 4.4, 3.1
    prob = make_problem(cfg, stack, mesh, **tables)
    try:
        be = prob.backend
        _open(be, nv, states, kcols, sample)
        be.batch_revalue()
        got = [be.batch_get_operator(j, want_M=cap) for j in range(nv)]
        nblk = (n + 255) // 256
        assert nblk >= 3
        be.batch_revalue(max_workgroups=max(1, nblk // 3))
        capped = [be.batch_get_operator(j, want_M=cap) for j in range(nv)]
        slots = be.lift_slots()
        be.batch_end()
        for a, b in zip(got, capped):
            for key in a:
                assert _same_bits(a[key], b[key]), key
        # the single run, column by column, on the same context and on one without Dirichlet rows
        free = HeatProblem(mesh.coords, mesh.tris, mesh.tags, tk, trc, dt, [], u0, **tables)
        try:
            rowptr, colidx = be.get_csr(values=False)[:2]
            rows = np.repeat(np.arange(n), np.diff(rowptr))
            diag = np.nonzero(rows == colidx)[0]
            assert len(diag) == n and len(slots) > 0
            for j in range(nv):
                tkj = dict(tk)
                tkj[sample] = kcols[j]
                for p in (prob, free):
                    p.set_materials(tkj, trc, assemble=False)
                    p.backend.set_state(states[j])
                    p.backend.assemble(dt, hip.ASM_ROW_GATHER)
                _, _, A, M = be.get_csr()
                A_free = free.backend.get_csr()[2]
                assert _same_bits(got[j]["A"], A), j
                assert _same_bits(got[j]["dinv"], 1.0 / A[diag]), j
                assert _same_bits(got[j]["lift"], A_free[slots]), j
                if cap:
                    assert _same_bits(got[j]["M"], M), j
                    assert not np.array_equal(got[j]["M"], got[(j + 1) % nv]["M"])      # the columns' capacities differ
                assert not np.array_equal(got[j]["A"], got[(j + 1) % nv]["A"])
        finally:
            free.close()
    finally:
        prob.close()
    if not cap:
        j = nv - 1
        tkj = dict(tk)
        tkj[sample] = kcols[j]
        Ahat, _ = KappaTOperator(mesh.coords, mesh.tris, mesh.tags, tkj, trc, dt, tables["kappa_tables"]).eliminated(states[j], dofs)
        ref = csr_values_on_pattern(Ahat, rowptr, colidx)
        rel = np.abs(got[j]["A"] - ref) / np.maximum(np.abs(ref), 1e-300)
        rel[ref == 0.0] = np.abs(got[j]["A"][ref == 0.0])
        assert rel.max() <= 1e-13, rel.max()
        S = sp.csr_matrix((got[j]["A"], colidx, rowptr), shape=(n, n))
        assert (S != S.T).nnz == 0


# ---- 2. fields ----------------------------------------------------------------------------------------------------------------------
_REF = {}


def _columns(case):
    """Four columns: two heating widths times two conductivities of the sample.  Per column (cfg, tag_to_k, g_all)."""
    cfg, stack, mesh = build_case(case, 8.0)
    nsteps = sum(STEPS)
    sample = mesh.material_tags["p_sample"]
    out = []
    for fwhm_scale, k in ((1.0, None), (0.6, None), (1.0, 4.4), (0.6, 4.4)):
        c = copy.deepcopy(cfg)
        c["heating"]["fwhm"] = float(cfg["heating"]["fwhm"]) * fwhm_scale
        tk, trc, dt, dofs, u0, g = problem_inputs(c, stack, mesh, nsteps)
        if k is not None:
            tk = dict(tk)
            tk[sample] = k
        out.append((c, tk, g))
    return (cfg, stack, mesh), out, (trc, dt, dofs, u0)


def _reference(case, scheme, kinds, j):
    key = (case, scheme, kinds, j)
    if key not in _REF:
        (cfg, stack, mesh), cols, (trc, dt, dofs, u0) = _columns(case)
        _, tk, g = cols[j]
        code = BDF2 if scheme == "bdf2" else BE
        tk0 = material_tables(stack, mesh)[0]
        t = _tables(stack, mesh, tk0, trc, kinds)
        if kinds == "k":
            ref = kappa_t_fields(mesh.coords, mesh.tris, mesh.tags, tk, trc, dt, dofs, u0, g, t["kappa_tables"], code, 1)[0]
        else:
            ref = primal_fields(mesh.coords, mesh.tris, mesh.tags, tk, trc, dt, dofs, u0, g, t["kappa_tables"], t["rhoc_tables"], code)
        lin = linear_fields(mesh.coords, mesh.tris, mesh.tags, tk, trc, dt, dofs, u0, g, code) if j == 0 else None
        _REF[key] = (np.asarray(ref), lin)
    return _REF[key]


@pytest.mark.parametrize("kinds", ["k", "k+cv"])
@pytest.mark.parametrize("scheme", ["backward_euler", "bdf2"])
@pytest.mark.parametrize("precond", [0, 1])
@pytest.mark.parametrize("case", ["geballe_with_diamond", "geballe_no_diamond"])
def test_fields_match_the_restatement_and_the_single_run_at_every_step(hip, case, precond, scheme, kinds):
    (cfg, stack, mesh), cols, (trc, dt, dofs, u0) = _columns(case)
    nv, nsteps, n = len(cols), sum(STEPS), len(mesh.coords)
    tk0 = material_tables(stack, mesh)[0]
    tables = _tables(stack, mesh, tk0, trc, kinds)
    sample = mesh.material_tags["p_sample"]
    nodes = np.arange(n, dtype=np.int32)
    prob = make_problem(cfg, stack, mesh, precond=precond, scheme=scheme, amg_reuse=True, **tables)
    try:
        be = prob.backend
        _open(be, nv, [u0] * nv, [c[1][sample] for c in cols], sample)
        g_all = np.stack([c[2] for c in cols], axis=2)
        parts, first = [], 0
        for k in STEPS:
            s, _ = be.batch_run(g_all[first:first + k], prob.rtol, 0.0, prob.max_it, nodes)
            parts.append(s)
            first += k
        batch = np.concatenate(parts)                                     # [step, column, node]
        fallbacks = be.amg_info()["jacobi_fallbacks"] if precond == 1 else 0
        be.batch_end()
    finally:
        prob.close()
    assert fallbacks == 0
    for j, (c, tk, g) in enumerate(cols):
        ref, lin = _reference(case, scheme, kinds, j)
        worst = np.abs(batch[:, j] - ref).max()
        one = make_problem(c, stack, mesh, precond=precond, scheme=scheme, **tables)
        try:
            if tk != tk0:
                one.set_materials(tk, trc)
            _, single, _ = one.run(nsteps, watcher_nodes=nodes, time_varying=[one.bcs[3]])
        finally:
            one.close()
        parity = np.abs(batch[:, j] - np.asarray(single)).max()
        print(f"{case} precond={precond} {scheme} {kinds} column {j}: |batch - restatement| {worst:.3e} K, |batch - single| {parity:.3e} K")
        assert worst <= FIELD_TOL_K, (j, worst)
        assert parity <= PARITY_TOL_K, (j, parity)
        assert np.abs(ref[-1] - ref[0]).max() > 100.0                     # the run heats ...
        if lin is not None:
            assert np.abs(ref - lin).max() > 100 * FIELD_TOL_K            # ... and the tables change the answer
    assert np.abs(batch[:, 0] - batch[:, 1]).max() > 1.0 and np.abs(batch[:, 0] - batch[:, 2]).max() > 100 * FIELD_TOL_K


# ---- 3. constant tables -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precond", [0, 1])
def test_constant_tables_give_the_per_column_batch_without_tables(hip, case_with_diamond_small, precond):
    cfg, stack, mesh = case_with_diamond_small
    nsteps = sum(STEPS)
    tk, trc, dt, dofs, u0, g = problem_inputs(cfg, stack, mesh, nsteps)
    tables = {t: (300.0, 10.0, [tk[t]] * 51) for t in _ins_tables(stack, mesh, tk)}
    sample = mesh.material_tags["p_sample"]
    kcols, nv = [tk[sample], 4.4], 2
    nodes = np.arange(0, len(mesh.coords), 7, dtype=np.int32)
    g_all = np.stack([g, g], axis=2)
    plain = make_problem(cfg, stack, mesh, precond=precond, amg_reuse=True)
    try:
        be = plain.backend
        be.batch_begin(nv, 1)
        for j in range(nv):
            be.update_kappa([sample], [kcols[j]])
            be.batch_load_column(j)
            be.batch_set_state(j, u0)
        A0 = [be.batch_get_operator(j) for j in range(nv)]
        s0, _ = be.batch_run(g_all, plain.rtol, 0.0, plain.max_it, nodes)
        be.batch_end()
    finally:
        plain.close()
    prob = make_problem(cfg, stack, mesh, precond=precond, amg_reuse=True, kappa_tables=tables)
    try:
        be = prob.backend
        _open(be, nv, [u0] * nv, kcols, sample)
        be.batch_revalue()
        A1 = [be.batch_get_operator(j) for j in range(nv)]
        s1, _ = be.batch_run(g_all, prob.rtol, 0.0, prob.max_it, nodes)
        be.batch_end()
    finally:
        prob.close()
    for j in range(nv):
        for key in ("A", "dinv", "lift"):
            assert _same_bits(A0[j][key], A1[j][key]), (j, key)
    assert np.abs(s0 - s1).max() <= PARITY_TOL_K
    assert np.abs(s0[-1] - s0[0]).max() > 100.0


# ---- 4. reproducibility -------------------------------------------------------------------------------------------------------------
def test_two_calls_and_two_contexts_give_the_same_bits(hip, case_with_diamond_small):
    cfg, stack, mesh = case_with_diamond_small
    tk, trc, dt, dofs, u0, g = problem_inputs(cfg, stack, mesh, 1)
    tables = _tables(stack, mesh, tk, trc, "k+cv")
    nv = 4
    states = [_random_state(len(mesh.coords), dofs, g[0], 40 + j) for j in range(nv)]
    runs = []
    for _ in range(2):
        prob = make_problem(cfg, stack, mesh, **tables)
        try:
            _open(prob.backend, nv, states)
            for _ in range(2):
                prob.backend.batch_revalue()
                runs.append([prob.backend.batch_get_operator(j, want_M=True) for j in range(nv)])
            prob.backend.batch_end()
        finally:
            prob.close()
    for other in runs[1:]:
        for a, b in zip(runs[0], other):
            for key in ("A", "dinv", "lift", "M"):
                assert _same_bits(a[key], b[key]), key


# ---- 5. the switch ------------------------------------------------------------------------------------------------------------------
def _refused(hip, call, code, *words):
    if code == hip.HF_ERR_ARG:
        with pytest.raises(ValueError) as e:
            call()
    else:
        with pytest.raises(hip.HipError) as e:
            call()
        assert e.value.code == code
    for w in words:
        assert w in str(e.value), (w, str(e.value))


def test_the_switch_its_refusals_and_the_restored_paths(hip, case_with_diamond_small):
    cfg, stack, mesh = case_with_diamond_small
    tk, trc, dt, dofs, u0, g = problem_inputs(cfg, stack, mesh, 4)
    tables = _tables(stack, mesh, tk, trc, "k+cv")
    t_ins, sample = sorted(tables["kappa_tables"])[0], mesh.material_tags["p_sample"]
    nodes = np.arange(0, len(mesh.coords), 7, dtype=np.int32)
    g_all = np.stack([g, g], axis=2)
    STATE, ARG = hip.HF_ERR_STATE, hip.HF_ERR_ARG
    prob = make_problem(cfg, stack, mesh, monitors={"sample": {"tags": [sample], "above": None}}, **tables)
    try:
        be = prob.backend
        # off (the default): today's message, word for word; the windows need a batch under tables
        _refused(hip, lambda: be.batch_begin(2, 1), STATE)
        with pytest.raises(hip.HipError) as e:
            be.batch_begin(2)
        assert str(e.value).endswith("hf_batch_begin: kappa(T) tables are set (batched sweeps of the nonlinear loop are not supported)")
        _refused(hip, lambda: be.batch_revalue(), STATE, "hf_batch_revalue")
        _refused(hip, lambda: be.batch_set_column_kappa(0, [sample], [4.0]), STATE, "hf_batch_set_column_kappa")
        be.set_batch_tables(True)
        _refused(hip, lambda: be.batch_begin(2, 0), ARG, "hf_batch_begin", "HF_BATCH_SHARED")
        _refused(hip, lambda: be.batch_begin(2, 2), ARG, "hf_batch_begin", "HF_BATCH_AFFINE")
        be.set_picard(2)
        _refused(hip, lambda: be.batch_begin(2, 1), STATE, "hf_batch_begin", "hf_set_picard")
        be.set_picard(1)
        be.table_derivatives(True)
        _refused(hip, lambda: be.batch_begin(2, 1), STATE, "hf_batch_begin", "hf_table_derivatives")
        be.table_derivatives(False)
        be.batch_begin(2, 1)
        _refused(hip, lambda: be.batch_set_source([sample], 1e-5, 0.0), STATE, "hf_batch_set_source", "hf_set_batch_tables")
        _refused(hip, lambda: be.batch_set_monitors(True), STATE, "hf_batch_set_monitors", "hf_set_batch_tables")
        _refused(hip, lambda: be.set_picard(2), STATE, "hf_set_picard")
        _refused(hip, lambda: be.batch_set_column_kappa(0, [t_ins], [4.0]), ARG, "hf_batch_set_column_kappa", f"tag {t_ins}")
        _refused(hip, lambda: be.batch_set_column_kappa(2, [sample], [4.0]), ARG, "hf_batch_set_column_kappa", "column 2")
        be.batch_revalue()
        be.batch_get_operator(1, want_M=True)
        be.batch_set_source(None)                                          # removing a source that is not there stays allowed
        # switching off closes the batch under tables; so do the table calls
        be.set_batch_tables(False)
        _refused(hip, lambda: be.batch_revalue(), STATE, "hf_batch_revalue")
        _refused(hip, lambda: be.batch_begin(2, 1), STATE, "tables are set (batched sweeps of the nonlinear loop are not supported)")
        be.set_batch_tables(True)
        be.batch_begin(2, 1)
        be.set_rhoc_tables({})
        _refused(hip, lambda: be.batch_revalue(), STATE, "hf_batch_revalue")
        be.set_state(u0)
        be.assemble(dt, hip.ASM_ROW_GATHER)
        be.batch_begin(2, 1)                                               # conductivity tables alone: no per-column M
        be.batch_revalue()
        _refused(hip, lambda: be.batch_get_operator(0, want_M=True), STATE, "hf_batch_get_operator", "capacity tables")
        # anisotropy under the switch
        be.batch_end()
        be.set_aniso_tables(True)
        be.set_anisotropy({sample: (2.0, 1.0)})
        be.assemble(dt, hip.ASM_ROW_GATHER)
        _refused(hip, lambda: be.batch_begin(2, 1), STATE, "hf_batch_begin", "hf_set_anisotropy")
        be.set_anisotropy({})
        # after the tables are cleared and the switch is off a plain batch returns what it did
        be.set_kappa_tables({})
        be.set_batch_tables(False)
        be.set_state(u0)
        be.assemble(dt, hip.ASM_ROW_GATHER)
        be.batch_begin(2)
        for j in range(2):
            be.batch_set_state(j, u0)
        s1, _ = be.batch_run(g_all, prob.rtol, 0.0, prob.max_it, nodes)
        be.batch_end()
    finally:
        prob.close()
    plain = make_problem(cfg, stack, mesh)
    try:
        plain.backend.batch_begin(2)
        for j in range(2):
            plain.backend.batch_set_state(j, u0)
        s0, _ = plain.backend.batch_run(g_all, plain.rtol, 0.0, plain.max_it, nodes)
        plain.backend.batch_end()
    finally:
        plain.close()
    assert np.array_equal(s0, s1)


# ---- 6. read-flux -------------------------------------------------------------------------------------------------------------------
def test_read_flux_of_every_column_under_tables(hip, case_no_diamond_small):
    """One batch_run with flux_nodes under tables: per column the projected gradient within 1e-8 of its largest entry of the single
    run's projection of that column's state at the same rtol (the bound of test_gpu_flux's layout test)."""
    cfg, stack, mesh = case_no_diamond_small
    nsteps = 14                                                            # past the start of the heating
    tk, trc, dt, dofs, u0, g = problem_inputs(cfg, stack, mesh, nsteps)
    tables = _tables(stack, mesh, tk, trc, "k")
    sample = mesh.material_tags["p_sample"]
    kcols, nv, rtol = [tk[sample], 4.4], 2, 1e-12
    n = len(mesh.coords)
    nodes = np.arange(n, dtype=np.int32)
    g_all = np.stack([g, g], axis=2)
    prob = make_problem(cfg, stack, mesh, **tables)
    single = make_problem(cfg, stack, mesh)
    try:
        be = prob.backend
        be.flux_setup()
        single.backend.flux_setup()
        _open(be, nv, [u0] * nv, kcols, sample)
        be.batch_run(g_all[:nsteps - 1], prob.rtol, 0.0, prob.max_it, None)
        _, _, flux = be.batch_run(g_all[nsteps - 1:], prob.rtol, 0.0, prob.max_it, None, flux_nodes=nodes, flux_components=3, flux_rtol=rtol)
        states = [be.batch_get_state(j) for j in range(nv)]
        be.batch_end()
        assert flux.shape == (1, 2, nv, n)
        assert np.abs(states[0] - states[1]).max() > 1e-3 and np.abs(states[0] - u0).max() > 10.0
        for j in range(nv):
            single.backend.set_state(states[j])
            own = single.backend.flux_project(rtol, 5000)
            for q in range(2):
                scale = np.abs(own[q]).max()
                assert scale > 0.0
                assert np.abs(flux[0, q, j] - own[q]).max() <= 1e-8 * scale, (j, q)
    finally:
        prob.close()
        single.close()


# ---- end to end ---------------------------------------------------------------------------------------------------------------------
def test_run_parameter_sweep_under_tables_end_to_end(hip, tmp_path):
    import csv

    from heatflow_amd import parameter_sweep as ps
    from heatflow_amd.geometry import scale_mesh_sizes
    from heatflow_amd.run_with_diamond import run_simulation

    cfg = scale_mesh_sizes(load_cfg("geballe_with_diamond_kT"), 8.0)
    cfg["timing"]["num_steps"] = 40
    cfg["timing"]["sweep_tables"] = True
    base = str(tmp_path / "base.yaml")
    with open(base, "w") as f:
        yaml.safe_dump(cfg, f)
    out = str(tmp_path / "sweep")
    width = float(cfg["mats"]["p_sample"]["z"])
    ok, failed = ps.run_parameter_sweep(base, out, (9e-6, 1.6e-5), (3.2, 4.4), (width, width), (2, 2, 1),
                                        base_mesh_folder=str(tmp_path / "meshes"), batch=4)
    assert len(ok) == 4 and not failed, failed
    with open(os.path.join(out, "successful_runs.csv"), newline="") as f:
        rows = list(csv.DictReader(f))
    assert len(rows) == 4 and all(r.get("batch") == "4" and not r.get("batch_error") for r in rows)
    curves = []
    for r in rows:
        with open(os.path.join(r["output_dir"], "used_config.yaml")) as f:
            used = yaml.safe_load(f)
        assert used["timing"]["sweep_tables"] is True and set(used["kappa_tables"]) == {"p_ins", "o_ins", "g_ins", "p_diam", "o_diam"}
        got = np.genfromtxt(os.path.join(r["output_dir"], "watcher_points.csv"), delimiter=",", names=True)
        point = {k: v for k, v in used.items() if k not in ("kappa_tables", "rhoc_tables")}
        res = run_simulation(point, ps.get_mesh_folder_for_width(str(tmp_path / "meshes"), width),
                             output_folder=str(tmp_path / ("one_" + os.path.basename(r["output_dir"]))),
                             watcher_points=ps.get_watcher_points(point), write_xdmf=False, suppress_print=True)
        for name in ("pside", "oside"):
            assert np.abs(got[name] - np.asarray(res["watchers"][name])).max() <= PARITY_TOL_K, (r["output_dir"], name)
        curves.append(got["oside"])
    assert max(c.max() for c in curves) > 301.0 and len({c.tobytes() for c in curves}) == 4
