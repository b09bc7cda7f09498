"""The enthalpy form of the capacity on the GPU (hf_set_capacity_form): fields at every step against the
restatement of tests/enthalpy_oracle.py (both small meshes, both preconditioners, hf_step then hf_run, fixed sweeps, the stop
rule, relaxation, the bump alone and with conductivity tables), the re-valued M and A entry by entry, the energy balance of the
GPU's fields, the stored heat, the default path bit for bit, the error returns and 1.04 M DOF."""
import copy
import functools

import numpy as np
import pytest
import scipy.sparse as sp

from conftest import build_case
from enthalpy_oracle import Enthalpy, Tw, bump_tables
from helpers import csr_values_on_pattern, make_problem
from kappa_T_oracle import linear_fields, problem_inputs, table_eval
from rhoc_T_oracle import rhoc_t_fields
from test_gpu_kappa_T import FIELD_TOL_K, STEPS, _ins_tables

pytestmark = pytest.mark.gpu

NSTEPS = sum(STEPS)
SETTINGS = {"fixed1": dict(picard=1), "fixed2": dict(picard=2), "fixed8": dict(picard=8), "tol": dict(picard=64, picard_tol=1e-7), "relax": dict(picard=64, picard_tol=1e-7, picard_relax=0.5)}


def _bump(stack, mesh, trc):
    return bump_tables(trc, [mesh.material_tags[m.name] for m in stack.materials if m.name.endswith("ins")])


@functools.lru_cache(maxsize=None)
def _case(name):
    c = build_case(name, 8.0)
    cfg, stack, mesh = c
    tk, trc, dt, dofs, u0, g = problem_inputs(cfg, stack, mesh, NSTEPS)
    return c, (tk, trc, dt, dofs, u0, g), _bump(stack, mesh, trc), _ins_tables(stack, mesh, tk)


@functools.lru_cache(maxsize=None)
def _oracle(name, kinds):
    (cfg, stack, mesh), (tk, trc, dt, dofs, u0, g), ct, kt = _case(name)
    return Enthalpy(mesh.coords, mesh.tris, mesh.tags, tk, trc, dt, dofs, ct, kt if kinds == "both" else None)


@functools.lru_cache(maxsize=None)
def _reference(name, kinds, setting):
    """(fields, sweeps, changes) of the restatement: computed once, shared, never written to."""
    _, (tk, trc, dt, dofs, u0, g), _, _ = _case(name)
    s = SETTINGS[setting]
    f, sw, ch = _oracle(name, kinds).enthalpy_fields(u0, g, sweeps=s["picard"], tol=s.get("picard_tol", 0.0), relax=s.get("picard_relax", 1.0))
    for a in (f, sw, ch):
        a.setflags(write=False)
    return f, sw, ch


@functools.lru_cache(maxsize=None)
def _linear(name):
    (cfg, stack, mesh), (tk, trc, dt, dofs, u0, g), _, _ = _case(name)
    return linear_fields(mesh.coords, mesh.tris, mesh.tags, tk, trc, dt, dofs, u0, g)


def _tables(name, kinds):
    _, _, ct, kt = _case(name)
    return dict(rhoc_tables=ct, **({"kappa_tables": kt} if kinds == "both" else {}))


def _gpu_fields(name, kinds, precond, setting, record_heat=False):
    (cfg, stack, mesh), *_ = _case(name)
    prob = make_problem(cfg, stack, mesh, precond=precond, capacity_form="enthalpy", **SETTINGS[setting], **_tables(name, kinds))
    try:
        if record_heat:
            prob.record_heat()
        nodes = np.arange(prob.n, dtype=np.int32)
        for bc in prob.bcs:
            bc.update(0.0)
        fields, heat_now = [], []
        for k in range(STEPS[0]):
            prob.step((k + 1) * prob.dt, [prob.bcs[3]])
            fields.append(prob.state())
            if record_heat:
                heat_now.append(prob.stored_heat())
        last_change = [prob.picard_change()]
        first = STEPS[0]
        for n in STEPS[1:]:
            _, s, _ = prob.run(n, watcher_nodes=nodes, time_varying=[prob.bcs[3]], first_step=first)
            fields.extend(s)
            last_change.append(prob.picard_change())
            first += n
        out = dict(fields=np.array(fields), hist=prob.picard_history(), last_change=last_change, iters=list(prob.iters))
        if record_heat:
            out.update(heat_now=heat_now, heat_hist=prob.heat_history(), heat_end=prob.stored_heat(), heat_end2=prob.stored_heat(),
                       raw=prob.backend.stored_heat(prob.monitor_T_ref))
        return out
    finally:
        prob.close()


def _check_fields(name, kinds, precond, setting):
    ref, ref_sw, ref_ch = _reference(name, kinds, setting)
    gpu = _gpu_fields(name, kinds, precond, setting)
    worst = np.abs(gpu["fields"] - ref).max()
    moved = np.abs(ref - _linear(name)).max()
    sw, ch = gpu["hist"]["sweeps"], gpu["hist"]["change"]
    print(f"{name} precond={precond} {kinds} {setting}: worst |dT| {worst:.3e} K, the bump moves the field by {moved:.4g} K, "
          f"sweeps {[int(q) for q in sw]} (restatement {[int(q) for q in ref_sw]}), worst change difference {np.abs(ch - ref_ch).max():.3e} K")
    assert worst <= FIELD_TOL_K
    assert moved > 100 * FIELD_TOL_K
    assert len(sw) == NSTEPS and np.abs(sw - ref_sw).max() <= 1
    cap = SETTINGS[setting]["picard"]
    if "picard_tol" in SETTINGS[setting]:
        assert sw.max() < cap                                                   # the stop rule ends every step
    else:
        assert np.all(sw == cap)
    # change_k is a difference of two states, each within FIELD_TOL_K of the restatement's; where the stop rule ends a step one
    # sweep apart from the restatement (a change within the PCG tolerance of tol), both changes are far below the bound anyway
    assert np.abs(ch - ref_ch).max() <= 4 * FIELD_TOL_K
    assert gpu["last_change"][-1] == ch[-1]                                     # hf_get_picard_change: the last step's
    return ch


@pytest.mark.parametrize("kinds", ["bump", "both"])
@pytest.mark.parametrize("setting", ["fixed8", "tol"])
@pytest.mark.parametrize("precond", [0, 1])
@pytest.mark.parametrize("name", ["geballe_with_diamond", "geballe_no_diamond"])
def test_fields_match_the_restatement_at_every_step(hip, name, precond, setting, kinds):
    _check_fields(name, kinds, precond, setting)


def test_fields_match_the_restatement_with_relaxation(hip):
    _check_fields("geballe_with_diamond", "bump", 0, "relax")


@pytest.mark.parametrize("setting", ["fixed1", "fixed2"])
def test_the_history_reports_changes_that_are_not_converged_away(hip, setting):
    """One and two sweeps: change_k is kelvins here (with 8 sweeps or the stop rule the last solve often starts converged, takes
    no iteration and reports exactly 0), so the comparison with the restatement's changes means something."""
    ch = _check_fields("geballe_no_diamond", "both", 1, setting)
    assert ch.max() > 100 * 4 * FIELD_TOL_K


@pytest.mark.parametrize("kinds", ["bump", "both"])
def test_revalued_M_and_A_are_symmetric_and_match_the_restatement(hip, kinds):
    """M and A after one re-valuation at a random pair (u^n, e) spanning 150..1050 K: bitwise symmetric; M within 1e-13 of each
    entry; A within 1e-13 of |M_ij| + dt |K_ij| (the bounds and the reasoning of test_gpu_rhoc_T.py: a rounding of the summands
    is what a double-precision evaluation can differ by where they cancel).  With e = u^n the capacity is table(Tw_e)."""
    from oracle import heat_oracle as ho

    name = "geballe_with_diamond"
    (cfg, stack, mesh), (tk, trc, dt, dofs, u0, g), ct, kt = _case(name)
    en = _oracle(name, kinds)
    n = len(mesh.coords)
    rng = np.random.default_rng(7)
    un = 150.0 + 900.0 * rng.random(n)
    e = 150.0 + 900.0 * rng.random(n)
    prob = make_problem(cfg, stack, mesh, capacity_form="enthalpy", picard=8, **_tables(name, kinds))
    try:
        prob.backend.enthalpy_revalue(un, e)
        rowptr, colidx, A, M = prob.backend.get_csr()
        prob.backend.enthalpy_revalue(un, un)
        _, _, _, M_same = prob.backend.get_csr()
    finally:
        prob.close()
    Me, Ke = en.element_terms(un, e)
    M_ref = ho.assemble_csr(n, en.tris, Me)
    A_ref = ho.eliminate_dirichlet(ho.assemble_csr(n, en.tris, Me + dt * Ke), dofs)
    for label, vals in (("A", A), ("M", M)):
        S = sp.csr_matrix((vals, colidx, rowptr), shape=(n, n))
        assert (S != S.T).nnz == 0, label                                       # bitwise symmetric
    ref = csr_values_on_pattern(M_ref, rowptr, colidx)
    rel = np.abs(M - ref) / np.maximum(np.abs(ref), 1e-300)
    print("M: worst difference relative to the entry", rel.max())
    assert rel.max() <= 1e-13
    mag = csr_values_on_pattern(ho.assemble_csr(n, en.tris, np.abs(Me) + dt * np.abs(Ke)), rowptr, colidx)
    ref = csr_values_on_pattern(A_ref, rowptr, colidx)
    mag = np.maximum(mag, np.abs(ref))
    print("A: worst difference relative to the summands", (np.abs(A - ref) / mag).max())
    assert (np.abs(A - ref) / mag).max() <= 1e-13
    # e = u^n: the chord capacity is the table at Tw_e
    rc = np.array([float(trc[int(t)]) for t in mesh.tags])
    T = Tw(un, mesh.coords, mesh.tris)
    for tag, (T0, dT, vals) in ct.items():
        sel = np.asarray(mesh.tags) == tag
        rc[sel] = table_eval(T[sel], T0, dT, vals)
    Me0, _ = ho.element_matrices(en.coords, en.tris, rc, np.ones(len(en.tris)))
    ref = csr_values_on_pattern(ho.assemble_csr(n, en.tris, Me0), rowptr, colidx)
    assert (np.abs(M_same - ref) / np.abs(ref)).max() <= 1e-13
    # and the pair matters: the chord capacity is not the table at either end
    assert (np.abs(M - M_same) / np.abs(M_same)).max() > 0.01


def _worst_defect(en, fields, u0, g):
    prev, worst, scale = u0, 0.0, 0.0
    for k, u in enumerate(fields):
        dE, rhs = en.balance(prev, u, g[k])
        worst, scale = max(worst, abs(dE - rhs)), max(scale, abs(dE))
        prev = u
    return worst, scale


@pytest.mark.parametrize("name", ["geballe_with_diamond", "geballe_no_diamond"])
def test_the_gpu_fields_conserve_the_stored_heat(hip, name):
    """The balance of the restatement applied to the GPU's fields at picard_tol = 1e-7: the worst defect is <= 1e-3 of the
    iterated lagged scheme's (8 sweeps, same inputs).  Measured on the MI355X: 2.4e-8 and 7.7e-8 of it (defect /
    largest dE 5.6e-10 and 2.4e-9 against 2.4e-2 and 3.1e-2); the PCG tolerance is the floor."""
    (cfg, stack, mesh), (tk, trc, dt, dofs, u0, g), ct, kt = _case(name)
    en = _oracle(name, "bump")
    gpu = _gpu_fields(name, "bump", 1, "tol")
    lag, _ = rhoc_t_fields(mesh.coords, mesh.tris, mesh.tags, tk, trc, dt, dofs, u0, g, ct, None, picard=8)
    d_gpu, scale = _worst_defect(en, gpu["fields"], u0, g)
    d_lag, _ = _worst_defect(en, lag, u0, g)
    print(f"{name}: balance defect / largest dE: GPU enthalpy form {d_gpu / scale:.3e}, iterated lagged scheme {d_lag / scale:.3e}, "
          f"ratio {d_gpu / d_lag:.3e}")
    assert d_gpu <= 1e-3 * d_lag


def test_stored_heat_against_the_restatement_and_the_records(hip):
    name = "geballe_with_diamond"
    (cfg, stack, mesh), (tk, trc, dt, dofs, u0, g), ct, kt = _case(name)
    en = _oracle(name, "bump")
    gpu = _gpu_fields(name, "bump", 0, "fixed8", record_heat=True)
    u_end = gpu["fields"][-1]
    T_ref = float(u0[0])
    # the restatement's terms are vol_e H(Tw_e): the heat above T_ref is a difference of two such sums, and sum |terms| is theirs
    t_end, t_ref = en.stored_heat_terms(u_end), en.stored_heat_terms(np.full(en.n, T_ref))
    for t in sorted(trc):
        sel = np.asarray(mesh.tags) == t
        ref = 2.0 * np.pi * (t_end[sel] - t_ref[sel]).sum()
        scale = 2.0 * np.pi * (np.abs(t_end[sel]).sum() + np.abs(t_ref[sel]).sum())
        print(f"tag {t}: stored heat {gpu['heat_end'][t]:.6e} J, restatement {ref:.6e} J, difference / sum |terms| "
              f"{abs(gpu['heat_end'][t] - ref) / max(scale, 1e-300):.2e}")
        assert abs(gpu["heat_end"][t] - ref) <= 1e-13 * scale + 1e-300
    assert gpu["heat_end"] == gpu["heat_end2"]                                  # two calls: equal bits
    hist = gpu["heat_hist"]
    assert all(len(v) == NSTEPS for v in hist.values())
    for k, now in enumerate(gpu["heat_now"]):                                   # the records of hf_step = on-demand calls at those states
        assert all(hist[t][k] == now[t] for t in now)
    assert all(hist[t][-1] == gpu["heat_end"][t] for t in hist)                  # and the last record of hf_run
    assert np.all(gpu["raw"][[t for t in range(len(gpu["raw"])) if t not in trc]] == 0.0)


def test_stored_heat_of_an_untabled_region_is_the_monitors_energy(hip):
    name = "geballe_with_diamond"
    (cfg, stack, mesh), (tk, trc, dt, dofs, u0, g), ct, kt = _case(name)
    untabled = sorted(t for t in trc if t not in ct)
    regions = {f"r{t}": {"tags": [t], "above": None} for t in untabled}
    for kw in ({}, dict(rhoc_tables=ct), dict(rhoc_tables=ct, capacity_form="enthalpy", picard=4)):
        prob = make_problem(cfg, stack, mesh, monitors=regions, **kw)
        try:
            prob.run(12, time_varying=[prob.bcs[3]])
            heat, mon = prob.stored_heat(), prob.monitors_now()
            rec = prob.backend.monitor_now().reshape(-1, 7)
        finally:
            prob.close()
        for t in untabled:
            content = 2.0 * np.pi * trc[t] * abs(rec[t, 5])                      # rho_c I1: the heat content
            print(kw.get("capacity_form", "lagged"), "tag", t, heat[t], mon[f"r{t}"]["energy"], abs(heat[t] - mon[f"r{t}"]["energy"]) / content)
            assert abs(heat[t] - mon[f"r{t}"]["energy"]) <= 1e-12 * content


def test_the_default_path_is_bit_for_bit_the_lagged_one(hip):
    name = "geballe_with_diamond"
    (cfg, stack, mesh), (tk, trc, dt, dofs, u0, g), ct, kt = _case(name)
    out = []
    for kw in ({}, {"capacity_form": "lagged"}):
        prob = make_problem(cfg, stack, mesh, precond=1, rhoc_tables=ct, kappa_tables=kt, picard=3, **kw)
        try:
            nodes = np.arange(0, prob.n, 7, dtype=np.int32)
            _, s, it = prob.run(12, watcher_nodes=nodes, time_varying=[prob.bcs[3]])
            _, _, A, M = prob.backend.get_csr()
            out.append((s, np.asarray(it), prob.state(), A, M, prob.picard_change()))
            with pytest.raises(hip.HipError, match="hf_set_picard_control") as e:
                prob.backend.set_picard_control(1e-6, 1.0, 8)
            assert e.value.code == hip.HF_ERR_STATE
            with pytest.raises(hip.HipError, match="hf_get_picard_history"):
                prob.backend.picard_history()
        finally:
            prob.close()
    for a, b in zip(*out):
        assert np.array_equal(a, b)


def test_error_returns_and_refusals(hip):
    name = "geballe_with_diamond"
    (cfg, stack, mesh), (tk, trc, dt, dofs, u0, g), ct, kt = _case(name)
    t_ins = sorted(ct)[0]

    def refused(call, words, code=None):
        with pytest.raises(hip.HipError, match=words) as e:
            call()
        assert e.value.code == (hip.HF_ERR_STATE if code is None else code)

    # what hf_set_capacity_form refuses
    prob = make_problem(cfg, stack, mesh)
    b = prob.backend
    try:
        refused(lambda: b.set_capacity_form("enthalpy"), "no capacity table")
        with pytest.raises(ValueError, match="unknown form"):
            b._check(b._lib.hf_set_capacity_form(b._ctx, 2))
        b.set_rhoc_tables(ct)
        b.set_time_scheme(1)
        refused(lambda: b.set_capacity_form("enthalpy"), "BDF2")
        b.set_time_scheme(0)
        b.set_aniso_tables(True)
        b.set_anisotropy({t_ins: (2.0, 1.0)})
        refused(lambda: b.set_capacity_form("enthalpy"), "anisotropic")
        b.set_anisotropy({})
        b.set_state(u0)
        b.assemble(prob.dt, hip.ASM_ROW_GATHER)
        b.set_capacity_form("enthalpy")
        b.set_capacity_form("lagged")
        b.set_rhoc_tables({})
        b.assemble(prob.dt, hip.ASM_LDS_COLORED)
        with pytest.raises(ValueError, match="row-gather"):
            b.set_rhoc_tables(ct)
    finally:
        prob.close()
    prob = make_problem(cfg, stack, mesh)
    b = prob.backend
    try:
        b.tangent_setup(1, {t_ins: 0})
        b.set_rhoc_tables(ct)
        refused(lambda: b.set_capacity_form("enthalpy"), "tangent")
    finally:
        prob.close()
    prob = make_problem(cfg, stack, mesh)
    b = prob.backend
    try:
        b.batch_begin(2)
        refused(lambda: b.stored_heat(300.0), "hf_stored_heat: a batch is open")
        refused(lambda: b.set_heat_records(True, 300.0), "hf_set_heat_records: a batch is open")
        b.batch_end()
    finally:
        prob.close()
    # a batch under tables (hf_set_batch_tables) is open: the form is refused
    prob = make_problem(cfg, stack, mesh, rhoc_tables=ct)
    b = prob.backend
    try:
        b.set_batch_tables(True)
        b.batch_begin(2, hip.BATCH_PER_COLUMN)
        refused(lambda: b.set_capacity_form("enthalpy"), "hf_set_capacity_form: a batch is open")
        b.batch_end()
        # under the lagged form the form's own calls are refused
        refused(lambda: b.clear_picard_history(), "hf_clear_picard_history: the capacity form is lagged")
        refused(lambda: b.enthalpy_revalue(u0, u0), "hf_enthalpy_revalue: the capacity form is lagged")
        refused(lambda: b.picard_history(), "hf_get_picard_history: the capacity form is lagged")
    finally:
        prob.close()
    # before a mesh
    with hip.HeatflowHIP() as bare:
        bare.tab_len = 4
        refused(lambda: bare.stored_heat(300.0), "hf_stored_heat needs hf_set_mesh")
        refused(lambda: bare.set_heat_records(True, 300.0), "hf_set_heat_records needs hf_set_mesh")
        assert bare.heat_count() == 0
    # what the enthalpy form refuses, and the ranges of its control
    prob = make_problem(cfg, stack, mesh, rhoc_tables=ct, capacity_form="enthalpy", picard=8)
    b = prob.backend
    try:
        refused(lambda: b.set_time_scheme(1), "hf_set_time_scheme.*enthalpy")
        refused(lambda: b.batch_begin(2), "hf_batch_begin.*enthalpy")
        refused(lambda: b.tangent_setup(1, {t_ins: 0}), "hf_tangent_setup.*enthalpy")
        refused(lambda: b.tangent_setup_dir(1, {t_ins: 0}, {}, {}), "hf_tangent_setup_dir.*enthalpy")
        refused(lambda: b.set_anisotropy({t_ins: (2.0, 1.0)}), "hf_set_anisotropy.*enthalpy")
        for bad in ((-1.0, 1.0, 8), (np.nan, 1.0, 8), (0.0, 0.0, 8), (0.0, 1.5, 8), (0.0, 1.0, 0), (0.0, 1.0, 65)):
            with pytest.raises(ValueError, match="hf_set_picard_control"):
                b.set_picard_control(*bad)
        with pytest.raises(ValueError, match="hf_set_picard"):
            b.set_picard(9)
        with pytest.raises(hip.HipError):                                      # no step yet
            prob.picard_change()
        sw, ch = b.picard_history()
        assert len(sw) == 0 and len(ch) == 0
        with pytest.raises(ValueError, match="hf_get_heat"):
            b.get_heat(0, 1)
        b.set_load(np.zeros(prob.n))                                            # a load keeps working
        prob.step(prob.dt, [prob.bcs[3]])
        b.set_load(None)
        assert len(b.picard_history()[0]) == 1
        b.clear_picard_history()
        assert len(b.picard_history()[0]) == 0
        b.set_rhoc_tables({})                                                   # clearing the tables: lagged again
        refused(lambda: b.set_picard_control(0.0, 1.0, 8), "lagged")
    finally:
        prob.close()


def test_run_simulation_end_to_end_on_the_latent_configuration(hip, tmp_path):
    """run_simulation on cfgs/geballe_with_diamond_latent.yaml at scale 8, 40 steps: the watchers against the restatement within
    FIELD_TOL_K, `energy` in monitors.csv for the region with the table - the stored heat of the restatement -, the keys in
    used_config.yaml and result["picard"]."""
    import csv
    import os
    import warnings

    import yaml

    from conftest import load_cfg
    from heatflow_amd.driver import prepare_mesh
    from heatflow_amd.geometry import build_stack, scale_mesh_sizes
    from heatflow_amd.parameter_sweep import get_watcher_points
    from heatflow_amd.run_with_diamond import run_simulation
    from heatflow_amd.solver import nearest_nodes

    cfg = scale_mesh_sizes(load_cfg("geballe_with_diamond_latent"), 8.0)
    cfg["timing"]["num_steps"] = 40
    out = str(tmp_path / "out")
    wp = get_watcher_points(cfg)
    with warnings.catch_warnings():
        warnings.simplefilter("error", RuntimeWarning)                         # no step ends at the cap
        res = run_simulation(cfg, str(tmp_path / "mesh"), rebuild_mesh=True, output_folder=out, watcher_points=wp,
                             write_xdmf=False, suppress_print=True)
    with open(os.path.join(out, "used_config.yaml")) as f:
        used = yaml.safe_load(f)
    assert used["timing"]["capacity_form"] == "enthalpy" and used["timing"]["picard_sweeps"] == 32
    assert used["timing"]["picard_tol"] == 1e-6 and "picard_relax" not in used["timing"]
    assert set(used["rhoc_tables"]) == {"p_ins", "o_ins", "g_ins"}
    assert all("latent" in used["mats"][m] for m in ("p_ins", "o_ins", "g_ins"))
    sw, ch = res["picard"]["sweeps"], res["picard"]["change"]
    assert len(sw) == 40 and sw.max() < 32 and ch.max() <= 1e-6
    # the restatement on the mesh the run wrote
    stack = build_stack(cfg)
    coords, tris, tags, material_tags = prepare_mesh(cfg, str(tmp_path / "mesh"), False, stack)

    class _M:
        pass
    mesh = _M()
    mesh.coords, mesh.tris, mesh.tags, mesh.material_tags = coords, tris, tags, material_tags
    tk, trc, dt, dofs, u0, g = problem_inputs(cfg, stack, mesh, 40)
    kt = {material_tags[m.name]: m.properties["k_table"] for m in stack.materials if "k_table" in m.properties}
    ct = {material_tags[m.name]: m.properties["rho_cv_table"] for m in stack.materials if "rho_cv_table" in m.properties}
    en = Enthalpy(coords, tris, tags, tk, trc, dt, dofs, ct, kt)
    ref, ref_sw, _ = en.enthalpy_fields(u0, g, sweeps=32, tol=1e-6)
    lin = linear_fields(coords, tris, tags, tk, trc, dt, dofs, u0, g)
    names = list(wp) if isinstance(wp, dict) else sorted(res["watchers"])
    nodes = nearest_nodes(coords, [wp[k] for k in names] if isinstance(wp, dict) else wp)
    for j, name in enumerate(names):
        w = np.asarray(res["watchers"][name])
        print(name, "worst |dT|", np.abs(w - ref[:, nodes[j]]).max(), "tables move it by", np.abs(ref[:, nodes[j]] - lin[:, nodes[j]]).max())
        assert np.abs(w - ref[:, nodes[j]]).max() <= FIELD_TOL_K, name
    assert np.abs(ref[:, nodes] - lin[:, nodes]).max() > 100 * FIELD_TOL_K
    assert np.abs(sw - ref_sw).max() <= 1
    # energy of the region with the table: in the result, in monitors.csv, and the restatement's stored heat above ic_temp
    assert "energy" in res["monitors"]["p_ins"] and "energy" in res["monitors"]["sample"]
    with open(os.path.join(out, "monitors.csv")) as f:
        rows = list(csv.reader(f))
    col = [i for i, h in enumerate(rows[0]) if "p_ins" in h and "energy" in h]
    assert len(col) == 1, rows[0]
    csv_energy = np.array([float(r[col[0]]) for r in rows[1:]])
    np.testing.assert_allclose(csv_energy, res["monitors"]["p_ins"]["energy"], rtol=1e-9)
    tag = material_tags["p_ins"]
    sel = np.asarray(tags) == tag
    t_ref = en.stored_heat_terms(np.full(en.n, float(u0[0])))
    for k in (9, 24, 39):
        t_k = en.stored_heat_terms(ref[k])
        want = 2.0 * np.pi * (t_k[sel] - t_ref[sel]).sum()
        # the GPU's field is within FIELD_TOL_K of the restatement's: the heat within rho_c_max * volume * FIELD_TOL_K
        slack = 2.0 * np.pi * en.vol[sel].sum() * np.max(ct[tag][2]) * FIELD_TOL_K
        print("step", k + 1, "energy of p_ins", res["monitors"]["p_ins"]["energy"][k], "restatement", want, "allowed", slack)
        assert abs(res["monitors"]["p_ins"]["energy"][k] - want) <= slack
    assert res["monitors"]["p_ins"]["energy"][-1] > 0.0


def test_one_million_dof_with_multigrid(hip):
    from heatflow_amd.parameter_sweep import get_watcher_points
    from heatflow_amd.solver import nearest_nodes

    cfg, stack, mesh = build_case("geballe_with_diamond", 0.43)
    assert len(mesh.coords) > 1_000_000
    cfg = copy.deepcopy(cfg)
    cfg["timing"]["num_steps"] = 20                                         # 10 steps reach the heating pulse
    tk, trc, *_ = problem_inputs(cfg, stack, mesh, 1)
    wp = get_watcher_points(cfg)
    nodes = nearest_nodes(mesh.coords, [v for v in wp.values()] if isinstance(wp, dict) else wp)
    prob = make_problem(cfg, stack, mesh, precond=1, rhoc_tables=_bump(stack, mesh, trc), kappa_tables=_ins_tables(stack, mesh, tk),
                        capacity_form="enthalpy", picard=32, picard_tol=1e-6)
    try:
        _, samples, iters = prob.run(10, watcher_nodes=nodes, time_varying=[prob.bcs[3]])   # raises unless every step converges
        fallbacks = prob.backend.amg_info()["jacobi_fallbacks"]
        hist = prob.picard_history()
    finally:
        prob.close()
    print("PCG iterations per step:", [int(i) for i in iters], "sweeps per step:", list(hist["sweeps"]), "last changes:", list(hist["change"]))
    assert fallbacks == 0
    assert np.all(np.isfinite(samples))
    assert np.abs(samples[-1] - samples[0]).max() > 1.0
    assert hist["sweeps"].max() < 32
