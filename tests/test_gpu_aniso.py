"""Anisotropic conductivities on the GPU (hf_set_anisotropy, k_assemble_rows_an): the operator entry by entry and bit for bit
where it must be, fields at every step against the restatement of tests/aniso_oracle.py, the stretch identity against the existing
isotropic path (small meshes and 1.04 M DOF), the steady state with its hold load, the batched sweeps, a tangent on an isotropic
tag, and the refusals.  Bounds: DESIGN.md 3.10, 3.12 and 5."""
import numpy as np
import pytest
import scipy.sparse as sp

from aniso_oracle import BDF2, BE, aniso_fields, hold_load, matrices, mixed_multipliers, operator, steady_solve, stretched
from conftest import build_case
from helpers import csr_values_on_pattern, make_problem, material_tables, reference_bcs
from kappa_T_oracle import linear_fields, problem_inputs
from test_steady_cpu import steady_bcs

pytestmark = pytest.mark.gpu

ENTRY_TOL = 1e-13          # of |M_ij| + dt |K_ij|
FIELD_TOL_K = 1e-4
STRETCH_TOL_K = 1e-5
SINGLE_RUN_TOL_K = 1e-5
NSTEPS = 20
STEADY_MAX_IT = 400000
STEADY_RTOL = 1e-12


def _case(name, request):
    return request.getfixturevalue({"geballe_with_diamond": "case_with_diamond_small", "geballe_no_diamond": "case_no_diamond_small"}[name])


def _assembled(hip, mesh, tk, trc, dt, aniso, mode=None):
    """(rowptr, colidx, A, M) of a context without Dirichlet rows."""
    tags = sorted(tk)
    with hip.HeatflowHIP(0) as be:
        be.set_mesh(mesh.coords, mesh.tris, mesh.tags)
        be.set_materials(tags, [tk[t] for t in tags], [trc[t] for t in tags])
        if aniso is not None:
            be.set_anisotropy(aniso)
        be.set_dirichlet(np.zeros(0, dtype=np.int32))
        be.assemble(dt, hip.ASM_ROW_GATHER if mode is None else mode)
        return be.get_csr()


# 1. operator ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["geballe_with_diamond", "geballe_no_diamond"])
def test_operator_matches_the_restatement_and_keeps_the_isotropic_bits(hip, request, case):
    cfg, stack, mesh = _case(case, request)
    tk, trc, dt, *_ = problem_inputs(cfg, stack, mesh, 1)
    aniso = mixed_multipliers(mesh)
    assert 0 < len(aniso) < len(tk)
    rowptr, colidx, A, M = _assembled(hip, mesh, tk, trc, dt, aniso)
    _, _, A0, M0 = _assembled(hip, mesh, tk, trc, dt, None)
    n = len(mesh.coords)
    Mr, Ar, Kr = operator(mesh.coords, mesh.tris, mesh.tags, tk, trc, aniso, dt)
    scale = csr_values_on_pattern(abs(Mr) + dt * abs(Kr), rowptr, colidx)
    err = np.abs(A - csr_values_on_pattern(Ar, rowptr, colidx))
    worst = float((err[scale > 0] / scale[scale > 0]).max())
    print(f"{case}: worst |A - A_restated| / (|M| + dt |K|) = {worst:.2e}")
    assert worst <= ENTRY_TOL and np.all(err[scale == 0] == 0.0)
    assert np.array_equal(M, M0)                                              # M bit for bit the isotropic M
    S = sp.csr_matrix((A, colidx, rowptr), shape=(n, n))
    assert (S != S.T).nnz == 0                                                # exactly symmetric
    # rows that touch only isotropic elements: bit for bit those of the isotropic assembly
    touched = np.zeros(n, dtype=bool)
    touched[np.asarray(mesh.tris)[np.isin(mesh.tags, list(aniso))].ravel()] = True
    rows = np.repeat(np.arange(n), np.diff(rowptr))
    assert touched.sum() > 0
    assert np.array_equal(A[~touched[rows]], A0[~touched[rows]])
    assert np.abs(A[touched[rows]] - A0[touched[rows]]).max() > 0.0           # ... and the others moved
    # no-diamond's couplers are one element thick, so there every node may touch an insulator or the sample: the same with the
    # sample alone anisotropic, which leaves whole layers untouched on both meshes
    only = {mesh.material_tags["p_sample"]: aniso[mesh.material_tags["p_sample"]]}
    _, _, As, Ms = _assembled(hip, mesh, tk, trc, dt, only)
    touched_s = np.zeros(n, dtype=bool)
    touched_s[np.asarray(mesh.tris)[np.isin(mesh.tags, list(only))].ravel()] = True
    assert touched_s.sum() > 0 and (~touched_s).sum() > 0
    assert np.array_equal(Ms, M0) and np.array_equal(As[~touched_s[rows]], A0[~touched_s[rows]])
    assert np.abs(As[touched_s[rows]] - A0[touched_s[rows]]).max() > 0.0
    # all multipliers 1, listed or not: M and A bit for bit (the anisotropic kernel is not even launched: both 1 = isotropic)
    _, _, A1, M1 = _assembled(hip, mesh, tk, trc, dt, {t: (1.0, 1.0) for t in tk})
    assert np.array_equal(A1, A0) and np.array_equal(M1, M0)


def test_equal_multipliers_go_through_the_isotropic_element_routine(hip, case_with_diamond_small):
    """One tag anisotropic (so k_assemble_rows_an runs), another with m_r == m_z = 3: the rows that touch no anisotropic element
    are bit for bit those of the isotropic kernel with that tag's kappa tripled."""
    cfg, stack, mesh = case_with_diamond_small
    tk, trc, dt, *_ = problem_inputs(cfg, stack, mesh, 1)
    t_an, t_eq = mesh.material_tags["p_sample"], mesh.material_tags["o_ins"]
    rowptr, colidx, A, M = _assembled(hip, mesh, tk, trc, dt, {t_an: (2.0, 0.25), t_eq: (3.0, 3.0)})
    _, _, A0, M0 = _assembled(hip, mesh, {**tk, t_eq: tk[t_eq] * 3.0}, trc, dt, None)
    n = len(mesh.coords)
    touched = np.zeros(n, dtype=bool)
    touched[np.asarray(mesh.tris)[np.asarray(mesh.tags) == t_an].ravel()] = True
    rows = np.repeat(np.arange(n), np.diff(rowptr))
    in_eq = np.zeros(n, dtype=bool)
    in_eq[np.asarray(mesh.tris)[np.asarray(mesh.tags) == t_eq].ravel()] = True
    assert (in_eq & ~touched).sum() > 0
    assert np.array_equal(M, M0) and np.array_equal(A[~touched[rows]], A0[~touched[rows]])


# 2. fields --------------------------------------------------------------------------------------------------------------------
def _gpu_fields(case, aniso, precond, scheme, kind=None, steps=(4, 8, 8)):
    """hf_step calls, then two hf_run calls; every field."""
    cfg, stack, mesh = case
    prob = make_problem(cfg, stack, mesh, precond=precond, scheme=scheme, k_aniso=aniso)
    try:
        if kind is not None:
            prob.backend.set_start_vector(kind)
        nodes = np.arange(prob.n, dtype=np.int32)
        for bc in prob.bcs:
            bc.update(0.0)
        fields = []
        for k in range(steps[0]):
            prob.step((k + 1) * prob.dt, [prob.bcs[3]])
            fields.append(prob.state())
        first = steps[0]
        for m in steps[1:]:
            _, s, _ = prob.run(m, watcher_nodes=nodes, time_varying=[prob.bcs[3]], first_step=first)
            fields.extend(s)
            first += m
        fb = prob.backend.amg_info()["jacobi_fallbacks"] if precond == 1 else 0
        return np.array(fields), list(prob.iters), fb
    finally:
        prob.close()


def _check_fields(case_name, case, precond, scheme, kind=None):
    cfg, stack, mesh = case
    tk, trc, dt, dofs, u0, g = problem_inputs(cfg, stack, mesh, NSTEPS)
    aniso = mixed_multipliers(mesh)
    code = BDF2 if scheme == "bdf2" else BE
    ref = aniso_fields(mesh.coords, mesh.tris, mesh.tags, tk, trc, dt, dofs, u0, g, aniso, code)
    iso = linear_fields(mesh.coords, mesh.tris, mesh.tags, tk, trc, dt, dofs, u0, g, code)
    gpu, iters, fb = _gpu_fields(case, aniso, precond, scheme, kind)
    worst = float(np.abs(gpu - ref).max())
    moved = float(np.abs(ref - iso).max())
    print(f"{case_name} precond={precond} {scheme} kind={kind}: worst |dT| = {worst:.2e} K, isotropic field differs by {moved:.1f} K, "
          f"iterations/step mean {np.mean(iters):.1f}, multigrid fallbacks {fb}")
    assert worst <= FIELD_TOL_K
    assert moved > 10.0                                                       # the test cannot pass by ignoring the multipliers
    assert np.abs(gpu - iso).max() > 10.0


@pytest.mark.parametrize("scheme", ["backward_euler", "bdf2"])
@pytest.mark.parametrize("precond", [0, 1])
@pytest.mark.parametrize("case", ["geballe_with_diamond", "geballe_no_diamond"])
def test_fields_match_the_restatement_at_every_step(hip, request, case, precond, scheme):
    _check_fields(case, _case(case, request), precond, scheme)


@pytest.mark.parametrize("kind", [0, 1, 2, 3])
def test_fields_match_the_restatement_for_every_start_vector(hip, case_with_diamond_small, kind):
    _check_fields("geballe_with_diamond", case_with_diamond_small, 1, "backward_euler", kind)


# 3. stretch identity against the existing isotropic path ----------------------------------------------------------------------
def _stretch_pair(case, precond, nsteps, nodes=None):
    """(anisotropic run with m_z = 1/4 on every tag, isotropic run with k / 2, rho_c / 2 on the z-doubled mesh, fallbacks): same
    Dirichlet dofs and values - the boundary conditions are located once, on the unstretched mesh."""
    from heatflow_amd.solver import HeatProblem

    cfg, stack, mesh = case
    tk, trc = material_tables(stack, mesh)
    dt = float(cfg["timing"]["t_final"]) / int(cfg["timing"]["num_steps"])
    cs, ks, rcs = stretched(mesh.coords, tk, trc, 2.0)
    out, fallbacks = [], 0
    for coords, k, rc, kw in ((mesh.coords, tk, trc, {"k_aniso": {t: (1.0, 0.25) for t in tk}}), (cs, ks, rcs, {})):
        bcs, ic, _ = reference_bcs(cfg, stack, mesh)
        prob = HeatProblem(coords, mesh.tris, mesh.tags, k, rc, dt, bcs, ic, precond=precond, **kw)
        try:
            sel = np.arange(prob.n, dtype=np.int32) if nodes is None else nodes
            _, s, iters = prob.run(nsteps, watcher_nodes=sel, time_varying=[prob.bcs[3]])
            out.append((s, prob.state(), np.asarray(iters)))
            if precond == 1:
                fallbacks += prob.backend.amg_info()["jacobi_fallbacks"]
        finally:
            prob.close()
    return out[0], out[1], fallbacks


@pytest.mark.parametrize("precond", [0, 1])
@pytest.mark.parametrize("case", ["geballe_with_diamond", "geballe_no_diamond"])
def test_stretch_identity_on_the_small_meshes(hip, request, case, precond):
    c = _case(case, request)
    (sa, ua, _), (si, ui, _), _ = _stretch_pair(c, precond, NSTEPS)
    worst = max(float(np.abs(sa - si).max()), float(np.abs(ua - ui).max()))
    cfg, stack, mesh = c
    tk, trc, dt, dofs, u0, g = problem_inputs(cfg, stack, mesh, NSTEPS)
    iso = linear_fields(mesh.coords, mesh.tris, mesh.tags, tk, trc, dt, dofs, u0, g)
    print(f"{case} precond={precond}: anisotropic vs stretched isotropic {worst:.2e} K; the anisotropy moves the field by "
          f"{np.abs(sa - iso).max():.1f} K")
    assert worst <= STRETCH_TOL_K
    assert np.abs(sa - iso).max() > 10.0


def test_stretch_identity_at_one_million_dof_with_multigrid(hip):
    c3 = build_case("geballe_with_diamond", 0.43)
    n = len(c3[2].coords)
    assert abs(n - 1.0e6) <= 0.05e6
    nodes = np.arange(0, n, 101, dtype=np.int32)
    (sa, ua, ita), (si, ui, iti), fallbacks = _stretch_pair(c3, 1, NSTEPS, nodes)
    worst = max(float(np.abs(sa - si).max()), float(np.abs(ua - ui).max()))
    print(f"C3 ({n} DOF): anisotropic vs stretched isotropic {worst:.2e} K; iterations/step anisotropic {ita.mean():.1f}, "
          f"stretched isotropic {iti.mean():.1f}; multigrid fallbacks {fallbacks}")
    assert worst <= 1e-4
    assert fallbacks == 0
    assert np.abs(ua - 300.0).max() > 10.0


# 4. steady state and hold load ------------------------------------------------------------------------------------------------
def _steady_problem(case, bcs, precond, aniso, **kw):
    from heatflow_amd.solver import HeatProblem

    cfg, stack, mesh = case
    tk, trc = material_tables(stack, mesh)
    dt = float(cfg["timing"]["t_final"]) / int(cfg["timing"]["num_steps"])
    kw.setdefault("max_it", STEADY_MAX_IT)
    return HeatProblem(mesh.coords, mesh.tris, mesh.tags, tk, trc, dt, bcs, float(cfg["heating"]["ic_temp"]), precond=precond,
                       k_aniso=aniso, **kw)


@pytest.mark.parametrize("precond", [0, 1])
@pytest.mark.parametrize("case", ["geballe_with_diamond", "geballe_no_diamond"])
def test_steady_state_hold_load_and_no_drift(hip, request, case, precond):
    from heatflow_amd.bc import gather_bc_values, merge_bcs

    c = _case(case, request)
    cfg, stack, mesh = c
    ic = float(cfg["heating"]["ic_temp"])
    aniso = mixed_multipliers(mesh)
    tk, trc = material_tables(stack, mesh)
    _, K = matrices(mesh.coords, mesh.tris, mesh.tags, tk, trc, aniso)
    _, K_iso = matrices(mesh.coords, mesh.tris, mesh.tags, tk, trc, {})
    sb = steady_bcs(cfg, stack, mesh, ic + 5.0, ic + 2.0)
    # the held lines first, the outer boundary last: where a line ends on the outer boundary (no-diamond: at r_max) the later
    # entry wins, so the steady state has there the value the transient's Dirichlet rows hold - otherwise that node alone
    # would jump by the line's amplitude at the first step, whatever the load
    sb = sb[3:] + sb[:3]
    dofs, owner, pos = merge_bcs(sb)
    for bc in sb:
        bc.update(0.0)
    g = gather_bc_values(sb, owner, pos)
    ref = steady_solve(K, dofs, g)
    assert ref.max() > ic + 4.9
    prob = _steady_problem(c, sb[-3:], precond, aniso, rtol=STEADY_RTOL)
    try:
        u, it, _ = prob.solve_steady(sb)
        err = float(np.abs(u - ref).max())
        moved = float(np.abs(ref - steady_solve(K_iso, dofs, g)).max())
        print(f"steady {case} precond={precond}: {it} iterations, max |u - u_direct| = {err:.2e} K; isotropic differs by {moved:.2e} K")
        assert err <= FIELD_TOL_K
        assert moved > 100 * FIELD_TOL_K
        F = prob.hold_load()
        B = np.asarray(prob.bc_dofs)
        assert np.all(F[B] == 0.0)
        bound = ENTRY_TOL * (abs(K) @ np.abs(u))
        assert np.all(np.abs(F - hold_load(K, u, B)) <= bound)                  # K u entry by entry
        assert np.abs(F - hold_load(K_iso, u, B)).max() > 1e3 * bound.max()     # (not the isotropic stiffness)
        prob.rtol = 1e-10
        worst = 0.0
        for k in range(10):
            prob.step((k + 1) * prob.dt)
            worst = max(worst, float(np.abs(prob.state() - u).max()))
        print(f"no drift {case} precond={precond}: {worst:.2e} K over 10 steps")
        assert worst <= 1e-5
    finally:
        prob.close()


# 5. sweeps --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precond", [0, 1])
def test_affine_kappa_batch_on_an_anisotropic_sample_matches_single_runs(hip, case_with_diamond_small, precond):
    cfg, stack, mesh = case_with_diamond_small
    nv, nsteps = 4, 12
    ks = [3.3 + 0.3 * j for j in range(nv)]
    tag_s = mesh.material_tags["p_sample"]
    aniso = mixed_multipliers(mesh)
    assert tag_s in aniso
    prob = make_problem(cfg, stack, mesh, precond=precond, amg_reuse=True, k_aniso=aniso)
    be = prob.backend
    try:
        for bc in prob.bcs:
            bc.update(0.0)
        g_one = np.array([prob.bc_values((k + 1) * prob.dt, [prob.bcs[3]]) for k in range(nsteps)])
        singles = []
        for kap in ks:
            be.update_kappa([tag_s], [kap])
            prob.set_state(300.0)
            be.run(g_one, prob.rtol, 0.0, prob.max_it, None)
            singles.append(prob.state())
        tk, trc, dt, dofs, u0, _ = problem_inputs(cfg, stack, mesh, 1)
        ref = aniso_fields(mesh.coords, mesh.tris, mesh.tags, {**tk, tag_s: ks[0]}, trc, dt, dofs, u0, g_one, aniso)
        assert np.abs(singles[0] - ref[-1]).max() <= FIELD_TOL_K               # the single runs are the restatement's
        ref_k = ks[nv // 2]
        be.update_kappa([tag_s], [ref_k])
        be.batch_begin(nv, per_column_operator=hip.BATCH_AFFINE)
        be.batch_set_affine([tag_s], [kap - ref_k for kap in ks])
        for j in range(nv):
            be.batch_set_state(j, np.full(prob.n, 300.0))
        be.batch_run(np.repeat(g_one[:, :, None], nv, axis=2), prob.rtol, 0.0, prob.max_it, None)
        for j in range(nv):
            d = float(np.abs(be.batch_get_state(j) - singles[j]).max())
            print(f"affine batch precond={precond} column {j}: {d:.2e} K")
            assert d <= SINGLE_RUN_TOL_K
        be.batch_end()
        assert np.abs(singles[0] - singles[-1]).max() > 100 * SINGLE_RUN_TOL_K
    finally:
        prob.close()


@pytest.mark.parametrize("precond", [0, 1])
def test_shared_operator_fwhm_batch_matches_single_runs(hip, case_no_diamond_small, precond):
    from conftest import HEATING_CSV
    from heatflow_amd.heating import HeatingCurve

    cfg, stack, mesh = case_no_diamond_small
    nsteps, nv = 14, 4
    fwhms = [8e-6, 1.32e-5, 2e-5, 4e-5]
    prob = make_problem(cfg, stack, mesh, precond=precond, k_aniso=mixed_multipliers(mesh))
    be = prob.backend
    try:
        ic = float(cfg["heating"]["ic_temp"])
        g_cols, singles = [], []
        for f in fwhms:
            prob.bcs[3]._value = HeatingCurve(HEATING_CSV, ic, f).gaussian
            for bc in prob.bcs:
                bc.update(0.0)
            g = np.array([prob.bc_values((k + 1) * prob.dt, [prob.bcs[3]]) for k in range(nsteps)])
            g_cols.append(g)
            prob.set_state(ic)
            be.run(g, prob.rtol, 0.0, prob.max_it, None)
            singles.append(prob.state())
        be.batch_begin(nv, per_column_operator=False)
        for j in range(nv):
            be.batch_set_state(j, np.full(prob.n, ic))
        be.batch_run(np.stack(g_cols, axis=2), prob.rtol, 0.0, prob.max_it, None)
        for j in range(nv):
            assert np.abs(be.batch_get_state(j) - singles[j]).max() <= SINGLE_RUN_TOL_K
        be.batch_end()
        assert np.abs(singles[0] - singles[3]).max() > 1.0
    finally:
        prob.close()


def test_update_kappa_on_an_anisotropic_tag_equals_a_set_up_from_scratch(hip, case_with_diamond_small):
    cfg, stack, mesh = case_with_diamond_small
    tk, trc, dt, *_ = problem_inputs(cfg, stack, mesh, 1)
    aniso = mixed_multipliers(mesh)
    tag_s = mesh.material_tags["p_sample"]
    tags = sorted(tk)
    with hip.HeatflowHIP(0) as be:
        be.set_mesh(mesh.coords, mesh.tris, mesh.tags)
        be.set_materials(tags, [tk[t] for t in tags], [trc[t] for t in tags])
        be.set_anisotropy(aniso)
        be.set_dirichlet(np.zeros(0, dtype=np.int32))
        be.assemble(dt, hip.ASM_ROW_GATHER)
        _, _, A_before, _ = be.get_csr()
        be.update_kappa([tag_s], [4.4])
        _, _, A_upd, M_upd = be.get_csr()
    _, _, A_new, M_new = _assembled(hip, mesh, {**tk, tag_s: 4.4}, trc, dt, aniso)
    assert np.array_equal(A_upd, A_new) and np.array_equal(M_upd, M_new)
    assert not np.array_equal(A_upd, A_before)


def test_multipliers_stay_over_a_later_set_materials(hip, case_with_diamond_small):
    cfg, stack, mesh = case_with_diamond_small
    tk, trc, dt, *_ = problem_inputs(cfg, stack, mesh, 1)
    aniso = mixed_multipliers(mesh)
    tags = sorted(tk)
    tk2 = {t: 1.5 * v for t, v in tk.items()}
    trc2 = {t: 0.75 * v for t, v in trc.items()}
    with hip.HeatflowHIP(0) as be:
        be.set_mesh(mesh.coords, mesh.tris, mesh.tags)
        be.set_materials(tags, [tk[t] for t in tags], [trc[t] for t in tags])
        be.set_anisotropy(aniso)
        be.set_dirichlet(np.zeros(0, dtype=np.int32))
        be.assemble(dt, hip.ASM_ROW_GATHER)
        be.set_materials(tags, [tk2[t] for t in tags], [trc2[t] for t in tags])   # no hf_set_anisotropy after it
        be.assemble(dt, hip.ASM_ROW_GATHER)
        _, _, A_kept, M_kept = be.get_csr()
    _, _, A_new, M_new = _assembled(hip, mesh, tk2, trc2, dt, aniso)
    _, _, A_iso, _ = _assembled(hip, mesh, tk2, trc2, dt, None)
    assert np.array_equal(A_kept, A_new) and np.array_equal(M_kept, M_new)
    assert not np.array_equal(A_kept, A_iso)


# 6. tangent on an isotropic tag -------------------------------------------------------------------------------------------------
def test_tangent_on_an_isotropic_tag_matches_central_differences(hip, case_with_diamond_small):
    """d/dk of a material that stays isotropic (the p-side coupler, the most sensitive of them) while the insulators and the
    sample are anisotropic, against central differences of primal runs at rtol = 1e-12 (the method of tests/test_gpu_tangent.py),
    bound 1e-6 of max |s|.
    The quotient is the fourth-order central one, (8 (f(+h) - f(-h)) - (f(+2h) - f(-2h))) / (12 h), with h = 1e-2 k over 40
    steps.  Measured on the restatement (sparse LU, no solver error): the second-order quotient at h = 1e-3 k, which
    tests/test_gpu_tangent.py checks to 1e-4, has a truncation error of 1.0e-6 of max |s| here - the bound itself - while this one
    has 3.7e-8 at h = 1e-2 k (6.4e-7 at 2e-2 k: the h^4 law), and max |s| k = 0.114 K, so that an error eps of the primal runs
    enters as 1.5 eps / (1e-2 * 0.114 K): the bound leaves 7.6e-10 K for it.  Both quotients' figures are printed."""
    import copy

    from heatflow_amd.geometry import build_stack

    cfg, stack, mesh = case_with_diamond_small
    aniso = mixed_multipliers(mesh)
    name, nsteps, rel = "p_coupler", 40, 1e-2
    tag = mesh.material_tags[name]
    assert tag not in aniso
    nodes = np.arange(0, len(mesh.coords), max(1, len(mesh.coords) // 50), dtype=np.int32)
    prob = make_problem(cfg, stack, mesh, precond=1, rtol=1e-12, k_aniso=aniso)
    try:
        _, _, ts, _, _ = prob.run_tangent(nsteps, nodes, conductivity=[[tag]], time_varying=[prob.bcs[3]])
    finally:
        prob.close()
    k0 = float(cfg["mats"][name]["k"])
    runs = {}
    for m in (2, 1, -1, -2):
        c = copy.deepcopy(cfg)
        c["mats"][name]["k"] = k0 * (1 + m * rel)
        p = make_problem(c, build_stack(c), mesh, precond=1, rtol=1e-12, k_aniso=aniso)
        try:
            runs[m] = p.run(nsteps, nodes, time_varying=[p.bcs[3]])[1]
        finally:
            p.close()
    h = rel * k0
    fd2 = (runs[1] - runs[-1]) / (2 * h)
    fd4 = (8.0 * (runs[1] - runs[-1]) - (runs[2] - runs[-2])) / (12 * h)
    scale = float(np.max(np.abs(ts[:, 0])))
    assert scale > 0
    e2, e4 = float(np.max(np.abs(ts[:, 0] - fd2))), float(np.max(np.abs(ts[:, 0] - fd4)))
    print(f"tangent on {name}: max |s| k = {scale * k0:.3e} K; |s - FD2| / max|s| = {e2 / scale:.2e}, |s - FD4| / max|s| = {e4 / scale:.2e}")
    assert e4 <= 1e-6 * scale


# 7. refusals and staleness -------------------------------------------------------------------------------------------------------
def test_refusals_bad_arguments_and_staleness(hip, case_with_diamond_small):
    cfg, stack, mesh = case_with_diamond_small
    tk, trc, dt, dofs, *_ = problem_inputs(cfg, stack, mesh, 1)
    aniso = mixed_multipliers(mesh)
    t_an, t_iso = mesh.material_tags["p_sample"], mesh.material_tags["p_coupler"]
    table = {t_iso: (300.0, 10.0, [1.0, 2.0])}
    prob = make_problem(cfg, stack, mesh, k_aniso=aniso)
    b = prob.backend
    try:
        # tables, the Picard set-up and a tangent column on an anisotropic tag are refused while a tag is anisotropic
        for call, text in ((lambda: b.set_kappa_tables(table), "hf_set_kappa_tables: anisotropic"),
                           (lambda: b.set_rhoc_tables(table), "hf_set_rhoc_tables: anisotropic"),
                           (lambda: b.steady_picard_setup(prob.bc_dofs), "hf_steady_picard_setup: anisotropic")):
            with pytest.raises(hip.HipError, match=text) as e:
                call()
            assert e.value.code == hip.HF_ERR_STATE
        with pytest.raises(ValueError, match=f"hf_tangent_setup: tag {t_an} is anisotropic"):
            b.tangent_setup(1, {t_an: 0})
        b.tangent_setup(1, {t_iso: 0})                                         # an isotropic tag is fine
        # a listed tag with m_r == m_z != 1 is assembled by the isotropic element routine but is no tangent column either: its
        # conductivity is m kappa, not kappa.  (1, 1) is an isotropic tag and stays one.
        b.set_anisotropy({**aniso, t_iso: (3.0, 3.0)})
        with pytest.raises(ValueError, match=f"hf_tangent_setup: tag {t_iso} is anisotropic"):
            b.tangent_setup(1, {t_iso: 0})
        b.set_anisotropy({**aniso, t_iso: (1.0, 1.0)})
        b.assemble(prob.dt, hip.ASM_ROW_GATHER)
        b.tangent_setup(1, {t_iso: 0})
        with pytest.raises(ValueError, match="hf_assemble: anisotropic conductivities"):
            b.assemble(prob.dt, hip.ASM_LDS_COLORED)
        # bad arguments
        for bad, text in (({999: (2.0, 0.25)}, "not a cell tag"), ({t_an: (0.0, 1.0)}, "positive and finite"),
                          ({t_an: (1.0, -1.0)}, "positive and finite"), ({t_an: (np.nan, 1.0)}, "positive and finite"),
                          ({t_an: (np.inf, 1.0)}, "positive and finite")):
            with pytest.raises(ValueError, match=f"hf_set_anisotropy.*{text}"):
                b.set_anisotropy(bad)
        i32, f64 = np.array([t_an, t_an], dtype=np.int32), np.array([2.0, 2.0])
        import ctypes

        pi, pd = ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_double)
        assert b._lib.hf_set_anisotropy(b._ctx, 2, i32.ctypes.data_as(pi), f64.ctypes.data_as(pd), f64.ctypes.data_as(pd)) == hip.HF_ERR_ARG
        assert "listed twice" in b._lib.hf_last_error(b._ctx).decode()
        assert b._lib.hf_set_anisotropy(b._ctx, -1, None, None, None) == hip.HF_ERR_ARG
        assert b._lib.hf_set_anisotropy(b._ctx, 1, None, None, None) == hip.HF_ERR_ARG
        # a refused call changed nothing: the problem still steps on the anisotropic operator
        b.assemble(prob.dt, hip.ASM_ROW_GATHER)
        prob.step(prob.dt, [prob.bcs[3]])
        # a steady set-up and a tangent made before hf_set_anisotropy are stale after it
        b.steady_setup(prob.bc_dofs)
        b.tangent_setup(1, {t_iso: 0})
        b.set_anisotropy({t_an: (4.0, 0.5)})
        g = np.zeros(len(prob.bc_dofs))
        with pytest.raises(hip.HipError, match="hf_steady_solve before hf_steady_setup") as e:
            b.steady_solve(g)
        assert e.value.code == hip.HF_ERR_STATE
        with pytest.raises(hip.HipError, match="hf_run_tangent") as e:
            b.run_tangent(np.zeros((1, len(prob.bc_dofs))))
        assert e.value.code == hip.HF_ERR_STATE
        with pytest.raises(hip.HipError) as e:                                 # and so is the assembly
            b.step(prob.bc_values(0.0), 1e-10, 0.0, 100)
        assert e.value.code == hip.HF_ERR_STATE
        # clearing with n = 0 restores the isotropic bits, and tables are accepted again
        b.set_anisotropy({})
        b.assemble(prob.dt, hip.ASM_ROW_GATHER)
        _, _, A_cleared, M_cleared = b.get_csr()
        b.set_kappa_tables(table)
        # ... after which hf_set_anisotropy is refused, in this order too
        with pytest.raises(hip.HipError, match=r"hf_set_anisotropy: kappa\(T\) tables are set") as e:
            b.set_anisotropy(aniso)
        assert e.value.code == hip.HF_ERR_STATE
        b.set_kappa_tables({})
        b.set_rhoc_tables(table)
        with pytest.raises(hip.HipError, match=r"hf_set_anisotropy: rho_c\(T\) tables are set"):
            b.set_anisotropy(aniso)
        b.set_rhoc_tables({})
        b.set_anisotropy({})                                                   # clearing nothing is always fine
        # after an assembly in another mode, anisotropy is refused
        b.assemble(prob.dt, hip.ASM_LDS_COLORED)
        with pytest.raises(ValueError, match="hf_set_anisotropy.*row-gather"):
            b.set_anisotropy(aniso)
    finally:
        prob.close()
    plain = make_problem(cfg, stack, mesh)
    try:
        _, _, A0, M0 = plain.backend.get_csr()
    finally:
        plain.close()
    assert np.array_equal(A_cleared, A0) and np.array_equal(M_cleared, M0)
    # before hf_set_materials
    with hip.HeatflowHIP(0) as be:
        be.set_mesh(mesh.coords, mesh.tris, mesh.tags)
        with pytest.raises(hip.HipError, match="hf_set_anisotropy needs") as e:
            be.set_anisotropy(aniso)
        assert e.value.code == hip.HF_ERR_STATE


# 8. a multigrid hierarchy kept (hf_set_precond(1, reuse = 1)) or installed across a change of the multipliers -------------------
_REFS = {}


def _restated(case, aniso, nsteps=NSTEPS):
    """Every field of the restatement for the multipliers ``aniso`` ({}: the linear oracle), computed once per set."""
    cfg, stack, mesh = case
    key = (id(mesh), tuple(sorted(aniso.items())), nsteps)
    if key not in _REFS:
        tk, trc, dt, dofs, u0, g = problem_inputs(cfg, stack, mesh, nsteps)
        _REFS[key] = (aniso_fields(mesh.coords, mesh.tris, mesh.tags, tk, trc, dt, dofs, u0, g, aniso, BE) if aniso else
                      linear_fields(mesh.coords, mesh.tris, mesh.tags, tk, trc, dt, dofs, u0, g, BE))
        _REFS[key].setflags(write=False)
    return _REFS[key]


def _loop(prob, ic, nsteps=NSTEPS):
    """(every field, iterations per step, multigrid fallbacks) of ``nsteps`` hf_step calls from the uniform state."""
    prob.set_state(ic)
    for bc in prob.bcs:
        bc.update(0.0)
    fb0, it0 = prob.backend.amg_info()["jacobi_fallbacks"], len(prob.iters)
    fields = []
    for k in range(nsteps):
        prob.step((k + 1) * prob.dt, [prob.bcs[3]])
        fields.append(prob.state())
    return np.array(fields), list(prob.iters)[it0:], prob.backend.amg_info()["jacobi_fallbacks"] - fb0


def _reassembled(prob, aniso):
    prob.backend.set_anisotropy(aniso)
    prob.backend.assemble(prob.dt, prob.assembly_mode)


def test_a_kept_hierarchy_is_a_frozen_one_after_the_multipliers_change(hip, case_with_diamond_small):
    """The multipliers are part of the operator's fingerprint: a hierarchy built from the isotropic A meets the anisotropic A as
    a frozen one (explicit finest-level legs over the new A - the fused down leg holds the old one and would leave the cycle
    unsymmetric), and clearing the multipliers gives the hierarchy its own operator back, bit for bit a fresh context's loop."""
    cfg, stack, mesh = case_with_diamond_small
    ic = float(cfg["heating"]["ic_temp"])
    aniso = mixed_multipliers(mesh)
    other = {t: (0.5, 4.0) for t in aniso}
    prob = make_problem(cfg, stack, mesh, precond=1, amg_reuse=True)           # assembled isotropic, hierarchy from that A
    try:
        assert prob.backend.amg_info()["levels"] >= 2
        u_iso, it_iso, fb = _loop(prob, ic)
        assert fb == 0 and np.abs(u_iso - _restated(case_with_diamond_small, {})).max() <= FIELD_TOL_K
        for an in (aniso, other):                                              # isotropic -> one set -> another set
            _reassembled(prob, an)
            u, it, fb = _loop(prob, ic)
            worst = float(np.abs(u - _restated(case_with_diamond_small, an)).max())
            print(f"kept hierarchy, multipliers {sorted(set(an.values()))}: worst |dT| = {worst:.2e} K, iterations/step mean "
                  f"{np.mean(it):.1f} (isotropic {np.mean(it_iso):.1f}), multigrid fallbacks {fb}")
            assert worst <= FIELD_TOL_K and fb == 0
            assert np.abs(u - u_iso).max() > 10.0
        _reassembled(prob, {})
        u_back, it_back, fb = _loop(prob, ic)
        assert fb == 0 and it_back == it_iso and np.array_equal(u_back, u_iso)
    finally:
        prob.close()


def test_an_installed_hierarchy_knows_the_multipliers_it_was_built_for(hip, case_with_diamond_small):
    """hf_amg_export / hf_amg_install carry the multipliers in the fingerprint: the same multipliers -> the exporting context's
    loop bit for bit; other multipliers (or none) -> a frozen hierarchy, bit for bit what the exporting context runs after
    changing its own multipliers, the restatement's fields and no fallbacks."""
    c = case_with_diamond_small
    cfg, stack, mesh = c
    ic = float(cfg["heating"]["ic_temp"])
    aniso = mixed_multipliers(mesh)
    other = {t: (0.5, 4.0) for t in aniso}
    a = make_problem(cfg, stack, mesh, precond=1, amg_reuse=True, k_aniso=aniso)
    try:
        blob = a.backend.amg_export()
        ua, ita, fb = _loop(a, ic)
        assert fb == 0 and np.abs(ua - _restated(c, aniso)).max() <= FIELD_TOL_K
        kept = {}
        for name, an in (("other", other), ("none", {})):
            _reassembled(a, an)
            kept[name] = _loop(a, ic)
    finally:
        a.close()
    for name, an in (("same", aniso), ("other", other), ("none", {})):
        b = make_problem(cfg, stack, mesh, precond=1, amg_reuse=True, amg=blob, **({"k_aniso": an} if an else {}))
        try:
            u, it, fb = _loop(b, ic)
        finally:
            b.close()
        worst = float(np.abs(u - _restated(c, an)).max())
        print(f"installed hierarchy, {name} multipliers: worst |dT| = {worst:.2e} K, iterations/step mean {np.mean(it):.1f} "
              f"(exporter {np.mean(ita):.1f}), multigrid fallbacks {fb}")
        assert worst <= FIELD_TOL_K and fb == 0
        if name == "same":
            assert it == ita and np.array_equal(u, ua)
        else:
            assert it == kept[name][1] and np.array_equal(u, kept[name][0]) and kept[name][2] == 0


def test_run_simulation_end_to_end_with_the_example_configuration(hip, tmp_path):
    import os

    import yaml

    from conftest import load_cfg
    from heatflow_amd.geometry import scale_mesh_sizes
    from heatflow_amd.parameter_sweep import get_watcher_points
    from heatflow_amd.run_with_diamond import run_simulation

    cfg = scale_mesh_sizes(load_cfg("geballe_with_diamond_aniso"), 8.0)
    cfg["timing"]["num_steps"] = 40
    out = str(tmp_path / "out")
    res = run_simulation(cfg, str(tmp_path / "mesh"), rebuild_mesh=True, output_folder=out, watcher_points=get_watcher_points(cfg),
                         write_xdmf=False, suppress_print=True)
    with open(os.path.join(out, "used_config.yaml")) as f:
        used = yaml.safe_load(f)
    assert used["mats"]["p_ins"]["k_aniso"] == {"r": 2.0, "z": 0.25} and "k_aniso" not in used["mats"]["p_sample"]
    base = scale_mesh_sizes(load_cfg("geballe_with_diamond"), 8.0)
    base["timing"]["num_steps"] = 40
    res0 = run_simulation(base, str(tmp_path / "mesh"), output_folder=str(tmp_path / "out0"), watcher_points=get_watcher_points(base),
                          write_xdmf=False, suppress_print=True)
    moved = float(np.abs(np.asarray(res["watchers"]["oside"]) - np.asarray(res0["watchers"]["oside"])).max())
    print(f"o-side watcher moves by {moved:.2f} K under the example anisotropy (coarse mesh, 40 steps)")
    assert moved > 1.0
