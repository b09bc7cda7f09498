"""Picard steady state and pre-heated transients under kappa(T) / rho_c(T) tables on the GPU (hf_steady_picard_setup /
hf_steady_picard_solve) against the restatement of tests/steady_picard_oracle.py: the fixed point, the held
load as K(u) u entry by entry, no drift of a held state (both preconditioners, both schemes, 1 and 3 Picard sweeps per step,
with and without capacity tables, from a converged and from an unconverged iterate), a pulse on top of the held state, the
degenerate cases bit for bit, the refusals, and 1.04 M DOF with multigrid."""
import ctypes

import numpy as np
import pytest

from conftest import build_case
from helpers import material_tables, reference_bcs
from heatflow_amd.bc import gather_bc_values, merge_bcs
from rhoc_T_oracle import einstein_tables
from steady_picard_oracle import BDF2, BE, loaded_fields, nl_residual, picard_steady, stiffness
from test_steady_cpu import steady_bcs

pytestmark = pytest.mark.gpu

STEADY_MAX_IT = 400000     # as tests/test_gpu_steady.py: Jacobi-PCG on the stiffness alone needs many iterations
STEADY_RTOL = 1e-12
PICARD_TOL = 1e-7
CASES = {"with_diamond_small": "geballe_with_diamond", "no_diamond_small": "geballe_no_diamond"}


@pytest.fixture(scope="module")
def small_cases():
    return {k: build_case(v, 8.0) for k, v in CASES.items()}


def _ins_tags(stack, mesh):
    return [mesh.material_tags[m.name] for m in stack.materials if m.name.endswith("ins")]


def _ins_tables(stack, mesh, tag_to_k):
    """1/T tables for the pressure media, 300..800 K at 51 knots (those of tests/test_gpu_kappa_T.py)."""
    T = 300.0 + 10.0 * np.arange(51)
    return {t: (300.0, 10.0, tag_to_k[t] * 300.0 / T) for t in _ins_tags(stack, mesh)}


def _cv_tables(stack, mesh, tag_to_rc):
    """Einstein tables (theta = 600 K) for the pressure media (those of tests/test_gpu_rhoc_T.py)."""
    return einstein_tables(tag_to_rc, _ins_tags(stack, mesh))


def _hot_bcs(case):
    cfg, stack, mesh = case
    ic = float(cfg["heating"]["ic_temp"])
    return steady_bcs(cfg, stack, mesh, ic + 400.0, ic + 250.0)


def _steady_set(sb):
    dofs, owner, pos = merge_bcs(sb)
    for bc in sb:
        bc.update(0.0)
    return np.asarray(dofs, dtype=np.int64), gather_bc_values(sb, owner, pos)


def problem(case, bcs, precond, **kw):
    from heatflow_amd.solver import HeatProblem

    cfg, stack, mesh = case
    tk, trc = material_tables(stack, mesh)
    dt = float(cfg["timing"]["t_final"]) / int(cfg["timing"]["num_steps"])
    kw.setdefault("max_it", STEADY_MAX_IT)
    kw.setdefault("rtol", STEADY_RTOL)
    return HeatProblem(mesh.coords, mesh.tris, mesh.tags, tk, trc, dt, bcs, float(cfg["heating"]["ic_temp"]), precond=precond, **kw)


def _oracle_fixed_point(case, sb, tables, tol=PICARD_TOL):
    cfg, stack, mesh = case
    tk, _ = material_tables(stack, mesh)
    dofs, g = _steady_set(sb)
    x0 = np.full(len(mesh.coords), float(cfg["heating"]["ic_temp"]))
    return picard_steady(mesh.coords, mesh.tris, mesh.tags, tk, dofs, g, x0, tables, picard_tol=tol, max_sweeps=60)


# 1. the fixed point ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precond", [0, 1])
@pytest.mark.parametrize("which", sorted(CASES))
def test_fixed_point_matches_the_restatement(hip, small_cases, which, precond):
    case = small_cases[which]
    cfg, stack, mesh = case
    tk, _ = material_tables(stack, mesh)
    tables = _ins_tables(stack, mesh, tk)
    sb = _hot_bcs(case)
    dofs, g = _steady_set(sb)
    ref = _oracle_fixed_point(case, sb, tables)
    lin = _oracle_fixed_point(case, sb, None)
    ch = np.array(ref["changes"])
    assert ref["converged"] and np.all(ch[1:] / ch[:-1] < 0.3), ch          # the contraction the bound below relies on
    prob = problem(case, sb[:3], precond, kappa_tables=tables)
    try:
        u, it, res = prob.solve_steady(sb, picard_tol=PICARD_TOL)
        info = prob.steady_info
        fallbacks = prob.backend.amg_info()["jacobi_fallbacks"] if precond else 0
    finally:
        prob.close()
    err = float(np.abs(u - ref["u"]).max())
    moved = float(np.abs(ref["u"] - lin["u"]).max())
    restated = nl_residual(stiffness(mesh.coords, mesh.tris, mesh.tags, tk, u, tables), dofs, g, u)
    print(f"fixed point {which} precond={precond}: {info['sweeps']} sweeps (oracle {ref['sweeps']}), PCG iterations {info['iters']}, "
          f"change {info['change']:.2e} K, nl_resid {info['nl_resid']:.2e} (restated {restated:.2e}, oracle's own {ref['nl_resid']:.2e}), "
          f"max |u - u_oracle| = {err:.2e} K, tables move the field by {moved:.1f} K, fallbacks {fallbacks}")
    assert err <= 1e-4, f"{err:.3e} K"
    assert info["sweeps"] <= ref["sweeps"] + 1
    assert info["change"] <= PICARD_TOL and len(info["iters"]) == info["sweeps"] and it == sum(info["iters"])
    assert res == info["nl_resid"]
    assert info["nl_resid"] <= 1e-10 or restated / 10.0 <= info["nl_resid"] <= restated * 10.0
    assert moved > 30.0
    assert np.array_equal(u[dofs], g)


# 2. the operator: the held load is K(u) u ---------------------------------------------------------------------------------------
def _check_hold_load(mesh, tk, tables, u, F, B):
    K = stiffness(mesh.coords, mesh.tris, mesh.tags, tk, u, tables)
    ref = K @ u
    scale = abs(K) @ np.abs(u)
    free = np.setdiff1d(np.arange(len(u)), B)
    assert np.all(F[B] == 0.0)
    worst = float((np.abs(F - ref)[free] / scale[free]).max())
    assert np.all(np.abs(F - ref)[free] <= 1e-13 * scale[free]), worst
    return worst


@pytest.mark.parametrize("precond", [0, 1])
def test_held_load_is_the_stiffness_at_the_returned_state_times_that_state(hip, small_cases, precond):
    case = small_cases["with_diamond_small"]
    cfg, stack, mesh = case
    tk, _ = material_tables(stack, mesh)
    tables = _ins_tables(stack, mesh, tk)
    sb = _hot_bcs(case)
    bcs, _, _ = reference_bcs(cfg, stack, mesh)                    # the transient's set B: outer boundary + the p-side line
    prob = problem(case, bcs, precond, kappa_tables=tables)
    try:
        u, _, _ = prob.solve_steady(sb, picard_tol=PICARD_TOL)
        F = prob.hold_load()
        B = np.asarray(prob.bc_dofs)
    finally:
        prob.close()
    worst = _check_hold_load(mesh, tk, tables, u, F, B)
    o_line = np.setdiff1d(sb[4].row_dofs, B)
    assert np.abs(F[o_line]).max() > 0.0                           # the o-side line is free in the transient: the load holds it
    print(f"held load precond={precond}: worst |F - K(u) u| / (|K| |u|) = {worst:.2e}")


# 3. no drift ----------------------------------------------------------------------------------------------------------------------
def _no_drift(case, precond, scheme, picard, with_cv, nsteps=10, **solve_kw):
    from heatflow_amd import hip_backend

    cfg, stack, mesh = case
    tk, trc = material_tables(stack, mesh)
    kw = {"kappa_tables": _ins_tables(stack, mesh, tk)}
    if with_cv:
        kw["rhoc_tables"] = _cv_tables(stack, mesh, trc)
    sb = _hot_bcs(case)
    prob = problem(case, sb[:3], precond, scheme=scheme, picard=picard, **kw)
    try:
        converged = True
        try:
            prob.solve_steady(sb, **solve_kw)
        except hip_backend.NotConverged:
            converged = False
        u_ss = prob.state()
        prob.hold_load()
        worst = 0.0
        for k in range(nsteps):
            prob.step((k + 1) * prob.dt)
            worst = max(worst, float(np.abs(prob.state() - u_ss).max()))
            assert worst <= 1e-5, f"step {k}: {worst:.3e} K"
        fallbacks = prob.backend.amg_info()["jacobi_fallbacks"] if precond else 0
        return converged, worst, float(u_ss.max() - u_ss.min()), fallbacks
    finally:
        prob.close()


@pytest.mark.parametrize("with_cv", [False, True])
@pytest.mark.parametrize("picard", [1, 3])
@pytest.mark.parametrize("scheme", ["backward_euler", "bdf2"])
@pytest.mark.parametrize("precond", [0, 1])
def test_hold_load_keeps_the_picard_steady_state(hip, small_cases, precond, scheme, picard, with_cv):
    converged, worst, span, fb = _no_drift(small_cases["with_diamond_small"], precond, scheme, picard, with_cv, picard_tol=PICARD_TOL)
    print(f"no drift precond={precond} {scheme} p={picard} cv={with_cv}: max drift {worst:.2e} K over a field spanning {span:.0f} K, "
          f"fallbacks {fb}")
    assert converged and span > 399.0


@pytest.mark.parametrize("precond", [0, 1])
def test_hold_load_keeps_an_unconverged_picard_iterate(hip, small_cases, precond):
    converged, worst, span, fb = _no_drift(small_cases["with_diamond_small"], precond, "backward_euler", 1, True,
                                           picard_tol=PICARD_TOL, max_sweeps=2)
    print(f"no drift from sweep 2 precond={precond}: max drift {worst:.2e} K, fallbacks {fb}")
    assert not converged and span > 399.0          # two sweeps are not enough: HF_ERR_NOCONV, and the iterate still holds


# 4. a pulse on top of the held state ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_cv", [False, True])
@pytest.mark.parametrize("scheme", ["backward_euler", "bdf2"])
@pytest.mark.parametrize("precond", [0, 1])
def test_pulse_from_the_held_state_matches_the_restated_loop(hip, small_cases, precond, scheme, with_cv):
    case = small_cases["with_diamond_small"]
    cfg, stack, mesh = case
    tk, trc = material_tables(stack, mesh)
    kt = _ins_tables(stack, mesh, tk)
    ct = _cv_tables(stack, mesh, trc) if with_cv else None
    sb = _hot_bcs(case)
    bcs, ic, _ = reference_bcs(cfg, stack, mesh)
    nsteps, picard = 10, 2
    prob = problem(case, bcs, precond, scheme=scheme, picard=picard, kappa_tables=kt, **({"rhoc_tables": ct} if ct else {}))
    try:
        u_ss, _, _ = prob.solve_steady(sb, picard_tol=PICARD_TOL)
        F = prob.hold_load()
        dofs, owner, pos = merge_bcs(bcs)
        assert np.array_equal(dofs, prob.bc_dofs)
        for bc in bcs:
            bc.update(0.0)
        g_all = []
        for k in range(nsteps):                    # the p-side line: its held value plus the pulse's rise above ic_temp
            bcs[3].update((k + 1) * prob.dt)
            g = gather_bc_values(bcs, owner, pos).copy()
            g[np.asarray(owner) == 3] += 400.0
            g_all.append(g)
        fields = []
        for g in g_all:
            prob.backend.step(g, prob.rtol, prob.atol, prob.max_it)
            fields.append(prob.state())
    finally:
        prob.close()
    ref = loaded_fields(mesh.coords, mesh.tris, mesh.tags, tk, trc, prob.dt, dofs, u_ss, g_all, F, ct, kt,
                        BDF2 if scheme == "bdf2" else BE, picard)
    worst = max(float(np.abs(f - r).max()) for f, r in zip(fields, ref))
    print(f"pulse from the held state precond={precond} {scheme} cv={with_cv}: worst |dT| = {worst:.2e} K, "
          f"the pulse moves the field by {np.abs(ref[-1] - u_ss).max():.3g} K")
    for k in range(nsteps):
        assert np.abs(fields[k] - ref[k]).max() <= 1e-4, f"step {k}: {np.abs(fields[k] - ref[k]).max():.3e} K"
    assert np.abs(ref[-1] - u_ss).max() > 0.1


# 5. degenerate cases, bit for bit -----------------------------------------------------------------------------------------------
def test_no_tables_and_constant_tables_give_the_linear_stiffness_and_solve_bitwise(hip, small_cases):
    case = small_cases["with_diamond_small"]
    cfg, stack, mesh = case
    tk, _ = material_tables(stack, mesh)
    sb = _hot_bcs(case)
    dofs, g = _steady_set(sb)
    rng = np.random.default_rng(11)
    u_any = 250.0 + 700.0 * rng.random(len(mesh.coords))
    const = {t: (300.0, 10.0, [tk[t]] * 51) for t in _ins_tags(stack, mesh)}
    ic = float(cfg["heating"]["ic_temp"])

    prob = problem(case, sb[:3], 0)
    try:
        be = prob.backend
        be.set_state(u_any)
        be.steady_setup(dofs, 0)
        be.hold_load()
        F_lin = be.get_load()
        be.set_load(None)
        be.set_state(np.full(prob.n, ic))
        be.steady_solve(g, False, STEADY_RTOL, 0.0, STEADY_MAX_IT)
        u_lin = be.get_state()
        # the Picard entry points with no table set, on the same context
        be.set_state(u_any)
        be.steady_picard_setup(dofs, 0)
        be.hold_load()
        assert np.array_equal(be.get_load(), F_lin)
        be.set_load(None)
        be.set_state(np.full(prob.n, ic))
        info = be.steady_picard_solve(g, False, STEADY_RTOL, 0.0, STEADY_MAX_IT, PICARD_TOL, 50)
        assert info["sweeps"] == 2 and info["iters"][1] == 0 and info["change"] == 0.0, info
        assert np.array_equal(be.get_state(), u_lin)
    finally:
        prob.close()

    prob = problem(case, sb[:3], 0, kappa_tables=const)
    try:
        be = prob.backend
        be.set_state(u_any)
        be.steady_picard_setup(dofs, 0)
        be.hold_load()
        assert np.array_equal(be.get_load(), F_lin)
        be.set_load(None)
        be.set_state(np.full(prob.n, ic))
        info = be.steady_picard_solve(g, False, STEADY_RTOL, 0.0, STEADY_MAX_IT, PICARD_TOL, 50)
        assert info["sweeps"] == 2 and info["iters"][1] == 0 and info["change"] == 0.0, info
        assert np.array_equal(be.get_state(), u_lin)
    finally:
        prob.close()
    assert np.abs(F_lin).max() > 0.0 and u_lin.max() > ic + 399.0


# 6. refusals ------------------------------------------------------------------------------------------------------------------------
def test_error_returns_and_staleness(hip, small_cases):
    case = small_cases["with_diamond_small"]
    cfg, stack, mesh = case
    tk, trc = material_tables(stack, mesh)
    tables = _ins_tables(stack, mesh, tk)
    sb = _hot_bcs(case)
    dofs, g = _steady_set(sb)
    pd = ctypes.POINTER(ctypes.c_double)
    gp = g.ctypes.data_as(pd)
    prob = problem(case, sb[:3], 0, kappa_tables=tables)
    be = prob.backend

    def solve(gptr=gp, rtol=1e-10, atol=0.0, max_it=100, tol=1e-6, sweeps=5):
        return be._lib.hf_steady_picard_solve(be._ctx, gptr, 0, rtol, atol, max_it, tol, sweeps, None, None, None, None)

    try:
        u0 = prob.state()
        assert solve() == hip.HF_ERR_STATE                                  # before the set-up
        with pytest.raises(ValueError, match="hf_steady_picard_setup: empty"):
            be.steady_picard_setup(np.zeros(0, dtype=np.int32))
        with pytest.raises(ValueError, match="hf_steady_picard_setup: unknown preconditioner"):
            be.steady_picard_setup(dofs, 2)
        with pytest.raises(ValueError, match="listed twice"):
            be.steady_picard_setup(np.concatenate([dofs, dofs[:1]]), 0)
        with pytest.raises(ValueError, match="outside"):
            be.steady_picard_setup(np.array([prob.n], dtype=np.int32), 0)
        with pytest.raises(hip.HipError, match=r"kappa\(T\) tables are set \(a Picard steady state is not supported\)") as e:
            be.steady_setup(dofs, 0)                                        # the linear entry points keep refusing
        assert e.value.code == hip.HF_ERR_STATE
        be.steady_picard_setup(dofs, 0)
        assert be._lib.hf_steady_solve(be._ctx, gp, 0, 1e-10, 0.0, 100, None, None) == hip.HF_ERR_STATE
        for bad in (dict(gptr=None), dict(rtol=-1.0), dict(atol=-1.0), dict(max_it=0), dict(tol=-1e-9), dict(tol=float("nan")),
                    dict(sweeps=0), dict(sweeps=1001)):
            assert solve(**bad) == hip.HF_ERR_ARG, bad
        assert np.array_equal(prob.state(), u0)                             # nothing ran
        # every change of the tables or the materials makes the set-up stale
        tags = np.array(sorted(tk), dtype=np.int32)
        for change in (lambda: be.set_kappa_tables(tables, 1), lambda: be.set_rhoc_tables(_cv_tables(stack, mesh, trc)),
                       lambda: be.set_rhoc_tables({}),
                       lambda: be.set_materials(tags, np.array([tk[t] for t in tags]), np.array([trc[t] for t in tags]))):
            be.steady_picard_setup(dofs, 0)
            change()
            assert solve() == hip.HF_ERR_STATE
            with pytest.raises(hip.HipError) as e:
                be.hold_load()
            assert e.value.code == hip.HF_ERR_STATE
        be.steady_picard_setup(dofs, 0)
        be.set_kappa_tables({}, 1)                                          # clearing as well
        assert solve() == hip.HF_ERR_STATE
        assert np.array_equal(prob.state(), u0)
        # capacity tables alone: the set-up and the solve work, K is the constant-coefficient one
        be.set_rhoc_tables(_cv_tables(stack, mesh, trc))
        be.steady_picard_setup(dofs, 0)
        info = be.steady_picard_solve(g, False, STEADY_RTOL, 0.0, STEADY_MAX_IT, PICARD_TOL, 5)
        assert info["sweeps"] == 2 and info["change"] == 0.0
        # max_sweeps run out: HF_ERR_NOCONV with every output filled
        be.set_kappa_tables(tables, 1)
        be.set_state(u0)
        be.steady_picard_setup(dofs, 0)
        with pytest.raises(hip.NotConverged):
            be.steady_picard_solve(g, False, STEADY_RTOL, 0.0, STEADY_MAX_IT, PICARD_TOL, 2)
        last = be.last_picard
        assert last["sweeps"] == 2 and len(last["iters"]) == 2 and last["change"] > PICARD_TOL and last["nl_resid"] > 0.0
    finally:
        prob.close()


# 7. 1.04 M DOF, multigrid ------------------------------------------------------------------------------------------------------------
def test_one_million_dof_with_multigrid(hip):
    case = build_case("geballe_with_diamond", 0.43)
    cfg, stack, mesh = case
    assert len(mesh.coords) > 1_000_000
    tk, _ = material_tables(stack, mesh)
    tables = _ins_tables(stack, mesh, tk)
    sb = _hot_bcs(case)
    prob = problem(case, sb[:3], 1, kappa_tables=tables)
    try:
        u_ss, it, res = prob.solve_steady(sb, picard_tol=1e-6, max_sweeps=30)
        info = prob.steady_info
        F = prob.hold_load()
        B = np.asarray(prob.bc_dofs)
        worst = 0.0
        for k in range(5):
            prob.step((k + 1) * prob.dt)
            worst = max(worst, float(np.abs(prob.state() - u_ss).max()))
            assert worst <= 1e-5, f"step {k}: {worst:.3e} K"
        fallbacks = prob.backend.amg_info()["jacobi_fallbacks"]
    finally:
        prob.close()
    print(f"1.04 M DOF: {info['sweeps']} sweeps, PCG iterations {info['iters']}, change {info['change']:.2e} K, "
          f"nl_resid {info['nl_resid']:.2e}, drift {worst:.2e} K, fallbacks {fallbacks}")
    assert info["sweeps"] <= 30 and info["change"] <= 1e-6
    assert fallbacks == 0
    assert u_ss.max() - u_ss.min() > 399.0
    rel = _check_hold_load(mesh, tk, tables, u_ss, F, B)
    print(f"1.04 M DOF: worst |F - K(u) u| / (|K| |u|) = {rel:.2e}")
