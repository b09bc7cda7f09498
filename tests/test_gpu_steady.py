"""Steady state and pre-heated transients on the GPU (with_ir_steady.ipynb cells 17-23) against restatements of the
same mathematics with scipy: K = element_matrices(...)[1] assembled, its own Dirichlet set eliminated symmetrically, the
hold load (K u)_i off the transient's Dirichlet rows, and the time step b = M u^n + dt F."""
import numpy as np
import pytest
import scipy.sparse.linalg as spla

from conftest import build_case
from helpers import material_tables, reference_bcs
from heatflow_amd.solver import DEFAULT_RTOL
from oracle import heat_oracle as ho
from test_steady_cpu import steady_bcs

pytestmark = pytest.mark.gpu

STEADY_MAX_IT = 400000     # Jacobi-PCG on the stiffness alone needs far more iterations than on M + dt K
STEADY_RTOL = 1e-12


@pytest.fixture(scope="module")
def c2():
    return build_case("geballe_no_diamond", 1.0)


@pytest.fixture(scope="module")
def c3():
    return build_case("geballe_with_diamond", 0.43)


def problem(case, bcs, precond, **kw):
    from heatflow_amd.solver import HeatProblem

    cfg, stack, mesh = case
    tag_to_k, tag_to_rc = material_tables(stack, mesh)
    dt = float(cfg["timing"]["t_final"]) / int(cfg["timing"]["num_steps"])
    kw.setdefault("max_it", STEADY_MAX_IT)
    return HeatProblem(mesh.coords, mesh.tris, mesh.tags, tag_to_k, tag_to_rc, dt, bcs, float(cfg["heating"]["ic_temp"]),
                       precond=precond, **kw)


def stiffness(case):
    cfg, stack, mesh = case
    tag_to_k, tag_to_rc = material_tables(stack, mesh)
    kappa, rho_c = ho.cell_coefficients(mesh.tags, tag_to_k, tag_to_rc)
    Me, Ke = ho.element_matrices(mesh.coords, mesh.tris, rho_c, kappa)
    n = len(mesh.coords)
    return ho.assemble_csr(n, mesh.tris, Ke), ho.assemble_csr(n, mesh.tris, Me)


def restated_steady(K, dofs, g, F=None):
    """K_hat_S u = F - K[:, S] g_S on the free rows, u_S = g_S (scipy direct solve)."""
    b = (np.zeros(K.shape[0]) if F is None else np.array(F, dtype=np.float64)) - K[:, dofs] @ g
    b[dofs] = g
    return spla.spsolve(ho.eliminate_dirichlet(K, dofs).tocsc(), b)


class LoadedOracle(ho.OracleSolver):
    """The reference loop with the load term: b = M u^n + dt F, lifting, set_bc (boundary values given per step)."""

    def __init__(self, case, bc_dofs_list, u0, F):
        cfg, stack, mesh = case
        tag_to_k, tag_to_rc = material_tables(stack, mesh)
        dt = float(cfg["timing"]["t_final"]) / int(cfg["timing"]["num_steps"])
        super().__init__(mesh.coords, mesh.tris, mesh.tags, tag_to_k, tag_to_rc, dt,
                         [{"dofs": d, "value": 0.0} for d in bc_dofs_list], u0)
        self.F = np.zeros(len(self.u)) if F is None else np.asarray(F, dtype=np.float64)

    def step_g(self, g):
        b = self.M @ self.u + self.dt * self.F
        b -= self.A_lift @ g
        b[self.bc_dofs] = g
        self.u = self.factor().solve(b)
        return self.u


def hold_load_restated(K, u, B):
    F = K @ u
    F[B] = 0.0
    return F


def two_line_steady(case):
    cfg = case[0]
    ic = float(cfg["heating"]["ic_temp"])
    return steady_bcs(cfg, case[1], case[2], ic + 5.0, ic + 2.0)


# 1. steady parity -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precond", [0, 1])
@pytest.mark.parametrize("which", ["with_diamond_small", "no_diamond_small", "c2"])
def test_steady_state_matches_a_direct_solve(hip, request, which, precond):
    case = request.getfixturevalue({"with_diamond_small": "case_with_diamond_small", "no_diamond_small": "case_no_diamond_small",
                                    "c2": "c2"}[which])
    cfg = case[0]
    ic = float(cfg["heating"]["ic_temp"])
    sb = steady_bcs(cfg, case[1], case[2], ic + 5.0)
    prob = problem(case, sb[:3], precond, rtol=STEADY_RTOL)
    try:
        u, it, res = prob.solve_steady(sb)
        from heatflow_amd.bc import gather_bc_values, merge_bcs

        dofs, owner, pos = merge_bcs(sb)
        ref = restated_steady(stiffness(case)[0], dofs, gather_bc_values(sb, owner, pos))
        err = float(np.abs(u - ref).max())
        print(f"steady {which} precond={precond}: {it} iterations, max |u - u_direct| = {err:.2e} K")
        assert err <= 1e-4, f"{err:.3e} K"
        assert ref.max() > ic + 4.9 and np.array_equal(u[dofs], gather_bc_values(sb, owner, pos))
    finally:
        prob.close()


# 2. no drift (notebook cell 22) ---------------------------------------------------------------------------------------
def _no_drift(case, precond, nsteps=10):
    sb = two_line_steady(case)
    prob = problem(case, sb[:3], precond)
    try:
        u_ss, it, _ = prob.solve_steady(sb)
        prob.hold_load()
        worst = 0.0
        for k in range(nsteps):
            prob.step((k + 1) * prob.dt)
            worst = max(worst, float(np.abs(prob.state() - u_ss).max()))
            assert worst <= 1e-5, f"step {k}: {worst:.3e} K"
        return it, worst
    finally:
        prob.close()


@pytest.mark.parametrize("precond", [0, 1])
def test_hold_load_keeps_the_steady_state(hip, case_with_diamond_small, precond):
    it, worst = _no_drift(case_with_diamond_small, precond)
    print(f"no drift precond={precond}: steady solve {it} iterations, max drift {worst:.2e} K")


def test_hold_load_keeps_the_steady_state_at_one_million_dof(hip, c3):
    assert len(c3[2].coords) > 1_000_000
    it, worst = _no_drift(c3, 1)
    print(f"no drift C3 multigrid: steady solve {it} iterations, max drift {worst:.2e} K")


# 3. pulsed from steady (notebook cell 23) ------------------------------------------------------------------------------
@pytest.mark.parametrize("precond", [0, 1])
def test_pulsed_transient_from_the_steady_state_matches_the_oracle(hip, case_with_diamond_small, precond):
    case = case_with_diamond_small
    cfg, stack, mesh = case
    sb = two_line_steady(case)
    bcs, ic, _ = reference_bcs(cfg, stack, mesh)           # outer boundary + the Gaussian pulsed line
    K, _ = stiffness(case)
    nsteps = 8
    for path in ("step", "run"):
        prob = problem(case, bcs, precond)
        try:
            # on the rows free in both sets (K u_ss)_i is the steady solve's residual: solve it as tightly as the parity test
            prob.rtol = STEADY_RTOL
            u_ss, _, _ = prob.solve_steady(sb)
            prob.rtol = DEFAULT_RTOL
            F = prob.hold_load()
            B = np.asarray(prob.bc_dofs)
            from heatflow_amd.bc import gather_bc_values, merge_bcs

            sd, so, sp_ = merge_bcs(sb)
            u_ss_ref = restated_steady(K, sd, gather_bc_values(sb, so, sp_))
            F_ref = hold_load_restated(K, u_ss_ref, B)
            assert np.all(F[B] == 0.0)
            # the kernel: K_free u of the state it held, up to the rounding of each row's sum (scale |K| |u|: the sum cancels);
            # against the direct solve's hold load, in addition the steady solve's error carried through K
            Ka = abs(K)
            rounding = 64 * np.finfo(np.float64).eps * (Ka @ np.abs(u_ss))
            assert np.all(np.abs(F - hold_load_restated(K, u_ss, B)) <= rounding)
            assert np.abs(u_ss - u_ss_ref).max() <= 1e-6
            assert np.all(np.abs(F - F_ref) <= Ka @ np.abs(u_ss - u_ss_ref) + rounding)
            oracle = LoadedOracle(case, [b.row_dofs for b in bcs], u_ss_ref, F_ref)
            for bc in prob.bcs:
                bc.update(0.0)
            g_all = [prob.bc_values((k + 1) * prob.dt, [prob.bcs[3]]) for k in range(nsteps)]
            if path == "step":
                fields = []
                for k in range(nsteps):
                    prob.step((k + 1) * prob.dt, only=[prob.bcs[3]])
                    fields.append(prob.state())
            else:
                _, fields, _ = prob.run(nsteps, watcher_nodes=np.arange(prob.n), time_varying=[prob.bcs[3]])
            worst = 0.0
            for k in range(nsteps):
                ref = oracle.step_g(g_all[k])
                worst = max(worst, float(np.abs(fields[k] - ref).max()))
            print(f"pulsed from steady ({path}, precond={precond}): worst |dT| = {worst:.2e} K")
            assert worst <= 1e-4, f"{path}: {worst:.3e} K"
            assert np.abs(oracle.u - u_ss_ref).max() > 0.1     # the pulse moved the field away from u_ss
        finally:
            prob.close()


# 4. arbitrary uploaded load ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precond", [0, 1])
def test_random_load_matches_the_oracle(hip, case_with_diamond_small, precond):
    case = case_with_diamond_small
    cfg, stack, mesh = case
    bcs, ic, _ = reference_bcs(cfg, stack, mesh)
    _, M = stiffness(case)
    prob = problem(case, bcs, precond)
    try:
        rng = np.random.default_rng(20261015)
        F = rng.uniform(-1.0, 1.0, prob.n) * M.diagonal() * (2.0 / prob.dt)     # a few kelvin per step
        prob.set_load(F)
        oracle = LoadedOracle(case, [b.row_dofs for b in bcs], np.full(prob.n, ic), F)
        for bc in prob.bcs:
            bc.update(0.0)
        worst = 0.0
        for k in range(6):
            t = (k + 1) * prob.dt
            prob.step(t, only=[prob.bcs[3]])
            ref = oracle.step_g(prob.bc_values(t, []))
            worst = max(worst, float(np.abs(prob.state() - ref).max()))
        print(f"random load precond={precond}: worst |dT| = {worst:.2e} K")
        assert worst <= 1e-4, f"{worst:.3e} K"
        assert np.abs(oracle.u - ic).max() > 1.0
    finally:
        prob.close()


# 5. existing behaviour untouched, bit for bit ---------------------------------------------------------------------------
def _fields(prob, nsteps):
    for bc in prob.bcs:
        bc.update(0.0)
    out = []
    for k in range(nsteps):
        prob.step((k + 1) * prob.dt, only=[prob.bcs[3]])
        out.append(prob.state())
    return out


@pytest.mark.parametrize("amg_reuse", [False, True])
def test_transient_after_a_steady_solve_is_bitwise_the_fresh_one(hip, case_with_diamond_small, amg_reuse):
    case = case_with_diamond_small
    cfg, stack, mesh = case
    nsteps = 6
    runs = []
    for with_steady in (True, False):
        bcs, ic, _ = reference_bcs(cfg, stack, mesh)
        prob = problem(case, bcs, 1, amg_reuse=amg_reuse, max_it=20000)
        try:
            u0 = ic + 0.01 * (np.arange(prob.n) % 7)
            if with_steady:
                prob.solve_steady(two_line_steady(case))
            prob.set_state(u0)
            runs.append(_fields(prob, nsteps))
        finally:
            prob.close()
    for k in range(nsteps):
        assert np.array_equal(runs[0][k], runs[1][k]), f"step {k}"
    assert np.abs(runs[1][-1] - runs[1][0]).max() > 0.0


@pytest.mark.parametrize("precond", [0, 1])
def test_cleared_load_is_bitwise_no_load(hip, case_with_diamond_small, precond):
    case = case_with_diamond_small
    cfg, stack, mesh = case
    runs = []
    for had_load in (True, False):
        bcs, ic, _ = reference_bcs(cfg, stack, mesh)
        prob = problem(case, bcs, precond, max_it=20000)
        try:
            if had_load:
                prob.set_load(np.ones(prob.n))
                prob.set_load(None)
            runs.append(_fields(prob, 5))
        finally:
            prob.close()
    for k in range(5):
        assert np.array_equal(runs[0][k], runs[1][k]), f"step {k}"


# 6. error returns --------------------------------------------------------------------------------------------------------
def test_errors_empty_steady_set_and_batch_with_a_load(hip, case_with_diamond_small):
    case = case_with_diamond_small
    cfg, stack, mesh = case
    bcs, ic, _ = reference_bcs(cfg, stack, mesh)
    prob = problem(case, bcs, 0, max_it=20000)
    be = prob.backend
    try:
        with pytest.raises(ValueError, match="empty"):
            be.steady_setup(np.zeros(0, dtype=np.int32))      # HF_ERR_ARG: K alone is singular
        with pytest.raises(hip.HipError) as ei:
            be.hold_load()                # needs the stiffness of a steady set-up
        assert ei.value.code == hip.HF_ERR_STATE
        be.set_load(np.ones(prob.n))
        with pytest.raises(hip.HipError) as ei:
            be.batch_begin(2)
        assert ei.value.code == hip.HF_ERR_STATE
        be.set_load(None)
        be.batch_begin(2)                 # without the load the batch opens as before
        be.batch_end()
    finally:
        prob.close()
