"""Steady state and pre-heated transients (with_ir_steady.ipynb cells 17-23) without a GPU: the C ABI declares and
exports the new entry points, and HeatProblem's solve_steady / set_load / hold_load drive a backend the way the
notebook's sequence needs - checked against an oracle-backed backend that restates K, the steady solve, the hold load
and the loaded time step with scipy."""
import numpy as np
import pytest
import scipy.sparse.linalg as spla

from helpers import material_tables, reference_bcs
from oracle import heat_oracle as ho
from oracle_backend import OracleBackend
from test_cabi import _declared_symbols

NEW_ENTRY_POINTS = ("hf_steady_setup", "hf_steady_solve", "hf_set_load", "hf_hold_load", "hf_get_load")


class SteadyOracleBackend(OracleBackend):
    """OracleBackend plus the steady entry points: K = element_matrices(...)[1] assembled (the dt K part of the transient
    operator at dt = 1), its own Dirichlet set eliminated symmetrically, b = M u^n + dt F in the time step."""

    load = None
    steady_setups = 0

    def _stiffness(self):
        kappa, rho_c = ho.cell_coefficients(self.tags, self.tag_to_k, self.tag_to_rc)
        return ho.assemble_csr(self.n, self.tris, ho.element_matrices(self.coords, self.tris, rho_c, kappa)[1])

    def steady_setup(self, dofs, precond=0):
        dofs = np.asarray(dofs, dtype=np.int64)
        if len(dofs) == 0:
            raise ValueError("empty steady Dirichlet set")
        self.K = self._stiffness()
        self.steady_dofs = dofs
        self._s_lift = self.K[:, dofs].tocsr()
        self._s_lu = spla.splu(ho.eliminate_dirichlet(self.K, dofs).tocsc())
        self.steady_setups += 1

    def steady_solve(self, g, use_load=False, rtol=1e-10, atol=0.0, max_it=20000):
        g = np.asarray(g, dtype=np.float64)
        b = (self.load.copy() if (use_load and self.load is not None) else np.zeros(self.n)) - self._s_lift @ g
        b[self.steady_dofs] = g
        self.u = self._s_lu.solve(b)
        return 1, 0.0

    def set_load(self, F):
        self.load = None if F is None else np.array(F, dtype=np.float64)

    def hold_load(self):
        F = self.K @ self.u
        F[self.bc_dofs] = 0.0
        self.load = F

    def get_load(self):
        return self.load.copy()

    def step(self, g, rtol=1e-10, atol=0.0, max_it=20000):
        b = self.M @ self.u
        if self.load is not None:
            b += self._dt * self.load
        if self.n_bc:
            b -= self.A_lift @ g
            b[self.bc_dofs] = g
        self.u = self._lu.solve(b)
        return 1, 0.0


def steady_bcs(cfg, stack, mesh, p_value, o_value=None):
    """Outer boundary at ic_temp and the heated line(s) at constant amplitudes (the notebook's steady_pside_bc /
    steady_oside_bc): [left, right, top, p-side line (, o-side line)]."""
    from heatflow_amd.bc import P1Space, RowDirichletBC

    ic = float(cfg["heating"]["ic_temp"])
    V = P1Space(mesh.coords)
    line = dict(length=abs(stack.r_sample) * 2, center=0.0)
    bcs = [RowDirichletBC(V, "left", value=ic), RowDirichletBC(V, "right", value=ic), RowDirichletBC(V, "top", value=ic),
           RowDirichletBC(V, "x", coord=stack.heated_z, value=p_value, **line)]
    if o_value is not None:
        bcs.append(RowDirichletBC(V, "x", coord=stack.heated_z_oside, value=o_value, **line))
    return bcs


def oracle_problem(cfg, stack, mesh, bcs):
    from heatflow_amd.solver import HeatProblem

    tag_to_k, tag_to_rc = material_tables(stack, mesh)
    dt = float(cfg["timing"]["t_final"]) / int(cfg["timing"]["num_steps"])
    return HeatProblem(mesh.coords, mesh.tris, mesh.tags, tag_to_k, tag_to_rc, dt, bcs, float(cfg["heating"]["ic_temp"]),
                       backend=SteadyOracleBackend())


def test_header_declares_and_library_exports_the_steady_entry_points():
    from heatflow_amd import hip_backend

    declared = _declared_symbols()
    lib = hip_backend.load_library()
    for name in NEW_ENTRY_POINTS:
        assert name in declared, name
        assert name in hip_backend.EXPORTS, name
        assert hasattr(lib, name), name


def test_steady_bc_merge_is_last_wins(case_with_diamond_small):
    from heatflow_amd.bc import P1Space, RowDirichletBC

    cfg, stack, mesh = case_with_diamond_small
    ic = float(cfg["heating"]["ic_temp"])
    bcs = steady_bcs(cfg, stack, mesh, ic + 7.0)
    prob = oracle_problem(cfg, stack, mesh, bcs[:3])
    hot_left = RowDirichletBC(P1Space(mesh.coords), "left", value=ic + 3.0)
    left, top, line = bcs[0].row_dofs, bcs[2].row_dofs, bcs[3].row_dofs
    corner = np.intersect1d(left, top)
    assert corner.size > 0
    u, _, _ = prob.solve_steady(bcs + [hot_left])            # the later left BC wins on the left rows, the corner included
    assert np.allclose(u[left], ic + 3.0) and np.allclose(u[line], ic + 7.0)
    assert np.allclose(u[np.setdiff1d(top, left)], ic)
    u2, _, _ = prob.solve_steady([hot_left] + bcs)           # listed first: the outer boundary at ic_temp wins
    assert np.allclose(u2[left], ic) and np.allclose(u2[line], ic + 7.0)
    u3, _, _ = prob.solve_steady([hot_left, bcs[3], bcs[1], bcs[0], bcs[2]])   # top after left: the corner goes to top
    assert np.allclose(u3[corner], ic)
    # the problem's own transient set is untouched
    assert np.array_equal(prob.backend.bc_dofs, prob.bc_dofs)
    assert not np.isin(line, prob.bc_dofs).any()


def test_hold_load_zeroes_exactly_the_merged_transient_dirichlet_rows(case_with_diamond_small):
    cfg, stack, mesh = case_with_diamond_small
    ic = float(cfg["heating"]["ic_temp"])
    bcs_t, _, _ = reference_bcs(cfg, stack, mesh)
    prob = oracle_problem(cfg, stack, mesh, bcs_t)
    u_ss, _, _ = prob.solve_steady(steady_bcs(cfg, stack, mesh, ic + 5.0, ic + 2.0))
    F = prob.hold_load()
    B = np.asarray(prob.bc_dofs)
    assert np.array_equal(B, np.unique(np.concatenate([b.row_dofs for b in bcs_t])))
    assert np.all(F[B] == 0.0)
    free = np.setdiff1d(np.arange(prob.n), B)
    assert np.allclose(F[free], (prob.backend.K @ u_ss)[free])
    # the rows of the steady set that are free in the transient carry the heat the held lines supply
    o_line = steady_bcs(cfg, stack, mesh, ic + 5.0, ic + 2.0)[4].row_dofs
    assert np.abs(F[np.setdiff1d(o_line, B)]).max() > 0.0
    prob.set_load(None)
    assert prob.backend.load is None


def test_steady_hold_transient_sequence_leaves_the_steady_state_in_place(case_with_diamond_small):
    """Notebook cells 17, 18, 22: steady state with both lines held, the transient with the outer boundary only plus the
    hold load stays at u_ss."""
    cfg, stack, mesh = case_with_diamond_small
    ic = float(cfg["heating"]["ic_temp"])
    sb = steady_bcs(cfg, stack, mesh, ic + 5.0, ic + 2.0)
    prob = oracle_problem(cfg, stack, mesh, sb[:3])
    u_ss, _, _ = prob.solve_steady(sb)
    assert u_ss.max() > ic + 4.9 and u_ss.min() >= ic - 1e-9
    prob.hold_load()
    for k in range(5):
        prob.step((k + 1) * prob.dt)
        assert np.abs(prob.state() - u_ss).max() <= 1e-8
    # without the load the held lines cool down
    prob.set_load(None)
    prob.step(6 * prob.dt)
    assert np.abs(prob.state() - u_ss).max() > 1e-3


def test_solve_steady_refuses_an_empty_set(case_with_diamond_small):
    cfg, stack, mesh = case_with_diamond_small
    prob = oracle_problem(cfg, stack, mesh, [])
    with pytest.raises(ValueError):
        prob.solve_steady()
