"""kappa(T) restatement of the time loop (hf_set_kappa_tables) for the CPU and GPU tests of temperature-dependent
conductivities.  TEST CODE: never imported by heatflow_amd.

Per step:
    u*     = u^n (backward Euler), 2 u^n - u^{n-1} (BDF2 once a history exists, else u^n)
    T_e    = ((lo + mid) + hi) / 3 of the element's nodal values of the evaluation state, sorted by value
    kappa_e = table_tag(T_e) (piecewise linear on T0 + i dT, clamped) for a tabled tag, the constant otherwise
    A(x)   = M + dt' K(kappa(x)), eliminated, lifting columns A[:, B]; b0 = M u^n (BDF2: M (4/3 u^n - 1/3 u^{n-1}))
    sweep k = 1..p:  x_0 = u*,  A(x_{k-1}) x_k = b0 - A(x_{k-1})[:, B] g on the free rows, (x_k)_B = g
    u^{n+1} = x_p;  the Picard change = max |x_p - x_{p-1}|
built on oracle.heat_oracle's element matrices, assembly and elimination.
"""
import numpy as np

from loops_oracle import BDF2, BE, linear_loop, table_loop
from oracle import heat_oracle as ho


def table_eval(T, T0, dT, values):
    """kappa(T) of one table, elementwise: s = (T - T0) * (1/dT), clamped to the end values, else v_i + (s - i)(v_{i+1} - v_i)."""
    v = np.asarray(values, dtype=np.float64)
    n = len(v)
    s = (np.asarray(T, dtype=np.float64) - float(T0)) * (1.0 / float(dT))
    i = np.clip(np.floor(np.where(np.isfinite(s), s, 0.0)).astype(np.int64), 0, n - 2)
    mid = v[i] + (s - i.astype(np.float64)) * (v[i + 1] - v[i])
    return np.where(~(s > 0.0), v[0], np.where(s >= n - 1, v[n - 1], mid))


def element_temperature(u, tris):
    """T_e = ((lo + mid) + hi) * (1/3) of the three nodal values sorted by value."""
    v = np.sort(np.asarray(u, dtype=np.float64)[np.asarray(tris)], axis=1)
    return ((v[:, 0] + v[:, 1]) + v[:, 2]) * (1.0 / 3.0)


def element_kappa(u, tris, tags, tag_to_k, tables):
    """kappa_e of every element at the state u: table_tag(T_e) for a tabled tag, tag_to_k[tag] otherwise."""
    tags = np.asarray(tags)
    kappa = np.array([float(tag_to_k[int(t)]) for t in tags]) if len(tags) else np.zeros(0)
    if tables:
        Te = element_temperature(u, tris)
        for tag, (T0, dT, vals) in tables.items():
            sel = tags == int(tag)
            kappa[sel] = table_eval(Te[sel], T0, dT, vals)
    return kappa


class KappaTOperator:
    """M and the per-state A(u) = M + dtp K(kappa(u)) of one mesh (dtp = the assembled step: dt, or 2 dt / 3 under BDF2)."""

    def __init__(self, coords, tris, tags, tag_to_k, tag_to_rc, dtp, tables):
        self.coords = np.asarray(coords, dtype=np.float64)
        self.tris = np.asarray(tris, dtype=np.int64)
        self.tags = np.asarray(tags)
        self.tag_to_k, self.tables, self.dtp = dict(tag_to_k), dict(tables or {}), float(dtp)
        self.n = len(self.coords)
        _, rc = ho.cell_coefficients(self.tags, tag_to_k, tag_to_rc)
        self.rho_c = rc
        Me, _ = ho.element_matrices(self.coords, self.tris, rc, np.ones(len(self.tris)))
        self.Me = Me
        self.M = ho.assemble_csr(self.n, self.tris, Me)

    def A(self, u):
        kappa = element_kappa(u, self.tris, self.tags, self.tag_to_k, self.tables)
        _, Ke = ho.element_matrices(self.coords, self.tris, self.rho_c, kappa)
        return ho.assemble_csr(self.n, self.tris, self.Me + self.dtp * Ke)

    def eliminated(self, u, bc_dofs):
        """(A_hat, lifting columns A[:, B]) at the state u."""
        A = self.A(u)
        if len(bc_dofs) == 0:
            return A, None
        return ho.eliminate_dirichlet(A, bc_dofs), A[:, bc_dofs].tocsr()


def kappa_t_fields(coords, tris, tags, tag_to_k, tag_to_rc, dt, bc_dofs, u0, g_all, tables, scheme=BE, picard=1):
    """Every step's field of the kappa(T) loop (n_steps x n) and the Picard change of every step."""
    dtp = 2.0 * dt / 3.0 if scheme == BDF2 else float(dt)
    op = KappaTOperator(coords, tris, tags, tag_to_k, tag_to_rc, dtp, tables)   # M does not change: valued once
    return table_loop(lambda _, x: (op.M, op.A(x)), dt, bc_dofs, u0, g_all, scheme, picard)


def linear_fields(coords, tris, tags, tag_to_k, tag_to_rc, dt, bc_dofs, u0, g_all, scheme=BE):
    """The same loop with constant conductivities, through oracle.heat_oracle's operator (one factorisation)."""
    dtp = 2.0 * dt / 3.0 if scheme == BDF2 else float(dt)
    kappa, rc = ho.cell_coefficients(np.asarray(tags), tag_to_k, tag_to_rc)
    Me, Ke = ho.element_matrices(np.asarray(coords, dtype=np.float64), np.asarray(tris, dtype=np.int64), rc, kappa)
    n = len(coords)
    return linear_loop(ho.assemble_csr(n, tris, Me), ho.assemble_csr(n, tris, Me + dtp * Ke), bc_dofs, u0, g_all, scheme)


def problem_inputs(cfg, stack, mesh, num_steps):
    """(tag_to_k, tag_to_rc, dt, bc_dofs, u0, g_all) of the reference set-up of tests/helpers.py, the heated line's values
    tabulated for ``num_steps`` steps as HeatProblem.run tabulates them."""
    from helpers import material_tables, reference_bcs

    from heatflow_amd.bc import gather_bc_values, gather_plan, merge_bcs

    bcs, ic, _ = reference_bcs(cfg, stack, mesh)
    tag_to_k, tag_to_rc = material_tables(stack, mesh)
    dt = float(cfg["timing"]["t_final"]) / int(cfg["timing"]["num_steps"])
    dofs, owner, pos = merge_bcs(bcs)
    for bc in bcs:
        bc.update(0.0)
    plan = gather_plan(len(bcs), owner, pos)
    g_all = []
    for k in range(num_steps):
        bcs[3].update((k + 1) * dt)
        g_all.append(gather_bc_values(bcs, owner, pos, plan).copy())
    return tag_to_k, tag_to_rc, dt, np.asarray(dofs, dtype=np.int64), np.full(len(mesh.coords), ic), np.array(g_all)
