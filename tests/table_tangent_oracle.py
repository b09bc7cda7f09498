"""Float64 restatement of tangent runs under kappa(T) / rho_c(T) tables, lagged scheme (hf_table_derivatives), for the
CPU and GPU tests.  TEST CODE: never imported by heatflow_amd.

Per step, with dt' the assembled step, u* and w as kappa_T_oracle / rhoc_T_oracle state them, s* formed from s^n, s^{n-1} exactly as u*
from u^n, u^{n-1}, T_e the element temperature of u* and sigma_e the mean of s* over the element's nodes:
    A(u*) s^{n+1} = M(u*) s_bar + dt' F_j - A[:, B] h^{n+1} (free rows),  (s)_B = h^{n+1}
    F_j = - K^1_j u^{n+1} - M^1_j w                                   (conductivity / capacity columns of untabled tags)
          - sum_{e in tabled tags} [ kdot_e (K^1_e u^{n+1})_i + cdot_e (M^1_e w)_i ]
    kdot_e = D^k_{j,tag}(T_e) + kappa'_tag(T_e) sigma_e,   cdot_e = D^c_{j,tag}(T_e) + rho_c'_tag(T_e) sigma_e
kappa' = the slope of the segment table_eval took, 0 in both clamped ranges; D a table on the tag's grid, evaluated by table_eval.
`mutate` switches one term off or wrong, for the floors the tests record.

FD_REL_STEP: the relative steps of the central differences that judge the recursion, found by the scan of
tests/test_table_tangent_cpu.py::test_fd_step_scan (printed there; 5 717-node mesh with diamond, 20 steps, 1/T conductivity tables
on both insulators - 11 knots to 400 K on the p side, so that its upper clamped range is reached, 51 knots to 800 K on the o side -
and 51-knot Einstein capacity tables on both).  Worst |s - FD| / max|s| in float64, backward Euler / BDF2:

    relative step   ins k table scale     p_ins exponent        ins cv table scale    p_sample.k
    1e-3            3.1e-5 / 9.1e-5       3.2e-9 / 4.5e-9       3.1e-5 / 9.1e-5       3.8e-7 / 4.0e-7
    1e-4 (chosen)   3.8e-9 / 4.1e-9       2.5e-9 / 2.1e-9       3.0e-9 / 3.1e-9       3.9e-9 / 3.9e-9
    1e-5            2.9e-8 / 1.4e-8       2.2e-8 / 2.1e-8       2.7e-8 / 2.2e-8       2.7e-8 / 3.1e-8
    1e-6            3.7e-7 / 2.7e-7       2.0e-7 / 1.4e-7       4.7e-7 / 2.4e-7       1.9e-7 / 3.2e-7

Larger steps run into the kinks of the piecewise-linear tables (an element whose T_e crosses a knot between the two runs), smaller
ones into the rounding of the direct solves.

Mutation floors on the same runs, |s_mutated - s| / max|s| of the three columns in parameters of tabled materials (k scale, exponent,
cv scale), backward Euler / BDF2 - the column in p_sample.k moves by 1e-5 at the most, which is why it is not judged:

    no_coupling       4.7e-2, 2.8e-2, 4.7e-2 / 5.3e-2, 3.8e-2, 5.3e-2
    sstar_lag         (identical under backward Euler) / 1.6e-2, 1.5e-2, 1.6e-2
    neighbour_slope   2.4e-3, 1.4e-3, 2.4e-3 / 3.0e-3, 2.1e-3, 3.0e-3
    clamped_slope     3.8e-3, 3.0e-3, 3.8e-3 / 4.3e-2, 4.0e-2, 4.3e-2
    no_Mw             1.9e-2, 9.8e-3, 1.0    / 2.3e-2, 1.5e-2, 1.0
"""
import numpy as np
import scipy.sparse.linalg as spla

from kappa_T_oracle import BDF2, BE, element_temperature, table_eval
from oracle import heat_oracle as ho
from rhoc_T_oracle import operators

__all__ = ["BE", "BDF2", "FD_REL_STEP", "MUTATIONS", "table_slope", "table_term", "tangent_fields", "primal_fields"]

FD_REL_STEP = {"k_table.scale": 1e-4, "k_power.exponent": 1e-4, "cv_table.scale": 1e-4, "k": 1e-4}
MUTATIONS = ("no_coupling", "sstar_lag", "neighbour_slope", "clamped_slope", "no_Mw")


def table_slope(T, T0, dT, values, mutate=None):
    """d table / dT, elementwise: (v_{i+1} - v_i) * (1/dT) of the segment table_eval takes (i = floor(s)), 0 where it clamps."""
    v = np.asarray(values, dtype=np.float64)
    n = len(v)
    inv = 1.0 / float(dT)
    s = (np.asarray(T, dtype=np.float64) - float(T0)) * inv
    i = np.clip(np.floor(np.where(np.isfinite(s), s, 0.0)).astype(np.int64), 0, n - 2)
    if mutate == "neighbour_slope":
        i = np.where(i + 1 <= n - 2, i + 1, i - 1) if n > 2 else i
    mid = (v[i + 1] - v[i]) * inv
    if mutate == "clamped_slope":
        return mid
    return np.where(~(s > 0.0) | (s >= n - 1), 0.0, mid)


def unit_rows(coords, tris):
    """(M^1_e, K^1_e): the element matrices at rho_c = 1 and kappa = 1, (n_e, 3, 3) each."""
    one = np.ones(len(tris))
    return ho.element_matrices(np.asarray(coords, dtype=np.float64), np.asarray(tris, dtype=np.int64), one, one)


def table_term(coords, tris, tags, kappa_tables, rhoc_tables, Dk, Dc, ncol, u_new, w, ustar, sstar, mutate=None, rows=None):
    """The tables' part of the load of every column, (n, ncol), and the sum of the magnitudes of its terms per row and column
    (what a row-by-row comparison is measured against).  Dk / Dc = {(column, tag): values}; sstar (n, ncol)."""
    tris = np.asarray(tris, dtype=np.int64)
    tags = np.asarray(tags)
    n = len(coords)
    Me1, Ke1 = rows if rows is not None else unit_rows(coords, tris)
    Te = element_temperature(ustar, tris)
    F = np.zeros((n, ncol))
    mag = np.zeros((n, ncol))
    sig = (sstar[tris[:, 0]] + sstar[tris[:, 1]] + sstar[tris[:, 2]]) / 3.0            # (n_e, ncol)
    for kind, (tables, D, El, vec) in enumerate(((kappa_tables or {}, Dk or {}, Ke1, u_new), (rhoc_tables or {}, Dc or {}, Me1, w))):
        if kind == 1 and mutate == "no_Mw":
            continue
        for tag, (T0, dT, vals) in tables.items():
            sel = np.flatnonzero(tags == int(tag))
            if not len(sel):
                continue
            rowv = np.einsum("eab,eb->ea", El[sel], vec[tris[sel]])                  # (K^1_e u)_a or (M^1_e w)_a
            rowm = np.einsum("eab,eb->ea", np.abs(El[sel]), np.abs(vec[tris[sel]]))
            slope = table_slope(Te[sel], T0, dT, vals, mutate)
            for j in range(ncol):
                dot = np.zeros(len(sel)) if mutate == "no_coupling" else slope * sig[sel, j]
                mdot = np.abs(dot)
                if (j, int(tag)) in D:
                    d = table_eval(Te[sel], T0, dT, D[(j, int(tag))])
                    dot = dot + d
                    mdot = mdot + np.abs(d)
                for a in range(3):
                    np.subtract.at(F[:, j], tris[sel, a], dot * rowv[:, a])
                    np.add.at(mag[:, j], tris[sel, a], mdot * rowm[:, a])
    return F, mag


def _tag_matrix(n, tris, tags, El, tag_list):
    sel = np.isin(np.asarray(tags), [int(t) for t in tag_list])
    return ho.assemble_csr(n, np.asarray(tris)[sel], El[sel])


def tangent_fields(coords, tris, tags, tag_to_k, tag_to_rc, dt, bc_dofs, u0, g_all, kappa_tables=None, rhoc_tables=None, scheme=BE,
                   ncol=1, conductivity=None, capacity=None, Dk=None, Dc=None, h_all=None, mutate=None):
    """(fields (n_steps, n), tangents (n_steps, ncol, n)) of the lagged loop and its exact tangent recursion.
    conductivity / capacity = {column: [untabled cell tags]}; Dk / Dc = {(column, tag): values}; h_all (n_steps, n_bc, ncol) or None."""
    coords = np.asarray(coords, dtype=np.float64)
    tris = np.asarray(tris, dtype=np.int64)
    bc_dofs = np.asarray(bc_dofs, dtype=np.int64)
    n = len(coords)
    dtp = 2.0 * dt / 3.0 if scheme == BDF2 else float(dt)
    rows = unit_rows(coords, tris)
    Kj = {j: _tag_matrix(n, tris, tags, rows[1], tl) for j, tl in (conductivity or {}).items()}
    Mj = {j: _tag_matrix(n, tris, tags, rows[0], tl) for j, tl in (capacity or {}).items()}
    u = np.array(u0, dtype=np.float64)
    up = None
    s = np.zeros((n, ncol))
    sp_ = None
    fields, tangents = [], []
    for k, g in enumerate(np.asarray(g_all, dtype=np.float64)):
        hist = scheme == BDF2 and up is not None
        if scheme == BDF2:
            ubar = (4.0 * u - (up if hist else u)) / 3.0
            sbar = (4.0 * s - (sp_ if hist else s)) / 3.0
        else:
            ubar, sbar = u, s
        ustar = 2.0 * u - up if hist else u.copy()
        sstar = 2.0 * s - sp_ if (hist and mutate != "sstar_lag") else s.copy()
        M, A = operators(coords, tris, tags, tag_to_k, tag_to_rc, dtp, ustar, kappa_tables, rhoc_tables)
        lift = A[:, bc_dofs].tocsr() if len(bc_dofs) else None
        Ahat = ho.eliminate_dirichlet(A, bc_dofs) if len(bc_dofs) else A
        lu = spla.splu(Ahat.tocsc())
        b = M @ ubar
        if len(bc_dofs):
            b -= lift @ g
            b[bc_dofs] = g
        un = lu.solve(b)
        w = (un - ubar) / dtp
        F, _ = table_term(coords, tris, tags, kappa_tables, rhoc_tables, Dk, Dc, ncol, un, w, ustar, sstar, mutate, rows)
        for j, K in Kj.items():
            F[:, j] -= K @ un
        for j, Mq in Mj.items():
            F[:, j] -= Mq @ w
        sn = np.empty_like(s)
        for j in range(ncol):
            bj = M @ sbar[:, j] + dtp * F[:, j]
            if len(bc_dofs):
                h = np.zeros(len(bc_dofs)) if h_all is None else np.asarray(h_all[k][:, j], dtype=np.float64)
                bj -= lift @ h
                bj[bc_dofs] = h
            sn[:, j] = lu.solve(bj)
        up, u = u, un
        sp_, s = s, sn
        fields.append(u.copy())
        tangents.append(s.T.copy())
    return np.array(fields), np.array(tangents)


def primal_fields(coords, tris, tags, tag_to_k, tag_to_rc, dt, bc_dofs, u0, g_all, kappa_tables=None, rhoc_tables=None, scheme=BE):
    """The primal loop alone (rhoc_T_oracle.rhoc_t_fields at one sweep), for the central differences."""
    from rhoc_T_oracle import rhoc_t_fields

    return rhoc_t_fields(coords, tris, tags, tag_to_k, tag_to_rc, dt, bc_dofs, u0, g_all, rhoc_tables, kappa_tables, scheme, 1)[0]
