"""Tables on anisotropic materials (hf_set_aniso_tables) restated for the CPU and GPU tests.  TEST CODE: never
imported by heatflow_amd.

A cell tag keeps its multipliers (m_r, m_z); its scalar conductivity is table_tag(T_e) where the tag has a table, else its
constant, so k_r = m_r kappa(T_e) and k_z = m_z kappa(T_e); rho_c(T_e) is untouched by the multipliers.  The restatement composes
what the tests already have, each extended by the multipliers ``aniso`` = {cell tag: (m_r, m_z)}:
    kappa_T_oracle.element_kappa / table_eval          the coefficients at T_e
    aniso_oracle.element_matrices_aniso                the element
    the loops of rhoc_T_oracle.rhoc_t_fields           lagged and picard > 1 sweeps, both schemes
    steady_picard_oracle.picard_steady                 the Picard steady state
With multipliers 1 or absent the operators are rhoc_T_oracle.operators' bit for bit, without tables aniso_oracle.operator's.
"""
import numpy as np
import scipy.sparse.linalg as spla

from aniso_oracle import cell_multipliers, element_matrices_aniso
from kappa_T_oracle import BDF2, BE, element_kappa
from oracle import heat_oracle as ho
from steady_picard_oracle import _system, nl_residual

__all__ = ["BE", "BDF2", "operators", "stiffness", "aniso_t_fields", "picard_steady", "scaled_tables"]


def operators(coords, tris, tags, tag_to_k, tag_to_rc, dtp, x, kappa_tables=None, rhoc_tables=None, aniso=None):
    """(M, A, K) = (M(rho_c(x)), M + dtp K(kappa(x) diag(m_z, m_r)) summed per element, K) at the state x, not eliminated."""
    coords = np.asarray(coords, dtype=np.float64)
    tris = np.asarray(tris, dtype=np.int64)
    kappa = element_kappa(x, tris, tags, tag_to_k, kappa_tables or {})
    rho_c = element_kappa(x, tris, tags, tag_to_rc, rhoc_tables or {})
    m_r, m_z = cell_multipliers(tags, aniso)
    Me, Ke = element_matrices_aniso(coords, tris, rho_c, kappa, m_r, m_z)
    n = len(coords)
    return ho.assemble_csr(n, tris, Me), ho.assemble_csr(n, tris, Me + dtp * Ke), ho.assemble_csr(n, tris, Ke)


def stiffness(coords, tris, tags, tag_to_k, x, kappa_tables=None, aniso=None):
    """K(x) alone: steady_picard_oracle.stiffness with the multipliers."""
    coords = np.asarray(coords, dtype=np.float64)
    tris = np.asarray(tris, dtype=np.int64)
    kappa = element_kappa(x, tris, tags, tag_to_k, kappa_tables or {})
    m_r, m_z = cell_multipliers(tags, aniso)
    Ke = element_matrices_aniso(coords, tris, np.ones(len(tris)), kappa, m_r, m_z)[1]
    return ho.assemble_csr(len(coords), tris, Ke)


def aniso_t_fields(coords, tris, tags, tag_to_k, tag_to_rc, dt, bc_dofs, u0, g_all, rhoc_tables=None, kappa_tables=None,
                   aniso=None, scheme=BE, picard=1):
    """Every step's field (n_steps x n) and the Picard change of every step: the loop of rhoc_T_oracle.rhoc_t_fields on the
    operators above."""
    bc_dofs = np.asarray(bc_dofs, dtype=np.int64)
    dtp = 2.0 * dt / 3.0 if scheme == BDF2 else float(dt)
    u = np.array(u0, dtype=np.float64)
    up = None
    fields, changes = [], []
    for g in np.asarray(g_all, dtype=np.float64):
        if scheme == BDF2:
            um1 = u if up is None else up
            w = (4.0 * u - um1) / 3.0
            x = u.copy() if up is None else 2.0 * u - up
        else:
            w = u
            x = u.copy()
        change = 0.0
        for _ in range(int(picard)):
            M, A, _ = operators(coords, tris, tags, tag_to_k, tag_to_rc, dtp, x, kappa_tables, rhoc_tables, aniso)
            b = M @ w
            if len(bc_dofs):
                b -= A[:, bc_dofs].tocsr() @ g
                b[bc_dofs] = g
                A = ho.eliminate_dirichlet(A, bc_dofs)
            xn = spla.splu(A.tocsc()).solve(b)
            change = float(np.abs(xn - x).max())
            x = xn
        up, u = u, x
        fields.append(u.copy())
        changes.append(change)
    return np.array(fields), np.array(changes)


def picard_steady(coords, tris, tags, tag_to_k, dofs, g, x0, kappa_tables=None, aniso=None, F=None, picard_tol=1e-6, max_sweeps=50):
    """steady_picard_oracle.picard_steady with the multipliers.  Returns {"u", "changes", "sweeps", "converged", "nl_resid", "K"}."""
    dofs = np.asarray(dofs, dtype=np.int64)
    g = np.asarray(g, dtype=np.float64)
    x = np.array(x0, dtype=np.float64)
    changes = []
    for _ in range(int(max_sweeps)):
        Khat, b = _system(stiffness(coords, tris, tags, tag_to_k, x, kappa_tables, aniso), dofs, g, F)
        xn = spla.splu(Khat.tocsc()).solve(b)
        xn[dofs] = g
        changes.append(float(np.abs(xn - x).max()))
        x = xn
        if changes[-1] <= picard_tol:
            break
    K = stiffness(coords, tris, tags, tag_to_k, x, kappa_tables, aniso)
    return {"u": x, "changes": changes, "sweeps": len(changes), "converged": changes[-1] <= picard_tol,
            "nl_resid": nl_residual(K, dofs, g, x, F), "K": K}


def scaled_tables(tables, s):
    """Every table value divided by s: the tables of the isotropic twin of aniso_oracle.stretched(..., s)."""
    return {t: (T0, dT, np.asarray(v, dtype=np.float64) / s) for t, (T0, dT, v) in (tables or {}).items()}
