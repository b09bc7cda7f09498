"""Tables on anisotropic materials (hf_set_aniso_tables) restated for the CPU and GPU tests.  TEST CODE: never
imported by heatflow_amd.

A cell tag keeps its multipliers (m_r, m_z); its scalar conductivity is table_tag(T_e) where the tag has a table, else its
constant, so k_r = m_r kappa(T_e) and k_z = m_z kappa(T_e); rho_c(T_e) is untouched by the multipliers.  The restatement composes
what the tests already have, each extended by the multipliers ``aniso`` = {cell tag: (m_r, m_z)}:
    kappa_T_oracle.element_kappa / table_eval          the coefficients at T_e
    aniso_oracle.element_matrices_aniso                the element
    loops_oracle.table_loop (rhoc_t_fields' loop)      lagged and picard > 1 sweeps, both schemes
    loops_oracle.picard_loop (picard_steady's loop)    the Picard steady state
With multipliers 1 or absent the operators are rhoc_T_oracle.operators' bit for bit, without tables aniso_oracle.operator's.
"""
import numpy as np

from aniso_oracle import cell_multipliers, element_matrices_aniso
from kappa_T_oracle import BDF2, BE, element_kappa
from loops_oracle import picard_loop, table_loop
from oracle import heat_oracle as ho

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
    def operators_at(dtp, x):
        return operators(coords, tris, tags, tag_to_k, tag_to_rc, dtp, x, kappa_tables, rhoc_tables, aniso)[:2]
    return table_loop(operators_at, dt, bc_dofs, u0, g_all, scheme, picard)


def picard_steady(coords, tris, tags, tag_to_k, dofs, g, x0, kappa_tables=None, aniso=None, F=None, picard_tol=1e-6, max_sweeps=50):
    """steady_picard_oracle.picard_steady with the multipliers.  Returns {"u", "changes", "sweeps", "converged", "nl_resid", "K"}."""
    return picard_loop(lambda x: stiffness(coords, tris, tags, tag_to_k, x, kappa_tables, aniso), dofs, g, x0, F, picard_tol, max_sweeps)


def scaled_tables(tables, s):
    """Every table value divided by s: the tables of the isotropic twin of aniso_oracle.stretched(..., s)."""
    return {t: (T0, dT, np.asarray(v, dtype=np.float64) / s) for t, (T0, dT, v) in (tables or {}).items()}
