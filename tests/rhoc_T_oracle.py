"""cv(T) restatement of the time loop (hf_set_rhoc_tables) for the CPU and GPU tests of temperature-dependent heat
capacities.  TEST CODE: never imported by heatflow_amd.

Per step, with dt' the assembled step (dt, or 2 dt / 3 under BDF2):
    u*      = u^n (backward Euler), 2 u^n - u^{n-1} (BDF2 once a history exists, else u^n)
    w       = u^n (BDF2: (4 u^n - u^{n-1}) / 3, u^{n-1} = u^n without a history)
    T_e     = ((lo + mid) + hi) / 3 of the element's nodal values of the evaluation state, sorted by value
    rho_c_e = capacity table_tag(T_e), kappa_e = conductivity table_tag(T_e) for a tabled tag, the constants otherwise
    x_0 = u*;  sweep k = 1..p:  M_k = M(rho_c(x_{k-1})),  A_k = M_k + dt' K(kappa(x_{k-1})),
               A_k x_k = M_k w - A_k[:, B] g on the free rows,  (x_k)_B = g
    u^{n+1} = x_p;  the Picard change = max |x_p - x_{p-1}|
built on oracle.heat_oracle's element matrices, assembly and elimination and kappa_T_oracle's table evaluation.  With no
tables the loop is kappa_T_oracle.linear_fields', with conductivity tables only kappa_T_oracle.kappa_t_fields'.
"""
import numpy as np

from kappa_T_oracle import BDF2, BE, element_kappa
from loops_oracle import table_loop
from oracle import heat_oracle as ho

__all__ = ["BE", "BDF2", "einstein", "einstein_tables", "operators", "rhoc_t_fields"]


def einstein(T, theta):
    """E(theta / T), E(x) = x^2 e^x / (e^x - 1)^2."""
    x = theta / np.asarray(T, dtype=np.float64)
    return x * x * np.exp(x) / (np.exp(x) - 1.0) ** 2


def einstein_tables(tag_to_rc, tags, theta=600.0, T0=300.0, dT=10.0, knots=51):
    """{tag: (T0, dT, rho_c E(theta / T) / E(theta / T0))}: the tables of the issue (theta = 600 K, 300..800 K, 51 knots)."""
    T = T0 + dT * np.arange(knots)
    return {int(t): (T0, dT, tag_to_rc[int(t)] * einstein(T, theta) / einstein(T0, theta)) for t in tags}


def operators(coords, tris, tags, tag_to_k, tag_to_rc, dtp, x, kappa_tables=None, rhoc_tables=None):
    """(M, A) = (M(rho_c(x)), M + dtp K(kappa(x))) at the state x, not eliminated."""
    coords = np.asarray(coords, dtype=np.float64)
    tris = np.asarray(tris, dtype=np.int64)
    kappa = element_kappa(x, tris, tags, tag_to_k, kappa_tables or {})
    rho_c = element_kappa(x, tris, tags, tag_to_rc, rhoc_tables or {})
    Me, Ke = ho.element_matrices(coords, tris, rho_c, kappa)
    n = len(coords)
    return ho.assemble_csr(n, tris, Me), ho.assemble_csr(n, tris, Me + dtp * Ke)


def rhoc_t_fields(coords, tris, tags, tag_to_k, tag_to_rc, dt, bc_dofs, u0, g_all, rhoc_tables=None, kappa_tables=None,
                  scheme=BE, picard=1):
    """Every step's field of the loop (n_steps x n) and the Picard change of every step."""
    def operators_at(dtp, x):
        return operators(coords, tris, tags, tag_to_k, tag_to_rc, dtp, x, kappa_tables, rhoc_tables)
    return table_loop(operators_at, dt, bc_dofs, u0, g_all, scheme, picard)
