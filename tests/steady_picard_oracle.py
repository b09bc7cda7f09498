"""Restatement of the Picard steady state under kappa(T) tables (hf_steady_picard_setup / hf_steady_picard_solve) and of the
loaded time loop under kappa(T) / rho_c(T) tables, for the CPU and GPU tests.  TEST CODE: never imported by heatflow_amd.

Steady state, with K(x) = the r-weighted stiffness at kappa_e = table_tag(T_e(x)) (kappa_T_oracle.element_kappa):
    x_0 = the start state
    sweep k = 1, 2, ...:  K_hat_S(x_{k-1}) x_k = F - K(x_{k-1})[:, S] g_S on the free rows, (x_k)_S = g_S   (direct solve)
                          change_k = max |x_k - x_{k-1}|;  stop when change_k <= picard_tol
    K(u) at the returned state u = x_k;  nl_resid = ||D^-1 (b(u) - K_hat_S(u) u)||_2 / ||D^-1 b(u)||_2, D = diag K_hat_S(u),
    b(u) = F - K(u)[:, S] g_S, b_S = g_S
Loaded loop: rhoc_T_oracle.rhoc_t_fields with b = M_k w + dt' F in every sweep.
"""
import numpy as np

from kappa_T_oracle import BDF2, BE, element_kappa
from loops_oracle import nl_residual, picard_loop, table_loop
from oracle import heat_oracle as ho
from rhoc_T_oracle import operators

__all__ = ["BE", "BDF2", "stiffness", "nl_residual", "picard_steady", "loaded_fields", "rectangle_mesh"]


def stiffness(coords, tris, tags, tag_to_k, x, kappa_tables=None):
    """K(x): the r-weighted P1 stiffness with kappa_e = table_tag(T_e(x)) for a tabled tag, the constant otherwise."""
    coords = np.asarray(coords, dtype=np.float64)
    tris = np.asarray(tris, dtype=np.int64)
    kappa = element_kappa(x, tris, tags, tag_to_k, kappa_tables or {})
    Ke = ho.element_matrices(coords, tris, np.ones(len(tris)), kappa)[1]
    return ho.assemble_csr(len(coords), tris, Ke)


def picard_steady(coords, tris, tags, tag_to_k, dofs, g, x0, kappa_tables=None, F=None, picard_tol=1e-6, max_sweeps=50):
    """The loop above.  Returns {"u", "changes" (per sweep), "sweeps", "converged", "nl_resid", "K" (valued at u)}."""
    return picard_loop(lambda x: stiffness(coords, tris, tags, tag_to_k, x, kappa_tables), dofs, g, x0, F, picard_tol, max_sweeps)


def loaded_fields(coords, tris, tags, tag_to_k, tag_to_rc, dt, bc_dofs, u0, g_all, F, rhoc_tables=None, kappa_tables=None,
                  scheme=BE, picard=1):
    """Every step's field of the time loop under tables with the load term: sweep k solves
    A_k x_k = M_k w + dt' F - A_k[:, B] g on the free rows, (x_k)_B = g (rhoc_T_oracle's loop plus dt' F)."""
    def operators_at(dtp, x):
        return operators(coords, tris, tags, tag_to_k, tag_to_rc, dtp, x, kappa_tables, rhoc_tables)
    return table_loop(operators_at, dt, bc_dofs, u0, g_all, scheme, picard, F=F)[0]


def rectangle_mesh(nz, nr, L, R):
    """Structured triangulation of [0, L] x [0, R] ((z, r) coordinates): nz x nr cells, two triangles each, diagonals alternating."""
    z = np.linspace(0.0, L, nz + 1)
    r = np.linspace(0.0, R, nr + 1)
    Z, Rr = np.meshgrid(z, r, indexing="ij")
    coords = np.column_stack([Z.ravel(), Rr.ravel()])
    idx = np.arange((nz + 1) * (nr + 1)).reshape(nz + 1, nr + 1)
    tris = []
    for i in range(nz):
        for j in range(nr):
            a, b, c, d = idx[i, j], idx[i + 1, j], idx[i + 1, j + 1], idx[i, j + 1]
            tris += [[a, b, c], [a, c, d]] if (i + j) % 2 == 0 else [[a, b, d], [b, c, d]]
    return coords, np.array(tris, dtype=np.int64)
